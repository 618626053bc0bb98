"""What tests/test_gpu_templates.py::test_nothing_left_behind runs in a process of its own (HYPHY_HIP_POISON is read once):

    python -m tests.template_child CASE

queues the nine steps of CASE (update_q_templates + build_q + evaluate_device, no wait in between), holds them to their references,
then a plain evaluation with dense host matrices, set_q_templates with another K and an evaluation under it, and close().  Also
what the test module runs on the device: a partition for a case, one step of a case, the comparisons (no pytest here)."""
import sys

import numpy as np

from tests import hold
from tests import template_cases as tc

NONE = np.zeros(0, dtype=np.int64)


def mk(cs):
    C = cs["C"] if cs["kind"] in ("cat", "percls") else 1
    from hyphy_amd import hip
    return hip.HipPartition(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def send(part, T, how):
    (part.set_q_templates if how == "set" else part.update_q_templates)(T)


def run_step(part, cs, st, how="update", T=None):
    """One step of a case on the device -> (log-L, per-pattern likelihoods, exponents)."""
    if st["t"] is not None:
        send(part, cs["T"][st["t"]] if T is None else T, how)
    qn, co = tc.coefficients(cs, st)
    pi = cs["pis"][st["pi"]]
    if st["entry"] == "none":
        return part.evaluate(st["update"], NONE, None, pi, per_site=True)
    if st["entry"] == "categories":
        return part.evaluate_categories_built_sites(st["update"], qn, cs["weights"], pi, co)
    if st["entry"] == "mixture":
        return part.evaluate_mixture_built(st["update"], qn, co, cs["mixw"][qn], pi, per_site=True)
    part.build_q(co)
    return part.evaluate_built(st["update"], qn, pi, cat=st["cls"] if cs["kind"] == "percls" else -1, per_site=True)


def hold_step(what, got, ref):
    hold._hold(what, got, ref["site_logl"], ref["logl"])


def hold_total(what, ll, ref):
    allow = hold.RTOL * abs(ref["logl"]) + hold.ATOL
    print(f"{what}: log-L {ll!r} against {ref['logl']!r}: deviation / allowance = {abs(ll - ref['logl']) / allow:.3f}")
    assert abs(ll - ref["logl"]) <= allow, (what, ll, ref["logl"])


def device_value(part, cs, st, d_out, k=0):
    """build_q + evaluate_device of a step into d_out[k] (nothing waits)."""
    import torch  # noqa: F401
    qn, co = tc.coefficients(cs, st)
    part.build_q(co)
    part.evaluate_device(st["update"], qn, part.q_buffer(), cs["pis"][st["pi"]], d_out[k].data_ptr())


def queue_nine(part, cs, d_out):
    """Nine steps of update_q_templates + build_q + evaluate_device into nine device doubles, nothing waited for in between."""
    for i, st in enumerate(cs["steps"]):
        send(part, cs["T"][st["t"]], "set" if i == 0 else "update")
        device_value(part, cs, st, d_out, i)


def main(name):
    import torch  # (before the library: tests/conftest.py)
    from tests import expm_ref as er
    from tests import scalefree as sf
    cs, ref = tc.cases_by_name()[name], tc.reference(name)
    D, B = cs["D"], cs["B"]
    pi = cs["pis"][0]
    nodes = np.arange(B, dtype=np.int64)
    last = cs["steps"][-1]
    d_out = torch.zeros(tc.N_VALUES, dtype=torch.float64, device="cuda")
    part = mk(cs)
    queue_nine(part, cs, d_out)
    part.synchronize()
    got = d_out.cpu().numpy()
    for i in range(tc.N_VALUES):
        hold_total(f"{name} step {i}", float(got[i]), ref[i])
    Q = np.stack([tc.rate_matrix(cs["T"][last["t"]], last["rows"][b]) for b in range(B)])
    hold_step(f"{name} dense host matrices", part.evaluate(nodes, nodes, Q, pi, per_site=True), ref[-1])
    K2 = 3 if cs["K"] != 3 else 2
    T = tc.template_values(D, K2, 900 + D, n=1)[0]
    rows = np.random.default_rng(901 + D).uniform(0.03, 0.5, size=(B, K2))
    P = np.stack([er.reference(tc.rate_matrix(T, r)) for r in rows])
    want = sf.prune(D, cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, pi)
    part.set_q_templates(T)
    part.build_q(rows)
    hold._hold(f"{name} under {K2} templates", part.evaluate_built(nodes, nodes, pi, per_site=True), want["site_logl"], want["logl"])
    part.close()
    torch.cuda.synchronize()
    print("template_child: done")


if __name__ == "__main__":
    main(sys.argv[1])
