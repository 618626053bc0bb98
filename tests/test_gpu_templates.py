"""The template path on the device across template UPDATES: hyphy_hip_set_q_templates / _update_q_templates / _build_q and every
evaluation that consumes what they stage, held to the references of tests/template_cases.py (expm_ref.reference + scalefree.prune
replayed over each case's sequence of steps) at the allowance of tests/hold.py, per pattern and in total — the only number here.

1 every consumer sees an update; 2 partial rebuilds keep the matrices of the old templates; 3 passes over resident matrices do not
re-derive them; 4 the caller's diagonals are ignored, bit for bit; 5 the staging ring and the early-out; 6 the host ahead of the
device; 7 nothing left behind (in a process of its own: tests/template_child.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import expm_child as ec
from tests import expm_ref as er
from tests import hold
from tests import scalefree as sf
from tests import template_cases as tc
from tests.template_child import NONE, device_value, hold_step, hold_total, mk, queue_nine, run_step, send  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY = tc.cases_by_name()


def _hip():
    from hyphy_amd import hip
    return hip


@pytest.fixture(scope="module")
def cus():
    return ec.cu_count()


def _env(monkeypatch, **env):
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _exact(monkeypatch, **env):
    _env(monkeypatch, HYPHY_HIP_TUNE="0", HYPHY_HIP_CUT="levels", **env)


def hold_site_logs(what, got, ref):
    """Per-pattern log-likelihoods (the site fits return those) at the same allowance."""
    want = ref["site_logl"]
    assert got.shape == want.shape and np.all(np.isfinite(got)), (what, got)
    worst = float(np.max(np.abs(got - want) / (hold.RTOL * np.abs(want) + hold.ATOL)))
    print(f"{what}: largest per-pattern deviation / allowance = {worst:.3f}")
    assert worst <= 1.0, (what, worst)


def expected_kernels(D, n, cus, images=True):
    """4 states: a launch of its own, or "" where the library folds the exponentials into the pruning launch (small shards of the
    plain view; not the materialised form, which has no coefficients to take along) — the tests that force either form say which."""
    return ("expm_nuc_kernel", "") if D == 4 else (er.kernel_for(D, n, cus, images=images),)


def four_state_form(monkeypatch, fold):
    """The settings under which, by the library's own rules, a 4-state partition of five or eight leaves and 40 patterns folds the
    exponentials (fold = "1") or launches expm_nuc_kernel (fold = "0"): the interpreter, no class compression (as
    tests/test_gpu_expm.py::test_four_state_images_under_interpreter_and_generated_kernel sets them)."""
    for k, v in (("HYPHY_HIP_NUCGEN", "0"), ("HYPHY_HIP_REPEATS", "0"), ("HYPHY_HIP_NUC_FOLD", fold)):
        monkeypatch.setenv(k, v)
    return "" if fold == "1" else "expm_nuc_kernel"


def trial_rows(cs, n=3):
    rng = np.random.default_rng(77 + cs["D"] + cs["K"])
    nodes = np.array([1, cs["L"] + 2, 5][:n], dtype=np.int64)
    return nodes, rng.uniform(0.03, 0.5, size=(n, cs["K"]))


def trial_reference(cs, ref, t, node, row):
    P = np.array(ref["P"][0])
    P[node] = er.reference(tc.rate_matrix(cs["T"][t], row))
    r = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, cs["pis"][0])
    return r


def site_fit_args(cs, st):
    qn, co = tc.coefficients(cs, st)
    S = cs["leaf_codes"].shape[1]
    return np.zeros(cs["B"], dtype=np.int64), co, np.ones((S, 1, cs["K"])), cs["pis"][st["pi"]]


def site_fits(part, cs, st):
    """(site_fits_evaluate, site_fits_evaluate_mixture with two equal components of weight 0.3 and 0.7) or "unsupported"."""
    hip = _hip()
    bg, bc, sm, pi = site_fit_args(cs, st)
    S = cs["leaf_codes"].shape[1]
    try:
        one = part.site_fits_evaluate(bg, bc, sm, pi)
        two = part.site_fits_evaluate_mixture(bg, bc, np.ones((S, 2, 1, cs["K"])), np.tile(np.array([0.3, 0.7]), (S, 1)), pi)
    except hip.HipUnsupported:
        return "unsupported"
    return one, two


# ---- 1. every consumer sees an update --------------------------------------------------------------------------------------------------

CONSUMER_NAMES = [f"consumer_D{D}_K{K}" for D, K in tc.CONSUMER_GRID]
PLAIN_CONSUMERS = ("built", "built_sites+trials+site_fits", "device", "materialize")


@pytest.mark.parametrize("consumer", PLAIN_CONSUMERS)
@pytest.mark.parametrize("name", CONSUMER_NAMES)
def test_every_consumer_sees_an_update(name, consumer, monkeypatch, cus):
    """set_q_templates(T0), a full pass, update_q_templates(T1), build_q, then the consumer: evaluate_built, evaluate_built_sites
    (followed by branch_trials_built and the site fits, which read the templates themselves), evaluate_device + fetch_device_scalar,
    and the materialised form (HYPHY_HIP_MATERIALIZE_Q=1).  The site fits take 5 states and up and at most four templates: they
    are refused at 4 states and at K = 5, and run at every other cell (49 states: the K = 2 case)."""
    _env(monkeypatch)
    _consumer(name, consumer, monkeypatch, expected_kernels(BY[name]["D"], BY[name]["B"], cus))


@pytest.mark.parametrize("fold", ("1", "0"), ids=("folded", "own launch"))
@pytest.mark.parametrize("consumer", ("built", "built_sites+trials+site_fits", "device"))
def test_four_state_consumers_in_either_form(consumer, fold, monkeypatch):
    """The 4-state case with the exponentials folded into the pruning launch (no exponential kernel is named) and in a launch of
    their own (expm_nuc_kernel reads the staged coefficients): the form is asserted, not accepted either way."""
    _env(monkeypatch)
    _consumer("consumer_D4_K2", consumer, monkeypatch, (four_state_form(monkeypatch, fold),))


def _consumer(name, consumer, monkeypatch, kernels):
    import torch
    hip = _hip()
    cs, ref = BY[name], tc.reference(name)
    s0, s1 = cs["steps"]
    D, K, B = cs["D"], cs["K"], cs["B"]
    with mk(cs) as part:
        hold_step(f"{name} under T0", run_step(part, cs, s0, "set"), ref[0])
        part.update_q_templates(cs["T"][1])
        qn, co = tc.coefficients(cs, s1)
        if D == 4:
            hip.expm_batch(np.zeros((1, D, D)))           # (so that an empty kernel name afterwards is the consumer's)
        if consumer == "built":
            step = part.prepare_built_step(s1["update"], qn, cs["pis"][0], co)
            hold_total(f"{name} evaluate_built", step(), ref[1])
            assert hip.last_expm_kernel() in kernels, hip.last_expm_kernel()
        elif consumer == "built_sites+trials+site_fits":
            part.build_q(co)
            hold_step(f"{name} evaluate_built_sites", part.evaluate_built(s1["update"], qn, cs["pis"][0], per_site=True), ref[1])
            assert hip.last_expm_kernel() in kernels, hip.last_expm_kernel()
            nodes, rows = trial_rows(cs)
            ll, lik, sc = part.branch_trials_built(nodes, rows, per_site=True)
            for k, (b, row) in enumerate(zip(nodes, rows)):
                want = trial_reference(cs, ref[1], 1, int(b), row)
                hold._hold(f"{name} trial on branch {b}", (float(ll[k]), lik[k], sc[k]), want["site_logl"], want["logl"])
            fits = site_fits(part, cs, s1)
            if D == 4 or K > 4:
                assert fits == "unsupported", (name, fits)
            else:
                hold_site_logs(f"{name} site_fits_evaluate", fits[0], ref[1])
                hold_site_logs(f"{name} site_fits_evaluate_mixture", fits[1], ref[1])
            hold_step(f"{name} afterwards", part.evaluate(s1["update"], NONE, None, cs["pis"][0], per_site=True), ref[1])
        else:
            if consumer == "materialize":
                monkeypatch.setenv("HYPHY_HIP_MATERIALIZE_Q", "1")
            d_out = torch.zeros(2, dtype=torch.float64, device="cuda")
            device_value(part, cs, s1, d_out)
            got = part.prepare_fetch(d_out.data_ptr())()
            hold_total(f"{name} evaluate_device ({consumer})", got, ref[1])
            assert hip.last_expm_kernel() in kernels, hip.last_expm_kernel()
            part.synchronize()
            assert float(d_out[0].item()) == got


@pytest.mark.parametrize("per_site", (False, True), ids=("total", "sites"))
@pytest.mark.parametrize("D,K", tc.CLASS_GRID)
def test_rate_classes_see_an_update(D, K, per_site, monkeypatch, cus):
    """evaluate_categories_built and _built_sites with three classes (class-major coefficient rows); the entry point exists from 5
    states up (at 4 states the library refuses it)."""
    hip = _hip()
    _env(monkeypatch)
    name = f"classes_D{D}_K{K}"
    cs, ref = BY[name], tc.reference(name)
    s0, s1 = cs["steps"]
    with mk(cs) as part:
        hold_step(f"{name} under T0", run_step(part, cs, s0, "set"), ref[0])
        if per_site:
            hold_step(f"{name} under T1", run_step(part, cs, s1), ref[1])
        else:
            part.update_q_templates(cs["T"][1])
            qn, co = tc.coefficients(cs, s1)
            hold_total(f"{name} under T1", part.prepare_built_categories_step(s1["update"], qn, cs["weights"], cs["pis"][0], co)(), ref[1])
        assert hip.last_expm_kernel() in expected_kernels(D, 3 * cs["B"], cus), hip.last_expm_kernel()


@pytest.mark.parametrize("D,K", tc.MIXTURE_GRID)
def test_mixture_sees_an_update(D, K, monkeypatch, cus):
    """evaluate_mixture_built with three components per branch."""
    hip = _hip()
    _env(monkeypatch)
    name = f"mixture_D{D}_K{K}"
    cs, ref = BY[name], tc.reference(name)
    with mk(cs) as part:
        hold_step(f"{name} under T0", run_step(part, cs, cs["steps"][0], "set"), ref[0])
        hold_step(f"{name} under T1", run_step(part, cs, cs["steps"][1]), ref[1])
        assert hip.last_expm_kernel() in expected_kernels(D, 3 * cs["B"], cus, images=False), hip.last_expm_kernel()


# ---- 2. partial rebuilds keep old matrices ----------------------------------------------------------------------------------------------

def _play(name, part, after=None):
    cs, ref = BY[name], tc.reference(name)
    for i, st in enumerate(cs["steps"]):
        hold_step(f"{name} step {i} ({len(st['rows'])} branches rebuilt)", run_step(part, cs, st, "set" if i == 0 else "update"), ref[i])
        if after:
            after(i)


@pytest.mark.parametrize("D", tc.PARTIAL_STATES)
def test_partial_rebuilds_keep_old_matrices(D, monkeypatch):
    """T0 everywhere; T1 and two branches; T2 and one other branch; everything under T2: a branch that is not rebuilt keeps the matrix
    of the templates it was built from."""
    _env(monkeypatch)
    with mk(BY[f"partial_D{D}_K2"]) as part:
        _play(f"partial_D{D}_K2", part)


def test_partial_rebuilds_on_a_rerooted_schedule(monkeypatch):
    """The same on the long ladder, re-rooted (the transposed twins of the rebuilt branches must follow), with pi changed in the
    middle; of the rebuilt branches L + 20 and 2 L - 3 lie between the given root and the new one, leaf 0 does not."""
    hip = _hip()
    _env(monkeypatch, HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2")
    cs = BY["partial_reroot_D61_K2"]
    L = cs["L"]
    on_path = {L + int(i) for i in hip.plan_reroot(cs["flat_parents"], L)[1:]}
    assert L + L // 2 in on_path and 2 * L - 3 in on_path and 0 not in on_path, sorted(on_path)
    rerooted = []
    with mk(cs) as part:
        _play(cs["name"], part, lambda i: rerooted.append(i) if "re-rooted" in part.schedule_info() else None)
    print(f"re-rooted schedule in use after steps {rerooted}")
    first_partial = next(i for i, st in enumerate(cs["steps"]) if 0 < len(st["rows"]) < cs["B"])
    assert any(i > first_partial for i in rerooted), rerooted          # (a re-rooted pass read the twins of rebuilt branches)


def test_partial_rebuilds_on_three_shards(monkeypatch):
    _env(monkeypatch, HYPHY_HIP_FORCE_SHARDS="3")
    with mk(BY["partial_shards_D20_K4"]) as part:
        _play("partial_shards_D20_K4", part)


@pytest.mark.parametrize("D", (20, 61))
def test_one_template_set_per_class(D, monkeypatch):
    """Two classes: class 0 under T0, update, class 1 under T1, update back, one branch of class 0 under T0."""
    _env(monkeypatch)
    with mk(BY[f"perclass_D{D}_K2"]) as part:
        _play(f"perclass_D{D}_K2", part)


# ---- 3. resident matrices are not re-derived --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", tc.RESIDENT_STATES)
def test_resident_matrices_are_not_rederived(D, monkeypatch):
    """Two full passes (the second lazy), update_q_templates(T1) WITHOUT build_q: download_partials, an evaluation without matrices,
    marginal_ancestral and the branch cache (above 4 states) all see the matrices of T0.  Conditionals and posteriors at the bars those
    entry points already carry (tests/test_gpu_parity.py, tests/test_gpu_marginal.py); likelihoods at the allowance of hold."""
    _env(monkeypatch)
    name = f"resident_D{D}_K2"
    cs, ref = BY[name], tc.reference(name)
    pi = cs["pis"][0]
    full = sf.prune(D, cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], ref[0]["P"][0], pi,
                    conditionals=True, posteriors=True)
    nodes = np.arange(cs["B"], dtype=np.int64)
    with mk(cs) as part:
        _play(name, part)
        part.update_q_templates(cs["T"][1])
        cache, _ = part.download_partials()
        for n in range(part.I):
            got = cache[n] / cache[n].max(axis=1, keepdims=True)
            assert np.allclose(got, full["cond"][n], rtol=1e-9, atol=1e-300), (name, n)
        hold_step(f"{name} evaluation without matrices", part.evaluate(nodes, NONE, None, pi, per_site=True), ref[0])
        sup = part.marginal_ancestral("internal")
        assert np.allclose(sup, full["post"], rtol=1e-9, atol=1e-12), name
        if D > 4:
            for node in (2, cs["L"] + 3):
                part.branch_cache_build(node)
                got = part.branch_cache_evaluate(node, ref[0]["P"][0][node], q_is_probability=True, per_site=True)
                hold_step(f"{name} branch cache at branch {node}", got, ref[0])
        hold_step(f"{name} afterwards", part.evaluate(nodes, NONE, None, pi, per_site=True), ref[0])


# ---- 4. diagonals are ignored, everywhere -------------------------------------------------------------------------------------------------

def _all_outputs(cs, kind, how, monkeypatch):
    """Every consumer's output under templates whose diagonal is of ``kind``: T0 by set_q_templates, T1 by ``how``."""
    import torch
    out = []
    T0, T1 = tc.set_diagonal(cs["T"][0], kind), tc.set_diagonal(cs["T"][1], kind)
    s0, s1 = cs["steps"]
    with mk(cs) as part:
        out += list(run_step(part, cs, s0, "set", T0))
        out += list(run_step(part, cs, s1, how, T1))
        if cs["kind"] == "plain":
            qn, co = tc.coefficients(cs, s1)
            out.append(np.array(part.prepare_built_step(s1["update"], qn, cs["pis"][0], co)()))
            d_out = torch.zeros(2, dtype=torch.float64, device="cuda")
            device_value(part, cs, s1, d_out, 0)
            monkeypatch.setenv("HYPHY_HIP_MATERIALIZE_Q", "1")
            device_value(part, cs, s1, d_out, 1)
            monkeypatch.delenv("HYPHY_HIP_MATERIALIZE_Q")
            part.synchronize()
            out.append(d_out.cpu().numpy())
            part.build_q(co)
            out += list(part.evaluate_built(s1["update"], qn, cs["pis"][0], per_site=True))
            nodes, rows = trial_rows(cs)
            out += list(part.branch_trials_built(nodes, rows, per_site=True))
            fits = site_fits(part, cs, s1)
            out += [np.zeros(0)] if fits == "unsupported" else list(fits)
        elif cs["kind"] == "cat":
            qn, co = tc.coefficients(cs, s1)
            out.append(np.array(part.prepare_built_categories_step(s1["update"], qn, cs["weights"], cs["pis"][0], co)()))
    return [np.asarray(x) for x in out]


@pytest.mark.parametrize("how", ("set", "update"))
@pytest.mark.parametrize("name", ("consumer_D4_K2", "consumer_D20_K4", "consumer_D49_K5", "consumer_D49_K2", "consumer_D64_K2",
                                  "classes_D20_K2", "classes_D49_K2", "classes_D64_K5",
                                  "mixture_D4_K4", "mixture_D20_K2", "mixture_D49_K2", "mixture_D64_K5"))
def test_diagonals_are_ignored(name, how, monkeypatch):
    """The same off-diagonals with diagonal 0, minus the row sum and +7: bit-identical through every consumer."""
    _exact(monkeypatch)
    cs = BY[name]
    base = _all_outputs(cs, "zero", how, monkeypatch)
    for kind in ("rowsum", "seven"):
        got = _all_outputs(cs, kind, how, monkeypatch)
        assert len(got) == len(base)
        for k, (x, y) in enumerate(zip(base, got)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (name, how, kind, k, float(np.max(np.abs(x - y))) if x.size else 0.0)
    ref = tc.reference(name)[1]
    hold._hold(f"{name} diagonal zero, step 1", (float(base[3]), base[4], base[5]), ref["site_logl"], ref["logl"])


# ---- 5. ring and early-out ----------------------------------------------------------------------------------------------------------------

def _bits(res):
    return (res[0], res[1].tobytes(), res[2].tobytes())


@pytest.mark.parametrize("name", ("consumer_D20_K2", "consumer_D61_K2", "consumer_D4_K2"))
def test_ring_and_early_out(name, monkeypatch):
    """update_q_templates with identical values; three updates in a row (the ring of two wraps, the last wins); update as the very
    first template call; K changed through update (2 -> 3 -> 2): each bit-identical to a fresh partition given set_q_templates of the
    final values and the same coefficients.  An evaluation straight after a K change without build_q is refused, and the partition
    evaluates correctly afterwards."""
    hip = _hip()
    _exact(monkeypatch)
    cs, ref = BY[name], tc.reference(name)
    D, B = cs["D"], cs["B"]
    s0, s1 = cs["steps"]
    pi = cs["pis"][0]
    final = cs["T"][3]
    qn, co = tc.coefficients(cs, s1)
    T3 = tc.template_values(D, 3, 31 + D, n=1)[0]
    co3 = np.random.default_rng(D).uniform(0.03, 0.5, size=(B, 3))

    def evaluate(part, c=co):
        part.build_q(c)
        return part.evaluate_built(s1["update"], qn, pi, per_site=True)

    with mk(cs) as part:
        part.set_q_templates(final)
        want = _bits(evaluate(part))
    with mk(cs) as part:
        part.set_q_templates(T3)
        want3 = _bits(evaluate(part, co3))
    assert want != want3
    with mk(cs) as part:                                   # identical values
        hold_step(f"{name} under T0", run_step(part, cs, s0, "set"), ref[0])
        part.update_q_templates(final)
        assert _bits(evaluate(part)) == want
        part.update_q_templates(final.copy())
        assert _bits(evaluate(part)) == want, "after an update with identical values"
    with mk(cs) as part:                                   # three in a row
        hold_step(f"{name} under T0", run_step(part, cs, s0, "set"), ref[0])
        for v in (1, 2, 3):
            part.update_q_templates(cs["T"][v])
        assert _bits(evaluate(part)) == want, "after three updates in a row"
    with mk(cs) as part:                                   # the very first template call
        part.update_q_templates(final)
        assert _bits(evaluate(part)) == want, "update as the first template call"
    with mk(cs) as part:                                   # K changed through update
        hold_step(f"{name} under T0", run_step(part, cs, s0, "set"), ref[0])
        part.update_q_templates(T3)
        assert _bits(evaluate(part, co3)) == want3, "K = 2 -> 3"
        part.update_q_templates(final)
        with pytest.raises(hip.HipError, match="staged a different number"):
            part.evaluate_built(s1["update"], qn, pi, per_site=True)
        assert _bits(evaluate(part)) == want, "K = 3 -> 2"


# ---- 6. the host ahead of the device ------------------------------------------------------------------------------------------------------

AHEAD_RUNS = [(a[0], None) for a in tc.AHEAD if a[1] == "plain" and a[2] != 4] + [("ahead_fold_D4_K2", "1"), ("ahead_fold_D4_K2", "0")]


@pytest.mark.parametrize("name,fold", AHEAD_RUNS, ids=[n + {None: "", "1": "-folded", "0": "-own launch"}[f] for n, f in AHEAD_RUNS])
def test_the_host_ahead_of_the_device(name, fold, monkeypatch):
    """Queued without any synchronisation, then one synchronize(): all nine values held to their references.  Coefficients inline
    (8 leaves, 61 states, K = 2), beyond the inline limit where the kernel reads the ring slot when it executes (70-leaf ladder,
    K = 3, 20 and 49 states), and at 4 states in the folded form (asserted: no exponential kernel is named) and with expm_nuc_kernel
    in a launch of its own, which reads the ring slot behind the same guard.  A mismatch is diagnosed from the code, not by running again."""
    import torch
    _env(monkeypatch)
    cs, ref = BY[name], tc.reference(name)
    if "ring" in name:
        assert cs["B"] * cs["K"] > 400
    d_out = torch.zeros(tc.N_VALUES, dtype=torch.float64, device="cuda")
    hip = _hip()
    want = None if fold is None else four_state_form(monkeypatch, fold)
    with mk(cs) as part:
        hip.expm_batch(np.zeros((1, cs["D"], cs["D"])))
        queue_nine(part, cs, d_out)
        kernel = hip.last_expm_kernel()
        part.synchronize()
        got = d_out.cpu().numpy()
    assert want is None or kernel == want, (name, fold, kernel)
    for i in range(tc.N_VALUES):
        hold_total(f"{name} step {i}", float(got[i]), ref[i])


def test_mixture_steps_back_to_back(monkeypatch):
    """Nine steps of update_q_templates + build_q + evaluate_mixture_built.  The library has only a synchronous form of this entry
    point, so every step waits for its result: the host is never ahead here, the rings turn nine times."""
    _env(monkeypatch)
    name = "ahead_mix_D20_K2"
    with mk(BY[name]) as part:
        _play(name, part)


# ---- 7. nothing left behind ----------------------------------------------------------------------------------------------------------------

def test_nothing_left_behind():
    """After the nine queued steps: a plain evaluation with dense host matrices, set_q_templates with another K, and close(), under
    HYPHY_HIP_POISON=1 in a process of its own (tests/template_child.py), which checks and reports."""
    env = dict(os.environ, HYPHY_HIP_POISON="1")
    r = subprocess.run([sys.executable, "-m", "tests.template_child", "ahead_inline_D61_K2"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-12:])
    print(tail)
    assert r.returncode == 0 and "template_child: done" in r.stdout, tail
