"""What tests/test_gpu_expm.py runs on the device: the batches of tests/expm_ref.py through hip.expm_batch, and the probe partitions
that read a transition matrix entry by entry through the images the pruning kernels read.  Also a runner:

    python -m tests.expm_child JOB OUT.npz

runs JOB ("forced": the 49-64-state batches and the 61- and 64-state probes; "timed": test_gpu_fullsize._timed_path) in a process
of its own, under whatever HYPHY_HIP_* switches its environment carries — launch_expm and its callers read theirs once per
process — and writes the results and hip.last_expm_kernel() to OUT.npz.

Probe.  On a ladder tree every branch but b carries the zero rate matrix (the identity, exactly); the leaves below b show state a,
all others state c.  The likelihood of that pattern is pi_c P_b[c, a] with exponent 0: one pattern per (a, c) reads the whole matrix
of branch b through the image that kind of branch uses — the column-gather image for a resolved leaf, the A-operand image for an
internal branch or a leaf whose codes are ambiguity rows (here: the indicator of the single state a).
"""
import os
import sys

import numpy as np

from tests import expm_ref as er


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------

def run_batches(D, cus):
    """[(kernel named by the library, case names, P)] of every hip.expm_batch call the state count asks for."""
    from hyphy_amd import hip
    by = er.cases_by_name()
    names = [c["name"] for c in er.cases_at(D)]
    calls = [names] if D < 49 else [b for _, b in er.batches(names, cus)]
    out = []
    for batch in calls:
        P = hip.expm_batch(np.stack([by[n]["Q"] for n in batch]))
        out.append((hip.last_expm_kernel(), list(batch), P))
    return out


def check_batch(kernel, names, P, fixed_degree=False):
    """Every entry within the allowance of the reference, rows summing to 1, nothing below minus the allowance, everything finite,
    the zero matrix the identity exactly.  Returns the largest deviation as a fraction of the allowance."""
    by = er.cases_by_name()
    worst = 0.0
    assert np.all(np.isfinite(P)), kernel
    for k, name in enumerate(names):
        ref = er.case_reference(name)
        allow = er.allowance(name, kernel, fixed_degree)
        dev = float(np.abs(P[k] - ref).max())
        worst = max(worst, dev / allow)
        assert dev <= allow, (kernel, name, k, dev, allow)
        assert np.abs(P[k].sum(axis=1) - 1.0).max() <= er.ROW_SUM_TOL, (kernel, name, k)
        assert P[k].min() >= -allow, (kernel, name, k, float(P[k].min()))
        if by[name]["family"] == "zero":
            assert np.array_equal(P[k], np.eye(P.shape[1])), (kernel, name, k)
    return worst


# ---- probes -----------------------------------------------------------------------------------------------------------------------------

def ladder(L):
    """flat_parents of the ladder over L leaves: internal 0 = (leaf 0, leaf 1), internal i = (internal i - 1, leaf i + 1), the root last."""
    fp = np.empty(2 * L - 1, dtype=np.int64)
    fp[0] = fp[1] = 0
    fp[2:L] = np.arange(1, L - 1)
    fp[L:2 * L - 2] = np.arange(1, L - 1)
    fp[2 * L - 2] = -1
    return fp


def leaves_below(L, b):
    return [b] if b < L else list(range(b - L + 2))


def path_above(fp, L, b):
    """Node codes to list for an update of branch b: b and every node between it and the root."""
    out = [b]
    while fp[out[-1]] != len(fp) - L - 1:
        out.append(L + int(fp[out[-1]]))
    return np.array(sorted(out), dtype=np.int64)


def split_templates(Q, K):
    """K templates with disjoint supports and power-of-two coefficients c whose combination sum_k c_k T_k is Q off the diagonal,
    bit for bit: entry (i, j) sits in template (i + j) mod K."""
    D = Q.shape[0]
    c = 2.0 ** ((np.arange(K) % 5) - 2.0)
    i, j = np.indices((D, D))
    T = np.stack([np.where(((i + j) % K == k) & (i != j), Q / c[k], 0.0) for k in range(K)])
    return T, c


class Probe:
    """A partition over a ladder of L leaves with one group of patterns per probed branch (module docstring).  ``ambig_leaves``:
    leaves whose codes are ambiguity rows (the indicator of the state).  ``pairs``: the (a, c) to read, default all D^2."""

    def __init__(self, D, L, branches, ambig_leaves=(), pairs=None, C=1, seed=1):
        from hyphy_amd import hip
        rng = np.random.default_rng(8200 + 97 * D + seed)
        self.D, self.L, self.B, self.C = D, L, 2 * L - 2, C
        self.fp = ladder(L)
        self.branches = list(branches)
        if pairs is None:
            a, c = np.divmod(np.arange(D * D), D)
        else:
            a, c = np.asarray(pairs, dtype=np.int64).T
        self.a, self.c, n = a, c, len(a)
        codes = np.empty((L, n * len(self.branches)), dtype=np.int64)
        for g, b in enumerate(self.branches):
            codes[:, g * n:(g + 1) * n] = c[None, :]
            codes[leaves_below(L, b), g * n:(g + 1) * n] = a[None, :]
        for leaf in ambig_leaves:
            codes[leaf] = -(codes[leaf] + 1)
        pi = rng.random(D) + 0.25
        self.pi = pi / pi.sum()
        self.nodes = np.arange(self.B, dtype=np.int64)
        self.part = hip.HipPartition(D, self.fp, L, codes, np.eye(D) if len(ambig_leaves) else None, np.ones(codes.shape[1], dtype=np.int64), C)

    def close(self):
        self.part.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def read(self, result, g):
        """lik / pi_c of group g's patterns, the 2^64 exponents undone: the entries P[c, a]."""
        _, lik, sc = result
        n = len(self.a)
        return np.ldexp(lik[g * n:(g + 1) * n], (-64 * sc[g * n:(g + 1) * n]).astype(np.int64)) / self.pi[self.c]

    def expected(self, P):
        return P[self.c, self.a]

    def all_zero_but(self, b, Q, n_class=1):
        Qs = np.zeros((n_class * self.B, self.D, self.D))
        Qs[b] = Q
        return Qs

    def plain(self, g, Q):
        return self.read(self.part.evaluate(self.nodes, self.nodes, self.all_zero_but(self.branches[g], Q), self.pi, per_site=True), g)

    def partial(self, g, Q):
        """Branch g's matrix alone replaced, after an evaluation of every branch."""
        b = self.branches[g]
        return self.read(self.part.evaluate(path_above(self.fp, self.L, b), [b], Q[None], self.pi, per_site=True), g)

    def built(self, g, Q, K):
        T, c = split_templates(Q, K)
        self.part.set_q_templates(T)
        coeffs = np.zeros((self.B, K))
        coeffs[self.branches[g]] = c
        self.part.build_q(coeffs)
        return self.read(self.part.evaluate_built(self.nodes, self.nodes, self.pi, per_site=True), g)


def check_probe(got, ref, allow, what):
    """|lik / pi_c - reference| within the allowance plus four ulps of the value.  Returns the largest deviation / allowance."""
    assert np.all(np.isfinite(got)), what
    dev = np.abs(got - ref)
    bound = allow + 4.0 * np.spacing(np.abs(ref))
    k = int(np.argmax(dev - bound))
    assert dev[k] <= bound[k], (what, k, float(got[k]), float(ref[k]), float(dev[k]), allow)
    return float((dev / bound).max())


PROBE_CASES = ("nonrev_D{D}_n0p2", "nonrev_D{D}_n3")      # not reversible (a transposed image shows), without and with squarings


def forced_probes(D):
    """The probes a forced-variant child runs at D = 61 / 64 states: a resolved leaf, an ambiguous leaf and an internal branch of a
    five-leaf ladder, through plain evaluate and the built path (K = 2).  {label: (kernel, values)}."""
    from hyphy_amd import hip
    by = er.cases_by_name()
    out = {}
    for kind, branches, amb in (("leaf", (3,), ()), ("ambig", (3,), (3,)), ("internal", (5 + 1,), ())):
        with Probe(D, 5, branches, amb) as pr:
            for tmpl in PROBE_CASES:
                name = tmpl.format(D=D)
                vals = pr.plain(0, by[name]["Q"])
                out[f"plain|{kind}|{name}"] = (hip.last_expm_kernel(), vals)
                vals = pr.built(0, by[name]["Q"], 2)
                out[f"built|{kind}|{name}"] = (hip.last_expm_kernel(), vals)
    return out


def rejects(Q):
    """(hip.expm_batch raised HipError with the reference's message, the kernel that ran) for a batch that holds Q."""
    from hyphy_amd import hip
    try:
        hip.expm_batch(Q)
    except hip.HipError as e:
        return "valid transition matrix" in str(e), hip.last_expm_kernel()
    return False, hip.last_expm_kernel()


# ---- runner -----------------------------------------------------------------------------------------------------------------------------

SWITCHES = ("HYPHY_HIP_EXPM", "HYPHY_HIP_EXPM_DEGREE", "HYPHY_HIP_COEF_INLINE", "HYPHY_HIP_EXPM_MASK")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(job, out, env, timeout):
    """One fresh process for one setting; returns its exit status and the end of its output.  Nothing is retried."""
    import subprocess
    full = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    full.update(env, HYPHY_HIP_POISON="1")
    r = subprocess.run([sys.executable, "-m", "tests.expm_child", job, str(out)], env=full, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    return r.returncode, "\n".join((r.stdout + r.stderr).strip().splitlines()[-8:])


def by_name_good(D):
    return er.cases_by_name()[f"nonrev_D{D}_n3"]["Q"]


class _Env:
    setenv = staticmethod(os.environ.__setitem__)


def main(job, out):
    import torch  # noqa: F401  (before the library: tests/conftest.py)
    from hyphy_amd import hip
    res = {}
    if job == "forced":
        cus = cu_count()
        res["cus"] = np.int64(cus)
        j = 0
        for D in (49, 61, 63, 64):
            for kernel, names, P in run_batches(D, cus):
                res[f"batch{j}_kernel"], res[f"batch{j}_names"], res[f"batch{j}_P"] = np.str_(kernel), np.array(names), P
                j += 1
        res["n_batches"] = np.int64(j)
        labels = []
        for D in (61, 64):
            for label, (kernel, vals) in forced_probes(D).items():
                labels.append(f"{D}|{label}")
                res[f"probe{len(labels) - 1}_kernel"], res[f"probe{len(labels) - 1}_values"] = np.str_(kernel), vals
        res["probe_labels"] = np.array(labels)
        # the failure path under this setting: 5 I alone (four workgroups per matrix by default), and in a batch large enough for two and one
        for tag, n in (("few", 1), ("more", cus // 4 + 1), ("many", cus // 2 + 1)):
            Q = np.stack([by_name_good(61)] * (n - 1) + [5.0 * np.eye(61)])
            ok, kernel = rejects(Q)
            res[f"reject_{tag}"], res[f"reject_{tag}_kernel"], res[f"reject_{tag}_n"] = np.bool_(ok), np.str_(kernel), np.int64(n)
    elif job == "timed":
        from tests import common
        from tests import test_gpu_fullsize as tf
        fx = common.load("full_mg94_64x10k_sweep")
        pts = [1, 2, 3, 11, 40]
        got, info, kernel = tf._timed_path(fx, {}, _Env, pts)
        res.update(points=np.array(pts), values=np.array([got[k] for k in pts]), info=np.str_(info), kernel=np.str_(kernel),
                   expm_kernel=np.str_(hip.last_expm_kernel()))
    else:
        raise SystemExit(f"unknown job {job}")
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
