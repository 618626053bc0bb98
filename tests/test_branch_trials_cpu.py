"""The recursion behind hyphy_hip_branch_trials, restated in numpy and held to the reference of the branch cache.

``outside`` is the pre-order pass: U_root = pi, for every child c of p  V_c = U_p * prod_{s != c} E_s  (E_s = P_s in_s, the edge product
of sibling s) and U_c = P_c^T V_c; ``trial_site_logl`` is L_s(P_c -> M) = sum_i V_c[i] (M in_c)[i].  No 2^64 scheme: every vector is
divided by its largest element and the logarithm of the divisor is carried beside it, as tests/scalefree.py does for the inside
vectors (which this module takes from it: ``prune(..., conditionals=True)``).

It is held to ``branchcache_cases.reference`` (``scalefree.prune`` with ``P[node] = M``) on every case, every branch in
``cs["branches"]`` and every kind of ``branchcache_cases.trials``, at tests/hold.py's allowance (scalefree.GPU_RTOL x |reference| +
1e-9 per pattern, -inf exactly where the reference has it) — and three mistakes are shown to miss it on every full-coverage case."""
import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests import scalefree as sf
from tests.hold import ATOL, RTOL

CASES = bc.cases_by_name()
D4 = dict(name="bal2x4_D4", shape="bal2x4", D=4, seed=7400)
MISTAKES = ("u_for_v", "sibling_dropped", "m_transposed")


def _norm(v, lg):
    m = v.max(axis=1)
    ok = m > 0
    with np.errstate(divide="ignore"):
        return np.where(ok[:, None], v / np.where(ok, m, 1.0)[:, None], 0.0), lg + np.log(m)


def outside(cs, P=None, mistake=None):
    """Per branch c: (V_c [S, D], its log-magnitude [S], in_c [S, D], its log-magnitude [S]).  ``mistake``: "u_for_v" hands out
    U_c = P_c^T V_c in place of V_c, "sibling_dropped" leaves the first other sibling out of the product."""
    D, L = int(cs["D"]), int(cs["L"])
    fp = np.asarray(cs["flat_parents"], dtype=np.int64)
    codes = np.asarray(cs["leaf_codes"], dtype=np.int64)
    amb = np.asarray(cs["ambig"], dtype=np.float64)
    P = cs["P"] if P is None else P
    pi = np.asarray(cs["root_freqs"], dtype=np.float64)
    S = codes.shape[1]
    sel = np.arange(S)
    base = sf.prune(D, fp, L, codes, amb, cs["pattern_freq"], P, pi, conditionals=True)
    cond, lg = list(base["cond"]), base["log_mag"]
    ch = sf.children_of(fp, L)
    I = len(ch)
    U, lU = [None] * I, [None] * I
    U[I - 1], lU[I - 1] = np.broadcast_to(pi, (S, D)).copy(), np.zeros(S)
    out = {}
    for n in range(I - 1, -1, -1):                       # children are numbered before their parents: this is a pre-order
        E = {c: sf._edge(P[c], c, L, codes, amb, cond, None, sel) for c in ch[n]}
        for c in ch[n]:
            V, lV = U[n].copy(), lU[n].copy()
            others = [s for s in ch[n] if s != c]
            if mistake == "sibling_dropped":
                others = others[1:]
            for s in others:
                V, lV = _norm(V * E[s], lV + (lg[s - L] if s >= L else 0.0))
            Uc, lUc = _norm(V @ P[c], lV)
            if c >= L:
                U[c - L], lU[c - L] = Uc, lUc
                inv, lin = cond[c - L], lg[c - L]
            else:
                k = codes[c]
                inv = np.where((k < 0)[:, None], amb[np.maximum(-k - 1, 0)], np.eye(D)[np.maximum(k, 0)])
                lin = np.zeros(S)
            out[c] = (Uc, lUc, inv, lin) if mistake == "u_for_v" else (V, lV, inv, lin)
    return out


def trial_site_logl(o, node, M, transposed=False):
    V, lV, inv, lin = o[node]
    M = np.asarray(M, dtype=np.float64)
    lik = (V * (inv @ (M if transposed else M.T))).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(lik > 0, np.log(lik) + lV + lin, -np.inf)


def _miss(site, want):
    """Largest per-pattern deviation over hold.py's allowance; inf where -inf sits in the wrong place."""
    if not np.array_equal(np.isneginf(site), np.isneginf(want)):
        return np.inf
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(site[fin] - want[fin]) / (RTOL * np.abs(want[fin]) + ATOL)))


def _worst(cs, mistake=None):
    """Per branch of the case: the largest miss over its six trial matrices."""
    o = outside(cs, mistake=None if mistake == "m_transposed" else mistake)
    out = {}
    for node in cs["branches"]:
        w = 0.0
        for kind, M in bc.trials(cs, node):
            want = bc.reference(cs, node, M, key=kind)["site_logl"]
            w = max(w, _miss(trial_site_logl(o, node, M, transposed=mistake == "m_transposed"), want))
        out[node] = w
    return out


@pytest.mark.parametrize("name", list(CASES) + [D4["name"]])
def test_the_recursion_is_the_reference(name):
    cs = CASES[name] if name in CASES else bc._make(**D4)
    worst = _worst(cs)
    print(f"{name}: largest deviation / allowance over {len(worst)} branches x 6 trials = {max(worst.values()):.3g}")
    assert max(worst.values()) <= 1.0, {n: w for n, w in worst.items() if w > 1.0}


def test_the_four_state_case_has_no_impossible_pattern_at_the_base_point():
    cs = bc._make(**D4)
    assert len(cs["branches"]) == 30
    assert np.all(np.isfinite(bc.reference(cs, key="base")["site_logl"]))


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_cases_tell_mistakes_apart(mistake):
    """Each mistake misses the allowance on at least one branch of every full-coverage case.  Smallest miss (deviation / allowance,
    the worst branch of the case that shows the mistake least; ``inf``: a -inf pattern in the wrong place), measured:
        u_for_v          inf      (every full-coverage case; every branch of every case misses)
        sibling_dropped  5.2e10   (bal4x3_D5; every branch of every case misses)
        m_transposed     1.6e9    (bal2x4_D33; every branch of every case misses)
    Over the patterns that stay finite alone (``_finite_miss``) the smallest misses are 9.0e9 (u_for_v, ladder40_D61), 4.7e10
    (sibling_dropped, bal2x4_D5) and 1.6e9 (m_transposed, bal2x4_D33)."""
    for name in bc.full_coverage_names():
        cs = CASES[name]
        worst = _worst(cs, mistake)
        hit = [n for n, w in worst.items() if w > 1.0]
        fin = _finite_miss(cs, mistake)
        print(f"{name} {mistake}: {len(hit)} of {len(worst)} branches miss; worst {max(worst.values()):.3g}, over finite patterns {fin:.3g}")
        assert hit, (name, mistake)
        assert fin > 1.0, (name, mistake, fin)


def _finite_miss(cs, mistake):
    """The worst branch's miss over the patterns that are finite in both the reference and the mistaken recursion."""
    o = outside(cs, mistake=None if mistake == "m_transposed" else mistake)
    w = 0.0
    for node in cs["branches"]:
        for kind, M in bc.trials(cs, node):
            want = bc.reference(cs, node, M, key=kind)["site_logl"]
            got = trial_site_logl(o, node, M, transposed=mistake == "m_transposed")
            fin = np.isfinite(want) & np.isfinite(got)
            if fin.any():
                w = max(w, float(np.max(np.abs(got[fin] - want[fin]) / (RTOL * np.abs(want[fin]) + ATOL))))
    return w


def test_symbols_are_exported_and_refuse_without_a_partition():
    from hyphy_amd import hip
    lib = hip.load()
    for sym in ("hyphy_hip_branch_trials", "hyphy_hip_branch_trials_built"):
        assert sym in hip.EXPORTS
        assert hasattr(lib, sym)
    one = np.zeros(1, dtype=np.int64)
    out = np.zeros(1)
    q = np.eye(4).reshape(1, 4, 4)
    assert lib.hyphy_hip_branch_trials(None, 1, hip._l(one), hip._d(q), 1, None, hip._d(out), None, None) < 0
    assert lib.hyphy_hip_branch_trials_built(None, 1, hip._l(one), hip._d(out), None, hip._d(out), None, None) < 0
    assert "partition == NULL" in lib.hyphy_hip_last_error().decode()
