"""The reference of hyphy_hip_branch_derivatives (tests/deriv_cases.py) pinned to finite differences of the branch cache's reference,
shown to tell the likely mistakes apart, and driving hyphy_amd.brlen's Newton iteration without a device."""
import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests import deriv_cases as dc
from tests import expm_ref
from tests import scalefree as sf

CASES = bc.cases_by_name()
FD_CASES = [f"{shape}_D5" for shape in bc.FULL_SHAPES] + ["bal2x4_D4"]


def _case(name):
    return CASES[name] if name in CASES else dc.d4_case()


H = 1e-3
ROUND = 256 * float(np.finfo(np.longdouble).eps)
FLOOR1 = 5 / 3 * 2 * ROUND / H
FLOOR2 = 5 / 3 * 4 * ROUND / (H / 2) ** 2


def _expm_taylor(A):
    """exp(A) for |A|_inf <= 1e-3 in longdouble: the Taylor series to degree 10 (the remainder is below 1e-36)."""
    A = np.asarray(A).astype(np.longdouble)
    out, term = np.eye(len(A), dtype=np.longdouble), np.eye(len(A), dtype=np.longdouble)
    for k in range(1, 11):
        term = term @ A / k
        out = out + term
    return out


@pytest.mark.parametrize("name", FD_CASES)
def test_the_reference_is_pinned_to_finite_differences(name):
    """r1, r2 against Richardson-extrapolated central differences of log l_s(theta) with P[node] = exp(theta G) P[node], theta =
    +-1e-3, +-5e-4, at 1e-6 A (A1 for r1, A2 + 2 |r1| A1 for r2).  With |G|_inf <= 1 the truncation after extrapolation is O(h^4).
    The rounding of the second difference is (rounding of log l_s) / h^2, and log l_s is of size 10 .. 100, not 1: taken from
    branchcache_cases.reference in float64 that is 4e-8 absolute (measured: up to 2.5e-7), above 1e-6 A wherever A < 0.05 — so
    l_s(theta) is the inside pass of deriv_cases in longdouble (``site_logl``, which shares nothing with the outside pass and the
    generator products under test) with the exponential as a longdouble Taylor series (tests/expm_ref.py's serves non-negative
    off-diagonals only: no theta < 0, no -0.25 I), 1e-11 absolute; at theta = 0 it is held to branchcache_cases.reference.
    The quotients are taken of u(theta) = l_s(theta) / l_s(0) itself, r1 = u'(0) and r2 = u''(0) - u'(0)^2: u is entire with k-th
    derivative below A1, while the k-th derivative of log u grows like r1^k and r1 reaches 1e3 on the nearly impossible patterns.
    What is left of the rounding is absolute, not a share of A: each u carries at most ROUND = 256 longdouble eps (the inside
    pass is fewer than 256 roundings deep on these trees), a central first difference at h / 2 then 2 ROUND / h, a second one
    4 ROUND / (h / 2)^2, times 5 / 3 for the extrapolation's weights: FLOOR1 = 9e-14 and FLOOR2 = 7.4e-10 are added to the bar (the
    sparse generators leave A2 as small as 2e-7 where they do not connect the states the pattern has at the branch's two ends;
    measured rounding there: 1e-11).
    The row-scaled generators are not differenced: their A goes down to 1e-20, below any difference quotient's rounding at this h;
    what they add to the sparse ones (rows of very different size in one product) is a matter of the device's arithmetic."""
    cs = _case(name)
    outs = dc.outs_of(cs)
    h = H
    worst = 0.0
    base = bc.reference(cs)["site_logl"]                     # (uncached: the cache goes by name, and bal2x4_D4 has a namesake)
    mine = dc.site_logl(cs, cs["P"]).astype(np.float64)
    assert np.array_equal(np.isneginf(mine), np.isneginf(base))
    assert np.allclose(mine[np.isfinite(base)], base[np.isfinite(base)], rtol=1e-13, atol=0)
    for node in cs["branches"]:
        for kind, G in dc.generators(cs, node):
            ref = dc.values(cs, outs, node, [G])
            fin = ~np.isnan(ref["r1"])
            assert np.array_equal(fin, np.isfinite(base))
            if kind == "zero":
                assert np.all(ref["r1"][fin] == 0) and np.all(ref["r2"][fin] == 0)
                continue
            if kind == "row_scaled":
                continue
            ll = {}
            for th in (-h, -h / 2, 0.0, h / 2, h):
                P = np.asarray(cs["P"]).astype(np.longdouble)
                P[node] = _expm_taylor(th * G) @ P[node]
                ll[th] = dc.site_logl(cs, P)
            with np.errstate(invalid="ignore"):              # u(theta) = l_s(theta) / l_s(0): r1 = u'(0), r2 = u''(0) - u'(0)^2
                u = {th: np.exp(ll[th] - ll[0.0]) for th in ll}
                d1 = lambda s: (u[s] - u[-s]) / (2 * s)
                d2 = lambda s: (u[s] - 2 + u[-s]) / (s * s)
                fd1 = (4 * d1(h / 2) - d1(h)) / 3
                fd2 = (4 * d2(h / 2) - d2(h)) / 3 - fd1 * fd1
            a1 = ref["A1"][fin]
            a2 = (ref["A2"] + 2 * np.abs(ref["r1"]) * ref["A1"])[fin]
            e1, e2 = np.abs(fd1[fin] - ref["r1"][fin]), np.abs(fd2[fin] - ref["r2"][fin])
            if kind == "quarter_identity":
                assert np.allclose(ref["r1"][fin].astype(np.float64), -0.25, rtol=1e-15, atol=0)
                assert np.all(np.abs(ref["r2"][fin]) <= 1e-17)
            worst = max(worst, float(np.max(e1 / (1e-6 * a1 + FLOOR1))), float(np.max(e2 / (1e-6 * a2 + FLOOR2))))
    print(f"{name}: largest |finite difference - reference| / (1e-6 A) = {worst:.3g}")
    assert worst <= 1.0


def test_the_float64_recursion_lies_within_the_allowance():
    """What the allowance leaves to the device: the same recursion in float64 against the longdouble one."""
    worst = 0.0
    for name in ("bal2x4_D5", "bal2x4_D61", "ladder40_D33", "conflict_D20_1em30"):
        cs = CASES[name]
        o64 = [dc.outside(cs, ft=np.float64)]
        for node in cs["branches"]:
            for kind, G in dc.generators(cs, node):
                ref, got = dc.values(cs, dc.outs_of(cs), node, [G]), dc.values(cs, o64, node, [G])
                assert ref["n_skipped"] == got["n_skipped"] == (len(range(5, len(cs["pattern_freq"]), 16)) if cs["seed"] % 2 else 0)
                worst = max(worst, dc.miss(got["r1"], got["r2"], got["d1"], got["d2"], ref))
    print(f"float64 against longdouble: largest deviation / allowance = {worst:.3g}")
    assert worst <= 0.05


@pytest.mark.parametrize("mistake", dc.MISTAKES)
def test_the_cases_see_the_mistakes(mistake):
    """Each mistake misses by more than 1000 allowances on every branch of every full-coverage case (mixing without aligning the
    exponents: of the rate-class cases)."""
    smallest = np.inf
    cases = bc.class_cases() if mistake == "unaligned" else [CASES[n] for n in bc.full_coverage_names()]
    for cs in cases:
        C = 1 if np.asarray(cs["P"]).ndim == 3 else len(cs["P"])
        good = dc.outs_of(cs)
        outs = good
        if mistake == "u_for_v":
            outs = [dc.outside(cs, mistake=mistake)]
        for node in cs["branches"]:
            w = 0.0
            for k in range(2):                           # the sparse generator and its row-scaled form
                Gs = [dc.generators(cs, node, c)[k][1] for c in range(C)]
                ref = dc.values(cs, good, node, Gs, cs.get("weights"))
                bad = dc.values(cs, outs, node, Gs, cs.get("weights"), mistake=mistake)
                w = max(w, dc.miss(bad["r1"], bad["r2"], bad["d1"], bad["d2"], ref))
            smallest = min(smallest, w)
            assert w > 1000.0, (cs["name"], node, mistake, w)
    print(f"{mistake}: smallest miss over all branches = {smallest:.3g} allowances")


def test_newton_on_the_numpy_reference():
    """brlen.fit_branch_lengths driven by the reference: 6 taxa, 5 states, patterns drawn from the model; from t = 0.1 everywhere it
    stops within max_iter with log L monotone, and no single branch at 0.99 or 1.01 of its length raises the reference log L."""
    from hyphy_amd import brlen
    cs = dc.fit_case("fit6_D5", dc.FIT_TREE_6, 5, 300, 7501)
    B = len(cs["flat_parents"]) - 1

    def evaluate(t):
        return dc.fit_logl(cs, t)

    def derivatives(t):
        return dc.fit_derivatives(cs, t)

    t, ll, it, hist = brlen.fit_branch_lengths(evaluate, derivatives, np.full(B, 0.1))
    print(f"fit6_D5: {it} iterations, log L {hist[0]:.6f} -> {ll:.6f}")
    assert it < 50 and len(hist) == it + 1 and hist[-1] == ll
    assert all(b >= a for a, b in zip(hist, hist[1:]))
    assert ll > hist[0]
    for b in range(B):
        for fac in (0.99, 1.01):
            t2 = t.copy()
            t2[b] *= fac
            assert evaluate(t2) <= ll, (b, fac)


def test_the_binding():
    from hyphy_amd import hip
    lib = hip.load()
    for sym in ("hyphy_hip_branch_derivatives", "hyphy_hip_branch_derivatives_built"):
        assert sym in hip.EXPORTS
        assert len(getattr(lib, sym).argtypes) == 10
    one = np.zeros(1, dtype=np.int64)
    out = np.zeros(1)
    g = np.zeros((1, 4, 4))
    assert lib.hyphy_hip_branch_derivatives(None, 1, hip._l(one), hip._d(g), None, hip._d(out), hip._d(out), None, None, None) < 0
    assert "partition == NULL" in lib.hyphy_hip_last_error().decode()
    assert lib.hyphy_hip_branch_derivatives_built(None, 1, hip._l(one), hip._d(out), None, hip._d(out), hip._d(out), None, None, None) < 0

    class Shape(hip.HipPartition):                       # the argument checks run before the library is called
        C, D, S, _h, _lib = 2, 5, 3, None, None

        def __init__(self):
            pass

        def __del__(self):
            pass
    fake = Shape()
    with pytest.raises(ValueError):
        hip.HipPartition.branch_derivatives(fake, [0, 1], np.zeros((2, 5, 5)), weights=np.array([0.5, 0.5]))
    with pytest.raises(ValueError):
        hip.HipPartition.branch_derivatives(fake, [0], np.zeros((1, 2, 5, 4)), weights=np.array([0.5, 0.5]))
    with pytest.raises(ValueError):
        hip.HipPartition.branch_derivatives(fake, [0], np.zeros((1, 2, 5, 5)), weights=np.ones(3) / 3)
    with pytest.raises(ValueError):
        hip.HipPartition.branch_derivatives_built(fake, [0, 1], np.zeros((1, 2, 3)), weights=np.array([0.5, 0.5]))
