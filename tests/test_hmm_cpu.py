"""Hidden-Markov rate classes on the host: the references of tests/hmm_ref.py against enumeration, the plan of the device's
launches, and hip.hmm_host (the device's block algebra run serially over that plan) against the 60-digit forward sum at the bar
hmm_ref.bar, and against the 60-digit Viterbi path wherever that path is decided by a margin of at least 1e-6."""
import math

import numpy as np
import pytest

from hyphy_amd import hip

from tests import hmm_ref

G = 32
BOUNDARIES = [1, 2, G, G + 1, G + 2, G * G + 1, G * G + 2]
MARGIN = 1e-6


def values(rng, C, S, spread=0):
    """Per-class per-pattern likelihoods over 12 decades, exponents 0 .. spread apart between the classes of a pattern."""
    l = 10.0 ** rng.uniform(-12, 0, size=(C, S))
    c = rng.integers(0, 3, size=(1, S)) + (rng.integers(0, spread + 1, size=(C, S)) if spread else 0)
    return l, np.asarray(np.broadcast_to(c, (C, S)), dtype=np.int64).copy()


def check_forward(l, c, T, pi, sites, what):
    N = l.shape[1] if sites is None else len(sites)
    ref = hmm_ref.to_float(hmm_ref.forward_mp(l, c, T, pi, sites))
    got = hip.hmm_host(l, c, T, pi, sites)
    if math.isnan(ref):
        assert math.isnan(got), what
        return got
    if ref == -math.inf:
        assert got == -math.inf, what
        return got
    tol = hmm_ref.bar(N, l.shape[0], ref)
    print(f"{what}: N={N} C={l.shape[0]} logL={ref!r} |err|={abs(got - ref):.3e} bar={tol:.3e}")
    assert abs(got - ref) <= tol, (what, got, ref, abs(got - ref), tol)
    return got


def check_viterbi(l, c, T, pi, sites, what):
    m = hmm_ref.margins(l, c, T, pi, sites)
    assert m >= MARGIN, f"{what}: margin {m:.3e} — change the seed, not the bar"
    ref = hmm_ref.viterbi_mp(l, c, T, pi, sites)
    got = hip.hmm_host(l, c, T, pi, sites, logl=False, path=True)
    assert got.dtype == np.int8 and np.array_equal(got, ref), what


# ---- the references themselves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("N", [1, 2, 3, 6])
def test_references_against_enumeration(C, N):
    rng = np.random.default_rng(100 * C + N)
    S = 4
    l, c = values(rng, C, S, spread=2)
    T, pi = hmm_ref.random_chain(rng, C)
    sites = rng.integers(0, S, size=N)
    total, best_path, best = hmm_ref.brute(l, c, T, pi, sites)
    fw = hmm_ref.forward_mp(l, c, T, pi, sites)
    assert abs(fw - total) <= 1e-50 * max(1, abs(total))
    vp = hmm_ref.viterbi_mp(l, c, T, pi, sites)
    assert abs(hmm_ref.path_score(l, c, T, pi, sites, vp) - best) <= 1e-50 * max(1, abs(best))
    if hmm_ref.margins(l, c, T, pi, sites) > 1e-9:
        assert np.array_equal(vp, best_path)


def test_single_site_is_the_weighted_sum():
    l = np.array([[0.25], [0.5]])
    c = np.array([[1], [1]])
    got = hmm_ref.to_float(hmm_ref.forward_mp(l, c, np.eye(2), [0.4, 0.6]))
    assert abs(got - (math.log(0.4 * 0.25 + 0.6 * 0.5) - 64 * math.log(2))) < 1e-13


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 8])
def test_plan_invariants(C):
    assert hip.plan_hmm(5, C)["G"] == G
    expect_levels = dict(zip(BOUNDARIES, [1, 2, 2, 2, 2, 2, 3]))
    for N in BOUNDARIES + [3, G - 1, 2 * G + 1, 5 * G, G * G, G * G + G + 2]:
        pl = hip.plan_hmm(N, C)
        items = pl["items"]
        assert len(items) == pl["levels"] and items[-1] == 1
        if N in expect_levels:
            assert pl["levels"] == expect_levels[N], N
        if N == 1:
            assert items == [1]
            continue
        assert items[0] % C == 0
        segs = items[0] // C
        # the segments cover the factors 0 .. N-2 exactly once, in order
        covered = []
        for j in range(segs):
            lo, hi = j * G, min((j + 1) * G, N - 1)
            assert lo < hi
            covered.extend(range(lo, hi))
        assert covered == list(range(N - 1))
        n = segs
        for k in range(1, pl["levels"] - 1):  # combine levels: G blocks into one while more than G are left
            assert n > G
            n = -(-n // G)
            assert items[k] == n * C
        assert 1 <= n <= G


def test_plan_refuses():
    for n, C in [(0, 3), (2 ** 31, 3), (10, 1), (10, 9)]:
        with pytest.raises(hip.HipError):
            hip.plan_hmm(n, C)


# ---- hmm_host against the 60-digit forward sum ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_forward_generic_chain_at_every_plan_boundary(C):
    """(a) and (f): an asymmetric chain, a non-stationary start; sites unsorted with repeats."""
    rng = np.random.default_rng(7 + C)
    S = 23
    l, c = values(rng, C, S)
    T, pi = hmm_ref.random_chain(rng, C)
    for N in BOUNDARIES:
        sites = rng.integers(0, S, size=N)
        check_forward(l, c, T, pi, sites, f"a C={C}")


@pytest.mark.parametrize("spread", [3, 40])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_forward_exponents_apart_between_classes(C, spread):
    """(b)"""
    rng = np.random.default_rng(31 * C + spread)
    S = 17
    l, c = values(rng, C, S, spread=spread)
    assert (c.max(axis=0) - c.min(axis=0)).max() >= min(spread, 3)
    T, pi = hmm_ref.random_chain(rng, C)
    for N in (1, 2, G + 2, 3 * G + 5):
        check_forward(l, c, T, pi, rng.integers(0, S, size=N), f"b spread={spread}")


def test_forward_identity_chain_with_dominance_crossing():
    """(c): T = I, class 0 ahead by 2^-5 per site for N/2 sites, then class 1: both per-class products survive."""
    N = 1000
    l = np.array([[2.0 ** -3, 2.0 ** -8], [2.0 ** -8, 2.0 ** -3]])
    c = np.zeros((2, 2), dtype=np.int64)
    sites = np.array([0] * (N // 2) + [1] * (N // 2))
    pi = np.array([0.3, 0.7])
    got = check_forward(l, c, np.eye(2), pi, sites, "c")
    per_class = -(3 + 8) * (N // 2) * math.log(2)  # each class: (2^-3 2^-8)^(N/2)
    assert abs(got - (per_class + math.log(0.3 + 0.7))) <= hmm_ref.bar(N, 2, got)
    # ... and with the classes' products apart: the log-sum-exp of the two per-class sums
    sites = np.array([0] * 520 + [1] * 480)
    got = check_forward(l, c, np.eye(2), pi, sites, "c'")
    a = math.log(0.3) - (3 * 520 + 8 * 480) * math.log(2)
    b = math.log(0.7) - (8 * 520 + 3 * 480) * math.log(2)
    assert abs(got - (max(a, b) + math.log1p(math.exp(-abs(a - b))))) <= hmm_ref.bar(N, 2, got)


def test_forward_identity_chain_rows_of_one_block_far_apart():
    """(c) past the segment level: N = 2400 > G^2 + 1, so a combine level forms blocks of 1024 sites whose two rows lie 2^-5120
    apart, and the crossing is 2^-6000 deep.  A product aligned on max_k b_k instead of the row's own largest term loses one class."""
    N = 2400
    l = np.array([[2.0 ** -3, 2.0 ** -8], [2.0 ** -8, 2.0 ** -3]])
    c = np.zeros((2, 2), dtype=np.int64)
    pi = np.array([0.3, 0.7])
    assert hip.plan_hmm(N, 2)["levels"] == 3
    for first in (N // 2, N // 2 + 9):
        sites = np.array([0] * first + [1] * (N - first))
        got = check_forward(l, c, np.eye(2), pi, sites, "c far")
        a = math.log(0.3) - (3 * first + 8 * (N - first)) * math.log(2)
        b = math.log(0.7) - (8 * first + 3 * (N - first)) * math.log(2)
        assert abs(got - (max(a, b) + math.log1p(math.exp(-abs(a - b))))) <= hmm_ref.bar(N, 2, got)


@pytest.mark.parametrize("T_kind", ["identity", "blocks"])
def test_forward_non_communicating_classes_with_exponents_far_apart(T_kind):
    """Classes whose 2^64 exponents lie 30 apart at every site (2^-1920: nothing a double holds) under a chain that does not let them
    communicate: every class's product survives on its own, whichever class has the smallest exponent at a site."""
    rng = np.random.default_rng(17)
    C, S, N = 3, 7, 3 * G + 2
    l = 10.0 ** rng.uniform(-6, 0, size=(C, S))
    c = np.stack([rng.integers(0, 3, size=S), 30 + rng.integers(0, 3, size=S), 60 + rng.integers(0, 3, size=S)]).astype(np.int64)
    c[:, ::2] = c[::-1, ::2]                          # (the class with the smallest exponent changes from pattern to pattern)
    T = np.eye(C) if T_kind == "identity" else np.array([[0.8, 0.2, 0.0], [0.3, 0.7, 0.0], [0.0, 0.0, 1.0]])
    sites = rng.integers(0, S, size=N)
    for pi in (np.array([0.2, 0.3, 0.5]), np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0])):
        assert math.isfinite(check_forward(l, c, T, pi, sites, f"far apart {T_kind}"))


def test_forward_zero_likelihoods():
    """(d)"""
    rng = np.random.default_rng(5)
    C, S, N = 3, 9, 3 * G + 1
    l, c = values(rng, C, S, spread=2)
    T, pi = hmm_ref.random_chain(rng, C)
    sites = rng.integers(0, S - 1, size=N)  # pattern S-1 is not listed
    sites[N // 2] = 4
    l1 = l.copy()
    l1[1, 4] = 0.0  # impossible under one class: finite
    got = check_forward(l1, c, T, pi, sites, "d one class")
    assert math.isfinite(got)
    l2 = l.copy()
    l2[:, 4] = 0.0  # under every class, at a listed site
    assert check_forward(l2, c, T, pi, sites, "d every class") == -math.inf
    for at in (0, N - 1):  # ... the first and the last site too
        s2 = sites.copy()
        s2[:] = np.where(s2 == 4, 3, s2)
        s2[at] = 4
        assert check_forward(l2, c, T, pi, s2, "d every class, end") == -math.inf
    l3 = l.copy()
    l3[:, S - 1] = 0.0  # at an unlisted pattern: no effect
    assert hip.hmm_host(l3, c, T, pi, sites) == hip.hmm_host(l, c, T, pi, sites)


def test_forward_nan():
    """(e), and NaN in T or pi"""
    rng = np.random.default_rng(6)
    C, S, N = 3, 9, 2 * G + 3
    l, c = values(rng, C, S)
    T, pi = hmm_ref.random_chain(rng, C)
    sites = rng.integers(0, S - 1, size=N)
    for at in (0, N // 2, N - 1):
        ln = l.copy()
        ln[2, sites[at]] = np.nan
        assert math.isnan(check_forward(ln, c, T, pi, sites, "e listed"))
        assert (hip.hmm_host(ln, c, T, pi, sites, logl=False, path=True) == -1).all()
    ln = l.copy()
    ln[:, S - 1] = np.nan
    assert hip.hmm_host(ln, c, T, pi, sites) == hip.hmm_host(l, c, T, pi, sites)
    Tn = T.copy()
    Tn[1, 2] = np.nan
    pn = pi.copy()
    pn[0] = np.nan
    for N1 in (1, N):
        assert math.isnan(hip.hmm_host(l, c, Tn, pi, sites[:N1]))
        assert math.isnan(hip.hmm_host(l, c, T, pn, sites[:N1]))
        assert (hip.hmm_host(l, c, Tn, pi, sites[:N1], logl=False, path=True) == -1).all()


def test_forward_site_list_shapes():
    """(f): a pattern with 300 sites, one with none, the rest unsorted with repeats; and no list at all."""
    rng = np.random.default_rng(8)
    C, S = 3, 12
    l, c = values(rng, C, S, spread=1)
    T, pi = hmm_ref.random_chain(rng, C)
    sites = np.concatenate([np.full(300, 5), rng.integers(0, S - 1, size=77)])
    rng.shuffle(sites)
    assert (sites == 5).sum() >= 300 and not (sites == S - 1).any()
    check_forward(l, c, T, pi, sites, "f")
    check_viterbi(l, c, T, pi, sites, "f")
    check_forward(l, c, T, pi, None, "f no list")
    assert hip.hmm_host(l, c, T, pi, None) == hip.hmm_host(l, c, T, pi, np.arange(S))


# ---- Viterbi ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_viterbi_equals_the_reference_path(C):
    rng = np.random.default_rng(211 + C)
    S = 29
    l, c = values(rng, C, S, spread=2)
    T, pi = hmm_ref.random_chain(rng, C)
    for N in BOUNDARIES:
        check_viterbi(l, c, T, pi, rng.integers(0, S, size=N), f"viterbi C={C} N={N}")


def test_viterbi_with_forbidden_transitions():
    rng = np.random.default_rng(13)
    C, S, N = 3, 11, 2 * G + 7
    l, c = values(rng, C, S)
    T = np.array([[0.7, 0.3, 0.0], [0.0, 0.6, 0.4], [0.5, 0.0, 0.5]])
    pi = np.array([0.0, 0.4, 0.6])
    sites = rng.integers(0, S, size=N)
    check_viterbi(l, c, T, pi, sites, "forbidden")
    check_forward(l, c, T, pi, sites, "forbidden")


def test_viterbi_all_impossible():
    rng = np.random.default_rng(14)
    C, S, N = 3, 7, G + 9
    l, c = values(rng, C, S)
    T, pi = hmm_ref.random_chain(rng, C)
    sites = rng.integers(0, S, size=N)
    l[:, sites[N // 3]] = 0.0
    assert (hmm_ref.viterbi_mp(l, c, T, pi, sites) == -1).all()
    assert (hip.hmm_host(l, c, T, pi, sites, logl=False, path=True) == -1).all()
    assert hip.hmm_host(l, c, T, pi, sites) == -math.inf


def test_host_refusals():
    l = np.full((3, 4), 0.5)
    c = np.zeros((3, 4), dtype=np.int64)
    T, pi = np.full((3, 3), 1 / 3), np.full(3, 1 / 3)
    with pytest.raises(hip.HipError):
        hip.hmm_host(l, c, T, pi, [0, 4])  # pattern out of range
    for bad in (-0.1, np.inf):
        Tb = T.copy()
        Tb[0, 1] = bad
        with pytest.raises(hip.HipError):
            hip.hmm_host(l, c, Tb, pi)
    with pytest.raises(hip.HipUnsupported):
        hip.hmm_host(l[:1], c[:1], np.ones((1, 1)), np.ones(1))
    l9 = np.full((9, 4), 0.5)
    with pytest.raises(hip.HipUnsupported):
        hip.hmm_host(l9, np.zeros((9, 4), dtype=np.int64), np.full((9, 9), 1 / 9), np.full(9, 1 / 9))


# ---- the reference binary's own answers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hmm_nuc_small", "hmm_codon_cat3"])
def test_references_and_host_reproduce_the_goldens(name):
    """tests/golden/hmm_*.npz (tools/make_hmm_golden.py): log L of the unmodified reference binary's LFCompute and the matrix its
    ConstructCategoryMatrix (.., SHORT) hands out (RunViterbi's path read through the duplicate map once more: printed[i] =
    path[site_to_pattern[i]]).  Per-class pattern likelihoods from tests/scalefree.py on oracle.expm matrices; forward_mp and
    hmm_host at 1e-10 relative (the README's parity bar), the path exactly."""
    from oracle import oracle
    from tests import common
    from tests import scalefree as sf
    fx = common.load(name)
    P = np.stack([oracle.expm(common.fixture_Q(fx, float(v)), str(fx["kind"]) == "codon") for v in fx["cat_values"]])
    per = sf.prune(fx["D"], fx["flat_parents"], fx["L"], fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], P, fx["root_freqs"],
                   weights=fx["cat_weights"])
    l = np.exp(per["class_site_logl"])
    c = np.zeros(l.shape, dtype=np.int64)
    sites, T, pi, want = fx["site_to_pattern"], fx["T"], fx["pi"], float(fx["logl"])
    assert abs(hmm_ref.to_float(hmm_ref.forward_mp(l, c, T, pi, sites)) - want) <= 1e-10 * abs(want)
    got, path = hip.hmm_host(l, c, T, pi, sites, logl=True, path=True)
    assert abs(got - want) <= 1e-10 * abs(want), (got, want)
    assert float(fx["min_margin"]) >= MARGIN and hmm_ref.margins(l, c, T, pi, sites) >= MARGIN
    assert np.array_equal(path, fx["path"]) and np.array_equal(hmm_ref.viterbi_mp(l, c, T, pi, sites), fx["path"])
    assert np.array_equal(path[sites], fx["printed"])
    assert abs(T.sum(axis=1) - 1).max() < 1e-15 and abs(pi - fx["cat_weights"]).max() > 0.05
