"""Hidden-Markov rate classes on the device (hyphy_hip_hmm_set_sites / _hmm_logl / _hmm_viterbi and the two fused category entry
points) against tests/hmm_ref.py.

Exact tier: the matrices go in as transition matrices (q_is_probability=True), the per-class per-pattern (l, c) are read back from
the device itself (evaluate(cat=c, per_site=True)), and the forward sum / Viterbi path are compared with the 60-digit references on
THOSE values: log L at hmm_ref.bar, the path exactly wherever it is decided by a margin of at least 1e-6 (asserted here: change the
seed, not the bar).  The other tiers compare bits with bits."""
import ctypes
import math

import numpy as np
import pytest

from tests import hmm_ref
from tests import scalefree as sf
from tests.test_gpu_joint import BAL8, POLY12, make_case

pytestmark = pytest.mark.gpu

G = 32
BOUNDARIES = [1, 2, G, G + 1, G + 2, G * G + 1, G * G + 2]
LEVELS = dict(zip(BOUNDARIES, [1, 2, 2, 2, 2, 2, 3]))
MARGIN = 1e-6
SF = sf.cases_by_name()


def _hip():
    from hyphy_amd import hip
    return hip


def _env(monkeypatch, **env):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _mk(cs, C):
    return _hip().HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def _nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def class_matrices(cs, C, seed):
    """[C, B, D, D]: class 0 is the case's own, the others are drawn like it."""
    from tests.test_gpu_joint import _random_P
    rng = np.random.default_rng(seed)
    B, D = cs["P"].shape[0], int(cs["D"])
    return np.stack([cs["P"]] + [_random_P(rng, B, D) for _ in range(C - 1)])


def evaluate_classes(part, cs, Pc):
    """Every class through hyphy_hip_evaluate; the device's own per-pattern values l [C, S] and exponents c [C, S]."""
    n = _nodes(cs)
    l, c = [], []
    for m in range(Pc.shape[0]):
        _, lm, cm = part.evaluate(n, n, Pc[m], cs["root_freqs"], cat=m, q_is_probability=True, per_site=True)
        l.append(lm)
        c.append(cm)
    return np.array(l), np.array(c, dtype=np.int64)


def form(N):
    segs = -(-(N - 1) // G)
    return f"hmm sites={N} segments={segs} levels={LEVELS.get(N, 2 if segs <= G else 3)}"


def hold(part, l, c, T, pi, sites, what, viterbi=True):
    """set_sites + hmm_logl (+ hmm_viterbi) against the references on (l, c)."""
    part.hmm_set_sites(sites)
    N = l.shape[1] if sites is None else len(sites)
    got = part.hmm_logl(T, pi)
    assert part.reduce_form() == form(N), (what, part.reduce_form())
    ref = hmm_ref.to_float(hmm_ref.forward_mp(l, c, T, pi, sites))
    if math.isnan(ref) or ref == -math.inf:
        assert (math.isnan(got) if math.isnan(ref) else got == ref), (what, got, ref)
    else:
        tol = hmm_ref.bar(N, l.shape[0], ref)
        print(f"{what}: N={N} C={l.shape[0]} logL={ref!r} |err|={abs(got - ref):.3e} bar={tol:.3e}")
        assert abs(got - ref) <= tol, (what, got, ref, abs(got - ref), tol)
    if viterbi:
        m = hmm_ref.margins(l, c, T, pi, sites)
        assert m >= MARGIN, f"{what}: margin {m:.3e} — change the seed, not the bar"
        path = part.hmm_viterbi(T, pi)
        assert path.dtype == np.int8 and np.array_equal(path, hmm_ref.viterbi_mp(l, c, T, pi, sites)), what
        assert part.reduce_form() == form(N)
    return got


# ---- exact tier ---------------------------------------------------------------------------------------------------------------------
GRID = [(D, C, S) for D in (4, 20, 61) for C in (2, 3, 8) for S in (1, 17, 70)]


@pytest.mark.parametrize("D,C,S", GRID)
def test_forward_and_viterbi_at_every_plan_boundary(D, C, S, monkeypatch):
    _env(monkeypatch)
    cs = make_case(D, (BAL8, POLY12)[(D + C) % 2], S, 500 + 10 * D + C + 1000 * S)
    Pc = class_matrices(cs, C, 900 + D + C)
    rng = np.random.default_rng(41 + D + C + 1000 * S)
    T, pi = hmm_ref.random_chain(rng, C)
    seen = set()
    with _mk(cs, C) as part:
        l, c = evaluate_classes(part, cs, Pc)
        assert np.all(l > 0)
        for N in BOUNDARIES:
            hold(part, l, c, T, pi, rng.integers(0, S, size=N), f"D{D} C{C} S{S}")
            seen.add(int(part.reduce_form().split("levels=")[1]))
    assert seen == {1, 2, 3}


@pytest.mark.parametrize("name", ["classes_D4_k3", "classes_D61_k2"])
def test_exponents_apart_between_classes(name, monkeypatch):
    """(b), (c), (f) on rescaling trees with three rate classes far apart (off-diagonals 1e-2, 1e-12, 1e-30)."""
    _env(monkeypatch)
    cs = SF[name]
    S = cs["leaf_codes"].shape[1]
    rng = np.random.default_rng(3)
    T, pi = hmm_ref.random_chain(rng, 3)
    with _mk(cs, 3) as part:
        l, c = evaluate_classes(part, cs, cs["P"])
        assert c.max() > 0 and (c.max(axis=0) - c.min(axis=0)).max() >= 1, c
        for N in (1, G + 2, 3 * G + 5):
            hold(part, l, c, T, pi, rng.integers(0, S, size=N), f"{name} b")
        # (f) a pattern with 300 sites, one with none, the rest unsorted with repeats; then no list at all
        sites = np.concatenate([np.full(300, 5), rng.integers(0, S - 1, size=77)])
        rng.shuffle(sites)
        hold(part, l, c, T, pi, sites, f"{name} f")
        hold(part, l, c, T, pi, None, f"{name} f, no list")
        # (c) classes that do not communicate, sites ordered so that class 0 leads first and class 2 last
        logr = (np.log(l[0]) - 64 * np.log(2) * c[0]) - (np.log(l[2]) - 64 * np.log(2) * c[2])
        sites = rng.integers(0, S, size=1000)
        sites = sites[np.argsort(-logr[sites], kind="stable")]
        hold(part, l, c, np.eye(3), pi, sites, f"{name} c", viterbi=False)


def test_impossible_patterns(monkeypatch):
    """(d): a pattern impossible under one class (finite), under every class at a listed site (-inf, path all -1), unlisted (no effect)."""
    _env(monkeypatch)
    D, C, S = 20, 3, 17
    cs = make_case(D, BAL8, S, 71)
    cs["leaf_codes"][cs["leaf_codes"] == D - 1] = 0      # the isolated state nowhere else
    cs["leaf_codes"][:, 5] = np.arange(cs["L"]) % (D - 1)
    cs["leaf_codes"][0, 5] = D - 1          # the isolated state at one leaf only
    cs["leaf_codes"][:, 6] = cs["leaf_codes"][:, 5]
    Pc = class_matrices(cs, C, 72)
    rng = np.random.default_rng(73)
    T, pi = hmm_ref.random_chain(rng, C)
    one = Pc.copy()
    one[1] = sf._block_zero(one[1], D)
    every = np.stack([sf._block_zero(P, D) for P in Pc])
    listed = np.array([0, 1, 5, 7, 8, 5, 9] * 11)
    unlisted = np.where(listed == 5, 4, listed)
    with _mk(cs, C) as part:
        l, c = evaluate_classes(part, cs, one)
        assert l[1, 5] == 0 and l[0, 5] > 0
        assert math.isfinite(hold(part, l, c, T, pi, listed, "d one class"))
        l, c = evaluate_classes(part, cs, every)
        assert np.all(l[:, 5] == 0) and np.all(l[:, 6] == 0)
        assert hold(part, l, c, T, pi, listed, "d every class", viterbi=False) == -math.inf
        assert (part.hmm_viterbi(T, pi) == -1).all()
        assert math.isfinite(hold(part, l, c, T, pi, unlisted, "d unlisted"))


@pytest.mark.parametrize("D", [4, 20])
def test_nan_in_listed_and_unlisted_patterns(D, monkeypatch):
    """(e): a NaN in one entry of an ambiguity row makes exactly the patterns that carry that code NaN (under every class: the table
    is shared).  Listed — first, inner or last site — it answers NaN and a path of -1; in patterns no site refers to it has no effect."""
    _env(monkeypatch)
    C, S = 2, 17
    cs = make_case(D, BAL8, S, 81)
    cs["ambig"][2, 0] = np.nan                       # code -3
    Pc = class_matrices(cs, C, 82)
    rng = np.random.default_rng(83)
    T, pi = hmm_ref.random_chain(rng, C)
    with _mk(cs, C) as part:
        l, c = evaluate_classes(part, cs, Pc)
        bad = np.flatnonzero(np.isnan(l).any(axis=0))
        good = np.flatnonzero(~np.isnan(l).any(axis=0))
        assert len(bad) > 0 and len(good) > 0 and set(bad) == set(np.flatnonzero((cs["leaf_codes"] == -3).any(axis=0)))
        clean = rng.choice(good, size=2 * G + 3)
        want = hold(part, l, c, T, pi, clean, "e unlisted")
        assert math.isfinite(want)
        for at in (0, G + 1, 2 * G + 2):
            sites = clean.copy()
            sites[at] = bad[0]
            assert math.isnan(hold(part, l, c, T, pi, sites, "e listed", viterbi=False))
            assert (part.hmm_viterbi(T, pi) == -1).all()
        assert math.isnan(hold(part, l, c, T, pi, bad[:1], "e listed, one site", viterbi=False))
        assert (part.hmm_viterbi(T, pi) == -1).all()
        assert hold(part, l, c, T, pi, clean, "e unlisted again") == want


@pytest.mark.parametrize("N", [1, G + 5, G * G + 2])
def test_nan_in_transition_or_initial(N, monkeypatch):
    """Over finite resident values: NaN in `transition` or in `initial` answers NaN from hmm_logl and the fused entry point and a path of
    -1 — also at N = 1, where the transition matrix takes no part in the sum —, and a clean call afterwards is what it was."""
    _env(monkeypatch)
    D, C, S = 20, 3, 17
    cs = make_case(D, BAL8, S, 84)
    Pc = class_matrices(cs, C, 85)
    rng = np.random.default_rng(86)
    T, pi = hmm_ref.random_chain(rng, C)
    n = _nodes(cs)
    with _mk(cs, C) as part:
        l, c = evaluate_classes(part, cs, Pc)
        assert np.all(np.isfinite(l)) and np.all(l > 0)
        sites = rng.integers(0, S, size=N)
        want = hold(part, l, c, T, pi, sites, "clean")
        path = part.hmm_viterbi(T, pi)
        assert math.isfinite(want) and (path >= 0).all()
        Tn, pn = T.copy(), pi.copy()
        Tn[1, 2], pn[C - 1] = np.nan, np.nan
        for Tx, px in ((Tn, pi), (T, pn), (Tn, pn)):
            assert math.isnan(part.hmm_logl(Tx, px))
            assert (part.hmm_viterbi(Tx, px) == -1).all()
            assert math.isnan(part.evaluate_categories_hmm(n, n, Pc, Tx, px, cs["root_freqs"], q_is_probability=True))
            assert part.hmm_logl(T, pi) == want and np.array_equal(part.hmm_viterbi(T, pi), path)


# ---- fused tier ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 61])
def test_fused_entry_point_gives_the_bits_of_the_two_calls(D, monkeypatch):
    _env(monkeypatch)
    C, S = 3, 70
    cs = make_case(D, POLY12, S, 600 + D)
    Pc = class_matrices(cs, C, 601 + D)
    rng = np.random.default_rng(602)
    T, pi = hmm_ref.random_chain(rng, C)
    n = _nodes(cs)
    sites = rng.integers(0, S, size=G * G + 2)
    w = np.array([0.5, 0.3, 0.2])
    with _mk(cs, C) as part:
        part.hmm_set_sites(sites)
        a = part.evaluate_categories_hmm(n, n, Pc, T, pi, cs["root_freqs"], q_is_probability=True)
        assert part.reduce_form() == form(len(sites))
        again = part.evaluate_categories_hmm(n, n, Pc, T, pi, cs["root_freqs"], q_is_probability=True)
        part.evaluate_categories(n, n, Pc, w, cs["root_freqs"], q_is_probability=True)
        b = part.hmm_logl(T, pi)
        assert math.isfinite(a) and a == again and a == b, (a, again, b)
        # a partial update through the fused entry point
        Pn = class_matrices(cs, C, 777)[:, 3:4]
        a = part.evaluate_categories_hmm(n[3:4], n[3:4], Pn, T, pi, cs["root_freqs"], q_is_probability=True)
        part.evaluate_categories(n[3:4], n[3:4], Pn, w, cs["root_freqs"], q_is_probability=True)
        assert a == part.hmm_logl(T, pi) and a != b


@pytest.mark.parametrize("D,K", [(20, 2), (61, 4)])
def test_fused_built_entry_point_gives_the_bits_of_the_two_calls(D, K, monkeypatch):
    from tests import template_cases as tc
    _env(monkeypatch)
    cs = tc.cases_by_name()[f"classes_D{D}_K{K}"]
    st = cs["steps"][0]
    qn, co = tc.coefficients(cs, st)
    rf = cs["pis"][st["pi"]]
    S = cs["leaf_codes"].shape[1]
    rng = np.random.default_rng(610 + D)
    T, pi = hmm_ref.random_chain(rng, 3)
    with _mk(cs, 3) as part:
        part.set_q_templates(cs["T"][st["t"]])
        part.hmm_set_sites(rng.integers(0, S, size=3 * G + 1))
        a = part.evaluate_categories_built_hmm(st["update"], qn, T, pi, rf, co)
        again = part.evaluate_categories_built_hmm(st["update"], qn, T, pi, rf, co)
        part.evaluate_categories_built_sites(st["update"], qn, cs["weights"], rf, co)
        b = part.hmm_logl(T, pi)
        assert math.isfinite(a) and a == again and a == b, (a, again, b)


# ---- residency, state, shards -------------------------------------------------------------------------------------------------------
def test_a_new_transition_matrix_runs_no_tree_work(monkeypatch):
    _env(monkeypatch)
    hip = _hip()
    D, C, S = 61, 3, 33
    cs = make_case(D, BAL8, S, 620)
    Pc = class_matrices(cs, C, 621) - np.eye(D)      # rate matrices: the exponential kernel runs
    rng = np.random.default_rng(622)
    T, pi = hmm_ref.random_chain(rng, C)
    T2, _ = hmm_ref.random_chain(rng, C)
    n = _nodes(cs)
    with _mk(cs, C) as part:
        part.hmm_set_sites(rng.integers(0, S, size=5 * G))
        a = part.evaluate_categories_hmm(n, n, Pc, T, pi, cs["root_freqs"])
        passes, kernel = len(part.prune_timings(1000)), hip.last_expm_kernel()
        b = part.hmm_logl(T2, pi)
        back = part.hmm_logl(T, pi)
        assert len(part.prune_timings(1000)) == passes and hip.last_expm_kernel() == kernel
        assert a == back and a != b


def _sequence(cs, Pc, with_hmm):
    """Category evaluations, a partial update, branch trials and marginal reconstruction — with HMM calls in between or without."""
    rng = np.random.default_rng(631)
    C = Pc.shape[0]
    T, pi = hmm_ref.random_chain(rng, C)
    w = np.full(C, 1.0 / C)
    n = _nodes(cs)
    Pn = class_matrices(cs, C, 632)[:, 2:3]
    trial = np.ascontiguousarray(np.swapaxes(class_matrices(cs, C, 633)[:, [1, 4]], 0, 1))
    out = []

    def hmm(part):
        if with_hmm:
            part.hmm_set_sites(rng.integers(0, cs["leaf_codes"].shape[1], size=G + 5))
            part.hmm_logl(T, pi)
            part.hmm_viterbi(T, pi)

    with _mk(cs, C) as part:
        out.append(part.evaluate_categories(n, n, Pc, w, cs["root_freqs"], q_is_probability=True, per_site=True))
        hmm(part)
        out.append(part.evaluate_categories(n[2:3], n[2:3], Pn, w, cs["root_freqs"], q_is_probability=True, per_site=True))
        hmm(part)
        out.append(part.branch_trials(n[[1, 4]], trial, weights=w, q_is_probability=True, per_site=True))
        hmm(part)
        out.append(part.marginal_ancestral("internal", weights=w))
        hmm(part)
        out.append(part.evaluate_categories(n, n, Pc, w, cs["root_freqs"], q_is_probability=True, per_site=True))
    return out


@pytest.mark.parametrize("D", [4, 61])
def test_hmm_calls_leave_no_state_behind(D, monkeypatch):
    _env(monkeypatch)
    cs = make_case(D, POLY12, 33, 630 + D)
    Pc = class_matrices(cs, 3, 634 + D)
    plain, mixed = _sequence(cs, Pc, False), _sequence(cs, Pc, True)
    for k, (x, y) in enumerate(zip(plain, mixed)):
        for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
            assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True), k


def test_three_shards_give_the_bits_of_one(monkeypatch):
    D, C, S = 20, 3, 70
    cs = make_case(D, POLY12, S, 640)
    Pc = class_matrices(cs, C, 641)
    rng = np.random.default_rng(642)
    T, pi = hmm_ref.random_chain(rng, C)
    sites = rng.integers(0, S, size=G * G + 2)
    n = _nodes(cs)
    got = []
    for shards in (None, "3"):
        _env(monkeypatch, **({"HYPHY_HIP_FORCE_SHARDS": shards} if shards else {}))
        with _mk(cs, C) as part:
            part.hmm_set_sites(sites)
            a = part.evaluate_categories_hmm(n, n, Pc, T, pi, cs["root_freqs"], q_is_probability=True)
            got.append((a, part.hmm_logl(T, pi), part.hmm_viterbi(T, pi), part.reduce_form()))
    assert got[0][0] == got[0][1] == got[1][0] == got[1][1] and math.isfinite(got[0][0])
    assert np.array_equal(got[0][2], got[1][2]) and (got[0][2] >= 0).all()
    assert got[0][3] == got[1][3] == form(len(sites))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    _env(monkeypatch)
    hip = _hip()
    lib = hip.load()
    D, S = 4, 17
    cs = make_case(D, BAL8, S, 650)
    n = _nodes(cs)
    T, pi = hmm_ref.random_chain(np.random.default_rng(651), 3)

    def refused(kind, call):
        with pytest.raises(kind) as e:
            call()
        assert len(str(e.value)) > 10, str(e.value)
        if kind is hip.HipError:
            assert not isinstance(e.value, hip.HipUnsupported)

    for C in (1, 9):  # "use the CPU path"
        Tc, pc = np.full((C, C), 1.0 / C), np.full(C, 1.0 / C)
        with _mk(cs, C) as part:
            part.hmm_set_sites(None)
            for m in range(C):
                part.evaluate(n, n, cs["P"], cs["root_freqs"], cat=m, q_is_probability=True)
            refused(hip.HipUnsupported, lambda: part.hmm_logl(Tc, pc))
            refused(hip.HipUnsupported, lambda: part.hmm_viterbi(Tc, pc))
            Pc = np.stack([cs["P"]] * C)
            refused(hip.HipUnsupported, lambda: part.evaluate_categories_hmm(n, n, Pc, Tc, pc, cs["root_freqs"], q_is_probability=True))
    Pc = class_matrices(cs, 3, 652)
    with _mk(cs, 3) as part:
        refused(hip.HipError, lambda: part.hmm_set_sites([0, S]))
        refused(hip.HipError, lambda: part.hmm_set_sites([-1]))
        refused(hip.HipError, lambda: part.hmm_set_sites(np.zeros(0, dtype=np.int64)))
        evaluate_classes(part, cs, Pc[:2])
        refused(hip.HipError, lambda: part.hmm_logl(T, pi))                      # no site list
        refused(hip.HipError, lambda: part.evaluate_categories_hmm(n, n, Pc, T, pi, cs["root_freqs"], q_is_probability=True))
        part.hmm_set_sites(None)
        refused(hip.HipError, lambda: part.hmm_logl(T, pi))                      # class 2 never evaluated
        refused(hip.HipError, lambda: part.hmm_viterbi(T, pi))
        evaluate_classes(part, cs, Pc)
        want = part.hmm_logl(T, pi)
        for bad in (-1e-3, np.inf):
            Tb, pb = T.copy(), pi.copy()
            Tb[2, 0], pb[1] = bad, bad
            refused(hip.HipError, lambda: part.hmm_logl(Tb, pi))
            refused(hip.HipError, lambda: part.hmm_viterbi(T, pb))
            refused(hip.HipError, lambda: part.evaluate_categories_hmm(n, n, Pc, Tb, pi, cs["root_freqs"], q_is_probability=True))
        out = ctypes.c_double(0.0)
        for args in ((None, hip._d(pi), ctypes.byref(out)), (hip._d(T), None, ctypes.byref(out)), (hip._d(T), hip._d(pi), None)):
            assert lib.hyphy_hip_hmm_logl(part._h, *args) < 0 and len(lib.hyphy_hip_last_error()) > 10
        assert lib.hyphy_hip_hmm_viterbi(part._h, hip._d(T), hip._d(pi), None) < 0 and len(lib.hyphy_hip_last_error()) > 10
        assert lib.hyphy_hip_hmm_logl(None, hip._d(T), hip._d(pi), ctypes.byref(out)) < 0 and len(lib.hyphy_hip_last_error()) > 10
        part.set_pinned_states(int(cs["L"]), np.zeros(S, dtype=np.int64))        # an active pin
        refused(hip.HipError, lambda: part.hmm_logl(T, pi))
        refused(hip.HipError, lambda: part.hmm_viterbi(T, pi))
        refused(hip.HipError, lambda: part.evaluate_categories_hmm(n, n, Pc, T, pi, cs["root_freqs"], q_is_probability=True))
        part.set_pinned_states()
        assert part.hmm_logl(T, pi) == want                                      # ... and nothing was disturbed


# ---- golden -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hmm_nuc_small", "hmm_codon_cat3"])
def test_goldens_of_the_reference_binary(name, monkeypatch):
    """tests/golden/hmm_*.npz: log L of the unmodified reference's LFCompute at 1e-10 relative (the README's parity bar), RunViterbi's
    path exactly, and — read through the duplicate map once more, as the reference's RemapMatrix does — the matrix it prints."""
    from tests import common
    _env(monkeypatch)
    fx = common.load(name)
    Q = np.stack([common.fixture_Q(fx, float(v)) for v in fx["cat_values"]])
    n = common.all_nodes(fx)
    want = float(fx["logl"])
    with _hip().HipPartition(int(fx["D"]), fx["flat_parents"], int(fx["L"]), fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], 3) as part:
        part.hmm_set_sites(fx["site_to_pattern"])
        got = part.evaluate_categories_hmm(n, n, Q, fx["T"], fx["pi"], fx["root_freqs"])
        print(f"{name}: log L {got!r} against {want!r}: relative deviation {abs(got - want) / abs(want):.2e}")
        assert abs(got - want) <= 1e-10 * abs(want), (got, want)
        assert part.hmm_logl(fx["T"], fx["pi"]) == got
        path = part.hmm_viterbi(fx["T"], fx["pi"])
        assert float(fx["min_margin"]) >= MARGIN
        assert np.array_equal(path, fx["path"])
        assert np.array_equal(path[fx["site_to_pattern"]], fx["printed"])
