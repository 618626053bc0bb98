"""tests/sitefit_ref.py checked on the CPU: ``transition`` against mpmath at 50 digits, ``site_fit_logl`` against the oracle route of
tests/test_gpu_parity.py and against the ordinary evaluation, the conditions the case list must meet, and that the short-branch
cases are ones a model of the absolute stopping rule loses."""
import numpy as np
import pytest

from tests import scalefree as sf
from tests import sitefit_ref as sr

CASES = sr.cases()
NAMES = [c["name"] for c in CASES]
_refs = {}
_stores = {}      # per case: the reference's exponentials by coefficient vector, shared by the tests that need them again


def _ref(cs):
    if cs["name"] not in _refs:
        _refs[cs["name"]] = sr.case_reference(cs, cache=_stores.setdefault(cs["name"], {}))
    return _refs[cs["name"]]


# ---- transition against mpmath ----------------------------------------------------------------------------------------------------

def _small_templates():
    rng = np.random.default_rng(5)
    out = {}
    for D in (4, 5, 8):
        out[f"chain{D}"] = sr.chain_templates(rng, D)[0]
    blk = np.zeros((8, 8))
    blk[:5, :5] = sr.chain_templates(rng, 5)[0]
    blk[5:7, 5:7] = sr.chain_templates(rng, 2)[0]          # a second block; state 7 is isolated
    out["block8"] = blk
    dense = rng.uniform(0.1, 2.0, (5, 5))
    np.fill_diagonal(dense, 0.0)
    out["dense5"] = dense
    return out


def _mp_expm(Q):
    """Taylor series of exp(Q / 2^s) at 50 digits, squared s times (mpmath matrices)."""
    import mpmath as mp
    D = Q.shape[0]
    A = mp.matrix(D, D)
    for i in range(D):
        for j in range(D):
            A[i, j] = mp.mpf(float(Q[i, j]))
    s = max(0, int(np.ceil(np.log2(max(float(np.abs(Q).max()) * D, 1e-300)))) + 1)
    A = A / mp.mpf(2) ** s
    E = mp.eye(D)
    term = mp.eye(D)
    for j in range(1, 80):
        term = term * A / j
        E = E + term
    for _ in range(s):
        E = E * E
    return E


@pytest.mark.parametrize("rate", [1e-13, 1e-10, 1e-7, 1e-4, 1e-2, 0.7, 1.0, 13.0, 200.0])
@pytest.mark.parametrize("name", sorted(_small_templates()))
def test_transition_matches_mpmath_entry_by_entry(name, rate):
    """Every entry relatively, within the bound the helper states for its float64 arithmetic; zeros exact and only where the
    graph has no path.  The longdouble variant is held to the same bound with its own rounding unit where that is smaller."""
    import mpmath as mp
    mp.mp.dps = 50
    T = _small_templates()[name]
    Q = sr.build_Q(T[None], [rate])
    # (50 digits carry the alternating-sign series of exp(Q) itself here: |Q| D / 2^s < 1 and entries down to rate^7 / 7!)
    want = _mp_expm(Q)
    D = Q.shape[0]
    reach = np.linalg.matrix_power((T > 0) + np.eye(D), D) > 0
    mu = float(-Q.diagonal().min())
    for extended in (False, True):
        got = sr.transition(Q, extended=extended)
        bound = sr.transition_bound(D, mu)
        worst = 0.0
        for i in range(D):
            for j in range(D):
                if not reach[i, j]:
                    assert got[i, j] == 0.0, (name, rate, i, j)
                    continue
                assert got[i, j] > 0.0, (name, rate, i, j)
                worst = max(worst, float(abs(mp.mpf(float(got[i, j])) - want[i, j]) / want[i, j]))
        print(f"{name} rate {rate:g} extended={extended}: worst relative error {worst:.2e} (bound {bound:.2e})")
        assert worst <= bound, (name, rate, extended, worst)


@pytest.mark.parametrize("rate", [1e-4, 1e-2])
def test_transition_on_the_20_state_chain_matches_mpmath(rate):
    """Nineteen steps from end to end: entries down to rate^19 / 19!, each within the stated bound."""
    import mpmath as mp
    mp.mp.dps = 50
    T = sr.chain_templates(np.random.default_rng(6), 20)
    Q = sr.build_Q(T, [rate])
    want = _mp_expm(Q)
    got = sr.transition(Q)
    worst = max(float(abs(mp.mpf(float(got[i, j])) - want[i, j]) / want[i, j]) for i in range(20) for j in range(20))
    print(f"chain20 rate {rate:g}: worst relative error {worst:.2e}; corner entry {got[0, 19]:.3e}")
    assert got[0, 19] < 1e-40 and worst <= sr.transition_bound(20, float(-Q.diagonal().min()))


def test_transition_at_codon_size_float64_against_longdouble():
    """D = 61 and 64 (MG94, three steps across): the float64 default against the extended evaluation, every entry, within the
    stated bound."""
    T, _ = sr.mg94_templates()
    for t in (1e-13, 1e-9, 1e-6, 1e-3, 0.3, 40.0):
        Q = sr.build_Q(T, [t, 0.5 * t])
        a, b = sr.transition(Q), sr.transition(Q, extended=True)
        assert (a > 0).all() and (b > 0).all()          # the codon graph is connected
        worst = float(np.max(np.abs(a - b) / b))
        assert worst <= sr.transition_bound(61, float(-Q.diagonal().min())), (t, worst)
    A, C = sr.codon("AAA"), sr.codon("CCC")
    P = sr.transition(sr.build_Q(T, [1e-10, 0.5e-10]))
    assert 1e-34 < P[A, C] < 1e-31                      # three substitutions at ~1e-10 each, over 3!


# ---- site_fit_logl ----------------------------------------------------------------------------------------------------------------

_worst = {}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_route_agrees_where_it_is_finite(name):
    """The route of test_gpu_parity.py::test_site_fits_* (oracle.expm + one OraclePartition per site) on every case, patterns where
    it is finite.  Prints the deviation: the largest over the list is sitefit_ref.ORACLE_MAX_REL."""
    cs = CASES[NAMES.index(name)]
    want = _ref(cs)
    got = sr.oracle_site_fit_reference(cs["D"], sr.case_flat(cs), cs["codes"], cs["ambig"], cs["pi"], cs["T"], cs["bgroup"], cs["bcoef"],
                                       cs["smult"], cs["smix"])
    assert got.shape == want.shape
    fin = np.isfinite(got)
    assert np.isfinite(want[fin]).all(), name            # finite in the oracle route: finite here
    assert not np.isnan(got).any(), name
    rel = float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))) if fin.any() else 0.0
    _worst[name] = rel
    lost = int((np.isfinite(want) & ~fin).sum())
    print(f"{name}: oracle route against sitefit_ref, largest deviation {rel:.3e} relative (largest so far {max(_worst.values()):.3e}); "
          f"{lost} of {want.size} values finite in the reference and not in the oracle route")
    bound = sr.ORACLE_MAX_REL if sr.oracle_deep(name) else sr.ORACLE_MAX_REL_SHALLOW
    assert rel <= bound, (name, rel, "sitefit_ref.ORACLE_MAX_REL / _SHALLOW is out of date")


def test_unit_multipliers_equal_the_ordinary_evaluation():
    """All multipliers 1: every site sees the same matrices — scalefree.prune fed oracle.expm matrices, all patterns at once."""
    from oracle import oracle
    cs = sr.cases_by_name()["dense_ordinary"]
    S = cs["codes"].shape[1]
    G, K = cs["smult"].shape[-2:]
    got = sr.site_fit_logl(cs["D"], cs["flat_parents"], cs["L"], cs["codes"], cs["ambig"], cs["pi"], cs["T"], cs["bgroup"], cs["bcoef"],
                           np.ones((1, S, G, K)))[0]
    Q = np.stack([sr.build_Q(cs["T"], x) for x in cs["bcoef"]])
    want = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["codes"], cs["ambig"], np.ones(S), oracle.expm(Q, True), cs["pi"])["site_logl"]
    fin = np.isfinite(want)
    assert fin.mean() > 0.9 and np.array_equal(np.isfinite(got), fin)
    assert np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])) < 1e-12


# ---- the list ---------------------------------------------------------------------------------------------------------------------

def test_case_list_meets_its_conditions():
    assert len(set(NAMES)) == len(NAMES)
    assert {c["D"] for c in CASES} >= {5, 16, 17, 20, 32, 33, 48, 49, 61, 64}
    assert {c["T"].shape[0] for c in CASES} == {1, 2, 3, 4}
    assert {c["smult"].shape[-2] for c in CASES} >= {1, 16}
    assert {c["smult"].shape[2] for c in CASES if c["smix"] is not None} == {2, 3, 8}
    assert any((c["smix"] == 0).any() for c in CASES if c["smix"] is not None)
    assert all(n in NAMES for n in sr.NEIGHBOURS)
    assert [sr.cases_by_name()[f"rate_{r}"]["n_sub"] for r in (60, 64, 65, 640, 4095)] == [1, 1, 2, 10, 64]
    for cs in CASES:
        rates = sr.case_rates(cs)
        assert rates.max() <= sr.MAX_RATE, cs["name"]
        if "n_sub" in cs:
            assert int(np.ceil(rates.max() / sr.K_MU_STEP)) == cs["n_sub"], cs["name"]
        off = cs["T"].copy()
        assert off.min() >= 0.0
    assert sr.template_reach(sr.mg94_templates()[0]) == 3 and sr.subset_reach(sr.mg94_templates()[0]) == 5
    off = [c for c in CASES if c["smix"] is None and c["T"].shape[0] > 1 and (c["smult"][0, :, :, 0] == 0).all()]
    assert {c["name"] for c in off} >= {"mg94_alpha0", "dense_off_chain20"}
    assert sr.template_reach(sr.chain_templates(np.random.default_rng(0), 20, K=2)) == 19


@pytest.mark.parametrize("name", NAMES)
def test_every_case_is_finite_where_it_should_be(name):
    """At least 90 % of the patterns finite in the reference, unless the case is named an impossible-pattern case; and a float64
    model of the 2^64 scheme (every node tested, up to 15 steps: scalefree.model_logl) fed the reference's matrices is finite
    wherever the reference is and agrees with it to 1e-12 — the cases lie inside what the scheme's range sustains, so a -inf from
    the kernel is the kernel's."""
    cs = CASES[NAMES.index(name)]
    ref = _ref(cs)
    assert not np.isnan(ref).any() and not np.isposinf(ref).any()
    share = float(np.isfinite(ref).mean())
    assert share >= 0.9 or (cs["impossible"] and "impossible" in name), (name, share)
    if cs["impossible"]:
        assert np.isneginf(ref).any() and share >= 0.5
        iso = (cs["codes"] == cs["D"] - 1) | (cs["codes"] == -1)
        assert np.isfinite(ref[:, iso.all(axis=0)]).all() and iso.all(axis=0).any()
    got = sr.case_reference(cs, cache=_stores[name], scheme=True)          # every set, every component, every case
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)), (name, np.argwhere(np.isfinite(got) != np.isfinite(ref))[:8].tolist())
    fin = np.isfinite(ref)
    assert np.all(np.abs(got[fin] - ref[fin]) <= 1e-12 * np.maximum(1.0, np.abs(ref[fin]))), name


# ---- the cases bite ---------------------------------------------------------------------------------------------------------------

def _miss(cs, got, ref):
    """Largest |got - ref| / allowance over the patterns, inf where finiteness differs."""
    if not np.array_equal(np.isfinite(got), np.isfinite(ref)):
        return np.inf
    fin = np.isfinite(ref)
    return float(np.max(np.abs(got[fin] - ref[fin]) / (sr.GPU_TOL * np.maximum(1.0, np.abs(ref[fin])))))


SHORT = [c["name"] for c in CASES if c["short"]]
ORDINARY = [c["name"] for c in CASES if c["ordinary"]]


@pytest.mark.parametrize("name", SHORT)
def test_absolute_tail_rule_loses_the_short_branch_cases(name):
    """model_series(tail="absolute") — every site in a tile of its like — pushed through the same pruning misses the reference by
    more than the GPU allowance or gives -inf; the kernel's present rule (tail="relative", looking back over the largest distance
    in the graph of any subset of the templates) does not."""
    cs = CASES[NAMES.index(name)]
    ref = _ref(cs)
    miss = _miss(cs, sr.case_reference(cs, matrix=sr.model_matrix("absolute")), ref)
    print(f"{name}: absolute rule misses by {miss:.3g} allowances")
    assert miss > 1.0, (name, miss)
    reach = sr.subset_reach(cs["T"])
    kept = _miss(cs, sr.case_reference(cs, matrix=sr.model_matrix("relative", reach=reach)), ref)
    print(f"{name}: relative rule looking {reach} terms back: {kept:.3g} allowances")
    assert kept <= 1.0, (name, kept)


@pytest.mark.parametrize("name", ["mg94_alpha0", "dense_off_chain20"])
def test_the_union_graph_is_not_enough_when_a_template_is_switched_off(name):
    """A zero or negligible multiplier takes a template out of a site's graph and lengthens distances (MG94: 3 -> 5): a rule that
    runs only the union's reach past the absolute criterion loses these cases."""
    cs = CASES[NAMES.index(name)]
    union = sr.template_reach(cs["T"])
    assert union < sr.subset_reach(cs["T"])
    miss = _miss(cs, sr.case_reference(cs, matrix=sr.model_matrix("reach", reach=union)), _ref(cs))
    print(f"{name}: {union} terms past the absolute rule: {miss:.3g} allowances")
    assert miss > 1.0, (name, miss)


@pytest.mark.parametrize("name", ORDINARY)
def test_absolute_tail_rule_keeps_the_ordinary_cases(name):
    cs = CASES[NAMES.index(name)]
    miss = _miss(cs, sr.case_reference(cs, matrix=sr.model_matrix("absolute")), _ref(cs))
    print(f"{name}: absolute rule: {miss:.3g} allowances")
    assert miss <= 1.0, (name, miss)


def test_slow_site_depends_on_its_tile_under_the_absolute_rule():
    """The same slow site: lost in a tile of its like, kept beside a site near the rate limit (the series is as long as the
    fastest lane needs) — the tile dependence the GPU test looks for."""
    cs = sr.cases_by_name()["neigh_like"]
    p = cs["probe"]
    ref = _ref(cs)[0, p]
    fast = sr.cases_by_name()["neigh_fast"]
    mu_fast = float(sr.case_rates(fast).max())
    one = dict(cs, codes=cs["codes"][:, p:p + 1], smult=cs["smult"][:, p:p + 1])
    alone = sr.case_reference(one, matrix=sr.model_matrix("absolute"))[0, 0]
    beside = sr.case_reference(one, matrix=sr.model_matrix("absolute", mu_max=mu_fast))[0, 0]
    assert np.isfinite(ref)
    assert not abs(alone - ref) <= sr.GPU_TOL * max(1.0, abs(ref))
    assert abs(beside - ref) <= sr.GPU_TOL * max(1.0, abs(ref))
