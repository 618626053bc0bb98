"""hyphy_hip_site_fits_evaluate / _mixture (sitefit.hip) held to the componentwise-accurate reference of tests/sitefit_ref.py on the
cases where that kernel can go wrong: structured templates (entries several substitutions away), coefficients down to 1e-13, slow
sites in fast and in empty tiles, every row-block count, mixtures with dead components, rates at the sub-series boundaries, and
trees deep enough for its own 2^64 steps and scratch spills.

Allowance: the bar the entry point already carries (tests/test_gpu_parity.py::test_site_fits_*): |got - ref| <= 1e-9 max(1, |ref|)
per site, -inf exactly where the reference has it, finite values finite.  The worst deviation / allowance is printed per case."""
import numpy as np
import pytest

from tests import sitefit_ref as sr

pytestmark = pytest.mark.gpu

CASES = sr.cases_by_name()
NAMES = list(CASES)
TOL = sr.GPU_TOL
_refs = {}


def _ref(name):
    if name not in _refs:
        _refs[name] = sr.case_reference(CASES[name])
    return _refs[name]


def _mk(cs):
    from hyphy_amd import hip
    S = cs["codes"].shape[1]
    part = hip.HipPartition(cs["D"], cs["flat_parents"], cs["L"], cs["codes"], cs["ambig"], np.ones(S, dtype=np.int64))
    part.set_q_templates(cs["T"])
    return part


def _evaluate(part, cs, smult=None, smix=None):
    smult = cs["smult"] if smult is None else smult
    if cs["smix"] is None:
        return part.site_fits_evaluate(cs["bgroup"], cs["bcoef"], smult, cs["pi"])
    return part.site_fits_evaluate_mixture(cs["bgroup"], cs["bcoef"], smult, cs["smix"] if smix is None else smix, cs["pi"])


def _hold(what, got, ref):
    assert got.shape == ref.shape, what
    assert not np.isnan(got).any() and not np.isposinf(got).any(), (what, got)
    wrong = np.argwhere(np.isneginf(got) != np.isneginf(ref))
    fin = np.isfinite(ref) & np.isfinite(got)
    dev = np.abs(got[fin] - ref[fin]) / (TOL * np.maximum(1.0, np.abs(ref[fin])))
    worst = float(dev.max()) if fin.any() else 0.0
    print(f"{what}: largest per-site deviation / allowance = {worst:.3g}; {len(wrong)} of {ref.size} values -inf on one side only "
          f"({int(np.isneginf(ref).sum())} -inf in the reference)")
    assert len(wrong) == 0, (what, "-inf on one side only at (set, site)", wrong[:8].tolist())
    assert worst <= 1.0, (what, worst, np.argwhere(fin)[int(np.argmax(dev))].tolist())


def _run(name, env, monkeypatch):
    """The case under ``env``: the same call twice with a single-set call in between, bit-identical, held to the reference."""
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cs = CASES[name]
    with _mk(cs) as part:
        got = _evaluate(part, cs)
        one = _evaluate(part, cs, cs["smult"][0], None if cs["smix"] is None else cs["smix"][0])
        again = _evaluate(part, cs)
    assert np.array_equal(again, got, equal_nan=True), (name, env)
    assert np.array_equal(one, got[0], equal_nan=True), (name, env)
    _hold(f"{name} {env}", got, _ref(name))
    return got


@pytest.mark.parametrize("name", NAMES)
def test_every_case_against_the_reference(name, monkeypatch):
    _run(name, {}, monkeypatch)


VARIANTS = {"unsorted": dict(HYPHY_HIP_SORT_PATTERNS="0"), "sorted": dict(HYPHY_HIP_SORT_PATTERNS="1"),
            "shards3": dict(HYPHY_HIP_FORCE_SHARDS="3")}
VARIED = list(sr.NEIGHBOURS) + ["mg94_span", "chain20_span", "block_isolated_impossible", "mix2_mg94", "shape_D49", "conflict_k4_d2_mg94",
                                "balanced128_mg94"]


@pytest.mark.parametrize("name", VARIED)
def test_sorted_unsorted_and_sharded_runs_agree(name, monkeypatch):
    """Each held to the reference; and with each other: to the bit where the tiles are the same sets of sites (one tile or less:
    sorted against unsorted — the stopping decisions are taken on the tile, not on the lane; one site: all three), to the
    allowance otherwise."""
    got = {v: _run(name, env, monkeypatch) for v, env in VARIANTS.items()}
    S = CASES[name]["codes"].shape[1]
    if S <= 16:
        assert np.array_equal(got["sorted"], got["unsorted"]), name
    if S == 1:
        assert np.array_equal(got["shards3"], got["unsorted"]), name
    for v in ("sorted", "shards3"):
        a, b = got[v], got["unsorted"]
        assert np.array_equal(np.isneginf(a), np.isneginf(b)), (name, v)
        fin = np.isfinite(b)
        assert np.all(np.abs(a[fin] - b[fin]) <= TOL * np.maximum(1.0, np.abs(b[fin]))), (name, v)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_slow_site_does_not_depend_on_its_tile(variant, monkeypatch):
    """The same slow site (a cherry three nucleotides apart, coefficients ~1e-9) in a tile of its like, beside a site near the
    rate limit, and as the only real site of a padded tile (S = 1, S = 17): one value, the reference's."""
    vals = {}
    for name in sr.NEIGHBOURS:
        cs = CASES[name]
        got = _run(name, VARIANTS[variant], monkeypatch)
        vals[name] = (float(got[0, cs["probe"]]), float(_ref(name)[0, cs["probe"]]))
    print(f"{variant}: " + "; ".join(f"{n} {g!r}" for n, (g, _) in vals.items()))
    refs = [r for (_, r) in vals.values()]
    assert np.isfinite(refs).all() and max(refs) - min(refs) <= 1e-12 * abs(refs[0])
    for n, (g, r) in vals.items():
        assert np.isfinite(g) and abs(g - r) <= TOL * max(1.0, abs(r)), (variant, n, g, r)
    gs = [g for (g, _) in vals.values()]
    assert max(gs) - min(gs) <= TOL * max(1.0, abs(refs[0])), (variant, vals)


def _short_branch_alignment():
    """Ten taxa, MG94 templates; five branches with coefficients near 1e-9 (two of them above the leaves of one cherry, one an
    internal branch), and a few sites whose codons differ by two and three nucleotides across exactly those branches."""
    from tests import scalefree as sf
    rng = np.random.default_rng(4242)
    T, pi = sr.mg94_templates()
    fp, L = sf.ladder_tree(10)
    B = len(fp) - 1
    S = 32
    base = rng.integers(0, 61, size=S)
    codes = np.where(rng.random((L, S)) < 0.25, rng.integers(0, 61, size=(L, S)), base[None, :]).astype(np.int64)
    A, C3, C2, G, G2 = sr.codon("AAA"), sr.codon("CCC"), sr.codon("ACC"), sr.codon("GGG"), sr.codon("GCC")
    codes[:, 0] = A
    codes[1, 0] = C3                     # leaves 0, 1: the cherry on two short branches, three nucleotides apart
    codes[:, 1] = A
    codes[1, 1] = C2
    codes[:, 2] = G
    codes[:3, 2] = G2                    # below the short internal branch above (0, 1, 2): two nucleotides
    codes[:, 3] = A
    codes[7, 3] = C3                     # the odd leaf on a short branch
    syn = rng.uniform(0.02, 0.4, B)
    short = np.array([0, 1, 7, L + 1, 5])
    syn[short] = rng.uniform(0.5e-9, 2e-9, len(short))
    nonsyn = syn * rng.uniform(0.3, 1.0, B)
    tested = np.zeros(B, dtype=bool)
    tested[[0, 3, 7, L + 1, L + 4]] = True
    return fp, L, codes, T, pi, syn, nonsyn, tested, S


def test_fel_on_a_short_branch_alignment(monkeypatch):
    """hyphy_amd/fel.py::fel where several branches have coefficients near 1e-9 and a few sites carry multi-nucleotide differences
    across them: the fitted logl_alt is reproduced by the reference at the fitted parameters, and no site comes back -inf that the
    reference finds finite (at the fitted parameters and on the starting grid)."""
    from hyphy_amd import fel, hip
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    fp, L, codes, T, pi, syn, nonsyn, tested, S = _short_branch_alignment()
    group = np.where(tested, 0, 1).astype(np.int64)
    bc = np.stack([syn, nonsyn], axis=1)
    pm = np.array([[0, 1], [0, 2]])
    grid_theta = np.broadcast_to(np.array([(a, b, b) for a, b in fel.START_GRID])[:, None, :], (len(fel.START_GRID), S, 3))
    with hip.HipPartition(61, fp, L, codes, None, np.ones(S, dtype=np.int64)) as part:
        part.set_q_templates(T)
        res = fel.fel(part, tested, syn, nonsyn, pi, max_iter=200)
        theta = np.stack([res.alpha, res.beta, res.beta_nuisance], axis=1)
        again = part.site_fits_evaluate(group, bc, fel._multipliers(theta, pm), pi)
        grid = part.site_fits_evaluate(group, bc, fel._multipliers(grid_theta, pm), pi)
    want = sr.site_fit_logl(61, fp, L, codes, None, pi, T, group, bc, fel._multipliers(theta, pm)[None])[0]
    want_grid = sr.site_fit_logl(61, fp, L, codes, None, pi, T, group, bc, fel._multipliers(grid_theta, pm))
    assert np.isfinite(want).all() and np.isfinite(want_grid).all()
    _hold("fel short branches: the whole starting grid", grid, want_grid)
    _hold("fel short branches: logl_alt at the fitted parameters", np.asarray(res.logl_alt)[None], want[None])
    _hold("fel short branches: re-evaluation", again[None], want[None])
    assert np.isfinite(res.logl_null).all() and (res.logl_alt >= res.logl_null - 1e-7).all()
    assert ((res.p_value >= 0) & (res.p_value <= 1)).all()


def test_error_paths_stay_refused():
    """A rate just above kSiteFitMaxRate, a negative template off-diagonal entry, five templates."""
    from hyphy_amd import hip
    cs = CASES["rate_4095"]
    with _mk(cs) as part:
        ok = _evaluate(part, cs)
        _hold("rate_4095 before the refusals", ok, _ref("rate_4095"))
        with pytest.raises(hip.HipUnsupported):
            part.site_fits_evaluate(cs["bgroup"], cs["bcoef"] * (4097.0 / 4095.0), cs["smult"], cs["pi"])
        bad = cs["T"].copy()
        bad[0, 2, 3] = -0.25
        part.set_q_templates(bad)
        with pytest.raises(hip.HipError):
            part.site_fits_evaluate(cs["bgroup"], cs["bcoef"], cs["smult"], cs["pi"])
        part.set_q_templates(np.repeat(cs["T"], 5, axis=0))
        S, B = cs["codes"].shape[1], len(cs["flat_parents"]) - 1
        with pytest.raises(hip.HipError):
            part.site_fits_evaluate(cs["bgroup"], np.full((B, 5), 0.1), np.ones((1, S, 1, 5)), cs["pi"])
        part.set_q_templates(cs["T"])
        assert np.array_equal(_evaluate(part, cs), ok)
