"""CPU-only: the host side of the nearest-neighbour interchanges.  hyphy_hip_plan_nni against the rule in plain Python, nni.apply_nni's
numbering on every move, and the formula the kernels implement (tests/nni_cases.py::model, numpy with the 2^64 rule) against
scalefree.prune on the neighbour tree, at scalefree.GPU_RTOL x |reference| + 1e-9 per pattern: the bar the GPU tests hold the device
to (tests/hold.py)."""
import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests import nni_cases as nc
from tests import scalefree as sf


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from hyphy_amd import hip as h
    return h


@pytest.mark.parametrize("name", sorted(nc.PLAN_TREES))
def test_plan_lists_every_move_in_order(name, hip):
    fp, L = nc.PLAN_TREES[name]()
    nc.check_numbering(fp, L)
    want = nc.enumerate_moves(fp, L)
    got = hip.plan_nni(fp, L)
    assert got.shape == (len(want), 2) and got.dtype == np.int64
    assert [tuple(int(v) for v in m) for m in got] == want, name
    if name in ("star", "three_leaves"):
        assert len(want) == 0
    if name == "balanced":                                 # binary: two moves per child of an internal non-root node ... per sibling
        I = len(fp) - L
        assert len(want) == 2 * (I - 1)
    if name == "wide41":
        wide = [c for c, k in enumerate(sf.children_of(fp, L)) if len(k) == 41]
        assert len(wide) == 1 and sum(1 for x, _ in want if fp[x] == wide[0]) == 41 * 2


@pytest.mark.parametrize("name", sorted(nc.PLAN_TREES))
def test_the_plan_is_exactly_the_pairs_the_rule_admits(name, hip):
    """Every pair of node codes (the root's and codes out of range included) is a move exactly when it is in the plan, and exactly
    then hyphy_hip_check_nni lets it pass: the host-only entry point runs the function hyphy_hip_nni_scores refuses by
    (nni_plan.h: nni_moves_error over nni_move_error, which the planner filters its candidates through), and names the pair and
    the part of the rule it breaks in the same words."""
    fp, L = nc.PLAN_TREES[name]()
    n = len(fp)
    planned = {tuple(int(v) for v in m) for m in hip.plan_nni(fp, L)}
    if planned:
        hip.check_nni(fp, L, sorted(planned))
    hip.check_nni(fp, L, np.zeros((0, 2), dtype=np.int64))
    rng = np.random.default_rng(5)
    pairs = [(x, y) for x in range(-1, n + 1) for y in range(-1, n + 1)]
    if len(pairs) > 4000:
        pairs = [pairs[k] for k in rng.choice(len(pairs), size=4000, replace=False)] + sorted(planned)
    good = sorted(planned)[:1]
    reasons = set()
    for x, y in pairs:
        assert nc.is_move(fp, L, x, y) == ((x, y) in planned), (name, x, y)
        why = nc.why_not_a_move(fp, L, x, y)
        assert (why is None) == ((x, y) in planned)
        if why is None:
            hip.check_nni(fp, L, [(x, y)])
            continue
        reasons.add(why)
        with pytest.raises(hip.HipError) as e:
            hip.check_nni(fp, L, good + [(x, y)])
        assert str(e.value) == f"check_nni: move {len(good)} ({x}, {y}): {why}", (name, x, y, str(e.value))
    assert "x is not the code of a branch (the root has none)" in reasons and "the parent of x is the root" in reasons
    if planned:
        assert {"y is the parent of x", "y is not a sibling of the parent of x"} <= reasons


def test_check_refuses_bad_arguments(hip):
    lib = hip.load()
    fp, L = nc.PLAN_TREES["three_child_root"]()
    I = len(fp) - L
    mv = np.array(nc.enumerate_moves(fp, L)[:2], dtype=np.int64)
    assert lib.hyphy_hip_check_nni(L, I, hip._l(fp), 2, hip._l(mv)) == 0
    assert lib.hyphy_hip_check_nni(L, I, hip._l(fp), 0, None) == 0
    assert lib.hyphy_hip_check_nni(L, I, hip._l(fp), 2, None) < 0
    assert lib.hyphy_hip_check_nni(L, I, hip._l(fp), -1, hip._l(mv)) < 0
    assert lib.hyphy_hip_check_nni(L, I, None, 2, hip._l(mv)) < 0
    bad = np.array([0, 0, 1, 1, 5, 2, -1], dtype=np.int64)
    assert lib.hyphy_hip_check_nni(4, 3, hip._l(bad), 2, hip._l(mv)) < 0
    assert lib.hyphy_hip_last_error().decode().startswith("check_nni: ")


def test_plan_refuses_bad_trees_and_follows_the_cap_convention(hip):
    lib = hip.load()
    fp, L = nc.PLAN_TREES["three_child_root"]()
    I = len(fp) - L
    want = nc.enumerate_moves(fp, L)
    words = 1 + 2 * len(want)
    assert lib.hyphy_hip_plan_nni(L, I, hip._l(fp), None, 0) == -words
    out = np.full(words + 3, -7, dtype=np.int64)
    assert lib.hyphy_hip_plan_nni(L, I, hip._l(fp), hip._l(out), words - 1) == -words and np.all(out == -7)
    assert lib.hyphy_hip_plan_nni(L, I, hip._l(fp), hip._l(out), len(out)) == words
    assert out[0] == len(want) and np.all(out[words:] == -7)
    star, Ls = nc.PLAN_TREES["star"]()
    one = np.full(1, -7, dtype=np.int64)
    assert lib.hyphy_hip_plan_nni(Ls, 1, hip._l(star), hip._l(one), 1) == 1 and one[0] == 0
    for bad in (np.array([0, 0, 1, 1, 5, 2, -1]), np.array([0, 0, 1, 1, 2, 2, 0]), np.array([0, 0, 1, 1, -1, 2, -1])):
        bad = bad.astype(np.int64)
        assert lib.hyphy_hip_plan_nni(4, 3, hip._l(bad), hip._l(out), len(out)) == -1
        assert lib.hyphy_hip_last_error().decode().startswith("plan_nni: ")
        with pytest.raises(hip.HipError):
            hip.plan_nni(bad, 4)
    assert lib.hyphy_hip_plan_nni(4, 3, None, hip._l(out), len(out)) == -1
    assert lib.hyphy_hip_plan_nni(0, 3, hip._l(fp), hip._l(out), len(out)) == -1


@pytest.mark.parametrize("name", sorted(nc.PLAN_TREES))
def test_apply_nni_numbers_every_neighbour_validly(name):
    from hyphy_amd import nni
    fp, L = nc.PLAN_TREES[name]()
    n = len(fp)
    ch = sf.children_of(fp, L)
    moved = 0
    for x, y in nc.enumerate_moves(fp, L):
        fp2, perm = nni.apply_nni(fp, L, x, y)
        nc.check_numbering(fp2, L)
        assert sorted(perm) == list(range(n)) and list(perm[:L]) == list(range(L)) and perm[-1] == n - 1
        c, p = L + int(fp[x]), L + int(fp[L + int(fp[x])])
        new_of = np.argsort(perm)
        kids = {L + i: sorted(int(perm[k]) for k in kk) for i, kk in enumerate(sf.children_of(fp2, L))}
        kids = {int(perm[k]): v for k, v in kids.items()}                        # in old codes
        for node in range(L, n):
            want = set(ch[node - L])
            if node == c:
                want = want - {x} | {y}
            if node == p:
                want = want - {y} | {x}
            assert set(kids[node]) == want, (name, x, y, node)
        rest = [int(k) for k in perm[L:] if k != c]                              # internal nodes keep their order but for c
        assert rest == [k for k in range(L, n) if k != c]
        if y >= L and y > c:
            assert new_of[c] == new_of[y] + 1
            moved += 1
        else:
            assert np.array_equal(perm, np.arange(n))
    if name in ("balanced", "shapes", "two_child_root"):
        assert moved > 0
    for x, y in ((0, 0), (n - 1, 0), (0, n - 1), (-1, 0)):
        if not nc.is_move(fp, L, x, y):
            with pytest.raises(ValueError):
                nni.apply_nni(fp, L, x, y)


def _hold_model(cs, moves, cls=None):
    worst = 0.0
    for (x, y), (lik, e) in zip(moves, nc.model(cs, moves, cls)):
        fp2, P2 = nc.neighbour(cs, x, y)
        ref = sf.prune(cs["D"], fp2, cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P2 if cls is None else P2[cls],
                       cs["root_freqs"])["site_logl"]
        with np.errstate(divide="ignore"):
            got = np.log(lik) - sf.LOG_SCALER * e
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (cs["name"], x, y)
        fin = np.isfinite(ref)
        if fin.any():
            worst = max(worst, float(np.max(np.abs(got[fin] - ref[fin]) / (sf.GPU_RTOL * np.abs(ref[fin]) + 1e-9))))
    print(f"{cs['name']}: {len(moves)} moves, largest deviation / allowance {worst:.3g}")
    assert worst <= 1.0, (cs["name"], worst)


@pytest.mark.parametrize("cs", nc.shape_cases(), ids=lambda c: c["name"])
def test_formula_on_the_shapes(cs):
    """Every move of the shape tree: a three-child root with y its third child, c with three children, x and y leaves and internal
    nodes, y numbered above c, ambiguity codes, an impossible pattern."""
    fp, L = cs["flat_parents"], int(cs["L"])
    moves = nc.enumerate_moves(fp, L)
    c_of = lambda x: L + int(fp[x])
    assert any(y >= L and y > c_of(x) for x, y in moves) and any(y >= L and y < c_of(x) for x, y in moves)
    assert any(y < L for x, y in moves) and any(x < L for x, y in moves) and any(x >= L for x, y in moves)
    ch = sf.children_of(fp, L)
    assert any(len(ch[int(fp[x])]) == 3 for x, y in moves)
    assert any(len(ch[-1]) == 3 and fp[y] == len(ch) - 1 and y == ch[-1][2] for x, y in moves)
    assert any(len(ch[int(fp[y])]) == 3 and fp[y] != len(ch) - 1 for x, y in moves)
    _hold_model(cs, moves)
    base = sf.case_reference(cs)["site_logl"]
    assert np.isfinite(base[7]) and cs["pattern_freq"][3] == 0
    for m in nc.IMPOSSIBLE_MOVES:
        assert m in moves and np.isneginf(nc.reference(cs, *m)["site_logl"][7])
    finite = [m for m in moves if np.isfinite(nc.reference(cs, *m)["logl"])]
    assert len(finite) >= len(moves) - 4, (len(finite), len(moves))
    neg = np.asarray(cs["leaf_codes"]) < 0
    assert set(np.flatnonzero(neg.any(axis=1))) == set(nc.AMBIG_ROWS) and not neg[:, :16].any() and not neg[:, 32:].any()


@pytest.mark.parametrize("name", ["bal2x4_D5", "bal4x3_D5", "root_internal_internal_D17", "starbelow5_D5", "conflict_D20_1em30",
                                  "bigladder_D20_600"])
def test_formula_where_rescaling_bites(name):
    """Branch-cache cases: binary and four-child nodes, a two-child root, near-identity matrices at 1e-30 (exponents far from zero)
    and the 600-taxon ladder at its lowest, a middle and its highest branch."""
    cs = bc.cases_by_name()[name]
    moves = nc.case_moves(cs)
    assert moves
    if name == "bal4x3_D5":
        moves = moves[::7]
    _hold_model(cs, moves)
    if name in ("conflict_D20_1em30", "bigladder_D20_600"):
        assert max(int(np.abs(e).max()) for _, e in nc.model(cs, moves[:4])) >= 1


def test_formula_per_class():
    cs = bc.class_cases()[0]
    moves = nc.shuffled(nc.enumerate_moves(cs["flat_parents"], int(cs["L"])), cs["flat_parents"], int(cs["L"]), 3)[:6]
    for c in range(3):
        _hold_model(cs, moves, cls=c)


def test_shuffled_keeps_a_branch_apart():
    fp, L = sf.balanced_tree(2, 4)
    mv = nc.enumerate_moves(fp, L)
    sh = nc.shuffled(mv, fp, L, 1)
    assert sorted(sh) == sorted(mv)
    assert all(fp[a[0]] != fp[b[0]] for a, b in zip(sh, sh[1:]))


def test_search_case_is_two_moves_from_the_generating_tree():
    cs = nc.search_case()
    L = int(cs["L"])
    nc.check_numbering(cs["start"], L)
    assert len(nc.splits(cs["start"], L) - nc.splits(cs["flat_parents"], L)) == 2
    assert cs["leaf_codes"].shape[0] == 8 and int(cs["pattern_freq"].sum()) == nc.SEARCH_SITES
    assert len(sf.children_of(cs["flat_parents"], L)[-1]) == 3 and len(sf.children_of(cs["start"], L)[-1]) == 3


class _FakePart:
    made = []

    def __init__(self, fp, scores):
        self.fp, self.scores, self.closed = fp, scores, 0
        _FakePart.made.append(self)

    def nni_scores(self, moves, weights=None):
        return np.asarray(self.scores(len(moves)), dtype=np.float64)

    def close(self):
        self.closed += 1


def test_search_closes_what_it_opened_and_skips_impossible_neighbours(hip):
    """nni.search over a stand-in partition: a fit that raises on the round's third candidate, while the first is held as the best so
    far, leaves no partition open; candidates whose score is -inf or NaN are not rebuilt; the floor on the starting lengths is off
    unless asked for."""
    from hyphy_amd import nni
    fp, L = nc.PLAN_TREES["three_child_root"]()
    B = len(fp) - 1
    n_moves = len(nc.enumerate_moves(fp, L))
    assert n_moves >= 4
    seen = []

    def run(scores, fit, **kw):
        _FakePart.made = []
        try:
            return nni.search(lambda f: _FakePart(f, scores), fit, fp, L, np.full(B, 1e-5), **kw)
        finally:
            assert all(p.closed >= 1 for p in _FakePart.made), [p.closed for p in _FakePart.made]

    def failing_fit(part, t):
        seen.append(np.array(t))
        k = len(_FakePart.made)
        if k == 4:
            raise RuntimeError("fit failed")
        return t, -100.0 + k                               # the start -99, candidates -98, -97: the first is held when the third raises
    with pytest.raises(RuntimeError):
        run(lambda n: -np.arange(n, dtype=np.float64), failing_fit)
    assert len(_FakePart.made) == 4 and all(np.all(t == 1e-5) for t in seen)
    seen.clear()
    with pytest.raises(RuntimeError):
        run(lambda n: -np.arange(n, dtype=np.float64), failing_fit, restart_floor=1e-2)
    assert np.all(seen[0] == 1e-5) and all(np.all(t == 1e-2) for t in seen[1:])

    def scores(n):
        s = np.full(n, -np.inf)
        s[1] = np.nan
        s[2] = -5.0
        return s
    res = run(scores, lambda part, t: (t, -50.0), max_rounds=3)
    assert len(_FakePart.made) == 2 and res["history"] == [-50.0] and res["moves"] == []   # one finite candidate, no gain
