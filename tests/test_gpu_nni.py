"""hyphy_hip_nni_scores held to the scale-free reference: ``scalefree.prune`` on ``nni.apply_nni``'s tree with the matrices permuted
along (tests/nni_cases.py: ``reference``), through tests/hold.py's ``_hold``: per pattern and total at scalefree.GPU_RTOL x
|reference| + 1e-9 (the trials' bar), -inf exactly where the reference has it.  A case is ONE call with all its moves."""
import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests import common
from tests import nni_cases as nc
from tests import scalefree as sf
from tests.hold import _hold, _site

pytestmark = pytest.mark.gpu

CASES = bc.cases_by_name()
FULL = bc.full_coverage_names()
WITH_MOVES = [n for n, c in CASES.items() if nc.enumerate_moves(c["flat_parents"], int(c["L"]))]
NONE = np.zeros(0, dtype=np.int64)


def _env(monkeypatch, env=None):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _mk(cs, C=1, fp=None, **kw):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"] if fp is None else fp, int(cs["L"]), cs["leaf_codes"], cs["ambig"],
                            cs["pattern_freq"], C, **kw)


def _nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def _full(cs, part, P=None, cat=-1):
    n = _nodes(cs)
    return part.evaluate(n, n, cs["P"] if P is None else P, cs["root_freqs"], cat=cat, q_is_probability=True, per_site=True)


def _base(cs):
    ref = bc.reference(cs, key="base")
    return ref["site_logl"], ref["logl"]


def _moves(cs):
    fp, L = cs["flat_parents"], int(cs["L"])
    mv = nc.shuffled(nc.case_moves(cs), fp, L, int(cs["seed"]) + 2)
    assert not nc.can_keep_apart(mv, fp) or all(fp[a[0]] != fp[b[0]] for a, b in zip(mv, mv[1:]))
    return mv


def _call(part, mv, **kw):
    return part.nni_scores(np.array(mv, dtype=np.int64), per_site=True, **kw)


def _hold_all(cs, what, mv, got, ref=None):
    ll, lik, sc = got
    for t, (x, y) in enumerate(mv):
        r = nc.reference(cs, x, y) if ref is None else ref(x, y)
        _hold(f"{what} move ({x}, {y})", (float(ll[t]), lik[t], sc[t]), r["site_logl"], r["logl"])
        assert np.array_equal(lik[t] == 0.0, np.isneginf(r["site_logl"])), (what, x, y)


def _same(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", WITH_MOVES)
def test_every_move_of_every_case_in_one_call(name, monkeypatch):
    """2 .. 64 states (every row-block count), four-child nodes, two-child roots, the 300 / 600-taxon ladders at their lowest, a
    middle and their highest branch, the conflict trees at 1e-15 / 1e-30; the moves of a branch are not adjacent in the call.  The
    full-coverage cases make the call a second time: identical bits."""
    _env(monkeypatch)
    cs = CASES[name]
    mv = _moves(cs)
    with _mk(cs) as part:
        _hold(f"{name} full pass [{part.prune_kernel_name()}]", _full(cs, part), *_base(cs))
        got = _call(part, mv)
        _hold_all(cs, name, mv, got)
        assert np.array_equal(part.nni_scores(np.array(mv)), got[0])             # (without the per-pattern outputs)
        if name in FULL:
            assert _same(got, _call(part, mv)), name


def test_four_states(monkeypatch):
    _env(monkeypatch)
    cs = bc._make(name="bal2x4_D4", shape="bal2x4", D=4, seed=7400)
    mv = _moves(cs)
    assert len(mv) == 28
    with _mk(cs) as part:
        _hold("bal2x4_D4 full pass", _full(cs, part), *_base(cs))
        got = _call(part, mv)
        _hold_all(cs, "bal2x4_D4", mv, got)
        assert _same(got, _call(part, mv))


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bal2x4_D4", "bal2x4_D5", "bal2x4_D17", "bal2x4_D33", "bal2x4_D61"])
def test_a_fresh_partition_on_the_neighbour_tree_agrees(name, monkeypatch):
    """The second, independent check: the library's own full evaluation of the neighbour tree (apply_nni's numbering, a move that
    renumbers c behind y and one that does not) against the score of that move, at the same bar.  One case per row-block count and
    the 4-state kernels."""
    _env(monkeypatch)
    cs = CASES[name] if name in CASES else bc._make(name="bal2x4_D4", shape="bal2x4", D=4, seed=7400)
    fp, L = cs["flat_parents"], int(cs["L"])
    all_mv = nc.enumerate_moves(fp, L)
    mv = [next(m for m in all_mv if m[0] < L and m[1] > L + fp[m[0]]), next(m for m in all_mv if m[0] >= L and m[1] > L + fp[m[0]]),
          next(m for m in all_mv if m[0] >= L and L <= m[1] < L + fp[m[0]])]
    with _mk(cs) as part:
        _full(cs, part)
        ll, lik, sc = _call(part, mv)
    for t, (x, y) in enumerate(mv):
        fp2, P2 = nc.neighbour(cs, x, y)
        with _mk(cs, fp=fp2) as fresh:
            n = _nodes(cs)
            own = fresh.evaluate(n, n, P2, cs["root_freqs"], q_is_probability=True, per_site=True)
        _hold(f"{name} move ({x}, {y}) against a fresh partition", (float(ll[t]), lik[t], sc[t]), _site(own[1], own[2]), own[0])


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", nc.shape_cases(), ids=lambda c: c["name"])
def test_shapes_the_cases_lack(cs, monkeypatch):
    """tests/nni_cases.py::shape_case: a three-child root with y its third child (R carries a product), c with three children, x and y
    leaves and internal nodes, y numbered above c, ambiguity codes in x's and y's leaf rows in some tiles only, a pattern of frequency
    0, and the two moves that make pattern 7 impossible."""
    from hyphy_amd import hip
    _env(monkeypatch)
    mv = _moves(cs)
    order = hip.plan_pattern_order(int(cs["D"]), cs["leaf_codes"])
    neg = (np.asarray(cs["leaf_codes"]) < 0)[:, order]
    for l in nc.AMBIG_ROWS:                                # on the device too: tiles with and tiles without ambiguity codes in the row
        tiles = [bool(neg[l, t: t + 16].any()) for t in range(0, neg.shape[1], 16)]
        assert any(tiles) and not all(tiles), (l, tiles)
    with _mk(cs) as part:
        _hold(f"{cs['name']} full pass", _full(cs, part), *_base(cs))
        got = _call(part, mv)
        _hold_all(cs, cs["name"], mv, got)
        for m in nc.IMPOSSIBLE_MOVES:
            t = mv.index(m)
            assert got[1][t][7] == 0.0 and got[0][t] == -np.inf
        assert sum(np.isfinite(got[0])) >= len(mv) - 4
        assert _same(got, _call(part, mv))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", bc.class_cases(), ids=lambda c: c["name"])
@pytest.mark.parametrize("w", [(0.5, 0.3, 0.2), (0.6, 0.0, 0.4)], ids=["weights", "a_weight_of_0"])
def test_rate_classes(cs, w, monkeypatch):
    """Three classes (off-diagonals 1e-2, 1e-12, 1e-30) against scalefree.prune on the neighbour tree in every class with the weights
    of the call; a class of weight 0 takes no part."""
    from hyphy_amd import hip
    _env(monkeypatch)
    w = np.array(w)
    mv = _moves(cs)[:20]
    with _mk(cs, C=3) as part:
        for c in range(3):
            ref = bc.reference(cs, key="base", cls=c)
            _hold(f"{cs['name']} class {c} pass", _full(cs, part, cs["P"][c], cat=c), ref["site_logl"], ref["logl"])
        with pytest.raises(hip.HipError):
            part.nni_scores(np.array(mv))
        got = _call(part, mv, weights=w)

        def ref(x, y):
            fp2, P2 = nc.neighbour(cs, x, y)
            with np.errstate(divide="ignore"):
                return sf.prune(cs["D"], fp2, cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P2, cs["root_freqs"], weights=w)
        _hold_all(cs, cs["name"], mv, got, ref=ref)
        assert _same(got, _call(part, mv, weights=w))


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,S,mb", [(33, 70, "1"), (4, 200, "0.1")], ids=["D33", "D4"])
def test_chunks_of_tiles(D, S, mb, monkeypatch):
    """Three rate classes on the shapes the outside pass walks in chunks: 33 states, five tiles in chunks of 2, 2 and 1; 4 states, four
    waves of 64 patterns, one a chunk.  U_p is the chunk's and the class's: the chunked call is held to the reference and to the
    unchunked one."""
    _env(monkeypatch)
    cs = bc.chunked_class_case(D, S)
    B = len(cs["flat_parents"]) - 1
    w = cs["weights"]
    if D == 33:
        assert (S + 15) // 16 == 5 and (1 << 20) // (B * 16 * 48 * 8) == 2
    else:
        assert (S + 63) // 64 == 4 and int(0.1 * (1 << 20)) // (B * 256 * 8) == 0
    mv = _moves(cs)[:16]
    with _mk(cs, C=3) as part:
        for c in range(3):
            _full(cs, part, cs["P"][c], cat=c)
        whole = _call(part, mv, weights=w)
        _hold_all(cs, cs["name"], mv, whole)
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", mb)
        chunked = _call(part, mv, weights=w)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        _hold_all(cs, cs["name"] + " in chunks", mv, chunked)
        for t, m in enumerate(mv):
            _hold(f"{cs['name']} move {m}: chunked against whole", (float(chunked[0][t]), chunked[1][t], chunked[2][t]),
                  _site(whole[1][t], whole[2][t]), float(whole[0][t]))


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------

def test_class_compressed_partition(monkeypatch):
    """Moves inside a compressed subtree, on the trunk and across the two, on a partition that runs class-compressed; the next ordinary
    evaluation equals the reference and still runs compressed."""
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"))
    fx = common.compressible_case(61, 7)
    D, L = int(fx["D"]), int(fx["L"])
    fp = np.asarray(fx["flat_parents"], dtype=np.int64)
    nodes = common.all_nodes(fx)
    pi = fx["root_freqs"]
    all_mv = nc.enumerate_moves(fp, L)
    assert len(all_mv) >= 8
    mv = nc.shuffled(all_mv, fp, L, 9)[:12]
    with _mk(fx) as part:
        for _ in range(3):
            part.evaluate(nodes, nodes, fx["Q"], pi)
        P = hip.expm_batch(fx["Q"])
        cs = dict(fx, P=P, name="compressible_61_7")
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        name = part.prune_kernel_name()
        _hold_all(cs, "compressed partition", mv, _call(part, mv))
        r = sf.prune(D, fp, L, fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], P, pi)
        _hold("compressed partition: the next evaluation", part.evaluate(nodes, NONE, None, pi, per_site=True), r["site_logl"], r["logl"])
        _hold("compressed partition: the one after", part.evaluate(nodes, NONE, None, pi, per_site=True), r["site_logl"], r["logl"])
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        assert part.prune_kernel_name() == name


def test_two_shards(monkeypatch):
    """Two shards on one device (HYPHY_HIP_FORCE_SHARDS): the totals are combined as the log-likelihoods are, the per-pattern rows
    come back in the caller's order."""
    _env(monkeypatch, dict(HYPHY_HIP_FORCE_SHARDS="2"))
    cs = bc.chunked_class_case(33, 70)
    one = dict(cs, P=cs["P"][0], name=cs["name"] + "_class0")
    one.pop("weights")
    mv = _moves(one)[:12]
    with _mk(one) as part:
        ref = sf.case_reference(one)
        _hold("two shards: full pass", _full(one, part), ref["site_logl"], ref["logl"])
        got = _call(part, mv)
        _hold_all(one, "two shards", mv, got)
        assert _same(got, _call(part, mv))


def test_re_rooted_schedule(monkeypatch):
    """The call behind two full passes of a re-rooted schedule (the persisted copies on the path belong to that rooting)."""
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0"))
    cs = CASES["ladder40_D33"]
    assert len(hip.plan_reroot(cs["flat_parents"], int(cs["L"]))) > 1
    mv = _moves(cs)[:20]
    with _mk(cs) as part:
        _hold("re-rooted: full pass", _full(cs, part), *_base(cs))
        _hold("re-rooted: second full pass", _full(cs, part), *_base(cs))
        assert "re-rooted" in part.schedule_info(), part.schedule_info()
        _hold_all(cs, "re-rooted", mv, _call(part, mv))
        _hold("re-rooted: full pass after the call", part.evaluate(_nodes(cs), NONE, None, cs["root_freqs"], per_site=True), *_base(cs))


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------

def _path(cs, node):
    from hyphy_amd import tree
    return tree.flat_from_parents(cs["flat_parents"], int(cs["L"])).path_update_nodes(int(node))


@pytest.mark.parametrize("form", ["workgroup", "wave", "default"])
@pytest.mark.parametrize("name", ["bal2x4_D33", "bal4x3_D61", "bal2x4_D4"])
def test_nothing_is_left_behind(name, form, monkeypatch):
    """The same sequence on two fresh partitions, with and without the call in the middle: a branch-cache evaluation built before the
    call, a partial update, full passes, hyphy_hip_last_expm_kernel and hyphy_hip_last_reduce_form give the same bits."""
    from hyphy_amd import hip
    env = {"workgroup": dict(HYPHY_HIP_KERNEL="0", HYPHY_HIP_REPEATS="0"), "wave": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REPEATS="0"),
           "default": {}}[form]
    _env(monkeypatch, env)
    cs = CASES[name] if name in CASES else bc._make(name="bal2x4_D4", shape="bal2x4", D=4, seed=7400)
    rng = np.random.default_rng(int(cs["seed"]))
    B = len(cs["flat_parents"]) - 1
    Q = common.random_rates(rng, B, int(cs["D"]))
    cached = B // 3
    M = bc.trials(cs, cached)[3][1]
    mv = _moves(cs)[:16]
    n = _nodes(cs)

    def run(with_call):
        out = []
        with _mk(cs) as part:
            out.append(part.evaluate(n, n, Q, cs["root_freqs"], per_site=True))
            if int(cs["D"]) != 4:                          # (4 states have no branch cache)
                part.branch_cache_build(cached)
            forms = (hip.last_expm_kernel(), part.reduce_form())
            if with_call:
                got = _call(part, mv)
                assert np.all(np.isfinite(got[1]))
                assert (hip.last_expm_kernel(), part.reduce_form()) == forms
            if int(cs["D"]) != 4:
                out.append(part.branch_cache_evaluate(cached, M, q_is_probability=True, per_site=True))
            ch = np.array([cached], dtype=np.int64)
            out.append(part.evaluate(_path(cs, cached), ch, Q[ch], cs["root_freqs"], per_site=True))
            out.append(part.evaluate(_path(cs, 1), NONE, None, cs["root_freqs"], per_site=True))
            for _ in range(2):
                out.append(part.evaluate(n, NONE, None, cs["root_freqs"], per_site=True))
            out.append((np.frombuffer(hip.last_expm_kernel().encode(), dtype=np.uint8),
                        np.frombuffer(part.reduce_form().encode(), dtype=np.uint8)))
        return out
    without, with_ = run(False), run(True)
    for k, (a, b) in enumerate(zip(without, with_)):
        assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b)), (name, form, k)


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_partition_usable(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = CASES["bal2x4_D17"]
    fp, L = cs["flat_parents"], int(cs["L"])
    n = len(fp)
    root = n - 1
    good = nc.enumerate_moves(fp, L)[5]
    base = _base(cs)
    lib = hip.load()
    with _mk(cs) as part:
        with pytest.raises(hip.HipError):                  # nothing evaluated yet
            part.nni_scores([good])
        _hold("first pass", _full(cs, part), *base)
        c = L + int(fp[0])
        bad = [((root, 0), "root"), ((0, root), "root"), ((n + 3, 0), "not the code"), ((0, -1), "not the code"),
               ((root - 1, root - 2), "the parent of x is the root"), ((0, c), "y is the parent of x"), ((0, 1), "not a sibling"),
               ((0, 5), "not a sibling"), ((0, 0), "not a sibling")]
        for k, (m, word) in enumerate(bad):
            assert not nc.is_move(fp, L, *m)
            with pytest.raises(hip.HipError) as e:
                part.nni_scores([good, m])
            assert str(e.value) == f"nni_scores: move 1 ({m[0]}, {m[1]}): {nc.why_not_a_move(fp, L, *m)}" and word in str(e.value)
            _hold(f"after the refused move {m}", _full(cs, part), *base)
        part.set_pinned_states(3, np.zeros(int(cs["leaf_codes"].shape[1]), dtype=np.int64))
        with pytest.raises(hip.HipError):
            part.nni_scores([good])
        part.set_pinned_states(None)
        _hold("after the pin", _full(cs, part), *base)
        mvp, out = np.array([good], dtype=np.int64), np.full(1, -7.0)
        refused = [("no moves", (part._h, 1, None, None, hip._d(out), None, None)),
                   ("no output", (part._h, 1, hip._l(mvp), None, None, None, None)),
                   ("no partition", (None, 1, hip._l(mvp), None, hip._d(out), None, None)),
                   ("n < 0", (part._h, -1, hip._l(mvp), None, hip._d(out), None, None))]
        for what, args in refused:
            assert lib.hyphy_hip_nni_scores(*args) < 0, what
            assert lib.hyphy_hip_last_error().decode().startswith("nni_scores: "), what
            assert out[0] == -7.0
            _hold(f"after the refusal: {what}", _full(cs, part), *base)
        for args in ((part._h, 0, None, None, None, None, None), (part._h, 0, hip._l(mvp), None, hip._d(out), None, None)):
            assert lib.hyphy_hip_nni_scores(*args) == 0 and out[0] == -7.0     # n == 0: nothing written
            _hold("after n == 0", _full(cs, part), *base)
        got = _call(part, [good])
        _hold_all(cs, "a move after the refusals", [good], got)
    with _mk(cs, C=3) as part:                             # a class not yet evaluated; weights missing
        _full(cs, part, cat=0)
        _full(cs, part, cat=1)
        w = np.array([0.2, 0.3, 0.5])
        with pytest.raises(hip.HipError):
            part.nni_scores([good], weights=w)
        _hold("class 2 after the refusal", _full(cs, part, cat=2), *base)
        with pytest.raises(hip.HipError):                  # C > 1 without weights
            part.nni_scores([good])
        for c in range(3):
            _hold(f"class {c} after the refusal without weights", _full(cs, part, cat=c), *base)
        got = _call(part, [good], weights=w)               # three equal classes: the single-class reference
        _hold_all(cs, "three equal classes", [good], got)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------

def test_search_finds_the_generating_tree(monkeypatch):
    """nni.search from a tree two moves away from the one the patterns were sampled down (tests/nni_cases.py::search_case: 4 states,
    8 taxa, a three-child root, HKY85, 600 sites from seed 11), lengths fitted by brlen.fit_branch_lengths on the device.
    The seed and the site count were chosen on the CPU: tests/nni_search_check.py fits the lengths of the generating tree and of each
    of its neighbours with scalefree.prune as the likelihood and asserts that the generating tree's fitted log L is above every
    neighbour's, and above every neighbour's score at the generating tree's fitted lengths."""
    from hyphy_amd import brlen, hip, nni
    _env(monkeypatch)
    cs = nc.search_case()
    L = int(cs["L"])
    B = len(cs["flat_parents"]) - 1
    unit = np.broadcast_to(cs["Q"], (B, 4, 4)).copy()
    pi = cs["root_freqs"]

    def make(fp):
        return _mk(cs, fp=fp)

    def fit(part, t):
        ev, dv = brlen.partition_callables(part, unit, pi)
        t, _, _, _ = brlen.fit_branch_lengths(ev, dv, t)
        return t, float(ev(t))                             # (the partition is left evaluated at the fitted lengths)
    res = nni.search(make, fit, cs["start"], L, np.full(B, 0.1), restart_floor=1e-2)   # (the fit works in log t: see nni.search)
    hist = res["history"]
    print("search history", hist, "moves", res["moves"])
    assert len(hist) >= 3 and all(b >= a for a, b in zip(hist, hist[1:])), hist
    assert nc.splits(res["flat_parents"], L) == nc.splits(cs["flat_parents"], L)
    nc.check_numbering(res["flat_parents"], L)
    with make(res["flat_parents"]) as part:
        nodes = np.arange(B, dtype=np.int64)
        ll = part.evaluate(nodes, nodes, res["lengths"][:, None, None] * unit, pi)
        assert abs(ll - res["logl"]) <= 1e-9 * abs(ll)
        scores = part.nni_scores(hip.plan_nni(res["flat_parents"], L))
        assert len(scores) and np.all(scores <= ll), (ll, scores)
