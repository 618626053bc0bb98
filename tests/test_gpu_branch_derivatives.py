"""hyphy_hip_branch_derivatives / _built held to the longdouble recursion of tests/deriv_cases.py at its allowances: per pattern
|dr1| <= GPU_RTOL A1 and |dr2| <= GPU_RTOL (A2 + 2 |r1| A1), the totals at the f-weighted sums of these, NaN exactly at the skipped
patterns, exact zeros for G = 0.  A case is ONE call with all its derivatives."""
import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests import common
from tests import deriv_cases as dc
from tests import scalefree as sf
from tests.hold import _hold

pytestmark = pytest.mark.gpu

CASES = bc.cases_by_name()
FULL = bc.full_coverage_names()
EVERY = FULL + [f"bal2x4_D{D}" for D in bc.STATE_COUNTS if D not in bc.FULL_D] + ["bal2x4_D4"]
NONE = np.zeros(0, dtype=np.int64)


def _env(monkeypatch, env=None):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _case(name):
    return CASES[name] if name in CASES else dc.d4_case()


def _mk(cs, C=1, **kw):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C, **kw)


def _nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def _path(cs, node):
    from hyphy_amd import tree
    return tree.flat_from_parents(cs["flat_parents"], int(cs["L"])).path_update_nodes(int(node))


def _full(cs, part, P=None, cat=-1):
    n = _nodes(cs)
    return part.evaluate(n, n, cs["P"] if P is None else P, cs["root_freqs"], cat=cat, q_is_probability=True, per_site=True)


def _base(cs):
    """(Not through branchcache_cases' cache of references, which goes by the case's name: the 4-state case here and the one of
    tests/test_gpu_branch_trials.py share a name and differ in their seed.)"""
    ref = bc.reference(cs)
    return ref["site_logl"], ref["logl"]


def _gen_list(cs, branches=None, kinds=range(len(dc.KINDS)), C=1):
    """[(node, kind, [G of every class])], kind by kind so that the derivatives of a branch are not adjacent in the call."""
    per = {node: [dc.generators(cs, node, c) for c in range(C)] for node in (cs["branches"] if branches is None else branches)}
    return [(node, dc.KINDS[k], [per[node][c][k][1] for c in range(C)]) for k in kinds for node in per]


def _call(part, gl, weights=None):
    nodes = np.array([g[0] for g in gl], dtype=np.int64)
    return part.branch_derivatives(nodes, np.stack([np.stack(g[2]) for g in gl]), weights=weights, per_site=True)


def _hold_all(cs, what, gl, got, outs=None, weights=None):
    d1, d2, sk, s1, s2 = got
    outs = dc.outs_of(cs) if outs is None else outs
    worst = 0.0
    for t, (node, kind, Gs) in enumerate(gl):
        ref = dc.values(cs, outs, node, Gs, weights)
        m = dc.miss(s1[t], s2[t], d1[t], d2[t], ref)
        worst = max(worst, m)
        assert m <= 1.0, (what, node, kind, m)
        assert int(sk[t]) == ref["n_skipped"], (what, node, kind, int(sk[t]), ref["n_skipped"])
        assert np.array_equal(np.isnan(s1[t]), np.isnan(ref["r1"])) and np.array_equal(np.isnan(s2[t]), np.isnan(ref["r1"])), (what, node)
        if kind == "zero":
            fin = ~np.isnan(ref["r1"])
            assert d1[t] == 0.0 and d2[t] == 0.0 and np.all(s1[t][fin] == 0.0) and np.all(s2[t][fin] == 0.0), (what, node)
    print(f"{what}: {len(gl)} derivatives, largest deviation / allowance = {worst:.3g}")
    return worst


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", EVERY)
def test_every_branch_every_generator_kind(name, monkeypatch):
    """The nine full-coverage cases, the 16-taxon tree at every state count (every row-block count) and at 4 states: every branch
    with the sparse, the row-scaled, the -0.25 I and the zero generator; a second call gives the same bits."""
    _env(monkeypatch)
    cs = _case(name)
    gl = _gen_list(cs)
    with _mk(cs) as part:
        _hold(f"{name} full pass", _full(cs, part), *_base(cs))
        got = _call(part, gl)
        _hold_all(cs, name, gl, got)
        expect = len(range(5, len(cs["pattern_freq"]), 16)) if cs["impossible_at_build"] else 0
        assert np.all(got[2] == expect), (name, got[2], expect)
        assert _same(got, _call(part, gl)), name
        lean = part.branch_derivatives(np.array([g[0] for g in gl]), np.stack([g[2][0] for g in gl]))
        assert _same(lean, got[:3]), name                                          # (without the per-pattern outputs)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bigladder_D20_600", "bigladder_D61_300", "conflict_D61_1em30", "conflict_D20_1em15"])
def test_exponents_in_play(name, monkeypatch):
    _env(monkeypatch)
    cs = CASES[name]
    gl = _gen_list(cs)
    with _mk(cs) as part:
        first = _full(cs, part)
        _hold(f"{name} full pass", first, *_base(cs))
        assert np.any(first[2] != 0), name                                         # (the 2^64 exponents are in play)
        got = _call(part, gl)
        _hold_all(cs, name, gl, got)
        assert _same(got, _call(part, gl)), name


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", bc.class_cases() + [dc.ladder_class_case()], ids=lambda c: c["name"])
def test_rate_classes(cs, monkeypatch):
    """(The 40-taxon ladder beside ``class_cases()``: the case that needs in_c's exponent for the alignment.)  Three classes (off-diagonals 1e-2, 1e-12, 1e-30: their exponents differ by up to dozens of 2^64), a generator per class, under
    the case's weights, with a weight of exactly 0, and with all the weight on one class (the first: the smallest exponents; the
    last: the largest)."""
    from hyphy_amd import hip
    _env(monkeypatch)
    gl = _gen_list(cs, C=3)
    with _mk(cs, C=3) as part:
        for c in range(3):
            ref = bc.reference(cs, key="base", cls=c)
            _hold(f"{cs['name']} class {c} pass", _full(cs, part, cs["P"][c], cat=c), ref["site_logl"], ref["logl"])
        with pytest.raises(hip.HipError):
            _call(part, gl)
        for w in (cs["weights"], np.array([0.6, 0.0, 0.4]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])):
            got = _call(part, gl, weights=w)
            _hold_all(cs, f"{cs['name']} weights {list(w)}", gl, got, weights=w)
            assert _same(got, _call(part, gl, weights=w))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------

def test_chunks_of_tiles(monkeypatch):
    """S = 70 (five tiles) at 33 states on the 32-taxon tree with a 1 MB budget for the outside vectors (62 branches x 6 144 bytes a
    tile: 2.7 tiles, chunks of 2, 2 and 1) against the unchunked call: identical bits."""
    _env(monkeypatch)
    D, depth = 33, 5
    cs = bc._make(name=f"wide_bal2x{depth}_D{D}", shape="wide", D=D, seed=7410 + depth, tree=sf.balanced_tree(2, depth), S=70)
    B = len(cs["flat_parents"]) - 1
    tile_bytes = B * 16 * 48 * 8
    assert (70 + 15) // 16 == 5 and (1 << 20) // tile_bytes == 2
    cs["branches"] = [int(b) for b in np.random.default_rng(depth).choice(B, size=12, replace=False)]
    gl = _gen_list(cs)
    with _mk(cs) as part:
        _hold(f"{cs['name']} full pass", _full(cs, part), *_base(cs))
        whole = _call(part, gl)
        _hold_all(cs, cs["name"], gl, whole)
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", "1")
        chunked = _call(part, gl)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        assert _same(whole, chunked)


def test_chunks_of_tiles_four_states(monkeypatch):
    """4 states: S = 200 (four waves of 64 patterns) on the 32-taxon tree; 62 branches x 2 048 bytes a wave under the smallest budget
    the switch takes give one wave a chunk."""
    _env(monkeypatch)
    cs = bc._make(name="wide_bal2x5_D4", shape="wide", D=4, seed=7421, tree=sf.balanced_tree(2, 5), S=200)
    B = len(cs["flat_parents"]) - 1
    cs["branches"] = [int(b) for b in np.random.default_rng(4).choice(B, size=12, replace=False)]
    gl = _gen_list(cs)
    with _mk(cs) as part:
        _hold(f"{cs['name']} full pass", _full(cs, part), *_base(cs))
        whole = _call(part, gl)
        _hold_all(cs, cs["name"], gl, whole)
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", "0.1")
        chunked = _call(part, gl)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        assert _same(whole, chunked)


@pytest.mark.parametrize("D,S,mb", [(33, 70, "1"), (4, 200, "0.1")], ids=["D33", "D4"])
def test_rate_classes_in_chunks_of_tiles(D, S, mb, monkeypatch):
    """Three rate classes on the chunked shapes: 33 states, five tiles in chunks of 2, 2 and 1; 4 states, four waves of 64 patterns,
    one a chunk.  The transposed images belong to a class, so every class of every chunk needs its own: the unchunked call is held
    to the reference as ``test_rate_classes`` holds it, and the chunked call gives the same bits."""
    _env(monkeypatch)
    cs = bc.chunked_class_case(D, S)
    B = len(cs["flat_parents"]) - 1
    w = cs["weights"]
    if D == 33:
        tile_bytes = B * 16 * 48 * 8
        assert (S + 15) // 16 == 5 and (1 << 20) // tile_bytes == 2, tile_bytes
    else:
        assert (S + 63) // 64 == 4 and int(0.1 * (1 << 20)) // (B * 256 * 8) == 0
    gl = _gen_list(cs, C=3)
    with _mk(cs, C=3) as part:
        for c in range(3):
            ref = bc.reference(cs, key="base", cls=c)
            _hold(f"{cs['name']} class {c} pass", _full(cs, part, cs["P"][c], cat=c), ref["site_logl"], ref["logl"])
        whole = _call(part, gl, weights=w)
        _hold_all(cs, f"{cs['name']} weights {list(w)}", gl, whole, weights=w)
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", mb)
        chunked = _call(part, gl, weights=w)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        assert _same(whole, chunked)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------

FORMS = {"lazy": dict(HYPHY_HIP_REPEATS="0"),
         "reroot": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0")}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["bal2x4_D61", "ladder40_D33", "bal4x3_D5"])
def test_behind_a_lazy_and_a_rerooted_pass(name, form, monkeypatch):
    """Two full passes, the second of which may have kept its conditionals on chip; with "reroot" under a re-rooted schedule where
    the tree has another rooting.  A partial update follows, and the derivatives behind it see the new matrix."""
    from hyphy_amd import hip
    _env(monkeypatch, FORMS[form])
    cs = CASES[name]
    rerooted = form == "reroot" and len(hip.plan_reroot(cs["flat_parents"], int(cs["L"]))) > 1
    gl = _gen_list(cs, kinds=(0, 1))
    with _mk(cs) as part:
        for k in range(2):
            _hold(f"{name} {form} full pass {k}", _full(cs, part), *_base(cs))
        if rerooted:
            assert "re-rooted" in part.schedule_info(), part.schedule_info()
        _hold_all(cs, f"{name} {form}", gl, _call(part, gl))
        _hold(f"{name} {form}: full pass after the call", part.evaluate(_nodes(cs), NONE, None, cs["root_freqs"], per_site=True), *_base(cs))
        # a partial update: one branch gets another matrix
        node = int(cs["branches"][len(cs["branches"]) // 2])
        kind, M = bc.trials(cs, node)[3]
        ch = np.array([node], dtype=np.int64)
        want = bc.reference(cs, node, M, key=kind)
        got = part.evaluate(_path(cs, node), ch, M[None], cs["root_freqs"], q_is_probability=True, per_site=True)
        _hold(f"{name} {form}: partial update", got, want["site_logl"], want["logl"])
        P2 = cs["P"].copy()
        P2[node] = M
        moved = dict(cs, P=P2)
        _hold_all(moved, f"{name} {form} behind the partial update", gl, _call(part, gl), outs=[dc.outside(moved)])


def test_class_compressed_partition(monkeypatch):
    """A leaf branch, a branch inside a compressed subtree and a trunk branch of a partition that runs class-compressed; the next
    evaluation equals the reference and still runs compressed."""
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"))
    fx = common.compressible_case(61, 7)
    L = int(fx["L"])
    fp = np.asarray(fx["flat_parents"], dtype=np.int64)
    I = len(fp) - L
    nodes = common.all_nodes(fx)
    pi = fx["root_freqs"]
    _, comp, _ = hip.plan_repeats(fp, L, fx["leaf_codes"], 0.35)
    inside = [c for c in range(len(fp) - 1) if comp[fp[c]]]
    trunk = [L + i for i in range(I - 1) if not comp[i]]
    assert inside and trunk
    with _mk(fx) as part:
        for _ in range(3):
            part.evaluate(nodes, nodes, fx["Q"], pi)
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        name = part.prune_kernel_name()
        cs = dict(fx, name="compressible_61_7", seed=61007, P=hip.expm_batch(fx["Q"]))
        gl = _gen_list(cs, branches=[0, inside[len(inside) // 2], trunk[0]])
        _hold_all(cs, "class-compressed partition", gl, _call(part, gl), outs=[dc.outside(cs)])
        r = sf.prune(cs["D"], fp, L, cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], cs["P"], pi)
        _hold("class-compressed partition: the next evaluation", part.evaluate(nodes, NONE, None, pi, per_site=True), r["site_logl"], r["logl"])
        _hold("class-compressed partition: the one after", part.evaluate(nodes, NONE, None, pi, per_site=True), r["site_logl"], r["logl"])
        assert part.repeat_stats()["in_use"] == 1 and part.prune_kernel_name() == name


@pytest.mark.parametrize("name", ["bal2x4_D17", "bal2x4_D61", "bal2x4_D4"])
def test_behind_a_mixture_and_a_template_pass(name, monkeypatch):
    """The resident matrix of a branch is whatever the last pass left: a two-component mixture sum_m w_m exp(Q_m), then matrices
    built from coefficient rows over templates."""
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = _case(name)
    D = int(cs["D"])
    B = len(cs["flat_parents"]) - 1
    rng = np.random.default_rng(int(cs["seed"]) + 5)
    nodes = _nodes(cs)
    gl = _gen_list(cs, branches=cs["branches"][::3], kinds=(0, 1))
    Qm = common.random_rates(rng, 2 * B, D).reshape(B, 2, D, D)
    wm = rng.dirichlet([2.0, 2.0], size=B)
    K = 2
    T = rng.random((K, D, D)) + 0.05
    T[:, np.arange(D), np.arange(D)] = 0.0
    co = rng.uniform(0.01, 0.05, size=(B, K))
    Qt = np.einsum("nk,kij->nij", co, T)
    Qt[:, np.arange(D), np.arange(D)] = -Qt.sum(axis=2)

    def ref(P):
        return sf.prune(D, cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, cs["root_freqs"])
    with _mk(cs) as part:
        mixed = dict(cs, P=np.einsum("bm,bmij->bij", wm, hip.expm_batch(Qm.reshape(2 * B, D, D)).reshape(B, 2, D, D)))
        r = ref(mixed["P"])
        _hold(f"{name} mixture pass", part.evaluate_mixture(nodes, nodes, Qm, wm, cs["root_freqs"], per_site=True), r["site_logl"], r["logl"])
        _hold_all(mixed, f"{name} behind the mixture pass", gl, _call(part, gl), outs=[dc.outside(mixed)])
        built = dict(cs, P=hip.expm_batch(Qt))
        r = ref(built["P"])
        part.set_q_templates(T)
        part.build_q(co)
        _hold(f"{name} template pass", part.evaluate_built(nodes, nodes, cs["root_freqs"], per_site=True), r["site_logl"], r["logl"])
        _hold_all(built, f"{name} behind the template pass", gl, _call(part, gl), outs=[dc.outside(built)])
        _hold(f"{name}: full pass after the calls", part.evaluate(nodes, NONE, None, cs["root_freqs"], per_site=True), r["site_logl"], r["logl"])


def test_two_shards_equal_the_reference(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    if hip.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    cs = bc._make(name="wide_bal2x4_D33_two_shards", shape="wide", D=33, seed=7431, tree=sf.balanced_tree(2, 4), S=70)
    gl = _gen_list(cs)
    with _mk(cs, device_count=2) as part:
        _hold(f"{cs['name']} full pass on two shards", _full(cs, part), *_base(cs))
        got = _call(part, gl)
        _hold_all(cs, f"{cs['name']} on two shards", gl, got)
        assert _same(got, _call(part, gl))


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bal2x4_D33", "bal2x4_D4"])
def test_no_state_is_left_behind(name, monkeypatch):
    """(full pass, branch_cache_build, [derivatives,] branch_cache_evaluate, partial update, full pass) gives the same bits with the
    call and without it; reduce_form() and last_expm_kernel() answer across the call what they answered before it.  (4 states:
    without the branch cache, which that path does not have.)"""
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="0"))
    cs = _case(name)
    gl = _gen_list(cs, kinds=(0, 3))
    cached = int(cs["branches"][len(cs["branches"]) // 3])
    kind, M = bc.trials(cs, cached)[3]
    ch = np.array([cached], dtype=np.int64)
    nuc = int(cs["D"]) == 4

    def sequence(with_call):
        out = []
        with _mk(cs) as part:
            out.append(_full(cs, part))
            if not nuc:
                part.branch_cache_build(cached)
            if with_call:
                forms = (part.reduce_form(), hip.last_expm_kernel(), part.schedule_info())
                a = _call(part, gl)
                assert (part.reduce_form(), hip.last_expm_kernel(), part.schedule_info()) == forms
                assert _same(a, _call(part, gl))
                _hold_all(cs, f"{name} between the cache's build and its evaluation", gl, a)
            if not nuc:
                out.append(part.branch_cache_evaluate(cached, M, q_is_probability=True, per_site=True))
            out.append(part.evaluate(_path(cs, cached), ch, cs["P"][ch], cs["root_freqs"], q_is_probability=True, per_site=True))
            out.append(part.evaluate(_nodes(cs), NONE, None, cs["root_freqs"], per_site=True))
        return out
    for x, y in zip(sequence(False), sequence(True)):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", ["bal2x4_D4", "conflict_D20_1em15", "bal2x4_D61"])
def test_built_against_dense(name, K, monkeypatch):
    """Generators formed on the device from coefficient rows over templates against the dense call given the same generators formed
    on the host: both within the reference's allowances of the reference, and of each other."""
    _env(monkeypatch)
    cs = _case(name)
    D, L = int(cs["D"]), int(cs["L"])
    rng = np.random.default_rng(int(cs["seed"]) + K)
    nodes = np.array([1, L + 8, 5, 1, L + 2], dtype=np.int64)
    T = (rng.random((K, D, D)) + 0.05) * (rng.random((K, D, D)) < 0.5)
    T[:, np.arange(D), np.arange(D)] = 0.0
    co = rng.uniform(0.002, 0.3, size=(len(nodes), K)) / D
    G = np.einsum("nk,kij->nij", co, T)
    G[:, np.arange(D), np.arange(D)] = -G.sum(axis=2)
    outs = dc.outs_of(cs)
    with _mk(cs) as part:
        _hold(f"{name} full pass", _full(cs, part), *_base(cs))
        part.set_q_templates(T)
        built = part.branch_derivatives_built(nodes, co, per_site=True)
        dense = part.branch_derivatives(nodes, G, per_site=True)
        for t, node in enumerate(nodes):
            ref = dc.values(cs, outs, int(node), [G[t]])
            for what, got in (("built", built), ("dense", dense)):
                m = dc.miss(got[3][t], got[4][t], got[0][t], got[1][t], ref)
                assert m <= 1.0, (name, K, t, what, m)
                assert int(got[2][t]) == ref["n_skipped"]
            twin = dict(ref, r1=dense[3][t], r2=dense[4][t], d1=dense[0][t], d2=dense[1][t])
            m = dc.miss(built[3][t], built[4][t], built[0][t], built[1][t], twin)
            assert m <= 1.0, (name, K, t, "built against dense", m)
        _hold(f"{name}: full pass after the calls", part.evaluate(_nodes(cs), NONE, None, cs["root_freqs"], per_site=True), *_base(cs))


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_partition_usable(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = CASES["bal2x4_D17"]
    B = len(cs["flat_parents"]) - 1
    G = dc.generators(cs, 0)[0][1][None]
    base = _base(cs)
    one = np.zeros(1, dtype=np.int64)
    with _mk(cs) as part:
        with pytest.raises(hip.HipError):                  # nothing evaluated yet
            part.branch_derivatives([0], G)
        _hold("first pass", _full(cs, part), *base)
        for bad in (B, B + 1, -1):                         # the root's code, past it, negative
            with pytest.raises(hip.HipError):
                part.branch_derivatives([0, bad], np.concatenate([G, G]))
            _hold(f"after node code {bad}", _full(cs, part), *base)
        part.set_pinned_states(3, np.zeros(int(cs["leaf_codes"].shape[1]), dtype=np.int64))
        with pytest.raises(hip.HipError):
            part.branch_derivatives([0], G)
        part.set_pinned_states(None)
        _hold("after the pin", _full(cs, part), *base)
        with pytest.raises(hip.HipError):                  # templates not set
            part.branch_derivatives_built([0], np.ones((1, 2)))
        _hold("after the missing templates", _full(cs, part), *base)
        lib, d = part._lib, np.full(1, 7.0)
        assert lib.hyphy_hip_branch_derivatives(part._h, 1, hip._l(one), hip._d(G), None, None, hip._d(d), None, None, None) < 0
        assert lib.hyphy_hip_branch_derivatives(part._h, 1, hip._l(one), hip._d(G), None, hip._d(d), None, None, None, None) < 0
        assert lib.hyphy_hip_branch_derivatives(part._h, 1, hip._l(one), None, None, hip._d(d), hip._d(d), None, None, None) < 0
        assert lib.hyphy_hip_branch_derivatives(None, 1, hip._l(one), hip._d(G), None, hip._d(d), hip._d(d), None, None, None) < 0
        _hold("after the null pointers", _full(cs, part), *base)
        d1, d2, sk = np.full(1, 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int64)
        assert lib.hyphy_hip_branch_derivatives(part._h, 0, hip._l(one), hip._d(G), None, hip._d(d1), hip._d(d2), hip._l(sk), None, None) == 0
        assert lib.hyphy_hip_branch_derivatives(part._h, 0, None, None, None, None, None, None, None, None) == 0
        assert d[0] == 7.0 and d1[0] == 7.0 and d2[0] == 7.0 and sk[0] == 7
        gl = _gen_list(cs, branches=[0, B - 1])
        _hold_all(cs, "a call after the refusals", gl, _call(part, gl))
    with _mk(cs, C=3) as part:                             # a class not yet evaluated
        _full(cs, part, cat=0)
        _full(cs, part, cat=1)
        with pytest.raises(hip.HipError):
            part.branch_derivatives([0], np.stack([G[0]] * 3)[None], weights=np.array([0.2, 0.3, 0.5]))
        _hold("class 2 after the refusal", _full(cs, part, cat=2), *base)
        with pytest.raises(hip.HipError):                  # C > 1 without weights
            part.branch_derivatives([0], np.stack([G[0]] * 3)[None])
        _hold("class 0 after the refusal", _full(cs, part, cat=0), *base)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,n_sites,seed,t_range,rates,weights",
                         [(5, 400, 7605, (0.05, 0.4), None, None), (61, 40, 7602, (0.15, 0.5), None, None),
                          (4, 400, 7605, (0.15, 0.5), (0.5, 1.5), (0.5, 0.5))], ids=["D5", "D61", "D4_two_classes"])
def test_newton_on_the_device(D, n_sites, seed, t_range, rates, weights, monkeypatch):
    """brlen.partition_callables + fit_branch_lengths on an 8-taxon tree (40 patterns at 5 and 61 states, one class; every pattern
    of 400 sites at 4 states, two classes): monotone, ends within max_iter, and at the returned lengths the scale-free reference
    log L is not raised by 1 % more or less on any single branch — beyond what the stopping rule itself leaves: the iteration ends
    with max |d1| <= tol max(1, |log L|), and a step of |log 0.99| along one theta_b from there gains at most |d1_b| |log 0.99|
    where log L is concave in theta_b (at 5 states two branches end at the boundary t -> 0, where it is: log L = c - s exp(theta)).
    On the host (numpy callables) the three cases end after 15, 15 and 34 iterations."""
    from tests import expm_ref
    from hyphy_amd import brlen
    _env(monkeypatch)
    cs = dc.fit_case(f"fit8_D{D}", dc.FIT_TREE_8, D, n_sites, seed, max_patterns=None if rates else 40, t_range=t_range)
    B = len(cs["flat_parents"]) - 1
    rates = None if rates is None else np.array(rates)
    weights = None if weights is None else np.array(weights)
    with _mk(cs, C=1 if rates is None else len(rates)) as part:
        ev, de = brlen.partition_callables(part, cs["unit_Q"], cs["root_freqs"], rates, weights)
        t, ll, it, hist = brlen.fit_branch_lengths(ev, de, np.full(B, 0.1))
    print(f"fit8_D{D}: {it} iterations, log L {hist[0]:.6f} -> {ll:.6f}, lengths {t.min():.3g} .. {t.max():.3g}")
    assert it < 50 and len(hist) == it + 1 and ll > hist[0]
    assert all(b >= a for a, b in zip(hist, hist[1:]))
    P = dc.fit_model(cs, t, rates)

    def ref(P):
        return sf.prune(D, cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, cs["root_freqs"],
                        weights=weights)["logl"]
    top = ref(P)
    slack = abs(np.log(0.99)) * 1e-8 * max(1.0, abs(top))
    assert abs(top - ll) <= sf.GPU_RTOL * abs(top) + 1e-9
    for b in range(B):
        for fac in (0.99, 1.01):
            P2 = P.copy()
            for c, r in enumerate([1.0] if rates is None else rates):
                M = expm_ref.reference(r * fac * t[b] * cs["unit_Q"][b])
                if rates is None:
                    P2[b] = M
                else:
                    P2[c, b] = M
            assert ref(P2) <= top + slack, (b, fac, ref(P2) - top)
