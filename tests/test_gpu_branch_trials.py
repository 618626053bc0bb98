"""hyphy_hip_branch_trials / _built held to the scale-free reference the branch cache is held to (tests/branchcache_cases.py:
``reference`` = ``scalefree.prune`` with the branch's matrix substituted) through tests/hold.py's ``_hold``: per pattern and total at
scalefree.GPU_RTOL x |reference| + 1e-9, -inf exactly where the reference has it.  A case is ONE call with all its trials."""
import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests import common
from tests import scalefree as sf
from tests.hold import _hold, _site

pytestmark = pytest.mark.gpu

CASES = bc.cases_by_name()
FULL = bc.full_coverage_names()
D4 = dict(name="bal2x4_D4", shape="bal2x4", D=4, seed=7400)


def _env(monkeypatch, env=None):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _mk(cs, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def _nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def _path(cs, node):
    from hyphy_amd import tree
    return tree.flat_from_parents(cs["flat_parents"], int(cs["L"])).path_update_nodes(int(node))


def _full(cs, part, P=None, cat=-1):
    n = _nodes(cs)
    return part.evaluate(n, n, cs["P"] if P is None else P, cs["root_freqs"], cat=cat, q_is_probability=True, per_site=True)


def _want(cs, node=None, kind=None, M=None):
    ref = bc.reference(cs, node, M, key=kind if node is not None else "base")
    return ref["site_logl"], ref["logl"]


def _trial_list(cs):
    """[(node, kind, M)]: all six trials of every branch under test, shuffled so that the trials of a branch are not adjacent (six
    rounds, every branch once per round in a fresh order, a round never starting with the branch the round before ended with)."""
    rng = np.random.default_rng(int(cs["seed"]) + 1)
    per = {node: bc.trials(cs, node) for node in cs["branches"]}
    kinds = {node: list(rng.permutation(len(bc.TRIAL_KINDS))) for node in cs["branches"]}
    out = []
    for r in range(len(bc.TRIAL_KINDS)):
        order = [int(b) for b in rng.permutation(cs["branches"])]
        if out and len(order) > 1 and order[0] == out[-1][0]:
            order = order[1:] + order[:1]
        for node in order:
            kind, M = per[node][kinds[node][r]]
            out.append((node, kind, M))
    assert all(a[0] != b[0] for a, b in zip(out, out[1:])) or len(cs["branches"]) == 1
    return out


def _call(part, tl, **kw):
    nodes = np.array([t[0] for t in tl], dtype=np.int64)
    return part.branch_trials(nodes, np.stack([t[2] for t in tl]), q_is_probability=True, per_site=True, **kw)


def _hold_all(cs, what, tl, got, own=None):
    ll, lik, sc = got
    for t, (node, kind, M) in enumerate(tl):
        want = _want(cs, node, kind, M)
        _hold(f"{what} branch {node} {kind}", (float(ll[t]), lik[t], sc[t]), *want)
        if kind in ("identity", "block_zero"):
            assert np.array_equal(lik[t] == 0.0, np.isneginf(want[0])), (what, node, kind)
            assert (ll[t] == -np.inf) == bool(np.isneginf(want[1])), (what, node, kind)
        if kind == "build" and own is not None:
            _hold(f"{what} branch {node} against the partition's own full pass", (float(ll[t]), lik[t], sc[t]), *own)


def _one_call(cs, part, what):
    first = _full(cs, part)
    _hold(f"{what} full pass [{part.prune_kernel_name()}]", first, *_want(cs))
    tl = _trial_list(cs)
    got = _call(part, tl)
    _hold_all(cs, what, tl, got, own=(_site(first[1], first[2]), first[0]))
    return tl, got


# ---- 1, 2 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_every_trial_of_every_case_in_one_call(name, monkeypatch):
    """2 .. 64 states (every row-block count), stars, two-child roots, the three-leaf tree, the 300 / 600-taxon ladders, the conflict
    trees at 1e-15 / 1e-30; the full-coverage cases also make the call a second time: identical bits."""
    _env(monkeypatch)
    cs = CASES[name]
    with _mk(cs) as part:
        tl, got = _one_call(cs, part, name)
        if name in FULL or name.startswith("bigladder"):
            again = _call(part, tl)
            for a, b in zip(got, again):
                assert a.tobytes() == b.tobytes(), name


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------

def test_four_states(monkeypatch):
    _env(monkeypatch)
    cs = bc._make(**D4)
    assert len(cs["branches"]) == 30
    with _mk(cs) as part:
        tl, got = _one_call(cs, part, "bal2x4_D4")
        again = _call(part, tl)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()
        _left_behind(cs, part, "bal2x4_D4")


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------

def _left_behind(cs, part, what):
    none = np.zeros(0, dtype=np.int64)
    one = np.array([cs["branches"][len(cs["branches"]) // 2]], dtype=np.int64)
    base = _want(cs)
    _hold(f"{what}: partial update after the call", part.evaluate(_path(cs, one[0]), none, None, cs["root_freqs"], per_site=True), *base)
    for k in range(2):
        _hold(f"{what}: full pass {k} after the call", part.evaluate(_nodes(cs), none, None, cs["root_freqs"], per_site=True), *base)


FORMS = {"lazy": dict(HYPHY_HIP_REPEATS="0"),
         "workgroup": dict(HYPHY_HIP_KERNEL="0", HYPHY_HIP_REPEATS="0"),
         "wave": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REPEATS="0"),
         "team": dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0"),
         "reroot": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0")}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", FULL)
def test_nothing_is_left_behind(name, form, monkeypatch):
    """After the call a partial update that passes no matrix, full passes with none and a branch cache built before the call give
    the base point.  "lazy": the call follows two full passes, the second of which kept its conditionals on chip; "reroot": the
    schedule is a re-rooted one where the tree has another rooting (the persisted copies on the path belong to that rooting)."""
    from hyphy_amd import hip
    _env(monkeypatch, FORMS[form])
    cs = CASES[name]
    rerooted = form == "reroot" and len(hip.plan_reroot(cs["flat_parents"], int(cs["L"]))) > 1
    tl = _trial_list(cs)[: 2 * len(cs["branches"])]
    cached = int(cs["branches"][len(cs["branches"]) // 3])
    with _mk(cs) as part:
        _hold(f"{name} {form} full pass", _full(cs, part), *_want(cs))
        if form in ("lazy", "reroot"):
            _hold(f"{name} {form} second full pass", _full(cs, part), *_want(cs))
            if rerooted:
                assert "re-rooted" in part.schedule_info(), part.schedule_info()
        else:
            part.branch_cache_build(cached)
        _hold_all(cs, f"{name} {form}", tl, _call(part, tl))
        if form not in ("lazy", "reroot"):
            kind, M = bc.trials(cs, cached)[3]
            got = part.branch_cache_evaluate(cached, M, q_is_probability=True, per_site=True)
            _hold(f"{name} {form} the cache built before the call", got, *_want(cs, cached, kind, M))
            ch = np.array([cached], dtype=np.int64)
            got = part.evaluate(_path(cs, cached), ch, cs["P"][ch], cs["root_freqs"], q_is_probability=True, per_site=True)
            _hold(f"{name} {form} branch {cached} put back", got, *_want(cs))
        _left_behind(cs, part, f"{name} {form}")


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", bc.class_cases(), ids=lambda c: c["name"])
def test_rate_classes(cs, monkeypatch):
    """Three classes (off-diagonals 1e-2, 1e-12, 1e-30), every class with its own trial matrix, against scalefree.prune with the
    branch replaced in every class and the case's weights."""
    from hyphy_amd import hip
    _env(monkeypatch)
    w = cs["weights"]
    with _mk(cs, C=3) as part:
        for c in range(3):
            ref = bc.reference(cs, key="base", cls=c)
            _hold(f"{cs['name']} class {c} pass", _full(cs, part, cs["P"][c], cat=c), ref["site_logl"], ref["logl"])
        per = {node: [bc.trials(cs, node, c) for c in range(3)] for node in cs["branches"]}
        tl = [(node, k) for k in range(len(bc.TRIAL_KINDS)) for node in cs["branches"]]
        nodes = np.array([t[0] for t in tl], dtype=np.int64)
        Ms = np.stack([np.stack([per[node][c][k][1] for c in range(3)]) for node, k in tl])
        with pytest.raises(hip.HipError):
            part.branch_trials(nodes, Ms, q_is_probability=True)
        ll, lik, sc = part.branch_trials(nodes, Ms, weights=w, q_is_probability=True, per_site=True)
        for t, (node, k) in enumerate(tl):
            P = cs["P"].copy()
            P[:, node] = Ms[t]
            ref = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, cs["root_freqs"],
                           weights=w)
            _hold(f"{cs['name']} branch {node} {bc.TRIAL_KINDS[k]}", (float(ll[t]), lik[t], sc[t]), ref["site_logl"], ref["logl"])
        again = part.branch_trials(nodes, Ms, weights=w, q_is_probability=True, per_site=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((ll, lik, sc), again))


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------

def test_class_compressed_partition(monkeypatch):
    """Trials on a leaf branch, on a branch inside a compressed subtree and on a trunk branch of a partition that runs class-compressed;
    the next ordinary evaluation equals the reference and still runs compressed."""
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"))
    fx = common.compressible_case(61, 7)
    D, L = int(fx["D"]), int(fx["L"])
    fp = np.asarray(fx["flat_parents"], dtype=np.int64)
    I = len(fp) - L
    nodes = common.all_nodes(fx)
    pi = fx["root_freqs"]
    rng = np.random.default_rng(61)
    _, comp, _ = hip.plan_repeats(fp, L, fx["leaf_codes"], 0.35)
    inside = [c for c in range(len(fp) - 1) if comp[fp[c]]]
    trunk = [L + i for i in range(I - 1) if not comp[i]]
    assert inside and trunk, (comp, "the case has no compressed subtree or no trunk branch")
    picks = [0, inside[len(inside) // 2], trunk[0]]

    def ref(P):
        return sf.prune(D, fp, L, fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], P, pi)
    with _mk(fx) as part:
        for _ in range(3):
            part.evaluate(nodes, nodes, fx["Q"], pi)
        P = hip.expm_batch(fx["Q"])
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        name = part.prune_kernel_name()
        tr = [(b, M) for b in picks for M in (sf.ordinary(rng, 1, D)[0], P[b], sf.near_identity(rng, 1, D, 1e-7)[0])]
        ll, lik, sc = part.branch_trials(np.array([t[0] for t in tr]), np.stack([t[1] for t in tr]), q_is_probability=True, per_site=True)
        for t, (b, M) in enumerate(tr):
            P2 = P.copy()
            P2[b] = M
            r = ref(P2)
            _hold(f"compressed partition branch {b} trial {t}", (float(ll[t]), lik[t], sc[t]), r["site_logl"], r["logl"])
        r = ref(P)
        none = np.zeros(0, dtype=np.int64)
        _hold("compressed partition: the next evaluation", part.evaluate(nodes, none, None, pi, per_site=True), r["site_logl"], r["logl"])
        _hold("compressed partition: the one after", part.evaluate(nodes, none, None, pi, per_site=True), r["site_logl"], r["logl"])
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        assert part.prune_kernel_name() == name


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [4, 5])
def test_chunks_of_tiles(depth, monkeypatch):
    """S = 70 (five tiles) at 33 states with a 1 MB budget for the outside vectors against the unchunked call: identical bits.  On
    the 16-taxon tree of the wide case 1 MB still holds all five tiles (30 branches x 6 144 bytes a tile: 5.7 tiles), so the chunked
    walk is asserted on the 32-taxon tree (62 branches: 2.7 tiles, chunks of 2, 2 and 1); the 16-taxon one runs beside it."""
    _env(monkeypatch)
    D = 33
    cs = bc._make(name=f"wide_bal2x{depth}_D{D}", shape="wide", D=D, seed=7410 + depth, tree=sf.balanced_tree(2, depth), S=70)
    B = len(cs["flat_parents"]) - 1
    tile_bytes = B * 16 * 48 * 8                            # one tile of V over every branch (48 = 33 states padded to row blocks)
    tiles = (70 + 15) // 16
    assert tiles == 5
    if depth == 5:
        assert (1 << 20) // tile_bytes < tiles, (tile_bytes, tiles)
    cs["branches"] = [int(b) for b in np.random.default_rng(depth).choice(B, size=12, replace=False)]
    with _mk(cs) as part:
        tl, whole = _one_call(cs, part, cs["name"])
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", "1")
        chunked = _call(part, tl)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        for a, b in zip(whole, chunked):
            assert a.tobytes() == b.tobytes()


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
    with _mk(cs, C=3) as part:
        for c in range(3):
            ref = bc.reference(cs, key="base", cls=c)
            _hold(f"{cs['name']} class {c} pass", _full(cs, part, cs["P"][c], cat=c), ref["site_logl"], ref["logl"])
        per = {node: [bc.trials(cs, node, c) for c in range(3)] for node in cs["branches"]}
        tl = [(node, k) for k in range(len(bc.TRIAL_KINDS)) for node in cs["branches"]]
        nodes = np.array([t[0] for t in tl], dtype=np.int64)
        Ms = np.stack([np.stack([per[node][c][k][1] for c in range(3)]) for node, k in tl])
        whole = part.branch_trials(nodes, Ms, weights=w, q_is_probability=True, per_site=True)
        for t, (node, k) in enumerate(tl):
            P = cs["P"].copy()
            P[:, node] = Ms[t]
            ref = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, cs["root_freqs"],
                           weights=w)
            _hold(f"{cs['name']} branch {node} {bc.TRIAL_KINDS[k]}", (float(whole[0][t]), whole[1][t], whole[2][t]),
                  ref["site_logl"], ref["logl"])
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", mb)
        chunked = part.branch_trials(nodes, Ms, weights=w, q_is_probability=True, per_site=True)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        for a, b in zip(whole, chunked):
            assert a.tobytes() == b.tobytes()


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bal2x4_D5", "bal2x4_D33", "bal2x4_D61", "bal2x4_D4"])
def test_rate_matrices_and_templates(name, monkeypatch):
    """Rate matrices as trials against the same call given expm_batch of them; coefficient rows over templates against the dense
    form of the same rate matrices."""
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = CASES[name] if name in CASES else bc._make(**D4)
    D, L = int(cs["D"]), int(cs["L"])
    rng = np.random.default_rng(int(cs["seed"]))
    nodes = np.array([1, L + 8, 5, 1, L + 2], dtype=np.int64)
    Q = common.random_rates(rng, len(nodes), D)
    Q[3] *= 8.0                                            # (past the first squaring)
    K = 3
    T = rng.random((K, D, D)) + 0.05
    T[:, np.arange(D), np.arange(D)] = 0.0
    co = rng.uniform(0.002, 0.02, size=(len(nodes), K))
    Qt = np.einsum("nk,kij->nij", co, T)
    Qt[:, np.arange(D), np.arange(D)] = -Qt.sum(axis=2)
    with _mk(cs) as part:
        _hold(f"{name} full pass", _full(cs, part), *_want(cs))
        ll, lik, sc = part.branch_trials(nodes, hip.expm_batch(Q), q_is_probability=True, per_site=True)
        direct = part.branch_trials(nodes, Q, per_site=True)
        for t in range(len(nodes)):
            _hold(f"{name} trial {t}: rate matrix", (float(direct[0][t]), direct[1][t], direct[2][t]), _site(lik[t], sc[t]), float(ll[t]))
        part.set_q_templates(T)
        built = part.branch_trials_built(nodes, co, per_site=True)
        ll, lik, sc = part.branch_trials(nodes, Qt, per_site=True)
        for t in range(len(nodes)):
            _hold(f"{name} trial {t}: templates", (float(built[0][t]), built[1][t], built[2][t]), _site(lik[t], sc[t]), float(ll[t]))
        assert np.array_equal(part.branch_trials(nodes, Qt), ll)                     # (without the per-pattern outputs)
        _left_behind(cs, part, name)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_partition_usable(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = CASES["bal2x4_D17"]
    B = len(cs["flat_parents"]) - 1
    M = np.stack([cs["P"][0]])
    base = _want(cs)
    with _mk(cs) as part:
        with pytest.raises(hip.HipError):                  # nothing evaluated yet
            part.branch_trials([0], M, q_is_probability=True)
        _hold("first pass", _full(cs, part), *base)
        for bad in (B, B + 1, -1):                         # the root's code, past it, negative
            with pytest.raises(hip.HipError):
                part.branch_trials([0, bad], np.stack([cs["P"][0]] * 2), q_is_probability=True)
            _hold(f"after node code {bad}", _full(cs, part), *base)
        part.set_pinned_states(3, np.zeros(int(cs["leaf_codes"].shape[1]), dtype=np.int64))
        with pytest.raises(hip.HipError):
            part.branch_trials([0], M, q_is_probability=True)
        part.set_pinned_states(None)
        _hold("after the pin", _full(cs, part), *base)
        bad_q = np.full((1, 17, 17), np.nan)
        with pytest.raises(hip.HipError):                  # cannot be exponentiated
            part.branch_trials([0], bad_q)
        _hold("after the bad rate matrix", _full(cs, part), *base)
        assert part._lib.hyphy_hip_branch_trials(part._h, 0, None, None, 1, None, None, None, None) == 0
        got = part.branch_trials([0], M, q_is_probability=True, per_site=True)
        _hold("a trial after the errors", (float(got[0][0]), got[1][0], got[2][0]), *base)
    with _mk(cs, C=3) as part:                             # a class not yet evaluated
        _full(cs, part, cat=0)
        _full(cs, part, cat=1)
        with pytest.raises(hip.HipError):
            part.branch_trials([0], np.stack([np.stack([cs["P"][0]] * 3)]), weights=np.array([0.2, 0.3, 0.5]), q_is_probability=True)
        ref = bc.reference(cs, key="base")
        _hold("class 2 after the refusal", _full(cs, part, cat=2), ref["site_logl"], ref["logl"])
