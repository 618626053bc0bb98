"""hyphy_hip_branch_cache_build / _evaluate held to the scale-free reference (tests/scalefree.py: ``prune`` with the branch's matrix
substituted) at every branch of the cases of tests/branchcache_cases.py: non-reversible matrices and a random pi (a missing
transposition or a misplaced pi shows), 2 .. 64 states (bc_eval_kernel<1..4>, transpose_frag_kernel at one to four row blocks),
tiles that mix coded and ambiguous lanes, ancestor paths up to 38 long and ~600 long, multifurcating and two-child roots, trial
matrices that are the identity or make patterns impossible, and what an ordinary evaluation sees after a line search.

Every comparison is tests/hold.py's ``_hold``: per pattern and total at scalefree.GPU_RTOL x |reference| + 1e-9 (the allowance rests
on the oracle deviation measured in tests/test_branchcache_cpu.py), -inf exactly where the reference has it."""
import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests.hold import _hold, _site

pytestmark = pytest.mark.gpu

CASES = bc.cases_by_name()
FULL = bc.full_coverage_names()
KERNELS = {"workgroup": dict(HYPHY_HIP_KERNEL="0", HYPHY_HIP_REPEATS="0"),
           "wave": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REPEATS="0"),
           "team": dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0"),
           "default": {}}


def _env(monkeypatch, env):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in env.items():
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


def _want(cs, node=None, kind=None, M=None, cls=None):
    ref = bc.reference(cs, node, M, key=kind if node is not None else "base", cls=cls)
    return ref["site_logl"], ref["logl"]


def _put_back(cs, part, node, what):
    """An ordinary partial update with the build-time matrix of ``node`` (the device kept the last trial matrix)."""
    ch = np.array([node], dtype=np.int64)
    got = part.evaluate(_path(cs, node), ch, cs["P"][ch], cs["root_freqs"], q_is_probability=True, per_site=True)
    _hold(f"{what}: branch {node} put back", got, *_want(cs))


def _rerootable(cs):
    """The tree has a re-rooting path (its root is not already the node that minimises its height)."""
    from hyphy_amd import hip
    return len(hip.plan_reroot(cs["flat_parents"], int(cs["L"]))) > 1


def _every_branch(cs, part, what, lazy_passes=0, rerooted=False):
    """One full pass, then for every branch under test a build followed by every trial matrix.  ``lazy_passes`` full passes come
    before every build: the last of them does not store its conditionals (the build has to restore the copies), and with
    ``rerooted`` it ran the re-rooted schedule (the conditionals on the path belong to the other rooting)."""
    first = _full(cs, part)
    _hold(f"{what} full pass [{part.prune_kernel_name()}]", first, *_want(cs))
    own = _site(first[1], first[2])
    for node in cs["branches"]:
        for k in range(lazy_passes):
            _hold(f"{what} lazy full pass {k} before branch {node}", _full(cs, part), *_want(cs))
        if rerooted:
            assert "re-rooted" in part.schedule_info(), part.schedule_info()
        part.branch_cache_build(node)
        for kind, M in bc.trials(cs, node):
            got = part.branch_cache_evaluate(node, M, q_is_probability=True, per_site=True)
            _hold(f"{what} branch {node} {kind}", got, *_want(cs, node, kind, M))
            if kind == "build":
                _hold(f"{what} branch {node} against the partition's own full pass", got, own, first[0])
        _put_back(cs, part, node, what)


# ---- 2a ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["workgroup", "wave", "team"])
@pytest.mark.parametrize("name", FULL)
def test_every_branch_of_the_full_coverage_shapes(name, kernel, monkeypatch):
    _env(monkeypatch, KERNELS[kernel])
    cs = CASES[name]
    with _mk(cs) as part:
        _every_branch(cs, part, f"{name} {kernel}")


@pytest.mark.parametrize("kernel", ["wave", "default"])
@pytest.mark.parametrize("name", [n for n in CASES if n not in FULL and not n.startswith("bigladder")])
def test_every_branch_of_the_other_cases(name, kernel, monkeypatch):
    """The other state counts on the binary tree, stars (leaf pairing with and without an ambiguous sibling), two-child roots seen
    from both children, the three-leaf tree, near-identity conflict trees at 1e-15 and 1e-30."""
    _env(monkeypatch, KERNELS[kernel])
    cs = CASES[name]
    with _mk(cs) as part:
        _every_branch(cs, part, f"{name} {kernel}")


# ---- 2b ---------------------------------------------------------------------------------------------------------------------------

FORMS = {"shards3": dict(HYPHY_HIP_FORCE_SHARDS="3", HYPHY_HIP_REPEATS="0"),
         "tiles1": dict(HYPHY_HIP_TILES="1", HYPHY_HIP_REPEATS="0"), "tiles2": dict(HYPHY_HIP_TILES="2", HYPHY_HIP_REPEATS="0"),
         "tiles3": dict(HYPHY_HIP_TILES="3", HYPHY_HIP_REPEATS="0"), "tiles4": dict(HYPHY_HIP_TILES="4", HYPHY_HIP_REPEATS="0"),
         "reroot-wave": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0"),
         "reroot-team": dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="3", HYPHY_HIP_REPEATS="0"),
         "repeats-0.05": dict(HYPHY_HIP_REPEATS="2", HYPHY_HIP_REP_THETA="0.05"),
         "repeats-0.9": dict(HYPHY_HIP_REPEATS="2", HYPHY_HIP_REP_THETA="0.9"),
         "cache-always": dict(HYPHY_HIP_CACHE="always", HYPHY_HIP_REPEATS="0"),
         "lazy": dict(HYPHY_HIP_REPEATS="0")}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["bal4x3_D33", "bal4x3_D61", "ladder40_D61"])
def test_every_branch_under_every_form(name, form, monkeypatch):
    """Shards, tile counts (leaf pairing on and off), re-rooted schedules, class-compressed partitions, both cache policies.  Under
    the lazy policy and the re-rooted forms two full passes come before every build, the second of which does not store its
    conditionals; under the re-rooted forms that pass is asserted to have run re-rooted (the ladder; the four-way balanced tree
    hangs from its centre already and has no other rooting)."""
    _env(monkeypatch, FORMS[form])
    cs = CASES[name]
    with _mk(cs) as part:
        if form.startswith("repeats"):
            assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        reroot = form.startswith("reroot")
        assert not (reroot and name.startswith("ladder")) or _rerootable(cs)
        _every_branch(cs, part, f"{name} {form}", lazy_passes=2 if form == "lazy" or reroot else 0, rerooted=reroot and _rerootable(cs))


# ---- 2c ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", bc.class_cases(), ids=lambda c: c["name"])
def test_one_cache_per_rate_class(cs, monkeypatch):
    """Classes with off-diagonals 1e-2, 1e-12, 1e-30: class 0 cached at a leaf branch, class 1 at a deep internal branch, class 2 at a
    root child; evaluated in reverse order, then in build order: building one class's cache does not disturb another's."""
    _env(monkeypatch, {})
    with _mk(cs, C=3) as part:
        for c in range(3):
            ref = bc.reference(cs, key="base", cls=c)
            _hold(f"{cs['name']} class {c} pass", _full(cs, part, cs["P"][c], cat=c), ref["site_logl"], ref["logl"])
        for c, node in enumerate(cs["branches"]):
            part.branch_cache_build(node, cat=c)
        for c in (2, 1, 0, 0, 1, 2):
            node = cs["branches"][c]
            for kind, M in bc.trials(cs, node, c):
                got = part.branch_cache_evaluate(node, M, cat=c, q_is_probability=True, per_site=True)
                _hold(f"{cs['name']} class {c} branch {node} {kind}", got, *_want(cs, node, kind, M, cls=c))


# ---- 2d ---------------------------------------------------------------------------------------------------------------------------

def _line_search_nodes(cs):
    """A leaf branch and an internal branch on the re-rooting path (where the tree has one; else the lowest internal node)."""
    from hyphy_amd import hip
    L = int(cs["L"])
    path = hip.plan_reroot(cs["flat_parents"], L)
    return [3, L + (int(path[1]) if len(path) > 1 else 0)]


@pytest.mark.parametrize("form", ["default", "reroot", "repeats"])
@pytest.mark.parametrize("name", ["ladder40_D5", "ladder40_D61", "bal4x3_D33"])
def test_line_search_and_what_follows(name, form, monkeypatch):
    """Six trial matrices in a row on one cache; the device keeps the last one: the ordinary partial update over the branch's path
    with no matrix passed, and two full passes with none, see it; then the cache is gone."""
    from hyphy_amd import hip
    _env(monkeypatch, {"default": {}, "reroot": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0"),
                       "repeats": dict(HYPHY_HIP_REPEATS="2", HYPHY_HIP_REP_THETA="0.9")}[form])
    cs = CASES[name]
    n = _nodes(cs)
    none = np.zeros(0, dtype=np.int64)
    pi = cs["root_freqs"]
    for node in _line_search_nodes(cs):
        what = f"{name} {form} branch {node}"
        with _mk(cs) as part:
            if form == "repeats":
                assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
            _hold(f"{what} full pass", _full(cs, part), *_want(cs))
            part.branch_cache_build(node)
            tr = bc.trials(cs, node)
            for kind, M in tr[4:] + tr[:4]:                      # identity, block_zero, build, near, near, ordinary
                got = part.branch_cache_evaluate(node, M, q_is_probability=True, per_site=True)
                _hold(f"{what} {kind}", got, *_want(cs, node, kind, M))
            last = _want(cs, node, kind, M)
            assert kind == "ordinary"
            _hold(f"{what} partial update after the search", part.evaluate(_path(cs, node), none, None, pi, per_site=True), *last)
            for k in range(2):                                   # (the first stores every node, the second is the lazy one)
                _hold(f"{what} full pass {k} after the search", part.evaluate(n, none, None, pi, per_site=True), *last)
            if form == "reroot" and name.startswith("ladder"):   # (the branch's twin image had to follow the last trial matrix)
                assert "re-rooted" in part.schedule_info(), part.schedule_info()
            with pytest.raises(hip.HipError):
                part.branch_cache_evaluate(node, M, q_is_probability=True)


# ---- 2e ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bal2x4_D5", "bal2x4_D33", "bal2x4_D61"])
def test_rate_matrix_entry(name, monkeypatch):
    """A rate matrix as the trial (the line search's own form) against the same call given expm_batch of it (held to its reference in
    test_gpu_expm.py): non-reversible Q at norms on either side of the first squaring (the scaled matrix is kept at or below 1/4)
    and well past it."""
    from hyphy_amd import hip
    _env(monkeypatch, {})
    cs = CASES[name]
    D, L = int(cs["D"]), int(cs["L"])
    rng = np.random.default_rng(int(cs["seed"]))
    with _mk(cs) as part:
        _hold(f"{name} full pass", _full(cs, part), *_want(cs))
        for node in (1, L + 8):
            part.branch_cache_build(node)
            for norm in (0.2, 0.3, 3.0):
                Q = rng.random((D, D)) + 0.05
                Q[np.arange(D), np.arange(D)] = 0.0
                Q *= 0.5 * norm / Q.sum(axis=1).max()
                Q[np.arange(D), np.arange(D)] = -Q.sum(axis=1)
                direct = part.branch_cache_evaluate(node, Q, q_is_probability=False, per_site=True)
                ll, lik, sc = part.branch_cache_evaluate(node, hip.expm_batch(Q), q_is_probability=True, per_site=True)
                _hold(f"{name} branch {node} rate matrix of norm {norm}", direct, _site(lik, sc), ll)
            _put_back(cs, part, node, name)


# ---- 2f ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["wave", "default"])
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("bigladder")])
def test_big_ladders(name, kernel, monkeypatch):
    """300 and 600 taxa: the child's conditionals and the outside vector both carry non-zero exponents; paths of hundreds of edges."""
    _env(monkeypatch, KERNELS[kernel])
    cs = CASES[name]
    with _mk(cs) as part:
        _every_branch(cs, part, f"{name} {kernel}")


# ---- 1e ---------------------------------------------------------------------------------------------------------------------------

def test_four_states_are_refused_and_the_partition_stays_usable(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch, {})
    cs = bc._make("bal2x4_D4", "bal2x4", 4, 7004)
    ref = bc.reference(cs)
    with _mk(cs) as part:
        _hold("D = 4 full pass", _full(cs, part), ref["site_logl"], ref["logl"])
        for node in (2, int(cs["L"]) + 1):
            with pytest.raises(hip.HipUnsupported):
                part.branch_cache_build(node)
            with pytest.raises(hip.HipError):
                part.branch_cache_evaluate(node, cs["P"][node], q_is_probability=True)
            _hold("D = 4 full pass after the refusal", _full(cs, part), ref["site_logl"], ref["logl"])
            ch = np.array([node], dtype=np.int64)
            got = part.evaluate(_path(cs, node), ch, cs["P"][ch], cs["root_freqs"], q_is_probability=True, per_site=True)
            _hold("D = 4 partial update after the refusal", got, ref["site_logl"], ref["logl"])
