"""hyphy_hip_sample_ancestral against tests/sample_ref.py.

Exact tier: the matrices go in as transition matrices (q_is_probability=True: the device's images are copies) and the reference runs
on the device's own download_partials(), so both sides see the same bits; the assertion is equality of every byte, no exclusions,
under caller-supplied uniforms and under the device's Philox.  Scale-free tier: rate matrices through the device's exponential,
the reference on the conditionals of tests/scalefree.py; columns the reference itself marks as near-ties (tests/sample_cases.py)
are left out, at most 1e-3 of them.  Distribution: sampled frequencies against marginal_ancestral."""
import numpy as np
import pytest

from tests import common
from tests import sample_cases as sc
from tests import sample_ref as sr
from tests import scalefree as sf
from tests.test_gpu_joint import BAL8, POLY12, _random_P, make_case

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, dtype=np.int64)
TOP = 1.0 - 2.0 ** -53


def _env(monkeypatch, env=None):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _mk(cs, C=1, **kw):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C, **kw)


def _nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def _I(cs):
    return len(cs["flat_parents"]) - int(cs["L"])


def sites_of(S, seed):
    """pattern_of_site: unsorted, with repeats; one pattern owns 300 sites, one pattern (when there are two) owns none."""
    rng = np.random.default_rng(seed)
    heavy = S // 2
    allowed = np.array([s for s in range(S) if s != 0 or S == 1], dtype=np.int64)   # pattern 0 owns no site
    pos = np.r_[np.full(300, heavy, dtype=np.int64), rng.choice(allowed, size=2 * S + 5), allowed]
    rng.shuffle(pos)
    assert (pos == heavy).sum() >= 300 and (S == 1 or not (pos == 0).any()) and (np.diff(pos) < 0).any() == (S > 2)
    return pos


def _want(cs, cond, u, pos=None, cls=None, P=None):
    return sr.sample_ref(cs["flat_parents"], cs["L"], cond, cs["P"] if P is None else P, cs["root_freqs"], u, pos, cls)


def _same(got, want, what):
    assert got.dtype == np.int8 and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def _hold(cs, part, cond, n_rep, pos, seed, what, cls=None, P=None):
    """Both sources of uniforms against the reference on ``cond``; returns the Philox draw."""
    n_sites = cond.shape[-2] if pos is None else len(pos)
    u = np.random.default_rng(seed).random((n_rep, _I(cs), n_sites))
    _same(part.sample_ancestral(n_rep, pos, cls, uniforms=u), _want(cs, cond, u, pos, cls, P), what + " supplied")
    got = part.sample_ancestral(n_rep, pos, cls, seed=seed)
    _same(got, _want(cs, cond, sr.uniforms(seed, n_rep, _I(cs), n_sites), pos, cls, P), what + " philox")
    return got


# ---- 1. exact tier -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 15, 17, 33, 70])
@pytest.mark.parametrize("D", [2, 4, 5, 16, 17, 20, 32, 33, 48, 49, 61, 64])
def test_every_state_count_and_tile_shape(D, S, monkeypatch):
    _env(monkeypatch)
    for k, tree in enumerate((BAL8, POLY12)):
        cs = make_case(D, tree, S, 1000 * D + 10 * S + k)
        pos = sites_of(S, D + S + k)
        with _mk(cs) as part:
            part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)
            cond = part.download_partials()[0]
            for n_rep in (1, 3):
                got = _hold(cs, part, cond, n_rep, pos, 7 * D + S + n_rep, f"D{D} S{S} tree{k} R{n_rep}")
                assert got.min() >= 0 and got.max() < D
            _hold(cs, part, cond, 3, None, D + S, f"D{D} S{S} tree{k} site = pattern")


# ---- 2. degenerate cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["identity", "zero_block", "u_zero", "u_top"])
def test_degenerate_cases(kind, monkeypatch):
    """The exact identity on branches (zero weights on most states); a block of exact zeros making patterns impossible (-1, and
    everything below it -1); u == 0 and u = 1 - 2^-53 supplied for every draw."""
    _env(monkeypatch)
    for D in (4, 20):
        cs = make_case(D, BAL8, 33, 77 + D)
        if kind == "identity":
            cs["P"][[1, 9, 12]] = np.eye(D)
        elif kind == "zero_block":
            cs["P"] = sf._block_zero(cs["P"], D)
            cs["leaf_codes"][0, 5] = D - 1                # the isolated state at one leaf only: an impossible pattern
        pos = sites_of(33, D)
        with _mk(cs) as part:
            part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)
            cond = part.download_partials()[0]
            if kind in ("u_zero", "u_top"):
                u = np.full((2, _I(cs), len(pos)), 0.0 if kind == "u_zero" else TOP)
                got = part.sample_ancestral(2, pos, uniforms=u)
                _same(got, _want(cs, cond, u, pos), f"{kind} D{D}")
                assert got.min() >= 0                      # u == 0 is a state of positive weight, never -1
                if kind == "u_zero":
                    first = (cs["root_freqs"] * cond[-1, pos] > 0).argmax(axis=1)
                    assert np.array_equal(got[0, -1], first)
                continue
            got = _hold(cs, part, cond, 3, pos, 5 + D, f"{kind} D{D}")
            dead = (got < 0).any(axis=1)
            assert np.array_equal(dead, (got < 0).all(axis=1))           # -1 at the root means -1 everywhere below
            if kind == "zero_block":
                assert dead[:, pos == 5].all() and not dead[:, pos != 5].all()
            elif kind == "identity":
                assert not dead.all()


# ---- 3. rate classes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 20, 61])
def test_rate_classes(D, monkeypatch):
    """C = 3, the class of each pattern drawn from {0, 2}: classes mix inside every tile; class 1 is used by no pattern and was
    never evaluated; referring to it is an error."""
    from hyphy_amd import hip
    _env(monkeypatch)
    rng = np.random.default_rng(300 + D)
    cs = make_case(D, POLY12, 70, 40 + D)
    B = len(cs["flat_parents"]) - 1
    P = np.stack([_random_P(rng, B, D) for _ in range(3)])
    cls = rng.choice([0, 2], size=70).astype(np.int64)
    pos = sites_of(70, D)
    with _mk(cs, C=3) as part:
        cond = np.zeros((3, _I(cs), 70, D))
        for c in (0, 2):
            part.evaluate(_nodes(cs), _nodes(cs), P[c], cs["root_freqs"], cat=c, q_is_probability=True)
        for c in (0, 2):
            cond[c] = part.download_partials(c)[0]
        _hold(cs, part, cond, 3, pos, 11 + D, f"classes D{D}", cls=cls, P=P)
        _hold(cs, part, cond, 2, None, 12 + D, f"classes D{D}: all in class 2", cls=np.full(70, 2, dtype=np.int64), P=P)
        cls[pos[0]] = 1
        with pytest.raises(hip.HipError, match="not been evaluated"):
            part.sample_ancestral(1, pos, cls)


# ---- 4. resident conditionals under every form ------------------------------------------------------------------------------------

def _forms_case(D):
    cs = make_case(D, POLY12, 70, 500 + D)
    return cs, _nodes(cs), sites_of(70, 3 * D)


@pytest.mark.parametrize("D", [4, 61])
def test_after_a_lazy_full_pass(D, monkeypatch):
    """A full pass that follows a full pass keeps nothing: the call restores the conditionals first; the evaluation after it
    gives the bits of the one before."""
    _env(monkeypatch)
    cs, nodes, pos = _forms_case(D)
    with _mk(cs) as part:
        part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True)
        before = part.evaluate(nodes, NONE, None, cs["root_freqs"], per_site=True)
        got = part.sample_ancestral(3, pos, seed=D)
        after = part.evaluate(nodes, NONE, None, cs["root_freqs"], per_site=True)
        assert before[0] == after[0] and before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
        cond = part.download_partials()[0]
        _same(got, _want(cs, cond, sr.uniforms(D, 3, _I(cs), len(pos)), pos), f"lazy D{D}")
        _hold(cs, part, cond, 2, pos, 1 + D, f"lazy D{D}, again")


@pytest.mark.parametrize("D", [4, 61])
def test_after_a_partial_update(D, monkeypatch):
    from hyphy_amd import tree
    _env(monkeypatch)
    cs, nodes, pos = _forms_case(D)
    b = 13
    un = tree.flat_from_parents(cs["flat_parents"], int(cs["L"])).path_update_nodes(b)
    P2 = cs["P"].copy()
    P2[b] = _random_P(np.random.default_rng(D), 1, D)[0]
    with _mk(cs) as part:
        part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True)
        before = part.evaluate(un, np.array([b]), P2[b:b + 1], cs["root_freqs"], q_is_probability=True)
        got = part.sample_ancestral(3, pos, seed=D)
        cond = part.download_partials()[0]
        _same(got, _want(cs, cond, sr.uniforms(D, 3, _I(cs), len(pos)), pos, P=P2), f"partial D{D}")
        assert part.evaluate(un, np.array([b]), P2[b:b + 1], cs["root_freqs"], q_is_probability=True) == before


def test_class_compressed_partition(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"))
    fx = common.compressible_case(61, 7)
    nodes = common.all_nodes(fx)
    P = hip.expm_batch(fx["Q"])
    cs = dict(fx, P=P)
    S = fx["leaf_codes"].shape[1]
    pos = sites_of(S, 61)
    with _mk(cs) as part:
        part.set_repeats(True)
        for _ in range(3):
            before = part.evaluate(nodes, nodes, P, fx["root_freqs"], q_is_probability=True)
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        compressed = part.sample_ancestral(2, pos, seed=61)
        assert part.evaluate(nodes, nodes, P, fx["root_freqs"], q_is_probability=True) == before
        assert part.repeat_stats()["in_use"] == 1
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    with _mk(cs) as part:
        part.evaluate(nodes, nodes, P, fx["root_freqs"], q_is_probability=True)
        cond = part.download_partials()[0]
        plain = part.sample_ancestral(2, pos, seed=61)
    _same(plain, _want(cs, cond, sr.uniforms(61, 2, _I(cs), len(pos)), pos), "plain")
    _same(compressed, plain, "class-compressed")


@pytest.mark.parametrize("D", [20, 61])
def test_after_a_branch_cache_build(D, monkeypatch):
    """(The 4-state path has no branch cache.)  The call between a branch-cache build and its evaluations changes neither: the sequence with the call equals, bit for bit,
    the sequence without it."""
    _env(monkeypatch)
    cs, nodes, pos = _forms_case(D)
    b = 13
    P2 = _random_P(np.random.default_rng(D), 1, D)[0]

    def sequence(with_call):
        out = []
        with _mk(cs) as part:
            out.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True))
            part.branch_cache_build(b)
            if with_call:
                got = part.sample_ancestral(3, pos, seed=D)
                cond = part.download_partials()[0]
                _same(got, _want(cs, cond, sr.uniforms(D, 3, _I(cs), len(pos)), pos), f"branch cache D{D}")
            out.append(part.branch_cache_evaluate(b, cs["P"][b], q_is_probability=True))
            out.append(part.branch_cache_evaluate(b, P2, q_is_probability=True))
            out.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True))
        return out
    assert sequence(False) == sequence(True)


# ---- 5. chunking -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 61])
def test_smallest_chunks_give_the_same_bytes(D, monkeypatch):
    """HYPHY_HIP_SAMPLE_MB below one tile x one replicate: one tile and one replicate per launch."""
    _env(monkeypatch)
    cs, nodes, pos = _forms_case(D)
    u = np.random.default_rng(D).random((3, _I(cs), len(pos)))
    with _mk(cs) as part:
        part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True)
        whole = part.sample_ancestral(3, pos, seed=9), part.sample_ancestral(3, pos, uniforms=u)
        monkeypatch.setenv("HYPHY_HIP_SAMPLE_MB", "0.000001")
        small = part.sample_ancestral(3, pos, seed=9), part.sample_ancestral(3, pos, uniforms=u)
        monkeypatch.setenv("HYPHY_HIP_SAMPLE_MB", "0.01")     # whole replicates of some tiles / a few replicates of every tile
        mid = part.sample_ancestral(3, pos, seed=9), part.sample_ancestral(3, pos, uniforms=u)
        monkeypatch.delenv("HYPHY_HIP_SAMPLE_MB")
    for a, b, c in zip(whole, small, mid):
        assert a.min() >= 0 and np.array_equal(a, b) and np.array_equal(a, c)


# ---- 6. scale-free tier -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sc.SCALEFREE))
def test_scale_free_tier(name, monkeypatch):
    _env(monkeypatch)
    cs, P, cond, R, seed = sc.scalefree_case(name)
    want, near = sc.scalefree_reference(name)
    with _mk(cs) as part:
        part.evaluate(_nodes(cs), _nodes(cs), cs["Q"], cs["root_freqs"])
        assert np.abs(part.download_partials()[1]).max() > 0          # the 2^64 rule has fired: rescaling bites here
        got = part.sample_ancestral(R, seed=seed)
    differ = (got != want).any(axis=1)
    print(name, "columns", near.size, "left out", int(near.sum()), "differ", int(differ.sum()), "differ outside", int((differ & ~near).sum()))
    assert near.sum() <= sc.MAX_LEFT_OUT * near.size
    bad = np.argwhere(differ & ~near)
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


# ---- 7. distribution ----------------------------------------------------------------------------------------------------------------

def test_sampled_frequencies_match_the_marginal_posteriors(monkeypatch):
    """D = 20, BAL8, S = 8, R = 4096: |f - p| <= 5 sqrt(p (1 - p) / R) + 2 / R for every internal node, pattern and state, p from
    marginal_ancestral.  Deterministic: Philox fixes the draws."""
    _env(monkeypatch)
    cs = sc.dist_case()
    with _mk(cs) as part:
        part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)
        post = part.marginal_ancestral()
        states = part.sample_ancestral(sc.DIST_R, seed=sc.DIST_SEED)
    assert states.min() >= 0
    bad = sc.distribution_violations(states, post, sc.DIST_R)
    assert not bad, (len(bad), bad[:5])


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_partition_usable(monkeypatch):
    import ctypes as C
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = make_case(17, BAL8, 33, 1717)
    nodes = _nodes(cs)
    I = _I(cs)
    out = np.zeros((1, I, 33), dtype=np.int8)
    po = out.ctypes.data_as(C.POINTER(C.c_int8))
    assert hip.load().hyphy_hip_sample_ancestral(None, 1, 33, None, None, 0, None, po) < 0          # NULL partition
    with _mk(cs) as part:
        with pytest.raises(hip.HipError, match="not been evaluated"):                                # nothing evaluated yet
            part.sample_ancestral(1)
        base = part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True)
        cond = part.download_partials()[0]
        assert part._lib.hyphy_hip_sample_ancestral(part._h, 1, 33, None, None, 0, None, None) < 0   # NULL output
        with pytest.raises(hip.HipError, match="out of range"):                                      # C == 1: a class other than 0
            part.sample_ancestral(1, class_of_pattern=np.ones(33, dtype=np.int64))
        for wrong in (33, -1):
            with pytest.raises(hip.HipError, match="out of range"):
                part.sample_ancestral(1, pattern_of_site=np.array([0, wrong, 2]))
        assert part._lib.hyphy_hip_sample_ancestral(part._h, 1, 32, None, None, 0, None, po) < 0     # no map: n_sites must be S
        part.set_pinned_states(3, np.zeros(33, dtype=np.int64))
        with pytest.raises(hip.HipError, match="pinned"):
            part.sample_ancestral(1)
        part.set_pinned_states(None)
        for wrong in (1.0, -1e-300, np.nan, 2.0):
            u = np.full((1, I, 33), 0.5)
            u[0, 2, 7] = wrong
            with pytest.raises(hip.HipError, match=r"outside \[0, 1\)"):
                part.sample_ancestral(1, uniforms=u)
        assert part.sample_ancestral(0).shape == (0, I, 33)                                          # n_rep == 0: nothing written
        assert part.sample_ancestral(2, pattern_of_site=NONE).shape == (2, I, 0)
        canary = np.full((1, I, 33), 77, dtype=np.int8)
        assert part._lib.hyphy_hip_sample_ancestral(part._h, 0, 33, None, None, 0, None, canary.ctypes.data_as(C.POINTER(C.c_int8))) == 0
        assert (canary == 77).all()
        assert part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True) == base
        _hold(cs, part, cond, 2, sites_of(33, 1), 4, "after the errors")
    with _mk(cs, C=3) as part:
        part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], cat=0, q_is_probability=True)
        cls = np.zeros(33, dtype=np.int64)
        for wrong in (3, -1):
            cls[7] = wrong
            with pytest.raises(hip.HipError, match="out of range"):
                part.sample_ancestral(1, class_of_pattern=cls)


@pytest.mark.parametrize("D", [4, 61])
def test_no_state_left_behind_and_determinism(D, monkeypatch):
    """evaluate -> sample -> partial update -> full pass equals, bit for bit, the same sequence without the call; the device memory
    the partition reports and the name of the last exponential kernel are unchanged; two identical calls give identical arrays."""
    from hyphy_amd import hip, tree
    _env(monkeypatch, dict(HYPHY_HIP_CUT="levels"))
    cs, nodes, pos = _forms_case(D)
    b = 13
    un = tree.flat_from_parents(cs["flat_parents"], int(cs["L"])).path_update_nodes(b)
    P2 = _random_P(np.random.default_rng(D), 1, D)

    def sequence(with_call):
        out = []
        with _mk(cs) as part:
            out.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True, per_site=True))
            if with_call:
                mem, kern = part.schedule_info(), hip.last_expm_kernel()
                a = part.sample_ancestral(3, pos, seed=5)
                assert np.array_equal(a, part.sample_ancestral(3, pos, seed=5))
                assert not np.array_equal(a, part.sample_ancestral(3, pos, seed=6))
                assert part.schedule_info() == mem and hip.last_expm_kernel() == kern
                assert "device memory" in mem
            out.append(part.evaluate(un, np.array([b]), P2, cs["root_freqs"], q_is_probability=True, per_site=True))
            out.append(part.evaluate(nodes, NONE, None, cs["root_freqs"], per_site=True))
        return out
    for x, y in zip(sequence(False), sequence(True)):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


def test_two_shards_equal_one(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    if hip.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    cs, nodes, pos = _forms_case(61)
    got = []
    for n_dev in (1, 2):
        with _mk(cs, device_count=n_dev) as part:
            part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True)
            got.append(part.sample_ancestral(3, pos, seed=3))
    assert np.array_equal(got[0], got[1])
