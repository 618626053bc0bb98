"""hyphy_hip_joint_ancestral against tests/joint_ref.py.  The matrices go in as transition matrices (q_is_probability=True: the
device's images are copies, so both sides multiply the same bits) and the assertion is exact equality of every state, -1 included,
with and without the leaves.  The rate-matrix tests at the end compare the probability of the two assignments instead."""
import numpy as np
import pytest

from tests import common
from tests import expm_ref as er
from tests import joint_ref as jr
from tests import scalefree as sf

pytestmark = pytest.mark.gpu

BAL8 = sf.balanced_tree(2, 3)
# 12 leaves: a 3-way node (leaves 0-2), a 5-way node (3-7), a cherry (8, 9), (3-way, 5-way), (cherry, leaf 10), root (.., .., leaf 11)
POLY12 = (np.array([0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 4, 5, 3, 3, 4, 5, 5, -1], dtype=np.int64), 12)
CHERRY = {8: (0, 1), 12: (8, 9)}      # two leaves that form a cherry, by leaf count


def _env(monkeypatch, env=None):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _random_P(rng, B, D):
    """Non-reversible, dense, diagonal-heavy row-stochastic matrices."""
    M = rng.random((B, D, D)) ** 2 + 1e-3
    M[:, np.arange(D), np.arange(D)] += rng.uniform(0.5, 3.0, size=(B, 1)) * D * 0.2
    return M / M.sum(axis=2, keepdims=True)


def make_case(D, tree, S, seed, P=None):
    fp, L = tree
    rng = np.random.default_rng(seed)
    B = len(fp) - 1
    P = _random_P(rng, B, D) if P is None else P
    pi = rng.random(D) + 0.05
    pi /= pi.sum()
    amb = (rng.random((3, D)) < 0.5).astype(np.float64)
    amb[0, :] = 1.0                                       # code -1: fully unresolved
    amb[1:, 0], amb[1:, D - 1] = 1.0, 0.0                 # codes -2, -3: partial
    codes = rng.integers(0, D, size=(L, S))
    for s in range(S):                                    # states, partial codes and unresolved leaves inside every tile
        if s % 4 == 1:
            m = rng.random(L) < 0.3
            codes[m, s] = -rng.integers(1, 4, size=int(m.sum()))
    if S > 2:
        codes[:, 2] = -1                                  # every leaf unresolved: all -1
    if S > 3:
        codes[list(CHERRY[L]), 3] = -1                    # an internal node at -1 below a resolved root
    return dict(D=D, L=L, flat_parents=fp, leaf_codes=codes, ambig=amb, pattern_freq=np.ones(S, dtype=np.int64), root_freqs=pi, P=P)


def _mk(cs, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def _nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def _ref(cs, P=None, cls=None):
    return jr.joint_ref(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["P"] if P is None else P,
                        cs["root_freqs"], class_of_pattern=cls)[0]


def _hold(cs, part, want, what, cls=None):
    I = len(cs["flat_parents"]) - int(cs["L"])
    both = part.joint_ancestral(do_leaves=True, class_of_pattern=cls)
    inner = part.joint_ancestral(do_leaves=False, class_of_pattern=cls)
    assert both.shape == want.shape and inner.shape == (I, want.shape[1]), what
    bad = np.argwhere(both != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), both[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(inner, want[:I]), what
    return both


def _run(cs, what):
    with _mk(cs) as part:
        part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)
        return _hold(cs, part, _ref(cs), what)


@pytest.mark.parametrize("S", [1, 15, 17, 33, 70])
@pytest.mark.parametrize("D", [2, 4, 5, 16, 17, 20, 32, 33, 48, 49, 61, 64])
def test_every_state_count_and_tile_shape(D, S, monkeypatch):
    """Every row-block count, exact and padded; partial tiles and a partial workgroup; the 8-leaf balanced tree and the 12-leaf
    tree with a 3- and a 5-way node; non-reversible P, random pi; states, partial codes and unresolved leaves in one tile; a
    pattern of unresolved leaves only (all -1) and an unresolved cherry (an internal node at -1 below a resolved root)."""
    _env(monkeypatch)
    for k, tree in enumerate((BAL8, POLY12)):
        cs = make_case(D, tree, S, 1000 * D + 10 * S + k)
        got = _run(cs, f"D{D} S{S} tree{k}")
        I = len(tree[0]) - tree[1]
        if S > 3:
            assert np.all(got[:, 2] == -1)
            node = int(tree[0][CHERRY[tree[1]][0]])
            assert got[node, 3] == -1 and got[I - 1, 3] >= 0


@pytest.mark.parametrize("kind", ["identity", "zero_block", "tie"])
def test_degenerate_matrices(kind, monkeypatch):
    """The exact identity on a branch; a block of exact zeros (all-zero rows of products: arg = 0); the all-ties pattern."""
    _env(monkeypatch)
    if kind == "tie":
        D, fp, L, codes, amb, P, pi = jr.tie_case()
        cs = dict(D=D, L=L, flat_parents=fp, leaf_codes=codes, ambig=amb, pattern_freq=np.ones(1, dtype=np.int64), root_freqs=pi, P=P)
        got = _run(cs, kind)
        assert got[:3, 0].tolist() == [0, 0, 0]
        return
    for D in (4, 20):
        cs = make_case(D, BAL8, 33, 77 + D)
        if kind == "identity":
            cs["P"][[1, 9, 12]] = np.eye(D)
        else:
            cs["P"] = sf._block_zero(cs["P"], D)
            cs["leaf_codes"][0, 5] = D - 1                # the isolated state at one leaf only: impossible patterns
        _run(cs, f"{kind} D{D}")


@pytest.mark.parametrize("D,n", [(4, 300), (61, 120)])
def test_ladders(D, n, monkeypatch):
    """Hundreds of factors along one path: without rescaling the products underflow and every comparison fails (state 0)."""
    _env(monkeypatch)
    fp, L = sf.ladder_tree(n)
    rng = np.random.default_rng(n + D)
    B = len(fp) - 1
    S = 20
    codes = sf._patterns(rng, L, D, S, 4)
    amb = np.ones((2, D))
    amb[1, 1:] = rng.random(D - 1) < 0.5
    pi = rng.random(D) + 0.05
    cs = dict(D=D, L=L, flat_parents=fp, leaf_codes=codes, ambig=amb, pattern_freq=np.ones(S, dtype=np.int64), root_freqs=pi / pi.sum(),
              P=sf.ordinary(rng, B, D))
    got = _run(cs, f"ladder D{D} n{n}")
    assert (got > 0).any()


def test_wide_star(monkeypatch):
    _env(monkeypatch)
    D, fp, L, codes, amb, P, pi = jr.wide_star()
    cs = dict(D=D, L=L, flat_parents=fp, leaf_codes=codes, ambig=amb, pattern_freq=np.ones(codes.shape[1], dtype=np.int64), root_freqs=pi, P=P)
    got = _run(cs, "wide star")
    assert got[1].tolist() == [1, 2, 3]


@pytest.mark.parametrize("D", [4, 20, 61])
def test_rate_classes(D, monkeypatch):
    """C = 3, the class of each pattern drawn at random from {0, 2}: classes mix inside every tile; class 1 is used by no pattern
    and was never evaluated."""
    _env(monkeypatch)
    rng = np.random.default_rng(300 + D)
    cs = make_case(D, POLY12, 70, 40 + D)
    B = len(cs["flat_parents"]) - 1
    P = np.stack([_random_P(rng, B, D) for _ in range(3)])
    cls = rng.choice([0, 2], size=70).astype(np.int64)
    with _mk(cs, C=3) as part:
        for c in (0, 2):
            part.evaluate(_nodes(cs), _nodes(cs), P[c], cs["root_freqs"], cat=c, q_is_probability=True)
        _hold(cs, part, _ref(cs, P, cls), f"classes D{D}", cls=cls)
        _hold(cs, part, _ref(cs, P, np.full(70, 2)), f"classes D{D}: all in class 2", cls=np.full(70, 2, dtype=np.int64))


def test_chunks_of_tiles(monkeypatch):
    """40 tiles at 61 states on the 8-leaf tree: 7 x 16 x 64 x 9 bytes = 64 512 bytes of scratch a tile, so 1 MB holds 16 tiles:
    chunks of 16, 16 and 8."""
    _env(monkeypatch)
    cs = make_case(61, BAL8, 640, 4061)
    assert (1 << 20) // (7 * 16 * 64 * 9) == 16
    with _mk(cs) as part:
        part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)
        whole = _hold(cs, part, _ref(cs), "40 tiles")
        monkeypatch.setenv("HYPHY_HIP_JOINT_MB", "1")
        chunked = part.joint_ancestral(do_leaves=True)
        monkeypatch.delenv("HYPHY_HIP_JOINT_MB")
        assert np.array_equal(whole, chunked)


def test_class_compressed_partition(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"))
    fx = common.compressible_case(61, 7)
    nodes = common.all_nodes(fx)
    P = hip.expm_batch(fx["Q"])
    cs = dict(fx, P=P)
    want = _ref(cs)
    with _mk(cs) as part:
        part.set_repeats(True)
        for _ in range(3):
            part.evaluate(nodes, nodes, P, fx["root_freqs"], q_is_probability=True)
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        compressed = _hold(cs, part, want, "class-compressed")
        assert part.repeat_stats()["in_use"] == 1
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    with _mk(cs) as part:
        part.evaluate(nodes, nodes, P, fx["root_freqs"], q_is_probability=True)
        assert np.array_equal(_hold(cs, part, want, "plain"), compressed)


def test_generated_four_state_kernel(monkeypatch):
    _env(monkeypatch, dict(HYPHY_HIP_NUCGEN="2", HYPHY_HIP_REPEATS="0"))
    cs = make_case(4, POLY12, 70, 4004)
    want = _ref(cs)
    with _mk(cs) as part:
        for _ in range(3):
            part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)
        assert part.prune_kernel_name() == "nucgen_kernel"
        generated = _hold(cs, part, want, "generated kernel")
    monkeypatch.setenv("HYPHY_HIP_NUCGEN", "0")
    with _mk(cs) as part:
        part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)
        assert np.array_equal(_hold(cs, part, want, "interpreter"), generated)


@pytest.mark.parametrize("D", [4, 61])
def test_no_state_left_behind_and_determinism(D, monkeypatch):
    """evaluate -> joint -> partial update -> full pass: log-L and per-pattern values equal, bit for bit, the same sequence without
    the joint call; the device memory the partition reports is unchanged; two identical calls give identical arrays."""
    from hyphy_amd import tree
    _env(monkeypatch, dict(HYPHY_HIP_CUT="levels"))
    cs = make_case(D, POLY12, 70, 500 + D)
    nodes = _nodes(cs)
    b = 13
    un = tree.flat_from_parents(cs["flat_parents"], int(cs["L"])).path_update_nodes(b)
    P2 = _random_P(np.random.default_rng(D), 1, D)
    none = np.zeros(0, dtype=np.int64)

    def sequence(with_joint):
        out = []
        with _mk(cs) as part:
            out.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True, per_site=True))
            if with_joint:
                mem = part.schedule_info()
                a = part.joint_ancestral(do_leaves=True)
                assert np.array_equal(a, part.joint_ancestral(do_leaves=True))
                assert part.schedule_info() == mem
                assert "device memory" in mem
            out.append(part.evaluate(un, np.array([b]), P2, cs["root_freqs"], q_is_probability=True, per_site=True))
            out.append(part.evaluate(nodes, none, None, cs["root_freqs"], per_site=True))
        return out
    for x, y in zip(sequence(False), sequence(True)):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


def test_errors_leave_the_partition_usable(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = make_case(17, BAL8, 33, 1717)
    nodes = _nodes(cs)
    with _mk(cs) as part:
        with pytest.raises(hip.HipError):                  # nothing evaluated yet
            part.joint_ancestral()
        base = part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True)
        with pytest.raises(hip.HipError):                  # C == 1: a class other than 0
            part.joint_ancestral(class_of_pattern=np.ones(33, dtype=np.int64))
        part.set_pinned_states(3, np.zeros(33, dtype=np.int64))
        with pytest.raises(hip.HipError, match="pinned"):
            part.joint_ancestral()
        part.set_pinned_states(None)
        assert part._lib.hyphy_hip_joint_ancestral(part._h, 0, None, None) < 0
        assert part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True) == base
        _hold(cs, part, _ref(cs), "after the errors")
    with _mk(cs, C=3) as part:
        part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], cat=0, q_is_probability=True)
        cls = np.zeros(33, dtype=np.int64)
        cls[7] = 1
        with pytest.raises(hip.HipError, match="not been evaluated"):   # referenced, never evaluated
            part.joint_ancestral(class_of_pattern=cls)
        cls[7] = 3
        with pytest.raises(hip.HipError, match="out of range"):
            part.joint_ancestral(class_of_pattern=cls)
        cls[7] = -1
        with pytest.raises(hip.HipError, match="out of range"):
            part.joint_ancestral(class_of_pattern=cls)
        _hold(cs, part, _ref(cs), "class 0 after the refusals", cls=np.zeros(33, dtype=np.int64))


@pytest.mark.parametrize("D", [4, 20])
def test_rate_matrix_path(D, monkeypatch):
    """Dense random reversible Q, branch lengths 0.05 - 0.5, B = 14, q_is_probability=False: the device's exponentials differ from
    the CPU's in the last bits, so a near-tie may fall the other way — the probability of the device's assignment under the CPU's
    matrices (tests/expm_ref.py) must agree with that of joint_ref's assignment under the same matrices to
    4 B 5e-14 / min_entry(P) relative (5e-14: the absolute per-entry guarantee of DESIGN.md §4.2; two assignments of B factors)."""
    _env(monkeypatch)
    rng = np.random.default_rng(9000 + D)
    cs = make_case(D, BAL8, 33, 600 + D)
    B = len(cs["flat_parents"]) - 1
    assert B <= 30
    pi = rng.uniform(0.8, 1.2, size=D)
    pi /= pi.sum()
    cs["root_freqs"] = pi
    R = rng.uniform(0.6, 1.4, size=(D, D))
    R = (R + R.T) / 2
    Q0 = R * pi[None, :]
    Q0[np.arange(D), np.arange(D)] = 0.0
    Q0[np.arange(D), np.arange(D)] = -Q0.sum(axis=1)
    Q0 /= -(pi * np.diag(Q0)).sum()                       # one expected substitution per unit length
    Q = Q0[None] * rng.uniform(0.05, 0.5, size=(B, 1, 1))
    P = np.stack([er.reference(q) for q in Q])
    floor = P.min()
    assert floor >= 1e-3, floor
    bound = 4 * B * 5e-14 / floor
    want = _ref(cs, P)
    with _mk(cs) as part:
        part.evaluate(_nodes(cs), _nodes(cs), Q, pi)
        got = part.joint_ancestral(do_leaves=True)
    args = (D, cs["flat_parents"], cs["L"])
    for s in range(33):
        a = jr.joint_probability(got[:, s], *args, cs["leaf_codes"][:, s], cs["ambig"], P, pi)
        b = jr.joint_probability(want[:, s], *args, cs["leaf_codes"][:, s], cs["ambig"], P, pi)
        pa, pb = np.ldexp(a[0], a[1]), np.ldexp(b[0], b[1])
        assert np.array_equal(got[:, s] < 0, want[:, s] < 0), s
        assert abs(pa - pb) <= bound * pb, (s, pa, pb, bound)
