"""No device: the Philox generator of tests/sample_ref.py against known answers, hyphy_hip_sample_uniforms against it bit for bit,
sample_ref on hand-made cases, and the reference's own standing under the bounds tests/test_gpu_sample.py holds the device to."""
import numpy as np
import pytest

from tests import sample_cases as sc
from tests import sample_ref as sr
from tests import scalefree as sf

KNOWN = [  # counter, key -> output (Random123's known-answer vectors for Philox4x32-10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert sr.philox4x32(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64)).tolist() == list(want)
    batch = sr.philox4x32(np.array([k[0] for k in KNOWN], dtype=np.uint64), np.array([k[1] for k in KNOWN], dtype=np.uint64))
    assert batch.tolist() == [list(k[2]) for k in KNOWN]


def test_uniform_from_two_words():
    """u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53 of the block at counter (j, n, r, 0) under key (seed low, seed high)."""
    seed, j, n, r = 0x299f31d0a4093822, 7, 3, 2
    x = sr.philox4x32(np.array([j, n, r, 0], dtype=np.uint64), np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
    want = ((int(x[0]) >> 5) * 2 ** 26 + (int(x[1]) >> 6)) / 2.0 ** 53
    u = sr.uniforms(seed, 3, 4, 8)
    assert u[r, n, j] == want and 0.0 <= u.min() and u.max() < 1.0


@pytest.fixture(scope="module")
def hip():
    """The binding over the built library (built once for this module; no device is touched)."""
    import __graft_entry__ as g
    g.build()
    from hyphy_amd import hip
    return hip


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 1), (2, 5, 33), (5, 11, 70)])
@pytest.mark.parametrize("seed", [0, 1, 0x299f31d0a4093822, 2 ** 64 - 1])
def test_library_uniforms_equal_numpy_philox(hip, shape, seed):
    """hyphy_hip_sample_uniforms (host only) equals the numpy Philox bit for bit."""
    got = hip.sample_uniforms(seed, *shape)
    assert got.shape == shape
    assert got.tobytes() == sr.uniforms(seed, *shape).tobytes()


def test_library_uniforms_do_not_depend_on_call_splitting(hip):
    """A draw depends on (seed, replicate, site, node) only: a smaller call returns the leading block of a larger one, and the
    remaining replicates and sites are what the numpy generator gives at those counters."""
    seed, R, I, n = 99, 6, 5, 40
    whole = hip.sample_uniforms(seed, R, I, n)
    assert np.array_equal(hip.sample_uniforms(seed, 2, I, 13), whole[:2, :, :13])
    assert np.array_equal(hip.sample_uniforms(seed, R, 3, n), whole[:, :3])
    assert np.array_equal(sr.uniforms(seed, 4, I, 27, sites=np.arange(13, 40), reps=np.arange(2, 6)), whole[2:, :, 13:])
    assert hip.sample_uniforms(seed, 0, I, n).shape == (0, I, n)
    assert hip.load().hyphy_hip_sample_uniforms(0, 1, 1, 1, None) < 0
    assert hip.load().hyphy_hip_sample_uniforms(0, -1, 1, 1, None) < 0


# ---- sample_ref on hand-made cases: a cherry below the root, ((leaf 0, leaf 1) node 0, leaf 2) root ----------------------------
FP3, L3 = np.array([0, 0, 1, 1, -1], dtype=np.int64), 3


def _hand(cond0, cond_root, P3, pi, u):
    D = len(pi)
    cond = np.zeros((2, 1, D))
    cond[0, 0], cond[1, 0] = cond0, cond_root
    P = np.zeros((4, D, D))
    P[3] = P3
    return sr.sample_ref(FP3, L3, cond, P, pi, np.asarray(u, dtype=np.float64).reshape(-1, 2, 1))[:, :, 0]


def test_ref_u_zero_picks_the_first_state_of_positive_weight():
    pi = np.array([0.25, 0.25, 0.5])
    P3 = np.array([[0.0, 0.0, 1.0], [0.5, 0.5, 0.0], [0.0, 0.3, 0.7]])
    #                 node 0      root   ->  root weights (0, .25, .5): state 1; node 0 weights P[1] * (1, 1, 1): state 0
    got = _hand([1.0, 1.0, 1.0], [0.0, 1.0, 1.0], P3, pi, [[0.0, 0.0]])
    assert got.tolist() == [[0, 1]]


def test_ref_zero_weight_leading_state_is_never_drawn():
    pi = np.array([0.25, 0.25, 0.5])
    P3 = np.eye(3)
    for u in (0.0, 1e-300, 0.3, 1.0 - 2.0 ** -53):
        got = _hand([0.0, 1.0, 1.0], [0.0, 0.0, 1.0], P3, pi, [[u, u]])
        assert got.tolist() == [[2, 2]], u


def test_ref_u_just_under_one_reaches_the_last_state_of_positive_weight():
    pi = np.array([0.2, 0.3, 0.5, 0.0])
    P3 = np.full((4, 4), 0.25)
    top = 1.0 - 2.0 ** -53
    got = _hand([1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0], P3, pi, [[top, top], [top, 0.0]])
    assert got.tolist() == [[2, 2], [2, 0]]         # columns: node 0, root


def test_ref_impossible_pattern_gives_minus_one_all_the_way_down():
    pi = np.array([0.5, 0.5])
    P3 = np.array([[1.0, 0.0], [0.0, 1.0]])
    assert _hand([1.0, 1.0], [0.0, 0.0], P3, pi, [[0.3, 0.3]]).tolist() == [[-1, -1]]      # the root's total is 0
    assert _hand([1.0, 1.0], [np.nan, 1.0], P3, pi, [[0.3, 0.3]]).tolist() == [[-1, -1]]   # ... or NaN
    assert _hand([0.0, 1.0], [1.0, 0.0], P3, pi, [[0.3, 0.3]]).tolist() == [[-1, 0]]       # node 0 alone: row 0 of P meets (0, 1)


def test_ref_running_sum_is_the_serial_one():
    """cum is the left-to-right sum of the rounded products (no pairwise summation): 1 + 2^-53 + 2^-53 stays 1 serially."""
    e = 2.0 ** -53
    w = np.array([1.0, e, e, e, e, 1.0, e, e])
    got = _hand(np.ones(8), w, np.eye(8), np.ones(8), [[0.0, (1.0 + 2 * e) / 2.0]])
    # total = 2 serially; x = u * 2 = 1 + 2^-52 > cum_4 = 1: the state is 5.  A pairwise sum would find cum_2 = 1 + 2^-52 >= x
    assert got[0, 1] == 5


# ---- the reference under the bounds of the device tests ---------------------------------------------------------------------

def test_reference_passes_the_distribution_bound():
    """sample_ref on scale-free conditionals with the GPU test's seed, against the scale-free marginal posteriors."""
    cs = sc.dist_case()
    ref = sf.case_reference(cs, conditionals=True, posteriors=True)
    I, S = ref["cond"].shape[:2]
    u = sr.uniforms(sc.DIST_SEED, sc.DIST_R, I, S)
    states = sr.sample_ref(cs["flat_parents"], cs["L"], ref["cond"], cs["P"], cs["root_freqs"], u)
    assert states.min() >= 0
    bad = sc.distribution_violations(states, ref["post"], sc.DIST_R)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("name", sorted(sc.SCALEFREE))
def test_reference_leaves_out_almost_no_column(name):
    states, near = sc.scalefree_reference(name)
    print(name, "columns", near.size, "left out", int(near.sum()))
    assert near.size >= 1000
    assert near.sum() <= sc.MAX_LEFT_OUT * near.size
    assert states.min() >= 0 and states.max() > 0
