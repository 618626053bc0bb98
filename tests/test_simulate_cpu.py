"""No device: hyphy_hip_simulate_uniforms against the numpy Philox bit for bit, tests/simulate_ref.py on hand-made cases, its
distribution against brute-force pattern probabilities, and the reference's own standing under the near-tie cap that
tests/test_gpu_simulate.py holds the device to."""
import numpy as np
import pytest

from tests import sample_ref as sr
from tests import simulate_cases as sc
from tests import simulate_ref as mr

TOP = 1.0 - 2.0 ** -53


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
    """hyphy_hip_simulate_uniforms (host only) equals the numpy Philox at counter (j, node, r, 1) bit for bit, and differs from
    hyphy_hip_sample_uniforms (counter word 0) under the same seed."""
    got = hip.simulate_uniforms(seed, *shape)
    assert got.shape == shape and 0.0 <= got.min() and got.max() < 1.0
    assert got.tobytes() == mr.uniforms(seed, *shape).tobytes()
    other = hip.sample_uniforms(seed, *shape)
    assert not (got == other).any()
    assert other.tobytes() == sr.uniforms(seed, *shape).tobytes()


def test_library_uniforms_do_not_depend_on_call_splitting(hip):
    seed, R, N, n = 99, 6, 5, 40
    whole = hip.simulate_uniforms(seed, R, N, n)
    assert np.array_equal(hip.simulate_uniforms(seed, 2, N, 13), whole[:2, :, :13])
    assert np.array_equal(hip.simulate_uniforms(seed, R, 3, n), whole[:, :3])
    assert np.array_equal(mr.uniforms(seed, 4, N, 27, sites=np.arange(13, 40), reps=np.arange(2, 6)), whole[2:, :, 13:])
    assert hip.simulate_uniforms(seed, 0, N, n).shape == (0, N, n)
    assert hip.load().hyphy_hip_simulate_uniforms(0, 1, 1, 1, None) < 0
    assert hip.load().hyphy_hip_simulate_uniforms(0, -1, 1, 1, None) < 0
    assert hip.load().hyphy_hip_simulate_uniforms(0, 2 ** 31, 1, 1, None) < 0


def test_simulate_refuses_a_null_partition(hip):
    import ctypes as C
    out = np.zeros(4, dtype=np.int8)
    assert hip.load().hyphy_hip_simulate(None, 1, 1, None, None, 0, None, 0, out.ctypes.data_as(C.POINTER(C.c_int8))) < 0


# ---- simulate_ref on hand-made cases: ((leaf 0, leaf 1) node 0, leaf 2) root; node codes 0, 1, 2, 3 (node 0), 4 (root) --------------
FP3, L3 = mr.DIST_FP, mr.DIST_L


def _rand_u(seed, R, n):
    return np.random.default_rng(seed).random((R, 5, n))


def test_ref_identity_matrices_copy_the_root():
    D = 5
    P = np.broadcast_to(np.eye(D), (4, D, D))
    pi = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    got = mr.simulate_ref(FP3, L3, P, pi, _rand_u(1, 3, 50))
    assert got.shape == (3, 5, 50) and got.min() >= 0 and len(np.unique(got[:, 4])) == D
    assert (got == got[:, 4:5, :]).all()


def test_ref_zero_row_gives_minus_one_and_minus_one_below():
    D = 3
    P = np.broadcast_to(np.eye(D), (4, D, D)).copy()
    P[3, 1] = 0.0                                        # node 0 below a root in state 1: no positive total
    pi = np.array([0.5, 0.5, 0.0])
    got = mr.simulate_ref(FP3, L3, P, pi, _rand_u(2, 2, 40))
    root = got[:, 4]
    assert set(np.unique(root)) == {0, 1}
    dead = root == 1
    assert (got[:, 3][dead] == -1).all() and (got[:, 0][dead] == -1).all() and (got[:, 1][dead] == -1).all()
    assert (got[:, 2][dead] == 1).all()                  # leaf 2 hangs off the root: alive
    assert (got[:, :, :].transpose(0, 2, 1)[~dead] == 0).all()
    assert (mr.simulate_ref(FP3, L3, P, np.zeros(D), _rand_u(2, 2, 40)) == -1).all()       # a -1 root: -1 everywhere
    assert (mr.simulate_ref(FP3, L3, P, np.array([np.nan, 1.0, 0.0]), _rand_u(2, 2, 40)) == -1).all()


def test_ref_u_zero_and_u_top():
    pi = np.array([0.0, 0.25, 0.5, 0.25, 0.0])
    P = np.zeros((4, 5, 5))
    P[:] = np.array([0.0, 0.0, 0.3, 0.7, 0.0])
    lo = mr.simulate_ref(FP3, L3, P, pi, np.zeros((1, 5, 4)))
    hi = mr.simulate_ref(FP3, L3, P, pi, np.full((1, 5, 4), TOP))
    assert (lo[:, 4] == 1).all() and (lo[:, :4] == 2).all()       # u == 0: the first state of positive weight
    assert (hi[:, 4] == 3).all() and (hi[:, :4] == 3).all()       # u just under 1: the last state of positive weight


def test_ref_running_sum_is_the_serial_one():
    e = 2.0 ** -53
    row = np.array([1.0, e, e, e, e, 1.0, e, e])
    st, cum, x, total = mr.draw(row[None], np.array([(1.0 + 2 * e) / 2.0]))
    assert total[0] == 2.0 and st[0] == 5


def test_ref_tiny_negative_entries_same_answer_under_the_running_maximum():
    """Rows with entries of -1e-17 (what an exponential can leave where the true value is 0): the running sum is not monotone;
    the lower-bound search over the running maximum finds the state the plain scan finds, at every u tried, the dips included."""
    rng = np.random.default_rng(5)
    D = 20
    P = rng.random((4, D, D))
    P[rng.random(P.shape) < 0.4] = -1e-17
    P[:, :, 0] = -1e-17                                   # a negative running sum at the start of every row
    P /= P.sum(axis=2, keepdims=True)
    pi = rng.random(D)
    pi[[0, 3, 7]] = -1e-17
    assert (np.diff(np.add.accumulate(P, axis=2), axis=2) < 0).any()
    u = rng.random((4, 5, 3000))
    u[0] = 0.0
    u[1] = TOP
    cum = np.add.accumulate(P[0, 5])                      # ... and u exactly on the sums of one row, dips included
    u[2, :, :D] = np.clip(cum / cum[-1], 0.0, TOP)
    plain = mr.simulate_ref(FP3, L3, P, pi, u)
    assert plain.min() >= 0
    assert np.array_equal(plain, mr.simulate_ref(FP3, L3, P, pi, u, use_max=True))
    row = np.array([-1e-17, 0.5, -1e-17, -1e-17, 0.5])
    for uu, want in ((0.0, 1), (0.25, 1), (0.5, 1), (0.5 + 2.0 ** -53, 4), (TOP, 4)):
        for use_max in (False, True):
            assert mr.draw(row[None], np.array([uu]), use_max)[0][0] == want, (uu, use_max)


def test_ref_root_states_and_classes_are_honoured():
    D = 4
    rng = np.random.default_rng(9)
    P = np.zeros((2, 4, D, D))
    P[0] = np.eye(D)
    P[1] = np.roll(np.eye(D), 1, axis=1)                  # class 1: every edge moves to the next state
    root = rng.integers(0, D, size=(2, 30))
    cls = rng.integers(0, 2, size=(2, 30))
    u = rng.random((2, 5, 30))
    got = mr.simulate_ref(FP3, L3, P, np.array([1.0, 0, 0, 0]), u, class_of_site=cls, root_states=root)
    assert np.array_equal(got[:, 4], root)
    assert np.array_equal(got[:, 2], (root + cls) % D) and np.array_equal(got[:, 0], (root + 2 * cls) % D)
    u2 = u.copy()
    u2[:, 4] = rng.random((2, 30))                        # the root's uniform is unused
    assert np.array_equal(got, mr.simulate_ref(FP3, L3, P, np.array([1.0, 0, 0, 0]), u2, class_of_site=cls, root_states=root))


# ---- distribution ------------------------------------------------------------------------------------------------------------------

def test_reference_leaf_patterns_follow_the_model():
    """3 leaves, 4 states, 200 000 columns under Philox: Pearson chi^2 of the 64 leaf-pattern counts against brute-force pattern
    probabilities, 63 degrees of freedom.  Bound 132 (the 1 - 1e-6 quantile); deterministic: the seed's statistic is 67.20,
    below 92 (the 0.99 quantile)."""
    Q, pi = mr.dist_case()
    P = sc.reference_P(Q)
    prob = mr.pattern_probabilities(P, pi)
    assert abs(prob.sum() - 1.0) < 1e-12 and prob.min() > 1e-5       # every expected count is above 2
    u = mr.uniforms(sc.DIST_SEED, 1, 5, mr.DIST_COLUMNS)
    states = mr.simulate_ref(mr.DIST_FP, mr.DIST_L, P, pi, u)
    chi2 = mr.chi2_of_leaves(states, prob)
    print("chi2", chi2)
    assert chi2 < mr.CHI2_SEED_BOUND < mr.CHI2_BOUND


# ---- the reference under the near-tie cap of the device tests -----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sc.EXPM_CASES))
def test_reference_leaves_out_almost_no_column(name):
    """Expected share of near-tie columns: about (L + I) D 2e-9 (1e-5 at 61 states on the 40-leaf caterpillar), far inside 1e-3."""
    cs = sc.expm_case(name)
    states, near = sc.expm_reference(name)
    print(name, "columns", near.size, "left out", int(near.sum()))
    assert near.size >= 1000 and near.sum() <= sc.MAX_LEFT_OUT * near.size
    assert states.min() >= 0 and states.max() == cs["D"] - 1
