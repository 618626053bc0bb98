"""hyphy_hip_simulate against tests/simulate_ref.py.

Exact tier: the matrices go in as transition matrices (q_is_probability=True: the device's images are copies of the host's), so the
cumulative rows are the same bits on both sides and the assertion is equality of every byte, under caller-supplied uniforms and under
the device's Philox, with and without the internal nodes.  Through the device's exponential (tests/simulate_cases.py): the reference
draws on P from tests/expm_ref.py; columns the reference itself marks as near-ties are left out, at most 1e-3 of them.
Distribution: chi^2 of the simulated leaf patterns against the device's own per-pattern likelihoods."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import simulate_cases as sc
from tests import simulate_ref as mr
from tests.test_gpu_joint import BAL8, POLY12, _random_P, make_case

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, dtype=np.int64)
TOP = 1.0 - 2.0 ** -53
SLICE = 2048            # simulate.hip: kSlice, the columns of a workgroup


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


def _rows(cs):
    return len(cs["flat_parents"])


def _same(got, want, what):
    assert got.dtype == np.int8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def _full(cs, part):
    part.evaluate(_nodes(cs), _nodes(cs), cs["P"], cs["root_freqs"], q_is_probability=True)


def _hold(cs, part, n_rep, n_sites, seed, what, P=None, cls=None, root=None):
    """Supplied uniforms and Philox, with and without the internal nodes, against the reference; returns the Philox draw."""
    L, P = int(cs["L"]), cs["P"] if P is None else P
    u = np.random.default_rng(seed).random((n_rep, _rows(cs), n_sites))
    want = mr.simulate_ref(cs["flat_parents"], L, P, cs["root_freqs"], u, cls, root)
    _same(part.simulate(n_rep, n_sites, cls, root, uniforms=u, with_internal=True), want, what + " supplied, with internal")
    _same(part.simulate(n_rep, n_sites, cls, root, uniforms=u), want[:, :L], what + " supplied")
    want = mr.simulate_ref(cs["flat_parents"], L, P, cs["root_freqs"], mr.uniforms(seed, n_rep, _rows(cs), n_sites), cls, root)
    got = part.simulate(n_rep, n_sites, cls, root, seed=seed, with_internal=True)
    _same(got, want, what + " philox, with internal")
    _same(part.simulate(n_rep, n_sites, cls, root, seed=seed), want[:, :L], what + " philox")
    return got


# ---- 1. exact tier -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_sites", [1, 15, 257, SLICE + 7])
@pytest.mark.parametrize("D", [2, 4, 5, 16, 17, 20, 32, 33, 48, 49, 61, 64])
def test_every_state_count_and_slice_shape(D, n_sites, monkeypatch):
    """Every row-block count, exact and padded, and the 4-state path; one column, a partial wave, more than one pass of a workgroup
    over its slice, more than one workgroup; the 8-leaf balanced tree and the 12-leaf tree with a 3- and a 5-way node."""
    _env(monkeypatch)
    for k, tree in enumerate((BAL8, POLY12)):
        cs = make_case(D, tree, 5, 1000 * D + n_sites + k)
        with _mk(cs) as part:
            _full(cs, part)
            for n_rep in (1, 3):
                got = _hold(cs, part, n_rep, n_sites, 7 * D + n_sites + n_rep, f"D{D} n{n_sites} tree{k} R{n_rep}")
                assert got.min() >= 0 and got.max() < D


# ---- 2. through the device's exponential -------------------------------------------------------------------------------------------

def _hold_near(got, want, near, what):
    differ = (got != want).any(axis=1)
    print(what, "columns", near.size, "left out", int(near.sum()), "differ", int(differ.sum()), "differ outside", int((differ & ~near).sum()))
    assert got.dtype == np.int8 and got.shape == want.shape and got.min() >= 0, what
    assert near.sum() <= sc.MAX_LEFT_OUT * near.size, what
    bad = np.argwhere(differ & ~near)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())


def _sim(part):
    return part.simulate(sc.EXPM_R, sc.EXPM_SITES, seed=sc.EXPM_SEED, with_internal=True)


@pytest.mark.parametrize("name", sorted(sc.EXPM_CASES))
def test_rate_matrices_through_the_exponential(name, monkeypatch):
    """61 and 64 states on a 40-leaf caterpillar (the exponential leaves a leaf's branch with the column-gather image only and an
    internal branch with the A-operand image only), 4 states on a 120-leaf caterpillar."""
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = sc.expm_case(name)
    want, near = sc.expm_reference(name)
    with _mk(cs) as part:
        part.evaluate(_nodes(cs), _nodes(cs), cs["Q"], cs["root_freqs"])
        if cs["D"] > 48:
            assert hip.last_expm_kernel().startswith("expm64_kernel")
        _hold_near(_sim(part), want, near, name)


@pytest.mark.parametrize("form", ["templates", "mixture", "reroot", "partial", "branch_cache_leaf", "branch_cache_internal"])
def test_behind_every_form_of_pass(form, monkeypatch):
    """61 states: evaluate_built (rate matrices formed on the device from templates), evaluate_mixture (P = sum_m w_m exp(Q_m)), a
    re-rooted schedule, a partial update that changes three matrices, and branch_cache_evaluate, whose new matrix is the one that is
    simulated."""
    from hyphy_amd import tree
    env = dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0") if form == "reroot" else {}
    _env(monkeypatch, env)
    name = "cat40_D61"
    cs = sc.expm_case(name)
    nodes, pi, L = _nodes(cs), cs["root_freqs"], int(cs["L"])
    want, near = sc.expm_reference(name)
    with _mk(cs) as part:
        if form == "templates":
            part.set_q_templates(cs["T"])
            part.build_q(cs["coeffs"])
            part.evaluate_built(nodes, nodes, pi)
        elif form == "mixture":
            comp, w, P = sc.mixture_of(name)
            part.evaluate_mixture(nodes, nodes, comp, w, pi)
            want, near = sc.reference(cs, P)
        elif form == "reroot":
            seen = False
            for _ in range(3):
                part.evaluate(nodes, nodes, cs["Q"], pi)
                seen = seen or "re-rooted" in part.schedule_info()
            assert seen, part.schedule_info()
        elif form == "partial":
            part.evaluate(nodes, nodes, cs["Q"], pi)
            b = np.array([3, L + 5, L + 20], dtype=np.int64)
            Q2, P2 = sc.changed(cs, b, 17)
            flat = tree.flat_from_parents(cs["flat_parents"], L)
            un = np.unique(np.concatenate([flat.path_update_nodes(int(x)) for x in b]))
            part.evaluate(un, b, Q2[b], pi)
            want, near = sc.reference(cs, P2)
        else:
            part.evaluate(nodes, nodes, cs["Q"], pi)
            b = 5 if form == "branch_cache_leaf" else L + 7
            Q2, P2 = sc.changed(cs, np.array([b]), 23 + b)
            part.branch_cache_build(b)
            part.branch_cache_evaluate(b, Q2[b])
            want, near = sc.reference(cs, P2)
            assert (want != sc.expm_reference(name)[0]).any()           # the new matrix draws other states than the old one
        _hold_near(_sim(part), want, near, form)


def test_behind_a_class_compressed_pass(monkeypatch):
    """HYPHY_HIP_REPEATS=1 at 61 states: the pass computes class tables, the matrix images are what a plain pass leaves."""
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"))
    fx = common.compressible_case(61, 7)
    nodes = common.all_nodes(fx)
    cs = dict(fx, P=sc.reference_P(fx["Q"]))
    want, near = sc.reference(cs, cs["P"])
    with _mk(cs) as part:
        part.set_repeats(True)
        for _ in range(3):
            before = part.evaluate(nodes, nodes, fx["Q"], fx["root_freqs"])
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        _hold_near(_sim(part), want, near, "class-compressed")
        assert part.evaluate(nodes, nodes, fx["Q"], fx["root_freqs"]) == before
        assert part.repeat_stats()["in_use"] == 1


# ---- 3. degenerate cases and classes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["identity", "zero_block", "u_zero", "u_top", "negative", "root_states"])
def test_degenerate_cases(kind, monkeypatch):
    """Identity matrices on every branch (every node equals the root); a block of exact zeros (rows without a positive total: -1, and
    -1 below), then zero root frequencies (-1 everywhere); u == 0 and u = 1 - 2^-53 supplied for every draw; entries of -1e-17 (the
    running sum dips: the search over the running maximum gives the plain scan's state); root states supplied."""
    _env(monkeypatch)
    for D in (4, 20, 61):
        cs = make_case(D, POLY12, 5, 77 + D)
        L, rows, n = int(cs["L"]), _rows(cs), 300
        rng = np.random.default_rng(D)
        if kind == "identity":
            cs["P"][:] = np.eye(D)
        elif kind == "zero_block":
            cs["P"][L + 1, D // 2:, :] = 0.0          # internal node 1 below a parent in the upper half of the states: no total
            cs["P"][4, 0, :] = 0.0                    # leaf 4 below a parent in state 0
        elif kind == "negative":
            cs["P"][rng.random(cs["P"].shape) < 0.3] = -1e-17
            cs["P"][:, :, 0] = -1e-17
            cs["root_freqs"][[0, 2]] = -1e-17
        with _mk(cs) as part:
            _full(cs, part)
            if kind in ("u_zero", "u_top"):
                u = np.full((2, rows, n), 0.0 if kind == "u_zero" else TOP)
                got = part.simulate(2, n, uniforms=u, with_internal=True)
                _same(got, mr.simulate_ref(cs["flat_parents"], L, cs["P"], cs["root_freqs"], u), f"{kind} D{D}")
                assert (got == (0 if kind == "u_zero" else D - 1)).all()      # every entry of P and pi is positive
                continue
            root = rng.integers(0, D, size=(3, n)) if kind == "root_states" else None
            got = _hold(cs, part, 3, n, 5 + D, f"{kind} D{D}", root=root)
            if kind == "identity":
                assert (got == got[:, -1:, :]).all() and got.min() >= 0
            elif kind == "root_states":
                assert np.array_equal(got[:, -1], root) and got.min() >= 0
            elif kind == "negative":
                assert got.min() >= 0
            else:
                fp = cs["flat_parents"]
                dead = got < 0
                assert dead.any() and not dead.all() and not dead[:, -1].any()
                for node in range(rows - 1):
                    assert (dead[:, node] >= dead[:, L + fp[node]]).all(), node      # -1 propagates to every descendant
                assert np.array_equal(dead[:, L + 1], got[:, L + fp[L + 1]] >= D // 2)
                assert np.array_equal(dead[:, 4] & ~dead[:, L + fp[4]], got[:, L + fp[4]] == 0)
                part.evaluate(NONE, NONE, np.zeros((0, D, D)), np.zeros(D))          # root frequencies without a positive total
                assert (part.simulate(2, 50, seed=1, with_internal=True) == -1).all()


@pytest.mark.parametrize("D", [4, 20, 61])
def test_rate_classes(D, monkeypatch):
    """C = 3, the class of each column drawn from {0, 2}: classes mix inside every slice; class 1 is used by no column and was never
    evaluated; referring to it is an error."""
    from hyphy_amd import hip
    _env(monkeypatch)
    rng = np.random.default_rng(300 + D)
    cs = make_case(D, POLY12, 5, 40 + D)
    B = _rows(cs) - 1
    P = np.stack([_random_P(rng, B, D) for _ in range(3)])
    n = SLICE + 300
    cls = rng.choice([0, 2], size=(3, n)).astype(np.int64)
    with _mk(cs, C=3) as part:
        for c in (0, 2):
            part.evaluate(_nodes(cs), _nodes(cs), P[c], cs["root_freqs"], cat=c, q_is_probability=True)
        _hold(cs, part, 3, n, 11 + D, f"classes D{D}", P=P, cls=cls)
        _hold(cs, part, 2, 70, 12 + D, f"classes D{D}: all in class 2", P=P, cls=np.full((2, 70), 2, dtype=np.int64))
        _hold(cs, part, 2, 70, 13 + D, f"classes D{D}: root states", P=P, cls=cls[:2, :70], root=rng.integers(0, D, size=(2, 70)))
        cls[1, 5] = 1
        with pytest.raises(hip.HipError, match="not been evaluated"):
            part.simulate(3, n, cls)


def test_refusals_leave_the_partition_usable(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = make_case(17, BAL8, 5, 1717)
    nodes, rows, L = _nodes(cs), _rows(cs), int(cs["L"])
    out = np.zeros((1, rows, 33), dtype=np.int8)
    po = out.ctypes.data_as(C.POINTER(C.c_int8))
    lib = hip.load()
    assert lib.hyphy_hip_simulate(None, 1, 33, None, None, 0, None, 1, po) < 0                       # NULL partition
    with _mk(cs) as part:
        with pytest.raises(hip.HipError, match="not been evaluated"):                                # nothing evaluated yet
            part.simulate(1, 33)
        base = part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True)
        assert lib.hyphy_hip_simulate(part._h, 1, 33, None, None, 0, None, 1, None) < 0              # NULL output
        for n_rep, n_sites in ((-1, 33), (1, -1), (2 ** 31, 33), (1, 2 ** 31)):                      # negative / above 2^31 - 1
            assert lib.hyphy_hip_simulate(part._h, n_rep, n_sites, None, None, 0, None, 1, po) < 0, (n_rep, n_sites)
        for wrong in (1, -1):                                                                         # C == 1: a class other than 0
            cls = np.zeros((1, 33), dtype=np.int64)
            cls[0, 7] = wrong
            with pytest.raises(hip.HipError, match="out of range"):
                part.simulate(1, 33, cls)
        for wrong in (1.0, -1e-300, np.nan, 2.0):
            u = np.full((1, rows, 33), 0.5)
            u[0, 2, 7] = wrong
            with pytest.raises(hip.HipError, match=r"outside \[0, 1\)"):
                part.simulate(1, 33, uniforms=u)
        for wrong in (17, -1):
            root = np.zeros((1, 33), dtype=np.int64)
            root[0, 32] = wrong
            with pytest.raises(hip.HipError, match="root state"):
                part.simulate(1, 33, root_states=root)
        assert part.simulate(0, 33).shape == (0, L, 33)                                              # n_rep == 0: nothing written
        assert part.simulate(2, 0, with_internal=True).shape == (2, rows, 0)
        canary = np.full((1, rows, 33), 77, dtype=np.int8)
        pc = canary.ctypes.data_as(C.POINTER(C.c_int8))
        assert lib.hyphy_hip_simulate(part._h, 0, 33, None, None, 0, None, 1, pc) == 0 and (canary == 77).all()
        assert lib.hyphy_hip_simulate(part._h, 1, 0, None, None, 0, None, 1, pc) == 0 and (canary == 77).all()
        assert part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True) == base
        _hold(cs, part, 2, 33, 4, "after the refusals")
    with _mk(cs, C=3) as part:
        part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], cat=0, q_is_probability=True)
        for wrong in (3, -1):
            cls = np.zeros((1, 33), dtype=np.int64)
            cls[0, 7] = wrong
            with pytest.raises(hip.HipError, match="out of range"):
                part.simulate(1, 33, cls)


# ---- 4. chunking -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 61])
def test_chunks_give_the_same_bytes(D, monkeypatch):
    """HYPHY_HIP_SIMULATE_MB for two whole replicates per chunk (5 replicates: a short last chunk), then for 100 columns (site ranges
    of one replicate, a short last range), then for 7 columns; below one column (a small call): one column per chunk.  Two classes,
    so the columns of every chunk are sorted by class."""
    _env(monkeypatch)
    rng = np.random.default_rng(D)
    cs = make_case(D, BAL8, 5, 500 + D)
    rows, n, R = _rows(cs), 330, 5
    P = np.stack([_random_P(rng, rows - 1, D) for _ in range(2)])
    cls = rng.integers(0, 2, size=(R, n))
    root = rng.integers(0, D, size=(R, n))
    u = rng.random((R, rows, n))
    with _mk(cs, C=2) as part:
        for c in (0, 1):
            part.evaluate(_nodes(cs), _nodes(cs), P[c], cs["root_freqs"], cat=c, q_is_probability=True)

        def calls(columns):
            """(Philox, supplied uniforms, supplied without the internal nodes, root states) under a budget of ``columns``."""
            out = []
            for kw, per_col in ((dict(seed=9, with_internal=True), rows), (dict(uniforms=u, with_internal=True), 9 * rows),
                                (dict(uniforms=u), 9 * rows), (dict(seed=9, root_states=root), rows)):
                if columns is None:
                    monkeypatch.delenv("HYPHY_HIP_SIMULATE_MB", raising=False)
                else:
                    monkeypatch.setenv("HYPHY_HIP_SIMULATE_MB", repr(columns * per_col / 1048576.0))
                out.append(part.simulate(R, n, cls, **kw))
            return out
        whole = calls(None)
        assert np.array_equal(whole[1][:, :int(cs["L"])], whole[2]) and whole[0].min() >= 0
        _same(whole[1], mr.simulate_ref(cs["flat_parents"], cs["L"], P, cs["root_freqs"], u, cls), "unchunked")
        for columns in (2.5 * n, 100.5, 7.5):
            for a, b in zip(whole, calls(columns)):
                assert np.array_equal(a, b), columns
        monkeypatch.setenv("HYPHY_HIP_SIMULATE_MB", repr(0.5 * rows / 1048576.0))
        small = part.simulate(2, 9, cls[:2, :9], seed=9, with_internal=True)
        monkeypatch.delenv("HYPHY_HIP_SIMULATE_MB")
        _same(small, whole[0][:2, :, :9], "one column per chunk")


# ---- 5. no state left ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 61])
def test_no_state_left_behind_and_determinism(D, monkeypatch):
    """evaluate -> simulate -> partial update -> full pass equals, bit for bit, the same sequence without the call; the device memory
    the partition reports and the name of the last exponential kernel are unchanged; two identical calls give identical arrays; the
    call works with a pin active."""
    from hyphy_amd import hip, tree
    _env(monkeypatch, dict(HYPHY_HIP_CUT="levels"))
    cs = make_case(D, POLY12, 70, 500 + D)
    nodes, L = _nodes(cs), int(cs["L"])
    b = 13
    un = tree.flat_from_parents(cs["flat_parents"], L).path_update_nodes(b)
    P2 = _random_P(np.random.default_rng(D), 1, D)

    def sequence(with_call):
        out = []
        with _mk(cs) as part:
            out.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True, per_site=True))
            out.append(part.evaluate(nodes, NONE, None, cs["root_freqs"], per_site=True))       # (a lazy full pass)
            if with_call:
                mem, kern = part.schedule_info(), hip.last_expm_kernel()
                a = part.simulate(3, 500, seed=5, with_internal=True)
                assert np.array_equal(a, part.simulate(3, 500, seed=5, with_internal=True))
                assert not np.array_equal(a, part.simulate(3, 500, seed=6, with_internal=True))
                assert part.schedule_info() == mem and hip.last_expm_kernel() == kern
                assert "device memory" in mem
                part.set_pinned_states(3, np.zeros(70, dtype=np.int64))
                assert np.array_equal(a, part.simulate(3, 500, seed=5, with_internal=True))      # with a pin active
                part.set_pinned_states(None)
            out.append(part.evaluate(nodes, NONE, None, cs["root_freqs"], per_site=True))
            out.append(part.evaluate(un, np.array([b]), P2, cs["root_freqs"], q_is_probability=True, per_site=True))
            out.append(part.evaluate(nodes, NONE, None, cs["root_freqs"], per_site=True))
        return out
    for x, y in zip(sequence(False), sequence(True)):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


@pytest.mark.parametrize("D", [20, 61])
def test_between_a_branch_cache_build_and_its_evaluations(D, monkeypatch):
    """(The 4-state path has no branch cache.)  A branch cache built before the call still evaluates to the same bits."""
    _env(monkeypatch)
    cs = make_case(D, POLY12, 70, 500 + D)
    nodes = _nodes(cs)
    b = 13
    P2 = _random_P(np.random.default_rng(D), 1, D)[0]

    def sequence(with_call):
        out = []
        with _mk(cs) as part:
            out.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True))
            part.branch_cache_build(b)
            if with_call:
                _hold(cs, part, 2, 100, D, f"branch cache built D{D}")
            out.append(part.branch_cache_evaluate(b, cs["P"][b], q_is_probability=True))
            out.append(part.branch_cache_evaluate(b, P2, q_is_probability=True))
            if with_call:                                             # the device keeps the trial matrix: it is the one simulated
                Pn = cs["P"].copy()
                Pn[b] = P2
                _hold(cs, part, 2, 100, D, f"branch cache evaluated D{D}", P=Pn)
            out.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True))
        return out
    assert sequence(False) == sequence(True)


# ---- 6. distribution ----------------------------------------------------------------------------------------------------------------

def test_leaf_patterns_follow_the_device_likelihoods(monkeypatch):
    """The 3-leaf, 4-state case of tests/test_simulate_cpu.py through rate matrices, on a partition that holds all 64 patterns: Pearson
    chi^2 of the 200 000 simulated leaf patterns against the device's own per-pattern likelihoods (2^64 exponents applied), 63
    degrees of freedom, bound 132 (the 1 - 1e-6 quantile).  Deterministic: Philox fixes the draws."""
    _env(monkeypatch)
    Q, pi = mr.dist_case()
    a, b, c = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    codes = np.stack([a.reshape(-1), b.reshape(-1), c.reshape(-1)])                 # pattern 16 a + 4 b + c
    cs = dict(D=4, L=mr.DIST_L, flat_parents=mr.DIST_FP, leaf_codes=codes, ambig=None, pattern_freq=np.ones(64, dtype=np.int64))
    with _mk(cs) as part:
        _, lik, cnt = part.evaluate(np.arange(4), np.arange(4), Q, pi, per_site=True)
        states = part.simulate(1, mr.DIST_COLUMNS, seed=sc.DIST_SEED)
    prob = np.ldexp(lik, (-64 * cnt).astype(np.int64))
    assert abs(prob.sum() - 1.0) < 1e-9 and states.shape == (1, 3, mr.DIST_COLUMNS)
    chi2 = mr.chi2_of_leaves(states, prob)
    print("chi2", chi2)
    assert chi2 < mr.CHI2_BOUND


# ---- 7. round trip ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 61])
def test_simulated_alignment_evaluates(D, monkeypatch):
    """simulate -> data.from_states -> a new partition -> evaluate: a finite log-likelihood, above that of uniform random data."""
    from hyphy_amd import data, hip
    _env(monkeypatch)
    cs = make_case(D, POLY12, 5, 900 + D)
    nodes = _nodes(cs)
    with _mk(cs) as part:
        _full(cs, part)
        sim = part.simulate(1, 400, seed=3)[0]
    assert sim.shape == (12, 400) and sim.min() >= 0
    lls = []
    for states in (sim, np.random.default_rng(D).integers(0, D, size=(12, 400))):
        pd = data.from_states(states, D)
        assert pd.pattern_freq.sum() == 400
        with hip.HipPartition(D, cs["flat_parents"], 12, pd.leaf_codes, None, pd.pattern_freq) as part:
            lls.append(part.evaluate(nodes, nodes, cs["P"], cs["root_freqs"], q_is_probability=True))
    assert np.isfinite(lls[0]) and lls[0] < 0 and lls[0] > lls[1]
