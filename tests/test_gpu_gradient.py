"""hyphy_hip_branch_sensitivities / _gradient / _gradient_built and hyphy_hip_expm_frechet_adjoint_batch held to tests/grad_cases.py.

W: componentwise |dW_ij| <= (GPU_RTOL + S 2^-53) W_ref,ij + 1e-280, exact zeros where the reference has them.
The adjoint: per entry ALLOW_PLAIN / ALLOW_SQUARED (grad_cases) times max |W|.  The device's measured worst case over the stand-alone
cases: 6.1e-16 max |W| without squarings and 6.3e-14 with (the float64 model's own 4.15e-16 and 6.30e-14: the device lies within
3e-15 max |W| of the model everywhere).
S and the coefficient gradient: the adjoint's allowance plus W's share, L(Q^T, allow_W), chained by sum_{i != j} |T_k,ij| (a_ij + a_ii)."""
import os

import numpy as np
import pytest

from tests import branchcache_cases as bc
from tests import common
from tests import deriv_cases as dc
from tests import grad_cases as gc
from tests import scalefree as sf

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, dtype=np.int64)


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


def _full(cs, part, P=None, cat=-1):
    n = _nodes(cs)
    return part.evaluate(n, n, cs["P"] if P is None else P, cs["root_freqs"], cat=cat, q_is_probability=True, per_site=True)


def _classes(cs, part):
    for c in range(len(cs["P"])):
        _full(cs, part, cs["P"][c], cat=c)


def _hold_w(cs, what, nodes, got, outs=None, weights=None):
    W, sk = got
    outs = gc.outs_of(cs) if outs is None else outs
    worst = 0.0
    for t, node in enumerate(nodes):
        ref = gc.sensitivities(cs, outs, int(node), weights)
        m = gc.miss_w(W[t], ref)
        worst = max(worst, m)
        assert m <= 1.0, (what, int(node), m)
        assert int(sk[t]) == ref["n_skipped"], (what, int(node), int(sk[t]), ref["n_skipped"])
    print(f"{what}: {len(nodes)} branches, largest deviation / allowance = {worst:.3g}")
    return worst


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the stand-alone adjoint --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 5, 16, 17, 48, 49, 61, 64])
def test_adjoint_batch(D):
    from hyphy_amd import hip
    gold = None
    if D in gc.GOLDEN_D:
        gold = np.load(os.path.join(os.path.dirname(__file__), "golden", f"frechet_adjoint_D{D}.npz"))["S"]
    worst = {False: 0.0, True: 0.0}
    for i, (kind, Q, W) in enumerate(gc.adjoint_cases(D)):
        got = hip.expm_frechet_adjoint_batch(Q, W)
        assert got.tobytes() == hip.expm_frechet_adjoint_batch(Q, W).tobytes(), (D, kind)
        if kind == "zero":
            assert np.array_equal(got, W), (D, kind)
        for k in range(len(Q)):
            want = gold[i][k] if gold is not None else gc.frechet_ref(Q[k], W[k])
            dev = float(np.max(np.abs(got[k] - want)))
            sq = gc.squarings(Q[k]) > 0
            worst[sq] = max(worst[sq], dev / float(np.abs(W[k]).max()))
            assert dev <= gc.adjoint_allowance(Q[k], W[k]), (D, kind, k, dev, gc.adjoint_allowance(Q[k], W[k]))
        assert np.array_equal(hip.expm_frechet_adjoint_batch(Q[0], W[0]), got[0])            # (a single matrix)
    print(f"D = {D}: largest deviation in units of max |W|: no squaring {worst[False]:.3g}, squarings {worst[True]:.3g}")


def test_adjoint_batch_refuses_and_flags():
    from hyphy_amd import hip
    Q = gc.adjoint_cases(5)[3][1].copy()
    W = gc.adjoint_cases(5)[3][2]
    Q[1, 2, 3] = np.nan
    got = hip.expm_frechet_adjoint_batch(Q, W)
    assert np.all(np.isnan(got[1])) and not np.isnan(got[0]).any() and not np.isnan(got[2]).any()
    Q[1] = gc.adjoint_cases(5)[3][1][1] * 1e14                                               # a norm beyond 2^40
    assert np.all(np.isnan(hip.expm_frechet_adjoint_batch(Q, W)[1]))
    with pytest.raises(hip.HipError):
        hip.expm_frechet_adjoint_batch(np.zeros((1, 65, 65)), np.zeros((1, 65, 65)))


# ---- branch_sensitivities -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 5, 20, 48, 49, 61, 64])
def test_sensitivities_every_branch(D, monkeypatch):
    """The 16-taxon tree, S = 40 (three tiles, the last padded), two leaves with ambiguity codes, a pattern of frequency 0, exact
    zeros in the matrices; odd D: three patterns impossible at build time (skipped)."""
    _env(monkeypatch)
    cs = gc.bal_case(D)
    with _mk(cs) as part:
        _full(cs, part)
        got = part.branch_sensitivities(_nodes(cs))
        _hold_w(cs, cs["name"], _nodes(cs), got)
        assert np.all(got[1] == (3 if D % 2 else 0))
        assert _same(got, part.branch_sensitivities(_nodes(cs)))
        rep = part.branch_sensitivities(np.array([5, 2, 5], dtype=np.int64))                  # any order, repeats
        _hold_w(cs, cs["name"] + " (5, 2, 5)", [5, 2, 5], rep)
        assert np.array_equal(rep[0][0], rep[0][2])


def test_sensitivities_star_node(monkeypatch):
    _env(monkeypatch)
    cs = gc.star_case(20)
    with _mk(cs) as part:
        _full(cs, part)
        _hold_w(cs, cs["name"], _nodes(cs), part.branch_sensitivities(_nodes(cs)))


def test_sensitivities_rate_classes(monkeypatch):
    """The 40-taxon three-class ladder (the exponents live in in_c), under the case's weights, with a weight of 0, with all the
    weight on one class."""
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = dc.ladder_class_case()
    nodes = np.array(cs["branches"], dtype=np.int64)
    with _mk(cs, C=3) as part:
        _classes(cs, part)
        with pytest.raises(hip.HipError):
            part.branch_sensitivities(nodes)
        for w in (cs["weights"], np.array([0.6, 0.0, 0.4]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])):
            got = part.branch_sensitivities(nodes, weights=w)
            _hold_w(cs, f"{cs['name']} weights {list(w)}", nodes, got, weights=w)
            assert _same(got, part.branch_sensitivities(nodes, weights=w))
            for c in np.flatnonzero(w == 0):
                assert np.all(got[0][:, c] == 0.0)


def test_sensitivities_impossible_patterns(monkeypatch):
    """A pattern impossible under one class only (that class contributes nothing there, the rest is unaffected) and, at 61 states,
    three impossible under all (skipped, the rest unaffected)."""
    _env(monkeypatch)
    cs = dict(bc.class_cases()[0])
    D, leaf = int(cs["D"]), 0
    P, codes = np.array(cs["P"]), np.array(cs["leaf_codes"])
    P[1, :2] = sf._block_zero(P[1, :2], D)                # class 1: the cut-off state cannot change along the branches of leaves 0 and 1
    codes[0, 3], codes[1, 3] = D - 1, 0                   # ... and pattern 3 asks for it at leaf 0 alone of that cherry
    cs["P"], cs["leaf_codes"], cs["name"] = P, codes, cs["name"] + "_one_class_shut"
    outs = gc.outs_of(cs)
    l0 = [(outs[c][leaf][0] * outs[c][leaf][1]).sum(axis=1) for c in range(3)]
    assert l0[1][3] == 0 and np.sum(l0[1] == 0) == 1 and np.all(l0[0] != 0) and np.all(l0[2] != 0)
    nodes = np.array(cs["branches"] + [leaf], dtype=np.int64)
    with _mk(cs, C=3) as part:
        _classes(cs, part)
        got = part.branch_sensitivities(nodes, weights=cs["weights"])
        _hold_w(cs, cs["name"], nodes, got, weights=cs["weights"])
        assert np.all(got[1] == 0)
    cs = dict(bc.class_cases()[1])                         # 61 states: the same pattern shut under every class
    D = int(cs["D"])
    P, codes = np.array(cs["P"]), np.array(cs["leaf_codes"])
    P[:, :2] = np.stack([sf._block_zero(P[c, :2], D) for c in range(3)])
    codes[0, 3], codes[1, 3] = D - 1, 0
    cs["P"], cs["leaf_codes"], cs["name"] = P, codes, cs["name"] + "_every_class_shut"
    nodes = np.array(cs["branches"] + [0], dtype=np.int64)
    shut = gc.sensitivities(cs, gc.outs_of(cs), 0, cs["weights"])["n_skipped"]
    assert shut == 3                                       # (pattern 3 and the case's own patterns 5 and 21, which put the state at leaf 0)
    with _mk(cs, C=3) as part:
        _classes(cs, part)
        got = part.branch_sensitivities(nodes, weights=cs["weights"])
        _hold_w(cs, cs["name"], nodes, got, weights=cs["weights"])
        assert np.all(got[1] == shut)


FORMS = {"lazy": dict(HYPHY_HIP_REPEATS="0"),
         "reroot": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0")}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["bal2x4_D61", "ladder40_D33", "bal4x3_D5"])
def test_behind_a_lazy_and_a_rerooted_pass(name, form, monkeypatch):
    _env(monkeypatch, FORMS[form])
    cs = bc.cases_by_name()[name]
    nodes = np.array(cs["branches"], dtype=np.int64)
    with _mk(cs) as part:
        first = [_full(cs, part) for _ in range(2)][-1]
        _hold_w(cs, f"{name} {form}", nodes, part.branch_sensitivities(nodes))
        again = part.evaluate(_nodes(cs), NONE, None, cs["root_freqs"], per_site=True)
        assert again[0] == first[0] and again[1].tobytes() == first[1].tobytes()


def test_class_compressed_partition(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"))
    fx = common.compressible_case(61, 7)
    L = int(fx["L"])
    fp = np.asarray(fx["flat_parents"], dtype=np.int64)
    nodes = common.all_nodes(fx)
    _, comp, _ = hip.plan_repeats(fp, L, fx["leaf_codes"], 0.35)
    inside = [c for c in range(len(fp) - 1) if comp[fp[c]]]
    trunk = [L + i for i in range(len(fp) - L - 1) if not comp[i]]
    with _mk(fx) as part:
        for _ in range(3):
            part.evaluate(nodes, nodes, fx["Q"], fx["root_freqs"])
        assert part.repeat_stats()["in_use"] == 1
        cs = dict(fx, name="grad_compressible_61_7", seed=61007, P=hip.expm_batch(fx["Q"]))
        req = np.array([0, inside[len(inside) // 2], trunk[0]], dtype=np.int64)
        _hold_w(cs, "class-compressed partition", req, part.branch_sensitivities(req), outs=[gc.outside(cs)])
        part.evaluate(nodes, NONE, None, fx["root_freqs"])
        part.evaluate(nodes, NONE, None, fx["root_freqs"])
        assert part.repeat_stats()["in_use"] == 1


@pytest.mark.parametrize("D", [17, 4])
def test_behind_a_mixture_pass(D, monkeypatch):
    """The resident matrix is a two-component mixture sum_m w_m exp(Q_m): branch_sensitivities is exact for it."""
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = gc.bal_case(D)
    B = len(cs["flat_parents"]) - 1
    rng = np.random.default_rng(int(cs["seed"]) + 5)
    Qm = common.random_rates(rng, 2 * B, D).reshape(B, 2, D, D)
    wm = rng.dirichlet([2.0, 2.0], size=B)
    with _mk(cs) as part:
        mixed = dict(cs, name=cs["name"] + "_mixture", P=np.einsum("bm,bmij->bij", wm, hip.expm_batch(Qm.reshape(2 * B, D, D)).reshape(B, 2, D, D)))
        part.evaluate_mixture(_nodes(cs), _nodes(cs), Qm, wm, cs["root_freqs"])
        _hold_w(mixed, mixed["name"], _nodes(cs)[::3], part.branch_sensitivities(_nodes(cs)[::3]), outs=[gc.outside(mixed)])


def test_two_shards(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    if hip.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    cs = gc.bal_case(20, 70)
    with _mk(cs, device_count=2) as part:
        _full(cs, part)
        got = part.branch_sensitivities(_nodes(cs))
        _hold_w(cs, cs["name"] + " on two shards", _nodes(cs), got)
        assert _same(got, part.branch_sensitivities(_nodes(cs)))


# ---- segments and chunks ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,S,budgets", [(17, 1040, ("1", "4.5")), (4, 1100, ("0.1",))], ids=["D17", "D4"])
def test_segments_and_chunks(D, S, budgets, monkeypatch):
    """Three segments of 512 patterns (65 tiles of 16; 18 waves of 64 at 4 states).  17 states, 30 branches x 4 096 bytes a tile: a
    1 MB budget gives chunks of 8 tiles (nine chunks, every segment continued across chunks), 4.5 MB gives 38, cut to 32 at the
    segment boundary (three chunks); 4 states, 30 branches x 2 048 bytes a wave under 0.1 MB: a wave a chunk.  Same allowances as the
    unchunked call; two identical calls give identical bytes."""
    _env(monkeypatch)
    cs = gc.bal_case(D, S)
    B = len(cs["flat_parents"]) - 1
    if D == 17:
        assert (S + 15) // 16 == 65 and (1 << 20) // (B * 16 * 32 * 8) == 8 and int(4.5 * (1 << 20)) // (B * 16 * 32 * 8) == 38
    else:
        assert (S + 63) // 64 == 18 and int(0.1 * (1 << 20)) // (B * 256 * 8) == 1
    nodes = _nodes(cs)[::2]
    with _mk(cs) as part:
        _full(cs, part)
        whole = part.branch_sensitivities(nodes)
        _hold_w(cs, cs["name"], nodes, whole)
        assert _same(whole, part.branch_sensitivities(nodes))
        for mb in budgets:
            monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", mb)
            chunked = part.branch_sensitivities(nodes)
            again = part.branch_sensitivities(nodes)
            monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
            _hold_w(cs, f"{cs['name']} under {mb} MB", nodes, chunked)
            assert _same(chunked, again)


def test_rate_classes_in_chunks(monkeypatch):
    _env(monkeypatch)
    cs = bc.chunked_class_case(33, 70)
    nodes = np.array(cs["branches"], dtype=np.int64)
    w = cs["weights"]
    with _mk(cs, C=3) as part:
        _classes(cs, part)
        _hold_w(cs, cs["name"], nodes, part.branch_sensitivities(nodes, weights=w), weights=w)
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", "1")
        chunked = part.branch_sensitivities(nodes, weights=w)
        again = part.branch_sensitivities(nodes, weights=w)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        _hold_w(cs, cs["name"] + " in chunks of two tiles", nodes, chunked, weights=w)
        assert _same(chunked, again)


# ---- branch_gradient and branch_gradient_built --------------------------------------------------------------------------------------

def _hold_gradient(what, cs, outs, douts, nodes, Qreq, xreq, T, S, g, d1, weights=None):
    """S and the coefficient gradient of every request against the reference; sum_k x_k grad_k against the device's own d1."""
    for t, node in enumerate(nodes):
        Qs = [Qreq[t]] if Qreq[t].ndim == 2 else list(Qreq[t])
        ref = gc.gradient(cs, outs, int(node), Qs, weights=weights, T=T)
        St, gt, xt = np.asarray(S[t]).reshape(ref["S"].shape), np.asarray(g[t]).reshape(ref["grad"].shape), np.asarray(xreq[t]).reshape(ref["grad"].shape)
        mS = float(np.max(np.abs(St - ref["S"]) / ref["allow_S"]))
        mg = float(np.max(np.abs(gt - ref["grad"]) / ref["allow_grad"]))
        print(f"{what} node {int(node)}: S {mS:.3g}, gradient {mg:.3g} of their allowances")
        assert mS <= 1.0 and mg <= 1.0, (what, int(node), mS, mg)
        v = dc.values(cs, douts, int(node), Qs, weights)
        both = float(v["allow_d1"]) + float(np.sum(np.abs(xt) * ref["allow_grad"]))
        assert abs(float(d1[t]) - float(np.sum(xt * gt))) <= both, (what, int(node), float(d1[t]), float(np.sum(xt * gt)), both)


@pytest.mark.parametrize("D,K", [(4, 1), (5, 2), (20, 4), (61, 2)])
def test_gradient_and_built(D, K, monkeypatch):
    """Templates with zero rows, a coefficient of 1e-13 (branch 0), a repeated branch."""
    _env(monkeypatch)
    cs, T, x, Q = gc.built_case(D, K)
    nodes = np.array([0, 17, 5, 0] if D < 61 else [0, 17], dtype=np.int64)
    n = _nodes(cs)
    with _mk(cs) as part:
        part.set_q_templates(T)
        part.build_q(x)
        part.evaluate_built(n, n, cs["root_freqs"])
        outs = [gc.outside(cs)]
        S, sk = part.branch_gradient(nodes, Q[nodes])
        g, sk2 = part.branch_gradient_built(nodes, x[nodes])
        assert _same((S, sk), part.branch_gradient(nodes, Q[nodes])) and _same((g, sk2), part.branch_gradient_built(nodes, x[nodes]))
        d1 = part.branch_derivatives_built(nodes, x[nodes])[0]
        _hold_gradient(cs["name"], cs, outs, [dc.outside(cs)], nodes, Q[nodes], x[nodes], T, S, g, d1)
        assert np.all(sk == 0) and np.array_equal(sk, sk2)                                   # (exp(Q) has no zeros: nothing is impossible)


def test_gradient_built_rate_classes(monkeypatch):
    _env(monkeypatch)
    cs, T, x, Q = gc.ladder_template_case()
    w = cs["weights"]
    nodes = np.array(cs["branches"][1::2], dtype=np.int64)
    n = _nodes(cs)
    with _mk(cs, C=3) as part:
        part.set_q_templates(T)
        _classes(cs, part)
        xr, Qr = np.ascontiguousarray(x[:, nodes].transpose(1, 0, 2)), np.ascontiguousarray(Q[:, nodes].transpose(1, 0, 2, 3))
        S, _ = part.branch_gradient(nodes, Qr, weights=w)
        g, _ = part.branch_gradient_built(nodes, xr, weights=w)
        d1 = part.branch_derivatives_built(nodes, xr, weights=w)[0]
        _hold_gradient(cs["name"], cs, gc.outs_of(cs), dc.outs_of(cs), nodes, Qr, xr, T, S, g, d1, weights=w)


# ---- state and refusals -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [33, 4])
def test_no_state_is_left_behind(D, monkeypatch):
    """(full pass, branch_cache_build, [the three calls,] branch_cache_evaluate, partial update, full pass) gives the same bits with
    the calls and without them; reduce_form(), last_expm_kernel() and schedule_info() (the device memory among it) answer across
    the calls what they answered before."""
    from hyphy_amd import hip, tree
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="0"))
    cs = bc.cases_by_name()["bal2x4_D33"] if D == 33 else dc.d4_case()
    rng = np.random.default_rng(D)
    T = rng.random((2, D, D))
    x = rng.uniform(0.01, 0.05, size=(3, 2))
    nodes = np.array([1, 20, 7], dtype=np.int64)
    Q = np.stack([gc.build_q(T, xb) for xb in x])
    cached = int(cs["branches"][len(cs["branches"]) // 3])
    kind, M = bc.trials(cs, cached)[3]
    ch = np.array([cached], dtype=np.int64)
    path = tree.flat_from_parents(cs["flat_parents"], int(cs["L"])).path_update_nodes(cached)

    def sequence(with_calls):
        out = []
        with _mk(cs) as part:
            part.set_q_templates(T)
            out.append(_full(cs, part))
            if D != 4:
                part.branch_cache_build(cached)
            if with_calls:
                forms = (part.reduce_form(), hip.last_expm_kernel(), part.schedule_info())
                a = part.branch_sensitivities(nodes)
                b = part.branch_gradient(nodes, Q)
                c = part.branch_gradient_built(nodes, x)
                assert (part.reduce_form(), hip.last_expm_kernel(), part.schedule_info()) == forms
                assert _same(a, part.branch_sensitivities(nodes)) and _same(b, part.branch_gradient(nodes, Q))
                assert _same(c, part.branch_gradient_built(nodes, x))
                _hold_w(cs, f"{cs['name']} between the cache's build and its evaluation", nodes, a)
            if D != 4:
                out.append(part.branch_cache_evaluate(cached, M, q_is_probability=True, per_site=True))
            out.append(part.evaluate(path, ch, cs["P"][ch], cs["root_freqs"], q_is_probability=True, per_site=True))
            out.append(part.evaluate(_nodes(cs), NONE, None, cs["root_freqs"], per_site=True))
        return out
    for a, b in zip(sequence(False), sequence(True)):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_refusals_leave_the_partition_usable(monkeypatch):
    from hyphy_amd import hip
    _env(monkeypatch)
    cs = gc.bal_case(20)
    D, B = int(cs["D"]), len(cs["flat_parents"]) - 1
    Q = gc.adjoint_cases(D)[2][1][:1]
    one = np.zeros(1, dtype=np.int64)

    def message(call):
        with pytest.raises(hip.HipError) as e:
            call()
        return str(e.value)
    with _mk(cs) as part:
        assert "has not been evaluated" in message(lambda: part.branch_sensitivities([0]))
        first = _full(cs, part)
        for bad in (B, B + 1, -1):
            assert "node code out of range" in message(lambda: part.branch_sensitivities([0, bad]))
            assert "node code out of range" in message(lambda: part.branch_gradient([0, bad], np.concatenate([Q, Q])))
        part.set_pinned_states(3, np.zeros(int(cs["leaf_codes"].shape[1]), dtype=np.int64))
        assert "pinned" in message(lambda: part.branch_gradient([0], Q))
        part.set_pinned_states(None)
        assert "templates not set" in message(lambda: part.branch_gradient_built([0], np.ones((1, 2))))
        bad_q = Q.copy()
        bad_q[0, 1, 2] = np.nan
        assert "cannot be handled" in message(lambda: part.branch_gradient([0], bad_q))
        lib, out = part._lib, np.full(D * D, 7.0)
        sk = np.full(1, 7, dtype=np.int64)
        assert lib.hyphy_hip_branch_sensitivities(part._h, 1, hip._l(one), None, None, None) < 0
        assert lib.hyphy_hip_branch_sensitivities(part._h, 1, None, None, hip._d(out), None) < 0
        assert lib.hyphy_hip_branch_sensitivities(None, 1, hip._l(one), None, hip._d(out), None) < 0
        assert lib.hyphy_hip_branch_gradient(part._h, 1, hip._l(one), None, None, hip._d(out), None) < 0
        assert lib.hyphy_hip_branch_gradient_built(part._h, 1, hip._l(one), None, None, hip._d(out), None) < 0
        assert lib.hyphy_hip_branch_sensitivities(part._h, 0, hip._l(one), None, hip._d(out), hip._l(sk)) == 0
        assert lib.hyphy_hip_branch_gradient(part._h, 0, None, None, None, None, None) == 0
        assert np.all(out == 7.0) and sk[0] == 7
        again = _full(cs, part)
        assert again[0] == first[0] and again[1].tobytes() == first[1].tobytes()
        _hold_w(cs, "a call after the refusals", [0, B - 1], part.branch_sensitivities([0, B - 1]))
    with _mk(cs, C=3) as part:
        _full(cs, part, cat=0)
        _full(cs, part, cat=1)
        assert "has not been evaluated" in message(lambda: part.branch_sensitivities([0], weights=np.array([0.2, 0.3, 0.5])))
        _full(cs, part, cat=2)
        assert "weights are required" in message(lambda: part.branch_sensitivities([0]))


# ---- gradfit ------------------------------------------------------------------------------------------------------------------------

def test_quasi_newton_on_the_device(monkeypatch):
    """deriv_cases.fit_case (8 taxa, 20 states), K = 2, x_b = (t_b, omega t_b) with a global omega: the partition-driven fit and the
    numpy-driven fit (float64 restatement: scale-free pruning, grad_cases' outside pass, frechet_model, chain) from the same start."""
    from tests import expm_ref
    from hyphy_amd import gradfit
    _env(monkeypatch)
    D = 20
    cs = dc.fit_case("gradfit8_D20", dc.FIT_TREE_8, D, 400, 7702, max_patterns=40)
    B = len(cs["flat_parents"]) - 1
    mask = (np.add.outer(np.arange(D), np.arange(D)) % 2 == 0)
    U = cs["unit_Q"][0] * ~np.eye(D, dtype=bool)
    T = np.stack([U * mask, U * ~mask])

    def coeffs_of(x):
        return np.stack([x[:B], x[B] * x[:B]], axis=1)

    def jac(x):
        J = np.zeros((B, 2, B + 1))
        J[np.arange(B), 0, np.arange(B)] = 1.0
        J[np.arange(B), 1, np.arange(B)] = x[B]
        J[:, 1, B] = x[:B]
        return J

    def model(x):
        return dict(cs, name="gradfit_model", P=np.stack([expm_ref.reference(gc.build_q(T, c)) for c in coeffs_of(x)]))

    def np_evaluate(x):
        m = model(x)
        return sf.prune(D, m["flat_parents"], m["L"], m["leaf_codes"], m["ambig"], m["pattern_freq"], m["P"], m["root_freqs"])["logl"]

    def np_gradient(x):
        m = model(x)
        outs = [gc.outside(m, ft=np.float64)]
        co = coeffs_of(x)
        return np.stack([gc.chain(gc.frechet_model(gc.build_q(T, co[b]), gc.sensitivities(m, outs, b)["W"][0]), T) for b in range(B)])
    x0 = np.concatenate([np.full(B, 0.1), [1.0]])
    host = gradfit.fit_parameters(np_evaluate, np_gradient, x0, jac)
    with _mk(cs) as part:
        ev, gr = gradfit.partition_callables(part, T, coeffs_of, cs["root_freqs"])
        dev = gradfit.fit_parameters(ev, gr, x0, jac)
    print(f"gradfit: host {host[2]} iterations to {host[1]:.6f} (|g| {host[4]:.3g}), device {dev[2]} to {dev[1]:.6f} (|g| {dev[4]:.3g}), omega {dev[0][B]:.4f}")
    assert abs(host[1] - dev[1]) <= 1e-8 * abs(host[1])
    for r in (host, dev):
        assert r[4] <= 1e-6 * max(1.0, abs(r[1])) and r[1] > r[3][0]
