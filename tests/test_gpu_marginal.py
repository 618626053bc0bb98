"""Marginal ancestral reconstruction on the device (hyphy_hip_marginal_ancestral): one pre-order pass over the resident conditionals
against the REAL reference's support matrix, against the CPU oracle's pinned-state loop (the computation the reference does:
RecoverAncestralSequencesMarginal, likefunc2.cpp:932-1120) at every state count, with rate classes, and against the device's own
pinned route at full size; plus the states the call must leave untouched."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

LN2_64 = 64 * np.log(2.0)


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")


def _mk(fx, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(fx["D"]), fx["flat_parents"], int(fx["L"]), fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], C)


def _Q(fx):
    return fx["Q"] if "Q" in fx else common.fixture_Q(fx)


def _pin_update_list(fp, L, code):
    from hyphy_amd import tree
    flat = tree.flat_from_parents(fp, L)
    out = set()
    if int(flat.flat_parents[code]) >= 0:
        out.update(int(x) for x in flat.path_update_nodes(int(code)))
    if code >= L:
        out.update(int(c) for c in flat.children_of(code - L))
    return np.array(sorted(out), dtype=np.int64)


def _oracle_support(fx, Ps, weights, codes_nodes):
    """support[row][S][D] of the pinned-state loop on the CPU oracle: sum_c w_c L_c(node = x) / sum_c w_c L_c, per pattern."""
    from oracle import oracle
    L, D = int(fx["L"]), int(fx["D"])
    C = len(Ps)
    nodes = common.all_nodes(fx)
    pi = fx["root_freqs"]
    op = oracle.OraclePartition(D, fx["flat_parents"], L, fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], C_cat=C)
    for c in range(C):
        op.set_P(nodes, Ps[c], cat=c)
    base = [op.site_block(nodes, pi, cat=c) for c in range(C)]
    e0 = np.min([b[1] for b in base], axis=0)
    den = sum(weights[c] * base[c][0] * np.exp(-(base[c][1] - e0) * LN2_64) for c in range(C))
    out = np.zeros((len(codes_nodes), op.S, D))
    for r, code in enumerate(codes_nodes):
        for x in range(D):
            op.set_branch(int(code), np.full(op.S, x))
            for c in range(C):
                lk, sc = op.site_block(nodes, pi, cat=c)
                out[r, :, x] += weights[c] * lk * np.exp(-(sc - e0) * LN2_64)
        op.set_branch(None)
    return out / den[None, :, None]


def _sample(n, k=4):
    return sorted(set(np.linspace(0, n - 1, k).round().astype(int).tolist()))


def _check_map(part, which, sup, weights=None):
    ms, mv = part.marginal_ancestral(which, weights=weights, support=False, map=True)
    assert np.array_equal(ms, sup.argmax(2))
    assert np.array_equal(mv, sup.max(2))


@pytest.mark.parametrize("kernel", ["0", "1"])
@pytest.mark.parametrize("repeats", ["2", "0"])
def test_reference_golden(kernel, repeats, monkeypatch):
    monkeypatch.setenv("HYPHY_HIP_KERNEL", kernel)
    monkeypatch.setenv("HYPHY_HIP_REPEATS", repeats)
    fx = common.load("codon_small_marginal")
    nodes = common.all_nodes(fx)
    with _mk(fx) as part:
        part.evaluate(nodes, nodes, common.fixture_Q(fx), fx["root_freqs"])
        sup = part.marginal_ancestral("internal")
        _check_map(part, "internal", sup)
    I, S = sup.shape[:2]
    assert np.allclose(sup.sum(2), 1.0, rtol=0, atol=1e-12)
    ours = sup.copy()
    ours[:, :, 60] = 1.0 - sup[:, :, :60].sum(2)
    ref = fx["support"].reshape(I, S, 61)
    used = set()
    for i in range(I):
        match = [r for r in range(I) if r not in used and np.allclose(ours[i], ref[r], rtol=1e-9, atol=1e-12)]
        assert match, (kernel, repeats, i)
        used.add(match[0])


def _oracle_case(name):
    if name.startswith("cc"):
        return common.compressible_case(int(name[2:]), 11)
    return common.load(name)


@pytest.mark.parametrize("name", ["nuc_ambig", "nuc_deep", "codon_ambig", "codon_deep"] +
                         ["cc%d" % d for d in common.REPEAT_STATE_COUNTS])
def test_oracle_every_state_count(name):
    from oracle import oracle
    fx = _oracle_case(name)
    L, D = int(fx["L"]), int(fx["D"])
    I = len(fx["flat_parents"]) - L
    nodes = common.all_nodes(fx)
    Q = _Q(fx)
    P = oracle.expm(Q, D > 4 and "Q" not in fx)
    with _mk(fx) as part:
        part.evaluate(nodes, nodes, Q, fx["root_freqs"])
        sup_i = part.marginal_ancestral("internal")
        sup_l = part.marginal_ancestral("leaves")
        _check_map(part, "internal", sup_i)
        _check_map(part, "leaves", sup_l)
    assert np.allclose(sup_i.sum(2), 1.0, rtol=0, atol=1e-12)
    ri, rl = _sample(I), _sample(L)
    ref = _oracle_support(fx, [P], [1.0], [L + i for i in ri] + rl)
    assert np.allclose(sup_i[ri], ref[:len(ri)], rtol=1e-9, atol=1e-12), name
    assert np.allclose(sup_l[rl], ref[len(ri):], rtol=1e-9, atol=1e-12), name


@pytest.mark.parametrize("name", ["codon_cat3", "cc20"])
def test_rate_classes(name):
    from oracle import oracle
    if name == "codon_cat3":
        fx = common.load(name)
        vals = [float(v) for v in fx["cat_values"]]
        w = np.asarray(fx["cat_weights"], dtype=np.float64)
        Qs = [common.fixture_Q(fx, v) for v in vals]
    else:
        fx = common.compressible_case(20, 5)
        vals = [0.3, 1.0, 2.5]
        w = np.array([0.2, 0.5, 0.3])
        Qs = [fx["Q"] * v for v in vals]
    L, D = int(fx["L"]), int(fx["D"])
    I = len(fx["flat_parents"]) - L
    nodes = common.all_nodes(fx)
    with _mk(fx, C=len(vals)) as part:
        for c, Q in enumerate(Qs):
            part.evaluate(nodes, nodes, Q, fx["root_freqs"], cat=c)
        sup_i = part.marginal_ancestral("internal", weights=w)
        sup_l = part.marginal_ancestral("leaves", weights=w)
        _check_map(part, "internal", sup_i, w)
    Ps = [oracle.expm(Q, name == "codon_cat3") for Q in Qs]
    ri, rl = _sample(I), _sample(L, 3)
    ref = _oracle_support(fx, Ps, w, [L + i for i in ri] + rl)
    assert np.allclose(sup_i[ri], ref[:len(ri)], rtol=1e-9, atol=1e-12)
    assert np.allclose(sup_l[rl], ref[len(ri):], rtol=1e-9, atol=1e-12)
    assert np.allclose(sup_i.sum(2), 1.0, rtol=0, atol=1e-12)


def _device_pinned(part, fx, code, Q_none_shape, base, bsc):
    """support of node `code` by the device's pinned route (partial updates along its path)."""
    L, D = int(fx["L"]), int(fx["D"])
    un = _pin_update_list(fx["flat_parents"], L, code)
    none = np.zeros(0, dtype=np.int64)
    out = np.zeros((part.S, D))
    for x in range(D):
        part.set_pinned_states(code, np.full(part.S, x))
        _, lk, sc = part.evaluate(un, none, np.zeros(Q_none_shape), fx["root_freqs"], per_site=True)
        out[:, x] = lk / base * np.exp(-(sc - bsc) * LN2_64)
    part.set_pinned_states(None)
    part.evaluate(un, none, np.zeros(Q_none_shape), fx["root_freqs"])
    return out


def test_explicit_mixture_against_device_pinned_route():
    from hyphy_amd import models
    fx = common.load("codon_mix3")
    L = int(fx["L"])
    I = len(fx["flat_parents"]) - L
    nodes = common.all_nodes(fx)
    rev = dict(zip(common.REV_KEYS, (float(x) for x in fx["rev"])))
    t = np.asarray(fx["t"], dtype=np.float64)
    Qc = np.stack([models.mg94rev_Q_batch(t, float(om), rev, fx["pos_freqs"]) for om in fx["omegas"]], axis=1)
    W = np.tile(np.asarray(fx["weights"], dtype=np.float64), (len(nodes), 1))
    with _mk(fx) as part:
        _, base, bsc = part.evaluate_mixture(nodes, nodes, Qc, W, fx["root_freqs"], per_site=True)
        sup = part.marginal_ancestral("internal")
        for i in (0, I // 2, I - 1):
            ref = _device_pinned(part, fx, L + i, (0, 61, 61), base, bsc)
            assert np.allclose(sup[i], ref, rtol=1e-9, atol=1e-12), i


@pytest.mark.parametrize("state", ["lazy", "partial", "pi_only", "reroot"])
def test_pass_states_before_the_call(state, monkeypatch):
    from oracle import oracle
    if state == "reroot":
        monkeypatch.setenv("HYPHY_HIP_REROOT", "1")
    fx = common.load("codon_deep")
    L = int(fx["L"])
    I = len(fx["flat_parents"]) - L
    nodes = common.all_nodes(fx)
    Q = common.fixture_Q(fx)
    pi = fx["root_freqs"]
    rng = np.random.default_rng(4)
    with _mk(fx) as part:
        part.evaluate(nodes, nodes, Q, pi)
        part.evaluate(nodes, nodes, Q, pi)   # (a full pass behind a full pass: lazy persistence)
        if state == "partial":
            node = L + 3
            Q = Q.copy()
            Q[node] *= 1.3
            part.evaluate(_pin_update_list(fx["flat_parents"], L, node), np.array([node]), Q[node][None], pi)
        elif state == "pi_only":
            pi = rng.random(61) + 0.1
            pi /= pi.sum()
            part.evaluate(nodes[:0], nodes[:0], np.zeros((0, 61, 61)), pi)
        sup = part.marginal_ancestral("internal")
    ri = _sample(I, 3)
    fx2 = dict(fx)
    fx2["root_freqs"] = pi
    ref = _oracle_support(fx2, [oracle.expm(Q, True)], [1.0], [L + i for i in ri])
    assert np.allclose(sup[ri], ref, rtol=1e-9, atol=1e-12), state


def test_no_residue():
    from oracle import oracle
    fx = common.compressible_case(61, 7)
    L, D = int(fx["L"]), int(fx["D"])
    nodes = common.all_nodes(fx)
    Q = fx["Q"]
    pi = fx["root_freqs"]
    op = oracle.OraclePartition(D, fx["flat_parents"], L, fx["leaf_codes"], fx["ambig"], fx["pattern_freq"])
    op.set_P(nodes, oracle.expm(Q, False))
    ref_full = op.compute_block(nodes, pi)
    bnode = L + 1
    with _mk(fx) as part:
        for _ in range(3):
            part.evaluate(nodes, nodes, Q, pi)
        stats = part.repeat_stats()
        name = part.prune_kernel_name()
        part.branch_cache_build(bnode)
        part.marginal_ancestral("internal")
        part.marginal_ancestral("leaves", map=True)
        ll_bc = part.branch_cache_evaluate(bnode, Q[bnode] * 1.5)
        ll = part.evaluate(nodes, nodes, Q, pi)
        assert abs(ll - ref_full) <= 1e-10 * abs(ref_full)
        assert part.repeat_stats()["in_use"] == stats["in_use"]
        assert part.prune_kernel_name() == name
        Q2 = Q.copy()
        Q2[bnode] = Q[bnode] * 1.5
        op2 = oracle.OraclePartition(D, fx["flat_parents"], L, fx["leaf_codes"], fx["ambig"], fx["pattern_freq"])
        op2.set_P(nodes, oracle.expm(Q2, False))
        ref2 = op2.compute_block(nodes, pi)
        assert abs(ll_bc - ref2) <= 1e-10 * abs(ref2)
        ll_p = part.evaluate(_pin_update_list(fx["flat_parents"], L, bnode), np.array([bnode]), Q2[bnode][None], pi)
        assert abs(ll_p - ref2) <= 1e-10 * abs(ref2)


def test_errors():
    from hyphy_amd import hip
    fx = common.load("codon_small_marginal")
    nodes = common.all_nodes(fx)
    with _mk(fx) as part:
        with pytest.raises(hip.HipError, match="not been evaluated"):
            part.marginal_ancestral("internal")
        part.evaluate(nodes, nodes, common.fixture_Q(fx), fx["root_freqs"])
        part.set_pinned_states(int(fx["L"]), np.zeros(part.S, dtype=np.int64))
        with pytest.raises(hip.HipError, match="pinned"):
            part.marginal_ancestral("internal")
        part.set_pinned_states(None)
    fx3 = common.load("codon_cat3")
    with _mk(fx3, C=3) as part:
        for c in range(3):
            part.evaluate(common.all_nodes(fx3), common.all_nodes(fx3), common.fixture_Q(fx3), fx3["root_freqs"], cat=c)
        with pytest.raises(ValueError):
            part.marginal_ancestral("internal")
        assert part._lib.hyphy_hip_marginal_ancestral(part._h, 0, None, None, None, None) < 0   # (the C-ABI's own refusal)
        assert b"weights" in part._lib.hyphy_hip_last_error()


def test_full_size_against_device_pinned_route():
    from hyphy_amd import hip, models
    from hyphy_amd import data
    fx = common.load("full_mg94_64x10k")
    syn = data.evolve(int(fx["taxa"]), int(fx["sites"]), 3, seed=int(fx["seed"]), p_change=float(fx["p_change"]))
    pd = data.from_states(syn.states, 61, compress_patterns=True)
    rev = dict(zip(common.REV_KEYS, (float(x) for x in fx["rev"])))
    B = syn.flat.n_branches
    pi = models.f3x4_codon_freqs(fx["pos_freqs"])
    Q = models.mg94rev_Q_batch(np.full(B, float(fx["t"])), float(fx["omega"]), rev, fx["pos_freqs"])
    nodes = np.arange(B, dtype=np.int64)
    L, I = syn.flat.L, syn.flat.I
    f = dict(L=np.int64(L), D=np.int64(61), flat_parents=np.asarray(syn.flat.flat_parents), root_freqs=pi)
    with hip.HipPartition(61, syn.flat.flat_parents, L, pd.leaf_codes, None, pd.pattern_freq) as part:
        _, base, bsc = part.evaluate(nodes, nodes, Q, pi, per_site=True)
        sup = part.marginal_ancestral("internal")
        assert np.allclose(sup.sum(2), 1.0, rtol=0, atol=1e-12)
        for i in _sample(I):
            ref = _device_pinned(part, f, L + i, (0, 61, 61), base, bsc)
            assert np.allclose(sup[i], ref, rtol=1e-9, atol=1e-12), i
