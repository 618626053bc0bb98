"""Marginal ancestral reconstruction on the device (hyphy_hip_marginal_ancestral): one pre-order pass over the resident conditionals
against the REAL reference's support matrix, against the CPU oracle's pinned-state loop (the computation the reference does:
RecoverAncestralSequencesMarginal, likefunc2.cpp:932-1120) at every state count, with rate classes, and against the device's own
pinned route at full size; plus the states the call must leave untouched.

Below those: the call held to the scale-free reference (tests/scalefree.py: ``post``, ``leaf_post``) componentwise, internal rows and
leaf rows, support and MAP, on the cases of tests/marginal_cases.py — every state count, the rescaling cases, 41 children at one
node, rate classes whose exponents lie far apart in every order, patterns impossible under one class and under all — in every form
of the call (shards, the caller's pattern order, every pruning kernel behind it), and twice over the same scratch.  These run with
HYPHY_HIP_TUNE=0 and probability matrices handed over as they are, so the device's exponentials are no part of the comparison."""
import numpy as np
import pytest

from tests import common, marginal_cases as mc, scalefree as sf

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


_pin_update_list = mc.pin_update_list


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


# ---- held to the scale-free reference (tests/marginal_cases.py) --------------------------------------------------------------------

WHICH = (("internal", "post"), ("leaves", "leaf_post"))


def _evaluate(cs, part, P=None):
    P = cs["P"] if P is None else P
    n = np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)
    if P.ndim == 4:
        for c in range(P.shape[0]):
            part.evaluate(n, n, P[c], cs["root_freqs"], cat=c, q_is_probability=True)
    else:
        part.evaluate(n, n, P, cs["root_freqs"], q_is_probability=True)


def _held(name, monkeypatch, env=None, cs=None, ref=None, compressed=False):
    """Both forms of the call on the case under ``env``: support through hold_support, impossible patterns NaN / -1 / NaN, MAP
    through hold_map.  One call per ``which``.  ``compressed``: the partition has to run class-compressed before the calls (three
    evaluations: the third is a compressed pass over resident tables) and again at the evaluation after them."""
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    cs = mc.cases()[name] if cs is None else cs
    ref = mc.reference(name) if ref is None else ref
    C = cs["P"].shape[0] if cs["P"].ndim == 4 else 1
    with _mk(cs, C) as part:
        _evaluate(cs, part)
        if compressed:
            part.set_repeats(True)
            for _ in range(2):
                _evaluate(cs, part)
            st = part.repeat_stats()
            assert st["in_use"] == 1 and st["tables"] > 0, st
        for which, key in WHICH:
            what = f"{name} {env or ''} {which} [{part.prune_kernel_name()}]"
            sup, ms, mv = part.marginal_ancestral(which, weights=cs.get("weights"), map=True)
            gone = np.isneginf(ref["site_logl"])
            assert np.isnan(ref[key][:, gone]).all() and np.isnan(sup[:, gone]).all(), what
            mc.hold_support(what, sup, ref[key], sums_to_one=which == "internal")
            mc.hold_map(what, ms, mv, sup, ref[key])
        if compressed:
            _evaluate(cs, part)
            assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()


@pytest.mark.parametrize("name", mc.group("states"))
def test_held_at_every_state_count(name, monkeypatch):
    _held(name, monkeypatch)


@pytest.mark.parametrize("name", mc.group("scalefree"))
def test_held_where_rescaling_bites(name, monkeypatch):
    _held(name, monkeypatch)


@pytest.mark.parametrize("name", mc.group("wide"))
def test_held_with_forty_children_at_one_node(name, monkeypatch):
    _held(name, monkeypatch)


@pytest.mark.parametrize("name", mc.group("classes"))
def test_held_with_classes_far_apart_in_every_order(name, monkeypatch):
    _held(name, monkeypatch)


@pytest.mark.parametrize("name", mc.group("one_class_impossible"))
def test_pattern_impossible_under_one_class(name, monkeypatch):
    """The other class's exponent is 17 or more above the impossible one's (test_marginal_cases_cpu.py): every row finite and held."""
    assert np.isfinite(mc.reference(name)["site_logl"]).all()
    _held(name, monkeypatch)


@pytest.mark.parametrize("name", mc.group("all_impossible"))
def test_pattern_impossible_under_every_class(name, monkeypatch):
    """NaN in all D entries, MAP state -1 and MAP support NaN on the impossible patterns (include/hyphy_hip.h); held on the rest."""
    assert np.isneginf(mc.reference(name)["site_logl"]).any()
    _held(name, monkeypatch)


FORM_ENVS = [dict(HYPHY_HIP_FORCE_SHARDS="3"), dict(HYPHY_HIP_SORT_PATTERNS="0"), dict(HYPHY_HIP_FORCE_SHARDS="3", HYPHY_HIP_SORT_PATTERNS="0"),
             dict(HYPHY_HIP_KERNEL="0"), dict(HYPHY_HIP_KERNEL="1"), dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_CHAIN_M="2"),
             dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2")]


@pytest.mark.parametrize("env", FORM_ENVS, ids=lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("name", mc.FORMS)
def test_forms_of_the_call(name, env, monkeypatch):
    """Held to the reference, not to each other's bits: the persisted conditionals may carry their exponents differently per kernel."""
    _held(name, monkeypatch, env)


@pytest.mark.parametrize("nucgen", ["0", "2"])
def test_forms_four_states_generated_and_interpreted(nucgen, monkeypatch):
    _held("mixed_D4_k4_1em20_S37", monkeypatch, dict(HYPHY_HIP_NUCGEN=nucgen))


_compressible = {}


@pytest.mark.parametrize("D", [61, 4])
def test_forms_class_compressed(D, monkeypatch):
    """The call behind a class-compressed evaluation (it restores the per-pattern copies first) on a partition whose subtrees repeat;
    its matrices are the CPU oracle's exponentials of the case's rates.  The form is asserted in use: at 61 states it exists only on
    the wave-per-tile kernel, which a partition this small takes on request alone; at 4 states only when forced (HYPHY_HIP_REPEATS=2)."""
    from oracle import oracle
    if D not in _compressible:
        cs = dict(common.compressible_case(D, 7), name=f"compressible_D{D}")
        cs["P"] = oracle.expm(cs["Q"], False)
        _compressible[D] = cs, sf.case_reference(cs, posteriors=True)
    cs, ref = _compressible[D]
    env = dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1") if D > 4 else dict(HYPHY_HIP_REPEATS="2")
    _held(cs["name"], monkeypatch, env, cs, ref, compressed=True)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


@pytest.mark.parametrize("name", mc.FORMS)
def test_scratch_reuse(name, monkeypatch):
    """The shard's scratch persists between calls: internal, leaves, internal gives the first call's bits again; after an evaluation
    with other matrices the call gives a fresh partition's bits under those matrices and none of the first call's."""
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    cs = mc.cases()[name]
    D, B = int(cs["D"]), len(cs["flat_parents"]) - 1
    P2 = sf.ordinary(np.random.default_rng(21), B, D)
    with _mk(cs) as part:
        _evaluate(cs, part)
        first = part.marginal_ancestral("internal", map=True)
        leaves = part.marginal_ancestral("leaves", map=True)
        third = part.marginal_ancestral("internal", map=True)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, third)), name
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(leaves, part.marginal_ancestral("leaves", map=True))), name
        _evaluate(cs, part, P2)
        after = part.marginal_ancestral("internal", map=True)
        after_l = part.marginal_ancestral("leaves")
    with _mk(cs) as part:
        _evaluate(cs, part, P2)
        fresh = part.marginal_ancestral("internal", map=True)
        fresh_l = part.marginal_ancestral("leaves")
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(after, fresh)), name
    assert np.array_equal(_bits(after_l), _bits(fresh_l)), name
    assert np.isfinite(after[0]).all() and not np.any(after[0] == first[0]), name
    ref = sf.case_reference(dict(cs, P=P2), posteriors=True)
    mc.hold_support(f"{name} after other matrices", after[0], ref["post"], sums_to_one=True)
    mc.hold_support(f"{name} after other matrices, leaves", after_l, ref["leaf_post"])


@pytest.mark.parametrize("name", ["conflict_k4_d3_D61_1em15", "conflict_k4_d3_D4_1em20", "conflict_k2_d8_D61_1em30", "conflict_k5_d3_D61_1em6",
                                  "ladder_D61_300", "ladder_D4_300", "mixed_D61_k4_1em15_S53"])
def test_marginal_posteriors(name, monkeypatch):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    cs = sf.cases_by_name()[name]
    ref = sf.case_reference(cs, posteriors=True)
    with _mk(cs) as part:
        n = np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)
        part.evaluate(n, n, cs["P"], cs["root_freqs"], q_is_probability=True, per_site=False)
        sup = part.marginal_ancestral("internal")
    ok = np.isfinite(ref["site_logl"])
    assert np.allclose(sup[:, ok], ref["post"][:, ok], rtol=1e-9, atol=1e-12)
