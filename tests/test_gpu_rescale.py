"""Every pruning path that owns a 2^64 rescale, held to a reference that has no such scheme (tests/scalefree.py), on the cases
where rescaling bites: near-identity matrices with off-diagonal entries down to 1e-30 on multifurcating conflict trees, tiles whose
lanes disagree about the rare path (conserved, conflicting, ambiguous and impossible patterns side by side), nodes that need two and
three steps at once, node sums within ulps of 2^-64, 300- and 600-taxon ladders, rate classes whose exponents lie far apart.

Per pattern ``log(lik) - 64 ln2 sc`` and the total against the reference at scalefree.GPU_RTOL (100 x the oracle's own measured
deviation from that reference, as the helper's docstring records) plus the absolute 1e-9 test_gpu_parity.py uses near zero;
-inf exactly where the reference has it; exponents integral.  (Marginal posteriors on these cases: tests/test_gpu_marginal.py.)"""
import numpy as np
import pytest

from tests import scalefree as sf
from tests.hold import _hold, _site, hold_download  # noqa: F401

pytestmark = pytest.mark.gpu

RTOL = sf.GPU_RTOL
ATOL = 1e-9
LOG_SCALER = sf.LOG_SCALER

CASES = sf.cases_by_name()
ALL = [n for n in CASES if not n.startswith("classes")]
FOUR = [n for n in ALL if int(CASES[n]["D"]) == 4]
WIDE = [n for n in ALL if int(CASES[n]["D"]) != 4]
SUBSET_WIDE = [n for n in sf.SUBSET if int(CASES[n]["D"]) != 4]
SUBSET_FOUR = [n for n in sf.SUBSET if int(CASES[n]["D"]) == 4]


def _mk(cs, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def _nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


_refs = {}


def _ref(name):
    if name not in _refs:
        _refs[name] = sf.case_reference(CASES[name])
    return _refs[name]


def _full(cs, part, per_site=True):
    n = _nodes(cs)
    return part.evaluate(n, n, cs["P"], cs["root_freqs"], q_is_probability=True, per_site=per_site)


def _run(name, env, monkeypatch, expect_kernel=None, passes=2):
    """A persisting and a lazy full pass under ``env``; both held to the reference, the second returned."""
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cs, ref = CASES[name], _ref(name)
    with _mk(cs) as part:
        for k in range(passes):
            got = _full(cs, part)
            _hold(f"{name} {env} pass {k} [{part.prune_kernel_name()}]", got, ref["site_logl"], ref["logl"])
        if expect_kernel:
            assert part.prune_kernel_name() == expect_kernel, (part.prune_kernel_name(), part.schedule_info())
    return got


KERNELS = {"workgroup": dict(HYPHY_HIP_KERNEL="0", HYPHY_HIP_REPEATS="0"),
           "wave": dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REPEATS="0"),
           "team": dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0")}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", WIDE)
def test_pruning_kernels_on_every_case(name, kernel, monkeypatch):
    _run(name, KERNELS[kernel], monkeypatch)


@pytest.mark.parametrize("mode", ["interpreter", "generated", "generated-small"])
@pytest.mark.parametrize("name", FOUR)
def test_four_state_kernels_on_every_case(name, mode, monkeypatch):
    env = {"interpreter": dict(HYPHY_HIP_NUCGEN="0"), "generated": dict(HYPHY_HIP_NUCGEN="2", HYPHY_HIP_NUCGEN_SMALL="0"),
           "generated-small": dict(HYPHY_HIP_NUCGEN="2", HYPHY_HIP_NUCGEN_SMALL="1")}[mode]
    _run(name, dict(env, HYPHY_HIP_REPEATS="0"), monkeypatch, passes=3)


@pytest.mark.parametrize("lp,fold", [("0", "0"), ("1", "0"), ("1", "1")])
@pytest.mark.parametrize("name", SUBSET_FOUR + ["mixed_D4_k2_1em6_S300", "ladder_D4_300", "threshold_D4_below", "star_D4_n8_1em9"])
def test_four_state_interpreter_with_and_without_the_lds_schedule(name, lp, fold, monkeypatch):
    _run(name, dict(HYPHY_HIP_NUCGEN="0", HYPHY_HIP_NUC_LP=lp, HYPHY_HIP_NUC_FOLD=fold, HYPHY_HIP_REPEATS="0"), monkeypatch)


@pytest.mark.parametrize("sort", ["0", "1"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", [n for n in WIDE if n.startswith("mixed")])
def test_mixed_tiles_sorted_and_in_the_callers_order(name, kernel, sort, monkeypatch):
    """With the caller's order kept, every group of 16 patterns is one tile: its lanes hold a zero, a conserved, a conflicting and an
    ambiguous pattern at once."""
    _run(name, dict(KERNELS[kernel], HYPHY_HIP_SORT_PATTERNS=sort), monkeypatch)


@pytest.mark.parametrize("sort", ["0", "1"])
@pytest.mark.parametrize("name", [n for n in FOUR if n.startswith("mixed")])
def test_mixed_tiles_four_states(name, sort, monkeypatch):
    for gen in ("0", "2"):
        _run(name, dict(HYPHY_HIP_NUCGEN=gen, HYPHY_HIP_SORT_PATTERNS=sort, HYPHY_HIP_REPEATS="0"), monkeypatch, passes=3)


@pytest.mark.parametrize("env", [dict(HYPHY_HIP_TILES=t) for t in "1234"] + [dict(HYPHY_HIP_FORCE_SHARDS="3"), dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2"),
                                 dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="3"), dict(HYPHY_HIP_FUSED_REDUCE="0"), dict(HYPHY_HIP_FUSED_REDUCE="1"),
                                 dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_CHAIN_M="1"), dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_CUT="levels", HYPHY_HIP_FRAGMENT="5")],
                         ids=lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("name", SUBSET_WIDE)
def test_tile_counts_shards_rerooting_and_reductions(name, env, monkeypatch):
    _run(name, dict(env, HYPHY_HIP_REPEATS="0"), monkeypatch, passes=3)


@pytest.mark.parametrize("name", SUBSET_FOUR)
def test_shards_and_reductions_four_states(name, monkeypatch):
    for env in (dict(HYPHY_HIP_FORCE_SHARDS="3"), dict(HYPHY_HIP_FUSED_REDUCE="0"), dict(HYPHY_HIP_FUSED_REDUCE="1")):
        _run(name, dict(env, HYPHY_HIP_REPEATS="0"), monkeypatch)


_TRUNKS = {"wave": dict(HYPHY_HIP_TRUNK_WALK="0"), "walk/1": dict(HYPHY_HIP_TRUNK_WALK="1", HYPHY_HIP_WALK_CHAINS="1"),
           "walk/2": dict(HYPHY_HIP_TRUNK_WALK="1", HYPHY_HIP_WALK_CHAINS="2"), "wg/0": dict(HYPHY_HIP_TRUNK_WALK="0", HYPHY_HIP_TRUNK_KERNEL="0")}


def _trunks(name):
    """The trunk forms that exist at the case's row-block count (the walk from two row blocks, the workgroup trunk at four)."""
    nw = (int(CASES[name]["D"]) + 15) // 16
    return ["wave"] + (["walk/1", "walk/2"] if nw >= 2 else []) + (["wg/0"] if nw == 4 else [])


_COMPRESSED = [(n, f) for n in SUBSET_WIDE + ["conflict_k4_d3_D20_1em15", "conflict_k3_d4_D64_1em3", "star_D61_n10_1em7", "ladder_D61_120_on_k4d3"]
               for f in _trunks(n)]


@pytest.mark.parametrize("theta", ["0.05", "0.9"])
@pytest.mark.parametrize("name,form", _COMPRESSED)
def test_class_compressed_form(name, form, theta, monkeypatch):
    """Conflict trees compress well (the leaf patterns repeat): class tables, the row-split walk and the trunks behind it."""
    env = _TRUNKS[form]
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")
    monkeypatch.setenv("HYPHY_HIP_REP_THETA", theta)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cs, ref = CASES[name], _ref(name)
    with _mk(cs) as part:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        for k in range(3):
            _hold(f"{name} compressed {form} theta {theta} pass {k} [{part.prune_kernel_name()}]", _full(cs, part), ref["site_logl"], ref["logl"])


@pytest.mark.parametrize("name", ["conflict_k4_d4_D4_1em15", "mixed_D4_k2_1em6_S300"])
def test_class_compressed_form_four_states(name, monkeypatch):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")
    monkeypatch.setenv("HYPHY_HIP_REP_THETA", "0.9")
    cs, ref = CASES[name], _ref(name)
    with _mk(cs) as part:
        for k in range(3):
            _hold(f"{name} compressed pass {k} [{part.prune_kernel_name()}]", _full(cs, part), ref["site_logl"], ref["logl"])


def _path_to_root(cs, code):
    L = int(cs["L"])
    out = [code]
    while out[-1] != len(cs["flat_parents"]) - 1:
        out.append(L + int(cs["flat_parents"][out[-1]]))
    return out[:-1]                                    # node codes whose branch lies on the path


@pytest.mark.parametrize("kernel", sorted(KERNELS) + ["default"])
@pytest.mark.parametrize("name", sf.SUBSET)
def test_partial_updates_after_a_full_pass(name, kernel, monkeypatch):
    """A full pass, then the branches along one leaf-to-root path change one at a time (conditionals persisted by the full pass are
    consumed by the partial ones), then the branch cache on a branch inside the tree (the 4-state path has no branch cache)."""
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    for k, v in KERNELS.get(kernel, {}).items():
        monkeypatch.setenv(k, v)
    cs = dict(CASES[name])
    P = cs["P"].copy()
    cs["P"] = P
    rng = np.random.default_rng(11)
    D, B = int(cs["D"]), len(P)
    with _mk(cs) as part:
        ref = sf.case_reference(cs)
        _hold(f"{name} full", _full(cs, part), ref["site_logl"], ref["logl"])
        _full(cs, part, per_site=False)                # (a lazy pass in between: the next partial update finds what it needs)
        path = _path_to_root(cs, 1)
        for code in path[:4] + path[-1:]:
            P[code] = sf.near_identity(rng, 1, D, min(float(P[code][0, 1]) * 3.0, 0.1 / D) if P[code][0, 1] > 0 else 1e-12)[0]
            ref = sf.case_reference(cs)
            ch = np.array([code], dtype=np.int64)
            got = part.evaluate(ch, ch, P[ch], cs["root_freqs"], q_is_probability=True, per_site=True)
            _hold(f"{name} partial update of branch {code}", got, ref["site_logl"], ref["logl"])
        if D == 4:
            return
        node = path[1]                                 # an internal branch
        part.branch_cache_build(node)
        P[node] = sf.near_identity(rng, 1, D, 1e-7)[0]
        ref = sf.case_reference(cs)
        got = part.branch_cache_evaluate(node, P[node], q_is_probability=True, per_site=True)
        _hold(f"{name} branch cache at {node}", got, ref["site_logl"], ref["logl"])


@pytest.mark.parametrize("kernel", ["wave", "workgroup", "default"])
@pytest.mark.parametrize("name", sf.SUBSET)
def test_pinned_states(name, kernel, monkeypatch):
    """A node of at most four children whose internal children are all tested (the kind of node that used to lose its own test), and a
    leaf."""
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    for k, v in KERNELS.get(kernel, {}).items():
        monkeypatch.setenv(k, v)
    cs = CASES[name]
    L, D, S = int(cs["L"]), int(cs["D"]), cs["leaf_codes"].shape[1]
    ch = sf.children_of(cs["flat_parents"], L)
    second = next(i for i in range(len(ch)) if any(c >= L for c in ch[i]))    # the first node above internal nodes
    n = _nodes(cs)
    with _mk(cs) as part:
        _full(cs, part, per_site=False)
        for node in (L + second, 2):
            states = ((np.arange(S) * 5 + 1) % D).astype(np.int64)
            ref = sf.case_reference(cs, pinned=(node, states))
            part.set_pinned_states(node, states)
            try:
                got = part.evaluate(n, n, cs["P"], cs["root_freqs"], q_is_probability=True, per_site=True)
            finally:
                part.set_pinned_states(None)
            _hold(f"{name} pinned at {node}", got, ref["site_logl"], ref["logl"])
        ref = _ref(name)
        _hold(f"{name} after the pins", _full(cs, part), ref["site_logl"], ref["logl"])


@pytest.mark.parametrize("repeats", ["0", "2"])
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("classes")])
def test_rate_classes_far_apart(name, repeats, monkeypatch):
    """Three classes with off-diagonals 1e-2, 1e-12 and 1e-30: per pattern their exponents differ by many units when they are mixed."""
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", repeats)
    cs, ref = CASES[name], _ref(name)
    n = _nodes(cs)
    with _mk(cs, C=3) as part:
        for k in range(2):
            got = part.evaluate_categories(n, n, cs["P"], cs["weights"], cs["root_freqs"], q_is_probability=True, per_site=True)
            _hold(f"{name} classes mixed, pass {k}", got, ref["site_logl"], ref["logl"])
        for c in range(3):
            got = part.evaluate(n, n, cs["P"][c], cs["root_freqs"], cat=c, q_is_probability=True, per_site=True)
            want = ref["class_site_logl"][c]
            _hold(f"{name} class {c} alone", got, want, float(np.sum(want * cs["pattern_freq"])))


@pytest.mark.parametrize("kernel", ["default", "wave"])
@pytest.mark.parametrize("name", list(sf.SUBSET) + ["star_D61_n9_2em8", "star_D4_n8_1em9"])
def test_downloaded_conditionals_and_counts(name, kernel, monkeypatch):
    """download_partials: conditionals divided by their largest element against the reference's, and the counts consistent with the
    values: log(largest element) - 64 ln2 count = the reference's log-magnitude."""
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    for k, v in KERNELS.get(kernel, {}).items():
        monkeypatch.setenv(k, v)
    cs = CASES[name]
    ref = sf.case_reference(cs, conditionals=True)
    with _mk(cs) as part:
        _full(cs, part, per_site=False)
        cache, counts = part.download_partials()
    hold_download(f"{name} {kernel}", cache, counts, ref["cond"], ref["log_mag"])
