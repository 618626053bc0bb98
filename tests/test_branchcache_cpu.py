"""The branch-cache cases (tests/branchcache_cases.py) are what the GPU tests need them to be.  CPU only.

1a  The CPU oracle agrees with ``scalefree.prune`` on every case with a sample of branches substituted by every kind of trial
    matrix.  Largest relative per-pattern deviation, measured by test_oracle_agrees_with_substituted_branches:

        BC_ORACLE_MAX_REL = 2.1e-15

    (2.03e-15 measured, bigladder_D61_300; the constant is that rounded up.)  It is at most scalefree.ORACLE_MAX_REL = 3.1e-15, so
    the GPU allowance for these cases stays scalefree.GPU_RTOL (plus the absolute 1e-9), and no case had to be taken out.
1b  The re-rooted recurrence the library runs, restated in numpy, gives ``prune``'s values at every branch of the full-coverage shapes.
1c  The same restatement without the transposition, and without pi on the edge below the old root, is off by at least 1000 x the
    GPU allowance on some branch at every path depth >= 1 of every full-coverage case: the cases can see those mistakes.
1d  Per row-block count 1 .. 4 the list reaches every arm of the build and of bc_eval_kernel.
"""
import numpy as np
import pytest

from tests import branchcache_cases as bc, scalefree as sf

BC_ORACLE_MAX_REL = 2.1e-15
CASES = bc.cases_by_name()
NAMES = list(CASES)
FULL = bc.full_coverage_names()
RTOL, ATOL = sf.GPU_RTOL, 1e-9


def _oracle(cs, P):
    from oracle import oracle
    nodes = np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)
    op = oracle.OraclePartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"])
    op.set_P(nodes, P)
    with np.errstate(divide="ignore"):
        return op.site_log_likelihoods(nodes, cs["root_freqs"])


def _sample(cs):
    br = cs["branches"]
    return sorted(set(br[:: max(1, len(br) // 6)] + br[-1:]))


_worst = {}


def _rel(got, want, what):
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


def test_allowance_rests_on_the_measured_deviation():
    assert BC_ORACLE_MAX_REL <= sf.ORACLE_MAX_REL and RTOL == 100 * sf.ORACLE_MAX_REL


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_substituted_branches(name):
    """1a, by the 1e-12 rule of test_scalefree_cpu.py; prints the deviation (the largest over the list is the docstring's figure)."""
    cs = CASES[name]
    worst = _rel(_oracle(cs, cs["P"]), bc.reference(cs)["site_logl"], name)
    for node in _sample(cs):
        for kind, M in bc.trials(cs, node):
            P = cs["P"].copy()
            P[node] = M
            worst = max(worst, _rel(_oracle(cs, P), bc.reference(cs, node, M)["site_logl"], (name, node, kind)))
    _worst[name] = worst
    print(f"{name}: oracle against scale-free, largest relative deviation {worst:.3e} (largest so far {max(_worst.values()):.3e})")
    assert worst < 1e-12, (name, worst)
    assert worst <= BC_ORACLE_MAX_REL, (name, worst, "BC_ORACLE_MAX_REL is out of date")


def test_class_cases_oracle():
    for cs in bc.class_cases():
        for c, node in enumerate(cs["branches"]):
            for kind, M in bc.trials(cs, node, c):
                P = cs["P"][c].copy()
                P[node] = M
                rel = _rel(_oracle(cs, P), bc.reference(cs, node, M, cls=c)["site_logl"], (cs["name"], c, node, kind))
                assert rel <= BC_ORACLE_MAX_REL, (cs["name"], c, node, kind, rel)


def test_case_list_is_what_the_issue_asks_for():
    assert not set(NAMES) & bc.REFERENCE_FAILS
    assert {int(CASES[n]["D"]) for n in NAMES if n.startswith("bal2x4")} == set(bc.STATE_COUNTS)
    assert {CASES[n]["shape"] for n in NAMES} == set(bc.SHAPES) | {"bigladder", "conflict"}
    for n in FULL:
        cs = CASES[n]
        assert cs["branches"] == list(range(len(cs["flat_parents"]) - 1))
    for cs in list(CASES.values()) + bc.class_cases():
        P, pi, D = cs["P"], cs["root_freqs"], int(cs["D"])
        S = cs["leaf_codes"].shape[1]
        assert S % 16 != 0 and (S == 1 or cs["pattern_freq"].max() > 1)
        assert P.min() >= 0.0 and np.allclose(P.sum(axis=-1), 1.0, rtol=0, atol=1e-14), cs["name"]
        assert abs(pi.sum() - 1) < 1e-14 and np.ptp(pi) > 0.1 / D
        for node in cs["branches"][:3]:
            tr = bc.trials(cs, node, 0 if P.ndim == 4 else None)
            assert [k for k, _ in tr] == list(bc.TRIAL_KINDS)
            for kind, M in tr:
                assert M.min() >= 0.0 and np.allclose(M.sum(axis=1), 1.0, rtol=0, atol=1e-14), (cs["name"], node, kind)
        if D < 3 or P.ndim == 4:
            continue
        # not reversible, and pi not stationary: detailed balance fails for dense matrices, pi P != pi
        dense = [M for M in P if (M > 0).all()]
        assert dense or cs["shape"] == "three_leaves"      # (every branch of that tree is a closed leaf branch)
        for M in dense[:8]:
            w, v = np.linalg.eig(M.T)
            st = np.real(v[:, np.argmax(np.real(w))])
            st = st / st.sum()
            flow = st[:, None] * M
            assert np.max(np.abs(flow - flow.T)) > 1e-3 * np.max(flow[~np.eye(D, dtype=bool)]), cs["name"]
            assert np.max(np.abs(pi @ M - pi)) > 1e-6 or float(cs["eps"]) < 1e-6, cs["name"]


def test_patterns_hold_every_kind_and_block_zero_trials_kill_some():
    """Every group of 16: a build-time impossible pattern, finite ones, ambiguity codes, a conserved pattern.  Per shape, a
    ``_block_zero`` trial makes a pattern impossible that was possible at build time on at least one tested branch (-inf total), and
    a dense trial brings the build-time impossible one back."""
    killed, revived = {}, {}
    for name, cs in CASES.items():
        base = bc.reference(cs)["site_logl"]
        S = len(base)
        for g in range(0, S - 15, 16):
            grp = slice(g, g + 16)
            assert np.isneginf(base[grp]).any() == cs["impossible_at_build"] and np.isfinite(base[grp]).any(), name
            assert (cs["leaf_codes"][:, grp] < 0).any()
            assert (cs["leaf_codes"][:, grp] == cs["leaf_codes"][:1, grp]).all(axis=0).any()
        for node in cs["branches"]:
            tr = dict(bc.trials(cs, node))
            ref = bc.reference(cs, node, tr["block_zero"])
            if (np.isneginf(ref["site_logl"]) & np.isfinite(base)).any():
                assert ref["logl"] == -np.inf
                killed[cs["shape"]] = killed.get(cs["shape"], 0) + 1
            if (np.isfinite(bc.reference(cs, node, tr["ordinary"])["site_logl"]) & np.isneginf(base)).any():
                revived[cs["shape"]] = revived.get(cs["shape"], 0) + 1
    print("block_zero kills a pattern at", killed, "; a dense trial revives one at", revived)
    shapes = {cs["shape"] for cs in CASES.values()} - {"three_leaves"}       # (one pattern: nothing to spare)
    assert shapes <= set(killed), shapes - set(killed)
    assert shapes - {"bigladder", "conflict"} <= set(revived), revived
    for shape in bc.FULL_SHAPES:             # with and without a build-time impossible pattern (the finite total is held too)
        assert {CASES[f"{shape}_D{D}"]["impossible_at_build"] for D in bc.FULL_D} == {False, True}
    for D in bc.FULL_D:
        assert {CASES[f"{shape}_D{D}"]["impossible_at_build"] for shape in bc.FULL_SHAPES} == {False, True}


def _allow(want):
    return RTOL * np.abs(want) + ATOL


@pytest.mark.parametrize("name", FULL)
def test_rerooted_recurrence_reproduces_the_reference_and_its_mutations_do_not(name):
    """1b and 1c."""
    cs = CASES[name]
    caught = {"untransposed": {}, "pi off the edge": {}}
    for node in cs["branches"]:
        depth = len(bc.ancestors(cs, node)) - 1
        for kind, M in bc.trials(cs, node):
            want = bc.reference(cs, node, M)["site_logl"]
            got = bc.rerooted_site_logl(cs, node, M)
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), (name, node, kind)
            fin = np.isfinite(want)
            assert np.all(np.abs(got[fin] - want[fin]) <= _allow(want[fin])), (name, node, kind)
            if depth < 1 or kind != "ordinary":
                continue
            for label, kw in (("untransposed", dict(transposed=False)), ("pi off the edge", dict(pi_on_edge=False))):
                bad = bc.rerooted_site_logl(cs, node, M, **kw)
                ok = fin & np.isfinite(bad)
                ratio = float(np.max(np.abs(bad[ok] - want[ok]) / _allow(want[ok])))
                caught[label][depth] = max(caught[label].get(depth, 0.0), ratio)
    depths = {len(bc.ancestors(cs, n)) - 1 for n in cs["branches"]} - {0}
    for label, by_depth in caught.items():
        assert set(by_depth) == depths
        print(f"{name}: {label}: smallest over the depths of the largest deviation / allowance = {min(by_depth.values()):.3g}")
        assert min(by_depth.values()) >= 1000.0, (name, label, by_depth)


def test_every_arm_is_reached_at_every_row_block_count():
    """1d."""
    from hyphy_amd import hip
    keys = ("internal child", "leaf child, unambiguous tile", "leaf child, mixed tile", "depth 0", "depth 1", "depth even >= 2",
            "depth odd >= 3", "pair of leaf siblings", "ambiguous leaf sibling")
    count = {nb: dict.fromkeys(keys, 0) for nb in (1, 2, 3, 4)}
    for cs in CASES.values():
        order = hip.plan_pattern_order(int(cs["D"]), cs["leaf_codes"])
        for node in cs["branches"]:
            f = bc.arm_features(cs, node, order)
            c = count[f["blocks"]]
            d = f["depth"]
            hits = (f["internal_child"], f["leaf_plain_tile"], f["leaf_mixed_tile"], d == 0, d == 1, d >= 2 and d % 2 == 0,
                    d >= 3 and d % 2 == 1, f["leaf_pair"], f["ambig_sibling"])
            for k, h in zip(keys, hits):
                c[k] += bool(h)
    for nb in count:
        print(f"{nb} row block(s): {count[nb]}")
        assert all(v > 0 for v in count[nb].values()), (nb, count[nb])
