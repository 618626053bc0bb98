"""CPU-only: the conditions under which the cases of tests/tuner_cases.py may be held to ``scalefree.case_reference`` at
scalefree.GPU_RTOL — the CPU oracle agrees with that reference on each within scalefree.ORACLE_MAX_REL (the constant the tolerance
is derived from; it is not raised here) — and under which they exercise what tests/test_gpu_tuner_forms.py forces: a pattern at
least three steps of 2^64 down, a re-rooting path, chain schedules at the forced cuts."""
import numpy as np
import pytest

from tests import scalefree as sf
from tests import tuner_cases as tc
from tests.test_scalefree_cpu import _oracle_site_logl

CASES = tc.cases_by_name()


@pytest.mark.parametrize("name", tc.NEW)
def test_oracle_agrees_with_the_scale_free_reference(name):
    cs = CASES[name]
    ref = sf.case_reference(cs)
    if cs["P"].ndim == 4:
        got = np.stack([_oracle_site_logl(cs, cs["P"][c]) for c in range(cs["P"].shape[0])])
        want = ref["class_site_logl"]
    else:
        got, want = _oracle_site_logl(cs, cs["P"]), ref["site_logl"]
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), name
    fin = np.isfinite(want)
    rel = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])))
    print(f"{name}: oracle against scale-free, largest relative deviation {rel:.3e}; smallest log-likelihood {want[fin].min():.1f}")
    assert rel <= sf.ORACLE_MAX_REL, (name, rel)


@pytest.mark.parametrize("name", tc.NEW)
def test_every_new_case_has_a_pattern_three_steps_down(name):
    """Some pattern's likelihood lies below 2^-192: the 2^64 rule fires at least three times on the way to the root (for the class
    case under each of the two classes with short branches; the sequence of the GPU test runs under the 1e-30 one)."""
    cs = CASES[name]
    ref = sf.case_reference(cs)
    per = ref["class_site_logl"][1:] if cs["P"].ndim == 4 else ref["site_logl"][None]
    for site in per:
        assert site[np.isfinite(site)].min() <= -3 * sf.LOG_SCALER, (name, site.min())
    sc = tc.scenario(name)                       # ... and so has every step of the sequence (the updates lengthen two branches)
    for step in (0, 1, 2, 3, "pin"):
        site = sc.ref(step)["site_logl"]
        assert site[np.isfinite(site)].min() <= -3 * sf.LOG_SCALER, (name, step)


@pytest.mark.parametrize("name", tc.NEW)
def test_every_new_case_can_be_rerooted_and_cut_into_chains(name):
    from hyphy_amd import hip
    cs = CASES[name]
    L = int(cs["L"])
    path = hip.plan_reroot(cs["flat_parents"], L)
    assert 3 <= len(path) <= 32, (name, path)
    ntiles = (cs["leaf_codes"].shape[1] + 15) // 16
    for kernel in (1, 2):
        for m in (1, 3, 8):
            for rr in (False, True):
                plan = hip.plan_schedule(cs["flat_parents"], L, kernel=kernel, chain_m=m, ntiles=ntiles, reroot=rr)
                assert plan["chain"] == 1 and plan["decode_errors"] == 0 and plan["rerooted"] == int(rr), (name, kernel, m, rr, plan)
    upd, pin, bc = tc.inner_nodes(cs)            # the nodes of the sequence lie on the path, below the root
    B = len(cs["flat_parents"]) - 1
    assert all(L <= n < B and n - L in path for n in (upd, pin, bc)), (name, upd, pin, bc)


def test_the_control_and_the_existing_cases_are_what_the_gpu_test_expects():
    from hyphy_amd import hip
    assert len(hip.plan_reroot(CASES[tc.CONTROL]["flat_parents"], int(CASES[tc.CONTROL]["L"]))) == 0
    assert set(tc.CLASS_CASES) == {n for n, c in CASES.items() if c["P"].ndim == 4}
    for name in tc.EXISTING:
        cs = CASES[name]
        S = cs["leaf_codes"].shape[1]
        assert 49 <= int(cs["D"]) <= 64 and 2 <= (S + 15) // 16 <= 5, name
    assert len(tc.EXISTING) == 11 and len(set(CASES)) == 16
