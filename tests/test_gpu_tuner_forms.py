"""Every form the schedule tuner can pick, held to the scale-free reference (tests/scalefree.py) on cases where the 2^64 rescale bites.

Which pruning kernel, instantiation and cut a partition runs in steady state is decided at run time by tune_schedule (csrc/tuner.hip)
from an event pair, and differs by machine and moment.  Here every candidate is forced in turn, and the tuner itself is run, on the
cases of tests/tuner_cases.py: rescale-heavy, two to five tiles, four of the new ones hung from an end of the tree so that re-rooting
has something to do.  ``HipPartition.prune_form()`` is written down where the launcher picks the instantiation, so a form that was
asked for and quietly replaced by the production one fails here instead of passing.

Everything is held with tests/hold.py::_hold: per pattern and total at scalefree.GPU_RTOL x |reference| + 1e-9, -inf exactly where
the reference has it, integral exponents.  HYPHY_HIP_POISON=1 and HYPHY_HIP_REPEATS=0 throughout.

The one sequence (tests/tuner_child.py::run_sequence): (1) a persisting full pass, (2) two lazy full passes, (3) a partial update of a
leaf branch, (4) of an internal branch on the re-rooting path, (5) a lazy full pass, (6) a pinned evaluation at an internal node,
un-pin and a full pass, (7) the branch cache at a node of the re-rooting path, (8) download_partials against the reference's
conditionals, (9) a last full pass; prune_form() is read behind every lazy full pass.

(a) every candidate forced (HYPHY_HIP_TUNE=0): the wave kernel with 0 / 1 / 2 parking slots, its two three-waves-per-SIMD
    instantiations, the row-split kernel on chains and the workgroup kernel, each on level cuts and chain cuts m = 1, 3, 8, the chain
    forms also re-rooted on the cases that have a re-rooting path.  A chain cut exists for m below the number of internal nodes: the
    stars and the threshold cases have three, and run m = 2 in place of 3 and 8.  A class case runs under its 1e-30 class.
    Nothing of the form x case product is left out, and no pair is skipped.
(b) class batches under the three-waves instantiations and each slot count, each class alone afterwards.
(c) the tuner itself, in a process of its own with HYPHY_HIP_TUNE_CACHE=0 (read once per process): the persisting pass, the pass the
    candidates run behind and two passes under the winner are held, the report lists what the stages must have tried, prune_form()
    is what the label behind "->" says, then the sequence.  (The row-split kernel forced, HYPHY_HIP_KERNEL=2, has no level-peeled
    candidate: its report lists chain cuts only.)  Variants: the tuner runs behind a pinned evaluation; one class / batch / one class.
(d) the cache: a second partition on the same tree takes the choice over; a third created under HYPHY_HIP_SLOTS or evaluated under
    HYPHY_HIP_WAVE_VARIANT=0 obeys the switch whatever the first one chose.

Measured on an MI355X (the figures are measurements against the reference, not tolerances):
    run time    496 tests in 17 s in one pytest process (the 22 child processes of (c) and (d) take 0.6-0.8 s each, a forced
                sequence 0.01-0.25 s); nothing of the form x case product had to be thinned, no pair is skipped.
    (c) winners, two runs (KERNEL=1 / KERNEL=2):
                cat24_on_k4d2_D61 rr1/m3, levels / rr1/team/m3; cat16_on_k2d3_D64 rr0/m3, rr0/m5 / rr0/team/m3; cat40_D61_1em6 rr0/m12,
                rr0/m24 / rr0/team/m16, rr0/team/m12; cat12_on_k2d3_D61_cls (1e-30 class) levels / rr0/team/m5, rr0/team/m3;
                classes_D61_k2 m3 / team/m3; conflict_k4_d3_D61_1em15 m3 / team/m3; behind a pinned pass m3, levels / team/m24;
                one class / batch / one class: levels five times / team/m16, team/m3 alternating.  A three-waves candidate was
                measured wherever a chain won stage one and never chosen: these shards are two to five tiles.
    (d)         the first partitions chose levels, rr0/m3, rr0/m5, rr0/m12 or rr0/m16: the hole in the cache key (a three-waves choice taken
                over by a partition under HYPHY_HIP_SLOTS) did not bite: no first partition chose the three-waves instantiation, here or
                on three large shards tried by hand (profiles/tuner_forms_tests_and_mutations.md); the invariant held either way.
    _hold       6 440 comparisons, largest per-pattern deviation / allowance 0.002 (ladder_D61_300, level cut, persisting pass).
"""
import numpy as np
import pytest

from tests import scalefree as sf
from tests import tuner_cases as tc
from tests import tuner_child as child
from tests.hold import _hold

pytestmark = pytest.mark.gpu

CASES = tc.cases_by_name()
ALL = list(tc.NEW) + [tc.CONTROL] + list(tc.EXISTING)
CAN_REROOT = list(tc.NEW)          # (the generator's ladders are longer than a re-rooting path may be; test_tuner_cases_cpu.py checks these)

CUTS = ("levels", "m1", "m3", "m8")


def _forms():
    """[(id, kernel switches, what prune_form() must say of the instantiation, cut)]"""
    out = []
    for cut in CUTS:
        for slots in (2, 3, 4):
            out.append((f"wave-park{slots - 2}-{cut}", dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_SLOTS=str(slots)),
                        f"prune_wave_kernel NW=4 park={slots - 2} occ2;", cut))
        for wv, inst in ((2, "occ3"), (3, "occ3+pre")):
            out.append((f"wave-{inst}-{cut}", dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_SLOTS="2", HYPHY_HIP_WAVE_VARIANT=str(wv)),
                        f"prune_wave_kernel NW=4 park=0 {inst};", cut))
        if cut != "levels":
            out.append((f"team-{cut}", dict(HYPHY_HIP_KERNEL="2"), "prune_mfma_kernel NW=4 T=1 on-chain;", cut))
    out.append(("workgroup", dict(HYPHY_HIP_KERNEL="0"), "prune_mfma_kernel NW=4 T=1;", "levels"))
    return out


FORMS = _forms()


def _pairs():
    out = []
    for fid, env, inst, cut in FORMS:
        for name in ALL:
            out.append(pytest.param(name, fid, False, id=f"{name}-{fid}"))
            if cut != "levels" and name in CAN_REROOT:
                out.append(pytest.param(name, fid, True, id=f"{name}-{fid}-rerooted"))
    return out


def _set(monkeypatch, env):
    for k in child.FORM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _forced(name, fid, reroot, monkeypatch, C=1):
    """The switches of a forced form on a case and the text prune_form() must give behind a lazy full pass."""
    _, env, inst, cut = next(f for f in FORMS if f[0] == fid)
    cs = CASES[name]
    env = dict(env, HYPHY_HIP_TUNE="0")
    if cut == "levels":
        env["HYPHY_HIP_CUT"] = "levels"
        want = inst + " levels"
    else:
        I = len(cs["flat_parents"]) - int(cs["L"])
        m = min(int(cut[1:]), I - 1)                    # (a chain cut needs m below the number of internal nodes)
        env["HYPHY_HIP_CHAIN_M"] = str(m)
        want = inst + f" chain m={m}"
    if reroot:
        assert len(tc.reroot_path(cs)) >= 3, name
        env["HYPHY_HIP_REROOT"] = "1"
        if C == 1:
            want += "; re-rooted"
    _set(monkeypatch, env)
    return want


def _check_forced(part, want, what, cs):
    form = part.prune_form()
    if form != want and "occ3" in want and "occ2" in form:
        L, I = int(cs["L"]), len(cs["flat_parents"]) - int(cs["L"])
        if L * 32 + (L + I) * 16 > 24576:               # the launcher's own condition for keeping the leaf codes in LDS
            pytest.skip(f"{what}: the leaf codes of {L} taxa do not fit LDS, the three-waves instantiation does not exist")
    assert form == want, (what, form, want, part.schedule_info())


@pytest.mark.parametrize("name,fid,reroot", _pairs())
def test_every_candidate_forced(name, fid, reroot, monkeypatch):
    want = _forced(name, fid, reroot, monkeypatch)
    cs = tc.scenario(name).cs
    with child.mk(cs) as part:
        child.run_sequence(name, part, f"{name} {fid}{' re-rooted' if reroot else ''}",
                           on_lazy=lambda p, tag: _check_forced(p, want, f"{name} {fid} {tag}", cs))


@pytest.mark.parametrize("fid", [f[0] for f in FORMS if f[0].startswith("wave-") and f[3] in ("levels", "m3")])
@pytest.mark.parametrize("name", tc.CLASS_CASES)
def test_class_batches(name, fid, monkeypatch):
    """evaluate_categories (three classes in one launch) under the form, then each class alone."""
    want = _forced(name, fid, False, monkeypatch, C=3)
    cs = CASES[name]
    ref = sf.case_reference(cs) if name not in _class_refs else _class_refs[name]
    _class_refs[name] = ref
    n = child.nodes(cs)
    with child.mk(cs, C=3) as part:
        for k in range(3):
            got = part.evaluate_categories(n, n, cs["P"], cs["weights"], cs["root_freqs"], q_is_probability=True, per_site=True)
            _hold(f"{name} {fid} classes mixed, pass {k}", got, ref["site_logl"], ref["logl"])
            if k:
                _check_forced(part, want, f"{name} {fid} batch pass {k}", cs)
        for c in range(3):
            for k in range(2):
                got = part.evaluate(n, n, cs["P"][c], cs["root_freqs"], cat=c, q_is_probability=True, per_site=True)
                site = ref["class_site_logl"][c]
                _hold(f"{name} {fid} class {c} alone, pass {k}", got, site, float(np.sum(site * cs["pattern_freq"])))
            _check_forced(part, want, f"{name} {fid} class {c} alone", cs)


_class_refs = {}


def _run_job(args):
    rc, out, rec = child.run_child(args)
    print(out)
    assert rc == 0 and rec is not None, (args, rc, out[-2000:])
    return rec


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("name", list(tc.NEW) + [tc.CONTROL, "conflict_k4_d3_D61_1em15"])
def test_the_tuner_itself(name, kernel):
    rec = _run_job(["tuner", name, kernel])
    print(f"winner: {name} kernel {kernel}: {rec['winners']}")


@pytest.mark.parametrize("name,kernel", [("cat24_on_k4d2_D61", 1), ("cat40_D61_1em6", 2)])
def test_the_tuner_behind_a_pinned_evaluation(name, kernel):
    rec = _run_job(["tuner", name, kernel, "pinned"])
    print(f"winner: {name} kernel {kernel} pinned: {rec['winners']}")


@pytest.mark.parametrize("kernel", [1, 2])
def test_the_tuner_runs_again_when_the_launch_changes_between_one_class_and_a_batch(kernel):
    rec = _run_job(["tuner", "cat12_on_k2d3_D61_cls", kernel, "classes"])
    print(f"winners: classes kernel {kernel}: {rec['winners']}")


@pytest.mark.parametrize("name", tc.NEW)
def test_a_cached_choice_is_taken_over_and_obeys_the_switches(name):
    rec = _run_job(["cache", name])
    print(f"cache: {name}: chose {rec['winners']}, the hole {'bit' if rec['bit'] else 'did not bite'}")
