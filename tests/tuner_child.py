"""What tests/test_gpu_tuner_forms.py runs on the device: the one call sequence of tests/tuner_cases.py under a forced form, and the
jobs that need a process of their own because HYPHY_HIP_TUNE_CACHE is read once per process:

    python -m tests.tuner_child tuner CASE KERNEL [pinned|classes]     the tuner itself, every partition measuring for itself
    python -m tests.tuner_child cache CASE                             a second and a third partition taking a choice over

Each job holds everything it computes to tests/scalefree.py through tests/hold.py, prints what the tuner chose, and ends with a
line "RESULT {json}"; any failed check ends the process with the assertion.
"""
import json
import os
import re
import sys

import numpy as np

from tests import scalefree as sf
from tests import tuner_cases as tc
from tests.hold import ATOL, LOG_SCALER, RTOL, _hold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_SWITCHES = ("HYPHY_HIP_TUNE", "HYPHY_HIP_TUNE_CACHE", "HYPHY_HIP_KERNEL", "HYPHY_HIP_SLOTS", "HYPHY_HIP_WAVE_VARIANT", "HYPHY_HIP_CHAIN_M",
                 "HYPHY_HIP_CUT", "HYPHY_HIP_FRAGMENT", "HYPHY_HIP_REROOT", "HYPHY_HIP_REPEATS", "HYPHY_HIP_POISON")


def mk(cs, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def nodes(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def full(cs, part, P):
    n = nodes(cs)
    return part.evaluate(n, n, P, cs["root_freqs"], q_is_probability=True, per_site=True)


def hold(what, got, ref):
    _hold(what, got, ref["site_logl"], ref["logl"])


def hold_downloaded(what, cache, counts, ref):
    """download_partials as test_gpu_rescale.py::test_downloaded_conditionals_and_counts holds it: conditionals divided by their
    largest element against the reference's, and log(largest element) - 64 ln2 count = the reference's log-magnitude."""
    top = cache.max(axis=2)
    zero = ~(ref["cond"].max(axis=2) > 0)
    assert np.array_equal(top == 0, zero), what
    norm = cache / np.where(top > 0, top, 1.0)[:, :, None]
    assert np.allclose(norm, ref["cond"], rtol=1e-9, atol=1e-12), what
    with np.errstate(divide="ignore"):
        mag = np.log(top) - LOG_SCALER * counts
    ok = ~zero
    assert np.all(np.abs(mag[ok] - ref["log_mag"][ok]) <= RTOL * np.abs(ref["log_mag"][ok]) + ATOL), what


def run_sequence(name, part, what, on_lazy=None, first=True):
    """The sequence (tests/test_gpu_tuner_forms.py's docstring) on a one-class partition of case ``name``.  ``on_lazy(part, tag)`` is
    called behind every lazy full pass.  first=False: the partition has had its persisting and lazy passes already."""
    sc = tc.scenario(name)
    cs, P = sc.cs, sc.P

    def lazy(tag, k, settle=True):
        if settle:   # (the first full pass behind a partial update, a pin or a download stores every node again: the next one is lazy)
            hold(f"{what}: {tag}, the pass in front", full(cs, part, P[k]), sc.ref(k))
        hold(f"{what}: {tag}", full(cs, part, P[k]), sc.ref(k))
        if on_lazy:
            on_lazy(part, tag)

    if first:
        hold(f"{what}: 1 persisting pass", full(cs, part, P[0]), sc.ref(0))
        lazy("2 lazy pass", 0, settle=False)
    lazy("2 second lazy pass", 0, settle=False)
    for step, code in ((1, sc.leaf), (2, sc.inner)):
        ch = np.array([code], dtype=np.int64)
        got = part.evaluate(ch, ch, P[step][ch], cs["root_freqs"], q_is_probability=True, per_site=True)
        hold(f"{what}: {2 + step} partial update of branch {code}", got, sc.ref(step))
    lazy("5 lazy pass", 2)
    part.set_pinned_states(sc.pin, sc.states)
    try:
        got = full(cs, part, P[2])
    finally:
        part.set_pinned_states(None)
    hold(f"{what}: 6 pinned at {sc.pin}", got, sc.ref("pin"))
    lazy("6 pass behind the pin", 2)
    part.branch_cache_build(sc.bc)
    got = part.branch_cache_evaluate(sc.bc, P[3][sc.bc], q_is_probability=True, per_site=True)
    hold(f"{what}: 7 branch cache at {sc.bc}", got, sc.ref(3))
    cache, counts = part.download_partials()
    hold_downloaded(f"{what}: 8 download", cache, counts, sc.ref("cond"))
    lazy("9 last pass", 2)


# ---- what the tuner's labels mean in the words of HipPartition.prune_form() -------------------------------------------------------

def park_by_lds(cs):
    """Parking slots of the wave kernel's production instantiation at 49-64 states: two where two tiles and the leaf codes fit an
    eighth of the CU's LDS (up to 128 taxa), else one."""
    return 2 if 2 * 8192 + int(cs["L"]) * 32 <= 20480 else 1


def form_of_label(label, cs):
    """(substrings prune_form() must contain, substrings it must not) for a candidate label of the tuner's report."""
    m = re.fullmatch(r"(rr[01]/)?(occ3/)?(wg-kernel|team/m|levels|m)(\d+)", label)
    assert m, label
    rr, occ3, kind, num = m.groups()
    want, never = ["NW=4"], []
    if kind in ("wg-kernel", "team/m"):
        want.append("prune_mfma_kernel")
        want.append("T=1 on-chain; chain m=%s" % num if kind == "team/m" else "T=1; levels")
    else:
        want.append("prune_wave_kernel")
        want.append("park=0 occ3;" if occ3 else "park=%d occ2;" % park_by_lds(cs))
        want.append("; levels" if kind == "levels" else "; chain m=%s" % num)
    (want if rr else never).append("re-rooted")
    return want, never


def check_form(form, want, never, what):
    assert all(w in form for w in want) and not any(n in form for n in never), (what, form, want, never)


def parse_report(info):
    """([(label, microseconds)] in the order measured, label chosen) of a schedule_info() text; ([], label) when taken over."""
    head = info.split(" [current:")[0]
    cands = [(m.group(1), float(m.group(2))) for m in re.finditer(r"(\S+):([0-9.]+)us", head)]
    chosen = re.search(r"-> (\S+)", head)
    assert chosen, info
    return cands, chosen.group(1)


def check_report(info, cs, kernel, rr_possible, what):
    """What the report must list (module docstring of the test).  rr_possible: re-rooted schedules exist for the pass the tuner ran
    behind (one class, a one-class partition, no pinned node).  Returns the chosen label."""
    cands, chosen = parse_report(info)
    assert cands, (what, "no candidate was measured", info)
    labels = [c[0] for c in cands]
    stage1 = [(lab, t) for lab, t in cands if not lab.startswith(("occ3/", "rr"))]
    chains = [lab for lab, _ in stage1 if re.fullmatch(r"(team/)?m\d+", lab)]
    assert chains, (what, info)
    if kernel == 1:
        assert "levels0" in labels, (what, info)
    else:   # (the row-split kernel on chains has no level-peeled candidate: its stage one is chain cuts only)
        assert all(lab.startswith("team/m") for lab, _ in stage1), (what, info)
    best = min(t for _, t in stage1)
    winners = [lab for lab, t in stage1 if t == best]     # (times are printed to 0.1 us: a tie leaves either outcome open)
    chain_won = [lab in chains for lab in winners]
    has_occ3 = any(lab.startswith("occ3/") for lab in labels)
    has_rr = any(lab.startswith("rr") for lab in labels)
    path = tc.reroot_path(cs)
    if all(chain_won):
        assert has_occ3 == (kernel == 1), (what, info)
        assert has_rr == (len(path) > 0 and rr_possible), (what, info)
    elif not any(chain_won):
        assert not has_occ3 and not has_rr, (what, info)
    if has_rr:
        assert "rr0/" in " ".join(labels), (what, info)
    assert chosen in labels, (what, info)
    return chosen


# ---- jobs ---------------------------------------------------------------------------------------------------------------------------

def job_tuner(name, kernel, variant):
    os.environ.update(HYPHY_HIP_TUNE_CACHE="0", HYPHY_HIP_KERNEL=str(kernel), HYPHY_HIP_POISON="1", HYPHY_HIP_REPEATS="0")
    os.environ.pop("HYPHY_HIP_TUNE", None)
    all_cases = tc.cases_by_name()
    res = {"case": name, "kernel": kernel, "variant": variant}
    if variant == "classes":
        cs = all_cases[name]
        ref = sf.case_reference(cs)
        n = nodes(cs)
        with mk(cs, C=3) as part:
            def batch(tag):
                got = part.evaluate_categories(n, n, cs["P"], cs["weights"], cs["root_freqs"], q_is_probability=True, per_site=True)
                hold(f"{name} tuner, {tag}", got, ref)

            def one(c, tag):
                got = part.evaluate(n, n, cs["P"][c], cs["root_freqs"], cat=c, q_is_probability=True, per_site=True)
                want = ref["class_site_logl"][c]
                _hold(f"{name} tuner, {tag}", got, want, float(np.sum(want * cs["pattern_freq"])))
            reports = []
            batch("persisting batch")
            batch("batch behind which the tuner runs")
            reports.append(check_report(part.schedule_info(), cs, kernel, False, name))
            batch("batch under the winner")
            check_form(part.prune_form(), *form_of_label(reports[-1], cs), what=name)
            for rnd in range(2):                      # one class / batch / one class: the tuner runs again at every switch
                for c in range(3):
                    one(c, f"round {rnd}, class {c} alone")
                    one(c, f"round {rnd}, class {c} alone again")
                reports.append(check_report(part.schedule_info(), cs, kernel, False, name))
                one(0, f"round {rnd}, class 0 under the winner")
                check_form(part.prune_form(), *form_of_label(reports[-1], cs), what=name)
                batch(f"round {rnd}, batch")
                batch(f"round {rnd}, batch again")
                reports.append(check_report(part.schedule_info(), cs, kernel, False, name))
                batch(f"round {rnd}, batch under the winner")
                check_form(part.prune_form(), *form_of_label(reports[-1], cs), what=name)
        res["winners"] = reports
        return res
    sc = tc.scenario(name)
    cs = sc.cs
    with mk(cs) as part:
        hold(f"{name} tuner: pass 0 (persisting)", full(cs, part, sc.P[0]), sc.ref(0))
        if variant == "pinned":                       # the first steady-state pass, the one the tuner runs behind, has a pinned node
            part.set_pinned_states(sc.pin, sc.states)
            try:
                got = full(cs, part, sc.P[0])
            finally:
                part.set_pinned_states(None)
            hold(f"{name} tuner: pass 1, pinned at {sc.pin}", got, sc.ref("pin0"))
        else:
            hold(f"{name} tuner: pass 1 (the tuner's)", full(cs, part, sc.P[0]), sc.ref(0))
        info = part.schedule_info()
        chosen = check_report(info, cs, kernel, variant != "pinned", name)
        print(f"{name} kernel {kernel} {variant or ''}: {info}")
        want, never = form_of_label(chosen, cs)
        for k in (2, 3):
            hold(f"{name} tuner: pass {k} under {chosen}", full(cs, part, sc.P[0]), sc.ref(0))
            check_form(part.prune_form(), want, never, f"{name} pass {k}")
        run_sequence(name, part, f"{name} tuned to {chosen}", on_lazy=lambda p, tag: check_form(p.prune_form(), want, never, tag), first=False)
        assert part.schedule_info().split(" [current:")[0] == info.split(" [current:")[0], "the tuner ran again"
    res["winners"] = [chosen]
    return res


def job_cache(name):
    os.environ.update(HYPHY_HIP_KERNEL="1", HYPHY_HIP_POISON="1", HYPHY_HIP_REPEATS="0")
    for k in ("HYPHY_HIP_TUNE", "HYPHY_HIP_TUNE_CACHE"):
        os.environ.pop(k, None)
    sc = tc.scenario(name)
    cs = sc.cs
    with mk(cs) as a:
        for k in range(3):
            hold(f"{name} A pass {k}", full(cs, a, sc.P[0]), sc.ref(0))
        chosen = check_report(a.schedule_info(), cs, 1, True, name)
        form_a = a.prune_form()
    check_form(form_a, *form_of_label(chosen, cs), what=f"{name} A")
    other = tc.other_data(cs, 77)
    ref_b = sf.case_reference(other)
    with mk(other) as b:
        for k in range(4):
            hold(f"{name} B pass {k}", full(other, b, other["P"]), ref_b)
        info_b = b.schedule_info()
        assert "as an earlier partition of this process" in info_b and parse_report(info_b) == ([], chosen), info_b
        assert b.prune_form() == form_a, (b.prune_form(), form_a)
    bit = "occ3/" in chosen
    forms = {}
    for env, must in ((dict(HYPHY_HIP_SLOTS="4"), "park=2 occ2;"), (dict(HYPHY_HIP_SLOTS="3"), "park=1 occ2;"), (dict(HYPHY_HIP_WAVE_VARIANT="0"), " occ2;")):
        os.environ.update(env)
        try:
            with mk(other) as c:
                for k in range(4):
                    hold(f"{name} C {env} pass {k}", full(other, c, other["P"]), ref_b)
                forms[str(env)] = c.prune_form()
                assert must in c.prune_form(), (env, c.prune_form(), c.schedule_info())
        finally:
            for k in env:
                os.environ.pop(k)
    print(f"{name}: A chose {chosen}; the cache hole {'bit (A runs occ3)' if bit else 'did not bite (A does not run occ3)'}; C: {forms}")
    return {"case": name, "winners": [chosen], "bit": bit}


def run_child(args, timeout=240):
    """A fresh process for one job; (exit status, its whole output, the RESULT record or None).  Nothing is retried."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in FORM_SWITCHES}
    r = subprocess.run([sys.executable, "-m", "tests.tuner_child"] + [str(a) for a in args], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    out = r.stdout + r.stderr
    rec = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    return r.returncode, out, json.loads(rec[-1]) if rec else None


def main(argv):
    if argv[0] == "tuner":
        res = job_tuner(argv[1], int(argv[2]), argv[3] if len(argv) > 3 else "")
    elif argv[0] == "cache":
        res = job_cache(argv[1])
    else:
        raise SystemExit(f"unknown job {argv[0]}")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
