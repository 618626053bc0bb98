#!/usr/bin/env python3
"""Every nearest-neighbour interchange of the headline tree (mg94_64x10k of BASELINE.json: 64 taxa x 10 000 codons, 61 states) scored
by ONE hyphy_hip_nni_scores call, against as many synchronous full evaluations of the resident partition as there are moves — a
lower bound on what scoring the neighbours took before (a partition per neighbour, an upload and a full evaluation each; the
evaluations timed here update no matrix and rebuild nothing).  Writes profiles/nni_rate.md.

  python tools/nni_rate.py                  wall times (host clock around synchronous calls; 40 rounds of 10 calls and one loop of
                                            evaluations in turn, after warm-up: medians, spread and the ratio per round), then
                                            the kernel times of the call by `rocprofv3 --kernel-trace --stats` in a run of its own
  python tools/nni_rate.py --phase kernels  (the workload that run profiles)
The plain form (HYPHY_HIP_REPEATS=0) and no tuner trials (HYPHY_HIP_TUNE=0) throughout."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["HYPHY_HIP_REPEATS"] = "0"
os.environ["HYPHY_HIP_TUNE"] = "0"
OMEGA = 0.3
T_BRANCH = 0.05
CALLS = 5             # calls of the profiled run


def setup():
    import bench
    from hyphy_amd import data, hip
    wl = bench.WORKLOADS["mg94_64x10k"]
    syn = data.evolve(wl["taxa"], wl["sites"], wl["unit"], seed=wl["seed"], p_change=wl.get("p_change", 0.04))
    pd = data.from_states(syn.states, 61, compress_patterns=True)
    flat = syn.flat
    B = flat.n_branches
    T, pi = bench.templates_for(3)
    part = hip.HipPartition(61, flat.flat_parents, flat.L, pd.leaf_codes, None, pd.pattern_freq)
    part.set_q_templates(T)
    nodes = np.arange(B, dtype=np.int64)
    base = np.stack([np.full(B, T_BRANCH), np.full(B, T_BRANCH * OMEGA)], axis=1)
    moves = hip.plan_nni(flat.flat_parents, flat.L)
    return part, flat, pi, nodes, base, moves


ROUNDS, CALLS_PER_ROUND = 40, 10   # timed: 400 calls (about 1.5 s) and 40 loops of evaluations (about 0.75 s), alternating


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(ts):
    ts = np.asarray(ts)
    return dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)),
                min=float(ts.min()), max=float(ts.max()), n=int(len(ts)))


def phase_wall():
    part, flat, pi, nodes, base, moves = setup()
    none = np.zeros(0, dtype=np.int64)
    with part:
        part.build_q(base)
        base_ll = part.evaluate_built(nodes, nodes, pi)

        def evaluations():
            for _ in range(len(moves)):
                part.evaluate(nodes, none, None, pi)
        t_end = time.perf_counter() + 1.5                   # clocks up and every shape seen before anything is timed
        while time.perf_counter() < t_end:
            part.nni_scores(moves)
            evaluations()
        first = part.nni_scores(moves)
        calls, evals, ratios = [], [], []
        for _ in range(ROUNDS):                             # the two in turn, so that what else the machine does falls on both
            c = [clock(lambda: part.nni_scores(moves)) for _ in range(CALLS_PER_ROUND)]
            e = clock(evaluations)
            calls += c
            evals.append(e)
            ratios.append(e / float(np.median(c)))
        again = part.nni_scores(moves)
        after = part.evaluate(nodes, none, None, pi)
    call, ev, ra = spread(calls), spread(evals), spread(ratios)
    return dict(workload="mg94_64x10k", moves=int(len(moves)), branches=int(len(nodes)), patterns=int(part.S), base_logl=base_ll,
                base_logl_after=after, identical_bits=bool(np.array_equal(first, again)), best_score=float(np.max(first)),
                scores_above_base=int(np.sum(first > base_ll)), rounds=ROUNDS, one_call_ms=call["median"], one_call=call,
                evaluations_ms=ev["median"], evaluations=ev, one_evaluation_ms=ev["median"] / len(moves),
                ratio=ev["median"] / call["median"], ratio_per_round=ra)


def phase_kernels():
    part, flat, pi, nodes, base, moves = setup()
    with part:
        part.build_q(base)
        part.evaluate_built(nodes, nodes, pi)
        for _ in range(CALLS):
            part.nni_scores(moves)


def kernel_stats():
    tmp = tempfile.mkdtemp(prefix="nniprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: float(r["TotalDurationNs"]) / CALLS / 1e6 for r in rows}
    mine = {k: v for k, v in stats.items() if any(w in k for w in ("outside_store", "nni_", "trials_reduce", "marg_transpose"))}
    phase1 = sum(v for k, v in mine.items() if "outside_store" in k or "marg_transpose" in k)
    phase2 = sum(v for k, v in mine.items() if "nni_" in k)
    return dict(kernels_ms_per_call=mine, total_ms=sum(mine.values()), phase1_ms=phase1, phase2_ms=phase2)


def report(res):
    w, k = res["wall"], res.get("rocprofv3")
    c, e, r = w["one_call"], w["evaluations"], w["ratio_per_round"]
    out = ["# Every NNI neighbour of the headline tree from one call, against one full evaluation per neighbour", "",
           f"`tools/nni_rate.py` on an MI355X: {w['workload']}, {w['branches']} branches, {w['patterns']} patterns, "
           f"{w['moves']} moves (`plan_nni`).  Host clock around synchronous calls after 1.5 s of warm-up on both; {w['rounds']} rounds, "
           f"each {c['n'] // w['rounds']} calls and then one loop of {w['moves']} evaluations, so the two alternate within one run; "
           "HYPHY_HIP_REPEATS=0, HYPHY_HIP_TUNE=0.", "",
           "| | n | median ms | 10 % .. 90 % | min .. max |", "|---|---|---|---|---|",
           f"| one `nni_scores` call over all {w['moves']} moves | {c['n']} | {c['median']:.3f} | {c['p10']:.3f} .. {c['p90']:.3f} | "
           f"{c['min']:.3f} .. {c['max']:.3f} |",
           f"| {w['moves']} synchronous full evaluations of the resident partition (no matrix updated) | {e['n']} | {e['median']:.3f} | "
           f"{e['p10']:.3f} .. {e['p90']:.3f} | {e['min']:.3f} .. {e['max']:.3f} |",
           f"| one such evaluation | | {w['one_evaluation_ms']:.4f} | | |", "",
           f"Ratio (evaluations / call) of the medians: **{w['ratio']:.2f}x**; per round (the loop over the median of the round's "
           f"calls) median {r['median']:.2f}, 10 % .. 90 % {r['p10']:.2f} .. {r['p90']:.2f}, min .. max {r['min']:.2f} .. {r['max']:.2f}.  "
           "The evaluations are a lower bound on the cost per neighbour before: a new partition, an upload and every exponential come "
           "on top.", "",
           f"Two calls gave identical bits: {w['identical_bits']}.  log L before {w['base_logl']!r}, after {w['base_logl_after']!r}; "
           f"best score {w['best_score']!r}, {w['scores_above_base']} scores above log L.", ""]
    if k:
        out += ["## Kernels of one call (`rocprofv3 --kernel-trace --stats`, a run of its own, per call of 5)", "",
                "| kernel | ms per call |", "|---|---|"]
        out += [f"| `{n.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:90]}` | {v:.3f} |" for n, v in sorted(k["kernels_ms_per_call"].items(), key=lambda kv: -kv[1])]
        share1 = k["phase1_ms"] / k["total_ms"] if k["total_ms"] else float("nan")
        share2 = k["phase2_ms"] / k["total_ms"] if k["total_ms"] else float("nan")
        out += ["", f"Phase 1 (transposition and outside walk) {k['phase1_ms']:.3f} ms = {100 * share1:.1f} % of the call's kernel time, "
                f"phase 2 (`nni_kernel`) {k['phase2_ms']:.3f} ms = {100 * share2:.1f} %; kernels in all {k['total_ms']:.3f} ms of the "
                f"{w['one_call_ms']:.3f} ms wall time (the rest: uploads of the tables, the pool, the download, launches).", "",
                f"Where the time goes: the walk of phase 1 alone takes as long as {k['phase1_ms'] / w['one_evaluation_ms']:.1f} of the "
                f"evaluations (it forms and stores V and U of every node through memory, one wave per tile), phase 2 as long as "
                f"{k['phase2_ms'] / w['one_evaluation_ms']:.1f}, and the host's share of the call as long as "
                f"{(w['one_call_ms'] - k['total_ms']) / w['one_evaluation_ms']:.1f}; a count of matrix instructions alone "
                "(one walk plus at most 5 products per move against 62 products per evaluation) would put the ratio near 9.", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nni_rate.md"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    res = dict(wall=phase_wall())
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats()
    open(a.out, "w").write(report(res))
    print(json.dumps(res, indent=1))
    if not res["wall"]["ratio"] > 1.0:
        raise SystemExit("the call is not faster than one evaluation per move")


if __name__ == "__main__":
    main()
