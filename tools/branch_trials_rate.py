#!/usr/bin/env python3
"""The 250 one-branch evaluations of a finite-difference gradient (mg94_64x10k: two per branch, the alpha + h and beta + h matrices)
from ONE hyphy_hip_branch_trials_built call, against the two ways the library offered before on the same build:
  (a) one partial-update evaluate_built per trial, listing the paths of the previous and the current branch (the host's set /
      compute / restore sequence);
  (b) per branch a branch_cache_build, two branch_cache_evaluate and an ordinary partial update that puts the matrix back.
Writes profiles/branch_trials_rate.json.

  python tools/branch_trials_rate.py                  wall times (median of 20 after warm-up), then the kernel times of the call by
                                                      `rocprofv3 --kernel-trace --stats` in a run of its own
  python tools/branch_trials_rate.py --phase kernels  (the workload that run profiles)
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
H = 1e-4          # relative step of the trial parameters
OMEGA = 0.3
T_BRANCH = 0.05


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
    base = np.stack([np.full(B, T_BRANCH), np.full(B, T_BRANCH * OMEGA)], axis=1)          # [B, 2]: (synRate, nonSynRate)
    tn = np.repeat(nodes, 2)                                                             # trial t: branch t // 2, parameter t % 2
    tc = np.repeat(base, 2, axis=0)
    tc[0::2, 0] *= 1.0 + H
    tc[1::2, 1] *= 1.0 + H
    return part, flat, T, pi, nodes, base, tn, tc


def dense_q(T, co):
    Q = np.einsum("nk,kij->nij", co, T)
    idx = np.arange(Q.shape[1])
    Q[:, idx, idx] = 0.0
    Q[:, idx, idx] = -Q.sum(axis=2)
    return Q


def median_ms(fn, n, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def phase_wall():
    part, flat, T, pi, nodes, base, tn, tc = setup()
    paths = [np.asarray(flat.path_update_nodes(int(b)), dtype=np.int64) for b in nodes]
    with part:
        def full():
            part.build_q(base)
            return part.evaluate_built(nodes, nodes, pi)
        base_ll = full()
        t_end = time.perf_counter() + 1.5                   # clocks up and every shape seen before anything is timed
        while time.perf_counter() < t_end:
            part.branch_trials_built(tn, tc)
        one_call = part.branch_trials_built(tn, tc)
        call_ms = median_ms(lambda: part.branch_trials_built(tn, tc), 20)

        def route_a():
            out = np.zeros(len(tn))
            prev = None
            for t in range(len(tn)):
                b = int(tn[t])
                if prev is None or prev == b:
                    un, qn, co = paths[b], np.array([b]), tc[t: t + 1]
                else:
                    un = np.union1d(paths[prev], paths[b])
                    qn, co = np.array([prev, b]), np.stack([base[prev], tc[t]])
                part.build_q(np.ascontiguousarray(co))
                out[t] = part.evaluate_built(un, qn, pi)
                prev = b
            part.build_q(base[prev: prev + 1])
            part.evaluate_built(paths[prev], np.array([prev]), pi)
            return out
        via_a = route_a()
        a_ms = median_ms(route_a, 3, warm=0)
        Qt = dense_q(T, tc)

        def route_b():
            out = np.zeros(len(tn))
            for b in nodes:
                b = int(b)
                part.branch_cache_build(b)
                for t in (2 * b, 2 * b + 1):
                    out[t] = part.branch_cache_evaluate(b, Qt[t])
                part.build_q(base[b: b + 1])
                part.evaluate_built(paths[b], np.array([b]), pi)
            return out
        full()
        via_b = route_b()
        b_ms = median_ms(route_b, 3, warm=0)
        again = part.branch_trials_built(tn, tc)
        after = full()
    return dict(workload="mg94_64x10k", trials=int(len(tn)), branches=int(len(nodes)), patterns=int(part.S), step=H,
                base_logl=base_ll, base_logl_after=after, identical_bits_after_the_other_routes=bool(np.array_equal(one_call, again)),
                one_call_ms=call_ms, partial_updates_ms=a_ms, branch_cache_ms=b_ms,
                speedup_vs_partial_updates=a_ms / call_ms, speedup_vs_branch_cache=b_ms / call_ms,
                max_abs_diff_vs_partial_updates=float(np.max(np.abs(one_call - via_a))),
                max_abs_diff_vs_branch_cache=float(np.max(np.abs(one_call - via_b))),
                largest_gradient_entry=float(np.max(np.abs(one_call - base_ll) / (np.repeat(base, 2, axis=0)[np.arange(len(tn)), np.arange(len(tn)) % 2] * H))))


def phase_kernels():
    part, flat, T, pi, nodes, base, tn, tc = setup()
    with part:
        part.build_q(base)
        part.evaluate_built(nodes, nodes, pi)
        for _ in range(5):
            part.branch_trials_built(tn, tc)


def kernel_stats():
    tmp = tempfile.mkdtemp(prefix="trialsprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    mine = {k: v for k, v in stats.items() if any(w in k for w in ("outside_store", "branch_trials", "trials_reduce", "marg_transpose"))}
    expm = {k: v for k, v in stats.items() if "expm" in k}
    per_call = {k: v["total_ns"] / 5 / 1e6 for k, v in mine.items()}
    expm_ms = sum(v["total_ns"] for v in expm.values()) / 1e6      # (one full pass of 125 matrices + 5 calls of 250)
    total = sum(per_call.values())
    phase1 = sum(v for k, v in per_call.items() if "outside_store" in k or "marg_transpose" in k)
    return dict(kernels_ms_per_call=per_call, kernels_ms_per_call_total=total, phase1_ms=phase1,
                phase1_share_of_the_call_kernels=phase1 / total if total else None, expm_kernels_ms_whole_run=expm_ms,
                kernels={k: v for k, v in stats.items() if k in mine or k in expm})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_trials_rate.json"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    res = dict(wall=phase_wall())
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats()
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
