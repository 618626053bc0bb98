#!/usr/bin/env python3
"""The gradient of log L in all 125 x 2 template coefficients of bench.py's headline shape (mg94_64x10k: 61 states, 64 taxa x 10 000
codons, K = 2) from ONE hyphy_hip_branch_gradient_built call, beside, on the same build, what the host does today for the same
information:
  * one hyphy_hip_branch_trials_built call with 250 trials (central differences of the 125 branch-local parameters), plus
  * 2 x G full evaluations (build_q + evaluate_built) for G = 6 global parameters.
Writes profiles/branch_gradient_rate.json.

  python tools/branch_gradient_rate.py                  times (median of 20 rounds after warm-up, the three alternating inside a
                                                        round), by device events on the partition's stream and by the host clock
                                                        around the calls; then the kernel times of the call by
                                                        `rocprofv3 --kernel-trace --stats` in a run of its own
  python tools/branch_gradient_rate.py --phase kernels  (the workload that run profiles)
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
H = 1e-4          # relative step of the central differences
OMEGA = 0.3
T_BRANCH = 0.05
ROUNDS = 20
GLOBALS = 6       # global parameters the host differences today: two full evaluations each


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
    tn = np.repeat(nodes, 2)                                                             # trial t: branch t // 2, length x (1 -+ H)
    tc = np.repeat(base, 2, axis=0)
    tc[0::2] *= 1.0 - H
    tc[1::2] *= 1.0 + H
    return part, pi, nodes, base, tn, tc


def phase_wall():
    import torch
    part, pi, nodes, base, tn, tc = setup()
    with part:
        stream = torch.cuda.ExternalStream(part.stream())

        def full():
            part.build_q(base)
            return part.evaluate_built(nodes, nodes, pi)
        work = dict(full_evaluation=full, gradient_125x2=lambda: part.branch_gradient_built(nodes, base),
                    trials_250=lambda: part.branch_trials_built(tn, tc))
        base_ll = full()
        t_end = time.perf_counter() + 1.5                   # clocks up and every shape seen before anything is timed
        while time.perf_counter() < t_end:
            for fn in work.values():
                fn()
        host = {k: [] for k in work}
        dev = {k: [] for k in work}
        for _ in range(ROUNDS):
            for k, fn in work.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e3)
                dev[k].append(e0.elapsed_time(e1))
        g, skipped = part.branch_gradient_built(nodes, base)
        again = part.branch_gradient_built(nodes, base)
        tr = part.branch_trials_built(tn, tc)
        fd1 = (tr[1::2] - tr[0::2]) / (2 * H)               # in a multiplier on the branch's matrix: sum_k x_k grad_k
        after = full()
    res = dict(workload="mg94_64x10k", branches=int(len(nodes)), K=2, patterns=int(part.S), rounds=ROUNDS, step=H, globals=GLOBALS,
               base_logl=base_ll, base_logl_after=after,
               identical_bits_twice=bool(all(np.array_equal(a, b) for a, b in zip((g, skipped), again))), skipped=int(skipped.max()),
               largest_gradient=float(np.max(np.abs(g))),
               max_abs_diff_x_dot_grad_vs_central_differences=float(np.max(np.abs((base * g).sum(axis=1) - fd1))))
    for k in work:
        res[k + "_ms_events"] = float(np.median(dev[k]))
        res[k + "_ms_host"] = float(np.median(host[k]))
        res[k + "_ms_events_min_max"] = [float(np.min(dev[k])), float(np.max(dev[k]))]
    res["finite_differences_ms_events"] = res["trials_250_ms_events"] + 2 * GLOBALS * res["full_evaluation_ms_events"]
    res["finite_differences_over_gradient"] = res["finite_differences_ms_events"] / res["gradient_125x2_ms_events"]
    return res


def phase_kernels():
    part, pi, nodes, base, tn, tc = setup()
    with part:
        part.build_q(base)
        part.evaluate_built(nodes, nodes, pi)
        for _ in range(5):
            part.branch_gradient_built(nodes, base)


def kernel_stats():
    tmp = tempfile.mkdtemp(prefix="gradprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    names = ("outside_store", "marg_transpose", "grad_weight", "grad_accum", "grad_reduce", "frechet_adjoint", "grad_contract", "build_q")
    mine = {k: v for k, v in stats.items() if any(w in k for w in names)}
    per_call = {k: v["total_ns"] / 5 / 1e6 for k, v in mine.items()}      # (build_q: one launch of the full pass among six)
    split = dict(phase1_walk_ms=sum(v for k, v in per_call.items() if "outside_store" in k or "marg_transpose" in k),
                 accumulation_ms=sum(v for k, v in per_call.items() if "grad_accum" in k),
                 adjoint_ms=sum(v for k, v in per_call.items() if "frechet_adjoint" in k),
                 rest_ms=sum(v for k, v in per_call.items() if any(w in k for w in ("grad_weight", "grad_reduce", "grad_contract", "build_q"))))
    return dict(kernels_ms_per_call=per_call, kernels_ms_per_call_total=sum(per_call.values()), **split, kernels=mine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_gradient_rate.json"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    res = dict(times=phase_wall())
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats()
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
