#!/usr/bin/env python3
"""The first and second log-L derivative of all 125 branch lengths of bench.py's headline shape (mg94_64x10k: 61 states, 64 taxa x
10 000 codons) from ONE hyphy_hip_branch_derivatives_built call with G = Q_b, beside, on the same build,
  * one steady-state full evaluation (build_q + evaluate_built), and
  * one hyphy_hip_branch_trials_built call with 250 trials: what central differences of the same 125 parameters cost.
Writes profiles/branch_derivatives_rate.json.

  python tools/branch_derivatives_rate.py                  times (median of 20 rounds after warm-up, the three alternating inside a
                                                           round), by device events on the partition's stream and by the host clock
                                                           around the calls (each ends in a stream synchronise); then the kernel
                                                           times of the call by `rocprofv3 --kernel-trace --stats` in a run of its own
  python tools/branch_derivatives_rate.py --phase kernels  (the workload that run profiles)
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
        work = dict(full_evaluation=full, derivatives_125=lambda: part.branch_derivatives_built(nodes, base),
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
        d1, d2, skipped = part.branch_derivatives_built(nodes, base)
        again = part.branch_derivatives_built(nodes, base)
        tr = part.branch_trials_built(tn, tc)
        fd1 = (tr[1::2] - tr[0::2]) / (2 * H)
        fd2 = (tr[1::2] - 2 * base_ll + tr[0::2]) / (H * H)
        after = full()
    res = dict(workload="mg94_64x10k", branches=int(len(nodes)), patterns=int(part.S), rounds=ROUNDS, step=H, base_logl=base_ll,
               base_logl_after=after, identical_bits_twice=bool(all(np.array_equal(a, b) for a, b in zip((d1, d2, skipped), again))),
               skipped=int(skipped.sum()), largest_d1=float(np.max(np.abs(d1))), largest_d2=float(np.max(np.abs(d2))),
               # (in a multiplier on the branch's matrix: first derivative d1, second d2; the second difference of a log L of size 1e5
               #  at this step carries 1e5 eps / H^2 = 2e-3 of rounding)
               max_abs_diff_d1_vs_central_differences=float(np.max(np.abs(d1 - fd1))),
               max_abs_diff_d2_vs_central_differences=float(np.max(np.abs(d2 - fd2))))
    for k in work:
        res[k + "_ms_events"] = float(np.median(dev[k]))
        res[k + "_ms_host"] = float(np.median(host[k]))
        res[k + "_ms_events_min_max"] = [float(np.min(dev[k])), float(np.max(dev[k]))]
    return res


def phase_kernels():
    part, pi, nodes, base, tn, tc = setup()
    with part:
        part.build_q(base)
        part.evaluate_built(nodes, nodes, pi)
        for _ in range(5):
            part.branch_derivatives_built(nodes, base)


def kernel_stats():
    tmp = tempfile.mkdtemp(prefix="derivprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    names = ("outside_store", "marg_transpose", "branch_derivs", "derivs_reduce", "deriv_image", "build_q")
    mine = {k: v for k, v in stats.items() if any(w in k for w in names)}
    per_call = {k: v["total_ns"] / 5 / 1e6 for k, v in mine.items()}      # (build_q: one launch of the full pass among six)
    split = dict(walk_ms=sum(v for k, v in per_call.items() if "outside_store" in k or "marg_transpose" in k),
                 phase2_ms=sum(v for k, v in per_call.items() if "branch_derivs" in k),
                 reduction_ms=sum(v for k, v in per_call.items() if "derivs_reduce" in k),
                 generators_ms=sum(v for k, v in per_call.items() if "deriv_image" in k or "build_q" in k))
    return dict(kernels_ms_per_call=per_call, kernels_ms_per_call_total=sum(per_call.values()), **split, kernels=mine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_derivatives_rate.json"))
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
