#!/usr/bin/env python3
"""Sampled ancestral reconstruction (hyphy_hip_sample_ancestral) at bench.py's mg94_64x10k (64 taxa, ~10 k patterns, 61 states),
100 replicates, site = pattern: the median wall time of one call (10 calls after 3 warm-up calls), its kernels' durations from one
`rocprofv3 --kernel-trace --stats` run of their own, and beside them, for scale, the single-thread numpy walk of tests/sample_ref.py
over downloaded conditionals (timed at 4 replicates, reported per replicate and scaled to 100).  Writes profiles/sample_rate.json.

  python tools/sample_rate.py                  wall times, then the kernel times
  python tools/sample_rate.py --phase kernels  (the workload that run profiles)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["HYPHY_HIP_REPEATS"] = "0"

from marginal_rate import setup  # noqa: E402  (the same alignment, model and partition)

R = 100
HOST_R = 4


def times(fn, n, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), calls=n, warm_up_calls=warm)


def phase_wall():
    from tests import sample_ref as sr
    part, flat, Q, pi, nodes, D = setup("mg94_64x10k")
    with part:
        part.evaluate(nodes, nodes, Q, pi)
        rec = dict(states=D, taxa=flat.L, internal_nodes=flat.I, patterns=part.S, replicates=R, draws=R * flat.I * part.S)
        rec["full_pass"] = times(lambda: part.evaluate(nodes, nodes[:0], Q[:0], pi), 20, 20)
        part.evaluate(nodes, nodes, Q, pi)
        part.download_partials()                        # conditionals resident: the calls below do not restore them
        rec["sample_call"] = times(lambda: part.sample_ancestral(R, seed=1), 10, 3)
        rec["sample_call_1_replicate"] = times(lambda: part.sample_ancestral(1, seed=1), 10, 3)
        u = sr.uniforms(1, HOST_R, flat.I, part.S)
        rec["sample_call_supplied_uniforms_%d_replicates" % HOST_R] = times(lambda: part.sample_ancestral(HOST_R, uniforms=u), 5, 1)
        t0 = time.perf_counter()
        cond = part.download_partials()[0]
        t1 = time.perf_counter()
        from hyphy_amd import hip
        P = hip.expm_batch(Q)
        t2 = time.perf_counter()
        want = sr.sample_ref(flat.flat_parents, flat.L, cond, P, pi, u)
        t3 = time.perf_counter()
        got = part.sample_ancestral(HOST_R, seed=1)
        rec["host_walk"] = dict(what="tests/sample_ref.py (numpy, one thread) on download_partials()", replicates_timed=HOST_R,
                                download_partials_ms=(t1 - t0) * 1e3, walk_ms=(t3 - t2) * 1e3,
                                walk_ms_per_replicate=(t3 - t2) * 1e3 / HOST_R,
                                scaled_to_100_replicates_ms=(t1 - t0) * 1e3 + (t3 - t2) * 1e3 / HOST_R * R,
                                equal_columns_share=float((got == want).all(axis=1).mean()))
        rec["host_walk_over_call"] = rec["host_walk"]["scaled_to_100_replicates_ms"] / rec["sample_call"]["median_ms"]
    return rec


def phase_kernels():
    os.environ["HYPHY_HIP_TUNE"] = "0"
    part, flat, Q, pi, nodes, D = setup("mg94_64x10k")
    with part:
        part.evaluate(nodes, nodes, Q, pi)
        part.download_partials()
        for _ in range(5):
            part.sample_ancestral(R, seed=1)


def kernel_stats():
    import csv
    import glob
    tmp = tempfile.mkdtemp(prefix="sampleprof_")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    mine = {k: v for k, v in stats.items() if "sample" in k}
    return dict(sample_kernels_ms_per_call=sum(v["total_ns"] for v in mine.values()) / 5 / 1e6, calls_profiled=5, kernels=mine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rate.json"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    res = dict(workload="mg94_64x10k", site_is_pattern=True,
               method="wall: time.perf_counter around the call, same process, median of the calls after the warm-up calls; "
                      "kernels: one rocprofv3 --kernel-trace --stats run of 5 calls in a process of its own",
               wall=phase_wall())
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats()
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
