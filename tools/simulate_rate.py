#!/usr/bin/env python3
"""Simulation down the tree (hyphy_hip_simulate) at bench.py's mg94_64x10k model (64 taxa, 61 states), 100 replicates of the
alignment's 10 000 codon sites: the median wall time of one call (10 calls after 3 warm-up calls), its kernels' durations from one
`rocprofv3 --kernel-trace --stats` run of their own, and beside them, for scale, the single-thread numpy walk of
tests/simulate_ref.py (timed at 2 replicates, reported per replicate and scaled to 100).  Writes profiles/simulate_rate.json.

  python tools/simulate_rate.py                  wall times, then the kernel times
  python tools/simulate_rate.py --phase kernels  (the workload that run profiles)"""
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
from sample_rate import times  # noqa: E402

R = 100
HOST_R = 2
N_PROFILED = 5


def n_sites_of(name):
    import bench
    return int(bench.WORKLOADS[name]["sites"])


def phase_wall():
    from hyphy_amd import hip
    from tests import simulate_ref as mr
    part, flat, Q, pi, nodes, D = setup("mg94_64x10k")
    n = n_sites_of("mg94_64x10k")
    rows = flat.L + flat.I
    with part:
        part.evaluate(nodes, nodes, Q, pi)
        rec = dict(states=D, taxa=flat.L, nodes=rows, sites=n, replicates=R, columns=R * n, draws=R * n * rows,
                   leaf_bytes_out=R * n * flat.L)
        rec["full_pass"] = times(lambda: part.evaluate(nodes, nodes[:0], Q[:0], pi), 20, 20)
        rec["simulate_call"] = times(lambda: part.simulate(R, n, seed=1), 10, 3)
        rec["simulate_call_with_internal"] = times(lambda: part.simulate(R, n, seed=1, with_internal=True), 10, 3)
        rec["simulate_call_1_replicate"] = times(lambda: part.simulate(1, n, seed=1), 10, 3)
        cls = np.zeros((R, n), dtype=np.int64)
        rec["simulate_call_class_of_site_given"] = times(lambda: part.simulate(R, n, cls, seed=1), 5, 1)
        u = mr.uniforms(1, HOST_R, rows, n)
        rec["simulate_call_supplied_uniforms_%d_replicates" % HOST_R] = times(lambda: part.simulate(HOST_R, n, uniforms=u), 5, 1)
        out = np.empty((R, flat.L, n), dtype=np.int8)
        rec["numpy_empty_and_fill_of_the_result"] = times(lambda: out.fill(-2), 10, 3)
        t0 = time.perf_counter()
        P = hip.expm_batch(Q)
        t1 = time.perf_counter()
        want = mr.simulate_ref(flat.flat_parents, flat.L, P, pi, u)
        t2 = time.perf_counter()
        got = part.simulate(HOST_R, n, seed=1, with_internal=True)
        rec["host_walk"] = dict(what="tests/simulate_ref.py (numpy, one thread) on hip.expm_batch(Q)", replicates_timed=HOST_R,
                                expm_batch_ms=(t1 - t0) * 1e3, walk_ms=(t2 - t1) * 1e3, walk_ms_per_replicate=(t2 - t1) * 1e3 / HOST_R,
                                scaled_to_100_replicates_ms=(t2 - t1) * 1e3 / HOST_R * R,
                                equal_columns_share=float((got == want).all(axis=1).mean()))
        rec["host_walk_over_call"] = rec["host_walk"]["scaled_to_100_replicates_ms"] / rec["simulate_call"]["median_ms"]
    return rec


def phase_kernels():
    os.environ["HYPHY_HIP_TUNE"] = "0"
    part, flat, Q, pi, nodes, D = setup("mg94_64x10k")
    n = n_sites_of("mg94_64x10k")
    with part:
        part.evaluate(nodes, nodes, Q, pi)
        for _ in range(N_PROFILED):
            part.simulate(R, n, seed=1)


def kernel_stats():
    import csv
    import glob
    tmp = tempfile.mkdtemp(prefix="simprof_")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    mine = {k: v for k, v in stats.items() if "simulate" in k}
    return dict(simulate_kernels_ms_per_call=sum(v["total_ns"] for v in mine.values()) / N_PROFILED / 1e6, calls_profiled=N_PROFILED,
                kernels=mine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate_rate.json"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    res = dict(workload="mg94_64x10k", sites_are_free=True,
               method="wall: time.perf_counter around the call, same process, median of the calls after the warm-up calls; "
                      "kernels: one rocprofv3 --kernel-trace --stats run of %d calls in a process of its own" % N_PROFILED,
               wall=phase_wall())
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats()
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
