#!/usr/bin/env python3
"""Marginal ancestral reconstruction: the one-pass device call (hyphy_hip_marginal_ancestral) against the pinned route it replaces
(I*(D-1) partial-update evaluations with a node pinned, as RecoverAncestralSequencesMarginal runs them) and against one plain full
pruning pass, on bench.py's alignments (same generator and seeds).  Writes profiles/marginal_rate.json.

  python tools/marginal_rate.py                  wall times (mg94_64x10k: full support and MAP only; gtr_32x1m: MAP only), then the
                                                 kernel times by `rocprofv3 --kernel-trace --stats` in a run of its own
  python tools/marginal_rate.py --phase kernels  (the workload that run profiles)
The plain form (HYPHY_HIP_REPEATS=0) throughout: its full pass is the yardstick."""
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


def setup(name):
    import bench
    from hyphy_amd import data, hip, models
    wl = bench.WORKLOADS[name]
    syn = data.evolve(wl["taxa"], wl["sites"], wl["unit"], seed=wl["seed"], p_change=wl.get("p_change", 0.04))
    D = 61 if wl["unit"] == 3 else 4
    pd = data.from_states(syn.states, D, compress_patterns=(D > 4))
    flat = syn.flat
    B = flat.n_branches
    if D == 61:
        Q = models.mg94rev_Q_batch(np.full(B, 0.05), 0.3, bench.REV, bench.POS_FREQS)
        pi = models.f3x4_codon_freqs(bench.POS_FREQS)
    else:
        Q = np.stack([models.nuc_rev_Q(0.05, models.hky85_rev(0.35), bench.NUC_FREQS)] * B)
        pi = bench.NUC_FREQS
    part = hip.HipPartition(D, flat.flat_parents, flat.L, pd.leaf_codes, None, pd.pattern_freq)
    nodes = np.arange(B, dtype=np.int64)
    return part, flat, Q, pi, nodes, D


def timed(fn, n):
    fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def pinned_ms(part, flat, pi, D, n_nodes=3):
    """ms per pinned evaluation, over ~n_nodes internal nodes x all states (partial updates along the node's path)."""
    L, I = flat.L, flat.I
    none = np.zeros(0, dtype=np.int64)
    q0 = np.zeros((0, D, D))
    ts = []
    for i in np.linspace(0, I - 2, n_nodes).round().astype(int):
        code = L + int(i)
        un = sorted(set(int(x) for x in flat.path_update_nodes(code)) | set(int(c) for c in flat.children_of(int(i))))
        un = np.array(un, dtype=np.int64)
        for x in range(D):
            part.set_pinned_states(code, np.full(part.S, x))
            t0 = time.perf_counter()
            part.evaluate(un, none, q0, pi, per_site=True)
            ts.append(time.perf_counter() - t0)
        part.set_pinned_states(None)
        part.evaluate(un, none, q0, pi)
    return float(np.mean(ts)) * 1e3, len(ts)


def phase_wall():
    out = {}
    for name, support in (("mg94_64x10k", True), ("gtr_32x1m", False)):
        part, flat, Q, pi, nodes, D = setup(name)
        with part:
            part.evaluate(nodes, nodes, Q, pi)
            full_ms = timed(lambda: part.evaluate(nodes, nodes[:0], Q[:0], pi), 10)   # (wall, pure re-evaluation: the yardstick pass)
            rec = dict(states=D, taxa=flat.L, internal_nodes=flat.I, patterns=part.S, full_pass_wall_ms=full_ms)
            rec["marginal_map_only_ms"] = timed(lambda: part.marginal_ancestral("internal", support=False, map=True), 5)
            if support:
                rec["marginal_full_support_ms"] = timed(lambda: part.marginal_ancestral("internal"), 3)
                rec["support_bytes_to_host"] = flat.I * part.S * D * 8
                per, n = pinned_ms(part, flat, pi, D)
                rec["pinned_ms_per_evaluation"] = per
                rec["pinned_evaluations_sampled"] = n
                rec["pinned_route_extrapolated_ms"] = per * flat.I * (D - 1)
                rec["speedup_full_support_vs_pinned"] = rec["pinned_route_extrapolated_ms"] / rec["marginal_full_support_ms"]
            out[name] = rec
    return out


def phase_kernels():
    os.environ["HYPHY_HIP_TUNE"] = "0"   # (no tuner trials among the profiled pruning launches: every one is a full pass)
    part, flat, Q, pi, nodes, D = setup("mg94_64x10k")
    with part:
        part.evaluate(nodes, nodes, Q, pi)
        for _ in range(5):
            part.evaluate(nodes, nodes, Q, pi)   # full passes (expm + pruning)
        for _ in range(5):
            part.marginal_ancestral("internal", support=False, map=True)


def kernel_stats():
    tmp = tempfile.mkdtemp(prefix="margprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    marg = {k: v for k, v in stats.items() if "marg" in k}
    prune = {k: v for k, v in stats.items() if "prune" in k or "walk" in k}
    marg_ms = sum(v["total_ns"] for v in marg.values()) / 5 / 1e6         # per call (5 calls)
    prune_ms = sum(v["total_ns"] for v in prune.values()) / 6 / 1e6       # per full pass (6 passes)
    return dict(workload="mg94_64x10k", marginal_kernels_ms_per_call=marg_ms, full_pass_pruning_ms=prune_ms,
                ratio=marg_ms / prune_ms if prune_ms else None,
                kernels={k: v for k, v in stats.items() if k in marg or k in prune})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal_rate.json"))
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
