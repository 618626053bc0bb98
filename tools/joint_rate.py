#!/usr/bin/env python3
"""Joint ancestral reconstruction (hyphy_hip_joint_ancestral) at bench.py's mg94_64x10k: one call with and without the leaves (median
of 20 after a 1.5 s warm-up) against one full pruning pass of the same partition, and its kernels' durations from one
`rocprofv3 --kernel-trace --stats` run of their own.  Writes profiles/joint_rate.json.

  python tools/joint_rate.py                  wall times, then the kernel times
  python tools/joint_rate.py --phase kernels  (the workload that run profiles)
The reference's own loop is the wall-clock difference of two runs of the reference binary (oracle/_ref/hyphy, when it is built) on the
same alignment and model, one with and one without the `ReconstructAncestors (lf)` line: "reference_loop" in the JSON.
  python tools/joint_rate.py --phase reference  (that difference alone; needs no device)"""
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


def timed(fn, n, warm_s):
    t_end = time.perf_counter() + warm_s
    while time.perf_counter() < t_end:
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def phase_wall():
    part, flat, Q, pi, nodes, D = setup("mg94_64x10k")
    with part:
        part.evaluate(nodes, nodes, Q, pi)
        rec = dict(states=D, taxa=flat.L, internal_nodes=flat.I, patterns=part.S)
        rec["full_pass_wall_ms"] = timed(lambda: part.evaluate(nodes, nodes[:0], Q[:0], pi), 20, 1.5)
        rec["joint_internal_ms"] = timed(lambda: part.joint_ancestral(False), 20, 1.5)
        rec["joint_with_leaves_ms"] = timed(lambda: part.joint_ancestral(True), 20, 1.5)
        rec["joint_over_full_pass"] = rec["joint_internal_ms"] / rec["full_pass_wall_ms"]
        # D^2 (I - 1) S multiply + compare + two selects
        rec["valu_floor_ops_each"] = float(D) ** 2 * (flat.I - 1) * part.S
    return rec


def reference_loop():
    """Seconds the reference spends in `ReconstructAncestors (lf)`: two runs of its binary, with and without the line."""
    import bench
    from hyphy_amd import data, models, tree
    from oracle import hbl
    if not hbl.have_reference():
        return dict(measured=False, why="oracle/_ref/hyphy is not built")
    wl = bench.WORKLOADS["mg94_64x10k"]
    syn = data.evolve(wl["taxa"], wl["sites"], wl["unit"], seed=wl["seed"], p_change=wl.get("p_change", 0.04))
    block = hbl.codon_model_block(models.mg94rev_template(bench.POS_FREQS), models.f3x4_codon_freqs(bench.POS_FREQS), rate_expr="t")
    tmp = tempfile.mkdtemp(prefix="jointref_")
    fasta = os.path.join(tmp, "aln.fasta")
    hbl.write_fasta(fasta, syn.flat.leaf_names, syn.seqs)
    txt = hbl.build_script(fasta=fasta, newick=tree.to_newick(syn.tree), unit=3, model_block=block, model_name="MGM",
                           globals_=dict(R=0.3, **bench.REV), branch_t={n: 0.05 for n in syn.flat.branch_names()},
                           out_path=os.path.join(tmp, "out.txt"), per_site=False)
    mark = "LFCompute (lf, LF_DONE_COMPUTE);\n"
    assert txt.count(mark) == 1
    line = "DataSet anc = ReconstructAncestors (lf);\n"
    secs = {}
    for name, script in (("without", txt), ("with", txt.replace(mark, line + mark))):
        t0 = time.perf_counter()
        hbl.run_script(script, tmp)
        secs[name] = time.perf_counter() - t0
    return dict(measured=True, run_without_s=secs["without"], run_with_s=secs["with"], reconstruct_s=secs["with"] - secs["without"])


def phase_kernels():
    os.environ["HYPHY_HIP_TUNE"] = "0"
    part, flat, Q, pi, nodes, D = setup("mg94_64x10k")
    with part:
        for _ in range(6):
            part.evaluate(nodes, nodes, Q, pi)
        for _ in range(5):
            part.joint_ancestral(False)


def kernel_stats():
    import csv
    import glob
    tmp = tempfile.mkdtemp(prefix="jointprof_")
    cmd = ["timeout", "-k", "10", "500", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    joint = {k: v for k, v in stats.items() if "joint" in k}
    prune = {k: v for k, v in stats.items() if "prune" in k or "walk" in k}
    joint_ms = sum(v["total_ns"] for v in joint.values()) / 5 / 1e6
    prune_ms = sum(v["total_ns"] for v in prune.values()) / 6 / 1e6
    return dict(joint_kernels_ms_per_call=joint_ms, full_pass_pruning_ms=prune_ms, ratio=joint_ms / prune_ms if prune_ms else None,
                kernels={**joint, **prune})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels", "reference"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_rate.json"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    if a.phase == "reference":
        print(json.dumps(reference_loop(), indent=1))
        return
    res = dict(workload="mg94_64x10k", wall=phase_wall(), reference_loop=reference_loop())
    if res["reference_loop"]["measured"]:
        res["reference_over_joint"] = res["reference_loop"]["reconstruct_s"] * 1e3 / res["wall"]["joint_internal_ms"]
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats()
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
