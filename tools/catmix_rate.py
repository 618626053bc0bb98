#!/usr/bin/env python3
"""Rate classes over branch-site mixtures at bench.py's busted3_64x10k tree and alignment (64 taxa, ~10 k codon sites, 61 states):
C = 3 synonymous-rate classes x 3 omega components on every branch, components built on the device from two templates (one
coefficient row per (class, branch, component): 1 125 rows).  Median wall time of 20 calls after 5 warm-up calls, same process,
time.perf_counter around the call, HYPHY_HIP_TUNE=0, HYPHY_HIP_REPEATS=0:

  (i)   evaluate_categories_mixture_built   build_q of C x n_tot rows + the one batched call (closure, ctypes arguments marshalled once)
  (ii)  what a host does today              C x (build_q + evaluate_mixture_built with per-pattern outputs) + the host's class mix
                                            (closure, arguments marshalled once; the mix in numpy)
  (iii) evaluate_categories_mixture         the dense entry point: 1 125 host matrices over PCIe (closure)

and the kernels' durations from one `rocprofv3 --kernel-trace --stats` run of its own: 5 batched calls, then 5 one-class
evaluate_mixture_built calls on class 0 (mix_images_kernel on one class's 375 components: what retiring that kernel will be judged
against).  Writes profiles/catmix_rate.json and profiles/catmix_kernel_stats.csv.

  python tools/catmix_rate.py                  wall times, then the kernel times
  python tools/catmix_rate.py --phase kernels  (the workload that run profiles)"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["HYPHY_HIP_REPEATS"] = "0"
os.environ["HYPHY_HIP_TUNE"] = "0"

T_BRANCH = 0.05
CLASS_RATE = np.array([0.4, 1.0, 2.5])          # synonymous-rate classes
CLASS_W = np.array([0.3, 0.5, 0.2])
OMEGA = np.array([0.1, 0.6, 3.0])               # the branch-site mixture of every branch
OMEGA_W = np.array([0.6, 0.3, 0.1])
CALLS, WARM, PROFILED = 20, 5, 5
LOG_SCALER = 64.0 * np.log(2.0)


def setup():
    import bench
    from hyphy_amd import data, hip
    wl = bench.WORKLOADS["busted3_64x10k"]
    syn = data.evolve(wl["taxa"], wl["sites"], wl["unit"], seed=wl["seed"], p_change=wl.get("p_change", 0.04))
    pd = data.from_states(syn.states, 61, compress_patterns=True)
    flat = syn.flat
    B, Cn, M = flat.n_branches, 3, 3
    T, pi = bench.templates_for(3)
    part = hip.HipPartition(61, flat.flat_parents, flat.L, pd.leaf_codes, None, pd.pattern_freq, Cn)
    part.set_q_templates(T)
    nodes = np.arange(B, dtype=np.int64)
    co = np.empty((Cn, B, M, 2))                 # row (c, b, m): (rate_c t_b, omega_m rate_c t_b)
    co[..., 0] = (CLASS_RATE * T_BRANCH)[:, None, None]
    co[..., 1] = co[..., 0] * OMEGA[None, None, :]
    mw = np.ascontiguousarray(np.broadcast_to(OMEGA_W, (Cn, B, M)))
    return part, T, pi, nodes, np.ascontiguousarray(co), mw, np.asarray(pd.pattern_freq, dtype=np.float64)


def times(fn, n=CALLS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return dict(median_us=float(np.median(ts)), min_us=float(np.min(ts)), max_us=float(np.max(ts)), calls=n, warm_up_calls=warm)


def closures(part, T, pi, nodes, co, mw, freq):
    from hyphy_amd import hip
    Cn, B, M, _ = co.shape
    lib, h = part._lib, part._h
    rf = np.ascontiguousarray(pi, dtype=np.float64)
    cw = np.ascontiguousarray(CLASS_W)
    cnt = np.full(B, M, dtype=np.int64)
    rows = co.reshape(Cn * B * M, 2)
    w_all = mw.reshape(-1)
    out = C.c_double(0.0)
    pout = C.byref(out)
    pn, prf, pcw, pcnt = hip._l(nodes), hip._d(rf), hip._d(cw), hip._l(cnt)
    keep = [rf, cw, cnt, rows, w_all]

    def batched(_keep=keep):
        rc = lib.hyphy_hip_build_q(h, rows.shape[0], hip._d(rows))
        if rc == 0:
            rc = lib.hyphy_hip_evaluate_categories_mixture_built(h, pn, B, pn, B, pcnt, hip._d(w_all), pcw, prf, pout, None, None)
        if rc:
            hip._check(rc)
        return out.value

    lik = np.zeros((Cn, part.S))
    cn = np.zeros((Cn, part.S), dtype=np.int64)
    per_rows = [np.ascontiguousarray(co[c].reshape(B * M, 2)) for c in range(Cn)]
    per_w = [np.ascontiguousarray(mw[c].reshape(-1)) for c in range(Cn)]

    def host_route(_keep=(per_rows, per_w, lik, cn)):
        for c in range(Cn):
            rc = lib.hyphy_hip_build_q(h, B * M, hip._d(per_rows[c]))
            if rc == 0:
                rc = lib.hyphy_hip_evaluate_mixture_built(h, c, pn, B, pn, B, pcnt, hip._d(per_w[c]), prf, pout, hip._d(lik[c]), hip._l(cn[c]))
            if rc:
                hip._check(rc)
        low = cn.min(axis=0)
        mixed = (cw[:, None] * lik * np.exp2(-64.0 * (cn - low))).sum(axis=0)
        return float(np.sum(freq * (np.log(mixed) - low * LOG_SCALER)))

    # dense: Q = x0 T0 + x1 T1 off the diagonal, the diagonal set on the host
    Q = np.tensordot(rows, T, axes=1)
    idx = np.arange(61)
    Q[:, idx, idx] = 0.0
    Q[:, idx, idx] = -Q.sum(axis=2)
    Q = np.ascontiguousarray(Q)

    def dense(_keep=(Q,)):
        rc = lib.hyphy_hip_evaluate_categories_mixture(h, pn, B, pn, B, pcnt, hip._d(Q), hip._d(w_all), pcw, prf, pout, None, None)
        if rc:
            hip._check(rc)
        return out.value

    def one_class(_keep=(per_rows, per_w)):
        rc = lib.hyphy_hip_build_q(h, B * M, hip._d(per_rows[0]))
        if rc == 0:
            rc = lib.hyphy_hip_evaluate_mixture_built(h, 0, pn, B, pn, B, pcnt, hip._d(per_w[0]), prf, pout, None, None)
        if rc:
            hip._check(rc)
        return out.value

    return batched, host_route, dense, one_class


def make():
    part, T, pi, nodes, co, mw, freq = setup()
    return part, closures(part, T, pi, nodes, co, mw, freq), co.shape


def phase_wall():
    from hyphy_amd import hip
    part, (batched, host_route, dense, _), shape = make()
    Cn, B, M, _k = shape
    rec = dict(states=61, taxa=int(part.L), patterns=int(part.S), branches=int(B), classes=int(Cn), components_per_branch=int(M),
               rows=int(Cn * B * M))
    with part:
        a = batched()
        rec["expm_kernel_batched"], rec["reduce_form"] = hip.last_expm_kernel(), part.reduce_form()
        b = host_route()
        rec["expm_kernel_one_class"] = hip.last_expm_kernel()
        c = dense()
        rec["logl_batched_built"], rec["logl_host_route"], rec["logl_batched_dense"] = a, b, c
        rec["i_evaluate_categories_mixture_built"] = times(batched)
        rec["ii_host_route"] = times(host_route)
        rec["iii_evaluate_categories_mixture_dense"] = times(dense)
        rec["i_again"] = times(batched)          # (i) once more behind the others: same process, same clocks
        rec["host_route_over_batched"] = rec["ii_host_route"]["median_us"] / rec["i_evaluate_categories_mixture_built"]["median_us"]
        rec["batched_is_faster"] = bool(rec["i_evaluate_categories_mixture_built"]["median_us"] < rec["ii_host_route"]["median_us"])
    return rec


def phase_kernels():
    part, (batched, _, _, one_class), _ = make()
    with part:
        for _ in range(PROFILED):
            batched()
        for _ in range(PROFILED):
            one_class()


def kernel_stats(csv_out):
    tmp = tempfile.mkdtemp(prefix="catmixprof_")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    shutil.copyfile(files[0], csv_out)
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    res = dict(batched_calls_profiled=PROFILED, one_class_calls_profiled=PROFILED, kernels=stats)
    # the statistics merge the launches of both halves under one kernel name: the trace of the same run tells them apart, the
    # first PROFILED dispatches of a kernel both halves launch being the batched calls'
    trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    trows = list(csv.DictReader(open(trace[0]))) if trace else []
    if trows and all(k in trows[0] for k in ("Kernel_Name", "Start_Timestamp", "End_Timestamp")):
        by = {}
        for r in sorted(trows, key=lambda r: int(r["Start_Timestamp"])):
            by.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        split = {}
        for name, d in by.items():
            m = re.search(r"\w+_kernel(<\d+>)?", name)   # ("void hyhip::(anonymous namespace)::expm64_kernel<1>(...)")
            short = m.group(0) if m else name
            if len(d) == 2 * PROFILED:
                split[short] = dict(batched_us=float(np.median(d[:PROFILED])), one_class_us=float(np.median(d[PROFILED:])))
            elif len(d) == PROFILED:
                split[short] = dict(us=float(np.median(d)))
        res["per_dispatch_median_us"] = split
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catmix_rate.json"))
    ap.add_argument("--csv", default=os.path.join(ROOT, "profiles", "catmix_kernel_stats.csv"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    res = dict(workload="busted3_64x10k tree and alignment, C = 3 rate classes x 3 mixture components per branch, template mode",
               method="wall: time.perf_counter around the call, same process, median of 20 calls after 5 warm-up calls, HYPHY_HIP_TUNE=0, "
                      "HYPHY_HIP_REPEATS=0, every route a closure with its ctypes arguments marshalled once; kernels: one rocprofv3 "
                      "--kernel-trace --stats run of 5 batched calls and 5 one-class calls in a process of its own",
               wall=phase_wall())
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats(a.csv)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
