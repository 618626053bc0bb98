#!/usr/bin/env python3
"""Hidden-Markov rate classes at bench.py's busted3_64x10k (64 taxa, ~10 k codon sites, 61 states, C = 3), for two site lists — one
site per pattern, and the alignment's own list (10 000 sites over its patterns, with repeats).  Median wall time of 20 calls after
5 warm-up calls, same process, time.perf_counter around the call.  (i) and (ii) are timed as closures whose ctypes arguments are
marshalled ONCE (HipPartition.prepare_built_categories_step and its twin here), so their difference is the library's; (i) is also
timed through the Python method, as (iii) and (iv) are, whose numpy / ctypes marshalling is part of every call:

  (i)   evaluate_categories_built_hmm      build_q + the class batch + the scan: one wait
  (ii)  evaluate_categories_built          build_q + the class batch + the i.i.d. mix, for scale
  (iii) what a host does today             C x (build_q + evaluate_built with per-pattern outputs) + hip.hmm_host
  (iv)  hmm_logl alone                     a new transition matrix over resident values

and the kernels' durations from one `rocprofv3 --kernel-trace --stats` run of its own.  Writes profiles/hmm_rate.json.

  python tools/hmm_rate.py                  wall times, then the kernel times
  python tools/hmm_rate.py --phase kernels  (the workload that run profiles)"""
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
os.environ["HYPHY_HIP_REPEATS"] = "0"
os.environ["HYPHY_HIP_TUNE"] = "0"

T_BRANCH, OMEGA, LAMBDA = 0.05, 0.3, 0.15
CLASS_OMEGA = np.array([0.1, 1.0, 5.0]) / 0.3
CLASS_W = np.array([0.7, 0.25, 0.05])
CALLS, WARM, PROFILED = 20, 5, 5


def setup():
    import bench
    from hyphy_amd import data, hip
    wl = bench.WORKLOADS["busted3_64x10k"]
    syn = data.evolve(wl["taxa"], wl["sites"], wl["unit"], seed=wl["seed"], p_change=wl.get("p_change", 0.04))
    pd = data.from_states(syn.states, 61, compress_patterns=True)
    flat = syn.flat
    B, C = flat.n_branches, 3
    T, pi = bench.templates_for(3)
    part = hip.HipPartition(61, flat.flat_parents, flat.L, pd.leaf_codes, None, pd.pattern_freq, C)
    part.set_q_templates(T)
    nodes = np.arange(B, dtype=np.int64)
    co = np.empty((B * C, 2))
    co[:, 0] = T_BRANCH
    co[:, 1] = np.repeat(CLASS_OMEGA * OMEGA, B) * co[:, 0]
    Th = LAMBDA * np.tile(CLASS_W, (C, 1))
    np.fill_diagonal(Th, 0.0)
    np.fill_diagonal(Th, 1.0 - Th.sum(axis=1))
    return part, pd, flat, pi, nodes, co, Th, CLASS_W.copy()


def times(fn, n=CALLS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return dict(median_us=float(np.median(ts)), min_us=float(np.min(ts)), max_us=float(np.max(ts)), calls=n, warm_up_calls=warm)


def prepare_built_hmm_step(part, nodes, Th, pih, pi, co):
    """build_q + hyphy_hip_evaluate_categories_built_hmm with the arguments marshalled once: the twin of prepare_built_categories_step."""
    import ctypes as C
    from hyphy_amd import hip
    keep = [np.ascontiguousarray(x, dtype=t) for x, t in ((nodes, np.int64), (Th, np.float64), (pih, np.float64), (pi, np.float64),
                                                          (co, np.float64))]
    un, t, f, rf, cf = keep
    lib, h = part._lib, part._h
    pun, pt, pf, prf, pco = hip._l(un), hip._d(t), hip._d(f), hip._d(rf), hip._d(cf)
    out = C.c_double(0.0)
    pout = C.byref(out)

    def step(_keep=keep):
        rc = lib.hyphy_hip_build_q(h, cf.shape[0], pco)
        if rc == 0:
            rc = lib.hyphy_hip_evaluate_categories_built_hmm(h, pun, len(un), pun, len(un), pt, pf, prf, pout)
        if rc:
            hip._check(rc)
        return out.value
    return step


def host_route(part, pd, nodes, pi, co, Th, pih, sites):
    from hyphy_amd import hip
    B, C = len(nodes), 3
    l, c = np.empty((C, part.S)), np.empty((C, part.S), dtype=np.int64)

    def run():
        for m in range(C):
            part.build_q(co[m * B:(m + 1) * B])
            _, l[m], c[m] = part.evaluate_built(nodes, nodes, pi, cat=m, per_site=True)
        return hip.hmm_host(l, c, Th, pih, sites)
    return run, l, c


def phase_wall():
    from hyphy_amd import hip
    part, pd, flat, pi, nodes, co, Th, pih = setup()
    rec = dict(states=61, taxa=flat.L, patterns=part.S, classes=3, G=hip.plan_hmm(2, 3)["G"])
    with part:
        for tag, sites in (("one_site_per_pattern", None), ("alignment_sites", pd.site_to_pattern)):
            part.hmm_set_sites(sites)
            n = part.S if sites is None else len(sites)
            r = dict(sites=int(n), plan=hip.plan_hmm(n, 3))
            fused = part.evaluate_categories_built_hmm(nodes, nodes, Th, pih, pi, co)
            r["form"] = part.reduce_form()
            host, l, c = host_route(part, pd, nodes, pi, co, Th, pih, sites)
            by_host = host()
            r["logl_fused"], r["logl_host_route"], r["abs_difference"] = fused, by_host, abs(fused - by_host)
            r["i_evaluate_categories_built_hmm"] = times(prepare_built_hmm_step(part, nodes, Th, pih, pi, co))
            r["i_through_the_python_method"] = times(lambda: part.evaluate_categories_built_hmm(nodes, nodes, Th, pih, pi, co))
            r["ii_evaluate_categories_built"] = times(part.prepare_built_categories_step(nodes, nodes, CLASS_W, pi, co))
            r["iii_host_route"] = times(host)
            r["iii_of_which_hmm_host"] = times(lambda: hip.hmm_host(l, c, Th, pih, sites))
            part.evaluate_categories_built_hmm(nodes, nodes, Th, pih, pi, co)
            T2 = Th.copy()
            T2[0, 1], T2[0, 0] = T2[0, 1] * 1.01, T2[0, 0] - T2[0, 1] * 0.01
            flip, turn = [Th, T2], [0]

            def line_search_step():
                turn[0] ^= 1
                return part.hmm_logl(flip[turn[0]], pih)
            r["iv_hmm_logl"] = times(line_search_step)
            r["host_route_over_fused"] = r["iii_host_route"]["median_us"] / r["i_through_the_python_method"]["median_us"]
            r["fused_minus_iid_mix_us"] = r["i_evaluate_categories_built_hmm"]["median_us"] - r["ii_evaluate_categories_built"]["median_us"]
            rec[tag] = r
    return rec


def phase_kernels():
    part, pd, flat, pi, nodes, co, Th, pih = setup()
    with part:
        part.hmm_set_sites(pd.site_to_pattern)
        for _ in range(PROFILED):
            part.evaluate_categories_built_hmm(nodes, nodes, Th, pih, pi, co)
        part.hmm_viterbi(Th, pih)


def kernel_stats():
    import csv
    import glob
    tmp = tempfile.mkdtemp(prefix="hmmprof_")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--phase", "kernels"]
    subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
    rows = list(csv.DictReader(open(files[0])))
    stats = {r["Name"]: dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]), avg_ns=float(r["AverageNs"])) for r in rows}
    mine = {k: v for k, v in stats.items() if "hmm_" in k or "vit_" in k}
    fwd = sum(v["total_ns"] for k, v in mine.items() if "hmm_" in k)
    return dict(site_list="alignment_sites", fused_calls_profiled=PROFILED, viterbi_calls_profiled=1,
                forward_kernels_us_per_call=fwd / PROFILED / 1e3, hmm_kernels=mine,
                other_kernels={k: v for k, v in stats.items() if k not in mine})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=["all", "wall", "kernels"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm_rate.json"))
    a = ap.parse_args()
    if a.phase == "kernels":
        phase_kernels()
        return
    res = dict(workload="busted3_64x10k",
               method="wall: time.perf_counter around the call, same process, median of 20 calls after 5 warm-up calls, HYPHY_HIP_TUNE=0, "
                      "HYPHY_HIP_REPEATS=0; i_evaluate_categories_built_hmm and ii_evaluate_categories_built are closures with ctypes "
                      "arguments marshalled once (fused_minus_iid_mix_us is their difference), every other entry is a Python method "
                      "call with its numpy / ctypes marshalling (host_route_over_fused compares two of those); kernels: one rocprofv3 --kernel-trace --stats run "
                      "of 5 fused calls and one Viterbi call in a process of its own",
               wall=phase_wall())
    if a.phase == "all":
        res["rocprofv3"] = kernel_stats()
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
