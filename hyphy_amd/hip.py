"""ctypes binding of the C-ABI in ``include/hyphy_hip.h`` (``hyphy_amd/lib/libhyphy_hip.so``).

This is the only way Python reaches the device code: there is no PyTorch/numpy/CPU fallback —
if the shared library is missing or no MI355X is visible, construction raises.  The class
mirrors the reference-side lifetime: ``HipPartition(...)`` ≙ the hook in
``_LikelihoodFunction::SetupLFCaches`` (``likefunc.cpp:4313-4316``), ``evaluate`` ≙ the call
from ``ComputeBlock`` (``likefunc.cpp:10978-11123``), ``close`` ≙ ``DeleteCaches``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HYPHY_HIP_LIB") or os.path.join(HERE, "lib", "libhyphy_hip.so")  # (override: A/B builds)

EXPORTS = [
    "hyphy_hip_device_count", "hyphy_hip_create", "hyphy_hip_destroy", "hyphy_hip_evaluate",
    "hyphy_hip_evaluate_device", "hyphy_hip_fetch_device_scalar", "hyphy_hip_plan_reroot", "hyphy_hip_plan_pattern_order", "hyphy_hip_plan_schedule", "hyphy_hip_evaluate_async", "hyphy_hip_collect", "hyphy_hip_evaluate_mixture", "hyphy_hip_evaluate_mixture_built", "hyphy_hip_comm_unique_id", "hyphy_hip_comm_init_rank", "hyphy_hip_comm_init_all", "hyphy_hip_allreduce_device", "hyphy_hip_evaluate_allreduce", "hyphy_hip_evaluate_built_allreduce", "hyphy_hip_last_allreduce_ms", "hyphy_hip_evaluate_categories", "hyphy_hip_download_partials",
    "hyphy_hip_expm_batch", "hyphy_hip_set_q_templates", "hyphy_hip_build_q", "hyphy_hip_q_buffer",
    "hyphy_hip_evaluate_built", "hyphy_hip_evaluate_built_sites", "hyphy_hip_update_q_templates", "hyphy_hip_evaluate_categories_built", "hyphy_hip_evaluate_categories_built_sites", "hyphy_hip_prune_timings", "hyphy_hip_prune_launches",
    "hyphy_hip_prune_kernel_name", "hyphy_hip_last_prune_form", "hyphy_hip_last_reduce_form", "hyphy_hip_branch_cache_build", "hyphy_hip_branch_cache_evaluate",
    "hyphy_hip_set_pinned_states", "hyphy_hip_marginal_ancestral", "hyphy_hip_plan_marginal", "hyphy_hip_joint_ancestral", "hyphy_hip_sample_ancestral", "hyphy_hip_sample_uniforms", "hyphy_hip_simulate", "hyphy_hip_simulate_uniforms", "hyphy_hip_branch_trials", "hyphy_hip_branch_trials_built", "hyphy_hip_branch_derivatives", "hyphy_hip_branch_derivatives_built", "hyphy_hip_branch_sensitivities", "hyphy_hip_branch_gradient", "hyphy_hip_branch_gradient_built", "hyphy_hip_expm_frechet_adjoint_batch", "hyphy_hip_site_fits_evaluate", "hyphy_hip_site_fits_evaluate_mixture", "hyphy_hip_site_fits_kernel_ms",
    "hyphy_hip_synchronize", "hyphy_hip_stream", "hyphy_hip_set_stream", "hyphy_hip_last_timings", "hyphy_hip_set_timing_detail", "hyphy_hip_schedule_info", "hyphy_hip_set_repeats", "hyphy_hip_repeat_stats", "hyphy_hip_plan_repeats", "hyphy_hip_plan_repeat_layout", "hyphy_hip_plan_trunk_walk", "hyphy_hip_plan_nucgen", "hyphy_hip_plan_switches", "hyphy_hip_comm_init_host", "hyphy_hip_evaluate_exchange", "hyphy_hip_evaluate_built_exchange",
    "hyphy_hip_xch_open", "hyphy_hip_xch_sum", "hyphy_hip_xch_close", "hyphy_hip_last_error", "hyphy_hip_last_expm_kernel",
    "hyphy_hip_evaluate_categories_mixture", "hyphy_hip_evaluate_categories_mixture_built",
    "hyphy_hip_hmm_set_sites", "hyphy_hip_hmm_logl", "hyphy_hip_hmm_viterbi", "hyphy_hip_evaluate_categories_hmm", "hyphy_hip_evaluate_categories_built_hmm", "hyphy_hip_plan_hmm", "hyphy_hip_hmm_host",
    "hyphy_hip_nni_scores", "hyphy_hip_plan_nni", "hyphy_hip_check_nni",
    "hyphy_hip_version",
]

_lib = None


class HipError(RuntimeError):
    pass


class HipUnsupported(HipError):
    """The library answered "> 0": use the CPU path of the host application."""


def load():
    """Load libhyphy_hip.so; raise loudly if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipError(f"{LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    dp, lp, vp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p
    lib.hyphy_hip_device_count.restype = C.c_int
    lib.hyphy_hip_create.restype = C.c_int
    lib.hyphy_hip_create.argtypes = [C.POINTER(vp)] + [C.c_int64] * 5 + [lp, lp, dp, C.c_int64, lp, C.c_int, C.c_int]
    lib.hyphy_hip_destroy.restype = None
    lib.hyphy_hip_destroy.argtypes = [vp]
    lib.hyphy_hip_evaluate.restype = C.c_int
    lib.hyphy_hip_evaluate.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, C.c_int, dp, dp, dp, lp]
    lib.hyphy_hip_comm_unique_id.restype = C.c_int
    lib.hyphy_hip_comm_unique_id.argtypes = [vp]
    lib.hyphy_hip_comm_init_rank.restype = C.c_int
    lib.hyphy_hip_comm_init_rank.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.hyphy_hip_comm_init_all.restype = C.c_int
    lib.hyphy_hip_comm_init_all.argtypes = [vp]
    lib.hyphy_hip_allreduce_device.restype = C.c_int
    lib.hyphy_hip_allreduce_device.argtypes = [vp, vp]
    lib.hyphy_hip_evaluate_allreduce.restype = C.c_int
    lib.hyphy_hip_evaluate_allreduce.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, C.c_int, dp, dp]
    lib.hyphy_hip_evaluate_mixture.restype = C.c_int
    lib.hyphy_hip_evaluate_mixture.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, lp, dp, dp, dp, dp, dp, lp]
    lib.hyphy_hip_evaluate_mixture_built.restype = C.c_int
    lib.hyphy_hip_evaluate_mixture_built.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, lp, dp, dp, dp, dp, lp]
    lib.hyphy_hip_evaluate_categories_mixture.restype = C.c_int
    lib.hyphy_hip_evaluate_categories_mixture.argtypes = [vp, lp, C.c_int64, lp, C.c_int64, lp, dp, dp, dp, dp, dp, dp, lp]
    lib.hyphy_hip_evaluate_categories_mixture_built.restype = C.c_int
    lib.hyphy_hip_evaluate_categories_mixture_built.argtypes = [vp, lp, C.c_int64, lp, C.c_int64, lp, dp, dp, dp, dp, dp, lp]
    lib.hyphy_hip_evaluate_async.restype = C.c_int
    lib.hyphy_hip_evaluate_async.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, C.c_int, dp]
    lib.hyphy_hip_collect.restype = C.c_int
    lib.hyphy_hip_collect.argtypes = [vp, dp, dp, lp]
    lib.hyphy_hip_plan_reroot.restype = C.c_int64
    lib.hyphy_hip_plan_reroot.argtypes = [C.c_int64, C.c_int64, lp, C.c_int64, lp, C.c_int64]
    lib.hyphy_hip_plan_pattern_order.restype = C.c_int
    lib.hyphy_hip_plan_pattern_order.argtypes = [C.c_int64, C.c_int64, C.c_int64, lp, lp]
    lib.hyphy_hip_plan_schedule.restype = C.c_int
    lib.hyphy_hip_plan_schedule.argtypes = [C.c_int64, C.c_int64, lp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, lp]
    lib.hyphy_hip_fetch_device_scalar.restype = C.c_int
    lib.hyphy_hip_fetch_device_scalar.argtypes = [vp, vp, C.POINTER(C.c_double)]
    lib.hyphy_hip_evaluate_device.restype = C.c_int
    lib.hyphy_hip_evaluate_device.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, vp, C.c_int, dp, vp]
    lib.hyphy_hip_evaluate_categories.restype = C.c_int
    lib.hyphy_hip_evaluate_categories.argtypes = [vp, lp, C.c_int64, lp, C.c_int64, dp, C.c_int, dp, dp, dp, dp, lp]
    lib.hyphy_hip_download_partials.restype = C.c_int
    lib.hyphy_hip_download_partials.argtypes = [vp, C.c_int64, dp, lp]
    lib.hyphy_hip_expm_batch.restype = C.c_int
    lib.hyphy_hip_expm_batch.argtypes = [C.c_int64, C.c_int64, dp, dp]
    lib.hyphy_hip_set_q_templates.restype = C.c_int
    lib.hyphy_hip_set_q_templates.argtypes = [vp, C.c_int64, dp]
    lib.hyphy_hip_update_q_templates.restype = C.c_int
    lib.hyphy_hip_update_q_templates.argtypes = [vp, C.c_int64, dp]
    lib.hyphy_hip_build_q.restype = C.c_int
    lib.hyphy_hip_build_q.argtypes = [vp, C.c_int64, dp]
    lib.hyphy_hip_evaluate_built.restype = C.c_int
    lib.hyphy_hip_evaluate_built.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, dp]
    lib.hyphy_hip_evaluate_built_sites.restype = C.c_int
    lib.hyphy_hip_evaluate_built_sites.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, dp, dp, lp]
    lib.hyphy_hip_evaluate_categories_built.restype = C.c_int
    lib.hyphy_hip_evaluate_categories_built.argtypes = [vp, lp, C.c_int64, lp, C.c_int64, dp, dp, dp]
    lib.hyphy_hip_evaluate_categories_built_sites.restype = C.c_int
    lib.hyphy_hip_evaluate_categories_built_sites.argtypes = [vp, lp, C.c_int64, lp, C.c_int64, dp, dp, dp, dp, lp]
    lib.hyphy_hip_site_fits_evaluate.restype = C.c_int
    lib.hyphy_hip_site_fits_evaluate.argtypes = [vp, C.c_int64, C.c_int64, lp, dp, dp, dp, dp]
    lib.hyphy_hip_site_fits_evaluate_mixture.restype = C.c_int
    lib.hyphy_hip_site_fits_evaluate_mixture.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, lp, dp, dp, dp, dp, dp]
    lib.hyphy_hip_site_fits_kernel_ms.restype = C.c_double
    lib.hyphy_hip_site_fits_kernel_ms.argtypes = [vp]
    lib.hyphy_hip_q_buffer.restype = vp
    lib.hyphy_hip_q_buffer.argtypes = [vp]
    lib.hyphy_hip_synchronize.restype = C.c_int
    lib.hyphy_hip_synchronize.argtypes = [vp]
    lib.hyphy_hip_stream.restype = vp
    lib.hyphy_hip_stream.argtypes = [vp]
    lib.hyphy_hip_set_stream.restype = C.c_int
    lib.hyphy_hip_set_stream.argtypes = [vp, vp]
    lib.hyphy_hip_evaluate_built_allreduce.restype = C.c_int
    lib.hyphy_hip_evaluate_built_allreduce.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, dp]
    lib.hyphy_hip_last_allreduce_ms.restype = C.c_double
    lib.hyphy_hip_last_allreduce_ms.argtypes = [vp]
    lib.hyphy_hip_last_timings.restype = C.c_int
    lib.hyphy_hip_last_timings.argtypes = [vp, dp]
    lib.hyphy_hip_schedule_info.restype = C.c_char_p
    lib.hyphy_hip_schedule_info.argtypes = [vp]
    lib.hyphy_hip_set_timing_detail.restype = C.c_int
    lib.hyphy_hip_set_timing_detail.argtypes = [vp, C.c_int]
    lib.hyphy_hip_prune_timings.restype = C.c_int64
    lib.hyphy_hip_prune_timings.argtypes = [vp, dp, C.c_int64]
    lib.hyphy_hip_prune_launches.restype = C.c_int
    lib.hyphy_hip_prune_launches.argtypes = [vp]
    lib.hyphy_hip_set_pinned_states.restype = C.c_int
    lib.hyphy_hip_set_pinned_states.argtypes = [vp, C.c_int64, lp]
    lib.hyphy_hip_branch_cache_build.restype = C.c_int
    lib.hyphy_hip_branch_cache_build.argtypes = [vp, C.c_int64, C.c_int64]
    lib.hyphy_hip_branch_cache_evaluate.restype = C.c_int
    lib.hyphy_hip_branch_cache_evaluate.argtypes = [vp, C.c_int64, C.c_int64, dp, C.c_int, dp, dp, lp]
    lib.hyphy_hip_prune_kernel_name.restype = C.c_char_p
    lib.hyphy_hip_prune_kernel_name.argtypes = [vp]
    lib.hyphy_hip_last_prune_form.restype = C.c_char_p
    lib.hyphy_hip_last_prune_form.argtypes = [vp]
    lib.hyphy_hip_last_reduce_form.restype = C.c_char_p
    lib.hyphy_hip_last_reduce_form.argtypes = [vp]
    lib.hyphy_hip_set_repeats.restype = C.c_int
    lib.hyphy_hip_set_repeats.argtypes = [vp, C.c_int]
    lib.hyphy_hip_marginal_ancestral.restype = C.c_int
    lib.hyphy_hip_marginal_ancestral.argtypes = [vp, C.c_int64, dp, dp, lp, dp]
    lib.hyphy_hip_joint_ancestral.restype = C.c_int
    lib.hyphy_hip_joint_ancestral.argtypes = [vp, C.c_int, lp, lp]
    lib.hyphy_hip_sample_ancestral.restype = C.c_int
    lib.hyphy_hip_sample_ancestral.argtypes = [vp, C.c_int64, C.c_int64, lp, lp, C.c_uint64, dp, C.POINTER(C.c_int8)]
    lib.hyphy_hip_sample_uniforms.restype = C.c_int
    lib.hyphy_hip_sample_uniforms.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, dp]
    lib.hyphy_hip_simulate.restype = C.c_int
    lib.hyphy_hip_simulate.argtypes = [vp, C.c_int64, C.c_int64, lp, lp, C.c_uint64, dp, C.c_int, C.POINTER(C.c_int8)]
    lib.hyphy_hip_simulate_uniforms.restype = C.c_int
    lib.hyphy_hip_simulate_uniforms.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, dp]
    lib.hyphy_hip_branch_trials.restype = C.c_int
    lib.hyphy_hip_branch_trials.argtypes = [vp, C.c_int64, lp, dp, C.c_int, dp, dp, dp, lp]
    lib.hyphy_hip_branch_trials_built.restype = C.c_int
    lib.hyphy_hip_branch_trials_built.argtypes = [vp, C.c_int64, lp, dp, dp, dp, dp, lp]
    for fn in (lib.hyphy_hip_branch_derivatives, lib.hyphy_hip_branch_derivatives_built):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.c_int64, lp, dp, dp, dp, dp, lp, dp, dp]
    lib.hyphy_hip_branch_sensitivities.restype = C.c_int
    lib.hyphy_hip_branch_sensitivities.argtypes = [vp, C.c_int64, lp, dp, dp, lp]
    for fn in (lib.hyphy_hip_branch_gradient, lib.hyphy_hip_branch_gradient_built):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.c_int64, lp, dp, dp, dp, lp]
    lib.hyphy_hip_expm_frechet_adjoint_batch.restype = C.c_int
    lib.hyphy_hip_expm_frechet_adjoint_batch.argtypes = [C.c_int64, C.c_int64, dp, dp, dp]
    lib.hyphy_hip_nni_scores.restype = C.c_int
    lib.hyphy_hip_nni_scores.argtypes = [vp, C.c_int64, lp, dp, dp, dp, lp]
    lib.hyphy_hip_plan_nni.restype = C.c_int64
    lib.hyphy_hip_plan_nni.argtypes = [C.c_int64, C.c_int64, lp, lp, C.c_int64]
    lib.hyphy_hip_check_nni.restype = C.c_int
    lib.hyphy_hip_check_nni.argtypes = [C.c_int64, C.c_int64, lp, C.c_int64, lp]
    lib.hyphy_hip_plan_marginal.restype = C.c_int64
    lib.hyphy_hip_plan_marginal.argtypes = [C.c_int64, C.c_int64, lp, lp, C.c_int64]
    lib.hyphy_hip_plan_trunk_walk.restype = C.c_int64
    lib.hyphy_hip_plan_trunk_walk.argtypes = [C.c_int64, C.c_int64, lp, lp, C.c_int64]
    lib.hyphy_hip_plan_repeats.restype = C.c_int64
    lib.hyphy_hip_plan_repeats.argtypes = [C.c_int64, C.c_int64, lp, C.c_int64, lp, C.c_double, lp, lp]
    lib.hyphy_hip_plan_repeat_layout.restype = C.c_int64
    lib.hyphy_hip_plan_repeat_layout.argtypes = [C.c_int64, C.c_int64, lp, C.c_int64, C.c_int64, C.c_int64, lp, lp, C.c_int64, C.c_double, C.c_double,
                                                 C.c_double, C.c_int64, C.c_int64, lp, C.c_int64, C.c_char_p, C.c_int64]
    lib.hyphy_hip_repeat_stats.restype = C.c_int
    lib.hyphy_hip_repeat_stats.argtypes = [vp, lp]
    lib.hyphy_hip_comm_init_host.restype = C.c_int
    lib.hyphy_hip_comm_init_host.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    lib.hyphy_hip_evaluate_exchange.restype = C.c_int
    lib.hyphy_hip_evaluate_exchange.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, C.c_int, dp, dp]
    lib.hyphy_hip_evaluate_built_exchange.restype = C.c_int
    lib.hyphy_hip_evaluate_built_exchange.argtypes = [vp, C.c_int64, lp, C.c_int64, lp, C.c_int64, dp, dp]
    lib.hyphy_hip_xch_open.restype = C.c_int
    lib.hyphy_hip_xch_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.hyphy_hip_xch_sum.restype = C.c_int
    lib.hyphy_hip_xch_sum.argtypes = [C.c_void_p, C.c_double, C.c_int, dp]
    lib.hyphy_hip_xch_close.restype = None
    lib.hyphy_hip_xch_close.argtypes = [C.c_void_p]
    lib.hyphy_hip_plan_nucgen.restype = C.c_int64
    lib.hyphy_hip_plan_nucgen.argtypes = [C.c_int64, C.c_int64, lp, lp, C.c_int64, C.c_char_p, C.c_int64, lp]
    lib.hyphy_hip_plan_switches.restype = C.c_int64
    lib.hyphy_hip_plan_switches.argtypes = [C.c_char_p, C.c_int64]
    lib.hyphy_hip_last_error.restype = C.c_char_p
    lib.hyphy_hip_last_expm_kernel.restype = C.c_char_p
    lib.hyphy_hip_last_expm_kernel.argtypes = []
    bp = C.POINTER(C.c_int8)
    lib.hyphy_hip_hmm_set_sites.restype = C.c_int
    lib.hyphy_hip_hmm_set_sites.argtypes = [vp, C.c_int64, lp]
    lib.hyphy_hip_hmm_logl.restype = C.c_int
    lib.hyphy_hip_hmm_logl.argtypes = [vp, dp, dp, dp]
    lib.hyphy_hip_hmm_viterbi.restype = C.c_int
    lib.hyphy_hip_hmm_viterbi.argtypes = [vp, dp, dp, bp]
    lib.hyphy_hip_evaluate_categories_hmm.restype = C.c_int
    lib.hyphy_hip_evaluate_categories_hmm.argtypes = [vp, lp, C.c_int64, lp, C.c_int64, dp, C.c_int, dp, dp, dp, dp]
    lib.hyphy_hip_evaluate_categories_built_hmm.restype = C.c_int
    lib.hyphy_hip_evaluate_categories_built_hmm.argtypes = [vp, lp, C.c_int64, lp, C.c_int64, dp, dp, dp, dp]
    lib.hyphy_hip_plan_hmm.restype = C.c_int64
    lib.hyphy_hip_plan_hmm.argtypes = [C.c_int64, C.c_int64, lp, C.c_int64]
    lib.hyphy_hip_hmm_host.restype = C.c_int
    lib.hyphy_hip_hmm_host.argtypes = [C.c_int64, C.c_int64, C.c_int64, lp, dp, lp, dp, dp, dp, bp]
    lib.hyphy_hip_version.restype = C.c_char_p
    _lib = lib
    return lib


def _check(rc: int):
    if rc == 0:
        return
    msg = load().hyphy_hip_last_error().decode()
    if rc > 0:
        raise HipUnsupported(msg)
    raise HipError(msg)


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _l(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None


def plan_reroot(flat_parents, L: int, candidate: int = 0) -> np.ndarray:
    """Host-only: internal indices from the given root to the ``candidate``-th height-minimising node (empty: none)."""
    fp = np.ascontiguousarray(flat_parents, dtype=np.int64)
    out = np.zeros(64, dtype=np.int64)
    n = int(load().hyphy_hip_plan_reroot(int(L), len(fp) - int(L), _l(fp), int(candidate), _l(out), len(out)))
    if n < 0:
        raise HipError("plan_reroot: bad arguments")
    return out[:n].copy()


def plan_pattern_order(D: int, leaf_codes) -> np.ndarray:
    """Host-only: the order in which the library stores the patterns on the device (caller's pattern indices)."""
    lc = np.ascontiguousarray(leaf_codes, dtype=np.int64)
    out = np.zeros(lc.shape[1], dtype=np.int64)
    if load().hyphy_hip_plan_pattern_order(int(D), lc.shape[0], lc.shape[1], _l(lc), _l(out)):
        raise HipError("plan_pattern_order: bad arguments")
    return out


def plan_schedule(flat_parents, L: int, kernel: int = 1, chain_m: int = 0, ntiles: int = 64, reroot: bool = False) -> dict:
    """Host-only: compile the steady-state full-pass schedule of a 61-state partition of this shape and decode its join
    table the way the kernels do (include/hyphy_hip.h: hyphy_hip_plan_schedule)."""
    fp = np.ascontiguousarray(flat_parents, dtype=np.int64)
    info = np.zeros(8, dtype=np.int64)
    if load().hyphy_hip_plan_schedule(int(L), len(fp) - int(L), _l(fp), int(kernel), int(chain_m), int(ntiles), int(bool(reroot)), _l(info)):
        raise HipError("plan_schedule: bad arguments")
    keys = ("chain", "programs", "entries", "max_slot", "max_need", "decode_errors", "rerooted", "trunk_nodes")
    return dict(zip(keys, (int(v) for v in info)))


def plan_repeats(flat_parents, L: int, leaf_codes, theta: float = 0.0):
    """Host-only: (classes per internal node, compressed flags, edge products of a full pass with one table per compressed node)."""
    lib = load()
    fp = np.ascontiguousarray(flat_parents, dtype=np.int64)
    lc = np.ascontiguousarray(leaf_codes, dtype=np.int64)
    I = len(fp) - L
    cl = np.zeros(I, dtype=np.int64)
    cp = np.zeros(I, dtype=np.int64)
    work = lib.hyphy_hip_plan_repeats(L, I, _l(fp), lc.shape[1], _l(lc), float(theta), _l(cl), _l(cp))
    if work < 0:
        raise HipError("plan_repeats: bad arguments")
    return cl, cp.astype(bool), int(work)


def plan_repeat_layout(flat_parents, L: int, shard_codes, D: int, n_classes: int = 1, mode: int = -1, theta: float = 0.0, rho: float = -1.0,
                       min_gain: float = -1.0, inline_chains: int = -1, variant: int = 1) -> dict:
    """Host-only: what hyphy_hip_create would upload for the class-compressed form (include/hyphy_hip.h:
    hyphy_hip_plan_repeat_layout).  ``shard_codes``: one [L][S_pad] array per shard, padded as for the device.  Returns
    ``{"declined": reason}`` when the plan declines, else a dict with ``compressed``, ``rep_desc_of``, ``descriptors`` (dicts: node,
    level, path, flags, kids, kid_desc), ``view`` (L, I, parents, slot, leaf_has_ambig, leaf_nodes, children) and ``shards`` (dicts:
    rows, tables [(U, rows, row0, map0)], and the uploaded words maps, desc [n][4], ct, lt [n][2], walk [n][4])."""
    lib = load()
    fp = np.ascontiguousarray(flat_parents, dtype=np.int64)
    I = len(fp) - int(L)
    sp = np.array([np.shape(c)[1] for c in shard_codes], dtype=np.int64)
    lc = np.concatenate([np.ascontiguousarray(c, dtype=np.int64).ravel() for c in shard_codes])
    reason = C.create_string_buffer(256)
    args = (int(L), I, _l(fp), int(D), int(n_classes), len(sp), _l(sp), _l(lc), int(mode), float(theta), float(rho), float(min_gain),
            int(inline_chains), int(variant))
    n = lib.hyphy_hip_plan_repeat_layout(*args, None, 0, reason, len(reason))
    if n == 0:
        return {"declined": reason.value.decode()}
    if n == -1:
        raise HipError("plan_repeat_layout: bad arguments")
    out = np.zeros(-n, dtype=np.int64)
    if lib.hyphy_hip_plan_repeat_layout(*args, _l(out), len(out), reason, len(reason)) != -n:
        raise HipError("plan_repeat_layout: the layout changed size between two calls")
    pos = [0]

    def take(k):
        pos[0] += k
        return out[pos[0] - k: pos[0]]

    def lst(width=1):
        k = int(take(1)[0])
        a = take(k * width).copy()
        return a.reshape(k, width) if width > 1 else a

    ND, vL, vI, nsh, _walk = (int(x) for x in take(5))
    res = {"compressed": lst().astype(bool), "rep_desc_of": lst(), "descriptors": [], "shards": []}
    for _ in range(ND):
        node, level = (int(x) for x in take(2))
        d = {"node": node, "level": level, "path": lst(), "flags": lst(), "kids": [], "kid_desc": []}
        for _x in range(len(d["path"])):
            d["kids"].append(lst())
            d["kid_desc"].append(lst())
        res["descriptors"].append(d)
    res["view"] = {"L": vL, "I": vI, "parents": lst(), "slot": lst(), "leaf_has_ambig": lst(), "leaf_nodes": lst()}
    res["view"]["children"] = [lst() for _ in range(vI)]
    for _ in range(nsh):
        sh = {"rows": int(take(1)[0]), "tables": []}
        for _d in range(ND):
            U, rows, row0 = (int(x) for x in take(3))
            sh["tables"].append((U, rows, row0, lst()))
        sh["maps"], sh["desc"], sh["ct"], sh["lt"], sh["walk"] = lst(), lst(4), lst(), lst(2), lst(4)
        res["shards"].append(sh)
    assert pos[0] == len(out)
    return res


def plan_trunk_walk(parents, L: int):
    """Host-only: the program trunk_walk_kernel runs for a trunk over ``L`` generalised leaves (``parents[c]`` = node code of c's
    parent; internal node i has code L + i, children before parents, the root last).  Returns a dict: ``nodes`` [(internal index or
    -1, leaf children, first input, flags)], ``inputs`` (leaf codes), ``depth``, ``one`` = (first, end) node range of the one-chain
    form, ``two`` = ((first, end), (first, end)) of the two chains or None."""
    lib = load()
    par = np.ascontiguousarray(parents, dtype=np.int64)
    I = len(par) + 1 - L
    cap = 16 + 8 * (L + I) + 4 * L
    out = np.zeros(cap, dtype=np.int64)
    n = lib.hyphy_hip_plan_trunk_walk(L, I, _l(par), _l(out), cap)
    if n < 0:
        raise HipError("plan_trunk_walk: bad arguments")
    nn, ni, depth, two = (int(x) for x in out[:4])
    nodes = [tuple(int(x) for x in out[10 + 4 * k: 14 + 4 * k]) for k in range(nn)]
    inputs = [int(x) for x in out[10 + 4 * nn: 10 + 4 * nn + ni]]
    return {"nodes": nodes, "inputs": inputs, "depth": depth, "one": (int(out[4]), int(out[5])),
            "two": ((int(out[6]), int(out[7])), (int(out[8]), int(out[9]))) if two else None}


def plan_marginal(flat_parents, L: int) -> dict:
    """Host-only: the pre-order program of the marginal-reconstruction pass over a tree (``flat_parents[c]`` = internal index of c's
    parent, internal node i has code L + i, the root last).  Returns ``entries`` [(kind, a, b, c)]: a node header (0, internal
    index, children, is root) followed by its children (1, node code, internal index or -1, position), and ``maxk``."""
    lib = load()
    par = np.ascontiguousarray(flat_parents, dtype=np.int64)
    I = len(par) - int(L)
    need = lib.hyphy_hip_plan_marginal(int(L), I, _l(par), None, 0)
    if need >= 0 or need == -1:
        raise HipError("plan_marginal: " + lib.hyphy_hip_last_error().decode())
    out = np.zeros(-need, dtype=np.int64)
    n = lib.hyphy_hip_plan_marginal(int(L), I, _l(par), _l(out), len(out))
    if n < 0:
        raise HipError("plan_marginal: " + lib.hyphy_hip_last_error().decode())
    ne = int(out[0])
    return {"entries": [tuple(int(x) for x in out[2 + 4 * k: 6 + 4 * k]) for k in range(ne)], "maxk": int(out[1])}


def plan_nni(flat_parents, L: int) -> np.ndarray:
    """Host-only: every nearest-neighbour interchange of a tree as rows (x, y), [n, 2], in ascending (c, y, x): c = parent(x) is an
    internal node other than the root and y a sibling of c; the move exchanges the parents of x and y (``HipPartition.nni_scores``,
    ``hyphy_amd.nni.apply_nni``)."""
    lib = load()
    par = np.ascontiguousarray(flat_parents, dtype=np.int64)
    I = len(par) - int(L)
    out = np.zeros(1, dtype=np.int64)
    n = lib.hyphy_hip_plan_nni(int(L), I, _l(par), _l(out), 1)            # (one word is enough for a tree without a move)
    if n < -1:
        out = np.zeros(-n, dtype=np.int64)
        n = lib.hyphy_hip_plan_nni(int(L), I, _l(par), _l(out), len(out))
    if n < 0:
        raise HipError("plan_nni: " + lib.hyphy_hip_last_error().decode())
    return out[1: 1 + 2 * int(out[0])].reshape(-1, 2).copy()


def check_nni(flat_parents, L: int, moves) -> None:
    """Host-only: raise ``HipError`` naming the first pair of ``moves`` ([n, 2]: x, y) that is not a move of the tree, in the words
    ``HipPartition.nni_scores`` refuses it with; return None when every pair is one."""
    lib = load()
    par = np.ascontiguousarray(flat_parents, dtype=np.int64)
    mv = np.ascontiguousarray(moves, dtype=np.int64).reshape(-1, 2)
    if lib.hyphy_hip_check_nni(int(L), len(par) - int(L), _l(par), len(mv), _l(mv)) < 0:
        raise HipError(lib.hyphy_hip_last_error().decode())


def plan_nucgen(flat_parents, L: int, leaf_has_ambig=None, compile_it: bool = True, small: bool = False):
    """Host-only (libhiprtc, no device): (source of the run-time generated 4-state kernel for this tree's steady-state full pass,
    compiled for gfx950?).  Empty source: the generator does not cover the schedule."""
    lib = load()
    fp = np.ascontiguousarray(flat_parents, dtype=np.int64)
    I = len(fp) - L
    amb = None if leaf_has_ambig is None else np.ascontiguousarray(leaf_has_ambig, dtype=np.int64)
    cap = 1 << 22
    buf = C.create_string_buffer(cap)
    ok = np.zeros(1, dtype=np.int64)
    n = lib.hyphy_hip_plan_nucgen(L, I, _l(fp), _l(amb), 1 if small else 0, buf, cap, _l(ok) if compile_it else None)
    if n < 0:
        raise HipError("plan_nucgen: bad arguments")
    return buf.value.decode(), bool(ok[0])


def plan_hmm(n_sites: int, C: int) -> dict:
    """Host-only: the launches of a hidden-Markov forward sum over ``n_sites`` sites and ``C`` classes: ``G`` (sites per segment =
    blocks per combine), ``levels`` and ``items`` (work items of each level: (block, row) pairs, 1 for the last)."""
    out = np.zeros(32, dtype=np.int64)
    n = int(load().hyphy_hip_plan_hmm(int(n_sites), int(C), _l(out), len(out)))
    if n < 0:
        raise HipError("plan_hmm: bad arguments (1 <= n_sites < 2^31, 2 <= C <= 8)")
    return dict(G=int(out[0]), levels=int(out[1]), items=[int(x) for x in out[2:n]])


def _hmm_params(T, pi, C):
    t = np.ascontiguousarray(T, dtype=np.float64)
    f = np.ascontiguousarray(pi, dtype=np.float64)
    if t.shape != (C, C) or f.shape != (C,):
        raise HipError(f"hmm: transition must be [{C}, {C}] and initial [{C}]")
    return t, f


def hmm_host(lik, cnt, T, pi, pattern_of_site=None, logl: bool = True, path: bool = False):
    """Host-only: the hidden-Markov forward sum / Viterbi path of ``HipPartition.hmm_logl`` / ``hmm_viterbi`` from per-class
    per-pattern values ``lik`` [C, S] and 2^64 exponents ``cnt`` [C, S], run serially over the device's plan.  Returns log L, the
    path (int8 [n_sites]), or both as a tuple."""
    lk = np.ascontiguousarray(lik, dtype=np.float64)
    cn = np.ascontiguousarray(cnt, dtype=np.int64)
    Cc, S = lk.shape
    if cn.shape != lk.shape:
        raise HipError("hmm_host: lik and cnt must both be [C, S]")
    t, f = _hmm_params(T, pi, Cc)
    ps = None if pattern_of_site is None else np.ascontiguousarray(pattern_of_site, dtype=np.int64)
    n = S if ps is None else len(ps)
    out = C.c_double(0.0)
    pth = np.zeros(n, dtype=np.int8) if path else None
    _check(load().hyphy_hip_hmm_host(Cc, S, n, _l(ps), _d(lk), _l(cn), _d(t), _d(f), C.byref(out) if logl else None,
                                     pth.ctypes.data_as(C.POINTER(C.c_int8)) if path else None))
    if logl and path:
        return out.value, pth
    return pth if path else out.value


def plan_switches() -> list:
    """Host-only: the library's environment switches (csrc/switches.h, docs/switches.md), one dict per row with ``name`` (without
    the HYPHY_HIP_ prefix), ``kind``, ``when`` (process | create | call), ``audience`` (integrator | diagnostic), ``default`` and
    ``value``: what the switch parses to in the environment as it is now (a fresh read, also of what the library caches per process)."""
    lib = load()
    need = -lib.hyphy_hip_plan_switches(None, 0)
    buf = C.create_string_buffer(need)
    if lib.hyphy_hip_plan_switches(buf, need) != need:
        raise HipError("plan_switches: the table changed size between two calls")
    keys = ("name", "kind", "when", "audience", "default", "value")
    return [dict(zip(keys, line.split("\t"))) for line in buf.value.decode().splitlines()]


class HostExchange:
    """The collective-free combine of one-process-per-GPU runs on one node (hyphy_hip_xch_*): every rank posts its partial
    log-likelihood into a shared-memory segment and reads the others'; ``sum`` returns the total (same bits on every rank)."""

    def __init__(self, name: str, rank: int, n_ranks: int):
        self._lib = load()
        h = C.c_void_p()
        _check(self._lib.hyphy_hip_xch_open(name.encode(), int(rank), int(n_ranks), C.byref(h)))
        self._h = h

    def sum(self, local: float, failed: bool = False) -> float:
        out = C.c_double(0.0)
        _check(self._lib.hyphy_hip_xch_sum(self._h, float(local), 1 if failed else 0, C.byref(out)))
        return out.value

    def close(self):
        if self._h:
            self._lib.hyphy_hip_xch_close(self._h)
            self._h = None


def device_count() -> int:
    return int(load().hyphy_hip_device_count())


def expm_batch(Q: np.ndarray) -> np.ndarray:
    """Batched P = exp(Q) on the device (drop-in for the loop at ``tree.cpp:3011-3037``)."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    single = Q.ndim == 2
    Qb = Q[None] if single else Q
    P = np.empty_like(Qb)
    _check(load().hyphy_hip_expm_batch(Qb.shape[1], Qb.shape[0], _d(Qb), _d(P)))
    return P[0] if single else P


def expm_frechet_adjoint_batch(Q: np.ndarray, W: np.ndarray) -> np.ndarray:
    """Batched L(Q^T, W) on the device, L(A, E) = int_0^1 exp(sA) E exp((1 - s)A) ds: with W = d f / d exp(Q) it is d f / d Q, the
    entries of Q taken as independent.  NaN where a matrix cannot be handled."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    W = np.ascontiguousarray(W, dtype=np.float64)
    if Q.shape != W.shape or Q.ndim not in (2, 3) or Q.shape[-1] != Q.shape[-2]:
        raise ValueError(f"expected two arrays of [n, D, D], got {Q.shape} and {W.shape}")
    single = Q.ndim == 2
    Qb, Wb = (Q[None], W[None]) if single else (Q, W)
    out = np.empty_like(Qb)
    _check(load().hyphy_hip_expm_frechet_adjoint_batch(Qb.shape[1], Qb.shape[0], _d(Qb), _d(Wb), _d(out)))
    return out[0] if single else out


def sample_uniforms(seed: int, n_rep: int, I: int, n_sites: int) -> np.ndarray:
    """Host-only: the uniforms [n_rep, I, n_sites] that ``HipPartition.sample_ancestral`` draws with under ``seed`` when none are
    supplied (Philox4x32-10, counter = (site, node, replicate, 0))."""
    out = np.zeros((int(n_rep), int(I), int(n_sites)))
    _check(load().hyphy_hip_sample_uniforms(C.c_uint64(int(seed) & (2 ** 64 - 1)), int(n_rep), int(I), int(n_sites), _d(out)))
    return out


def simulate_uniforms(seed: int, n_rep: int, n_nodes: int, n_sites: int) -> np.ndarray:
    """Host-only: the uniforms [n_rep, n_nodes, n_sites] (nodes by node code) that ``HipPartition.simulate`` draws with under
    ``seed`` when none are supplied (Philox4x32-10, counter = (site, node code, replicate, 1))."""
    out = np.zeros((int(n_rep), int(n_nodes), int(n_sites)))
    _check(load().hyphy_hip_simulate_uniforms(C.c_uint64(int(seed) & (2 ** 64 - 1)), int(n_rep), int(n_nodes), int(n_sites), _d(out)))
    return out


def pack_mixture(n_q: int, components, weights, tail_ndim: int):
    """Host-only: what the mixture entry points pass on.  ``components``: one array [n_q, M, ...] (the same M on every branch), or a
    sequence of n_q per-branch arrays [M_k, ...] (``tail_ndim`` trailing axes: 2 for rate matrices, 1 for coefficient rows);
    ``weights`` [n_q, M], or a sequence of [M_k].  Returns (components [sum M_k, ...], weights [sum M_k], counts [n_q]), branch-major:
    the components of the first branch, then those of the second, ..."""
    if isinstance(components, np.ndarray) and components.ndim == tail_ndim + 2:
        q = np.ascontiguousarray(components, dtype=np.float64)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert w.shape == q.shape[:2] and q.shape[0] == n_q
        return q.reshape((q.shape[0] * q.shape[1],) + q.shape[2:]), w.reshape(-1), np.full(n_q, q.shape[1], dtype=np.int64)
    per = [np.asarray(c, dtype=np.float64) for c in components]
    wts = [np.asarray(x, dtype=np.float64).reshape(-1) for x in weights]
    assert len(per) == n_q and len(wts) == n_q, (len(per), len(wts), n_q)
    for c, x in zip(per, wts):
        assert c.ndim == tail_ndim + 1 and c.shape[0] == len(x) and c.shape[1:] == per[0].shape[1:], (c.shape, x.shape)
    cnt = np.array([len(x) for x in wts], dtype=np.int64)
    if not n_q:
        return np.zeros((0,) * (tail_ndim + 1)), np.zeros(0), cnt
    return np.ascontiguousarray(np.concatenate(per, axis=0)), np.ascontiguousarray(np.concatenate(wts)), cnt


def pack_class_mixture(n_q: int, components, weights, tail_ndim: int):
    """Host-only: what the class-batched mixture entry points pass on.  ``components`` and ``weights``: a sequence over the rate
    classes of what ``pack_mixture`` takes for one class, under the same component counts in every class (ValueError otherwise, and
    for no class at all).  Returns (components [C * n_tot, ...], weights [C * n_tot], counts [n_q]): class-major, inside a class
    branch-major."""
    if len(components) != len(weights) or len(components) < 1:
        raise ValueError(f"pack_class_mixture: {len(components)} classes of components, {len(weights)} of weights")
    packed = [pack_mixture(n_q, q, w, tail_ndim) for q, w in zip(components, weights)]
    cnt = packed[0][2]
    for c, (q, w, k) in enumerate(packed):
        if not np.array_equal(k, cnt):
            raise ValueError(f"pack_class_mixture: class {c} has other component counts than class 0")
        if q.shape[1:] != packed[0][0].shape[1:]:
            raise ValueError(f"pack_class_mixture: class {c} has components of another shape than class 0")
    return (np.ascontiguousarray(np.concatenate([x[0] for x in packed], axis=0)), np.ascontiguousarray(np.concatenate([x[1] for x in packed])),
            cnt)


def last_expm_kernel() -> str:
    """The matrix-exponential kernel this thread's last launch ran ("expm64_kernel<2>", "expm_mfma_kernel<4,2>", "expm_nuc_kernel",
    ...); "" before the first launch and when the exponentials were folded into a pruning launch."""
    return load().hyphy_hip_last_expm_kernel().decode()


class HipPartition:
    """Device-resident state of one (filter, tree) partition."""

    def __init__(self, D: int, flat_parents, L: int, leaf_codes, ambig, pattern_freq, C_cat: int = 1,
                 device_first: int = 0, device_count: int = 1):
        lib = load()
        self.D, self.L = int(D), int(L)
        fp = np.ascontiguousarray(flat_parents, dtype=np.int64)
        self.I = len(fp) - self.L
        codes = np.ascontiguousarray(leaf_codes, dtype=np.int64)
        self.S = int(codes.shape[1])
        self.C = int(C_cat)
        self._hmm_n = 0                    # sites of the list set through hmm_set_sites (0: none)
        self.B = self.L + self.I - 1
        amb = np.ascontiguousarray(ambig, dtype=np.float64) if ambig is not None and len(ambig) else None
        freq = np.ascontiguousarray(pattern_freq, dtype=np.int64)
        h = C.c_void_p()
        _check(lib.hyphy_hip_create(C.byref(h), self.D, self.S, self.L, self.I, self.C, _l(fp), _l(codes),
                                    _d(amb), 0 if amb is None else amb.shape[0], _l(freq), device_first, device_count))
        self._h = h
        self._lib = lib

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hyphy_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- evaluation -------------------------------------------------------------------------
    def evaluate(self, update_nodes, q_nodes, q_dense, root_freqs, cat: int = -1, q_is_probability: bool = False,
                 per_site: bool = False):
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        q = np.ascontiguousarray(q_dense, dtype=np.float64) if len(qn) else None
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_evaluate(self._h, cat, _l(un), len(un), _l(qn), len(qn), _d(q),
                                            int(q_is_probability), _d(rf), C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    # -- RCCL (one process per GPU: the C-ABI's own all-reduce of the partition log-likelihood) ---------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(load().hyphy_hip_comm_unique_id(C.cast(buf, C.c_void_p)))
        return buf.raw

    def comm_init_rank(self, unique_id: bytes, rank: int, n_ranks: int):
        buf = C.create_string_buffer(unique_id, 128)
        _check(self._lib.hyphy_hip_comm_init_rank(self._h, C.cast(buf, C.c_void_p), rank, n_ranks))

    def comm_init_all(self):
        _check(self._lib.hyphy_hip_comm_init_all(self._h))

    def evaluate_allreduce(self, update_nodes, q_nodes, q_dense, root_freqs, cat: int = -1, q_is_probability: bool = False):
        """``evaluate`` on this rank's pattern shard + one RCCL all-reduce of the partial log-L: the whole alignment's value."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        q = np.ascontiguousarray(q_dense, dtype=np.float64) if len(qn) else None
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        _check(self._lib.hyphy_hip_evaluate_allreduce(self._h, cat, _l(un), len(un), _l(qn), len(qn), _d(q), int(q_is_probability),
                                                      _d(rf), C.byref(out)))
        return out.value

    def evaluate_mixture(self, update_nodes, q_nodes, q_components, weights, root_freqs, cat: int = -1, per_site: bool = False):
        """Branch-site mixture on every listed branch: ``q_components`` [n_q, M, D, D] rate matrices, ``weights`` [n_q, M], or a
        sequence of per-branch arrays [M_k, D, D] and [M_k] (1 to 16 components, any count per branch: ``pack_mixture``);
        the device forms ``P_k = sum_m w_km exp(Q_km)`` (explicit-form models: BUSTED / BS-REL)."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        q, w, cnt = pack_mixture(len(qn), q_components, weights, 2)
        assert q.ndim == 3 and q.shape[1:] == (self.D, self.D)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_evaluate_mixture(self._h, cat, _l(un), len(un), _l(qn), len(qn), _l(cnt), _d(q), _d(w),
                                                    _d(rf), C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def evaluate_mixture_built(self, update_nodes, q_nodes, coeffs, weights, root_freqs, cat: int = -1, per_site: bool = False):
        """The same with the component rate matrices formed on the device from the uploaded templates: ``coeffs`` [n_q, M, K]
        or a sequence of per-branch [M_k, K] (one coefficient row per branch and component, ``sum M_k`` rows in all:
        ``hyphy_hip_build_q`` + ``hyphy_hip_evaluate_mixture_built``)."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        c, w, cnt = pack_mixture(len(qn), coeffs, weights, 1)
        assert c.ndim == 2
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_build_q(self._h, c.shape[0], _d(c)))
        _check(self._lib.hyphy_hip_evaluate_mixture_built(self._h, cat, _l(un), len(un), _l(qn), len(qn), _l(cnt), _d(w), _d(rf),
                                                          C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def prepare_mixture_built_step(self, update_nodes, q_nodes, weights, root_freqs, coeffs: np.ndarray, cat: int = -1, counts=None):
        """Zero-argument callable: ``build_q`` of one coefficient row per (branch, component) + ``evaluate_mixture_built`` -> log-L.
        ``coeffs`` [n_q, M, K] and ``weights`` [n_q, M] are read at call time.  ``counts`` [n_q]: a component count per branch;
        ``coeffs`` is then [sum counts, K] and ``weights`` [sum counts], branch-major (``pack_mixture``)."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        assert coeffs.flags.c_contiguous and coeffs.dtype == np.float64 and weights.flags.c_contiguous and weights.dtype == np.float64
        if counts is None:
            assert coeffs.ndim == 3 and coeffs.shape[0] == len(qn) and weights.shape == coeffs.shape[:2]
            cnt = np.full(len(qn), coeffs.shape[1], dtype=np.int64)
        else:
            cnt = np.ascontiguousarray(counts, dtype=np.int64)
            assert cnt.shape == (len(qn),) and coeffs.ndim == 2 and coeffs.shape[0] == int(cnt.sum()) and weights.shape == (coeffs.shape[0],)
        keep = (un, qn, rf, coeffs, weights, cnt)
        lib, h = self._lib, self._h
        pun, pqn, prf, pco, pw, pcnt = _l(un), _l(qn), _d(rf), _d(coeffs), _d(weights), _l(cnt)
        nun, nqn, nrows = len(un), len(qn), int(cnt.sum())
        out = C.c_double(0.0)
        pout = C.byref(out)

        def step(_keep=keep):
            rc = lib.hyphy_hip_build_q(h, nrows, pco)
            if rc == 0:
                rc = lib.hyphy_hip_evaluate_mixture_built(h, cat, pun, nun, pqn, nqn, pcnt, pw, prf, pout, None, None)
            if rc:
                _check(rc)
            return out.value
        return step

    def evaluate_async(self, update_nodes, q_nodes, q_dense, root_freqs, cat: int = -1, q_is_probability: bool = False):
        """Enqueue an evaluation and return at once (``collect`` waits for it): lets the partitions of one
        likelihood function overlap on different devices / streams."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        q = np.ascontiguousarray(q_dense, dtype=np.float64) if len(qn) else None
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        _check(self._lib.hyphy_hip_evaluate_async(self._h, cat, _l(un), len(un), _l(qn), len(qn), _d(q),
                                                  int(q_is_probability), _d(rf)))

    def collect(self, per_site: bool = False):
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_collect(self._h, C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def evaluate_device(self, update_nodes, q_nodes, d_q_ptr: int, root_freqs, d_logl_ptr: int, cat: int = -1,
                        q_is_probability: bool = False):
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        _check(self._lib.hyphy_hip_evaluate_device(self._h, cat, _l(un), len(un), _l(qn), len(qn),
                                                   C.c_void_p(d_q_ptr), int(q_is_probability), _d(rf),
                                                   C.c_void_p(d_logl_ptr)))

    def prepare_device_step(self, update_nodes, q_nodes, root_freqs, d_logl_ptr: int, coeffs: np.ndarray,
                            cat: int = -1):
        """Returns a zero-argument callable that enqueues ``build_q(coeffs)`` + ``evaluate_device`` with
        all ctypes arguments marshalled ONCE (numpy's ``.ctypes.data_as`` costs tens of microseconds per
        call — more than the C-ABI calls themselves).  ``coeffs`` is read at call time (update it in
        place between calls)."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        assert coeffs.flags.c_contiguous and coeffs.dtype == np.float64
        keep = (un, qn, rf, coeffs)
        lib, h = self._lib, self._h
        pun, pqn, prf, pco = _l(un), _l(qn), _d(rf), _d(coeffs)
        nun, nqn, nco = len(un), len(qn), coeffs.shape[0]
        dq, dl = C.c_void_p(self.q_buffer()), C.c_void_p(d_logl_ptr)

        def step(_keep=keep):
            rc = lib.hyphy_hip_build_q(h, nco, pco)
            if rc == 0:
                rc = lib.hyphy_hip_evaluate_device(h, cat, pun, nun, pqn, nqn, dq, 0, prf, dl)
            if rc:
                _check(rc)
        return step

    def prepare_fetch(self, d_ptr: int):
        """Zero-argument callable: the double at device address ``d_ptr`` (written by work queued on this partition's
        stream, e.g. an all-reduce behind ``evaluate_device``) through the host-mapped result record -> float."""
        lib, h, src, out = self._lib, self._h, C.c_void_p(d_ptr), C.c_double(0.0)
        ref = C.byref(out)

        def fetch():
            rc = lib.hyphy_hip_fetch_device_scalar(h, src, ref)
            if rc:
                _check(rc)
            return out.value
        return fetch

    def prepare_built_step(self, update_nodes, q_nodes, root_freqs, coeffs: np.ndarray, cat: int = -1):
        """Zero-argument callable: ``build_q(coeffs)`` + synchronous ``evaluate_built`` -> log-L (float).
        ctypes arguments are marshalled once; ``coeffs`` is read at call time."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        assert coeffs.flags.c_contiguous and coeffs.dtype == np.float64
        keep = (un, qn, rf, coeffs)
        lib, h = self._lib, self._h
        pun, pqn, prf, pco = _l(un), _l(qn), _d(rf), _d(coeffs)
        nun, nqn, nco = len(un), len(qn), coeffs.shape[0]
        out = C.c_double(0.0)
        pout = C.byref(out)

        def step(_keep=keep):
            rc = lib.hyphy_hip_build_q(h, nco, pco)
            if rc == 0:
                rc = lib.hyphy_hip_evaluate_built(h, cat, pun, nun, pqn, nqn, prf, pout)
            if rc:
                _check(rc)
            return out.value
        return step

    def prepare_built_allreduce_step(self, update_nodes, q_nodes, root_freqs, coeffs: np.ndarray, cat: int = -1):
        """Zero-argument callable: ``build_q(coeffs)`` + ``evaluate_built_allreduce`` -> log-L of the WHOLE alignment on every
        rank (local evaluation of this rank's pattern shard, one ncclAllReduce in the partition's stream, value back through
        the host-mapped record).  Needs ``comm_init_rank`` first."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        assert coeffs.flags.c_contiguous and coeffs.dtype == np.float64
        keep = (un, qn, rf, coeffs)
        lib, h = self._lib, self._h
        pun, pqn, prf, pco = _l(un), _l(qn), _d(rf), _d(coeffs)
        nun, nqn, nco = len(un), len(qn), coeffs.shape[0]
        out = C.c_double(0.0)
        pout = C.byref(out)

        def step(_keep=keep):
            rc = lib.hyphy_hip_build_q(h, nco, pco)
            if rc == 0:
                rc = lib.hyphy_hip_evaluate_built_allreduce(h, cat, pun, nun, pqn, nqn, prf, pout)
            if rc:
                _check(rc)
            return out.value
        return step

    def comm_init_host(self, name: str, rank: int, n_ranks: int):
        """Attach this rank's partition to the run's shared-memory exchange (collective-free combine, one node)."""
        _check(self._lib.hyphy_hip_comm_init_host(self._h, name.encode(), int(rank), int(n_ranks)))

    def prepare_built_exchange_step(self, update_nodes, q_nodes, root_freqs, coeffs: np.ndarray, cat: int = -1):
        """``build_q`` + ``evaluate_built_exchange``: the local evaluation, then ONE host-side exchange of the partial log-likelihoods
        through shared memory (no collective on the device); the total on every rank.  Needs ``comm_init_host`` first."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        assert coeffs.flags.c_contiguous and coeffs.dtype == np.float64
        keep = (un, qn, rf, coeffs)
        lib, h = self._lib, self._h
        pun, pqn, prf, pco = _l(un), _l(qn), _d(rf), _d(coeffs)
        nun, nqn, nco = len(un), len(qn), coeffs.shape[0]
        out = C.c_double(0.0)
        pout = C.byref(out)

        def step(_keep=keep):
            rc = lib.hyphy_hip_build_q(h, nco, pco)
            if rc == 0:
                rc = lib.hyphy_hip_evaluate_built_exchange(h, cat, pun, nun, pqn, nqn, prf, pout)
            if rc:
                _check(rc)
            return out.value
        return step

    def last_allreduce_ms(self) -> float:
        """Event-timed duration of the last in-stream all-reduce (``set_all_timings(True)``), ms."""
        return float(self._lib.hyphy_hip_last_allreduce_ms(self._h))

    def prepare_built_categories_step(self, update_nodes, q_nodes, weights, root_freqs, coeffs: np.ndarray):
        """``build_q`` (C*n_q coefficient rows, class-major) + ``evaluate_categories_built`` -> log-L."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        wt = np.ascontiguousarray(weights, dtype=np.float64)
        assert coeffs.flags.c_contiguous and coeffs.dtype == np.float64 and coeffs.shape[0] == self.C * len(qn)
        keep = (un, qn, rf, wt, coeffs)
        lib, h = self._lib, self._h
        pun, pqn, prf, pwt, pco = _l(un), _l(qn), _d(rf), _d(wt), _d(coeffs)
        nun, nqn, nco = len(un), len(qn), coeffs.shape[0]
        out = C.c_double(0.0)
        pout = C.byref(out)

        def step(_keep=keep):
            rc = lib.hyphy_hip_build_q(h, nco, pco)
            if rc == 0:
                rc = lib.hyphy_hip_evaluate_categories_built(h, pun, nun, pqn, nqn, pwt, prf, pout)
            if rc:
                _check(rc)
            return out.value
        return step

    def evaluate_categories_built_sites(self, update_nodes, q_nodes, weights, root_freqs, coeffs: np.ndarray):
        """``build_q`` (C*n_q coefficient rows, class-major) + ``evaluate_categories_built_sites`` -> (log-L, mixed per-pattern
        likelihoods, mixed 2^64 exponents) — what the host's weighted-sum category loop leaves in its buffer and scalers."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        wt = np.ascontiguousarray(weights, dtype=np.float64)
        co = np.ascontiguousarray(coeffs, dtype=np.float64)
        assert co.shape[0] == self.C * len(qn)
        out = C.c_double(0.0)
        sl = np.zeros(self.S)
        sc = np.zeros(self.S, dtype=np.int64)
        _check(self._lib.hyphy_hip_build_q(self._h, co.shape[0], _d(co)))
        _check(self._lib.hyphy_hip_evaluate_categories_built_sites(self._h, _l(un), len(un), _l(qn), len(qn), _d(wt), _d(rf),
                                                                   C.byref(out), _d(sl), _l(sc)))
        return out.value, sl, sc

    def evaluate_categories(self, update_nodes, q_nodes, q_dense, weights, root_freqs, q_is_probability: bool = False,
                            per_site: bool = False):
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        q = np.ascontiguousarray(q_dense, dtype=np.float64) if len(qn) else None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_evaluate_categories(self._h, _l(un), len(un), _l(qn), len(qn), _d(q),
                                                       int(q_is_probability), _d(w), _d(rf), C.byref(out), _d(sl),
                                                       _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def evaluate_categories_mixture(self, update_nodes, q_nodes, q_components, mix_weights, class_weights, root_freqs,
                                    per_site: bool = False):
        """Rate classes over branch-site mixtures in one batched evaluation: ``q_components`` and ``mix_weights`` are sequences
        over the classes of what ``evaluate_mixture`` takes for one class (the same component counts in every class:
        ``pack_class_mixture``), ``class_weights`` [C].  With no branch listed both may be empty: a re-mix, or a pure update."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        q = w = cnt = None
        if len(qn):
            q, w, cnt = pack_class_mixture(len(qn), q_components, mix_weights, 2)
            assert q.ndim == 3 and q.shape[1:] == (self.D, self.D) and q.shape[0] == self.C * int(cnt.sum()), q.shape
        cw = None if class_weights is None else np.ascontiguousarray(class_weights, dtype=np.float64)
        assert cw is None or cw.shape == (self.C,)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_evaluate_categories_mixture(self._h, _l(un), len(un), _l(qn), len(qn), _l(cnt), _d(q), _d(w), _d(cw),
                                                               _d(rf), C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def evaluate_categories_mixture_built(self, update_nodes, q_nodes, coeffs, mix_weights, class_weights, root_freqs,
                                          per_site: bool = False):
        """The same with the components formed on the device: ``coeffs`` is a sequence over the classes of what
        ``evaluate_mixture_built`` takes (``hyphy_hip_build_q`` of one row per (class, branch, component) +
        ``hyphy_hip_evaluate_categories_mixture_built``).  With no branch listed nothing is staged."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        w = cnt = None
        if len(qn):
            c, w, cnt = pack_class_mixture(len(qn), coeffs, mix_weights, 1)
            assert c.ndim == 2 and c.shape[0] == self.C * int(cnt.sum()), c.shape
            _check(self._lib.hyphy_hip_build_q(self._h, c.shape[0], _d(c)))
        cw = None if class_weights is None else np.ascontiguousarray(class_weights, dtype=np.float64)
        assert cw is None or cw.shape == (self.C,)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_evaluate_categories_mixture_built(self._h, _l(un), len(un), _l(qn), len(qn), _l(cnt), _d(w), _d(cw),
                                                                     _d(rf), C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def hmm_set_sites(self, pattern_of_site=None):
        """The site list of the hidden-Markov entry points: the pattern (caller's order) of each site in alignment order;
        ``None``: site j is pattern j.  Stays on the device until replaced."""
        ps = None if pattern_of_site is None else np.ascontiguousarray(pattern_of_site, dtype=np.int64)
        n = self.S if ps is None else len(ps)
        _check(self._lib.hyphy_hip_hmm_set_sites(self._h, n, _l(ps)))
        self._hmm_n = n

    def hmm_logl(self, T, pi) -> float:
        """log L of the hidden-Markov chain over the site list from the RESIDENT per-class values (no tree work)."""
        t, f = _hmm_params(T, pi, self.C)
        out = C.c_double(0.0)
        _check(self._lib.hyphy_hip_hmm_logl(self._h, _d(t), _d(f), C.byref(out)))
        return out.value

    def hmm_viterbi(self, T, pi) -> np.ndarray:
        """The Viterbi path over the site list (int8 [n_sites]; all -1: no path of positive probability, or a NaN)."""
        t, f = _hmm_params(T, pi, self.C)
        if self._hmm_n <= 0:  # (the library writes n_sites bytes: the size must be known here)
            raise HipError("hmm_viterbi: no site list set through this object's hmm_set_sites")
        pth = np.zeros(self._hmm_n, dtype=np.int8)
        _check(self._lib.hyphy_hip_hmm_viterbi(self._h, _d(t), _d(f), pth.ctypes.data_as(C.POINTER(C.c_int8))))
        return pth

    def evaluate_categories_hmm(self, update_nodes, q_nodes, q_dense, T, pi, root_freqs, q_is_probability: bool = False) -> float:
        """``evaluate_categories`` with the hidden-Markov combine in place of the weighted mix: one wait."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        q = np.ascontiguousarray(q_dense, dtype=np.float64) if len(qn) else None
        t, f = _hmm_params(T, pi, self.C)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        _check(self._lib.hyphy_hip_evaluate_categories_hmm(self._h, _l(un), len(un), _l(qn), len(qn), _d(q), int(q_is_probability),
                                                           _d(t), _d(f), _d(rf), C.byref(out)))
        return out.value

    def evaluate_categories_built_hmm(self, update_nodes, q_nodes, T, pi, root_freqs, coeffs: np.ndarray) -> float:
        """``build_q`` (C*n_q coefficient rows, class-major) + ``evaluate_categories_built`` with the hidden-Markov combine."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        t, f = _hmm_params(T, pi, self.C)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        co = np.ascontiguousarray(coeffs, dtype=np.float64)
        assert co.shape[0] == self.C * len(qn)
        out = C.c_double(0.0)
        _check(self._lib.hyphy_hip_build_q(self._h, co.shape[0], _d(co)))
        _check(self._lib.hyphy_hip_evaluate_categories_built_hmm(self._h, _l(un), len(un), _l(qn), len(qn), _d(t), _d(f), _d(rf),
                                                                 C.byref(out)))
        return out.value

    def download_partials(self, cat: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        cache = np.zeros((self.I, self.S, self.D))
        counts = np.zeros((self.I, self.S), dtype=np.int64)
        _check(self._lib.hyphy_hip_download_partials(self._h, cat, _d(cache), _l(counts)))
        return cache, counts

    def set_pinned_states(self, node=None, states=None):
        """Fix node ``node`` (node code) to ``states[pattern]`` for the evaluations that follow; ``None`` removes it."""
        if node is None:
            _check(self._lib.hyphy_hip_set_pinned_states(self._h, -1, None))
            return
        st = np.ascontiguousarray(states, dtype=np.int64)
        assert st.shape == (self.S,)
        _check(self._lib.hyphy_hip_set_pinned_states(self._h, int(node), _l(st)))

    def marginal_ancestral(self, which: str = "internal", weights=None, support: bool = True, map: bool = False):
        """Marginal ancestral reconstruction in one pass over the resident conditionals (call after an evaluation of every
        class).  ``which``: "internal" (rows = internal nodes) or "leaves" (rows = leaves, unnormalised L_s(leaf = x) / L_s).
        ``weights``: class weights when C > 1.  Returns the support [rows, S, D] (``support``), and with ``map`` also the MAP
        state [rows, S] and its support [rows, S]: a single array, or a tuple of those asked for.  A class under which a pattern
        is impossible (or of weight 0) takes no part in that pattern's rows; a pattern impossible under every class has NaN
        support, MAP state -1 and MAP support NaN."""
        if which not in ("internal", "leaves"):
            raise ValueError("which must be 'internal' or 'leaves'")
        rows = self.I if which == "internal" else self.L
        w = None
        if self.C > 1:
            if weights is None:
                raise ValueError("weights are required when C > 1")
            w = np.ascontiguousarray(weights, dtype=np.float64)
            assert w.shape == (self.C,)
        sup = np.zeros((rows, self.S, self.D)) if support else None
        ms = np.zeros((rows, self.S), dtype=np.int64) if map else None
        mv = np.zeros((rows, self.S)) if map else None
        _check(self._lib.hyphy_hip_marginal_ancestral(self._h, 0 if which == "internal" else 1, _d(w), _d(sup), _l(ms), _d(mv)))
        out = tuple(x for x in (sup, ms, mv) if x is not None)
        return out[0] if len(out) == 1 else out

    def joint_ancestral(self, do_leaves: bool = False, class_of_pattern=None) -> np.ndarray:
        """Joint maximum-likelihood ancestral states (the reference's default ``ReconstructAncestors``) under the matrices, root
        frequencies and leaf data of the last evaluation: int64 [I (+ L with ``do_leaves``), S], rows = internal nodes by internal
        index (the root last), then the leaves; -1 where a node is completely unresolved.  ``class_of_pattern`` [S]: the rate class
        whose matrices each pattern uses (default: class 0).  Nothing on the device changes."""
        cls = None
        if class_of_pattern is not None:
            cls = np.ascontiguousarray(class_of_pattern, dtype=np.int64)
            assert cls.shape == (self.S,)
        out = np.full((self.I + (self.L if do_leaves else 0), self.S), -2, dtype=np.int64)
        _check(self._lib.hyphy_hip_joint_ancestral(self._h, int(bool(do_leaves)), _l(cls), _l(out)))
        return out

    def sample_ancestral(self, n_rep: int, pattern_of_site=None, class_of_pattern=None, seed: int = 0, uniforms=None) -> np.ndarray:
        """Posterior draws of the internal nodes' states (the reference's ``SampleAncestors``) under the matrices, root frequencies,
        leaf data and conditionals of the last evaluation: int8 [n_rep, I, n_sites], internal index (the root last), -1 where the
        pattern is impossible.  ``pattern_of_site`` [n_sites]: the pattern each site shows (default: site j = pattern j);
        ``class_of_pattern`` [S]: the rate class of each pattern (default: class 0); ``uniforms`` [n_rep, I, n_sites] in [0, 1): the
        uniform of every draw (default: Philox4x32-10 keyed by ``seed``, see ``sample_uniforms``).  Nothing on the device changes."""
        pos = None
        n_sites = self.S
        if pattern_of_site is not None:
            pos = np.ascontiguousarray(pattern_of_site, dtype=np.int64).reshape(-1)
            n_sites = len(pos)
        cls = None
        if class_of_pattern is not None:
            cls = np.ascontiguousarray(class_of_pattern, dtype=np.int64)
            assert cls.shape == (self.S,)
        u = None
        if uniforms is not None:
            u = np.ascontiguousarray(uniforms, dtype=np.float64)
            assert u.shape == (int(n_rep), self.I, n_sites)
        out = np.full((int(n_rep), self.I, n_sites), -2, dtype=np.int8)
        _check(self._lib.hyphy_hip_sample_ancestral(self._h, int(n_rep), n_sites, _l(pos), _l(cls), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                    _d(u), out.ctypes.data_as(C.POINTER(C.c_int8))))
        return out

    def simulate(self, n_rep: int, n_sites: int, class_of_site=None, root_states=None, seed: int = 0, uniforms=None,
                 with_internal: bool = False) -> np.ndarray:
        """Alignments drawn down the tree (the reference's ``SimulateDataSet``) under the matrices of the last evaluation of each
        referenced class and the root frequencies on the device: int8 [n_rep, L (+ I with ``with_internal``), n_sites] by node
        code (leaves, then internal nodes, the root last), -1 where a row has no positive total.  ``class_of_site``
        [n_rep, n_sites]: the rate class of each column (default: class 0); ``root_states`` [n_rep, n_sites]: the root's state
        (default: drawn from pi); ``uniforms`` [n_rep, L + I, n_sites] in [0, 1): the uniform of every draw (default:
        Philox4x32-10 keyed by ``seed``, see ``simulate_uniforms``).  Nothing on the device changes."""
        n_rep, n_sites = int(n_rep), int(n_sites)
        rows = self.L + self.I

        def per_column(x):
            if x is None:
                return None
            x = np.ascontiguousarray(x, dtype=np.int64)
            assert x.shape == (n_rep, n_sites)
            return x
        cls, root = per_column(class_of_site), per_column(root_states)
        u = None
        if uniforms is not None:
            u = np.ascontiguousarray(uniforms, dtype=np.float64)
            assert u.shape == (n_rep, rows, n_sites)
        out = np.full((max(n_rep, 0), rows if with_internal else self.L, max(n_sites, 0)), -2, dtype=np.int8)
        _check(self._lib.hyphy_hip_simulate(self._h, n_rep, n_sites, _l(cls), _l(root), C.c_uint64(int(seed) & (2 ** 64 - 1)), _d(u),
                                            int(bool(with_internal)), out.ctypes.data_as(C.POINTER(C.c_int8))))
        return out

    # -- trial matrices on any number of branches from one outside pass ----------------------------
    def _trial_args(self, nodes, mats, tail, weights, per_site):
        nd = np.ascontiguousarray(nodes, dtype=np.int64).reshape(-1)
        m = np.ascontiguousarray(mats, dtype=np.float64)
        if m.size != len(nd) * self.C * int(np.prod(tail)):
            raise ValueError(f"expected [{len(nd)}, {self.C}, {', '.join(str(x) for x in tail)}] values, got {m.shape}")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            assert w.shape == (self.C,)
        ll = np.zeros(len(nd))
        sl = np.zeros((len(nd), self.S)) if per_site else None
        sc = np.zeros((len(nd), self.S), dtype=np.int64) if per_site else None
        return nd, m, w, ll, sl, sc

    def branch_trials(self, nodes, q_dense, weights=None, q_is_probability: bool = False, per_site: bool = False):
        """log-L [n_trials] with the matrix of branch ``nodes[t]`` replaced by exp(``q_dense[t]``) (``q_dense``: [n_trials, D, D], or
        [n_trials, C, D, D] with one matrix per rate class), everything else as at the last evaluation of every class: one outside
        pass serves every trial of the call.  ``weights``: class weights when C > 1.  ``per_site``: also the per-pattern values and
        2^64 exponents, [n_trials, S] each.  Nothing on the device changes."""
        nd, q, w, ll, sl, sc = self._trial_args(nodes, q_dense, (self.D, self.D), weights, per_site)
        _check(self._lib.hyphy_hip_branch_trials(self._h, len(nd), _l(nd), _d(q), int(q_is_probability), _d(w), _d(ll), _d(sl), _l(sc)))
        return (ll, sl, sc) if per_site else ll

    def branch_trials_built(self, nodes, coeffs, weights=None, per_site: bool = False):
        """``branch_trials`` with the trial rate matrices formed on the device from coefficient rows over the templates of
        ``set_q_templates`` (``coeffs``: [n_trials, K] or [n_trials, C, K]), as ``build_q`` forms them."""
        K = int(np.asarray(coeffs).shape[-1])
        nd, co, w, ll, sl, sc = self._trial_args(nodes, coeffs, (K,), weights, per_site)
        _check(self._lib.hyphy_hip_branch_trials_built(self._h, len(nd), _l(nd), _d(co), _d(w), _d(ll), _d(sl), _l(sc)))
        return (ll, sl, sc) if per_site else ll

    # -- every nearest-neighbour interchange's log-L from one outside pass ---------------------------
    def nni_scores(self, moves, weights=None, per_site: bool = False):
        """log-L [n] of the trees in which ``moves[t] = (x, y)`` exchange parents (c = parent(x) internal and not the root, y a sibling
        of c; ``plan_nni`` lists every such pair), every branch keeping its matrix and everything else as at the last evaluation of
        every class: one outside pass serves every move of the call.  ``weights``: class weights when C > 1.  ``per_site``: also the
        per-pattern values and 2^64 exponents, [n, S] each.  Nothing on the device changes."""
        mv = np.ascontiguousarray(moves, dtype=np.int64).reshape(-1, 2)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            assert w.shape == (self.C,)
        ll = np.zeros(len(mv))
        sl = np.zeros((len(mv), self.S)) if per_site else None
        sc = np.zeros((len(mv), self.S), dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_nni_scores(self._h, len(mv), _l(mv), _d(w), _d(ll), _d(sl), _l(sc)))
        return (ll, sl, sc) if per_site else ll

    # -- first and second log-L derivatives of any number of branches from one outside pass --------
    def _derivative_call(self, fn, nodes, mats, tail, weights, per_site):
        nd = np.ascontiguousarray(nodes, dtype=np.int64).reshape(-1)
        m = np.ascontiguousarray(mats, dtype=np.float64)
        if m.size != len(nd) * self.C * int(np.prod(tail)):
            raise ValueError(f"expected [{len(nd)}, {self.C}, {', '.join(str(x) for x in tail)}] values, got {m.shape}")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (self.C,):
                raise ValueError(f"expected {self.C} class weights, got {w.shape}")
        d1, d2 = np.zeros(len(nd)), np.zeros(len(nd))
        sk = np.zeros(len(nd), dtype=np.int64)
        s1 = np.zeros((len(nd), self.S)) if per_site else None
        s2 = np.zeros((len(nd), self.S)) if per_site else None
        _check(getattr(self._lib, fn)(self._h, len(nd), _l(nd), _d(m), _d(w), _d(d1), _d(d2), _l(sk), _d(s1), _d(s2)))
        return (d1, d2, sk, s1, s2) if per_site else (d1, d2, sk)

    def branch_derivatives(self, nodes, g_dense, weights=None, per_site: bool = False):
        """(d1, d2, skipped), [n] each: the first and second derivative at theta = 0 of log L under P_b(theta) = exp(theta G) P_b for
        branch ``nodes[t]`` and generator ``g_dense[t]`` ([n, D, D], or [n, C, D, D] with one generator per rate class), everything
        else as at the last evaluation of every class; ``skipped``: the patterns of positive frequency whose likelihood is exactly 0
        (they take no part).  With G = Q_b the derivatives in log t_b are d1 and d2 + d1.  ``per_site``: also the per-pattern r1 and
        r2, [n, S] each (NaN at skipped patterns).  Nothing on the device changes."""
        return self._derivative_call("hyphy_hip_branch_derivatives", nodes, g_dense, (self.D, self.D), weights, per_site)

    def branch_derivatives_built(self, nodes, coeffs, weights=None, per_site: bool = False):
        """``branch_derivatives`` with the generators formed on the device from coefficient rows over the templates of
        ``set_q_templates`` (``coeffs``: [n, K] or [n, C, K]), as ``build_q`` forms rate matrices."""
        K = int(np.asarray(coeffs).shape[-1])
        return self._derivative_call("hyphy_hip_branch_derivatives_built", nodes, coeffs, (K,), weights, per_site)

    # -- the gradient of log L in every matrix entry, rate-matrix entry and template coefficient ----
    def _gradient_call(self, fn, nodes, mats, tail, out_tail, weights):
        nd = np.ascontiguousarray(nodes, dtype=np.int64).reshape(-1)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (self.C,):
                raise ValueError(f"expected {self.C} class weights, got {w.shape}")
        out = np.zeros((len(nd), self.C) + tuple(out_tail))
        sk = np.zeros(len(nd), dtype=np.int64)
        if mats is None:
            _check(getattr(self._lib, fn)(self._h, len(nd), _l(nd), _d(w), _d(out), _l(sk)))
        else:
            m = np.ascontiguousarray(mats, dtype=np.float64)
            if m.size != len(nd) * self.C * int(np.prod(tail)):
                raise ValueError(f"expected [{len(nd)}, {self.C}, {', '.join(str(x) for x in tail)}] values, got {m.shape}")
            _check(getattr(self._lib, fn)(self._h, len(nd), _l(nd), _d(m), _d(w), _d(out), _l(sk)))
        return (out[:, 0] if self.C == 1 else out), sk

    def branch_sensitivities(self, nodes, weights=None):
        """(W, skipped): W[t] = d log L / d P of branch ``nodes[t]``, [n, D, D] (or [n, C, D, D]: class c's block is the derivative
        in class c's matrix and contains its weight), everything as at the last evaluation of every class; ``skipped``: the patterns
        of positive frequency whose likelihood is exactly 0.  Holds for any resident matrix.  Nothing on the device changes."""
        return self._gradient_call("hyphy_hip_branch_sensitivities", nodes, None, None, (self.D, self.D), weights)

    def branch_gradient(self, nodes, q_dense, weights=None):
        """(S, skipped): S[t] = d log L / d Q of branch ``nodes[t]`` where its resident matrix is exp(``q_dense[t]``) ([n, D, D] or
        [n, C, D, D]), the entries of Q taken as independent, the diagonal included.  For a mixture branch pass a component's rate
        matrix and multiply the result by that component's mixture weight."""
        return self._gradient_call("hyphy_hip_branch_gradient", nodes, q_dense, (self.D, self.D), (self.D, self.D), weights)

    def branch_gradient_built(self, nodes, coeffs, weights=None):
        """(grad, skipped): grad[t][k] = d log L / d ``coeffs[t][k]`` where the resident matrix of branch ``nodes[t]`` is the
        exponential of the rate matrix ``build_q`` forms from ``coeffs[t]`` ([n, K] or [n, C, K]) over the templates of
        ``set_q_templates``."""
        K = int(np.asarray(coeffs).shape[-1])
        return self._gradient_call("hyphy_hip_branch_gradient_built", nodes, coeffs, (K,), (K,), weights)

    # -- branch cache (one-branch line searches) --------------------------------------------------
    def branch_cache_build(self, node: int, cat: int = 0):
        """Prepare the device branch cache for branch ``node`` (call after an ``evaluate``)."""
        _check(self._lib.hyphy_hip_branch_cache_build(self._h, cat, int(node)))

    def branch_cache_evaluate(self, node: int, q_dense: np.ndarray, cat: int = 0, q_is_probability: bool = False,
                              per_site: bool = False):
        """log-L with branch ``node``'s matrix replaced by exp(q_dense); everything else as at build time."""
        q = np.ascontiguousarray(q_dense, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_branch_cache_evaluate(self._h, cat, int(node), _d(q), int(q_is_probability),
                                                         C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def prepare_branch_cache_step(self, node: int, q_dense: np.ndarray, cat: int = 0):
        """Zero-argument callable evaluating the cached branch with the CURRENT contents of ``q_dense``
        (update it in place between calls); arguments marshalled once."""
        assert q_dense.flags.c_contiguous and q_dense.dtype == np.float64
        lib, h, pq, out = self._lib, self._h, _d(q_dense), C.c_double(0.0)
        ref = C.byref(out)

        def step(_keep=q_dense):
            _check(lib.hyphy_hip_branch_cache_evaluate(h, cat, int(node), pq, 0, ref, None, None))
            return out.value
        return step

    # -- device-side Q construction -------------------------------------------------------------
    def evaluate_built(self, update_nodes, q_nodes, root_freqs, cat: int = -1, per_site: bool = False):
        """Synchronous evaluation over the rate matrices staged by ``build_q`` (one coefficient row per entry of q_nodes);
        ``per_site``: also the per-pattern values and 2^64 exponents (hyphy_hip_evaluate_built_sites)."""
        un = np.ascontiguousarray(update_nodes, dtype=np.int64)
        qn = np.ascontiguousarray(q_nodes, dtype=np.int64)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = C.c_double(0.0)
        sl = np.zeros(self.S) if per_site else None
        sc = np.zeros(self.S, dtype=np.int64) if per_site else None
        _check(self._lib.hyphy_hip_evaluate_built_sites(self._h, cat, _l(un), len(un), _l(qn), len(qn), _d(rf), C.byref(out), _d(sl), _l(sc)))
        return (out.value, sl, sc) if per_site else out.value

    def set_q_templates(self, templates: np.ndarray):
        t = np.ascontiguousarray(templates, dtype=np.float64)
        _check(self._lib.hyphy_hip_set_q_templates(self._h, t.shape[0], _d(t)))

    def update_q_templates(self, templates: np.ndarray):
        """New VALUES for the templates of ``set_q_templates`` ([K, D, D], C-contiguous float64): copied before the call returns,
        uploaded in-stream ahead of the next exponential launch; branches not rebuilt afterwards keep their matrices."""
        t = np.ascontiguousarray(templates, dtype=np.float64)
        if t.ndim != 3 or t.shape[1:] != (self.D, self.D):
            raise ValueError(f"expected [K, {self.D}, {self.D}] templates, got {t.shape}")
        _check(self._lib.hyphy_hip_update_q_templates(self._h, t.shape[0], _d(t)))

    def build_q(self, coeffs: np.ndarray):
        c = np.ascontiguousarray(coeffs, dtype=np.float64)
        _check(self._lib.hyphy_hip_build_q(self._h, c.shape[0], _d(c)))

    def site_fits_evaluate(self, branch_group, branch_coeffs, site_mult, root_freqs) -> np.ndarray:
        """Per-site batched fits: ``site_mult`` is [n_sets, S, n_groups, K] (or [S, n_groups, K]);
        returns the site log-likelihoods [n_sets, S] (or [S]) of every pattern under its own multipliers."""
        bg = np.ascontiguousarray(branch_group, dtype=np.int64)
        bc = np.ascontiguousarray(branch_coeffs, dtype=np.float64)
        sm = np.ascontiguousarray(site_mult, dtype=np.float64)
        single = sm.ndim == 3
        if single:
            sm = sm[None]
        n_sets, S, G, K = sm.shape
        assert S == self.S and bg.shape == (self.B,) and bc.shape == (self.B, K)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = np.zeros((n_sets, S))
        _check(self._lib.hyphy_hip_site_fits_evaluate(self._h, n_sets, G, _l(bg), _d(bc), _d(sm), _d(rf), _d(out)))
        return out[0] if single else out

    def site_fits_evaluate_mixture(self, branch_group, branch_coeffs, site_mult, site_weights, root_freqs) -> np.ndarray:
        """Branch-site mixture per site: ``site_mult`` [n_sets, S, n_mix, n_groups, K], ``site_weights`` [n_sets, S, n_mix]
        (or both without the leading n_sets axis); returns site log-likelihoods [n_sets, S] (or [S])."""
        bg = np.ascontiguousarray(branch_group, dtype=np.int64)
        bc = np.ascontiguousarray(branch_coeffs, dtype=np.float64)
        sm = np.ascontiguousarray(site_mult, dtype=np.float64)
        sw = np.ascontiguousarray(site_weights, dtype=np.float64)
        single = sm.ndim == 4
        if single:
            sm, sw = sm[None], sw[None]
        n_sets, S, M, G, K = sm.shape
        assert S == self.S and sw.shape == (n_sets, S, M) and bg.shape == (self.B,) and bc.shape == (self.B, K)
        rf = np.ascontiguousarray(root_freqs, dtype=np.float64)
        out = np.zeros((n_sets, S))
        _check(self._lib.hyphy_hip_site_fits_evaluate_mixture(self._h, n_sets, G, M, _l(bg), _d(bc), _d(sm), _d(sw), _d(rf), _d(out)))
        return out[0] if single else out

    def site_fits_kernel_ms(self) -> float:
        return float(self._lib.hyphy_hip_site_fits_kernel_ms(self._h))

    def q_buffer(self) -> int:
        return int(self._lib.hyphy_hip_q_buffer(self._h))

    def synchronize(self):
        _check(self._lib.hyphy_hip_synchronize(self._h))

    def stream(self) -> int:
        return int(self._lib.hyphy_hip_stream(self._h) or 0)

    def set_stream(self, stream_ptr: int):
        _check(self._lib.hyphy_hip_set_stream(self._h, C.c_void_p(stream_ptr)))

    def prune_timings(self, n: int) -> np.ndarray:
        """Durations (ms) of the pruning launches of the last ``n`` evaluations (HIP event ring; queried
        only now, never while evaluations run)."""
        out = np.zeros(int(n))
        m = int(self._lib.hyphy_hip_prune_timings(self._h, _d(out), int(n)))
        return out[:m]

    def prune_launches(self) -> int:
        return int(self._lib.hyphy_hip_prune_launches(self._h))

    def prune_kernel_name(self) -> str:
        return self._lib.hyphy_hip_prune_kernel_name(self._h).decode()

    def prune_form(self) -> str:
        """Form of the pruning launch of the last evaluation: kernel, row blocks, instantiation, cut (include/hyphy_hip.h)."""
        return self._lib.hyphy_hip_last_prune_form(self._h).decode()

    def reduce_form(self) -> str:
        """Which final combine produced the last evaluation's log-L, and over how many partials (include/hyphy_hip.h)."""
        return self._lib.hyphy_hip_last_reduce_form(self._h).decode()

    def schedule_info(self) -> str:
        return self._lib.hyphy_hip_schedule_info(self._h).decode()

    def set_repeats(self, on: bool):
        """Subtree repeats (class-compressed lower phase) on / off for this partition; same results either way."""
        _check(self._lib.hyphy_hip_set_repeats(self._h, 1 if on else 0))

    def repeat_stats(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        _check(self._lib.hyphy_hip_repeat_stats(self._h, _l(out)))
        keys = ("available", "tables", "table_rows", "trunk_internal", "trunk_leaves", "edge_products_on", "edge_products_off", "in_use")
        return {k: int(v) for k, v in zip(keys, out)}

    def set_all_timings(self, on: bool):
        """Also stamp the expm and reduction kernels of the evaluations that follow (``last_timings()[0]``, ``[2]``)."""
        _check(self._lib.hyphy_hip_set_timing_detail(self._h, 1 if on else 0))

    def last_timings(self) -> np.ndarray:
        out = np.zeros(3)
        _check(self._lib.hyphy_hip_last_timings(self._h, _d(out)))
        return out
