// The host side of the passes that keep every branch's outside vector (trials.hip, nni.hip, deriv.hip, grad.hip), once: behind outside.h's
// check_pass_ready, what they refuse of their requests, then the per-shard scratch and the loop over chunks of tiles and rate classes.
//   check_requests                      the refusals, in the order and with the words the entry points have always had
//   begin_outside                       outside.h's (pending work finished, classes resident, program, pi), and the requests grouped
//   OutsideScratch                      one shard's walk blocks and branch tables, from the call's Blocks
//   outside_chunks                      per (chunk, class): WalkArgs, transposition, phase 1, then the caller's phase 2 per grid slice,
//                                       which gets the WalkArgs and the filled OutsideSlice (outside.h) to pass on to its kernel as they are
//   download_rows                       [n][S_pad] on the device -> the caller's pattern order
//   KeepForms                           the last reduce form and exponential kernel put back when the call returns (deriv.hip, grad.hip)
// Tiles are independent in both phases, so phases 1-2 run over chunks of tiles that keep the V scratch ([B][tiles of the chunk][TILE]
// doubles) within HYPHY_HIP_TRIALS_MB (default 1024, read at every call, never less than one tile).  4 states: a "tile" of the
// chunking is one wave's 64 patterns.  (The marginal reconstruction needs none of this: its chunk is the whole shard and its scratch
// stays with the shard.  It must not include this file: launch_outside_store would put phase 1's kernels into its code object.)
#pragma once
#include "outside.h"
#include "outside_plan.h"
#include "partition.h"

namespace hyhip {
namespace {

// n > 0 requests of one kind (`noun`: "trial", "derivative", "request"), each naming a branch
inline int check_requests(const hyphy_hip_partition *p, const std::string &pre, const char *noun, int64_t n, const int64_t *nodes,
                          bool from_templates) {
  if (from_templates && !p->K) return fail(pre + "templates not set (hyphy_hip_set_q_templates)");
  if (n * p->C > 0x3fffffff) return fail(pre + "too many " + noun + "s");
  for (int64_t t = 0; t < n; t++)
    if (nodes[t] < 0 || nodes[t] >= p->B)
      return fail(pre + noun + " " + std::to_string(t) + ": node code out of range (the root has no branch)");
  return 0;
}

struct OutsideCall {       // what every shard of one call reads
  std::vector<double> pi;  // the root frequencies, padded
  BranchGroups groups;     // the requests by branch
  double budget = 0.;      // bytes for the V scratch
};

inline int begin_outside(hyphy_hip_partition *p, OutsideCall &oc, const int64_t *nodes, int64_t n) {
  if (begin_outside(p, oc.pi)) return -1;
  oc.groups = group_by_branch(nodes, n);
  oc.budget = sw::scratch_budget(sw::TRIALS_MB);
  return 0;
}

// hyphy_hip_last_reduce_form and hyphy_hip_last_expm_kernel answer behind the call what they answered before it
struct KeepForms {
  hyphy_hip_partition *p;
  hyphy_hip_partition::ReduceForm reduce;
  const char *expm;
  ~KeepForms() {
    p->last_reduce = reduce;
    set_last_expm_kernel(expm);
  }
};

struct OutsideScratch {  // one shard
  int ntiles = 0, ct = 0, part_stride = 0;
  size_t TILE = 0;       // doubles of one tile of one node
  int TP = 0;            // its patterns
  double *PT = nullptr, *V = nullptr, *U = nullptr, *work = nullptr, *d_pi = nullptr;
  int32_t *Vcnt = nullptr, *Ucnt = nullptr, *wcnt = nullptr;
  int4 *d_prog = nullptr;
  int *d_branch = nullptr, *d_off = nullptr, *d_idx = nullptr;

  void plan(const hyphy_hip_partition *p, const Shard &s, const OutsideCall &oc) {
    TILE = p->nuc ? 256 : (size_t)16 * p->DP;
    TP = p->nuc ? 64 : 16;
    ntiles = s.S_pad / TP;
    ct = chunk_tiles(oc.budget, p->B, TILE * sizeof(double), ntiles);
    part_stride = hyhip::part_stride(ntiles);
  }
  int get(const hyphy_hip_partition *p, const OutsideCall &oc, Blocks &blk) {
    const size_t B = (size_t)p->B, I = (size_t)p->I, maxk = (size_t)p->marg_maxk;
    HIPCHK(blk.get(&d_pi, oc.pi.size()));
    HIPCHK(blk.get(&d_prog, p->marg_prog.size()));
    HIPCHK(blk.get(&d_branch, oc.groups.branch.size()));
    HIPCHK(blk.get(&d_off, oc.groups.off.size()));
    HIPCHK(blk.get(&d_idx, oc.groups.order.size()));
    if (!p->nuc) HIPCHK(blk.get(&PT, B * p->DP * p->DP));
    HIPCHK(blk.get(&V, B * ct * TILE));
    HIPCHK(blk.get(&Vcnt, B * ct * TP));
    HIPCHK(blk.get(&U, I * ct * TILE));
    HIPCHK(blk.get(&Ucnt, I * ct * TP));
    HIPCHK(blk.get(&work, (size_t)ct * 2 * maxk * TILE));
    HIPCHK(blk.get(&wcnt, (size_t)ct * 2 * maxk * TP));
    return 0;
  }
  int upload(const hyphy_hip_partition *p, const OutsideCall &oc, hipStream_t stream) {
    const BranchGroups &g = oc.groups;
    HIPCHK(hipMemcpyAsync(d_pi, oc.pi.data(), oc.pi.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_prog, p->marg_prog.data(), p->marg_prog.size() * sizeof(int4), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_branch, g.branch.data(), g.branch.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_off, g.off.data(), g.off.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_idx, g.order.data(), g.order.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    return 0;
  }
};

// phase 1 over the tiles [a.first, a.first + a.count) of a's class, behind the transposition of that class's images into PT (nullptr: PT holds them)
inline void launch_outside_store(const hyphy_hip_partition *p, const Shard &s, const WalkArgs &a, const OutsideStore &o, double *PT) {
  if (p->nuc) {
    hipLaunchKernelGGL(outside_store_nuc_kernel, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, s.stream, a, o);
    return;
  }
  if (PT)
    hipLaunchKernelGGL(marg_transpose_kernel, dim3((unsigned)p->B), dim3(256), 0, s.stream, a.Pfrag, a.PTg, PT, p->NW, (int)p->L);
  LAUNCH_NW(outside_store_kernel, p->NW, dim3((unsigned)a.count), dim3(64), s.stream, a, o);
}

// Chunk after chunk, class after class: phase 1 into V / Vcnt, then phase2(walk args, slice, grid) once per slice of the branch grid.
// The transposed images PT belong to a class: with several classes they are rebuilt for every class of every chunk, with one class once.
template <typename Phase2>
inline int outside_chunks(const hyphy_hip_partition *p, const Shard &s, const OutsideCall &oc, const OutsideScratch &sc,
                          const double *weights, Phase2 phase2) {
  const int C = (int)p->C, n_branch = (int)oc.groups.branch.size();
  for (int tile0 = 0; tile0 < sc.ntiles; tile0 += sc.ct) {
    const int nt = std::min(sc.ct, sc.ntiles - tile0);
    for (int c = 0; c < C; c++) {
      WalkArgs a = walk_args(p, s, c, {sc.d_prog, sc.d_pi, sc.PT, sc.U, sc.Ucnt, sc.work, sc.wcnt});
      const int unit = p->nuc ? sc.TP : 1;  // (4 states: the walk counts patterns)
      a.first = tile0 * unit, a.count = nt * unit, a.chunk = sc.ct * unit;
      launch_outside_store(p, s, a, {sc.V, sc.Vcnt}, C > 1 || tile0 == 0 ? sc.PT : nullptr);
      OutsideSlice sl = {tile0, sc.ct, nt, C, c, c == 0, c == C - 1, 0, C > 1 ? weights[c] : 1.0, sc.d_branch, sc.d_off, sc.d_idx,
                         sc.V, sc.Vcnt, s.freq, sc.part_stride};
      for (; sl.b0 < n_branch; sl.b0 += 65535) phase2(a, sl, dim3((unsigned)nt, (unsigned)std::min(65535, n_branch - sl.b0)));
      HIPCHK(hipGetLastError());
    }
  }
  return 0;
}

// rows [n][S_pad] of a shard's per-pattern result -> out[request][caller pattern]
template <typename T, typename O>
inline int download_rows(const hyphy_hip_partition *p, const Shard &s, const T *rows, int64_t n, O *out) {
  std::vector<T> h((size_t)n * s.S_pad);
  HIPCHK(hipMemcpy(h.data(), rows, h.size() * sizeof(T), hipMemcpyDeviceToHost));
  rows_to_caller(p, s, h.data(), (size_t)s.S_pad, n, s.S, out);
  return 0;
}

}  // namespace
}  // namespace hyhip
