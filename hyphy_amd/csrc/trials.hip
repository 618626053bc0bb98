// Every branch's trial likelihoods from one outside pass — the device counterpart of the finite-difference gradient of
// _LikelihoodFunction::ComputeGradient (likefunc.cpp:7025-7109), which re-evaluates the partition once per independent parameter.
// A parameter local to one branch changes that branch's transition matrix only, and with the branch's outside vector in hand
//   V_c = U_p * prod_{s in children(p), s != c} E_s        (U_root = pi, U_c = P_c^T V_c: the walk of outside.h)
// the likelihood under ANY replacement M of the matrix of branch c is one contraction per pattern,
//   L_s(P_c -> M) = sum_i V_c[i] (M in_c)[i],    2^64 exponent = exponent(V_c) + exponent(in_c),
// in_c the stored conditional of an internal child, the state indicator / ambiguity vector of a leaf.
//
// Phase 1 (outside_store_kernel<NW>, outside_store_nuc_kernel): outside.h's walk — the one the marginal reconstruction runs, over
// the same program (plan_marginal_program), one wave per 16-pattern tile — with the OutsideStore sink: it keeps V_c and its exponent
// of EVERY child, leaves included, forms no U for a leaf and accumulates no support.
// Phase 2 (branch_trials_kernel<NW>, branch_trials_nuc_kernel): one wave per (branch with at least one trial, tile), the tile the
// fastest grid index — the workgroups that run together read the same trial images.  V_c and in_c are loaded once; every trial of
// the branch is one [D x D] x [D x 16] product on the FP64 MFMA and a weighted row sum.  Classes run one launch after another and
// are mixed by weight with their exponents aligned; the last class's launch leaves one partial sum per (trial, tile).
// Reduction (trials_reduce_kernel): one wave per trial, combine.h's fixed-order compensated sum over the partial sums.
// Nothing here joins by order of arrival: two identical calls give identical bits.
//
// The refusals, the scratch of the walk and the loop over chunks of tiles and classes are outside_pass.h's, shared with deriv.hip and
// grad.hip; a phase-2 kernel gets (WalkArgs, OutsideSlice, TrialArgs) and starts from outside.h's branch prologue (branch_outside,
// child_vec and their 4-state forms), mixes through align_exponents and ends in wave_sum / wave_or.  The per-pattern mix, the records
// and the reduction are site_mix.h's, shared with nni.hip.  What is here is the trials' own: the trial images (and the column gather
// from them) and phase 2.  All scratch comes from the pool
// and goes back before the call returns.  The partition's matrices, images, schedules and caches are not written.
// 4 states: one thread per pattern over the plane layout and row-major matrices.
#include "combine.h"
#include "devutil.h"
#include "outside_pass.h"
#include "partition.h"
#include "site_mix.h"

using namespace hyhip;

namespace hyhip {
namespace {

template <int NW>
__global__ __launch_bounds__(64) void branch_trials_kernel(WalkArgs wa, OutsideSlice sl, TrialArgs a) {
  constexpr int NKK = 4 * NW, DP = 16 * NW, TILE = NKK * 64;
  const int lane = threadIdx.x, g = lane >> 4;
  const int tile = sl.tile0 + blockIdx.x, site = tile * 16 + (lane & 15);
  const int bi = sl.b0 + blockIdx.y;
  double V[NKK], in[NKK];
  int bcnt, ecnt;
  const int4 ce = branch_outside<NKK>(wa, sl, bi, tile, lane, V, bcnt);
  const int c = child_vec<NKK>(wa, ce, tile, lane, in, ecnt);
  bcnt += ecnt;
  const bool gather = ce.z < 0 && !__any(c < 0);
  const double f = sl.freq[site];
  for (int k = sl.off[bi]; k < sl.off[bi + 1]; k++) {
    const int t = sl.idx[k];
    const double *M = a.img + ((size_t)t * sl.C + sl.cls) * DP * DP;
    double E[NKK];
    if (gather) {  // column M[.][code] out of the A-operand image: M[r][c] sits in row block r >> 4 at k-step c >> 2, lane (c & 3) * 16 + (r & 15)
#pragma unroll
      for (int w = 0; w < NW; w++)
#pragma unroll
        for (int r = 0; r < 4; r++) E[4 * w + r] = M[w * TILE + frag_index(c >> 2, (c & 3) * 16 + 4 * r + g)];
    } else {
      mfma_product<NW>(M, in, lane, E);
    }
    double s = 0.;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) s += V[kk] * E[kk];
    s = row_sum4(s);
    double wsum = 0.;
    long long wcnt = 0;
    int wflag = 0;
    if (g == 0) {
      const size_t q = (size_t)t * wa.S_pad + site;
      int e = bcnt;
      mix_in(sl, a, q, s, e);
      a.lik[q] = s;
      a.cnt[q] = e;
      if (sl.last) site_term(s, e, f, wsum, wcnt, wflag);
    }
    if (sl.last) put_record<16>(sl, a, t, tile, lane, wsum, wcnt, wflag);
  }
}

// 4 states: one thread per pattern, one wave per (branch, 64 patterns)
__global__ __launch_bounds__(64) void branch_trials_nuc_kernel(WalkArgs wa, OutsideSlice sl, TrialArgs a) {
  const int lane = threadIdx.x, tile = sl.tile0 + blockIdx.x;
  const size_t s = (size_t)tile * 64 + lane;
  const int bi = sl.b0 + blockIdx.y;
  double V[4], in[4];
  int bcnt, ecnt;
  const int4 ce = nuc_branch_outside(wa, sl, bi, tile, lane, V, bcnt);
  nuc_child_vec(wa, ce, s, in, ecnt);
  bcnt += ecnt;
  const double f = sl.freq[s];
  for (int k = sl.off[bi]; k < sl.off[bi + 1]; k++) {
    const int t = sl.idx[k];
    double E[4], l = 0.;
    mat4_vec(a.img + ((size_t)t * sl.C + sl.cls) * 16, in, E);
    for (int x = 0; x < 4; x++) l += V[x] * E[x];
    const size_t q = (size_t)t * wa.S_pad + s;
    int e = bcnt;
    mix_in(sl, a, q, l, e);
    a.lik[q] = l;
    a.cnt[q] = e;
    if (sl.last) {
      double wsum = 0.;
      long long wcnt = 0;
      int wflag = 0;
      site_term(l, e, f, wsum, wcnt, wflag);
      put_record<64>(sl, a, t, tile, lane, wsum, wcnt, wflag);
    }
  }
}

int trials_common(const char *what, hyphy_hip_partition *p, int64_t n_trials, const int64_t *nodes, const double *q_dense,
                  const double *coeffs, int q_is_probability, const double *weights, double *logl_out, double *site_lik_out,
                  int64_t *site_scaler_out) {
  const std::string pre = std::string(what) + ": ";
  if (!p) return fail(pre + "partition == NULL");
  if (n_trials < 0) return fail(pre + "n_trials < 0");
  if (check_pass_ready(p, pre, weights)) return -1;
  if (n_trials == 0) return 0;
  if (!nodes || !logl_out || (!q_dense && !coeffs)) return fail(pre + "null argument");
  if (check_requests(p, pre, "trial", n_trials, nodes, coeffs != nullptr)) return -1;
  OutsideCall oc;
  if (begin_outside(p, oc, nodes, n_trials)) return -1;
  const int C = (int)p->C, NW = p->NW;
  const int64_t D = p->D;
  const bool nuc = p->nuc;
  const size_t MS = nuc ? 16 : (size_t)p->DP * p->DP;  // doubles of a trial matrix on the device
  std::vector<double> totals((size_t)n_trials);
  std::vector<std::vector<double>> parts((size_t)n_trials);
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    Blocks blk;
    OutsideScratch sc;
    sc.plan(p, s, oc);
    const size_t nm = (size_t)n_trials * C, nq = q_dense ? nm * D * D : nm * p->K, np = (size_t)n_trials * sc.part_stride;
    double *img = nullptr, *src = nullptr, *lik = nullptr, *part_sum = nullptr, *d_tot = nullptr;
    int32_t *cnt = nullptr, *status = nullptr;
    long long *part_cnt = nullptr;
    int *part_flag = nullptr;
    HIPCHK(blk.get(&img, nm * MS));
    HIPCHK(blk.get(&src, nq));
    HIPCHK(blk.get(&lik, (size_t)n_trials * s.S_pad));
    HIPCHK(blk.get(&cnt, (size_t)n_trials * s.S_pad));
    HIPCHK(blk.get(&part_sum, np));
    HIPCHK(blk.get(&part_cnt, np));
    HIPCHK(blk.get(&part_flag, np));
    HIPCHK(blk.get(&d_tot, (size_t)n_trials));
    HIPCHK(blk.get(&status, 1));
    if (sc.get(p, oc, blk)) return -1;
    HIPCHK(hipMemsetAsync(status, 0, sizeof(int32_t), s.stream));
    HIPCHK(hipMemcpyAsync(src, q_dense ? q_dense : coeffs, nq * sizeof(double), hipMemcpyHostToDevice, s.stream));
    if (sc.upload(p, oc, s.stream)) return -1;
    // trial images: one launch of the exponential kernels into the call's own slots (slot = trial * C + class)
    ExpmArgs ea;
    ea.n = (int)nm, ea.D = (int)D, ea.status = status;
    if (nuc) ea.Prow = img;
    else ea.Pfrag = img;
    if (q_dense) ea.Q = src, ea.is_prob = q_is_probability;
    if (coeffs) ea.templates = s.templates, ea.templates_pad = s.templates_pad, ea.coeffs = src, ea.K = (int)p->K;
    const char *expm_before = last_expm_kernel();
    launch_expm(ea, s.stream);
    set_last_expm_kernel(expm_before);
    HIPCHK(hipGetLastError());
    const TrialArgs ta = {img, lik, cnt, part_sum, part_cnt, part_flag};
    const int walked = outside_chunks(p, s, oc, sc, weights, [&](const WalkArgs &a, const OutsideSlice &sl, dim3 grid) {
      if (nuc) hipLaunchKernelGGL(branch_trials_nuc_kernel, grid, dim3(64), 0, s.stream, a, sl, ta);
      else LAUNCH_NW(branch_trials_kernel, NW, grid, dim3(64), s.stream, a, sl, ta);
    });
    if (walked) return -1;
    hipLaunchKernelGGL(trials_reduce_kernel, dim3((unsigned)n_trials), dim3(64), 0, s.stream, part_sum, part_cnt, part_flag, sc.ntiles,
                       sc.part_stride, d_tot);
    if (&s == &p->shards[0]) p->last_reduce = {"wave", sc.ntiles, false};  // (one wave per trial over its own partials)
    HIPCHK(hipGetLastError());
    int32_t h_status = 0;
    HIPCHK(hipMemcpyAsync(totals.data(), d_tot, (size_t)n_trials * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(&h_status, status, sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (h_status)
      return fail(pre + "Failed to compute a valid transition matrix; this is usually caused by ill-conditioned rate matrices "
                        "(e.g. very large rate values)");
    for (int64_t t = 0; t < n_trials; t++) parts[(size_t)t].push_back(totals[(size_t)t]);
    if (site_lik_out && download_rows(p, s, lik, n_trials, site_lik_out)) return -1;
    if (site_scaler_out && download_rows(p, s, cnt, n_trials, site_scaler_out)) return -1;
  }
  for (int64_t t = 0; t < n_trials; t++) logl_out[t] = combine(parts[(size_t)t]);
  return 0;
}

}  // namespace
}  // namespace hyhip

extern "C" {

int hyphy_hip_branch_trials(hyphy_hip_partition *p, int64_t n_trials, const int64_t *nodes, const double *q_dense,
                            int q_is_probability, const double *weights, double *logl_out, double *site_lik_out,
                            int64_t *site_scaler_out) {
  if (p && n_trials > 0 && !q_dense) return fail("branch_trials: null matrix pointer");
  return trials_common("branch_trials", p, n_trials, nodes, q_dense, nullptr, q_is_probability, weights, logl_out, site_lik_out,
                       site_scaler_out);
}

int hyphy_hip_branch_trials_built(hyphy_hip_partition *p, int64_t n_trials, const int64_t *nodes, const double *coeffs,
                                  const double *weights, double *logl_out, double *site_lik_out, int64_t *site_scaler_out) {
  if (p && n_trials > 0 && !coeffs) return fail("branch_trials_built: null coefficient pointer");
  return trials_common("branch_trials_built", p, n_trials, nodes, nullptr, coeffs, 0, weights, logl_out, site_lik_out,
                       site_scaler_out);
}

}  // extern "C"
