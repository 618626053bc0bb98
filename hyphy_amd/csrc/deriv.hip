// Every branch's first and second derivative of log L along a generator, from one outside pass.  With the outside vector V_c of
// branch c (outside.h), its conditional in_c and its resident matrix P_c, E = P_c in_c, the likelihood under P_c(theta) =
// exp(theta G) P_c is  l(theta) = sum_i V[i] (exp(theta G) E)[i]  per pattern, hence at theta = 0
//   l0 = V . E        l1 = V . (G E)        l2 = V . (G (G E)),      2^64 exponent of all three = exponent(V_c) + exponent(in_c),
//   d log l / d theta = l1 / l0,    d^2 log l / d theta^2 = l2 / l0 - (l1 / l0)^2.
// No exponential is computed and the exponents cancel inside each pattern's ratio.  Rate classes: (l0, l1, l2) are mixed by weight
// with their exponents aligned on the smallest, then the ratios are taken of the mixed (L0, L1, L2).
//
// Phase 1 (outside_store_kernel<NW>, outside_store_nuc_kernel of outside.h): the walk with the OutsideStore sink, as the branch
// trials run it.
// Generator images (deriv_image_kernel): the row-major G of every (derivative, class) as an A-operand image, zero-padded to DP
// (4 states: [16] row-major as given).
// Phase 2 (branch_derivs_kernel<NW>, branch_derivs_nuc_kernel): one wave per (branch with a derivative, tile), the tile the fastest
// grid index.  V and E (outside.h's edge_product over the resident images) are formed once; every generator of the branch is two
// [D x D] x [D x 16] products on the FP64 MFMA — the C/D fragment of G E is the B operand of G (G E) — and three row sums.  Classes
// run one launch after another; the last class's launch forms r1, r2 and one partial record per (derivative, tile).
// Reduction (derivs_reduce_kernel): one wave per derivative, combine.h's fixed-order compensated sum, once per total.
// Nothing joins by order of arrival: two identical calls give identical bits.  The refusals, the scratch of the walk, the loop over
// chunks of tiles and classes and KeepForms are outside_pass.h's, as for trials.hip and under the same budget (HYPHY_HIP_TRIALS_MB);
// the kernels get (WalkArgs, OutsideSlice, DerivArgs) and take the branch, V, E (4 states: mat4_vec), the exponent alignment and the
// wave sums of their records from outside.h; all scratch comes from the pool and goes back before the call returns.  The partition's
// matrices, images, schedules and caches are not written.
#include "combine.h"
#include "devutil.h"
#include "outside_pass.h"
#include "partition.h"

using namespace hyhip;

namespace hyhip {
namespace {

struct DerivArgs {             // the derivatives' own blocks, beside the WalkArgs and the OutsideSlice
  const double *img;           // [n][C] generators: A-operand images (4 states: [16] row-major)
  double *L0, *L1, *L2;        // [n][S_pad] per pattern: classes mixed so far; behind the last class L1 = r1, L2 = r2
  int32_t *cnt;                // their common exponent
  double *part_d1, *part_d2;   // [n][part_stride] per (derivative, tile): sum_s f_s r1, sum_s f_s r2
  long long *part_skip;        // patterns of positive frequency with L0 == 0
  int *part_flag;              // 2: not a number
};

// this class's (l0, l1, l2; exponent e) of pattern q into the mix of the classes before it, aligned on the smaller exponent as
// mix_in of trials.hip aligns likelihoods.  A triple of exact zeros (a weight of 0, an impossible pattern) carries no exponent: it
// leaves the others as they are, where aligning on its exponent could flush them to zero.
__device__ __forceinline__ void mix3(const OutsideSlice &sl, const DerivArgs &a, size_t q, double &l0, double &l1, double &l2, int &e) {
  l0 *= sl.w, l1 *= sl.w, l2 *= sl.w;
  if (sl.first) return;
  const double o0 = a.L0[q], o1 = a.L1[q], o2 = a.L2[q];
  const int e_old = a.cnt[q];
  if (l0 == 0. && l1 == 0. && l2 == 0.) {
    l0 = o0, l1 = o1, l2 = o2, e = e_old;
  } else if (!(o0 == 0. && o1 == 0. && o2 == 0.)) {
    double so, sn;
    e = align_exponents(e_old, e, so, sn);
    l0 = o0 * so + l0 * sn, l1 = o1 * so + l1 * sn, l2 = o2 * so + l2 * sn;
  }
}

// r1, r2 of the mixed (L0, L1, L2) and the pattern's terms of the totals
__device__ __forceinline__ void site_ratio(double l0, double l1, double l2, double f, double &r1, double &r2, double &s1, double &s2,
                                           long long &skip, int &flag) {
  if (l0 != l0 || l1 != l1 || l2 != l2) {
    r1 = r2 = NAN;
    if (f != 0.) flag |= 2;
  } else if (l0 == 0.) {
    r1 = r2 = NAN;
    if (f != 0.) skip += 1;
  } else {
    r1 = l1 / l0;
    r2 = l2 / l0 - r1 * r1;
    if (f != 0.) {
      if (r1 != r1 || r2 != r2) flag |= 2;
      s1 += f * r1;
      s2 += f * r2;
    }
  }
}

// the record of (derivative t, tile): the terms of its W lanes summed, written by lane 0
template <int W>
__device__ __forceinline__ void put_record(const OutsideSlice &sl, const DerivArgs &a, int t, int tile, int lane, double w1, double w2,
                                           long long wskip, int wflag) {
  w1 = wave_sum<W>(w1), w2 = wave_sum<W>(w2), wskip = wave_sum<W>(wskip), wflag = wave_or<W>(wflag);
  if (lane == 0) {
    const size_t pq = (size_t)t * sl.part_stride + tile;
    a.part_d1[pq] = w1;
    a.part_d2[pq] = w2;
    a.part_skip[pq] = wskip;
    a.part_flag[pq] = wflag;
  }
}

__global__ __launch_bounds__(256) void deriv_image_kernel(const double *__restrict__ G, double *__restrict__ img, int D, int NW, int nuc) {
  const double *src = G + (size_t)blockIdx.x * D * D;
  if (nuc) {
    if (threadIdx.x < 16) img[(size_t)blockIdx.x * 16 + threadIdx.x] = src[threadIdx.x];
    return;
  }
  const int DP = 16 * NW;
  double *dst = img + (size_t)blockIdx.x * DP * DP;
  for (int idx = threadIdx.x; idx < DP * DP; idx += blockDim.x) {
    int r, c;
    frag_image_rc(idx, NW, r, c);
    dst[idx] = r < D && c < D ? src[r * D + c] : 0.;
  }
}

template <int NW>
__global__ __launch_bounds__(64) void branch_derivs_kernel(WalkArgs wa, OutsideSlice sl, DerivArgs a) {
  constexpr int NKK = 4 * NW, DP = 16 * NW;
  const int lane = threadIdx.x, g = lane >> 4;
  const int tile = sl.tile0 + blockIdx.x, site = tile * 16 + (lane & 15);
  const int bi = sl.b0 + blockIdx.y;
  double V[NKK], E[NKK];
  int bcnt, ecnt;
  const int4 ce = branch_outside<NKK>(wa, sl, bi, tile, lane, V, bcnt);
  edge_product<NW>(wa, ce, tile, lane, E, ecnt);
  bcnt += ecnt;
  double s0 = 0.;
#pragma unroll
  for (int kk = 0; kk < NKK; kk++) s0 += V[kk] * E[kk];
  s0 = row_sum4(s0);
  const double f = sl.freq[site];
  for (int k = sl.off[bi]; k < sl.off[bi + 1]; k++) {
    const int t = sl.idx[k];
    const double *G = a.img + ((size_t)t * sl.C + sl.cls) * DP * DP;
    double X[NKK];
    mfma_product<NW>(G, E, lane, X);
    double s1 = 0., s2 = 0.;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) s1 += V[kk] * X[kk];
    __builtin_amdgcn_sched_barrier(0);  // (the second product's operand loads stay behind the first product: registers)
    {
      double Y[NKK];
      mfma_product<NW>(G, X, lane, Y);
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) s2 += V[kk] * Y[kk];
    }
    s1 = row_sum4(s1);
    s2 = row_sum4(s2);
    double w1 = 0., w2 = 0.;
    long long wskip = 0;
    int wflag = 0;
    if (g == 0) {
      const size_t q = (size_t)t * wa.S_pad + site;
      double l0 = s0;
      int e = bcnt;
      mix3(sl, a, q, l0, s1, s2, e);
      if (sl.last) {
        double r1, r2;
        site_ratio(l0, s1, s2, f, r1, r2, w1, w2, wskip, wflag);
        s1 = r1, s2 = r2;
      }
      a.L0[q] = l0;
      a.L1[q] = s1;
      a.L2[q] = s2;
      a.cnt[q] = e;
    }
    if (sl.last) put_record<16>(sl, a, t, tile, lane, w1, w2, wskip, wflag);
  }
}

// 4 states: one thread per pattern, one wave per (branch, 64 patterns)
__global__ __launch_bounds__(64) void branch_derivs_nuc_kernel(WalkArgs wa, OutsideSlice sl, DerivArgs a) {
  const int lane = threadIdx.x, tile = sl.tile0 + blockIdx.x;
  const size_t s = (size_t)tile * 64 + lane;
  const int bi = sl.b0 + blockIdx.y;
  double V[4], in[4], E[4];
  int bcnt, ecnt;
  const int4 ce = nuc_branch_outside(wa, sl, bi, tile, lane, V, bcnt);
  nuc_child_vec(wa, ce, s, in, ecnt);
  bcnt += ecnt;
  mat4_vec(wa.Prow + (size_t)ce.y * 16, in, E);
  const double s0 = dot4(V, E);
  const double f = sl.freq[s];
  for (int k = sl.off[bi]; k < sl.off[bi + 1]; k++) {
    const int t = sl.idx[k];
    const double *G = a.img + ((size_t)t * sl.C + sl.cls) * 16;
    double X[4], Y[4];
    mat4_vec(G, E, X);
    mat4_vec(G, X, Y);
    double l0 = s0, l1 = dot4(V, X), l2 = dot4(V, Y);
    const size_t q = (size_t)t * wa.S_pad + s;
    int e = bcnt;
    mix3(sl, a, q, l0, l1, l2, e);
    double w1 = 0., w2 = 0.;
    long long wskip = 0;
    int wflag = 0;
    if (sl.last) {
      double r1, r2;
      site_ratio(l0, l1, l2, f, r1, r2, w1, w2, wskip, wflag);
      l1 = r1, l2 = r2;
    }
    a.L0[q] = l0;
    a.L1[q] = l1;
    a.L2[q] = l2;
    a.cnt[q] = e;
    if (sl.last) put_record<64>(sl, a, t, tile, lane, w1, w2, wskip, wflag);
  }
}

// totals of derivative blockIdx.x from its per-tile records: one wave, fixed order, compensated; out = [n] d1, [n] d2, [n] skipped
__global__ __launch_bounds__(64) void derivs_reduce_kernel(double *part_d1, double *part_d2, long long *part_skip, int *part_flag, int n,
                                                           int stride, double *__restrict__ out, long long *__restrict__ skip_out) {
  const size_t o = (size_t)blockIdx.x * stride;
  double s1, c1, s2, c2;
  long long k1, k2;
  int f1, f2;
  combine_range(part_d1 + o, part_skip + o, part_flag + o, n, 0, n, (int)threadIdx.x, s1, c1, k1, f1);
  combine_range(part_d2 + o, part_skip + o, part_flag + o, n, 0, n, (int)threadIdx.x, s2, c2, k2, f2);
  if (threadIdx.x == 0) {
    const bool bad = ((f1 | f2) & 2) != 0;
    out[blockIdx.x] = bad ? NAN : s1 - c1;
    out[gridDim.x + blockIdx.x] = bad ? NAN : s2 - c2;
    skip_out[blockIdx.x] = k1;
  }
}

int derivs_common(const char *what, hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *g_dense, const double *coeffs,
                  const double *weights, double *d1_out, double *d2_out, int64_t *skipped_out, double *site_d1_out,
                  double *site_d2_out) {
  const std::string pre = std::string(what) + ": ";
  if (!p) return fail(pre + "partition == NULL");
  if (n < 0) return fail(pre + "n < 0");
  if (check_pass_ready(p, pre, weights)) return -1;
  if (n == 0) return 0;
  if (!nodes || !d1_out || !d2_out || (!g_dense && !coeffs)) return fail(pre + "null argument");
  if (check_requests(p, pre, "derivative", n, nodes, coeffs != nullptr)) return -1;
  const KeepForms keep = {p, p->last_reduce, last_expm_kernel()};
  OutsideCall oc;
  if (begin_outside(p, oc, nodes, n)) return -1;
  const int C = (int)p->C, NW = p->NW;
  const int64_t D = p->D;
  const bool nuc = p->nuc;
  const size_t MS = nuc ? 16 : (size_t)p->DP * p->DP;  // doubles of a generator on the device
  std::vector<double> totals((size_t)2 * n);
  std::vector<long long> h_skip((size_t)n);
  std::vector<std::vector<double>> parts1((size_t)n), parts2((size_t)n);
  std::vector<int64_t> skipped((size_t)n, 0);
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    Blocks blk;
    OutsideScratch sc;
    sc.plan(p, s, oc);
    const size_t nm = (size_t)n * C, nq = g_dense ? nm * D * D : nm * p->K, np = (size_t)n * sc.part_stride;
    double *img = nullptr, *src = nullptr, *gq = nullptr, *L0 = nullptr, *L1 = nullptr, *L2 = nullptr, *part_d1 = nullptr, *part_d2 = nullptr;
    double *d_tot = nullptr;
    int32_t *cnt = nullptr;
    long long *part_skip = nullptr, *d_skip = nullptr;
    int *part_flag = nullptr;
    HIPCHK(blk.get(&img, nm * MS));
    HIPCHK(blk.get(&src, nq));
    if (coeffs) HIPCHK(blk.get(&gq, nm * D * D));
    HIPCHK(blk.get(&L0, (size_t)n * s.S_pad));
    HIPCHK(blk.get(&L1, (size_t)n * s.S_pad));
    HIPCHK(blk.get(&L2, (size_t)n * s.S_pad));
    HIPCHK(blk.get(&cnt, (size_t)n * s.S_pad));
    HIPCHK(blk.get(&part_d1, np));
    HIPCHK(blk.get(&part_d2, np));
    HIPCHK(blk.get(&part_skip, np));
    HIPCHK(blk.get(&part_flag, np));
    HIPCHK(blk.get(&d_tot, (size_t)2 * n));
    HIPCHK(blk.get(&d_skip, (size_t)n));
    if (sc.get(p, oc, blk)) return -1;
    HIPCHK(hipMemcpyAsync(src, g_dense ? g_dense : coeffs, nq * sizeof(double), hipMemcpyHostToDevice, s.stream));
    if (sc.upload(p, oc, s.stream)) return -1;
    // generators: built from the templates into the call's own scratch (never the partition's Q buffer), then their images
    if (coeffs) launch_build_q(s.templates, src, (int)nm, (int)p->K, (int)D, gq, s.stream);
    hipLaunchKernelGGL(deriv_image_kernel, dim3((unsigned)nm), dim3(256), 0, s.stream, coeffs ? gq : src, img, (int)D, NW, nuc ? 1 : 0);
    HIPCHK(hipGetLastError());
    const DerivArgs da = {img, L0, L1, L2, cnt, part_d1, part_d2, part_skip, part_flag};
    const int walked = outside_chunks(p, s, oc, sc, weights, [&](const WalkArgs &a, const OutsideSlice &sl, dim3 grid) {
      if (nuc) hipLaunchKernelGGL(branch_derivs_nuc_kernel, grid, dim3(64), 0, s.stream, a, sl, da);
      else LAUNCH_NW(branch_derivs_kernel, NW, grid, dim3(64), s.stream, a, sl, da);
    });
    if (walked) return -1;
    hipLaunchKernelGGL(derivs_reduce_kernel, dim3((unsigned)n), dim3(64), 0, s.stream, part_d1, part_d2, part_skip, part_flag, sc.ntiles,
                       sc.part_stride, d_tot, d_skip);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(totals.data(), d_tot, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(h_skip.data(), d_skip, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    for (int64_t t = 0; t < n; t++) {
      parts1[(size_t)t].push_back(totals[(size_t)t]);
      parts2[(size_t)t].push_back(totals[(size_t)(n + t)]);
      skipped[(size_t)t] += (int64_t)h_skip[(size_t)t];
    }
    if (site_d1_out && download_rows(p, s, L1, n, site_d1_out)) return -1;
    if (site_d2_out && download_rows(p, s, L2, n, site_d2_out)) return -1;
  }
  for (int64_t t = 0; t < n; t++) {
    d1_out[t] = combine(parts1[(size_t)t]);
    d2_out[t] = combine(parts2[(size_t)t]);
    if (skipped_out) skipped_out[t] = skipped[(size_t)t];
  }
  return 0;
}

}  // namespace
}  // namespace hyhip

extern "C" {

int hyphy_hip_branch_derivatives(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *g_dense, const double *weights,
                                 double *d1_out, double *d2_out, int64_t *skipped_out, double *site_d1_out, double *site_d2_out) {
  if (p && n > 0 && !g_dense) return fail("branch_derivatives: null generator pointer");
  return derivs_common("branch_derivatives", p, n, nodes, g_dense, nullptr, weights, d1_out, d2_out, skipped_out, site_d1_out,
                       site_d2_out);
}

int hyphy_hip_branch_derivatives_built(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *coeffs,
                                       const double *weights, double *d1_out, double *d2_out, int64_t *skipped_out, double *site_d1_out,
                                       double *site_d2_out) {
  if (p && n > 0 && !coeffs) return fail("branch_derivatives_built: null coefficient pointer");
  return derivs_common("branch_derivatives_built", p, n, nodes, nullptr, coeffs, weights, d1_out, d2_out, skipped_out, site_d1_out,
                       site_d2_out);
}

}  // extern "C"
