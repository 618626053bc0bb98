// The gradient of log L in every entry of every branch's transition matrix, rate matrix and template coefficient, from one outside pass.
// With V_b the outside vector of branch b (outside.h), in_b the conditional below it and L_s the pattern's likelihood, per class c
//   W_b[i][j] = d log L / d P_b[i][j] = sum_s f_s w_c V_{b,s}[i] in_{b,s}[j] / L_s                          (all terms >= 0)
//   S_b       = d log L / d Q_b       = L(Q_b^T, W_b),   L(A, E) = int_0^1 e^{sA} E e^{(1-s)A} ds           (P_b = exp(Q_b))
//   d log L / d x_bk                  = sum_{i != j} T_k[i][j] (S_b[i][j] - S_b[i][i])                      (Q_b = sum_k x_bk T_k)
// Phase 1 (outside_store_kernel<NW>, outside_store_nuc_kernel of outside.h): the walk with the OutsideStore sink, as the branch trials
// and the branch derivatives run it, under the same chunks of tiles and the same budget (outside_pass.h).  Like theirs, the kernels
// below get (WalkArgs, OutsideSlice, GradArgs) and take the branch, its V, the conditional below it and the exponent alignment from
// outside.h's phase-2 helpers (grad_accum_kernel: branch_entry once, outside_index per tile, its own quarter loads of V and of the
// conditional — per-tile address helpers cost it 1 %); the adjoint's launch is common.h's LAUNCH_NW_DYN_LDS.
// Pattern weights (grad_weight_kernel<NW>, grad_weight_nuc_kernel): per pattern l0 = V . (P in) at the first requested branch, as
// deriv.hip forms it, mixed over the classes by weight with the exponents aligned on the smallest (mix3's rule: an exact zero carries
// no exponent), then ginv = f_s / L_s (0: the pattern takes no part).  With one class this runs inside the chunk it serves; with several
// the mixed L_s must be complete before any class accumulates, so the walk runs twice: once for the weights, once for the sums.
// Phase 2 (grad_accum_kernel<NW>): one workgroup of NW waves per (branch with a request, segment of 32 tiles); per tile V diag(g) and in
// go through LDS into the A / B operand layouts (the pattern is the reduction index: four k-steps a tile) and W stays in NW x NW
// accumulator tiles, one row block a wave.  4 states (grad_accum_nuc_kernel): a thread per pattern, 16 products, a wave sum.
// Every (branch, class, segment) leaves one D x D partial; a chunk that starts inside a segment continues that segment's partial.
// grad_reduce_kernel sums the partials in ascending segment order; shards are summed on the host in shard order.
// Adjoint (frechet_adjoint_kernel<NW>, frechet_adjoint4_kernel): one workgroup per matrix, on A = Q^T: X = A / 2^p with
// ||X||_inf <= 1/4, E' = W / 2^p, the degree-13 Taylor pair A_j = A_{j-1} X / j, D_j = (D_{j-1} X + A_{j-1} E') / j, then p times
// L <- P L + L P, P <- P P; four matrices in LDS, the running sums in registers, every product on the FP64 MFMA.  No diag_populator.
// Remainder: ||sum_{j > 13} D_j|| <= ||E'|| (1/4)^13 / 13! / (1 - 1/56) < 2.5e-18 ||E'||.
// Nothing joins by order of arrival and there are no floating-point atomics: two identical calls give identical bits.  All scratch comes
// from the pool and goes back before the call returns; the partition's matrices, images, schedules and caches are not written.
#include "devutil.h"
#include "outside_pass.h"
#include "partition.h"

using namespace hyhip;

namespace hyhip {
namespace {

constexpr int kSegPatterns = 512;  // a segment: 32 tiles of 16 patterns (4 states: 8 waves of 64)
constexpr int kTaylorDegree = 13;
constexpr double kFrechetMaxNorm = 1099511627776.0;  // 2^40: beyond it the matrix is refused (output NaN)

struct GradArgs {        // the gradient's own blocks, beside the WalkArgs and the OutsideSlice
  double *Lm;            // [S_pad] likelihood mixed over the classes so far
  int32_t *em;           // its exponent
  int32_t *live;         // [C][S_pad] the class's weighted likelihood is not exactly 0
  double *ginv;          // [S_pad] f_s / L_s, 0 where the pattern takes no part
  long long *tile_skip;  // [tiles] patterns of positive frequency with L_s == 0
  int seg_tiles, nseg, D;
  double *part;          // [branches][C][nseg][D * D]
};

// this class's l0 (exponent e) of pattern `site` into the mix; behind the last class ginv.  Returns 1 for a skipped pattern.
__device__ __forceinline__ int mix_weight(const WalkArgs &wa, const OutsideSlice &sl, const GradArgs &a, int site, double l0, int e) {
  l0 *= sl.w;
  a.live[(size_t)sl.cls * wa.S_pad + site] = l0 != 0.;
  if (!sl.first) {
    const double o = a.Lm[site];
    const int eo = a.em[site];
    if (l0 == 0.) {
      l0 = o, e = eo;
    } else if (o != 0.) {
      double so, sn;
      e = align_exponents(eo, e, so, sn);
      l0 = o * so + l0 * sn;
    }
  }
  a.Lm[site] = l0;
  a.em[site] = e;
  int skip = 0;
  if (sl.last) {
    const double f = sl.freq[site];
    double gi = 0.;
    if (f != 0.) {
      if (l0 == 0.) skip = 1;
      else gi = f / l0;
    }
    a.ginv[site] = gi;
  }
  return skip;
}

// g_{s,c}: what multiplies V in^T of pattern `site` in class sl.cls (e: exponent of V plus exponent of in)
__device__ __forceinline__ double pattern_scale(const WalkArgs &wa, const OutsideSlice &sl, const GradArgs &a, int site, int e) {
  double gs = a.ginv[site];
  if (sl.C > 1 && !a.live[(size_t)sl.cls * wa.S_pad + site]) gs = 0.;
  return gs == 0. ? 0. : sl.w * gs * ldexp(1.0, -64 * (e - a.em[site]));
}

template <int NW>
__global__ __launch_bounds__(64) void grad_weight_kernel(WalkArgs wa, OutsideSlice sl, GradArgs a) {
  constexpr int NKK = 4 * NW;
  const int lane = threadIdx.x, tile = sl.tile0 + blockIdx.x, site = tile * 16 + (lane & 15);
  double V[NKK], E[NKK];
  int e, ecnt;
  const int4 ce = branch_outside<NKK>(wa, sl, 0, tile, lane, V, e);
  edge_product<NW>(wa, ce, tile, lane, E, ecnt);
  e += ecnt;
  double l0 = 0.;
#pragma unroll
  for (int kk = 0; kk < NKK; kk++) l0 += V[kk] * E[kk];
  l0 = row_sum4(l0);
  int skip = 0;
  if (lane >> 4 == 0) skip = mix_weight(wa, sl, a, site, l0, e);
  if (sl.last) {
    skip = wave_sum<16>(skip);
    if (lane == 0) a.tile_skip[tile] = skip;
  }
}

__global__ __launch_bounds__(64) void grad_weight_nuc_kernel(WalkArgs wa, OutsideSlice sl, GradArgs a) {
  const int lane = threadIdx.x, tile = sl.tile0 + blockIdx.x;
  const size_t s = (size_t)tile * 64 + lane;
  double V[4], in[4], E[4];
  int e, ecnt;
  const int4 ce = nuc_branch_outside(wa, sl, 0, tile, lane, V, e);
  nuc_child_vec(wa, ce, s, in, ecnt);
  e += ecnt;
  mat4_vec(wa.Prow + (size_t)ce.y * 16, in, E);
  int skip = mix_weight(wa, sl, a, (int)s, dot4(V, E), e);
  if (sl.last) {
    skip = wave_sum<64>(skip);
    if (lane == 0) a.tile_skip[tile] = skip;
  }
}

// W += V_tile diag(g) in_tile^T over the tiles of one segment that this chunk holds
template <int NW>
__global__ __launch_bounds__(64 * NW) void grad_accum_kernel(WalkArgs wa, OutsideSlice sl, GradArgs a) {
  constexpr int NKK = 4 * NW, DP = 16 * NW, TILE = NKK * 64, LD = 17;
  __shared__ double As[DP * LD], Bs[DP * LD];  // [state][pattern of the tile]: V g and in
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, sp = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int seg = sl.tile0 / a.seg_tiles + (int)blockIdx.x;
  const int t_lo = max(seg * a.seg_tiles, sl.tile0), t_hi = min((seg + 1) * a.seg_tiles, sl.tile0 + sl.nt);
  const int bi = sl.b0 + (int)blockIdx.y;
  const int4 ce = branch_entry(wa, sl, bi);  // (.y the node code, .z the internal index below the branch or -1)
  const int D = a.D;
  double *part = a.part + (((size_t)bi * sl.C + sl.cls) * a.nseg + seg) * D * D;
  const bool cont = t_lo > seg * a.seg_tiles;  // an earlier chunk began this segment
  f64x4 acc[NW];
#pragma unroll
  for (int w = 0; w < NW; w++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * wv + 4 * r + g, col = 16 * w + sp;
      acc[w][r] = cont && row < D && col < D ? part[row * D + col] : 0.;
    }
  for (int tile = t_lo; tile < t_hi; tile++) {
    const int site = tile * 16 + sp;
    const size_t o = outside_index(sl, ce.y, tile);
    int e = sl.Vcnt[o * 16 + sp];
    int code = 0;
    if (ce.z >= 0) e += wa.counts[(size_t)ce.z * wa.S_pad + site];
    else code = (int)wa.codes_tile[((size_t)tile * wa.L + ce.y) * 16 + sp];
    const double sc = pattern_scale(wa, sl, a, site, e);
    const double *vb = sl.V + o * TILE;
    const double *ib = wa.partials + ((size_t)max(ce.z, 0) * wa.ntiles + tile) * TILE;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int k2 = 2 * wv + q;
      const unsigned off = (unsigned)(k2 * 64 + lane) * 16u;
      const f64x2 v = ld16(vb, off);
      f64x2 b;
      if (ce.z >= 0) {
        b = ld16(ib, off);
      } else {
#pragma unroll
        for (int h = 0; h < 2; h++) b[h] = leaf_value<DP>(wa, code, 4 * (2 * k2 + h) + g);
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int st = 4 * (2 * k2 + h) + g;
        As[st * LD + sp] = sc != 0. ? v[h] * sc : 0.;  // (a pattern that takes no part must not bring a NaN of its own)
        Bs[st * LD + sp] = sc != 0. ? b[h] : 0.;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      const double av = As[(16 * wv + sp) * LD + 4 * ks + g];
#pragma unroll
      for (int w = 0; w < NW; w++) acc[w] = mfma(av, Bs[(16 * w + sp) * LD + 4 * ks + g], acc[w]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int w = 0; w < NW; w++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * wv + 4 * r + g, col = 16 * w + sp;
      if (row < D && col < D) part[row * D + col] = acc[w][r];
    }
}

// 4 states: one wave per (branch, segment), one thread per pattern of a tile of 64
__global__ __launch_bounds__(64) void grad_accum_nuc_kernel(WalkArgs wa, OutsideSlice sl, GradArgs a) {
  const int lane = threadIdx.x;
  const int seg = sl.tile0 / a.seg_tiles + (int)blockIdx.x;
  const int t_lo = max(seg * a.seg_tiles, sl.tile0), t_hi = min((seg + 1) * a.seg_tiles, sl.tile0 + sl.nt);
  const int bi = sl.b0 + (int)blockIdx.y;
  double *part = a.part + (((size_t)bi * sl.C + sl.cls) * a.nseg + seg) * 16;
  double acc[16];
  for (int k = 0; k < 16; k++) acc[k] = 0.;
  for (int tile = t_lo; tile < t_hi; tile++) {
    const size_t s = (size_t)tile * 64 + lane;
    double V[4], in[4];
    int e, ecnt;
    const int4 ce = nuc_branch_outside(wa, sl, bi, tile, lane, V, e);
    nuc_child_vec(wa, ce, s, in, ecnt);
    const double sc = pattern_scale(wa, sl, a, (int)s, e + ecnt);
    if (sc != 0.)
      for (int i = 0; i < 4; i++) {
        const double vi = V[i] * sc;
        for (int j = 0; j < 4; j++) acc[4 * i + j] += vi * in[j];
      }
  }
  const bool cont = t_lo > seg * a.seg_tiles;
  for (int k = 0; k < 16; k++) {
    const double x = wave_sum<64>(acc[k]);
    if (lane == 0) part[k] = cont ? part[k] + x : x;
  }
}

// W of (branch, class) blockIdx.x: its segments' partials in ascending order; a NaN anywhere makes the whole block NaN
__global__ __launch_bounds__(256) void grad_reduce_kernel(const double *__restrict__ part, int nseg, int DD, double *__restrict__ out) {
  const double *src = part + (size_t)blockIdx.x * nseg * DD;
  double *dst = out + (size_t)blockIdx.x * DD;
  int bad = 0;
  for (int e = threadIdx.x; e < DD; e += 256) {
    double s = 0.;
    for (int k = 0; k < nseg; k++) s += src[(size_t)k * DD + e];
    if (s != s) bad = 1;
    dst[e] = s;
  }
  if (__syncthreads_or(bad))
    for (int e = threadIdx.x; e < DD; e += 256) dst[e] = NAN;
}

// ---- the adjoint of the exponential's Frechet derivative -----------------------------------------------------------------------------
struct FrechetArgs {
  const double *Q, *W;  // [n][D * D] row-major; matrix m reads W block w_map[m] (nullptr: m)
  const int *w_map;
  double *out;          // [n][D * D]: L(Q^T, W)
  int *status;          // [n] 1: the matrix could not be handled (its output is NaN)
  int D, n;
};

// acc (row block wv, C/D layout) += M1 M2, both [DP][LD] in LDS
template <int NW>
__device__ __forceinline__ void lds_product(const double *M1, const double *M2, int wv, int lane, f64x4 (&acc)[NW]) {
  constexpr int NKK = 4 * NW, LD = 16 * NW + 2;
  const int g = lane >> 4, sl = lane & 15;
#pragma unroll 4
  for (int kk = 0; kk < NKK; kk++) {
    const double av = M1[(16 * wv + sl) * LD + 4 * kk + g];
#pragma unroll
    for (int w = 0; w < NW; w++) acc[w] = mfma(av, M2[(4 * kk + g) * LD + 16 * w + sl], acc[w]);
  }
}

template <int NW>
__device__ __forceinline__ void lds_put(double *M, int wv, int lane, const f64x4 (&x)[NW]) {
  constexpr int LD = 16 * NW + 2;
  const int g = lane >> 4, sl = lane & 15;
#pragma unroll
  for (int w = 0; w < NW; w++)
#pragma unroll
    for (int r = 0; r < 4; r++) M[(16 * wv + 4 * r + g) * LD + 16 * w + sl] = x[w][r];
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void frechet_adjoint_kernel(FrechetArgs a) {
  constexpr int DP = 16 * NW, LD = DP + 2, NT = 64 * NW;
  extern __shared__ __align__(16) double sm[];
  double *X = sm, *Ep = X + DP * LD, *Aj = Ep + DP * LD, *Dj = Aj + DP * LD, *red = Dj + DP * LD;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, sl = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = blockIdx.x, D = a.D;
  const double *Q = a.Q + (size_t)m * D * D, *W = a.W + (size_t)(a.w_map ? a.w_map[m] : m) * D * D;
  for (int idx = tid; idx < DP * DP; idx += NT) {
    const int r = idx / DP, c = idx - r * DP;
    const bool in = r < D && c < D;
    X[r * LD + c] = in ? Q[c * D + r] : 0.;  // A = Q^T
    Ep[r * LD + c] = in ? W[r * D + c] : 0.;
  }
  __syncthreads();
  if (tid < DP) {
    double s = 0.;
    for (int c = 0; c < DP; c++) s += fabs(X[tid * LD + c]);
    red[tid] = s;
  }
  __syncthreads();
  double norm = 0.;
  bool bad = false;
  for (int r = 0; r < DP; r++) {
    norm = fmax(norm, red[r]);
    bad = bad || red[r] != red[r];
  }
  bad = bad || !(norm < kFrechetMaxNorm);
  int p = 0;
  if (!bad)
    for (double s = norm; s > 0.25; s *= 0.5) p++;
  const double scale = ldexp(1.0, -p);
  __syncthreads();
  for (int idx = tid; idx < DP * DP; idx += NT) {
    const int r = idx / DP, c = idx - r * DP;
    const double x = X[r * LD + c] * scale, e = Ep[r * LD + c] * scale;
    X[r * LD + c] = x, Aj[r * LD + c] = x;
    Ep[r * LD + c] = e, Dj[r * LD + c] = e;
  }
  __syncthreads();
  f64x4 sa[NW], sd[NW];  // this wave's row block of I + sum_j A_j and of sum_j D_j
#pragma unroll
  for (int w = 0; w < NW; w++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * wv + 4 * r + g, col = 16 * w + sl;
      sa[w][r] = X[row * LD + col] + (row == col ? 1. : 0.);
      sd[w][r] = Ep[row * LD + col];
    }
  for (int j = 2; j <= kTaylorDegree; j++) {
    f64x4 na[NW], nd[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) na[w] = nd[w] = (f64x4){0., 0., 0., 0.};
    lds_product<NW>(Dj, X, wv, lane, nd);
    lds_product<NW>(Aj, Ep, wv, lane, nd);
    lds_product<NW>(Aj, X, wv, lane, na);
    const double dj = (double)j;
#pragma unroll
    for (int w = 0; w < NW; w++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        na[w][r] /= dj, nd[w][r] /= dj;
        sa[w][r] += na[w][r], sd[w][r] += nd[w][r];
      }
    __syncthreads();
    lds_put<NW>(Aj, wv, lane, na);
    lds_put<NW>(Dj, wv, lane, nd);
    __syncthreads();
  }
  // squarings: P in Aj's place, L in Dj's
  if (p > 0) {
    lds_put<NW>(Aj, wv, lane, sa);
    lds_put<NW>(Dj, wv, lane, sd);
    __syncthreads();
  }
  for (int it = 0; it < p; it++) {
#pragma unroll
    for (int w = 0; w < NW; w++) sd[w] = (f64x4){0., 0., 0., 0.};
    lds_product<NW>(Aj, Dj, wv, lane, sd);
    lds_product<NW>(Dj, Aj, wv, lane, sd);
    if (it + 1 < p) {
#pragma unroll
      for (int w = 0; w < NW; w++) sa[w] = (f64x4){0., 0., 0., 0.};
      lds_product<NW>(Aj, Aj, wv, lane, sa);
      __syncthreads();
      lds_put<NW>(Aj, wv, lane, sa);
      lds_put<NW>(Dj, wv, lane, sd);
      __syncthreads();
    }
  }
  int nonfinite = bad ? 1 : 0;
#pragma unroll
  for (int w = 0; w < NW; w++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * wv + 4 * r + g, col = 16 * w + sl;
      if (row < D && col < D && !(fabs(sd[w][r]) < HUGE_VAL)) nonfinite = 1;
    }
  nonfinite = __syncthreads_or(nonfinite);
  double *out = a.out + (size_t)m * D * D;
#pragma unroll
  for (int w = 0; w < NW; w++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * wv + 4 * r + g, col = 16 * w + sl;
      if (row < D && col < D) out[row * D + col] = nonfinite ? NAN : sd[w][r];
    }
  if (tid == 0) a.status[m] = nonfinite;
}

__device__ __forceinline__ void mm4_add(const double *x, const double *y, double *z) {  // z += x y
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = z[4 * i + j];
      for (int k = 0; k < 4; k++) s += x[4 * i + k] * y[4 * k + j];
      z[4 * i + j] = s;
    }
}

// 4 states: the same scheme in scalar form, one thread per matrix
__global__ __launch_bounds__(64) void frechet_adjoint4_kernel(FrechetArgs a) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= a.n) return;
  const double *Q = a.Q + (size_t)m * 16, *W = a.W + (size_t)(a.w_map ? a.w_map[m] : m) * 16;
  double X[16], Ep[16], Aj[16], Dj[16], SA[16], SD[16], na[16], nd[16];
  double norm = 0.;
  bool bad = false;
  for (int r = 0; r < 4; r++) {
    double s = 0.;
    for (int c = 0; c < 4; c++) {
      X[4 * r + c] = Q[4 * c + r];
      Ep[4 * r + c] = W[4 * r + c];
      s += fabs(X[4 * r + c]);
    }
    norm = fmax(norm, s);
    bad = bad || s != s;
  }
  bad = bad || !(norm < kFrechetMaxNorm);
  int p = 0;
  if (!bad)
    for (double s = norm; s > 0.25; s *= 0.5) p++;
  const double scale = ldexp(1.0, -p);
  for (int k = 0; k < 16; k++) {
    X[k] *= scale, Ep[k] *= scale;
    Aj[k] = X[k], Dj[k] = Ep[k];
    SA[k] = X[k] + ((k >> 2) == (k & 3) ? 1. : 0.), SD[k] = Ep[k];
  }
  for (int j = 2; j <= kTaylorDegree; j++) {
    for (int k = 0; k < 16; k++) na[k] = nd[k] = 0.;
    mm4_add(Dj, X, nd);
    mm4_add(Aj, Ep, nd);
    mm4_add(Aj, X, na);
    for (int k = 0; k < 16; k++) {
      Aj[k] = na[k] / (double)j, Dj[k] = nd[k] / (double)j;
      SA[k] += Aj[k], SD[k] += Dj[k];
    }
  }
  for (int it = 0; it < p; it++) {
    for (int k = 0; k < 16; k++) na[k] = nd[k] = 0.;
    mm4_add(SA, SD, nd);
    mm4_add(SD, SA, nd);
    mm4_add(SA, SA, na);
    for (int k = 0; k < 16; k++) SA[k] = na[k], SD[k] = nd[k];
  }
  for (int k = 0; k < 16; k++) bad = bad || !(fabs(SD[k]) < HUGE_VAL);
  for (int k = 0; k < 16; k++) a.out[(size_t)m * 16 + k] = bad ? NAN : SD[k];
  a.status[m] = bad ? 1 : 0;
}

int launch_frechet(const FrechetArgs &a, hipStream_t stream) {
  if (a.D == 4) {
    hipLaunchKernelGGL(frechet_adjoint4_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, stream, a);
    HIPCHK(hipGetLastError());
    return 0;
  }
  static bool attr_done[64][5];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const int NW = (a.D + 15) / 16, DP = 16 * NW;
  const size_t lds = (size_t)(4 * DP * (DP + 2) + DP) * sizeof(double);
  LAUNCH_NW_DYN_LDS(frechet_adjoint_kernel, NW, attr_done, dev, dim3((unsigned)a.n), dim3((unsigned)(64 * NW)), lds, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// grad[m][k] = sum_{i != j} T_k[i][j] (S_m[i][j] - S_m[i][i]): one workgroup per matrix, a fixed-order tree per coefficient
__global__ __launch_bounds__(256) void grad_contract_kernel(const double *__restrict__ S, const double *__restrict__ T, int D, int K,
                                                            double *__restrict__ out) {
  __shared__ double red[256];
  const int m = blockIdx.x, tid = threadIdx.x, DD = D * D;
  const double *Sm = S + (size_t)m * DD;
  for (int k = 0; k < K; k++) {
    double acc = 0.;
    for (int e = tid; e < DD; e += 256) {
      const int i = e / D, j = e - i * D;
      if (i != j) acc += T[(size_t)k * DD + e] * (Sm[e] - Sm[i * D + i]);
    }
    red[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    if (tid == 0) out[(size_t)m * K + k] = red[0];
    __syncthreads();
  }
}


// W of every branch with a request: [groups][C][D * D] on the host, summed over the shards in shard order; skipped patterns of the call
int sensitivities(hyphy_hip_partition *p, const OutsideCall &oc, const double *weights, std::vector<double> &Wh, int64_t &skipped) {
  const int C = (int)p->C, NW = p->NW, D = (int)p->D, DD = D * D;
  const bool nuc = p->nuc;
  const int nb = (int)oc.groups.branch.size();
  Wh.assign((size_t)nb * C * DD, 0.);
  skipped = 0;
  std::vector<double> part_h(Wh.size());
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    Blocks blk;
    OutsideScratch sc;
    sc.plan(p, s, oc);
    const int seg_tiles = kSegPatterns / sc.TP, nseg = (sc.ntiles + seg_tiles - 1) / seg_tiles;
    if (sc.ct < sc.ntiles && sc.ct >= seg_tiles) sc.ct -= sc.ct % seg_tiles;  // chunks are cut at segment boundaries
    double *Lm = nullptr, *ginv = nullptr, *part = nullptr, *Wd = nullptr;
    int32_t *em = nullptr, *live = nullptr;
    long long *tile_skip = nullptr;
    HIPCHK(blk.get(&Lm, (size_t)s.S_pad));
    HIPCHK(blk.get(&ginv, (size_t)s.S_pad));
    HIPCHK(blk.get(&em, (size_t)s.S_pad));
    HIPCHK(blk.get(&live, (size_t)C * s.S_pad));
    HIPCHK(blk.get(&tile_skip, (size_t)sc.ntiles));
    HIPCHK(blk.get(&part, (size_t)nb * C * nseg * DD));
    HIPCHK(blk.get(&Wd, (size_t)nb * C * DD));
    if (sc.get(p, oc, blk)) return -1;
    if (sc.upload(p, oc, s.stream)) return -1;
    const GradArgs ga = {Lm, em, live, ginv, tile_skip, seg_tiles, nseg, D, part};
    auto weigh = [&](const WalkArgs &a, const OutsideSlice &sl, dim3 grid) {
      if (sl.b0) return;
      if (nuc) hipLaunchKernelGGL(grad_weight_nuc_kernel, dim3(grid.x), dim3(64), 0, s.stream, a, sl, ga);
      else LAUNCH_NW(grad_weight_kernel, NW, dim3(grid.x), dim3(64), s.stream, a, sl, ga);
    };
    auto accumulate = [&](const WalkArgs &a, const OutsideSlice &sl, dim3 grid) {
      const unsigned segs = (unsigned)((sl.tile0 + sl.nt - 1) / seg_tiles - sl.tile0 / seg_tiles + 1);
      if (nuc) hipLaunchKernelGGL(grad_accum_nuc_kernel, dim3(segs, grid.y), dim3(64), 0, s.stream, a, sl, ga);
      else LAUNCH_NW(grad_accum_kernel, NW, dim3(segs, grid.y), dim3((unsigned)(64 * NW)), s.stream, a, sl, ga);
    };
    int walked;
    if (C == 1) {
      walked = outside_chunks(p, s, oc, sc, weights, [&](const WalkArgs &a, const OutsideSlice &sl, dim3 grid) {
        weigh(a, sl, grid);
        accumulate(a, sl, grid);
      });
    } else {
      walked = outside_chunks(p, s, oc, sc, weights, weigh);
      if (!walked) walked = outside_chunks(p, s, oc, sc, weights, accumulate);
    }
    if (walked) return -1;
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)(nb * C)), dim3(256), 0, s.stream, part, nseg, DD, Wd);
    HIPCHK(hipGetLastError());
    std::vector<long long> h_skip((size_t)sc.ntiles);
    HIPCHK(hipMemcpyAsync(part_h.data(), Wd, part_h.size() * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(h_skip.data(), tile_skip, h_skip.size() * sizeof(long long), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    for (size_t k = 0; k < Wh.size(); k++) Wh[k] += part_h[k];
    for (long long k : h_skip) skipped += (int64_t)k;
  }
  return 0;
}

// out[m] = L(q[m]^T, W[w_map[m]]) (coeffs: q built from the templates, and out[m][k] the chained coefficient gradient) on shard 0's device
int adjoint_on_device(hyphy_hip_partition *p, const std::string &pre, int64_t nm, const double *q_dense, const double *coeffs,
                      const std::vector<double> &Wh, const std::vector<int> &w_map, double *out) {
  Shard &s = p->shards[0];
  const int D = (int)p->D, DD = D * D, K = (int)p->K;
  HIPCHK(hipSetDevice(s.device));
  Blocks blk;
  double *src = nullptr, *gq = nullptr, *Wd = nullptr, *Sd = nullptr, *gd = nullptr;
  int *map = nullptr, *status = nullptr;
  const size_t nq = coeffs ? (size_t)nm * K : (size_t)nm * DD;
  HIPCHK(blk.get(&src, nq));
  if (coeffs) HIPCHK(blk.get(&gq, (size_t)nm * DD));
  if (coeffs) HIPCHK(blk.get(&gd, (size_t)nm * K));
  HIPCHK(blk.get(&Wd, Wh.size()));
  HIPCHK(blk.get(&Sd, (size_t)nm * DD));
  HIPCHK(blk.get(&map, (size_t)nm));
  HIPCHK(blk.get(&status, (size_t)nm));
  HIPCHK(hipMemcpyAsync(src, coeffs ? coeffs : q_dense, nq * sizeof(double), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(Wd, Wh.data(), Wh.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(map, w_map.data(), (size_t)nm * sizeof(int), hipMemcpyHostToDevice, s.stream));
  // rate matrices built from the templates into the call's own scratch, never the partition's Q buffer
  if (coeffs) launch_build_q(s.templates, src, (int)nm, K, D, gq, s.stream);
  FrechetArgs fa = {coeffs ? gq : src, Wd, map, Sd, status, D, (int)nm};
  if (launch_frechet(fa, s.stream)) return -1;
  if (coeffs) {
    hipLaunchKernelGGL(grad_contract_kernel, dim3((unsigned)nm), dim3(256), 0, s.stream, Sd, s.templates, D, K, gd);
    HIPCHK(hipGetLastError());
  }
  std::vector<int> h_status((size_t)nm);
  HIPCHK(hipMemcpyAsync(out, coeffs ? gd : Sd, (coeffs ? (size_t)nm * K : (size_t)nm * DD) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipMemcpyAsync(h_status.data(), status, (size_t)nm * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  for (int64_t m = 0; m < nm; m++)
    if (h_status[(size_t)m])
      return fail(pre + "request " + std::to_string(m / p->C) + " class " + std::to_string(m % p->C) +
                  ": the rate matrix or the sensitivities cannot be handled (not a number, or a norm of 2^40 or more)");
  return 0;
}

int grad_common(const char *what, hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *q_dense, const double *coeffs,
                const double *weights, double *out, int64_t *skipped_out) {
  const std::string pre = std::string(what) + ": ";
  if (!p) return fail(pre + "partition == NULL");
  if (n < 0) return fail(pre + "n < 0");
  if (check_pass_ready(p, pre, weights)) return -1;
  if (n == 0) return 0;
  if (!nodes || !out) return fail(pre + "null argument");
  if (check_requests(p, pre, "request", n, nodes, coeffs != nullptr)) return -1;
  const KeepForms keep = {p, p->last_reduce, last_expm_kernel()};
  OutsideCall oc;
  if (begin_outside(p, oc, nodes, n)) return -1;
  const int C = (int)p->C;
  const size_t DD = (size_t)p->D * p->D;
  std::vector<double> Wh;
  int64_t skipped = 0;
  if (sensitivities(p, oc, weights, Wh, skipped)) return -1;
  std::vector<int> group_of((size_t)n);
  for (size_t g = 0; g + 1 < oc.groups.off.size(); g++)
    for (int k = oc.groups.off[g]; k < oc.groups.off[g + 1]; k++) group_of[(size_t)oc.groups.order[(size_t)k]] = (int)g;
  if (skipped_out)
    for (int64_t t = 0; t < n; t++) skipped_out[t] = skipped;
  if (!q_dense && !coeffs) {
    for (int64_t t = 0; t < n; t++)
      std::copy(Wh.begin() + (size_t)group_of[(size_t)t] * C * DD, Wh.begin() + (size_t)(group_of[(size_t)t] + 1) * C * DD, out + (size_t)t * C * DD);
    return 0;
  }
  std::vector<int> w_map((size_t)n * C);
  for (int64_t t = 0; t < n; t++)
    for (int c = 0; c < C; c++) w_map[(size_t)t * C + c] = group_of[(size_t)t] * C + c;
  return adjoint_on_device(p, pre, n * C, q_dense, coeffs, Wh, w_map, out);
}

}  // namespace
}  // namespace hyhip

extern "C" {

int hyphy_hip_branch_sensitivities(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *weights, double *dp_out,
                                   int64_t *skipped_out) {
  return grad_common("branch_sensitivities", p, n, nodes, nullptr, nullptr, weights, dp_out, skipped_out);
}

int hyphy_hip_branch_gradient(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *q_dense, const double *weights,
                              double *dq_out, int64_t *skipped_out) {
  if (p && n > 0 && !q_dense) return fail("branch_gradient: null rate-matrix pointer");
  return grad_common("branch_gradient", p, n, nodes, q_dense, nullptr, weights, dq_out, skipped_out);
}

int hyphy_hip_branch_gradient_built(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *coeffs, const double *weights,
                                    double *grad_out, int64_t *skipped_out) {
  if (p && n > 0 && !coeffs) return fail("branch_gradient_built: null coefficient pointer");
  return grad_common("branch_gradient_built", p, n, nodes, nullptr, coeffs, weights, grad_out, skipped_out);
}

int hyphy_hip_expm_frechet_adjoint_batch(int64_t D, int64_t n, const double *q_dense, const double *w_dense, double *out) {
  if (D < 2 || D > 64) return fail("expm_frechet_adjoint_batch: unsupported state count (this version: 2 <= D <= 64)");
  if (n <= 0) return 0;
  if (n > 0x3fffffff) return fail("expm_frechet_adjoint_batch: too many matrices");
  if (!q_dense || !w_dense || !out) return fail("expm_frechet_adjoint_batch: null matrix pointer");
  if (hyphy_hip_device_count() <= 0) return fail("no HIP device available (this library has no CPU fallback)");
  const size_t count = (size_t)n * D * D;
  Blocks blk;
  double *dq = nullptr, *dw = nullptr, *dout = nullptr;
  int *status = nullptr;
  HIPCHK(blk.get(&dq, count));
  HIPCHK(blk.get(&dw, count));
  HIPCHK(blk.get(&dout, count));
  HIPCHK(blk.get(&status, (size_t)n));
  HIPCHK(hipMemcpy(dq, q_dense, count * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dw, w_dense, count * sizeof(double), hipMemcpyHostToDevice));
  FrechetArgs fa = {dq, dw, nullptr, dout, status, (int)D, (int)n};
  if (launch_frechet(fa, nullptr)) return -1;
  HIPCHK(hipMemcpy(out, dout, count * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
