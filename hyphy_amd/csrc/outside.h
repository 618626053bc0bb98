// Device helpers of the pre-order ("outside") walks: the marginal reconstruction (marginal.hip) and the outside pass of the branch
// trials (trials.hip) walk the same host-compiled program (plan_marginal_program) with the same products, the same 2^64 rescaling
// and the same transposed matrix images.  gfx950 only.
#pragma once
#include "devutil.h"

namespace hyhip {
namespace {

// program entries (int4): a node header (0, internal index, children, 1 for the root), then one entry per child
// (1, child node code = matrix slot, child internal index or -1 for a leaf, position among the children)
struct MargArgs {
  const int4 *prog;
  int n_prog;
  int NW, L, S, S_pad, ntiles, maxk, which, first, D;
  double w;                  // weight of this class (1 when C == 1)
  const double *Pfrag;       // [B][NW][NKK*64] A-operand images of this class
  const double *PTg;         // [B][DP][NW][4][4] column-gather images (leaf edges)
  const double *PT;          // [B][NW][NKK*64] A-operand images of the TRANSPOSED matrices (marginal scratch)
  const int16_t *codes_tile; // [ntiles][L][16]
  const double *ambig;       // [n_ambig][DP]
  const double *pi;          // [DP]
  const double *partials;    // this class: [I][ntiles][TILE]
  const int32_t *counts;     // this class: [I][S_pad]
  double *U;                 // [I][ntiles][TILE] outside vectors
  int32_t *Ucnt;             // [I][S_pad]
  double *work;              // [ntiles][2 maxk][TILE]
  int32_t *wcnt;             // [ntiles][2 maxk][16]
  double *acc;               // [rows][S][D]
  double *den;               // [rows][S_pad]
  int32_t *aexp;             // [rows][S_pad]
};

// transposed A-operand images M[r][c] = P[c][r] of every branch of one class: leaves from the column-gather image (the only
// image the exponential writes for a leaf without ambiguity codes), internal nodes from the A-operand image
__global__ __launch_bounds__(256) void marg_transpose_kernel(const double *__restrict__ Pfrag, const double *__restrict__ PTg,
                                                             double *__restrict__ PT, int NW, int L) {
  const int NKK = 4 * NW, DP = 16 * NW, TILE = NKK * 64;
  const int b = blockIdx.x;
  const double *src = Pfrag + (size_t)b * DP * DP, *gsrc = PTg + (size_t)b * DP * DP;
  double *dst = PT + (size_t)b * DP * DP;
  for (int idx = threadIdx.x; idx < DP * DP; idx += blockDim.x) {
    const int w = idx / TILE, rem = idx - w * TILE;
    const int k2 = rem >> 7, l = (rem >> 1) & 63, kk = 2 * k2 + (rem & 1);
    const int r = 16 * w + (l & 15), c = 4 * kk + (l >> 4);  // M[r][c] = P[c][r]
    dst[idx] = b < L ? gsrc[(r * NW + (c >> 4)) * 16 + (c & 3) * 4 + ((c >> 2) & 3)]
                     : src[(c >> 4) * TILE + frag_index(r >> 2, (r & 3) * 16 + (c & 15))];
  }
}

template <int NKK>
__device__ __forceinline__ void rescale_vec(double (&v)[NKK], int &cnt) {
  double t = 0.;
#pragma unroll
  for (int kk = 0; kk < NKK; kk++) t += v[kk];
  const double tot = row_sum4(t);
  if (__any(!(tot >= kScalerThreshold && tot <= kScalerUp))) {  // rare
    double sc;
    cnt += rescale_decision(tot, sc);
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) v[kk] *= sc;
  }
}

template <int NKK>
__device__ __forceinline__ void ld_vec(const double *base, int lane, double (&v)[NKK]) {
#pragma unroll
  for (int k2 = 0; k2 < NKK / 2; k2++) {
    const f64x2 x = ld16(base, (unsigned)(k2 * 64 + lane) * 16u);
    v[2 * k2] = x[0];
    v[2 * k2 + 1] = x[1];
  }
}
template <int NKK>
__device__ __forceinline__ void st_vec(double *base, int lane, const double (&v)[NKK]) {
#pragma unroll
  for (int k2 = 0; k2 < NKK / 2; k2++) st16(base, (unsigned)(k2 * 64 + lane) * 16u, (f64x2){v[2 * k2], v[2 * k2 + 1]});
}

// out = A x B where A is an A-operand image ([NW][NKK*64]) and B the fragment vector `b` (B operand of k-step kk = b[kk])
template <int NW>
__device__ __forceinline__ void mfma_product(const double *A, const double (&b)[4 * NW], int lane, double (&out)[4 * NW]) {
  constexpr int NKK = 4 * NW, TILE = NKK * 64;
  f64x4 prod[NW];
#pragma unroll
  for (int w = 0; w < NW; w++) prod[w] = (f64x4){0., 0., 0., 0.};
#pragma unroll
  for (int k2 = 0; k2 < NKK / 2; k2++) {
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const f64x2 av = ld16(A + w * TILE, (unsigned)(k2 * 64 + lane) * 16u);
      prod[w] = mfma(av[0], b[2 * k2], prod[w]);
      prod[w] = mfma(av[1], b[2 * k2 + 1], prod[w]);
    }
  }
#pragma unroll
  for (int w = 0; w < NW; w++)
#pragma unroll
    for (int r = 0; r < 4; r++) out[4 * w + r] = prod[w][r];  // C/D row 16w + 4r + g = fragment k-step 4w + r
}

// leaf vector of leaf code c at this lane's states (state indicator or ambiguity row)
template <int NKK>
__device__ __forceinline__ void leaf_vec(const MargArgs &a, int c, int g, double (&lv)[NKK]) {
  const int DP = 4 * NKK;
#pragma unroll
  for (int kk = 0; kk < NKK; kk++) lv[kk] = c >= 0 ? (4 * kk + g == c ? 1. : 0.) : a.ambig[(size_t)(-c - 1) * DP + 4 * kk + g];
}

// edge product E of child entry ce and its 2^64 exponent
template <int NW>
__device__ __forceinline__ void edge_product(const MargArgs &a, const int4 &ce, int tile, int lane, double (&E)[4 * NW], int &ecnt) {
  constexpr int NKK = 4 * NW, DP = 16 * NW, TILE = NKK * 64;
  const int g = lane >> 4, sl = lane & 15;
  const double *Pf = a.Pfrag + (size_t)ce.y * DP * DP;
  if (ce.z >= 0) {
    double b[NKK];
    ld_vec<NKK>(a.partials + ((size_t)ce.z * a.ntiles + tile) * TILE, lane, b);
    ecnt = a.counts[(size_t)ce.z * a.S_pad + tile * 16 + sl];
    mfma_product<NW>(Pf, b, lane, E);
    return;
  }
  ecnt = 0;
  const int c = (int)a.codes_tile[((size_t)tile * a.L + ce.y) * 16 + sl];
  if (!__any(c < 0)) {  // column gather, [code][w][g][r] = P[16w + 4r + g][code]
    const double *Pg = a.PTg + (size_t)ce.y * DP * DP;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const unsigned off = (unsigned)((c * NW + w) * 16 + g * 4) * 8u;
      const f64x2 v0 = ld16(Pg, off), v1 = ld16(Pg, off + 16u);
      E[4 * w] = v0[0], E[4 * w + 1] = v0[1], E[4 * w + 2] = v1[0], E[4 * w + 3] = v1[1];
    }
  } else {  // ambiguity codes in this tile: product with the resolution vectors
    double lv[NKK];
    leaf_vec<NKK>(a, c, g, lv);
    mfma_product<NW>(Pf, lv, lane, E);
  }
}

struct MargNucArgs {
  const int4 *prog;
  int n_prog, L, S, S_pad, maxk, which, first;
  double w;
  const double *P;           // this class: [B][16] row-major
  const int16_t *codes;      // [L][S_pad]
  const double *ambig;       // [n_ambig][4]
  const double *pi;          // [4]
  const double *partials;    // this class: [I][4][S_pad]
  const int32_t *counts;     // this class: [I][S_pad]
  double *U;                 // [I][4][S_pad]
  int32_t *Ucnt;             // [I][S_pad]
  double *work;              // [2 maxk][4][S_pad]
  int32_t *wcnt;             // [2 maxk][S_pad]
  double *acc;               // [rows][S][4]
  double *den;               // [rows][S_pad]
  int32_t *aexp;             // [rows][S_pad]
};

__device__ __forceinline__ void rescale4(double (&v)[4], int &cnt) {
  const double tot = (v[0] + v[1]) + (v[2] + v[3]);
  if (!(tot >= kScalerThreshold && tot <= kScalerUp)) {
    double sc;
    cnt += rescale_decision(tot, sc);
    for (int j = 0; j < 4; j++) v[j] *= sc;
  }
}

__device__ __forceinline__ void nuc_leaf_vec(const MargNucArgs &a, int c, double (&lv)[4]) {
  for (int j = 0; j < 4; j++) lv[j] = c >= 0 ? (j == c ? 1. : 0.) : a.ambig[(size_t)(-c - 1) * 4 + j];
}

}  // namespace
}  // namespace hyhip
