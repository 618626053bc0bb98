// The pre-order ("outside") walk over the resident conditionals, once per layout: outside_walk<NW, Sink> (fragment layout, one wave
// per 16-pattern tile) and outside_walk_nuc<Sink> (4 states, plane layout, one thread per pattern).  Both walk the host-compiled
// program (plan_marginal_program): per node load U_p (the root: pi), a prefix pass over the children into the work area (prefix
// product and edge product per child), a suffix pass in reverse child order, V_c = prefix * suffix, U_c = P_c^T V_c, every vector
// rescaled by 2^64 where the pruning pass would.  What a pass keeps is its sink's business — a small struct, inlined, with hooks
//   node      a node's finished prefix product (= in_n * U_n) and its exponent
//   leaves    whether the V of a leaf child is wanted at all
//   branch    a child's rescaled V and its exponent
//   leaf      a leaf's U = P_l^T V_l (not rescaled), formed only when the sink's kLeafProduct is set
// in two forms each, told apart by their arguments: (tile, lane, fragment vector) and (pattern, 4 values).  The marginal
// reconstruction (marginal.hip) accumulates support in `node` / `leaf`; the branch trials (trials.hip), the branch derivatives
// (deriv.hip) and the gradient (grad.hip) store V in `branch`, through the OutsideStore sink and its two kernels, launched by the host
// driver they share (outside_pass.h).  What all four do on the host before a launch is here too: check_pass_ready, begin_outside.
// U, Ucnt, work and wcnt are indexed by (tile or pattern within the chunk, size of the chunk): a chunk that is the whole shard gives
// the [I][ntiles][TILE] / [I][S_pad] shapes of the partials.
// The device side of those three passes' phase 2 is at the end of this file, once: OutsideSlice (what their kernels get by value beside
// the WalkArgs), the branch prologue (branch_entry, branch_outside / nuc_branch_outside: the branch, its V and exponent from the chunk's blocks;
// child_vec / nuc_child_vec: the conditional below it; edge_product, mat4_vec: its edge product), the record epilogue's wave sums
// (wave_sum, wave_or) and align_exponents.  gfx950 only.
#pragma once
#include "devutil.h"
#include "partition.h"

namespace hyhip {
namespace {

// program entries (int4): a node header (0, internal index, children, 1 for the root), then one entry per child
// (1, child node code = matrix slot, child internal index or -1 for a leaf, position among the children)
struct WalkArgs {  // what the walks read; "tile" below: 16 patterns (4 states: ONE pattern)
  const int4 *prog;
  int n_prog;
  int L, S_pad, ntiles, maxk;
  int first, count, chunk;   // first tile of the launch, its tiles, tiles the blocks U .. wcnt are shaped for
  const double *Pfrag;       // [B][NW][NKK*64] A-operand images of this class
  const double *PTg;         // [B][DP][NW][4][4] column-gather images (leaf edges)
  const double *PT;          // [B][NW][NKK*64] A-operand images of the TRANSPOSED matrices (scratch of the pass)
  const double *Prow;        // 4 states: [B][16] row-major
  const int16_t *codes_tile; // [ntiles][L][16]
  const int16_t *codes;      // 4 states: [L][S_pad]
  const double *ambig;       // [n_ambig][DP]
  const double *pi;          // [DP]
  const double *partials;    // this class: [I][ntiles][TILE]       (4 states: [I][4][S_pad])
  const int32_t *counts;     // this class: [I][S_pad]
  double *U;                 // [I][chunk][TILE] outside vectors     (4 states: [I][4][chunk])
  int32_t *Ucnt;             // [I][chunk][16]                       (4 states: [I][chunk])
  double *work;              // [chunk][2 maxk][TILE]                (4 states: [2 maxk][4][chunk])
  int32_t *wcnt;             // [chunk][2 maxk][16]                  (4 states: [2 maxk][chunk])
};

// What phase 2 of a pass that keeps every branch's V (outside_pass.h) reads beside the WalkArgs: the chunk, the class and the slice of
// the branch grid of one launch.  Here and not with the driver that fills it, because the branch prologue below reads it.
struct OutsideSlice {
  int tile0, ct, nt;            // first tile of the chunk, tiles V and Vcnt are shaped for, tiles of the chunk that exist
  int C, cls, first, last, b0;  // classes, class of this launch, it is the first / the last one, first branch of the grid
  double w;                     // weight of this class (1 when C == 1)
  const int *branch;            // [branches with a request] node codes
  const int *off, *idx;         // requests of branch k: idx[off[k] .. off[k + 1])
  const double *V;              // phase 1's blocks of this chunk
  const int32_t *Vcnt;
  const double *freq;           // [S_pad] pattern frequencies
  int part_stride;              // per-(request, tile) records: [n][part_stride]
};

struct WalkScratch {  // what a pass brings to the walk: the uploaded program and pi, and the blocks the walk writes
  const int4 *prog;
  const double *pi;
  double *PT, *U;
  int32_t *Ucnt;
  double *work;
  int32_t *wcnt;
};

// the block for class c of shard s over the pass's scratch, with the whole shard as the chunk
inline WalkArgs walk_args(const hyphy_hip_partition *p, const Shard &s, int c, const WalkScratch &w) {
  const size_t img = (size_t)c * p->B * p->DP * p->DP;
  WalkArgs a = {};
  a.prog = w.prog, a.pi = w.pi, a.PT = w.PT, a.U = w.U, a.Ucnt = w.Ucnt, a.work = w.work, a.wcnt = w.wcnt;
  a.n_prog = (int)p->marg_prog.size();
  a.L = (int)p->L, a.S_pad = s.S_pad, a.ntiles = s.ntiles, a.maxk = p->marg_maxk;
  a.count = a.chunk = p->nuc ? s.S_pad : s.ntiles;
  if (p->nuc) a.Prow = s.Prow + (size_t)c * p->B * 16;
  else a.Pfrag = s.Pfrag + img, a.PTg = s.PTg + img;
  a.codes_tile = s.codes_tile, a.codes = s.codes, a.ambig = s.ambig;
  a.partials = s.partials + (size_t)c * s.partial_stride;
  a.counts = s.counts + (size_t)c * p->I * s.S_pad;
  return a;
}

// ---- what every pass over the walk does on the host before it launches anything ----
// pinned states, class weights, every class evaluated (`pre`: the entry point's name and ": ")
inline int check_pass_ready(const hyphy_hip_partition *p, const std::string &pre, const double *weights) {
  if (check_unpinned(p, pre)) return -1;
  if (p->C > 1 && !weights) return fail(pre + "class weights are required when C > 1");
  return check_evaluated(p, pre);
}

// Pending work finished, every class resident, the program planned (once per partition), pi padded.
// (the pass reads the plain tree's persisted copies.  When ensure_resident has to restore them, its persisting pass switches the
//  partition to the plain view and marks the class tables stale, as before a branch-cache build; the next evaluation switches back)
inline int begin_outside(hyphy_hip_partition *p, std::vector<double> &pi) {
  if (finish_pending_async(p)) return -1;
  for (int c = 0; c < (int)p->C; c++)
    if (ensure_resident(p, c)) return -1;
  if (p->marg_prog.empty()) p->marg_prog = plan_marginal_program(p->L, p->I, p->parents.data(), &p->marg_maxk);
  pi = padded_pi(p);
  return 0;
}

// transposed A-operand images M[r][c] = P[c][r] of every branch of one class: leaves from the column-gather image (the only
// image the exponential writes for a leaf without ambiguity codes), internal nodes from the A-operand image
__global__ __launch_bounds__(256) void marg_transpose_kernel(const double *__restrict__ Pfrag, const double *__restrict__ PTg,
                                                             double *__restrict__ PT, int NW, int L) {
  const int DP = 16 * NW, TILE = DP * 16;
  const int b = blockIdx.x;
  const double *src = Pfrag + (size_t)b * DP * DP, *gsrc = PTg + (size_t)b * DP * DP;
  double *dst = PT + (size_t)b * DP * DP;
  for (int idx = threadIdx.x; idx < DP * DP; idx += blockDim.x) {
    int r, c;  // M[r][c] = P[c][r]
    frag_image_rc(idx, NW, r, c);
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
__device__ __forceinline__ void leaf_vec(const WalkArgs &a, int c, int g, double (&lv)[NKK]) {
  const int DP = 4 * NKK;
#pragma unroll
  for (int kk = 0; kk < NKK; kk++) lv[kk] = c >= 0 ? (4 * kk + g == c ? 1. : 0.) : a.ambig[(size_t)(-c - 1) * DP + 4 * kk + g];
}

// ... one element of it, `state` of DP (leaf_vec keeps its own text: a call here moves instructions in marginal.hip's kernels)
template <int DP>
__device__ __forceinline__ double leaf_value(const WalkArgs &a, int c, int state) {
  return c >= 0 ? (state == c ? 1. : 0.) : a.ambig[(size_t)(-c - 1) * DP + state];
}

// the conditional below child entry ce at this lane's states, `in`, and its exponent: stored partial or leaf vector; returns the
// leaf's code (0 for an internal child)
template <int NKK>
__device__ __forceinline__ int child_vec(const WalkArgs &a, const int4 &ce, int tile, int lane, double (&in)[NKK], int &ecnt) {
  const int sl = lane & 15;
  ecnt = 0;
  if (ce.z >= 0) {
    ld_vec<NKK>(a.partials + ((size_t)ce.z * a.ntiles + tile) * (NKK * 64), lane, in);
    ecnt = a.counts[(size_t)ce.z * a.S_pad + tile * 16 + sl];
    return 0;
  }
  const int c = (int)a.codes_tile[((size_t)tile * a.L + ce.y) * 16 + sl];
  leaf_vec<NKK>(a, c, lane >> 4, in);
  return c;
}

// edge product E of child entry ce and its 2^64 exponent
template <int NW>
__device__ __forceinline__ void edge_product(const WalkArgs &a, const int4 &ce, int tile, int lane, double (&E)[4 * NW], int &ecnt) {
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
  if (!__any(c < 0)) {
    gather_column<NW>(a.PTg + (size_t)ce.y * DP * DP, c, g, E);
  } else {  // ambiguity codes in this tile: product with the resolution vectors
    double lv[NKK];
    leaf_vec<NKK>(a, c, g, lv);
    mfma_product<NW>(Pf, lv, lane, E);
  }
}

// the walk of one tile
template <int NW, typename Sink>
__device__ __forceinline__ void outside_walk(const WalkArgs &a, Sink &sink) {
  constexpr int NKK = 4 * NW, TILE = NKK * 64;
  const int lane = threadIdx.x, sl = lane & 15;
  const int lt = blockIdx.x, tile = a.first + lt;
  double *work = a.work + (size_t)lt * 2 * a.maxk * TILE;
  int32_t *wcnt = a.wcnt + (size_t)lt * 2 * a.maxk * 16;
  for (int pc = 0; pc < a.n_prog;) {
    const int4 h = a.prog[pc];
    const int node = h.y, k = h.z;
    double pre[NKK];
    int pcnt = 0;
    if (h.w) {  // the root: U = pi
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) pre[kk] = a.pi[4 * kk + (lane >> 4)];
    } else {
      ld_vec<NKK>(a.U + ((size_t)node * a.chunk + lt) * TILE, lane, pre);
      pcnt = a.Ucnt[((size_t)node * a.chunk + lt) * 16 + sl];
    }
    // prefix pass: slot 2i = U_p * prod_{j < i} E_j, slot 2i + 1 = E_i
    for (int i = 0; i < k; i++) {
      const int4 ce = a.prog[pc + 1 + i];
      double E[NKK];
      int ecnt;
      edge_product<NW>(a, ce, tile, lane, E, ecnt);
      st_vec<NKK>(work + (size_t)(2 * i) * TILE, lane, pre);
      st_vec<NKK>(work + (size_t)(2 * i + 1) * TILE, lane, E);
      wcnt[(2 * i) * 16 + sl] = pcnt;  // (every lane of the pattern stores the same word: each reads back its own store)
      wcnt[(2 * i + 1) * 16 + sl] = ecnt;
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) pre[kk] *= E[kk];
      pcnt += ecnt;
      rescale_vec<NKK>(pre, pcnt);
    }
    sink.node(a, node, tile, lane, pre, pcnt);
    // suffix pass, children in reverse order
    double suf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) suf[kk] = 1.;
    int scnt = 0;
    for (int i = k - 1; i >= 0; i--) {
      const int4 ce = a.prog[pc + 1 + i];
      if (ce.z >= 0 || sink.leaves()) {
        double V[NKK];
        ld_vec<NKK>(work + (size_t)(2 * i) * TILE, lane, V);
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) V[kk] *= suf[kk];
        int vcnt = wcnt[(2 * i) * 16 + sl] + scnt;
        rescale_vec<NKK>(V, vcnt);
        sink.branch(a, ce.y, lt, lane, V, vcnt);
        if (ce.z >= 0 || Sink::kLeafProduct) {
          double U[NKK];
          mfma_product<NW>(a.PT + (size_t)ce.y * 16 * NW * 16 * NW, V, lane, U);
          if (ce.z >= 0) {
            rescale_vec<NKK>(U, vcnt);
            st_vec<NKK>(a.U + ((size_t)ce.z * a.chunk + lt) * TILE, lane, U);
            a.Ucnt[((size_t)ce.z * a.chunk + lt) * 16 + sl] = vcnt;
          } else {
            sink.leaf(a, ce.y, tile, lane, U, vcnt);
          }
        }
      }
      if (i > 0) {
        double E[NKK];
        ld_vec<NKK>(work + (size_t)(2 * i + 1) * TILE, lane, E);
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) suf[kk] *= E[kk];
        scnt += wcnt[(2 * i + 1) * 16 + sl];
        rescale_vec<NKK>(suf, scnt);
      }
    }
    pc += 1 + k;
  }
}

__device__ __forceinline__ void rescale4(double (&v)[4], int &cnt) {
  const double tot = (v[0] + v[1]) + (v[2] + v[3]);
  if (!(tot >= kScalerThreshold && tot <= kScalerUp)) {
    double sc;
    cnt += rescale_decision(tot, sc);
    for (int j = 0; j < 4; j++) v[j] *= sc;
  }
}

__device__ __forceinline__ void nuc_leaf_vec(const WalkArgs &a, int c, double (&lv)[4]) {
  for (int j = 0; j < 4; j++) lv[j] = leaf_value<4>(a, c, j);
}

// 4 states: the conditional below child entry ce at pattern s and its exponent: stored partial or leaf vector
__device__ __forceinline__ void nuc_child_vec(const WalkArgs &a, const int4 &ce, size_t s, double (&in)[4], int &ecnt) {
  const size_t SP = a.S_pad;
  ecnt = 0;
  if (ce.z >= 0) {
    for (int j = 0; j < 4; j++) in[j] = a.partials[((size_t)ce.z * 4 + j) * SP + s];
    ecnt = a.counts[(size_t)ce.z * SP + s];
  } else {
    nuc_leaf_vec(a, (int)a.codes[(size_t)ce.y * SP + s], in);
  }
}

// y = M x and y = M^T x of a row-major 4 x 4 matrix
__device__ __forceinline__ void mat4_vec(const double *M, const double (&x)[4], double (&y)[4]) {
  for (int i = 0; i < 4; i++) y[i] = M[4 * i] * x[0] + M[4 * i + 1] * x[1] + M[4 * i + 2] * x[2] + M[4 * i + 3] * x[3];
}
__device__ __forceinline__ void mat4t_vec(const double *M, const double (&x)[4], double (&y)[4]) {
  for (int i = 0; i < 4; i++) y[i] = M[i] * x[0] + M[4 + i] * x[1] + M[8 + i] * x[2] + M[12 + i] * x[3];
}
__device__ __forceinline__ double dot4(const double (&x)[4], const double (&y)[4]) {
  return (x[0] * y[0] + x[1] * y[1]) + (x[2] * y[2] + x[3] * y[3]);
}

// 4 states: the walk of one pattern (launch: 256 threads per workgroup, any grid that covers a.count)
template <typename Sink>
__device__ __forceinline__ void outside_walk_nuc(const WalkArgs &a, Sink &sink) {
  const int ls = blockIdx.x * blockDim.x + threadIdx.x;
  if (ls >= a.count) return;
  const size_t s = (size_t)a.first + ls, CS = (size_t)a.chunk;
  for (int pc = 0; pc < a.n_prog;) {
    const int4 h = a.prog[pc];
    const int node = h.y, k = h.z;
    double pre[4];
    int pcnt = 0;
    if (h.w) {
      for (int j = 0; j < 4; j++) pre[j] = a.pi[j];
    } else {
      for (int j = 0; j < 4; j++) pre[j] = a.U[((size_t)node * 4 + j) * CS + ls];
      pcnt = a.Ucnt[(size_t)node * CS + ls];
    }
    for (int i = 0; i < k; i++) {
      const int4 ce = a.prog[pc + 1 + i];
      double in[4], E[4];
      int ecnt;
      nuc_child_vec(a, ce, s, in, ecnt);
      mat4_vec(a.Prow + (size_t)ce.y * 16, in, E);
      for (int j = 0; j < 4; j++) {
        a.work[((size_t)(2 * i) * 4 + j) * CS + ls] = pre[j];
        a.work[((size_t)(2 * i + 1) * 4 + j) * CS + ls] = E[j];
        pre[j] *= E[j];
      }
      a.wcnt[(size_t)(2 * i) * CS + ls] = pcnt;
      a.wcnt[(size_t)(2 * i + 1) * CS + ls] = ecnt;
      pcnt += ecnt;
      rescale4(pre, pcnt);
    }
    sink.node(a, node, s, pre, pcnt);
    double suf[4] = {1., 1., 1., 1.};
    int scnt = 0;
    for (int i = k - 1; i >= 0; i--) {
      const int4 ce = a.prog[pc + 1 + i];
      if (ce.z >= 0 || sink.leaves()) {
        double V[4];
        for (int j = 0; j < 4; j++) V[j] = a.work[((size_t)(2 * i) * 4 + j) * CS + ls] * suf[j];
        int vcnt = a.wcnt[(size_t)(2 * i) * CS + ls] + scnt;
        rescale4(V, vcnt);
        sink.branch(a, ce.y, (size_t)ls, V, vcnt);
        if (ce.z >= 0 || Sink::kLeafProduct) {
          double U[4];
          mat4t_vec(a.Prow + (size_t)ce.y * 16, V, U);
          if (ce.z >= 0) {
            rescale4(U, vcnt);
            for (int j = 0; j < 4; j++) a.U[((size_t)ce.z * 4 + j) * CS + ls] = U[j];
            a.Ucnt[(size_t)ce.z * CS + ls] = vcnt;
          } else {
            sink.leaf(a, ce.y, s, U, vcnt);
          }
        }
      }
      if (i > 0) {
        for (int j = 0; j < 4; j++) suf[j] *= a.work[((size_t)(2 * i + 1) * 4 + j) * CS + ls];
        scnt += a.wcnt[(size_t)(2 * i + 1) * CS + ls];
        rescale4(suf, scnt);
      }
    }
    pc += 1 + k;
  }
}

// phase 1's sink: V_c and its exponent of every child, leaves included, into blocks of one chunk of tiles (a.chunk of them), indexed
// by the tile within the chunk.  A leaf's U is not formed.
struct OutsideStore {
  static constexpr bool kLeafProduct = false;
  double *V;      // [B][ct][TILE]   (4 states: [B][4][ct * 64])
  int32_t *Vcnt;  // [B][ct][16]     (4 states: [B][ct * 64])

  __device__ __forceinline__ bool leaves() const { return true; }
  template <int NKK>
  __device__ __forceinline__ void node(const WalkArgs &, int, int, int, const double (&)[NKK], int) const {}
  template <int NKK>
  __device__ __forceinline__ void branch(const WalkArgs &a, int c, int lt, int lane, const double (&v)[NKK], int vcnt) const {
    st_vec<NKK>(V + ((size_t)c * a.chunk + lt) * (NKK * 64), lane, v);
    Vcnt[((size_t)c * a.chunk + lt) * 16 + (lane & 15)] = vcnt;
  }
  template <int NKK>
  __device__ __forceinline__ void leaf(const WalkArgs &, int, int, int, const double (&)[NKK], int) const {}
  // 4 states
  __device__ __forceinline__ void node(const WalkArgs &, int, size_t, const double (&)[4], int) const {}
  __device__ __forceinline__ void branch(const WalkArgs &a, int c, size_t ls, const double (&v)[4], int vcnt) const {
    for (int j = 0; j < 4; j++) V[((size_t)c * 4 + j) * a.chunk + ls] = v[j];
    Vcnt[(size_t)c * a.chunk + ls] = vcnt;
  }
  __device__ __forceinline__ void leaf(const WalkArgs &, int, size_t, const double (&)[4], int) const {}
};

template <int NW>
__global__ __launch_bounds__(64) void outside_store_kernel(WalkArgs a, OutsideStore o) {
  outside_walk<NW>(a, o);
}

__global__ __launch_bounds__(256) void outside_store_nuc_kernel(WalkArgs a, OutsideStore o) { outside_walk_nuc(a, o); }

// ---- what phase 2 of a pass that kept every branch's V starts from and ends with (trials.hip, deriv.hip, grad.hip) ----
// branch bi of the slice as the child entry the program has for it (.y node code, .z internal index or -1)
__device__ __forceinline__ int4 branch_entry(const WalkArgs &a, const OutsideSlice &sl, int bi) {
  const int node = sl.branch[bi];
  return make_int4(1, node, node >= a.L ? node - a.L : -1, 0);
}
// where phase 1 left branch `node` at `tile`: its block among the chunk's, V [..][TILE] and Vcnt [..][16] alike
__device__ __forceinline__ size_t outside_index(const OutsideSlice &sl, int node, int tile) {
  return (size_t)node * sl.ct + (tile - sl.tile0);
}
// the entry, V and its exponent of branch bi at `tile`
template <int NKK>
__device__ __forceinline__ int4 branch_outside(const WalkArgs &a, const OutsideSlice &sl, int bi, int tile, int lane, double (&V)[NKK],
                                               int &vcnt) {
  const int4 ce = branch_entry(a, sl, bi);
  const size_t o = outside_index(sl, ce.y, tile);
  ld_vec<NKK>(sl.V + o * (NKK * 64), lane, V);
  vcnt = sl.Vcnt[o * 16 + (lane & 15)];
  return ce;
}
// 4 states: pattern `lane` of the wave's 64
__device__ __forceinline__ int4 nuc_branch_outside(const WalkArgs &a, const OutsideSlice &sl, int bi, int tile, int lane, double (&V)[4],
                                                   int &vcnt) {
  const int4 ce = branch_entry(a, sl, bi);
  const size_t ls = (size_t)(tile - sl.tile0) * 64 + lane, CS = (size_t)sl.ct * 64;
  for (int j = 0; j < 4; j++) V[j] = sl.V[((size_t)ce.y * 4 + j) * CS + ls];
  vcnt = sl.Vcnt[(size_t)ce.y * CS + ls];
  return ce;
}

// sum / OR over the W lanes around this one (16: the patterns of a tile within one state group; 64: the wave), xor-shuffles from W / 2 down
template <int W, typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
template <int W>
__device__ __forceinline__ int wave_or(int x) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) x |= __shfl_xor(x, off);
  return x;
}

// two values with 2^64 exponents e_old and e on the smaller exponent (the larger scale): that exponent and what each is multiplied by.
// (what an exact zero does to the mix is the caller's rule)
__device__ __forceinline__ int align_exponents(int e_old, int e, double &s_old, double &s_new) {
  const int e_new = min(e_old, e);
  s_old = ldexp(1.0, -64 * (e_old - e_new)), s_new = ldexp(1.0, -64 * (e - e_new));
  return e_new;
}

}  // namespace
}  // namespace hyhip
