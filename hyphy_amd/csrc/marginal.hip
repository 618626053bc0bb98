// Marginal ancestral reconstruction in one pre-order ("outside") pass over the resident conditionals — the device
// counterpart of _LikelihoodFunction::RecoverAncestralSequencesMarginal (likefunc2.cpp:932-1120), which pins every internal
// node to each of its states in turn and re-evaluates the partition, I * (D - 1) evaluations (L * D more for DOLEAVES).
//
// Per rate class and pattern, with in_n the stored conditional of internal node n (a leaf: its state indicator or ambiguity
// vector) and E_c = P_c in_c the edge product of child c:
//   U_root = pi                                        (the root frequencies of the last evaluation)
//   V_p^{not c} = U_p * prod_{s in children(p), s != c} E_s,   U_c = P_c^T V_p^{not c}
//   internal n:  num_n(x) = in_n(x) U_n(x)  = (U_n * prod_s E_s)(x),  L_s = sum_x num_n(x)
//   leaf l:      num_l(x) = U_l(x),                                    L_s = sum_x U_l(x) leafvec_l(x)
//   support = sum_c w_c num_c / sum_c w_c L_{s,c}   (classes combined by their 2^64 exponents, as mix_categories_kernel does)
// The sibling products come from a prefix pass (prefix product stored per child, edge products stored beside it) and a suffix
// pass in reverse child order: every edge product is formed once, every needed transposed product once.
//
// Decomposition (MFMA path, every state count but 4 — 2..64): one wave per 16-pattern tile walks the host-compiled pre-order program (plan_marginal
// below).  Vectors live in the fragment layout (common.h), so elementwise products are lane-local and the MFMA's C/D image of
// a product is the B operand of the next one.  The outside vectors and their exponents go to a scratch block shaped like one
// class of the partials ([I][ntiles][TILE] + [I][S_pad]); the prefix / edge products of the children of the node being walked
// go to a per-tile work area ([ntiles][2 * max children][TILE]).  A tile is owned by one wave: no synchronisation.
// 4 states: one thread per pattern, the same walk over the [I][4][S_pad] plane layout.
// Classes run one after another (one launch each), accumulating into the output block [rows][S][D] with a denominator and an
// exponent per (row, pattern); a last kernel normalises in place and picks the MAP state.
#include "devutil.h"
#include "outside.h"
#include "partition.h"

using namespace hyhip;

namespace hyhip {
namespace {

// add w * num (exponent e) to the accumulated support of `row`; den = sum of num * lv over the states
template <int NKK>
__device__ __forceinline__ void accumulate(const MargArgs &a, int row, int site, int g, const double (&num)[NKK], double den, int e) {
  if (site >= a.S) return;
  double *out = a.acc + ((size_t)row * a.S + site) * a.D;
  const size_t q = (size_t)row * a.S_pad + site;
  if (a.first) {
#pragma unroll
    for (int kk = 0; kk < NKK; kk++)
      if (4 * kk + g < a.D) out[4 * kk + g] = a.w * num[kk];
    if (g == 0) {
      a.den[q] = a.w * den;
      a.aexp[q] = e;
    }
    return;
  }
  const int e_old = a.aexp[q];
  const double d_old = a.den[q];
  const int e_new = min(e_old, e);  // (true value = stored * 2^(-64 e): the smaller exponent is the larger scale)
  const double f_old = ldexp(1.0, -64 * (e_old - e_new)), f_new = a.w * ldexp(1.0, -64 * (e - e_new));
#pragma unroll
  for (int kk = 0; kk < NKK; kk++)
    if (4 * kk + g < a.D) out[4 * kk + g] = out[4 * kk + g] * f_old + num[kk] * f_new;
  if (g == 0) {
    a.den[q] = d_old * f_old + den * f_new;
    a.aexp[q] = e_new;
  }
}

template <int NW>
__global__ __launch_bounds__(64) void marginal_mfma_kernel(MargArgs a) {
  constexpr int NKK = 4 * NW, TILE = NKK * 64;
  const int lane = threadIdx.x, g = lane >> 4, sl = lane & 15;
  const int tile = blockIdx.x, site = tile * 16 + sl;
  double *work = a.work + (size_t)tile * 2 * a.maxk * TILE;
  int32_t *wcnt = a.wcnt + (size_t)tile * 2 * a.maxk * 16;
  for (int pc = 0; pc < a.n_prog;) {
    const int4 h = a.prog[pc];
    const int node = h.y, k = h.z;
    double pre[NKK];
    int pcnt = 0;
    if (h.w) {  // the root: U = pi
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) pre[kk] = a.pi[4 * kk + g];
    } else {
      ld_vec<NKK>(a.U + ((size_t)node * a.ntiles + tile) * TILE, lane, pre);
      pcnt = a.Ucnt[(size_t)node * a.S_pad + site];
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
    if (a.which == 0) {  // in_n * U_n
      double t = 0.;
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) t += pre[kk];
      accumulate<NKK>(a, node, site, g, pre, row_sum4(t), pcnt);
    }
    // suffix pass, children in reverse order
    double suf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) suf[kk] = 1.;
    int scnt = 0;
    for (int i = k - 1; i >= 0; i--) {
      const int4 ce = a.prog[pc + 1 + i];
      if (ce.z >= 0 || a.which == 1) {
        double V[NKK], U[NKK];
        ld_vec<NKK>(work + (size_t)(2 * i) * TILE, lane, V);
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) V[kk] *= suf[kk];
        int vcnt = wcnt[(2 * i) * 16 + sl] + scnt;
        rescale_vec<NKK>(V, vcnt);
        mfma_product<NW>(a.PT + (size_t)ce.y * 16 * NW * 16 * NW, V, lane, U);
        if (ce.z >= 0) {
          rescale_vec<NKK>(U, vcnt);
          st_vec<NKK>(a.U + ((size_t)ce.z * a.ntiles + tile) * TILE, lane, U);
          a.Ucnt[(size_t)ce.z * a.S_pad + site] = vcnt;
        } else {  // leaf (DOLEAVES): U_l / sum_y U_l(y) leafvec_l(y)
          const int c = (int)a.codes_tile[((size_t)tile * a.L + ce.y) * 16 + sl];
          double lv[NKK];
          leaf_vec<NKK>(a, c, g, lv);
          double t = 0.;
#pragma unroll
          for (int kk = 0; kk < NKK; kk++) t += U[kk] * lv[kk];
          accumulate<NKK>(a, ce.y, site, g, U, row_sum4(t), vcnt);
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

// 4 states: one thread per pattern (argument block and helpers: outside.h)
__device__ __forceinline__ void nuc_accumulate(const MargNucArgs &a, int row, int s, const double (&num)[4], double den, int e) {
  if (s >= a.S) return;
  double *out = a.acc + ((size_t)row * a.S + s) * 4;
  const size_t q = (size_t)row * a.S_pad + s;
  if (a.first) {
    for (int j = 0; j < 4; j++) out[j] = a.w * num[j];
    a.den[q] = a.w * den;
    a.aexp[q] = e;
    return;
  }
  const int e_old = a.aexp[q], e_new = min(e_old, e);
  const double f_old = ldexp(1.0, -64 * (e_old - e_new)), f_new = a.w * ldexp(1.0, -64 * (e - e_new));
  for (int j = 0; j < 4; j++) out[j] = out[j] * f_old + num[j] * f_new;
  a.den[q] = a.den[q] * f_old + den * f_new;
  a.aexp[q] = e_new;
}

__global__ __launch_bounds__(256) void marginal_nuc_kernel(MargNucArgs a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.S_pad) return;
  const size_t SP = a.S_pad;
  for (int pc = 0; pc < a.n_prog;) {
    const int4 h = a.prog[pc];
    const int node = h.y, k = h.z;
    double pre[4];
    int pcnt = 0;
    if (h.w) {
      for (int j = 0; j < 4; j++) pre[j] = a.pi[j];
    } else {
      for (int j = 0; j < 4; j++) pre[j] = a.U[((size_t)node * 4 + j) * SP + s];
      pcnt = a.Ucnt[(size_t)node * SP + s];
    }
    for (int i = 0; i < k; i++) {
      const int4 ce = a.prog[pc + 1 + i];
      const double *P = a.P + (size_t)ce.y * 16;
      double in[4], E[4];
      int ecnt = 0;
      if (ce.z >= 0) {
        for (int j = 0; j < 4; j++) in[j] = a.partials[((size_t)ce.z * 4 + j) * SP + s];
        ecnt = a.counts[(size_t)ce.z * SP + s];
      } else {
        nuc_leaf_vec(a, (int)a.codes[(size_t)ce.y * SP + s], in);
      }
      for (int x = 0; x < 4; x++) E[x] = P[4 * x] * in[0] + P[4 * x + 1] * in[1] + P[4 * x + 2] * in[2] + P[4 * x + 3] * in[3];
      for (int j = 0; j < 4; j++) {
        a.work[((size_t)(2 * i) * 4 + j) * SP + s] = pre[j];
        a.work[((size_t)(2 * i + 1) * 4 + j) * SP + s] = E[j];
        pre[j] *= E[j];
      }
      a.wcnt[(size_t)(2 * i) * SP + s] = pcnt;
      a.wcnt[(size_t)(2 * i + 1) * SP + s] = ecnt;
      pcnt += ecnt;
      rescale4(pre, pcnt);
    }
    if (a.which == 0) nuc_accumulate(a, node, s, pre, (pre[0] + pre[1]) + (pre[2] + pre[3]), pcnt);
    double suf[4] = {1., 1., 1., 1.};
    int scnt = 0;
    for (int i = k - 1; i >= 0; i--) {
      const int4 ce = a.prog[pc + 1 + i];
      if (ce.z >= 0 || a.which == 1) {
        const double *P = a.P + (size_t)ce.y * 16;
        double V[4], U[4];
        for (int j = 0; j < 4; j++) V[j] = a.work[((size_t)(2 * i) * 4 + j) * SP + s] * suf[j];
        int vcnt = a.wcnt[(size_t)(2 * i) * SP + s] + scnt;
        rescale4(V, vcnt);
        for (int y = 0; y < 4; y++) U[y] = P[y] * V[0] + P[4 + y] * V[1] + P[8 + y] * V[2] + P[12 + y] * V[3];
        if (ce.z >= 0) {
          rescale4(U, vcnt);
          for (int j = 0; j < 4; j++) a.U[((size_t)ce.z * 4 + j) * SP + s] = U[j];
          a.Ucnt[(size_t)ce.z * SP + s] = vcnt;
        } else {
          double lv[4];
          nuc_leaf_vec(a, (int)a.codes[(size_t)ce.y * SP + s], lv);
          nuc_accumulate(a, ce.y, s, U, (U[0] * lv[0] + U[1] * lv[1]) + (U[2] * lv[2] + U[3] * lv[3]), vcnt);
        }
      }
      if (i > 0) {
        for (int j = 0; j < 4; j++) suf[j] *= a.work[((size_t)(2 * i + 1) * 4 + j) * SP + s];
        scnt += a.wcnt[(size_t)(2 * i + 1) * SP + s];
        rescale4(suf, scnt);
      }
    }
    pc += 1 + k;
  }
}

// support = accumulated numerator / denominator, in place; MAP state (first maximum) and its support
__global__ __launch_bounds__(256) void marginal_finish_kernel(double *__restrict__ acc, const double *__restrict__ den, int rows, int S,
                                                              int S_pad, int D, int32_t *__restrict__ map_state,
                                                              double *__restrict__ map_support) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)rows * S) return;
  const size_t row = t / S, s = t - row * S;
  const double inv = 1.0 / den[row * S_pad + s];
  double *v = acc + t * D;
  double best = -1.;
  int arg = 0;
  for (int j = 0; j < D; j++) {
    const double x = v[j] * inv;
    v[j] = x;
    if (x > best) best = x, arg = j;
  }
  map_state[t] = arg;
  map_support[t] = best;
}

}  // namespace

// The pre-order program over the partition's own tree: per internal node (root first, every node after its parent) a header and
// one entry per child, in ascending node-code order.  Returns the entries; *maxk_out = most children of a node.
std::vector<int4> plan_marginal_program(int64_t L, int64_t I, const int64_t *parents /* [L+I] internal index of the parent */,
                                       int *maxk_out) {
  std::vector<std::vector<int>> ch((size_t)I);
  for (int64_t c = 0; c < L + I - 1; c++) ch[(size_t)parents[c]].push_back((int)c);
  std::vector<int4> prog;
  int maxk = 1;
  std::vector<int> stack{(int)(I - 1)};
  while (!stack.empty()) {
    const int n = stack.back();
    stack.pop_back();
    const std::vector<int> &k = ch[(size_t)n];
    maxk = std::max(maxk, (int)k.size());
    prog.push_back(make_int4(0, n, (int)k.size(), n == I - 1 ? 1 : 0));
    for (size_t i = 0; i < k.size(); i++) prog.push_back(make_int4(1, k[i], k[i] >= L ? (int)(k[i] - L) : -1, (int)i));
    for (size_t i = k.size(); i-- > 0;)
      if (k[i] >= L) stack.push_back((int)(k[i] - L));
  }
  if (maxk_out) *maxk_out = maxk;
  return prog;
}

}  // namespace hyhip

extern "C" {

int64_t hyphy_hip_plan_marginal(int64_t L, int64_t I, const int64_t *flat_parents, int64_t *out, int64_t cap) {
  if (L < 1 || I < 1 || !flat_parents) return fail("plan_marginal: bad arguments");
  for (int64_t c = 0; c < L + I - 1; c++)
    if (flat_parents[c] < 0 || flat_parents[c] >= I) return fail("plan_marginal: parent out of range");
  if (flat_parents[L + I - 1] >= 0) return fail("plan_marginal: the root (last node) must have no parent");
  int maxk = 0;
  const std::vector<int4> prog = plan_marginal_program(L, I, flat_parents, &maxk);
  const int64_t words = 2 + 4 * (int64_t)prog.size();
  if (!out || cap < words) return -words;
  out[0] = (int64_t)prog.size();
  out[1] = maxk;
  for (size_t e = 0; e < prog.size(); e++) {
    out[2 + 4 * e] = prog[e].x;
    out[3 + 4 * e] = prog[e].y;
    out[4 + 4 * e] = prog[e].z;
    out[5 + 4 * e] = prog[e].w;
  }
  return words;
}

int hyphy_hip_marginal_ancestral(hyphy_hip_partition *p, int64_t which, const double *weights, double *support_out,
                                 int64_t *map_state_out, double *map_support_out) {
  if (!p) return fail("marginal_ancestral: partition == NULL");
  if (which != 0 && which != 1) return fail("marginal_ancestral: which must be 0 (internal nodes) or 1 (leaves)");
  if (p->pin_node >= 0) return fail("marginal_ancestral: a node's states are pinned (clear the pin first)");
  const int C = (int)p->C;
  if (C > 1 && !weights) return fail("marginal_ancestral: class weights are required when C > 1");
  for (int c = 0; c < C; c++)
    if (!p->initialized[c] || p->cached_pi.size() != (size_t)p->D)
      return fail("marginal_ancestral: rate class " + std::to_string(c) + " has not been evaluated");
  if (finish_pending_async(p)) return -1;
  for (int c = 0; c < C; c++)
    if (ensure_resident(p, c)) return -1;
  // (the pass reads the plain tree's persisted copies.  When ensure_resident has to restore them, its persisting pass switches the
  //  partition to the plain view and marks the class tables stale, as before a branch-cache build; the next evaluation switches back)
  const int64_t D = p->D, L = p->L, I = p->I, B = p->B, S = p->S;
  const int DP = p->DP, NW = p->NW;
  const int64_t rows = which == 0 ? I : L;
  if (p->marg_prog.empty()) p->marg_prog = plan_marginal_program(L, I, p->parents.data(), &p->marg_maxk);
  const std::vector<int4> &prog = p->marg_prog;
  const int maxk = p->marg_maxk;
  std::vector<double> pi_pad((size_t)(p->nuc ? 4 : DP), 0.);
  for (int64_t j = 0; j < D; j++) pi_pad[(size_t)j] = p->cached_pi[(size_t)j];
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    const size_t node_stride = p->nuc ? (size_t)4 * s.S_pad : (size_t)s.ntiles * 16 * DP;
    if (!s.marg_U) {  // scratch of the pass, kept until the partition is destroyed; published only when every block is there
      const size_t work = p->nuc ? (size_t)2 * maxk * 4 * s.S_pad : (size_t)s.ntiles * 2 * maxk * 16 * DP;
      const size_t wcnt = p->nuc ? (size_t)2 * maxk * s.S_pad : (size_t)s.ntiles * 2 * maxk * 16;
      const size_t bytes[7] = {(size_t)I * node_stride * sizeof(double), (size_t)I * s.S_pad * sizeof(int32_t), work * sizeof(double),
                               wcnt * sizeof(int32_t), prog.size() * sizeof(int4), pi_pad.size() * sizeof(double),
                               p->nuc ? 0 : (size_t)B * DP * DP * sizeof(double)};
      void *blk[7] = {};
      hipError_t ae = hipSuccess;
      for (int k = 0; k < 7 && ae == hipSuccess; k++)
        if (bytes[k]) ae = pool_malloc(&blk[k], bytes[k]);
      if (ae == hipSuccess) ae = hipMemcpy(blk[4], prog.data(), bytes[4], hipMemcpyHostToDevice);
      if (ae != hipSuccess) {
        for (void *b : blk)
          if (b) pool_free(b);
        return fail(std::string("marginal_ancestral: scratch: ") + hipGetErrorString(ae));
      }
      s.marg_U = (double *)blk[0], s.marg_Ucnt = (int32_t *)blk[1], s.marg_work = (double *)blk[2], s.marg_wcnt = (int32_t *)blk[3];
      s.marg_prog = (int4 *)blk[4], s.marg_pi = (double *)blk[5], s.marg_PT = (double *)blk[6];
      for (size_t b : bytes) s.dev_bytes += b;
    }
    HIPCHK(hipMemcpy(s.marg_pi, pi_pad.data(), pi_pad.size() * sizeof(double), hipMemcpyHostToDevice));
    double *acc = nullptr, *den = nullptr, *msup = nullptr;
    int32_t *aexp = nullptr, *mst = nullptr;
    const size_t nrs = (size_t)rows * s.S;
    hipError_t e = pool_malloc((void **)&acc, std::max<size_t>(1, nrs * D) * sizeof(double));
    if (e == hipSuccess) e = pool_malloc((void **)&den, (size_t)rows * s.S_pad * sizeof(double));
    if (e == hipSuccess) e = pool_malloc((void **)&aexp, (size_t)rows * s.S_pad * sizeof(int32_t));
    if (e == hipSuccess) e = pool_malloc((void **)&msup, std::max<size_t>(1, nrs) * sizeof(double));
    if (e == hipSuccess) e = pool_malloc((void **)&mst, std::max<size_t>(1, nrs) * sizeof(int32_t));
    for (int c = 0; c < C && e == hipSuccess; c++) {
      const double w = C > 1 ? weights[c] : 1.0;
      if (p->nuc) {
        MargNucArgs a;
        a.prog = s.marg_prog;
        a.n_prog = (int)prog.size();
        a.L = (int)L, a.S = (int)s.S, a.S_pad = s.S_pad, a.maxk = maxk, a.which = (int)which, a.first = c == 0;
        a.w = w;
        a.P = s.Prow + (size_t)c * B * 16;
        a.codes = s.codes;
        a.ambig = s.ambig;
        a.pi = s.marg_pi;
        a.partials = s.partials + (size_t)c * s.partial_stride;
        a.counts = s.counts + (size_t)c * I * s.S_pad;
        a.U = s.marg_U, a.Ucnt = s.marg_Ucnt, a.work = s.marg_work, a.wcnt = s.marg_wcnt;
        a.acc = acc, a.den = den, a.aexp = aexp;
        hipLaunchKernelGGL(marginal_nuc_kernel, dim3((unsigned)((s.S_pad + 255) / 256)), dim3(256), 0, s.stream, a);
      } else {
        MargArgs a;
        a.prog = s.marg_prog;
        a.n_prog = (int)prog.size();
        a.NW = NW, a.L = (int)L, a.S = (int)s.S, a.S_pad = s.S_pad, a.ntiles = s.ntiles, a.maxk = maxk, a.which = (int)which;
        a.first = c == 0, a.D = (int)D;
        a.w = w;
        a.Pfrag = s.Pfrag + (size_t)c * B * DP * DP;
        a.PTg = s.PTg + (size_t)c * B * DP * DP;
        a.PT = s.marg_PT;
        a.codes_tile = s.codes_tile;
        a.ambig = s.ambig;
        a.pi = s.marg_pi;
        a.partials = s.partials + (size_t)c * s.partial_stride;
        a.counts = s.counts + (size_t)c * I * s.S_pad;
        a.U = s.marg_U, a.Ucnt = s.marg_Ucnt, a.work = s.marg_work, a.wcnt = s.marg_wcnt;
        a.acc = acc, a.den = den, a.aexp = aexp;
        hipLaunchKernelGGL(marg_transpose_kernel, dim3((unsigned)B), dim3(256), 0, s.stream, a.Pfrag, a.PTg, s.marg_PT, NW, (int)L);
        const dim3 grid((unsigned)s.ntiles), block(64);
        switch (NW) {
          case 1: hipLaunchKernelGGL(marginal_mfma_kernel<1>, grid, block, 0, s.stream, a); break;
          case 2: hipLaunchKernelGGL(marginal_mfma_kernel<2>, grid, block, 0, s.stream, a); break;
          case 3: hipLaunchKernelGGL(marginal_mfma_kernel<3>, grid, block, 0, s.stream, a); break;
          default: hipLaunchKernelGGL(marginal_mfma_kernel<4>, grid, block, 0, s.stream, a); break;
        }
      }
      e = hipGetLastError();
    }
    if (e == hipSuccess && nrs > 0) {
      hipLaunchKernelGGL(marginal_finish_kernel, dim3((unsigned)((nrs + 255) / 256)), dim3(256), 0, s.stream, acc, den, (int)rows,
                         (int)s.S, s.S_pad, (int)D, mst, msup);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    // -> the caller's pattern order: out[row][caller pattern][...]
    if (e == hipSuccess && support_out) {
      if (p->perm.empty()) {
        e = hipMemcpy2D(support_out + s.s0 * D, (size_t)S * D * sizeof(double), acc, (size_t)s.S * D * sizeof(double),
                        (size_t)s.S * D * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost);
      } else {
        std::vector<double> tmp((size_t)s.S * D);
        for (int64_t r = 0; r < rows && e == hipSuccess; r++) {
          e = hipMemcpy(tmp.data(), acc + (size_t)r * s.S * D, tmp.size() * sizeof(double), hipMemcpyDeviceToHost);
          for (int64_t k = 0; k < s.S; k++)
            memcpy(support_out + ((size_t)r * S + p->perm[s.s0 + k]) * D, tmp.data() + (size_t)k * D, (size_t)D * sizeof(double));
        }
      }
    }
    if (e == hipSuccess && (map_state_out || map_support_out)) {
      std::vector<int32_t> hs(nrs);
      std::vector<double> hv(nrs);
      e = hipMemcpy(hs.data(), mst, nrs * sizeof(int32_t), hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(hv.data(), msup, nrs * sizeof(double), hipMemcpyDeviceToHost);
      for (int64_t r = 0; r < rows && e == hipSuccess; r++)
        for (int64_t k = 0; k < s.S; k++) {
          const size_t o = (size_t)r * S + caller_pattern(p, s.s0 + k);
          if (map_state_out) map_state_out[o] = hs[(size_t)r * s.S + k];
          if (map_support_out) map_support_out[o] = hv[(size_t)r * s.S + k];
        }
    }
    for (void *d : {(void *)acc, (void *)den, (void *)aexp, (void *)msup, (void *)mst})
      if (d) pool_free_sync(d);
    if (e != hipSuccess) return fail(std::string("marginal_ancestral: ") + hipGetErrorString(e));
  }
  return 0;
}

}  // extern "C"
