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
// Decomposition: the walk is outside.h's — outside_walk<NW> (every state count but 4: one wave per 16-pattern tile over the
// host-compiled pre-order program, plan_marginal_program below, vectors in the fragment layout of common.h, so elementwise products
// are lane-local and the MFMA's C/D image of a product is the B operand of the next one) and outside_walk_nuc (4 states: one thread
// per pattern over the [I][4][S_pad] planes).  The kernels here are that walk with MargSink, which accumulates num_n at every node
// (which == 0) or num_l at every leaf (which == 1).  The chunk of the walk is the whole shard: the outside vectors and their
// exponents go to a scratch block shaped like one class of the partials ([I][ntiles][TILE] + [I][S_pad]), the prefix / edge
// products of the children of the node being walked to a per-tile work area ([ntiles][2 * max children][TILE]).  A tile is owned
// by one wave: no synchronisation.  That scratch stays with the shard (Shard::marg_*) until the partition is destroyed.
// Classes run one after another (one launch each), accumulating into the output block [rows][S][D] with a denominator and an
// exponent per (row, pattern); a last kernel normalises in place and picks the MAP state.  The output block and its companions are
// per-call pool blocks.
#include "devutil.h"
#include "outside.h"
#include "partition.h"

using namespace hyhip;

namespace hyhip {
namespace {

// The walk's sink: the support block [rows][S][D] of the call, with a denominator and a 2^64 exponent per (row, pattern), and which
// rows it has — the internal nodes (which == 0: `node`) or the leaves (which == 1: `leaf`, U_l / sum_y U_l(y) leafvec_l(y))
struct MargSink {
  static constexpr bool kLeafProduct = true;
  double w;        // weight of this class (1 when C == 1)
  int first;       // the first class: store, do not add
  int which, D, S;
  double *acc;     // [rows][S][D]
  double *den;     // [rows][S_pad]
  int32_t *aexp;   // [rows][S_pad]

  __device__ __forceinline__ bool leaves() const { return which == 1; }

  // add w * num (exponent e) to the accumulated support of `row`; den = sum of num * lv over the states.  A contribution whose
  // weighted denominator is exactly 0 (the pattern is impossible under this class, or the class has weight 0) is passed over, and a
  // stored denominator of 0 is overwritten: such a contribution's exponent says nothing (a zero vector is never rescaled), and under
  // the min rule it would scale the other classes by 2^(-64 x difference), to nothing from a difference of 17.  Every lane of a
  // pattern decides alike: dn is a row_sum4, and den[q] is read by all four lanes before lane g == 0 stores it.
  template <int NKK>
  __device__ __forceinline__ void add(const WalkArgs &a, int row, int site, int g, const double (&num)[NKK], double dn, int e) const {
    if (site >= S) return;
    double *out = acc + ((size_t)row * S + site) * D;
    const size_t q = (size_t)row * a.S_pad + site;
    const double wd = w * dn, d_old = first ? 0. : den[q];
    if (!(wd > 0.) && !first) return;
    if (!(d_old > 0.)) {
      const double f = wd > 0. ? w : 0.;
#pragma unroll
      for (int kk = 0; kk < NKK; kk++)
        if (4 * kk + g < D) out[4 * kk + g] = f * num[kk];
      if (g == 0) {
        den[q] = wd;
        aexp[q] = e;
      }
      return;
    }
    const int e_old = aexp[q];
    const int e_new = min(e_old, e);  // (true value = stored * 2^(-64 e): the smaller exponent is the larger scale)
    const double f_old = ldexp(1.0, -64 * (e_old - e_new)), f_new = w * ldexp(1.0, -64 * (e - e_new));
#pragma unroll
    for (int kk = 0; kk < NKK; kk++)
      if (4 * kk + g < D) out[4 * kk + g] = out[4 * kk + g] * f_old + num[kk] * f_new;
    if (g == 0) {
      den[q] = d_old * f_old + dn * f_new;
      aexp[q] = e_new;
    }
  }
  template <int NKK>
  __device__ __forceinline__ void node(const WalkArgs &a, int n, int tile, int lane, const double (&pre)[NKK], int pcnt) const {
    if (which != 0) return;  // in_n * U_n
    double t = 0.;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) t += pre[kk];
    add<NKK>(a, n, tile * 16 + (lane & 15), lane >> 4, pre, row_sum4(t), pcnt);
  }
  template <int NKK>
  __device__ __forceinline__ void branch(const WalkArgs &, int, int, int, const double (&)[NKK], int) const {}
  template <int NKK>
  __device__ __forceinline__ void leaf(const WalkArgs &a, int l, int tile, int lane, const double (&U)[NKK], int vcnt) const {
    const int g = lane >> 4, sl = lane & 15;
    const int c = (int)a.codes_tile[((size_t)tile * a.L + l) * 16 + sl];
    double lv[NKK];
    leaf_vec<NKK>(a, c, g, lv);
    double t = 0.;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) t += U[kk] * lv[kk];
    add<NKK>(a, l, tile * 16 + sl, g, U, row_sum4(t), vcnt);
  }

  // 4 states: one thread per pattern
  __device__ __forceinline__ void add(const WalkArgs &a, int row, size_t s, const double (&num)[4], double dn, int e) const {
    if (s >= (size_t)S) return;
    double *out = acc + ((size_t)row * S + s) * 4;
    const size_t q = (size_t)row * a.S_pad + s;
    const double wd = w * dn, d_old = first ? 0. : den[q];
    if (!(wd > 0.) && !first) return;
    if (!(d_old > 0.)) {
      const double f = wd > 0. ? w : 0.;
      for (int j = 0; j < 4; j++) out[j] = f * num[j];
      den[q] = wd;
      aexp[q] = e;
      return;
    }
    const int e_old = aexp[q], e_new = min(e_old, e);
    const double f_old = ldexp(1.0, -64 * (e_old - e_new)), f_new = w * ldexp(1.0, -64 * (e - e_new));
    for (int j = 0; j < 4; j++) out[j] = out[j] * f_old + num[j] * f_new;
    den[q] = d_old * f_old + dn * f_new;
    aexp[q] = e_new;
  }
  __device__ __forceinline__ void node(const WalkArgs &a, int n, size_t s, const double (&pre)[4], int pcnt) const {
    if (which == 0) add(a, n, s, pre, (pre[0] + pre[1]) + (pre[2] + pre[3]), pcnt);
  }
  __device__ __forceinline__ void branch(const WalkArgs &, int, size_t, const double (&)[4], int) const {}
  __device__ __forceinline__ void leaf(const WalkArgs &a, int l, size_t s, const double (&U)[4], int vcnt) const {
    double lv[4];
    nuc_leaf_vec(a, (int)a.codes[(size_t)l * a.S_pad + s], lv);
    add(a, l, s, U, (U[0] * lv[0] + U[1] * lv[1]) + (U[2] * lv[2] + U[3] * lv[3]), vcnt);
  }
};

template <int NW>
__global__ __launch_bounds__(64) void marginal_mfma_kernel(WalkArgs a, MargSink k) {
  outside_walk<NW>(a, k);
}

__global__ __launch_bounds__(256) void marginal_nuc_kernel(WalkArgs a, MargSink k) { outside_walk_nuc(a, k); }

// support = accumulated numerator / denominator, in place; MAP state (first maximum) and its support.  A denominator of 0 (the
// pattern is impossible under every class): NaN in all D entries, state -1, support NaN
__global__ __launch_bounds__(256) void marginal_finish_kernel(double *__restrict__ acc, const double *__restrict__ den, int rows, int S,
                                                              int S_pad, int D, int32_t *__restrict__ map_state,
                                                              double *__restrict__ map_support) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)rows * S) return;
  const size_t row = t / S, s = t - row * S;
  const double d = den[row * S_pad + s];
  double *v = acc + t * D;
  if (!(d > 0.)) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int j = 0; j < D; j++) v[j] = nan;
    map_state[t] = -1;
    map_support[t] = nan;
    return;
  }
  const double inv = 1.0 / d;
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
  if (check_pass_ready(p, "marginal_ancestral: ", weights)) return -1;
  std::vector<double> pi_pad;
  if (begin_outside(p, pi_pad)) return -1;
  const int C = (int)p->C;
  const int64_t D = p->D, L = p->L, I = p->I, B = p->B, S = p->S;
  const int DP = p->DP, NW = p->NW;
  const int64_t rows = which == 0 ? I : L;
  const std::vector<int4> &prog = p->marg_prog;
  const int maxk = p->marg_maxk;
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    const size_t node_stride = p->nuc ? (size_t)4 * s.S_pad : (size_t)s.ntiles * 16 * DP;
    if (!s.marg_U) {  // scratch of the pass, kept until the partition is destroyed; published only when every block is there
      const size_t work = p->nuc ? (size_t)2 * maxk * 4 * s.S_pad : (size_t)s.ntiles * 2 * maxk * 16 * DP;
      const size_t wcnt = p->nuc ? (size_t)2 * maxk * s.S_pad : (size_t)s.ntiles * 2 * maxk * 16;
      const BlockReq scratch[] = {device_block(s.marg_U, (size_t)I * node_stride * sizeof(double)),
                                  device_block(s.marg_Ucnt, (size_t)I * s.S_pad * sizeof(int32_t)),
                                  device_block(s.marg_work, work * sizeof(double)),
                                  device_block(s.marg_wcnt, wcnt * sizeof(int32_t)),
                                  device_block(s.marg_prog, prog.size() * sizeof(int4)),
                                  device_block(s.marg_pi, pi_pad.size() * sizeof(double)),
                                  device_block(s.marg_PT, p->nuc ? 0 : (size_t)B * DP * DP * sizeof(double))};
      hipError_t ae = s.own.get_group(scratch, 7);
      if (ae == hipSuccess && (ae = hipMemcpy(s.marg_prog, prog.data(), prog.size() * sizeof(int4), hipMemcpyHostToDevice)) != hipSuccess)
        s.own.drop(scratch, 7, FreeMode::NoSync);
      if (ae != hipSuccess) return fail(std::string("marginal_ancestral: scratch: ") + hipGetErrorString(ae));
    }
    HIPCHK(hipMemcpy(s.marg_pi, pi_pad.data(), pi_pad.size() * sizeof(double), hipMemcpyHostToDevice));
    Blocks blk;  // the call's own blocks: back to the pool on every way out of this shard
    double *acc = nullptr, *den = nullptr, *msup = nullptr;
    int32_t *aexp = nullptr, *mst = nullptr;
    const size_t nrs = (size_t)rows * s.S;
    hipError_t e = blk.get(&acc, nrs * D);
    if (e == hipSuccess) e = blk.get(&den, (size_t)rows * s.S_pad);
    if (e == hipSuccess) e = blk.get(&aexp, (size_t)rows * s.S_pad);
    if (e == hipSuccess) e = blk.get(&msup, nrs);
    if (e == hipSuccess) e = blk.get(&mst, nrs);
    for (int c = 0; c < C && e == hipSuccess; c++) {
      const WalkArgs a = walk_args(p, s, c, {s.marg_prog, s.marg_pi, s.marg_PT, s.marg_U, s.marg_Ucnt, s.marg_work, s.marg_wcnt});
      const MargSink k = {C > 1 ? weights[c] : 1.0, c == 0, (int)which, (int)D, (int)s.S, acc, den, aexp};
      if (p->nuc) {
        hipLaunchKernelGGL(marginal_nuc_kernel, dim3((unsigned)((s.S_pad + 255) / 256)), dim3(256), 0, s.stream, a, k);
      } else {
        hipLaunchKernelGGL(marg_transpose_kernel, dim3((unsigned)B), dim3(256), 0, s.stream, a.Pfrag, a.PTg, s.marg_PT, NW, (int)L);
        LAUNCH_NW(marginal_mfma_kernel, NW, dim3((unsigned)s.ntiles), dim3(64), s.stream, a, k);
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
      if (e == hipSuccess && map_state_out) rows_to_caller(p, s, hs.data(), (size_t)s.S, rows, s.S, map_state_out);
      if (e == hipSuccess && map_support_out) rows_to_caller(p, s, hv.data(), (size_t)s.S, rows, s.S, map_support_out);
    }
    if (e != hipSuccess) return fail(std::string("marginal_ancestral: ") + hipGetErrorString(e));
  }
  return 0;
}

}  // extern "C"
