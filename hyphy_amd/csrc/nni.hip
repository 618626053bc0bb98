// Every nearest-neighbour interchange's likelihood from one outside pass — the device counterpart of scoring the neighbours of a tree
// one full evaluation each (the reference's doNNISwap.bf / branchSwappingFunctions.bf rebuild the tree and the likelihood function per
// swap).  A move (x, y): c = parent(x) internal and not the root, y a sibling of c below p = parent(c); x and y exchange parents, every
// branch keeps its own matrix.  Only the child sets of c and p change, so with outside.h's notation (E_k = P_k in_k, U_n the outside
// vector at n, U_root = pi), per pattern and class
//   R     = U_p * prod E_k   over the children k of p other than c and y
//   inner = E_y * prod E_k   over the children k of c other than x
//   l     = sum_i R[i] E_x[i] (P_c inner)[i],      2^64 exponent = exponent(R) + exponent(E_x) + exponent(inner),
// every vector rescaled where rescale_vec would.
//
// Phase 1 and the loop over chunks of tiles and classes are outside_pass.h's, unchanged: the walk leaves U_p and its exponent of the
// chunk and class it has just walked in WalkArgs::U / Ucnt (the root's is pi and is never stored).
// Phase 2 (nni_kernel<NW>, nni_nuc_kernel): one wave per (branch c with at least one move, tile), the tile the fastest grid index; the
// moves of a branch run in ascending y, and R and E_y — what the moves (., y) of one branch have in common — are formed once per y.
// Everything stays in registers; a move costs the products of E_x, of c's other internal children and of P_c, plus those of a new y.
// The per-pattern mix over classes, the per-(move, tile) records and the reduction are site_mix.h's, the trials' own: two identical
// calls give identical bits.  No exponential, no atomics, nothing joins by order of arrival.  All scratch comes from the pool and goes
// back before the call returns; the partition's matrices, images, schedules and caches are read and never written.
// 4 states: one thread per pattern over the plane layout and row-major matrices.
#include "combine.h"
#include "devutil.h"
#include "nni_plan.h"
#include "outside_pass.h"
#include "partition.h"
#include "site_mix.h"

using namespace hyhip;

namespace hyhip {
namespace {

struct NniArgs {        // the request tables (nni_plan.h), beside the WalkArgs, the OutsideSlice and the TrialArgs
  const int4 *entries;  // [n][3]
  const int *others;
};

__device__ __forceinline__ int4 node_entry(const WalkArgs &a, int node) { return make_int4(1, node, node >= a.L ? node - a.L : -1, 0); }

template <int NW>
__global__ __launch_bounds__(64) void nni_kernel(WalkArgs wa, OutsideSlice sl, TrialArgs a, NniArgs na) {
  constexpr int NKK = 4 * NW, DP = 16 * NW, TILE = NKK * 64;
  const int lane = threadIdx.x, g = lane >> 4;
  const int tile = sl.tile0 + blockIdx.x, lt = blockIdx.x, site = tile * 16 + (lane & 15);
  const int bi = sl.b0 + blockIdx.y;
  const int4 cen = branch_entry(wa, sl, bi);
  const double *Pc = wa.Pfrag + (size_t)cen.y * DP * DP;
  const double f = sl.freq[site];
  double R[NKK], Ey[NKK];
  int rcnt = 0, ycnt = 0, have_y = -1;
  for (int k = sl.off[bi]; k < sl.off[bi + 1]; k++) {
    const int t = sl.idx[k];
    const int4 ex = na.entries[3 * t], ey = na.entries[3 * t + 1], m = na.entries[3 * t + 2];
    const int *oc = na.others + m.y, *op = oc + m.z;
    if (ey.y != have_y) {  // (the moves of a branch come in ascending y)
      if (m.x < 0) {
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) R[kk] = wa.pi[4 * kk + g];
        rcnt = 0;
      } else {
        const size_t o = (size_t)m.x * wa.chunk + lt;
        ld_vec<NKK>(wa.U + o * TILE, lane, R);
        rcnt = wa.Ucnt[o * 16 + (lane & 15)];
      }
      for (int j = 0; j < m.w; j++) {
        double E[NKK];
        int ecnt;
        edge_product<NW>(wa, node_entry(wa, op[j]), tile, lane, E, ecnt);
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) R[kk] *= E[kk];
        rcnt += ecnt;
        rescale_vec<NKK>(R, rcnt);
      }
      edge_product<NW>(wa, ey, tile, lane, Ey, ycnt);
      have_y = ey.y;
    }
    double inner[NKK], F[NKK];
    int icnt = ycnt, xcnt;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) inner[kk] = Ey[kk];
    for (int j = 0; j < m.z; j++) {
      double E[NKK];
      int ecnt;
      edge_product<NW>(wa, node_entry(wa, oc[j]), tile, lane, E, ecnt);
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) inner[kk] *= E[kk];
      icnt += ecnt;
      rescale_vec<NKK>(inner, icnt);
    }
    mfma_product<NW>(Pc, inner, lane, F);
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) F[kk] *= R[kk];
    double Ex[NKK];
    edge_product<NW>(wa, ex, tile, lane, Ex, xcnt);
    double s = 0.;
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) s += F[kk] * Ex[kk];
    s = row_sum4(s);
    double wsum = 0.;
    long long wcnt = 0;
    int wflag = 0;
    if (g == 0) {
      const size_t q = (size_t)t * wa.S_pad + site;
      int e = rcnt + xcnt + icnt;
      mix_in(sl, a, q, s, e);
      a.lik[q] = s;
      a.cnt[q] = e;
      if (sl.last) site_term(s, e, f, wsum, wcnt, wflag);
    }
    if (sl.last) put_record<16>(sl, a, t, tile, lane, wsum, wcnt, wflag);
  }
}

// 4 states: the edge product of node `node` at pattern s and its exponent
__device__ __forceinline__ void nuc_edge(const WalkArgs &wa, int node, size_t s, double (&E)[4], int &ecnt) {
  double in[4];
  nuc_child_vec(wa, node_entry(wa, node), s, in, ecnt);
  mat4_vec(wa.Prow + (size_t)node * 16, in, E);
}

// 4 states: one thread per pattern, one wave per (branch, 64 patterns)
__global__ __launch_bounds__(64) void nni_nuc_kernel(WalkArgs wa, OutsideSlice sl, TrialArgs a, NniArgs na) {
  const int lane = threadIdx.x, tile = sl.tile0 + blockIdx.x;
  const size_t s = (size_t)tile * 64 + lane, ls = (size_t)blockIdx.x * 64 + lane, CS = (size_t)wa.chunk;
  const int bi = sl.b0 + blockIdx.y;
  const int4 cen = branch_entry(wa, sl, bi);
  const double f = sl.freq[s];
  double R[4], Ey[4];
  int rcnt = 0, ycnt = 0, have_y = -1;
  for (int k = sl.off[bi]; k < sl.off[bi + 1]; k++) {
    const int t = sl.idx[k];
    const int4 ex = na.entries[3 * t], ey = na.entries[3 * t + 1], m = na.entries[3 * t + 2];
    const int *oc = na.others + m.y, *op = oc + m.z;
    if (ey.y != have_y) {
      rcnt = 0;
      if (m.x < 0) {
        for (int j = 0; j < 4; j++) R[j] = wa.pi[j];
      } else {
        for (int j = 0; j < 4; j++) R[j] = wa.U[((size_t)m.x * 4 + j) * CS + ls];
        rcnt = wa.Ucnt[(size_t)m.x * CS + ls];
      }
      for (int j = 0; j < m.w; j++) {
        double E[4];
        int ecnt;
        nuc_edge(wa, op[j], s, E, ecnt);
        for (int i = 0; i < 4; i++) R[i] *= E[i];
        rcnt += ecnt;
        rescale4(R, rcnt);
      }
      nuc_edge(wa, ey.y, s, Ey, ycnt);
      have_y = ey.y;
    }
    double inner[4] = {Ey[0], Ey[1], Ey[2], Ey[3]}, F[4], Ex[4], l = 0.;
    int icnt = ycnt, xcnt;
    for (int j = 0; j < m.z; j++) {
      double E[4];
      int ecnt;
      nuc_edge(wa, oc[j], s, E, ecnt);
      for (int i = 0; i < 4; i++) inner[i] *= E[i];
      icnt += ecnt;
      rescale4(inner, icnt);
    }
    mat4_vec(wa.Prow + (size_t)cen.y * 16, inner, F);
    nuc_edge(wa, ex.y, s, Ex, xcnt);
    for (int i = 0; i < 4; i++) l += R[i] * F[i] * Ex[i];
    const size_t q = (size_t)t * wa.S_pad + s;
    int e = rcnt + xcnt + icnt;
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

}  // namespace
}  // namespace hyhip

extern "C" {

int hyphy_hip_nni_scores(hyphy_hip_partition *p, int64_t n, const int64_t *moves, const double *weights, double *logl_out,
                         double *site_lik_out, int64_t *site_scaler_out) {
  const std::string pre = "nni_scores: ";
  if (!p) return fail(pre + "partition == NULL");
  if (n < 0) return fail(pre + "n < 0");
  if (check_pass_ready(p, pre, weights)) return -1;
  if (n == 0) return 0;
  if (!moves || !logl_out) return fail(pre + "null argument");
  if (n * p->C > 0x3fffffff) return fail(pre + "too many moves");
  const std::string bad = nni_moves_error(p->L, p->I, p->parents.data(), n, moves);
  if (!bad.empty()) return fail(pre + bad);
  const NniTables tab = plan_nni_tables(p->L, p->I, p->parents.data(), p->children, n, moves);
  const KeepForms keep = {p, p->last_reduce, last_expm_kernel()};
  OutsideCall oc;
  if (begin_outside(p, oc, tab.branch.data(), n)) return -1;
  for (size_t gi = 0; gi + 1 < oc.groups.off.size(); gi++)  // the moves of a branch in ascending y (then in the caller's order)
    std::stable_sort(oc.groups.order.begin() + oc.groups.off[gi], oc.groups.order.begin() + oc.groups.off[gi + 1],
                     [&](int a, int b) { return moves[2 * a + 1] < moves[2 * b + 1]; });
  const int NW = p->NW;
  const bool nuc = p->nuc;
  std::vector<double> totals((size_t)n);
  std::vector<std::vector<double>> parts((size_t)n);
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    Blocks blk;
    OutsideScratch sc;
    sc.plan(p, s, oc);
    const size_t np = (size_t)n * sc.part_stride;
    double *lik = nullptr, *part_sum = nullptr, *d_tot = nullptr;
    int32_t *cnt = nullptr;
    long long *part_cnt = nullptr;
    int *part_flag = nullptr, *d_others = nullptr;
    int4 *d_entries = nullptr;
    HIPCHK(blk.get(&lik, (size_t)n * s.S_pad));
    HIPCHK(blk.get(&cnt, (size_t)n * s.S_pad));
    HIPCHK(blk.get(&part_sum, np));
    HIPCHK(blk.get(&part_cnt, np));
    HIPCHK(blk.get(&part_flag, np));
    HIPCHK(blk.get(&d_tot, (size_t)n));
    HIPCHK(blk.get(&d_entries, (size_t)n * 3));
    HIPCHK(blk.get(&d_others, tab.others.size()));
    if (sc.get(p, oc, blk)) return -1;
    if (sc.upload(p, oc, s.stream)) return -1;
    HIPCHK(hipMemcpyAsync(d_entries, tab.entries.data(), tab.entries.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    if (!tab.others.empty())
      HIPCHK(hipMemcpyAsync(d_others, tab.others.data(), tab.others.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    const TrialArgs ta = {nullptr, lik, cnt, part_sum, part_cnt, part_flag};
    const NniArgs na = {d_entries, d_others};
    const int walked = outside_chunks(p, s, oc, sc, weights, [&](const WalkArgs &a, const OutsideSlice &sl, dim3 grid) {
      if (nuc) hipLaunchKernelGGL(nni_nuc_kernel, grid, dim3(64), 0, s.stream, a, sl, ta, na);
      else LAUNCH_NW(nni_kernel, NW, grid, dim3(64), s.stream, a, sl, ta, na);
    });
    if (walked) return -1;
    hipLaunchKernelGGL(trials_reduce_kernel, dim3((unsigned)n), dim3(64), 0, s.stream, part_sum, part_cnt, part_flag, sc.ntiles,
                       sc.part_stride, d_tot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(totals.data(), d_tot, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    for (int64_t t = 0; t < n; t++) parts[(size_t)t].push_back(totals[(size_t)t]);
    if (site_lik_out && download_rows(p, s, lik, n, site_lik_out)) return -1;
    if (site_scaler_out && download_rows(p, s, cnt, n, site_scaler_out)) return -1;
  }
  for (int64_t t = 0; t < n; t++) logl_out[t] = combine(parts[(size_t)t]);
  return 0;
}

static int check_nni_tree(const std::string &pre, int64_t L, int64_t I, const int64_t *flat_parents) {
  if (L < 1 || I < 1 || !flat_parents) return fail(pre + "bad arguments");
  for (int64_t c = 0; c < L + I - 1; c++)
    if (flat_parents[c] < 0 || flat_parents[c] >= I) return fail(pre + "parent out of range");
  if (flat_parents[L + I - 1] >= 0) return fail(pre + "the root (last node) must have no parent");
  return 0;
}

int hyphy_hip_check_nni(int64_t L, int64_t I, const int64_t *flat_parents, int64_t n, const int64_t *moves) {
  const std::string pre = "check_nni: ";
  if (check_nni_tree(pre, L, I, flat_parents)) return -1;
  if (n < 0 || (n > 0 && !moves)) return fail(pre + "bad arguments");
  const std::string bad = nni_moves_error(L, I, flat_parents, n, moves);
  return bad.empty() ? 0 : fail(pre + bad);
}

int64_t hyphy_hip_plan_nni(int64_t L, int64_t I, const int64_t *flat_parents, int64_t *out, int64_t cap) {
  if (check_nni_tree("plan_nni: ", L, I, flat_parents)) return -1;
  const std::vector<int64_t> mv = plan_nni_moves(L, I, flat_parents);
  const int64_t words = 1 + (int64_t)mv.size();
  if (!out || cap < words) return -words;
  out[0] = (int64_t)mv.size() / 2;
  std::copy(mv.begin(), mv.end(), out + 1);
  return words;
}

}  // extern "C"
