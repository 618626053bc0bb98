// Simulation down the tree — the device counterpart of _LikelihoodFunction::Simulate / BuildLeafProbs / SingleBuildLeafProbs
// (src/core/likefunc.cpp:12584-13259) with DrawFromDiscrete (src/core/include/function_templates.h:404-413): HBL's SimulateDataSet.
//
// A column is (replicate r, site j) with rate class c = class_of_site[r][j]; sites are free (no relation to the partition's patterns).
// Nodes are visited parent-first; per node n of a column:
//   root (node code L + I - 1): row = pi (or the caller's root state);    otherwise: row = P_n^(c)[state of the parent]
//   cum_i = row[0] + ... + row[i] in ascending i, every addition rounded;  total = cum_{D-1};  x = u * total
//   state = the smallest i with cum_i >= x and cum_i > 0
// Three deviations from the reference: x = u * total instead of x = u (rows sum to 1 within a few ulp; the reference returns index D,
// past the row, when u exceeds the rounded sum); u == 0 picks the first state of positive weight; total <= 0 or NaN gives -1 and every
// descendant of a -1 node is -1 (the reference would index with a bad state).
// Uniforms: the caller's array [n_rep][L + I][n_sites] by node code, or Philox4x32-10 (philox.h) with key = (seed low, seed high),
// counter = (j, node code, r, 1): a draw depends on (seed, r, j, node) only — not on chunks, slices or the sort by class; the last
// counter word keeps the stream disjoint from sample_ancestral's (0).
//
// Reads the matrix images of the last evaluation of each referenced class and the root frequencies — no conditionals, no leaf data.
// Which image: ONE rule for 2, 3, 5..64 states — a leaf's branch (node code < L) is read from the column-gather image PTg
// ([code][wb][g][r] = P[16 wb + 4 r + g][code]), an internal node's from the A-operand image Pfrag.  Every path that writes matrices
// leaves at least that image: the 49..64-state exponential writes per Shard::expm_need (leaves: bit 1, always; internal branches:
// bit 0, always), every other writer (smaller exponentials, the mixing kernel, the branch cache's exponential) writes both.
// 4 states: the row-major Prow.
//
// simulate_tables_kernel<NW> (simulate_nuc_tables_kernel): per referenced class and node a table [B + 1][DP][LD], LD = DP + 1 (4 states:
// [B + 1][4][5]); table B is pi (row 0).  Row s: entries i < D the running maximum m_i = max(cum_0 .. cum_i), entries D .. DP - 1
// m_{D-1}, entry DP the total.  One thread sums one row, serially.  The smallest i with m_i >= x and m_i > 0 is the contract's i
// (m is non-decreasing; for x > 0 the first cum_i >= x is the first m_i >= x, for x == 0 the first cum_i > 0 is the first m_i > 0),
// also for rows with tiny negative entries, which is what allows the lower-bound search below.
// simulate_kernel<NW>: the host buckets the columns of a chunk by class (counting sort, stable in (r, j)); a workgroup of 256 threads
// owns a slice of at most kSlice columns of ONE class and walks the internal nodes in descending index, then the leaves.  Per node it
// stages the node's table in LDS (leading dimension DP + 1, odd: threads read different rows); each thread then takes its columns in
// turn: the parent's byte (stored by itself), u, x = u * total, a branch-free lower-bound search over m (log2 D probes), one byte
// out at [(r - r0) * (L + I) + node][j - j0] — consecutive columns store consecutive bytes, and the chunk goes back to the caller's
// array as it lies.  simulate_nuc_kernel: one column per thread, tables from global memory.
// No hand-off between workgroups, no fences, no atomics; every loop is bounded by the node count, D or the slice.
#include "partition.h"
#include "philox.h"

using namespace hyhip;

namespace hyhip {
namespace {

constexpr int kSlice = 2048;     // columns of a workgroup (simulate_kernel)
constexpr int kSliceNuc = 256;   // ... of simulate_nuc_kernel: one per thread
constexpr int64_t kMaxChunkCols = (int64_t)1 << 30;  // columns of a chunk: entry numbers and offsets within a row stay 32-bit

struct SimTabArgs {
  int D, L, B;
  const int32_t *cls;    // [sets] class of table set k
  const double *Pfrag;   // class 0: [B][NW][NKK*64]   (class stride cs)
  const double *PTg;     // class 0: [B][DP][NW][16]
  const double *Prow;    // class 0: [B][16] (4 states)
  size_t cs;
  const double *pi;      // [DP] (4 states: [4])
  double *tab;           // [sets][B + 1][DP][LD]
};

// one row's running maxima and total
template <typename Get>
__device__ __forceinline__ void sim_row_out(Get get, int D, int DP, double *out) {
#pragma clang fp contract(off)
  double cum = 0., m = -INFINITY;
  for (int i = 0; i < D; i++) {
    cum = cum + get(i);
    m = fmax(m, cum);
    out[i] = m;
  }
  for (int i = D; i < DP; i++) out[i] = m;
  out[DP] = cum;
}

template <int NW>
__global__ __launch_bounds__(64) void simulate_tables_kernel(SimTabArgs a) {
  constexpr int DP = 16 * NW, LD = DP + 1, TILE = DP * 16;
  const int D = a.D, B = a.B;
  const int k = blockIdx.x / (B + 1), b = blockIdx.x - k * (B + 1), r = threadIdx.x;  // grid = sets x (B + 1)
  if (r >= DP) return;
  double *out = a.tab + (((size_t)k * (B + 1) + b) * DP + r) * LD;
  const bool live = b == B ? r == 0 : r < D;
  if (!live) {
    for (int i = 0; i < LD; i++) out[i] = 0.;
    return;
  }
  if (b == B) {
    const double *pi = a.pi;
    sim_row_out([=](int i) { return pi[i]; }, D, DP, out);
  } else if (b < a.L) {  // P[r][i] from the column-gather image
    const double *g = a.PTg + (size_t)a.cls[k] * a.cs + (size_t)b * DP * DP + (r >> 4) * 16 + (r & 3) * 4 + ((r >> 2) & 3);
    sim_row_out([=](int i) { return g[(size_t)i * NW * 16]; }, D, DP, out);
  } else {               // ... from the A-operand image
    const double *f = a.Pfrag + (size_t)a.cls[k] * a.cs + (size_t)b * DP * DP + (r >> 4) * TILE;
    sim_row_out([=](int i) { return f[frag_index(i >> 2, (i & 3) * 16 + (r & 15))]; }, D, DP, out);
  }
}

__global__ __launch_bounds__(64) void simulate_nuc_tables_kernel(SimTabArgs a) {
  const int B = a.B, nb = ((B + 1) * 4 + 63) / 64;  // grid = sets x nb
  const int k = blockIdx.x / nb, idx = (blockIdx.x - k * nb) * 64 + threadIdx.x;
  if (idx >= (B + 1) * 4) return;
  const int b = idx >> 2, r = idx & 3;
  double *out = a.tab + (((size_t)k * (B + 1) + b) * 4 + r) * 5;
  if (b == B && r != 0) {
    for (int i = 0; i < 5; i++) out[i] = 0.;
    return;
  }
  const double *src = b == B ? a.pi : a.Prow + (size_t)a.cls[k] * a.cs + (size_t)b * 16 + 4 * r;
  sim_row_out([=](int i) { return src[i]; }, 4, 4, out);
}

struct SimArgs {
  int D, L, I;
  int nc;                     // sites of the chunk (stride of a scratch row)
  int64_t r0, j0;             // its first replicate and site
  const int4 *work;           // [grid] (table set, first entry, entries, 0)
  const int32_t *cols;        // [entries of the chunk] column (rr * nc + jj) of entry e, or nullptr: entry e is column e
  const int32_t *parent;      // [L + I] internal index of the parent
  const double *tab;          // [sets][B + 1][DP][LD]
  const int8_t *root;         // [Rc * nc] the caller's root states by column, or nullptr: drawn from pi
  const double *u;            // [Rc][L + I][nc] or nullptr: Philox
  uint64_t seed;
  int8_t *out;                // [Rc][L + I][nc]
};

// the smallest i < D with m[i] >= u * total and m[i] > 0 (m = row[0 .. D), non-decreasing; total = row[tot]); -1: none
__device__ __forceinline__ int sim_search(const double *row, int D, int tot, double u) {
  const double total = row[tot];
  if (!(total > 0.)) return -1;  // (a NaN total compares false)
  const double x = u * total;
  const double *base = row;
  int len = D;
  while (len > 1) {              // at most log2 D + 1 probes
    const int half = len >> 1;
    const double v = base[half - 1];
    base += (v >= x && v > 0.) ? 0 : half;
    len -= half;
  }
  const double v = *base;
  const int i = (int)(base - row) + ((v >= x && v > 0.) ? 0 : 1);
  return i < D ? i : -1;
}

template <int NW>
__global__ __launch_bounds__(256) void simulate_kernel(SimArgs a) {
  constexpr int DP = 16 * NW, LD = DP + 1;
  __shared__ double T[DP * LD];   // [parent state][m_0 .. m_{DP-1}, total]
  const int4 w = a.work[blockIdx.x];
  const int e0 = w.y, e1 = w.y + w.z;
  const int D = a.D, L = a.L, I = a.I, rows = L + I, nc = a.nc;
  const double *tab = a.tab + (size_t)w.x * rows * DP * LD;  // (B + 1 = L + I tables)
  for (int step = 0; step < rows; step++) {
    const int node = step < I ? rows - 1 - step : step - I;  // internal nodes in descending index, then the leaves
    const bool is_root = step == 0;
    __syncthreads();  // the previous node's readers of T are done
    {
      const double *src = tab + (size_t)node * DP * LD;  // (the root's node code is B: the table of pi)
      const int n = is_root ? LD : D * LD;
      for (int idx = threadIdx.x; idx < n; idx += 256) T[idx] = src[idx];
    }
    __syncthreads();
    const int par = is_root ? 0 : L + a.parent[node];
    for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
      const int col = a.cols ? a.cols[e] : e;
      const int rr = col / nc, jj = col - rr * nc;
      const size_t o = ((size_t)rr * rows + node) * nc + jj;
      int st = -1;
      if (is_root && a.root) {
        st = a.root[col];
      } else {
        int ps = 0;
        if (!is_root) ps = a.out[((size_t)rr * rows + par) * nc + jj];  // (stored by this thread)
        if (ps >= 0) {
          const double u = a.u ? a.u[o] : philox_uniform(a.seed, (uint32_t)(a.j0 + jj), (uint32_t)node, (uint32_t)(a.r0 + rr), kPhiloxSimulate);
          st = sim_search(T + ps * LD, D, DP, u);
        }
      }
      a.out[o] = (int8_t)st;
    }
  }
}

// 4 states: one column per thread, the tables (20 doubles per node) from global memory
__global__ __launch_bounds__(256) void simulate_nuc_kernel(SimArgs a) {
  const int4 w = a.work[blockIdx.x];
  const int e = w.y + (int)threadIdx.x;
  if (e >= w.y + w.z) return;
  const int L = a.L, I = a.I, rows = L + I, nc = a.nc;
  const double *tab = a.tab + (size_t)w.x * rows * 20;
  const int col = a.cols ? a.cols[e] : e;
  const int rr = col / nc, jj = col - rr * nc;
  for (int step = 0; step < rows; step++) {
    const int node = step < I ? rows - 1 - step : step - I;
    const bool is_root = step == 0;
    const size_t o = ((size_t)rr * rows + node) * nc + jj;
    int st = -1;
    if (is_root && a.root) {
      st = a.root[col];
    } else {
      int ps = 0;
      if (!is_root) ps = a.out[((size_t)rr * rows + L + a.parent[node]) * nc + jj];
      if (ps >= 0) {
        const double u = a.u ? a.u[o] : philox_uniform(a.seed, (uint32_t)(a.j0 + jj), (uint32_t)node, (uint32_t)(a.r0 + rr), kPhiloxSimulate);
        st = sim_search(tab + (size_t)node * 20 + ps * 5, 4, 4, u);
      }
    }
    a.out[o] = (int8_t)st;
  }
}

}  // namespace
}  // namespace hyhip

extern "C" {

int hyphy_hip_simulate_uniforms(uint64_t seed, int64_t n_rep, int64_t n_nodes, int64_t n_sites, double *out) {
  if (n_rep < 0 || n_nodes < 0 || n_sites < 0) return fail("simulate_uniforms: negative count");
  if (n_rep > INT32_MAX || n_nodes > INT32_MAX || n_sites > INT32_MAX) return fail("simulate_uniforms: count above 2^31 - 1");
  if (n_rep == 0 || n_nodes == 0 || n_sites == 0) return 0;
  if (!out) return fail("simulate_uniforms: out == NULL");
  for (int64_t r = 0; r < n_rep; r++)
    for (int64_t n = 0; n < n_nodes; n++) {
      double *row = out + ((size_t)r * n_nodes + n) * n_sites;
      for (int64_t j = 0; j < n_sites; j++) row[j] = philox_uniform(seed, (uint32_t)j, (uint32_t)n, (uint32_t)r, kPhiloxSimulate);
    }
  return 0;
}

int hyphy_hip_simulate(hyphy_hip_partition *p, int64_t n_rep, int64_t n_sites, const int64_t *class_of_site, const int64_t *root_states,
                       uint64_t seed, const double *uniforms, int with_internal, int8_t *states_out) {
  if (!p) return fail("simulate: partition == NULL");
  if (!states_out) return fail("simulate: states_out == NULL");
  if (n_rep < 0 || n_sites < 0) return fail("simulate: negative count");
  if (n_rep > INT32_MAX || n_sites > INT32_MAX) return fail("simulate: count above 2^31 - 1");
  if (n_rep == 0 || n_sites == 0) return 0;
  const int C = (int)p->C;
  const int64_t D = p->D, L = p->L, I = p->I, B = p->B, rows = L + I;
  const size_t n_cols = (size_t)n_rep * n_sites;
  std::vector<int32_t> set_of((size_t)C, -1), cls_of_set;  // table set of a class (-1: not referenced), and back
  if (class_of_site) {
    std::vector<char> seen((size_t)C, 0);
    for (size_t k = 0; k < n_cols; k++) {
      const int64_t c = class_of_site[k];
      if (c < 0 || c >= C)
        return fail("simulate: column " + std::to_string(k) + ": rate class " + std::to_string(c) + " out of range");
      seen[(size_t)c] = 1;
    }
    for (int c = 0; c < C; c++)
      if (seen[(size_t)c]) set_of[(size_t)c] = (int32_t)cls_of_set.size(), cls_of_set.push_back(c);
  } else {
    set_of[0] = 0, cls_of_set.push_back(0);
  }
  {
    std::vector<char> used((size_t)C, 0);
    for (int32_t c : cls_of_set) used[(size_t)c] = 1;
    if (check_evaluated(p, "simulate: ", &used)) return -1;
  }
  if (uniforms) {
    const size_t total = n_cols * (size_t)rows;
    for (size_t k = 0; k < total; k++)
      if (!(uniforms[k] >= 0. && uniforms[k] < 1.)) return fail("simulate: uniform " + std::to_string(k) + " is outside [0, 1)");
  }
  if (root_states)
    for (size_t k = 0; k < n_cols; k++)
      if (root_states[k] < 0 || root_states[k] >= D)
        return fail("simulate: column " + std::to_string(k) + ": root state " + std::to_string(root_states[k]) + " out of range");
  if (finish_pending_async(p)) return -1;
  const int NW = p->NW;
  const bool nuc = p->nuc;
  const int tDP = nuc ? 4 : p->DP, tLD = tDP + 1, slice = nuc ? kSliceNuc : kSlice;
  const int K = (int)cls_of_set.size();
  std::vector<int32_t> parent((size_t)rows, -1);
  for (int64_t c = 0; c < rows - 1; c++) parent[(size_t)c] = (int32_t)p->parents[(size_t)c];
  const std::vector<double> pi_pad = padded_pi(p);
  Shard &s = p->shards[0];  // (every shard holds every matrix)
  HIPCHK(hipSetDevice(s.device));
  HIPCHK(hipStreamSynchronize(s.stream));
  // ---- the tables of the referenced classes -----------------------------------------------------------------------------------
  Blocks tree;
  int32_t *d_parent = nullptr, *d_cls = nullptr;
  double *d_pi = nullptr, *d_tab = nullptr;
  HIPCHK(tree.get(&d_parent, parent.size()));
  HIPCHK(tree.get(&d_cls, cls_of_set.size()));
  HIPCHK(tree.get(&d_pi, pi_pad.size()));
  HIPCHK(tree.get(&d_tab, (size_t)K * rows * tDP * tLD));
  HIPCHK(hipMemcpyAsync(d_parent, parent.data(), parent.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(d_cls, cls_of_set.data(), cls_of_set.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(d_pi, pi_pad.data(), pi_pad.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
  {
    SimTabArgs t;
    t.D = (int)D, t.L = (int)L, t.B = (int)B, t.cls = d_cls, t.pi = d_pi, t.tab = d_tab;
    t.Pfrag = s.Pfrag, t.PTg = s.PTg, t.Prow = s.Prow;
    t.cs = nuc ? (size_t)B * 16 : (size_t)B * p->DP * p->DP;
    if ((double)K * (double)rows > 2147483647.) return fail("simulate: too many referenced classes for one table launch");
    if (nuc) hipLaunchKernelGGL(simulate_nuc_tables_kernel, dim3((unsigned)(((rows * 4 + 63) / 64) * K)), dim3(64), 0, s.stream, t);
    else LAUNCH_NW(simulate_tables_kernel, NW, dim3((unsigned)(rows * K)), dim3(64), s.stream, t);
    HIPCHK(hipGetLastError());
  }
  // ---- chunks: as many whole replicates as fit the budget, else site ranges of one replicate (at least one column) ------------
  const double budget = sw::scratch_budget(sw::SIMULATE_MB);
  const double col_bytes = (double)rows * (uniforms ? 9. : 1.);  // scratch of one column: a byte (and a uniform) per node
  int64_t Rc = 1, ncap = n_sites;
  if (col_bytes * (double)n_sites <= budget && n_sites <= kMaxChunkCols) {
    Rc = (int64_t)std::min<double>((double)n_rep, floor(budget / (col_bytes * (double)n_sites)));
    Rc = std::max<int64_t>(1, std::min<int64_t>(Rc, kMaxChunkCols / n_sites));
  } else {
    ncap = (int64_t)std::min<double>((double)std::min<int64_t>(n_sites, kMaxChunkCols), floor(budget / col_bytes));
    ncap = std::max<int64_t>(1, ncap);
  }
  const size_t cap_cols = (size_t)Rc * (size_t)ncap;
  const size_t max_work = (size_t)K + cap_cols / (size_t)slice + 1;
  Blocks blk;
  int8_t *d_out = nullptr, *d_root = nullptr;
  double *d_u = nullptr;
  int32_t *d_cols = nullptr;
  int4 *d_work = nullptr;
  HIPCHK(blk.get(&d_out, cap_cols * (size_t)rows));
  if (uniforms) HIPCHK(blk.get(&d_u, cap_cols * (size_t)rows));
  if (root_states) HIPCHK(blk.get(&d_root, cap_cols));
  if (K > 1) HIPCHK(blk.get(&d_cols, cap_cols));
  HIPCHK(blk.get(&d_work, max_work));
  SimArgs a;
  a.D = (int)D, a.L = (int)L, a.I = (int)I;
  a.work = d_work, a.cols = d_cols, a.parent = d_parent, a.tab = d_tab, a.root = d_root, a.u = d_u, a.seed = seed, a.out = d_out;
  const int64_t rows_out = with_internal ? rows : L;
  std::vector<int32_t> cols, first;
  std::vector<int4> work;
  std::vector<int8_t> h_root;
  std::vector<double> h_u;
  for (int64_t r0 = 0; r0 < n_rep; r0 += Rc) {
    const int64_t R = std::min(Rc, n_rep - r0);
    for (int64_t j0 = 0; j0 < n_sites; j0 += ncap) {
      const int64_t nc = std::min(ncap, n_sites - j0);
      const size_t ncols = (size_t)R * (size_t)nc;
      a.nc = (int)nc, a.r0 = r0, a.j0 = j0;
      // the columns by class: a counting sort, stable in (r, j)
      first.assign((size_t)K + 1, 0);
      if (K > 1) {
        for (int64_t rr = 0; rr < R; rr++) {
          const int64_t *cs = class_of_site + (size_t)(r0 + rr) * n_sites + j0;
          for (int64_t jj = 0; jj < nc; jj++) first[(size_t)set_of[(size_t)cs[jj]] + 1]++;
        }
        for (int k = 0; k < K; k++) first[(size_t)k + 1] += first[(size_t)k];
        cols.resize(ncols);
        std::vector<int32_t> next(first.begin(), first.end() - 1);
        for (int64_t rr = 0; rr < R; rr++) {
          const int64_t *cs = class_of_site + (size_t)(r0 + rr) * n_sites + j0;
          for (int64_t jj = 0; jj < nc; jj++) cols[(size_t)next[(size_t)set_of[(size_t)cs[jj]]]++] = (int32_t)(rr * nc + jj);
        }
        HIPCHK(hipMemcpyAsync(d_cols, cols.data(), ncols * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
      } else {
        first[1] = (int32_t)ncols;
      }
      work.clear();
      for (int k = 0; k < K; k++)
        for (int32_t e = first[(size_t)k]; e < first[(size_t)k + 1]; e += slice)
          work.push_back(make_int4(k, e, std::min<int32_t>(slice, first[(size_t)k + 1] - e), 0));
      if (work.size() > max_work) return fail("simulate: internal: work list larger than planned");
      HIPCHK(hipMemcpyAsync(d_work, work.data(), work.size() * sizeof(int4), hipMemcpyHostToDevice, s.stream));
      if (root_states) {
        h_root.resize(ncols);
        for (int64_t rr = 0; rr < R; rr++)
          for (int64_t jj = 0; jj < nc; jj++) h_root[(size_t)(rr * nc + jj)] = (int8_t)root_states[(size_t)(r0 + rr) * n_sites + j0 + jj];
        HIPCHK(hipMemcpyAsync(d_root, h_root.data(), ncols, hipMemcpyHostToDevice, s.stream));
      }
      if (uniforms) {
        const double *src = uniforms + (size_t)r0 * rows * n_sites;
        if (nc == n_sites) {  // whole replicates: the caller's rows are the chunk's
          HIPCHK(hipMemcpyAsync(d_u, src, ncols * (size_t)rows * sizeof(double), hipMemcpyHostToDevice, s.stream));
        } else {              // a site range of one replicate
          h_u.resize((size_t)rows * nc);
          for (int64_t n = 0; n < rows; n++) memcpy(h_u.data() + (size_t)n * nc, src + (size_t)n * n_sites + j0, (size_t)nc * sizeof(double));
          HIPCHK(hipMemcpyAsync(d_u, h_u.data(), h_u.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
        }
      }
      if (nuc) hipLaunchKernelGGL(simulate_nuc_kernel, dim3((unsigned)work.size()), dim3(256), 0, s.stream, a);
      else LAUNCH_NW(simulate_kernel, NW, dim3((unsigned)work.size()), dim3(256), s.stream, a);
      HIPCHK(hipGetLastError());
      // -> [replicate][node][site]: the chunk lies as the caller's array does (leaves first: without the internal nodes, L rows)
      if (nc == n_sites && with_internal) {
        HIPCHK(hipMemcpyAsync(states_out + (size_t)r0 * rows * n_sites, d_out, ncols * (size_t)rows, hipMemcpyDeviceToHost, s.stream));
      } else if (nc == n_sites) {
        for (int64_t rr = 0; rr < R; rr++)
          HIPCHK(hipMemcpyAsync(states_out + (size_t)(r0 + rr) * L * n_sites, d_out + (size_t)rr * rows * n_sites, (size_t)L * n_sites,
                                hipMemcpyDeviceToHost, s.stream));
      } else {
        for (int64_t n = 0; n < rows_out; n++)
          HIPCHK(hipMemcpyAsync(states_out + ((size_t)r0 * rows_out + n) * n_sites + j0, d_out + (size_t)n * nc, (size_t)nc,
                                hipMemcpyDeviceToHost, s.stream));
      }
      HIPCHK(hipStreamSynchronize(s.stream));  // (the host vectors are rewritten by the next chunk)
    }
  }
  return 0;
}

}  // extern "C"
