// Hidden-Markov rate classes: the forward sum of SumUpHiddenMarkov and the path of RunViterbi
// (likefunc2.cpp:1166-1399) from the per-class per-pattern values that stay on the device behind any class evaluation
// (Shard::site_lik / site_cnt).  The arithmetic is hmm.h; here are its kernels, their launches and the entry points.
//   forward   hmm_segment_kernel   item = (segment of kG sites, row): the row's product over the segment, nothing crosses lanes
//             hmm_combine_kernel   item = (kG blocks, row): the same shape one level up, while more than kG blocks are left
//             hmm_final_kernel     one workgroup: the rows of what is left, e_{N-1}, pi, log — and the host-mapped result record
//   Viterbi   vit_segment_kernel   max-plus block rows;  vit_boundary_kernel: the serial pass over the segment boundaries;
//             vit_path_kernel      every segment again between its entry and exit state, writing its bytes
// Levels are separate launches on shard 0's stream: stream order is the only synchronisation, so the parenthesisation — and with it
// every bit of the result — depends on (n_sites, C) alone.  T and pi travel as kernel arguments (no upload, no staging buffer).
#include "partition.h"

#include "hmm.h"

using namespace hyhip;
using hyhip::hmm::ll;

namespace hyhip {

namespace {

struct HmmParams {
  double T[hmm::kMaxC * hmm::kMaxC];  // [C*C] row-major (Viterbi: logarithms)
  double pi[hmm::kMaxC];
};

// the class values of site i: through the site list (device pattern of the site) out of [C][stride] arrays
template <int C>
struct DevLoad {
  const double *lik;
  const int32_t *cnt;
  const int32_t *sites;
  int64_t stride;
  __host__ __device__ int64_t site(int64_t i) const { return sites[i]; }
  __host__ __device__ void values(int64_t s, double *l, ll *c) const {
#pragma unroll
    for (int m = 0; m < C; m++) {
      l[m] = lik[(size_t)m * stride + s];
      c[m] = cnt[(size_t)m * stride + s];
    }
  }
};
template <int C>
struct HostLoad {
  const double *lik;
  const int64_t *cnt;
  const int64_t *sites;  // or nullptr: site i = pattern i
  int64_t stride;
  __host__ __device__ int64_t site(int64_t i) const { return sites ? sites[i] : i; }
  __host__ __device__ void values(int64_t s, double *l, ll *c) const {
    for (int m = 0; m < C; m++) {
      l[m] = lik[(size_t)m * stride + s];
      c[m] = cnt[(size_t)m * stride + s];
    }
  }
};

constexpr int kBlock = 64;

template <int C>
__global__ __launch_bounds__(kBlock) void hmm_segment_kernel(HmmParams P, DevLoad<C> ld, int64_t n_factors, int64_t n_seg,
                                                             double *__restrict__ Bm, ll *__restrict__ Be) {
  const int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (item >= n_seg * C) return;
  const int64_t g = item / C;
  const int row = (int)(item - g * C);
  const int64_t i0 = g * hmm::kG;
  const int len = (int)(n_factors - i0 < hmm::kG ? n_factors - i0 : hmm::kG);
  hmm::segment_row<C>(P.T, ld, i0, len, row, Bm + (size_t)item * C, Be + item);
}

template <int C>
__global__ __launch_bounds__(kBlock) void hmm_combine_kernel(const double *__restrict__ Bm, const ll *__restrict__ Be, int64_t n_in,
                                                             int64_t n_out, double *__restrict__ Om, ll *__restrict__ Oe) {
  const int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (item >= n_out * C) return;
  const int64_t g = item / C;
  const int row = (int)(item - g * C);
  const int64_t b0 = g * hmm::kG;
  const int nb = (int)(n_in - b0 < hmm::kG ? n_in - b0 : hmm::kG);
  hmm::Row<C> r;
  hmm::combine_row<C>(Bm, Be, b0, nb, row, r);
#pragma unroll
  for (int m = 0; m < C; m++) Om[(size_t)item * C + m] = r.v[m];
  Oe[item] = r.e;
}

// rec: [log L, 0, expm status, sequence word] as every synchronous entry point posts it
template <int C>
__global__ __launch_bounds__(kBlock) void hmm_final_kernel(HmmParams P, DevLoad<C> ld, int64_t n_sites, const double *__restrict__ Bm,
                                                           const ll *__restrict__ Be, int nb, int force_nan, double *__restrict__ rec,
                                                           const int *__restrict__ status, double seq) {
  __shared__ double val[hmm::kMaxC];
  __shared__ ll ex[hmm::kMaxC];
  const int row = (int)threadIdx.x;
  if (row < C) {
    double v;
    ll e;
    hmm::final_row<C>(ld, n_sites, Bm, Be, nb, row, v, e);
    val[row] = v, ex[row] = e;
  }
  __syncthreads();
  if (row == 0) {
    double v[C];
    ll e[C];
#pragma unroll
    for (int r = 0; r < C; r++) v[r] = val[r], e[r] = ex[r];
    rec[0] = force_nan ? NAN : hmm::finish<C>(v, e, P.pi);
    rec[1] = 0.;
    rec[2] = status ? (double)*status : 0.;
    if (seq != 0.) {
      __threadfence_system();
      reinterpret_cast<volatile double *>(rec)[3] = seq;
    }
  }
}

template <int C>
__global__ __launch_bounds__(kBlock) void vit_segment_kernel(HmmParams P, DevLoad<C> ld, int64_t n_sites, int64_t n_seg,
                                                             double *__restrict__ W) {
  const int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (item >= n_seg * C) return;
  const int64_t g = item / C;
  const int row = (int)(item - g * C);
  const int64_t i0 = 1 + g * hmm::kG;
  const int len = (int)(n_sites - i0 < hmm::kG ? n_sites - i0 : hmm::kG);
  hmm::vit_segment_row<C>(P.T, ld, i0, len, row, W + (size_t)item * C);
}

template <int C>
__global__ void vit_boundary_kernel(HmmParams P, DevLoad<C> ld, const double *__restrict__ W, int64_t n_seg, int force_fail,
                                    int8_t *__restrict__ back, int8_t *__restrict__ bnd, int *__restrict__ ok_out,
                                    int8_t *__restrict__ path) {
  double l[C], le[C];
  ll c[C];
  ld.values(ld.site(0), l, c);
  bool ok = hmm::vit_emit<C>(l, c, le) && !force_fail;
  ok = ok && hmm::vit_boundaries<C>(P.pi, le, W, n_seg, back, bnd);
  *ok_out = ok ? 1 : 0;
  path[0] = ok ? bnd[0] : (int8_t)-1;
}

template <int C>
__global__ __launch_bounds__(kBlock) void vit_path_kernel(HmmParams P, DevLoad<C> ld, int64_t n_sites, int64_t n_seg,
                                                          const int8_t *__restrict__ bnd, const int *__restrict__ ok,
                                                          int8_t *__restrict__ path) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n_seg) return;
  const int64_t i0 = 1 + g * hmm::kG;
  const int len = (int)(n_sites - i0 < hmm::kG ? n_sites - i0 : hmm::kG);
  if (!*ok) {
    for (int j = 0; j < len; j++) path[i0 + j] = (int8_t)-1;
    return;
  }
  hmm::vit_segment_path<C>(P.T, ld, i0, len, bnd[g], bnd[g + 1], path);
}

#define HMM_DISPATCH_C(C_, ...)               \
  switch (C_) {                               \
    case 2: { constexpr int CC = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int CC = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int CC = 4; __VA_ARGS__; } break; \
    case 5: { constexpr int CC = 5; __VA_ARGS__; } break; \
    case 6: { constexpr int CC = 6; __VA_ARGS__; } break; \
    case 7: { constexpr int CC = 7; __VA_ARGS__; } break; \
    case 8: { constexpr int CC = 8; __VA_ARGS__; } break; \
    default: break;                           \
  }

unsigned grid_of(int64_t items) { return (unsigned)((items + kBlock - 1) / kBlock); }

// transition / initial: non-negative and finite, or NaN (which the result then is).  -1: an entry is neither
int scan_params(int C, const double *T, const double *pi, bool *has_nan) {
  *has_nan = false;
  for (int k = 0; k < C * C + C; k++) {
    const double x = k < C * C ? T[k] : pi[k - C * C];
    if (x != x) *has_nan = true;
    else if (x < 0. || x == INFINITY) return -1;
  }
  return 0;
}

// ---- the host's run of the same plan --------------------------------------------------------------------------------------------------
template <int C>
void host_forward(const HostLoad<C> &ld, int64_t n_sites, const double *T, const double *pi, bool has_nan, double *logl_out) {
  const hmm::Plan pl = hmm::make_plan(n_sites);
  std::vector<double> Bm((size_t)pl.segments * C * C), Om;
  std::vector<ll> Be((size_t)pl.segments * C), Oe;
  const int64_t n_factors = n_sites - 1;
  for (int64_t g = 0; g < pl.segments; g++)
    for (int row = 0; row < C; row++) {
      const int64_t i0 = g * hmm::kG;
      hmm::segment_row<C>(T, ld, i0, (int)std::min<int64_t>(hmm::kG, n_factors - i0), row, Bm.data() + ((size_t)g * C + row) * C,
                          Be.data() + (size_t)g * C + row);
    }
  int64_t n = pl.segments;
  while (n > hmm::kG) {
    const int64_t n_out = (n + hmm::kG - 1) / hmm::kG;
    Om.assign((size_t)n_out * C * C, 0.), Oe.assign((size_t)n_out * C, 0);
    for (int64_t g = 0; g < n_out; g++)
      for (int row = 0; row < C; row++) {
        hmm::Row<C> r;
        hmm::combine_row<C>(Bm.data(), Be.data(), g * hmm::kG, (int)std::min<int64_t>(hmm::kG, n - g * hmm::kG), row, r);
        for (int m = 0; m < C; m++) Om[((size_t)g * C + row) * C + m] = r.v[m];
        Oe[(size_t)g * C + row] = r.e;
      }
    Bm.swap(Om), Be.swap(Oe);
    n = n_out;
  }
  double val[C];
  ll ex[C];
  for (int row = 0; row < C; row++) hmm::final_row<C>(ld, n_sites, Bm.data(), Be.data(), (int)n, row, val[row], ex[row]);
  *logl_out = has_nan ? NAN : hmm::finish<C>(val, ex, pi);
}

template <int C>
void host_viterbi(const HostLoad<C> &ld, int64_t n_sites, const double *T, const double *pi, bool has_nan, int8_t *path) {
  double logT[C * C], logpi[C];
  for (int k = 0; k < C * C; k++) logT[k] = log(T[k]);
  for (int k = 0; k < C; k++) logpi[k] = log(pi[k]);
  const int64_t n_seg = (n_sites - 1 + hmm::kG - 1) / hmm::kG;
  std::vector<double> W((size_t)n_seg * C * C);
  for (int64_t g = 0; g < n_seg; g++)
    for (int row = 0; row < C; row++) {
      const int64_t i0 = 1 + g * hmm::kG;
      hmm::vit_segment_row<C>(logT, ld, i0, (int)std::min<int64_t>(hmm::kG, n_sites - i0), row, W.data() + ((size_t)g * C + row) * C);
    }
  std::vector<int8_t> back((size_t)n_seg * C + 1), bnd((size_t)n_seg + 1);
  double l[C], le[C];
  ll c[C];
  ld.values(ld.site(0), l, c);
  bool ok = hmm::vit_emit<C>(l, c, le) && !has_nan;
  ok = ok && hmm::vit_boundaries<C>(logpi, le, W.data(), n_seg, back.data(), bnd.data());
  if (!ok) {
    std::fill(path, path + n_sites, (int8_t)-1);
    return;
  }
  path[0] = bnd[0];
  for (int64_t g = 0; g < n_seg; g++) {
    const int64_t i0 = 1 + g * hmm::kG;
    hmm::vit_segment_path<C>(logT, ld, i0, (int)std::min<int64_t>(hmm::kG, n_sites - i0), bnd[(size_t)g], bnd[(size_t)g + 1], path);
  }
}

// ---- the device's --------------------------------------------------------------------------------------------------------------------
struct Events {  // events of one call, destroyed when it returns
  std::vector<hipEvent_t> held;
  ~Events() {
    for (hipEvent_t e : held) (void)hipEventDestroy(e);
  }
};

void set_form(hyphy_hip_partition *p, const hmm::Plan &pl) {
  p->hmm_form = "hmm sites=" + std::to_string(pl.n_sites) + " segments=" + std::to_string(pl.segments) + " levels=" + std::to_string(pl.levels);
  p->last_reduce = {"hmm", 0, false};
}

// The per-class per-pattern values where shard 0's stream can read them as [C][stride], indexed by the partition's internal pattern:
// a single shard's own arrays, else a copy gathered from every shard behind an event on that shard's stream.
int gather_values(hyphy_hip_partition *p, Blocks &blk, Events &evs, const double **lik, const int32_t **cnt, int64_t *stride) {
  Shard &s0 = p->shards[0];
  if (p->shards.size() == 1) {
    *lik = s0.site_lik, *cnt = s0.site_cnt, *stride = s0.S_pad;
    return 0;
  }
  const int64_t C = p->C, S = p->S;
  double *dl = nullptr;
  int32_t *dc = nullptr;
  HIPCHK(hipSetDevice(s0.device));
  HIPCHK(blk.get(&dl, (size_t)C * S));
  HIPCHK(blk.get(&dc, (size_t)C * S));
  for (Shard &s : p->shards) {
    if (s.S <= 0) continue;
    if (&s != &s0) {
      hipEvent_t ev = nullptr;
      HIPCHK(hipSetDevice(s.device));
      HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      evs.held.push_back(ev);
      HIPCHK(hipEventRecord(ev, s.stream));
      HIPCHK(hipSetDevice(s0.device));
      HIPCHK(hipStreamWaitEvent(s0.stream, ev, 0));
    }
    HIPCHK(hipMemcpy2DAsync(dl + s.s0, (size_t)S * sizeof(double), s.site_lik, (size_t)s.S_pad * sizeof(double), (size_t)s.S * sizeof(double),
                            (size_t)C, hipMemcpyDeviceToDevice, s0.stream));
    HIPCHK(hipMemcpy2DAsync(dc + s.s0, (size_t)S * sizeof(int32_t), s.site_cnt, (size_t)s.S_pad * sizeof(int32_t), (size_t)s.S * sizeof(int32_t),
                            (size_t)C, hipMemcpyDeviceToDevice, s0.stream));
  }
  *lik = dl, *cnt = dc, *stride = S;
  return 0;
}

template <int C>
int device_forward(hyphy_hip_partition *p, const HmmParams &P, bool has_nan, double *logl_out) {
  Shard &s0 = p->shards[0];
  Blocks blk;
  Events evs;
  DevLoad<C> ld;
  ld.sites = s0.hmm_sites;
  HIPCHK(hipSetDevice(s0.device));
  if (gather_values(p, blk, evs, &ld.lik, &ld.cnt, &ld.stride)) return -1;
  const int64_t n_sites = p->hmm_n_sites;
  const hmm::Plan pl = hmm::make_plan(n_sites);
  size_t total = 0;
  for (int k = 0; k + 1 < pl.levels; k++) total += (size_t)pl.items[k];
  double *Bm = nullptr;
  ll *Be = nullptr;
  HIPCHK(blk.get(&Bm, total * C * C));
  HIPCHK(blk.get(&Be, total * C));
  int64_t n = pl.segments;
  size_t at = 0;  // first block of the level that is being read
  if (n > 0) hipLaunchKernelGGL(hmm_segment_kernel<C>, dim3(grid_of(n * C)), dim3(kBlock), 0, s0.stream, P, ld, n_sites - 1, n, Bm, Be);
  while (n > hmm::kG) {
    const int64_t n_out = (n + hmm::kG - 1) / hmm::kG;
    hipLaunchKernelGGL(hmm_combine_kernel<C>, dim3(grid_of(n_out * C)), dim3(kBlock), 0, s0.stream, Bm + at * C * C, Be + at * C, n, n_out,
                       Bm + (at + (size_t)n) * C * C, Be + (at + (size_t)n) * C);
    at += (size_t)n;
    n = n_out;
  }
  double *rec = s0.d_hout ? s0.d_hout : s0.out;
  hipLaunchKernelGGL(hmm_final_kernel<C>, dim3(1), dim3(kBlock), 0, s0.stream, P, ld, n_sites, Bm + at * C * C, Be + at * C, (int)n,
                     has_nan ? 1 : 0, rec, (const int *)s0.status, result_seq(s0, rec == s0.d_hout));
  HIPCHK(hipGetLastError());
  for (size_t k = 1; k < p->shards.size(); k++)
    if (post_status_record(p->shards[k])) return -1;
  set_form(p, pl);
  if (collect_status(p)) return -1;
  *logl_out = s0.h_out[0];
  return 0;
}

template <int C>
int device_viterbi(hyphy_hip_partition *p, const HmmParams &P, bool has_nan, int8_t *path_out) {
  Shard &s0 = p->shards[0];
  Blocks blk;
  Events evs;
  DevLoad<C> ld;
  ld.sites = s0.hmm_sites;
  HIPCHK(hipSetDevice(s0.device));
  if (gather_values(p, blk, evs, &ld.lik, &ld.cnt, &ld.stride)) return -1;
  const int64_t n_sites = p->hmm_n_sites;
  const hmm::Plan pl = hmm::make_plan(n_sites);
  const int64_t n_seg = pl.segments;
  double *W = nullptr;
  int8_t *back = nullptr, *bnd = nullptr, *path = nullptr;
  int *ok = nullptr;
  HIPCHK(blk.get(&W, (size_t)n_seg * C * C));
  HIPCHK(blk.get(&back, (size_t)n_seg * C));
  HIPCHK(blk.get(&bnd, (size_t)n_seg + 1));
  HIPCHK(blk.get(&path, (size_t)n_sites));
  HIPCHK(blk.get(&ok, 1));
  if (n_seg > 0) hipLaunchKernelGGL(vit_segment_kernel<C>, dim3(grid_of(n_seg * C)), dim3(kBlock), 0, s0.stream, P, ld, n_sites, n_seg, W);
  hipLaunchKernelGGL(vit_boundary_kernel<C>, dim3(1), dim3(1), 0, s0.stream, P, ld, (const double *)W, n_seg, has_nan ? 1 : 0, back, bnd, ok, path);
  if (n_seg > 0)
    hipLaunchKernelGGL(vit_path_kernel<C>, dim3(grid_of(n_seg)), dim3(kBlock), 0, s0.stream, P, ld, n_sites, n_seg, (const int8_t *)bnd,
                       (const int *)ok, path);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(path_out, path, (size_t)n_sites, hipMemcpyDeviceToHost, s0.stream));
  HIPCHK(hipStreamSynchronize(s0.stream));
  set_form(p, pl);
  return 0;
}

}  // namespace

// What every device entry point refuses, before it touches anything.  0: served; 1: C outside 2..8 (the CPU path); -1: refused
int hmm_check(const hyphy_hip_partition *p, const double *transition, const double *initial, const char *who, bool need_evaluated) {
  const std::string pre = std::string(who) + ": ";
  if (!p) return fail(pre + "partition == NULL");
  if (!transition || !initial) return fail(pre + "transition / initial == NULL");
  if (p->C < hmm::kMinC || p->C > hmm::kMaxC) {
    fail(pre + std::to_string(p->C) + " rate classes: the device serves 2 to 8 (use the CPU path)");
    return 1;
  }
  bool has_nan;
  if (scan_params((int)p->C, transition, initial, &has_nan)) return fail(pre + "transition / initial: an entry is negative or infinite");
  if (p->hmm_n_sites <= 0 || !p->shards[0].hmm_sites) return fail(pre + "no site list (hyphy_hip_hmm_set_sites)");
  if (check_unpinned(p, pre)) return -1;
  if (need_evaluated && check_evaluated(p, pre)) return -1;
  // (the per-pattern values of a class carry the root frequencies of that class's own last evaluation: one class evaluated alone
  //  under new frequencies leaves the others' values behind, and the chain would mix the two)
  for (size_t c = 0; need_evaluated && c < p->pi_stale.size(); c++)
    if (p->pi_stale[c])
      return fail(pre + "the per-pattern values of rate class " + std::to_string(c) +
                  " were combined under other root frequencies than the last evaluation's (evaluate that class again)");
  return 0;
}

// The combine behind the class passes that are queued (or finished) on the shards' streams: log L into *logl_out, or the path
int hmm_combine(hyphy_hip_partition *p, const double *transition, const double *initial, double *logl_out, int8_t *path_out) {
  const int C = (int)p->C;
  HmmParams P;
  memset(&P, 0, sizeof P);
  bool has_nan;
  scan_params(C, transition, initial, &has_nan);
  for (int k = 0; k < C * C; k++) P.T[k] = path_out ? log(transition[k]) : transition[k];
  for (int k = 0; k < C; k++) P.pi[k] = path_out ? log(initial[k]) : initial[k];
  int rc = -1;
  if (path_out) {
    HMM_DISPATCH_C(C, rc = device_viterbi<CC>(p, P, has_nan, path_out));
  } else {
    HMM_DISPATCH_C(C, rc = device_forward<CC>(p, P, has_nan, logl_out));
  }
  return rc;
}

}  // namespace hyhip

extern "C" {

int hyphy_hip_hmm_set_sites(hyphy_hip_partition *p, int64_t n_sites, const int64_t *pattern_of_site) {
  if (!p) return fail("hmm_set_sites: partition == NULL");
  if (n_sites < 1 || n_sites > 2147483647LL) return fail("hmm_set_sites: n_sites must be in 1 .. 2^31-1");
  if (!pattern_of_site && n_sites != p->S) return fail("hmm_set_sites: no list given (site j = pattern j) needs n_sites == S");
  std::vector<int32_t> inv;  // internal pattern of the caller's pattern (empty: the same)
  if (!p->perm.empty()) {
    inv.resize((size_t)p->S);
    for (int64_t j = 0; j < p->S; j++) inv[(size_t)p->perm[(size_t)j]] = (int32_t)j;
  }
  std::vector<int32_t> list((size_t)n_sites);
  for (int64_t i = 0; i < n_sites; i++) {
    const int64_t s = pattern_of_site ? pattern_of_site[i] : i;
    if (s < 0 || s >= p->S) return fail("hmm_set_sites: site " + std::to_string(i) + ": pattern " + std::to_string(s) + " out of range");
    list[(size_t)i] = inv.empty() ? (int32_t)s : inv[(size_t)s];
  }
  if (finish_pending_async(p)) return -1;
  Shard &s0 = p->shards[0];
  HIPCHK(hipSetDevice(s0.device));
  s0.own.drop(s0.hmm_sites, FreeMode::Sync);
  p->hmm_n_sites = 0;
  HIPCHK(s0.own.get(device_block(s0.hmm_sites, list.size() * sizeof(int32_t), "s.hmm_sites")));
  HIPCHK(hipMemcpy(s0.hmm_sites, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  p->hmm_n_sites = n_sites;
  return 0;
}

int hyphy_hip_hmm_logl(hyphy_hip_partition *p, const double *transition, const double *initial, double *logl_out) {
  if (p && !logl_out) return fail("hmm_logl: logl_out == NULL");
  if (const int rc = hmm_check(p, transition, initial, "hmm_logl", true)) return rc;
  if (finish_pending_async(p)) return -1;
  return hmm_combine(p, transition, initial, logl_out, nullptr);
}

int hyphy_hip_hmm_viterbi(hyphy_hip_partition *p, const double *transition, const double *initial, int8_t *path_out) {
  if (p && !path_out) return fail("hmm_viterbi: path_out == NULL");
  if (const int rc = hmm_check(p, transition, initial, "hmm_viterbi", true)) return rc;
  if (finish_pending_async(p)) return -1;
  return hmm_combine(p, transition, initial, nullptr, path_out);
}

int64_t hyphy_hip_plan_hmm(int64_t n_sites, int64_t C, int64_t *out, int64_t cap) {
  if (n_sites < 1 || n_sites > 2147483647LL || C < hmm::kMinC || C > hmm::kMaxC || (cap > 0 && !out)) return -1;
  const hmm::Plan pl = hmm::make_plan(n_sites);
  const int64_t need = 2 + pl.levels;
  for (int64_t k = 0; k < need && k < cap; k++) out[k] = k == 0 ? hmm::kG : k == 1 ? pl.levels : pl.items[k - 2] * (k - 2 < pl.levels - 1 ? C : 1);
  return need;
}

int hyphy_hip_hmm_host(int64_t C, int64_t S, int64_t n_sites, const int64_t *pattern_of_site, const double *lik, const int64_t *cnt,
                       const double *transition, const double *initial, double *logl_out, int8_t *path_out) {
  if (!lik || !cnt || !transition || !initial) return fail("hmm_host: lik / cnt / transition / initial == NULL");
  if (S < 1 || n_sites < 1 || n_sites > 2147483647LL) return fail("hmm_host: S >= 1 and n_sites in 1 .. 2^31-1");
  if (C < hmm::kMinC || C > hmm::kMaxC) {
    fail("hmm_host: " + std::to_string(C) + " rate classes: 2 to 8 are served");
    return 1;
  }
  if (!pattern_of_site && n_sites != S) return fail("hmm_host: no list given (site j = pattern j) needs n_sites == S");
  if (pattern_of_site)
    for (int64_t i = 0; i < n_sites; i++)
      if (pattern_of_site[i] < 0 || pattern_of_site[i] >= S) return fail("hmm_host: site " + std::to_string(i) + ": pattern out of range");
  bool has_nan;
  if (scan_params((int)C, transition, initial, &has_nan)) return fail("hmm_host: transition / initial: an entry is negative or infinite");
  HMM_DISPATCH_C((int)C, {
    const HostLoad<CC> ld{lik, cnt, pattern_of_site, S};
    if (logl_out) host_forward<CC>(ld, n_sites, transition, initial, has_nan, logl_out);
    if (path_out) host_viterbi<CC>(ld, n_sites, transition, initial, has_nan, path_out);
  });
  return 0;
}

}  // extern "C"
