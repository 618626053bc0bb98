// Sampled ancestral reconstruction — the device counterpart of _TheTree::SampleAncestorsBySequence (src/core/tree.cpp:4086-4205,
// called from likefunc2.cpp:413-436), the `sample == true` mode of ReconstructAncestors (HBL's SampleAncestors).
//
// A draw is (replicate r, site j, internal node n); site j shows pattern s = pattern_of_site[j], which uses the matrices and the stored
// conditionals of rate class c = class_of_pattern[s].  With in_n the stored conditional of node n at pattern s in class c:
//   root (n = I - 1):  w[i] = pi[i] * in_n[i];    otherwise:  w[i] = P_n[state of the parent][i] * in_n[i]       (one rounded product)
//   cum_i = w[0] + ... + w[i] in ascending i, every addition rounded; total = cum_{D-1};  x = u * total
//   state = the smallest i with cum_i >= x and cum_i > 0
// No fused multiply-add, no reassociation: the products and sums below are compiled with contraction off, whatever the build says.
// The 2^64 scaler of a stored conditional multiplies w, total and x alike and is not applied.
// Two deviations from the reference: total == 0 or NaN (an impossible pattern) gives -1 and every descendant of a -1 node is -1 (the
// reference would index row -1); u == 0 picks the first state of positive weight (the reference's `while (totalSum < randVal)`
// returns -1 there).
// Uniforms: the caller's array, or Philox4x32-10 with key = (seed low, seed high), counter = (j, n, r, 0),
// u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53: a draw depends on (seed, r, j, n) only.
//
// 2, 3, 5..64 states (sample_kernel<NW>): the host sorts the sites of a rate class by device pattern; a workgroup of 256 threads takes
// a slice of at most kSlice draws of ONE 16-pattern tile (its sites x the replicates of the chunk; a pattern that owns thousands of
// sites spreads over as many workgroups as it needs) and walks the internal nodes in descending index, parents before children.  Per
// node it stages the node's matrix row-major in LDS from the A-operand image (leading dimension DP + 1: threads read different rows;
// the root stages pi as row 0) and the tile's 16 conditional vectors as [pattern][state] from the fragment layout; each thread then
// takes draws in a strided loop: the parent's state byte, two serial D-loops (total, then the search over the same running sum), one
// byte out to scratch [replicate][node][entry].  A thread reads back only bytes it stored itself.  No hand-off between workgroups;
// every loop is bounded by I, D or the slice.
// 4 states (sample_nuc_kernel): one thread per draw, matrices row-major (Prow), conditionals from the [I][4][S_pad] planes.
// The host scatters the bytes to [replicate][node][site] in the caller's site order.
#include "partition.h"
#include "philox.h"

using namespace hyhip;

namespace hyhip {
namespace {

constexpr int kSlice = 1024;  // draws of a workgroup

struct SampleArgs {
  int NW, D, L, I, S_pad, ntiles;
  int Rc;                    // replicates of the chunk
  int64_t r0;                // its first replicate
  int64_t Ec;                // entries of the chunk (stride of a scratch row)
  const int4 *work;          // [grid] (tile, first entry of the tile in the chunk, its entries, first draw of the slice)
  const int32_t *parent;     // [L+I] internal index of the parent
  const double *Pfrag;       // this class: [B][NW][NKK*64]
  const double *Prow;        // this class: [B][16] (4 states)
  const double *partials;    // this class: [I][ntiles][NKK*64] (4 states: [I][4][S_pad])
  const double *pi;          // [DP] (4 states: [4])
  const int32_t *epat;       // [Ec] pattern (of the shard) of entry e
  const int32_t *esite;      // [Ec] its site, as the caller numbers them
  const double *u;           // [Rc][I][Ec] or nullptr: Philox
  uint64_t seed;
  int8_t *out;               // [Rc][I][Ec]
};

// the draw itself: w[i] = row[i] * in[i * stride]; -1 when nothing has positive weight
__device__ __forceinline__ int draw_state(const double *row, const double *in, int stride, int D, double u) {
#pragma clang fp contract(off)
  double total = 0.;
  for (int i = 0; i < D; i++) total = total + row[i] * in[i * stride];
  const double x = u * total;
  double cum = 0.;
  int st = -1;
  for (int i = 0; i < D; i++) {
    cum = cum + row[i] * in[i * stride];
    if (st < 0 && cum >= x && cum > 0.) st = i;
  }
  return total > 0. ? st : -1;  // (a NaN total compares false)
}

template <int NW>
__global__ __launch_bounds__(256) void sample_kernel(SampleArgs a) {
  constexpr int DP = 16 * NW, LD = DP + 1, TILE = DP * 16;
  __shared__ double Pl[DP * LD];   // [parent state][state]
  __shared__ double cv[16 * LD];   // [pattern of the tile][state]
  const int4 w = a.work[blockIdx.x];
  const int tile = w.x, eb = w.y, ne = w.z, d0 = w.w;
  const int d1 = min(d0 + kSlice, ne * a.Rc);
  const int D = a.D, L = a.L, I = a.I;
  for (int n = I - 1; n >= 0; n--) {
    __syncthreads();  // the previous node's readers of Pl and cv are done
    if (n == I - 1) {
      for (int c = threadIdx.x; c < DP; c += 256) Pl[c] = c < D ? a.pi[c] : 0.;
    } else {
      const double *Pf = a.Pfrag + (size_t)(L + n) * DP * DP;
      for (int idx = threadIdx.x; idx < DP * DP; idx += 256) {
        int row, c;
        frag_image_rc(idx, NW, row, c);
        Pl[row * LD + c] = Pf[idx];
      }
    }
    {
      const double *cf = a.partials + ((size_t)n * a.ntiles + tile) * TILE;
      for (int idx = threadIdx.x; idx < TILE; idx += 256) {  // (one row block: row = pattern of the tile)
        int pat, c;
        frag_image_rc(idx, NW, pat, c);
        cv[pat * LD + c] = cf[idx];
      }
    }
    __syncthreads();
    const int par = n == I - 1 ? 0 : a.parent[L + n];
    for (int d = d0 + (int)threadIdx.x; d < d1; d += 256) {
      const int rr = d / ne;
      const int64_t e = eb + (d - rr * ne);
      int ps = 0;
      if (n != I - 1) ps = a.out[((size_t)rr * I + par) * a.Ec + e];  // (stored by this thread)
      const size_t o = ((size_t)rr * I + n) * a.Ec + e;
      int st = -1;
      if (ps >= 0) {
        const double u = a.u ? a.u[o] : philox_uniform(a.seed, (uint32_t)a.esite[e], (uint32_t)n, (uint32_t)(a.r0 + rr), kPhiloxSample);
        st = draw_state(Pl + ps * LD, cv + (a.epat[e] & 15) * LD, 1, D, u);
      }
      a.out[o] = (int8_t)st;
    }
  }
}

// 4 states: one thread per draw
__global__ __launch_bounds__(256) void sample_nuc_kernel(SampleArgs a) {
  const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= (size_t)a.Rc * a.Ec) return;
  const size_t rr = d / a.Ec;
  const int64_t e = (int64_t)(d - rr * a.Ec);
  const int pat = a.epat[e];
  const int L = a.L, I = a.I;
  for (int n = I - 1; n >= 0; n--) {
    int ps = 0;
    if (n != I - 1) ps = a.out[(rr * I + a.parent[L + n]) * a.Ec + e];
    const size_t o = (rr * I + n) * a.Ec + e;
    int st = -1;
    if (ps >= 0) {
      const double u = a.u ? a.u[o] : philox_uniform(a.seed, (uint32_t)a.esite[e], (uint32_t)n, (uint32_t)(a.r0 + rr), kPhiloxSample);
      const double *row = n == I - 1 ? a.pi : a.Prow + (size_t)(L + n) * 16 + 4 * ps;
      st = draw_state(row, a.partials + (size_t)n * 4 * a.S_pad + pat, a.S_pad, 4, u);
    }
    a.out[o] = (int8_t)st;
  }
}

struct Entry {
  int32_t cls, pat, site;  // rate class, pattern of the shard, site
};

}  // namespace
}  // namespace hyhip

extern "C" {

int hyphy_hip_sample_uniforms(uint64_t seed, int64_t n_rep, int64_t I, int64_t n_sites, double *out) {
  if (n_rep < 0 || I < 0 || n_sites < 0) return fail("sample_uniforms: negative count");
  if (n_rep > INT32_MAX || I > INT32_MAX || n_sites > INT32_MAX) return fail("sample_uniforms: count above 2^31 - 1");
  if (n_rep == 0 || I == 0 || n_sites == 0) return 0;
  if (!out) return fail("sample_uniforms: out == NULL");
  for (int64_t r = 0; r < n_rep; r++)
    for (int64_t n = 0; n < I; n++) {
      double *row = out + ((size_t)r * I + n) * n_sites;
      for (int64_t j = 0; j < n_sites; j++) row[j] = philox_uniform(seed, (uint32_t)j, (uint32_t)n, (uint32_t)r, kPhiloxSample);
    }
  return 0;
}

int hyphy_hip_sample_ancestral(hyphy_hip_partition *p, int64_t n_rep, int64_t n_sites, const int64_t *pattern_of_site,
                               const int64_t *class_of_pattern, uint64_t seed, const double *uniforms, int8_t *states_out) {
  if (!p) return fail("sample_ancestral: partition == NULL");
  if (!states_out) return fail("sample_ancestral: states_out == NULL");
  if (check_unpinned(p, "sample_ancestral: ")) return -1;
  if (n_rep < 0 || n_sites < 0) return fail("sample_ancestral: negative count");
  if (n_rep > INT32_MAX || n_sites > INT32_MAX) return fail("sample_ancestral: count above 2^31 - 1");
  if (n_rep == 0 || n_sites == 0) return 0;
  const int C = (int)p->C;
  const int64_t D = p->D, L = p->L, I = p->I, B = p->B, S = p->S;
  if (!pattern_of_site && n_sites != S)
    return fail("sample_ancestral: without pattern_of_site, n_sites must be the pattern count " + std::to_string(S));
  std::vector<char> used((size_t)C, 0);
  for (int64_t j = 0; j < n_sites; j++) {
    const int64_t s = pattern_of_site ? pattern_of_site[j] : j;
    if (s < 0 || s >= S) return fail("sample_ancestral: site " + std::to_string(j) + ": pattern " + std::to_string(s) + " out of range");
    const int64_t c = class_of_pattern ? class_of_pattern[s] : 0;
    if (c < 0 || c >= C)
      return fail("sample_ancestral: pattern " + std::to_string(s) + ": rate class " + std::to_string(c) + " out of range");
    used[(size_t)c] = 1;
  }
  if (check_evaluated(p, "sample_ancestral: ", &used)) return -1;
  if (uniforms) {
    const size_t total = (size_t)n_rep * I * n_sites;
    for (size_t k = 0; k < total; k++)
      if (!(uniforms[k] >= 0. && uniforms[k] < 1.))
        return fail("sample_ancestral: uniform " + std::to_string(k) + " is outside [0, 1)");
  }
  if (finish_pending_async(p)) return -1;
  for (int c = 0; c < C; c++)
    if (used[(size_t)c] && ensure_resident(p, c)) return -1;
  const int DP = p->DP, NW = p->NW;
  const bool nuc = p->nuc;
  std::vector<int32_t> parent((size_t)(L + I), -1);
  for (int64_t c = 0; c < L + I - 1; c++) parent[(size_t)c] = (int32_t)p->parents[(size_t)c];
  const std::vector<double> pi_pad = padded_pi(p);
  const double budget = sw::scratch_budget(sw::SAMPLE_MB);
  const double draw_bytes = (double)I * (uniforms ? 9. : 1.);  // scratch of one entry and replicate: a byte (and a uniform) per node
  // device pattern (over all shards) of every caller pattern
  std::vector<int64_t> dev_of((size_t)S);
  for (int64_t k = 0; k < S; k++) dev_of[(size_t)caller_pattern(p, k)] = k;
  std::vector<Entry> ent;
  std::vector<int32_t> epat, esite;
  std::vector<int4> tiles, work;  // tiles: (tile, first entry, entries, 0)
  std::vector<double> h_u;
  std::vector<int8_t> h_out;
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    // the sites of this shard by (rate class, pattern of the shard, site)
    ent.clear();
    for (int64_t j = 0; j < n_sites; j++) {
      const int64_t sp = pattern_of_site ? pattern_of_site[j] : j, k = dev_of[(size_t)sp] - s.s0;
      if (k < 0 || k >= s.S) continue;
      ent.push_back(Entry{(int32_t)(class_of_pattern ? class_of_pattern[sp] : 0), (int32_t)k, (int32_t)j});
    }
    if (ent.empty()) continue;
    std::sort(ent.begin(), ent.end(), [](const Entry &x, const Entry &y) {
      return x.cls != y.cls ? x.cls < y.cls : (x.pat != y.pat ? x.pat < y.pat : x.site < y.site);
    });
    Blocks tree;
    int32_t *d_parent = nullptr;
    double *d_pi = nullptr;
    HIPCHK(tree.get(&d_parent, parent.size()));
    HIPCHK(tree.get(&d_pi, pi_pad.size()));
    HIPCHK(hipMemcpyAsync(d_parent, parent.data(), parent.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(d_pi, pi_pad.data(), pi_pad.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
    for (size_t c0 = 0; c0 < ent.size();) {
      const int c = ent[c0].cls;
      size_t c1 = c0;
      while (c1 < ent.size() && ent[c1].cls == c) c1++;
      const size_t E = c1 - c0;
      epat.resize(E), esite.resize(E);
      tiles.clear();
      int max_ne = 0;
      for (size_t e = 0; e < E; e++) {
        epat[e] = ent[c0 + e].pat, esite[e] = ent[c0 + e].site;
        if (tiles.empty() || tiles.back().x != (epat[e] >> 4)) tiles.push_back(make_int4(epat[e] >> 4, (int)e, 0, 0));
        max_ne = std::max(max_ne, ++tiles.back().z);
      }
      c0 = c1;
      // chunks: whole replicates of every tile while they fit the budget, else one replicate of as many tiles as fit (at least one)
      int64_t Rc = 1;
      size_t cap_E = E;
      if (draw_bytes * (double)E <= budget) {
        Rc = (int64_t)std::min<double>((double)n_rep, floor(budget / (draw_bytes * (double)E)));
        Rc = std::max<int64_t>(1, std::min<int64_t>(Rc, (int64_t)(INT32_MAX - kSlice) / max_ne));
      } else {
        cap_E = 0;
        for (size_t t0 = 0; t0 < tiles.size();) {
          size_t t1 = t0 + 1, n_e = (size_t)tiles[t0].z;
          while (t1 < tiles.size() && draw_bytes * (double)(n_e + tiles[t1].z) <= budget) n_e += (size_t)tiles[t1++].z;
          cap_E = std::max(cap_E, n_e);
          t0 = t1;
        }
      }
      Blocks blk;
      int32_t *d_epat = nullptr, *d_esite = nullptr;
      int4 *d_work = nullptr;
      double *d_u = nullptr;
      int8_t *d_out = nullptr;
      const size_t max_work = nuc ? 1 : tiles.size() + (size_t)(((double)Rc * (double)cap_E) / kSlice) + 1;
      HIPCHK(blk.get(&d_epat, E));
      HIPCHK(blk.get(&d_esite, E));
      HIPCHK(blk.get(&d_work, max_work));
      HIPCHK(blk.get(&d_out, (size_t)Rc * I * cap_E));
      if (uniforms) HIPCHK(blk.get(&d_u, (size_t)Rc * I * cap_E));
      HIPCHK(hipMemcpyAsync(d_epat, epat.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
      HIPCHK(hipMemcpyAsync(d_esite, esite.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
      SampleArgs a;
      a.NW = NW, a.D = (int)D, a.L = (int)L, a.I = (int)I, a.S_pad = s.S_pad, a.ntiles = s.ntiles;
      a.work = d_work, a.parent = d_parent;
      a.Pfrag = nuc ? nullptr : s.Pfrag + (size_t)c * B * DP * DP;
      a.Prow = nuc ? s.Prow + (size_t)c * B * 16 : nullptr;
      a.partials = s.partials + (size_t)c * s.partial_stride;
      a.pi = d_pi, a.u = d_u, a.seed = seed, a.out = d_out;
      for (size_t t0 = 0; t0 < tiles.size();) {
        size_t t1 = t0 + 1, Ec = (size_t)tiles[t0].z;
        while (t1 < tiles.size() && Ec + (size_t)tiles[t1].z <= cap_E) Ec += (size_t)tiles[t1++].z;
        const size_t e0 = (size_t)tiles[t0].y;
        a.Ec = (int64_t)Ec, a.epat = d_epat + e0, a.esite = d_esite + e0;
        for (int64_t r0 = 0; r0 < n_rep; r0 += Rc) {
          const int64_t R = std::min(Rc, n_rep - r0);
          a.Rc = (int)R, a.r0 = r0;
          if (uniforms) {
            h_u.resize((size_t)R * I * Ec);
            for (int64_t rn = 0; rn < R * I; rn++) {
              const double *src = uniforms + ((size_t)r0 * I + rn) * n_sites;
              double *dst = h_u.data() + (size_t)rn * Ec;
              for (size_t e = 0; e < Ec; e++) dst[e] = src[esite[e0 + e]];
            }
            HIPCHK(hipMemcpyAsync(d_u, h_u.data(), h_u.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
          }
          if (nuc) {
            const size_t draws = (size_t)R * Ec;
            hipLaunchKernelGGL(sample_nuc_kernel, dim3((unsigned)((draws + 255) / 256)), dim3(256), 0, s.stream, a);
          } else {
            work.clear();
            for (size_t t = t0; t < t1; t++)
              for (int64_t d = 0; d < (int64_t)tiles[t].z * R; d += kSlice)
                work.push_back(make_int4(tiles[t].x, (int)((size_t)tiles[t].y - e0), tiles[t].z, (int)d));
            if (work.size() > max_work) return fail("sample_ancestral: internal: work list larger than planned");
            HIPCHK(hipMemcpyAsync(d_work, work.data(), work.size() * sizeof(int4), hipMemcpyHostToDevice, s.stream));
            LAUNCH_NW(sample_kernel, NW, dim3((unsigned)work.size()), dim3(256), s.stream, a);
          }
          HIPCHK(hipGetLastError());
          // -> [replicate][node][site], the caller's site order
          bool run = true;  // the chunk's sites are consecutive: whole rows move at once
          for (size_t e = 1; e < Ec && run; e++) run = esite[e0 + e] == esite[e0] + (int32_t)e;
          if (run && Ec == (size_t)n_sites) {  // ... and they are all the sites (site = pattern, one class): the rows are the caller's
            HIPCHK(hipMemcpyAsync(states_out + (size_t)r0 * I * n_sites, d_out, (size_t)R * I * Ec, hipMemcpyDeviceToHost, s.stream));
            HIPCHK(hipStreamSynchronize(s.stream));
            continue;
          }
          h_out.resize((size_t)R * I * Ec);
          HIPCHK(hipMemcpyAsync(h_out.data(), d_out, h_out.size(), hipMemcpyDeviceToHost, s.stream));
          HIPCHK(hipStreamSynchronize(s.stream));
          for (int64_t rn = 0; rn < R * I; rn++) {
            const int8_t *src = h_out.data() + (size_t)rn * Ec;
            int8_t *dst = states_out + ((size_t)r0 * I + rn) * n_sites;
            if (run) memcpy(dst + esite[e0], src, Ec);
            else
              for (size_t e = 0; e < Ec; e++) dst[esite[e0 + e]] = src[e];
          }
        }
        t0 = t1;
      }
    }
  }
  return 0;
}

}  // extern "C"
