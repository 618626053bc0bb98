// Joint maximum-likelihood ancestral reconstruction — the device counterpart of _TheTree::RecoverAncestralSequences
// (src/core/tree.cpp:4209-4510), the max-product (Viterbi) pass behind `ReconstructAncestors (lf)` without MARGINAL.
//
// Per pattern, with the matrices of ONE rate class (the reference's catAssignments):
//   upward, nodes in ascending node code (tree.cpp:4252-4407): the parent's vector m_parent starts at all ones; a leaf with state
//   s >= 0 multiplies column s of its matrix in; any other child with vector v (a leaf's ambiguity row, an internal node's m) is
//   "completely unresolved" when every entry of v is exactly 1.0 (backpointer -1, no contribution), else
//   msg[p] = max_c P[p][c] v[c], arg[p] = the FIRST c that attains it (strict >, starting from 0), and m_parent[p] *= msg[p];
//   root (:4434-4456): all entries exactly 1 -> every node of the pattern is -1, else the first argmax of pi[c] m_root[c];
//   traceback (:4458-4483): state[n] = arg_n[state[parent]], or -1 when the parent is -1.
// Only the argmax is observable, so any rescaling by exact powers of two leaves the result unchanged.  The factors
// of a parent are multiplied in the reference's order (its children in ascending node code: leaves, then internal nodes), as plain
// products (the pass has no additions, so nothing can be contracted), and a vector is multiplied by 2^64 as often as it takes
// whenever its largest entry falls below 2^-64: after EVERY factor multiplied into m_parent and on every msg.  (The reference
// rescales msg once and never the factors of resolved leaves: it underflows on wide polytomies.)
//
// 2, 3, 5..64 states: a workgroup of 256 threads owns four 16-pattern tiles, one per wave, and walks the internal nodes in ascending
// index.  Vectors live in the fragment layout (common.h): lane (g, sl) holds the rows p = 4 kk + g of pattern sl, so the factors
// of a parent multiply lane-locally and a node's msg, stored as it is computed, is what the parent loads.  Per node the workgroup
// stages the node's matrix in LDS once ([c][g][kk]: a lane's rows of a column are contiguous, the 16 lanes of a row group read the
// same address), each wave writes its m as a [c][16] tile, and each lane loops c < D over (one m[c], its NKK rows of column c):
// multiply, compare, two selects.  Backpointers go out as bytes [node][tile][lane][kk] (255: unresolved), msg as doubles
// [node][tile][fragment], both into the chunk's scratch.  After the root the lanes of row group 0 walk the internal nodes downwards
// (state of the parent -> one byte) and write int32 states, 16 consecutive patterns per store; the leaves follow on all four row
// groups.  A leaf with a partial ambiguity code is not staged: its few patterns read the A-operand image from memory, upwards and —
// for the one row the traceback needs — again downwards (the same products, so the same decision; no backpointers of leaves kept).
// 4 states: one thread per pattern, matrices row-major (Prow), the same walk.
// Rate classes: one launch per class over a compacted list of that class's patterns (built on the host); leaf codes are read
// through the list, the output is scattered back on the host.
#include "devutil.h"
#include "partition.h"

using namespace hyhip;

namespace hyhip {
namespace {

struct JointArgs {
  int NW, D, L, I, S_pad;
  int n;                     // patterns of this launch (entries of `list`)
  int tile0, nt, ct;         // first tile of the chunk, its tiles, tiles the scratch holds
  int out_stride;            // n padded to whole tiles
  int do_leaves;
  const int32_t *list;       // [n] pattern (of the shard) of slot k, or nullptr: pattern k
  const int32_t *parent;     // [L+I] internal index of the parent
  const int32_t *kids;       // children of internal node i: kids[kid_off[i] .. kid_off[i+1]), ascending node codes
  const int32_t *kid_off;    // [I+1]
  const double *Pfrag;       // this class: [B][NW][NKK*64] (internal branches, leaves with ambiguity codes)
  const double *PTg;         // this class: [B][DP][NW][4][4] column-gather images (leaves)
  const double *Prow;        // this class: [B][16] row-major (4 states)
  const int16_t *codes;      // [L][S_pad]
  const double *ambig;       // [n_ambig][DP] (4 states: [n_ambig][4])
  const double *pi;          // [DP] (4 states: [4])
  double *msg;               // [I][ct][NKK*64]     (4 states: [I][4][ct*64])
  uint32_t *bp;              // [I][ct][64][NW]     (4 states: [I][ct*64], a byte per parent state)
  int32_t *out;              // [I (+ L)][out_stride]
};

constexpr int kUnresolved = 255;

__device__ __forceinline__ double scale_up(double mx) {  // the power of 2^64 that lifts a largest entry mx to 2^-64 or above
  double sc = 1.0;
  if (mx < kScalerThreshold && mx > 0.0) {
    int k = 0;
    do {
      mx *= kScalerUp;
      sc *= kScalerUp;
      k++;
    } while (mx < kScalerThreshold && k < 15);
  }
  return sc;
}

// max over the four 16-lane rows of a wave (devutil.h: row_sum4)
__device__ __forceinline__ double row_max4(double x) {
  unsigned lo = __double2loint(x), hi = __double2hiint(x);
  u32x2_t a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  x = fmax(__hiloint2double(b[0], a[0]), __hiloint2double(b[1], a[1]));
  lo = __double2loint(x), hi = __double2hiint(x);
  a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return fmax(__hiloint2double(b[0], a[0]), __hiloint2double(b[1], a[1]));
}

// (call with every lane of the wave active; padding rows hold 0)
template <int NKK>
__device__ __forceinline__ void rescale_max(double (&v)[NKK]) {
  double mx = 0.;
#pragma unroll
  for (int kk = 0; kk < NKK; kk++) mx = fmax(mx, v[kk]);
  mx = row_max4(mx);
  if (mx < kScalerThreshold && mx > 0.0) {
    const double sc = scale_up(mx);
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) v[kk] *= sc;
  }
}

// P[row][col] of an A-operand image
template <int NW>
__device__ __forceinline__ double pfrag_at(const double *Pf, int row, int col) {
  return Pf[(row >> 4) * (NW * 256) + frag_index(col >> 2, (col & 3) * 16 + (row & 15))];
}

template <int NW>
__global__ __launch_bounds__(256) void joint_kernel(JointArgs a) {
  constexpr int NKK = 4 * NW, DP = 16 * NW, TILE = NKK * 64;
  __shared__ double Pl[DP * DP];      // [c][g][kk] = P[4 kk + g][c], zero outside D x D
  __shared__ double vt[4][DP * 16];   // per wave: [c][pattern of the tile]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, sl = lane & 15;
  const int tl = blockIdx.x * 4 + wave;  // tile of the chunk
  const bool live = tl < a.nt;           // (a wave without a tile still stages matrices and meets the barriers)
  const int D = a.D, L = a.L, I = a.I;
  const size_t col = (size_t)(a.tile0 + (live ? tl : 0)) * 16 + sl;  // slot of the launch: < out_stride
  const int k = (int)(col < (size_t)a.n ? col : 0);                 // (a padding slot repeats slot 0; the host ignores it)
  const int pat = a.list ? a.list[k] : k;
  double *const vw = vt[wave];
  double *const msg_t = a.msg + (size_t)(live ? tl : 0) * TILE;
  uint32_t *const bp_t = a.bp + ((size_t)(live ? tl : 0) * 64 + lane) * NW;
  const size_t node_msg = (size_t)a.ct * TILE, node_bp = (size_t)a.ct * 64 * NW;
  int root_state = -1;

  for (int n = 0; n < I; n++) {
    double m[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) m[kk] = (4 * kk + g < D) ? 1. : 0.;
    if (live) {
      for (int j = a.kid_off[n]; j < a.kid_off[n + 1]; j++) {
        const int c = a.kids[j];
        double f[NKK];
        if (c >= L) {  // internal child: its stored msg (all ones where it is unresolved)
#pragma unroll
          for (int k2 = 0; k2 < NKK / 2; k2++) {
            const f64x2 x = ld16(msg_t + (size_t)(c - L) * node_msg, (unsigned)(k2 * 64 + lane) * 16u);
            f[2 * k2] = x[0], f[2 * k2 + 1] = x[1];
          }
        } else {
          const int code = (int)a.codes[(size_t)c * a.S_pad + pat];
          if (code >= 0) {
            gather_column<NW>(a.PTg + (size_t)c * DP * DP, code, g, f);
          } else {
            const double *av = a.ambig + (size_t)(-code - 1) * DP;
            const double *Pf = a.Pfrag + (size_t)c * DP * DP;
            bool one = true;
            for (int cc = 0; cc < D; cc++) one = one && av[cc] == 1.0;
#pragma unroll
            for (int kk = 0; kk < NKK; kk++) f[kk] = one ? 1. : 0.;
            if (!one)
              for (int cc = 0; cc < D; cc++) {
                const double vc = av[cc];
#pragma unroll
                for (int kk = 0; kk < NKK; kk++) {
                  const double prod = ((4 * kk + g < D) ? pfrag_at<NW>(Pf, 4 * kk + g, cc) : 0.) * vc;
                  f[kk] = prod > f[kk] ? prod : f[kk];
                }
              }
          }
#pragma unroll
          for (int kk = 0; kk < NKK; kk++) f[kk] = (4 * kk + g < D) ? f[kk] : 0.;
          rescale_max<NKK>(f);
        }
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) m[kk] *= f[kk];
        rescale_max<NKK>(m);
      }
    }
    __syncthreads();  // the previous node's readers of Pl and vt are done
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) vw[(4 * kk + g) * 16 + sl] = m[kk];
    if (n == I - 1) {  // the root: first argmax of pi[c] m_root[c]
      __syncthreads();
      bool one = true;
      double best = 0.;
      int arg = 0;
      for (int c = 0; c < D; c++) {
        const double vc = vw[c * 16 + sl];
        one = one && vc == 1.0;
        const double prod = a.pi[c] * vc;
        if (prod > best) best = prod, arg = c;
      }
      root_state = one ? -1 : arg;
      break;
    }
    {  // stage the matrix of branch L + n
      const double *Pf = a.Pfrag + (size_t)(L + n) * DP * DP;
      for (int idx = threadIdx.x; idx < DP * DP; idx += 256) {
        int row, c;
        frag_image_rc(idx, NW, row, c);
        const double x = Pf[idx];
        Pl[c * DP + (row & 3) * NKK + (row >> 2)] = row < D && c < D ? x : 0.;
      }
    }
    __syncthreads();
    if (live) {
      double best[NKK];
      int arg[NKK];
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) best[kk] = 0., arg[kk] = 0;
      bool one = true;
      for (int c = 0; c < D; c++) {
        const double vc = vw[c * 16 + sl];
        one = one && vc == 1.0;
        const double *pr = Pl + c * DP + g * NKK;
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) {
          const double prod = pr[kk] * vc;
          const bool up = prod > best[kk];
          best[kk] = up ? prod : best[kk];
          arg[kk] = up ? c : arg[kk];
        }
      }
      if (one) {
#pragma unroll
        for (int kk = 0; kk < NKK; kk++) best[kk] = (4 * kk + g < D) ? 1. : 0., arg[kk] = kUnresolved;
      }
      rescale_max<NKK>(best);
#pragma unroll
      for (int k2 = 0; k2 < NKK / 2; k2++)
        st16(msg_t + (size_t)n * node_msg, (unsigned)(k2 * 64 + lane) * 16u, (f64x2){best[2 * k2], best[2 * k2 + 1]});
#pragma unroll
      for (int w = 0; w < NW; w++)
        bp_t[(size_t)n * node_bp + w] = (uint32_t)arg[4 * w] | (uint32_t)arg[4 * w + 1] << 8 | (uint32_t)arg[4 * w + 2] << 16 |
                                       (uint32_t)arg[4 * w + 3] << 24;
    }
  }
  if (!live) return;
  // traceback: a lane reads back the states it stored itself.  The backpointer bytes it reads were stored by other lanes of its wave
  // before the __syncthreads() that precedes the root's read of vt (every path to here passes it after the last bp store): that
  // barrier, which also drains the stores, is what makes them visible.  Keep a barrier between the last bp store and this loop.
  int32_t *const o = a.out + col;
  const size_t os = (size_t)a.out_stride;
  if (g == 0) {
    o[(size_t)(I - 1) * os] = root_state;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(a.bp + (size_t)tl * 64 * NW);
    for (int n = I - 2; n >= 0; n--) {
      const int ps = o[(size_t)a.parent[L + n] * os];
      int st = -1;
      if (ps >= 0) {
        const int b = bytes[(size_t)n * node_bp * 4 + (size_t)((ps & 3) * 16 + sl) * NKK + (ps >> 2)];
        st = b == kUnresolved ? -1 : b;
      }
      o[(size_t)n * os] = st;
    }
  }
  if (!a.do_leaves) return;
  __threadfence_block();  // the other row groups read the states row group 0 stored
  for (int l = g; l < L; l += 4) {
    const int ps = o[(size_t)a.parent[l] * os];
    const int code = (int)a.codes[(size_t)l * a.S_pad + pat];
    int st = -1;
    if (ps >= 0) {
      st = code;
      if (code < 0) {  // the one row the traceback needs, with the products of the upward pass
        const double *av = a.ambig + (size_t)(-code - 1) * DP;
        const double *Pf = a.Pfrag + (size_t)l * DP * DP;
        bool one = true;
        double best = 0.;
        int arg = 0;
        for (int cc = 0; cc < D; cc++) {
          const double vc = av[cc];
          one = one && vc == 1.0;
          const double prod = pfrag_at<NW>(Pf, ps, cc) * vc;
          if (prod > best) best = prod, arg = cc;
        }
        st = one ? -1 : arg;
      }
    }
    o[(size_t)(I + l) * os] = st;
  }
}

// 4 states: one thread per pattern
__global__ __launch_bounds__(256) void joint_nuc_kernel(JointArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;  // slot of the chunk
  if (t >= a.nt * 64) return;
  const size_t col = (size_t)a.tile0 * 64 + t;
  const int k = (int)(col < (size_t)a.n ? col : 0);
  const int pat = a.list ? a.list[k] : k;
  const int L = a.L, I = a.I;
  const size_t cs = (size_t)a.ct * 64;
  int32_t *const o = a.out + col;
  const size_t os = (size_t)a.out_stride;
  int root_state = -1;
  for (int n = 0; n < I; n++) {
    double m[4] = {1., 1., 1., 1.};
    for (int j = a.kid_off[n]; j < a.kid_off[n + 1]; j++) {
      const int c = a.kids[j];
      double f[4];
      if (c >= L) {
        for (int p = 0; p < 4; p++) f[p] = a.msg[((size_t)(c - L) * 4 + p) * cs + t];
      } else {
        const int code = (int)a.codes[(size_t)c * a.S_pad + pat];
        const double *P = a.Prow + (size_t)c * 16;
        if (code >= 0) {
          for (int p = 0; p < 4; p++) f[p] = P[4 * p + code];
        } else {
          const double *av = a.ambig + (size_t)(-code - 1) * 4;
          const bool one = av[0] == 1.0 && av[1] == 1.0 && av[2] == 1.0 && av[3] == 1.0;
          for (int p = 0; p < 4; p++) {
            double best = 0.;
            for (int cc = 0; cc < 4; cc++) {
              const double prod = P[4 * p + cc] * av[cc];
              best = prod > best ? prod : best;
            }
            f[p] = one ? 1. : best;
          }
        }
        const double sc = scale_up(fmax(fmax(f[0], f[1]), fmax(f[2], f[3])));
        for (int p = 0; p < 4; p++) f[p] *= sc;
      }
      for (int p = 0; p < 4; p++) m[p] *= f[p];
      const double sc = scale_up(fmax(fmax(m[0], m[1]), fmax(m[2], m[3])));
      for (int p = 0; p < 4; p++) m[p] *= sc;
    }
    const bool one = m[0] == 1.0 && m[1] == 1.0 && m[2] == 1.0 && m[3] == 1.0;
    if (n == I - 1) {
      double best = 0.;
      int arg = 0;
      for (int c = 0; c < 4; c++) {
        const double prod = a.pi[c] * m[c];
        if (prod > best) best = prod, arg = c;
      }
      root_state = one ? -1 : arg;
      break;
    }
    const double *P = a.Prow + (size_t)(L + n) * 16;
    double best[4];
    uint32_t word = 0;
    for (int p = 0; p < 4; p++) {
      double b = 0.;
      int arg = 0;
      for (int c = 0; c < 4; c++) {
        const double prod = P[4 * p + c] * m[c];
        if (prod > b) b = prod, arg = c;
      }
      best[p] = one ? 1. : b;
      word |= (uint32_t)(one ? kUnresolved : arg) << (8 * p);
    }
    const double sc = scale_up(fmax(fmax(best[0], best[1]), fmax(best[2], best[3])));
    for (int p = 0; p < 4; p++) a.msg[((size_t)n * 4 + p) * cs + t] = best[p] * sc;
    a.bp[(size_t)n * cs + t] = word;
  }
  o[(size_t)(I - 1) * os] = root_state;
  for (int n = I - 2; n >= 0; n--) {
    const int ps = o[(size_t)a.parent[L + n] * os];
    int st = -1;
    if (ps >= 0) {
      const int b = (int)(a.bp[(size_t)n * cs + t] >> (8 * ps) & 255u);
      st = b == kUnresolved ? -1 : b;
    }
    o[(size_t)n * os] = st;
  }
  if (!a.do_leaves) return;
  for (int l = 0; l < L; l++) {
    const int ps = o[(size_t)a.parent[l] * os];
    const int code = (int)a.codes[(size_t)l * a.S_pad + pat];
    int st = -1;
    if (ps >= 0) {
      st = code;
      if (code < 0) {
        const double *av = a.ambig + (size_t)(-code - 1) * 4;
        const double *P = a.Prow + (size_t)l * 16 + 4 * ps;
        const bool one = av[0] == 1.0 && av[1] == 1.0 && av[2] == 1.0 && av[3] == 1.0;
        double best = 0.;
        int arg = 0;
        for (int cc = 0; cc < 4; cc++) {
          const double prod = P[cc] * av[cc];
          if (prod > best) best = prod, arg = cc;
        }
        st = one ? -1 : arg;
      }
    }
    o[(size_t)(I + l) * os] = st;
  }
}

}  // namespace
}  // namespace hyhip

extern "C" {

int hyphy_hip_joint_ancestral(hyphy_hip_partition *p, int do_leaves, const int64_t *class_of_pattern, int64_t *states_out) {
  if (!p) return fail("joint_ancestral: partition == NULL");
  if (!states_out) return fail("joint_ancestral: states_out == NULL");
  if (check_unpinned(p, "joint_ancestral: ")) return -1;
  const int C = (int)p->C;
  const int64_t D = p->D, L = p->L, I = p->I, B = p->B, S = p->S;
  std::vector<char> used((size_t)C, 0);
  if (!class_of_pattern) used[0] = 1;
  else
    for (int64_t i = 0; i < S; i++) {
      const int64_t c = class_of_pattern[i];
      if (c < 0 || c >= C)
        return fail("joint_ancestral: pattern " + std::to_string(i) + ": rate class " + std::to_string(c) + " out of range");
      used[(size_t)c] = 1;
    }
  if (check_evaluated(p, "joint_ancestral: ", &used)) return -1;
  if (finish_pending_async(p)) return -1;
  const int DP = p->DP, NW = p->NW;
  const bool nuc = p->nuc;
  const int64_t rows = I + (do_leaves ? L : 0);
  // the tree: parents, and every internal node's children in ascending node code (the reference's order of factors)
  std::vector<int32_t> parent((size_t)(L + I), -1), kid_off((size_t)I + 1, 0), kids((size_t)(L + I - 1));
  for (int64_t c = 0; c < L + I - 1; c++) {
    parent[(size_t)c] = (int32_t)p->parents[(size_t)c];
    kid_off[(size_t)p->parents[(size_t)c] + 1]++;
  }
  for (int64_t i = 0; i < I; i++) kid_off[(size_t)i + 1] += kid_off[(size_t)i];
  {
    std::vector<int32_t> fill(kid_off.begin(), kid_off.end() - 1);
    for (int64_t c = 0; c < L + I - 1; c++) kids[(size_t)fill[(size_t)p->parents[(size_t)c]]++] = (int32_t)c;
  }
  const std::vector<double> pi_pad = padded_pi(p);
  const double budget = sw::scratch_budget(sw::JOINT_MB);
  const int TP = nuc ? 64 : 16;                                                  // patterns of a tile
  const size_t tile_msg = nuc ? (size_t)4 * 64 : (size_t)16 * DP;                // doubles of one node's msg per tile
  const size_t tile_bp = nuc ? (size_t)64 : (size_t)64 * NW;                     // words of its backpointers
  const double tile_bytes = (double)I * (tile_msg * sizeof(double) + tile_bp * sizeof(uint32_t));
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    Blocks tree;
    int32_t *d_parent = nullptr, *d_kids = nullptr, *d_off = nullptr;
    double *d_pi = nullptr;
    HIPCHK(tree.get(&d_parent, parent.size()));
    HIPCHK(tree.get(&d_kids, kids.size()));
    HIPCHK(tree.get(&d_off, kid_off.size()));
    HIPCHK(tree.get(&d_pi, pi_pad.size()));
    HIPCHK(hipMemcpyAsync(d_parent, parent.data(), parent.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(d_kids, kids.data(), kids.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(d_off, kid_off.data(), kid_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(d_pi, pi_pad.data(), pi_pad.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
    std::vector<int32_t> list, h_out;
    for (int c = 0; c < C; c++) {
      if (!used[(size_t)c]) continue;
      list.clear();
      if (class_of_pattern && C > 1) {
        for (int64_t j = 0; j < s.S; j++)
          if (class_of_pattern[caller_pattern(p, s.s0 + j)] == c) list.push_back((int32_t)j);
        if (list.empty()) continue;
      }
      const int64_t n = list.empty() ? s.S : (int64_t)list.size();
      if (n <= 0) continue;
      const int ntiles = (int)((n + TP - 1) / TP);
      const int ct = (int)std::min<double>(ntiles, std::max(1., floor(budget / tile_bytes)));
      const size_t npad = (size_t)ntiles * TP;
      Blocks blk;
      int32_t *d_list = nullptr, *d_out = nullptr;
      double *d_msg = nullptr;
      uint32_t *d_bp = nullptr;
      if (!list.empty()) {
        HIPCHK(blk.get(&d_list, list.size()));
        HIPCHK(hipMemcpyAsync(d_list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
      }
      HIPCHK(blk.get(&d_msg, (size_t)I * ct * tile_msg));
      HIPCHK(blk.get(&d_bp, (size_t)I * ct * tile_bp));
      HIPCHK(blk.get(&d_out, (size_t)rows * npad));
      JointArgs a;
      a.NW = NW, a.D = (int)D, a.L = (int)L, a.I = (int)I, a.S_pad = s.S_pad;
      a.n = (int)n, a.ct = ct, a.out_stride = (int)npad, a.do_leaves = do_leaves ? 1 : 0;
      a.list = d_list, a.parent = d_parent, a.kids = d_kids, a.kid_off = d_off;
      a.Pfrag = nuc ? nullptr : s.Pfrag + (size_t)c * B * DP * DP;
      a.PTg = nuc ? nullptr : s.PTg + (size_t)c * B * DP * DP;
      a.Prow = nuc ? s.Prow + (size_t)c * B * 16 : nullptr;
      a.codes = s.codes, a.ambig = s.ambig, a.pi = d_pi;
      a.msg = d_msg, a.bp = d_bp, a.out = d_out;
      for (int tile0 = 0; tile0 < ntiles; tile0 += ct) {
        a.tile0 = tile0, a.nt = std::min(ct, ntiles - tile0);
        const dim3 grid((unsigned)((a.nt + 3) / 4)), block(256);
        if (nuc) hipLaunchKernelGGL(joint_nuc_kernel, grid, block, 0, s.stream, a);
        else LAUNCH_NW(joint_kernel, NW, grid, block, s.stream, a);
        HIPCHK(hipGetLastError());
      }
      h_out.resize((size_t)rows * npad);
      HIPCHK(hipMemcpyAsync(h_out.data(), d_out, h_out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
      HIPCHK(hipStreamSynchronize(s.stream));
      rows_to_caller(p, s, h_out.data(), npad, rows, n, states_out, list.empty() ? nullptr : list.data());
    }
  }
  return 0;
}

}  // extern "C"
