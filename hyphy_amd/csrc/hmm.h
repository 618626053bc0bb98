// Hidden-Markov rate classes: the block algebra of the forward sum and of the Viterbi path, shared by the kernels of
// hmm.hip and by hyphy_hip_hmm_host, which runs the same plan serially.  Only the arithmetic lives here: no memory, no launches.
//
// Forward sum.  L = pi^T [ prod_{i=0}^{N-2} T diag(e_i) ] e_{N-1}, e_i[m] = l[m][s(i)] 2^(-64 c[m][s(i)]).  A running product
// P <- P T diag(e_i) updates every ROW of P on its own, so the unit of work is a Row: C doubles and ONE integer exponent, value
// v[k] 2^e, rescaled by exact powers of two only (ldexp).  A Block is C rows (C*C doubles, C exponents).
//   step        one site: every class value enters with its own 2^64 exponent and the row is put on the exponent of its largest entry
//               (align_row) — not on the smallest exponent among the classes, as the reference's acquireScalerMultiplier logic does:
//               that zeroes a class 17 exponents above another, for good when T is block-diagonal and the row lives in that class
//   mul_block   row x block: terms are aligned PER OUTPUT ROW on the largest term exponent ilogb(v[k]) + b_k over the k with v[k] > 0
//               whose row of the block is not 0 — never on max_k b_k: under a block-diagonal T the rows of one block lie arbitrarily
//               far apart.  CONTRACT (step, mul_block, dot_last, finish alike): a term more than 2^-900 below the largest term of the SAME row is dropped.
//   finish      sum_r pi_r val_r 2^(e_r), aligned on the largest term, then log(mantissa) + exponent ln 2
// An all-zero row carries the exponent kZeroExp (no finite value takes part in an alignment through it).  NaN is never dropped: a
// skipped term is multiplied by 0 and added, so it stays NaN.
//
// Viterbi path.  The same structure in (max, +) on log T[k][m] + log l - 64 ln2 c: vit_step is one site, its packed argmaxes (3 bits
// per state) recover the path inside a segment.  Ties go to the lowest state; comparisons are strict.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#ifndef HMM_HD
#define HMM_HD __host__ __device__ inline
#endif

namespace hyhip {
namespace hmm {

typedef long long ll;

constexpr int kG = 32;                  // sites per segment = blocks per combine (hyphy_hip_plan_hmm reports it)
constexpr int kMinC = 2, kMaxC = 8;
constexpr int kMaxLevels = 16;          // (2^31 sites: 8)
constexpr ll kZeroExp = -(1LL << 60);   // exponent of an all-zero row
constexpr int kDrop = 900;              // mul_block / finish: terms below 2^-kDrop of the row's largest are dropped
constexpr int kPrefetch = 4;            // sites whose values are loaded ahead of the product chain (8 up to 4 classes: prefetch_of)
constexpr int prefetch_of(int C) { return C <= 4 ? 8 : kPrefetch; }
constexpr int blocks_ahead_of(int C) { return C <= 4 ? 4 : 2; }  // blocks whose loads are issued ahead of a chain of products
constexpr double kLn2 = 0.693147180559945309417232121458;

// The launches of a forward sum over n_sites sites: level 0 turns the N-1 factors T diag(e_i) into ceil((N-1)/G) segment blocks
// (segment j: factors [jG, min((j+1)G, N-1))), combine levels turn G consecutive blocks into one while more than G are left, and the
// last level (1 item) multiplies what is left, applies e_{N-1} and pi.  Depends on n_sites alone.
struct Plan {
  int64_t n_sites = 0, segments = 0;
  int levels = 0;
  int64_t items[kMaxLevels] = {0};
};
inline Plan make_plan(int64_t n_sites) {
  Plan pl;
  pl.n_sites = n_sites;
  pl.segments = (n_sites - 1 + kG - 1) / kG;
  int64_t n = pl.segments;
  if (n > 0) pl.items[pl.levels++] = n;
  while (n > kG) {
    n = (n + kG - 1) / kG;
    pl.items[pl.levels++] = n;
  }
  pl.items[pl.levels++] = 1;
  return pl;
}

template <int C>
struct Row {
  double v[C];
  ll e;
};

template <int C>
HMM_HD void unit_row(Row<C> &r, int row) {
#pragma unroll
  for (int k = 0; k < C; k++) r.v[k] = k == row ? 1. : 0.;
  r.e = 0;
}

// largest entry into [1, 2) (exact); an all-zero row gets kZeroExp
template <int C>
HMM_HD void normalise(Row<C> &r) {
  double mx = 0.;
  bool nan = false;
#pragma unroll
  for (int k = 0; k < C; k++) {
    if (r.v[k] > mx) mx = r.v[k];
    nan = nan || r.v[k] != r.v[k];
  }
  if (mx > 0. && mx < INFINITY) {
    const int s = ilogb(mx);
#pragma unroll
    for (int k = 0; k < C; k++) r.v[k] = ldexp(r.v[k], -s);
    r.e += s;
  } else if (mx == 0. && !nan) {
    r.e = kZeroExp;
  }
}

// Entries w[m] 2^(x[m]) of one row, each with an exponent of its own, onto ONE exponent: that of the row's largest entry (exact
// powers of two; an entry more than 2^-kDrop below the largest is dropped, NaN stays NaN).  Returns that exponent, or LLONG_MIN when
// no entry is positive.  x[m] is the exponent to ADD to w[m]'s own (ilogb is taken here).
template <int C>
HMM_HD ll align_row(const double *w, const ll *x_add, double *out) {
  ll x[C], ref = LLONG_MIN;
#pragma unroll
  for (int m = 0; m < C; m++) {
    x[m] = LLONG_MIN;
    if (w[m] > 0. && w[m] < INFINITY && x_add[m] > kZeroExp / 2) {
      x[m] = (ll)ilogb(w[m]) + x_add[m];
      if (x[m] > ref) ref = x[m];
    }
  }
#pragma unroll
  for (int m = 0; m < C; m++) out[m] = (x[m] == LLONG_MIN || x[m] - ref < -kDrop) ? w[m] * 0. : ldexp(w[m], (int)(x_add[m] - ref));
  return ref;
}

// r <- r T diag(e), e[m] = l[m] 2^(-64 c[m]): every class enters with its OWN exponent and the row is put on the exponent of its
// largest entry, so a row that lives in one class alone (block-diagonal T) never sees the other classes' exponents.  The result has
// its largest entry in [1, 2).
template <int C>
HMM_HD void step(Row<C> &r, const double *T, const double *l, const ll *c) {
  double w[C];
  ll xa[C];
  bool nan = false;
#pragma unroll
  for (int m = 0; m < C; m++) {
    double acc = 0.;
#pragma unroll
    for (int k = 0; k < C; k++) acc += r.v[k] * T[k * C + m];
    w[m] = acc * l[m];
    xa[m] = -64 * c[m];
    nan = nan || w[m] != w[m];
  }
  const ll ref = align_row<C>(w, xa, r.v);
  if (ref != LLONG_MIN) r.e += ref;
  else if (!nan) r.e = kZeroExp;
}

// r <- r B, B = (Bm [C*C], Be [C]): row k of B is Bm[k][.] 2^(Be[k])
template <int C>
HMM_HD void mul_block(Row<C> &r, const double *Bm, const ll *Be) {
  ll x[C], ref = LLONG_MIN;
#pragma unroll
  for (int k = 0; k < C; k++) {
    x[k] = LLONG_MIN;
    if (r.v[k] > 0. && r.v[k] < INFINITY && Be[k] > kZeroExp / 2) {
      x[k] = (ll)ilogb(r.v[k]) + Be[k];
      if (x[k] > ref) ref = x[k];
    }
  }
  double a[C];
#pragma unroll
  for (int k = 0; k < C; k++)
    a[k] = (x[k] == LLONG_MIN || x[k] - ref < -kDrop) ? r.v[k] * 0. : ldexp(r.v[k], (int)(Be[k] - ref));
  double w[C];
#pragma unroll
  for (int m = 0; m < C; m++) {
    double acc = 0.;
#pragma unroll
    for (int k = 0; k < C; k++) acc += a[k] * Bm[k * C + m];
    w[m] = acc;
  }
#pragma unroll
  for (int m = 0; m < C; m++) r.v[m] = w[m];
  if (ref != LLONG_MIN) r.e += ref;
  normalise(r);
}

// the last site enters without a transition: val 2^e = r . e_{N-1}, the terms on the exponent of the largest
template <int C>
HMM_HD void dot_last(const Row<C> &r, const double *l, const ll *c, double &val, ll &e) {
  double t[C], a[C];
  ll xa[C];
#pragma unroll
  for (int m = 0; m < C; m++) t[m] = r.v[m] * l[m], xa[m] = -64 * c[m];
  const ll ref = align_row<C>(t, xa, a);
  double acc = 0.;
#pragma unroll
  for (int m = 0; m < C; m++) acc += a[m];
  val = acc;
  e = (ref == LLONG_MIN || r.e <= kZeroExp / 2) ? kZeroExp : r.e + ref;
}

// log sum_r pi[r] val[r] 2^(e[r]);  0 -> -INFINITY, NaN -> NaN
template <int C>
HMM_HD double finish(const double *val, const ll *e, const double *pi) {
  double t[C];
  ll x[C], ref = LLONG_MIN;
#pragma unroll
  for (int r = 0; r < C; r++) {
    t[r] = pi[r] * val[r];
    x[r] = LLONG_MIN;
    if (t[r] > 0. && t[r] < INFINITY && e[r] > kZeroExp / 2) {
      x[r] = (ll)ilogb(t[r]) + e[r];
      if (x[r] > ref) ref = x[r];
    }
  }
  double sum = 0.;
#pragma unroll
  for (int r = 0; r < C; r++) sum += (x[r] == LLONG_MIN || x[r] - ref < -kDrop) ? t[r] * 0. : ldexp(t[r], (int)(e[r] - ref));
  if (sum != sum) return sum;
  if (!(sum > 0.)) return -INFINITY;
  const int s = ilogb(sum);
  return log(ldexp(sum, -s)) + (double)(ref + s) * kLn2;
}

// ---- the work items, over a loader of the class values: ld.site(i) = where site i's values are, ld.values(where, l[C], c[C]) ----------
// Loads do not depend on the product chain, so they are issued ahead of it: the places of a whole segment first, then the values of
// prefetch_of(C) sites in front of their steps (static indices throughout: registers).
// row `row` of the block of the factors [i0, i0 + len), len <= kG
template <int C, typename Load>
HMM_HD void segment_row(const double *T, const Load &ld, int64_t i0, int len, int row, double *out_m, ll *out_e) {
  constexpr int P = prefetch_of(C);
  static_assert(kG % P == 0, "whole chunks");
  Row<C> r;
  unit_row(r, row);
  int64_t at[kG];
#pragma unroll
  for (int j = 0; j < kG; j++) at[j] = ld.site(i0 + (j < len ? j : 0));
#pragma unroll
  for (int j0 = 0; j0 < kG; j0 += P) {
    if (j0 < len) {
      double l[P][C];
      ll c[P][C];
#pragma unroll
      for (int u = 0; u < P; u++) ld.values(at[j0 + u], l[u], c[u]);  // (past the end: site i0 again, not used)
#pragma unroll
      for (int u = 0; u < P; u++)
        if (j0 + u < len) step<C>(r, T, l[u], c[u]);
    }
  }
#pragma unroll
  for (int m = 0; m < C; m++) out_m[m] = r.v[m];
  *out_e = r.e;
}

// row `row` of the product of the blocks [b0, b0 + nb) -> r
template <int C>
HMM_HD void combine_row(const double *Bm, const ll *Be, int64_t b0, int nb, int row, Row<C> &r) {
  constexpr int kAhead = blocks_ahead_of(C);  // (one basic block per kAhead products: their loads move to its top)
  unit_row(r, row);
#pragma unroll kAhead
  for (int b = 0; b < nb; b++) mul_block<C>(r, Bm + (size_t)(b0 + b) * C * C, Be + (size_t)(b0 + b) * C);
}

// row `row` of the whole product times e_{N-1}
template <int C, typename Load>
HMM_HD void final_row(const Load &ld, int64_t n_sites, const double *Bm, const ll *Be, int nb, int row, double &val, ll &e) {
  Row<C> r;
  combine_row<C>(Bm, Be, 0, nb, row, r);
  double l[C];
  ll c[C];
  ld.values(ld.site(n_sites - 1), l, c);
  dot_last<C>(r, l, c, val, e);
}

// ---- Viterbi ------------------------------------------------------------------------------------------------------------------------------
template <int C>
HMM_HD bool vit_emit(const double *l, const ll *c, double *le) {  // false: a value is NaN (or negative)
  bool ok = true;
#pragma unroll
  for (int m = 0; m < C; m++) {
    le[m] = log(l[m]) - 64. * kLn2 * (double)c[m];
    ok = ok && le[m] == le[m];
  }
  return ok;
}

// w'[m] = max_k (w[k] + logT[k][m]) + le[m]; returns the argmaxes, 3 bits per m
template <int C>
HMM_HD unsigned vit_step(double *w, const double *logT, const double *le) {
  double nw[C];
  unsigned bp = 0;
#pragma unroll
  for (int m = 0; m < C; m++) {
    double best = w[0] + logT[m];
    unsigned arg = 0;
#pragma unroll
    for (int k = 1; k < C; k++) {
      const double cand = w[k] + logT[k * C + m];
      if (cand > best) best = cand, arg = (unsigned)k;
    }
    nw[m] = best + le[m];
    bp |= arg << (3 * m);
  }
#pragma unroll
  for (int m = 0; m < C; m++) w[m] = nw[m];
  return bp;
}

// Row `row` of the max-plus block of the sites [i0, i0 + len): best score from state `row` at site i0 - 1 to each state at the last
// site.  A NaN among the values read turns the whole row into NaN (the boundary pass looks for it).
template <int C, typename Load>
HMM_HD void vit_segment_row(const double *logT, const Load &ld, int64_t i0, int len, int row, double *out) {
  double w[C];
#pragma unroll
  for (int k = 0; k < C; k++) w[k] = k == row ? 0. : -INFINITY;
  bool ok = true;
  for (int j = 0; j < len; j++) {
    double l[C], le[C];
    ll c[C];
    ld.values(ld.site(i0 + j), l, c);
    ok = vit_emit<C>(l, c, le) && ok;
    vit_step<C>(w, logT, le);
  }
#pragma unroll
  for (int m = 0; m < C; m++) out[m] = ok ? w[m] : NAN;
}

// The states of the sites [i0, i0 + len) on the best path that leaves state `entry` at site i0 - 1 and is in state `exit_state` at the
// last site: the recursion of vit_segment_row again, with its argmaxes kept (static indices: registers).
template <int C, typename Load>
HMM_HD void vit_segment_path(const double *logT, const Load &ld, int64_t i0, int len, int entry, int exit_state, int8_t *path) {
  double w[C];
#pragma unroll
  for (int k = 0; k < C; k++) w[k] = k == entry ? 0. : -INFINITY;
  unsigned bp[kG];
#pragma unroll
  for (int j = 0; j < kG; j++) {
    bp[j] = 0;
    if (j < len) {
      double l[C], le[C];
      ll c[C];
      ld.values(ld.site(i0 + j), l, c);
      vit_emit<C>(l, c, le);
      bp[j] = vit_step<C>(w, logT, le);
    }
  }
  unsigned z = (unsigned)exit_state;
#pragma unroll
  for (int j = kG - 1; j >= 0; j--)
    if (j < len) {
      path[i0 + j] = (int8_t)z;
      z = (bp[j] >> (3 * z)) & 7u;
    }
}

// The boundary pass, serial: d0[k] = log pi[k] + le_0[k], then one max-plus product per segment block W [n_seg][C*C]; bnd[g] = state
// at the last site before segment g (bnd[0]: site 0), bnd[n_seg] = state of the last site.  back [n_seg][C] is scratch.
// false: no path of positive probability, or a NaN.
template <int C>
HMM_HD bool vit_boundaries(const double *logpi, const double *le0, const double *W, int64_t n_seg, int8_t *back, int8_t *bnd) {
  double d[C];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < C; k++) {
    d[k] = logpi[k] + le0[k];
    ok = ok && d[k] == d[k];
  }
  for (int64_t g = 0; g < n_seg; g++) {
    const double *Wg = W + (size_t)g * C * C;
    double nd[C];
#pragma unroll
    for (int b = 0; b < C; b++) {
      double best = d[0] + Wg[b];
      int arg = 0;
      ok = ok && Wg[b] == Wg[b];
#pragma unroll
      for (int a = 1; a < C; a++) {
        const double cand = d[a] + Wg[a * C + b];
        ok = ok && Wg[a * C + b] == Wg[a * C + b];
        if (cand > best) best = cand, arg = a;
      }
      nd[b] = best;
      back[(size_t)g * C + b] = (int8_t)arg;
    }
#pragma unroll
    for (int b = 0; b < C; b++) d[b] = nd[b];
  }
  double best = d[0];
  int arg = 0;
#pragma unroll
  for (int k = 1; k < C; k++)
    if (d[k] > best) best = d[k], arg = k;
  if (!ok || !(best > -INFINITY)) return false;
  bnd[n_seg] = (int8_t)arg;
  for (int64_t g = n_seg; g-- > 0;) bnd[g] = back[(size_t)g * C + bnd[g + 1]];
  return true;
}

}  // namespace hmm
}  // namespace hyhip
