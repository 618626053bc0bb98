// What the passes that score whole-likelihood requests from one outside pass (trials.hip: a replaced matrix; nni.hip: two exchanged
// subtrees) do with a request's per-pattern value once they have it: mix it into the classes before it (mix_in), take the pattern's
// term of the request's total (site_term), leave one record per (request, tile) (put_record), and sum the records of a request in a
// fixed order with compensation (trials_reduce_kernel).  Nothing here joins by order of arrival.  gfx950 only.
#pragma once
#include "combine.h"
#include "devutil.h"
#include "outside.h"

namespace hyhip {
namespace {

struct TrialArgs {      // the trials' own blocks, beside the WalkArgs and the OutsideSlice
  const double *img;    // [n_trials][C] trial matrices: A-operand images (4 states: [16] row-major)
  double *lik;          // [n_trials][S_pad] per pattern: classes mixed so far
  int32_t *cnt;
  double *part_sum;     // [n_trials][part_stride] per (trial, tile): sum_s f_s log l_s, sum_s f_s c_s, flags
  long long *part_cnt;
  int *part_flag;
};

// this class's value (l, exponent e) of pattern q into the mix of the classes before it, aligned on the smaller exponent (the larger
// scale), as MargSink::add of marginal.hip aligns its numerators
__device__ __forceinline__ void mix_in(const OutsideSlice &sl, const TrialArgs &a, size_t q, double &l, int &e) {
  l *= sl.w;
  if (sl.first) return;
  double so, sn;
  e = align_exponents(a.cnt[q], e, so, sn);
  l = a.lik[q] * so + l * sn;
}

// the pattern's term of the trial's total (bc_eval_kernel's rule: 1 a zero likelihood, 2 not a number)
__device__ __forceinline__ void site_term(double l, int e, double f, double &wsum, long long &wcnt, int &wflag) {
  if (f == 0.) return;
  if (l != l || isinf(l)) wflag |= 2;
  else if (l <= 0.) wflag |= 1;
  else {
    wsum += log(l) * f;
    wcnt += (long long)e * (long long)f;
  }
}

// the record of (trial t, tile): the terms of its W lanes summed, written by lane 0
template <int W>
__device__ __forceinline__ void put_record(const OutsideSlice &sl, const TrialArgs &a, int t, int tile, int lane, double wsum,
                                           long long wcnt, int wflag) {
  wsum = wave_sum<W>(wsum), wcnt = wave_sum<W>(wcnt), wflag = wave_or<W>(wflag);
  if (lane == 0) {
    const size_t pq = (size_t)t * sl.part_stride + tile;
    a.part_sum[pq] = wsum;
    a.part_cnt[pq] = wcnt;
    a.part_flag[pq] = wflag;
  }
}

// log-L of trial blockIdx.x = sum_s f_s log l_s - 64 ln2 sum_s f_s c_s from its per-tile partial sums: one wave, fixed order, compensated
__global__ __launch_bounds__(64) void trials_reduce_kernel(double *part_sum, long long *part_cnt, int *part_flag, int n, int stride,
                                                           double *__restrict__ out) {
  const size_t o = (size_t)blockIdx.x * stride;
  double sum, comp;
  long long c;
  int fl;
  combine_range(part_sum + o, part_cnt + o, part_flag + o, n, 0, n, (int)threadIdx.x, sum, comp, c, fl);
  if (threadIdx.x == 0) {
    double r = (sum - comp) - kLogScaler * (double)c;
    if (fl & 2) r = NAN;
    else if (fl & 1) r = -INFINITY;
    out[blockIdx.x] = r;
  }
}

}  // namespace
}  // namespace hyhip
