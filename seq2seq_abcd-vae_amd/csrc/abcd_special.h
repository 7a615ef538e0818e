// abcd_special.h -- device special functions and wave / block reductions
// shared by the sampler kernels (abcd_sampler.hip) and the per-segment scoring
// kernels (abcd_score.hip): both form the Dirichlet prior's digamma terms and
// must round them alike.  The pairwise, span, chain and vocoder kernels take
// their wave reductions and the packed-offset search from here too.
#pragma once
#include "abcd_common.h"

namespace abcd {

// ---- special functions (fp64, x > 0) --------------------------------------
DEV double digamma_d(double x) {
  double r = 0.0;
  while (x < 6.0) { r -= 1.0 / x; x += 1.0; }
  const double f = 1.0 / (x * x);
  return r + log(x) - 0.5 / x -
         f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))));
}
DEV double trigamma_d(double x) {
  double r = 0.0;
  while (x < 6.0) { r += 1.0 / (x * x); x += 1.0; }
  const double f = 1.0 / (x * x);
  return r + 1.0 / x + 0.5 * f +
         (1.0 / x) * f * (1.0 / 6 - f * (1.0 / 30 - f * (1.0 / 42 - f * (1.0 / 30 - f * (5.0 / 66)))));
}

DEV float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
DEV float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
DEV double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The largest v among the `width` lanes (a power of two, aligned) around this
// one and its index i, the lowest index winning a tie; every lane gets the
// result.  A NaN fails every comparison.  Selects with no short-circuit: the
// callers sit on latency chains (span_viterbi's step), where a branch per
// level costs more than the two moves it skips.  The width is a template
// parameter, not an argument: as an argument span_viterbi's gap form measured
// 0.3 to 0.6 % over the tree written out in the kernel, as a parameter it is
// level with it.  chain_kernel keeps its own tree (abcd_chain.hip says why).
template <int width = 64, class T> DEV void wave_argmax(T& v, int& i) {
  for (int o = width >> 1; o > 0; o >>= 1) {
    const T v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    const bool take = (v2 > v) | ((v2 == v) & (i2 < i));
    v = take ? v2 : v;
    i = take ? i2 : i;
  }
}

// Packed time-major rows: the number of steps t with batch_sizes[t] =
// off[t + 1] - off[t] > b, i.e. the length of segment b (batch_sizes is
// non-increasing: a binary search).  Here, not in a feature's own file,
// because the pairwise kernels and the vocoder both need it and both include
// this header; it has nothing to do with the emission tile.
DEV int steps_longer(const int* __restrict__ off, int T, int b) {
  int lo = 0, hi = T;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid + 1] - off[mid] > b) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Block reductions (blockDim = 64 x nw, nw <= 16); `sh` holds 16 doubles.
// Every thread returns the block-wide value.
DEV double block_sum_dd(double v, double* sh) {
  const int nw = blockDim.x >> 6;
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t += sh[i];
  return t;
}
DEV double block_max_dd(double v, double* sh) {
  const int nw = blockDim.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
  for (int i = 1; i < nw; ++i) t = fmax(t, sh[i]);
  return t;
}

}  // namespace abcd
