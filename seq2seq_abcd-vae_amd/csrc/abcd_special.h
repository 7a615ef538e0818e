// abcd_special.h -- device special functions and wave / block reductions
// shared by the sampler kernels (abcd_sampler.hip) and the per-segment scoring
// kernels (abcd_score.hip): both form the Dirichlet prior's digamma terms and
// must round them alike.
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
