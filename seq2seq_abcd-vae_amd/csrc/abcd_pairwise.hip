// abcd_pairwise.hip -- every segment against every category prototype.
//
// The decoder feeds back its own output and never sees the ground truth, so in
// its deterministic eval form (eps = 0) the emission parameters at step t
// depend on (features, speaker, t) alone: decoding P feature vectors once, as a
// P-row rectangle, gives the per-step mu / log_var / offset logit every segment
// would get under each of them.
//
//   pair_nll        one workgroup per (32 segments x 32 prototypes x 16 steps):
//                   fp64 partials [slice][b][p] of the emission NLL and the
//                   offset BCE
//   pair_reduce     one thread per pair: the slices in slice order, one cast
//   pair_posterior  one wave per segment: log-sum-exp over the prototypes in
//                   fp64, responsibilities, the best prototype
//
// The per-term expressions are those of dec_emission_nll / dec_offset_head
// (abcd_rnn.hip) as seg_losses (abcd_score.hip) repeats them; pair_nll's
// emission half (staging, pipelining, the 2 x 2 accumulation) is the tile of
// abcd_emtile.h, which span_nll (abcd_span.hip) shares.  Every sum has a fixed
// order: a frame's F columns in column order in fp32, the frames of a slice in
// step order in fp64, the slices in slice order in fp64.  No atomics, no
// device-global word, and no workgroup waits for another.
#include <vector>

#include "abcd_common.h"
#include "abcd_emtile.h"
#include "abcd_internal.h"
#include "abcd_persist.h"
#include "abcd_special.h"

namespace abcd {

constexpr int PW_TS = 16;      // steps per time slice: a constant, so a pair's order of sums depends on its length only
constexpr int PW_MAX_T = 16383;   // T + 1 ints fit one slot of the pinned offset ring

// Workgroup (x: prototype tile, y: segment tile, z: time slice), 256 threads,
// over the emission tile of abcd_emtile.h (staging, pipelining, the 2 x 2
// accumulation and the order of sums are described there).  What this kernel
// adds: the tile's rows of x are the packed rows off[t] + b0 + r of step t
// (contiguous), rows with b >= batch_sizes[t] (past the last step they lie
// beyond L) are not read; want_em / want_off switch the two losses; a step's
// offset logits and targets ride along its first pass (one value per thread of
// waves 0 and 1) for the BCE; the frames of a slice join an fp64 sum in step
// order, and the slice's partials go to its slab for pair_reduce.
__global__ __launch_bounds__(256) void pair_nll(const float* __restrict__ X, const float* __restrict__ Y,
                                                const float* __restrict__ MU, long ldm,
                                                const float* __restrict__ LV, long ldl,
                                                const float* __restrict__ OL, const int* __restrict__ off, int T,
                                                int F, int B, int P, int want_em, int want_off,
                                                double* __restrict__ part_em, double* __restrict__ part_off) {
  __shared__ EmTile tile;
  __shared__ float os[2][EM_TP], sps[2][EM_TP], ys[2][EM_TR];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int p0 = blockIdx.x * EM_TP, b0 = blockIdx.y * EM_TR, t0 = blockIdx.z * PW_TS;
  const int len0 = steps_longer(off, T, b0);  // the tile's first segment is its longest
  if (t0 >= len0) return;                     // uniform: pair_reduce never reads this slice of this tile
  const int t1 = min(t0 + PW_TS, len0);
  const int ti = tid >> 4, tj = tid & 15;
  const int nch = want_em ? (F + EM_FC - 1) / EM_FC : 1;  // passes per step
  const int nit = (t1 - t0) * nch;
  EmRegs g;
  float gs;  // the next step's offset logit or target
  auto fetch = [&](int it) {
    const int t = t0 + it / nch, c = it % nch, f = c * EM_FC + lane;
    const int o = off[t], nb = off[t + 1] - o;  // rows b < nb exist at this step
    if (want_em) {
#pragma unroll
      for (int i = 0; i < EM_TR / 4; ++i) {
        const int r = w + 4 * i;
        g.x[i] = (f < F && b0 + r < nb) ? X[(long)(o + b0 + r) * F + f] : 0.f;
      }
      em_fetch_proto(g, MU, ldm, LV, ldl, w, t, p0, P, f, F);
    }
    if (want_off && c == 0) {
      gs = 0.f;
      if (tid < EM_TP) {
        if (p0 + tid < P) gs = OL[(long)t * P + p0 + tid];
      } else if (tid >= 64 && tid < 64 + EM_TR) {
        if (b0 + tid - 64 < nb) gs = Y[o + b0 + tid - 64];
      }
    }
  };
  double em[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, bce[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  float q[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  float csum[EM_TP / 4] = {};
  fetch(0);
  for (int it = 0; it < nit; ++it) {
    const int t = t0 + it / nch, c = it % nch, f0 = c * EM_FC, k = it & 1;
    const bool first = c == 0, last = c == nch - 1;
    if (want_em) tile.stage(k, g, csum, w, lane, p0, P, f0, F, first, last);
    if (want_off && first) {
      if (tid < EM_TP) {
        os[k][tid] = gs;
        sps[k][tid] = log1pf(__expf(-fabsf(gs)));
      } else if (tid >= 64 && tid < 64 + EM_TR) {
        ys[k][tid - 64] = gs;
      }
    }
    __syncthreads();
    if (it + 1 < nit) fetch(it + 1);  // in flight while this pass is computed
    const int nb = off[t + 1] - off[t];
    const bool v0 = b0 + 2 * ti < nb, v1 = b0 + 2 * ti + 1 < nb;
    if (want_em) {
      tile.accumulate(k, q, ti, tj, f0, F, first);
      if (last) {  // the frame is complete: one fp32 value per pair joins the fp64 sum
        const float c0 = tile.cs[k][tj], c1 = tile.cs[k][tj + 16];
        if (v0) {
          em[0][0] += (double)(c0 + 0.5f * q[0][0]);
          em[0][1] += (double)(c1 + 0.5f * q[0][1]);
        }
        if (v1) {
          em[1][0] += (double)(c0 + 0.5f * q[1][0]);
          em[1][1] += (double)(c1 + 0.5f * q[1][1]);
        }
      }
    }
    if (want_off && first) {
      const float xa = os[k][tj], xb = os[k][tj + 16], sa = sps[k][tj], sb = sps[k][tj + 16];
      const float y0 = ys[k][2 * ti], y1 = ys[k][2 * ti + 1];
      if (v0) {
        bce[0][0] += (double)(fmaxf(xa, 0.f) - xa * y0 + sa);
        bce[0][1] += (double)(fmaxf(xb, 0.f) - xb * y0 + sb);
      }
      if (v1) {
        bce[1][0] += (double)(fmaxf(xa, 0.f) - xa * y1 + sa);
        bce[1][1] += (double)(fmaxf(xb, 0.f) - xb * y1 + sb);
      }
    }
  }
  const size_t slab = (size_t)blockIdx.z * (size_t)B * (size_t)P;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int b = b0 + 2 * ti + i;
    if (b >= B) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = p0 + tj + 16 * j;
      if (p >= P) continue;
      const size_t at = slab + (size_t)b * P + p;
      if (want_em) part_em[at] = em[i][j];
      if (want_off) part_off[at] = bce[i][j];
    }
  }
}

// pair (b, p): the slices its tile wrote, in slice order
__global__ __launch_bounds__(256) void pair_reduce(const double* __restrict__ part_em,
                                                   const double* __restrict__ part_off,
                                                   const int* __restrict__ off, int T, int B, int P,
                                                   float* __restrict__ pair_em, float* __restrict__ pair_off,
                                                   long ldp) {
  const long at = (long)blockIdx.x * 256 + threadIdx.x;
  if (at >= (long)B * P) return;
  const int b = (int)(at / P), p = (int)(at - (long)b * P);
  const int ns = (steps_longer(off, T, b / EM_TR * EM_TR) + PW_TS - 1) / PW_TS;
  const size_t slab = (size_t)B * (size_t)P;
  if (pair_em) {
    double s = 0.0;
    for (int k = 0; k < ns; ++k) s += part_em[k * slab + at];
    pair_em[(long)b * ldp + p] = (float)s;
  }
  if (pair_off) {
    double s = 0.0;
    for (int k = 0; k < ns; ++k) s += part_off[k * slab + at];
    pair_off[(long)b * ldp + p] = (float)s;
  }
}

// One wave per row: s[p] = lw[p] - em[b, p] - off[b, p] in fp64.  A prototype
// whose score is NaN or -inf (a NaN or +inf NLL, a NaN or -inf weight) is
// excluded.  Lane-strided passes, shuffle trees: a fixed order.
__global__ __launch_bounds__(256) void pair_posterior(const float* __restrict__ EM, const float* __restrict__ OFF,
                                                      long ldp, int B, int P, const float* __restrict__ LW,
                                                      float* __restrict__ log_ev, int32_t* __restrict__ best,
                                                      float* __restrict__ best_prob, float* __restrict__ resp,
                                                      long ldr) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* em = EM + (long)b * ldp;
  const float* of = OFF ? OFF + (long)b * ldp : nullptr;
  auto score = [&](int p) -> double {
    double s = (LW ? (double)LW[p] : 0.0) - (double)em[p];
    if (of) s -= (double)of[p];
    return s > -INFINITY ? s : -INFINITY;  // NaN and -inf: excluded
  };
  double m = -INFINITY;
  int arg = 0x7fffffff;
  for (int p = lane; p < P; p += 64) {
    const double s = score(p);
    if (s > m) { m = s; arg = p; }  // ascending p per lane: the lowest index of the lane's maximum
  }
  wave_argmax(m, arg);
  const bool none = !(m > -INFINITY);
  double se = 0.0;
  if (!none)
    for (int p = lane; p < P; p += 64) {
      const double s = score(p);
      if (s > -INFINITY) se += exp(s - m);
    }
  se = wave_sum_d(se);
  const double lse = none ? -INFINITY : m + log(se);
  if (resp) {
    float* r = resp + (long)b * ldr;
    for (int p = lane; p < P; p += 64) {
      const double s = score(p);
      r[p] = (none || !(s > -INFINITY)) ? 0.f : (float)exp(s - lse);
    }
  }
  if (lane == 0) {
    if (log_ev) log_ev[b] = (float)lse;
    if (best) best[b] = none ? -1 : arg;
    if (best_prob) best_prob[b] = none ? 0.f : (float)exp(m - lse);
  }
}

constexpr int PAIR_POST_MAX_P = 1 << 20;

}  // namespace abcd

using namespace abcd;

extern "C" size_t abcd_pairwise_nll_workspace_bytes(int T, int B, int P) {
  if (T < 1 || T > PW_MAX_T || B < 1 || P < 1 || (long)B * P >= (1L << 31)) return 0;
  const size_t offb = (((size_t)T + 1) * sizeof(int) + 255) & ~(size_t)255;
  return offb + 2 * (size_t)cdiv(T, PW_TS) * (size_t)B * (size_t)P * sizeof(double) + 256;
}

extern "C" int abcd_pairwise_nll(const abcd_packed* x, const float* gt_offset, int P, int T_proto,
                                 const float* proto_mu, long ld_mu, const float* proto_lv, long ld_lv,
                                 const float* proto_offset_logits, float* pair_em, float* pair_off, long ld_pair,
                                 void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(x && x->F >= 1 && x->T >= 1 && x->T <= PW_MAX_T);
  ABCD_REQUIRE(validate_batch(x->batch_sizes, x->T, x->L, x->B) == 0);
  ABCD_REQUIRE(P >= 1 && T_proto >= x->T && ld_pair >= P && (long)x->B * P < (1L << 31));
  ABCD_REQUIRE((proto_mu == nullptr || ld_mu >= x->F) && (proto_lv == nullptr || ld_lv >= x->F));
  ABCD_REQUIRE(!pair_em || (x->data && proto_mu && proto_lv));
  ABCD_REQUIRE(!pair_off || (gt_offset && proto_offset_logits));
  const size_t need = abcd_pairwise_nll_workspace_bytes(x->T, x->B, P);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  if (!pair_em && !pair_off) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int T = x->T, B = x->B;
  const std::vector<int> off = step_offsets(x->batch_sizes, T);
  int* doff = (int*)ws;
  const size_t offb = (((size_t)T + 1) * sizeof(int) + 255) & ~(size_t)255;
  const int ns = cdiv(T, PW_TS);
  double* part_em = (double*)((char*)ws + offb);
  double* part_off = part_em + (size_t)ns * B * P;
  ABCD_TRY((hipError_t)upload_offsets(s, off, doff));  // pinned ring + async copy: no host synchronisation
  const dim3 grid(cdiv(P, EM_TP), cdiv(B, EM_TR), ns);
  note_dispatch(TK_PAIR_NLL, "pair_nll<%dx%dx%d> grid %dx%dx%d", EM_TR, EM_TP, PW_TS, grid.x, grid.y, grid.z);
  {
    TimedScope ts(s, TK_PAIR_NLL);
    pair_nll<<<grid, 256, 0, s>>>(x->data, gt_offset, proto_mu, ld_mu, proto_lv, ld_lv, proto_offset_logits, doff, T,
                                  x->F, B, P, pair_em != nullptr, pair_off != nullptr, part_em, part_off);
    pair_reduce<<<cdiv((long)B * P, 256), 256, 0, s>>>(part_em, part_off, doff, T, B, P, pair_em, pair_off, ld_pair);
  }
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" int abcd_pair_posterior(const float* pair_em, const float* pair_off, long ld_pair, int B, int P,
                                   const float* log_weight, float* log_evidence, int32_t* best, float* best_prob,
                                   float* resp, long ld_resp, void* stream) {
  ABCD_REQUIRE(pair_em && B >= 1 && P >= 1 && P <= PAIR_POST_MAX_P && ld_pair >= P);
  ABCD_REQUIRE(!resp || ld_resp >= P);
  if (!log_evidence && !best && !best_prob && !resp) return 0;
  hipStream_t s = (hipStream_t)stream;
  note_dispatch(TK_PAIR_POST, "pair_posterior<%d> grid %d", P, cdiv(B, 4));
  {
    TimedScope ts(s, TK_PAIR_POST);
    pair_posterior<<<cdiv(B, 4), 256, 0, s>>>(pair_em, pair_off, ld_pair, B, P, log_weight, log_evidence, best,
                                              best_prob, resp, ld_resp);
  }
  ABCD_CHECK_LAUNCH();
  return 0;
}
