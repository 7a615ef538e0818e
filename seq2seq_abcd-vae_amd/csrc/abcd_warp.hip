// abcd_warp.hip -- time-warped scoring: align a segment to a prototype.
//
// pair_nll (abcd_pairwise.hip) scores frame t of a segment against step t of a
// prototype.  Here the prototype's steps are the states of a left-to-right HMM
// (DESIGN.md s3.11): frame t is emitted by state a(t), a(0) = 0 and a(t + 1) -
// a(t) is 0, 1 or 2 (stay, step, skip) at a cost of -log_move[m]; the cell cost
// c(t, s) is pair_nll's emission term of frame t under step s plus the
// end-of-segment BCE of step s's logit against frame t's target.
//
//   warp_dp<false>  one workgroup per (segment, prototype): the best alignment's
//                   cost (Viterbi) or -log of the sum over alignments (marginal)
//   warp_dp<true>   one workgroup per segment, for its chosen prototype: the
//                   same Viterbi programme with a back-pointer and the emission
//                   term of every cell kept in the workspace, the backtrack, and
//                   the path's emission / BCE / move costs
//
// A workgroup walks its segment in blocks of 32 frames and, inside a block, the
// states in super-blocks of 128.  The emission terms of a super-block (up to
// four 32 x 32 tiles of abcd_emtile.h: its 32 "rows of x" are the 32 frames,
// its 32 "prototypes" 32 steps of the one prototype, fetched with a row stride
// of P) go to LDS, never to memory; then threads 0 .. 127, one state each, run
// the recurrence over the block's frames in fp64, one barrier per frame.  The
// row D[t0 - 1, .] of the whole state axis lives in LDS between frame blocks;
// the two states a super-block needs from its left neighbour are handed over
// per frame.  Tiles wholly outside the band, above s = 2 t or beyond T_proto
// are not computed, and cells outside them are masked, not read.
//
// Every sum has a fixed order: a frame's F columns as the emission tile sums
// them in fp32; the recurrence in fp64 with the three moves in move order; the
// final states lane-strided in state order, a shuffle tree, the waves in
// order.  All of it is a function of (len_b, T_proto, F, band) and this
// tiling: no atomics, no device-global word, no workgroup waits for another.
#include <climits>
#include <cmath>
#include <vector>

#include "abcd_common.h"
#include "abcd_emtile.h"
#include "abcd_internal.h"
#include "abcd_persist.h"
#include "abcd_special.h"

namespace abcd {

constexpr int WP_SW = 128;         // states per super-block = threads of the recurrence
constexpr int WP_CLD = WP_SW + 8;  // row stride of the emission terms in LDS
constexpr int WP_MAX_T = 4096;     // frames: a path reaches at most 2 T - 1 states, whose fp64 row fits LDS
constexpr int WP_MAX_S = 16383;
constexpr int WP_NOMOVE = 3;       // back-pointer of a cell no path reaches

struct WarpMoves {
  double lm[3];
};

// states any path of a T-frame segment can reach
inline int warp_states(int T, int T_proto) { return std::min(T_proto, 2 * T - 1); }

template <bool PATH>
__global__ __launch_bounds__(256) void warp_dp(const float* __restrict__ X, const float* __restrict__ Y,
                                               const float* __restrict__ MU, long ldm,
                                               const float* __restrict__ LV, long ldl,
                                               const float* __restrict__ OL, const int* __restrict__ off, int T,
                                               int F, int P, int S, WarpMoves mv, int band, int marginal,
                                               float* __restrict__ warp, long ldw,
                                               const int32_t* __restrict__ choice, int32_t* __restrict__ state,
                                               float* __restrict__ path_em, float* __restrict__ path_off,
                                               float* __restrict__ path_move, uint8_t* __restrict__ BP,
                                               float* __restrict__ EC, int Sa) {
  extern __shared__ __attribute__((aligned(16))) double drow[];  // D[t0 - 1, s]: the row above the frame block
  __shared__ EmTile tile;
  __shared__ float C[EM_TR * WP_CLD];             // e(t0 + r, s0 + i) of the super-block
  __shared__ double W[2][WP_SW + 2];              // two rows of D over the super-block; [0], [1]: states s0 - 2, s0 - 1
  __shared__ double halo[2][EM_TR + 1][2];        // rows -1 .. 31 of a super-block's last two states, for its neighbour
  __shared__ float ys[EM_TR];
  __shared__ double redv[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, ti = tid >> 4, tj = tid & 15;
  int b, p;
  if (PATH) {
    b = blockIdx.x;
    p = choice[b];
  } else {
    b = blockIdx.x / P;
    p = blockIdx.x - b * P;
  }
  const int len = steps_longer(off, T, b);
  if (PATH && (p < 0 || p >= P)) {  // a skipped segment: none of its frames is read
    for (int t = tid; t < len; t += 256) state[off[t] + b] = -1;
    if (tid == 0) {
      if (path_em) path_em[b] = INFINITY;
      if (path_off) path_off[b] = INFINITY;
      if (path_move) path_move[b] = INFINITY;
    }
    return;
  }
  const int Sb = min(S, 2 * len - 1);
  const size_t cell0 = PATH ? (size_t)b * (size_t)T * (size_t)Sa : 0;
  for (int s = tid; s < Sb; s += 256) drow[s] = INFINITY;
  const int nch = (F + EM_FC - 1) / EM_FC;
  bool dead = false;  // a frame block without a cell: nothing reaches the end
  for (int t0 = 0; t0 < len && !dead; t0 += EM_TR) {
    const int nf = min(EM_TR, len - t0), tl = t0 + nf - 1;
    const int slo = band >= 0 ? max(0, t0 - band) : 0;
    int shi = min(Sb - 1, 2 * tl);
    if (band >= 0) shi = min(shi, tl + band);
    if (shi < slo) { dead = true; break; }
    int xrow[EM_TR / 4];  // the packed rows of this thread's 8 frames; -1: none
#pragma unroll
    for (int i = 0; i < EM_TR / 4; ++i) {
      const int r = w + 4 * i;
      xrow[i] = r < nf ? off[t0 + r] + b : -1;
    }
    __syncthreads();  // the last block's readers of ys are done
    if (tid < EM_TR) ys[tid] = tid < nf ? Y[off[t0 + tid] + b] : 0.f;
    int hb = 0;
    const int sfirst = slo / WP_SW * WP_SW;
    for (int s0 = sfirst; s0 <= shi; s0 += WP_SW, hb ^= 1) {
      // ---- the emission terms of the super-block's tiles, pipelined as one run of passes
      const int sta = max(s0, slo & ~(EM_TP - 1)), stb = min(s0 + WP_SW - EM_TP, shi & ~(EM_TP - 1));
      const int nit = ((stb - sta) / EM_TP + 1) * nch;
      EmRegs g;
      auto fetch = [&](int it) {
        const int st = sta + it / nch * EM_TP, f = it % nch * EM_FC + lane;
        const bool fin = f < F;
#pragma unroll
        for (int i = 0; i < EM_TR / 4; ++i) {
          g.x[i] = (fin && xrow[i] >= 0) ? X[(long)xrow[i] * F + f] : 0.f;
          const int s = st + w + 4 * i;
          const bool ok = fin && s < S;
          const long row = (long)s * P + p;  // the prototype's steps lie P rows apart
          g.m[i] = ok ? MU[row * ldm + f] : 0.f;
          g.l[i] = ok ? LV[row * ldl + f] : 0.f;
        }
      };
      float q[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
      float csum[EM_TP / 4] = {};
      fetch(0);
      for (int it = 0; it < nit; ++it) {
        const int st = sta + it / nch * EM_TP, c = it % nch, f0 = c * EM_FC, k = it & 1;
        const bool first = c == 0, last = c == nch - 1;
        tile.stage(k, g, csum, w, lane, st, S, f0, F, first, last);
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);  // in flight while this pass is computed
        tile.accumulate(k, q, ti, tj, f0, F, first);
        if (last) {
          const float c0 = tile.cs[k][tj], c1 = tile.cs[k][tj + 16];
          float* cr = C + (2 * ti) * WP_CLD + (st - s0) + tj;
          cr[0] = c0 + 0.5f * q[0][0];
          cr[16] = c1 + 0.5f * q[0][1];
          cr[WP_CLD] = c0 + 0.5f * q[1][0];
          cr[WP_CLD + 16] = c1 + 0.5f * q[1][1];
        }
      }
      __syncthreads();
      // ---- the recurrence: thread i owns state s0 + i
      const int s = s0 + tid;
      const bool mine = tid < WP_SW;
      float v = 0.f, sp = 0.f;
      if (mine) {
        const double d = s < Sb ? drow[s] : (double)INFINITY;
        W[0][2 + tid] = d;
        // row t0 - 1 of the two states to the left.  The block's first super-block has no neighbour that ran:
        // those states come from drow, where the last frame block left row t0 - 1 (state s0 - 1 lies on the
        // band's edge there when t0 - band = s0; the recurrence masks what is outside).  On the block's own
        // rows they are outside the band, so + inf serves (below).
        if (tid < 2)
          W[0][tid] = s0 != sfirst ? halo[hb][0][tid] : s0 > 0 ? drow[s0 - 2 + tid] : (double)INFINITY;
        if (tid >= WP_SW - 2) halo[hb ^ 1][0][tid - (WP_SW - 2)] = d;
        if (s < Sb) {
          v = OL[(long)s * P + p];
          sp = log1pf(__expf(-fabsf(v)));
        }
      }
      __syncthreads();
      for (int r = 0; r < nf; ++r) {
        if (mine) {
          const int t = t0 + r;
          const double* wp = W[r & 1];
          double* wc = W[(r + 1) & 1];
          const bool exists = s < Sb && s <= 2 * t && (band < 0 || abs(s - t) <= band);
          float e = 0.f, o = 0.f;
          double d = INFINITY;
          int m = WP_NOMOVE;
          if (exists) {
            e = C[r * WP_CLD + tid];
            o = fmaxf(v, 0.f) - v * ys[r] + sp;
            const double c = (double)e + (double)o;
            double best;
            if (t == 0) {
              best = s == 0 ? 0.0 : (double)INFINITY;
              m = 0;
            } else {
              double a[3];
#pragma unroll
              for (int k = 0; k < 3; ++k) {
                const int sq = s - k;
                const bool ok = sq >= 0 && (band < 0 || abs(sq - (t - 1)) <= band);
                a[k] = ok ? wp[2 + tid - k] - mv.lm[k] : (double)INFINITY;  // a disabled move: + inf
              }
              best = a[0];
              m = 0;
              if (a[1] < best) { best = a[1]; m = 1; }
              if (a[2] < best) { best = a[2]; m = 2; }
              if (marginal && best < INFINITY)
                best = best - log(exp(best - a[0]) + exp(best - a[1]) + exp(best - a[2]));
            }
            if (best < INFINITY && c < INFINITY) d = c + best;  // a NaN cost fails the comparison
            else m = WP_NOMOVE;
          }
          wc[2 + tid] = d;
          if (tid < 2) wc[tid] = s0 == sfirst ? (double)INFINITY : halo[hb][r + 1][tid];
          if (tid >= WP_SW - 2) halo[hb ^ 1][r + 1][tid - (WP_SW - 2)] = d;
          if (PATH && s < Sb) {
            const size_t at = cell0 + (size_t)t * Sa + s;
            BP[at] = (uint8_t)m;
            EC[at] = e;
          }
        }
        __syncthreads();
      }
      if (mine && s < Sb) drow[s] = W[nf & 1][2 + tid];
      __syncthreads();
    }
  }
  // ---- the last frame's row
  __syncthreads();
  const int te = len - 1;
  double bestv = INFINITY;
  int besti = INT_MAX;
  if (!dead)
    for (int s = tid; s < Sb; s += 256) {
      const bool exists = band < 0 || abs(s - te) <= band;
      const double d = exists ? drow[s] : (double)INFINITY;
      if (d < bestv) { bestv = d; besti = s; }  // ascending s per thread: its lowest state wins a tie
    }
  double nv = -bestv;
  wave_argmax(nv, besti);
  if (lane == 0) { redv[w] = nv; redi[w] = besti; }
  __syncthreads();
  nv = redv[0];
  besti = redi[0];
  for (int i = 1; i < 4; ++i)
    if (redv[i] > nv || (redv[i] == nv && redi[i] < besti)) { nv = redv[i]; besti = redi[i]; }
  bestv = -nv;
  const bool none = !(bestv < INFINITY);
  if (!PATH) {
    double res = bestv;
    if (marginal && !none) {
      double se = 0.0;
      for (int s = tid; s < Sb; s += 256) {
        const bool exists = band < 0 || abs(s - te) <= band;
        if (exists) se += exp(bestv - drow[s]);
      }
      se = wave_sum_d(se);
      __syncthreads();  // everyone has read redv
      if (lane == 0) redv[w] = se;
      __syncthreads();
      se = ((redv[0] + redv[1]) + redv[2]) + redv[3];
      res = bestv - log(se);
    }
    if (tid == 0) warp[(long)b * ldw + p] = none ? INFINITY : (float)res;
    return;
  }
  if (none) {
    for (int t = tid; t < len; t += 256) state[off[t] + b] = -1;
    if (tid == 0) {
      if (path_em) path_em[b] = INFINITY;
      if (path_off) path_off[b] = INFINITY;
      if (path_move) path_move[b] = INFINITY;
    }
    return;
  }
  if (tid != 0) return;
  // the backtrack, then the path's costs in frame order
  double pm = 0.0;
  for (int t = te, s = besti; t >= 0; --t) {
    state[off[t] + b] = s;
    if (t > 0) {
      const int m = BP[cell0 + (size_t)t * Sa + s];
      pm -= mv.lm[m];
      s -= m;
    }
  }
  double pe = 0.0, po = 0.0;
  for (int t = 0; t < len; ++t) {
    const int r = off[t] + b, s = state[r];
    const float v = OL[(long)s * P + p];
    pe += (double)EC[cell0 + (size_t)t * Sa + s];
    po += (double)(fmaxf(v, 0.f) - v * Y[r] + log1pf(__expf(-fabsf(v))));
  }
  if (path_em) path_em[b] = (float)pe;
  if (path_off) path_off[b] = (float)po;
  if (path_move) path_move[b] = (float)pm;
}

static bool warp_shape_ok(int T, int B, int P, int T_proto) {
  return T >= 1 && T <= WP_MAX_T && B >= 1 && P >= 1 && (long)B * P < (1L << 31) && T_proto >= 1 &&
         T_proto <= WP_MAX_S;
}

// -inf disables a move; NaN, +inf and "all three disabled" are errors
static bool warp_moves_ok(const double* lm) {
  if (!lm) return false;
  int live = 0;
  for (int k = 0; k < 3; ++k) {
    if (std::isnan(lm[k]) || lm[k] == INFINITY) return false;
    live += lm[k] > -INFINITY;
  }
  return live > 0;
}

static inline size_t warp_offsets_bytes(int T) { return (((size_t)T + 1) * sizeof(int) + 255) & ~(size_t)255; }

// the dynamic LDS of the longest admissible batch, once per kernel
template <bool PATH>
static int warp_allow_lds() {
  static bool attr = false;
  if (!attr) {
    ABCD_TRY(hipFuncSetAttribute((const void*)warp_dp<PATH>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (2 * WP_MAX_T - 1) * (int)sizeof(double)));
    attr = true;
  }
  return 0;
}

static bool warp_common_ok(const abcd_packed* x, const float* gt_offset, int P, int T_proto, const float* proto_mu,
                           long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                           const double* log_move) {
  if (!(x && x->F >= 1 && x->T >= 1 && x->T <= WP_MAX_T)) return false;
  if (validate_batch(x->batch_sizes, x->T, x->L, x->B) != 0) return false;
  if (!warp_shape_ok(x->T, x->B, P, T_proto)) return false;
  if (!(x->data && gt_offset && proto_mu && proto_lv && proto_offset_logits)) return false;
  if (!(ld_mu >= x->F && ld_lv >= x->F)) return false;
  return warp_moves_ok(log_move);
}

}  // namespace abcd

using namespace abcd;

extern "C" size_t abcd_warp_nll_workspace_bytes(int T, int B, int P, int T_proto) {
  if (!warp_shape_ok(T, B, P, T_proto)) return 0;
  return warp_offsets_bytes(T) + 256;
}

extern "C" int abcd_warp_nll(const abcd_packed* x, const float* gt_offset, int P, int T_proto, const float* proto_mu,
                             long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                             const double* log_move, int band, int marginal, float* warp, long ld_warp, void* ws,
                             size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(warp_common_ok(x, gt_offset, P, T_proto, proto_mu, ld_mu, proto_lv, ld_lv, proto_offset_logits,
                              log_move));
  ABCD_REQUIRE(warp && ld_warp >= P);
  const size_t need = abcd_warp_nll_workspace_bytes(x->T, x->B, P, T_proto);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  const int T = x->T, Sa = warp_states(T, T_proto);
  const std::vector<int> off = step_offsets(x->batch_sizes, T);
  int* doff = (int*)ws;
  ABCD_TRY((hipError_t)upload_offsets(s, off, doff));
  ABCD_TRY((hipError_t)warp_allow_lds<false>());
  WarpMoves mv = {{log_move[0], log_move[1], log_move[2]}};
  const size_t lds = ((size_t)Sa * sizeof(double) + 15) & ~(size_t)15;
  warp_dp<false><<<(unsigned)((long)x->B * P), 256, lds, s>>>(
      x->data, gt_offset, proto_mu, ld_mu, proto_lv, ld_lv, proto_offset_logits, doff, T, x->F, P, T_proto, mv,
      band < 0 ? -1 : band, marginal != 0, warp, ld_warp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
      nullptr, Sa);
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t abcd_warp_path_workspace_bytes(int T, int B, int T_proto) {
  if (!warp_shape_ok(T, B, 1, T_proto)) return 0;
  const size_t cells = (size_t)B * (size_t)T * (size_t)warp_states(T, T_proto);
  return warp_offsets_bytes(T) + ((cells * sizeof(float) + 255) & ~(size_t)255) + cells + 256;
}

extern "C" int abcd_warp_path(const abcd_packed* x, const float* gt_offset, int P, int T_proto, const float* proto_mu,
                              long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                              const double* log_move, int band, const int32_t* choice, int32_t* state,
                              float* path_em, float* path_off, float* path_move, void* ws, size_t ws_bytes,
                              void* stream) {
  ABCD_REQUIRE(warp_common_ok(x, gt_offset, P, T_proto, proto_mu, ld_mu, proto_lv, ld_lv, proto_offset_logits,
                              log_move));
  ABCD_REQUIRE(choice && state);
  const size_t need = abcd_warp_path_workspace_bytes(x->T, x->B, T_proto);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  const int T = x->T, Sa = warp_states(T, T_proto);
  const std::vector<int> off = step_offsets(x->batch_sizes, T);
  int* doff = (int*)ws;
  const size_t cells = (size_t)x->B * (size_t)T * (size_t)Sa;
  float* EC = (float*)((char*)ws + warp_offsets_bytes(T));
  uint8_t* BP = (uint8_t*)EC + ((cells * sizeof(float) + 255) & ~(size_t)255);
  ABCD_TRY((hipError_t)upload_offsets(s, off, doff));
  ABCD_TRY((hipError_t)warp_allow_lds<true>());
  WarpMoves mv = {{log_move[0], log_move[1], log_move[2]}};
  const size_t lds = ((size_t)Sa * sizeof(double) + 15) & ~(size_t)15;
  warp_dp<true><<<(unsigned)x->B, 256, lds, s>>>(x->data, gt_offset, proto_mu, ld_mu, proto_lv, ld_lv,
                                                 proto_offset_logits, doff, T, x->F, P, T_proto, mv,
                                                 band < 0 ? -1 : band, 0, nullptr, 0, choice, state, path_em,
                                                 path_off, path_move, BP, EC, Sa);
  ABCD_CHECK_LAUNCH();
  return 0;
}
