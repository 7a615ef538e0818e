// abcd_chain.hip -- a hidden Markov model over category sequences.
//
// The K categories are the states, score[n, k] (a row-normalised log
// likelihood of segment n under category k, ops.chain_scores) the emission
// term, log_trans / log_init the chain.  One workgroup owns a
// whole sequence and runs its time loops in a single launch:
//
//   forward    alpha_0 = log_init + score_0,
//              alpha_t+1[j] = score_t+1[j] + logsumexp_i(alpha_t[i] + log_trans[i, j])
//   backward   beta_T-1 = 0, beta_t[i] = logsumexp_j(log_trans[i, j] + score_t+1[j] + beta_t+1[j]),
//              gamma_t = softmax(alpha_t + beta_t),
//              xi_t[i, j] = exp(alpha_t[i] + log_trans[i, j] + score_t+1[j] + beta_t+1[j] - log Z)
//   Viterbi    the same recurrence in the max-plus semiring with back-pointers
//
// Everything is kept in the log domain (a state 90 nats behind in its row, or
// in alpha, still carries the chain when it is the only one allowed).  Every
// vector is renormalised to a maximum of 0 after each step in fp32; what the
// renormalisation takes off is summed in fp64, as are the expected counts and
// the path's log joint.
//
//   chain_kernel<true>   K <= 128: log_trans resident in LDS, row stride K | 1
//                        (odd, so the backward pass's column-wise reads -- lanes
//                        on consecutive rows -- fall on distinct banks, as the
//                        forward pass's row-wise reads do)
//   chain_kernel<false>  K <= 1024: log_trans read from global memory (L2) every step
//   chain_counts         resident: workgroup g's sequences again, from the stored
//                        alpha and score + beta rows, into its slab of fp64 partials
//   chain_counts_tiled   streaming: the K x K entries tiled over the workgroups,
//                        each walking every sequence in order (one slab)
//   chain_reduce         the workgroups' count partials in workgroup order
//
// Workgroup g takes sequences g, g + G, ...: a function of (S, G) alone.  No
// atomics, no device-global word, and no workgroup waits for another.
#include <vector>

#include "abcd_common.h"
#include "abcd_internal.h"
#include "abcd_persist.h"
#include "abcd_special.h"

namespace abcd {

constexpr int CH_MAX_K = 1024;
constexpr int CH_RES_K = 128;     // the largest K of the resident form
constexpr int CH_THREADS = 512;
constexpr int CH_NV = CH_MAX_K / CH_THREADS;  // vector entries per thread
constexpr int CH_NW = CH_THREADS / 64;
constexpr int CH_MAX_WG = 256;
constexpr int CH_Q = CH_RES_K * CH_RES_K / CH_THREADS;  // count accumulators per thread (resident form)
constexpr int CH_BT = 8192;       // back-pointers staged in LDS per chunk of the backtrack
constexpr int CH_TQ = 16;         // count entries per thread of the streaming form
constexpr int CH_OFF_CHUNK = 16384;  // ints per slot of the pinned offset ring
enum { CH_EVID = 1, CH_GAMMA = 2, CH_PATH = 4, CH_COUNTS = 8 };

struct ChainArgs {
  const float* score; long ld_score;
  const int* off; int S, K;
  const float* lt; long ld_trans;
  const float* li;
  double* ev; float* gamma; long ld_gamma;
  int32_t* path; double* pscore;
  float* A;          // N x K: the renormalised log alphas (the backward pass takes the transition's log Z off)
  float* W;          // N x K: score_t + beta_t, what the counts need of the backward pass
  int* deadf;        // S: the sequence has no path
  uint16_t* bp;      // N x K: Viterbi back-pointers
  int32_t* ptmp;     // N: the path when only its score is asked for
  double* pc;        // G x K x K count partials
  double* pi;        // G x K initial-count partials
  int want;
};

// NaN and +inf count as -inf (an excluded entry)
DEV float ch_fin(float x) { return (x > -INFINITY && x < INFINITY) ? x : -INFINITY; }

// (m, s) = (max_i x_i, sum_i exp(x_i - m)) of a strided run of terms in two passes: the maximum first, so the
// exponentials of the second pass do not wait for one another; an all -inf run gives (-inf, 0)
template <class F>
DEV void lse_run(float& m, float& s, int begin, int end, int step, F term) {
  m = -INFINITY;
#pragma unroll 4
  for (int i = begin; i < end; i += step) m = fmaxf(m, term(i));
  const float mm = m > -INFINITY ? m : 0.f;
  s = 0.f;
#pragma unroll 4
  for (int i = begin; i < end; i += step) s += __expf(term(i) - mm);  // arguments <= 0: |error| <= 4e-8 of the largest term
}
DEV void lse_merge(float& m, float& s, float m2, float s2) {
  const float hi = fmaxf(m, m2);
  const float e1 = m > -INFINITY ? expf(m - hi) : 0.f, e2 = m2 > -INFINITY ? expf(m2 - hi) : 0.f;
  s = s * e1 + s2 * e2;
  m = hi;
}

template <bool RES>
__global__ __launch_bounds__(CH_THREADS) void chain_kernel(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float Tl[];  // RES: K rows of stride K | 1
  __shared__ float va[CH_MAX_K], vb[CH_MAX_K], vw[CH_MAX_K], pm[CH_MAX_K], ps[CH_MAX_K];
  __shared__ uint16_t bt[CH_BT];
  __shared__ double red[16];
  __shared__ float am_v[CH_NW];
  __shared__ int am_i[CH_NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, K = a.K, KK = K * K;
  const int ld = K | 1;
  // column passes: thread (r, c) takes columns c, c + CW, ... and rows r, r + R, ...
  const int CW = K <= 64 ? 64 : (K <= 128 ? 128 : (K <= 256 ? 256 : 512)), R = CH_THREADS / CW, c = tid & (CW - 1), r = tid / CW;
  // count entries e = tid + 512 q = i K + j, advanced without a division
  const int di = CH_THREADS / K, dj = CH_THREADS % K, i0 = tid / K, j0 = tid % K;
  const bool want_counts = (a.want & CH_COUNTS) != 0;
  double ia[CH_NV] = {};
  if (RES) {
    for (int e = tid, i = i0, j = j0; e < KK; e += CH_THREADS) {
      Tl[i * ld + j] = ch_fin(a.lt[(long)i * a.ld_trans + j]);
      i += di; j += dj;
      if (j >= K) { j -= K; ++i; }
    }
  }
  __syncthreads();
  auto Tij = [&](int i, int j) -> float {
    if (RES) return Tl[i * ld + j];
    return ch_fin(a.lt[(long)i * a.ld_trans + j]);
  };
  // pm / ps[r K + j]: the partial log-sum-exp over rows r, r + R, ... of va[i] + T(i, j)
  auto col_lse = [&]() {
    for (int j = c; j < K; j += CW) {
      float m, s;
      lse_run(m, s, r, K, R, [&](int i) { return va[i] + Tij(i, j); });
      pm[r * K + j] = m;
      ps[r * K + j] = s;
    }
  };
  auto merged = [&](int j) -> float {  // the R partials in r order
    float m = pm[j], s = ps[j];
    for (int rr = 1; rr < R; ++rr) lse_merge(m, s, pm[rr * K + j], ps[rr * K + j]);
    return m + logf(s);
  };

  for (int sq = blockIdx.x; sq < a.S; sq += gridDim.x) {
    const int r0 = a.off[sq], T = a.off[sq + 1] - r0;
    if (T <= 0) {
      if (tid == 0 && a.ev) a.ev[sq] = 0.0;
      continue;
    }
    __syncthreads();
    bool dead = false;
    // ------------------------------------------------------------ forward
    if (a.want & (CH_EVID | CH_GAMMA | CH_COUNTS)) {
      double cs = 0.0;  // what the renormalisations took off
      for (int t = 0; t < T; ++t) {
        const float* sr = a.score + (long)(r0 + t) * a.ld_score;
        float x[CH_NV], mx = -INFINITY;
        if (t > 0) {
          col_lse();
          __syncthreads();
        }
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) {
            x[n] = ch_fin(sr[j]) + (t == 0 ? ch_fin(a.li[j]) : merged(j));
            mx = fmaxf(mx, x[n]);
          }
        }
        const float bm = (float)block_max_dd((double)mx, red);
        if (!(bm > -INFINITY)) { dead = true; break; }  // uniform
        cs += (double)bm;
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) {
            va[j] = x[n] - bm;
            if (a.A) a.A[(long)(r0 + t) * K + j] = x[n] - bm;
          }
        }
        __syncthreads();
      }
      if (!dead) {
        double se = 0.0;
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) se += exp((double)va[j]);
        }
        se = block_sum_dd(se, red);
        if (tid == 0 && a.ev) a.ev[sq] = cs + log(se);
      }
    }
    // ------------------------------------------------------------ backward
    if (!dead && (a.want & (CH_GAMMA | CH_COUNTS))) {
      {  // the last row: beta = 0, va still holds its alpha
        float u[CH_NV], mx = -INFINITY;
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) {
            u[n] = va[j];
            vb[j] = 0.f;
            mx = fmaxf(mx, u[n]);
          }
        }
        const float bm = (float)block_max_dd((double)mx, red);
        double se = 0.0;
#pragma unroll
        for (int n = 0; n < CH_NV; ++n)
          if (tid + CH_THREADS * n < K) se += (double)expf(u[n] - bm);
        se = block_sum_dd(se, red);
        const float z = bm + (float)log(se);
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) {
            const float g = expf(u[n] - z);
            if (a.gamma) a.gamma[(long)(r0 + T - 1) * a.ld_gamma + j] = g;
            if (T == 1) ia[n] += (double)g;
          }
        }
      }
      for (int t = T - 1; t >= 1; --t) {  // the transition t - 1 -> t
        const float* sr = a.score + (long)(r0 + t) * a.ld_score;
        __syncthreads();  // the previous transition's readers of va / vw are done
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) {
            vw[j] = ch_fin(sr[j]) + vb[j];
            if (want_counts) a.W[(long)(r0 + t) * K + j] = vw[j];
            va[j] = a.A[(long)(r0 + t - 1) * K + j];  // this thread's own store
          }
        }
        __syncthreads();
        // beta_t-1[i] before renormalisation = logsumexp_j(T(i, j) + vw[j])
        if (RES) {  // thread (r, c): rows c, c + CW, ..., columns r, r + R, ...; lanes on consecutive rows
          for (int i = c; i < K; i += CW) {
            float m, s;
            lse_run(m, s, r, K, R, [&](int j) { return Tl[i * ld + j] + vw[j]; });
            pm[r * K + i] = m;
            ps[r * K + i] = s;
          }
        } else {  // one wave per row, its lanes along the row (coalesced)
          for (int i = wv; i < K; i += CH_NW) {
            float m, s;
            lse_run(m, s, lane, K, 64, [&](int j) { return Tij(i, j) + vw[j]; });
            for (int o = 32; o > 0; o >>= 1) {
              const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
              lse_merge(m, s, m2, s2);
            }
            if (lane == 0) pm[i] = m + logf(s);
          }
        }
        __syncthreads();
        float br[CH_NV], u[CH_NV], mxu = -INFINITY, mxb = -INFINITY;
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int i = tid + CH_THREADS * n;
          if (i < K) {
            br[n] = RES ? merged(i) : pm[i];
            u[n] = va[i] + br[n];
            mxu = fmaxf(mxu, u[n]);
            mxb = fmaxf(mxb, br[n]);
          }
        }
        const float bmu = (float)block_max_dd((double)mxu, red);
        const float bmb = (float)block_max_dd((double)mxb, red);
        double se = 0.0;
#pragma unroll
        for (int n = 0; n < CH_NV; ++n)
          if (tid + CH_THREADS * n < K) se += (double)expf(u[n] - bmu);
        se = block_sum_dd(se, red);
        const float z = bmu + (float)log(se);  // log Z of this transition, in the renormalised units
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int i = tid + CH_THREADS * n;
          if (i < K) {
            const float g = expf(u[n] - z);
            if (a.gamma) a.gamma[(long)(r0 + t - 1) * a.ld_gamma + i] = g;
            if (t == 1) ia[n] += (double)g;
            vb[i] = br[n] - bmb;
            if (want_counts) a.A[(long)(r0 + t - 1) * K + i] = va[i] - z;  // chain_counts reads alpha_t-1 - log Z
          }
        }
      }
      __syncthreads();
    }
    // ------------------------------------------------------------ Viterbi
    if (!dead && (a.want & CH_PATH)) {
      for (int t = 0; t < T; ++t) {
        const float* sr = a.score + (long)(r0 + t) * a.ld_score;
        float x[CH_NV], mx = -INFINITY;
        if (t > 0) {
          for (int j = c; j < K; j += CW) {  // ascending rows, strict >: the lowest index of the maximum
            float bv = -INFINITY;
            int bi = 0;
            for (int i = r; i < K; i += R) {
              const float v = va[i] + Tij(i, j);
              if (v > bv) { bv = v; bi = i; }
            }
            pm[r * K + j] = bv;
            ps[r * K + j] = __int_as_float(bi);
          }
          __syncthreads();
        }
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) {
            float base;
            if (t == 0) {
              base = ch_fin(a.li[j]);
            } else {
              base = pm[j];
              int bi = __float_as_int(ps[j]);
              for (int rr = 1; rr < R; ++rr) {
                const float v = pm[rr * K + j];
                const int vi = __float_as_int(ps[rr * K + j]);
                if (v > base || (v == base && vi < bi)) { base = v; bi = vi; }
              }
              a.bp[(long)(r0 + t) * K + j] = (uint16_t)bi;
            }
            x[n] = ch_fin(sr[j]) + base;
            mx = fmaxf(mx, x[n]);
          }
        }
        const float bm = (float)block_max_dd((double)mx, red);
        if (!(bm > -INFINITY)) { dead = true; break; }  // uniform; reached only without a forward pass
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K) va[j] = x[n] - bm;
        }
        __syncthreads();
      }
      if (!dead) {
        // the final state: the lowest index of the maximum
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int n = 0; n < CH_NV; ++n) {
          const int j = tid + CH_THREADS * n;
          if (j < K && va[j] > bv) { bv = va[j]; bi = j; }
        }
        // wave_argmax (abcd_special.h) written out, with a branch: with the selects of the shared form the
        // Viterbi-only call measured 1.2 % slower at K = 128 (1357 against 1339 us) in two sessions
        for (int o = 32; o > 0; o >>= 1) {
          const float v2 = __shfl_xor(bv, o, 64);
          const int i2 = __shfl_xor(bi, o, 64);
          if (v2 > bv || (v2 == bv && i2 < bi)) { bv = v2; bi = i2; }
        }
        if (lane == 0) { am_v[wv] = bv; am_i[wv] = bi; }
        __syncthreads();
        int cur = am_i[0];
        {
          float cv = am_v[0];
          for (int w2 = 1; w2 < CH_NW; ++w2)
            if (am_v[w2] > cv || (am_v[w2] == cv && am_i[w2] < cur)) { cv = am_v[w2]; cur = am_i[w2]; }
        }
        // backtrack: the back-pointer rows in chunks through LDS, one thread walking each chunk
        int32_t* P = a.path ? a.path : a.ptmp;
        const int nb = CH_BT / K;
        for (int hi = T - 1; hi >= 1; hi -= nb) {
          const int lo = max(hi - nb + 1, 1);
          __syncthreads();
          const uint16_t* src = a.bp + (long)(r0 + lo) * K;
          for (int e = tid; e < (hi - lo + 1) * K; e += CH_THREADS) bt[e] = src[e];
          __syncthreads();
          if (tid == 0)
            for (int t = hi; t >= lo; --t) {
              P[r0 + t] = cur;
              cur = bt[(t - lo) * K + cur];
            }
        }
        if (tid == 0) P[r0] = cur;
        __syncthreads();
        if (a.pscore) {  // the path's log joint: its terms in fp64, threads strided over the steps, a fixed tree
          double sc = 0.0;
          for (int t = tid; t < T; t += CH_THREADS) {
            const int p = P[r0 + t];
            const float tr = t == 0 ? ch_fin(a.li[p]) : ch_fin(a.lt[(long)P[r0 + t - 1] * a.ld_trans + p]);
            sc += (double)tr + (double)ch_fin(a.score[(long)(r0 + t) * a.ld_score + p]);
          }
          sc = block_sum_dd(sc, red);
          if (tid == 0) a.pscore[sq] = sc;
        }
      }
    }
    if (want_counts && tid == 0) a.deadf[sq] = dead;
    if (dead) {  // no path through the sequence
      if (tid == 0) {
        if (a.ev) a.ev[sq] = -INFINITY;
        if (a.pscore) a.pscore[sq] = -INFINITY;
      }
      if (a.gamma)
        for (int t = 0; t < T; ++t)
          for (int j = tid; j < K; j += CH_THREADS) a.gamma[(long)(r0 + t) * a.ld_gamma + j] = 0.f;
      if (a.path)
        for (int t = tid; t < T; t += CH_THREADS) a.path[r0 + t] = -1;
    }
  }
  if (want_counts) {
#pragma unroll
    for (int n = 0; n < CH_NV; ++n) {
      const int j = tid + CH_THREADS * n;
      if (j < K) a.pi[(size_t)blockIdx.x * K + j] = ia[n];
    }
  }
}

// The expected transition counts from what the backward pass left: xi_t-1[i, j] = exp(A[t - 1, i] + T(i, j) + W[t, j]).
// A thread owns its entries for the whole launch, so every sum runs in (sequence, step) order in fp64 in registers.
// The two vectors of a step alternate between two LDS images: one barrier per step.
//
// Resident form: workgroup g sums the sequences chain_kernel gave it (g, g + G, ...) into its slab of partials, with
// log_trans in LDS; thread e owns entries e, e + 512, ...
__global__ __launch_bounds__(CH_THREADS) void chain_counts(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float Tl[];
  __shared__ float sa[2][CH_MAX_K], sw[2][CH_MAX_K];
  const int tid = threadIdx.x, K = a.K, KK = K * K, ld = K | 1;
  const int di = CH_THREADS / K, dj = CH_THREADS % K, i0 = tid / K, j0 = tid % K;
  double* pcg = a.pc + (size_t)blockIdx.x * KK;
  double acc[CH_Q];
#pragma unroll
  for (int q = 0; q < CH_Q; ++q) acc[q] = 0.0;
  for (int e = tid, i = i0, j = j0; e < KK; e += CH_THREADS) {
    Tl[i * ld + j] = ch_fin(a.lt[(long)i * a.ld_trans + j]);
    i += di; j += dj;
    if (j >= K) { j -= K; ++i; }
  }
  int k = 0;
  for (int sq = blockIdx.x; sq < a.S; sq += gridDim.x) {
    const int r0 = a.off[sq], T = a.off[sq + 1] - r0;
    if (T < 2 || a.deadf[sq]) continue;  // uniform
    for (int t = 1; t < T; ++t, k ^= 1) {
      for (int j = tid; j < K; j += CH_THREADS) {
        sa[k][j] = a.A[(long)(r0 + t - 1) * K + j];
        sw[k][j] = a.W[(long)(r0 + t) * K + j];
      }
      __syncthreads();  // also: every thread is done with image k as the step before last left it
      int i = i0, j = j0;
#pragma unroll
      for (int q = 0; q < CH_Q; ++q) {  // no early exit: acc[] stays in registers only when fully unrolled
        if (i < K) acc[q] += (double)__expf(sa[k][i] + Tl[i * ld + j] + sw[k][j]);
        i += di; j += dj;
        if (j >= K) { j -= K; ++i; }
      }
    }
  }
  int e = tid;
#pragma unroll
  for (int q = 0; q < CH_Q; ++q) {
    if (e < KK) pcg[e] = acc[q];
    e += CH_THREADS;
  }
}

// Streaming form: the K x K entries are tiled over the workgroups, 512 x 16 each, and every workgroup walks all
// sequences in order: one slab, no partials.  A thread keeps its 16 log_trans entries in registers.
__global__ __launch_bounds__(CH_THREADS) void chain_counts_tiled(ChainArgs a) {
  __shared__ float sa[2][CH_MAX_K], sw[2][CH_MAX_K];
  const int tid = threadIdx.x, K = a.K, KK = K * K;
  const int e0 = blockIdx.x * (CH_THREADS * CH_TQ) + tid;
  int qi[CH_TQ], qj[CH_TQ];
  float tl[CH_TQ];
  double acc[CH_TQ];
#pragma unroll
  for (int q = 0; q < CH_TQ; ++q) {
    const int e = e0 + q * CH_THREADS;
    const bool ok = e < KK;
    qi[q] = ok ? e / K : 0;
    qj[q] = ok ? e - qi[q] * K : 0;
    tl[q] = ok ? ch_fin(a.lt[(long)qi[q] * a.ld_trans + qj[q]]) : -INFINITY;  // -inf: the entry adds exp(-inf) = 0
    acc[q] = 0.0;
  }
  int k = 0;
  for (int sq = 0; sq < a.S; ++sq) {
    const int r0 = a.off[sq], T = a.off[sq + 1] - r0;
    if (T < 2 || a.deadf[sq]) continue;  // uniform
    for (int t = 1; t < T; ++t, k ^= 1) {
      for (int j = tid; j < K; j += CH_THREADS) {
        sa[k][j] = a.A[(long)(r0 + t - 1) * K + j];
        sw[k][j] = a.W[(long)(r0 + t) * K + j];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < CH_TQ; ++q) acc[q] += (double)__expf(sa[k][qi[q]] + tl[q] + sw[k][qj[q]]);
    }
  }
#pragma unroll
  for (int q = 0; q < CH_TQ; ++q) {
    const int e = e0 + q * CH_THREADS;
    if (e < KK) a.pc[e] = acc[q];
  }
}

// the workgroups' partials in workgroup order
__global__ __launch_bounds__(256) void chain_reduce(const double* __restrict__ pc, int Gc,
                                                    const double* __restrict__ pi, int G, int K,
                                                    double* __restrict__ tc, double* __restrict__ ic) {
  const int KK = K * K;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < KK && tc) {
    double s = 0.0;
    for (int g = 0; g < Gc; ++g) s += pc[(size_t)g * KK + e];
    tc[e] = s;
  }
  if (e < K && ic) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += pi[(size_t)g * K + e];
    ic[e] = s;
  }
}

static bool chain_shape_ok(long N, int S, int K) {
  return K >= 1 && K <= CH_MAX_K && N >= 0 && S >= 0 && N * (long)K < (1L << 31);
}

static int chain_workgroups(int K, int S) {
  (void)K;
  return std::max(1, std::min(S, CH_MAX_WG));
}

struct ChainWS {
  int* off;
  float* A;
  uint16_t* bp;
  int32_t* ptmp;
  double *pc, *pi;
  float* W;
  int* deadf;
};
static ChainWS carve_chain(Arena& A, long N, int S, int K, int want) {
  ChainWS w{};
  const size_t nk = (size_t)N * K, G = (size_t)chain_workgroups(K, S);
  w.off = (int*)A.f((size_t)S + 1);
  if (want & (CH_GAMMA | CH_COUNTS)) w.A = A.f(nk);
  if (want & CH_PATH) {
    w.bp = (uint16_t*)A.f((nk + 1) / 2);
    w.ptmp = (int32_t*)A.f((size_t)N);
  }
  if (want & CH_COUNTS) {
    w.pc = A.d((K <= CH_RES_K ? G : 1) * K * K);  // the streaming form tiles the entries: one slab
    w.pi = A.d(G * K);
    w.W = A.f(nk);
    w.deadf = (int*)A.f((size_t)S);
  }
  return w;
}

}  // namespace abcd

using namespace abcd;

extern "C" int abcd_chain_plan(int K, int S, int* resident, int* workgroups) {
  ABCD_REQUIRE(K >= 1 && K <= CH_MAX_K && S >= 0);
  if (resident) *resident = K <= CH_RES_K;
  if (workgroups) *workgroups = chain_workgroups(K, S);
  return 0;
}

extern "C" size_t abcd_chain_workspace_bytes(long N, int S, int K, int want) {
  if (!chain_shape_ok(N, S, K) || want < 0 || want > 15) return 0;
  Arena A(nullptr, 0);
  carve_chain(A, N, S, K, want);
  return A.off + 256;
}

extern "C" int abcd_chain_posterior(const float* score, long ld_score, long N, int K, const int64_t* seq_off, int S,
                                    const float* log_trans, long ld_trans, const float* log_init,
                                    double* log_evidence, float* gamma, long ld_gamma, int32_t* path,
                                    double* path_score, double* trans_counts, double* init_counts, void* ws,
                                    size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(chain_shape_ok(N, S, K) && seq_off);
  ABCD_REQUIRE(seq_off[0] == 0 && seq_off[S] == N);
  for (int s = 0; s < S; ++s) ABCD_REQUIRE(seq_off[s + 1] >= seq_off[s]);
  ABCD_REQUIRE(ld_score >= K && ld_trans >= K && (!gamma || ld_gamma >= K));
  const int want = (log_evidence ? CH_EVID : 0) | (gamma ? CH_GAMMA : 0) | ((path || path_score) ? CH_PATH : 0) |
                   ((trans_counts || init_counts) ? CH_COUNTS : 0);
  ABCD_REQUIRE(!want || (score && log_trans && log_init));
  const size_t need = abcd_chain_workspace_bytes(N, S, K, want);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  if (!want) return 0;
  hipStream_t s = (hipStream_t)stream;
  Arena A(ws, ws_bytes);
  const ChainWS w = carve_chain(A, N, S, K, want);
  ABCD_REQUIRE(A.ok);
  // the offsets through the pinned ring, one slot's worth at a time (no host synchronisation)
  for (int at = 0; at <= S; at += CH_OFF_CHUNK) {
    const int n = std::min(CH_OFF_CHUNK, S + 1 - at);
    std::vector<int> part((size_t)n);
    for (int i = 0; i < n; ++i) part[i] = (int)seq_off[at + i];
    ABCD_TRY((hipError_t)upload_offsets(s, part, w.off + at));
  }
  const int G = chain_workgroups(K, S);
  ChainArgs a{score, ld_score, w.off, S, K, log_trans, ld_trans, log_init, log_evidence, gamma, ld_gamma,
              path, path_score, w.A, w.W, w.deadf, w.bp, w.ptmp, w.pc, w.pi, want};
  if (K <= CH_RES_K) {
    const size_t lds = (size_t)K * (K | 1) * sizeof(float);
    static bool attr = false;
    if (!attr) {
      ABCD_TRY(hipFuncSetAttribute((const void*)chain_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   CH_RES_K * (CH_RES_K | 1) * (int)sizeof(float)));
      ABCD_TRY(hipFuncSetAttribute((const void*)chain_counts, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   CH_RES_K * (CH_RES_K | 1) * (int)sizeof(float)));
      attr = true;
    }
    chain_kernel<true><<<G, CH_THREADS, lds, s>>>(a);
    if (want & CH_COUNTS) chain_counts<<<G, CH_THREADS, lds, s>>>(a);
  } else {
    chain_kernel<false><<<G, CH_THREADS, 0, s>>>(a);
    if (want & CH_COUNTS) chain_counts_tiled<<<cdiv((long)K * K, CH_THREADS * CH_TQ), CH_THREADS, 0, s>>>(a);
  }
  ABCD_CHECK_LAUNCH();
  if (want & CH_COUNTS) {
    chain_reduce<<<cdiv((long)K * K, 256), 256, 0, s>>>(w.pc, K <= CH_RES_K ? G : 1, w.pi, G, K, trans_counts,
                                                              init_counts);
    ABCD_CHECK_LAUNCH();
  }
  return 0;
}
