// abcd_warppost.hip -- posteriors under the time-warped cut:
// the sum half of abcd_warpseg.hip.  A forward-backward over (frame, category
// k, prototype step s) in fp64 on abcd_frame_costs' plane, every maximum of the
// best-path programme replaced by a log-sum-exp:
//
//   warp_post_fwd   frames n0 .. n1 - 1 ascending: aU, aX, aW and G into the
//                   lattice, the aH row carried (and kept, when asked for),
//                   log_z at n1 = N
//   warp_post_bwd   frames n1 - 1 .. n0 descending: bU, bW into the lattice, the
//                   bA row carried, the expected counts in frame order; at n0 =
//                   0 bG, the posteriors and the counts
//
// The recurrences are written out in include/abcd_hip.h.  One workgroup of
// 1024 threads, abcd_warpseg.hip's (r, k) grid; no atomics, no device-global
// word, no workgroup waits for another.
//
// Measured on one MI355X at N = 15 000, K = 128, T_proto = 200, F = 129
// (profiles/warppost_bench.json): warp_post_fwd 81.2 us per
// frame, warp_post_bwd 101.2 without counts, 108.4 with the bigram counts,
// 129.6 with the move counts, against 52.4 us per frame of warp_seg on the same
// plane.  Up to four fp64 exp and a log per cell and sweep behind warp_seg's
// loads and barriers; no counter was collected.
#include <algorithm>
#include <climits>
#include <cmath>

#include "abcd_common.h"
#include "abcd_internal.h"

namespace abcd {

constexpr int WP_THREADS = 1024;
constexpr int WP_RES_K = 128;  // log_trans resident in LDS (K rows of K + 1 floats) up to here
constexpr int WP_MAX_K = 1024;
constexpr int WP_MAX_T = 16383;

// both kernels: five K vectors, the pairs, the move parts, the matrix
static size_t warp_post_lds(int K) {
  return (size_t)K * 5 * sizeof(double) + (size_t)WP_THREADS * 5 * sizeof(double) +
         (K <= WP_RES_K ? (size_t)K * (K + 1) * sizeof(float) : 0);
}

DEV double wp_softplus(double v) { return fmax(v, 0.0) + log1p(exp(-fabs(v))); }

// log(e^a + e^b); -inf when neither is above -inf (NaN counts as -inf)
DEV double wp_lae(double a, double b) {
  const bool va = a > -INFINITY, vb = b > -INFINITY;
  if (!va) return vb ? b : -INFINITY;
  if (!vb) return a;
  const double hi = fmax(a, b), lo = fmin(a, b);
  return hi + log1p(exp(lo - hi));
}

// (maximum, sum of exp(c - maximum)) with candidate c folded in; c = NaN or -inf: excluded
DEV void wp_fold(double& m, double& z, double c) {
  if (c > -INFINITY) {
    const double w = exp(-fabs(m - c));  // m = -inf: 0
    if (c > m) { z = z * w + 1.0; m = c; } else z += w;
  }
}

// the parts pairs of k at pm / pz [i K + k], joined in order; -inf over none
DEV double wp_join(const double* pm, const double* pz, int parts, int K, int k) {
  double M = -INFINITY;
  for (int i = 0; i < parts; ++i) M = fmax(M, pm[i * K + k]);
  if (!(M > -INFINITY)) return -INFINITY;
  double Z = 0.0;
  for (int i = 0; i < parts; ++i) Z += pz[i * K + k] * exp(pm[i * K + k] - M);  // an empty pair: 0 * 0
  return M + log(Z);
}

// LSE of up to four candidates in argument order; a single live one is returned as it is
DEV double wp_lse4(double c0, double c1, double c2, double c3) {
  const double a0 = c0 > -INFINITY ? c0 : -INFINITY, a1 = c1 > -INFINITY ? c1 : -INFINITY;
  const double a2 = c2 > -INFINITY ? c2 : -INFINITY, a3 = c3 > -INFINITY ? c3 : -INFINITY;
  const double m = fmax(fmax(a0, a1), fmax(a2, a3));
  if (!(m > -INFINITY)) return -INFINITY;
  double z = 0.0;
  if (a0 > -INFINITY) z += exp(a0 - m);
  if (a1 > -INFINITY) z += exp(a1 - m);
  if (a2 > -INFINITY) z += exp(a2 - m);
  if (a3 > -INFINITY) z += exp(a3 - m);
  return z == 1.0 ? m : m + log(z);
}

// every lane's pair joined across the wave (all lanes end with the same bits); -inf over none
DEV double wp_wave_lse(double m, double z) {
  for (int o = 32; o > 0; o >>= 1) {
    const double m2 = __shfl_xor(m, o, 64), z2 = __shfl_xor(z, o, 64);
    const double M = fmax(m, m2);
    if (M > -INFINITY) {
      const double a = z * exp(m - M), b = z2 * exp(m2 - M);
      z = (m >= m2) ? a + b : b + a;  // the same two operands in the same order on both lanes
    }
    m = M;
  }
  return m > -INFINITY ? m + log(z) : -INFINITY;
}

// The workspace, doubles in this order (cells = (N + 1) K, S = K T):
struct WpPlan {
  double *G, *bG;                   // N + 1 each
  double *aU, *aX, *aW, *bU, *bW;   // the lattice, cells each
  double *cont, *last;              // sp(v), sp(-v), S each (row s K + k), unscaled
  double* rows;                     // 2 S: aH[n] (forward) or bA[n] (backward) in row n mod 2
  double *tc, *ic, *mc;             // the count accumulators: K K, K, 3 K
  double* log_z;                    // then the three 64-bit integers below
  long *next_fwd, *next_bwd, *status;
};

static __host__ __device__ inline WpPlan wp_plan(void* ws, long N, int K, int T) {
  const long cells = (N + 1) * K, S = (long)K * T;
  WpPlan p;
  p.G = (double*)ws;
  p.bG = p.G + (N + 1);
  p.aU = p.bG + (N + 1);
  p.aX = p.aU + cells;
  p.aW = p.aX + cells;
  p.bU = p.aW + cells;
  p.bW = p.bU + cells;
  p.cont = p.bW + cells;
  p.last = p.cont + S;
  p.rows = p.last + S;
  p.tc = p.rows + 2 * S;
  p.ic = p.tc + (long)K * K;
  p.mc = p.ic + K;
  p.log_z = p.mc + 3 * K;
  p.next_fwd = (long*)(p.log_z + 1);
  p.next_bwd = p.next_fwd + 1;
  p.status = p.next_bwd + 1;
  return p;
}

struct WpLds {
  double *Wc, *Li, *Uc, *En, *Aw, *pm, *pz, *pc;
  float* lt;
};

DEV WpLds wp_lds(double* base, int K) {
  WpLds l;
  l.Wc = base;       // aW[n] (forward), bW[n + 1] (backward)
  l.Li = l.Wc + K;   // scale * log_init
  l.Uc = l.Li + K;   // aU[n] (forward), bU[n] (backward)
  l.En = l.Uc + K;   // scale * log_enter
  l.Aw = l.En + K;   // aW[n], for the bigram counts
  l.pm = l.Aw + K;   // the threads' pairs
  l.pz = l.pm + WP_THREADS;
  l.pc = l.pz + WP_THREADS;  // the threads' parts of the three move counts
  l.lt = (float*)(l.pc + 3 * WP_THREADS);  // RES: K rows of K + 1
  return l;
}

// Thread tid < R K is (r, k) = (tid / K, tid % K) and owns the states s = r, r +
// R, ... of category k and the k' = r, r + R, ... of column k.  Per frame n:
//   1  the pairs of LSE_k' (aW[n][k'] + lt[k'][k])
//   2  thread (0, k) joins them in r order, then the initial term: aU[n][k]
//   3  the owned cells: aA from aH[n-1] (the other row), aH[n], the thread's
//      pair over its endings
//   4  thread (0, k) joins the endings in r order: aX[n+1], aW[n+1]
// with a barrier after each.
template <bool RES>
__global__ __launch_bounds__(WP_THREADS) void warp_post_fwd(
    const float* __restrict__ C, long ldc, long n0, long n1, long N, int K, int T, const float* __restrict__ V,
    double lm0, double lm1, double lm2, const float* __restrict__ LE, const float* __restrict__ gap, double bonus,
    double scale, const float* __restrict__ LT, long ldt, const float* __restrict__ LI, int smin,
    double* __restrict__ alpha_out, long lda, double* __restrict__ log_z, void* ws) {
  extern __shared__ __attribute__((aligned(16))) double wp_sh[];
  const WpLds L = wp_lds(wp_sh, K);
  const WpPlan P = wp_plan(ws, N, K, T);
  const int tid = threadIdx.x;
  const int R = WP_THREADS / K, r = tid / K, k = tid - r * K;
  const bool active = r < R, head = tid < K;
  const int Ru = min(R, K), Rx = min(R, T);  // rows r >= K hold no k', rows r >= T no state
  const int ldl = K + 1;
  const long S = (long)K * T;
  const bool fresh = n0 == 0;
  if (!fresh && *P.next_fwd != n0) {  // uniform: every thread reads the same word, nobody has written it yet
    if (tid == 0) *log_z = __builtin_nan("");
    return;
  }
  if (head) {
    L.Li[k] = scale * (double)LI[k];
    L.En[k] = LE ? scale * (double)LE[k] : 0.0;
    if (fresh) {
      L.Wc[k] = -INFINITY;
      P.aW[k] = -INFINITY;
      P.aX[k] = -INFINITY;
    } else {
      L.Wc[k] = P.aW[n0 * K + k];
    }
  }
  if (fresh)
    for (long j = tid; j < S; j += WP_THREADS) {
      const double v = (double)V[j];
      P.cont[j] = wp_softplus(v);
      P.last[j] = wp_softplus(-v);
      P.rows[S + j] = -INFINITY;  // aH[-1] lives in row 1
    }
  if (RES)
    for (int i = tid; i < K * K; i += WP_THREADS) L.lt[(i / K) * ldl + i % K] = LT[(long)(i / K) * ldt + i % K];
  double G = fresh ? 0.0 : P.G[n0];
  if (fresh && tid == 0) {
    P.G[0] = 0.0;
    *P.next_bwd = -1;  // no backward call before the forward sweep is through
  }
  __syncthreads();
  for (long n = n0; n < n1; ++n) {
    // ---- 1
    if (active) {
      double m = -INFINITY, z = 0.0;
#pragma unroll 4
      for (int kp = r; kp < K; kp += R)
        wp_fold(m, z, L.Wc[kp] + scale * (double)(RES ? L.lt[kp * ldl + k] : LT[(long)kp * ldt + k]));
      L.pm[tid] = m;
      L.pz[tid] = z;
    }
    __syncthreads();
    // ---- 2
    if (head) {
      const double u = wp_lae(G + L.Li[k], wp_join(L.pm, L.pz, Ru, K, k));
      L.Uc[k] = u;
      P.aU[n * K + k] = u;
    }
    __syncthreads();
    // ---- 3
    const double* const Hp = P.rows + ((n + 1) & 1) * S;  // aH[n-1]
    double* const Hn = P.rows + (n & 1) * S;
    if (active) {
      const float* const Crow = C + (n - n0) * ldc;
      double* const Arow = alpha_out ? alpha_out + (n - n0) * lda : nullptr;
      double m = -INFINITY, z = 0.0;
      for (int s = r; s < T; s += R) {
        const long j = (long)s * K + k;
        const double A = wp_lse4(s == 0 ? L.Uc[k] + L.En[k] : -INFINITY, Hp[j] + lm0,
                                 s >= 1 ? Hp[j - K] + lm1 : -INFINITY, s >= 2 ? Hp[j - 2 * K] + lm2 : -INFINITY);
        const double e = (double)Crow[j];
        double base = e < INFINITY ? A - scale * e : -INFINITY;  // a NaN or +inf e: the cell does not exist
        if (!(base > -INFINITY)) base = -INFINITY;
        const double h = base - scale * P.cont[j];
        Hn[j] = h;
        if (Arow) Arow[j] = h;
        if (s >= smin) wp_fold(m, z, base - scale * P.last[j]);
      }
      L.pm[tid] = m;
      L.pz[tid] = z;
    }
    __syncthreads();
    // ---- 4
    const double gv = gap ? scale * (double)gap[n] : -INFINITY;
    G = G + gv;
    if (head) {
      const double seg = wp_join(L.pm, L.pz, Rx, K, k);
      const double ax = seg > -INFINITY ? seg + bonus : -INFINITY;
      const double aw = wp_lae(L.Wc[k] + gv, ax);
      L.Wc[k] = aw;
      P.aX[(n + 1) * K + k] = ax;
      P.aW[(n + 1) * K + k] = aw;
      if (n + 1 == N) P.aU[N * K + k] = -INFINITY;  // no segment starts at N
    }
    if (tid == 0) P.G[n + 1] = G;
    __syncthreads();
  }
  if (tid != 0) return;
  *P.next_fwd = n1;
  if (n1 != N) return;
  double m = -INFINITY, z = 0.0;
  for (int q = 0; q < K; ++q) wp_fold(m, z, L.Wc[q]);
  const double lz = wp_lae(G, m > -INFINITY ? m + log(z) : -INFINITY);
  *P.log_z = lz;
  *log_z = lz;
  *P.next_bwd = N;
}

// The same grid.  Per frame n (descending):
//   1  the owned cells: bA[n] from bA[n+1] (the other row) and bW[n+1]; the
//      thread's parts of the move counts against alpha[n]; thread (0, k): bU[n][k]
//   2  the pairs of LSE_k'' (lt[k][k''] + bU[n][k'']); the bigram entries (k', k)
//      of the thread; thread (0, k): the initial count and the move parts in r order
//   3  thread (0, k) joins the pairs in r order: bW[n][k]
// with a barrier after each.  The call with n0 = 0 then forms bG (the LSE over
// k by one wave per frame, the recursion over n by wave 0), the posteriors
// elementwise and copies the counts out.
template <bool RES>
__global__ __launch_bounds__(WP_THREADS) void warp_post_bwd(
    const float* __restrict__ C, long ldc, long n0, long n1, long N, int K, int T, double lm0, double lm1, double lm2,
    const float* __restrict__ LE, const float* __restrict__ gap, double bonus, double scale,
    const float* __restrict__ LT, long ldt, const float* __restrict__ LI, int smin, const double* __restrict__ alpha,
    long lda, double* __restrict__ post_k, double* __restrict__ gap_post, double* __restrict__ tc_out,
    double* __restrict__ ic_out, double* __restrict__ mc_out, void* ws) {
  extern __shared__ __attribute__((aligned(16))) double wp_sh[];
  const WpLds L = wp_lds(wp_sh, K);
  const WpPlan P = wp_plan(ws, N, K, T);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int R = WP_THREADS / K, r = tid / K, k = tid - r * K;
  const bool active = r < R, head = tid < K;
  const int Ru = min(R, K), Rx = min(R, T);
  const int ldl = K + 1;
  const long S = (long)K * T;
  const bool first = n1 == N;
  // uniform: the three words are read by every thread before anybody writes them
  if (*P.next_fwd != N || (first ? *P.next_bwd < 0 : *P.next_bwd != n1)) {
    __syncthreads();
    if (tid == 0) *P.status = 1;
    return;
  }
  const double lz = *P.log_z;
  const bool reach = lz > -INFINITY;
  const bool want_tc = tc_out != nullptr && reach, want_mc = mc_out != nullptr && reach;
  auto trans = [&](int kp, int kq) {  // scale * log_trans[kp][kq]
    return scale * (double)(RES ? L.lt[kp * ldl + kq] : LT[(long)kp * ldt + kq]);
  };
  double icr = 0.0, mcr[3] = {0.0, 0.0, 0.0};
  if (head) {
    L.Li[k] = scale * (double)LI[k];
    L.En[k] = LE ? scale * (double)LE[k] : 0.0;
    if (first) {
      L.Wc[k] = 0.0;
      P.bW[N * K + k] = 0.0;
      P.bU[N * K + k] = -INFINITY;
    } else {
      L.Wc[k] = P.bW[n1 * K + k];
      icr = P.ic[k];
      for (int m = 0; m < 3; ++m) mcr[m] = P.mc[3 * k + m];
    }
  }
  if (first && active)  // each bigram entry by the thread that adds to it below
    for (int kp = r; kp < K; kp += R) P.tc[(long)kp * K + k] = 0.0;
  if (RES)
    for (int i = tid; i < K * K; i += WP_THREADS) L.lt[(i / K) * ldl + i % K] = LT[(long)(i / K) * ldt + i % K];
  __syncthreads();
  for (long n = n1 - 1; n >= n0; --n) {
    const double gv = gap ? scale * (double)gap[n] : -INFINITY;
    // ---- 1
    const double* const Bp = P.rows + ((n + 1) & 1) * S;  // bA[n+1]
    double* const Bn = P.rows + (n & 1) * S;
    const bool inner = n < N - 1;
    if (active) {
      const float* const Crow = C + (n - n0) * ldc;
      const double* const Arow = (want_mc && inner) ? alpha + (n - n0) * lda : nullptr;
      const double bw = L.Wc[k];
      double part[3] = {0.0, 0.0, 0.0};
      for (int s = r; s < T; s += R) {
        const long j = (long)s * K + k;
        const double b0 = inner ? Bp[j] : -INFINITY;
        const double b1 = (inner && s + 1 < T) ? Bp[j + K] : -INFINITY;
        const double b2 = (inner && s + 2 < T) ? Bp[j + 2 * K] : -INFINITY;
        const double go = wp_lse4(lm0 + b0, lm1 + b1, lm2 + b2, -INFINITY);
        const double endc = s >= smin ? (bonus - scale * P.last[j]) + bw : -INFINITY;
        const double contc = go > -INFINITY ? go - scale * P.cont[j] : -INFINITY;
        const double e = (double)Crow[j];
        double b = e < INFINITY ? wp_lae(endc, contc) - scale * e : -INFINITY;
        if (!(b > -INFINITY)) b = -INFINITY;
        Bn[j] = b;
        if (Arow) {
          const double a = Arow[j] - lz;
          if (a > -INFINITY) {
            const double c0 = (a + lm0) + b0, c1 = (a + lm1) + b1, c2 = (a + lm2) + b2;
            if (c0 > -INFINITY) part[0] += exp(c0);
            if (c1 > -INFINITY) part[1] += exp(c1);
            if (c2 > -INFINITY) part[2] += exp(c2);
          }
        }
        if (s == 0) {  // r = 0: thread (0, k)
          const double bu = L.En[k] + b;
          L.Uc[k] = bu > -INFINITY ? bu : -INFINITY;
        }
      }
      if (want_mc)
        for (int m = 0; m < 3; ++m) L.pc[m * WP_THREADS + tid] = part[m];
    }
    if (head) {
      P.bU[n * K + k] = L.Uc[k];
      if (want_tc) L.Aw[k] = P.aW[n * K + k];
    }
    __syncthreads();
    // ---- 2
    if (active) {
      double m = -INFINITY, z = 0.0;
#pragma unroll 4
      for (int kq = r; kq < K; kq += R) wp_fold(m, z, trans(k, kq) + L.Uc[kq]);
      L.pm[tid] = m;
      L.pz[tid] = z;
      if (want_tc) {
        const double bu = L.Uc[k] - lz;
        if (bu > -INFINITY)
          for (int kp = r; kp < K; kp += R) {
            const double c = (L.Aw[kp] + trans(kp, k)) + bu;
            if (c > -INFINITY) P.tc[(long)kp * K + k] += exp(c);
          }
      }
    }
    if (head) {
      if (want_tc) {
        const double c = (P.G[n] + L.Li[k]) + L.Uc[k] - lz;
        if (c > -INFINITY) icr += exp(c);
      }
      if (want_mc && inner)
        for (int m = 0; m < 3; ++m) {
          double t = 0.0;
          for (int i = 0; i < Rx; ++i) t += L.pc[m * WP_THREADS + i * K + k];
          mcr[m] += t;
        }
    }
    __syncthreads();
    // ---- 3
    if (head) {
      const double bw = wp_lae(gv + L.Wc[k], wp_join(L.pm, L.pz, Ru, K, k));
      L.Wc[k] = bw;
      P.bW[n * K + k] = bw;
    }
    __syncthreads();
  }
  if (head) {
    P.ic[k] = icr;
    for (int m = 0; m < 3; ++m) P.mc[3 * k + m] = mcr[m];
  }
  if (tid == 0) {
    *P.next_bwd = n0;
    *P.status = 0;
  }
  if (n0 != 0) return;
  __syncthreads();
  // ---- bG: LSE_k (li[k] + bU[n][k]) per frame, then the recursion over n
  const int nw = WP_THREADS / 64;
  if (tid == 0) P.bG[N] = 0.0;
  for (long n = w; n < N; n += nw) {
    double m = -INFINITY, z = 0.0;
    for (int q = lane; q < K; q += 64) wp_fold(m, z, L.Li[q] + P.bU[n * K + q]);
    const double v = wp_wave_lse(m, z);
    if (lane == 0) P.bG[n] = v;
  }
  __syncthreads();
  if (w == 0) {
    double b = 0.0;
    for (long base = N - 1; base >= 0; base -= 64) {
      const long at = base - lane;
      const double q = at >= 0 ? P.bG[at] : -INFINITY;
      const double g = (at >= 0 && gap) ? scale * (double)gap[at] : -INFINITY;
      double mine = -INFINITY;
      for (int j = 0; j < 64; ++j) {
        b = wp_lae(__shfl(g, j, 64) + b, __shfl(q, j, 64));
        if (lane == j) mine = b;
      }
      if (at >= 0) P.bG[at] = mine;
    }
  }
  __syncthreads();
  // ---- the posteriors
  for (long n = w; n <= N; n += nw) {
    double gp = 0.0;
    if (n < N && gap && reach) {
      double m = -INFINITY, z = 0.0;
      for (int q = lane; q < K; q += 64) wp_fold(m, z, P.aW[n * K + q] + P.bW[(n + 1) * K + q]);
      const double in = wp_lae(P.G[n] + P.bG[n + 1], wp_wave_lse(m, z));
      const double c = in + scale * (double)gap[n] - lz;
      if (c > -INFINITY) gp = exp(c);
    }
    if (lane == 0) gap_post[n] = gp > 0.0 ? gp : 0.0;
  }
  const long cells = (N + 1) * K;
  for (long i = tid; i < cells; i += WP_THREADS) {
    double on = 0.0, en = 0.0;
    if (reach) {
      on = exp(P.aU[i] + P.bU[i] - lz);
      en = exp(P.aX[i] + P.bW[i] - lz);
    }
    post_k[i] = on > 0.0 ? on : 0.0;  // a NaN (inf - inf, outside the contract) reads as 0
    post_k[cells + i] = en > 0.0 ? en : 0.0;
  }
  if (tc_out) {
    for (long i = tid; i < (long)K * K; i += WP_THREADS) tc_out[i] = reach ? P.tc[i] : 0.0;
    if (head) ic_out[k] = icr;
  }
  if (mc_out && head)
    for (int m = 0; m < 3; ++m) mc_out[3 * k + m] = mcr[m];
}

static bool warp_post_shape_ok(long N, int K, int T) {
  return K >= 1 && K <= WP_MAX_K && T >= 1 && T <= WP_MAX_T && (long)K * T < (1L << 24) && N >= 0 &&
         N < (1L << 31) && (N + 1) * K < (1L << 31);
}

template <auto KERNEL>
static hipError_t warp_post_raise_lds(size_t bytes) {
  static bool done = false;
  if (done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  done = e == hipSuccess;
  return e;
}

// the model arguments both entry points share, decided on the host
static bool warp_post_model_ok(long N, int K, int T, const double* log_move, double scale, long ld_trans, int s_min,
                               const void* ws, size_t ws_bytes, size_t need) {
  if (!(warp_post_shape_ok(N, K, T) && s_min >= 0 && s_min < T && ld_trans >= K)) return false;
  if (!log_move || !(scale > 0.0) || !(scale < INFINITY)) return false;
  bool any = false;
  for (int m = 0; m < 3; ++m) {
    if (!(log_move[m] < INFINITY)) return false;  // NaN fails too
    any = any || log_move[m] > -INFINITY;
  }
  return any && need && ws && ws_bytes >= need;
}

}  // namespace abcd

using namespace abcd;

extern "C" int abcd_warp_posterior_plan(int K, int T_proto, int* resident, int* threads, size_t* lds_bytes) {
  ABCD_REQUIRE(warp_post_shape_ok(0, K, T_proto));
  if (resident) *resident = K <= WP_RES_K;
  if (threads) *threads = WP_THREADS;
  if (lds_bytes) *lds_bytes = warp_post_lds(K);
  return 0;
}

extern "C" size_t abcd_warp_posterior_workspace_bytes(long N, int K, int T_proto) {
  if (!warp_post_shape_ok(N, K, T_proto)) return 0;
  const size_t cells = ((size_t)N + 1) * (size_t)K, S = (size_t)K * (size_t)T_proto;
  return sizeof(double) * (2 * ((size_t)N + 1) + 5 * cells + 4 * S + (size_t)K * K + 4 * (size_t)K + 4) + 256;
}

extern "C" int abcd_warp_posterior_forward(const float* cost, long ld_cost, long n0, long n1, long N, int K,
                                           int T_proto, const float* proto_offset_logits, const double* log_move,
                                           const float* log_enter, const float* gap, double seg_bonus, double scale,
                                           const float* log_trans, long ld_trans, const float* log_init, int s_min,
                                           double* alpha_out, long ld_alpha, double* log_z, void* ws, size_t ws_bytes,
                                           void* stream) {
  ABCD_REQUIRE(warp_post_model_ok(N, K, T_proto, log_move, scale, ld_trans, s_min, ws, ws_bytes,
                                  abcd_warp_posterior_workspace_bytes(N, K, T_proto)));
  ABCD_REQUIRE(!alpha_out || ld_alpha >= (long)K * T_proto);
  ABCD_REQUIRE(log_z != nullptr);
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {  // the empty cover alone: log_z = 0, nothing is read
    ABCD_REQUIRE(n0 == 0 && n1 == 0);
    ABCD_TRY(hipMemsetAsync(log_z, 0, sizeof(double), s));
    return 0;
  }
  ABCD_REQUIRE(0 <= n0 && n0 < n1 && n1 <= N);
  ABCD_REQUIRE(ld_cost >= (long)K * T_proto && ld_cost < (1L << 31) && (n1 - n0) * ld_cost < (1L << 31));
  ABCD_REQUIRE(cost && proto_offset_logits && log_trans && log_init);
  ABCD_TRY(warp_post_raise_lds<warp_post_fwd<true>>(warp_post_lds(WP_RES_K)));
  ABCD_TRY(warp_post_raise_lds<warp_post_fwd<false>>(warp_post_lds(WP_MAX_K)));
  (K <= WP_RES_K ? warp_post_fwd<true> : warp_post_fwd<false>)<<<1, WP_THREADS, warp_post_lds(K), s>>>(
      cost, ld_cost, n0, n1, N, K, T_proto, proto_offset_logits, scale * log_move[0], scale * log_move[1],
      scale * log_move[2], log_enter, gap, scale * seg_bonus, scale, log_trans, ld_trans, log_init, s_min, alpha_out,
      ld_alpha, log_z, ws);
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" int abcd_warp_posterior_backward(const float* cost, long ld_cost, long n0, long n1, long N, int K,
                                            int T_proto, const float* proto_offset_logits, const double* log_move,
                                            const float* log_enter, const float* gap, double seg_bonus, double scale,
                                            const float* log_trans, long ld_trans, const float* log_init, int s_min,
                                            const double* alpha, long ld_alpha, double* post_k, double* gap_post,
                                            double* trans_counts, double* init_counts, double* move_counts, void* ws,
                                            size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(warp_post_model_ok(N, K, T_proto, log_move, scale, ld_trans, s_min, ws, ws_bytes,
                                  abcd_warp_posterior_workspace_bytes(N, K, T_proto)));
  ABCD_REQUIRE(!alpha || ld_alpha >= (long)K * T_proto);
  ABCD_REQUIRE(!move_counts || alpha);
  ABCD_REQUIRE((trans_counts == nullptr) == (init_counts == nullptr));
  ABCD_REQUIRE(post_k && gap_post);
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {  // zero posteriors and counts, nothing is read
    ABCD_REQUIRE(n0 == 0 && n1 == 0);
    ABCD_TRY(hipMemsetAsync(post_k, 0, 2 * (size_t)K * sizeof(double), s));
    ABCD_TRY(hipMemsetAsync(gap_post, 0, sizeof(double), s));
    if (trans_counts) {
      ABCD_TRY(hipMemsetAsync(trans_counts, 0, (size_t)K * K * sizeof(double), s));
      ABCD_TRY(hipMemsetAsync(init_counts, 0, (size_t)K * sizeof(double), s));
    }
    if (move_counts) ABCD_TRY(hipMemsetAsync(move_counts, 0, 3 * (size_t)K * sizeof(double), s));
    return 0;
  }
  ABCD_REQUIRE(0 <= n0 && n0 < n1 && n1 <= N);
  ABCD_REQUIRE(ld_cost >= (long)K * T_proto && ld_cost < (1L << 31) && (n1 - n0) * ld_cost < (1L << 31));
  ABCD_REQUIRE(cost && proto_offset_logits && log_trans && log_init);
  ABCD_TRY(warp_post_raise_lds<warp_post_bwd<true>>(warp_post_lds(WP_RES_K)));
  ABCD_TRY(warp_post_raise_lds<warp_post_bwd<false>>(warp_post_lds(WP_MAX_K)));
  (K <= WP_RES_K ? warp_post_bwd<true> : warp_post_bwd<false>)<<<1, WP_THREADS, warp_post_lds(K), s>>>(
      cost, ld_cost, n0, n1, N, K, T_proto, scale * log_move[0], scale * log_move[1], scale * log_move[2], log_enter,
      gap, scale * seg_bonus, scale, log_trans, ld_trans, log_init, s_min, alpha, ld_alpha, post_k, gap_post,
      trans_counts, init_counts, move_counts, ws);
  ABCD_CHECK_LAUNCH();
  return 0;
}
