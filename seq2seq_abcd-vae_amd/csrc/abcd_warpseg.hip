// abcd_warpseg.hip -- time-warped segmentation: the span
// programme of abcd_span.hip with the prototypes warped inside it.  The state is
// (category k, prototype step s); inside a category the moves are stay, step
// and skip (abcd_warp.hip's), leaving a category ends a segment, entering the
// next one pays the chain's transition.  The programme is frame-synchronous:
// O(N K T_proto) cell updates, no D factor, and nothing of size N D K.
//
//   frame_costs   the emission plane e(n, r) of frames n0 .. n1 - 1 against every
//                 rectangle row r = s K + k: the tile of abcd_emtile.h with the
//                 rectangle's rows as the "prototypes" of one step, one
//                 32 x 32 tile per workgroup
//   warp_seg      one workgroup: frames n0 .. n1 - 1 of the recurrence on such a
//                 plane, the carry in the workspace, the backtrack at n1 = N
//
// The recurrence is written out in include/abcd_hip.h.  No atomics, no
// device-global word, no workgroup waits for another.
//
// Measured on one MI355X at N = 15 000, K = 128, T_proto = 200, F = 129
// (profiles/warpseg_bench.json): frame_costs 0.39 us per frame, warp_seg 52.5
// us per frame on a plane in HBM, 46.0 end to end on chunks just written,
// against 13.96 us per step of span_chain at D = 200.  The step is latency: 25 cells per thread
// and frame, each behind its own loads.  Next: a thread owning consecutive s
// keeps H in registers, and the plane's next row is fetched during this one.
#include <algorithm>
#include <climits>
#include <cmath>

#include "abcd_common.h"
#include "abcd_emtile.h"
#include "abcd_internal.h"
#include "abcd_special.h"

namespace abcd {

// One workgroup of 256 threads per tile, the tiles of a frame block side by side
// on a one-dimensional grid (tile = frame block * row tiles + row tile: up to
// 2^26 of them at K T = 1, which neither grid.y nor grid.z holds).  A pair's sum runs over
// the F columns in column order whatever the tile, so its bits depend on its
// frame and its row alone.
__global__ __launch_bounds__(256) void frame_costs(const float* __restrict__ X, long ldx, long n0, long n1, int F,
                                                   int R, const float* __restrict__ MU, long ldm,
                                                   const float* __restrict__ LV, long ldl, float* __restrict__ cost,
                                                   long ldc) {
  __shared__ EmTile tile;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, ti = tid >> 4, tj = tid & 15;
  const int rtiles = (R + EM_TP - 1) / EM_TP;
  const int r0 = (int)(blockIdx.x % rtiles) * EM_TP;
  const long f0n = n0 + (long)(blockIdx.x / rtiles) * EM_TR;  // the tile's first frame
  const int nch = (F + EM_FC - 1) / EM_FC;
  EmRegs g;
  auto fetch = [&](int c) {
    const int f = c * EM_FC + lane;
#pragma unroll
    for (int i = 0; i < EM_TR / 4; ++i) {
      const long n = f0n + w + 4 * i;
      g.x[i] = (f < F && n < n1) ? X[n * ldx + f] : 0.f;
    }
    em_fetch_proto(g, MU, ldm, LV, ldl, w, 0, r0, R, f, F);
  };
  float q[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  float csum[EM_TP / 4] = {};
  fetch(0);
  for (int c = 0; c < nch; ++c) {
    const int k = c & 1;
    tile.stage(k, g, csum, w, lane, r0, R, c * EM_FC, F, c == 0, c == nch - 1);
    __syncthreads();
    if (c + 1 < nch) fetch(c + 1);
    tile.accumulate(k, q, ti, tj, c * EM_FC, F, c == 0);
  }
  const int k = (nch - 1) & 1;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long n = f0n + 2 * ti + i;
    if (n >= n1) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = r0 + tj + 16 * j;
      if (r < R) cost[(n - n0) * ldc + r] = tile.cs[k][tj + 16 * j] + 0.5f * q[i][j];
    }
  }
}

constexpr int WS_THREADS = 1024;
constexpr int WS_RES_K = 128;  // log_trans resident in LDS (64 KB) up to here
constexpr int WS_MAX_K = 1024;
constexpr int WS_MAX_T = 16383;

static size_t warp_seg_lds(int K) {
  return (size_t)K * 4 * sizeof(double) + (size_t)WS_THREADS * (sizeof(double) + 2 * sizeof(int)) +
         (K <= WS_RES_K ? (size_t)K * K * sizeof(float) : 0);
}

DEV double ws_softplus(double v) { return fmax(v, 0.0) + log1p(exp(-fabs(v))); }

// The workspace, in this order (cells = (N + 1) K, S = K T):
struct WsPlan {
  double *U, *xsel;                     // U[n][k]; X[n][k] where W chose the segment
  int32_t *wsel, *on, *st, *back_k;     // W's choice (0 gap, 1 segment), the segment's onset and last state, U's k'
  double *cont, *last, *H;              // sp(v), sp(-v); the two H rows
  int32_t* Hon;                         // and their onsets
  double* carry;                        // W[n1] (K), G[n1], next frame (one 64-bit integer)
};

static __host__ __device__ inline WsPlan ws_plan(void* ws, long N, int K, int T) {
  const long cells = (N + 1) * K, S = (long)K * T;
  WsPlan p;
  p.U = (double*)ws;
  p.xsel = p.U + cells;
  p.wsel = (int32_t*)(p.xsel + cells);
  p.on = p.wsel + cells;
  p.st = p.on + cells;
  p.back_k = p.st + cells;
  p.cont = (double*)(p.back_k + cells);  // 16 cells bytes of int32 in: 8-byte aligned
  p.last = p.cont + S;
  p.H = p.last + S;
  p.Hon = (int32_t*)(p.H + 2 * S);
  p.carry = (double*)(p.Hon + 2 * S);
  return p;
}

// One workgroup of 1024 threads.  With R = 1024 / K, thread tid < R K is (r, k)
// = (tid / K, tid % K): it owns the states s = r, r + R, ... of category k, so
// consecutive threads touch consecutive j = s K + k of H, the plane and the
// logits.  The same (r, k) grid splits k' in U.  Per frame n:
//   1  U's partial maxima over k' = r, r + R, ... (ascending, strict: the lowest)
//   2  thread (0, k) joins them in r order (a tie: the lower k'), then the
//      initial term; U[n][k] and its k' go to the planes
//   3  the owned cells: A from H[n-1] (the other H row), H[n], the thread's
//      best ending over its s (ascending, strict: the lowest)
//   4  thread (0, k) joins the endings in r order (a tie: the lower s), W[n+1]
// with a barrier after each; the H rows alternate in the workspace, and the
// workgroup reads its own global stores a barrier later.
template <bool RES>
__global__ __launch_bounds__(WS_THREADS) void warp_seg(
    const float* __restrict__ C, long ldc, long n0, long n1, long N, int K, int T, const float* __restrict__ V,
    double lm0, double lm1, double lm2, const float* __restrict__ LE, const float* __restrict__ gap, double bonus,
    const float* __restrict__ LT, long ldt, const float* __restrict__ LI, int smin, double* __restrict__ path_score,
    int32_t* __restrict__ n_segments, int32_t* __restrict__ seg_onset, int32_t* __restrict__ seg_length,
    int32_t* __restrict__ seg_cat, int32_t* __restrict__ seg_state, double* __restrict__ seg_enter,
    double* __restrict__ seg_exit, double* __restrict__ seg_link, double* __restrict__ W_out, void* ws) {
  extern __shared__ __attribute__((aligned(16))) double ws_lds[];
  double* const Wc = ws_lds;   // W[n][k]
  double* const Li = Wc + K;   // log_init, widened
  double* const Uc = Li + K;   // U[n][k]
  double* const En = Uc + K;   // log_enter, widened
  double* const pv = En + K;   // the partial maxima, R x K
  int* const pa = (int*)(pv + WS_THREADS);   // their arguments (k' or s)
  int* const po = pa + WS_THREADS;           // the endings' onsets
  const float* const lt = (const float*)(po + WS_THREADS);  // RES: K x K
  const WsPlan P = ws_plan(ws, N, K, T);
  const int tid = threadIdx.x;
  const int R = WS_THREADS / K, r = tid / K, k = tid - r * K;
  const bool active = r < R, head = tid < K;
  const int Ru = min(R, K), Rx = min(R, T);  // rows r >= K hold no k', rows r >= T no state: the joins skip them
  const long S = (long)K * T;
  long* const next_n = (long*)(P.carry + K + 1);
  const bool fresh = n0 == 0;
  if (!fresh && *next_n != n0) {  // uniform: every thread reads the same word, nobody has written it yet
    if (tid == 0) {
      *path_score = __builtin_nan("");
      *n_segments = -1;
    }
    return;
  }
  if (head) {
    Li[k] = (double)LI[k];
    En[k] = LE ? (double)LE[k] : 0.0;
    if (fresh) {
      Wc[k] = -INFINITY;
      P.wsel[k] = 0;
      if (W_out) W_out[k] = -INFINITY;
    } else {
      Wc[k] = P.carry[k];
    }
  }
  if (fresh)
    for (long j = tid; j < S; j += WS_THREADS) {
      const double v = (double)V[j];
      P.cont[j] = ws_softplus(v);
      P.last[j] = ws_softplus(-v);
      P.H[S + j] = -INFINITY;  // H[-1] lives in row 1
      P.Hon[S + j] = 0;
    }
  if (RES) {
    float* const dst = (float*)(po + WS_THREADS);
    for (int i = tid; i < K * K; i += WS_THREADS) dst[i] = LT[(long)(i / K) * ldt + i % K];
  }
  double G = fresh ? 0.0 : P.carry[K];
  __syncthreads();
  for (long n = n0; n < n1; ++n) {
    // ---- 1: the best way into a segment of k that starts at n
    if (active) {
      double best = -INFINITY;
      int bk = INT_MAX;
#pragma unroll 4
      for (int kp = r; kp < K; kp += R) {
        const double c = Wc[kp] + (double)(RES ? lt[kp * K + k] : LT[(long)kp * ldt + k]);
        if (c > best) { best = c; bk = kp; }
      }
      pv[tid] = best;
      pa[tid] = bk;
    }
    __syncthreads();
    // ---- 2: U[n]
    if (head) {
      double best = pv[k];
      int bk = pa[k];
      for (int i = 1; i < Ru; ++i) {
        const double b2 = pv[i * K + k];
        const int k2 = pa[i * K + k];
        if (b2 > best || (b2 == best && k2 < bk)) { best = b2; bk = k2; }
      }
      const double init = G + Li[k];
      const bool vi = init > -INFINITY, vp = best > -INFINITY && bk != INT_MAX;
      double Un = -INFINITY;
      int from = -1;  // -1: the initial term (or nothing)
      if (vi && (!vp || init >= best)) Un = init;
      else if (vp) { Un = best; from = bk; }
      Uc[k] = Un;
      P.U[n * K + k] = Un;
      P.back_k[n * K + k] = from;
    }
    __syncthreads();
    // ---- 3: the cells of frame n
    const double* const Hp = P.H + ((n + 1) & 1) * S;  // H[n-1]
    const int32_t* const Op = P.Hon + ((n + 1) & 1) * S;
    double* const Hn = P.H + (n & 1) * S;
    int32_t* const On = P.Hon + (n & 1) * S;
    if (active) {
      const float* const Crow = C + (n - n0) * ldc;
      double xb = -INFINITY;
      int xs = INT_MAX, xo = 0;
      for (int s = r; s < T; s += R) {
        const long j = (long)s * K + k;
        double A = -INFINITY;
        int o = 0;
        if (s == 0) {  // enter, then stay
          const double c = Uc[k] + En[k];
          if (c > A) { A = c; o = (int)n; }
        }
        {
          const double c = Hp[j] + lm0;
          if (c > A) { A = c; o = Op[j]; }
        }
        if (s >= 1) {
          const double c = Hp[j - K] + lm1;
          if (c > A) { A = c; o = Op[j - K]; }
        }
        if (s >= 2) {
          const double c = Hp[j - 2 * K] + lm2;
          if (c > A) { A = c; o = Op[j - 2 * K]; }
        }
        const double e = (double)Crow[j];
        const double base = e < INFINITY ? A - e : -INFINITY;  // a NaN or +inf e: the cell does not exist
        Hn[j] = base - P.cont[j];
        On[j] = o;
        if (s >= smin) {
          const double c = base - P.last[j];
          if (c > xb) { xb = c; xs = s; xo = o; }
        }
      }
      pv[tid] = xb;
      pa[tid] = xs;
      po[tid] = xo;
    }
    __syncthreads();
    // ---- 4: X[n+1] and W[n+1]
    const double gv = gap ? (double)gap[n] : -INFINITY;
    G = G + gv;
    if (head) {
      double best = pv[k];
      int bs = pa[k], bo = po[k];
      for (int i = 1; i < Rx; ++i) {
        const double b2 = pv[i * K + k];
        const int s2 = pa[i * K + k];
        if (b2 > best || (b2 == best && s2 < bs)) { best = b2; bs = s2; bo = po[i * K + k]; }
      }
      const double seg = best + bonus, gapc = Wc[k] + gv;
      const bool vg = gapc > -INFINITY, vs = seg > -INFINITY && bs != INT_MAX;
      double Wn = -INFINITY;
      int choice = 0;  // 0: the gap (or nothing); 1: a segment of k ends with frame n
      if (vg && (!vs || gapc >= seg)) Wn = gapc;
      else if (vs) { Wn = seg; choice = 1; }
      Wc[k] = Wn;
      const long at = (n + 1) * K + k;
      P.wsel[at] = choice;
      P.on[at] = bo;
      P.st[at] = choice ? bs : -1;
      P.xsel[at] = choice ? seg : -INFINITY;
      if (W_out) W_out[at] = Wn;
    }
    __syncthreads();
  }
  if (head) P.carry[k] = Wc[k];
  if (tid != 0) return;
  P.carry[K] = G;
  *next_n = n1;
  if (n1 != N) return;
  // the backtrack of span_chain: "no segment" wins a tie, then the lowest k
  double best = G > -INFINITY ? G : -INFINITY;
  int kb = -1;
  for (int q = 0; q < K; ++q)
    if (Wc[q] > best) { best = Wc[q]; kb = q; }
  *path_score = best;
  int count = 0;
  {
    long n = N;
    int q = kb;
    while (q >= 0 && n > 0) {
      if (P.wsel[n * K + q] == 0) { --n; continue; }
      ++count;
      n = P.on[n * K + q];
      q = P.back_k[n * K + q];
    }
  }
  *n_segments = count;
  int i = count;
  long n = N;
  int q = kb;
  while (q >= 0 && n > 0) {
    if (P.wsel[n * K + q] == 0) { --n; continue; }
    --i;
    const long o = P.on[n * K + q];
    seg_onset[i] = (int32_t)o;
    seg_length[i] = (int32_t)(n - o);
    seg_cat[i] = q;
    seg_state[i] = P.st[n * K + q];
    seg_exit[i] = P.xsel[n * K + q];
    seg_enter[i] = P.U[o * K + q];
    const int from = P.back_k[o * K + q];
    seg_link[i] = from < 0 ? Li[q] : (double)LT[(long)from * ldt + q];
    n = o;
    q = from;
  }
}

__global__ __launch_bounds__(256) void warp_seg_fill(double* __restrict__ p, long n, double v) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

static bool warp_seg_shape_ok(long N, int K, int T) {
  return K >= 1 && K <= WS_MAX_K && T >= 1 && T <= WS_MAX_T && (long)K * T < (1L << 24) && N >= 0 &&
         N < (1L << 31) && (N + 1) * K < (1L << 31);
}

template <auto KERNEL>
static hipError_t warp_seg_raise_lds(size_t bytes) {
  static bool done = false;
  if (done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  done = e == hipSuccess;
  return e;
}

}  // namespace abcd

using namespace abcd;

extern "C" int abcd_frame_costs(const float* x, long ld_x, long N, long n0, long n1, int F, int K, int T_proto,
                                const float* proto_mu, long ld_mu, const float* proto_lv, long ld_lv, float* cost,
                                long ld_cost, void* stream) {
  ABCD_REQUIRE(warp_seg_shape_ok(N, K, T_proto) && F >= 1 && 0 <= n0 && n0 < n1 && n1 <= N);
  const long R = (long)K * T_proto;
  ABCD_REQUIRE(ld_x >= F && ld_mu >= F && ld_lv >= F && ld_cost >= R && ld_cost < (1L << 31) &&
               (n1 - n0) * ld_cost < (1L << 31));
  ABCD_REQUIRE(x && proto_mu && proto_lv && cost);
  // (n1 - n0) ld_cost < 2^31 and ld_cost >= R: 2^26 tiles at the most (R = 1)
  const unsigned grid = (unsigned)(cdiv(R, EM_TP) * (long)cdiv(n1 - n0, EM_TR));
  frame_costs<<<grid, 256, 0, (hipStream_t)stream>>>(x, ld_x, n0, n1, F, (int)R, proto_mu, ld_mu, proto_lv, ld_lv, cost,
                                                     ld_cost);
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" int abcd_warp_segment_plan(int K, int T_proto, int* resident, int* threads, size_t* lds_bytes) {
  ABCD_REQUIRE(warp_seg_shape_ok(0, K, T_proto));
  if (resident) *resident = K <= WS_RES_K;
  if (threads) *threads = WS_THREADS;
  if (lds_bytes) *lds_bytes = warp_seg_lds(K);
  return 0;
}

extern "C" size_t abcd_warp_segment_workspace_bytes(long N, int K, int T_proto) {
  if (!warp_seg_shape_ok(N, K, T_proto)) return 0;
  const size_t cells = ((size_t)N + 1) * (size_t)K, S = (size_t)K * (size_t)T_proto;
  return cells * (2 * sizeof(double) + 4 * sizeof(int32_t)) + S * (4 * sizeof(double) + 2 * sizeof(int32_t)) +
         ((size_t)K + 2) * sizeof(double) + 256;
}

extern "C" int abcd_warp_segment_window(const float* cost, long ld_cost, long n0, long n1, long N, int K, int T_proto,
                                        const float* proto_offset_logits, const double* log_move,
                                        const float* log_enter, const float* gap, double seg_bonus,
                                        const float* log_trans, long ld_trans, const float* log_init, int s_min,
                                        double* path_score, int32_t* n_segments, int32_t* seg_onset,
                                        int32_t* seg_length, int32_t* seg_cat, int32_t* seg_last_state,
                                        double* seg_enter, double* seg_exit, double* seg_link, double* W_out, void* ws,
                                        size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(warp_seg_shape_ok(N, K, T_proto) && s_min >= 0 && s_min < T_proto && ld_trans >= K);
  ABCD_REQUIRE(log_move != nullptr);
  bool any = false;
  for (int m = 0; m < 3; ++m) {
    ABCD_REQUIRE(log_move[m] < INFINITY);  // NaN fails too
    any = any || log_move[m] > -INFINITY;
  }
  ABCD_REQUIRE(any);
  const size_t need = abcd_warp_segment_workspace_bytes(N, K, T_proto);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {  // the empty path: score 0, no segments, W[0] = -inf, nothing is read
    ABCD_REQUIRE(n0 == 0 && n1 == 0);
    if (path_score) ABCD_TRY(hipMemsetAsync(path_score, 0, sizeof(double), s));
    if (n_segments) ABCD_TRY(hipMemsetAsync(n_segments, 0, sizeof(int32_t), s));
    if (W_out) {
      warp_seg_fill<<<cdiv(K, 256), 256, 0, s>>>(W_out, K, -INFINITY);
      ABCD_CHECK_LAUNCH();
    }
    return 0;
  }
  ABCD_REQUIRE(0 <= n0 && n0 < n1 && n1 <= N);
  ABCD_REQUIRE(ld_cost >= (long)K * T_proto && ld_cost < (1L << 31) && (n1 - n0) * ld_cost < (1L << 31));
  ABCD_REQUIRE(cost && proto_offset_logits && log_trans && log_init && path_score && n_segments && seg_onset &&
               seg_length && seg_cat && seg_last_state && seg_enter && seg_exit && seg_link);
  ABCD_TRY(warp_seg_raise_lds<warp_seg<true>>(warp_seg_lds(WS_RES_K)));
  ABCD_TRY(warp_seg_raise_lds<warp_seg<false>>(warp_seg_lds(WS_MAX_K)));
  (K <= WS_RES_K ? warp_seg<true> : warp_seg<false>)<<<1, WS_THREADS, warp_seg_lds(K), s>>>(
      cost, ld_cost, n0, n1, N, K, T_proto, proto_offset_logits, log_move[0], log_move[1], log_move[2], log_enter, gap,
      seg_bonus, log_trans, ld_trans, log_init, s_min, path_score, n_segments, seg_onset, seg_length, seg_cat,
      seg_last_state, seg_enter, seg_exit, seg_link, W_out, ws);
  ABCD_CHECK_LAUNCH();
  return 0;
}
