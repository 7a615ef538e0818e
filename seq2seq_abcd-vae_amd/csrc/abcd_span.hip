// abcd_span.hip -- cut a recording into segments by the decoder.
//
// The prototypes of abcd_pairwise.hip do not depend on the data, and the
// end-of-segment logits are a duration model, so the log-likelihood of "frames
// s .. s + d - 1 are one segment of category p that ends at d" is defined for
// every start s, length d and prototype p of an uncut recording (DESIGN.md
// s3.10):
//
//   span_prefix   one thread per prototype: O[p, d], the duration term, in fp64
//   span_fill     the entries with d > e (row 0 among them): -inf / -1
//   span_nll      one workgroup per 32 consecutive starts: the running emission
//                 sums E[s, p, d] of 32 starts x 32 prototypes in fp64, the best
//                 prototype per (s, d) folded into the end-major output
//   span_viterbi  one workgroup: the semi-Markov dynamic programme over the
//                 output of span_nll and the backtrack
//   span_nll<SPAN_LSE>  the same pass with the log-sum over the prototypes beside
//                 (or instead of) the maximum (abcd_span_evidence, s3.12)
//   span_fb       one workgroup: the sum form of span_viterbi, forward and
//                 backward over one recording, and the per-frame posteriors
//   span_post_table  the per-span posteriors from the lattice, many workgroups
//   span_nll<SPAN_TABLE>  the same pass keeping every prototype's score
//                 (abcd_span_table, s3.13)
//   span_chain    one workgroup: span_viterbi with a first-order chain over the
//                 categories of consecutive segments, state (frame, last category)
//
// span_nll runs on the emission tile pair_nll runs on (abcd_emtile.h: the
// staging, the per-term expressions and the order of a frame's sums, F columns
// in column order in fp32), with the frame of start s at step t being row s + t
// of the recording; frames join in step order in fp64.  No atomics, no
// device-global word, and no workgroup waits for another.
#include <climits>

#include "abcd_common.h"
#include "abcd_emtile.h"
#include "abcd_internal.h"
#include "abcd_special.h"

namespace abcd {

constexpr int SP_MAX_D = 16383;

DEV double softplus_d(double v) { return fmax(v, 0.0) + log1p(exp(-fabs(v))); }

// O[p, d] = sum_{t < d - 1} sp(o[t, p]) + sp(-o[d - 1, p]) at Otab[(d - 1) P + p]: the prefix in step order,
// then the last step's term
__global__ __launch_bounds__(256) void span_prefix(const float* __restrict__ OL, int P, int D,
                                                   double* __restrict__ Otab) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  double cum = 0.0;
  for (int t = 0; t < D; ++t) {
    const double o = (double)OL[(long)t * P + p];
    Otab[(long)t * P + p] = cum + softplus_d(-o);
    cum += softplus_d(o);
  }
}

// rows e <= min(N, D - 1): the entries with d > e
// (span_lse, and span_score with span_cat, each where not NULL)
__global__ __launch_bounds__(256) void span_fill(long rows, int D, double* __restrict__ span_score,
                                                 int32_t* __restrict__ span_cat, double* __restrict__ span_lse,
                                                 long lds) {
  const long at = (long)blockIdx.x * 256 + threadIdx.x;
  if (at >= rows * D) return;
  const long e = at / D;
  const int c = (int)(at - e * D);  // d - 1
  if (c < e) return;
  if (span_score) {
    span_score[e * lds + c] = -INFINITY;
    span_cat[e * lds + c] = -1;
  }
  if (span_lse) span_lse[e * lds + c] = -INFINITY;
}

// log(e^a + e^b) in fp64; -inf when neither is above -inf (NaN counts as -inf)
DEV double logaddexp_d(double a, double b) {
  const bool va = a > -INFINITY, vb = b > -INFINITY;
  if (!va) return vb ? b : -INFINITY;
  if (!vb) return a;
  const double hi = fmax(a, b), lo = fmin(a, b);
  return hi + log1p(exp(lo - hi));
}

// Workgroup blockIdx.x owns starts s0 = 32 blockIdx.x .. s0 + 31 and every
// output entry (e = s + d, d) of theirs, so it max-combines the prototype tiles
// itself, in tile order, each over the emission tile of abcd_emtile.h (staging,
// pipelining, the 2 x 2 accumulation and the order of sums are described
// there).  What this kernel adds: the tile's rows of x at step t are the frame
// rows s0 + t .. s0 + t + 31 of the recording, so thread (i, j) owns starts
// s0 + 2 i, + 1; the frames of a start join an fp64 sum in step order.  After
// a step's last column chunk the 16 lanes that hold one start's 32 prototypes
// reduce (score, index), the lowest index winning a tie, and lane j = 0 folds
// the result into the output entry: a plain store for the first prototype
// tile, a read and a strict comparison for the later ones (the same thread
// wrote what it reads).  Rows >= N and steps >= D are not read.
//
// LSE (abcd_span_evidence) adds the log-sum over the same admissible
// prototypes: the 16 lanes reduce the maximum m (the one the argmax tree just
// found) and then sum_p exp(S - m), the differences exponentiated in fp32 and
// summed in fp64 in a fixed shuffle order; lane j = i (i = 0, 1: the thread's
// two starts, so the two logarithms of a step run side by side) writes m + log
// sum for the first prototype tile and folds later tiles into what it wrote
// with a logaddexp.  The maximum's code is the same statements in both
// instantiations, span_score / span_cat may be NULL in this one.
//
// MODE = SPAN_TABLE (abcd_span_table, s3.13) keeps the per-prototype scores
// instead: after a step's last chunk every thread stores its own four S values
// (two starts x two prototypes, an excluded one as -inf) at table[(e D + t) ldk
// + p], table passed in span_lse's place.  No thread reads what another wrote
// and nothing is folded across the prototype tiles; the 16-lane reduction runs
// only when span_score / span_cat are asked for, with the statements of the
// other two instantiations.
constexpr int SPAN_MAX = 0, SPAN_LSE = 1, SPAN_TABLE = 2;

template <int MODE>
__global__ __launch_bounds__(256) void span_nll(const float* __restrict__ X, long ldx, long N, int F, int P, int D,
                                                const float* __restrict__ MU, long ldm,
                                                const float* __restrict__ LV, long ldl,
                                                const double* __restrict__ Otab, const float* __restrict__ LW,
                                                double* __restrict__ span_score, int32_t* __restrict__ span_cat,
                                                double* __restrict__ span_lse, long lds, long ldk) {
  constexpr bool LSE = MODE == SPAN_LSE, TAB = MODE == SPAN_TABLE;
  __shared__ EmTile tile;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const long s0 = (long)blockIdx.x * EM_TR;
  const int nst = (int)min((long)D, N - s0);  // the tile's first start has the most steps
  const int ti = tid >> 4, tj = tid & 15;
  const int nch = (F + EM_FC - 1) / EM_FC;  // passes per step
  const int nit = nst * nch;
  // gridDim.y > 1 (SPAN_TABLE without the best outputs, where nothing is folded across the prototype tiles): one
  // workgroup per tile, so a short slice of a recording (s3.15) still fills the device; otherwise all tiles in turn
  const int pfirst = gridDim.y > 1 ? (int)blockIdx.y * EM_TP : 0;
  const int pend = gridDim.y > 1 ? min(P, pfirst + EM_TP) : P;
  for (int p0 = pfirst; p0 < pend; p0 += EM_TP) {
    EmRegs g;
    auto fetch = [&](int it) {
      const int t = it / nch, c = it % nch, f = c * EM_FC + lane;
#pragma unroll
      for (int i = 0; i < EM_TR / 4; ++i) {
        const long row = s0 + t + w + 4 * i;
        g.x[i] = (f < F && row < N) ? X[row * ldx + f] : 0.f;
      }
      em_fetch_proto(g, MU, ldm, LV, ldl, w, t, p0, P, f, F);
    };
    const int pa = p0 + tj, pb = p0 + tj + 16;
    const double lwa = (pa < P && LW) ? (double)LW[pa] : 0.0, lwb = (pb < P && LW) ? (double)LW[pb] : 0.0;
    double em[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    float q[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    float csum[EM_TP / 4] = {};
    fetch(0);
    for (int it = 0; it < nit; ++it) {
      const int t = it / nch, c = it % nch, f0 = c * EM_FC, k = it & 1;
      const bool first = c == 0, last = c == nch - 1;
      tile.stage(k, g, csum, w, lane, p0, P, f0, F, first, last);
      __syncthreads();
      if (it + 1 < nit) fetch(it + 1);  // in flight while this pass is computed
      tile.accumulate(k, q, ti, tj, f0, F, first);
      if (last) {  // the frame is complete: one fp32 value per (start, prototype) joins the fp64 sum
        const float c0 = tile.cs[k][tj], c1 = tile.cs[k][tj + 16];
        const double oa = pa < P ? Otab[(long)t * P + pa] : 0.0, ob = pb < P ? Otab[(long)t * P + pb] : 0.0;
        double tm[2], tsum[2];  // LSE: the tile's maximum and sum_p exp(S - maximum) of the thread's two starts
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const long e = s0 + 2 * ti + i + t + 1;  // the end of start s0 + 2 ti + i at length t + 1
          const bool v = e <= N;
          if (v) {
            em[i][0] += (double)(c0 + 0.5f * q[i][0]);
            em[i][1] += (double)(c1 + 0.5f * q[i][1]);
          }
          double sa = pa < P ? lwa - em[i][0] - oa : -INFINITY;
          double sb = pb < P ? lwb - em[i][1] - ob : -INFINITY;
          int arg = pa, ab = pb;
          if (!(sa > -INFINITY)) { sa = -INFINITY; arg = INT_MAX; }  // NaN and -inf: excluded
          if (!(sb > -INFINITY)) { sb = -INFINITY; ab = INT_MAX; }
          const double ua = sa, ub = sb;
          if (TAB) {
            if (v) {
              double* const row = span_lse + (e * D + t) * ldk;
              if (pa < P) row[pa] = ua;
              if (pb < P) row[pb] = ub;
            }
            if (!span_score) continue;  // uniform: the whole workgroup skips the reduction
          }
          if (sb > sa) { sa = sb; arg = ab; }
          wave_argmax<16>(sa, arg);  // the 16 lanes of one start
          if (LSE) {
            double z = 0.0;  // an excluded prototype adds nothing; sa = -inf leaves every term out
            if (ua > -INFINITY) z += (double)__expf((float)(ua - sa));
            if (ub > -INFINITY) z += (double)__expf((float)(ub - sa));
            for (int o = 8; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
            tm[i] = sa;
            tsum[i] = z;
          }
          if (tj == 0 && v && (!LSE || span_score)) {
            const long at = e * lds + t;
            if (p0 == 0) {
              span_score[at] = sa;
              span_cat[at] = arg == INT_MAX ? -1 : arg;
            } else if (sa > span_score[at]) {  // a later tile holds higher indices: it needs a strictly better score
              span_score[at] = sa;
              span_cat[at] = arg;
            }
          }
        }
        if (LSE && tj < 2) {
          const long e = s0 + 2 * ti + tj + t + 1;
          if (e <= N) {
            const double m = tj ? tm[1] : tm[0], z = tj ? tsum[1] : tsum[0];
            const double here = m > -INFINITY ? m + log(z) : -INFINITY;
            const long at = e * lds + t;
            span_lse[at] = p0 == 0 ? here : logaddexp_d(span_lse[at], here);
          }
        }
      }
    }
    __syncthreads();  // the next prototype tile starts over at image 0
  }
}

constexpr int SV_THREADS = 256;  // the widest launch; D <= SV_ONE_WAVE_D runs as a single wave
constexpr int SV_ONE_WAVE_D = 256;
constexpr int SV_PRE = 4;  // span entries per thread loaded one step ahead (D <= 4 x the launch width runs from registers)

// (maximum, sum of exp(c - maximum)) with candidate c folded in: one exp per candidate
DEV void pair_fold(double& m, double& z, double c) {  // c = NaN or -inf: excluded
  if (c > -INFINITY) {
    const double w = exp(-fabs(m - c));  // m = -inf: 0
    if (c > m) { z = z * w + 1.0; m = c; } else z += w;
  }
}

// One workgroup, one launch: V[n] for n = 1 .. N, then the backtrack.
//   V[n] = max(V[n-1] + gap[n-1], max_{d_min <= d <= min(D, n)} (V[n-d] + span[n, d]) + bonus)
// Lanes stride over d; each thread's candidates in ascending d under a strict
// comparison, then a wave shuffle tree and the waves in order, the smaller d
// winning a tie; the gap wins a tie against the segment.  The step is a chain
// of dependent latencies, not throughput: up to D = 256 one wave takes four
// candidates per lane and its barrier and LDS exchange cost next to nothing;
// wider D runs on four waves.  NaN
// candidates fail every comparison.  V lives in a ring of D doubles in LDS.
// Every thread forms V[n] itself from the wave results, so the candidate
// d = 1 comes from a register and the ring entry thread 0 stores after barrier
// n is first read after barrier n + 1: one barrier per step.  The span row and
// the gap of step n + 1 do not depend on V and are loaded while step n reduces.
__global__ __launch_bounds__(SV_THREADS) void span_viterbi(const double* __restrict__ SS,
                                                           const int32_t* __restrict__ SC, long lds, long N, int D,
                                                           int dmin, const float* __restrict__ gap, double bonus,
                                                           double* __restrict__ path_score,
                                                           int32_t* __restrict__ n_segments,
                                                           int32_t* __restrict__ seg_onset,
                                                           int32_t* __restrict__ seg_length,
                                                           int32_t* __restrict__ seg_cat, double* __restrict__ seg_score,
                                                           double* __restrict__ V_out, int32_t* __restrict__ back) {
  extern __shared__ __attribute__((aligned(16))) double ring[];  // V[n] at n mod D
  __shared__ double wb[2][SV_THREADS / 64];
  __shared__ int wd[2][SV_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  if (tid == 0) {
    ring[0] = 0.0;
    back[0] = 0;
    if (V_out) V_out[0] = 0.0;
  }
  __syncthreads();
  double vprev = 0.0;
  double pre[SV_PRE];
  float gnext = 0.f;
  auto load_row = [&](long n) {
#pragma unroll
    for (int r = 0; r < SV_PRE; ++r) {
      const int d = tid + 1 + nt * r;  // an unconditional load from a clamped index: no branch, a counted wait
      pre[r] = SS[n * lds + min(d, D) - 1];  // used one step later, under the candidate's own mask
    }
    if (gap) gnext = gap[n - 1];
  };
  if (N >= 1) load_row(1);
  int pos = 0;  // (n - 1) mod D
  for (long n = 1; n <= N; ++n) {
    double cur[SV_PRE];
#pragma unroll
    for (int r = 0; r < SV_PRE; ++r) cur[r] = pre[r];
    const double gapc = gap ? vprev + (double)gnext : -INFINITY;
    if (n < N) load_row(n + 1);
    pos = pos + 1 == D ? 0 : pos + 1;  // n mod D
    const int dmax = (int)min((long)D, n);
    double best = -INFINITY;
    int bd = INT_MAX;
#pragma unroll
    for (int r = 0; r < SV_PRE; ++r) {
      const int d = tid + 1 + nt * r;
      int at = pos - min(d, D);
      at += at < 0 ? D : 0;
      const double v = ring[at];  // a slot not written yet (d > n) is read and masked
      const double c = (d == 1 ? vprev : v) + cur[r];
      const bool take = (d >= dmin) & (d <= dmax) & (c > best);
      best = take ? c : best;
      bd = take ? d : bd;
    }
    for (int d = tid + 1 + nt * SV_PRE; d <= dmax; d += nt) {
      if (d < dmin) continue;
      int at = pos - d;
      if (at < 0) at += D;
      const double c = ring[at] + SS[n * lds + d - 1];
      if (c > best) { best = c; bd = d; }
    }
    wave_argmax(best, bd);
    const int k = (int)(n & 1);
    if (lane == 0) { wb[k][w] = best; wd[k][w] = bd; }
    __syncthreads();
    best = wb[k][0];
    bd = wd[k][0];
    for (int i = 1; i < nw; ++i) {
      const double b2 = wb[k][i];
      const int d2 = wd[k][i];
      if (b2 > best || (b2 == best && d2 < bd)) { best = b2; bd = d2; }
    }
    const double seg = best + bonus;
    const bool vg = gapc > -INFINITY, vs = seg > -INFINITY && bd != INT_MAX;
    double V = -INFINITY;
    int choice = 0;  // 0: the gap (or nothing); d: a segment of d frames ends here
    if (vg && (!vs || gapc >= seg)) V = gapc;
    else if (vs) { V = seg; choice = bd; }
    vprev = V;
    if (tid == 0) {
      ring[pos] = V;
      back[n] = choice;
      if (V_out) V_out[n] = V;
    }
  }
  if (tid != 0) return;
  if (!(vprev > -INFINITY)) {  // the end cannot be reached
    *path_score = -INFINITY;
    *n_segments = 0;
    return;
  }
  int count = 0;
  for (long n = N; n > 0;) {
    const int d = back[n];
    if (d == 0) { --n; } else { ++count; n -= d; }
  }
  int i = count;
  for (long n = N; n > 0;) {
    const int d = back[n];
    if (d == 0) { --n; continue; }
    --i;
    seg_onset[i] = (int32_t)(n - d);
    seg_length[i] = d;
    seg_cat[i] = SC[n * lds + d - 1];
    seg_score[i] = SS[n * lds + d - 1];
    n -= d;
  }
  *n_segments = count;
  *path_score = vprev;
}

// The sum form of span_viterbi: one workgroup, one launch,
// the same launch widths, row prefetch and ring.  lat holds alpha, alpha_seg,
// beta, beta_seg, N + 1 doubles each.
//
// Forward, n = 1 .. N: the candidates alpha[n-d] + W[n,d] as in span_viterbi
// (four per thread from registers, the rest in a loop); their maximum over the
// thread, a wave shuffle tree and the waves in order; then each candidate's
// exp(c - maximum), summed the same way: one exp per candidate, one log per
// step.  Every thread forms alpha[n] itself, so d = 1 comes from a register
// and thread 0's ring store is first read two barriers later.
//
// Backward, e = N .. 0, over ENDS: beta_seg[s] = LSE_d (W[s+d,d] + bonus +
// beta[s+d]) reads an anti-diagonal of the end-major table, so the sweep walks
// the rows instead and thread d folds W[e,d] + bonus + beta[e] into the slot
// of start e - d with a logaddexp.  The ring has D + 1 slots, start s at s mod
// (D + 1): at step e the slots e-1 .. e-D are written, each by one thread, and
// slot e, complete since step e + 1, is only read, so one barrier per step
// orders everything.  The thread with d = D is the first to reach its start and
// starts from an empty slot; starts within D of the end find the empty slots
// the ring was filled with.  PAIR: a slot is (maximum, sum of exp(c - maximum)),
// the sums in a second ring behind the first, so a fold costs one exp and the
// logarithm is taken once per start, when the slot is read; it measured 24 %
// under the whole launch with log-domain slots (a logaddexp, exp and log1p, per
// fold) and is used while both rings fit the LDS the widest
// span_viterbi ring takes, D <= SF_PAIR_MAX_D.
//
// Then log_z = alpha[N] and the per-frame posteriors, elementwise from the
// lattice this workgroup wrote (a barrier apart).
constexpr int SF_PAIR_MAX_D = (SP_MAX_D + 1) / 2 - 1;  // 8191: 2 (D + 1) doubles in 128 KB

template <bool PAIR>
__global__ __launch_bounds__(SV_THREADS) void span_fb(const double* __restrict__ W, long ldw, long N, int D, int dmin,
                                                      const float* __restrict__ gap, double bonus, double* log_z,
                                                      double* lat, double* post) {
  extern __shared__ __attribute__((aligned(16))) double ring[];  // D + 1 slots (PAIR: twice)
  __shared__ double wm[SV_THREADS / 64], wz[SV_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  double* const A = lat;
  double* const AS = lat + (N + 1);
  double* const B = lat + 2 * (N + 1);
  double* const BS = lat + 3 * (N + 1);
  double pre[SV_PRE];
  float gnext = 0.f;
  auto load_row = [&](long n, long g) {  // row n of the table and gap[g] (g >= 0), both one step ahead of their use
#pragma unroll
    for (int r = 0; r < SV_PRE; ++r) {
      const int d = tid + 1 + nt * r;
      pre[r] = W[n * ldw + min(d, D) - 1];
    }
    if (gap && g >= 0) gnext = gap[g];
  };
  // ---- forward
  if (tid == 0) {
    ring[0] = 0.0;
    A[0] = 0.0;
    AS[0] = -INFINITY;
  }
  __syncthreads();
  double vprev = 0.0;
  if (N >= 1) load_row(1, 0);
  int pos = 0;  // (n - 1) mod D
  for (long n = 1; n <= N; ++n) {
    double cur[SV_PRE];
#pragma unroll
    for (int r = 0; r < SV_PRE; ++r) cur[r] = pre[r];
    const double gapc = gap ? vprev + (double)gnext : -INFINITY;
    if (n < N) load_row(n + 1, n);
    pos = pos + 1 == D ? 0 : pos + 1;  // n mod D
    const int dmax = (int)min((long)D, n);
    double m = -INFINITY;
#pragma unroll
    for (int r = 0; r < SV_PRE; ++r) {
      const int d = tid + 1 + nt * r;
      int at = pos - min(d, D);
      at += at < 0 ? D : 0;
      const double v = ring[at];  // a slot not written yet (d > n) is read and masked
      const double c = (d == 1 ? vprev : v) + cur[r];
      cur[r] = ((d >= dmin) & (d <= dmax) & (c > -INFINITY)) ? c : -INFINITY;  // NaN and -inf: excluded
      m = fmax(m, cur[r]);
    }
    for (int d = tid + 1 + nt * SV_PRE; d <= dmax; d += nt) {
      if (d < dmin) continue;
      int at = pos - d;
      if (at < 0) at += D;
      const double c = ring[at] + W[n * ldw + d - 1];
      if (c > m) m = c;
    }
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) wm[w] = m;
    __syncthreads();
    m = wm[0];
    for (int i = 1; i < nw; ++i) m = fmax(m, wm[i]);
    double z = 0.0;
    if (m > -INFINITY) {
#pragma unroll
      for (int r = 0; r < SV_PRE; ++r) z += cur[r] > -INFINITY ? exp(cur[r] - m) : 0.0;
      for (int d = tid + 1 + nt * SV_PRE; d <= dmax; d += nt) {
        if (d < dmin) continue;
        int at = pos - d;
        if (at < 0) at += D;
        const double c = ring[at] + W[n * ldw + d - 1];  // the same two operands as in the pass above
        if (c > -INFINITY) z += exp(c - m);
      }
    }
    z = wave_sum_d(z);
    if (lane == 0) wz[w] = z;
    __syncthreads();
    z = wz[0];
    for (int i = 1; i < nw; ++i) z += wz[i];
    const double aseg = m > -INFINITY ? bonus + (m + log(z)) : -INFINITY;
    const double a = logaddexp_d(gapc, aseg);
    vprev = a;
    if (tid == 0) {
      ring[pos] = a;
      A[n] = a;
      AS[n] = aseg;
    }
  }
  // ---- backward
  __syncthreads();
  const int R = D + 1;
  double* const ring2 = ring + R;  // PAIR: the sums
  for (int i = tid; i < R; i += nt) {
    ring[i] = -INFINITY;
    if (PAIR) ring2[i] = 0.0;
  }
  auto fold = [&](int at, int d, double c) {  // candidate c (-inf: none) of length d into the slot of its start
    double mo = ring[at], zo = PAIR ? ring2[at] : 0.0;
    if (d == D) { mo = -INFINITY; zo = 0.0; }  // the first to reach this start: the slot's earlier start is done
    if (PAIR) {
      pair_fold(mo, zo, c);
      ring[at] = mo;
      ring2[at] = zo;
    } else {
      ring[at] = logaddexp_d(mo, c);
    }
  };
  if (N >= 1) load_row(N, -1);  // step e uses row e and gap[e]; step N has no gap
  double bnext = 0.0;
  int slot = (int)(N % R);  // e mod (D + 1)
  for (long e = N; e >= 0; --e) {
    double cur[SV_PRE];
#pragma unroll
    for (int r = 0; r < SV_PRE; ++r) cur[r] = pre[r];
    const float gnow = gnext;
    if (e >= 1) load_row(e - 1, e - 1);  // row 0 exists (all -inf) and is not used
    __syncthreads();
    double b = 0.0, bseg = -INFINITY;
    if (e < N) {
      bseg = ring[slot];
      if (PAIR) bseg = bseg > -INFINITY ? bseg + log(ring2[slot]) : -INFINITY;
      b = logaddexp_d(gap ? (double)gnow + bnext : -INFINITY, bseg);
    }
    bnext = b;
    if (tid == 0) {
      B[e] = b;
      BS[e] = bseg;
    }
    if (e >= 1) {
      const int dmax = (int)min((long)D, e);
#pragma unroll
      for (int r = 0; r < SV_PRE; ++r) {
        const int d = tid + 1 + nt * r;
        if (d <= dmax) {
          int at = slot - d;
          at += at < 0 ? R : 0;
          double c = (cur[r] + bonus) + b;
          if (!((d >= dmin) & (c > -INFINITY))) c = -INFINITY;
          fold(at, d, c);
        }
      }
      for (int d = tid + 1 + nt * SV_PRE; d <= dmax; d += nt) {
        int at = slot - d;
        if (at < 0) at += R;
        double c = (W[e * ldw + d - 1] + bonus) + b;
        if (!((d >= dmin) & (c > -INFINITY))) c = -INFINITY;
        fold(at, d, c);
      }
    }
    slot = slot == 0 ? R - 1 : slot - 1;
  }
  // ---- log_z and the per-frame posteriors
  __syncthreads();
  const double lz = A[N];
  if (tid == 0 && log_z) *log_z = lz;
  if (!post) return;
  const bool reach = lz > -INFINITY;
  for (long n = tid; n <= N; n += nt) {
    double on = 0.0, en = 0.0, gp = 0.0;
    if (reach) {
      if (n < N) on = exp(A[n] + BS[n] - lz);
      if (n >= 1) en = exp(AS[n] + B[n] - lz);
      if (n < N && gap) gp = exp(A[n] + (double)gap[n] + B[n + 1] - lz);
    }
    post[n] = on > 0.0 ? on : 0.0;  // a NaN (inf - inf, outside the contract) reads as 0
    post[(N + 1) + n] = en > 0.0 ? en : 0.0;
    post[2 * (N + 1) + n] = gp > 0.0 ? gp : 0.0;
  }
}

// span_post[e, d - 1] = exp(alpha[e-d] + W[e,d] + bonus + beta[e] - log_z), 0 outside d_min .. min(D, e)
__global__ __launch_bounds__(256) void span_post_table(const double* __restrict__ W, long ldw, long N, int D, int dmin,
                                                       double bonus, const double* __restrict__ lat,
                                                       double* __restrict__ span_post, long ldp) {
  const long at = (long)blockIdx.x * 256 + threadIdx.x;
  if (at >= (N + 1) * D) return;
  const long e = at / D;
  const int d = (int)(at - e * D) + 1;
  const double lz = lat[N];
  double v = 0.0;
  if (d >= dmin && d <= e && lz > -INFINITY) {
    const double c = ((lat[e - d] + W[e * ldw + d - 1]) + bonus) + lat[2 * (N + 1) + e];
    if (c > -INFINITY) v = exp(c - lz);
  }
  span_post[e * ldp + d - 1] = v > 0.0 ? v : 0.0;
}

// the table entries with d > e (row 0 among them), prototypes < P: -inf
__global__ __launch_bounds__(256) void span_table_fill(long rows, int D, int P, double* __restrict__ table, long ldk) {
  const long at = (long)blockIdx.x * 256 + threadIdx.x;
  if (at >= rows * D * P) return;
  const long ec = at / P;
  const int p = (int)(at - ec * P);
  const long e = ec / D;
  const int c = (int)(ec - e * D);  // d - 1
  if (c < e) return;
  table[ec * ldk + p] = -INFINITY;
}

// span_viterbi with category transitions: one workgroup, one
// launch, the state is (frame, last category).
//   G[n]     = G[n-1] + gap[n-1]                                  no segment yet
//   U[n][k]  = max(G[n] + log_init[k], max_k' (W[n][k'] + log_trans[k'][k]))
//   Vs[n][k] = max_{d_min <= d <= min(D, n)} (U[n-d][k] + T[n,d,k]) + bonus
//   W[n][k]  = max(W[n-1][k] + gap[n-1], Vs[n][k])
// Lanes run over k in both maxima, so a table row T[n,d,:], a lattice row
// U[n-d,:] and a matrix row log_trans[k',:] are read contiguously; the waves
// (16 up to K = SC_WIDE_K, 4 above: the partial results must fit LDS) split d
// (phase A) and k' (phase B), each thread taking its candidates in ascending
// order under a strict comparison, and the waves' partial results of a k meet
// in LDS and are combined in wave order with the tie rule spelled out (the
// smaller d, the lower k'), so no comparison is decided by scheduling.  The
// step is latency: 16 waves keep 16 rows of the table in flight at once.
// The gap wins a tie in W, the initial term in U.  NaN and -inf candidates fail
// every comparison.  U and the two back-pointer planes (d, 0 for the gap; k',
// -1 for the initial term) live in the workspace: the workgroup reads its own
// global stores a barrier later.  W[n] and log_init stay in LDS; RES keeps
// log_trans there too (K <= SC_RES_K), otherwise its rows stream from global
// memory.  U[N] is not formed: no segment starts at N.
constexpr int SC_THREADS = 1024;  // the widest launch
constexpr int SC_WIDE_K = 256;    // 16 waves up to here, 4 above
constexpr int SC_RES_K = 128;   // log_trans resident in LDS (64 KB) up to here
constexpr int SC_MAX_K = 1024;

static int span_chain_waves(int K) { return K <= SC_WIDE_K ? SC_THREADS / 64 : 4; }

static size_t span_chain_lds(int K) {
  const int nw = span_chain_waves(K);
  return (size_t)K * ((2 + nw) * sizeof(double) + nw * sizeof(int)) +
         (K <= SC_RES_K ? (size_t)K * K * sizeof(float) : 0);
}

// The step, shared by span_chain and span_chain_win (s3.15); the whole workgroup
// calls each function with a barrier between them.  `row` is the table's row
// of end n: n itself for the whole table, n - row0 for a window.
// ---- phase A: the best segment of each k that ends at n
DEV void sc_phase_a(const double* __restrict__ T, long ldk, long row, const double* U, long n, int D, int K, int dmin,
                    int lane, int w, int nw, double* pv, int* pa) {
  const int dmax = (int)min((long)D, n);
  for (int k = lane; k < K; k += 64) {
    double best = -INFINITY;
    int bd = INT_MAX;
    const double* const Trow = T + (row * D - 1) * ldk + k;  // + d ldk
    const double* const Urow = U + n * K + k;                 // - d K
#pragma unroll 4
    for (int d = dmin + w; d <= dmax; d += nw) {
      const double c = Urow[-(long)d * K] + Trow[(long)d * ldk];
      if (c > best) { best = c; bd = d; }
    }
    pv[w * K + k] = best;
    pa[w * K + k] = bd;
  }
}

// the waves' partial results of phase A in wave order, then W[n]; KEEP also stores the chosen segment's table entry
template <bool KEEP>
DEV void sc_combine_a(const double* __restrict__ T, long ldk, long row, long n, int D, int K, int tid, int nt, int nw,
                      const double* pv, const int* pa, double bonus, double gv, double* Wc, int32_t* back_d,
                      double* __restrict__ W_out, double* sel) {
  for (int k = tid; k < K; k += nt) {
    double best = pv[k];
    int bd = pa[k];
    for (int i = 1; i < nw; ++i) {
      const double b2 = pv[i * K + k];
      const int d2 = pa[i * K + k];
      if (b2 > best || (b2 == best && d2 < bd)) { best = b2; bd = d2; }
    }
    const double seg = best + bonus, gapc = Wc[k] + gv;
    const bool vg = gapc > -INFINITY, vs = seg > -INFINITY && bd != INT_MAX;
    double Wn = -INFINITY;
    int choice = 0;  // 0: the gap (or nothing); d: a segment of k of d frames ends here
    if (vg && (!vs || gapc >= seg)) Wn = gapc;
    else if (vs) { Wn = seg; choice = bd; }
    Wc[k] = Wn;
    back_d[n * K + k] = choice;
    if (W_out) W_out[n * K + k] = Wn;
    if (KEEP) sel[n * K + k] = choice ? T[(row * D + choice - 1) * ldk + k] : -INFINITY;
  }
}

// ---- phase B: the best way into a segment of k that starts at n
template <bool RES>
DEV void sc_phase_b(const double* Wc, const float* lt, const float* __restrict__ LT, long ldt, int K, int lane, int w,
                    int nw, double* pv, int* pa) {
  for (int k = lane; k < K; k += 64) {
    double best = -INFINITY;
    int bk = INT_MAX;
#pragma unroll 4
    for (int kp = w; kp < K; kp += nw) {
      const double c = Wc[kp] + (double)(RES ? lt[kp * K + k] : LT[(long)kp * ldt + k]);
      if (c > best) { best = c; bk = kp; }
    }
    pv[w * K + k] = best;
    pa[w * K + k] = bk;
  }
}

// the waves' partial results of phase B in wave order, then U[n]
DEV void sc_combine_b(long n, int K, int tid, int nt, int nw, const double* pv, const int* pa, double G,
                      const double* Li, double* U, int32_t* back_k) {
  for (int k = tid; k < K; k += nt) {
    double best = pv[k];
    int bk = pa[k];
    for (int i = 1; i < nw; ++i) {
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
    U[n * K + k] = Un;
    back_k[n * K + k] = from;
  }
}

// one thread: path_score and the walk from (N, best k) into the segment lists; seg_score from the table, KEEP: from sel
template <bool KEEP>
DEV void sc_backtrack(const double* __restrict__ T, long ldk, int D, const double* sel, long N, int K, double G,
                      const double* Wc, const double* Li, const float* __restrict__ LT, long ldt,
                      const int32_t* back_d, const int32_t* back_k, double* __restrict__ path_score,
                      int32_t* __restrict__ n_segments, int32_t* __restrict__ seg_onset,
                      int32_t* __restrict__ seg_length, int32_t* __restrict__ seg_cat, double* __restrict__ seg_score,
                      double* __restrict__ seg_link) {
  double best = G > -INFINITY ? G : -INFINITY;  // "no segment" wins a tie, then the lowest k
  int kb = -1;
  for (int k = 0; k < K; ++k)
    if (Wc[k] > best) { best = Wc[k]; kb = k; }
  *path_score = best;
  int count = 0;
  {
    long n = N;
    int k = kb;
    while (k >= 0 && n > 0) {
      const int d = back_d[n * K + k];
      if (d == 0) { --n; continue; }
      ++count;
      n -= d;
      k = back_k[n * K + k];
    }
  }
  *n_segments = count;
  int i = count;
  long n = N;
  int k = kb;
  while (k >= 0 && n > 0) {
    const int d = back_d[n * K + k];
    if (d == 0) { --n; continue; }
    --i;
    seg_onset[i] = (int32_t)(n - d);
    seg_length[i] = d;
    seg_cat[i] = k;
    seg_score[i] = KEEP ? sel[n * K + k] : T[(n * D + d - 1) * ldk + k];
    n -= d;
    const int from = back_k[n * K + k];
    seg_link[i] = from < 0 ? Li[k] : (double)LT[(long)from * ldt + k];
    k = from;
  }
}

template <bool RES>
__global__ __launch_bounds__(SC_THREADS) void span_chain(
    const double* __restrict__ T, long ldk, long N, int D, int K, int dmin, const float* __restrict__ gap, double bonus,
    const float* __restrict__ LT, long ldt, const float* __restrict__ LI, double* __restrict__ path_score,
    int32_t* __restrict__ n_segments, int32_t* __restrict__ seg_onset, int32_t* __restrict__ seg_length,
    int32_t* __restrict__ seg_cat, double* __restrict__ seg_score, double* __restrict__ seg_link,
    double* __restrict__ W_out, double* U, int32_t* back_d, int32_t* back_k) {
  extern __shared__ __attribute__((aligned(16))) double sc_lds[];
  double* const Wc = sc_lds;                        // W[n][k]
  double* const Li = Wc + K;                        // log_init, widened
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  double* const pv = Li + K;                        // the waves' partial maxima, nw x K
  int* const pa = (int*)(pv + nw * K);              // and their arguments
  const float* const lt = (const float*)(pa + nw * K);  // RES: K x K
  for (int k = tid; k < K; k += nt) {
    const double li = (double)LI[k];
    Wc[k] = -INFINITY;
    Li[k] = li;
    U[k] = li;  // G[0] = 0 and W[0] = -inf: the initial term
    back_k[k] = -1;
    if (W_out) W_out[k] = -INFINITY;
  }
  if (RES) {
    float* const dst = (float*)(pa + nw * K);
    for (int i = tid; i < K * K; i += nt) dst[i] = LT[(long)(i / K) * ldt + i % K];
  }
  __syncthreads();
  double G = 0.0;
  for (long n = 1; n <= N; ++n) {
    const double gv = gap ? (double)gap[n - 1] : -INFINITY;
    G = G + gv;
    // ---- phase A: the best segment of each k that ends at n
    const int dmax = (int)min((long)D, n);
    for (int k = lane; k < K; k += 64) {
      double best = -INFINITY;
      int bd = INT_MAX;
      const double* const Trow = T + (n * D - 1) * ldk + k;  // + d ldk
      const double* const Urow = U + n * K + k;               // - d K
#pragma unroll 4
      for (int d = dmin + w; d <= dmax; d += nw) {
        const double c = Urow[-(long)d * K] + Trow[(long)d * ldk];
        if (c > best) { best = c; bd = d; }
      }
      pv[w * K + k] = best;
      pa[w * K + k] = bd;
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
      double best = pv[k];
      int bd = pa[k];
      for (int i = 1; i < nw; ++i) {
        const double b2 = pv[i * K + k];
        const int d2 = pa[i * K + k];
        if (b2 > best || (b2 == best && d2 < bd)) { best = b2; bd = d2; }
      }
      const double seg = best + bonus, gapc = Wc[k] + gv;
      const bool vg = gapc > -INFINITY, vs = seg > -INFINITY && bd != INT_MAX;
      double Wn = -INFINITY;
      int choice = 0;  // 0: the gap (or nothing); d: a segment of k of d frames ends here
      if (vg && (!vs || gapc >= seg)) Wn = gapc;
      else if (vs) { Wn = seg; choice = bd; }
      Wc[k] = Wn;
      back_d[n * K + k] = choice;
      if (W_out) W_out[n * K + k] = Wn;
    }
    __syncthreads();
    if (n == N) break;
    // ---- phase B: the best way into a segment of k that starts at n
    for (int k = lane; k < K; k += 64) {
      double best = -INFINITY;
      int bk = INT_MAX;
#pragma unroll 4
      for (int kp = w; kp < K; kp += nw) {
        const double c = Wc[kp] + (double)(RES ? lt[kp * K + k] : LT[(long)kp * ldt + k]);
        if (c > best) { best = c; bk = kp; }
      }
      pv[w * K + k] = best;
      pa[w * K + k] = bk;
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
      double best = pv[k];
      int bk = pa[k];
      for (int i = 1; i < nw; ++i) {
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
      U[n * K + k] = Un;
      back_k[n * K + k] = from;
    }
    __syncthreads();
  }
  if (tid != 0) return;
  double best = G > -INFINITY ? G : -INFINITY;  // "no segment" wins a tie, then the lowest k
  int kb = -1;
  for (int k = 0; k < K; ++k)
    if (Wc[k] > best) { best = Wc[k]; kb = k; }
  *path_score = best;
  int count = 0;
  {
    long n = N;
    int k = kb;
    while (k >= 0 && n > 0) {
      const int d = back_d[n * K + k];
      if (d == 0) { --n; continue; }
      ++count;
      n -= d;
      k = back_k[n * K + k];
    }
  }
  *n_segments = count;
  int i = count;
  long n = N;
  int k = kb;
  while (k >= 0 && n > 0) {
    const int d = back_d[n * K + k];
    if (d == 0) { --n; continue; }
    --i;
    seg_onset[i] = (int32_t)(n - d);
    seg_length[i] = d;
    seg_cat[i] = k;
    seg_score[i] = T[(n * D + d - 1) * ldk + k];
    n -= d;
    const int from = back_k[n * K + k];
    seg_link[i] = from < 0 ? Li[k] : (double)LT[(long)from * ldt + k];
    k = from;
  }
}

// span_chain in windows of ends: steps n0 .. n1 of the same
// recurrences with span_chain's launch widths, partition, tie rules and LDS
// plan, the step being the sc_* functions above.  T is a window of the table:
// its row 0 is absolute end row0, so step n reads row n - row0 (rows n0 - row0
// .. n1 - row0 and nothing else).  What the next launch needs is carried in the
// workspace: the lattice U (phase B runs at n1 too unless n1 = N, so U[n1] is
// there), the two back-pointer planes, `sel` (the chosen segment's table entry
// per (n, k): the table is gone by backtrack time) and the carry block, W[n1]
// (K doubles), G[n1] and next_n = n1 + 1.  n0 = 1 initialises as span_chain
// does; any other n0 must equal the carried next_n, otherwise the launch
// writes path_score = NaN and n_segments = -1 and touches nothing else.  The
// launch with n1 = N writes path_score and walks the back-pointers.  log_init
// and (RES) log_trans are reloaded into LDS by every launch.
template <bool RES>
__global__ __launch_bounds__(SC_THREADS) void span_chain_win(
    const double* __restrict__ T, long ldk, long row0, long n0, long n1, long N, int D, int K, int dmin,
    const float* __restrict__ gap, double bonus, const float* __restrict__ LT, long ldt, const float* __restrict__ LI,
    double* __restrict__ path_score, int32_t* __restrict__ n_segments, int32_t* __restrict__ seg_onset,
    int32_t* __restrict__ seg_length, int32_t* __restrict__ seg_cat, double* __restrict__ seg_score,
    double* __restrict__ seg_link, double* __restrict__ W_out, double* U, int32_t* back_d, int32_t* back_k,
    double* sel, double* carry) {
  extern __shared__ __attribute__((aligned(16))) double sc_lds[];
  double* const Wc = sc_lds;                        // W[n][k]
  double* const Li = Wc + K;                        // log_init, widened
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  double* const pv = Li + K;                        // the waves' partial maxima, nw x K
  int* const pa = (int*)(pv + nw * K);              // and their arguments
  const float* const lt = (const float*)(pa + nw * K);  // RES: K x K
  long* const next_n = (long*)(carry + K + 1);
  const bool fresh = n0 == 1;
  if (!fresh && *next_n != n0) {  // uniform: every thread reads the same word, nobody has written it yet
    if (tid == 0) {
      *path_score = __builtin_nan("");
      *n_segments = -1;
    }
    return;
  }
  for (int k = tid; k < K; k += nt) {
    const double li = (double)LI[k];
    Li[k] = li;
    if (fresh) {
      Wc[k] = -INFINITY;
      U[k] = li;  // G[0] = 0 and W[0] = -inf: the initial term
      back_k[k] = -1;
      if (W_out) W_out[k] = -INFINITY;
    } else {
      Wc[k] = carry[k];
    }
  }
  if (RES) {
    float* const dst = (float*)(pa + nw * K);
    for (int i = tid; i < K * K; i += nt) dst[i] = LT[(long)(i / K) * ldt + i % K];
  }
  double G = fresh ? 0.0 : carry[K];
  __syncthreads();
  for (long n = n0; n <= n1; ++n) {
    const double gv = gap ? (double)gap[n - 1] : -INFINITY;
    G = G + gv;
    sc_phase_a(T, ldk, n - row0, U, n, D, K, dmin, lane, w, nw, pv, pa);
    __syncthreads();
    sc_combine_a<true>(T, ldk, n - row0, n, D, K, tid, nt, nw, pv, pa, bonus, gv, Wc, back_d, W_out, sel);
    __syncthreads();
    if (n == N) break;
    sc_phase_b<RES>(Wc, lt, LT, ldt, K, lane, w, nw, pv, pa);
    __syncthreads();
    sc_combine_b(n, K, tid, nt, nw, pv, pa, G, Li, U, back_k);
    __syncthreads();
  }
  for (int k = tid; k < K; k += nt) carry[k] = Wc[k];
  if (tid != 0) return;
  carry[K] = G;
  *next_n = n1 + 1;
  if (n1 != N) return;
  sc_backtrack<true>(nullptr, 0, D, sel, N, K, G, Wc, Li, LT, ldt, back_d, back_k, path_score, n_segments, seg_onset,
                     seg_length, seg_cat, seg_score, seg_link);
}

// The sum form of span_chain: one workgroup, one launch, both
// sweeps over the state (frame, last category), span_chain's launch widths and
// partition.  Every term (table, gap, bonus, log_trans, log_init) is multiplied
// by `scale` in fp64 after widening; bonus arrives multiplied.
//   forward   aU / aV / aW as U / Vs / W of span_chain with LSE for max and LAE
//             for the two-term maxima
//   backward  n = N-1 .. 0 over STARTS: bU[n][k] = LSE_d (T[n+d,d,k] + bonus +
//             bW[n+d][k]) reads K contiguous doubles per d, as the forward does;
//             bW[n][k] = LAE(gap[n] + bW[n+1][k], LSE_k'' (lt[k][k''] + bU[n][k'']))
// A thread folds its candidates in ascending order into a pair (maximum, sum of
// exp(c - maximum)): one exp per candidate.  The waves' pairs of a k meet in
// LDS and thread k joins them in wave order, one log per k and phase.  RES
// keeps log_trans in LDS at a row stride of K + 1 floats: the forward reads
// along a row, the backward chain phase (lanes over the ROW index k) at stride
// K + 1 = 1 mod 64 banks.  Streamed (K > SC_RES_K), the backward chain phase
// gives each wave whole rows instead, lanes over k'' (contiguous in global
// memory), and joins the lanes' pairs by an xor butterfly: the join is
// symmetric, so every lane holds the same bits.
// The five lattice planes ((N + 1) x K each) and G / bG live in global memory;
// the workgroup reads its own stores a barrier later.  The expected counts are
// accumulated in the backward sweep (log_z is known by then) into the caller's
// buffers: thread (wave w, lane l) owns the entries (k' = w mod waves, k = l mod
// 64), the forward chain phase's partition, and adds to them in n order.  After
// the sweeps: bG (the per-frame LSE over k by one wave per frame, then the
// recursion over n by wave 0, 64 frames loaded at a time), the gap posterior
// (one wave per frame) and the per-(frame, category) posteriors, elementwise.
// No atomics, no device-global word.
// the parts pairs of k at pm / pz [i K + k], joined in order; -inf over none
DEV double pair_join(const double* pm, const double* pz, int parts, int K, int k) {
  double M = -INFINITY;
  for (int i = 0; i < parts; ++i) M = fmax(M, pm[i * K + k]);
  if (!(M > -INFINITY)) return -INFINITY;
  double Z = 0.0;
  for (int i = 0; i < parts; ++i) Z += pz[i * K + k] * exp(pm[i * K + k] - M);  // an empty pair: 0 * 0
  return M + log(Z);
}

// every lane's pair joined across the wave (all lanes end with the same bits); -inf over none
DEV double pair_wave_lse(double m, double z) {
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

static size_t span_chain_fb_lds(int K) {
  const int nw = span_chain_waves(K);
  // bW / aW of the step, log_init, bU of the step, aW[n] for the counts; the waves' pairs; RES: the matrix
  return (size_t)K * (4 + 2 * nw) * sizeof(double) + (K <= SC_RES_K ? (size_t)K * (K + 1) * sizeof(float) : 0);
}

template <bool RES>
__global__ __launch_bounds__(SC_THREADS) void span_chain_fb(
    const double* __restrict__ T, long ldk, long N, int D, int K, int dmin, const float* __restrict__ gap, double bonus,
    double scale, const float* __restrict__ LT, long ldt, const float* __restrict__ LI, double* log_z, double* lat,
    double* latg, double* post_k, double* gap_post, double* tc, double* ic) {
  extern __shared__ __attribute__((aligned(16))) double sc_lds[];
  __shared__ double lz_sh;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  double* const Wc = sc_lds;         // aW[n] (forward), bW[n + 1] (backward)
  double* const Li = Wc + K;         // scale * log_init
  double* const Bu = Li + K;         // bU[n]
  double* const Aw = Bu + K;         // aW[n], for the counts
  double* const pm = Aw + K;         // the waves' pairs, nw x K each
  double* const pz = pm + nw * K;
  const float* const lt = (const float*)(pz + nw * K);  // RES: K rows of K + 1
  const int lds_t = K + 1;
  const long P = (N + 1) * K;
  double* const aU = lat;
  double* const aV = lat + P;
  double* const aW = lat + 2 * P;
  double* const bU = lat + 3 * P;
  double* const bW = lat + 4 * P;
  double* const Gp = latg;
  double* const bG = latg + (N + 1);
  auto trans = [&](int kp, int k) {  // scale * log_trans[kp][k]
    return scale * (double)(RES ? lt[kp * lds_t + k] : LT[(long)kp * ldt + k]);
  };
  for (int k = tid; k < K; k += nt) {
    const double li = scale * (double)LI[k];
    Wc[k] = -INFINITY;
    Li[k] = li;
    aU[k] = li > -INFINITY ? li : -INFINITY;  // G[0] = 0 and aW[0] = -inf: the initial term
    aV[k] = -INFINITY;
    aW[k] = -INFINITY;
  }
  if (RES) {
    float* const dst = (float*)(pz + nw * K);
    for (int i = tid; i < K * K; i += nt) dst[(i / K) * lds_t + i % K] = LT[(long)(i / K) * ldt + i % K];
  }
  if (tid == 0) Gp[0] = 0.0;
  __syncthreads();
  // ---- forward
  double G = 0.0;
  for (long n = 1; n <= N; ++n) {
    const double gv = gap ? scale * (double)gap[n - 1] : -INFINITY;
    G = G + gv;
    const int dmax = (int)min((long)D, n);
    for (int k = lane; k < K; k += 64) {
      double m = -INFINITY, z = 0.0;
      const double* const Trow = T + (n * D - 1) * ldk + k;  // + d ldk
      const double* const Urow = aU + n * K + k;              // - d K
#pragma unroll 4
      for (int d = dmin + w; d <= dmax; d += nw) pair_fold(m, z, Urow[-(long)d * K] + scale * Trow[(long)d * ldk]);
      pm[w * K + k] = m;
      pz[w * K + k] = z;
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
      const double seg = pair_join(pm, pz, nw, K, k);
      const double av = seg > -INFINITY ? bonus + seg : -INFINITY;
      const double aw = logaddexp_d(Wc[k] + gv, av);
      Wc[k] = aw;
      aV[n * K + k] = av;
      aW[n * K + k] = aw;
      if (n == N) aU[n * K + k] = -INFINITY;  // no segment starts at N
    }
    if (tid == 0) Gp[n] = G;
    __syncthreads();
    if (n == N) break;
    for (int k = lane; k < K; k += 64) {
      double m = -INFINITY, z = 0.0;
#pragma unroll 4
      for (int kp = w; kp < K; kp += nw) pair_fold(m, z, Wc[kp] + trans(kp, k));
      pm[w * K + k] = m;
      pz[w * K + k] = z;
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) aU[n * K + k] = logaddexp_d(G + Li[k], pair_join(pm, pz, nw, K, k));
    __syncthreads();
  }
  if (tid == 0) {  // log_z = LAE(G[N], LSE_k aW[N][k])
    double m = -INFINITY, z = 0.0;
    for (int k = 0; k < K; ++k) pair_fold(m, z, Wc[k]);
    const double lz = logaddexp_d(G, m > -INFINITY ? m + log(z) : -INFINITY);
    lz_sh = lz;
    *log_z = lz;
  }
  __syncthreads();
  const double lz = lz_sh;
  // ---- backward
  for (int k = tid; k < K; k += nt) {
    Wc[k] = 0.0;
    bW[N * K + k] = 0.0;
    bU[N * K + k] = -INFINITY;
  }
  if (tc) {  // each entry by the thread that adds to it below
    for (int kp = w; kp < K; kp += nw)
      for (int k = lane; k < K; k += 64) tc[(long)kp * K + k] = 0.0;
    for (int k = tid; k < K; k += nt) ic[k] = 0.0;
  }
  __syncthreads();
  const bool count = tc && lz > -INFINITY;
  for (long n = N - 1; n >= 0; --n) {
    const double gv = gap ? scale * (double)gap[n] : -INFINITY;
    const int dmax = (int)min((long)D, N - n);
    for (int k = lane; k < K; k += 64) {
      double m = -INFINITY, z = 0.0;
      const double* const Trow = T + (n * D - 1) * ldk + k;  // + d (D + 1) ldk: row n + d, column d - 1
      const double* const Brow = bW + n * K + k;              // + d K
#pragma unroll 4
      for (int d = dmin + w; d <= dmax; d += nw)
        pair_fold(m, z, (scale * Trow[(long)d * (D + 1) * ldk] + bonus) + Brow[(long)d * K]);
      pm[w * K + k] = m;
      pz[w * K + k] = z;
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
      const double bu = pair_join(pm, pz, nw, K, k);
      Bu[k] = bu;
      bU[n * K + k] = bu;
      if (count) {
        Aw[k] = aW[n * K + k];
        const double c = (Gp[n] + Li[k]) + bu - lz;
        if (c > -INFINITY) ic[k] += exp(c);
      }
    }
    __syncthreads();
    int parts = nw;
    if (RES) {
      for (int k = lane; k < K; k += 64) {  // lanes over the row index
        double m = -INFINITY, z = 0.0;
#pragma unroll 4
        for (int kq = w; kq < K; kq += nw) pair_fold(m, z, trans(k, kq) + Bu[kq]);
        pm[w * K + k] = m;
        pz[w * K + k] = z;
      }
    } else {
      parts = 1;
      for (int k = w; k < K; k += nw) {  // a wave per row, lanes along it
        double m = -INFINITY, z = 0.0;
        for (int kq = lane; kq < K; kq += 64) pair_fold(m, z, trans(k, kq) + Bu[kq]);
        const double v = pair_wave_lse(m, z);
        if (lane == 0) { pm[k] = v; pz[k] = 1.0; }
      }
    }
    if (count) {
      for (int kp = w; kp < K; kp += nw) {
        const double a = Aw[kp];
        if (!(a > -INFINITY)) continue;  // uniform over the wave
        for (int k = lane; k < K; k += 64) {
          const double c = (a + trans(kp, k)) + Bu[k] - lz;
          if (c > -INFINITY) tc[(long)kp * K + k] += exp(c);
        }
      }
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
      const double bw = logaddexp_d(gv + Wc[k], pair_join(pm, pz, parts, K, k));
      Wc[k] = bw;
      bW[n * K + k] = bw;
    }
    __syncthreads();
  }
  // ---- bG: LSE_k (li[k] + bU[n][k]) per frame, then the recursion over n
  if (tid == 0) bG[N] = 0.0;
  for (long n = w; n < N; n += nw) {
    double m = -INFINITY, z = 0.0;
    for (int k = lane; k < K; k += 64) pair_fold(m, z, Li[k] + bU[n * K + k]);
    const double v = pair_wave_lse(m, z);
    if (lane == 0) bG[n] = v;
  }
  __syncthreads();
  if (w == 0) {
    double b = 0.0;
    for (long base = N - 1; base >= 0; base -= 64) {
      const long at = base - lane;
      const double q = at >= 0 ? bG[at] : -INFINITY;
      const double g = (at >= 0 && gap) ? scale * (double)gap[at] : -INFINITY;
      double mine = -INFINITY;
      for (int j = 0; j < 64; ++j) {
        b = logaddexp_d(__shfl(g, j, 64) + b, __shfl(q, j, 64));
        if (lane == j) mine = b;
      }
      if (at >= 0) bG[at] = mine;
    }
  }
  __syncthreads();
  // ---- the posteriors
  const bool reach = lz > -INFINITY;
  for (long n = w; n <= N; n += nw) {
    double gp = 0.0;
    if (n < N && gap && reach) {
      double m = -INFINITY, z = 0.0;
      for (int k = lane; k < K; k += 64) pair_fold(m, z, aW[n * K + k] + bW[(n + 1) * K + k]);
      const double in = logaddexp_d(Gp[n] + bG[n + 1], pair_wave_lse(m, z));
      const double c = in + scale * (double)gap[n] - lz;
      if (c > -INFINITY) gp = exp(c);
    }
    if (lane == 0) gap_post[n] = gp > 0.0 ? gp : 0.0;
  }
  for (long i = tid; i < P; i += nt) {
    double on = 0.0, en = 0.0;
    if (reach) {
      on = exp(aU[i] + bU[i] - lz);
      en = exp(aV[i] + bW[i] - lz);
    }
    post_k[i] = on > 0.0 ? on : 0.0;  // a NaN (inf - inf, outside the contract) reads as 0
    post_k[P + i] = en > 0.0 ? en : 0.0;
  }
}

// span_post[e, d - 1] = sum_k exp(aU[e-d][k] + scale T[e,d,k] + bonus + bW[e][k] - log_z), 0 outside d_min ..
// min(D, e): 16 lanes per entry, strided over k, their sums joined by an xor butterfly
__global__ __launch_bounds__(256) void span_chain_post_table(const double* __restrict__ T, long ldk, long N, int D,
                                                             int K, int dmin, double bonus, double scale,
                                                             const double* __restrict__ lat,
                                                             const double* __restrict__ log_z,
                                                             double* __restrict__ span_post, long ldp) {
  const long at = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  const bool in = at < (N + 1) * D;  // whole 16-lane groups leave the sums together
  const long e = in ? at / D : 0;
  const int d = in ? (int)(at - e * D) + 1 : 1;
  const double lz = *log_z;
  double v = 0.0;
  if (in && d >= dmin && d <= e && lz > -INFINITY) {
    const double* const Trow = T + (e * D + d - 1) * ldk;
    const double* const Urow = lat + (e - d) * K;
    const double* const Brow = lat + 4 * (N + 1) * K + e * K;
    for (int k = j; k < K; k += 16) {
      const double c = ((Urow[k] + scale * Trow[k]) + bonus) + Brow[k];
      if (c > -INFINITY) v += exp(c - lz);
    }
  }
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (in && j == 0) span_post[e * ldp + d - 1] = v > 0.0 ? v : 0.0;
}

__global__ __launch_bounds__(256) void span_fill_value(double* __restrict__ p, long n, double v) {
  const long at = (long)blockIdx.x * 256 + threadIdx.x;
  if (at < n) p[at] = v;
}

static bool span_shape_ok(long N, int D) {
  return D >= 1 && D <= SP_MAX_D && N >= 0 && N < (1L << 31) && (N + 1) * (long)D < (1L << 31);
}

// the per-category table's index limit on top of span_shape_ok
static bool span_table_ok(long N, int D, long ldk) {
  return span_shape_ok(N, D) && ldk >= 1 && ldk < (1L << 31) && (N + 1) * (long)D * ldk < (1L << 31);
}

}  // namespace abcd

using namespace abcd;

extern "C" size_t abcd_span_scores_workspace_bytes(long N, int D, int P) {
  if (!span_shape_ok(N, D) || P < 1) return 0;
  return (size_t)D * (size_t)P * sizeof(double) + 256;  // O[p, d]
}

// What the three passes over the frames share, after an entry point's own requires (every failed require returns
// ABCD_EINVAL, so their order is not seen): the requires on the frames, the prototypes and the workspace, the rows
// e < D of each output that is there (`out`: span_lse or the table, by MODE), span_prefix and span_nll<MODE>.
template <int MODE>
static int span_pass(const float* x, long ld_x, long N, int F, int P, int D, int T_proto, const float* proto_mu,
                     long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                     const float* log_weight, double* out, long ld_k, double* span_score, int32_t* span_cat,
                     long ld_span, void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(P >= 1 && F >= 1 && T_proto >= D && ld_x >= F && ld_mu >= F && ld_lv >= F);
  ABCD_REQUIRE(N == 0 || (x && proto_mu && proto_lv && proto_offset_logits));
  const size_t need = abcd_span_scores_workspace_bytes(N, D, P);  // 0: span_shape_ok fails
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  const long rows = std::min(N, (long)D - 1) + 1;
  const bool best = span_score && span_cat;
  if (MODE == SPAN_TABLE && out) {
    span_table_fill<<<cdiv(rows * D * P, 256), 256, 0, s>>>(rows, D, P, out, ld_k);
    ABCD_CHECK_LAUNCH();
  }
  if (best || (MODE == SPAN_LSE && out)) {  // neither: N = 0 with nowhere to write row 0
    span_fill<<<cdiv(rows * D, 256), 256, 0, s>>>(rows, D, span_score, span_cat, MODE == SPAN_LSE ? out : nullptr,
                                                  ld_span);
    ABCD_CHECK_LAUNCH();
  }
  if (N == 0) return 0;
  double* Otab = (double*)ws;
  span_prefix<<<cdiv(P, 256), 256, 0, s>>>(proto_offset_logits, P, D, Otab);
  // the table alone: the prototype tiles are independent and run side by side
  const dim3 grid((unsigned)cdiv(N, EM_TR), MODE == SPAN_TABLE && !best ? (unsigned)cdiv(P, EM_TP) : 1u);
  span_nll<MODE><<<grid, 256, 0, s>>>(x, ld_x, N, F, P, D, proto_mu, ld_mu, proto_lv, ld_lv, Otab,
                                                log_weight, span_score, span_cat, out, ld_span, ld_k);
  ABCD_CHECK_LAUNCH();
  return 0;
}

// hipFuncAttributeMaxDynamicSharedMemorySize of KERNEL, raised once
template <auto KERNEL>
static hipError_t raise_lds(size_t bytes) {
  static bool done = false;
  if (done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  done = e == hipSuccess;
  return e;
}

// one workgroup of span_chain's width with `lds` bytes: `resident` up to K = SC_RES_K, `streamed` above
template <class... P, class... A>
static void chain_launch(void (*resident)(P...), void (*streamed)(P...), int K, size_t lds, hipStream_t s, A... args) {
  (K <= SC_RES_K ? resident : streamed)<<<1, 64 * span_chain_waves(K), lds, s>>>(args...);
}

extern "C" int abcd_span_scores(const float* x, long ld_x, long N, int F, int P, int D, int T_proto,
                                const float* proto_mu, long ld_mu, const float* proto_lv, long ld_lv,
                                const float* proto_offset_logits, const float* log_weight, double* span_score,
                                int32_t* span_cat, long ld_span, void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(ld_span >= D && (N == 0 || (span_score && span_cat)));
  return span_pass<SPAN_MAX>(x, ld_x, N, F, P, D, T_proto, proto_mu, ld_mu, proto_lv, ld_lv, proto_offset_logits,
                             log_weight, nullptr, 0, span_score, span_cat, ld_span, ws, ws_bytes, stream);
}

extern "C" size_t abcd_span_evidence_workspace_bytes(long N, int D, int P) {
  return abcd_span_scores_workspace_bytes(N, D, P);
}

extern "C" int abcd_span_evidence(const float* x, long ld_x, long N, int F, int P, int D, int T_proto,
                                  const float* proto_mu, long ld_mu, const float* proto_lv, long ld_lv,
                                  const float* proto_offset_logits, const float* log_weight, double* span_lse,
                                  double* span_score, int32_t* span_cat, long ld_span, void* ws, size_t ws_bytes,
                                  void* stream) {
  ABCD_REQUIRE(ld_span >= D && (N == 0 || span_lse));
  ABCD_REQUIRE(!span_score == !span_cat);  // the best outputs come together or not at all
  return span_pass<SPAN_LSE>(x, ld_x, N, F, P, D, T_proto, proto_mu, ld_mu, proto_lv, ld_lv, proto_offset_logits,
                             log_weight, span_lse, 0, span_score, span_cat, ld_span, ws, ws_bytes, stream);
}

extern "C" size_t abcd_span_viterbi_workspace_bytes(long N, int D) {
  if (!span_shape_ok(N, D)) return 0;
  return ((size_t)N + 1) * sizeof(int32_t) + 256;  // the back-pointers
}

extern "C" int abcd_span_viterbi(const double* span_score, const int32_t* span_cat, long ld_span, long N, int D,
                                 int d_min, const float* gap, double seg_bonus, double* path_score,
                                 int32_t* n_segments, int32_t* seg_onset, int32_t* seg_length, int32_t* seg_cat,
                                 double* seg_score, double* V_out, void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(span_shape_ok(N, D) && d_min >= 1 && d_min <= D && ld_span >= D);
  ABCD_REQUIRE(N == 0 || (span_score && span_cat && path_score && n_segments && seg_onset && seg_length && seg_cat &&
                          seg_score));
  const size_t need = abcd_span_viterbi_workspace_bytes(N, D);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {  // the empty path: score 0, no segments, nothing is read
    if (path_score) ABCD_TRY(hipMemsetAsync(path_score, 0, sizeof(double), s));
    if (n_segments) ABCD_TRY(hipMemsetAsync(n_segments, 0, sizeof(int32_t), s));
    if (V_out) ABCD_TRY(hipMemsetAsync(V_out, 0, sizeof(double), s));
    return 0;
  }
  ABCD_TRY(raise_lds<span_viterbi>((SP_MAX_D + 1) * sizeof(double)));
  span_viterbi<<<1, D <= SV_ONE_WAVE_D ? 64 : SV_THREADS, (size_t)D * sizeof(double), s>>>(
      span_score, span_cat, ld_span, N, D, d_min, gap, seg_bonus, path_score, n_segments, seg_onset, seg_length,
      seg_cat, seg_score, V_out, (int32_t*)ws);
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t abcd_span_posterior_workspace_bytes(long N, int D) {
  if (!span_shape_ok(N, D)) return 0;
  return 4 * ((size_t)N + 1) * sizeof(double) + 256;  // the lattice when the caller keeps none
}

extern "C" int abcd_span_posterior(const double* span, long ld_span, long N, int D, int d_min, const float* gap,
                                   double seg_bonus, double* log_z, double* lattice, double* post, double* span_post,
                                   long ld_post, void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(span_shape_ok(N, D) && d_min >= 1 && d_min <= D && ld_span >= D);
  ABCD_REQUIRE(!span_post || ld_post >= D);
  ABCD_REQUIRE(N == 0 || (span && log_z && post));
  const size_t need = abcd_span_posterior_workspace_bytes(N, D);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  if (!log_z && !lattice && !post && !span_post) return 0;  // N = 0 with nowhere to write
  hipStream_t s = (hipStream_t)stream;
  ABCD_TRY(raise_lds<span_fb<true>>((SP_MAX_D + 1) * sizeof(double)));
  ABCD_TRY(raise_lds<span_fb<false>>((SP_MAX_D + 1) * sizeof(double)));
  double* lat = lattice ? lattice : (double*)ws;
  const int threads = D <= SV_ONE_WAVE_D ? 64 : SV_THREADS;
  const size_t slots = ((size_t)D + 1) * sizeof(double);
  if (D <= SF_PAIR_MAX_D)
    span_fb<true><<<1, threads, 2 * slots, s>>>(span, ld_span, N, D, d_min, gap, seg_bonus, log_z, lat, post);
  else
    span_fb<false><<<1, threads, slots, s>>>(span, ld_span, N, D, d_min, gap, seg_bonus, log_z, lat, post);
  ABCD_CHECK_LAUNCH();
  if (span_post) {
    span_post_table<<<cdiv((N + 1) * D, 256), 256, 0, s>>>(span, ld_span, N, D, d_min, seg_bonus, lat, span_post,
                                                           ld_post);
    ABCD_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" size_t abcd_span_table_workspace_bytes(long N, int D, int P, long ld_k) {
  if (!span_table_ok(N, D, ld_k) || P < 1 || ld_k < P) return 0;
  return abcd_span_scores_workspace_bytes(N, D, P);  // O[p, d]
}

extern "C" int abcd_span_table(const float* x, long ld_x, long N, int F, int P, int D, int T_proto,
                               const float* proto_mu, long ld_mu, const float* proto_lv, long ld_lv,
                               const float* proto_offset_logits, const float* log_weight, double* table, long ld_k,
                               double* span_score, int32_t* span_cat, long ld_span, void* ws, size_t ws_bytes,
                               void* stream) {
  ABCD_REQUIRE(span_table_ok(N, D, ld_k) && ld_k >= P && (N == 0 || table));
  ABCD_REQUIRE(!span_score == !span_cat);  // the best outputs come together or not at all
  ABCD_REQUIRE(!span_score || ld_span >= D);
  return span_pass<SPAN_TABLE>(x, ld_x, N, F, P, D, T_proto, proto_mu, ld_mu, proto_lv, ld_lv, proto_offset_logits,
                               log_weight, table, ld_k, span_score, span_cat, ld_span, ws, ws_bytes, stream);
}

extern "C" int abcd_span_chain_plan(int K, int D, int* resident, int* threads, size_t* lds_bytes) {
  ABCD_REQUIRE(K >= 1 && K <= SC_MAX_K && D >= 1 && D <= SP_MAX_D);
  if (resident) *resident = K <= SC_RES_K;
  if (threads) *threads = 64 * span_chain_waves(K);
  if (lds_bytes) *lds_bytes = span_chain_lds(K);
  return 0;
}

extern "C" size_t abcd_span_chain_workspace_bytes(long N, int D, int K) {
  if (K < 1 || K > SC_MAX_K || !span_table_ok(N, D, K)) return 0;
  // U, then the two back-pointer planes
  return ((size_t)N + 1) * (size_t)K * (sizeof(double) + 2 * sizeof(int32_t)) + 256;
}

extern "C" int abcd_span_chain_viterbi(const double* table, long ld_k, long N, int D, int K, int d_min,
                                       const float* gap, double seg_bonus, const float* log_trans, long ld_trans,
                                       const float* log_init, double* path_score, int32_t* n_segments,
                                       int32_t* seg_onset, int32_t* seg_length, int32_t* seg_cat, double* seg_score,
                                       double* seg_link, double* W_out, void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(K >= 1 && K <= SC_MAX_K && span_table_ok(N, D, ld_k) && d_min >= 1 && d_min <= D);
  ABCD_REQUIRE(ld_k >= K && ld_trans >= K);
  ABCD_REQUIRE(N == 0 || (table && log_trans && log_init && path_score && n_segments && seg_onset && seg_length &&
                          seg_cat && seg_score && seg_link));
  const size_t need = abcd_span_chain_workspace_bytes(N, D, K);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {  // the empty path: score 0, no segments, W[0] = -inf, nothing is read
    if (path_score) ABCD_TRY(hipMemsetAsync(path_score, 0, sizeof(double), s));
    if (n_segments) ABCD_TRY(hipMemsetAsync(n_segments, 0, sizeof(int32_t), s));
    if (W_out) {
      span_table_fill<<<cdiv(K, 256), 256, 0, s>>>(1, 1, K, W_out, K);
      ABCD_CHECK_LAUNCH();
    }
    return 0;
  }
  ABCD_TRY(raise_lds<span_chain<true>>(span_chain_lds(SC_RES_K)));
  ABCD_TRY(raise_lds<span_chain<false>>(std::max(span_chain_lds(SC_WIDE_K), span_chain_lds(SC_MAX_K))));
  double* U = (double*)ws;
  int32_t* back_d = (int32_t*)(U + (N + 1) * K);
  int32_t* back_k = back_d + (N + 1) * K;
  chain_launch(span_chain<true>, span_chain<false>, K, span_chain_lds(K), s, table, ld_k, N, D, K, d_min, gap,
               seg_bonus, log_trans, ld_trans, log_init, path_score, n_segments, seg_onset, seg_length, seg_cat,
               seg_score, seg_link, W_out, U, back_d, back_k);
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t abcd_span_chain_window_workspace_bytes(long N, int D, int K) {
  if (K < 1 || K > SC_MAX_K || !span_shape_ok(N, D)) return 0;
  // U and sel, the two back-pointer planes, then the carry block (W[n], G, next_n)
  return ((size_t)N + 1) * (size_t)K * (2 * sizeof(double) + 2 * sizeof(int32_t)) + ((size_t)K + 2) * sizeof(double) +
         256;
}

extern "C" int abcd_span_chain_viterbi_window(const double* table, long ld_k, long row0, long rows, long n0, long n1,
                                              long N, int D, int K, int d_min, const float* gap, double seg_bonus,
                                              const float* log_trans, long ld_trans, const float* log_init,
                                              double* path_score, int32_t* n_segments, int32_t* seg_onset,
                                              int32_t* seg_length, int32_t* seg_cat, double* seg_score,
                                              double* seg_link, double* W_out, void* ws, size_t ws_bytes,
                                              void* stream) {
  ABCD_REQUIRE(K >= 1 && K <= SC_MAX_K && span_shape_ok(N, D) && d_min >= 1 && d_min <= D);
  ABCD_REQUIRE(1 <= n0 && n0 <= n1 && n1 <= N);
  ABCD_REQUIRE(row0 >= 0 && row0 <= std::max(0L, n0 - D) && rows >= 1 && n1 - row0 < rows);
  ABCD_REQUIRE(ld_k >= K && ld_k < (1L << 31) && ld_trans >= K);
  ABCD_REQUIRE(rows < (1L << 31) && rows * (long)D < (1L << 31) && rows * (long)D * ld_k < (1L << 31));
  ABCD_REQUIRE(table && log_trans && log_init && path_score && n_segments && seg_onset && seg_length && seg_cat &&
               seg_score && seg_link);
  const size_t need = abcd_span_chain_window_workspace_bytes(N, D, K);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  ABCD_TRY(raise_lds<span_chain_win<true>>(span_chain_lds(SC_RES_K)));
  ABCD_TRY(raise_lds<span_chain_win<false>>(std::max(span_chain_lds(SC_WIDE_K), span_chain_lds(SC_MAX_K))));
  const long cells = (N + 1) * K;
  double* U = (double*)ws;
  double* sel = U + cells;
  int32_t* back_d = (int32_t*)(sel + cells);
  int32_t* back_k = back_d + cells;
  double* carry = (double*)(back_k + cells);  // 16 cells bytes in: 8-byte aligned
  chain_launch(span_chain_win<true>, span_chain_win<false>, K, span_chain_lds(K), s, table, ld_k, row0, n0, n1, N, D, K,
               d_min, gap, seg_bonus, log_trans, ld_trans, log_init, path_score, n_segments, seg_onset, seg_length,
               seg_cat, seg_score, seg_link, W_out, U, back_d, back_k, sel, carry);
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" int abcd_span_chain_posterior_plan(int K, int D, int* resident, int* threads, size_t* lds_bytes) {
  ABCD_REQUIRE(K >= 1 && K <= SC_MAX_K && D >= 1 && D <= SP_MAX_D);
  if (resident) *resident = K <= SC_RES_K;
  if (threads) *threads = 64 * span_chain_waves(K);
  if (lds_bytes) *lds_bytes = span_chain_fb_lds(K);
  return 0;
}

extern "C" size_t abcd_span_chain_posterior_workspace_bytes(long N, int D, int K) {
  if (K < 1 || K > SC_MAX_K || !span_table_ok(N, D, K)) return 0;
  // the five lattice planes and G / bG, for the caller that keeps none
  return ((size_t)N + 1) * (5 * (size_t)K + 2) * sizeof(double) + 256;
}

extern "C" int abcd_span_chain_posterior(const double* table, long ld_k, long N, int D, int K, int d_min,
                                         const float* gap, double seg_bonus, double scale, const float* log_trans,
                                         long ld_trans, const float* log_init, double* log_z, double* lattice,
                                         double* lattice_g, double* post_k, double* gap_post, double* trans_counts,
                                         double* init_counts, double* span_post, long ld_post, void* ws,
                                         size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(K >= 1 && K <= SC_MAX_K && span_table_ok(N, D, ld_k) && d_min >= 1 && d_min <= D);
  ABCD_REQUIRE(scale > 0.0 && scale < INFINITY);  // NaN fails both
  ABCD_REQUIRE(ld_k >= K && ld_trans >= K);
  ABCD_REQUIRE(!span_post || ld_post >= D);
  ABCD_REQUIRE(!trans_counts == !init_counts);  // the counts come together or not at all
  ABCD_REQUIRE(N == 0 || (table && log_trans && log_init && log_z && post_k && gap_post));
  const size_t need = abcd_span_chain_posterior_workspace_bytes(N, D, K);
  ABCD_REQUIRE(need && ws && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {  // the empty cover: log_z = 0, bW[0] = G[0] = bG[0] = 0, the other planes -inf, zeros; nothing is read
    if (log_z) ABCD_TRY(hipMemsetAsync(log_z, 0, sizeof(double), s));
    if (lattice) {
      span_fill_value<<<cdiv(4 * K, 256), 256, 0, s>>>(lattice, 4 * K, -INFINITY);
      ABCD_CHECK_LAUNCH();
      ABCD_TRY(hipMemsetAsync(lattice + 4 * K, 0, K * sizeof(double), s));
    }
    if (lattice_g) ABCD_TRY(hipMemsetAsync(lattice_g, 0, 2 * sizeof(double), s));
    if (post_k) ABCD_TRY(hipMemsetAsync(post_k, 0, 2 * K * sizeof(double), s));
    if (gap_post) ABCD_TRY(hipMemsetAsync(gap_post, 0, sizeof(double), s));
    if (trans_counts) {
      ABCD_TRY(hipMemsetAsync(trans_counts, 0, (size_t)K * K * sizeof(double), s));
      ABCD_TRY(hipMemsetAsync(init_counts, 0, K * sizeof(double), s));
    }
    if (span_post) ABCD_TRY(hipMemsetAsync(span_post, 0, D * sizeof(double), s));
    return 0;
  }
  ABCD_TRY(raise_lds<span_chain_fb<true>>(span_chain_fb_lds(SC_RES_K)));
  ABCD_TRY(raise_lds<span_chain_fb<false>>(std::max(span_chain_fb_lds(SC_WIDE_K), span_chain_fb_lds(SC_MAX_K))));
  double* lat = lattice ? lattice : (double*)ws;
  double* latg = lattice_g ? lattice_g : (double*)ws + 5 * (N + 1) * K;
  const double bonus = seg_bonus * scale;
  chain_launch(span_chain_fb<true>, span_chain_fb<false>, K, span_chain_fb_lds(K), s, table, ld_k, N, D, K, d_min, gap,
               bonus, scale, log_trans, ld_trans, log_init, log_z, lat, latg, post_k, gap_post, trans_counts,
               init_counts);
  ABCD_CHECK_LAUNCH();
  if (span_post) {
    span_chain_post_table<<<cdiv((N + 1) * D, 16), 256, 0, s>>>(table, ld_k, N, D, K, d_min, bonus, scale, lat, log_z,
                                                                span_post, ld_post);
    ABCD_CHECK_LAUNCH();
  }
  return 0;
}
