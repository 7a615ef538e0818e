// abcd_score.hip -- per-segment ELBO terms: what the scalar losses of
// abcd_decoder_forward (emission NLL, offset BCE) and abcd_sampler_kl are
// before they are summed over the batch.
//
//   seg_losses   one workgroup per segment over the packed layout: segment b
//                owns packed rows off[t] + b for every t with batch_sizes[t] > b
//   kl_rows_seg  one wave per row: sum_k q log q - sum_k q elog[k], and the
//                batch-independent Dirichlet bracket (block 0)
//   kl_rows_plain  the plain Gaussian sampler's row terms
//
// The per-term expressions are those of dec_emission_nll / dec_offset_head
// (abcd_rnn.hip) and kl_prior / kl_rows (abcd_sampler.hip): fp32 terms, fp64
// accumulation, one cast per result.  Every sum has a fixed order (lane-strided
// partial sums, a shuffle tree, the waves in index order): no atomics, nothing
// depends on how workgroups are scheduled, and no device-global ticket word is
// touched, so these launches may run beside any other entry point.
#include <vector>

#include "abcd_common.h"
#include "abcd_internal.h"
#include "abcd_persist.h"
#include "abcd_special.h"

namespace abcd {

// Block b = segment b (packed row order).  Its length is the number of steps
// with batch_sizes[t] = off[t + 1] - off[t] > b; batch_sizes is non-increasing,
// so those are the steps t < len.  Wave w of NW takes steps w, w + NW, ...; its
// lanes stride over the F columns of the step's row (coalesced; columns >= F of
// a padded row and rows of other segments are never read).  A segment's rows
// lie batch_sizes[t] rows apart, so the kernel is bound by how many row loads it
// keeps in flight: NW = 16 (two 1024-thread workgroups fill a CU's 32 wave
// slots) measured 28 us against 42 us (NW = 8) and 72 us (NW = 4) at the c2
// shape.
constexpr int SEG_WAVES = 16;
template <int NW>
__global__ __launch_bounds__(64 * NW) void seg_losses(const float* __restrict__ Y, const float* __restrict__ MU,
                                                      long ldm, const float* __restrict__ LV, long ldl,
                                                      const float* __restrict__ X, const float* __restrict__ TGT,
                                                      const int* __restrict__ off, int T, int F,
                                                      float* __restrict__ seg_em, float* __restrict__ seg_off,
                                                      int32_t* __restrict__ seg_len) {
  __shared__ int shn[NW];
  __shared__ double she[NW], sho[NW];
  const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int n = 0;  // integer count: order-free
  for (int t = threadIdx.x; t < T; t += 64 * NW) n += off[t + 1] - off[t] > b;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
  if (lane == 0) shn[w] = n;
  __syncthreads();
  int len = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) len += shn[k];
  double em = 0.0, bce = 0.0;
  if (seg_em) {
#pragma unroll 2
    for (int t = w; t < len; t += NW) {
      const long r = (long)off[t] + b;
      const float* y = Y + r * F;
      const float* mu = MU + r * ldm;
      const float* lv = LV + r * ldl;
#pragma unroll 3
      for (int j = lane; j < F; j += 64) {
        const float m = mu[j], l = lv[j], d = y[j] - m;
        em += 0.5f * (1.8378770664093453f + l + d * d * __expf(-l));
      }
    }
  }
  if (seg_off) {  // one term per step: lane-strided over the segment's steps
    for (int t = threadIdx.x; t < len; t += 64 * NW) {
      const long r = (long)off[t] + b;
      const float x = X[r], y = TGT[r];
      bce += fmaxf(x, 0.f) - x * y + log1pf(__expf(-fabsf(x)));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    em += __shfl_down(em, o, 64);
    bce += __shfl_down(bce, o, 64);
  }
  if (lane == 0) {
    she[w] = em;
    sho[w] = bce;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // the waves' sums in wave order
    double e = she[0], o = sho[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) {
      e += she[k];
      o += sho[k];
    }
    if (seg_em) seg_em[b] = (float)e;
    if (seg_off) seg_off[b] = (float)o;
    if (seg_len) seg_len[b] = len;
  }
}

// ABCDSampler.kl_divergence (model.py:608-639) per row.  Every workgroup forms
// the prior's alpha / elog in LDS with kl_prior's arithmetic (prior_block of
// abcd_sampler.hip: softmax in fp64, the product p N in fp32, alpha and elog
// rounded to fp32) -- K digammas, cheaper than a second launch and a global
// stash -- then its 4 waves take one row each with kl_rows' arithmetic.  Block
// 0 also writes the bracket Eq log q(pi) - Eq log p(pi).  Only the first Kv of
// a row's K columns are categories.
__global__ __launch_bounds__(256) void kl_rows_seg(const float* __restrict__ logits, int B, int K, int Kv,
                                                   const float* __restrict__ psl, double N, float a0,
                                                   float* __restrict__ rows, float* __restrict__ prior) {
  extern __shared__ float lds[];  // alpha [Kv] | elog [Kv]
  __shared__ double sh[16];
  float* alphaL = lds;
  float* elogL = lds + Kv;
  const int tid = threadIdx.x, nt = blockDim.x;
  double m = -1e300;
  for (int k = tid; k < Kv; k += nt) m = fmax(m, (double)psl[k]);
  m = block_max_dd(m, sh);
  double se = 0.0;
  for (int k = tid; k < Kv; k += nt) se += exp((double)psl[k] - m);
  se = block_sum_dd(se, sh);
  double sa = 0.0;
  for (int k = tid; k < Kv; k += nt) {
    const double p = exp((double)psl[k] - m) / se;
    const double al = (double)(float)((float)p * (float)N) + (double)a0;  // the product in fp32 like the reference
    alphaL[k] = (float)al;
    sa += al;
  }
  sa = block_sum_dd(sa, sh);
  const double S = sa, psiS = digamma_d(S);
  const bool first = blockIdx.x == 0;  // uniform per workgroup
  double acc = 0.0;  // -sum lgamma(alpha) + sum (alpha-1) elog - (a0-1) sum elog
  for (int k = tid; k < Kv; k += nt) {
    const double al = alphaL[k];
    const double el = digamma_d(al) - psiS;
    elogL[k] = (float)el;
    if (first) acc += -lgamma(al) + (al - 1.0) * el - ((double)a0 - 1.0) * el;
  }
  if (first) {
    acc = block_sum_dd(acc, sh);
    if (tid == 0) {
      const double a0d = a0;
      prior[0] = (float)(lgamma(S) + acc - (lgamma(a0d * Kv) - Kv * lgamma(a0d)));
    }
  }
  __syncthreads();
  const int lane = tid & 63;
  const int b = blockIdx.x * 4 + (tid >> 6);
  if (b >= B) return;
  const float* l = logits + (long)b * K;
  float mx = -INFINITY;
  for (int k = lane; k < Kv; k += 64) mx = fmaxf(mx, l[k]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int k = lane; k < Kv; k += 64) s += __expf(l[k] - mx);
  s = wave_sum(s);
  const float ls = __logf(s);
  float v = 0.f;
  for (int k = lane; k < Kv; k += 64) {
    const float lq = l[k] - mx - ls;
    v += __expf(lq) * (lq - elogL[k]);
  }
  v = wave_sum(v);
  if (lane == 0) rows[b] = v;
}

// plain Sampler: rows[b] = -0.5 sum_f (1 + lv - mu^2 - e^lv) of MV = [mean | log_var]
// (plain_kl's fp64 terms); a padding column (mean = log_var = 0) adds 0
__global__ __launch_bounds__(256) void kl_rows_plain(const float* __restrict__ MV, int B, int f,
                                                     float* __restrict__ rows, float* __restrict__ prior) {
  if (blockIdx.x == 0 && threadIdx.x == 0) prior[0] = 0.f;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* mv = MV + (long)b * 2 * f;
  double acc = 0.0;
  for (int j = lane; j < f; j += 64) {
    const float mu = mv[j], lv = mv[f + j];
    acc += 1.0 + lv - (double)mu * mu - exp((double)lv);
  }
  acc = wave_sum_d(acc);
  if (lane == 0) rows[b] = (float)(-0.5 * acc);
}

constexpr int SEG_MAX_T = 16383;    // T + 1 ints fit one slot of the pinned offset ring
constexpr int KL_ROWS_MAX_K = 8192; // alpha | elog in 64 KiB of LDS

}  // namespace abcd

using namespace abcd;

extern "C" size_t abcd_segment_losses_workspace_bytes(int T, int B) {
  if (T < 1 || T > SEG_MAX_T || B < 1) return 0;
  return ((size_t)T + 1) * sizeof(int) + 256;
}

extern "C" int abcd_segment_losses(const abcd_packed* x, const float* mu, long ld_mu, const float* log_var,
                                   long ld_lv, const float* offset_logits, const float* gt_offset, float* seg_em,
                                   float* seg_off, int32_t* seg_len, void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(x && x->F >= 1 && x->T <= SEG_MAX_T);
  ABCD_REQUIRE(validate_batch(x->batch_sizes, x->T, x->L, x->B) == 0);
  ABCD_REQUIRE((mu == nullptr || ld_mu >= x->F) && (log_var == nullptr || ld_lv >= x->F));
  ABCD_REQUIRE((offset_logits == nullptr) == (gt_offset == nullptr));
  ABCD_REQUIRE(!seg_em || (x->data && mu && log_var));
  ABCD_REQUIRE(!seg_off || offset_logits);
  ABCD_REQUIRE(ws && ws_bytes >= abcd_segment_losses_workspace_bytes(x->T, x->B));
  if (!seg_em && !seg_off && !seg_len) return 0;
  hipStream_t s = (hipStream_t)stream;
  const std::vector<int> off = step_offsets(x->batch_sizes, x->T);
  int* doff = (int*)ws;
  ABCD_TRY((hipError_t)upload_offsets(s, off, doff));  // pinned ring + async copy: no host synchronisation
  note_dispatch(TK_SEG_LOSSES, "seg_losses<%d> grid %d", 64 * SEG_WAVES, x->B);
  {
    TimedScope ts(s, TK_SEG_LOSSES);
    seg_losses<SEG_WAVES><<<x->B, 64 * SEG_WAVES, 0, s>>>(x->data, mu, ld_mu, log_var, ld_lv, offset_logits,
                                                          gt_offset, doff, x->T, x->F, seg_em, seg_off, seg_len);
  }
  ABCD_CHECK_LAUNCH();
  return 0;
}

extern "C" int abcd_sampler_kl_rows(const abcd_sampler_cfg* c, const abcd_sampler_params* p, const float* logits,
                                    int B, double N, float* rows, float* prior, void* ws, size_t ws_bytes,
                                    void* stream) {
  (void)ws;
  (void)ws_bytes;
  ABCD_REQUIRE(c && p && logits && rows && prior && B > 0);
  hipStream_t s = (hipStream_t)stream;
  if (c->plain) {
    const int f = c->feature_dim;
    ABCD_REQUIRE(f > 0);
    note_dispatch(TK_KL_ROWS, "kl_rows_plain<%d> grid %d", f, cdiv(B, 4));
    {
      TimedScope ts(s, TK_KL_ROWS);
      kl_rows_plain<<<cdiv(B, 4), 256, 0, s>>>(logits, B, f, rows, prior);
    }
    ABCD_CHECK_LAUNCH();
    return 0;
  }
  const int K = c->num_categories;
  ABCD_REQUIRE(K > 0 && K <= KL_ROWS_MAX_K && c->valid_categories >= 0 && c->valid_categories <= K);
  ABCD_REQUIRE(p->posterior_shape_logits && N > 0);
  const int Kv = c->valid_categories ? c->valid_categories : K;
  note_dispatch(TK_KL_ROWS, "kl_rows_seg<%d,%d> grid %d", K, Kv, cdiv(B, 4));
  {
    TimedScope ts(s, TK_KL_ROWS);
    kl_rows_seg<<<cdiv(B, 4), 256, (size_t)2 * Kv * sizeof(float), s>>>(logits, B, K, Kv, p->posterior_shape_logits, N,
                                                                       p->prior_concentration, rows, prior);
  }
  ABCD_CHECK_LAUNCH();
  return 0;
}
