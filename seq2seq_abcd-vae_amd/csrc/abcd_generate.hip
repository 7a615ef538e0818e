// abcd_generate.hip -- free-running decoder generation with learned stopping.
//
// The decoder's rows are independent: row b's frames depend on row b's
// features, speaker and noise alone.  "Generate until the offset predictor
// fires" is therefore the decoder forward on the full B x T_max rectangle
// (dec_forward_impl as it stands: batch_sizes[t] = B, no ground truth, no
// losses) followed by a cut: every row ends at the first step whose offset
// logit exceeds the threshold, and the survivors are laid out as a
// PackedSequence.  The steps a row runs past its stop are wasted; no kernel of
// the forward changes for it.  The three kernels of the cut live here:
//   gen_stop_scan  one thread per row over the time-major logits -> lengths
//   gen_order      one workgroup: LDS length histogram -> batch_sizes, step
//                  offsets, total, and the stable descending rank -> order
//   gen_gather     padded rectangle rows (t, order[j]) -> packed rows off[t] + j
#include <vector>

#include "abcd_common.h"
#include "abcd_internal.h"

namespace abcd {

// abcd_timing_read_kernel ids of the three launches (timing only: they keep no
// dispatch record)
enum { TK_GEN_SCAN = 8, TK_GEN_ORDER = 9, TK_GEN_GATHER = 10 };

// offlog[t * B + b]: adjacent threads read adjacent rows of one step (coalesced).
__global__ __launch_bounds__(256) void gen_stop_scan(const float* __restrict__ offlog, int B, int T, float stop,
                                                     int min_len, int32_t* __restrict__ lengths) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int len = T;
  for (int t = 0; t < T; ++t)
    if (offlog[(long)t * B + b] > stop) {  // false for NaN
      len = t + 1;
      break;
    }
  lengths[b] = max(len, min_len);  // min_len <= T (checked by the caller)
}

// One workgroup.  cnt[l] starts as the number of rows of length l (LDS integer
// adds: the counts do not depend on their order) and becomes, in place, the
// number of rows longer than l -- batch_sizes[l], and the rank of the first row
// of length l.  A row's rank adds the rows of its own length before it in
// input order, counted by a plain loop, so equal lengths keep their order.
__global__ __launch_bounds__(256) void gen_order(const int32_t* __restrict__ lengths, int B, int T,
                                                 int64_t* __restrict__ order, int64_t* __restrict__ batch_sizes,
                                                 int* __restrict__ goff, int64_t* __restrict__ total) {
  __shared__ int cnt[ABCD_GEN_MAX_T + 1];
  for (int l = threadIdx.x; l <= T; l += 256) cnt[l] = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) atomicAdd(&cnt[lengths[b]], 1);  // 1 <= lengths[b] <= T
  __syncthreads();
  if (threadIdx.x == 0) {
    int longer = 0;
    for (int l = T; l >= 0; --l) {
      const int here = cnt[l];
      cnt[l] = longer;
      longer += here;
    }
    int off = 0;
    for (int t = 0; t < T; ++t) {
      batch_sizes[t] = cnt[t];
      goff[t] = off;
      off += cnt[t];
    }
    goff[T] = off;
    total[0] = off;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) {
    const int len = lengths[b];
    int r = cnt[len];
    for (int k = 0; k < b; ++k) r += lengths[k] == len;
    order[r] = b;
  }
}

// grid (T, ceil(B / 4)): one wave per packed row; the lanes walk the row's F
// floats, so loads (stride Fp) and stores (stride F) are contiguous per row.
__global__ __launch_bounds__(256) void gen_gather(const float* __restrict__ OUT, const float* __restrict__ MU,
                                                  const float* __restrict__ LV, const float* __restrict__ offlog,
                                                  int B, int F, int Fp, const int64_t* __restrict__ order,
                                                  const int64_t* __restrict__ batch_sizes,
                                                  const int* __restrict__ goff, float* __restrict__ out,
                                                  float* __restrict__ mu, float* __restrict__ lv,
                                                  float* __restrict__ logits) {
  const int t = blockIdx.x, lane = threadIdx.x & 63;
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= (int)batch_sizes[t]) return;
  const long src = (long)t * B + order[j], dst = (long)goff[t] + j;
  for (int c = lane; c < F; c += 64) {
    if (out) out[dst * F + c] = OUT[src * Fp + c];
    if (mu) mu[dst * F + c] = MU[src * Fp + c];
    if (lv) lv[dst * F + c] = LV[src * Fp + c];
  }
  if (logits && lane == 0) logits[dst] = offlog[src];
}

struct GenWS {
  void* dec;  // the decoder forward's own workspace (carve_decoder)
  size_t dec_bytes;
  int* goff;  // T_max + 1 step offsets of the packed result
};

static GenWS carve_generate(Arena& A, const abcd_decoder_cfg* c, int T, int B) {
  GenWS g{};
  g.dec_bytes = abcd_decoder_workspace_bytes(c, T, T * B, B);
  g.dec = A.f(g.dec_bytes / 4 + 1);
  g.goff = (int*)A.f((size_t)T + 1);
  return g;
}

static bool gen_shape_ok(const abcd_decoder_cfg* c, int T, int B) {
  return c && T >= 1 && T <= ABCD_GEN_MAX_T && B >= 1 && B <= ABCD_GEN_MAX_B && (long)T * B <= 0x7fffffffL &&
         abcd_decoder_workspace_bytes(c, T, T * B, B) != 0;
}

}  // namespace abcd

using namespace abcd;

extern "C" size_t abcd_decoder_generate_workspace_bytes(const abcd_decoder_cfg* c, int T_max, int B) {
  if (!gen_shape_ok(c, T_max, B)) return 0;
  Arena A(nullptr, 0);
  carve_generate(A, c, T_max, B);
  return A.off + 256;
}

extern "C" int abcd_decoder_generate(const abcd_decoder_cfg* c, const abcd_decoder_params* p, const float* features,
                                     const int64_t* speakers, int B, int T_max, int mode, const float* eps,
                                     uint64_t seed, uint64_t offset, float stop_logit, int min_len, float* out,
                                     float* mu, float* log_var, float* offset_logits, int32_t* lengths,
                                     int64_t* order, int64_t* batch_sizes, int64_t* total, void* ws,
                                     size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(gen_shape_ok(c, T_max, B) && c->feedback == 1);
  ABCD_REQUIRE(mode == ABCD_GEN_MEAN || mode == ABCD_GEN_SAMPLE);
  ABCD_REQUIRE(min_len <= T_max);
  ABCD_REQUIRE(p && features && lengths && order && batch_sizes && total && ws);
  hipStream_t s = (hipStream_t)stream;
  Arena A(ws, ws_bytes);
  GenWS g = carve_generate(A, c, T_max, B);
  ABCD_REQUIRE(A.ok);
  const int L = T_max * B, F = c->output_size, Fp = rup16(F);
  Arena D(g.dec, g.dec_bytes);
  const DecWS w = carve_decoder(D, c, T_max, L, B);
  ABCD_REQUIRE(D.ok);
  if (mode == ABCD_GEN_MEAN) {  // the mean, emitted and fed back: the sample at eps = 0
    ABCD_TRY(hipMemsetAsync(w.EPS, 0, (size_t)L * F * sizeof(float), s));
    eps = w.EPS;
  }
  // ---- the forward on the rectangle: every step has all B rows ----
  const std::vector<int64_t> bs((size_t)T_max, (int64_t)B);
  abcd_packed x{};
  x.data = nullptr; x.batch_sizes = bs.data(); x.T = T_max; x.L = L; x.B = B; x.F = F;
  const int rc = dec_forward_impl(c, p, &x, features, speakers, nullptr, eps, nullptr, seed, offset, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, g.dec, g.dec_bytes, stream, s);
  if (rc) return rc;
  // ---- the cut ----
  {
    TimedScope ts(s, TK_GEN_SCAN);
    gen_stop_scan<<<cdiv(B, 256), 256, 0, s>>>(w.offlog, B, T_max, stop_logit, min_len, lengths);
  }
  ABCD_CHECK_LAUNCH();
  {
    TimedScope ts(s, TK_GEN_ORDER);
    gen_order<<<1, 256, 0, s>>>(lengths, B, T_max, order, batch_sizes, g.goff, total);
  }
  ABCD_CHECK_LAUNCH();
  if (out || mu || log_var || offset_logits) {
    TimedScope ts(s, TK_GEN_GATHER);
    gen_gather<<<dim3(T_max, cdiv(B, 4)), 256, 0, s>>>(w.OUT, w.MU, w.LV, w.offlog, B, F, Fp, order, batch_sizes,
                                                       g.goff, out, mu, log_var, offset_logits);
  }
  ABCD_CHECK_LAUNCH();
  return 0;
}
