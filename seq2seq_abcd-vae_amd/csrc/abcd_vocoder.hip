// abcd_vocoder.hip -- log-spectra back to audio: Griffin-Lim on the device.
//
// The inverse of abcd_feat.hip.  A segment's packed log-amplitude frames give
// the magnitudes A = max(exp(x norm) - eps, 0); with an initial phase the loop
//
//   C = A exp(i phase0);  R_prev = 0
//   n_iter times:  y = istft(C);  R = stft(y);  t = R - alpha R_prev;  R_prev = R;
//                  C = A t / (|t| + 1e-16)             (alpha = momentum / (1 + momentum))
//   wave = istft(C);  residual = || |stft(wave)| - A ||_F / ||A||_F
//
// runs in ONE launch, one 1024-thread workgroup per segment, with nothing but
// __syncthreads() between its phases.  The reflect-padded
// signal (S + n_fft floats) stays in LDS for the whole loop beside the window
// and the twiddle table wherever that fits in 160 KiB, else in the caller's
// workspace (the same kernel, griffin_lim<false>); the scaled phasors C and
// R_prev (T x F complex per segment) live in the workspace, which L2 holds.
//
//   istft  a gather per output sample: a thread owns GL_KT residues s0 of the
//          sample index mod hop and GL_MT consecutive hop-sized chunks m, so
//          sample (m, s0) takes frame m - r at local index k = s0 + r hop: the
//          twiddle of (f, k) serves all GL_MT chunks and a phasor of (frame, f)
//          all GL_KT residues.  Frames in descending order, bins ascending: a
//          fixed order, no atomics.
//   stft   a thread owns one bin f and GL_TT consecutive frames: the twiddle
//          of (f, k) serves all of them, the samples are LDS broadcasts.
//
// Both are direct fp32 DFTs with a twiddle table built in double (angle index
// (f k) mod n_fft kept incrementally: any n_fft, odd included).
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "abcd_common.h"
#include "abcd_internal.h"
#include "abcd_persist.h"
#include "abcd_special.h"

namespace abcd {

constexpr int GL_THREADS = 1024;
constexpr int GL_KT = 2;   // istft: sample residues (mod hop) per thread
constexpr int GL_MT = 4;   // istft: hop-sized chunks per thread
constexpr int GL_TT = 8;   // stft: frames per thread
constexpr int GL_MAX_T = 16383;            // T + 1 ints fit one slot of the pinned offset ring
constexpr size_t GL_LDS_MAX = 160 * 1024;  // one workgroup may hold the whole CU's LDS
constexpr size_t GL_LDS_FIXED = 256;       // the residual's wave partials (32 doubles)

struct GlArgs {
  const float* x;        // packed log-amplitudes, row stride ld
  const float* ph;       // initial phase, row stride ldp
  const int* off;        // device: packed step offsets off[0..T]
  const float* window;   // n
  const float* tw;       // device: cos(2 pi j / n), sin(2 pi j / n), j < n (2n floats, rounded from double)
  float2* C;             // [B][T * F] scaled phasors
  float2* Rp;            // [B][T * F] R_prev
  float* sig;            // global form: [B][sig_ld] reflect-padded signals; LDS form: unused
  float* wave;           // B x ldw
  float* residual;       // B, or null
  long sig_ld;
  int ld, ldp, ldw, T, n, hop, F, n_iter, smax;
  float eps, norm, alpha;
};

template <bool LDS>
__global__ __launch_bounds__(GL_THREADS) void griffin_lim(GlArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gsm[];
  const int n = a.n, hop = a.hop, F = a.F, tid = threadIdx.x, b = blockIdx.x;
  const int nthr = blockDim.x;  // 1024, or what ABCD_GL_WAVES asks for
  const int Tb = steps_longer(a.off, a.T, b);  // this segment's frames
  const int pad = n / 2, rpad = n - pad;
  const int S = hop * (Tb - 1);
  float* wrow = a.wave + (long)b * a.ldw;
  if (S <= rpad) {  // too short for the reflect padding (uniform: before any barrier)
    for (int i = tid; i < a.smax; i += nthr) wrow[i] = 0.f;
    if (tid == 0 && a.residual) a.residual[b] = __builtin_nanf("");
    return;
  }
  const int Pn = S + n;  // the padded signal: pad in front, S samples, rpad behind
  double* red = reinterpret_cast<double*>(gsm);        // [32]
  float* cs = gsm + GL_LDS_FIXED / sizeof(float);      // [n]
  float* sn = cs + n;                                  // [n]
  float* w = sn + n;                                   // [n]
  float* xp;
  if constexpr (LDS) xp = w + n; else xp = a.sig + (long)b * a.sig_ld;
  float2* C = a.C + (long)b * a.T * F;
  float2* Rp = a.Rp + (long)b * a.T * F;
  const float inv_n = 1.0f / (float)n;

  for (int j = tid; j < n; j += nthr) {
    cs[j] = a.tw[j];
    sn[j] = a.tw[n + j];
    w[j] = a.window[j];
  }
  auto magnitude = [&](int t, int f) {
    const long row = (long)a.off[t] + b;
    return fmaxf(expf(a.x[row * a.ld + f] * a.norm) - a.eps, 0.f);
  };
  for (int e = tid; e < Tb * F; e += nthr) {
    const int t = e / F, f = e - t * F;
    const float A = magnitude(t, f);
    float sp, cp;
    sincosf(a.ph[((long)a.off[t] + b) * a.ldp + f], &sp, &cp);
    C[e] = make_float2(A * cp, A * sp);
    Rp[e] = make_float2(0.f, 0.f);
  }
  __syncthreads();

  // y = istft(C) into the S real samples of xp
  const int HQ = (hop + GL_KT - 1) / GL_KT;              // residues per thread are u, u + HQ, ...
  const int nchunk = (Pn + hop - 1) / hop;
  const int nmt = (nchunk + GL_MT - 1) / GL_MT;
  const int nyq = (n & 1) ? -1 : n / 2;
  auto istft = [&]() {
    for (int e = tid; e < nmt * HQ; e += nthr) {
      const int mt = e / HQ, u = e - mt * HQ, m0 = mt * GL_MT;
      // chunks m0 .. m0 + MT - 1 hold samples [m0 hop, (m0 + MT) hop): any real one?
      if ((m0 + GL_MT) * hop <= pad || m0 * hop >= pad + S) continue;
      float acc[GL_KT][GL_MT], env[GL_KT][GL_MT];
#pragma unroll
      for (int q = 0; q < GL_KT; ++q)
#pragma unroll
        for (int j = 0; j < GL_MT; ++j) acc[q][j] = env[q][j] = 0.f;
      for (int r = 0; r * hop < n; ++r) {
        int k[GL_KT], jd[GL_KT];
        float wk[GL_KT];
        bool any = false;
#pragma unroll
        for (int q = 0; q < GL_KT; ++q) {
          const int s0 = u + q * HQ;
          k[q] = s0 + r * hop;
          const bool ok = s0 < hop && k[q] < n;
          wk[q] = ok ? w[k[q]] : 0.f;
          if (!ok) k[q] = 0;
          jd[q] = 0;
          any |= ok;
        }
        if (!any) continue;
        int tf[GL_MT];  // frame of chunk j at this r, clamped; fv: does it exist
        float fv[GL_MT];
#pragma unroll
        for (int j = 0; j < GL_MT; ++j) {
          const int t = m0 + j - r;
          fv[j] = (t >= 0 && t < Tb) ? 1.f : 0.f;
          tf[j] = min(max(t, 0), Tb - 1) * F;
        }
        float s[GL_KT][GL_MT];
#pragma unroll
        for (int q = 0; q < GL_KT; ++q)
#pragma unroll
          for (int j = 0; j < GL_MT; ++j) s[q][j] = 0.f;
        for (int f = 0; f < F; ++f) {
          const float cf = (f == 0 || f == nyq) ? 1.f : 2.f;  // the one-sided spectrum's weights
          float2 c[GL_MT];
#pragma unroll
          for (int j = 0; j < GL_MT; ++j) c[j] = C[tf[j] + f];
#pragma unroll
          for (int q = 0; q < GL_KT; ++q) {
            const float cc = cf * cs[jd[q]], ss = cf * sn[jd[q]];
#pragma unroll
            for (int j = 0; j < GL_MT; ++j) s[q][j] = fmaf(c[j].x, cc, fmaf(-c[j].y, ss, s[q][j]));
            jd[q] += k[q];
            if (jd[q] >= n) jd[q] -= n;
          }
        }
#pragma unroll
        for (int q = 0; q < GL_KT; ++q)
#pragma unroll
          for (int j = 0; j < GL_MT; ++j) {
            const float wv = wk[q] * fv[j];
            acc[q][j] = fmaf(wv, s[q][j], acc[q][j]);
            env[q][j] = fmaf(wv, wv, env[q][j]);
          }
      }
#pragma unroll
      for (int q = 0; q < GL_KT; ++q) {
        const int s0 = u + q * HQ;
        if (s0 >= hop) continue;
#pragma unroll
        for (int j = 0; j < GL_MT; ++j) {
          const int i = (m0 + j) * hop + s0;
          if (i >= pad && i < pad + S) xp[i] = env[q][j] < 1e-11f ? 0.f : acc[q][j] * inv_n / env[q][j];
        }
      }
    }
  };
  // torch.stft's reflect padding of the S real samples (rpad behind: one more than pad for odd n)
  auto reflect = [&]() {
    for (int i = tid; i < pad; i += nthr) xp[i] = xp[2 * pad - i];
    for (int i = tid; i < rpad; i += nthr) xp[pad + S + i] = xp[pad + S - 2 - i];
  };
  // R = stft(xp); then the phase update, or (last) the residual's sums
  const int ntt = (Tb + GL_TT - 1) / GL_TT;
  auto stft = [&](bool last) {
    double num = 0.0, den = 0.0;
    for (int e = tid; e < ntt * F; e += nthr) {
      const int tt = e / F, f = e - tt * F, t0 = tt * GL_TT;
      const float* xr[GL_TT];
#pragma unroll
      for (int j = 0; j < GL_TT; ++j) xr[j] = xp + min(t0 + j, Tb - 1) * hop;
      float re[GL_TT], im[GL_TT];
#pragma unroll
      for (int j = 0; j < GL_TT; ++j) re[j] = im[j] = 0.f;
      int jd = 0;  // (f * k) mod n
      for (int k = 0; k < n; ++k) {
        const float wc = w[k] * cs[jd], wsn = w[k] * sn[jd];
#pragma unroll
        for (int j = 0; j < GL_TT; ++j) {
          const float v = xr[j][k];
          re[j] = fmaf(v, wc, re[j]);
          im[j] = fmaf(-v, wsn, im[j]);
        }
        jd += f;
        if (jd >= n) jd -= n;
      }
#pragma unroll
      for (int j = 0; j < GL_TT; ++j) {
        const int t = t0 + j;
        if (t >= Tb) continue;
        const float A = magnitude(t, f);
        const int at = t * F + f;
        if (last) {
          const double d = (double)sqrtf(re[j] * re[j] + im[j] * im[j]) - (double)A;
          num += d * d;
          den += (double)A * (double)A;
        } else {
          const float2 rp = Rp[at];
          const float tr = re[j] - a.alpha * rp.x, ti = im[j] - a.alpha * rp.y;
          Rp[at] = make_float2(re[j], im[j]);
          const float sc = A / (sqrtf(tr * tr + ti * ti) + 1e-16f);
          C[at] = make_float2(tr * sc, ti * sc);
        }
      }
    }
    if (last) {  // lanes in a shuffle tree, waves in wave order
      num = wave_sum_d(num);
      den = wave_sum_d(den);
      if ((tid & 63) == 0) {
        red[tid >> 6] = num;
        red[16 + (tid >> 6)] = den;
      }
      __syncthreads();
      if (tid == 0) {
        double sn_ = 0.0, sd_ = 0.0;
        for (int i = 0; i < nthr / 64; ++i) {
          sn_ += red[i];
          sd_ += red[16 + i];
        }
        a.residual[b] = (float)sqrt(sn_ / sd_);
      }
    }
  };

  for (int it = 0;; ++it) {
    istft();
    __syncthreads();
    const bool last = it == a.n_iter;
    if (last) {
      for (int i = tid; i < a.smax; i += nthr) wrow[i] = i < S ? xp[pad + i] : 0.f;
      if (!a.residual) break;
    }
    reflect();
    __syncthreads();
    stft(last);
    if (last) break;
    __syncthreads();
  }
}

// n-point twiddle table per (device, n): cos | sin, built once on the host in
// double and rounded once (sin(pi) is stored as the exact 0 it stands for)
static int gl_twiddles(int n, const float** out) {
  static std::mutex mu;
  static std::vector<std::pair<long, float*>> cache;  // key: device * 2^20 + n
  int dev = 0;
  ABCD_TRY(hipGetDevice(&dev));
  const long key = (long)dev * (1L << 20) + n;
  std::lock_guard<std::mutex> lk(mu);
  for (auto& kv : cache)
    if (kv.first == key) {
      *out = kv.second;
      return 0;
    }
  std::vector<float> h(2 * (size_t)n);
  for (int j = 0; j < n; ++j) {
    const double ang = 2.0 * M_PI * (double)j / (double)n;
    h[j] = (float)std::cos(ang);
    h[n + j] = (2 * j == n) ? 0.f : (float)std::sin(ang);
  }
  float* d = nullptr;
  ABCD_TRY(hipMalloc((void**)&d, h.size() * sizeof(float)));
  ABCD_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  cache.push_back({key, d});
  *out = d;
  return 0;
}

// ABCD_GL_LDS=0 keeps the signal in the workspace whatever its length
static bool gl_lds_on() {
  const char* v = getenv("ABCD_GL_LDS");
  return !(v && v[0] == '0');
}

// ABCD_GL_WAVES=4 / 8 runs the workgroups with fewer than the default 16 waves
// (same-box A/B: DESIGN.md s3.8 has the measurement); any partition of a phase's
// items over the threads gives the same samples, every item's sums being its
// own (the residual's sum of thread partials follows the thread count)
static int gl_threads() {
  const char* v = getenv("ABCD_GL_WAVES");
  const int w = (v && v[0]) ? atoi(v) : 16;
  return (w == 4 || w == 8) ? 64 * w : GL_THREADS;
}

// LDS bytes of the two forms for a longest segment of T frames; the workspace layout
struct GlPlan {
  bool ok;
  size_t lds_tables, lds_resident;  // global form / LDS form
  size_t off_bytes, spec_bytes, sig_ld, total;
};
static GlPlan gl_plan(int B, int T, int n, int hop) {
  GlPlan p{};
  if (B < 1 || T < 1 || T > GL_MAX_T || n < 2 || n > (1 << 20) || hop < 1) return p;
  const size_t F = (size_t)n / 2 + 1;
  const size_t Pn = (size_t)hop * (size_t)(T - 1) + (size_t)n;
  if (Pn >= (1ull << 30) || (size_t)T * F >= (1ull << 28)) return p;  // 32-bit indices inside a segment
  p.lds_tables = GL_LDS_FIXED + 3 * (size_t)n * sizeof(float);
  if (p.lds_tables > GL_LDS_MAX) return p;
  p.lds_resident = p.lds_tables + Pn * sizeof(float);
  p.off_bytes = (((size_t)T + 1) * sizeof(int) + 255) & ~(size_t)255;
  p.spec_bytes = (size_t)B * (size_t)T * F * sizeof(float2);
  p.sig_ld = (Pn + 63) & ~(size_t)63;
  p.total = p.off_bytes + 2 * p.spec_bytes + (size_t)B * p.sig_ld * sizeof(float) + 256;
  p.ok = true;
  return p;
}

}  // namespace abcd

using namespace abcd;

extern "C" int abcd_griffin_lim_samples(int frames, int n_fft, int hop, int center) {
  if (frames < 1 || n_fft < 2 || hop < 1 || !center) return 0;
  const long long S = (long long)hop * (frames - 1);
  if (S <= n_fft - n_fft / 2 || S >= (1LL << 30)) return 0;
  return (int)S;
}

extern "C" size_t abcd_griffin_lim_workspace_bytes(int B, int T, int n_fft, int hop) {
  const GlPlan p = gl_plan(B, T, n_fft, hop);
  return p.ok ? p.total : 0;
}

extern "C" int abcd_griffin_lim(const float* logamp, int ld, const int64_t* batch_sizes, int T, int L, int B,
                                int n_fft, int hop, int center, const float* window, float eps, float norm,
                                const float* phase0, int ldp, int n_iter, float momentum, float* wave, int ldw,
                                float* residual, void* ws, size_t ws_bytes, void* stream) {
  ABCD_REQUIRE(logamp && batch_sizes && window && phase0 && wave && ws);
  ABCD_REQUIRE(center == 1 && n_iter >= 0 && momentum >= 0.f && momentum < 1.f && norm != 0.f);
  const GlPlan p = gl_plan(B, T, n_fft, hop);
  ABCD_REQUIRE(p.ok && ws_bytes >= p.total);
  const int F = n_fft / 2 + 1;
  ABCD_REQUIRE(ld >= F && ldp >= F);
  ABCD_REQUIRE(validate_batch(batch_sizes, T, L, B) == 0);
  const int smax = abcd_griffin_lim_samples(T, n_fft, hop, 1);
  ABCD_REQUIRE(ldw >= smax && ldw >= 1);
  hipStream_t s = (hipStream_t)stream;
  const std::vector<int> off = step_offsets(batch_sizes, T);
  char* base = (char*)ws;
  int* doff = (int*)base;
  float2* C = (float2*)(base + p.off_bytes);
  float2* Rp = (float2*)(base + p.off_bytes + p.spec_bytes);
  float* sig = (float*)(base + p.off_bytes + 2 * p.spec_bytes);
  ABCD_TRY((hipError_t)upload_offsets(s, off, doff));  // pinned ring + async copy: no host synchronisation
  const float* tw = nullptr;
  ABCD_TRY((hipError_t)gl_twiddles(n_fft, &tw));
  // the switch point follows from the kernel's real LDS use at the longest segment
  const bool resident = gl_lds_on() && p.lds_resident <= GL_LDS_MAX;
  const size_t lds = resident ? p.lds_resident : p.lds_tables;
  GlArgs a{logamp, phase0, doff, window, tw, C, Rp, sig, wave, residual, (long)p.sig_ld, ld, ldp, ldw, T, n_fft, hop, F,
           n_iter, smax, eps, norm, momentum / (1.0f + momentum)};
  const int threads = gl_threads();
  if (threads == GL_THREADS)
    note_dispatch(TK_GRIFFIN_LIM, "griffin_lim<%s,dft> grid %d lds %zu", resident ? "lds" : "global", B, lds);
  else
    note_dispatch(TK_GRIFFIN_LIM, "griffin_lim<%s,dft> grid %d lds %zu waves %d", resident ? "lds" : "global", B, lds,
                  threads / 64);
  {
    TimedScope ts(s, TK_GRIFFIN_LIM);
    if (resident) {
      ABCD_TRY(hipFuncSetAttribute((const void*)griffin_lim<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)GL_LDS_MAX));
      griffin_lim<true><<<B, threads, lds, s>>>(a);
    } else {
      ABCD_TRY(hipFuncSetAttribute((const void*)griffin_lim<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)GL_LDS_MAX));
      griffin_lim<false><<<B, threads, lds, s>>>(a);
    }
  }
  ABCD_CHECK_LAUNCH();
  return 0;
}
