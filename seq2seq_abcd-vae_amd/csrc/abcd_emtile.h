// abcd_emtile.h -- the emission tile of pair_nll (abcd_pairwise.hip) and
// span_nll (abcd_span.hip): 32 rows of x against 32 prototypes, one step at a
// time, in a 256-thread workgroup.  Both kernels get the same staging, the same
// per-term expressions and the same order of sums from here (a frame's F
// columns in column order in fp32), so their results agree bit for bit on the
// same frames; what a kernel does with a finished frame is its own.
//
// Per step the tile's 32 rows of x and its 32 prototype rows of mu / log_var
// (contiguous: t P + p0 ...) are staged in LDS, 64 columns at a time, wave w
// taking rows w, w + 4, ... with its lanes on the columns (coalesced).  e^-lv
// and 0.5 sum_f (log 2pi + lv) are formed there, once per staged prototype
// element, so a pair costs a subtract, a multiply and a fused multiply-add per
// column.  Thread (i, j) = (tid / 16, tid % 16) owns rows 2 i, + 1 and
// prototypes p0 + j, + 16.  Prototypes >= P are not read; columns >= F read as
// zero terms.  Which rows of x exist is the kernel's affair: it fetches them
// into EmRegs::x itself, zero where there is none.
//
// The passes (step, column chunk) are pipelined inside the workgroup: the
// global loads of pass i + 1 are issued into registers (EmRegs) before pass i
// is computed from LDS, and the two LDS images alternate, so one barrier per
// pass orders everything (a thread writing image i + 1 has passed barrier i,
// which every thread reaches only after computing pass i - 1 from that image):
//
//   fetch(0)
//   for each pass it:  tile.stage(it & 1, ...);  __syncthreads();
//                      fetch(it + 1);  tile.accumulate(it & 1, ...)
//
// The kernel passes its own w = tid / 64, lane = tid % 64, ti = tid / 16 and
// tj = tid % 16 in: recomputed in here from threadIdx.x they cost pair_nll six
// VGPRs (162 against 156 before the tile was shared, 154 with them passed).
#pragma once
#include "abcd_common.h"
#include "abcd_special.h"

namespace abcd {

constexpr int EM_TR = 32;          // rows of x per tile
constexpr int EM_TP = 32;          // prototypes per tile
constexpr int EM_FC = 64;          // columns staged per pass
constexpr int EM_LD = EM_FC + 4;   // LDS row stride (16-byte aligned rows, staggered banks)

// What one thread holds of the next staging pass while the current one is
// computed: its 8 rows x 1 column of x, mu and log_var.
struct EmRegs {
  float x[EM_TR / 4], m[EM_TP / 4], l[EM_TP / 4];
};

// the prototype half of a fetch: step t, column f, rows t P + p0 + w + 4 i
DEV void em_fetch_proto(EmRegs& g, const float* __restrict__ MU, long ldm, const float* __restrict__ LV, long ldl,
                        int w, int t, int p0, int P, int f, int F) {
  const bool fin = f < F;
#pragma unroll
  for (int i = 0; i < EM_TP / 4; ++i) {
    const int r = w + 4 * i;
    const bool ok = fin && p0 + r < P;
    const long row = (long)t * P + p0 + r;
    g.m[i] = ok ? MU[row * ldm + f] : 0.f;
    g.l[i] = ok ? LV[row * ldl + f] : 0.f;
  }
}

DEV void em_term(float& q, const float4& a, const float4& u, const float4& e) {
  float d = a.x - u.x; q = fmaf(d * d, e.x, q);
  d = a.y - u.y; q = fmaf(d * d, e.y, q);
  d = a.z - u.z; q = fmaf(d * d, e.z, q);
  d = a.w - u.w; q = fmaf(d * d, e.w, q);
}

// The two LDS images: x, mu, e^-lv and the prototypes' 0.5 sum_f (log 2pi + lv).
struct __attribute__((aligned(16))) EmTile {
  float xs[2][EM_TR * EM_LD], ms[2][EM_TP * EM_LD], wsh[2][EM_TP * EM_LD], cs[2][EM_TP];

  // The fetched pass (column chunk f0 of a step; first / last: the step's
  // first / last chunk) into image k.  csum is the thread's running
  // sum_f (log 2pi + lv) of its 8 prototype rows; cs[k] is complete after the
  // step's last chunk.
  DEV void stage(int k, const EmRegs& g, float (&csum)[EM_TP / 4], int w, int lane, int p0, int P, int f0, int F,
                 bool first, bool last) {
    const bool fin = f0 + lane < F;
#pragma unroll
    for (int i = 0; i < EM_TR / 4; ++i) xs[k][(w + 4 * i) * EM_LD + lane] = g.x[i];
#pragma unroll
    for (int i = 0; i < EM_TP / 4; ++i) {
      const int r = w + 4 * i;
      const bool ok = fin && p0 + r < P;
      const float l = g.l[i];
      ms[k][r * EM_LD + lane] = g.m[i];
      wsh[k][r * EM_LD + lane] = ok ? __expf(-l) : 0.f;
      const float cv = ok ? 1.8378770664093453f + l : 0.f;
      csum[i] = first ? cv : csum[i] + cv;  // per lane: columns lane, lane + 64, ... in order
    }
    if (last) {  // the lanes' sums in a fixed tree
#pragma unroll
      for (int i = 0; i < EM_TP / 4; ++i) {
        const float v = wave_sum(csum[i]);
        if (lane == 0) cs[k][w + 4 * i] = 0.5f * v;
      }
    }
  }

  // Image k's columns into the thread's 2 x 2 sums q[row][prototype] of
  // (x - mu)^2 e^-lv, which start over at a step's first chunk.  After the last
  // chunk the frame's term of pair (i, j) is cs[k][tj + 16 j] + 0.5f * q[i][j].
  DEV void accumulate(int k, float (&q)[2][2], int ti, int tj, int f0, int F, bool first) const {
    if (first) q[0][0] = q[0][1] = q[1][0] = q[1][1] = 0.f;
    const int n4 = (min(F - f0, EM_FC) + 3) >> 2;
    const float4* x0 = (const float4*)(xs[k] + (2 * ti) * EM_LD);
    const float4* x1 = (const float4*)(xs[k] + (2 * ti + 1) * EM_LD);
    const float4* m0 = (const float4*)(ms[k] + tj * EM_LD);
    const float4* m1 = (const float4*)(ms[k] + (tj + 16) * EM_LD);
    const float4* w0 = (const float4*)(wsh[k] + tj * EM_LD);
    const float4* w1 = (const float4*)(wsh[k] + (tj + 16) * EM_LD);
#pragma unroll 2
    for (int n = 0; n < n4; ++n) {
      const float4 a0 = x0[n], a1 = x1[n], u0 = m0[n], u1 = m1[n], e0 = w0[n], e1 = w1[n];
      em_term(q[0][0], a0, u0, e0);
      em_term(q[0][1], a0, u1, e1);
      em_term(q[1][0], a1, u0, e0);
      em_term(q[1][1], a1, u1, e1);
    }
  }
};

}  // namespace abcd
