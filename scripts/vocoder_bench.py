#!/usr/bin/env python
"""Times the Griffin-Lim vocoder (abcd_griffin_lim) on one GPU at the config-2
framing of bench.py (n_fft 256, hop 128, T <= 200, F = 129), 32 iterations at
momentum 0.99 without the residual:

  B = 128   "prototypes": a full rectangle, every segment 200 frames
  B = 512   a training batch: lengths uniform in [20, 200], the longest 200

against the same loop composed from torch.stft / torch.istft on the same GPU on
the zero-padded rectangle (what a user would write today; for B = 512 the
padding makes its output differ at the segment ends, its cost is that of the
rectangle).  Each is warmed up and then timed --runs times with stream events,
the two alternating; the best and the median are kept.  ABCD_GL_WAVES = 8 and 4
(fewer waves per workgroup) are timed in the same run for the A/B of DESIGN.md
s3.8.  The per-iteration time is (t(32) - t(0)) / 32.  Writes one JSON document
to --out (default profiles/vocoder_bench.json) and to stdout.

    python scripts/vocoder_bench.py [--runs 5] [--warmup 2] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "seq2seq_abcd-vae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_FFT, HOP, T_MAX, ITERS, MOMENTUM, EPS = 256, 128, 200, 32, 0.99, 2.0 ** -15


def torch_griffin_lim(A, phase0, window, n_iter, momentum):
    """A, phase0: B x F x T on the device -> B x S"""
    length = HOP * (A.shape[2] - 1)
    C = torch.polar(A, phase0)
    prev = torch.zeros_like(C)
    alpha = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        y = torch.istft(C, N_FFT, hop_length=HOP, window=window, center=True, length=length)
        R = torch.stft(y, N_FFT, hop_length=HOP, window=window, center=True, pad_mode="reflect", return_complex=True)
        t = R - alpha * prev
        prev = R
        C = A * t / (t.abs() + 1e-16)
    return torch.istft(C, N_FFT, hop_length=HOP, window=window, center=True, length=length)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return dict(best_ms=min(ms), median_ms=statistics.median(ms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "vocoder_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vocoder_bench.py needs a GPU: timings are not taken on the CPU")
    from modules import _native as N, ops
    F = N_FFT // 2 + 1
    window = torch.hann_window(N_FFT, device="cuda")
    res = dict(framing=dict(n_fft=N_FFT, hop=HOP, T=T_MAX, F=F), iterations=ITERS, momentum=MOMENTUM, runs=a.runs,
               warmup=a.warmup, library=N.lib().abcd_version().decode())
    for B in (128, 512):
        g = torch.Generator().manual_seed(B)
        if B == 128:
            lengths = [T_MAX] * B
        else:
            lengths = sorted([T_MAX] + torch.randint(20, T_MAX + 1, (B - 1,), generator=g).tolist(), reverse=True)
        bs = torch.tensor([sum(n > t for n in lengths) for t in range(T_MAX)], dtype=torch.int64)
        L = int(bs.sum())
        x = (torch.randn(L, F, generator=g) * 2.0 + 3.0).cuda()
        ph = ((torch.rand(L, F, generator=g) * 2.0 - 1.0) * np.pi).cuda()
        # the same spectra as a zero-padded B x F x T rectangle for the torch composition
        off = np.concatenate([[0], np.cumsum(bs.numpy())])
        rows = torch.full((B, T_MAX), L, dtype=torch.int64)  # L: a row of zeros
        for t in range(T_MAX):
            rows[:int(bs[t]), t] = torch.arange(off[t], off[t] + int(bs[t]))
        mag = torch.cat([(torch.exp(x) - EPS).clamp_min(0.0), torch.zeros(1, F, device="cuda")])
        A = mag[rows.cuda()].permute(0, 2, 1).contiguous()
        P0 = torch.cat([ph, torch.zeros(1, F, device="cuda")])[rows.cuda()].permute(0, 2, 1).contiguous()

        def ours(n_iter=ITERS):
            return ops.griffin_lim(x, bs, window, ph, HOP, EPS, 1.0, n_iter, MOMENTUM, False)[0]

        def composed():
            return torch_griffin_lim(A, P0, window, ITERS, MOMENTUM)
        r = dict(B=B, L=L, frames_min=min(lengths), samples_max=HOP * (T_MAX - 1))
        with torch.no_grad():
            os.environ.pop("ABCD_GL_WAVES", None)
            for _ in range(a.warmup):
                w_ours, w_torch = ours(), composed()
                ours(0)
            torch.cuda.synchronize()
            r["dispatch"] = N.dispatch()["griffin_lim"][0]
            full = [b for b, n in enumerate(lengths) if n == T_MAX]  # no padding: the two compute the same thing
            d = (w_ours[full] - w_torch[full]).abs().max() / w_torch[full].abs().max()
            r["ours_vs_torch_max_over_peak"] = float(d)
            t_ours, t_torch, t_zero = [], [], []
            for _ in range(a.runs):  # alternating
                t_ours.append(event_ms(ours))
                t_torch.append(event_ms(composed))
                t_zero.append(event_ms(lambda: ours(0)))
            r["griffin_lim"], r["torch_composed"], r["griffin_lim_0_iterations"] = (
                summary(t_ours), summary(t_torch), summary(t_zero))
            r["torch_over_ours"] = min(t_torch) / min(t_ours)
            r["per_iteration_us"] = (min(t_ours) - min(t_zero)) / ITERS * 1e3
            # real DFT work of one iteration (an inverse and a forward transform of every frame):
            # 2 * L * F * n_fft complex-by-real multiply-adds, 2 fused multiply-adds each
            r["fma_per_iteration"] = 2 * 2 * L * F * N_FFT
            r["fp32_vector_peak_fraction"] = 2.0 * r["fma_per_iteration"] / (r["per_iteration_us"] * 1e-6) / 157e12
            for waves in (8, 4):
                os.environ["ABCD_GL_WAVES"] = str(waves)
                ours()
                ts = [event_ms(ours) for _ in range(a.runs)]
                r[f"griffin_lim_waves{waves}"] = dict(summary(ts), dispatch=N.dispatch()["griffin_lim"][0])
            os.environ.pop("ABCD_GL_WAVES", None)
        res[f"B{B}"] = r
    res["device_status"] = int(N.lib().abcd_device_status())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
