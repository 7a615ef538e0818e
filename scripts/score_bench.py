#!/usr/bin/env python
"""Times the per-segment scoring entry points on one GPU at the c2 shape of
bench.py (b = 512, lengths as bench.py draws them, F = 129):

  abcd_segment_losses   after a decoder forward on the same batch, 3 warm-up
                        calls then 10 timed ones, each bracketed by stream
                        events (the whole call: offset-table copy + kernel)
                        and by the library's live timing (id 11: the kernel);
                        once with the inputs left where the previous call put
                        them, once with a 1 GiB fill in between (inputs back
                        in HBM)
  abcd_sampler_kl_rows  the same at K = 128 and K = 1024 (live timing id 12)
  decoder forward       the op the scoring follows (events; live timing id 3)

and prints one JSON line with the medians, the byte counts computed from the
shapes and the time those bytes take at the achievable HBM rate (6.3 TB/s).

    python scripts/score_bench.py [--calls 10] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "seq2seq_abcd-vae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def timed(fn, calls, warmup, kid, between=None):
    """-> (median call us by events, median kernel us by the library's timing id `kid`)"""
    from modules import _native as N
    lib = N.lib()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, ker = [], []
    out = (ctypes.c_double * 4)()
    for _ in range(calls):
        if between is not None:
            between()
        lib.abcd_timing_reset()
        lib.abcd_timing_enable(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        lib.abcd_timing_enable(0)
        ev.append(a.elapsed_time(b) * 1e3)
        lib.abcd_timing_read_kernel(kid, out)
        ker.append(out[0] * 1e3)
    return statistics.median(ev), statistics.median(ker)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("score_bench.py needs a GPU: timings are not taken on the CPU")
    import bench
    from modules import _native as N, ops
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec = step.decoder.eval()
    batch = bench.make_batch(cfg, 0, "cuda")
    bsz, data, is_off = batch["batch_sizes"], batch["data"], batch["is_offset"]
    B, L, F = cfg["B"], batch["L"], cfg["F"]
    feats = torch.randn(B, cfg["D"], device="cuda")
    eps = torch.zeros(L, F, device="cuda")

    def forward():
        return ops.decoder(feats, bsz, None, data, is_off, eps, 0, 0, None, dec._param_list(), dec._cfg_list(1))

    with torch.no_grad():
        _, _, _, mu, lv, offl, _ = forward()
        flush_buf = torch.empty(1 << 28, device="cuda")  # 1 GiB of fp32: past the 256 MiB Infinity Cache

        def seg():
            return ops.segment_losses(data, bsz, mu, lv, offl, is_off, F)
        res = dict(shape=dict(B=B, T=batch["T"], L=L, F=F), calls=a.calls, warmup=a.warmup)
        res["decoder_forward_us"], res["dec_fwd_kernel_us"] = timed(forward, a.calls, a.warmup, 3)
        res["seg_losses_call_us"], res["seg_losses_kernel_us"] = timed(seg, a.calls, a.warmup, N.SEG_LOSSES)
        res["seg_losses_call_us_hbm"], res["seg_losses_kernel_us_hbm"] = timed(
            seg, a.calls, a.warmup, N.SEG_LOSSES, between=lambda: flush_buf.fill_(1.0))
        res["seg_losses_dispatch"] = N.dispatch()["seg_losses"][0]
        nbytes = 3 * L * F * 4 + 2 * L * 4 + (batch["T"] + 1) * 4 + 3 * B * 4
        res["seg_losses_bytes"] = nbytes
        res["seg_losses_hbm_floor_us"] = nbytes / HBM_BYTES_PER_S * 1e6
        res["seg_losses_share_of_forward"] = res["seg_losses_kernel_us_hbm"] / res["decoder_forward_us"]
        for K in (128, 1024):
            logits = torch.randn(B, K, device="cuda") * 2.0
            psl = torch.randn(K, device="cuda")
            kcfg = [16, 16, K, 16, 0, 0, 0]

            def kl():
                return ops.sampler_kl_rows(logits, psl, kcfg, 1.0, float(cfg["N"]))
            call, ker = timed(kl, a.calls, a.warmup, N.KL_ROWS)
            kb = B * K * 4 + K * 4 + B * 4 + 4
            res[f"kl_rows_K{K}"] = dict(call_us=call, kernel_us=ker, bytes=kb, hbm_floor_us=kb / HBM_BYTES_PER_S * 1e6,
                                        dispatch=N.dispatch()["kl_rows"][0])
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
