#!/usr/bin/env python
"""Times time-warped scoring (abcd_warp_nll: every segment aligned to every
category prototype) on one GPU at the c2 shape of bench.py (b = 512, lengths as
bench.py draws them, F = 129) with P = 128 prototypes decoded for T_proto = 300
steps, for band = -1 (none) and band = 32, Viterbi and marginal, and
abcd_pairwise_nll in the same run:

  warp_nll  --warmup calls then --calls timed ones per (band, mode), each
            bracketed by stream events (the whole call: workspace, offset-table
            copy, the launch)
  pair_nll  the same, on the same batch and the first T steps of the same
            prototypes

and writes one JSON document with the medians, the term counts, the term rates
and the ratio warp / pair of the rates to --out (default
profiles/warp_bench.json) and to stdout.  A term is one (x - mu)^2 e^-lv of one
column.  pair_nll's count is L P F.  warp_nll's is counted over the cells that
EXIST (s < T_proto, s <= 2 t, |s - t| <= band), times P F: what the definition
asks for, not what the tiling computes on top of it (the parts of 32 x 32 tiles
that hang over the band, the s = 2 t line and T_proto; `tile_terms` counts
those too).

    python scripts/warp_bench.py [--calls 10] [--warmup 3] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "seq2seq_abcd-vae_amd"), os.path.join(REPO, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

P_PROTO, T_PROTO, BANDS = 128, 300, (-1, 32)


def cell_counts(lengths, S, band, tile=32):
    """(cells that exist, cells of the 32 x 32 tiles the kernel computes) summed over the segments."""
    import numpy as np
    exist = tiles = 0
    for n in lengths:
        t = np.arange(n)
        lo = np.maximum(0, t - band) if band >= 0 else np.zeros(n, dtype=np.int64)
        hi = np.minimum(S - 1, 2 * t)
        if band >= 0:
            hi = np.minimum(hi, t + band)
        exist += int(np.maximum(hi - lo + 1, 0).sum())
        for t0 in range(0, n, tile):
            tl = min(t0 + tile, n) - 1
            slo = max(0, t0 - band) if band >= 0 else 0
            shi = min(S - 1, 2 * tl, tl + band if band >= 0 else S)
            if shi >= slo:
                tiles += (shi // tile - slo // tile + 1) * tile * tile
    return exist, tiles


def events(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ev), ev


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "warp_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("warp_bench.py needs a GPU: timings are not taken on the CPU")
    import bench
    from modules import _native as N, ops
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec, samp = step.decoder.eval(), step.sampler.eval()
    batch = bench.make_batch(cfg, 0, "cuda")
    bsz, data, is_off = batch["batch_sizes"], batch["data"], batch["is_offset"]
    B, F = cfg["B"], cfg["F"]
    T, L = int(bsz.numel()), int(data.shape[0])
    lengths = [int((bsz > b).sum()) for b in range(B)]
    res = dict(shape=dict(B=B, T=T, L=L, F=F, P=P_PROTO, T_proto=T_PROTO), calls=a.calls, warmup=a.warmup)
    with torch.no_grad():
        code = samp.codebook.detach().t().contiguous()  # K x D
        assert code.shape[0] == P_PROTO
        protos = dec.prototypes(code, T_PROTO)
        mu, lv, offl = (t.reshape(T_PROTO * P_PROTO, -1) for t in protos)

        def pair():
            return ops.pairwise_nll(data, bsz, is_off, mu, lv, offl.reshape(-1), P_PROTO, F)
        us, _ = events(pair, a.calls, a.warmup)
        terms = L * P_PROTO * F
        res["pair_nll"] = dict(call_us=us, terms=terms, terms_per_s=terms / (us * 1e-6),
                               dispatch=N.dispatch()["pair_nll"][0])
        moves = list(ops.DEFAULT_LOG_MOVES)
        for band in BANDS:
            exist, tiles = cell_counts(lengths, T_PROTO, band)
            for marginal in (False, True):
                def warp():
                    return ops.warp_nll(data, bsz, is_off, mu, lv, offl.reshape(-1), moves, band, marginal, P_PROTO, F)
                us, all_us = events(warp, a.calls, a.warmup)
                terms = exist * P_PROTO * F
                r = dict(band=band, marginal=marginal, call_us=us, calls_us=all_us, terms=terms,
                         tile_terms=tiles * P_PROTO * F, terms_per_s=terms / (us * 1e-6),
                         tile_terms_per_s=tiles * P_PROTO * F / (us * 1e-6))
                r["rate_over_pair_nll"] = r["terms_per_s"] / res["pair_nll"]["terms_per_s"]
                r["tile_rate_over_pair_nll"] = r["tile_terms_per_s"] / res["pair_nll"]["terms_per_s"]
                r["time_over_pair_nll"] = us / res["pair_nll"]["call_us"]
                res[f"band{band}_{'marginal' if marginal else 'viterbi'}"] = r
        res["device_status"] = int(N.lib().abcd_device_status())
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
