#!/usr/bin/env python
"""Times pairwise scoring (every segment against every category prototype) on
one GPU at the c2 shape of bench.py (b = 512, lengths as bench.py draws them,
F = 129), for P = 128 and P = 1024 prototypes:

  abcd_pairwise_nll    3 warm-up calls then 10 timed ones, each bracketed by
                       stream events (the whole call: workspace, offset-table
                       copy, both launches) and by the library's live timing
                       (id 13: the tile kernel and the slice reduction)
  abcd_pair_posterior  the same (live timing id 14)
  prototypes()         the P-row decode that feeds them (events; id 3)
  score()              in the same run, one B-row call -- a decoder forward
                       (id 3) and abcd_segment_losses -- and, for P = 128, P of
                       them: the only route to the matrix without this kernel

and writes one JSON document with the medians, the count of squared-difference
terms, the achieved fraction of the fp32 vector peak (a term is a subtract, a
multiply and a fused multiply-add: 4 flops of the 157 TFLOP/s peak) and the
ratios, to --out (default profiles/pairwise_bench.json) and to stdout.

    python scripts/pairwise_bench.py [--calls 10] [--warmup 3] [--out PATH]
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

VECTOR_PEAK_FLOPS = 157e12  # fp32 vector peak of the MI355X (a fused multiply-add counts 2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "pairwise_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pairwise_bench.py needs a GPU: timings are not taken on the CPU")
    import bench
    from modules import _native as N, ops
    from score_bench import timed
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec, samp = step.decoder.eval(), step.sampler.eval()
    batch = bench.make_batch(cfg, 0, "cuda")
    bsz, data, is_off = batch["batch_sizes"], batch["data"], batch["is_offset"]
    B, L, T, F = cfg["B"], batch["L"], batch["T"], cfg["F"]
    res = dict(shape=dict(B=B, T=T, L=L, F=F), calls=a.calls, warmup=a.warmup)
    with torch.no_grad():
        feats_b = samp.codebook.detach().t()[torch.arange(B, device="cuda") % cfg["K"]].contiguous()

        def score():
            return dec.score(feats_b, bsz, ground_truth_out=data, ground_truth_offset=is_off, mean=True)
        res["score_call_us"], res["score_dec_fwd_kernel_us"] = timed(score, a.calls, a.warmup, N.DEC_FWD)
        for P in (128, 1024):
            code = samp.codebook.detach().t().contiguous()  # K x D
            feats = code if P == cfg["K"] else torch.randn(P, cfg["D"], device="cuda",
                                                           generator=torch.Generator("cuda").manual_seed(P))

            def decode():
                return dec.prototypes(feats, T)
            protos = decode()
            mu, lv, offl = (t.reshape(T * P, -1) for t in protos)

            def pair():
                return ops.pairwise_nll(data, bsz, is_off, mu, lv, offl.reshape(-1), P, F)
            em, off = pair()
            lw = torch.randn(P, device="cuda")

            def post():
                return ops.pair_posterior(em, off, lw)
            r = dict(P=P)
            r["prototypes_call_us"], r["prototypes_dec_fwd_kernel_us"] = timed(decode, a.calls, a.warmup, N.DEC_FWD)
            if not r["prototypes_dec_fwd_kernel_us"]:  # this row count takes a decoder route without the timing hook
                r["prototypes_dec_fwd_kernel_us"] = None
            r["pair_nll_call_us"], r["pair_nll_kernel_us"] = timed(pair, a.calls, a.warmup, N.PAIR_NLL)
            r["pair_post_call_us"], r["pair_post_kernel_us"] = timed(post, a.calls, a.warmup, N.PAIR_POST)
            d = N.dispatch()
            r["pair_nll_dispatch"], r["pair_post_dispatch"] = d["pair_nll"][0], d["pair_post"][0]
            r["terms"] = L * P * F
            r["vector_peak_fraction"] = 4.0 * r["terms"] / (r["pair_nll_kernel_us"] * 1e-6) / VECTOR_PEAK_FLOPS
            r["pair_nll_over_one_score_dec_fwd"] = r["pair_nll_kernel_us"] / res["score_dec_fwd_kernel_us"]
            r["workspace_bytes"] = int(N.lib().abcd_pairwise_nll_workspace_bytes(T, B, P))
            if P == 128:  # the matrix by the only route without the kernel: P calls of score()
                def loop():
                    for p in range(P):
                        dec.score(feats[p:p + 1].expand(B, -1), bsz, ground_truth_out=data, ground_truth_offset=is_off,
                                  mean=True)
                loop()
                torch.cuda.synchronize()
                ev = []
                for _ in range(a.calls):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    loop()
                    e.record()
                    e.synchronize()
                    ev.append(s.elapsed_time(e) * 1e3)
                r["score_loop_us"] = statistics.median(ev)
                r["score_loop_over_pairwise_route"] = r["score_loop_us"] / (
                    r["prototypes_call_us"] + r["pair_nll_call_us"])
            res[f"P{P}"] = r
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
