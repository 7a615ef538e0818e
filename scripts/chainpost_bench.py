#!/usr/bin/env python
"""Times the segmentation posteriors under the chain (the semi-Markov
forward-backward over (frame, last category), ops.span_chain_posterior) on one
GPU at syntax_bench.py's shape and recording: N = 15 000 frames at a 4 ms hop,
D = 200, K = 128 prototypes, F = 129; 3 warm-up calls then 10 timed ones, each
bracketed by stream events around the operator, medians reported:

  span_chain_viterbi    the yardstick, in the same run on the same table
  span_chain_posterior  the whole operator and microseconds per step (a step is
                        one frame of BOTH sweeps), its ratio to the yardstick:
                          resident   K = 128, log_trans in LDS
                          streaming  K = 130 (the table with two categories
                                     repeated), log_trans read from global memory
                        each tiled and with a gap and a bonus, and each
                          plain       the lattice and the per-frame posteriors
                          counts      with the expected bigram counts
                          table       with span_post (a second kernel)
                          all         both
                        and at temperature 4 (scale = 0.25), plain

and writes one JSON document to --out (default profiles/chainpost_bench.json)
and to stdout.  Nothing outside the repository is read.  Run it under a time
limit of its own:

    timeout -k 10 600 python scripts/chainpost_bench.py [--calls 10] [--warmup 3] [--out PATH]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "seq2seq_abcd-vae_amd"), os.path.join(REPO, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from segment_bench import events  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15000)
    ap.add_argument("--max_length", type=int, default=200)
    ap.add_argument("--stream_k", type=int, default=130)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "chainpost_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("chainpost_bench.py needs a GPU: timings are not taken on the CPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import bench
    from modules import _native as N, ops
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec, samp = step.decoder.eval(), step.sampler.eval()
    n, D, F, P = a.frames, a.max_length, cfg["F"], cfg["K"]
    res = dict(shape=dict(N=n, D=D, K=P, F=F), calls=a.calls, warmup=a.warmup)
    lib = N.lib()
    with torch.no_grad():
        code = samp.codebook.detach().t().contiguous()
        protos = dec.prototypes(code, D)
        mu, lv, offl = protos[0].reshape(D * P, F), protos[1].reshape(D * P, F), protos[2].reshape(-1)
        gen = torch.Generator("cuda").manual_seed(1)
        lw = torch.log_softmax(torch.randn(P, device="cuda", generator=gen), 0)
        # syntax_bench.py's recording: chained segments of random categories and lengths around the prototypes
        g = torch.Generator().manual_seed(2)
        parts, at = [], 0
        while at < n:
            d = min(int(torch.randint(20, D + 1, (1,), generator=g)), n - at)
            k = int(torch.randint(0, P, (1,), generator=g))
            parts.append(protos[0][:d, k] + 0.5 * torch.exp(0.5 * protos[1][:d, k]) *
                         torch.randn(d, F, generator=g).cuda())
            at += d
        frames = torch.cat(parts).contiguous()
        score, _ = ops.span_scores(frames, mu, lv, offl, lw, P, D)
        gap = torch.full((n,), float(score[torch.isfinite(score)].median()) / 100.0, device="cuda")
        del score
        tb = ops.span_table(frames, mu, lv, offl, None, P, D, False)[0]
        for form, K in (("resident", P), ("streaming", a.stream_k)):
            if K > P:
                tb = torch.cat([tb, tb[:, :, :K - P]], 2).contiguous()
            resident, threads, lds = N.c_int(-1), N.c_int(-1), N.ctypes.c_size_t(0)
            assert lib.abcd_span_chain_posterior_plan(K, D, N.ctypes.byref(resident), N.ctypes.byref(threads),
                                                      N.ctypes.byref(lds)) == 0
            lt = torch.log_softmax(torch.randn(K, K, device="cuda", generator=gen) * 2.0, 1)
            li = torch.log_softmax(torch.randn(K, device="cuda", generator=gen), 0)
            c = dict(K=K, resident=bool(resident.value), threads=threads.value, lds_bytes=int(lds.value),
                     table_bytes=8 * (n + 1) * D * K,
                     workspace_bytes=int(lib.abcd_span_chain_posterior_workspace_bytes(n, D, K)))
            for name, d_min, gp, bonus in (("tiled", 1, None, 0.0), ("gap", 5, gap, -10.0)):
                def chain():
                    return ops.span_chain_viterbi(tb, d_min, gp, bonus, lt, li, False)
                best = chain()
                vit_us = events(chain, a.calls, a.warmup)
                r = dict(d_min=d_min, seg_bonus=bonus, span_chain_viterbi_call_us=vit_us,
                         path_score=float(best[0]))
                forms = (("plain", False, False, 1.0), ("counts", True, False, 1.0), ("table", False, True, 1.0),
                         ("all", True, True, 1.0), ("plain_temperature_4", False, False, 0.25))
                for what, counts, table, scale in forms:
                    def post():
                        return ops.span_chain_posterior(tb, d_min, gp, bonus, scale, lt, li, counts, table)
                    out = post()
                    us = events(post, a.calls, a.warmup)
                    r[what] = dict(call_us=us, us_per_step=us / n, over_span_chain_viterbi=us / vit_us,
                                   log_evidence=float(out[0]), expected_segments=float(out[3][1].sum()))
                    del out
                    print(f"{form} {name} {what}: {us / 1e3:.1f} ms", file=sys.stderr, flush=True)
                c[name] = r
            res[form] = c
        res["device_status"] = int(lib.abcd_device_status())
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
