#!/usr/bin/env python
"""Times the segmentation posteriors on one GPU at segment_bench.py's shape (a
60 s recording at the c2 feature shape of bench.py: N = 15 000 frames, D = 200,
P = 128 prototypes, F = 129), 3 warm-up calls then 10 timed ones, each
bracketed by stream events around the operator, medians:

  span_evidence   with want_best (the log-sum, the maximum and its category in
                  one pass) and without, against span_scores in the same run,
                  and the ratios
  span_posterior  without the table (both sweeps and the per-frame posteriors,
                  one launch), on the sum table, tiled and with a gap and a
                  bonus, against span_viterbi on the best table in the same
                  run, the ratios and microseconds per step
  span table      span_posterior with the table minus without it: the
                  many-workgroup kernel has no entry point of its own, so its
                  time is that difference of medians

and writes one JSON document to --out (default profiles/spanpost_bench.json)
and to stdout.

    python scripts/spanpost_bench.py [--calls 10] [--warmup 3] [--date D] [--parent_commit C] [--out PATH]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15000)
    ap.add_argument("--max_length", type=int, default=200)
    ap.add_argument("--date", type=str, default=None)
    ap.add_argument("--parent_commit", type=str, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "spanpost_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("spanpost_bench.py needs a GPU: timings are not taken on the CPU")
    import bench
    from modules import _native as N, ops
    from segment_bench import events
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec, samp = step.decoder.eval(), step.sampler.eval()
    n, D, F, P = a.frames, a.max_length, cfg["F"], cfg["K"]
    res = dict(shape=dict(N=n, D=D, P=P, F=F), calls=a.calls, warmup=a.warmup, date=a.date,
               parent_commit=a.parent_commit)
    with torch.no_grad():
        code = samp.codebook.detach().t().contiguous()
        protos = dec.prototypes(code, D)
        mu, lv, offl = protos[0].reshape(D * P, F), protos[1].reshape(D * P, F), protos[2].reshape(-1)
        lw = torch.log_softmax(torch.randn(P, device="cuda", generator=torch.Generator("cuda").manual_seed(1)), 0)
        g = torch.Generator().manual_seed(2)            # segment_bench.py's recording
        parts, at = [], 0
        while at < n:
            d = min(int(torch.randint(20, D + 1, (1,), generator=g)), n - at)
            k = int(torch.randint(0, P, (1,), generator=g))
            parts.append(protos[0][:d, k] + 0.5 * torch.exp(0.5 * protos[1][:d, k]) *
                         torch.randn(d, F, generator=g).cuda())
            at += d
        frames = torch.cat(parts).contiguous()

        def scores():
            return ops.span_scores(frames, mu, lv, offl, lw, P, D)

        def evidence(best=True):
            return ops.span_evidence(frames, mu, lv, offl, lw, P, D, best)
        score, cat = scores()
        lse, score2, cat2 = evidence()
        r = dict(best_outputs_equal=bool(torch.equal(score.view(torch.int64), score2.view(torch.int64))
                                         and torch.equal(cat, cat2)))
        fin = torch.isfinite(score)
        r["largest_sum_over_maximum"] = float((lse[fin] - score[fin]).max())
        # interleaved, so that a drift of the clocks falls on both alike
        us = {k: [] for k in ("scores", "evidence_best", "evidence")}
        for _ in range(3):
            us["scores"].append(events(scores, a.calls, a.warmup))
            us["evidence_best"].append(events(evidence, a.calls, a.warmup))
            us["evidence"].append(events(lambda: evidence(False), a.calls, a.warmup))
        r["span_scores_call_us"] = sorted(us["scores"])[1]
        r["span_evidence_best_call_us"] = sorted(us["evidence_best"])[1]
        r["span_evidence_call_us"] = sorted(us["evidence"])[1]
        r["rounds_us"] = us
        r["evidence_best_over_scores"] = r["span_evidence_best_call_us"] / r["span_scores_call_us"]
        r["evidence_over_scores"] = r["span_evidence_call_us"] / r["span_scores_call_us"]
        res["span_evidence"] = r
        v = {}
        gap = torch.full((n,), float(score[fin].median()) / 100.0, device="cuda")
        for name, d_min, gp, bonus in (("tiled", 1, None, 0.0), ("gap", 5, gap, -10.0)):
            def vit():
                return ops.span_viterbi(score, cat, d_min, gp, bonus, False)

            def post(table=False):
                return ops.span_posterior(lse, d_min, gp, bonus, table)
            out, path = post(True), vit()
            t_vit, t_post = events(vit, a.calls, a.warmup), events(post, a.calls, a.warmup)
            t_table = events(lambda: post(True), a.calls, a.warmup)
            v[name] = dict(d_min=d_min, seg_bonus=bonus, span_viterbi_call_us=t_vit, span_posterior_call_us=t_post,
                           posterior_over_viterbi=t_post / t_vit, us_per_step=t_post / n,
                           span_posterior_with_table_call_us=t_table, table_kernel_us=t_table - t_post,
                           log_evidence=float(out[0]), path_score=float(path[0]),
                           expected_segments=float(out[2][1].sum()), segments=int(path[1]))
        v["workspace_bytes"] = int(N.lib().abcd_span_posterior_workspace_bytes(n, D))
        res["span_posterior"] = v
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
