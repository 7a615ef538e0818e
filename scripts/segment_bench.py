#!/usr/bin/env python
"""Times segmentation (span scores and the semi-Markov programme) on one GPU
for a 60 s recording at the c2 feature shape of bench.py: N = 15 000 frames at
a 4 ms hop, D = 200, P = 128 prototypes, F = 129 (4.95e10 squared-difference
terms), 3 warm-up calls then 10 timed ones, each bracketed by stream events
around the operator:

  span_scores    the whole operator (workspace, O table, fill, tile kernel);
                 its terms per second next to pair_nll's at P = 128 in the
                 same run (the c2 batch of bench.py, the library's live timing
                 id 13) and their ratio
  span_viterbi   the whole operator, and microseconds per step
  prior route    at --small_n frames, where it fits: ops.pairwise_nll on all
                 cut-out spans as one packed batch with one-hot end targets
                 (the batch is built outside the timed region), against
                 span_scores at the same N, and the speed-up

and writes one JSON document to --out (default profiles/segment_bench.json)
and to stdout.

    python scripts/segment_bench.py [--calls 10] [--warmup 3] [--small_n 1024] [--out PATH]
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


def events(fn, calls, warmup):
    """median microseconds of fn() by stream events"""
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
    return statistics.median(ev)


def all_spans(frames, D):
    """Every cut-out span of the recording as one packed batch, longest first:
    (data L x F, batch_sizes T, one-hot end targets L), built on the device."""
    n = frames.shape[0]
    dev = frames.device
    s = torch.arange(n, device=dev)[:, None].expand(n, D)
    d = torch.arange(1, D + 1, device=dev)[None, :].expand(n, D)
    ok = s + d <= n
    s, d = s[ok], d[ok]
    order = torch.argsort(d, descending=True, stable=True)
    s, d = s[order], d[order]
    rows, y, bs = [], [], []
    for t in range(int(d.max())):
        live = d > t
        rows.append(s[live] + t)
        y.append((d[live] == t + 1).float())
        bs.append(int(live.sum()))
    return frames[torch.cat(rows)].contiguous(), torch.tensor(bs, dtype=torch.int64), torch.cat(y)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15000)
    ap.add_argument("--max_length", type=int, default=200)
    ap.add_argument("--small_n", type=int, default=1024)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "segment_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("segment_bench.py needs a GPU: timings are not taken on the CPU")
    import bench
    from modules import _native as N, ops
    from score_bench import timed
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec, samp = step.decoder.eval(), step.sampler.eval()
    n, D, F, P = a.frames, a.max_length, cfg["F"], cfg["K"]
    res = dict(shape=dict(N=n, D=D, P=P, F=F), calls=a.calls, warmup=a.warmup)
    with torch.no_grad():
        code = samp.codebook.detach().t().contiguous()
        protos = dec.prototypes(code, D)
        mu, lv, offl = protos[0].reshape(D * P, F), protos[1].reshape(D * P, F), protos[2].reshape(-1)
        lw = torch.log_softmax(torch.randn(P, device="cuda", generator=torch.Generator("cuda").manual_seed(1)), 0)
        # a recording around the prototypes: chained segments of random categories and lengths
        g = torch.Generator().manual_seed(2)
        parts, at = [], 0
        while at < n:
            d = min(int(torch.randint(20, D + 1, (1,), generator=g)), n - at)
            k = int(torch.randint(0, P, (1,), generator=g))
            parts.append(protos[0][:d, k] + 0.5 * torch.exp(0.5 * protos[1][:d, k]) *
                         torch.randn(d, F, generator=g).cuda())
            at += d
        frames = torch.cat(parts).contiguous()

        def spans(x=frames):
            return ops.span_scores(x, mu, lv, offl, lw, P, D)
        score, cat = spans()
        terms = int(((torch.arange(n) + 1).clamp(max=D)).sum()) * P * F  # every (frame, step, prototype) once
        r = dict(terms=terms)
        r["span_scores_call_us"] = events(spans, a.calls, a.warmup)
        r["span_scores_terms_per_s"] = terms / (r["span_scores_call_us"] * 1e-6)
        r["workspace_bytes"] = int(N.lib().abcd_span_scores_workspace_bytes(n, D, P))
        # pair_nll at P = 128 on the c2 batch, in the same run
        batch = bench.make_batch(cfg, 0, "cuda")
        T = batch["T"]
        pp = dec.prototypes(code, T)
        pmu, plv, pol = pp[0].reshape(T * P, F), pp[1].reshape(T * P, F), pp[2].reshape(-1)

        def pair():
            return ops.pairwise_nll(batch["data"], batch["batch_sizes"], batch["is_offset"], pmu, plv, pol, P, F)
        r["pair_nll_call_us"], r["pair_nll_kernel_us"] = timed(pair, a.calls, a.warmup, N.PAIR_NLL)
        r["pair_nll_terms"] = batch["L"] * P * F
        r["pair_nll_terms_per_s"] = r["pair_nll_terms"] / (r["pair_nll_kernel_us"] * 1e-6)
        r["span_over_pair_terms_per_s"] = r["span_scores_terms_per_s"] / r["pair_nll_terms_per_s"]
        res["span_scores"] = r
        # the dynamic programme on that table: tiled, and with a gap and a bonus
        v = {}
        gap = torch.full((n,), float(score[torch.isfinite(score)].median()) / 100.0, device="cuda")
        for name, d_min, gp, bonus in (("tiled", 1, None, 0.0), ("gap", 5, gap, -10.0)):
            def vit():
                return ops.span_viterbi(score, cat, d_min, gp, bonus, False)
            out = vit()
            us = events(vit, a.calls, a.warmup)
            v[name] = dict(d_min=d_min, seg_bonus=bonus, call_us=us, us_per_step=us / n, segments=int(out[1]),
                           path_score=float(out[0]))
        v["workspace_bytes"] = int(N.lib().abcd_span_viterbi_workspace_bytes(n, D))
        res["span_viterbi"] = v
        # the only prior route, where it fits
        m = min(a.small_n, n)
        small = frames[:m].contiguous()
        data, bs, y = all_spans(small, D)
        smu, slv, sol = mu, lv, offl

        def prior():
            return ops.pairwise_nll(data, bs, y, smu, slv, sol, P, F)
        q = dict(N=m, spans=int(bs[0]), rows=int(data.shape[0]), terms=int(data.shape[0]) * P * F)
        q["pairwise_route_call_us"] = events(prior, a.calls, a.warmup)
        q["span_scores_call_us"] = events(lambda: spans(small), a.calls, a.warmup)
        q["speed_up"] = q["pairwise_route_call_us"] / q["span_scores_call_us"]
        q["pairwise_route_workspace_bytes"] = int(N.lib().abcd_pairwise_nll_workspace_bytes(int(bs.numel()),
                                                                                             int(bs[0]), P))
        res["prior_route"] = q
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
