#!/usr/bin/env python
"""Times syntax-aware segmentation with the table in windows
on one GPU, next to the one-shot path in the same run, at the c2 feature shape
of bench.py (D = 200, K = 128 prototypes, F = 129); warm-up calls then timed
ones, each bracketed by stream events, medians reported:

  flagship   N = 15 000: the one-shot path (span_table + span_chain_viterbi)
             and the windowed path (per window span_table on the slice +
             span_chain_viterbi_window) at W in --windows, without the second
             sweep: total, the table's share and the programme's (events around
             every operator of one more pass, summed), microseconds per step,
             the peak of torch.cuda.max_memory_allocated over the call, and the
             ratio to the one-shot total (the bar: at most 1.10 at W = 1024);
             segment_frames end to end with and without window_frames = 1024
             (the second sweep for context_free_category included)
  long       N = 150 000, on which the one-shot operator raises: the windowed
             path at W = 1024, its time, its peak memory and the formula's 8 (W
             + D + 32) D K table bytes plus the state's 24 (N + 1) K

and writes one JSON document to --out (default profiles/stream_bench.json) and
to stdout.  Nothing outside the repository is read.  Run it under a time limit
of its own:

    timeout -k 10 900 python scripts/stream_bench.py [--calls 10] [--warmup 3] [--date D] [--parent_commit C]
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


def recording(protos, n, D, F, P, seed):
    """A recording around the prototypes: chained segments of random categories and lengths."""
    g = torch.Generator().manual_seed(seed)
    parts, at = [], 0
    while at < n:
        d = min(int(torch.randint(20, D + 1, (1,), generator=g)), n - at)
        k = int(torch.randint(0, P, (1,), generator=g))
        parts.append(protos[0][:d, k] + 0.5 * torch.exp(0.5 * protos[1][:d, k]) * torch.randn(d, F, generator=g).cuda())
        at += d
    return torch.cat(parts).contiguous()


def peak_of(fn):
    """(fn's result, peak bytes torch allocated during fn beyond what was allocated before it)"""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, int(torch.cuda.max_memory_allocated() - before)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15000)
    ap.add_argument("--long_frames", type=int, default=150000)
    ap.add_argument("--max_length", type=int, default=200)
    ap.add_argument("--windows", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--date", type=str, default=None)
    ap.add_argument("--parent_commit", type=str, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "stream_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench.py needs a GPU: timings are not taken on the CPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import bench
    from modules import _native as N, ops, segmentation
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec, samp = step.decoder.eval(), step.sampler.eval()
    D, F, P = a.max_length, cfg["F"], cfg["K"]
    res = dict(what="scripts/stream_bench.py on one MI355X: medians of stream-event timings in microseconds",
               date=a.date, parent_commit=a.parent_commit, calls=a.calls, warmup=a.warmup)
    lib = N.lib()
    with torch.no_grad():
        code = samp.codebook.detach().t().contiguous()
        protos = dec.prototypes(code, D)
        mu, lv, offl = protos[0].reshape(D * P, F), protos[1].reshape(D * P, F), protos[2].reshape(-1)
        gen = torch.Generator("cuda").manual_seed(1)
        lt = torch.log_softmax(torch.randn(P, P, device="cuda", generator=gen) * 2.0, 1)
        li = torch.log_softmax(torch.randn(P, device="cuda", generator=gen), 0)

        def one_shot(frames):
            tb = ops.span_table(frames, mu, lv, offl, None, P, D, False)[0]
            return ops.span_chain_viterbi(tb, 1, None, 0.0, lt, li, False)

        def windowed(frames, W, marks=None):
            n = int(frames.shape[0])
            state = ops.span_chain_window_state(n, D, P, frames.device)
            out = None
            for row0, n0, n1 in segmentation.plan_windows(n, D, W):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if marks is not None else None
                if ev:
                    ev[0].record()
                tb = ops.span_table(frames[row0:n1], mu, lv, offl, None, P, D, False)[0]
                if ev:
                    ev[1].record()
                out = ops.span_chain_viterbi_window(tb, row0, n0, n1, n, 1, None, 0.0, lt, li, state, None)
                if ev:
                    ev[2].record()
                    marks.append(ev)
                del tb
            return out

        def shares(frames, W):
            """(table us, programme us, the slowest window's us) of one more pass, events around every operator"""
            marks = []
            windowed(frames, W, marks)
            torch.cuda.synchronize()
            t = [m[0].elapsed_time(m[1]) * 1e3 for m in marks]
            p = [m[1].elapsed_time(m[2]) * 1e3 for m in marks]
            return sum(t), sum(p), max(x + y for x, y in zip(t, p))

        # ---- 1. the flagship shape
        n = a.frames
        frames = recording(protos, n, D, F, P, 2)
        r = dict(shape=dict(N=n, D=D, K=P, F=F), table_bytes=8 * (n + 1) * D * P,
                 one_shot_workspace_bytes=int(lib.abcd_span_chain_workspace_bytes(n, D, P)),
                 window_state_bytes=int(lib.abcd_span_chain_window_workspace_bytes(n, D, P)))
        ref, peak = peak_of(lambda: one_shot(frames))
        tab_us = events(lambda: ops.span_table(frames, mu, lv, offl, None, P, D, False), a.calls, a.warmup)
        tot_us = events(lambda: one_shot(frames), a.calls, a.warmup)
        r["one_shot"] = dict(total_us=tot_us, table_us=tab_us, programme_us=tot_us - tab_us,
                             us_per_step=(tot_us - tab_us) / n, peak_bytes=peak, segments=int(ref[1]),
                             path_score=float(ref[0]))
        r["windowed"] = {}
        for W in a.windows:
            out, peak = peak_of(lambda: windowed(frames, W))
            same = bool(float(out[0]) == float(ref[0]) and int(out[1]) == int(ref[1])
                        and all(torch.equal(x, y) for x, y in zip(out[2:], ref[2:7])))
            us = events(lambda: windowed(frames, W), a.calls, a.warmup)
            t_us, p_us, worst = shares(frames, W)
            plan = segmentation.plan_windows(n, D, W)
            r["windowed"][str(W)] = dict(
                windows=len(plan), total_us=us, table_us=t_us, programme_us=p_us, us_per_step=p_us / n,
                slowest_window_us=worst, peak_bytes=peak,
                formula_table_bytes=max(segmentation.window_table_bytes(w, D, P) for w in plan),
                over_one_shot=us / tot_us, equal_to_one_shot=same)
        if "1024" in r["windowed"]:
            r["bar"] = dict(what="windowed total at W = 1024 over the one-shot total of the same run, at most 1.10",
                            ratio=r["windowed"]["1024"]["over_one_shot"],
                            met=bool(r["windowed"]["1024"]["over_one_shot"] <= 1.10))
        e1 = events(lambda: segmentation.segment_frames(dec, protos, frames, D, transitions=(lt, li)), a.calls, a.warmup)
        e2 = events(lambda: segmentation.segment_frames(dec, protos, frames, D, transitions=(lt, li), window_frames=1024),
                    a.calls, a.warmup)
        r["segment_frames"] = dict(one_shot_us=e1, window_frames_1024_us=e2, ratio=e2 / e1)
        res["flagship"] = r
        del frames, ref

        # ---- 2. a recording beyond the one-shot limit
        n, W = a.long_frames, 1024
        frames = recording(protos, n, D, F, P, 3)
        q = dict(shape=dict(N=n, D=D, K=P, F=F), W=W, whole_table_bytes=8 * (n + 1) * D * P,
                 state_bytes=int(lib.abcd_span_chain_window_workspace_bytes(n, D, P)),
                 formula_table_bytes=8 * (W + D + 32) * D * P)
        try:
            one_shot(frames)
            q["one_shot"] = "completed"
        except N.HipError as e:
            q["one_shot"] = "HipError: " + str(e)
        out, peak = peak_of(lambda: windowed(frames, W))
        q.update(segments=int(out[1]), path_score=float(out[0]), peak_bytes=peak,
                 peak_over_formula=peak / (q["formula_table_bytes"] + q["state_bytes"]))
        q["total_us"] = events(lambda: windowed(frames, W), max(a.calls // 3, 1), 1)
        t_us, p_us, worst = shares(frames, W)
        q.update(table_us=t_us, programme_us=p_us, us_per_step=p_us / n, slowest_window_us=worst)
        got, peak = peak_of(lambda: segmentation.segment_frames(dec, protos, frames, D, transitions=(lt, li),
                                                                window_frames=W))
        q["segment_frames"] = dict(segments=int(got["onset"].numel()), path_score=float(got["path_score"]),
                                   peak_bytes=peak)
        res["long"] = q
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
