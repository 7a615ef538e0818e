#!/usr/bin/env python
"""Times time-warped segmentation (the emission plane and the frame-synchronous
programme over (category, prototype step)) on one GPU for a 60 s recording at
the c2 feature shape of bench.py: N = 15 000 frames at a 4 ms hop, K = 128
prototypes of T_proto = 200 steps, F = 129; 3 warm-up calls then 10 timed ones,
each bracketed by stream events, median, minimum and maximum reported:

  frame_costs          the plane in chunks of segment_frames_warped's default
                       (256 MiB), every chunk's operator call
  warp_segment_window  the programme over the same chunks of a plane built
                       beforehand, microseconds per frame; default moves and
                       the step move alone, tiled and with a gap
  end_to_end           plane and programme chunk by chunk, the plane freed in
                       between: what segment_frames_warped runs
  span_table + span_chain_viterbi at D = 200 on the same frames in the same
                       process: the rigid programme this one is compared with

with the two memory peaks (the plane chunk and the carried state against the
whole table) and writes one JSON document to --out (default
profiles/warpseg_bench.json) and to stdout.  Nothing outside the repository is
read.  Run it under a time limit of its own:

    timeout -k 10 600 python scripts/warpseg_bench.py [--calls 10] [--warmup 3] [--out PATH]
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


def timed(fn, calls, warmup):
    """dict(median, min, max) microseconds of fn() by stream events"""
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
    return dict(median_us=statistics.median(ev), min_us=min(ev), max_us=max(ev))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "warpseg_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("warpseg_bench.py needs a GPU: timings are not taken on the CPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import bench
    from modules import _native as N, ops, segmentation
    cfg = bench.CONFIGS["c2"]
    step = bench.build(cfg, "cuda")
    dec, samp = step.decoder.eval(), step.sampler.eval()
    n, T, F, K = a.frames, a.steps, cfg["F"], cfg["K"]
    res = dict(shape=dict(N=n, K=K, T_proto=T, F=F), calls=a.calls, warmup=a.warmup)
    lib = N.lib()
    with torch.no_grad():
        code = samp.codebook.detach().t().contiguous()
        protos = dec.prototypes(code, T)
        mu, lv, offl = protos[0].reshape(T * K, F), protos[1].reshape(T * K, F), protos[2].reshape(-1)
        gen = torch.Generator("cuda").manual_seed(1)
        # a recording around the prototypes: chained segments of random categories, each at a tempo of its own
        g = torch.Generator().manual_seed(2)
        parts, at = [], 0
        while at < n:
            d = min(int(torch.randint(20, T + 1, (1,), generator=g)), n - at)
            k = int(torch.randint(0, K, (1,), generator=g))
            tempo = float(torch.rand(1, generator=g)) * 0.6 + 0.7
            s = torch.clamp((torch.arange(d) * tempo).long(), max=T - 1).cuda()
            parts.append(protos[0][s, k] + 0.5 * torch.exp(0.5 * protos[1][s, k]) * torch.randn(d, F, generator=g).cuda())
            at += d
        frames = torch.cat(parts).contiguous()
        lt = torch.log_softmax(torch.randn(K, K, device="cuda", generator=gen) * 2.0, 1)
        li = torch.log_softmax(torch.randn(K, device="cuda", generator=gen), 0)
        chunk = segmentation.default_chunk_frames(T, K)
        chunks = [(n0, min(n, n0 + chunk)) for n0 in range(0, n, chunk)]
        resident, threads, lds = N.c_int(-1), N.c_int(-1), N.ctypes.c_size_t(0)
        assert lib.abcd_warp_segment_plan(K, T, N.ctypes.byref(resident), N.ctypes.byref(threads),
                                          N.ctypes.byref(lds)) == 0
        state_bytes = int(lib.abcd_warp_segment_workspace_bytes(n, K, T))
        res["plan"] = dict(resident=bool(resident.value), threads=threads.value, lds_bytes=int(lds.value),
                           chunk_frames=chunk, chunks=len(chunks))
        res["memory"] = dict(plane_chunk_bytes=4 * min(chunk, n) * T * K, state_bytes=state_bytes,
                             warped_peak_bytes=4 * min(chunk, n) * T * K + state_bytes,
                             rigid_table_bytes=8 * (n + 1) * T * K,
                             rigid_workspace_bytes=int(lib.abcd_span_chain_workspace_bytes(n, T, K)))

        def costs():
            for n0, n1 in chunks:
                ops.frame_costs(frames, mu, lv, K, n0, n1)
        r = timed(costs, a.calls, a.warmup)
        r["us_per_frame"] = r["median_us"] / n
        res["frame_costs"] = r

        plane = torch.cat([ops.frame_costs(frames, mu, lv, K, n0, n1) for n0, n1 in chunks])
        state = ops.warp_segment_state(n, K, T, "cuda")
        gap = torch.full((n,), -float(plane.min(1).values.median()) - 1.0, device="cuda")
        res["warp_segment_window"] = {}
        for name, moves, gp, bonus in (("default_tiled", ops.DEFAULT_LOG_MOVES, None, 0.0),
                                       ("default_gap", ops.DEFAULT_LOG_MOVES, gap, -10.0),
                                       ("step_only_tiled", ops.IDENTITY_LOG_MOVES, None, 0.0)):
            def prog():
                out = None
                for n0, n1 in chunks:
                    out = ops.warp_segment_window(plane[n0:n1], n0, n1, n, K, offl, list(moves), None, gp, bonus, lt, li,
                                                  0, state, None)
                return out
            out = prog()
            r = timed(prog, a.calls, a.warmup)
            r.update(us_per_frame=r["median_us"] / n, segments=int(out[1]), path_score=float(out[0]),
                     cells_per_us=n * K * T / r["median_us"])
            res["warp_segment_window"][name] = r
        del plane

        def whole():
            out = None
            for n0, n1 in chunks:
                cost = ops.frame_costs(frames, mu, lv, K, n0, n1)
                out = ops.warp_segment_window(cost, n0, n1, n, K, offl, list(ops.DEFAULT_LOG_MOVES), None, None, 0.0, lt,
                                              li, 0, state, None)
                del cost
            return out
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = timed(whole, a.calls, a.warmup)
        r.update(us_per_frame=r["median_us"] / n, peak_allocated_bytes=int(torch.cuda.max_memory_allocated() - base))
        res["end_to_end"] = r

        def table():
            return ops.span_table(frames, mu, lv, offl, None, K, T, False)
        r = timed(table, a.calls, a.warmup)
        res["span_table"] = r
        tb = table()[0]

        def chain():
            return ops.span_chain_viterbi(tb, 1, None, 0.0, lt, li, False)
        out = chain()
        r = timed(chain, a.calls, a.warmup)
        r.update(us_per_step=r["median_us"] / n, segments=int(out[1]), path_score=float(out[0]))
        res["span_chain_viterbi"] = r
        rigid = res["span_table"]["median_us"] + r["median_us"]
        res["warped_over_rigid"] = res["end_to_end"]["median_us"] / rigid
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
