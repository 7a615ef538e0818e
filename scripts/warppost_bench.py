#!/usr/bin/env python
"""Times the posteriors under the time-warped cut (the forward-backward over
(frame, category, prototype step)) on one GPU for a 60 s
recording at the c2 feature shape of bench.py: N = 15 000 frames at a 4 ms hop,
K = 128 prototypes of T_proto = 200 steps, F = 129; 3 warm-up calls then 10
timed ones, each bracketed by stream events, median, minimum and maximum
reported:

  forward              warp_posterior_forward over the chunks of a plane built
                       beforehand (segment_warp_posteriors' default chunks),
                       without and with the aH plane kept
  backward             warp_posterior_backward over the same chunks, descending:
                       without counts, with the bigram counts, with the move
                       counts (which read the aH plane)
  end_to_end           segmentation.segment_warp_posteriors: the plane chunk by
                       chunk twice and both sweeps, without counts and with all
  warp_segment_window  the best-path programme on the same plane in the same
                       process: the yardstick

with the peak allocation of each end-to-end form, and writes one JSON document
to --out (default profiles/warppost_bench.json) and to stdout.  Nothing outside
the repository is read.  Run it under a time limit of its own:

    timeout -k 10 900 python scripts/warppost_bench.py [--calls 10] [--warmup 3] [--out PATH]
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

from warpseg_bench import timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "warppost_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("warppost_bench.py needs a GPU: timings are not taken on the CPU")
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
        # warpseg_bench.py's recording: chained segments of random categories, each at a tempo of its own
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
        assert lib.abcd_warp_posterior_plan(K, T, N.ctypes.byref(resident), N.ctypes.byref(threads),
                                            N.ctypes.byref(lds)) == 0
        state_bytes = int(lib.abcd_warp_posterior_workspace_bytes(n, K, T))
        res["plan"] = dict(resident=bool(resident.value), threads=threads.value, lds_bytes=int(lds.value),
                           chunk_frames=chunk, chunks=len(chunks))
        res["memory"] = dict(plane_chunk_bytes=4 * min(chunk, n) * T * K, state_bytes=state_bytes,
                             alpha_plane_bytes=8 * n * K * T)
        moves = list(ops.DEFAULT_LOG_MOVES)
        plane = torch.cat([ops.frame_costs(frames, mu, lv, K, n0, n1) for n0, n1 in chunks])
        state = ops.warp_posterior_state(n, K, T, "cuda")
        alpha = torch.empty(n, K * T, dtype=torch.float64, device="cuda")
        args = (n, K, offl, moves, None, None, 0.0, 1.0, lt, li, 0, state)

        def forward(keep):
            lz = None
            for n0, n1 in chunks:
                lz = ops.warp_posterior_forward(plane[n0:n1], n0, n1, *args, alpha[n0:n1] if keep else None)
            return lz

        res["forward"] = {}
        for name, keep in (("plain", False), ("keeping_alpha", True)):
            r = timed(lambda: forward(keep), a.calls, a.warmup)
            r.update(us_per_frame=r["median_us"] / n, cells_per_us=n * K * T / r["median_us"])
            res["forward"][name] = r
        res["log_evidence"] = float(forward(True))

        def backward(counts, mv):
            # the status word is read once per chunk: that synchronisation is part of the operator
            out = None
            for n0, n1 in reversed(chunks):
                out = ops.warp_posterior_backward(plane[n0:n1], n0, n1, *args, alpha[n0:n1] if mv else None, counts, mv)
            return out

        res["backward"] = {}
        for name, counts, mv in (("no_counts", False, False), ("bigram_counts", True, False),
                                 ("move_counts", False, True), ("all_counts", True, True)):
            out = backward(counts, mv)
            r = timed(lambda: backward(counts, mv), a.calls, a.warmup)
            r.update(us_per_frame=r["median_us"] / n, cells_per_us=n * K * T / r["median_us"],
                     expected_segments=float(out[0][1].sum()))
            if mv:
                r["move_counts"] = out[4].sum(0).tolist()
            res["backward"][name] = r
        del alpha

        wstate = ops.warp_segment_state(n, K, T, "cuda")

        def viterbi():
            out = None
            for n0, n1 in chunks:
                out = ops.warp_segment_window(plane[n0:n1], n0, n1, n, K, offl, moves, None, None, 0.0, lt, li, 0,
                                              wstate, None)
            return out
        out = viterbi()
        r = timed(viterbi, a.calls, a.warmup)
        r.update(us_per_frame=r["median_us"] / n, segments=int(out[1]), path_score=float(out[0]))
        res["warp_segment_window"] = r
        del plane, wstate, state

        res["end_to_end"] = {}
        for name, kw in (("no_counts", {}), ("all_counts", dict(want_counts=True, want_moves=True))):
            def whole():
                return segmentation.segment_warp_posteriors(dec, protos, frames, T, transitions=(lt, li), **kw)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            r = timed(whole, a.calls, a.warmup)
            r.update(us_per_frame=r["median_us"] / n, peak_allocated_bytes=int(torch.cuda.max_memory_allocated() - base))
            res["end_to_end"][name] = r
        vit = res["warp_segment_window"]["median_us"]
        res["derived"] = dict(
            forward_over_viterbi=res["forward"]["plain"]["median_us"] / vit,
            backward_over_viterbi=res["backward"]["no_counts"]["median_us"] / vit,
            sweeps_over_viterbi=(res["forward"]["plain"]["median_us"] + res["backward"]["no_counts"]["median_us"]) / vit,
            sweeps_all_counts_over_viterbi=(res["forward"]["keeping_alpha"]["median_us"] +
                                            res["backward"]["all_counts"]["median_us"]) / vit)
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
