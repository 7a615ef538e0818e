#!/usr/bin/env python
"""Times the category-sequence HMM (abcd_chain_posterior: forward-backward,
expected counts and Viterbi in one call) on one GPU:

  K = 128    N = 20 000 segments in 100 sequences of unequal length (resident form)
  K = 1024   N = 2 000 segments in 20 sequences of unequal length (streaming form)

each with 3 warm-up calls then 10 timed ones, the whole call (workspace,
offset-table copy, every launch) bracketed by stream events; abcd_chain_plan
says which form ran.  Beside it, the same recurrences written as a per-step
torch loop on the same GPU (fp32, log domain, the sequences padded to the
longest and batched, counts summed in fp64): the only baseline there is.  One
JSON document with the medians goes to --out (default
profiles/chain_bench.json) and to stdout.

    python scripts/chain_bench.py [--calls 10] [--warmup 3] [--out PATH]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((128, 20000, 100), (1024, 2000, 20))


def draw_lengths(N, S, g):
    """S unequal lengths summing to N (between a quarter of and twice the mean)."""
    w = g.uniform(0.25, 2.0, size=S)
    lens = np.maximum(1, np.floor(w / w.sum() * N)).astype(np.int64)
    lens[np.argmax(lens)] += N - lens.sum()
    assert lens.sum() == N and lens.min() >= 1
    return lens


def event_times(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return out


def torch_loop(score, lens, lt, li):
    """The same outputs from per-step torch calls: score S x Tmax x K (padded),
    lens S (device).  Returns (log_evidence, gamma S x Tmax x K, counts K x K
    fp64, path S x Tmax)."""
    S, Tmax, K = score.shape
    alive = [(lens > t)[:, None] for t in range(Tmax)]
    alpha = li[None] + score[:, 0]
    alphas = [alpha]
    for t in range(1, Tmax):
        new = score[:, t] + torch.logsumexp(alpha[:, :, None] + lt[None], 1)
        alpha = torch.where(alive[t], new, alpha)
        alphas.append(alpha)
    ev = torch.logsumexp(alpha, 1)
    beta = torch.zeros_like(alpha)
    counts = torch.zeros(K, K, dtype=torch.float64, device=score.device)
    gamma = torch.empty_like(score)
    gamma[:, Tmax - 1] = torch.exp(alphas[Tmax - 1] + beta - ev[:, None])
    for t in range(Tmax - 2, -1, -1):
        w = score[:, t + 1] + beta
        inner = lt[None] + w[:, None, :]
        xi = torch.exp(alphas[t][:, :, None] + inner - ev[:, None, None])
        counts += (xi * alive[t + 1][:, :, None]).sum(0).double()
        beta = torch.where(alive[t + 1], torch.logsumexp(inner, 2), beta)
        gamma[:, t] = torch.exp(alphas[t] + beta - ev[:, None])
    delta = li[None] + score[:, 0]
    bps = []
    for t in range(1, Tmax):
        m, arg = (delta[:, :, None] + lt[None]).max(1)
        delta = torch.where(alive[t], score[:, t] + m, delta)
        bps.append(torch.where(alive[t], arg, torch.arange(K, device=score.device)[None]))
    path = torch.empty(S, Tmax, dtype=torch.int64, device=score.device)
    cur = delta.argmax(1)
    path[:, Tmax - 1] = cur
    for t in range(Tmax - 1, 0, -1):
        cur = bps[t - 1].gather(1, cur[:, None])[:, 0]
        path[:, t - 1] = cur
    return ev, gamma, counts, path


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "chain_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("chain_bench.py needs a GPU: timings are not taken on the CPU")
    from modules import _native as N, ops
    res = dict(calls=a.calls, warmup=a.warmup)
    for K, n, S in SHAPES:
        g = np.random.default_rng(K)
        lens = draw_lengths(n, S, g)
        seq_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        tg = torch.Generator("cuda").manual_seed(K)
        score = -10.0 * torch.rand(n, K, device="cuda", generator=tg)
        score[torch.arange(n, device="cuda"), torch.randint(0, K, (n,), device="cuda", generator=tg)] = 0.0
        lt = torch.log_softmax(3.0 * torch.randn(K, K, device="cuda", generator=tg), 1)
        li = torch.log_softmax(torch.randn(K, device="cuda", generator=tg), 0)
        resident, wg = ops.chain_plan(K, S)
        r = dict(K=K, N=n, S=S, longest=int(lens.max()), shortest=int(lens.min()), resident=resident, workgroups=wg,
                 workspace_bytes=int(N.lib().abcd_chain_workspace_bytes(n, S, K, ops.CHAIN_ALL)))
        with torch.no_grad():
            full = event_times(lambda: ops.chain_posterior(score, seq_off, lt, li, ops.CHAIN_ALL), a.calls, a.warmup)
            vit = event_times(lambda: ops.chain_posterior(score, seq_off, lt, li, ops.CHAIN_PATH), a.calls, a.warmup)
            evid = event_times(lambda: ops.chain_posterior(score, seq_off, lt, li, ops.CHAIN_EVIDENCE), a.calls,
                               a.warmup)
            pad = torch.zeros(S, int(lens.max()), K, device="cuda")
            for s in range(S):
                pad[s, :lens[s]] = score[seq_off[s]:seq_off[s + 1]]
            lens_d = torch.from_numpy(lens).cuda()
            loop = event_times(lambda: torch_loop(pad, lens_d, lt, li), a.calls, a.warmup)
            # the two routes compute the same thing
            ev, gamma, path, _, tc, _ = ops.chain_posterior(score, seq_off, lt, li, ops.CHAIN_ALL)
            ev2, gamma2, tc2, path2 = torch_loop(pad, lens_d, lt, li)
            r["evidence_rel_diff"] = float(((ev - ev2.double()).abs() / ev.abs()).max())
            r["counts_abs_diff"] = float((tc - tc2).abs().max())
            s0 = int(np.argmax(lens))
            r["gamma_abs_diff_longest"] = float((gamma[seq_off[s0]:seq_off[s0 + 1]] - gamma2[s0, :lens[s0]]).abs().max())
            r["path_agreement_longest"] = float((path[seq_off[s0]:seq_off[s0 + 1]].long() == path2[s0, :lens[s0]])
                                                .double().mean())
        r["chain_call_us"] = statistics.median(full)
        r["chain_call_us_min_max"] = [min(full), max(full)]
        r["viterbi_only_call_us"] = statistics.median(vit)
        r["evidence_only_call_us"] = statistics.median(evid)
        r["torch_loop_us"] = statistics.median(loop)
        r["torch_loop_us_min_max"] = [min(loop), max(loop)]
        r["torch_loop_over_chain"] = r["torch_loop_us"] / r["chain_call_us"]
        res[f"K{K}"] = r
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
