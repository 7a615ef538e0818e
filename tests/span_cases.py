"""Cases and the float64 references of segmentation: every span of an uncut
recording against every category prototype (``abcd_span_scores``) and the
semi-Markov dynamic programme over them (``abcd_span_viterbi``,
``modules.segmentation``, ``segment.py``).

The prototypes are the time-major rectangle of ``pairwise_cases``.  With the
numpy float64 reference on the SAME fp32 inputs,

    e(n, t, p) = 0.5 sum_f (log 2pi + lv[t,p,f] + (x[n,f] - mu[t,p,f])^2 e^-lv[t,p,f])
    E[s, p, d] = sum_{t < d} e(s + t, t, p)
    O[p, d]    = sum_{t < d - 1} sp(o[t,p]) + sp(-o[d-1,p]),  sp(v) = max(v,0) + log1p(e^-|v|)
    S[s, p, d] = log_weight[p] - E[s,p,d] - O[p,d]

errors of S are measured in its unit ``A[s,p,d]``: the float64 sum of the
absolute values of the emission terms (as ``pairwise_cases``) plus O, whose
terms are non-negative.  ``pairwise_cases`` is imported and left as it is."""
import functools

import numpy as np
import torch

import pairwise_cases as PW

LOG2PI = PW.LOG2PI
BAR = PW.BAR
NEG = -np.inf

ABI_N = (1, 31, 33, 70)
ABI_D = (1, 5, 16, 17, 37)
ABI_P = (1, 17, 33)
ABI_F = (1, 65, 129)
PAD_LD = 144
T_EXTRA = 3


def abi_shapes():
    """(N, D) pairs: D <= N, and the one case with D = 37 > N = 33."""
    out = [(n, d) for n in ABI_N for d in ABI_D if d <= n]
    out.append((33, 37))
    return out


def softplus(v):
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def duration_reference(o, D):
    """O[p, d - 1] (P x D) in float64, the prefix in step order and then the last step's term."""
    o = np.asarray(o, dtype=np.float64)[:D]
    P = o.shape[1]
    out = np.zeros((P, D))
    cum = np.zeros(P)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(D):
            out[:, t] = cum + softplus(-o[t])
            cum = cum + softplus(o[t])
    return out


def span_reference(x, mu, lv, o, lw, D):
    """dict(S, A: N x P x D float64 (NaN where s + d > N), score, cat: N + 1 x D
    end-major (the maximum over the prototypes whose S is neither NaN nor -inf
    and the lowest index attaining it; -inf / -1 where nothing is left or d >
    e)).  mu / lv are T' x P x F and o is T' x P with T' >= D; later steps are
    not read."""
    x, mu, lv = (np.asarray(t, dtype=np.float64) for t in (x, mu, lv))
    N, P = x.shape[0], mu.shape[1]
    O = duration_reference(o, D)
    lw = np.zeros(P) if lw is None else np.asarray(lw, dtype=np.float64)
    S = np.full((N, P, D), np.nan)
    A = np.full((N, P, D), np.nan)
    E, EA = np.zeros((N, P)), np.zeros((N, P))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(min(D, N)):
            n = N - t                       # starts 0 .. n - 1 have a frame at step t
            d = x[t:, None, :] - mu[t][None, :, :]
            q = d * d * np.exp(-lv[t])[None, :, :]
            E[:n] = E[:n] + (0.5 * (LOG2PI + lv[t][None] + q)).sum(-1)
            EA[:n] = EA[:n] + (0.5 * (LOG2PI + np.abs(lv[t])[None] + q)).sum(-1)
            S[:n, :, t] = lw[None, :] - E[:n] - O[None, :, t]
            A[:n, :, t] = EA[:n] + O[None, :, t]
        score = np.full((N + 1, D), NEG)
        cat = np.full((N + 1, D), -1, dtype=np.int64)
        for e in range(1, N + 1):
            for dd in range(1, min(D, e) + 1):
                s = S[e - dd, :, dd - 1]
                ok = s > NEG                # False for NaN and -inf
                if ok.any():
                    m = np.where(ok, s, NEG)
                    score[e, dd - 1] = m.max()
                    cat[e, dd - 1] = int(m.argmax())
    return dict(S=S, A=A, score=score, cat=cat, O=O)


def viterbi_reference(span_score, span_cat, d_min, gap=None, seg_bonus=0.0):
    """The dynamic programme in a float64 loop, each addition in the kernel's
    order: dict(V (N + 1), path_score, onset, length, cat, score (lists in time
    order)).  NaN candidates are excluded, the gap wins a tie against any
    segment, then the smallest d; an unreachable end gives -inf and no segment."""
    ss = np.asarray(span_score, dtype=np.float64)
    N, D = ss.shape[0] - 1, ss.shape[1]
    bonus = np.float64(seg_bonus)
    g = None if gap is None else np.asarray(gap, dtype=np.float32).astype(np.float64)
    V = np.zeros(N + 1)
    back = np.zeros(N + 1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for n in range(1, N + 1):
            best, bd = NEG, 0
            hi = min(D, n)
            if hi >= d_min:     # c[d] = V[n - d] + span[n, d], elementwise: the scalar loop's additions
                c = V[n - d_min:(n - hi - 1 if n > hi else None):-1] + ss[n, d_min - 1:hi]
                c = np.where(np.isnan(c), NEG, c)
                i = int(c.argmax())   # the first maximum: the smallest d
                if c[i] > NEG:
                    best, bd = c[i], d_min + i
            seg = best + bonus
            gapc = V[n - 1] + g[n - 1] if g is not None else NEG
            vg, vs = gapc > NEG, bool(seg > NEG) and bd > 0
            if vg and (not vs or gapc >= seg):
                V[n], back[n] = gapc, 0
            elif vs:
                V[n], back[n] = seg, bd
            else:
                V[n], back[n] = NEG, 0
    out = dict(V=V, path_score=V[N] if N else 0.0, onset=[], length=[], cat=[], score=[])
    if not V[N] > NEG:
        out["path_score"] = NEG
        return out
    n = N
    while n > 0:
        d = int(back[n])
        if d == 0:
            n -= 1
            continue
        out["onset"].append(n - d)
        out["length"].append(d)
        out["cat"].append(int(np.asarray(span_cat)[n, d - 1]))
        out["score"].append(float(ss[n, d - 1]))
        n -= d
    for k in ("onset", "length", "cat", "score"):
        out[k].reverse()
    return out


def brute_force(span_score, d_min, gap=None, seg_bonus=0.0):
    """Every cover of N <= 8 frames by gap frames (when gap is given) and
    segments of d_min .. D frames: (best total, its moves in time order; 0 is
    a gap frame).  Totals are summed left to right as the programme sums them;
    NaN and -inf totals are no cover.  Among equal totals the moves read from
    the END are the lexicographically smallest (the gap before any segment,
    then the smallest d), which is what the programme's tie rule selects."""
    ss = np.asarray(span_score, dtype=np.float64)
    N, D = ss.shape[0] - 1, ss.shape[1]
    assert N <= 8
    g = None if gap is None else np.asarray(gap, dtype=np.float32).astype(np.float64)
    moves = ([0] if g is not None else []) + list(range(d_min, D + 1))
    best, arg = NEG, None

    def walk(n, total, path):
        nonlocal best, arg
        if n == N:
            if total > NEG and (total > best or (total == best and path[::-1] < arg[::-1])):
                best, arg = total, list(path)
            return
        for m in moves:
            with np.errstate(invalid="ignore"):
                if m == 0:
                    walk(n + 1, total + g[n], path + [0])
                elif n + m <= N:
                    walk(n + m, (total + ss[n + m, m - 1]) + np.float64(seg_bonus), path + [m])
    walk(0, np.float64(0.0), [])
    return best, arg


def moves_of(ref, N):
    """The moves (0 per gap frame, d per segment) of a viterbi_reference result."""
    out, at = [], 0
    for s, d in zip(ref["onset"], ref["length"]):
        out += [0] * (s - at) + [d]
        at = s + d
    return out + [0] * (N - at)


# ----------------------------------------------------------------------------
# inputs of the C-ABI cases
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def abi_inputs(N, D, P, F):
    """Random fp32 inputs drawn as pairwise_cases.abi_inputs draws them (mu N(0,
    1), lv U[-6, 2], offset logits U[-8, 8], log weights N(0, 1)); the recording
    is a chain of segments of random lengths 1 .. D, each around one random
    prototype (x = mu + N(0, 1) e^{lv / 2} 1.5); and the float64 reference.
    Shared, never modified."""
    g = torch.Generator().manual_seed(1000003 * N + 10007 * D + 101 * P + F)
    T = D + T_EXTRA
    mu = torch.randn(T, P, F, generator=g)
    lv = torch.rand(T, P, F, generator=g) * 8.0 - 6.0
    o = torch.rand(T, P, generator=g) * 16.0 - 8.0
    lw = torch.randn(P, generator=g)
    x = torch.empty(N, F)
    at = 0
    while at < N:
        d = min(int(torch.randint(1, D + 1, (1,), generator=g)), N - at)
        p = int(torch.randint(0, P, (1,), generator=g))
        x[at:at + d] = mu[:d, p] + torch.randn(d, F, generator=g) * torch.exp(0.5 * lv[:d, p]) * 1.5
        at += d
    return dict(N=N, D=D, P=P, F=F, T=T, x=x, mu=mu, lv=lv, o=o, lw=lw, ref=span_reference(x, mu, lv, o, lw, D))


@functools.lru_cache(maxsize=None)
def table_inputs(N, D, kind):
    """A drawn span table for the dynamic programme alone: "random" (N(0, 3)
    scores), "tied" (small integers: every sum is exact and ties abound), "holes"
    (random with NaN and -inf entries and whole rows of them)."""
    g = np.random.default_rng(7919 * N + 31 * D + len(kind))
    if kind == "tied":
        ss = g.integers(-3, 2, size=(N + 1, D)).astype(np.float64)
    else:
        ss = g.normal(0.0, 3.0, size=(N + 1, D))
    if kind == "holes":
        ss[g.random((N + 1, D)) < 0.15] = np.nan
        ss[g.random((N + 1, D)) < 0.15] = NEG
        for r in g.integers(0, N + 1, size=max(N // 8, 1)):
            ss[r] = np.nan if r % 2 else NEG
    cat = g.integers(0, 5, size=(N + 1, D)).astype(np.int32)
    for e in range(N + 1):
        ss[e, e:] = NEG
        cat[e, e:] = -1
    gap = (g.integers(-2, 1, size=N) if kind == "tied" else g.normal(-1.0, 1.0, size=N)).astype(np.float32)
    return dict(score=ss, cat=cat, gap=gap)


# ----------------------------------------------------------------------------
# candidate lengths past the registers
# ----------------------------------------------------------------------------
TAIL_FROM = 1025
"""The shortest candidate that the dynamic programmes take from their loop and
not from a register: four waves hold four candidates per thread, d <= 1024."""
TAIL_CASES = dict(forced=(2055, 1030, 1025), mixed=(1100, 1030, 1))
"""(N, D, d_min).  forced: without a gap the only covers are the six pairs
(1025, 1030) .. (1030, 1025), so every candidate of every step comes from the
loop.  mixed: columns d >= TAIL_FROM carry TAIL_REWARD, so both kinds of
candidate compete in one step."""
TAIL_REWARD = 2200.0
"""The best cover by segments of at most 1024 frames scores 1973 over the 1100
frames on these N(0, 3) entries without a gap and 2047 with one (the float64
loop), and the sum over such covers lies some tens above the best of them: at
2000 the best path already holds a long segment while its posterior is 5e-15.
At 2200 the best path holds one long segment with short ones around it and the
posterior agrees (test_span_cpu.py and test_spanpost_cpu.py assert both)."""


@functools.lru_cache(maxsize=None)
def tail_inputs(name):
    """table_inputs("random") at TAIL_CASES[name]: dict(score, cat, gap, N, D, d_min).  Shared, never modified."""
    N, D, d_min = TAIL_CASES[name]
    g = np.random.default_rng(7919 * N + 31 * D + d_min)
    ss = g.normal(0.0, 3.0, size=(N + 1, D))
    if name == "mixed":
        ss[:, TAIL_FROM - 1:] += TAIL_REWARD
    cat = g.integers(0, 5, size=(N + 1, D)).astype(np.int32)
    late = np.arange(D)[None, :] >= np.arange(N + 1)[:, None]   # d > e
    ss[late] = NEG
    cat[late] = -1
    gap = g.normal(-1.0, 1.0, size=N).astype(np.float32)
    return dict(score=ss, cat=cat, gap=gap, N=N, D=D, d_min=d_min)


@functools.lru_cache(maxsize=None)
def tail_viterbi(name, with_gap):
    """viterbi_reference on tail_inputs(name), bonus 0.  Shared, never modified."""
    t = tail_inputs(name)
    return viterbi_reference(t["score"], t["cat"], t["d_min"], t["gap"] if with_gap else None, 0.0)


# ----------------------------------------------------------------------------
# the planted case
# ----------------------------------------------------------------------------
PLANT_F, PLANT_P, PLANT_D = 33, 5, 12
PLANT_LENGTHS = (7, 3, 12, 5, 9)            # category k ends after PLANT_LENGTHS[k] frames
PLANT_LOGIT = 8.0                           # |offset logit|: sp(-8) = 3.4e-4 per agreeing step, 8 per disagreeing one
PLANT_NOISE = 0.05                          # frames = prototype mean + N(0, 0.05^2): far inside e^{lv / 2} = 0.37
PLANT_GAP_MU, PLANT_GAP_LV = 6.0, -2.0      # the background sits 6 prototype deviations away from every mean
PLANT_LAYOUT = ((2, None), (0, 0), (1, None), (2, 2), (0, 1), (3, None), (4, 4), (0, 3), (1, 1), (2, None))
"""(gap frames before, category) in time order; a trailing (gap, None)."""


@functools.lru_cache(maxsize=None)
def planted():
    """dict(x N x F, mu, lv, o, lw, gap (N fp32 background log-likelihoods), truth
    = [(onset, length, cat)], D): a recording built from the prototype means of
    chosen categories at their own lengths plus small noise, separated by
    background frames.  The offset logits are -PLANT_LOGIT before a category's
    length and +PLANT_LOGIT at it."""
    g = torch.Generator().manual_seed(20261020)
    F, P, D = PLANT_F, PLANT_P, PLANT_D
    mu = torch.randn(D, P, F, generator=g)
    lv = torch.full((D, P, F), -2.0)
    o = torch.full((D, P), -PLANT_LOGIT)
    for k, L in enumerate(PLANT_LENGTHS):
        o[L - 1, k] = PLANT_LOGIT
    lw = torch.log_softmax(torch.randn(P, generator=g), 0)
    rows, truth, at = [], [], 0
    for gapn, k in PLANT_LAYOUT:
        if gapn:
            rows.append(PLANT_GAP_MU + torch.randn(gapn, F, generator=g) * PLANT_NOISE)
            at += gapn
        if k is not None:
            L = PLANT_LENGTHS[k]
            rows.append(mu[:L, k] + torch.randn(L, F, generator=g) * PLANT_NOISE)
            truth.append((at, L, k))
            at += L
    x = torch.cat(rows)
    x64 = x.double().numpy()
    gap = (-0.5 * (LOG2PI + PLANT_GAP_LV + (x64 - PLANT_GAP_MU) ** 2 * np.exp(-PLANT_GAP_LV)).sum(1)).astype(np.float32)
    return dict(x=x, mu=mu, lv=lv, o=o, lw=lw, gap=gap, truth=truth, D=D, N=int(x.shape[0]))


def segment_alternatives(s, d, k, N, D, P):
    """The (start, length, category) spans that move one boundary of (s, d, k)
    by one frame or swap its category."""
    out = [(s, d, q) for q in range(P) if q != k]
    for s2, d2 in ((s + 1, d - 1), (s - 1, d + 1), (s, d - 1), (s, d + 1)):
        if s2 >= 0 and 1 <= d2 <= D and s2 + d2 <= N:
            out.append((s2, d2, k))
    return out


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as edge_cases.dump_observed)."""
    PW.E.dump_observed("span_" + name, rows)


def assemble(dump_dir, out_path, date, parent_commit):
    """profiles/span_errors.json from a run of tests/test_gpu_span.py with
    ABCD_PARITY_DUMP=<dump_dir>."""
    import glob
    import json
    import os
    abi, e2e = [], []
    for path in sorted(glob.glob(os.path.join(dump_dir, "span_abi_*.json"))):
        with open(path) as f:
            abi += json.load(f)
    for path in sorted(glob.glob(os.path.join(dump_dir, "span_e2e_*.json"))):
        with open(path) as f:
            e2e += json.load(f)
    vs = [r for r in abi if "vs_pairwise" in r]
    doc = dict(what="figures observed by tests/test_gpu_span.py (ABCD_PARITY_DUMP) on one MI355X; units and bars: "
                    "tests/span_cases.py", date=date, parent_commit=parent_commit,
               bars=dict(span_score=BAR, category=2 * BAR, vs_pairwise="(F + 4) 2^-23 A[s,p,d]",
                         vs_score_against="2 (F + 4) 2^-23 A[s,p,d]", path_under_oracle=BAR, viterbi="equality"),
               worst=dict(abi_span_score=max(r["score"] for r in abi), abi_category=max(r["category"] for r in abi),
                          abi_vs_pairwise=max(r["vs_pairwise"] for r in vs),
                          abi_vs_pairwise_over_bar=max(r["vs_pairwise"] / PW.cross_bar(r["F"]) for r in vs),
                          e2e_vs_score_against=max(r["vs_score_against"] for r in e2e),
                          e2e_path_under_oracle=max(r["under_oracle"] for r in e2e)),
               abi=abi, e2e=e2e)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


if __name__ == "__main__":  # python tests/span_cases.py <dump directory> <out.json> <date> <parent commit>
    import sys
    print(assemble(*sys.argv[1:5])["worst"])
