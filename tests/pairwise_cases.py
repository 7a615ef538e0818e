"""Cases and the float64 references of pairwise scoring: every segment against
every category prototype (``abcd_pairwise_nll``, ``abcd_pair_posterior``,
``RNN_Variational_Decoder.prototypes`` / ``score_against``,
``ABCDSampler.expected_log_prior``, ``classify.py``).

The prototypes are a time-major rectangle: ``mu`` / ``lv`` are ``T x P x F``,
the offset logits ``T x P``; prototype p at step t is row ``t * P + p`` of the
flattened form the kernels read.  The reference is numpy float64 on the SAME
fp32 inputs:

    em [b, p] = sum_{t < len_b} sum_f 0.5 (log 2pi + lv[t,p,f] + (x[off_t + b, f] - mu[t,p,f])^2 e^-lv[t,p,f])
    off[b, p] = sum_{t < len_b} max(o,0) - o y + log1p(e^-|o|),  o = logits[t, p], y = gt_offset[off_t + b]

Errors of ``em`` are measured in its unit ``A[b, p]``, the float64 sum of the
absolute values of its terms (as ``score_cases.emission_rows``); BCE terms are
non-negative, so ``off`` is its own unit.  ``score_cases`` and ``edge_cases``
are imported and left as they are.
"""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import edge_cases as E  # noqa: E402
import score_cases as S  # noqa: E402

LOG2PI = S.LOG2PI
BAR = S.BAR                      # 1e-4 of the unit, the project's loss bar
# score_cases' segment lengths, and one more: the kernel cuts time into 16-step slices per 32-segment
# tile, and none of those shapes is longer than 12 steps
ABI_SHAPES = OrderedDict(S.ABI_SHAPES)
ABI_SHAPES["b40t37"] = [37, 33, 32, 17, 16, 16] + [15] * 10 + [9] * 16 + [6, 5, 3, 2, 2, 1, 1, 1]  # 3 slices, then 1
ABI_F = S.ABI_F
ABI_P = (1, 17, 33)              # one prototype, one past a 16- and a 32-wide tile
PAD_LD = S.PAD_LD
T_EXTRA = 3                      # the rectangle is decoded T + 3 steps long
NAN_SHAPES = ("b1t1", "ties", "b33t9", "b40t37")   # the per-segment NaN check runs up to b33t9 and on the sliced shape


def cross_bar(F):
    """|pair_em[b,p] - seg_em[b]| <= (F + 4) 2^-23 A[b,p] against
    abcd_segment_losses on prototype p expanded to the packed layout: at most F
    fp32 additions per frame in each of the two per-frame sums (the quadratic
    form and sum_f (log 2pi + lv)), each rounding by 2^-24 of a partial no
    larger than the frame's unit, a few roundings from precomputing e^-lv, and
    fp64 across frames in both kernels."""
    return (F + 4) * 2.0 ** -23


POST_B = (1, 5, 33)
POST_P = (1, 16, 65, 130)
LOGEV_BAR = 2.0 ** -22           # fp64 arithmetic and one cast to fp32, with a factor of 4
RESP_BAR = 1e-5                  # 106 x 2^-24 relative for an fp32 fast exponential; an fp64 one sits far inside

E2E_SMALL = S.E2E_SMALL
E2E_EDGE = S.E2E_EDGE
E2E_EDGE_CATEGORIES = 17


# ----------------------------------------------------------------------------
# float64 references
# ----------------------------------------------------------------------------
def step_of_rows(batch_sizes):
    """t[r] = the step packed row r belongs to."""
    return np.concatenate([np.full(int(b), t, dtype=np.int64) for t, b in enumerate(batch_sizes)])


def pairwise_reference(batch_sizes, gt=None, mu=None, lv=None, o=None, y=None):
    """dict(em, A, off, lengths): B x P float64 emission NLL, its unit and the
    offset BCE of every (segment, prototype); mu / lv are T' x P x F and o is
    T' x P with T' >= len(batch_sizes) (later steps are not read)."""
    bs = np.asarray(batch_sizes, dtype=np.int64)
    B, T = int(bs[0]), len(bs)
    out = dict(lengths=S.lengths_of(bs))
    off = np.concatenate([[0], np.cumsum(bs)])
    if gt is not None:
        gt, mu, lv = S._np64(gt), S._np64(mu), S._np64(lv)
        P = mu.shape[1]
        em, A = np.zeros((B, P)), np.zeros((B, P))
        for t in range(T):
            n = int(bs[t])
            d = gt[off[t]:off[t] + n, None, :] - mu[t][None, :, :]
            q = d * d * np.exp(-lv[t])[None, :, :]
            em[:n] += (0.5 * (LOG2PI + lv[t][None] + q)).sum(-1)
            A[:n] += (0.5 * (LOG2PI + np.abs(lv[t])[None] + q)).sum(-1)
        out["em"], out["A"] = em, A
    if o is not None:
        o, y = S._np64(o), S._np64(y)
        bce = np.zeros((B, o.shape[1]))
        for t in range(T):
            n = int(bs[t])
            x = o[t][None, :]
            bce[:n] += np.maximum(x, 0.0) - x * y[off[t]:off[t] + n, None] + np.log1p(np.exp(-np.abs(x)))
        out["off"] = bce
    return out


def expand_prototype(batch_sizes, p, mu, lv, o):
    """Prototype p in the packed layout of the batch: (mu L x F, lv L x F, o L),
    row r holding step t[r] of the prototype -- what every segment would get
    from a decoder run on prototype p's features."""
    t = step_of_rows(batch_sizes)
    return mu[t, p], lv[t, p], o[t, p]


def posterior_reference(em, off=None, lw=None):
    """dict(log_evidence B, resp B x P, best B, best_prob B, s B x P) in float64.
    A NaN or +inf NLL, or a NaN or -inf weight, excludes its prototype; a row
    with none left has log_evidence = -inf, best = -1, best_prob = 0."""
    em = S._np64(em)
    s = -em
    if off is not None:
        s = s - S._np64(off)
    if lw is not None:
        s = s + S._np64(lw)[None, :]
    with np.errstate(invalid="ignore"):
        ok = s > -np.inf          # False for NaN and -inf
    s = np.where(ok, s, -np.inf)
    m = s.max(1)
    some = m > -np.inf
    ms = np.where(some, m, 0.0)
    e = np.exp(s - ms[:, None])   # 0 for an excluded prototype; the winner's is 1
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.where(some, ms + np.log(e.sum(1)), -np.inf)
        resp = np.where(some[:, None], e / e.sum(1)[:, None], 0.0)   # not exp(s - lse): lse ~ 5e4 rounds by 7e-12
    best = np.where(some, s.argmax(1), -1)   # argmax: the lowest index of the maximum
    bp = np.where(some, resp[np.arange(len(s)), np.maximum(best, 0)], 0.0)
    return dict(log_evidence=lse, resp=resp, best=best, best_prob=bp, s=s)


# ----------------------------------------------------------------------------
# inputs of the C-ABI cases
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def abi_inputs(shape, F, P):
    """Random fp32 inputs of one (shape, F, P), drawn as score_cases.abi_inputs
    draws them: mu N(0, 1), lv U[-6, 2] (terms of both signs), every segment's
    frames around one random prototype (x = mu + N(0, 1) e^{lv / 2} 1.5), offset
    logits U[-8, 8], 0/1 targets; and their float64 reference.  Shared, never
    modified."""
    lengths = ABI_SHAPES[shape]
    bs = S.batch_sizes_of(lengths)
    T, B, L = len(bs), len(lengths), int(bs.sum())
    g = torch.Generator().manual_seed(100000 * P + 1000 * B + F)
    mu = torch.randn(T, P, F, generator=g)
    lv = torch.rand(T, P, F, generator=g) * 8.0 - 6.0
    own = torch.randint(0, P, (B,), generator=g)
    t_of, b_of = torch.from_numpy(step_of_rows(bs)), torch.from_numpy(S.segment_of_rows(bs))
    m, v = mu[t_of, own[b_of]], lv[t_of, own[b_of]]
    gt = m + torch.randn(L, F, generator=g) * torch.exp(0.5 * v) * 1.5
    o = torch.rand(T, P, generator=g) * 16.0 - 8.0
    y = (torch.rand(L, generator=g) < 0.3).float()
    ref = pairwise_reference(bs, gt, mu, lv, o, y)
    return dict(lengths=lengths, batch_sizes=bs, T=T, B=B, L=L, F=F, P=P, gt=gt, mu=mu, lv=lv, o=o, y=y, own=own,
                ref=ref)


@functools.lru_cache(maxsize=None)
def posterior_inputs(B, P):
    """em ~ 5e4 + U[0, 60], off ~ U[0, 10], log_weight ~ N(0, 1) in fp32; 1.0 is
    then taken off the NLL of each row's float64 winner, so every row's top-two
    gap is at least 1 minus what the fp32 subtraction rounds (>= 0.5, asserted on
    the CPU) and ``best`` is decided."""
    g = torch.Generator().manual_seed(977 * B + P)
    em = 5e4 + torch.rand(B, P, generator=g) * 60.0
    off = torch.rand(B, P, generator=g) * 10.0
    lw = torch.randn(P, generator=g)
    win = posterior_reference(em, off, lw)["best"]
    em[torch.arange(B), torch.from_numpy(win)] -= 1.0
    return dict(em=em, off=off, lw=lw, ref=posterior_reference(em, off, lw))


def top_two_gap(s):
    """per row: the best score minus the second best (inf with one prototype)."""
    if s.shape[1] == 1:
        return np.full(s.shape[0], np.inf)
    srt = np.sort(s, axis=1)
    return srt[:, -1] - srt[:, -2]


# ----------------------------------------------------------------------------
# the float64 oracle's prototypes and pairwise scores
# ----------------------------------------------------------------------------
def oracle_prototypes(P, ocfg, categories, speakers, length):
    """(mu, lv, o): length x len(categories) x F (x 2) and length x len(categories)
    in float64: the oracle's decoder on the rectangle, features = the codebook
    columns of ``categories`` (with ``speakers`` alike, or None), zero eps,
    train=False."""
    from oracle import abcd_oracle as O
    P64 = E._cast(P, torch.float64)
    cats = torch.as_tensor(categories, dtype=torch.int64)
    n, F = int(cats.numel()), ocfg["F"]
    feats = P64["feature_sampler/codebook"].t()[cats]
    spk = None
    if "decoder/embed_speaker.weight" in P64:
        spk = torch.as_tensor(speakers, dtype=torch.int64)
    with torch.no_grad():
        _, _, _, (mu, lv), offl = O.decoder_forward(P64, feats, [n] * int(length), ocfg,
                                                    torch.zeros(n * int(length), F, dtype=torch.float64),
                                                    speakers=spk, train=False)
    return mu.view(length, n, F), lv.view(length, n, F), offl.view(length, n)


def oracle_pairwise(P, ocfg, batch, categories, speakers):
    """The float64 pairwise scores of a batch: dict(em, A, off, lengths) with a
    column per (categories[i], speakers[i])."""
    bsz = batch["batch_sizes"].numpy()
    mu, lv, o = oracle_prototypes(P, ocfg, categories, speakers, len(bsz))
    return pairwise_reference(bsz, batch["data"].double(), mu, lv, o, batch["is_offset"].double())


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as edge_cases.dump_observed)."""
    E.dump_observed("pairwise_" + name, rows)
