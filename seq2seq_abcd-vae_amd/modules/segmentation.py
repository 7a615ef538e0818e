# coding: utf-8
"""Cutting an uncut recording into labelled segments by the decoder.

``RNN_Variational_Decoder.span_scores`` scores every span (start, length) of
the recording's frames against every category prototype; ``segment_frames``
then picks the best cover of the recording by non-overlapping segments and gap
frames (``ops.span_viterbi``, a semi-Markov dynamic programme in fp64 on the
device).  A gap frame costs its log-likelihood under a background model:
``gap_scores`` is a diagonal Gaussian per frame, ``fit_gap_model`` takes its
moments from the frames an existing annotation leaves uncovered.  Without a
gap model the segments tile the recording."""
import math

import torch

from . import _native as N
from . import ops


def segment_frames(decoder, prototypes, frames, max_length, min_length=1, log_weight=None, gap=None, seg_bonus=0.0):
    """The best segmentation of ``frames`` (N x F on the GPU): a dict of
    ``onset``, ``length``, ``category`` (int64, one entry per segment in time
    order, frames), ``score`` (float64: each segment's ``log_weight[cat] - em -
    off``) and ``path_score`` (0-d float64: the segments' scores, ``seg_bonus``
    per segment and ``gap`` per uncovered frame summed; -inf with no segment
    when the recording cannot be covered).  ``prototypes`` is what
    ``decoder.prototypes()`` returned, decoded for at least ``max_length``
    steps; ``gap`` holds N per-frame log-likelihoods of "no segment here", or
    None: every frame then belongs to a segment."""
    N.require_gpu(frames)
    n, D, d_min = int(frames.shape[0]), int(max_length), int(min_length)
    if not 1 <= d_min <= D:
        raise ValueError(f"segment_frames: 1 <= min_length <= max_length, got {d_min} and {D}")
    with torch.no_grad():
        score, cat = decoder.span_scores(prototypes, frames, D, log_weight=log_weight)
        g = None if gap is None else torch.as_tensor(gap, device=frames.device).float()
        ps, ns, onset, length, category, seg, _ = ops.span_viterbi(score, cat, d_min, g, float(seg_bonus), False)
        k = int(ns)
    return {"onset": onset[:k].to(torch.int64), "length": length[:k].to(torch.int64),
            "category": category[:k].to(torch.int64), "score": seg[:k], "path_score": ps}


def gap_scores(frames, mu, log_var):
    """Per-frame log-likelihood (N, float32) of ``frames`` (N x F) under the
    diagonal Gaussian background ``(mu, log_var)`` (F each), formed in float64
    torch on the frames' device."""
    x = frames.double()
    mu = torch.as_tensor(mu, device=x.device).double()
    lv = torch.as_tensor(log_var, device=x.device).double()
    ll = -0.5 * (math.log(2.0 * math.pi) + lv[None, :] + (x - mu[None, :]) ** 2 * torch.exp(-lv)[None, :]).sum(1)
    return ll.float()


def fit_gap_model(frames, covered_mask):
    """``(mu, log_var)`` (F each, float64): the per-column mean and log variance
    of the frames of ``frames`` (N x F) that ``covered_mask`` (N booleans: True
    where an annotated segment covers the frame) leaves out."""
    keep = ~torch.as_tensor(covered_mask, dtype=torch.bool, device=frames.device)
    if int(keep.sum()) < 2:
        raise ValueError("fit_gap_model: fewer than two uncovered frames")
    x = frames[keep].double()
    mu = x.mean(0)
    var = ((x - mu[None, :]) ** 2).mean(0).clamp_min(1e-12)
    return mu, var.log()
