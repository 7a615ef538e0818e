# coding: utf-8
"""Cutting an uncut recording into labelled segments by the decoder.

``RNN_Variational_Decoder.span_scores`` scores every span (start, length) of
the recording's frames against every category prototype; ``segment_frames``
then picks the best cover of the recording by non-overlapping segments and gap
frames (``ops.span_viterbi``, a semi-Markov dynamic programme in fp64 on the
device).  A gap frame costs its log-likelihood under a background model:
``gap_scores`` is a diagonal Gaussian per frame, ``fit_gap_model`` takes its
moments from the frames an existing annotation leaves uncovered.  Without a
gap model the segments tile the recording.  ``segment_posteriors`` (and
``segment_frames(posteriors=True)``) say how far to trust the cut: onset, end,
gap and span posteriors over every cover and the recording's log evidence
(``ops.span_evidence`` / ``ops.span_posterior``)."""
import math

import torch

from . import _native as N
from . import ops


def segment_frames(decoder, prototypes, frames, max_length, min_length=1, log_weight=None, gap=None, seg_bonus=0.0,
                   posteriors=False, temperature=1.0):
    """The best segmentation of ``frames`` (N x F on the GPU): a dict of
    ``onset``, ``length``, ``category`` (int64, one entry per segment in time
    order, frames), ``score`` (float64: each segment's ``log_weight[cat] - em -
    off``) and ``path_score`` (0-d float64: the segments' scores, ``seg_bonus``
    per segment and ``gap`` per uncovered frame summed; -inf with no segment
    when the recording cannot be covered).  ``prototypes`` is what
    ``decoder.prototypes()`` returned, decoded for at least ``max_length``
    steps; ``gap`` holds N per-frame log-likelihoods of "no segment here", or
    None: every frame then belongs to a segment.

    With ``posteriors=True`` the span pass also sums over the categories
    (``decoder.span_evidence(want_best=True)``: one pass, the same best table
    and so the same segments bit for bit) and the dict additionally holds, per
    segment, ``onset_posterior`` (a segment starts at its first frame),
    ``offset_posterior`` (a segment ends with its last frame) and
    ``span_posterior`` (exactly this span is a segment, of any category), all
    float64 under the posterior over every cover at ``temperature`` (see
    ``segment_posteriors``), and ``log_evidence``, ``expected_segments`` (0-d
    float64) and ``curves`` (3 x (N + 1) float64: the onset, end and gap
    posteriors per frame)."""
    N.require_gpu(frames)
    n, D, d_min = int(frames.shape[0]), int(max_length), int(min_length)
    if not 1 <= d_min <= D:
        raise ValueError(f"segment_frames: 1 <= min_length <= max_length, got {d_min} and {D}")
    with torch.no_grad():
        if posteriors:
            lse, score, cat = decoder.span_evidence(prototypes, frames, D, log_weight=log_weight, want_best=True)
        else:
            score, cat = decoder.span_scores(prototypes, frames, D, log_weight=log_weight)
        g = None if gap is None else torch.as_tensor(gap, device=frames.device).float()
        ps, ns, onset, length, category, seg, _ = ops.span_viterbi(score, cat, d_min, g, float(seg_bonus), False)
        k = int(ns)
    out = {"onset": onset[:k].to(torch.int64), "length": length[:k].to(torch.int64),
           "category": category[:k].to(torch.int64), "score": seg[:k], "path_score": ps}
    if posteriors:
        log_z, _, post, table = _tempered_posterior(lse, d_min, g, seg_bonus, temperature, True)
        end = out["onset"] + out["length"]
        out.update(onset_posterior=post[0][out["onset"]], offset_posterior=post[1][end],
                   span_posterior=table[end, out["length"] - 1], log_evidence=log_z, curves=post,
                   expected_segments=post[1].sum())
    return out


def _tempered_posterior(table, d_min, gap, seg_bonus, temperature, want_table):
    """ops.span_posterior on the table, the gap and the bonus divided by the temperature in float64."""
    T = float(temperature)
    if not T > 0.0:
        raise ValueError(f"temperature must be positive, got {temperature}")
    with torch.no_grad():
        if T != 1.0:
            table = table.double() / T
            gap = None if gap is None else gap.double() / T
        return ops.span_posterior(table, int(d_min), gap, float(seg_bonus) / T, bool(want_table))


def segment_posteriors(decoder, prototypes, frames, max_length, min_length=1, log_weight=None, gap=None,
                       seg_bonus=0.0, marginal=True, temperature=1.0, want_table=False):
    """How far to trust a segmentation: the posterior over EVERY cover of
    ``frames`` by segments of ``min_length .. max_length`` frames and gap
    frames (arguments as ``segment_frames``), from a semi-Markov
    forward-backward in fp64 on the device (``ops.span_posterior``).  A dict of

    ``log_evidence``       0-d float64: the log of the sum over all covers
    ``onset``              N + 1 float64: P(a segment starts at frame n); [N] = 0
    ``end``                N + 1 float64: P(a segment ends before frame n); [0] = 0
    ``gap``                N + 1 float64: P(frame n is background); [N] = 0
    ``expected_segments``  0-d float64: the sum of ``end``
    ``span``               with ``want_table``: N + 1 x max_length float64,
                           end-major, P(frames e - d .. e - 1 are one segment)

    ``marginal=True`` sums each span over the categories
    (``decoder.span_evidence``); ``marginal=False`` runs on ``span_scores``'
    maximum, the table the best path is read from.  ``temperature`` divides the
    span table, the gap and the bonus before the programme, in float64:
    ``log_evidence`` is then the TEMPERED model's, not the decoder's.  With
    some hundred columns per frame the raw posteriors are almost all 0 or 1;
    the temperature is the calibration knob.  An uncoverable recording gives
    ``log_evidence`` = -inf and zeros."""
    N.require_gpu(frames)
    D, d_min = int(max_length), int(min_length)
    if not 1 <= d_min <= D:
        raise ValueError(f"segment_posteriors: 1 <= min_length <= max_length, got {d_min} and {D}")
    with torch.no_grad():
        if marginal:
            table, _, _ = decoder.span_evidence(prototypes, frames, D, log_weight=log_weight)
        else:
            table, _ = decoder.span_scores(prototypes, frames, D, log_weight=log_weight)
        g = None if gap is None else torch.as_tensor(gap, device=frames.device).float()
        log_z, _, post, span = _tempered_posterior(table, d_min, g, seg_bonus, temperature, want_table)
    out = {"log_evidence": log_z, "onset": post[0], "end": post[1], "gap": post[2], "expected_segments": post[1].sum()}
    if want_table:
        out["span"] = span
    return out


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
