# coding: utf-8
"""Time-warped alignment of segments to category prototypes: what a path says
about its segment, move weights refitted from paths, and the call the
``align.py`` tool makes per batch.

The kernels are ``ops.warp_nll`` / ``ops.warp_path`` behind
``RNN_Variational_Decoder.warp_against`` / ``align_to``: a
prototype's steps are the states of a left-to-right HMM, frame t of a segment
sits on state a(t), a(0) = 0, and a(t + 1) - a(t) is 0, 1 or 2 (stay, step,
skip).  Paths come packed as the batch is: row ``off_t + b`` holds a(t) of
segment b, -1 for a segment without a path."""
import math

import torch

from . import ops

STAY, STEP, SKIP = 0, 1, 2


def _padded(states, batch_sizes):
    """(B x T int64 states, -2 past a segment's end; lengths B) from packed states."""
    states = torch.as_tensor(states).to("cpu", torch.int64)
    bs = torch.as_tensor(batch_sizes).to("cpu", torch.int64)
    B, T = int(bs[0]), int(bs.numel())
    if int(bs.sum()) != states.numel():
        raise ValueError(f"states holds {states.numel()} rows, batch_sizes {int(bs.sum())}")
    pad = torch.full((B, T), -2, dtype=torch.int64)
    off = 0
    for t, n in enumerate(bs.tolist()):
        pad[:n, t] = states[off:off + n]
        off += n
    return pad, (pad != -2).sum(1)


def _move_counts(pad, lengths):
    """B x 3: how often each segment's path stays, steps and skips (zeros without a path)."""
    mv = pad[:, 1:] - pad[:, :-1]
    live = (torch.arange(1, pad.shape[1])[None, :] < lengths[:, None]) & (pad[:, :1] >= 0)
    return torch.stack([((mv == m) & live).sum(1) for m in (STAY, STEP, SKIP)], 1)


def summarize_paths(states, batch_sizes):
    """Per segment (packed row order), as a dict of B-entry tensors:
    ``end_state`` (the state of the last frame, -1 without a path), ``n_stay``
    and ``n_skip`` (moves of 0 and of 2 states along the path), ``length`` and
    ``tempo = (end_state + 1) / length``: prototype steps covered per frame, 1
    for the prototype's own pace, below 1 for a slower rendition (0 without a
    path)."""
    pad, lengths = _padded(states, batch_sizes)
    end = pad.gather(1, (lengths - 1)[:, None])[:, 0]
    counts = _move_counts(pad, lengths)
    return dict(end_state=end, n_stay=counts[:, STAY], n_skip=counts[:, SKIP], length=lengths,
                tempo=(end + 1).double() / lengths.double())


def fit_moves(states, batch_sizes, smoothing=1.0, log_moves=None):
    """New ``log_moves`` (stay, step, skip) from the move counts along the
    paths -- one round of hard EM: ``log((count_m + smoothing) / sum)``.
    Segments without a path count nothing.  A move that ``log_moves`` (the
    weights the paths were found under) disables stays disabled."""
    pad, lengths = _padded(states, batch_sizes)
    return moves_from_counts(_move_counts(pad, lengths).sum(0), smoothing, log_moves)


def moves_from_counts(counts, smoothing=1.0, log_moves=None):
    """``fit_moves`` from the three move counts (e.g. summed over batches)."""
    if smoothing < 0:
        raise ValueError("smoothing must not be negative")
    on = [True] * 3 if log_moves is None else [float(v) > -math.inf for v in log_moves]
    mass = [float(c) + float(smoothing) if k else 0.0 for c, k in zip(torch.as_tensor(counts).tolist(), on)]
    total = sum(mass)
    if not total > 0:
        raise ValueError("fit_moves: no move was counted and smoothing is 0")
    return tuple(math.log(m / total) if m > 0 else -math.inf for m in mass)


def moves_from_probabilities(probs):
    """``--moves STAY STEP SKIP``: non-negative weights, normalised; 0 disables a move."""
    probs = [float(p) for p in probs]
    if len(probs) != 3 or any(p < 0 or math.isnan(p) or math.isinf(p) for p in probs) or not sum(probs) > 0:
        raise ValueError(f"moves: three non-negative weights, not all zero (got {probs})")
    total = sum(probs)
    return tuple(math.log(p / total) if p > 0 else -math.inf for p in probs)


def align_segments(decoder, prototypes, batch_sizes, data, is_offset, log_weight=None, log_moves=ops.DEFAULT_LOG_MOVES,
                   band=None, marginal=False, columns=None):
    """One batch against every category, time-warped, and each segment's path
    to its best category.  ``columns`` (B x K int64, optional) selects each
    segment's K columns of a wider prototype rectangle (its own speaker's), as
    ``classify.py`` does.  Returns a dict: ``warp`` (B x K), ``log_evidence``,
    ``best`` (int64, -1 when no category is reachable), ``best_prob`` (from
    ``ops.pair_posterior`` on the warped matrix with ``log_weight``),
    ``warp_nll`` (the best category's entry; +inf without one), ``states``
    (L, packed), the path's ``em`` / ``off`` / ``move``, and
    ``summarize_paths``'s entries."""
    warp = decoder.warp_against(prototypes, batch_sizes, data, is_offset, log_moves=log_moves, band=band,
                                marginal=marginal)
    if columns is not None:
        warp = warp.gather(1, columns)
    ev, best, best_prob, _resp = ops.pair_posterior(warp, None, log_weight)
    best = best.to(torch.int64)
    col = best.clamp(min=0)[:, None]
    choice = torch.where(best >= 0, (col if columns is None else columns.gather(1, col))[:, 0], best)
    states, em, off, move = decoder.align_to(prototypes, batch_sizes, data, choice, is_offset, log_moves=log_moves,
                                             band=band)
    nll = torch.where(best >= 0, warp.gather(1, col)[:, 0], torch.full_like(ev, math.inf))
    out = dict(warp=warp, log_evidence=ev, best=best, best_prob=best_prob, warp_nll=nll, states=states, em=em, off=off,
               move=move)
    out.update(summarize_paths(states, batch_sizes))
    return out
