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
(``ops.span_evidence`` / ``ops.span_posterior``).
``segment_frames(transitions=...)`` puts a first-order chain over the
categories of consecutive segments inside the programme
(``ops.span_table`` / ``ops.span_chain_viterbi``); ``count_transitions`` and
``refit_transitions`` fit that chain on uncut recordings by Viterbi training.
``segment_frames(..., window_frames=W)`` runs the same programme on recordings
whose whole table does not fit: ``plan_windows`` cuts the ends into windows,
each window's table is built from a slice of the frames and
``ops.span_chain_viterbi_window`` carries the programme across them.
``segment_chain_posteriors`` is the sum half of that programme (onset, end,
gap, span and label posteriors, the evidence and the expected bigram counts
under the chain, ``ops.span_chain_posterior``) and ``refit_transitions_em``
fits the chain by EM on those counts.  ``segment_frames_warped`` cuts with the
prototypes time-warped inside the programme; ``segment_warp_posteriors`` is its
sum half and ``refit_warp_em`` fits the moves and the chain under it by EM."""
import bisect
import math

import torch

from . import _native as N
from . import ops


def segment_frames(decoder, prototypes, frames, max_length, min_length=1, log_weight=None, gap=None, seg_bonus=0.0,
                   posteriors=False, temperature=1.0, transitions=None, include_weight=False, window_frames=None):
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
    posteriors per frame).

    With ``transitions`` (a ``sequence.TransitionModel`` or a ``(log_trans,
    log_init)`` pair over the K prototypes) the categories of consecutive
    segments form a first-order chain INSIDE the programme, so the matrix moves
    boundaries as well as labels: the per-category table
    (``decoder.span_table``) goes through ``ops.span_chain_viterbi``, the
    transition being paid between consecutive segments however many gap frames
    lie between them and ``log_init`` on the first.  The chain is the prior
    over the categories, so the table is built WITHOUT ``log_weight`` unless
    ``include_weight`` is set.  ``score`` is then the chosen table entry and
    the dict additionally holds ``link`` (float64 per segment: the ``log_init``
    or ``log_trans`` term paid on entering it) and ``context_free_category``
    (int64: the lowest argmax over k of ``table[e, d, :] + log_weight`` at the
    chosen span, what the span alone would have been labelled).
    ``path_score`` sums scores, links, bonuses and gaps.  Together with
    ``posteriors=True`` this raises ValueError.

    ``window_frames`` (with ``transitions`` only; None: the whole table at
    once, which stops at ``(N + 1) max_length K < 2^31``) cuts a long recording
    into windows of that many ends (``plan_windows``): each window's table is
    built from a slice of the frames, ``ops.span_chain_viterbi_window`` runs
    the window's steps and carries the programme to the next, and the table is
    freed.  The dict is the one-shot dict, bit for bit, for every
    ``window_frames >= 1``.  Peak table memory is ``8 (n1 - row0 + 1)
    max_length K`` bytes, at most ``8 (window_frames + max_length + 32)
    max_length K``, whatever N; the carried state takes ``24 (N + 1) K``.
    ``context_free_category`` needs the chosen spans under every category: a
    second sweep rebuilds the tables of the windows that hold the end of a
    chosen segment.  Together with ``posteriors=True`` this raises
    ValueError."""
    N.require_gpu(frames)
    n, D, d_min = int(frames.shape[0]), int(max_length), int(min_length)
    if not 1 <= d_min <= D:
        raise ValueError(f"segment_frames: 1 <= min_length <= max_length, got {d_min} and {D}")
    if window_frames is not None:
        if posteriors:
            raise ValueError("segment_frames: posteriors are not available in windows; give window_frames or "
                             "posteriors=True, not both")
        if transitions is None:
            raise ValueError("segment_frames: window_frames cuts the table of the programme under a transition "
                             "model; give transitions too")
        if int(window_frames) < 1:
            raise ValueError(f"segment_frames: window_frames must be at least 1, got {window_frames}")
        return _segment_chain_windows(decoder, prototypes, frames, D, d_min, log_weight, gap, seg_bonus, transitions,
                                      include_weight, int(window_frames))
    if transitions is not None:
        if posteriors:
            raise ValueError("segment_frames: posteriors under a transition model are not available; give "
                             "transitions or posteriors=True, not both")
        return _segment_chain(decoder, prototypes, frames, D, d_min, log_weight, gap, seg_bonus, transitions,
                              include_weight)
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


def _chain_setup(name, transitions, prototypes, device):
    """(log_trans K x K, log_init K, K) from a TransitionModel or a pair, fp32 on
    ``device``, K being the prototypes' category count (``name``: the caller, for the message)."""
    if hasattr(transitions, "log_trans") and hasattr(transitions, "log_init"):
        lt, li = transitions.log_trans, transitions.log_init
    else:
        lt, li = transitions
    lt = torch.as_tensor(lt).to(device=device, dtype=torch.float32)
    li = torch.as_tensor(li).to(device=device, dtype=torch.float32).reshape(-1)
    if lt.dim() != 2 or lt.shape[0] != lt.shape[1] or li.numel() != lt.shape[0]:
        raise ValueError(f"transitions: log_trans must be K x K and log_init hold K entries, got {tuple(lt.shape)} "
                         f"and {tuple(li.shape)}")
    K = int(prototypes[2].shape[1])
    if lt.shape[0] != K:
        raise ValueError(f"{name}: the transition model has {lt.shape[0]} categories, the prototypes {K}")
    return lt, li, K


TABLE_ALIGN = 32  # the table pass's start tile (EM_TR of csrc/abcd_emtile.h)


def plan_windows(N, D, window_frames, align=TABLE_ALIGN):
    """The windows ``segment_frames(window_frames=...)`` cuts a recording of N
    frames into: a list of ``(row0, n0, n1)``, the ends ``1 .. N`` exactly once
    and in order, ``n1 - n0 + 1 <= window_frames``, and ``row0 = align *
    floor(max(0, n0 - D) / align)`` the frame the window's table starts at: a
    segment of up to D frames that ends at n0 starts no earlier, and a start
    that is a multiple of the table pass's tile puts every span at the place
    of its tile, on the thread, it has in the pass over the whole recording, so
    the window's entries have the whole table's bits.  The window's table is
    ``span_table(frames[row0:n1])``, ``8 (n1 - row0 + 1) D K`` bytes
    (``window_table_bytes``), at most ``8 (window_frames + D + align) D K``.
    A pure function."""
    N, D, W, align = int(N), int(D), int(window_frames), int(align)
    if N < 0 or D < 1 or W < 1 or align < 1:
        raise ValueError(f"plan_windows: N >= 0 and D, window_frames, align >= 1, got {N}, {D}, {W}, {align}")
    plan, n0 = [], 1
    while n0 <= N:
        n1 = min(N, n0 + W - 1)
        plan.append((align * (max(0, n0 - D) // align), n0, n1))
        n0 = n1 + 1
    return plan


def window_table_bytes(window, D, K):
    """The bytes of one ``plan_windows`` window's table over K categories."""
    row0, _, n1 = window
    return 8 * (int(n1) - int(row0) + 1) * int(D) * int(K)


def _segment_chain_windows(decoder, prototypes, frames, D, d_min, log_weight, gap, seg_bonus, transitions,
                           include_weight, window_frames):
    """segment_frames under a transition model with the table in windows (see there)."""
    if int(frames.shape[0]) == 0:   # nothing to carry: the one-shot entry point's empty path
        return _segment_chain(decoder, prototypes, frames, D, d_min, log_weight, gap, seg_bonus, transitions,
                              include_weight)
    lt, li, K = _chain_setup("segment_frames", transitions, prototypes, frames.device)
    lw = None if log_weight is None else torch.as_tensor(log_weight, device=frames.device).float().reshape(-1)
    tlw = lw if include_weight else None
    n = int(frames.shape[0])
    plan = plan_windows(n, D, window_frames)
    with torch.no_grad():
        g = None if gap is None else torch.as_tensor(gap, device=frames.device).float()
        state = ops.span_chain_window_state(n, D, K, frames.device)
        for row0, n0, n1 in plan:
            table, _, _ = decoder.span_table(prototypes, frames[row0:n1], D, log_weight=tlw)
            ps, ns, onset, length, category, seg, link = ops.span_chain_viterbi_window(
                table, row0, n0, n1, n, d_min, g, float(seg_bonus), lt, li, state, None)
            del table
        k = int(ns)
        if k < 0:
            raise RuntimeError("segment_frames: the windows of the programme ran out of order")
        onset, length = onset[:k].to(torch.int64), length[:k].to(torch.int64)
        # the second sweep: the chosen spans under every category, from the windows that hold a chosen end
        ends = (onset + length).tolist()                        # ascending
        v = torch.empty(k, K, dtype=torch.float64, device=frames.device)
        for row0, n0, n1 in plan:
            a, b = bisect.bisect_left(ends, n0), bisect.bisect_right(ends, n1)
            if a == b:
                continue
            table, _, _ = decoder.span_table(prototypes, frames[row0:n1], D, log_weight=tlw)
            v[a:b] = table[onset[a:b] + length[a:b] - row0, length[a:b] - 1]
            del table
        return _chain_dict(ps, k, onset, length, category, seg, link, v, lw, include_weight, K)


def _segment_chain(decoder, prototypes, frames, D, d_min, log_weight, gap, seg_bonus, transitions, include_weight):
    """segment_frames under a transition model (see there)."""
    lt, li, K = _chain_setup("segment_frames", transitions, prototypes, frames.device)
    lw = None if log_weight is None else torch.as_tensor(log_weight, device=frames.device).float().reshape(-1)
    n = int(frames.shape[0])
    if (N.lib().abcd_span_table_workspace_bytes(n, D, K, K) == 0
            and N.lib().abcd_span_chain_window_workspace_bytes(n, D, K) != 0):
        raise N.HipError(f"segment_frames: the whole table is beyond its index limit (N + 1) * D * K < 2^31 (N = {n}, "
                         f"D = {D}, K = {K}); give window_frames (1024, say) to build it in windows")
    with torch.no_grad():
        table, _, _ = decoder.span_table(prototypes, frames, D, log_weight=lw if include_weight else None)
        g = None if gap is None else torch.as_tensor(gap, device=frames.device).float()
        return _chain_cut(table, d_min, g, seg_bonus, lt, li, lw, include_weight, K)


def _chain_cut(table, d_min, g, seg_bonus, lt, li, lw, include_weight, K):
    """The best cover of span_table's ``table`` under the chain and the dict
    ``segment_frames(transitions=...)`` returns (inside ``torch.no_grad()``)."""
    ps, ns, onset, length, category, seg, link, _ = ops.span_chain_viterbi(table, d_min, g, float(seg_bonus), lt, li,
                                                                           False)
    k = int(ns)
    onset, length = onset[:k].to(torch.int64), length[:k].to(torch.int64)
    v = table[onset + length, length - 1]                   # k x K: the chosen spans under every category
    return _chain_dict(ps, k, onset, length, category, seg, link, v, lw, include_weight, K)


def _chain_dict(ps, k, onset, length, category, seg, link, v, lw, include_weight, K):
    """``segment_frames(transitions=...)``'s dict from the programme's outputs and ``v`` (k x K: the table's rows at
    the chosen spans)."""
    if lw is not None and not include_weight:
        v = v + lw.double()[None, :]
    v = torch.nan_to_num(v, nan=-math.inf, posinf=math.inf, neginf=-math.inf)
    ix = torch.arange(K, device=v.device)[None, :].expand_as(v)
    free = torch.where(v == v.max(1, keepdim=True).values, ix, K).min(1).values if k else onset.new_zeros(0)
    return {"onset": onset, "length": length, "category": category[:k].to(torch.int64), "score": seg[:k],
            "path_score": ps, "link": link[:k], "context_free_category": free.to(torch.int64)}


PLANE_BUDGET_BYTES = 256 << 20  # segment_frames_warped's default chunk keeps the emission plane under this


def default_chunk_frames(steps, K, budget=PLANE_BUDGET_BYTES):
    """The frames per chunk that keep ``4 chunk_frames steps K`` bytes under ``budget`` (at least 1).  A pure function."""
    return max(1, int(budget) // (4 * int(steps) * int(K)))


def _warped_plain_args(name, prototypes, steps, min_state, chunk_frames, log_moves, log_weight):
    """The plain arguments of the warped entry points, whose errors need no device -> (T, s_min, K, chunk, lm)."""
    offl = prototypes[2]
    T, s_min = int(steps), int(min_state)
    if offl.dim() != 2 or not 1 <= T <= int(offl.shape[0]):
        raise ValueError(f"{name}: 1 <= steps <= the prototypes' {int(offl.shape[0])} steps, got {T}")
    if not 0 <= s_min < T:
        raise ValueError(f"{name}: min_state must lie in 0 .. {T - 1}, got {s_min}")
    K = int(offl.shape[1])
    chunk = default_chunk_frames(T, K) if chunk_frames is None else int(chunk_frames)
    if chunk < 1:
        raise ValueError(f"{name}: chunk_frames must be at least 1, got {chunk_frames}")
    lm = list(ops._log_moves_arg(name, log_moves))
    if log_weight is not None and torch.as_tensor(log_weight).numel() != K:
        raise ValueError(f"{name}: log_weight must hold {K} entries, got {torch.as_tensor(log_weight).numel()}")
    return T, s_min, K, chunk, lm


def _warped_device_args(name, prototypes, frames, transitions, log_weight, include_weight, K):
    """-> (n, device, log_trans, log_init, log_enter) of the warped entry points, on the frames' device."""
    N.require_gpu(frames)
    n = int(frames.shape[0])
    dev = frames.device
    lw = None if log_weight is None else torch.as_tensor(log_weight, device=dev).float().reshape(-1)
    if transitions is None:
        lt, li, le = torch.zeros(K, K, device=dev), torch.zeros(K, device=dev), lw
    else:
        lt, li, _ = _chain_setup(name, transitions, prototypes, dev)
        le = lw if include_weight else None
    return n, dev, lt, li, le


def segment_frames_warped(decoder, prototypes, frames, steps, log_moves=ops.DEFAULT_LOG_MOVES, transitions=None,
                          log_weight=None, gap=None, seg_bonus=0.0, min_state=0, chunk_frames=None,
                          include_weight=False):
    """``segment_frames`` with the prototypes time-warped INSIDE the cut: the
    state of the dynamic programme is (category, prototype step), a frame stays
    on its step, moves to the next or skips one at ``log_moves`` (stay, step,
    skip; -inf disables a move), a segment ends in a step ``>= min_state`` and
    pays that step's end-of-segment logit, and the next one pays the
    transition (``ops.warp_segment_window``).  ``steps`` is
    how many of the prototypes' steps are states.  The programme costs ``N K
    steps`` cell updates, whatever the segments' lengths.

    The emission plane is built ``chunk_frames`` frames at a time
    (``decoder.frame_costs``), run and freed: peak plane memory is ``4
    chunk_frames steps K`` bytes whatever N (None: ``default_chunk_frames``,
    under ``PLANE_BUDGET_BYTES`` = 256 MiB); the carried state takes ``32 (N +
    1) K + 40 K steps`` bytes.  The result does not depend on ``chunk_frames``.

    ``transitions=None`` is a zero matrix and a zero initial vector with
    ``log_weight`` as the price of entering a category; with ``transitions``
    ``log_weight`` is used only under ``include_weight``, as in
    ``segment_frames``.  Returns ``segment_frames``' dict: ``onset``,
    ``length``, ``category`` (int64), ``link``, ``path_score`` and ``score``
    (float64: what the segment adds to the path between entering and leaving
    it, its log weight, emissions, end-of-segment logits and moves), and
    ``last_state`` (int64: the step the segment ends in) and ``tempo`` (float64:
    ``(last_state + 1) / length``, prototype steps per frame)."""
    offl = prototypes[2]
    T, s_min, K, chunk, lm = _warped_plain_args("segment_frames_warped", prototypes, steps, min_state, chunk_frames,
                                                log_moves, log_weight)
    n, dev, lt, li, le = _warped_device_args("segment_frames_warped", prototypes, frames, transitions, log_weight,
                                             include_weight, K)
    i64, f64 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float64, device=dev)
    if n == 0:
        return {"onset": torch.zeros(0, **i64), "length": torch.zeros(0, **i64), "category": torch.zeros(0, **i64),
                "score": torch.zeros(0, **f64), "path_score": torch.zeros((), **f64), "link": torch.zeros(0, **f64),
                "last_state": torch.zeros(0, **i64), "tempo": torch.zeros(0, **f64)}
    with torch.no_grad():
        g = None if gap is None else torch.as_tensor(gap, device=dev).float()
        v = offl[:T].reshape(-1)
        state = ops.warp_segment_state(n, K, T, dev)
        for n0 in range(0, n, chunk):
            n1 = min(n, n0 + chunk)
            cost = decoder.frame_costs(prototypes, frames, T, n0, n1)
            ps, ns, onset, length, category, last, enter, exit_, link = ops.warp_segment_window(
                cost, n0, n1, n, K, v, lm, le, g, float(seg_bonus), lt, li, s_min, state, None)
            del cost
        k = int(ns)
        if k < 0:
            raise RuntimeError("segment_frames_warped: the chunks of the programme ran out of order")
        length = length[:k].to(torch.int64)
        last = last[:k].to(torch.int64)
        return {"onset": onset[:k].to(torch.int64), "length": length, "category": category[:k].to(torch.int64),
                "score": exit_[:k] - enter[:k] - float(seg_bonus), "path_score": ps, "link": link[:k],
                "last_state": last, "tempo": (last + 1).double() / length.double()}


def count_transitions(categories_per_recording, K):
    """``(trans_counts K x K, init_counts K)`` in float64 on the CPU:
    ``trans_counts[i, j]`` is how often a segment of category j follows one of
    category i inside a recording, ``init_counts[k]`` how many recordings start
    with k.  ``categories_per_recording`` is a list of per-recording category
    lists in time order; empty recordings count nothing.  A pure function."""
    K = int(K)
    tc = torch.zeros(K, K, dtype=torch.float64)
    ic = torch.zeros(K, dtype=torch.float64)
    for cats in categories_per_recording:
        cats = [int(c) for c in cats]
        if any(c < 0 or c >= K for c in cats):
            raise ValueError(f"count_transitions: categories must lie in 0 .. {K - 1}")
        if cats:
            ic[cats[0]] += 1.0
        for a, b in zip(cats[:-1], cats[1:]):
            tc[a, b] += 1.0
    return tc, ic


def refit_transitions(segment_fn, recordings, model, n_iter, pseudo_count):
    """Viterbi training of a ``TransitionModel`` on uncut recordings: per
    iteration ``segment_fn(recording, model)`` (a ``segment_frames(...,
    transitions=model)`` result) segments every recording, the category
    bigrams of the paths are counted (``count_transitions``) and the model is
    set to ``(counts + pseudo_count)`` normalised per row (the same for the
    initial distribution; a row whose total is zero is kept).  Returns the
    summed path score of every iteration's segmentation, ``n_iter`` floats:
    entry i is the score under the model iteration i started from;
    ``model.last_counts`` keeps the final iteration's ``(trans, init)`` counts."""
    c = float(pseudo_count)
    totals = []
    for _ in range(int(n_iter)):
        total, cats = 0.0, []
        for rec in recordings:
            out = segment_fn(rec, model)
            total += float(out["path_score"])
            cats.append(out["category"].tolist())
        tc, ic = count_transitions(cats, model.K)
        _m_step(model, tc, ic, c)
        totals.append(total)
    return totals


def _m_step(model, tc, ic, c):
    """``(counts + c)`` normalised per row into ``model`` (a row whose total is zero is kept); keeps the counts."""
    t, i = tc + c, ic + c
    old_t, old_i = model.log_trans.double().exp().cpu(), model.log_init.double().exp().cpu()
    rs = t.sum(1, keepdim=True)
    trans = torch.where(rs > 0, t / rs.clamp_min(1e-300), old_t)
    init = i / i.sum() if float(i.sum()) > 0 else old_i
    model.set_probabilities(trans, init)
    model.last_counts = (tc, ic)


def segment_chain_posteriors(decoder, prototypes, frames, max_length, transitions, min_length=1, log_weight=None,
                             include_weight=False, gap=None, seg_bonus=0.0, temperature=1.0, want_counts=False,
                             want_table=False, with_segments=False):
    """The sum half of ``segment_frames(transitions=...)``: the posterior over
    EVERY labelled cover of ``frames`` under the transition model, from a
    semi-Markov forward-backward over (frame, last category) in fp64 on the
    device (``ops.span_chain_posterior``).  The table is built once
    (``decoder.span_table``, without ``log_weight`` unless ``include_weight``,
    as ``segment_frames`` does).  A dict of

    ``log_evidence``        0-d float64; the TEMPERED model's when ``temperature != 1``
    ``onset`` ``end`` ``gap``   N + 1 float64 each, summed over the categories (``segment_posteriors``' keys)
    ``onset_by_category``   (N + 1) x K: P(a segment of k starts at frame n)
    ``end_by_category``     (N + 1) x K: P(a segment of k ends before frame n)
    ``frame_category``      N x K: P(frame n lies in a segment of k)
    ``expected_segments``   0-d: the sum of ``end``
    ``category_usage``      K: the expected number of segments of each category
    ``no_segment``          0-d: P(the recording holds no segment at all)
    ``trans_counts`` ``init_counts``  with ``want_counts``: the expected bigram (K x K) and first-label (K) counts
    ``span``                with ``want_table``: (N + 1) x max_length, P(frames e - d .. e - 1 are one segment)

    ``temperature`` divides every term (table, gap, bonus, log_trans,
    log_init) in float64 inside the kernel.  ``with_segments`` also runs
    ``ops.span_chain_viterbi`` on the same table (at temperature 1) and adds
    ``segmentation``, what ``segment_frames(..., transitions=...)`` returns bit
    for bit, and per chosen segment ``span_posterior`` (summed over the
    categories) and ``label_posterior`` (this span with this label)."""
    N.require_gpu(frames)
    D, d_min, T = int(max_length), int(min_length), float(temperature)
    if not 1 <= d_min <= D:
        raise ValueError(f"segment_chain_posteriors: 1 <= min_length <= max_length, got {d_min} and {D}")
    if not (T > 0.0 and math.isfinite(T)):
        raise ValueError(f"temperature must be positive, got {temperature}")
    lt, li, K = _chain_setup("segment_chain_posteriors", transitions, prototypes, frames.device)
    lw = None if log_weight is None else torch.as_tensor(log_weight, device=frames.device).float().reshape(-1)
    s = 1.0 / T
    with torch.no_grad():
        table, _, _ = decoder.span_table(prototypes, frames, D, log_weight=lw if include_weight else None)
        g = None if gap is None else torch.as_tensor(gap, device=frames.device).float()
        want_span = bool(want_table or with_segments)
        log_z, lat, lat_g, post_k, gap_post, tc, ic, span = ops.span_chain_posterior(
            table, d_min, g, float(seg_bonus), s, lt, li, bool(want_counts), want_span)
        n = int(frames.shape[0])
        onset_k, end_k = post_k[0], post_k[1]
        reach = bool(log_z > -math.inf)
        no_seg = torch.exp(lat_g[0, n] - log_z) if reach else torch.zeros((), dtype=torch.float64, device=frames.device)
        out = {"log_evidence": log_z, "onset": onset_k.sum(1), "end": end_k.sum(1), "gap": gap_post,
               "onset_by_category": onset_k, "end_by_category": end_k,
               "frame_category": torch.cumsum(onset_k - end_k, 0)[:n], "expected_segments": end_k.sum(),
               "category_usage": end_k.sum(0), "no_segment": no_seg}
        if want_counts:
            out.update(trans_counts=tc, init_counts=ic)
        if want_table:
            out["span"] = span
        if with_segments:
            seg = _chain_cut(table, d_min, g, seg_bonus, lt, li, lw, include_weight, K)
            on, ln = seg["onset"], seg["length"]
            end = on + ln
            out["segmentation"] = seg
            out["span_posterior"] = span[end, ln - 1]
            if reach and on.numel():
                c = (lat[0][on, seg["category"]] + s * seg["score"] + s * float(seg_bonus)
                     + lat[4][end, seg["category"]] - log_z)
                out["label_posterior"] = torch.nan_to_num(torch.exp(c), nan=0.0)
            else:
                out["label_posterior"] = torch.zeros(on.numel(), dtype=torch.float64, device=frames.device)
    return out


def refit_transitions_em(posterior_fn, recordings, model, n_iter, pseudo_count, temperature=1.0):
    """EM (Baum-Welch) of a ``TransitionModel`` on uncut recordings, the sum
    form of ``refit_transitions``: per iteration ``posterior_fn(recording,
    model)`` (a ``segment_chain_posteriors(..., want_counts=True)`` result)
    gives every recording's expected counts and log evidence, the counts are
    summed and the M-step is ``refit_transitions``' own.  Returns per
    iteration ``temperature * sum log_evidence + pseudo_count * (sum of the
    finite log_trans and log_init)`` under the model the iteration started
    from; ``model.last_counts`` keeps the final iteration's ``(trans, init)``
    expected counts (float64, on the CPU)."""
    c, T = float(pseudo_count), float(temperature)
    totals = []
    for _ in range(int(n_iter)):
        tc = torch.zeros(model.K, model.K, dtype=torch.float64)
        ic = torch.zeros(model.K, dtype=torch.float64)
        ev = 0.0
        for rec in recordings:
            out = posterior_fn(rec, model)
            ev += float(out["log_evidence"])
            tc += torch.as_tensor(out["trans_counts"]).double().cpu()
            ic += torch.as_tensor(out["init_counts"]).double().cpu()
        lt, li = model.log_trans.double().cpu(), model.log_init.double().cpu()
        pen = float(lt[torch.isfinite(lt)].sum() + li[torch.isfinite(li)].sum())
        totals.append(T * ev + c * pen)
        _m_step(model, tc, ic, c)
    return totals


ALPHA_BUDGET_BYTES = 8 << 30  # segment_warp_posteriors(want_moves=True) keeps 8 N K steps bytes of aH: at most this


def segment_warp_posteriors(decoder, prototypes, frames, steps, log_moves=ops.DEFAULT_LOG_MOVES, transitions=None,
                            log_weight=None, gap=None, seg_bonus=0.0, min_state=0, chunk_frames=None,
                            include_weight=False, temperature=1.0, want_counts=False, want_moves=False,
                            with_segments=False):
    """The sum half of ``segment_frames_warped``: the posterior over EVERY
    cover, labelling and alignment of ``frames`` under the time-warped
    programme, from a forward-backward over (frame, category, prototype step)
    in fp64 on the device (``ops.warp_posterior_forward`` /
    ``ops.warp_posterior_backward``).  The arguments are
    ``segment_frames_warped``'s.  The emission plane is built ``chunk_frames``
    frames at a time, ascending for the forward sweep and again descending for
    the backward one, so peak plane memory is ``4 chunk_frames steps K`` bytes;
    the carried state takes ``8 (5 (N + 1) K + 4 K steps + K K)`` bytes and a
    little.  The result does not depend on ``chunk_frames``.  A dict of
    ``segment_chain_posteriors``' keys,

    ``log_evidence``        0-d float64; the TEMPERED model's when ``temperature != 1``
    ``onset`` ``end`` ``gap``   N + 1 float64 each, summed over the categories
    ``onset_by_category``   (N + 1) x K: P(a segment of k starts at frame n)
    ``end_by_category``     (N + 1) x K: P(a segment of k ends before frame n)
    ``frame_category``      N x K: P(frame n lies in a segment of k)
    ``expected_segments``   0-d: the sum of ``end``
    ``category_usage``      K: the expected number of segments of each category
    ``no_segment``          0-d: P(the recording holds no segment at all)
    ``trans_counts`` ``init_counts``  with ``want_counts``: the expected bigram (K x K) and first-label (K) counts
    ``move_counts``         with ``want_moves``: K x 3, the expected stay / step / skip moves inside segments of k
    ``expected_tempo``      with ``want_moves``: K, ``(step + 2 skip + usage) / (stay + step + skip + usage)``,
                            the expected prototype steps per frame (NaN where category k is never used)

    ``temperature`` divides every term (emissions, end-of-segment logits,
    moves, log_enter, gap, bonus, log_trans, log_init) in float64 inside the
    kernel.  ``want_moves`` keeps the forward sweep's aH plane, ``8 N K steps``
    bytes, for the backward sweep; beyond ``ALPHA_BUDGET_BYTES`` (8 GiB) it
    raises ValueError before any device work.  ``with_segments`` also runs
    ``segment_frames_warped`` with the same arguments (at temperature 1) and
    adds ``segmentation``, its dict bit for bit, and per chosen segment
    ``onset_posterior`` and ``end_posterior`` (its category's onset / end
    posterior at its first frame / behind its last) and ``occupancy`` (the mean
    of ``frame_category`` over its frames in its category)."""
    name = "segment_warp_posteriors"
    T, s_min, K, chunk, lm = _warped_plain_args(name, prototypes, steps, min_state, chunk_frames, log_moves, log_weight)
    temp = float(temperature)
    if not (temp > 0.0 and math.isfinite(temp)):
        raise ValueError(f"temperature must be positive, got {temperature}")
    n = int(frames.shape[0])
    if want_moves and 8 * n * K * T > ALPHA_BUDGET_BYTES:
        raise ValueError(f"{name}: want_moves keeps 8 N K steps = {8 * n * K * T} bytes of the forward sweep, more "
                         f"than ALPHA_BUDGET_BYTES = {ALPHA_BUDGET_BYTES}; cut the recording or raise the constant")
    n, dev, lt, li, le = _warped_device_args(name, prototypes, frames, transitions, log_weight, include_weight, K)
    f64 = dict(dtype=torch.float64, device=dev)
    s = 1.0 / temp
    want_counts, want_moves = bool(want_counts), bool(want_moves)
    with torch.no_grad():
        g = None if gap is None else torch.as_tensor(gap, device=dev).float()
        v = prototypes[2][:T].reshape(-1)
        state = ops.warp_posterior_state(n, K, T, dev)
        alpha = torch.empty(n, K * T, **f64) if want_moves else None
        args = (K, v, lm, le, g, float(seg_bonus), s, lt, li, s_min, state)
        if n == 0:
            cost = torch.empty(0, K * T, device=dev)
            log_z = ops.warp_posterior_forward(cost, 0, 0, 0, *args, None)
            post_k, gap_post, tc, ic, mc = ops.warp_posterior_backward(cost, 0, 0, 0, *args, alpha, want_counts,
                                                                       want_moves)
        starts = list(range(0, n, chunk))
        for n0 in starts:
            n1 = min(n, n0 + chunk)
            cost = decoder.frame_costs(prototypes, frames, T, n0, n1)
            log_z = ops.warp_posterior_forward(cost, n0, n1, n, *args, None if alpha is None else alpha[n0:n1])
            del cost
        for n0 in reversed(starts):
            n1 = min(n, n0 + chunk)
            cost = decoder.frame_costs(prototypes, frames, T, n0, n1)
            post_k, gap_post, tc, ic, mc = ops.warp_posterior_backward(
                cost, n0, n1, n, *args, None if alpha is None else alpha[n0:n1], want_counts, want_moves)
            del cost
        del alpha
        onset_k, end_k = post_k[0], post_k[1]
        reach = bool(log_z > -math.inf)
        G_end = ops.warp_posterior_planes(state, n, K, T)["G"][n] if n > 0 else torch.zeros((), **f64)
        no_seg = torch.exp(G_end - log_z) if reach else torch.zeros((), **f64)
        usage = end_k.sum(0)
        out = {"log_evidence": log_z, "onset": onset_k.sum(1), "end": end_k.sum(1), "gap": gap_post,
               "onset_by_category": onset_k, "end_by_category": end_k,
               "frame_category": torch.cumsum(onset_k - end_k, 0)[:n], "expected_segments": end_k.sum(),
               "category_usage": usage, "no_segment": no_seg}
        if want_counts:
            out.update(trans_counts=tc, init_counts=ic)
        if want_moves:
            den = mc.sum(1) + usage
            tempo = (mc[:, 1] + 2.0 * mc[:, 2] + usage) / den
            out.update(move_counts=mc, expected_tempo=torch.where(den > 0, tempo, torch.full_like(den, math.nan)))
    if with_segments:
        seg = segment_frames_warped(decoder, prototypes, frames, steps, log_moves=log_moves, transitions=transitions,
                                    log_weight=log_weight, gap=gap, seg_bonus=seg_bonus, min_state=min_state,
                                    chunk_frames=chunk_frames, include_weight=include_weight)
        on, ln, cat = seg["onset"], seg["length"], seg["category"]
        out["segmentation"] = seg
        out["onset_posterior"] = out["onset_by_category"][on, cat]
        out["end_posterior"] = out["end_by_category"][on + ln, cat]
        inside = torch.cat([torch.zeros(1, K, **f64), torch.cumsum(out["frame_category"], 0)])
        out["occupancy"] = (inside[on + ln, cat] - inside[on, cat]) / ln.double()
    return out


def refit_warp_em(posterior_fn, recordings, model, log_moves, n_iter, pseudo_count, move_smoothing=1.0, fit_moves=True,
                  temperature=1.0):
    """EM of the time-warped programme's parameters on uncut recordings: the
    ``TransitionModel`` (``model``; None: no matrix is fitted) and the moves
    (stay, step, skip; ``fit_moves=False`` keeps them).  Per iteration
    ``posterior_fn(recording, model, log_moves)`` (a
    ``segment_warp_posteriors(..., want_counts=True, want_moves=True)`` result)
    gives every recording's expected counts and log evidence; the counts are
    summed, the matrix takes ``refit_transitions``' M-step with
    ``pseudo_count`` and the moves take
    ``alignment.moves_from_counts(move_counts.sum(0), move_smoothing,
    log_moves)``, so a disabled move stays disabled.  Returns ``(totals,
    log_moves)``: per iteration ``refit_transitions_em``'s objective,
    ``temperature * sum log_evidence + pseudo_count * (sum of the finite
    log_trans and log_init)``, under the parameters the iteration started
    from, and the fitted moves.  ``model.last_counts`` keeps the final
    iteration's ``(trans, init)`` expected counts."""
    from . import alignment
    c, T = float(pseudo_count), float(temperature)
    lm = tuple(float(m) for m in log_moves)
    totals = []
    for _ in range(int(n_iter)):
        K = None if model is None else model.K
        tc = None if model is None else torch.zeros(K, K, dtype=torch.float64)
        ic = None if model is None else torch.zeros(K, dtype=torch.float64)
        mc = torch.zeros(3, dtype=torch.float64)
        ev = 0.0
        for rec in recordings:
            out = posterior_fn(rec, model, lm)
            ev += float(out["log_evidence"])
            if model is not None:
                tc += torch.as_tensor(out["trans_counts"]).double().cpu()
                ic += torch.as_tensor(out["init_counts"]).double().cpu()
            if fit_moves:
                mc += torch.as_tensor(out["move_counts"]).double().cpu().sum(0)
        pen = 0.0
        if model is not None:
            lt, li = model.log_trans.double().cpu(), model.log_init.double().cpu()
            pen = float(lt[torch.isfinite(lt)].sum() + li[torch.isfinite(li)].sum())
        totals.append(T * ev + c * pen)
        if model is not None:
            _m_step(model, tc, ic, c)
        if fit_moves:
            lm = alignment.moves_from_counts(mc, move_smoothing, lm)
    return totals, lm


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
