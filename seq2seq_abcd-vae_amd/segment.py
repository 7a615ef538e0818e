# coding: utf-8
"""Segmentation on the HIP path: cut uncut recordings into labelled segments
with a trained ABCD-VAE's decoder.

Every other entry point starts from an annotation table that already gives each
segment's onset and offset.  This script needs the recordings only.  The K
categories are decoded once as prototypes (``classify.Classifier.prototypes_for``);
the end-of-segment logits make them a duration model, so ``log p(frames s .. s
+ d - 1, ends after d | category k)`` is defined for every start, length and
category of a recording (``RNN_Variational_Decoder.span_scores``), and a
semi-Markov dynamic programme picks the best cover of the recording by
non-overlapping segments (``modules.segmentation.segment_frames``).  Frames no
segment covers cost ``--gap_score`` each, or their log-likelihood under a
diagonal Gaussian background (``--gap_model``, fitted from the uncovered frames
of an existing annotation by ``--fit_gap``); without either the segments tile
the recording.

Same checkpoint, STFT, epsilon, normaliser and channel arguments as
``classify.py``.  The input table needs an ``input_path`` column only (an
existing annotation works: its distinct paths are used); each recording is
featurised whole.  Output: an annotation CSV in the reference's format,

``onset, offset, input_path, data_type, speaker, label, category_ix, length,
segment_score``

with times in seconds and ``label`` = ``category_ix``, which feeds straight into
``encode.py``, ``classify.py``, ``sequence.py`` or ``learning.py``.  A segment of
frames ``s .. s + d - 1`` is written as samples ``s hop .. (s + d - 1) hop +
(hop - 1) // 2`` (plus the window length without centring), which the package's
loader turns into exactly d frames again.  The loader pads each segment at its
own edges, so the frames nearest a boundary differ from the whole-recording
frames this script scored: ``classify.py`` on the result can disagree with
``category_ix`` there.

``--transitions transitions.csv`` (what ``sequence.py`` wrote) makes the
categories of consecutive segments a first-order chain inside the dynamic
programme, so the matrix moves boundaries as well as labels; the table then
also holds ``transition_score`` (the log initial or transition probability paid
on entering the segment), ``context_free_category_ix`` (the span's label
without the chain) and ``changed``.  ``--refit_transitions N`` runs N rounds of
Viterbi training of the matrix on the recordings first and writes it to
``--transitions_out``; ``--refit_method em`` makes those rounds EM on the expected
bigram counts over every labelled cover instead.  ``--chain_posteriors`` sums
over every labelled cover under the chain (``segmentation.segment_chain_posteriors``)
and appends ``onset_posterior``, ``offset_posterior``, ``span_posterior`` and
``label_posterior``: how far to trust each cut and each label.
``--window_frames W`` (with ``--transitions``) cuts long recordings' tables into
windows of W ends: the same segments, bit for bit, at a table memory that does
not grow with the recording.

``--warp`` cuts with the prototypes time-warped inside the dynamic programme
(``segmentation.segment_frames_warped``): a frame stays on its prototype step,
moves to the next or skips one with the probabilities ``--moves``, so a segment
sung slower or faster than its prototype is still one segment.  ``--max_length``
is then the number of prototype steps, not a bound on the segments' frames; the
table gains ``last_state`` and ``tempo`` (prototype steps per frame), and
``transition_score`` with ``--transitions``.  ``--warp_posteriors`` sums over
every cover, labelling and alignment under that programme
(``segmentation.segment_warp_posteriors``) and appends ``onset_posterior``,
``offset_posterior`` and ``occupancy``; ``--warp_refit N`` first runs N rounds of
EM on the recordings (``segmentation.refit_warp_em``): the moves go to
``--moves_out`` (``--keep_moves`` fixes them) and, with ``--transitions``, the
matrix to ``--transitions_out``."""
import os
import sys

import numpy as np
import pandas as pd
import scipy.io.wavfile as spw
import torch

import classify
import cli
from modules import _native, alignment, segmentation

COLUMNS = ("onset", "offset", "input_path", "data_type", "speaker", "label", "category_ix", "length", "segment_score")
POSTERIOR_COLUMNS = ("onset_posterior", "offset_posterior", "span_posterior")   # appended by --posteriors
SYNTAX_COLUMNS = ("transition_score", "context_free_category_ix", "changed")      # appended by --transitions
CHAIN_POSTERIOR_COLUMNS = POSTERIOR_COLUMNS + ("label_posterior",)                # appended by --chain_posteriors
WARP_COLUMNS = ("last_state", "tempo")                                            # appended by --warp
WARP_POSTERIOR_COLUMNS = ("onset_posterior", "offset_posterior", "occupancy")     # appended by --warp_posteriors
MOVE_COLUMNS = ("stay", "step", "skip")                                           # --moves_out: one row of probabilities
REFIT_METHODS = ("viterbi", "em")
TRANSITION_COLUMNS = ("from_ix", "to_ix", "probability", "expected_count")       # sequence.py's transitions.csv
RECORDING_COLUMNS = ("input_path", "n_frames", "n_segments", "path_score", "log_evidence", "expected_segments")


def num_frames(samples, frame, hop, centering=True):
    """Frames ``torch.stft`` gives for ``samples`` samples."""
    return 1 + samples // hop if centering else (1 + (samples - frame) // hop if samples >= frame else 0)


def min_loadable_length(frame, hop, centering=True):
    """The shortest segment (frames) the loader can featurise again: the
    centred STFT reflects frame // 2 samples at each edge and needs more
    samples than that."""
    if not centering:
        return 1
    d = 1
    while frames_to_samples(0, d, frame, hop, True)[1] <= frame // 2:
        d += 1
    return d


def frames_to_samples(onset, length, frame, hop, centering=True, total=None):
    """(onset_ix, offset_ix) in samples of the segment of frames ``onset ..
    onset + length - 1`` of a whole-recording STFT, such that the loader's cut
    ``wav[onset_ix:offset_ix]`` has exactly ``length`` frames, centred on (or
    starting at) the same samples.  The cut ends in the middle of the range of
    sample counts that give ``length`` frames, so rounding a time by one sample
    does not change the count; ``total`` (the recording's samples) clips it."""
    on = int(onset) * hop
    off = (int(onset) + int(length) - 1) * hop + (hop - 1) // 2 + (0 if centering else frame)
    if total is not None:
        off = min(off, int(total))
    return on, off


def covered_frames(n_frames, onsets, offsets, fs, frame, hop, centering=True):
    """N booleans: whether a frame of the whole-recording STFT lies inside one
    of the annotated segments (seconds), by its centre sample (centred STFT) or
    by any overlap of its window."""
    at = np.arange(n_frames, dtype=np.int64) * hop
    mask = np.zeros(n_frames, dtype=bool)
    for on, off in zip(np.round(np.asarray(onsets) * fs), np.round(np.asarray(offsets) * fs)):
        mask |= ((at >= on) & (at <= off)) if centering else ((at < off) & (at + frame > on))
    return mask


def segment_rows(input_path, onset, length, category, score, fs, frame, hop, centering, total, data_type="segmented",
                 speaker=float("nan"), posteriors=None, syntax=None, chain_posteriors=None, warp=None,
                 warp_posteriors=None):
    """The table rows of one recording's segments (frame units -> seconds);
    ``posteriors``: the three per-segment lists of POSTERIOR_COLUMNS;
    ``syntax``: (link, context-free category) per segment for SYNTAX_COLUMNS;
    ``chain_posteriors``: the four per-segment lists of CHAIN_POSTERIOR_COLUMNS;
    ``warp``: (last state, tempo, link or None) per segment for WARP_COLUMNS
    and, with a link, ``transition_score``; ``warp_posteriors``: the three
    per-segment lists of WARP_POSTERIOR_COLUMNS."""
    rows = []
    for i, (s, d, k, v) in enumerate(zip(onset, length, category, score)):
        on, off = frames_to_samples(s, d, frame, hop, centering, total)
        rows.append({"onset": on / fs, "offset": off / fs, "input_path": input_path, "data_type": data_type,
                     "speaker": speaker, "label": int(k), "category_ix": int(k), "length": int(d),
                     "segment_score": float(v)})
        if posteriors is not None:
            rows[-1].update({c: float(p[i]) for c, p in zip(POSTERIOR_COLUMNS, posteriors)})
        if syntax is not None:
            link, free = syntax
            rows[-1].update({"transition_score": float(link[i]), "context_free_category_ix": int(free[i]),
                             "changed": int(int(free[i]) != int(k))})
        if chain_posteriors is not None:
            rows[-1].update({c: float(p[i]) for c, p in zip(CHAIN_POSTERIOR_COLUMNS, chain_posteriors)})
        if warp is not None:
            last, tempo, link = warp
            rows[-1].update({"last_state": int(last[i]), "tempo": float(tempo[i])})
            if link is not None:
                rows[-1]["transition_score"] = float(link[i])
        if warp_posteriors is not None:
            rows[-1].update({c: float(p[i]) for c, p in zip(WARP_POSTERIOR_COLUMNS, warp_posteriors)})
    return rows


def write_segments(save_path, rows, posteriors=False, recordings_out=None, recordings=(), curves=None, syntax=False,
                   transitions_out=None, transitions=None, chain_posteriors=False, warp=False,
                   warp_posteriors=False, moves_out=None, moves=None):
    """Writes the annotation table (an existing file is kept as .prev, nothing
    partial is left behind) and, with ``posteriors``, its three extra columns,
    the per-recording table and the per-recording curve files ({path: dict of
    arrays}) in the same replacement; with ``syntax`` the SYNTAX_COLUMNS, and
    ``transitions`` (a table in TRANSITION_COLUMNS) to ``transitions_out``;
    with ``chain_posteriors`` the CHAIN_POSTERIOR_COLUMNS after those; with
    ``warp`` the WARP_COLUMNS (and, with ``syntax``, ``transition_score`` alone
    of the SYNTAX_COLUMNS: the warped programme has no context-free label);
    with ``warp_posteriors`` the WARP_POSTERIOR_COLUMNS last, and ``moves``
    (three probabilities) to ``moves_out``.  Returns the number of rows."""
    df = pd.DataFrame(rows, columns=list(COLUMNS) + (list(POSTERIOR_COLUMNS) if posteriors else []) +
                      (list(WARP_COLUMNS) if warp else []) +
                      (list(SYNTAX_COLUMNS[:1] if warp else SYNTAX_COLUMNS) if syntax else []) +
                      (list(CHAIN_POSTERIOR_COLUMNS) if chain_posteriors else []) +
                      (list(WARP_POSTERIOR_COLUMNS) if warp_posteriors else []))
    with cli.replacing_outputs() as tmp:
        df.to_csv(tmp(save_path), index=False)
        if recordings_out is not None:
            pd.DataFrame(list(recordings), columns=list(RECORDING_COLUMNS)).to_csv(tmp(recordings_out), index=False)
        if transitions_out is not None:
            transitions.to_csv(tmp(transitions_out), index=False)
        if moves_out is not None:
            pd.DataFrame([list(moves)], columns=list(MOVE_COLUMNS)).to_csv(tmp(moves_out), index=False)
        for path, arrays in (curves or {}).items():
            with open(tmp(path), "wb") as f:
                np.savez(f, **arrays)
    return len(df)


def curve_path(curves_dir, input_path):
    """<curves_dir>/<the recording's path with separators replaced, without its extension>.npz"""
    stem = os.path.splitext(input_path)[0].replace(os.sep, "__").replace("/", "__")
    return os.path.join(curves_dir, stem + ".npz")


def read_wave(input_root, input_path, channel=0):
    fs, data = spw.read(os.path.join(input_root, input_path))
    if data.ndim > 1:
        data = data[:, channel]
    return fs, np.ascontiguousarray(data).astype(np.float32)


class Segmenter(classify.Classifier):
    """A trained ABCD checkpoint opened for segmentation."""

    def segment_recording(self, frames, max_length, min_length=1, log_weight=None, gap=None, seg_bonus=0.0,
                          speaker=None, posteriors=False, temperature=1.0, transitions=None, window_frames=None):
        """``segmentation.segment_frames`` of one recording's frames under the
        categories' prototypes (of ``speaker`` when the decoder embeds speakers);
        ``transitions``: a TransitionModel for the programme with category
        transitions; ``window_frames``: that programme with the table in
        windows of so many ends."""
        if self.decoder.embed_speaker is not None and speaker is None:
            raise ValueError("this decoder embeds speakers: a speaker index is required")
        protos = self.prototypes_for([0 if speaker is None else int(speaker)], int(max_length))
        extra = dict(posteriors=True, temperature=temperature) if posteriors else {}
        if transitions is not None:
            extra["transitions"] = transitions
        if window_frames is not None:
            extra["window_frames"] = window_frames
        return segmentation.segment_frames(self.decoder, protos, frames.to(self.device), max_length,
                                           min_length=min_length, log_weight=log_weight, gap=gap, seg_bonus=seg_bonus,
                                           **extra)

    def segment_recording_warped(self, frames, steps, log_moves, min_state=0, log_weight=None, gap=None,
                                 seg_bonus=0.0, speaker=None, transitions=None, chunk_frames=None):
        """``segmentation.segment_frames_warped`` of one recording's frames under
        the categories' prototypes decoded for ``steps`` steps."""
        if self.decoder.embed_speaker is not None and speaker is None:
            raise ValueError("this decoder embeds speakers: a speaker index is required")
        protos = self.prototypes_for([0 if speaker is None else int(speaker)], int(steps))
        return segmentation.segment_frames_warped(self.decoder, protos, frames.to(self.device), int(steps),
                                                  log_moves=log_moves, transitions=transitions, log_weight=log_weight,
                                                  gap=gap, seg_bonus=seg_bonus, min_state=min_state,
                                                  chunk_frames=chunk_frames)

    def warp_posteriors(self, frames, steps, log_moves, min_state=0, log_weight=None, gap=None, seg_bonus=0.0,
                        speaker=None, transitions=None, chunk_frames=None, **kw):
        """``segmentation.segment_warp_posteriors`` of one recording's frames
        under the categories' prototypes decoded for ``steps`` steps."""
        if self.decoder.embed_speaker is not None and speaker is None:
            raise ValueError("this decoder embeds speakers: a speaker index is required")
        protos = self.prototypes_for([0 if speaker is None else int(speaker)], int(steps))
        return segmentation.segment_warp_posteriors(self.decoder, protos, frames.to(self.device), int(steps),
                                                    log_moves=log_moves, transitions=transitions,
                                                    log_weight=log_weight, gap=gap, seg_bonus=seg_bonus,
                                                    min_state=min_state, chunk_frames=chunk_frames, **kw)

    def chain_posteriors(self, frames, max_length, transitions, min_length=1, log_weight=None, gap=None,
                         seg_bonus=0.0, speaker=None, **kw):
        """``segmentation.segment_chain_posteriors`` of one recording's frames
        under the categories' prototypes and the TransitionModel ``transitions``."""
        if self.decoder.embed_speaker is not None and speaker is None:
            raise ValueError("this decoder embeds speakers: a speaker index is required")
        protos = self.prototypes_for([0 if speaker is None else int(speaker)], int(max_length))
        return segmentation.segment_chain_posteriors(self.decoder, protos, frames.to(self.device), max_length,
                                                     transitions, min_length=min_length, log_weight=log_weight,
                                                     gap=gap, seg_bonus=seg_bonus, **kw)


def get_parameters(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="Cut recordings into labelled segments with a trained ABCD-VAE's decoder "
                                            "(MI355X): span scores under every category and a semi-Markov cover.")
    cli.add_data_arguments(
        p, table="recording_table",
        table_help="table (csv) with an input_path column; an existing annotation works (its distinct paths)",
        save_help="output csv (default: <input_root>/segmented.csv); an existing file is kept as .prev",
        root_help="directory the table's wav paths are relative to", sep_help="field separator of the tables",
        batch=False)
    p.add_argument("--max_length", type=int, required=True, help="longest segment, frames")
    p.add_argument("--min_length", type=int, default=1,
                   help="shortest segment, frames (raised to the shortest the loader can featurise again)")
    cli.add_prior_arguments(
        p, prior_help="log weights of the categories: the Dirichlet posterior's E[log pi_k] (default) or zero",
        size_help="N of the Dirichlet posterior softmax(shape logits) * N + a0 (default: the table's rows)")
    p.add_argument("--segment_bonus", type=float, default=0.0,
                   help="log prior added per segment; negative values discourage over-segmentation")
    p.add_argument("--gap_score", type=float, default=None,
                   help="constant log-likelihood of a frame no segment covers (default: none, the segments tile "
                        "the recording)")
    p.add_argument("--gap_model", type=str, default=None,
                   help="npz with mu and log_var (F each): a diagonal Gaussian background for uncovered frames")
    p.add_argument("--fit_gap", type=str, default=None,
                   help="annotation table: fit the background from the frames its segments leave uncovered, write "
                        "it to --gap_model_out and use it")
    p.add_argument("--gap_model_out", type=str, default=None, help="where --fit_gap writes the npz")
    p.add_argument("--speaker", type=int, default=None,
                   help="speaker index; required when the decoder embeds speakers")
    p.add_argument("--posteriors", action="store_true",
                   help="also sum over every segmentation: append onset_posterior, offset_posterior and "
                        "span_posterior (how far to trust each cut) after segment_score")
    p.add_argument("--posterior_temperature", type=float, default=1.0,
                   help="divides the span scores, the gap scores and the bonus before the posteriors are formed; "
                        "above 1 softens them (the raw ones are almost all 0 or 1)")
    p.add_argument("--curves_dir", type=str, default=None,
                   help="with --posteriors: one npz per recording with the per-frame onset, end and gap posteriors, "
                        "log_evidence, fs and hop")
    p.add_argument("--recordings_out", type=str, default=None,
                   help="with --posteriors: csv with input_path, n_frames, n_segments, path_score, log_evidence, "
                        "expected_segments per recording")
    p.add_argument("--transitions", type=str, default=None,
                   help="a transitions.csv as sequence.py writes it: the categories of consecutive segments follow "
                        "this matrix inside the dynamic programme (initial distribution: softmax of the prior's log "
                        "weights); appends transition_score, context_free_category_ix and changed")
    p.add_argument("--refit_transitions", type=int, default=0,
                   help="iterations of Viterbi training of the matrix on the recordings before the final cut "
                        "(0: none); starts from --transitions, or from the context-free matrix")
    p.add_argument("--transitions_out", type=str, default=None,
                   help="where --refit_transitions writes the refitted matrix (transitions.csv's columns)")
    p.add_argument("--refit_method", type=str, default="viterbi", choices=REFIT_METHODS,
                   help="how --refit_transitions counts bigrams: those of each recording's best path (viterbi) or "
                        "the expected counts over every labelled cover (em); with em --transitions_out carries the "
                        "expected counts in expected_count")
    p.add_argument("--chain_posteriors", action="store_true",
                   help="with --transitions / --refit_transitions: also sum over every labelled segmentation under "
                        "the chain and append onset_posterior, offset_posterior, span_posterior and label_posterior; "
                        "--posterior_temperature, --curves_dir (which also holds each frame's most probable category "
                        "and its probability) and --recordings_out apply")
    p.add_argument("--window_frames", type=int, default=None,
                   help="with --transitions: build the per-category table in windows of this many end frames "
                        "instead of at once, for recordings whose whole table (8 (N + 1) max_length K bytes, (N + 1) "
                        "max_length K < 2^31) does not fit; the same segments bit for bit at a peak table memory of at "
                        "most 8 (W + max_length + 32) max_length K bytes whatever the recording's length; 1024 is a "
                        "good value")
    p.add_argument("--warp", action="store_true",
                   help="time-warp the prototypes inside the dynamic programme: --max_length is then the number of "
                        "prototype steps, and a segment may be shorter or longer than that; appends last_state and "
                        "tempo")
    cli.add_moves_argument(p, "with --warp: probabilities of advancing 0, 1 or 2 prototype steps per frame "
                              "(normalised; 0 disables a move; 0 1 0 is the rigid programme)")
    p.add_argument("--min_state", type=int, default=0,
                   help="with --warp: the lowest prototype step a segment may end in (raised so that every segment "
                        "has the frames the loader needs)")
    p.add_argument("--chunk_frames", type=int, default=None,
                   help="with --warp: frames of the emission plane built at a time, 4 chunk_frames max_length K bytes "
                        "(default: as many as fit 256 MiB); the result does not depend on it")
    p.add_argument("--warp_posteriors", action="store_true",
                   help="with --warp: also sum over every cover, labelling and alignment under the time-warped "
                        "programme and append onset_posterior, offset_posterior and occupancy (the mean probability "
                        "that the segment's frames lie in a segment of its category); --posterior_temperature, "
                        "--curves_dir and --recordings_out apply as with --chain_posteriors")
    p.add_argument("--warp_refit", type=int, default=0,
                   help="with --warp: iterations of EM on the recordings before the final cut (0: none): the moves "
                        "are refitted from their expected counts and written to --moves_out, and with --transitions "
                        "the matrix from its expected bigram counts, written to --transitions_out")
    p.add_argument("--moves_out", type=str, default=None,
                   help="where --warp_refit writes the refitted moves (csv: stay, step, skip probabilities)")
    p.add_argument("--keep_moves", action="store_true",
                   help="with --warp_refit: keep --moves as given and refit the matrix only")
    a = p.parse_args(argv)
    cli.check_moves_argument(p, a)
    if not a.warp and (a.warp_posteriors or a.warp_refit != 0):
        p.error("--warp_posteriors and --warp_refit need --warp")
    if a.warp_refit < 0:
        p.error("--warp_refit must not be negative")
    if a.warp_refit == 0 and (a.moves_out is not None or a.keep_moves):
        p.error("--moves_out and --keep_moves need --warp_refit")
    if a.warp_refit > 0:
        if a.keep_moves == (a.moves_out is not None):
            p.error("--warp_refit writes the refitted moves to --moves_out; give --moves_out, or --keep_moves to "
                    "fix the moves, not both")
        if a.keep_moves and a.transitions is None:
            p.error("--warp_refit with --keep_moves has nothing to fit without --transitions")
        if (a.transitions is not None) != (a.transitions_out is not None):
            p.error("--warp_refit refits the matrix of --transitions and writes it to --transitions_out: the two go "
                    "together")
    if a.warp:
        for flag, on in (("--posteriors", a.posteriors), ("--chain_posteriors", a.chain_posteriors),
                         ("--window_frames", a.window_frames is not None),
                         ("--refit_transitions", a.refit_transitions > 0)):
            if on:
                p.error(f"--warp cannot be combined with {flag}: the time-warped programme gives the best cut only "
                        "and needs no table in windows")
        if not 0 <= a.min_state < a.max_length:
            p.error("--min_state must lie in 0 .. --max_length - 1")
        if a.chunk_frames is not None and a.chunk_frames < 1:
            p.error("--chunk_frames must be at least 1")
    elif a.min_state != 0 or a.chunk_frames is not None or list(a.moves) != list(cli.DEFAULT_MOVES):
        p.error("--moves, --min_state and --chunk_frames need --warp")
    if a.window_frames is not None:
        if a.window_frames < 1:
            p.error("--window_frames must be at least 1")
        if a.transitions is None:
            p.error("--window_frames needs --transitions: it cuts the table of the programme under a transition model")
        if a.chain_posteriors:
            p.error("--window_frames cannot be combined with --chain_posteriors: the sum over every labelled cover "
                    "sweeps the whole table backwards and is not available in windows")
        if a.refit_transitions > 0 and a.refit_method == "em":
            p.error("--window_frames cannot be combined with --refit_method em: its expected counts come from the sum "
                    "over every labelled cover, which is not available in windows; use --refit_method viterbi")
    if a.chain_posteriors and a.transitions is None and a.refit_transitions <= 0:
        p.error("--chain_posteriors needs --transitions or --refit_transitions")
    if a.refit_method != "viterbi" and a.refit_transitions <= 0:
        p.error("--refit_method needs --refit_transitions")
    if a.refit_transitions < 0:
        p.error("--refit_transitions must not be negative")
    if a.warp_refit <= 0 and (a.refit_transitions > 0) != (a.transitions_out is not None):
        p.error("--refit_transitions and --transitions_out go together")
    if a.posteriors and (a.transitions is not None or a.refit_transitions > 0):
        p.error("--transitions / --refit_transitions cannot be combined with --posteriors: posteriors under a "
                "transition model are not available")
    if not a.posterior_temperature > 0:
        p.error("--posterior_temperature must be positive")
    if not (a.posteriors or a.chain_posteriors or a.warp_posteriors) and (a.posterior_temperature != 1.0 or a.curves_dir is not None
                                                     or a.recordings_out is not None):
        p.error("--posterior_temperature, --curves_dir and --recordings_out need --posteriors")
    if a.max_length < 1 or a.max_length > 16383:
        p.error("--max_length must lie in 1 .. 16383")
    if a.min_length < 1 or a.min_length > a.max_length:
        p.error("--min_length must lie in 1 .. --max_length")
    cli.check_prior_arguments(p, a)
    if sum(v is not None for v in (a.gap_score, a.gap_model, a.fit_gap)) > 1:
        p.error("--gap_score, --gap_model and --fit_gap exclude one another")
    if (a.fit_gap is None) != (a.gap_model_out is None):
        p.error("--fit_gap and --gap_model_out go together")
    return a


def main(argv=None):
    a = get_parameters(argv)
    save_path = a.save_path or os.path.join(a.input_root, "segmented.csv")
    for path in (save_path, a.gap_model_out, a.recordings_out, a.transitions_out, a.moves_out):
        if path and os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
    if a.curves_dir:
        os.makedirs(a.curves_dir, exist_ok=True)
    table = pd.read_csv(a.recording_table, sep=a.annotation_sep)
    if "input_path" not in table.columns:
        raise SystemExit(f"{a.recording_table}: no input_path column")
    paths = list(dict.fromkeys(table["input_path"].tolist()))
    seg = Segmenter(a.model_path, device=a.device)
    if seg.decoder.embed_speaker is not None and a.speaker is None:
        raise SystemExit("this checkpoint's decoder embeds speakers: --speaker is required")
    centering = not a.fft_no_centering
    spectrum = {}

    def featurise(path):
        fs, wave = read_wave(a.input_root, path, a.channel)
        frame, hop = cli.frame_hop(a, fs)
        if (frame, hop) not in spectrum:
            spectrum[frame, hop] = cli.log_spectrum(a, frame, hop)
        return fs, frame, hop, len(wave), spectrum[frame, hop](torch.from_numpy(wave)).to(seg.device)

    gap_model = None
    if a.fit_gap is not None:
        ann = pd.read_csv(a.fit_gap, sep=a.annotation_sep)
        kept = []
        for path, sub in ann.groupby("input_path"):
            fs, frame, hop, _, frames = featurise(path)
            mask = covered_frames(frames.shape[0], sub.onset.to_numpy(), sub.offset.to_numpy(), fs, frame, hop,
                                  centering)
            kept.append(frames[torch.from_numpy(~mask).to(frames.device)])
        kept = torch.cat(kept)
        gap_model = segmentation.fit_gap_model(kept, torch.zeros(kept.shape[0], dtype=torch.bool))
        np.savez(a.gap_model_out, mu=gap_model[0].cpu().numpy(), log_var=gap_model[1].cpu().numpy())
    elif a.gap_model is not None:
        with np.load(a.gap_model) as z:
            gap_model = (torch.from_numpy(z["mu"]), torch.from_numpy(z["log_var"]))

    lw = seg.log_weight(a.prior, len(table) if a.entire_data_size is None else a.entire_data_size)
    syntax = a.transitions is not None or a.refit_transitions > 0
    model, trans_table, prepared, warned = None, None, {}, []
    log_moves = alignment.moves_from_probabilities(a.moves) if a.warp else None

    def prepare(path):
        if path in prepared:
            return prepared[path]
        fs, frame, hop, total, frames = featurise(path)
        d_min = max(a.min_length, min_loadable_length(frame, hop, centering))
        if d_min > a.min_length:
            print(f"{path}: --min_length raised from {a.min_length} to {d_min} frames, the shortest segment the "
                  "loader can featurise", file=sys.stderr)
        if d_min > a.max_length:
            raise SystemExit(f"{path}: --max_length {a.max_length} is below the shortest loadable segment ({d_min})")
        gap = None
        if a.gap_score is not None:
            gap = torch.full((frames.shape[0],), float(a.gap_score), device=seg.device)
        elif gap_model is not None:
            gap = segmentation.gap_scores(frames, *gap_model)
        got = (fs, frame, hop, total, frames, d_min, gap)
        if a.refit_transitions > 0 or a.warp_refit > 0:     # the training passes and the final cut share the features
            prepared[path] = got
        return got

    def warp_min_state(path, d_min):
        """--min_state raised so that every segment has the d_min frames the loader needs."""
        # a segment that ends in state s has at least s / (the largest advance) + 1 frames
        stride = 2 if a.moves[2] > 0 else 1
        s_min = max(a.min_state, stride * (d_min - 1))
        if s_min > a.min_state and not warned:
            warned.append(s_min)
            print(f"--min_state raised from {a.min_state} to {s_min}: every segment then has the {d_min} frames "
                  "the loader can featurise", file=sys.stderr)
        if s_min >= a.max_length:
            raise SystemExit(f"{path}: --max_length {a.max_length} leaves no state >= {s_min} to end in")
        return s_min

    def cut(path, transitions=None, got=None):
        _, _, _, _, frames, d_min, gap = got or prepare(path)
        if a.warp:
            return seg.segment_recording_warped(frames, a.max_length, log_moves,
                                                min_state=warp_min_state(path, d_min), log_weight=lw, gap=gap,
                                                seg_bonus=a.segment_bonus, speaker=a.speaker, transitions=transitions,
                                                chunk_frames=a.chunk_frames)
        return seg.segment_recording(frames, a.max_length, min_length=d_min, log_weight=lw, gap=gap,
                                     seg_bonus=a.segment_bonus, speaker=a.speaker, posteriors=a.posteriors,
                                     temperature=a.posterior_temperature, transitions=transitions,
                                     window_frames=a.window_frames if transitions is not None else None)

    def posterior(path, transitions, got=None, **kw):
        _, _, _, _, frames, d_min, gap = got or prepare(path)
        return seg.chain_posteriors(frames, a.max_length, transitions, min_length=d_min, log_weight=lw, gap=gap,
                                    seg_bonus=a.segment_bonus, speaker=a.speaker, **kw)

    def warp_posterior(path, transitions, moves, got=None, **kw):
        _, _, _, _, frames, d_min, gap = got or prepare(path)
        return seg.warp_posteriors(frames, a.max_length, moves, min_state=warp_min_state(path, d_min), log_weight=lw,
                                   gap=gap, seg_bonus=a.segment_bonus, speaker=a.speaker, transitions=transitions,
                                   chunk_frames=a.chunk_frames, **kw)

    if syntax:
        import sequence
        from modules.sequence import TransitionModel
        K = int(lw.numel())
        model = TransitionModel.from_log_weight(lw)
        if a.transitions is not None:
            model.set_probabilities(sequence.load_transitions(a.transitions, K), torch.softmax(lw.double(), 0))
        if a.refit_transitions > 0 and a.refit_method == "em":
            totals = segmentation.refit_transitions_em(lambda path, m: posterior(path, m, want_counts=True), paths,
                                                       model, a.refit_transitions, 1.0 / K)
            for i, v in enumerate(totals):
                print(f"refit iteration {i}: log posterior of the matrix {v:.6f}", file=sys.stderr)
        elif a.refit_transitions > 0:
            totals = segmentation.refit_transitions(cut, paths, model, a.refit_transitions, 1.0 / K)
            for i, v in enumerate(totals):
                print(f"refit iteration {i}: summed path score {v:.6f}", file=sys.stderr)
        if a.warp_refit > 0:
            totals, log_moves = segmentation.refit_warp_em(
                lambda path, m, moves: warp_posterior(path, m, moves, want_counts=True, want_moves=not a.keep_moves),
                paths, model, log_moves, a.warp_refit, 1.0 / K, fit_moves=not a.keep_moves)
            for i, v in enumerate(totals):
                print(f"warp refit iteration {i}: log posterior of the matrix and the moves {v:.6f}", file=sys.stderr)
        if a.refit_transitions > 0 or a.warp_refit > 0:
            ft, tt = np.divmod(np.arange(K * K), K)
            trans_table = pd.DataFrame({"from_ix": ft, "to_ix": tt,
                                        "probability": model.log_trans.double().exp().reshape(-1).cpu().numpy(),
                                        "expected_count": model.last_counts[0].reshape(-1).cpu().numpy()},
                                       columns=list(TRANSITION_COLUMNS))

    if a.warp_refit > 0 and not syntax:
        totals, log_moves = segmentation.refit_warp_em(
            lambda path, m, moves: warp_posterior(path, m, moves, want_moves=True), paths, None, log_moves,
            a.warp_refit, 0.0)
        for i, v in enumerate(totals):
            print(f"warp refit iteration {i}: summed log evidence {v:.6f}", file=sys.stderr)

    rows, recordings, curves = [], [], {}
    for path in paths:
        got = prepare(path)
        fs, frame, hop, total, frames, d_min, _ = got
        post = None
        if a.chain_posteriors:
            post = posterior(path, model, got, temperature=a.posterior_temperature, with_segments=True)
            out = post["segmentation"]
        elif a.warp_posteriors:
            post = warp_posterior(path, model, log_moves, got, temperature=a.posterior_temperature,
                                  with_segments=True)
            out = post["segmentation"]
        else:
            out = cut(path, model, got)
        if not bool(out["path_score"] > float("-inf")):
            print(f"{path}: no cover of its {frames.shape[0]} frames by segments of {d_min} .. {a.max_length} "
                  "frames (give a gap score or model)", file=sys.stderr)
        first = table[table["input_path"] == path].iloc[0]
        speaker = first["speaker"] if "speaker" in table.columns else (
            float("nan") if a.speaker is None else a.speaker)
        data_type = first["data_type"] if "data_type" in table.columns else "segmented"
        rows += segment_rows(path, out["onset"].tolist(), out["length"].tolist(), out["category"].tolist(),
                             out["score"].tolist(), fs, frame, hop, centering, total, data_type=data_type,
                             speaker=speaker,
                             posteriors=[out[c].tolist() for c in POSTERIOR_COLUMNS] if a.posteriors else None,
                             syntax=(out["link"].tolist(), out["context_free_category"].tolist())
                             if syntax and not a.warp else None,
                             warp=(out["last_state"].tolist(), out["tempo"].tolist(),
                                   out["link"].tolist() if syntax else None) if a.warp else None,
                             warp_posteriors=[post[c].tolist() for c in ("onset_posterior", "end_posterior",
                                                                         "occupancy")] if a.warp_posteriors else None,
                             chain_posteriors=None if post is None or a.warp_posteriors else [
                                 post["onset"][out["onset"]].tolist(),
                                 post["end"][out["onset"] + out["length"]].tolist(),
                                 post["span_posterior"].tolist(), post["label_posterior"].tolist()])
        if post is not None:
            recordings.append({"input_path": path, "n_frames": int(frames.shape[0]), "n_segments": len(out["onset"]),
                               "path_score": float(out["path_score"]), "log_evidence": float(post["log_evidence"]),
                               "expected_segments": float(post["expected_segments"])})
            if a.curves_dir:
                prob, label = post["frame_category"].max(1)
                curves[curve_path(a.curves_dir, path)] = dict(
                    onset=post["onset"].cpu().numpy(), end=post["end"].cpu().numpy(), gap=post["gap"].cpu().numpy(),
                    frame_category=label.cpu().numpy(), frame_category_probability=prob.cpu().numpy(),
                    log_evidence=float(post["log_evidence"]), fs=fs, hop=hop)
        if a.posteriors:
            recordings.append({"input_path": path, "n_frames": int(frames.shape[0]), "n_segments": len(out["onset"]),
                               "path_score": float(out["path_score"]), "log_evidence": float(out["log_evidence"]),
                               "expected_segments": float(out["expected_segments"])})
            if a.curves_dir:
                on, end, gp = out["curves"].cpu().numpy()
                curves[curve_path(a.curves_dir, path)] = dict(onset=on, end=end, gap=gp,
                                                              log_evidence=float(out["log_evidence"]), fs=fs, hop=hop)
    _native.op_status.sync("segment")
    write_segments(save_path, rows, posteriors=a.posteriors, recordings_out=a.recordings_out, recordings=recordings,
                   curves=curves, syntax=syntax, transitions_out=a.transitions_out, transitions=trans_table,
                   chain_posteriors=a.chain_posteriors, warp=a.warp, warp_posteriors=a.warp_posteriors,
                   moves_out=a.moves_out if a.warp_refit > 0 and not a.keep_moves else None,
                   moves=None if log_moves is None else [float(np.exp(m)) for m in log_moves])
    return save_path


if __name__ == "__main__":
    main()
