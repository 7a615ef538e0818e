# coding: utf-8
"""Time-warped classification on the HIP path: is this segment another
category, or the same one at a different tempo?

``classify.py`` scores frame t of a segment against step t of each category's
prototype.  This script aligns first: the prototype's steps are the states of a
left-to-right HMM, frame t sits on state a(t), a(0) = 0 and a(t + 1) - a(t) is
0, 1 or 2 (stay, step, skip) with probabilities ``--moves``; ``warp_nll[b, k]``
is the NLL of segment b under its best alignment to category k (``--marginal``:
under all alignments), and the best path to the winning category gives the
segment's tempo (``RNN_Variational_Decoder.warp_against`` / ``align_to``,
``modules/alignment.py``).  ``--moves 0 1 0`` is ``classify.py``'s comparison.

Same checkpoint, annotation and STFT arguments and the same loader as
``classify.py``.  Prototypes are decoded for ``ceil(proto_factor * T)`` steps,
T the longest segment of the batch.  Output: a CSV with one row per segment,

``data_ix, length, category_ix, category_prob, warp_category_ix, warp_nll,
warp_log_evidence, warp_best_prob, end_state, tempo, n_stay, n_skip``

followed by the annotation columns as ``encode.py`` appends them.
``category_ix`` / ``category_prob`` are the encoder's argmax and its softmax
probability; ``warp_category_ix`` / ``warp_best_prob`` the argmax of ``q*(k)``
proportional to ``exp(log_weight_k - warp_nll[b, k])`` and its value,
``warp_log_evidence`` its log normaliser, ``warp_nll`` the winner's entry;
``end_state`` the prototype step of the last frame, ``tempo = (end_state + 1)
/ length`` (1: the prototype's pace, below 1: slower), ``n_stay`` / ``n_skip``
the moves of 0 and 2 steps on the path.  ``--paths PATH`` also writes one row
per frame, ``data_ix, frame, state``.  ``--fit_moves N`` first runs N rounds of
aligning the whole table and refitting the move probabilities from the paths'
move counts (hard EM), and prints each round's probabilities."""
import math
import os

import numpy as np
import torch

import classify
import cli
import score
from modules import _native, alignment

COLUMNS = ("data_ix", "length", "category_ix", "category_prob", "warp_category_ix", "warp_nll", "warp_log_evidence",
           "warp_best_prob", "end_state", "tempo", "n_stay", "n_skip")
TABLE = (("length", np.int64), ("category_ix", np.int64), ("category_prob", np.float64),
         ("warp_category_ix", np.int64), ("warp_nll", np.float64), ("warp_log_evidence", np.float64),
         ("warp_best_prob", np.float64), ("end_state", np.int64), ("tempo", np.float64), ("n_stay", np.int64),
         ("n_skip", np.int64))
PATH_COLUMNS = ("data_ix", "frame", "state")
PATHS = (("frame", np.int64), ("state", np.int64))
DEFAULT_MOVES = cli.DEFAULT_MOVES


class Aligner(classify.Classifier):
    """A trained ABCD checkpoint opened for time-warped classification."""

    def align_batch(self, packed, is_offset, speaker, log_weight, log_moves, band=None, marginal=False,
                    proto_factor=1.5, paths=False):
        """One batch -> {column: B values in the batch's packed row order} (every
        column of COLUMNS but data_ix), ``move_counts`` (3) and under "long" the
        per-frame rows when asked for."""
        dev = self.device
        K = self.feature_sampler.num_categories
        with torch.no_grad():
            data = packed.data.to(dev, non_blocking=True)
            bsz = packed.batch_sizes
            is_off = is_offset.data.to(dev, non_blocking=True)
            B, T = int(bsz[0]), int(bsz.numel())
            logits = self.feature_sampler(self.encoder(torch.nn.utils.rnn.PackedSequence(data, bsz)))
            cat_prob, cat = torch.softmax(logits.double(), -1).max(-1)
            if self.decoder.embed_speaker is not None:
                spk = torch.as_tensor(speaker, dtype=torch.int64).cpu()
                present, own = torch.unique(spk, sorted=True, return_inverse=True)
            else:
                present, own = torch.zeros(1, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)
            steps = max(1, int(math.ceil(proto_factor * T)))
            protos = tuple(t[:steps] for t in self.prototypes_for(present.tolist(), steps))  # exactly `steps` states
            cols = None
            if len(present) > 1:  # each segment's K columns under its own speaker
                cols = (own.to(dev) * K)[:, None] + torch.arange(K, device=dev)[None, :]
            r = alignment.align_segments(self.decoder, protos, bsz, data, is_off, log_weight=log_weight,
                                         log_moves=log_moves, band=band, marginal=marginal, columns=cols)
            n_step = r["length"] - 1 - r["n_stay"] - r["n_skip"]
            out = {"length": r["length"], "category_ix": cat, "category_prob": cat_prob,
                   "warp_category_ix": r["best"], "warp_nll": r["warp_nll"].double(),
                   "warp_log_evidence": r["log_evidence"].double(), "warp_best_prob": r["best_prob"].double(),
                   "end_state": r["end_state"], "tempo": r["tempo"], "n_stay": r["n_stay"], "n_skip": r["n_skip"],
                   "move_counts": torch.stack([r["n_stay"], torch.where(r["end_state"] >= 0, n_step, 0 * n_step),
                                               r["n_skip"]], 1).sum(0)}
            if paths:  # packed rows: step-major, segment b of step t at off_t + b
                out["long"] = {"row": torch.cat([torch.arange(int(n)) for n in bsz.tolist()]),
                               "frame": torch.repeat_interleave(torch.arange(T), bsz), "state": r["states"]}
            return out

    def align_dataset(self, dataset, save_path, batch_size=1, prior="dirichlet", entire_data_size=None,
                      moves=DEFAULT_MOVES, band=None, marginal=False, proto_factor=1.5, fit_rounds=0,
                      paths_path=None, smoothing=1.0):
        """Writes the table (and the per-frame paths) -> (rows written, the log_moves used)."""
        from modules import data_utils
        n = len(dataset) if entire_data_size is None else entire_data_size
        lw = self.log_weight(prior, n)
        log_moves = alignment.moves_from_probabilities(moves)
        for rnd in range(int(fit_rounds)):
            counts = torch.zeros(3, dtype=torch.int64)
            for packed, is_offset, speaker, _ixs in data_utils.DataLoader(dataset, batch_size=batch_size,
                                                                          shuffle=False):
                counts += self.align_batch(packed, is_offset, speaker, lw, log_moves, band=band, marginal=marginal,
                                           proto_factor=proto_factor)["move_counts"].cpu()
            log_moves = alignment.moves_from_counts(counts, smoothing, log_moves)
            print(f"fit_moves round {rnd + 1}: counts {counts.tolist()} -> stay / step / skip = "
                  + " ".join(f"{math.exp(v):.4f}" for v in log_moves))
        written = score.score_table(
            lambda p, o, s: self.align_batch(p, o, s, lw, log_moves, band=band, marginal=marginal,
                                             proto_factor=proto_factor, paths=paths_path is not None),
            dataset, save_path, batch_size=batch_size, finish=lambda: _native.op_status.sync("align_dataset"),
            columns=TABLE, long_path=paths_path, long_columns=PATHS)
        return written, log_moves


def get_parameters(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="Align annotated segments to every category of a trained ABCD-VAE "
                                            "(MI355X): time-warped classification, tempo and per-frame paths.")
    cli.add_data_arguments(p, table_help="annotation table (csv) of the segments to align",
                           save_help="output csv (default: <input_root>/aligned.csv); an existing file is kept as "
                                     ".prev")
    cli.add_prior_arguments(
        p, prior_help="log weights of the categories: the Dirichlet posterior's E[log pi_k] (default) or zero",
        size_help="N of the Dirichlet posterior softmax(shape logits) * N + a0 (default: the number of segments)")
    cli.add_moves_argument(p, "probabilities of advancing 0, 1 or 2 prototype steps per frame (normalised; 0 disables "
                              "a move; 0 1 0 is classify.py's rigid comparison)")
    p.add_argument("--band", type=int, default=None, help="only alignments with |step - frame| <= N (default: no band)")
    p.add_argument("--marginal", action="store_true",
                   help="sum over all alignments instead of taking the best one (paths stay the best ones)")
    p.add_argument("--proto_factor", type=float, default=1.5,
                   help="prototypes are decoded for ceil(factor * T) steps, T the longest segment of a batch")
    p.add_argument("--fit_moves", type=int, default=0, metavar="N",
                   help="first run N rounds of aligning the table and refitting --moves from the paths (hard EM)")
    p.add_argument("--paths", type=str, default=None, help="also write one row per frame (data_ix, frame, state) here")
    a = p.parse_args(argv)
    cli.check_prior_arguments(p, a)
    cli.check_moves_argument(p, a)
    if a.band is not None and a.band < 0:
        p.error("--band must not be negative")
    if not a.proto_factor > 0:
        p.error("--proto_factor must be positive")
    if a.fit_moves < 0:
        p.error("--fit_moves must not be negative")
    return a


def main(argv=None):
    a = get_parameters(argv)
    save_path = a.save_path or os.path.join(a.input_root, "aligned.csv")
    for path in (save_path, a.paths):
        if path and os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
    dataset = cli.open_dataset(a)
    Aligner(a.model_path, device=a.device).align_dataset(
        dataset, save_path, batch_size=a.batch_size, prior=a.prior, entire_data_size=a.entire_data_size,
        moves=a.moves, band=a.band, marginal=a.marginal, proto_factor=a.proto_factor, fit_rounds=a.fit_moves,
        paths_path=a.paths)
    return save_path


if __name__ == "__main__":
    main()
