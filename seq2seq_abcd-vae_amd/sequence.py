# coding: utf-8
"""Context-aware labels on the HIP path: a hidden Markov model over the
category sequence of every recording.

``classify.py`` scores every segment against every category, ``nll[b, k] = -log
p(x_b | z = c_k)``, and labels each segment on its own.  This script treats
those scores as the emission term of a hidden Markov model whose states are
the K categories (``modules.sequence.TransitionModel``): the annotation is cut
into sequences (``--sequence_columns``, ``--max_gap``), the transition matrix is
fitted by EM (``--em_iterations``, ``--pseudo_count``) starting from the
context-free model whose rows all equal ``softmax(log_weight)`` (``--prior``, as
in ``classify.py``), and every segment is labelled again by the forward-backward
posterior and by Viterbi (``abcd_chain_posterior``).

Same checkpoint, annotation and STFT arguments and the same loader as
``classify.py``.  Output, in the directory ``-S`` (default: the input root):

``sequenced.csv``    one row per segment: ``data_ix, sequence_ix, position,
                     decoder_category_ix, smoothed_category_ix,
                     smoothed_category_prob, viterbi_category_ix, changed`` and
                     the annotation columns; ``decoder_category_ix`` is
                     ``classify.py``'s context-free label, ``changed`` whether the
                     Viterbi label differs from it
``transitions.csv``  ``from_ix, to_ix, probability, expected_count``: the fitted
                     matrix and the expected number of transitions
``sequences.csv``    ``sequence_ix, length, log_evidence,
                     context_free_log_evidence``: the evidence under the chain in
                     ``classify.py``'s units (with the context-free chain the two
                     columns agree) and the sum of ``classify.py``'s per-segment
                     evidence
"""
import os

import numpy as np
import pandas as pd
import torch

import classify
import cli
from modules import _native, data_utils, ops
from modules.sequence import TransitionModel, split_sequences

COLUMNS = ("data_ix", "sequence_ix", "position", "decoder_category_ix", "smoothed_category_ix",
           "smoothed_category_prob", "viterbi_category_ix", "changed")
TRANSITION_COLUMNS = ("from_ix", "to_ix", "probability", "expected_count")
SEQUENCE_COLUMNS = ("sequence_ix", "length", "log_evidence", "context_free_log_evidence")
FILES = ("sequenced.csv", "transitions.csv", "sequences.csv")


class Sequencer(classify.Classifier):
    """``classify.Classifier`` keeping every segment's normalised scores on the
    device, for the chain to run over."""

    def score_dataset(self, dataset, batch_size, log_weight):
        """-> dict(score n x K fp32, row_offset n fp64, best n int64, evidence n
        fp64) on the device, indexed by data_ix: the scores without the
        weights (the chain carries them), ``classify.py``'s label and evidence."""
        n, K = len(dataset), self.feature_sampler.num_categories
        dev = self.device
        score = torch.empty(n, K, device=dev)
        row_off = torch.empty(n, dtype=torch.float64, device=dev)
        best = torch.empty(n, dtype=torch.int64, device=dev)
        ev = torch.empty(n, dtype=torch.float64, device=dev)
        for packed, is_offset, speaker, ixs in data_utils.DataLoader(dataset, batch_size=batch_size, shuffle=False):
            out = self.classify_batch(packed, is_offset, speaker, log_weight, matrix=True)
            ix = torch.as_tensor(np.asarray(ixs, dtype=np.int64), device=dev)
            B = ix.numel()
            em = out["long"]["emission_nll"].reshape(K, B).t()
            off = out["long"]["end_prediction_loss"].reshape(K, B).t()
            score[ix], row_off[ix] = ops.chain_scores(em, off)
            best[ix], ev[ix] = out["decoder_category_ix"], out["log_evidence"]
        _native.op_status.sync("sequence.py")
        return dict(score=score, row_offset=row_off, best=best, evidence=ev)


def load_transitions(path, K):
    """transitions.csv -> the K x K probability matrix (rows renormalised)."""
    df = pd.read_csv(path)
    if len(df) != K * K:
        raise SystemExit(f"{path}: {len(df)} rows, expected {K} x {K}")
    m = np.zeros((K, K))
    m[df["from_ix"].to_numpy(), df["to_ix"].to_numpy()] = df["probability"].to_numpy()
    return m / m.sum(1, keepdims=True)


def run(seqr, dataset, save_dir, batch_size=1, prior="dirichlet", entire_data_size=None, em_iterations=10,
        pseudo_count=None, max_gap=None, sequence_columns=("input_path",), transitions=None):
    n = len(dataset)
    K = seqr.feature_sampler.num_categories
    lw = seqr.log_weight(prior, n if entire_data_size is None else entire_data_size)
    got = seqr.score_dataset(dataset, batch_size, lw)
    ann = dataset.df_annotation
    order, seq_off = split_sequences(ann, by=sequence_columns, max_gap=max_gap)
    S = len(seq_off) - 1
    order_d = torch.as_tensor(order, device=seqr.device)
    score = got["score"][order_d].contiguous()
    model = TransitionModel.from_log_weight(lw)
    if transitions is not None:
        model.set_probabilities(load_transitions(transitions, K), torch.softmax(lw.double(), 0))
    elif em_iterations > 0:
        model.fit(score, seq_off, n_iter=em_iterations, pseudo_count=pseudo_count)
    post = model.posterior(score, seq_off, counts=True)
    path, _ = model.viterbi(score, seq_off)
    prob, smooth = post["gamma"].max(1)
    lens = np.diff(seq_off)
    seq_ix = np.repeat(np.arange(S), lens)
    seq_d = torch.as_tensor(seq_ix, device=seqr.device)
    zero = torch.zeros(S, dtype=torch.float64, device=seqr.device)
    # the chain's evidence in classify.py's units: the rows' offsets and logsumexp(log_weight) per segment
    units = got["row_offset"][order_d] + torch.logsumexp(lw.double(), 0)
    ev = post["log_evidence"] + zero.index_add(0, seq_d, units)
    cf = zero.index_add(0, seq_d, got["evidence"][order_d])
    best = got["best"][order_d].cpu().numpy()
    vit = path.cpu().numpy().astype(np.int64)
    seg = pd.DataFrame({"data_ix": order, "sequence_ix": seq_ix,
                        "position": np.arange(len(order)) - np.repeat(seq_off[:-1], lens),
                        "decoder_category_ix": best, "smoothed_category_ix": smooth.cpu().numpy(),
                        "smoothed_category_prob": prob.double().cpu().numpy(), "viterbi_category_ix": vit,
                        "changed": (vit != best).astype(np.int64)})
    seg = cli.join_annotation(seg, cli.annotation_columns(dataset))
    ft, tt = np.divmod(np.arange(K * K), K)
    tr = pd.DataFrame({"from_ix": ft, "to_ix": tt,
                       "probability": model.log_trans.double().exp().reshape(-1).cpu().numpy(),
                       "expected_count": post["trans_counts"].reshape(-1).cpu().numpy()})
    sq = pd.DataFrame({"sequence_ix": np.arange(S), "length": lens, "log_evidence": ev.cpu().numpy(),
                       "context_free_log_evidence": cf.cpu().numpy()})
    _native.op_status.sync("sequence.py")
    tables = dict(zip(FILES, (seg, tr, sq)))
    with cli.replacing_outputs() as tmp:  # every table is complete before any earlier one is moved aside
        for name, table in tables.items():
            table.to_csv(tmp(os.path.join(save_dir, name)), index=False)
    return tables


def get_parameters(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="Label annotated segments in context (MI355X): a hidden Markov model over "
                                            "the category sequence of every recording, fitted by EM.")
    cli.add_data_arguments(p, table_help="annotation table (csv) of the segments to label",
                           save_help="output directory (default: <input_root>); existing tables are kept as .prev")
    cli.add_prior_arguments(
        p, prior_help="the initial, context-free model: every row softmax of the Dirichlet posterior's E[log pi_k] "
                      "(default) or uniform",
        size_help="N of the Dirichlet posterior softmax(shape logits) * N + a0 (default: the number of segments)")
    p.add_argument("--em_iterations", type=int, default=10, help="EM iterations of the transition matrix (0: none)")
    p.add_argument("--pseudo_count", type=float, default=None,
                   help="added to every expected count in the M-step (default: 1 / K)")
    p.add_argument("--max_gap", type=float, default=None,
                   help="a silence longer than this many seconds starts a new sequence (default: never)")
    p.add_argument("--sequence_columns", type=str, nargs="+", default=["input_path"],
                   help="annotation columns whose values delimit a sequence")
    p.add_argument("--transitions", type=str, default=None,
                   help="a transitions.csv to load instead of fitting one")
    a = p.parse_args(argv)
    cli.check_prior_arguments(p, a)
    if a.em_iterations < 0:
        p.error("--em_iterations must not be negative")
    if a.pseudo_count is not None and not a.pseudo_count >= 0:
        p.error("--pseudo_count must not be negative")
    if a.max_gap is not None and not a.max_gap >= 0:
        p.error("--max_gap must not be negative")
    return a


def main(argv=None):
    a = get_parameters(argv)
    save_dir = a.save_path or a.input_root
    os.makedirs(save_dir, exist_ok=True)
    dataset = cli.open_dataset(a)
    run(Sequencer(a.model_path, device=a.device), dataset, save_dir, batch_size=a.batch_size, prior=a.prior,
        entire_data_size=a.entire_data_size, em_iterations=a.em_iterations, pseudo_count=a.pseudo_count,
        max_gap=a.max_gap, sequence_columns=tuple(a.sequence_columns), transitions=a.transitions)
    return save_dir


if __name__ == "__main__":
    main()
