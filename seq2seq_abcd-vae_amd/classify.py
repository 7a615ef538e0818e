# coding: utf-8
"""Decoder-side classification on the HIP path: how well does each category
explain each annotated segment?

``encode.py`` writes the encoder's posterior over the categories and
``score.py`` a segment's losses under that posterior; this script scores every
segment against every category, ``nll[b, k] = -log p(x_b | z = c_k)``.  The
decoder feeds back its own output and never sees the ground truth, so with its
mean fed back the emission parameters under category k depend on (codebook
column k, speaker, step) only: the K categories (times the speakers present in
a batch) are decoded once as a rectangle
(``RNN_Variational_Decoder.prototypes``) and every segment is scored against
every one of them (``score_against``).  The categorical posterior that maximises
the ELBO for this decoder is ``q*(k | x_b)`` proportional to ``exp(log_weight_k
- nll[b, k])`` (``ops.pair_posterior``), with ``log_weight`` the Dirichlet
posterior's ``E[log pi_k]`` (``--prior dirichlet``,
``ABCDSampler.expected_log_prior``) or zero (``--prior uniform``).

Same checkpoint, annotation and STFT arguments and the same loader as
``score.py`` (ABCD checkpoints only; one device).  Output: a CSV with one row
per segment,

``data_ix, length, category_ix, category_prob, decoder_category_ix,
decoder_category_prob, log_evidence, agree``

followed by the annotation columns as ``encode.py`` appends them.
``category_ix`` / ``category_prob`` are the encoder's argmax and its softmax
probability, ``decoder_category_ix`` / ``decoder_category_prob`` the argmax of
``q*`` and its value, ``log_evidence = logsumexp_k(log_weight_k - nll[b, k])``
the segment's evidence bound, ``agree`` whether the two argmaxes coincide.
``--matrix PATH`` also writes the long table ``data_ix, category_ix,
emission_nll, end_prediction_loss, log_weight, responsibility`` (``nll`` is the
sum of the two losses), category-major within a batch as ``encode.py`` orders
its rows."""
import os

import numpy as np
import torch

import cli
import score
from cli import PRIORS
from modules import _native, ops

COLUMNS = ("data_ix", "length", "category_ix", "category_prob", "decoder_category_ix", "decoder_category_prob",
           "log_evidence", "agree")
TABLE = (("length", np.int64), ("category_ix", np.int64), ("category_prob", np.float64),
         ("decoder_category_ix", np.int64), ("decoder_category_prob", np.float64), ("log_evidence", np.float64),
         ("agree", np.int64))
MATRIX_COLUMNS = ("data_ix", "category_ix", "emission_nll", "end_prediction_loss", "log_weight", "responsibility")
MATRIX = (("category_ix", np.int64), ("emission_nll", np.float64), ("end_prediction_loss", np.float64),
          ("log_weight", np.float64), ("responsibility", np.float64))


class Classifier(score.Scorer):
    """A trained ABCD checkpoint opened for decoder-side classification
    (parameters frozen, modules in eval mode; a plain checkpoint exits)."""

    def __init__(self, model_config_path, device="cuda"):
        super().__init__(model_config_path, device=device)
        self._protos = {}  # speaker set -> (prototypes, steps decoded)

    def log_weight(self, prior, entire_data_size):
        K = self.feature_sampler.num_categories
        if prior == "uniform":
            return torch.zeros(K, device=self.device)
        if prior != "dirichlet":
            raise ValueError(f"prior: one of {PRIORS}, not {prior!r}")
        return self.feature_sampler.expected_log_prior(entire_data_size)

    def prototypes_for(self, speakers, length):
        """The prototypes of every (speaker, category), speaker-major (column
        ``i * K + k`` for the i-th of ``speakers``), decoded for at least
        ``length`` steps.  Cached per speaker set: decoded again only for a
        batch longer than the cached rectangle."""
        key = tuple(int(s) for s in speakers)
        have = self._protos.get(key)
        if have is None or have[1] < length:
            feats = self.feature_sampler.codebook.detach().t().contiguous()  # K x D: decode.py's category_features
            K = feats.shape[0]
            spk = None
            if self.decoder.embed_speaker is not None:
                spk = torch.tensor(key, dtype=torch.int64, device=self.device).repeat_interleave(K)
            have = (self.decoder.prototypes(feats.repeat(len(key), 1), length, speaker=spk), int(length))
            self._protos[key] = have
        return have[0]

    def classify_batch(self, packed, is_offset, speaker, log_weight, matrix=False):
        """One batch -> {column: B device values in the batch's packed row
        order} (every column of COLUMNS but data_ix), and under "long" the
        B * K rows of the matrix table when asked for."""
        dev = self.device
        K = self.feature_sampler.num_categories
        with torch.no_grad():
            data = packed.data.to(dev, non_blocking=True)
            bsz = packed.batch_sizes
            is_off = is_offset.data.to(dev, non_blocking=True)
            B = int(bsz[0])
            logits = self.feature_sampler(self.encoder(torch.nn.utils.rnn.PackedSequence(data, bsz)))
            probs = torch.softmax(logits.double(), -1)
            cat_prob, cat = probs.max(-1)
            if self.decoder.embed_speaker is not None:
                spk = torch.as_tensor(speaker, dtype=torch.int64).cpu()
                present, own = torch.unique(spk, sorted=True, return_inverse=True)
            else:
                present, own = torch.zeros(1, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)
            protos = self.prototypes_for(present.tolist(), int(bsz.numel()))
            em, off, lengths = self.decoder.score_against(protos, bsz, data, is_off)
            if len(present) > 1:  # each segment's K columns under its own speaker
                cols = (own.to(dev) * K)[:, None] + torch.arange(K, device=dev)[None, :]
                em, off = em.gather(1, cols), off.gather(1, cols)
            ev, best, best_prob, resp = ops.pair_posterior(em, off, log_weight)
            best = best.to(torch.int64)
            out = {"length": lengths, "category_ix": cat, "category_prob": cat_prob, "decoder_category_ix": best,
                   "decoder_category_prob": best_prob.double(), "log_evidence": ev.double(), "agree": best == cat}
            if matrix:  # category-major, as encode.py orders a batch's rows
                out["long"] = {"row": torch.arange(B).repeat(K), "category_ix": torch.arange(K).repeat_interleave(B),
                               "emission_nll": em.t().reshape(-1), "end_prediction_loss": off.t().reshape(-1),
                               "log_weight": log_weight.repeat_interleave(B),
                               "responsibility": resp.t().reshape(-1)}
            return out

    def classify_dataset(self, dataset, save_path, batch_size=1, prior="dirichlet", entire_data_size=None,
                         matrix_path=None):
        n = len(dataset) if entire_data_size is None else entire_data_size
        lw = self.log_weight(prior, n)
        return score.score_table(lambda p, o, s: self.classify_batch(p, o, s, lw, matrix=matrix_path is not None),
                                 dataset, save_path, batch_size=batch_size,
                                 finish=lambda: _native.op_status.sync("classify_dataset"), columns=TABLE,
                                 long_path=matrix_path, long_columns=MATRIX)


def get_parameters(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="Score annotated segments against every category of a trained ABCD-VAE "
                                            "(MI355X): decoder-side classification, responsibilities and evidence.")
    cli.add_data_arguments(p, table_help="annotation table (csv) of the segments to classify",
                           save_help="output csv (default: <input_root>/classified.csv); an existing file is kept as "
                                     ".prev")
    cli.add_prior_arguments(
        p, prior_help="log weights of the categories: the Dirichlet posterior's E[log pi_k] (default) or zero",
        size_help="N of the Dirichlet posterior softmax(shape logits) * N + a0 (default: the number of segments)")
    p.add_argument("--matrix", type=str, default=None,
                   help="also write the long table of every (segment, category) to this csv")
    a = p.parse_args(argv)
    cli.check_prior_arguments(p, a)
    return a


def main(argv=None):
    a = get_parameters(argv)
    save_path = a.save_path or os.path.join(a.input_root, "classified.csv")
    for path in (save_path, a.matrix):
        if path and os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
    dataset = cli.open_dataset(a)
    Classifier(a.model_path, device=a.device).classify_dataset(
        dataset, save_path, batch_size=a.batch_size, prior=a.prior, entire_data_size=a.entire_data_size,
        matrix_path=a.matrix)
    return save_path


if __name__ == "__main__":
    main()
