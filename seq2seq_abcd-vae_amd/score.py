# coding: utf-8
"""Per-segment ELBO scoring on the HIP path: how well does a trained ABCD-VAE
explain each annotated segment?

The counterpart of ``encode.py`` for likelihoods.  The reference only logs
per-epoch means of its three losses (learning.py:200-240); here every segment
gets its own share of them.  Same checkpoint, annotation and STFT arguments and
the same loader as ``encode.py``; output: a CSV with one row per segment,

``data_ix, length, category_ix, emission_nll, end_prediction_loss, kl_row,
kl_prior_share, total``

followed by the annotation columns as ``encode.py`` appends them.  ``length``
is the segment's frame count, ``category_ix`` the argmax of its logits,
``emission_nll`` / ``end_prediction_loss`` its rows' share of the decoder's
two losses (``RNN_Variational_Decoder.score``), ``kl_row`` its row of the
categorical KL and ``kl_prior_share`` the Dirichlet bracket divided by the
number of segments N (``ABCDSampler.kl_rows``).  ``total`` is their sum: the
segment's share of the reference's "loss per string" -- summed over the table
it is N times what ``Learner.test_or_validate`` logs under the same noise.

``--mean`` (default) scores deterministically: the decoder is fed the softmax
mixture of the codebook and feeds back its emission mean.  ``--sample`` draws
the Gumbel-softmax features and the emission samples as validation does;
``--samples S`` averages ``emission_nll`` and ``end_prediction_loss`` over S
such draws (consecutive blocks of the Philox stream ``--seed`` keys)."""
import argparse
import os

import numpy as np
import pandas as pd
import torch

import cli
import learning
from modules import _native, data_utils, noise

COLUMNS = ("data_ix", "length", "category_ix", "emission_nll", "end_prediction_loss", "kl_row", "kl_prior_share",
           "total")
_TERMS = ("emission_nll", "end_prediction_loss", "kl_row", "kl_prior_share")


class Scorer(cli.FrozenCheckpoint, learning.Learner):
    """A trained ABCD checkpoint (ours or the reference's) opened for scoring:
    parameters frozen, modules in eval mode."""
    NOT_ABCD = ("not an ABCD-VAE checkpoint (its feature sampler has no categories, e.g. the plain Gaussian VAE): "
                "score.py scores the categorical model")

    def score_batch(self, packed, is_offset, speaker, num_strings, sample=False, samples=1):
        """One batch -> {column: B device values in the batch's packed row order}
        (every column of COLUMNS but data_ix and total)."""
        dev = self.device
        with torch.no_grad():
            data = packed.data.to(dev, non_blocking=True)
            bsz = packed.batch_sizes
            is_off = is_offset.data.to(dev, non_blocking=True)
            spk = speaker.to(dev, non_blocking=True) if self.decoder.embed_speaker is not None else None
            logits = self.feature_sampler(self.encoder(torch.nn.utils.rnn.PackedSequence(data, bsz)))
            rows, prior = self.feature_sampler.kl_rows(logits, num_strings)
            draws = max(int(samples), 1) if sample else 1
            em = off = None
            for _ in range(draws):
                feats = self.feature_sampler.sample(logits, no_sample=not sample)
                e, o, lengths = self.decoder.score(feats, bsz, speaker=spk, ground_truth_out=data,
                                                   ground_truth_offset=is_off, mean=not sample)
                e, o = e.double(), o.double()
                em, off = (e, o) if em is None else (em + e, off + o)
            return {"length": lengths, "category_ix": logits.argmax(-1), "emission_nll": em / draws,
                    "end_prediction_loss": off / draws, "kl_row": rows.double(),
                    "kl_prior_share": (prior.double() / float(num_strings)).expand(rows.shape[0])}

    def score_dataset(self, dataset, save_path, batch_size=1, sample=False, samples=1):
        n = len(dataset)
        return score_table(lambda p, o, s: self.score_batch(p, o, s, n, sample=sample, samples=samples), dataset,
                           save_path, batch_size=batch_size, finish=lambda: _native.op_status.sync("score_dataset"))


# the table's columns after data_ix: (name, dtype), or (name, names) for the sum of other columns
TABLE = ((("length", np.int64), ("category_ix", np.int64)) + tuple((k, np.float64) for k in _TERMS)
         + (("total", _TERMS),))


def score_table(score_batch, dataset, save_path, batch_size=1, finish=None, columns=TABLE, long_path=None,
                long_columns=None):
    """Writes the table: ``score_batch(packed, is_offset, speaker)`` gives a
    batch's columns in packed row order, which the loader's ``ixs`` map back to
    ``data_ix``.  ``columns`` lists what follows ``data_ix``: ``(name, dtype)``
    for a column ``score_batch`` returns, ``(name, names)`` for the sum of
    earlier columns.  The table goes to a temporary path and takes save_path
    (an earlier output kept as .prev) only once every batch is written and
    ``finish()`` (the device status check) has passed, so an error part way
    leaves nothing partial behind.  Returns the number of rows written.

    ``long_path``: a second, long table written under the same discipline from
    ``score_batch(...)["long"]``, a dict holding ``row`` (the packed row each
    long row belongs to, mapped to ``data_ix`` here) and the ``long_columns``
    (``(name, dtype)``), in the order the rows are to be written."""
    ann = cli.annotation_columns(dataset)

    def host(v):
        return v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)

    header, written = True, 0
    with cli.replacing_outputs() as tmp:
        tmp_path, long_tmp_path = tmp(save_path), long_path and tmp(long_path)
        for packed, is_offset, speaker, ixs in data_utils.DataLoader(dataset, batch_size=batch_size, shuffle=False):
            out = score_batch(packed, is_offset, speaker)
            ix = np.asarray(ixs, dtype=np.int64)
            table = pd.DataFrame({"data_ix": ix})
            for name, kind in columns:
                if isinstance(kind, (tuple, list)):
                    table[name] = table[list(kind)].sum(axis=1)
                else:
                    table[name] = host(out[name]).astype(kind)
            if len(table) != len(ix):
                raise RuntimeError(f"score_batch returned {len(table)} rows for a batch of {len(ix)} segments")
            mode = "w" if header else "a"
            cli.join_annotation(table, ann).to_csv(tmp_path, index=False, mode=mode, header=header)
            if long_path is not None:
                long = out["long"]
                lt = pd.DataFrame({"data_ix": ix[host(long["row"]).astype(np.int64)]})
                for name, kind in long_columns:
                    lt[name] = host(long[name]).astype(kind)
                cli.join_annotation(lt, ann).to_csv(long_tmp_path, index=False, mode=mode, header=header)
            header = False
            written += len(table)
        if finish is not None:
            finish()  # a timed-out persistent launch fails the run, not the table
    return written


def get_parameters(argv=None):
    p = argparse.ArgumentParser(description="Score annotated segments under a trained ABCD-VAE (MI355X): "
                                            "per-segment emission NLL, end-prediction loss and KL.")
    cli.add_data_arguments(p, table_help="annotation table (csv) of the segments to score",
                           save_help="output csv (default: <input_root>/scores.csv); an existing file is kept as .prev")
    how = p.add_mutually_exclusive_group()
    how.add_argument("--mean", action="store_true",
                     help="deterministic score (default): softmax features, the emission mean fed back")
    how.add_argument("--sample", action="store_true",
                     help="score under sampled Gumbel-softmax features and emission samples, as validation does")
    p.add_argument("--samples", type=int, default=1,
                   help="average emission_nll and end_prediction_loss over this many draws (> 1 implies --sample)")
    p.add_argument("--seed", type=int, default=None, help="seed of the sampling noise (--sample)")
    a = p.parse_args(argv)
    if a.samples < 1:
        p.error("--samples must be at least 1")
    if a.mean and a.samples > 1:
        p.error("--samples > 1 averages over noise draws: it cannot be combined with --mean")
    a.sample = a.sample or a.samples > 1
    a.mean = not a.sample
    return a


def main(argv=None):
    a = get_parameters(argv)
    save_path = a.save_path or os.path.join(a.input_root, "scores.csv")
    if os.path.dirname(save_path):
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
    dataset = cli.open_dataset(a)
    scorer = Scorer(a.model_path, device=a.device)
    if a.seed is not None:
        noise.manual_seed(a.seed)
    scorer.score_dataset(dataset, save_path, batch_size=a.batch_size, sample=a.sample, samples=a.samples)
    return save_path


if __name__ == "__main__":
    main()
