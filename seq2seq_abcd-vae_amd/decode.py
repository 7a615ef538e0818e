# coding: utf-8
"""Post-training decoding on the HIP path: what does category k sound like?

The counterpart of ``encode.py``.  The features of category k are column k of
the trained codebook -- what ``ABCDSampler.sample`` gives for a one-hot y
(model.py:592-606) -- and the decoder runs free from them
(``RNN_Variational_Decoder.generate``): every sequence stops where the offset
predictor's probability first exceeds ``--stop_prob``, so no segment length has
to be known.  The reference has no such script: its decoder is only ever run
at the lengths of the data (learning.py:153).

Output: one ``.npz`` with ``category_ix`` (the categories, in input order),
``lengths`` (frames per category, same order), and the frames as a
``PackedSequence``: ``batch_sizes``, ``sorted_indices`` (the categories' rows by
length, descending) and packed ``data`` / ``mu`` / ``log_var`` (L x F
log-amplitude frames) / ``offset_logits`` (L).  Sequence i is rows
``off[t] + j`` for ``t < lengths[sorted_indices[j]]`` with
``sorted_indices[j] == i`` -- ``torch.nn.utils.rnn.pad_packed_sequence``
unpacks it."""
import argparse
import os

import numpy as np
import torch

import cli
import learning
from modules import _native, noise


class Decoder(cli.FrozenCheckpoint, learning.Learner):
    """A trained ABCD checkpoint (ours or the reference's) opened for
    generation: parameters frozen, modules in eval mode."""
    NOT_ABCD = ("not an ABCD-VAE checkpoint (its feature sampler has no categories / codebook, e.g. the plain "
                "Gaussian VAE): decode.py decodes categories")

    def category_features(self, categories):
        """K' x D: the codebook's columns of the given categories."""
        K = self.feature_sampler.num_categories
        ix = torch.as_tensor(categories, dtype=torch.int64)
        if ix.numel() == 0 or int(ix.min()) < 0 or int(ix.max()) >= K:
            raise ValueError(f"categories must be in 0..{K - 1}")
        return self.feature_sampler.codebook.detach().t()[ix.to(self.device)].contiguous()

    def decode(self, categories, max_length=200, sample=False, stop_prob=0.5, min_length=1, speaker_ix=0):
        """-> (packed, lengths, (mu, log_var), offset_logits) of ``generate``."""
        feats = self.category_features(categories)
        spk = None
        if self.decoder.embed_speaker is not None:
            spk = torch.full((feats.shape[0],), int(speaker_ix), dtype=torch.int64, device=self.device)
        return self.decoder.generate(feats, max_length, speaker=spk, mean=not sample, stop_prob=stop_prob,
                                     min_length=min_length)

    def decode_to_file(self, categories, save_path, **kw):
        """The result is written to a temporary path and takes save_path (an
        earlier output kept as .prev) only once the device status is clean, so
        a timed-out persistent launch or an error leaves nothing partial."""
        with cli.replacing_outputs() as tmp:
            tmp_path = tmp(save_path, ext=".npz")
            packed, lengths, (mu, lv), offl = self.decode(categories, **kw)
            arrays = dict(category_ix=np.asarray(categories, dtype=np.int64), lengths=lengths.cpu().numpy(),
                          batch_sizes=packed.batch_sizes.numpy(), sorted_indices=packed.sorted_indices.cpu().numpy(),
                          data=packed.data.cpu().numpy(), mu=mu.cpu().numpy(), log_var=lv.cpu().numpy(),
                          offset_logits=offl.cpu().numpy())
            np.savez(tmp_path, **arrays)
            _native.op_status.sync("decode")  # a timed-out persistent launch fails the run, not the file
        return arrays


def parse_categories(spec, K):
    if spec == "all":
        return list(range(K))
    try:
        return [int(s) for s in spec.split(",") if s.strip() != ""]
    except ValueError:
        raise SystemExit(f"--categories: 'all' or a comma-separated list of indices, not {spec!r}")


def get_parameters(argv=None):
    p = argparse.ArgumentParser(description="Decode categories of a trained ABCD-VAE into spectrogram frames (MI355X).")
    p.add_argument("model_path", type=str, help="checkpoint.pt written by learning.py (this package or the reference)")
    p.add_argument("-S", "--save_path", type=str, required=True, help="output .npz; an existing file is kept as .prev")
    p.add_argument("--categories", type=str, default="all", help="'all' or a comma-separated list, e.g. 0,3,7")
    p.add_argument("--max_length", type=int, default=200, help="frames after which a sequence is cut if it never stops")
    p.add_argument("--sample", action="store_true", help="feed back samples of the emission instead of its mean")
    p.add_argument("--seed", type=int, default=None, help="seed of the sampling noise (--sample)")
    p.add_argument("--stop_prob", type=float, default=0.5,
                   help="a sequence ends at the first frame whose offset probability exceeds this")
    p.add_argument("--min_length", type=int, default=1, help="frames every sequence gets at least")
    p.add_argument("--speaker_ix", type=int, default=0, help="speaker index (models with a speaker embedding)")
    cli.add_device_argument(p)
    return p.parse_args(argv)


def main(argv=None):
    a = get_parameters(argv)
    if os.path.dirname(a.save_path):
        os.makedirs(os.path.dirname(a.save_path), exist_ok=True)
    dec = Decoder(a.model_path, device=a.device)
    if a.seed is not None:
        noise.manual_seed(a.seed)
    cats = parse_categories(a.categories, dec.feature_sampler.num_categories)
    dec.decode_to_file(cats, a.save_path, max_length=a.max_length, sample=a.sample, stop_prob=a.stop_prob,
                       min_length=a.min_length, speaker_ix=a.speaker_ix)
    return a.save_path


if __name__ == "__main__":
    main()
