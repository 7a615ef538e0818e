# coding: utf-8
"""Post-training encoding of the plain Gaussian VAE on the HIP path: the
drop-in for plain/encode.py.

Same command line and the same long-format CSV as the reference
(plain/encode.py:37-52, 56-107): one row per (segment, Gaussian parameter,
feature dimension) with columns ``data_ix, parameter_name, feature_dim,
parameter_value``, sorted by (data_ix, parameter_name, feature_dim), then the
annotation columns when the annotation has a ``label`` column.
``parameter_name`` is the parameter's index (0 = mean, 1 = log-variance of
``Sampler.forward``, plain/modules/model.py:545-550) unless ``-p`` names
them.

How it runs here: each batch goes through the encoder kernels and the
plain sampler's MLP kernels once (model.py:60-66; plain model.py:545-550) and
its (mean, log-variance) rows stay on the device until the dataset is done;
the table is then built with numpy index arithmetic from two N x f host
matrices instead of one Python tuple per value.  The reference sorts the
whole table before writing it, so nothing is written per batch here either."""
import argparse
import os

import numpy as np
import pandas as pd
import torch

import cli
import plain_learning
from modules import _native, data_utils

COLUMNS = ["data_ix", "parameter_name", "feature_dim", "parameter_value"]


class Encoder(cli.FrozenCheckpoint, plain_learning.Learner):
    """A trained plain checkpoint (ours or the reference's, plain/learning.py
    keys) opened for inference: parameters frozen, modules in eval mode
    (plain/encode.py:12-20)."""

    def _device_params(self, packed):
        with torch.no_grad():
            h = self.encoder(packed.to(self.device))
            return self.feature_sampler(h)

    def encode(self, data, is_packed=False, to_numpy=True):
        """One batch -> the sampler's parameters [mean (B x f), log-variance
        (B x f)]; with to_numpy a generator of numpy arrays, as the reference
        returns (plain/encode.py:23-34)."""
        if not is_packed:
            data = torch.nn.utils.rnn.pack_sequence(data if isinstance(data, list) else [data])
        params = self._device_params(data)
        if to_numpy:
            return (p.cpu().numpy() for p in params)
        return params

    def encode_dataset(self, dataset, to_numpy=True, parameter_ix2name=None, batch_size=1):
        """plain/encode.py:37-52: the long table over the whole dataset,
        UNSORTED in the reference's row order (batch, parameter, segment,
        dimension); main() sorts it as the reference does."""
        if parameter_ix2name is None:
            parameter_ix2name = {}
        outs, ixs = [], []
        for packed, _, _, ix in data_utils.DataLoader(dataset, batch_size=batch_size):
            outs.append(self._device_params(packed))  # device tensors; copied once at the end
            ixs.append(np.asarray(ix, dtype=np.int64))
        _native.op_status.sync("encode_dataset")  # a timed-out persistent launch fails the run, not the table
        frames = []
        for params, ix in zip(outs, ixs):
            for pix, p in enumerate(params):
                v = p.cpu().numpy()
                n, f = v.shape
                name = parameter_ix2name.get(pix, pix)
                frames.append(pd.DataFrame({"data_ix": np.repeat(ix, f), "parameter_name": [name] * (n * f),
                                            "feature_dim": np.tile(np.arange(f), n),
                                            "parameter_value": v.reshape(-1)}))
        if not frames:
            return pd.DataFrame(columns=COLUMNS)
        return pd.concat(frames, ignore_index=True)[COLUMNS]


def plain_annotation(annotation_file, sep=","):
    """The annotation table as plain/modules/data_utils.py:10-22 leaves it
    (speaker ids mapped to their first-appearance index, or a NaN speaker
    column when there is none): the columns the reference's output carries."""
    df = pd.read_csv(annotation_file, sep=sep)
    if "speaker" in df.columns:
        speaker2ix = {spk: ix for ix, spk in enumerate(df.speaker.unique())}
        df.loc[:, "speaker"] = df.speaker.map(speaker2ix)
    else:
        df["speaker"] = float("nan")
    return df


def get_parameters(argv=None):
    p = argparse.ArgumentParser(description="Encode annotated segments with a trained plain VAE (MI355X).")
    cli.add_data_arguments(
        p, table_help="annotation table (csv) of the segments to encode",
        save_help="output csv (default: <input_root>/autoencoded.csv)",
        model_help="checkpoint.pt written by plain_learning.py or plain/learning.py",
        before_epsilon=lambda p: p.add_argument("-p", "--parameter_names", type=str, default=None,
                                                help="comma-separated parameter names"))
    return p.parse_args(argv)


def main(argv=None):
    a = get_parameters(argv)
    save_path = a.save_path or os.path.join(a.input_root, "autoencoded.csv")
    if os.path.dirname(save_path):
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
    dataset = cli.open_dataset(a)
    ix2name = {} if a.parameter_names is None else dict(enumerate(a.parameter_names.split(",")))
    df = Encoder(a.model_path, device=a.device).encode_dataset(dataset, parameter_ix2name=ix2name,
                                                               batch_size=a.batch_size)
    df = df.sort_values(["data_ix", "parameter_name", "feature_dim"])
    ann = plain_annotation(a.annotation_file, a.annotation_sep)
    if "label" in ann.columns:
        df = df.merge(ann, how="left", left_on="data_ix", right_index=True)
    df.to_csv(save_path, index=False)
    return save_path


if __name__ == "__main__":
    main()
