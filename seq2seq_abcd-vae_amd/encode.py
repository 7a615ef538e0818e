# coding: utf-8
"""Post-training encoding on the HIP path: the drop-in for ABCD-VAE/encode.py
(and, through ``output=``, encode_logit.py / encode_features.py).

Same command line and the same long-format CSV as the reference
(encode.py:38-55): one row per (segment, category) with columns
``data_ix, category_ix, prob`` (``dimension, logit`` / ``dimension,
feature_value`` for the logit / feature variants) followed by the
annotation columns, rows ordered category-major within each batch.

How it runs here: every batch goes through the encoder and sampler forward
kernels once (model.py:60-66, 581-590) and stays on the device; the softmax
(or nothing, or the to_code_like MLP) is applied there, and the table is
written batch by batch with numpy index arithmetic (no DataFrame melt /
merge / append cycle), the previous batch's rows while the current one runs."""
import argparse
import os

import numpy as np
import pandas as pd
import torch

import cli
import learning
from cli import rename_existing_file  # noqa: F401 (re-exported: it used to live here)
from modules import _native, data_utils

OUTPUT = "probs"  # encode_logit.py -> "logits", encode_features.py -> "features"
COLUMNS = {"probs": ("category_ix", "prob"), "logits": ("dimension", "logit"),
           "features": ("dimension", "feature_value")}


class Encoder(cli.FrozenCheckpoint, learning.Learner):
    """A trained checkpoint (ours or the reference's: learning.py:317-347 keys)
    opened for inference: parameters frozen, modules in eval mode."""

    def _device_output(self, packed, output):
        with torch.no_grad():
            h = self.encoder(packed.to(self.device))
            if output == "features":
                return self.feature_sampler.to_code_like(h)
            logits = self.feature_sampler(h)
            return torch.softmax(logits, -1) if output == "probs" else logits

    def encode(self, data, is_packed=False, to_numpy=True, output=None):
        """One batch (a PackedSequence, a tensor or a list of tensors) ->
        B x K probabilities (or logits / features); with to_numpy, an iterator
        of per-segment numpy rows as the reference returns."""
        if not is_packed:
            data = torch.nn.utils.rnn.pack_sequence(data if isinstance(data, list) else [data])
        out = self._device_output(data, output or OUTPUT)
        if to_numpy:
            return iter(out.cpu().numpy())
        return out

    def encode_dataset(self, dataset, save_path, to_numpy=True, batch_size=1, output=None):
        """Streams the table: each batch's device output is copied to pinned
        host memory without blocking, and the PREVIOUS batch's rows are written
        while the current one computes, so host and device memory stay bounded
        by two batches whatever the dataset size (the reference also writes
        per batch, encode.py:38-55)."""
        output = output or OUTPUT
        var_name, value_name = COLUMNS[output]
        ann = cli.annotation_columns(dataset)
        state = {"header": True}
        # the table takes save_path only once every batch is written and the
        # device status is clean: a timed-out persistent launch or an error
        # part way leaves no invalid or partial table behind
        with cli.replacing_outputs() as tmp:
            tmp_path = tmp(save_path)

            def write(host, event, ix):
                event.synchronize()
                v = host.numpy()
                n, k = v.shape
                table = pd.DataFrame({"data_ix": np.tile(ix, k), var_name: np.repeat(np.arange(k), n),
                                      value_name: v.T.reshape(-1)})
                cli.join_annotation(table, ann).to_csv(tmp_path, index=False, mode="w" if state["header"] else "a",
                                                       header=state["header"])
                state["header"] = False

            pending = None
            for packed, _, _, ix in data_utils.DataLoader(dataset, batch_size=batch_size):
                vals = self._device_output(packed, output)
                host = torch.empty(vals.shape, dtype=vals.dtype, pin_memory=True)
                host.copy_(vals, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                if pending is not None:
                    write(*pending)
                pending = (host, event, np.asarray(ix, dtype=np.int64))
            if pending is not None:
                write(*pending)
            _native.op_status.sync("encode_dataset")  # a timed-out persistent launch fails the run, not the table


def get_parameters(argv=None):
    p = argparse.ArgumentParser(description="Encode annotated segments with a trained ABCD-VAE (MI355X).")
    cli.add_data_arguments(p, table_help="annotation table (csv) of the segments to encode",
                           save_help="output csv (default: <input_root>/autoencoded.csv); an existing file is kept "
                                     "as .prev")
    return p.parse_args(argv)


def main(argv=None, output=None):
    a = get_parameters(argv)
    save_path = a.save_path or os.path.join(a.input_root, "autoencoded.csv")
    if os.path.dirname(save_path):
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
    dataset = cli.open_dataset(a)
    Encoder(a.model_path, device=a.device).encode_dataset(dataset, save_path, batch_size=a.batch_size, output=output)
    return save_path


if __name__ == "__main__":
    main()
