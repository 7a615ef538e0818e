# coding: utf-8
"""Spectrogram frames back to audio on the HIP path: listen to what
``decode.py`` wrote.

Reads ``decode.py``'s ``.npz`` -- any file with ``batch_sizes``,
``sorted_indices`` and the chosen ``--field`` (packed L x F log-amplitude
frames), plus ``category_ix`` if present -- and inverts the featuriser
(``log(|STFT| + eps) / N``) by Griffin-Lim phase retrieval on the GPU
(``DeviceVocoder``: one launch for all sequences and every iteration).  The
reference has no such script.

Output in ``--save_dir``: one ``category_<k>.wav`` per sequence
(``sequence_<i>.wav`` without ``category_ix``) and ``synthesis.csv`` with
``index, category_ix, frames, samples, residual, clipped_samples, path``.
Samples are int16 with saturation: the data are int16-scale because the
reference never rescales them (``--float32`` writes float instead).  A sequence
too short for the STFT's reflect padding (``hop * (frames - 1) <= n_fft -
n_fft // 2``) gets a row and no file."""
import argparse
import os

import numpy as np
import pandas as pd
import scipy.io.wavfile as spw
import torch

import cli
from modules import _native, data_utils

COLUMNS = ("index", "category_ix", "frames", "samples", "residual", "clipped_samples", "path")


def to_int16(wave):
    """-> (int16 samples, how many saturated)"""
    r = np.rint(wave)
    clipped = int(((r > 32767) | (r < -32768)).sum())
    return np.clip(r, -32768, 32767).astype(np.int16), clipped


def synthesize_to_dir(arrays, save_dir, fs, vocoder, field="mu", n_iter=32, momentum=0.99, seed=0, float32=False):
    """Writes the wavs and synthesis.csv; every file goes to a temporary name and
    takes its place (an earlier one kept as .prev) only once the device status
    is clean, so an error leaves nothing partial.  -> the table."""
    for k in ("batch_sizes", "sorted_indices", field):
        if k not in arrays:
            raise SystemExit(f"the input has no array {k!r} (decode.py writes batch_sizes, sorted_indices, data, mu)")
    data = torch.from_numpy(np.asarray(arrays[field], dtype=np.float32))
    bs = torch.from_numpy(np.asarray(arrays["batch_sizes"], dtype=np.int64))
    order = np.asarray(arrays["sorted_indices"], dtype=np.int64)  # packed position j holds sequence order[j]
    F = vocoder.n_fft // 2 + 1
    if data.dim() != 2 or data.shape[1] != F:
        raise SystemExit(f"{field} has {tuple(data.shape)[-1]} frequency bins, the framing ({vocoder.n_fft} samples per "
                         f"frame) gives {F}: pass the sampling rate and --fft_frame_length of the model's training data")
    cats = np.asarray(arrays["category_ix"], dtype=np.int64) if "category_ix" in arrays else None
    os.makedirs(save_dir, exist_ok=True)
    with cli.replacing_outputs() as tmp:
        waves, n_samples, residual = vocoder((data, bs), n_iter=n_iter, momentum=momentum, seed=seed)
        waves, residual = waves.cpu().numpy(), residual.cpu().numpy()
        rows = []
        for j, i in enumerate(order):
            n = int(n_samples[j])
            name = f"category_{int(cats[i])}.wav" if cats is not None else f"sequence_{int(i)}.wav"
            row = dict(index=int(i), category_ix=int(cats[i]) if cats is not None else -1,
                       frames=int((bs > j).sum()), samples=n, residual=float(residual[j]), clipped_samples=0, path="")
            if n > 0:
                if float32:
                    out = waves[j, :n].astype(np.float32)
                else:
                    out, row["clipped_samples"] = to_int16(waves[j, :n])
                spw.write(tmp(os.path.join(save_dir, name)), int(fs), out)
                row["path"] = name
            rows.append(row)
        table = pd.DataFrame(sorted(rows, key=lambda r: r["index"]), columns=list(COLUMNS))
        table.to_csv(tmp(os.path.join(save_dir, "synthesis.csv")), index=False)
        _native.op_status.sync("synthesize")
    return table


def get_parameters(argv=None):
    p = argparse.ArgumentParser(description="Griffin-Lim synthesis of decoded spectrogram frames (MI355X).")
    p.add_argument("decoded_path", type=str, help=".npz written by decode.py")
    p.add_argument("sampling_rate", type=int, help="sampling rate of the model's training audio, Hz")
    p.add_argument("data_normalizer", type=float, help="the normaliser N of log(|STFT| + eps) / N used in training")
    p.add_argument("-S", "--save_dir", type=str, required=True, help="output directory")
    p.add_argument("--field", type=str, default="mu", help="which frames to invert: mu (default) or data")
    cli.add_stft_arguments(p, no_centering_help="not supported: see the message", channel=False)
    p.add_argument("--iterations", type=int, default=32, help="Griffin-Lim iterations")
    p.add_argument("--momentum", type=float, default=0.99, help="0: classic Griffin-Lim; 0.99: the fast variant")
    p.add_argument("--seed", type=int, default=0, help="seed of the random initial phase")
    p.add_argument("--float32", action="store_true", help="write float32 wavs instead of saturated int16")
    cli.add_device_argument(p)
    return p.parse_args(argv)


def main(argv=None):
    a = get_parameters(argv)
    if a.fft_no_centering:
        raise SystemExit("synthesize.py: an STFT without centre padding cannot be inverted at the edges (a Hann window "
                         "violates the overlap-add condition there; the library returns ABCD_EINVAL for center = 0)")
    fs = a.sampling_rate
    frame, hop = cli.frame_hop(a, fs)
    voc = data_utils.DeviceVocoder(frame, hop, window=a.fft_window_type, eps=a.epsilon, normalizer=a.data_normalizer,
                                   device=a.device)
    with np.load(a.decoded_path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    synthesize_to_dir(arrays, a.save_dir, fs, voc, field=a.field, n_iter=a.iterations, momentum=a.momentum,
                      seed=a.seed, float32=a.float32)
    return a.save_dir


if __name__ == "__main__":
    main()
