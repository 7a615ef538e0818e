# coding: utf-8
"""What the command-line tools share: the data and prior arguments, the
featurisation they describe, a checkpoint opened for inference, outputs that
leave nothing partial behind, and the annotation columns joined to a table.

``learning.py`` and ``plain_learning.py`` keep their own parsers: their flags
and help mirror the reference's trainers."""
import contextlib
import math
import os

import numpy as np
import pandas as pd
import torch

from modules import data_utils
from modules.data_utils import Compose

PRIORS = ("dirichlet", "uniform")


def add_stft_arguments(p, no_centering_help="STFT without centre padding", channel=True, before_epsilon=None):
    """``before_epsilon(p)`` adds a tool's own arguments where its --help has
    always listed them (plain_encode.py's -p)."""
    p.add_argument("--fft_frame_length", type=float, default=0.008, help="STFT window length, seconds")
    p.add_argument("--fft_step_size", type=float, default=0.004, help="STFT hop, seconds")
    p.add_argument("--fft_window_type", type=str, default="hann_window", help="torch window function name")
    p.add_argument("--fft_no_centering", action="store_true", help=no_centering_help)
    if channel:
        p.add_argument("--channel", type=int, default=0, help="channel (0-based) of multi-channel wav files")
    if before_epsilon is not None:
        before_epsilon(p)
    p.add_argument("-E", "--epsilon", type=float, default=2 ** (-15), help="offset inside log(|STFT| + eps)")


def add_device_argument(p):
    p.add_argument("-d", "--device", type=str, default="cuda", help="GPU device (there is no CPU path)")


def add_data_arguments(p, table_help, save_help, table="annotation_file",
                       model_help="checkpoint.pt written by learning.py (this package or the reference)",
                       root_help="directory the annotation's wav paths are relative to",
                       sep_help="field separator of the annotation table", batch=True, before_epsilon=None):
    """The checkpoint, the table of segments (or recordings) and how they are
    featurised: one interface for every tool that reads data."""
    p.add_argument("model_path", type=str, help=model_help)
    p.add_argument("input_root", type=str, help=root_help)
    p.add_argument(table, type=str, help=table_help)
    p.add_argument("data_normalizer", type=float, help="log-amplitudes are divided by this (training's -N)")
    p.add_argument("--annotation_sep", type=str, default=",", help=sep_help)
    add_device_argument(p)
    p.add_argument("-S", "--save_path", type=str, default=None, help=save_help)
    add_stft_arguments(p, before_epsilon=before_epsilon)
    if batch:
        p.add_argument("-b", "--batch_size", type=int, default=1, help="segments per forward pass")


def add_prior_arguments(p, prior_help, size_help):
    p.add_argument("--prior", type=str, default="dirichlet", choices=PRIORS, help=prior_help)
    p.add_argument("--entire_data_size", type=float, default=None, help=size_help)


def check_prior_arguments(p, a):
    if a.entire_data_size is not None and not a.entire_data_size > 0:
        p.error("--entire_data_size must be positive")


DEFAULT_MOVES = (0.2, 0.6, 0.2)   # stay, step, skip


def add_moves_argument(p, moves_help):
    p.add_argument("--moves", type=float, nargs=3, default=list(DEFAULT_MOVES), metavar=("STAY", "STEP", "SKIP"),
                   help=moves_help)


def check_moves_argument(p, a):
    if any(m < 0 or math.isnan(m) or math.isinf(m) for m in a.moves) or not sum(a.moves) > 0:
        p.error("--moves: three non-negative weights, not all zero")


def frame_hop(a, fs):
    """The STFT window and hop in samples at sampling rate ``fs``."""
    return int(np.floor(a.fft_frame_length * fs)), int(np.floor(a.fft_step_size * fs))


def log_spectrum(a, frame, hop):
    """wave tensor -> frames x (frame // 2 + 1) of ``log(|STFT| + eps) / N``."""
    eps, norm = a.epsilon, a.data_normalizer
    return Compose([data_utils.STFT(frame, hop, window=a.fft_window_type, centering=not a.fft_no_centering),
                    data_utils.Transform(lambda x: (x + eps).log() / norm)])


def open_dataset(a):
    """The annotated segments as the loader's dataset of log-spectra."""
    parser = data_utils.Data_Parser(a.input_root, a.annotation_file, annotation_sep=a.annotation_sep)
    frame, hop = frame_hop(a, parser.get_sample_freq())
    return parser.get_data(transform=Compose([data_utils.ToTensor(), log_spectrum(a, frame, hop)]),
                           channel=a.channel)


class FrozenCheckpoint(object):
    """Mixed in before a ``Learner``: a trained checkpoint (ours or the
    reference's) opened for inference, parameters frozen, modules in eval mode.
    A class that sets ``NOT_ABCD`` (the rest of the message) refuses a
    checkpoint whose feature sampler has no categories."""
    NOT_ABCD = None

    def __init__(self, model_config_path, device="cuda"):
        self.device = torch.device(device)
        if self.NOT_ABCD is not None:
            ckpt = torch.load(model_config_path, map_location="cpu", weights_only=True)
            if "num_categories" not in ckpt.get("feature_sampler_init_parameters", {}):
                raise SystemExit(f"{model_config_path}: {self.NOT_ABCD}")
            del ckpt
        self.retrieve_model(checkpoint_path=model_config_path, device=device)
        for m in (self.encoder, self.feature_sampler, self.decoder):
            m.requires_grad_(False)
            m.eval()


def rename_existing_file(filepath):
    """Keep earlier outputs: path -> path.prev -> path.prev.prev -> ..."""
    chain = []
    p = filepath
    while os.path.isfile(p):
        chain.append(p)
        p += ".prev"
    for src in reversed(chain):
        os.rename(src, src + ".prev")


@contextlib.contextmanager
def replacing_outputs():
    """``with replacing_outputs() as tmp``: ``tmp(path)`` is the temporary path
    to write (or append) in ``path``'s stead.  When the block ends, every
    temporary that exists takes its path's place, the earlier file kept as
    .prev; when it raises, the temporaries are removed and no path is touched.
    So an error part way, or a device status check failing as the block's last
    statement, leaves nothing invalid or partial behind.  ``tmp(path,
    ext=".npz")`` ends the temporary's name in the extension ``np.savez`` would
    otherwise append."""
    pending = {}  # path -> temporary

    def tmp(path, ext=""):
        return pending.setdefault(path, path + ".partial" + ext)

    try:
        yield tmp
    except BaseException:
        for t in pending.values():
            if os.path.isfile(t):
                os.remove(t)
        raise
    for path, t in pending.items():
        if os.path.isfile(t):  # (an empty dataset writes no table, as the reference)
            rename_existing_file(path)
            os.replace(t, path)


def annotation_columns(dataset):
    """The annotation columns the tables carry, or None when the annotation has
    no ``label`` column (as the reference's encode.py)."""
    ann = dataset.df_annotation
    if "label" not in ann.columns:
        return None
    return ann.drop(columns=["onset_ix", "offset_ix", "length"], errors="ignore")


def join_annotation(table, ann):
    """``table`` with the annotation columns of its ``data_ix`` appended."""
    if ann is None:
        return table
    return pd.concat([table, ann.reindex(table["data_ix"].to_numpy()).reset_index(drop=True)], axis=1)
