"""Cases and the float64 reference of per-segment scoring
(``abcd_segment_losses``, ``abcd_sampler_kl_rows``,
``RNN_Variational_Decoder.score``, ``ABCDSampler.kl_rows``, ``score.py``).

The reference is numpy / torch float64 on the SAME fp32 inputs the kernels
read: the per-row terms of the emission NLL and the offset BCE, summed into
segments through the packed layout's row -> segment map (``segment_of_rows``),
and the KL's row terms with ``torch.digamma`` / ``torch.lgamma`` in float64.

Every error is measured in a unit that cannot cancel: the float64 sum of the
ABSOLUTE values of the terms a result adds up.  For the emission NLL that is
``A_b = sum 0.5 (log 2pi + |lv| + d^2 e^-lv)`` over the segment (log-variances
of both signs are drawn so that the NLL itself may cancel); BCE terms are
non-negative, so their sum is its own unit; for a KL row it is ``sum_k |q log
q| + |q elog_k|``, for the plain row ``0.5 sum (1 + |lv| + mu^2 + e^lv)``, for
the Dirichlet bracket the sum of the absolute values of its lgamma and elog
terms.  The bar is the project's loss bar, 1e-4 of that unit.
"""
import functools
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import edge_cases as E  # noqa: E402
from golden_io import batch_from, load_small, params_from, small_cfg  # noqa: E402

LOG2PI = math.log(2 * math.pi)
BAR = 1e-4            # the project's loss bar
SUM_BAR = 2.0 ** -21  # sum_b seg[b] against the decoder's own scalar, in units of A (test_gpu_score.py)
KL_SUM_BAR = 1e-5     # prior * B / N + sum rows against abcd_sampler_kl (two HIP forms, test_gpu_persist.py)
N_DATA = E.N_DATA
PAD_LD = 144          # the padded row stride the ABI cases also run at (roundup16(129))


def _drawn(longest, n, seed):
    g = torch.Generator().manual_seed(seed)
    return sorted([longest] + torch.randint(1, longest + 1, (n,), generator=g).tolist(), reverse=True)


# segment lengths (sorted descending) of the ABI cases: the smallest shapes at
# which the segment indexing can go wrong
ABI_SHAPES = OrderedDict([
    ("b1t1", [1]),                          # one row
    ("ties", [7, 7, 3, 1, 1]),              # equal lengths and length-1 segments
    ("b33t9", _drawn(9, 32, 33)),           # one past a 32-row boundary, T not a multiple of the 4 waves
    ("b97steep", E.CASES["b97steep"]),      # 97 rows falling to 1
])
ABI_F = (1, 65, 129)                        # one column, one past a 64-lane pass, the c2 bin count

# KL cases: (name, K or f of the C configuration, valid size or 0, plain)
KL_CASES = OrderedDict([
    ("k16", (16, 0, False)),
    ("k128", (128, 0, False)),
    ("k10pad", (16, 10, False)),            # the zero-padded K = 10 model: columns 10..15 are padding
    ("plain16", (16, 0, True)),
    ("plain10pad", (16, 10, True)),         # f = 10 padded to 16: padding mean = log_var = 0
])
KL_B = (1, 5, 33)

# end-to-end cases: small fixtures (full step fixtures of tests/golden) and one H = 256 batch edge
E2E_SMALL = ("lstm_speaker", "gru_gumbel", "lstm_odd")
E2E_EDGE = ("b65", "c2")
# decoder-scalar consistency: three batch-edge geometries at the H = 256 widths, and the odd small model
SUM_EDGES = (("b33", "c2"), ("b97steep", "c2gru"), ("b160", "c2"))


# ----------------------------------------------------------------------------
# the packed layout
# ----------------------------------------------------------------------------
def batch_sizes_of(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.array([(lengths > t).sum() for t in range(int(lengths.max()))], dtype=np.int64)


def segment_of_rows(batch_sizes):
    """seg[r] = the segment packed row r belongs to: step t owns rows
    off[t] .. off[t] + bs[t], row off[t] + b is segment b's."""
    return np.concatenate([np.arange(int(b), dtype=np.int64) for b in batch_sizes])


def lengths_of(batch_sizes):
    bs = np.asarray(batch_sizes, dtype=np.int64)
    return np.array([(bs > b).sum() for b in range(int(bs[0]))], dtype=np.int64)


def segment_sums(batch_sizes, per_row):
    """float64 sum of a per-row quantity (L values) into its B segments."""
    bs = np.asarray(batch_sizes, dtype=np.int64)
    out = np.zeros(int(bs[0]), dtype=np.float64)
    np.add.at(out, segment_of_rows(bs), np.asarray(per_row, dtype=np.float64))
    return out


# ----------------------------------------------------------------------------
# per-row terms in float64 (inputs as given, e.g. fp32 tensors)
# ----------------------------------------------------------------------------
def _np64(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def emission_rows(gt, mu, lv):
    """(per-row NLL, per-row unit): sums over the F columns of
    0.5 (log 2pi + lv + d^2 e^-lv) and of 0.5 (log 2pi + |lv| + d^2 e^-lv)."""
    gt, mu, lv = _np64(gt), _np64(mu), _np64(lv)
    q = (gt - mu) ** 2 * np.exp(-lv)
    return (0.5 * (LOG2PI + lv + q)).sum(1), (0.5 * (LOG2PI + np.abs(lv) + q)).sum(1)


def bce_rows(x, y):
    x, y = _np64(x), _np64(y)
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def segment_reference(batch_sizes, gt=None, mu=None, lv=None, x=None, y=None):
    """dict(em, A, off, lengths): float64 per-segment emission NLL, its unit
    A_b, the offset BCE (its own unit) and the lengths."""
    out = dict(lengths=lengths_of(batch_sizes))
    if gt is not None:
        nll, unit = emission_rows(gt, mu, lv)
        out["em"], out["A"] = segment_sums(batch_sizes, nll), segment_sums(batch_sizes, unit)
    if x is not None:
        out["off"] = segment_sums(batch_sizes, bce_rows(x, y))
    return out


def padded_loop_reference(lengths, gt, mu, lv, x, y):
    """The same sums the slow way: unpack to one (T_b x F) block per sequence
    (pad_packed_sequence) and loop over the sequences."""
    bs = torch.from_numpy(batch_sizes_of(lengths))
    PS = torch.nn.utils.rnn.PackedSequence

    def pad(t):
        return torch.nn.utils.rnn.pad_packed_sequence(PS(torch.as_tensor(t).double(), bs), batch_first=True)[0]
    G, M, V, X, Y = (pad(t) for t in (gt, mu, lv, x, y))
    em, off = [], []
    for b, n in enumerate(lengths):
        g, m, v = G[b, :n], M[b, :n], V[b, :n]
        em.append(float((0.5 * (LOG2PI + v + (g - m) ** 2 * torch.exp(-v))).sum()))
        off.append(float(torch.nn.functional.binary_cross_entropy_with_logits(X[b, :n], Y[b, :n], reduction="sum")))
    return np.array(em), np.array(off)


# ----------------------------------------------------------------------------
# KL rows in float64
# ----------------------------------------------------------------------------
def kl_reference(logits, psl, a0, N):
    """ABCDSampler.kl_divergence (model.py:608-639) in float64, split:
    dict(rows, row_unit, prior, prior_unit, kl) with kl = prior * B / N + sum rows."""
    lg = torch.as_tensor(logits).double()
    psl = torch.as_tensor(psl).double()
    K = psl.shape[0]
    # the reference forms softmax(psl) * N + a0 in fp32; its float64 value is the reference here
    alpha = torch.softmax(psl, -1) * N + a0
    S = alpha.sum()
    elog = torch.digamma(alpha) - torch.digamma(S)
    terms_q = [torch.lgamma(S), -torch.lgamma(alpha).sum(), ((alpha - 1.0) * elog).sum()]
    a0t = torch.tensor(float(a0), dtype=torch.float64)
    terms_p = [torch.lgamma(a0t * K), -torch.lgamma(a0t) * K, ((a0 - 1.0) * elog).sum()]
    prior = float(sum(terms_q) - sum(terms_p))
    prior_unit = float(torch.lgamma(S).abs() + torch.lgamma(alpha).abs().sum() + ((alpha - 1.0) * elog).abs().sum()
                       + torch.lgamma(a0t * K).abs() + torch.lgamma(a0t).abs() * K
                       + ((a0 - 1.0) * elog).abs().sum())
    q = torch.softmax(lg, -1)
    logq = torch.log_softmax(lg, -1)
    rows = (q * logq).sum(-1) - (q * elog[None, :]).sum(-1)
    unit = (q * logq).abs().sum(-1) + (q * elog[None, :]).abs().sum(-1)
    B = lg.shape[0]
    return dict(rows=rows.numpy(), row_unit=unit.numpy(), prior=prior, prior_unit=prior_unit,
                kl=prior * B / N + float(rows.sum()))


def plain_kl_reference(mu, lv):
    """-0.5 sum_f (1 + lv - mu^2 - e^lv) per row and its unit."""
    mu, lv = _np64(mu), _np64(lv)
    return (-0.5 * (1.0 + lv - mu ** 2 - np.exp(lv))).sum(1), (0.5 * (1.0 + np.abs(lv) + mu ** 2 + np.exp(lv))).sum(1)


# ----------------------------------------------------------------------------
# inputs of the C-ABI cases
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def abi_inputs(shape, F):
    """Random fp32 inputs of one (shape, F): mu N(0, 1), log_var U[-6, 2] (terms
    of both signs), gt = mu + N(0, 1) e^{lv / 2} 1.5, offset logits U[-8, 8],
    0/1 targets; and their float64 reference.  Shared, never modified."""
    lengths = ABI_SHAPES[shape]
    bs = batch_sizes_of(lengths)
    L = int(bs.sum())
    g = torch.Generator().manual_seed(1000 * len(lengths) + F)
    mu = torch.randn(L, F, generator=g)
    lv = torch.rand(L, F, generator=g) * 8.0 - 6.0
    gt = mu + torch.randn(L, F, generator=g) * torch.exp(0.5 * lv) * 1.5
    x = torch.rand(L, generator=g) * 16.0 - 8.0
    y = (torch.rand(L, generator=g) < 0.3).float()
    ref = segment_reference(bs, gt, mu, lv, x, y)
    return dict(lengths=lengths, batch_sizes=bs, L=L, F=F, gt=gt, mu=mu, lv=lv, x=x, y=y, ref=ref)


@functools.lru_cache(maxsize=None)
def kl_inputs(name, B):
    """Random logits N(0, 2^2) and shape logits N(0, 1) of a KL case and the
    float64 reference on the model's own (valid) columns.  Padding columns of
    the logits and shape logits hold 50.0: a kernel that read them would be
    far off."""
    width, valid, plain = KL_CASES[name]
    real = valid or width
    g = torch.Generator().manual_seed(97 * B + width + 7 * real + plain)
    if plain:
        mu, lv = torch.randn(B, real, generator=g), torch.rand(B, real, generator=g) * 4.0 - 3.0
        mv = torch.zeros(B, 2 * width)
        mv[:, :real], mv[:, width:width + real] = mu, lv
        rows, unit = plain_kl_reference(mu, lv)
        return dict(plain=True, logits=mv, psl=None, a0=1.0, width=width, valid=valid,
                    ref=dict(rows=rows, row_unit=unit, prior=0.0, prior_unit=1.0, kl=float(rows.sum())))
    logits = torch.full((B, width), 50.0)
    logits[:, :real] = torch.randn(B, real, generator=g) * 2.0
    psl = torch.full((width,), 50.0)
    psl[:real] = torch.randn(real, generator=g)
    a0 = 0.5 if name == "k128" else 1.0
    return dict(plain=False, logits=logits, psl=psl, a0=a0, width=width, valid=valid,
                ref=kl_reference(logits[:, :real], psl[:real], a0, N_DATA))


# ----------------------------------------------------------------------------
# the float64 oracle's per-segment scores (eps = 0, eval mode)
# ----------------------------------------------------------------------------
def oracle_scores(P, ocfg, batch, N):
    """The deterministic score of a batch under the float64 oracle: encoder ->
    logits -> softmax features -> decoder with eps = 0 and train=False, its
    losses segmented by ``segment_reference``; the KL by ``kl_reference``."""
    from oracle import abcd_oracle as O
    P64 = E._cast(P, torch.float64)
    data, bsz = batch["data"].double(), batch["batch_sizes"]
    with torch.no_grad():
        h = O.encoder_forward(P64, data, bsz, ocfg)
        logits = O.abcd_logits(P64, h)
        feats = O.abcd_sample(P64, logits, None)
        spk = batch.get("speakers") if ocfg["num_speakers"] else None
        em, off, _, (mu, lv), offl = O.decoder_forward(P64, feats, bsz, ocfg, torch.zeros_like(data), speakers=spk,
                                                       gt=data, gt_off=batch["is_offset"].double(), train=False)
        kl = O.digamma_kl(P64, logits, N)
    seg = segment_reference(bsz.numpy(), data, mu, lv, offl, batch["is_offset"])
    klr = kl_reference(logits, P64["feature_sampler/posterior_shape_logits"],
                       float(P64["feature_sampler/prior_concentration"]), N)
    return dict(em=seg["em"], off=seg["off"], lengths=seg["lengths"], rows=klr["rows"], prior=klr["prior"],
                logits=logits, em_total=float(em), off_total=float(off), kl_total=float(kl))


@functools.lru_cache(maxsize=None)
def small_reference(name):
    meta, arr = load_small(name)
    ocfg = small_cfg(meta)
    P, batch = params_from(arr), batch_from(arr)
    return dict(meta=meta, arr=arr, ocfg=ocfg, P=P, batch=batch, scores=oracle_scores(P, ocfg, batch, N_DATA))


@functools.lru_cache(maxsize=None)
def edge_reference(case, widths):
    """The batch of an edge_cases geometry (its weights, frames and speakers;
    the training step's oracle is not run) and its oracle scores."""
    from oracle import abcd_oracle as O
    lengths = E.CASES[case]
    cfg = E.config(widths, len(lengths))
    ocfg = E.oracle_cfg(cfg)
    P = O.init_params(ocfg, 1111)
    batch, _ = E.make_batch(lengths, cfg, E.SEED, E.REDRAW.get((case, widths)))
    return dict(cfg=cfg, ocfg=ocfg, P=P, batch=batch, lengths=lengths)


def checkpoint_oracle(ckpt):
    """(P, ocfg) of a checkpoint written by learning.py (ABCD model)."""
    from oracle import abcd_oracle as O
    P = OrderedDict()
    for pfx in ("encoder", "feature_sampler", "decoder"):
        P.update({f"{pfx}/{k}": v for k, v in ckpt[pfx].items()})
    e, s, d = (ckpt[k + "_init_parameters"] for k in ("encoder", "feature_sampler", "decoder"))
    ocfg = O.default_cfg(F=e["input_size"], H=e["rnn_hidden_size"], Hdec=d["rnn_hidden_size"],
                         Hm=s["mlp_hidden_size"], D=s["feature_dim"], K=s["num_categories"], rnn=e["rnn_type"],
                         dec_rnn=d["rnn_type"], layers=e.get("rnn_layers", 1),
                         bidirectional=e.get("bidirectional", True),
                         prior_concentration=s.get("prior_concentration", 1.0))
    return P, ocfg


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as edge_cases.dump_observed)."""
    E.dump_observed("score_" + name, rows)
