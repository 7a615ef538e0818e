"""Cases and the float64 reference of free-running generation
(``abcd_decoder_generate`` / ``RNN_Variational_Decoder.generate``).

The reference is ``oracle.abcd_oracle.decoder_forward`` in float64 on the full
rectangle (``batch_sizes = [B] * T``, ``train=False``, eps zeros for the mean or
a replayed draw), then, written out in numpy here: the stop rule
(``stop_lengths``), the stable sort and the repacking (``pack_rows``).

A length is a decision on a logit.  At random init the offset logits of a
rectangle span a few tenths, and with one threshold per case the nearest logit
is 1e-4 .. 1e-3 away -- under what fp32 kernels may differ from float64 by.
So, as ``edge_cases.py`` does for the argmax, every row whose float64 logits
come within ``STOP_GAP`` of the threshold at any step up to and including its
stop is redrawn (its feature row reseeded) until every row clears the gap; no
row is left out.  ``REDRAW`` is what ``find_redraws`` returns (``python
tests/gen_cases.py`` prints it); ``test_generate_cpu.py`` asserts the gap, that
the table is current, and that each case has what its name claims.
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

import edge_cases as E  # noqa: E402  (widths -> configuration, rel_err)
from golden_io import load_small, params_from, small_cfg  # noqa: E402

STOP_GAP = 1e-3     # 40x the 1e-4-of-max logit bar at these magnitudes (max |logit| ~ 0.25)
REDRAW_GAP = 1.2e-3  # what a redraw has to clear: a margin over STOP_GAP
SEED = 5
MEAN, SAMPLE = 0, 1  # abcd_hip.h abcd_gen_mode


def f32(x):
    """x rounded to fp32: the threshold the kernel compares with."""
    return float(np.float32(x))


def prob_to_logit(p):
    """stop_prob -> the fp32 logit ``generate()`` hands to the kernel."""
    return -math.inf if p <= 0 else math.inf if p >= 1 else f32(math.log(p / (1.0 - p)))


# widths: a bench.py width set of edge_cases.WIDTHS, or "odd" = the dimensions
# and weights of the small_lstm_odd fixture (off the 16-grid, speaker embedding).
# stop: the threshold as a logit (C ABI cases) or stop_prob (the generate() case).
CASES = OrderedDict([
    # rows that stop at step 1, rows that never stop (the mean's logits settle under the threshold) and
    # ties far apart in input order
    ("c2_mean", dict(widths="c2", B=48, T=12, mode=MEAN, stop_logit=f32(0.03), min_len=1)),
    # lengths 1 .. 8: the longest row stops before T, so batch_sizes ends in a zero
    ("c2gru_sample", dict(widths="c2gru", B=33, T=9, mode=SAMPLE, stop_logit=f32(-0.12), min_len=1)),
    # min_len = 2 lifts the rows that fire at step 1; the longest row is 4 of 6
    ("c5gru_mean", dict(widths="c5gru", B=65, T=6, mode=MEAN, stop_logit=f32(-0.05), min_len=2)),
    # through generate(): stop_prob, the padded twin, the forward's other forms; one row never stops
    ("odd_mean", dict(widths="odd", B=7, T=8, mode=MEAN, stop_prob=0.5055, min_len=1)),
])

REDRAW = {
    "c2_mean": {21: 1, 28: 1, 40: 1},
    "odd_mean": {3: 1},
}


def _model(widths, B):
    """(oracle cfg, fp32 parameters, dims dict)"""
    from oracle import abcd_oracle as O
    if widths == "odd":
        meta, arr = load_small("lstm_odd")
        ocfg = small_cfg(meta)
        return ocfg, params_from(arr), meta
    cfg = E.config(widths, B)
    ocfg = E.oracle_cfg(cfg)
    return ocfg, O.init_params(ocfg, 1111), cfg


def make_inputs(name, redraw=None):
    """features (B x D, row i from its own generator seeded by SEED, i and
    redraw[i]), speakers and eps (zeros for the mean; B*T x F, time-major)."""
    c = CASES[name]
    redraw = redraw or {}
    ocfg, P, _ = _model(c["widths"], c["B"])
    B, T, F, D = c["B"], c["T"], ocfg["F"], ocfg["D"]
    feats = torch.stack([torch.randn(D, generator=torch.Generator().manual_seed(
        SEED + 7919 * (i + 1) + 104729 * redraw.get(i, 0))) for i in range(B)])
    g = torch.Generator().manual_seed(SEED)
    nspk = ocfg["num_speakers"] or 0
    spk = torch.randint(0, max(nspk, 1), (B,), generator=g)
    eps = torch.randn(B * T, F, generator=g) if c["mode"] == SAMPLE else torch.zeros(B * T, F)
    return feats, spk, eps


def stop_logit(name):
    c = CASES[name]
    return c["stop_logit"] if "stop_logit" in c else prob_to_logit(c["stop_prob"])


def stop_lengths(logits, thr, min_len):
    """logits: T x B.  max(min_len, t* + 1), t* the first step with logit > thr
    (strict; NaN never fires); T where none does.  Also returns t* (T - 1 where none)."""
    T = logits.shape[0]
    fired = logits > thr
    any_ = fired.any(0)
    first = np.where(any_, fired.argmax(0), T - 1)
    return np.maximum(min_len, np.where(any_, first + 1, T)).astype(np.int64), first


def pack_rows(lengths, T):
    """(order, batch_sizes[T], rows): order = rows by length descending, stable;
    batch_sizes[t] = rows longer than t; rows[off[t] + j] = t * B + order[j], the
    rectangle row of packed row off[t] + j."""
    B = len(lengths)
    order = np.argsort(-lengths, kind="stable")
    bs = np.array([(lengths > t).sum() for t in range(T)], dtype=np.int64)
    rows = np.concatenate([t * B + order[:bs[t]] for t in range(T)]) if T else np.zeros(0, np.int64)
    return order.astype(np.int64), bs, rows.astype(np.int64)


def rectangle64(name, redraw=None):
    """The float64 oracle on the rectangle: dict(out, mu, lv, logits) of T*B rows."""
    from oracle import abcd_oracle as O
    c = CASES[name]
    ocfg, P, _ = _model(c["widths"], c["B"])
    feats, spk, eps = make_inputs(name, redraw)
    P64 = E._cast(P, torch.float64)
    with torch.no_grad():
        _, _, out, (mu, lv), logits = O.decoder_forward(
            P64, feats.double(), [c["B"]] * c["T"], ocfg, eps.double(),
            speakers=spk if ocfg["num_speakers"] else None, train=False)
    return dict(out=out, mu=mu, lv=lv, logits=logits)


def row_gaps(logits, thr, first):
    """Per row: the smallest |logit - thr| over steps 0 .. t* (T x B logits)."""
    T, B = logits.shape
    d = np.abs(logits - thr)
    d[np.arange(T)[:, None] > first[None, :]] = np.inf
    return d.min(0)


def find_redraws(name, limit=60):
    c = CASES[name]
    thr = stop_logit(name)
    redraw = {}
    for _ in range(limit):
        lg = rectangle64(name, redraw)["logits"].numpy().reshape(c["T"], c["B"])
        _, first = stop_lengths(lg, thr, c["min_len"])
        bad = (row_gaps(lg, thr, first) < REDRAW_GAP).nonzero()[0].tolist()
        if not bad:
            return redraw
        for i in bad:
            redraw[i] = redraw.get(i, 0) + 1
    raise RuntimeError(f"{name}: rows {bad} still under the gap after {limit} attempts")


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests of one case share, computed once, never modified."""
    c = CASES[name]
    ocfg, P, meta = _model(c["widths"], c["B"])
    feats, spk, eps = make_inputs(name, REDRAW.get(name))
    rect = rectangle64(name, REDRAW.get(name))
    thr = stop_logit(name)
    lg = rect["logits"].numpy().reshape(c["T"], c["B"])
    lengths, first = stop_lengths(lg, thr, c["min_len"])
    order, bs, rows = pack_rows(lengths, c["T"])
    idx = torch.from_numpy(rows)
    packed = {k: v[idx] for k, v in rect.items()}
    return dict(case=c, ocfg=ocfg, P=P, meta=meta, feats=feats, speakers=spk, eps=eps, stop_logit=thr, rect=rect,
                lengths=lengths, first=first, gaps=row_gaps(lg, thr, first), order=order, batch_sizes=bs,
                total=int(lengths.sum()), packed=packed)


if __name__ == "__main__":  # regenerate REDRAW
    print("REDRAW = {")
    for n in CASES:
        r = find_redraws(n)
        if r:
            print(f'    "{n}": {r},')
    print("}")
