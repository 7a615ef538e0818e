"""Decoder input dropout, the decoder's own Philox draw and the encoder's
inter-layer dropout: cases, masks, streams and the float64 references they are
judged against.

tests/test_gpu_edges.py and tests/test_gpu_ladder.py hold every recurrent
route to the float64 oracle with the decoder's noise passed in as ``eps``, no
``xmask`` and ``hidden_dropout = 0``.  Three paths of a real training step are
left: the mask of the *next* step's cell input (read with pitch F beside
MU / LV / OUT of pitch Fp, guarded by ``b < next_bs`` or a buffer extent), the
noise the decoder draws itself (``eps == NULL``: idle members filling a
workspace one step ahead, a pre-fill, or ``philox_normal`` inline), and
``Ydrop = Y * noise`` between encoder layers.

* Part A (``MASK_CASES``): p = 0.3 on every decoder route at batch edges.  The
  rows are ``ladder_cases.DEC_ROWS`` plus ``rung1``, the first rung (F = 129,
  H = Hm = 256: ``dec_fwd_x6<13,..>`` / ``dec_bwd_w16<9,..>``) at the ladder's
  D = 32, K = 16.  The mask is ``bernoulli(0.7) / 0.7`` from a generator seeded
  per case (``mask_seed``); the oracle takes it as ``noise["xmask"]``.
* Part B (``STREAM_CASES``): ``noise.set_state(mode="philox", seed=S,
  offset=O)`` with only the Gumbel noise replayed.  The decoder's L x F block
  is element ``O + row * F + col`` of stream S (``stream``); with p > 0 the
  mask's block follows it at ``O + 4 * ceil(L F / 4)`` (``mask_offset``).
* Part C (``ENC_DROP_CASES``): the two-layer bidirectional encoder alone with
  ``hidden_dropout = 0.25`` against ``oracle.encoder_forward(hmask=...)`` with
  autograd.

This module imports no GPU code.  The batch helpers, the oracle step and the
error metrics are those of tests/edge_cases.py; rows, configurations and
routes those of tests/ladder_cases.py; the numpy Philox that of
tests/sampler_cases.py.
"""
import functools
from collections import OrderedDict

import numpy as np
import torch

import edge_cases as E
import ladder_cases as L
import sampler_cases as S

SEED = 1
P_DROP = 0.3          # decoder input dropout
P_HIDDEN = 0.25       # encoder inter-layer dropout
RUNG1 = "rung1"
RUNG1_DIMS = dict(F=129, H=256, Hm=256)


def rup16(n):
    return L.cdiv(n, 16) * 16


# ----------------------------------------------------------------------------
# rows: ladder_cases.DEC_ROWS and the first rung
# ----------------------------------------------------------------------------
def dims(row):
    return RUNG1_DIMS if row == RUNG1 else L.DEC_ROWS[row]


def config(row, rnn, B):
    if row != RUNG1:
        return L.dec_config(row, rnn, B)
    return dict(RUNG1_DIMS, D=L.DEC_D, K=L.DEC_K, rnn=rnn, plain=False, spk=0, sdim=None, B=B, greedy=False,
                persist=True)


def expected(row, rnn, B):
    """{role: dispatch string} of one training step.  The first rung's kernel
    names are test_gpu_edges.KERNELS; its grids follow ladder_cases' arithmetic."""
    if row != RUNG1:
        return L.dec_expected(row, rnn, B)
    import test_gpu_edges as TE
    ef, eb, df, db = TE.KERNELS[rnn]
    gf, gb = L.enc_grid(256, B, rnn)
    return {"enc_fwd": f"{ef} grid {gf}", "enc_bwd": f"{eb} grid {gb}",
            "dec_fwd": f"{df} grid {L.dec_grid(df, 256, B)}", "dec_bwd": f"{db} grid {L.dec_grid(db, 256, B)}"}


def meta(cfg, p=0.0):
    m = L.meta_of(cfg)
    if p:
        m["input_dropout"] = p
    return m


# ----------------------------------------------------------------------------
# Part A: input dropout
# ----------------------------------------------------------------------------
RUNG1_BATCHES = ("b1t1", "b33", "b65", "b97steep", "b160")
MASK_CASES = [(RUNG1, rnn, b) for rnn in ("LSTM", "GRU") for b in RUNG1_BATCHES] + \
    [(row, rnn, b) for row, rnn in (("f65", "LSTM"), ("f65", "GRU"), ("hm128", "LSTM"), ("hm128", "GRU"),
                                   ("h64", "LSTM"), ("stepwise", "LSTM")) for b in L.BASE_BATCHES]
MASK_FRAME_CASES = [(RUNG1, "LSTM", "b33"), ("hm128", "LSTM", "b65"), ("h64", "LSTM", "b65")]

# The mask generator's seed is MASK_SEED0 + 101 * (the case's index in
# MASK_CASES) + MASK_RESEED[case]: re-seeded until column F - 1 (the lone column
# of the ragged 16-wide tile at F = 129 / 65) holds a kept and a dropped entry
# among the rows of steps >= 1.  The table is what find_mask_reseed() returns
# for every case (`python tests/noise_cases.py` prints it);
# test_noise_cases_cpu.py asserts the property and that the table is current.
MASK_SEED0 = 7001
MASK_RESEED = {
}


def lengths_of(case):
    return E.CASES[case]


def batch_sizes(case):
    ln = lengths_of(case)
    return [sum(1 for x in ln if x > t) for t in range(ln[0])]


def draw_mask(L_, F, seed, p=P_DROP):
    g = torch.Generator().manual_seed(seed)
    return torch.empty(L_, F).bernoulli_(1.0 - p, generator=g).div_(1.0 - p)


def _mask_at(key, attempt):
    row, rnn, case = key
    return draw_mask(sum(lengths_of(case)), dims(row)["F"], MASK_SEED0 + 101 * MASK_CASES.index(key) + attempt)


def last_column_mixed(mask, bsz):
    """Column F - 1 of the rows of steps >= 1 holds a kept and a dropped entry."""
    col = mask[bsz[0]:, -1]
    return bool((col != 0).any() and (col == 0).any())


def find_mask_reseed(key, limit=50):
    bsz = batch_sizes(key[2])
    if len(bsz) < 2:
        return 0
    for a in range(limit):
        if last_column_mixed(_mask_at(key, a), bsz):
            return a
    raise RuntimeError(f"{key}: no mask with a mixed last column in {limit} seeds")


def mask_seed(key):
    return MASK_SEED0 + 101 * MASK_CASES.index(key) + MASK_RESEED.get(key, 0)


def mask_of(key):
    return _mask_at(key, MASK_RESEED.get(key, 0))


WRONG_MASKS = ("none", "row", "column", "pitch")


def wrong_mask(mask, kind, bsz):
    """The mask a mistaken read would see: none at all, the row before, the
    column before, or the flat L x F block re-read with pitch Fp (an element
    past the block reads as 1: no mask)."""
    L_, F = mask.shape
    if kind == "none":
        return torch.ones_like(mask)
    if kind == "row":
        return torch.roll(mask, 1, 0)
    if kind == "column":
        return torch.roll(mask, 1, 1)
    assert kind == "pitch"
    idx = torch.arange(L_)[:, None] * rup16(F) + torch.arange(F)[None, :]
    flat = torch.cat([mask.reshape(-1), torch.ones(int(idx.max()) + 1 - L_ * F)])
    return flat[idx]


def same_for_the_decoder(a, b, bsz):
    """Two masks the decoder cannot tell apart: equal on the rows of steps >= 1
    (step 0's input is zero)."""
    return torch.equal(a[bsz[0]:], b[bsz[0]:])


def _step_reference(row, rnn, case, noise):
    from oracle import abcd_oracle as O
    cfg = config(row, rnn, len(lengths_of(case)))
    ocfg = dict(E.oracle_cfg(cfg), greedy=cfg["greedy"])
    P = O.init_params(ocfg, 1111)
    batch, drawn = E.make_batch(lengths_of(case), cfg, SEED)
    noise = dict(drawn, **noise)
    r64 = E.oracle64(ocfg, P, batch, noise, E.N_DATA)
    r32 = E.oracle32(ocfg, P, batch, noise, E.N_DATA)
    return dict(cfg=cfg, ocfg=ocfg, P=P, batch=batch, noise=noise, r64=r64, r32=r32)


@functools.lru_cache(maxsize=None)
def mask_reference(row, rnn, case):
    """Everything the tests of one Part A case share, computed once and never
    modified.  ``noise["xmask"]`` is what the GPU is given; at one frame the
    oracle runs without it (x_0 = 0 and there is no next step: the mask cannot
    matter, and the GPU's result is held to the no-mask one)."""
    mask = mask_of((row, rnn, case))
    one_frame = len(batch_sizes(case)) == 1
    ref = _step_reference(row, rnn, case, {} if one_frame else {"xmask": mask})
    ref["noise"] = dict(ref["noise"], xmask=mask)
    return ref


def frame_e32(ref, keys=("mu", "lv", "flatten_out", "offset_logits")):
    r32, r64 = ref["r32"]["out"], ref["r64"]["out"]
    return {k: (E.rel_err(r32[k], r64[k]), E.block_err(r32[k], r64[k])) for k in keys}


# ----------------------------------------------------------------------------
# Part B: the decoder's Philox draw
# ----------------------------------------------------------------------------
GOLDEN = 0x9E3779B97F4A7C15   # a seed with a non-zero high word (test_gpu_philox.SEED)
HI = 5 << 32                  # every offset has a non-zero high word: a draw from the low word alone is another stream


def packed_row(case, step, b):
    bsz = batch_sizes(case)
    return sum(bsz[:step]) + b


def carry_offset(case, F, step, b):
    """O with O + row * F + F // 2 == 2^32 at packed row (step, b): the counter's
    low word wraps in the middle of that row."""
    return (1 << 32) - (packed_row(case, step, b) * F + F // 2)


# name -> row, rnn, batch, seed, offset (None: carry_offset at CARRY_AT), p, and the environment the step runs under
STREAM_CASES = OrderedDict([
    ("rung1-LSTM-b33", dict(row=RUNG1, rnn="LSTM", case="b33", seed=0x5EED1111, offset=HI + 12344, p=P_DROP)),
    ("rung1-GRU-b33", dict(row=RUNG1, rnn="GRU", case="b33", seed=GOLDEN ^ 0x33, offset=HI + 4)),
    ("rung1-LSTM-b160", dict(row=RUNG1, rnn="LSTM", case="b160", seed=GOLDEN, offset=None)),
    ("rung1-GRU-b160", dict(row=RUNG1, rnn="GRU", case="b160", seed=0x1234567, offset=HI + (1 << 31))),
    ("f65-LSTM-b65", dict(row="f65", rnn="LSTM", case="b65", seed=0xABCDEF0123, offset=HI + 8)),
    ("greedy-LSTM-b65", dict(row="greedy", rnn="LSTM", case="b65", seed=0xF00D, offset=HI + 1000)),
    ("hm128-LSTM-b65", dict(row="hm128", rnn="LSTM", case="b65", seed=0xBEEF0000BEEF, offset=HI + 64)),
    ("h64-LSTM-b65", dict(row="h64", rnn="LSTM", case="b65", seed=77, offset=HI + 20)),
    ("stepwise-LSTM-b65", dict(row="stepwise", rnn="LSTM", case="b65", seed=GOLDEN, offset=None)),
    ("rung1-LSTM-b33-inline", dict(row=RUNG1, rnn="LSTM", case="b33", seed=0x5EED1111, offset=HI + 12344,
                                   env={"ABCD_DEC_EPSFILL": "0"})),
])
# (step, row of the step): a row of a step >= 1 in the second 64-row tile
CARRY_AT = {"rung1-LSTM-b160": (1, 74), "stepwise-LSTM-b65": (1, 64)}
# the second (seed, offset) of the no-stale-workspace runs
STALE_CASES = OrderedDict([("rung1-LSTM-b33", (0xC0FFEE, HI + 40)), ("hm128-LSTM-b65", (0xC0FFEE00C0FFEE, HI + 96))])
# idle members of the x6 forms that draw the noise a step ahead: 32 members, two per 16-wide emit tile
IDLE_MEMBERS = {"rung1-LSTM-b33": 14, "rung1-GRU-b33": 14, "rung1-LSTM-b160": 14, "rung1-GRU-b160": 14,
                "f65-LSTM-b65": 22}


def stream_spec(name):
    c = dict(STREAM_CASES[name])
    c.setdefault("p", 0.0)
    c.setdefault("env", {})
    c["F"] = dims(c["row"])["F"]
    c["L"] = sum(lengths_of(c["case"]))
    if c["offset"] is None:
        c["offset"] = carry_offset(c["case"], c["F"], *CARRY_AT[name])
    return c


def stream(seed, offset, L_, F):
    """The decoder's L x F noise block: element (row, col) is the Box-Muller
    normal of counter offset + row * F + col of stream `seed` (float64)."""
    return S.normal(seed, S.indices(offset, L_ * F)).reshape(L_, F)


def mask_offset(offset, L_, F):
    """Where the input-dropout mask's block starts: noise.philox reserves
    whole groups of four counters."""
    return offset + 4 * L.cdiv(L_ * F, 4)


def stream_mask(seed, offset, L_, F, p=P_DROP):
    """The mask abcd_fill_dropout draws behind the decoder's block (float64)."""
    keep, val = S.dropout(seed, S.indices(mask_offset(offset, L_, F), L_ * F), p)
    return (keep * val).reshape(L_, F)


WRONG_STREAMS = ("pitch", "offset0", "low_word", "next_block")


def wrong_stream(seed, offset, L_, F, kind):
    rows, cols = np.arange(L_, dtype=np.uint64)[:, None], np.arange(F, dtype=np.uint64)[None, :]
    base = np.uint64(offset)
    if kind == "pitch":
        idx = base + rows * np.uint64(rup16(F)) + cols
    elif kind == "offset0":
        idx = rows * np.uint64(F) + cols
    elif kind == "low_word":
        idx = (base + rows * np.uint64(F) + cols) & np.uint64(0xFFFFFFFF)
    else:
        assert kind == "next_block"
        idx = base + np.uint64(L_ * F) + rows * np.uint64(F) + cols
    return S.normal(seed, idx)


def eps_hat(flatten_out, mu, lv):
    """(the noise the step used, the elementwise tolerance it is known to):
    eps = (x - mu) exp(-lv / 2) in float64.  1e-4 is what test_gpu_philox.py
    grants the device's Box-Muller; x and mu are stored fp32 values of
    mu + exp(lv / 2) eps, each within an ulp (2^-23 relative) of it even after
    the kernel's fast exp, and the division scales both roundings by
    exp(-lv / 2): 2^-22 (|x| + |mu|) exp(-lv / 2)."""
    x, m, v = (np.asarray(t.detach().double().cpu()) for t in (flatten_out, mu, lv))
    s = np.exp(-0.5 * v)
    return (x - m) * s, 1e-4 + 2.0 ** -22 * (np.abs(x) + np.abs(m)) * s


def tiles_with_rows(case, rows=L.ROWS):
    """(first packed row, one past the last) of every 64-row tile of every step that has rows."""
    out, o = [], 0
    for bs in batch_sizes(case):
        out += [(o + r, o + min(r + rows, bs)) for r in range(0, bs, rows)]
        o += bs
    return out


def stream_reference(name, eps, xmask=None):
    """The oracle step (float64, fp32) of a Part B case fed the noise the
    device drew (``eps``, and the mask where p > 0)."""
    c = stream_spec(name)
    noise = {"eps": eps} if xmask is None else {"eps": eps, "xmask": xmask}
    return _step_reference(c["row"], c["rnn"], c["case"], noise)


# ----------------------------------------------------------------------------
# Part C: encoder inter-layer dropout
# ----------------------------------------------------------------------------
ENC_DROP_CASES = [(H, rnn, b) for H, rnn in ((48, "LSTM"), (128, "LSTM"), (256, "LSTM"), (128, "GRU"))
                  for b in L.BASE_BATCHES]


def hidden_mask_seed(H, rnn, case):
    return 4242 + 13 * ENC_DROP_CASES.index((H, rnn, case))


def draw_hidden_mask(L_, width, seed):
    """The draw modules.noise.dropout_noise makes in reference mode after
    torch.manual_seed(seed): torch's global CPU generator, the same call."""
    torch.manual_seed(seed)
    return torch.empty(L_, width).bernoulli_(1 - P_HIDDEN).div_(1 - P_HIDDEN)


def _enc_run(P, ocfg, packed, dout, hmask, dtype):
    from oracle import abcd_oracle as O
    Pd = OrderedDict((k, v.detach().to(dtype).requires_grad_(k.startswith("encoder/"))) for k, v in P.items()
                     if v.is_floating_point())
    out = O.encoder_forward(Pd, packed.data.to(dtype), packed.batch_sizes, ocfg,
                            hmask=None if hmask is None else [m.to(dtype) for m in hmask])
    (out * dout.to(dtype)).sum().backward()
    res = OrderedDict(last_hidden=out.detach())
    res.update(("g/" + k[len("encoder/rnn."):], v.grad.detach().clone()) for k, v in Pd.items()
               if k.startswith("encoder/"))
    return res


@functools.lru_cache(maxsize=None)
def enc_drop_reference(H, rnn, case):
    """One two-layer bidirectional encoder with hidden_dropout = 0.25: the
    weights, batch and ``dout`` of ``ladder_cases.enc_reference``, the mask, and
    the oracle's forward with autograd in float64 (``r64``), in fp32 (``r32``)
    and in float64 without the mask (``r64_nomask``)."""
    base = L.enc_reference(H, rnn, case, 2, True)
    seed = hidden_mask_seed(H, rnn, case)
    mask = draw_hidden_mask(base["packed"].data.shape[0], 2 * H, seed)
    args = (base["P"], base["ocfg"], base["packed"], base["dout"])
    r64 = _enc_run(*args, [mask], torch.float64)
    r32 = _enc_run(*args, [mask], torch.float32)
    r64_nomask = _enc_run(*args, None, torch.float64)
    e32 = OrderedDict((k, (E.rel_err(r32[k], v), E.block_err(r32[k], v))) for k, v in r64.items())
    return dict(base, seed=seed, mask=mask, r64=r64, r32=r32, r64_nomask=r64_nomask, e32=e32)


if __name__ == "__main__":  # regenerate MASK_RESEED
    print("MASK_RESEED = {")
    for key in MASK_CASES:
        a = find_mask_reseed(key)
        if a:
            print(f"    {key!r}: {a},")
    print("}")
