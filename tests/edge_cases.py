"""Batch-edge geometries for the H = Hm = 256 recurrent kernels, and the
float64 oracle they are judged against.

The persistent kernels (``enc_fwd_persist<*,16,8>``, ``enc_bwd_w8``,
``dec_fwd_x6``, ``dec_bwd_w16``) mask rows through buffer extents, decide per
32- / 64-row group whether a step has work, and map groups to workgroups
differently when the group count is a multiple of 8.  Each entry of ``CASES``
is a list of segment lengths (sorted descending, T <= 12) built to sit on one
of those boundaries; ``tests/test_edge_cases_cpu.py`` pins that each one has
the property its name claims.

The reference is ``oracle.abcd_oracle.train_step`` with every floating tensor
cast to float64 (``oracle64``).  The same call in fp32 (``oracle32``) gives
the unit the GPU's error is measured in: what honest fp32 arithmetic costs at
the same shape.  ``block_err`` is the error per 16 x 16 block (the unit tile
every workgroup member owns), so a wrong tile cannot hide behind a tensor's
largest entry elsewhere.
"""
import functools
import json
import os
import sys
from collections import OrderedDict

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

N_DATA = 10000  # entire_data_size of the KL term (bench.py's N)


def _drawn(longest, n, seed):
    """[longest] + n lengths from U{1..longest}, sorted descending."""
    g = torch.Generator().manual_seed(seed)
    rest = torch.randint(1, longest + 1, (n,), generator=g).tolist()
    return sorted([longest] + rest, reverse=True)


# mildest to hardest (the GPU tests run them in this order)
CASES = OrderedDict([
    ("b32eq", [5] * 32),                                  # exactly one 32-row group, no shrink
    ("b1t7", [7]),
    ("b1t1", [1]),                                        # one frame
    ("b31tail", [9, 8, 7, 6, 5, 4, 3, 2] + [1] * 23),
    ("b33", [6] * 32 + [1]),                              # the 2nd 32-row group: one row for one step, then empty
    ("b65", [12] * 3 + [10] * 14 + [7] * 16 + [5] * 31 + [2]),  # bs crosses 64, 32 and 16 mid-sequence
    ("b97steep", [12] + [1] * 96),                        # 97 rows -> 1 after the first step
    ("b160", _drawn(8, 159, 160)),                        # 5 groups of 32, 3 tiles of 64: ngroups % 8 != 0
    ("b256t3", _drawn(3, 255, 256)),                      # 8 groups of 32, 16 of 16: ngroups % 8 == 0
])

# gradients that are identically zero in exact arithmetic (a product with an
# all-zero operand: h_0 = 0 in the encoder, x_0 = 0 in the decoder)
ZERO_GRADS = {
    "b1t1": {"encoder/rnn.weight_hh_l0", "encoder/rnn.weight_hh_l0_reverse", "decoder/rnn_cell.cell.weight_ih"},
}

# bench.py configuration each width set derives from, and what it overrides
WIDTHS = {
    "c2": ("c2", {}),
    "c2gru": ("c2", {"rnn": "GRU"}),
    "c5gru": ("c5gru", {}),
    "c4": ("c4", {}),
}

# The batch seed, and the rows of each (case, widths) batch that are redrawn: row
# i comes from its own generator, seeded by (SEED, i, REDRAW[...][i] or 0).  A row's
# logits depend on that row's frames alone, so rows whose float64 top-2 logit
# gap fell under ARGMAX_GAP were redrawn (the first attempt that clears it)
# until every row of every case has a gap >= ARGMAX_GAP: an argmax comparison
# under a 1e-4 logit tolerance is then a fair test.  The table is what
# find_redraws() returns (`python tests/edge_cases.py` prints it; after a change
# to the oracle's init or to make_batch, paste its output here);
# test_edge_cases_cpu.py asserts both the gap and that the table is current.
ARGMAX_GAP = 1e-3
REDRAW_GAP = 1.2e-3  # what a redraw has to clear: a margin over ARGMAX_GAP
SEED = 1
REDRAW = {
    ("b32eq", "c2"): {4: 1, 18: 1},
    ("b32eq", "c2gru"): {21: 1},
    ("b31tail", "c2"): {4: 1},
    ("b31tail", "c2gru"): {1: 1, 13: 1},
    ("b65", "c2"): {1: 1, 35: 1, 42: 1},
    ("b65", "c2gru"): {20: 1},
    ("b97steep", "c2"): {40: 1, 59: 2, 61: 1, 96: 1},
    ("b97steep", "c2gru"): {13: 1},
    ("b160", "c2"): {33: 1, 37: 1, 59: 1, 144: 1, 145: 1, 148: 1, 154: 1},
    ("b160", "c2gru"): {1: 1, 67: 1, 77: 1, 82: 1, 94: 1, 131: 1, 151: 1},
    ("b256t3", "c2"): {27: 1, 34: 1, 51: 1, 144: 1, 148: 1, 154: 2, 188: 1, 199: 1, 203: 1, 213: 1, 231: 1, 232: 1},
    ("b256t3", "c2gru"): {12: 1, 40: 1, 54: 1, 123: 1, 131: 1, 161: 1, 165: 1, 191: 1},
    ("b33", "c5gru"): {7: 1, 28: 1},
    ("b97steep", "c5gru"): {8: 1, 13: 1, 14: 1, 29: 1, 48: 1, 77: 1, 91: 1, 94: 1, 96: 1},
    ("b160", "c5gru"): {8: 1, 59: 1, 90: 1, 112: 1, 118: 1, 129: 1, 134: 1, 139: 2},
}


def config(widths, B):
    import bench
    base, over = WIDTHS[widths]
    return dict(bench.CONFIGS[base], B=B, **over)


def oracle_cfg(cfg):
    from oracle import abcd_oracle as O
    return O.default_cfg(F=cfg["F"], H=cfg["H"], Hdec=cfg["H"], Hm=cfg["Hm"], D=cfg["D"], K=cfg["K"] or 16,
                         rnn=cfg["rnn"], plain=cfg["plain"], fplain=cfg["D"],
                         num_speakers=cfg["spk"] or None, speaker_dim=cfg["sdim"])


def make_batch(lengths, cfg, seed, redraw=None):
    """A packed batch of the given segment lengths (sorted descending):
    N(0, 1) frames (row i from a generator of its own, seeded by the batch
    seed, i and redraw[i]), is_offset 1 on each segment's last frame, the
    sampler's noise (Gumbel, or N(0, 1) for the plain model), the decoder's
    eps and the speakers from the batch seed's generator."""
    assert list(lengths) == sorted(lengths, reverse=True)
    F = cfg["F"]
    redraw = redraw or {}
    seqs = [torch.randn(T, F, generator=torch.Generator().manual_seed(seed + 7919 * (i + 1) + 104729 * redraw.get(i, 0)))
            for i, T in enumerate(lengths)]
    g = torch.Generator().manual_seed(seed)
    packed = torch.nn.utils.rnn.pack_sequence(seqs)
    is_off = torch.nn.utils.rnn.pack_sequence([torch.tensor([0.0] * (T - 1) + [1.0]) for T in lengths]).data
    B = len(lengths)
    feat = torch.randn(B, cfg["D"], generator=g) if cfg["plain"] else \
        -torch.empty(B, cfg["K"]).exponential_(generator=g).log()
    eps = torch.randn(packed.data.shape[0], F, generator=g)
    spk = torch.randint(0, max(cfg["spk"], 1), (B,), generator=g)
    batch = dict(data=packed.data, batch_sizes=packed.batch_sizes, is_offset=is_off, speakers=spk)
    return batch, dict(feat=feat, eps=eps)


def _cast(d, dtype):
    return type(d)((k, v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items())


def _oracle(cfg, P, batch, noise, N, dtype):
    from oracle import abcd_oracle as O
    out, grads, new, total, _ = O.train_step(_cast(P, dtype), _cast(batch, dtype), cfg, _cast(noise, dtype), N)
    if dtype == torch.float64:  # train_step rounds the norm to fp32: restate it (and the clipped update) in float64
        tot = torch.sqrt(sum((g ** 2).sum() for g in grads.values()))
        coef = torch.clamp(1.0 / (tot + 1e-6), max=1.0)
        new = OrderedDict((k, P[k].to(dtype) - grads[k] * coef if k in grads else P[k].to(dtype)) for k in P)
        total = float(tot)
    delta = OrderedDict((k, new[k].double() - P[k].double()) for k in grads)
    return dict(out=out, grads=grads, new=new, total=total, delta=delta)


def oracle64(cfg, P, batch, noise, N):
    """One oracle training step (lr = 1, momentum = 0, clip = 1) in float64."""
    return _oracle(cfg, P, batch, noise, N, torch.float64)


def oracle32(cfg, P, batch, noise, N):
    """The same step in fp32: the reference's own rounding error."""
    return _oracle(cfg, P, batch, noise, N, torch.float32)


def _abs_diff(a, ref, slack):
    d = (a.detach().double().cpu() - ref.detach().double().cpu()).abs()
    return d if slack is None else (d - slack.detach().double().cpu()).clamp_min(0.0)


def rel_err(a, ref, slack=None):
    """max|a - ref| / max|ref| over the whole tensor (slack: an elementwise
    allowance taken off |a - ref| first, see ``store_slack``)."""
    ref = ref.detach().double().cpu()
    return _abs_diff(a, ref, slack).max().item() / max(ref.abs().max().item(), 1e-30)


def block_err(a, ref, bs=16, floor=1e-2, slack=None):
    """The worst bs x bs block of max|a - ref| / max(block max|ref|, floor *
    tensor max|ref|).  The tensor is zero-padded to whole blocks; a 1-D tensor
    is one row."""
    diff = _abs_diff(a, ref, slack)
    ref = ref.detach().double().cpu()
    if ref.dim() < 2:
        diff, ref = diff.reshape(1, -1), ref.reshape(1, -1)
    diff, ref = diff.reshape(diff.shape[0], -1), ref.reshape(ref.shape[0], -1)
    R, C = ref.shape
    Rp, Cp = -(-R // bs) * bs, -(-C // bs) * bs
    pad = torch.nn.functional.pad
    d = pad(diff, (0, Cp - C, 0, Rp - R)).reshape(Rp // bs, bs, Cp // bs, bs).amax((1, 3))
    m = pad(ref.abs(), (0, Cp - C, 0, Rp - R)).reshape(Rp // bs, bs, Cp // bs, bs).amax((1, 3))
    lo = max(floor * ref.abs().max().item(), 1e-30)
    return (d / m.clamp_min(lo)).max().item()


def store_slack(new64):
    """What storing an updated parameter in fp32 costs: half an ulp of each
    entry (<= 2^-24 |p|).  A post-SGD delta is read back as fp32(p_new) - p, so
    it carries that rounding whatever computed the update -- at these shapes
    the clipped update is 1e-2 .. 1e-5 of the parameter, and the rounding alone
    is 1e-5 .. 1e-2 of the delta.  It is taken off the measured delta's error
    elementwise before the error is judged."""
    return new64.detach().double().abs() * 2.0 ** -24


def top2_gap(logits):
    """The smallest gap between a row's two largest logits."""
    top = logits.double().topk(2, -1).values
    return float((top[:, 0] - top[:, 1]).min())


def logits64(case, widths, redraw):
    """The float64 oracle's logits (B x K) of a case's batch drawn with `redraw`."""
    from oracle import abcd_oracle as O
    lengths = CASES[case]
    cfg = config(widths, len(lengths))
    ocfg = oracle_cfg(cfg)
    P = _cast(O.init_params(ocfg, 1111), torch.float64)
    batch, _ = make_batch(lengths, cfg, SEED, redraw)
    with torch.no_grad():
        return O.abcd_logits(P, O.encoder_forward(P, batch["data"].double(), batch["batch_sizes"], ocfg))


def find_redraws(case, widths, limit=60):
    """The REDRAW entry of (case, widths): from no redraws, every row whose
    top-2 gap is under REDRAW_GAP moves to its next attempt, until none is."""
    redraw = {}
    for _ in range(limit):
        top = logits64(case, widths, redraw).topk(2, -1).values
        bad = ((top[:, 0] - top[:, 1]) < REDRAW_GAP).nonzero().flatten().tolist()
        if not bad:
            return redraw
        for i in bad:
            redraw[i] = redraw.get(i, 0) + 1
    raise RuntimeError(f"{case}/{widths}: rows {bad} still under the gap after {limit} attempts")


@functools.lru_cache(maxsize=None)
def reference(case, widths):
    """Everything the tests of one (case, widths) share, computed once and
    never modified: the configuration, seed-1111 weights, the batch, the
    noise, and the float64 and fp32 oracle steps."""
    from oracle import abcd_oracle as O
    lengths = CASES[case]
    cfg = config(widths, len(lengths))
    ocfg = oracle_cfg(cfg)
    P = O.init_params(ocfg, 1111)
    batch, noise = make_batch(lengths, cfg, SEED, REDRAW.get((case, widths)))
    r64 = oracle64(ocfg, P, batch, noise, N_DATA)
    r32 = oracle32(ocfg, P, batch, noise, N_DATA)
    return dict(cfg=cfg, ocfg=ocfg, P=P, batch=batch, noise=noise, r64=r64, r32=r32)


def oracle_errors(ref):
    """{tensor: (rel_err, block_err)} of the fp32 oracle against the float64
    one: gradients ("g/<name>"), the forward tensors, the clip norm ("norm":
    relative, both slots) and post-SGD deltas ("d/<name>").  A delta is
    coef(norm) x gradient, and both metrics are scale-free, so its fp32 error
    is the gradient's plus the norm's; the fp32 oracle's own stored delta is
    not used (it measures the oracle's parameter rounding, see store_slack)."""
    r32, r64 = ref["r32"], ref["r64"]
    e = OrderedDict()
    for k in ("last_hidden", "logits", "feats"):
        e[k] = (rel_err(r32["out"][k], r64["out"][k]), block_err(r32["out"][k], r64["out"][k]))
    for k, g in r64["grads"].items():
        e["g/" + k] = (rel_err(r32["grads"][k], g), block_err(r32["grads"][k], g))
    n = abs(r32["total"] - r64["total"]) / r64["total"]
    e["norm"] = (n, n)
    for k in r64["delta"]:
        e["d/" + k] = (e["g/" + k][0] + n, e["g/" + k][1] + n)
    return e


def dump_observed(name, rows):
    """ABCD_PARITY_DUMP=<dir>: keep the figures a GPU test observed as
    <dir>/<name>.json (scripts/parity_table.py assembles
    profiles/parity_errors.json from them).  Unset: nothing is written."""
    d = os.environ.get("ABCD_PARITY_DUMP")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":  # regenerate REDRAW
    print("REDRAW = {")
    for c, w in [(c, w) for c in CASES for w in ("c2", "c2gru")] + [(c, "c5gru") for c in ("b33", "b97steep", "b160")]:
        r = find_redraws(c, w)
        if r:
            print(f'    ("{c}", "{w}"): {r},')
    print("}")
