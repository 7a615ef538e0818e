"""Width-edge geometries for the sampler kernels, the float64 oracle they are
judged against, and a numpy Philox4x32-10 with the kernels' transforms.

``samp_head_fwd`` / ``samp_head_bwd`` (abcd_sampler.hip) dispatch on KPL =
ceil(K / 64) rounded up to a power of two (1 .. 16), size their LDS rows by
max(Hm, K) and max(D, K), deal the 16-column subtiles of every product two at
a time to 8 waves, and reduce the KL / perplexity / bias sums over the 16-row
tiles in their last workgroup (32 tiles at a time, then a tail).  Past K = 1024
or 160 KiB of LDS the fused entry points fall back to the per-method kernels.
Each entry of ``CASES`` sits on one of those boundaries;
``tests/test_sampler_cases_cpu.py`` pins that each has the property its name
claims.

The reference is ``oracle.abcd_oracle`` (abcd_logits, abcd_sample, digamma_kl,
perplexities; plain: plain_params, mu + exp(lv / 2) eps, gaussian_kl) with
autograd, in float64 (``r64``) and in float32 (``r32``); ``e32`` -- r32 against
r64 in ``edge_cases.rel_err`` and ``edge_cases.block_err`` -- is the unit the
GPU's error is measured in.  The scalar that is differentiated is
``(feats * d_feats).sum() + d_kl * kl`` with d_feats = randn / B, d_kl = 1 / B.
A padded case's reference is the oracle on the un-padded (Kv, Dv) model; the
GPU gets the zero-padded twin ``modules/padding.py`` makes.
"""
import functools
import math
import os
import sys
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from edge_cases import ARGMAX_GAP, REDRAW_GAP, block_err, rel_err  # noqa: F401  (shared with the tests)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "seq2seq_abcd-vae_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_DATA = 10000  # entire_data_size of the KL term
SEED = 1
HEAD_ROWS = 16          # rows of one samp_head tile
HEAD_WAVES = 8          # HEAD_THREADS / 64
HEAD_LDS_MAX = 160 * 1024

# every width a multiple of 16 (samp_check); Kv / Dv: the model's own sizes where they are padded
CASES = OrderedDict([
    ("k16_b520", dict(E=64, Hm=32, K=16, D=16, B=520)),          # KPL 1; one subtile for 8 waves; 33 tiles
    ("k80_b17", dict(E=64, Hm=48, K=80, D=32, B=17)),            # KPL 2; subtiles 3 / 5 / 2; 2nd tile: one row
    ("k144_b33_tau01", dict(E=128, Hm=112, K=144, D=48, B=33, tau=0.1, a0=0.1)),  # KPL 4
    ("k272pad_b15", dict(E=128, Hm=112, K=272, Kv=260, D=48, Dv=40, B=15)),       # KPL 8; one ragged tile; padded
    # codebook x 4: logits of std ~1 over 528 categories; the tau = 0.5 Gumbel sample peaks at 0.55, the softmax at 0.03
    ("k528_b1_peaked", dict(E=1024, Hm=256, K=528, D=256, B=1, cb_scale=4.0)),    # KPL 16 below 1024; one row
    ("k1024pad_b16", dict(E=1024, Hm=256, K=1024, Kv=1000, D=256, B=16)),         # KPL 16, padded; one full tile
    ("hm512_b31", dict(E=64, Hm=512, K=64, D=128, B=31)),        # Hm > K, D > K: LDS pitches from Hm and D
    ("k1040_b17", dict(E=64, Hm=48, K=1040, D=32, B=17)),        # K > 1024: per-method fallback
    ("lds_b17", dict(E=64, Hm=2048, K=64, D=512, B=17)),         # head LDS > 160 KiB: fallback
    ("plain_b17", dict(E=64, Hm=48, K=0, D=32, Dv=20, B=17, plain=True)),  # plain Gaussian sampler, padded f
])
ABCD_CASES = [c for c in CASES if not CASES[c].get("plain")]
FALLBACK = ("k1040_b17", "lds_b17")  # the fused entries run the per-method kernels
MODES = ("gumbel", "softmax")

_PRE = "feature_sampler/to_code_like.whole_network"
_PPRE = "feature_sampler/to_parameters.mlps.%d.whole_network"
PSL, CB = "feature_sampler/posterior_shape_logits", "feature_sampler/codebook"

# Rows of each case's h that are redrawn: row i comes from its own generator,
# seeded by (SEED, case, i, REDRAW[case][i] or 0).  A row's logits depend on
# that row alone, so rows whose float64 top-2 logit gap fell under REDRAW_GAP
# were redrawn until every row clears it (`python tests/sampler_cases.py`
# prints the table; test_sampler_cases_cpu.py asserts it is current).
REDRAW = {
    "k16_b520": {73: 1, 116: 1},
    "k144_b33_tau01": {9: 1, 20: 1},
}


def spec(case):
    """The case with its defaults filled in."""
    c = dict(CASES[case])
    c.setdefault("Kv", c["K"])
    c.setdefault("Dv", c["D"])
    c.setdefault("tau", 0.5)
    c.setdefault("a0", 1.0)
    c.setdefault("cb_scale", 1.0)
    c.setdefault("plain", False)
    c["index"] = list(CASES).index(case)
    return SimpleNamespace(**c)


def kpl(K):
    """Categories per lane: ceil(K / 64) rounded up to a power of two."""
    n = -(-K // 64)
    return 1 << (n - 1).bit_length()


def tiles(B):
    return -(-B // HEAD_ROWS)


def head_fwd_lds(Hm, D, K):
    return (HEAD_ROWS * (max(Hm, K) + 4) + HEAD_ROWS * (max(D, K) + 4) + 2 * K) * 4 + 16 * 8 + 16


def head_bwd_lds(Hm, D, K):
    return (HEAD_ROWS * (K + 4) + HEAD_ROWS * (D + 4) + HEAD_ROWS * (Hm + 4) + (HEAD_WAVES + 2) * K) * 4 + 16 * 8 + 16


def fused(case):
    """Whether the fused entry points run the sampler-head kernels at this case."""
    s = spec(case)
    return (not s.plain and s.K <= 1024 and head_fwd_lds(s.Hm, s.D, s.K) <= HEAD_LDS_MAX
            and head_bwd_lds(s.Hm, s.D, s.K) <= HEAD_LDS_MAX)


def _uniform(shape, bound, g):
    return torch.empty(shape).uniform_(-bound, bound, generator=g)


def _linear(fan_in, fan_out, g):  # torch.nn.Linear's init
    return _uniform((fan_out, fan_in), 1.0 / math.sqrt(fan_in), g), _uniform((fan_out,), 1.0 / math.sqrt(fan_in), g)


@functools.lru_cache(maxsize=None)
def params(case):
    """The un-padded model's parameters under the oracle's names (fp32)."""
    s = spec(case)
    g = torch.Generator().manual_seed(1000 + s.index)
    P = OrderedDict()
    if s.plain:
        for k in range(2):
            pre = _PPRE % k
            P[pre + ".0.weight"], P[pre + ".0.bias"] = _linear(s.E, s.Hm, g)
            P[pre + ".2.weight"], P[pre + ".2.bias"] = _linear(s.Hm, s.Dv, g)
        return P
    P[PSL] = 2.0 * torch.randn(s.Kv, generator=g)
    P[CB] = s.cb_scale * torch.randn(s.Dv, s.Kv, generator=g)
    P["feature_sampler/prior_concentration"] = torch.tensor(float(s.a0))
    P[_PRE + ".0.weight"], P[_PRE + ".0.bias"] = _linear(s.E, s.Hm, g)
    P[_PRE + ".2.weight"], P[_PRE + ".2.bias"] = _linear(s.Hm, s.Dv, g)
    return P


def grad_names(case):
    return [k for k in params(case) if not k.endswith("prior_concentration")]


def padded_shape(case, name):
    s = spec(case)
    short = name.split("/", 1)[1]
    if short == "posterior_shape_logits":
        return (s.K,)
    if short == "codebook":
        return (s.D, s.K)
    layer, kind = short.split(".")[-2:]
    rows = s.Hm if layer == "0" else s.D
    return (rows, s.E if layer == "0" else s.Hm) if kind == "weight" else (rows,)


def pad_layout(case, name):
    """(rows, cols) of the real entries of a parameter in its padded twin (modules/padding.py)."""
    from modules import padding as pad
    s = spec(case)
    d = SimpleNamespace(K=s.Kv, D=s.Dv, Hm=s.Hm, in_cols=pad.prefix(s.E))
    return pad.sampler_layout(d, name.split("/", 1)[1])


def padded_params(case, P=None):
    """The zero-padded twin of the case's parameters (or of P, same names)."""
    from modules import padding as pad
    P = params(case) if P is None else P
    out = OrderedDict()
    for k, v in P.items():
        if k.endswith("prior_concentration"):
            out[k] = v
            continue
        rows, cols = pad_layout(case, k)
        out[k] = pad.embed(v, rows, cols, padded_shape(case, k))
    return out


def valid_slice(case, name, t):
    """The real entries of a padded tensor, and a copy with them zeroed (the padding alone)."""
    rows, cols = pad_layout(case, name)
    rows = rows.to(t.device)
    rest = t.clone()
    if cols is None:
        rest[rows] = 0
        return t[rows], rest
    cols = cols.to(t.device)
    rest[rows[:, None], cols[None, :]] = 0
    return t[rows[:, None], cols[None, :]], rest


def _row(case, i, attempt):
    s = spec(case)
    g = torch.Generator().manual_seed(SEED + 7919 * (i + 1) + 104729 * attempt + 15485863 * s.index)
    return torch.randn(s.E, generator=g)


def make_h(case, redraw=None):
    redraw = redraw or {}
    return torch.stack([_row(case, i, redraw.get(i, 0)) for i in range(spec(case).B)])


def _cast(d, dtype):
    return type(d)((k, v.to(dtype)) for k, v in d.items())


def logits64(case, redraw):
    from oracle import abcd_oracle as O
    with torch.no_grad():
        return O.abcd_logits(_cast(params(case), torch.float64), make_h(case, redraw).double())


def top2_gaps(logits):
    top = logits.double().topk(2, -1).values
    return top[:, 0] - top[:, 1]


def find_redraws(case, limit=60):
    """The REDRAW entry of a case: from no redraws, every row whose top-2 gap
    is under REDRAW_GAP moves to its next attempt, until none is."""
    redraw = {}
    if spec(case).plain:
        return redraw
    for _ in range(limit):
        bad = (top2_gaps(logits64(case, redraw)) < REDRAW_GAP).nonzero().flatten().tolist()
        if not bad:
            return redraw
        for i in bad:
            redraw[i] = redraw.get(i, 0) + 1
    raise RuntimeError(f"{case}: rows {bad} still under the gap after {limit} attempts")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """h (B x E), the given noise (Gumbel B x Kv; plain: N(0, 1) B x Dv) and
    the upstream gradients d_feats = randn / B (B x Dv), d_kl = 1 / B."""
    s = spec(case)
    g = torch.Generator().manual_seed(2000 + s.index)
    h = make_h(case, REDRAW.get(case))
    if s.plain:
        noise = torch.randn(s.B, s.Dv, generator=g)
    else:
        noise = -torch.empty(s.B, s.Kv).exponential_(generator=g).log()
    d_feats = torch.randn(s.B, s.Dv, generator=g) / s.B
    return dict(h=h, noise=noise, d_feats=d_feats, d_kl=torch.tensor(1.0 / s.B))


def run_oracle(case, mode, dtype, term="both", noise=None, P=None):
    """The oracle's forward and autograd backward.  mode: "gumbel" (the case's
    tau, the given noise -- `noise` overrides the case's own), "softmax", or
    "plain"; term: which part of the scalar is differentiated ("both",
    "feats", "kl").  Returns logits, feats, kl, ppl (cluster, batch), d_h and
    g/<name> for every parameter."""
    from oracle import abcd_oracle as O
    s, inp = spec(case), inputs(case)
    P = params(case) if P is None else P
    P = OrderedDict((k, v.detach().to(dtype).requires_grad_(not k.endswith("prior_concentration")))
                    for k, v in P.items())
    h = inp["h"].detach().clone().to(dtype).requires_grad_(True)  # a leaf of its own: the cached input stays as it is
    noise = (inp["noise"] if noise is None else noise).to(dtype)
    out = {}
    if s.plain:
        mu, lv = O.plain_params(P, h)
        feats = mu + (0.5 * lv).exp() * noise
        kl = O.gaussian_kl(mu, lv)
        out["logits"] = torch.cat([mu, lv], -1).detach()
    else:
        logits = O.abcd_logits(P, h)
        feats = O.abcd_sample(P, logits, noise if mode == "gumbel" else None, s.tau if mode == "gumbel" else 1.0)
        kl = O.digamma_kl(P, logits, N_DATA)
        out["logits"] = logits.detach()
        with torch.no_grad():
            out["ppl"] = O.perplexities(logits, P[PSL])[:2]
    scalar = 0.0
    if term in ("both", "feats"):
        scalar = scalar + (feats * inp["d_feats"].to(dtype)).sum()
    if term in ("both", "kl"):
        scalar = scalar + inp["d_kl"].to(dtype) * kl
    scalar.backward()
    out["feats"], out["kl"] = feats.detach(), float(kl.detach())
    out["d_h"] = h.grad.detach() if h.grad is not None else torch.zeros_like(h)
    for k, v in P.items():
        if v.requires_grad:
            out["g/" + k] = v.grad.detach() if v.grad is not None else torch.zeros_like(v)
    return out


def tensor_keys(case):
    return ["logits", "feats", "d_h"] + ["g/" + k for k in grad_names(case)]


@functools.lru_cache(maxsize=None)
def reference(case, mode, term="both"):
    """What the tests of one (case, mode) share, computed once and never
    modified: r64, r32 and e32 = {tensor: (rel_err, block_err)} of r32 against r64."""
    r64 = run_oracle(case, mode, torch.float64, term)
    r32 = run_oracle(case, mode, torch.float32, term)
    e32 = OrderedDict((k, (rel_err(r32[k], r64[k]), block_err(r32[k], r64[k]))) for k in tensor_keys(case))
    return dict(r64=r64, r32=r32, e32=e32)


# ----------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al. 2011) as abcd_common.h lays it out: counter =
# (low, high word of the 64-bit element index, 0, 0), key = (low, high word of
# the seed).  All arithmetic in uint64 arrays, masked to 32 bits.
# ----------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 words (scalars or equal-shaped arrays), key: 2 words ->
    the 4 output words as a uint32 array of shape (4,) + counter shape."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in np.broadcast_arrays(*counter)]
    k0, k1 = (np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _M32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return np.stack(c).astype(np.uint32)


def words(seed, idx):
    """The 4 words of element index idx (uint64, wraps) of stream `seed`."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10((idx & _M32, idx >> _S32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))


def indices(offset, n):
    """offset + i for i < n, modulo 2^64, as uint64."""
    return np.uint64(int(offset) & (2 ** 64 - 1)) + np.arange(int(n), dtype=np.uint64)


def u01(x):
    """((x >> 8) + 1) * 2^-24: uniform in (0, 1], exact in fp32 and float64."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def normal(seed, idx):
    """Box-Muller of words 0 and 1, in float64."""
    w = words(seed, idx)
    return np.sqrt(-2.0 * np.log(u01(w[0]))) * np.cos(2.0 * np.pi * u01(w[1]))


def gumbel(seed, idx):
    """-log(max(-log(u01(word 0)), 1e-30)), in float64."""
    e = -np.log(u01(words(seed, idx)[0]))
    return -np.log(np.maximum(e, 1e-30))


def dropout(seed, idx, p):
    """(keep mask, the kept value): keep where u01(word 0) <= fp32(1 - p),
    the kept value 1 / (1 - p) in float64."""
    keep = np.float32(1.0) - np.float32(p)
    return u01(words(seed, idx)[0]) <= np.float64(keep), 1.0 / (1.0 - float(p))


# Random123's known answers for philox4x32_10: (counter, key) -> output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


if __name__ == "__main__":  # regenerate REDRAW
    print("REDRAW = {")
    for c in CASES:
        r = find_redraws(c)
        if r:
            print(f'    "{c}": {r},')
    print("}")
