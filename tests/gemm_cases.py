"""Cases, buffers, data and bars of the GEMM layer's route tests
(``csrc/abcd_gemm.hip``: ``abcd_gemm_nt``, ``abcd_gemm_tn``, ``abcd_linear``,
``abcd_linear_backward``).  No GPU code: tests/test_gemm_cases_cpu.py runs the
same tables, data and checks on torch's CPU GEMM, tests/test_gpu_gemm_routes.py
on the library.

Buffers.  Every operand is a view inside a larger tensor filled with NaN: a
margin before and after, rows past the valid ones, columns past the valid
width up to the leading dimension.  ``C`` is a view inside a tensor filled
with one sentinel bit pattern; its own ``M x N`` region starts as NaN.  After
a call every element of the view must be finite and inside the bars, and every
other element of the enclosing tensor bit-identical to the sentinel (compared
as int32): a read of padding that reaches a valid output, or a write outside
``C``'s ``M x N``, shows in the values.  Nothing is made to fault.

Data, per case (all drawn on the CPU from a seed of the shape):
  a    randn operands with column k of A scaled by 2^e[k], |e[k]| <= 20, and
       column k of B by 2^-e[k]: magnitudes differ by 2^40 inside every
       fragment while every product, and the reference, stays O(1) / O(sqrt K)
  b    B has exactly one nonzero +-2^j per row, at k = sel_k(row); A is
       full-mantissa randn.  Each output is one exact product.  ``bs``: the
       roles swapped (A selects)
  c    the same one nonzero per row, drawn randn.  ``cs``: roles swapped

Bars, elementwise against float64 torch on the same fp32 values, u = 2^-24,
S = |A| |B|^T + |bias| in float64:
  a        |C - ref| <= 2 max(K, 16) u S: any summation order of K rounded
           products obeys ~K u S; the factor 2 covers the split form's dropped
           cross terms (<= 2.01 u per product by abcd_x6.h's split widths) and
           the epilogue roundings.  Derived, loose by ~sqrt K: the structural
           check.
  a, x6 and side routes
           max-norm relative error <= 4 e32 + 1e-7, e32 the error of torch's
           fp32 product of the same operands against the same reference
           (tests/test_gpu_x6.py's margin)
  b, bs    C == ref bit for bit on every route
  c, cs    |C - ref| <= 8 u |ref|: 2.01 u of dropped terms + one final rounding
           + the partial sums' roundings is 3-4 u; the bar is twice that.  (A
           sequential fp32 emulation of the six-term product gives 1.6 u at
           worst over 2^20 products, and a median of 23 u with one of the
           u-sized cross terms missing.)
  tanh     every bar gains 4 max |tanh_fp32(z) - tanh(z)| measured on the
           float64 pre-activations z (tanh is 1-Lipschitz: the GEMM bar carries
           through unchanged)
"""
import functools
import glob
import json
import os
import sys
from collections import OrderedDict

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import edge_cases as E  # noqa: E402

U = 2.0 ** -24
SENTINEL = 0x4B5A3C69            # a finite fp32 (1.43e7) no product of these cases gives
MARGIN = 64                      # floats before and after every view (256 B: keeps 16-B alignment)
EXTRA_ROWS = 2                   # NaN rows past the valid ones
C_BAR = 8 * U
KINDS = ("a", "b", "bs", "c", "cs")
EINVAL = 1000


# ----------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------
def _nt(name, M, N, K, route, lda=None, ldb=None, ldc=None, a_off=0, c_off=0, bias=True, ws="std", side=False,
        x6=False, rc=0):
    return dict(name=name, M=M, N=N, K=K, lda=lda or K, ldb=ldb or K, ldc=ldc or N, a_off=a_off, c_off=c_off,
                bias=bias, ws=ws, side=side, x6=x6 or side, route=route, rc=rc)


def _nt_cases():
    c = []
    FM, FN = 15233, 129   # 120 x 2 tiles of 128 x 128: the smallest frame-parallel M at N in 129..256;
    # its x6r8 grid has one frame range holding a single row and eight empty ones
    for K in (16, 128, 160):
        c.append(_nt(f"x6r8_5_k{K}_ldc129", FM, FN, K, "x6r8<5,128>", lda=K + 4, x6=True))
        c.append(_nt(f"x6r8_5_k{K}_ldc132", FM, FN, K, "x6r8<5,128>", lda=K + 4, ldb=K + 4, ldc=132, x6=True))
    c.append(_nt("x6r8_5_t16_k144", FM, FN, 144, "x6r8<5,128,t16>", lda=148, c_off=1, x6=True))
    for K in (176, 240, 256):
        c.append(_nt(f"x6r8_8_k{K}", FM, FN, K, "x6r8<8,64>", x6=True))
    for K in (272, 304):
        c.append(_nt(f"x6f_k{K}_ldc129", FM, FN, K, "x6f", x6=True))
        c.append(_nt(f"x6f_k{K}_ldc132", FM, FN, K, "x6f", lda=K + 4, ldc=132, x6=True))
    c.append(_nt("ks_under_threshold", FM - 1, FN, 144, "ks z=1", lda=148, c_off=1))
    c.append(_nt("ks_z1", 33, 70, 48, "ks z=1"))
    c.append(_nt("ks_z2_vec", 32, 64, 256, "ks z=2 vec"))
    c.append(_nt("ks_z8_zg4", 32, 64, 1024, "ks z=8 zg4"))
    c.append(_nt("ks_z16_zg16", 32, 64, 2048, "ks z=16 zg16"))
    c.append(_nt("ks_scalar", 33, 71, 1024, "ks z=8 scalar"))
    c.append(_nt("ks_z16_zg4_big_output", 256, 512, 4096, "ks z=16 zg4"))
    c.append(_nt("ks_scratch_clamps_z3", 32, 64, 2048, "ks z=3 vec", ws=3 * 32 * 64))
    c.append(_nt("ks_ws_null", 32, 64, 2048, "ks z=1", ws=None))
    c.append(_nt("pack_k45", 33, 70, 45, "ks z=1", lda=45, ldb=45))
    c.append(_nt("pack_lda49_offset", 33, 70, 48, "ks z=1", lda=49, a_off=1))
    c.append(_nt("pack_ws_one_short", 33, 70, 45, None, lda=45, ldb=45, ws=(33 + 70) * 48 - 1, rc=EINVAL))
    # side mode (the training step's mode beside a persistent recurrent kernel)
    c.append(_nt("side_tn44", FM, FN, 144, "tn<4,4,kc>", side=True))
    c.append(_nt("side_tn48", 10113, 257, 48, "tn<4,8,kc>", side=True))
    return OrderedDict((x["name"], x) for x in c)


def _tn(name, M, N, K, route, lda=None, ldb=None, ldc=None, ws="std", side=False, x6=False):
    return dict(name=name, M=M, N=N, K=K, lda=lda or M, ldb=ldb or N, ldc=ldc or N, ws=ws, side=side, x6=x6 or side,
                route=route, bias=False, rc=0)


def _tn_cases():
    c = [
        _tn("x6t_ldc161", 129, 161, 4099, "x6t z=9 scalar", lda=132, ldb=164, x6=True),
        _tn("x6t_ldc164", 129, 161, 4099, "x6t z=9 scalar", lda=132, ldb=164, ldc=164, x6=True),
        _tn("x6t_ws_null", 129, 161, 4099, "x6t", lda=132, ldb=164, ws=None, x6=True),
        _tn("x6s45", 129, 130, 4099, "x6s<4,5> z=9 scalar", lda=132, ldb=132, x6=True),
        _tn("ks_split_not_tn_ok", 129, 161, 4099, "ks z=29 scalar", lda=129, ldb=164),
        _tn("big", 1795, 1923, 48, "big"),
        _tn("side_x6s45_one", 129, 130, 4099, "x6s<4,5,one> z=9 scalar", lda=132, ldb=132, side=True),
        _tn("side_x6s54_one", 130, 200, 4099, "x6s<5,4,one> z=9 zg4", lda=132, side=True),
        _tn("side_x6s44_one", 200, 200, 4099, "x6s<4,4,one> z=9 zg4", side=True),
        # 8 tiles of 32 x 64, 264 chunks: the default budget (1024 workgroups) gives Z = min(128, 264 / 8) = 33;
        # the side budget (256) caps it at 32, which 9 chunks per slab make 30
        _tn("ks_split_default_budget", 33, 200, 4224, "ks z=33 zg16"),
        _tn("side_ks_split_capped", 33, 200, 4224, "ks z=30 zg16", side=True),
    ]
    return OrderedDict((x["name"], x) for x in c)


def _lin(name, M, N, K, route, act, bias, ldx=None, ldw=None, ldy=None, x6=False):
    return dict(name=name, M=M, N=N, K=K, lda=ldx or K, ldb=ldw or K, ldc=ldy or N, a_off=0, c_off=0, bias=bias,
                act=act, ws="std", side=False, x6=x6, route=route, rc=0)


def _linear_cases():
    c = [
        _lin("tanh_x6r8_t16", 15233, 129, 144, "x6r8<5,128,t16>", 1, True, ldy=132, x6=True),
        _lin("tanh_x6r8_8", 15233, 129, 256, "x6r8<8,64>", 1, True, ldy=132, x6=True),
        _lin("none_padded_lds", 50, 7, 33, "ks z=1", 0, False, ldx=40, ldw=36, ldy=9),
        _lin("tanh_tiny", 3, 1, 9, "ks z=1", 1, True),
    ]
    return OrderedDict((x["name"], x) for x in c)


NT_CASES = _nt_cases()
TN_CASES = _tn_cases()
LINEAR_CASES = _linear_cases()

# abcd_linear_backward: (M, N, K); every leading dimension padded (ldx = K + 3, ldw = K + 1, ldy = N + 2,
# lddy = N + 1, lddx = K + 5).  (7553, 7, 385): dx = dy' W is 60 x 4 tiles of 128 x 128 with K = 16, the fp32-MFMA
# `big` kernel on one K-major operand; its dW reduces over 7553 >= 4096 rows (x6t).
BWD_SHAPES = OrderedDict([("m50n7k33", (50, 7, 33)), ("m3n1k9", (3, 1, 9)), ("m7553n7k385", (7553, 7, 385))])
BWD_WANTS = ("all", "dx", "dW", "db")
BWD_ROUTE = {("m7553n7k385", "dx"): "big", ("m7553n7k385", "dW"): "x6t z=15 scalar",
             ("m7553n7k385", "all"): "x6t z=15 scalar",   # the last product of the call
             ("m50n7k33", "dx"): "ks z=1", ("m50n7k33", "dW"): "ks z=1", ("m50n7k33", "all"): "ks z=1",
             ("m3n1k9", "dx"): "ks z=1", ("m3n1k9", "dW"): "ks z=1", ("m3n1k9", "all"): "ks z=1"}

# every route string the issue's tables name; the GPU run must see each in a passing case
ROUTES_EXPECTED = sorted({c["route"] for t in (NT_CASES, TN_CASES, LINEAR_CASES) for c in t.values() if c["route"]}
                         | set(BWD_ROUTE.values()))


# ----------------------------------------------------------------------------
# guarded buffers
# ----------------------------------------------------------------------------
class Guarded:
    """``view``: rows x cols at stride ld, ``off`` floats past a 16-B aligned
    point of ``flat``.  fill = "nan" (an operand) or "sentinel" (an output,
    whose view starts as NaN)."""

    def __init__(self, rows, cols, ld, device, fill="nan", off=0):
        assert ld >= cols
        self.n = MARGIN + off + (rows + EXTRA_ROWS) * ld + MARGIN
        self.start = MARGIN + off
        if fill == "nan":
            self.flat = torch.full((self.n,), float("nan"), device=device)
        else:
            self.flat = torch.full((self.n,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
        self.view = self.flat.as_strided((rows, cols), (ld, 1), self.start)
        if fill != "nan":
            self.view.fill_(float("nan"))

    def ptr(self):
        return self.flat.data_ptr() + 4 * self.start

    def guard_intact(self):
        """True when everything outside the view still holds the sentinel's bits."""
        c = self.flat.clone()
        c.as_strided(self.view.shape, self.view.stride(), self.start).view(torch.int32).fill_(SENTINEL)
        return bool((c.view(torch.int32) == SENTINEL).all())


def operand(x, ld, device, off=0):
    """A Guarded copy of the 2-D fp32 tensor x."""
    g = Guarded(x.shape[0], x.shape[1], ld, device, "nan", off)
    g.view.copy_(x)
    return g


# ----------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------
def sel_stride(R, K):
    """The step between adjacent rows' selected k: odd, coprime to K, about
    K / R for K > R (the R rows then spread over the whole depth) and 13
    otherwise: at least 13 apart, so adjacent rows sit in different 4-lane and
    8-lane groups, and 13 mod 32 beyond one chunk, so they also sit at
    different places of a 32-deep (and a 16-deep) chunk."""
    import math
    s = max(13, K // max(R, 1))
    s = s - s % 32 + 13 if s > 32 else s | 1   # 13 mod 32 beyond a chunk, odd below
    while math.gcd(s, K) != 1:               # odd from the start; a few steps of 2 at the most
        s += 2
    return s


def sel_k(R, K):
    """k[r] = (K - 1 - r s) mod K: row 0 selects the last valid k; every k is
    selected once R >= K."""
    if K == 0:
        return torch.zeros(R, dtype=torch.int64)
    return (K - 1 - torch.arange(R, dtype=torch.int64) * sel_stride(R, K)) % K


def _selection(R, K, g, pow2):
    x = torch.zeros(R, K)
    if K == 0:
        return x
    if pow2:
        v = torch.ldexp(torch.ones(R), torch.randint(-6, 7, (R,), generator=g).float())
        v = v * (torch.randint(0, 2, (R,), generator=g).float() * 2 - 1)
    else:
        v = torch.randn(R, generator=g)
    x[torch.arange(R), sel_k(R, K)] = v
    return x


def operands(kind, M, N, K, seed):
    """(A M x K, B N x K) fp32 on the CPU for data kind a / b / bs / c / cs."""
    g = torch.Generator().manual_seed(seed)
    if kind == "a":
        e = torch.randint(-20, 21, (K,), generator=g).float()
        return torch.ldexp(torch.randn(M, K, generator=g), e), torch.ldexp(torch.randn(N, K, generator=g), -e)
    pow2 = kind[0] == "b"
    if kind in ("b", "c"):
        return torch.randn(M, K, generator=g), _selection(N, K, g, pow2)
    return _selection(M, K, g, pow2), torch.randn(N, K, generator=g)


def case_seed(c, kind):
    return 1000003 * c["M"] + 1009 * c["N"] + 17 * c["K"] + KINDS.index(kind)


@functools.lru_cache(maxsize=4)
def case_data(table, name, kind):
    """dict(A, B, bias) on the CPU, shared and never modified.  A and B are
    M x K and N x K whatever the entry point (abcd_gemm_tn gets their
    transposes)."""
    c = {"nt": NT_CASES, "tn": TN_CASES, "linear": LINEAR_CASES}[table][name]
    A, B = operands(kind, c["M"], c["N"], c["K"], case_seed(c, kind))
    bias = None
    if c["bias"] and kind == "a":   # b / c: one exact product per output, nothing added
        bias = torch.randn(c["N"], generator=torch.Generator().manual_seed(case_seed(c, kind) + 7))
    return dict(A=A, B=B, bias=bias)


# ----------------------------------------------------------------------------
# references and bars (device-agnostic torch)
# ----------------------------------------------------------------------------
def reference(A, B, bias=None, unit=True):
    """dict(ref, S): the float64 product A B^T (+ bias) and, with ``unit``, its
    unit |A| |B|^T (+ |bias|) (data kind a's bar; None otherwise)."""
    A64, B64 = A.double(), B.double()
    ref = A64 @ B64.t()
    S = A64.abs() @ B64.abs().t() if unit else None
    if bias is not None:
        ref = ref + bias.double()
        S = S + bias.double().abs() if unit else None
    return dict(ref=ref, S=S)


def tanh_error(z64):
    """max |tanh_fp32(z) - tanh(z)| over the float64 pre-activations z."""
    if z64.numel() == 0:
        return 0.0
    return float((torch.tanh(z64.float()).double() - torch.tanh(z64)).abs().max())


def max_norm_err(C, ref):
    return float((C.double() - ref).abs().max() / ref.abs().max())


def check(kind, C, rf, K, act=0, e32=None):
    """dict of figures and ``fails``, the list of the checks C misses.  C is the
    M x N fp32 result; rf = reference(...); with act = 1 the reference is
    tanh(rf["ref"]).  e32: the max-norm error of torch's fp32 result of the same
    operands (the x6 / side bar); None: that bar is not applied."""
    out, fails = {}, []
    if not bool(torch.isfinite(C).all()):
        return dict(fails=["finite"], nonfinite=int((~torch.isfinite(C)).sum()))
    z, S = rf["ref"], rf["S"]
    ref = torch.tanh(z) if act == 1 else z
    slack = 4 * tanh_error(z) if act == 1 else 0.0
    err = (C.double() - ref).abs()
    out["tanh_slack"] = slack
    if kind == "a":
        bar = 2 * max(K, 16) * U * S + slack
        out["worst_of_bar"] = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
        if not bool((err <= bar).all()):
            fails.append("a")
        if e32 is not None and err.numel():
            out["e_maxnorm"], out["e32"] = max_norm_err(C, ref), e32
            if not out["e_maxnorm"] <= 4 * e32 + 1e-7:
                fails.append("maxnorm")
    elif kind in ("b", "bs"):
        if act == 1:
            out["worst_abs"] = float(err.max()) if err.numel() else 0.0
            if not bool((err <= slack).all()):
                fails.append("b")
        else:
            same = C.view(torch.int32) == ref.float().view(torch.int32)
            out["mismatches"] = int((~same).sum())
            if out["mismatches"]:
                fails.append("b")
    else:
        bar = C_BAR * z.abs() + slack
        nz = z != 0
        out["worst_u"] = float((err[nz] / z[nz].abs()).max() / U) if bool(nz.any()) and act == 0 else None
        if not bool((err <= bar).all()):
            fails.append("c")
    out["fails"] = fails
    return out


# ----------------------------------------------------------------------------
# abcd_linear_backward
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bwd_data(shape, act):
    """x M x K, W N x K, y M x N, dy M x N on the CPU.  With tanh y is a real
    forward output, tanh(x W^T) in fp32, and one entry in five is set to exactly
    +-1, whose gradient must be exactly 0."""
    M, N, K = BWD_SHAPES[shape]
    g = torch.Generator().manual_seed(31 * M + 7 * N + K + act)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    dy = torch.randn(M, N, generator=g)
    y = torch.tanh(x @ W.t()) if act == 1 else torch.randn(M, N, generator=g)
    if act == 1:
        ones = torch.rand(M, N, generator=g) < 0.2
        ones[0, 0] = True
        sign = torch.randint(0, 2, (M, N), generator=g).float() * 2 - 1
        y = torch.where(ones, sign, y)
    return dict(x=x, W=W, y=y, dy=dy)


def bwd_reference(x, W, y, dy, act):
    """float64 dx = dy' W, dW = dy'^T x, db = colsum(dy') and their units, built
    from |dy'|; dy' = dy (1 - y^2) for tanh."""
    d = dy.double()
    if act == 1:
        d = d * (1 - y.double() ** 2)
    a = d.abs()
    return dict(dyp=d, dx=d @ W.double(), S_dx=a @ W.double().abs(), dW=d.t() @ x.double(),
                S_dW=a.t() @ x.double().abs(), db=d.sum(0), S_db=a.sum(0))


def bwd_check(got, ref, M, N, K):
    """Bars as data (a): 2 max(depth, 16) u S, the depth N for dx and M for dW
    and db.  Returns (figures, fails)."""
    out, fails = {}, []
    for name, depth in (("dx", N), ("dW", M), ("db", M)):
        if got.get(name) is None:
            continue
        c = got[name]
        if not bool(torch.isfinite(c).all()):
            fails.append(name + ":finite")
            continue
        err, bar = (c.double() - ref[name]).abs(), 2 * max(depth, 16) * U * ref["S_" + name]
        out[name + "_worst_of_bar"] = float((err / bar.clamp_min(1e-300)).max())
        if not bool((err <= bar).all()):
            fails.append(name)
    return out, fails


# ----------------------------------------------------------------------------
# a bf16 emulation of the six-term product (abcd_x6.h), for the CPU test that
# the bars can fail
# ----------------------------------------------------------------------------
def split3(x):
    """x = x0 + x1 + x2 exactly, each piece a bf16 value held in fp32."""
    x0 = x.bfloat16().float()
    r = x - x0
    x1 = r.bfloat16().float()
    return x0, x1, (r - x1).bfloat16().float()


SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))   # (A piece, B piece), smallest first


def x6_emulated(A, B, drop=None, kmax=None):
    """A B^T by the six-term split product, each term's GEMM accumulated in
    float64 and the sum of the terms rounded once to fp32 (the honest form's
    error is the dropped cross terms plus one rounding).  drop: a term of SIX
    to leave out.  kmax: columns >= kmax are not read (a dropped tail)."""
    if kmax is not None:
        A, B = A[:, :kmax], B[:, :kmax]
    a, b = split3(A), split3(B)
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float64)
    for i, j in SIX:
        if (i, j) != drop:
            acc += a[i].double() @ b[j].double().t()
    return acc.float()


# ----------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------
def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as edge_cases.dump_observed)."""
    E.dump_observed("gemm_" + name, rows)


SECTIONS = OrderedDict([("lstm_wgrad", ("lstm_wgrad",)), ("offset_head", ("offset_head_fwd", "offset_head_bwd")),
                        ("tn_batch", ("tn_batch",)), ("colsum_batch", ("colsum_batch",))])


def _walk(x, key=""):
    """Every (key, value) leaf of the nested figures of one dumped row."""
    if isinstance(x, dict):
        for k, v in x.items():
            yield from _walk(v, k)
    elif isinstance(x, (int, float)) and not isinstance(x, bool):
        yield key, x


def section_worst(rows):
    """The worst figures of the rows tests/test_gpu_wgrad_offset.py dumped for one group."""
    out = dict(worst_of_bar=None, worst_u=None, maxnorm_worst_of_e32=None, mismatches=0, bce_dlog_worst_abs=None,
               failed_checks=sum(len(k.get("fails", [])) for r in rows for k in r.get("kinds", {}).values())
               + sum(len(r.get("fails", [])) for r in rows))
    up = lambda k, v: out.__setitem__(k, v if out[k] is None else max(out[k], v))

    def visit(d):
        if isinstance(d, dict):
            if d.get("e32") and d.get("e_maxnorm") is not None:
                up("maxnorm_worst_of_e32", d["e_maxnorm"] / d["e32"])
            for v in d.values():
                visit(v)
    for r in rows:
        fig = r.get("kinds", r.get("figures", {}))
        visit(fig)
        for k, v in _walk(fig):
            if k.endswith("worst_of_bar"):
                up("worst_of_bar", v)
            elif k.endswith("worst_u"):
                up("worst_u", v)
            elif k.endswith("mismatches"):
                out["mismatches"] += int(v)
            elif k in ("bce_worst", "dlog_worst"):
                up("bce_dlog_worst_abs", v)
    return out


def assemble(src, parent_commit, date):
    """Build profiles/gemm_errors.json from the files a GPU run of
    tests/test_gpu_gemm_routes.py and tests/test_gpu_wgrad_offset.py left in
    ``src`` (ABCD_PARITY_DUMP=<src>)."""
    rows, extra = [], OrderedDict((s, []) for s in SECTIONS)
    for path in sorted(glob.glob(os.path.join(src, "gemm_*.json"))):
        with open(path) as f:
            r = json.load(f)
        sec = [s for s, entries in SECTIONS.items() if r.get("entry") in entries]
        (extra[sec[0]] if sec else rows).append(r)
    routes = sorted({r["route"] for r in rows if r.get("route")})
    worst = dict(
        a_worst_of_bar=max((k["worst_of_bar"] for r in rows for k in r.get("kinds", {}).values()
                            if k.get("worst_of_bar") is not None), default=None),
        c_worst_u=max((k["worst_u"] for r in rows for k in r.get("kinds", {}).values()
                       if k.get("worst_u") is not None), default=None),
        maxnorm_worst_of_e32=max((k["e_maxnorm"] / k["e32"] for r in rows for k in r.get("kinds", {}).values()
                                  if k.get("e32")), default=None),
        b_mismatches=sum(k.get("mismatches", 0) for r in rows for k in r.get("kinds", {}).values()))
    doc = dict(what="figures observed by tests/test_gpu_gemm_routes.py (cases, worst, routes_seen) and "
                    "tests/test_gpu_wgrad_offset.py (the sections lstm_wgrad, offset_head, tn_batch, colsum_batch, each "
                    "with its own worst) in one run (ABCD_PARITY_DUMP) on one MI355X; data kinds "
                    "and bars: tests/gemm_cases.py.  worst_of_bar: max |C - ref| / (2 max(K, 16) u S); worst_u: max "
                    "|C - ref| / (u |ref|) on single-product data (bar 8); e_maxnorm / e32: max-norm relative errors "
                    "of the library and of torch's fp32 GEMM (bar 4 e32 + 1e-7); mismatches: outputs of the "
                    "power-of-two selection data that differ from the exact product in any bit (bar 0)",
               date=date, parent_commit=parent_commit, worst=worst, routes_seen=routes,
               routes_expected_missing=[r for r in ROUTES_EXPECTED if r not in routes], cases=rows)
    for s, rs in extra.items():   # tests/test_gpu_wgrad_offset.py (tables and bars: tests/wgrad_cases.py)
        # routes_seen: dispatch records / route strings the tests read back and asserted (colsum_batch has one
        # form and records none)
        doc[s] = dict(worst=section_worst(rs), routes_seen=sorted({r["route"] for r in rs if r.get("route")}), cases=rs)
    out = os.path.join(REPO, "profiles", "gemm_errors.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":  # python tests/gemm_cases.py <dump directory> <parent commit> <date>
    print(assemble(sys.argv[1], sys.argv[2], sys.argv[3]))
