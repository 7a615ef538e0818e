"""Cases, buffers, data, float64 references and bars of the tests of the GEMM
layer's kernels that ``gemm()`` does not dispatch: ``gemm_wg3b`` / ``gemm_wg2``
(``abcd_lstm_wgrad``), the fused offset head (``gemm_x6r8_kernel<8,64,2,16,1>``
and ``<...,2>`` with ``dec_offset_logit``, through ``abcd_debug_offset_head_fwd``
/ ``_bwd``), ``gemm_tn_batch`` and ``colsum_batch`` (``abcd_debug_gemm_tn_batch``
/ ``abcd_debug_colsum_batch``).  No GPU code: tests/test_wgrad_cases_cpu.py runs
the tables on torch's CPU fp32, tests/test_gpu_wgrad_offset.py on the library.

Buffers, data kinds (a, b, bs, c, cs) and bars are those of tests/gemm_cases.py
(``Guarded``, ``operands``, ``reference``, ``check``); what is new is derived
here:

  lstm_wgrad   the frames k are the reduction depth: "A" is dG^T (4H x K), "B"
               is [X | Hprev]^T ((F + H) x K).  The bias is the product of dG^T
               with the ones column: a full sum (bar a: 2 max(K, 16) u
               colsum |dG|) but where dG itself selects (bs, cs: one product).
  logit        logit = tanh(z) . w2 + b2.  An error e[m, n] <= barZ[m, n] of Zo
               reaches the logit as sum_n e |w2[n]|; the dot product of N fp32
               terms (16 per slice in a tree, the slices in order) and b2 add
               at most N u (sum |Zo| |w2| + |b2|); the factor 2 as in bar a.
  bce, dlog    fp32 __expf / log1pf of an O(1) logit against float64 of the
               SAME fp32 logit: 1e-6 absolute (an estimate; the worst is kept).
  dZo          dZo = s dlog w2 (1 - Zo^2): two products, one square and one
               difference, each rounded once, contracted or not: <= 4 roundings
               of 2 u relative to the largest intermediate |s dlog w2| (1 - Zo^2
               <= 1); the bar is 8 u |s dlog w2|.  Zo = +-1 gives 0 exactly.
  DHO          against the float64 product of the dZo THE KERNEL STORED with
               W1oT: the GEMM's bars apply unchanged.
  tn_batch     fp32 MFMA: the bars of gemm_cases without the x6 margin.  The
               beta = 1 job adds C0: S gains |C0|, and the single-product bar
               becomes 8 u (|product| + |C0|) (one more rounding, of the sum).
  colsum       2 max(nrows, 16) u (|w|^T |Z| + beta |out0|).
"""
import functools
import math
from collections import OrderedDict

import torch

import gemm_cases as G

U = G.U
cdiv = lambda a, b: -(-a // b)
rup16 = lambda x: (x + 15) // 16 * 16


# ----------------------------------------------------------------------------
# 1. abcd_lstm_wgrad: the launch arithmetic of wgrad_wg2_launch, restated
# ----------------------------------------------------------------------------
def wgrad_workspace_floats(nd, F, H, K):
    """(floats the call needs, floats of the packed [X | 1 | 0] in front)."""
    xp = (K * rup16(F + 1) + 63) // 64 * 64
    M = 4 * H
    return xp + max(16 * nd * M * (rup16(F + 1) + H), M * max(F, H) * 64), xp


def wg_launch(form, nd, K, F=129, H=256):
    """dict(tw, Z, kq, kps, last, chunks_last) of the gemm_wg3b / gemm_wg2
    launch at the exact workspace: tw workgroups per (direction, K range), Z
    ranges of kps frames (a multiple of kq), the last of ``last`` frames in
    ``chunks_last`` 32-frame chunks."""
    M, NT = 4 * H, rup16(F + 1) + H
    need, xp = wgrad_workspace_floats(nd, F, H, K)
    tw = 2 * cdiv(M, 256) if form == "wg3b" else cdiv(M, 128)
    Z = max(1, 256 // (nd * tw))
    while (nd * tw * Z) % 8:
        Z += 1
    Z = min(Z, (need - xp) // (nd * M * NT))
    kq = 64 if form == "wg3b" else 32
    kps = cdiv(cdiv(K, Z), kq) * kq
    Z = cdiv(K, kps)
    last = K - (Z - 1) * kps
    return dict(tw=tw, Z=Z, kq=kq, kps=kps, last=last, chunks_last=cdiv(last, 32))


# what the issue's table claims of the resident shape: (form, nd, K) -> the fields that must hold
WG_CLAIMS = {
    ("wg3b", 1, 33): dict(Z=1, last=33, chunks_last=2), ("wg3b", 2, 33): dict(Z=1, last=33, chunks_last=2),
    ("wg2", 1, 33): dict(Z=2, last=1), ("wg2", 2, 33): dict(Z=2, last=1),
    ("wg3b", 1, 65): dict(Z=2, last=1), ("wg3b", 2, 65): dict(Z=2, last=1),
    ("wg3b", 1, 97): dict(Z=2, last=33, chunks_last=2), ("wg3b", 2, 97): dict(Z=2, last=33, chunks_last=2),
    ("wg3b", 1, 193): dict(Z=4, last=1), ("wg3b", 2, 193): dict(Z=4, last=1),
    ("wg2", 1, 193): dict(Z=7, last=1), ("wg2", 2, 193): dict(Z=7, last=1),
    ("wg3b", 2, 1024): dict(Z=16, kps=64, last=64), ("wg2", 2, 1024): dict(Z=16, kps=64, last=64),
    ("wg3b", 2, 1025): dict(kps=128, Z=9, last=1), ("wg3b", 1, 1025): dict(Z=17),
    ("wg2", 2, 1025): dict(kps=96, Z=11, last=65),
    ("wg3b", 2, 2049): dict(kps=192, Z=11, last=129, chunks_last=5),
    ("wg3b", 1, 2049): dict(kps=128, Z=17, last=1),
}
WG_KS = (1, 31, 32, 33, 64, 65, 97, 193, 1024, 1025, 2049)


def _wg(name, form, nd, K, F=129, H=256, ldx=None, x_off=0, dg_off=(0, 0), hp_off=(0, 0), env=None, bhh_null=False):
    Fp = rup16(F + 1)
    e = dict(env or {})
    if form != "split":
        e["ABCD_WG3"] = "1" if form == "wg3b" else "0"
        route = f"gemm_{form}<{Fp},{H}> x{nd}"
    else:
        route = "gemm split (x6s/x6t)"
    return dict(name=name, form=form, nd=nd, K=K, F=F, H=H, ldx=ldx or F, x_off=x_off, dg_off=dg_off, hp_off=hp_off,
                env=e, bhh_null=bhh_null, route=route)


def _wg_cases():
    c = []
    for form in ("wg3b", "wg2"):
        for nd in (1, 2):
            for K in WG_KS:
                c.append(_wg(f"{form}_nd{nd}_k{K}", form, nd, K))
        c.append(_wg(f"{form}_f128", form, 2, 193, F=128))     # the ones column is column 128
        c.append(_wg(f"{form}_f143", form, 2, 193, F=143))     # ... the last of Fp
        c.append(_wg(f"{form}_ldx136", form, 2, 193, ldx=136))
        c.append(_wg(f"{form}_x_off1", form, 2, 193, x_off=1))  # pack2d takes both: the route stays wg
        c.append(_wg(f"{form}_bhh_null", form, 2, 193, bhh_null=True))
    for K in (193, 4099):
        c.append(_wg(f"split_wg2off_k{K}", "split", 2, K, env={"ABCD_WG2": "0"}))
        c.append(_wg(f"split_dg1_off_k{K}", "split", 2, K, dg_off=(0, 1)))
        c.append(_wg(f"split_hp0_off_k{K}", "split", 2, K, hp_off=(1, 0)))
        c.append(_wg(f"split_f127_k{K}", "split", 2, K, F=127))
        c.append(_wg(f"split_f144_k{K}", "split", 2, K, F=144))
        c.append(_wg(f"split_h252_k{K}", "split", 2, K, H=252))
        c.append(_wg(f"split_h260_k{K}", "split", 2, K, H=260))
        c.append(_wg(f"split_h48_f33_k{K}", "split", 2, K, F=33, H=48))
        c.append(_wg(f"split_h24_f20_nd1_k{K}", "split", 1, K, F=20, H=24))
    return OrderedDict((x["name"], x) for x in c)


WG_CASES = _wg_cases()


def wg_seed(c, kind, d):
    return 1000003 * c["K"] + 1009 * c["F"] + 17 * c["H"] + 5 * G.KINDS.index(kind) + d


@functools.lru_cache(maxsize=4)
def wg_data(name, kind):
    """dict(dG [nd] K x 4H, X K x F, Hp [nd] K x H) on the CPU, shared and never
    modified: one G.operands draw whose A is the directions' dG^T stacked (nd 4H
    x K) and whose B is [X | Hprev[0] | Hprev[1]]^T, so that the directions, which
    share X, share the frame scales 2^e[k] of kind a too."""
    c = WG_CASES[name]
    nd, F, H, K = c["nd"], c["F"], c["H"], c["K"]
    A, B = G.operands(kind, nd * 4 * H, F + nd * H, K, wg_seed(c, kind, 0))
    return dict(dG=[A[4 * H * d:4 * H * (d + 1)].t().contiguous() for d in range(nd)], X=B[:F].t().contiguous(),
                Hp=[B[F + H * d:F + H * (d + 1)].t().contiguous() for d in range(nd)])


def wg_buffers(c, data, device):
    """Guarded operands and outputs of one call.  dG / X / Hprev: views inside
    NaN (margins, EXTRA_ROWS rows past K, columns F .. ldx of X); w_ih (row pitch
    F), b_ih, b_hh, w_hh: NaN views inside the sentinel."""
    nd, F, H = c["nd"], c["F"], c["H"]
    M = 4 * H
    b = dict(dG=[G.operand(data["dG"][d], M, device, c["dg_off"][d]) for d in range(nd)],
             X=G.operand(data["X"], c["ldx"], device, c["x_off"]),
             Hp=[G.operand(data["Hp"][d], H, device, c["hp_off"][d]) for d in range(nd)],
             w_ih=[G.Guarded(M, F, F, device, "sentinel") for _ in range(nd)],
             b_ih=[G.Guarded(1, M, M, device, "sentinel") for _ in range(nd)],
             b_hh=[G.Guarded(1, M, M, device, "sentinel") for _ in range(nd)],
             w_hh=[G.Guarded(M, H, H, device, "sentinel") for _ in range(nd)])
    return b


WG_OUTS = ("w_ih", "b_ih", "b_hh", "w_hh")


def bias_kind(kind):
    """The bias is a full sum over the frames unless dG itself selects."""
    return kind if kind in ("bs", "cs") else "a"


def wg_check(c, kind, data, bufs, maxnorm=("w_ih", "b_ih", "w_hh")):
    """(figures, fails) of one call's outputs against float64 of ``data`` (on
    the outputs' device).  maxnorm: the tensors that carry the 4 e32 + 1e-7 bar
    on data kind a (the wg forms: all; a fallback: those whose route is x6)."""
    fig, fails = {}, []
    K, dev = c["K"], bufs["w_ih"][0].flat.device
    X = data["X"].to(dev)
    ones = torch.ones(1, K, device=dev)
    for d in range(c["nd"]):
        A = data["dG"][d].to(dev).t()
        Hp = data["Hp"][d].to(dev)
        for name in WG_OUTS:
            g = bufs[name][d]
            tag = f"{name}{d}"
            if not g.guard_intact():
                fails.append(tag + ":guard")
            if name == "b_hh":
                if c["bhh_null"]:
                    if not bool(torch.isnan(g.view).all()):
                        fails.append(tag + ":written though NULL")
                elif not torch.equal(g.view, bufs["b_ih"][d].view):
                    fails.append(tag + ":differs from b_ih")
                continue
            B = {"w_ih": X.t(), "w_hh": Hp.t(), "b_ih": ones}[name]
            kd = bias_kind(kind) if name == "b_ih" else kind
            rf = G.reference(A, B, None, unit=kd == "a")
            C = g.view.t().contiguous() if name == "b_ih" else g.view.contiguous()
            e32 = None
            if kd == "a" and kind == "a" and name in maxnorm:
                e32 = G.max_norm_err(A @ B.t(), rf["ref"])
            f = G.check(kd, C, rf, K, 0, e32)
            fails += [f"{tag}:{x}" for x in f.pop("fails")]
            fig[tag] = f
    return fig, fails


def wg_cpu_kernel(c, bufs, ones_col=None, frames=None):
    """torch's CPU fp32 in the library's place (frames: only the first ``frames``
    are summed; ones_col: where the bias is taken from the packed [X | 1 | 0],
    default F) -- through the same views, so the buffer checks run too."""
    F, K = c["F"], c["K"] if frames is None else frames
    Xp = torch.zeros(c["K"], rup16(F + 1))
    Xp[:, :F] = bufs["X"].view
    Xp[:, F] = 1.0
    for d in range(c["nd"]):
        dG = bufs["dG"][d].view[:K]
        bufs["w_ih"][d].view.copy_(dG.t() @ Xp[:K, :F])
        bias = dG.t() @ Xp[:K, F if ones_col is None else ones_col]
        bufs["b_ih"][d].view.copy_(bias[None])
        if not c["bhh_null"]:
            bufs["b_hh"][d].view.copy_(bias[None])
        bufs["w_hh"][d].view.copy_(dG.t() @ bufs["Hp"][d].view[:K])


# ----------------------------------------------------------------------------
# 2. the fused offset head: X6r8Grid<8, 64, 2>, restated
# ----------------------------------------------------------------------------
def x6r8_grid(M, N, BN=64, MR=2):
    """dict(nslices, nparts, grid, rows_per, used, last, passes): ``used`` row
    ranges hold rows, the last of them ``last``; ``passes`` turns of a
    workgroup's block loop (8 waves x 16 MR rows a turn) over a full range, and
    ``waves2`` waves that enter the last turn."""
    nslices = cdiv(N, BN)
    step = 8 // math.gcd(nslices, 8)
    nparts = max(step, (256 // nslices) // step * step)
    rows_per = cdiv(cdiv(M, nparts), 16 * MR) * 16 * MR
    used = cdiv(M, rows_per)
    first = min(M, rows_per)
    passes = cdiv(first, 8 * 16 * MR)
    waves_last = cdiv(first - (passes - 1) * 8 * 16 * MR, 16 * MR)
    return dict(nslices=nslices, nparts=nparts, grid=nslices * nparts, rows_per=rows_per, used=used,
                last=M - (used - 1) * rows_per, passes=passes, waves_last=waves_last)


GRID_CLAIMS = {
    (65, 68): dict(nslices=2, used=3, last=1), (65, 192): dict(nslices=3, grid=240, used=3, last=1),
    (65, 320): dict(nslices=5, grid=240, used=3, last=1), (65, 1024): dict(nslices=16, used=3, last=1),
    (65, 16): dict(nslices=1, used=3, last=1), (65, 256): dict(nslices=4, used=3, last=1),
    (16385, 256): dict(rows_per=288, passes=2, waves_last=1, last=257),
    (23041, 192): dict(rows_per=320, passes=2, last=1),
    (4097, 1024): dict(rows_per=288, passes=2, waves_last=1),
}
OFF_NS = (16, 64, 68, 80, 128, 192, 256, 320, 1024)
OFF_BIG = ((16385, 256), (23041, 192), (4097, 1024))   # (M, N): a second turn of the block loop


def _off(M, N, K, hs_off=0, tgt=True):
    return dict(name=f"m{M}_n{N}_k{K}" + ("_hsoff" if hs_off else "") + ("" if tgt else "_notgt"), M=M, N=N, K=K,
                hs_off=hs_off, tgt=tgt)


def _off_fwd_cases():
    c = [_off(M, N, 256) for N in OFF_NS for M in (1, 65)]
    c += [_off(M, 128, K) for K in (64, 8) for M in (1, 65)]
    c += [_off(M, N, 256) for M, N in OFF_BIG]
    c.append(_off(65, 80, 256, tgt=False))
    return OrderedDict((x["name"], x) for x in c)


def _off_bwd_cases():
    c = [_off(M, N, 256) for N in OFF_NS for M in (1, 65)]
    c += [_off(M, 256, 80) for M in (1, 65)]          # K chunks past Hm
    c += [_off(M, N, 256) for M, N in OFF_BIG]
    return OrderedDict((x["name"], x) for x in c)


OFF_FWD_CASES = _off_fwd_cases()
OFF_BWD_CASES = _off_bwd_cases()
OFF_FWD_DECLINES = OrderedDict((x["name"], x) for x in
                               (_off(65, 128, 264), _off(65, 128, 20), _off(65, 128, 256, hs_off=1), _off(65, 66, 256)))
OFF_BWD_DECLINES = OrderedDict((x["name"], x) for x in
                               (_off(65, 128, 264), _off(65, 128, 20), _off(65, 128, 256, hs_off=1), _off(65, 66, 256)))
BWD_KINDS = ("a", "b", "bs")


def off_seed(c, kind):
    return 1000003 * c["M"] + 1009 * c["N"] + 17 * c["K"] + G.KINDS.index(kind)


@functools.lru_cache(maxsize=2)
def off_fwd_data(name, kind):
    """Hs M x K, W1o N x K (G.operands), b1o (randn on kind a, else 0: one
    exact product per output), w2 = randn / sqrt N, b2, 0/1 targets."""
    c = {**OFF_FWD_CASES, **OFF_FWD_DECLINES}[name]
    M, N, K = c["M"], c["N"], c["K"]
    Hs, W1o = G.operands(kind, M, N, K, off_seed(c, kind))
    g = torch.Generator().manual_seed(off_seed(c, kind) + 7)
    b1o = torch.randn(N, generator=g) if kind == "a" else torch.zeros(N)
    return dict(Hs=Hs, W1o=W1o, b1o=b1o, w2=torch.randn(N, generator=g) / N ** 0.5, b2=torch.randn(1, generator=g),
                tgt=torch.randint(0, 2, (M,), generator=g).float())


def off_fwd_buffers(c, d, device):
    M, N, K = c["M"], c["N"], c["K"]
    nsl = cdiv(N, 64)
    vec = lambda x: G.operand(x[None, :], x.numel(), device)
    out = lambda r, n: G.Guarded(r, n, n, device, "sentinel")
    return dict(Hs=G.operand(d["Hs"], K + 4, device, c["hs_off"]), W1o=G.operand(d["W1o"], K, device),
                b1o=vec(d["b1o"]), w2=vec(d["w2"]), b2=vec(d["b2"]), tgt=vec(d["tgt"]), Zo=out(M, N), part=out(M, nsl),
                logit=out(1, M), dlog_raw=out(1, M), bce=out(1, M))


def zo_bar(kind, rf, K):
    """The elementwise bar G.check puts on tanh(z): the kind's GEMM bar plus
    the tanh slack."""
    slack = 4 * G.tanh_error(rf["ref"])
    if kind == "a":
        return 2 * max(K, 16) * U * rf["S"] + slack
    if kind in ("b", "bs"):
        return torch.full_like(rf["ref"], slack)
    return G.C_BAR * rf["ref"].abs() + slack


BCE_TOL = 1e-6


def off_fwd_check(c, kind, d, bufs):
    """(figures, fails): Zo by G.check(act = 1) with the x6 max-norm bar, the
    logit's derived bar, part (finite; its row sums in slice order + b2 are the
    logit bit for bit), bce / dlog_raw at BCE_TOL, every guard."""
    fig, fails = {}, []
    M, N, K = c["M"], c["N"], c["K"]
    dev = bufs["Zo"].flat.device
    Hs, W1o, b1o, w2, b2 = (d[k].to(dev) for k in ("Hs", "W1o", "b1o", "w2", "b2"))
    for k in ("Zo", "part", "logit", "dlog_raw", "bce"):
        if not bufs[k].guard_intact():
            fails.append(k + ":guard")
    rf = G.reference(Hs, W1o, b1o, unit=True)
    Zref = torch.tanh(rf["ref"])
    e32 = G.max_norm_err(torch.tanh(Hs @ W1o.t() + b1o), Zref) if kind == "a" else None
    f = G.check(kind, bufs["Zo"].view.contiguous(), rf, K, 1, e32)
    fails += ["Zo:" + x for x in f.pop("fails")]
    fig["Zo"] = f
    part, logit = bufs["part"].view, bufs["logit"].view[0]
    if not bool(torch.isfinite(part).all() and torch.isfinite(logit).all()):
        return fig, fails + ["part/logit:finite"]
    s = torch.zeros(M, device=dev)
    for k in range(part.shape[1]):
        s = s + part[:, k]
    fig["logit_from_part_mismatches"] = int((~((s + b2) .view(torch.int32) == logit.view(torch.int32))).sum())
    if fig["logit_from_part_mismatches"]:
        fails.append("logit:not the partials' sum")
    w64 = w2.double().abs()
    lref = Zref @ w2.double() + b2.double()
    lbar = zo_bar(kind, rf, K) @ w64 + 2 * max(N, 16) * U * (Zref.abs() @ w64 + b2.double().abs())
    lerr = (logit.double() - lref).abs()
    fig["logit_worst_of_bar"] = float((lerr / lbar).max())
    if not bool((lerr <= lbar).all()):
        fails.append("logit:bar")
    x = logit.double()
    if c["tgt"]:
        y = d["tgt"].to(dev).double()
        bce = x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))
        dl = torch.sigmoid(x) - y
        fig["bce_worst"] = float((bufs["bce"].view[0].double() - bce).abs().max())
        fig["dlog_worst"] = float((bufs["dlog_raw"].view[0].double() - dl).abs().max())
        if not (fig["bce_worst"] <= BCE_TOL and fig["dlog_worst"] <= BCE_TOL):   # NaN fails too
            fails.append("bce/dlog:tolerance")
    elif not bool(torch.isnan(bufs["bce"].view).all() and torch.isnan(bufs["dlog_raw"].view).all()):
        fails.append("bce/dlog:written without targets")
    return fig, fails


def off_fwd_cpu_kernel(c, bufs, x6=False, skip_slice=None):
    """torch's CPU fp32 (or the six-term emulation) in the kernel's place;
    skip_slice: that slice's partial is left out of the logit."""
    M, N, K = c["M"], c["N"], c["K"]
    Hs, W1o = bufs["Hs"].view, bufs["W1o"].view
    z = G.x6_emulated(Hs, W1o) if x6 else Hs @ W1o.t()
    Zo = torch.tanh(z + bufs["b1o"].view)
    bufs["Zo"].view.copy_(Zo)
    zw = Zo * bufs["w2"].view
    nsl = cdiv(N, 64)
    for k in range(nsl):
        bufs["part"].view[:, k] = zw[:, 64 * k:64 * k + 64].sum(1)
    s = torch.zeros(M)
    for k in range(nsl):
        if k != skip_slice:
            s = s + bufs["part"].view[:, k]
    x = s + bufs["b2"].view[0]
    bufs["logit"].view[0] = x
    if c["tgt"]:
        y = bufs["tgt"].view[0]
        bufs["bce"].view[0] = x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))
        bufs["dlog_raw"].view[0] = torch.sigmoid(x) - y


@functools.lru_cache(maxsize=2)
def off_bwd_data(name, kind):
    """Zo M x K in [-1, 1] with one entry in ten exactly +-1, W1oT N x K, w2
    (K), dlog_raw (M), s.  a: w2[k] carries 2^e[k] and column k of W1oT 2^-e[k]
    (dZo's column k is then scaled by 2^e[k], as G.operands scales A).  b: W1oT
    selects (+-2^j).  bs: Zo is +-1 everywhere but at one k per row, so dZo
    selects."""
    c = {**OFF_BWD_CASES, **OFF_BWD_DECLINES}[name]
    M, N, K = c["M"], c["N"], c["K"]
    g = torch.Generator().manual_seed(off_seed(c, kind) + 13)
    Zo = torch.tanh(torch.randn(M, K, generator=g))
    sign = torch.randint(0, 2, (M, K), generator=g).float() * 2 - 1
    w2 = torch.randn(K, generator=g)
    if kind == "bs":
        keep = torch.zeros(M, K, dtype=torch.bool)
        keep[torch.arange(M), G.sel_k(M, K)] = True
        Zo = torch.where(keep, Zo, sign)
    else:
        ones = torch.rand(M, K, generator=g) < 0.1
        ones[0, 0] = True
        Zo = torch.where(ones, sign, Zo)
    W = torch.randn(N, K, generator=g)
    if kind == "a":
        e = torch.randint(-20, 21, (K,), generator=g).float()
        w2, W = torch.ldexp(w2, e), torch.ldexp(W, -e)
    elif kind == "b":
        W = G.operands("b", 4, N, K, off_seed(c, kind))[1]
    return dict(Zo=Zo, W1oT=W, w2=w2, dlog_raw=torch.randn(M, generator=g), s=torch.rand(1, generator=g) + 0.5)


def off_bwd_buffers(c, d, device):
    M, N, K = c["M"], c["N"], c["K"]
    vec = lambda x: G.operand(x[None, :], x.numel(), device)
    out = lambda r, n: G.Guarded(r, n, n, device, "sentinel")
    return dict(Zo=G.operand(d["Zo"], K, device, c["hs_off"]), W1oT=G.operand(d["W1oT"], K, device), w2=vec(d["w2"]),
                dlog_raw=vec(d["dlog_raw"]), s=vec(d["s"]), DHO=out(M, N), dZo=out(M, K), dlog_s=out(1, M))


def off_bwd_check(c, kind, d, bufs):
    fig, fails = {}, []
    M, N, K = c["M"], c["N"], c["K"]
    dev = bufs["DHO"].flat.device
    Zo, W, w2, dl, s = (d[k].to(dev) for k in ("Zo", "W1oT", "w2", "dlog_raw", "s"))
    for k in ("DHO", "dZo", "dlog_s"):
        if not bufs[k].guard_intact():
            fails.append(k + ":guard")
        if not bool(torch.isfinite(bufs[k].view).all()):
            fails.append(k + ":finite")
    if fails:
        return fig, fails
    if not torch.equal(bufs["dlog_s"].view[0], s * dl):
        fails.append("dlog_s:bits")
    lead = (s.double() * dl.double())[:, None] * w2.double()[None, :]
    ref = lead * (1 - Zo.double() ** 2)
    dZo = bufs["dZo"].view.contiguous()
    err, bar = (dZo.double() - ref).abs(), 8 * U * lead.abs()
    nz = lead != 0
    fig["dZo_worst_u"] = float((err[nz] / lead[nz].abs()).max() / U) if bool(nz.any()) else 0.0
    if not bool((err <= bar).all()):
        fails.append("dZo:bar")
    if not bool((dZo[Zo.abs() == 1] == 0).all()):
        fails.append("dZo:nonzero at Zo = +-1")
    rf = G.reference(dZo, W, None, unit=kind == "a")
    e32 = G.max_norm_err(dZo @ W.t(), rf["ref"]) if kind == "a" else None
    f = G.check({"a": "a", "b": "b", "bs": "cs"}[kind], bufs["DHO"].view.contiguous(), rf, K, 0, e32)
    fails += ["DHO:" + x for x in f.pop("fails")]
    fig["DHO"] = f
    return fig, fails


def off_bwd_cpu_kernel(c, bufs, chunks_written=None):
    """torch's CPU fp32 in the kernel's place.  chunks_written: only the
    32-column chunks below it are stored to dZo (the rest stays NaN)."""
    s, dl = bufs["s"].view[0], bufs["dlog_raw"].view[0]
    Zo = bufs["Zo"].view
    dls = s * dl
    bufs["dlog_s"].view[0] = dls
    dZo = dls[:, None] * bufs["w2"].view * (1 - Zo * Zo)
    n = c["K"] if chunks_written is None else min(c["K"], 32 * chunks_written)
    bufs["dZo"].view[:, :n] = dZo[:, :n]
    bufs["DHO"].view.copy_(dZo @ bufs["W1oT"].view.t())


# ----------------------------------------------------------------------------
# 3. gemm_tn_batch and colsum_batch
# ----------------------------------------------------------------------------
# (M, N, K, alpha, beta); lda = M + 4, ldb = N + 4, ldc = N + 3 (even jobs) / N + 4 (odd jobs)
TN_JOBS = ((4, 32, 15, 1.0, 0.0), (32, 36, 16, 1.0, 0.0), (36, 64, 17, -2.0, 0.0), (64, 68, 63, 1.0, 1.0),
           (0, 64, 1, 1.0, 0.0), (68, 132, 64, 1.0, 0.0), (132, 4, 65, 1.0, 0.0), (36, 68, 513, 1.0, 0.0))
TN_JOBS_ONE = ((4, 4, 1, 1.0, 0.0),)    # K = 1, and a batch of one job


@functools.lru_cache(maxsize=4)
def tn_data(batch, kind):
    """Per job dict(A M x K, B N x K, C0 M x N or None) on the CPU."""
    jobs = TN_JOBS if batch == "eight" else TN_JOBS_ONE
    out = []
    for i, (M, N, K, alpha, beta) in enumerate(jobs):
        seed = 1000003 * M + 1009 * N + 17 * K + G.KINDS.index(kind)
        A, B = G.operands(kind, M, N, K, seed)
        C0 = torch.randn(M, N, generator=torch.Generator().manual_seed(seed + 3)) if beta else None
        out.append(dict(A=A, B=B, C0=C0))
    return out


def tn_buffers(jobs, data, device):
    bufs = []
    for i, ((M, N, K, alpha, beta), d) in enumerate(zip(jobs, data)):
        Cg = G.Guarded(max(M, 1), N, N + 3 + i % 2, device, "sentinel")
        if d["C0"] is not None:
            Cg.view.copy_(d["C0"])
        bufs.append(dict(A=G.operand(d["A"].t().contiguous(), M + 4, device),
                         B=G.operand(d["B"].t().contiguous(), N + 4, device), C=Cg))
    return bufs


def tn_check(jobs, kind, data, bufs):
    fig, fails = {}, []
    for i, ((M, N, K, alpha, beta), d, b) in enumerate(zip(jobs, data, bufs)):
        tag = f"job{i}"
        dev = b["C"].flat.device
        if not b["C"].guard_intact():
            fails.append(tag + ":guard")
        if M == 0:
            if not bool(torch.isnan(b["C"].view).all()):
                fails.append(tag + ":a skipped job wrote")
            continue
        A, B = d["A"].to(dev), d["B"].to(dev)
        rf = G.reference(alpha * A, B, None, unit=True)
        C = b["C"].view.contiguous()
        if beta:
            C0 = d["C0"].to(dev).double()
            prod, rf = rf["ref"], dict(ref=rf["ref"] + beta * C0, S=rf["S"] + C0.abs())
        if beta and kind in ("c", "cs"):   # the single-product bar with the addend's rounding
            err, unit = (C.double() - rf["ref"]).abs(), prod.abs() + C0.abs()
            f = dict(worst_u=float((err / unit).max() / U) if bool(torch.isfinite(C).all()) else None,
                     fails=[] if bool((err <= G.C_BAR * unit).all()) else ["c"])
        else:
            f = G.check(kind, C, rf, K)
        if kind == "a" and "worst_of_bar" in f:   # recorded, not barred: fp32 MFMA, no x6 margin
            f["e_maxnorm"] = G.max_norm_err(C, rf["ref"])
            f["e32"] = G.max_norm_err(alpha * A @ B.t() + (beta * d["C0"].to(dev) if beta else 0.0), rf["ref"])
        fails += [f"{tag}:{x}" for x in f.pop("fails")]
        fig[tag] = f
    return fig, fails


def tn_cpu_kernel(jobs, bufs):
    for (M, N, K, alpha, beta), b in zip(jobs, bufs):
        if M:
            prod = alpha * (b["A"].view.t() @ b["B"].view)
            b["C"].view.copy_(prod + beta * b["C"].view if beta else prod)


# (nrows, ncols, weights, out2, beta); ldz = ncols + 3
CS_JOBS = ((1, 1029, False, False, 0.0), (15, 65, True, True, 1.0), (16, 64, False, True, 0.0),
           (17, 63, True, False, 0.0), (4097, 1, True, False, 1.0), (4097, 1029, False, True, 0.0),
           (17, 65, True, True, 1.0), (16, 1, False, False, 0.0))


def colsum_slicing(jobs, scratch_floats):
    """colsum_batch's slicing, restated: per job (slices, rows_per, offset of
    its partials), or None where the scratch cannot hold a job's one slice."""
    used, out = 0, []
    for nrows, ncols, *_ in jobs:
        cblocks = cdiv(ncols, 64)
        slices = min(max(1, min(cdiv(max(nrows, 1), 16), max(1, 1024 // cblocks))), 256)
        left = scratch_floats - used
        if left < ncols:
            return None
        slices = max(1, min(slices, left // ncols))
        rows_per = cdiv(max(nrows, 1), slices)
        slices = max(1, cdiv(max(nrows, 1), rows_per))
        out.append((slices, rows_per, used))
        used += slices * ncols
    return out


CS_AMPLE = sum(256 * j[1] for j in CS_JOBS)


@functools.lru_cache(maxsize=1)
def cs_data():
    """Per job dict(Z nrows x ncols, w or None, out0 or None): with weights row r
    of Z carries 2^e[r] and w[r] 2^-e[r] (data kind a)."""
    out = []
    for i, (nrows, ncols, hasw, has2, beta) in enumerate(CS_JOBS):
        g = torch.Generator().manual_seed(7919 * nrows + 31 * ncols + i)
        Z, w = torch.randn(nrows, ncols, generator=g), None
        if hasw:
            e = torch.randint(-20, 21, (nrows,), generator=g).float()
            Z, w = torch.ldexp(Z, e[:, None]), torch.ldexp(torch.randn(nrows, generator=g), -e)
        out.append(dict(Z=Z, w=w, out0=torch.randn(ncols, generator=g) if beta else None))
    return out


def cs_buffers(jobs, data, device):
    bufs = []
    for (nrows, ncols, hasw, has2, beta), d in zip(jobs, data):
        b = dict(Z=G.operand(d["Z"], ncols + 3, device), w=G.operand(d["w"][None, :], nrows, device) if hasw else None,
                 out=G.Guarded(1, ncols, ncols, device, "sentinel"),
                 out2=G.Guarded(1, ncols, ncols, device, "sentinel") if has2 else None)
        if beta:
            b["out"].view[0] = d["out0"]
            if has2:
                b["out2"].view[0] = d["out0"]
        bufs.append(b)
    return bufs


def cs_check(jobs, data, bufs):
    fig, fails = {}, []
    for i, ((nrows, ncols, hasw, has2, beta), d, b) in enumerate(zip(jobs, data, bufs)):
        tag = f"job{i}"
        dev = b["out"].flat.device
        Z = d["Z"].to(dev).double()
        w = d["w"].to(dev).double() if hasw else torch.ones(nrows, dtype=torch.float64, device=dev)
        ref, S = w @ Z, w.abs() @ Z.abs()
        if beta:
            o = d["out0"].to(dev).double()
            ref, S = ref + beta * o, S + beta * o.abs()
        bar = 2 * max(nrows, 16) * U * S
        for k in ("out", "out2"):
            if b[k] is None:
                continue
            if not b[k].guard_intact():
                fails.append(f"{tag}:{k}:guard")
            v = b[k].view[0]
            if not bool(torch.isfinite(v).all()):
                fails.append(f"{tag}:{k}:finite")
                continue
            err = (v.double() - ref).abs()
            fig[f"{tag}_{k}_worst_of_bar"] = float((err / bar.clamp_min(1e-300)).max())
            if not bool((err <= bar).all()):
                fails.append(f"{tag}:{k}:bar")
        if has2 and not torch.equal(b["out"].view, b["out2"].view):
            fails.append(tag + ":out2 differs")
    return fig, fails


def cs_cpu_kernel(jobs, bufs, slicing, skip_last_slice=False):
    """The two passes in fp32 on the CPU, sliced as ``slicing`` says."""
    for (nrows, ncols, hasw, has2, beta), b, (slices, rows_per, _) in zip(jobs, bufs, slicing):
        Z = b["Z"].view
        w = b["w"].view[0] if hasw else torch.ones(nrows)
        n = slices - 1 if skip_last_slice and slices > 1 else slices
        v = torch.zeros(ncols)
        for sl in range(n):
            r0, r1 = sl * rows_per, min(nrows, (sl + 1) * rows_per)
            v = v + (w[r0:r1, None] * Z[r0:r1]).sum(0)
        for k in ("out", "out2"):
            if b[k] is not None:
                b[k].view[0] = (beta * b[k].view[0] if beta else 0.0) + v


def dump(name, rows):
    G.dump(name, rows)
