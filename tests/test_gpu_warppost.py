"""Posteriors under the time-warped cut on the GPU:
abcd_warp_posterior_forward / abcd_warp_posterior_backward against the
np.longdouble recursions of tests/warppost_cases.py on given planes, bit
equality over every split into calls, the order protocol, the rigid anchor
(ops.span_chain_posterior on the same plane), segment_warp_posteriors and
refit_warp_em on the small models and segment.py --warp --warp_posteriors /
--warp_refit.

Units and bars: tests/warppost_cases.py.  sp(v) is where the device's libm
enters the inputs; the two planes the kernel formed are read out of its state,
bounded against numpy's in ulps, and the reference runs on them."""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import chainpost_cases as CP
import score_cases as S
import warppost_cases as WP
import warpseg_cases as WS
from test_gpu_score import ANN, CKPT, TOY
from test_gpu_syntax import _small_recording

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")
SENT = -7.0   # what the outputs hold before a call
TAIL = 64     # guard bytes behind the workspace
OUTS = ("log_z", "post_k", "gap_post", "tc", "ic", "mc")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _split(N, w):
    return [(a, min(N, a + w)) for a in range(0, N, w)]


def _splits(N):
    """One call, (1, N - 1) and chunks of 7 (each once)."""
    out = [[(0, N)]]
    if N > 1:
        out.append([(0, 1), (1, N)])
    if N > 7:
        out.append(_split(N, 7))
    return out


class Post:
    """The device buffers of one case at padded strides with poisoned padding; ``run`` makes one forward and one
    backward sequence of calls through the C ABI."""

    def __init__(self, d, N, K, T):
        from modules import _native as Nt
        self.N, self.K, self.T, self.d = N, K, T, d
        self.Nt, self.lib = Nt, Nt.lib()
        S_ = K * T
        self.ldc, self.ldt, self.lda = S_ + 5, K + 3, S_ + 3
        self.cost = torch.full((max(N, 1), self.ldc), NAN, device="cuda")
        self.cost[:N, :S_] = torch.from_numpy(d["cost"])
        self.v = torch.from_numpy(d["v"]).reshape(-1).cuda()
        self.trans = torch.full((K, self.ldt), NAN, device="cuda")
        self.trans[:, :K] = torch.from_numpy(d["trans"])
        self.init = torch.from_numpy(d["init"]).cuda()
        self.enter = torch.from_numpy(d["enter"]).cuda()
        self.gap = None if d["gap"] is None else torch.from_numpy(d["gap"]).cuda()
        self.nbytes = self.lib.abcd_warp_posterior_workspace_bytes(N, K, T)
        assert self.nbytes > 0

    def run(self, moves, s_min, scale, fwd=None, bwd=None, want_alpha=True, want_counts=True, want_moves=True, ws=None,
            enter=True, only_forward=False):
        Nt, N, K, T = self.Nt, self.N, self.K, self.T
        f64 = dict(dtype=torch.float64, device="cuda")
        fwd = [(0, N)] if fwd is None else fwd
        bwd = [(0, N)] if bwd is None else bwd
        o = dict(log_z=torch.full((2,), SENT, **f64), post_k=torch.full((2 * (N + 1) * K + 2,), SENT, **f64),
                 gap_post=torch.full((N + 3,), SENT, **f64), tc=torch.full((K * K + 2,), SENT, **f64),
                 ic=torch.full((K + 2,), SENT, **f64), mc=torch.full((3 * K + 2,), SENT, **f64),
                 alpha=torch.full((N + 1, self.lda), SENT, **f64) if want_alpha else None)
        if ws is None:
            ws = torch.full((self.nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        o["ws"] = ws
        lm = (Nt.c_double * 3)(*WP.MOVES[moves] if isinstance(moves, str) else moves)
        model = (Nt.ptr(self.v), lm, Nt.ptr(self.enter) if enter else None, Nt.ptr(self.gap), float(self.d["bonus"]),
                 float(scale), Nt.ptr(self.trans), self.ldt, Nt.ptr(self.init), s_min)
        rcs = []
        for n0, n1 in fwd:
            rcs.append(self.lib.abcd_warp_posterior_forward(
                Nt.ptr(self.cost[n0:]), self.ldc, n0, n1, N, K, T, *model,
                Nt.ptr(o["alpha"][n0:]) if want_alpha else None, self.lda, Nt.ptr(o["log_z"]), Nt.ptr(ws), self.nbytes,
                Nt.stream()))
        for n0, n1 in ([] if only_forward else reversed(bwd)):
            rcs.append(self.lib.abcd_warp_posterior_backward(
                Nt.ptr(self.cost[n0:]), self.ldc, n0, n1, N, K, T, *model,
                Nt.ptr(o["alpha"][n0:]) if want_alpha else None, self.lda, Nt.ptr(o["post_k"]), Nt.ptr(o["gap_post"]),
                Nt.ptr(o["tc"]) if want_counts else None, Nt.ptr(o["ic"]) if want_counts else None,
                Nt.ptr(o["mc"]) if want_moves else None, Nt.ptr(ws), self.nbytes, Nt.stream()))
        torch.cuda.synchronize()
        o["rc"] = rcs
        return o

    def planes(self, o):
        from modules import ops
        return ops.warp_posterior_planes(o["ws"][:self.nbytes], self.N, self.K, self.T)

    def result(self, o):
        """The device's outputs under the reference's keys (numpy)."""
        N, K = self.N, self.K
        p = self.planes(o)
        return dict(log_z=float(o["log_z"][0]), lattice=p["lattice"].cpu().numpy(),
                    lattice_g=np.stack([p["G"].cpu().numpy(), p["bG"].cpu().numpy()]),
                    post_k=o["post_k"][:2 * (N + 1) * K].reshape(2, N + 1, K).cpu().numpy(),
                    gap_post=o["gap_post"][:N + 1].cpu().numpy(), trans_counts=o["tc"][:K * K].reshape(K, K).cpu().numpy(),
                    init_counts=o["ic"][:K].cpu().numpy(), move_counts=o["mc"][:3 * K].reshape(K, 3).cpu().numpy())

    def untouched(self, o, want_counts=True, want_moves=True):
        """Nothing outside the blocks was written: the tails of the outputs, alpha's padding, the workspace's tail."""
        N, K, S_ = self.N, self.K, self.K * self.T
        ok = bool((o["ws"][self.nbytes:] == 0xA5).all())
        ok = ok and float(o["log_z"][1]) == SENT and bool((o["post_k"][2 * (N + 1) * K:] == SENT).all())
        ok = ok and bool((o["gap_post"][N + 1:] == SENT).all())
        ok = ok and bool((o["tc"][K * K if want_counts else 0:] == SENT).all())
        ok = ok and bool((o["ic"][K if want_counts else 0:] == SENT).all())
        ok = ok and bool((o["mc"][3 * K if want_moves else 0:] == SENT).all())
        if o["alpha"] is not None:
            ok = ok and bool((o["alpha"][:, S_:] == SENT).all()) and bool((o["alpha"][N:] == SENT).all())
        return ok


def _same(a, b, p, outs=OUTS, lattice=True):
    for key in outs:
        if not torch.equal(_bits(a[key]), _bits(b[key])):
            return key
    if lattice:
        pa, pb = p.planes(a), p.planes(b)
        for key in ("lattice", "G", "bG", "cont", "last"):
            if not torch.equal(_bits(pa[key]), _bits(pb[key])):
                return key
    return None


def _over(got, ref, bar, rel=False):
    """The worst |got - ref| over its bar (bar (1 + ref) with ``rel``) on the finite reference entries; the
    reference's -inf entries must be -inf."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), "the -inf entries differ"
    assert not np.isnan(got).any()
    if not fin.any():
        return 0.0
    scale = bar * (1.0 + np.abs(ref[fin])) if rel else bar
    return float((np.abs(got[fin] - ref[fin]) / scale).max())


# ----------------------------------------------------------------------------
# 1. against the reference
# ----------------------------------------------------------------------------
def check_case(N, K, T, kind):
    d = WS.prog_inputs(N, K, T, kind)
    p = Post(d, N, K, T)
    rows = []
    for s_min in WP.PROG_SMIN:
        for scale in WP.SCALES:
            moves = "default" if scale == 1.0 else "staystep"            # a disabled move at the second scale
            tag = (N, K, T, kind, s_min, scale)
            if s_min >= T:
                assert p.run(moves, s_min, scale)["rc"] == [p.Nt.ABCD_EINVAL] * 2
                continue
            o = p.run(moves, s_min, scale)
            assert o["rc"] == [0, 0], tag
            assert p.untouched(o), tag
            pl = p.planes(o)
            cont, last = pl["cont"].cpu().numpy(), pl["last"].cpu().numpy()
            v64 = d["v"].astype(np.float64)
            ulps = max(WS.ulps_apart(cont, WS.softplus(v64)), WS.ulps_apart(last, WS.softplus(-v64)))
            assert ulps <= WP.SP_ULPS, (tag, ulps)
            ref = WP.prog_reference(N, K, T, kind, moves, s_min, scale, cont, last)
            got = p.result(o)
            bar = WP.lattice_bar(N, K, T, ref["lattice"])
            row = dict(N=N, K=K, T=T, kind=kind, s_min=s_min, scale=scale, moves=moves, bar=bar, sp_ulps=ulps)
            if ref["log_z"] == NEG:
                assert got["log_z"] == NEG, tag
                row["log_z_over_bar"] = 0.0
            else:
                row["log_z_over_bar"] = abs(got["log_z"] - ref["log_z"]) / bar
            row["lattice_over_bar"] = max(_over(got["lattice"], ref["lattice"], bar),
                                          _over(got["lattice_g"], ref["lattice_g"], bar))
            row["post_over_bar"] = _over(got["post_k"], ref["post_k"], 5 * bar)
            row["gap_over_bar"] = _over(got["gap_post"], ref["gap_post"], 5 * bar)
            row["trans_over_bar"] = _over(got["trans_counts"], ref["trans_counts"], 5 * bar, rel=True)
            row["init_over_bar"] = _over(got["init_counts"], ref["init_counts"], 5 * bar, rel=True)
            row["moves_over_bar"] = _over(got["move_counts"], ref["move_counts"], 5 * bar, rel=True)
            bg0 = got["lattice_g"][1][0]
            row["bg0_over_bar"] = 0.0 if (bg0 == NEG and got["log_z"] == NEG) else abs(bg0 - got["log_z"]) / (2 * bar)
            print(f"warp_posterior {tag}: " + " ".join(f"{k}={v:.3g}" for k, v in row.items() if k.endswith("_bar")))
            for key, val in row.items():
                if key.endswith("_over_bar"):
                    assert val <= 1.0, (tag, key, val)
            # exact zeros where no path passes
            lat = ref["lattice"]
            with np.errstate(invalid="ignore"):
                dead_on, dead_end = ~(lat[0] + lat[3] > NEG), ~(lat[1] + lat[4] > NEG)
            assert (got["post_k"][0][dead_on] == 0.0).all() and (got["post_k"][1][dead_end] == 0.0).all(), tag
            assert got["gap_post"][N] == 0.0
            if d["gap"] is None:
                assert (got["gap_post"] == 0.0).all()
            if kind == "nopath":
                assert got["log_z"] == NEG
                for key in ("post_k", "gap_post", "trans_counts", "init_counts", "move_counts"):
                    assert (got[key] == 0.0).all(), (tag, key)
            ids = WP.identities(got)
            row.update({"id_" + k: v for k, v in ids.items()})
            if got["log_z"] > NEG:
                # every posterior is within 5 bars of a value that satisfies the identity exactly
                assert max(ids["cover"], ids["onsets"]) <= 10 * bar * (N + 1) * K + 5 * bar * (K * K + K), (tag, ids)
            rows.append(row)
    WP.dump(f"sweep_n{N}k{K}t{T}_{kind}", rows)
    return rows


@pytest.mark.parametrize("kind", WP.PROG_KINDS)
@pytest.mark.parametrize("KT", WP.PROG_KT, ids=lambda v: f"k{v[0]}t{v[1]}")
@pytest.mark.parametrize("N", WP.PROG_N)
def test_sweeps_against_the_longdouble_recursions(N, KT, kind):
    K, T = KT
    rows = check_case(N, K, T, kind)
    if kind == "random" and N >= 33:
        assert any(r["scale"] == 1.0 for r in rows)


def test_plan_and_workspace_match_the_cases():
    """(130, 5) streams log_trans, (33, 37) and (65, 20) hold more states than the workgroup has threads; the
    plan has one launch width, so there is no threshold in K to straddle."""
    import ctypes
    from modules import _native as Nt
    res, thr, lds = Nt.c_int(-1), Nt.c_int(-1), Nt.c_size_t(0)
    for K, T in WP.PROG_KT + ((256, 5), (257, 5), (1024, 5)):
        assert Nt.lib().abcd_warp_posterior_plan(K, T, ctypes.byref(res), ctypes.byref(thr), ctypes.byref(lds)) == 0
        assert res.value == (K <= 128) and thr.value == 1024 and lds.value <= 160 * 1024
    assert any(K * T > 1024 for K, T in WP.PROG_KT) and any(K > 128 for K, _ in WP.PROG_KT)


# ----------------------------------------------------------------------------
# 2. bits
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,T,kind", [(2, 2, 3, "random"), (33, 33, 37, "random"), (70, 130, 5, "gaps"),
                                        (33, 65, 20, "holes"), (70, 1, 1, "random")])
def test_every_split_gives_the_one_call_bits(N, K, T, kind):
    d = WS.prog_inputs(N, K, T, kind)
    p = Post(d, N, K, T)
    s_min = min(2, T - 1)
    one = p.run("default", s_min, 0.25)
    assert one["rc"] == [0, 0] and p.untouched(one)
    again = p.run("default", s_min, 0.25)
    assert _same(again, one, p) is None                                       # two runs agree
    assert torch.equal(_bits(again["alpha"]), _bits(one["alpha"]))
    for fwd in _splits(N):
        for bwd in _splits(N):
            got = p.run("default", s_min, 0.25, fwd=fwd, bwd=bwd)
            assert all(rc == 0 for rc in got["rc"]) and p.untouched(got)
            assert _same(got, one, p) is None, (fwd, bwd, _same(got, one, p))
            assert torch.equal(_bits(got["alpha"]), _bits(one["alpha"]))
    # what is asked for changes no other output's bits
    bare = p.run("default", s_min, 0.25, fwd=_splits(N)[-1], bwd=_splits(N)[-1], want_alpha=False, want_counts=False,
                 want_moves=False)
    assert bare["rc"] == [0] * len(bare["rc"]) and p.untouched(bare, False, False)
    assert _same(bare, one, p, outs=("log_z", "post_k", "gap_post")) is None
    counts = p.run("default", s_min, 0.25, want_alpha=True, want_counts=True, want_moves=False)
    assert _same(counts, one, p, outs=("log_z", "post_k", "gap_post", "tc", "ic")) is None
    assert p.untouched(counts, True, False)
    moves = p.run("default", s_min, 0.25, want_counts=False)
    assert _same(moves, one, p, outs=("log_z", "post_k", "gap_post", "mc")) is None


# ----------------------------------------------------------------------------
# 3. the order protocol
# ----------------------------------------------------------------------------
def test_calls_out_of_order_are_visible_and_harmless():
    from modules import ops
    N, K, T = 70, 33, 37
    d = WS.prog_inputs(N, K, T, "random")
    p = Post(d, N, K, T)
    one = p.run("default", 0, 1.0)
    a = p.run("default", 0, 1.0, fwd=[(0, 10)], only_forward=True)
    assert a["rc"] == [0] and float(a["log_z"][0]) == SENT                    # not the last call: log_z is not written
    keep = a["ws"].clone()
    b = p.run("default", 0, 1.0, fwd=[(12, 20)], only_forward=True, ws=a["ws"])   # 10 is due
    assert b["rc"] == [0] and math.isnan(float(b["log_z"][0]))
    assert torch.equal(b["ws"], keep)                                         # the carry is as it was
    # a backward call before the forward sweep is through: status 1, nothing else changes
    c = p.run("default", 0, 1.0, fwd=[], bwd=[(0, N)], ws=a["ws"])
    nxt = p.planes(c)["next"].tolist()
    assert c["rc"] == [0] and nxt[0] == 10 and nxt[2] == 1
    assert bool((c["post_k"] == SENT).all()) and bool((c["gap_post"] == SENT).all())
    e = p.run("default", 0, 1.0, fwd=[(10, 40), (40, N)], bwd=[(50, N)], ws=a["ws"])
    assert e["rc"] == [0, 0, 0] and p.planes(e)["next"].tolist() == [N, 50, 0]
    keep = e["ws"].clone()
    f = p.run("default", 0, 1.0, fwd=[], bwd=[(0, 40)], ws=e["ws"])          # 50 is due
    assert p.planes(f)["next"].tolist() == [N, 50, 1]
    status_at = 8 * (ops._warp_posterior_words(N, K, T) + 3)                  # the status word alone differs
    assert torch.equal(f["ws"][:status_at], keep[:status_at])
    g = p.run("default", 0, 1.0, fwd=[], bwd=[(0, 50)], ws=e["ws"])
    assert p.planes(g)["next"].tolist() == [N, 0, 0]
    g["log_z"][0] = one["log_z"][0]                                           # the forward call wrote it elsewhere
    g["alpha"] = None
    assert _same(g, one, p, outs=("post_k", "gap_post", "tc", "ic")) is None  # (the move counts need alpha's rows)
    # the operators: the forward call reports NaN, the backward call raises and the sweep goes on
    cost = torch.from_numpy(d["cost"]).cuda()
    state = ops.warp_posterior_state(N, K, T, "cuda")
    alpha = torch.empty(N, K * T, dtype=torch.float64, device="cuda")
    args = (N, K, p.v, list(WP.MOVES["default"]), p.enter, p.gap, d["bonus"], 1.0, p.trans[:, :K], p.init, 0, state)
    with pytest.raises(RuntimeError, match="out of order"):
        ops.warp_posterior_backward(cost, 0, N, *args, alpha, True, True)     # a new state: nothing has run
    assert math.isnan(float(ops.warp_posterior_forward(cost[:32], 0, 32, *args, alpha[:32])))
    assert math.isnan(float(ops.warp_posterior_forward(cost[40:], 40, N, *args, alpha[40:])))
    lz = ops.warp_posterior_forward(cost[32:], 32, N, *args, alpha[32:])
    assert torch.equal(_bits(lz.reshape(1)), _bits(one["log_z"][:1]))
    first = ops.warp_posterior_backward(cost[20:], 20, N, *args, alpha[20:], True, True)
    assert bool(torch.isnan(first[0]).all())
    with pytest.raises(RuntimeError, match="out of order"):
        ops.warp_posterior_backward(cost[:10], 0, 10, *args, alpha[:10], True, True)
    out = ops.warp_posterior_backward(cost[:20], 0, 20, *args, alpha[:20], True, True)
    got = dict(post_k=out[0].reshape(-1), gap_post=out[1], tc=out[2].reshape(-1), ic=out[3], mc=out[4].reshape(-1))
    want = dict(post_k=one["post_k"][:2 * (N + 1) * K], gap_post=one["gap_post"][:N + 1], tc=one["tc"][:K * K],
                ic=one["ic"][:K], mc=one["mc"][:3 * K])
    for key in got:
        assert torch.equal(_bits(got[key]), _bits(want[key])), key
    pl = ops.warp_posterior_planes(state, N, K, T)
    assert torch.equal(_bits(pl["lattice"]), _bits(p.planes(one)["lattice"]))


# ----------------------------------------------------------------------------
# 4. anchors on the device
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,T,kind,s_min", [(33, 33, 37, "random", 0), (70, 65, 20, "gaps", 2),
                                              (33, 130, 5, "zeros", 0), (70, 2, 3, "holes", 1)])
def test_step_only_is_the_rigid_posterior(N, K, T, kind, s_min):
    from modules import ops
    d = WS.prog_inputs(N, K, T, kind)
    p = Post(d, N, K, T)
    o = p.run("identity", s_min, 1.0, enter=False)
    assert o["rc"] == [0, 0]
    got = p.result(o)
    pl = p.planes(o)
    table = WP.rigid_table64(d["cost"], d["v"], pl["cont"].cpu().numpy(), pl["last"].cpu().numpy())
    r = ops.span_chain_posterior(torch.from_numpy(table).cuda(), s_min + 1, p.gap, d["bonus"], 1.0, p.trans[:, :K],
                                 p.init, True, False)
    lz, lat, latg, post_k, gap_post, tc, ic = (t.cpu().numpy() for t in r[:7])
    bar = WP.lattice_bar(N, K, T, got["lattice"]) + CP.lattice_bar(N, T, K, lat)
    worst = 0.0
    if float(lz) == NEG:
        assert got["log_z"] == NEG
    else:
        worst = abs(got["log_z"] - float(lz)) / bar
    worst = max(worst, _over(got["lattice"], lat, bar), _over(got["lattice_g"], latg, bar),
                _over(got["post_k"], post_k, 5 * bar), _over(got["gap_post"], gap_post, 5 * bar),
                _over(got["trans_counts"], tc, 5 * bar, rel=True), _over(got["init_counts"], ic, 5 * bar, rel=True))
    print(f"step-only warped posterior against span_chain_posterior N={N} K={K} T={T} {kind}: {worst:.3g} of the "
          "summed bars")
    assert worst <= 1.0
    # with the step move alone every move is a step
    assert (got["move_counts"][:, 0] == 0.0).all() and (got["move_counts"][:, 2] == 0.0).all()
    WP.dump(f"rigid_n{N}k{K}t{T}_{kind}", [dict(N=N, K=K, T=T, kind=kind, over_bar=worst)])


@pytest.mark.parametrize("kind", ("random", "gaps", "holes"))
def test_evidence_is_at_least_the_best_path(kind):
    from modules import ops
    N, K, T = 70, 33, 37
    d = WS.prog_inputs(N, K, T, kind)
    p = Post(d, N, K, T)
    o = p.run("default", 0, 1.0)
    cost = torch.from_numpy(d["cost"]).cuda()
    best = ops.warp_segment_window(cost, 0, N, N, K, p.v, list(WP.MOVES["default"]), p.enter, p.gap, d["bonus"],
                                   p.trans[:, :K], p.init, 0, ops.warp_segment_state(N, K, T, "cuda"), None)
    bar = WP.lattice_bar(N, K, T, p.result(o)["lattice"])
    assert float(o["log_z"][0]) >= float(best[0]) - bar


def test_einval_and_the_empty_recording():
    from modules import _native as Nt
    N, K, T = 33, 2, 3
    d = WS.prog_inputs(N, K, T, "random")
    p = Post(d, N, K, T)
    E = Nt.ABCD_EINVAL
    for scale in (0.0, -1.0, math.inf, math.nan):
        o = p.run("default", 0, scale)
        assert o["rc"] == [E, E] and p.untouched(o, False, False) and float(o["log_z"][0]) == SENT
        assert bool((o["ws"] == 0xA5).all())                                   # nothing is written
    assert p.run((NEG, NEG, NEG), 0, 1.0)["rc"] == [E, E]
    assert p.run((0.0, NAN, 0.0), 0, 1.0)["rc"] == [E, E]
    assert p.run("default", 0, 1.0, want_alpha=False, want_counts=True, want_moves=True)["rc"] == [0, E]
    lib, lm = p.lib, (Nt.c_double * 3)(*WP.MOVES["default"])
    f64 = dict(dtype=torch.float64, device="cuda")
    ws = torch.full((p.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * (N + 1) * K,), SENT, **f64)

    def bw(tc=None, ic=None, mc=None, alpha=None, lda=K * T, nb=p.nbytes):
        return lib.abcd_warp_posterior_backward(Nt.ptr(p.cost), p.ldc, 0, N, N, K, T, Nt.ptr(p.v), lm, None, None, 0.0,
                                                1.0, Nt.ptr(p.trans), p.ldt, Nt.ptr(p.init), 0, alpha, lda, Nt.ptr(out),
                                                Nt.ptr(out), tc, ic, mc, Nt.ptr(ws), nb, Nt.stream())
    some = Nt.ptr(out)
    assert bw(tc=some) == E and bw(ic=some) == E                               # exactly one bigram buffer
    assert bw(mc=some) == E and bw(mc=some, alpha=some, lda=K * T - 1) == E   # move counts need alpha at a full stride
    assert bw(nb=p.nbytes - 1) == E
    assert lib.abcd_warp_posterior_forward(Nt.ptr(p.cost), p.ldc, 0, N, N, K, T, Nt.ptr(p.v), lm, None, None, 0.0, 1.0,
                                           Nt.ptr(p.trans), p.ldt, Nt.ptr(p.init), 0, some, K * T - 1, some, Nt.ptr(ws),
                                           p.nbytes, Nt.stream()) == E
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ws == 0xA5).all())
    # N = 0: log_z = 0, zero posteriors and counts, nothing is read
    z = Post(dict(d, cost=d["cost"][:0], gap=None), 0, K, T)
    o = z.run("default", 0, 1.0, fwd=[(0, 0)], bwd=[(0, 0)], want_alpha=False, want_moves=False)
    assert o["rc"] == [0, 0] and float(o["log_z"][0]) == 0.0 and z.untouched(o, True, False)
    assert bool((o["post_k"][:2 * K] == 0.0).all()) and float(o["gap_post"][0]) == 0.0
    assert bool((o["tc"][:K * K] == 0.0).all()) and bool((o["ic"][:K] == 0.0).all())
    assert bool((o["ws"] == 0xA5).all())


# ----------------------------------------------------------------------------
# 5. segment_warp_posteriors on the small models
# ----------------------------------------------------------------------------
KEYS = ("log_evidence", "onset", "end", "gap", "onset_by_category", "end_by_category", "frame_category",
        "expected_segments", "category_usage", "no_segment")


@pytest.mark.parametrize("name", list(S.E2E_SMALL))
def test_segment_warp_posteriors_on_a_small_model(name):
    from modules import segmentation
    from modules.sequence import TransitionModel
    dec, protos, frames, K, D = _small_recording(name)
    n = int(frames.shape[0])
    model = TransitionModel.from_log_weight(torch.linspace(-1.0, 1.0, K).cuda())
    gap = torch.full((n,), -60.0, device="cuda")
    kw = dict(transitions=model, gap=gap, seg_bonus=-1.0, min_state=1, temperature=4.0)
    out = segmentation.segment_warp_posteriors(dec, protos, frames, D, want_counts=True, want_moves=True,
                                               with_segments=True, **kw)
    assert set(KEYS) <= set(out) and {"trans_counts", "init_counts", "move_counts", "expected_tempo"} <= set(out)
    shapes = dict(log_evidence=(), onset=(n + 1,), end=(n + 1,), gap=(n + 1,), onset_by_category=(n + 1, K),
                  end_by_category=(n + 1, K), frame_category=(n, K), expected_segments=(), category_usage=(K,),
                  no_segment=(), trans_counts=(K, K), init_counts=(K,), move_counts=(K, 3), expected_tempo=(K,))
    for key, shape in shapes.items():
        assert tuple(out[key].shape) == shape and out[key].dtype == torch.float64, key
    assert math.isfinite(float(out["log_evidence"]))
    for key in ("onset", "end", "gap", "frame_category", "onset_posterior", "end_posterior", "occupancy"):
        assert bool((out[key] >= 0).all()) and bool((out[key] <= 1 + 1e-9).all()), key
    # 1e-9: the tolerance segment_chain_posteriors' test gives the same identities
    cover = out["frame_category"].sum(1) + out["gap"][:n]
    assert float((cover - 1.0).abs().max()) <= 1e-9
    total = float(out["onset"].sum())
    assert abs(total - float(out["end"].sum())) <= 1e-9 * max(1.0, total)
    assert abs(total - float(out["trans_counts"].sum() + out["init_counts"].sum())) <= 1e-9 * max(1.0, total)
    inside = float(out["frame_category"].sum())
    assert abs(float(out["move_counts"].sum()) + float(out["end"].sum()) - inside) <= 1e-9 * max(1.0, inside)
    assert abs(float(out["init_counts"].sum()) + float(out["no_segment"]) - 1.0) <= 1e-9
    # the cut is segment_frames_warped's, bit for bit
    seg = segmentation.segment_frames_warped(dec, protos, frames, D, transitions=model, gap=gap, seg_bonus=-1.0,
                                             min_state=1)
    assert set(seg) == set(out["segmentation"])
    for key in seg:
        assert torch.equal(seg[key], out["segmentation"][key]), key
    k = len(seg["onset"])
    assert tuple(out["onset_posterior"].shape) == tuple(out["end_posterior"].shape) == tuple(out["occupancy"].shape) == (k,)
    assert float(out["log_evidence"]) * 4.0 >= float(seg["path_score"]) - 1e-6 * abs(float(seg["path_score"]))
    # the chunks change no bit
    for chunk in (7, 1000):
        again = segmentation.segment_warp_posteriors(dec, protos, frames, D, want_counts=True, want_moves=True,
                                                     chunk_frames=chunk, **kw)
        for key in again:
            assert torch.equal(_bits(again[key]), _bits(out[key])), (chunk, key)
    print(f"{name}: log evidence {float(out['log_evidence']):.3f} at temperature 4, {float(out['expected_segments']):.2f} "
          f"expected segments, {k} chosen")
    WP.dump(f"e2e_{name}", [dict(case=name, cover=float((cover - 1.0).abs().max()))])


@pytest.mark.parametrize("name", list(S.E2E_SMALL)[:1])
def test_expected_tempo_follows_the_playing_speed(name):
    from modules import segmentation
    dec, protos, _, K, D = _small_recording(name)
    plain = protos[0][:D, 0].float().contiguous()                              # prototype 0's mean frames, as they are
    doubled = plain.repeat_interleave(2, 0)                                    # and with every frame doubled
    tempo = []
    for frames in (plain, doubled):
        out = segmentation.segment_warp_posteriors(dec, protos, frames, D, seg_bonus=-10.0, min_state=D - 1,
                                                   want_moves=True)
        use, t = out["category_usage"], out["expected_tempo"]
        ok = use > 0
        assert bool(ok.any()) and bool(torch.isnan(t[~ok]).all())
        tempo.append(float((t[ok] * use[ok]).sum() / use[ok].sum()))
    print(f"{name}: expected tempo {tempo[0]:.3f} as it is, {tempo[1]:.3f} with every frame doubled")
    assert tempo[1] < tempo[0]


# ----------------------------------------------------------------------------
# 6. EM
# ----------------------------------------------------------------------------
def test_refit_warp_em_on_the_device_is_the_reference_em():
    from modules import ops, segmentation
    from modules.sequence import TransitionModel
    recs = WP.em_recordings()
    K, T = recs[0]["v"].shape[1], recs[0]["v"].shape[0]
    seen = []

    def device_fn(rec, model, log_moves):
        n = rec["cost"].shape[0]
        cost = torch.from_numpy(rec["cost"]).cuda()
        v = torch.from_numpy(rec["v"]).reshape(-1).cuda()
        state = ops.warp_posterior_state(n, K, T, "cuda")
        alpha = torch.empty(n, K * T, dtype=torch.float64, device="cuda")
        args = (n, K, v, list(log_moves), None, None, 0.0, 1.0, model.log_trans.cuda(), model.log_init.cuda(), 0, state)
        lz = ops.warp_posterior_forward(cost, 0, n, *args, alpha)
        _, _, tc, ic, mc = ops.warp_posterior_backward(cost, 0, n, *args, alpha, True, True)
        ref = WP.em_posterior_fn()(rec, model, log_moves)
        bar = WP.lattice_bar(n, K, T, ref["lattice"])
        over = max(_over(tc.cpu().numpy(), ref["trans_counts"], 5 * bar, rel=True),
                   _over(ic.cpu().numpy(), ref["init_counts"], 5 * bar, rel=True),
                   _over(mc.cpu().numpy(), ref["move_counts"], 5 * bar, rel=True),
                   abs(float(lz) - ref["log_evidence"]) / bar)
        seen.append(over)
        return dict(log_evidence=lz, trans_counts=tc, init_counts=ic, move_counts=mc)

    start = (math.log(0.2), math.log(0.6), NEG)                               # skip disabled: it stays disabled
    a, b = TransitionModel(K), TransitionModel(K)
    tot_d, lm_d = segmentation.refit_warp_em(device_fn, recs, a, start, 3, 0.0, move_smoothing=0.0)
    tot_r, lm_r = segmentation.refit_warp_em(WP.em_posterior_fn(), recs, b, start, 3, 0.0, move_smoothing=0.0)
    assert max(seen) <= 1.0, seen
    assert lm_d[2] == NEG and lm_r[2] == NEG
    assert max(abs(x - y) for x, y in zip(lm_d[:2], lm_r[:2])) <= 1e-9
    assert max(abs(x - y) for x, y in zip(tot_d, tot_r)) <= 1e-9 * max(abs(t) for t in tot_r)
    assert torch.allclose(a.log_trans.cpu(), b.log_trans.cpu(), atol=1e-6)
    print(f"refit_warp_em: device counts within {max(seen):.3g} of their bars; moves "
          f"{[round(math.exp(m), 4) if m > NEG else 0.0 for m in lm_d]}")
    WP.dump("em_planted", [dict(over_bar=max(seen))])


# ----------------------------------------------------------------------------
# 7. segment.py --warp --warp_posteriors / --warp_refit on the toy data
# ----------------------------------------------------------------------------
def test_segment_cli_with_warp_posteriors_and_refit(tmp_path):
    import segment
    K = 16
    base = [CKPT, TOY, ANN, "1.0", "--max_length", "60", "--min_length", "3", "--warp"]
    out = os.path.join(str(tmp_path), "p", "segmented.csv")
    rec = os.path.join(str(tmp_path), "p", "recordings.csv")
    curves = os.path.join(str(tmp_path), "p", "curves")
    segment.main(base + ["-S", out, "--warp_posteriors", "--posterior_temperature", "8", "--recordings_out", rec,
                         "--curves_dir", curves, "--chunk_frames", "50"])
    df = pd.read_csv(out)
    assert list(df.columns) == list(segment.COLUMNS) + list(segment.WARP_COLUMNS) + list(segment.WARP_POSTERIOR_COLUMNS)
    assert len(df) >= 1
    for c in segment.WARP_POSTERIOR_COLUMNS:
        assert ((df[c] >= 0) & (df[c] <= 1 + 1e-9)).all(), c
    plain = os.path.join(str(tmp_path), "q", "segmented.csv")
    segment.main(base + ["-S", plain, "--chunk_frames", "50"])
    pd.testing.assert_frame_equal(df[list(segment.COLUMNS) + list(segment.WARP_COLUMNS)], pd.read_csv(plain),
                                  check_exact=True)                            # the cut is --warp's own
    rt = pd.read_csv(rec)
    assert list(rt.columns) == list(segment.RECORDING_COLUMNS) and len(rt) == df["input_path"].nunique()
    assert np.isfinite(rt["log_evidence"]).all() and (rt["expected_segments"] > 0).all()
    files = sorted(os.listdir(curves))
    assert len(files) == len(rt)
    with np.load(os.path.join(curves, files[0])) as z:
        n = int(rt["n_frames"][0]) if len(rt) == 1 else len(z["onset"]) - 1
        for key in ("onset", "end", "gap"):
            assert z[key].shape == (n + 1,) and (z[key] >= 0).all() and (z[key] <= 1 + 1e-9).all()
        assert z["frame_category"].shape == (n,) and (z["frame_category_probability"] <= 1 + 1e-9).all()
    # EM of the moves and the matrix under the warped programme
    p = np.full((K, K), 0.2 / (K - 1))
    np.fill_diagonal(p, 0.8)
    ft, tt = np.divmod(np.arange(K * K), K)
    tcsv = os.path.join(str(tmp_path), "transitions.csv")
    pd.DataFrame({"from_ix": ft, "to_ix": tt, "probability": p.reshape(-1), "expected_count": 0.0}).to_csv(
        tcsv, index=False)
    out_r = os.path.join(str(tmp_path), "r", "segmented.csv")
    tout = os.path.join(str(tmp_path), "r", "transitions.csv")
    mout = os.path.join(str(tmp_path), "r", "moves.csv")
    segment.main(base + ["-S", out_r, "--transitions", tcsv, "--warp_refit", "2", "--transitions_out", tout,
                         "--moves_out", mout, "--chunk_frames", "50"])
    dr = pd.read_csv(out_r)
    assert list(dr.columns) == list(segment.COLUMNS) + list(segment.WARP_COLUMNS) + ["transition_score"]
    tr = pd.read_csv(tout)
    assert list(tr.columns) == list(segment.TRANSITION_COLUMNS) and len(tr) == K * K
    assert np.allclose(tr["probability"].to_numpy().reshape(K, K).sum(1), 1.0, atol=1e-5)
    assert ((tr["probability"] >= 0) & (tr["probability"] <= 1)).all() and (tr["expected_count"] >= 0).all()
    mv = pd.read_csv(mout)
    assert list(mv.columns) == list(segment.MOVE_COLUMNS) and len(mv) == 1
    probs = mv.iloc[0].to_numpy(dtype=np.float64)
    assert ((probs >= 0) & (probs <= 1)).all() and abs(probs.sum() - 1.0) <= 1e-9
    print(f"segment.py --warp_refit 2: moves {probs.round(4).tolist()}, {len(dr)} segments")
