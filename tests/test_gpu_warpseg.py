"""Time-warped segmentation on the GPU: abcd_frame_costs
against float64 inside guarded buffers, abcd_warp_segment_window for EQUALITY
with the float64 loop of tests/warpseg_cases.py on given planes and in any
split into calls, segment_frames_warped on the small models, the planted
recording and segment.py --warp.

Units and bars: tests/warpseg_cases.py.  sp(v) is where the device's libm
enters; the two planes the kernel formed are read out of its state, bounded
against numpy's in ulps, and the programme is checked for equality on them."""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import score_cases as S
import warp_cases as WC
import warpseg_cases as WS
from test_gpu_score import ANN, CKPT, TOY
from test_gpu_syntax import _small_recording

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")
SENT = -7.0   # what the outputs hold before a call
TAIL = 64     # guard bytes behind the workspace


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _padded(a, ld):
    """a (rows x cols fp32 numpy) on the device at row stride ld, NaN in the padding -> (buffer, view)."""
    rows, cols = a.shape
    buf = torch.full((rows, ld), NAN, device="cuda")
    buf[:, :cols] = torch.from_numpy(a)
    return buf


# ----------------------------------------------------------------------------
# 1. the plane
# ----------------------------------------------------------------------------
def plane_call(d, N, K, T, F, n0, n1, pad):
    """abcd_frame_costs on frames n0 .. n1 - 1 -> (rc, the (n1 - n0 + 2) x ld_cost buffer that held SENT)."""
    from modules import _native as Nt
    lib = Nt.lib()
    ld = WS.PAD_LD if pad else F
    x, mu, lv = (_padded(d[k], ld) for k in ("x", "mu", "lv"))
    ldc = K * T + (3 if pad else 0)
    cost = torch.full((n1 - n0 + 2, ldc), SENT, device="cuda")
    rc = lib.abcd_frame_costs(Nt.ptr(x), ld, N, n0, n1, F, K, T, Nt.ptr(mu), ld, Nt.ptr(lv), ld, Nt.ptr(cost), ldc,
                              Nt.stream())
    torch.cuda.synchronize()
    return rc, cost


@pytest.mark.parametrize("F", WS.PLANE_F)
@pytest.mark.parametrize("T", WS.PLANE_T)
@pytest.mark.parametrize("K", WS.PLANE_K)
@pytest.mark.parametrize("N", WS.PLANE_N)
def test_frame_costs_abi(N, K, T, F):
    d = WS.plane_inputs(N, K, T, F)
    e, unit = WS.plane_reference(N, K, T, F)
    R = K * T
    worst = 0.0
    whole = None
    for pad in (False, True):
        rc, cost = plane_call(d, N, K, T, F, 0, N, pad)
        assert rc == 0
        got = cost[:N, :R]
        err = float(((got.double().cpu() - torch.from_numpy(e)).abs() / torch.from_numpy(unit)).max())
        worst = max(worst, err)
        assert err <= WS.BAR, (N, K, T, F, pad, err)
        assert bool((cost[N:] == SENT).all()) and bool((cost[:, R:] == SENT).all())   # nothing outside the block
        if whole is None:
            whole = got.clone()
        assert torch.equal(_bits(got), _bits(whole))                                  # the strides change no bit
        rc2, again = plane_call(d, N, K, T, F, 0, N, pad)
        assert torch.equal(_bits(again), _bits(cost))                                 # two calls agree
    chunks = [(0, min(32, N))] + ([(32, N)] if N > 32 else []) + ([(5, 40)] if N >= 40 else [])
    for n0, n1 in chunks:
        rc, cost = plane_call(d, N, K, T, F, n0, n1, True)
        assert rc == 0
        assert torch.equal(_bits(cost[:n1 - n0, :R]), _bits(whole[n0:n1])), (n0, n1)
        assert bool((cost[n1 - n0:] == SENT).all()) and bool((cost[:, R:] == SENT).all())
    print(f"frame_costs N={N} K={K} T={T} F={F}: worst error {worst:.2e} of the unit (bar {WS.BAR})")
    WS.dump(f"plane_n{N}k{K}t{T}f{F}", [dict(N=N, K=K, T=T, F=F, plane=worst)])


def test_frame_costs_beyond_65535_frame_tiles():
    """A chunk of more than 32 * 65535 frames (allowed while (n1 - n0) ld_cost < 2^31): more frame tiles than a
    grid's second dimension holds."""
    from modules import ops
    N = 32 * 65536 + 5
    g = np.random.default_rng(5)
    x = g.normal(size=(N, 1)).astype(np.float32)
    mu, lv = np.float32(0.25), np.float32(-1.5)
    got = ops.frame_costs(torch.from_numpy(x).cuda(), torch.full((1, 1), float(mu)).cuda(),
                          torch.full((1, 1), float(lv)).cuda(), 1, 0, N)
    assert tuple(got.shape) == (N, 1)
    q = (x.astype(np.float64) - float(mu)) ** 2 * np.exp(-float(lv))
    e, unit = 0.5 * (WC.LOG2PI + float(lv) + q), 0.5 * (WC.LOG2PI + abs(float(lv)) + q)
    err = float((np.abs(got.double().cpu().numpy() - e) / unit).max())
    print(f"frame_costs on {N} frames in one chunk: worst error {err:.2e} of the unit")
    assert err <= WS.BAR


def test_frame_costs_operator_and_method():
    from modules import ops
    N, K, T, F = 70, 33, 5, 65
    d = WS.plane_inputs(N, K, T, F)
    x, mu, lv = (torch.from_numpy(d[k]).cuda() for k in ("x", "mu", "lv"))
    _, want = plane_call(d, N, K, T, F, 5, 40, False)
    got = ops.frame_costs(x, mu, lv, K, 5, 40)
    assert got.dtype == torch.float32 and tuple(got.shape) == (35, K * T)
    assert torch.equal(_bits(got), _bits(want[:35]))
    wide = torch.full((N, WS.PAD_LD), NAN, device="cuda")
    wide[:, :F] = x
    assert torch.equal(_bits(ops.frame_costs(wide[:, :F], mu, lv, K, 5, 40)), _bits(got))   # a row-strided view
    for bad in ((x, mu, lv, K, 5, 5), (x, mu, lv, K, 0, N + 1), (x, mu[:-1], lv[:-1], K, 0, N), (x, mu, lv, 0, 0, N),
                (x[:, :-1], mu, lv, K, 0, N)):
        with pytest.raises(ValueError):
            ops.frame_costs(*bad)
    with pytest.raises(RuntimeError, match="forward-only|no_grad|grad"):
        ops.frame_costs(x.clone().requires_grad_(), mu, lv, K, 0, N)


# ----------------------------------------------------------------------------
# 2. the programme on given planes
# ----------------------------------------------------------------------------
class Prog:
    """The device buffers of one programme case; ``run`` makes one sequence of calls."""

    def __init__(self, d, N, K, T, pad=True):
        from modules import _native as Nt
        self.N, self.K, self.T, self.d = N, K, T, d
        self.Nt, self.lib = Nt, Nt.lib()
        S_ = K * T
        self.ldc = S_ + (5 if pad else 0)
        self.cost = torch.full((N, self.ldc), NAN, device="cuda")
        self.cost[:, :S_] = torch.from_numpy(d["cost"])
        self.v = torch.from_numpy(d["v"]).reshape(-1).cuda()
        self.ldt = K + (3 if pad else 0)
        self.trans = torch.full((K, self.ldt), NAN, device="cuda")
        self.trans[:, :K] = torch.from_numpy(d["trans"])
        self.init = torch.from_numpy(d["init"]).cuda()
        self.enter = torch.from_numpy(d["enter"]).cuda()
        self.gap = None if d["gap"] is None else torch.from_numpy(d["gap"]).cuda()
        self.nbytes = self.lib.abcd_warp_segment_workspace_bytes(N, K, T)
        assert self.nbytes > 0

    def run(self, moves, s_min, windows, want_w=True, ws=None, enter=True, gap=True):
        Nt, N, K = self.Nt, self.N, self.K
        i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")
        o = dict(ps=torch.full((2,), SENT, **f64), ns=torch.full((2,), int(SENT), **i32),
                 W=torch.full((N + 2, K), SENT, **f64) if want_w else None)
        for key in ("onset", "length", "cat", "last_state"):
            o[key] = torch.full((N + 1,), int(SENT), **i32)
        for key in ("enter", "exit", "link"):
            o[key] = torch.full((N + 1,), SENT, **f64)
        if ws is None:
            ws = torch.full((self.nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        o["ws"] = ws
        lm = (Nt.c_double * 3)(*WC.MOVES[moves])
        rcs = []
        for n0, n1 in windows:
            rcs.append(self.lib.abcd_warp_segment_window(
                Nt.ptr(self.cost[n0:]) if n0 < N else Nt.ptr(self.cost), self.ldc, n0, n1, N, K, self.T, Nt.ptr(self.v),
                lm, Nt.ptr(self.enter) if enter else None, Nt.ptr(self.gap) if gap else None, float(self.d["bonus"]),
                Nt.ptr(self.trans), self.ldt, Nt.ptr(self.init), s_min, Nt.ptr(o["ps"]), Nt.ptr(o["ns"]),
                Nt.ptr(o["onset"]), Nt.ptr(o["length"]), Nt.ptr(o["cat"]), Nt.ptr(o["last_state"]),
                Nt.ptr(o["enter"]), Nt.ptr(o["exit"]), Nt.ptr(o["link"]), Nt.ptr(o["W"]), Nt.ptr(ws), self.nbytes,
                Nt.stream()))
        torch.cuda.synchronize()
        o["rc"] = rcs
        return o


def _split(N, w):
    return [(a, min(N, a + w)) for a in range(0, N, w)]


def _same_outputs(a, b, N):
    k = int(a["ns"][0])
    if k != int(b["ns"][0]) or not torch.equal(_bits(a["ps"]), _bits(b["ps"])):
        return False
    if a["W"] is not None and b["W"] is not None and not torch.equal(_bits(a["W"]), _bits(b["W"])):
        return False
    return all(torch.equal(_bits(a[key][:k]), _bits(b[key][:k]))
               for key in ("onset", "length", "cat", "last_state", "enter", "exit", "link"))


def check_programme(N, K, T, kind):
    d = WS.prog_inputs(N, K, T, kind)
    p = Prog(d, N, K, T)
    # state_planes reads the kernel's sp planes at 32 (N + 1) K bytes: the size the header's layout gives
    assert p.nbytes == 32 * (N + 1) * K + 40 * K * T + 8 * (K + 2) + 256
    segments, worst_ulps = 0, 0.0
    for moves in WC.MOVES:
        for s_min in WS.PROG_SMIN:
            if s_min >= T:
                assert p.run(moves, s_min, [(0, N)])["rc"] == [p.Nt.ABCD_EINVAL]
                continue
            one = p.run(moves, s_min, [(0, N)])
            assert one["rc"] == [0]
            tag = (N, K, T, kind, moves, s_min)
            state = one["ws"].cpu().numpy()
            assert (state[p.nbytes:] == 0xA5).all(), tag                     # nothing behind the workspace
            cont, last = WS.state_planes(state, N, K, T)
            v64 = d["v"].astype(np.float64)
            ulps = max(WS.ulps_apart(cont, WS.softplus(v64)), WS.ulps_apart(last, WS.softplus(-v64)))
            worst_ulps = max(worst_ulps, ulps)                               # sp depends on the logits alone
            assert ulps <= WS.SP_ULPS, (tag, ulps)
            if kind == "tied":                                                # sp(+-800) is 0 or 800 in any libm
                assert ulps == 0.0
            ref = WS.prog_reference(d, moves, s_min, cont, last)
            k = int(one["ns"][0])
            assert k == len(ref["onset"]), tag
            segments += k
            assert float(one["ps"][0]) == ref["path_score"], tag
            assert float(one["ps"][1]) == SENT and int(one["ns"][1]) == int(SENT)
            assert np.array_equal(one["W"][:N + 1].cpu().numpy(), ref["W"]), tag
            assert bool((one["W"][N + 1:] == SENT).all())
            for key in ("onset", "length", "cat", "last_state"):
                assert one[key][:k].tolist() == ref[key], (tag, key)
                assert bool((one[key][k:] == int(SENT)).all()), (tag, key)
            for key in ("enter", "exit", "link"):
                assert one[key][:k].tolist() == ref[key], (tag, key)
                assert bool((one[key][k:] == SENT).all()), (tag, key)
            if kind == "nopath":
                assert k == 0 and ref["path_score"] == NEG
            for w in sorted({1, 32, N}):
                if w == N:
                    got = p.run(moves, s_min, [(0, N)], want_w=False)         # again, and without W_out
                else:
                    got = p.run(moves, s_min, _split(N, w))
                assert all(rc == 0 for rc in got["rc"])
                assert _same_outputs(got, one, N), (tag, w)
    print(f"warp_segment_window N={N} K={K} T={T} {kind}: {segments} segments; sp within {worst_ulps:.2f} ulps of "
          "numpy's")
    WS.dump(f"prog_n{N}k{K}t{T}_{kind}", [dict(N=N, K=K, T=T, kind=kind, segments=segments, sp_ulps=worst_ulps)])
    return segments


@pytest.mark.parametrize("kind", WS.PROG_KINDS)
@pytest.mark.parametrize("KT", WS.PROG_KT, ids=lambda v: f"k{v[0]}t{v[1]}")
@pytest.mark.parametrize("N", WS.PROG_N)
def test_programme_is_the_float64_loop(N, KT, kind):
    K, T = KT
    segments = check_programme(N, K, T, kind)
    if kind == "random" and N >= 33:
        assert segments > 0


def test_plan_matches_the_cases():
    """(130, 5) streams log_trans, (33, 37) and (65, 20) hold more states than the workgroup has threads."""
    from modules import _native as Nt
    import ctypes
    res, thr = Nt.c_int(-1), Nt.c_int(-1)
    for K, T in WS.PROG_KT:
        assert Nt.lib().abcd_warp_segment_plan(K, T, ctypes.byref(res), ctypes.byref(thr), None) == 0
        assert res.value == (K <= 128)
    assert any(K * T > thr.value for K, T in WS.PROG_KT) and any(K > 128 for K, _ in WS.PROG_KT)


def test_null_enter_and_null_gap():
    N, K, T = 33, 33, 37
    d = dict(WS.prog_inputs(N, K, T, "random"))
    p = Prog(d, N, K, T, pad=False)
    one = p.run("default", 0, [(0, N)], enter=False, gap=False)
    cont, last = WS.state_planes(one["ws"].cpu().numpy(), N, K, T)
    ref = WS.warpseg_reference(d["cost"], d["v"], WC.MOVES["default"], None, None, d["bonus"], d["trans"], d["init"], 0,
                               cont, last)
    k = int(one["ns"][0])
    assert k == len(ref["onset"]) > 0 and float(one["ps"][0]) == ref["path_score"]
    assert one["onset"][:k].tolist() == ref["onset"] and one["cat"][:k].tolist() == ref["cat"]
    assert sum(ref["length"]) == N                                            # no gap: the segments tile the frames
    assert np.array_equal(one["W"][:N + 1].cpu().numpy(), ref["W"])


def test_a_call_out_of_order_is_visible_and_harmless():
    N, K, T = 70, 33, 37
    d = WS.prog_inputs(N, K, T, "random")
    p = Prog(d, N, K, T)
    one = p.run("default", 0, [(0, N)])
    a = p.run("default", 0, [(0, 10)])
    assert a["rc"] == [0] and float(a["ps"][0]) == SENT                       # not the last call: nothing is written
    keep = a["ws"].clone()
    b = p.run("default", 0, [(12, 20)], ws=a["ws"])                           # 10 is due
    assert b["rc"] == [0] and math.isnan(float(b["ps"][0])) and int(b["ns"][0]) == -1
    assert torch.equal(b["ws"], keep)                                         # the carry is as it was
    assert bool((b["W"] == SENT).all())
    c = p.run("default", 0, [(10, 40), (40, N)], ws=a["ws"])
    assert c["rc"] == [0, 0]
    c["W"][:11] = a["W"][:11]                                                 # rows 0 .. 10 were the first call's
    assert _same_outputs(c, one, N)
    # a fresh start on a used workspace
    again = p.run("default", 0, [(0, N)], ws=a["ws"])
    assert _same_outputs(again, one, N)


def test_empty_recording():
    from modules import _native as Nt
    lib = Nt.lib()
    K, T = 5, 3
    nb = lib.abcd_warp_segment_workspace_bytes(0, K, T)
    ws = Nt.workspace(nb, "cuda")
    ps = torch.full((1,), SENT, dtype=torch.float64, device="cuda")
    ns = torch.full((1,), int(SENT), dtype=torch.int32, device="cuda")
    W = torch.full((2, K), SENT, dtype=torch.float64, device="cuda")
    lm = (Nt.c_double * 3)(*WC.MOVES["default"])
    rc = lib.abcd_warp_segment_window(None, K * T, 0, 0, 0, K, T, None, lm, None, None, 0.0, None, K, None, 0,
                                      Nt.ptr(ps), Nt.ptr(ns), None, None, None, None, None, None, None, Nt.ptr(W),
                                      Nt.ptr(ws), nb, Nt.stream())
    torch.cuda.synchronize()
    assert rc == 0 and float(ps[0]) == 0.0 and int(ns[0]) == 0
    assert bool((W[0] == NEG).all()) and bool((W[1] == SENT).all())


def test_window_operator():
    from modules import ops
    N, K, T = 70, 33, 37
    d = WS.prog_inputs(N, K, T, "random")
    p = Prog(d, N, K, T, pad=False)
    one = p.run("default", 2, [(0, N)])
    k = int(one["ns"][0])
    cost = torch.from_numpy(d["cost"]).cuda()
    state = ops.warp_segment_state(N, K, T, "cuda")
    W = torch.full((N + 1, K), SENT, dtype=torch.float64, device="cuda")
    args = (K, p.v, list(WC.MOVES["default"]), p.enter, p.gap, d["bonus"], p.trans[:, :K], p.init, 2, state, W)
    first = ops.warp_segment_window(cost[:32], 0, 32, N, *args)
    assert math.isnan(float(first[0])) and int(first[1]) == -1
    out = ops.warp_segment_window(cost[32:], 32, N, N, *args)
    assert float(out[0]) == float(one["ps"][0]) and int(out[1]) == k
    for got, key in zip(out[2:], ("onset", "length", "cat", "last_state", "enter", "exit", "link")):
        assert tuple(got.shape) == (N,) and torch.equal(_bits(got[:k]), _bits(one[key][:k])), key
    assert torch.equal(_bits(W), _bits(one["W"][:N + 1]))
    for bad in (dict(n0=5, n1=5), dict(s_min=T), dict(moves=[NEG, NEG, NEG]), dict(state=state[:100])):
        a = dict(n0=0, n1=N, s_min=0, moves=list(WC.MOVES["default"]), state=state)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.warp_segment_window(cost, a["n0"], a["n1"], N, K, p.v, a["moves"], None, None, 0.0, p.trans[:, :K],
                                    p.init, a["s_min"], a["state"], None)


# ----------------------------------------------------------------------------
# 3. segment_frames_warped on the small models
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.E2E_SMALL))
def test_step_only_is_segment_frames_under_the_chain(name):
    from modules import ops, segmentation
    from modules.sequence import TransitionModel
    dec, protos, frames, K, D = _small_recording(name)
    model = TransitionModel.from_log_weight(torch.linspace(-1.0, 1.0, K).cuda())
    tiled = segmentation.segment_frames(dec, protos, frames, D, transitions=model)
    per_frame = float(tiled["path_score"]) / frames.shape[0]
    const = torch.full((frames.shape[0],), per_frame, device="cuda")
    rels, segments = [], 0
    for gap, bonus, s_min in ((None, 0.0, 0), (None, -3.0, 1), (const, 0.0, 0), (const, -3.0, 1)):
        rigid = segmentation.segment_frames(dec, protos, frames, D, min_length=s_min + 1, gap=gap, seg_bonus=bonus,
                                            transitions=model)
        outs = [segmentation.segment_frames_warped(dec, protos, frames, D, log_moves=ops.IDENTITY_LOG_MOVES,
                                                   transitions=model, gap=gap, seg_bonus=bonus, min_state=s_min,
                                                   chunk_frames=c) for c in (None, 7)]
        out = outs[0]
        for key in ("onset", "length", "category"):
            assert out[key].tolist() == rigid[key].tolist(), (name, key)
        segments += len(out["onset"])
        assert out["last_state"].tolist() == (out["length"] - 1).tolist() and bool((out["tempo"] == 1.0).all())
        assert out["link"].tolist() == rigid["link"].tolist()
        if len(out["onset"]) == 0 and gap is None:                            # no cover under either programme
            assert float(out["path_score"]) == float(rigid["path_score"]) == NEG
            continue
        rel = abs(float(out["path_score"]) - float(rigid["path_score"])) / abs(float(rigid["path_score"]))
        rels.append(rel)
        assert rel <= 1e-9
        assert torch.allclose(out["score"], rigid["score"], rtol=1e-9, atol=0.0)
        for key in out:                                                       # the chunks change no bit
            assert torch.equal(outs[1][key], out[key]), (name, key)
    assert segments > 0
    print(f"{name}: step-only warped programme against segment_frames(transitions): path score relative difference "
          f"{max(rels):.1e}")
    WS.dump(f"e2e_rigid_{name}", [dict(case=name, rigid=max(rels))])


@pytest.mark.parametrize("name", list(S.E2E_SMALL))
def test_segment_scores_are_the_warped_nll_of_the_cut_segments(name):
    from modules import ops, segmentation
    dec, protos, frames, K, D = _small_recording(name)
    lw = torch.log_softmax(torch.linspace(-1.0, 1.0, K), 0).cuda()
    lm = ops.DEFAULT_LOG_MOVES
    out = segmentation.segment_frames_warped(dec, protos, frames, D, log_moves=lm, log_weight=lw)
    n = len(out["onset"])
    assert n > 0 and int(out["length"].sum()) == frames.shape[0]
    assert torch.allclose(out["tempo"], (out["last_state"] + 1).double() / out["length"].double())
    mu, lv, offl = (t[:D].float().cpu() for t in protos)
    worst = 0.0
    for i in range(n):
        o, d, k = int(out["onset"][i]), int(out["length"][i]), int(out["category"][i])
        seg = frames[o:o + d]
        bs = torch.ones(d, dtype=torch.int64)
        y = torch.zeros(d)
        y[-1] = 1.0
        protos_d = tuple(t[:D] for t in protos)
        warp = dec.warp_against(protos_d, bs, seg, None, log_moves=lm)
        ref = WC.warp_reference(bs.numpy(), seg.cpu(), mu, lv, offl, y, lm)
        unit = float(ref["A"][0, k]) + abs(float(lw[k]))
        err = abs(float(out["score"][i]) - (float(lw[k]) - float(warp[0, k]))) / unit
        worst = max(worst, err)
        assert err <= WC.BAR, (name, i, err)
        assert int(out["last_state"][i]) == int(ref["paths"][(0, k)][-1])
    print(f"{name}: {n} segments, score against log_enter - warp_nll: worst {worst:.2e} of the unit (bar {WC.BAR})")
    WS.dump(f"e2e_score_{name}", [dict(case=name, score=worst)])


# ----------------------------------------------------------------------------
# 4. the planted recording
# ----------------------------------------------------------------------------
def test_planted_recording_on_the_device():
    from modules import ops
    d = WS.planted()
    N, K, T = d["N"], d["K"], d["T"]
    x, mu, lv = (torch.from_numpy(d[k]).cuda() for k in ("x", "mu", "lv"))
    v = torch.from_numpy(d["v"]).reshape(-1).cuda()
    trans, init = torch.from_numpy(d["trans"]).cuda(), torch.from_numpy(d["init"]).cuda()
    state = ops.warp_segment_state(N, K, T, "cuda")
    out = None
    for n0 in range(0, N, 32):
        n1 = min(N, n0 + 32)
        out = ops.warp_segment_window(ops.frame_costs(x, mu, lv, K, n0, n1), n0, n1, N, K, v, list(WS.PLANT_MOVES), None,
                                      None, 0.0, trans, init, 0, state, None)
    k = int(out[1])
    assert out[2][:k].tolist() == d["onset"] and out[3][:k].tolist() == d["length"] and out[4][:k].tolist() == d["cat"]
    assert out[5][:k].tolist() == [T - 1] * k
    want, rigid_ref = WS.planted_references()
    assert abs(float(out[0]) - want["path_score"]) <= 1e-6 * abs(want["path_score"])
    table, _, _ = ops.span_table(x, mu, lv, v, None, K, T, False)
    r = ops.span_chain_viterbi(table, 1, None, 0.0, trans, init, False)
    kr = int(r[1])
    rigid = (r[2][:kr].tolist(), r[3][:kr].tolist(), r[4][:kr].tolist())
    assert rigid != (d["onset"], d["length"], d["cat"])
    assert rigid == (rigid_ref["onset"], rigid_ref["length"], rigid_ref["cat"])
    assert float(out[0]) > float(r[0])
    print(f"planted: the warped programme recovers {k} segments of {d['length']} frames; the rigid one cuts {kr}")


# ----------------------------------------------------------------------------
# 5. segment.py --warp on the toy data
# ----------------------------------------------------------------------------
def test_segment_cli_with_warp(tmp_path):
    import segment
    from modules import alignment
    base = [CKPT, TOY, ANN, "1.0", "--max_length", "60", "--min_length", "3"]
    out = os.path.join(str(tmp_path), "w", "segmented.csv")
    assert segment.main(base + ["-S", out, "--warp", "--moves", "0.25", "0.5", "0.25", "--chunk_frames", "50"]) == out
    df = pd.read_csv(out)
    assert list(df.columns) == list(segment.COLUMNS) + list(segment.WARP_COLUMNS)
    seg = segment.Segmenter(CKPT, device="cuda")
    ann = pd.read_csv(ANN)
    wav = ann["input_path"][0]
    fs, wave = segment.read_wave(TOY, wav)
    a = segment.get_parameters(base + ["--warp"])
    frame, hop = segment.cli.frame_hop(a, fs)
    frames = segment.cli.log_spectrum(a, frame, hop)(torch.from_numpy(wave)).to(seg.device)
    lw = seg.log_weight(a.prior, len(ann))
    d_min = max(3, segment.min_loadable_length(frame, hop, True))
    got = seg.segment_recording_warped(frames, 60, alignment.moves_from_probabilities([0.25, 0.5, 0.25]),
                                       min_state=2 * (d_min - 1), log_weight=lw)
    first = ann.iloc[0]
    rows = segment.segment_rows(wav, got["onset"].tolist(), got["length"].tolist(), got["category"].tolist(),
                                got["score"].tolist(), fs, frame, hop, True, len(wave), data_type=first["data_type"],
                                speaker=first["speaker"], warp=(got["last_state"].tolist(), got["tempo"].tolist(), None))
    want = os.path.join(str(tmp_path), "want.csv")
    pd.DataFrame(rows, columns=list(segment.COLUMNS) + list(segment.WARP_COLUMNS)).to_csv(want, index=False)
    sub = df[df["input_path"] == wav]
    assert len(sub) == len(rows) >= 1
    pd.testing.assert_frame_equal(sub.reset_index(drop=True), pd.read_csv(want), check_exact=True)
    # a table the other tools read: every segment has the frames the loader needs
    assert (df["length"] >= d_min).all() and (df["last_state"] >= 2 * (d_min - 1)).all()
    assert np.allclose(df["tempo"], (df["last_state"] + 1) / df["length"])
    print(f"segment.py --warp: {len(df)} segments, tempo {df['tempo'].min():.2f} .. {df['tempo'].max():.2f}")
    with pytest.raises(SystemExit):
        segment.main(base + ["-S", out, "--warp", "--posteriors"])
