"""The GEMM layer's kernels that ``gemm()`` does not dispatch, at their edges,
inside guarded buffers, against float64 torch: ``gemm_wg3b`` / ``gemm_wg2`` and
the split fallback behind ``abcd_lstm_wgrad``; the fused offset head's two
passes (``x6r8<8,64,offset_fwd>`` + ``dec_offset_logit``, ``x6r8<8,64,offset_bwd>``)
through ``abcd_debug_offset_head_fwd`` / ``_bwd``; ``gemm_tn_batch`` (quiet and
side mode) and ``colsum_batch`` through ``abcd_debug_gemm_tn_batch`` /
``abcd_debug_colsum_batch``.

tests/wgrad_cases.py holds the tables, the data, the references and the bars
(and the launch arithmetic the shapes were chosen from; its CPU twin asserts
it).  Every test asserts the kernel that ran (dispatch record or route string)
before it compares values, checks ``abcd_device_status() == 0``, prints its
figures and keeps them under ``ABCD_PARITY_DUMP`` (profiles/gemm_errors.json).

``colsum_batch`` has one form and records no dispatch: nothing to assert there.

Not reached: the wg forms' ``K * 4H * 4 >= 2 GiB`` guard and the offset head's
declines on operands of 2 GiB or more (2 GiB operands); ``gemm_offset_bwd``'s
decline where a row range's LDS request passes 160 KiB (more than 7424 rows
per range: M above 118784 at 16 slices, a 0.5 GB DHO).
bce / dlog_raw are compared with float64 of the kernel's own fp32 logit, not of
the float64 logit: the logit carries its own bar, and these two the error of
the fp32 exp / log1p / divide alone."""
import ctypes

import pytest
import torch

import gemm_cases as G
import wgrad_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nn():
    from modules import _native as Nn
    return Nn


def _status_ok():
    assert _nn().lib().abcd_device_status() == 0


def _sync(rc=0):
    """Wait for the call.  A HIP error (anything but 0 / ABCD_EINVAL / hipErrorInvalidValue from a host-side check)
    or a failed synchronisation ends the whole session: nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, stopping: {e}", 3)
    if rc not in (0, 1, G.EINVAL):
        pytest.exit(f"HIP error {rc}, stopping", 3)


# ----------------------------------------------------------------------------
# 1. abcd_lstm_wgrad
# ----------------------------------------------------------------------------
def _wg_call(c, data, ws_fill=0xFF):
    """One call on fresh guarded buffers: (rc, dispatch name, gemm route, buffers)."""
    Nn = _nn()
    lib = Nn.lib()
    nd, F, H, K = c["nd"], c["F"], c["H"], c["K"]
    b = W.wg_buffers(c, data, DEV)
    nbytes = lib.abcd_lstm_wgrad_workspace_bytes(nd, F, H, K)
    assert nbytes == 4 * W.wgrad_workspace_floats(nd, F, H, K)[0] + 256
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device=DEV)
    arr = lambda gs: (ctypes.c_void_p * nd)(*[g.ptr() for g in gs])
    keep = [arr(b[k]) for k in ("dG", "Hp", "w_ih", "b_ih", "b_hh", "w_hh")]
    lib.abcd_dispatch_reset()
    rc = lib.abcd_lstm_wgrad(nd, F, H, K, keep[0], b["X"].ptr(), c["ldx"], keep[1], keep[2], keep[3],
                             None if c["bhh_null"] else keep[4], keep[5], Nn.ptr(ws), nbytes, Nn.stream())
    route = lib.abcd_debug_gemm_route().decode()
    _sync(rc)
    return rc, Nn.dispatch()["enc_wgrad"][0], route, b


@pytest.mark.parametrize("name", list(W.WG_CASES))
def test_lstm_wgrad(name, monkeypatch):
    c = W.WG_CASES[name]
    monkeypatch.delenv("ABCD_WG2", raising=False)
    monkeypatch.delenv("ABCD_WG3", raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    rows = dict(entry="lstm_wgrad", case=name, form=c["form"], nd=c["nd"], F=c["F"], H=c["H"], K=c["K"], route=None,
                kinds={})
    problems = []
    for kind in G.KINDS:
        data = W.wg_data(name, kind)
        rc, disp, route, b = _wg_call(c, data)
        assert rc == 0 and disp == c["route"], f"{name}: rc {rc}, ran {disp!r}, the case is for {c['route']!r}"
        rows["route"] = disp
        # a fallback's max-norm bar: only the product whose route the library names (the last: w_hh) and only on x6
        mx = ("w_ih", "b_ih", "w_hh") if c["form"] != "split" else (("w_hh",) if route.startswith("x6") else ())
        fig, fails = W.wg_check(c, kind, data, b, mx)
        if c["form"] == "split":
            fig["gemm_route"] = route
        if kind == "a":
            _, _, _, b2 = _wg_call(c, data, ws_fill=0x00)
            same = all(torch.equal(b[k][d].view, b2[k][d].view) for k in ("w_ih", "b_ih", "w_hh")
                       for d in range(c["nd"]))
            fig["repeatable"] = same
            if not same:
                fails.append("repeat")
        print(name, kind, disp, fig)
        rows["kinds"][kind] = dict(fig, fails=fails)
        problems += [f"{kind}:{f}" for f in fails]
    _status_ok()
    W.dump("wgrad_" + name, rows)
    assert not problems, (name, problems)


@pytest.mark.parametrize("form", ["wg3b", "wg2"])
def test_lstm_wgrad_bhh_null_changes_nothing_else(form, monkeypatch):
    """b_hh = NULL: w_ih, b_ih and w_hh are those of the non-NULL call bit for bit."""
    monkeypatch.delenv("ABCD_WG2", raising=False)
    c0, c1 = W.WG_CASES[f"{form}_nd2_k193"], W.WG_CASES[f"{form}_bhh_null"]
    monkeypatch.setenv("ABCD_WG3", c0["env"]["ABCD_WG3"])
    data = W.wg_data(c0["name"], "a")
    rc0, d0, _, b0 = _wg_call(c0, data)
    rc1, d1, _, b1 = _wg_call(c1, data)
    assert rc0 == 0 and rc1 == 0 and d0 == d1 == c0["route"]
    for k in ("w_ih", "b_ih", "w_hh"):
        for d in range(2):
            assert torch.equal(b0[k][d].view, b1[k][d].view), (k, d)
    for d in range(2):
        assert bool(torch.isnan(b1["b_hh"][d].view).all()) and b1["b_hh"][d].guard_intact()
    _status_ok()


@pytest.mark.parametrize("form", ["wg3b", "split"])
def test_lstm_wgrad_no_frames(form, monkeypatch):
    """K = 0: returns 0 and writes nothing."""
    monkeypatch.delenv("ABCD_WG2", raising=False)
    monkeypatch.delenv("ABCD_WG3", raising=False)
    c = dict(W.WG_CASES["wg3b_nd2_k1" if form == "wg3b" else "split_h48_f33_k193"], K=0)
    H, F = c["H"], c["F"]
    data = dict(dG=[torch.zeros(0, 4 * H)] * 2, X=torch.zeros(0, F), Hp=[torch.zeros(0, H)] * 2)
    rc, _, _, b = _wg_call(c, data)
    assert rc == 0
    for k in W.WG_OUTS:
        for g in b[k]:
            assert bool(torch.isnan(g.view).all()) and g.guard_intact(), k
    _status_ok()


# ----------------------------------------------------------------------------
# 2. the fused offset head
# ----------------------------------------------------------------------------
def _off_fwd_call(c, d):
    Nn = _nn()
    lib = Nn.lib()
    b = W.off_fwd_buffers(c, d, DEV)
    fused = ctypes.c_int(-1)
    rc = lib.abcd_debug_offset_head_fwd(c["M"], c["N"], c["K"], b["Hs"].ptr(), c["K"] + 4, b["W1o"].ptr(),
                                        b["b1o"].ptr(), b["w2"].ptr(), b["b2"].ptr(),
                                        b["tgt"].ptr() if c["tgt"] else None, b["Zo"].ptr(), b["part"].ptr(),
                                        b["logit"].ptr(), b["dlog_raw"].ptr(), b["bce"].ptr(), ctypes.byref(fused),
                                        Nn.stream())
    route = lib.abcd_debug_gemm_route().decode()
    _sync(rc)
    return rc, fused.value, route, b


@pytest.mark.parametrize("name", list(W.OFF_FWD_CASES))
def test_offset_head_forward(name):
    c = W.OFF_FWD_CASES[name]
    rows = dict(entry="offset_head_fwd", case=name, M=c["M"], N=c["N"], K=c["K"], grid=W.x6r8_grid(c["M"], c["N"]),
                route=None, kinds={})
    problems = []
    for kind in G.KINDS:
        d = W.off_fwd_data(name, kind)
        rc, fused, route, b = _off_fwd_call(c, d)
        assert rc == 0 and fused == 1 and route == "x6r8<8,64,offset_fwd>", (name, rc, fused, route)
        rows["route"] = route
        fig, fails = W.off_fwd_check(c, kind, d, b)
        if kind == "a":
            _, _, _, b2 = _off_fwd_call(c, d)
            fig["repeatable"] = all(torch.equal(b[k].view, b2[k].view) for k in ("Zo", "part", "logit"))
            if not fig["repeatable"]:
                fails.append("repeat")
        print(name, kind, route, fig)
        rows["kinds"][kind] = dict(fig, fails=fails)
        problems += [f"{kind}:{f}" for f in fails]
    _status_ok()
    W.dump("offfwd_" + name, rows)
    assert not problems, (name, problems)


@pytest.mark.parametrize("name", list(W.OFF_FWD_DECLINES))
def test_offset_head_forward_declines(name):
    c = W.OFF_FWD_DECLINES[name]
    rc, fused, _, b = _off_fwd_call(c, W.off_fwd_data(name, "a"))
    assert rc == 0 and fused == 0
    for k in ("Zo", "part", "logit", "dlog_raw", "bce"):
        assert bool(torch.isnan(b[k].view).all()) and b[k].guard_intact(), k
    _status_ok()


def _off_bwd_call(c, d):
    Nn = _nn()
    lib = Nn.lib()
    b = W.off_bwd_buffers(c, d, DEV)
    fused = ctypes.c_int(-1)
    rc = lib.abcd_debug_offset_head_bwd(c["M"], c["N"], c["K"], b["Zo"].ptr(), b["W1oT"].ptr(), b["w2"].ptr(),
                                        b["dlog_raw"].ptr(), b["s"].ptr(), b["DHO"].ptr(), b["dZo"].ptr(),
                                        b["dlog_s"].ptr(), ctypes.byref(fused), Nn.stream())
    route = lib.abcd_debug_gemm_route().decode()
    _sync(rc)
    return rc, fused.value, route, b


@pytest.mark.parametrize("name", list(W.OFF_BWD_CASES))
def test_offset_head_backward(name):
    c = W.OFF_BWD_CASES[name]
    rows = dict(entry="offset_head_bwd", case=name, M=c["M"], N=c["N"], K=c["K"], grid=W.x6r8_grid(c["M"], c["N"]),
                route=None, kinds={})
    problems = []
    for kind in W.BWD_KINDS:
        d = W.off_bwd_data(name, kind)
        rc, fused, route, b = _off_bwd_call(c, d)
        assert rc == 0 and fused == 1 and route == "x6r8<8,64,offset_bwd>", (name, rc, fused, route)
        rows["route"] = route
        fig, fails = W.off_bwd_check(c, kind, d, b)
        if kind == "a":
            _, _, _, b2 = _off_bwd_call(c, d)
            fig["repeatable"] = all(torch.equal(b[k].view, b2[k].view) for k in ("DHO", "dZo", "dlog_s"))
            if not fig["repeatable"]:
                fails.append("repeat")
        print(name, kind, route, fig)
        rows["kinds"][kind] = dict(fig, fails=fails)
        problems += [f"{kind}:{f}" for f in fails]
    _status_ok()
    W.dump("offbwd_" + name, rows)
    assert not problems, (name, problems)


@pytest.mark.parametrize("name", list(W.OFF_BWD_DECLINES))
def test_offset_head_backward_declines(name):
    c = W.OFF_BWD_DECLINES[name]
    rc, fused, _, b = _off_bwd_call(c, W.off_bwd_data(name, "a"))
    assert rc == 0 and fused == 0
    for k in ("DHO", "dZo", "dlog_s"):
        assert bool(torch.isnan(b[k].view).all()) and b[k].guard_intact(), k
    _status_ok()


# ----------------------------------------------------------------------------
# 3. gemm_tn_batch, colsum_batch
# ----------------------------------------------------------------------------
def _tn_call(jobs, bufs, side, n=None):
    Nn = _nn()
    lib = Nn.lib()
    n = len(jobs) if n is None else n
    jj = (list(jobs) + [jobs[0]] * n)[:n]
    bb = (list(bufs) + [bufs[0]] * n)[:n]
    vp = lambda k: (ctypes.c_void_p * n)(*[b[k].ptr() for b in bb])
    lg = lambda v: (ctypes.c_long * n)(*v)
    it = lambda v: (ctypes.c_int * n)(*v)
    fl = lambda v: (ctypes.c_float * n)(*v)
    args = [vp("A"), lg([j[0] + 4 for j in jj]), vp("B"), lg([j[1] + 4 for j in jj]), vp("C"),
            lg([b["C"].view.stride(0) for b in bb]), it([j[0] for j in jj]), it([j[1] for j in jj]),
            it([j[2] for j in jj]), fl([j[3] for j in jj]), fl([j[4] for j in jj])]
    # a 1 x 1 x 16 product first, so that the route read after the batch is this call's and not an earlier one's
    one = torch.ones(3, 16, device=DEV)
    assert lib.abcd_gemm_nt(1, 1, 16, Nn.ptr(one[0]), 16, Nn.ptr(one[1]), 16, Nn.ptr(one[2]), 1, None, None, 0,
                            Nn.stream()) == 0 and lib.abcd_debug_gemm_route().decode() == "ks z=1"
    lib.abcd_debug_gemm_side(1 if side else 0)
    try:
        rc = lib.abcd_debug_gemm_tn_batch(n, *args, Nn.stream())
        route = lib.abcd_debug_gemm_route().decode()
    finally:
        lib.abcd_debug_gemm_side(0)
    _sync(rc)
    return rc, route


@pytest.mark.parametrize("side", [False, True], ids=["quiet_1_1_64", "side_2_2_16"])
@pytest.mark.parametrize("batch", ["eight", "one"])
def test_gemm_tn_batch(batch, side):
    jobs = W.TN_JOBS if batch == "eight" else W.TN_JOBS_ONE
    want = "tn_batch<2,2,16>" if side else "tn_batch<1,1,64>"   # what the launcher says it started
    rows = dict(entry="tn_batch", case=f"{batch}/{'side' if side else 'quiet'}", route=None, jobs=list(jobs), kinds={})
    problems = []
    for kind in G.KINDS:
        data = W.tn_data(batch, kind)
        bufs = W.tn_buffers(jobs, data, DEV)
        rc, route = _tn_call(jobs, bufs, side)
        assert rc == 0 and route == want, f"rc {rc}, ran {route!r}, the case is for {want!r}"
        rows["route"] = route
        fig, fails = W.tn_check(jobs, kind, data, bufs)
        if kind == "a":
            bufs2 = W.tn_buffers(jobs, data, DEV)
            assert _tn_call(jobs, bufs2, side) == (0, want)
            if not all(torch.equal(x["C"].flat.view(torch.int32), y["C"].flat.view(torch.int32))
                       for x, y in zip(bufs, bufs2)):
                fails.append("repeat")
        print(batch, side, kind, fig)
        rows["kinds"][kind] = dict(fig, fails=fails)
        problems += [f"{kind}:{f}" for f in fails]
    _status_ok()
    W.dump(f"tnbatch_{batch}_{'side' if side else 'quiet'}", rows)
    assert not problems, problems


@pytest.mark.parametrize("how", ["nine_jobs", "m_not_multiple_of_4"])
def test_gemm_tn_batch_refuses(how):
    """An error before any launch: nothing is written."""
    jobs = list(W.TN_JOBS)
    if how != "nine_jobs":
        jobs[1] = (30, 36, 16, 1.0, 0.0)
    data = W.tn_data("eight", "a")
    if how != "nine_jobs":
        data = [dict(d) for d in data]
        data[1] = dict(A=data[1]["A"][:30], B=data[1]["B"], C0=None)
    bufs = W.tn_buffers(jobs, data, DEV)
    before = [b["C"].flat.view(torch.int32).clone() for b in bufs]
    rc, route = _tn_call(jobs, bufs, False, n=9 if how == "nine_jobs" else None)
    assert rc != 0 and (how == "nine_jobs" or rc == G.EINVAL), rc
    assert route == "ks z=1", route   # nothing was launched: the route is still the product's before it
    for b, x in zip(bufs, before):
        assert torch.equal(b["C"].flat.view(torch.int32), x)
    _status_ok()


def _cs_call(jobs, bufs, scratch_floats):
    Nn = _nn()
    lib = Nn.lib()
    n = len(jobs)
    vp = lambda k: (ctypes.c_void_p * n)(*[b[k].ptr() if b[k] is not None else None for b in bufs])
    scratch = torch.full((max(scratch_floats, 1) + 64,), float("nan"), device=DEV)
    rc = lib.abcd_debug_colsum_batch(n, vp("Z"), (ctypes.c_long * n)(*[j[1] + 3 for j in jobs]),
                                     (ctypes.c_int * n)(*[j[0] for j in jobs]), (ctypes.c_int * n)(*[j[1] for j in jobs]),
                                     vp("w"), vp("out"), (ctypes.c_float * n)(*[j[4] for j in jobs]), vp("out2"),
                                     Nn.ptr(scratch), scratch_floats, Nn.stream())
    _sync(rc)
    assert bool(torch.isnan(scratch[scratch_floats:]).all()), "partials written past the scratch"
    return rc


def test_colsum_batch():
    """The eight jobs in one batch inside their bars, and each bit-identical to
    the same job run alone through the batch entry."""
    jobs, data = W.CS_JOBS, W.cs_data()
    bufs = W.cs_buffers(jobs, data, DEV)
    assert _cs_call(jobs, bufs, W.CS_AMPLE) == 0
    fig, fails = W.cs_check(jobs, data, bufs)
    for i, j in enumerate(jobs):
        alone = W.cs_buffers([j], [data[i]], DEV)
        assert _cs_call([j], alone, W.CS_AMPLE) == 0
        for k in ("out", "out2"):
            if bufs[i][k] is not None and not torch.equal(alone[0][k].view, bufs[i][k].view):
                fails.append(f"job{i}:{k} differs from the job alone")
    print(fig)
    _status_ok()
    W.dump("colsum_batch", dict(entry="colsum_batch", case="ample", jobs=list(jobs), figures=fig, fails=fails))
    assert not fails, fails


def test_colsum_batch_scratch_clamps_last_job():
    jobs, data = W.CS_JOBS[:6], W.cs_data()[:6]   # the last: 4097 x 1029
    full = W.colsum_slicing(jobs, W.CS_AMPLE)
    floats = full[-1][2] + jobs[-1][1]
    sl = W.colsum_slicing(jobs, floats)
    assert full[-1][0] > 1 and sl[-1][0] == 1 and sl[:-1] == full[:-1]
    bufs = W.cs_buffers(jobs, data, DEV)
    assert _cs_call(jobs, bufs, floats) == 0
    fig, fails = W.cs_check(jobs, data, bufs)
    print(fig)
    _status_ok()
    W.dump("colsum_batch_clamped", dict(entry="colsum_batch", case="clamped", jobs=list(jobs), figures=fig, fails=fails))
    assert not fails, fails


def test_colsum_batch_refuses_short_scratch():
    jobs, data = W.CS_JOBS[:6], W.cs_data()[:6]
    floats = W.colsum_slicing(jobs, W.CS_AMPLE)[-1][2] + jobs[-1][1] - 1
    assert W.colsum_slicing(jobs, floats) is None
    bufs = W.cs_buffers(jobs, data, DEV)
    before = [[b[k].flat.view(torch.int32).clone() for k in ("out", "out2") if b[k] is not None] for b in bufs]
    assert _cs_call(jobs, bufs, floats) != 0
    for b, x in zip(bufs, before):
        now = [b[k].flat.view(torch.int32) for k in ("out", "out2") if b[k] is not None]
        assert all(torch.equal(p, q) for p, q in zip(now, x))
    _status_ok()
