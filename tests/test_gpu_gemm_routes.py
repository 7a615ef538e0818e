"""Every route of the GEMM dispatcher (csrc/abcd_gemm.hip, ``gemm()``) at its
edges, inside guarded buffers, against float64 torch.

tests/gemm_cases.py holds the case tables, the buffers (operands inside NaN,
``C`` inside a sentinel pattern), the three kinds of data and the bars.  Each
case first asserts ``abcd_debug_gemm_route()``: a case that drifts to another
kernel fails instead of passing vacuously.  Then, for every data kind: the
return code, the guard band (bit-identical to the sentinel outside ``C``'s
``M x N``), finiteness (no padding NaN reached an output), the kind's bars, and
for the random data a second call with ``torch.equal`` output (no atomics).
Side-mode cases switch ``abcd_debug_gemm_side`` on and, in a ``finally``, off.
Every observed figure is kept with ``ABCD_PARITY_DUMP``
(profiles/gemm_errors.json, assembled by gemm_cases.assemble).

Not reached here (operands >= 2 GiB): ``gemm_x6s<4,4,kc,kc>`` and the
non-buffer fallback of the K-major path (``x6s<4,4>``).  gemm_wg2 / gemm_wg3b,
the offset-head modes of gemm_x6r8, gemm_tn_batch and colsum_batch are pinned
the same way by tests/test_gpu_wgrad_offset.py (tables: tests/wgrad_cases.py)."""
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nn():
    from modules import _native as Nn
    return Nn


def _ws(c, Nn, extra_floats=0):
    """(pointer or None, bytes, tensor): "std" = room for the packed copies and up to 64 slabs (16 MB at most)."""
    M, N, K = c["M"], c["N"], c["K"]
    if c["ws"] is None:
        return None, 0, None
    pack = (M + N) * ((K + 15) // 16 * 16)
    floats = c["ws"] if c["ws"] != "std" else pack + min(64 * M * N, 4 << 20) + 1024
    t = Nn.workspace(max(4 * (floats + extra_floats), 16), DEV)
    return Nn.ptr(t), 4 * floats, t


def _call(entry, c, d):
    """One library call on fresh guarded buffers: (rc, route, C Guarded)."""
    Nn = _nn()
    lib = Nn.lib()
    M, N, K = c["M"], c["N"], c["K"]
    A, B = d["A"], d["B"]
    if entry == "tn":
        Ag, Bg = G.operand(A.t().contiguous(), c["lda"], DEV), G.operand(B.t().contiguous(), c["ldb"], DEV)
    else:
        Ag, Bg = G.operand(A, c["lda"], DEV, c["a_off"]), G.operand(B, c["ldb"], DEV)
    Cg = G.Guarded(M, N, c["ldc"], DEV, "sentinel", c.get("c_off", 0))
    bg = G.operand(d["bias"][None, :], N, DEV) if d["bias"] is not None else None
    wp, wbytes, wt = _ws(c, Nn)
    lib.abcd_debug_gemm_side(1 if c["side"] else 0)
    try:
        if entry == "nt":
            rc = lib.abcd_gemm_nt(M, N, K, Ag.ptr(), c["lda"], Bg.ptr(), c["ldb"], Cg.ptr(), c["ldc"],
                                  bg.ptr() if bg else None, wp, wbytes, Nn.stream())
        elif entry == "tn":
            rc = lib.abcd_gemm_tn(M, N, K, Ag.ptr(), c["lda"], Bg.ptr(), c["ldb"], Cg.ptr(), c["ldc"], wp, wbytes,
                                  Nn.stream())
        else:
            rc = lib.abcd_linear(M, N, K, Ag.ptr(), c["lda"], Bg.ptr(), c["ldb"], bg.ptr() if bg else None, c["act"],
                                 Cg.ptr(), c["ldc"], wp, wbytes, Nn.stream())
        route = lib.abcd_debug_gemm_route().decode()
    finally:
        lib.abcd_debug_gemm_side(0)
    torch.cuda.synchronize()
    return rc, route, Cg


def _run_case(entry, table, name):
    c = table[name]
    act = c.get("act", 0)
    rows = dict(entry=entry, case=name, M=c["M"], N=c["N"], K=c["K"], side=c["side"], route=None, kinds={})
    problems = []
    for kind in G.KINDS:
        d = G.case_data({"nt": "nt", "tn": "tn", "linear": "linear"}[entry], name, kind)
        rc, route, Cg = _call(entry, c, d)
        if kind == "a":   # the route first: nothing below means anything on another kernel
            assert rc == c["rc"], (name, rc)
            if c["rc"] != 0:
                assert Cg.guard_intact() and bool(torch.isnan(Cg.view).all()), f"{name}: a refused call wrote"
                G.dump(f"{entry}_{name}", rows)
                return
            assert route == c["route"], f"{name}: ran {route!r}, the case is for {c['route']!r}"
            rows["route"] = route
        assert rc == 0 and route == c["route"], (name, kind, rc, route)
        Ad, Bd = d["A"].to(DEV), d["B"].to(DEV)
        bd = d["bias"].to(DEV) if d["bias"] is not None else None
        rf = G.reference(Ad, Bd, bd, unit=kind == "a")
        e32 = None
        if kind == "a" and c["x6"]:
            z32 = Ad @ Bd.t() + (bd if bd is not None else 0.0)
            e32 = G.max_norm_err(torch.tanh(z32) if act == 1 else z32, torch.tanh(rf["ref"]) if act == 1 else rf["ref"])
        C = Cg.view.contiguous()
        fig = G.check(kind, C, rf, c["K"], act, e32)
        fig["guard_intact"] = Cg.guard_intact()
        if not fig["guard_intact"]:
            fig["fails"].append("guard")
        if kind == "a":
            _, _, Cg2 = _call(entry, c, d)
            fig["repeatable"] = bool(torch.equal(C, Cg2.view.contiguous()))
            if not fig["repeatable"]:
                fig["fails"].append("repeat")
        print(name, kind, route, fig)
        rows["kinds"][kind] = fig
        problems += [f"{kind}:{f}" for f in fig["fails"]]
    G.dump(f"{entry}_{name}", rows)
    assert not problems, (name, problems, rows["kinds"])


@pytest.mark.parametrize("name", list(G.NT_CASES))
def test_gemm_nt_route(name):
    _run_case("nt", G.NT_CASES, name)


@pytest.mark.parametrize("name", list(G.TN_CASES))
def test_gemm_tn_route(name):
    _run_case("tn", G.TN_CASES, name)


@pytest.mark.parametrize("name", list(G.LINEAR_CASES))
def test_linear_route(name):
    _run_case("linear", G.LINEAR_CASES, name)


@pytest.mark.parametrize("M,N,bias", [(33, 70, True), (33, 70, False), (0, 70, True), (33, 0, True)])
def test_gemm_nt_degenerate(M, N, bias):
    """K = 0: C = bias broadcast (or 0), exactly.  M = 0 or N = 0: returns 0 and touches nothing."""
    Nn = _nn()
    lib = Nn.lib()
    Ag, Bg = G.Guarded(max(M, 1), 16, 16, DEV), G.Guarded(max(N, 1), 16, 16, DEV)   # all NaN: nothing may be read
    K = 0 if M and N else 48
    Cg = G.Guarded(max(M, 1), max(N, 1), max(N, 1) + 3, DEV, "sentinel")
    b = torch.randn(max(N, 1))
    bg = G.operand(b[None, :], max(N, 1), DEV) if bias else None
    ws = Nn.workspace(1 << 20, DEV)
    rc = lib.abcd_gemm_nt(M, N, K, Ag.ptr(), 16 if K == 0 else K, Bg.ptr(), 16 if K == 0 else K, Cg.ptr(),
                          max(N, 1) + 3, bg.ptr() if bg else None, Nn.ptr(ws), ws.numel(), Nn.stream())
    torch.cuda.synchronize()
    assert rc == 0
    if M == 0 or N == 0:
        assert bool(torch.isnan(Cg.view).all()) and Cg.guard_intact()
        return
    assert lib.abcd_debug_gemm_route().decode() == "ks z=1"
    want = b.to(DEV)[None, :].expand(M, N) if bias else torch.zeros(M, N, device=DEV)
    assert torch.equal(Cg.view, want) and Cg.guard_intact()


# ----------------------------------------------------------------------------
# abcd_linear_backward
# ----------------------------------------------------------------------------
def _bwd_call(shape, act, want, ws_short=0, y_null=False):
    Nn = _nn()
    lib = Nn.lib()
    M, N, K = G.BWD_SHAPES[shape]
    d = G.bwd_data(shape, act)
    ldx, ldw, ldy, lddy, lddx = K + 3, K + 1, N + 2, N + 1, K + 5
    xg, Wg = G.operand(d["x"], ldx, DEV), G.operand(d["W"], ldw, DEV)
    yg, dyg = G.operand(d["y"], ldy, DEV), G.operand(d["dy"], lddy, DEV)
    out = dict(dx=G.Guarded(M, K, lddx, DEV, "sentinel"), dW=G.Guarded(N, K, K, DEV, "sentinel"),
               db=G.Guarded(1, N, N, DEV, "sentinel"))
    need = lib.abcd_linear_backward_workspace_bytes(M, N, K)
    ws = Nn.workspace(need, DEV)
    p = {k: (g.ptr() if want in ("all", k) else None) for k, g in out.items()}
    rc = lib.abcd_linear_backward(M, N, K, xg.ptr(), ldx, Wg.ptr(), ldw, None if y_null else yg.ptr(), ldy, act,
                                  dyg.ptr(), lddy, p["dx"], lddx, p["dW"], p["db"], Nn.ptr(ws), need - ws_short,
                                  Nn.stream())
    route = lib.abcd_debug_gemm_route().decode()
    torch.cuda.synchronize()
    return rc, route, out, d


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("want", G.BWD_WANTS)
@pytest.mark.parametrize("shape", list(G.BWD_SHAPES))
def test_linear_backward(shape, want, act):
    M, N, K = G.BWD_SHAPES[shape]
    rc, route, out, d = _bwd_call(shape, act, want)
    assert rc == 0
    if want != "db":
        assert route == G.BWD_ROUTE[(shape, want)], (shape, want, route)
    ref = G.bwd_reference(d["x"].to(DEV), d["W"].to(DEV), d["y"].to(DEV), d["dy"].to(DEV), act)
    got = {}
    for k, g in out.items():
        assert g.guard_intact(), f"{k}: written outside its extent"
        if want in ("all", k):
            got[k] = g.view.contiguous().reshape(ref[k].shape)
        else:
            assert bool(torch.isnan(g.view).all()), f"{k} was NULL and its tensor changed"
    fig, fails = G.bwd_check(got, ref, M, N, K)
    if act == 1 and "dx" in got:   # rows whose every y is +-1 have dy' = 0 exactly: dx = 0 exactly
        dead = (ref["dyp"] == 0).all(1)
        fig["dead_rows"] = int(dead.sum())
        if bool(dead.any()) and not bool((got["dx"][dead] == 0).all()):
            fails.append("dx:dead rows")
    _, _, out2, _ = _bwd_call(shape, act, want)
    for k in got:
        if not torch.equal(out[k].view, out2[k].view):
            fails.append(k + ":repeat")
    print(shape, want, act, route, fig)
    G.dump(f"bwd_{shape}_{want}_act{act}", dict(entry="linear_backward", case=f"{shape}/{want}/act{act}", M=M, N=N, K=K,
                                                 route=route if want != "db" else None, figures=fig, fails=fails))
    assert not fails, (fails, fig)


def test_linear_backward_tanh_zero_gradient():
    """y = +-1 everywhere in one column: that column of dW and its db are exactly 0."""
    shape, act = "m50n7k33", 1
    M, N, K = G.BWD_SHAPES[shape]
    d = {k: v.clone() for k, v in G.bwd_data(shape, act).items()}
    d["y"][:, 3] = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)
    Nn = _nn()
    lib = Nn.lib()
    xg, Wg, yg, dyg = (G.operand(d[k], d[k].shape[1] + 1, DEV) for k in ("x", "W", "y", "dy"))
    dW, db = G.Guarded(N, K, K, DEV, "sentinel"), G.Guarded(1, N, N, DEV, "sentinel")
    need = lib.abcd_linear_backward_workspace_bytes(M, N, K)
    ws = Nn.workspace(need, DEV)
    rc = lib.abcd_linear_backward(M, N, K, xg.ptr(), K + 1, Wg.ptr(), K + 1, yg.ptr(), N + 1, act, dyg.ptr(), N + 1,
                                  None, 0, dW.ptr(), db.ptr(), Nn.ptr(ws), need, Nn.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((dW.view[3] == 0).all()) and float(db.view[0, 3]) == 0.0
    assert bool(torch.isfinite(dW.view).all()) and dW.guard_intact() and db.guard_intact()


@pytest.mark.parametrize("how", ["ws_short", "tanh_without_y"])
def test_linear_backward_refuses(how):
    """ABCD_EINVAL, and nothing is written."""
    rc, _, out, _ = _bwd_call("m50n7k33", 1, "all", ws_short=4 if how == "ws_short" else 0,
                              y_null=how == "tanh_without_y")
    assert rc == G.EINVAL
    for k, g in out.items():
        assert g.guard_intact() and bool(torch.isnan(g.view).all()), k
