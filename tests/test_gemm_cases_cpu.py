"""tests/gemm_cases.py without a GPU: torch's CPU fp32 GEMM stands in for the
library on every case of the tables (so the reference alone stays inside every
bar), a bf16 emulation of the six-term product shows that each bar can fail,
and the tables and the guard band are checked for what they promise."""
import pytest
import torch

import gemm_cases as G

ALL = [(t, n) for t, tab in (("nt", G.NT_CASES), ("tn", G.TN_CASES), ("linear", G.LINEAR_CASES)) for n in tab]


@pytest.mark.parametrize("table,name", ALL)
def test_cpu_fp32_gemm_meets_every_bar(table, name):
    c = {"nt": G.NT_CASES, "tn": G.TN_CASES, "linear": G.LINEAR_CASES}[table][name]
    act = c.get("act", 0)
    for kind in G.KINDS:
        d = G.case_data(table, name, kind)
        rf = G.reference(d["A"], d["B"], d["bias"], unit=kind == "a")
        z32 = d["A"] @ d["B"].t()
        if d["bias"] is not None:
            z32 = z32 + d["bias"]
        C = torch.tanh(z32) if act == 1 else z32
        # the max-norm bar compares with torch's fp32 GEMM itself: e32 = this C's own error, trivially met
        fig = G.check(kind, C, rf, c["K"], act, G.max_norm_err(C, torch.tanh(rf["ref"]) if act else rf["ref"]))
        assert not fig["fails"], (name, kind, fig)


@pytest.mark.parametrize("shape", list(G.BWD_SHAPES))
@pytest.mark.parametrize("act", [0, 1])
def test_cpu_fp32_backward_meets_the_bars(shape, act):
    M, N, K = G.BWD_SHAPES[shape]
    d = G.bwd_data(shape, act)
    ref = G.bwd_reference(d["x"], d["W"], d["y"], d["dy"], act)
    dyp = d["dy"] * (1 - d["y"] * d["y"]) if act == 1 else d["dy"]
    got = dict(dx=dyp @ d["W"], dW=dyp.t() @ d["x"], db=dyp.sum(0))
    fig, fails = G.bwd_check(got, ref, M, N, K)
    assert not fails, (fails, fig)
    if act == 1:
        ones = d["y"].abs() == 1
        assert bool(ones.any()) and bool((ref["dyp"][ones] == 0).all())


# ----------------------------------------------------------------------------
# the bars can fail
# ----------------------------------------------------------------------------
EMU = ("nt", "x6r8_5_t16_k144")   # 15233 x 129 x 144


def _emu(kind):
    d = G.case_data(*EMU, kind)
    A, B = d["A"][:2048], d["B"]
    return A, B, G.reference(A, B, None, unit=kind == "a")


def test_honest_emulation_passes():
    for kind in G.KINDS:
        A, B, rf = _emu(kind)
        fig = G.check(kind, G.x6_emulated(A, B), rf, A.shape[1])
        assert not fig["fails"], (kind, fig)


@pytest.mark.parametrize("drop", [(2, 0), (1, 1), (0, 2)])
def test_missing_cross_term_fails_bar_c(drop):
    """One u-sized cross term of the six left out: the single-product data sees it."""
    failed = []
    for kind in ("c", "cs"):
        A, B, rf = _emu(kind)
        failed.append("c" in G.check(kind, G.x6_emulated(A, B, drop=drop), rf, A.shape[1])["fails"])
    # a2 b0 vanishes where B's one value per row has no third piece to lose (A selects: cs sees it), and so on:
    # each term is seen by the orientation in which its operands are full-mantissa
    assert any(failed), (drop, failed)


def test_dropped_last_k_fails_bars_a_and_b():
    K = G.NT_CASES[EMU[1]]["K"]
    A, B, rf = _emu("a")
    assert "a" in G.check("a", G.x6_emulated(A, B, kmax=K - 1), rf, K)["fails"]
    for kind in ("b", "bs"):
        A, B, rf = _emu(kind)
        assert "b" in G.check(kind, G.x6_emulated(A, B, kmax=K - 1), rf, K)["fails"], kind


def test_one_padding_nan_fails_finiteness():
    A, B, rf = _emu("a")
    C = G.x6_emulated(A, B)
    C[17, 5] = float("nan")
    assert G.check("a", C, rf, A.shape[1])["fails"] == ["finite"]


# ----------------------------------------------------------------------------
# the tables
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("table,name", ALL)
def test_selection_patterns(table, name):
    """Row 0 selects the last valid k; every k is selected where the operand
    has at least K rows (all K positions of every fragment layout), min(rows,
    K) distinct ones spread over the whole depth otherwise; at K >= 64 adjacent
    rows sit in different 4-lane and 8-lane groups (but where the pattern wraps)."""
    c = {"nt": G.NT_CASES, "tn": G.TN_CASES, "linear": G.LINEAR_CASES}[table][name]
    K = c["K"]
    for R in (c["M"], c["N"]):
        k = G.sel_k(R, K)
        assert int(k[0]) == K - 1
        assert len(set(k.tolist())) == min(R, K)
        if R > 1 and K >= 64:   # a shorter depth has too few groups for every adjacent pair to differ
            nowrap = k[:-1] > k[1:]
            assert bool(((k[:-1] // 8 != k[1:] // 8) & (k[:-1] // 4 != k[1:] // 4))[nowrap].all())
            assert int(nowrap.sum()) >= (R - 1) // 2
        if R < K:   # the rows reach down to the first tenth of the depth
            assert int(k.min()) < max(K // 10, 32), (R, K, int(k.min()))
    if max(c["M"], c["N"]) >= K:
        R = max(c["M"], c["N"])
        assert set(G.sel_k(R, K).tolist()) == set(range(K))
    for kind in ("b", "bs"):
        d = G.case_data(table, name, kind)
        sel = d["B"] if kind == "b" else d["A"]
        assert bool(((sel != 0).sum(1) == 1).all())
        v = sel[sel != 0].abs()
        assert bool((torch.frexp(v)[0] == 0.5).all())   # powers of two


def test_tables_name_every_route():
    want = {"x6r8<5,128>", "x6r8<5,128,t16>", "x6r8<8,64>", "x6f", "x6t", "x6s<4,5>", "x6s<4,5,one>", "x6s<5,4,one>",
            "x6s<4,4,one>", "tn<4,4,kc>", "tn<4,8,kc>", "ks", "big"}
    have = {r.split(" ")[0] for r in G.ROUTES_EXPECTED}
    assert want <= have, want - have
    reduces = {r.split(" ")[2] for r in G.ROUTES_EXPECTED if r.count(" ") == 2}
    assert reduces == {"zg4", "zg16", "vec", "scalar"}


def test_case_memory():
    """Each case's operands and output stay near 16 MB (the largest: 15233 x 129 x 304 at lda = 308)."""
    for tab in (G.NT_CASES, G.TN_CASES, G.LINEAR_CASES):
        for c in tab.values():
            floats = c["M"] * c["K"] + c["N"] * c["K"] + c["M"] * c["N"]
            assert floats * 4 <= 28 << 20, c["name"]


def test_guard_band_flags_one_changed_sentinel():
    g = G.Guarded(5, 7, 9, "cpu", "sentinel", off=1)
    assert bool(torch.isnan(g.view).all()) and g.guard_intact()
    g.view.copy_(torch.randn(5, 7))
    assert g.guard_intact()
    for pos in (0, g.start - 1, g.start + 7, g.start + 9 * 4 + 8, g.start + 5 * 9, g.n - 1):
        h = G.Guarded(5, 7, 9, "cpu", "sentinel", off=1)
        h.view.zero_()
        h.flat.view(torch.int32)[pos] ^= 1      # one bit of one guard word
        assert not h.guard_intact(), pos
    o = G.operand(torch.ones(3, 4), 6, "cpu", off=1)
    assert bool(torch.isnan(o.flat).sum() == o.n - 12) and o.ptr() == o.flat.data_ptr() + 4 * (G.MARGIN + 1)


def test_route_seam_on_the_host():
    """The two diagnostics need no device: "" before any dispatch on this thread, and the side switch returns."""
    import threading
    from modules import _native as Nn
    lib = Nn.lib()
    seen = []

    def fresh_thread():
        seen.append(lib.abcd_debug_gemm_route())
        lib.abcd_debug_gemm_side(1)
        lib.abcd_debug_gemm_side(0)

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen == [b""]
