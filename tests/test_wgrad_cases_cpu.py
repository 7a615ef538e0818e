"""tests/wgrad_cases.py without a GPU: torch's CPU fp32 stands in for the
library on every table (through the same guarded views, so honest fp32 meets
every bar and leaves every guard intact), the launch arithmetic the shapes were
chosen from is asserted against its restatements, and emulations of the
defects the bars are for show that each bar can fail."""
import pytest

import gemm_cases as G
import wgrad_cases as W


# ----------------------------------------------------------------------------
# honest fp32 meets every bar
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(W.WG_CASES))
def test_cpu_fp32_wgrad_meets_every_bar(name):
    c = W.WG_CASES[name]
    for kind in G.KINDS:
        data = W.wg_data(name, kind)
        b = W.wg_buffers(c, data, "cpu")
        W.wg_cpu_kernel(c, b)
        fig, fails = W.wg_check(c, kind, data, b)   # e32 is this result's own error: trivially met
        assert not fails, (name, kind, fails, fig)


@pytest.mark.parametrize("name", list(W.OFF_FWD_CASES))
def test_cpu_fp32_offset_forward_meets_every_bar(name):
    c = W.OFF_FWD_CASES[name]
    for kind in G.KINDS:
        d = W.off_fwd_data(name, kind)
        b = W.off_fwd_buffers(c, d, "cpu")
        W.off_fwd_cpu_kernel(c, b)
        fig, fails = W.off_fwd_check(c, kind, d, b)
        assert not fails, (name, kind, fails, fig)


@pytest.mark.parametrize("name", list(W.OFF_BWD_CASES))
def test_cpu_fp32_offset_backward_meets_every_bar(name):
    c = W.OFF_BWD_CASES[name]
    for kind in W.BWD_KINDS:
        d = W.off_bwd_data(name, kind)
        b = W.off_bwd_buffers(c, d, "cpu")
        W.off_bwd_cpu_kernel(c, b)
        fig, fails = W.off_bwd_check(c, kind, d, b)
        assert not fails, (name, kind, fails, fig)


@pytest.mark.parametrize("batch", ["eight", "one"])
def test_cpu_fp32_tn_batch_meets_every_bar(batch):
    jobs = W.TN_JOBS if batch == "eight" else W.TN_JOBS_ONE
    for kind in G.KINDS:
        data = W.tn_data(batch, kind)
        b = W.tn_buffers(jobs, data, "cpu")
        W.tn_cpu_kernel(jobs, b)
        fig, fails = W.tn_check(jobs, kind, data, b)
        assert not fails, (kind, fails, fig)


def test_cpu_fp32_colsum_meets_the_bar_at_every_slicing():
    jobs, data = W.CS_JOBS, W.cs_data()
    tight = W.colsum_slicing(jobs, W.CS_AMPLE)[5][2] + 3 * 1029 + 2 * 65 + 1   # 3 of job 5's 60 slices fit
    assert [s[0] for s in W.colsum_slicing(jobs, tight)][5:] == [3, 2, 1]
    for floats in (W.CS_AMPLE, tight):
        sl = W.colsum_slicing(jobs, floats)
        b = W.cs_buffers(jobs, data, "cpu")
        W.cs_cpu_kernel(jobs, b, sl)
        fig, fails = W.cs_check(jobs, data, b)
        assert not fails, (fails, fig)


# ----------------------------------------------------------------------------
# the arithmetic the shapes were chosen from
# ----------------------------------------------------------------------------
def test_wg_launch_claims():
    for (form, nd, K), want in W.WG_CLAIMS.items():
        got = W.wg_launch(form, nd, K)
        assert {k: got[k] for k in want} == want, (form, nd, K, got)
    for form, kq in (("wg3b", 64), ("wg2", 32)):
        for nd in (1, 2):
            for K in W.WG_KS:
                g = W.wg_launch(form, nd, K)
                assert g["kps"] % kq == 0 and (g["Z"] - 1) * g["kps"] < K <= g["Z"] * g["kps"] and g["tw"] == 8
    # K below one chunk, on a chunk, one past it; one past a wg3b range
    assert [W.wg_launch("wg3b", 2, K)["chunks_last"] for K in (1, 31, 32, 33, 64)] == [1, 1, 1, 2, 2]
    assert W.wg_launch("wg2", 2, 64)["Z"] == 2 and W.wg_launch("wg2", 2, 64)["last"] == 32


def test_wg_tables():
    names = set(W.WG_CASES)
    for form in ("wg3b", "wg2"):
        for nd in (1, 2):
            for K in W.WG_KS:
                assert f"{form}_nd{nd}_k{K}" in names
    for c in W.WG_CASES.values():
        resident = c["H"] == 256 and W.rup16(c["F"] + 1) == 144
        if c["form"] != "split":
            assert resident and c["route"] == f"gemm_{c['form']}<144,256> x{c['nd']}"
        else:
            assert c["route"] == "gemm split (x6s/x6t)"
            assert not resident or c["env"].get("ABCD_WG2") == "0" or any(c["dg_off"]) or any(c["hp_off"])
        # the largest operand stays at 16 MiB
        assert 4 * c["K"] * 4 * c["H"] <= 17 << 20
    assert W.rup16(128 + 1) == 144 and W.rup16(143 + 1) == 144 and W.rup16(127 + 1) == 128 and W.rup16(144 + 1) == 160


def test_x6r8_grid_claims():
    for (M, N), want in W.GRID_CLAIMS.items():
        got = W.x6r8_grid(M, N)
        assert {k: got[k] for k in want} == want, (M, N, got)
    for N in W.OFF_NS:
        g = W.x6r8_grid(65, N)
        assert g["grid"] % 8 == 0 and g["used"] == 3 and g["last"] == 1 and g["passes"] == 1
        assert W.x6r8_grid(1, N)["used"] == 1
    assert W.x6r8_grid(65, 1024)["nslices"] > 256 // 32   # more slices than the 8 K chunks of the backward
    for tab in (W.OFF_FWD_CASES, W.OFF_BWD_CASES):
        for c in tab.values():
            assert c["K"] <= 256 and c["K"] % 8 == 0 and c["N"] % 4 == 0
            assert 4 * c["M"] * max(c["N"], c["K"] + 4) <= 24 << 20


def test_colsum_slicing():
    sl = W.colsum_slicing(W.CS_JOBS, W.CS_AMPLE)
    assert [s[0] for s in sl] == [1, 1, 1, 2, 241, 60, 2, 1]
    assert all(s[0] * s[1] >= j[0] > (s[0] - 1) * s[1] for s, j in zip(sl, W.CS_JOBS))


# ----------------------------------------------------------------------------
# the bars can fail (emulations only)
# ----------------------------------------------------------------------------
def _wg_emulated(name, kind, **kw):
    """w_ih of direction 0 by the six-term emulation: (result, reference, K)."""
    c = W.WG_CASES[name]
    d = W.wg_data(name, kind)
    A, B = d["dG"][0].t()[:256].contiguous(), d["X"].t().contiguous()
    return G.x6_emulated(A, B, **kw), G.reference(A, B, None, unit=kind == "a"), c["K"]


def test_honest_emulation_passes_the_wgrad_bars():
    for kind in G.KINDS:
        C, rf, K = _wg_emulated("wg3b_nd2_k193", kind)
        assert not G.check(kind, C, rf, K)["fails"], kind


@pytest.mark.parametrize("drop", [(2, 0), (1, 1), (0, 2)])
def test_missing_cross_term_fails_bar_c(drop):
    failed = []
    for kind in ("c", "cs"):
        C, rf, K = _wg_emulated("wg3b_nd2_k193", kind, drop=drop)
        failed.append("c" in G.check(kind, C, rf, K)["fails"])
    assert any(failed), (drop, failed)


@pytest.mark.parametrize("K", [65, 193])
def test_last_frame_of_last_range_left_out_fails_bars_a_and_b(K):
    name = f"wg3b_nd2_k{K}"
    C, rf, _ = _wg_emulated(name, "a", kmax=K - 1)
    assert "a" in G.check("a", C, rf, K)["fails"]
    for kind in ("b", "bs"):
        C, rf, _ = _wg_emulated(name, kind, kmax=K - 1)
        assert "b" in G.check(kind, C, rf, K)["fails"], kind
    # and through the buffers, with torch's fp32: both weights of both directions notice on kind a (every frame's
    # products are O(1)); the bias, whose frame k weighs 2^e[k] there, on kind b (dG unscaled)
    c = W.WG_CASES[name]
    for kind, want in (("a", {"w_ih0", "w_hh0", "w_ih1", "w_hh1"}), ("b", {"b_ih0", "b_ih1"})):
        data = W.wg_data(name, kind)
        b = W.wg_buffers(c, data, "cpu")
        W.wg_cpu_kernel(c, b, frames=K - 1)
        _, fails = W.wg_check(c, kind, data, b)
        assert {f.split(":")[0] for f in fails} >= want, (kind, fails)


@pytest.mark.parametrize("name", ["wg3b_nd2_k193", "wg3b_f128", "wg3b_f143"])
def test_ones_column_one_off_fails_the_bias(name):
    c = W.WG_CASES[name]
    for kind in ("a", "bs"):
        data = W.wg_data(name, kind)
        b = W.wg_buffers(c, data, "cpu")
        W.wg_cpu_kernel(c, b, ones_col=c["F"] + 1 if c["F"] + 1 < W.rup16(c["F"] + 1) else c["F"] - 1)
        _, fails = W.wg_check(c, kind, data, b)
        assert fails and {f.split(":")[0] for f in fails} == {"b_ih0", "b_ih1"}, (kind, fails)


@pytest.mark.parametrize("name,skip", [("m65_n192_k256", 2), ("m65_n68_k256", 1), ("m1_n1024_k256", 9)])
def test_one_partial_left_out_fails_the_logit(name, skip):
    c = W.OFF_FWD_CASES[name]
    d = W.off_fwd_data(name, "a")
    b = W.off_fwd_buffers(c, d, "cpu")
    W.off_fwd_cpu_kernel(c, b, skip_slice=skip)
    _, fails = W.off_fwd_check(c, "a", d, b)
    assert "logit:not the partials' sum" in fails and "logit:bar" in fails, fails


def test_offset_forward_by_the_six_term_emulation():
    """The honest emulation meets Zo's bars; one cross term less and c / cs fail."""
    c = W.OFF_FWD_CASES["m65_n192_k256"]
    for kind in G.KINDS:
        d = W.off_fwd_data(c["name"], kind)
        b = W.off_fwd_buffers(c, d, "cpu")
        W.off_fwd_cpu_kernel(c, b, x6=True)
        _, fails = W.off_fwd_check(c, kind, d, b)
        assert not fails, (kind, fails)


@pytest.mark.parametrize("name", ["m65_n64_k256", "m65_n192_k256", "m1_n320_k256"])
def test_unwritten_dzo_chunks_fail_the_finite_check(name):
    """Slice s storing chunk c == s only: the chunks >= nslices are never written."""
    c = W.OFF_BWD_CASES[name]
    d = W.off_bwd_data(name, "a")
    b = W.off_bwd_buffers(c, d, "cpu")
    W.off_bwd_cpu_kernel(c, b, chunks_written=W.x6r8_grid(c["M"], c["N"])["nslices"])
    _, fails = W.off_bwd_check(c, "a", d, b)
    assert fails == ["dZo:finite"], fails


def test_dzo_bar_fails_on_a_missing_factor():
    c = W.OFF_BWD_CASES["m65_n64_k256"]
    d = W.off_bwd_data(c["name"], "a")
    b = W.off_bwd_buffers(c, d, "cpu")
    W.off_bwd_cpu_kernel(c, b)
    b["dlog_s"].view[0, 3] *= 1 + 2.0 ** -23
    b["dZo"].view[5] *= 1 + 2.0 ** -18   # 64 u (1 - Zo^2) of the leading product: over the bar wherever Zo^2 < 7 / 8
    _, fails = W.off_bwd_check(c, "a", d, b)
    assert "dlog_s:bits" in fails and "dZo:bar" in fails, fails


def test_colsum_skipping_its_last_slice_fails():
    jobs, data = W.CS_JOBS, W.cs_data()
    b = W.cs_buffers(jobs, data, "cpu")
    W.cs_cpu_kernel(jobs, b, W.colsum_slicing(jobs, W.CS_AMPLE), skip_last_slice=True)
    _, fails = W.cs_check(jobs, data, b)
    multi = {f"job{i}" for i, s in enumerate(W.colsum_slicing(jobs, W.CS_AMPLE)) if s[0] > 1}
    assert multi and {f.split(":")[0] for f in fails} == multi, fails


def test_debug_entry_points_refuse_null_and_negative_arguments():
    """Host-side returns, no device needed."""
    import ctypes
    from modules import _native as Nn
    lib = Nn.lib()
    fused = ctypes.c_int(-1)
    p = ctypes.c_void_p(256)   # never dereferenced: every call below returns before any launch
    assert lib.abcd_debug_offset_head_fwd(0, 64, 64, p, 64, p, p, p, p, None, p, p, p, p, p, ctypes.byref(fused),
                                          None) == G.EINVAL
    assert lib.abcd_debug_offset_head_fwd(4, 64, 64, None, 64, p, p, p, p, None, p, p, p, p, p, ctypes.byref(fused),
                                          None) == G.EINVAL
    assert lib.abcd_debug_offset_head_bwd(4, -1, 64, p, p, p, p, p, p, p, p, ctypes.byref(fused), None) == G.EINVAL
    assert lib.abcd_debug_offset_head_bwd(4, 64, 64, p, p, p, p, p, None, p, p, ctypes.byref(fused), None) == G.EINVAL
    assert lib.abcd_debug_gemm_tn_batch(-1, *[None] * 11, None) == G.EINVAL
    assert lib.abcd_debug_gemm_tn_batch(1, *[None] * 11, None) == G.EINVAL
    assert lib.abcd_debug_gemm_tn_batch(0, *[None] * 11, None) == 0
    assert lib.abcd_debug_colsum_batch(-1, *[None] * 8, None, 0, None) == G.EINVAL
    assert lib.abcd_debug_colsum_batch(1, *[None] * 8, None, 0, None) == G.EINVAL
    assert lib.abcd_debug_colsum_batch(0, *[None] * 8, None, 0, None) == 0
