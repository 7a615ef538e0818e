"""Syntax-aware segmentation with the table in windows, checked on the CPU:
``segmentation.plan_windows`` (cover, alignment, sizes, the peak-bytes bound),
the numpy windowed reference of ``stream_cases.py`` against
``syntax_cases.chain_reference`` on the whole table (the algebra of the carry,
of ``row0`` and of the phase B that is skipped at N), the new entry points'
surface and host-side argument checks, and ``segment.py --window_frames``."""
import numpy as np
import pytest
import torch

import stream_cases as ST
import syntax_cases as SX

SYMS = ("abcd_span_chain_window_workspace_bytes", "abcd_span_chain_viterbi_window")


# ----------------------------------------------------------------------------
# plan_windows
# ----------------------------------------------------------------------------
def _check_plan(plan, N, D, W, align, K=128):
    from modules import segmentation
    assert all(isinstance(v, int) for w in plan for v in w)
    at = 1
    for row0, n0, n1 in plan:
        assert n0 == at and n0 <= n1 <= N                                   # in order, no hole, no overlap
        assert 1 <= n1 - n0 + 1 <= W
        assert row0 % align == 0 and 0 <= row0 <= max(0, n0 - D)
        assert row0 == align * (max(0, n0 - D) // align)
        assert max(0, n0 - D) - row0 < align                                # no more than a tile of extra frames
        nbytes = segmentation.window_table_bytes((row0, n0, n1), D, K)
        assert nbytes == 8 * (n1 - row0 + 1) * D * K <= 8 * (W + D + align) * D * K
        at = n1 + 1
    assert at == N + 1                                                      # the ends 1 .. N exactly once
    if N:
        assert len(plan) == -(-N // W)


@pytest.mark.parametrize("D", ST.PLAN_D)
@pytest.mark.parametrize("N", ST.PLAN_N)
def test_plan_windows(N, D):
    from modules import segmentation
    for W in (1, 3, D, N, N + 5):
        plan = segmentation.plan_windows(N, D, W)
        _check_plan(plan, N, D, W, 32)
        assert plan == ST.plan(N, D, W)
        assert len(segmentation.plan_windows(N, D, W, align=1)) == len(plan)
        _check_plan(segmentation.plan_windows(N, D, W, align=1), N, D, W, 1)


def test_plan_windows_beyond_the_one_shot_limit_and_arguments():
    from modules import segmentation
    N, D = ST.LONG_ND
    K = 128
    assert (N + 1) * D * K >= 1 << 31                                       # no one-shot table at this shape
    for W in (256, 1024, 4096):
        plan = segmentation.plan_windows(N, D, W)
        _check_plan(plan, N, D, W, 32, K)
        peak = max(segmentation.window_table_bytes(w, D, K) for w in plan)
        assert peak <= 8 * (W + D + 32) * D * K
        assert max((n1 - row0 + 1) * D * K for row0, _, n1 in plan) < 1 << 31  # every window's table is indexable
    assert segmentation.plan_windows(0, 5, 4) == []
    assert segmentation.TABLE_ALIGN == 32
    for bad in ((-1, 5, 4), (9, 0, 4), (9, 5, 0)):
        with pytest.raises(ValueError):
            segmentation.plan_windows(*bad)
    with pytest.raises(ValueError):
        segmentation.plan_windows(9, 5, 4, align=0)


# ----------------------------------------------------------------------------
# the windowed reference is the reference
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SX.CHAIN_KINDS)
@pytest.mark.parametrize("ND", ST.REF_ND, ids=lambda v: f"n{v[0]}d{v[1]}")
def test_windowed_reference_is_the_reference(ND, kind):
    N, D = ND
    K = 5
    c = SX.chain_inputs(N, D, K, kind)
    segments = 0
    for i, (d_min, gap, bonus, tag) in enumerate(c["calls"]):
        ref = ST.reference(N, D, K, kind, i)
        segments += len(ref["onset"])
        for W in ST.window_sizes(N, D):
            for align in (32, 1):
                got = ST.windowed_reference(c["table"], d_min, c["trans"], c["init"], gap, bonus,
                                            ST.plan(N, D, W, align))
                assert ST.same_result(got, ref), (N, D, kind, tag, W, align)
        if kind == "nopath":
            ref0 = ST.reference(N, D, K, kind, i, "init_none")
            got = ST.windowed_reference(c["table"], d_min, c["trans"], c["init_none"], gap, bonus, ST.plan(N, D, 3))
            assert ST.same_result(got, ref0) and ref0["onset"] == []
    if kind in ("random", "tied", "gaps", "bonus"):
        assert segments > 0


def test_windowed_reference_refuses_a_call_out_of_order():
    N, D, K = 33, 5, 5
    c = SX.chain_inputs(N, D, K, "random")
    d_min, gap, bonus, _ = c["calls"][1]
    st = ST.new_state(N, K)
    args = (N, d_min, c["trans"], c["init"], gap, bonus)
    assert ST.window_step(st, ST.window_of(c["table"], 0, 1, 10), 0, 1, 10, *args)
    keep = (st["Wc"].copy(), st["G"], st["next_n"])
    assert not ST.window_step(st, ST.window_of(c["table"], 0, 12, 20), 0, 12, 20, *args)      # 11 is due
    assert np.array_equal(st["Wc"], keep[0]) and st["G"] == keep[1] and st["next_n"] == keep[2] == 11
    assert ST.window_step(st, ST.window_of(c["table"], 0, 11, 33), 0, 11, 33, *args)
    assert ST.same_result(ST.finish(st, N, c["trans"], c["init"]), ST.reference(N, D, K, "random", 1))


# ----------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in SYMS:
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.library_hash() == N.source_hash()
    ww, wc = N.lib().abcd_span_chain_window_workspace_bytes, N.lib().abcd_span_chain_workspace_bytes
    n, D = ST.LONG_ND
    assert wc(n, D, 128) == 0                                               # beyond the one-shot limit
    assert ww(n, D, 128) >= 24 * (n + 1) * 128 + 8 * (128 + 2)              # three planes' worth and the carry
    assert ww(n, D, 1025) == 0 and ww(n, D, 0) == 0 and ww(n, D, 1024) > 0
    assert ww(15000, 200, 128) >= 24 * 15001 * 128
    assert ww(0, 1, 1) > 0 and ww(-1, 1, 1) == 0 and ww(4, 0, 1) == 0 and ww(4, 16383, 1) > 0 and ww(4, 16384, 1) == 0
    assert ww((1 << 31) // 8 - 2, 8, 1) > 0 and ww((1 << 31) // 8 - 1, 8, 1) == 0       # (N + 1) D < 2^31 stays
    assert ww((1 << 31) // 64 - 1, 8, 8) > 0                                            # (N + 1) D K does not count


def test_window_entry_point_rejects_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, D, K = 40, 3, 5
    nb = lib.abcd_span_chain_window_workspace_bytes(n, D, K)

    def win(tb=fake, ldk=K, row0=0, rows=11, n0=1, n1=10, n=n, D=D, K=K, dmin=1, gap=None, bonus=0.0, lt=fake, ldt=K,
            li=fake, ps=fake, ns=fake, on=fake, ln=fake, ct=fake, sv=fake, lk=fake, W=None, ws=fake, nb=nb):
        return lib.abcd_span_chain_viterbi_window(tb, ldk, row0, rows, n0, n1, n, D, K, dmin, gap, bonus, lt, ldt, li,
                                                  ps, ns, on, ln, ct, sv, lk, W, ws, nb, None)

    assert win(n0=0) == E and win(n0=11, n1=10) == E and win(n1=n + 1, rows=n + 2) == E       # 1 <= n0 <= n1 <= N
    assert win(n=0, n0=1, n1=1) == E and win(n=-1) == E
    assert win(row0=-1) == E
    assert win(row0=1) == E                                                 # n0 - D < 0: the window starts at 0
    assert win(n0=9, n1=10, row0=7, rows=4) == E                            # row0 > n0 - D
    assert win(n0=9, n1=10, row0=6, rows=4) == E                            # n1 - row0 = 4 >= rows
    assert win(rows=10) == E and win(rows=0) == E
    assert win(rows=(1 << 31) // 15 + 1) == E                               # rows D ld_k >= 2^31
    assert win(rows=(1 << 31) // 30 + 1, ldk=2 * K) == E                    # the stride counts
    assert win(K=0, ldk=1, ldt=1) == E and win(K=1025, ldk=1025, ldt=1025, nb=1 << 40) == E
    assert win(dmin=0) == E and win(dmin=D + 1) == E and win(D=0) == E and win(D=16384, nb=1 << 40) == E
    assert win(n=(1 << 31) // 3, nb=1 << 40) == E                           # (N + 1) D >= 2^31
    assert win(ldk=K - 1) == E and win(ldt=K - 1) == E
    for k in ("tb", "lt", "li", "ps", "ns", "on", "ln", "ct", "sv", "lk"):
        assert win(**{k: None}) == E, k
    assert win(ws=None) == E and win(nb=nb - 1) == E and win(nb=0) == E


def test_operator_planner_and_keyword_exist():
    import inspect

    from modules import ops, segmentation
    assert hasattr(torch.ops.abcd, "span_chain_viterbi_window")
    assert "span_chain_viterbi_window" in ops.STATEFUL_OPS and "span_chain_viterbi_window" not in ops.OPS
    schema = str(torch.ops.abcd.span_chain_viterbi_window.default._schema)
    assert "!) state" in schema and "!)? W" in schema, schema               # the state and W are mutated, nothing else
    assert schema.count("!") == 2
    assert "window_frames" in inspect.signature(segmentation.segment_frames).parameters
    assert "window_frames" not in inspect.signature(segmentation.segment_chain_posteriors).parameters
    doc = " ".join(segmentation.segment_frames.__doc__.split())
    assert "8 (window_frames + max_length + 32) max_length K" in doc        # the peak-memory formula
    with pytest.raises(RuntimeError):                                       # no CPU path
        ops.span_chain_viterbi_window(torch.zeros(3, 2, 2, dtype=torch.float64), 0, 1, 2, 2, 1, None, 0.0,
                                      torch.zeros(2, 2), torch.zeros(2), torch.zeros(4096, dtype=torch.uint8), None)


def test_segment_frames_window_arguments():
    from modules import model as M, segmentation
    from modules.sequence import TransitionModel
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    x = torch.zeros(4, 33)
    with pytest.raises(RuntimeError):                                       # a CPU tensor: no CPU path
        segmentation.segment_frames(dec, None, x, 3, transitions=TransitionModel(4), window_frames=2)


# ----------------------------------------------------------------------------
# segment.py --window_frames
# ----------------------------------------------------------------------------
def test_segment_cli_window_arguments(capsys):
    import segment
    base = ["c", "r", "t", "1", "--max_length", "9"]
    assert segment.get_parameters(base).window_frames is None
    a = segment.get_parameters(base + ["--transitions", "t.csv", "--window_frames", "1024"])
    assert a.window_frames == 1024
    a = segment.get_parameters(base + ["--transitions", "t.csv", "--window_frames", "16", "--refit_transitions", "2",
                                       "--transitions_out", "o.csv"])       # Viterbi training runs in windows too
    assert a.window_frames == 16 and a.refit_method == "viterbi"
    for bad, why in ((["--window_frames", "16"], "needs --transitions"),
                     (["--window_frames", "16", "--refit_transitions", "1", "--transitions_out", "o.csv"],
                      "needs --transitions"),
                     (["--transitions", "t.csv", "--window_frames", "0"], "at least 1"),
                     (["--transitions", "t.csv", "--window_frames", "16", "--chain_posteriors"],
                      "sweeps the whole table backwards"),
                     (["--transitions", "t.csv", "--window_frames", "16", "--refit_transitions", "1",
                       "--transitions_out", "o.csv", "--refit_method", "em"], "not available in windows"),
                     (["--transitions", "t.csv", "--window_frames", "16", "--posteriors"], "--posteriors")):
        with pytest.raises(SystemExit):
            segment.get_parameters(base + bad)
        assert why in " ".join(capsys.readouterr().err.split()), bad
    with pytest.raises(SystemExit):
        segment.get_parameters(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--window_frames" in text and "8 (W + max_length + 32) max_length K" in text and "1024" in text
