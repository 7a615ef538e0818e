"""Time-warped segmentation without a GPU: the float64 reference of
tests/warpseg_cases.py against the enumeration of every cover, against the rigid
programme with the step move alone and on the planted recording, and the new
surface (symbols, host-side argument checks, workspace queries, the plan, the
operators' schemas, the Python and command-line arguments)."""
import itertools
import math

import numpy as np
import pytest
import torch

import syntax_cases as SY
import warpseg_cases as WS

SYMS = ("abcd_frame_costs", "abcd_warp_segment_plan", "abcd_warp_segment_workspace_bytes",
        "abcd_warp_segment_window")
NINF = -math.inf


# ----------------------------------------------------------------------------
# the reference against brute force
# ----------------------------------------------------------------------------
def _tiny(seed, N, K, T, tied):
    g = np.random.default_rng(seed)
    if tied:
        cost = g.integers(0, 3, size=(N, T * K)).astype(np.float32)
        v = np.where(g.random((T, K)) < 0.5, 800.0, -800.0).astype(np.float32)
        gap = g.integers(-3, 0, size=N).astype(np.float32)
        trans = g.integers(-2, 1, size=(K, K)).astype(np.float32)
        init = g.integers(-2, 1, size=K).astype(np.float32)
        enter = g.integers(-1, 1, size=K).astype(np.float32)
    else:
        cost = (g.random((N, T * K)) * 4.0).astype(np.float32)
        v = g.normal(0.0, 2.0, size=(T, K)).astype(np.float32)
        gap = g.normal(-3.0, 1.0, size=N).astype(np.float32)
        trans = g.normal(-1.0, 1.0, size=(K, K)).astype(np.float32)
        init = g.normal(-1.0, 1.0, size=K).astype(np.float32)
        enter = g.normal(0.0, 1.0, size=K).astype(np.float32)
    if seed % 3 == 0:
        cost[g.random(cost.shape) < 0.15] = np.nan if seed % 2 else np.inf
    if seed % 5 == 0:
        trans[g.random(trans.shape) < 0.3] = NINF
    return cost, v, enter, gap, trans, init


@pytest.mark.parametrize("moves", list(WS.MOVES))
@pytest.mark.parametrize("NKT", [(1, 1, 1), (2, 2, 1), (3, 1, 3), (4, 2, 2), (5, 2, 3), (5, 1, 2)],
                         ids=lambda v: "n%dk%dt%d" % v)
def test_reference_is_the_enumeration(NKT, moves):
    N, K, T = NKT
    segments = 0
    for seed, tied, with_gap, s_min, bonus in itertools.product(range(6), (False, True), (False, True), (0, 1),
                                                                (0.0, -1.0)):
        if s_min >= T:
            continue
        cost, v, enter, gap, trans, init = _tiny(1000 * N + 100 * K + 10 * T + seed, N, K, T, tied)
        args = (cost, v, WS.MOVES[moves], enter if seed % 2 else None, gap if with_gap else None, bonus, trans, init,
                s_min)
        ref = WS.warpseg_reference(*args)
        best, segs, count = WS.brute_force(*args)
        assert ref["path_score"] == best, (NKT, moves, seed, tied, with_gap, s_min)
        got = list(zip(ref["onset"], ref["length"], ref["cat"], ref["last_state"]))
        segments += len(got)
        if count == 1 and not tied:
            assert got == segs, (NKT, moves, seed, with_gap, s_min)
        # the segments the reference reports are a cover in time order, and their ends are where it says
        at = 0
        for o, d, k, s in got:
            assert o >= at and d >= 1 and 0 <= k < K and s_min <= s < T
            at = o + d
        assert at <= N
    assert segments > 0


def test_reference_outputs_are_consistent():
    """enter, exit and link of every segment are the U, X and chain terms of the planes."""
    d = WS.prog_inputs(33, 2, 3, "random")
    ref = WS.prog_reference(d, "default", 0)
    assert len(ref["onset"]) > 1
    for o, n, k, e, x in zip(ref["onset"], ref["length"], ref["cat"], ref["enter"], ref["exit"]):
        assert e == ref["U"][o, k] and x == ref["W"][o + n, k]


# ----------------------------------------------------------------------------
# the step move alone is the rigid programme
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("s_min", (0, 2))
@pytest.mark.parametrize("kind", ("random", "gaps", "zeros"))
@pytest.mark.parametrize("NKT", [(33, 2, 3), (33, 5, 7), (70, 3, 5)], ids=lambda v: "n%dk%dt%d" % v)
def test_step_only_is_the_chain_programme(NKT, kind, s_min):
    N, K, T = NKT
    d = WS.prog_inputs(N, K, T, kind)
    for gap in (None, d["gap"]):
        ref = WS.warpseg_reference(d["cost"], d["v"], WS.MOVES["identity"], None, gap, d["bonus"], d["trans"],
                                   d["init"], s_min)
        table = WS.rigid_table(d["cost"], d["v"])
        rigid = SY.chain_reference(table, s_min + 1, d["trans"], d["init"], gap, d["bonus"])
        assert ref["onset"] == rigid["onset"] and ref["length"] == rigid["length"] and ref["cat"] == rigid["cat"]
        assert ref["last_state"] == [n - 1 for n in rigid["length"]]
        if not ref["onset"]:
            assert ref["path_score"] == rigid["path_score"]
            continue
        _, mag = SY.terms_of(rigid, N, gap if gap is not None else np.zeros(N), d["bonus"])
        assert abs(ref["path_score"] - rigid["path_score"]) <= 1e-9 * mag, (NKT, kind, s_min)
        assert len(ref["onset"]) > 0


# ----------------------------------------------------------------------------
# the planted recording
# ----------------------------------------------------------------------------
def test_planted_recording_separates_the_two_programmes():
    d = WS.planted()
    warped, rigid = WS.planted_references()
    assert warped["onset"] == d["onset"] and warped["length"] == d["length"] and warped["cat"] == d["cat"]
    assert warped["last_state"] == [WS.PLANT_S - 1] * len(d["onset"])
    assert (rigid["onset"], rigid["length"], rigid["cat"]) != (d["onset"], d["length"], d["cat"])
    assert warped["path_score"] > rigid["path_score"]
    assert any(n > WS.PLANT_S for n in d["length"]) and any(n < WS.PLANT_S for n in d["length"])


# ----------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_exported_and_hashed():
    from modules import _native as N
    from test_host import header_symbols
    for s in SYMS:
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.library_hash() == N.source_hash()


def test_workspace_queries_and_plan():
    from modules import _native as N
    lib = N.lib()
    ws = lib.abcd_warp_segment_workspace_bytes
    assert ws(0, 1, 1) > 0 and ws(-1, 1, 1) == 0
    assert ws(10, 1024, 1) > 0 and ws(10, 1025, 1) == 0 and ws(10, 0, 1) == 0
    assert ws(10, 1, 16383) > 0 and ws(10, 1, 16384) == 0 and ws(10, 1, 0) == 0
    assert ws(10, 1024, 16383) > 0 and ws(10, 1024, 16384) == 0             # K T < 2^24: 1024 * 16384 = 2^24
    assert ws(10, 1023, 16383) > 0
    assert ws((1 << 31) // 8 - 2, 8, 1) > 0 and ws((1 << 31) // 8 - 1, 8, 1) == 0   # (N + 1) K < 2^31
    n, K, T = 15000, 128, 200
    assert ws(n, K, T) >= 32 * (n + 1) * K + 40 * K * T + 8 * (K + 2)
    assert ws(n, K, T) <= 32 * (n + 1) * K + 40 * K * T + 8 * (K + 2) + 256
    res, thr, lds = N.c_int(-1), N.c_int(-1), N.c_size_t(0)
    import ctypes
    for K, want in ((1, 1), (128, 1), (129, 0), (1024, 0)):
        assert lib.abcd_warp_segment_plan(K, 5, ctypes.byref(res), ctypes.byref(thr), ctypes.byref(lds)) == 0
        assert res.value == want and thr.value == 1024
        assert lds.value == 32 * K + 16 * 1024 + (4 * K * K if want else 0)
        assert lds.value <= 160 * 1024
    assert lib.abcd_warp_segment_plan(128, 5, None, None, None) == 0
    for K, T in ((0, 5), (1025, 5), (5, 0), (5, 16384), (1024, 16384)):
        assert lib.abcd_warp_segment_plan(K, T, None, None, None) == N.ABCD_EINVAL


def test_window_entry_point_rejects_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, K, T = 40, 5, 3
    nb = lib.abcd_warp_segment_workspace_bytes(n, K, T)
    ok_moves = (N.c_double * 3)(*WS.MOVES["default"])

    def moves(*v):
        return (N.c_double * 3)(*v)

    def win(c=fake, ldc=K * T, n0=0, n1=10, n=n, K=K, T=T, v=fake, lm=ok_moves, le=None, gap=None, bonus=0.0, lt=fake,
            ldt=K, li=fake, smin=0, ps=fake, ns=fake, on=fake, ln=fake, ct=fake, st=fake, en=fake, ex=fake, lk=fake,
            W=None, ws=fake, nb=nb):
        return lib.abcd_warp_segment_window(c, ldc, n0, n1, n, K, T, v, lm, le, gap, bonus, lt, ldt, li, smin, ps, ns,
                                            on, ln, ct, st, en, ex, lk, W, ws, nb, None)

    assert win(n0=-1) == E and win(n0=10, n1=10) == E and win(n0=11, n1=10) == E and win(n1=n + 1) == E
    assert win(n=-1) == E
    assert win(n=0, n0=0, n1=1) == E                                        # N = 0 takes n0 = n1 = 0
    assert win(K=0, ldc=T, ldt=1) == E and win(K=1025, ldc=1025 * T, ldt=1025, nb=1 << 40) == E
    assert win(T=0) == E and win(T=16384, ldc=K * 16384, nb=1 << 40) == E
    assert win(K=1024, T=16384, ldc=1 << 24, ldt=1024, nb=1 << 50) == E     # K T >= 2^24
    assert win(n=(1 << 31) // K, nb=1 << 50) == E                           # (N + 1) K >= 2^31
    assert win(ldc=K * T - 1) == E and win(ldt=K - 1) == E
    assert win(n0=0, n1=40, ldc=(1 << 31) // 40 + 1) == E                   # (n1 - n0) ld_cost >= 2^31
    assert win(ldc=1 << 31) == E
    assert win(smin=-1) == E and win(smin=T) == E
    assert win(lm=None) == E
    assert win(lm=moves(math.nan, 0.0, 0.0)) == E and win(lm=moves(0.0, math.inf, 0.0)) == E
    assert win(lm=moves(NINF, NINF, NINF)) == E
    for k in ("c", "v", "lt", "li", "ps", "ns", "on", "ln", "ct", "st", "en", "ex", "lk"):
        assert win(**{k: None}) == E, k
    assert win(ws=None) == E and win(nb=nb - 1) == E and win(nb=0) == E


def test_frame_costs_rejects_bad_arguments_on_the_host():
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, F, K, T = 40, 9, 5, 3

    def fc(x=fake, ldx=F, n=n, n0=0, n1=10, F=F, K=K, T=T, mu=fake, ldm=F, lv=fake, ldl=F, c=fake, ldc=K * T):
        return lib.abcd_frame_costs(x, ldx, n, n0, n1, F, K, T, mu, ldm, lv, ldl, c, ldc, None)

    assert fc(n0=-1) == E and fc(n0=10) == E and fc(n1=n + 1) == E and fc(n=0, n0=0, n1=0) == E
    assert fc(F=0, ldx=1, ldm=1, ldl=1) == E and fc(ldx=F - 1) == E and fc(ldm=F - 1) == E and fc(ldl=F - 1) == E
    assert fc(ldc=K * T - 1) == E and fc(K=0) == E and fc(K=1025, ldc=1025 * T) == E and fc(T=0) == E
    assert fc(T=16384, ldc=K * 16384) == E
    assert fc(n1=40, ldc=(1 << 31) // 40 + 1) == E
    for k in ("x", "mu", "lv", "c"):
        assert fc(**{k: None}) == E, k


def test_operators_are_registered_with_their_schemas():
    from modules import ops
    assert hasattr(torch.ops.abcd, "frame_costs") and hasattr(torch.ops.abcd, "warp_segment_window")
    assert "frame_costs" in ops.OPS and "frame_costs" not in ops.STATEFUL_OPS
    assert "warp_segment_window" in ops.STATEFUL_OPS and "warp_segment_window" not in ops.OPS
    assert "frame_costs" in ops.registered()
    assert "!" not in str(torch.ops.abcd.frame_costs.default._schema)
    schema = str(torch.ops.abcd.warp_segment_window.default._schema)
    assert "!) state" in schema and "!)? W" in schema, schema               # the state and W are mutated, nothing else
    assert schema.count("!") == 2
    assert callable(ops.warp_segment_state)
    # the fakes give the shapes without a device
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        c = torch.ops.abcd.frame_costs(torch.empty(40, 9), torch.empty(15, 9), torch.empty(15, 9), 5, 8, 20)
        assert tuple(c.shape) == (12, 15) and c.dtype == torch.float32
        out = torch.ops.abcd.warp_segment_window(c, 8, 20, 40, 5, torch.empty(15), [0.0, 0.0, 0.0], None, None, 0.0,
                                                 torch.empty(5, 5), torch.empty(5), 0,
                                                 torch.empty(64, dtype=torch.uint8), None)
        assert [tuple(t.shape) for t in out] == [(), ()] + [(40,)] * 7
        assert [t.dtype for t in out] == [torch.float64] + [torch.int32] * 5 + [torch.float64] * 3
    with pytest.raises(RuntimeError):                                       # no CPU path
        ops.frame_costs(torch.zeros(4, 9), torch.zeros(6, 9), torch.zeros(6, 9), 2, 0, 4)
    with pytest.raises(RuntimeError):
        ops.warp_segment_window(torch.zeros(4, 6), 0, 4, 4, 2, torch.zeros(6), [0.0, 0.0, 0.0], None, None, 0.0,
                                torch.zeros(2, 2), torch.zeros(2), 0, torch.zeros(4096, dtype=torch.uint8), None)


def test_segment_frames_warped_arguments():
    import inspect

    from modules import model as M, ops, segmentation
    sig = inspect.signature(segmentation.segment_frames_warped).parameters
    for name in ("log_moves", "transitions", "log_weight", "gap", "seg_bonus", "min_state", "chunk_frames"):
        assert name in sig, name
    assert sig["log_moves"].default == ops.DEFAULT_LOG_MOVES and sig["chunk_frames"].default is None
    doc = " ".join(segmentation.segment_frames_warped.__doc__.split())
    assert "4 chunk_frames steps K" in doc                                  # the peak-memory formula
    assert segmentation.default_chunk_frames(200, 128) * 4 * 200 * 128 <= segmentation.PLANE_BUDGET_BYTES
    assert segmentation.default_chunk_frames(16383, 1024) == max(1, segmentation.PLANE_BUDGET_BYTES // (4 * 16383 * 1024))
    assert hasattr(M.RNN_Variational_Decoder, "frame_costs")
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    T, K, F = 5, 4, 33
    protos = (torch.zeros(T, K, F), torch.zeros(T, K, F), torch.zeros(T, K))
    x = torch.zeros(4, F)

    def call(steps=3, **kw):
        return segmentation.segment_frames_warped(dec, protos, x, steps, **kw)

    # every rule of the function's own, decided before a device is asked for
    for bad, why in ((dict(steps=0), "steps"), (dict(steps=T + 1), "steps"),
                     (dict(min_state=-1), "min_state"), (dict(min_state=3), "min_state"),
                     (dict(steps=T, min_state=T), "min_state"),
                     (dict(chunk_frames=0), "chunk_frames"), (dict(chunk_frames=-4), "chunk_frames"),
                     (dict(log_moves=(0.0, 0.0)), "log_moves"), (dict(log_moves=(0.0, 0.0, 0.0, 0.0)), "log_moves"),
                     (dict(log_moves=(math.nan, 0.0, 0.0)), "log_moves"),
                     (dict(log_moves=(0.0, math.inf, 0.0)), "log_moves"),
                     (dict(log_moves=(NINF, NINF, NINF)), "log_moves"),
                     (dict(log_weight=torch.zeros(K + 1)), "log_weight"),
                     (dict(log_weight=torch.zeros(K - 1)), "log_weight")):
        with pytest.raises(ValueError, match=why):
            call(**bad)
    # the edges that are allowed get past the checks and stop at the device
    for good in (dict(steps=1), dict(steps=T, min_state=T - 1), dict(min_state=2), dict(chunk_frames=1),
                 dict(log_moves=(NINF, 0.0, NINF)), dict(log_weight=torch.zeros(K))):
        with pytest.raises(RuntimeError):                                   # a CPU tensor: no CPU path
            call(**good)


def test_segment_cli_warp_arguments(capsys):
    import segment
    base = ["c", "r", "t", "1", "--max_length", "9"]
    a = segment.get_parameters(base)
    assert a.warp is False and a.min_state == 0 and a.chunk_frames is None
    a = segment.get_parameters(base + ["--warp", "--moves", "1", "2", "1", "--min_state", "3", "--chunk_frames", "64",
                                       "--transitions", "t.csv"])
    assert a.warp and a.moves == [1.0, 2.0, 1.0] and a.min_state == 3 and a.chunk_frames == 64
    for bad, why in ((["--warp", "--posteriors"], "--warp cannot be combined with --posteriors"),
                     (["--warp", "--transitions", "t.csv", "--chain_posteriors"],
                      "--warp cannot be combined with --chain_posteriors"),
                     (["--warp", "--transitions", "t.csv", "--window_frames", "16"],
                      "--warp cannot be combined with --window_frames"),
                     (["--warp", "--refit_transitions", "1", "--transitions_out", "o.csv"],
                      "--warp cannot be combined with --refit_transitions"),
                     (["--warp", "--min_state", "9"], "--min_state must lie in"),
                     (["--warp", "--chunk_frames", "0"], "at least 1"),
                     (["--warp", "--moves", "0", "0", "0"], "not all zero"),
                     (["--min_state", "1"], "need --warp"),
                     (["--moves", "0", "1", "0"], "need --warp")):
        with pytest.raises(SystemExit):
            segment.get_parameters(base + bad)
        assert why in " ".join(capsys.readouterr().err.split()), bad
    assert segment.WARP_COLUMNS == ("last_state", "tempo")
    rows = segment.segment_rows("a.wav", [0, 5], [5, 4], [1, 0], [-1.0, -2.0], 16000, 400, 160, True, 16000,
                                warp=([11, 7], [2.4, 2.0], [-0.5, -0.25]))
    assert rows[1]["last_state"] == 7 and rows[1]["tempo"] == 2.0 and rows[0]["transition_score"] == -0.5
