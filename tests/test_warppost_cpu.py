"""The posteriors under the time-warped cut without a GPU:
the np.longdouble recursions of tests/warppost_cases.py against the enumeration
of every cover, labelling and move sequence, their identities at every shape,
the rigid programme they reduce to, EM on a planted alternation, and the host
side of the new entry points, operators, module functions and flags."""
import math

import numpy as np
import pytest
import torch

import chainpost_cases as CP
import warppost_cases as WP
import warpseg_cases as WS

NEG = -np.inf
NINF = -math.inf
SYMS = ("abcd_warp_posterior_plan", "abcd_warp_posterior_workspace_bytes", "abcd_warp_posterior_forward",
        "abcd_warp_posterior_backward")


def _tiny(seed, N, K, T, gap, nan_cell):
    g = np.random.default_rng(seed)
    cost = (g.random((N, T, K)) * 3.0).astype(np.float32)
    if nan_cell and N >= 2:
        cost[1, 0, 0] = np.nan
        cost[N - 1, T - 1, K - 1] = np.inf
    return dict(cost=cost, v=g.normal(0.0, 2.0, size=(T, K)).astype(np.float32),
                gap=g.normal(-2.0, 1.0, size=N).astype(np.float32) if gap else None,
                trans=g.normal(0.0, 1.0, size=(K, K)).astype(np.float32),
                init=g.normal(0.0, 1.0, size=K).astype(np.float32), enter=g.normal(0.0, 1.0, size=K).astype(np.float32))


@pytest.mark.parametrize("moves", ("default", "staystep", "identity"))
@pytest.mark.parametrize("gap", (False, True))
@pytest.mark.parametrize("N,K,T", [(1, 1, 1), (2, 2, 3), (3, 2, 2), (4, 2, 3), (4, 1, 3)])
def test_reference_is_the_enumeration(N, K, T, gap, moves):
    covered, counted = 0, 0.0
    for s_min in sorted({0, min(1, T - 1), T - 1}):
        for nan_cell in (False, True):
            for scale in WP.SCALES:
                d = _tiny(7 * N + K + T + s_min, N, K, T, gap, nan_cell)
                args = (d["cost"], d["v"], WP.MOVES[moves], d["enter"], d["gap"], 0.5, d["trans"], d["init"], s_min, scale)
                ref, want = WP.warp_posterior_reference(*args), WP.enumerate_covers(*args)
                tag = (N, K, T, gap, moves, s_min, nan_cell, scale)
                if want["log_z"] == NEG:
                    assert ref["log_z"] == NEG, tag
                else:
                    covered += 1
                    assert abs(ref["log_z"] - want["log_z"]) <= 1e-12 * max(1.0, abs(want["log_z"])), tag
                for key in ("post_k", "gap_post", "trans_counts", "init_counts", "move_counts"):
                    assert np.abs(ref[key] - want[key]).max() <= 1e-12, (tag, key)
                assert abs(ref["no_segment"] - want["no_segment"]) <= 1e-12, tag
                counted += want["move_counts"].sum() + want["trans_counts"].sum()
                if moves != "default":                                   # a disabled move is never counted
                    assert (ref["move_counts"][:, 2] == 0.0).all()
    assert covered > 0
    if N >= 3 and T >= 2:
        assert counted > 0.0                                              # the counts are not vacuous


@pytest.mark.parametrize("kind", WP.PROG_KINDS)
@pytest.mark.parametrize("KT", WP.PROG_KT, ids=lambda v: f"k{v[0]}t{v[1]}")
@pytest.mark.parametrize("N", WP.PROG_N)
def test_identities_hold_on_the_reference(N, KT, kind):
    K, T = KT
    for s_min, scale in ((0, 1.0), (min(2, T - 1), 0.25)):
        r = WP.reference_of(N, K, T, kind, "default", s_min, scale)
        ids = WP.identities(r)
        if kind == "nopath":
            assert r["log_z"] == NEG
        if r["log_z"] == NEG:                                             # no cover (nopath; s_min beyond a short N)
            for key in ("post_k", "gap_post", "trans_counts", "init_counts", "move_counts"):
                assert (r[key] == 0.0).all(), key
            assert max(ids.values()) == 0.0
            continue
        # float64 copies of longdouble values: a rounding of 2^-53 per summed entry
        sums = 2.0 ** -52 * (N + 1) * K * (1.0 + abs(r["log_z"]))
        assert ids["bg0"] <= 2.0 ** -50 * (1.0 + abs(r["log_z"])), (ids, N, K, T, kind)
        assert ids["cover"] <= sums and ids["onsets"] <= sums * K and ids["moves"] <= sums * T, (ids, N, K, T, kind)
        d = WS.prog_inputs(N, K, T, kind)
        best = WS.prog_reference(d, "default", s_min)["path_score"]
        if scale == 1.0:
            assert r["log_z"] >= best - WP.lattice_bar(N, K, T, r["lattice"])


@pytest.mark.parametrize("N,K,T,kind,s_min", [(33, 2, 3, "random", 0), (33, 33, 37, "gaps", 2), (70, 65, 20, "random", 0),
                                              (33, 130, 5, "zeros", 1), (70, 2, 3, "holes", 1)])
def test_step_only_is_the_rigid_reference(N, K, T, kind, s_min):
    d = WS.prog_inputs(N, K, T, kind)
    for scale in WP.SCALES:
        r = WP.warp_posterior_reference(d["cost"], d["v"], WP.MOVES["identity"], None, d["gap"], d["bonus"], d["trans"],
                                        d["init"], s_min, scale)
        v64 = d["v"].astype(np.float64)
        table = WP.rigid_table64(d["cost"], d["v"], WS.softplus(v64), WS.softplus(-v64))
        c = CP.chain_posterior_reference(table, s_min + 1, d["trans"], d["init"], d["gap"], d["bonus"], scale,
                                         want_table=False)
        bar = WP.lattice_bar(N, K, T, r["lattice"]) + CP.lattice_bar(N, T, K, c["lattice"])
        assert (r["log_z"] == NEG) == (c["log_z"] == NEG)
        if r["log_z"] > NEG:
            assert abs(r["log_z"] - c["log_z"]) <= bar
        for a, b in ((r["lattice"], c["lattice"]), (r["lattice_g"], c["lattice_g"])):
            assert np.array_equal(np.isneginf(a), np.isneginf(b))
            fin = np.isfinite(b)
            assert np.abs(a[fin] - b[fin]).max() <= bar
        assert np.abs(r["post_k"] - c["post_k"]).max() <= 5 * bar and np.abs(r["gap_post"] - c["gap_post"]).max() <= 5 * bar
        assert (np.abs(r["trans_counts"] - c["trans_counts"]) <= 5 * bar * (1 + c["trans_counts"])).all()
        assert (np.abs(r["init_counts"] - c["init_counts"]) <= 5 * bar * (1 + c["init_counts"])).all()
        assert (r["move_counts"][:, (0, 2)] == 0.0).all()


def test_refit_warp_em_climbs_on_a_planted_alternation():
    from modules import segmentation
    from modules.sequence import TransitionModel
    recs = WP.em_recordings()
    K = recs[0]["v"].shape[1]
    bars = []

    def fn(rec, model, log_moves):
        out = WP.em_posterior_fn()(rec, model, log_moves)
        bars.append(WP.lattice_bar(rec["cost"].shape[0], K, rec["v"].shape[0], out["lattice"]))
        return out
    model = TransitionModel(K)
    start = (math.log(0.3), math.log(0.7), NINF)
    totals, lm = segmentation.refit_warp_em(fn, recs, model, start, WP.EM_ITERS + 1, 0.0, move_smoothing=0.0)
    assert len(totals) == WP.EM_ITERS + 1 and len(lm) == 3
    slack = len(recs) * max(bars)
    for a, b in zip(totals[:-1], totals[1:]):
        assert b >= a - slack, totals
    assert totals[-1] > totals[0]
    assert lm[2] == NINF and abs(math.exp(lm[0]) + math.exp(lm[1]) - 1.0) <= 1e-12
    assert math.exp(lm[0]) > 0.3                                          # half the segments are played at half speed
    p = model.log_trans.double().exp()
    assert float(p[0, 1]) > 0.9 and float(p[1, 0]) > 0.9                  # the alternation is found
    tc, ic = model.last_counts
    assert tuple(tc.shape) == (K, K) and abs(float(ic.sum()) - len(recs)) <= 1e-9
    # the moves alone, and the moves kept
    totals2, lm2 = segmentation.refit_warp_em(fn, recs, None, start, 2, 0.0, move_smoothing=0.0)
    assert totals2[1] >= totals2[0] - slack and lm2[2] == NINF
    model3 = TransitionModel(K)
    _, lm3 = segmentation.refit_warp_em(fn, recs, model3, start, 1, 0.0, fit_moves=False)
    assert tuple(lm3) == start


def test_new_entry_points_are_declared_bound_exported_and_hashed():
    from modules import _native as N
    from test_host import header_symbols
    for s in SYMS:
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.library_hash() == N.source_hash()


def test_workspace_queries_and_plan():
    import ctypes
    from modules import _native as N
    lib = N.lib()
    ws = lib.abcd_warp_posterior_workspace_bytes
    assert ws(0, 1, 1) > 0 and ws(-1, 1, 1) == 0
    assert ws(10, 1024, 1) > 0 and ws(10, 1025, 1) == 0 and ws(10, 0, 1) == 0
    assert ws(10, 1, 16383) > 0 and ws(10, 1, 16384) == 0 and ws(10, 1, 0) == 0
    assert ws(10, 1024, 16383) > 0 and ws(10, 1024, 16384) == 0
    assert ws((1 << 31) // 8 - 2, 8, 1) > 0 and ws((1 << 31) // 8 - 1, 8, 1) == 0
    n, K, T = 15000, 128, 200
    words = 2 * (n + 1) + 5 * (n + 1) * K + 4 * K * T + K * K + 4 * K + 4
    assert 8 * words <= ws(n, K, T) <= 8 * words + 256
    from modules import ops
    assert ops._warp_posterior_words(n, K, T) == words - 4
    res, thr, lds = N.c_int(-1), N.c_int(-1), N.c_size_t(0)
    for K, want in ((1, 1), (128, 1), (129, 0), (1024, 0)):
        assert lib.abcd_warp_posterior_plan(K, 5, ctypes.byref(res), ctypes.byref(thr), ctypes.byref(lds)) == 0
        assert res.value == want and thr.value == 1024
        assert lds.value == 40 * K + 40 * 1024 + (4 * K * (K + 1) if want else 0)
        assert lds.value <= 160 * 1024
    assert lib.abcd_warp_posterior_plan(128, 5, None, None, None) == 0
    for K, T in ((0, 5), (1025, 5), (5, 0), (5, 16384), (1024, 16384)):
        assert lib.abcd_warp_posterior_plan(K, T, None, None, None) == N.ABCD_EINVAL


def test_entry_points_reject_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, K, T = 40, 5, 3
    nb = lib.abcd_warp_posterior_workspace_bytes(n, K, T)
    ok_moves = (N.c_double * 3)(*WP.MOVES["default"])

    def moves(*v):
        return (N.c_double * 3)(*v)

    def fw(c=fake, ldc=K * T, n0=0, n1=10, n=n, K=K, T=T, v=fake, lm=ok_moves, bonus=0.0, scale=1.0, lt=fake, ldt=K,
           li=fake, smin=0, alpha=None, lda=K * T, lz=fake, ws=fake, nb=nb):
        return lib.abcd_warp_posterior_forward(c, ldc, n0, n1, n, K, T, v, lm, None, None, bonus, scale, lt, ldt, li,
                                               smin, alpha, lda, lz, ws, nb, None)

    def bw(c=fake, ldc=K * T, n0=30, n1=40, n=n, K=K, T=T, v=fake, lm=ok_moves, scale=1.0, lt=fake, ldt=K, li=fake,
           smin=0, alpha=None, lda=K * T, pk=fake, gp=fake, tc=None, ic=None, mc=None, ws=fake, nb=nb):
        return lib.abcd_warp_posterior_backward(c, ldc, n0, n1, n, K, T, v, lm, None, None, 0.0, scale, lt, ldt, li,
                                                smin, alpha, lda, pk, gp, tc, ic, mc, ws, nb, None)

    for f in (fw, bw):
        assert f(n0=-1) == E and f(n0=10, n1=10) == E and f(n0=41, n1=40) == E and f(n1=n + 1) == E
        assert f(n=-1) == E and f(n=0, n0=0, n1=1) == E
        assert f(K=0, ldc=T, ldt=1) == E and f(K=1025, ldc=1025 * T, ldt=1025, nb=1 << 40) == E
        assert f(T=0) == E and f(T=16384, ldc=K * 16384, nb=1 << 40) == E
        assert f(ldc=K * T - 1) == E and f(ldt=K - 1) == E and f(ldc=1 << 31) == E
        assert f(smin=-1) == E and f(smin=T) == E
        assert f(lm=None) == E and f(lm=moves(math.nan, 0.0, 0.0)) == E and f(lm=moves(0.0, math.inf, 0.0)) == E
        assert f(lm=moves(NINF, NINF, NINF)) == E
        for scale in (0.0, -1.0, math.inf, math.nan):
            assert f(scale=scale) == E, scale
        for k in ("c", "v", "lt", "li"):
            assert f(**{k: None}) == E, k
        assert f(ws=None) == E and f(nb=nb - 1) == E and f(nb=0) == E
        assert f(alpha=fake, lda=K * T - 1) == E
    assert fw(lz=None) == E
    assert bw(pk=None) == E and bw(gp=None) == E
    assert bw(tc=fake) == E and bw(ic=fake) == E                            # the bigram buffers come together
    assert bw(mc=fake) == E                                                   # move counts need alpha


def test_operators_are_registered_with_their_schemas():
    from modules import ops
    for name in ("warp_posterior_forward", "warp_posterior_backward"):
        assert hasattr(torch.ops.abcd, name) and name in ops.STATEFUL_OPS and name not in ops.OPS
    schema = str(torch.ops.abcd.warp_posterior_forward.default._schema)
    assert "!) state" in schema and "!)? alpha" in schema and schema.count("!") == 2, schema
    schema = str(torch.ops.abcd.warp_posterior_backward.default._schema)
    assert "!) state" in schema and schema.count("!") == 1, schema
    assert callable(ops.warp_posterior_state) and callable(ops.warp_posterior_planes)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        c = torch.empty(12, 15)
        args = (40, 5, torch.empty(15), [0.0, 0.0, 0.0], None, None, 0.0, 1.0, torch.empty(5, 5), torch.empty(5), 0,
                torch.empty(64, dtype=torch.uint8))
        lz = torch.ops.abcd.warp_posterior_forward(c, 8, 20, *args, None)
        assert tuple(lz.shape) == () and lz.dtype == torch.float64
        out = torch.ops.abcd.warp_posterior_backward(c, 8, 20, *args, None, True, False)
        assert [tuple(t.shape) for t in out] == [(2, 41, 5), (41,), (5, 5), (5,), (0, 3)]
        assert all(t.dtype == torch.float64 for t in out)
    # the plain checks come first and need no device; then there is no CPU path
    c, v, lt, li = torch.zeros(4, 6), torch.zeros(6), torch.zeros(2, 2), torch.zeros(2)
    st = torch.zeros(4096, dtype=torch.uint8)

    def fwd(cost=c, n0=0, n1=4, n=4, K=2, v=v, moves=(0.0, 0.0, 0.0), scale=1.0, lt=lt, li=li, s_min=0, state=st,
            alpha=None):
        return ops.warp_posterior_forward(cost, n0, n1, n, K, v, list(moves), None, None, 0.0, scale, lt, li, s_min,
                                          state, alpha)
    for bad, why in ((dict(scale=0.0), "scale"), (dict(scale=math.inf), "scale"), (dict(moves=(NINF, NINF, NINF)), "log_moves"),
                     (dict(n0=2, n1=2), "n0"), (dict(s_min=3), "s_min"), (dict(v=torch.zeros(5)), "proto_offset_logits"),
                     (dict(lt=torch.zeros(2, 3)), "log_trans"), (dict(cost=torch.zeros(3, 6)), "cost"),
                     (dict(alpha=torch.zeros(4, 6)), "alpha"), (dict(alpha=torch.zeros(3, 6, dtype=torch.float64)), "alpha"),
                     (dict(state=torch.zeros(64)), "state")):
        with pytest.raises(ValueError, match=why):
            fwd(**bad)
    with pytest.raises(ValueError, match="want_moves needs alpha"):
        ops.warp_posterior_backward(c, 0, 4, 4, 2, v, [0.0, 0.0, 0.0], None, None, 0.0, 1.0, lt, li, 0, st, None, False,
                                    True)
    with pytest.raises(RuntimeError):
        fwd()
    with pytest.raises(RuntimeError):
        ops.warp_posterior_backward(c, 0, 4, 4, 2, v, [0.0, 0.0, 0.0], None, None, 0.0, 1.0, lt, li, 0, st, None, True,
                                    False)
    assert ops._warp_posterior_words(4, 2, 3) == 2 * 5 + 5 * 5 * 2 + 4 * 6 + 4 + 8


def test_segment_warp_posteriors_arguments():
    import inspect

    from modules import model as M, ops, segmentation
    sig = inspect.signature(segmentation.segment_warp_posteriors).parameters
    warped = inspect.signature(segmentation.segment_frames_warped).parameters
    assert list(sig)[:len(warped)] == list(warped)                          # segment_frames_warped's arguments first
    for name, default in (("temperature", 1.0), ("want_counts", False), ("want_moves", False), ("with_segments", False)):
        assert sig[name].default == default, name
    assert sig["log_moves"].default == ops.DEFAULT_LOG_MOVES
    assert segmentation.ALPHA_BUDGET_BYTES == 8 << 30
    em = inspect.signature(segmentation.refit_warp_em).parameters
    assert list(em) == ["posterior_fn", "recordings", "model", "log_moves", "n_iter", "pseudo_count", "move_smoothing",
                        "fit_moves", "temperature"]
    assert em["move_smoothing"].default == 1.0 and em["fit_moves"].default is True and em["temperature"].default == 1.0
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    T, K, F = 5, 4, 33
    protos = (torch.zeros(T, K, F), torch.zeros(T, K, F), torch.zeros(T, K))
    x = torch.zeros(4, F)

    def call(steps=3, frames=x, **kw):
        return segmentation.segment_warp_posteriors(dec, protos, frames, steps, **kw)

    for bad, why in ((dict(steps=0), "steps"), (dict(steps=T + 1), "steps"), (dict(min_state=-1), "min_state"),
                     (dict(min_state=3), "min_state"), (dict(chunk_frames=0), "chunk_frames"),
                     (dict(log_moves=(0.0, 0.0)), "log_moves"), (dict(log_moves=(NINF, NINF, NINF)), "log_moves"),
                     (dict(log_weight=torch.zeros(K + 1)), "log_weight"), (dict(temperature=0.0), "temperature"),
                     (dict(temperature=-2.0), "temperature"), (dict(temperature=math.inf), "temperature"),
                     (dict(temperature=math.nan), "temperature")):
        with pytest.raises(ValueError, match=why):
            call(**bad)
    # the aH plane of want_moves: 8 N K steps bytes against the budget, decided before any device work
    long = torch.zeros(1, F).expand((segmentation.ALPHA_BUDGET_BYTES // (8 * K * 3)) + 1, F)
    with pytest.raises(ValueError, match="ALPHA_BUDGET_BYTES"):
        call(frames=long, want_moves=True)
    with pytest.raises(RuntimeError):                                       # without the plane the budget does not apply
        call(frames=long)
    for good in (dict(steps=1), dict(steps=T, min_state=T - 1), dict(temperature=4.0), dict(want_moves=True),
                 dict(want_counts=True, with_segments=True)):
        with pytest.raises(RuntimeError):                                   # a CPU tensor: no CPU path
            call(**good)


def test_segment_cli_warp_posterior_arguments(capsys):
    import segment
    base = ["c", "r", "t", "1", "--max_length", "9"]
    a = segment.get_parameters(base)
    assert a.warp_posteriors is False and a.warp_refit == 0 and a.moves_out is None and a.keep_moves is False
    a = segment.get_parameters(base + ["--warp", "--warp_posteriors", "--posterior_temperature", "4", "--curves_dir", "c",
                                       "--recordings_out", "r.csv"])
    assert a.warp and a.warp_posteriors and a.posterior_temperature == 4.0
    a = segment.get_parameters(base + ["--warp", "--warp_refit", "3", "--moves_out", "m.csv"])
    assert a.warp_refit == 3 and a.moves_out == "m.csv" and a.transitions_out is None
    a = segment.get_parameters(base + ["--warp", "--transitions", "t.csv", "--warp_refit", "2", "--transitions_out", "o.csv",
                                       "--keep_moves"])
    assert a.keep_moves and a.transitions_out == "o.csv"
    for bad, why in ((["--warp_posteriors"], "need --warp"),
                     (["--warp_refit", "2", "--moves_out", "m.csv"], "need --warp"),
                     (["--warp", "--moves_out", "m.csv"], "need --warp_refit"),
                     (["--warp", "--keep_moves"], "need --warp_refit"),
                     (["--warp", "--warp_refit", "-1"], "must not be negative"),
                     (["--warp", "--warp_refit", "1"], "--moves_out"),
                     (["--warp", "--warp_refit", "1", "--moves_out", "m.csv", "--keep_moves"], "not both"),
                     (["--warp", "--warp_refit", "1", "--keep_moves"], "nothing to fit"),
                     (["--warp", "--warp_refit", "1", "--moves_out", "m.csv", "--transitions", "t.csv"], "go together"),
                     (["--warp", "--warp_refit", "1", "--moves_out", "m.csv", "--transitions_out", "o.csv"], "go together"),
                     (["--warp", "--posterior_temperature", "2"], "need --posteriors"),
                     # the four refusals of --warp keep their text
                     (["--warp", "--posteriors"], "--warp cannot be combined with --posteriors: the time-warped programme "
                                                  "gives the best cut only and needs no table in windows"),
                     (["--warp", "--transitions", "t.csv", "--chain_posteriors"],
                      "--warp cannot be combined with --chain_posteriors: the time-warped programme gives the best cut "
                      "only and needs no table in windows"),
                     (["--warp", "--transitions", "t.csv", "--window_frames", "16"],
                      "--warp cannot be combined with --window_frames: the time-warped programme gives the best cut only "
                      "and needs no table in windows"),
                     (["--warp", "--refit_transitions", "1", "--transitions_out", "o.csv"],
                      "--warp cannot be combined with --refit_transitions: the time-warped programme gives the best cut "
                      "only and needs no table in windows"),
                     (["--refit_transitions", "1"], "--refit_transitions and --transitions_out go together")):
        with pytest.raises(SystemExit):
            segment.get_parameters(base + bad)
        assert why in " ".join(capsys.readouterr().err.split()), bad
    assert segment.WARP_POSTERIOR_COLUMNS == ("onset_posterior", "offset_posterior", "occupancy")
    rows = segment.segment_rows("a.wav", [0, 5], [5, 4], [1, 0], [-1.0, -2.0], 16000, 400, 160, True, 16000,
                                warp=([11, 7], [2.4, 2.0], None), warp_posteriors=([0.9, 0.8], [0.7, 0.6], [0.5, 0.4]))
    assert rows[1]["onset_posterior"] == 0.8 and rows[0]["offset_posterior"] == 0.7 and rows[1]["occupancy"] == 0.4


def test_writer_with_warp_posterior_columns_and_moves(tmp_path):
    import os

    import pandas as pd
    import segment
    rows = segment.segment_rows("a.wav", [0], [5], [1], [-1.0], 16000, 400, 160, True, 16000,
                                warp=([4], [1.0], None), warp_posteriors=([0.9], [0.7], [0.5]))
    out, mout = os.path.join(str(tmp_path), "s.csv"), os.path.join(str(tmp_path), "m.csv")
    assert segment.write_segments(out, rows, warp=True, warp_posteriors=True, moves_out=mout, moves=[0.25, 0.5, 0.25]) == 1
    df = pd.read_csv(out)
    assert list(df.columns) == list(segment.COLUMNS) + list(segment.WARP_COLUMNS) + list(segment.WARP_POSTERIOR_COLUMNS)
    mv = pd.read_csv(mout)
    assert list(mv.columns) == ["stay", "step", "skip"] and mv.iloc[0].tolist() == [0.25, 0.5, 0.25]
