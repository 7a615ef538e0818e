"""Syntax-aware segmentation, checked on the CPU: the float64 reference of
``syntax_cases.py`` (it reduces to ``span_cases.viterbi_reference`` under a
context-free chain; the planted alternation; brute-force enumeration on tiny
tables), the new entry points' surface (header, binding, workspace limits,
host-side argument checks, operators, methods), ``count_transitions`` and
``segment.py``'s new arguments."""
import itertools

import numpy as np
import pytest
import torch

import span_cases as SP
import syntax_cases as SX

NEG = SX.NEG


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
def test_reference_reduces_to_the_context_free_programme():
    """All rows of log_trans and log_init equal one log_softmax(lw): the same
    segments as viterbi_reference on max_k (T + lw), the path score within 1e-9
    relative.  Random tables hold no exact ties."""
    g = np.random.default_rng(5)
    seen_gap = 0
    for trial in range(200):
        N, D, K = int(g.integers(1, 41)), int(g.integers(1, 9)), int(g.integers(1, 6))
        T = SX.random_table(g, N, D, K)
        p = SX.log_softmax(g.normal(0.0, 1.0, size=K)).astype(np.float32)     # what the chain holds: fp32
        gap = g.normal(-4.0, 1.0, size=N).astype(np.float32) if trial % 2 else None
        d_min = int(g.integers(1, D + 1))
        bonus = float(g.normal()) if trial % 3 == 0 else 0.0
        ref = SX.chain_reference(T, d_min, np.tile(p[None, :], (K, 1)), p, gap, bonus)
        score, cat = SX.context_free(T, p.astype(np.float64))
        want = SP.viterbi_reference(score, cat, d_min, gap, bonus)
        assert ref["onset"] == want["onset"] and ref["length"] == want["length"] and ref["cat"] == want["cat"], trial
        if want["path_score"] == NEG:
            assert ref["path_score"] == NEG
            continue
        assert abs(ref["path_score"] - want["path_score"]) <= 1e-9 * abs(want["path_score"]), trial
        assert ref["score"] == [float(T[s + d, d - 1, k]) for s, d, k in zip(ref["onset"], ref["length"], ref["cat"])]
        assert ref["link"] == [float(p[k]) for k in ref["cat"]]
        total, mag = SX.terms_of(ref, N, gap, bonus)
        assert abs(ref["path_score"] - total) <= 1e-9 * max(mag, 1e-300)
        seen_gap += gap is not None and sum(ref["length"]) < N
    assert seen_gap > 0


def test_planted_alternation():
    c = SX.planted_alternation()
    N = c["N"]
    score, cat = SX.context_free(c["table"], c["lw"])
    free = SP.viterbi_reference(score, cat, 1, None, 0.0)
    assert free["length"] == [SX.ALT_L] * SX.ALT_SEGMENTS and free["cat"] == [0] * SX.ALT_SEGMENTS
    ref = SX.chain_reference(c["table"], 1, c["trans"], c["init"])
    assert ref["onset"] == free["onset"] and ref["length"] == free["length"]
    assert ref["cat"] == [i % 2 for i in range(SX.ALT_SEGMENTS)]           # the lowest k wins the tie of the two phases
    assert ref["link"][0] == float(c["init"][0]) and set(ref["link"][1:]) == {float(c["trans"][0, 1])}
    total, mag = SX.terms_of(ref, N, None, 0.0)
    assert abs(ref["path_score"] - total) <= 1e-9 * mag


def _brute(T, d_min, lt, li, gap, bonus):
    """Every labelled cover of N <= 6 frames: the best total (summed in any
    order: integers) over all of them."""
    N, D, K = T.shape[0] - 1, T.shape[1], T.shape[2]
    best = NEG

    def walk(n, total, last):
        nonlocal best
        if n == N:
            best = max(best, total)
            return
        if gap is not None:
            walk(n + 1, total + float(gap[n]), last)
        for d in range(d_min, min(D, N - n) + 1):
            for k in range(K):
                link = li[k] if last < 0 else lt[last, k]
                v = total + link + T[n + d, d - 1, k] + bonus
                if v > NEG:
                    walk(n + d, v, k)
    walk(0, 0.0, -1)
    return best


def test_reference_is_brute_force_on_integer_tables():
    g = np.random.default_rng(17)
    unreachable = 0
    for N, D, K in ((1, 1, 1), (3, 2, 2), (5, 3, 2), (6, 2, 3), (6, 6, 2), (4, 3, 3)):
        for d_min, use_gap, bonus, zeros in itertools.product((1, 2), (False, True), (0.0, -1.0), (False, True)):
            if d_min > D:
                continue
            T = SX.mask_impossible(g.integers(-3, 2, size=(N + 1, D, K)).astype(np.float64))
            T[g.random(T.shape) < 0.1] = NEG
            lt = g.integers(-2, 1, size=(K, K)).astype(np.float64)
            li = g.integers(-2, 1, size=K).astype(np.float64)
            if zeros:
                lt[g.random(lt.shape) < 0.4] = NEG
            gap = g.integers(-3, 0, size=N).astype(np.float32) if use_gap else None
            ref = SX.chain_reference(T, d_min, lt, li, gap, bonus)
            want = _brute(T, d_min, lt, li, gap, bonus)
            assert ref["path_score"] == want, (N, D, K, d_min, use_gap, bonus, zeros)
            unreachable += want == NEG
            if want > NEG:
                total, _ = SX.terms_of(ref, N, gap, bonus)
                assert total == want
                at = 0
                for s, d, k in zip(ref["onset"], ref["length"], ref["cat"]):
                    assert s >= at and d_min <= d <= D and 0 <= k < K
                    at = s + d
                assert at <= N and (use_gap or at == N)
    assert unreachable > 0


def test_reference_tie_rules():
    # two categories, identical everything: the initial term and the lowest indices win
    T = SX.mask_impossible(np.zeros((3, 2, 2)))
    z2, z = np.zeros((2, 2)), np.zeros(2)
    r = SX.chain_reference(T, 1, z2, z)
    assert r["length"] == [1, 1] and r["cat"] == [0, 0] and r["path_score"] == 0.0     # the smallest d, the lowest k
    r = SX.chain_reference(T, 1, z2, z, gap=np.zeros(2, dtype=np.float32))
    assert r["length"] == [] and r["path_score"] == 0.0                                   # "no segment" wins at the end
    r = SX.chain_reference(T, 1, z2, z, gap=np.array([0.0, -1.0], dtype=np.float32))
    assert (r["onset"], r["length"], r["link"]) == ([1], [1], [0.0])                      # the initial term after a gap
    r = SX.chain_reference(T[:1], 1, z2, z)
    assert r["path_score"] == 0.0 and r["onset"] == []                                    # N = 0
    r = SX.chain_reference(T, 1, np.full((2, 2), NEG), np.full(2, NEG))
    assert r["path_score"] == NEG and r["onset"] == []


# ----------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------
SYMS = ("abcd_span_table_workspace_bytes", "abcd_span_table", "abcd_span_chain_plan",
        "abcd_span_chain_workspace_bytes", "abcd_span_chain_viterbi")


def test_new_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in SYMS:
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.library_hash() == N.source_hash()
    wt = N.lib().abcd_span_table_workspace_bytes
    assert wt(15000, 200, 128, 128) >= 200 * 128 * 8
    assert wt(0, 1, 1, 1) > 0 and wt(-1, 1, 1, 1) == 0 and wt(4, 0, 1, 1) == 0 and wt(4, 1, 0, 1) == 0
    assert wt(4, 16383, 1, 1) > 0 and wt(4, 16384, 1, 1) == 0
    assert wt(4, 3, 5, 5) > 0 and wt(4, 3, 5, 4) == 0 and wt(4, 3, 5, 8) > 0                 # ld_k >= P
    assert wt((1 << 31) // 8 - 2, 8, 1, 1) > 0 and wt((1 << 31) // 8 - 1, 8, 1, 1) == 0     # (N + 1) D < 2^31
    assert wt((1 << 31) // 64 - 2, 8, 8, 8) > 0 and wt((1 << 31) // 64 - 1, 8, 8, 8) == 0   # (N + 1) D ld_k < 2^31
    assert wt((1 << 31) // 64 - 1, 8, 7, 8) == 0 and wt(1 << 40, 1, 1, 1) == 0
    wc = N.lib().abcd_span_chain_workspace_bytes
    assert wc(15000, 200, 128) >= 15001 * 128 * 16
    assert wc(0, 1, 1) > 0 and wc(-1, 1, 1) == 0 and wc(4, 0, 1) == 0 and wc(4, 1, 0) == 0
    assert wc(4, 1, 1024) > 0 and wc(4, 1, 1025) == 0 and wc(4, 16383, 1) > 0 and wc(4, 16384, 1) == 0
    assert wc((1 << 31) // 64 - 2, 8, 8) > 0 and wc((1 << 31) // 64 - 1, 8, 8) == 0 and wc(1 << 40, 1, 1) == 0


def test_chain_plan_is_a_pure_function():
    from modules import _native as N
    lib = N.lib()
    res, thr, lds = N.c_int(-1), N.c_int(-1), N.ctypes.c_size_t(0)
    for K, want in ((1, 1), (2, 1), (33, 1), (65, 1), (128, 1), (129, 0), (130, 0), (256, 0), (257, 0), (1024, 0)):
        assert lib.abcd_span_chain_plan(K, 200, N.ctypes.byref(res), N.ctypes.byref(thr), N.ctypes.byref(lds)) == 0
        waves = 16 if K <= 256 else 4               # the partial results of every wave must fit LDS
        assert res.value == want and thr.value == 64 * waves, K
        per_k = (2 + waves) * 8 + waves * 4         # W, log_init, the partial maxima; the partial arguments
        assert lds.value == K * per_k + (K * K * 4 if want else 0) and lds.value <= 160 * 1024
    assert lib.abcd_span_chain_plan(128, 1, None, None, None) == 0
    E = N.ABCD_EINVAL
    for K, D in ((0, 5), (1025, 5), (4, 0), (4, 16384)):
        assert lib.abcd_span_chain_plan(K, D, None, None, None) == E


def test_entry_points_reject_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, F, P, D = 9, 4, 5, 3
    nb = lib.abcd_span_table_workspace_bytes(n, D, P, P)

    def table(x=fake, ldx=F, n=n, F=F, P=P, D=D, Tp=D, mu=fake, ldm=F, lv=fake, ldl=F, o=fake, lw=None, tb=fake, ldk=P,
              ss=None, sc=None, lds=D, ws=fake, nb=nb):
        return lib.abcd_span_table(x, ldx, n, F, P, D, Tp, mu, ldm, lv, ldl, o, lw, tb, ldk, ss, sc, lds, ws, nb, None)

    assert table(D=0, Tp=4) == E and table(D=16384, Tp=16384, lds=16384, nb=1 << 40) == E
    assert table(P=0) == E and table(F=0) == E and table(n=-1) == E
    assert table(n=(1 << 31) // 3, nb=1 << 40) == E                    # (N + 1) D >= 2^31
    assert table(n=(1 << 31) // 15, nb=1 << 40) == E                   # (N + 1) D ld_k >= 2^31
    assert table(n=(1 << 31) // 30, ldk=2 * P, nb=1 << 40) == E        # the stride counts, not P
    assert table(Tp=D - 1) == E
    assert table(ldx=F - 1) == E and table(ldm=F - 1) == E and table(ldl=F - 1) == E and table(ldk=P - 1) == E
    assert table(ss=fake, sc=fake, lds=D - 1) == E
    assert table(ss=fake) == E and table(sc=fake) == E                 # both or neither
    for k in ("x", "mu", "lv", "o", "tb"):
        assert table(**{k: None}) == E, k
    assert table(ws=None) == E and table(nb=nb - 1) == E and table(nb=0) == E
    # N = 0 is valid; with nowhere to write row 0 it needs no device
    nb0 = lib.abcd_span_table_workspace_bytes(0, D, P, P)
    assert table(n=0, x=None, mu=None, lv=None, o=None, tb=None, nb=nb0) == 0
    assert table(n=0, tb=None, ws=None, nb=nb0) == E

    K = P
    nv = lib.abcd_span_chain_workspace_bytes(n, D, K)

    def vit(tb=fake, ldk=K, n=n, D=D, K=K, dmin=1, gap=None, bonus=0.0, lt=fake, ldt=K, li=fake, ps=fake, ns=fake,
            on=fake, ln=fake, ct=fake, sv=fake, lk=fake, W=None, ws=fake, nb=nv):
        return lib.abcd_span_chain_viterbi(tb, ldk, n, D, K, dmin, gap, bonus, lt, ldt, li, ps, ns, on, ln, ct, sv, lk,
                                           W, ws, nb, None)

    assert vit(K=0, ldk=1, ldt=1) == E and vit(K=1025, ldk=1025, ldt=1025, nb=1 << 40) == E
    assert vit(dmin=0) == E and vit(dmin=D + 1) == E
    assert vit(D=0) == E and vit(D=16384, nb=1 << 40) == E and vit(n=-1) == E
    assert vit(n=(1 << 31) // 3, nb=1 << 40) == E and vit(n=(1 << 31) // 15, nb=1 << 40) == E
    assert vit(n=(1 << 31) // 30, ldk=2 * K, nb=1 << 40) == E
    assert vit(ldk=K - 1) == E and vit(ldt=K - 1) == E
    for k in ("tb", "lt", "li", "ps", "ns", "on", "ln", "ct", "sv", "lk"):
        assert vit(**{k: None}) == E, k
    assert vit(ws=None) == E and vit(nb=nv - 1) == E and vit(nb=0) == E
    nv0 = lib.abcd_span_chain_workspace_bytes(0, D, K)
    assert vit(n=0, tb=None, lt=None, li=None, ps=None, ns=None, on=None, ln=None, ct=None, sv=None, lk=None,
               nb=nv0) == 0
    assert vit(n=0, dmin=0, ps=None, ns=None, nb=nv0) == E


def test_ops_and_methods_exist():
    from modules import model as M, ops, segmentation
    from modules.sequence import TransitionModel
    for name in ("span_table", "span_chain_viterbi"):
        assert name in ops.OPS and hasattr(torch.ops.abcd, name)
    assert set(ops.registered()) == set(ops.OPS)
    schema = str(torch.ops.abcd.span_table.default._schema)
    assert schema.startswith("abcd::span_table(Tensor frames, Tensor proto_mu, Tensor proto_lv, Tensor "
                             "proto_offset_logits, Tensor? log_weight, SymInt P, SymInt D, bool want_best) -> "
                             "Tensor[]"), schema
    schema = str(torch.ops.abcd.span_chain_viterbi.default._schema)
    assert schema.startswith("abcd::span_chain_viterbi(Tensor table, SymInt d_min, Tensor? gap, float seg_bonus, "
                             "Tensor log_trans, Tensor log_init, bool want_w) -> Tensor[]"), schema
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a = (torch.empty(9, 4), torch.empty(15, 4), torch.empty(15, 4), torch.empty(15), None, 5, 3)
        tb, ss, sc = torch.ops.abcd.span_table(*a, True)
        assert tb.shape == (10, 3, 5) and tb.dtype == torch.float64
        assert ss.shape == sc.shape == (10, 3) and ss.dtype == torch.float64 and sc.dtype == torch.int32
        tb, ss, sc = torch.ops.abcd.span_table(*a, False)
        assert ss.shape == sc.shape == (0, 0)
        out = torch.ops.abcd.span_chain_viterbi(tb, 2, None, 0.0, torch.empty(5, 5), torch.empty(5), True)
        assert [tuple(t.shape) for t in out] == [(), (), (4,), (4,), (4,), (4,), (4,), (10, 5)]
        assert out[0].dtype == out[5].dtype == out[6].dtype == out[7].dtype == torch.float64
        assert out[1].dtype == out[4].dtype == torch.int32
    assert callable(M.RNN_Variational_Decoder.span_table)
    # no CPU fallback anywhere
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    protos = (torch.zeros(3, 4, 33), torch.zeros(3, 4, 33), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        dec.span_table(protos, torch.zeros(9, 33), 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        segmentation.segment_frames(dec, protos, torch.zeros(9, 33), 3, transitions=TransitionModel(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.span_table(torch.zeros(9, 4), torch.zeros(15, 4), torch.zeros(15, 4), torch.zeros(15), None, 5, 3, False)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.span_chain_viterbi(torch.zeros(10, 3, 5, dtype=torch.float64), 1, None, 0.0, torch.zeros(5, 5),
                               torch.zeros(5), False)


def test_count_transitions():
    from modules import segmentation
    tc, ic = segmentation.count_transitions([[0, 1, 1, 2], [], [2], [1, 0, 1]], 3)
    assert tc.dtype == ic.dtype == torch.float64
    assert tc.tolist() == [[0.0, 2.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]
    assert ic.tolist() == [1.0, 1.0, 1.0]
    tc, ic = segmentation.count_transitions([], 2)
    assert tc.tolist() == [[0.0, 0.0], [0.0, 0.0]] and ic.tolist() == [0.0, 0.0]
    tc, ic = segmentation.count_transitions([torch.tensor([1, 1, 1])], 2)
    assert tc.tolist() == [[0.0, 0.0], [0.0, 2.0]] and ic.tolist() == [0.0, 1.0]
    with pytest.raises(ValueError):
        segmentation.count_transitions([[0, 3]], 3)
    with pytest.raises(ValueError):
        segmentation.count_transitions([[-1]], 3)


def test_refit_transitions_counts_and_normalises():
    """Viterbi training with a segment function that ignores the model: the
    rows become (counts + c) normalised, the scores are summed per iteration."""
    from modules import segmentation
    from modules.sequence import TransitionModel
    paths = {"a": [0, 1, 0, 1], "b": [1, 0]}
    calls = []

    def segment_fn(rec, model):
        calls.append(rec)
        return dict(category=torch.tensor(paths[rec]), path_score=torch.tensor(-2.0, dtype=torch.float64))

    m = TransitionModel(2)
    totals = segmentation.refit_transitions(segment_fn, ["a", "b"], m, 2, 0.5)
    assert totals == [-4.0, -4.0] and calls == ["a", "b", "a", "b"]
    want_t = torch.tensor([[0.5, 2.5], [2.5, 0.5]], dtype=torch.float64) / 3.0
    want_i = torch.tensor([1.5, 1.5], dtype=torch.float64) / 3.0
    assert torch.allclose(m.log_trans.double().exp(), want_t, rtol=1e-6)
    assert torch.allclose(m.log_init.double().exp(), want_i, rtol=1e-6)
    assert m.last_counts[0].tolist() == [[0.0, 2.0], [2.0, 0.0]] and m.last_counts[1].tolist() == [1.0, 1.0]


def test_segment_frames_rejects_posteriors_with_transitions():
    from modules import model as M, segmentation
    from modules.sequence import TransitionModel
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    protos = (torch.zeros(3, 4, 33), torch.zeros(3, 4, 33), torch.zeros(3, 4))
    import unittest.mock as mock
    with mock.patch.object(segmentation.N, "require_gpu", lambda t: None):      # the argument check needs no device
        with pytest.raises(ValueError, match="posteriors"):
            segmentation.segment_frames(dec, protos, torch.zeros(9, 33), 3, posteriors=True,
                                        transitions=TransitionModel(4))


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def test_segment_cli_arguments():
    import segment
    base = ["c", "r", "t", "1", "--max_length", "9"]
    a = segment.get_parameters(base)
    assert a.transitions is None and a.refit_transitions == 0 and a.transitions_out is None
    a = segment.get_parameters(base + ["--transitions", "transitions.csv"])
    assert a.transitions == "transitions.csv" and a.refit_transitions == 0
    a = segment.get_parameters(base + ["--transitions", "t.csv", "--refit_transitions", "3", "--transitions_out",
                                       "new.csv"])
    assert (a.transitions, a.refit_transitions, a.transitions_out) == ("t.csv", 3, "new.csv")
    a = segment.get_parameters(base + ["--refit_transitions", "2", "--transitions_out", "new.csv"])
    assert a.transitions is None and a.refit_transitions == 2
    for bad in (["--transitions", "t.csv", "--posteriors"], ["--refit_transitions", "2"],
                ["--transitions_out", "new.csv"], ["--refit_transitions", "-1", "--transitions_out", "n.csv"],
                ["--refit_transitions", "1", "--transitions_out", "n.csv", "--posteriors"]):
        with pytest.raises(SystemExit):
            segment.get_parameters(base + bad)
    assert segment.SYNTAX_COLUMNS == ("transition_score", "context_free_category_ix", "changed")


def test_segment_rows_and_writer_with_syntax_columns(tmp_path):
    import os

    import pandas as pd

    import segment
    rows = segment.segment_rows("a.wav", [0, 5], [5, 4], [1, 2], [-1.5, -2.5], 1000, 8, 4, True, 100,
                                syntax=([-0.5, -0.25], [1, 0]))
    out = os.path.join(str(tmp_path), "segmented.csv")
    tr = pd.DataFrame({"from_ix": [0], "to_ix": [0], "probability": [1.0], "expected_count": [1.0]})
    tout = os.path.join(str(tmp_path), "transitions.csv")
    assert segment.write_segments(out, rows, syntax=True, transitions_out=tout, transitions=tr) == 2
    df = pd.read_csv(out)
    assert list(df.columns) == list(segment.COLUMNS) + list(segment.SYNTAX_COLUMNS)
    assert df["transition_score"].tolist() == [-0.5, -0.25] and df["context_free_category_ix"].tolist() == [1, 0]
    assert df["changed"].tolist() == [0, 1]
    assert list(pd.read_csv(tout).columns) == list(segment.TRANSITION_COLUMNS)
    # without the chain the table is what it was
    plain = segment.segment_rows("a.wav", [0, 5], [5, 4], [1, 2], [-1.5, -2.5], 1000, 8, 4, True, 100)
    out2 = os.path.join(str(tmp_path), "plain.csv")
    segment.write_segments(out2, plain)
    assert list(pd.read_csv(out2).columns) == list(segment.COLUMNS)
    assert pd.read_csv(out2).equals(df[list(segment.COLUMNS)])
