"""Segmentation posteriors under the chain, checked on the CPU: the
longdouble reference of ``chainpost_cases.py`` (brute-force enumeration of
every labelled cover on tiny tables, the identities, the reduction to the
context-free posteriors, the planted alternation, EM), the new entry points'
surface (header, binding, workspace limits, host-side argument checks, the
operator's schema and fake outputs) and ``segment.py``'s new arguments,
columns and writer."""
import numpy as np
import pytest
import torch

import chainpost_cases as CP
import spanpost_cases as PC
import syntax_cases as SX

NEG = CP.NEG
TOL = 1e-15 if CP.LD_OK else 1e-12      # float64 outputs of a longdouble computation


def _drawn(g, trial):
    """One tiny configuration: N <= 7, D <= 5, K <= 3."""
    N, D, K = int(g.integers(1, 8)), int(g.integers(1, 6)), int(g.integers(1, 4))
    kind = trial % 5
    if kind == 1:                       # integer ties
        T = SX.mask_impossible(g.integers(-3, 2, size=(N + 1, D, K)).astype(np.float64))
        lt = g.integers(-2, 1, size=(K, K)).astype(np.float32)
        li = g.integers(-2, 1, size=K).astype(np.float32)
    else:
        T = SX.random_table(g, N, D, K)
        lt = np.stack([SX.log_softmax(g.normal(0.0, 2.0, size=K)) for _ in range(K)]).astype(np.float32)
        li = SX.log_softmax(g.normal(0.0, 1.0, size=K)).astype(np.float32)
    if kind == 2:                       # holes
        T[g.random(T.shape) < 0.2] = np.nan
        T[g.random(T.shape) < 0.2] = NEG
    if kind == 3:                       # structural zeros
        lt[g.random(lt.shape) < 0.4] = NEG
        li[K - 1] = NEG
    if kind == 4:                       # an all-zero chain: one segment at most
        lt[:] = NEG
    d_min = (1, min(2, D), D)[trial % 3]
    gap = g.normal(-1.0, 1.0, size=N).astype(np.float32) if (trial // 5) % 2 else None
    bonus = (0.0, -1.25)[(trial // 10) % 2]
    return T, d_min, lt, li, gap, bonus


def test_reference_is_brute_force_and_the_identities_hold():
    g = np.random.default_rng(314159)
    worst, worst_id, unreachable = 0.0, 0.0, 0
    for trial in range(120):
        T, d_min, lt, li, gap, bonus = _drawn(g, trial)
        scale = 0.25 if trial % 7 == 0 else 1.0
        ref = CP.chain_posterior_reference(T, d_min, lt, li, gap, bonus, scale)
        bf = CP.brute_force(T, d_min, lt, li, gap, bonus, scale)
        if bf["log_z"] == NEG:
            unreachable += 1
            assert ref["log_z"] == NEG
        else:
            assert abs(ref["log_z"] - bf["log_z"]) <= TOL * (1.0 + abs(bf["log_z"])), trial
            assert abs(ref["lattice_g"][1][0] - ref["log_z"]) <= TOL * (1.0 + abs(bf["log_z"])), trial   # bG[0]
        for key in ("post_k", "gap_post", "trans_counts", "init_counts", "span_post"):
            err = float(np.abs(ref[key] - bf[key]).max())
            worst = max(worst, err)
            assert err <= 16 * TOL, (trial, key, err)
        assert abs(ref["no_segment"] - bf["no_segment"]) <= 16 * TOL
        ids = CP.identities(ref)
        worst_id = max([worst_id] + list(ids.values()))
        assert max(ids.values()) <= 16 * TOL, (trial, ids)
    print(f"reference against brute force: worst difference {worst:.1e}, worst identity violation {worst_id:.1e}, "
          f"{unreachable} configurations without a cover")
    assert unreachable > 0


def test_empty_recording():
    ref = CP.chain_posterior_reference(np.full((1, 3, 2), NEG), 1, np.zeros((2, 2)), np.zeros(2))
    assert ref["log_z"] == 0.0 and (ref["post_k"] == 0).all() and (ref["trans_counts"] == 0).all()
    assert (ref["lattice"][:4] == NEG).all() and (ref["lattice"][4] == 0).all() and (ref["lattice_g"] == 0).all()


def test_reference_reduces_to_the_context_free_posteriors():
    """(vi): every row of log_trans and log_init equal to one log_softmax(lw):
    log_z, the category-summed curves and span_post are those of
    spanpost_cases.posterior_reference on LSE_k (T + lw)."""
    g = np.random.default_rng(2718)
    worst = 0.0
    for trial in range(40):
        N, D, K = int(g.integers(1, 13)), int(g.integers(1, 6)), int(g.integers(1, 5))
        T = SX.random_table(g, N, D, K)
        if trial % 4 == 3:
            T[g.random(T.shape) < 0.15] = NEG
        p = SX.log_softmax(g.normal(0.0, 1.0, size=K)).astype(np.float32)
        gap = g.normal(-1.0, 1.0, size=N).astype(np.float32) if trial % 2 else None
        d_min, bonus = int(g.integers(1, D + 1)), (0.0, 0.75)[trial % 3 == 0]
        ref = CP.chain_posterior_reference(T, d_min, np.tile(p[None, :], (K, 1)), p, gap, bonus)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = T.astype(CP.RT) + p.astype(CP.RT)[None, None, :]
            span = np.asarray(CP._lse(v, 2), dtype=np.float64)
        want = PC.posterior_reference(span, d_min, gap, bonus)
        if want["log_z"] == NEG:
            assert ref["log_z"] == NEG
            continue
        assert abs(ref["log_z"] - want["log_z"]) <= 1e-13 * (1.0 + abs(want["log_z"]))
        got = np.stack([ref["post_k"][0].sum(1), ref["post_k"][1].sum(1), ref["gap_post"]])
        err = max(float(np.abs(got - want["post"]).max()), float(np.abs(ref["span_post"] - want["span_post"]).max()))
        worst = max(worst, err)
        assert err <= 1e-12, (trial, err)
    print(f"reduction to the context-free posteriors: worst difference {worst:.1e}")


def test_planted_alternation():
    c = SX.planted_alternation()
    ref = CP.chain_posterior_reference(c["table"], 1, c["trans"], c["init"])
    assert abs(ref["post_k"][1].sum() - SX.ALT_SEGMENTS) <= 1e-9                    # 7 expected segments
    stay = 6.0 * SX.ALT_STAY                                                        # six links, almost surely alternating
    want = np.array([[stay / 2, 3.0 - stay / 2], [3.0 - stay / 2, stay / 2]])
    assert np.abs(ref["trans_counts"] - want).max() <= 1e-3, ref["trans_counts"]
    assert np.abs(ref["trans_counts"] - np.array([[0.003, 2.997], [2.997, 0.003]])).max() <= 1e-3
    assert np.abs(ref["init_counts"] - 0.5).max() <= 1e-12
    # every frame lies in a segment; the two labellings are equally likely
    inside = np.cumsum(ref["post_k"][0] - ref["post_k"][1], 0)[:c["N"]]
    assert np.abs(inside.sum(1) - 1.0).max() <= 1e-9 and np.abs(inside - 0.5).max() <= 1e-9


@pytest.mark.parametrize("temperature", (1.0, 4.0))
def test_reference_em_climbs(temperature):
    N, D, K, d_min = 14, 3, 3, 1
    recs = CP.em_recordings(N, D, K, 3)
    c = 1.0 / K
    out = CP.em_reference(recs, K, d_min, 6, c, temperature)
    slack = CP.em_slack(out["L"], recs, d_min, c, K)
    objs = out["objectives"]
    drops = [a - b for a, b in zip(objs[:-1], objs[1:])]
    print(f"temperature {temperature}: objectives {['%.6f' % v for v in objs]}; largest drop {max(drops):.2e} "
          f"against the slack {slack:.2e}")
    assert max(drops) <= slack
    assert objs[-1] > objs[0]
    assert np.allclose(np.exp(out["trans"].astype(np.float64)).sum(1), 1.0, atol=1e-6)


# ----------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------
SYMS = ("abcd_span_chain_posterior_plan", "abcd_span_chain_posterior_workspace_bytes", "abcd_span_chain_posterior")


def test_new_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in SYMS:
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.library_hash() == N.source_hash()
    wc = N.lib().abcd_span_chain_posterior_workspace_bytes
    assert wc(15000, 200, 128) >= 15001 * (5 * 128 + 2) * 8
    assert wc(0, 1, 1) > 0 and wc(-1, 1, 1) == 0 and wc(4, 0, 1) == 0 and wc(4, 1, 0) == 0
    assert wc(4, 1, 1024) > 0 and wc(4, 1, 1025) == 0 and wc(4, 16383, 1) > 0 and wc(4, 16384, 1) == 0
    assert wc((1 << 31) // 64 - 2, 8, 8) > 0 and wc((1 << 31) // 64 - 1, 8, 8) == 0 and wc(1 << 40, 1, 1) == 0


def test_posterior_plan_is_a_pure_function_and_leaves_the_viterbi_plan_alone():
    from modules import _native as N
    lib = N.lib()
    res, thr, lds = N.c_int(-1), N.c_int(-1), N.ctypes.c_size_t(0)
    res0, thr0 = N.c_int(-1), N.c_int(-1)
    for K, want in ((1, 1), (2, 1), (33, 1), (128, 1), (129, 0), (130, 0), (256, 0), (257, 0), (1024, 0)):
        assert lib.abcd_span_chain_posterior_plan(K, 200, N.ctypes.byref(res), N.ctypes.byref(thr),
                                                  N.ctypes.byref(lds)) == 0
        assert lib.abcd_span_chain_plan(K, 200, N.ctypes.byref(res0), N.ctypes.byref(thr0), None) == 0
        waves = 16 if K <= 256 else 4
        assert res.value == want == res0.value and thr.value == 64 * waves == thr0.value, K
        # four vectors of K doubles, a (maximum, sum) pair per wave and k; the matrix at a row stride of K + 1 floats
        assert lds.value == K * (4 + 2 * waves) * 8 + (K * (K + 1) * 4 if want else 0) and lds.value <= 160 * 1024
    E = N.ABCD_EINVAL
    for K, D in ((0, 5), (1025, 5), (4, 0), (4, 16384)):
        assert lib.abcd_span_chain_posterior_plan(K, D, None, None, None) == E


def test_entry_point_rejects_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, D, K = 9, 3, 5
    nv = lib.abcd_span_chain_posterior_workspace_bytes(n, D, K)

    def fb(tb=fake, ldk=K, n=n, D=D, K=K, dmin=1, gap=None, bonus=0.0, scale=1.0, lt=fake, ldt=K, li=fake, lz=fake,
           lat=None, latg=None, pk=fake, gp=fake, tc=None, ic=None, sp=None, ldp=D, ws=fake, nb=nv):
        return lib.abcd_span_chain_posterior(tb, ldk, n, D, K, dmin, gap, bonus, scale, lt, ldt, li, lz, lat, latg, pk,
                                             gp, tc, ic, sp, ldp, ws, nb, None)

    assert fb(K=0, ldk=1, ldt=1) == E and fb(K=1025, ldk=1025, ldt=1025, nb=1 << 40) == E
    assert fb(dmin=0) == E and fb(dmin=D + 1) == E
    assert fb(D=0) == E and fb(D=16384, nb=1 << 40) == E and fb(n=-1) == E
    assert fb(n=(1 << 31) // 3, nb=1 << 40) == E and fb(n=(1 << 31) // 15, nb=1 << 40) == E
    assert fb(n=(1 << 31) // 30, ldk=2 * K, nb=1 << 40) == E
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert fb(scale=bad) == E, bad
    assert fb(ldk=K - 1) == E and fb(ldt=K - 1) == E
    assert fb(sp=fake, ldp=D - 1) == E
    assert fb(tc=fake) == E and fb(ic=fake) == E                        # both or neither
    for k in ("tb", "lt", "li", "lz", "pk", "gp"):
        assert fb(**{k: None}) == E, k
    assert fb(ws=None) == E and fb(nb=nv - 1) == E and fb(nb=0) == E
    # N = 0 is valid; with nowhere to write it needs no device
    nv0 = lib.abcd_span_chain_posterior_workspace_bytes(0, D, K)
    assert fb(n=0, tb=None, lt=None, li=None, lz=None, pk=None, gp=None, nb=nv0) == 0
    assert fb(n=0, dmin=0, lz=None, pk=None, gp=None, nb=nv0) == E
    assert fb(n=0, scale=0.0, lz=None, pk=None, gp=None, nb=nv0) == E


def test_operator_and_functions_exist():
    from modules import model as M, ops, segmentation
    from modules.sequence import TransitionModel
    assert "span_chain_posterior" in ops.OPS and hasattr(torch.ops.abcd, "span_chain_posterior")
    assert set(ops.registered()) == set(ops.OPS)
    schema = str(torch.ops.abcd.span_chain_posterior.default._schema)
    assert schema.startswith("abcd::span_chain_posterior(Tensor table, SymInt d_min, Tensor? gap, float seg_bonus, "
                             "float scale, Tensor log_trans, Tensor log_init, bool want_counts, bool want_table) -> "
                             "Tensor[]"), schema
    # the Viterbi operator's schema is what it was
    schema = str(torch.ops.abcd.span_chain_viterbi.default._schema)
    assert schema.startswith("abcd::span_chain_viterbi(Tensor table, SymInt d_min, Tensor? gap, float seg_bonus, "
                             "Tensor log_trans, Tensor log_init, bool want_w) -> Tensor[]"), schema
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        tb = torch.empty(10, 3, 5, dtype=torch.float64)
        a = (tb, 2, None, 0.0, 1.0, torch.empty(5, 5), torch.empty(5))
        out = torch.ops.abcd.span_chain_posterior(*a, True, True)
        assert [tuple(t.shape) for t in out] == [(), (5, 10, 5), (2, 10), (2, 10, 5), (10,), (5, 5), (5,), (10, 3)]
        assert all(t.dtype == torch.float64 for t in out)
        out = torch.ops.abcd.span_chain_posterior(*a, False, False)
        assert [tuple(t.shape) for t in out[5:]] == [(0, 0), (0,), (0, 0)]
    assert callable(segmentation.segment_chain_posteriors) and callable(segmentation.refit_transitions_em)
    # no CPU fallback
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    protos = (torch.zeros(3, 4, 33), torch.zeros(3, 4, 33), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        segmentation.segment_chain_posteriors(dec, protos, torch.zeros(9, 33), 3, TransitionModel(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.span_chain_posterior(torch.zeros(10, 3, 5, dtype=torch.float64), 1, None, 0.0, 1.0, torch.zeros(5, 5),
                                 torch.zeros(5), False, False)


def test_refit_transitions_em_sums_counts_and_normalises():
    """EM with a posterior function that ignores the model: the rows become
    (expected counts + c) normalised, the objective is temperature * evidence +
    c * the finite log-probabilities of the model the iteration started from."""
    from modules import segmentation
    from modules.sequence import TransitionModel
    counts = {"a": ([[0.25, 1.5], [1.25, 0.0]], [0.75, 0.25]), "b": ([[0.0, 0.5], [0.5, 0.0]], [0.5, 0.5])}
    calls = []

    def posterior_fn(rec, model):
        calls.append(rec)
        tc, ic = counts[rec]
        return dict(log_evidence=torch.tensor(-2.0, dtype=torch.float64),
                    trans_counts=torch.tensor(tc, dtype=torch.float64), init_counts=torch.tensor(ic, dtype=torch.float64))

    m = TransitionModel(2)
    before = float(m.log_trans.double().sum() + m.log_init.double().sum())
    totals = segmentation.refit_transitions_em(posterior_fn, ["a", "b"], m, 2, 0.5, temperature=4.0)
    assert calls == ["a", "b", "a", "b"] and len(totals) == 2
    assert abs(totals[0] - (4.0 * -4.0 + 0.5 * before)) <= 1e-12
    want_t = torch.tensor([[0.75, 2.5], [2.25, 0.5]], dtype=torch.float64)
    want_t = want_t / want_t.sum(1, keepdim=True)
    want_i = torch.tensor([1.75, 1.25], dtype=torch.float64) / 3.0
    assert torch.allclose(m.log_trans.double().exp(), want_t, rtol=1e-6)
    assert torch.allclose(m.log_init.double().exp(), want_i, rtol=1e-6)
    after = float(m.log_trans.double().sum() + m.log_init.double().sum())
    assert abs(totals[1] - (4.0 * -4.0 + 0.5 * after)) <= 1e-12
    assert m.last_counts[0].tolist() == [[0.25, 2.0], [1.75, 0.0]] and m.last_counts[1].tolist() == [1.25, 0.75]
    # Viterbi training is what it was
    paths = {"a": [0, 1, 0, 1], "b": [1, 0]}
    m2 = TransitionModel(2)
    tot = segmentation.refit_transitions(
        lambda rec, model: dict(category=torch.tensor(paths[rec]), path_score=torch.tensor(-2.0, dtype=torch.float64)),
        ["a", "b"], m2, 1, 0.5)
    assert tot == [-4.0] and m2.last_counts[0].tolist() == [[0.0, 2.0], [2.0, 0.0]]


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def test_segment_cli_arguments():
    import segment
    base = ["c", "r", "t", "1", "--max_length", "9"]
    a = segment.get_parameters(base)
    assert a.chain_posteriors is False and a.refit_method == "viterbi"
    a = segment.get_parameters(base + ["--transitions", "t.csv", "--chain_posteriors"])
    assert a.chain_posteriors and a.transitions == "t.csv" and not a.posteriors
    a = segment.get_parameters(base + ["--transitions", "t.csv", "--chain_posteriors", "--posterior_temperature", "4",
                                       "--curves_dir", "c", "--recordings_out", "r.csv"])
    assert (a.posterior_temperature, a.curves_dir, a.recordings_out) == (4.0, "c", "r.csv")
    a = segment.get_parameters(base + ["--refit_transitions", "2", "--transitions_out", "n.csv", "--refit_method", "em",
                                       "--chain_posteriors"])
    assert (a.refit_transitions, a.refit_method, a.chain_posteriors) == (2, "em", True)
    a = segment.get_parameters(base + ["--refit_transitions", "2", "--transitions_out", "n.csv", "--refit_method",
                                       "viterbi"])
    assert a.refit_method == "viterbi"
    for bad in (["--chain_posteriors"],                                             # no chain
                ["--refit_method", "em"],                                           # nothing to refit
                ["--transitions", "t.csv", "--refit_method", "em"],
                ["--refit_transitions", "1", "--transitions_out", "n.csv", "--refit_method", "other"],
                # the pinned refusals stay
                ["--transitions", "t.csv", "--posteriors"],
                ["--transitions", "t.csv", "--posteriors", "--chain_posteriors"],
                ["--refit_transitions", "1", "--transitions_out", "n.csv", "--posteriors"],
                ["--refit_transitions", "1", "--transitions_out", "n.csv", "--posteriors", "--refit_method", "em"],
                ["--transitions", "t.csv", "--posterior_temperature", "2"],         # needs a posterior flag
                ["--transitions", "t.csv", "--chain_posteriors", "--posterior_temperature", "0"]):
        with pytest.raises(SystemExit):
            segment.get_parameters(base + bad)
    assert segment.CHAIN_POSTERIOR_COLUMNS == ("onset_posterior", "offset_posterior", "span_posterior",
                                               "label_posterior")
    assert segment.POSTERIOR_COLUMNS == ("onset_posterior", "offset_posterior", "span_posterior")


def test_segment_rows_and_writer_with_chain_posterior_columns(tmp_path):
    import os

    import pandas as pd

    import segment
    args = ("a.wav", [0, 5], [5, 4], [1, 2], [-1.5, -2.5], 1000, 8, 4, True, 100)
    rows = segment.segment_rows(*args, syntax=([-0.5, -0.25], [1, 0]),
                                chain_posteriors=[[0.9, 0.8], [0.7, 0.6], [0.5, 0.4], [0.3, 0.2]])
    out = os.path.join(str(tmp_path), "segmented.csv")
    assert segment.write_segments(out, rows, syntax=True, chain_posteriors=True) == 2
    df = pd.read_csv(out)
    assert list(df.columns) == list(segment.COLUMNS) + list(segment.SYNTAX_COLUMNS) + list(
        segment.CHAIN_POSTERIOR_COLUMNS)
    assert df["onset_posterior"].tolist() == [0.9, 0.8] and df["offset_posterior"].tolist() == [0.7, 0.6]
    assert df["span_posterior"].tolist() == [0.5, 0.4] and df["label_posterior"].tolist() == [0.3, 0.2]
    # without the flag the table is what it was
    plain = segment.segment_rows(*args, syntax=([-0.5, -0.25], [1, 0]))
    out2 = os.path.join(str(tmp_path), "plain.csv")
    segment.write_segments(out2, plain, syntax=True)
    assert list(pd.read_csv(out2).columns) == list(segment.COLUMNS) + list(segment.SYNTAX_COLUMNS)
    assert pd.read_csv(out2).equals(df[list(segment.COLUMNS) + list(segment.SYNTAX_COLUMNS)])
