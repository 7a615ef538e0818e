"""Segmentation posteriors, checked on the CPU: the references of
``spanpost_cases.py`` (the forward-backward recursions against brute-force
enumeration of every cover, the four identities, the category log-sum); the new
entry points' surface (header, binding, host-side argument checks, custom ops,
methods); ``segment.py``'s new arguments."""
import itertools

import numpy as np
import pytest
import torch

import span_cases as SP
import spanpost_cases as SQ

NEG = SQ.NEG


def _small_cases():
    """(N, D, kind, table, gap variants, bonus, d_min) for every N <= 9, D <= 5."""
    for N, D, kind in itertools.product(range(0, 10), range(1, 6), SQ.KINDS):
        t = SP.table_inputs(N, D, kind)
        gap_inf = t["gap"].copy()
        if N:
            gap_inf[::3] = NEG
        for (gname, gap), bonus, d_min in itertools.product(
                (("none", None), ("drawn", t["gap"]), ("inf", gap_inf)), (0.0, -1.5), sorted({1, min(3, D)})):
            yield N, D, kind, t["score"], gname, gap, bonus, d_min


def test_longdouble_is_extended():
    assert SQ.LD_OK, "np.longdouble is no wider than float64 here: the references run in float64 (bars doubled)"


def test_posterior_reference_is_brute_force():
    worst = dict(log_z=0.0, post=0.0, span=0.0)
    unreachable = reachable = 0
    for N, D, kind, W, gname, gap, bonus, d_min in _small_cases():
        ref = SQ.posterior_reference(W, d_min, gap, bonus)
        bf = SQ.brute_force_posterior(W, d_min, gap, bonus)
        fast = SQ.posterior_reference_fast(W, d_min, gap, bonus)
        tag = (N, D, kind, gname, bonus, d_min)
        for k in ("lattice", "post", "span_post"):
            with np.errstate(invalid="ignore"):         # -inf - -inf where both are -inf: equal
                same = (ref[k] == fast[k]) | (np.abs(ref[k] - fast[k]) <= 1e-13 * (1 + np.abs(ref[k])))
            assert same.all(), (tag, k)
        assert ref["post"].shape == (3, N + 1) and ref["span_post"].shape == (N + 1, D)
        assert ref["lattice"][0, 0] == 0.0 and ref["lattice"][2, N] == 0.0
        assert ref["lattice"][1, 0] == NEG and ref["lattice"][3, N] == NEG
        assert ref["post"][0, N] == 0 and ref["post"][1, 0] == 0 and ref["post"][2, N] == 0
        if bf["log_z"] == NEG:
            unreachable += 1
            assert ref["log_z"] == NEG and not ref["post"].any() and not ref["span_post"].any(), tag
            continue
        reachable += 1
        worst["log_z"] = max(worst["log_z"], abs(ref["log_z"] - bf["log_z"]) / max(1.0, abs(bf["log_z"])))
        worst["post"] = max(worst["post"], np.abs(ref["post"] - bf["post"]).max())
        worst["span"] = max(worst["span"], np.abs(ref["span_post"] - bf["span_post"]).max())
        # beta[0] is the same evidence
        assert abs(ref["lattice"][2, 0] - ref["log_z"]) <= 1e-12 * max(1.0, abs(ref["log_z"])), tag
    print(f"{reachable} reachable and {unreachable} unreachable configurations; worst differences {worst}")
    assert unreachable > 0 and reachable > 1000
    assert worst["log_z"] <= 1e-14 and worst["post"] <= 1e-13 and worst["span"] <= 1e-13


def test_empty_recording_and_special_cases():
    for D in (1, 4):
        r = SQ.posterior_reference(np.full((1, D), NEG), 1, None, 0.0)
        assert r["log_z"] == 0.0 and not r["post"].any() and r["lattice"][:, 0].tolist() == [0.0, NEG, 0.0, NEG]
    # one frame, one span of score w, a gap of score g: P(segment) = e^w / (e^w + e^g)
    W = np.array([[NEG], [0.5]])
    r = SQ.posterior_reference(W, 1, np.array([-0.25], dtype=np.float32), 0.0)
    p = np.exp(0.5) / (np.exp(0.5) + np.exp(-0.25))
    assert abs(r["log_z"] - np.log(np.exp(0.5) + np.exp(-0.25))) <= 1e-15
    assert np.allclose(r["post"], [[p, 0], [0, p], [1 - p, 0]], atol=1e-15) and abs(r["span_post"][1, 0] - p) <= 1e-15
    # without a gap and with d_min = 2 a single frame cannot be covered
    r = SQ.posterior_reference(np.array([[NEG, NEG], [1.0, NEG]]), 2, None, 0.0)
    assert r["log_z"] == NEG and not r["post"].any()
    # a NaN entry is a hole, not a poison
    W = np.array([[NEG, NEG], [np.nan, NEG], [1.0, 2.0]])
    r = SQ.posterior_reference(W, 1, None, 0.0)
    assert r["log_z"] == 2.0 and r["span_post"][2, 1] == 1.0 and r["post"][0].tolist() == [1.0, 0.0, 0.0]


def test_the_four_identities_hold():
    worst = 0.0
    for N, D, kind, W, gname, gap, bonus, d_min in _small_cases():
        ref = SQ.posterior_reference(W, d_min, gap, bonus)
        if ref["log_z"] == NEG:
            continue
        v = SQ.identities(ref["post"], ref["span_post"], gap is not None)
        worst = max(worst, v["cover"], v["ends"], v["onsets"])
        # the expected number of segments: sum end_post = the total span mass
        assert abs(ref["post"][1].sum() - ref["span_post"].sum()) <= 1e-12
    print(f"worst identity violation {worst:.1e}")
    assert worst <= 1e-12


def test_lse_reference():
    c = SQ.evidence_case(33, 5, 17, 1)
    S, best = c["ref"]["S"], c["ref"]["score"]
    fin = np.isfinite(best)
    assert (c["lse"][~fin] == NEG).all() and (c["lse"][fin] >= best[fin]).all()
    assert (c["lse"][fin] <= best[fin] + np.log(17) + 1e-12).all()
    assert (c["lse"][fin] - best[fin]).max() > 0.1             # at F = 1 the sum and the maximum really differ
    e, d = 20, 3
    s = S[e - d, :, d - 1]
    assert abs(c["lse"][e, d - 1] - np.log(np.exp(s - s.max()).sum()) - s.max()) <= 1e-12
    one = SQ.evidence_case(33, 5, 1, 65)
    assert np.array_equal(one["lse"], one["ref"]["score"])     # one prototype: the sum is the maximum
    # exclusions follow span_reference's rule
    lw = c["lw"].clone()
    lw[2], lw[5] = float("-inf"), float("nan")
    r = SP.span_reference(c["x"], c["mu"], c["lv"], c["o"], lw, 5)
    lse = SQ.lse_reference(r["S"])
    keep = [p for p in range(17) if p not in (2, 5)]
    s = r["S"][e - d, keep, d - 1]
    assert abs(lse[e, d - 1] - np.log(np.exp(s - s.max()).sum()) - s.max()) <= 1e-12
    assert np.isnan(SQ.unit_reference(r["S"], r["A"])[0]).all()


# ----------------------------------------------------------------------------
# surface
# ----------------------------------------------------------------------------
SYMS = ("abcd_span_evidence_workspace_bytes", "abcd_span_evidence", "abcd_span_posterior_workspace_bytes",
        "abcd_span_posterior")


def test_new_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in SYMS:
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.library_hash() == N.source_hash()
    we, ws = N.lib().abcd_span_evidence_workspace_bytes, N.lib().abcd_span_scores_workspace_bytes
    assert we(15000, 200, 128) >= 200 * 128 * 8
    assert we(0, 1, 1) > 0 and we(-1, 1, 1) == 0 and we(4, 0, 1) == 0 and we(4, 1, 0) == 0
    assert we(4, 16383, 1) > 0 and we(4, 16384, 1) == 0
    assert we((1 << 31) // 8 - 2, 8, 1) > 0 and we((1 << 31) // 8 - 1, 8, 1) == 0 and we(1 << 40, 1, 1) == 0
    assert we(70, 17, 33) == ws(70, 17, 33)
    wp = N.lib().abcd_span_posterior_workspace_bytes
    assert wp(15000, 200) >= 4 * 15001 * 8
    assert wp(0, 1) > 0 and wp(-1, 1) == 0 and wp(4, 0) == 0 and wp(4, 16383) > 0 and wp(4, 16384) == 0
    assert wp((1 << 31) // 8 - 2, 8) > 0 and wp((1 << 31) // 8 - 1, 8) == 0 and wp(1 << 40, 1) == 0


def test_entry_points_reject_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, F, P, D = 9, 4, 5, 3
    nb = lib.abcd_span_evidence_workspace_bytes(n, D, P)

    def ev(x=fake, ldx=F, n=n, F=F, P=P, D=D, Tp=D, mu=fake, ldm=F, lv=fake, ldl=F, o=fake, lw=None, lse=fake,
           ss=fake, sc=fake, lds=D, ws=fake, nb=nb):
        return lib.abcd_span_evidence(x, ldx, n, F, P, D, Tp, mu, ldm, lv, ldl, o, lw, lse, ss, sc, lds, ws, nb, None)

    assert ev(D=0, Tp=4) == E and ev(D=16384, Tp=16384, lds=16384, nb=1 << 40) == E
    assert ev(P=0) == E and ev(F=0) == E and ev(n=-1) == E
    assert ev(n=(1 << 31) // 3, nb=1 << 40) == E
    assert ev(Tp=D - 1) == E
    assert ev(ldx=F - 1) == E and ev(ldm=F - 1) == E and ev(ldl=F - 1) == E and ev(lds=D - 1) == E
    for k in ("x", "mu", "lv", "o", "lse"):
        assert ev(**{k: None}) == E, k
    assert ev(ss=None) == E and ev(sc=None) == E               # the best outputs come together or not at all
    assert ev(ws=None) == E and ev(nb=nb - 1) == E and ev(nb=0) == E
    assert ev(ss=None, sc=None, ws=None) == E
    nb0 = lib.abcd_span_evidence_workspace_bytes(0, D, P)
    assert ev(n=0, x=None, mu=None, lv=None, o=None, lse=None, ss=None, sc=None, nb=nb0) == 0
    assert ev(n=0, lse=None, ss=None, sc=None, ws=None, nb=nb0) == E
    assert ev(n=0, lse=None, ss=None, nb=nb0) == E

    npb = lib.abcd_span_posterior_workspace_bytes(n, D)

    def post(sp=fake, lds=D, n=n, D=D, dmin=1, gap=None, bonus=0.0, lz=fake, lat=None, po=fake, tb=None, ldp=D,
             ws=fake, nb=npb):
        return lib.abcd_span_posterior(sp, lds, n, D, dmin, gap, bonus, lz, lat, po, tb, ldp, ws, nb, None)

    assert post(dmin=0) == E and post(dmin=D + 1) == E
    assert post(D=0) == E and post(D=16384, lds=16384, ldp=16384, nb=1 << 40) == E and post(n=-1) == E
    assert post(n=(1 << 31) // 3, nb=1 << 40) == E
    assert post(lds=D - 1) == E
    assert post(tb=fake, ldp=D - 1) == E and post(tb=fake, lat=fake, ldp=0) == E
    for k in ("sp", "lz", "po"):
        assert post(**{k: None}) == E, k
    assert post(ws=None) == E and post(nb=npb - 1) == E and post(nb=0) == E
    np0 = lib.abcd_span_posterior_workspace_bytes(0, D)
    assert post(n=0, sp=None, lz=None, po=None, nb=np0) == 0     # valid, with nowhere to write: no device
    assert post(n=0, sp=None, lz=None, po=None, dmin=0, nb=np0) == E
    assert post(n=0, sp=None, lz=None, po=None, ws=None, nb=np0) == E


def test_ops_and_methods_exist():
    from modules import model as M, ops, segmentation
    for name in ("span_evidence", "span_posterior"):
        assert name in ops.OPS and hasattr(torch.ops.abcd, name)
        assert f"``abcd::{name}``" in ops.__doc__
    assert set(ops.registered()) == set(ops.OPS)
    schema = str(torch.ops.abcd.span_evidence.default._schema)
    assert schema.startswith("abcd::span_evidence(Tensor frames, Tensor proto_mu, Tensor proto_lv, Tensor "
                             "proto_offset_logits, Tensor? log_weight, SymInt P, SymInt D, bool want_best) -> "
                             "Tensor[]"), schema
    schema = str(torch.ops.abcd.span_posterior.default._schema)
    assert schema.startswith("abcd::span_posterior(Tensor span, SymInt d_min, Tensor? gap, float seg_bonus, "
                             "bool want_table) -> Tensor[]"), schema
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a = (torch.empty(9, 4), torch.empty(15, 4), torch.empty(15, 4), torch.empty(15), None, 5, 3)
        lse, ss, sc = torch.ops.abcd.span_evidence(*a, True)
        assert lse.shape == ss.shape == sc.shape == (10, 3)
        assert lse.dtype == ss.dtype == torch.float64 and sc.dtype == torch.int32
        lse, ss, sc = torch.ops.abcd.span_evidence(*a, False)
        assert lse.shape == (10, 3) and ss.shape == sc.shape == (0, 0) and sc.dtype == torch.int32
        for want in (True, False):
            lz, lat, po, tb = torch.ops.abcd.span_posterior(lse, 2, None, 0.0, want)
            assert [tuple(t.shape) for t in (lz, lat, po, tb)] == [(), (4, 10), (3, 10), (10, 3) if want else (0, 0)]
            assert {t.dtype for t in (lz, lat, po, tb)} == {torch.float64}
    assert callable(M.RNN_Variational_Decoder.span_evidence) and callable(segmentation.segment_posteriors)
    # no CPU fallback anywhere
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    protos = (torch.zeros(3, 4, 33), torch.zeros(3, 4, 33), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        dec.span_evidence(protos, torch.zeros(9, 33), 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        segmentation.segment_posteriors(dec, protos, torch.zeros(9, 33), 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        segmentation.segment_frames(dec, protos, torch.zeros(9, 33), 3, posteriors=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.span_evidence(torch.zeros(9, 4), torch.zeros(15, 4), torch.zeros(15, 4), torch.zeros(15), None, 5, 3, True)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.span_posterior(torch.zeros(10, 3, dtype=torch.float64), 1, None, 0.0, False)


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def test_segment_cli_posterior_arguments():
    import segment
    base = ["c", "r", "t", "1", "--max_length", "9"]
    a = segment.get_parameters(base)
    assert (a.posteriors, a.posterior_temperature, a.curves_dir, a.recordings_out) == (False, 1.0, None, None)
    a = segment.get_parameters(base + ["--posteriors"])
    assert (a.posteriors, a.posterior_temperature, a.curves_dir, a.recordings_out) == (True, 1.0, None, None)
    a = segment.get_parameters(base + ["--posteriors", "--posterior_temperature", "40", "--curves_dir", "cd",
                                       "--recordings_out", "rec.csv"])
    assert (a.posteriors, a.posterior_temperature, a.curves_dir, a.recordings_out) == (True, 40.0, "cd", "rec.csv")
    for bad in (["--posterior_temperature", "2"], ["--curves_dir", "cd"], ["--recordings_out", "rec.csv"],
                ["--posteriors", "--posterior_temperature", "0"], ["--posteriors", "--posterior_temperature", "-1"],
                ["--posteriors", "--posterior_temperature", "nan"]):
        with pytest.raises(SystemExit):
            segment.get_parameters(base + bad)
    assert segment.COLUMNS[-1] == "segment_score"
    assert segment.POSTERIOR_COLUMNS == ("onset_posterior", "offset_posterior", "span_posterior")
    assert segment.RECORDING_COLUMNS == ("input_path", "n_frames", "n_segments", "path_score", "log_evidence",
                                         "expected_segments")


def test_segment_cli_old_arguments_parse_as_before():
    """The argument lists of test_span_cpu.py::test_segment_cli_arguments, to the same values."""
    import segment
    a = segment.get_parameters(["ckpt.pt", "root", "rec.csv", "1.0", "--max_length", "200"])
    assert (a.model_path, a.input_root, a.recording_table, a.data_normalizer) == ("ckpt.pt", "root", "rec.csv", 1.0)
    assert (a.max_length, a.min_length, a.prior, a.entire_data_size, a.segment_bonus) == \
        (200, 1, "dirichlet", None, 0.0)
    assert a.gap_score is None and a.gap_model is None and a.fit_gap is None and a.speaker is None
    assert a.device == "cuda" and a.save_path is None and a.epsilon == 2 ** -15
    a = segment.get_parameters(["c", "r", "t", "2.5", "--max_length", "50", "--min_length", "4", "--prior", "uniform",
                                "--entire_data_size", "900", "--segment_bonus", "-3.5", "--gap_score", "-120",
                                "--speaker", "2", "-S", "out.csv", "-d", "cuda:1"])
    assert (a.max_length, a.min_length, a.prior, a.entire_data_size, a.segment_bonus, a.gap_score, a.speaker) == \
        (50, 4, "uniform", 900.0, -3.5, -120.0, 2)
    assert not a.posteriors
    a = segment.get_parameters(["c", "r", "t", "1", "--max_length", "9", "--fit_gap", "ann.csv", "--gap_model_out",
                                "g.npz"])
    assert (a.fit_gap, a.gap_model_out) == ("ann.csv", "g.npz") and not a.posteriors


def test_segment_rows_and_writer_carry_the_posterior_columns(tmp_path):
    import os
    import pandas as pd
    import segment
    rows = segment.segment_rows("a.wav", [0, 5], [5, 3], [1, 2], [-1.0, -2.0], 8000, 64, 32, True, 400)
    both = segment.segment_rows("a.wav", [0, 5], [5, 3], [1, 2], [-1.0, -2.0], 8000, 64, 32, True, 400,
                                posteriors=[[0.9, 0.8], [0.7, 0.6], [0.5, 0.4]])
    assert [{k: r[k] for k in segment.COLUMNS} for r in both] == rows
    assert [r["span_posterior"] for r in both] == [0.5, 0.4] and both[1]["onset_posterior"] == 0.8
    plain, post = (os.path.join(str(tmp_path), n) for n in ("plain.csv", "post.csv"))
    rec, cur = os.path.join(str(tmp_path), "rec.csv"), segment.curve_path(str(tmp_path), "d/a.wav")
    assert os.path.basename(cur) == "d__a.npz"
    segment.write_segments(plain, rows)
    segment.write_segments(post, both, posteriors=True, recordings_out=rec,
                           recordings=[dict(input_path="a.wav", n_frames=13, n_segments=2, path_score=-3.0,
                                            log_evidence=-2.5, expected_segments=2.1)],
                           curves={cur: dict(onset=np.zeros(14), end=np.zeros(14), gap=np.zeros(14),
                                             log_evidence=-2.5, fs=8000, hop=32)})
    a, b = pd.read_csv(plain), pd.read_csv(post)
    assert list(a.columns) == list(segment.COLUMNS)
    assert list(b.columns) == list(segment.COLUMNS) + list(segment.POSTERIOR_COLUMNS)
    assert a.equals(b[list(segment.COLUMNS)])
    assert list(pd.read_csv(rec).columns) == list(segment.RECORDING_COLUMNS)
    with np.load(cur) as z:
        assert z["onset"].shape == (14,) and float(z["log_evidence"]) == -2.5 and int(z["hop"]) == 32
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".partial")]


@pytest.mark.parametrize("with_gap", (False, True), ids=("nogap", "gap"))
def test_tail_cases_keep_mass_on_both_kinds_of_candidate(with_gap):
    """The conditions of span_cases.TAIL_CASES on the reference alone: the forced
    case can be covered, all of its mass on loop candidates; the mixed case's
    span posterior has at least 1e-3 on either side of the registers' reach."""
    cut = SP.TAIL_FROM - 1
    forced = SQ.tail_posterior("forced", with_gap)
    assert forced["log_z"] > NEG and forced["span_post"][:, cut:].sum() >= 1e-3 and not forced["span_post"][:, :cut].any()
    mixed = SQ.tail_posterior("mixed", with_gap)["span_post"]
    print(f"mixed: mass {mixed[:, cut:].sum():.3g} on d >= {SP.TAIL_FROM}, {mixed[:, :cut].sum():.3g} below")
    assert mixed[:, cut:].sum() >= 1e-3 and mixed[:, :cut].sum() >= 1e-3
