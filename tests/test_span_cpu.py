"""Segmentation, checked on the CPU: the float64 references of
``span_cases.py`` (the dynamic programme against brute-force enumeration, the
span scores against ``pairwise_cases`` on the cut-out span, the planted
recording and its margins); the new entry points' surface (header, binding,
host-side argument checks, custom ops, methods); ``segment.py``'s arguments and
its frames-to-seconds mapping through the package's own loader."""
import itertools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import pairwise_cases as PW
import span_cases as SP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "toy_data")
ANN = os.path.join(TOY, "annotation_20170806-080002_89.2-94.22.csv")
NEG = SP.NEG


def _draw_table(g, N, D, kind):
    if kind == "tied":
        ss = g.integers(-2, 2, size=(N + 1, D)).astype(np.float64)
        gap = g.integers(-2, 1, size=N).astype(np.float32)
    else:
        ss = g.normal(0, 2, size=(N + 1, D))
        gap = g.normal(-1, 1, size=N).astype(np.float32)
    if kind == "holes":
        ss[g.random(ss.shape) < 0.2] = np.nan
        ss[g.random(ss.shape) < 0.2] = NEG
    cat = g.integers(0, 4, size=(N + 1, D))
    return ss, cat, gap


@pytest.mark.parametrize("kind", ["random", "tied", "holes"])
def test_viterbi_reference_is_brute_force(kind):
    g = np.random.default_rng(11)
    seen_unreachable = seen_gap_tie = 0
    for N, D in ((0, 3), (1, 1), (2, 3), (5, 2), (6, 4), (8, 3), (8, 8), (7, 5)):
        for d_min, use_gap, bonus in itertools.product((1, 2, D), (False, True), (0.0, -1.0)):
            if d_min > D:
                continue
            ss, cat, gap = _draw_table(g, N, D, kind)
            gp = gap if use_gap else None
            ref = SP.viterbi_reference(ss, cat, d_min, gp, bonus)
            best, moves = SP.brute_force(ss, d_min, gp, bonus)
            assert len(ref["V"]) == N + 1 and ref["V"][0] == 0.0
            if moves is None:                       # no cover (N < d_min without a gap, or holes everywhere)
                assert ref["path_score"] == NEG and ref["onset"] == []
                seen_unreachable += 1
                continue
            if kind == "tied":                      # small integers: every sum is exact
                assert ref["path_score"] == best
                assert SP.moves_of(ref, N) == moves, (N, D, d_min, use_gap)
                seen_gap_tie += 0 in moves
            else:
                assert abs(ref["path_score"] - best) <= 1e-9 * max(abs(best), 1.0)
                if kind == "random":                # no ties: the cover itself is decided
                    assert SP.moves_of(ref, N) == moves
            # the reported segments are ordered, disjoint, within the length bounds, and carry their table entries
            at = 0
            for s, d, c, v in zip(ref["onset"], ref["length"], ref["cat"], ref["score"]):
                assert s >= at and d_min <= d <= D and s + d <= N
                assert c == cat[s + d, d - 1] and v == ss[s + d, d - 1]
                at = s + d
            if not use_gap:
                assert sum(ref["length"]) == N
    assert seen_unreachable > 0
    if kind == "tied":
        assert seen_gap_tie > 0


def test_viterbi_reference_special_cases():
    ss = np.array([[NEG, NEG], [1.0, NEG], [1.0, 2.0], [np.nan, 2.0]])
    cat = np.zeros((4, 2), dtype=np.int64)
    r = SP.viterbi_reference(ss, cat, 1)            # 1 + 1 = 2 ties with the two-frame span: the smaller d wins
    assert r["V"].tolist() == [0.0, 1.0, 2.0, 3.0] and r["length"] == [1, 2] and r["onset"] == [0, 1]
    r = SP.viterbi_reference(ss, cat, 1, gap=np.array([1.0, 1.0, 1.0], dtype=np.float32))
    assert r["length"] == [] and r["path_score"] == 3.0          # the gap wins every tie
    r = SP.viterbi_reference(ss, cat, 2)            # frame 0 cannot be covered: N = 3 needs a span of 1
    assert r["path_score"] == NEG and r["V"].tolist() == [0.0, NEG, 2.0, NEG]
    r = SP.viterbi_reference(ss[:1], cat[:1], 1)
    assert r["path_score"] == 0.0 and r["onset"] == []
    r = SP.viterbi_reference(ss, cat, 1, seg_bonus=-0.75)
    assert r["V"].tolist() == [0.0, 0.25, 1.25, 1.5] and r["length"] == [1, 2]


def test_span_reference_is_pairwise_reference_on_the_cut():
    for N, D, F in ((7, 5, 3), (33, 17, 65), (12, 12, 129)):
        c = SP.abi_inputs(N, D, 1, F)
        ref = c["ref"]
        for s in range(N):
            for d in range(1, min(D, N - s) + 1):
                y = np.zeros(d)
                y[-1] = 1.0
                one = PW.pairwise_reference([1] * d, c["x"][s:s + d], c["mu"], c["lv"], c["o"], y)
                S = float(c["lw"][0]) - one["em"][0, 0] - one["off"][0, 0]
                A = one["A"][0, 0] + one["off"][0, 0]
                assert abs(ref["S"][s, 0, d - 1] - S) <= 1e-12 * A
                assert abs(ref["A"][s, 0, d - 1] - A) <= 1e-12 * A
                assert ref["score"][s + d, d - 1] == ref["S"][s, 0, d - 1] and ref["cat"][s + d, d - 1] == 0
        assert (ref["score"][0] == NEG).all() and (ref["cat"][0] == -1).all()
        for e in range(N + 1):
            assert (ref["score"][e, e:] == NEG).all() and (ref["cat"][e, e:] == -1).all()
    assert (33, 37) in SP.abi_shapes() and all(d <= n or (n, d) == (33, 37) for n, d in SP.abi_shapes())


def test_span_reference_exclusions():
    c = SP.abi_inputs(7, 5, 17, 3)
    x = c["x"].clone()
    x[3, 1] = float("nan")
    lw = c["lw"].clone()
    lw[2], lw[5] = float("-inf"), float("nan")
    r = SP.span_reference(x, c["mu"], c["lv"], c["o"], lw, 5)
    for e in range(1, 8):
        for d in range(1, min(5, e) + 1):
            poisoned = e - d <= 3 < e
            assert (r["score"][e, d - 1] == NEG and r["cat"][e, d - 1] == -1) == poisoned
            assert r["cat"][e, d - 1] not in (2, 5)


def test_planted_recording_is_recovered_with_margin():
    c = SP.planted()
    ref = SP.span_reference(c["x"], c["mu"], c["lv"], c["o"], c["lw"], c["D"])
    N, D, P = c["N"], c["D"], SP.PLANT_P
    assert {k for _, _, k in c["truth"]} == set(range(P)) and max(d for _, d, _ in c["truth"]) == D
    path = SP.viterbi_reference(ref["score"], ref["cat"], 1, c["gap"], 0.0)
    assert list(zip(path["onset"], path["length"], path["cat"])) == c["truth"]
    S, A = ref["S"], ref["A"]
    for s, d, k in c["truth"]:
        alt = max(S[s2, k2, d2 - 1] for s2, d2, k2 in SP.segment_alternatives(s, d, k, N, D, P))
        assert S[s, k, d - 1] - alt >= 4 * SP.BAR * A[s, k, d - 1], (s, d, k)
    # the whole path beats every path that differs in one boundary or one category by the same margin: rerun the
    # programme with the planted entry of one segment removed
    for s, d, k in c["truth"]:
        sc = ref["score"].copy()
        sc[s + d, d - 1] = NEG
        other = SP.viterbi_reference(sc, ref["cat"], 1, c["gap"], 0.0)
        assert path["path_score"] - other["path_score"] >= 4 * SP.BAR * A[s, k, d - 1]
    # and without a gap model the recording can still be tiled, by worse segments
    tiled = SP.viterbi_reference(ref["score"], ref["cat"], 1, None, 0.0)
    assert sum(tiled["length"]) == N and tiled["path_score"] < path["path_score"]


# ----------------------------------------------------------------------------
# surface
# ----------------------------------------------------------------------------
SYMS = ("abcd_span_scores_workspace_bytes", "abcd_span_scores", "abcd_span_viterbi_workspace_bytes",
        "abcd_span_viterbi")


def test_new_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in SYMS:
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.library_hash() == N.source_hash()
    ws = N.lib().abcd_span_scores_workspace_bytes
    assert ws(15000, 200, 128) >= 200 * 128 * 8
    assert ws(0, 1, 1) > 0 and ws(-1, 1, 1) == 0 and ws(4, 0, 1) == 0 and ws(4, 1, 0) == 0
    assert ws(4, 16383, 1) > 0 and ws(4, 16384, 1) == 0
    assert ws((1 << 31) // 8 - 2, 8, 1) > 0 and ws((1 << 31) // 8 - 1, 8, 1) == 0   # (N + 1) D < 2^31
    assert ws(1 << 40, 1, 1) == 0
    wv = N.lib().abcd_span_viterbi_workspace_bytes
    assert wv(15000, 200) >= 15001 * 4
    assert wv(0, 1) > 0 and wv(-1, 1) == 0 and wv(4, 0) == 0 and wv(4, 16383) > 0 and wv(4, 16384) == 0
    assert wv((1 << 31) // 8 - 2, 8) > 0 and wv((1 << 31) // 8 - 1, 8) == 0 and wv(1 << 40, 1) == 0


def test_span_entry_points_reject_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    fake = N.c_void_p(4096)
    E = N.ABCD_EINVAL
    n, F, P, D = 9, 4, 5, 3
    nb = lib.abcd_span_scores_workspace_bytes(n, D, P)

    def scores(x=fake, ldx=F, n=n, F=F, P=P, D=D, Tp=D, mu=fake, ldm=F, lv=fake, ldl=F, o=fake, lw=None, ss=fake,
               sc=fake, lds=D, ws=fake, nb=nb):
        return lib.abcd_span_scores(x, ldx, n, F, P, D, Tp, mu, ldm, lv, ldl, o, lw, ss, sc, lds, ws, nb, None)

    assert scores(D=0, Tp=4) == E and scores(D=16384, Tp=16384, lds=16384, nb=1 << 40) == E
    assert scores(P=0) == E and scores(F=0) == E and scores(n=-1) == E
    assert scores(n=(1 << 31) // 3, nb=1 << 40) == E                   # (N + 1) D >= 2^31
    assert scores(Tp=D - 1) == E
    assert scores(ldx=F - 1) == E and scores(ldm=F - 1) == E and scores(ldl=F - 1) == E and scores(lds=D - 1) == E
    for k in ("x", "mu", "lv", "o", "ss", "sc"):
        assert scores(**{k: None}) == E, k
    assert scores(ws=None) == E and scores(nb=nb - 1) == E and scores(nb=0) == E
    # N = 0 is valid; with nowhere to write row 0 it needs no device
    nb0 = lib.abcd_span_scores_workspace_bytes(0, D, P)
    assert scores(n=0, x=None, mu=None, lv=None, o=None, ss=None, sc=None, nb=nb0) == 0
    assert scores(n=0, ss=None, sc=None, ws=None, nb=nb0) == E

    nv = lib.abcd_span_viterbi_workspace_bytes(n, D)

    def vit(ss=fake, sc=fake, lds=D, n=n, D=D, dmin=1, gap=None, bonus=0.0, ps=fake, ns=fake, on=fake, ln=fake,
            ct=fake, sv=fake, V=None, ws=fake, nb=nv):
        return lib.abcd_span_viterbi(ss, sc, lds, n, D, dmin, gap, bonus, ps, ns, on, ln, ct, sv, V, ws, nb, None)

    assert vit(dmin=0) == E and vit(dmin=D + 1) == E
    assert vit(D=0) == E and vit(D=16384, lds=16384, nb=1 << 40) == E and vit(n=-1) == E
    assert vit(n=(1 << 31) // 3, nb=1 << 40) == E
    assert vit(lds=D - 1) == E
    for k in ("ss", "sc", "ps", "ns", "on", "ln", "ct", "sv"):
        assert vit(**{k: None}) == E, k
    assert vit(ws=None) == E and vit(nb=nv - 1) == E and vit(nb=0) == E
    nv0 = lib.abcd_span_viterbi_workspace_bytes(0, D)
    assert vit(n=0, ss=None, sc=None, ps=None, ns=None, on=None, ln=None, ct=None, sv=None, nb=nv0) == 0
    assert vit(n=0, dmin=0, ps=None, ns=None, nb=nv0) == E


def test_ops_and_methods_exist():
    from modules import model as M, ops, segmentation
    for name in ("span_scores", "span_viterbi"):
        assert name in ops.OPS and hasattr(torch.ops.abcd, name)
    assert set(ops.registered()) == set(ops.OPS)
    schema = str(torch.ops.abcd.span_scores.default._schema)
    assert schema.startswith("abcd::span_scores(Tensor frames, Tensor proto_mu, Tensor proto_lv, Tensor "
                             "proto_offset_logits, Tensor? log_weight, SymInt P, SymInt D) -> Tensor[]"), schema
    schema = str(torch.ops.abcd.span_viterbi.default._schema)
    assert schema.startswith("abcd::span_viterbi(Tensor span_score, Tensor span_cat, SymInt d_min, Tensor? gap, "
                             "float seg_bonus, bool want_v) -> Tensor[]"), schema
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        ss, sc = torch.ops.abcd.span_scores(torch.empty(9, 4), torch.empty(15, 4), torch.empty(15, 4), torch.empty(15),
                                            None, 5, 3)
        assert ss.shape == sc.shape == (10, 3) and ss.dtype == torch.float64 and sc.dtype == torch.int32
        out = torch.ops.abcd.span_viterbi(ss, sc, 2, None, 0.0, True)
        assert [tuple(t.shape) for t in out] == [(), (), (4,), (4,), (4,), (4,), (10,)]
        assert out[0].dtype == out[5].dtype == out[6].dtype == torch.float64 and out[2].dtype == torch.int32
    assert callable(M.RNN_Variational_Decoder.span_scores)
    # no CPU fallback anywhere
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    protos = (torch.zeros(3, 4, 33), torch.zeros(3, 4, 33), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        dec.span_scores(protos, torch.zeros(9, 33), 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        segmentation.segment_frames(dec, protos, torch.zeros(9, 33), 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.span_scores(torch.zeros(9, 4), torch.zeros(15, 4), torch.zeros(15, 4), torch.zeros(15), None, 5, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.span_viterbi(torch.zeros(10, 3, dtype=torch.float64), torch.zeros(10, 3, dtype=torch.int32), 1, None, 0.0,
                         False)


def test_gap_model_helpers():
    from modules import segmentation
    g = torch.Generator().manual_seed(3)
    x = torch.randn(50, 6, generator=g) * 2.0 + 1.0
    mask = torch.zeros(50, dtype=torch.bool)
    mask[10:30] = True
    mu, lv = segmentation.fit_gap_model(x, mask)
    keep = x[~mask].double()
    assert torch.allclose(mu, keep.mean(0)) and torch.allclose(lv.exp(), keep.var(0, unbiased=False))
    ll = segmentation.gap_scores(x, mu, lv)
    want = torch.distributions.Normal(mu, (0.5 * lv).exp()).log_prob(x.double()).sum(1)
    assert ll.dtype == torch.float32 and ll.shape == (50,) and torch.allclose(ll.double(), want, rtol=1e-6)
    with pytest.raises(ValueError):
        segmentation.fit_gap_model(x, torch.ones(50, dtype=torch.bool))


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def test_segment_cli_arguments():
    import classify
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
    a = segment.get_parameters(["c", "r", "t", "1", "--max_length", "9", "--fit_gap", "ann.csv", "--gap_model_out",
                                "g.npz"])
    assert (a.fit_gap, a.gap_model_out) == ("ann.csv", "g.npz")
    base = ["c", "r", "t", "1"]
    for bad in ([], ["--max_length", "0"], ["--max_length", "16384"], ["--max_length", "5", "--min_length", "6"],
                ["--max_length", "5", "--min_length", "0"], ["--max_length", "5", "--prior", "flat"],
                ["--max_length", "5", "--entire_data_size", "0"],
                ["--max_length", "5", "--gap_score", "-1", "--gap_model", "g.npz"],
                ["--max_length", "5", "--fit_gap", "a.csv"], ["--max_length", "5", "--gap_model_out", "g.npz"]):
        with pytest.raises(SystemExit):
            segment.get_parameters(base + bad)
    # the same checkpoint, STFT, epsilon, normaliser and channel arguments as classify.py
    c = vars(classify.get_parameters(base))
    s = vars(segment.get_parameters(base + ["--max_length", "5"]))
    for k in ("model_path", "input_root", "data_normalizer", "annotation_sep", "device", "fft_frame_length",
              "fft_step_size", "fft_window_type", "fft_no_centering", "channel", "epsilon", "prior",
              "entire_data_size"):
        assert s[k] == c[k], k


@pytest.mark.parametrize("centering", [True, False])
def test_frames_to_seconds_round_trip_through_the_loader(tmp_path, centering):
    """A synthetic segment table written by segment.py's writer and read back
    through Data_Parser on the toy wav gives every segment exactly its frames,
    centred on the whole-recording frames it was cut from."""
    import segment
    from modules import data_utils
    from modules.data_utils import Compose
    wav = pd.read_csv(ANN)["input_path"][0]
    fs, wave = segment.read_wave(TOY, wav)
    frame, hop = int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))
    total = len(wave)
    stft = data_utils.STFT(frame, hop, centering=centering)
    whole = stft(torch.from_numpy(wave))
    n = whole.shape[0]
    assert n == segment.num_frames(total, frame, hop, centering)
    d0 = segment.min_loadable_length(frame, hop, centering)
    assert d0 == (2 if centering else 1)
    # segments that tile the recording, the shortest loadable one and the last frame among them
    onset, length, at, g = [], [], 0, np.random.default_rng(0)
    while at < n:
        d = min(int(g.integers(d0, 40)), n - at)
        if n - at - d < d0:
            d = n - at
        onset.append(at)
        length.append(d)
        at += d
    length[0], onset[1], length[1] = d0, d0, length[1] + length[0] - d0
    rows = segment.segment_rows(wav, onset, length, [3] * len(onset), [-1.5] * len(onset), fs, frame, hop, centering,
                                total)
    out = os.path.join(str(tmp_path), "segmented.csv")
    assert segment.write_segments(out, rows) == len(onset)
    assert segment.write_segments(out, rows) == len(onset) and os.path.isfile(out + ".prev")
    df = pd.read_csv(out)
    assert list(df.columns) == list(segment.COLUMNS)
    assert (df["label"] == 3).all() and (df["category_ix"] == 3).all() and df["length"].tolist() == length
    parser = data_utils.Data_Parser(TOY, out)
    ds = parser.get_data(transform=Compose([data_utils.ToTensor(), stft]))
    assert len(ds) == len(onset)
    for i, (s, d) in enumerate(zip(onset, length)):
        seq, _ = ds[i]
        assert seq.shape[0] == d, (i, s, d)
        assert int(ds.df_annotation["onset_ix"][i]) == s * hop
        inner = slice(2, d - 2) if centering else slice(0, d)     # away from the segment's own edge padding
        if d > 4 or not centering:
            assert torch.allclose(seq[inner], whole[s:s + d][inner], rtol=1e-4, atol=1e-3 * float(whole.max()))
    on = df["onset"].to_numpy()
    off = df["offset"].to_numpy()
    assert (on[1:] >= on[:-1]).all() and (off <= total / fs + 1e-12).all()
    if centering:
        assert (off[:-1] < on[1:]).all()
    mask = segment.covered_frames(n, on[:1], off[:1], fs, frame, hop, centering)
    assert mask[:d0].all() and not mask[d0 + (0 if centering else 2):].any()


@pytest.mark.parametrize("with_gap", (False, True), ids=("nogap", "gap"))
def test_tail_cases_reach_past_the_register_candidates(with_gap):
    """The conditions of span_cases.TAIL_CASES on the float64 loop alone: the
    forced case has a cover and every segment of it is a loop candidate; the
    mixed case's best path holds segments of both kinds."""
    forced, mixed = SP.tail_viterbi("forced", with_gap), SP.tail_viterbi("mixed", with_gap)
    N, D, d_min = SP.TAIL_CASES["forced"]
    assert d_min >= SP.TAIL_FROM and 2 * d_min <= N <= 2 * D
    if not with_gap:                                # nothing but the six pairs (1025, 1030) .. (1030, 1025)
        assert sum(1 for a in range(d_min, D + 1) if d_min <= N - a <= D) == 6 and N < 3 * d_min
        assert len(forced["length"]) == 2 and sum(forced["length"]) == N
    assert forced["path_score"] > NEG and forced["length"] and min(forced["length"]) >= SP.TAIL_FROM
    lengths = np.array(mixed["length"])
    print(f"mixed: {(lengths >= SP.TAIL_FROM).sum()} long and {(lengths < SP.TAIL_FROM).sum()} short segments")
    assert (lengths >= SP.TAIL_FROM).any() and (lengths < SP.TAIL_FROM).any()
