"""Syntax-aware segmentation with the table in windows, on the GPU:
``abcd_span_chain_viterbi_window`` through the C ABI, ``abcd_span_table`` on
slices of the frames, ``segment_frames(transitions=..., window_frames=W)`` end
to end and ``segment.py --window_frames``.

Every bar is EQUALITY of bits: the windowed programme against
``abcd_span_chain_viterbi`` on the whole table and against the float64 loop of
``syntax_cases.chain_reference`` in every output; a slice's table against rows
n0 .. n1 of the one-shot table; the windowed dict against the one-shot dict in
every key; the CLI's bytes.  Every buffer is guarded: the windows' tables carry
NaN in the padding columns, in the rows below n0 - row0 and in a tail row, the
outputs hold a sentinel with one extra entry each, the workspace 0xFF and a
tail."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import score_cases as S
import stream_cases as ST
import syntax_cases as SX
from test_gpu_score import ANN, CKPT, TOY
from test_gpu_span import _bits, span_buffers
from test_gpu_syntax import _small_recording, chain_call, table_call

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")
SENT = -7.0  # what the outputs hold before a call
TAIL = 64    # guard bytes behind the workspace


# ----------------------------------------------------------------------------
# 1. abcd_span_chain_viterbi_window through ctypes, on synthetic tables
# ----------------------------------------------------------------------------
class Windowed:
    """One recording's device buffers for sequences of window calls: the whole
    table (from which every window's own guarded buffer is cut), log_trans with
    NaN padding, the guarded outputs and the workspace."""

    def __init__(self, table, trans, init, d_min):
        from modules import _native as N_
        self.N_, self.lib = N_, N_.lib()
        self.N, self.D, self.K = table.shape[0] - 1, table.shape[1], table.shape[2]
        N, K = self.N, self.K
        self.full = torch.from_numpy(np.ascontiguousarray(table)).cuda()
        lt = torch.full((K, K + 2), NAN)
        lt[:, :K] = torch.from_numpy(np.asarray(trans, dtype=np.float32))
        self.lt, self.li = lt.cuda(), torch.from_numpy(np.asarray(init, dtype=np.float32)).cuda()
        self.d_min, self.cap = d_min, N // d_min
        self.nbytes = self.lib.abcd_span_chain_window_workspace_bytes(N, self.D, K)
        assert self.nbytes >= 24 * (N + 1) * K
        self.ws = torch.full((self.nbytes + TAIL,), 0xFF, dtype=torch.uint8, device="cuda")
        self.fresh()

    def fresh(self):
        f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        self.ps, self.ns = torch.full((2,), SENT, **f64), torch.full((2,), int(SENT), **i32)
        self.on, self.ln, self.ct = (torch.full((self.cap + 1,), int(SENT), **i32) for _ in range(3))
        self.sv, self.lk = torch.full((self.cap + 1,), SENT, **f64), torch.full((self.cap + 1,), SENT, **f64)
        self.W = torch.full((self.N + 2, self.K), SENT, **f64)

    def window(self, row0, n0, n1):
        """The window's table in a buffer of its own: rows row0 .. n1 with ld_k
        = K + 3; the padding columns, the rows below n0 - row0 and a tail row
        hold NaN."""
        K = self.K
        buf = torch.full((n1 - row0 + 2, self.D, K + 3), NAN, dtype=torch.float64, device="cuda")
        buf[n0 - row0:n1 - row0 + 1, :, :K] = self.full[n0:n1 + 1]
        return buf

    def call(self, row0, n0, n1, gap, bonus, want_w=True):
        p = self.N_.ptr
        buf = self.window(row0, n0, n1)
        return self.lib.abcd_span_chain_viterbi_window(
            p(buf), K3(self.K), row0, n1 - row0 + 1, n0, n1, self.N, self.D, self.K, self.d_min, p(gap), float(bonus),
            p(self.lt), self.K + 2, p(self.li), p(self.ps), p(self.ns), p(self.on), p(self.ln), p(self.ct), p(self.sv),
            p(self.lk), p(self.W) if want_w else None, p(self.ws), self.nbytes, self.N_.stream())

    def unfinished(self):
        """No call with n1 = N has run: only W_out was written."""
        assert float(self.ps[0]) == SENT and int(self.ns[0]) == int(SENT)
        for t in (self.on, self.ln, self.ct):
            assert (t == int(SENT)).all()
        assert (self.sv == SENT).all() and (self.lk == SENT).all()

    def result(self, want_w=True):
        """The outputs after the last window, the guards checked."""
        torch.cuda.synchronize()
        k = int(self.ns[0])
        assert 0 <= k <= self.cap
        assert float(self.ps[1]) == SENT and int(self.ns[1]) == int(SENT)
        for t in (self.on, self.ln, self.ct):
            assert (t[k:] == int(SENT)).all()
        assert (self.sv[k:] == SENT).all() and (self.lk[k:] == SENT).all()
        assert (self.W[self.N + 1] == SENT).all() and (want_w or (self.W == SENT).all())
        assert (self.ws[self.nbytes:] == 0xFF).all()
        return dict(path_score=float(self.ps[0]), n=k, onset=self.on[:k].tolist(), length=self.ln[:k].tolist(),
                    cat=self.ct[:k].tolist(), score=self.sv[:k].tolist(), link=self.lk[:k].tolist(),
                    W=self.W[:self.N + 1].cpu().numpy() if want_w else None)

    def run(self, plan, gap, bonus, want_w=True):
        self.fresh()
        for i, (row0, n0, n1) in enumerate(plan):
            assert self.call(row0, n0, n1, gap, bonus, want_w) == 0
        return self.result(want_w)


def K3(K):
    return K + 3


def _same(got, ref, tag):
    """A windowed result (dict of ``Windowed.result``) against ``chain_call``'s
    dict or ``chain_reference``'s: bit for bit."""
    assert np.array_equal(got["W"].view(np.int64), np.asarray(ref["W"]).view(np.int64)), \
        (tag, np.argwhere(got["W"].view(np.int64) != np.asarray(ref["W"]).view(np.int64))[:4])
    assert np.float64(got["path_score"]).view(np.int64) == np.float64(ref["path_score"]).view(np.int64), tag
    assert got["n"] == len(ref["onset"]), tag
    for key in ("onset", "length", "cat"):
        assert got[key] == list(ref[key]), (tag, key)
    for key in ("score", "link"):
        a, b = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (tag, key)


def check_windows(N, D, K, kind):
    c = SX.chain_inputs(N, D, K, kind)
    by_dmin = {}
    launches = segments = 0
    for i, (d_min, gap, bonus, tag) in enumerate(c["calls"]):
        ref = ST.reference(N, D, K, kind, i)                               # the float64 loop on the whole table
        one = chain_call(c["table"], d_min, gap, bonus, c["trans"], c["init"])   # abcd_span_chain_viterbi on it
        segments += len(ref["onset"])
        if d_min not in by_dmin:
            by_dmin[d_min] = Windowed(c["table"], c["trans"], c["init"], d_min)
        w = by_dmin[d_min]
        g = None if gap is None else torch.from_numpy(np.asarray(gap, dtype=np.float32)).cuda()
        for W in ST.window_sizes(N, D):
            plan = ST.plan(N, D, W)
            got = w.run(plan, g, bonus)
            launches += len(plan)
            _same(got, one, (N, D, K, kind, tag, W, "one-shot"))
            _same(got, ref, (N, D, K, kind, tag, W, "float64 loop"))
        # a second run on the used workspace (n0 = 1 starts over), the windows of W = D: equal
        again = w.run(ST.plan(N, D, D), g, bonus)
        _same(again, one, (N, D, K, kind, tag, "second run"))
    return launches, segments


@pytest.mark.parametrize("kind", SX.CHAIN_KINDS)
@pytest.mark.parametrize("K", ST.STREAM_K)
@pytest.mark.parametrize("ND", ST.STREAM_ND, ids=lambda v: f"n{v[0]}d{v[1]}")
def test_windowed_programme_is_the_one_shot_programme(ND, K, kind):
    N, D = ND
    launches, segments = check_windows(N, D, K, kind)
    print(f"N={N} D={D} K={K} {kind}: {launches} window launches, {segments} segments in the references; every output "
          "equal to the one-shot call and to the float64 loop")
    if kind in ("random", "tied", "gaps", "bonus"):
        assert segments > 0


@pytest.mark.parametrize("kind", SX.CHAIN_KINDS)
@pytest.mark.parametrize("K", ST.WIDTH_K)
def test_windowed_programme_at_the_launch_width_threshold(K, kind):
    """K = 256 is the last shape of the 16-wave launch, 257 the first of the
    4-wave one (abcd_span_chain_plan)."""
    from modules import _native as N_
    thr = N_.c_int(-1)
    assert N_.lib().abcd_span_chain_plan(K, 5, None, N_.ctypes.byref(thr), None) == 0
    assert thr.value == (1024 if K <= 256 else 256)
    check_windows(33, 5, K, kind)


def test_windowed_programme_without_w_out_and_reads_only_its_rows():
    N, D, K = 70, 17, 130
    c = SX.chain_inputs(N, D, K, "random")
    d_min, gap, bonus, _ = c["calls"][1]
    g = torch.from_numpy(gap).cuda()
    w = Windowed(c["table"], c["trans"], c["init"], d_min)
    a = w.run(ST.plan(N, D, 7), g, bonus)
    b = w.run(ST.plan(N, D, 7), g, bonus, want_w=False)
    assert b["W"] is None
    for key in ("path_score", "n", "onset", "length", "cat", "score", "link"):
        assert a[key] == b[key], key
    # nothing but W_out is written before the last window
    w.fresh()
    plan = ST.plan(N, D, 20)
    for row0, n0, n1 in plan[:-1]:
        assert w.call(row0, n0, n1, g, bonus) == 0
        torch.cuda.synchronize()
        w.unfinished()
        assert (w.W[n1 + 1:] == SENT).all() and not (w.W[:n1 + 1] == SENT).any()
    assert w.call(*plan[-1], g, bonus) == 0
    _same(w.result(), a, "after the partial runs")
    # windows of unequal sizes, and a window whose buffer starts earlier than it must
    got = w.run([(0, 1, 1), (0, 2, 30), (0, 31, 31), (0, 32, 69), (32, 70, 70)], g, bonus)
    _same(got, a, "unequal windows")


def test_a_call_out_of_order_is_visible_and_harmless():
    N, D, K = 33, 5, 33
    c = SX.chain_inputs(N, D, K, "random")
    d_min, gap, bonus, _ = c["calls"][1]
    g = torch.from_numpy(gap).cuda()
    ref = ST.reference(N, D, K, "random", 1)
    w = Windowed(c["table"], c["trans"], c["init"], d_min)
    # on a workspace nothing has run on (0xFF everywhere): n0 = 12 follows nothing
    assert w.call(ST.ALIGN * 0, 12, 20, g, bonus) == 0
    torch.cuda.synchronize()
    assert np.isnan(float(w.ps[0])) and int(w.ns[0]) == -1
    assert (w.W == SENT).all() and (w.ws[:w.nbytes] == 0xFF).all()          # no step ran, the carry is untouched
    # after windows 1 .. 10, the window 12 .. 20 skips end 11
    w.fresh()
    assert w.call(0, 1, 10, g, bonus) == 0
    torch.cuda.synchronize()
    w.unfinished()
    before = w.ws.clone()
    assert w.call(0, 12, 20, g, bonus) == 0
    torch.cuda.synchronize()
    assert np.isnan(float(w.ps[0])) and int(w.ns[0]) == -1
    assert torch.equal(w.ws, before) and (w.W[11:] == SENT).all()
    # ... and repeating a window is refused as well
    assert w.call(0, 5, 10, g, bonus) == 0
    torch.cuda.synchronize()
    assert np.isnan(float(w.ps[0])) and int(w.ns[0]) == -1 and torch.equal(w.ws, before)
    # the carry is intact: the due window goes on
    w.ps.fill_(SENT)
    w.ns.fill_(int(SENT))
    assert w.call(0, 11, 33, g, bonus) == 0
    _same(w.result(), ref, "resumed")
    # a finished recording takes no further window but n0 = 1
    assert w.call(0, 20, 33, g, bonus) == 0
    torch.cuda.synchronize()
    assert np.isnan(float(w.ps[0])) and int(w.ns[0]) == -1
    # a correct sequence from n0 = 1 on the same workspace gives the right result
    _same(w.run(ST.plan(N, D, 3), g, bonus), ref, "from n0 = 1 again")


def test_window_operator():
    from modules import ops
    N, D, K = 33, 5, 33
    c = SX.chain_inputs(N, D, K, "random")
    d_min, gap, bonus, _ = c["calls"][1]
    ref = ST.reference(N, D, K, "random", 1)
    tb = torch.from_numpy(c["table"]).cuda()
    lt, li = torch.from_numpy(c["trans"]).cuda(), torch.from_numpy(c["init"]).cuda()
    g = torch.from_numpy(gap).cuda()
    state = ops.span_chain_window_state(N, D, K, "cuda")
    Wt = torch.full((N + 1, K), SENT, dtype=torch.float64, device="cuda")
    plan = ST.plan(N, D, 7)
    for row0, n0, n1 in plan:
        out = ops.span_chain_viterbi_window(tb[row0:n1 + 1], row0, n0, n1, N, d_min, g, bonus, lt, li, state, Wt)
        if n1 < N:
            assert np.isnan(float(out[0])) and int(out[1]) == -1            # not finished
    k = int(out[1])
    assert float(out[0]) == ref["path_score"] and k == len(ref["onset"])
    assert out[2][:k].tolist() == ref["onset"] and out[3][:k].tolist() == ref["length"]
    assert out[4][:k].tolist() == ref["cat"] and out[5][:k].tolist() == ref["score"]
    assert out[6][:k].tolist() == ref["link"]
    assert [tuple(t.shape) for t in out[2:]] == [(N // d_min,)] * 5
    assert np.array_equal(Wt.cpu().numpy().view(np.int64), ref["W"].view(np.int64))
    one = ops.span_chain_viterbi(tb, d_min, g, bonus, lt, li, True)
    for a, b in zip(out, one[:7]):
        assert torch.equal(_bits(a[:k] if a.dim() else a), _bits(b[:k] if b.dim() else b))
    # out of order through the operator
    out = ops.span_chain_viterbi_window(tb[0:21], 0, 12, 20, N, d_min, g, bonus, lt, li, state, None)
    assert np.isnan(float(out[0])) and int(out[1]) == -1
    for bad in (dict(n0=0), dict(n1=N + 1), dict(row0=1), dict(n0=12, n1=25, row0=0, rows=21)):
        a = dict(row0=0, n0=1, n1=7, rows=8)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.span_chain_viterbi_window(tb[a["row0"]:a["row0"] + a["rows"]], a["row0"], a["n0"], a["n1"], N, d_min,
                                          g, bonus, lt, li, state, None)
    with pytest.raises(ValueError):
        ops.span_chain_viterbi_window(tb[:8], 0, 1, 7, N, d_min, g, bonus, lt, li, state[:100], None)
    with pytest.raises(ValueError):
        ops.span_chain_viterbi_window(tb[:8], 0, 1, 7, N, d_min, g, bonus, lt, li, state, Wt[:5])


# ----------------------------------------------------------------------------
# 2. abcd_span_table on slices of the frames
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("P", ST.SLICE_P)
@pytest.mark.parametrize("D", ST.SLICE_D)
def test_a_slice_s_table_is_the_one_shot_table(D, P):
    N, F = ST.SLICE_N, ST.SLICE_F
    c = ST.slice_inputs(N, D, P, F)
    b = span_buffers(c, SX.SP.PAD_LD)
    ldk = P + 3
    rc, full, _, _ = table_call(c, b, ldk, False)
    assert rc == 0
    starts = set()
    for W in ST.SLICE_W:
        for row0, n0, n1 in ST.plan(N, D, W):
            starts.add(row0)
            x = b["x"].clone()
            x[n1:] = NAN                                                    # the slice ends at n1: nothing behind it is read
            rc, part, _, _ = table_call(c, dict(b, x=x[row0:]), ldk, False, n=n1 - row0)
            assert rc == 0
            assert (part[n1 - row0 + 1:] == -7.0).all() and (part[:, :, P:] == -7.0).all()
            assert torch.equal(_bits(part[n0 - row0:n1 - row0 + 1, :, :P]), _bits(full[n0:n1 + 1, :, :P])), \
                (D, P, W, row0, n0, n1)
    assert starts == ({0, 32, 64, 96} if D == 17 else {0, 32, 64})          # the last n0 is 129: 129 - 37 = 92 -> 64
    print(f"N={N} D={D} P={P} F={F}: the tables of the slices that start at {sorted(starts)} equal the one-shot "
          "table's rows bit for bit")


# ----------------------------------------------------------------------------
# 3. segment_frames(transitions=..., window_frames=W) on the small models
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.E2E_SMALL))
def test_segment_frames_in_windows_is_segment_frames(name):
    from modules import segmentation
    from modules.sequence import TransitionModel
    dec, protos, frames, K, D = _small_recording(name)
    n = int(frames.shape[0])
    lw = torch.linspace(-1.0, 1.0, K).cuda()
    g = torch.Generator().manual_seed(5)
    model = TransitionModel(K).cuda()
    model.set_probabilities(torch.softmax(torch.randn(K, K, generator=g) * 2.0, 1), torch.softmax(lw.double().cpu(), 0))
    tiled = segmentation.segment_frames(dec, protos, frames, D, log_weight=lw)
    const = torch.full((n,), float(tiled["path_score"]) / n, device="cuda")
    odd = next(w for w in (5, 9, 11, 13) if n % w)                          # a size that does not divide N
    sizes = sorted({1, 7, D, odd, n, n + 5})
    keys = ("onset", "length", "category", "score", "path_score", "link", "context_free_category")
    counts = []
    low = const - const.abs()                                               # a costlier gap: fewer frames left uncovered
    for gap, bonus, d_min in ((None, 0.0, 1), (None, -3.0, 2), (const, 0.0, 1), (const, -3.0, 2), (low, 0.0, 1)):
        kw = dict(min_length=d_min, gap=gap, seg_bonus=bonus, log_weight=lw, transitions=model)
        one = segmentation.segment_frames(dec, protos, frames, D, **kw)
        assert set(one) == set(keys)
        counts.append((int(one["onset"].numel()), float(one["path_score"])))
        for W in sizes:
            got = segmentation.segment_frames(dec, protos, frames, D, window_frames=W, **kw)
            assert set(got) == set(one)
            for key in keys:
                assert got[key].dtype == one[key].dtype and got[key].shape == one[key].shape, (name, W, key)
                assert torch.equal(_bits(got[key]), _bits(one[key])), (name, W, key)
    w2 = segmentation.segment_frames(dec, protos, frames, D, window_frames=7, include_weight=True, log_weight=lw,
                                     transitions=model)
    o2 = segmentation.segment_frames(dec, protos, frames, D, include_weight=True, log_weight=lw, transitions=model)
    for key in keys:
        assert torch.equal(_bits(w2[key]), _bits(o2[key])), key
    print(f"{name}: N = {n}, D = {D}, K = {K}: window_frames in {sizes} equal to the one-shot dict in every key; "
          f"(segments, path score) of the five settings: {counts}")
    assert max(c for c, _ in counts) >= 1                                   # some setting cuts the recording
    with pytest.raises(ValueError, match="posteriors"):
        segmentation.segment_frames(dec, protos, frames, D, transitions=model, window_frames=7, posteriors=True)
    with pytest.raises(ValueError, match="transitions"):
        segmentation.segment_frames(dec, protos, frames, D, window_frames=7)
    with pytest.raises(ValueError):
        segmentation.segment_frames(dec, protos, frames, D, transitions=model, window_frames=0)
    e = segmentation.segment_frames(dec, protos, frames[:0], D, transitions=model, window_frames=7)
    assert float(e["path_score"]) == 0.0 and e["onset"].numel() == 0


def test_planted_alternation_in_windows():
    """``segment_frames`` on a decoder cannot plant a table, so the planted
    alternation runs through what ``segment_frames(window_frames=5)`` runs on its
    windows' tables: ``plan_windows`` and the window operator."""
    from modules import ops, segmentation
    c = SX.planted_alternation()
    N, D = c["N"], c["D"]
    tb = torch.from_numpy(c["table"]).cuda()
    lt, li = torch.from_numpy(c["trans"]).cuda(), torch.from_numpy(c["init"]).cuda()
    state = ops.span_chain_window_state(N, D, 2, "cuda")
    for row0, n0, n1 in segmentation.plan_windows(N, D, 5):
        out = ops.span_chain_viterbi_window(tb[row0:n1 + 1], row0, n0, n1, N, 1, None, 0.0, lt, li, state, None)
    k = int(out[1])
    assert k == SX.ALT_SEGMENTS and out[3][:k].tolist() == [SX.ALT_L] * k
    assert out[2][:k].tolist() == [SX.ALT_L * i for i in range(k)]
    assert out[4][:k].tolist() == [i % 2 for i in range(k)]                 # the alternation
    ref = SX.chain_reference(c["table"], 1, c["trans"], c["init"])
    assert float(out[0]) == ref["path_score"] and out[6][:k].tolist() == ref["link"]


def test_one_shot_refusal_names_window_frames():
    from modules import _native as N_, segmentation
    K, D, n, F = 128, 300, 70000, 4                  # (N + 1) D K >= 2^31 while (N + 1) D < 2^31
    dec = None                                       # refused before the decoder is asked for anything
    protos = (torch.zeros(D, K, F).cuda(), torch.zeros(D, K, F).cuda(), torch.zeros(D, K).cuda())
    pair = (torch.zeros(K, K).cuda(), torch.zeros(K).cuda())
    with pytest.raises(N_.HipError, match="index limit.*window_frames"):
        segmentation.segment_frames(dec, protos, torch.zeros(n, F).cuda(), D, transitions=pair)


# ----------------------------------------------------------------------------
# 4. segment.py --window_frames on the toy data
# ----------------------------------------------------------------------------
def test_segment_cli_with_window_frames(tmp_path):
    import segment
    K = 16
    base = [CKPT, TOY, ANN, "1.0", "--max_length", "60", "--min_length", "3"]
    p = np.full((K, K), 0.2 / (K - 1))
    np.fill_diagonal(p, 0.8)
    ft, tt = np.divmod(np.arange(K * K), K)
    tcsv = os.path.join(str(tmp_path), "transitions.csv")
    pd.DataFrame({"from_ix": ft, "to_ix": tt, "probability": p.reshape(-1), "expected_count": 0.0}).to_csv(
        tcsv, index=False)
    out_t = os.path.join(str(tmp_path), "t", "segmented.csv")
    assert segment.main(base + ["-S", out_t, "--transitions", tcsv]) == out_t
    out_w = os.path.join(str(tmp_path), "w", "segmented.csv")
    assert segment.main(base + ["-S", out_w, "--transitions", tcsv, "--window_frames", "16"]) == out_w
    with open(out_t, "rb") as f, open(out_w, "rb") as g:
        a, b = f.read(), g.read()
    assert a == b and len(pd.read_csv(out_w)) >= 1
    # Viterbi training in windows: the same matrix, the same cut
    outs = []
    for tag, extra in (("r1", []), ("r2", ["--window_frames", "16"])):
        o = os.path.join(str(tmp_path), tag, "segmented.csv")
        t = os.path.join(str(tmp_path), tag, "transitions.csv")
        segment.main(base + ["-S", o, "--transitions", tcsv, "--refit_transitions", "1", "--transitions_out", t] + extra)
        with open(o, "rb") as f, open(t, "rb") as g:
            outs.append((f.read(), g.read()))
    assert outs[0] == outs[1]
