"""Syntax-aware segmentation on the GPU: ``abcd_span_table`` and
``abcd_span_chain_viterbi`` through the C ABI and the operators,
``segment_frames(transitions=...)`` end to end and ``segment.py
--transitions``, against the float64 references of ``syntax_cases.py`` and
``span_cases.py``.

Bars: every table entry within ``span_cases.BAR`` (1e-4) of its unit ``A`` of
``span_reference``'s ``S``; impossible entries exactly -inf; the table's
maximum over the categories, its lowest argmax and the optional best outputs
EQUAL to ``abcd_span_scores``' bits; the dynamic programme EQUAL to the float64
loop in every output; ``path_score`` within 1e-9 of the sum of the absolute
values of its own terms; the context-free chain's path score within 1e-9
relative of the context-free programme's.  Every observed figure is printed
(``-rA``) and kept with ``ABCD_PARITY_DUMP`` (profiles/syntax_errors.json)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import score_cases as S
import span_cases as SP
import syntax_cases as SX
from test_gpu_score import ANN, CKPT, TOY, _small_modules
from test_gpu_span import _bits, span_buffers, span_call

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")
SENT = -7.0  # what the outputs hold before a call


# ----------------------------------------------------------------------------
# 1. abcd_span_table through ctypes
# ----------------------------------------------------------------------------
def table_call(c, b, ldk, want_best, n=None):
    """abcd_span_table on span_buffers' arrays -> (rc, table, score, cat):
    (N + 2) x D x ldk and (N + 2) x (D + 1) buffers holding SENT before the
    call (score / cat None without want_best); the workspace holds NaN."""
    from modules import _native as N
    lib = N.lib()
    n = c["N"] if n is None else n
    D, P, F = c["D"], c["P"], c["F"]
    table = torch.full((n + 2, D, ldk), SENT, dtype=torch.float64, device="cuda")
    score = torch.full((n + 2, D + 1), SENT, dtype=torch.float64, device="cuda") if want_best else None
    cat = torch.full((n + 2, D + 1), int(SENT), dtype=torch.int32, device="cuda") if want_best else None
    ws = N.workspace(lib.abcd_span_table_workspace_bytes(n, D, P, ldk), "cuda")
    ws.fill_(0xFF)
    rc = lib.abcd_span_table(N.ptr(b["x"]), b["ldx"], n, F, P, D, D + SP.T_EXTRA, N.ptr(b["mu"]), b["ldm"],
                             N.ptr(b["lv"]), b["ldl"], N.ptr(b["o"]), N.ptr(b["lw"]), N.ptr(table), ldk, N.ptr(score),
                             N.ptr(cat), D + 1, N.ptr(ws), ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, table, score, cat


@pytest.mark.parametrize("F", SP.ABI_F)
@pytest.mark.parametrize("P", SP.ABI_P)
@pytest.mark.parametrize("ND", SX.table_shapes(), ids=lambda v: f"n{v[0]}d{v[1]}")
def test_span_table_abi(ND, P, F):
    N, D = ND
    c = SP.abi_inputs(N, D, P, F)
    ref = c["ref"]
    valid = np.zeros((N + 1, D), dtype=bool)
    for e in range(1, N + 1):
        valid[e, :min(D, e)] = True
    ee, dd = np.nonzero(valid)
    ix = np.arange(len(ee))
    S_at = ref["S"][ee - dd - 1][ix, :, dd]         # (entries, P): each entry's P scores
    A_at = ref["A"][ee - dd - 1][ix, :, dd]
    assert np.isfinite(S_at).all()
    rows = []
    for ld in (F, SP.PAD_LD):
        b = span_buffers(c, ld)                     # NaN in padding columns, tail rows and the steps >= D
        rc, score0, cat0 = span_call(c, **b)        # abcd_span_scores on the same buffers
        assert rc == 0
        for ldk in (P, P + 3):
            rc, table, score, cat = table_call(c, b, ldk, True)
            assert rc == 0
            assert (table[N + 1:] == SENT).all() and (table[:, :, P:] == SENT).all()   # nothing outside N + 1 x D x P
            assert (score[:, D:] == SENT).all() and (score[N + 1:] == SENT).all()
            assert (cat[:, D:] == int(SENT)).all() and (cat[N + 1:] == int(SENT)).all()
            tb = table[:N + 1, :, :P]
            t = tb.cpu().numpy()
            assert (t[~valid] == NEG).all()                                             # exactly -inf
            err = np.abs(t[ee, dd] - S_at) / A_at
            print(f"N={N} D={D} P={P} F={F} ld={ld} ld_k={ldk}: worst |table - S| / A {err.max():.2e}")
            rows.append(dict(N=N, D=D, P=P, F=F, ld=ld, ld_k=ldk, table=float(err.max())))
            assert np.isfinite(err).all() and err.max() <= SP.BAR
            # the maximum over the categories and its lowest argmax: abcd_span_scores' bits
            best = tb.max(-1).values
            lowest = torch.where(tb == best[..., None], torch.arange(P, device="cuda"), P).min(-1).values
            lowest = torch.where(best > NEG, lowest, -1).to(torch.int32)
            assert torch.equal(_bits(best), _bits(score0[:N + 1, :D])) and torch.equal(lowest, cat0[:N + 1, :D])
            # the optional outputs of the same pass hold those bits too
            assert torch.equal(_bits(score), _bits(score0)) and torch.equal(cat, cat0)
            # a second call, and one without the best outputs: bit for bit
            rc, table2, score2, cat2 = table_call(c, b, ldk, True)
            assert rc == 0 and torch.equal(_bits(table), _bits(table2))
            assert torch.equal(_bits(score), _bits(score2)) and torch.equal(cat, cat2)
            rc, table3, _, _ = table_call(c, b, ldk, False)
            assert rc == 0 and torch.equal(_bits(table), _bits(table3))
    SX.dump(f"table_n{N}d{D}p{P}f{F}", rows)


def test_span_table_exclusions_and_empty_recording():
    N, D, P, F = 70, 17, 33, 65
    c = SP.abi_inputs(N, D, P, F)
    b = span_buffers(c, SP.PAD_LD)
    rc, table, _, _ = table_call(c, b, P + 3, False)
    assert rc == 0
    tb = table[:N + 1, :, :P]
    # a NaN frame makes -inf of exactly the spans that contain it, under every category
    n0 = 40
    x = c["x"].clone()
    x[n0, F // 2] = NAN
    rc, t2, s2, c2 = table_call(c, span_buffers(c, SP.PAD_LD, x=x), P + 3, True)
    assert rc == 0
    e = torch.arange(N + 1)[:, None]
    d = torch.arange(1, D + 1)[None, :]
    hit = ((e - d <= n0) & (n0 < e) & (d <= e)).cuda()
    assert (t2[:N + 1, :, :P][hit] == NEG).all() and (s2[:N + 1, :D][hit] == NEG).all()
    assert (c2[:N + 1, :D][hit] == -1).all()
    assert torch.equal(_bits(t2[:N + 1, :, :P][~hit]), _bits(tb[~hit]))
    # a -inf or NaN weight removes its category alone
    for bad in (NEG, NAN):
        lw = c["lw"].clone()
        lw[5] = bad
        rc, t3, _, _ = table_call(c, span_buffers(c, SP.PAD_LD, lw=lw.cuda()), P + 3, False)
        assert rc == 0 and (t3[:N + 1, :, 5] == NEG).all()
        keep = [p for p in range(P) if p != 5]
        assert torch.equal(_bits(t3[:N + 1, :, keep]), _bits(tb[:, :, keep]))
    # a NULL weight vector counts as zeros
    rc, t4, _, _ = table_call(c, span_buffers(c, SP.PAD_LD, lw=None), P, False)
    rc5, t5, _, _ = table_call(c, span_buffers(c, SP.PAD_LD, lw=torch.zeros(P).cuda()), P, False)
    assert rc == 0 and rc5 == 0 and torch.equal(_bits(t4), _bits(t5))
    # N = 0 writes row 0 only
    rc, t6, s6, c6 = table_call(c, b, P + 3, True, n=0)
    assert rc == 0 and (t6[0, :, :P] == NEG).all() and (t6[0, :, P:] == SENT).all() and (t6[1:] == SENT).all()
    assert (s6[0, :D] == NEG).all() and (c6[0, :D] == -1).all() and (s6[1:] == SENT).all()


# ----------------------------------------------------------------------------
# 2. abcd_span_chain_viterbi through ctypes, on synthetic tables
# ----------------------------------------------------------------------------
def chain_call(table, d_min, gap, bonus, trans, init, want_w=True):
    """abcd_span_chain_viterbi on host arrays -> dict of numpy outputs.  The
    table travels with ld_k = K + 3 and log_trans with ld_trans = K + 2 (NaN
    padding); every output holds SENT before the call and carries one guard
    entry (W_out a guard row); the workspace holds 0xFF."""
    from modules import _native as N_
    lib = N_.lib()
    N, D, K = table.shape[0] - 1, table.shape[1], table.shape[2]
    tb = torch.full((N + 1, D, K + 3), NAN, dtype=torch.float64)
    tb[:, :, :K] = torch.from_numpy(table)
    lt = torch.full((K, K + 2), NAN)
    lt[:, :K] = torch.from_numpy(np.asarray(trans, dtype=np.float32))
    tb, lt, li = tb.cuda(), lt.cuda(), torch.from_numpy(np.asarray(init, dtype=np.float32)).cuda()
    g = None if gap is None else torch.from_numpy(np.asarray(gap, dtype=np.float32)).cuda()
    cap = N // d_min
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    ps, ns = torch.full((2,), SENT, **f64), torch.full((2,), int(SENT), **i32)
    on, ln, ct = (torch.full((cap + 1,), int(SENT), **i32) for _ in range(3))
    sv, lk = torch.full((cap + 1,), SENT, **f64), torch.full((cap + 1,), SENT, **f64)
    W = torch.full((N + 2, K), SENT, **f64) if want_w else None
    ws = N_.workspace(lib.abcd_span_chain_workspace_bytes(N, D, K), "cuda")
    ws.fill_(0xFF)
    rc = lib.abcd_span_chain_viterbi(N_.ptr(tb), K + 3, N, D, K, d_min, N_.ptr(g), float(bonus), N_.ptr(lt), K + 2,
                                     N_.ptr(li), N_.ptr(ps), N_.ptr(ns), N_.ptr(on), N_.ptr(ln), N_.ptr(ct),
                                     N_.ptr(sv), N_.ptr(lk), N_.ptr(W), N_.ptr(ws), ws.numel(), N_.stream())
    torch.cuda.synchronize()
    assert rc == 0
    k = int(ns[0])
    assert 0 <= k <= cap
    # guards: the entries past n_segments, the extra entry of every buffer, W_out's extra row
    assert float(ps[1]) == SENT and int(ns[1]) == int(SENT)
    for t in (on, ln, ct):
        assert (t[k:] == int(SENT)).all()
    assert (sv[k:] == SENT).all() and (lk[k:] == SENT).all()
    if want_w:
        assert (W[N + 1] == SENT).all()
    return dict(path_score=float(ps[0]), n=k, onset=on[:k].tolist(), length=ln[:k].tolist(), cat=ct[:k].tolist(),
                score=sv[:k].tolist(), link=lk[:k].tolist(), W=None if W is None else W[:N + 1].cpu().numpy())


def check_chain(table, d_min, gap, bonus, trans, init, tag):
    """One call against the float64 loop: equality in every output, and the
    path score against the sum of its own terms."""
    ref = SX.chain_reference(table, d_min, trans, init, gap, bonus)
    got = chain_call(table, d_min, gap, bonus, trans, init)
    N = table.shape[0] - 1
    assert np.array_equal(got["W"].view(np.int64), ref["W"].view(np.int64)), \
        (tag, np.argwhere(got["W"].view(np.int64) != ref["W"].view(np.int64))[:4])
    assert np.float64(got["path_score"]).view(np.int64) == np.float64(ref["path_score"]).view(np.int64), tag
    assert got["n"] == len(ref["onset"]), tag
    for key in ("onset", "length", "cat", "score", "link"):
        assert got[key] == ref[key], (tag, key)
    if ref["path_score"] == NEG:
        assert got["n"] == 0
        return ref, 0.0
    total, mag = SX.terms_of(got, N, gap, bonus)
    rel = abs(got["path_score"] - total) / mag if mag > 0 else abs(got["path_score"] - total)
    assert rel <= 1e-9, (tag, rel)
    return ref, rel


def _resident(K, D):
    from modules import _native as N_
    res = N_.c_int(-1)
    assert N_.lib().abcd_span_chain_plan(K, D, N_.ctypes.byref(res), None, None) == 0
    return bool(res.value)


@pytest.mark.parametrize("kind", SX.CHAIN_KINDS)
@pytest.mark.parametrize("K", SX.CHAIN_K)
@pytest.mark.parametrize("ND", SX.CHAIN_ND, ids=lambda v: f"n{v[0]}d{v[1]}")
def test_span_chain_viterbi_is_the_float64_loop(ND, K, kind):
    N, D = ND
    assert _resident(K, D) == (K <= 128)            # K = 130 streams log_trans from global memory
    c = SX.chain_inputs(N, D, K, kind)
    reached = segments = 0
    worst = 0.0
    for d_min, gap, bonus, tag in c["calls"]:
        ref, rel = check_chain(c["table"], d_min, gap, bonus, c["trans"], c["init"], (N, D, K, kind, tag))
        reached += ref["path_score"] > NEG
        segments += len(ref["onset"])
        worst = max(worst, rel)
        if kind == "nopath":
            assert len(ref["onset"]) <= 1           # nothing may follow anything
            if gap is None and N > D:
                assert ref["path_score"] == NEG     # one segment cannot cover the recording
            # no initial distribution either: a gap-only path or nothing
            ref0, _ = check_chain(c["table"], d_min, gap, bonus, c["trans"], c["init_none"],
                                  (N, D, K, kind, tag, "noinit"))
            assert ref0["onset"] == [] and (ref0["path_score"] > NEG) == (gap is not None)
    print(f"N={N} D={D} K={K} {kind}: {len(c['calls'])} calls, {reached} reachable, {segments} segments; worst "
          f"|path_score - sum of terms| / sum |terms| {worst:.1e}")
    SX.dump(f"e2e_chain_n{N}d{D}k{K}{kind}", [dict(case=f"n{N}d{D}k{K}{kind}", terms=worst)])
    if kind in ("random", "tied", "gaps", "bonus"):
        assert reached > 0 and segments > 0


@pytest.mark.parametrize("kind", ("random", "tied", "zeros"))
@pytest.mark.parametrize("K", (256, 257, 600))
def test_span_chain_viterbi_at_the_launch_width_threshold(K, kind):
    """K = 256 is the last shape of the 16-wave launch, 257 the first of the
    4-wave one (abcd_span_chain_plan); 600 takes several strides over k."""
    from modules import _native as N_
    thr = N_.c_int(-1)
    assert N_.lib().abcd_span_chain_plan(K, 5, None, N_.ctypes.byref(thr), None) == 0
    assert thr.value == (1024 if K <= 256 else 256)
    c = SX.chain_inputs(33, 5, K, kind)
    for d_min, gap, bonus, tag in c["calls"]:
        check_chain(c["table"], d_min, gap, bonus, c["trans"], c["init"], (K, kind, tag))


def test_span_chain_viterbi_without_w_out_and_two_calls():
    c = SX.chain_inputs(70, 17, 130, "random")
    d_min, gap, bonus, _ = c["calls"][1]
    a = chain_call(c["table"], d_min, gap, bonus, c["trans"], c["init"], want_w=True)
    b = chain_call(c["table"], d_min, gap, bonus, c["trans"], c["init"], want_w=False)
    a2 = chain_call(c["table"], d_min, gap, bonus, c["trans"], c["init"], want_w=True)
    assert b["W"] is None and np.array_equal(a["W"].view(np.int64), a2["W"].view(np.int64))
    for key in ("path_score", "n", "onset", "length", "cat", "score", "link"):
        assert a[key] == b[key] == a2[key], key


def test_chain_ops_are_forward_only_and_check_shapes():
    from modules import ops
    c = SX.chain_inputs(33, 5, 33, "random")
    tb = torch.from_numpy(c["table"]).cuda()
    lt, li = torch.from_numpy(c["trans"]).cuda(), torch.from_numpy(c["init"]).cuda()
    out = ops.span_chain_viterbi(tb, 1, None, 0.0, lt, li, True)
    ref = SX.chain_reference(c["table"], 1, c["trans"], c["init"])
    k = int(out[1])
    assert float(out[0]) == ref["path_score"] and out[4][:k].tolist() == ref["cat"]
    assert np.array_equal(out[7].cpu().numpy().view(np.int64), ref["W"].view(np.int64))
    assert [tuple(t.shape) for t in out[2:]] == [(33,)] * 5 + [(34, 33)]
    N0 = ops.span_chain_viterbi(tb[:1], 1, None, 0.0, lt, li, True)    # N = 0
    assert float(N0[0]) == 0.0 and int(N0[1]) == 0 and (N0[7] == NEG).all()
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.span_chain_viterbi(tb.clone().requires_grad_(True), 1, None, 0.0, lt, li, False)
    with pytest.raises(ValueError):
        ops.span_chain_viterbi(tb, 6, None, 0.0, lt, li, False)
    with pytest.raises(ValueError):
        ops.span_chain_viterbi(tb, 1, None, 0.0, lt[:, :5], li, False)
    with pytest.raises(ValueError):
        ops.span_chain_viterbi(tb, 1, torch.zeros(5).cuda(), 0.0, lt, li, False)
    with pytest.raises(ValueError):
        ops.span_chain_viterbi(tb[:, :, 0], 1, None, 0.0, lt, li, False)


def test_planted_alternation_through_the_operator():
    from modules import ops
    c = SX.planted_alternation()
    tb = torch.from_numpy(c["table"]).cuda()
    score, cat = SX.context_free(c["table"], c["lw"])
    free = ops.span_viterbi(torch.from_numpy(score).cuda(), torch.from_numpy(cat.astype(np.int32)).cuda(), 1, None,
                            0.0, False)
    k = int(free[1])
    assert k == SX.ALT_SEGMENTS and free[3][:k].tolist() == [SX.ALT_L] * k and free[4][:k].tolist() == [0] * k
    out = ops.span_chain_viterbi(tb, 1, None, 0.0, torch.from_numpy(c["trans"]).cuda(),
                                 torch.from_numpy(c["init"]).cuda(), False)
    k = int(out[1])
    assert k == SX.ALT_SEGMENTS and out[2][:k].tolist() == free[2][:k].tolist()
    assert out[3][:k].tolist() == [SX.ALT_L] * k
    assert out[4][:k].tolist() == [i % 2 for i in range(k)]             # the alternation
    ref = SX.chain_reference(c["table"], 1, c["trans"], c["init"])
    assert float(out[0]) == ref["path_score"] and out[6][:k].tolist() == ref["link"]


# ----------------------------------------------------------------------------
# 3. segment_frames(transitions=...) on the small models
# ----------------------------------------------------------------------------
def _small_recording(name):
    """(decoder, prototypes, frames, K, D): the recording of test_gpu_span's
    small-model test, the generated mean frames of a few categories."""
    r = S.small_reference(name)
    _, samp, dec = _small_modules(r)
    K, D = samp.num_categories, 12
    feats = samp.codebook.detach().t().contiguous()
    spk = None
    if dec.embed_speaker is not None:
        spk = torch.full((K,), int(r["batch"]["speakers"][0]), dtype=torch.int64, device="cuda")
    protos = dec.prototypes(feats, D + 2, speaker=spk)
    pick = [1, K - 1, 0, K // 2, 1, K - 1, 0, 1]
    sp = None if spk is None else spk[:len(pick)]
    packed, lengths, _, _ = dec.generate(feats[pick], D, speaker=sp, mean=True, stop_prob=0.5, min_length=2)
    padded, lens = torch.nn.utils.rnn.pad_packed_sequence(packed, batch_first=True)
    padded, lens = padded[packed.unsorted_indices], lens[packed.unsorted_indices.cpu()]
    frames = torch.cat([padded[i, :int(n)] for i, n in enumerate(lens)])
    return dec, protos, frames, K, D


@pytest.mark.parametrize("name", list(S.E2E_SMALL))
def test_context_free_chain_reduces_to_segment_frames(name):
    from modules import segmentation
    from modules.sequence import TransitionModel
    dec, protos, frames, K, D = _small_recording(name)
    lw = torch.linspace(-1.0, 1.0, K).cuda()
    model = TransitionModel.from_log_weight(lw)
    rels = []
    tiled = segmentation.segment_frames(dec, protos, frames, D, log_weight=model.log_init)
    per_frame = float(tiled["path_score"]) / frames.shape[0]   # a gap at the average frame's score: some frames uncovered
    const = torch.full((frames.shape[0],), per_frame, device="cuda")
    for gap, bonus, d_min in ((None, 0.0, 1), (None, -3.0, 2), (const, 0.0, 1), (const, -3.0, 2)):
        free = segmentation.segment_frames(dec, protos, frames, D, min_length=d_min, gap=gap, seg_bonus=bonus,
                                           log_weight=model.log_init)       # log_softmax(lw), as the chain holds it
        out = segmentation.segment_frames(dec, protos, frames, D, min_length=d_min, gap=gap, seg_bonus=bonus,
                                          log_weight=model.log_init, transitions=model)
        for key in ("onset", "length", "category"):
            assert out[key].tolist() == free[key].tolist(), (name, key)
        rel = abs(float(out["path_score"]) - float(free["path_score"])) / abs(float(free["path_score"]))
        rels.append(rel)
        assert rel <= 1e-9
        assert out["context_free_category"].tolist() == free["category"].tolist()
        assert out["link"].dtype == torch.float64
        assert out["link"].tolist() == [float(model.log_init[k]) for k in out["category"].tolist()]
        # score + link is the context-free segment score
        assert torch.allclose(out["score"] + out["link"], free["score"], rtol=1e-12, atol=0.0)
    print(f"{name}: context-free chain against segment_frames: path score relative difference {max(rels):.1e}")
    SX.dump(f"e2e_reduction_{name}", [dict(case=name, reduction=max(rels))])
    with pytest.raises(ValueError, match="posteriors"):
        segmentation.segment_frames(dec, protos, frames, D, transitions=model, posteriors=True)
    with pytest.raises(ValueError):
        segmentation.segment_frames(dec, protos, frames, D, transitions=TransitionModel(K + 1).cuda())
    # the method's table is the operator's; a shorter rectangle is refused
    tb, ss, cc = dec.span_table(protos, frames, D, want_best=True)
    ss0, cc0 = dec.span_scores(protos, frames, D)
    assert tuple(tb.shape) == (frames.shape[0] + 1, D, K) and tb.dtype == torch.float64
    assert torch.equal(_bits(ss), _bits(ss0)) and torch.equal(cc, cc0)
    assert dec.span_table(protos, frames, D)[1] is None
    with pytest.raises(ValueError):
        dec.span_table(protos, frames, D + 3)


def test_forbidden_bigram_is_avoided():
    """A matrix that forbids the context-free path's most frequent bigram
    yields a path without it, whose context-free score is no higher than the
    context-free optimum."""
    from modules import segmentation
    from modules.sequence import TransitionModel
    dec, protos, frames, K, D = _small_recording(list(S.E2E_SMALL)[0])
    lw = torch.log_softmax(torch.linspace(-1.0, 1.0, K), 0).cuda()
    free = segmentation.segment_frames(dec, protos, frames, D, log_weight=lw)
    cats = free["category"].tolist()
    assert len(cats) >= 2
    bigrams = list(zip(cats[:-1], cats[1:]))
    a, b = max(sorted(set(bigrams)), key=bigrams.count)
    model = TransitionModel.from_log_weight(lw)
    model.log_trans[a, b] = NEG
    out = segmentation.segment_frames(dec, protos, frames, D, log_weight=lw, transitions=model)
    got = out["category"].tolist()
    assert float(out["path_score"]) > NEG and len(got) >= 1
    assert (a, b) not in list(zip(got[:-1], got[1:]))
    # the same cut scored context-free: every segment at its own category under lw
    cf = float((out["score"] + lw.double()[out["category"]]).sum())
    print(f"forbidden bigram {(a, b)}: context-free path {cats} -> {got}; context-free score {cf:.4f} against the "
          f"optimum {float(free['path_score']):.4f}")
    assert cf <= float(free["path_score"]) + 1e-9 * abs(float(free["path_score"]))


def test_table_beyond_the_index_limit_is_refused():
    from modules import _native as N_, ops
    n, D, P, F = 70000, 300, 128, 4                  # (N + 1) D K >= 2^31 while (N + 1) D < 2^31
    T = D
    with pytest.raises(N_.HipError, match="index limit"):
        ops.span_table(torch.zeros(n, F).cuda(), torch.zeros(T * P, F).cuda(), torch.zeros(T * P, F).cuda(),
                       torch.zeros(T * P).cuda(), None, P, D, False)


# ----------------------------------------------------------------------------
# 4. segment.py --transitions on the toy data
# ----------------------------------------------------------------------------
def test_segment_cli_with_transitions(tmp_path):
    import segment
    K = 16
    base = [CKPT, TOY, ANN, "1.0", "--max_length", "60", "--min_length", "3"]
    # without the flag: the bytes of the unchanged writer on the unchanged function's result
    out = os.path.join(str(tmp_path), "s", "segmented.csv")
    assert segment.main(base + ["-S", out]) == out
    seg = segment.Segmenter(CKPT, device="cuda")
    wav = pd.read_csv(ANN)["input_path"][0]
    fs, wave = segment.read_wave(TOY, wav)
    a = segment.get_parameters(base)
    frame, hop = segment.cli.frame_hop(a, fs)
    frames = segment.cli.log_spectrum(a, frame, hop)(torch.from_numpy(wave)).to(seg.device)
    lw = seg.log_weight(a.prior, len(pd.read_csv(ANN)))
    d_min = max(3, segment.min_loadable_length(frame, hop, True))
    got = seg.segment_recording(frames, 60, min_length=d_min, log_weight=lw)
    first = pd.read_csv(ANN).iloc[0]
    rows = segment.segment_rows(wav, got["onset"].tolist(), got["length"].tolist(), got["category"].tolist(),
                                got["score"].tolist(), fs, frame, hop, True, len(wave), data_type=first["data_type"],
                                speaker=first["speaker"])
    want = os.path.join(str(tmp_path), "w", "segmented.csv")
    os.makedirs(os.path.dirname(want))
    pd.DataFrame(rows, columns=list(segment.COLUMNS)).to_csv(want, index=False)
    with open(out, "rb") as f, open(want, "rb") as g:
        assert f.read() == g.read()
    df = pd.read_csv(out)
    # a transitions.csv as sequence.py writes it: a sticky chain
    p = np.full((K, K), 0.2 / (K - 1))
    np.fill_diagonal(p, 0.8)
    ft, tt = np.divmod(np.arange(K * K), K)
    tcsv = os.path.join(str(tmp_path), "transitions.csv")
    pd.DataFrame({"from_ix": ft, "to_ix": tt, "probability": p.reshape(-1), "expected_count": 0.0}).to_csv(
        tcsv, index=False)
    out_t = os.path.join(str(tmp_path), "t", "segmented.csv")
    assert segment.main(base + ["-S", out_t, "--transitions", tcsv]) == out_t
    dt = pd.read_csv(out_t)
    assert list(dt.columns) == list(segment.COLUMNS) + list(segment.SYNTAX_COLUMNS)
    assert len(dt) >= 1 and int(dt["length"].sum()) == int(df["length"].sum())      # the segments tile the recording
    assert ((dt["category_ix"] >= 0) & (dt["category_ix"] < K)).all()
    assert ((dt["context_free_category_ix"] >= 0) & (dt["context_free_category_ix"] < K)).all()
    assert (dt["changed"] == (dt["category_ix"] != dt["context_free_category_ix"]).astype(int)).all()
    cats = dt["category_ix"].tolist()
    li = torch.log_softmax(lw.double(), 0).float().double().cpu().numpy()
    want_link = [li[cats[0]]] + [float(np.log(p[i, j]).astype(np.float32)) for i, j in zip(cats[:-1], cats[1:])]
    assert np.allclose(dt["transition_score"].to_numpy(), want_link, rtol=1e-6, atol=0.0)
    print(f"segment.py --transitions: {len(dt)} segments ({len(df)} context-free), {int(dt['changed'].sum())} changed")
    # refitting writes the matrix in transitions.csv's columns; --posteriors is refused
    out_r = os.path.join(str(tmp_path), "r", "segmented.csv")
    tout = os.path.join(str(tmp_path), "r", "transitions.csv")
    segment.main(base + ["-S", out_r, "--transitions", tcsv, "--refit_transitions", "1", "--transitions_out", tout])
    tr = pd.read_csv(tout)
    assert list(tr.columns) == list(segment.TRANSITION_COLUMNS) and len(tr) == K * K
    assert np.allclose(tr["probability"].to_numpy().reshape(K, K).sum(1), 1.0, atol=1e-5)
    assert tr["expected_count"].sum() == len(dt) - 1                                # the first pass is out_t's cut
    with pytest.raises(SystemExit):
        segment.main(base + ["-S", out_r, "--transitions", tcsv, "--posteriors"])
