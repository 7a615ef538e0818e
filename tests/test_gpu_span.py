"""Segmentation on the GPU: ``abcd_span_scores`` and ``abcd_span_viterbi``
through the C ABI and the operators, ``RNN_Variational_Decoder.span_scores`` /
``modules.segmentation.segment_frames`` end to end and the ``segment.py`` CLI,
against the float64 references of ``span_cases.py``.

Bars (``span_cases.py``): every ``span_score`` within 1e-4 of the unit ``A`` of
the entry that attains the float64 maximum; the chosen category's float64 score
within 2e-4 of its unit of that maximum (``classify.py``'s rule); entries that
cannot exist exactly -inf / -1; at P = 1 within ``cross_bar(F) A`` of
``ops.pairwise_nll`` on the cut-out spans; the dynamic programme EQUAL to the
float64 loop in every output.  Every observed figure is printed (``-rA``) and
kept with ``ABCD_PARITY_DUMP`` (profiles/span_errors.json)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import pairwise_cases as PW
import score_cases as S
import span_cases as SP
from test_gpu_pairwise import _rect
from test_gpu_score import ANN, CKPT, TOY, _rows, _small_modules

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")
SENT = -7.0  # what the outputs hold before a call


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


# ----------------------------------------------------------------------------
# 1. abcd_span_scores through ctypes
# ----------------------------------------------------------------------------
def span_buffers(c, ld, x=None, lw="own"):
    """The device buffers of a case with row stride ld: padding columns, tail
    rows and the rectangle's steps >= D are NaN."""
    D = c["D"]
    return dict(x=_rows(c["x"] if x is None else x, ld), ldx=ld, mu=_rect(c["mu"][:D], ld, extra=SP.T_EXTRA), ldm=ld,
                lv=_rect(c["lv"][:D], ld, extra=SP.T_EXTRA), ldl=ld, o=_rect(c["o"][:D], 1, extra=SP.T_EXTRA),
                lw=(c["lw"].cuda() if isinstance(lw, str) else lw))


def span_call(c, x, ldx, mu, ldm, lv, ldl, o, lw, n=None, pad=1):
    """abcd_span_scores -> (rc, score, cat): (N + 2) x (D + pad) buffers holding
    SENT before the call; the workspace holds NaN."""
    from modules import _native as N
    lib = N.lib()
    n = c["N"] if n is None else n
    D, P, F = c["D"], c["P"], c["F"]
    score = torch.full((n + 2, D + pad), SENT, dtype=torch.float64, device="cuda")
    cat = torch.full((n + 2, D + pad), int(SENT), dtype=torch.int32, device="cuda")
    ws = N.workspace(lib.abcd_span_scores_workspace_bytes(n, D, P), "cuda")
    ws.fill_(0xFF)
    rc = lib.abcd_span_scores(N.ptr(x), ldx, n, F, P, D, D + SP.T_EXTRA, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(o),
                              N.ptr(lw), N.ptr(score), N.ptr(cat), D + pad, N.ptr(ws), ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, score, cat


def _all_spans_pairwise(c):
    """ops.pairwise_nll on every cut-out span of a P = 1 case as one packed
    batch with one-hot end targets: {(s, d): lw - em - off} in float64."""
    from modules import ops
    N, D, F = c["N"], c["D"], c["F"]
    spans = sorted(((d, s) for s in range(N) for d in range(1, min(D, N - s) + 1)), key=lambda v: -v[0])
    starts = np.array([s for _, s in spans])
    lens = np.array([d for d, _ in spans])
    rows, y, bs = [], [], []
    for t in range(int(lens.max())):
        live = lens > t
        rows.append(starts[live] + t)
        y.append((lens[live] == t + 1).astype(np.float32))
        bs.append(int(live.sum()))
    gt = c["x"][torch.from_numpy(np.concatenate(rows))].cuda()
    yy = torch.from_numpy(np.concatenate(y)).cuda()
    T = D + SP.T_EXTRA
    em, off = ops.pairwise_nll(gt, torch.tensor(bs), yy, c["mu"].reshape(T, F).cuda(), c["lv"].reshape(T, F).cuda(),
                               c["o"].reshape(T).cuda(), 1, F)
    s = float(c["lw"][0]) - em[:, 0].double().cpu().numpy() - off[:, 0].double().cpu().numpy()
    return {(int(st), int(d)): float(v) for st, d, v in zip(starts, lens, s)}


@pytest.mark.parametrize("F", SP.ABI_F)
@pytest.mark.parametrize("P", SP.ABI_P)
@pytest.mark.parametrize("ND", SP.abi_shapes(), ids=lambda v: f"n{v[0]}d{v[1]}")
def test_span_scores_abi(ND, P, F):
    N, D = ND
    c = SP.abi_inputs(N, D, P, F)
    ref = c["ref"]
    valid = np.zeros((N + 1, D), dtype=bool)
    for e in range(1, N + 1):
        valid[e, :min(D, e)] = True
    ee, dd = np.nonzero(valid)
    S_at = ref["S"][ee - dd - 1]                    # (entries, P, D) -> each entry's P scores
    S_at = S_at[np.arange(len(ee)), :, dd]
    A_at = ref["A"][ee - dd - 1][np.arange(len(ee)), :, dd]
    rows = []
    for ld in (F, SP.PAD_LD):
        b = span_buffers(c, ld)
        rc, score, cat = span_call(c, **b)
        assert rc == 0
        assert (score[:, D:] == SENT).all() and (score[N + 1:] == SENT).all()      # nothing outside N + 1 x D
        assert (cat[:, D:] == int(SENT)).all() and (cat[N + 1:] == int(SENT)).all()
        sc, ct = score[:N + 1, :D].cpu().numpy(), cat[:N + 1, :D].cpu().numpy()
        assert (sc[~valid] == NEG).all() and (ct[~valid] == -1).all()               # exactly -inf / -1
        got, k = sc[ee, dd], ct[ee, dd]
        assert ((k >= 0) & (k < P)).all()
        best = S_at.argmax(1)
        ix = np.arange(len(ee))
        e_score = np.abs(got - S_at[ix, best]) / A_at[ix, best]
        e_cat = (S_at[ix, best] - S_at[ix, k]) / A_at[ix, k]
        line = f"N={N} D={D} P={P} F={F} ld={ld}: worst |span_score - max S| / A {e_score.max():.2e}; chosen " \
               f"category under the float64 maximum by {e_cat.max():.2e} of its unit"
        row = dict(N=N, D=D, P=P, F=F, ld=ld, score=float(e_score.max()), category=float(e_cat.max()))
        assert np.isfinite(e_score).all()
        if P == 1:                                  # against the pairwise kernel on every cut-out span
            pw = _all_spans_pairwise(c)
            e_x = max(abs(sc[s + d, d - 1] - v) / ref["A"][s, 0, d - 1] for (s, d), v in pw.items())
            line += f"; |span_score - pairwise| / A {e_x:.2e} (bar {PW.cross_bar(F):.2e})"
            row["vs_pairwise"] = float(e_x)
        print(line)
        rows.append(row)
        assert e_score.max() <= SP.BAR
        assert e_cat.max() <= 2 * SP.BAR
        if P == 1:
            assert len(pw) == len(ee) and e_x <= PW.cross_bar(F)
        # a second call: bit for bit; an exact-width output holds the same bits
        rc, score2, cat2 = span_call(c, **b)
        assert rc == 0 and torch.equal(_bits(score), _bits(score2)) and torch.equal(cat, cat2)
        rc, score3, cat3 = span_call(c, **b, pad=0)
        assert rc == 0 and torch.equal(_bits(score3[:N + 1]), _bits(score[:N + 1, :D])) and \
            torch.equal(cat3[:N + 1], cat[:N + 1, :D])
    SP.dump(f"abi_n{N}d{D}p{P}f{F}", rows)


def test_span_scores_nan_weights_and_shift():
    N, D, P, F = 70, 17, 33, 65
    c = SP.abi_inputs(N, D, P, F)
    b = span_buffers(c, SP.PAD_LD)
    rc, score, cat = span_call(c, **b)
    assert rc == 0
    sc, ct = score[:N + 1, :D], cat[:N + 1, :D]
    # one NaN frame poisons exactly the spans that contain it
    n0 = 40
    x = c["x"].clone()
    x[n0, F // 2] = NAN
    rc, s2, c2 = span_call(c, **span_buffers(c, SP.PAD_LD, x=x))
    assert rc == 0
    e = torch.arange(N + 1)[:, None]
    d = torch.arange(1, D + 1)[None, :]
    hit = ((e - d <= n0) & (n0 < e) & (d <= e)).cuda()
    assert (s2[:N + 1, :D][hit] == NEG).all() and (c2[:N + 1, :D][hit] == -1).all()
    assert torch.equal(_bits(s2[:N + 1, :D][~hit]), _bits(sc[~hit])) and torch.equal(c2[:N + 1, :D][~hit], ct[~hit])
    # a -inf (or NaN) weight removes its category and leaves every other entry's bits
    for bad in (NEG, NAN):
        k = int(torch.mode(ct[ct >= 0].flatten()).values)
        lw = c["lw"].clone()
        lw[k] = bad
        rc, s3, c3 = span_call(c, **span_buffers(c, SP.PAD_LD, lw=lw.cuda()))
        assert rc == 0 and not (c3[:N + 1, :D] == k).any()
        keep = ct != k
        assert (ct == k).any() and torch.equal(_bits(s3[:N + 1, :D][keep]), _bits(sc[keep]))
        assert torch.equal(c3[:N + 1, :D][keep], ct[keep])
        want = SP.span_reference(c["x"], c["mu"], c["lv"], c["o"], lw, D)
        assert ((c3[:N + 1, :D] >= 0).cpu().numpy() == (want["cat"] >= 0)).all()
    # a NULL weight vector counts as zeros
    rc, s4, c4 = span_call(c, **span_buffers(c, SP.PAD_LD, lw=None))
    rc5, s5, c5 = span_call(c, **span_buffers(c, SP.PAD_LD, lw=torch.zeros(P).cuda()))
    assert rc == 0 and rc5 == 0 and torch.equal(_bits(s4), _bits(s5)) and torch.equal(c4, c5)
    # 5 frames prepended shift the bits unchanged
    pre = torch.randn(5, F, generator=torch.Generator().manual_seed(5))
    rc, s6, c6 = span_call(c, **span_buffers(c, SP.PAD_LD, x=torch.cat([pre, c["x"]])), n=N + 5)
    assert rc == 0
    own = (d <= e).cuda()[1:]                       # spans that start at or after the old frame 0
    assert torch.equal(_bits(s6[6:N + 6, :D][own]), _bits(sc[1:][own]))
    assert torch.equal(c6[6:N + 6, :D][own], ct[1:][own])
    # N = 0 writes row 0 only
    rc, s7, c7 = span_call(c, **b, n=0)
    assert rc == 0 and (s7[0, :D] == NEG).all() and (c7[0, :D] == -1).all() and (s7[1:] == SENT).all()


# ----------------------------------------------------------------------------
# 2. abcd_span_viterbi
# ----------------------------------------------------------------------------
def _check_viterbi(ss, sc, d_min, gap, bonus, tag):
    """ops.span_viterbi on a host table against the float64 loop: equality."""
    from modules import ops
    N = ss.shape[0] - 1
    ref = SP.viterbi_reference(ss, sc, d_min, gap, bonus)
    g = None if gap is None else torch.from_numpy(np.asarray(gap, dtype=np.float32)).cuda()
    out = ops.span_viterbi(torch.from_numpy(ss).cuda(), torch.from_numpy(np.asarray(sc, dtype=np.int32)).cuda(), d_min,
                           g, float(bonus), True)
    ps, ns, onset, length, cat, score, V = (t.cpu().numpy() for t in out)
    k = int(ns)
    assert onset.shape == (N // d_min,), tag
    assert np.array_equal(V, ref["V"]), (tag, np.nonzero(V != ref["V"])[0][:4])
    assert float(ps) == ref["path_score"], tag
    assert k == len(ref["onset"]), tag
    assert onset[:k].tolist() == ref["onset"] and length[:k].tolist() == ref["length"], tag
    assert cat[:k].tolist() == ref["cat"] and score[:k].tolist() == ref["score"], tag
    return ref


VIT_N = (0, 1, 2, 33, 300)
VIT_D = (1, 5, 64, 65, 256, 257, 300)   # 256 / 257: the widest single-wave launch and the first four-wave one


@pytest.mark.parametrize("D", VIT_D)
@pytest.mark.parametrize("N", VIT_N)
def test_span_viterbi_is_the_float64_loop(N, D):
    reached = tied_gap = 0
    for kind in ("random", "tied", "holes"):
        t = SP.table_inputs(N, D, kind)
        for d_min in sorted({1, min(3, D), D}):
            for gname, gap in (("null", None), ("const", np.full(N, -2.0, dtype=np.float32)), ("drawn", t["gap"])):
                for bonus in ((0.0, -1.0) if kind != "tied" else (0.0, -1.0, 1.0)):
                    ref = _check_viterbi(t["score"], t["cat"], d_min, gap, bonus, (N, D, kind, d_min, gname, bonus))
                    reached += ref["path_score"] > NEG
    print(f"N={N} D={D}: {reached} reachable configurations")
    assert reached > 0


@pytest.mark.parametrize("with_gap", (False, True), ids=("nogap", "gap"))
@pytest.mark.parametrize("name", list(SP.TAIL_CASES))
def test_span_viterbi_past_the_register_candidates(name, with_gap):
    """Candidate lengths above 1024 come from the step's loop, not from the
    four registers per thread (span_cases.TAIL_CASES; the conditions on the
    reference are asserted in test_span_cpu.py): equality with the float64 loop."""
    t = SP.tail_inputs(name)
    ref = _check_viterbi(t["score"], t["cat"], t["d_min"], t["gap"] if with_gap else None, 0.0, (name, with_gap))
    assert ref["path_score"] > NEG and max(ref["length"]) >= SP.TAIL_FROM


def test_span_viterbi_on_the_span_kernel_output():
    """The programme on abcd_span_scores' own (row-strided) output through the C
    ABI, with and without V_out: equal to the loop on the same table."""
    from modules import _native as N_
    lib = N_.lib()
    for N, D, P, F in ((70, 37, 17, 65), (33, 37, 33, 129), (31, 5, 1, 1)):
        c = SP.abi_inputs(N, D, P, F)
        rc, score, cat = span_call(c, **span_buffers(c, SP.PAD_LD))
        assert rc == 0
        ss, sc = score[:N + 1, :D].cpu().numpy(), cat[:N + 1, :D].cpu().numpy()
        gap = torch.full((N,), float(np.median(ss[np.isfinite(ss)])) / 4.0)
        for d_min, g, bonus in ((1, None, 0.0), (3, None, -5.0), (1, gap, 0.0), (2, gap, -50.0)):
            if d_min > D:
                continue
            ref = SP.viterbi_reference(ss, sc, d_min, None if g is None else g.numpy(), bonus)
            cap = N // d_min
            for want_v in (True, False):
                ps = torch.full((1,), SENT, dtype=torch.float64, device="cuda")
                ns = torch.full((1,), int(SENT), dtype=torch.int32, device="cuda")
                on, ln, ct = (torch.full((cap + 1,), int(SENT), dtype=torch.int32, device="cuda") for _ in range(3))
                sv = torch.full((cap + 1,), SENT, dtype=torch.float64, device="cuda")
                V = torch.full((N + 2,), SENT, dtype=torch.float64, device="cuda") if want_v else None
                ws = N_.workspace(lib.abcd_span_viterbi_workspace_bytes(N, D), "cuda")
                ws.fill_(0xFF)
                gd = None if g is None else g.cuda()
                rc = lib.abcd_span_viterbi(N_.ptr(score), N_.ptr(cat), D + 1, N, D, d_min, N_.ptr(gd), bonus,
                                           N_.ptr(ps), N_.ptr(ns), N_.ptr(on), N_.ptr(ln), N_.ptr(ct), N_.ptr(sv),
                                           N_.ptr(V), N_.ptr(ws), ws.numel(), N_.stream())
                torch.cuda.synchronize()
                assert rc == 0
                k = int(ns)
                assert float(ps) == ref["path_score"] and k == len(ref["onset"])
                assert on[:k].tolist() == ref["onset"] and ln[:k].tolist() == ref["length"]
                assert ct[:k].tolist() == ref["cat"] and sv[:k].tolist() == ref["score"]
                assert (on[k:] == int(SENT)).all() and (sv[k:] == SENT).all()          # nothing past n_segments
                if want_v:
                    assert np.array_equal(V[:N + 1].cpu().numpy(), ref["V"]) and float(V[N + 1]) == SENT
            if g is None:
                assert sum(ref["length"]) == N


def test_span_ops_are_forward_only():
    from modules import ops
    c = SP.abi_inputs(31, 5, 17, 65)
    T = c["D"] + SP.T_EXTRA
    a = (c["x"].cuda(), c["mu"].reshape(T * 17, 65).cuda(), c["lv"].reshape(T * 17, 65).cuda(),
         c["o"].reshape(-1).cuda(), c["lw"].cuda(), 17, 5)
    ss, sc = ops.span_scores(*a)
    assert np.abs(ss.cpu().numpy()[1:, 0] - c["ref"]["score"][1:, 0]).max() < 1.0
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.span_scores(a[0].clone().requires_grad_(True), *a[1:])
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.span_viterbi(ss.clone().requires_grad_(True), sc, 1, None, 0.0, False)
    with pytest.raises(ValueError):
        ops.span_scores(a[0], a[1], a[2], a[3], a[4], 17, T + 1)       # a rectangle shorter than D
    with pytest.raises(ValueError):
        ops.span_scores(a[0], a[1], a[2], a[3], a[4][:5], 17, 5)
    with pytest.raises(ValueError):
        ops.span_viterbi(ss, sc, 6, None, 0.0, False)
    with pytest.raises(ValueError):
        ops.span_viterbi(ss, sc[:, :4], 1, None, 0.0, False)
    with pytest.raises(ValueError):
        ops.span_viterbi(ss, sc, 1, torch.zeros(5).cuda(), 0.0, False)


# ----------------------------------------------------------------------------
# 3. the planted recording through segment_frames
# ----------------------------------------------------------------------------
def test_planted_recording_through_segment_frames():
    from modules import model as M, segmentation
    c = SP.planted()
    dec = M.RNN_Variational_Decoder(SP.PLANT_F, 32, 32, 32).cuda().eval()
    protos = tuple(c[k].cuda() for k in ("mu", "lv", "o"))
    gap = torch.from_numpy(c["gap"]).cuda()
    for bonus in (0.0, -2.0):
        out = segmentation.segment_frames(dec, protos, c["x"].cuda(), c["D"], log_weight=c["lw"].cuda(), gap=gap,
                                          seg_bonus=bonus)
        got = list(zip(out["onset"].tolist(), out["length"].tolist(), out["category"].tolist()))
        assert got == c["truth"]
        covered = np.zeros(c["N"], dtype=bool)
        for s, d, _ in got:
            covered[s:s + d] = True
        total = float(out["score"].sum()) + float(c["gap"].astype(np.float64)[~covered].sum()) + bonus * len(got)
        rel = abs(float(out["path_score"]) - total) / abs(total)
        print(f"planted, bonus {bonus}: path_score {float(out['path_score']):.6f} against the sum of its parts: "
              f"{rel:.1e}")
        assert rel <= 1e-9
        ref = SP.span_reference(c["x"], c["mu"], c["lv"], c["o"], c["lw"], c["D"])
        for (s, d, k), v in zip(got, out["score"].tolist()):
            assert abs(v - ref["S"][s, k, d - 1]) <= SP.BAR * ref["A"][s, k, d - 1]
    # the same recording's own gap model, fitted from the frames the truth leaves uncovered
    mu, lv = segmentation.fit_gap_model(c["x"].cuda(), torch.from_numpy(covered))
    out = segmentation.segment_frames(dec, protos, c["x"].cuda(), c["D"], log_weight=c["lw"].cuda(),
                                      gap=segmentation.gap_scores(c["x"].cuda(), mu, lv))
    assert list(zip(out["onset"].tolist(), out["length"].tolist(), out["category"].tolist())) == c["truth"]
    with pytest.raises(ValueError):
        segmentation.segment_frames(dec, protos, c["x"].cuda(), c["D"], min_length=c["D"] + 1)


# ----------------------------------------------------------------------------
# 4. the modules on the small models
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.E2E_SMALL))
def test_segment_frames_on_small_models(name):
    from modules import segmentation
    r = S.small_reference(name)
    _, samp, dec = _small_modules(r)
    K, D = samp.num_categories, 12
    F = dec.rnn_cell.cell.input_size
    feats = samp.codebook.detach().t().contiguous()
    spk_ix = None
    if dec.embed_speaker is not None:
        spk_ix = int(r["batch"]["speakers"][0])
    spk = None if spk_ix is None else torch.full((K,), spk_ix, dtype=torch.int64, device="cuda")
    protos = dec.prototypes(feats, D + 2, speaker=spk)
    lw = torch.log_softmax(torch.linspace(-1.0, 1.0, K), 0).cuda()
    # a recording: the generated mean frames of a few categories, one after another
    pick = [1, K - 1, 0, K // 2, 1]
    sp = None if spk is None else spk[:len(pick)]
    packed, lengths, _, _ = dec.generate(feats[pick], D, speaker=sp, mean=True, stop_prob=0.5, min_length=2)
    padded, lens = torch.nn.utils.rnn.pad_packed_sequence(packed, batch_first=True)
    padded, lens = padded[packed.unsorted_indices], lens[packed.unsorted_indices.cpu()]
    assert lens.tolist() == lengths.tolist()
    frames = torch.cat([padded[i, :int(n)] for i, n in enumerate(lens)])
    N = int(frames.shape[0])
    out = segmentation.segment_frames(dec, protos, frames, D, log_weight=lw)
    k = len(out["onset"])
    on, ln, ct, sc = (out[x].tolist() for x in ("onset", "length", "category", "score"))
    assert k >= 1 and on[0] == 0 and sum(ln) == N and all(on[i] + ln[i] == on[i + 1] for i in range(k - 1))
    # the float64 oracle's prototypes, scores and path
    mu, lv, o = PW.oracle_prototypes(r["P"], r["ocfg"], list(range(K)), None if spk_ix is None else [spk_ix] * K, D)
    ref = SP.span_reference(frames.cpu(), mu.numpy(), lv.numpy(), o.numpy(), lw.cpu(), D)
    path = SP.viterbi_reference(ref["score"], ref["cat"], 1, None, 0.0)
    sum_A = sum(ref["A"][s, c, d - 1] for s, d, c in zip(path["onset"], path["length"], path["cat"]))
    under = path["path_score"] - float(out["path_score"])
    print(f"{name}: N = {N}, generated lengths {lens.tolist()}, segments {list(zip(on, ln, ct))}; oracle path "
          f"{list(zip(path['onset'], path['length'], path['cat']))}; path_score under the oracle's by "
          f"{under / sum_A:.2e} of sum A")
    assert under <= SP.BAR * sum_A
    # every segment's score is what score_against gives for that cut with a one-hot end
    worst = 0.0
    for s, d, c, v in zip(on, ln, ct, sc):
        y = torch.zeros(d)
        y[-1] = 1.0
        em, off, _ = dec.score_against(protos, [1] * d, frames[s:s + d], y.cuda())
        want = float(lw[c].double()) - float(em[0, c].double()) - float(off[0, c].double())
        e = abs(v - want) / ref["A"][s, c, d - 1]
        worst = max(worst, e)
        assert e <= 2 * PW.cross_bar(F), (s, d, c, e)
    print(f"{name}: worst |score - (lw - em - off of score_against)| / A {worst:.2e} (bar {2 * PW.cross_bar(F):.2e})")
    SP.dump(f"e2e_{name}", [dict(case=name, under_oracle=float(under / sum_A), vs_score_against=worst)])
    # span_scores: the method's table is the operator's; a shorter rectangle is refused
    ss, cc = dec.span_scores(protos, frames, D, log_weight=lw)
    assert tuple(ss.shape) == (N + 1, D) and ss.dtype == torch.float64 and cc.dtype == torch.int32
    with pytest.raises(ValueError):
        dec.span_scores(protos, frames, D + 3, log_weight=lw)


# ----------------------------------------------------------------------------
# 5. segment.py on the toy data with the reference's small checkpoint
# ----------------------------------------------------------------------------
def _reload(table, frame, hop):
    from modules import data_utils
    from modules.data_utils import Compose
    parser = data_utils.Data_Parser(TOY, table)
    return parser.get_data(transform=Compose([data_utils.ToTensor(), data_utils.STFT(frame, hop)]))


def test_segment_cli_on_toy_data(tmp_path):
    import segment
    out = os.path.join(str(tmp_path), "s", "segmented.csv")
    base = [CKPT, TOY, ANN, "1.0", "--max_length", "60", "--min_length", "3"]
    assert segment.main(base + ["-S", out]) == out
    df = pd.read_csv(out)
    assert list(df.columns) == list(segment.COLUMNS)
    wav = pd.read_csv(ANN)["input_path"][0]
    fs, wave = segment.read_wave(TOY, wav)
    frame, hop = int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))
    n_frames = segment.num_frames(len(wave), frame, hop)
    assert len(df) >= 1 and (df["input_path"] == wav).all() and (df["label"] == df["category_ix"]).all()
    assert ((df["category_ix"] >= 0) & (df["category_ix"] < 16)).all()
    assert ((df["length"] >= 3) & (df["length"] <= 60)).all()
    on, off = df["onset"].to_numpy(), df["offset"].to_numpy()
    assert (on >= 0).all() and (off <= len(wave) / fs).all() and (on < off).all() and (off[:-1] < on[1:]).all()
    # without a gap score the segments tile the recording
    assert int(df["length"].sum()) == n_frames and round(on[0] * fs) == 0
    assert (np.round(on[1:] * fs) == (np.cumsum(df["length"].to_numpy())[:-1]) * hop).all()
    ds = _reload(out, frame, hop)
    assert len(ds) == len(df)
    for i in range(len(ds)):
        assert ds[i][0].shape[0] == int(df["length"][i]), i
    print(f"segment.py: {len(df)} segments over {n_frames} frames, lengths {df['length'].min()} .. "
          f"{df['length'].max()}, categories {sorted(df['category_ix'].unique().tolist())}")
    # a rerun is identical and keeps the earlier table as .prev
    segment.main(base + ["-S", out])
    assert sorted(os.listdir(os.path.dirname(out))) == ["segmented.csv", "segmented.csv.prev"]
    assert pd.read_csv(out).equals(pd.read_csv(out + ".prev"))
    # a gap score and a negative bonus: fewer segments, frames left uncovered, still loadable
    out_g = os.path.join(str(tmp_path), "g", "segmented.csv")
    best = float(df["segment_score"].sum()) / n_frames
    segment.main(base + ["-S", out_g, "--gap_score", str(best), "--segment_bonus", "-20", "--prior", "uniform"])
    dg = pd.read_csv(out_g)
    assert int(dg["length"].sum()) < n_frames and ((dg["length"] >= 3) & (dg["length"] <= 60)).all()
    assert (dg["offset"].to_numpy()[:-1] < dg["onset"].to_numpy()[1:]).all()
    dsg = _reload(out_g, frame, hop)
    assert all(dsg[i][0].shape[0] == int(dg["length"][i]) for i in range(len(dsg)))
    # a background fitted from the frames the toy annotation leaves uncovered
    out_f = os.path.join(str(tmp_path), "f", "segmented.csv")
    npz = os.path.join(str(tmp_path), "f", "gap.npz")
    segment.main(base + ["-S", out_f, "--fit_gap", ANN, "--gap_model_out", npz])
    with np.load(npz) as z:
        assert z["mu"].shape == z["log_var"].shape == (65,)
    out_m = os.path.join(str(tmp_path), "m", "segmented.csv")
    segment.main(base + ["-S", out_m, "--gap_model", npz])
    assert pd.read_csv(out_m).equals(pd.read_csv(out_f))
