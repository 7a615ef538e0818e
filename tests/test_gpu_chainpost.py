"""Segmentation posteriors under the chain on the GPU:
``abcd_span_chain_posterior`` through the C ABI and the operator,
``segment_chain_posteriors`` / ``refit_transitions_em`` and ``segment.py
--chain_posteriors`` / ``--refit_method em``, against the longdouble reference
of ``chainpost_cases.py``.

Bars (derived in ``chainpost_cases.py``): the lattice and log_z within the
lattice bar 8 N (D + K + 2) 2^-53 (M + 1); posteriors, the gap curve and
span_post within 5 lattice bars; a count entry within 5 lattice bars times (1 +
its reference value); identities (i)-(v) on the device's own outputs within 5
lattice bars times N; |bG[0] - log_z| within a lattice bar; two calls, and the
strided and the dense layout, agree bit for bit.  Every observed figure is
printed (``-rA``) and kept with ``ABCD_PARITY_DUMP``
(profiles/chainpost_errors.json)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import chainpost_cases as CP
import score_cases as S
import syntax_cases as SX
from test_gpu_score import ANN, CKPT, TOY
from test_gpu_syntax import _small_recording

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")
SENT = -7.0  # what the outputs hold before a call
KEYS = ("lattice", "lattice_g", "post_k", "gap_post", "trans_counts", "init_counts", "span_post")


# ----------------------------------------------------------------------------
# 1. abcd_span_chain_posterior through ctypes, on synthetic tables
# ----------------------------------------------------------------------------
def fb_call(table, d_min, gap, bonus, trans, init, scale=1.0, padded=True, keep_lattice=True, want_counts=True,
            want_table=True, n=None):
    """abcd_span_chain_posterior on host arrays -> dict of numpy outputs under
    the reference's keys.  ``padded``: the table travels with ld_k = K + 3,
    log_trans with ld_trans = K + 1 and span_post with ld_post = D + 2 (NaN in
    the padding); otherwise everything is dense.  The table's entries with d >
    e hold NaN: they are never read.  Every output holds SENT before the call
    and carries a guard (an extra row or entry) that must keep it; the
    workspace holds 0xFF.  ``keep_lattice`` False leaves the lattice in the
    workspace."""
    from modules import _native as N_
    lib = N_.lib()
    N, D, K = table.shape[0] - 1, table.shape[1], table.shape[2]
    N = N if n is None else n
    ldk, ldt, ldp = (K + 3, K + 1, D + 2) if padded else (K, K, D)
    tb = torch.full((N + 1, D, ldk), NAN, dtype=torch.float64)
    tb[:, :, :K] = torch.from_numpy(table[:N + 1])
    for e in range(min(N + 1, D)):
        tb[e, e:] = NAN
    lt = torch.full((K, ldt), NAN)
    lt[:, :K] = torch.from_numpy(np.asarray(trans, dtype=np.float32))
    tb, lt, li = tb.cuda(), lt.cuda(), torch.from_numpy(np.asarray(init, dtype=np.float32)).cuda()
    g = None if gap is None else torch.from_numpy(np.asarray(gap, dtype=np.float32)[:N]).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    lz = torch.full((2,), SENT, **f64)
    lat = torch.full((5 * (N + 1) * K + 1,), SENT, **f64) if keep_lattice else None
    latg = torch.full((2 * (N + 1) + 1,), SENT, **f64) if keep_lattice else None
    pk = torch.full((2 * (N + 1) * K + 1,), SENT, **f64)
    gp = torch.full((N + 2,), SENT, **f64)
    tc = torch.full((K * K + 1,), SENT, **f64) if want_counts else None
    ic = torch.full((K + 1,), SENT, **f64) if want_counts else None
    sp = torch.full((N + 2, ldp), SENT, **f64) if want_table else None
    ws = N_.workspace(lib.abcd_span_chain_posterior_workspace_bytes(N, D, K), "cuda")
    ws.fill_(0xFF)
    rc = lib.abcd_span_chain_posterior(N_.ptr(tb), ldk, N, D, K, d_min, N_.ptr(g), float(bonus), float(scale),
                                       N_.ptr(lt), ldt, N_.ptr(li), N_.ptr(lz), N_.ptr(lat), N_.ptr(latg), N_.ptr(pk),
                                       N_.ptr(gp), N_.ptr(tc), N_.ptr(ic), N_.ptr(sp), ldp, N_.ptr(ws), ws.numel(),
                                       N_.stream())
    torch.cuda.synchronize()
    assert rc == 0
    # the guards
    assert float(lz[1]) == SENT and float(pk[-1]) == SENT and float(gp[N + 1]) == SENT
    out = dict(log_z=float(lz[0]), post_k=pk[:-1].reshape(2, N + 1, K).cpu().numpy(), gap_post=gp[:N + 1].cpu().numpy())
    if keep_lattice:
        assert float(lat[-1]) == SENT and float(latg[-1]) == SENT
        out.update(lattice=lat[:-1].reshape(5, N + 1, K).cpu().numpy(), lattice_g=latg[:-1].reshape(2, N + 1).cpu().numpy())
    if want_counts:
        assert float(tc[-1]) == SENT and float(ic[-1]) == SENT
        out.update(trans_counts=tc[:-1].reshape(K, K).cpu().numpy(), init_counts=ic[:-1].cpu().numpy())
    if want_table:
        assert (sp[N + 1] == SENT).all() and (sp[:, D:] == SENT).all()
        out["span_post"] = sp[:N + 1, :D].cpu().numpy()
    return out


def _same_bits(a, b, keys):
    for key in keys:
        if key in a and key in b:
            assert np.array_equal(np.asarray(a[key], dtype=np.float64).view(np.int64),
                                  np.asarray(b[key], dtype=np.float64).view(np.int64)), key


def check_fb(ref, got, N, D, K, tag):
    """One call's outputs against the reference -> the worst error over its bar per group."""
    bar = CP.lattice_bar(N, D, K, np.concatenate([ref["lattice"].reshape(-1), ref["lattice_g"].reshape(-1)]))
    fig = {}
    if ref["log_z"] == NEG:                                         # no cover: -inf and zeros, exactly
        assert got["log_z"] == NEG, tag
        for key in ("post_k", "gap_post", "trans_counts", "init_counts", "span_post"):
            assert (got[key] == 0).all(), (tag, key)
    else:
        fig["log_z_over_bar"] = abs(got["log_z"] - ref["log_z"]) / bar
    worst = 0.0
    for key in ("lattice", "lattice_g"):
        r, g = ref[key], got[key]
        fin = np.isfinite(r)
        assert np.array_equal(g[~fin].view(np.int64), r[~fin].view(np.int64)), (tag, key)   # -inf where the reference is
        if fin.any():
            worst = max(worst, float(np.abs(g[fin] - r[fin]).max()))
    fig["lattice_over_bar"] = worst / bar
    fig["post_over_bar"] = max(float(np.abs(got[k] - ref[k]).max()) for k in ("post_k", "gap_post")) / (5 * bar)
    fig["span_over_bar"] = float(np.abs(got["span_post"] - ref["span_post"]).max()) / (5 * bar)
    fig["counts_over_bar"] = max(float((np.abs(got[k] - ref[k]) / (1.0 + ref[k])).max())
                                 for k in ("trans_counts", "init_counts")) / (5 * bar)
    ids = CP.identities(got)
    fig["identities_over_bar"] = max(ids.values()) / (5 * bar * max(N, 1))
    bg0 = got["lattice_g"][1][0]
    fig["bg0_over_bar"] = 0.0 if (bg0 == NEG and got["log_z"] == NEG) else abs(bg0 - got["log_z"]) / bar
    for key in ("post_k", "gap_post", "span_post"):
        assert (got[key] >= 0).all() and (got[key] <= 1.0 + 5 * bar).all(), (tag, key)
    for key, v in fig.items():
        assert np.isfinite(v) and v <= 1.0, (tag, key, v, bar)
    return fig


def sweep_case(N, D, K, kind):
    """Every call of chain_inputs(N, D, K, kind): the padded layout with the
    caller's lattice against the reference, the dense layout with the lattice
    in the workspace bit for bit against it; the first call twice; the last
    call also at scale = 0.25; nopath also without an initial distribution."""
    c = SX.chain_inputs(N, D, K, kind)
    rows, reached = [], 0
    for i, (d_min, gap, bonus, tag) in enumerate(c["calls"]):
        variants = [(False, 1.0)] + ([(True, 1.0)] if kind == "nopath" else []) + (
            [(False, CP.SCALE)] if i == len(c["calls"]) - 1 else [])
        for init_none, scale in variants:
            init = c["init_none"] if init_none else c["init"]
            ref = CP.reference_of(N, D, K, kind, i, init_none, scale)
            got = fb_call(c["table"], d_min, gap, bonus, c["trans"], init, scale)
            fig = check_fb(ref, got, N, D, K, (N, D, K, kind, tag, init_none, scale))
            dense = fb_call(c["table"], d_min, gap, bonus, c["trans"], init, scale, padded=False, keep_lattice=False)
            _same_bits(got, dense, ("log_z",) + KEYS)
            if i == 0:
                _same_bits(got, fb_call(c["table"], d_min, gap, bonus, c["trans"], init, scale), ("log_z",) + KEYS)
            reached += ref["log_z"] > NEG
            if init_none:                                           # a gap-only cover or nothing
                assert (ref["log_z"] > NEG) == (gap is not None) and ref["post_k"].sum() == 0
            rows.append(dict(case=f"n{N}d{D}k{K}{kind}{tag}{'noinit' if init_none else ''}s{scale}", **fig))
    worst = {k: max(r[k] for r in rows if k in r) for k in sorted({k for r in rows for k in r} - {"case"})}
    print(f"N={N} D={D} K={K} {kind}: {len(rows)} calls, {reached} with a cover; worst error over bar: "
          + ", ".join(f"{k[:-9]} {v:.2g}" for k, v in worst.items()))
    if kind in ("random", "tied", "gaps", "bonus"):
        assert reached > 0
    return [dict(case=f"n{N}d{D}k{K}{kind}", calls=len(rows), with_cover=int(reached), **worst)]


@pytest.mark.parametrize("kind", CP.CHAIN_KINDS)
@pytest.mark.parametrize("K", CP.CHAIN_K)
@pytest.mark.parametrize("ND", CP.CHAIN_ND, ids=lambda v: f"n{v[0]}d{v[1]}")
def test_span_chain_posterior_is_the_reference(ND, K, kind):
    from modules import _native as N_
    N, D = ND
    res = N_.c_int(-1)
    assert N_.lib().abcd_span_chain_posterior_plan(K, D, N_.ctypes.byref(res), None, None) == 0
    assert bool(res.value) == (K <= 128)            # K = 130 streams log_trans from global memory
    CP.dump(f"sweep_n{N}d{D}k{K}{kind}", sweep_case(N, D, K, kind))


@pytest.mark.parametrize("kind", CP.CHAIN_KINDS)
@pytest.mark.parametrize("K", CP.WIDTH_K)
def test_span_chain_posterior_at_the_launch_width_threshold(K, kind):
    """K = 256 is the last shape of the 16-wave launch, 257 the first of the 4-wave one."""
    from modules import _native as N_
    thr = N_.c_int(-1)
    assert N_.lib().abcd_span_chain_posterior_plan(K, 5, None, N_.ctypes.byref(thr), None) == 0
    assert thr.value == (1024 if K <= 256 else 256)
    CP.dump(f"width_k{K}{kind}", sweep_case(33, 5, K, kind))


def test_span_chain_posterior_at_the_category_limit():
    """K = 1024: the largest LDS request of the 4-wave launch, 16 strides over k per lane."""
    CP.dump("width_k1024random", sweep_case(2, 1, 1024, "random"))


def test_span_chain_posterior_optional_outputs_and_empty_recording():
    c = SX.chain_inputs(70, 17, 130, "random")
    d_min, gap, bonus, _ = c["calls"][1]
    a = fb_call(c["table"], d_min, gap, bonus, c["trans"], c["init"])
    b = fb_call(c["table"], d_min, gap, bonus, c["trans"], c["init"], want_counts=False, want_table=False)
    assert "trans_counts" not in b and "span_post" not in b
    _same_bits(a, b, ("log_z", "lattice", "lattice_g", "post_k", "gap_post"))
    # N = 0: log_z = 0, bW[0] = G[0] = bG[0] = 0, the other planes -inf, zeros; nothing is read (the inputs hold NaN)
    K, D = 5, 3
    z = fb_call(np.full((1, D, K), NAN), 1, None, 0.0, np.full((K, K), NAN), np.full(K, NAN), n=0)
    assert z["log_z"] == 0.0 and (z["lattice"][:4] == NEG).all() and (z["lattice"][4] == 0).all()
    assert (z["lattice_g"] == 0).all() and (z["post_k"] == 0).all() and (z["gap_post"] == 0).all()
    assert (z["trans_counts"] == 0).all() and (z["init_counts"] == 0).all() and (z["span_post"] == 0).all()
    ref = CP.chain_posterior_reference(np.full((1, D, K), NEG), 1, np.zeros((K, K)), np.zeros(K))
    _same_bits(z, ref, KEYS)


# ----------------------------------------------------------------------------
# 2. the operator
# ----------------------------------------------------------------------------
def _op(c, d_min, gap, bonus, scale=1.0, counts=True, table=True, trans=None, init=None):
    from modules import ops
    g = None if gap is None else torch.from_numpy(np.asarray(gap, dtype=np.float32)).cuda()
    lt = torch.from_numpy(np.asarray(c["trans"] if trans is None else trans, dtype=np.float32)).cuda()
    li = torch.from_numpy(np.asarray(c["init"] if init is None else init, dtype=np.float32)).cuda()
    return ops.span_chain_posterior(torch.from_numpy(c["table"]).cuda(), d_min, g, float(bonus), float(scale), lt, li,
                                    counts, table)


def test_operator_is_the_abi_is_forward_only_and_checks_shapes():
    from modules import ops
    N, D, K = 33, 5, 33
    c = SX.chain_inputs(N, D, K, "random")
    d_min, gap, bonus, _ = c["calls"][1]
    out = _op(c, d_min, gap, bonus)
    got = fb_call(c["table"], d_min, gap, bonus, c["trans"], c["init"])
    assert [tuple(t.shape) for t in out] == [(), (5, N + 1, K), (2, N + 1), (2, N + 1, K), (N + 1,), (K, K), (K,),
                                             (N + 1, D)]
    for t, key in zip(out, ("log_z",) + KEYS):
        assert np.array_equal(t.cpu().numpy().view(np.int64), np.asarray(got[key], dtype=np.float64).view(np.int64)), key
    out = _op(c, d_min, gap, bonus, counts=False, table=False)
    assert [tuple(t.shape) for t in out[5:]] == [(0, 0), (0,), (0, 0)]
    tb = torch.from_numpy(c["table"]).cuda()
    lt, li = torch.from_numpy(c["trans"]).cuda(), torch.from_numpy(c["init"]).cuda()
    z = ops.span_chain_posterior(tb[:1], 1, None, 0.0, 1.0, lt, li, True, True)         # N = 0
    assert float(z[0]) == 0.0 and (z[3] == 0).all() and (z[5] == 0).all() and tuple(z[7].shape) == (1, D)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.span_chain_posterior(tb.clone().requires_grad_(True), 1, None, 0.0, 1.0, lt, li, False, False)
    for bad in (dict(d_min=6), dict(scale=0.0), dict(scale=float("inf")), dict(lt=lt[:, :5]),
                dict(gap=torch.zeros(5).cuda()), dict(tb=tb[:, :, 0])):
        a = dict(tb=tb, d_min=1, gap=None, scale=1.0, lt=lt, li=li)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.span_chain_posterior(a["tb"], a["d_min"], a["gap"], 0.0, a["scale"], a["lt"], a["li"], False, False)


def test_table_beyond_the_index_limit_is_refused():
    from modules import _native as N_
    assert N_.lib().abcd_span_chain_posterior_workspace_bytes(70000, 300, 128) == 0
    from modules import ops
    with pytest.raises(N_.HipError, match="index limit"):
        # an expanded view: the shape check comes before any copy
        ops.span_chain_posterior(torch.zeros(1, 1, 1, dtype=torch.float64, device="cuda").expand(70001, 300, 128), 1,
                                 None, 0.0, 1.0, torch.zeros(128, 128).cuda(), torch.zeros(128).cuda(), False, False)


@pytest.mark.parametrize("K", (3, 33, 130))
def test_context_free_chain_reduces_to_span_posterior(K):
    """(vi): every row of log_trans and log_init equal to one log_softmax(lw):
    log_z, the category-summed curves and span_post are ops.span_posterior's on
    LSE_k (T + lw), formed on the same device."""
    from modules import ops
    N, D = 70, 17
    c = SX.chain_inputs(N, D, K, "random")
    g = np.random.default_rng(K)
    p = SX.log_softmax(g.normal(0.0, 1.0, size=K)).astype(np.float32)
    rows = []
    for d_min, gap, bonus, tag in c["calls"] + [(2, c["calls"][1][1], -1.5, "bonus")]:
        out = _op(c, d_min, gap, bonus, trans=np.tile(p[None, :], (K, 1)), init=p)
        span = torch.logsumexp(torch.from_numpy(c["table"]).cuda() + torch.from_numpy(p).cuda().double(), 2)
        gp = None if gap is None else torch.from_numpy(gap).cuda()
        log_z, lat, post, table = ops.span_posterior(span, d_min, gp, float(bonus), True)
        if not bool(log_z > NEG):                       # d_min = D without a gap: 70 frames are no multiple of 17
            assert float(out[0]) == NEG and gap is None and float(out[3].sum()) == 0.0
            continue
        bar = CP.lattice_bar(N, D, K, np.concatenate([out[1].cpu().numpy().reshape(-1), lat.cpu().numpy().reshape(-1)]))
        err = [abs(float(out[0]) - float(log_z)) / bar,
               float((torch.stack([out[3][0].sum(1), out[3][1].sum(1), out[4]]) - post).abs().max()) / (5 * bar),
               float((out[7] - table).abs().max()) / (5 * bar)]
        rows.append(dict(case=f"k{K}{tag}", over_bar=max(err)))
        assert max(err) <= 2.0, (K, tag, err)           # two programmes, each within its bar of the truth
    print(f"K={K}: context-free chain against ops.span_posterior: worst difference over bar "
          f"{max(r['over_bar'] for r in rows):.2g}")
    assert len(rows) >= 5
    CP.dump(f"reduction_k{K}", rows)


@pytest.mark.parametrize("kind", CP.CHAIN_KINDS)
@pytest.mark.parametrize("K", CP.CHAIN_K)
@pytest.mark.parametrize("ND", CP.CHAIN_ND, ids=lambda v: f"n{v[0]}d{v[1]}")
def test_evidence_is_at_least_the_best_path(ND, K, kind):
    from modules import ops
    N, D = ND
    c = SX.chain_inputs(N, D, K, kind)
    tb = torch.from_numpy(c["table"]).cuda()
    lt, li = torch.from_numpy(c["trans"]).cuda(), torch.from_numpy(c["init"]).cuda()
    covered = 0
    for d_min, gap, bonus, tag in c["calls"]:
        g = None if gap is None else torch.from_numpy(gap).cuda()
        ev = float(ops.span_chain_posterior(tb, d_min, g, float(bonus), 1.0, lt, li, False, False)[0])
        best = float(ops.span_chain_viterbi(tb, d_min, g, float(bonus), lt, li, False)[0])
        assert (ev > NEG) == (best > NEG), (K, kind, tag)
        if best > NEG:
            covered += 1
            assert ev >= best - 1e-9 * (1.0 + abs(best)), (K, kind, tag, ev, best)
    if kind in ("random", "tied", "gaps", "bonus"):
        assert covered > 0


def test_planted_alternation_through_the_operator():
    c = SX.planted_alternation()
    out = _op(c, 1, None, 0.0)
    assert abs(float(out[3][1].sum()) - SX.ALT_SEGMENTS) <= 1e-9
    tc, ic = out[5].cpu().numpy(), out[6].cpu().numpy()
    assert np.abs(tc - np.array([[0.003, 2.997], [2.997, 0.003]])).max() <= 1e-3, tc
    assert np.abs(ic - 0.5).max() <= 1e-12
    ref = CP.chain_posterior_reference(c["table"], 1, c["trans"], c["init"])
    bar = CP.lattice_bar(c["N"], c["D"], 2, ref["lattice"])
    assert np.abs(tc - ref["trans_counts"]).max() <= 5 * bar * 4.0 and abs(float(out[0]) - ref["log_z"]) <= bar


# ----------------------------------------------------------------------------
# 3. segment_chain_posteriors and EM
# ----------------------------------------------------------------------------
def test_segment_chain_posteriors_on_a_small_model():
    from modules import segmentation
    from modules.sequence import TransitionModel
    dec, protos, frames, K, D = _small_recording(list(S.E2E_SMALL)[0])
    n = frames.shape[0]
    lw = torch.linspace(-1.0, 1.0, K).cuda()
    model = TransitionModel.from_log_weight(lw)
    model.log_trans.add_(torch.eye(K, device="cuda"))                       # a sticky chain, rows renormalised
    model.log_trans.copy_(torch.log_softmax(model.log_trans, 1))
    tiled = segmentation.segment_frames(dec, protos, frames, D, log_weight=lw, transitions=model)
    # a gap two nats below the tiled path's average frame: most frames stay inside segments, a few do not
    const = torch.full((n,), float(tiled["path_score"]) / n - 2.0, device="cuda")
    for gap, bonus, d_min, T in ((None, 0.0, 1, 1.0), (const, -3.0, 2, 1.0), (const, 0.0, 1, 8.0)):
        want = segmentation.segment_frames(dec, protos, frames, D, min_length=d_min, gap=gap, seg_bonus=bonus,
                                           log_weight=lw, transitions=model)
        out = segmentation.segment_chain_posteriors(dec, protos, frames, D, model, min_length=d_min, log_weight=lw,
                                                    gap=gap, seg_bonus=bonus, temperature=T, want_counts=True,
                                                    want_table=True, with_segments=True)
        seg = out["segmentation"]
        assert set(seg) == set(want)
        for key in want:                                                    # the segments and the path score, bit for bit
            assert seg[key].dtype == want[key].dtype and torch.equal(
                seg[key].view(torch.int64) if seg[key].dtype == torch.float64 else seg[key],
                want[key].view(torch.int64) if want[key].dtype == torch.float64 else want[key]), key
        k = len(seg["onset"])
        assert (k >= 1 or gap is not None) and out["label_posterior"].shape == out["span_posterior"].shape == (k,)
        tol = 1e-9
        assert (out["label_posterior"] >= 0).all() and (out["label_posterior"] <= out["span_posterior"] + tol).all()
        assert (out["span_posterior"] <= 1.0 + tol).all()
        assert out["frame_category"].shape == (n, K) and out["frame_category"].dtype == torch.float64
        assert out["onset_by_category"].shape == out["end_by_category"].shape == (n + 1, K)
        assert out["onset"].shape == out["end"].shape == out["gap"].shape == (n + 1,)
        assert out["span"].shape == (n + 1, D) and out["trans_counts"].shape == (K, K)
        # every frame is background or inside a segment of some category
        assert float((out["gap"][:n] + out["frame_category"].sum(1) - 1.0).abs().max()) <= 1e-9
        assert abs(float(out["expected_segments"]) - float(out["category_usage"].sum())) <= 1e-9
        assert abs(float(out["init_counts"].sum()) - (1.0 - float(out["no_segment"]))) <= 1e-9
        if T == 1.0:
            assert float(out["log_evidence"]) >= float(want["path_score"]) - 1e-9 * abs(float(want["path_score"]))
        print(f"gap {'none' if gap is None else 'const'} bonus {bonus} d_min {d_min} T {T}: {k} segments, expected "
              f"{float(out['expected_segments']):.3f}; label posteriors {out['label_posterior'].min():.3f} .. "
              f"{out['label_posterior'].max():.3f}, span posteriors {out['span_posterior'].min():.3f} .. "
              f"{out['span_posterior'].max():.3f}")
    with pytest.raises(ValueError):
        segmentation.segment_chain_posteriors(dec, protos, frames, D, TransitionModel(K + 1).cuda())
    with pytest.raises(ValueError):
        segmentation.segment_chain_posteriors(dec, protos, frames, D, model, temperature=0.0)
    with pytest.raises(ValueError, match="posteriors"):                     # the pinned refusal stays
        segmentation.segment_frames(dec, protos, frames, D, transitions=model, posteriors=True)


@pytest.mark.parametrize("temperature", (1.0, 4.0))
def test_refit_transitions_em_is_the_reference_em(temperature):
    from modules import ops, segmentation
    from modules.sequence import TransitionModel
    N, D, K = CP.EM_SHAPE
    recs = CP.em_recordings()
    d_min, c = 1, 1.0 / K
    ref = CP.em_reference(recs, K, d_min, CP.EM_ITERS, c, temperature)
    dev = [(torch.from_numpy(t).cuda(), torch.from_numpy(g).cuda()) for t, g in recs]

    def posterior_fn(rec, model):
        out = ops.span_chain_posterior(rec[0], d_min, rec[1], 0.0, 1.0 / temperature, model.log_trans,
                                       model.log_init, True, False)
        return dict(log_evidence=out[0], trans_counts=out[5], init_counts=out[6])

    model = TransitionModel(K).cuda()
    totals = segmentation.refit_transitions_em(posterior_fn, dev, model, CP.EM_ITERS + 1, c, temperature)
    # the evidence part of the bar: a lattice bar per recording, times the temperature; the stored fp32 parameters
    # may round differently after an M-step on counts that differ within their bar, which the slack covers
    bar = temperature * len(recs) * 8.0 * N * (D + K + 2) * 2.0 ** -53 * (ref["M"] + 1.0) * (1 if CP.LD_OK else 2)
    slack = CP.em_slack(ref["L"], recs, d_min, c, K)
    err = max(abs(a - b) for a, b in zip(totals, ref["objectives"]))
    drops = [a - b for a, b in zip(totals[:-1], totals[1:])]
    print(f"temperature {temperature}: objectives {['%.6f' % v for v in totals]}; worst difference from the reference "
          f"EM {err:.2e} (bar {bar:.2e} + slack {slack:.2e}); largest drop {max(drops):.2e}")
    CP.dump(f"em_t{temperature}", [dict(case=f"t{temperature}", over_bar=err / (bar + slack))])
    assert err <= bar + slack
    assert max(drops) <= slack and totals[-1] > totals[0]
    tc, ic = model.last_counts
    assert tc.shape == (K, K) and 0.0 < float(ic.sum()) <= len(recs) + 1e-9     # one first segment per recording at most


# ----------------------------------------------------------------------------
# 4. segment.py --chain_posteriors and --refit_method em on the toy data
# ----------------------------------------------------------------------------
def test_segment_cli_with_chain_posteriors_and_em(tmp_path):
    import segment
    K = 16
    base = [CKPT, TOY, ANN, "1.0", "--max_length", "60", "--min_length", "3"]
    p = np.full((K, K), 0.2 / (K - 1))
    np.fill_diagonal(p, 0.8)
    ft, tt = np.divmod(np.arange(K * K), K)
    tcsv = os.path.join(str(tmp_path), "transitions.csv")
    pd.DataFrame({"from_ix": ft, "to_ix": tt, "probability": p.reshape(-1), "expected_count": 0.0}).to_csv(
        tcsv, index=False)
    plain = os.path.join(str(tmp_path), "t", "segmented.csv")
    segment.main(base + ["-S", plain, "--transitions", tcsv])
    out = os.path.join(str(tmp_path), "p", "segmented.csv")
    rec = os.path.join(str(tmp_path), "p", "recordings.csv")
    curves = os.path.join(str(tmp_path), "p", "curves")
    segment.main(base + ["-S", out, "--transitions", tcsv, "--chain_posteriors", "--posterior_temperature", "50",
                         "--recordings_out", rec, "--curves_dir", curves])
    dt, dp = pd.read_csv(plain), pd.read_csv(out)
    assert list(dp.columns) == list(segment.COLUMNS) + list(segment.SYNTAX_COLUMNS) + list(
        segment.CHAIN_POSTERIOR_COLUMNS)
    assert dp[list(dt.columns)].equals(dt)                                  # the cut itself is the flag-less one
    for col in segment.CHAIN_POSTERIOR_COLUMNS:
        assert ((dp[col] >= 0) & (dp[col] <= 1 + 1e-9)).all(), col
    assert (dp["label_posterior"] <= dp["span_posterior"] + 1e-9).all()
    rr = pd.read_csv(rec)
    assert list(rr.columns) == list(segment.RECORDING_COLUMNS) and len(rr) == dt["input_path"].nunique()
    assert np.isfinite(rr["log_evidence"]).all() and (rr["expected_segments"] > 0).all()
    files = sorted(os.listdir(curves))
    assert len(files) == len(rr)
    with np.load(segment.curve_path(curves, rr["input_path"][0])) as z:
        n = int(rr["n_frames"][0])
        assert z["onset"].shape == z["end"].shape == z["gap"].shape == (n + 1,)
        assert z["frame_category"].shape == z["frame_category_probability"].shape == (n,)
        assert ((z["frame_category"] >= 0) & (z["frame_category"] < K)).all()
        assert ((z["frame_category_probability"] > 0) & (z["frame_category_probability"] <= 1 + 1e-9)).all()
    print(f"segment.py --chain_posteriors: {len(dp)} segments; label posteriors {dp['label_posterior'].min():.3f} .. "
          f"{dp['label_posterior'].max():.3f} at temperature 50")
    # EM: a row-stochastic matrix and non-integer expected counts
    out_r = os.path.join(str(tmp_path), "r", "segmented.csv")
    tout = os.path.join(str(tmp_path), "r", "transitions.csv")
    segment.main(base + ["-S", out_r, "--transitions", tcsv, "--refit_transitions", "1", "--refit_method", "em",
                         "--transitions_out", tout])
    tr = pd.read_csv(tout)
    assert list(tr.columns) == list(segment.TRANSITION_COLUMNS) and len(tr) == K * K
    assert np.allclose(tr["probability"].to_numpy().reshape(K, K).sum(1), 1.0, atol=1e-5)
    cnt = tr["expected_count"].to_numpy()
    assert (cnt >= 0).all() and cnt.sum() > 0 and np.abs(cnt - np.round(cnt)).max() > 1e-6
    assert list(pd.read_csv(out_r).columns) == list(segment.COLUMNS) + list(segment.SYNTAX_COLUMNS)
    for bad in (["--transitions", tcsv, "--posteriors"], ["--chain_posteriors"], ["--refit_method", "em"]):
        with pytest.raises(SystemExit):
            segment.main(base + ["-S", out_r] + bad)
