"""Segmentation posteriors on the GPU: ``abcd_span_evidence`` and
``abcd_span_posterior`` through the C ABI and the operators,
``RNN_Variational_Decoder.span_evidence`` / ``segmentation.segment_posteriors``
/ ``segment_frames(posteriors=True)`` end to end and ``segment.py
--posteriors``, against the references of ``spanpost_cases.py``.

Bars (``spanpost_cases.py``): ``span_lse`` within 1e-4 of ``max_p A`` over the
admissible prototypes; the best outputs of the same pass EQUAL to
``abcd_span_scores``' bits; identical prototypes give ``log P`` within 1e-6; the
lattice within ``8 N (D + 2) 2^-53 (M + 1)`` and the posteriors within five
times that of the np.longdouble recursions.  Every observed figure is printed
(``-rA``) and kept with ``ABCD_PARITY_DUMP`` (profiles/spanpost_errors.json)."""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import pairwise_cases as PW
import score_cases as S
import span_cases as SP
import spanpost_cases as SQ
from test_gpu_score import ANN, CKPT, TOY, _small_modules
from test_gpu_span import SENT, _bits, span_buffers, span_call

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")


# ----------------------------------------------------------------------------
# 1. abcd_span_evidence through ctypes
# ----------------------------------------------------------------------------
def evidence_call(c, x, ldx, mu, ldm, lv, ldl, o, lw, n=None, pad=1, want_best=True):
    """abcd_span_evidence -> (rc, lse, score, cat): (N + 2) x (D + pad) buffers
    holding SENT before the call (score / cat None without want_best); the
    workspace holds NaN."""
    from modules import _native as N
    lib = N.lib()
    n = c["N"] if n is None else n
    D, P, F = c["D"], c["P"], c["F"]
    lse = torch.full((n + 2, D + pad), SENT, dtype=torch.float64, device="cuda")
    score = torch.full((n + 2, D + pad), SENT, dtype=torch.float64, device="cuda") if want_best else None
    cat = torch.full((n + 2, D + pad), int(SENT), dtype=torch.int32, device="cuda") if want_best else None
    ws = N.workspace(lib.abcd_span_evidence_workspace_bytes(n, D, P), "cuda")
    ws.fill_(0xFF)
    rc = lib.abcd_span_evidence(N.ptr(x), ldx, n, F, P, D, D + SP.T_EXTRA, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(o),
                                N.ptr(lw), N.ptr(lse), N.ptr(score), N.ptr(cat), D + pad, N.ptr(ws), ws.numel(),
                                N.stream())
    torch.cuda.synchronize()
    return rc, lse, score, cat


@pytest.mark.parametrize("F", SQ.EV_F)
@pytest.mark.parametrize("P", SQ.EV_P)
@pytest.mark.parametrize("ND", SQ.EV_SHAPES, ids=lambda v: f"n{v[0]}d{v[1]}")
def test_span_evidence_abi(ND, P, F):
    N, D = ND
    c = SQ.evidence_case(N, D, P, F)
    valid = np.zeros((N + 1, D), dtype=bool)
    for e in range(1, N + 1):
        valid[e, :min(D, e)] = True
    rows = []
    for ld in (F, SP.PAD_LD):
        b = span_buffers(c, ld)                     # padding columns, tail rows and steps >= D are NaN
        rc, lse, score, cat = evidence_call(c, **b)
        assert rc == 0
        for t in (lse, score):
            assert (t[:, D:] == SENT).all() and (t[N + 1:] == SENT).all()          # nothing outside N + 1 x D
        assert (cat[:, D:] == int(SENT)).all() and (cat[N + 1:] == int(SENT)).all()
        got = lse[:N + 1, :D].cpu().numpy()
        assert (got[~valid] == NEG).all()                                          # exactly -inf
        assert np.isfinite(got[valid]).all() and np.isfinite(c["lse"][valid]).all()
        err = np.abs(got[valid] - c["lse"][valid]) / c["unit"][valid]
        over_best = (got[valid] - c["ref"]["score"][valid]).max()
        print(f"N={N} D={D} P={P} F={F} ld={ld}: worst |span_lse - ref| / max_p A {err.max():.2e}; the sum exceeds the "
              f"maximum by up to {over_best:.3f}")
        rows.append(dict(N=N, D=D, P=P, F=F, ld=ld, lse=float(err.max()), over_best=float(over_best)))
        assert err.max() <= SQ.BAR
        # the best outputs of the same pass: abcd_span_scores' bits on the same buffers
        rc, score0, cat0 = span_call(c, **b)
        assert rc == 0 and torch.equal(_bits(score), _bits(score0)) and torch.equal(cat, cat0)
        if P == 1:
            assert torch.equal(_bits(lse), _bits(score))
        # a second call, a call without the best outputs and an exact-width output: the same bits
        rc, lse2, score2, cat2 = evidence_call(c, **b)
        assert rc == 0 and torch.equal(_bits(lse), _bits(lse2)) and torch.equal(_bits(score), _bits(score2)) and \
            torch.equal(cat, cat2)
        rc, lse3, s3, c3 = evidence_call(c, **b, want_best=False)
        assert rc == 0 and s3 is None and c3 is None and torch.equal(_bits(lse), _bits(lse3))
        rc, lse4, _, _ = evidence_call(c, **b, pad=0)
        assert rc == 0 and torch.equal(_bits(lse4[:N + 1]), _bits(lse[:N + 1, :D])) and (lse4[N + 1:] == SENT).all()
    SQ.dump(f"evidence_n{N}d{D}p{P}f{F}", rows)


# ----------------------------------------------------------------------------
# 2. identical prototypes: the sum is the maximum plus log P
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("P", (2, 33, 65))
def test_identical_prototypes_give_log_p(P):
    rows = []
    for N, D, F in ((33, 5, 65), (70, 17, 1)):
        one = SP.abi_inputs(N, D, 1, F)
        c = dict(one, P=P, mu=one["mu"].repeat(1, P, 1), lv=one["lv"].repeat(1, P, 1), o=one["o"].repeat(1, P),
                 lw=torch.full((P,), -0.375))
        rc, lse, score, cat = evidence_call(c, **span_buffers(c, SP.PAD_LD))
        assert rc == 0
        e = torch.arange(N + 1)[:, None]
        d = torch.arange(1, D + 1)[None, :]
        ok = (d <= e).cuda()
        diff = (lse[:N + 1, :D] - score[:N + 1, :D])[ok]
        err = float((diff - math.log(P)).abs().max())
        print(f"P={P} N={N} D={D} F={F}: worst |span_lse - span_score - log P| {err:.2e}")
        rows.append(dict(P=P, N=N, D=D, F=F, err=err))
        assert (cat[:N + 1, :D][ok] == 0).all() and err <= 1e-6
    SQ.dump(f"identical_p{P}", rows)


# ----------------------------------------------------------------------------
# 3. exclusions
# ----------------------------------------------------------------------------
def test_span_evidence_exclusions():
    N, D, P, F = 70, 17, 65, 1
    c = SQ.evidence_case(N, D, P, F)
    lw = c["lw"].clone()
    lw[2], lw[5], lw[40], lw[64] = NEG, NAN, NEG, NAN
    x = c["x"].clone()
    n0 = 40
    x[n0, 0] = NAN                                   # every span that holds frame 40 has nothing left
    ref = SP.span_reference(x, c["mu"], c["lv"], c["o"], lw, D)
    want, unit = SQ.lse_reference(ref["S"]), SQ.unit_reference(ref["S"], ref["A"])
    rc, lse, score, cat = evidence_call(c, **span_buffers(c, SP.PAD_LD, x=x, lw=lw.cuda()))
    assert rc == 0
    got = lse[:N + 1, :D].cpu().numpy()
    e = np.arange(N + 1)[:, None]
    d = np.arange(1, D + 1)[None, :]
    hit = (e - d <= n0) & (n0 < e) & (d <= e)
    assert (got[hit] == NEG).all() and (got[d > e] == NEG).all() and ((want == NEG) == (got == NEG)).all()
    fin = np.isfinite(want)
    assert fin.any() and (np.abs(got[fin] - want[fin]) <= SQ.BAR * unit[fin]).all()
    assert not np.isin(cat[:N + 1, :D].cpu().numpy(), (2, 5, 40, 64)).any()
    # with every weight excluded nothing is left anywhere
    rc, lse, score, cat = evidence_call(c, **span_buffers(c, SP.PAD_LD, lw=torch.full((P,), NEG).cuda()))
    assert rc == 0 and (lse[:N + 1, :D] == NEG).all() and (cat[:N + 1, :D] == -1).all()
    # N = 0 writes row 0 only
    rc, lse, score, cat = evidence_call(c, **span_buffers(c, SP.PAD_LD), n=0)
    assert rc == 0 and (lse[0, :D] == NEG).all() and (lse[1:] == SENT).all() and (lse[0, D:] == SENT).all()


# ----------------------------------------------------------------------------
# 4. abcd_span_posterior on drawn tables
# ----------------------------------------------------------------------------
def posterior_call(W, d_min, gap, bonus, lattice=True, table=True, pad=1):
    """abcd_span_posterior on a host table in a buffer of row stride D + pad
    (NaN padding) -> (rc, log_z, lattice, post, span_post): every output holds
    SENT before the call and has a tail (and the table a padding column) that
    must still hold it afterwards (checked here)."""
    from modules import _native as N_
    lib = N_.lib()
    N, D = W.shape[0] - 1, W.shape[1]
    buf = torch.full((N + 2, D + pad), NAN, dtype=torch.float64)
    buf[:N + 1, :D] = torch.from_numpy(W)
    buf = buf.cuda()
    g = None if gap is None else torch.cat([torch.from_numpy(np.asarray(gap, dtype=np.float32)),
                                            torch.full((1,), NAN)]).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    lz = torch.full((2,), SENT, **f64)
    lat = torch.full((4 * (N + 1) + 1,), SENT, **f64) if lattice else None
    post = torch.full((3 * (N + 1) + 1,), SENT, **f64)
    tb = torch.full((N + 2, D + pad), SENT, **f64) if table else None
    ws = N_.workspace(lib.abcd_span_posterior_workspace_bytes(N, D), "cuda")
    ws.fill_(0xFF)
    rc = lib.abcd_span_posterior(N_.ptr(buf), D + pad, N, D, d_min, N_.ptr(g), float(bonus), N_.ptr(lz), N_.ptr(lat),
                                 N_.ptr(post), N_.ptr(tb), D + pad, N_.ptr(ws), ws.numel(), N_.stream())
    torch.cuda.synchronize()
    assert float(lz[1]) == SENT and float(post[-1]) == SENT
    if lattice:
        assert float(lat[-1]) == SENT
    if table:
        assert (tb[N + 1:] == SENT).all() and (tb[:, D:] == SENT).all()
    return (rc, lz[0], None if lat is None else lat[:-1].view(4, N + 1), post[:-1].view(3, N + 1),
            None if tb is None else tb[:N + 1, :D])


def check_posterior(got, ref, N, D, with_gap, tag):
    """(lattice error, posterior error, identity violation) / their bars, each asserted <= 1."""
    rc, lz, lat, post, tb = got
    assert rc == 0, tag
    lat, post, tb = lat.cpu().numpy(), post.cpu().numpy(), tb.cpu().numpy()
    bar = SQ.lattice_bar(N, D, ref["lattice"])
    assert float(lz) == lat[0, N], tag
    fin = np.isfinite(ref["lattice"])
    assert ((lat == NEG) == (ref["lattice"] == NEG)).all() and np.isfinite(lat[fin]).all(), tag
    e_lat = float(np.abs(lat[fin] - ref["lattice"][fin]).max()) if fin.any() else 0.0
    e_post = max(float(np.abs(post - ref["post"]).max()), float(np.abs(tb - ref["span_post"]).max()))
    assert (post >= 0).all() and (tb >= 0).all(), tag
    e_id = 0.0
    if ref["log_z"] == NEG:                             # no cover: -inf and all zeros
        assert float(lz) == NEG and not post.any() and not tb.any(), tag
    else:
        v = SQ.identities(post, tb, with_gap)
        e_id = max(v["cover"], v["ends"], v["onsets"], abs(lat[2, 0] - float(lz)))
    assert e_lat <= bar and e_post <= 5 * bar and e_id <= 5 * bar, (tag, e_lat, e_post, e_id, bar)
    return e_lat / bar, e_post / (5 * bar), e_id / (5 * bar)


@pytest.mark.parametrize("D", SQ.POST_D)
@pytest.mark.parametrize("N", SQ.POST_N)
def test_span_posterior_on_drawn_tables(N, D):
    worst = [0.0, 0.0, 0.0]
    reached = unreached = 0
    for kind in SQ.KINDS:
        t = SP.table_inputs(N, D, kind)
        gap_inf = t["gap"].copy()
        gap_inf[::3] = -np.inf
        first = True
        for gname, gap in (("none", None), ("drawn", t["gap"]), ("inf", gap_inf)):
            for bonus in (0.0, -1.5):
                for d_min in sorted({1, min(3, D)}):
                    tag = (N, D, kind, gname, bonus, d_min)
                    ref = SQ.posterior_reference_fast(t["score"], d_min, gap, bonus)
                    got = posterior_call(t["score"], d_min, gap, bonus)
                    e = check_posterior(got, ref, N, D, gap is not None, tag)
                    worst = [max(a, b) for a, b in zip(worst, e)]
                    reached += ref["log_z"] > NEG
                    unreached += ref["log_z"] == NEG
                    if first or gname == "drawn" and bonus == 0.0 and d_min == 1:
                        # a second call, NULL lattice, NULL table, an exact-width table: the same bits
                        first = False
                        for kw in (dict(), dict(lattice=False), dict(table=False), dict(lattice=False, table=False),
                                   dict(pad=0)):
                            rc, lz, lat, post, tb = posterior_call(t["score"], d_min, gap, bonus, **kw)
                            assert rc == 0 and torch.equal(_bits(lz), _bits(got[1])), (tag, kw)
                            assert torch.equal(_bits(post), _bits(got[3])), (tag, kw)
                            assert lat is None or torch.equal(_bits(lat), _bits(got[2])), (tag, kw)
                            assert tb is None or torch.equal(_bits(tb), _bits(got[4])), (tag, kw)
    # nothing admissible and no gap: no cover (N = 0: the empty cover, log_z = 0)
    W = np.full((N + 1, D), -np.inf)
    rc, lz, lat, post, tb = posterior_call(W, 1, None, 0.0)
    assert rc == 0 and float(lz) == (0.0 if N == 0 else NEG) and not post.any() and not tb.any()
    assert lat[:, 0].tolist() == [0.0, NEG, 0.0 if N == 0 else NEG, NEG]
    print(f"N={N} D={D}: {reached} reachable and {unreached} unreachable configurations; worst lattice error "
          f"{worst[0]:.2e} of its bar, posteriors {worst[1]:.2e}, identities and beta[0] {worst[2]:.2e} of theirs")
    SQ.dump(f"posterior_n{N}d{D}", [dict(N=N, D=D, lattice_over_bar=worst[0], post_over_bar=worst[1],
                                         identities_over_bar=worst[2], reachable=int(reached))])
    assert reached > 0


@pytest.mark.parametrize("D", (8191, 8192))
def test_span_posterior_at_the_ring_threshold(D):
    """D = 8191 is the widest table whose backward ring holds a (maximum, sum)
    pair per slot; from 8192 on a slot is one log-domain value.  N stays small:
    the table has N + 1 rows of D."""
    N = 40
    worst = [0.0, 0.0, 0.0]
    reached = 0
    for kind in SQ.KINDS:
        t = SP.table_inputs(N, D, kind)
        for gap in (None, t["gap"]):
            for d_min in (1, 3):
                ref = SQ.posterior_reference_fast(t["score"], d_min, gap, -1.5)
                reached += ref["log_z"] > NEG
                got = posterior_call(t["score"], d_min, gap, -1.5)
                e = check_posterior(got, ref, N, D, gap is not None, (N, D, kind, gap is not None, d_min))
                worst = [max(a, b) for a, b in zip(worst, e)]
        again = posterior_call(t["score"], 1, t["gap"], -1.5)
        once = posterior_call(t["score"], 1, t["gap"], -1.5, lattice=False, table=False)
        assert torch.equal(_bits(again[3]), _bits(once[3])) and torch.equal(_bits(again[1]), _bits(once[1]))
    print(f"N={N} D={D}: worst lattice error {worst[0]:.2e} of its bar, posteriors {worst[1]:.2e}, identities and "
          f"beta[0] {worst[2]:.2e} of theirs")
    SQ.dump(f"posterior_n{N}d{D}", [dict(N=N, D=D, lattice_over_bar=worst[0], post_over_bar=worst[1],
                                         identities_over_bar=worst[2], reachable=int(reached))])
    assert reached >= 8


@pytest.mark.parametrize("with_gap", (False, True), ids=("nogap", "gap"))
@pytest.mark.parametrize("name", list(SP.TAIL_CASES))
def test_span_posterior_past_the_register_candidates(name, with_gap):
    """Candidate lengths above 1024 come from the loops of the forward sweep's
    two passes and of the backward fold (span_cases.TAIL_CASES; the conditions
    on the reference are asserted in test_spanpost_cpu.py)."""
    t = SP.tail_inputs(name)
    gap = t["gap"] if with_gap else None
    got = posterior_call(t["score"], t["d_min"], gap, 0.0)
    e = check_posterior(got, SQ.tail_posterior(name, with_gap), t["N"], t["D"], with_gap, (name, with_gap))
    print(f"{name} gap={with_gap}: lattice error {e[0]:.2e} of its bar, posteriors {e[1]:.2e}, identities and "
          f"beta[0] {e[2]:.2e} of theirs")


# ----------------------------------------------------------------------------
# 5 / 6. the programme on the span kernel's own output; the order of the three quantities
# ----------------------------------------------------------------------------
KERNEL_CASES = ((70, 37, 17, 1), (70, 16, 17, 65), (70, 37, 1, 1))
"""(N, D, P, F).  The last one guards against a degenerate table: on the float64
reference 87 % of its onset posteriors lie strictly between 1e-3 and 1 - 1e-3
(46 % at P = 17, below the half asked for, hence P = 1; none at F = 65)."""


def _device_tables(N, D, P, F):
    c = SQ.evidence_case(N, D, P, F)
    rc, lse, score, cat = evidence_call(c, **span_buffers(c, SP.PAD_LD))
    assert rc == 0
    return lse[:N + 1, :D], score[:N + 1, :D], cat[:N + 1, :D]      # row-strided views of the padded buffers


@pytest.mark.parametrize("NDPF", KERNEL_CASES, ids=lambda v: "n%dd%dp%df%d" % v)
def test_span_posterior_on_the_span_kernel_output(NDPF):
    from modules import ops
    N, D, P, F = NDPF
    lse, score, cat = _device_tables(*NDPF)
    assert not lse.is_contiguous()
    W = lse.cpu().numpy()
    gap = torch.full((N,), float(np.median(W[np.isfinite(W)])) / 4.0)
    rows = []
    for d_min, g, bonus in ((1, None, 0.0), (3, None, -5.0), (1, gap, 0.0), (2, gap, -2.0)):
        ref = SQ.posterior_reference_fast(W, d_min, None if g is None else g.numpy(), bonus)
        lz, lat, post, tb = ops.span_posterior(lse, d_min, None if g is None else g.cuda(), bonus, True)
        e = check_posterior((0, lz, lat, post, tb), ref, N, D, g is not None, (NDPF, d_min, bonus))
        soft = float(((ref["post"][0][:N] > 1e-3) & (ref["post"][0][:N] < 1 - 1e-3)).mean())
        print(f"N={N} D={D} P={P} F={F} d_min={d_min} gap={'none' if g is None else 'const'} bonus={bonus}: log_z "
              f"{float(lz):.6f}; lattice error {e[0]:.2e} of its bar, posteriors {e[1]:.2e}; {soft:.0%} of the onset "
              f"posteriors strictly between 1e-3 and 1 - 1e-3")
        rows.append(dict(N=N, D=D, P=P, F=F, d_min=d_min, bonus=bonus, gap=g is not None, lattice_over_bar=e[0],
                         post_over_bar=e[1], soft_onsets=soft))
        if (P, F, d_min, bonus) == (1, 1, 1, 0.0) and g is None:
            assert soft > 0.5                           # not a degenerate table: the posteriors really are soft
        lz2, lat2, post2, tb2 = ops.span_posterior(lse, d_min, None if g is None else g.cuda(), bonus, False)
        assert torch.equal(_bits(lz), _bits(lz2)) and torch.equal(_bits(post), _bits(post2)) and tb2.numel() == 0
    SQ.dump("kernel_n%dd%dp%df%d" % NDPF, rows)


def _ordered(lz_sum, lz_best, path, bar, tag):
    print(f"{tag}: log evidence {lz_sum:.6f} (categories summed) >= {lz_best:.6f} (best table) >= {path:.6f} "
          f"(Viterbi path), bar {bar:.1e}")
    assert lz_sum >= lz_best - bar and lz_best >= path - bar, tag
    return dict(case=str(tag), marginal=lz_sum, best_table=lz_best, path=path)


@pytest.mark.parametrize("NDPF", KERNEL_CASES, ids=lambda v: "n%dd%dp%df%d" % v)
def test_evidence_orders_above_the_best_path(NDPF):
    from modules import ops
    N, D, P, F = NDPF
    lse, score, cat = _device_tables(*NDPF)
    rows = []
    gap = torch.full((N,), float(score[torch.isfinite(score)].median()) / 4.0).cuda()
    for d_min, g, bonus in ((1, None, 0.0), (2, gap, -2.0)):
        lz_sum, lat, _, _ = ops.span_posterior(lse, d_min, g, bonus, False)
        lz_best, lat_b, _, _ = ops.span_posterior(score, d_min, g, bonus, False)
        path = ops.span_viterbi(score, cat, d_min, g, bonus, False)[0]
        bar = max(SQ.lattice_bar(N, D, t.cpu().numpy()) for t in (lat, lat_b))
        rows.append(_ordered(float(lz_sum), float(lz_best), float(path), bar, (NDPF, d_min, bonus)))
    SQ.dump("order_n%dd%dp%df%d" % NDPF, rows)


# ----------------------------------------------------------------------------
# 7. the planted recording through segment_posteriors
# ----------------------------------------------------------------------------
def test_planted_recording_through_segment_posteriors():
    from modules import model as M, segmentation
    c = SP.planted()
    N = c["N"]
    dec = M.RNN_Variational_Decoder(SP.PLANT_F, 32, 32, 32).cuda().eval()
    protos = tuple(c[k].cuda() for k in ("mu", "lv", "o"))
    gap = torch.from_numpy(c["gap"]).cuda()
    onsets = np.zeros(N + 1, dtype=bool)
    ends = np.zeros(N + 1, dtype=bool)
    covered = np.zeros(N + 1, dtype=bool)
    for s, d, _ in c["truth"]:
        onsets[s], ends[s + d] = True, True
        covered[s:s + d] = True
    rows = []
    for marginal in (True, False):
        out = segmentation.segment_posteriors(dec, protos, c["x"].cuda(), c["D"], log_weight=c["lw"].cuda(), gap=gap,
                                              marginal=marginal, want_table=True)
        on, en, gp = (out[k].cpu().numpy() for k in ("onset", "end", "gap"))
        assert on.shape == en.shape == gp.shape == (N + 1,) and tuple(out["span"].shape) == (N + 1, c["D"])
        count = float(out["expected_segments"])
        print(f"planted, marginal={marginal}: onsets at the truth >= {on[onsets].min():.6f}, elsewhere <= "
              f"{on[~onsets].max():.1e}; ends >= {en[ends].min():.6f} / <= {en[~ends].max():.1e}; expected segments "
              f"{count:.9f}; log evidence {float(out['log_evidence']):.4f}")
        rows.append(dict(marginal=marginal, onset_true=float(on[onsets].min()), onset_else=float(on[~onsets].max()),
                         end_true=float(en[ends].min()), end_else=float(en[~ends].max()), expected=count))
        assert (on[onsets] > 0.99).all() and (on[~onsets] < 0.01).all()
        assert (en[ends] > 0.99).all() and (en[~ends] < 0.01).all()
        assert (gp[:N][~covered[:N]] > 0.99).all() and (gp[:N][covered[:N]] < 0.01).all() and gp[N] == 0
        assert abs(count - 6.0) <= 1e-6 and len(c["truth"]) == 6
        sp = out["span"].cpu().numpy()
        assert all(sp[s + d, d - 1] > 0.99 for s, d, _ in c["truth"])
    SQ.dump("planted_segment_posteriors", rows)
    with pytest.raises(ValueError):
        segmentation.segment_posteriors(dec, protos, c["x"].cuda(), c["D"], min_length=c["D"] + 1)
    with pytest.raises(ValueError):
        segmentation.segment_posteriors(dec, protos, c["x"].cuda(), c["D"], temperature=0.0)


# ----------------------------------------------------------------------------
# 8. the modules on the small models
# ----------------------------------------------------------------------------
def _small_recording(name, D=12):
    """The recording of test_gpu_span.test_segment_frames_on_small_models: the
    generated mean frames of a few categories, one after another."""
    r = S.small_reference(name)
    _, samp, dec = _small_modules(r)
    K = samp.num_categories
    feats = samp.codebook.detach().t().contiguous()
    spk = None
    if dec.embed_speaker is not None:
        spk = torch.full((K,), int(r["batch"]["speakers"][0]), dtype=torch.int64, device="cuda")
    protos = dec.prototypes(feats, D + 2, speaker=spk)
    lw = torch.log_softmax(torch.linspace(-1.0, 1.0, K), 0).cuda()
    pick = [1, K - 1, 0, K // 2, 1]
    sp = None if spk is None else spk[:len(pick)]
    packed, lengths, _, _ = dec.generate(feats[pick], D, speaker=sp, mean=True, stop_prob=0.5, min_length=2)
    padded, lens = torch.nn.utils.rnn.pad_packed_sequence(packed, batch_first=True)
    padded, lens = padded[packed.unsorted_indices], lens[packed.unsorted_indices.cpu()]
    frames = torch.cat([padded[i, :int(n)] for i, n in enumerate(lens)])
    return dec, protos, lw, frames


@pytest.mark.parametrize("name", list(S.E2E_SMALL))
def test_segment_frames_with_posteriors_on_small_models(name):
    from modules import ops, segmentation
    D = 12
    dec, protos, lw, frames = _small_recording(name, D)
    N = int(frames.shape[0])
    tiled = segmentation.segment_frames(dec, protos, frames, D, log_weight=lw)
    # a background two nats a frame under the tiling's own average: competitive, not dominant
    gap = torch.full((N,), float(tiled["path_score"]) / N - 2.0, device="cuda")
    rows = []
    for g, bonus, d_min in ((None, 0.0, 1), (gap, -3.0, 2)):
        kw = dict(min_length=d_min, log_weight=lw, gap=g, seg_bonus=bonus)
        plain = segmentation.segment_frames(dec, protos, frames, D, **kw)
        both = segmentation.segment_frames(dec, protos, frames, D, posteriors=True, **kw)
        for k in ("onset", "length", "category"):
            assert torch.equal(plain[k], both[k]), k
        assert torch.equal(_bits(plain["score"]), _bits(both["score"]))
        assert torch.equal(_bits(plain["path_score"]), _bits(both["path_score"]))
        assert set(both) - set(plain) >= {"onset_posterior", "offset_posterior", "span_posterior", "log_evidence"}
        # the tables of the one pass, the ordering of the three quantities and the bar
        lse, score, cat = dec.span_evidence(protos, frames, D, log_weight=lw, want_best=True)
        s0, c0 = dec.span_scores(protos, frames, D, log_weight=lw)
        assert torch.equal(_bits(score), _bits(s0)) and torch.equal(cat, c0)
        only, none_s, none_c = dec.span_evidence(protos, frames, D, log_weight=lw)
        assert none_s is None and none_c is None and torch.equal(_bits(only), _bits(lse))
        lz, lat, post, tb = ops.span_posterior(lse, d_min, g, bonus, True)
        lz_b, lat_b, _, _ = ops.span_posterior(score, d_min, g, bonus, False)
        bar = max(SQ.lattice_bar(N, D, t.cpu().numpy()) for t in (lat, lat_b))
        assert torch.equal(_bits(lz), _bits(both["log_evidence"]))
        rows.append(_ordered(float(lz), float(lz_b), float(plain["path_score"]), bar, (name, d_min, bonus)))
        k = len(both["onset"])
        on, off, sp = (both[x].cpu().numpy() for x in ("onset_posterior", "offset_posterior", "span_posterior"))
        assert (k >= 1 or g is not None) and on.shape == off.shape == sp.shape == (k,)
        for v in (on, off, sp, post.cpu().numpy(), tb.cpu().numpy()):
            assert (v >= 0).all() and (v <= 1 + bar).all()
        assert (sp <= np.minimum(on, off) + bar).all()
        end = (both["onset"] + both["length"])
        assert torch.equal(_bits(both["onset_posterior"]), _bits(post[0][both["onset"]]))
        assert torch.equal(_bits(both["offset_posterior"]), _bits(post[1][end]))
        assert torch.equal(_bits(both["span_posterior"]), _bits(tb[end, both["length"] - 1]))
        # a temperature: the operators on the table, the gap and the bonus divided by it
        T = 25.0
        warm = segmentation.segment_frames(dec, protos, frames, D, posteriors=True, temperature=T, **kw)
        lzT, _, postT, tbT = ops.span_posterior(lse / T, d_min, None if g is None else g.double() / T, bonus / T, True)
        assert torch.equal(_bits(warm["log_evidence"]), _bits(lzT))
        assert torch.equal(_bits(warm["onset_posterior"]), _bits(postT[0][both["onset"]]))
        assert torch.equal(_bits(warm["span_posterior"]), _bits(tbT[end, both["length"] - 1]))
        assert torch.equal(warm["onset"], plain["onset"]) and torch.equal(warm["category"], plain["category"])
        full = segmentation.segment_posteriors(dec, protos, frames, D, temperature=T, want_table=True, **kw)
        assert torch.equal(_bits(full["log_evidence"]), _bits(lzT)) and torch.equal(_bits(full["onset"]), _bits(postT[0]))
        assert torch.equal(_bits(full["end"]), _bits(postT[1])) and torch.equal(_bits(full["gap"]), _bits(postT[2]))
        assert torch.equal(_bits(full["span"]), _bits(tbT))
        assert abs(float(full["expected_segments"]) - float(postT[1].sum())) <= 1e-12 * N
        best = segmentation.segment_posteriors(dec, protos, frames, D, marginal=False, **kw)
        assert torch.equal(_bits(best["log_evidence"]), _bits(lz_b)) and "span" not in best
        print(f"{name} d_min={d_min}: N = {N}, {k} segments; onset posteriors {np.round(on, 4).tolist()}, span "
              f"posteriors {np.round(sp, 4).tolist()}; at T = {T:g}: "
              f"{np.round(warm['span_posterior'].cpu().numpy(), 4).tolist()}")
    SQ.dump(f"e2e_{name}", rows)


# ----------------------------------------------------------------------------
# 9. forward-only; segment.py --posteriors on the toy data
# ----------------------------------------------------------------------------
def test_spanpost_ops_are_forward_only():
    from modules import ops
    c = SP.abi_inputs(31, 5, 17, 65)
    T = c["D"] + SP.T_EXTRA
    a = (c["x"].cuda(), c["mu"].reshape(T * 17, 65).cuda(), c["lv"].reshape(T * 17, 65).cuda(),
         c["o"].reshape(-1).cuda(), c["lw"].cuda(), 17, 5)
    lse, ss, sc = ops.span_evidence(*a, True)
    s0, c0 = ops.span_scores(*a)
    assert torch.equal(_bits(ss), _bits(s0)) and torch.equal(sc, c0)
    lse1, e1, e2 = ops.span_evidence(*a, False)
    assert torch.equal(_bits(lse), _bits(lse1)) and tuple(e1.shape) == tuple(e2.shape) == (0, 0)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.span_evidence(a[0].clone().requires_grad_(True), *a[1:], False)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.span_posterior(lse.clone().requires_grad_(True), 1, None, 0.0, False)
    with pytest.raises(ValueError):
        ops.span_evidence(a[0], a[1], a[2], a[3], a[4], 17, T + 1, False)   # a rectangle shorter than D
    with pytest.raises(ValueError):
        ops.span_evidence(a[0], a[1], a[2], a[3], a[4][:5], 17, 5, False)
    with pytest.raises(ValueError):
        ops.span_posterior(lse, 6, None, 0.0, False)
    with pytest.raises(ValueError):
        ops.span_posterior(lse, 1, torch.zeros(5).cuda(), 0.0, False)


def test_segment_cli_posteriors_on_toy_data(tmp_path):
    import segment
    plain = os.path.join(str(tmp_path), "a", "segmented.csv")
    post = os.path.join(str(tmp_path), "b", "segmented.csv")
    rec = os.path.join(str(tmp_path), "b", "recordings.csv")
    cdir = os.path.join(str(tmp_path), "b", "curves")
    base = [CKPT, TOY, ANN, "1.0", "--max_length", "60", "--min_length", "3"]
    segment.main(base + ["-S", plain])
    segment.main(base + ["-S", post, "--posteriors", "--posterior_temperature", "50", "--curves_dir", cdir,
                         "--recordings_out", rec])
    a, b = pd.read_csv(plain), pd.read_csv(post)
    assert list(a.columns) == list(segment.COLUMNS)
    assert list(b.columns) == list(segment.COLUMNS) + list(segment.POSTERIOR_COLUMNS)
    with open(plain) as f, open(post) as h:             # the first nine columns: the same text
        for la, lb in zip(f.read().splitlines(), h.read().splitlines()):
            assert lb.startswith(la + ",")
    assert len(a) == len(b) >= 1
    for k in segment.POSTERIOR_COLUMNS:
        assert ((b[k] >= 0) & (b[k] <= 1 + 1e-9)).all(), k
    assert (b["span_posterior"] <= np.minimum(b["onset_posterior"], b["offset_posterior"]) + 1e-9).all()
    wav = pd.read_csv(ANN)["input_path"][0]
    fs, wave = segment.read_wave(TOY, wav)
    frame, hop = int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))
    n_frames = segment.num_frames(len(wave), frame, hop)
    r = pd.read_csv(rec)
    assert list(r.columns) == list(segment.RECORDING_COLUMNS) and len(r) == 1 and r["input_path"][0] == wav
    assert int(r["n_frames"][0]) == n_frames and int(r["n_segments"][0]) == len(b)
    assert abs(float(r["path_score"][0]) - float(a["segment_score"].sum())) <= 1e-9 * abs(float(r["path_score"][0]))
    files = os.listdir(cdir)
    assert files == [os.path.basename(segment.curve_path(cdir, wav))]
    with np.load(os.path.join(cdir, files[0])) as z:
        assert z["onset"].shape == z["end"].shape == z["gap"].shape == (n_frames + 1,)
        assert int(z["fs"]) == fs and int(z["hop"]) == hop
        assert float(z["log_evidence"]) == float(r["log_evidence"][0])
        assert abs(float(z["end"].sum()) - float(r["expected_segments"][0])) <= 1e-9 * n_frames
        assert not z["gap"].any()                       # no gap model: the segments tile the recording
    print(f"segment.py --posteriors at T = 50: {len(b)} segments over {n_frames} frames, expected "
          f"{float(r['expected_segments'][0]):.2f}; span posteriors {b['span_posterior'].min():.3f} .. "
          f"{b['span_posterior'].max():.3f}; log evidence {float(r['log_evidence'][0]):.2f}, tempered path "
          f"{float(r['path_score'][0]) / 50:.2f}")
    # at temperature 1 the evidence is the model's own and bounds the best path
    rec1 = os.path.join(str(tmp_path), "c", "recordings.csv")
    segment.main(base + ["-S", os.path.join(str(tmp_path), "c", "segmented.csv"), "--posteriors", "--recordings_out",
                         rec1])
    r1 = pd.read_csv(rec1)
    assert float(r1["log_evidence"][0]) >= float(r1["path_score"][0])
    assert pd.read_csv(os.path.join(str(tmp_path), "c", "segmented.csv"))[list(segment.COLUMNS)].equals(a)
