"""Pairwise scoring on the GPU: ``abcd_pairwise_nll`` and ``abcd_pair_posterior``
through the C ABI, ``RNN_Variational_Decoder.prototypes`` / ``score_against``
end to end and the ``classify.py`` CLI, against the float64 references of
``pairwise_cases.py``.

Bars (``pairwise_cases.py``): every ``pair_em`` within 1e-4 of its unit
``A[b, p]`` (the float64 sum of the absolute values of its terms), every
``pair_off`` within 1e-4 of its own value; against ``abcd_segment_losses`` on
prototype p expanded to the packed layout within ``(F + 4) 2^-23 A[b, p]``
(``cross_bar``); ``log_evidence`` within ``2^-22 max(|ref|, 1)``, ``resp`` and
``best_prob`` within 1e-5 absolute; end to end ``edge_cases.rel_err`` < 1e-4
against ``score(mean=True)`` on the category's features repeated and against
the float64 oracle.  Every observed figure is printed (``-rA``) and kept with
``ABCD_PARITY_DUMP`` (profiles/pairwise_errors.json).
"""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import edge_cases as E
import pairwise_cases as PW
import score_cases as S
from test_gpu_score import ANN, CKPT, GOLDEN, TOY, _bench_modules, _bits, _one_segment, _rows, _small_modules, seg_call

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -7.0  # what the outputs hold before a call


# ----------------------------------------------------------------------------
# 1. abcd_pairwise_nll through ctypes
# ----------------------------------------------------------------------------
def _rect(t, ld, extra=PW.T_EXTRA, tail=2):
    """A T x P (x F) prototype tensor on the device as the time-major rectangle
    the kernel reads, ``extra`` steps longer, in a buffer of row stride ld with
    ``tail`` more rows: padding columns, the extra steps and the tail are NaN."""
    T, P = t.shape[:2]
    rows = (T + extra) * P
    if t.dim() == 2:
        buf = torch.full((rows + tail,), NAN)
        buf[:T * P] = t.reshape(-1)
    else:
        buf = torch.full((rows + tail, ld), NAN)
        buf[:T * P, :t.shape[2]] = t.reshape(T * P, -1)
    return buf.cuda()


def pair_call(c, gt, y, mu, ldm, lv, ldl, o, want=("em", "off"), ws="auto", pad=1, **over):
    """abcd_pairwise_nll -> (rc, em, off): B x (P + pad) buffers holding SENT
    before the call (None when not asked for); ``over`` replaces arguments."""
    from modules import _native as N
    lib = N.lib()
    a = dict(bs=c["batch_sizes"], L=c["L"], B=c["B"], F=c["F"], P=c["P"], Tp=c["T"] + PW.T_EXTRA, T=None)
    a.update(over)
    bs = torch.as_tensor(np.asarray(a["bs"]), dtype=torch.int64).contiguous()
    pk = N.Packed()
    pk.data = None if gt is None else gt.data_ptr()
    pk.batch_sizes = bs.data_ptr()
    pk.T, pk.L, pk.B, pk.F = (int(bs.numel()) if a["T"] is None else a["T"]), int(a["L"]), int(a["B"]), int(a["F"])
    ldp = a.get("ldp", c["P"] + pad)
    em = torch.full((c["B"], c["P"] + pad), SENT, device="cuda") if "em" in want else None
    off = torch.full((c["B"], c["P"] + pad), SENT, device="cuda") if "off" in want else None
    if ws == "auto":
        ws = N.workspace(lib.abcd_pairwise_nll_workspace_bytes(pk.T, pk.B, c["P"]), "cuda")
        ws.fill_(0xFF)  # NaN partials: a slice that is read without having been written shows
    rc = lib.abcd_pairwise_nll(pk, N.ptr(y), a["P"], a["Tp"], N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(o), N.ptr(em),
                               N.ptr(off), ldp, N.ptr(ws), 0 if ws is None else ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, em, off


def _buffers(c, ld):
    return dict(gt=_rows(c["gt"], c["F"]), y=_rows(c["y"], 1), mu=_rect(c["mu"], ld), ldm=ld, lv=_rect(c["lv"], ld),
                ldl=ld, o=_rect(c["o"], 1))


@pytest.mark.parametrize("P", PW.ABI_P)
@pytest.mark.parametrize("F", PW.ABI_F)
@pytest.mark.parametrize("shape", list(PW.ABI_SHAPES))
def test_pairwise_nll_abi(shape, F, P):
    from modules import _native as N
    c = PW.abi_inputs(shape, F, P)
    ref, bs, L, B, T = c["ref"], c["batch_sizes"], c["L"], c["B"], c["T"]
    rows = []
    for ld in (F, PW.PAD_LD):
        b = _buffers(c, ld)
        N.lib().abcd_dispatch_reset()
        rc, em, off = pair_call(c, **b)
        assert rc == 0
        kern, count = N.dispatch()["pair_nll"]
        assert count == 1 and kern == f"pair_nll<32x32x16> grid {-(-P // 32)}x{-(-B // 32)}x{-(-T // 16)}", kern
        assert (em[:, P:] == SENT).all() and (off[:, P:] == SENT).all()  # columns >= P of a wider row are not written
        e_em = np.abs(em[:, :P].double().cpu().numpy() - ref["em"]) / ref["A"]
        e_off = np.abs(off[:, :P].double().cpu().numpy() - ref["off"]) / ref["off"]
        # against the per-segment kernel on each prototype expanded to the packed layout
        e_x = 0.0
        for p in range(P):
            m1, v1, o1 = PW.expand_prototype(bs, p, c["mu"], c["lv"], c["o"])
            rc, sem, soff, _ = seg_call(bs, L, B, F, b["gt"], _rows(m1, ld), ld, _rows(v1, ld), ld, _rows(o1, 1),
                                        b["y"])
            assert rc == 0
            d = np.abs(em[:, p].double().cpu().numpy() - sem.double().cpu().numpy()) / ref["A"][:, p]
            e_x = max(e_x, float(d.max()))
            assert np.abs(off[:, p].double().cpu().numpy() - soff.double().cpu().numpy()).max() <= \
                2.0 ** -22 * ref["off"][:, p].max()  # the same fp32 terms in fp64: a rounding of each result
        print(f"{shape} F={F} P={P} ld={ld}: worst |pair - ref| / unit  em {e_em.max():.2e}  off {e_off.max():.2e}; "
              f"|pair_em - seg_em| / A {e_x:.2e} (bar {PW.cross_bar(F):.2e})")
        rows.append(dict(shape=shape, F=F, P=P, ld=ld, em=float(e_em.max()), off=float(e_off.max()), vs_seg=e_x))
        assert np.isfinite(e_em).all() and np.isfinite(e_off).all()
        assert e_em.max() <= PW.BAR and e_off.max() <= PW.BAR
        assert e_x <= PW.cross_bar(F)
        # a second call: bit for bit
        rc, em2, off2 = pair_call(c, **b)
        assert rc == 0 and torch.equal(_bits(em), _bits(em2)) and torch.equal(_bits(off), _bits(off2))
        # each output NULL in turn (and without its inputs): the other keeps its bits
        rc, a, o2 = pair_call(c, **b, want=("em",))
        assert rc == 0 and o2 is None and torch.equal(_bits(a), _bits(em))
        rc, a, o2 = pair_call(c, **dict(b, y=None, o=None), want=("em",))
        assert rc == 0 and torch.equal(_bits(a), _bits(em))
        rc, a, o2 = pair_call(c, **b, want=("off",))
        assert rc == 0 and a is None and torch.equal(_bits(o2), _bits(off))
        rc, a, o2 = pair_call(c, **dict(b, gt=None, mu=None, lv=None), want=("off",))
        assert rc == 0 and torch.equal(_bits(o2), _bits(off))
        # an exact-width output (ld_pair = P) holds the same bits
        rc, a, o2 = pair_call(c, **b, pad=0)
        assert rc == 0 and torch.equal(_bits(a), _bits(em[:, :P].contiguous()))
        assert torch.equal(_bits(o2), _bits(off[:, :P].contiguous()))
        if ld != PW.PAD_LD:
            continue
        # nothing outside a prototype's rows is read: with every other prototype NaN, column p keeps its bits
        pcol = torch.arange((T + PW.T_EXTRA) * P + 2) % P
        for p in range(P):
            keep = (pcol == p).cuda()

            def only(t):
                return torch.where(keep if t.dim() == 1 else keep[:, None], t, torch.full_like(t, NAN))
            rc, a, o2 = pair_call(c, **dict(b, mu=only(b["mu"]), lv=only(b["lv"]), o=only(b["o"])))
            assert rc == 0
            assert torch.equal(_bits(a[:, p]), _bits(em[:, p])) and torch.equal(_bits(o2[:, p]), _bits(off[:, p])), p
            assert torch.isnan(a[:, :P]).sum() == B * (P - 1) and torch.isnan(o2[:, :P]).sum() == B * (P - 1)
        # nor outside a segment's rows
        if shape in PW.NAN_SHAPES:
            seg_of = torch.from_numpy(S.segment_of_rows(bs))
            for s in range(B):
                keep2 = torch.cat([seg_of == s, torch.zeros(2, dtype=torch.bool)]).cuda()

                def mine(t):
                    return torch.where(keep2 if t.dim() == 1 else keep2[:, None], t, torch.full_like(t, NAN))
                rc, a, o2 = pair_call(c, **dict(b, gt=mine(b["gt"]), y=mine(b["y"])))
                assert rc == 0
                assert torch.equal(_bits(a[s]), _bits(em[s])) and torch.equal(_bits(o2[s]), _bits(off[s])), s
                assert torch.isnan(a[:, :P]).sum() == (B - 1) * P
    assert N.lib().abcd_device_status() == 0
    PW.dump(f"abi_{shape}_F{F}_P{P}", rows)


def test_pairwise_nll_abi_rejects_bad_arguments():
    from modules import _native as N
    c = PW.abi_inputs("ties", 65, 17)
    F, P, T = 65, 17, c["T"]
    b = _buffers(c, F)

    def refused(**kw):
        over = {k: kw.pop(k) for k in list(kw) if k in ("bs", "L", "B", "P", "Tp", "T", "ldp")}
        rc, em, off = pair_call(c, **dict(b, **kw), **over)
        assert rc == N.ABCD_EINVAL == 1000, (kw.keys(), over, rc)
        assert (em == SENT).all() and (off == SENT).all()  # nothing written

    assert pair_call(c, **b)[0] == 0
    bs = c["batch_sizes"]
    up = bs.copy()
    up[2], up[3] = bs[3], bs[2]
    assert not (np.diff(up) <= 0).all() and up.sum() == c["L"]
    refused(bs=up)
    refused(B=c["B"] - 1)
    refused(L=c["L"] + 1)
    refused(P=0)
    refused(Tp=T - 1)
    refused(ldm=F - 1)
    refused(ldl=F - 1)
    refused(ldp=P - 1)
    refused(gt=None)
    refused(mu=None)
    refused(lv=None)
    refused(y=None)
    refused(o=None)
    refused(ws=None)
    refused(ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    assert N.lib().abcd_device_status() == 0


# ----------------------------------------------------------------------------
# 2. abcd_pair_posterior through ctypes
# ----------------------------------------------------------------------------
def post_call(em, off, lw, ld=None, want=("ev", "best", "bp", "resp")):
    from modules import _native as N
    B, P = em.shape
    ld = P if ld is None else ld

    def wide(t):
        if t is None:
            return None
        buf = torch.full((B, ld), NAN)
        buf[:, :P] = t
        return buf.cuda()
    emd, offd, lwd = wide(em), wide(off), None if lw is None else lw.cuda()
    ev = torch.full((B,), SENT, device="cuda") if "ev" in want else None
    best = torch.full((B,), -7, dtype=torch.int32, device="cuda") if "best" in want else None
    bp = torch.full((B,), SENT, device="cuda") if "bp" in want else None
    resp = torch.full((B, P + 1), SENT, device="cuda") if "resp" in want else None
    rc = N.lib().abcd_pair_posterior(N.ptr(emd), N.ptr(offd), ld, B, P, N.ptr(lwd), N.ptr(ev), N.ptr(best), N.ptr(bp),
                                     N.ptr(resp), P + 1, N.stream())
    torch.cuda.synchronize()
    return rc, ev, best, bp, resp


@pytest.mark.parametrize("P", PW.POST_P)
@pytest.mark.parametrize("B", PW.POST_B)
def test_pair_posterior_abi(B, P):
    from modules import _native as N
    c = PW.posterior_inputs(B, P)
    ref = c["ref"]
    N.lib().abcd_dispatch_reset()
    rc, ev, best, bp, resp = post_call(c["em"], c["off"], c["lw"], ld=P + 3)
    assert rc == 0 and N.dispatch()["pair_post"] == (f"pair_posterior<{P}> grid {-(-B // 4)}", 1)
    assert best.cpu().tolist() == ref["best"].tolist()  # every row: the cases' top-two gap is >= 0.5
    e_ev = np.abs(ev.double().cpu().numpy() - ref["log_evidence"]) / np.maximum(np.abs(ref["log_evidence"]), 1.0)
    e_r = np.abs(resp[:, :P].double().cpu().numpy() - ref["resp"]).max()
    e_bp = np.abs(bp.double().cpu().numpy() - ref["best_prob"]).max()
    e_sum = np.abs(resp[:, :P].double().sum(1).cpu().numpy() - 1.0).max()
    print(f"posterior B={B} P={P}: log_evidence {e_ev.max():.2e} (bar {PW.LOGEV_BAR:.2e}), resp {e_r:.2e}, "
          f"best_prob {e_bp:.2e}, |sum resp - 1| {e_sum:.2e} (bar {PW.RESP_BAR:.0e})")
    PW.dump(f"post_B{B}_P{P}", [dict(B=B, P=P, log_evidence=float(e_ev.max()), resp=float(e_r),
                                     best_prob=float(e_bp), resp_sum=float(e_sum))])
    assert e_ev.max() <= PW.LOGEV_BAR
    assert e_r <= PW.RESP_BAR and e_bp <= PW.RESP_BAR and e_sum <= PW.RESP_BAR
    assert (resp[:, P] == SENT).all()
    assert torch.equal(bp, resp[torch.arange(B), best.long()])
    # a second call, each output alone, and absent terms: NULL counts as 0
    rc, ev2, best2, bp2, resp2 = post_call(c["em"], c["off"], c["lw"], ld=P + 3)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in ((ev, ev2), (bp, bp2), (resp, resp2)))
    assert torch.equal(best, best2)
    for k, full in (("ev", ev), ("best", best), ("bp", bp), ("resp", resp)):
        out = dict(zip(("ev", "best", "bp", "resp"), post_call(c["em"], c["off"], c["lw"], want=(k,))[1:]))
        assert torch.equal(out[k], full) and all(v is None for n, v in out.items() if n != k)
    rc, ev0, best0, _, _ = post_call(c["em"], None, None)
    ref0 = PW.posterior_reference(c["em"])
    assert rc == 0 and best0.cpu().tolist() == ref0["best"].tolist()
    assert (np.abs(ev0.double().cpu().numpy() - ref0["log_evidence"])
            <= PW.LOGEV_BAR * np.abs(ref0["log_evidence"])).all()
    rc, evz, _, _, _ = post_call(c["em"], torch.zeros(B, P), torch.zeros(P))
    assert torch.equal(_bits(ev0), _bits(evz))


def test_pair_posterior_ties_and_exclusions():
    inf = float("inf")
    em = torch.tensor([[5e4 + 3.0, 5e4 + 1.0, 5e4 + 1.0, 5e4 + 2.0],     # a two-way tie: the lowest index wins
                       [NAN, 7.0, inf, 7.5],                               # a NaN and a +inf NLL
                       [1.0, 2.0, 3.0, 4.0],                               # weights: NaN on 0, -inf on 3
                       [NAN, inf, NAN, inf],                               # nothing left
                       [2.0, 2.0, 2.0, 2.0]])
    lw = torch.zeros(4)
    rc, ev, best, bp, resp = post_call(em, None, lw)
    ref = PW.posterior_reference(em, None, lw)
    assert rc == 0 and best.cpu().tolist() == ref["best"].tolist() == [1, 1, 0, -1, 0]
    r = resp[:, :4].double().cpu().numpy()
    assert np.abs(r - ref["resp"]).max() <= PW.RESP_BAR
    assert r[1, 0] == 0.0 and r[1, 2] == 0.0 and (r[3] == 0.0).all()       # excluded: exactly 0
    assert ev[3].item() == -inf and bp[3].item() == 0.0
    assert abs(r[0, 1] - r[0, 2]) == 0.0 and abs(ev[4].item() - (-2.0 + np.log(4.0))) <= 1e-6
    lw2 = torch.tensor([NAN, 0.0, 0.0, -inf])
    rc, ev, best, bp, resp = post_call(em, torch.zeros(5, 4), lw2)
    ref = PW.posterior_reference(em, None, lw2)
    r = resp[:, :4].double().cpu().numpy()
    assert best.cpu().tolist() == ref["best"].tolist() == [1, 1, 1, -1, 1]
    assert (r[:, 0] == 0.0).all() and (r[:, 3] == 0.0).all() and np.abs(r - ref["resp"]).max() <= PW.RESP_BAR
    fin = np.isfinite(ref["log_evidence"])
    assert np.abs(ev.double().cpu().numpy()[fin] - ref["log_evidence"][fin]).max() <= \
        PW.LOGEV_BAR * np.abs(ref["log_evidence"][fin]).max()
    from modules import _native as N
    assert N.lib().abcd_device_status() == 0


# ----------------------------------------------------------------------------
# 3. the operators
# ----------------------------------------------------------------------------
def test_pairwise_ops():
    from modules import ops
    c = PW.abi_inputs("b33t9", 65, 17)
    F, P, T, ref = 65, 17, c["T"], c["ref"]
    bs = torch.from_numpy(c["batch_sizes"])
    gt, y = c["gt"].cuda(), c["y"].cuda()
    mu, lv, o = (c[k].cuda().reshape(T * P, -1) for k in ("mu", "lv", "o"))
    with torch.no_grad():
        em, off = ops.pairwise_nll(gt, bs, y, mu, lv, o.reshape(-1), P, F)
    assert em.shape == off.shape == (c["B"], P)
    assert (np.abs(em.double().cpu().numpy() - ref["em"]) / ref["A"]).max() <= PW.BAR
    assert (np.abs(off.double().cpu().numpy() - ref["off"]) / ref["off"]).max() <= PW.BAR
    # row-strided views (a padded stash) pass without a copy and give the same bits
    wide = [torch.full((T * P, PW.PAD_LD), NAN, device="cuda") for _ in range(2)]
    wide[0][:, :F], wide[1][:, :F] = mu, lv
    em2, off2 = ops.pairwise_nll(gt, bs, y, wide[0][:, :F], wide[1][:, :F], o.reshape(-1), P, F)
    assert torch.equal(_bits(em), _bits(em2)) and torch.equal(_bits(off), _bits(off2))
    # one half only: the other is zeros
    em3, off3 = ops.pairwise_nll(gt, bs, None, mu, lv, None, P, F)
    assert torch.equal(_bits(em), _bits(em3)) and not off3.any()
    # forward-only
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.pairwise_nll(gt, bs, y, mu.clone().requires_grad_(True), lv, o.reshape(-1), P, F)
    with pytest.raises(ValueError):
        ops.pairwise_nll(gt, bs, y, mu[:-1], lv[:-1], o.reshape(-1)[:-1], P, F)  # not a whole rectangle
    with pytest.raises(ValueError):
        ops.pairwise_nll(gt, bs, y, mu[:P], lv[:P], o.reshape(-1)[:P], P, F)     # shorter than the batch
    with pytest.raises(RuntimeError):
        ops.pairwise_nll(c["gt"], bs, c["y"], mu.cpu(), lv.cpu(), o.reshape(-1).cpu(), P, F)  # CPU tensors
    lw = torch.randn(P, generator=torch.Generator().manual_seed(1)).cuda()
    ev, best, bp, resp = ops.pair_posterior(em, off, lw)
    want = PW.posterior_reference(em.cpu(), off.cpu(), lw.cpu())
    assert best.dtype == torch.int32 and best.cpu().tolist() == want["best"].tolist()
    assert np.abs(resp.double().cpu().numpy() - want["resp"]).max() <= PW.RESP_BAR
    assert (np.abs(ev.double().cpu().numpy() - want["log_evidence"])
            <= PW.LOGEV_BAR * np.maximum(np.abs(want["log_evidence"]), 1.0)).all()
    # a strided view of a wider matrix, the posterior of its first 9 columns
    ev9, best9, _, resp9 = ops.pair_posterior(em[:, :9], off[:, :9], lw[:9])
    want9 = PW.posterior_reference(em[:, :9].cpu(), off[:, :9].cpu(), lw[:9].cpu())
    assert resp9.shape == (c["B"], 9) and best9.cpu().tolist() == want9["best"].tolist()
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.pair_posterior(em.clone().requires_grad_(True), off, lw)


def test_expected_log_prior():
    from modules import model as M
    for K, a0, n in ((16, 1.0, 100.0), (128, 0.5, float(S.N_DATA))):
        torch.manual_seed(K)
        samp = M.ABCDSampler(32, 32, K, 32, prior_concentration=a0).cuda()
        got = samp.expected_log_prior(n)
        psl = samp.posterior_shape_logits.detach().double().cpu()
        alpha = torch.softmax(psl, -1) * n + a0
        want = torch.digamma(alpha) - torch.digamma(alpha.sum())
        e = float((got.double().cpu() - want).abs().max() / want.abs().max())
        print(f"expected_log_prior K={K}: rel {e:.2e}")
        assert got.shape == (K,) and got.dtype == torch.float32 and e < 1e-5  # alpha is formed in fp32


# ----------------------------------------------------------------------------
# 4. prototypes() / score_against() end to end
# ----------------------------------------------------------------------------
def _columns(samp, dec, batch, categories):
    """(features P x D, speakers P or None, categories P, speakers P as lists):
    speaker-major over the speakers present in the batch."""
    cats = torch.as_tensor(categories, dtype=torch.int64)
    code = samp.codebook.detach().t()[cats.cuda()].contiguous()
    if dec.embed_speaker is None:
        return code, None, cats.tolist(), None
    present = torch.unique(batch["speakers"]).tolist()
    spk = torch.tensor(present, dtype=torch.int64).repeat_interleave(len(cats))
    return code.repeat(len(present), 1), spk.cuda(), cats.tolist() * len(present), spk.tolist()


@pytest.mark.parametrize("name", list(PW.E2E_SMALL) + ["edge"])
def test_score_against_end_to_end(name):
    from modules import _native as N
    if name == "edge":
        r = S.edge_reference(*PW.E2E_EDGE)
        _, samp, dec = _bench_modules(r)
        K = r["cfg"]["K"]
        cats = list(range(0, K, K // PW.E2E_EDGE_CATEGORIES))[:PW.E2E_EDGE_CATEGORIES]
    else:
        r = S.small_reference(name)
        _, samp, dec = _small_modules(r)
        cats = list(range(samp.num_categories))
    batch = r["batch"]
    bsz = batch["batch_sizes"]
    B, T = int(bsz[0]), int(bsz.numel())
    data, is_off = batch["data"].cuda(), batch["is_offset"].cuda()
    feats, spk, col_cat, col_spk = _columns(samp, dec, batch, cats)
    P = feats.shape[0]
    N.lib().abcd_dispatch_reset()
    protos = dec.prototypes(feats, T, speaker=spk)
    em, off, lengths = dec.score_against(protos, bsz, data, is_off)
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    ran = N.dispatch()
    print(name, f"P = {P}", "dec_fwd:", ran["dec_fwd"], "| pair_nll:", ran["pair_nll"])
    assert ran["pair_nll"][1] == 1 and ran["dec_fwd"][1] == 1  # one P-row decode, one pairwise call
    assert em.shape == off.shape == (B, P) and lengths.dtype == torch.int64
    assert lengths.cpu().tolist() == list(S.lengths_of(bsz.numpy()))
    assert tuple(protos[0].shape) == (T, P, data.shape[1]) and tuple(protos[2].shape) == (T, P)
    assert dec.score_against(protos, bsz, data)[1] is None  # no offset targets: no BCE
    rows = []
    # every column against score() on that category's features repeated, mean fed back
    w_em = w_off = 0.0
    for p in range(P):
        sp = None if spk is None else spk[p].repeat(B)
        e1, o1, _ = dec.score(feats[p:p + 1].repeat(B, 1), bsz, speaker=sp, ground_truth_out=data,
                              ground_truth_offset=is_off, mean=True)
        w_em, w_off = max(w_em, E.rel_err(em[:, p], e1)), max(w_off, E.rel_err(off[:, p], o1))
    print(f"{name}: worst column against score(): em {w_em:.2e} off {w_off:.2e}")
    rows.append(dict(case=name, against="score", em=w_em, off=w_off))
    assert w_em < PW.BAR and w_off < PW.BAR
    # against the float64 oracle
    want = PW.oracle_pairwise(r["P"], r["ocfg"], batch, col_cat, col_spk)
    o_em, o_off = E.rel_err(em, torch.from_numpy(want["em"])), E.rel_err(off, torch.from_numpy(want["off"]))
    c_em = max(E.rel_err(em[:, p], torch.from_numpy(want["em"][:, p])) for p in range(P))
    u_em = float((np.abs(em.double().cpu().numpy() - want["em"]) / want["A"]).max())
    print(f"{name}: against the float64 oracle: em {o_em:.2e} (worst column {c_em:.2e}, of the unit {u_em:.2e}) "
          f"off {o_off:.2e}")
    rows.append(dict(case=name, against="oracle64", em=o_em, em_column=c_em, em_unit=u_em, off=o_off))
    assert o_em < PW.BAR and o_off < PW.BAR and c_em < PW.BAR and u_em < PW.BAR
    # a segment scored alone gets its in-batch row (pairs are independent)
    for b in sorted({0, B // 2, B - 1}):
        one = _one_segment(batch, b)
        e1, o1, l1 = dec.score_against(protos, one["batch_sizes"], one["data"].cuda(), one["is_offset"].cuda())
        assert l1.tolist() == [int(lengths[b])]
        d_em = float((e1[0] - em[b]).abs().max() / em.abs().max())
        d_off = float((o1[0] - off[b]).abs().max() / off.abs().max())
        print(f"{name} segment {b} alone: em {d_em:.2e} off {d_off:.2e}")
        rows.append(dict(case=name, against=f"alone{b}", em=d_em, off=d_off))
        assert d_em < PW.BAR and d_off < PW.BAR
    # a longer rectangle agrees on the common steps bit for bit, and serves the batch as well
    longer = dec.prototypes(feats, T + 3, speaker=spk)
    for a, l in zip(protos, longer):
        assert l.shape[0] == T + 3 and torch.equal(_bits(a), _bits(l[:T]))
    em_l, off_l, _ = dec.score_against(longer, bsz, data, is_off)
    assert torch.equal(_bits(em), _bits(em_l)) and torch.equal(_bits(off), _bits(off_l))
    with pytest.raises(ValueError):
        dec.score_against(tuple(t[:T - 1] for t in protos), bsz, data, is_off) if T > 1 else \
            dec.score_against((protos[0][0], protos[1][0], protos[2][0]), bsz, data, is_off)
    PW.dump(f"e2e_{name}", rows)


# ----------------------------------------------------------------------------
# 5. classify.py on the toy data with the reference's small checkpoint
# ----------------------------------------------------------------------------
def _oracle_matrix():
    """Float64 oracle tables of the toy segments by data_ix (the CLI's loader,
    -b 4): em, A, off (n x K), the Dirichlet log weights and the lengths."""
    from modules import data_utils
    from modules.data_utils import Compose
    ck = torch.load(CKPT, map_location="cpu", weights_only=True)
    P, ocfg = S.checkpoint_oracle(ck)
    K = ocfg["K"]
    parser = data_utils.Data_Parser(TOY, ANN)
    fs = parser.get_sample_freq()
    tfm = Compose([data_utils.ToTensor(), data_utils.STFT(int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))),
                   data_utils.Transform(lambda x: (x + 2 ** -15).log() / 1.0)])
    ds = parser.get_data(transform=tfm)
    n = len(ds)
    out = {k: np.zeros((n, K)) for k in ("em", "A", "off")}
    out["length"] = np.zeros(n)
    for packed, is_offset, speaker, ixs in data_utils.DataLoader(ds, batch_size=4):
        sc = PW.oracle_pairwise(P, ocfg, dict(data=packed.data, batch_sizes=packed.batch_sizes,
                                              is_offset=is_offset.data), list(range(K)), None)
        ix = np.asarray(ixs)
        for k in ("em", "A", "off"):
            out[k][ix] = sc[k]
        out["length"][ix] = sc["lengths"]
    psl = P["feature_sampler/posterior_shape_logits"].double()
    alpha = torch.softmax(psl, -1) * n + float(P["feature_sampler/prior_concentration"])
    out["lw"] = (torch.digamma(alpha) - torch.digamma(alpha.sum())).numpy()
    return out


def test_classify_cli_on_toy_data(tmp_path):
    import classify
    z = np.load(os.path.join(GOLDEN, "ref_ckpt_small_encode.npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    base = [CKPT, TOY, ANN, "1.0", "-b", "4"]
    out = os.path.join(str(tmp_path), "c", "classified.csv")
    mat = os.path.join(str(tmp_path), "c", "matrix.csv")
    assert classify.main(base + ["-S", out, "--matrix", mat]) == out
    df, lt = pd.read_csv(out), pd.read_csv(mat)
    n, K = z["probs"].shape
    assert list(df.columns) == list(classify.COLUMNS) + meta["annotation_columns"]
    assert list(lt.columns) == list(classify.MATRIX_COLUMNS) + meta["annotation_columns"]
    assert len(df) == n and sorted(df["data_ix"].tolist()) == list(range(n)) and len(lt) == n * K
    assert df["data_ix"].tolist()[:4] == list(z["row_order"][:4])  # encode.py's first batch at -b 4, in its order
    ix = df["data_ix"].to_numpy()
    assert (df["category_ix"].to_numpy() == z["argmax"][ix]).all()
    assert np.abs(df["category_prob"].to_numpy() - z["probs"][ix].max(1)).max() <= 1e-5
    # the long table is category-major within a batch of 4, as encode.py orders its rows
    assert lt["data_ix"].tolist()[:4 * K] == df["data_ix"].tolist()[:4] * K
    assert lt["category_ix"].tolist()[:4 * K] == [k for k in range(K) for _ in range(4)]
    want = _oracle_matrix()
    assert df["length"].tolist() == want["length"][ix].astype(int).tolist()
    li, lk = lt["data_ix"].to_numpy(), lt["category_ix"].to_numpy()
    em, off, lw = lt["emission_nll"].to_numpy(), lt["end_prediction_loss"].to_numpy(), lt["log_weight"].to_numpy()
    e_em = np.abs(em - want["em"][li, lk])
    e_off = np.abs(off - want["off"][li, lk])
    print(f"classify.py emission_nll: rel_err {e_em.max() / np.abs(want['em']).max():.2e}, of the unit "
          f"{(e_em / want['A'][li, lk]).max():.2e}; end_prediction_loss rel_err "
          f"{e_off.max() / want['off'].max():.2e}, of its value {(e_off / want['off'][li, lk]).max():.2e}")
    assert e_em.max() < S.BAR * np.abs(want["em"]).max() and (e_em <= S.BAR * want["A"][li, lk]).all()
    assert e_off.max() < S.BAR * want["off"].max() and (e_off <= S.BAR * want["off"][li, lk]).all()
    assert np.abs(lw - want["lw"][lk]).max() <= 1e-5 * np.abs(want["lw"]).max()
    resp = lt.groupby("data_ix")["responsibility"].sum()
    assert np.abs(resp.to_numpy() - 1.0).max() <= PW.RESP_BAR and len(resp) == n
    # the evidence and the chosen category against the oracle's scores
    total = want["em"] + want["off"] - want["lw"][None, :]          # n x K: what the posterior minimises
    unit = want["A"] + want["off"] + np.abs(want["lw"])[None, :]
    ev = PW.posterior_reference(want["em"], want["off"], want["lw"])["log_evidence"]
    e_ev = np.abs(df["log_evidence"].to_numpy() - ev[ix])
    chosen = df["decoder_category_ix"].to_numpy()
    over = (total[ix, chosen] - total[ix].min(1)) / unit[ix, chosen]
    gap = np.sort(total, 1)
    print(f"classify.py log_evidence: rel_err {e_ev.max() / np.abs(ev).max():.2e}, of the unit "
          f"{(e_ev / unit[ix].min(1)).max():.2e}; chosen category over the oracle minimum {over.max():.2e} of its "
          f"unit (oracle top-two gaps {((gap[:, 1] - gap[:, 0]) / unit.min(1)).min():.1e} .. "
          f"{((gap[:, 1] - gap[:, 0]) / unit.min(1)).max():.1e})")
    assert e_ev.max() < S.BAR * np.abs(ev).max() and (e_ev <= S.BAR * unit[ix].min(1)).all()
    assert (over <= 2e-4).all()                                     # every segment, none left out
    assert ((chosen >= 0) & (chosen < K)).all()
    assert (df["agree"].to_numpy() == (chosen == df["category_ix"].to_numpy())).all()
    best = lt.loc[lt.groupby("data_ix")["responsibility"].idxmax()].set_index("data_ix")
    assert np.abs(best["responsibility"][ix].to_numpy() - df["decoder_category_prob"].to_numpy()).max() <= 1e-6
    # a rerun is identical and keeps the earlier tables as .prev
    classify.main(base + ["-S", out, "--matrix", mat])
    assert sorted(os.listdir(os.path.dirname(out))) == ["classified.csv", "classified.csv.prev", "matrix.csv",
                                                        "matrix.csv.prev"]
    assert pd.read_csv(out).equals(pd.read_csv(out + ".prev")) and pd.read_csv(mat).equals(pd.read_csv(mat + ".prev"))
    # a uniform prior changes the evidence and the weights, not the NLLs
    out_u = os.path.join(str(tmp_path), "u", "classified.csv")
    mat_u = os.path.join(str(tmp_path), "u", "matrix.csv")
    classify.main(base + ["-S", out_u, "--matrix", mat_u, "--prior", "uniform"])
    du, lu = pd.read_csv(out_u), pd.read_csv(mat_u)
    assert (lu["emission_nll"] == lt["emission_nll"]).all() and (lu["end_prediction_loss"] ==
                                                                  lt["end_prediction_loss"]).all()
    assert (lu["log_weight"] == 0).all() and not (du["log_evidence"] == df["log_evidence"]).any()
    ev_u = PW.posterior_reference(want["em"], want["off"])["log_evidence"]
    assert np.abs(du["log_evidence"].to_numpy() - ev_u[du["data_ix"].to_numpy()]).max() < S.BAR * np.abs(ev_u).max()
    with pytest.raises(SystemExit):
        classify.Classifier(os.path.join(GOLDEN, "ref_ckpt_plain.pt"))
