"""Time-warped scoring on the GPU: ``abcd_warp_nll`` and ``abcd_warp_path``
through the C ABI, ``RNN_Variational_Decoder.warp_against`` / ``align_to`` end
to end and the ``align.py`` CLI, against the float64 references of
``warp_cases.py``.

Bars (``warp_cases.py``): every ``warp`` within 1e-4 of its unit ``A[b, p]``
(along the float64 Viterbi path: the emission units, the |BCE| terms and the
|log_move| of the cells it visits), ``+inf`` exactly where the reference has
it; under identity moves with T_proto >= T within ``2 (F + 4) 2^-23 A`` of
``pair_em + pair_off`` of ``abcd_pairwise_nll`` on the same buffers.  Paths are
judged by their float64 cost (within 1e-4 A of the optimum), planted paths by
equality.  Every observed figure is printed (``-rA``) and kept with
``ABCD_PARITY_DUMP`` (profiles/warp_errors.json).
"""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import pairwise_cases as PW
import score_cases as S
import warp_cases as W
from test_gpu_score import ANN, CKPT, TOY, _bench_modules, _bits, _rows, _small_modules

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -7.0  # what the outputs hold before a call


# ----------------------------------------------------------------------------
# the C calls
# ----------------------------------------------------------------------------
def _rect(t, ld, tail=2):
    """An S x P (x F) prototype tensor on the device as the time-major rectangle
    the kernels read, in a buffer of row stride ld with ``tail`` more rows:
    padding columns and the tail are NaN."""
    S_, P = t.shape[:2]
    if t.dim() == 2:
        buf = torch.full((S_ * P + tail,), NAN)
        buf[:S_ * P] = t.reshape(-1)
    else:
        buf = torch.full((S_ * P + tail, ld), NAN)
        buf[:S_ * P, :t.shape[2]] = t.reshape(S_ * P, -1)
    return buf.cuda()


def _buffers(c, ld=0):
    ld = ld or c["F"]
    return dict(gt=_rows(c["gt"], c["F"]), y=_rows(c["y"], 1), mu=_rect(c["mu"], ld), ldm=ld, lv=_rect(c["lv"], ld),
                ldl=ld, o=_rect(c["o"], 1))


def _packed(c, gt, a):
    from modules import _native as N
    bs = torch.as_tensor(np.asarray(a["bs"]), dtype=torch.int64).contiguous()
    pk = N.Packed()
    pk.data = None if gt is None else gt.data_ptr()
    pk.batch_sizes = bs.data_ptr()
    pk.T, pk.L, pk.B, pk.F = (int(bs.numel()) if a["T"] is None else a["T"]), int(a["L"]), int(a["B"]), int(a["F"])
    return pk, bs


def _moves(lm):
    from modules import _native as N
    return None if lm is None else (N.c_double * 3)(*[float(v) for v in lm])


def warp_call(c, gt, y, mu, ldm, lv, ldl, o, moves, band=-1, marginal=False, ws="auto", out=True, pad=1, **over):
    """abcd_warp_nll -> (rc, warp): a B x (P + pad) buffer holding SENT before the call."""
    from modules import _native as N
    lib = N.lib()
    a = dict(bs=c["batch_sizes"], L=c["L"], B=c["B"], F=c["F"], P=c["P"], Tp=c["S"], T=None)
    a.update(over)
    pk, bs = _packed(c, gt, a)
    ldw = a.get("ldw", c["P"] + pad)
    warp = torch.full((c["B"], c["P"] + pad), SENT, device="cuda")
    if ws == "auto":
        ws = N.workspace(lib.abcd_warp_nll_workspace_bytes(pk.T, pk.B, c["P"], c["S"]), "cuda")
        ws.fill_(0xFF)
    rc = lib.abcd_warp_nll(pk, N.ptr(y), a["P"], a["Tp"], N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(o), _moves(moves),
                           band, int(marginal), N.ptr(warp) if out else None, ldw, N.ptr(ws),
                           0 if ws is None else ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, warp


def path_call(c, gt, y, mu, ldm, lv, ldl, o, moves, band, choice, ws="auto", want=("state", "comps"), **over):
    """abcd_warp_path -> (rc, state (L + 2 entries, -7 before the call), em, off, move (B, SENT before the call))."""
    from modules import _native as N
    lib = N.lib()
    a = dict(bs=c["batch_sizes"], L=c["L"], B=c["B"], F=c["F"], P=c["P"], Tp=c["S"], T=None)
    a.update(over)
    pk, bs = _packed(c, gt, a)
    state = torch.full((c["L"] + 2,), -7, dtype=torch.int32, device="cuda")
    pe, po, pm = (torch.full((c["B"],), SENT, device="cuda") for _ in range(3))
    ch = None if choice is None else torch.as_tensor(np.asarray(choice), dtype=torch.int32).cuda()
    if ws == "auto":
        ws = N.workspace(lib.abcd_warp_path_workspace_bytes(pk.T, pk.B, c["S"]), "cuda")
        ws.fill_(0xFF)
    comps = "comps" in want
    rc = lib.abcd_warp_path(pk, N.ptr(y), a["P"], a["Tp"], N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(o), _moves(moves),
                            band, N.ptr(ch), N.ptr(state) if "state" in want else None, N.ptr(pe) if comps else None,
                            N.ptr(po) if comps else None, N.ptr(pm) if comps else None, N.ptr(ws),
                            0 if ws is None else ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, state, pe, po, pm


def _err(got, ref, A):
    """(worst |got - ref| / A over the pairs where ref is finite, +inf agreement)."""
    got = got.double().cpu().numpy()
    fin = np.isfinite(ref)
    same_inf = bool(np.array_equal(np.isposinf(got), ~fin))
    e = np.abs(got[fin] - ref[fin]) / A[fin]
    return (float(e.max()) if e.size else 0.0), same_inf


def _suffix(c, b0):
    """The batch without its first b0 segments (the longest): the case's dict for segments b0 ..."""
    bs = c["batch_sizes"]
    keep = S.segment_of_rows(bs) >= b0
    nbs = (bs - b0)[bs > b0]
    d = dict(c, batch_sizes=nbs, T=len(nbs), B=c["B"] - b0, L=int(nbs.sum()), gt=c["gt"][torch.from_numpy(keep)],
             y=c["y"][torch.from_numpy(keep)])
    return d


# ----------------------------------------------------------------------------
# 1. abcd_warp_nll
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("marginal", (False, True), ids=("viterbi", "marginal"))
@pytest.mark.parametrize("case", W.ABI_CASES, ids=W.case_id)
def test_warp_nll_abi(case, marginal):
    from modules import _native as N
    shape, F, P, ld, kind, band, mname = case
    c = W.abi_inputs(shape, F, P, kind)
    ref = W.abi_reference(shape, F, P, kind, band, mname, marginal)
    moves, B, T = W.MOVES[mname], c["B"], c["T"]
    b = _buffers(c, ld)
    rc, warp = warp_call(c, **b, moves=moves, band=band, marginal=marginal)
    assert rc == 0
    assert (warp[:, P:] == SENT).all()  # columns >= P of a wider row are not written
    e, same_inf = _err(warp[:, :P], ref["value"], ref["A"])
    row = dict(case=W.case_id(case), marginal=marginal, F=F, warp=e, n_inf=int((~np.isfinite(ref["value"])).sum()))
    print(f"{W.case_id(case)} marginal={marginal}: worst |warp - ref| / A {e:.2e} (bar {W.BAR:.0e}), "
          f"{row['n_inf']} of {B * P} pairs unreachable")
    assert same_inf
    assert not torch.isnan(warp[:, :P]).any()
    assert e <= W.BAR
    if mname == "identity" and c["S"] >= T:  # pair_nll's comparison, on the same buffers
        from test_gpu_pairwise import pair_call
        rc, em, off = pair_call(dict(c, T=T), **b, Tp=c["S"])
        assert rc == 0
        d = np.abs(warp[:, :P].double().cpu().numpy() - (em[:, :P].double() + off[:, :P].double()).cpu().numpy())
        row["vs_pairwise"] = float((d / ref["A"]).max())
        print(f"   |warp - (pair_em + pair_off)| / A {row['vs_pairwise']:.2e} (bar {2 * W.cross_bar(F):.2e})")
        assert row["vs_pairwise"] <= 2 * W.cross_bar(F)
    # a second call and an exact-width output: bit for bit
    rc, w2 = warp_call(c, **b, moves=moves, band=band, marginal=marginal)
    assert rc == 0 and torch.equal(_bits(warp), _bits(w2))
    rc, w3 = warp_call(c, **b, moves=moves, band=band, marginal=marginal, pad=0)
    assert rc == 0 and torch.equal(_bits(w3), _bits(warp[:, :P].contiguous()))
    # a batch without its longest segments, down to the last one alone: its rows keep their bits
    for b0 in sorted({B // 2, B - 1} - {0}):
        cs = _suffix(c, b0)
        rc, ws_ = warp_call(cs, **_buffers(cs, ld), moves=moves, band=band, marginal=marginal)
        assert rc == 0 and torch.equal(_bits(ws_[:, :P]), _bits(warp[b0:, :P])), b0
    assert N.lib().abcd_device_status() == 0
    W.dump(f"abi_{W.case_id(case)}_{int(marginal)}", [row])


def test_warp_nll_live_nan_excludes_only_its_state():
    shape, F, P, kind, band, mname = "b33t9", 65, 17, "long", -1, "default"
    c = W.abi_inputs(shape, F, P, kind)
    moves = W.MOVES[mname]
    s_bad, p_bad = 2, 5
    mu = c["mu"].clone()
    mu[s_bad, p_bad, 7] = NAN
    lv = c["lv"].clone()
    lv[:, 11] = NAN          # a prototype that is all NaN
    c2 = dict(c, mu=mu, lv=lv)
    for marginal in (False, True):
        rc, clean = warp_call(c, **_buffers(c), moves=moves, marginal=marginal)
        ref = W.warp_reference(c["batch_sizes"], c["gt"], mu, lv, c["o"], c["y"], moves, band, marginal)
        rc2, warp = warp_call(c2, **_buffers(c2), moves=moves, marginal=marginal)
        assert rc == 0 and rc2 == 0
        other = [p for p in range(P) if p not in (p_bad, 11)]
        assert torch.equal(_bits(warp[:, other]), _bits(clean[:, other]))
        assert torch.isposinf(warp[:, 11]).all() and np.isposinf(ref["value"][:, 11]).all()
        e, same_inf = _err(warp[:, :P], ref["value"], ref["A"])
        print(f"live NaN, marginal={marginal}: worst |warp - ref| / A {e:.2e}; column {p_bad} moved by "
              f"{(warp[:, p_bad] - clean[:, p_bad]).abs().max().item():.3g}")
        assert same_inf and e <= W.BAR
        assert np.isfinite(ref["value"][:, p_bad]).all()  # only the paths through that state are lost
        if not marginal:
            assert all(s_bad not in ref["paths"][(b_, p_bad)][:] for b_ in range(c["B"]))


# ----------------------------------------------------------------------------
# 2. abcd_warp_path
# ----------------------------------------------------------------------------
def _check_path(path, n, S_, moves, band):
    assert path[0] == 0 and len(path) == n
    mv = np.diff(path)
    assert ((mv >= 0) & (mv <= 2)).all()
    assert all(moves[m] > -math.inf for m in mv)
    assert path.max() < S_
    if band >= 0:
        assert (np.abs(path - np.arange(n)) <= band).all()


@pytest.mark.parametrize("case", W.ABI_CASES, ids=W.case_id)
def test_warp_path_abi(case):
    from modules import _native as N
    shape, F, P, ld, kind, band, mname = case
    c = W.abi_inputs(shape, F, P, kind)
    ref = W.abi_reference(shape, F, P, kind, band, mname, False)
    moves, B, L = W.MOVES[mname], c["B"], c["L"]
    bs = c["batch_sizes"]
    off = np.concatenate([[0], np.cumsum(bs)])
    lens = ref["lengths"]
    # each segment's best prototype, the next one for every second segment, and every third segment skipped
    choice = np.array([(int(np.argmin(ref["viterbi"][b_])) + (b_ % 2)) % P for b_ in range(B)])
    skipped = np.arange(B) % 3 == 2
    choice[skipped] = -1
    seg_of = torch.from_numpy(S.segment_of_rows(bs))
    dead = torch.from_numpy(skipped)[seg_of]
    cn = dict(c, gt=torch.where(dead[:, None], torch.full_like(c["gt"], NAN), c["gt"]),
              y=torch.where(dead, torch.full_like(c["y"], NAN), c["y"]))   # the frames of skipped segments: NaN
    b = _buffers(cn, ld)
    rc, warp = warp_call(c, **_buffers(c, ld), moves=moves, band=band)
    rc2, state, pe, po, pm = path_call(cn, **b, moves=moves, band=band, choice=choice)
    assert rc == 0 and rc2 == 0
    assert (state[L:] == -7).all()
    state = state[:L].cpu().numpy()
    pe, po, pm, warp = (t.double().cpu().numpy() for t in (pe, po, pm, warp))
    worst_cost = worst_comp = 0.0
    for b_ in range(B):
        rows = off[:lens[b_]] + b_
        p = int(choice[b_])
        if p < 0 or not np.isfinite(ref["viterbi"][b_, p]):
            assert (state[rows] == -1).all() and np.isposinf([pe[b_], po[b_], pm[b_]]).all()
            assert p < 0 or np.isposinf(warp[b_, p])
            continue
        path = state[rows].astype(np.int64)
        _check_path(path, int(lens[b_]), c["S"], moves, band)
        A = ref["A"][b_, p]
        cost, mcost = W.path_cost(ref["c"][b_, p], path, moves)
        worst_cost = max(worst_cost, abs(cost + mcost - ref["viterbi"][b_, p]) / A)
        worst_comp = max(worst_comp, abs(pe[b_] + po[b_] + pm[b_] - warp[b_, p]) / A)
        assert abs(pm[b_] - mcost) <= 1e-6 * max(1.0, abs(mcost))
    print(f"{W.case_id(case)}: worst (path cost - optimum) / A {worst_cost:.2e}, "
          f"|em + off + move - warp| / A {worst_comp:.2e} (bars {W.BAR:.0e})")
    assert worst_cost <= W.BAR and worst_comp <= W.BAR
    rc3, state2, pe2, po2, pm2 = path_call(cn, **b, moves=moves, band=band, choice=choice)
    assert rc3 == 0 and torch.equal(state2[:L].cpu(), torch.from_numpy(state))
    assert N.lib().abcd_device_status() == 0
    W.dump(f"path_{W.case_id(case)}", [dict(case=W.case_id(case), under_optimum=worst_cost, components=worst_comp)])


@pytest.mark.parametrize("name", list(W.PLANTS))
def test_planted_alignment_is_recovered(name):
    c = W.planted(name)
    moves = W.MOVES["default"]
    ref = W.warp_reference(c["batch_sizes"], c["gt"], c["mu"], c["lv"], c["o"], c["y"], moves)
    assert np.array_equal(ref["paths"][(0, W.PLANT_CAT)], c["plant"])
    margin = np.sort(ref["value"][0])[1] - ref["value"][0, W.PLANT_CAT]
    assert int(np.argmin(ref["value"][0])) == W.PLANT_CAT and margin > 400.0
    b = _buffers(c)
    rc, warp = warp_call(c, **b, moves=moves)
    rc2, state, pe, po, pm = path_call(c, **b, moves=moves, band=-1, choice=[W.PLANT_CAT])
    assert rc == 0 and rc2 == 0
    print(f"plant {name}: warp {warp[0, :W.PLANT_P].tolist()}, margin {margin:.1f} nats")
    assert int(torch.argmin(warp[0, :W.PLANT_P])) == W.PLANT_CAT
    assert state[:c["L"]].cpu().tolist() == c["plant"].tolist()


def test_band_edge_on_a_super_block_boundary():
    """The planted path runs along the lower edge of the band and crosses from
    state 127 to 128 exactly where a frame block starts (frame 160): the
    predecessor lies in a super-block that block does not compute."""
    c = W.edge_planted()
    moves, band = W.MOVES["default"], W.EDGE_BAND
    b = _buffers(c)
    rows = []
    for marginal in (False, True):
        ref = W.warp_reference(c["batch_sizes"], c["gt"], c["mu"], c["lv"], c["o"], c["y"], moves, band, marginal)
        assert np.array_equal(ref["paths"][(0, W.EDGE_CAT)], c["plant"])
        rc, warp = warp_call(c, **b, moves=moves, band=band, marginal=marginal)
        assert rc == 0
        e, same_inf = _err(warp[:, :c["P"]], ref["value"], ref["A"])
        print(f"band edge, marginal={marginal}: warp {warp[0, :c['P']].tolist()}, float64 {ref['value'][0].tolist()}, "
              f"worst |warp - ref| / A {e:.2e} (bar {W.BAR:.0e})")
        rows.append(dict(case="edge_planted", marginal=marginal, F=c["F"], warp=e, n_inf=0))
        assert same_inf and e <= W.BAR
        assert int(torch.argmin(warp[0, :c["P"]])) == W.EDGE_CAT
    rc, state, pe, po, pm = path_call(c, **b, moves=moves, band=band, choice=[W.EDGE_CAT])
    assert rc == 0 and state[:c["L"]].cpu().tolist() == c["plant"].tolist()
    assert state[159] == 127 and state[160] == 128
    W.dump("abi_edge_planted", rows)


# ----------------------------------------------------------------------------
# 3. rejected arguments
# ----------------------------------------------------------------------------
def test_warp_abi_rejects_bad_arguments():
    from modules import _native as N
    c = W.abi_inputs("ties", 65, 17, "short")
    F, P = 65, 17
    b = _buffers(c)
    ok = W.MOVES["default"]
    choice = [0] * c["B"]

    def refused(moves=ok, nll=True, path=True, **kw):
        over = {k: kw.pop(k) for k in list(kw) if k in ("bs", "L", "B", "P", "Tp", "T", "ldw")}
        nkw = {k: kw.pop(k) for k in list(kw) if k in ("out",)}
        pkw = {k: kw.pop(k) for k in list(kw) if k in ("choice", "want")}
        if nll:
            rc, warp = warp_call(c, **dict(b, **kw), moves=moves, **nkw, **over)
            assert rc == N.ABCD_EINVAL == 1000, (kw.keys(), over, rc)
            assert (warp == SENT).all()  # nothing written
        if path and "ldw" not in over:
            rc, state, pe, po, pm = path_call(c, **dict(b, **kw), moves=moves, band=-1,
                                              **dict(dict(choice=choice), **pkw), **over)
            assert rc == N.ABCD_EINVAL, (kw.keys(), over, rc)
            assert (state == -7).all() and (pe == SENT).all() and (po == SENT).all() and (pm == SENT).all()

    assert warp_call(c, **b, moves=ok)[0] == 0
    assert path_call(c, **b, moves=ok, band=-1, choice=choice)[0] == 0
    assert c["S"] < c["T"]  # a rectangle shorter than the batch is accepted
    bs = c["batch_sizes"]
    up = bs.copy()
    up[2], up[3] = bs[3], bs[2]
    assert not (np.diff(up) <= 0).all() and up.sum() == c["L"]
    refused(bs=up)
    refused(B=c["B"] - 1)
    refused(L=c["L"] + 1)
    refused(P=0)
    refused(Tp=0)
    refused(Tp=16384)
    refused(ldm=F - 1)
    refused(ldl=F - 1)
    refused(ldw=P - 1)
    for k in ("gt", "mu", "lv", "y", "o"):
        refused(**{k: None})
    refused(ws=None)
    refused(ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    refused(moves=None)
    refused(moves=(NAN, 0.0, 0.0))
    refused(moves=(math.log(0.5), math.inf, math.log(0.5)))
    refused(moves=(-math.inf, -math.inf, -math.inf))
    refused(out=False, path=False)
    refused(choice=None, nll=False)
    refused(want=("comps",), nll=False)
    lib = N.lib()
    assert lib.abcd_warp_nll_workspace_bytes(4097, 4, 4, 10) == 0 and lib.abcd_warp_nll_workspace_bytes(4096, 4, 4, 10)
    assert lib.abcd_warp_nll_workspace_bytes(10, 1 << 16, 1 << 15, 10) == 0
    assert lib.abcd_warp_nll_workspace_bytes(10, 4, 4, 16384) == 0 and lib.abcd_warp_path_workspace_bytes(10, 4, 16384) == 0
    assert lib.abcd_warp_path_workspace_bytes(4097, 4, 10) == 0 and lib.abcd_warp_path_workspace_bytes(10, 4, 16383)
    assert lib.abcd_device_status() == 0


# ----------------------------------------------------------------------------
# 4. warp_against() / align_to() end to end
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PW.E2E_SMALL) + ["edge"])
def test_warp_against_end_to_end(name):
    from modules import _native as N
    from modules import alignment, ops
    from test_gpu_pairwise import _columns
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
    feats, spk, _, _ = _columns(samp, dec, batch, cats)
    P, F = feats.shape[0], data.shape[1]
    Tp = int(math.ceil(1.5 * T))
    protos = dec.prototypes(feats, Tp, speaker=spk)
    mu, lv, o = (t.cpu() for t in protos)
    # identity moves: score_against's comparison
    em, off, _ = dec.score_against(protos, bsz, data, is_off)
    ident = dec.warp_against(protos, bsz, data, is_off, log_moves=ops.IDENTITY_LOG_MOVES)
    ref_i = W.warp_reference(bsz.numpy(), batch["data"], mu, lv, o, batch["is_offset"], W.MOVES["identity"])
    e_id = float((np.abs(ident.double().cpu().numpy() - (em.double() + off.double()).cpu().numpy()) / ref_i["A"]).max())
    print(f"{name}: P = {P}, T = {T}, T_proto = {Tp}; identity moves against score_against: {e_id:.2e} of A "
          f"(bar {2 * W.cross_bar(F):.2e})")
    assert tuple(ident.shape) == (B, P) and e_id <= 2 * W.cross_bar(F)
    # default moves: marginal <= Viterbi <= the identity path's cost, each against float64 on the same prototypes
    moves = W.MOVES["default"]
    vit = dec.warp_against(protos, bsz, data, is_off)
    mar = dec.warp_against(protos, bsz, data, is_off, marginal=True)
    ref_v = W.warp_reference(bsz.numpy(), batch["data"], mu, lv, o, batch["is_offset"], moves)
    ref_m = W.warp_reference(bsz.numpy(), batch["data"], mu, lv, o, batch["is_offset"], moves, marginal=True)
    e_v, inf_v = _err(vit, ref_v["value"], ref_v["A"])
    e_m, inf_m = _err(mar, ref_m["value"], ref_m["A"])
    print(f"{name}: default moves against float64: Viterbi {e_v:.2e}, marginal {e_m:.2e} of A (bar {W.BAR:.0e})")
    assert inf_v and inf_m and e_v <= W.BAR and e_m <= W.BAR
    vit64, mar64, A = vit.double().cpu().numpy(), mar.double().cpu().numpy(), ref_v["A"]
    lens = ref_v["lengths"]
    ident_path = ident.double().cpu().numpy() - ((lens - 1) * moves[1])[:, None]  # the identity path under these moves
    assert (mar64 <= vit64 + W.BAR * A).all() and (vit64 <= ident_path + W.BAR * A).all()
    # a banded call, and no offset targets: the end target is one on the last frame
    band = dec.warp_against(protos, bsz, data, is_off, band=2)
    assert (band.double().cpu().numpy() >= vit64 - W.BAR * A).all()
    assert torch.equal(_bits(dec.warp_against(protos, bsz, data)), _bits(vit))  # the fixtures' targets are those
    # each segment's path to its best column
    best = vit.argmin(1)
    choice = best.clone()
    choice[B // 2] = -1
    states, pe, po, pm = dec.align_to(protos, bsz, data, choice, is_off)
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    assert states.dtype == torch.int32 and states.shape[0] == data.shape[0]
    s = alignment.summarize_paths(states, bsz)
    off_rows = np.concatenate([[0], np.cumsum(bsz.numpy())])
    worst = 0.0
    for b in range(B):
        rows = off_rows[:lens[b]] + b
        path = states[rows].cpu().numpy().astype(np.int64)
        if b == B // 2:
            assert (path == -1).all() and s["end_state"][b] == -1 and torch.isposinf(pe[b])
            continue
        p = int(best[b])
        _check_path(path, int(lens[b]), Tp, moves, -1)
        cost, mcost = W.path_cost(ref_v["c"][b, p], path, moves)
        worst = max(worst, abs(cost + mcost - ref_v["viterbi"][b, p]) / A[b, p],
                    abs(float(pe[b]) + float(po[b]) + float(pm[b]) - vit64[b, p]) / A[b, p])
        assert int(s["end_state"][b]) == path[-1] and int(s["length"][b]) == lens[b]
        assert int(s["n_stay"][b]) == int((np.diff(path) == 0).sum())
    print(f"{name}: paths: worst of (cost - optimum) and |em + off + move - warp| {worst:.2e} of A")
    assert worst <= W.BAR
    lm = alignment.fit_moves(states, bsz)
    assert abs(sum(math.exp(v) for v in lm) - 1.0) < 1e-12
    r2 = alignment.align_segments(dec, protos, bsz, data, is_off)
    assert torch.equal(r2["best"].cpu(), best.cpu()) and torch.equal(_bits(r2["warp"]), _bits(vit))
    W.dump(f"e2e_{name}", [dict(case=name, P=P, T=T, T_proto=Tp, F=F, vs_score_against=e_id,
                                vs_score_against_over_bar=e_id / (2 * W.cross_bar(F)), viterbi=e_v, marginal=e_m,
                                paths=worst)])
    with pytest.raises(ValueError):
        dec.warp_against((protos[0][0], protos[1][0], protos[2][0]), bsz, data, is_off)
    with pytest.raises(ValueError):
        dec.warp_against(protos, bsz, data, is_off, log_moves=(-math.inf,) * 3)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.warp_nll(data.clone().requires_grad_(True), bsz, is_off, protos[0].reshape(-1, F), protos[1].reshape(-1, F),
                     protos[2].reshape(-1), list(moves), -1, False, P, F)


# ----------------------------------------------------------------------------
# 5. align.py on the toy data with the reference's small checkpoint
# ----------------------------------------------------------------------------
def test_align_cli_on_toy_data(tmp_path):
    import align
    import classify
    base = [CKPT, TOY, ANN, "1.0", "-b", "4"]
    out = os.path.join(str(tmp_path), "a", "aligned.csv")
    paths = os.path.join(str(tmp_path), "a", "paths.csv")
    assert align.main(base + ["-S", out, "--paths", paths, "--fit_moves", "1"]) == out
    df, pt = pd.read_csv(out), pd.read_csv(paths)
    assert list(df.columns)[:len(align.COLUMNS)] == list(align.COLUMNS)
    assert list(pt.columns)[:3] == list(align.PATH_COLUMNS)
    assert len(df) > 0 and sorted(df["data_ix"]) == list(range(len(df)))
    assert (df["tempo"] > 0).all() and (df["end_state"] >= 0).all() and np.isfinite(df["warp_nll"]).all()
    assert ((df["end_state"] + 1) / df["length"] - df["tempo"]).abs().max() < 1e-12
    assert (df["warp_best_prob"] > 0).all() and (df["warp_best_prob"] <= 1 + 1e-6).all()
    # the per-frame table: every segment's frames in order, from state 0 to end_state by moves of 0, 1 or 2
    assert len(pt) == int(df["length"].sum())
    for ix, g in pt.groupby("data_ix"):
        row = df[df["data_ix"] == ix].iloc[0]
        g = g.sort_values("frame")
        st = g["state"].to_numpy()
        assert g["frame"].tolist() == list(range(int(row["length"]))) and st[0] == 0 and st[-1] == row["end_state"]
        assert set(np.diff(st).tolist()) <= {0, 1, 2}
        assert int((np.diff(st) == 0).sum()) == row["n_stay"] and int((np.diff(st) == 2).sum()) == row["n_skip"]
    # rigid moves: classify.py's comparison and its chosen category, on every row
    rigid = os.path.join(str(tmp_path), "a", "rigid.csv")
    cl = os.path.join(str(tmp_path), "a", "classified.csv")
    align.main(base + ["-S", rigid, "--moves", "0", "1", "0"])
    classify.main(base + ["-S", cl])
    dr, dc = pd.read_csv(rigid).sort_values("data_ix"), pd.read_csv(cl).sort_values("data_ix")
    assert dr["warp_category_ix"].tolist() == dc["decoder_category_ix"].tolist()
    assert (dr["tempo"] == 1.0).all() and (dr["n_stay"] == 0).all() and (dr["n_skip"] == 0).all()
    assert np.abs(dr["warp_log_evidence"].to_numpy() - dc["log_evidence"].to_numpy()).max() <= \
        1e-4 * np.abs(dc["log_evidence"]).max()
    assert dr[["data_ix", "length", "category_ix"]].equals(dc[["data_ix", "length", "category_ix"]])
