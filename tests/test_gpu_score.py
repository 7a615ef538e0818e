"""Per-segment ELBO scoring on the GPU: ``abcd_segment_losses`` and
``abcd_sampler_kl_rows`` through the C ABI, ``RNN_Variational_Decoder.score``
/ ``ABCDSampler.kl_rows`` end to end and the ``score.py`` CLI, against the
float64 references of ``score_cases.py``.

Bars (``score_cases.py``): a per-segment result within 1e-4 of its unit (the
float64 sum of the absolute values of its terms); sum_b seg[b] within 2^-21 A
of the decoder's own scalar (both are fp64 sums of the same fp32 terms: one
fp32 rounding per segment and one for the total, times 4 for a differently
contracted multiply-add); prior * B / N + sum rows within 1e-5 of
``abcd_sampler_kl`` (two HIP forms of one sum); end to end
``edge_cases.rel_err`` < 1e-4 against the float64 oracle.  Every observed
figure is printed (``-rA``) and kept with ``ABCD_PARITY_DUMP``
(profiles/score_errors.json).
"""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import edge_cases as E
import score_cases as S
from gpu_helpers import build_from_meta, named_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "toy_data")
ANN = os.path.join(TOY, "annotation_20170806-080002_89.2-94.22.csv")
CKPT = os.path.join(GOLDEN, "ref_ckpt_small.pt")
NAN = float("nan")
SENT = -7.0  # what the outputs hold before a call


# ----------------------------------------------------------------------------
# 1. abcd_segment_losses through ctypes
# ----------------------------------------------------------------------------
def _rows(t, ld, tail=2):
    """t (L x F or L) on the device in a buffer of row stride ld with `tail`
    extra rows, padding columns and tail rows NaN."""
    if t.dim() == 1:
        buf = torch.full((t.shape[0] + tail,), NAN)
        buf[:t.shape[0]] = t
    else:
        buf = torch.full((t.shape[0] + tail, ld), NAN)
        buf[:t.shape[0], :t.shape[1]] = t
    return buf.cuda()


def seg_call(bs, L, B, F, gt, mu, ldm, lv, ldl, x, y, want=("em", "off", "len"), ws="auto", T=None):
    """abcd_segment_losses -> (rc, em, off, len) with the outputs not asked for None."""
    from modules import _native as N
    lib = N.lib()
    bs = torch.as_tensor(np.asarray(bs), dtype=torch.int64).contiguous()
    pk = N.Packed()
    pk.data = None if gt is None else gt.data_ptr()
    pk.batch_sizes = bs.data_ptr()
    pk.T, pk.L, pk.B, pk.F = (int(bs.numel()) if T is None else T), int(L), int(B), int(F)
    n = max(int(B), 1)
    em = torch.full((n,), SENT, device="cuda") if "em" in want else None
    off = torch.full((n,), SENT, device="cuda") if "off" in want else None
    ln = torch.full((n,), int(SENT), dtype=torch.int32, device="cuda") if "len" in want else None
    if ws == "auto":
        ws = N.workspace(lib.abcd_segment_losses_workspace_bytes(pk.T, pk.B), "cuda")
    rc = lib.abcd_segment_losses(pk, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(x), N.ptr(y), N.ptr(em), N.ptr(off),
                                 N.ptr(ln), N.ptr(ws), 0 if ws is None else ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, em, off, ln


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("F", S.ABI_F)
@pytest.mark.parametrize("shape", list(S.ABI_SHAPES))
def test_segment_losses_abi(shape, F):
    c = S.abi_inputs(shape, F)
    ref, bs, L, B = c["ref"], c["batch_sizes"], c["L"], len(c["lengths"])
    seg_of = torch.from_numpy(S.segment_of_rows(bs))
    rows = []
    for ld in (F, S.PAD_LD):
        gt, mu, lv = _rows(c["gt"], F), _rows(c["mu"], ld), _rows(c["lv"], ld)
        x, y = _rows(c["x"], 1), _rows(c["y"], 1)
        rc, em, off, ln = seg_call(bs, L, B, F, gt, mu, ld, lv, ld, x, y)
        assert rc == 0
        assert ln.cpu().tolist() == ref["lengths"].tolist()
        e_em = np.abs(em.double().cpu().numpy() - ref["em"]) / ref["A"]
        e_off = np.abs(off.double().cpu().numpy() - ref["off"]) / ref["off"]
        print(f"{shape} F={F} ld={ld}: worst |seg - ref| / unit  em {e_em.max():.2e}  off {e_off.max():.2e}")
        rows.append(dict(shape=shape, F=F, ld=ld, em=float(e_em.max()), off=float(e_off.max())))
        assert np.isfinite(e_em).all() and np.isfinite(e_off).all()
        assert e_em.max() <= S.BAR and e_off.max() <= S.BAR
        # a second call: bit for bit
        rc, em2, off2, ln2 = seg_call(bs, L, B, F, gt, mu, ld, lv, ld, x, y)
        assert rc == 0 and torch.equal(_bits(em), _bits(em2)) and torch.equal(_bits(off), _bits(off2))
        assert torch.equal(ln, ln2)
        # without the offset pair, and with each output NULL in turn: the others are unchanged
        rc, em3, off3, ln3 = seg_call(bs, L, B, F, gt, mu, ld, lv, ld, None, None, want=("em", "len"))
        assert rc == 0 and off3 is None and torch.equal(_bits(em), _bits(em3)) and torch.equal(ln, ln3)
        for drop in ("em", "off", "len"):
            want = tuple(k for k in ("em", "off", "len") if k != drop)
            rc, a, b, n = seg_call(bs, L, B, F, gt, mu, ld, lv, ld, x, y, want=want)
            assert rc == 0
            assert a is None if drop == "em" else torch.equal(_bits(a), _bits(em))
            assert b is None if drop == "off" else torch.equal(_bits(b), _bits(off))
            assert n is None if drop == "len" else torch.equal(n, ln)
        # lengths alone need no tensors at all
        rc, _, _, n = seg_call(bs, L, B, F, None, None, 0, None, 0, None, None, want=("len",))
        assert rc == 0 and torch.equal(n, ln)
        # nothing outside a segment's rows is read: with every other row NaN, segment b's results keep their bits
        for b in range(B):
            mine = (seg_of == b)
            keep2 = torch.cat([mine, torch.zeros(2, dtype=torch.bool)]).cuda()

            def only(t):
                m = keep2 if t.dim() == 1 else keep2[:, None]
                return torch.where(m, t, torch.full_like(t, NAN))
            rc, a, o, _ = seg_call(bs, L, B, F, only(gt), only(mu), ld, only(lv), ld, only(x), only(y))
            assert rc == 0
            assert _bits(a)[b] == _bits(em)[b] and _bits(o)[b] == _bits(off)[b], (b, ld)
            if B > 1:
                assert torch.isnan(a).sum() == B - 1  # the scratch copy's NaNs do reach the other segments
    S.dump(f"abi_{shape}_F{F}", rows)


def test_segment_losses_abi_rejects_bad_arguments():
    from modules import _native as N
    c = S.abi_inputs("ties", 65)
    bs, L, B, F = c["batch_sizes"], c["L"], 5, 65
    gt, mu, lv, x, y = (_rows(c[k], F) for k in ("gt", "mu", "lv", "x", "y"))

    def refused(**kw):
        a = dict(bs=bs, L=L, B=B, F=F, gt=gt, mu=mu, ldm=F, lv=lv, ldl=F, x=x, y=y)
        a.update(kw)
        rc, em, off, ln = seg_call(**a)
        assert rc == N.ABCD_EINVAL == 1000, (kw.keys(), rc)
        assert (em == SENT).all() and (off == SENT).all() and (ln == int(SENT)).all()  # nothing written

    assert seg_call(bs, L, B, F, gt, mu, F, lv, F, x, y)[0] == 0
    up = bs.copy()
    up[2], up[3] = bs[3], bs[2]      # [5, 3, 2, 3, ...]: a step grows
    assert (np.diff(bs) <= 0).all() and not (np.diff(up) <= 0).all() and up.sum() == L
    refused(bs=up)                       # not non-increasing
    refused(B=B - 1)                     # batch_sizes[0] != B
    refused(B=B + 1)
    refused(L=L + 1)                     # L != sum batch_sizes
    refused(L=L - 1)
    refused(ldm=F - 1)                   # a stride below F
    refused(ldl=F - 1)
    refused(gt=None)                     # seg_em without the ground truth
    refused(mu=None)
    refused(x=None)                      # one of the offset pair alone
    refused(y=None)
    refused(ws=None)
    refused(ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    refused(bs=np.zeros(0, dtype=np.int64), T=0)
    assert N.lib().abcd_device_status() == 0


# ----------------------------------------------------------------------------
# 2. consistency with the decoder's own scalars
# ----------------------------------------------------------------------------
def _bench_modules(r):
    """enc, samp, dec at a bench.py width set, seed-1111 weights (checked against the oracle's)."""
    from modules import model as M
    cfg = r["cfg"]
    torch.manual_seed(1111)
    enc = M.RNN_Variational_Encoder(cfg["F"], cfg["H"], rnn_type=cfg["rnn"])
    samp = M.ABCDSampler(enc.hidden_size_total, cfg["Hm"], cfg["K"], cfg["D"])
    dec = M.RNN_Variational_Decoder(cfg["F"], cfg["H"], cfg["Hm"], cfg["D"], rnn_type=cfg["rnn"],
                                    num_speakers=cfg["spk"] or None, speaker_embed_dim=cfg["sdim"])
    for m in (enc, samp, dec):
        m.cuda().eval()
    for k, p in named_params(enc, samp, dec).items():
        assert torch.equal(p.detach().cpu(), r["P"][k]), k
    return enc, samp, dec


def _small_modules(r):
    mods = build_from_meta(r["meta"], r["arr"], device="cuda")
    for m in mods:
        m.eval()
    return mods


@pytest.mark.parametrize("case,widths", list(S.SUM_EDGES) + [("lstm_odd", None)])
def test_segment_sums_match_decoder_scalars(case, widths):
    from modules import _native as N
    if widths is None:
        r = S.small_reference(case)
        _, _, dec = _small_modules(r)
    else:
        r = S.edge_reference(case, widths)
        _, _, dec = _bench_modules(r)
    batch = r["batch"]
    bsz = batch["batch_sizes"]
    B, F = int(bsz[0]), r["ocfg"]["F"]
    data, is_off = batch["data"].cuda(), batch["is_offset"].cuda()
    feats = torch.randn(B, dec.feature_size, generator=torch.Generator().manual_seed(3)).cuda()
    spk = batch["speakers"].cuda() if dec.embed_speaker is not None else None
    N.lib().abcd_dispatch_reset()
    with torch.no_grad():  # the existing op, eval mode, Philox noise
        em, off, _, (mu, lv), offl = dec(feats, batch_sizes=bsz, speaker=spk, ground_truth_out=data,
                                         ground_truth_offset=is_off)
    L = int(data.shape[0])
    rc, sem, soff, ln = seg_call(bsz.numpy(), L, B, F, data, mu, F, lv, F, offl, is_off)
    assert rc == 0 and N.lib().abcd_device_status() == 0
    ran = N.dispatch()
    print(case, widths, "dec_fwd:", ran["dec_fwd"][0], "| seg_losses:", ran["seg_losses"])
    assert ran["seg_losses"] == (f"seg_losses<1024> grid {B}", 1)
    ref = S.segment_reference(bsz.numpy(), data, mu, lv, offl, is_off)  # float64 on the op's fp32 outputs
    assert ln.cpu().tolist() == ref["lengths"].tolist() == list(S.lengths_of(bsz.numpy()))
    A, O = ref["A"].sum(), ref["off"].sum()
    d_em = abs(sem.double().sum().item() - em.double().item()) / A
    d_off = abs(soff.double().sum().item() - off.double().item()) / O
    e_em = (np.abs(sem.double().cpu().numpy() - ref["em"]) / ref["A"]).max()
    e_off = (np.abs(soff.double().cpu().numpy() - ref["off"]) / ref["off"]).max()
    print(f"{case} {widths}: |sum seg - scalar| / A  em {d_em:.2e} off {d_off:.2e} (bar {S.SUM_BAR:.2e}); "
          f"per segment vs float64  em {e_em:.2e} off {e_off:.2e}")
    S.dump(f"sum_{case}_{widths}", [dict(case=case, widths=widths, sum_em=d_em, sum_off=d_off, em=float(e_em),
                                         off=float(e_off))])
    assert d_em <= S.SUM_BAR and d_off <= S.SUM_BAR
    assert e_em <= S.BAR and e_off <= S.BAR


# ----------------------------------------------------------------------------
# 3. abcd_sampler_kl_rows
# ----------------------------------------------------------------------------
def _kl_cfg(c):
    """[input_size, mlp_hidden, num_categories, feature_dim, plain, valid_categories, valid_feature_dim]"""
    if c["plain"]:
        return [16, 16, 16, c["width"], 1, 0, c["valid"]]
    return [16, 16, c["width"], 16, 0, c["valid"], 0]


@pytest.mark.parametrize("B", S.KL_B)
@pytest.mark.parametrize("name", list(S.KL_CASES))
def test_sampler_kl_rows(name, B):
    from modules import _native as N, ops
    c = S.kl_inputs(name, B)
    ref, cfg = c["ref"], _kl_cfg(c)
    logits = c["logits"].cuda()
    psl = None if c["plain"] else c["psl"].cuda()
    N.lib().abcd_dispatch_reset()
    rows, prior = ops.sampler_kl_rows(logits, psl, cfg, c["a0"], float(S.N_DATA))
    rows2, prior2 = ops.sampler_kl_rows(logits, psl, cfg, c["a0"], float(S.N_DATA))
    kl = ops.sampler_kl(logits, psl, cfg, c["a0"], float(S.N_DATA))[0]
    torch.cuda.synchronize()
    kern, count = N.dispatch()["kl_rows"]
    print(name, B, kern)
    assert count == 2 and kern.startswith("kl_rows_plain<" if c["plain"] else "kl_rows_seg<")
    assert torch.equal(_bits(rows), _bits(rows2)) and torch.equal(prior, prior2)
    e_rows = (np.abs(rows.double().cpu().numpy() - ref["rows"]) / ref["row_unit"]).max()
    e_prior = abs(float(prior) - ref["prior"]) / ref["prior_unit"]
    total = float(prior.double()) * B / S.N_DATA + float(rows.double().sum())
    d_kl = abs(total - float(kl))
    print(f"{name} B={B}: rows {e_rows:.2e} prior {e_prior:.2e} of their units; "
          f"|prior B/N + sum rows - abcd_sampler_kl| = {d_kl:.2e} (kl {float(kl):.6g})")
    S.dump(f"kl_{name}_B{B}", [dict(case=name, B=B, rows=float(e_rows), prior=e_prior,
                                    kl_diff_rel=d_kl / max(abs(float(kl)), 1e-30))])
    assert rows.shape == (B,) and prior.shape == ()
    assert e_rows <= S.BAR and e_prior <= S.BAR
    assert d_kl <= S.KL_SUM_BAR * abs(float(kl)) + 1e-6  # the bar of test_gpu_persist.py between two HIP forms
    assert abs(float(kl) - ref["kl"]) <= S.BAR * (ref["row_unit"].sum() + ref["prior_unit"] * B / S.N_DATA)
    if c["plain"]:
        assert float(prior) == 0.0


def test_scoring_ops_are_forward_only():
    from modules import ops
    c = S.kl_inputs("k16", 5)
    logits = c["logits"].cuda().requires_grad_(True)
    psl = c["psl"].cuda()
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.sampler_kl_rows(logits, psl, _kl_cfg(c), 1.0, 100.0)
    with torch.no_grad():
        rows, _ = ops.sampler_kl_rows(logits, psl, _kl_cfg(c), 1.0, 100.0)
    assert not rows.requires_grad
    a = S.abi_inputs("ties", 65)
    mu = a["mu"].cuda().requires_grad_(True)
    args = (a["gt"].cuda(), torch.from_numpy(a["batch_sizes"]), mu, a["lv"].cuda(), a["x"].cuda(), a["y"].cuda(), 65)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.segment_losses(*args)
    with torch.no_grad():
        em, off, ln = ops.segment_losses(*args)
    assert np.abs(em.double().cpu().numpy() - a["ref"]["em"]).max() <= S.BAR * a["ref"]["A"].max()
    # a row-strided view (a padded stash) passes without a copy and gives the same bits
    wide = torch.full((a["L"], S.PAD_LD), NAN, device="cuda")
    wide[:, :65] = a["mu"].cuda()
    em2, _, _ = ops.segment_losses(args[0], args[1], wide[:, :65], args[3], args[4], args[5], 65)
    assert torch.equal(_bits(em), _bits(em2))
    with pytest.raises(RuntimeError):
        ops.segment_losses(a["gt"], args[1], a["mu"], a["lv"], None, None, 65)  # CPU tensors are refused


# ----------------------------------------------------------------------------
# 4. decoder.score(mean=True) and sampler.kl_rows end to end
# ----------------------------------------------------------------------------
def _score_batch(enc, samp, dec, batch, N_data):
    bsz = batch["batch_sizes"]
    data, is_off = batch["data"].cuda(), batch["is_offset"].cuda()
    spk = batch["speakers"].cuda() if dec.embed_speaker is not None else None
    with torch.no_grad():
        logits = samp(enc(torch.nn.utils.rnn.PackedSequence(data, bsz)))
        feats = samp.sample(logits, no_sample=True)
    em, off, lengths = dec.score(feats, bsz, speaker=spk, ground_truth_out=data, ground_truth_offset=is_off,
                                 mean=True)
    rows, prior = samp.kl_rows(logits, N_data)
    return dict(em=em, off=off, lengths=lengths, rows=rows, prior=prior, logits=logits)


def _one_segment(batch, b):
    """Segment b of a packed batch as a batch of its own."""
    PS = torch.nn.utils.rnn.PackedSequence
    seq = torch.nn.utils.rnn.unpack_sequence(PS(batch["data"], batch["batch_sizes"]))[b]
    n = seq.shape[0]
    return dict(data=seq.contiguous(), batch_sizes=torch.ones(n, dtype=torch.int64),
                is_offset=torch.tensor([0.0] * (n - 1) + [1.0]), speakers=batch["speakers"][b:b + 1])


@pytest.mark.parametrize("name", list(S.E2E_SMALL) + ["edge"])
def test_score_end_to_end_vs_oracle64(name):
    from modules import _native as N
    if name == "edge":
        r = S.edge_reference(*S.E2E_EDGE)
        mods = _bench_modules(r)
        want = S.oracle_scores(r["P"], r["ocfg"], r["batch"], S.N_DATA)
    else:
        r = S.small_reference(name)
        mods = _small_modules(r)
        want = r["scores"]
    batch = r["batch"]
    N.lib().abcd_dispatch_reset()
    got = _score_batch(*mods, batch, S.N_DATA)
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    print(name, "dec_fwd:", N.dispatch()["dec_fwd"][0])
    B = int(batch["batch_sizes"][0])
    assert got["lengths"].cpu().tolist() == want["lengths"].tolist()
    assert got["lengths"].dtype == torch.int64 and got["em"].shape == got["off"].shape == got["rows"].shape == (B,)
    rows = []
    for k in ("em", "off", "rows"):
        e = E.rel_err(got[k], torch.from_numpy(want[k]))
        print(f"{name} {k}: rel_err {e:.2e}")
        rows.append(dict(case=name, tensor=k, rel_err=e))
        assert e < S.BAR, (k, e)
    e = abs(float(got["prior"]) - want["prior"]) / abs(want["prior"])
    print(f"{name} prior: rel {e:.2e}")
    rows.append(dict(case=name, tensor="prior", rel_err=e))
    assert e < S.BAR
    # the sums are the batch scalars of the oracle
    for k, tot in (("em", "em_total"), ("off", "off_total")):
        assert abs(got[k].double().sum().item() - want[tot]) <= S.BAR * abs(want[tot]), k
    kl = float(got["prior"].double()) * B / S.N_DATA + got["rows"].double().sum().item()
    assert abs(kl - want["kl_total"]) <= S.BAR * abs(want["kl_total"]) + 1e-6
    # a segment scored alone gets its in-batch score (rows are independent)
    for b in sorted({0, B // 2, B - 1}):
        alone = _score_batch(*mods, _one_segment(batch, b), S.N_DATA)
        assert alone["lengths"].tolist() == [int(want["lengths"][b])]
        for k in ("em", "off", "rows"):
            d = abs(float(alone[k][0]) - float(got[k][b])) / float(got[k].abs().max())
            print(f"{name} segment {b} alone, {k}: {d:.2e}")
            rows.append(dict(case=name, tensor=f"alone{b}/{k}", rel_err=d))
            assert d < S.BAR, (b, k, d)
    S.dump(f"e2e_{name}", rows)


def test_score_sampled_noise():
    """mean=False: an explicit eps reproduces the decoder op's scalars under
    that eps; Philox draws are seeded; zero eps is the mean."""
    from modules import noise
    r = S.small_reference("lstm_speaker")
    enc, samp, dec = _small_modules(r)
    batch = r["batch"]
    bsz = batch["batch_sizes"]
    data, is_off, spk = batch["data"].cuda(), batch["is_offset"].cuda(), batch["speakers"].cuda()
    feats = torch.randn(int(bsz[0]), dec.feature_size, generator=torch.Generator().manual_seed(5)).cuda()
    eps = r["arr"]["eps"].cuda()
    kw = dict(speaker=spk, ground_truth_out=data, ground_truth_offset=is_off)
    em, off, _ = dec.score(feats, bsz, mean=False, eps=eps, **kw)
    noise.replay(eps)
    with torch.no_grad():
        em_s, off_s = dec(feats, batch_sizes=bsz, **kw)[:2]
    assert abs(em.double().sum().item() - float(em_s)) <= 1e-5 * abs(float(em_s))
    assert abs(off.double().sum().item() - float(off_s)) <= 1e-5 * abs(float(off_s))
    em0, off0, _ = dec.score(feats, bsz, mean=False, eps=torch.zeros_like(eps), **kw)
    emm, offm, _ = dec.score(feats, bsz, mean=True, **kw)
    assert torch.equal(em0, emm) and torch.equal(off0, offm) and not torch.equal(em, emm)
    saved = noise.get_state()
    try:
        runs = []
        for seed in (7, 7, 8):
            noise.set_mode("philox")
            noise.manual_seed(seed)
            runs.append(dec.score(feats, bsz, mean=False, **kw)[0])
    finally:
        noise.set_state(saved)
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    assert dec.score(feats, bsz, speaker=spk, ground_truth_out=data)[1] is None  # no offset targets: no BCE
    with pytest.raises(ValueError):
        dec.score(feats, bsz, ground_truth_out=data)  # this decoder embeds speakers
    with pytest.raises(ValueError):
        dec.score(feats, bsz, mean=False, eps=eps[:-1], **kw)


def test_plain_sampler_kl_rows():
    """Sampler.kl_rows on the plain fixtures (f = 16 and the padded f = 10): the
    rows sum to kl_divergence, on its own forward's parameters and on foreign ones."""
    from golden_io import load_small
    for name in ("plain_lstm", "plain_odd"):
        meta, arr = load_small(name)
        enc, samp, _ = build_from_meta(meta, arr, device="cuda")
        h = torch.randn(5, enc.hidden_size_total, generator=torch.Generator().manual_seed(2)).cuda()
        with torch.no_grad():
            params = samp(h)
            kl = samp.kl_divergence(params)
        rows, prior = samp.kl_rows(params)
        want, unit = S.plain_kl_reference(params[0], params[1])
        e = (np.abs(rows.double().cpu().numpy() - want) / unit).max()
        print(f"{name}: f = {params[0].shape[1]}, rows {e:.2e} of their unit")
        assert rows.shape == (5,) and float(prior) == 0.0 and e <= S.BAR
        assert abs(rows.double().sum().item() - float(kl)) <= S.KL_SUM_BAR * abs(float(kl)) + 1e-6
        rows2, _ = samp.kl_rows([params[0].clone(), params[1].clone()])
        assert (np.abs(rows2.double().cpu().numpy() - want) / unit).max() <= S.BAR


# ----------------------------------------------------------------------------
# 5. score.py on the toy data with the reference's small checkpoint
# ----------------------------------------------------------------------------
def _oracle_table():
    """Per-segment float64 oracle scores of the toy segments, by data_ix (the CLI's loader, -b 4)."""
    from modules import data_utils
    from modules.data_utils import Compose
    ck = torch.load(CKPT, map_location="cpu", weights_only=True)
    P, ocfg = S.checkpoint_oracle(ck)
    parser = data_utils.Data_Parser(TOY, ANN)
    fs = parser.get_sample_freq()
    tfm = Compose([data_utils.ToTensor(), data_utils.STFT(int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))),
                   data_utils.Transform(lambda x: (x + 2 ** -15).log() / 1.0)])
    ds = parser.get_data(transform=tfm)
    n = len(ds)
    out = {k: np.zeros(n) for k in ("em", "off", "rows", "share", "length")}
    for packed, is_offset, speaker, ixs in data_utils.DataLoader(ds, batch_size=4):
        sc = S.oracle_scores(P, ocfg, dict(data=packed.data, batch_sizes=packed.batch_sizes, is_offset=is_offset.data,
                                           speakers=speaker), n)
        ix = np.asarray(ixs)
        out["em"][ix], out["off"][ix], out["rows"][ix] = sc["em"], sc["off"], sc["rows"]
        out["share"][ix], out["length"][ix] = sc["prior"] / n, sc["lengths"]
    return out


def test_score_cli_on_toy_data(tmp_path):
    import json
    import score
    z = np.load(os.path.join(GOLDEN, "ref_ckpt_small_encode.npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    base = [CKPT, TOY, ANN, "1.0", "-b", "4"]
    out = os.path.join(str(tmp_path), "s", "scores.csv")
    assert score.main(base + ["-S", out]) == out
    df = pd.read_csv(out)
    n = z["probs"].shape[0]
    assert list(df.columns) == list(score.COLUMNS) + meta["annotation_columns"]
    assert len(df) == n and sorted(df["data_ix"].tolist()) == list(range(n))  # one row per segment
    assert df["data_ix"].tolist()[:4] == list(z["row_order"][:4])  # encode.py's first batch at -b 4, in its order
    assert (df["category_ix"].to_numpy() == z["argmax"][df["data_ix"].to_numpy()]).all()
    want = _oracle_table()
    ix = df["data_ix"].to_numpy()
    assert df["length"].tolist() == want["length"][ix].astype(int).tolist()
    for col, k in (("emission_nll", "em"), ("end_prediction_loss", "off"), ("kl_row", "rows"),
                   ("kl_prior_share", "share")):
        e = np.abs(df[col].to_numpy() - want[k][ix]).max() / np.abs(want[k]).max()
        s = abs(df[col].sum() - want[k].sum()) / abs(want[k].sum())
        print(f"score.py {col}: per segment {e:.2e}, column sum {s:.2e}")
        assert e < S.BAR and s < S.BAR, (col, e, s)
    terms = df[["emission_nll", "end_prediction_loss", "kl_row", "kl_prior_share"]].sum(axis=1).to_numpy()
    assert np.abs(df["total"].to_numpy() - terms).max() <= 1e-9 * np.abs(terms).max()
    total = want["em"].sum() + want["off"].sum() + want["rows"].sum() + want["share"].sum()
    assert abs(df["total"].sum() - total) <= S.BAR * abs(total)  # = num_strings x the mean loss per string
    ann = pd.read_csv(ANN)
    assert df["label"].tolist() == ann["label"][ix].tolist()
    # sampled scores: seeded, reproducible, and not the mean's
    runs = []
    for k in range(2):
        p = os.path.join(str(tmp_path), f"r{k}", "scores.csv")
        score.main(base + ["-S", p, "--sample", "--samples", "2", "--seed", "7"])
        runs.append(pd.read_csv(p))
    assert runs[0].equals(runs[1])
    assert runs[0]["data_ix"].tolist() == df["data_ix"].tolist()
    assert (runs[0]["kl_row"] == df["kl_row"]).all() and not (runs[0]["emission_nll"] == df["emission_nll"]).any()
    other = os.path.join(str(tmp_path), "r8", "scores.csv")
    score.main(base + ["-S", other, "--sample", "--samples", "2", "--seed", "8"])
    assert not (pd.read_csv(other)["emission_nll"] == runs[0]["emission_nll"]).all()
    # a rerun keeps the earlier table as .prev
    score.main(base + ["-S", out])
    assert sorted(os.listdir(os.path.dirname(out))) == ["scores.csv", "scores.csv.prev"]
    assert pd.read_csv(out).equals(pd.read_csv(out + ".prev"))
    with pytest.raises(SystemExit):
        score.Scorer(os.path.join(GOLDEN, "ref_ckpt_plain.pt"))
