"""The conditions that make tests/test_gpu_sampler_widths.py and
tests/test_gpu_philox.py meaningful (no GPU).

* the numpy Philox4x32-10 of ``sampler_cases`` gives Random123's three known
  answers, and its transforms are the ones the kernels state (u01 in (0, 1],
  the counter's carry into the high word);
* every row of every ABCD case clears ``ARGMAX_GAP`` in float64 and the table
  of redrawn rows is what ``find_redraws`` gives;
* each case has the property its name claims: KPL, tile count, 16-column
  subtile counts, which LDS pitch wins, which side of the fused / per-method
  threshold it is on;
* the zero-padded twin (modules/padding.py), with the kernels' masking of the
  padding categories and 1 / sqrt(real D) scale, agrees with the un-padded
  model in float64, and its padding stays exactly 0;
* the unit of the GPU comparison, the fp32 oracle against the float64 one, is
  finite and below 1e-5 for every tensor (measured 2e-7 .. 3e-6).
"""
import math

import numpy as np
import pytest
import torch

import sampler_cases as S


def test_philox_known_answers():
    for ctr, key, want in S.KNOWN_ANSWERS:
        got = S.philox4x32_10(ctr, key)
        assert [int(x) for x in got] == list(want), ([hex(int(x)) for x in got], [hex(x) for x in want])
    # vectorised over the counter: the same words as one call each
    ctrs = np.array([k[0] for k in S.KNOWN_ANSWERS], dtype=np.uint64).T
    got = S.philox4x32_10(tuple(ctrs), S.KNOWN_ANSWERS[0][1])
    assert [int(x) for x in got[:, 0]] == list(S.KNOWN_ANSWERS[0][2])
    # words(): counter = (low, high word of the index, 0, 0), key = (low, high word of the seed)
    seed, idx = (0x299f31d0 << 32) | 0xa4093822, (0x85a308d3 << 32) | 0x243f6a88
    assert [int(x) for x in S.words(seed, idx)] == [int(x) for x in
                                                    S.philox4x32_10((0x243f6a88, 0x85a308d3, 0, 0),
                                                                    (0xa4093822, 0x299f31d0))]


def test_philox_transforms():
    assert S.u01(0) == 2.0 ** -24 and S.u01(0xFFFFFFFF) == 1.0 and S.u01(0xFF) == 2.0 ** -24
    # offset + i carries into the counter's high word
    idx = S.indices(2 ** 32 - 2, 4)
    assert [int(i) for i in idx] == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    w = S.words(1234, idx)
    assert [int(x) for x in w[:, 2]] == [int(x) for x in S.philox4x32_10((0, 1, 0, 0), (1234, 0))]
    assert [int(x) for x in w[:, 2]] != [int(x) for x in S.philox4x32_10((0, 0, 0, 0), (1234, 0))]
    n = 1 << 16
    z, g = S.normal(7, S.indices(0, n)), S.gumbel(7, S.indices(0, n))
    assert np.isfinite(z).all() and np.isfinite(g).all()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert abs(g.mean() - 0.5772) < 0.02 and abs(g.var() - math.pi ** 2 / 6) < 0.05
    for p in (0.0, 0.2, 0.5):
        keep, val = S.dropout(7, S.indices(0, n), p)
        assert abs(keep.mean() - (1.0 - p)) < 0.01 and val == 1.0 / (1.0 - p)
    assert S.dropout(7, S.indices(0, n), 0.0)[0].all()


def test_case_table():
    assert list(S.CASES) == ["k16_b520", "k80_b17", "k144_b33_tau01", "k272pad_b15", "k528_b1_peaked",
                             "k1024pad_b16", "hm512_b31", "k1040_b17", "lds_b17", "plain_b17"]
    for case in S.CASES:
        s = S.spec(case)
        assert all(x % 16 == 0 for x in (s.E, s.Hm, s.D, s.K)), case  # samp_check
        assert 0 < s.Dv <= s.D and s.Kv <= s.K, case
        inp = S.inputs(case)
        assert inp["h"].shape == (s.B, s.E) and inp["d_feats"].shape == (s.B, s.Dv)
        assert inp["noise"].shape == (s.B, s.Dv if s.plain else s.Kv)
        assert float(inp["d_kl"]) == pytest.approx(1.0 / s.B)
        if not s.plain:
            assert S.params(case)[S.PSL].shape == (s.Kv,) and S.params(case)[S.CB].shape == (s.Dv, s.Kv)
            assert float(S.params(case)["feature_sampler/prior_concentration"]) == pytest.approx(s.a0)


def test_case_geometry():
    sub = lambda n: n // 16  # noqa: E731  (16-column subtiles of a product)
    sp = {c: S.spec(c) for c in S.CASES}
    assert [S.kpl(sp[c].K) for c in S.ABCD_CASES] == [1, 2, 4, 8, 16, 16, 1, 32, 1]
    assert [S.kpl(k) for k in (64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    s = sp["k16_b520"]   # one subtile for 8 waves; 33 tiles: one pass of the unrolled-32 loop + 1 remainder
    assert sub(s.K) == sub(s.D) == 1 < S.HEAD_WAVES and S.tiles(s.B) == 33 and s.B % 16
    s = sp["k80_b17"]    # odd subtile counts (the bok tail of tile_mma<2,...>) and fewer than 8; 2nd tile: one row
    assert (sub(s.Hm), sub(s.K), sub(s.D)) == (3, 5, 2) and S.tiles(s.B) == 2 and s.B - 16 == 1
    s = sp["k144_b33_tau01"]
    assert 128 < s.K <= 256 and s.tau == 0.1 and s.a0 == 0.1 and S.tiles(s.B) == 3 and sub(s.K) % 2 == 1
    s = sp["k272pad_b15"]
    assert 256 < s.K <= 512 and S.tiles(s.B) == 1 and s.B < 16 and (s.Kv, s.Dv) == (260, 40) and sub(s.K) == 17
    s = sp["k528_b1_peaked"]  # one tile transposes the whole codebook and W2
    assert 512 < s.K < 1024 and s.B == 1 and s.cb_scale == 4.0 and sub(s.K) == 33
    s = sp["k1024pad_b16"]
    assert s.K == 1024 and s.Kv == 1000 and s.B == 16 and S.tiles(s.B) == 1
    s = sp["hm512_b31"]  # LDS pitches come from Hm and D, not K
    assert s.Hm > s.K and s.D > s.K and S.tiles(s.B) == 2
    assert sp["k1040_b17"].K > 1024
    s = sp["lds_b17"]
    assert s.K <= 1024 and S.head_fwd_lds(s.Hm, s.D, s.K) > S.HEAD_LDS_MAX < S.head_bwd_lds(s.Hm, s.D, s.K)
    assert [c for c in S.ABCD_CASES if not S.fused(c)] == list(S.FALLBACK) and not S.fused("plain_b17")
    s = sp["plain_b17"]
    assert s.plain and s.Dv == 20 and s.D == 32 and s.B % 16 == 1
    # the peaked case: 4 x the codebook is 4 x the logits (std ~1 over 528 categories where 1 x gives ~0.26);
    # its softmax tops out ~7 x higher than the 1 x model's, and the tau = 0.5 Gumbel sample above 0.5
    r = S.reference("k528_b1_peaked", "gumbel")["r64"]
    q, q1 = torch.softmax(r["logits"], -1), torch.softmax(r["logits"] / 4, -1)
    y = torch.softmax((r["logits"] + S.inputs("k528_b1_peaked")["noise"].double()) / 0.5, -1)
    assert float(q.max()) > 5 * float(q1.max()) and float(y.max()) > 0.5


@pytest.mark.parametrize("case", S.ABCD_CASES)
def test_argmax_gap_and_redraw_table(case):
    gaps = S.top2_gaps(S.logits64(case, S.REDRAW.get(case)))
    assert float(gaps.min()) >= S.REDRAW_GAP > S.ARGMAX_GAP, (case, float(gaps.min()))
    assert S.find_redraws(case) == S.REDRAW.get(case, {}), "REDRAW is stale: python tests/sampler_cases.py"
    ref = S.reference(case, "gumbel")
    assert torch.equal(ref["r64"]["logits"], S.logits64(case, S.REDRAW.get(case)))
    assert float(S.top2_gaps(ref["r64"]["logits"]).min()) >= S.ARGMAX_GAP


def test_redraw_is_needed():
    assert float(S.top2_gaps(S.logits64("k16_b520", None)).min()) < S.ARGMAX_GAP


@pytest.mark.parametrize("case", ["k272pad_b15", "k1024pad_b16", "plain_b17"])
def test_padded_twin_agrees_in_float64(case):
    """The twin's parameters at the padded sizes, with what the kernels know of
    the real sizes (the first Kv logit columns are the categories, the scale is
    1 / sqrt(Dv), plain: zero noise in the padding columns): the un-padded
    model's values and gradients at the real positions, exact zeros elsewhere."""
    from oracle import abcd_oracle as O
    s, inp = S.spec(case), S.inputs(case)
    r64 = S.reference(case, "plain" if s.plain else "gumbel")["r64"]
    twin = S.padded_params(case)
    for k, v in S.params(case).items():
        if k.endswith("prior_concentration"):
            continue
        assert tuple(twin[k].shape) == S.padded_shape(case, k), k
        val, rest = S.valid_slice(case, k, twin[k])
        assert torch.equal(val, v) and not rest.any(), k
    P = {k: v.double().requires_grad_(not k.endswith("prior_concentration")) for k, v in twin.items()}
    h = inp["h"].double().requires_grad_(True)
    pad = torch.nn.functional.pad
    d_feats = pad(inp["d_feats"].double(), (0, s.D - s.Dv))
    if s.plain:
        mu, lv = O.plain_params(P, h)
        assert not mu[:, s.Dv:].any() and not lv[:, s.Dv:].any()
        feats = mu + (0.5 * lv).exp() * pad(inp["noise"].double(), (0, s.D - s.Dv))
        kl = O.gaussian_kl(mu, lv)
        logits = torch.cat([mu[:, :s.Dv], lv[:, :s.Dv]], -1)
    else:
        u = O.mlp(h, P, "feature_sampler/to_code_like.whole_network")
        assert not u[:, s.Dv:].any()
        full = u @ P[S.CB] / math.sqrt(s.Dv)
        assert not full[:, s.Kv:].any()
        logits = full[:, :s.Kv]
        Pv = dict(P)
        Pv[S.CB], Pv[S.PSL] = P[S.CB][:, :s.Kv], P[S.PSL][:s.Kv]
        feats = O.abcd_sample(Pv, logits, inp["noise"].double(), s.tau)
        kl = O.digamma_kl(Pv, logits, S.N_DATA)
    assert not feats[:, s.Dv:].any()
    ((feats * d_feats).sum() + inp["d_kl"].double() * kl).backward()
    assert S.rel_err(logits, r64["logits"]) < 1e-12 and S.rel_err(feats[:, :s.Dv], r64["feats"]) < 1e-12
    assert abs(float(kl) - r64["kl"]) <= 1e-12 * abs(r64["kl"])
    assert S.rel_err(h.grad, r64["d_h"]) < 1e-12
    for k in S.grad_names(case):
        val, rest = S.valid_slice(case, k, P[k].grad)
        assert S.rel_err(val, r64["g/" + k]) < 1e-12, k
        assert not rest.any(), k


@pytest.mark.parametrize("case", list(S.CASES))
def test_fp32_oracle_error_is_small(case):
    modes = ("plain",) if S.spec(case).plain else S.MODES
    for mode in modes:
        ref = S.reference(case, mode)
        for k, (rel, blk) in ref["e32"].items():
            print(f"{case}-{mode} {k}: e32 rel {rel:.2e} blk {blk:.2e}")
            assert math.isfinite(rel) and math.isfinite(blk), (mode, k)
            assert rel < 1e-5 and blk < 1e-5, (mode, k, rel, blk)
        r32, r64 = ref["r32"], ref["r64"]
        assert abs(r32["kl"] - r64["kl"]) <= 1e-4 * abs(r64["kl"])
        assert ref["r64"]["logits"].shape[0] == S.spec(case).B


def test_sequential_row_sum_moves_codebook_gradient():
    """What test_gpu_sampler_widths.py raises R for at k16_b520: the codebook
    gradient dC = [d_feats; U]^T [Y; dL / sqrt(D)] is one 16 x 16 output tile
    there, so the GPU sums its 2 B = 1040 rows in one fp32 chain, where torch's
    GEMM blocks the reduction.  The same fp32 operands summed row by row on
    the CPU err 3 x more than summed by torch's matmul, and land where the GPU
    does (1.1e-6 of the tensor's max)."""
    from oracle import abcd_oracle as O
    case, mode = "k16_b520", "softmax"
    s, inp = S.spec(case), S.inputs(case)
    P = {k: v.clone() for k, v in S.params(case).items()}
    u = O.mlp(inp["h"], P, S._PRE)
    logits = (u @ P[S.CB] / math.sqrt(s.D)).requires_grad_(True)
    y = torch.softmax(logits, -1)
    ((y @ P[S.CB].t() * inp["d_feats"]).sum() + inp["d_kl"] * O.digamma_kl(P, logits, S.N_DATA)).backward()
    A = torch.cat([inp["d_feats"], u], 0)                               # 2B x D
    Bm = torch.cat([y.detach(), logits.grad / math.sqrt(s.D)], 0)       # 2B x K
    r64 = S.reference(case, mode)["r64"]["g/" + S.CB]
    blocked = S.rel_err(A.t() @ Bm, r64)
    acc = torch.zeros(s.D, s.K)
    for i in range(A.shape[0]):
        acc = acc + A[i][:, None] * Bm[i][None, :]
    chain = S.rel_err(acc, r64)
    print(f"dC at {case}: torch matmul {blocked:.2e}, one fp32 chain over {A.shape[0]} rows {chain:.2e}")
    assert A.shape[0] == 1040 and blocked < 5e-7
    assert chain > 2.5 * blocked and 6e-7 < chain < 2e-6


def test_single_term_references_sum_to_both():
    """The float64 gradients of the two terms alone (the d_kl = NULL and
    d_feats = NULL branches of the backward) add up to the gradient of both."""
    both, fe, kl = (S.reference("k80_b17", "gumbel", t)["r64"] for t in ("both", "feats", "kl"))
    for k in S.tensor_keys("k80_b17")[2:]:
        assert S.rel_err(fe[k] + kl[k], both[k]) < 1e-12, k
    assert not fe["g/" + S.PSL].any()   # the sample does not read posterior_shape_logits
    assert kl["g/" + S.CB].any()        # the KL reaches the codebook through the logits
