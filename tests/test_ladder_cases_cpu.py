"""The conditions that make tests/test_gpu_ladder.py meaningful (no GPU).

Every entry of ``ladder_cases`` has the property its row claims.  The
ladder's arithmetic (csrc/abcd_persist.hip: ``ring_depth``, ``x6_enabled``,
the member / tile counts and LDS sizes of the launchers) is restated here,
not imported from the product: the chunk counts H/16, G*H/16, Fp/16 and
cdiv(Fp,32) + H/32, the ring depth and template they select, the LDS a
persistent form needs against the 160 KiB a workgroup has, the shares that
make h64 idle and h32 ragged, and cdiv(B, 64) per batch.  The float64 and
fp32 oracle steps are finite at every decoder row, and a greedy row's
``weight_ih`` gradient is identically zero in float64 (the GPU test then
requires exact zeros).
"""
import math

import pytest
import torch

import edge_cases as E
import ladder_cases as L

KIB = 1024


def cdiv(a, b):
    return -(-a // b)


def rup16(n):
    return cdiv(n, 16) * 16


def ring_depth(nch):
    return 16 if nch % 16 == 0 else (4 if nch % 4 == 0 else 1)


def enc_fwd(H, G):
    """(template, LDS bytes) of the encoder forward at width H."""
    tp = 4 * 16 * 20 * 4  # four wave-private 16 x 20 transpose tiles
    if H in (64, 128, 256):  # split-fp32 on the bf16 matrix cores: 6 bytes per weight
        return f"enc_fwd_persist<{G},16,{H // 32}>", G * 16 * H * 6 + tp
    return f"enc_fwd_persist<{G},{ring_depth(H // 16)},0>", G * 16 * H * 4 + tp


def enc_bwd(H, G):
    if H == 256:
        return f"enc_bwd_w8<{G}>", None
    if H in (64, 128):
        nsub = H // 16
        return f"enc_bwd_sk<{G},{nsub}>", nsub * 2 * 3 * 64 * 16 + 4 * 16 * 68 * 4 + 4 * 16 * 20 * 4
    return f"enc_bwd_persist<{G},{ring_depth(G * H // 16)}>", 16 * G * H * 4


def dec_fwd(F, H, Hm, rnn, feedback):
    """(kernel, LDS bytes or None) of the decoder forward."""
    Fp, G = rup16(F), L.gates(rnn)
    ncc = (cdiv(Fp, 32) if feedback else 0) + H // 32
    if H == 256 and Hm == 256 and 2 * (Fp // 16) <= H // 8 and ncc in (13, 11, 8):
        return f"dec_fwd_x6<{ncc},8,8,{rnn}>", 64 * 16 * 3 * (2 * ncc + 8 + 16) + 2 * 16 * 16 * 4 + 4 * 16 * 20 * 4
    if G == 3:
        return "per-step decoder forward<3>", None
    M = H // 8
    nchx, nchh, nchm = (Fp // 16 if feedback else 0), H // 16, Hm // 16
    n1, n2 = cdiv(2 * Hm // 16, M), cdiv(Fp // 16, M)
    ncc = ncc if (H == 256 and ncc in (13, 8)) else 0
    cell = 2 * ncc * 3 if ncc else 2 * (nchx + nchh)
    lds = 64 * 16 * (cell + n1 * nchh + 2 * n2 * nchm)
    return (f"dec_fwd_persist<{ncc}>", lds) if lds <= L.LDS_LIMIT else ("per-step decoder forward<4>", None)


def dec_bwd(F, H, Hm, rnn, feedback):
    Fp, G = rup16(F), L.gates(rnn)
    nxs, ncz = (Fp // 16 if feedback else 0), cdiv(Fp, 32)
    if H == 256 and Hm == 256 and Fp // 16 <= H // 8 and nxs in (9, 5, 0) and ncz == (nxs or 9) // 2 + 1:
        return f"dec_bwd_w16<{nxs},{rnn}>", None
    if G == 3:
        return "per-step decoder backward<3>", None
    M = H // 8
    n0, n1 = cdiv(Fp // 16 + H // 16, M), cdiv(2 * Hm // 16, M)
    lds = 64 * 16 * (n0 * (4 * H // 16) + n1 * (Fp // 16) + 2 * Hm // 16)
    return ("dec_bwd_persist", lds) if lds <= L.LDS_LIMIT else ("per-step decoder backward<4>", lds)


def test_every_width_is_a_multiple_of_16():
    assert L.ENC_F == 33 and rup16(L.ENC_F) == 48
    assert L.ENC_WIDTHS == [16, 48, 64, 128, 192, 512]
    for H in L.ENC_ROUTES:
        assert H % 16 == 0
    assert L.DEC_D % 16 == 0 and L.DEC_K % 16 == 0
    for row, d in L.DEC_ROWS.items():
        assert d["H"] % 16 == 0 and d["Hm"] % 16 == 0, row
    # no padded twin is built at these widths: the kernels see the model's own dimensions
    from modules import padding
    assert padding.__name__  # (importable without a GPU)


@pytest.mark.parametrize("H", list(L.ENC_ROUTES))
def test_encoder_routes(H):
    fwd, bwd = L.ENC_ROUTES[H]
    for rnn in ("LSTM", "GRU"):
        G = L.gates(rnn)
        kf, lf = enc_fwd(H, G)
        kb, lb = enc_bwd(H, G)
        assert fwd % G == kf and bwd[rnn] == kb, (H, rnn, kf, kb)
        assert lf <= L.LDS_LIMIT and (lb is None or lb <= L.LDS_LIMIT), (H, rnn, lf, lb)
    # the chunk counts behind the ring depths the table names
    nch = {16: 1, 32: 2, 48: 3, 64: 4, 128: 8, 192: 12, 256: 16, 512: 32}[H]
    assert H // 16 == nch
    want = {16: (1, 4, 1), 32: (1, 4, 1), 48: (1, 4, 1), 192: (4, 16, 4), 512: (16, 16, 16)}.get(H)
    if want:  # (forward, LSTM backward, GRU backward); 64 / 128 / 256 take the split-fp32 forms
        assert (ring_depth(nch), ring_depth(4 * nch), ring_depth(3 * nch)) == want
    assert ring_depth(4 * nch) != 1  # 4 H / 16 is a multiple of 4: enc_bwd_persist<4,1> is never selected


def test_h512_is_the_only_depth16_fp32_ring_and_fits():
    assert [H for H in L.ENC_WIDTHS if enc_fwd(H, 4)[0].endswith(",16,0>")] == [512]
    assert enc_fwd(512, 4)[1] == 128 * KIB + 5 * KIB  # weights + transpose tiles
    assert enc_bwd(512, 4)[1] == 128 * KIB
    assert L.enc_grid(512, 65, "LSTM") == (2 * 2 * 32, 2 * 2 * 32)
    assert L.enc_grid(512, 160, "LSTM")[0] == 192 <= 256  # one workgroup per CU at this LDS size: 256 CUs


def test_encoder_case_lists():
    for H in L.ENC_WIDTHS:
        for rnn in ("LSTM", "GRU"):
            for b in L.BASE_BATCHES:
                assert (H, rnn, b) in L.ENC_CASES
    fwd_templates = {L.ENC_ROUTES[H][0] for H in L.ENC_WIDTHS}
    assert {L.ENC_ROUTES[H][0] for H in L.ENC_EXTRA_WIDTHS} == fwd_templates
    assert len(set(L.ENC_CASES)) == len(L.ENC_CASES) == 44
    bwd_all = {k for H in L.ENC_WIDTHS for k in L.ENC_ROUTES[H][1].values()}
    assert {L.ENC_ROUTES[H][1][r] for H in L.ENC_EXTRA_WIDTHS for r in ("LSTM", "GRU")} == bwd_all


def test_batches_cross_the_64_row_tile():
    assert L.ROWS == 64
    bs = {c: [sum(1 for n in E.CASES[c] if n > t) for t in range(E.CASES[c][0])]
          for c in L.BASE_BATCHES + L.EXTRA_BATCHES}
    assert [cdiv(len(E.CASES[c]), 64) for c in ("b1t1", "b65", "b97steep", "b160")] == [1, 2, 2, 3]
    assert bs["b65"][:3] == [65, 65, 64] and bs["b97steep"] == [97] + [1] * 11  # the 2nd tile empties
    assert 160 % 64 and any(x % 64 for x in bs["b160"])  # three tiles, the last ragged
    assert all(max(E.CASES[c]) <= 12 and len(E.CASES[c]) <= 160 for c in bs)
    assert L.enc_grid(48, 65, "LSTM") == (12, 12) and L.enc_grid(64, 160, "GRU") == (24, 24)
    assert L.enc_grid(256, 65, "LSTM") == (64, 48)  # enc_bwd_w8: 32-row groups of 8
    assert L.enc_grid(48, 65, "LSTM", nd=1) == (6, 6)


@pytest.mark.parametrize("row", list(L.DEC_ROWS))
def test_decoder_routes(row):
    d = L.DEC_ROWS[row]
    fb = not d.get("greedy", False)
    for rnn, (kf, kb) in d["routes"].items():
        if d.get("persist", True):
            assert dec_fwd(d["F"], d["H"], d["Hm"], rnn, fb)[0] == kf.format(rnn=rnn), (row, rnn)
            assert dec_bwd(d["F"], d["H"], d["Hm"], rnn, fb)[0] == kb.format(rnn=rnn), (row, rnn)
        else:
            assert (kf, kb) == ("per-step decoder forward<4>", "per-step decoder backward<4>")
            exp = L.dec_expected(row, rnn, 65)
            assert exp["enc_fwd"] == "per-step rnn_fwd_step<4>" and exp["enc_bwd"] == "per-step launch_bwd_step<4>"
        assert d["H"] in L.ENC_ROUTES  # its encoder side is a pinned row too


def test_decoder_chunk_counts():
    ncc = lambda F, H, fb: (cdiv(rup16(F), 32) if fb else 0) + H // 32  # noqa: E731
    assert (rup16(65), rup16(129), rup16(257), rup16(33)) == (80, 144, 272, 48)
    assert ncc(65, 256, True) == 11 and 80 // 16 == 5            # f65
    assert ncc(129, 256, False) == 8                             # greedy: no x chunks
    assert ncc(129, 256, True) == 13                             # hm128: the cell of the c2 form, Hm != 256
    assert 2 * (272 // 16) == 34 > 256 // 8                      # f257: more emit tiles than members
    assert ncc(257, 256, True) == 17                             # ... and no compiled cell chunk count
    # f257's BPTT: 33 x/h tiles on 32 members double the gate image
    assert dec_bwd(257, 256, 256, "LSTM", True) == ("per-step decoder backward<4>", 177 * KIB)
    assert dec_bwd(129, 256, 128, "LSTM", True) == ("dec_bwd_persist", 89 * KIB)
    # h64: 8 members, 6 mlp tiles and 3 emit tiles -> one tile each at most, 2 and 5 members idle
    M = 64 // 8
    assert (M, 2 * 48 // 16, 48 // 16) == (8, 6, 3) and cdiv(6, M) == cdiv(3, M) == 1
    # member m owns tiles m, m + M, ...
    share = lambda nt, M: [(nt - 1 - m) // M + 1 if m < nt else 0 for m in range(M)]  # noqa: E731
    assert share(6, M) == [1] * 6 + [0] * 2 and share(3, M) == [1] * 3 + [0] * 5
    # h32: 4 members, 10 mlp tiles and 9 emit tiles -> LDS for 3 each, uneven shares
    M = 32 // 8
    assert (M, 2 * 80 // 16, 144 // 16) == (4, 10, 9)
    assert cdiv(10, M) == cdiv(9, M) == 3 and 10 % M and 9 % M
    assert share(10, M) == [3, 3, 2, 2] and share(9, M) == [3, 2, 2, 2]


def test_decoder_case_lists():
    names = set()
    for row, rnn, b in L.DEC_CASES:
        assert rnn in L.DEC_ROWS[row]["routes"] and b in L.BASE_BATCHES + L.EXTRA_BATCHES
    for row, d in L.DEC_ROWS.items():
        for rnn, ks in d["routes"].items():
            names |= {k.format(rnn=rnn) for k in ks}
            assert all((row, rnn, b) in L.DEC_CASES for b in L.BASE_BATCHES)
    extra = {k.format(rnn=rnn) for row, rnn in L.DEC_EXTRA for k in L.DEC_ROWS[row]["routes"][rnn]}
    assert extra == names  # every decoder kernel name runs the extra batches once
    assert len(set(L.DEC_CASES)) == len(L.DEC_CASES) == 2 * 13 + 2 * 9
    assert L.dec_grid("dec_bwd_w16<5,LSTM>", 256, 65) == 48 and L.dec_grid("dec_fwd_x6<11,8,8,GRU>", 256, 65) == 64
    assert L.dec_grid("dec_fwd_persist<0>", 32, 160) == 12
    assert L.dec_grid("per-step decoder forward<3>", 256, 65) is None
    exp = L.dec_expected("f65", "GRU", 65)
    assert exp == {"enc_fwd": "enc_fwd_persist<3,16,8> grid 64", "enc_bwd": "enc_bwd_w8<3> grid 48",
                   "dec_fwd": "dec_fwd_x6<11,8,8,GRU> grid 64", "dec_bwd": "dec_bwd_w16<5,GRU> grid 48"}
    exp = L.dec_expected("h32", "LSTM", 160)
    assert exp == {"enc_fwd": "enc_fwd_persist<4,1,0> grid 12", "enc_bwd": "enc_bwd_persist<4,4> grid 12",
                   "dec_fwd": "dec_fwd_persist<0> grid 12", "dec_bwd": "dec_bwd_persist grid 12"}


ROW_RNN = [(row, rnn) for row, d in L.DEC_ROWS.items() for rnn in d["routes"]]


@pytest.mark.parametrize("row,rnn", ROW_RNN)
def test_oracle_steps_are_finite(row, rnn):
    ref = L.dec_reference(row, rnn, "b65")
    r32, r64 = ref["r32"], ref["r64"]
    assert all(g.dtype == torch.float64 for g in r64["grads"].values())
    for r in (r32, r64):
        assert math.isfinite(r["total"]) and r["total"] > 0
        assert all(torch.isfinite(g).all() for g in r["grads"].values())
        assert all(torch.isfinite(r["out"][k]).all() for k in (
            "loss", "em", "off", "kl", "last_hidden", "logits", "feats", "mu", "lv", "flatten_out", "offset_logits"))
    err = E.oracle_errors(ref)
    assert all(math.isfinite(a) and math.isfinite(b) for a, b in err.values())
    assert set(err) >= {"g/" + k for k in r64["grads"]} | {"d/" + k for k in r64["grads"]} | {"norm", "logits"}
    zero = {k for k, g in r64["grads"].items() if not g.any()}
    assert zero == L.zero_grads(row, "b65"), zero
    if L.DEC_ROWS[row].get("greedy"):
        assert zero == {"decoder/rnn_cell.cell.weight_ih"}
    else:
        assert not zero


def test_encoder_reference_is_torch_in_both_precisions():
    ref = L.enc_reference(48, "LSTM", "b65")
    assert ref["r64"]["last_hidden"].dtype == torch.float64 and ref["r32"]["last_hidden"].dtype == torch.float32
    assert ref["r64"]["last_hidden"].shape == (65, 4 * 48)
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    assert set(ref["r64"]) == {"last_hidden"} | {f"g/{n}_l0{s}" for n in names for s in ("", "_reverse")}
    assert all(math.isfinite(a) and math.isfinite(b) and a <= 1e-5 and b <= 1e-5 for a, b in ref["e32"].values())
    # the same operation as the oracle's encoder
    from oracle import abcd_oracle as O
    P64 = {k: v.double() for k, v in ref["P"].items()}
    lh = O.encoder_forward(P64, ref["packed"].data.double(), ref["packed"].batch_sizes, ref["ocfg"])
    assert E.rel_err(lh, ref["r64"]["last_hidden"]) < 1e-12
    two = L.enc_reference(48, "LSTM", "b65", 2, True)
    assert two["r64"]["last_hidden"].shape == (65, 2 * 4 * 48) and "g/weight_hh_l1_reverse" in two["r64"]
    uni = L.enc_reference(48, "LSTM", "b65", 1, False)
    assert uni["r64"]["last_hidden"].shape == (65, 2 * 48) and "g/weight_hh_l0_reverse" not in uni["r64"]
    # one frame: h_0 = 0, so the recurrent weights get no gradient (the GPU must give exact zeros)
    one = L.enc_reference(48, "GRU", "b1t1")
    assert not one["r64"]["g/weight_hh_l0"].any() and not one["r64"]["g/weight_hh_l0_reverse"].any()


def test_fast_cell_forms_move_encoder_tensors(monkeypatch):
    """What test_gpu_ladder.R_ENCODER is attributed to, checked without a GPU.
    The recurrent kernels' activations are fsigmoid / ftanh (abcd_common.h:
    1 / (1 + e^-x), 1 - 2 / (1 + e^2x)), whose error is absolute (~1e-7) where
    torch's is relative.  The fp32 oracle's encoder run with those forms,
    against the same fp32 oracle with torch's (same machine, same summation
    order: the difference is the forms alone), moves the final state and the
    bias gradients of a single frame at H = 512 by what the GPU shows against
    float64 (1.6e-6 per block in profiles/parity_errors.json): several times
    the fp32 reference's own error, and far under the hard 1e-4."""
    from oracle import abcd_oracle as O
    ref = L.enc_reference(512, "LSTM", "b1t1")

    def run():
        P = {k: v.clone().requires_grad_(k.startswith("encoder/")) for k, v in ref["P"].items()}
        lh = O.encoder_forward(P, ref["packed"].data, ref["packed"].batch_sizes, ref["ocfg"])
        (lh * ref["dout"]).sum().backward()
        out = {"last_hidden": lh.detach()}
        out.update(("g/" + k[len("encoder/rnn."):], p.grad) for k, p in P.items() if p.grad is not None)
        return out

    base = run()
    with monkeypatch.context() as m:
        m.setattr(torch, "tanh", lambda x: 1.0 - 2.0 / (1.0 + torch.exp(2.0 * x)))
        m.setattr(torch, "sigmoid", lambda x: 1.0 / (1.0 + torch.exp(-x)))
        fast = run()
    assert E.rel_err(base["last_hidden"], ref["r32"]["last_hidden"]) < 1e-6  # the oracle's encoder is torch's
    for k in ("last_hidden", "g/bias_ih_l0", "g/bias_ih_l0_reverse", "g/weight_ih_l0"):
        shift, e32 = E.block_err(fast[k], base[k]), ref["e32"][k][1]
        print(k, "shift %.2e e32 %.2e" % (shift, e32))
        assert 5e-7 <= shift <= 5e-6 and shift >= 3 * e32, (k, shift, e32)
        assert E.rel_err(fast[k], base[k]) <= 1e-6
