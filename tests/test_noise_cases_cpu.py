"""The conditions that make tests/test_gpu_decoder_noise.py meaningful (no GPU).

* Part A: every case's mask has a kept and a dropped entry in column F - 1 of
  the rows the decoder reads (steps >= 1), and the float64 oracle run with a
  mask a mistaken kernel would see -- none, the row before, the column before,
  the flat block re-read with pitch Fp -- moves a tensor the GPU test judges by
  more than 100 x that tensor's bound.  The routes the GPU test asserts are
  ``ladder_cases.dec_expected`` for the ladder rows and, for the first rung,
  ``test_gpu_edges.KERNELS`` with ``ladder_cases``' grids.
* Part B: the Philox bookkeeping of ``modules.noise`` (the decoder's block at
  (S, O), the mask's behind it), four wrong streams that are O(1) off in every
  case's block, and the placement of the counter carry.
* Part C: without the inter-layer mask the float64 ``weight_ih_l1`` gradient
  moves by more than 100 x its bound.
"""
import numpy as np
import pytest
import torch

import edge_cases as E
import ladder_cases as L
import noise_cases as NC
import sampler_cases as S
import test_gpu_edges as TE
import test_gpu_ladder as TL

W_IH, W_HH = "decoder/rnn_cell.cell.weight_ih", "decoder/rnn_cell.cell.weight_hh"
MULTI = [k for k in NC.MASK_CASES if len(NC.batch_sizes(k[2])) >= 2]
_ids = ["-".join(k) for k in MULTI]


def test_case_tables_are_what_the_issue_lists():
    assert len(NC.MASK_CASES) == 22 and len(set(NC.MASK_CASES)) == 22
    assert [k for k in NC.MASK_CASES if k not in MULTI] == [(NC.RUNG1, "LSTM", "b1t1"), (NC.RUNG1, "GRU", "b1t1")]
    for row, rnn, case in NC.MASK_CASES:
        assert not NC.dims(row).get("greedy"), row  # a greedy decoder is p = 1: the C ABI rejects a mask without feedback
        assert len(E.CASES[case]) <= 160 and E.CASES[case][0] <= 12
        cfg = NC.config(row, rnn, len(E.CASES[case]))
        assert (cfg["D"], cfg["K"]) == (32, 16)
    assert set(NC.MASK_FRAME_CASES) <= set(NC.MASK_CASES)
    assert list(NC.STALE_CASES) == ["rung1-LSTM-b33", "hm128-LSTM-b65"]
    assert len(NC.ENC_DROP_CASES) == 8


def test_mask_reseed_table_is_current():
    assert {k: NC.find_mask_reseed(k) for k in NC.MASK_CASES if NC.find_mask_reseed(k)} == NC.MASK_RESEED


@pytest.mark.parametrize("key", MULTI, ids=_ids)
def test_last_column_holds_kept_and_dropped(key):
    row, rnn, case = key
    mask, bsz = NC.mask_of(key), NC.batch_sizes(case)
    F = NC.dims(row)["F"]
    assert mask.shape == (sum(bsz), F) and F % 16 == 1  # column F - 1 is alone in its 16-wide tile
    assert set(mask.unique().tolist()) == {0.0, float(torch.tensor(1.0) / torch.tensor(0.7))}
    assert NC.last_column_mixed(mask, bsz)
    assert torch.equal(mask, NC.draw_mask(sum(bsz), F, NC.mask_seed(key)))


# The pitch-Fp re-read of a b97steep mask is "no mask": the rows of steps >= 1
# start at packed row 97, and 97 * Fp is past the L x F block at every width
# (97 * 144 > 108 * 129, 97 * 80 > 108 * 65, 97 * 48 > 108 * 33).  It is skipped there.
def _coincides(key, kind):
    bsz = NC.batch_sizes(key[2])
    mask = NC.mask_of(key)
    return kind == "pitch" and NC.same_for_the_decoder(NC.wrong_mask(mask, "pitch", bsz),
                                                       NC.wrong_mask(mask, "none", bsz), bsz)


def test_pitch_variant_is_no_mask_exactly_at_b97steep():
    assert [k for k in MULTI if _coincides(k, "pitch")] == [k for k in MULTI if k[2] == "b97steep"]
    for row in ("f65", "hm128", "h64", NC.RUNG1):
        F = NC.dims(row)["F"]
        assert 97 * NC.rup16(F) > 108 * F


def _bound(key, tensor, e32):
    table = TE.R_TENSOR if key[0] == NC.RUNG1 else TL.R_TENSOR
    return table.get(tensor, 4.0) * e32 + 1e-7


@pytest.mark.parametrize("key", MULTI, ids=_ids)
def test_wrong_masks_move_the_float64_oracle(key):
    row, rnn, case = key
    ref = NC.mask_reference(*key)
    bsz = NC.batch_sizes(case)
    r64 = ref["r64"]
    assert all(torch.isfinite(g).all() for g in r64["grads"].values())
    e32 = E.oracle_errors(ref)
    e32["flatten_out"] = NC.frame_e32(ref)["flatten_out"]
    mask = ref["noise"]["xmask"]
    for kind in NC.WRONG_MASKS:
        wrong = NC.wrong_mask(mask, kind, bsz)
        if _coincides(key, kind):
            continue
        assert not NC.same_for_the_decoder(wrong, mask, bsz), kind
        w = E.oracle64(ref["ocfg"], ref["P"], ref["batch"], dict(ref["noise"], xmask=wrong), E.N_DATA)
        moved = {"g/" + W_IH: E.rel_err(w["grads"][W_IH], r64["grads"][W_IH]),
                 "g/" + W_HH: E.rel_err(w["grads"][W_HH], r64["grads"][W_HH]),
                 "flatten_out": E.rel_err(w["out"]["flatten_out"], r64["out"]["flatten_out"])}
        ratio = {k: v / _bound(key, k, e32[k][0]) for k, v in moved.items()}
        print(f"{'-'.join(key)} {kind}: " + ", ".join(f"{k} {moved[k]:.2e} ({ratio[k]:.0f} x bound)" for k in moved))
        assert max(ratio.values()) > 100.0, (kind, moved, ratio)


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_one_frame_has_no_use_for_the_mask(rnn):
    ref = NC.mask_reference(NC.RUNG1, rnn, "b1t1")
    assert "xmask" in ref["noise"] and ref["noise"]["xmask"].shape == (1, 129)
    assert not ref["r64"]["grads"][W_IH].any()
    assert W_IH in E.ZERO_GRADS["b1t1"]


def test_routes_come_from_the_existing_tables():
    for row, rnn, case in NC.MASK_CASES + [(c["row"], c["rnn"], c["case"]) for c in NC.STREAM_CASES.values()]:
        B = len(E.CASES[case])
        exp = NC.expected(row, rnn, B)
        if row != NC.RUNG1:
            assert exp == L.dec_expected(row, rnn, B)
            continue
        grids = {"enc_fwd": (B + 63) // 64 * 32, "enc_bwd": (B + 31) // 32 * 16, "dec_fwd": (B + 63) // 64 * 32,
                 "dec_bwd": (B + 31) // 32 * 16}  # test_gpu_edges' own grid arithmetic
        for role, kern in zip(("enc_fwd", "enc_bwd", "dec_fwd", "dec_bwd"), TE.KERNELS[rnn]):
            assert exp[role] == f"{kern} grid {grids[role]}", (role, exp[role])
    # the forms Part B names
    assert NC.expected("greedy", "LSTM", 65)["dec_fwd"].startswith("dec_fwd_x6<8,")
    assert NC.expected("hm128", "LSTM", 65)["dec_fwd"].startswith("dec_fwd_persist<13>")
    assert NC.expected("h64", "LSTM", 65)["dec_fwd"].startswith("dec_fwd_persist<0>")
    assert NC.expected("stepwise", "LSTM", 65)["dec_fwd"] == "per-step decoder forward<4>"
    for name, idle in NC.IDLE_MEMBERS.items():  # 32 members, a mu and an lv member per 16-wide emit tile
        assert idle == 32 - 2 * (NC.rup16(NC.stream_spec(name)["F"]) // 16)


# ---------------------------------------------------------------------------- Part B
def test_philox_bookkeeping_of_the_decoder_draw(monkeypatch):
    """noise.decoder_noise with an empty replay queue: the decoder's block is
    (S, O), the mask's starts 4 * ceil(L F / 4) counters on, and the state ends
    behind both."""
    from modules import noise
    saved = noise.get_state()
    calls = []

    def stub(shape, p, device):
        calls.append((shape, p) + noise.philox(shape[0] * shape[1]))
        return "mask"

    monkeypatch.setattr(noise, "dropout_noise", stub)
    try:
        for name in NC.STREAM_CASES:
            c = NC.stream_spec(name)
            bsz = NC.batch_sizes(c["case"])
            n = c["L"] * c["F"]
            del calls[:]
            noise.set_state({"mode": "philox", "seed": c["seed"], "offset": c["offset"]})
            eps, s, o, xm = noise.decoder_noise(bsz, c["F"], c["p"], "cpu")
            assert eps is None and (s, o) == (c["seed"], c["offset"]), name
            end = c["offset"] + 4 * L.cdiv(n, 4)
            if c["p"]:
                assert xm == "mask" and calls == [((c["L"], c["F"]), c["p"], c["seed"], end)]
                assert NC.mask_offset(c["offset"], c["L"], c["F"]) == end
                end += 4 * L.cdiv(n, 4)
            else:
                assert xm is None and not calls
            assert noise.get_state()["offset"] == end
    finally:
        noise.set_state(saved)
    assert sum(1 for c in NC.STREAM_CASES.values() if c.get("p")) == 1  # the mask's block: first rung LSTM b33 only
    assert S.indices(5, 3).tolist() == [5, 6, 7]


@pytest.mark.parametrize("name", list(NC.STREAM_CASES))
def test_wrong_streams_are_far_from_the_right_one(name):
    c = NC.stream_spec(name)
    right = NC.stream(c["seed"], c["offset"], c["L"], c["F"])
    assert right.shape == (c["L"], c["F"]) and np.isfinite(right).all()
    for kind in NC.WRONG_STREAMS:
        wrong = NC.wrong_stream(c["seed"], c["offset"], c["L"], c["F"], kind)
        assert np.abs(wrong - right).max() > 1.0, kind
    assert np.abs(np.zeros_like(right) - right).max() > 1.0  # a lost draw
    # every 64-row tile of every step: a stale block of another (seed, offset) is far off in it
    other = NC.stream(*NC.STALE_CASES.get(name, (c["seed"] + 1, c["offset"])), c["L"], c["F"])
    for lo, hi in NC.tiles_with_rows(c["case"]):
        assert np.abs(other[lo:hi] - right[lo:hi]).max() > 1.0, (lo, hi)


@pytest.mark.parametrize("name", list(NC.CARRY_AT))
def test_counter_carry_sits_inside_a_row_of_the_second_tile(name):
    c = NC.stream_spec(name)
    step, b = NC.CARRY_AT[name]
    bsz = NC.batch_sizes(c["case"])
    assert c["seed"] == 0x9E3779B97F4A7C15
    assert step >= 1 and 64 <= b < min(128, bsz[step])
    rr = sum(bsz[:step]) + b
    first, last = c["offset"] + rr * c["F"], c["offset"] + rr * c["F"] + c["F"] - 1
    assert first < 2 ** 32 <= last  # the low word wraps between two columns of this row
    assert c["offset"] + c["L"] * c["F"] > 2 ** 32 > c["offset"]
    idx = S.indices(c["offset"], c["L"] * c["F"])
    assert int(idx[rr * c["F"]]) >> 32 == 0 and int(idx[(rr + 1) * c["F"] - 1]) >> 32 == 1


def test_stale_cases_use_another_seed_and_offset():
    for name, (s2, o2) in NC.STALE_CASES.items():
        c = NC.stream_spec(name)
        assert s2 != c["seed"] and o2 != c["offset"]


# ---------------------------------------------------------------------------- Part C
@pytest.mark.parametrize("H,rnn,case", NC.ENC_DROP_CASES)
def test_inter_layer_mask_moves_weight_ih_l1(H, rnn, case):
    ref = NC.enc_drop_reference(H, rnn, case)
    mask = ref["mask"]
    assert mask.shape == (sum(E.CASES[case]), 2 * H)
    assert set(mask.unique().tolist()) == {0.0, float(torch.tensor(1.0) / torch.tensor(0.75))}
    assert set(ref["r64"]) == set(L.enc_reference(H, rnn, case, 2, True)["r64"])  # the tensors test_gpu_ladder judges
    k = "g/weight_ih_l1"
    moved = E.rel_err(ref["r64_nomask"][k], ref["r64"][k])
    bound = TL.bound(TL.R_ENCODER.get(k, TL.R_DEFAULT), ref["e32"][k][0])
    print(f"h{H}-{rnn}-{case}: {k} moves {moved:.2e} without the mask, bound {bound:.2e}")
    assert moved > 100.0 * bound
    assert L.enc_expected(H, rnn, len(E.CASES[case]))["enc_fwd"].startswith("enc_fwd_persist<")


def test_hmask_default_leaves_the_encoder_unchanged():
    from oracle import abcd_oracle as O
    base = L.enc_reference(48, "LSTM", "b65", 2, True)
    a = O.encoder_forward(base["P"], base["packed"].data, base["packed"].batch_sizes, base["ocfg"])
    b = O.encoder_forward(base["P"], base["packed"].data, base["packed"].batch_sizes, base["ocfg"], hmask=None)
    ones = [torch.ones(base["packed"].data.shape[0], 96)]
    c = O.encoder_forward(base["P"], base["packed"].data, base["packed"].batch_sizes, base["ocfg"], hmask=ones)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert E.rel_err(a, base["r32"]["last_hidden"]) < 1e-5  # torch.nn.LSTM's own fp32 forward


def test_fast_cell_forms_move_layer1_gradients(monkeypatch):
    """What test_gpu_decoder_noise.R_ENC is attributed to, checked without a
    GPU (as test_ladder_cases_cpu.test_fast_cell_forms_move_encoder_tensors
    does for R_ENCODER).  The fp32 oracle's encoder with fsigmoid / ftanh's
    forms (abcd_common.h: 1 / (1 + e^-x), 1 - 2 / (1 + e^2x)) against the same
    fp32 oracle with torch's -- the forms alone -- moves layer 1's gradients at
    h256-LSTM-b97steep by 2e-6 .. 2.5e-6 per block, what the GPU shows against
    float64 there (2.4e-6 .. 3.1e-6): several times the fp32 reference's own
    error, far under the hard 1e-4, and under 1e-6 of the tensor's maximum."""
    ref = NC.enc_drop_reference(256, "LSTM", "b97steep")
    args = (ref["P"], ref["ocfg"], ref["packed"], ref["dout"], [ref["mask"]], torch.float32)
    base = NC._enc_run(*args)
    with monkeypatch.context() as m:
        m.setattr(torch, "tanh", lambda x: 1.0 - 2.0 / (1.0 + torch.exp(2.0 * x)))
        m.setattr(torch, "sigmoid", lambda x: 1.0 / (1.0 + torch.exp(-x)))
        fast = NC._enc_run(*args)
    assert E.rel_err(base["last_hidden"], ref["r32"]["last_hidden"]) < 1e-6  # the same fp32 run
    for k in ("g/weight_ih_l1", "g/weight_hh_l1", "g/bias_ih_l1_reverse", "g/bias_hh_l1_reverse"):
        shift, e32 = E.block_err(fast[k], base[k]), ref["e32"][k][1]
        print(k, "shift %.2e e32 %.2e" % (shift, e32))
        assert 5e-7 <= shift <= 5e-6 and shift >= 2 * e32, (k, shift, e32)
        assert E.rel_err(fast[k], base[k]) <= 1e-6
