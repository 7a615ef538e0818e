"""The recurrent dispatch ladder off H = Hm = 256, F = 129 against float64,
route by route.

tests/test_gpu_edges.py, test_gpu_fullshape.py and test_gpu_prod.py pin the
first rung (``enc_fwd_persist<*,16,8>``, ``enc_bwd_w8``, ``dec_fwd_x6<13,..>``,
``dec_bwd_w16<9,..>``).  Every other rung of ``persist_encoder_fwd / _bwd`` and
``persist_decoder_fwd / _bwd`` (csrc/abcd_persist.hip) and the four per-step
fallbacks (csrc/abcd_rnn.hip) are pinned here: ``ladder_cases`` names, for each
width, the kernel template and grid the ladder selects, and each case asserts
that exactly that kernel ran, once per layer, with no hand-off timeout
(``abcd_device_status() == 0``).  The batches put these forms' 64-row tile on
its boundaries (B = 65, a second tile that empties after one step, three tiles
with a ragged one, one frame).

* the encoder alone (forward, and backward from a fixed ``dout``) against
  ``torch.nn.LSTM / GRU`` in float64, at H = 16 .. 512, two layers and one
  direction included;
* one whole training step (seed-1111 weights, replayed noise) against
  ``oracle.train_step`` in float64, at the decoder rows of ``ladder_cases``;
* the decoder's per-frame outputs on the ``nn.Module`` surface.

Forward scalars keep the project's bar (1e-4 relative).  Tensors are measured
over the whole tensor (``rel_err``) and per 16 x 16 block (``block_err``) in
units of the same computation in fp32 against float64:

    e_hip <= R * e32 + 1e-7        and, whatever R,       e_hip <= 1e-4

``R`` is 4 (what tests/test_gpu_x6.py grants one split-fp32 product);
``R_TENSOR`` (steps, frames) and ``R_ENCODER`` (the encoder alone) list the
tensors whose measured error needed more, each with its worst observed ratio,
the case and the attributed cause (profiles/parity_errors.json, section
``ladder``).

Observed on MI355X over the 48 encoder cases, 44 steps and 3 frame cases (every
figure is printed, ``-rA``): every route as pinned; worst e_hip 1.1e-6
(rel_err) and 8.2e-6 (block_err, the log-var head's b2 gradient at
f65-GRU-b65); the only tensors past the R = 4 bound are those of the two tables.
The F = 257 row's BPTT is pinned per step: ``dec_bwd_persist`` needs 177 KiB of
LDS there and ``fits_resident`` declines it (ladder_cases.DEC_ROWS).
"""
import os

import pytest
import torch

import edge_cases as E
import ladder_cases as L
from gpu_helpers import build_from_meta, named_params

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
HARD = 1e-4  # no tensor may exceed this in either metric, whatever R
R_DEFAULT = 4.0
# tensor -> R, raised only where that tensor's e_hip / e32 went past 4 on the GPU, to at most 2 x its own worst
# observed ratio (in brackets, with the case and the figures).  Every one is a ~1e-6 error downstream of the
# kernels' short-latency activations.
R_NOTE = ("The recurrent kernels' sigmoid and tanh are fsigmoid / ftanh (abcd_common.h: v_exp + v_rcp, tanh as "
          "1 - 2 / (1 + e^2x)), whose error is absolute (~1e-7) where torch's is relative.  Decoder steps: the "
          "emission heads' second layer reads the ftanh hidden activation, so its weight / bias gradients and deltas "
          "carry it (the tensors of test_gpu_edges.R_TENSOR, same cause).  Encoder alone: at one frame, or where all "
          "rows but one end after a step, the final state and the gate gradients are a single cell's outputs, and the "
          "quietest 16-wide block of a bias gradient is ~1% of the tensor's max.  The fp32 oracle run with those "
          "forms moves the same tensors by the same amounts "
          "(tests/test_ladder_cases_cpu.py::test_fast_cell_forms_move_encoder_tensors, "
          "tests/test_edge_cases_cpu.py::test_fast_tanh_form_moves_emission_w2).")
_EM = "decoder/emission_sampler.to_parameters.mlps.%d.whole_network.2.%s"
R_TENSOR = {  # training steps and frames
    "g/" + _EM % (0, "weight"): 17.0,   # [8.57, hm128g-LSTM-b65, block_err 6.1e-6 against 7.2e-7]
    "g/" + _EM % (1, "weight"): 10.5,   # [5.32, h64-LSTM-b97steep, block_err 2.7e-6 against 5.0e-7]
    "g/" + _EM % (1, "bias"): 10.0,     # [5.08, f65-GRU-b65, block_err 8.2e-6 against 1.6e-6]
    "d/" + _EM % (0, "weight"): 11.5,   # [5.91, hm128g-LSTM-b65, block_err 4.5e-6 against 7.6e-7]
    "d/" + _EM % (1, "weight"): 9.5,    # [4.84, hm128-LSTM-b1t1, rel_err 6.1e-7 against 1.3e-7]
    "d/" + _EM % (1, "bias"): 8.0,      # [4.10, f65-GRU-b65, block_err 6.7e-6 against 1.6e-6]
}
R_ENCODER = {  # the encoder alone against torch.nn.LSTM / GRU
    "last_hidden": 11.0,                # [5.50, h512-LSTM-b1t1, block_err 1.6e-6 against 3.0e-7]
    "g/weight_ih_l0": 8.0,              # [4.24, h512-LSTM-b1t1, block_err 1.65e-6 against 3.9e-7]
    "g/bias_ih_l0": 8.5,                # [4.38, h512-LSTM-b1t1, block_err 1.65e-6 against 3.8e-7]
    "g/bias_hh_l0": 8.5,                # [4.38, h512-LSTM-b1t1: the same gradient]
    "g/bias_ih_l0_reverse": 9.5,        # [4.92, h512-LSTM-b97steep, block_err 1.7e-6 against 3.5e-7]
    "g/bias_hh_l0_reverse": 9.0,        # [4.65, h128-LSTM-b1t1, block_err 7.5e-7 against 1.6e-7]
    "g/bias_ih_l1": 9.0,                # [4.52, h128-LSTM-b65 two layers, block_err 1.4e-6 against 3.0e-7]
    "g/bias_hh_l1": 9.0,                # [4.52, the same gradient]
}


def bound(R, e32):
    return R * e32 + 1e-7


def _check_table(tag, hip, ref64, e32, record_property, slack=None, table=R_TENSOR):
    """hip / ref64: {key: tensor}; e32: {key: (rel, blk)}; slack: {key: the
    elementwise allowance of edge_cases.store_slack}; table: the raised R's.
    Prints and records every figure, then asserts the bound and the hard 1e-4
    on all of them."""
    rows, bad = [], []
    for k, r in ref64.items():
        sl = (slack or {}).get(k)
        R = table.get(k, R_DEFAULT)
        rel, blk = E.rel_err(hip[k], r, slack=sl), E.block_err(hip[k], r, slack=sl)
        b_rel, b_blk = bound(R, e32[k][0]), bound(R, e32[k][1])
        rows.append(dict(tensor=k, e32_rel=e32[k][0], e_hip_rel=rel, e32_blk=e32[k][1], e_hip_blk=blk, R=R))
        print(f"{tag} {k}: rel e32 {e32[k][0]:.2e} hip {rel:.2e} | blk e32 {e32[k][1]:.2e} hip {blk:.2e}")
        if not (rel <= b_rel and blk <= b_blk and rel <= HARD and blk <= HARD):
            bad.append((k, rel, b_rel, blk, b_blk))
    record_property("parity_errors", rows)
    E.dump_observed(tag, rows)
    assert not bad, bad


def _persist(on, fn):
    """Run fn with ABCD_PERSIST set (the library reads it per call) and restore it."""
    old = os.environ.get("ABCD_PERSIST")
    os.environ["ABCD_PERSIST"] = "1" if on else "0"
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("ABCD_PERSIST", None)
        else:
            os.environ["ABCD_PERSIST"] = old


def _assert_routes(ran, expected, count=1):
    for role, want in expected.items():
        assert ran[role] == (want, count), (role, ran[role], want)  # the pinned kernel, no fallback, once per layer


ENC_PARAMS = [pytest.param(H, rnn, case, 1, True, id=f"h{H}-{rnn}-{case}") for H, rnn, case in L.ENC_CASES] + \
    [pytest.param(H, "LSTM", "b65", layers, bidir, id=f"h{H}-LSTM-b65-{'l2' if layers == 2 else 'uni'}")
     for H, layers, bidir in L.ENC_VARIANTS]


@pytest.mark.parametrize("H,rnn,case,layers,bidir", ENC_PARAMS)
def test_encoder_route_vs_torch_f64(H, rnn, case, layers, bidir, record_property):
    from modules import _native as N
    ref = L.enc_reference(H, rnn, case, layers, bidir)
    P, packed, r64 = ref["P"], ref["packed"], ref["r64"]
    B = ref["cfg"]["B"]
    enc, samp, dec = build_from_meta(ref["meta"], L.arrays_of(P))
    for k, p in named_params(enc, samp, dec).items():  # the same weights on both sides
        assert torch.equal(p.detach().cpu(), P[k]), k

    N.lib().abcd_dispatch_reset()
    out = enc(torch.nn.utils.rnn.PackedSequence(packed.data.cuda(), packed.batch_sizes))
    (out * ref["dout"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    _assert_routes(N.dispatch(), L.enc_expected(H, rnn, B, nd=2 if bidir else 1), count=layers)

    hip = {"last_hidden": out.detach().double().cpu()}
    for n, p in enc.rnn.named_parameters():
        g = p.grad.detach().double().cpu()
        assert torch.isfinite(g).all(), n
        if not r64["g/" + n].any():  # h_0 = 0 at a single frame: anything else was read from a stale row
            assert not g.any(), (n, float(g.abs().max()))
        hip["g/" + n] = g
    assert set(hip) == set(r64)
    for k, t in hip.items():
        assert t.shape == r64[k].shape, (k, t.shape, r64[k].shape)
    tag = f"ladder-enc-h{H}-{rnn}-{case}" + ("" if (layers, bidir) == (1, True) else f"-l{layers}d{2 if bidir else 1}")
    _check_table(tag, hip, r64, ref["e32"], record_property, table=R_ENCODER)


@pytest.mark.parametrize("row,rnn,case", L.DEC_CASES)
def test_decoder_route_step_vs_oracle64(row, rnn, case, record_property):
    from modules import engine, noise, _native as N
    ref = L.dec_reference(row, rnn, case)
    cfg, P, batch, r64 = ref["cfg"], ref["P"], ref["batch"], ref["r64"]
    out, grads = r64["out"], r64["grads"]
    bsz, B = batch["batch_sizes"], cfg["B"]
    assert int(bsz[0]) == B == len(E.CASES[case])

    enc, samp, dec = build_from_meta(L.meta_of(cfg), L.arrays_of(P))
    step = engine.FusedStep(enc, samp, dec)
    named = named_params(step.encoder, step.sampler, step.decoder)
    for k, p in named.items():  # the same weights on both sides
        assert torch.equal(p.detach().cpu(), P[k]), k
    assert set(named) == set(grads)
    init = {k: p.detach().clone() for k, p in named.items()}

    noise.replay(ref["noise"]["feat"], ref["noise"]["eps"])
    N.lib().abcd_dispatch_reset()
    sc, logits = _persist(cfg["persist"], lambda: step.forward_backward(
        batch["data"].cuda(), bsz, batch["is_offset"].cuda(), batch["speakers"].cuda(), E.N_DATA))
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    _assert_routes(N.dispatch(), L.dec_expected(row, rnn, B))

    sc = sc.cpu()
    for i, k in ((engine.EM, "em"), (engine.OFF, "off"), (engine.KL, "kl"), (engine.LOSS, "loss")):
        r = float(out[k])
        print(f"{row}-{rnn}-{case} {k}: hip {float(sc[i]):.9g} ref {r:.9g} rel {abs(float(sc[i]) - r) / abs(r):.2e}")
        assert abs(float(sc[i]) - r) <= LOSS_TOL * abs(r) + 1e-5, (k, float(sc[i]), r)
    fwd = {"last_hidden": step.last_hidden, "logits": logits, "feats": step.feats}
    for k, t in fwd.items():
        assert t.shape == out[k].shape, (k, t.shape, out[k].shape)
        assert E.rel_err(t, out[k]) < 1e-4, (k, E.rel_err(t, out[k]))
    # (no argmax assertion: the logits are bounded elementwise below, and these batches' rows were not
    # redrawn for a top-2 gap)

    hip = {k: t.detach().double().cpu() for k, t in fwd.items()}
    for k, p in named.items():
        g = step.flat.grad_of(p).detach().double().cpu()
        assert torch.isfinite(g).all(), k
        if not grads[k].any():  # a product with an all-zero operand: anything else was read from a stale row
            assert not g.any(), (k, float(g.abs().max()))
        hip["g/" + k] = g
    zero = {k for k in named if not grads[k].any()}
    assert zero == L.zero_grads(row, case), zero

    step.optimizer_step(lr=1.0, momentum=0.0, clip=1.0)
    torch.cuda.synchronize()
    hip["norm"] = step.scalars[engine.NORM].detach().double().cpu().reshape(1)
    for k, p in named.items():
        hip["d/" + k] = p.detach().double().cpu() - init[k].double().cpu()

    ref64 = {k: out[k] for k in fwd}
    ref64.update(("g/" + k, g) for k, g in grads.items())
    ref64["norm"] = torch.tensor([r64["total"]], dtype=torch.float64)
    ref64.update(("d/" + k, d) for k, d in r64["delta"].items())
    slack = {"d/" + k: E.store_slack(r64["new"][k]) for k in grads}
    _check_table(f"ladder-dec-{row}-{rnn}-{case}", hip, ref64, E.oracle_errors(ref), record_property, slack)


@pytest.mark.parametrize("row,rnn,case", L.FRAME_CASES)
def test_decoder_route_frames_vs_oracle64(row, rnn, case, record_property):
    """encoder(packed) -> sampler -> sample -> decoder on the nn.Module surface:
    every packed row of the decoder's per-frame mu, log-var, self-fed samples
    and offset logits, elementwise against the float64 oracle."""
    from modules import noise, _native as N
    ref = L.dec_reference(row, rnn, case)
    cfg, P, batch, out = ref["cfg"], ref["P"], ref["batch"], ref["r64"]["out"]
    enc, samp, dec = build_from_meta(L.meta_of(cfg), L.arrays_of(P))
    for k, p in named_params(enc, samp, dec).items():
        assert torch.equal(p.detach().cpu(), P[k]), k
    packed = torch.nn.utils.rnn.PackedSequence(batch["data"].cuda(), batch["batch_sizes"])
    noise.replay(ref["noise"]["feat"], ref["noise"]["eps"])
    N.lib().abcd_dispatch_reset()
    logits = samp(enc(packed))
    feats = samp.sample(logits)
    em, off, flat, (mu, lv), offl = dec(feats, batch_sizes=batch["batch_sizes"], speaker=batch["speakers"].cuda(),
                                        ground_truth_out=packed.data, ground_truth_offset=batch["is_offset"].cuda())
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    exp = L.dec_expected(row, rnn, cfg["B"])
    _assert_routes(N.dispatch(), {r: exp[r] for r in ("enc_fwd", "dec_fwd")})
    for k, v in (("em", em), ("off", off)):
        assert abs(float(v) - float(out[k])) <= LOSS_TOL * abs(float(out[k])) + 1e-5, (k, float(v), float(out[k]))
    hip = {"mu": mu, "lv": lv, "flatten_out": flat, "offset_logits": offl}
    r32 = ref["r32"]["out"]
    e32 = {k: (E.rel_err(r32[k], out[k]), E.block_err(r32[k], out[k])) for k in hip}
    for k, t in hip.items():
        assert t.shape == out[k].shape, (k, t.shape, out[k].shape)
        assert E.rel_err(t, out[k]) < 1e-4, (k, E.rel_err(t, out[k]))
    _check_table(f"ladder-frames-{row}-{rnn}-{case}", hip, {k: out[k] for k in hip}, e32, record_property)
