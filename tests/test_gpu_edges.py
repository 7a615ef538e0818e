"""The H = Hm = 256 recurrent kernels at batch edges against a float64 oracle.

``enc_fwd_persist<*,16,8>``, ``enc_bwd_w8``, ``dec_fwd_x6`` and
``dec_bwd_w16`` dispatch at every batch size and length once H = Hm = 256.
They mask rows through buffer extents, skip row groups that have no work at a
step, and map groups to workgroups differently when the group count is a
multiple of 8.  ``edge_cases.CASES`` puts one small batch (T <= 12) on each of
those boundaries: B = 1, T = 1, B on and one past a 32-row group, length-1
segments, a group that empties while the others run on, no shrink at all, and
8 / 16 groups at three steps.

One ``FusedStep`` step (seed-1111 weights, replayed noise) is compared with
``oracle.train_step`` in float64.  The forward scalars keep the project's bar
(1e-4 relative); tensors are measured twice, over the whole tensor
(``rel_err``) and per 16 x 16 block (``block_err``), in units of the fp32
oracle's own error against float64:

    e_hip <= R * e32 + 1e-7        and, whatever R,       e_hip <= 1e-4

``R`` starts at 4 (what tests/test_gpu_x6.py grants one split-fp32 product
over torch's fp32 GEMM); ``R_TENSOR`` lists the tensors whose measured error
needed more, with the approximation it is attributed to (DESIGN.md s4,
profiles/parity_errors.json).  A post-SGD delta is coef(norm) x gradient read
back through an fp32 parameter: its e32 is the gradient's plus the norm's, and
the half-ulp of the stored parameter is taken off its measured error
(edge_cases.store_slack).

Observed on MI355X over the 24 steps and 3 frame cases (every figure is
printed, ``-rA``): worst e_hip 1.4e-6 (rel_err) and 5.4e-6 (block_err); the
only tensors past the R = 4 bound are those of ``R_TENSOR``.
"""
import math

import pytest
import torch

import edge_cases as E
from gpu_helpers import named_params

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
HARD = 1e-4  # no tensor may exceed this in either metric, whatever R
R_DEFAULT = 4.0
# tensor -> R, raised only where that tensor exceeded 4 x e32 + 1e-7 on the GPU,
# to at most 2 x its own worst observed e_hip / e32 (in brackets).  Every one
# reads the emission MLP's hidden activation.
R_NOTE = ("The emission heads' hidden activation is ftanh (abcd_common.h: 1 - 2 / (1 + e^2x), absolute error ~1e-7 "
          "where torch's tanh is relative).  The heads' second layer reads it: mu in the forward pass, the W2 / b2 "
          "gradients (dOut^T a) and their deltas in the backward pass.  The fp32 oracle run with that tanh form moves "
          "the same tensors by the same amounts (tests/test_edge_cases_cpu.py::test_fast_tanh_form_moves_emission_w2).")
_EM = "decoder/emission_sampler.to_parameters.mlps.%d.whole_network.2.%s"
R_TENSOR = {
    "mu": 9.0,                              # [4.9, b33 frames, block_err 2.7e-6 against 5.6e-7]
    "g/" + _EM % (0, "weight"): 10.0,       # [5.3, b1t1 c2]
    "g/" + _EM % (1, "weight"): 10.0,       # [5.3, b1t1 c2]
    "g/" + _EM % (1, "bias"): 48.0,         # [24.4, b65 c2, block_err 5.4e-6 against 2.2e-7]
    "d/" + _EM % (0, "weight"): 10.0,       # [5.2, b1t1 c2]
    "d/" + _EM % (1, "weight"): 10.0,       # [5.1, b1t1 c2]
    "d/" + _EM % (1, "bias"): 37.0,         # [18.7, b65 c2]
}

KERNELS = {
    "LSTM": ("enc_fwd_persist<4,16,8>", "enc_bwd_w8<4>", "dec_fwd_x6<13,8,8,LSTM>", "dec_bwd_w16<9,LSTM>"),
    "GRU": ("enc_fwd_persist<3,16,8>", "enc_bwd_w8<3>", "dec_fwd_x6<13,8,8,GRU>", "dec_bwd_w16<9,GRU>"),
}

# mildest first: every case at c2 widths (LSTM, GRU); the three with a second
# row group also at c5gru (K = 1024, speakers: DS = 512 in dec_init_f2h) and c4 (plain, D = 16)
STEP_CASES = [(c, w) for c in E.CASES for w in ("c2", "c2gru")] + \
    [(c, w) for c in ("b33", "b97steep", "b160") for w in ("c5gru", "c4")]


def ratio(key):
    return R_TENSOR.get(key, R_DEFAULT)


def bound(key, e32, R=None):
    return (ratio(key) if R is None else R) * e32 + 1e-7


def _check_table(tag, hip, ref64, e32, record_property, slack=None):
    """hip / ref64: {key: tensor}; e32: {key: (rel, blk)}; slack: {key: the
    elementwise allowance of edge_cases.store_slack}.  Prints and records every
    figure, then asserts the bound and the hard 1e-4 on all of them."""
    rows, bad = [], []
    for k, r in ref64.items():
        sl = (slack or {}).get(k)
        rel, blk = E.rel_err(hip[k], r, slack=sl), E.block_err(hip[k], r, slack=sl)
        b_rel, b_blk = bound(k, e32[k][0]), bound(k, e32[k][1])
        rows.append(dict(tensor=k, e32_rel=e32[k][0], e_hip_rel=rel, e32_blk=e32[k][1], e_hip_blk=blk,
                         R=ratio(k)))
        print(f"{tag} {k}: rel e32 {e32[k][0]:.2e} hip {rel:.2e} | blk e32 {e32[k][1]:.2e} hip {blk:.2e}")
        if not (rel <= b_rel and blk <= b_blk and rel <= HARD and blk <= HARD):
            bad.append((k, rel, b_rel, blk, b_blk))
    record_property("parity_errors", rows)
    E.dump_observed(tag, rows)
    assert not bad, bad


@pytest.mark.parametrize("case,widths", STEP_CASES)
def test_edge_step_vs_oracle64(case, widths, record_property):
    import bench
    from modules import engine, noise, _native as N
    ref = E.reference(case, widths)
    cfg, P, batch, r64 = ref["cfg"], ref["P"], ref["batch"], ref["r64"]
    out, grads = r64["out"], r64["grads"]
    bsz, B = batch["batch_sizes"], cfg["B"]
    assert int(bsz[0]) == B == len(E.CASES[case])

    step = bench.build(cfg, "cuda")
    named = named_params(step.encoder, step.sampler, step.decoder)
    for k, p in named.items():  # the same weights on both sides (init-order parity)
        assert torch.equal(p.detach().cpu(), P[k]), k
    assert set(named) == set(grads)
    init = {k: p.detach().clone() for k, p in named.items()}

    noise.replay(ref["noise"]["feat"], ref["noise"]["eps"])
    N.lib().abcd_dispatch_reset()
    sc, logits = step.forward_backward(batch["data"].cuda(), bsz, batch["is_offset"].cuda(),
                                       batch["speakers"].cuda(), E.N_DATA)
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    ran = N.dispatch()
    grids = {"enc_fwd": (B + 63) // 64 * 32, "enc_bwd": (B + 31) // 32 * 16, "dec_fwd": (B + 63) // 64 * 32,
             "dec_bwd": (B + 31) // 32 * 16}
    for role, kern in zip(("enc_fwd", "enc_bwd", "dec_fwd", "dec_bwd"), KERNELS[cfg["rnn"]]):
        assert ran[role] == (f"{kern} grid {grids[role]}", 1), (role, ran[role])  # no per-step fallback

    sc = sc.cpu()
    for i, k in ((engine.EM, "em"), (engine.OFF, "off"), (engine.KL, "kl"), (engine.LOSS, "loss")):
        r = float(out[k])
        print(f"{case}-{widths} {k}: hip {float(sc[i]):.9g} ref {r:.9g} rel {abs(float(sc[i]) - r) / abs(r):.2e}")
        assert abs(float(sc[i]) - r) <= LOSS_TOL * abs(r) + 1e-5, (k, float(sc[i]), r)
    fwd = {"last_hidden": step.last_hidden, "logits": logits, "feats": step.feats}
    for k, t in fwd.items():
        assert t.shape == out[k].shape, (k, t.shape, out[k].shape)
        assert E.rel_err(t, out[k]) < 1e-4, (k, E.rel_err(t, out[k]))
    if not cfg["plain"]:
        assert E.top2_gap(out["logits"]) >= E.ARGMAX_GAP
        assert torch.equal(logits.argmax(-1).cpu(), out["logits"].argmax(-1))

    hip = {k: t.detach().double().cpu() for k, t in fwd.items()}
    for k, p in named.items():
        g = step.flat.grad_of(p).detach().double().cpu()
        assert torch.isfinite(g).all(), k
        if not grads[k].any():  # a product with an all-zero operand: anything else was read from a stale row
            assert not g.any(), (k, float(g.abs().max()))
        hip["g/" + k] = g
    zero = {k for k in named if not grads[k].any()}
    assert zero == E.ZERO_GRADS.get(case, set()), zero

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
    _check_table(f"{case}-{widths}", hip, ref64, E.oracle_errors(ref), record_property, slack)


@pytest.mark.parametrize("case", ["b33", "b65", "b97steep"])
def test_edge_decoder_frames_vs_oracle64(case, record_property):
    """encoder(packed) -> sampler -> sample -> decoder on the nn.Module surface
    at c2 widths: every packed row of the decoder's per-frame mu, log-var,
    self-fed samples and offset logits, elementwise against the float64
    oracle (the fixtures' row sums cannot see one wrong frame)."""
    from modules import noise
    from modules import model as M
    ref = E.reference(case, "c2")
    cfg, P, batch, out = ref["cfg"], ref["P"], ref["batch"], ref["r64"]["out"]
    torch.manual_seed(1111)
    enc = M.RNN_Variational_Encoder(cfg["F"], cfg["H"], rnn_type=cfg["rnn"])
    samp = M.ABCDSampler(enc.hidden_size_total, cfg["Hm"], cfg["K"], cfg["D"])
    dec = M.RNN_Variational_Decoder(cfg["F"], cfg["H"], cfg["Hm"], cfg["D"], rnn_type=cfg["rnn"])
    for m in (enc, samp, dec):
        m.cuda().train()
    for k, p in named_params(enc, samp, dec).items():
        assert torch.equal(p.detach().cpu(), P[k]), k
    packed = torch.nn.utils.rnn.PackedSequence(batch["data"].cuda(), batch["batch_sizes"])
    noise.replay(ref["noise"]["feat"], ref["noise"]["eps"])
    logits = samp(enc(packed))
    feats = samp.sample(logits)
    em, off, flat, (mu, lv), offl = dec(feats, batch_sizes=batch["batch_sizes"], speaker=batch["speakers"].cuda(),
                                        ground_truth_out=packed.data, ground_truth_offset=batch["is_offset"].cuda())
    torch.cuda.synchronize()
    for k, v in (("em", em), ("off", off)):
        assert abs(float(v) - float(out[k])) <= LOSS_TOL * abs(float(out[k])) + 1e-5, (k, float(v), float(out[k]))
    hip = {"mu": mu, "lv": lv, "flatten_out": flat, "offset_logits": offl}
    r32 = ref["r32"]["out"]
    e32 = {k: (E.rel_err(r32[k], out[k]), E.block_err(r32[k], out[k])) for k in hip}
    for k, t in hip.items():
        assert t.shape == out[k].shape, (k, t.shape, out[k].shape)
        assert E.rel_err(t, out[k]) < 1e-4, (k, E.rel_err(t, out[k]))
    _check_table(f"{case}-frames", hip, {k: out[k] for k in hip}, e32, record_property)


def test_edge_workspace_reuse_is_clean():
    """One FusedStep runs b256t3, then b33, then b1t1: its workspaces are sized
    by the largest case and hold its leftovers when the smaller ones run.  A
    fresh FusedStep that runs b33 (or b1t1) alone must give the same bits
    (scalars, logits, the flat gradient): the kernels are deterministic, so any
    difference is a read of a row the smaller batch never wrote."""
    import bench
    from modules import engine, noise, _native as N

    def run(step, case):
        ref = E.reference(case, "c2")
        batch = ref["batch"]
        noise.replay(ref["noise"]["feat"], ref["noise"]["eps"])
        sc, logits = step.forward_backward(batch["data"].cuda(), batch["batch_sizes"], batch["is_offset"].cuda(),
                                           batch["speakers"].cuda(), E.N_DATA)
        torch.cuda.synchronize()
        assert N.lib().abcd_device_status() == 0
        return sc[:engine.NORM].clone(), logits.clone(), step.flat.grad.clone()

    cfg = E.reference("b256t3", "c2")["cfg"]
    used = bench.build(cfg, "cuda")
    run(used, "b256t3")
    reused = {c: run(used, c) for c in ("b33", "b1t1")}
    for c in ("b33", "b1t1"):
        fresh_step = bench.build(cfg, "cuda")
        assert torch.equal(fresh_step.flat.flat, used.flat.flat)
        fresh = run(fresh_step, c)
        for name, a, b in zip(("scalars", "logits", "grad"), reused[c], fresh):
            assert torch.equal(a, b), (c, name, float((a - b).abs().max()))
        assert math.isfinite(float(fresh[0][engine.LOSS]))
