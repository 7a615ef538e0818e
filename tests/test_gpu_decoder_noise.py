"""Decoder input dropout, the decoder's in-kernel Philox draw and the encoder's
inter-layer dropout against float64, route by route.

tests/test_gpu_edges.py and tests/test_gpu_ladder.py hold every recurrent
route to the float64 oracle with the decoder's noise replayed as ``eps``, no
``xmask`` and ``hidden_dropout = 0``.  The cases of tests/noise_cases.py cover
what a real training step adds (tests/test_noise_cases_cpu.py pins that a
mistaken mask or stream is far outside every bar used here):

* Part A -- p = 0.3 input dropout on every decoder route at batch edges: one
  ``FusedStep`` step and the ``nn.Module`` frames against ``oracle.train_step``
  fed the same mask.  ``eps`` and ``xmask`` are views of buffers whose 64 rows
  past L are NaN: a read past the block shows in an output.
* Part B -- ``noise.mode == "philox"`` with only the Gumbel noise replayed: the
  noise each form drew, recovered from the step's own ``flatten_out``, ``mu``
  and ``lv`` (FusedStep's decoder call is given output buffers; nothing else
  changes), is element ``O + row * F + col`` of stream S, also on a workspace
  that holds another draw and across the counter's carry; the step then agrees
  with the oracle fed ``abcd_fill_normal`` / ``abcd_fill_dropout``'s values.
* Part C -- the two-layer bidirectional encoder alone with
  ``hidden_dropout = 0.25`` against ``oracle.encoder_forward(hmask=...)``.

Every case asserts the kernel ladder_cases / test_gpu_edges.KERNELS pins for it
and ``abcd_device_status() == 0``.  Tensors are judged as in those two files,

    e_hip <= R * e32 + 1e-7        and, whatever R,       e_hip <= 1e-4

in ``rel_err`` and ``block_err``, R = 4 but for the tensors of
``test_gpu_edges.R_TENSOR`` (first rung) / ``test_gpu_ladder.R_TENSOR`` and
``R_ENCODER`` (the other rows, the encoder), whose values are used unchanged,
and those of ``R_STEP`` / ``R_ENC`` below (profiles/parity_errors.json, section
``decoder_noise``).

Observed on MI355X over the 22 masked steps, 3 frame cases, 10 Philox steps and
8 encoder cases (every figure is printed, ``-rA``): every route as pinned;
worst e_hip 9.5e-7 (rel_err) and 3.8e-6 (block_err).  No step or frame tensor
went past the bounds of the two imported tables (worst ratio 4.63 under R = 10:
the mu head's W2 gradient at rung1-LSTM-b1t1).  The recovered noise is within
1.7e-6 of the numpy stream where 1e-4 and the operands' rounding are allowed.
Raised here, encoder alone (``R_ENC``): layer 1's ``weight_ih`` / ``weight_hh``
gradients (4.44 x e32 at h256-LSTM-b97steep, block_err 3.1e-6 against 6.9e-7)
and its reverse direction's bias gradients (6.50 x e32 at the same case, 2.4e-6
against 3.8e-7), attributed to the absolute error of fsigmoid / ftanh where all
rows but one end after the first step.

With the library broken on purpose (local builds, not kept): without the
``b < next_bs`` guard of ``dec_fwd_persist``'s hand-off store, the masked steps
hm128-LSTM-b65 and h64-LSTM-b65 fail their tensor bars (the cell's ``weight_hh``
gradient 0.5 of its maximum off); with pitch Fp in ``dec_fwd_x6``'s mask read,
the first rung's masked steps and frames fail on NaN losses; without
``fill_eps(t + 1)``, the first rung's Philox cases find 0 where the stream has
|eps| ~ 4, and the used-workspace case does not find the second stream.
"""
import os

import numpy as np
import pytest
import torch

import edge_cases as E
import ladder_cases as L
import noise_cases as NC
import test_gpu_edges as TE
import test_gpu_ladder as TL
from gpu_helpers import build_from_meta, named_params

pytestmark = pytest.mark.gpu

LOSS_TOL = TL.LOSS_TOL
NAN_ROWS = 64
# tensor -> R, raised only where that tensor's e_hip / e32 went past its bound in this file, to at most 2 x its
# own worst observed ratio (in brackets, with the case and the figures).  No step or frame tensor needed it.
R_STEP = {
}
# The encoder alone: layer 1's gradients where all rows but one end after a step (b97steep), or in the
# quietest block of a bias gradient.  Same cause as test_gpu_ladder.R_ENCODER (its R_NOTE): fsigmoid / ftanh
# carry an absolute error of ~1e-7.  The fp32 oracle run with those forms moves these tensors by the same
# amounts (tests/test_noise_cases_cpu.py::test_fast_cell_forms_move_layer1_gradients).
R_ENC = {
    "g/weight_ih_l1": 8.5,              # [4.44, h256-LSTM-b97steep, block_err 3.08e-6 against 6.93e-7]
    "g/weight_hh_l1": 8.5,              # [4.44, h256-LSTM-b97steep, block_err 2.95e-6 against 6.64e-7]
    "g/bias_ih_l1_reverse": 13.0,       # [6.50, h256-LSTM-b97steep, block_err 2.44e-6 against 3.76e-7]
    "g/bias_hh_l1_reverse": 13.0,       # [6.50, the same gradient]
}
R_NOTE = ("No training-step or frame tensor went past the bounds of test_gpu_edges.R_TENSOR / "
          "test_gpu_ladder.R_TENSOR.  The encoder alone with inter-layer dropout: layer 1's weight_ih / weight_hh "
          "gradients and its reverse direction's bias gradients, where all rows but one end after the first step "
          "(b97steep) or in the quietest 16-wide block of a bias gradient -- the absolute ~1e-7 error of fsigmoid / "
          "ftanh (test_gpu_ladder.R_NOTE); the fp32 oracle run with those forms moves them by the same amounts "
          "(tests/test_noise_cases_cpu.py::test_fast_cell_forms_move_layer1_gradients).")


def _table(row):
    return dict(TE.R_TENSOR if row == NC.RUNG1 else TL.R_TENSOR, **R_STEP)


def _guarded(t):
    """A CUDA view buf[:L] of an (L + 64) x F buffer whose tail is NaN; noise._pop hands it on as it is."""
    n, F = t.shape
    buf = torch.full((n + NAN_ROWS, F), float("nan"), device="cuda")
    buf[:n] = t.to("cuda", torch.float32)
    view = buf[:n]
    assert view.to(device="cuda", dtype=torch.float32).contiguous().data_ptr() == buf.data_ptr()
    return view


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _build_step(cfg, P, p):
    from modules import engine
    enc, samp, dec = build_from_meta(NC.meta(cfg, p), L.arrays_of(P))
    step = engine.FusedStep(enc, samp, dec)
    named = named_params(step.encoder, step.sampler, step.decoder)
    for k, v in named.items():  # the same weights on both sides
        assert torch.equal(v.detach().cpu(), P[k]), k
    return step, named, {k: v.detach().clone() for k, v in named.items()}


def _forward_backward(step, cfg, batch, env=None):
    """One forward_backward under the row's ABCD_PERSIST; returns (scalars, logits, what ran)."""
    from modules import _native as N
    N.lib().abcd_dispatch_reset()
    sc, logits = _with_env(env or {}, lambda: TL._persist(cfg["persist"], lambda: step.forward_backward(
        batch["data"].cuda(), batch["batch_sizes"], batch["is_offset"].cuda(), batch["speakers"].cuda(), E.N_DATA)))
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    return sc, logits, N.dispatch()


def _judge_step(tag, row, step, named, init, sc, logits, ref, zero_expected, record_property):
    """The bars of test_gpu_ladder.test_decoder_route_step_vs_oracle64 on one finished forward_backward."""
    from modules import engine
    r64 = ref["r64"]
    out, grads = r64["out"], r64["grads"]
    assert set(named) == set(grads)
    sc = sc.cpu()
    for i, k in ((engine.EM, "em"), (engine.OFF, "off"), (engine.KL, "kl"), (engine.LOSS, "loss")):
        r = float(out[k])
        print(f"{tag} {k}: hip {float(sc[i]):.9g} ref {r:.9g} rel {abs(float(sc[i]) - r) / abs(r):.2e}")
        assert abs(float(sc[i]) - r) <= LOSS_TOL * abs(r) + 1e-5, (k, float(sc[i]), r)
    fwd = {"last_hidden": step.last_hidden, "logits": logits, "feats": step.feats}
    for k, t in fwd.items():
        assert t.shape == out[k].shape, (k, t.shape, out[k].shape)
        assert torch.isfinite(t).all(), k
        assert E.rel_err(t, out[k]) < 1e-4, (k, E.rel_err(t, out[k]))
    hip = {k: t.detach().double().cpu() for k, t in fwd.items()}
    for k, p in named.items():
        g = step.flat.grad_of(p).detach().double().cpu()
        assert torch.isfinite(g).all(), k  # a mask or eps row past L is NaN
        if not grads[k].any():  # a product with an all-zero operand: anything else was read from a stale row
            assert not g.any(), (k, float(g.abs().max()))
        hip["g/" + k] = g
    assert {k for k in named if not grads[k].any()} == zero_expected
    step.optimizer_step(lr=1.0, momentum=0.0, clip=1.0)
    torch.cuda.synchronize()
    hip["norm"] = step.scalars[engine.NORM].detach().double().cpu().reshape(1)
    for k, p in named.items():
        hip["d/" + k] = p.detach().double().cpu() - init[k].double().cpu()
        assert torch.isfinite(hip["d/" + k]).all(), k
    ref64 = {k: out[k] for k in fwd}
    ref64.update(("g/" + k, g) for k, g in grads.items())
    ref64["norm"] = torch.tensor([r64["total"]], dtype=torch.float64)
    ref64.update(("d/" + k, d) for k, d in r64["delta"].items())
    slack = {"d/" + k: E.store_slack(r64["new"][k]) for k in grads}
    TL._check_table(tag, hip, ref64, E.oracle_errors(ref), record_property, slack, table=_table(row))


def _zero_grads(row, case):
    return set(E.ZERO_GRADS.get(case, set())) if row == NC.RUNG1 else L.zero_grads(row, case)


def _assert_routes(tag, ran, expected):
    TL._assert_routes(ran, expected)
    print(f"{tag} routes: " + "; ".join(f"{r} = {ran[r][0]}" for r in expected))


# ---------------------------------------------------------------------------- Part A
@pytest.mark.parametrize("row,rnn,case", NC.MASK_CASES)
def test_input_dropout_step_vs_oracle64(row, rnn, case, record_property):
    """One training step with p = 0.3 and a replayed mask.  At b1t1 the
    reference is the oracle's no-mask step (x_0 = 0, no next step), and the
    cell's input-weight gradient must be exactly zero."""
    from modules import noise
    ref = NC.mask_reference(row, rnn, case)
    cfg, batch = ref["cfg"], ref["batch"]
    assert int(batch["batch_sizes"][0]) == cfg["B"] == len(E.CASES[case])
    step, named, init = _build_step(cfg, ref["P"], NC.P_DROP)
    assert step.decoder._input_dropout_p() == NC.P_DROP
    noise.replay(ref["noise"]["feat"], _guarded(ref["noise"]["eps"]), _guarded(ref["noise"]["xmask"]))
    sc, logits, ran = _forward_backward(step, cfg, batch)
    assert not noise._replay  # Gumbel, eps and the mask were all taken
    tag = f"noise-mask-{row}-{rnn}-{case}"
    _assert_routes(tag, ran, NC.expected(row, rnn, cfg["B"]))
    _judge_step(tag, row, step, named, init, sc, logits, ref, _zero_grads(row, case), record_property)


@pytest.mark.parametrize("row,rnn,case", NC.MASK_FRAME_CASES)
def test_input_dropout_frames_vs_oracle64(row, rnn, case, record_property):
    """encoder -> sampler -> sample -> decoder on the nn.Module surface with
    p = 0.3: every packed row of mu, log-var, the self-fed samples and the
    offset logits, elementwise."""
    from modules import noise, _native as N
    ref = NC.mask_reference(row, rnn, case)
    cfg, P, batch, out = ref["cfg"], ref["P"], ref["batch"], ref["r64"]["out"]
    enc, samp, dec = build_from_meta(NC.meta(cfg, NC.P_DROP), L.arrays_of(P))
    for k, p in named_params(enc, samp, dec).items():
        assert torch.equal(p.detach().cpu(), P[k]), k
    packed = torch.nn.utils.rnn.PackedSequence(batch["data"].cuda(), batch["batch_sizes"])
    noise.replay(ref["noise"]["feat"], _guarded(ref["noise"]["eps"]), _guarded(ref["noise"]["xmask"]))
    N.lib().abcd_dispatch_reset()
    logits = samp(enc(packed))
    feats = samp.sample(logits)
    em, off, flat, (mu, lv), offl = dec(feats, batch_sizes=batch["batch_sizes"], speaker=batch["speakers"].cuda(),
                                        ground_truth_out=packed.data, ground_truth_offset=batch["is_offset"].cuda())
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0 and not noise._replay
    tag = f"noise-maskframes-{row}-{rnn}-{case}"
    exp = NC.expected(row, rnn, cfg["B"])
    _assert_routes(tag, N.dispatch(), {r: exp[r] for r in ("enc_fwd", "dec_fwd")})
    for k, v in (("em", em), ("off", off)):
        assert abs(float(v) - float(out[k])) <= LOSS_TOL * abs(float(out[k])) + 1e-5, (k, float(v), float(out[k]))
    hip = {"mu": mu, "lv": lv, "flatten_out": flat, "offset_logits": offl}
    for k, t in hip.items():
        assert t.shape == out[k].shape, (k, t.shape, out[k].shape)
        assert torch.isfinite(t).all(), k
        assert E.rel_err(t, out[k]) < 1e-4, (k, E.rel_err(t, out[k]))
    TL._check_table(tag, hip, {k: out[k] for k in hip}, NC.frame_e32(ref), record_property, table=_table(row))


# ---------------------------------------------------------------------------- Part B
class _Frames:
    """Gives FusedStep's decoder-forward call buffers for flatten_out, mu and
    lv (it passes none): the launch copies its own stashes of that run into
    them.  ``out`` holds those of the last call."""

    def __init__(self, monkeypatch):
        from modules import _native as N
        lib = N.lib()
        orig = lib.abcd_decoder_forward_split
        self.out = None

        def call(*a):
            a = list(a)
            assert a[10] is None and a[11] is None and a[12] is None
            self.out = [torch.full((a[2].L, a[0].output_size), float("nan"), device="cuda") for _ in range(3)]
            a[10:13] = [N.ptr(t) for t in self.out]
            return orig(*a)

        monkeypatch.setattr(lib, "abcd_decoder_forward_split", call)


def _philox_run(step, cfg, batch, feat, seed, offset, c, frames):
    """One forward_backward in Philox mode with only the Gumbel noise replayed;
    returns (scalars, logits, what ran, eps_hat, its tolerance)."""
    from modules import noise
    saved = noise.get_state()
    try:
        noise.set_state({"mode": "philox", "seed": seed, "offset": offset})
        noise.replay(feat)
        sc, logits, ran = _forward_backward(step, cfg, batch, c["env"])
        assert not noise._replay
        n4 = 4 * L.cdiv(c["L"] * c["F"], 4)
        assert noise.get_state()["offset"] == offset + (2 * n4 if c["p"] else n4)  # the decoder's block, then the mask's
    finally:
        noise.set_state(saved)
    flat, mu, lv = frames.out
    for t in (flat, mu, lv):
        assert torch.isfinite(t).all()
    return (sc, logits, ran) + NC.eps_hat(flat, mu, lv)


def _fill(kind, n, seed, offset, p=None):
    from modules import _native as N
    buf = torch.full((n + 4,), float("nan"), device="cuda")
    if kind == "normal":
        rc = N.lib().abcd_fill_normal(N.ptr(buf), n, seed, offset, N.stream())
    else:
        rc = N.lib().abcd_fill_dropout(N.ptr(buf), n, p, seed, offset, N.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(buf[n:]).all())
    return buf[:n].cpu()


def _stream_batch(c):
    cfg = NC.config(c["row"], c["rnn"], len(E.CASES[c["case"]]))
    batch, drawn = E.make_batch(E.CASES[c["case"]], cfg, NC.SEED)
    return cfg, batch, drawn["feat"]


@pytest.mark.parametrize("name", list(NC.STREAM_CASES))
def test_philox_draw_is_the_stream_and_step_vs_oracle64(name, monkeypatch, record_property):
    """1. the noise the form drew is element O + row * F + col of stream S
    (tolerance: noise_cases.eps_hat), also across the counter's carry
    (noise_cases.CARRY_AT); 4. the step against the oracle fed the fill
    kernels' values of the same (S, O)."""
    from oracle import abcd_oracle as O
    c = NC.stream_spec(name)
    cfg, batch, feat = _stream_batch(c)
    ocfg = dict(E.oracle_cfg(cfg), greedy=cfg["greedy"])
    P = O.init_params(ocfg, 1111)
    step, named, init = _build_step(cfg, P, c["p"])
    frames = _Frames(monkeypatch)
    sc, logits, ran, got, tol = _philox_run(step, cfg, batch, feat, c["seed"], c["offset"], c, frames)
    tag = f"noise-philox-{name}"
    _assert_routes(tag, ran, NC.expected(c["row"], c["rnn"], cfg["B"]))

    want = NC.stream(c["seed"], c["offset"], c["L"], c["F"])
    err = np.abs(got - want)
    i = np.unravel_index(np.argmax(err - tol), err.shape)
    print(f"{tag} eps_hat: max |err| {err.max():.3e}, worst err - tol {float((err - tol).max()):.3e} at {i}")
    assert (err <= tol).all(), (i, got[i], want[i], tol[i])

    # the fill kernels of the same (S, O) against the numpy stream, then the step against the oracle fed them
    n = c["L"] * c["F"]
    eps = _fill("normal", n, c["seed"], c["offset"]).reshape(c["L"], c["F"])
    assert np.abs(eps.double().numpy() - want).max() <= 1e-4
    xmask = None
    if c["p"]:
        xmask = _fill("dropout", n, c["seed"], NC.mask_offset(c["offset"], c["L"], c["F"]), c["p"])
        xmask = xmask.reshape(c["L"], c["F"])
        m = NC.stream_mask(c["seed"], c["offset"], c["L"], c["F"], c["p"])
        assert np.array_equal(xmask.numpy() != 0, m != 0)  # the keep pattern, exactly
        assert np.all(np.abs(xmask.double().numpy() - m) <= np.spacing(np.float32(1.0 / (1.0 - c["p"]))))
        assert NC.last_column_mixed(xmask, NC.batch_sizes(c["case"]))
    ref = NC.stream_reference(name, eps, xmask)
    assert torch.equal(ref["P"]["decoder/rnn_cell.cell.weight_ih"], P["decoder/rnn_cell.cell.weight_ih"])
    _judge_step(tag, c["row"], step, named, init, sc, logits, ref, _zero_grads(c["row"], c["case"]), record_property)


@pytest.mark.parametrize("name", list(NC.STALE_CASES))
def test_philox_draw_on_a_used_workspace(name, monkeypatch):
    """2. the same FusedStep, two draws: the second run's noise is the second
    stream, and it differs from the first run's by more than 1 in every 64-row
    tile of every step -- a lost or late fill_eps store, or a skipped pre-fill,
    would leave the first run's values there."""
    from oracle import abcd_oracle as O
    c = NC.stream_spec(name)
    cfg, batch, feat = _stream_batch(c)
    P = O.init_params(dict(E.oracle_cfg(cfg), greedy=cfg["greedy"]), 1111)
    step, _, _ = _build_step(cfg, P, c["p"])
    frames = _Frames(monkeypatch)
    exp = NC.expected(c["row"], c["rnn"], cfg["B"])
    _, _, ran, first, _ = _philox_run(step, cfg, batch, feat, c["seed"], c["offset"], c, frames)
    _assert_routes(f"noise-stale-{name} run 1", ran, exp)
    ws = {k: v.data_ptr() for k, v in step._ws.items()}
    s2, o2 = NC.STALE_CASES[name]
    _, _, ran, second, tol = _philox_run(step, cfg, batch, feat, s2, o2, c, frames)
    _assert_routes(f"noise-stale-{name} run 2", ran, exp)
    assert {k: v.data_ptr() for k, v in step._ws.items()} == ws  # the second run reused the first one's workspaces
    want = NC.stream(s2, o2, c["L"], c["F"])
    err = np.abs(second - want)
    assert (err <= tol).all(), float((err - tol).max())
    for lo, hi in NC.tiles_with_rows(c["case"]):
        assert np.abs(second[lo:hi] - first[lo:hi]).max() > 1.0, (lo, hi)


# ---------------------------------------------------------------------------- Part C
@pytest.mark.parametrize("H,rnn,case", NC.ENC_DROP_CASES)
def test_encoder_inter_layer_dropout_vs_oracle64(H, rnn, case, record_property):
    """enc(packed) with hidden_dropout = 0.25 under noise.mode("reference"):
    the mask is torch's CPU draw after manual_seed, rebuilt for the oracle by
    noise_cases.draw_hidden_mask."""
    from modules import noise, _native as N
    ref = NC.enc_drop_reference(H, rnn, case)
    P, packed, r64 = ref["P"], ref["packed"], ref["r64"]
    enc, samp, dec = build_from_meta(ref["meta"], L.arrays_of(P))
    for k, p in named_params(enc, samp, dec).items():
        assert torch.equal(p.detach().cpu(), P[k]), k
    enc.rnn.dropout = NC.P_HIDDEN
    N.lib().abcd_dispatch_reset()
    with noise.mode("reference"):
        torch.manual_seed(ref["seed"])
        out = enc(torch.nn.utils.rnn.PackedSequence(packed.data.cuda(), packed.batch_sizes))
    (out * ref["dout"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    tag = f"noise-encdrop-h{H}-{rnn}-{case}"
    ran, exp = N.dispatch(), L.enc_expected(H, rnn, ref["cfg"]["B"])
    TL._assert_routes(ran, exp, count=2)
    print(f"{tag} routes: " + "; ".join(f"{r} = {ran[r][0]} x {ran[r][1]}" for r in exp))

    hip = {"last_hidden": out.detach().double().cpu()}
    for n, p in enc.rnn.named_parameters():
        g = p.grad.detach().double().cpu()
        assert torch.isfinite(g).all(), n
        hip["g/" + n] = g
    assert set(hip) == set(r64)
    for k, t in hip.items():
        assert t.shape == r64[k].shape, (k, t.shape, r64[k].shape)
    TL._check_table(tag, hip, r64, ref["e32"], record_property, table=dict(TL.R_ENCODER, **R_ENC))
