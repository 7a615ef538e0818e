"""The timed configuration against the oracle at its FULL shape (VERDICT r2
"next" item 1).

bench.py times one training step at b = 512 / GPU, T_max = 200 (c2, c4) and
T_max = 512 (c5, c5gru).  The other parity tests anchor the persistent kernels
at B = 72 / T = 20 (reference fixtures, two row groups) and at the b = 64
sub-batch (one row group); bugs that need more than two row groups, the
XCD-aware group order, the 16 encoder groups or the full time loop were only
visible HIP-vs-HIP.  Here one ``FusedStep`` step runs at the bench's own batch
(``bench.make_batch``: lengths U{tmin..tmax}, the longest forced to T_max),
seed-1111 weights (the reference's init order, ``learning.py:84-92``) and
replayed Gumbel / N(0, 1) noise, against ``oracle.train_step`` on the same
inputs (the torch-CPU restatement of ``learning.py:147-163`` pinned to the
reference's fixtures in ``tests/golden``):

* dispatch: the kernels and grids bench.py times (c2: ``dec_bwd_w16<9,LSTM>
  grid 256``, 16 encoder groups = ``grid 256``);
* em / off / kl / loss within 1e-4 relative (north star);
* logits within 1e-4 of their max, argmax categories identical;
* every parameter gradient within 3e-5 of its own max (norms 3e-5 relative)
  and within 4e-5 in its worst 16 x 16 block (``edge_cases.block_err``): 3 x
  the worst observed, every tensor's figures reported (``-rA``);
* the global gradient norm (clip) within 1e-4, post-SGD parameters within
  3e-5 of each tensor's update.

Reference: ``ABCD-VAE/modules/model.py:53,60-66,165-196,581-639``,
``ABCD-VAE/learning.py:155-163``.
"""
import os
import sys

import pytest
import torch

from edge_cases import block_err, dump_observed
from gpu_helpers import named_params, rel_err

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOSS_TOL = 1e-4
# 3 x the worst figure observed in this file on MI355X (profiles/parity_errors.json), rounded up to one digit:
# gradients 9.5e-6 of a tensor's max (c5 B = 512), norms 7.9e-7, post-SGD deltas 9.2e-6 -> 3e-5 (was 1e-3);
# the worst 16 x 16 block (edge_cases.block_err) 1.29e-5 -> 4e-5
GRAD_TOL = 3e-5
BLOCK_TOL = 4e-5


KERNELS = {
    "LSTM": ("enc_fwd_persist<4,16,8>", "enc_bwd_w8<4>", "dec_fwd_x6<13,8,8,LSTM>", "dec_bwd_w16<9,LSTM>"),
    "GRU": ("enc_fwd_persist<3,16,8>", "enc_bwd_w8<3>", "dec_fwd_x6<13,8,8,GRU>", "dec_bwd_w16<9,GRU>"),
}
# the encoder weight-gradient form (ABCD_WG3=0: gemm_wg2; default gemm_wg3b)
WG_FORM = "gemm_wg2" if os.environ.get("ABCD_WG3", "") == "0" else "gemm_wg3b"


# (bench config, batch, seed of the synthetic batch)
CASES = [("c2", 512, 2024), ("c4", 512, 2025), ("c5", 128, 2026), ("c5gru", 128, 2027),
         # the batch bench.py times at c5 / c5gru: 8 row groups, T_max = 512
         ("c5", 512, 2028), ("c5gru", 512, 2029)]


def _oracle_cfg(O, cfg):
    return O.default_cfg(F=cfg["F"], H=cfg["H"], Hdec=cfg["H"], Hm=cfg["Hm"], D=cfg["D"], K=cfg["K"] or 16,
                         rnn=cfg["rnn"], plain=cfg["plain"], fplain=cfg["D"],
                         num_speakers=cfg["spk"] or None, speaker_dim=cfg["sdim"])


@pytest.mark.parametrize("name,B,seed", CASES)
def test_full_shape_step_vs_oracle(name, B, seed, record_property):
    sys.path.insert(0, REPO)
    import bench
    from oracle import abcd_oracle as O
    from modules import engine, noise, _native as N
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    cfg = dict(bench.CONFIGS[name], B=B)
    batch = bench.make_batch(cfg, seed, "cpu")
    bsz, L = batch["batch_sizes"], batch["L"]
    assert int(bsz[0]) == B and len(bsz) == cfg["tmax"]
    g = torch.Generator().manual_seed(seed + 1)
    feat = torch.randn(B, cfg["D"], generator=g) if cfg["plain"] else \
        -torch.empty(B, cfg["K"]).exponential_(generator=g).log()
    eps = torch.randn(L, cfg["F"], generator=g)

    ocfg = _oracle_cfg(O, cfg)
    P = O.init_params(ocfg, 1111)
    step = bench.build(cfg, "cuda")
    named = named_params(step.encoder, step.sampler, step.decoder)
    for k, p in named.items():  # the same weights on both sides (init-order parity)
        assert torch.equal(p.detach().cpu(), P[k]), k
    init = {k: p.detach().clone() for k, p in named.items()}

    noise.replay(feat, eps)
    N.lib().abcd_dispatch_reset()
    sc, logits = step.forward_backward(batch["data"].cuda(), bsz, batch["is_offset"].cuda(),
                                       batch["speakers"].cuda(), cfg["N"])
    torch.cuda.synchronize()
    assert N.lib().abcd_device_status() == 0
    ran = N.dispatch()
    tiles = (B + 63) // 64
    grids = {"enc_fwd": tiles * 2 * 16, "enc_bwd": (B + 31) // 32 * 2 * 8, "dec_fwd": tiles * 32,
             "dec_bwd": (B + 31) // 32 * 16}
    for role, kern in zip(("enc_fwd", "enc_bwd", "dec_fwd", "dec_bwd"), KERNELS[cfg["rnn"]]):
        assert ran[role][0] == f"{kern} grid {grids[role]}", (role, ran[role])
        assert ran[role][1] == 1, (role, ran[role])
    # the encoder's weight gradients: one gemm_wg3b launch for both directions (LSTM), split GEMMs (GRU)
    wg = f"{WG_FORM}<144,256> x2" if cfg["rnn"] == "LSTM" else "gemm split (x6s/x6t)"
    assert ran["enc_wgrad"] == (wg, 1), ran["enc_wgrad"]

    obatch = dict(data=batch["data"], batch_sizes=bsz, is_offset=batch["is_offset"], speakers=batch["speakers"])
    out, grads, new, total, _ = O.train_step(P, obatch, ocfg, dict(feat=feat, eps=eps), cfg["N"])

    sc = sc.cpu()
    for i, k in ((engine.EM, "em"), (engine.OFF, "off"), (engine.KL, "kl"), (engine.LOSS, "loss")):
        ref = float(out[k])
        assert abs(float(sc[i]) - ref) <= LOSS_TOL * abs(ref) + 1e-5, (k, float(sc[i]), ref)
    assert rel_err(step.last_hidden, out["last_hidden"]) < 1e-4
    assert rel_err(logits, out["logits"]) < 1e-4
    assert rel_err(step.feats, out["feats"]) < 1e-4
    if not cfg["plain"]:
        assert torch.equal(logits.argmax(-1).cpu(), out["logits"].argmax(-1))
    seen = {}  # tensor -> the observed figures (reported with -rA, kept in profiles/parity_errors.json)
    for k, p in named.items():
        gh = step.flat.grad_of(p).detach().double().cpu()
        gr = grads[k].double()
        seen[k] = dict(rel=rel_err(gh, gr), blk=block_err(gh, gr),
                       norm=abs(float(gh.norm()) - float(gr.norm())) / max(float(gr.norm()), 1e-30))
        assert abs(float(gh.norm()) - float(gr.norm())) <= GRAD_TOL * float(gr.norm()) + 1e-12, \
            (k, float(gh.norm()), float(gr.norm()))
        assert rel_err(gh, gr) < GRAD_TOL, (k, rel_err(gh, gr))

    step.optimizer_step(lr=1.0, momentum=0.0, clip=1.0)
    torch.cuda.synchronize()
    assert abs(float(step.scalars[engine.NORM]) - total) <= 1e-4 * total, (float(step.scalars[engine.NORM]), total)
    clip = abs(float(step.scalars[engine.NORM]) - total) / total
    sgd_bad = []
    for k, p in named.items():
        # the update is formed in fp32 on both sides (p - lr * coef * g): besides
        # GRAD_TOL of the update itself, allow the rounding of the stored parameter
        # (2 ulp of its largest entry) -- the clipped update is ~1e-4 of p here
        dh = p.detach().double().cpu() - init[k].double().cpu()
        dr = new[k].double() - P[k].double()
        ulp = 2 * 2.0 ** -23 * float(P[k].abs().max())
        tol = GRAD_TOL * float(dr.abs().max()) + ulp
        err = float((dh - dr).abs().max())
        seen[k]["sgd"] = max(err - ulp, 0.0) / max(float(dr.abs().max()), 1e-30)  # the part GRAD_TOL has to cover
        if not err <= tol:
            sgd_bad.append((k, err, tol))
    for k, v in seen.items():
        print(f"{name}-B{B} {k}: rel {v['rel']:.2e} blk {v['blk']:.2e} norm {v['norm']:.2e} sgd {v['sgd']:.2e}")
    worst = {m: max(v[m] for v in seen.values()) for m in ("rel", "blk", "norm", "sgd")}
    print(f"{name}-B{B} worst: " + " ".join(f"{m} {x:.2e}" for m, x in worst.items()) + f" clip {clip:.2e}")
    record_property("parity_errors", dict(case=f"{name}-B{B}", clip=clip, worst=worst, tensors=seen))
    dump_observed(f"fullshape-{name}-B{B}", dict(clip=clip, worst=worst, tensors=seen))
    assert not sgd_bad, sgd_bad
    for k, v in seen.items():
        assert v["blk"] < BLOCK_TOL, (k, v["blk"])


def test_side_gate_released_by_per_step_encoder_backward(monkeypatch):
    """A batch past the persistent kernels' resident capacity (B = 544: 17
    encoder BPTT groups x 2 directions x 8 members = 272 workgroups > 256 CUs)
    runs the per-step encoder backward.  The training step arms the
    side-stream gate around its decoder backward, but the gate kernel is only
    queued when a persistent encoder BPTT was launched since the arming
    (side_gate(): target 0 queues nothing); with the per-step encoder backward
    there is nothing to wait for, so the decoder's weight gradients must not
    wait out the gate's spin bound every step.  Checked: the
    dispatch is the per-step one, the step with the gate on is no slower than
    with it off (ABCD_SIDE_GATE=0) beyond noise, and both give the same loss."""
    import time
    sys.path.insert(0, REPO)
    import bench
    from modules import engine, noise, _native as N
    cfg = dict(bench.CONFIGS["c2"], B=544, tmin=12, tmax=24)
    batch = bench.make_batch(cfg, 77, "cpu")
    L = batch["L"]
    g = torch.Generator().manual_seed(78)
    feat = -torch.empty(cfg["B"], cfg["K"]).exponential_(generator=g).log()
    eps = torch.randn(L, cfg["F"], generator=g)
    step = bench.build(cfg, "cuda")
    args = (batch["data"].cuda(), batch["batch_sizes"], batch["is_offset"].cuda(), batch["speakers"].cuda(), cfg["N"])

    def run(gate):
        if gate:
            monkeypatch.delenv("ABCD_SIDE_GATE", raising=False)
        else:
            monkeypatch.setenv("ABCD_SIDE_GATE", "0")
        best, loss = 1e9, None
        for _ in range(3):
            noise.replay(feat, eps)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc, _ = step.forward_backward(*args)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
            loss = float(sc.cpu()[engine.LOSS])
        return best, loss

    N.lib().abcd_dispatch_reset()
    t_on, loss_on = run(True)
    assert "per-step" in N.dispatch()["enc_bwd"][0], N.dispatch()["enc_bwd"]
    assert N.lib().abcd_device_status() == 0
    t_off, loss_off = run(False)
    assert loss_on == loss_off, (loss_on, loss_off)
    assert t_on <= 1.5 * t_off + 0.01, (t_on, t_off)
