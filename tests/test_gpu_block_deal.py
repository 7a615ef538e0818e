"""The cyclic deal of 16-row blocks to the recurrence groups
against the contiguous deal, bit for bit, and against the float64 oracle.

``enc_fwd_persist<*,16,8>``, ``dec_fwd_x6`` (64-row groups) and ``enc_bwd_w8``,
``dec_bwd_w16`` (32-row groups) address a group's rows block by block: local
block j of group g is packed block ``g + groups * j`` (cyclic) or
``g * blocks_per_group + j`` (contiguous, ``ABCD_PERSIST_DEAL=0``).  Each row's
arithmetic is the same under both, and split-K partials are summed per member,
so everything one training step exposes must be EQUAL between the two deals.

One step at H = Hm = 256, F = 129 (feedback on, the decoder's noise drawn
in-kernel from the Philox stream: the idle members' fill walks the group's
rows), T = 6 .. 10, lengths mixed with ties so that the row blocks die at
different steps:

* 32-row-group kernels: B = 17, 33, 48, 65 (65: three groups, row 64 is the
  second block of group 1);
* 64-row-group kernels: B = 65, 80, 129;
* ``PARTIAL``: batches where the last live block is partly filled at every step.

A step runs all four kernels, so every batch goes through every kernel, for the
LSTM; the GRU forms run B = 65 and 129.

Compared with ``torch.equal``: the scalars, logits, last hidden states, the
sampled features, MU / LV / OUT of every frame, and the whole flat gradient.
The dG / dZ stashes and the gradients with respect to the decoder's initial
state and the encoder's output are not addressable from Python; every row of
them is an operand of a weight-gradient GEMM (dW_ih, dW_hh, W1, W2) or of the
sampler's / encoder's backward, whose results are in the flat gradient.

The cyclic step is then held to the float64 oracle with the helpers, tables
and tolerances of tests/test_gpu_decoder_noise.py (those of
tests/test_gpu_edges.py for this rung); no tolerance is introduced here.
"""
import functools

import pytest
import torch

import edge_cases as E
import ladder_cases as L
import noise_cases as NC
import test_gpu_decoder_noise as TN

pytestmark = pytest.mark.gpu

ROLES = ("enc_fwd", "enc_bwd", "dec_fwd", "dec_bwd")
CYCLIC, CONTIGUOUS = "15", "0"  # ABCD_PERSIST_DEAL: every role / none
SEED, OFFSET = 0x5EED1111, NC.HI + 12344

# B -> (T, stride of the length pattern)
SHAPES = {17: (6, 5), 33: (7, 3), 48: (8, 3), 65: (9, 4), 80: (10, 3), 129: (8, 5)}
PARTIAL = (17, 33, 65, 129)
CASES = [("LSTM", B) for B in SHAPES] + [("GRU", 65), ("GRU", 129)]


def lengths(B):
    """B lengths in 1 .. T, every length taken by several rows, the longest T."""
    T, m = SHAPES[B]
    ln = [1 + (i * m) % T for i in range(B)]
    ln[0] = T
    return sorted(ln, reverse=True)


def batch_sizes(B):
    ln = lengths(B)
    return [sum(1 for x in ln if x > t) for t in range(ln[0])]


def test_shapes_have_the_properties_claimed():
    for B, (T, _) in SHAPES.items():
        ln, bs = lengths(B), batch_sizes(B)
        assert 6 <= T <= 10 and len(bs) == T and bs[0] == B
        assert len(set(ln)) == T and all(ln.count(x) > 1 for x in set(ln) if x < T)  # mixed, with ties
        live = [L.cdiv(b, 16) for b in bs]
        assert len(set(live)) >= min(T, L.cdiv(B, 16)) - 1  # the blocks die at different steps
        if B in PARTIAL:
            assert all(b % 16 for b in bs)
    assert L.cdiv(65, 32) == 3 and 64 // 16 == 1 + 3 * 1  # row 64: block 4 = group 1's second block of the cyclic deal


def _run(cfg, P, batch, feat, deal):
    """One forward_backward of a fresh FusedStep under ABCD_PERSIST_DEAL = deal."""
    from modules import _native as N
    step, named, init = TN._build_step(cfg, P, 0.0)
    c = dict(env={"ABCD_PERSIST_DEAL": deal}, L=int(batch["data"].shape[0]), F=cfg["F"], p=0.0)
    with pytest.MonkeyPatch.context() as mp:
        frames = TN._Frames(mp)
        sc, logits, ran, eps_hat, tol = TN._philox_run(step, cfg, batch, feat, SEED, OFFSET, c, frames)
        flat, mu, lv = (t.clone() for t in frames.out)
    deals = N.dispatch_deal()
    exposed = dict(scalars=sc.clone(), logits=logits.clone(), last_hidden=step.last_hidden.clone(),
                   feats=step.feats.clone(), OUT=flat, MU=mu, LV=lv, grad=step.flat.grad.clone())
    return dict(step=step, named=named, init=init, sc=sc, logits=logits, ran=ran, deals=deals, exposed=exposed,
                eps_hat=eps_hat, tol=tol)


@functools.lru_cache(maxsize=None)
def runs(rnn, B):
    """The batch, both deals' steps and the oracle's, computed once per case."""
    from oracle import abcd_oracle as O
    cfg = NC.config(NC.RUNG1, rnn, B)
    ocfg = dict(E.oracle_cfg(cfg), greedy=cfg["greedy"])
    P = O.init_params(ocfg, 1111)
    batch, drawn = E.make_batch(lengths(B), cfg, NC.SEED)
    cyc = _run(cfg, P, batch, drawn["feat"], CYCLIC)
    con = _run(cfg, P, batch, drawn["feat"], CONTIGUOUS)
    # the oracle is fed the fill kernel's values of the same (seed, offset)
    n, F = int(batch["data"].shape[0]), cfg["F"]
    eps = TN._fill("normal", n * F, SEED, OFFSET).reshape(n, F)
    noise = dict(drawn, eps=eps)
    ref = dict(cfg=cfg, ocfg=ocfg, P=P, batch=batch, noise=noise,
               r64=E.oracle64(ocfg, P, batch, noise, E.N_DATA), r32=E.oracle32(ocfg, P, batch, noise, E.N_DATA))
    return dict(cfg=cfg, cyc=cyc, con=con, ref=ref)


@pytest.mark.parametrize("rnn,B", CASES)
def test_cyclic_deal_equals_contiguous_bit_for_bit(rnn, B):
    r = runs(rnn, B)
    expected = NC.expected(NC.RUNG1, rnn, B)
    for run, deal in ((r["cyc"], 1), (r["con"], 0)):
        TN._assert_routes(f"deal-{rnn}-b{B}-{deal}", run["ran"], expected)
        assert run["deals"] == {role: deal for role in ROLES}, run["deals"]
    for k, a in r["cyc"]["exposed"].items():
        b = r["con"]["exposed"][k]
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, b), (k, float((a - b).abs().max()), int((a != b).sum()))


@pytest.mark.parametrize("rnn,B", CASES)
def test_cyclic_deal_step_vs_oracle64(rnn, B, record_property):
    import numpy as np
    r = runs(rnn, B)
    run, ref, cfg = r["cyc"], r["ref"], r["cfg"]
    assert run["deals"] == {role: 1 for role in ROLES}, run["deals"]
    tag = f"deal-{rnn}-b{B}"
    # the noise the launch drew is the stream (noise_cases.eps_hat's tolerance)
    want = NC.stream(SEED, OFFSET, int(ref["batch"]["data"].shape[0]), cfg["F"])
    err = np.abs(run["eps_hat"] - want)
    assert (err <= run["tol"]).all(), float((err - run["tol"]).max())
    TN._judge_step(tag, NC.RUNG1, run["step"], run["named"], run["init"], run["sc"], run["logits"], ref,
                   set(), record_property)
