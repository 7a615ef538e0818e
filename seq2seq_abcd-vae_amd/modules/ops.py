# coding: utf-8
"""The C ABI (``include/abcd_hip.h``) registered as PyTorch custom operators
(``torch.library``, namespace ``abcd``) with their autograd formulas -- the
operator boundary the module classes of ``model.py`` call.

One operator per reference method on the hot path, and one per backward:

=========================  ==============================================  =========================================
operator                   replaces (reference)                            C entry point
=========================  ==============================================  =========================================
``abcd::encoder``          ``RNN_Variational_Encoder.forward`` model.py:60  ``abcd_encoder_forward_dropout``
``abcd::encoder_bwd``      its autograd backward                           ``abcd_encoder_backward_dropout``
``abcd::sampler``          ``ABCDSampler.forward`` model.py:581 /           ``abcd_sampler_forward``
                           ``Sampler.forward`` plain/model.py:552
``abcd::sampler_bwd``      its backward                                    ``abcd_sampler_forward_backward``
``abcd::sampler_sample``   ``ABCDSampler.sample`` model.py:592             ``abcd_sampler_sample``
``abcd::sampler_sample_bwd``                                               ``abcd_sampler_sample_backward``
``abcd::sampler_kl``       ``ABCDSampler.kl_divergence`` model.py:608      ``abcd_sampler_kl``
``abcd::sampler_kl_bwd``                                                   ``abcd_sampler_kl_backward``
``abcd::decoder``          ``RNN_Variational_Decoder.forward`` model.py:147 ``abcd_decoder_forward_dropout``
``abcd::decoder_bwd``      its backward (emission + offset losses)         ``abcd_decoder_backward_dropout``
``abcd::linear``           ``MLP`` layers (Linear [+ Tanh]) model.py:316   ``abcd_linear``
``abcd::linear_bwd``       their backward                                  ``abcd_linear_backward``
``abcd::segment_losses``   (none: per-segment emission NLL / offset BCE)   ``abcd_segment_losses``
``abcd::sampler_kl_rows``  (none: per-row part of ``kl_divergence``)       ``abcd_sampler_kl_rows``
``abcd::pairwise_nll``     (none: every segment x every prototype)         ``abcd_pairwise_nll``
``abcd::pair_posterior``   (none: responsibilities, evidence, argmax)      ``abcd_pair_posterior``
``abcd::griffin_lim``      (none: log-spectra back to audio)               ``abcd_griffin_lim``
``abcd::chain_posterior``  (none: an HMM over category sequences)          ``abcd_chain_posterior``
``abcd::span_scores``      (none: every span of an uncut recording)        ``abcd_span_scores``
``abcd::span_viterbi``     (none: the best cover by segments)              ``abcd_span_viterbi``
``abcd::warp_nll``         (none: segments time-warped to prototypes)      ``abcd_warp_nll``
``abcd::warp_path``        (none: the best alignment and its costs)        ``abcd_warp_path``
``abcd::span_evidence``    (none: span scores summed over the categories)  ``abcd_span_evidence``
``abcd::span_posterior``   (none: posteriors over all covers by segments)  ``abcd_span_posterior``
``abcd::span_table``       (none: span scores of every category)           ``abcd_span_table``
``abcd::span_chain_viterbi`` (none: the best cover under a category chain) ``abcd_span_chain_viterbi``
``abcd::span_chain_posterior`` (none: posteriors and counts under the chain) ``abcd_span_chain_posterior``
``abcd::span_chain_viterbi_window`` (none: that cover, the table in windows) ``abcd_span_chain_viterbi_window``
``abcd::frame_costs``      (none: frames against every prototype step)     ``abcd_frame_costs``
``abcd::warp_segment_window`` (none: the cut with warped prototypes)       ``abcd_warp_segment_window``
``abcd::warp_posterior_forward`` (none: the sum half of that cut, forward) ``abcd_warp_posterior_forward``
``abcd::warp_posterior_backward`` (none: its backward sweep and counts)    ``abcd_warp_posterior_backward``
=========================  ==============================================  =========================================

The last twenty are forward-only (scoring, synthesis, segmentation, alignment): they have no autograd
formula and raise when an input requires grad outside ``torch.no_grad()``.

``span_chain_viterbi_window``, ``warp_segment_window`` and the two ``warp_posterior`` sweeps are the
operators that are NOT functional: they carry a recording's programme from call to call in a state tensor they mutate
(``STATEFUL_OPS``; ``OPS`` lists the functional ones).

Operators take tensors, ints and floats only (no module objects): the
configuration travels as an ``int[]`` in the C struct's field order, the
parameters as a ``Tensor[]`` in the module's parameter order.  The forward
operators also return the kernels' workspace (a uint8 tensor holding the
forward stash the backward reads), so every operator is functional (autograd
formulas need that): ``sampler_sample`` and ``sampler_kl`` each stash into a
workspace of their own.  Philox keys (64-bit) cross the schema as
two's-complement int64.

Every operator runs the HIP kernels on the tensors' device; there is no CPU
kernel (a CPU tensor raises, as everywhere on the product path)."""
import math
from typing import List, Optional, Sequence

import torch

from . import _native as N

Tensor = torch.Tensor
_U64 = (1 << 64) - 1


def _i64(x):
    """uint64 -> int64 (two's complement) for the schema."""
    x = int(x) & _U64
    return x - (1 << 64) if x >= (1 << 63) else x


def _u64(x):
    return int(x) & _U64


def _ptrs(ts):
    return [None if t is None else t.data_ptr() for t in ts]


# ----------------------------------------------------------------------------
# encoder
# ----------------------------------------------------------------------------
def _enc_cfg(cfg):
    c = N.EncoderCfg()
    c.input_size, c.hidden_size, c.rnn_type, c.layers, c.bidirectional = (int(v) for v in cfg)
    return c


def _enc_struct(cfg, ts):
    """ts: (w_ih, w_hh, b_ih, b_hh) per (layer, direction), layer-major."""
    st = N.EncoderParams()
    dirs = 2 if cfg[4] else 1
    for i in range(int(cfg[3]) * dirs):
        l, d = divmod(i, dirs)
        st.w[l][d].w_ih, st.w[l][d].w_hh, st.w[l][d].b_ih, st.w[l][d].b_hh = _ptrs(ts[4 * i:4 * i + 4])
    return st


def _enc_out_width(cfg):
    w = int(cfg[3]) * int(cfg[1]) * (2 if cfg[4] else 1)
    return w * 2 if int(cfg[2]) == N.LSTM else w


@torch.library.custom_op("abcd::encoder", mutates_args=())
def encoder(data: Tensor, batch_sizes: Tensor, weights: List[Tensor], noise: List[Tensor],
            cfg: List[int]) -> List[Tensor]:
    """-> [last hidden (B x hidden_size_total), workspace].  noise: the
    inter-layer dropout masks (layers - 1 of them) or [] (no dropout)."""
    N.require_gpu(data)
    L = N.lib()
    c = _enc_cfg(cfg)
    pk, bs = N.packed(data, batch_sizes, cfg[0])
    nbytes = L.abcd_encoder_workspace_bytes(c, pk.T, pk.L, pk.B)
    if nbytes == 0:
        raise N.HipError("encoder: unsupported configuration (hidden size must be a multiple of 16)")
    ws = N.workspace(nbytes, data.device)
    out = torch.empty(pk.B, _enc_out_width(cfg), device=data.device)
    N.check(L.abcd_encoder_forward_dropout(c, _enc_struct(cfg, weights), pk, N.ptr_array(list(noise) or None), N.ptr(out),
                                           N.ptr(ws), ws.numel(), N.stream()), "encoder forward")
    N.op_status.probe(data.device, "encoder forward")
    return [out, ws]


@encoder.register_fake
def _(data, batch_sizes, weights, noise, cfg):
    B = batch_sizes[0] if batch_sizes.numel() else 0
    return [data.new_empty(int(B), _enc_out_width(cfg)), data.new_empty(0, dtype=torch.uint8)]


@torch.library.custom_op("abcd::encoder_bwd", mutates_args=())
def encoder_bwd(data: Tensor, batch_sizes: Tensor, weights: List[Tensor], noise: List[Tensor],
                ws: Tensor, d_out: Tensor, cfg: List[int]) -> List[Tensor]:
    c = _enc_cfg(cfg)
    pk, bs = N.packed(data, batch_sizes, cfg[0])
    grads = [torch.empty_like(w) for w in weights]
    N.check(N.lib().abcd_encoder_backward_dropout(c, _enc_struct(cfg, weights), pk, N.ptr_array(list(noise) or None),
                                                  N.ptr(d_out.contiguous()), _enc_struct(cfg, grads), N.ptr(ws),
                                                  ws.numel(), N.stream(), None), "encoder backward")
    N.op_status.probe(data.device, "encoder backward")
    return grads


@encoder_bwd.register_fake
def _(data, batch_sizes, weights, noise, ws, d_out, cfg):
    return [torch.empty_like(w) for w in weights]


def _encoder_setup(ctx, inputs, output):
    data, batch_sizes, weights, noise, cfg = inputs
    ctx.data, ctx.batch_sizes, ctx.weights, ctx.noise, ctx.cfg = data, batch_sizes, weights, noise, cfg
    ctx.ws = output[1]
    ctx.mark_non_differentiable(output[1])


def _encoder_backward(ctx, grads):
    d_out = grads[0]
    g = encoder_bwd(ctx.data, ctx.batch_sizes, list(ctx.weights), ctx.noise, ctx.ws, d_out, list(ctx.cfg))
    return None, None, g, [None] * len(ctx.noise), None


encoder.register_autograd(_encoder_backward, setup_context=_encoder_setup)


# ----------------------------------------------------------------------------
# samplers (ABCD: cfg[4] == 0; plain Gaussian: cfg[4] == 1)
# ----------------------------------------------------------------------------
def _samp_cfg(cfg):
    """cfg: [input_size, mlp_hidden, num_categories, feature_dim, plain(, valid_categories, valid_feature_dim)]"""
    c = N.SamplerCfg()
    v = [int(x) for x in cfg] + [0] * (7 - len(cfg))
    (c.input_size, c.mlp_hidden, c.num_categories, c.feature_dim, c.plain, c.valid_categories,
     c.valid_feature_dim) = v
    return c


def _samp_struct(cfg, mlp, codebook=None, psl=None, prior=1.0):
    st = N.SamplerParams()
    for k in range(len(mlp) // 4):
        st.mlp[k].w1, st.mlp[k].b1, st.mlp[k].w2, st.mlp[k].b2 = _ptrs(mlp[4 * k:4 * k + 4])
    st.codebook = None if codebook is None else codebook.data_ptr()
    st.posterior_shape_logits = None if psl is None else psl.data_ptr()
    st.prior_concentration = float(prior)
    return st


def _logit_width(cfg):
    return 2 * int(cfg[3]) if cfg[4] else int(cfg[2])


def _sampler_ws(cfg, B, device):
    nbytes = N.lib().abcd_sampler_workspace_bytes(_samp_cfg(cfg), B)
    if nbytes == 0:
        raise N.HipError("sampler: unsupported configuration (sizes must be multiples of 16)")
    return N.workspace(nbytes, device)


@torch.library.custom_op("abcd::sampler", mutates_args=())
def sampler(h: Tensor, mlp: List[Tensor], codebook: Optional[Tensor], cfg: List[int]) -> List[Tensor]:
    """-> [logits (B x K; plain: [mean | log_var], B x 2f), workspace]"""
    N.require_gpu(h)
    h = h.contiguous()
    B = h.shape[0]
    ws = _sampler_ws(cfg, B, h.device)
    out = torch.empty(B, _logit_width(cfg), device=h.device)
    N.check(N.lib().abcd_sampler_forward(_samp_cfg(cfg), _samp_struct(cfg, mlp, codebook), N.ptr(h), B, N.ptr(out),
                                         N.ptr(ws), ws.numel(), N.stream()), "sampler forward")
    return [out, ws]


@sampler.register_fake
def _(h, mlp, codebook, cfg):
    return [h.new_empty(h.shape[0], _logit_width(cfg)), h.new_empty(0, dtype=torch.uint8)]


@torch.library.custom_op("abcd::sampler_bwd", mutates_args=())
def sampler_bwd(h: Tensor, mlp: List[Tensor], codebook: Optional[Tensor], ws: Tensor, d_logits: Tensor,
                cfg: List[int]) -> List[Tensor]:
    """-> [d_h, d_mlp..., (d_codebook)]"""
    h = h.contiguous()
    d_h = torch.empty_like(h)
    gm = [torch.empty_like(t) for t in mlp]
    gc = None if codebook is None else torch.empty_like(codebook)
    g = N.SamplerGrads()
    for k in range(len(mlp) // 4):
        g.mlp[k].w1, g.mlp[k].b1, g.mlp[k].w2, g.mlp[k].b2 = _ptrs(gm[4 * k:4 * k + 4])
    g.codebook = None if gc is None else gc.data_ptr()
    N.check(N.lib().abcd_sampler_forward_backward(_samp_cfg(cfg), _samp_struct(cfg, mlp, codebook), N.ptr(h),
                                                  h.shape[0], N.ptr(d_logits.contiguous()), N.ptr(d_h), g, 0,
                                                  N.ptr(ws), ws.numel(), N.stream()), "sampler forward backward")
    return [d_h] + gm + ([] if gc is None else [gc])


@sampler_bwd.register_fake
def _(h, mlp, codebook, ws, d_logits, cfg):
    return [torch.empty_like(h)] + [torch.empty_like(t) for t in mlp] + ([] if codebook is None
                                                                         else [torch.empty_like(codebook)])


def _sampler_setup(ctx, inputs, output):
    h, mlp, codebook, cfg = inputs
    ctx.h, ctx.mlp, ctx.codebook, ctx.cfg, ctx.ws = h, mlp, codebook, cfg, output[1]
    ctx.mark_non_differentiable(output[1])


def _sampler_backward(ctx, grads):
    g = sampler_bwd(ctx.h, list(ctx.mlp), ctx.codebook, ctx.ws, grads[0], list(ctx.cfg))
    nm = len(ctx.mlp)
    return g[0], g[1:1 + nm], (g[1 + nm] if ctx.codebook is not None else None), None


sampler.register_autograd(_sampler_backward, setup_context=_sampler_setup)


@torch.library.custom_op("abcd::sampler_sample", mutates_args=())
def sampler_sample(logits: Tensor, codebook: Optional[Tensor], cfg: List[int], mode: int, temperature: float,
                   noise: Optional[Tensor], seed: int, offset: int) -> List[Tensor]:
    """-> [feats (B x D), workspace]: ABCD Gumbel-softmax / softmax y C^T;
    plain mu + e^{lv/2} eps.  The workspace holds the stash its backward reads."""
    N.require_gpu(logits)
    logits = logits.contiguous()
    B = logits.shape[0]
    ws = _sampler_ws(cfg, B, logits.device)
    feats = torch.empty(B, int(cfg[3]), device=logits.device)
    N.check(N.lib().abcd_sampler_sample(_samp_cfg(cfg), _samp_struct(cfg, [], codebook), N.ptr(logits), B,
                                        int(mode), float(temperature), N.ptr(noise), _u64(seed), _u64(offset),
                                        N.ptr(feats), N.ptr(ws), ws.numel(), N.stream()), "sampler sample")
    return [feats, ws]


@sampler_sample.register_fake
def _(logits, codebook, cfg, mode, temperature, noise, seed, offset):
    return [logits.new_empty(logits.shape[0], int(cfg[3])), logits.new_empty(0, dtype=torch.uint8)]


@torch.library.custom_op("abcd::sampler_sample_bwd", mutates_args=())
def sampler_sample_bwd(ws: Tensor, codebook: Optional[Tensor], d_feats: Tensor, cfg: List[int], B: int, mode: int,
                       temperature: float) -> List[Tensor]:
    """-> [d_logits, (d_codebook)]"""
    d_logits = torch.empty(B, _logit_width(cfg), device=d_feats.device)
    d_cb = None if codebook is None else torch.empty_like(codebook)
    N.check(N.lib().abcd_sampler_sample_backward(_samp_cfg(cfg), _samp_struct(cfg, [], codebook), B, int(mode),
                                                 float(temperature), N.ptr(d_feats.contiguous()), N.ptr(d_logits),
                                                 N.ptr(d_cb), N.ptr(ws), ws.numel(), N.stream()),
            "sampler sample backward")
    return [d_logits] + ([] if d_cb is None else [d_cb])


@sampler_sample_bwd.register_fake
def _(ws, codebook, d_feats, cfg, B, mode, temperature):
    return [d_feats.new_empty(B, _logit_width(cfg))] + ([] if codebook is None else [torch.empty_like(codebook)])


def _sample_setup(ctx, inputs, output):
    logits, codebook, cfg, mode, temperature, noise, seed, offset = inputs
    ctx.ws, ctx.codebook, ctx.cfg, ctx.mode, ctx.tau, ctx.B = output[1], codebook, cfg, mode, temperature, \
        logits.shape[0]
    ctx.mark_non_differentiable(output[1])


def _sample_backward(ctx, grads):
    g = sampler_sample_bwd(ctx.ws, ctx.codebook, grads[0], list(ctx.cfg), ctx.B, ctx.mode, ctx.tau)
    return g[0], (g[1] if ctx.codebook is not None else None), None, None, None, None, None, None


sampler_sample.register_autograd(_sample_backward, setup_context=_sample_setup)


@torch.library.custom_op("abcd::sampler_kl", mutates_args=())
def sampler_kl(logits: Tensor, psl: Optional[Tensor], cfg: List[int], prior: float,
               entire_data_size: float) -> List[Tensor]:
    """-> [KL scalar, workspace]: ABCD Dirichlet-categorical; plain Gaussian"""
    N.require_gpu(logits)
    logits = logits.contiguous()
    ws = _sampler_ws(cfg, logits.shape[0], logits.device)
    kl = torch.empty((), device=logits.device)
    N.check(N.lib().abcd_sampler_kl(_samp_cfg(cfg), _samp_struct(cfg, [], None, psl, prior), N.ptr(logits),
                                    logits.shape[0], float(entire_data_size), N.ptr(kl), N.ptr(ws), ws.numel(),
                                    N.stream()), "sampler kl")
    return [kl, ws]


@sampler_kl.register_fake
def _(logits, psl, cfg, prior, entire_data_size):
    return [logits.new_empty(()), logits.new_empty(0, dtype=torch.uint8)]


@torch.library.custom_op("abcd::sampler_kl_bwd", mutates_args=())
def sampler_kl_bwd(ws: Tensor, psl: Optional[Tensor], d_kl: Tensor, cfg: List[int], B: int, prior: float,
                   entire_data_size: float) -> List[Tensor]:
    """-> [d_logits, (d_posterior_shape_logits)]"""
    d_logits = torch.empty(B, _logit_width(cfg), device=d_kl.device)
    d_psl = None if psl is None else torch.empty_like(psl)
    N.check(N.lib().abcd_sampler_kl_backward(_samp_cfg(cfg), _samp_struct(cfg, [], None, psl, prior), B,
                                             float(entire_data_size), N.ptr(d_kl.reshape(()).contiguous()), 0,
                                             N.ptr(d_logits), N.ptr(d_psl), N.ptr(ws), ws.numel(), N.stream()),
            "sampler kl backward")
    return [d_logits] + ([] if d_psl is None else [d_psl])


@sampler_kl_bwd.register_fake
def _(ws, psl, d_kl, cfg, B, prior, entire_data_size):
    return [d_kl.new_empty(B, _logit_width(cfg))] + ([] if psl is None else [torch.empty_like(psl)])


def _kl_setup(ctx, inputs, output):
    logits, psl, cfg, prior, n = inputs
    ctx.ws, ctx.psl, ctx.cfg, ctx.prior, ctx.n, ctx.B = output[1], psl, cfg, prior, n, logits.shape[0]
    ctx.mark_non_differentiable(output[1])


def _kl_backward(ctx, grads):
    g = sampler_kl_bwd(ctx.ws, ctx.psl, grads[0], list(ctx.cfg), ctx.B, ctx.prior, ctx.n)
    return g[0], (g[1] if ctx.psl is not None else None), None, None, None


sampler_kl.register_autograd(_kl_backward, setup_context=_kl_setup)


# ----------------------------------------------------------------------------
# decoder
# ----------------------------------------------------------------------------
def _dec_cfg(cfg):
    c = N.DecoderCfg()
    (c.output_size, c.hidden_size, c.mlp_hidden, c.feature_size, c.rnn_type, c.feedback, c.num_speakers,
     c.speaker_dim) = (int(v) for v in cfg)
    return c


def _dec_struct(cfg, ts):
    """ts: [embed_speaker (if cfg[6])] f2h_w f2h_b offset(4) mu(4) lv(4) cell(w_ih w_hh b_ih b_hh)"""
    st = N.DecoderParams()
    i = 0
    if int(cfg[6]):
        st.embed_speaker = None if ts[0] is None else ts[0].data_ptr()
        i = 1
    p = _ptrs(ts[i:])
    st.f2h_w, st.f2h_b = p[0], p[1]
    for name, k in (("offset", 2), ("mu", 6), ("lv", 10)):
        m = getattr(st, name)
        m.w1, m.b1, m.w2, m.b2 = p[k:k + 4]
    st.cell.w_ih, st.cell.w_hh, st.cell.b_ih, st.cell.b_hh = p[14:18]
    return st


@torch.library.custom_op("abcd::decoder", mutates_args=())
def decoder(features: Tensor, batch_sizes: Tensor, speaker: Optional[Tensor], gt: Optional[Tensor],
            gt_off: Optional[Tensor], eps: Optional[Tensor], seed: int, offset: int, xmask: Optional[Tensor],
            params: List[Tensor], cfg: List[int]) -> List[Tensor]:
    """-> [em, off, flat, mu, lv, offset_logits, workspace]; em / off are 0-d
    (0 when the target is absent); flat / mu / lv are L x F."""
    N.require_gpu(features)
    features = features.contiguous()
    L_ = N.lib()
    c = _dec_cfg(cfg)
    F = int(cfg[0])
    pk, bs = N.packed(gt, batch_sizes, F)
    nbytes = L_.abcd_decoder_workspace_bytes(c, pk.T, pk.L, pk.B)
    if nbytes == 0:
        raise N.HipError("decoder: unsupported configuration (sizes must be multiples of 16)")
    dev = features.device
    ws = N.workspace(nbytes, dev)
    spk = speaker.to(dev, torch.int64).contiguous() if int(cfg[6]) else None
    flat = torch.empty(pk.L, F, device=dev)
    mu = torch.empty(pk.L, F, device=dev)
    lv = torch.empty(pk.L, F, device=dev)
    offl = torch.empty(pk.L, device=dev)
    losses = torch.zeros(2, device=dev)
    N.check(L_.abcd_decoder_forward_dropout(c, _dec_struct(cfg, params), pk, N.ptr(features), N.ptr(spk),
                                            N.ptr(None if gt_off is None else gt_off.contiguous()), N.ptr(eps),
                                            N.ptr(xmask), _u64(seed), _u64(offset), N.ptr(flat), N.ptr(mu),
                                            N.ptr(lv), N.ptr(offl), N.ptr(losses), N.ptr(ws), ws.numel(),
                                            N.stream()), "decoder forward")
    N.op_status.probe(dev, "decoder forward")
    return [losses[0].clone(), losses[1].clone(), flat, mu, lv, offl, ws]


@decoder.register_fake
def _(features, batch_sizes, speaker, gt, gt_off, eps, seed, offset, xmask, params, cfg):
    L = int(batch_sizes.sum())
    F = int(cfg[0])
    e = features.new_empty
    return [e(()), e(()), e(L, F), e(L, F), e(L, F), e(L), features.new_empty(0, dtype=torch.uint8)]


@torch.library.custom_op("abcd::decoder_bwd", mutates_args=())
def decoder_bwd(features: Tensor, batch_sizes: Tensor, speaker: Optional[Tensor], gt: Tensor, gt_off: Tensor,
                xmask: Optional[Tensor], params: List[Tensor], ws: Tensor, d_em: Tensor, d_off: Tensor,
                cfg: List[int]) -> List[Tensor]:
    """-> [d_features, d_params...]"""
    c = _dec_cfg(cfg)
    pk, bs = N.packed(gt, batch_sizes, int(cfg[0]))
    dev = features.device
    spk = speaker.to(dev, torch.int64).contiguous() if int(cfg[6]) else None
    grads = [torch.empty_like(p) for p in params]
    d_features = torch.empty_like(features)
    N.check(N.lib().abcd_decoder_backward_dropout(c, _dec_struct(cfg, params), pk, N.ptr(features.contiguous()),
                                                  N.ptr(spk), N.ptr(gt_off.contiguous()), N.ptr(xmask),
                                                  N.ptr(d_em.reshape(()).contiguous()),
                                                  N.ptr(d_off.reshape(()).contiguous()), N.ptr(d_features),
                                                  _dec_struct(cfg, grads), N.ptr(ws), ws.numel(), N.stream(), None),
            "decoder backward")
    N.op_status.probe(dev, "decoder backward")
    return [d_features] + grads


@decoder_bwd.register_fake
def _(features, batch_sizes, speaker, gt, gt_off, xmask, params, ws, d_em, d_off, cfg):
    return [torch.empty_like(features)] + [torch.empty_like(p) for p in params]


def _decoder_setup(ctx, inputs, output):
    features, batch_sizes, speaker, gt, gt_off, eps, seed, offset, xmask, params, cfg = inputs
    ctx.saved = (features, batch_sizes, speaker, gt, gt_off, xmask, params, cfg)
    ctx.ws = output[6]
    ctx.mark_non_differentiable(*output[2:])  # per-frame outputs and the workspace: inspection only
    ctx.set_materialize_grads(False)


def _decoder_backward(ctx, grads):
    d_em, d_off = grads[0], grads[1]
    features, batch_sizes, speaker, gt, gt_off, xmask, params, cfg = ctx.saved
    if gt is None or gt_off is None:
        raise NotImplementedError("decoder backward needs ground_truth_out and ground_truth_offset "
                                  "(the losses it differentiates)")
    z = torch.zeros((), device=features.device)
    d_em = z if d_em is None else d_em
    d_off = z if d_off is None else d_off
    g = decoder_bwd(features, batch_sizes, speaker, gt, gt_off, xmask, list(params), ctx.ws, d_em, d_off, list(cfg))
    return g[0], None, None, None, None, None, None, None, None, g[1:], None


decoder.register_autograd(_decoder_backward, setup_context=_decoder_setup)


# ----------------------------------------------------------------------------
# nn.Linear (+ Tanh): the standalone MLP (model.py:316-334) outside the step
# ----------------------------------------------------------------------------
def _linear_ws(rows, cols, depth, device, backward=False):
    if backward:
        return N.workspace(N.lib().abcd_linear_backward_workspace_bytes(rows, cols, depth), device)
    Kp = (max(depth, cols) + 15) // 16 * 16
    return N.workspace((rows + cols) * Kp * 4 + (1 << 22), device)


@torch.library.custom_op("abcd::linear", mutates_args=())
def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor], act: int) -> Tensor:
    """y = act(x W^T + b), act 0 = identity, 1 = tanh; x M x K, W N x K."""
    N.require_gpu(x)
    x = x.contiguous()
    weight = weight.contiguous()
    M, K = x.shape
    Nn = weight.shape[0]
    y = torch.empty(M, Nn, device=x.device)
    ws = _linear_ws(M, Nn, K, x.device)
    N.check(N.lib().abcd_linear(M, Nn, K, N.ptr(x), K, N.ptr(weight), K, N.ptr(None if bias is None else bias.contiguous()),
                                int(act), N.ptr(y), Nn, N.ptr(ws), ws.numel(), N.stream()), "linear")
    return y


@linear.register_fake
def _(x, weight, bias, act):
    return x.new_empty(x.shape[0], weight.shape[0])


@torch.library.custom_op("abcd::linear_bwd", mutates_args=())
def linear_bwd(x: Tensor, weight: Tensor, y: Tensor, dy: Tensor, act: int, need_bias: bool) -> List[Tensor]:
    """-> [dx, dW, db (empty when need_bias is false)]"""
    x, weight, y, dy = x.contiguous(), weight.contiguous(), y.contiguous(), dy.contiguous()
    M, K = x.shape
    Nn = weight.shape[0]
    dx = torch.empty_like(x)
    dW = torch.empty_like(weight)
    db = torch.empty(Nn if need_bias else 0, device=x.device)
    ws = _linear_ws(M, Nn, K, x.device, backward=True)
    N.check(N.lib().abcd_linear_backward(M, Nn, K, N.ptr(x), K, N.ptr(weight), K, N.ptr(y), Nn, int(act), N.ptr(dy),
                                         Nn, N.ptr(dx), K, N.ptr(dW), N.ptr(db) if need_bias else None, N.ptr(ws),
                                         ws.numel(), N.stream()), "linear backward")
    return [dx, dW, db]


@linear_bwd.register_fake
def _(x, weight, y, dy, act, need_bias):
    return [torch.empty_like(x), torch.empty_like(weight), x.new_empty(weight.shape[0] if need_bias else 0)]


def _linear_setup(ctx, inputs, output):
    x, weight, bias, act = inputs
    ctx.save_for_backward(x, weight, output)
    ctx.act, ctx.has_bias = act, bias is not None


def _linear_backward(ctx, dy):
    x, weight, y = ctx.saved_tensors
    dx, dW, db = linear_bwd(x, weight, y, dy, ctx.act, ctx.has_bias)
    return dx, dW, (db if ctx.has_bias else None), None


linear.register_autograd(_linear_backward, setup_context=_linear_setup)


# ----------------------------------------------------------------------------
# per-segment scoring (forward-only)
# ----------------------------------------------------------------------------
def _forward_only(op, name):
    """No autograd formula: an input that requires grad (with grad mode on)
    raises here instead of silently returning constants."""
    def setup(ctx, inputs, output):
        raise RuntimeError(f"abcd::{name} is forward-only (per-segment scores have no gradient): call it under "
                           "torch.no_grad() or on detached tensors")

    def backward(ctx, *grads):
        raise RuntimeError(f"abcd::{name} is forward-only (per-segment scores have no gradient)")

    op.register_autograd(backward, setup_context=setup)


def _rows(t):
    """(tensor, row stride): a row-strided 2-d view passes as it is; anything else is made contiguous."""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t, t.stride(0)
    t = t.contiguous()
    return t, t.shape[1]


@torch.library.custom_op("abcd::segment_losses", mutates_args=())
def segment_losses(gt: Optional[Tensor], batch_sizes: Tensor, mu: Optional[Tensor], log_var: Optional[Tensor],
                   offset_logits: Optional[Tensor], gt_offset: Optional[Tensor], F: int) -> List[Tensor]:
    """-> [em (B), off (B), lengths (B, int32)] in packed row order: the
    emission NLL of (gt, mu, log_var) (L x F each; zeros when one is None) and
    the offset BCE of (offset_logits, gt_offset) (L each; zeros when one is
    None) summed per segment, and the segments' lengths.  mu / log_var may be
    row-strided views (stride(0) >= F, stride(1) == 1)."""
    ref = next((t for t in (gt, mu, log_var, offset_logits, gt_offset) if t is not None), None)
    if ref is None:
        raise ValueError("segment_losses: no input tensor (the lengths alone follow from batch_sizes on the host)")
    N.require_gpu(ref)
    dev = ref.device
    want_em = gt is not None and mu is not None and log_var is not None
    want_off = offset_logits is not None and gt_offset is not None
    gt = gt.contiguous() if want_em else None
    (mu, ldm), (log_var, ldl) = (_rows(mu), _rows(log_var)) if want_em else ((None, 0), (None, 0))
    offset_logits = offset_logits.contiguous() if want_off else None
    gt_offset = gt_offset.contiguous() if want_off else None
    L_ = N.lib()
    pk, bs = N.packed(gt, batch_sizes, F)
    if want_em and not (tuple(mu.shape) == tuple(log_var.shape) == (pk.L, int(F)) and gt.shape[1] == int(F)):
        raise ValueError(f"segment_losses: gt, mu and log_var must be {(pk.L, int(F))}")
    if want_off and not (offset_logits.numel() == gt_offset.numel() == pk.L):
        raise ValueError(f"segment_losses: offset_logits and gt_offset must hold {pk.L} entries")
    nbytes = L_.abcd_segment_losses_workspace_bytes(pk.T, pk.B)
    if nbytes == 0:
        raise N.HipError("segment_losses: unsupported number of steps")
    ws = N.workspace(nbytes, dev)
    em = torch.empty(pk.B, device=dev) if want_em else torch.zeros(pk.B, device=dev)
    off = torch.empty(pk.B, device=dev) if want_off else torch.zeros(pk.B, device=dev)
    lengths = torch.empty(pk.B, dtype=torch.int32, device=dev)
    N.check(L_.abcd_segment_losses(pk, N.ptr(mu), ldm, N.ptr(log_var), ldl, N.ptr(offset_logits), N.ptr(gt_offset),
                                   N.ptr(em) if want_em else None, N.ptr(off) if want_off else None, N.ptr(lengths),
                                   N.ptr(ws), ws.numel(), N.stream()), "segment losses")
    return [em, off, lengths]


@segment_losses.register_fake
def _(gt, batch_sizes, mu, log_var, offset_logits, gt_offset, F):
    ref = next(t for t in (gt, mu, log_var, offset_logits, gt_offset) if t is not None)
    B = int(batch_sizes[0]) if batch_sizes.numel() else 0
    return [ref.new_empty(B, dtype=torch.float32), ref.new_empty(B, dtype=torch.float32),
            ref.new_empty(B, dtype=torch.int32)]


_forward_only(segment_losses, "segment_losses")


@torch.library.custom_op("abcd::sampler_kl_rows", mutates_args=())
def sampler_kl_rows(logits: Tensor, psl: Optional[Tensor], cfg: List[int], prior: float,
                    entire_data_size: float) -> List[Tensor]:
    """-> [rows (B), prior (0-d)]: ABCD rows[b] = sum_k q log q - sum_k q elog[k]
    and the batch-independent Dirichlet bracket (kl = prior * B / N + rows.sum());
    plain rows[b] = -0.5 sum_f (1 + lv - mu^2 - e^lv), prior = 0."""
    N.require_gpu(logits)
    logits = logits.contiguous()
    B = logits.shape[0]
    if logits.shape[1] != _logit_width(cfg):
        raise ValueError(f"sampler_kl_rows: logits must be B x {_logit_width(cfg)}, got {tuple(logits.shape)}")
    rows = torch.empty(B, device=logits.device)
    pr = torch.empty((), device=logits.device)
    N.check(N.lib().abcd_sampler_kl_rows(_samp_cfg(cfg), _samp_struct(cfg, [], None, psl, prior), N.ptr(logits), B,
                                         float(entire_data_size), N.ptr(rows), N.ptr(pr), None, 0, N.stream()),
            "sampler kl rows")
    return [rows, pr]


@sampler_kl_rows.register_fake
def _(logits, psl, cfg, prior, entire_data_size):
    return [logits.new_empty(logits.shape[0]), logits.new_empty(())]


_forward_only(sampler_kl_rows, "sampler_kl_rows")


@torch.library.custom_op("abcd::pairwise_nll", mutates_args=())
def pairwise_nll(gt: Optional[Tensor], batch_sizes: Tensor, gt_offset: Optional[Tensor], proto_mu: Optional[Tensor],
                 proto_lv: Optional[Tensor], proto_offset_logits: Optional[Tensor], P: int, F: int) -> List[Tensor]:
    """-> [em (B x P), off (B x P)]: every segment of the packed batch (gt L x
    F, gt_offset L) against every prototype.  The prototypes are a time-major
    rectangle, prototype p at step t in row t * P + p: proto_mu / proto_lv
    (T_proto * P x F, row-strided views pass without a copy) and
    proto_offset_logits (T_proto * P), T_proto >= the batch's steps.  em needs
    (gt, proto_mu, proto_lv), off needs (gt_offset, proto_offset_logits); the
    one whose inputs are absent is zeros."""
    ref = next((t for t in (gt, gt_offset, proto_mu, proto_lv, proto_offset_logits) if t is not None), None)
    if ref is None:
        raise ValueError("pairwise_nll: no input tensor")
    for t in (gt, gt_offset, proto_mu, proto_lv, proto_offset_logits):
        if t is not None:
            N.require_gpu(t)
    dev = ref.device
    P, F = int(P), int(F)
    want_em = gt is not None and proto_mu is not None and proto_lv is not None
    want_off = gt_offset is not None and proto_offset_logits is not None
    if not (want_em or want_off):
        raise ValueError("pairwise_nll: needs (gt, proto_mu, proto_lv) or (gt_offset, proto_offset_logits)")
    if P < 1:
        raise ValueError("pairwise_nll: P must be at least 1")
    gt = gt.contiguous() if want_em else None
    (mu, ldm), (lv, ldl) = (_rows(proto_mu), _rows(proto_lv)) if want_em else ((None, 0), (None, 0))
    ol = proto_offset_logits.contiguous() if want_off else None
    gt_offset = gt_offset.contiguous() if want_off else None
    L_ = N.lib()
    pk, bs = N.packed(gt, batch_sizes, F)
    rows = mu.shape[0] if want_em else ol.numel()
    if rows % P or rows // P < pk.T:
        raise ValueError(f"pairwise_nll: the prototype rectangle must hold T_proto * {P} rows with T_proto >= {pk.T}, "
                         f"got {rows}")
    if want_em and not (tuple(mu.shape) == tuple(lv.shape) == (rows, F) and tuple(gt.shape) == (pk.L, F)):
        raise ValueError(f"pairwise_nll: gt must be {(pk.L, F)}, proto_mu and proto_lv {(rows, F)}")
    if want_off and not (gt_offset.numel() == pk.L and ol.numel() == rows):
        raise ValueError(f"pairwise_nll: gt_offset must hold {pk.L} entries, proto_offset_logits {rows}")
    nbytes = L_.abcd_pairwise_nll_workspace_bytes(pk.T, pk.B, P)
    if nbytes == 0:
        raise N.HipError("pairwise_nll: unsupported shape (more than 16383 steps, or B * P >= 2^31)")
    ws = N.workspace(nbytes, dev)
    em = torch.empty(pk.B, P, device=dev) if want_em else torch.zeros(pk.B, P, device=dev)
    off = torch.empty(pk.B, P, device=dev) if want_off else torch.zeros(pk.B, P, device=dev)
    N.check(L_.abcd_pairwise_nll(pk, N.ptr(gt_offset), P, rows // P, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(ol),
                                 N.ptr(em) if want_em else None, N.ptr(off) if want_off else None, P, N.ptr(ws),
                                 ws.numel(), N.stream()), "pairwise nll")
    return [em, off]


@pairwise_nll.register_fake
def _pairwise_nll_fake(gt, batch_sizes, gt_offset, proto_mu, proto_lv, proto_offset_logits, P, F):
    ref = next(t for t in (gt, gt_offset, proto_mu, proto_lv, proto_offset_logits) if t is not None)
    B = int(batch_sizes[0]) if batch_sizes.numel() else 0
    return [ref.new_empty(B, int(P), dtype=torch.float32), ref.new_empty(B, int(P), dtype=torch.float32)]


_forward_only(pairwise_nll, "pairwise_nll")


@torch.library.custom_op("abcd::pair_posterior", mutates_args=())
def pair_posterior(pair_em: Tensor, pair_off: Optional[Tensor], log_weight: Optional[Tensor]) -> List[Tensor]:
    """-> [log_evidence (B), best (B, int32), best_prob (B), resp (B x P)] of the
    scores s[b, p] = log_weight[p] - pair_em[b, p] - pair_off[b, p] (absent
    terms count as 0), taken in fp64: log_evidence = logsumexp_p s, resp =
    exp(s - log_evidence), best the lowest index of the maximum (-1 when every
    prototype is excluded by a NaN / +inf NLL or a NaN / -inf weight)."""
    N.require_gpu(pair_em)
    if pair_em.dim() != 2 or pair_em.shape[0] < 1 or pair_em.shape[1] < 1:
        raise ValueError(f"pair_posterior: pair_em must be B x P, got {tuple(pair_em.shape)}")
    B, P = (int(v) for v in pair_em.shape)
    dev = pair_em.device
    em, ld = _rows(pair_em.float())
    off = None
    if pair_off is not None:
        N.require_gpu(pair_off)
        if tuple(pair_off.shape) != (B, P):
            raise ValueError(f"pair_posterior: pair_off must be {(B, P)}, got {tuple(pair_off.shape)}")
        off, ldo = _rows(pair_off.float())
        if ldo != ld:  # one row stride serves both
            em, off, ld = em.contiguous(), off.contiguous(), P
    lw = None
    if log_weight is not None:
        N.require_gpu(log_weight)
        if log_weight.numel() != P:
            raise ValueError(f"pair_posterior: log_weight must hold {P} entries, got {log_weight.numel()}")
        lw = log_weight.float().contiguous()
    ev = torch.empty(B, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    bp = torch.empty(B, device=dev)
    resp = torch.empty(B, P, device=dev)
    N.check(N.lib().abcd_pair_posterior(N.ptr(em), N.ptr(off), ld, B, P, N.ptr(lw), N.ptr(ev), N.ptr(best), N.ptr(bp),
                                        N.ptr(resp), P, N.stream()), "pair posterior")
    return [ev, best, bp, resp]


@pair_posterior.register_fake
def _(pair_em, pair_off, log_weight):
    B, P = pair_em.shape
    e = pair_em.new_empty
    return [e(B, dtype=torch.float32), e(B, dtype=torch.int32), e(B, dtype=torch.float32),
            e(B, P, dtype=torch.float32)]


_forward_only(pair_posterior, "pair_posterior")


# ----------------------------------------------------------------------------
# a hidden Markov model over category sequences (forward-only)
# ----------------------------------------------------------------------------
CHAIN_EVIDENCE, CHAIN_GAMMA, CHAIN_PATH, CHAIN_COUNTS = 1, 2, 4, 8  # the groups of `want` (abcd_hip.h)
CHAIN_ALL = 15


def chain_plan(K, S):
    """(resident, workgroups) of abcd_chain_plan: whether K runs with log_trans
    resident in LDS, and how many workgroups S sequences get."""
    res, wg = N.c_int(0), N.c_int(0)
    N.check(N.lib().abcd_chain_plan(int(K), int(S), res, wg), "chain plan")
    return bool(res.value), int(wg.value)


def chain_scores(pair_em: Tensor, pair_off: Optional[Tensor], log_weight: Optional[Tensor] = None):
    """-> (score B x K fp32, row_offset B fp64): s = log_weight - pair_em -
    pair_off formed in float64 on the device (the NLLs are ~1e5 with gaps of
    order 1, as in pair_posterior) with each row's maximum taken off; s =
    score + row_offset[:, None].  NaN and +inf NLLs become -inf scores; a row
    with nothing left keeps offset 0."""
    s = -pair_em.double()
    if pair_off is not None:
        s = s - pair_off.double()
    if log_weight is not None:
        s = s + log_weight.double()[None, :]
    ninf = torch.full_like(s, float("-inf"))
    s = torch.where((s > float("-inf")) & (s < float("inf")), s, ninf)
    m = s.max(dim=1).values
    m = torch.where(m > float("-inf"), m, torch.zeros_like(m))
    return (s - m[:, None]).float(), m


@torch.library.custom_op("abcd::chain_posterior", mutates_args=())
def chain_posterior(score: Tensor, seq_off: Tensor, log_trans: Tensor, log_init: Tensor, want: int) -> List[Tensor]:
    """-> [log_evidence (S, fp64), gamma (N x K), path (N, int32), path_score
    (S, fp64), trans_counts (K x K, fp64), init_counts (K, fp64)] of the hidden
    Markov model with emission scores score (N x K, row-strided views pass
    without a copy), sequences seq_off (S + 1 row offsets, a HOST int64 tensor),
    log_trans (K x K) and log_init (K): abcd_chain_posterior.  want is a sum of
    CHAIN_EVIDENCE, CHAIN_GAMMA, CHAIN_PATH and CHAIN_COUNTS; the outputs of a
    group that is not asked for are empty tensors."""
    for t in (score, log_trans, log_init):
        N.require_gpu(t)
    want = int(want)
    if score.dim() != 2 or score.shape[1] < 1:
        raise ValueError(f"chain_posterior: score must be N x K, got {tuple(score.shape)}")
    n, K = (int(v) for v in score.shape)
    if tuple(log_trans.shape) != (K, K) or log_init.numel() != K:
        raise ValueError(f"chain_posterior: log_trans must be {(K, K)} and log_init hold {K} entries")
    if want < 0 or want > CHAIN_ALL:
        raise ValueError(f"chain_posterior: want must lie in 0 .. {CHAIN_ALL}")
    so = seq_off
    if so.dtype != torch.int64 or so.device.type != "cpu":
        so = so.to("cpu", torch.int64)
    so = so.contiguous()
    S = int(so.numel()) - 1
    if S < 0:
        raise ValueError("chain_posterior: seq_off must hold S + 1 offsets")
    dev = score.device
    (sc, lds), (lt, ldt) = _rows(score.float()), _rows(log_trans.float())
    li = log_init.float().contiguous()
    L_ = N.lib()
    nbytes = L_.abcd_chain_workspace_bytes(n, S, K, want)
    if nbytes == 0:
        raise N.HipError("chain_posterior: unsupported shape (K > 1024 or N * K >= 2^31)")
    ws = N.workspace(nbytes, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    ev = torch.empty(S if want & CHAIN_EVIDENCE else 0, **f64)
    gamma = torch.empty(n if want & CHAIN_GAMMA else 0, K, device=dev)
    path = torch.empty(n if want & CHAIN_PATH else 0, dtype=torch.int32, device=dev)
    ps = torch.zeros(S if want & CHAIN_PATH else 0, **f64)  # a zero-length sequence's entry is not written
    tc = torch.empty((K, K) if want & CHAIN_COUNTS else (0, K), **f64)
    ic = torch.empty(K if want & CHAIN_COUNTS else 0, **f64)

    def p(t, bit):
        return N.ptr(t) if want & bit else None
    N.check(L_.abcd_chain_posterior(N.ptr(sc), lds, n, K, so.data_ptr(), S, N.ptr(lt), ldt, N.ptr(li),
                                    p(ev, CHAIN_EVIDENCE), p(gamma, CHAIN_GAMMA), K, p(path, CHAIN_PATH),
                                    p(ps, CHAIN_PATH), p(tc, CHAIN_COUNTS), p(ic, CHAIN_COUNTS), N.ptr(ws),
                                    ws.numel(), N.stream()), "chain posterior")
    return [ev, gamma, path, ps, tc, ic]


@chain_posterior.register_fake
def _chain_posterior_fake(score, seq_off, log_trans, log_init, want):
    n, K = score.shape
    S = int(seq_off.numel()) - 1
    want = int(want)
    e = score.new_empty
    return [e(S if want & CHAIN_EVIDENCE else 0, dtype=torch.float64),
            e(n if want & CHAIN_GAMMA else 0, K, dtype=torch.float32),
            e(n if want & CHAIN_PATH else 0, dtype=torch.int32),
            e(S if want & CHAIN_PATH else 0, dtype=torch.float64),
            e((K, K) if want & CHAIN_COUNTS else (0, K), dtype=torch.float64),
            e(K if want & CHAIN_COUNTS else 0, dtype=torch.float64)]


_forward_only(chain_posterior, "chain_posterior")


# ----------------------------------------------------------------------------
# segmentation: span scores of an uncut recording and the semi-Markov programme (forward-only)
# ----------------------------------------------------------------------------
_TABLE_LIMIT = "D > 16383, (N + 1) * D >= 2^31 or the table's index limit (N + 1) * D * K >= 2^31"


def _span_pass_args(name, frames, proto_mu, proto_lv, proto_offset_logits, log_weight, P, D):
    """The argument checks span_scores, span_evidence and span_table share -> the C call's inputs."""
    for t in (frames, proto_mu, proto_lv, proto_offset_logits):
        N.require_gpu(t)
    P, D = int(P), int(D)
    if frames.dim() != 2 or frames.shape[1] < 1:
        raise ValueError(f"{name}: frames must be N x F, got {tuple(frames.shape)}")
    n, F = (int(v) for v in frames.shape)
    if P < 1 or D < 1:
        raise ValueError(f"{name}: P and D must be at least 1")
    (x, ldx), (mu, ldm), (lv, ldl) = _rows(frames.float()), _rows(proto_mu.float()), _rows(proto_lv.float())
    ol = proto_offset_logits.float().contiguous()
    rows = int(ol.numel())
    if rows % P or rows // P < D:
        raise ValueError(f"{name}: the prototype rectangle must hold T_proto * {P} rows with T_proto >= {D}, "
                         f"got {rows}")
    if not (tuple(mu.shape) == tuple(lv.shape) == (rows, F)):
        raise ValueError(f"{name}: proto_mu and proto_lv must be {(rows, F)}")
    lw = None
    if log_weight is not None:
        N.require_gpu(log_weight)
        if log_weight.numel() != P:
            raise ValueError(f"{name}: log_weight must hold {P} entries, got {log_weight.numel()}")
        lw = log_weight.float().contiguous()
    return n, F, P, D, x, ldx, mu, ldm, lv, ldl, ol, rows // P, lw


def _best_tables(like, n, D, want_best):
    """span_scores' two tables (N + 1 x D, fp64 and int32) on ``like``'s device, 0 x 0 unless wanted."""
    shape = (n + 1, D) if want_best else (0, 0)
    return like.new_empty(shape, dtype=torch.float64), like.new_empty(shape, dtype=torch.int32)


def _gap_arg(name, gap, n):
    """The N per-frame gap scores as the C call takes them (fp32, contiguous), or None."""
    if gap is None:
        return None
    N.require_gpu(gap)
    if gap.numel() != n:
        raise ValueError(f"{name}: gap must hold {n} entries, got {gap.numel()}")
    return gap.float().contiguous()


def _segment_lists(cap, dev, with_link):
    """[path_score, n_segments (0-d), onset, length, category (int32), score (, link) (fp64)], the lists max(cap,
    1) zeros each, in the C call's order: the operators return the lists' first cap entries."""
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    return ([torch.empty((), **f64), torch.empty((), **i32)] + [torch.zeros(max(cap, 1), **i32) for _ in range(3)] +
            [torch.zeros(max(cap, 1), **f64) for _ in range(2 if with_link else 1)])


def _chain_args(name, table, d_min, log_trans, log_init):
    """The argument checks span_chain_viterbi and span_chain_posterior share -> n, D, K, d_min and the C call's
    log_trans with its row stride and log_init."""
    for t in (table, log_trans, log_init):
        N.require_gpu(t)
    if table.dim() != 3 or min(table.shape) < 1:
        raise ValueError(f"{name}: table must be N + 1 x D x K, got {tuple(table.shape)}")
    n, D, K = int(table.shape[0]) - 1, int(table.shape[1]), int(table.shape[2])
    d_min = int(d_min)
    if d_min < 1 or d_min > D:
        raise ValueError(f"{name}: d_min must lie in 1 .. {D}, got {d_min}")
    if tuple(log_trans.shape) != (K, K) or log_init.numel() != K:
        raise ValueError(f"{name}: log_trans must be {K} x {K} and log_init hold {K} entries, got "
                         f"{tuple(log_trans.shape)} and {tuple(log_init.shape)}")
    if K > 1024:
        raise ValueError(f"{name}: at most 1024 categories, got {K}")
    lt, ldt = _rows(log_trans.float())
    return n, D, K, d_min, lt, ldt, log_init.float().contiguous()


@torch.library.custom_op("abcd::span_scores", mutates_args=())
def span_scores(frames: Tensor, proto_mu: Tensor, proto_lv: Tensor, proto_offset_logits: Tensor,
                log_weight: Optional[Tensor], P: int, D: int) -> List[Tensor]:
    """-> [span_score (N + 1 x D, fp64), span_cat (N + 1 x D, int32)], end-major:
    entry [e, d - 1] is the best prototype's log-likelihood of frames e - d ..
    e - 1 (N x F, row-strided views pass without a copy) being one segment that
    ends after d frames, and that prototype (abcd_span_scores).  The prototypes
    are the time-major rectangle pairwise_nll takes, T_proto >= D; entries with
    d > e, and spans with every prototype excluded, hold -inf / -1."""
    n, F, P, D, x, ldx, mu, ldm, lv, ldl, ol, T_proto, lw = _span_pass_args(
        "span_scores", frames, proto_mu, proto_lv, proto_offset_logits, log_weight, P, D)
    L_ = N.lib()
    nbytes = L_.abcd_span_scores_workspace_bytes(n, D, P)
    if nbytes == 0:
        raise N.HipError("span_scores: unsupported shape (D > 16383 or (N + 1) * D >= 2^31)")
    ws = N.workspace(nbytes, frames.device)
    score, cat = _best_tables(frames, n, D, True)
    N.check(L_.abcd_span_scores(N.ptr(x), ldx, n, F, P, D, T_proto, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(ol),
                                     N.ptr(lw), N.ptr(score), N.ptr(cat), D, N.ptr(ws), ws.numel(), N.stream()),
            "span scores")
    return [score, cat]


@span_scores.register_fake
def _(frames, proto_mu, proto_lv, proto_offset_logits, log_weight, P, D):
    return list(_best_tables(frames, frames.shape[0], int(D), True))


_forward_only(span_scores, "span_scores")


@torch.library.custom_op("abcd::span_viterbi", mutates_args=())
def span_viterbi(span_score: Tensor, span_cat: Tensor, d_min: int, gap: Optional[Tensor], seg_bonus: float,
                 want_v: bool) -> List[Tensor]:
    """-> [path_score (0-d, fp64), n_segments (0-d, int32), onset, length,
    category (N // d_min each, int32), score (N // d_min, fp64), V (N + 1 fp64,
    or empty)]: the best cover of the N frames by non-overlapping segments of
    d_min .. D frames and gap frames under span_scores' table (N + 1 x D,
    row-strided views pass without a copy), abcd_span_viterbi.  Only the first
    n_segments entries of the segment lists are written."""
    N.require_gpu(span_score)
    N.require_gpu(span_cat)
    if span_score.dim() != 2 or span_score.shape[0] < 1 or span_score.shape[1] < 1 or \
            tuple(span_cat.shape) != tuple(span_score.shape):
        raise ValueError(f"span_viterbi: span_score and span_cat must both be N + 1 x D, got "
                         f"{tuple(span_score.shape)} and {tuple(span_cat.shape)}")
    n, D = int(span_score.shape[0]) - 1, int(span_score.shape[1])
    d_min = int(d_min)
    if d_min < 1 or d_min > D:
        raise ValueError(f"span_viterbi: d_min must lie in 1 .. {D}, got {d_min}")
    dev = span_score.device
    ss, ld = _rows(span_score.double())
    sc, ldc = _rows(span_cat.to(torch.int32))
    if ldc != ld:  # one row stride serves both
        ss, sc, ld = ss.contiguous(), sc.contiguous(), D
    g = _gap_arg("span_viterbi", gap, n)
    L_ = N.lib()
    nbytes = L_.abcd_span_viterbi_workspace_bytes(n, D)
    if nbytes == 0:
        raise N.HipError("span_viterbi: unsupported shape (D > 16383 or (N + 1) * D >= 2^31)")
    ws = N.workspace(nbytes, dev)
    cap = n // d_min
    outs = _segment_lists(cap, dev, False)
    V = torch.empty(n + 1 if want_v else 0, dtype=torch.float64, device=dev)
    N.check(L_.abcd_span_viterbi(N.ptr(ss), N.ptr(sc), ld, n, D, d_min, N.ptr(g), float(seg_bonus),
                                 *(N.ptr(t) for t in outs), N.ptr(V) if want_v else None, N.ptr(ws), ws.numel(),
                                 N.stream()), "span viterbi")
    return outs[:2] + [t[:cap] for t in outs[2:]] + [V]


@span_viterbi.register_fake
def _(span_score, span_cat, d_min, gap, seg_bonus, want_v):
    n = span_score.shape[0] - 1
    cap = n // int(d_min)
    e = span_score.new_empty
    return [e((), dtype=torch.float64), e((), dtype=torch.int32), e(cap, dtype=torch.int32),
            e(cap, dtype=torch.int32), e(cap, dtype=torch.int32), e(cap, dtype=torch.float64),
            e(n + 1 if want_v else 0, dtype=torch.float64)]


_forward_only(span_viterbi, "span_viterbi")


@torch.library.custom_op("abcd::span_evidence", mutates_args=())
def span_evidence(frames: Tensor, proto_mu: Tensor, proto_lv: Tensor, proto_offset_logits: Tensor,
                  log_weight: Optional[Tensor], P: int, D: int, want_best: bool) -> List[Tensor]:
    """-> [span_lse (N + 1 x D, fp64), span_score, span_cat]: span_scores' pass
    with the prototypes summed, entry [e, d - 1] the log of the sum over the
    admissible prototypes of exp(log_weight[p] - em - off) for frames e - d ..
    e - 1 (abcd_span_evidence).  With want_best the same pass also gives
    span_scores' two tables, bit for bit; without it they are 0 x 0."""
    n, F, P, D, x, ldx, mu, ldm, lv, ldl, ol, T_proto, lw = _span_pass_args(
        "span_evidence", frames, proto_mu, proto_lv, proto_offset_logits, log_weight, P, D)
    L_ = N.lib()
    nbytes = L_.abcd_span_evidence_workspace_bytes(n, D, P)
    if nbytes == 0:
        raise N.HipError("span_evidence: unsupported shape (D > 16383 or (N + 1) * D >= 2^31)")
    ws = N.workspace(nbytes, frames.device)
    lse = torch.empty(n + 1, D, dtype=torch.float64, device=frames.device)
    score, cat = _best_tables(frames, n, D, want_best)
    N.check(L_.abcd_span_evidence(N.ptr(x), ldx, n, F, P, D, T_proto, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(ol),
                                       N.ptr(lw), N.ptr(lse), N.ptr(score) if want_best else None,
                                       N.ptr(cat) if want_best else None, D, N.ptr(ws), ws.numel(), N.stream()),
            "span evidence")
    return [lse, score, cat]


@span_evidence.register_fake
def _(frames, proto_mu, proto_lv, proto_offset_logits, log_weight, P, D, want_best):
    n = frames.shape[0]
    return [frames.new_empty(n + 1, int(D), dtype=torch.float64), *_best_tables(frames, n, int(D), want_best)]


_forward_only(span_evidence, "span_evidence")


@torch.library.custom_op("abcd::span_posterior", mutates_args=())
def span_posterior(span: Tensor, d_min: int, gap: Optional[Tensor], seg_bonus: float,
                   want_table: bool) -> List[Tensor]:
    """-> [log_z (0-d, fp64), lattice (4 x (N + 1): alpha, alpha_seg, beta,
    beta_seg), post (3 x (N + 1): onset, end, gap posteriors), span_post (N + 1
    x D, or 0 x 0)]: the semi-Markov forward-backward over span_scores' or
    span_evidence's table (N + 1 x D; row-strided views pass without a copy)
    under span_viterbi's d_min, gap and seg_bonus, abcd_span_posterior.  An
    unreachable end gives log_z = -inf and zero posteriors."""
    N.require_gpu(span)
    if span.dim() != 2 or span.shape[0] < 1 or span.shape[1] < 1:
        raise ValueError(f"span_posterior: span must be N + 1 x D, got {tuple(span.shape)}")
    n, D = int(span.shape[0]) - 1, int(span.shape[1])
    d_min = int(d_min)
    if d_min < 1 or d_min > D:
        raise ValueError(f"span_posterior: d_min must lie in 1 .. {D}, got {d_min}")
    dev = span.device
    ss, ld = _rows(span.double())
    g = _gap_arg("span_posterior", gap, n)
    L_ = N.lib()
    nbytes = L_.abcd_span_posterior_workspace_bytes(n, D)
    if nbytes == 0:
        raise N.HipError("span_posterior: unsupported shape (D > 16383 or (N + 1) * D >= 2^31)")
    ws = N.workspace(nbytes, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    log_z = torch.empty((), **f64)
    lattice, post = torch.empty(4, n + 1, **f64), torch.empty(3, n + 1, **f64)
    table = torch.empty((n + 1, D) if want_table else (0, 0), **f64)
    N.check(L_.abcd_span_posterior(N.ptr(ss), ld, n, D, d_min, N.ptr(g), float(seg_bonus), N.ptr(log_z),
                                   N.ptr(lattice), N.ptr(post), N.ptr(table) if want_table else None, D, N.ptr(ws),
                                   ws.numel(), N.stream()), "span posterior")
    return [log_z, lattice, post, table]


@span_posterior.register_fake
def _(span, d_min, gap, seg_bonus, want_table):
    n = span.shape[0] - 1
    e = span.new_empty
    return [e((), dtype=torch.float64), e((4, n + 1), dtype=torch.float64), e((3, n + 1), dtype=torch.float64),
            e((n + 1, span.shape[1]) if want_table else (0, 0), dtype=torch.float64)]


_forward_only(span_posterior, "span_posterior")


@torch.library.custom_op("abcd::span_table", mutates_args=())
def span_table(frames: Tensor, proto_mu: Tensor, proto_lv: Tensor, proto_offset_logits: Tensor,
               log_weight: Optional[Tensor], P: int, D: int, want_best: bool) -> List[Tensor]:
    """-> [table (N + 1 x D x P, fp64), span_score, span_cat]: span_scores' pass
    keeping every prototype, table[e, d - 1, p] = log_weight[p] - em - off of
    frames e - d .. e - 1 as one segment of prototype p that ends after d
    frames (abcd_span_table); excluded prototypes and entries with d > e hold
    -inf.  With want_best the same pass also gives span_scores' two tables, bit
    for bit; without it they are 0 x 0."""
    n, F, P, D, x, ldx, mu, ldm, lv, ldl, ol, T_proto, lw = _span_pass_args(
        "span_table", frames, proto_mu, proto_lv, proto_offset_logits, log_weight, P, D)
    L_ = N.lib()
    nbytes = L_.abcd_span_table_workspace_bytes(n, D, P, P)
    if nbytes == 0:
        raise N.HipError(f"span_table: unsupported shape ({_TABLE_LIMIT}); N = {n}, D = {D}, K = {P}")
    ws = N.workspace(nbytes, frames.device)
    table = torch.empty(n + 1, D, P, dtype=torch.float64, device=frames.device)
    score, cat = _best_tables(frames, n, D, want_best)
    N.check(L_.abcd_span_table(N.ptr(x), ldx, n, F, P, D, T_proto, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(ol),
                                    N.ptr(lw), N.ptr(table), P, N.ptr(score) if want_best else None,
                                    N.ptr(cat) if want_best else None, D, N.ptr(ws), ws.numel(), N.stream()),
            "span table")
    return [table, score, cat]


@span_table.register_fake
def _(frames, proto_mu, proto_lv, proto_offset_logits, log_weight, P, D, want_best):
    n = frames.shape[0]
    return [frames.new_empty(n + 1, int(D), int(P), dtype=torch.float64), *_best_tables(frames, n, int(D), want_best)]


_forward_only(span_table, "span_table")


@torch.library.custom_op("abcd::span_chain_viterbi", mutates_args=())
def span_chain_viterbi(table: Tensor, d_min: int, gap: Optional[Tensor], seg_bonus: float, log_trans: Tensor,
                       log_init: Tensor, want_w: bool) -> List[Tensor]:
    """-> [path_score (0-d, fp64), n_segments (0-d, int32), onset, length,
    category (N // d_min each, int32), score, link (N // d_min, fp64), W ((N +
    1) x K fp64, or empty)]: the best cover of the N frames by segments of
    d_min .. D frames and gap frames under span_table's table (N + 1 x D x K)
    with the transition log_trans[k', k] (K x K, row-strided views pass without
    a copy) paid between consecutive segments and log_init[k] on the first
    (abcd_span_chain_viterbi).  link is that term per segment.  Only the first
    n_segments entries of the segment lists are written."""
    n, D, K, d_min, lt, ldt, li = _chain_args("span_chain_viterbi", table, d_min, log_trans, log_init)
    dev = table.device
    tb = table.double().contiguous()
    g = _gap_arg("span_chain_viterbi", gap, n)
    L_ = N.lib()
    nbytes = L_.abcd_span_chain_workspace_bytes(n, D, K)
    if nbytes == 0:
        raise N.HipError(f"span_chain_viterbi: unsupported shape ({_TABLE_LIMIT}); N = {n}, D = {D}, K = {K}")
    ws = N.workspace(nbytes, dev)
    cap = n // d_min
    outs = _segment_lists(cap, dev, True)
    W = torch.empty((n + 1, K) if want_w else (0, K), dtype=torch.float64, device=dev)
    N.check(L_.abcd_span_chain_viterbi(N.ptr(tb), K, n, D, K, d_min, N.ptr(g), float(seg_bonus), N.ptr(lt), ldt,
                                       N.ptr(li), *(N.ptr(t) for t in outs), N.ptr(W) if want_w else None, N.ptr(ws),
                                       ws.numel(), N.stream()), "span chain viterbi")
    return outs[:2] + [t[:cap] for t in outs[2:]] + [W]


@span_chain_viterbi.register_fake
def _(table, d_min, gap, seg_bonus, log_trans, log_init, want_w):
    n, K = table.shape[0] - 1, table.shape[2]
    cap = n // int(d_min)
    e = table.new_empty
    return [e((), dtype=torch.float64), e((), dtype=torch.int32), e(cap, dtype=torch.int32),
            e(cap, dtype=torch.int32), e(cap, dtype=torch.int32), e(cap, dtype=torch.float64),
            e(cap, dtype=torch.float64), e((n + 1, K) if want_w else (0, K), dtype=torch.float64)]


_forward_only(span_chain_viterbi, "span_chain_viterbi")


def span_chain_window_state(n, D, K, device):
    """The state tensor ``span_chain_viterbi_window`` carries a recording of
    ``n`` frames in (uint8; abcd_span_chain_window_workspace_bytes: the lattice,
    the back-pointers, the chosen entries and the carry block, 24 (n + 1) K
    bytes and a little).  Its contents mean nothing outside the operator."""
    nbytes = N.lib().abcd_span_chain_window_workspace_bytes(int(n), int(D), int(K))
    if nbytes == 0:
        raise N.HipError(f"span_chain_viterbi_window: unsupported shape (D > 16383, (N + 1) * D >= 2^31 or K > 1024); "
                         f"N = {n}, D = {D}, K = {K}")
    return N.workspace(nbytes, device)


@torch.library.custom_op("abcd::span_chain_viterbi_window", mutates_args=("state", "W"))
def span_chain_viterbi_window(table: Tensor, row0: int, n0: int, n1: int, n: int, d_min: int, gap: Optional[Tensor],
                              seg_bonus: float, log_trans: Tensor, log_init: Tensor, state: Tensor,
                              W: Optional[Tensor]) -> List[Tensor]:
    """Steps n0 .. n1 of span_chain_viterbi's programme over a recording of n
    frames on a WINDOW of the table (rows x D x K, its row 0 the absolute end
    row0 <= max(0, n0 - D), rows > n1 - row0), the programme being carried from
    call to call in ``state`` (span_chain_window_state; mutated) and, when
    given, rows n0 .. n1 of W ((n + 1) x K fp64; mutated) being written
    (abcd_span_chain_viterbi_window).  The calls of a recording run in order on
    one stream: n0 = 1 first, then every n0 the previous n1 + 1.  -> span_chain_
    viterbi's [path_score, n_segments, onset, length, category, score, link],
    written by the call with n1 = n; before that, and after a call out of
    order, path_score is NaN and n_segments -1.  gap holds the n scores of the
    whole recording."""
    rows, D, K, d_min, lt, ldt, li = _chain_args("span_chain_viterbi_window", table, d_min, log_trans, log_init)
    rows += 1
    row0, n0, n1, n = int(row0), int(n0), int(n1), int(n)
    if not 1 <= n0 <= n1 <= n:
        raise ValueError(f"span_chain_viterbi_window: 1 <= n0 <= n1 <= N, got {n0}, {n1} and N = {n}")
    if not (0 <= row0 <= max(0, n0 - D) and n1 - row0 < rows):
        raise ValueError(f"span_chain_viterbi_window: the window must start at 0 <= row0 <= max(0, n0 - D) and hold "
                         f"end n1; got row0 = {row0}, {rows} rows, n0 = {n0}, n1 = {n1}, D = {D}")
    dev = table.device
    tb = table.double().contiguous()
    g = _gap_arg("span_chain_viterbi_window", gap, n)
    L_ = N.lib()
    nbytes = L_.abcd_span_chain_window_workspace_bytes(n, D, K)
    N.require_gpu(state)
    if nbytes == 0 or state.dtype != torch.uint8 or not state.is_contiguous() or state.numel() < nbytes:
        raise ValueError(f"span_chain_viterbi_window: state must be span_chain_window_state({n}, {D}, {K})")
    if W is not None:
        N.require_gpu(W)
        if tuple(W.shape) != (n + 1, K) or W.dtype != torch.float64 or not W.is_contiguous():
            raise ValueError(f"span_chain_viterbi_window: W must be {(n + 1, K)} contiguous float64")
    cap = n // d_min
    outs = _segment_lists(cap, dev, True)
    outs[0].fill_(float("nan"))
    outs[1].fill_(-1)
    N.check(L_.abcd_span_chain_viterbi_window(N.ptr(tb), K, row0, rows, n0, n1, n, D, K, d_min, N.ptr(g),
                                              float(seg_bonus), N.ptr(lt), ldt, N.ptr(li), *(N.ptr(t) for t in outs),
                                              N.ptr(W), N.ptr(state), state.numel(), N.stream()),
            "span chain viterbi window")
    return outs[:2] + [t[:cap] for t in outs[2:]]


@span_chain_viterbi_window.register_fake
def _(table, row0, n0, n1, n, d_min, gap, seg_bonus, log_trans, log_init, state, W):
    cap = int(n) // int(d_min)
    e = table.new_empty
    return [e((), dtype=torch.float64), e((), dtype=torch.int32), e(cap, dtype=torch.int32),
            e(cap, dtype=torch.int32), e(cap, dtype=torch.int32), e(cap, dtype=torch.float64),
            e(cap, dtype=torch.float64)]


# torch.library takes no autograd formula for an operator that mutates an argument, so _forward_only does not apply:
# torch's own fallback makes backward through the outputs raise ("not implemented"), and every caller runs under
# torch.no_grad().


@torch.library.custom_op("abcd::span_chain_posterior", mutates_args=())
def span_chain_posterior(table: Tensor, d_min: int, gap: Optional[Tensor], seg_bonus: float, scale: float,
                         log_trans: Tensor, log_init: Tensor, want_counts: bool, want_table: bool) -> List[Tensor]:
    """-> [log_z (0-d, fp64), lattice (5 x (N + 1) x K: aU, aV, aW, bU, bW),
    lattice_g (2 x (N + 1): G, bG), post_k (2 x (N + 1) x K: onset, end),
    gap_post (N + 1), trans_counts (K x K), init_counts (K), span_post ((N + 1)
    x D)], fp64 each: the semi-Markov forward-backward over (frame, last
    category) on span_table's table under span_chain_viterbi's d_min, gap,
    seg_bonus, log_trans and log_init, every term multiplied by ``scale`` (1 /
    temperature) in fp64 (abcd_span_chain_posterior).  The counts and
    span_post are empty tensors unless asked for.  An uncoverable recording
    gives log_z = -inf and zeros."""
    scale = float(scale)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"span_chain_posterior: scale must be positive and finite, got {scale}")
    n, D, K, d_min, lt, ldt, li = _chain_args("span_chain_posterior", table, d_min, log_trans, log_init)
    L_ = N.lib()
    nbytes = L_.abcd_span_chain_posterior_workspace_bytes(n, D, K)
    if nbytes == 0:
        raise N.HipError(f"span_chain_posterior: unsupported shape ({_TABLE_LIMIT}); N = {n}, D = {D}, K = {K}")
    dev = table.device
    tb = table.double().contiguous()
    g = _gap_arg("span_chain_posterior", gap, n)
    ws = N.workspace(nbytes, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    log_z = torch.empty((), **f64)
    lattice, lattice_g = torch.empty(5, n + 1, K, **f64), torch.empty(2, n + 1, **f64)
    post_k, gap_post = torch.empty(2, n + 1, K, **f64), torch.empty(n + 1, **f64)
    tc = torch.empty((K, K) if want_counts else (0, 0), **f64)
    ic = torch.empty(K if want_counts else 0, **f64)
    span = torch.empty((n + 1, D) if want_table else (0, 0), **f64)
    N.check(L_.abcd_span_chain_posterior(N.ptr(tb), K, n, D, K, d_min, N.ptr(g), float(seg_bonus), scale, N.ptr(lt),
                                         ldt, N.ptr(li), N.ptr(log_z), N.ptr(lattice), N.ptr(lattice_g),
                                         N.ptr(post_k), N.ptr(gap_post), N.ptr(tc) if want_counts else None,
                                         N.ptr(ic) if want_counts else None, N.ptr(span) if want_table else None, D,
                                         N.ptr(ws), ws.numel(), N.stream()), "span chain posterior")
    return [log_z, lattice, lattice_g, post_k, gap_post, tc, ic, span]


@span_chain_posterior.register_fake
def _(table, d_min, gap, seg_bonus, scale, log_trans, log_init, want_counts, want_table):
    n, D, K = table.shape[0] - 1, table.shape[1], table.shape[2]

    def e(*shape):
        return table.new_empty(shape, dtype=torch.float64)
    return [e(), e(5, n + 1, K), e(2, n + 1), e(2, n + 1, K), e(n + 1), e(K, K) if want_counts else e(0, 0),
            e(K) if want_counts else e(0), e(n + 1, D) if want_table else e(0, 0)]


_forward_only(span_chain_posterior, "span_chain_posterior")


# ----------------------------------------------------------------------------
# time-warped scoring: segments aligned to prototypes (forward-only)
# ----------------------------------------------------------------------------
DEFAULT_LOG_MOVES = (math.log(0.2), math.log(0.6), math.log(0.2))   # stay, step, skip
IDENTITY_LOG_MOVES = (-math.inf, 0.0, -math.inf)                    # step only: pairwise_nll's comparison


def _log_moves_arg(name, log_moves):
    """Three log weights (stay, step, skip) as the C calls take them (a host array of doubles)."""
    lm = [float(v) for v in log_moves]
    if len(lm) != 3 or any(math.isnan(v) or v == math.inf for v in lm) or all(v == -math.inf for v in lm):
        raise ValueError(f"{name}: log_moves must be three log weights (stay, step, skip), -inf to disable a move, "
                         f"at least one enabled; got {lm}")
    return (N.c_double * 3)(*lm)


def _warp_args(name, gt, batch_sizes, gt_offset, proto_mu, proto_lv, proto_offset_logits, log_moves, band, P, F):
    """The argument checks warp_nll and warp_path share -> the C call's inputs."""
    for t in (gt, gt_offset, proto_mu, proto_lv, proto_offset_logits):
        N.require_gpu(t)
    P, F = int(P), int(F)
    if P < 1:
        raise ValueError(f"{name}: P must be at least 1")
    moves = _log_moves_arg(name, log_moves)
    gt = gt.contiguous()
    (mu, ldm), (lv, ldl) = _rows(proto_mu), _rows(proto_lv)
    ol = proto_offset_logits.contiguous()
    gt_offset = gt_offset.contiguous()
    pk, bs = N.packed(gt, batch_sizes, F)
    rows = mu.shape[0]
    if rows % P or rows < P:
        raise ValueError(f"{name}: the prototype rectangle must hold T_proto * {P} rows with T_proto >= 1, got {rows}")
    if not (tuple(mu.shape) == tuple(lv.shape) == (rows, F) and tuple(gt.shape) == (pk.L, F)):
        raise ValueError(f"{name}: gt must be {(pk.L, F)}, proto_mu and proto_lv {(rows, F)}")
    if not (gt_offset.numel() == pk.L and ol.numel() == rows):
        raise ValueError(f"{name}: gt_offset must hold {pk.L} entries, proto_offset_logits {rows}")
    return pk, bs, gt, gt_offset, mu, ldm, lv, ldl, ol, rows // P, moves, int(band)


@torch.library.custom_op("abcd::warp_nll", mutates_args=())
def warp_nll(gt: Tensor, batch_sizes: Tensor, gt_offset: Tensor, proto_mu: Tensor, proto_lv: Tensor,
             proto_offset_logits: Tensor, log_moves: List[float], band: int, marginal: bool, P: int,
             F: int) -> Tensor:
    """-> warp (B x P): the time-warped NLL of every segment of the packed batch
    under every prototype (the rectangle of pairwise_nll; T_proto may be shorter
    or longer than the batch).  log_moves = log weights of (stay, step, skip),
    -inf disabling a move; band < 0: no band, else |state - frame| <= band;
    marginal: -log of the sum over alignments instead of the best one.  +inf
    where no alignment exists."""
    pk, bs, gt, gt_offset, mu, ldm, lv, ldl, ol, T_proto, moves, band = _warp_args(
        "warp_nll", gt, batch_sizes, gt_offset, proto_mu, proto_lv, proto_offset_logits, log_moves, band, P, F)
    L_ = N.lib()
    nbytes = L_.abcd_warp_nll_workspace_bytes(pk.T, pk.B, int(P), T_proto)
    if nbytes == 0:
        raise N.HipError("warp_nll: unsupported shape (more than 4096 steps, more than 16383 prototype steps, "
                         "or B * P >= 2^31)")
    ws = N.workspace(nbytes, gt.device)
    out = torch.empty(pk.B, int(P), device=gt.device)
    N.check(L_.abcd_warp_nll(pk, N.ptr(gt_offset), int(P), T_proto, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(ol), moves,
                             band, int(bool(marginal)), N.ptr(out), int(P), N.ptr(ws), ws.numel(), N.stream()),
            "warp nll")
    return out


@warp_nll.register_fake
def _warp_nll_fake(gt, batch_sizes, gt_offset, proto_mu, proto_lv, proto_offset_logits, log_moves, band, marginal, P, F):
    B = int(batch_sizes[0]) if batch_sizes.numel() else 0
    return gt.new_empty(B, int(P), dtype=torch.float32)


_forward_only(warp_nll, "warp_nll")


@torch.library.custom_op("abcd::warp_path", mutates_args=())
def warp_path(gt: Tensor, batch_sizes: Tensor, gt_offset: Tensor, proto_mu: Tensor, proto_lv: Tensor,
              proto_offset_logits: Tensor, log_moves: List[float], band: int, choice: Tensor, P: int,
              F: int) -> List[Tensor]:
    """-> [state (L, int32, packed row order), path_em (B), path_off (B),
    path_move (B)]: the best alignment of every segment to prototype choice[b]
    (a choice outside 0 .. P - 1 skips the segment) and the three components of
    its cost.  state is -1, and the components +inf, for a skipped segment and
    for one no alignment reaches."""
    pk, bs, gt, gt_offset, mu, ldm, lv, ldl, ol, T_proto, moves, band = _warp_args(
        "warp_path", gt, batch_sizes, gt_offset, proto_mu, proto_lv, proto_offset_logits, log_moves, band, P, F)
    N.require_gpu(choice)
    if choice.numel() != pk.B:
        raise ValueError(f"warp_path: choice must hold {pk.B} entries, got {choice.numel()}")
    choice = choice.to(torch.int32).contiguous()
    L_ = N.lib()
    nbytes = L_.abcd_warp_path_workspace_bytes(pk.T, pk.B, T_proto)
    if nbytes == 0 or pk.B * int(P) >= 2 ** 31:
        raise N.HipError("warp_path: unsupported shape (more than 4096 steps, more than 16383 prototype steps, "
                         "or B * P >= 2^31)")
    dev = gt.device
    ws = N.workspace(nbytes, dev)
    state = torch.empty(pk.L, dtype=torch.int32, device=dev)
    pe, po, pm = (torch.empty(pk.B, device=dev) for _ in range(3))
    N.check(L_.abcd_warp_path(pk, N.ptr(gt_offset), int(P), T_proto, N.ptr(mu), ldm, N.ptr(lv), ldl, N.ptr(ol), moves,
                              band, N.ptr(choice), N.ptr(state), N.ptr(pe), N.ptr(po), N.ptr(pm), N.ptr(ws),
                              ws.numel(), N.stream()), "warp path")
    return [state, pe, po, pm]


@warp_path.register_fake
def _warp_path_fake(gt, batch_sizes, gt_offset, proto_mu, proto_lv, proto_offset_logits, log_moves, band, choice, P, F):
    B = int(batch_sizes[0]) if batch_sizes.numel() else 0
    e = gt.new_empty
    return [e(gt.shape[0], dtype=torch.int32), e(B, dtype=torch.float32), e(B, dtype=torch.float32),
            e(B, dtype=torch.float32)]


_forward_only(warp_path, "warp_path")


# ----------------------------------------------------------------------------
# time-warped segmentation: prototypes warped inside the cut (forward-only)
# ----------------------------------------------------------------------------
_WARPSEG_LIMIT = "K > 1024, T_proto > 16383, K * T_proto >= 2^24 or (N + 1) * K >= 2^31"


@torch.library.custom_op("abcd::frame_costs", mutates_args=())
def frame_costs(frames: Tensor, proto_mu: Tensor, proto_lv: Tensor, K: int, n0: int, n1: int) -> Tensor:
    """-> cost ((n1 - n0) x T_proto K, fp32): the emission NLL of frames n0 ..
    n1 - 1 (of N x F, row-strided views pass without a copy) under every row r
    = s K + k of the prototype rectangle of pairwise_nll (abcd_frame_costs).
    An entry's bits depend on its frame and its row alone, so the plane may be
    built in chunks."""
    for t in (frames, proto_mu, proto_lv):
        N.require_gpu(t)
    K, n0, n1 = int(K), int(n0), int(n1)
    if frames.dim() != 2 or frames.shape[1] < 1:
        raise ValueError(f"frame_costs: frames must be N x F, got {tuple(frames.shape)}")
    n, F = (int(v) for v in frames.shape)
    if not 0 <= n0 < n1 <= n:
        raise ValueError(f"frame_costs: 0 <= n0 < n1 <= N, got {n0}, {n1} and N = {n}")
    (x, ldx), (mu, ldm), (lv, ldl) = _rows(frames.float()), _rows(proto_mu.float()), _rows(proto_lv.float())
    rows = int(mu.shape[0]) if mu.dim() == 2 else 0
    if K < 1 or rows < K or rows % K or not (tuple(mu.shape) == tuple(lv.shape) == (rows, F)):
        raise ValueError(f"frame_costs: proto_mu and proto_lv must be T_proto * {K} x {F} with T_proto >= 1, got "
                         f"{tuple(proto_mu.shape)} and {tuple(proto_lv.shape)}")
    L_ = N.lib()
    if L_.abcd_warp_segment_workspace_bytes(n, K, rows // K) == 0 or (n1 - n0) * rows >= 2 ** 31:
        raise N.HipError(f"frame_costs: unsupported shape ({_WARPSEG_LIMIT}, or (n1 - n0) * K * T_proto >= 2^31); "
                         f"N = {n}, K = {K}, T_proto = {rows // K}")
    cost = torch.empty(n1 - n0, rows, device=frames.device)
    N.check(L_.abcd_frame_costs(N.ptr(x), ldx, n, n0, n1, F, K, rows // K, N.ptr(mu), ldm, N.ptr(lv), ldl,
                                N.ptr(cost), rows, N.stream()), "frame costs")
    return cost


@frame_costs.register_fake
def _(frames, proto_mu, proto_lv, K, n0, n1):
    return frames.new_empty(int(n1) - int(n0), proto_mu.shape[0], dtype=torch.float32)


_forward_only(frame_costs, "frame_costs")


def warp_segment_state(n, K, T, device=None):
    """The state tensor ``warp_segment_window`` carries a recording of ``n``
    frames in (uint8; abcd_warp_segment_workspace_bytes: 32 (n + 1) K + 40 K T
    bytes and a little).  In this order, with cells = (n + 1) K and S = K T: U
    and the chosen X (cells fp64 each), W's choice, the onset, the last state
    and k' (cells int32 each), sp(v) and sp(-v) (S fp64 each), the two H rows
    (2 S fp64) with their onsets (2 S int32), W (K fp64), G, the next frame."""
    nbytes = N.lib().abcd_warp_segment_workspace_bytes(int(n), int(K), int(T))
    if nbytes == 0:
        raise N.HipError(f"warp_segment_window: unsupported shape ({_WARPSEG_LIMIT}); N = {n}, K = {K}, T_proto = {T}")
    return N.workspace(nbytes, device if device is not None else torch.device("cuda"))


@torch.library.custom_op("abcd::warp_segment_window", mutates_args=("state", "W"))
def warp_segment_window(cost: Tensor, n0: int, n1: int, n: int, K: int, proto_offset_logits: Tensor,
                        log_moves: List[float], log_enter: Optional[Tensor], gap: Optional[Tensor],
                        seg_bonus: float, log_trans: Tensor, log_init: Tensor, s_min: int, state: Tensor,
                        W: Optional[Tensor]) -> List[Tensor]:
    """Frames n0 .. n1 - 1 of the time-warped segmentation programme over a
    recording of n frames on frame_costs' plane of those frames (row 0 is frame
    n0; more rows may follow), the programme being carried from call to call in
    ``state`` (warp_segment_state; mutated) and, when given, rows n0 + 1 .. n1 of
    W ((n + 1) x K fp64; mutated; row 0 too at n0 = 0) being written
    (abcd_warp_segment_window).  The calls of a recording run in order on one
    stream: n0 = 0 first, then every n0 the previous n1.  -> [path_score (0-d,
    fp64), n_segments (0-d, int32), onset, length, category, last_state (n
    each, int32), enter, exit, link (n each, fp64)], written by the call with
    n1 = n; before that, and after a call out of order, path_score is NaN and
    n_segments -1.  gap holds the n scores of the whole recording."""
    for t in (cost, proto_offset_logits, log_trans, log_init):
        N.require_gpu(t)
    n0, n1, n, K, s_min = int(n0), int(n1), int(n), int(K), int(s_min)
    moves = _log_moves_arg("warp_segment_window", log_moves)
    ol = proto_offset_logits.float().contiguous()
    S = int(ol.numel())
    if K < 1 or S < K or S % K:
        raise ValueError(f"warp_segment_window: proto_offset_logits must hold T_proto * {K} entries, got {S}")
    T = S // K
    if K > 1024:
        raise ValueError(f"warp_segment_window: at most 1024 categories, got {K}")
    if not 0 <= n0 < n1 <= n:
        raise ValueError(f"warp_segment_window: 0 <= n0 < n1 <= N, got {n0}, {n1} and N = {n}")
    if cost.dim() != 2 or cost.shape[0] < n1 - n0 or cost.shape[1] != S:
        raise ValueError(f"warp_segment_window: cost must hold at least {n1 - n0} rows of {S}, got {tuple(cost.shape)}")
    if not 0 <= s_min < T:
        raise ValueError(f"warp_segment_window: s_min must lie in 0 .. {T - 1}, got {s_min}")
    if tuple(log_trans.shape) != (K, K) or log_init.numel() != K:
        raise ValueError(f"warp_segment_window: log_trans must be {K} x {K} and log_init hold {K} entries, got "
                         f"{tuple(log_trans.shape)} and {tuple(log_init.shape)}")
    le = None
    if log_enter is not None:
        N.require_gpu(log_enter)
        if log_enter.numel() != K:
            raise ValueError(f"warp_segment_window: log_enter must hold {K} entries, got {log_enter.numel()}")
        le = log_enter.float().contiguous()
    c, ldc = _rows(cost.float())
    lt, ldt = _rows(log_trans.float())
    li = log_init.float().contiguous()
    g = _gap_arg("warp_segment_window", gap, n)
    L_ = N.lib()
    nbytes = L_.abcd_warp_segment_workspace_bytes(n, K, T)
    N.require_gpu(state)
    if nbytes == 0 or state.dtype != torch.uint8 or not state.is_contiguous() or state.numel() < nbytes:
        raise ValueError(f"warp_segment_window: state must be warp_segment_state({n}, {K}, {T})")
    if W is not None:
        N.require_gpu(W)
        if tuple(W.shape) != (n + 1, K) or W.dtype != torch.float64 or not W.is_contiguous():
            raise ValueError(f"warp_segment_window: W must be {(n + 1, K)} contiguous float64")
    dev = cost.device
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    outs = ([torch.full((), float("nan"), **f64), torch.full((), -1, **i32)] +
            [torch.zeros(n, **i32) for _ in range(4)] + [torch.zeros(n, **f64) for _ in range(3)])
    N.check(L_.abcd_warp_segment_window(N.ptr(c), ldc, n0, n1, n, K, T, N.ptr(ol), moves, N.ptr(le), N.ptr(g),
                                        float(seg_bonus), N.ptr(lt), ldt, N.ptr(li), s_min,
                                        *(N.ptr(t) for t in outs), N.ptr(W), N.ptr(state), state.numel(), N.stream()),
            "warp segment window")
    return outs


@warp_segment_window.register_fake
def _(cost, n0, n1, n, K, proto_offset_logits, log_moves, log_enter, gap, seg_bonus, log_trans, log_init, s_min,
      state, W):
    n = int(n)
    e = cost.new_empty
    return ([e((), dtype=torch.float64), e((), dtype=torch.int32)] + [e(n, dtype=torch.int32) for _ in range(4)] +
            [e(n, dtype=torch.float64) for _ in range(3)])


# ----------------------------------------------------------------------------
# posteriors under the time-warped cut (forward-only, stateful)
# ----------------------------------------------------------------------------
def _warp_posterior_words(n, K, T):
    """How many doubles of the state precede log_z (abcd_warp_posterior_workspace_bytes' layout)."""
    return 2 * (n + 1) + 5 * (n + 1) * K + 4 * K * T + K * K + 4 * K


def warp_posterior_state(n, K, T, device=None):
    """The state tensor ``warp_posterior_forward`` / ``warp_posterior_backward``
    carry a recording of ``n`` frames in (uint8;
    abcd_warp_posterior_workspace_bytes: 8 (2 (n + 1) + 5 (n + 1) K + 4 K T + K K
    + 4 K + 4) bytes and a little).  Doubles in this order: G, bG (n + 1 each),
    aU, aX, aW, bU, bW ((n + 1) K each), sp(v), sp(-v) (K T each), the two
    alternating aH / bA rows (2 K T), the count accumulators (K K, K, 3 K),
    log_z, then the next forward frame, the next backward n1 and the status of
    the last backward call (64-bit integers, zero in a new state)."""
    n, K, T = int(n), int(K), int(T)
    nbytes = N.lib().abcd_warp_posterior_workspace_bytes(n, K, T)
    if nbytes == 0:
        raise N.HipError(f"warp_posterior: unsupported shape ({_WARPSEG_LIMIT}); N = {n}, K = {K}, T_proto = {T}")
    state = N.workspace(nbytes, device if device is not None else torch.device("cuda"))
    state[8 * _warp_posterior_words(n, K, T):].zero_()
    return state


def warp_posterior_planes(state, n, K, T):
    """Views into a ``warp_posterior_state``: dict of ``cont``, ``last`` (T x K),
    ``lattice`` (5 x (n + 1) x K: aU, aX, aW, bU, bW), ``G``, ``bG`` (n + 1),
    ``log_z`` (0-d) (float64) and ``next`` (3 int64: the next forward frame, the
    next backward n1, the last backward call's status)."""
    n, K, T = int(n), int(K), int(T)
    words = _warp_posterior_words(n, K, T)
    d = state[:8 * (words + 1)].view(torch.float64)
    cells, S = (n + 1) * K, K * T
    at = 2 * (n + 1)
    lattice = d[at:at + 5 * cells].view(5, n + 1, K)
    at += 5 * cells
    return dict(G=d[:n + 1], bG=d[n + 1:2 * (n + 1)], lattice=lattice, cont=d[at:at + S].view(T, K),
                last=d[at + S:at + 2 * S].view(T, K), log_z=d[words],
                next=state[8 * (words + 1):8 * (words + 4)].view(torch.int64))


def _warp_posterior_args(name, cost, n0, n1, n, K, proto_offset_logits, log_moves, log_enter, gap, scale, log_trans,
                         log_init, s_min, state, alpha):
    """The checks the two sweeps share (the plain ones first: they need no device) -> the C calls' inputs."""
    n0, n1, n, K, s_min, scale = int(n0), int(n1), int(n), int(K), int(s_min), float(scale)
    moves = _log_moves_arg(name, log_moves)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"{name}: scale must be positive and finite, got {scale}")
    S = int(proto_offset_logits.numel())
    if K < 1 or S < K or S % K:
        raise ValueError(f"{name}: proto_offset_logits must hold T_proto * {K} entries, got {S}")
    T = S // K
    if K > 1024:
        raise ValueError(f"{name}: at most 1024 categories, got {K}")
    if not (0 <= n0 < n1 <= n or n0 == n1 == n == 0):
        raise ValueError(f"{name}: 0 <= n0 < n1 <= N, got {n0}, {n1} and N = {n}")
    if cost.dim() != 2 or cost.shape[0] < n1 - n0 or cost.shape[1] != S:
        raise ValueError(f"{name}: cost must hold at least {n1 - n0} rows of {S}, got {tuple(cost.shape)}")
    if not 0 <= s_min < T:
        raise ValueError(f"{name}: s_min must lie in 0 .. {T - 1}, got {s_min}")
    if tuple(log_trans.shape) != (K, K) or log_init.numel() != K:
        raise ValueError(f"{name}: log_trans must be {K} x {K} and log_init hold {K} entries, got "
                         f"{tuple(log_trans.shape)} and {tuple(log_init.shape)}")
    if log_enter is not None and log_enter.numel() != K:
        raise ValueError(f"{name}: log_enter must hold {K} entries, got {log_enter.numel()}")
    if gap is not None and gap.numel() != n:
        raise ValueError(f"{name}: gap must hold {n} entries, got {gap.numel()}")
    if alpha is not None and (alpha.dim() != 2 or alpha.shape[0] < n1 - n0 or alpha.shape[1] != S or
                              alpha.dtype != torch.float64 or not alpha.is_contiguous()):
        raise ValueError(f"{name}: alpha must hold at least {n1 - n0} rows of {S} contiguous float64, got "
                         f"{tuple(alpha.shape)} {alpha.dtype}")
    if state.dtype != torch.uint8 or state.dim() != 1 or not state.is_contiguous():
        raise ValueError(f"{name}: state must be warp_posterior_state({n}, {K}, {T})")
    for t in (cost, proto_offset_logits, log_trans, log_init, state, log_enter, alpha):
        if t is not None:
            N.require_gpu(t)
    nbytes = N.lib().abcd_warp_posterior_workspace_bytes(n, K, T)
    if nbytes == 0 or state.numel() < nbytes:
        raise ValueError(f"{name}: state must be warp_posterior_state({n}, {K}, {T})")
    ol = proto_offset_logits.float().contiguous()
    le = None if log_enter is None else log_enter.float().contiguous()
    c, ldc = _rows(cost.float())
    lt, ldt = _rows(log_trans.float())
    li = log_init.float().contiguous()
    g = _gap_arg(name, gap, n)
    keep = (ol, le, c, lt, li, g)
    return (N.ptr(c), ldc, n0, n1, n, K, T, N.ptr(ol), moves, N.ptr(le), N.ptr(g)), (N.ptr(lt), ldt, N.ptr(li),
                                                                                    s_min), T, S, keep


@torch.library.custom_op("abcd::warp_posterior_forward", mutates_args=("state", "alpha"))
def warp_posterior_forward(cost: Tensor, n0: int, n1: int, n: int, K: int, proto_offset_logits: Tensor,
                           log_moves: List[float], log_enter: Optional[Tensor], gap: Optional[Tensor],
                           seg_bonus: float, scale: float, log_trans: Tensor, log_init: Tensor, s_min: int,
                           state: Tensor, alpha: Optional[Tensor]) -> Tensor:
    """Frames n0 .. n1 - 1 of the forward sweep of the posteriors under the
    time-warped cut, on frame_costs' plane of those frames (row 0 is frame n0),
    the programme being carried in ``state`` (warp_posterior_state; mutated)
    and, when given, the aH rows of these frames written to ``alpha`` (at least
    n1 - n0 rows of T_proto K fp64; row 0 is frame n0; mutated)
    (abcd_warp_posterior_forward).  Calls run in order on one stream: n0 = 0
    first, then every n0 the previous n1.  -> log_z (0-d fp64): the log evidence
    from the call with n1 = n, NaN before that and after a call out of order.
    ``scale`` (1 / temperature) multiplies every term in fp64."""
    a, b, T, S, keep = _warp_posterior_args("warp_posterior_forward", cost, n0, n1, n, K, proto_offset_logits,
                                            log_moves, log_enter, gap, scale, log_trans, log_init, s_min, state, alpha)
    log_z = torch.full((), float("nan"), dtype=torch.float64, device=cost.device)
    N.check(N.lib().abcd_warp_posterior_forward(*a, float(seg_bonus), float(scale), *b, N.ptr(alpha), S, N.ptr(log_z),
                                                N.ptr(state), state.numel(), N.stream()), "warp posterior forward")
    return log_z


@warp_posterior_forward.register_fake
def _(cost, n0, n1, n, K, proto_offset_logits, log_moves, log_enter, gap, seg_bonus, scale, log_trans, log_init,
      s_min, state, alpha):
    return cost.new_empty((), dtype=torch.float64)


@torch.library.custom_op("abcd::warp_posterior_backward", mutates_args=("state",))
def warp_posterior_backward(cost: Tensor, n0: int, n1: int, n: int, K: int, proto_offset_logits: Tensor,
                            log_moves: List[float], log_enter: Optional[Tensor], gap: Optional[Tensor],
                            seg_bonus: float, scale: float, log_trans: Tensor, log_init: Tensor, s_min: int,
                            state: Tensor, alpha: Optional[Tensor], want_counts: bool,
                            want_moves: bool) -> List[Tensor]:
    """Frames n1 - 1 .. n0 of the backward sweep, after the forward sweep has
    finished: the first call has n1 = n, every next call's n1 is the previous
    n0; ``cost`` is the plane of THESE frames (row 0 is frame n0) and ``alpha``
    (needed by ``want_moves``) the rows ``warp_posterior_forward`` wrote for
    them (abcd_warp_posterior_backward).  A call out of order raises
    RuntimeError and leaves the carried programme usable.  -> [post_k (2 x (n +
    1) x K: onset, end), gap_post (n + 1), trans_counts (K x K), init_counts (K),
    move_counts (K x 3: stay, step, skip)], fp64, written by the call with n0 =
    0 (NaN before that); the counts are empty tensors unless asked for."""
    want_counts, want_moves = bool(want_counts), bool(want_moves)
    if want_moves and alpha is None:
        raise ValueError("warp_posterior_backward: want_moves needs alpha, the aH rows of the forward sweep")
    a, b, T, S, keep = _warp_posterior_args("warp_posterior_backward", cost, n0, n1, n, K, proto_offset_logits,
                                            log_moves, log_enter, gap, scale, log_trans, log_init, s_min, state, alpha)
    n0, n, K = int(n0), int(n), int(K)
    f64 = dict(dtype=torch.float64, device=cost.device)
    fill = 0.0 if n0 == 0 else float("nan")
    post_k, gap_post = torch.full((2, n + 1, K), fill, **f64), torch.full((n + 1,), fill, **f64)
    tc = torch.full((K, K) if want_counts else (0, 0), fill, **f64)
    ic = torch.full((K if want_counts else 0,), fill, **f64)
    mc = torch.full((K, 3) if want_moves else (0, 3), fill, **f64)
    N.check(N.lib().abcd_warp_posterior_backward(*a, float(seg_bonus), float(scale), *b, N.ptr(alpha), S,
                                                 N.ptr(post_k), N.ptr(gap_post), N.ptr(tc) if want_counts else None,
                                                 N.ptr(ic) if want_counts else None,
                                                 N.ptr(mc) if want_moves else None, N.ptr(state), state.numel(),
                                                 N.stream()), "warp posterior backward")
    if n > 0:
        words = _warp_posterior_words(n, K, T)
        if int(state[8 * (words + 3):8 * (words + 4)].view(torch.int64).item()) != 0:
            raise RuntimeError(f"warp_posterior_backward: the call for frames {n0} .. {int(n1) - 1} is out of order "
                               "(the forward sweep is not through, or n1 is not the frame the sweep has reached); "
                               "nothing was run")
    return [post_k, gap_post, tc, ic, mc]


@warp_posterior_backward.register_fake
def _(cost, n0, n1, n, K, proto_offset_logits, log_moves, log_enter, gap, seg_bonus, scale, log_trans, log_init,
      s_min, state, alpha, want_counts, want_moves):
    n, K = int(n), int(K)

    def e(*shape):
        return cost.new_empty(shape, dtype=torch.float64)
    return [e(2, n + 1, K), e(n + 1), e(K, K) if want_counts else e(0, 0), e(K) if want_counts else e(0),
            e(K, 3) if want_moves else e(0, 3)]


# ----------------------------------------------------------------------------
# log-spectra back to audio (forward-only)
# ----------------------------------------------------------------------------
@torch.library.custom_op("abcd::griffin_lim", mutates_args=())
def griffin_lim(logamp: Tensor, batch_sizes: Tensor, window: Tensor, phase0: Tensor, hop: int, eps: float,
                norm: float, n_iter: int, momentum: float, want_residual: bool) -> List[Tensor]:
    """-> [waves (B x S_max), residual (B)]: Griffin-Lim phase retrieval of the
    packed log-amplitude frames (L x F, F = n_fft / 2 + 1, n_fft = the
    window's length; row-strided views pass without a copy) from the initial
    phase phase0 (L x F radians), torch.stft semantics with center=True.  Row b
    is the segment at packed position b, hop * (T_b - 1) samples followed by
    zeros; a segment too short for the reflect padding gets a zero row and a
    NaN residual.  residual is NaN everywhere when not asked for."""
    for t in (logamp, window, phase0):
        N.require_gpu(t)
    n_fft = int(window.numel())
    F = n_fft // 2 + 1
    if logamp.dim() != 2 or logamp.shape[1] != F or tuple(phase0.shape) != tuple(logamp.shape):
        raise ValueError(f"griffin_lim: logamp and phase0 must be L x {F}, got {tuple(logamp.shape)} and "
                         f"{tuple(phase0.shape)}")
    dev = logamp.device
    (x, ld), (ph, ldp) = _rows(logamp.float()), _rows(phase0.float())
    win = window.float().contiguous()
    L_ = N.lib()
    pk, bs = N.packed(x, batch_sizes, F)
    smax = int(L_.abcd_griffin_lim_samples(pk.T, n_fft, int(hop), 1))
    nbytes = L_.abcd_griffin_lim_workspace_bytes(pk.B, pk.T, n_fft, int(hop))
    if nbytes == 0:
        raise N.HipError("griffin_lim: unsupported shape (more than 16383 steps, or an n_fft whose tables exceed the LDS)")
    ws = N.workspace(nbytes, dev)
    waves = torch.empty(pk.B, max(smax, 1), device=dev)
    residual = torch.full((pk.B,), float("nan"), device=dev)
    N.check(L_.abcd_griffin_lim(N.ptr(x), ld, bs.data_ptr(), pk.T, pk.L, pk.B, n_fft, int(hop), 1, N.ptr(win),
                                float(eps), float(norm), N.ptr(ph), ldp, int(n_iter), float(momentum), N.ptr(waves),
                                waves.shape[1], N.ptr(residual) if want_residual else None, N.ptr(ws), ws.numel(),
                                N.stream()), "griffin lim")
    return [waves[:, :smax], residual]


@griffin_lim.register_fake
def _(logamp, batch_sizes, window, phase0, hop, eps, norm, n_iter, momentum, want_residual):
    B = int(batch_sizes[0]) if batch_sizes.numel() else 0
    n_fft = int(window.numel())
    smax = max(int(hop) * (int(batch_sizes.numel()) - 1), 0)
    if smax <= n_fft - n_fft // 2:  # abcd_griffin_lim_samples: too short for the reflect padding
        smax = 0
    return [logamp.new_empty(B, smax, dtype=torch.float32), logamp.new_empty(B, dtype=torch.float32)]


_forward_only(griffin_lim, "griffin_lim")


OPS = ("encoder", "encoder_bwd", "sampler", "sampler_bwd", "sampler_sample", "sampler_sample_bwd", "sampler_kl",
       "sampler_kl_bwd", "decoder", "decoder_bwd", "linear", "linear_bwd", "segment_losses", "sampler_kl_rows",
       "pairwise_nll", "pair_posterior", "griffin_lim", "chain_posterior", "span_scores", "span_viterbi",
       "warp_nll", "warp_path", "span_evidence", "span_posterior", "span_table", "span_chain_viterbi",
       "span_chain_posterior", "frame_costs")
STATEFUL_OPS = ("span_chain_viterbi_window", "warp_segment_window", "warp_posterior_forward",
                "warp_posterior_backward")  # mutate a state argument: kept apart from the functional OPS


def registered() -> Sequence[str]:
    """Names of the abcd:: operators torch knows about."""
    return [n for n in OPS if hasattr(torch.ops.abcd, n)]
