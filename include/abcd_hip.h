/* abcd_hip.h -- C ABI of the MI355X (gfx950) ABCD-VAE training path.
 *
 * libabcd_hip.so implements the hot path of the reference trainer
 * (ABCD-VAE/learning.py:147-163: encoder -> sampler -> KL -> decoder -> loss ->
 * backward -> clip_grad_norm_ -> SGD) as hand-written HIP kernels for CDNA4.
 * The reference has no native plugin boundary: its hot path sits behind
 * PyTorch nn.Module methods.  Each entry point below replaces one of those
 * methods (cited per function); the reference-side ctypes binding a
 * maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is DEVICE memory unless marked HOST;
 *   - all floating point is IEEE fp32 (the reference trains in fp32);
 *   - the packed layout is PyTorch's PackedSequence: rows are time-major,
 *     step t owns rows [off_t, off_t + batch_sizes[t]), batch_sizes is
 *     non-increasing and lives on the HOST (as in PackedSequence);
 *   - `stream` is a hipStream_t (void* here to keep this header HIP-free);
 *     every call is asynchronous and stream-ordered, no host synchronisation;
 *   - the caller owns all memory; `ws` is a caller-allocated workspace of at
 *     least *_workspace_bytes(); the SAME workspace must be passed to the
 *     backward of a module as to its forward (it holds the activation stash);
 *   - return value: 0 on success, a hipError_t code, or ABCD_EINVAL for
 *     unsupported shapes/arguments.  Nothing throws across this ABI.
 *
 * Shape support: the kernels take hidden sizes, MLP width, codebook dim,
 * #categories, speaker embedding dim and the plain feature size in multiples
 * of 16; the frequency-bin count F is arbitrary (padded internally); encoder
 * layers <= 4.  Any other size (the reference accepts every -K, -f and
 * --*_hidden_size, learning.py:371-376) runs as the ZERO-PADDED model: each
 * size rounded up to 16, the real weights embedded at their unit / gate /
 * block positions and every padding weight 0.  Padding units then stay exactly
 * 0 through every recurrence, tanh and product, so values and gradients at the
 * real positions are the real model's; only the categorical softmax needs to
 * know the real sizes (abcd_sampler_cfg.valid_categories / valid_feature_dim).
 * The Python host (modules/padding.py) embeds the parameters and extracts the
 * gradients; INTEGRATION.md shows the index maps.
 */
#ifndef ABCD_HIP_H
#define ABCD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABCD_EINVAL 1000
#define ABCD_MAX_LAYERS 4

enum abcd_rnn_type { ABCD_LSTM = 0, ABCD_GRU = 1 };

typedef struct abcd_rnn_w { const float *w_ih, *w_hh, *b_ih, *b_hh; } abcd_rnn_w;
typedef struct abcd_rnn_g { float *w_ih, *w_hh, *b_ih, *b_hh; } abcd_rnn_g;
typedef struct abcd_mlp_w { const float *w1, *b1, *w2, *b2; } abcd_mlp_w; /* Linear->Tanh->Linear */
typedef struct abcd_mlp_g { float *w1, *b1, *w2, *b2; } abcd_mlp_g;

/* A packed batch (torch.nn.utils.rnn.PackedSequence): data is L x F. */
typedef struct abcd_packed {
  const float* data;          /* L x F, may be NULL for the decoder without ground truth */
  const int64_t* batch_sizes; /* HOST, T entries */
  int T, L, B, F;
} abcd_packed;

/* ------------------------------------------------------------------------
 * Encoder: RNN_Variational_Encoder (ABCD-VAE/modules/model.py:40-66)
 * ---------------------------------------------------------------------- */
typedef struct abcd_encoder_cfg {
  int input_size, hidden_size, rnn_type, layers, bidirectional;
} abcd_encoder_cfg;
typedef struct abcd_encoder_params { abcd_rnn_w w[ABCD_MAX_LAYERS][2]; } abcd_encoder_params;
typedef struct abcd_encoder_grads { abcd_rnn_g g[ABCD_MAX_LAYERS][2]; } abcd_encoder_grads;

/* hidden_size_total of model.py:54-58 */
int abcd_encoder_out_size(const abcd_encoder_cfg* cfg);
size_t abcd_encoder_workspace_bytes(const abcd_encoder_cfg* cfg, int T, int L, int B);
/* replaces RNN_Variational_Encoder.forward (model.py:60-66): last_hidden is
 * B x out_size laid out [h_l0f, c_l0f, h_l0b, c_l0b, h_l1f, ...] */
int abcd_encoder_forward(const abcd_encoder_cfg* cfg, const abcd_encoder_params* p, const abcd_packed* x,
                         float* last_hidden, void* ws, size_t ws_bytes, void* stream);
/* autograd backward of the above: writes (overwrites) every weight gradient */
int abcd_encoder_backward(const abcd_encoder_cfg* cfg, const abcd_encoder_params* p, const abcd_packed* x,
                          const float* d_last_hidden, const abcd_encoder_grads* g, void* ws, size_t ws_bytes,
                          void* stream);

/* The same backward with part of the weight-gradient reductions on
 * `wgrad_stream`: for a bidirectional encoder, the first layer's
 * backward-direction weight gradients are reduced on wgrad_stream (forked
 * after the BPTT) beside the forward direction's on `stream`, which then
 * waits for wgrad_stream, so on return every gradient is complete in
 * `stream` order.  wgrad_stream == NULL or == stream: identical to
 * abcd_encoder_backward. */
int abcd_encoder_backward_overlap(const abcd_encoder_cfg* cfg, const abcd_encoder_params* p, const abcd_packed* x,
                                  const float* d_last_hidden, const abcd_encoder_grads* g, void* ws, size_t ws_bytes,
                                  void* stream, void* wgrad_stream);

/* Training-mode inter-layer dropout of nn.LSTM/GRU(dropout = p) (applied by
 * ATen to the packed output of every layer but the last, model.py:53):
 * noise is a HOST array of layers - 1 DEVICE pointers, noise[l] = L x dirs*H
 * values bernoulli(1 - p) / (1 - p) drawn by the caller (in the reference's
 * RNG order for parity, or abcd_fill_dropout); noise == NULL or noise[l] ==
 * NULL: no dropout at that boundary.  The backward takes the same noise. */
int abcd_encoder_forward_dropout(const abcd_encoder_cfg* cfg, const abcd_encoder_params* p, const abcd_packed* x,
                                 const float* const* noise, float* last_hidden, void* ws, size_t ws_bytes,
                                 void* stream);
int abcd_encoder_backward_dropout(const abcd_encoder_cfg* cfg, const abcd_encoder_params* p, const abcd_packed* x,
                                  const float* const* noise, const float* d_last_hidden, const abcd_encoder_grads* g,
                                  void* ws, size_t ws_bytes, void* stream, void* wgrad_stream);
/* The weight gradients of one LSTM layer over its packed frames, every
 * direction at once: the autograd of nn.LSTM's w_ih, b_ih, b_hh, w_hh
 * (model.py:53,60-66) given the gate gradients.  For direction d < nd <= 2:
 *   w_ih[d] = dG[d]^T X,  b_ih[d] = b_hh[d] = colsum(dG[d]),  w_hh[d] = dG[d]^T Hprev[d]
 * dG[d]: K x 4H (row stride 4H, gate blocks i, f, g, o), X: K x F (row
 * stride ldx), Hprev[d]: K x H (stride H; the hidden state each frame's step
 * consumed, zero where it had no predecessor).  b_hh[d] may be NULL.  The
 * encoder backward runs this after its BPTT (layer 0); at F <= 143 with
 * roundup16(F) = 144 and H = 256 it is one gemm_wg3b launch + one slab reduction.
 * K = 0 returns 0 and writes nothing (the gradients are not zeroed). */
size_t abcd_lstm_wgrad_workspace_bytes(int nd, int F, int H, int K);
int abcd_lstm_wgrad(int nd, int F, int H, int K, const float* const* dG, const float* X, long ldx,
                    const float* const* Hprev, float* const* w_ih, float* const* b_ih, float* const* b_hh,
                    float* const* w_hh, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * ABCDSampler (model.py:538-639) and the plain Gaussian Sampler
 * (plain/modules/model.py:538-567, model.py:17-28)
 * ---------------------------------------------------------------------- */
typedef struct abcd_sampler_cfg {
  int input_size, mlp_hidden, num_categories, feature_dim;
  int plain; /* 1: plain Gaussian feature sampler (feature_dim = output_size) */
  /* A zero-padded model (every size rounded up to 16, padding weights 0; see
   * "Shape support" above): the model's own category count (the first
   * valid_categories of the num_categories logit columns are categories, the
   * rest are masked out of every softmax, KL and perplexity) and feature dim
   * (the logits scale 1 / sqrt(valid_feature_dim), model.py:589; plain: the
   * feature columns >= valid_feature_dim draw zero noise, so their samples are
   * the padding mean 0).  0: the padded size itself. */
  int valid_categories, valid_feature_dim;
} abcd_sampler_cfg;
typedef struct abcd_sampler_params {
  abcd_mlp_w mlp[2];                 /* ABCD: mlp[0] = to_code_like; plain: mlps.0 (mean), mlps.1 (log-var) */
  const float* codebook;             /* D x K  (ABCD only) */
  const float* posterior_shape_logits; /* K (ABCD only) */
  float prior_concentration;
} abcd_sampler_params;
typedef struct abcd_sampler_grads {
  abcd_mlp_g mlp[2];
  float* codebook;
  float* posterior_shape_logits;
} abcd_sampler_grads;

/* sampling modes */
enum abcd_sample_mode { ABCD_SAMPLE_SOFTMAX = 0, ABCD_SAMPLE_GUMBEL = 1 };

size_t abcd_sampler_workspace_bytes(const abcd_sampler_cfg* cfg, int B);
/* replaces ABCDSampler.forward (model.py:581-590): logits B x K.
 * plain: Sampler.forward -> params_out = [mean | log_var] (B x 2f). */
int abcd_sampler_forward(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* h, int B,
                         float* logits, void* ws, size_t ws_bytes, void* stream);
/* replaces ABCDSampler.sample (model.py:592-606) / plain Sampler.sample:
 * feats B x D.  noise: ABCD gumbel mode: B x K gumbel g = -log(Exp(1));
 * plain: B x f standard normal.  noise == NULL -> in-kernel Philox(seed, offset). */
int abcd_sampler_sample(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* logits, int B,
                        int mode, float temperature, const float* noise, uint64_t seed, uint64_t offset,
                        float* feats, void* ws, size_t ws_bytes, void* stream);
/* replaces ABCDSampler.kl_divergence (model.py:608-639) / plain kl: writes a device scalar */
int abcd_sampler_kl(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* logits, int B,
                    double entire_data_size, float* kl_out, void* ws, size_t ws_bytes, void* stream);
/* forward + sample + kl of one training step (learning.py:149-153 calls
 * feature_sampler(h), .sample(logits), .kl_divergence(logits, N) in turn):
 * logits B x K, feats B x D and the KL scalar (kl_out may be NULL), the same
 * values and backward stash as the three calls above.  ABCD: two launches --
 * the split-K h W1^T GEMM and one row-tiled sampler-head kernel (MLP tail,
 * logits, Gumbel-softmax, y C^T and the KL row terms per 16-row tile, the KL
 * scalar reduced by the last tile).  plain: the three calls in turn.
 * ppl_out (ABCD, may be NULL): ppl_out[0..1] = the cluster and batch
 * perplexities of abcd_perplexities on these logits (reduced by the same
 * last tile); ppl_out[2] is left to abcd_shape_perplexity (it reads
 * posterior_shape_logits after the SGD step, learning.py:171-178). */
/* The Dirichlet prior's per-category terms of ABCDSampler.kl_divergence
 * (model.py:608-639: alpha = softmax(posterior_shape_logits) * N + a0, its
 * digamma / trigamma / lgamma terms) into the workspace stash -- they depend
 * on the parameters only, not on the batch, so a training step can run this
 * one-workgroup kernel on a side stream early and pass
 * mode | ABCD_SAMPLE_PRIOR_READY to abcd_sampler_forward_fused (same ws and
 * B, same entire_data_size, the side stream joined first).  plain: no-op. */
#define ABCD_SAMPLE_PRIOR_READY 0x100
int abcd_sampler_prior(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, int B, double entire_data_size,
                       void* ws, size_t ws_bytes, void* stream);
int abcd_sampler_forward_fused(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* h, int B,
                               int mode, float temperature, const float* noise, uint64_t seed, uint64_t offset,
                               double entire_data_size, float* logits, float* feats, float* kl_out, float* ppl_out,
                               void* ws, size_t ws_bytes, void* stream);
/* backward of forward+sample+kl.  d_feats: B x D (may be NULL); d_kl: device
 * scalar upstream grad of kl (may be NULL); d_h: B x E (may be NULL). */
int abcd_sampler_backward(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* h, int B,
                          int mode, float temperature, double entire_data_size, const float* d_feats,
                          const float* d_kl, float* d_h, const abcd_sampler_grads* g, void* ws, size_t ws_bytes,
                          void* stream);
/* the same, with the parameter gradients (codebook, posterior_shape_logits,
 * MLP weights and biases) queued on wgrad_stream (NULL or == stream: one
 * stream) after an event on `stream`; only the d_h chain stays on `stream`.
 * ABCD with d_feats and d_kl: one row-tiled sampler-head backward kernel
 * (d_logits, dU, dZ1, the bias / prior column sums and d posterior_shape_logits
 * in its last tile) + the d_h GEMM on `stream`; codebook / W2 / W1 GEMMs on
 * wgrad_stream.
 * The caller joins wgrad_stream before reading the gradients.
 * wgrad_stream == ABCD_DEFER_PARAMS (fused ABCD path only): the codebook / W2
 * / W1 gradients are not launched; the caller runs
 * abcd_sampler_backward_params with the same workspace (and h) later -- the
 * training step queues them after the encoder BPTT, off its critical path. */
#define ABCD_DEFER_PARAMS ((void*)(intptr_t)-1)
int abcd_sampler_backward_split(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* h, int B,
                                int mode, float temperature, double entire_data_size, const float* d_feats,
                                const float* d_kl, float* d_h, const abcd_sampler_grads* g, void* ws,
                                size_t ws_bytes, void* stream, void* wgrad_stream);
/* the deferred codebook / W2 / W1 gradients of a preceding
 * abcd_sampler_backward_split(..., ABCD_DEFER_PARAMS) on `stream`: one
 * batched launch (dC = [d_feats; U]^T [Y; dL / sqrt(D)], dW2 = dU^T Z1,
 * dW1 = dZ1^T h); returns 0 without work when that call took another path
 * (the split call records per workspace whether it deferred; a params call
 * without a matching deferral does nothing).
 * wgrad_stream (NULL or == stream: on `stream`): the launch goes there behind
 * an event on `stream`, in a tiling that co-resides with the encoder's
 * persistent BPTT (the training step queues it on its side stream behind the
 * decoder's weight gradients); the caller joins before reading them. */
int abcd_sampler_backward_params(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* h, int B,
                                 const abcd_sampler_grads* g, void* ws, size_t ws_bytes, void* stream,
                                 void* wgrad_stream);
/* The same backward split the way autograd sees the three reference methods:
 * sample_backward:  d_feats -> d_logits (written), d_codebook (written, may be NULL)
 *                   (plain: d_feats -> d[mean | log_var])
 * kl_backward:      d_kl -> d_logits (written, or added when accumulate), d_psl (may be NULL)
 * forward_backward: d_logits -> MLP grads, codebook grad of the logits product
 *                   (added to g->codebook when accumulate_codebook), d_h (may be NULL) */
int abcd_sampler_sample_backward(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, int B, int mode,
                                 float temperature, const float* d_feats, float* d_logits, float* d_codebook,
                                 void* ws, size_t ws_bytes, void* stream);
int abcd_sampler_kl_backward(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, int B,
                             double entire_data_size, const float* d_kl, int accumulate, float* d_logits,
                             float* d_psl, void* ws, size_t ws_bytes, void* stream);
int abcd_sampler_forward_backward(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* h, int B,
                                  const float* d_logits, float* d_h, const abcd_sampler_grads* g,
                                  int accumulate_codebook, void* ws, size_t ws_bytes, void* stream);
/* learning.py:171-178 diagnostics: out[0..2] = posterior clustering /
 * batch-mean / Dirichlet-shape perplexities (device floats) */
int abcd_perplexities(const float* logits, int B, int K, const float* posterior_shape_logits, float* out,
                      void* stream);
/* out[0] = exp(entropy of softmax(posterior_shape_logits)) (abcd_perplexities' out[2]) */
int abcd_shape_perplexity(const float* posterior_shape_logits, int K, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Decoder: RNN_Variational_Decoder (model.py:84-196, unidirectional)
 * ---------------------------------------------------------------------- */
typedef struct abcd_decoder_cfg {
  int output_size, hidden_size, mlp_hidden, feature_size, rnn_type;
  int feedback;      /* 1: feed the reparameterised sample back (self_feedback, or eval mode) */
  int num_speakers;  /* 0: no speaker embedding */
  int speaker_dim;
} abcd_decoder_cfg;
typedef struct abcd_decoder_params {
  const float* embed_speaker;  /* num_speakers x speaker_dim or NULL */
  const float *f2h_w, *f2h_b;  /* feature2hidden */
  abcd_mlp_w offset, mu, lv;   /* offset_predictor, emission mlps.0, mlps.1 */
  abcd_rnn_w cell;             /* rnn_cell.cell */
} abcd_decoder_params;
typedef struct abcd_decoder_grads {
  float* embed_speaker;
  float *f2h_w, *f2h_b;
  abcd_mlp_g offset, mu, lv;
  abcd_rnn_g cell;
} abcd_decoder_grads;

size_t abcd_decoder_workspace_bytes(const abcd_decoder_cfg* cfg, int T, int L, int B);
/* replaces RNN_Variational_Decoder.forward (model.py:147-196).
 * features: B x feature_size; speakers: device int64 B (or NULL);
 * gt = ground_truth_out (L x F, or NULL); gt_offset (L, or NULL);
 * eps: L x F standard normals in packed order (or NULL -> Philox(seed,offset));
 * outputs (each may be NULL): flatten_out, mu, log_var (L x F), offset_logits (L);
 * losses[0] = emission NLL, losses[1] = offset BCE (device floats). */
int abcd_decoder_forward(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const abcd_packed* x,
                         const float* features, const int64_t* speakers, const float* gt_offset,
                         const float* eps, uint64_t seed, uint64_t offset, float* flatten_out, float* mu,
                         float* log_var, float* offset_logits, float* losses, void* ws, size_t ws_bytes,
                         void* stream);
/* backward w.r.t. losses[0] (scaled by *d_em) and losses[1] (scaled by *d_off);
 * d_em/d_off are device scalars; d_features: B x feature_size (may be NULL).
 * ws must hold the abcd_decoder_forward of the same inputs and parameters
 * (its stashes and its packed weight layouts, transposed ones included). */
int abcd_decoder_backward(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const abcd_packed* x,
                          const float* features, const int64_t* speakers, const float* gt_offset,
                          const float* d_em, const float* d_off, float* d_features,
                          const abcd_decoder_grads* g, void* ws, size_t ws_bytes, void* stream);
/* The same backward with the weight-gradient reductions (K = all packed
 * frames) moved to `wgrad_stream`: d_features is complete in `stream` order
 * on return (so the sampler/encoder backward can follow on `stream` at once),
 * the weight gradients only in `wgrad_stream` order -- the caller joins the
 * two streams before reading them (e.g. before clip_grad_norm_).  The
 * weight-gradient kernels use a tiling that co-resides with the encoder's
 * persistent BPTT kernel.  wgrad_stream == NULL or == stream: identical to
 * abcd_decoder_backward. */
int abcd_decoder_backward_overlap(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const abcd_packed* x,
                                  const float* features, const int64_t* speakers, const float* gt_offset,
                                  const float* d_em, const float* d_off, float* d_features,
                                  const abcd_decoder_grads* g, void* ws, size_t ws_bytes, void* stream,
                                  void* wgrad_stream);
/* Training-mode decoder input dropout (RNN_Cell's nn.Dropout, model.py:289,297):
 * xmask is L x F (DEVICE, packed order) holding bernoulli(1-p)/(1-p) -- the
 * noise the dropout applies to step t's cell input at rows off[t] .. off[t]+bs_t
 * (row block 0 multiplies the zero initial input and only keeps the RNG
 * order).  The sample fed back is mask * x; flatten_out keeps x.  The
 * backward needs the same xmask.  xmask == NULL: no dropout (eval mode,
 * p = 0); cfg->feedback must be 1 when xmask is given. */
int abcd_decoder_forward_dropout(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const abcd_packed* x,
                                 const float* features, const int64_t* speakers, const float* gt_offset,
                                 const float* eps, const float* xmask, uint64_t seed, uint64_t offset,
                                 float* flatten_out, float* mu, float* log_var, float* offset_logits, float* losses,
                                 void* ws, size_t ws_bytes, void* stream);
/* the same, with the loss reductions (emission NLL, offset BCE sum -> losses)
 * queued on loss_stream (NULL or == stream: one stream) after events on
 * `stream`; the caller joins loss_stream before reading `losses`. */
int abcd_decoder_forward_split(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const abcd_packed* x,
                               const float* features, const int64_t* speakers, const float* gt_offset,
                               const float* eps, const float* xmask, uint64_t seed, uint64_t offset,
                               float* flatten_out, float* mu, float* log_var, float* offset_logits, float* losses,
                               void* ws, size_t ws_bytes, void* stream, void* loss_stream);
/* wgrad_stream == ABCD_DEFER_PARAMS: only the data-gradient part (offset head,
 * BPTT, initial-state / feature gradients: d_features complete in `stream`
 * order); the weight gradients are queued by abcd_decoder_backward_params
 * with the SAME arguments later on this host thread (the training step calls
 * it after queuing the sampler and encoder backward). */
int abcd_decoder_backward_dropout(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const abcd_packed* x,
                                  const float* features, const int64_t* speakers, const float* gt_offset,
                                  const float* xmask, const float* d_em, const float* d_off, float* d_features,
                                  const abcd_decoder_grads* g, void* ws, size_t ws_bytes, void* stream,
                                  void* wgrad_stream);
/* the deferred weight gradients of the preceding
 * abcd_decoder_backward_dropout(..., ABCD_DEFER_PARAMS) (same arguments): on
 * wgrad_stream (NULL or == stream: on `stream`) behind an event recorded at the
 * end of that call's data path, in the tiling that co-resides with the
 * encoder's persistent BPTT; with the side-stream gate on, behind a wait for
 * the encoder BPTT launched in between to be resident.  The caller joins
 * wgrad_stream before reading the gradients. */
int abcd_decoder_backward_params(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const abcd_packed* x,
                                 const float* features, const int64_t* speakers, const float* gt_offset,
                                 const float* xmask, const float* d_em, const float* d_off, float* d_features,
                                 const abcd_decoder_grads* g, void* ws, size_t ws_bytes, void* stream,
                                 void* wgrad_stream);

/* Free-running generation with learned stopping: what the reference's eval-mode
 * decoder loop (model.py:147-196 with no ground truth, sampler2mean for the
 * mean) would give if it cut each row where the offset predictor
 * (model.py:121-122,191) first fires, instead of at a length the caller knows.
 * Decoder rows are independent, so the forward runs on the full B x T_max
 * rectangle (abcd_decoder_forward's kernels, batch_sizes[t] = B) and the rows
 * are cut afterwards; the steps a row runs past its stop are the price.
 * features: B x feature_size; speakers: int64 B (or NULL).
 * mode ABCD_GEN_MEAN: the mean is emitted and fed back (run as eps = 0: out
 *   equals mu); eps, seed and offset are ignored.
 * mode ABCD_GEN_SAMPLE: the sample is fed back; eps: B*T_max x F standard
 *   normals in rectangle (time-major) order, or NULL -> Philox(seed, offset)
 *   as abcd_decoder_forward draws it.
 * cfg->feedback must be 1 (generation is eval mode).
 * Row b's length is max(min_len, t* + 1) with t* the first step whose offset
 * logit is > stop_logit (the firing frame is the segment's last, as is_offset
 * marks it in training); T_max when none is; a NaN logit never fires.
 * 1 <= T_max <= ABCD_GEN_MAX_T (the ordering kernel's LDS histogram),
 * min_len <= T_max, B <= ABCD_GEN_MAX_B (the stable rank is one workgroup's
 * O(B^2) count), B * T_max < 2^31.
 * Outputs: lengths[B] in input row order; order[B] = input row indices by
 * length descending, ties in input order (stable); batch_sizes[T_max] = rows
 * with length > t (0 past the longest row; DEVICE here, the caller copies it
 * to the host for a PackedSequence); total[0] = the sum of the lengths; out,
 * mu, log_var (x F) and offset_logits, each B*T_max rows or NULL, in
 * PackedSequence.data order of the sorted rows: packed row off[t] + j holds
 * step t of input row order[j] (off = exclusive scan of batch_sizes); rows at
 * and past total[0] are unspecified.
 * With abcd_timing_enable on, abcd_timing_read_kernel ids 8 / 9 / 10 read the
 * gen_stop_scan / gen_order / gen_gather launches (3: the decoder forward). */
enum abcd_gen_mode { ABCD_GEN_MEAN = 0, ABCD_GEN_SAMPLE = 1 };
#define ABCD_GEN_MAX_T 4096
#define ABCD_GEN_MAX_B 16384
size_t abcd_decoder_generate_workspace_bytes(const abcd_decoder_cfg* cfg, int T_max, int B);
int abcd_decoder_generate(const abcd_decoder_cfg* cfg, const abcd_decoder_params* p, const float* features,
                          const int64_t* speakers, int B, int T_max, int mode, const float* eps, uint64_t seed,
                          uint64_t offset, float stop_logit, int min_len, float* out, float* mu, float* log_var,
                          float* offset_logits, int32_t* lengths, int64_t* order, int64_t* batch_sizes,
                          int64_t* total, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Per-segment ELBO terms: the losses above before they are summed over the
 * batch.  The reference only ever forms the batch scalars (model.py:193-195,
 * 608-639; learning.py:200-240 logs their per-epoch means).
 *
 * abcd_segment_losses: segment b (packed row order, b = 0 the longest) owns
 * packed rows off[t] + b for every t with batch_sizes[t] > b.
 *   seg_em[b]  = sum over those rows and F columns of
 *                0.5 (log 2pi + lv + (y - mu)^2 e^-lv), y = x->data (L x F);
 *   seg_off[b] = sum over those rows of max(x,0) - x y + log1p(e^-|x|),
 *                x = offset_logits (L), y = gt_offset (L): both or neither;
 *   seg_len[b] = the segment's length, the number of t with batch_sizes[t] > b.
 * Each output (B entries) may be NULL.  mu / log_var: L rows with row strides
 * ld_mu / ld_lv >= F floats (the L x F outputs of abcd_decoder_forward, or a
 * padded stash); columns >= F and rows of other segments are not read.  The
 * terms are those of abcd_decoder_forward's losses: fp32 terms, fp64 sums in a
 * fixed order (no atomics: two calls on the same inputs agree bit for bit), one
 * cast to fp32 per segment.  One launch, one 1024-thread workgroup per segment;
 * the step offsets travel through ws (abcd_segment_losses_workspace_bytes, 0
 * for an unsupported T > 16383) without a host synchronisation.
 * ABCD_EINVAL (nothing is written): batch_sizes not non-increasing,
 * batch_sizes[0] != B, L != sum batch_sizes, a stride below F, seg_em with
 * x->data, mu or log_var NULL, seg_off without the logits, one of
 * offset_logits / gt_offset alone.
 *
 * abcd_sampler_kl_rows: the per-row part of ABCDSampler.kl_divergence.  With
 * elog = digamma(alpha) - digamma(sum alpha) as abcd_sampler_kl forms it,
 *   rows[b]  = sum_k q log q - sum_k q elog[k], q = softmax(logits[b]) over the
 *              first valid_categories columns (padding columns masked out);
 *   prior[0] = Eq log q(pi) - Eq log p(pi), the batch-independent bracket;
 * abcd_sampler_kl's scalar is prior[0] * B / entire_data_size + sum_b rows[b].
 * plain: rows[b] = -0.5 sum_f (1 + lv - mu^2 - e^lv) of logits = [mean |
 * log_var] (B x 2 feature_dim), prior[0] = 0.  One launch, one wave per row;
 * num_categories <= 8192 (any size, no multiple of 16 needed).  The call keeps
 * no stash: ws / ws_bytes are not used (NULL / 0 are fine) and a sampler
 * workspace holding a forward's stash is left as it is.
 *
 * Neither entry point touches a device-global ticket word: both may run
 * beside any other launch.  With abcd_timing_enable on,
 * abcd_timing_read_kernel ids 11 / 12 read the seg_losses / kl_rows launches;
 * abcd_dispatch_name(11 / 12) names them ("seg_losses<1024> grid 512",
 * "kl_rows_seg<128,128> grid 128", "kl_rows_plain<16> grid 128").
 * ---------------------------------------------------------------------- */
size_t abcd_segment_losses_workspace_bytes(int T, int B);
int abcd_segment_losses(const abcd_packed* x, const float* mu, long ld_mu, const float* log_var, long ld_lv,
                        const float* offset_logits, const float* gt_offset, float* seg_em, float* seg_off,
                        int32_t* seg_len, void* ws, size_t ws_bytes, void* stream);
int abcd_sampler_kl_rows(const abcd_sampler_cfg* cfg, const abcd_sampler_params* p, const float* logits, int B,
                         double entire_data_size, float* rows, float* prior, void* ws, size_t ws_bytes,
                         void* stream);

/* ------------------------------------------------------------------------
 * Every segment against every category prototype.  The decoder feeds back its
 * own output and never sees the ground truth, so with eps = 0 in eval form its
 * mu / log_var / offset logit at step t depend on (features, speaker, t) only:
 * decoding P feature vectors once as a P-row rectangle (abcd_decoder_forward
 * with batch_sizes[t] = P) gives the emission parameters every segment would
 * get under each of them, the prototypes.
 *
 * abcd_pairwise_nll: x is the packed batch (L x F, HOST batch_sizes) as
 * abcd_segment_losses takes it, gt_offset its L offset targets.  The
 * prototypes are a time-major rectangle, prototype p at step t in row t P + p:
 * proto_mu / proto_lv with row strides ld_mu / ld_lv >= F floats,
 * proto_offset_logits T_proto * P entries; T_proto >= x->T (a rectangle
 * decoded for the longest batch serves shorter ones).  Rows at steps >= x->T
 * and columns >= F are never read.  With len_b the number of t with
 * batch_sizes[t] > b and off the exclusive scan of batch_sizes,
 *   pair_em [b ld_pair + p] = sum_{t < len_b} sum_{f < F} 0.5 (log 2pi + lv[t,p,f]
 *                             + (x[off_t + b, f] - mu[t,p,f])^2 e^-lv[t,p,f]);
 *   pair_off[b ld_pair + p] = sum_{t < len_b} max(o,0) - o y + log1p(e^-|o|),
 *                             o = proto_offset_logits[t P + p], y = gt_offset[off_t + b].
 * Either output (B rows, ld_pair >= P) may be NULL.  fp32 terms; e^-lv, the
 * softplus of the logit and 0.5 sum_f (log 2pi + lv) are formed once per staged
 * prototype element, not per pair; one frame's F columns are summed in fp32,
 * frames in fp64 in step order, one cast per result.  Workgroups take 32
 * segments x 32 prototypes x 16 steps and write fp64 partials to ws, which a
 * second launch sums in slice order: the order of every sum is a function of
 * (len_b, F) alone, there are no atomics and no workgroup waits for another,
 * and two calls on the same inputs agree bit for bit.
 * abcd_pairwise_nll_workspace_bytes is 0 for T > 16383 or B * P >= 2^31.
 * ABCD_EINVAL (nothing is written, checked before any launch): a batch_sizes
 * abcd_segment_losses rejects, P < 1, T_proto < x->T, a stride below F,
 * ld_pair < P, pair_em with x->data, proto_mu or proto_lv NULL, pair_off
 * without gt_offset and proto_offset_logits, a missing or short workspace.
 *
 * abcd_pair_posterior: s[b,p] = log_weight[p] - pair_em[b,p] - pair_off[b,p]
 * (a NULL log_weight or pair_off counts as 0), differences and log-sum-exp in
 * fp64 (the NLLs are ~1e5 with gaps of order 1).  One wave per row, 1 <= P <=
 * 2^20, no workspace.  Each output may be NULL:
 *   log_evidence[b] = logsumexp_p s[b,p];  resp[b ld_resp + p] = exp(s[b,p] -
 *   log_evidence[b]);  best[b] = the lowest index attaining the maximum;
 *   best_prob[b] = resp[b, best[b]].
 * A NaN or +inf NLL, or a NaN or -inf weight, excludes that prototype (resp
 * exactly 0); a row with every prototype excluded gets log_evidence = -inf,
 * best = -1, best_prob = 0, resp = 0.
 *
 * Neither entry point touches a device-global ticket word.  With
 * abcd_timing_enable on, abcd_timing_read_kernel ids 13 / 14 read the pair_nll
 * (both of its launches) / pair_posterior launches; abcd_dispatch_name(13 / 14)
 * names them ("pair_nll<32x32x16> grid 4x16x7", "pair_posterior<128> grid 128").
 * ---------------------------------------------------------------------- */
size_t abcd_pairwise_nll_workspace_bytes(int T, int B, int P);
int abcd_pairwise_nll(const abcd_packed* x, const float* gt_offset, int P, int T_proto, const float* proto_mu,
                      long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                      float* pair_em, float* pair_off, long ld_pair, void* ws, size_t ws_bytes, void* stream);
int abcd_pair_posterior(const float* pair_em, const float* pair_off, long ld_pair, int B, int P,
                        const float* log_weight, float* log_evidence, int32_t* best, float* best_prob, float* resp,
                        long ld_resp, void* stream);

/* ------------------------------------------------------------------------
 * A hidden Markov model over the category sequence of a recording: the K
 * categories are the states, score[n ld_score + k] the log-likelihood of
 * segment n under category k up to a per-row constant (the callers take each
 * row's maximum off, ops.chain_scores), log_trans[i ld_trans + j] = log p(z_t+1
 * = j | z_t = i) and log_init[k] log-probabilities (-inf: a structural zero).
 * Sequence s owns rows seq_off[s] .. seq_off[s + 1] - 1 in time order; seq_off
 * is a HOST array of S + 1 entries, validated on the host and copied to the
 * workspace through the pinned offset ring, 16384 entries per slot (a longer
 * table takes several slots); the call does no host synchronisation.
 *
 * abcd_chain_posterior, per sequence of rows 0 .. T - 1:
 *   alpha_0 = log_init + score_0,
 *   alpha_t+1[j] = score_t+1[j] + logsumexp_i(alpha_t[i] + log_trans[i,j]);
 *   log_evidence[s] = logsumexp_k alpha_T-1[k];
 *   beta_T-1 = 0, beta_t[i] = logsumexp_j(log_trans[i,j] + score_t+1[j] + beta_t+1[j]);
 *   gamma[n ld_gamma + k] = exp(alpha_t[k] + beta_t[k] - log_evidence) (rows sum to 1);
 *   xi_t[i,j] = exp(alpha_t[i] + log_trans[i,j] + score_t+1[j] + beta_t+1[j] - log_evidence);
 *   trans_counts[i K + j] = sum_s sum_t xi_t[i,j];  init_counts[k] = sum_s gamma_0[k];
 *   path: delta_0 = alpha_0, delta_t+1[j] = score_t+1[j] + max_i(delta_t[i] + log_trans[i,j]),
 *   the final state and every back-pointer the LOWEST index attaining the
 *   maximum; path_score[s] = the path's log joint log_init[p_0] + score_0[p_0] +
 *   sum_t log_trans[p_t, p_t+1] + score_t+1[p_t+1].
 * Every output may be NULL.  Groups (the `want` of the workspace query): 1
 * log_evidence, 2 gamma, 4 path / path_score, 8 trans_counts / init_counts; a
 * Viterbi-only call stores no alphas.  All of it runs in the log domain: every
 * vector is renormalised to a maximum of 0 after each step in fp32, and what
 * was taken off (the evidence), the counts and path_score accumulate in fp64.
 * A score entry that is NaN or +inf counts as -inf.  A sequence whose forward
 * mass vanishes (an all-excluded row, zeros that leave no path) gets
 * log_evidence = -inf, gamma = 0, path = -1, path_score = -inf and adds nothing
 * to the counts; a zero-length sequence gets log_evidence = 0 and nothing else;
 * a length-1 sequence adds to init_counts only.
 *
 * One workgroup owns a sequence for all of its time loops; workgroup g of G
 * takes sequences g, g + G, ...  abcd_chain_plan (a pure function) reports G
 * for an S and whether a K runs resident (log_trans in LDS for the whole
 * launch, K <= 128) or streaming (log_trans read from global memory every
 * step, K <= 1024).  The counts are summed by a launch of their own from the
 * alpha and score + beta rows the backward pass stores (resident: workgroup g
 * sums its sequences into a slab of fp64 partials in the workspace, and a last
 * small launch adds the slabs in workgroup order; streaming: the K x K entries
 * are tiled over the workgroups and each walks every sequence in order): no
 * atomics, no device-global word, no workgroup waits for another, and two
 * calls on the same inputs agree bit for bit.  No timing or dispatch id is
 * assigned.
 * abcd_chain_workspace_bytes is 0 for K < 1, K > 1024, N < 0, S < 0, N K >=
 * 2^31 or a want outside 0 .. 15.  ABCD_EINVAL (checked before any launch,
 * nothing is written): those shapes; seq_off NULL, not non-decreasing,
 * seq_off[0] != 0 or seq_off[S] != N; a stride below K; score, log_trans or
 * log_init NULL while an output is requested; a missing or short workspace.
 * With every output NULL a valid call returns 0 without a device.
 * ---------------------------------------------------------------------- */
size_t abcd_chain_workspace_bytes(long N, int S, int K, int want);
int abcd_chain_plan(int K, int S, int* resident, int* workgroups);
int abcd_chain_posterior(const float* score, long ld_score, long N, int K, const int64_t* seq_off, int S,
                         const float* log_trans, long ld_trans, const float* log_init, double* log_evidence,
                         float* gamma, long ld_gamma, int32_t* path, double* path_score, double* trans_counts,
                         double* init_counts, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Segmentation: cutting an uncut recording into labelled segments.  With the
 * prototypes of abcd_pairwise_nll (time-major rectangle, row t P + p, T_proto
 * >= D steps) the log-likelihood of "frames s .. s + d - 1 are one segment of
 * prototype p that ends after d frames" is
 *   S[s,p,d] = log_weight[p] - E[s,p,d] - O[p,d],
 *   E[s,p,d] = sum_{t < d} 0.5 sum_{f < F} (log 2pi + lv[t,p,f] + (x[s+t,f] - mu[t,p,f])^2 e^-lv[t,p,f]),
 *   O[p,d]   = sum_{t < d-1} sp(o[t,p]) + sp(-o[d-1,p]),  sp(v) = max(v,0) + log1p(e^-|v|)
 * (the BCE of the offset logits o against a target that is one on the last
 * step: a duration model).  A frame's F columns are summed in fp32 in column
 * order exactly as abcd_pairwise_nll sums them; everything across steps (E, O,
 * the differences) is fp64 in step order.  A NULL log_weight counts as 0.
 *
 * abcd_span_scores: x is the recording, N frames with row stride ld_x >= F.
 * The output is END-major: for e = s + d, 1 <= e <= N, 1 <= d <= min(D, e),
 *   span_score[e ld_span + d - 1] = max_p S[e-d, p, d],
 *   span_cat  [e ld_span + d - 1] = the lowest p attaining it,
 * rows e = 0 .. N (N + 1 rows, ld_span >= D), so that the dynamic programme
 * reads one contiguous row per step.  A p whose S is NaN or -inf (a NaN or
 * +inf E, a NaN or -inf weight, a NaN O) is excluded; a span with nothing left,
 * and every entry with d > e (row 0 among them), gets -inf and -1.  One
 * workgroup owns 32 consecutive starts and walks the prototype tiles of 32
 * itself, in order, so the maximum does not depend on scheduling: no atomics,
 * no device-global word, no workgroup waits for another, two calls agree bit
 * for bit, and S[s,p,d] is a function of frames s .. s + d - 1 alone (frames
 * prepended to the recording shift the same bits).  Rows >= N of x, steps >= D
 * of the rectangle and columns >= F are never read.  The workspace holds O
 * (D P doubles).
 * Limits: 1 <= D <= 16383, P >= 1, F >= 1, 0 <= N, (N + 1) D < 2^31; the
 * workspace query returns 0 beyond them.  ABCD_EINVAL (checked before any
 * launch, nothing is written): those shapes, T_proto < D, a stride below F,
 * ld_span < D, x, proto_mu, proto_lv, proto_offset_logits, span_score or
 * span_cat NULL while N > 0, a missing or short workspace.  N = 0 is valid and
 * writes row 0 only (nothing when the outputs are NULL).
 *
 * abcd_span_viterbi: the semi-Markov dynamic programme over one recording,
 *   V[0] = 0,
 *   V[n] = max(V[n-1] + gap[n-1],
 *              max_{d_min <= d <= min(D, n)} (V[n-d] + span_score[n ld_span + d - 1]) + seg_bonus)
 * in fp64 with the additions made in exactly that order.  gap (N floats, may
 * be NULL = -inf: the recording must be tiled by segments) is the per-frame
 * log-likelihood of "no segment here", seg_bonus a per-segment log prior.  NaN
 * candidates are excluded; the gap wins a tie against any segment, then the
 * smallest d; V[n] = -inf when nothing is left.  One workgroup runs the whole
 * loop and the backtrack in one launch (V in a ring of D doubles in LDS, one
 * barrier per step) and writes the segments in time order: seg_onset,
 * seg_length, seg_cat (span_cat of the chosen entry), seg_score (its
 * span_score), each of N / d_min entries, n_segments of them valid;
 * path_score = V[N].  An unreachable end (V[N] = -inf) gives path_score = -inf
 * and n_segments = 0.  V_out (N + 1 doubles) may be NULL.  The workspace holds
 * the N + 1 back-pointers.
 * ABCD_EINVAL: d_min < 1 or d_min > D, the limits above, ld_span < D, a NULL
 * among span_score, span_cat, path_score, n_segments and the four segment
 * buffers while N > 0, a missing or short workspace.  N = 0 gives path_score =
 * 0 and n_segments = 0 (each where not NULL) without reading anything.
 *
 * No timing or dispatch id is assigned to either entry point.
 * ---------------------------------------------------------------------- */
size_t abcd_span_scores_workspace_bytes(long N, int D, int P);
int abcd_span_scores(const float* x, long ld_x, long N, int F, int P, int D, int T_proto, const float* proto_mu,
                     long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                     const float* log_weight, double* span_score, int32_t* span_cat, long ld_span, void* ws,
                     size_t ws_bytes, void* stream);
size_t abcd_span_viterbi_workspace_bytes(long N, int D);
int abcd_span_viterbi(const double* span_score, const int32_t* span_cat, long ld_span, long N, int D, int d_min,
                      const float* gap, double seg_bonus, double* path_score, int32_t* n_segments,
                      int32_t* seg_onset, int32_t* seg_length, int32_t* seg_cat, double* seg_score, double* V_out,
                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Segmentation posteriors: the sum half of the section above (DESIGN.md
 * s3.12).  S, E and O are those of abcd_span_scores.
 *
 * abcd_span_evidence: the pass of abcd_span_scores with the prototypes summed,
 *   span_lse[e ld_span + d - 1] = log sum_p exp S[e-d, p, d],
 * over the prototypes abcd_span_scores would not exclude; -inf where nothing is
 * left and where d > e.  span_score and span_cat may both be NULL; given, they
 * come out of the same pass and hold the bits abcd_span_scores writes for the
 * same inputs (all three outputs share ld_span).  Per prototype tile of 32 the
 * 16 lanes of a start reduce the maximum and then sum_p exp(S - maximum) (the
 * differences, <= 0, exponentiated in fp32; the maximum, the sum and the
 * logarithm in fp64) in a fixed shuffle order, and the thread that wrote an
 * entry folds the later tiles into it with a logaddexp, in tile order: the
 * ownership rule, the determinism, the limits, the never-read regions, the
 * workspace and the ABCD_EINVAL rules of abcd_span_scores hold, with span_lse
 * in span_score's place; span_score NULL and span_cat not, or the reverse, is
 * ABCD_EINVAL too.
 *
 * abcd_span_posterior: the semi-Markov forward-backward over one recording in
 * fp64.  span is a table laid out as span_score (the maximum or the sum: the
 * programme does not care), gap / seg_bonus / d_min are those of
 * abcd_span_viterbi.  A candidate that is NaN or -inf is excluded; LAE is
 * logaddexp, LSE the log-sum-exp over the admissible candidates, -inf over none:
 *   a[0] = 0, aseg[0] = -inf;  n = 1 .. N:
 *     aseg[n] = seg_bonus + LSE_{d_min <= d <= min(D,n)} (a[n-d] + span[n,d])
 *     a[n]    = LAE(a[n-1] + gap[n-1], aseg[n])
 *   b[N] = 0, bseg[N] = -inf;  n = N-1 .. 0:
 *     bseg[n] = LSE_{d_min <= d <= min(D,N-n)} (span[n+d,d] + seg_bonus + b[n+d])
 *     b[n]    = LAE(gap[n] + b[n+1], bseg[n])
 *   log_z = a[N]
 *   post[n]             = exp(a[n] + bseg[n] - log_z), n < N      a segment starts at frame n
 *   post[N+1 + n]       = exp(aseg[n] + b[n] - log_z), n >= 1     a segment ends before frame n
 *   post[2 (N+1) + n]   = exp(a[n] + gap[n] + b[n+1] - log_z), n < N   frame n is background
 *   span_post[e ld_post + d - 1] = exp(a[e-d] + span[e,d] + seg_bonus + b[e] - log_z)
 * and 0 elsewhere (post is 3 x (N + 1), span_post N + 1 rows with ld_post >=
 * D, zero outside d_min .. min(D, e)); log_z = -inf (no cover) makes every
 * posterior 0.  lattice (4 x (N + 1): a, aseg, b, bseg) and span_post may be
 * NULL.  One workgroup runs both sweeps and the per-frame posteriors in one
 * launch; the backward sweep walks the ENDS e = N .. 1 and folds span[e,d] +
 * seg_bonus + b[e] into a ring slot per start, so it reads the same contiguous
 * rows as the forward sweep.  span_post comes from a second, ordinary kernel,
 * launched only when asked for.  No atomics, no device-global word, nothing is
 * allocated, two calls agree bit for bit.  A table that holds +inf is outside
 * the contract (the result is unspecified; nothing outside the arguments is
 * touched).  The workspace holds the lattice when the caller keeps none.
 * Limits: those of abcd_span_viterbi; the workspace query returns 0 beyond
 * them.  ABCD_EINVAL (checked before any launch, nothing is written): d_min < 1
 * or d_min > D, ld_span < D, ld_post < D with span_post given, span, log_z or
 * post NULL while N > 0, a missing or short workspace.  N = 0 writes log_z = 0
 * (and a = b = 0, aseg = bseg = -inf, zero posteriors, each where not NULL) and
 * reads nothing.
 *
 * No timing or dispatch id is assigned to either entry point.
 * ---------------------------------------------------------------------- */
size_t abcd_span_evidence_workspace_bytes(long N, int D, int P);
int abcd_span_evidence(const float* x, long ld_x, long N, int F, int P, int D, int T_proto, const float* proto_mu,
                       long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                       const float* log_weight, double* span_lse, double* span_score, int32_t* span_cat,
                       long ld_span, void* ws, size_t ws_bytes, void* stream);
size_t abcd_span_posterior_workspace_bytes(long N, int D);
int abcd_span_posterior(const double* span, long ld_span, long N, int D, int d_min, const float* gap,
                        double seg_bonus, double* log_z, double* lattice, double* post, double* span_post,
                        long ld_post, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Syntax-aware segmentation: category transitions inside the span programme
 * (DESIGN.md s3.13).  S is that of abcd_span_scores; K categories = the P
 * prototypes.
 *
 * abcd_span_table: the pass of abcd_span_scores keeping every prototype,
 *   table[(e D + d - 1) ld_k + p] = S[e-d, p, d],  0 <= e <= N, 1 <= d <= D, p < P
 * (end-major, ld_k >= P; columns P .. ld_k - 1 are not written).  A p that
 * abcd_span_scores would exclude (S NaN or -inf) and every entry with d > e (row
 * 0 among them) hold -inf.  Each thread of the emission tile stores its own
 * four values: no thread reads what another wrote, nothing is folded across
 * prototype tiles, no atomics, no device-global word, two calls agree bit for
 * bit.  span_score and span_cat (row stride ld_span >= D) may both be NULL;
 * given, they come out of the same pass and hold the bits abcd_span_scores
 * writes; one of them alone is ABCD_EINVAL.  table.max over p and its lowest
 * argmax are those bits too.  Rows >= N of x, steps >= D, prototypes >= P and
 * columns >= F are never read.  The workspace holds O (D P doubles).
 * Limits: those of abcd_span_scores and (N + 1) D ld_k < 2^31; the workspace
 * query returns 0 beyond them (and for ld_k < P).  ABCD_EINVAL (before any
 * launch, nothing is written): as abcd_span_scores with table in span_score's
 * place, ld_k < P, ld_span < D with span_score given.  N = 0 writes row 0 only.
 * The table takes 8 (N + 1) D ld_k bytes.
 *
 * abcd_span_chain_viterbi: the semi-Markov programme with a first-order chain
 * over the categories of consecutive segments, one recording per launch, in
 * fp64 with every addition as written (fp32 inputs widened first):
 *   G[0] = 0,  G[n] = G[n-1] + gap[n-1]         (gap NULL: -inf for n >= 1)
 *   W[0][k] = -inf
 *   U[n][k]  = max(G[n] + log_init[k], max_k' (W[n][k'] + log_trans[k' ld_trans + k]))
 *   Vs[n][k] = max_{d_min <= d <= min(D,n)} (U[n-d][k] + table[(n D + d - 1) ld_k + k]) + seg_bonus
 *   W[n][k]  = max(W[n-1][k] + gap[n-1], Vs[n][k])
 *   path_score = max(G[N], max_k W[N][k])
 * Gap frames are transparent: the transition is paid between consecutive
 * segments however many gap frames lie between them.  log_trans (K rows,
 * ld_trans >= K) and log_init are log-probabilities as in abcd_chain_posterior:
 * -inf is a structural zero, NaN counts as -inf.  NaN and -inf candidates are
 * excluded; +inf in the table is outside the contract.  Ties: the smallest d
 * in Vs; the gap against a segment in W; the initial term against any
 * predecessor in U, then the lowest k'; at the end "no segment", then the
 * lowest k.  The backtrack from (N, k) follows d = 0 to (n-1, k), otherwise
 * emits (n-d, d, k) and goes to (n-d, the k' chosen in U[n-d][k]), and stops at
 * the initial term.  Segments come out in time order, N / d_min entries per
 * buffer, n_segments valid: seg_score is the chosen table entry, seg_link the
 * log_init or log_trans term paid on entering the segment, widened to fp64.
 * An uncoverable recording gives path_score = -inf and n_segments = 0.  W_out
 * ((N + 1) x K doubles) may be NULL.  One workgroup (1024 threads up to K =
 * 256, 256 threads above) runs the whole loop and the backtrack; lanes run
 * over k, the waves split d and k' and their partial maxima are combined in
 * wave order under the tie rules, so nothing is decided by scheduling and two
 * calls agree bit for bit.
 * log_trans is resident in LDS up to K = 128 and streamed from global memory
 * above (abcd_span_chain_plan says which, with the launch width and the LDS
 * bytes; it is a pure function).  The workspace holds U ((N + 1) K doubles)
 * and the two back-pointer planes ((N + 1) K int32 each).
 * Limits: 1 <= K <= 1024, those of abcd_span_table with ld_k; the workspace
 * query returns 0 beyond them ((N + 1) D K >= 2^31 included).  ABCD_EINVAL
 * (decided on the host before any launch, nothing is written): those limits,
 * d_min outside 1 .. D, ld_k < K, ld_trans < K, a NULL among table, log_trans,
 * log_init, path_score, n_segments and the five segment buffers while N > 0, a
 * missing or short workspace.  N = 0 gives path_score = 0, n_segments = 0 and
 * W_out[0][k] = -inf (each where not NULL) and reads nothing.
 *
 * Measured on one MI355X at N = 15 000, D = 200, K = 128, F = 129 (DESIGN.md
 * s3.13): abcd_span_table 9.7 ms (0.96 x abcd_span_scores),
 * abcd_span_chain_viterbi 209 ms (14 us per step; 19 us at K = 130, streaming):
 * the step is bound by reading its 205 KB table row on one CU.
 *
 * abcd_span_chain_viterbi_window: abcd_span_chain_viterbi in windows of ends
 * (DESIGN.md s3.15), for recordings whose whole table does not fit.  One call
 * runs steps n0 .. n1 of the recurrences above on a WINDOW of the table: row 0
 * of `table` is absolute end row0 and the buffer holds `rows` rows,
 *   step n reads table[((n - row0) D + d - 1) ld_k + k],  d_min <= d <= min(D, n)
 * (rows n0 - row0 .. n1 - row0 and no others).  abcd_span_table on the frames
 * row0 .. n1 - 1 (x + row0 ld_x, N = n1 - row0) IS that window when row0 is a
 * multiple of 32, the table pass's start tile: every start then sits at the
 * same place of its tile as in the pass over the whole recording, and every
 * entry with end >= n0 has the same bits.  The caller guarantees row0 <=
 * max(0, n0 - D), so every entry read is a real one.
 * Call order: n0 = 1 first, then every call's n0 = the previous call's n1 + 1,
 * until n1 = N; all calls of one recording on ONE stream (or otherwise
 * ordered) with the same workspace, N, D, K, d_min, seg_bonus, log_trans,
 * log_init, gap and W_out.  gap (N floats or NULL) and W_out ((N + 1) x K
 * doubles or NULL) are whole-recording buffers; each call reads gap[n0 - 1 ..
 * n1 - 1] and writes rows n0 .. n1 of W_out (row 0 too when n0 = 1).
 * path_score, n_segments and the five segment buffers are written by the call
 * with n1 = N alone, with the bits abcd_span_chain_viterbi writes on the whole
 * table.  The workspace carries the programme across the calls and must not
 * be touched between them: U and sel (the chosen segment's table entry per
 * (n, k): the table is gone when the backtrack runs), (N + 1) K doubles each,
 * the two back-pointer planes ((N + 1) K int32 each), and the carry block W[n1]
 * (K doubles), G[n1] and next_n = n1 + 1 (one 64-bit integer).  A call with n0
 * = 1 starts over on whatever the workspace holds.  A call whose n0 is neither
 * 1 nor the carried next_n is a caller's mistake: it runs no step, writes
 * path_score = NaN and n_segments = -1 and leaves the carry as it is.
 * Launch widths, LDS plan, tie rules: abcd_span_chain_plan; log_init and the
 * resident log_trans are loaded into LDS by every call.  No atomics, no
 * device-global word; two sequences of calls agree bit for bit.
 * Limits: 1 <= K <= 1024, span_scores' on (N, D); rows D ld_k < 2^31 (the
 * window's index limit; (N + 1) D K is NOT limited).  The workspace query
 * returns 0 beyond them.  ABCD_EINVAL (on the host before any launch, nothing
 * is written): those limits, not 1 <= n0 <= n1 <= N (N = 0 among them: take
 * abcd_span_chain_viterbi), row0 < 0, row0 > max(0, n0 - D), n1 - row0 >= rows,
 * d_min outside 1 .. D, ld_k < K, ld_trans < K, a NULL among table, log_trans,
 * log_init, path_score, n_segments and the five segment buffers, a missing or
 * short workspace.
 *
 * No timing or dispatch id is assigned to these entry points.
 * ---------------------------------------------------------------------- */
size_t abcd_span_table_workspace_bytes(long N, int D, int P, long ld_k);
int abcd_span_table(const float* x, long ld_x, long N, int F, int P, int D, int T_proto, const float* proto_mu,
                    long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                    const float* log_weight, double* table, long ld_k, double* span_score, int32_t* span_cat,
                    long ld_span, void* ws, size_t ws_bytes, void* stream);
int abcd_span_chain_plan(int K, int D, int* resident, int* threads, size_t* lds_bytes);
size_t abcd_span_chain_workspace_bytes(long N, int D, int K);
int abcd_span_chain_viterbi(const double* table, long ld_k, long N, int D, int K, int d_min, const float* gap,
                            double seg_bonus, const float* log_trans, long ld_trans, const float* log_init,
                            double* path_score, int32_t* n_segments, int32_t* seg_onset, int32_t* seg_length,
                            int32_t* seg_cat, double* seg_score, double* seg_link, double* W_out, void* ws,
                            size_t ws_bytes, void* stream);
size_t abcd_span_chain_window_workspace_bytes(long N, int D, int K);
int abcd_span_chain_viterbi_window(const double* table, long ld_k, long row0, long rows, long n0, long n1, long N,
                                   int D, int K, int d_min, const float* gap, double seg_bonus,
                                   const float* log_trans, long ld_trans, const float* log_init, double* path_score,
                                   int32_t* n_segments, int32_t* seg_onset, int32_t* seg_length, int32_t* seg_cat,
                                   double* seg_score, double* seg_link, double* W_out, void* ws, size_t ws_bytes,
                                   void* stream);

/* ------------------------------------------------------------------------
 * Segmentation posteriors under the chain: the sum half of
 * abcd_span_chain_viterbi.  table, gap, seg_bonus, d_min,
 * log_trans and log_init are those of abcd_span_chain_viterbi; scale is 1 /
 * temperature and multiplies every term (table entries, gap, seg_bonus,
 * log_trans, log_init) in fp64 after widening, so scale = 1 is exact.  Below
 * T, gap, bonus, lt, li are the multiplied terms; a candidate that is NaN or
 * -inf is excluded; LAE is logaddexp, LSE the log-sum-exp over the admissible
 * candidates, -inf over none:
 *   G[0] = 0,  G[n] = G[n-1] + gap[n-1]         (gap NULL: -inf for n >= 1)
 *   aW[0][k] = aV[0][k] = -inf
 *   aU[n][k] = LAE(G[n] + li[k], LSE_k' (aW[n][k'] + lt[k'][k])),  n < N;  aU[N][k] = -inf
 *   aV[n][k] = bonus + LSE_{d_min <= d <= min(D,n)} (aU[n-d][k] + T[n,d,k])
 *   aW[n][k] = LAE(aW[n-1][k] + gap[n-1], aV[n][k])
 *   log_z    = LAE(G[N], LSE_k aW[N][k])
 *   bW[N][k] = 0, bG[N] = 0, bU[N][k] = -inf;  n = N-1 .. 0:
 *   bU[n][k] = LSE_{d_min <= d <= min(D,N-n)} (T[n+d,d,k] + bonus + bW[n+d][k])
 *   bW[n][k] = LAE(gap[n] + bW[n+1][k], LSE_k'' (lt[k][k''] + bU[n][k'']))
 *   bG[n]    = LAE(gap[n] + bG[n+1], LSE_k (li[k] + bU[n][k]))          (bG[0] = log_z)
 *   post_k[n K + k]             = exp(aU[n][k] + bU[n][k] - log_z)   a segment of k starts at frame n
 *   post_k[(N + 1) K + n K + k] = exp(aV[n][k] + bW[n][k] - log_z)   a segment of k ends before frame n
 *   gap_post[n] = exp(LAE(G[n] + bG[n+1], LSE_k (aW[n][k] + bW[n+1][k])) + gap[n] - log_z),  n < N;  [N] = 0
 *   init_counts[k]          = sum_{n < N} exp(G[n] + li[k] + bU[n][k] - log_z)
 *   trans_counts[k' K + k]  = sum_{n < N} exp(aW[n][k'] + lt[k'][k] + bU[n][k] - log_z)
 *   span_post[e ld_post + d - 1] = sum_k exp(aU[e-d][k] + T[e,d,k] + bonus + bW[e][k] - log_z)
 * (span_post: N + 1 rows, zero outside d_min .. min(D, e)).  log_z = -inf (no
 * cover) makes every posterior and count 0.  lattice is five planes of (N + 1)
 * x K doubles (aU, aV, aW, bU, bW), lattice_g two of N + 1 (G, bG); both may be
 * NULL and then live in the workspace.  trans_counts (K x K, row stride K) and
 * init_counts (K) come together or not at all; span_post may be NULL.
 * One workgroup (abcd_span_chain_viterbi's launch widths: 1024 threads up to K
 * = 256, 256 above) runs both sweeps, the counts and the per-frame posteriors
 * in one launch: lanes over k, the waves split d and k', each wave keeps a
 * (maximum, sum of exp(c - maximum)) pair per k, the pairs meet in LDS and one
 * thread per k joins them in wave order.  The backward sweep walks the starts
 * n = N-1 .. 0 (T[n+d, d, :] is contiguous).  log_trans is resident in LDS up
 * to K = 128 at a row stride of K + 1 floats and streamed above; streamed, the
 * backward chain phase gives each wave whole rows of log_trans
 * (abcd_span_chain_posterior_plan says which, with the launch width and the
 * LDS bytes; it is a pure function).  A count entry is owned by one thread
 * and summed in n order.  span_post comes from a second, ordinary kernel,
 * launched only when asked for.  No atomics, no device-global word, nothing is
 * allocated, two calls agree bit for bit.  +inf in the table is outside the
 * contract.
 * Limits: those of abcd_span_chain_viterbi (1 <= K <= 1024, (N + 1) D ld_k <
 * 2^31); the workspace query returns 0 beyond them.  ABCD_EINVAL (decided on
 * the host before any launch, nothing is written): those limits, d_min outside
 * 1 .. D, scale not finite or not positive, ld_k < K, ld_trans < K, ld_post < D
 * with span_post given, exactly one of the two count buffers, a NULL among
 * table, log_trans, log_init, log_z, post_k and gap_post while N > 0, a missing
 * or short workspace.  N = 0 writes log_z = 0, bW[0][k] = G[0] = bG[0] = 0,
 * -inf in the other four planes and zero posteriors and counts (each where not
 * NULL) and reads nothing.
 *
 * No timing or dispatch id is assigned to these entry points.
 * ---------------------------------------------------------------------- */
int abcd_span_chain_posterior_plan(int K, int D, int* resident, int* threads, size_t* lds_bytes);
size_t abcd_span_chain_posterior_workspace_bytes(long N, int D, int K);
int abcd_span_chain_posterior(const double* table, long ld_k, long N, int D, int K, int d_min, const float* gap,
                              double seg_bonus, double scale, const float* log_trans, long ld_trans,
                              const float* log_init, double* log_z, double* lattice, double* lattice_g,
                              double* post_k, double* gap_post, double* trans_counts, double* init_counts,
                              double* span_post, long ld_post, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Time-warped scoring: a segment aligned to a prototype.  abcd_pairwise_nll
 * scores frame t against step t; here the T_proto steps of prototype p are the
 * states of a left-to-right HMM and frame t of segment b is emitted by state
 * a(t), with a(0) = 0 and a(t + 1) - a(t) = m in {0, 1, 2} (stay, step, skip)
 * at a cost of -log_move[m].  x, gt_offset and the prototype rectangle are
 * those of abcd_pairwise_nll, except that T_proto (1 .. 16383) may be shorter
 * or longer than x->T.  log_move is a HOST array of three doubles; -inf
 * disables a move.  band < 0: no band; otherwise cells with |s - t| > band do
 * not exist.  With r = off_t + b,
 *   e(t,s) = 0.5 sum_f (log 2pi + lv[s,p,f] + (x[r,f] - mu[s,p,f])^2 e^-lv[s,p,f])
 *            (fp32, one frame's F columns exactly as abcd_pairwise_nll sums them),
 *   o(t,s) = max(v,0) - v y[r] + log1p(e^-|v|),  v = proto_offset_logits[s P + p]  (fp32),
 *   c(t,s) = e(t,s) + o(t,s), and in fp64
 *   D[0,0] = c(0,0), D[0,s>0] = +inf,
 *   D[t,s] = c(t,s) + (+)_{m, s-m >= 0} (D[t-1,s-m] - log_move[m]),
 *   warp[b ld_warp + p] = (+)_s D[len_b - 1, s],
 * where (+) is min (marginal = 0: the best alignment) or -log sum exp(-.)
 * (marginal != 0: all alignments).  A disabled move, a +inf predecessor, a
 * cell outside the band and a NaN cost are excluded; a cell with nothing left
 * is +inf, and a pair no alignment reaches gets warp = +inf (which
 * abcd_pair_posterior excludes).  Viterbi ties go to the lowest move, then to
 * the lowest final state.  With log_move = (-inf, 0, -inf) and T_proto >= len_b
 * warp is pair_em + pair_off up to the order of the fp64 sums.
 *
 * abcd_warp_nll: one workgroup per (b, p) walks the segment in blocks of 32
 * frames and the states in super-blocks of 128: the emission terms of up to
 * four 32-frame x 32-step tiles (the tile of abcd_pairwise_nll, the prototype's
 * steps fetched P rows apart) go to LDS, then 128 threads, one state each, run
 * the recurrence over the block's frames.  The cost plane is never written to
 * memory.  Tiles wholly outside the band, above s = 2 t or beyond T_proto are
 * skipped.  States >= T_proto, rows >= L and columns >= F are never read.  The
 * order of every sum is a function of (len_b, T_proto, F, band) alone: no
 * atomics, no device-global word, no workgroup waits for another, two calls
 * agree bit for bit, and a segment scored alone gets the bits of its in-batch
 * row.  The workspace holds the step offsets.
 *
 * abcd_warp_path: the Viterbi programme for ONE prototype per segment,
 * choice[b] (device, B entries; a value outside 0 .. P - 1 skips the segment,
 * whose frames are then never read).  state (device, L entries, packed: row
 * off_t + b) receives a(t), or -1 for a skipped segment and for one no
 * alignment reaches; path_em / path_off / path_move (B floats each, may be
 * NULL) the path's sum of e, of o and of -log_move in fp64 (+inf where state
 * is -1), so that their sum is the path's cost.  One workgroup per segment;
 * the workspace holds a one-byte back-pointer and the fp32 emission term of
 * every (t, s) with s < min(T_proto, 2 x->T - 1), and the backtrack runs on
 * the device in the same launch.
 *
 * Limits: x->T <= 4096, B P < 2^31, 1 <= T_proto <= 16383; the workspace
 * queries return 0 beyond them.  ABCD_EINVAL (checked before any launch,
 * nothing is written): those limits, a batch_sizes abcd_segment_losses
 * rejects, P < 1, a stride below F, x->data, gt_offset, proto_mu, proto_lv,
 * proto_offset_logits or log_move NULL, a NaN or +inf move weight, all three
 * moves disabled, ld_warp < P, warp (abcd_warp_nll) or choice / state
 * (abcd_warp_path) NULL, a missing or short workspace.  No timing or dispatch
 * id is assigned to either entry point.
 * ---------------------------------------------------------------------- */
size_t abcd_warp_nll_workspace_bytes(int T, int B, int P, int T_proto);
int abcd_warp_nll(const abcd_packed* x, const float* gt_offset, int P, int T_proto, const float* proto_mu,
                  long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                  const double* log_move, int band, int marginal, float* warp, long ld_warp, void* ws,
                  size_t ws_bytes, void* stream);
size_t abcd_warp_path_workspace_bytes(int T, int B, int T_proto);
int abcd_warp_path(const abcd_packed* x, const float* gt_offset, int P, int T_proto, const float* proto_mu,
                   long ld_mu, const float* proto_lv, long ld_lv, const float* proto_offset_logits,
                   const double* log_move, int band, const int32_t* choice, int32_t* state, float* path_em,
                   float* path_off, float* path_move, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Time-warped segmentation: the recording is cut with the
 * prototypes warped inside the dynamic programme.  The state is (category k,
 * prototype step s); inside a category the moves are those of abcd_warp_nll
 * (stay, step, skip, log_move a HOST array of three doubles, -inf disables a
 * move); leaving a category's lattice ends a segment and pays the end-of-segment
 * logit; entering the next one pays abcd_span_chain_viterbi's transition.  x is
 * the recording (N x F, row stride ld_x), the prototypes are the rectangle of
 * abcd_pairwise_nll (T = T_proto steps, K prototypes, row r = s K + k), v[s,k]
 * = proto_offset_logits[s K + k], log_enter[k] floats (NULL: 0), gap,
 * seg_bonus, log_trans, log_init those of abcd_span_chain_viterbi, s_min the
 * lowest state a segment may end in.  In fp64 after widening, every addition as
 * written, sp(u) = max(u,0) + log1p(e^-|u|):
 *   e(n,k,s)  = 0.5 sum_f (log 2pi + lv[s,k,f] + (x[n,f] - mu[s,k,f])^2 e^-lv[s,k,f])
 *               (fp32, the column order of abcd_pairwise_nll)
 *   cont[k,s] = sp(v[s,k])     last[k,s] = sp(-v[s,k])
 *   G[0] = 0, G[n] = G[n-1] + gap[n-1]          (gap NULL: -inf for n >= 1)
 *   W[0][k] = -inf,  H[-1][k][s] = -inf
 *   for frame n = 0 .. N-1:
 *     U[n][k]    = max(G[n] + log_init[k], max_k' (W[n][k'] + log_trans[k' ld_trans + k]))
 *     A[n][k][0] = max(U[n][k] + log_enter[k], H[n-1][k][0] + log_move[0])
 *     A[n][k][s] = max_{m in 0..2, s-m >= 0} (H[n-1][k][s-m] + log_move[m])          s >= 1
 *     H[n][k][s] = (A[n][k][s] - e(n,k,s)) - cont[k,s]                               the segment goes on
 *     X[n+1][k]  = max_{s >= s_min} ((A[n][k][s] - e(n,k,s)) - last[k,s]) + seg_bonus  it ends with frame n
 *     W[n+1][k]  = max(W[n][k] + gap[n], X[n+1][k])
 *   path_score = max(G[N], max_k W[N][k])
 * NaN and -inf candidates are excluded; a NaN or +inf e excludes its cell (H
 * = -inf, no ending); +inf anywhere else is outside the contract.  Ties: in A
 * enter, then stay, step, skip; in X the lowest s; in W the gap against a
 * segment; in U the initial term, then the lowest k'; at the end "no segment",
 * then the lowest k.  Every H cell carries the frame at which its segment was
 * entered; X's winner records that onset and its state per (n + 1, k), W gap or
 * segment, U its k' (-1: the initial term).  There is no per-cell back-pointer
 * plane: a segment's state path comes from abcd_warp_path on the cut segment.
 * The backtrack is abcd_span_chain_viterbi's and runs on the device.  Segments
 * come out in time order, N entries per buffer, n_segments valid: seg_onset,
 * seg_length, seg_cat, seg_last_state, seg_enter (the U[onset][k] the segment
 * was entered from), seg_exit (its X[end][k]) and seg_link (the log_init or
 * log_trans term, widened).  With the step move alone and log_enter = 0 the
 * programme is abcd_span_chain_viterbi with D = T_proto and d_min = s_min + 1.
 *
 * abcd_frame_costs: cost[(n - n0) ld_cost + r] = e(n, r) in fp32 for n0 <= n <
 * n1 and every rectangle row r < T K.  The emission tile of abcd_pairwise_nll
 * with the rectangle's rows as the "prototypes" of one step: 32 frames x 32
 * rows per 256-thread workgroup over a grid of all the tiles.  A pair's bits
 * depend on its frame and its row alone, not on n0, the chunk or the tile
 * position.  No atomics, no device-global word, two calls agree bit for bit.
 * Rows >= N of x, columns >= F and the padding of every stride are never read;
 * nothing outside the (n1 - n0) x T K block is written.  ABCD_EINVAL: the
 * limits below, F < 1, ld_x, ld_mu or ld_lv < F, ld_cost < T K, not 0 <= n0 <
 * n1 <= N, a NULL pointer.
 *
 * abcd_warp_segment_window: frames n0 .. n1 - 1 of the recurrence on such a
 * plane, whose row 0 is frame n0.  The programme is carried across the calls
 * in the workspace, which must not be touched between them; in this order,
 * cells = (N + 1) K and S = K T: U and the chosen X (cells doubles each), W's
 * choice, the onset, the last state and k' (cells int32 each), cont and last
 * (S doubles each, formed by the call with n0 = 0), the two H rows (2 S
 * doubles; H[n] is row n mod 2) with their onsets (2 S int32), W[n1] (K
 * doubles), G[n1] and the next frame (one 64-bit integer).  Calls go in order
 * on ONE stream with the same arguments but cost, n0 and n1; n0 = 0 starts
 * over.  A call whose n0 is not the carried frame runs nothing, writes
 * path_score = NaN and n_segments = -1 and leaves the carry as it is.  The call
 * with n1 = N backtracks and writes the outputs.  W_out ((N + 1) x K doubles,
 * may be NULL) receives rows n0 + 1 .. n1 (row 0 too when n0 = 0).  Any split
 * of 0 .. N into calls gives the one-call outputs bit for bit.
 * One workgroup of 1024 threads.  With R = 1024 / K, thread r K + k owns the
 * states s = r, r + R, ... of category k, as many as K T needs, so consecutive
 * threads touch consecutive s K + k of H, the plane and the logits.  The H
 * rows alternate in the workspace (L2); the workgroup reads its own stores a
 * barrier later.  U splits k' over the same (r, k) grid; log_trans is resident
 * in LDS up to K = 128 and streamed above (abcd_warp_segment_plan says which,
 * with the launch width and the LDS bytes; it is a pure function).  The
 * threads' partial maxima of U and X meet in LDS and thread k joins them in r
 * order under the tie rules.  No atomics, no device-global word, no workgroup
 * waits for another; two sequences of calls agree bit for bit.
 * Limits: 1 <= K <= 1024, 1 <= T_proto <= 16383, K T_proto < 2^24, (N + 1) K <
 * 2^31, (n1 - n0) ld_cost < 2^31; the queries return 0 beyond them.
 * ABCD_EINVAL (on the host before any launch, nothing is written): those
 * limits, ld_cost < K T_proto, ld_trans < K, s_min outside 0 .. T_proto - 1, a
 * NaN or +inf move, all three moves disabled, anything but 0 <= n0 < n1 <= N, a
 * NULL among cost, proto_offset_logits, log_move, log_trans, log_init,
 * path_score, n_segments and the seven segment buffers, a missing or short
 * workspace.  N = 0 (with n0 = n1 = 0) gives path_score = 0, n_segments = 0 and
 * W_out[0][k] = -inf (each where not NULL) and reads nothing.
 *
 * Measured on one MI355X at N = 15 000, K = 128, T_proto = 200, F = 129
 * (profiles/warpseg_bench.json): abcd_frame_costs 5.85 ms (0.39
 * us per frame), abcd_warp_segment_window 787.3 ms on a plane read from HBM
 * (52.5 us per frame), plane and programme chunk by chunk 690.0 ms (46.0 us per
 * frame), against abcd_span_table + abcd_span_chain_viterbi at D = 200 on the
 * same frames, 8.39 + 209.4 ms (13.96 us per step): 3.17 x slower end to end.  The step is bound by
 * latency, not bandwidth: each thread walks 25 cells per frame and each cell
 * waits for its loads from L2 (H, onsets, logits) or HBM (the plane) behind
 * four barriers per frame.  Peak memory 0.33 GB (a 268 MB plane chunk and 62 MB
 * of state) against the table's 3.07 GB.
 *
 * No timing or dispatch id is assigned to these entry points.
 * ---------------------------------------------------------------------- */
int abcd_frame_costs(const float* x, long ld_x, long N, long n0, long n1, int F, int K, int T_proto,
                     const float* proto_mu, long ld_mu, const float* proto_lv, long ld_lv, float* cost, long ld_cost,
                     void* stream);
int abcd_warp_segment_plan(int K, int T_proto, int* resident, int* threads, size_t* lds_bytes);
size_t abcd_warp_segment_workspace_bytes(long N, int K, int T_proto);
int abcd_warp_segment_window(const float* cost, long ld_cost, long n0, long n1, long N, int K, int T_proto,
                             const float* proto_offset_logits, const double* log_move, const float* log_enter,
                             const float* gap, double seg_bonus, const float* log_trans, long ld_trans,
                             const float* log_init, int s_min, double* path_score, int32_t* n_segments,
                             int32_t* seg_onset, int32_t* seg_length, int32_t* seg_cat, int32_t* seg_last_state,
                             double* seg_enter, double* seg_exit, double* seg_link, double* W_out, void* ws,
                             size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Posteriors under the time-warped cut: the sum half of
 * abcd_warp_segment_window.  cost, proto_offset_logits (v),
 * log_move (HOST, three doubles), log_enter, gap, seg_bonus, log_trans,
 * log_init and s_min are those of abcd_warp_segment_window; scale is 1 /
 * temperature and multiplies every term (e, cont, last, log_move, log_enter,
 * gap, seg_bonus, log_trans, log_init) in fp64 after widening, so scale = 1 is
 * exact.  cont[k,s] = sp(v[s,k]) and last[k,s] = sp(-v[s,k]) are formed before
 * the multiplication.  Below every symbol is the multiplied term (lm, le, lt,
 * li, bonus), T = T_proto; a candidate that is NaN or -inf is excluded, a NaN
 * or +inf e excludes its cell in both sweeps; LAE is logaddexp, LSE the
 * log-sum-exp over the admissible candidates, -inf over none:
 *   G[0] = 0,  G[n] = G[n-1] + gap[n-1]                    (gap NULL: -inf for n >= 1)
 *   aW[0][k] = -inf,  aH[-1][k][s] = -inf
 *   n = 0 .. N-1:
 *     aU[n][k]    = LAE(G[n] + li[k], LSE_k' (aW[n][k'] + lt[k'][k]))
 *     aA[n][k][0] = LAE(aU[n][k] + le[k], aH[n-1][k][0] + lm[0])
 *     aA[n][k][s] = LSE_{m in 0..2, s-m >= 0} (aH[n-1][k][s-m] + lm[m])                 s >= 1
 *     aB[n][k][s] = aA[n][k][s] - e(n,k,s)
 *     aH[n][k][s] = aB[n][k][s] - cont[k,s]
 *     aX[n+1][k]  = LSE_{s >= s_min} (aB[n][k][s] - last[k,s]) + bonus
 *     aW[n+1][k]  = LAE(aW[n][k] + gap[n], aX[n+1][k])
 *   aU[N][k] = -inf,  aX[0][k] = -inf
 *   log_z = LAE(G[N], LSE_k aW[N][k])
 *   bW[N][k] = 0,  bG[N] = 0,  bU[N][k] = -inf;   n = N-1 .. 0:
 *     bA[n][k][s] = -e(n,k,s) + LAE( [s >= s_min] (-last[k,s] + bonus + bW[n+1][k]),
 *                                    [n < N-1]    (-cont[k,s] + LSE_{m, s+m < T} (lm[m] + bA[n+1][k][s+m])) )
 *     bU[n][k] = le[k] + bA[n][k][0]
 *     bW[n][k] = LAE(gap[n] + bW[n+1][k], LSE_k'' (lt[k][k''] + bU[n][k'']))
 *     bG[n]    = LAE(gap[n] + bG[n+1], LSE_k (li[k] + bU[n][k]))                        (bG[0] = log_z)
 *   post_k[n K + k]             = exp(aU[n][k] + bU[n][k] - log_z)     a segment of k starts at frame n
 *   post_k[(N + 1) K + n K + k] = exp(aX[n][k] + bW[n][k] - log_z)     a segment of k ends before frame n
 *   gap_post[n]   = exp(LAE(G[n] + bG[n+1], LSE_k (aW[n][k] + bW[n+1][k])) + gap[n] - log_z),  n < N;  [N] = 0
 *   init_counts[k]         = sum_{n < N} exp(G[n] + li[k] + bU[n][k] - log_z)
 *   trans_counts[k' K + k] = sum_{n < N} exp(aW[n][k'] + lt[k'][k] + bU[n][k] - log_z)
 *   move_counts[3 k + m]   = sum_{n <= N-2} sum_{s, s+m < T} exp(aH[n][k][s] + lm[m] + bA[n+1][k][s+m] - log_z)
 * log_z = -inf (no cover) makes every posterior and count 0.  +inf anywhere
 * but in e is outside the contract.
 *
 * The programme lives in the workspace, which must not be touched between the
 * calls of a recording; doubles in this order, cells = (N + 1) K and S = K T:
 * G and bG (N + 1 each), the lattice aU, aX, aW, bU, bW (cells each), cont and
 * last (S each, row s K + k, formed by the forward call with n0 = 0), the two
 * alternating rows of aH (forward) or bA (backward) (2 S; frame n is row n mod
 * 2), the count accumulators (K K bigram, K initial, 3 K move), log_z, and
 * three 64-bit integers: the next frame of the forward sweep, the next n1 of
 * the backward sweep, the status of the last backward call.
 *
 * abcd_warp_posterior_forward: frames n0 .. n1 - 1 ascending on the plane whose
 * row 0 is frame n0; calls go in order on ONE stream with the same arguments
 * but cost, alpha_out, n0 and n1; n0 = 0 starts over.  A call whose n0 is not
 * the carried frame runs nothing, writes log_z = NaN and leaves the carry as it
 * is.  The call with n1 = N writes log_z; no other call writes it.  alpha_out
 * (may be NULL) receives aH[n][k][s] at alpha_out[(n - n0) ld_alpha + s K + k].
 *
 * abcd_warp_posterior_backward: frames n1 - 1 .. n0 descending after the
 * forward sweep has finished, the first call with n1 = N, every next call's n1
 * the previous n0, each on the plane of ITS frames (row 0 = frame n0) and, for
 * move_counts, on the rows alpha_out received for them (row 0 = frame n0).
 * A call out of order (or before the forward sweep is through) runs nothing,
 * changes no lattice entry, count or carried frame and sets the status word to
 * 1; a call in order sets it to 0.  The call with n0 = 0 forms bG, writes
 * post_k (2 (N + 1) K), gap_post (N + 1) and the counts that were asked for:
 * trans_counts (K x K, row stride K) and init_counts (K) together or not at
 * all, move_counts (3 K) only with alpha.  n1 = N starts the sweep over.
 *
 * One workgroup of 1024 threads, abcd_warp_segment_window's grid: with R =
 * 1024 / K thread r K + k owns the states s = r, r + R, ... of category k and
 * the k' = r, r + R, ... of column k.  log_trans is resident in LDS up to K =
 * 128 (K rows of K + 1 floats) and streamed above (abcd_warp_posterior_plan
 * says which, with the launch width and the LDS bytes; it is a pure
 * function).  Every thread keeps a (maximum, sum of exp(c - maximum)) pair per
 * reduction; the pairs of aU, aX and bW's chain term meet in LDS and thread k
 * joins them in r order.  A count entry is owned by one thread and summed in
 * the order the backward sweep visits the frames (a move count: the threads'
 * parts of a frame joined in r order by thread k).  No atomics, no
 * device-global word, nothing is allocated.  Any split of 0 .. N into forward
 * calls and any split into backward calls gives the one-call bits, two runs
 * agree bit for bit, and passing or omitting alpha_out, alpha or the count
 * buffers changes no other output's bits.
 * Limits: those of abcd_warp_segment_window; the workspace query returns 0
 * beyond them.  ABCD_EINVAL (on the host before any launch, nothing is
 * written): those limits and argument rules, scale not finite or not positive,
 * ld_alpha < K T_proto with a plane given, move_counts without alpha, exactly
 * one of the two bigram buffers, a NULL log_z (forward) or post_k / gap_post
 * (backward), a missing or short workspace.  N = 0 (n0 = n1 = 0): the forward
 * call writes log_z = 0, the backward call zero posteriors and counts; neither
 * reads anything nor touches the workspace.
 *
 * Measured on one MI355X at N = 15 000, K = 128, T_proto = 200, F = 129
 * (profiles/warppost_bench.json), the plane read from HBM in
 * 6 chunks: the forward sweep 1218.5 ms (81.2 us per frame; 1228.6 keeping
 * aH), the backward sweep 1518.3 ms without counts (101.2 us per frame),
 * 1626.4 with the bigram counts, 1944.4 with the move counts, 2052.6 with
 * both; segment_warp_posteriors end to end 2668.4 ms (3284.7 with every
 * count), against abcd_warp_segment_window on the same plane in the same
 * process, 785.5 ms: derived, the two sweeps take 3.48 x the best-path
 * programme.  State 78.0 MB; the aH plane of the move counts 3.07 GB.
 *
 * No timing or dispatch id is assigned to these entry points.
 * ---------------------------------------------------------------------- */
int abcd_warp_posterior_plan(int K, int T_proto, int* resident, int* threads, size_t* lds_bytes);
size_t abcd_warp_posterior_workspace_bytes(long N, int K, int T_proto);
int abcd_warp_posterior_forward(const float* cost, long ld_cost, long n0, long n1, long N, int K, int T_proto,
                                const float* proto_offset_logits, const double* log_move, const float* log_enter,
                                const float* gap, double seg_bonus, double scale, const float* log_trans,
                                long ld_trans, const float* log_init, int s_min, double* alpha_out, long ld_alpha,
                                double* log_z, void* ws, size_t ws_bytes, void* stream);
int abcd_warp_posterior_backward(const float* cost, long ld_cost, long n0, long n1, long N, int K, int T_proto,
                                 const float* proto_offset_logits, const double* log_move, const float* log_enter,
                                 const float* gap, double seg_bonus, double scale, const float* log_trans,
                                 long ld_trans, const float* log_init, int s_min, const double* alpha, long ld_alpha,
                                 double* post_k, double* gap_post, double* trans_counts, double* init_counts,
                                 double* move_counts, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Featurisation + packing on the device: replaces the per-item host path
 * Dataset.__getitem__ -> STFT.__call__ -> log_and_normalize -> pack_sequence
 * (data_utils.py:88-103, 124-139, 165-182; learning.py:466-470) for a whole
 * batch.  wave: concatenated fp32 samples (DEVICE); seg_off / seg_len: HOST,
 * one entry per segment in packed (length-descending) order; window: n_fft
 * floats (DEVICE, e.g. torch.hann_window); batch_sizes: HOST, T entries,
 * consistent with the per-segment frame counts.  out: L x (n_fft/2 + 1)
 * packed log-amplitudes log(|STFT| + eps) / norm; is_offset: L (may be NULL),
 * 1 at each segment's last frame.
 * ---------------------------------------------------------------------- */
/* frames torch.stft produces for `length` samples (0 if none) */
int abcd_stft_frames(long long length, int n_fft, int hop, int center);
size_t abcd_featurize_workspace_bytes(int B, int T);
int abcd_featurize_packed(const float* wave, const long long* seg_off, const long long* seg_len, int B, int n_fft,
                          int hop, int center, const float* window, float eps, float norm,
                          const int64_t* batch_sizes, int T, int L, float* out, float* is_offset, void* ws,
                          size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Log-spectra back to audio: the inverse of the featuriser above, phase
 * retrieval by Griffin-Lim (Griffin & Lim 1984; momentum form: Perraudin,
 * Balazs & Sondergaard 2013) run entirely on the device.  The reference has
 * no such path.
 *
 * logamp: packed L x F log-amplitudes (row stride ld >= F = n_fft/2 + 1), what
 * abcd_featurize_packed writes and abcd_decoder_generate returns; phase0: L
 * rows of F radians (row stride ldp >= F), the initial phase; batch_sizes:
 * HOST.  Magnitudes A = max(exp(logamp * norm) - eps, 0).  torch.stft /
 * torch.istft semantics with center = 1: segment b (packed position b, T_b
 * frames) gets S_b = hop (T_b - 1) samples,
 *
 *   C = A exp(i phase0);  R_prev = 0
 *   n_iter times:  y = istft(C);  R = stft(y);  t = R - momentum / (1 + momentum) R_prev;
 *                  R_prev = R;  C = A t / (|t| + 1e-16)
 *   wave[b] = istft(C);  residual[b] = || |stft(wave[b])| - A ||_F / ||A||_F
 *
 * istft: the inverse real DFT of each frame (imaginary parts of the DC and,
 * for even n_fft, Nyquist bins ignored) times the window, overlap-added and
 * divided by the overlap-added squared window (samples where that is < 1e-11
 * become 0), n_fft/2 samples trimmed at the front, S_b kept.  stft: the signal
 * reflect-padded by n_fft/2 in front and n_fft - n_fft/2 behind and framed as
 * abcd_featurize_packed frames it: T_b frames (for odd n_fft the last frame
 * reads one reflected sample more than torch.stft's centre padding holds, which
 * would drop that frame).  n_iter = 0 is the plain inverse STFT of a spectrum
 * with known phase; momentum = 0 is classic Griffin-Lim, 0.99 the fast form.
 *
 * The padding needs S_b > n_fft - n_fft/2: abcd_griffin_lim_samples returns 0
 * for fewer frames than that (or center = 0), and such a segment gets a zero
 * row and residual NaN.  Row b of wave (B rows, stride ldw >= the longest
 * S_b) holds segment b's samples followed by zeros.  residual: B floats or
 * NULL (it costs one more STFT).
 *
 * One launch: one 1024-thread workgroup per segment runs the whole iteration
 * loop with nothing but workgroup barriers between the phases; no atomics, no
 * workgroup waits for another.  The reflect-padded signal stays in LDS for the
 * whole loop wherever it fits beside the window and the twiddle table
 * (S + 4 n_fft floats + 256 bytes <= 160 KiB for the longest segment's S: the
 * switch is computed per call, e.g. at n_fft 256, hop 128 up to T = 312), else
 * in ws; the phasors (scaled by A) and R_prev (T x F complex each per segment)
 * live in ws.  ABCD_GL_LDS=0 in the environment forces the signal into ws
 * (ABCD_GL_WAVES=8 / 4: fewer than 16 waves per workgroup, for A/B timing; the
 * dispatch name then ends in " waves 8").  The DFTs are direct, fp32, with an
 * n_fft-entry twiddle table built in double (any n_fft >= 2, odd included);
 * every sum has a fixed order (the overlap-add is a gather per output sample in
 * frame order), so two calls agree bit for bit and a segment's result does not
 * depend on the rest of the batch.
 * abcd_dispatch_name(16) names the form that ran ("griffin_lim<lds,dft> grid 3
 * lds 106240" / "griffin_lim<global,dft> grid 2 lds 3328": the signal's home,
 * the DFT form, workgroups, LDS bytes); abcd_timing_read_kernel id 16.
 * ABCD_EINVAL (checked before any launch, nothing is written): center = 0
 * (a Hann window violates the overlap-add condition at the edges there),
 * ld or ldp < F, ldw too short, a NULL window / logamp / phase0 / wave, a
 * missing or short workspace, n_iter < 0, momentum outside [0, 1), norm = 0,
 * T > 16383, a batch_sizes abcd_segment_losses rejects, an n_fft whose tables
 * alone exceed the LDS.
 * abcd_griffin_lim_workspace_bytes is 0 for unsupported sizes.
 * ---------------------------------------------------------------------- */
int abcd_griffin_lim_samples(int frames, int n_fft, int hop, int center); /* S_b, 0 if too short */
size_t abcd_griffin_lim_workspace_bytes(int B, int T, int n_fft, int hop);
int abcd_griffin_lim(const float* logamp, int ld, const int64_t* batch_sizes, int T, int L, int B, int n_fft, int hop,
                     int center, const float* window, float eps, float norm, const float* phase0, int ldp,
                     int n_iter, float momentum, float* wave, int ldw, float* residual /* B or NULL */, void* ws,
                     size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Optimiser: torch.nn.utils.clip_grad_norm_ + torch.optim.SGD
 * (learning.py:161-163, 256) over one flat fp32 parameter/gradient buffer.
 * ---------------------------------------------------------------------- */
size_t abcd_optim_workspace_bytes(long n);
/* The norm's last-block hand-over uses one device-wide ticket word (as do the
 * sampler-head kernels of abcd_sampler_forward_fused / abcd_sampler_backward*):
 * launches of these entry points on one device must not run concurrently on
 * different streams (the training step queues them on one stream). */
/* total 2-norm of g (device scalar) */
int abcd_grad_norm(const float* g, long n, float* out_norm, void* ws, size_t ws_bytes, void* stream);
/* g *= min(1, max_norm / (||g|| + 1e-6)); buf = momentum*buf + g (buf = g if
 * momentum_init); p -= lr * (momentum ? buf : g).  out_norm (device, may be
 * NULL) receives the pre-clip norm. */
int abcd_clip_sgd(float* p, float* g, float* momentum_buf, long n, float max_norm, float lr, float momentum,
                  int momentum_init, float* out_norm, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Utilities
 * ---------------------------------------------------------------------- */
/* loss = (losses[0] + losses[1] + kl[0]) / B  (learning.py:155-157) */
int abcd_total_loss(const float* losses, const float* kl, int B, float* loss, void* stream);
/* C = A(MxK) @ B(NxK)^T (+bias[n]); row-major, plain GEMM used by tests */
int abcd_gemm_nt(int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                 const float* bias, void* ws, size_t ws_bytes, void* stream);
/* C = A^T @ B, A K x M (lda >= M), B K x N (ldb >= N), row-major: the
 * weight-gradient GEMM (reduction over packed frames); ws enables split-K
 * (>= 16 * M * N * 4 bytes recommended) */
int abcd_gemm_tn(int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                 void* ws, size_t ws_bytes, void* stream);
/* y = act(x @ W^T + b): nn.Linear (act 0) / Linear->Tanh (act 1); x M x K, W N x K.
 * Used by the standalone MLP modules (model.py:316-334) outside the training step;
 * ws >= (M + N) * roundup(K,16) * 4 bytes when K is not a multiple of 16. */
int abcd_linear(int M, int N, int K, const float* x, long ldx, const float* W, long ldw, const float* b, int act,
                float* y, long ldy, void* ws, size_t ws_bytes, void* stream);
/* backward of abcd_linear (the standalone MLP's training path, model.py:316-334):
 * dy' = dy (act 0) or dy (1 - y^2) (act 1, y = the forward's output);
 * dx = dy' W (M x K, may be NULL), dW = dy'^T x (N x K, row stride K, may be
 * NULL), db = column sums of dy' (N, may be NULL).  Any M, N, K. */
size_t abcd_linear_backward_workspace_bytes(int M, int N, int K);
int abcd_linear_backward(int M, int N, int K, const float* x, long ldx, const float* W, long ldw, const float* y,
                         long ldy, int act, const float* dy, long lddy, float* dx, long lddx, float* dW, float* db,
                         void* ws, size_t ws_bytes, void* stream);
/* n standard normals from Philox-4x32-10(seed, offset + i) */
int abcd_fill_normal(float* out, long n, uint64_t seed, uint64_t offset, void* stream);
/* dropout noise bernoulli(1 - p) / (1 - p) from the same Philox stream */
int abcd_fill_dropout(float* out, long n, float p, uint64_t seed, uint64_t offset, void* stream);
/* live device timing of the recurrent kernel family (encoder and decoder,
 * persistent or per-step): HIP events around every launch while enabled;
 * read: out[0] = summed device ms, out[1] = number of launches */
void abcd_timing_enable(int on);
void abcd_timing_reset(void);
int abcd_timing_read(double* out);
/* the same for one kernel: 0 per-step recurrent kernels, 1 encoder forward,
 * 2 encoder backward, 3 decoder forward, 4 decoder backward (persistent) */
int abcd_timing_read_kernel(int kid, double* out);
/* which kernel the last launch of a role ran (same ids as abcd_timing_read_kernel,
 * 5 / 6 the sampler head forward / backward, 7 the encoder's layer-0 weight
 * gradients; e.g. "dec_bwd_sk<9,16,16,LSTM> grid 256" or "per-step ..."), and how many
 * launches of the role since abcd_dispatch_reset; host-side bookkeeping only.
 * An id outside the table reads as "" / -1; so does 15, which stays unassigned
 * (it was the first id out of range before the table grew, and callers probe it). */
const char* abcd_dispatch_name(int kid);
long abcd_dispatch_count(int kid);
void abcd_dispatch_reset(void);
/* how that launch dealt its 16-row blocks to the row groups (persistent
 * recurrent kernels, ids 1 .. 4): 1 cyclic (block j of group g is packed block
 * g + groups * j), 0 contiguous (also every launch without a deal: per-step
 * kernels, the other ids); -1: no launch of the role since the reset, or an id
 * outside the table.  Environment ABCD_PERSIST_DEAL (read per call): a mask of
 * 1 enc fwd, 2 enc bwd, 4 dec fwd, 8 dec bwd that deal cyclically; 0: none. */
int abcd_dispatch_deal(int kid);
/* diagnostics (scripts/, not part of the reference's interface):
 * abcd_debug_persist_prof -- the persistent kernels of the roles in `mask`
 * (1 enc fwd, 2 enc bwd, 4 dec fwd, 8 dec bwd) stamp s_memrealtime at their
 * phase boundaries into dev_buf (blocks x T x 8 u64; null: off); 16 / 32:
 * the sampler-head forward / backward kernels (tiles x 8 u64);
 * abcd_debug_xcc_map -- launches `blocks` one-per-CU workgroups that record
 * their (XCC id, HW_ID) pair into dev_out[2 * block], dev_out[2 * block + 1]
 * (dev_out holds 2 * blocks u32; the placement the persistent kernels' group
 * roles rely on).  Returns 0 / a HIP error;
 * abcd_debug_gemm_route -- names what the calling thread's last GEMM
 * dispatch (abcd_gemm_nt / abcd_gemm_tn / abcd_linear / the products of
 * abcd_linear_backward, and every GEMM inside the other entry points)
 * launched: "x6r8<5,128>", "x6r8<5,128,t16>", "x6r8<8,64>", "x6f", "x6t",
 * "x6s<4,5>", "x6s<4,4,kc>", "x6s<5,4,one>", "tn<4,8,kc>", "ks", "big"; where
 * split-K ran, " z=<Z> <reduce>" follows with the slab reduction's form
 * (zg4, zg16, vec, scalar), and the un-split gemm_ks reads "ks z=1".  "" before
 * the first dispatch.  The string is thread-local and valid until the
 * thread's next dispatch; each launch stores the name's pointer (and the
 * slab count) on the host, no device work;
 * abcd_debug_gemm_side -- sets (on != 0) or clears the calling thread's
 * side-stream GEMM mode, the one the training step enters beside a
 * persistent recurrent kernel: abcd_gemm_nt / abcd_gemm_tn then take the
 * small-footprint routes.  For tests; nothing in the training path calls
 * either;
 * abcd_debug_offset_head_fwd -- the decoder's fused offset head forward on
 * the caller's buffers, as the decoder forward runs it: Zo = tanh(Hs W1o^T +
 * b1o) (M x N at stride N; Hs M x K at stride ldh, W1o N x K) with part[m *
 * nsl + slice] = the 64-column slice's share of Zo . w2 (nsl = ceil(N / 64)),
 * then logit = sum of the partials in slice order + b2[0] and, with tgt,
 * bce / dlog_raw (tgt NULL: neither is touched).  *fused_out = 1 when the
 * fused form ran ("x6r8<8,64,offset_fwd>"); 0 when it declines (K > 256, K % 8,
 * N % 4, ldh % 4, Hs / W1o / Zo not 16-B aligned, Hs or W1o of 2 GiB or
 * more): nothing is launched;
 * abcd_debug_offset_head_bwd -- its backward: dlog_s = s_off[0] dlog_raw,
 * dZo = dlog_s w2 (1 - Zo^2) (M x K at stride K) and DHO = dZo W1oT^T (M x N
 * at stride N; W1oT N x K), "x6r8<8,64,offset_bwd>"; *fused_out as above
 * (it declines on the same conditions, DHO and dZo for Zo, and also where a
 * workgroup's row range is so long that its LDS request passes 160 KiB:
 * more than 7424 rows per range, M above about 118000 at 16 slices);
 * abcd_debug_gemm_tn_batch -- up to 8 jobs C_j = alpha_j A_j^T B_j + beta_j
 * C_j (A_j K x M at stride lda, B_j K x N at stride ldb) in the one launch
 * the sampler backward uses (abcd_debug_gemm_route then reads
 * "tn_batch<1,1,64>", or "tn_batch<2,2,16>" in side mode: the instance the
 * launcher started); the job fields as arrays of n.  A job with M or
 * N = 0 is skipped; n > 8, M % 4, N % 4, lda % 4, ldb % 4 or an A / B not
 * 16-B aligned return an error before any launch;
 * abcd_debug_colsum_batch -- up to 8 jobs out_j[c] = beta_j out_j[c] + sum_r
 * w_j[r] Z_j[r * ldz + c] (w_j NULL: 1; out2_j, optional, receives the same)
 * in the decoder backward's two launches; scratch holds every job's partial
 * sums and clamps their slice counts; too little of it for a job's one slice
 * returns an error before any launch.
 * All four are host-only wrappers that launch existing kernels under the
 * launchers' own preconditions and return ABCD_EINVAL on null or negative
 * arguments.  For tests; nothing in the training path calls them. */
void abcd_debug_persist_prof(unsigned long long* dev_buf, int mask);
const char* abcd_debug_gemm_route(void);
void abcd_debug_gemm_side(int on);
int abcd_debug_offset_head_fwd(int M, int N, int K, const float* Hs, long ldh, const float* W1o, const float* b1o,
                               const float* w2, const float* b2, const float* tgt, float* Zo, float* part,
                               float* logit, float* dlog_raw, float* bce, int* fused_out, void* stream);
int abcd_debug_offset_head_bwd(int M, int N, int K, const float* Zo, const float* W1oT, const float* w2,
                               const float* dlog_raw, const float* s_off, float* DHO, float* dZo, float* dlog_s,
                               int* fused_out, void* stream);
int abcd_debug_gemm_tn_batch(int n, const float* const* A, const long* lda, const float* const* B, const long* ldb,
                             float* const* C, const long* ldc, const int* M, const int* N, const int* K,
                             const float* alpha, const float* beta, void* stream);
int abcd_debug_colsum_batch(int n, const float* const* Z, const long* ldz, const int* nrows, const int* ncols,
                            const float* const* w, float* const* out, const float* beta, float* const* out2,
                            float* scratch, size_t scratch_floats, void* stream);
/* Side-stream gate (per calling host thread, default off): read by a deferred
 * abcd_decoder_backward_dropout(..., ABCD_DEFER_PARAMS).  The first encoder
 * BPTT this thread launches persistently after it becomes the gate's target,
 * and the abcd_decoder_backward_params call that follows queues, in front of
 * its side-stream work, a wait (on the device, bounded) until every workgroup
 * of that launch is resident -- without it the side GEMMs can take a CU's
 * room before a BPTT member is placed there.  No persistent BPTT in between
 * (a per-step encoder backward): no wait.  The wait is queued after the
 * BPTT's launch, so a side stream that shares the BPTT's hardware queue
 * cannot hold the BPTT back. */
void abcd_side_gate_enable(int on);
int abcd_debug_xcc_map(unsigned* dev_out, int blocks, void* stream);
/* 0 if no persistent recurrent kernel has timed out waiting for its group
 * since the last call (a timeout means the grid was not co-resident; the
 * results of that launch are invalid).  Reads and clears the device word;
 * synchronises the device.  Returns -1 on a HIP error. */
int abcd_device_status(void);
/* stream-ordered form for the training step (no host sync): out[0] = the
 * timeout status raised since the previous call (0 ok, 1 a persistent kernel's
 * hand-off wait timed out, 2 a side-stream gate timed out; non-zero means
 * that step's results are invalid), then clears it.  The trainer and bench.py
 * raise on a non-zero value. */
int abcd_step_status(float* out, void* stream);
/* library build identification (gfx target, version) */
const char* abcd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ABCD_HIP_H */
