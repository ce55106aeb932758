/* gicap.h - C ABI of libgicap.so: hand-written HIP (gfx950 / MI355X) kernels for the
 * adversarial image-captioning train step.
 *
 * The reference (kawshik8/GAN-Image-Captioning) has no FFI: its boundary for this
 * path is the Python module API consumed by src/training.py.  Each entry point below
 * therefore cites the reference interface whose compute it replaces (file:line under
 * /root/reference/); the Python host in gan-image-captioning_amd/ keeps the module
 * API and binds these symbols with ctypes.
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is DEVICE memory unless named host_*.
 *  - the caller owns every buffer (parameters, outputs, saved-for-backward state,
 *    workspaces); the library allocates nothing and keeps no global state except
 *    the thread-local last-error string.
 *  - every function enqueues on `stream` (a hipStream_t passed as void*) and returns
 *    immediately: 0 = OK, negative = gic_status.  No exceptions, no exit().
 *  - dtype: GIC_F32 (parity mode; exact-f32 MFMA) or GIC_BF16 (bf16 MFMA operands,
 *    f32 accumulation, f32 master weights / grads / optimizer state).
 *    "act" buffers below have the compute dtype; everything else is f32.
 */
#ifndef GICAP_H_
#define GICAP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GIC_ABI_VERSION 5
#define GIC_MAX_LAYERS 4
#define GIC_MAX_CONVS 8

enum gic_status {
  GIC_STATUS_OK = 0,
  GIC_STATUS_INVALID_ARG = -1,
  GIC_STATUS_UNSUPPORTED = -2,
  GIC_STATUS_LAUNCH = -3,
  GIC_STATUS_WORKSPACE = -4
};
enum gic_dtype { GIC_F32 = 0, GIC_BF16 = 1 };
enum gic_loss_type {           /* src/utils.py:10-53 */
  GIC_LOSS_STANDARD = 0, GIC_LOSS_JS = 1, GIC_LOSS_KL = 2, GIC_LOSS_HINGE = 3, GIC_LOSS_TV = 4, GIC_LOSS_RSGAN = 5
};

int gic_abi_version(void);
/* Message of the last failing call on this host thread ("" if none). */
const char* gic_last_error(void);

/* (ABI v5) Route-only mode, a per-thread debugging switch: while it is on, gic_gemm, every convolution entry point that goes through the
 * GEMM dispatch (gic_conv2d, gic_conv2d_bn_in, gic_conv1x1_bn_in_stats, gic_conv1x1_res_in), the fused vocabulary product and gic_conv_b2b
 * validate their arguments, select a kernel and return the status they would return -- GIC_STATUS_UNSUPPORTED included -- WITHOUT touching
 * the GPU (pointers are only checked for null and alignment).  gic_debug_last_route() is this thread's last selection as one line: the
 * kernel with its template arguments, grid, block, dynamic LDS bytes and, for the 4-wave kernel, splits / per / pipe, e.g.
 * "tile8<bf16,128,2,true,2,true,false,1024> grid=1568 block=512 lds=0"; "unsupported" when nothing was selected.
 * The sequence discriminator's entry points honour it too: gic_disc_fwd answers with the selection of its highway product; gic_disc_bwd,
 * gic_disc_bwd_cond and gic_disc_fwd_redrop validate, select their own kernels (gic_debug_disc_plan prints that selection) and return
 * their status without a launch, the route line left as it was.
 * So do the LSTM decoder's passes and the attention decoder's roll-out: gic_decoder_sample_fwd, gic_decoder_sample_bwd, the teacher-forced
 * entries (gic_decoder_forward_tf / _ss / _tf_bwd and their _drop and gic_attn_ twins) and gic_attn_rollout validate, select
 * (gic_debug_decoder_plan prints that selection) and launch, fill and copy nothing.  What they leave as the route line is, as ever, the
 * last product they select: none on the fused paths of gic_decoder_sample_fwd and in the backward entries (they return before their first
 * product: the line stays as it was); on the generic roll-out paths and in gic_attn_rollout the last step's vocabulary product (the
 * steps are walked over host_active_rows: the tile8 kernel with the Gumbel-max epilogue where the step took it); in the teacher-forced
 * forwards the logits product -- the projection, or scheduled sampling's per-step product, or the recurrence's product with
 * " ss_logits=fused" behind it where the vocab_step_logits kernel takes that product's place.  The step kernels' own launchers answer
 * with their plan (gic_debug_step_plan's line). */
void gic_debug_route_only(int on);
const char* gic_debug_last_route(void);
/* Host-only: what the selection answers the library's own weight-gradient call sites (dW = dy^T x with the bias gradient as the column
 * sums of dy) for a product of these operands: the tile width (64 | 128) of the 4-wave kernel that folds the column sums of A into the
 * product -- a second output matrix may start at any multiple of it --, or 0: the product runs as ever and the separate column-sum pass
 * stays (f32 operands, k-contiguous or unaligned operands, leading dimensions that are no whole 16-byte chunks, the deterministic mode).  Never touches
 * the GPU; the pointers are only looked at for their alignment. */
int gic_debug_wgrad_fold(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb, int a_kc, int b_kc, int in_dtype,
                         int out_dtype);
/* How many weight-gradient products this process has launched in that folding form since the library was loaded, and how many of them
 * wrote two output matrices (dW_ih | dW_hh as one product): what a test reads before and after a call to see which route it took. */
void gic_debug_wgrad_launches(int64_t* launches, int64_t* two_matrix);
/* gic_gemm (below) with the descriptor fields that only the library's own call sites set, so that a test can run them in isolation:
 *   c_zeroed  the caller guarantees that C is all zero: a split-K launch skips its zero fill
 *   no_split  K is never split: the same bits on every call, in or out of the deterministic mode
 *   wgrad     != 0: the weight-gradient extras follow; 0: they are not looked at (and not set in the descriptor)
 *   a_sum, a_sum2   [M] f32, a_sum[m] (+)= sum_k A(m,k), a_sum2 (optional) the same values; OPTIONAL: written only where the product runs
 *                   in the folding form (the route line then ends in " a_sum=.. n_split=.."), left untouched otherwise
 *   C2, ldc2, n_split   the columns n >= n_split go to C2[m * ldc2 + (n - n_split)] instead of C; GIC_STATUS_UNSUPPORTED where the
 *                   selection cannot honour it (n_split off the tile boundary, at 0 or at N; f32, k-contiguous or unaligned operands;
 *                   c_zeroed; the deterministic mode)
 * Goes through the same dispatch as gic_gemm, route-only mode included; no selection logic of its own. */
int gic_debug_gemm_desc(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int a_kc, int b_kc,
                        int in_dtype, int out_dtype, const float* bias, int accumulate, float alpha, int c_zeroed, int no_split, int wgrad,
                        float* a_sum, float* a_sum2, void* C2, int64_t ldc2, int n_split, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-step scalars resident in DEVICE memory (ABI v3).  The values that change from one train step to the next -- the decoder's
 * temperature (src/training.py:183, 190-191: updated after every batch) and the seeds of the device noise streams (Gumbel uniforms,
 * src/generator.py:86-90; the three dropout draws, src/discriminator.py:58) -- can be read by the kernels from this struct instead
 * of being passed by value: the launch arguments of a whole step then never change, which is what lets the step be ONE replayed
 * hipGraph.  Entry points that take a `dev_scalars` pointer ignore their by-value `temperature` / `seed` when it is non-NULL and
 * read dev_scalars->temperature / dev_scalars->seed[seed_slot] on the device.  gic_step_scalars_set enqueues a one-thread kernel
 * that writes *dev from the host values (captured by value at the call: no pinned staging buffer to keep alive). */
#define GIC_STEP_SEEDS 6
typedef struct gic_step_scalars {
  float temperature;
  uint32_t reserved;
  uint64_t seed[GIC_STEP_SEEDS];
} gic_step_scalars;
int gic_step_scalars_set(gic_step_scalars* dev, const gic_step_scalars* host_values, void* stream);

/* ------------------------------------------------------------------------------------------
 * Generic dense contraction (used by the tests and by every entry point below).
 *   C[m,n] = alpha * sum_k A(m,k) B(n,k) + bias[n]  (+ C if accumulate)
 *   A(m,k) = a_kc ? A[m*lda+k] : A[k*lda+m];  B(n,k) = b_kc ? B[n*ldb+k] : B[k*ldb+n]
 * M = 0 or N = 0: GIC_OK, nothing is done.  K = 0: the sum is empty, C = bias (+ C if accumulate) (0 where bias is NULL); A and B
 * must be non-NULL but are never read.
 * Replaces the ATen GEMMs behind nn.Linear / nn.LSTM / autograd (generator.py:61,68;
 * discriminator.py:40,53,58,60).
 */
int gic_gemm(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
             int a_kc, int b_kc, int in_dtype, int out_dtype, const float* bias, int accumulate, float alpha,
             void* stream);

/* 2-D copy with dtype conversion: dst[r*ldd + c] = src[r*lds + c]. */
int gic_cast2d(const void* src, int src_dtype, int64_t lds, void* dst, int dst_dtype, int64_t ldd,
               int64_t rows, int64_t cols, void* stream);

/* ------------------------------------------------------------------------------------------
 * Generator: Decoder.sample (src/generator.py:55-96) forward + backward.
 */
typedef struct gic_decoder_dims {
  int32_t B, L, V, E, H, NL;   /* batch, max_caption_len, vocab, gen_embed_dim, gen_hidden_dim, gen_num_layers */
  int32_t dtype;               /* compute dtype */
} gic_decoder_dims;

typedef struct gic_decoder_params {      /* f32 master weights, state-dict layout of nn.Embedding/nn.LSTM/nn.Linear */
  const float* embed;                    /* decoder.embed.weight            [V,E]      */
  const float* w_ih[GIC_MAX_LAYERS];     /* decoder.lstm.weight_ih_l{k}     [4H,Din_k] */
  const float* w_hh[GIC_MAX_LAYERS];     /* decoder.lstm.weight_hh_l{k}     [4H,H]     */
  const float* b_ih[GIC_MAX_LAYERS];     /* decoder.lstm.bias_ih_l{k}       [4H]       */
  const float* b_hh[GIC_MAX_LAYERS];     /* decoder.lstm.bias_hh_l{k}       [4H]       */
  const float* w_out;                    /* decoder.linear.weight           [V,H]      */
  const float* b_out;                    /* decoder.linear.bias             [V]        */
} gic_decoder_params;

typedef struct gic_decoder_grads {       /* f32, same shapes as gic_decoder_params; all overwritten */
  float* embed;
  float* w_ih[GIC_MAX_LAYERS];
  float* w_hh[GIC_MAX_LAYERS];
  float* b_ih[GIC_MAX_LAYERS];
  float* b_hh[GIC_MAX_LAYERS];
  float* w_out;
  float* b_out;
  float* features;                       /* d(features) [B,E] */
} gic_decoder_grads;

/* Derived per-step weight images in the compute dtype (caller-owned, refreshed by gic_decoder_prepare). */
typedef struct gic_decoder_shadow {
  void* wcat[GIC_MAX_LAYERS];            /* act [4H, Din_k+H] = [w_ih | w_hh] */
  float* bsum[GIC_MAX_LAYERS];           /* [4H] = b_ih + b_hh */
  void* wout;                            /* act [V,H] (may alias params.w_out in f32 mode) */
  void* wcat_t[GIC_MAX_LAYERS];          /* act [Din_k+H, 4H] = Wcat^T, the k-contiguous operand of the BPTT input-gradient
                                            product (the fused BPTT step kernel needs it); NULL: that product reads Wcat
                                            transposed instead, one generic product + one pointwise launch per step */
} gic_decoder_shadow;

/* Saved-for-backward state + scratch of one sample() call (caller-owned). Din_0=E, Din_k=H. */
typedef struct gic_decoder_state {
  void* xh[GIC_MAX_LAYERS];              /* act [(L+1), B, Din_k+H]: LSTM input | previous hidden, time-major */
  float* gates[GIC_MAX_LAYERS];          /* [L, B, 4H] post-activation i,f,g,o */
  float* c[GIC_MAX_LAYERS];              /* [(L+1), B, H] cell state, slot 0 = zeros */
  void* hout;                            /* act [B, L, H] last layer's h, batch-major (vocab GEMM operand) */
  float* logits;                         /* scratch [B, V] */
  float* gpre;                           /* scratch [B, 4H] */
  float* part;                           /* scratch of the fused step kernels: [2][L][B][ceil(V/64)] per-tile softmax partials (max, sum of
                                            exp) + [L][B] 64-bit argmax keys + two reserved 32-bit words; size from gic_decoder_state_bytes,
                                            8-byte aligned.
                                            NULL selects the unfused launches. */
} gic_decoder_state;

typedef struct gic_decoder_bwd_ws {      /* scratch for backward (caller-owned) */
  void* dlogits;                         /* act [B, L, V] */
  float* dhout;                          /* [B, L, H] */
  void* dgates[GIC_MAX_LAYERS];          /* act [L, B, 4H] */
  float* dxh[GIC_MAX_LAYERS];            /* [(L+1), B, Din_k+H] */
  float* dc[GIC_MAX_LAYERS];             /* [B, H] */
} gic_decoder_bwd_ws;

/* Byte size of every buffer of the caller-owned structs above for `dims`, in field order (per-layer arrays take GIC_MAX_LAYERS
 * entries, 0 for unused layers): gic_decoder_state -> xh[], gates[], c[], hout, logits, gpre, part (3*GIC_MAX_LAYERS + 4 values);
 * gic_decoder_bwd_ws -> dlogits, dhout, dgates[], dxh[], dc[] (2 + 3*GIC_MAX_LAYERS values).  Host-only: no GPU needed. */
int gic_decoder_state_bytes(const gic_decoder_dims* dims, uint64_t* out);
int gic_decoder_bwd_ws_bytes(const gic_decoder_dims* dims, uint64_t* out);

int gic_decoder_prepare(const gic_decoder_dims* dims, const gic_decoder_params* params,
                        const gic_decoder_shadow* shadow, void* stream);

/* Optional arguments of gic_decoder_sample_fwd (NULL = none). */
typedef struct gic_decoder_sample_opts {
  const float* h0;                       /* [NL,B,H] initial hidden state: sample(features, states=(h0, c0)), generator.py:55,61; NULL = zeros */
  const float* c0;                       /* [NL,B,H] initial cell state; NULL = zeros */
  const int64_t* force_ids;              /* [B,L] trajectory to FOLLOW: where forced, step t feeds embed(force_ids[b,t]) to step t+1 and
                                            returns it in ids (out is computed as usual).  Prefixes of Monte-Carlo roll-outs; parity tests. */
  const int32_t* force_len;              /* [B] number of leading steps that are forced per caption; NULL = all L */
  int32_t no_state;                      /* != 0: inference roll-out -- nothing is saved for a backward pass: state->gates / hout and
                                            `out` may be NULL (ids only) */
  /* Resumed roll-outs (Monte-Carlo completions of prefixes of ONE sampled batch; generic-product path, i.e. more rows than the fused
   * step kernels take): a row does not recompute its forced prefix.  Row r starts at step force_len[r] (>= 1) from the recurrent state
   * that the call which filled `resume_from` (same weights; caption r % resume_B; the same forced tokens) had reached there.  Rows must
   * be sorted by force_len ascending; host_active_rows[t] (HOST memory, L values) = number of rows with force_len <= t. */
  const struct gic_decoder_state* resume_from;
  int32_t resume_B;
  const int32_t* host_active_rows;
  /* device-resident temperature and Philox seed (gic_step_scalars above; fused step kernels only: GIC_STATUS_UNSUPPORTED where
   * gic_debug_decoder_plan's forward path is not FUSED) */
  const gic_step_scalars* dev_scalars;
  int32_t seed_slot;
} gic_decoder_sample_opts;

/* features [B,E] f32.  noise_u: explicit U[0,1) draws [L,B,V] f32 (generator.py:86-90 order) or NULL to
 * draw on device with Philox(seed, step).  pretrain != 0: generator.py:63-66 (out = raw logits, feedback =
 * argmax).  out: act [B,L,V] (probabilities or logits).  ids: int64 [B,L].
 * With state->part set and V % 4 == 0, E % 8 == 0, H % 8 == 0 a step is two fused launches (gates product + LSTM cell;
 * vocabulary product + Gumbel + per-tile softmax partials) and the probabilities are normalised by one launch at the end. */
int gic_decoder_sample_fwd(const gic_decoder_dims* dims, const gic_decoder_params* params,
                           const gic_decoder_shadow* shadow, const gic_decoder_state* state,
                           const float* features, const float* noise_u, uint64_t seed, float temperature,
                           int pretrain, void* out, int64_t* ids, const gic_decoder_sample_opts* opts, void* stream);

/* Tools only (tools/rollout_bench.py): phase-ablation mask of the fused step kernels; 0 = normal operation. */
void gic_debug_decoder_step(int mask);

/* Which roll-out path gic_decoder_sample_fwd takes for `dims` (host-only, no GPU needed): *out_rows = the largest batch B the fused
 * step kernels take for these V / E / H / NL (GIC_FUSED_ROLLOUT_MAX_ROWS, default 512), or 0 when they decline the shapes
 * (V % 4, E % 8, H % 8, GIC_NO_FUSED_ROLLOUT).  A call with B beyond that, with state->part == NULL or with opts->resume_from runs
 * the generic products and NEEDS state->logits and state->gpre; a caller that sizes its buffers by this query never trips that check
 * (Decoder.sample, src/generator.py:55-81, takes any vocabulary / embedding size). */
int gic_decoder_fused_rollout_rows(const gic_decoder_dims* dims, int32_t* out_rows);

/* (an addition to ABI v5) Host-only: what gic_decoder_sample_fwd and gic_decoder_sample_bwd select for these dims (csrc/decoder_step.h
 * select_decoder_fwd / select_decoder_bwd, the library's very selection), as '\n'-terminated lines written to out (out_len bytes, the
 * terminating 0 included).  "forward path=FUSED | GENERIC | GENERIC_ROWKEY from=<rows>" (from: the rows from which a GENERIC_ROWKEY step's
 * vocabulary product carries the Gumbel-max, 0 = never), then one line per distinct launch of the roll-out's steps in launch order, as in
 * gic_debug_last_route -- kernel<template args> grid= block= lds= (the step kernels: KC= too; products: their gemm / tile8 line and
 * M= N= K=) -- with " x<count>", the launches of that line per call (layers above the first share a line).  With GIC_DECODER_PLAN_TRAIN,
 * "backward path=FUSED | GENERIC" and the backward's lines follow: softmax_bwd's variant, lstm_bwd_step's chain or the pointwise kernel and
 * the per-layer products, then per layer the weight gradient as one folded product or two and "colsum" (the output layer's two products
 * are gic_gemm's business).  Slot 0's fills and casts, the copies of a resumed roll-out and the embedding scatter are not listed.
 * A resumed roll-out's steps run over host_active_rows[t] <= B rows: the lines are those of a step with all B rows, the last step's
 * upper bound; gic_decoder_sample_fwd in route-only mode walks a call's own rows.  The deterministic mode is the library's current one.
 * GIC_STATUS_UNSUPPORTED with gic_decoder_sample_fwd's message: GIC_DECODER_PLAN_DEV_SCALARS off the fused path. */
#define GIC_DECODER_PLAN_TRAIN 1             /* out and the saved state are there and a backward follows; else an ids-only roll-out */
#define GIC_DECODER_PLAN_PRETRAIN 2          /* pretrain != 0 */
#define GIC_DECODER_PLAN_DEV_SCALARS 4       /* opts->dev_scalars */
#define GIC_DECODER_PLAN_RESUMED 8           /* opts->resume_from */
#define GIC_DECODER_PLAN_NO_PART 16          /* state->part == NULL */
#define GIC_DECODER_PLAN_NO_WCAT_T 32        /* the last layer's shadow->wcat_t is NULL */
#define GIC_DECODER_PLAN_STATE_GRADS 64      /* phases has GIC_DECODER_BWD_STATE_GRADS */
#define GIC_DECODER_PLAN_LOGITS_UNALIGNED 128 /* state->logits is 4-byte, not 8-byte aligned */
int gic_debug_decoder_plan(const gic_decoder_dims* dims, int flags, char* out, int64_t out_len);
/* Host-only: the launch plan of one fused step kernel as one line.  lstm != 0: lstm_step's variant 0 plain | 1 packed rows | 2 beam over
 * B rows, H units and input rows of ldx_or_V values; else vocab_step's variant 0 sample | 1 logits | 2 beam | 3 beam + ban lists | 4 beam +
 * ban + hop lists (K: the beam width) over B rows, H units and ldx_or_V words. */
int gic_debug_step_plan(int lstm, int variant, int dtype, int B, int H, int64_t ldx_or_V, int K, char* out, int64_t out_len);

/* Beam-search caption decode (the reference's unbuilt evaluation step; no sampling noise, no temperature: sample(pretrain=True)'s
 * distribution).  dims->B = images, dims->L = maximum caption length.  Rows = B * beam (row r = image r / beam, beam r % beam).
 * Step 0 feeds `features` [B,E] with (h0, c0) (zeros when NULL), every later step embed(token) of the beam's previous token from its
 * PARENT's state.  Token log-probability = logit - logsumexp(logits), the score is the running f32 sum.  Only beam 0 is live at step 0.
 * A live beam proposes its top-`beam` tokens by raw logit (ties to the lower id); a finished beam (it emitted eos_id) proposes itself
 * once, with pad_id and its score unchanged; per image the best `beam` of these candidates are kept (ties to the lower (parent beam,
 * rank)).  The search stops after L steps or once every beam of every image has finished.  A beam's length counts the tokens up to and
 * including its eos_id (L if none).  Outputs, beams sorted by score / length^length_penalty (descending, ties to the lower beam index):
 * ids int64 [B,beam,L] (pad_id after eos_id), scores f32 [B,beam] (raw sums), lengths int32 [B,beam].  No f32 atomics: two calls on the
 * same inputs give the same bits.  The fused step kernels run where gic_decoder_fused_rollout_rows admits B * beam rows, else the
 * generic products (any V). */
typedef struct gic_decoder_beam_opts {
  int32_t beam;                          /* 1..8 (and <= V) */
  int32_t eos_id;                        /* [0, V); <E> = 2 */
  int32_t pad_id;                        /* [0, V); <PAD> = 0 */
  float length_penalty;                  /* alpha of the final order; 0 = raw scores */
  const float* h0;                       /* [NL,B,H] initial hidden state or NULL = zeros */
  const float* c0;                       /* [NL,B,H] initial cell state or NULL = zeros */
} gic_decoder_beam_opts;
/* Bytes of the (256-byte aligned) workspace of gic_decoder_beam_search for these dims and beam size.  Host-only: no GPU needed. */
int gic_decoder_beam_ws_bytes(const gic_decoder_dims* dims, int32_t beam, uint64_t* out);
int gic_decoder_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                            const gic_decoder_beam_opts* opts, void* ws, const float* features, int64_t* ids, float* scores,
                            int32_t* lengths, void* stream);

/* Decoder.forward, the teacher-forced decode (src/generator.py:39-53; the reference's training never calls it).
 * dims->L = T = caption length + 1 time steps: step 0 is fed `features`, step t > 0 embed(caps[b, t-1]) (caps int64 [B, T-1]).
 * lengths int32 [B] (each 1..T) with pack_padded_sequence semantics: a row past its length keeps its state and contributes a
 * zero LSTM output.  Tmax = max(lengths) (the host knows it).  out: act [B, Tmax, V] = logits (pretrain != 0) or
 * softmax((logits + gumbel(u)) * temperature) with u = noise_u f32 [B, Tmax, V] (ONE draw over the whole tensor,
 * generator.py:50,86-90) or Philox(seed) when NULL.  h_n / c_n: f32 [NL, B, H], each row's state at ITS last step.
 * state: as for gic_decoder_sample_fwd with L = T; logits_ws f32 [B*Tmax, V] and ids_ws int64 [B*Tmax]: scratch.  With
 * state->gates[k] non-NULL the gate activations of every step are saved and gic_decoder_forward_tf_bwd can follow. */
int gic_decoder_forward_tf(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                           const gic_decoder_state* state, const float* features, const int64_t* caps, const int32_t* lengths,
                           int Tmax, const float* noise_u, uint64_t seed, float temperature, int pretrain, float* logits_ws,
                           int64_t* ids_ws, void* out, float* h_n, float* c_n, void* stream);

/* (ABI v4) autograd through Decoder.forward (src/generator.py:39-53): gradients of a loss on `out` of the gic_decoder_forward_tf
 * call that filled `state` (same dims, caps, lengths, Tmax, temperature, pretrain; state->gates given).  pred = that call's `out`,
 * d_pred: act [B, Tmax, V].  Padded positions (t >= lengths[b]) are pad_packed_sequence's zeros (generator.py:45): their
 * gradient reaches b_out only.  ws / grads as for gic_decoder_sample_bwd with L = Tmax (grads->embed: scatter-add over caps;
 * grads->features = d features).  The returned hidden (h_n, c_n) is not differentiated. */
int gic_decoder_forward_tf_bwd(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                               const gic_decoder_state* state, const gic_decoder_bwd_ws* ws, const void* pred, const int64_t* caps,
                               const int32_t* lengths, int Tmax, const void* d_pred, float temperature, int pretrain,
                               const gic_decoder_grads* grads, void* stream);

/* Scheduled sampling (Bengio et al., 2015) inside the teacher-forced decode, for MLE pre-training: gic_decoder_forward_tf with
 * pretrain != 0, except that the input of step t = 1..Tmax-1 of caption b is decided after step t-1:
 *   replaced[b, t-1] = coin[b, t-1] < prob and t < lengths[b]
 *   inputs[b, t-1]   = replaced ? m[b, t-1] : clamp(caps[b, t-1], 0, V-1)
 *   m[b, t-1]        = argmax_v l[v] + g(u[t-1, b, v])   (pick 0; g(u) = -log(-log(u + 1e-10) + 1e-10))
 *                    = argmax_v l[v]                      (pick 1)
 * with l the f32 logits of step t-1 (bias included, before any rounding to the compute dtype); ties go to the lower id, a row with
 * NaN logits picks some id in [0, V).  Step t is fed embed(inputs[b, t-1]); positions >= Tmax-1 of inputs are copies of caps and
 * never count as replaced.  coin_u: f32 [B, T-1]; noise_u: f32 [T-1, B, V] (unread with pick 1); either NULL: Philox keyed by
 * (seed, a stream tag of its own, t, b) -- a caption's draws do not depend on B.  The comparison coin < prob is made in f32.
 * out: act [B, Tmax, V] raw logits; h_n / c_n as gic_decoder_forward_tf.  ws: scratch of gic_decoder_forward_ss_ws_bytes bytes, 16-byte
 * aligned.  state: as for gic_decoder_forward_tf (state->gpre, and state->gates[k] for a backward pass).  The vocabulary product of
 * a step runs inside the loop (the fused step kernels' logits epilogue where gic_decoder_fused_rollout_rows admits B, else the
 * library GEMM); one launch per step (ss_pick) tosses the coin, picks and writes the pick's embedding row into the next step's
 * input.  Backward: gic_decoder_forward_tf_bwd, unchanged, with `inputs` where it takes caps -- no gradient flows through the
 * choice.  Any V, NL in 1..GIC_MAX_LAYERS.  Argument errors (NULL required pointers, prob outside [0, 1] or NaN, pick not 0 / 1, Tmax
 * outside 1..L) return GIC_STATUS_INVALID_ARG before any launch.  No f32 atomics and no split-K: the same inputs give the same bits,
 * in and out of the deterministic mode. */
typedef struct gic_sched_sample_opts {
  float prob;                            /* p in [0, 1] */
  int32_t pick;                          /* 0 = sample, 1 = argmax */
  const float* coin_u;                   /* f32 [B, T-1] or NULL */
  const float* noise_u;                  /* f32 [T-1, B, V] or NULL */
  uint64_t seed;                         /* Philox seed of whichever of the two is NULL */
  int64_t* inputs;                       /* out, int64 [B, T-1], required (may be NULL when T = 1): the inputs the decode realised */
  int32_t* replaced;                     /* out, int32 [B, T-1] (0 / 1) or NULL */
} gic_sched_sample_opts;
int gic_decoder_forward_ss_ws_bytes(const gic_decoder_dims* dims, int Tmax, uint64_t* out);      /* host-only: no GPU needed */
int gic_decoder_forward_ss(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                           const gic_decoder_state* state, const float* features, const int64_t* caps, const int32_t* lengths,
                           int Tmax, const gic_sched_sample_opts* opts, void* ws, void* out, float* h_n, float* c_n, void* stream);

/* d_out: act [B,L,V] gradient w.r.t. `out`; probs = the forward's `out`.
 * phases (bit mask; GIC_DECODER_BWD_ALL = both, in this order):
 *   GIC_DECODER_BWD_OUTPUT     softmax/Gumbel backward, d_hout, and the COMPLETE gradients of the vocabulary projection
 *                              (grads->w_out, grads->b_out): a data-parallel caller can start all-reducing them here
 *   GIC_DECODER_BWD_RECURRENT  BPTT, LSTM weight gradients, d_features, embedding gradient */
#define GIC_DECODER_BWD_OUTPUT 1
#define GIC_DECODER_BWD_RECURRENT 2
#define GIC_DECODER_BWD_ALL 3
/* with GIC_DECODER_BWD_RECURRENT: also the gradient of the initial states (sample(states=...)): d h0 of layer k is left in the h
 * columns of ws->dxh[k] slot 0, d c0 in ws->dc[k] */
#define GIC_DECODER_BWD_STATE_GRADS 4
int gic_decoder_sample_bwd(const gic_decoder_dims* dims, const gic_decoder_params* params,
                           const gic_decoder_shadow* shadow, const gic_decoder_state* state,
                           const gic_decoder_bwd_ws* ws, const void* probs, const int64_t* ids,
                           const void* d_out, float temperature, int pretrain,
                           const gic_decoder_grads* grads, int phases, const gic_step_scalars* dev_scalars, void* stream);

/* nn.Embedding used as a callable (training.py:68,147): out[i,:] = weight[ids[i],:] and its scatter-add. */
int gic_embedding_fwd(const float* weight, const int64_t* ids, float* out, int64_t n, int32_t V, int32_t E, void* stream);
int gic_embedding_bwd(const float* d_out, const int64_t* ids, float* d_weight, int64_t n, int32_t V, int32_t E,
                      int zero_first, void* stream);

/* ------------------------------------------------------------------------------------------
 * Visual-attention caption decoder (BASELINE config 4; NO reference counterpart: the reference's decoder, src/generator.py:27-96,
 * sees the image only through the pooled feature).  The reference's roll-out loop (generator.py:55-81) with a Show-Attend-Tell soft
 * attention over the trunk's feature map in front of a one-layer LSTM; definition + CPU oracle: oracle/cpu_attention.py.
 *   fp_i = W_f a_i + b_f;  e_ti = w_a . tanh(fp_i + W_h h_{t-1});  alpha_t = softmax_i e_t;  z_t = sum_i alpha_ti a_i;
 *   LSTM input [x_t ; z_t];  logits, Gumbel, softmax, argmax feedback as gic_decoder_sample_fwd.
 */
typedef struct gic_attn_dims {
  int32_t B, L, V, E, H;       /* as gic_decoder_dims */
  int32_t C, P, A;             /* feature channels, positions (h*w) of the feature map, attention width */
  int32_t dtype;
} gic_attn_dims;

typedef struct gic_attn_params {         /* f32 master weights */
  const float* embed;                    /* decoder.embed.weight        [V,E]     */
  const float* w_ih;                     /* decoder.lstm.weight_ih_l0   [4H,E+C]  */
  const float* w_hh;                     /* decoder.lstm.weight_hh_l0   [4H,H]    */
  const float* b_ih; const float* b_hh;  /* [4H] */
  const float* w_out; const float* b_out;/* decoder.linear              [V,H],[V] */
  const float* w_f; const float* b_f;    /* decoder.attn.w_f / b_f      [A,C],[A] */
  const float* w_h;                      /* decoder.attn.w_h            [A,H]     */
  const float* w_a;                      /* decoder.attn.w_a            [A]       */
} gic_attn_params;

typedef struct gic_attn_grads {          /* f32, shapes of gic_attn_params; all overwritten */
  float* embed; float* w_ih; float* w_hh; float* b_ih; float* b_hh; float* w_out; float* b_out;
  float* w_f; float* b_f; float* w_h; float* w_a;
  float* features;                       /* d(features) [B,E] */
} gic_attn_grads;

typedef struct gic_attn_shadow {         /* compute-dtype weight images, refreshed by gic_attn_prepare */
  void* wcat;                            /* act [4H, E+C+H] = [w_ih | w_hh] */
  float* bsum;                           /* [4H] */
  void* wout;                            /* act [V,H] (may alias params.w_out in f32 mode) */
  void* wcat_t;                          /* act [E+C+H, 4H] */
  void* wf;                              /* act [A,C] */
  void* wh;                              /* act [A,H] */
} gic_attn_shadow;

typedef struct gic_attn_state {          /* saved for backward + scratch (caller-owned) */
  void* xh;                              /* act [(L+1), B, E+C+H]: x_t | z_t | h_{t-1} */
  float* gates;                          /* [L, B, 4H] */
  float* c;                              /* [(L+1), B, H] */
  void* hout;                            /* act [B, L, H] */
  float* part;                           /* scratch of the fused step kernels, as gic_decoder_state.part */
  void* fproj;                           /* act [B, P, A] */
  float* alpha;                          /* [L, B, P] attention weights */
  float* hproj;                          /* [L, B, A] W_h h_{t-1} */
} gic_attn_state;

typedef struct gic_attn_bwd_ws {
  void* dlogits;                         /* act [B, L, V] */
  float* dhout;                          /* [B, L, H] */
  void* dgates;                          /* act [L, B, 4H] */
  float* dc;                             /* [B, H] */
  float* dz;                             /* [B, C] */
  float* dalpha;                         /* [B, P] */
  float* dh_extra;                       /* [B, H] */
  void* dhproj;                          /* act [L, B, A] */
  float* dfproj;                         /* [B, P, A] */
  void* dfproj_act;                      /* act [B, P, A] (bf16 mode; may be NULL in f32 mode) */
  float* dwa_rows;                       /* [B, A] */
  float* dx;                             /* [L*B, E] */
} gic_attn_bwd_ws;

int gic_attn_prepare(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow, void* stream);
/* features f32 [B,E] (the encoder head's output, x_0); fmap act [B,P,C] (the trunk's last feature map, NHWC flattened; no gradient
 * flows into it: the trunk is frozen, generator.py:21).  noise_u / seed / temperature / pretrain / out / ids as
 * gic_decoder_sample_fwd.  V % 4 == 0 and E, H, C, A % 8 == 0.  h0 / c0: f32 [B, H] initial hidden / cell state (the `states`
 * argument of Decoder.sample's signature, generator.py:55,61) or NULL = zeros; they are constants of the backward pass (no
 * gradient is returned for them).  dev_scalars / seed_slot: temperature and seed from device memory (gic_step_scalars). */
int gic_attn_sample_fwd(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                        const gic_attn_state* state, const float* features, const void* fmap, const float* noise_u, uint64_t seed,
                        float temperature, int pretrain, void* out, int64_t* ids, const float* h0, const float* c0,
                        const gic_step_scalars* dev_scalars, int seed_slot, void* stream);
int gic_attn_sample_bwd(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                        const gic_attn_state* state, const gic_attn_bwd_ws* ws, const void* fmap, const void* probs,
                        const int64_t* ids, const void* d_out, float temperature, int pretrain, const gic_attn_grads* grads,
                        const gic_step_scalars* dev_scalars, void* stream);
/* Beam-search caption decode with the attention decoder: the semantics of gic_decoder_beam_search (candidates, tie order, eos_id /
 * pad_id, early stop, lengths, final order) with the step of gic_attn_sample_fwd(pretrain = 1): the attention of a beam at step t
 * uses its h_{t-1}, which is its parent's state; the LSTM input is [x_t ; z_t] with x_0 = features and x_t = embed(the beam's previous
 * token).  opts->h0 / c0: f32 [B, H] or NULL.  fmap act [B,P,C] as for gic_attn_sample_fwd (shadow refreshed by gic_attn_prepare).
 * ids / scores / lengths as gic_decoder_beam_search; alphas f32 [B, beam, L, P] or NULL: alphas[b, r, t, :] = the attention weights
 * with which the t-th token of the r-th returned beam was produced, zero for t >= lengths[b, r].  Limits: those of gic_attn_sample_fwd
 * and of gic_decoder_beam_search (beam 1..8 and <= V, L <= 1024, B * beam <= 2^24).  No f32 atomics: two calls on the same inputs
 * give the same bits, and the deterministic mode accepts the call and gives the same bits as outside it. */
int gic_attn_beam_ws_bytes(const gic_attn_dims* dims, int32_t beam, uint64_t* out);      /* host-only: no GPU needed */
int gic_attn_beam_search(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                         const gic_decoder_beam_opts* opts, void* ws, const float* features, const void* fmap, int64_t* ids,
                         float* scores, int32_t* lengths, float* alphas, void* stream);

/* Diverse beam search (Vijayakumar et al., AAAI 2018, Algorithm 1 with the Hamming diversity) for either decoder: K = beam.beam beams
 * (1..8 and <= V) in G = groups groups of K' = K / G (G must divide K), diversity strength lambda = diversity (finite, >= 0).  Row r
 * belongs to image r / K, beam j = r % K, group j / K'.  The recurrences, token log-probabilities, eos_id / pad_id, early stop, lengths
 * and pad handling are those of gic_decoder_beam_search / gic_attn_beam_search.
 *   start      at step 0 beam 0 of every group is live with score 0, the group's other beams have score -inf.
 *   step t     the groups select in order g = 0..G-1, each among the candidates of beam search over its own K' rows: a live row
 *              proposes its top-K tokens by raw logit (ties to the lower id), a finished row proposes itself once, with pad_id and its
 *              score unchanged.  A live row's candidate (parent p, token v) is ranked by score[p] + logp(v) - lambda * h_g(v), h_g(v) =
 *              the number of candidates with token v that groups 0..g-1 selected at this step from live parents (eos_id counts like any
 *              token); a finished row's pad proposal is neither counted nor penalised.  Each group keeps its best K' (ties to the lower
 *              (parent beam within the group, rank)).
 *   score      the kept score is the raw sum score[p] + logp(v): the penalty steers step t's selection only and is never accumulated
 *              (the paper's Algorithm 1; Hugging Face's group beam search accumulates it instead).
 * Each row's top-K by raw logit holds every winner: at most K - K' distinct tokens are penalised, so at least K' unpenalised tokens of
 * the list outrank every token outside it.  G = 1 is gic_*_beam_search, bit for bit, for any lambda; lambda = 0 makes the groups
 * independent beam searches of width K'.  Outputs in group-major order: slots g * K' .. g * K' + K' - 1 of ids int64 [B,K,L] (pad_id after
 * eos_id), scores f32 [B,K] (raw log-probability sums), lengths int32 [B,K] and (attention, or NULL) alphas f32 [B,K,L,P] hold group g's
 * beams, sorted by score / length^length_penalty (ties to the lower beam index).  The workspace is that of gic_decoder_beam_ws_bytes /
 * gic_attn_beam_ws_bytes for the same beam size.  Every argument check runs before any launch and returns GIC_STATUS_INVALID_ARG:
 * those of the beam searches, groups < 1 or not dividing K, diversity NaN, negative or infinite.  Integer atomics only: two calls on
 * the same inputs give the same bits, and the deterministic mode accepts the call and gives the same bits as outside it. */
typedef struct gic_diverse_beam_opts {
  gic_decoder_beam_opts beam;            /* beam = K, eos_id, pad_id, length_penalty, h0 / c0 as for the beam searches */
  int32_t groups;                        /* G: 1..K, divides K */
  float diversity;                       /* lambda: finite, >= 0 */
} gic_diverse_beam_opts;
int gic_decoder_diverse_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                                    const gic_diverse_beam_opts* opts, void* ws, const float* features, int64_t* ids, float* scores,
                                    int32_t* lengths, void* stream);
int gic_attn_diverse_beam_search(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                                 const gic_diverse_beam_opts* opts, void* ws, const float* features, const void* fmap, int64_t* ids,
                                 float* scores, int32_t* lengths, float* alphas, void* stream);

/* Caption sampling: n = num_samples captions per image by temperature / top-k / top-p (nucleus) sampling, for either decoder.
 * Rows = B * n: row r belongs to image r / n and is sample r % n; every row is live from step 0.  Step 0 is fed `features` with
 * (h0, c0) or zeros, step t > 0 embed(the row's own previous token); the attention decoder follows the step of gic_attn_sample_fwd
 * (the attention at step t uses h_{t-1}, the LSTM input is [x_t ; z_t]).  Per step and row, with l = the f32 logits o + b_out (never
 * rounded to bf16 before the draw) and tau = temperature (the conventional sampling temperature, dividing the logits):
 *   top-k (top_k = 0: off)   K = {v : l_v >= l_(k)}, l_(k) the k-th largest logit; ties at the boundary are kept.
 *   top-p (top_p = 1: off)   after top-k, with q = softmax(l / tau) renormalised over K: beta = the largest value such that
 *                            sum_{v in K, l_v >= beta} q_v >= top_p; kept = {v in K : l_v >= beta} (ties kept).
 *   draw                     token = argmax over kept v of l_v / tau + g(u_v), g(u) = -log(-log(u + 1e-10) + 1e-10), ties to the lower id:
 *                            an exact draw from the truncated, tempered distribution.  u = noise_u f32 [L, B*n, V] (the order of
 *                            gic_decoder_sample_fwd's noise), or Philox keyed by (seed, t, r) when noise_u is NULL: a row's noise does not
 *                            depend on the batch's other rows.
 * A row that emits eos_id has finished: afterwards it emits pad_id and its score and length stay fixed.  The decode stops after L steps
 * or once every row has finished.  Outputs in row order (not sorted): ids int64 [B, n, L]; lengths int32 [B, n] (tokens up to and
 * including eos_id, L if none); scores f32 [B, n] = the running sum of l_tok - logsumexp(l), the model's untempered, untruncated
 * log-probability (the units of the beam scores).  No f32 atomics and no split-K: two calls on the same inputs and seed give the same
 * bits; the deterministic mode accepts every call and gives the same bits inside it as outside it.  Every argument check runs before
 * any launch: num_samples outside 1..8, top_k < 0 or > V, top_p NaN / <= 0 / > 1, temperature not finite or <= 0, eos_id / pad_id
 * outside [0, V), L > 1024, rows > 2^24 or a workspace that is not 256-byte aligned return GIC_STATUS_INVALID_ARG. */
typedef struct gic_sample_opts {
  int32_t num_samples;                   /* n: 1..8 captions per image (gic_sample_logits ignores it) */
  int32_t top_k;                         /* 0 = off, else 1..V */
  float top_p;                           /* (0, 1]; 1 = off */
  float temperature;                     /* > 0 and finite; divides the logits */
  int32_t eos_id;                        /* [0, V); <E> = 2 (gic_sample_logits ignores it) */
  int32_t pad_id;                        /* [0, V); <PAD> = 0 (gic_sample_logits ignores it) */
  const float* h0;                       /* initial hidden state or NULL = zeros: [NL,B,H] (LSTM decoder), [B,H] (attention decoder) */
  const float* c0;                       /* initial cell state, as h0 */
} gic_sample_opts;
/* One truncated draw per row of f32 logits [rows, ld] (ld >= V; rows 1..2^24, V >= 2): the per-step selection of the decoders above.
 * noise_u f32 [rows, V] or NULL = Philox keyed by (seed, stream_id, r).  ids int64 [rows]; logp f32 [rows] = l_tok - logsumexp(l) (or
 * NULL); kept int32 [rows] = the size of the kept set (or NULL). */
int gic_sample_logits(const float* logits, int64_t ld, int32_t rows, int32_t V, const gic_sample_opts* opts, const float* noise_u,
                      uint64_t seed, uint64_t stream_id, int64_t* ids, float* logp, int32_t* kept, void* stream);
/* Bytes of the (256-byte aligned) workspaces of the two sampling decodes for these dims and num_samples.  Host-only: no GPU needed. */
int gic_decoder_sample_ws_bytes(const gic_decoder_dims* dims, int32_t num_samples, uint64_t* out);
int gic_attn_sample_ws_bytes(const gic_attn_dims* dims, int32_t num_samples, uint64_t* out);
/* The LSTM decoder's sampling decode: the fused step kernels where gic_decoder_fused_rollout_rows admits B * n rows, else the generic
 * products (any V). */
int gic_decoder_sample_captions(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                                const gic_sample_opts* opts, void* ws, const float* features, const float* noise_u, uint64_t seed,
                                int64_t* ids, float* scores, int32_t* lengths, void* stream);
/* The attention decoder's sampling decode: fmap act [B,P,C] as for gic_attn_sample_fwd (shadow refreshed by gic_attn_prepare); the limits
 * of gic_attn_sample_fwd apply. */
int gic_attn_sample_captions(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                             const gic_sample_opts* opts, void* ws, const float* features, const void* fmap, const float* noise_u,
                             uint64_t seed, int64_t* ids, float* scores, int32_t* lengths, void* stream);

/* Decode constraints for the beam, diverse-beam and sampling decodes of either decoder: what a caption may not contain.  A constraint
 * set is (n = no_repeat_ngram, min_length, suppress[0..S), S = num_suppress).  A live row about to emit its token of step t (0-based)
 * has the history y_0..y_{t-1} of the tokens it has emitted (in a beam search: the chain through the parent pointers, not the row
 * index).  Its banned set is
 *     banned = set(suppress)
 *     if t + 1 < min_length: banned.add(eos_id)
 *     if n >= 1 and t >= n - 1:
 *         prefix = y[t-n+1 : t]                       (n-1 tokens; empty for n = 1)
 *         for i in range(0, t - n + 1):
 *             if y[i : i+n-1] == prefix: banned.add(y[i+n-1])
 * (n = 1: every token already emitted).
 *   beam, diverse beam   a live row proposes its top-K tokens by raw logit AMONG THE TOKENS NOT BANNED, ties to the lower id.  The token
 *                        log-probability stays logit - logsumexp(all V logits): the constraint truncates the choice and never
 *                        renormalises.  Finished rows, the pad proposal, the tie orders, the Hamming count of the diverse groups, early
 *                        stop, lengths and the final order are those of the unconstrained searches.
 *   sampling             the banned tokens are removed first; top-k takes the k largest of what remains and top-p is renormalised over
 *                        that; the draw is the same Gumbel-max over the kept set; scores stay the running sum of l_tok - logsumexp(l)
 *                        over the full vocabulary.
 * A caption that cannot end before L steps has length L and no eos_id.  Limits: n and min_length in 0..L (0 = off), S in 0..16, every
 * suppressed id in [0, V) and none equal to eos_id (min_length = L forbids eos_id), and enough admissible tokens for every row to
 * propose K (the beam size; 1 for sampling): V - (S + 1 + max(0, L - n)) >= K when n >= 1, V - (S + 1) >= K when n = 0.  Every check
 * runs before any launch and returns GIC_STATUS_INVALID_ARG.  With n = 0, min_length = 0, S = 0 every constrained entry point returns
 * the bits of its unconstrained counterpart.
 * cws: the per-row ban lists, a caller-owned 256-byte aligned buffer of gic_decode_constraints_ws_bytes(rows = B * K, L, c) bytes,
 * separate from the search's own workspace `ws` (that of the unconstrained call).  The other arguments and the outputs are those of
 * gic_*_diverse_beam_search (groups = 1: plain beam search) and gic_*_sample_captions.  Integer atomics only: two calls on the same
 * inputs give the same bits, and the deterministic mode accepts the calls and gives the same bits as outside it. */
typedef struct gic_decode_constraints {
  int32_t no_repeat_ngram;               /* n: 0 = off, else 1..L */
  int32_t min_length;                    /* 0 = off, else 1..L: eos_id is banned while t + 1 < min_length */
  int32_t num_suppress;                  /* S: 0..16 */
  int32_t suppress[16];                  /* the first S are read: ids in [0, V), never eos_id */
} gic_decode_constraints;
int gic_decode_constraints_ws_bytes(int64_t rows, int32_t L, const gic_decode_constraints* c, uint64_t* out);   /* host-only: no GPU needed */
int gic_decoder_constrained_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                                        const gic_diverse_beam_opts* opts, const gic_decode_constraints* c, void* ws, void* cws,
                                        const float* features, int64_t* ids, float* scores, int32_t* lengths, void* stream);
int gic_attn_constrained_beam_search(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                                     const gic_diverse_beam_opts* opts, const gic_decode_constraints* c, void* ws, void* cws,
                                     const float* features, const void* fmap, int64_t* ids, float* scores, int32_t* lengths,
                                     float* alphas, void* stream);
int gic_decoder_constrained_sample_captions(const gic_decoder_dims* dims, const gic_decoder_params* params,
                                            const gic_decoder_shadow* shadow, const gic_sample_opts* opts,
                                            const gic_decode_constraints* c, void* ws, void* cws, const float* features,
                                            const float* noise_u, uint64_t seed, int64_t* ids, float* scores, int32_t* lengths,
                                            void* stream);
int gic_attn_constrained_sample_captions(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                                         const gic_sample_opts* opts, const gic_decode_constraints* c, void* ws, void* cws,
                                         const float* features, const void* fmap, const float* noise_u, uint64_t seed, int64_t* ids,
                                         float* scores, int32_t* lengths, void* stream);

/* Forced words: lexically constrained beam search (Anderson et al., "Guided Open Vocabulary Image Captioning with Constrained Beam
 * Search", EMNLP 2017) for either decoder: what a caption MUST contain.  Image b carries C (1..3) constraint sets of up to D (1..4)
 * token ids, ids = int32 [B, C, D] on the device, padded with -1.  A set is met once the caption has emitted any of its ids; an all -1
 * set is absent and met from the start, so the images of one batch may carry different numbers of constraints.  A token may belong
 * to several sets.  The caller keeps <PAD>, <E>, suppressed ids, ids outside [0, V) and duplicates within a set out of the sets (the
 * ids live on the device: the library reads them in its kernels only, and drops an id >= V there).
 *   state      s = the bitmask of met sets.  The K (<= 8) beams of an image are S = 2^C state groups of Kg = K / S beams, beam j in
 *              state j / Kg.  At t = 0 the first beam of the initial state (the bits of the absent sets) is live, the others at -inf.
 *   one step   for a live parent in state s the hop tokens are the ids of the sets outside s; token w moves the hypothesis to
 *              s | m(w), m(w) = the mask of every set that holds w; any other token stays in s.  State group g keeps the Kg best of:
 *              the stay candidates (the top-K admissible non-hop tokens of its live parents; the decode constraints apply as in the
 *              constrained search), the single pad proposal of each of its finished parents, and every hop token that lands in g
 *              from a live parent of another group.  Score = parent score + logit - logsumexp(all V logits), never renormalised; a
 *              hop token's logit is the same element of the same vocabulary product.  A parent at -inf proposes nothing.  A group
 *              with fewer than Kg candidates leaves the remaining beams dead: score -inf, finished.  <E> in a non-accepting state
 *              finishes the beam there.  min_length acts on <E> as before; a no-repeat rule never bans a hop token (the row has not
 *              emitted it).
 *   ties       score, then the lower parent beam, then stay before hop, then the rank in the parent's row (stay) or the slot
 *              c * D + d of the token's first unmet set (hop).
 *   early stop as in the beam search; dead beams count as finished.
 *   outputs    the K beams sorted by (real -- non-absent -- constraints met, descending; score / length^alpha, descending; beam
 *              index); dead beams last, as all-pad ids of length 0 and score -inf.  met int32 [B, K]: each returned beam's state
 *              (absent sets set; a dead beam's: the initial state).  alphas as in gic_attn_beam_search.
 * opts: groups must be 1.  c may be NULL (no decode constraints; cws unread), else c / cws as for gic_*_constrained_beam_search, with
 * the feasibility bound grown by the C * D hop tokens: V - (S + 1 + max(0, L - n) + C * D) >= K.  ws: 256-byte aligned,
 * gic_*_forced_beam_ws_bytes(dims, beam) bytes.  Limits: K <= 8, 2^C divides K, C <= 3, D <= 4; no groups, ensemble, re-ranking or
 * sampling.  Every check runs before any launch.  Integer atomics only, no split-K: the same bits run to run, in and out of the
 * deterministic mode. */
typedef struct gic_forced_words {
  int32_t C;                             /* constraint sets per image: 1..3 */
  int32_t D;                             /* ids per set: 1..4 */
  const int32_t* ids;                    /* device: int32 [B, C, D], -1 padded */
} gic_forced_words;
int gic_decoder_forced_beam_ws_bytes(const gic_decoder_dims* dims, int32_t beam, uint64_t* out);   /* host-only: no GPU needed */
int gic_attn_forced_beam_ws_bytes(const gic_attn_dims* dims, int32_t beam, uint64_t* out);         /* host-only: no GPU needed */
int gic_decoder_forced_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                                   const gic_diverse_beam_opts* opts, const gic_forced_words* forced, const gic_decode_constraints* c,
                                   void* ws, void* cws, const float* features, int64_t* ids, float* scores, int32_t* lengths,
                                   int32_t* met, void* stream);
int gic_attn_forced_beam_search(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                                const gic_diverse_beam_opts* opts, const gic_forced_words* forced, const gic_decode_constraints* c,
                                void* ws, void* cws, const float* features, const void* fmap, int64_t* ids, float* scores,
                                int32_t* lengths, float* alphas, int32_t* met, void* stream);

/* Ensemble decoding: M members (1..GIC_MAX_ENSEMBLE) of one decoder kind, dims and compute dtype share one search.  weights w_m > 0
 * are normalised to sum 1 by the library.  At a step, member m, in its own recurrent state, gives the f32 logits l_m[r, :] of row r;
 * with lp_m = l_m - logsumexp(l_m) the ensemble's logits are
 *   GIC_ENSEMBLE_PROB      z[r, v] = log sum_m w_m exp(lp_m[r, v])      (arithmetic mean of the probabilities)
 *   GIC_ENSEMBLE_LOGPROB   z[r, v] = sum_m w_m lp_m[r, v]               (geometric mean, product of experts; not normalised)
 * and the heads treat z exactly as they treat one model's logits: selection by z, a token's log-probability z - logsumexp(z) (the units
 * of the scores), the sampler's temperature / top-k / top-p, the diverse groups, the decode constraints and the early stop.  Every
 * member advances with the same chosen tokens and parent pointers.
 * gic_ensemble_mix: the mixing step itself.  logits f32 [M][rows][V] (contiguous), weights: HOST f32 [M], out f32 [rows][V]; rows
 * 1..2^24, V >= 2.  Every exp has its maximum subtracted first (finite for logits of magnitude 1e4); a member whose probability
 * underflows adds 0 (prob) and its true log-probability (logprob).  No atomics and a fixed reduction order: the same bits on every
 * call, in and out of the deterministic mode.
 * The searches: dims are those of every member; params / shadows: arrays of M pointers to the members' structs; features: array of M
 * device pointers, f32 [B, E] each (fmaps: M device pointers, act [B, P, C] each); opts->beam.h0 / c0 and the sampler's h0 / c0 must
 * be NULL.  dopts with groups = 1, diversity = 0 is the plain beam search; c may be NULL (no constraints; cws then unread), else c / cws
 * as for the gic_*_constrained_* decodes.  ids / scores / lengths as for the single-model searches.  Each member's logits are
 * materialised (the fused vocabulary product's logits form, else the GEMM), mixed into one [rows, V] slab and handed to the heads'
 * generic path.  The workspace: gic_*_ensemble_*_ws_bytes (host-only: no GPU needed), 256-byte aligned.  Every argument check runs
 * before any launch and returns GIC_STATUS_INVALID_ARG: those of the single-model searches and M out of range, a bad mode, a weight
 * that is not finite and > 0, a null member or member array. */
#define GIC_MAX_ENSEMBLE 4
#define GIC_ENSEMBLE_PROB 0
#define GIC_ENSEMBLE_LOGPROB 1
typedef struct gic_ensemble_opts {
  int32_t M;                             /* members: 1..GIC_MAX_ENSEMBLE */
  int32_t mode;                          /* GIC_ENSEMBLE_PROB / GIC_ENSEMBLE_LOGPROB */
  float weights[GIC_MAX_ENSEMBLE];       /* the first M are read: finite, > 0; normalised by the library */
} gic_ensemble_opts;
int gic_ensemble_mix(const float* logits, int32_t M, int64_t rows, int32_t V, const float* weights, int32_t mode, float* out, void* stream);
int gic_decoder_ensemble_beam_ws_bytes(const gic_decoder_dims* dims, int32_t M, int32_t beam, uint64_t* out);
int gic_attn_ensemble_beam_ws_bytes(const gic_attn_dims* dims, int32_t M, int32_t beam, uint64_t* out);
int gic_decoder_ensemble_sample_ws_bytes(const gic_decoder_dims* dims, int32_t M, int32_t num_samples, uint64_t* out);
int gic_attn_ensemble_sample_ws_bytes(const gic_attn_dims* dims, int32_t M, int32_t num_samples, uint64_t* out);
int gic_decoder_ensemble_beam_search(const gic_decoder_dims* dims, int32_t M, const gic_decoder_params* const* params,
                                     const gic_decoder_shadow* const* shadows, const gic_ensemble_opts* eopts,
                                     const gic_diverse_beam_opts* dopts, const gic_decode_constraints* c, void* ws, void* cws,
                                     const float* const* features, int64_t* ids, float* scores, int32_t* lengths, void* stream);
int gic_attn_ensemble_beam_search(const gic_attn_dims* dims, int32_t M, const gic_attn_params* const* params,
                                  const gic_attn_shadow* const* shadows, const gic_ensemble_opts* eopts,
                                  const gic_diverse_beam_opts* dopts, const gic_decode_constraints* c, void* ws, void* cws,
                                  const float* const* features, const void* const* fmaps, int64_t* ids, float* scores,
                                  int32_t* lengths, void* stream);
int gic_decoder_ensemble_sample_captions(const gic_decoder_dims* dims, int32_t M, const gic_decoder_params* const* params,
                                         const gic_decoder_shadow* const* shadows, const gic_ensemble_opts* eopts,
                                         const gic_sample_opts* sopts, const gic_decode_constraints* c, void* ws, void* cws,
                                         const float* const* features, const float* noise_u, uint64_t seed, int64_t* ids,
                                         float* scores, int32_t* lengths, void* stream);
int gic_attn_ensemble_sample_captions(const gic_attn_dims* dims, int32_t M, const gic_attn_params* const* params,
                                      const gic_attn_shadow* const* shadows, const gic_ensemble_opts* eopts,
                                      const gic_sample_opts* sopts, const gic_decode_constraints* c, void* ws, void* cws,
                                      const float* const* features, const void* const* fmaps, const float* noise_u, uint64_t seed,
                                      int64_t* ids, float* scores, int32_t* lengths, void* stream);

/* Teacher-forced decode with the attention decoder: the semantics of gic_decoder_forward_tf with the step of gic_attn_sample_fwd.
 * dims->L = T = caption length + 1: step 0 is fed `features`, step t > 0 embed(caps[b, t-1]) (caps int64 [B, T-1]; may be NULL when
 * T = 1); the attention of step t uses h_{t-1} and the LSTM input is [x_t ; z_t].  lengths int32 [B] (each 1..T) with
 * pack_padded_sequence semantics: a row with t >= lengths[b] keeps (h, c), its LSTM output is zero (its `out` row is b_out with
 * pretrain, else softmax((b_out + g) * temperature)) and its alphas row is zero.  Tmax = max(lengths) (the host knows it).
 * out act [B, Tmax, V] as gic_decoder_forward_tf (noise_u f32 [B, Tmax, V], ONE draw, or Philox(seed) when NULL).  alphas: f32
 * [B, Tmax, P] attention weights, or NULL.  h_n / c_n: f32 [B, H], each row's state at ITS last step.  state: as for
 * gic_attn_sample_fwd with L = T (every buffer, gates included, is needed by gic_attn_forward_tf_bwd).  logits_ws: f32 scratch of
 * gic_attn_forward_tf_ws_bytes bytes (the energies during the recurrence, the logits after it).  No f32 atomics and no split-K: two
 * calls on the same inputs give the same bits, and the deterministic mode accepts the call. */
int gic_attn_forward_tf_ws_bytes(const gic_attn_dims* dims, int Tmax, uint64_t* out);      /* host-only: no GPU needed */
int gic_attn_forward_tf(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                        const gic_attn_state* state, const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths,
                        int Tmax, const float* noise_u, uint64_t seed, float temperature, int pretrain, float* logits_ws, void* out,
                        float* alphas, float* h_n, float* c_n, void* stream);
/* Gradients of a loss on `out` (d_pred act [B, Tmax, V]; pred = that call's `out`) and, optionally, on the attention weights (d_alphas
 * f32 [B, Tmax, P] or NULL) of the gic_attn_forward_tf call that filled `state` (same dims, fmap, caps, lengths, Tmax, temperature,
 * pretrain).  Padded positions pass gradient to b_out only.  ws / grads as for gic_attn_sample_bwd with L = T (grads->embed:
 * scatter-add over caps; grads->features = d features).  (h_n, c_n) is not differentiated.  Accepted in the deterministic mode,
 * where two calls give the same bits. */
int gic_attn_forward_tf_bwd(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                            const gic_attn_state* state, const gic_attn_bwd_ws* ws, const void* fmap, const void* pred, const int64_t* caps,
                            const int32_t* lengths, int Tmax, const void* d_pred, const float* d_alphas, float temperature, int pretrain,
                            const gic_attn_grads* grads, void* stream);
/* Scheduled sampling inside the attention decoder's teacher-forced decode: gic_decoder_forward_ss's definition with the step of
 * gic_attn_forward_tf (pretrain != 0), alphas included.  ws: scratch of gic_attn_forward_ss_ws_bytes bytes (the logits of every step
 * and the energies of one), 16-byte aligned.  Backward: gic_attn_forward_tf_bwd, unchanged, with `inputs` where it takes caps.
 * Argument errors as gic_decoder_forward_ss, plus the dims gic_attn_* refuse.  GIC_STATUS_UNSUPPORTED in the deterministic mode, as
 * gic_attn_sample_fwd. */
int gic_attn_forward_ss_ws_bytes(const gic_attn_dims* dims, int Tmax, uint64_t* out);      /* host-only: no GPU needed */
int gic_attn_forward_ss(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                        const gic_attn_state* state, const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths,
                        int Tmax, const gic_sched_sample_opts* opts, void* ws, void* out, float* alphas, float* h_n, float* c_n,
                        void* stream);

/* Output dropout of the caption decoder, for teacher-forced MLE pre-training: the LSTM output is dropped in front of the vocabulary
 * projection, as Show-Attend-Tell's dropout(h) before fc; the recurrence keeps the undropped h.  With hout act [B, Tmax, H]:
 *   keep[b, t, h]  = u[b, t, h] >= p
 *   hdrop[b, t, :] = keep ? hout[b, t, :] * s : 0          s = 1.0f / (1.0f - p) in f32; the product is formed in f32 and rounded to
 *                                                          the compute dtype
 *   logits         = hdrop W_out^T + b_out
 * Rows past a caption's length are zero in hout and stay zero.  u = keep_u, or Philox keyed by (seed, a stream tag of its own) and
 * the flat index i = (b * Tmax + t) * H + h of the element: lane i & 3 of counter i >> 2.  The mask is not stored: the backward
 * regenerates it from (seed, p) or reads keep_u again, so both calls must be given the same values.  hdrop is written by the forward
 * call and read by the backward call (the gradient of W_out is taken against what the projection consumed).
 * The gic_*_drop entry points take their plain counterpart's arguments with `drop` in front of `stream` and return its errors first;
 * then a NULL drop, p outside (0, 1) or NaN, a NULL or misaligned hdrop return GIC_STATUS_INVALID_ARG before any launch.  They launch
 * what the plain entry points launch plus one dropout kernel per call and direction (scheduled sampling: one per step, on the B rows
 * of that step, in front of the step's logits -- the picks see the dropped logits); the backward's replaces the launch that zeroes
 * d hout past the lengths.  No atomics: valid in the deterministic mode wherever the plain entry point is. */
typedef struct gic_decoder_dropout {
  float p;                               /* 0 < p < 1 */
  uint64_t seed;                         /* Philox seed of the mask when keep_u is NULL */
  const float* keep_u;                   /* f32 [B, Tmax, H] or NULL = device draw */
  void* hdrop;                           /* compute dtype [B, Tmax, H], 16-byte aligned; forward writes, backward reads */
} gic_decoder_dropout;
int gic_decoder_forward_tf_drop(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                                const gic_decoder_state* state, const float* features, const int64_t* caps, const int32_t* lengths,
                                int Tmax, const float* noise_u, uint64_t seed, float temperature, int pretrain, float* logits_ws,
                                int64_t* ids_ws, void* out, float* h_n, float* c_n, const gic_decoder_dropout* drop, void* stream);
int gic_decoder_forward_ss_drop(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                                const gic_decoder_state* state, const float* features, const int64_t* caps, const int32_t* lengths,
                                int Tmax, const gic_sched_sample_opts* opts, void* ws, void* out, float* h_n, float* c_n,
                                const gic_decoder_dropout* drop, void* stream);
int gic_decoder_forward_tf_drop_bwd(const gic_decoder_dims* dims, const gic_decoder_params* params, const gic_decoder_shadow* shadow,
                                    const gic_decoder_state* state, const gic_decoder_bwd_ws* ws, const void* pred, const int64_t* caps,
                                    const int32_t* lengths, int Tmax, const void* d_pred, float temperature, int pretrain,
                                    const gic_decoder_grads* grads, const gic_decoder_dropout* drop, void* stream);
int gic_attn_forward_tf_drop(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                             const gic_attn_state* state, const float* features, const void* fmap, const int64_t* caps,
                             const int32_t* lengths, int Tmax, const float* noise_u, uint64_t seed, float temperature, int pretrain,
                             float* logits_ws, void* out, float* alphas, float* h_n, float* c_n, const gic_decoder_dropout* drop,
                             void* stream);
int gic_attn_forward_ss_drop(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                             const gic_attn_state* state, const float* features, const void* fmap, const int64_t* caps,
                             const int32_t* lengths, int Tmax, const gic_sched_sample_opts* opts, void* ws, void* out, float* alphas,
                             float* h_n, float* c_n, const gic_decoder_dropout* drop, void* stream);
int gic_attn_forward_tf_drop_bwd(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                                 const gic_attn_state* state, const gic_attn_bwd_ws* ws, const void* fmap, const void* pred,
                                 const int64_t* caps, const int32_t* lengths, int Tmax, const void* d_pred, const float* d_alphas,
                                 float temperature, int pretrain, const gic_attn_grads* grads, const gic_decoder_dropout* drop,
                                 void* stream);
/* The two stages on their own.  gic_hidden_dropout: y = keep ? x * s : 0 over x / y of `dtype` [rows, H] (contiguous; any H and any
 * alignment: 16-byte loads and stores where H % 4 == 0 (f32) / H % 8 == 0 (bf16) and both bases are 16-byte aligned, else scalar
 * ones), element (r, h) drawn at i = r * H + h as above; keep_u f32 [rows, H] or NULL.  gic_hidden_dropout_bwd, in place on dhout
 * f32 [B, Tmax, H]: dhout = (t < lengths[b] && keep) ? dhout * s : 0 (lengths int32 [B]). */
int gic_hidden_dropout(const void* x, int dtype, int64_t rows, int32_t H, float p, uint64_t seed, const float* keep_u, void* y,
                       void* stream);
int gic_hidden_dropout_bwd(float* dhout, const int32_t* lengths, int32_t B, int32_t Tmax, int32_t H, float p, uint64_t seed,
                           const float* keep_u, void* stream);

/* Monte-Carlo roll-outs of the attention decoder (the SeqGAN step's): the counterpart of gic_decoder_sample_fwd with force_ids,
 * force_len, no_state and resume_from.  dims->B = images, dims->L = caption length.  `rows` roll-out rows, row r of image r % B: it
 * copies force_ids[r % B, :force_len[r]] (force_ids int64 [B, L], the captions; force_len int32 [rows], ascending, each 1..L-1), joins
 * at step t = force_len[r] from the recurrent state resume_from reached there -- the state of a gic_attn_forward_tf call along the
 * captions with T = L and every length L (its xh, c and fproj are read) -- and from then on samples with Gumbel-max at temperature 1:
 * argmax(o + b_out + gumbel(u)), the first maximal index.  host_active_rows: L host ints, [t] = the number of rows with force_len <= t
 * ([0] == 0, non-decreasing, <= rows): at step t the first host_active_rows[t] rows run.  fmap act [B, P, C].  noise_u f32
 * [L, rows, V] or NULL = Philox(seed, stream t) indexed as gic_decoder_sample_fwd indexes it.  ids int64 [rows, L] (entries a row
 * never reaches are 0).  ws: gic_attn_rollout_ws_bytes bytes, 256-byte aligned; it is affine in rows and holds nothing per (row,
 * position, channel): the image data is read from fproj / fmap, once per image.  The launch count per step does not depend on the
 * rows.  Every argument check (the limits of gic_attn_sample_fwd; L 2..1024; rows 1..2^22 with rows * (E+C+H) below 2^30 and rows * 4H below 2^31)
 * runs before any launch and returns GIC_STATUS_INVALID_ARG.  No f32 atomics and no split-K (the fused vocabulary product's integer
 * atomicMax is order-independent): two calls give the same bits, and the deterministic mode accepts the call. */
int gic_attn_rollout_ws_bytes(const gic_attn_dims* dims, int64_t rows, uint64_t* out);      /* host-only: no GPU needed */
int gic_attn_rollout(const gic_attn_dims* dims, const gic_attn_params* params, const gic_attn_shadow* shadow,
                     const gic_attn_state* resume_from, const void* fmap, const int64_t* force_ids, int64_t rows,
                     const int32_t* force_len, const int32_t* host_active_rows, const float* noise_u, uint64_t seed, void* ws,
                     int64_t* ids, void* stream);

/* ------------------------------------------------------------------------------------------
 * Discriminator.forward (src/discriminator.py:34-62) forward + backward.
 */
typedef struct gic_disc_dims {
  int32_t B, L, V, De, R, nconv;         /* De=disc_embed_dim, R=disc_num_rep, s = De/R */
  int32_t fsize[GIC_MAX_CONVS];          /* disc_filter_sizes */
  int32_t nfilt[GIC_MAX_CONVS];          /* disc_num_filters */
  int32_t F;                             /* sum(nfilt) */
  int32_t Fp;                            /* leading dim of the [B*R, F] activations (>= F, multiple of 8) */
  int32_t dtype;
  float drop_p;                          /* nn.Dropout p before feature2out (discriminator.py:10,30; default 0.2), 0 <= p < 1 */
} gic_disc_dims;

typedef struct gic_disc_params {
  const float* emb;                      /* embeddings.weight  [De,V] */
  const float* conv_w[GIC_MAX_CONVS];    /* convs.k.weight     [n_k,1,f_k,s] */
  const float* conv_b[GIC_MAX_CONVS];    /* convs.k.bias       [n_k] */
  const float* hw_w; const float* hw_b;  /* highway            [F,F],[F] */
  const float* f2o_w; const float* f2o_b;/* feature2out        [100,F],[100] */
  const float* o2l_w; const float* o2l_b;/* out2logits         [1,100],[1] */
} gic_disc_params;

typedef struct gic_disc_grads {          /* f32; accumulate != 0 adds to the existing contents */
  float* emb; float* conv_w[GIC_MAX_CONVS]; float* conv_b[GIC_MAX_CONVS];
  float* hw_w; float* hw_b; float* f2o_w; float* f2o_b; float* o2l_w; float* o2l_b;
} gic_disc_grads;

typedef struct gic_disc_shadow {         /* compute-dtype weight images (may alias params in f32 mode) */
  void* emb;                             /* act [De,V] */
  void* hw_w;                            /* act [F,F]  */
  void* f2o_w;                           /* act [100,F] */
  void* hw_w_t;                          /* act [Fp,Fp] = highway^T, the k-contiguous operand of the highway input-gradient
                                            product; NULL: that product reads hw_w transposed instead */
} gic_disc_shadow;

typedef struct gic_disc_state {          /* saved-for-backward of one forward call (caller-owned) */
  float* emb;                            /* [B*L, De] */
  void* pooled;                          /* act [B*R, Fp] conv+relu+max-over-time, row = b*R+r */
  uint8_t* argmax;                       /* [B*R, Fp] time index of the max */
  float* hpre;                           /* [B*R, Fp] highway pre-activation */
  uint8_t* keep;                         /* [B*R, Fp] dropout keep mask actually used (train mode) */
  void* ydrop;                           /* act [B*R, Fp] dropped highway output */
  float* feat;                           /* [B*R, 100] */
} gic_disc_state;

typedef struct gic_disc_bwd_ws {
  void* dfeat;                           /* act [B*R, 104] */
  void* dh;                              /* act [B*R, Fp] */
  float* dydrop;                         /* [B*R, Fp] */
  float* dpooled;                        /* [B*R, Fp] */
  void* demb;                            /* act [B*L, De] */
} gic_disc_bwd_ws;

/* Byte sizes in field order: gic_disc_state -> emb, pooled, argmax, hpre, keep, ydrop, feat (7 values; ydrop must start zeroed:
 * its pad columns are read); gic_disc_bwd_ws -> dfeat, dh, dydrop, dpooled, demb (5 values).  Host-only.
 * Pad columns F .. Fp-1: gic_disc_fwd writes those of pooled and argmax as zero and leaves ydrop's zero; gic_disc_bwd writes those of dh,
 * dydrop and dpooled as zero.  Those of hpre and keep are never read as values and may be left unwritten (the highway epilogues store
 * live columns only, or whole 8-column groups up to the one that holds column F-1): a caller must not rely on their contents. */
int gic_disc_state_bytes(const gic_disc_dims* dims, uint64_t* out);
int gic_disc_bwd_ws_bytes(const gic_disc_dims* dims, uint64_t* out);

int gic_disc_prepare(const gic_disc_dims* dims, const gic_disc_params* params, const gic_disc_shadow* shadow, void* stream);

/* Exactly one of inp_soft (act [B*L, V], row stride ld_inp, rows in (b,l) order) and inp_ids (int64 [B,L];
 * the one-hot of training.py:158 evaluated as a gather) is non-NULL.
 * train != 0: dropout(dims->drop_p) with keep_mask (uint8 0/1 [B*R,F], row stride F) or, if NULL, Philox(seed) -- the seed read
 * from dev_scalars->seed[seed_slot] on the device when dev_scalars != NULL (gic_step_scalars).
 * train == 0 with state->argmax == NULL and / or state->hpre == NULL: a forward that no backward follows (reward evaluation of
 * the SeqGAN-style step): those buffers are not written.  logits: f32 [B*R]. */
int gic_disc_fwd(const gic_disc_dims* dims, const gic_disc_params* params, const gic_disc_shadow* shadow,
                 const gic_disc_state* state, const void* inp_soft, int64_t ld_inp, const int64_t* inp_ids,
                 int train, const uint8_t* keep_mask, uint64_t seed, float* logits, const gic_step_scalars* dev_scalars,
                 int seed_slot, void* stream);

/* A second forward on the SAME input as the pass that filled `src` (training.py:163-164 run D twice on gen_captions: only
 * the dropout draw differs): reuses src's pooled features and highway pre-activation, applies a fresh dropout mask
 * (keep_mask or Philox(seed)) and the feature2out / out2logits head.  Writes dst->keep, dst->ydrop, dst->feat and logits; for
 * the backward pass of this forward, dst->emb / pooled / argmax / hpre must alias src's buffers. */
int gic_disc_fwd_redrop(const gic_disc_dims* dims, const gic_disc_params* params, const gic_disc_shadow* shadow,
                        const gic_disc_state* src, const gic_disc_state* dst, int train, const uint8_t* keep_mask,
                        uint64_t seed, float* logits, const gic_step_scalars* dev_scalars, int seed_slot, void* stream);

/* d_logits f32 [B*R].  grads may be NULL (no parameter gradients wanted: the generator's path,
 * training.py:169).  d_inp: act [B*L, V] (row stride ld_dinp) or NULL.
 * Exactly one of inp_soft / inp_ids describes the input of the forward(s) that filled `state` -- or BOTH, for a state whose first
 * B/2 captions were evaluated from token ids (inp_ids: int64 [B/2, L]) and whose last B/2 from soft rows (inp_soft: act
 * [B/2*L, V]): the step's D(real) and D(fake) passes written into the two halves of one state, differentiated in one call
 * (grads required, d_inp must be NULL). */
int gic_disc_bwd(const gic_disc_dims* dims, const gic_disc_params* params, const gic_disc_shadow* shadow,
                 const gic_disc_state* state, const gic_disc_bwd_ws* ws, const void* inp_soft, int64_t ld_inp,
                 const int64_t* inp_ids, int train, const float* d_logits, const gic_disc_grads* grads,
                 int accumulate, void* d_inp, int64_t ld_dinp, void* stream);

/* (an addition to ABI v5) Host-only: the kernels gic_disc_fwd and gic_disc_bwd / gic_disc_bwd_cond launch of their own for these dims (the
 * library's very selection, csrc/disc.hip select_disc_fwd / select_disc_bwd; their GEMMs are gic_gemm's business), one line per launch in
 * launch order, '\n'-terminated, written to out (out_len bytes, the terminating 0 included): the kernel with its template arguments,
 * grid= (workgroups), block=, lds= (dynamic bytes) as in gic_debug_last_route, and where they apply blocks= / rows_y= with part= (1: the
 * deterministic mode's partials are written and folded; the fold is the next line) and rpb= (rows per block).  Line 0 is the forward's
 * conv + pool kernel, the others the backward's.  flags: GIC_DISC_PLAN_* below.  The deterministic mode is the library's current one.
 * Never touches the GPU and looks at no pointer (dims->B .. drop_p are validated as gic_disc_fwd validates them).
 * GIC_STATUS_INVALID_ARG: bad dims, the conv weights do not fit gic_disc_bwd's LDS staging (its message), out too small. */
#define GIC_DISC_PLAN_NO_ARGMAX 1      /* the forward keeps no argmax (state->argmax == NULL: no backward follows); line 0 only */
#define GIC_DISC_PLAN_GRADS 2          /* parameter gradients wanted (grads != NULL) */
#define GIC_DISC_PLAN_TRAIN 4          /* train != 0 */
#define GIC_DISC_PLAN_HW_UNALIGNED 8   /* a buffer of the highway backward is off its 16-byte (keep: 8-byte) alignment */
int gic_debug_disc_plan(const gic_disc_dims* dims, int flags, char* out, int64_t out_len);

/* Image-conditioned discriminator (--disc-cond projection; no reference counterpart): the projection match term
 *   logits[m] (+)= scale * sum_{n<F} ydrop[m, n] * q[m / R, n]       q: f32 [B, F], one row per caption; scale = F^-1/2
 * on state->ydrop of a gic_disc_fwd / gic_disc_fwd_redrop pass (a forward-only state included: only ydrop is read).
 * accumulate != 0 adds to logits (the conditioned forward = gic_disc_fwd, then this), else logits is overwritten with the term alone. */
int gic_disc_match_fwd(const gic_disc_dims* dims, const gic_disc_state* state, const float* q, float scale, int accumulate,
                       float* logits, void* stream);
/* gic_disc_bwd of logits that carry the match term: additionally d ydrop[m, :] += scale * d_logits[m] * q[m / R, :] before the highway
 * backward, and d_q[b, :] = scale * sum_r d_logits[b R + r] * ydrop[b R + r, :F] (f32 [B, F], overwritten; may be NULL), summed in row
 * order without atomics (the same bits in and out of deterministic mode).  A mixed batch passes q of its 2 * (B/2) captions.
 * q == NULL (then d_q must be NULL): exactly gic_disc_bwd. */
int gic_disc_bwd_cond(const gic_disc_dims* dims, const gic_disc_params* params, const gic_disc_shadow* shadow,
                      const gic_disc_state* state, const gic_disc_bwd_ws* ws, const void* inp_soft, int64_t ld_inp,
                      const int64_t* inp_ids, int train, const float* d_logits, const gic_disc_grads* grads,
                      int accumulate, void* d_inp, int64_t ld_dinp, const float* q, float scale, float* d_q, void* stream);
/* The D loss with mismatched pairs, d_loss = (1 - w) d(real, fake) + w d(real, wrong), from two gic_gan_losses evaluations a =
 * (real, fake) and b = (real, wrong), in place: losses_a[1] becomes the mix, dd_real_a the mixed gradient w.r.t. the real logits,
 * dd_fake_a is scaled by 1 - w and dd_fake_b (the gradient w.r.t. the wrong-pair logits) by w.  0 <= w < 1.  The four gradient
 * vectors (f32 [n]) are all given or all NULL. */
int gic_gan_losses_mismatch(float w, int64_t n, float* losses_a, const float* losses_b, float* dd_real_a, float* dd_fake_a,
                            const float* dd_real_b, float* dd_fake_b, void* stream);

/* Inference uses of D (no reference counterpart; additions to ABI v5).
 * The match term with an image index per caption: caption b (of dims->B) is scored against row q_index[b] of q (f32 [q_rows, F]),
 *   logits[b R + r] (+)= scale * sum_{n<F} ydrop[b R + r, n] * q[q_index[b], n]
 * q_index == NULL is the identity (then q_rows must equal B, and the result carries the bits of gic_disc_match_fwd).  An index outside
 * [0, q_rows) is never dereferenced: the R logits of that caption become NaN.  One kernel serves both entries. */
int gic_disc_match_fwd_grouped(const gic_disc_dims* dims, const gic_disc_state* state, const float* q, int32_t q_rows,
                               const int32_t* q_index, float scale, int accumulate, float* logits, void* stream);
/* Re-rank K candidates per image (K in 1..64) by G's length-normalised log-probability plus weight times D's score:
 *   d[b,k] = (1/R) sum_r d_logits[(b K + k) R + r]   (r in index order)      final[b,k] = lm[b,k] / max(len,1)^length_penalty + weight d[b,k]
 * (weight == 0: final is the first term alone, whatever d_logits holds).  order[b,:] = the input indices by final descending, ties to the
 * lower input index, a NaN final last; final_scores, d_scores, out_ids [B,K,L], out_lm_scores, out_lengths and out_alphas [B,K,L,P] are
 * the inputs' rows in that order (out_ids / out_lm_scores / out_lengths / out_alphas may be NULL; alphas == NULL or P == 0: none).  One
 * workgroup per image, no atomics.  An output that overlaps an input or another output is refused (GIC_STATUS_INVALID_ARG). */
int gic_rerank(const float* lm_scores, const int32_t* lengths, float length_penalty, const float* d_logits, int32_t R, float weight,
               const int64_t* ids, const float* alphas, int32_t B, int32_t K, int32_t L, int32_t P, int32_t* order, float* final_scores,
               float* d_scores, int64_t* out_ids, float* out_lm_scores, int32_t* out_lengths, float* out_alphas, void* stream);
/* Means over the R representations of a forward's state: ybar[c, :] = (1/R) sum_r ydrop[c R + r, :F] (f32 [B, F]) and, when logits
 * (f32 [B*R], the base logits) and lbar (f32 [B]) are given, lbar[c] = (1/R) sum_r logits[c R + r]; r in index order.  B <= 65535 per call. */
int gic_disc_rep_mean(const gic_disc_dims* dims, const gic_disc_state* state, const float* logits, float* ybar, float* lbar, void* stream);
/* Retrieval ranks (0-based) of N (image, caption) pairs from their score matrix: T[c,j] = S[c,j] + row_bias[c] (row_bias NULL = 0),
 *   rank_c2i[c] = #{j != c : !(T[c,j] < T[c,c])}        rank_i2c[j] = #{c != j : !(T[c,j] < T[j,j])}
 * so a tie or a NaN counts against the true pair.  S is f32 with row stride ld >= N; the counts are integers (order-free). */
int gic_match_ranks(const float* S, int64_t ld, const float* row_bias, int32_t N, int32_t* rank_c2i, int32_t* rank_i2c, void* stream);

/* ------------------------------------------------------------------------------------------
 * Encoder (src/generator.py:8-25): ResNet trunk forward (frozen, BatchNorm on batch statistics) and the trainable
 * Linear + BatchNorm1d(momentum=0.01) head.  Activations are NHWC in the compute dtype ("act").
 */
/* NCHW f32 [N,3,S,S] -> zero-bordered NHWC4 act [N, S+2*pad, Wp, 4] (channel 3 = 0); Wp >= S+2*pad. */
int gic_pack_image(const float* nchw, void* out, int dtype, int N, int S, int pad, int Wp, void* stream);

/* Image pipeline: everything between the JPEG decode and that NCHW tensor (the Resize / ToTensor / Normalize of src/tasks.py:92-100,
 * plus an optional crop box and horizontal flip) for a ragged batch of uint8 images in ONE kernel.
 *
 * Per axis (source length n, box [b0, b1) in source pixels, S outputs) the triangle filter with its support scaled by the downscale
 * factor, separable, horizontal pass first, no 8-bit rounding between the passes:
 *   scale = (b1 - b0) / S   fs = max(scale, 1)   c_i = b0 + (i + 0.5) scale
 *   taps first = max(int(c_i - fs + 0.5), 0) .. last - 1, last = min(int(c_i + fs + 0.5), n)       clipped to the image, not the box
 *   w_x = max(0, 1 - |x - c_i + 0.5| / fs), normalised to sum 1 over the taps
 * = PIL Image.resize(BILINEAR, box=) up to its 8-bit roundings = F.interpolate(bilinear, antialias=True).  flip mirrors the output
 * horizontally; a one-channel image feeds all three planes; out = (v / 255 - mean_c) / std_c.
 *
 * pixels: DEVICE bytes (any alignment; 4-byte aligned takes the dword-load path); src / mean / std: HOST; out_nchw: DEVICE f32
 * [N,3,S,S], 16-byte aligned; ws: DEVICE scratch of gic_image_preprocess_ws_bytes(N, S) bytes, 16-byte aligned.  Every descriptor is
 * checked on the host before anything is enqueued -- N in 1..65535, S in 1..1024, height / width in 1..16384, channels 1 | 3,
 * row_stride >= width * channels, offset + (height-1) row_stride + width channels <= pixels_bytes, a finite ordered box inside the
 * image, flip 0 | 1, std > 0; anything else GIC_STATUS_INVALID_ARG -- and the descriptors travel to ws as kernel arguments: no host
 * memory is read after the call returns.  The kernel checks every load against pixels_bytes as well.  Centres and weight sums are
 * float64, tap offsets f32 relative to the first tap, accumulation f32 in a fixed order, no atomics: two calls give the same bits,
 * and any offset / row_stride gives the bits of any other. */
typedef struct {            /* one source image; host array */
  int64_t offset;           /* byte offset of pixel (0,0) in `pixels` */
  int32_t height, width;    /* 1 .. 16384 */
  int32_t channels;         /* 1 or 3, interleaved (HWC) */
  int32_t row_stride;       /* bytes, >= width*channels */
  float   box[4];           /* x0, y0, x1, y1 in source pixels, 0 <= x0 < x1 <= width (same for y); the whole image = 0,0,W,H */
  int32_t flip;             /* 0 / 1: mirror the output horizontally */
  int32_t reserved;
} gic_image_src;
/* Host-only (no GPU needed): bytes of `ws` for N images. */
int gic_image_preprocess_ws_bytes(int32_t N, int32_t S, uint64_t* out);
int gic_image_preprocess(const uint8_t* pixels, uint64_t pixels_bytes, const gic_image_src* src, int32_t N, int32_t S,
                         const float mean[3], const float std[3], float* out_nchw, void* ws, void* stream);
/* conv weight [Cout,Cin,KH,KW] f32 -> act [Cout,KH,KW_pad,Cin_pad] (zero padded). */
int gic_repack_conv_weight(const float* w, void* out, int dtype, int Cout, int Cin, int KH, int KW, int Cin_pad, int KW_pad,
                           void* stream);
/* Implicit-GEMM convolution on MFMA: in act [N,H,W,Cin], w act [Cout,KH,KW,Cin], out act [N,Ho,Wo,Cout].  stats (optional,
 * f32 [stats_nrep][2*Cout], accumulated with atomics: the caller zeroes it; workgroup b adds into replica b % stats_nrep so that
 * few adders share an address, readers sum the replicas): per-channel sum and sum of squares of the f32 results = the batch
 * statistics nn.BatchNorm2d needs in train mode.  Replaces nn.Conv2d of the torchvision trunk (generator.py:12-14,22). */
int gic_conv2d(const void* in, const void* w, void* out, float* stats, int stats_nrep, int dtype, int N, int H, int W, int Cin,
               int Cout, int KH, int KW, int stride, int pad, void* stream);

/* Convolution whose INPUT is normalised on the fly: out = conv(pad(relu(gamma (in - mean) / sqrt(var + 1e-5) + beta))) with
 * mean / var from `in_stats` ([in_nrep][2*Cin] sums written by the gic_conv2d that produced `in`, over in_count rows).  Replaces the
 * bn -> ReLU -> conv links inside the torchvision residual blocks (src/generator.py:12-14) without the separate gic_bn_act pass
 * and without the normalised tensor: 1x1 windows rewrite each A tile in LDS before its MFMAs; 3x3 / stride 1 / pad 1 windows with
 * Cin % 64 == 0 keep the input patch of a 128-pixel tile in LDS for all nine taps and normalise it once per 64-channel chunk
 * (padding stays zero).  `stats` receives this convolution's own column sums as gic_conv2d does.  Returns GIC_STATUS_UNSUPPORTED
 * (and launches nothing) in f32 mode, for Cin > 1024 or Cin % 8 != 0, for any other window, or for shapes the kernels do not
 * take: the caller then runs gic_bn_act + gic_conv2d. */
int gic_conv2d_bn_in(const void* in, const float* in_stats, int in_nrep, const float* in_gamma, const float* in_beta, float in_count,
                     const void* w, void* out, float* stats, int stats_nrep, int dtype, int N, int H, int W, int Cin, int Cout, int KH,
                     int KW, int stride, int pad, void* stream);
/* The 1x1 convolution that opens a bottleneck block, with the PREVIOUS block's output formed on load: its A operand is
 *   x = relu( bn(in) + r ),   r = res (identity shortcut, res_stats == NULL) or bn_res(res) (projection shortcut),
 * with both BatchNorms on batch statistics (sums over `count` rows: in_stats [in_nrep][2*Cin], res_stats [res_nrep][2*Cin]) --
 * torchvision's `out = relu(bn3(conv3(..)) + identity)` followed by the next block's conv1 (src/generator.py:12-14) without the
 * separate normalise + add + relu pass: the workgroups of the first output-channel tile also write x to block_out [N,H,W,Cin]
 * (the next shortcut / the projection convolution read it from there).  in, res: act [N,H,W,Cin]; w act [Cout,Cin]; out act
 * [N,H,W,Cout]; stats as gic_conv2d.  GIC_STATUS_UNSUPPORTED (nothing launched) in f32 mode, for Cin % 8 != 0 or Cin > 2048, or for
 * shapes the 8-wave kernel does not take: the caller then runs gic_bn_act + gic_conv2d. */
int gic_conv1x1_res_in(const void* in, const float* in_stats, int in_nrep, const float* in_gamma, const float* in_beta, const void* res,
                       const float* res_stats, int res_nrep, const float* res_gamma, const float* res_beta, float count, void* block_out,
                       const void* w, void* out, float* stats, int stats_nrep, int dtype, int N, int H, int W, int Cin, int Cout,
                       void* stream);

/* (ABI v4) The tail of a bottleneck block and the head of the next one in ONE launch, with conv3's output never written
 * (src/generator.py:12-14: `out = relu(bn3(conv3(relu(bn2(y2)))) + shortcut)` followed by the next block's conv1):
 *   gic_conv1x1_bn_in_stats   conv3's BatchNorm column sums ONLY (its own statistics have to exist before any of its output can be
 *                             normalised): in = y2 act [rows, Cin] read as relu(bn(in)) as in gic_conv2d_bn_in, w act [Cout, Cin],
 *                             stats [stats_nrep][2*Cout] added to as gic_conv2d does; nothing else is written.
 *   gic_conv_b2b              recomputes conv3 from y2 (C2 channels; w3 act [4*C2, C2]), forms out = relu(bn3(.) + r), r = res (identity
 *                             shortcut, res_stats == NULL) or bn_res(res) (projection), writes it to block_out act [rows, 4*C2] and feeds
 *                             it to the next conv1 (w1n act [C1N, 4*C2]): y1n act [rows, C1N] and its column sums into stats1.
 *                             All BatchNorms on batch statistics over `count` rows.
 * Both return GIC_STATUS_UNSUPPORTED (nothing launched) in f32 mode and for shapes they have no kernel for (C2 in {64, 128},
 * (C2, C1N) in {(64, 64), (64, 128), (128, 128), (128, 256)}, rows % 128 == 0, rows * 4 * C2 * 2 < 2^31 bytes, enough rows for the
 * streaming kernel): the caller runs gic_conv2d_bn_in + gic_conv1x1_res_in. */
int gic_conv1x1_bn_in_stats(const void* in, const float* in_stats, int in_nrep, const float* in_gamma, const float* in_beta, float in_count,
                            const void* w, float* stats, int stats_nrep, int dtype, int64_t rows, int Cin, int Cout, void* stream);
int gic_conv_b2b(const void* y2, const float* stats2, int nrep2, const float* gamma2, const float* beta2, const void* w3, const float* stats3,
                 int nrep3, const float* gamma3, const float* beta3, const void* res, const float* res_stats, int res_nrep,
                 const float* res_gamma, const float* res_beta, float count, void* block_out, const void* w1n, void* y1n, float* stats1,
                 int nrep1, int dtype, int64_t rows, int C2, int C1N, void* stream);
/* (ABI v5) 1 if gic_conv_b2b has a kernel for these shapes (the list above), else 0: a host-only query, the very test gic_conv_b2b applies
 * before it looks at its pointers. */
int gic_conv_b2b_supported(int dtype, int64_t rows, int C2, int C1N);
/* out = [relu]( bn(y) + (res ? bn_res(res) : 0) ) over rows x C.  A BatchNorm takes its mean/var from `stats` (raw sums over
 * `count` rows; train mode) or from run_mean/run_var (eval mode); res_gamma == NULL -> the residual is added as is. */
int gic_bn_act(const void* y, const float* stats, const float* gamma, const float* beta, const float* run_mean,
               const float* run_var, const void* res, const float* res_stats, const float* res_gamma, const float* res_beta,
               const float* res_run_mean, const float* res_run_var, int stats_nrep, float count, int relu, void* out, int dtype,
               int64_t rows, int C, void* stream);
/* Stem: relu(bn(y)) then 3x3 / stride 2 / pad 1 max-pool.  y act [N,H,W,C] -> out act [N,(H+1)/2,(W+1)/2,C]. */
int gic_bn_relu_maxpool(const void* y, const float* stats, const float* gamma, const float* beta, const float* run_mean,
                        const float* run_var, int stats_nrep, float count, void* out, int dtype, int N, int H, int W, int C,
                        void* stream);
/* Global average pool: x act [N,HW,C] -> out act [N,C]. */
int gic_avgpool(const void* x, void* out, int dtype, int N, int HW, int C, void* stream);
/* Running mean/var of every trunk BatchNorm2d in one launch; `table_dev` is a DEVICE array built once by the caller. */
typedef struct gic_bn_running_desc {
  const float* stats;      /* [nrep][2C] raw sums of this step */
  float* running_mean;     /* [C] */
  float* running_var;      /* [C] */
  float count;             /* rows the sums were taken over */
  float momentum;
  int32_t C;
  int32_t nrep;
} gic_bn_running_desc;
int gic_bn_running_update(const gic_bn_running_desc* table_dev, int nlayers, void* stream);
/* nn.BatchNorm1d over the batch axis of x [B,E] (generator.py:16,24) forward / backward. */
int gic_bn1d_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, int training,
                 float momentum, float eps, float* y, float* xhat, float* invstd, int B, int E, void* stream);
int gic_bn1d_bwd(const float* dy, const float* xhat, const float* invstd, const float* gamma, int training, float* dx,
                 float* dgamma, float* dbeta, int B, int E, void* stream);
/* out[c] (+)= sum_r A[r*lda + c] (bias gradients). */
int gic_colsum(const void* A, int dtype, int64_t lda, int64_t rows, int64_t cols, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deterministic mode (torch.backends.cudnn.deterministic, src/main.py:22-23).  Process-wide, host-only (no GPU needed), off by
 * default; GIC_DETERMINISTIC=1 in the environment turns it on when the library is loaded.  While it is on, every entry point
 * that accepts the call gives bit-identical results for the same inputs, shapes, library build and device model: each f32 sum
 * that several workgroups contribute to has a fixed order (no racing f32 atomics).  Entry points without a deterministic form
 * return GIC_STATUS_UNSUPPORTED instead (gic_attn_sample_fwd / gic_attn_sample_bwd; the attention decoder's beam searches and teacher-forced decode are accepted), as do the embedding scatters beyond their
 * limit (more than 8192 tokens, or V > 2^19).  It does not hold across GPU models or library builds.
 * The mode is read when work is enqueued: a captured graph keeps the kernels of the mode it was captured in.
 * gic_set_deterministic returns 0; gic_get_deterministic returns the current mode (0 / 1). */
int gic_set_deterministic(int on);
int gic_get_deterministic(void);
/* BatchNorm batch statistics of y [rows, C] (C % 8 == 0) in a fixed order: stats[0..C) = column sums, stats[C..2C) = sums of
 * squares (one replica: consumers take nrep = 1).  slab is f32 scratch of gic_bn_stats_slab_floats(rows, C) floats. */
int gic_bn_stats_slab_floats(int64_t rows, int32_t C, int64_t* out);
int gic_bn_stats(const void* y, int dtype, int64_t rows, int32_t C, float* slab, float* stats, void* stream);

/* ------------------------------------------------------------------------------------------
 * get_losses (src/utils.py:10-53): losses[0]=g_loss, losses[1]=d_loss (device scalars) and, when the
 * d_* pointers are non-NULL, the gradients of d_loss w.r.t. (d_real, d_fake) and of g_loss w.r.t.
 * (g_out, and for rsgan d_real/d_fake through dg_real/dg_fake).
 */
int gic_gan_losses(int loss_type, const float* d_real, const float* d_fake, const float* g_out, int64_t n,
                   float* losses, float* dd_real, float* dd_fake, float* dg_out, float* dg_real, float* dg_fake,
                   void* stream);

/* CrossEntropyLoss over all rows (training.py:81-83): loss = device f32[1+rows] (loss[0] = mean, rest = per-row
 * scratch) and d_logits = (softmax - onehot)/rows (optional).  A target outside [0, V) makes loss[0] NaN (the reference's
 * nn.CrossEntropyLoss raises).  row_weight (optional, f32 [rows]): the policy-gradient form, loss = mean_r w_r * nll_r and
 * d_logits scaled by w_r -- the REINFORCE generator loss of the SeqGAN update with w = the roll-out rewards. */
int gic_xent(const void* logits, int dtype, int64_t rows, int32_t V, const int64_t* targets, float* loss,
             void* d_logits, const float* row_weight, void* stream);

/* Masked, label-smoothed sequence cross entropy with per-caption log-likelihoods (no reference counterpart).
 * logits [rows, V] (f32 / bf16, contiguous), targets int64 [rows]; `group` (>= 1, divides rows) = the rows per caption, row r is position
 * t = r % group of caption b = r / group.  Row (b, t) is COUNTED when targets[r] != ignore_index (any value, -100 ignores nothing real)
 * and, with lengths (optional, int32 [rows / group]), t < lengths[b].  With lp = log_softmax(logits[r]), eps = smoothing in [0, 1) and
 * w = row_weight (optional, f32 [rows]; 1 without):
 *   nll_r = -lp[t_r]     row_r = (1 - eps) nll_r + eps * (-mean_v lp[v])
 *   row_nll f32 [rows]            nll_r of a counted row, else 0 (plain, unsmoothed: the log-likelihood output)
 *   cap_nll f32 [rows / group]    the row_nll of caption b added in index order (optional)
 *   cap_tokens int32 [rows/group] the counted rows of caption b (optional)
 *   loss f32 [2]                  loss[0] = sum over the counted rows of w_r row_r / count, loss[1] = count = sum_b cap_tokens[b]
 *   d_logits [rows, V] (optional, dtype of logits) = w_r (softmax - (1 - eps) onehot(t_r) - eps / V) / count, zeros in an uncounted row
 * row_ws: f32 [rows] scratch.  Every output is written by the call.  With w = 1 this is F.cross_entropy(ignore_index, label_smoothing),
 * values and gradient, with two differences: count = 0 gives loss[0] = 0 and a zero gradient (torch: NaN), and a counted target outside
 * [0, V) makes loss[0] (and its row_nll / cap_nll) NaN as in gic_xent; it is never used as an index.  nll = (max - x_t) + log sum
 * exp(x - max): a common offset of a row's logits costs no digits.  Three launches, no f32 atomics, no host synchronisation; every sum has
 * a fixed order, so two calls give the same bits in either mode of gic_set_deterministic.  GIC_STATUS_INVALID_ARG, before any launch: a
 * NULL logits / targets / loss / row_nll / row_ws, rows <= 0 (or beyond 2^24 - 1: a 256-thread workgroup per row, and the f32 count), V <= 0, group < 1, rows % group != 0, smoothing outside
 * [0, 1) or NaN; GIC_STATUS_UNSUPPORTED: a dtype other than f32 / bf16. */
int gic_xent_seq(const void* logits, int dtype, int64_t rows, int32_t V, const int64_t* targets, int64_t group,
                 const int32_t* lengths, int64_t ignore_index, float smoothing, const float* row_weight, float* loss,
                 float* row_nll, float* row_ws, float* cap_nll, int32_t* cap_tokens, void* d_logits, void* stream);

/* SeqGAN Monte-Carlo rewards (BASELINE config 5; no reference counterpart): mc_logits f32 [(L-1), N, B, R] = D's logits on the
 * N roll-outs of every prefix length 1..L-1 (caption b, representation r), full_logits f32 [B, R] = D on the complete captions.
 * rewards f32 [B, L]: reward[b, t] = mean_{n,r} sigmoid(mc_logits[t, n, b, r]) for t < L-1, mean_r sigmoid(full_logits[b, r]) for
 * t = L-1. */
int gic_rollout_rewards(const float* mc_logits, const float* full_logits, float* rewards, int B, int L, int N, int R, void* stream);

/* ------------------------------------------------------------------------------------------
 * CIDEr-D (Vedantam et al. 2015, the coco-caption CiderScorer; no reference counterpart) of token-id captions, for SCST rewards and
 * evaluation.  A caption's tokens are its first `len` ids with <PAD> = 0, <S> = 1 and <E> = 2 removed.  For
 * n = 1..4, vec_n[g] = count(g) * idf(g), idf(g) = log N - log max(1, df(g)) from the document-frequency table (keys / idf, built on the
 * host from a reference corpus of N images; an n-gram absent from it has idf = log_n); length = the caption's number of bigrams;
 * sim_n(c, r) = sum_g min(vec_n^c[g], vec_n^r[g]) * vec_n^r[g] / (|vec_n^c| |vec_n^r|) (the division only when both norms are non-zero)
 * * exp(-(len_c - len_r)^2 / 72); score(c) = 10 * mean_n(sum_{r in R} sim_n(c, r)) / |R| (0 for an image without references).
 *   table    keys uint64 [K] sorted ascending, unique: bits 60..61 = n - 1, then the n token ids (15 bits each) from bit 45 down, the
 *            unused slots zero; idf f32 [K]; log_n = log N.
 *   cand     cand_ids int64 [n_cand, ld_cand] (row c: Lc ids), cand_len int32 [n_cand], cand_img int32 [n_cand] in [0, B) (a
 *            candidate outside it scores NaN); scores f32 [n_cand].
 *   refs     ref_ids int64 [n_ref, ld_ref] (row: Lr ids), ref_len int32 [n_ref]; image b owns rows ref_off[b] .. ref_off[b+1]
 *            (ref_off int32 [B+1]) and at most max_refs of them (the host knows the largest count; an image with more, or offsets
 *            outside [0, n_ref], scores NaN and nothing past them is read).  Lengths are clamped to [0, Lc] / [0, Lr].
 * Limits: Lc, Lr <= GIC_CIDER_MAX_LEN, max_refs <= GIC_CIDER_MAX_REFS and V <= GIC_CIDER_MAX_VOCAB (the 15-bit keys) -- beyond them
 * GIC_STATUS_UNSUPPORTED; negative sizes, V < 1, a stride below its row length, a log_n that is negative or not finite, B = 0 with
 * candidates and NULL pointers GIC_STATUS_INVALID_ARG; all checked before any launch.  No workspace.  Fixed-order sums and no atomics:
 * two calls give the same bits, and the deterministic mode accepts every call. */
#define GIC_CIDER_MAX_LEN 64
#define GIC_CIDER_MAX_REFS 32
#define GIC_CIDER_MAX_VOCAB 32768
int gic_cider_d(const int64_t* cand_ids, int64_t ld_cand, const int32_t* cand_len, const int32_t* cand_img, int32_t n_cand, int32_t Lc,
                const int64_t* ref_ids, int64_t ld_ref, const int32_t* ref_len, const int32_t* ref_off, int32_t n_ref, int32_t Lr,
                int32_t B, int32_t max_refs, const uint64_t* keys, const float* idf, int64_t K, float log_n, int32_t V, float* scores,
                void* stream);

/* Pairwise CIDEr-D among the K captions of each image (no reference counterpart; an addition to ABI v5), for
 * consensus (minimum-Bayes-risk) selection and the Self-CIDEr diversity of Wang & Chan (CVPR 2019).  ids int64 [B, K, ld_ids] (row:
 * L ids), lengths int32 [B, K] (clamped to [0, L]); tokens, vectors, idf table, length and sigma exactly as gic_cider_d above.
 *   matrix     f32 [B, K, K]: M[b,i,j] = the CIDEr-D (0..10) of caption i as the candidate against caption j as the single reference.
 *              Not symmetric (the clipping min(v_i, v_j) v_j is not); M[b,i,i] = 2.5 * #{n : vec_n of caption i is non-zero}.
 *   consensus  f32 [B, K]: (1 / (K - 1)) sum_{j != i} M[b,i,j], j ascending; 0 for K = 1.
 *   self_cider f32 [B]: with S = (M + M^T) / 20, clamp(-ln(lambda_max(S) / trace(S)) / ln K, 0, 1); 0 for K = 1 or trace(S) = 0.
 *              lambda_max: GIC_CIDER_PAIR_SQUARINGS trace-normalised squarings of S, then the Rayleigh quotient of S at the row sums
 *              of the power (= 2^squarings power-iteration steps from the all-ones vector), always that many, in a fixed order.
 * Each output may be NULL (at least one is given).  One workgroup per image, one launch, no workspace, no atomics: two calls give the
 * same bits, and the deterministic mode accepts every call.  Refused before any launch with GIC_STATUS_INVALID_ARG and a message that
 * names the argument: K outside 1..GIC_CIDER_PAIR_MAX_K, L outside 1..GIC_CIDER_MAX_LEN, V outside 1..GIC_CIDER_MAX_VOCAB, B < 1,
 * n_keys < 0, ld_ids < L, NULL ids / lengths / keys / idf (the table only with n_keys > 0), all three outputs NULL, a log_n that is
 * negative or not finite. */
#define GIC_CIDER_PAIR_MAX_K 32
#define GIC_CIDER_PAIR_SQUARINGS 16
int gic_cider_pairwise(const int64_t* ids, int64_t ld_ids, const int32_t* lengths, int32_t B, int32_t K, int32_t L, const uint64_t* keys,
                       const float* idf, int64_t n_keys, float log_n, int32_t V, float* matrix, float* consensus, float* self_cider,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * N-gram overlap metrics of token-id captions (no reference counterpart): the per-candidate terms of corpus
 * BLEU-1..4 (Papineni et al. 2002, with the semantics of utils.bleu_score), ROUGE-L (Lin 2004, the coco-caption Rouge, beta = 1.2) and an
 * add-one smoothed sentence BLEU-4 (Lin & Och 2004; NLTK's smoothing method 2) for rewards.  Candidates and references have exactly the
 * layout, stripping (<PAD> = 0, <S> = 1, <E> = 2 removed from the first `len` ids) and clamping rules of gic_cider_d above; len_c / len_r
 * below are the stripped lengths, count_x(g) the occurrences of the n-gram g in caption x, r ranges over the image's references.
 *   stats    int32 [n_cand, GIC_OVERLAP_STATS]:
 *              [0..3]  clipped_n, n = 1..4 = sum over the candidate's distinct n-grams g of min(count_c(g), max_r count_r(g))
 *              [4..7]  total_n = max(len_c - n + 1, 0)
 *              [8]     len_c
 *              [9]     the closest reference length: the len_r of the minimum over r of (|len_c - len_r|, len_r) (ties: the shorter)
 *            summed over a corpus they are the integers of corpus BLEU: p_n = sum clipped_n / sum total_n, BP = exp(min(1 - r/c, 0))
 *            with c = sum [8] and r = sum [9].
 *   rouge    f32 [n_cand]: with lcs_r the length of the longest common subsequence of the candidate and reference r, P = max_r lcs_r /
 *            len_c, R = max_r lcs_r / len_r (a reference of length 0 contributes 0); (1 + beta^2) P R / (R + beta^2 P) when both are
 *            positive, else 0.
 *   sbleu    f32 [n_cand]: p_1 = clipped_1 / total_1, p_n = (clipped_n + 1) / (total_n + 1) for n = 2..4, BP = exp(min(1 - r/c, 0)) with
 *            c = len_c and r = the closest reference length; BP * exp(1/4 sum_n log p_n), and 0 when clipped_1 = 0.
 * An image without references gives all-zero stats and scores.  A candidate whose cand_img is outside [0, B), or whose image has more
 * than max_refs references or offsets outside [0, n_ref], gets NaN scores and stats -1, and nothing past the offsets is read.
 * Limits: Lc, Lr <= GIC_CIDER_MAX_LEN, max_refs <= GIC_CIDER_MAX_REFS and V <= GIC_CIDER_MAX_VOCAB -- beyond them GIC_STATUS_UNSUPPORTED;
 * negative sizes, V < 1, a stride below its row length, B = 0 with candidates and NULL pointers GIC_STATUS_INVALID_ARG; all checked
 * before any launch.  No idf table, no workspace.  Integer sums and fixed-order loops, no atomics: two calls give the same bits, and
 * the deterministic mode accepts every call. */
#define GIC_OVERLAP_STATS 10
int gic_caption_overlap(const int64_t* cand_ids, int64_t ld_cand, const int32_t* cand_len, const int32_t* cand_img, int32_t n_cand,
                        int32_t Lc, const int64_t* ref_ids, int64_t ld_ref, const int32_t* ref_len, const int32_t* ref_off, int32_t n_ref,
                        int32_t Lr, int32_t B, int32_t max_refs, int32_t V, int32_t* stats, float* rouge, float* sbleu, void* stream);

/* ------------------------------------------------------------------------------------------
 * optimize(): clip_grad_norm_ + Adam (src/training.py:194-199, :24-26) over a flat f32 parameter arena.
 * step_count: device int64 (incremented here); norm_out: device f32 (pre-clip global L2 norm);
 * partials: device f32 scratch [gic_clip_adam_partials(n)].  Hyper-parameters are doubles: torch.optim.Adam forms
 * 1-beta, lr/(1-beta1^t) and sqrt(1-beta2^t) in Python float64 before touching f32 tensors, and so does the kernel.
 */
int64_t gic_clip_adam_partials(int64_t n);
int gic_clip_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                  double beta1, double beta2, double eps, double clip_norm, int64_t* step_count, float* norm_out,
                  float* partials, void* stream);

/* gic_clip_adam with a learning-rate schedule, decoupled weight decay (torch.optim.AdamW) over arena ranges and an exponential moving
 * average of the parameters, all inside the same two launches.  With t the step counter after this call's increment and s = t - 1:
 *   schedule   lr_t = lr * lambda(s) in float64 (torch.optim.lr_scheduler.LambdaLR: the t-th step uses lambda(t - 1)).  With W =
 *              warmup_steps, T = total_steps, r = min_ratio, u = s - W, D = T - W:  s < W: (s + 1) / W;  else NONE 1;
 *              LINEAR r + (1 - r) max(0, 1 - u/D);  COSINE r + (1 - r) (1 + cos(pi min(1, u/D))) / 2;
 *              INVSQRT max(r, sqrt(max(W, 1) / (s + 1)));  STEP max(r, gamma^floor(u / step_size)).
 *   decay      p *= (float)(1 - lr_t * weight_decay) before the Adam update, for the elements inside the range table only
 *              (weight_decay = 0 or n_ranges = 0: nothing is multiplied).
 *   Adam       as gic_clip_adam, with the step size lr_t / (1 - beta1^t).
 *   EMA        with k = ema_count before the call (the call increments it, as it does step_count): d_k = ema_warmup ?
 *              min(ema_decay, (1 + k) / (10 + k)) : ema_decay;  a = (float)(1 - d_k);  ema += (p_new - ema) * a.  ema NULL: none.
 *   sched_out  optional device f32[2]: lr_t rounded to f32, and a (0 without an EMA).
 * The range table holds n_ranges half-open element ranges [start, end) as int64 pairs, sorted, non-empty and disjoint, every boundary
 * a multiple of 4 (arena slots are 16-byte aligned), at most GIC_ADAMW_MAX_RANGES of them.  It is passed twice: `ranges_host` (host
 * memory) is validated on every call before anything is launched, `ranges` is its copy in device memory, which the kernel reads.
 * Neutral options (weight_decay 0, GIC_LR_NONE, warmup_steps 0, no ema) give gic_clip_adam's outputs bit for bit.  Invalid options
 * (negative weight_decay, min_ratio outside [0, 1], LINEAR / COSINE with total_steps <= warmup_steps, STEP without a positive
 * step_size, ema_decay outside [0, 1), a refused table) return GIC_STATUS_INVALID_ARG with nothing launched.  No atomics. */
#define GIC_ADAMW_MAX_RANGES 256
enum { GIC_LR_NONE = 0, GIC_LR_LINEAR = 1, GIC_LR_COSINE = 2, GIC_LR_INVSQRT = 3, GIC_LR_STEP = 4 };
typedef struct gic_adamw_opts {
  double weight_decay;
  const int64_t* ranges_host;   /* host   int64 [2 * n_ranges] */
  const int64_t* ranges;        /* device int64 [2 * n_ranges], the same values */
  int32_t n_ranges;
  int32_t schedule;             /* GIC_LR_* */
  int64_t warmup_steps, total_steps, step_size;
  double min_ratio, gamma;
  float* ema;                   /* device f32 [n] shadow arena, or NULL */
  int64_t* ema_count;           /* device int64, with ema */
  double ema_decay;
  int32_t ema_warmup;
  int32_t reserved;
  float* sched_out;             /* device f32 [2], or NULL */
} gic_adamw_opts;
int gic_clip_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                   double beta1, double beta2, double eps, double clip_norm, int64_t* step_count, float* norm_out,
                   float* partials, const gic_adamw_opts* opts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GICAP_H_ */
