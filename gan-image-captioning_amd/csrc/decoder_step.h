// Fused per-timestep kernels of the caption roll-out (reference src/generator.py:60-76) -- launchers shared with decoder.hip.
//
// One decode step = TWO launches (the two all-to-all seams of the step: every hidden unit feeds every vocabulary logit, and
// every logit feeds the argmax that selects the next input):
//   lstm_step   [argmax of the previous step's partials -> next-input embedding gather] -> gates GEMM on MFMA -> LSTM pointwise
//   vocab_step  vocabulary GEMM on MFMA -> + bias + Gumbel(u) -> * temperature -> per-tile softmax partials (max, sum, argmax)
//               and the UNNORMALISED probabilities e = exp(y - tile max)
// and one launch after the last step (sample_finish): global max / sum per (caption, step) from the partials, token ids,
// probabilities p = e * exp(tile max - global max) / global sum.
// A grid-wide barrier inside one persistent launch costs 4.1-4.8 us on this chip (MI355X_MICROARCH.md price list, barrier-xcd; the
// single-launch roll-out built in round 2 measured ~19 us per barrier with the step's dirty lines to write back: 943 us per roll-out
// against 423 us; removed in round 3) against 1.45 us for a dependent kernel boundary, so the seams stay kernel
// boundaries and each kernel is sized to its floor:
// the 14 MB of decoder weights stay resident in the eight XCD L2s (4 MB each) between steps because the block -> weight-slice
// map is the same in every step.
#pragma once
#include "../../include/gicap.h"
#include "common.h"

struct gic_decoder_dims;
struct gic_decoder_params;
struct gic_decoder_shadow;
struct gic_decoder_state;
struct gic_decoder_bwd_ws;
struct gic_decoder_grads;
struct gic_attn_dims;
struct gic_attn_params;
struct gic_attn_shadow;
struct gic_attn_state;
struct gic_attn_bwd_ws;
struct gic_attn_grads;

namespace gic {

constexpr int kStepRows = 64;      // batch rows per block (4 MFMA tiles)
constexpr int kVocabTile = 64;     // vocabulary entries per vocab_step block
constexpr int kUnitsPerBlock = 4;  // hidden units per lstm_step block (4 gates x 4 units = one 16-wide MFMA tile)

struct LstmStepArgs {
  const void* xh_t = nullptr;        // act [B, ldx]: [x_t | h_{t-1}] (the x part is ignored when `gather`)
  void* xh_next = nullptr;           // act [B, ldx]: h_t is written at [:, din:]
  const void* wcat = nullptr;        // act [4H, ldx] = [w_ih | w_hh]
  const float* bsum = nullptr;       // [4H]
  const float* c_prev = nullptr;     // [B, H]
  float* c_new = nullptr;            // [B, H]
  float* gates = nullptr;            // [B, 4H] post-activation i,f,g,o (saved for backward) or null
  void* h_up = nullptr; long ld_up = 0;     // act: next layer's input slot, or null
  void* h_out = nullptr; long ld_out = 0;   // act: hout[b, t, :], or null
  int B = 0, H = 0, din = 0; long ldx = 0;
  // layer 0, t > 0: x_t = embed[id_{t-1}], id = argmax over the previous step's partials (or the forced trajectory)
  int gather = 0;
  int gw = 0;                        // width of the gathered x (= embedding dim): columns [0, gw) of the input; 0 = din
  const float* embed = nullptr; int V = 0;
  const unsigned long long* rowkey = nullptr;      // [B] argmax keys of step t-1 (vocab_step's atomicMax; see row_key())
  const int64_t* force_ids = nullptr; long force_stride = 0; const int32_t* force_len = nullptr; int tprev = 0;
  // beam search (beam.h), all optional: with every one null the kernel is the roll-out's
  const int32_t* parent = nullptr;   // [B]: the h part of xh_t and c_prev are read from row parent[r]
  const int32_t* token = nullptr;    // [B]: the gathered x part is embed[token[r]] (needs `gather`)
  const int32_t* stop = nullptr; int stop_at = 0;  // *stop >= stop_at: return at once (every beam has finished)
  // teacher-forced decode (teacher_forced.hip AttnTf), optional: with pack_len, a row with pack_t >= pack_len[b] keeps (h, c) (pack_padded_sequence)
  // and writes a zero h_out row and zero gates; not combined with the beam arguments
  const int32_t* pack_len = nullptr; int pack_t = 0;
  int dbg = 0;
};

struct VocabStepArgs {
  const void* h = nullptr; long ldh = 0;     // act rows: h + b*ldh, H values each
  const void* wout = nullptr;                // act [V, H]
  const float* bias = nullptr;               // [V]
  const float* u = nullptr;                  // explicit uniforms [B, V] of this step, or null -> Philox(seed, rng_stream)
  uint64_t seed = 0, rng_stream = 0;
  float temperature = 1.f;
  const float* t_dev = nullptr;              // non-null: temperature / seed are read from device memory (gic_step_scalars), the values
  const uint64_t* seed_dev = nullptr;        // above are ignored
  int pretrain = 0;
  void* out = nullptr; long out_stride = 0;  // act: out + b*out_stride + v (e or raw logits); null: ids only
  float* part_m = nullptr; float* part_s = nullptr; int nblk = 0;   // [B][nblk] per-tile max / sum of exp
  unsigned long long* rowkey = nullptr;      // [B], zeroed by the caller: atomicMax of (ordered tile max, ~first maximal index)
  float* part_v = nullptr; int32_t* part_i = nullptr;   // beam epilogue only (vocab_step_beam): [B][nblk][K] tile top-K pairs
  const int32_t* stop = nullptr; int stop_at = 0;         // beam / logits epilogues only: *stop >= stop_at -> return at once
  float* logits = nullptr; long ld_logits = 0;            // logits epilogue only (vocab_step_logits): f32 o + b_out [B][ld_logits]
  int B = 0, V = 0, H = 0;
  int dbg = 0;
};

struct SampleFinishArgs {
  const float* part_m = nullptr; const float* part_s = nullptr;   // [L][B][nblk]
  const unsigned long long* rowkey = nullptr;                       // [L][B]
  int nblk = 0, B = 0, L = 0, V = 0, E = 0;
  int pretrain = 0;
  void* out = nullptr;                       // act [B, L, V] or null
  int64_t* ids = nullptr;                    // [B, L]
  const int64_t* force_ids = nullptr; const int32_t* force_len = nullptr;
  const float* embed = nullptr; void* xh0 = nullptr; long ldx0 = 0;     // x rows of XH_0 slots 1..L-1 (for the weight gradient) or null
};

// One BPTT step of one layer (reverse of lstm_step): dh = dh_above + dgates_{t+1} W_hh [+ dgates^{l+1}_t W_ih^{l+1}], then the
// cell's pointwise backward -> dgates_t, dc.  Tile = 16 batch rows x 16 hidden units per block, K (= 4H per segment) split over
// the 8 waves, operands straight from L2 (the k-contiguous operand of W is the transposed weight image wcat_t).
struct LstmBwdStepArgs {
  const float* dh_above = nullptr; long ld_above = 0;   // f32 rows (top layer: dhout[b, t, :]) or null
  const float* dh_extra = nullptr;                      // f32 [B, H] added as is (attention decoder: gradient through W_h h_{t-1}) or null
  int zero_extra = 0;                                   // != 0: dh_extra is zeroed behind the read (the next split-K product adds into it)
  const void* dg_next = nullptr;                        // act [B, 4H] dgates of step t+1, this layer (null at t = L-1)
  const void* w_rec = nullptr;                          // act rows j of wcat_t (+ din rows): [H][4H], W_hh^T
  const void* dg_up = nullptr;                          // act [B, 4H] dgates of step t, layer l+1 (null for the top layer)
  const void* w_up = nullptr;                           // act rows j of the upper layer's wcat_t: [H][4H], W_ih^{l+1,T}
  const float* gates = nullptr;                         // [B, 4H] post-activation i,f,g,o of step t
  const float* c_prev = nullptr; const float* c_cur = nullptr;   // [B, H]
  float* dc_state = nullptr;                            // [B, H] in/out
  int dc_zero = 0;                                      // != 0: dc_state is taken as zero instead of read (the first step of a chain, t = L-1:
                                                        // no zero fill in front of the chain); it is written as always
  void* dgates = nullptr;                               // act [B, 4H] out
  int B = 0, H = 0;
};
int lstm_bwd_step(const LstmBwdStepArgs& a, int dtype, hipStream_t stream);

// THE predicate "fused step kernels or generic products": the most batch rows for which a pass over these shapes runs lstm_step /
// vocab_step* (up to a few hundred rows the per-step products are latency-bound; beyond that they are large GEMMs and the generic
// 128-row-tile kernels are the efficient form), 0 where the kernels do not take the shapes at all.  V >= 4, V % 4 == 0, E % 8 == 0,
// H % 8 == 0, NL >= 1, at most 1024 vocabulary tiles (sample_finish's scale table); the rows are GIC_FUSED_ROLLOUT_MAX_ROWS (default
// 512); GIC_NO_FUSED_ROLLOUT switches every fused pass off.  Every caller compares its rows with this one answer.
int decoder_fused_rows(int dtype, int V, int E, int H, int NL);
// the backward's own condition, lstm_bwd_step's chain: H % 8 == 0 (the transposed images' 16-byte rows; the kernel's unit pairs need
// H % 2 == 0), NL >= 1, the same row limit and switch -- V and E do not enter it.  The caller adds that every wcat_t[l] exists.
int decoder_bwd_fused_rows(int H, int NL);
int decoder_step_max_rows();                                // the row limit alone (GIC_FUSED_ROLLOUT_MAX_ROWS), for messages
size_t decoder_step_part_floats(int B, int L, int V);       // floats in the partials scratch: [2][L][B][nblk] floats + [L][B] 64-bit keys + 4 reserved words
void decoder_step_debug(int v);                             // phase-ablation knob of tools/rollout_bench.py (0 = normal)

// The partials scratch (state->part) of a fused roll-out of L steps over B rows, carved: the one place that knows its layout
// (decoder_step_part_floats sizes it).  The two fused roll-outs (decoder.hip sample_fwd_fused, attention.hip attn_fwd_t) zero the
// keys once, take step t's vocab_step arguments and the sample_finish arguments from here and add their decoder's own fields.
struct StepScratch {
  float* part_m; float* part_s;      // [L][B][nblk] per-tile max / sum of exp
  unsigned long long* rowkey;        // [L][B] argmax keys, 8-byte aligned: atomicMax targets, zeroed before step 0
  int nblk, B, L, V;
  unsigned long long* keys(int t) const { return rowkey + (long)t * B; }
  size_t key_bytes() const { return (size_t)L * B * sizeof(unsigned long long); }
};
StepScratch decoder_step_scratch(float* part, int B, int L, int V);
// what a roll-out draws with and writes, the same for every step: explicit uniforms [L, B, V] or Philox(seed, stream t), the scalars
// (t_dev / seed_dev: read from device memory instead), out act [B, L, V] or null, ids [B, L]
struct StepDraw {
  const float* noise_u; uint64_t seed; float temperature; int pretrain;
  const float* t_dev; const uint64_t* seed_dev;
  void* out; int64_t* ids;
};
// step t's vocab_step arguments but the decoder's own (h, ldh, wout, bias, H); sample_finish's but force_ids / force_len and the
// x rows (embed, xh0, ldx0)
VocabStepArgs step_vocab_args(const StepScratch& s, const StepDraw& d, int t, int dtype);
SampleFinishArgs step_finish_args(const StepScratch& s, const StepDraw& d, int E);
int lstm_step(const LstmStepArgs& a, int dtype, hipStream_t stream);
int vocab_step(const VocabStepArgs& a, int dtype, hipStream_t stream);
int sample_finish(const SampleFinishArgs& a, int dtype, hipStream_t stream);
// the vocabulary product of vocab_step with the logits epilogue: a.logits = o + b_out in f32, the roll-out's bits before its noise
// (caption sampling, sample.hip); a.stop / stop_at; the sampling and beam fields are unused
int vocab_step_logits(const VocabStepArgs& a, int dtype, hipStream_t stream);

// ---- the launchers' plans (gemm.h's convention: select_* is a pure host function that fills a plan, launch_* asks for the LDS grant,
// switches on the variant and launches).  lstm_step / vocab_step* above and in beam.h are "check the arguments, select, launch".
enum { LSTM_PLAIN, LSTM_PACK, LSTM_BEAM };
enum { VOCAB_SAMPLE, VOCAB_LOGITS, VOCAB_BEAM, VOCAB_BEAM_BAN, VOCAB_BEAM_HOP };      // (the three beam forms last: select_vocab_step)
struct StepPlan {
  bool lstm; int variant, dtype, K;       // K: the beam forms' template argument, else 0
  dim3 grid; int block; size_t lds; int KC;
};
StepPlan select_lstm_step(int variant, int dtype, int B, int H, long ldx);
StepPlan select_vocab_step(int variant, int dtype, int K, int B, int V, int H);
// the plan as one line in the route line's format: kernel<template args> grid=XxY block=.. lds=.. KC=..
void step_plan_line(const StepPlan& p, char* out, size_t len);

// ---- the LSTM decoder's (decoder.hip) shapes, shared with the teacher-forced decode (teacher_forced.hip)
struct DCtx {
  int B, L, V, E, H, NL, dt;
  int din(int l) const { return l == 0 ? E : H; }
  long ldx(int l) const { return (long)din(l) + H; }
  size_t asz() const { return (size_t)dtype_size(dt); }
};
int check_decoder_dims(const gic_decoder_dims* d, DCtx& c);   // B, L, E, H > 0, V > 1, NL in 1..GIC_MAX_LAYERS

// ---- one plan for gic_decoder_sample_fwd / gic_decoder_sample_bwd (decoder.hip: "select, then the stages").  select_decoder_* are pure
// host functions of the shapes and of the facts about the call below; pointers are read for their alignment only.
enum { DEC_FUSED, DEC_GENERIC, DEC_GENERIC_ROWKEY };
struct DecoderFwdCall {
  bool part, resumed, dev_scalars, out, pretrain;      // state->part, opts->resume_from, opts->dev_scalars, out present; pretrain != 0
  const void* logits;                                  // state->logits
};
struct DecoderBwdCall {
  int phases; bool pretrain;
  const void* probs; const void* d_out; const void* dlogits;
  const void* wcat_t[GIC_MAX_LAYERS];                  // presence
  const void* dgates[GIC_MAX_LAYERS]; const void* xh[GIC_MAX_LAYERS];      // the weight-gradient products' operands
};
struct DecoderPlan {
  // forward.  DEC_GENERIC_ROWKEY: the generic path of an ids-only bf16 roll-out, one 64-bit argmax key per (step, row) in the logits
  // scratch and the Gumbel-max in the vocabulary product's epilogue for every step of at least rowkey_from rows (0: no step)
  int fwd = DEC_GENERIC; long rowkey_from = 0;
  // backward: lstm_bwd_step's chain or pointwise + product per (step, layer); per layer ONE weight-gradient product with the bias sums
  // folded in, or two products and colsum; softmax_bwd_vec_kernel's NCH (0: the scalar kernel)
  bool bwd_fused = false; bool wgrad_folded[GIC_MAX_LAYERS] = {}; int softmax_nch = 0;
};
// GIC_OK, or GIC_ERR_UNSUPPORTED with its message: device-resident step scalars off the fused path
int select_decoder_fwd(const DCtx& c, const DecoderFwdCall& f, DecoderPlan& p);
void select_decoder_bwd(const DCtx& c, const DecoderBwdCall& b, DecoderPlan& p);
int select_softmax_bwd(int dt, int V, const void* probs, const void* d_out, const void* dlogits);      // decoder_output_bwd's variant (NCH | 0)
// The steps of a DEC_GENERIC_ROWKEY roll-out: step t's M rows take the fused product iff M >= from and no earlier step was declined --
// after one decline the separate launches run from there on, whatever a later step's rows.
struct RowkeySteps {
  long from; bool on;
  bool sticky = true;                   // gic_attn_rollout: false -- each step on its own rows (its logits scratch holds only the steps below `from`)
  bool take(int M) {
    const bool ok = on && from > 0 && M >= from;
    if (sticky) on = ok;
    return ok;
  }
  void decline() { on = false; }        // the product's own status is the last word (gemm_gumbelmax also reads pointers and the temperature)
};
// decoder.hip: the recurrent phase of gic_decoder_sample_bwd (ws->dhout filled) over c.L steps and the embedding scatter over ids
// (rows ids_stride apart; 0 = c.L)
int decoder_bwd_recurrent(const DCtx& c, const gic_decoder_params* P, const gic_decoder_shadow* S, const gic_decoder_state* st,
                          const gic_decoder_bwd_ws* ws, const int64_t* ids, long ids_stride, const gic_decoder_grads* G, hipStream_t stream);

// ---- the attention decoder's (attention.hip) shapes, shared with its beam search (attn_beam.hip)
struct ACtx {
  int B, L, V, E, H, C, P, A, dt;
  long ldx() const { return (long)E + C + H; }        // xh row [x | z | h]
  int din() const { return E + C; }
  size_t asz() const { return (size_t)dtype_size(dt); }
};
int check_attn_dims(const gic_attn_dims* d, ACtx& c);   // V % 4, E / H / C / A % 8, P <= 1024, A <= 2048
// attention.hip: everything of gic_attn_sample_bwd after the output layer's backward (ws->dhout filled) over c.L steps -- the reverse
// recurrence, the batched weight gradients, d features and the embedding scatter over ids (rows ids_stride apart; 0 = c.L).
// d_alphas: f32 [B, c.L, P] added to d alpha before the softmax backward, or null.
int attn_bwd_recurrent(const ACtx& c, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st, const gic_attn_bwd_ws* ws,
                       const void* fmap, const int64_t* ids, long ids_stride, const float* d_alphas, const gic_attn_grads* G, hipStream_t stream);

// 16 bytes of compute-dtype values as floats: NV = 8 (bf16) or 4 (f32)
template <typename TA> struct Vec16;
template <> struct Vec16<bf16_t> {
  static constexpr int NV = 8;
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
    const bf16x8 x = __builtin_bit_cast(bf16x8, *(const __attribute__((address_space(1))) u4*)p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
    bf16x8 x;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (bf16_t)v[i];
    *(bf16x8*)p = x;
  }
};
template <> struct Vec16<float> {
  static constexpr int NV = 4;
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    const f32x4 x = *(const __attribute__((address_space(1))) f32x4*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = x[i];
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
    *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]};
  }
};

}  // namespace gic
