// Internal host-side launchers shared between translation units (all enqueue on `stream`).
#pragma once
#include "common.h"
#include "gemm.h"

struct gic_sched_sample_opts;
struct gic_decoder_dropout;

namespace gic {

// dst[r*ldd + c] = cast(src[r*lds + c])
int cast2d(const void* src, int src_dtype, long lds, void* dst, int dst_dtype, long ldd, long rows, long cols,
           hipStream_t stream);
// out[c] (+)= sum_r A[r*lda + c]   (A in `dtype`, out f32; out2 optional second destination).  scratch (optional, scratch_floats
// f32): room for the deterministic mode's per-block-row partials (without it that mode runs at most two block rows)
int colsum(const void* A, int dtype, long lda, long rows, long cols, float* out, float* out2, int accumulate,
           hipStream_t stream, float* scratch = nullptr, long scratch_floats = 0);
int embedding_fwd(const float* weight, const int64_t* ids, float* out, long n, int V, int E, hipStream_t stream);
int embedding_bwd(const float* d_out, const int64_t* ids, float* d_weight, long n, int V, int E, int zero_first,
                  hipStream_t stream);
int fill_zero(void* p, size_t bytes, hipStream_t stream);
// dst[c][r] = src[r][c] for a row-major [rows, cols] matrix of `dtype`
int transpose2d(const void* src, void* dst, int dtype, long rows, long cols, hipStream_t stream);

// decoder.hip internals shared with attention.hip
int decoder_output_bwd(int dt, int B, int L, int V, int H, const void* probs, const void* d_out, float temperature, const float* t_dev, int pretrain,
                       void* dlogits_ws, const void* wout, const void* hout, float* dhout, float* d_wout, float* d_bout, hipStream_t stream);
// the LSTM pointwise step (decoder.hip) of every generic path -- the roll-outs (decoder.hip, attn_rollout.hip), the caption decode's
// LstmGeneric (decode.hip) and the teacher-forced LSTM recurrence (teacher_forced.hip): gate pre-activations gpre f32 [rows, 4H],
// c_prev / c_new [rows, H], h into h_next (and h_up, h_out when not null), the activated gates into gates [rows, 4H] when not null.
// With lengths (int32 [rows]; h_prev then = the act rows of h_{t-1}) a row with t >= lengths[b] keeps (h, c): pack_padded_sequence
int lstm_pointwise_fwd(int dt, const float* gpre, const float* c_prev, float* c_new, void* h_next, long ld_next, void* h_up, long ld_up,
                       int rows, int H, hipStream_t stream, void* h_out = nullptr, long ld_out = 0, float* gates = nullptr,
                       const int32_t* lengths = nullptr, int t = 0, const void* h_prev = nullptr, long ld_prev = 0);
// the generic roll-out's per-step launches (decoder.hip), shared with the attention decoder's roll-out (attn_rollout.hip):
//   rollout_join    rows [r0, r1) of dst_xh / dst_c = the rows r % srcB of src_xh / src_c (rows of rowbytes bytes / H floats)
//   rollout_pick    after gemm_gumbelmax: ids[r * ids_stride] = the index of rowkey[r] (or the forced id) and its embedding row into x_next
//   rollout_argmax  after the plain vocabulary product into logits f32 [rows, V]: the per-row Gumbel-softmax, its argmax into ids and the
//                   embedding row into x_next; out (act, rows out_stride apart) may be null
int rollout_join(const unsigned char* src_xh, unsigned char* dst_xh, long rowbytes, const float* src_c, float* dst_c, int H, long r0, long r1,
                 int srcB, hipStream_t stream);
int rollout_pick(int dt, const unsigned long long* rowkey, int64_t* ids, long ids_stride, const float* embed, void* x_next, long ld_x, int rows,
                 int V, int E, const int64_t* force_ids, const int32_t* force_len, int t, hipStream_t stream);
int rollout_argmax(int dt, float* logits, const float* u, uint64_t seed, uint64_t rng_stream, float temperature, int pretrain, void* out,
                   long out_stride, int64_t* ids, long ids_stride, const float* embed, void* x_next, long ld_x, int rows, int V, int E,
                   const int64_t* force_ids, const int32_t* force_len, int t, hipStream_t stream);
// determinism.hip: the process-wide deterministic mode (gic_set_deterministic) and its ordered embedding scatter:
// dst[id(r) * d_id + e * d_e] += sum over tokens r of src[(r + row_off) * ld + e] (ascending r), id(r) = ids[(r % B) * s_b + (r / B) * s_t]
int det_mode();
int det_scatter(const void* src, int dt, long ld, long row_off, const int64_t* ids, int B, long s_b, long s_t, long n, float* dst,
                long d_id, long d_e, int E, int V, hipStream_t stream);
// the teacher-forced decode's epilogue (teacher_forced.hip), beside the Gumbel-softmax kernel it launches (decoder.hip): per-row
// Gumbel-softmax of logits [rows, V] into out (no ids)
int gumbel_softmax_rows(int dt, float* logits, const float* u, uint64_t seed, uint64_t rng_stream, float temperature, int pretrain, void* out,
                        long rows, int V, hipStream_t stream);
int embed_scatter_time(const float* dx, long ld, const int64_t* ids, float* d_embed, int B, int L, int E, int V, hipStream_t stream, long ids_stride = 0);

// sched_sample.hip: scheduled sampling inside the teacher-forced decodes (gic_decoder_forward_ss, gic_attn_forward_ss).
//   ss_check_opts    the argument checks of gic_sched_sample_opts (`what` names the entry point in the message)
//   ss_step_logits   logits[b, t, :] = hout[b, t, :] W_out^T + b_out in f32 for every caption b (hout act [B, Tmax, H], logits [B, Tmax, V]);
//                    fused: vocab_step_logits (the caller's B <= decoder_fused_rows, decoder_step.h) instead of the GEMM
//   ss_pick          between steps t-1 and t: coin, pick and the pick's embedding row into x_next (= x of slot t), one launch
//   ss_tail          inputs[:, from:] = caps[:, from:], replaced = 0 there (the positions no step is fed from)
struct SsPickArgs {
  const float* logits = nullptr; long ld_logits = 0;    // f32 logits of step t-1: row b at logits + b * ld_logits
  const int64_t* caps = nullptr;                        // [B, Tm1]
  const int32_t* lengths = nullptr;                     // [B]
  const float* coin_u = nullptr;                        // [B, Tm1] or null -> Philox(seed)
  const float* noise_u = nullptr;                       // [Tm1, B, V] or null -> Philox(seed); unread when pick != 0
  uint64_t seed = 0;
  float prob = 0.f; int pick = 0;                       // 0 = sample (Gumbel-max), 1 = argmax
  int t = 0;                                            // the step whose input is decided, 1..Tm1
  int B = 0, V = 0, E = 0, Tm1 = 0;
  const float* embed = nullptr;                         // f32 [V, E]
  void* x_next = nullptr; long ld_x = 0;                // act rows of slot t: columns [0, E) of row b receive embed[pick]
  int64_t* inputs = nullptr; int32_t* replaced = nullptr;   // [B, Tm1]; replaced may be null
};
int ss_check_opts(const gic_sched_sample_opts* o, int L, const char* what);
int ss_step_logits(int dt, const void* hout, int t, int Tmax, const void* wout, const float* b_out, float* logits, int B, int V, int H,
                   bool fused, hipStream_t stream);
int ss_pick(const SsPickArgs& a, int dt, hipStream_t stream);
int ss_tail(const int64_t* caps, int64_t* inputs, int32_t* replaced, int B, int Tm1, int from, hipStream_t stream);

// gen_dropout.hip: output dropout of the caption decoder (gic_decoder_dropout), the stage between hout and the vocabulary projection.
//   drop_check          the argument checks of gic_decoder_dropout (`who` names the entry point in the message)
//   hidden_dropout_fwd  y = keep ? x * s : 0 over x / y act [B, Tmax, H]: every row (step < 0) or the B rows of step `step`
//   hidden_dropout_bwd  in place: dhout f32 [B, Tmax, H] = (t < lengths[b] && keep) ? dhout * s : 0
// keep is drawn from Philox(seed) or read from keep_u (f32 [B, Tmax, H]); both index it by the flat element index (gen_dropout.hip)
int drop_check(const gic_decoder_dropout* d, const char* who);
int hidden_dropout_fwd(int dt, const void* x, void* y, const float* keep_u, uint64_t seed, float p, int B, int Tmax, int H, int step,
                       hipStream_t stream);
int hidden_dropout_bwd(float* dhout, const int32_t* lengths, const float* keep_u, uint64_t seed, float p, int B, int Tmax, int H,
                       hipStream_t stream);

// disc_cond.hip: the conditioned discriminator's match-term backward for disc_bwd_t (disc.hip): dydrop[m, :] = scale g[m] q[m / R, :]
// (f32 [B*R, Fp], pad columns zero) and, when d_q is not null, d_q[b, :] = scale sum_r g[b R + r] ydrop[b R + r, :F] (f32 [B, F])
int disc_match_bwd(int dt, const void* ydrop, const float* q, const float* g, float scale, float* dydrop, float* d_q, int B, int R, int F,
                   int Fp, hipStream_t stream);

}  // namespace gic
