// Teacher-forced decode (gicap.h gic_decoder_forward_tf, gic_attn_forward_tf, their scheduled-sampling forms gic_*_forward_ss, the
// *_ws_bytes queries and gic_*_forward_tf_bwd; Decoder.forward, reference src/generator.py:39-53): one driver for both decoders.
// The inputs are known before the loop and the sequences are packed (pack_padded_sequence): caption b is live for steps t < lengths[b];
// past its length a row keeps (h, c), writes a zero output row and zero gates.
//
// A forward pass is a recurrence, chosen at the entry point, under one skeleton (teacher_forced<Rec>):
//   before the loop  scheduled sampling: ss_tail (the positions of inputs / replaced that no step is fed from; in front of the
//                    attention decoder's begin(), behind the LSTM decoder's); the recurrence's begin(): its slots zeroed,
//                    x_0 = features, x_t = embed(caps[:, t-1]) gathered once for every step (tf_inputs), and what it computes once
//   per step t       the recurrence's step(t): h_t into slot t + 1 of its xh and into hout[:, t, :] ([B, Tmax, H]); under scheduled
//                    sampling then the logits of step t (ss_step_logits) and ss_pick, which decides the x rows of slot t + 1 from
//                    them (rows it does not replace keep the teacher's embedding)
//   after the loop   one vocabulary product over B * Tmax rows (scheduled sampling: the logits are there already), the Gumbel-softmax
//                    epilogue (gumbel_softmax_rows; the draw u is [B, Tmax, V]), h_n / c_n out of slot Tmax, where every row's state
//                    at its own last step sits
// with
//   LstmTf  begin: slot 0 of every layer zeroed.  step: per layer the library GEMM into gpre and lstm_pointwise_fwd with lengths
//           (decoder.hip), h_up into the next layer's slot t.  The gate GEMMs never split K under scheduled sampling (the picks are
//           discrete: the same inputs must give the same bits) and may otherwise; the final vocabulary product may always
//   AttnTf  begin: slots 0..Tmax of xh zeroed (z of padded rows stays zero: finite operands of the weight gradients), c_0 = 0,
//           fp = fmap W_f^T + b_f (one product over B * P rows).  step: hp [B, A] = h_{t-1} W_h^T (the library GEMM), attn_step -- the
//           caption decode's attention kernels (attn_beam.hip) in their packed form at k = 1: a caption past its length returns from
//           both at once (one zero alpha row) -- and lstm_step in its packed form (decoder_step.h LstmStepArgs.pack_len).  The
//           energies [B, P] lie in logits_ws, behind the logits under scheduled sampling (which forms them inside the loop).  No GEMM
//           of it splits K and it adds no f32 atomically, so its forward gives the same bits on every call in either mode.
//
// Backward: decoder_output_bwd over B * Tmax rows, dhout zeroed past the lengths (pad_packed_sequence's constant zeros: no gradient
// reaches the recurrence from a padded step), then the decoder's own recurrent backward on the Tmax view of the saved state:
// decoder_bwd_recurrent (decoder.hip; caps stand in for the sampled ids) or attn_bwd_recurrent (attention.hip; with the d alphas added
// in front of the softmax backward).  The zero alpha rows of padded steps make their attention terms vanish, their zero gates / zero
// dhout rows the LSTM terms.
//
// Output dropout (gen_dropout.hip; the gic_*_drop entry points, io.drop / g.drop set): hidden_dropout_fwd writes drop->hdrop from hout
// -- over all rows after the loop, or under scheduled sampling over the rows of step t in front of ss_step_logits -- and the vocabulary
// product reads hdrop; the backward gives decoder_output_bwd hdrop for hout and runs hidden_dropout_bwd where zero_past_length stood.
// Neither recurrence changes: the state keeps the undropped h.  With drop null not one launch, argument or check differs.
//
// Entry path: every extern "C" function is a model (LstmTrain / AttnTrain: the decoder's dims, weights, state and, with attention,
// the feature map; its shape check, its buffer checks with its own texts, run()) and one call of forward_entry, backward_entry or
// ws_bytes_entry.  Order of checks: shapes, null arguments, caps (L = 1 has no caption column), Tmax, then the scheduled-sampling
// options and the workspace's alignment, then the model's buffers; gic_attn_forward_ss is refused by the deterministic mode before
// all of them, gic_attn_forward_tf and gic_attn_forward_tf_bwd are not.  tests/test_train_entry_errors.py pins texts and order with
// a recorded table.
#include <stdio.h>
#include <string.h>

#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

using namespace gic;

// (the two kernels stand at global scope, where they were written: their names in a kernel trace are those of every earlier profile)
// x rows of slots 1..Tm1 of xh0: embed(caps[b, t-1]) (caps rows Tm1 apart)
template <typename TA>
__global__ void embed_rows_tf_kernel(const float* __restrict__ embed, const int64_t* __restrict__ caps, TA* __restrict__ xh0, long ld,
                                     int B, int Tm1, int E, int V) {
  const long total = (long)Tm1 * B * E;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int e = (int)(i % E);
    const long r = i / E;
    const int b = (int)(r % B), t = (int)(r / B) + 1;
    long id = caps[(long)b * Tm1 + (t - 1)];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    xh0[((long)t * B + b) * ld + e] = from_f32<TA>(embed[id * E + e]);
  }
}

// d_hout [B, Tmax, H]: rows past their sequence's length are pad_packed_sequence's constant zeros (generator.py:45): no gradient reaches the LSTM
__global__ void zero_past_length_kernel(float* __restrict__ dhout, const int32_t* __restrict__ lengths, int B, int Tmax, int H) {
  const long total = (long)B * Tmax * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / H;
    const int b = (int)(r / Tmax), t = (int)(r % Tmax);
    if (t >= lengths[b]) dhout[i] = 0.f;
  }
}

namespace gic {
namespace {

int embed_rows_tf(int dt, const float* embed, const int64_t* caps, void* xh0, long ld, int B, int Tm1, int E, int V, hipStream_t stream) {
  if (Tm1 < 1) return GIC_OK;
  const long total = (long)Tm1 * B * E;
  const dim3 grid((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256));
  if (dt == DT_F32) hipLaunchKernelGGL((embed_rows_tf_kernel<float>), grid, dim3(256), 0, stream, embed, caps, (float*)xh0, ld, B, Tm1, E, V);
  else hipLaunchKernelGGL((embed_rows_tf_kernel<bf16_t>), grid, dim3(256), 0, stream, embed, caps, (bf16_t*)xh0, ld, B, Tm1, E, V);
  GIC_CHECK_LAUNCH("embed_rows_tf");
  return GIC_OK;
}

int zero_past_length(float* dhout, const int32_t* lengths, int B, int Tmax, int H, hipStream_t stream) {
  const long total = (long)B * Tmax * H;
  hipLaunchKernelGGL(zero_past_length_kernel, dim3((unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256)), dim3(256), 0, stream,
                     dhout, lengths, B, Tmax, H);
  GIC_CHECK_LAUNCH("zero_past_length");
  return GIC_OK;
}

// what a forward call takes beside its model
struct TfIo {
  const float* features; const int64_t* caps; const int32_t* lengths; int Tmax;
  const float* noise_u; uint64_t seed; float temperature; int pretrain;
  float* logits_ws;              // f32 [B * Tmax, V]; the attention decoder's energies too (AttnTf)
  void* out; float* h_n; float* c_n;
  const gic_sched_sample_opts* ss;         // scheduled sampling, or null
  hipStream_t stream;
  const gic_decoder_dropout* drop = nullptr;      // output dropout (gen_dropout.hip), or null: the gic_*_drop entry points set it
};

void* act(const void* p, long n, size_t asz) { return (char*)p + n * (long)asz; }      // p + n compute-dtype values

// x of every step, known up front: x_0 = features, x_t = embed(caps[:, t-1]) into the x columns of xh0's slots
int tf_inputs(int dt, const TfIo& io, const float* embed, void* xh0, long ld, int B, int T, int E, int V) {
  GIC_PROPAGATE(cast2d(io.features, DT_F32, E, xh0, dt, ld, B, E, io.stream));
  return embed_rows_tf(dt, embed, io.caps, xh0, ld, B, T - 1, E, V, io.stream);
}

// ---- recurrences: begin() once, step(t) leaves h_t in slot t + 1 of the top layer's xh and in hout[:, t, :].  c: the shapes
// (B, L = T, V, E, H, dt); layer l's xh(l) rows are ldx(l) wide with h at column din(l), its cell states cell(l) are [T + 1][B][H]
struct LstmTf {
  static constexpr int kNoSplitVocab = 0;
  static constexpr bool kTailFirst = false;
  const DCtx& c; const gic_decoder_params* P; const gic_decoder_shadow* S; const gic_decoder_state* st;
  int layers() const { return c.NL; }
  int din(int l) const { return c.din(l); }
  long ldx(int l) const { return c.ldx(l); }
  void* xh(int l) const { return st->xh[l]; }
  float* cell(int l) const { return st->c[l]; }
  int begin(const TfIo& io) const {
    for (int l = 0; l < c.NL; ++l) {
      GIC_PROPAGATE(fill_zero(st->xh[l], (size_t)c.B * c.ldx(l) * c.asz(), io.stream));
      GIC_PROPAGATE(fill_zero(st->c[l], (size_t)c.B * c.H * sizeof(float), io.stream));
    }
    return tf_inputs(c.dt, io, P->embed, st->xh[0], c.ldx(0), c.B, c.L, c.E, c.V);
  }
  GemmDesc gates_product(const TfIo& io, int l, int t) const {      // layer l's gate pre-activations of step t
    const long ld = c.ldx(l);
    GemmDesc g;
    g.A = act(st->xh[l], (long)t * c.B * ld, c.asz()); g.lda = ld; g.B = S->wcat[l]; g.ldb = ld; g.C = st->gpre; g.ldc = 4 * c.H;
    g.M = c.B; g.N = 4 * c.H; g.K = (int)ld; g.in_dtype = c.dt; g.out_dtype = DT_F32; g.bias = S->bsum[l];
    g.no_split = io.ss != nullptr;          // the picks are discrete: the same inputs must give the same bits
    return g;
  }
  int route(const TfIo& io) const {          // route-only mode: a step's products, selected in launch order
    for (int l = 0; l < c.NL; ++l) GIC_PROPAGATE(gemm(gates_product(io, l, 0), io.stream));
    return GIC_OK;
  }
  int step(const TfIo& io, int t) const {
    const int B = c.B, H = c.H;
    for (int l = 0; l < c.NL; ++l) {
      const long ld = c.ldx(l);
      void* xh_t = act(st->xh[l], (long)t * B * ld, c.asz());
      void* xh_n = act(st->xh[l], (long)(t + 1) * B * ld, c.asz());
      GIC_PROPAGATE(gemm(gates_product(io, l, t), io.stream));
      const bool top = l + 1 == c.NL;
      GIC_PROPAGATE(lstm_pointwise_fwd(c.dt, st->gpre, st->c[l] + (long)t * B * H, st->c[l] + (long)(t + 1) * B * H, act(xh_n, c.din(l), c.asz()), ld,
                                       top ? nullptr : act(st->xh[l + 1], (long)t * B * c.ldx(l + 1), c.asz()), top ? 0 : c.ldx(l + 1), B, H,
                                       io.stream, top ? act(st->hout, (long)t * H, c.asz()) : nullptr, (long)io.Tmax * H,      // hout viewed as [B, Tmax, H]
                                       st->gates[l] ? st->gates[l] + (long)t * B * 4 * H : nullptr,         // saved for the backward as lstm_step saves them
                                       io.lengths, t, act(xh_t, c.din(l), c.asz()), ld));
    }
    return GIC_OK;
  }
};

struct AttnTf {
  static constexpr int kNoSplitVocab = 1;
  static constexpr bool kTailFirst = true;
  const ACtx& c; const gic_attn_params* P; const gic_attn_shadow* S; const gic_attn_state* st;
  const void* fmap; float* alphas;         // alphas: f32 [B, Tmax, P] or null
  int layers() const { return 1; }
  int din(int) const { return c.din(); }
  long ldx(int) const { return c.ldx(); }
  void* xh(int) const { return st->xh; }
  float* cell(int) const { return st->c; }
  int begin(const TfIo& io) const {
    const long ld = c.ldx();
    GIC_PROPAGATE(fill_zero(st->xh, (size_t)(io.Tmax + 1) * c.B * ld * c.asz(), io.stream));
    GIC_PROPAGATE(fill_zero(st->c, (size_t)c.B * c.H * sizeof(float), io.stream));
    GIC_PROPAGATE(tf_inputs(c.dt, io, P->embed, st->xh, ld, c.B, c.L, c.E, c.V));
    GemmDesc g;                  // fp = fmap W_f^T + b_f
    g.A = fmap; g.lda = c.C; g.B = S->wf; g.ldb = c.C; g.C = st->fproj; g.ldc = c.A;
    g.M = c.B * c.P; g.N = c.A; g.K = c.C; g.in_dtype = c.dt; g.out_dtype = c.dt; g.bias = P->b_f;
    g.no_split = 1;
    return gemm(g, io.stream);
  }
  GemmDesc hp_product(int t) const {          // hp [B, A] = h_{t-1} W_h^T
    GemmDesc g;
    g.A = act(st->xh, (long)t * c.B * c.ldx() + c.din(), c.asz()); g.lda = c.ldx(); g.B = S->wh; g.ldb = c.H;
    g.C = st->hproj + (long)t * c.B * c.A; g.ldc = c.A;
    g.M = c.B; g.N = c.A; g.K = c.H; g.in_dtype = c.dt; g.out_dtype = DT_F32;
    g.no_split = 1;
    return g;
  }
  int route(const TfIo& io) const { return gemm(hp_product(0), io.stream); }      // route-only mode: a step's product
  int step(const TfIo& io, int t) const {
    const int B = c.B, E = c.E, H = c.H, Tmax = io.Tmax;
    const long ld = c.ldx();
    void* xh_t = act(st->xh, (long)t * B * ld, c.asz());
    float* hp = st->hproj + (long)t * B * c.A;
    GIC_PROPAGATE(gemm(hp_product(t), io.stream));
    AttnStepArgs f{};                // par and stop stay null: the packed form reads lengths instead
    f.fproj = st->fproj; f.fmap = fmap; f.w_a = P->w_a; f.hp = hp;
    f.e = io.ss ? io.logits_ws + (size_t)B * Tmax * c.V : io.logits_ws;      // scheduled sampling: the logits are live inside the loop
    f.z = act(xh_t, E, c.asz()); f.ldx = ld; f.alpha = st->alpha + (long)t * B * c.P;
    f.P = c.P; f.A = c.A; f.C = c.C;
    f.lengths = io.lengths; f.t = t;
    f.alphas = alphas ? alphas + (long)t * c.P : nullptr; f.alphas_ld = (long)Tmax * c.P;
    GIC_PROPAGATE(attn_step(f, 1, B, c.dt, io.stream));
    LstmStepArgs a;
    a.xh_t = xh_t; a.xh_next = act(xh_t, (long)B * ld, c.asz()); a.wcat = S->wcat; a.bsum = S->bsum;
    a.c_prev = st->c + (long)t * B * H; a.c_new = st->c + (long)(t + 1) * B * H;
    a.gates = st->gates + (long)t * B * 4 * H;
    a.h_out = act(st->hout, (long)t * H, c.asz()); a.ld_out = (long)Tmax * H;        // hout viewed as [B, Tmax, H]
    a.B = B; a.H = H; a.din = c.din(); a.ldx = ld; a.gw = E;
    a.pack_len = io.lengths; a.pack_t = t;
    return lstm_step(a, c.dt, io.stream);
  }
};

// one forward pass (header comment); wout / b_out / embed / hout carry the same names in both decoders' structs
template <typename Rec>
int teacher_forced(const Rec& rec, const TfIo& io) {
  const auto& c = rec.c;
  const int B = c.B, T = c.L, V = c.V, E = c.E, H = c.H, Tmax = io.Tmax;
  const gic_sched_sample_opts* ss = io.ss;
  const bool ss_fused = ss && B <= decoder_fused_rows(c.dt, V, E, H, rec.layers());
  const gic_decoder_dropout* dr = io.drop;
  const void* hproj = dr ? dr->hdrop : rec.st->hout;       // what the vocabulary projection consumes
  const long rows = (long)B * Tmax;
  auto projection = [&] {      // the logits of all B * Tmax rows at once
    GemmDesc g;
    g.A = hproj; g.lda = H; g.B = rec.S->wout; g.ldb = H; g.C = io.logits_ws; g.ldc = V;
    g.M = (int)rows; g.N = V; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32; g.bias = rec.P->b_out;
    g.no_split = Rec::kNoSplitVocab;
    return g;
  };
  // route-only mode (gemm.h): nothing is launched; the pass's products are selected in launch order -- a step's recurrence, then the
  // logits: the projection, or scheduled sampling's per-step product, or " ss_logits=fused" behind the recurrence's line where
  // vocab_step_logits takes that product's place
  if (route_only()) {
    GIC_PROPAGATE(rec.route(io));
    if (!ss) return gemm(projection(), io.stream);
    if (!ss_fused) return ss_step_logits(c.dt, hproj, 0, Tmax, rec.S->wout, rec.P->b_out, io.logits_ws, B, V, H, false, io.stream);
    char* line = route_line();
    const size_t n = strlen(line);
    snprintf(line + n, kRouteLen - n, " ss_logits=fused");
    return GIC_OK;
  }
  // ss_tail depends on nothing begin() enqueues and nothing there on it.  That it precedes the attention decoder's begin() and follows
  // the LSTM decoder's is history, not design: kept, so that a kernel trace of either call lists the launches it always listed
  auto tail = [&] { return ss ? ss_tail(io.caps, ss->inputs, ss->replaced, B, T - 1, Tmax - 1, io.stream) : (int)GIC_OK; };
  if (Rec::kTailFirst) GIC_PROPAGATE(tail());
  GIC_PROPAGATE(rec.begin(io));
  if (!Rec::kTailFirst) GIC_PROPAGATE(tail());
  for (int t = 0; t < Tmax; ++t) {
    GIC_PROPAGATE(rec.step(io, t));
    if (!ss) continue;
    if (dr) GIC_PROPAGATE(hidden_dropout_fwd(c.dt, rec.st->hout, dr->hdrop, dr->keep_u, dr->seed, dr->p, B, Tmax, H, t, io.stream));
    GIC_PROPAGATE(ss_step_logits(c.dt, hproj, t, Tmax, rec.S->wout, rec.P->b_out, io.logits_ws, B, V, H, ss_fused, io.stream));
    if (t + 1 < Tmax) {
      SsPickArgs a;
      a.logits = io.logits_ws + (long)t * V; a.ld_logits = (long)Tmax * V;
      a.caps = io.caps; a.lengths = io.lengths; a.coin_u = ss->coin_u; a.noise_u = ss->noise_u; a.seed = ss->seed;
      a.prob = ss->prob; a.pick = ss->pick; a.t = t + 1; a.B = B; a.V = V; a.E = E; a.Tm1 = T - 1;
      a.embed = rec.P->embed; a.x_next = act(rec.xh(0), (long)(t + 1) * B * rec.ldx(0), c.asz()); a.ld_x = rec.ldx(0);
      a.inputs = ss->inputs; a.replaced = ss->replaced;
      GIC_PROPAGATE(ss_pick(a, c.dt, io.stream));
    }
  }
  if (!ss) {  // one projection over all B * Tmax rows
    if (dr) GIC_PROPAGATE(hidden_dropout_fwd(c.dt, rec.st->hout, dr->hdrop, dr->keep_u, dr->seed, dr->p, B, Tmax, H, -1, io.stream));
    GIC_PROPAGATE(gemm(projection(), io.stream));
  }
  GIC_PROPAGATE(gumbel_softmax_rows(c.dt, io.logits_ws, io.noise_u, io.seed, (uint64_t)0x7466, io.temperature, io.pretrain, io.out, rows, V, io.stream));
  for (int l = 0; l < rec.layers(); ++l) {
    const long ld = rec.ldx(l);
    GIC_PROPAGATE(cast2d(act(rec.xh(l), (long)Tmax * B * ld + rec.din(l), c.asz()), c.dt, ld, io.h_n + (long)l * B * H, DT_F32, H, B, H, io.stream));
    GIC_PROPAGATE(cast2d(rec.cell(l) + (long)Tmax * B * H, DT_F32, H, io.c_n + (long)l * B * H, DT_F32, H, B, H, io.stream));
  }
  return GIC_OK;
}

// what a backward call takes beside its model
struct TfGrad {
  const void* pred; const int64_t* caps; const int32_t* lengths; int Tmax;
  const void* d_pred; float temperature; int pretrain;
  hipStream_t stream;
  const gic_decoder_dropout* drop = nullptr;      // the forward call's output dropout, or null
};

// ---- the entry path (header comment): a model is the decoder's side of a call
struct LstmTrain {
  const gic_decoder_dims* dims; const gic_decoder_params* P; const gic_decoder_shadow* S; const gic_decoder_state* st;
  const gic_decoder_bwd_ws* ws; const gic_decoder_grads* G;       // backward calls only
  DCtx c;
  int shape() { return check_decoder_dims(dims, c); }
  bool set() const { return P && S && st; }
  // the scheduled-sampling workspace (the plain call's logits_ws is sized by the caller): the f32 logits [B, Tmax, V]
  uint64_t ws_bytes(int Tmax, bool) const { return (((uint64_t)c.B * Tmax * c.V * sizeof(float)) + 15) & ~(uint64_t)15; }
  int check_fwd(const char* who) const {
    GIC_CHECK_ARG(P->embed && P->b_out && S->wout && st->hout && st->gpre, "%s: null buffer", who);
    for (int l = 0; l < c.NL; ++l) GIC_CHECK_ARG(st->xh[l] && st->c[l] && S->wcat[l] && S->bsum[l], "%s: null layer %d buffer", who, l);
    return GIC_OK;
  }
  int run(const TfIo& io) const { return teacher_forced(LstmTf{c, P, S, st}, io); }
  int check_bwd(const char* who) const {
    GIC_CHECK_ARG(ws->dlogits && ws->dhout && st->hout && S->wout && G->embed && G->w_out && G->b_out && G->features, "%s: null buffer", who);
    for (int l = 0; l < c.NL; ++l)
      GIC_CHECK_ARG(st->xh[l] && st->c[l] && st->gates[l] && ws->dgates[l] && ws->dxh[l] && ws->dc[l] && G->w_ih[l] && G->w_hh[l] && G->b_ih[l] && G->b_hh[l],
                    "%s: null layer %d buffer (the forward call must have been given state->gates)", who, l);
    return GIC_OK;
  }
  // caps stands in for the sampled ids (the input of step t is embed(caps[b, t-1]))
  int recurrent_bwd(const DCtx& view, const TfGrad& g) const { return decoder_bwd_recurrent(view, P, S, st, ws, g.caps, c.L - 1, G, g.stream); }
};

struct AttnTrain {
  const gic_attn_dims* dims; const gic_attn_params* P; const gic_attn_shadow* S; const gic_attn_state* st;
  const void* fmap;
  float* alphas;                 // forward: f32 [B, Tmax, P] or null
  const gic_attn_bwd_ws* ws; const gic_attn_grads* G; const float* d_alphas;       // backward calls only
  ACtx c;
  int shape() { return check_attn_dims(dims, c); }
  bool set() const { return P && S && st && fmap; }
  // logits_ws: the logits [B * Tmax, V] after the loop and the energies [B, P] during it; scheduled sampling: the logits, then the energies
  uint64_t ws_bytes(int Tmax, bool ss) const {
    const uint64_t lg = (uint64_t)c.B * Tmax * c.V, en = (uint64_t)c.B * c.P;
    return (ss ? lg + en : (lg > en ? lg : en)) * sizeof(float);
  }
  int check_state(const char* who) const {
    GIC_CHECK_ARG(st->xh && st->gates && st->c && st->hout && st->fproj && st->alpha && st->hproj, "%s: null state buffer", who);
    return GIC_OK;
  }
  int check_fwd(const char* who) const {
    GIC_CHECK_ARG(P->embed && P->b_out && P->b_f && P->w_a && S->wcat && S->bsum && S->wout && S->wf && S->wh, "%s: null weights", who);
    return check_state(who);
  }
  int run(const TfIo& io) const { return teacher_forced(AttnTf{c, P, S, st, fmap, alphas}, io); }
  int check_bwd(const char* who) const {
    GIC_CHECK_ARG(S->wcat_t && S->wout && S->wh && P->w_a, "%s: null weights", who);
    GIC_PROPAGATE(check_state(who));
    GIC_CHECK_ARG(ws->dlogits && ws->dhout && ws->dgates && ws->dc && ws->dz && ws->dalpha && ws->dh_extra && ws->dhproj && ws->dfproj && ws->dwa_rows && ws->dx &&
                  (c.dt == DT_F32 || ws->dfproj_act), "%s: null workspace buffer", who);
    GIC_CHECK_ARG(G->embed && G->w_ih && G->w_hh && G->b_ih && G->b_hh && G->w_out && G->b_out && G->w_f && G->b_f && G->w_h && G->w_a && G->features,
                  "%s: null gradient buffer", who);
    return GIC_OK;
  }
  int recurrent_bwd(const ACtx& view, const TfGrad& g) const {
    return attn_bwd_recurrent(view, P, S, st, ws, fmap, g.caps, c.L - 1, d_alphas, G, g.stream);
  }
};

// the checks every teacher-forced call opens with (args: the caller's other pointer arguments are all set)
template <typename Model>
int open_entry(Model& m, const char* who, bool args, const int64_t* caps, int Tmax) {
  GIC_PROPAGATE(m.shape());
  GIC_CHECK_ARG(m.set() && args, "%s: null argument", who);
  GIC_CHECK_ARG(m.c.L == 1 || caps, "%s: caps is null", who);
  GIC_CHECK_ARG(Tmax >= 1 && Tmax <= m.c.L, "%s: Tmax must be in 1..L (= caption length + 1)", who);
  return GIC_OK;
}

// gic_*_forward_tf (io.ss null) and gic_*_forward_ss (io.ss = the options, io.logits_ws = the caller's ws); dropout: a gic_*_drop
// entry point, whose io.drop is checked after everything its plain counterpart checks
template <typename Model>
int forward_entry(Model m, const char* who, bool args, const TfIo& io, bool dropout = false) {
  GIC_PROPAGATE(open_entry(m, who, args && io.features && io.lengths && io.logits_ws && io.out && io.h_n && io.c_n, io.caps, io.Tmax));
  if (io.ss) {
    GIC_PROPAGATE(ss_check_opts(io.ss, m.c.L, who));
    GIC_CHECK_ARG(((uintptr_t)io.logits_ws & 15) == 0, "%s: ws must be 16-byte aligned", who);
  }
  GIC_PROPAGATE(m.check_fwd(who));
  if (dropout) GIC_PROPAGATE(drop_check(io.drop, who));
  return m.run(io);
}

// the output layer over B * Tmax rows and the padded steps' zero gradient, then the decoder's recurrent backward on the Tmax view:
// the saved state and every [B, Tmax, .] tensor are laid out for Tmax steps
template <typename Model>
int backward_entry(Model m, const char* who, const TfGrad& g, bool dropout = false) {
  GIC_PROPAGATE(open_entry(m, who, m.ws && m.G && g.pred && g.lengths && g.d_pred, g.caps, g.Tmax));
  GIC_PROPAGATE(m.check_bwd(who));
  if (dropout) GIC_PROPAGATE(drop_check(g.drop, who));
  if (route_only()) return GIC_OK;       // (gemm.h) validated; gic_debug_decoder_plan prints the LSTM decoder's backward selection
  auto view = m.c;
  view.L = g.Tmax;
  GIC_PROPAGATE(decoder_output_bwd(view.dt, view.B, g.Tmax, view.V, view.H, g.pred, g.d_pred, g.temperature, nullptr, g.pretrain, m.ws->dlogits,
                                   m.S->wout, g.drop ? g.drop->hdrop : m.st->hout, m.ws->dhout, m.G->w_out, m.G->b_out, g.stream));
  if (g.drop) GIC_PROPAGATE(hidden_dropout_bwd(m.ws->dhout, g.lengths, g.drop->keep_u, g.drop->seed, g.drop->p, view.B, g.Tmax, view.H, g.stream));
  else GIC_PROPAGATE(zero_past_length(m.ws->dhout, g.lengths, view.B, g.Tmax, view.H, g.stream));
  return m.recurrent_bwd(view, g);
}

template <typename Model>
int ws_bytes_entry(Model m, const char* who, int Tmax, uint64_t* out, bool ss) {
  GIC_PROPAGATE(m.shape());
  GIC_CHECK_ARG(Tmax >= 1 && Tmax <= m.c.L, "%s: Tmax must be in 1..L (= caption length + 1)", who);
  GIC_CHECK_ARG(out, "%s: null out", who);
  *out = m.ws_bytes(Tmax, ss);
  return GIC_OK;
}

}  // namespace
}  // namespace gic

extern "C" {

int gic_decoder_forward_tf(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                           const gic_decoder_state* st, const float* features, const int64_t* caps, const int32_t* lengths, int Tmax,
                           const float* noise_u, uint64_t seed, float temperature, int pretrain, float* logits_ws, int64_t* ids_ws,
                           void* out, float* h_n, float* c_n, void* stream) {
  return forward_entry(LstmTrain{dims, P, S, st}, "decoder_forward_tf", ids_ws != nullptr,
                       {features, caps, lengths, Tmax, noise_u, seed, temperature, pretrain, logits_ws, out, h_n, c_n, nullptr, (hipStream_t)stream});
}

int gic_decoder_forward_ss_ws_bytes(const gic_decoder_dims* dims, int Tmax, uint64_t* out) {
  return ws_bytes_entry(LstmTrain{dims}, "decoder_forward_ss_ws_bytes", Tmax, out, true);
}

int gic_decoder_forward_ss(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                           const gic_decoder_state* st, const float* features, const int64_t* caps, const int32_t* lengths, int Tmax,
                           const gic_sched_sample_opts* opts, void* ws, void* out, float* h_n, float* c_n, void* stream) {
  return forward_entry(LstmTrain{dims, P, S, st}, "decoder_forward_ss", opts != nullptr,
                       {features, caps, lengths, Tmax, nullptr, 0, 1.f, 1, (float*)ws, out, h_n, c_n, opts, (hipStream_t)stream});
}

int gic_decoder_forward_tf_bwd(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                               const gic_decoder_state* st, const gic_decoder_bwd_ws* ws, const void* pred, const int64_t* caps,
                               const int32_t* lengths, int Tmax, const void* d_pred, float temperature, int pretrain,
                               const gic_decoder_grads* G, void* stream) {
  return backward_entry(LstmTrain{dims, P, S, st, ws, G}, "decoder_forward_tf_bwd",
                        {pred, caps, lengths, Tmax, d_pred, temperature, pretrain, (hipStream_t)stream});
}

int gic_attn_forward_tf_ws_bytes(const gic_attn_dims* dims, int Tmax, uint64_t* out) {
  return ws_bytes_entry(AttnTrain{dims}, "attn_forward_tf_ws_bytes", Tmax, out, false);
}

int gic_attn_forward_tf(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                        const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths, int Tmax, const float* noise_u,
                        uint64_t seed, float temperature, int pretrain, float* logits_ws, void* out, float* alphas, float* h_n, float* c_n,
                        void* stream) {
  return forward_entry(AttnTrain{dims, P, S, st, fmap, alphas}, "attn_forward_tf", true,
                       {features, caps, lengths, Tmax, noise_u, seed, temperature, pretrain, logits_ws, out, h_n, c_n, nullptr, (hipStream_t)stream});
}

int gic_attn_forward_ss_ws_bytes(const gic_attn_dims* dims, int Tmax, uint64_t* out) {
  return ws_bytes_entry(AttnTrain{dims}, "attn_forward_ss_ws_bytes", Tmax, out, true);
}

int gic_attn_forward_ss(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                        const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths, int Tmax,
                        const gic_sched_sample_opts* opts, void* ws, void* out, float* alphas, float* h_n, float* c_n, void* stream) {
  if (det_mode()) {
    set_last_error("attn_forward_ss: the attention decoder is not available in the deterministic mode (gic_set_deterministic)");
    return GIC_STATUS_UNSUPPORTED;
  }
  return forward_entry(AttnTrain{dims, P, S, st, fmap, alphas}, "attn_forward_ss", opts != nullptr,
                       {features, caps, lengths, Tmax, nullptr, 0, 1.f, 1, (float*)ws, out, h_n, c_n, opts, (hipStream_t)stream});
}

int gic_attn_forward_tf_bwd(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                            const gic_attn_bwd_ws* ws, const void* fmap, const void* pred, const int64_t* caps, const int32_t* lengths, int Tmax,
                            const void* d_pred, const float* d_alphas, float temperature, int pretrain, const gic_attn_grads* G, void* stream) {
  return backward_entry(AttnTrain{dims, P, S, st, fmap, nullptr, ws, G, d_alphas}, "attn_forward_tf_bwd",
                        {pred, caps, lengths, Tmax, d_pred, temperature, pretrain, (hipStream_t)stream});
}

// ---- the same calls with output dropout: the plain entry's arguments, then drop
int gic_decoder_forward_tf_drop(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                                const gic_decoder_state* st, const float* features, const int64_t* caps, const int32_t* lengths, int Tmax,
                                const float* noise_u, uint64_t seed, float temperature, int pretrain, float* logits_ws, int64_t* ids_ws,
                                void* out, float* h_n, float* c_n, const gic_decoder_dropout* drop, void* stream) {
  return forward_entry(LstmTrain{dims, P, S, st}, "decoder_forward_tf_drop", ids_ws != nullptr,
                       {features, caps, lengths, Tmax, noise_u, seed, temperature, pretrain, logits_ws, out, h_n, c_n, nullptr, (hipStream_t)stream, drop},
                       true);
}

int gic_decoder_forward_ss_drop(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                                const gic_decoder_state* st, const float* features, const int64_t* caps, const int32_t* lengths, int Tmax,
                                const gic_sched_sample_opts* opts, void* ws, void* out, float* h_n, float* c_n,
                                const gic_decoder_dropout* drop, void* stream) {
  return forward_entry(LstmTrain{dims, P, S, st}, "decoder_forward_ss_drop", opts != nullptr,
                       {features, caps, lengths, Tmax, nullptr, 0, 1.f, 1, (float*)ws, out, h_n, c_n, opts, (hipStream_t)stream, drop}, true);
}

int gic_decoder_forward_tf_drop_bwd(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                                    const gic_decoder_state* st, const gic_decoder_bwd_ws* ws, const void* pred, const int64_t* caps,
                                    const int32_t* lengths, int Tmax, const void* d_pred, float temperature, int pretrain,
                                    const gic_decoder_grads* G, const gic_decoder_dropout* drop, void* stream) {
  return backward_entry(LstmTrain{dims, P, S, st, ws, G}, "decoder_forward_tf_drop_bwd",
                        {pred, caps, lengths, Tmax, d_pred, temperature, pretrain, (hipStream_t)stream, drop}, true);
}

int gic_attn_forward_tf_drop(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                             const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths, int Tmax,
                             const float* noise_u, uint64_t seed, float temperature, int pretrain, float* logits_ws, void* out, float* alphas,
                             float* h_n, float* c_n, const gic_decoder_dropout* drop, void* stream) {
  return forward_entry(AttnTrain{dims, P, S, st, fmap, alphas}, "attn_forward_tf_drop", true,
                       {features, caps, lengths, Tmax, noise_u, seed, temperature, pretrain, logits_ws, out, h_n, c_n, nullptr, (hipStream_t)stream, drop},
                       true);
}

int gic_attn_forward_ss_drop(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                             const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths, int Tmax,
                             const gic_sched_sample_opts* opts, void* ws, void* out, float* alphas, float* h_n, float* c_n,
                             const gic_decoder_dropout* drop, void* stream) {
  if (det_mode()) {
    set_last_error("attn_forward_ss: the attention decoder is not available in the deterministic mode (gic_set_deterministic)");
    return GIC_STATUS_UNSUPPORTED;
  }
  return forward_entry(AttnTrain{dims, P, S, st, fmap, alphas}, "attn_forward_ss_drop", opts != nullptr,
                       {features, caps, lengths, Tmax, nullptr, 0, 1.f, 1, (float*)ws, out, h_n, c_n, opts, (hipStream_t)stream, drop}, true);
}

int gic_attn_forward_tf_drop_bwd(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                                 const gic_attn_bwd_ws* ws, const void* fmap, const void* pred, const int64_t* caps, const int32_t* lengths,
                                 int Tmax, const void* d_pred, const float* d_alphas, float temperature, int pretrain,
                                 const gic_attn_grads* G, const gic_decoder_dropout* drop, void* stream) {
  return backward_entry(AttnTrain{dims, P, S, st, fmap, nullptr, ws, G, d_alphas}, "attn_forward_tf_drop_bwd",
                        {pred, caps, lengths, Tmax, d_pred, temperature, pretrain, (hipStream_t)stream, drop}, true);
}

}  // extern "C"
