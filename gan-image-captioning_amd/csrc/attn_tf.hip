// Teacher-forced decode with the attention decoder (gicap.h gic_attn_forward_tf / gic_attn_forward_tf_bwd): gic_decoder_forward_tf's
// packed-sequence semantics with the step of attention.hip.  The inputs are known before the loop, so:
//   before the loop  x rows of every step gathered once (embed_rows_tf), fp = fmap W_f^T + b_f (one product over B * P rows)
//   per step t       hp GEMM        hp [B, A] = h_{t-1} W_h^T (the library GEMM, never split over K)
//                    attn_step      the caption decode's attention kernels (attn_beam.hip) in their packed form at k = 1:
//                                   attn_step_energy per (caption, 8 positions), attn_step_ctx per (caption, 32 channel pieces); a
//                                   caption past its length returns from both at once (one zero alpha row)
//                    lstm_step      the roll-out's fused step in its packed form (decoder_step.h LstmStepArgs.pack_len): a row past its
//                                   length keeps (h, c), writes a zero output row and zero gates
//   after the loop   one vocabulary product over B * Tmax rows, then the Gumbel-softmax epilogue of gic_decoder_forward_tf.
// No f32 atomics and no GEMM splits K, so the forward gives the same bits on every call in either mode.
// Backward: decoder_output_bwd over B * Tmax rows, dhout zeroed past the lengths, then the reverse recurrence of gic_attn_sample_bwd
// (attention.hip attn_bwd_recurrent) with the d alphas added in front of the softmax backward; the zero alpha rows of padded steps make
// their attention terms vanish, and their zero gates / zero dhout rows make the LSTM terms vanish.
#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {
namespace {

// floats of logits_ws: the logits [B * Tmax, V] after the loop, the energies [B, P] during it
size_t tf_ws_floats(const ACtx& c, int Tmax) {
  const size_t lg = (size_t)c.B * Tmax * c.V, en = (size_t)c.B * c.P;
  return lg > en ? lg : en;
}

template <typename TA>
int attn_tf_fwd_t(const ACtx& c, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st, const float* features,
                  const void* fmap, const int64_t* caps, const int32_t* lengths, int Tmax, const float* noise_u, uint64_t seed,
                  float temperature, int pretrain, float* logits_ws, void* out, float* alphas, float* h_n, float* c_n, hipStream_t stream,
                  const gic_sched_sample_opts* ss = nullptr) {
  const int B = c.B, T = c.L, V = c.V, E = c.E, H = c.H;
  const long ld = c.ldx();
  // scheduled sampling (gic_attn_forward_ss): the logits of step t are formed inside the loop (so the energies sit behind them in the
  // workspace) and ss_pick decides the x rows of slot t + 1 from them; rows it does not replace keep the teacher's embedding
  float* energies = ss ? logits_ws + (size_t)B * Tmax * V : logits_ws;
  const bool ss_fused = ss && ss_fused_logits(c.dt, B, V, E, H, 1);
  if (ss) GIC_PROPAGATE(ss_tail(caps, ss->inputs, ss->replaced, B, T - 1, Tmax - 1, stream));
  // slots 0..Tmax of xh start at zero (z of padded rows stays zero: finite operands of the weight gradients), c_0 = 0, x_0 = features,
  // x_t = embed(caps[:, t-1])
  GIC_PROPAGATE(fill_zero(st->xh, (size_t)(Tmax + 1) * B * ld * c.asz(), stream));
  GIC_PROPAGATE(fill_zero(st->c, (size_t)B * H * sizeof(float), stream));
  GIC_PROPAGATE(cast2d(features, DT_F32, E, st->xh, c.dt, ld, B, E, stream));
  GIC_PROPAGATE(embed_rows_tf(c.dt, P->embed, caps, st->xh, ld, B, T - 1, E, V, stream));
  {  // fp = fmap W_f^T + b_f
    GemmDesc g;
    g.A = fmap; g.lda = c.C; g.B = S->wf; g.ldb = c.C; g.C = st->fproj; g.ldc = c.A;
    g.M = B * c.P; g.N = c.A; g.K = c.C; g.in_dtype = c.dt; g.out_dtype = c.dt; g.bias = P->b_f;
    g.no_split = 1;
    GIC_PROPAGATE(gemm(g, stream));
  }
  for (int t = 0; t < Tmax; ++t) {
    TA* xh_t = (TA*)st->xh + (long)t * B * ld;
    float* hp = st->hproj + (long)t * B * c.A;
    {  // hp [B, A] = h_{t-1} W_h^T
      GemmDesc g;
      g.A = xh_t + c.din(); g.lda = ld; g.B = S->wh; g.ldb = H; g.C = hp; g.ldc = c.A;
      g.M = B; g.N = c.A; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32;
      g.no_split = 1;
      GIC_PROPAGATE(gemm(g, stream));
    }
    AttnStepArgs f{};                // par and stop stay null: the packed form reads lengths instead
    f.fproj = st->fproj; f.fmap = fmap; f.w_a = P->w_a; f.hp = hp; f.e = energies;
    f.z = xh_t + E; f.ldx = ld; f.alpha = st->alpha + (long)t * B * c.P;
    f.P = c.P; f.A = c.A; f.C = c.C;
    f.lengths = lengths; f.t = t;
    f.alphas = alphas ? alphas + (long)t * c.P : nullptr; f.alphas_ld = (long)Tmax * c.P;
    GIC_PROPAGATE(attn_step(f, 1, B, c.dt, stream));
    LstmStepArgs a;
    a.xh_t = xh_t; a.xh_next = xh_t + (long)B * ld; a.wcat = S->wcat; a.bsum = S->bsum;
    a.c_prev = st->c + (long)t * B * H; a.c_new = st->c + (long)(t + 1) * B * H;
    a.gates = st->gates + (long)t * B * 4 * H;
    a.h_out = (TA*)st->hout + (long)t * H; a.ld_out = (long)Tmax * H;        // hout viewed as [B, Tmax, H]
    a.B = B; a.H = H; a.din = c.din(); a.ldx = ld; a.gw = E;
    a.pack_len = lengths; a.pack_t = t;
    GIC_PROPAGATE(lstm_step(a, c.dt, stream));
    if (ss) {
      GIC_PROPAGATE(ss_step_logits(c.dt, st->hout, t, Tmax, S->wout, P->b_out, logits_ws, B, V, H, ss_fused, stream));
      if (t + 1 < Tmax) {
        SsPickArgs k;
        k.logits = logits_ws + (long)t * V; k.ld_logits = (long)Tmax * V;
        k.caps = caps; k.lengths = lengths; k.coin_u = ss->coin_u; k.noise_u = ss->noise_u; k.seed = ss->seed;
        k.prob = ss->prob; k.pick = ss->pick; k.t = t + 1; k.B = B; k.V = V; k.E = E; k.Tm1 = T - 1;
        k.embed = P->embed; k.x_next = xh_t + (long)B * ld; k.ld_x = ld;
        k.inputs = ss->inputs; k.replaced = ss->replaced;
        GIC_PROPAGATE(ss_pick(k, c.dt, stream));
      }
    }
  }
  const long rows = (long)B * Tmax;
  if (!ss) {  // one projection over all B * Tmax rows
    GemmDesc g;
    g.A = st->hout; g.lda = H; g.B = S->wout; g.ldb = H; g.C = logits_ws; g.ldc = V;
    g.M = (int)rows; g.N = V; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32; g.bias = P->b_out;
    g.no_split = 1;
    GIC_PROPAGATE(gemm(g, stream));
  }
  GIC_PROPAGATE(gumbel_softmax_rows(c.dt, logits_ws, noise_u, seed, (uint64_t)0x7466, temperature, pretrain, out, rows, V, stream));
  // slot Tmax holds every row's state at its own last step (rows past their length kept it)
  GIC_PROPAGATE(cast2d((const TA*)st->xh + (long)Tmax * B * ld + c.din(), c.dt, ld, h_n, DT_F32, H, B, H, stream));
  return cast2d(st->c + (long)Tmax * B * H, DT_F32, H, c_n, DT_F32, H, B, H, stream);
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_attn_forward_tf_ws_bytes(const gic_attn_dims* dims, int Tmax, uint64_t* out) {
  ACtx c;
  GIC_PROPAGATE(check_attn_dims(dims, c));
  GIC_CHECK_ARG(Tmax >= 1 && Tmax <= c.L, "attn_forward_tf_ws_bytes: Tmax must be in 1..L (= caption length + 1)");
  GIC_CHECK_ARG(out, "attn_forward_tf_ws_bytes: null out");
  *out = (uint64_t)tf_ws_floats(c, Tmax) * sizeof(float);
  return GIC_OK;
}

int gic_attn_forward_tf(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                        const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths, int Tmax, const float* noise_u,
                        uint64_t seed, float temperature, int pretrain, float* logits_ws, void* out, float* alphas, float* h_n, float* c_n,
                        void* stream) {
  ACtx c;
  GIC_PROPAGATE(check_attn_dims(dims, c));
  GIC_CHECK_ARG(P && S && st && features && fmap && lengths && logits_ws && out && h_n && c_n, "attn_forward_tf: null argument");
  GIC_CHECK_ARG(c.L == 1 || caps, "attn_forward_tf: caps is null");
  GIC_CHECK_ARG(Tmax >= 1 && Tmax <= c.L, "attn_forward_tf: Tmax must be in 1..L (= caption length + 1)");
  GIC_CHECK_ARG(P->embed && P->b_out && P->b_f && P->w_a && S->wcat && S->bsum && S->wout && S->wf && S->wh, "attn_forward_tf: null weights");
  GIC_CHECK_ARG(st->xh && st->gates && st->c && st->hout && st->fproj && st->alpha && st->hproj, "attn_forward_tf: null state buffer");
  if (c.dt == DT_F32)
    return attn_tf_fwd_t<float>(c, P, S, st, features, fmap, caps, lengths, Tmax, noise_u, seed, temperature, pretrain, logits_ws, out, alphas,
                                h_n, c_n, (hipStream_t)stream);
  return attn_tf_fwd_t<bf16_t>(c, P, S, st, features, fmap, caps, lengths, Tmax, noise_u, seed, temperature, pretrain, logits_ws, out, alphas,
                               h_n, c_n, (hipStream_t)stream);
}

int gic_attn_forward_ss_ws_bytes(const gic_attn_dims* dims, int Tmax, uint64_t* out) {
  ACtx c;
  GIC_PROPAGATE(check_attn_dims(dims, c));
  GIC_CHECK_ARG(Tmax >= 1 && Tmax <= c.L, "attn_forward_ss_ws_bytes: Tmax must be in 1..L (= caption length + 1)");
  GIC_CHECK_ARG(out, "attn_forward_ss_ws_bytes: null out");
  *out = ((uint64_t)c.B * Tmax * c.V + (uint64_t)c.B * c.P) * sizeof(float);       // the f32 logits [B, Tmax, V], then the energies [B, P]
  return GIC_OK;
}

int gic_attn_forward_ss(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                        const float* features, const void* fmap, const int64_t* caps, const int32_t* lengths, int Tmax,
                        const gic_sched_sample_opts* opts, void* ws, void* out, float* alphas, float* h_n, float* c_n, void* stream) {
  ACtx c;
  if (det_mode()) {
    set_last_error("attn_forward_ss: the attention decoder is not available in the deterministic mode (gic_set_deterministic)");
    return GIC_STATUS_UNSUPPORTED;
  }
  GIC_PROPAGATE(check_attn_dims(dims, c));
  GIC_CHECK_ARG(P && S && st && features && fmap && lengths && opts && ws && out && h_n && c_n, "attn_forward_ss: null argument");
  GIC_CHECK_ARG(c.L == 1 || caps, "attn_forward_ss: caps is null");
  GIC_CHECK_ARG(Tmax >= 1 && Tmax <= c.L, "attn_forward_ss: Tmax must be in 1..L (= caption length + 1)");
  GIC_PROPAGATE(ss_check_opts(opts, c.L, "attn_forward_ss"));
  GIC_CHECK_ARG(((uintptr_t)ws & 15) == 0, "attn_forward_ss: ws must be 16-byte aligned");
  GIC_CHECK_ARG(P->embed && P->b_out && P->b_f && P->w_a && S->wcat && S->bsum && S->wout && S->wf && S->wh, "attn_forward_ss: null weights");
  GIC_CHECK_ARG(st->xh && st->gates && st->c && st->hout && st->fproj && st->alpha && st->hproj, "attn_forward_ss: null state buffer");
  if (c.dt == DT_F32)
    return attn_tf_fwd_t<float>(c, P, S, st, features, fmap, caps, lengths, Tmax, nullptr, 0, 1.f, 1, (float*)ws, out, alphas, h_n, c_n,
                                (hipStream_t)stream, opts);
  return attn_tf_fwd_t<bf16_t>(c, P, S, st, features, fmap, caps, lengths, Tmax, nullptr, 0, 1.f, 1, (float*)ws, out, alphas, h_n, c_n,
                               (hipStream_t)stream, opts);
}

int gic_attn_forward_tf_bwd(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* st,
                            const gic_attn_bwd_ws* ws, const void* fmap, const void* pred, const int64_t* caps, const int32_t* lengths, int Tmax,
                            const void* d_pred, const float* d_alphas, float temperature, int pretrain, const gic_attn_grads* G, void* stream_) {
  ACtx c;
  GIC_PROPAGATE(check_attn_dims(dims, c));
  GIC_CHECK_ARG(P && S && st && ws && fmap && pred && lengths && d_pred && G, "attn_forward_tf_bwd: null argument");
  GIC_CHECK_ARG(c.L == 1 || caps, "attn_forward_tf_bwd: caps is null");
  GIC_CHECK_ARG(Tmax >= 1 && Tmax <= c.L, "attn_forward_tf_bwd: Tmax must be in 1..L (= caption length + 1)");
  GIC_CHECK_ARG(S->wcat_t && S->wout && S->wh && P->w_a, "attn_forward_tf_bwd: null weights");
  GIC_CHECK_ARG(st->xh && st->gates && st->c && st->hout && st->fproj && st->alpha && st->hproj, "attn_forward_tf_bwd: null state buffer");
  GIC_CHECK_ARG(ws->dlogits && ws->dhout && ws->dgates && ws->dc && ws->dz && ws->dalpha && ws->dh_extra && ws->dhproj && ws->dfproj && ws->dwa_rows && ws->dx &&
                (c.dt == DT_F32 || ws->dfproj_act), "attn_forward_tf_bwd: null workspace buffer");
  GIC_CHECK_ARG(G->embed && G->w_ih && G->w_hh && G->b_ih && G->b_hh && G->w_out && G->b_out && G->w_f && G->b_f && G->w_h && G->w_a && G->features,
                "attn_forward_tf_bwd: null gradient buffer");
  hipStream_t stream = (hipStream_t)stream_;
  const int T = c.L;
  // the saved state and every [B, Tmax, .] tensor are laid out for Tmax steps: the sampled path's backward runs on that view
  c.L = Tmax;
  GIC_PROPAGATE(decoder_output_bwd(c.dt, c.B, Tmax, c.V, c.H, pred, d_pred, temperature, nullptr, pretrain, ws->dlogits, S->wout, st->hout,
                                   ws->dhout, G->w_out, G->b_out, stream));
  GIC_PROPAGATE(zero_past_length(ws->dhout, lengths, c.B, Tmax, c.H, stream));
  return attn_bwd_recurrent(c, P, S, st, ws, fmap, caps, T - 1, d_alphas, G, stream);
}

}  // extern "C"
