// Caption decode (gicap.h gic_decoder_beam_search, gic_attn_beam_search, gic_decoder_diverse_beam_search, gic_attn_diverse_beam_search,
// gic_decoder_sample_captions, gic_attn_sample_captions, their *_ws_bytes and the gic_*_constrained_* forms): one step loop for both
// decoders and both heads.
// Rows = B * K (row r = image r / K, beam or sample r % K).
//
// A search is a recurrence and a head, chosen at the entry point:
//   LstmFused    lstm_step's beam form per layer: h / c read from row parent[r], layer 0's x = embed[token[r]]
//   LstmGeneric  where the fused kernels decline the shapes: beam_gather, then per layer the library GEMM and lstm_pointwise_fwd
//   Attn         the fproj GEMM once; per step the hp GEMM, attn_step (attn_beam.hip) and lstm_step's beam form
// and
//   BeamHead     vocab_step_beam (generic path: the GEMM into logits + beam_tile_topk), beam_select; beam_finalize (beam.h); with
//                G > 1 groups the diverse search: the same kernels, beam_select's group-sequential form and a per-group final order
//   SampleHead   vocab_step_logits (generic path: the GEMM into logits), sample_step; sample_finalize (sample.hip)
// A sampled row is its own parent: beam_init sets par[r] = r and only beam_select writes it again, so both heads run the same
// recurrences.  The beam head stops once B images have finished, the sampler once B * K rows have: from then on the kernels of every
// later step read the count and return at once (the launch count stays fixed; the generic path's GEMMs and pointwise launches still
// run on stale rows that nothing reads).  No GEMM of a decode splits K, so no f32 partials are added atomically: a one-ulp reorder could
// flip a selection, and two calls give the same bits.
//
// Scratch (one caller-owned workspace; every region 256-byte aligned), in this order, each region only where it is listed:
//   xh[l]   act [2][rows][din_l + H]   slots t % 2 / (t + 1) % 2 hold [x_t | h_{t-1}] / h_t (attention: x_t = [x | z]); generic path:
//                                      slot 0 = the gathered GEMM input, slot 1 = the pointwise output
//   c[l]    f32 [2][rows][H]           as xh
//   gpre    f32 [rows][4H]             LSTM generic path
//   fproj act [B][P][A], hp f32 [rows][A], e f32 [rows][P]                 attention
//   ahist   f32 [L][rows][P]           attention beam: the alpha history
//   logits  f32 [rows][V]              sampler; beam on the generic path
//   part_m, part_s f32 [rows][nblk]; part_v f32, part_i i32 [rows][nblk][K]          beam: tile partials (nblk = ceil(V / 64))
//   score f32, fin / len / tok / par i32 [rows]; hist_tok i32 [L][rows]; hist_par i32 [L][rows] (beam); anc i32 [B][K][L] (attention
//   beam); last / done i32 [B]; count i32
//
// Decode constraints (gic_decode_constraints; the gic_*_constrained_* entry points): each live row's banned ids of the coming step lie
// in the caller's second workspace (nban i32 [rows], ban i32 [rows][S + 1 + L], hist i32 [2][rows][L]).  ban_init writes step 0's
// before the loop; the tail of step t's selection kernel (beam_select, sample_step), which holds every row's new token and parent,
// writes step t + 1's: no launch is added to a step.  The step's consumers -- vocab_step_beam's epilogue, beam_tile_topk, sample_step
// -- are the instantiations that read the lists; beam_select's selection is unchanged, since the tile partials it merges already
// hold admissible tokens only.  With every constraint off the entry points run the unconstrained search itself.
//
// Ensemble searches (the gic_*_ensemble_* entry points): M instances of one recurrence, each over its own recurrent regions, features
// and feature map, around ONE search state and one set of tile partials (decode_ensemble).  Per step each member runs its recurrence and
// writes its f32 logits into its slab (vocab_step_logits where the fused kernels take the shapes, else the GEMM), ensemble_mix
// (ensemble.hip) writes the mixed logits into `logits`, and the heads take them as they take the generic path's: beam_tile_topk +
// beam_select, or sample_step.  (Folding the tile top-k into the mix's second pass was built and measured slower: DESIGN.md section 27.)
// Scratch: the regions above with the logits always present and without ahist / anc (member 0's recurrent regions are the ones
// listed first), then slabs f32 [M][rows][V], then xh / c / gpre / fproj / hp / e of members 1..M-1.
// The single-model entry points launch what they launched before.
//
// Forced words (gic_forced_words; gic_*_forced_beam_search): lexically constrained beam search is one more head, ForcedHead, around the
// same recurrences (forced_beam.hip).  Its vocabulary side is vocab_step_beam_hop / forced_tile_topk, the ban forms that also keep each
// row's hop tokens out of the tile top-K and record their raw logits; its selection is forced_select, a beam per state; its final order
// forced_finalize's.  It always runs with ban lists (empty without decode constraints).  Workspace: the beam search's regions, then
// hop_id / hop_tgt i32 and hop_val f32 [rows][12], init i32 [B] and the ban-list regions of a search without decode constraints.
// Order of checks: beam_entry's, then groups == 1, C, D, null ids, 2^C | K, the constraints, the feasibility bound grown by the C * D
// hop tokens, the workspaces' alignment.  No existing head, kernel or entry point changes.
//
// Entry path: every extern "C" decode is a model (LstmModel / AttnModel: the decoder's dims, weights and, with attention, the feature
// map; its shape check, its argument check, run()), the two prefixes of its error texts and one call of beam_entry or sample_entry;
// the four *_ws_bytes are ws_bytes_entry.  Order of checks -- beam: null options, shapes, arguments and weights, options; sampler: null
// options, shapes, options, arguments and weights; then for both (entry_tail) the constraints, the workspace's alignment, the
// every-constraint-off shortcut, the constraint workspace.  That the two heads differ in whether the weights or the options come first
// is history (the sampler was written after the beam search, with its own order), not design; callers may have come to rely on which
// text a doubly wrong call gets, so both orders are kept and tests/test_decode_entry_errors.py pins them with a recorded table.
#include <cfloat>

#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {
namespace {

struct DecodeDims {
  int B, L, V, E, H, NL, dt;
  int C, P, A;                   // the attention decoder's (C = 0: the LSTM decoder)
  int K, rows, nblk;             // beams or samples per image, rows = B * K, nblk = ceil(V / 64)
  bool fused;                    // the fused step kernels take the shapes (always with attention)
  int din(int l) const { return l == 0 ? E + C : H; }
  long ldx(int l) const { return (long)din(l) + H; }
  size_t asz() const { return (size_t)dtype_size(dt); }
  bool attn() const { return C > 0; }
  void* act(void* p, long n) const { return (char*)p + n * asz(); }      // p + n compute-dtype values
};

// the limits every decode shares, after the decoder's own shape checks (who: the prefix of the error text)
int decode_dims(DecodeDims& d, int K, bool beam, const char* who) {
  if (beam) {
    GIC_CHECK_ARG(K >= 1 && K <= kBeamMax, "%s: beam size must be 1..%d, got %d", who, kBeamMax, K);
    GIC_CHECK_ARG(K <= d.V, "%s: beam size %d exceeds the vocabulary (%d)", who, K, d.V);
  } else {
    GIC_CHECK_ARG(K >= 1 && K <= kBeamMax, "%s: num_samples must be 1..%d, got %d", who, kBeamMax, K);
  }
  GIC_CHECK_ARG(d.L <= 1024, "%s: at most 1024 steps", who);
  GIC_CHECK_ARG((long)d.B * K <= (1l << 24), "%s: too many rows", who);
  d.K = K;
  d.rows = d.B * K;
  d.nblk = cdiv(d.V, kBeamTile);
  d.fused = d.attn() || d.rows <= decoder_fused_rows(d.dt, d.V, d.E, d.H, d.NL);
  return GIC_OK;
}

int lstm_dims(const gic_decoder_dims* dims, int K, bool beam, const char* who, DecodeDims& d) {
  GIC_CHECK_ARG(dims, "%s: null dims", who);
  GIC_CHECK_ARG(dims->B > 0 && dims->L > 0 && dims->V > 1 && dims->E > 0 && dims->H > 0, "%s: bad dims", who);
  GIC_CHECK_ARG(dims->NL >= 1 && dims->NL <= GIC_MAX_LAYERS, "%s: gen_num_layers must be 1..%d", who, GIC_MAX_LAYERS);
  GIC_CHECK_ARG(dims->dtype == DT_F32 || dims->dtype == DT_BF16, "%s: bad dtype", who);
  d = DecodeDims{dims->B, dims->L, dims->V, dims->E, dims->H, dims->NL, dims->dtype};
  return decode_dims(d, K, beam, who);
}

int attn_dims(const gic_attn_dims* dims, int K, bool beam, const char* who, DecodeDims& d) {
  ACtx c;
  GIC_PROPAGATE(check_attn_dims(dims, c));
  d = DecodeDims{c.B, c.L, c.V, c.E, c.H, 1, c.dt, c.C, c.P, c.A};
  return decode_dims(d, K, beam, who);
}

struct DecodeBufs {
  BeamLayerPtrs slot[2];
  float* gpre; void* fproj; float* hp; float* e; float* ahist; float* logits;
  float* pm; float* ps; float* pv; int* pi;
  BeamState st;
  int* anc;
  size_t total;
};

// carves 256-byte aligned regions out of a workspace (null: only the running total is meaningful)
struct Carver {
  void* ws; size_t at = 0;
  void* take(size_t bytes) { void* p = (void*)((uintptr_t)ws + at); at += (bytes + 255) & ~(size_t)255; return p; }
};

// one recurrence's own regions (xh, c, gpre, fproj, hp, e), in the header comment's order
void recurrent_layout(const DecodeDims& d, Carver& cv, DecodeBufs& o) {
  const size_t R = d.rows;
  for (int l = 0; l < d.NL; ++l) {
    const size_t xb = R * d.ldx(l) * d.asz();
    char* xh = (char*)cv.take(2 * xb);
    float* c = (float*)cv.take(2 * R * d.H * 4);
    for (int s = 0; s < 2; ++s) { o.slot[s].xh[l] = xh + s * xb; o.slot[s].c[l] = c + s * R * d.H; }
  }
  if (!d.fused) o.gpre = (float*)cv.take(R * 4 * d.H * 4);
  if (d.attn()) {
    o.fproj = cv.take((size_t)d.B * d.P * d.A * d.asz());
    o.hp = (float*)cv.take(R * d.A * 4);
    o.e = (float*)cv.take(R * d.P * 4);
  }
}

// the regions of the header comment (ensemble: always the logits, never the alpha history and the ancestors)
DecodeBufs decode_layout(const DecodeDims& d, bool beam, Carver& cv, bool ensemble) {
  DecodeBufs o{};
  const size_t R = d.rows, pn = R * d.nblk, LR = (size_t)d.L * R;
  recurrent_layout(d, cv, o);
  if (d.attn() && beam && !ensemble) o.ahist = (float*)cv.take(LR * d.P * 4);
  if (!beam || !d.fused || ensemble) o.logits = (float*)cv.take(R * d.V * 4);
  if (beam) {
    o.pm = (float*)cv.take(pn * 4); o.ps = (float*)cv.take(pn * 4);
    o.pv = (float*)cv.take(pn * d.K * 4); o.pi = (int*)cv.take(pn * d.K * 4);
  }
  BeamState& s = o.st;
  s.score = (float*)cv.take(R * 4);
  s.fin = (int*)cv.take(R * 4); s.len = (int*)cv.take(R * 4); s.tok = (int*)cv.take(R * 4); s.par = (int*)cv.take(R * 4);
  s.htok = (int*)cv.take(LR * 4);
  if (beam) s.hpar = (int*)cv.take(LR * 4);
  if (beam && d.attn() && !ensemble) o.anc = (int*)cv.take(LR * 4);
  s.last = (int*)cv.take((size_t)d.B * 4); s.done = (int*)cv.take((size_t)d.B * 4); s.count = (int*)cv.take(4);
  o.total = cv.at;
  return o;
}

DecodeBufs decode_layout(const DecodeDims& d, bool beam, void* ws) {
  Carver cv{ws};
  return decode_layout(d, beam, cv, false);
}

// an ensemble search's workspace: the single search's regions with member 0's recurrence (w), the members' logits, then the
// recurrent regions of members 1..M-1; mem[m] = w with member m's recurrent regions and its slab as the logits
struct EnsembleBufs {
  DecodeBufs w;
  DecodeBufs mem[GIC_MAX_ENSEMBLE];
  float* slabs;                  // f32 [M][rows][V]
  size_t total;
};

EnsembleBufs ensemble_layout(const DecodeDims& d, bool beam, int M, void* ws) {
  EnsembleBufs e{};
  Carver cv{ws};
  e.w = decode_layout(d, beam, cv, true);
  const size_t slab = (size_t)d.rows * d.V;
  e.slabs = (float*)cv.take((size_t)M * slab * 4);
  for (int m = 0; m < M; ++m) {
    e.mem[m] = e.w;
    if (m > 0) recurrent_layout(d, cv, e.mem[m]);
    e.mem[m].logits = e.slabs + m * slab;
  }
  e.total = cv.at;
  return e;
}

// decode constraints: the caller's struct and the regions of its workspace (cws)
struct Constraints {
  const gic_decode_constraints* c;
  int* nban; int* ban; int* hist;
  int cap;
  size_t total;
  int L;
  BanLists lists() const { BanLists b; b.nban = nban; b.ban = ban; b.cap = cap; return b; }
  BanOut out() const { BanOut b; b.nban = nban; b.ban = ban; b.hist = hist; b.cap = cap; b.L = L; return b; }
  BanRule rule(int eos) const {
    BanRule r;
    r.n = c->no_repeat_ngram; r.min_length = c->min_length; r.eos = eos; r.S = c->num_suppress;
    for (int i = 0; i < r.S; ++i) r.suppress[i] = c->suppress[i];
    return r;
  }
};

Constraints constraints_layout(const gic_decode_constraints* c, size_t rows, int L, void* cws) {
  Constraints o{};
  size_t at = 0;
  auto take = [&](size_t bytes) { void* p = (void*)((uintptr_t)cws + at); at += (bytes + 255) & ~(size_t)255; return p; };
  o.c = c;
  o.L = L;
  o.cap = c->num_suppress + 1 + L;
  o.nban = (int*)take(rows * 4);
  o.ban = (int*)take(rows * (size_t)o.cap * 4);
  o.hist = (int*)take(2 * rows * (size_t)L * 4);
  o.total = at;
  return o;
}

// the checks of a constraint set for a decode of L steps over V tokens in which a row proposes K tokens (who: the prefix of the error text)
int check_constraints(const gic_decode_constraints* c, int L, int V, int K, int eos, const char* who) {
  GIC_CHECK_ARG(c, "%s: null constraints", who);
  GIC_CHECK_ARG(c->no_repeat_ngram >= 0 && c->no_repeat_ngram <= L, "%s: no_repeat_ngram must be 0..L (%d), got %d", who, L, c->no_repeat_ngram);
  GIC_CHECK_ARG(c->min_length >= 0 && c->min_length <= L, "%s: min_length must be 0..L (%d), got %d", who, L, c->min_length);
  GIC_CHECK_ARG(c->num_suppress >= 0 && c->num_suppress <= kBanSuppressMax, "%s: num_suppress must be 0..%d, got %d", who, kBanSuppressMax,
                c->num_suppress);
  for (int i = 0; i < c->num_suppress; ++i) {
    GIC_CHECK_ARG(c->suppress[i] >= 0 && c->suppress[i] < V, "%s: suppress[%d] = %d outside [0, %d)", who, i, c->suppress[i], V);
    GIC_CHECK_ARG(c->suppress[i] != eos, "%s: suppress[%d] is eos_id (%d); min_length = L forbids it", who, i, eos);
  }
  const int n = c->no_repeat_ngram;
  const long banned = c->num_suppress + 1 + (n >= 1 ? L - n : 0);      // the most ids one row's list can hold apart
  GIC_CHECK_ARG((long)V - banned >= K, "%s: infeasible constraints: up to %ld of %d tokens banned (no_repeat_ngram %d, num_suppress %d, L %d) "
                "leave fewer than the %d a row proposes", who, banned, V, n, c->num_suppress, L, K);
  return GIC_OK;
}

bool constraints_off(const gic_decode_constraints* c) { return c->no_repeat_ngram == 0 && c->min_length == 0 && c->num_suppress == 0; }

// what every part of one search reads
struct Search {
  const DecodeDims& d;
  const DecodeBufs& w;
  int stop_at;                   // the finished count (w.st.count) that ends the search
  hipStream_t stream;
};

// lstm_step's beam form for layer l of step t, slot t % 2 -> (t + 1) % 2: from t = 1 on, h / c come from row parent[r] and layer 0's x
// part [0, gw) (gw = 0: all of it) is embed[token[r]]
int lstm_beam_step(const Search& s, int t, int l, const void* wcat, const float* bsum, const float* embed, int gw) {
  const DecodeDims& d = s.d;
  const BeamLayerPtrs &cur = s.w.slot[t & 1], &nxt = s.w.slot[(t & 1) ^ 1];
  LstmStepArgs a;
  a.xh_t = cur.xh[l]; a.xh_next = nxt.xh[l];
  a.wcat = wcat; a.bsum = bsum;
  a.c_prev = cur.c[l]; a.c_new = nxt.c[l];
  if (l + 1 < d.NL) { a.h_up = cur.xh[l + 1]; a.ld_up = d.ldx(l + 1); }
  a.B = d.rows; a.H = d.H; a.din = d.din(l); a.ldx = d.ldx(l); a.gw = gw;
  a.stop = s.w.st.count; a.stop_at = s.stop_at;
  if (t > 0) {
    a.parent = s.w.st.par;
    if (l == 0) { a.gather = 1; a.embed = embed; a.V = d.V; a.token = s.w.st.tok; }
  }
  return lstm_step(a, d.dt, s.stream);
}

// ---- recurrences: begin() once after beam_init, step(t) leaves the top layer's h_t in slot (t + 1) % 2 (kFused) or slot 1
struct LstmFused {
  static constexpr bool kFused = true;
  const gic_decoder_params* P; const gic_decoder_shadow* S;
  int begin(const Search&) const { return GIC_OK; }
  int step(const Search& s, int t) const {
    for (int l = 0; l < s.d.NL; ++l) GIC_PROPAGATE(lstm_beam_step(s, t, l, S->wcat[l], S->bsum[l], P->embed, 0));
    return GIC_OK;
  }
};

struct LstmGeneric {
  static constexpr bool kFused = false;
  const gic_decoder_params* P; const gic_decoder_shadow* S;
  int begin(const Search&) const { return GIC_OK; }
  int step(const Search& s, int t) const {
    const DecodeDims& d = s.d;
    const BeamLayerPtrs &in = s.w.slot[0], &out = s.w.slot[1];
    if (t > 0) GIC_PROPAGATE(beam_gather(in, out, d.NL, d.E, d.H, d.rows, d.dt, P->embed, s.w.st.tok, s.w.st.par, s.w.st.count, s.stop_at, s.stream));
    for (int l = 0; l < d.NL; ++l) {
      const long ld = d.ldx(l);
      GemmDesc g;
      g.A = in.xh[l]; g.lda = ld; g.B = S->wcat[l]; g.ldb = ld; g.C = s.w.gpre; g.ldc = 4 * d.H;
      g.M = d.rows; g.N = 4 * d.H; g.K = (int)ld; g.in_dtype = d.dt; g.out_dtype = DT_F32; g.bias = S->bsum[l];
      g.no_split = 1;
      GIC_PROPAGATE(gemm(g, s.stream));
      GIC_PROPAGATE(lstm_pointwise_fwd(d.dt, s.w.gpre, in.c[l], out.c[l], d.act(out.xh[l], d.din(l)), ld, l + 1 < d.NL ? in.xh[l + 1] : nullptr,
                                       l + 1 < d.NL ? d.ldx(l + 1) : 0, d.rows, d.H, s.stream));
    }
    return GIC_OK;
  }
};

struct Attn {
  static constexpr bool kFused = true;
  const gic_attn_params* P; const gic_attn_shadow* S;
  const void* fmap;
  bool history;                  // each step's alpha rows into ahist (for the alphas of the returned beams)
  int begin(const Search& s) const {        // fp = fmap W_f^T + b_f, once per image
    const DecodeDims& d = s.d;
    GemmDesc g;
    g.A = fmap; g.lda = d.C; g.B = S->wf; g.ldb = d.C; g.C = s.w.fproj; g.ldc = d.A;
    g.M = d.B * d.P; g.N = d.A; g.K = d.C; g.in_dtype = d.dt; g.out_dtype = d.dt; g.bias = P->b_f;
    g.no_split = 1;
    return gemm(g, s.stream);
  }
  int step(const Search& s, int t) const {
    const DecodeDims& d = s.d;
    void* xh_t = s.w.slot[t & 1].xh[0];
    GemmDesc g;                  // hp [rows, A] = h_{t-1} W_h^T, the rows as the previous step left them (the attention kernels read row parent[r])
    g.A = d.act(xh_t, d.din(0)); g.lda = d.ldx(0); g.B = S->wh; g.ldb = d.H; g.C = s.w.hp; g.ldc = d.A;
    g.M = d.rows; g.N = d.A; g.K = d.H; g.in_dtype = d.dt; g.out_dtype = DT_F32;
    g.no_split = 1;
    GIC_PROPAGATE(gemm(g, s.stream));
    AttnStepArgs f;
    f.fproj = s.w.fproj; f.fmap = fmap; f.w_a = P->w_a; f.hp = s.w.hp; f.par = s.w.st.par; f.e = s.w.e;
    f.z = d.act(xh_t, d.E); f.ldx = d.ldx(0); f.alpha = history ? s.w.ahist + (long)t * d.rows * d.P : nullptr;
    f.stop = s.w.st.count; f.stop_at = s.stop_at;
    f.P = d.P; f.A = d.A; f.C = d.C;
    GIC_PROPAGATE(attn_step(f, d.K, d.B, d.dt, s.stream));
    return lstm_beam_step(s, t, 0, S->wcat, S->bsum, P->embed, d.E);
  }
};

// ---- heads: vocab() finishes the fused vocabulary product's arguments and runs it, logits() follows the generic path's GEMM into
// w.logits, select(t) picks the step's tokens, finish() writes the outputs
struct BeamHead {
  static constexpr bool kBeam = true;
  const gic_decoder_beam_opts* o;
  int64_t* ids; float* scores; int32_t* lengths;
  float* alphas;                 // attention: f32 [B, K, L, P] or null
  int groups = 1;                // diverse beam search: G groups of K / G beams (1: beam search)
  float diversity = 0.f;         // and its Hamming penalty lambda
  const Constraints* cons = nullptr;       // decode constraints (null: none)
  int live_stride(const DecodeDims& d) const { return d.K / groups; }
  int eos() const { return o->eos_id; }
  int begin(const Search&) const { return GIC_OK; }
  int vocab(VocabStepArgs& v, const Search& s) const {
    v.part_m = s.w.pm; v.part_s = s.w.ps; v.part_v = s.w.pv; v.part_i = s.w.pi; v.nblk = s.d.nblk;
    return vocab_step_beam(v, s.d.K, s.d.dt, s.stream, cons ? cons->lists() : BanLists());
  }
  int logits(const Search& s) const {
    return beam_tile_topk(s.w.logits, s.d.rows, s.d.V, s.d.K, s.w.pm, s.w.ps, s.w.pv, s.w.pi, s.w.st.count, s.stop_at, s.stream,
                          cons ? cons->lists() : BanLists());
  }
  int select(const Search& s, int t) const {
    const BeamState& st = s.w.st;
    const BeamSelectArgs a{s.w.pm, s.w.ps, s.w.pv, s.w.pi, st.score, st.fin, st.len, st.tok, st.par, st.htok, st.hpar, st.last, st.done,
                           st.count, s.d.nblk, s.d.rows, t, o->eos_id, o->pad_id, groups, diversity};
    if (cons) return beam_select(a, s.d.K, s.d.B, s.stream, cons->out(), cons->rule(o->eos_id));
    return beam_select(a, s.d.K, s.d.B, s.stream);
  }
  int finish(const Search& s) const {
    const DecodeDims& d = s.d;
    GIC_PROPAGATE(beam_finalize(s.w.st, d.B, d.K, d.L, o->pad_id, o->length_penalty, d.K / groups, ids, scores, lengths,
                                alphas ? s.w.anc : nullptr, s.stream));
    return alphas ? attn_beam_alphas(s.w.ahist, s.w.anc, lengths, d.rows, d.L, d.P, alphas, s.stream) : GIC_OK;
  }
};

struct SampleHead {
  static constexpr bool kBeam = false;
  const gic_sample_opts* o;
  const float* noise_u; uint64_t seed;
  int64_t* ids; float* scores; int32_t* lengths;
  const Constraints* cons = nullptr;       // decode constraints (null: none)
  int live_stride(const DecodeDims&) const { return 1; }        // every row live from step 0
  int eos() const { return o->eos_id; }
  int begin(const Search&) const { return GIC_OK; }
  int vocab(VocabStepArgs& v, const Search& s) const {
    v.logits = s.w.logits; v.ld_logits = s.d.V;
    return vocab_step_logits(v, s.d.dt, s.stream);
  }
  int logits(const Search&) const { return GIC_OK; }
  int select(const Search& s, int t) const {
    if (!cons) return sample_step(s.w.logits, s.d.rows, s.d.V, o, noise_u, seed, t, s.w.st, s.stream);
    return sample_step(s.w.logits, s.d.rows, s.d.V, o, noise_u, seed, t, s.w.st, s.stream, cons->lists(), cons->out(), cons->rule(o->eos_id));
  }
  int finish(const Search& s) const { return sample_finalize(s.w.st, s.d.rows, s.d.L, o->pad_id, ids, scores, lengths, s.stream); }
};

// the forced search's head (forced_beam.hip; gicap.h gic_forced_words): the beam head's places with the hop lists beside the ban lists
// (cons is always set: with no decode constraints the lists are empty), the selection per state group and the forced final order
struct ForcedHead {
  static constexpr bool kBeam = true;
  const gic_decoder_beam_opts* o;
  int64_t* ids; float* scores; int32_t* lengths; int32_t* met;
  float* alphas;                 // attention: f32 [B, K, L, P] or null
  ForcedArgs f;
  const Constraints* cons = nullptr;
  HopLists hops() const { HopLists h; h.id = f.hop_id; h.val = f.hop_val; h.n = f.C * f.D; return h; }
  int live_stride(const DecodeDims& d) const { return d.K; }
  int eos() const { return o->eos_id; }
  int begin(const Search& s) const { return forced_init(f, s.w.st, s.d.B, s.d.K, s.stream); }       // (after beam_init: rewrites the scores)
  int vocab(VocabStepArgs& v, const Search& s) const {
    v.part_m = s.w.pm; v.part_s = s.w.ps; v.part_v = s.w.pv; v.part_i = s.w.pi; v.nblk = s.d.nblk;
    return vocab_step_beam_hop(v, s.d.K, s.d.dt, s.stream, cons->lists(), hops());
  }
  int logits(const Search& s) const {
    return forced_tile_topk(s.w.logits, s.d.rows, s.d.V, s.d.K, s.w.pm, s.w.ps, s.w.pv, s.w.pi, s.w.st.count, s.stop_at, s.stream,
                            cons->lists(), hops());
  }
  int select(const Search& s, int t) const {
    const BeamState& st = s.w.st;
    const BeamSelectArgs a{s.w.pm, s.w.ps, s.w.pv, s.w.pi, st.score, st.fin, st.len, st.tok, st.par, st.htok, st.hpar, st.last, st.done,
                           st.count, s.d.nblk, s.d.rows, t, o->eos_id, o->pad_id, 1, 0.f};
    return forced_select(a, f, s.d.K, s.d.B, s.stream, cons->out(), cons->rule(o->eos_id));
  }
  int finish(const Search& s) const {
    const DecodeDims& d = s.d;
    GIC_PROPAGATE(forced_finalize(s.w.st, f, d.B, d.K, d.L, o->pad_id, o->length_penalty, ids, scores, lengths, met,
                                  alphas ? s.w.anc : nullptr, s.stream));
    return alphas ? attn_beam_alphas(s.w.ahist, s.w.anc, lengths, d.rows, d.L, d.P, alphas, s.stream) : GIC_OK;
  }
};

// the step's vocabulary product of one recurrence: the fused product's arguments (the head finishes them), or the GEMM into w.logits
template <typename Rec>
const void* top_h(const Search& s, int t) {
  const int top = s.d.NL - 1;
  return s.d.act(s.w.slot[Rec::kFused ? (t & 1) ^ 1 : 1].xh[top], s.d.din(top));
}

template <typename Rec>
VocabStepArgs vocab_args(const Search& s, const Rec& rec, int t) {
  const DecodeDims& d = s.d;
  VocabStepArgs v;
  v.h = top_h<Rec>(s, t); v.ldh = d.ldx(d.NL - 1);
  v.wout = rec.S->wout; v.bias = rec.P->b_out;
  v.stop = s.w.st.count; v.stop_at = s.stop_at;
  v.B = d.rows; v.V = d.V; v.H = d.H;
  return v;
}

template <typename Rec>
int logits_gemm(const Search& s, const Rec& rec, int t) {
  const DecodeDims& d = s.d;
  GemmDesc g;
  g.A = top_h<Rec>(s, t); g.lda = d.ldx(d.NL - 1); g.B = rec.S->wout; g.ldb = d.H; g.C = s.w.logits; g.ldc = d.V;
  g.M = d.rows; g.N = d.V; g.K = d.H; g.in_dtype = d.dt; g.out_dtype = DT_F32; g.bias = rec.P->b_out;
  g.no_split = 1;
  return gemm(g, s.stream);
}

// one search: beam_init (and step 0's ban lists) and the recurrence's begin(), then per step the recurrence, the vocabulary product
// and the head's selection
template <typename Rec, typename Head>
int decode(const DecodeDims& d, const Rec& rec, const Head& head, void* ws, const float* features, const float* h0, const float* c0,
           void* stream) {
  const DecodeBufs w = decode_layout(d, Head::kBeam, ws);
  const Search s{d, w, Head::kBeam ? d.B : d.rows, (hipStream_t)stream};
  GIC_PROPAGATE(beam_init(w.slot[0], d.NL, d.din(0), d.E, d.H, d.B, d.K, d.dt, features, h0, c0, w.st, s.stream, head.live_stride(d)));
  if (head.cons) GIC_PROPAGATE(ban_init(head.cons->out(), head.cons->rule(head.eos()), d.rows, s.stream));
  GIC_PROPAGATE(head.begin(s));
  GIC_PROPAGATE(rec.begin(s));
  for (int t = 0; t < d.L; ++t) {
    GIC_PROPAGATE(rec.step(s, t));
    if constexpr (Rec::kFused) {
      VocabStepArgs v = vocab_args(s, rec, t);
      GIC_PROPAGATE(head.vocab(v, s));
    } else {
      GIC_PROPAGATE(logits_gemm(s, rec, t));
      GIC_PROPAGATE(head.logits(s));
    }
    GIC_PROPAGATE(head.select(s, t));
  }
  return head.finish(s);
}

// one ensemble search: M instances of one recurrence, each over its own recurrent regions and features, around one search state.  Per
// step every member's f32 logits go into its slab (the fused product's logits form, else the GEMM), ensemble_mix writes the mixed
// logits into w.logits, and the head takes them as it takes the generic path's
template <typename Rec, typename Head>
int decode_ensemble(const DecodeDims& d, const Rec* rec, const gic_ensemble_opts& eo, const Head& head, void* ws, const float* const* features,
                    void* stream) {
  const EnsembleBufs e = ensemble_layout(d, Head::kBeam, eo.M, ws);
  const int stop_at = Head::kBeam ? d.B : d.rows;
  const Search s{d, e.w, stop_at, (hipStream_t)stream};
  for (int m = 0; m < eo.M; ++m)         // (every member writes the same initial search state)
    GIC_PROPAGATE(beam_init(e.mem[m].slot[0], d.NL, d.din(0), d.E, d.H, d.B, d.K, d.dt, features[m], nullptr, nullptr, e.w.st, s.stream,
                            head.live_stride(d)));
  if (head.cons) GIC_PROPAGATE(ban_init(head.cons->out(), head.cons->rule(head.eos()), d.rows, s.stream));
  for (int m = 0; m < eo.M; ++m) GIC_PROPAGATE(rec[m].begin(Search{d, e.mem[m], stop_at, s.stream}));
  for (int t = 0; t < d.L; ++t) {
    for (int m = 0; m < eo.M; ++m) {
      const Search sm{d, e.mem[m], stop_at, s.stream};
      GIC_PROPAGATE(rec[m].step(sm, t));
      if constexpr (Rec::kFused) {
        VocabStepArgs v = vocab_args(sm, rec[m], t);
        v.logits = sm.w.logits; v.ld_logits = d.V;
        GIC_PROPAGATE(vocab_step_logits(v, d.dt, s.stream));
      } else {
        GIC_PROPAGATE(logits_gemm(sm, rec[m], t));
      }
    }
    GIC_PROPAGATE(ensemble_mix(e.slabs, (long)d.rows * d.V, d.rows, d.V, eo, e.w.logits, e.w.st.count, stop_at, s.stream));
    GIC_PROPAGATE(head.logits(s));
    GIC_PROPAGATE(head.select(s, t));
  }
  return head.finish(s);
}

template <typename Head>
int lstm_decode(const DecodeDims& d, const gic_decoder_params* P, const gic_decoder_shadow* S, const Head& head, void* ws, const float* features,
                const float* h0, const float* c0, void* stream) {
  if (d.fused) return decode(d, LstmFused{P, S}, head, ws, features, h0, c0, stream);
  return decode(d, LstmGeneric{P, S}, head, ws, features, h0, c0, stream);
}

// ---- the entry points' argument checks beyond the shapes (bufs: the caller's buffer pointers are all set)
int check_lstm_args(const gic_decoder_params* P, const gic_decoder_shadow* S, int NL, bool bufs, const char* who) {
  GIC_CHECK_ARG(P && S && bufs, "%s: null argument", who);
  GIC_CHECK_ARG(P->embed && P->b_out && S->wout, "%s: null embedding / output layer", who);
  for (int l = 0; l < NL; ++l) GIC_CHECK_ARG(S->wcat[l] && S->bsum[l], "%s: null layer %d weights", who, l);
  return GIC_OK;
}

int check_attn_args(const gic_attn_params* P, const gic_attn_shadow* S, bool bufs, const char* who) {
  GIC_CHECK_ARG(P && S && bufs, "%s: null argument", who);
  GIC_CHECK_ARG(P->embed && P->b_out && P->b_f && P->w_a && S->wcat && S->bsum && S->wout && S->wf && S->wh, "%s: null weights", who);
  return GIC_OK;
}

int check_beam_opts(const gic_decoder_beam_opts* o, int V, const char* who) {
  GIC_CHECK_ARG(o->eos_id >= 0 && o->eos_id < V, "%s: eos_id %d outside [0, %d)", who, o->eos_id, V);
  GIC_CHECK_ARG(o->pad_id >= 0 && o->pad_id < V, "%s: pad_id %d outside [0, %d)", who, o->pad_id, V);
  GIC_CHECK_ARG(o->length_penalty == o->length_penalty, "%s: length_penalty is NaN", who);
  return GIC_OK;
}

int check_diverse_opts(const gic_diverse_beam_opts* o, int V, const char* who) {
  GIC_PROPAGATE(check_beam_opts(&o->beam, V, who));
  GIC_CHECK_ARG(o->groups >= 1 && o->beam.beam % o->groups == 0, "%s: groups must be >= 1 and divide the beam size %d, got %d", who,
                o->beam.beam, o->groups);
  GIC_CHECK_ARG(o->diversity >= 0.f && o->diversity <= FLT_MAX, "%s: diversity must be finite and >= 0", who);
  return GIC_OK;
}

// ---- the entry path (header comment): a model is the decoder's side of a call, the helpers below are the head's
struct LstmModel {
  const gic_decoder_dims* dims; const gic_decoder_params* P; const gic_decoder_shadow* S;
  int shape(int K, bool beam, const char* who, DecodeDims& d) const { return lstm_dims(dims, K, beam, who, d); }
  int check(const DecodeDims& d, bool bufs, const char* who) const { return check_lstm_args(P, S, d.NL, bufs, who); }
  template <typename Head>
  int run(const DecodeDims& d, const Head& head, void* ws, const float* features, void* stream) const {
    return lstm_decode(d, P, S, head, ws, features, head.o->h0, head.o->c0, stream);
  }
};

struct AttnModel {
  const gic_attn_dims* dims; const gic_attn_params* P; const gic_attn_shadow* S;
  const void* fmap;
  bool history;                  // keep the alpha history (the beam searches that return alphas)
  int shape(int K, bool beam, const char* who, DecodeDims& d) const { return attn_dims(dims, K, beam, who, d); }
  int check(const DecodeDims&, bool bufs, const char* who) const { return check_attn_args(P, S, bufs && fmap, who); }
  template <typename Head>
  int run(const DecodeDims& d, const Head& head, void* ws, const float* features, void* stream) const {
    return decode(d, Attn{P, S, fmap, history}, head, ws, features, head.o->h0, head.o->c0, stream);
  }
};

// the prefixes of an entry point's error texts: its own and the one its shape checks have carried since they were written
struct Who { const char* call; const char* dims; };

// the buffers every decode takes
struct Io {
  void* ws; const float* features; int64_t* ids; float* scores; int32_t* lengths; void* stream;
  bool set() const { return ws && features && ids && scores && lengths; }
};

// a constrained entry point's extra arguments (the other entry points pass none)
struct ConsArgs { const gic_decode_constraints* c; void* cws; };

template <typename Model>
int ws_bytes_entry(const Model& m, int K, bool beam, const char* who, uint64_t* out) {
  DecodeDims d;
  GIC_PROPAGATE(m.shape(K, beam, who, d));
  GIC_CHECK_ARG(out, "%s_ws_bytes: null out", who);
  *out = (uint64_t)decode_layout(d, beam, nullptr).total;
  return GIC_OK;
}

// what follows the model's and the options' checks in every entry point
template <typename Model, typename Head>
int entry_tail(const Model& m, const DecodeDims& d, Head head, const char* who, const ConsArgs* k, const Io& io) {
  if (k) GIC_PROPAGATE(check_constraints(k->c, d.L, d.V, Head::kBeam ? d.K : 1, head.eos(), who));
  GIC_CHECK_ARG(((uintptr_t)io.ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  if (!k || constraints_off(k->c)) return m.run(d, head, io.ws, io.features, io.stream);
  GIC_CHECK_ARG(k->cws && ((uintptr_t)k->cws & 255) == 0, "%s: the constraint workspace must be non-null and 256-byte aligned", who);
  const Constraints cons = constraints_layout(k->c, (size_t)d.rows, d.L, k->cws);
  head.cons = &cons;
  return m.run(d, head, io.ws, io.features, io.stream);
}

// o: the plain search's options (one group, no diversity); dv: the diverse and constrained searches' (then o is unread)
template <typename Model>
int beam_entry(const Model& m, Who who, const gic_decoder_beam_opts* o, const gic_diverse_beam_opts* dv, const ConsArgs* k, const Io& io,
               float* alphas) {
  GIC_CHECK_ARG(o || dv, "%s: null options", who.call);
  if (dv) o = &dv->beam;
  DecodeDims d;
  GIC_PROPAGATE(m.shape(o->beam, true, who.dims, d));
  GIC_PROPAGATE(m.check(d, io.set(), who.call));        // the beam searches check the weights before the options (header comment)
  GIC_PROPAGATE(dv ? check_diverse_opts(dv, d.V, who.call) : check_beam_opts(o, d.V, who.call));
  const BeamHead head{o, io.ids, io.scores, io.lengths, alphas, dv ? dv->groups : 1, dv ? dv->diversity : 0.f};
  return entry_tail(m, d, head, who.call, k, io);
}

// the forced search's workspace: the beam search's regions, then hop_id / hop_tgt i32 and hop_val f32 [rows][kHopMax], init i32 [B], and
// the ban-list regions of a search without decode constraints (constraints_layout at S = 0; a call with constraints uses its cws)
struct ForcedBufs { ForcedArgs f; void* cws0; size_t total; };

ForcedBufs forced_layout(const DecodeDims& d, void* ws) {
  static const gic_decode_constraints none{};
  ForcedBufs o{};
  Carver cv{ws};
  cv.at = decode_layout(d, true, nullptr).total;
  const size_t hb = (size_t)d.rows * kHopMax * 4;
  o.f.hop_id = (int*)cv.take(hb); o.f.hop_tgt = (int*)cv.take(hb); o.f.hop_val = (float*)cv.take(hb);
  o.f.init = (int*)cv.take((size_t)d.B * 4);
  o.cws0 = cv.take(constraints_layout(&none, (size_t)d.rows, d.L, nullptr).total);
  o.total = cv.at;
  return o;
}

template <typename Model>
int forced_ws_bytes_entry(const Model& m, int K, const char* who, uint64_t* out) {
  DecodeDims d;
  GIC_PROPAGATE(m.shape(K, true, who, d));
  GIC_CHECK_ARG(out, "%s_ws_bytes: null out", who);
  *out = (uint64_t)forced_layout(d, nullptr).total;
  return GIC_OK;
}

// beam_entry's order -- null options, shapes, arguments and weights, options -- then the forced words (groups, C, D, the beam size's
// divisibility), the constraints with the feasibility bound grown by the C * D hop tokens, the workspaces' alignment
template <typename Model>
int forced_entry(const Model& m, Who who, const gic_diverse_beam_opts* dv, const gic_forced_words* fw, const ConsArgs& k, const Io& io,
                 float* alphas, int32_t* met) {
  static const gic_decode_constraints none{};
  GIC_CHECK_ARG(dv, "%s: null options", who.call);
  const gic_decoder_beam_opts* o = &dv->beam;
  DecodeDims d;
  GIC_PROPAGATE(m.shape(o->beam, true, who.dims, d));
  GIC_PROPAGATE(m.check(d, io.set() && met && fw, who.call));
  GIC_PROPAGATE(check_diverse_opts(dv, d.V, who.call));
  GIC_CHECK_ARG(dv->groups == 1, "%s: forced words do not combine with diverse groups (groups must be 1, got %d)", who.call, dv->groups);
  GIC_CHECK_ARG(fw->C >= 1 && fw->C <= kForceSetsMax, "%s: forced words: C must be 1..%d, got %d (with no constraint set use the plain search)",
                who.call, kForceSetsMax, fw->C);
  GIC_CHECK_ARG(fw->D >= 1 && fw->D <= kForceIdsMax, "%s: forced words: D must be 1..%d, got %d", who.call, kForceIdsMax, fw->D);
  GIC_CHECK_ARG(fw->ids, "%s: forced words: null ids", who.call);
  GIC_CHECK_ARG(d.K % (1 << fw->C) == 0, "%s: forced words: 2^C = %d must divide the beam size %d", who.call, 1 << fw->C, d.K);
  const gic_decode_constraints* c = k.c ? k.c : &none;
  GIC_PROPAGATE(check_constraints(c, d.L, d.V, d.K, o->eos_id, who.call));
  const int n = c->no_repeat_ngram, hop = fw->C * fw->D;
  const long banned = c->num_suppress + 1 + (n >= 1 ? d.L - n : 0) + hop;
  GIC_CHECK_ARG((long)d.V - banned >= d.K, "%s: infeasible constraints: up to %ld of %d tokens banned or forced (no_repeat_ngram %d, num_suppress %d, "
                "L %d, %d hop tokens) leave fewer than the %d a row proposes", who.call, banned, d.V, n, c->num_suppress, d.L, hop, d.K);
  GIC_CHECK_ARG(((uintptr_t)io.ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who.call);
  const bool own = constraints_off(c);
  GIC_CHECK_ARG(own || (k.cws && ((uintptr_t)k.cws & 255) == 0), "%s: the constraint workspace must be non-null and 256-byte aligned", who.call);
  ForcedBufs fb = forced_layout(d, io.ws);
  fb.f.force = fw->ids; fb.f.C = fw->C; fb.f.D = fw->D; fb.f.V = d.V;
  const Constraints cons = constraints_layout(c, (size_t)d.rows, d.L, own ? fb.cws0 : k.cws);
  ForcedHead head{o, io.ids, io.scores, io.lengths, met, alphas, fb.f, &cons};
  return m.run(d, head, io.ws, io.features, io.stream);
}

template <typename Model>
int sample_entry(const Model& m, Who who, const gic_sample_opts* o, const ConsArgs* k, const Io& io, const float* noise_u, uint64_t seed) {
  GIC_CHECK_ARG(o, "%s: null options", who.call);
  DecodeDims d;
  GIC_PROPAGATE(m.shape(o->num_samples, false, who.dims, d));
  GIC_PROPAGATE(check_sample_opts(o, d.V, true, who.call));      // the samplers check the options before the weights (header comment)
  GIC_PROPAGATE(m.check(d, io.set(), who.call));
  const SampleHead head{o, noise_u, seed, io.ids, io.scores, io.lengths};
  return entry_tail(m, d, head, who.call, k, io);
}

// ---- the ensemble entry path: the members' side of a call (M of one decoder kind behind one set of dims), then the heads' own
// checks.  Order: null options, the ensemble options (M, mode, weights), shapes, the head's options, the member arrays and every
// member's weights and inputs, the constraints, the workspace's alignment, the constraint workspace
struct LstmEnsemble {
  const gic_decoder_dims* dims; const gic_decoder_params* const* P; const gic_decoder_shadow* const* S;
  const float* const* features; const void* const* fmaps;
  int shape(int K, bool beam, const char* who, DecodeDims& d) const { return lstm_dims(dims, K, beam, who, d); }
  int check(const DecodeDims& d, int M, const char* who) const {
    GIC_CHECK_ARG(P && S && features, "%s: null member array", who);
    for (int m = 0; m < M; ++m) {
      GIC_CHECK_ARG(P[m] && S[m] && features[m], "%s: null member %d", who, m);
      GIC_PROPAGATE(check_lstm_args(P[m], S[m], d.NL, true, who));
    }
    return GIC_OK;
  }
  template <typename Head>
  int run(const DecodeDims& d, const gic_ensemble_opts& eo, const Head& head, void* ws, void* stream) const {
    if (d.fused) {
      LstmFused r[GIC_MAX_ENSEMBLE];
      for (int m = 0; m < eo.M; ++m) r[m] = LstmFused{P[m], S[m]};
      return decode_ensemble(d, r, eo, head, ws, features, stream);
    }
    LstmGeneric r[GIC_MAX_ENSEMBLE];
    for (int m = 0; m < eo.M; ++m) r[m] = LstmGeneric{P[m], S[m]};
    return decode_ensemble(d, r, eo, head, ws, features, stream);
  }
};

struct AttnEnsemble {
  const gic_attn_dims* dims; const gic_attn_params* const* P; const gic_attn_shadow* const* S;
  const float* const* features; const void* const* fmaps;
  int shape(int K, bool beam, const char* who, DecodeDims& d) const { return attn_dims(dims, K, beam, who, d); }
  int check(const DecodeDims&, int M, const char* who) const {
    GIC_CHECK_ARG(P && S && features && fmaps, "%s: null member array", who);
    for (int m = 0; m < M; ++m) {
      GIC_CHECK_ARG(P[m] && S[m] && features[m] && fmaps[m], "%s: null member %d", who, m);
      GIC_PROPAGATE(check_attn_args(P[m], S[m], true, who));
    }
    return GIC_OK;
  }
  template <typename Head>
  int run(const DecodeDims& d, const gic_ensemble_opts& eo, const Head& head, void* ws, void* stream) const {
    Attn r[GIC_MAX_ENSEMBLE];
    for (int m = 0; m < eo.M; ++m) r[m] = Attn{P[m], S[m], fmaps[m], false};
    return decode_ensemble(d, r, eo, head, ws, features, stream);
  }
};

int check_ensemble_count(int M, const gic_ensemble_opts* eo, const char* who) {
  GIC_PROPAGATE(check_ensemble_opts(eo, who));
  GIC_CHECK_ARG(M == eo->M, "%s: M (%d) differs from the ensemble options' (%d)", who, M, eo->M);
  return GIC_OK;
}

template <typename Members>
int ensemble_ws_bytes_entry(const Members& e, int M, int K, bool beam, const char* who, uint64_t* out) {
  GIC_CHECK_ARG(M >= 1 && M <= GIC_MAX_ENSEMBLE, "%s_ws_bytes: M must be 1..%d, got %d", who, GIC_MAX_ENSEMBLE, M);
  DecodeDims d;
  GIC_PROPAGATE(e.shape(K, beam, who, d));
  GIC_CHECK_ARG(out, "%s_ws_bytes: null out", who);
  *out = (uint64_t)ensemble_layout(d, beam, M, nullptr).total;
  return GIC_OK;
}

template <typename Members, typename Head>
int ensemble_tail(const Members& e, const DecodeDims& d, const gic_ensemble_opts& eo, Head head, const char* who, const gic_decode_constraints* c,
                  void* ws, void* cws, void* stream) {
  GIC_CHECK_ARG(ws && head.ids && head.scores && head.lengths, "%s: null argument", who);
  GIC_PROPAGATE(e.check(d, eo.M, who));
  if (c) GIC_PROPAGATE(check_constraints(c, d.L, d.V, Head::kBeam ? d.K : 1, head.eos(), who));
  GIC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  if (!c || constraints_off(c)) return e.run(d, eo, head, ws, stream);
  GIC_CHECK_ARG(cws && ((uintptr_t)cws & 255) == 0, "%s: the constraint workspace must be non-null and 256-byte aligned", who);
  const Constraints cons = constraints_layout(c, (size_t)d.rows, d.L, cws);
  head.cons = &cons;
  return e.run(d, eo, head, ws, stream);
}

template <typename Members>
int ensemble_beam_entry(const Members& e, int M, const char* who, const gic_ensemble_opts* eo, const gic_diverse_beam_opts* dv,
                        const gic_decode_constraints* c, void* ws, void* cws, int64_t* ids, float* scores, int32_t* lengths, void* stream) {
  GIC_CHECK_ARG(dv, "%s: null options", who);
  GIC_PROPAGATE(check_ensemble_count(M, eo, who));
  DecodeDims d;
  GIC_PROPAGATE(e.shape(dv->beam.beam, true, who, d));
  GIC_PROPAGATE(check_diverse_opts(dv, d.V, who));
  GIC_CHECK_ARG(!dv->beam.h0 && !dv->beam.c0, "%s: an ensemble search takes no initial states (h0 / c0 must be null)", who);
  const BeamHead head{&dv->beam, ids, scores, lengths, nullptr, dv->groups, dv->diversity};
  return ensemble_tail(e, d, *eo, head, who, c, ws, cws, stream);
}

template <typename Members>
int ensemble_sample_entry(const Members& e, int M, const char* who, const gic_ensemble_opts* eo, const gic_sample_opts* o,
                          const gic_decode_constraints* c, void* ws, void* cws, const float* noise_u, uint64_t seed, int64_t* ids,
                          float* scores, int32_t* lengths, void* stream) {
  GIC_CHECK_ARG(o, "%s: null options", who);
  GIC_PROPAGATE(check_ensemble_count(M, eo, who));
  DecodeDims d;
  GIC_PROPAGATE(e.shape(o->num_samples, false, who, d));
  GIC_PROPAGATE(check_sample_opts(o, d.V, true, who));
  GIC_CHECK_ARG(!o->h0 && !o->c0, "%s: an ensemble search takes no initial states (h0 / c0 must be null)", who);
  const SampleHead head{o, noise_u, seed, ids, scores, lengths};
  return ensemble_tail(e, d, *eo, head, who, c, ws, cws, stream);
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_decoder_beam_ws_bytes(const gic_decoder_dims* dims, int32_t beam, uint64_t* out) {
  return ws_bytes_entry(LstmModel{dims}, beam, true, "decoder_beam", out);
}

int gic_attn_beam_ws_bytes(const gic_attn_dims* dims, int32_t beam, uint64_t* out) {
  return ws_bytes_entry(AttnModel{dims}, beam, true, "attn_beam", out);
}

int gic_decoder_sample_ws_bytes(const gic_decoder_dims* dims, int32_t num_samples, uint64_t* out) {
  return ws_bytes_entry(LstmModel{dims}, num_samples, false, "decoder_sample", out);
}

int gic_attn_sample_ws_bytes(const gic_attn_dims* dims, int32_t num_samples, uint64_t* out) {
  return ws_bytes_entry(AttnModel{dims}, num_samples, false, "attn_sample", out);
}

int gic_decode_constraints_ws_bytes(int64_t rows, int32_t L, const gic_decode_constraints* c, uint64_t* out) {
  GIC_CHECK_ARG(c && out, "decode_constraints_ws_bytes: null argument");
  GIC_CHECK_ARG(rows >= 1 && rows <= (1l << 24) && L >= 1 && L <= 1024, "decode_constraints_ws_bytes: rows must be 1..2^24 and L 1..1024");
  GIC_CHECK_ARG(c->num_suppress >= 0 && c->num_suppress <= kBanSuppressMax, "decode_constraints_ws_bytes: num_suppress must be 0..%d, got %d",
                kBanSuppressMax, c->num_suppress);
  *out = (uint64_t)constraints_layout(c, (size_t)rows, L, nullptr).total;
  return GIC_OK;
}

int gic_decoder_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S, const gic_decoder_beam_opts* o,
                            void* ws, const float* features, int64_t* ids, float* scores, int32_t* lengths, void* stream) {
  return beam_entry(LstmModel{dims, P, S}, {"decoder_beam_search", "decoder_beam"}, o, nullptr, nullptr,
                    {ws, features, ids, scores, lengths, stream}, nullptr);
}

int gic_attn_beam_search(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_decoder_beam_opts* o, void* ws,
                         const float* features, const void* fmap, int64_t* ids, float* scores, int32_t* lengths, float* alphas, void* stream) {
  return beam_entry(AttnModel{dims, P, S, fmap, alphas != nullptr}, {"attn_beam_search", "attn_beam"}, o, nullptr, nullptr,
                    {ws, features, ids, scores, lengths, stream}, alphas);
}

// the diverse searches share the beam searches' workspace: gic_*_beam_ws_bytes for the same beam size
int gic_decoder_diverse_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                                    const gic_diverse_beam_opts* o, void* ws, const float* features, int64_t* ids, float* scores,
                                    int32_t* lengths, void* stream) {
  return beam_entry(LstmModel{dims, P, S}, {"decoder_diverse_beam_search", "decoder_diverse_beam"}, nullptr, o, nullptr,
                    {ws, features, ids, scores, lengths, stream}, nullptr);
}

int gic_attn_diverse_beam_search(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_diverse_beam_opts* o,
                                 void* ws, const float* features, const void* fmap, int64_t* ids, float* scores, int32_t* lengths,
                                 float* alphas, void* stream) {
  return beam_entry(AttnModel{dims, P, S, fmap, alphas != nullptr}, {"attn_diverse_beam_search", "attn_diverse_beam"}, nullptr, o, nullptr,
                    {ws, features, ids, scores, lengths, stream}, alphas);
}

int gic_decoder_constrained_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                                        const gic_diverse_beam_opts* o, const gic_decode_constraints* c, void* ws, void* cws,
                                        const float* features, int64_t* ids, float* scores, int32_t* lengths, void* stream) {
  const ConsArgs k{c, cws};
  return beam_entry(LstmModel{dims, P, S}, {"decoder_constrained_beam_search", "decoder_constrained_beam"}, nullptr, o, &k,
                    {ws, features, ids, scores, lengths, stream}, nullptr);
}

int gic_attn_constrained_beam_search(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S,
                                     const gic_diverse_beam_opts* o, const gic_decode_constraints* c, void* ws, void* cws,
                                     const float* features, const void* fmap, int64_t* ids, float* scores, int32_t* lengths, float* alphas,
                                     void* stream) {
  const ConsArgs k{c, cws};
  return beam_entry(AttnModel{dims, P, S, fmap, alphas != nullptr}, {"attn_constrained_beam_search", "attn_constrained_beam"}, nullptr, o, &k,
                    {ws, features, ids, scores, lengths, stream}, alphas);
}

int gic_decoder_forced_beam_ws_bytes(const gic_decoder_dims* dims, int32_t beam, uint64_t* out) {
  return forced_ws_bytes_entry(LstmModel{dims}, beam, "decoder_forced_beam", out);
}

int gic_attn_forced_beam_ws_bytes(const gic_attn_dims* dims, int32_t beam, uint64_t* out) {
  return forced_ws_bytes_entry(AttnModel{dims}, beam, "attn_forced_beam", out);
}

int gic_decoder_forced_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                                   const gic_diverse_beam_opts* o, const gic_forced_words* fw, const gic_decode_constraints* c, void* ws,
                                   void* cws, const float* features, int64_t* ids, float* scores, int32_t* lengths, int32_t* met,
                                   void* stream) {
  return forced_entry(LstmModel{dims, P, S}, {"decoder_forced_beam_search", "decoder_forced_beam"}, o, fw, {c, cws},
                      {ws, features, ids, scores, lengths, stream}, nullptr, met);
}

int gic_attn_forced_beam_search(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_diverse_beam_opts* o,
                                const gic_forced_words* fw, const gic_decode_constraints* c, void* ws, void* cws, const float* features,
                                const void* fmap, int64_t* ids, float* scores, int32_t* lengths, float* alphas, int32_t* met, void* stream) {
  return forced_entry(AttnModel{dims, P, S, fmap, alphas != nullptr}, {"attn_forced_beam_search", "attn_forced_beam"}, o, fw, {c, cws},
                      {ws, features, ids, scores, lengths, stream}, alphas, met);
}

int gic_decoder_sample_captions(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S, const gic_sample_opts* o,
                                void* ws, const float* features, const float* noise_u, uint64_t seed, int64_t* ids, float* scores,
                                int32_t* lengths, void* stream) {
  return sample_entry(LstmModel{dims, P, S}, {"decoder_sample_captions", "decoder_sample"}, o, nullptr,
                      {ws, features, ids, scores, lengths, stream}, noise_u, seed);
}

int gic_attn_sample_captions(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_sample_opts* o, void* ws,
                             const float* features, const void* fmap, const float* noise_u, uint64_t seed, int64_t* ids, float* scores,
                             int32_t* lengths, void* stream) {
  return sample_entry(AttnModel{dims, P, S, fmap, false}, {"attn_sample_captions", "attn_sample"}, o, nullptr,
                      {ws, features, ids, scores, lengths, stream}, noise_u, seed);
}

int gic_decoder_constrained_sample_captions(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S,
                                            const gic_sample_opts* o, const gic_decode_constraints* c, void* ws, void* cws,
                                            const float* features, const float* noise_u, uint64_t seed, int64_t* ids, float* scores,
                                            int32_t* lengths, void* stream) {
  const ConsArgs k{c, cws};
  return sample_entry(LstmModel{dims, P, S}, {"decoder_constrained_sample_captions", "decoder_constrained_sample"}, o, &k,
                      {ws, features, ids, scores, lengths, stream}, noise_u, seed);
}

int gic_attn_constrained_sample_captions(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_sample_opts* o,
                                         const gic_decode_constraints* c, void* ws, void* cws, const float* features, const void* fmap,
                                         const float* noise_u, uint64_t seed, int64_t* ids, float* scores, int32_t* lengths, void* stream) {
  const ConsArgs k{c, cws};
  return sample_entry(AttnModel{dims, P, S, fmap, false}, {"attn_constrained_sample_captions", "attn_constrained_sample"}, o, &k,
                      {ws, features, ids, scores, lengths, stream}, noise_u, seed);
}

int gic_decoder_ensemble_beam_ws_bytes(const gic_decoder_dims* dims, int32_t M, int32_t beam, uint64_t* out) {
  return ensemble_ws_bytes_entry(LstmEnsemble{dims}, M, beam, true, "decoder_ensemble_beam", out);
}

int gic_attn_ensemble_beam_ws_bytes(const gic_attn_dims* dims, int32_t M, int32_t beam, uint64_t* out) {
  return ensemble_ws_bytes_entry(AttnEnsemble{dims}, M, beam, true, "attn_ensemble_beam", out);
}

int gic_decoder_ensemble_sample_ws_bytes(const gic_decoder_dims* dims, int32_t M, int32_t num_samples, uint64_t* out) {
  return ensemble_ws_bytes_entry(LstmEnsemble{dims}, M, num_samples, false, "decoder_ensemble_sample", out);
}

int gic_attn_ensemble_sample_ws_bytes(const gic_attn_dims* dims, int32_t M, int32_t num_samples, uint64_t* out) {
  return ensemble_ws_bytes_entry(AttnEnsemble{dims}, M, num_samples, false, "attn_ensemble_sample", out);
}

int gic_decoder_ensemble_beam_search(const gic_decoder_dims* dims, int32_t M, const gic_decoder_params* const* P,
                                     const gic_decoder_shadow* const* S, const gic_ensemble_opts* eo, const gic_diverse_beam_opts* o,
                                     const gic_decode_constraints* c, void* ws, void* cws, const float* const* features, int64_t* ids,
                                     float* scores, int32_t* lengths, void* stream) {
  return ensemble_beam_entry(LstmEnsemble{dims, P, S, features, nullptr}, M, "decoder_ensemble_beam_search", eo, o, c, ws, cws, ids, scores,
                             lengths, stream);
}

int gic_attn_ensemble_beam_search(const gic_attn_dims* dims, int32_t M, const gic_attn_params* const* P, const gic_attn_shadow* const* S,
                                  const gic_ensemble_opts* eo, const gic_diverse_beam_opts* o, const gic_decode_constraints* c, void* ws,
                                  void* cws, const float* const* features, const void* const* fmaps, int64_t* ids, float* scores,
                                  int32_t* lengths, void* stream) {
  return ensemble_beam_entry(AttnEnsemble{dims, P, S, features, fmaps}, M, "attn_ensemble_beam_search", eo, o, c, ws, cws, ids, scores,
                             lengths, stream);
}

int gic_decoder_ensemble_sample_captions(const gic_decoder_dims* dims, int32_t M, const gic_decoder_params* const* P,
                                         const gic_decoder_shadow* const* S, const gic_ensemble_opts* eo, const gic_sample_opts* o,
                                         const gic_decode_constraints* c, void* ws, void* cws, const float* const* features,
                                         const float* noise_u, uint64_t seed, int64_t* ids, float* scores, int32_t* lengths, void* stream) {
  return ensemble_sample_entry(LstmEnsemble{dims, P, S, features, nullptr}, M, "decoder_ensemble_sample_captions", eo, o, c, ws, cws, noise_u,
                               seed, ids, scores, lengths, stream);
}

int gic_attn_ensemble_sample_captions(const gic_attn_dims* dims, int32_t M, const gic_attn_params* const* P,
                                      const gic_attn_shadow* const* S, const gic_ensemble_opts* eo, const gic_sample_opts* o,
                                      const gic_decode_constraints* c, void* ws, void* cws, const float* const* features,
                                      const void* const* fmaps, const float* noise_u, uint64_t seed, int64_t* ids, float* scores,
                                      int32_t* lengths, void* stream) {
  return ensemble_sample_entry(AttnEnsemble{dims, P, S, features, fmaps}, M, "attn_ensemble_sample_captions", eo, o, c, ws, cws, noise_u, seed,
                               ids, scores, lengths, stream);
}

}  // extern "C"
