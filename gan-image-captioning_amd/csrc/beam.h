// Beam-search caption decode (gicap.h gic_decoder_beam_search): per-tile partials, per-image selection, final sort.
//
// One decode step over rows = B*k (row r = image r / k, beam r % k) is NL + 2 launches on the fused path:
//   lstm_step (per layer)  the recurrent state is read from row parent[r] (reorder without a copy), layer 0's input is embed[token[r]]
//   vocab_step_beam        the vocabulary product of vocab_step; epilogue: per (row, 64-wide tile) max, sum of exp and the tile's top-k
//                          (logit, index) pairs, each in a fixed slot (no atomics)
//   beam_select            one workgroup per image: merges the tile partials of its k rows (logsumexp, row top-k), builds the <= k*k
//                          candidates, keeps the k best, writes the new scores / tokens / parents / history
// and one launch after the last step (beam_finalize).  The generic path (shapes the fused kernels decline) replaces the first two by
// beam_gather + the library GEMM + LSTM pointwise per layer, and the GEMM + beam_tile_topk.
// The global top-k of a row is a subset of the union of its tile top-k sets, so the tile partials lose nothing.
// Once every image has finished, the beam kernels of each later step (lstm_step's beam form, vocab_step_beam, beam_gather,
// beam_tile_topk, beam_select) read the count of finished images and return at once: the launch count stays fixed.  On the generic
// path the library GEMMs and the LSTM pointwise launches between them still run in full on stale rows; nothing reads their results.
// The generic path's GEMMs never split K, so neither path adds f32 partials atomically.
#pragma once
#include <climits>
#include <type_traits>

#include "../../include/gicap.h"
#include "common.h"
#include "decoder_step.h"

namespace gic {

constexpr int kBeamMax = 8;
constexpr int kBeamTile = 64;     // vocabulary entries per tile partial (= kVocabTile)

// (logit, index) order of the candidate lists: larger logit first, equal logits -> lower index (sample's first maximal index)
__device__ __forceinline__ bool beam_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// insert (v, i) into the sorted list (lv, li)[K]: static indices only (the lists stay in registers)
template <int K>
__device__ __forceinline__ void beam_insert(float (&lv)[K], int (&li)[K], float v, int i) {
#pragma unroll
  for (int q = 0; q < K; ++q) {
    if (beam_better(v, i, lv[q], li[q])) {
      const float tv = lv[q]; const int ti = li[q];
      lv[q] = v; li[q] = i; v = tv; i = ti;
    }
  }
}

// butterfly merge of the lists held by lane groups: after the levels [lo, hi) every lane of a 2^hi group holds the group's top-K.
// The lists of two partners come from disjoint index sets, so the union's top-K is well defined and both partners agree on it.
template <int K, int LO, int HI>
__device__ __forceinline__ void beam_merge_levels(float (&lv)[K], int (&li)[K]) {
#pragma unroll
  for (int o = 1 << LO; o < (1 << HI); o <<= 1) {
    float pv[K]; int pi[K];
#pragma unroll
    for (int q = 0; q < K; ++q) { pv[q] = __shfl_xor(lv[q], o, 64); pi[q] = __shfl_xor(li[q], o, 64); }
#pragma unroll
    for (int q = 0; q < K; ++q) beam_insert<K>(lv, li, pv[q], pi[q]);
  }
}

// (max, sum of exp(x - max)) of two parts; symmetric in its arguments, so butterfly partners compute the same bits
__device__ __forceinline__ void lse_combine(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mn));
  m = mn;
}

// One (row, 64-entry tile) held by 8 consecutive lanes, 8 entries each (index INT_MAX / value -inf past V): the tile's max, sum of
// exp and top-K, written by the group's first lane to slot (row, tile) of the partials.
template <int K>
__device__ __forceinline__ void beam_tile_reduce8(const float (&x)[8], const int (&ix)[8], bool store, long slot, float* part_m, float* part_s,
                                                  float* part_v, int* part_i) {
  float m = x[0];
#pragma unroll
  for (int e = 1; e < 8; ++e) m = fmaxf(m, x[e]);
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += x[e] == -INFINITY ? 0.f : expf(x[e] - m);
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o, 64);
  float lv[K]; int li[K];
#pragma unroll
  for (int q = 0; q < K; ++q) { lv[q] = -INFINITY; li[q] = INT_MAX; }
#pragma unroll
  for (int e = 0; e < 8; ++e) beam_insert<K>(lv, li, x[e], ix[e]);
  beam_merge_levels<K, 0, 3>(lv, li);
  if (store) {
    part_m[slot] = m;
    part_s[slot] = s;
#pragma unroll
    for (int q = 0; q < K; ++q) { part_v[slot * K + q] = lv[q]; part_i[slot * K + q] = li[q]; }
  }
}

// beam_tile_reduce8 with the top-K list built from (xs, ixs), the copy of (x, ix) in which the row's banned entries are (-inf, INT_MAX)
// (decode constraints); the max and the sum stay those of the raw x.  A function of its own, so that the one above compiles as it did
template <int K>
__device__ __forceinline__ void beam_tile_reduce8_sel(const float (&x)[8], const float (&xs)[8], const int (&ixs)[8], bool store, long slot,
                                                      float* part_m, float* part_s, float* part_v, int* part_i) {
  float m = x[0];
#pragma unroll
  for (int e = 1; e < 8; ++e) m = fmaxf(m, x[e]);
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += x[e] == -INFINITY ? 0.f : expf(x[e] - m);
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o, 64);
  float lv[K]; int li[K];
#pragma unroll
  for (int q = 0; q < K; ++q) { lv[q] = -INFINITY; li[q] = INT_MAX; }
#pragma unroll
  for (int e = 0; e < 8; ++e) beam_insert<K>(lv, li, xs[e], ixs[e]);
  beam_merge_levels<K, 0, 3>(lv, li);
  if (store) {
    part_m[slot] = m;
    part_s[slot] = s;
#pragma unroll
    for (int q = 0; q < K; ++q) { part_v[slot * K + q] = lv[q]; part_i[slot * K + q] = li[q]; }
  }
}

// ---- decode constraints (gicap.h gic_decode_constraints): the per-row ban lists, rebuilt before every step's vocabulary product
constexpr int kBanSuppressMax = 16;
// nban i32 [rows], ban i32 [rows][cap] (cap = S + 1 + L: the suppressed ids, <E>, one id per earlier position); null nban = no constraints
struct BanLists { const int* nban = nullptr; const int* ban = nullptr; int cap = 0; };

// the rule of a constraint set as the kernels that build the lists take it, and where they write: the lists of the NEXT step and (beam
// search) the rows' flat histories hist i32 [2][rows][L], slot (tokens emitted) % 2, so that no step walks the parent pointers
struct BanRule { int n = 0, min_length = 0, eos = 0, S = 0; int suppress[kBanSuppressMax] = {}; };
struct BanOut { int* nban = nullptr; int* ban = nullptr; int* hist = nullptr; int cap = 0, L = 0; };

// One wave: the ban list of a row that has emitted hs[0 .. t) and is about to emit its token of step t -- the suppressed ids, eos while
// t + 1 < min_length, and with n >= 1 the token that followed every earlier occurrence of the row's last n - 1 tokens, compacted in
// position order by a ballot (no atomics; at most S + 1 + t entries <= cap).  hs is in LDS, complete before the call (t = 0: unused)
__device__ __forceinline__ void ban_list_wave(const int* hs, int t, int lane, const BanRule& c, int* __restrict__ out, int* __restrict__ nban) {
#pragma unroll
  for (int s = 0; s < kBanSuppressMax; ++s)
    if (lane == s && s < c.S) out[s] = c.suppress[s];
  int nb = c.S;
  if (t + 1 < c.min_length) {
    if (lane == 0) out[nb] = c.eos;
    ++nb;
  }
  const int n = c.n, np = t - n + 1;                       // np earlier positions can start the row's last n - 1 tokens
  if (n >= 1) {
    for (int base = 0; base < np; base += 64) {
      const int i = base + lane;
      bool m = i < np;
      for (int k = 0; m && k < n - 1; ++k) m = hs[i + k] == hs[np + k];
      const unsigned long long mask = __ballot(m);
      if (m) out[nb + __popcll(mask & ((1ull << lane) - 1ull))] = hs[i + n - 1];
      nb += __popcll(mask);
    }
  }
  if (lane == 0) *nban = nb;
}

// the copy of a lane's 8 entries v0 .. v0 + 7 in which the ids of the row's ban list are (-inf, INT_MAX): a walk over the row's short
// list, not over a V-wide mask.  (Every lane reads every id itself: sharing a batch of 8 loads among the 8 lanes of a (row, tile) by
// shuffles measured slower, +0.6 us per step at k = 1 -- the loads do not depend on each other and the list is L2-resident.)
__device__ __forceinline__ void ban_apply8(float (&x)[8], int (&ix)[8], int v0, const int* __restrict__ list, int n) {
  for (int i = 0; i < n; ++i) {
    const int d = list[i] - v0;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (d == e) { x[e] = -INFINITY; ix[e] = INT_MAX; }
  }
}

// ---- forced words (gicap.h gic_forced_words; forced_beam.hip): a row's hop tokens, the ids of its image's constraint sets that its
// state has not met.  A row's state is its beam's state group, so its hop list never changes during a search: forced_init writes it once
constexpr int kForceSetsMax = 3, kForceIdsMax = 4, kHopMax = kForceSetsMax * kForceIdsMax;
// id i32 [rows][kHopMax] (slot c * D + d; -1: not a hop token of the row), val f32 [rows][kHopMax]: the raw logit of each hop token, written
// by the step's vocabulary side; n = C * D, the slots in use (the walk reads no further).  null id = no forced words
struct HopLists { const int* id = nullptr; float* val = nullptr; int n = 0; };

// ban_apply8 for the hop list, after it: a hop token leaves the copy like a banned one, and its raw logit -- the element the walk has in
// hand -- goes to the row's slot (store: this lane's row is a real one).  One lane of the grid holds a given (row, id): a single writer.
// The row's kHopMax ids (48 bytes, 16-byte aligned: the region is 256-byte aligned) come in three loads issued together, before the
// compares: a loop that loads id by id pays one L2 latency per slot (measured: 1.2 us per slot and step at cfg2)
__device__ __forceinline__ void hop_apply8(float (&x)[8], int (&ix)[8], int v0, const int* __restrict__ ids, float* __restrict__ vals, int n,
                                           bool store) {
  static_assert(kHopMax == 12, "three 16-byte loads");
  const int4 q0 = ((const int4*)ids)[0], q1 = ((const int4*)ids)[1], q2 = ((const int4*)ids)[2];
  const int id[kHopMax] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
  for (int i = 0; i < kHopMax; ++i) {
    if (i < n) {                                             // (uniform: n = C * D)
      const int d = id[i] - v0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (d == e) {
          if (store) vals[i] = x[e];
          x[e] = -INFINITY; ix[e] = INT_MAX;
        }
    }
  }
}

// the fused vocabulary product of vocab_step with the beam epilogue (decoder_step.hip): a.B = rows, a.part_m / part_s [rows][nblk],
// a.part_v / part_i [rows][nblk][K]; a.stop / stop_at; the sampling fields (u, seed, temperature, out, rowkey) are unused.  bans (decode
// constraints): the epilogue that takes each row's top-K among the ids outside its ban list
int vocab_step_beam(const VocabStepArgs& a, int K, int dtype, hipStream_t stream, const BanLists& bans = BanLists());
// the forced search's instantiation (K even): the ban epilogue, which also keeps each row's hop tokens out of the tile top-K and records
// their raw logits; bans and hops both set
int vocab_step_beam_hop(const VocabStepArgs& a, int K, int dtype, hipStream_t stream, const BanLists& bans, const HopLists& hops);

// ---- the kernels of a caption decode (decode.hip drives them: one step loop for both decoders and both heads)
struct BeamLayerPtrs { void* xh[GIC_MAX_LAYERS]; float* c[GIC_MAX_LAYERS]; };

// the search state in the workspace: score f32, fin / len / tok / par i32 [rows]; htok / hpar i32 [L][rows] (hpar: beam only);
// last / done i32 [B]; count i32
struct BeamState { float* score; int* fin; int* len; int* tok; int* par; int* htok; int* hpar; int* last; int* done; int* count; };

struct BeamSelectArgs {
  const float* part_m; const float* part_s; const float* part_v; const int* part_i;
  float* score; int* fin; int* len; int* tok; int* par; int* htok; int* hpar; int* last; int* done; int* count;
  int nblk, rows, t, eos, pad;
  int groups;                        // diverse beam search: G groups of K / G beams (1 = plain beam search, diversity unused)
  float diversity;                   // lambda >= 0: the Hamming penalty of a token per earlier group's selection of it this step
};

// f(std::integral_constant<int, K>()) for the beam width or sample count K = 1..kBeamMax (callers check the range first)
template <typename F>
int with_beam_k(int K, F&& f) {
  switch (K) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    default: return f(std::integral_constant<int, 8>());
  }
}

// beam.hip.  beam_init: slot 0 of every layer into the K rows of each image (layer 0's input row [0, din0): features in [0, E), zeros
// behind; h part = h0 or 0; c = c0 or 0; h0 / c0 f32 [NL, B, H] or null) and the state at t = 0: beam j live (score 0) where
// j % live_stride == 0, the others at -inf (live_stride K: beam search, K / G: the first beam of each diverse group, 1: the sampler),
// par[r] = r
int beam_init(const BeamLayerPtrs& slot0, int NL, int din0, int E, int H, int B, int K, int dtype, const float* features, const float* h0,
              const float* c0, const BeamState& s, hipStream_t stream, int live_stride);
// the generic path's GEMM input rows of t > 0: [x | h] of every layer from row par[r] of the previous output slot, x of layer 0 =
// embed[tok[r]]; c likewise
int beam_gather(const BeamLayerPtrs& in, const BeamLayerPtrs& out, int NL, int E, int H, int rows, int dtype, const float* embed, const int* tok,
                const int* par, const int* stop, int stop_at, hipStream_t stream);
// the generic path's tile partials of f32 logits [rows, V] (the fused path's are vocab_step_beam's epilogue)
int beam_tile_topk(const float* logits, int rows, int V, int K, float* part_m, float* part_s, float* part_v, int* part_i, const int* stop,
                   int stop_at, hipStream_t stream, const BanLists& bans = BanLists());
// a.groups == 1: plain beam search; else diverse beam search (the caller checks that a.groups divides K).  bans (decode constraints,
// bans.nban set): the kernel's tail builds the ban lists of step t + 1 by rule
int beam_select(const BeamSelectArgs& a, int K, int B, hipStream_t stream, const BanOut& bans = BanOut(), const BanRule& rule = BanRule());
// The ban lists of step 0 (decode constraints; empty histories), one wave per row.  The lists of step t + 1 are built by the tail of
// step t's selection kernel (beam_select with bans set, sample_step with out set), which holds the row's new token and parent:
// a launch per search, not per step
int ban_init(const BanOut& out, const BanRule& rule, int rows, hipStream_t stream);
// ids / scores / lengths of the K beams of each image, sorted within each group of `width` consecutive beams (width K: one sort of
// all K, beam search; K / G: the diverse groups, group g in slots g * width ..), best first; anc: null or i32 [B, K, L], the row
// (image * K + beam) of step t whose logits gave the t-th token of each returned beam (-1 past the last step that ran)
int beam_finalize(const BeamState& s, int B, int K, int L, int pad, float length_penalty, int width, int64_t* ids, float* scores,
                  int32_t* lengths, int32_t* anc, hipStream_t stream);

// ---- forced_beam.hip: lexically constrained beam search (gicap.h gic_forced_words).  The K beams of an image are S = 2^C state groups
// of Kg = K / S beams, beam j in state j / Kg (the bitmask of met constraint sets)
// force i32 [B][C][D] (the caller's, -1 padded); hop_id / hop_tgt i32, hop_val f32 [rows][kHopMax]: each row's hop tokens, the state each
// leads to, and its raw logit of the current step; init i32 [B]: the image's initial state (the bits of its absent sets).  The ids live on
// the device, so the host cannot refuse one outside [0, V): forced_init drops it (no row ever proposes it)
struct ForcedArgs { const int* force; int C, D, V; int* hop_id; int* hop_tgt; float* hop_val; int* init; };
// after beam_init: the rows' hop lists, init, and the scores of t = 0 (the first beam of the initial state's group at 0, the others -inf)
int forced_init(const ForcedArgs& f, const BeamState& s, int B, int K, hipStream_t stream);
// beam_tile_topk's forced form: bans and hops both set
int forced_tile_topk(const float* logits, int rows, int V, int K, float* part_m, float* part_s, float* part_v, int* part_i, const int* stop,
                     int stop_at, hipStream_t stream, const BanLists& bans, const HopLists& hops);
// the selection per state group (a.groups / a.diversity unused); its tail builds the ban lists of step t + 1 as beam_select's BAN form does
int forced_select(const BeamSelectArgs& a, const ForcedArgs& f, int K, int B, hipStream_t stream, const BanOut& bans, const BanRule& rule);
// beam_finalize in the forced order: real constraints met (descending), score / length^alpha (descending), beam index; dead beams last,
// as all-pad ids of length 0 and score -inf.  met i32 [B, K]: the returned beams' states (a dead beam's: the initial state)
int forced_finalize(const BeamState& s, const ForcedArgs& f, int B, int K, int L, int pad, float length_penalty, int64_t* ids, float* scores,
                    int32_t* lengths, int32_t* met, int32_t* anc, hipStream_t stream);

// attn_beam.hip: the attention kernels of one step (K rows per image, row r reads hp of row par[r]; the sampler's par[r] = r).  With
// lengths set, the packed form of teacher forcing (K = 1): row b = caption b reads its own hp row and takes part while t < lengths[b]
struct AttnStepArgs {
  const void* fproj;                 // act [B, P, A]
  const void* fmap;                  // act [B, P, C]
  const float* w_a;                  // [A]
  const float* hp;                   // [rows, A]: h W_h^T of the rows before the reorder
  const int* par;                    // [rows]
  float* e;                          // [rows, P] energies
  void* z; long ldx;                 // act: row r's z at z + r * ldx
  float* alpha;                      // [rows, P]: this step's slot of the alpha history, or null (packed form: never null)
  const int* stop; int stop_at;      // *stop >= stop_at: every image has finished
  int P, A, C;
  const int32_t* lengths = nullptr;  // packed form: [B]; par and stop unused
  int t = 0;                         // packed form: the step
  float* alphas = nullptr; long alphas_ld = 0;   // packed form: the caller's alphas at step t (caption b at + b * alphas_ld), or null
};
// attn_step_energy then attn_step_ctx for the K rows of each of the B images (rows = B * K)
int attn_step(const AttnStepArgs& f, int K, int B, int dtype, hipStream_t stream);
// alphas f32 [B, K, L, P] of the returned beams: row anc[b, j, t] of step t of the history ahist [L][rows][P] for t < lengths[b, j], else 0
int attn_beam_alphas(const float* ahist, const int* anc, const int* lengths, int rows, int L, int P, float* alphas, hipStream_t stream);

// sample.hip: the option checks of gic_sample_logits (decode = false) and the samplers (eos_id / pad_id too)
int check_sample_opts(const gic_sample_opts* o, int V, bool decode, const char* who);
// sample_select over f32 logits [rows, V] at step t: draws the next token of every live row into the state (score, len, tok, htok slot t,
// fin and count on <E>); noise_u f32 [L, rows, V] or null -> Philox(seed, stream t)
int sample_step(const float* logits, int rows, int V, const gic_sample_opts* o, const float* noise_u, uint64_t seed, int t, const BeamState& st,
                hipStream_t stream, const BanLists& bans = BanLists(), const BanOut& out = BanOut(), const BanRule& rule = BanRule());
// ids [rows][L] = each row's history up to its length, pad behind; scores / lengths [rows]
int sample_finalize(const BeamState& st, int rows, int L, int pad, int64_t* ids, float* scores, int32_t* lengths, hipStream_t stream);

// ---- ensemble.hip: the mixing step of the ensemble searches
// M in 1..GIC_MAX_ENSEMBLE, mode, every weight finite and > 0 (who: the prefix of the error text)
int check_ensemble_opts(const gic_ensemble_opts* o, const char* who);
// z f32 [rows, V] = the members' logits f32 [M][rows][V] (member m at logits + m * mstride) mixed by o (weights normalised here);
// stop (may be null) / stop_at as for the other step kernels
int ensemble_mix(const float* logits, long mstride, int rows, int V, const gic_ensemble_opts& o, float* out, const int* stop, int stop_at,
                 hipStream_t stream);

}  // namespace gic
