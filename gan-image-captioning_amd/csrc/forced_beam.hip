// Lexically constrained beam search (gicap.h gic_forced_words; Anderson et al., EMNLP 2017): the kernels of the forced head.  decode.hip
// drives them with the unchanged recurrences; the vocabulary side is vocab_step_beam_hop (decoder_step.hip) or forced_tile_topk.
//
// Image b carries C <= 3 constraint sets of D <= 4 token ids (force i32 [B][C][D], -1 padded; an all -1 set is absent and met from the
// start).  A hypothesis' state is the bitmask of the sets it has met.  The K beams of an image are S = 2^C state groups of Kg = K / S
// beams; beam j is in state j / Kg.  Since a row's state is fixed by its slot, so is its hop list (the ids of the sets outside its
// state): forced_init writes the lists once, and a step's selection moves hypotheses between slots, never lists between rows.
//
// One step, state group g: the Kg best of
//   stay  the top-K admissible non-hop tokens of each live parent of group g (the tile partials: hop tokens were kept out of them),
//   pad   the single proposal of each finished parent of group g,
//   hop   token w of a live parent p in state s != g with s | m(w) == g, at p's raw logit of w as the vocabulary side recorded it.
// Score = parent score + (logit - logsumexp of all V logits), for a hop exactly as for a stay.  A parent at -inf proposes nothing; a
// slot without a candidate is dead: score -inf, finished, length 0.
// Tie order (one total order, the oracle's too): score, then the lower parent beam, then stay before hop, then the rank within the
// parent's row (stay) or the slot c * D + d (hop).  ord = parent * 32 + (stay: rank, hop: 16 + slot) is that order's key.
#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {
namespace {

// one workgroup per image, thread = (beam j, slot i): row (img, j)'s hop list and the image's initial state
__global__ __launch_bounds__(128) void forced_init_kernel(const ForcedArgs f, float* score, int K) {
  const int img = blockIdx.x, tid = threadIdx.x;
  const int CD = f.C * f.D;
  const int* ids = f.force + (long)img * CD;
  int init = 0;
  for (int c = 0; c < f.C; ++c) {
    bool any = false;
    for (int d = 0; d < f.D; ++d) any = any || ids[c * f.D + d] >= 0;
    if (!any) init |= 1 << c;
  }
  const int Kg = K >> f.C;
  if (tid >= K * kHopMax) return;
  const int j = tid / kHopMax, i = tid % kHopMax, r = img * K + j;
  const int s = j / Kg;
  int id = -1, tgt = -1;
  if (i < CD && (s & init) == init && !((s >> (i / f.D)) & 1)) {
    id = ids[i] < f.V ? ids[i] : -1;
    for (int e = 0; e < i; ++e)                              // the token's first slot among the row's unmet sets speaks for it
      if (ids[e] == id && !((s >> (e / f.D)) & 1)) id = -1;
    if (id >= 0) {
      tgt = s;
      for (int e = 0; e < CD; ++e)
        if (ids[e] == id) tgt |= 1 << (e / f.D);
    }
  }
  f.hop_id[(long)r * kHopMax + i] = id;
  f.hop_tgt[(long)r * kHopMax + i] = tgt;
  f.hop_val[(long)r * kHopMax + i] = -INFINITY;
  if (i == 0) score[r] = j == init * Kg ? 0.f : -INFINITY;
  if (tid == 0) f.init[img] = init;
}

// beam_tile_topk_kernel's BAN form with the hop walk behind the ban walk (the generic path and its materialised logits)
template <int K>
__global__ __launch_bounds__(512) void forced_tile_topk_kernel(const float* __restrict__ logits, int rows, int V, int nblk, float* part_m,
                                                               float* part_s, float* part_v, int* part_i, const int* stop, int stop_at,
                                                               const BanLists bans, const HopLists hops) {
  if (*stop >= stop_at) return;
  const int tid = threadIdx.x, row = blockIdx.y * 64 + (tid >> 3), seg = tid & 7;
  const int v0 = blockIdx.x * kBeamTile + seg * 8;
  const int rr = min(row, rows - 1);
  float x[8], xs[8];
  int ixs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int v = v0 + e;
    x[e] = v < V ? logits[(long)rr * V + v] : -INFINITY;
    xs[e] = x[e];
    ixs[e] = v < V ? v : INT_MAX;
  }
  ban_apply8(xs, ixs, v0, bans.ban + (long)rr * bans.cap, bans.nban[rr]);
  hop_apply8(xs, ixs, v0, hops.id + (long)rr * kHopMax, hops.val + (long)rr * kHopMax, hops.n, row < rows);
  beam_tile_reduce8_sel<K>(x, xs, ixs, seg == 0 && row < rows, (long)rr * nblk + blockIdx.x, part_m, part_s, part_v, part_i);
}

// a lane's candidate: valid, score, order key, target state
struct Cand { bool v; float s; int ord; int tgt; };

// (valid, score, ord) order of the selection: valid first, larger score, then the lower order key
__device__ __forceinline__ bool cand_better(bool va, float a, int oa, bool vb, float b, int ob) {
  return va && (!vb || a > b || (a == b && oa < ob));
}

struct ForcedSelectArgs { BeamSelectArgs a; ForcedArgs f; BanOut out; BanRule rule; };

// one workgroup per image: wave w < K merges row (image, w)'s tile partials as beam_select does; then every wave runs the selection on
// the same LDS operands (the same result in every wave), wave 0 writes the state and wave j < K builds new beam j's ban list of step
// t + 1 from lane j of its own copy.  A lane holds up to three candidates: stay / pad (parent lane / K, rank lane % K) and the hop
// slots lane and lane + 64 of the image's K * kHopMax <= 96
template <int K>
__global__ __launch_bounds__(512) void forced_select_kernel(const ForcedSelectArgs g) {
  const BeamSelectArgs& a = g.a;
  __shared__ float cv[K][K], lse_s[K], hv[K][kHopMax], psc[K];
  __shared__ int ci[K][K], hid[K][kHopMax], htg[K][kHopMax], pfn[K], pln[K];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (a.done[img]) return;                                 // every beam of this image has finished: the step is the identity
  if (w < K) {
    const int r = img * K + w;
    float m = -INFINITY, s = 0.f;
    float lv[K]; int li[K];
#pragma unroll
    for (int q = 0; q < K; ++q) { lv[q] = -INFINITY; li[q] = INT_MAX; }
    for (int j = lane; j < a.nblk; j += 64) {
      const long o = (long)r * a.nblk + j;
      lse_combine(m, s, a.part_m[o], a.part_s[o]);
#pragma unroll
      for (int q = 0; q < K; ++q) beam_insert<K>(lv, li, a.part_v[o * K + q], a.part_i[o * K + q]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
      lse_combine(m, s, m2, s2);
    }
    beam_merge_levels<K, 0, 6>(lv, li);
    if (lane == 0) {
      lse_s[w] = m + logf(s);
#pragma unroll
      for (int q = 0; q < K; ++q) { cv[w][q] = lv[q]; ci[w][q] = li[q]; }
      psc[w] = a.score[r]; pfn[w] = a.fin[r]; pln[w] = a.len[r];
    }
    if (lane < kHopMax) {
      const long o = (long)r * kHopMax + lane;
      hid[w][lane] = g.f.hop_id[o]; htg[w][lane] = g.f.hop_tgt[o]; hv[w][lane] = g.f.hop_val[o];
    }
  }
  __syncthreads();                                         // (every read of the old state lies before this barrier)
  const int Kg = K >> g.f.C;
  Cand c[3];
  {
    const int p = min(lane / K, K - 1), q = lane % K;
    const bool fin = pfn[p] != 0;
    const float ps = psc[p];
    c[0].v = lane < K * K && ps != -INFINITY && (fin ? q == 0 : ci[p][q] != INT_MAX);
    c[0].s = fin ? ps : ps + (cv[p][q] - lse_s[p]);
    c[0].ord = p * 32 + q;
    c[0].tgt = p / Kg;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int idx = lane + 64 * h;
    const int p = min(idx / kHopMax, K - 1), i = idx % kHopMax;
    const float ps = psc[p];
    // (a value of -inf: the id was also on the row's ban list -- a C caller's suppressed id in a set -- and proposes nothing)
    c[1 + h].v = idx < K * kHopMax && pfn[p] == 0 && ps != -INFINITY && hid[p][i] >= 0 && hv[p][i] != -INFINITY;
    c[1 + h].s = ps + (hv[p][i] - lse_s[p]);
    c[1 + h].ord = p * 32 + 16 + i;
    c[1 + h].tgt = htg[p][i];
  }
  float my_s = -INFINITY; int my_t = a.pad, my_p = lane < K ? lane : 0, my_fin = 1, my_len = 0;      // (a slot nobody lands in: dead)
  for (int slot = 0; slot < K; ++slot) {
    const int grp = slot / Kg;
    // ---- the lane's best candidate for the group, then a wave argmax; the winner leaves the pool
    bool bv = false; float bs = -INFINITY; int bo = INT_MAX;
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const bool v = c[h].v && c[h].tgt == grp;
      if (cand_better(v, c[h].s, c[h].ord, bv, bs, bo)) { bv = v; bs = c[h].s; bo = c[h].ord; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const bool ov = __shfl_xor((int)bv, o, 64) != 0;
      const float os = __shfl_xor(bs, o, 64);
      const int oo = __shfl_xor(bo, o, 64);
      if (cand_better(ov, os, oo, bv, bs, bo)) { bv = ov; bs = os; bo = oo; }
    }
    if (!bv) continue;                                     // (wave-uniform: the butterfly leaves every lane the same winner)
#pragma unroll
    for (int h = 0; h < 3; ++h)
      if (c[h].ord == bo) c[h].v = false;                  // (order keys are unique, and a candidate has one target group)
    if (lane == slot) {
      const int p = bo >> 5, i = bo & 31;
      const bool fin = pfn[p] != 0;
      const int tok = i >= 16 ? hid[p][i - 16] : fin ? a.pad : ci[p][i];
      my_s = bs; my_t = tok; my_p = p; my_fin = fin || tok == a.eos; my_len = fin ? pln[p] : a.t + 1;
    }
  }
  const int all_fin = __all(lane >= K || my_fin);
  if (lane < K && w == 0) {
    const int r = img * K + lane;
    a.score[r] = my_s; a.fin[r] = my_fin; a.len[r] = my_len; a.tok[r] = my_t; a.par[r] = img * K + my_p;
    a.htok[(long)a.t * a.rows + r] = my_t;
    a.hpar[(long)a.t * a.rows + r] = my_p;
  }
  if (lane == 0 && w == 0) {
    a.last[img] = a.t;
    if (all_fin) { a.done[img] = 1; atomicAdd(a.count, 1); }      // (integer count: the later launches of the search return at once)
  }
  // ---- wave j < K: the ban list of step t + 1 for the image's new beam j, as in beam_select's BAN form: its parent's flat history (slot
  // t % 2) plus the token it just took, written to slot (t + 1) % 2 on the way.  A finished or dead beam gets an empty list
  __shared__ int hs[K][1024];                              // (L <= 1024: decode_dims)
  const BanOut& o = g.out;
  const int tn = a.t + 1, L = o.L;
  const int j = w < K ? w : 0, r = img * K + j;
  const int kp = __shfl(my_p, j, 64), kt = __shfl(my_t, j, 64), kf = __shfl(my_fin, j, 64);
  const bool next = w < K && tn < L && !all_fin;
  if (next && !kf) {
    const int* src = o.hist + ((long)(a.t & 1) * a.rows + img * K + kp) * L;
    int* dst = o.hist + ((long)(tn & 1) * a.rows + r) * L;
    for (int i = lane; i < tn; i += 64) {
      const int y = i < a.t ? src[i] : kt;
      hs[j][i] = y;
      dst[i] = y;
    }
  }
  __syncthreads();
  if (next) {
    if (kf) { if (lane == 0) o.nban[r] = 0; }
    else ban_list_wave(hs[j], tn, lane, g.rule, o.ban + (long)r * o.cap, o.nban + r);
  }
}

// beam_finalize_kernel in the forced order (file comment of beam.h's forced_finalize)
__global__ __launch_bounds__(64) void forced_finalize_kernel(const float* __restrict__ score, const int* __restrict__ len, const int* __restrict__ htok,
                                                             const int* __restrict__ hpar, const int* __restrict__ last, const int* __restrict__ init,
                                                             int K, int Kg, int L, int rows, int pad, float alpha, int64_t* __restrict__ ids,
                                                             float* __restrict__ scores_out, int32_t* __restrict__ lengths_out,
                                                             int32_t* __restrict__ met, int32_t* __restrict__ anc) {
  extern __shared__ int hs[];                              // [L][K] tokens, then [L][K] parent beams
  __shared__ int rank_s[kBeamMax], dead_s[kBeamMax];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int tl = last[img], s0 = init[img];
  for (int i = tid; i < (tl + 1) * K; i += 64) {
    const int t = i / K, j = i % K;
    hs[i] = htok[(long)t * rows + img * K + j];
    hs[L * K + i] = hpar[(long)t * rows + img * K + j];
  }
  if (tid < K) {
    const int r = img * K + tid;
    const bool dead = score[r] == -INFINITY;
    const int nm = __popc((tid / Kg) & ~s0);
    const float ns = dead ? -INFINITY : score[r] / powf((float)len[r], alpha);
    int rank = 0;
    for (int i = 0; i < K; ++i) {
      const bool od = score[img * K + i] == -INFINITY;
      const int om = __popc((i / Kg) & ~s0);
      const float os = od ? -INFINITY : score[img * K + i] / powf((float)len[img * K + i], alpha);
      bool before;
      if (od != dead) before = dead;
      else if (dead) before = i < tid;
      else before = om > nm || (om == nm && (os > ns || (os == ns && i < tid)));
      rank += before ? 1 : 0;
    }
    rank_s[tid] = rank;
    dead_s[tid] = dead;
    scores_out[(long)img * K + rank] = dead ? -INFINITY : score[r];
    lengths_out[(long)img * K + rank] = dead ? 0 : len[r];
    met[(long)img * K + rank] = dead ? s0 : tid / Kg;
  }
  __syncthreads();
  for (int i = tid; i < K * L; i += 64) {                  // positions past the last step that ran, and the dead beams
    const int j = i / L, t = i % L;
    if (t > tl || dead_s[j]) {
      ids[((long)img * K + rank_s[j]) * L + t] = pad;
      if (anc) anc[((long)img * K + rank_s[j]) * L + t] = -1;
    }
  }
  if (tid < K && !dead_s[tid]) {
    int64_t* row = ids + ((long)img * K + rank_s[tid]) * L;
    int32_t* arow = anc ? anc + ((long)img * K + rank_s[tid]) * L : nullptr;
    int cur = tid;
    for (int t = tl; t >= 0; --t) {
      row[t] = hs[t * K + cur];
      cur = hs[L * K + t * K + cur];
      if (arow) arow[t] = img * K + cur;              // the parent row of step t: its logits gave this token
    }
  }
}

// f(std::integral_constant<int, K>()) for the forced search's beam sizes (even: 2^C divides K, C >= 1)
template <typename F>
int with_forced_k(int K, F&& f) {
  switch (K) {
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 6: return f(std::integral_constant<int, 6>());
    default: return f(std::integral_constant<int, 8>());
  }
}

int check_forced_args(const ForcedArgs& f, int K, const char* who) {
  GIC_CHECK_ARG(f.force && f.hop_id && f.hop_tgt && f.hop_val && f.init, "%s: null buffer", who);
  GIC_CHECK_ARG(f.C >= 1 && f.C <= kForceSetsMax && f.D >= 1 && f.D <= kForceIdsMax && K >= 2 && K <= kBeamMax && K % (1 << f.C) == 0,
                "%s: bad dims", who);
  return GIC_OK;
}

}  // namespace

int forced_init(const ForcedArgs& f, const BeamState& s, int B, int K, hipStream_t stream) {
  GIC_PROPAGATE(check_forced_args(f, K, "forced_init"));
  hipLaunchKernelGGL(forced_init_kernel, dim3((unsigned)B), dim3(128), 0, stream, f, s.score, K);
  GIC_CHECK_LAUNCH("forced_init");
  return GIC_OK;
}

int forced_tile_topk(const float* logits, int rows, int V, int K, float* part_m, float* part_s, float* part_v, int* part_i, const int* stop,
                     int stop_at, hipStream_t stream, const BanLists& bans, const HopLists& hops) {
  GIC_CHECK_ARG(bans.nban && bans.ban && hops.id && hops.val && hops.n >= 1 && hops.n <= kHopMax && K >= 2 && K <= kBeamMax && K % 2 == 0, "forced_tile_topk: bad arguments");
  const int nblk = cdiv(V, kBeamTile);
  return with_forced_k(K, [&](auto k) -> int {
    const dim3 grid((unsigned)nblk, (unsigned)cdiv(rows, 64));
    hipLaunchKernelGGL((forced_tile_topk_kernel<k>), grid, dim3(512), 0, stream, logits, rows, V, nblk, part_m, part_s, part_v, part_i, stop,
                       stop_at, bans, hops);
    GIC_CHECK_LAUNCH("forced_tile_topk");
    return GIC_OK;
  });
}

int forced_select(const BeamSelectArgs& a, const ForcedArgs& f, int K, int B, hipStream_t stream, const BanOut& bans, const BanRule& rule) {
  GIC_PROPAGATE(check_forced_args(f, K, "forced_select"));
  GIC_CHECK_ARG(bans.nban && bans.ban && bans.hist && bans.L >= 1 && bans.L <= 1024, "forced_select: the ban lists must be set");
  const ForcedSelectArgs g{a, f, bans, rule};
  return with_forced_k(K, [&](auto k) -> int {
    hipLaunchKernelGGL((forced_select_kernel<k>), dim3((unsigned)B), dim3(512), 0, stream, g);
    GIC_CHECK_LAUNCH("forced_select");
    return GIC_OK;
  });
}

int forced_finalize(const BeamState& s, const ForcedArgs& f, int B, int K, int L, int pad, float length_penalty, int64_t* ids, float* scores,
                    int32_t* lengths, int32_t* met, int32_t* anc, hipStream_t stream) {
  GIC_PROPAGATE(check_forced_args(f, K, "forced_finalize"));
  const size_t lds = (size_t)2 * L * K * sizeof(int);
  static LdsGrant gfin;
  GIC_CHECK_ARG(grant_lds(forced_finalize_kernel, lds, gfin), "forced_finalize: cannot reserve %zu bytes of LDS", lds);
  hipLaunchKernelGGL(forced_finalize_kernel, dim3((unsigned)B), dim3(64), lds, stream, s.score, s.len, s.htok, s.hpar, s.last, f.init, K,
                     K >> f.C, L, B * K, pad, length_penalty, ids, scores, lengths, met, anc);
  GIC_CHECK_LAUNCH("forced_finalize");
  return GIC_OK;
}

}  // namespace gic
