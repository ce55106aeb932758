// Beam-search kernels (beam.h): init, the generic path's gather and tile top-k, the per-image selection, the final sort.  The step loop
// that drives them, and the workspace they share, is decode.hip's.
#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {
namespace {

using LayerPtrs = BeamLayerPtrs;

// slot 0 of every layer: x part of layer 0 = the image's features (zeros in [E, din0)), h part = h0 (or 0), c = c0 (or 0); beam state at
// t = 0: beam j live where j % live_stride == 0 (the others at -inf, so the beams of a search, or of a diverse group, never copy one
// hypothesis)
template <typename TA>
__global__ __launch_bounds__(256) void beam_init_kernel(LayerPtrs p, int NL, int din0, int E, int H, int B, int K, const float* __restrict__ features,
                                                        const float* __restrict__ h0, const float* __restrict__ c0, float* score, int* fin, int* len,
                                                        int* tok, int* par, int* last, int* done, int* count, int live_stride) {
  const int r = blockIdx.x, img = r / K, tid = threadIdx.x;
  for (int l = 0; l < NL; ++l) {
    const int din = l == 0 ? din0 : H;
    const long ld = din + H;
    TA* x = (TA*)p.xh[l] + (long)r * ld;
    for (int e = tid; e < din; e += 256) x[e] = from_f32<TA>(l == 0 && e < E ? features[(long)img * E + e] : 0.f);
    for (int j = tid; j < H; j += 256) {
      const long s = ((long)l * B + img) * H + j;
      x[din + j] = from_f32<TA>(h0 ? h0[s] : 0.f);
      p.c[l][(long)r * H + j] = c0 ? c0[s] : 0.f;
    }
  }
  if (tid == 0) {
    score[r] = (r % K) % live_stride == 0 ? 0.f : -INFINITY;
    fin[r] = 0; len[r] = 0; tok[r] = 0; par[r] = r;
    if (r % K == 0) { last[img] = -1; done[img] = 0; }
    if (r == 0) *count = 0;
  }
}

// generic path, t > 0: the GEMM input rows [x | h] of every layer from the parent rows of the previous step's output, layer 0's x part =
// embed[token]; the cell state likewise
template <typename TA>
__global__ __launch_bounds__(256) void beam_gather_kernel(LayerPtrs in, LayerPtrs out, int NL, int E, int H, const float* __restrict__ embed,
                                                          const int* __restrict__ tok, const int* __restrict__ par, const int* stop, int stop_at) {
  if (*stop >= stop_at) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int p = par[r], id = tok[r];
  for (int l = 0; l < NL; ++l) {
    const int din = l == 0 ? E : H;
    const long ld = din + H;
    TA* dst = (TA*)in.xh[l] + (long)r * ld;
    const TA* src = (const TA*)out.xh[l] + (long)p * ld;
    if (l == 0)
      for (int e = tid; e < E; e += 256) dst[e] = from_f32<TA>(embed[(long)id * E + e]);
    for (int j = tid; j < H; j += 256) {
      dst[din + j] = src[din + j];
      in.c[l][(long)r * H + j] = out.c[l][(long)p * H + j];
    }
  }
}

// generic path: tile partials of an f32 logits matrix [rows, V] (any V: a ragged last tile reads -inf past V); 8 lanes per (row, tile).
// BAN: the tile's top-K is taken from the copy without the row's banned ids (its max and sum of exp stay those of the raw values)
// (Ban = BanLists, else the empty NoBan: the unconstrained instantiation keeps its argument layout)
struct NoBan {};

template <int K, bool BAN, typename Ban>
__global__ __launch_bounds__(512) void beam_tile_topk_kernel(const float* __restrict__ logits, int rows, int V, int nblk, float* part_m,
                                                             float* part_s, float* part_v, int* part_i, const int* stop, int stop_at,
                                                             const Ban bans) {
  if (*stop >= stop_at) return;
  const int tid = threadIdx.x, row = blockIdx.y * 64 + (tid >> 3), seg = tid & 7;
  const int v0 = blockIdx.x * kBeamTile + seg * 8;
  const int rr = min(row, rows - 1);
  float x[8];
  int ix[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int v = v0 + e;
    x[e] = v < V ? logits[(long)rr * V + v] : -INFINITY;
    ix[e] = v < V ? v : INT_MAX;
  }
  if constexpr (BAN) {
    float xs[8];
    int ixs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { xs[e] = x[e]; ixs[e] = ix[e]; }
    ban_apply8(xs, ixs, v0, bans.ban + (long)rr * bans.cap, bans.nban[rr]);
    beam_tile_reduce8_sel<K>(x, xs, ixs, seg == 0 && row < rows, (long)rr * nblk + blockIdx.x, part_m, part_s, part_v, part_i);
  } else {
    beam_tile_reduce8<K>(x, ix, seg == 0 && row < rows, (long)rr * nblk + blockIdx.x, part_m, part_s, part_v, part_i);
  }
}

// one wave per row: the ban list of step 0
__global__ __launch_bounds__(64) void ban_init_kernel(const BanOut o, const BanRule rule) {
  const int r = blockIdx.x;
  ban_list_wave(nullptr, 0, threadIdx.x, rule, o.ban + (long)r * o.cap, o.nban + r);
}

using SelectArgs = BeamSelectArgs;

// (candidate score, lane) order of the selection: valid first, larger score, then the lower (parent beam, rank) = lower lane
__device__ __forceinline__ bool sel_better(bool va, float a, int la, bool vb, float b, int lb) {
  return va && (!vb || a > b || (a == b && la < lb));
}

// one workgroup per image: wave w < K merges row (image, w)'s tile partials into its logsumexp and top-K; wave 0 selects.  DIVERSE:
// the G = a.groups groups of Kg = K / G beams select in order g = 0..G-1, each over the candidates of its own Kg parents (lane = local
// parent * K + rank, at most Kg * K <= 64 lanes), ranked by score + logp - diversity * h(token), where h counts the earlier groups' picks
// of the token from live parents at this step; the kept score is the raw score + logp.  Plain beam search (G = 1) is the other
// instantiation, so its selection is the one it always was.
// BAN (decode constraints; Ban = BanArgs, else NoBan): the kernel's tail builds the ban lists of step t + 1.  Every wave then runs the
// selection (the same reads, the same result in every wave), wave 0 alone writes the state -- after a barrier, so that no wave still
// reads what it overwrites -- and wave j < K takes beam j's parent and token from lane j of its own copy: no exchange through LDS
struct BanArgs { BanOut out; BanRule rule; };

template <int K, bool DIVERSE, bool BAN, typename Ban>
__global__ __launch_bounds__(512) void beam_select_kernel(const SelectArgs a, const Ban ban) {
  __shared__ float cv[K][K], lse_s[K];
  __shared__ int ci[K][K];
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
    }
  }
  __syncthreads();
  if constexpr (!BAN) {
    if (w != 0) return;
  }
  float my_s = 0.f; int my_t = 0, my_p = 0, my_fin = 0, my_len = 0;
  if constexpr (!DIVERSE) {
    // ---- candidates: lane = p * K + q (parent beam p, rank q in its row)
    const int p = lane / K, q = lane % K;
    const bool in = lane < K * K;
    const int pr = img * K + (in ? p : 0);
    const bool pfin = a.fin[pr] != 0;
    const float ps = a.score[pr];
    const int plen = a.len[pr];
    bool valid = in && (!pfin || q == 0);
    float cs = -INFINITY;
    int ct = a.pad;
    if (valid) {
      if (pfin) cs = ps;
      else { cs = ps + (cv[p][q] - lse_s[p]); ct = ci[p][q]; }
    }
    // ---- K rounds of a wave argmax with exclusion; lane n keeps the n-th winner
#pragma unroll
    for (int n = 0; n < K; ++n) {
      bool bv = valid; float bs = cs; int bl = lane;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const bool ov = __shfl_xor((int)bv, o, 64) != 0;
        const float os = __shfl_xor(bs, o, 64);
        const int ol = __shfl_xor(bl, o, 64);
        if (sel_better(ov, os, ol, bv, bs, bl)) { bv = ov; bs = os; bl = ol; }
      }
      const float ws = __shfl(cs, bl, 64);
      const int wt = __shfl(ct, bl, 64), wp = __shfl(p, bl, 64), wf = __shfl((int)pfin, bl, 64), wlen = __shfl(plen, bl, 64);
      if (lane == bl) valid = false;
      if (lane == n) { my_s = ws; my_t = wt; my_p = wp; my_fin = wf || wt == a.eos; my_len = wf ? wlen : a.t + 1; }
    }
  } else {
    const int Kg = K / a.groups;
    int my_h = -1;                                         // this lane's kept token if it counts toward h (its parent was live), else -1
    for (int g = 0; g < a.groups; ++g) {
      // ---- the group's candidates: lane = pl * K + q (parent beam p = g * Kg + pl, rank q in its row)
      const int pl = lane / K, q = lane % K, p = g * Kg + pl;
      const bool in = lane < Kg * K;
      const int pr = img * K + (in ? p : 0);
      const bool pfin = a.fin[pr] != 0;
      const float ps = a.score[pr];
      const int plen = a.len[pr];
      bool valid = in && (!pfin || q == 0);
      float cs = -INFINITY;
      int ct = a.pad;
      if (valid) {
        if (pfin) cs = ps;
        else { cs = ps + (cv[p][q] - lse_s[p]); ct = ci[p][q]; }
      }
      // h: the picks of the groups before g (lanes 0 .. g * Kg - 1 hold them) that carry this token; a finished parent's pad proposal
      // is neither counted nor penalised
      int h = 0;
      for (int j = 0; j < g * Kg; ++j) h += __shfl(my_h, j, 64) == ct ? 1 : 0;
      const float key = valid && !pfin ? cs - a.diversity * (float)h : cs;
      // ---- Kg rounds of a wave argmax with exclusion over the keys; lane g * Kg + n keeps the n-th winner
      for (int n = 0; n < Kg; ++n) {
        bool bv = valid; float bs = key; int bl = lane;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const bool ov = __shfl_xor((int)bv, o, 64) != 0;
          const float os = __shfl_xor(bs, o, 64);
          const int ol = __shfl_xor(bl, o, 64);
          if (sel_better(ov, os, ol, bv, bs, bl)) { bv = ov; bs = os; bl = ol; }
        }
        const float ws = __shfl(cs, bl, 64);
        const int wt = __shfl(ct, bl, 64), wp = __shfl(p, bl, 64), wf = __shfl((int)pfin, bl, 64), wlen = __shfl(plen, bl, 64);
        if (lane == bl) valid = false;
        if (lane == g * Kg + n) {
          my_s = ws; my_t = wt; my_p = wp; my_fin = wf || wt == a.eos; my_len = wf ? wlen : a.t + 1;
          my_h = wf ? -1 : wt;
        }
      }
    }
  }
  const int all_fin = __all(lane >= K || my_fin);
  if constexpr (BAN) __syncthreads();
  if (lane < K && (!BAN || w == 0)) {
    const int r = img * K + lane;
    a.score[r] = my_s; a.fin[r] = my_fin; a.len[r] = my_len; a.tok[r] = my_t; a.par[r] = img * K + my_p;
    a.htok[(long)a.t * a.rows + r] = my_t;
    a.hpar[(long)a.t * a.rows + r] = my_p;
  }
  if (lane == 0 && (!BAN || w == 0)) {
    a.last[img] = a.t;
    if (all_fin) { a.done[img] = 1; atomicAdd(a.count, 1); }      // (integer count: the later launches of the search return at once)
  }
  if constexpr (BAN) {
    // ---- wave j < K: the ban list of step t + 1 for the image's new beam j -- its history is its parent's flat history (slot t % 2)
    // plus the token it just took, written to slot (t + 1) % 2 on the way.  A finished beam gets an empty list, a finished image
    // none (nothing reads it), and the last step has no successor
    __shared__ int hs[K][1024];                            // (L <= 1024: decode_dims)
    const BanOut& o = ban.out;
    const int tn = a.t + 1, L = o.L;                       // tokens emitted so far
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
      else ban_list_wave(hs[j], tn, lane, ban.rule, o.ban + (long)r * o.cap, o.nban + r);
    }
  }
}

// one workgroup per image: walk each beam's parent pointers back through the history, sort each group of W consecutive beams by
// score / length^alpha (descending, ties to the lower beam index; W = K: one group) into the group's slots, write ids [B, K, L] (pad
// after <E> and after the last step run), scores, lengths
__global__ __launch_bounds__(64) void beam_finalize_kernel(const float* __restrict__ score, const int* __restrict__ len, const int* __restrict__ htok,
                                                           const int* __restrict__ hpar, const int* __restrict__ last, int K, int W, int L, int rows, int pad,
                                                           float alpha, int64_t* __restrict__ ids, float* __restrict__ scores_out,
                                                           int32_t* __restrict__ lengths_out, int32_t* __restrict__ anc) {
  extern __shared__ int hs[];                              // [L][K] tokens, then [L][K] parent beams
  __shared__ int rank_s[kBeamMax];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int tl = last[img];
  for (int i = tid; i < (tl + 1) * K; i += 64) {
    const int t = i / K, j = i % K;
    hs[i] = htok[(long)t * rows + img * K + j];
    hs[L * K + i] = hpar[(long)t * rows + img * K + j];
  }
  if (tid < K) {
    const int r = img * K + tid, g0 = tid - tid % W;
    const float ns = score[r] / powf((float)len[r], alpha);
    int rank = g0;
    for (int i = g0; i < g0 + W; ++i) {
      const float o = score[img * K + i] / powf((float)len[img * K + i], alpha);
      rank += (o > ns || (o == ns && i < tid)) ? 1 : 0;
    }
    rank_s[tid] = rank;
    scores_out[(long)img * K + rank] = score[r];
    lengths_out[(long)img * K + rank] = len[r];
  }
  __syncthreads();
  for (int i = tid; i < K * L; i += 64) {                  // positions past the last step that ran
    const int j = i / L, t = i % L;
    if (t > tl) {
      ids[((long)img * K + rank_s[j]) * L + t] = pad;
      if (anc) anc[((long)img * K + rank_s[j]) * L + t] = -1;
    }
  }
  if (tid < K) {
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

}  // namespace

int beam_select(const SelectArgs& s, int K, int B, hipStream_t stream, const BanOut& bans, const BanRule& rule) {
  return with_beam_k(K, [&](auto k) -> int {
    if (bans.nban) {
      const BanArgs ban{bans, rule};
      if (s.groups > 1) hipLaunchKernelGGL((beam_select_kernel<k, true, true, BanArgs>), dim3(B), dim3(512), 0, stream, s, ban);
      else hipLaunchKernelGGL((beam_select_kernel<k, false, true, BanArgs>), dim3(B), dim3(512), 0, stream, s, ban);
    } else if (s.groups > 1) {
      hipLaunchKernelGGL((beam_select_kernel<k, true, false, NoBan>), dim3(B), dim3(512), 0, stream, s, NoBan());
    } else {
      hipLaunchKernelGGL((beam_select_kernel<k, false, false, NoBan>), dim3(B), dim3(512), 0, stream, s, NoBan());
    }
    GIC_CHECK_LAUNCH("beam_select");
    return GIC_OK;
  });
}

int beam_gather(const BeamLayerPtrs& in, const BeamLayerPtrs& out, int NL, int E, int H, int rows, int dtype, const float* embed, const int* tok,
                const int* par, const int* stop, int stop_at, hipStream_t stream) {
  if (dtype == DT_F32)
    hipLaunchKernelGGL((beam_gather_kernel<float>), dim3((unsigned)rows), dim3(256), 0, stream, in, out, NL, E, H, embed, tok, par, stop, stop_at);
  else
    hipLaunchKernelGGL((beam_gather_kernel<bf16_t>), dim3((unsigned)rows), dim3(256), 0, stream, in, out, NL, E, H, embed, tok, par, stop, stop_at);
  GIC_CHECK_LAUNCH("beam_gather");
  return GIC_OK;
}

int beam_tile_topk(const float* logits, int rows, int V, int K, float* part_m, float* part_s, float* part_v, int* part_i, const int* stop,
                   int stop_at, hipStream_t stream, const BanLists& bans) {
  const int nblk = cdiv(V, kBeamTile);
  return with_beam_k(K, [&](auto k) -> int {
    const dim3 grid((unsigned)nblk, (unsigned)cdiv(rows, 64));
    if (bans.nban)
      hipLaunchKernelGGL((beam_tile_topk_kernel<k, true, BanLists>), grid, dim3(512), 0, stream, logits, rows, V, nblk, part_m, part_s, part_v,
                         part_i, stop, stop_at, bans);
    else
      hipLaunchKernelGGL((beam_tile_topk_kernel<k, false, NoBan>), grid, dim3(512), 0, stream, logits, rows, V, nblk, part_m, part_s, part_v,
                         part_i, stop, stop_at, NoBan());
    GIC_CHECK_LAUNCH("beam_tile_topk");
    return GIC_OK;
  });
}

int ban_init(const BanOut& out, const BanRule& rule, int rows, hipStream_t stream) {
  GIC_CHECK_ARG(out.nban && out.ban && out.L >= 1 && out.L <= 1024 && rule.S >= 0 && rule.S <= kBanSuppressMax && out.cap >= rule.S + 1 + out.L,
                "ban_init: bad dims");
  hipLaunchKernelGGL(ban_init_kernel, dim3((unsigned)rows), dim3(64), 0, stream, out, rule);
  GIC_CHECK_LAUNCH("ban_init");
  return GIC_OK;
}

int beam_init(const BeamLayerPtrs& slot0, int NL, int din0, int E, int H, int B, int K, int dtype, const float* features, const float* h0,
              const float* c0, const BeamState& s, hipStream_t stream, int live_stride) {
  const dim3 grid((unsigned)(B * K));
  if (dtype == DT_F32)
    hipLaunchKernelGGL((beam_init_kernel<float>), grid, dim3(256), 0, stream, slot0, NL, din0, E, H, B, K, features, h0, c0, s.score, s.fin,
                       s.len, s.tok, s.par, s.last, s.done, s.count, live_stride);
  else
    hipLaunchKernelGGL((beam_init_kernel<bf16_t>), grid, dim3(256), 0, stream, slot0, NL, din0, E, H, B, K, features, h0, c0, s.score, s.fin,
                       s.len, s.tok, s.par, s.last, s.done, s.count, live_stride);
  GIC_CHECK_LAUNCH("beam_init");
  return GIC_OK;
}

int beam_finalize(const BeamState& s, int B, int K, int L, int pad, float length_penalty, int width, int64_t* ids, float* scores,
                  int32_t* lengths, int32_t* anc, hipStream_t stream) {
  const size_t lds = (size_t)2 * L * K * sizeof(int);
  static LdsGrant gfin;
  GIC_CHECK_ARG(grant_lds(beam_finalize_kernel, lds, gfin), "beam_finalize: cannot reserve %zu bytes of LDS", lds);
  hipLaunchKernelGGL(beam_finalize_kernel, dim3((unsigned)B), dim3(64), lds, stream, s.score, s.len, s.htok, s.hpar, s.last, K, width, L, B * K, pad,
                     length_penalty, ids, scores, lengths, anc);
  GIC_CHECK_LAUNCH("beam_finalize");
  return GIC_OK;
}

}  // namespace gic
