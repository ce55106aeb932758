// Beam-search caption decode (gicap.h gic_decoder_beam_search); design notes in beam.h.
//
// Scratch (one caller-owned workspace, gic_decoder_beam_ws_bytes; every region 256-byte aligned), rows = B * k:
//   xh[l]     act [2][rows][Din_l + H]   fused path: slots t % 2 / (t + 1) % 2 hold [x_t | h_{t-1}] / h_t (read from parent rows);
//                                        generic path: slot 0 = the gathered GEMM input, slot 1 = the pointwise output
//   c[l]      f32 [2][rows][H]           as xh
//   gpre, logits (generic path only)     f32 [rows][4H], [rows][V]
//   part_m, part_s f32 [rows][nblk]; part_v f32, part_i i32 [rows][nblk][k]     tile partials (nblk = ceil(V / 64))
//   score f32, fin / len / tok / par i32 [rows]; hist_tok / hist_par i32 [L][rows]; last / img_done i32 [B]; count i32 [1]
#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {

int lstm_pointwise_fwd(int dt, const float* gpre, const float* c_prev, float* c_new, void* h_next, long ld_next, void* h_up, long ld_up,
                       int rows, int H, hipStream_t stream);      // decoder.hip

namespace {

struct BeamDims {
  int B, L, V, E, H, NL, dt, K, rows, nblk;
  bool fused;
  int din(int l) const { return l == 0 ? E : H; }
  long ldx(int l) const { return (long)din(l) + H; }
  size_t asz() const { return (size_t)dtype_size(dt); }
};

struct BeamLayout {
  size_t xh[GIC_MAX_LAYERS], c[GIC_MAX_LAYERS], gpre, logits, pm, ps, pv, pi, score, fin, len, tok, par, htok, hpar, last, done, count, total;
};

BeamLayout beam_layout(const BeamDims& d) {
  BeamLayout o{};
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t p = at; at += (bytes + 255) & ~(size_t)255; return p; };
  const size_t R = d.rows, pn = (size_t)d.rows * d.nblk;
  for (int l = 0; l < d.NL; ++l) {
    o.xh[l] = take(2 * R * d.ldx(l) * d.asz());
    o.c[l] = take(2 * R * d.H * 4);
  }
  o.gpre = d.fused ? 0 : take(R * 4 * d.H * 4);
  o.logits = d.fused ? 0 : take(R * d.V * 4);
  o.pm = take(pn * 4); o.ps = take(pn * 4);
  o.pv = take(pn * d.K * 4); o.pi = take(pn * d.K * 4);
  o.score = take(R * 4); o.fin = take(R * 4); o.len = take(R * 4); o.tok = take(R * 4); o.par = take(R * 4);
  o.htok = take((size_t)d.L * R * 4); o.hpar = take((size_t)d.L * R * 4);
  o.last = take((size_t)d.B * 4); o.done = take((size_t)d.B * 4); o.count = take(4);
  o.total = at;
  return o;
}

int beam_dims(const gic_decoder_dims* dims, int K, BeamDims& d) {
  GIC_CHECK_ARG(dims, "decoder_beam: null dims");
  GIC_CHECK_ARG(dims->B > 0 && dims->L > 0 && dims->V > 1 && dims->E > 0 && dims->H > 0, "decoder_beam: bad dims");
  GIC_CHECK_ARG(dims->NL >= 1 && dims->NL <= GIC_MAX_LAYERS, "decoder_beam: gen_num_layers must be 1..%d", GIC_MAX_LAYERS);
  GIC_CHECK_ARG(dims->dtype == DT_F32 || dims->dtype == DT_BF16, "decoder_beam: bad dtype");
  GIC_CHECK_ARG(K >= 1 && K <= kBeamMax, "decoder_beam: beam size must be 1..%d, got %d", kBeamMax, K);
  GIC_CHECK_ARG(K <= dims->V, "decoder_beam: beam size %d exceeds the vocabulary (%d)", K, dims->V);
  GIC_CHECK_ARG(dims->L <= 1024, "decoder_beam: at most 1024 steps");
  GIC_CHECK_ARG((long)dims->B * K <= (1l << 24), "decoder_beam: too many rows");
  d.B = dims->B; d.L = dims->L; d.V = dims->V; d.E = dims->E; d.H = dims->H; d.NL = dims->NL; d.dt = dims->dtype; d.K = K;
  d.rows = d.B * K;
  d.nblk = cdiv(d.V, kBeamTile);
  d.fused = d.rows <= decoder_step_max_rows() && decoder_step_supported(d.dt, d.V, d.E, d.H, d.NL);
  return GIC_OK;
}

using LayerPtrs = BeamLayerPtrs;

// slot 0 of every layer: x part of layer 0 = the image's features (zeros in [E, din0)), h part = h0 (or 0), c = c0 (or 0); beam state at
// t = 0: only beam 0 live (the others at -inf, so the k beams never copy one hypothesis)
template <typename TA>
__global__ __launch_bounds__(256) void beam_init_kernel(LayerPtrs p, int NL, int din0, int E, int H, int B, int K, const float* __restrict__ features,
                                                        const float* __restrict__ h0, const float* __restrict__ c0, float* score, int* fin, int* len,
                                                        int* tok, int* par, int* last, int* done, int* count, int all_live) {
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
    score[r] = all_live || r % K == 0 ? 0.f : -INFINITY;
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

// generic path: tile partials of an f32 logits matrix [rows, V] (any V: a ragged last tile reads -inf past V); 8 lanes per (row, tile)
template <int K>
__global__ __launch_bounds__(512) void beam_tile_topk_kernel(const float* __restrict__ logits, int rows, int V, int nblk, float* part_m,
                                                             float* part_s, float* part_v, int* part_i, const int* stop, int stop_at) {
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
  beam_tile_reduce8<K>(x, ix, seg == 0 && row < rows, (long)rr * nblk + blockIdx.x, part_m, part_s, part_v, part_i);
}

using SelectArgs = BeamSelectArgs;

// (candidate score, lane) order of the selection: valid first, larger score, then the lower (parent beam, rank) = lower lane
__device__ __forceinline__ bool sel_better(bool va, float a, int la, bool vb, float b, int lb) {
  return va && (!vb || a > b || (a == b && la < lb));
}

// one workgroup per image: wave w < K merges row (image, w)'s tile partials into its logsumexp and top-K; wave 0 selects
template <int K>
__global__ __launch_bounds__(512) void beam_select_kernel(const SelectArgs a) {
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
  if (w != 0) return;
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
  float my_s = 0.f; int my_t = 0, my_p = 0, my_fin = 0, my_len = 0;
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
  const int all_fin = __all(lane >= K || my_fin);
  if (lane < K) {
    const int r = img * K + lane;
    a.score[r] = my_s; a.fin[r] = my_fin; a.len[r] = my_len; a.tok[r] = my_t; a.par[r] = img * K + my_p;
    a.htok[(long)a.t * a.rows + r] = my_t;
    a.hpar[(long)a.t * a.rows + r] = my_p;
  }
  if (lane == 0) {
    a.last[img] = a.t;
    if (all_fin) { a.done[img] = 1; atomicAdd(a.count, 1); }      // (integer count: the later launches of the search return at once)
  }
}

// one workgroup per image: walk each beam's parent pointers back through the history, sort the K beams by score / length^alpha
// (descending, ties to the lower beam index), write ids [B, K, L] (pad after <E> and after the last step run), scores, lengths
__global__ __launch_bounds__(64) void beam_finalize_kernel(const float* __restrict__ score, const int* __restrict__ len, const int* __restrict__ htok,
                                                           const int* __restrict__ hpar, const int* __restrict__ last, int K, int L, int rows, int pad,
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
    const int r = img * K + tid;
    const float ns = score[r] / powf((float)len[r], alpha);
    int rank = 0;
    for (int i = 0; i < K; ++i) {
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

template <int K>
int select_launch(const SelectArgs& s, int B, hipStream_t stream) {
  hipLaunchKernelGGL((beam_select_kernel<K>), dim3(B), dim3(512), 0, stream, s);
  GIC_CHECK_LAUNCH("beam_select");
  return GIC_OK;
}
}  // namespace

int beam_select(const SelectArgs& s, int K, int B, hipStream_t stream) {
  switch (K) {
    case 1: return select_launch<1>(s, B, stream);
    case 2: return select_launch<2>(s, B, stream);
    case 3: return select_launch<3>(s, B, stream);
    case 4: return select_launch<4>(s, B, stream);
    case 5: return select_launch<5>(s, B, stream);
    case 6: return select_launch<6>(s, B, stream);
    case 7: return select_launch<7>(s, B, stream);
    default: return select_launch<8>(s, B, stream);
  }
}

int beam_init(const BeamLayerPtrs& slot0, int NL, int din0, int E, int H, int B, int K, int dtype, const float* features, const float* h0,
              const float* c0, const BeamState& s, hipStream_t stream, bool all_live) {
  const dim3 grid((unsigned)(B * K));
  if (dtype == DT_F32)
    hipLaunchKernelGGL((beam_init_kernel<float>), grid, dim3(256), 0, stream, slot0, NL, din0, E, H, B, K, features, h0, c0, s.score, s.fin,
                       s.len, s.tok, s.par, s.last, s.done, s.count, (int)all_live);
  else
    hipLaunchKernelGGL((beam_init_kernel<bf16_t>), grid, dim3(256), 0, stream, slot0, NL, din0, E, H, B, K, features, h0, c0, s.score, s.fin,
                       s.len, s.tok, s.par, s.last, s.done, s.count, (int)all_live);
  GIC_CHECK_LAUNCH("beam_init");
  return GIC_OK;
}

int beam_finalize(const BeamState& s, int B, int K, int L, int pad, float length_penalty, int64_t* ids, float* scores, int32_t* lengths,
                  int32_t* anc, hipStream_t stream) {
  const size_t lds = (size_t)2 * L * K * sizeof(int);
  static LdsGrant gfin;
  GIC_CHECK_ARG(grant_lds(beam_finalize_kernel, lds, gfin), "beam_finalize: cannot reserve %zu bytes of LDS", lds);
  hipLaunchKernelGGL(beam_finalize_kernel, dim3((unsigned)B), dim3(64), lds, stream, s.score, s.len, s.htok, s.hpar, s.last, K, L, B * K, pad,
                     length_penalty, ids, scores, lengths, anc);
  GIC_CHECK_LAUNCH("beam_finalize");
  return GIC_OK;
}

namespace {

template <int K>
int topk_launch(const float* logits, const BeamDims& d, float* pm, float* ps, float* pv, int* pi, const int* count, hipStream_t stream) {
  hipLaunchKernelGGL((beam_tile_topk_kernel<K>), dim3((unsigned)d.nblk, (unsigned)cdiv(d.rows, 64)), dim3(512), 0, stream, logits, d.rows, d.V,
                     d.nblk, pm, ps, pv, pi, count, d.B);
  GIC_CHECK_LAUNCH("beam_tile_topk");
  return GIC_OK;
}
int beam_tile_topk(const float* logits, const BeamDims& d, float* pm, float* ps, float* pv, int* pi, const int* count, hipStream_t stream) {
  switch (d.K) {
    case 1: return topk_launch<1>(logits, d, pm, ps, pv, pi, count, stream);
    case 2: return topk_launch<2>(logits, d, pm, ps, pv, pi, count, stream);
    case 3: return topk_launch<3>(logits, d, pm, ps, pv, pi, count, stream);
    case 4: return topk_launch<4>(logits, d, pm, ps, pv, pi, count, stream);
    case 5: return topk_launch<5>(logits, d, pm, ps, pv, pi, count, stream);
    case 6: return topk_launch<6>(logits, d, pm, ps, pv, pi, count, stream);
    case 7: return topk_launch<7>(logits, d, pm, ps, pv, pi, count, stream);
    default: return topk_launch<8>(logits, d, pm, ps, pv, pi, count, stream);
  }
}

template <typename TA>
int beam_search_t(const BeamDims& d, const gic_decoder_params* P, const gic_decoder_shadow* S, const gic_decoder_beam_opts* o, unsigned char* ws,
                  const float* features, int64_t* ids, float* scores, int32_t* lengths, hipStream_t stream) {
  const BeamLayout lay = beam_layout(d);
  const int R = d.rows, H = d.H, NL = d.NL;
  LayerPtrs slot[2];
  for (int l = 0; l < NL; ++l)
    for (int s = 0; s < 2; ++s) {
      slot[s].xh[l] = (TA*)(ws + lay.xh[l]) + (long)s * R * d.ldx(l);
      slot[s].c[l] = (float*)(ws + lay.c[l]) + (long)s * R * H;
    }
  float* pm = (float*)(ws + lay.pm); float* ps = (float*)(ws + lay.ps); float* pv = (float*)(ws + lay.pv); int* pi = (int*)(ws + lay.pi);
  float* score = (float*)(ws + lay.score);
  int* fin = (int*)(ws + lay.fin); int* len = (int*)(ws + lay.len); int* tok = (int*)(ws + lay.tok); int* par = (int*)(ws + lay.par);
  int* htok = (int*)(ws + lay.htok); int* hpar = (int*)(ws + lay.hpar);
  int* last = (int*)(ws + lay.last); int* done = (int*)(ws + lay.done); int* count = (int*)(ws + lay.count);

  const BeamState st{score, fin, len, tok, par, htok, hpar, last, done, count};
  GIC_PROPAGATE(beam_init(slot[0], NL, d.E, d.E, H, d.B, d.K, d.dt, features, o->h0, o->c0, st, stream));
  SelectArgs sa{pm, ps, pv, pi, score, fin, len, tok, par, htok, hpar, last, done, count, d.nblk, R, 0, o->eos_id, o->pad_id};
  for (int t = 0; t < d.L; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    if (d.fused) {
      for (int l = 0; l < NL; ++l) {
        LstmStepArgs a;
        a.xh_t = slot[cur].xh[l]; a.xh_next = slot[nxt].xh[l];
        a.wcat = S->wcat[l]; a.bsum = S->bsum[l];
        a.c_prev = slot[cur].c[l]; a.c_new = slot[nxt].c[l];
        if (l + 1 < NL) { a.h_up = slot[cur].xh[l + 1]; a.ld_up = d.ldx(l + 1); }
        a.B = R; a.H = H; a.din = d.din(l); a.ldx = d.ldx(l);
        a.stop = count; a.stop_at = d.B;
        if (t > 0) {
          a.parent = par;
          if (l == 0) { a.gather = 1; a.embed = P->embed; a.V = d.V; a.token = tok; }
        }
        GIC_PROPAGATE(lstm_step(a, d.dt, stream));
      }
      VocabStepArgs v;
      v.h = (const TA*)slot[nxt].xh[NL - 1] + d.din(NL - 1); v.ldh = d.ldx(NL - 1);
      v.wout = S->wout; v.bias = P->b_out;
      v.part_m = pm; v.part_s = ps; v.part_v = pv; v.part_i = pi; v.nblk = d.nblk;
      v.stop = count; v.stop_at = d.B;
      v.B = R; v.V = d.V; v.H = H;
      GIC_PROPAGATE(vocab_step_beam(v, d.K, d.dt, stream));
    } else {
      if (t > 0) {
        hipLaunchKernelGGL((beam_gather_kernel<TA>), dim3((unsigned)R), dim3(256), 0, stream, slot[0], slot[1], NL, d.E, H, P->embed, tok, par,
                           count, d.B);
        GIC_CHECK_LAUNCH("beam_gather");
      }
      float* gpre = (float*)(ws + lay.gpre);
      for (int l = 0; l < NL; ++l) {
        const long ld = d.ldx(l);
        GemmDesc g;
        g.A = slot[0].xh[l]; g.lda = ld; g.B = S->wcat[l]; g.ldb = ld; g.C = gpre; g.ldc = 4 * H;
        g.M = R; g.N = 4 * H; g.K = (int)ld; g.in_dtype = d.dt; g.out_dtype = DT_F32; g.bias = S->bsum[l];
        g.no_split = 1;                                    // no split-K atomics: a one-ulp reorder could flip a selection
        GIC_PROPAGATE(gemm(g, stream));
        GIC_PROPAGATE(lstm_pointwise_fwd(d.dt, gpre, slot[0].c[l], slot[1].c[l], (TA*)slot[1].xh[l] + d.din(l), ld,
                                         l + 1 < NL ? slot[0].xh[l + 1] : nullptr, l + 1 < NL ? d.ldx(l + 1) : 0, R, H, stream));
      }
      float* logits = (float*)(ws + lay.logits);
      GemmDesc g;
      g.A = (const TA*)slot[1].xh[NL - 1] + d.din(NL - 1); g.lda = d.ldx(NL - 1);
      g.B = S->wout; g.ldb = H; g.C = logits; g.ldc = d.V;
      g.M = R; g.N = d.V; g.K = H; g.in_dtype = d.dt; g.out_dtype = DT_F32; g.bias = P->b_out;
      g.no_split = 1;
      GIC_PROPAGATE(gemm(g, stream));
      GIC_PROPAGATE(beam_tile_topk(logits, d, pm, ps, pv, pi, count, stream));
    }
    sa.t = t;
    GIC_PROPAGATE(beam_select(sa, d.K, d.B, stream));
  }
  return beam_finalize(st, d.B, d.K, d.L, o->pad_id, o->length_penalty, ids, scores, lengths, nullptr, stream);
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_decoder_beam_ws_bytes(const gic_decoder_dims* dims, int32_t beam, uint64_t* out) {
  BeamDims d;
  GIC_PROPAGATE(beam_dims(dims, beam, d));
  GIC_CHECK_ARG(out, "decoder_beam_ws_bytes: null out");
  *out = (uint64_t)beam_layout(d).total;
  return GIC_OK;
}

int gic_decoder_beam_search(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S, const gic_decoder_beam_opts* o,
                            void* ws, const float* features, int64_t* ids, float* scores, int32_t* lengths, void* stream) {
  GIC_CHECK_ARG(o, "decoder_beam_search: null options");
  BeamDims d;
  GIC_PROPAGATE(beam_dims(dims, o->beam, d));
  GIC_CHECK_ARG(P && S && ws && features && ids && scores && lengths, "decoder_beam_search: null argument");
  GIC_CHECK_ARG(P->embed && P->b_out && S->wout, "decoder_beam_search: null embedding / output layer");
  for (int l = 0; l < d.NL; ++l) GIC_CHECK_ARG(S->wcat[l] && S->bsum[l], "decoder_beam_search: null layer %d weights", l);
  GIC_CHECK_ARG(o->eos_id >= 0 && o->eos_id < d.V, "decoder_beam_search: eos_id %d outside [0, %d)", o->eos_id, d.V);
  GIC_CHECK_ARG(o->pad_id >= 0 && o->pad_id < d.V, "decoder_beam_search: pad_id %d outside [0, %d)", o->pad_id, d.V);
  GIC_CHECK_ARG(o->length_penalty == o->length_penalty, "decoder_beam_search: length_penalty is NaN");
  GIC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "decoder_beam_search: the workspace must be 256-byte aligned");
  if (d.dt == DT_F32) return beam_search_t<float>(d, P, S, o, (unsigned char*)ws, features, ids, scores, lengths, (hipStream_t)stream);
  return beam_search_t<bf16_t>(d, P, S, o, (unsigned char*)ws, features, ids, scores, lengths, (hipStream_t)stream);
}

}  // extern "C"
