// Beam-search caption decode for the visual-attention decoder (gicap.h gic_attn_beam_search): the search of beam.h with the step of
// attention.hip.  Rows = B * k (row r = image r / k, beam r % k).  One step:
//   hp GEMM          hp [rows, A] = h W_h^T over the rows of the current slot, before the reorder (the library GEMM, never split over K)
//   attn_beam_energy e[r, i] = w_a . tanh(fp_i + hp[parent[r]]): workgroup = (image, 8 positions); each fp piece it loads feeds the k beams
//   attn_beam_ctx    alpha = softmax_i e[r, :], z_r = sum_i alpha_ri a_i: workgroup = (image, 32 channel pieces); every workgroup of an image
//                    forms the same softmax of its k rows, 8 position groups each sum a share of the positions for the k beams, and
//                    the 8 partial sums meet in LDS in group order.  z goes to row r's z columns of the slot, alpha to the history.
//   lstm_step        the BEAM form of the LSTM decoder's search: x = embed[token[r]] into [0, E), z from row r, h / c from row parent[r]
//   vocab_step_beam, beam_select      unchanged
// fp = fmap W_f^T + b_f is formed once per search (B * P rows), and beam_finalize's ancestor rows pick the alpha rows of the returned
// beams out of the history (one gather launch).  The image data (fp and fmap) is read once per image and step whatever k is.  No f32
// atomics: each energy, alpha and z value is written by one thread, the partial sums are added in a fixed order, and neither GEMM splits K.
//
// Scratch (one caller-owned workspace, gic_attn_beam_ws_bytes; every region 256-byte aligned):
//   xh act [2][rows][E + C + H] (slots t % 2 / (t + 1) % 2: [x_t | z_t | h_{t-1}] / h_t), c f32 [2][rows][H], fproj act [B][P][A],
//   hp f32 [rows][A], e f32 [rows][P], alpha history f32 [L][rows][P], the tile partials, search state and history of beam.hip,
//   anc i32 [B][k][L]
#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {
namespace {

constexpr int kEnergyPos = 8;                    // positions per attn_beam_energy workgroup (2 per wave)
constexpr int kCtxPieces = 32;                   // 16-byte channel pieces per attn_beam_ctx workgroup
constexpr int kCtxGroups = 256 / kCtxPieces;     // its position groups

struct AttnBeamDims {
  ACtx c;
  int K, rows, nblk;
};

struct AttnBeamLayout {
  size_t xh, c, fproj, hp, e, ahist, pm, ps, pv, pi, score, fin, len, tok, par, htok, hpar, anc, last, done, count, total;
};

AttnBeamLayout attn_beam_layout(const AttnBeamDims& d) {
  AttnBeamLayout o{};
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t p = at; at += (bytes + 255) & ~(size_t)255; return p; };
  const ACtx& c = d.c;
  const size_t R = d.rows, pn = (size_t)d.rows * d.nblk;
  o.xh = take(2 * R * c.ldx() * c.asz());
  o.c = take(2 * R * c.H * 4);
  o.fproj = take((size_t)c.B * c.P * c.A * c.asz());
  o.hp = take(R * c.A * 4);
  o.e = take(R * c.P * 4);
  o.ahist = take((size_t)c.L * R * c.P * 4);
  o.pm = take(pn * 4); o.ps = take(pn * 4);
  o.pv = take(pn * d.K * 4); o.pi = take(pn * d.K * 4);
  o.score = take(R * 4); o.fin = take(R * 4); o.len = take(R * 4); o.tok = take(R * 4); o.par = take(R * 4);
  o.htok = take((size_t)c.L * R * 4); o.hpar = take((size_t)c.L * R * 4);
  o.anc = take((size_t)c.L * R * 4);
  o.last = take((size_t)c.B * 4); o.done = take((size_t)c.B * 4); o.count = take(4);
  o.total = at;
  return o;
}

int attn_beam_dims(const gic_attn_dims* dims, int K, AttnBeamDims& d) {
  GIC_PROPAGATE(check_attn_dims(dims, d.c));
  GIC_CHECK_ARG(K >= 1 && K <= kBeamMax, "attn_beam: beam size must be 1..%d, got %d", kBeamMax, K);
  GIC_CHECK_ARG(K <= d.c.V, "attn_beam: beam size %d exceeds the vocabulary (%d)", K, d.c.V);
  GIC_CHECK_ARG(d.c.L <= 1024, "attn_beam: at most 1024 steps");
  GIC_CHECK_ARG((long)d.c.B * K <= (1l << 24), "attn_beam: too many rows");
  d.K = K;
  d.rows = d.c.B * K;
  d.nblk = cdiv(d.c.V, kBeamTile);
  return GIC_OK;
}


// e[r, i] for the k rows of image blockIdx.x and positions blockIdx.y * 8 .. + 7: wave w takes positions w and w + 4, a lane the 16-byte
// pieces lane, lane + 64, ... of a position's fp row; the k parents' hp rows are staged in LDS
template <typename TA, int K>
__global__ __launch_bounds__(256) void attn_beam_energy_kernel(const AttnBeamArgs a) {
  constexpr int NV = Vec16<TA>::NV;
  constexpr int kPW = kEnergyPos / 4;
  extern __shared__ float hp_s[];                          // [K][A]
  if (*a.stop >= a.stop_at) return;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int r = 0; r < K; ++r) {
    const float* src = a.hp + (long)a.par[img * K + r] * a.A;
    for (int j = tid; j < a.A; j += 256) hp_s[r * a.A + j] = src[j];
  }
  __syncthreads();
  const TA* fp = (const TA*)a.fproj + (long)img * a.P * a.A;
  const int i0 = blockIdx.y * kEnergyPos + w;
  float s[kPW][K];
#pragma unroll
  for (int u = 0; u < kPW; ++u)
#pragma unroll
    for (int r = 0; r < K; ++r) s[u][r] = 0.f;
  for (int j0 = lane * NV; j0 < a.A; j0 += 64 * NV) {
    float v[kPW][NV];
#pragma unroll
    for (int u = 0; u < kPW; ++u) {                         // unconditional loads (a position past P re-reads the last one)
      const int i = min(i0 + 4 * u, a.P - 1);
      Vec16<TA>::load(fp + (long)i * a.A + j0, v[u]);
    }
    float wa[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) wa[q] = a.w_a[j0 + q];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      float hp[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) hp[q] = hp_s[r * a.A + j0 + q];
#pragma unroll
      for (int u = 0; u < kPW; ++u)
#pragma unroll
        for (int q = 0; q < NV; ++q) s[u][r] += wa[q] * tanhf(v[u][q] + hp[q]);
    }
  }
#pragma unroll
  for (int u = 0; u < kPW; ++u) {
    const int i = i0 + 4 * u;
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const float t = wave_sum(s[u][r]);
      if (lane == 0 && i < a.P) a.e[(long)(img * K + r) * a.P + i] = t;
    }
  }
}

// z of the k rows of image blockIdx.x for the channel pieces blockIdx.y * 32 .. + 31 (LDS: alpha [K][P], then the partials
// [kCtxGroups][kCtxPieces * NV])
template <typename TA, int K>
__global__ __launch_bounds__(256) void attn_beam_ctx_kernel(const AttnBeamArgs a) {
  constexpr int NV = Vec16<TA>::NV;
  constexpr int W = kCtxPieces * NV;                       // channels per workgroup
  constexpr int kZ = K <= 4 ? 8 : 4;                       // positions in flight per thread
  extern __shared__ float ctx_s[];
  float* al_s = ctx_s;
  float* part_s = ctx_s + ((K * a.P + 3) & ~3);
  if (*a.stop >= a.stop_at) return;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // alpha = softmax over the P positions, row r by wave r % 4 (the same bits in every workgroup of the image)
  for (int r = w; r < K; r += 4) {
    const float* er = a.e + (long)(img * K + r) * a.P;
    float m = -INFINITY;
    for (int i = lane; i < a.P; i += 64) m = fmaxf(m, er[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < a.P; i += 64) {
      const float x = expf(er[i] - m);
      al_s[r * a.P + i] = x;
      s += x;
    }
    s = wave_sum(s);
    float* hist = a.alpha && blockIdx.y == 0 ? a.alpha + (long)(img * K + r) * a.P : nullptr;
    for (int i = lane; i < a.P; i += 64) {
      const float al = al_s[r * a.P + i] / s;
      al_s[r * a.P + i] = al;
      if (hist) hist[i] = al;
    }
  }
  __syncthreads();
  // thread = (position group g, channel piece p): group g sums the positions g, g + 8, ... for all K rows
  const int p = tid % kCtxPieces, g = tid / kCtxPieces;
  const int c0 = (blockIdx.y * kCtxPieces + p) * NV;
  const TA* fm = (const TA*)a.fmap + (long)img * a.P * a.C + (c0 < a.C ? c0 : 0);
  float acc[K][NV];
#pragma unroll
  for (int r = 0; r < K; ++r)
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[r][q] = 0.f;
  for (int i0 = g; i0 < a.P; i0 += kCtxGroups * kZ) {
    float v[kZ][NV];
#pragma unroll
    for (int u = 0; u < kZ; ++u) {                          // unconditional loads (a position past P re-reads the group's first)
      const int i = i0 + u * kCtxGroups;
      Vec16<TA>::load(fm + (long)(i < a.P ? i : i0) * a.C, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kZ; ++u) {
      const int i = i0 + u * kCtxGroups;
#pragma unroll
      for (int r = 0; r < K; ++r) {
        const float al = i < a.P ? al_s[r * a.P + i] : 0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[r][q] += al * v[u][q];
      }
    }
  }
  // the groups' partial sums, one row at a time, added in group order by the thread that owns the channel
#pragma unroll
  for (int r = 0; r < K; ++r) {
#pragma unroll
    for (int q = 0; q < NV; ++q) part_s[g * W + p * NV + q] = acc[r][q];
    __syncthreads();
    const int cl = blockIdx.y * W + tid;
    if (tid < W && cl < a.C) {
      float z = part_s[tid];
#pragma unroll
      for (int gg = 1; gg < kCtxGroups; ++gg) z += part_s[gg * W + tid];
      ((TA*)a.z)[(long)(img * K + r) * a.ldx + cl] = from_f32<TA>(z);
    }
    __syncthreads();
  }
}

// alphas[b, j, t, :] = the history row anc[b, j, t] of step t for t < lengths[b, j], else 0: one workgroup per (returned beam, step)
__global__ __launch_bounds__(64) void attn_beam_alphas_kernel(const float* __restrict__ ahist, const int* __restrict__ anc,
                                                              const int* __restrict__ lengths, int rows, int L, int P, float* __restrict__ alphas) {
  const long br = blockIdx.x;                              // image * K + rank
  const int t = blockIdx.y, tid = threadIdx.x;
  const int row = t < lengths[br] ? anc[br * L + t] : -1;
  float* dst = alphas + (br * L + t) * P;
  if (row < 0) {
    for (int i = tid; i < P; i += 64) dst[i] = 0.f;
    return;
  }
  const float* src = ahist + ((long)t * rows + row) * P;
  for (int i = tid; i < P; i += 64) dst[i] = src[i];
}

template <typename TA, int K>
int attn_beam_step_launch(const AttnBeamArgs& f, int B, hipStream_t stream) {
  constexpr int NV = Vec16<TA>::NV;
  const size_t lds_e = (size_t)K * f.A * sizeof(float);
  const size_t lds_c = (size_t)(((K * f.P + 3) & ~3) + kCtxGroups * kCtxPieces * NV) * sizeof(float);
  static LdsGrant ge, gc;
  GIC_CHECK_ARG(grant_lds(attn_beam_energy_kernel<TA, K>, lds_e, ge), "attn_beam_energy: cannot reserve %zu bytes of LDS", lds_e);
  GIC_CHECK_ARG(grant_lds(attn_beam_ctx_kernel<TA, K>, lds_c, gc), "attn_beam_ctx: cannot reserve %zu bytes of LDS", lds_c);
  hipLaunchKernelGGL((attn_beam_energy_kernel<TA, K>), dim3((unsigned)B, (unsigned)cdiv(f.P, kEnergyPos)), dim3(256), lds_e, stream, f);
  GIC_CHECK_LAUNCH("attn_beam_energy");
  hipLaunchKernelGGL((attn_beam_ctx_kernel<TA, K>), dim3((unsigned)B, (unsigned)cdiv(f.C, kCtxPieces * NV)), dim3(256), lds_c, stream, f);
  GIC_CHECK_LAUNCH("attn_beam_ctx");
  return GIC_OK;
}

template <typename TA>
int attn_beam_step_t(const AttnBeamArgs& f, int K, int B, hipStream_t stream) {
  switch (K) {
    case 1: return attn_beam_step_launch<TA, 1>(f, B, stream);
    case 2: return attn_beam_step_launch<TA, 2>(f, B, stream);
    case 3: return attn_beam_step_launch<TA, 3>(f, B, stream);
    case 4: return attn_beam_step_launch<TA, 4>(f, B, stream);
    case 5: return attn_beam_step_launch<TA, 5>(f, B, stream);
    case 6: return attn_beam_step_launch<TA, 6>(f, B, stream);
    case 7: return attn_beam_step_launch<TA, 7>(f, B, stream);
    default: return attn_beam_step_launch<TA, 8>(f, B, stream);
  }
}

template <typename TA>
int attn_beam_t(const AttnBeamDims& d, const gic_attn_params* P, const gic_attn_shadow* S, const gic_decoder_beam_opts* o, unsigned char* ws,
                const float* features, const void* fmap, int64_t* ids, float* scores, int32_t* lengths, float* alphas, hipStream_t stream) {
  const AttnBeamLayout lay = attn_beam_layout(d);
  const ACtx& c = d.c;
  const int R = d.rows, H = c.H, B = c.B;
  const long ldx = c.ldx();
  BeamLayerPtrs slot[2] = {};
  for (int s = 0; s < 2; ++s) {
    slot[s].xh[0] = (TA*)(ws + lay.xh) + (long)s * R * ldx;
    slot[s].c[0] = (float*)(ws + lay.c) + (long)s * R * H;
  }
  float* pm = (float*)(ws + lay.pm); float* ps = (float*)(ws + lay.ps); float* pv = (float*)(ws + lay.pv); int* pi = (int*)(ws + lay.pi);
  const BeamState st{(float*)(ws + lay.score), (int*)(ws + lay.fin), (int*)(ws + lay.len), (int*)(ws + lay.tok), (int*)(ws + lay.par),
                     (int*)(ws + lay.htok), (int*)(ws + lay.hpar), (int*)(ws + lay.last), (int*)(ws + lay.done), (int*)(ws + lay.count)};
  void* fproj = ws + lay.fproj;
  float* hp = (float*)(ws + lay.hp);
  float* ahist = (float*)(ws + lay.ahist);
  int32_t* anc = (int32_t*)(ws + lay.anc);

  GIC_PROPAGATE(beam_init(slot[0], 1, c.din(), c.E, H, B, d.K, c.dt, features, o->h0, o->c0, st, stream));
  {  // fp = fmap W_f^T + b_f, once per image
    GemmDesc g;
    g.A = fmap; g.lda = c.C; g.B = S->wf; g.ldb = c.C; g.C = fproj; g.ldc = c.A;
    g.M = B * c.P; g.N = c.A; g.K = c.C; g.in_dtype = c.dt; g.out_dtype = c.dt; g.bias = P->b_f;
    g.no_split = 1;
    GIC_PROPAGATE(gemm(g, stream));
  }
  BeamSelectArgs sa{pm, ps, pv, pi, st.score, st.fin, st.len, st.tok, st.par, st.htok, st.hpar, st.last, st.done, st.count, d.nblk, R, 0,
                    o->eos_id, o->pad_id};
  for (int t = 0; t < c.L; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    TA* xh_t = (TA*)slot[cur].xh[0];
    {  // hp [rows, A] = h_{t-1} W_h^T, the rows as the previous step left them (the attention kernels read row parent[r])
      GemmDesc g;
      g.A = xh_t + c.din(); g.lda = ldx; g.B = S->wh; g.ldb = H; g.C = hp; g.ldc = c.A;
      g.M = R; g.N = c.A; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32;
      g.no_split = 1;                                      // no split-K atomics: a one-ulp reorder could flip a selection
      GIC_PROPAGATE(gemm(g, stream));
    }
    AttnBeamArgs f;
    f.fproj = fproj; f.fmap = fmap; f.w_a = P->w_a; f.hp = hp; f.par = st.par; f.e = (float*)(ws + lay.e);
    f.z = xh_t + c.E; f.ldx = ldx; f.alpha = alphas ? ahist + (long)t * R * c.P : nullptr;
    f.stop = st.count; f.stop_at = B;
    f.P = c.P; f.A = c.A; f.C = c.C;
    GIC_PROPAGATE(attn_beam_step_t<TA>(f, d.K, B, stream));
    LstmStepArgs a;
    a.xh_t = xh_t; a.xh_next = slot[nxt].xh[0]; a.wcat = S->wcat; a.bsum = S->bsum;
    a.c_prev = slot[cur].c[0]; a.c_new = slot[nxt].c[0];
    a.B = R; a.H = H; a.din = c.din(); a.ldx = ldx; a.gw = c.E;
    a.stop = st.count; a.stop_at = B;
    if (t > 0) { a.parent = st.par; a.gather = 1; a.embed = P->embed; a.V = c.V; a.token = st.tok; }
    GIC_PROPAGATE(lstm_step(a, c.dt, stream));
    VocabStepArgs v;
    v.h = (const TA*)slot[nxt].xh[0] + c.din(); v.ldh = ldx;
    v.wout = S->wout; v.bias = P->b_out;
    v.part_m = pm; v.part_s = ps; v.part_v = pv; v.part_i = pi; v.nblk = d.nblk;
    v.stop = st.count; v.stop_at = B;
    v.B = R; v.V = c.V; v.H = H;
    GIC_PROPAGATE(vocab_step_beam(v, d.K, c.dt, stream));
    sa.t = t;
    GIC_PROPAGATE(beam_select(sa, d.K, B, stream));
  }
  GIC_PROPAGATE(beam_finalize(st, B, d.K, c.L, o->pad_id, o->length_penalty, ids, scores, lengths, alphas ? anc : nullptr, stream));
  if (alphas) {
    hipLaunchKernelGGL(attn_beam_alphas_kernel, dim3((unsigned)R, (unsigned)c.L), dim3(64), 0, stream, ahist, anc, lengths, R, c.L, c.P, alphas);
    GIC_CHECK_LAUNCH("attn_beam_alphas");
  }
  return GIC_OK;
}

}  // namespace

int attn_beam_step(const AttnBeamArgs& f, int K, int B, int dtype, hipStream_t stream) {
  GIC_CHECK_ARG(K >= 1 && K <= kBeamMax, "attn_beam_step: K must be 1..%d", kBeamMax);
  return dtype == DT_F32 ? attn_beam_step_t<float>(f, K, B, stream) : attn_beam_step_t<bf16_t>(f, K, B, stream);
}

}  // namespace gic

using namespace gic;

extern "C" {

int gic_attn_beam_ws_bytes(const gic_attn_dims* dims, int32_t beam, uint64_t* out) {
  AttnBeamDims d;
  GIC_PROPAGATE(attn_beam_dims(dims, beam, d));
  GIC_CHECK_ARG(out, "attn_beam_ws_bytes: null out");
  *out = (uint64_t)attn_beam_layout(d).total;
  return GIC_OK;
}

int gic_attn_beam_search(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_decoder_beam_opts* o, void* ws,
                         const float* features, const void* fmap, int64_t* ids, float* scores, int32_t* lengths, float* alphas, void* stream) {
  GIC_CHECK_ARG(o, "attn_beam_search: null options");
  AttnBeamDims d;
  GIC_PROPAGATE(attn_beam_dims(dims, o->beam, d));
  GIC_CHECK_ARG(P && S && ws && features && fmap && ids && scores && lengths, "attn_beam_search: null argument");
  GIC_CHECK_ARG(P->embed && P->b_out && P->b_f && P->w_a && S->wcat && S->bsum && S->wout && S->wf && S->wh, "attn_beam_search: null weights");
  GIC_CHECK_ARG(o->eos_id >= 0 && o->eos_id < d.c.V, "attn_beam_search: eos_id %d outside [0, %d)", o->eos_id, d.c.V);
  GIC_CHECK_ARG(o->pad_id >= 0 && o->pad_id < d.c.V, "attn_beam_search: pad_id %d outside [0, %d)", o->pad_id, d.c.V);
  GIC_CHECK_ARG(o->length_penalty == o->length_penalty, "attn_beam_search: length_penalty is NaN");
  GIC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "attn_beam_search: the workspace must be 256-byte aligned");
  if (d.c.dt == DT_F32)
    return attn_beam_t<float>(d, P, S, o, (unsigned char*)ws, features, fmap, ids, scores, lengths, alphas, (hipStream_t)stream);
  return attn_beam_t<bf16_t>(d, P, S, o, (unsigned char*)ws, features, fmap, ids, scores, lengths, alphas, (hipStream_t)stream);
}

}  // extern "C"
