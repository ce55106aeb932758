// The attention kernels of a caption decode step (beam.h attn_step): the split attention step of every decode but the training
// roll-out's (attention.hip).  decode.hip's step loop drives them for gic_attn_beam_search, gic_attn_diverse_beam_search and
// gic_attn_sample_captions, teacher_forced.hip's AttnTf recurrence for gic_attn_forward_tf.  Rows = B * k (row r = image r / k, beam r % k).  One step:
//   hp GEMM          hp [rows, A] = h W_h^T over the rows of the current slot, before the reorder (the library GEMM, never split over K)
//   attn_step_energy e[r, i] = w_a . tanh(fp_i + hp[parent[r]]): workgroup = (image, 8 positions); each fp piece it loads feeds the k beams
//   attn_step_ctx    alpha = softmax_i e[r, :], z_r = sum_i alpha_ri a_i: workgroup = (image, 32 channel pieces); every workgroup of an image
//                    forms the same softmax of its k rows, 8 position groups each sum a share of the positions for the k beams, and
//                    the 8 partial sums meet in LDS in group order.  z goes to row r's z columns of the slot, alpha to the history.
//   lstm_step        the BEAM form of the LSTM decoder's search: x = embed[token[r]] into [0, E), z from row r, h / c from row parent[r]
//   vocab_step_beam, beam_select      unchanged
// fp = fmap W_f^T + b_f is formed once per search (B * P rows), and beam_finalize's ancestor rows pick the alpha rows of the returned
// beams out of the history (one gather launch).  The image data (fp and fmap) is read once per image and step whatever k is.  No f32
// atomics: each energy, alpha and z value is written by one thread, the partial sums are added in a fixed order, and neither GEMM splits K.
// The packed form (PACK, k = 1; teacher forcing) gates each caption by its length instead of the finished count: a caption past its
// length leaves both kernels at once and gets a zero alpha row.  Its parents are the identity, and the alpha row also goes to the
// caller's alphas when given.
#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {
namespace {

constexpr int kEnergyPos = 8;                    // positions per attn_step_energy workgroup (2 per wave)
constexpr int kCtxPieces = 32;                   // 16-byte channel pieces per attn_step_ctx workgroup
constexpr int kCtxGroups = 256 / kCtxPieces;     // its position groups

// e[r, i] for the k rows of image blockIdx.x and positions blockIdx.y * 8 .. + 7: wave w takes positions w and w + 4, a lane the 16-byte
// pieces lane, lane + 64, ... of a position's fp row; the k parents' hp rows are staged in LDS (the packed form reads its own row from
// global memory: staging one row before the fp loads cost 0.5 us per step)
template <typename TA, int K, bool PACK>
__global__ __launch_bounds__(256) void attn_step_energy_kernel(const AttnStepArgs a) {
  constexpr int NV = Vec16<TA>::NV;
  constexpr int kPW = kEnergyPos / 4;
  extern __shared__ float hp_s[];                          // [K][A]
  if (!PACK && *a.stop >= a.stop_at) return;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (PACK && a.t >= a.lengths[img]) return;
  if (!PACK) {
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const float* src = a.hp + (long)a.par[img * K + r] * a.A;
      for (int j = tid; j < a.A; j += 256) hp_s[r * a.A + j] = src[j];
    }
    __syncthreads();
  }
  const float* hp_rows = PACK ? a.hp + (long)img * a.A : hp_s;
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
      for (int q = 0; q < NV; ++q) hp[q] = hp_rows[r * a.A + j0 + q];
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
template <typename TA, int K, bool PACK>
__global__ __launch_bounds__(256) void attn_step_ctx_kernel(const AttnStepArgs a) {
  constexpr int NV = Vec16<TA>::NV;
  constexpr int W = kCtxPieces * NV;                       // channels per workgroup
  constexpr int kZ = K <= 4 ? 8 : 4;                       // positions in flight per thread
  extern __shared__ float ctx_s[];
  float* al_s = ctx_s;
  float* part_s = ctx_s + ((K * a.P + 3) & ~3);
  if (!PACK && *a.stop >= a.stop_at) return;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float* alphas = PACK && a.alphas && blockIdx.y == 0 ? a.alphas + (long)img * a.alphas_ld : nullptr;
  if (PACK && a.t >= a.lengths[img]) {                    // past the caption's length: a zero alpha row, z stays zero
    if (blockIdx.y == 0)
      for (int i = tid; i < a.P; i += 256) {
        a.alpha[(long)img * a.P + i] = 0.f;
        if (alphas) alphas[i] = 0.f;
      }
    return;
  }
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
      if (alphas) alphas[i] = al;
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

template <typename TA, int K, bool PACK>
int attn_step_t(const AttnStepArgs& f, int B, hipStream_t stream) {
  constexpr int NV = Vec16<TA>::NV;
  const size_t lds_e = (size_t)K * f.A * sizeof(float);
  const size_t lds_c = (size_t)(((K * f.P + 3) & ~3) + kCtxGroups * kCtxPieces * NV) * sizeof(float);
  static LdsGrant ge, gc;
  GIC_CHECK_ARG(grant_lds(attn_step_energy_kernel<TA, K, PACK>, lds_e, ge), "attn_step_energy: cannot reserve %zu bytes of LDS", lds_e);
  GIC_CHECK_ARG(grant_lds(attn_step_ctx_kernel<TA, K, PACK>, lds_c, gc), "attn_step_ctx: cannot reserve %zu bytes of LDS", lds_c);
  hipLaunchKernelGGL((attn_step_energy_kernel<TA, K, PACK>), dim3((unsigned)B, (unsigned)cdiv(f.P, kEnergyPos)), dim3(256), lds_e, stream, f);
  GIC_CHECK_LAUNCH("attn_step_energy");
  hipLaunchKernelGGL((attn_step_ctx_kernel<TA, K, PACK>), dim3((unsigned)B, (unsigned)cdiv(f.C, kCtxPieces * NV)), dim3(256), lds_c, stream, f);
  GIC_CHECK_LAUNCH("attn_step_ctx");
  return GIC_OK;
}

}  // namespace

int attn_step(const AttnStepArgs& f, int K, int B, int dtype, hipStream_t stream) {
  GIC_CHECK_ARG(K >= 1 && K <= kBeamMax, "attn_step: K must be 1..%d", kBeamMax);
  GIC_CHECK_ARG(!f.lengths || K == 1, "attn_step: the packed form takes K = 1");
  const bool f32 = dtype == DT_F32;
  if (f.lengths) return f32 ? attn_step_t<float, 1, true>(f, B, stream) : attn_step_t<bf16_t, 1, true>(f, B, stream);
  return with_beam_k(K, [&](auto k) -> int {
    return f32 ? attn_step_t<float, k, false>(f, B, stream) : attn_step_t<bf16_t, k, false>(f, B, stream);
  });
}

int attn_beam_alphas(const float* ahist, const int* anc, const int* lengths, int rows, int L, int P, float* alphas, hipStream_t stream) {
  hipLaunchKernelGGL(attn_beam_alphas_kernel, dim3((unsigned)rows, (unsigned)L), dim3(64), 0, stream, ahist, anc, lengths, rows, L, P, alphas);
  GIC_CHECK_LAUNCH("attn_beam_alphas");
  return GIC_OK;
}

}  // namespace gic
