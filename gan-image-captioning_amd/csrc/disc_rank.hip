// Inference uses of the discriminator (no reference counterpart): re-ranking G's K candidates per image with D's score, and image-caption
// retrieval ranks of the conditioned D.  The grouped match term they rest on is disc_cond.hip's forward kernel (gic_disc_match_fwd_grouped).
//
//   gic_rerank         d[b,k] = (1/R) sum_r d_logits[(b K + k) R + r]  (r in index order);  final = lm / max(len,1)^lp + weight d;
//                      order[b,:] = the beams by final descending, ties to the lower input index, NaN last; every output gathered.
//   gic_disc_rep_mean  ybar[c,:F] = (1/R) sum_r ydrop[c R + r, :F], lbar[c] = (1/R) sum_r logits[c R + r]  (r in index order)
//   gic_match_ranks    T[c,j] = S[c,j] + row_bias[c];  rank_c2i[c] = #{j != c : !(T[c,j] < T[c,c])},  rank_i2c[j] = #{c != j : !(T[c,j] < T[j,j])}
// No f32 atomics anywhere: the counts of gic_match_ranks are integers (order-free), so all three give the same bits in either mode.
#include "../../include/gicap.h"
#include "kernels.h"

namespace gic {
namespace {

constexpr int RERANK_MAX_K = 64;

// ---- re-rank.  One workgroup (256 threads) per image.  Thread k < K forms d and final of beam k and counts the beams that precede it
// (rank by counting: K <= 64, no sort network); then the whole workgroup gathers the rows into the new order.
__global__ __launch_bounds__(256) void rerank_kernel(const float* __restrict__ lm, const int32_t* __restrict__ lengths, float length_penalty,
                                                       const float* __restrict__ d_logits, int R, float weight, const int64_t* __restrict__ ids,
                                                       const float* __restrict__ alphas, int K, int L, int P, int32_t* __restrict__ order,
                                                       float* __restrict__ final_scores, float* __restrict__ d_scores, int64_t* __restrict__ out_ids,
                                                       float* __restrict__ out_lm, int32_t* __restrict__ out_lengths, float* __restrict__ out_alphas) {
  __shared__ float fin[RERANK_MAX_K], dsc[RERANK_MAX_K];
  __shared__ int ord[RERANK_MAX_K];
  const int b = blockIdx.x, t = threadIdx.x;
  const long bk = (long)b * K;
  if (t < K) {
    const float* g = d_logits + (bk + t) * R;
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += g[r];
    const float d = s / (float)R;
    const int len = lengths[bk + t] > 1 ? lengths[bk + t] : 1;
    const float term = lm[bk + t] / powf((float)len, length_penalty);
    dsc[t] = d;
    ord[t] = t;
    fin[t] = weight == 0.f ? term : term + weight * d;           // weight 0: G's own order, whatever D says (a NaN logit included)
  }
  __syncthreads();
  if (t < K) {
    const float f = fin[t];
    const bool fn = f != f;
    int before = 0;
    for (int j = 0; j < K; ++j) {
      const float o = fin[j];
      const bool on = o != o;
      const bool first = on ? (fn && j < t) : (fn || o > f || (o == f && j < t));
      before += first ? 1 : 0;
    }
    ord[before] = t;                                              // a strict total order: the ranks are a permutation of 0 .. K-1
  }
  __syncthreads();
  if (t < K) {
    const int src = ord[t];
    order[bk + t] = src;
    final_scores[bk + t] = fin[src];
    d_scores[bk + t] = dsc[src];
    if (out_lm) out_lm[bk + t] = lm[bk + src];
    if (out_lengths) out_lengths[bk + t] = lengths[bk + src];
  }
  if (out_ids)
    for (int i = t; i < K * L; i += 256) out_ids[bk * L + i] = ids[(bk + ord[i / L]) * L + i % L];
  if (out_alphas) {
    const long row = (long)L * P;
    for (long i = t; i < K * row; i += 256) out_alphas[bk * row + i] = alphas[(bk + ord[i / row]) * row + i % row];
  }
}

// ---- mean over the representations.  One thread per (caption, 4 columns) walks the caption's R rows in index order (the layout of
// disc_match_bwd_kernel); thread 0 of a caption's first workgroup sums its R base logits.  grid = (column groups / 64, captions).
template <typename TA>
__global__ __launch_bounds__(64) void disc_rep_mean_kernel(const TA* __restrict__ y, const float* __restrict__ logits, float* __restrict__ ybar,
                                                             float* __restrict__ lbar, int R, int F, int Fp) {
  const int b = blockIdx.y;
  const long m0 = (long)b * R;
  if (blockIdx.x == 0 && threadIdx.x == 0 && lbar) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += logits[m0 + r];
    lbar[b] = s / (float)R;
  }
  const int n0 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (n0 >= F) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int r = 0; r < R; ++r) {
    const long o = (m0 + r) * Fp + n0;
    __attribute__((aligned(16))) TA v[4];
    if (sizeof(TA) == 4) *(float4*)v = *(const float4*)(y + o);
    else *(float2*)v = *(const float2*)(y + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += to_f32<TA>(v[e]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n0 + e < F) ybar[(long)b * F + n0 + e] = acc[e] / (float)R;
}

// ---- retrieval ranks.  grid = (column tiles of 256, row chunks of RANK_ROWS).  A thread owns column j and walks the chunk's rows: every
// load is a wave's 256 contiguous bytes of one row of S (no strided column walk).  Row counts: a ballot per wave, one integer atomic per
// (row, wave); column counts: a register per thread, one integer atomic per (column, row chunk).  The diagonal comes from the same S.
constexpr int RANK_ROWS = 32;
__global__ __launch_bounds__(256) void match_ranks_kernel(const float* __restrict__ S, long ld, const float* __restrict__ bias, int N,
                                                            int32_t* __restrict__ rank_c2i, int32_t* __restrict__ rank_i2c) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const bool live = j < N;
  const int c0 = blockIdx.y * RANK_ROWS;
  const int c1 = c0 + RANK_ROWS < N ? c0 + RANK_ROWS : N;
  const float tjj = live ? S[(long)j * ld + j] + (bias ? bias[j] : 0.f) : 0.f;
  int col = 0;
  for (int c = c0; c < c1; ++c) {                                 // workgroup-uniform
    const float bc = bias ? bias[c] : 0.f;
    const float tcc = S[(long)c * ld + c] + bc;
    const float tcj = live ? S[(long)c * ld + j] + bc : 0.f;
    const bool other = live && j != c;
    const bool row_hit = other && !(tcj < tcc);                   // a tie or a NaN counts against the true pair
    col += other && !(tcj < tjj) ? 1 : 0;
    const int n = __popcll(__ballot(row_hit));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(rank_c2i + c, n);
  }
  if (live && col) atomicAdd(rank_i2c + j, col);
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_rerank(const float* lm_scores, const int32_t* lengths, float length_penalty, const float* d_logits, int32_t R, float weight,
               const int64_t* ids, const float* alphas, int32_t B, int32_t K, int32_t L, int32_t P, int32_t* order, float* final_scores,
               float* d_scores, int64_t* out_ids, float* out_lm_scores, int32_t* out_lengths, float* out_alphas, void* stream) {
  GIC_CHECK_ARG(lm_scores, "rerank: null lm_scores");
  GIC_CHECK_ARG(lengths, "rerank: null lengths");
  GIC_CHECK_ARG(d_logits, "rerank: null d_logits");
  GIC_CHECK_ARG(order && final_scores && d_scores, "rerank: null order / final_scores / d_scores");
  GIC_CHECK_ARG(B >= 1, "rerank: B=%d must be >= 1", B);
  GIC_CHECK_ARG(K >= 1 && K <= RERANK_MAX_K, "rerank: K=%d must be in 1..%d", K, RERANK_MAX_K);
  GIC_CHECK_ARG(R >= 1, "rerank: R=%d must be >= 1", R);
  GIC_CHECK_ARG(L >= 0 && P >= 0, "rerank: L=%d and P=%d must be >= 0", L, P);
  GIC_CHECK_ARG(length_penalty == length_penalty && weight == weight, "rerank: length_penalty or weight is NaN");
  GIC_CHECK_ARG(!out_ids || (ids && L >= 1), "rerank: out_ids needs ids and L >= 1");
  GIC_CHECK_ARG(!out_alphas || (alphas && L >= 1 && P >= 1), "rerank: out_alphas needs alphas, L >= 1 and P >= 1");
  const size_t n = (size_t)B * K;
  const void* in[5] = {lm_scores, lengths, d_logits, ids, alphas};
  const size_t in_b[5] = {n * 4, n * 4, n * R * 4, n * L * 8, n * L * P * 4};
  const char* in_n[5] = {"lm_scores", "lengths", "d_logits", "ids", "alphas"};
  const void* out[7] = {order, final_scores, d_scores, out_ids, out_lm_scores, out_lengths, out_alphas};
  const size_t out_b[7] = {n * 4, n * 4, n * 4, n * L * 8, n * 4, n * 4, n * L * P * 4};
  const char* out_n[7] = {"order", "final_scores", "d_scores", "out_ids", "out_lm_scores", "out_lengths", "out_alphas"};
  for (int o = 0; o < 7; ++o) {
    for (int i = 0; i < 5; ++i)
      GIC_CHECK_ARG(!overlaps(out[o], out_b[o], in[i], in_b[i]), "rerank: %s aliases %s (the gather is not in-place)", out_n[o], in_n[i]);
    for (int p = 0; p < o; ++p)
      GIC_CHECK_ARG(!overlaps(out[o], out_b[o], out[p], out_b[p]), "rerank: %s aliases %s", out_n[o], out_n[p]);
  }
  hipLaunchKernelGGL(rerank_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, lm_scores, lengths, length_penalty, d_logits, R, weight, ids, alphas,
                     K, L, P, order, final_scores, d_scores, out_ids, out_lm_scores, out_lengths, out_alphas);
  GIC_CHECK_LAUNCH("rerank");
  return GIC_OK;
}

int gic_disc_rep_mean(const gic_disc_dims* dims, const gic_disc_state* state, const float* logits, float* ybar, float* lbar, void* stream) {
  GIC_CHECK_ARG(dims, "disc_rep_mean: null dims");
  GIC_CHECK_ARG(dims->B >= 1 && dims->R >= 1, "disc_rep_mean: B=%d and R=%d must be >= 1", dims->B, dims->R);
  GIC_CHECK_ARG(dims->B <= 65535, "disc_rep_mean: B=%d exceeds 65535 captions per call (the grid's second dimension)", dims->B);
  GIC_CHECK_ARG(dims->dtype == DT_F32 || dims->dtype == DT_BF16, "disc_rep_mean: bad dtype");
  GIC_CHECK_ARG(dims->F >= 1 && dims->Fp >= dims->F && dims->Fp % 8 == 0, "disc_rep_mean: Fp=%d must be >= F=%d >= 1 and a multiple of 8", dims->Fp,
                dims->F);
  GIC_CHECK_ARG(state, "disc_rep_mean: null state");
  GIC_CHECK_ARG(state->ydrop, "disc_rep_mean: null state buffer (ydrop)");
  GIC_CHECK_ARG((((uintptr_t)state->ydrop) & 15) == 0, "disc_rep_mean: ydrop must be 16-byte aligned");
  GIC_CHECK_ARG(ybar, "disc_rep_mean: null ybar");
  GIC_CHECK_ARG((logits != nullptr) == (lbar != nullptr), "disc_rep_mean: pass logits and lbar together or neither");
  const dim3 grid(cdiv(dims->Fp / 4, 64), dims->B);
  if (dims->dtype == DT_F32)
    hipLaunchKernelGGL((disc_rep_mean_kernel<float>), grid, dim3(64), 0, (hipStream_t)stream, (const float*)state->ydrop, logits, ybar, lbar, dims->R,
                       dims->F, dims->Fp);
  else
    hipLaunchKernelGGL((disc_rep_mean_kernel<bf16_t>), grid, dim3(64), 0, (hipStream_t)stream, (const bf16_t*)state->ydrop, logits, ybar, lbar, dims->R,
                       dims->F, dims->Fp);
  GIC_CHECK_LAUNCH("disc_rep_mean");
  return GIC_OK;
}

int gic_match_ranks(const float* S, int64_t ld, const float* row_bias, int32_t N, int32_t* rank_c2i, int32_t* rank_i2c, void* stream) {
  GIC_CHECK_ARG(S, "match_ranks: null S");
  GIC_CHECK_ARG(rank_c2i && rank_i2c, "match_ranks: null rank_c2i / rank_i2c");
  GIC_CHECK_ARG(N >= 1, "match_ranks: N=%d must be >= 1", N);
  GIC_CHECK_ARG(ld >= N, "match_ranks: ld=%lld must be >= N=%d", (long long)ld, N);
  GIC_CHECK_ARG(rank_c2i != rank_i2c, "match_ranks: rank_c2i aliases rank_i2c");
  hipStream_t st = (hipStream_t)stream;
  GIC_PROPAGATE(fill_zero(rank_c2i, (size_t)N * sizeof(int32_t), st));      // (the rank counters; fill_zero: a kernel node inside a capture)
  GIC_PROPAGATE(fill_zero(rank_i2c, (size_t)N * sizeof(int32_t), st));
  hipLaunchKernelGGL(match_ranks_kernel, dim3(cdiv(N, 256), cdiv(N, RANK_ROWS)), dim3(256), 0, st, S, (long)ld, row_bias, N, rank_c2i, rank_i2c);
  GIC_CHECK_LAUNCH("match_ranks");
  return GIC_OK;
}

}  // extern "C"
