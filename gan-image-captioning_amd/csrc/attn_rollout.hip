// Monte-Carlo roll-outs of the attention decoder (gicap.h gic_attn_rollout / gic_attn_rollout_ws_bytes): the SeqGAN step's roll-out batch
// -- rows = (L - 1) * N * B, row r of image r % B -- which copies its caption's prefix and then samples, joined at its prefix length from
// the recurrent state of a teacher-forced pass along the captions (gic_attn_forward_tf).  The attention counterpart of the LSTM
// decoder's resumed roll-out (decoder.hip, resume_from), whose join, pick and Gumbel-argmax launches it shares (kernels.h).
//
// Step t with M_t = host_active_rows[t] rows (the first M_t: rows are sorted by prefix length):
//   rollout_join        rows [M_{t-1}, M_t) take the whole slot row [x_t | z_t | h_{t-1}] and c_t of caption r % B from the saved state:
//                       attention at step t depends on h_{t-1} only, so their z_t is already there
//   hp GEMM             hp [M_{t-1}, A] = h_{t-1} W_h^T of the rows that were already running (the library GEMM, never split over K)
//   attn_rows           energies, softmax and context of those rows (below); z into the rows' z columns
//   gates GEMM          [M_t, 4H] = [x | z | h] Wcat^T + bsum (never split over K), lstm_pointwise_fwd (h in place, c ping-pong)
//   gemm_gumbelmax      the vocabulary product with Gumbel-max in its epilogue, rollout_pick (token, ids[:, t], next x); where it declines
//                       the shapes (f32 mode, few rows): the product into logits and rollout_argmax
// 6 launches a step (5 at the first step with rows, where nothing was running yet) whatever M_t and the rows per image are.
//
// attn_rows: the image data is stored once per image (fproj [B, P, A], fmap [B, P, C]) and a workgroup = (image, tile of TR of its
// rows).  Nothing has a [rows, P, .] shape: the tile's energies / alphas live in LDS.
//   energies   e[r, i] = w_a . tanh(fp[i, :] + hp[r, :]): the (row, position) pairs of a chunk of 64 positions are dealt to the threads
//              (thread q takes pairs q, q + 256, ...: every lane works whatever P is), the attention width is walked in chunks of 64
//              columns staged in LDS as f32 (fp chunk [64][64], hp chunk [TR][64], w_a chunk), so an image's P x A slab of any size is
//              walked, never held.  A pair's sum runs over the columns in ascending order in one thread.
//   softmax    one wave per row over the P positions (expf as attn_step); positions P .. Ppad and rows past the tile's last get alpha 0
//   context    z[r, :] = sum_i alpha[r, i] fmap[i, :]: bf16 mode -- per 128 channels the [TR x Ppad] . [Ppad x 128] product on
//              mfma_f32_16x16x32_bf16: A operand = alpha from LDS (f32 -> bf16), B operand = the fmap tile stored TRANSPOSED in LDS
//              ([channel][position], P padded with zeros to the chunk of 64 = two K steps) so a lane's 8 consecutive positions are one
//              16-byte read; f32 mode -- plain FMAs, thread = (channel, TR / 4 rows), positions in ascending order.
// No atomics; each energy, alpha and z value has one writer and every sum a fixed order: two calls give the same bits.
//
// Workspace (one caller-owned buffer, every region 256-byte aligned, all affine in rows):
//   xh act [rows][E + C + H]; c f32 [2][rows][H]; gpre f32 [rows][4H]; hp f32 [rows][A]; rowkey u64 [L][rows];
//   logits f32 [fallback rows][V] -- only the row counts gemm_gumbelmax declines (all rows where it never takes the shapes)
#include "../../include/gicap.h"
#include "decoder_step.h"
#include "kernels.h"

namespace gic {
namespace {

constexpr int kPC = 64;              // positions per chunk (two K steps of the MFMA)
constexpr int kAC = 64;              // attention columns per chunk
constexpr int kLd = kAC + 4;         // row stride of the staged chunks (f32; 16-byte rows, off the bank period)
constexpr int kCtxT = kPC + 8;       // row stride of the transposed fmap tile (bf16; 16-byte rows)

struct AttnRowsArgs {
  const void* fproj;                 // act [B, P, A]
  const void* fmap;                  // act [B, P, C]
  const float* w_a;                  // [A]
  const float* hp;                   // [M, A]
  void* z; long ldx;                 // act: row r's z at z + r * ldx
  int B, M, P, A, C;                 // images, active rows (row r of image r % B)
};

__host__ __device__ inline int attn_rows_ppad(int P) { return (P + kPC - 1) / kPC * kPC; }
template <int TR>
__host__ __device__ inline size_t attn_rows_lds(int P) {
  return ((size_t)TR * (attn_rows_ppad(P) + 4) + kPC * kLd + TR * kLd + kAC) * sizeof(float);
}

template <typename TA, int TR>
__global__ __launch_bounds__(256) void attn_rows_kernel(const AttnRowsArgs a) {
  constexpr int NV = Vec16<TA>::NV;
  constexpr int KP = TR * kPC / 256;                     // pairs per thread and position chunk
  extern __shared__ float ar_smem[];
  const int Ppad = attn_rows_ppad(a.P), Pld = Ppad + 4;
  float* e_s = ar_smem;                                  // [TR][Pld] energies, then alphas
  float* stage = e_s + TR * Pld;
  float* fp_s = stage;                                   // [kPC][kLd]
  float* hp_s = fp_s + kPC * kLd;                        // [TR][kLd]
  float* wa_s = hp_s + TR * kLd;                         // [kAC]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nrows = a.M > b ? (a.M - b + a.B - 1) / a.B : 0;          // rows b, b + B, ... below M
  const int r0 = blockIdx.y * TR;
  const int tr = min(TR, nrows - r0);
  if (tr <= 0) return;
  const TA* fp = (const TA*)a.fproj + (long)b * a.P * a.A;
  const float* hp = a.hp + ((long)b + (long)a.B * r0) * a.A;          // tile row r at hp + r * B * A
  const long hp_ld = (long)a.B * a.A;

  // ---- energies
  for (int p0 = 0; p0 < a.P; p0 += kPC) {
    const int pv = min(kPC, a.P - p0), npairs = tr * pv;
    float acc[KP];
    int pr[KP], pi[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int q = tid + 256 * k, r = q / pv;
      pr[k] = q < npairs ? r : -1;
      pi[k] = q - r * pv;
      acc[k] = 0.f;
    }
    for (int a0 = 0; a0 < a.A; a0 += kAC) {
      const int av = min(kAC, a.A - a0);                 // a multiple of 8
      __syncthreads();
      const int pcs = av / NV;
      for (int x = tid; x < pv * pcs; x += 256) {
        const int i = x / pcs, jp = x - i * pcs;
        float v[NV];
        Vec16<TA>::load(fp + (long)(p0 + i) * a.A + a0 + jp * NV, v);
#pragma unroll
        for (int q = 0; q < NV; q += 4) *(f32x4*)(fp_s + i * kLd + jp * NV + q) = (f32x4){v[q], v[q + 1], v[q + 2], v[q + 3]};
      }
      const int pc4 = av / 4;
      for (int x = tid; x < tr * pc4; x += 256) {
        const int r = x / pc4, j4 = x - r * pc4;
        *(f32x4*)(hp_s + r * kLd + j4 * 4) = *(const f32x4*)(hp + r * hp_ld + a0 + j4 * 4);
      }
      if (tid < av) wa_s[tid] = a.w_a[a0 + tid];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (pr[k] < 0) continue;
        const float* f = fp_s + pi[k] * kLd;
        const float* h = hp_s + pr[k] * kLd;
        float s = acc[k];
        for (int j = 0; j < av; j += 4) {
          const f32x4 fv = *(const f32x4*)(f + j), hv = *(const f32x4*)(h + j), wv = *(const f32x4*)(wa_s + j);
          s += wv.x * tanhf(fv.x + hv.x);
          s += wv.y * tanhf(fv.y + hv.y);
          s += wv.z * tanhf(fv.z + hv.z);
          s += wv.w * tanhf(fv.w + hv.w);
        }
        acc[k] = s;
      }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (pr[k] >= 0) e_s[pr[k] * Pld + p0 + pi[k]] = acc[k];
  }
  __syncthreads();

  // ---- alpha = softmax over the P positions, one wave per row; zero beyond P and beyond the tile's rows
  for (int r = w; r < TR; r += 4) {
    float* er = e_s + r * Pld;
    if (r < tr) {
      float m = -INFINITY;
      for (int i = lane; i < a.P; i += 64) m = fmaxf(m, er[i]);
      m = wave_max(m);
      float s = 0.f;
      for (int i = lane; i < a.P; i += 64) {
        const float x = expf(er[i] - m);
        er[i] = x;
        s += x;
      }
      s = wave_sum(s);
      for (int i = lane; i < a.P; i += 64) er[i] = er[i] / s;
      for (int i = a.P + lane; i < Ppad; i += 64) er[i] = 0.f;
    } else {
      for (int i = lane; i < Ppad; i += 64) er[i] = 0.f;
    }
  }
  __syncthreads();

  // ---- context
  TA* z = (TA*)a.z + ((long)b + (long)a.B * r0) * a.ldx;              // tile row r at z + r * B * ldx
  const long z_ld = (long)a.B * a.ldx;
  if constexpr (sizeof(TA) == 2) {
    constexpr int MT = TR / 16;
    bf16_t* fmT = (bf16_t*)stage;                        // [128 channels][kCtxT positions]
    const int lr = lane & 15, lg = lane >> 4;
    const bf16_t* fm = (const bf16_t*)a.fmap + (long)b * a.P * a.C;
    for (int c0 = 0; c0 < a.C; c0 += 128) {
      f32x4 acc[MT][2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      for (int p0 = 0; p0 < Ppad; p0 += kPC) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {                    // 64 positions x 16 pieces of 8 channels (zeros beyond P and C)
          const int x = tid + 256 * k, i = x >> 4, cp = x & 15, c = c0 + cp * 8;
          bf16x8 v;
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = (bf16_t)0.f;
          if (p0 + i < a.P && c < a.C) v = *(const bf16x8*)(fm + (long)(p0 + i) * a.C + c);
#pragma unroll
          for (int q = 0; q < 8; ++q) fmT[(cp * 8 + q) * kCtxT + i] = v[q];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kPC / 32; ++ks) {
          bf16x8 fa[MT], fb[2];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const float* src = e_s + (mt * 16 + lr) * Pld + p0 + ks * 32 + lg * 8;
            const f32x4 x0 = *(const f32x4*)src, x1 = *(const f32x4*)(src + 4);
            fa[mt][0] = (bf16_t)x0.x; fa[mt][1] = (bf16_t)x0.y; fa[mt][2] = (bf16_t)x0.z; fa[mt][3] = (bf16_t)x0.w;
            fa[mt][4] = (bf16_t)x1.x; fa[mt][5] = (bf16_t)x1.y; fa[mt][6] = (bf16_t)x1.z; fa[mt][7] = (bf16_t)x1.w;
          }
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) fb[nt] = *(const bf16x8*)(fmT + (w * 32 + nt * 16 + lr) * kCtxT + ks * 32 + lg * 8);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mt], fb[nt], acc[mt][nt], 0, 0, 0);
        }
      }
      // accumulator register q of lane (lr, lg): row 4 lg + q, column lr
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const int c = c0 + w * 32 + nt * 16 + lr;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int r = mt * 16 + 4 * lg + q;
            if (r < tr && c < a.C) z[r * z_ld + c] = (bf16_t)acc[mt][nt][q];
          }
        }
    }
  } else {
    constexpr int RW = TR / 4;                           // rows per thread: wave w takes rows w * RW ..
    float* fm_s = stage;                                 // [kPC positions][64 channels]
    const float* fm = (const float*)a.fmap + (long)b * a.P * a.C;
    for (int c0 = 0; c0 < a.C; c0 += 64) {
      float acc[RW];
#pragma unroll
      for (int k = 0; k < RW; ++k) acc[k] = 0.f;
      for (int p0 = 0; p0 < Ppad; p0 += kPC) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {                    // 64 positions x 16 pieces of 4 channels (zeros beyond P and C)
          const int x = tid + 256 * k, i = x >> 4, cp = x & 15, c = c0 + cp * 4;
          f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (p0 + i < a.P && c < a.C) v = *(const f32x4*)(fm + (long)(p0 + i) * a.C + c);
          *(f32x4*)(fm_s + i * 64 + cp * 4) = v;
        }
        __syncthreads();
        for (int i = 0; i < kPC; ++i) {
          const float v = fm_s[i * 64 + lane];
#pragma unroll
          for (int k = 0; k < RW; ++k) acc[k] += e_s[(w * RW + k) * Pld + p0 + i] * v;
        }
      }
      const int c = c0 + lane;
#pragma unroll
      for (int k = 0; k < RW; ++k) {
        const int r = w * RW + k;
        if (r < tr && c < a.C) z[r * z_ld + c] = acc[k];
      }
    }
  }
}

template <typename TA, int TR>
int attn_rows_launch(const AttnRowsArgs& f, hipStream_t stream) {
  const size_t lds = attn_rows_lds<TR>(f.P);
  static LdsGrant granted;
  if (!grant_lds(attn_rows_kernel<TA, TR>, lds, granted)) {
    set_last_error("attn_rows: cannot reserve %zu bytes of LDS", lds);
    return GIC_ERR_LAUNCH;
  }
  const int per_image = cdiv(f.M, f.B);
  hipLaunchKernelGGL((attn_rows_kernel<TA, TR>), dim3((unsigned)f.B, (unsigned)cdiv(per_image, TR)), dim3(256), lds, stream, f);
  GIC_CHECK_LAUNCH("attn_rows");
  return GIC_OK;
}

// tiles of 32 rows while their energies and the staged chunks fit the 64 KB every kernel has, else tiles of 16 (P = 1024: 88 KB)
int attn_rows(const AttnRowsArgs& f, int dt, hipStream_t stream) {
  const bool big = attn_rows_lds<32>(f.P) <= 64 * 1024;
  if (dt == DT_F32) return big ? attn_rows_launch<float, 32>(f, stream) : attn_rows_launch<float, 16>(f, stream);
  return big ? attn_rows_launch<bf16_t, 32>(f, stream) : attn_rows_launch<bf16_t, 16>(f, stream);
}

// ids[r, t] = the caption of image r % B for t < force_len[r], else 0: the steps from force_len[r] on are written by the roll-out
__global__ void rollout_ids_init_kernel(const int64_t* __restrict__ caps, const int32_t* __restrict__ force_len, int64_t* __restrict__ ids,
                                        long rows, int B, int L) {
  const long total = rows * L;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / L;
    const int t = (int)(i - r * L);
    ids[i] = t < force_len[r] ? caps[(r % B) * L + t] : 0;
  }
}

// gemm_gumbelmax takes a step's vocabulary product from this many rows on (gemm.h: the selection's own predicate, its environment
// switches included); 0 = never.  Steps with fewer rows go through the logits scratch, which is sized for exactly those.
long gumbelmax_from_rows(const ACtx& c) { return gemm_gumbelmax_from_cols(c.dt, c.V, c.H, c.H, c.ldx()); }

struct RolloutBufs {
  void* xh; float* c[2]; float* gpre; float* hp; unsigned long long* rowkey; float* logits;
  long logit_rows;
  size_t total;
};

RolloutBufs rollout_layout(const ACtx& c, long rows, void* ws) {
  RolloutBufs o{};
  size_t at = 0;
  auto take = [&](size_t bytes) { void* p = (void*)((uintptr_t)ws + at); at += (bytes + 255) & ~(size_t)255; return p; };
  const size_t R = (size_t)rows;
  o.xh = take(R * c.ldx() * c.asz());
  float* cc = (float*)take(2 * R * c.H * 4);
  o.c[0] = cc; o.c[1] = cc + R * c.H;
  o.gpre = (float*)take(R * 4 * c.H * 4);
  o.hp = (float*)take(R * c.A * 4);
  o.rowkey = (unsigned long long*)take((size_t)c.L * R * 8);
  const long from = gumbelmax_from_rows(c);
  o.logit_rows = from == 0 || rows < from ? rows : from - 1;
  o.logits = (float*)take((size_t)o.logit_rows * c.V * 4);
  o.total = at;
  return o;
}

int check_rollout_rows(const ACtx& c, int64_t rows, const char* who) {
  GIC_CHECK_ARG(rows >= 1 && rows <= (1l << 22) && rows * (long)c.ldx() < (1l << 30) && rows * 4l * c.H < (1l << 31),
                "%s: rows must be 1..2^22 with rows * (E + C + H) below 2^30 and rows * 4H below 2^31, got %lld", who, (long long)rows);
  GIC_CHECK_ARG(c.L >= 2 && c.L <= 1024, "%s: L must be 2..1024", who);
  return GIC_OK;
}

int attn_rollout_run(const ACtx& c, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* from, const void* fmap,
                     const int64_t* caps, int rows, const int32_t* force_len, const int32_t* act, const float* noise_u, uint64_t seed, void* ws, int64_t* ids,
                     hipStream_t stream) {
  const int B = c.B, L = c.L, V = c.V, E = c.E, H = c.H;
  const long ld = c.ldx();
  const size_t asz = c.asz();
  const RolloutBufs w = rollout_layout(c, rows, ws);
  // a step of at least `from` rows takes the fused vocabulary product (the logits scratch holds only the steps below it)
  RowkeySteps keyed{gumbelmax_from_rows(c), true, false};
  // route-only mode (gemm.h): the steps' products are selected in launch order; nothing is launched or filled
  const bool probe = route_only();
  if (!probe) {
    const long total = (long)rows * L;
    const unsigned grid = (unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
    hipLaunchKernelGGL(rollout_ids_init_kernel, dim3(grid), dim3(256), 0, stream, caps, force_len, ids, (long)rows, B, L);
    GIC_CHECK_LAUNCH("rollout_ids_init");
  }
  if (!probe) GIC_PROPAGATE(fill_zero(w.rowkey, (size_t)L * rows * sizeof(unsigned long long), stream));        // atomicMax targets start below every key
  char* xh = (char*)w.xh;
  char* h = xh + (size_t)c.din() * asz;                  // the h columns of row 0
  for (int t = 0; t < L; ++t) {
    const int M = act[t], Mp = t > 0 ? act[t - 1] : 0;
    float* c_cur = w.c[t & 1];
    float* c_new = w.c[(t & 1) ^ 1];
    if (M > Mp)
      GIC_PROPAGATE(rollout_join((const unsigned char*)from->xh + (size_t)t * B * ld * asz, (unsigned char*)xh, ld * (long)asz,
                                 from->c + (long)t * B * H, c_cur, H, Mp, M, B, stream));
    if (M == 0) continue;
    if (Mp > 0) {
      GemmDesc g;                // hp [Mp, A] = h_{t-1} W_h^T
      g.A = h; g.lda = ld; g.B = S->wh; g.ldb = H; g.C = w.hp; g.ldc = c.A;
      g.M = Mp; g.N = c.A; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32;
      g.no_split = 1;
      GIC_PROPAGATE(gemm(g, stream));
      AttnRowsArgs f;
      f.fproj = from->fproj; f.fmap = fmap; f.w_a = P->w_a; f.hp = w.hp; f.z = xh + (size_t)E * asz; f.ldx = ld;
      f.B = B; f.M = Mp; f.P = c.P; f.A = c.A; f.C = c.C;
      if (!probe) GIC_PROPAGATE(attn_rows(f, c.dt, stream));
    }
    {
      GemmDesc g;                // gate pre-activations of all M rows
      g.A = xh; g.lda = ld; g.B = S->wcat; g.ldb = ld; g.C = w.gpre; g.ldc = 4 * H;
      g.M = M; g.N = 4 * H; g.K = (int)ld; g.in_dtype = c.dt; g.out_dtype = DT_F32; g.bias = S->bsum;
      g.no_split = 1;
      GIC_PROPAGATE(gemm(g, stream));
    }
    GIC_PROPAGATE(lstm_pointwise_fwd(c.dt, w.gpre, c_cur, c_new, h, ld, nullptr, 0, M, H, stream));
    const float* u_t = noise_u ? noise_u + (long)t * rows * V : nullptr;
    int s = GIC_ERR_UNSUPPORTED;
    unsigned long long* key = w.rowkey + (long)t * rows;
    if (keyed.take(M)) {
      GemmDesc g;                // vocabulary product with Gumbel-max in its epilogue
      g.A = S->wout; g.lda = H; g.B = h; g.ldb = ld;
      g.M = V; g.N = M; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32;
      g.gm_rowkey = key; g.gm_bias = P->b_out; g.gm_u = u_t; g.gm_ldu = V; g.gm_temperature = 1.f;
      g.seed = seed; g.stream = (uint64_t)t;
      s = gemm_gumbelmax(g, stream);
    }
    if (s == GIC_OK) {
      GIC_PROPAGATE(rollout_pick(c.dt, key, ids + t, (long)L, P->embed, xh, ld, M, V, E, nullptr, nullptr, t, stream));
      continue;
    }
    if (s != GIC_ERR_UNSUPPORTED) return s;
    if (M > w.logit_rows) {
      set_last_error("attn_rollout: the fused vocabulary product declined a step of %d rows; the workspace holds logits for %ld", M, w.logit_rows);
      return GIC_ERR_WORKSPACE;
    }
    GemmDesc g;
    g.A = h; g.lda = ld; g.B = S->wout; g.ldb = H; g.C = w.logits; g.ldc = V;
    g.M = M; g.N = V; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32; g.bias = P->b_out;
    g.no_split = 1;
    GIC_PROPAGATE(gemm(g, stream));
    GIC_PROPAGATE(rollout_argmax(c.dt, w.logits, u_t, seed, (uint64_t)t, 1.f, 0, nullptr, 0, ids + t, (long)L, P->embed, xh, ld, M, V, E, nullptr,
                                 nullptr, t, stream));
  }
  return GIC_OK;
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_attn_rollout_ws_bytes(const gic_attn_dims* dims, int64_t rows, uint64_t* out) {
  ACtx c;
  GIC_PROPAGATE(check_attn_dims(dims, c));
  GIC_PROPAGATE(check_rollout_rows(c, rows, "attn_rollout_ws_bytes"));
  GIC_CHECK_ARG(out, "attn_rollout_ws_bytes: null out");
  *out = (uint64_t)rollout_layout(c, rows, nullptr).total;
  return GIC_OK;
}

int gic_attn_rollout(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_attn_state* resume_from,
                     const void* fmap, const int64_t* force_ids, int64_t rows, const int32_t* force_len, const int32_t* host_active_rows,
                     const float* noise_u, uint64_t seed, void* ws, int64_t* ids, void* stream) {
  ACtx c;
  GIC_PROPAGATE(check_attn_dims(dims, c));
  GIC_PROPAGATE(check_rollout_rows(c, rows, "attn_rollout"));
  GIC_CHECK_ARG(P && S && resume_from && fmap && force_ids && force_len && host_active_rows && ws && ids, "attn_rollout: null argument");
  GIC_CHECK_ARG(P->embed && P->b_out && P->w_a && S->wcat && S->bsum && S->wout && S->wh, "attn_rollout: null weights");
  GIC_CHECK_ARG(resume_from->xh && resume_from->c && resume_from->fproj, "attn_rollout: resume_from lacks xh, c or fproj");
  GIC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "attn_rollout: the workspace must be 256-byte aligned");
  // what the fused vocabulary product asks of its pointers beyond the shapes: checked here, so that a step it is sized to take is taken
  GIC_CHECK_ARG(gumbelmax_from_rows(c) == 0 || ((((uintptr_t)P->b_out | (uintptr_t)S->wout | (uintptr_t)noise_u) & 15) == 0),
                "attn_rollout: b_out, the wout image and noise_u must be 16-byte aligned");
  GIC_CHECK_ARG(host_active_rows[0] == 0, "attn_rollout: host_active_rows[0] must be 0 (a row has a prefix of at least one token)");
  for (int t = 1; t < c.L; ++t)
    GIC_CHECK_ARG(host_active_rows[t] >= host_active_rows[t - 1] && host_active_rows[t] <= rows,
                  "attn_rollout: host_active_rows must be non-decreasing and <= rows");
  return attn_rollout_run(c, P, S, resume_from, fmap, force_ids, (int)rows, force_len, host_active_rows, noise_u, seed, ws, ids, (hipStream_t)stream);
}

}  // extern "C"
