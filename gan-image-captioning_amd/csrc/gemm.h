// Host-side descriptor of the one MFMA GEMM family every dense contraction of
// the hot path goes through (kernels in gemm.hip).
//
//   C[m,n] = epi( alpha * sum_k A(m,k) * B(n,k) )
//
// A(m,k) = a_kc ? A[m*lda + k] : A[k*lda + m]      (k-contiguous / m-contiguous)
// B(n,k) = b_kc ? B[n*ldb + k] : B[k*ldb + n]
// so  forward  y = x W^T      : a_kc=1, b_kc=1   ("NT")
//     dgrad    dx = dy W      : a_kc=1, b_kc=0   ("NN")
//     wgrad    dW = dy^T x    : a_kc=0, b_kc=0   ("TN")
// The wgrad form can carry two extras (fields at the end of GemmDesc): the column sums of A -- a_sum[m] (+)= sum_k A(m,k), the bias
// gradient of the layer, out of the A chunks the product stages anyway -- and a second output matrix C2 for the columns from n_split on
// (dW_ih | dW_hh of an LSTM layer over xh = [x | h] in one launch).  Conditions: bf16 operands, a_kc == 0 && b_kc == 0, EPI_PLAIN, no convolution, the
// 16-byte vectorised path, deterministic mode off, c_zeroed == 0; n_split a multiple of the tile width.  wgrad_folds_a_sum() /
// wgrad_tile_n() below are the rule as host predicates.
#pragma once
#include "common.h"

namespace gic {

enum GemmEpi { EPI_PLAIN = 0, EPI_HIGHWAY = 1, EPI_BNSTATS = 2, EPI_GUMBELMAX = 3 };

struct GemmDesc {
  const void* A = nullptr;
  const void* B = nullptr;
  void* C = nullptr;
  int M = 0, N = 0, K = 0;
  long lda = 0, ldb = 0, ldc = 0;
  int a_kc = 1, b_kc = 1;
  int in_dtype = DT_F32, out_dtype = DT_F32;
  const float* bias = nullptr;   // per output column n (optional)
  int accumulate = 0;            // C += result
  int c_zeroed = 0;              // caller guarantees C is all zero: a split-K launch skips its own zero fill
  int no_split = 0;              // never split K (no f32 atomics: the same bits on every call, in or out of the deterministic mode)
  float alpha = 1.f;
  int epi = EPI_PLAIN;
  // ---- EPI_HIGHWAY (discriminator.py:53-58): h = acc+bias; y = sig(h)*relu(h) + (1-sig(h))*x; C = y*keep*keep_scale
  const void* X = nullptr; long ldx = 0;        // carry input, in_dtype
  union { float* Hpre = nullptr; float* a_sum2; };   // pre-activation h (saved for backward)          | a_sum2, below
  union { long ldh = 0; long ldc2; };                //                                                | ldc2, below
  const uint8_t* mask = nullptr; long ldmask = 0;   // explicit keep mask (0/1) or null
  uint8_t* mask_out = nullptr; long ldmask_out = 0;   // keep mask actually used, written for backward (optional)
  float keep_scale = 1.f;                       // 1/(1-p) in train mode, 1 in eval
  union { int use_philox = 0; int wgrad; }; float drop_p = 0.f; uint64_t seed = 0, stream = 0;
  const uint64_t* seed_dev = nullptr;           // non-null: the Philox seed is read from device memory (gic_step_scalars), `seed` is ignored
  // ---- implicit-GEMM convolution (conv != 0): A(m,k) is gathered from an NHWC activation `A`
  //      [Nimg, cH, cW, cCin] with m = (n, ho, wo) and k = (r, s, c); M = Nimg*cHo*cWo, K = cKH*cKW*cCin;
  //      B = weights [Cout, cKH, cKW, cCin] (k-contiguous).  Out-of-image taps read as zero.
  int conv = 0;
  int cH = 0, cW = 0, cCin = 0, cHo = 0, cWo = 0, cKH = 0, cKW = 0, cStride = 1, cPad = 0;
  // ---- EPI_BNSTATS: C = result (+bias) and stats[n] += sum_m v, stats[N+n] += sum_m v^2 (f32 atomics)
  union { float* stats = nullptr; float* a_sum; };   // [stats_nrep][2N]; block b adds into replica b % stats_nrep (readers sum the replicas) | a_sum, below
  int stats_nrep = 1;
  // ---- A-side BatchNorm + ReLU (tile8 convolutions with Cin % 8 == 0, Cin <= 1024): the input activation is read as
  //      relu(scale[c] * x + shift[c]) (zero padding applied AFTER it, as the reference pads the normalised tensor) with
  //      scale / shift from the producer's batch statistics in_stats [in_nrep][2 Cin] (sum, sum of squares over
  //      in_inv_count^-1 rows), in_gamma, in_beta.  The producer's raw output is consumed directly: its separate
  //      normalisation pass (and the normalised tensor) disappear.
  const float* in_stats = nullptr; int in_nrep = 1;
  const float* in_gamma = nullptr; const float* in_beta = nullptr;
  float in_inv_count = 0.f;
  // ---- ... + residual (the block output of a ResNet bottleneck formed on load; 1x1 / stride 1 / pad 0 consumers only): the operand is
  //      relu(scale*x + shift + r) with r = res[m, c] as is (identity shortcut) or res_scale*res + res_shift from res_stats / res_gamma /
  //      res_beta (projection shortcut, its own BatchNorm).  Workgroups of the first N tile also WRITE the formed tile to out_wb
  //      [M, Cin] (the block output, needed again as the next shortcut): the separate bn + add + relu pass disappears.
  const void* res = nullptr;
  const float* res_stats = nullptr; int res_nrep = 1;
  const float* res_gamma = nullptr; const float* res_beta = nullptr;
  float res_inv_count = 0.f;
  union { void* out_wb = nullptr; void* C2; };       //                                                | C2, below
  // ---- EPI_GUMBELMAX (gemm_gumbelmax below): C is NOT written.  Rows m = vocabulary entries (A = W_out [V, H]), columns n = roll-out
  //      rows (B = their hidden states): key[n] = atomicMax over m of row_key((acc + gm_bias[m] + gumbel(u[n, m])) * gm_temperature, m)
  //      -- the token of an ids-only roll-out step (generator.py:68-73 with the softmax skipped: it is monotone) without the [rows, V]
  //      logits ever reaching memory.  u: gm_u (explicit uniforms, row n at gm_u + n * gm_ldu) or Philox(seed | seed_dev, stream) indexed
  //      as the unfused kernels index it (4 consecutive vocabulary entries of a row per call).
  unsigned long long* gm_rowkey = nullptr;
  const float* gm_bias = nullptr;
  const float* gm_u = nullptr; long gm_ldu = 0;
  float gm_temperature = 1.f;
  int n_fast = 0;           // tile8: the output-channel tiles of a row tile are neighbours on one XCD (xcd_share_a) instead of the row tiles of a channel tile
  union { int stats_only = 0; int n_split; };        // | n_split, below.  EPI_BNSTATS convolutions the streaming 1x1 kernel takes: the column sums only, C is NOT written (conv_b2b.hip's first pass);
                            // honoured by conv1x1_stream.hip alone: gemm() answers GIC_ERR_UNSUPPORTED when that kernel declines the shape
  int dbg = 0;              // phase-ablation knob, honoured only by -DGIC_STAMPS tool builds
  // ---- weight-gradient extras: honoured by gemm_kernel's vectorised form of a plain bf16 product with a_kc == 0 && b_kc == 0 (16-byte aligned
  //      operands, lda / ldb whole 16-byte chunks), outside the deterministic mode and without c_zeroed.
  //      a_sum[m] (+)= sum_k A(m,k), a_sum2 (optional) receives the same values: overwritten or accumulated as `accumulate` says for C;
  //      formed from the A chunks the workgroups of the first N tile stage anyway (a fixed-order sum without split-K, f32 atomics with
  //      it, over the split-K zero-fill launch, which clears them with C).  OPTIONAL: where another kernel runs the product the pointers
  //      are ignored, so a caller asks wgrad_folds_a_sum(d) and keeps its colsum() when the answer is false.
  //      C2 / ldc2 / n_split: columns n >= n_split go to C2[m * ldc2 + (n - n_split)], the others to C: one product over adjacent column
  //      ranges of one B for two output matrices.  n_split must be a multiple of the tile width (wgrad_tile_n(d)); gemm() answers
  //      GIC_ERR_UNSUPPORTED where it cannot honour a C2.
  //      `wgrad` != 0 says that the descriptor carries them: without it none of the fields below is looked at, whatever the unions hold.
  //      STORAGE: int wgrad, float* a_sum, float* a_sum2, void* C2, long ldc2 and int n_split are the union members declared above, beside stats, Hpre,
  //      out_wb, ldh, stats_only and use_philox -- fields of the BatchNorm-sum / highway epilogues and of convolutions, none of which a plain
  //      m/n-contiguous product has.  The descriptor is every GEMM kernel's by-value argument: with five more fields its size moved the
  //      scalar loads and waits of 16 instantiations that have nothing to do with them (tools/isa_diff.py --by-kernel); as unions every
  //      existing instantiation keeps its instruction stream (profiles/wgrad_fold_isa.txt).  Set them on plain products only.
};

// Enqueue on `stream`. Returns GIC_OK or a negative Status (message via gic_last_error()).
int gemm(const GemmDesc& d, hipStream_t stream);

// Every kernel family of the dispatch comes as a pair: select_*(shapes, plan) is a pure host function (no HIP call, no launch, no heap) that
// answers false or fills a plan -- the kernel's descriptor, the template arguments as plain values, the grid and the dynamic LDS bytes --
// and launch_*(plan, stream) asks for the LDS grant, switches on the variant and launches, with no condition on shapes or pointers of its
// own (false: the grant was refused, the caller goes on to its next candidate).

// What the trunk's convolution kernels (conv_stem / conv3x3 / conv1x1_stream / conv1x1_pix / conv1x1_panel .hip) share of a GemmDesc; their
// descriptors derive from it.
struct ConvBase {
  const void* A; const void* B; void* C; float* stats;
  const float* in_stats; const float* in_gamma; const float* in_beta;
  int M, N, lda, ldb, ldc, stats_nrep, in_nrep;
  float in_inv_count;
  unsigned a_bytes, b_bytes;
};

// BatchNorm on load: the coefficients' sources are all there
inline bool bn_in_args_ok(const GemmDesc& d) { return d.in_gamma && d.in_beta && d.in_inv_count > 0.f; }

// The preconditions those kernels have in common -- a bf16 convolution with the BatchNorm-sum epilogue and nothing else in it (no bias, alpha
// or accumulate), 16-byte aligned A, B and C, valid BatchNorm-on-load arguments if any, both operands (a_elems / b_elems elements, which the
// caller derives from its own window) under 2 GiB -- and, when they hold, the shared fields.
bool conv_base(const GemmDesc& d, long a_elems, long b_elems, ConvBase& b);

// Pure host predicates beside the selection (no HIP call): would gemm(d) fold d.a_sum into the product; the tile width (64 | 128) the
// 4-wave kernel would run d with where it can honour the weight-gradient extras at all, else 0 (C2 needs n_split % that == 0).
bool wgrad_folds_a_sum(const GemmDesc& d);
int wgrad_tile_n(const GemmDesc& d);
// Launches of the weight-gradient-extras form since the library was loaded, and those of them that wrote two matrices (tests: which route ran)
void wgrad_launch_counts(long* launches, long* two_matrix);

// Route-only mode (gic_debug_route_only, util.hip): gemm(), gemm_gumbelmax() and gic_conv_b2b validate and select, write the plan as one
// line into route_line() and return their status without touching the GPU.  gic_disc_fwd (disc.hip) answers with the selection of its
// highway product, the one caller of EPI_HIGHWAY, and launches none of its own kernels.  gic_disc_bwd, gic_disc_bwd_cond and
// gic_disc_fwd_redrop validate, run select_disc_bwd (the pair of this convention in disc.hip; gic_debug_disc_plan prints its plans) and
// return before their first launch or product.  So do the decoder passes (decoder_step.h: select_decoder_fwd / select_decoder_bwd,
// select_lstm_step / select_vocab_step; gic_debug_decoder_plan prints the plans): gic_decoder_sample_fwd, gic_decoder_sample_bwd, the
// teacher-forced entries of teacher_forced.hip (forward, scheduled sampling and backward, both decoders) and gic_attn_rollout.  lstm_step /
// vocab_step* answer with their plan as the route line; the fused roll-out and the backward entries return before their first product;
// the generic roll-outs and the teacher-forced forwards walk their steps and select each product in launch order, launching nothing, so
// the route line is their last product's (teacher_forced.hip: " ss_logits=fused" where vocab_step_logits replaces it).
bool route_only();
char* route_line();                    // thread-local, kRouteLen bytes
constexpr int kRouteLen = 160;

// The vocabulary product of an ids-only roll-out step fused with Gumbel-max (EPI_GUMBELMAX above): bf16 k-contiguous operands, M = V a
// multiple of 4, many roll-out rows (the 8-wave kernel's grid conditions).  GIC_ERR_UNSUPPORTED (no message) when the shapes do not
// qualify: the caller runs the product and the Gumbel-argmax kernel separately.
int gemm_gumbelmax(const GemmDesc& d, hipStream_t stream);
// Pure host function: the smallest N from which gemm_gumbelmax takes an M x N x K product of these operand layouts (the selection's own
// predicate, the GIC_NO_TILE8 / GIC_NO_FUSED_GUMBELMAX switches included), 0 = never.  Callers size the fallback's logits scratch by it.
long gemm_gumbelmax_from_cols(int in_dtype, int M, int K, long lda, long ldb);

}  // namespace gic
