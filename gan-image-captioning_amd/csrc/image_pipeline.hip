// gic_image_preprocess: everything between the JPEG decode and the trunk's input tensor in ONE kernel.  A ragged batch of uint8 images
// (HWC or HW, any size, any byte offset / row stride inside one flat buffer) -> crop box, horizontal flip, antialiased bilinear resize
// to S x S, grey -> 3 channels, ImageNet normalisation -> f32 [N,3,S,S].
//
// Filter (per axis; source length n, box [b0,b1), S outputs): the triangle filter whose support is scaled by the downscale factor,
//   scale = (b1-b0)/S, fs = max(scale,1), c_i = b0 + (i+0.5) scale, taps first = max(int(c_i-fs+0.5),0) .. last = min(int(c_i+fs+0.5),n),
//   w_x = max(0, 1 - |x - c_i + 0.5| / fs) normalised to sum 1 over the (image-clipped) taps;
// separable, horizontal pass first, no 8-bit rounding between the passes (what PIL's resize(BILINEAR, box=) and F.interpolate(bilinear,
// antialias=True) compute).
//
// Layout: one workgroup of 256 threads per (band of R = 8 output rows, image).  Thread t owns the items t, t+256, ... (ITEMS of them;
// item = 3 * column + channel, so neighbouring lanes read neighbouring bytes of a staged row) of all 8 rows in registers.  The workgroup
//   1. computes the tap descriptor of every output column {first, count, d0, norm} into LDS: centres and the weight sum in float64,
//      d0 = first - c_i + 0.5 rounded ONCE to f32 -- a tap's weight is then max(0, 1 - |d0 + k| / fs) norm with k = 0.. small, so no
//      absolute f32 coordinate ever appears; the descriptors of the band's 8 rows likewise;
//   2. streams the source rows the band needs, a few per pass: their bytes go to an LDS stage with aligned dword loads (each row from
//      its start rounded down to 4 bytes; the row keeps the shift), every load extent-checked against pixels_bytes (a dword that would
//      cross the end of the buffer is assembled from checked byte loads, past-the-end bytes read as 0), or byte by byte when `pixels`
//      itself is not 4-byte aligned;
//   3. resamples each staged row horizontally (k ascending) and adds w_y x that value into the accumulators of the band rows whose
//      support holds the row (y ascending): a fixed order, no atomics, the same bits whatever the staging.
// The tap count is a loop bound, not an array size: LDS = 16 S + the stage (>= one row span), independent of the downscale factor.
// Stores: every third lane holds consecutive x of one channel plane, so a wave writes three runs of ~21 consecutive floats per row;
// the next items complete the lines.
//
// The descriptors are validated on the host before anything is enqueued and travel to `ws` as kernel arguments of a staging kernel (no
// host memory is read after the call returns).
#include <math.h>

#include "../../include/gicap.h"
#include "common.h"

namespace gic {

static constexpr int IMG_R = 8;            // output rows per workgroup
static constexpr int IMG_THREADS = 256;
static constexpr int IMG_LOADS = 8;        // global loads a thread issues before it stores the first to LDS
static constexpr int IMG_MAX_S = 1024, IMG_MAX_SIDE = 16384;
static constexpr int IMG_STAGE_DESCS = 64;      // descriptors per staging launch (3.5 KB of kernel arguments: a batch of 64 is one launch)
static constexpr int IMG_STAGE_MIN = 16 * 1024; // bytes of row stage a workgroup takes when the rows are short (several rows per pass)

// what the kernel reads: the validated gic_image_src plus the source columns [x_lo, x_hi) any output column can touch
struct ImgDesc {
  int64_t offset;
  int32_t H, W, C, stride;
  float box[4];
  int32_t flip, x_lo, x_hi, pad;
};
struct ImgDescPack { ImgDesc d[IMG_STAGE_DESCS]; };

struct ColTap { int32_t first, count; float d0, norm; };

// one axis, output index i: taps [first, last) clipped to [lo, hi), d0 = first - c_i + 0.5 (f32), norm = 1 / sum of the weights
__host__ __device__ static inline void axis_taps(const double b0, const double b1, const int S, const int i, const int lo, const int hi,
                                                 int& first, int& last, double& centre, double& fs) {
  const double scale = (b1 - b0) / (double)S;
  fs = scale > 1.0 ? scale : 1.0;
  centre = b0 + ((double)i + 0.5) * scale;
  first = (int)(centre - fs + 0.5);
  last = (int)(centre + fs + 0.5);
  first = first < lo ? lo : first;
  last = last > hi ? hi : last;
  if (first > hi - 1) first = hi - 1;      // a centre in the last half pixel: keep one tap (its weight is > 0)
  if (last < first + 1) last = first + 1;
}

__device__ static inline ColTap make_tap(const double b0, const double b1, const int S, const int i, const int lo, const int hi) {
  int first, last;
  double c, fs;
  axis_taps(b0, b1, S, i, lo, hi, first, last, c, fs);
  const double d0 = (double)first - c + 0.5;
  const float d0f = (float)d0, inv = (float)(1.0 / fs);
  // the sum of the f32 weights the resampling loops will form, added in float64: the normalised weights then sum to 1 up to their
  // own roundings
  double sum = 0.0;
  for (int k = 0; k < last - first; ++k) sum += (double)fmaxf(0.f, 1.f - fabsf(d0f + (float)k) * inv);
  ColTap t;
  t.first = first;
  t.count = last - first;
  t.d0 = d0f;
  t.norm = sum > 0.0 ? (float)(1.0 / sum) : 0.f;
  return t;
}

__global__ void image_stage_descs_kernel(ImgDesc* dst, const ImgDescPack pack, const int n) {
  const int i = threadIdx.x;
  if (i < n) dst[i] = pack.d[i];
}

template <int ITEMS>
__global__ __launch_bounds__(IMG_THREADS) void image_preprocess_kernel(const uint8_t* __restrict__ pixels, const uint64_t pixels_bytes,
                                                                       const ImgDesc* __restrict__ descs, const int S, const float a0,
                                                                       const float a1, const float a2, const float m0, const float m1,
                                                                       const float m2, float* __restrict__ out, const int stage_bytes,
                                                                       const int dwords_ok) {
  extern __shared__ uint4 img_smem[];
  __shared__ ColTap row_tap[IMG_R];
  ColTap* col_tap = (ColTap*)img_smem;                        // [S]
  uint8_t* stage = (uint8_t*)(col_tap + S);                   // [stage_bytes], 16-byte aligned (sizeof(ColTap) = 16)
  const int tid = threadIdx.x, n = blockIdx.y, r0 = blockIdx.x * IMG_R;
  const int nr = min(IMG_R, S - r0);
  const ImgDesc d = descs[n];
  const int C = d.C;

  for (int i = tid; i < S; i += IMG_THREADS) col_tap[i] = make_tap((double)d.box[0], (double)d.box[2], S, i, d.x_lo, d.x_hi);
  if (tid < IMG_R) {
    ColTap t = {0, 0, 0.f, 0.f};
    if (tid < nr) t = make_tap((double)d.box[1], (double)d.box[3], S, r0 + tid, 0, d.H);
    row_tap[tid] = t;
  }
  __syncthreads();

  const int span = (d.x_hi - d.x_lo) * C;                     // bytes of a source row that the columns can touch
  const int pitch = (span + 3 + 3) & ~3;                      // + the shift of a row start rounded down to 4 bytes
  if (span <= 0 || pitch > stage_bytes) return;               // never for a validated descriptor: the host sized the stage from x_lo/x_hi
  const int rows_per_pass = stage_bytes / pitch, dw_per_row = pitch >> 2;
  const int y_lo = row_tap[0].first, y_hi = row_tap[nr - 1].first + row_tap[nr - 1].count;
  const double sx = ((double)d.box[2] - (double)d.box[0]) / (double)S, sy = ((double)d.box[3] - (double)d.box[1]) / (double)S;
  const float inv_x = (float)(1.0 / (sx > 1.0 ? sx : 1.0)), inv_y = (float)(1.0 / (sy > 1.0 ? sy : 1.0));

  // item e = 3 * column + channel: neighbouring lanes read neighbouring bytes of the stage (a grey image gives its one value to all three)
  float acc[ITEMS][IMG_R];
#pragma unroll
  for (int c = 0; c < ITEMS; ++c)
#pragma unroll
    for (int r = 0; r < IMG_R; ++r) acc[c][r] = 0.f;

  for (int yb = y_lo; yb < y_hi; yb += rows_per_pass) {
    const int rows = min(rows_per_pass, y_hi - yb);
    __syncthreads();                                          // the previous pass has been read
    if (dwords_ok) {
      // IMG_LOADS loads per thread in flight before the first LDS store: a pass costs one or two memory latencies, not fifteen
      const int total = rows * dw_per_row;
      for (int e0 = tid; e0 < total; e0 += IMG_THREADS * IMG_LOADS) {
        uint32_t v[IMG_LOADS];
#pragma unroll
        for (int u = 0; u < IMG_LOADS; ++u) {
          const int e = e0 + u * IMG_THREADS;
          v[u] = 0;
          if (e < total) {
            const int j = e / dw_per_row, t = e - j * dw_per_row;
            const int64_t g = d.offset + (int64_t)(yb + j) * d.stride + (int64_t)d.x_lo * C;
            const uint64_t off = (uint64_t)((g & ~(int64_t)3) + 4 * (int64_t)t);
            if (off + 4 <= pixels_bytes) {
              v[u] = *(const uint32_t*)(pixels + off);
            } else {
#pragma unroll
              for (int b = 0; b < 4; ++b)
                if (off + b < pixels_bytes) v[u] |= (uint32_t)pixels[off + b] << (8 * b);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < IMG_LOADS; ++u) {
          const int e = e0 + u * IMG_THREADS;                // = j * dw_per_row + t
          if (e < total) ((uint32_t*)stage)[e] = v[u];
        }
      }
    } else {
      for (int e = tid; e < rows * pitch; e += IMG_THREADS) {
        const int j = e / pitch, t = e - j * pitch;
        const uint64_t off = (uint64_t)(d.offset + (int64_t)(yb + j) * d.stride + (int64_t)d.x_lo * C + t);
        stage[e] = (t < span && off < pixels_bytes) ? pixels[off] : (uint8_t)0;
      }
    }
    __syncthreads();
    for (int j = 0; j < rows; ++j) {
      const int y = yb + j;
      float wy[IMG_R];
#pragma unroll
      for (int r = 0; r < IMG_R; ++r) {
        const ColTap t = row_tap[r];
        const int k = y - t.first;
        wy[r] = (k >= 0 && k < t.count) ? fmaxf(0.f, 1.f - fabsf(t.d0 + (float)k) * inv_y) * t.norm : 0.f;
      }
      const int shift = dwords_ok ? (int)((d.offset + (int64_t)y * d.stride + (int64_t)d.x_lo * C) & 3) : 0;
      const uint8_t* row = stage + j * pitch + shift;
#pragma unroll
      for (int c = 0; c < ITEMS; ++c) {
        const int e = tid + c * IMG_THREADS;
        if (e >= 3 * S) continue;
        const int i = e / 3, ch = e - 3 * i;
        const ColTap t = col_tap[i];
        const uint8_t* p = row + (t.first - d.x_lo) * C + (C == 3 ? ch : 0);
        float h = 0.f;
        // unrolled so that the LDS reads of several taps are in flight together; the additions keep their order (k ascending)
#pragma unroll 4
        for (int k = 0; k < t.count; ++k) {
          const float w = fmaxf(0.f, 1.f - fabsf(t.d0 + (float)k) * inv_x) * t.norm;
          h = fmaf(w, (float)p[C * k], h);
        }
#pragma unroll
        for (int r = 0; r < IMG_R; ++r) acc[c][r] = fmaf(wy[r], h, acc[c][r]);
      }
    }
  }

  const size_t plane = (size_t)S * S;
  float* o = out + (size_t)n * 3 * plane;
#pragma unroll
  for (int c = 0; c < ITEMS; ++c) {
    const int e = tid + c * IMG_THREADS;
    if (e >= 3 * S) continue;
    const int i = e / 3, ch = e - 3 * i;
    const int x = d.flip ? S - 1 - i : i;
    const float a = ch == 0 ? a0 : (ch == 1 ? a1 : a2), m = ch == 0 ? m0 : (ch == 1 ? m1 : m2);
#pragma unroll
    for (int r = 0; r < IMG_R; ++r) {
      if (r >= nr) break;
      o[(size_t)ch * plane + (size_t)(r0 + r) * S + x] = fmaf(acc[c][r], a, -m);
    }
  }
}

static inline uint64_t image_ws_bytes(const int N) { return (((uint64_t)N * sizeof(ImgDesc)) + 255) & ~(uint64_t)255; }

static LdsGrant g_img_grant3, g_img_grant12;

}  // namespace gic

using namespace gic;

extern "C" {

int gic_image_preprocess_ws_bytes(int32_t N, int32_t S, uint64_t* out) {
  GIC_CHECK_ARG(out, "image_preprocess_ws_bytes: null out");
  GIC_CHECK_ARG(N >= 1, "image_preprocess_ws_bytes: N = %d (need N >= 1)", N);
  GIC_CHECK_ARG(S >= 1 && S <= IMG_MAX_S, "image_preprocess_ws_bytes: S = %d (need 1 .. %d)", S, IMG_MAX_S);
  *out = image_ws_bytes(N);
  return GIC_OK;
}

int gic_image_preprocess(const uint8_t* pixels, uint64_t pixels_bytes, const gic_image_src* src, int32_t N, int32_t S,
                         const float mean[3], const float std[3], float* out_nchw, void* ws, void* stream) {
  GIC_CHECK_ARG(pixels && src && mean && std && out_nchw && ws, "image_preprocess: null argument");
  GIC_CHECK_ARG(N >= 1 && N <= 65535, "image_preprocess: N = %d (need 1 .. 65535)", N);
  GIC_CHECK_ARG(S >= 1 && S <= IMG_MAX_S, "image_preprocess: S = %d (need 1 .. %d)", S, IMG_MAX_S);
  GIC_CHECK_ARG((((uintptr_t)out_nchw) & 15) == 0 && (((uintptr_t)ws) & 15) == 0, "image_preprocess: out / ws not 16-byte aligned");
  float a[3], m[3];
  for (int c = 0; c < 3; ++c) {
    GIC_CHECK_ARG(isfinite(mean[c]) && isfinite(std[c]) && std[c] > 0.f, "image_preprocess: mean[%d] = %g, std[%d] = %g (need finite, std > 0)",
                  c, (double)mean[c], c, (double)std[c]);
    a[c] = (float)(1.0 / (255.0 * (double)std[c]));
    m[c] = (float)((double)mean[c] / (double)std[c]);
  }
  int max_pitch = 0;
  for (int i = 0; i < N; ++i) {
    const gic_image_src& s = src[i];
    GIC_CHECK_ARG(s.height >= 1 && s.height <= IMG_MAX_SIDE && s.width >= 1 && s.width <= IMG_MAX_SIDE,
                  "image_preprocess: image %d is %d x %d (need 1 .. %d per side)", i, s.height, s.width, IMG_MAX_SIDE);
    GIC_CHECK_ARG(s.channels == 1 || s.channels == 3, "image_preprocess: image %d has %d channels (need 1 or 3)", i, s.channels);
    GIC_CHECK_ARG(s.row_stride >= s.width * s.channels, "image_preprocess: image %d row_stride %d < width * channels = %d", i, s.row_stride,
                  s.width * s.channels);
    GIC_CHECK_ARG(s.offset >= 0 && (uint64_t)s.offset <= pixels_bytes &&
                      (uint64_t)s.offset + (uint64_t)(s.height - 1) * (uint64_t)s.row_stride + (uint64_t)(s.width * s.channels) <= pixels_bytes,
                  "image_preprocess: image %d (offset %lld, %d rows of stride %d) reaches past pixels_bytes = %llu", i, (long long)s.offset,
                  s.height, s.row_stride, (unsigned long long)pixels_bytes);
    const float x0 = s.box[0], y0 = s.box[1], x1 = s.box[2], y1 = s.box[3];
    GIC_CHECK_ARG(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1), "image_preprocess: image %d has a non-finite box", i);
    GIC_CHECK_ARG(x0 < x1 && y0 < y1, "image_preprocess: image %d has an empty or reversed box (%g, %g, %g, %g)", i, (double)x0, (double)y0,
                  (double)x1, (double)y1);
    GIC_CHECK_ARG(x0 >= 0.f && y0 >= 0.f && x1 <= (float)s.width && y1 <= (float)s.height,
                  "image_preprocess: image %d box (%g, %g, %g, %g) leaves the %d x %d image", i, (double)x0, (double)y0, (double)x1, (double)y1,
                  s.width, s.height);
    GIC_CHECK_ARG(s.flip == 0 || s.flip == 1, "image_preprocess: image %d flip = %d (need 0 or 1)", i, s.flip);
  }
  // nothing above touched the GPU; from here on every descriptor is in range
  const hipStream_t st = (hipStream_t)stream;
  ImgDesc* dev = (ImgDesc*)ws;
  for (int base = 0; base < N; base += IMG_STAGE_DESCS) {
    ImgDescPack pack;
    const int cnt = N - base < IMG_STAGE_DESCS ? N - base : IMG_STAGE_DESCS;
    for (int j = 0; j < IMG_STAGE_DESCS; ++j) {
      const gic_image_src& s = src[base + (j < cnt ? j : 0)];
      ImgDesc& d = pack.d[j];
      d.offset = s.offset;
      d.H = s.height; d.W = s.width; d.C = s.channels; d.stride = s.row_stride;
      for (int k = 0; k < 4; ++k) d.box[k] = s.box[k];
      d.flip = s.flip;
      int f0, l0, f1, l1;
      double c, fs;
      axis_taps((double)s.box[0], (double)s.box[2], S, 0, 0, s.width, f0, l0, c, fs);
      axis_taps((double)s.box[0], (double)s.box[2], S, S - 1, 0, s.width, f1, l1, c, fs);
      d.x_lo = f0;
      d.x_hi = l1 > f0 ? l1 : f0 + 1;
      d.pad = 0;
      const int pitch = ((d.x_hi - d.x_lo) * d.C + 3 + 3) & ~3;
      if (j < cnt && pitch > max_pitch) max_pitch = pitch;
    }
    hipLaunchKernelGGL(image_stage_descs_kernel, dim3(1), dim3(IMG_STAGE_DESCS), 0, st, dev + base, pack, cnt);
    GIC_CHECK_LAUNCH("image_preprocess (descriptors)");
  }
  int stage = max_pitch;
  if (stage < IMG_STAGE_MIN) stage = (8 * max_pitch < IMG_STAGE_MIN) ? 8 * max_pitch : IMG_STAGE_MIN / max_pitch * max_pitch;
  stage = (stage + 15) & ~15;
  const size_t lds = (size_t)S * sizeof(ColTap) + (size_t)stage;
  const int dwords_ok = (((uintptr_t)pixels) & 3) == 0;
  const dim3 grid((S + IMG_R - 1) / IMG_R, N);
  if (S <= IMG_THREADS) {
    if (!grant_lds(image_preprocess_kernel<3>, lds, g_img_grant3)) {
      set_last_error("image_preprocess: %zu bytes of LDS refused", lds);
      return GIC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(image_preprocess_kernel<3>, grid, dim3(IMG_THREADS), lds, st, pixels, pixels_bytes, dev, S, a[0], a[1], a[2], m[0],
                       m[1], m[2], out_nchw, stage, dwords_ok);
  } else {
    if (!grant_lds(image_preprocess_kernel<12>, lds, g_img_grant12)) {
      set_last_error("image_preprocess: %zu bytes of LDS refused", lds);
      return GIC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(image_preprocess_kernel<12>, grid, dim3(IMG_THREADS), lds, st, pixels, pixels_bytes, dev, S, a[0], a[1], a[2], m[0],
                       m[1], m[2], out_nchw, stage, dwords_ok);
  }
  GIC_CHECK_LAUNCH("image_preprocess");
  return GIC_OK;
}

}  // extern "C"
