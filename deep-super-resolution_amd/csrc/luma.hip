// Y-channel PSNR / SSIM with a border shave: the protocol every published SRGAN / ESRGAN / EDSR table is measured by
// (metrics.LumaPeakSignalNoiseRatio, metrics.LumaStructuralSimilarityIndexMeasure, metrics.rgb_to_y).  PARITY UNPINNED:
// neither basicsr nor MATLAB is at hand; the definitions below restate what they document.
//   q(x)      = rintf(fminf(fmaxf(x, 0), 1) * 255.0f) / 255 when `quantize` (one fp32 multiply, round half to even: the
//               integer evaluate.to_uint8_image writes into a PNG), else x
//   Y(r,g,b)  = (16 + 65.481 r + 128.553 g + 24.966 b) / 255          BT.601 luma of MATLAB's rgb2ycbcr, unit scale
//   region    = rows [s, H-s), columns [s, W-s), s = shave >= 0
// Inputs are [N,3,H,W] in fp32, fp16 or bf16, read as they are (no fp32 copy); the arithmetic is fp32.
//
// The squared error is formed from the CHANNEL differences, dY = (65.481 dr + 128.553 dg + 24.966 db) / 255 with
// d. = q(p.) - q(t.), never as Y(p) - Y(t): two lumas of ~0.4 carry an absolute rounding error of ~3e-8 each, which is 1e-2
// of the dY of a one-step change of one channel (2e-3 / 255) -- and PSNR of near-identical images is exactly where the
// protocol is used.  With `quantize` the channel differences are taken between the two integers (exact in fp32) and the
// second / 255 goes into the constant.
//
// One thread per cropped pixel, consecutive lanes on consecutive columns: a shaved row starts at any element and W - 2s is odd
// in general, so the loads are one element per lane (dword for fp32, 2 bytes for the 16-bit types) -- coalesced within a row,
// nothing to align.  A block owns LUMA_CHUNK consecutive cropped pixels of one image and stores one partial sum; partials are
// folded per image in a fixed order, in double, by a one-block launch: no atomics, the same bits on every run.
#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define LUMA_CHUNK 4096          // cropped pixels per block: 16 per thread
#define LUMA_WIN 11              // the SSIM window the luma pair feeds

template <int D>
__device__ __forceinline__ float luma_load(const void* __restrict__ p, size_t i) {
  if constexpr (D == DSR_F32) {
    return reinterpret_cast<const float*>(p)[i];
  } else {
    return h2f<D>(reinterpret_cast<const unsigned short*>(p)[i]);
  }
}

// the 8-bit code of x as a float (0 .. 255), or x itself
__device__ __forceinline__ float luma_level(float x, int quantize) {
  return quantize ? rintf(fminf(fmaxf(x, 0.f), 1.f) * 255.0f) : x;
}

// 65.481 r + 128.553 g + 24.966 b (of levels, unit values or their differences)
__device__ __forceinline__ float luma_dot(float r, float g, float b) {
  return fmaf(24.966f, b, fmaf(128.553f, g, 65.481f * r));
}

// Y in unit scale from levels (quantize) or unit values
__device__ __forceinline__ float luma_y(float r, float g, float b, int quantize) {
  float t = luma_dot(r, g, b);
  if (quantize) t = t / 255.0f;
  return (16.0f + t) / 255.0f;
}

// PAIR: reads p and t; writes yp / yt (both or neither) and, if partial != null, the block's sum of dY^2.
// !PAIR: reads p, writes yp.
template <int DP, int DT, bool PAIR>
__global__ __launch_bounds__(256) void luma_kernel(const void* __restrict__ p, const void* __restrict__ t, int H, int W, int s,
                                                   int w, unsigned hw, int B, int quantize, float* __restrict__ yp,
                                                   float* __restrict__ yt, float* __restrict__ partial) {
  __shared__ float red[4];
  const int n = blockIdx.x / B, blk = blockIdx.x % B;
  const size_t plane = (size_t)H * W;
  const size_t img = (size_t)n * 3 * plane;
  const float inv = quantize ? 1.0f / (255.0f * 255.0f) : 1.0f / 255.0f;
  float acc = 0.f;
#pragma unroll 4
  for (int k = 0; k < LUMA_CHUNK / 256; ++k) {
    const unsigned i = (unsigned)blk * LUMA_CHUNK + k * 256 + threadIdx.x;
    if (i < hw) {
      const unsigned y = i / (unsigned)w, x = i - y * (unsigned)w;
      const size_t o = img + (size_t)(y + s) * W + (x + s);
      const float pr = luma_level(luma_load<DP>(p, o), quantize);
      const float pg = luma_level(luma_load<DP>(p, o + plane), quantize);
      const float pb = luma_level(luma_load<DP>(p, o + 2 * plane), quantize);
      if (yp) yp[(size_t)n * hw + i] = luma_y(pr, pg, pb, quantize);
      if constexpr (PAIR) {
        const float tr = luma_level(luma_load<DT>(t, o), quantize);
        const float tg = luma_level(luma_load<DT>(t, o + plane), quantize);
        const float tb = luma_level(luma_load<DT>(t, o + 2 * plane), quantize);
        if (yt) yt[(size_t)n * hw + i] = luma_y(tr, tg, tb, quantize);
        const float d = luma_dot(pr - tr, pg - tg, pb - tb) * inv;
        acc = fmaf(d, d, acc);
      }
    }
  }
  if constexpr (PAIR) {
    if (partial) {                      // uniform over the grid
      acc = wave_sum(acc);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
      __syncthreads();
      if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
  }
}

// per_image[n] = 10 log10(count / SSE_n) (+inf when SSE_n == 0), SSE_n = the B partials of image n folded in a fixed order in
// double; value = value_scale * sum_n per_image[n]; state[0] += sum_n per_image[n], state[1] += N (dsr_metric_accumulate's pair)
__global__ __launch_bounds__(1024) void luma_psnr_finalize_kernel(const float* __restrict__ partial, int N, int B, double count,
                                                                  float* __restrict__ per_image, float* __restrict__ value,
                                                                  float value_scale, double* __restrict__ state) {
  __shared__ double wsum[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double mine = 0.0;
  for (int n = wave; n < N; n += 16) {
    double sse = 0.0;
    for (int k = lane; k < B; k += 64) sse += (double)partial[(size_t)n * B + k];
    sse = wave_sum(sse);
    const double v = sse > 0.0 ? 10.0 * log10(count / sse) : (double)INFINITY;
    if (lane == 0 && per_image) per_image[n] = (float)v;
    mine += v;
  }
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double acc = 0.0;
  for (int k = 0; k < 16; ++k) acc += wsum[k];
  if (value) value[0] = (float)((double)value_scale * acc);
  if (state) {
    state[0] += acc;
    state[1] += (double)N;
  }
}

// ---- host side
static bool luma_dtype_ok(int dt) { return dt == DSR_BF16 || dt == DSR_F16 || dt == DSR_F32; }

// the cropped size, or an error; min_side: 1 (PSNR, rgb_to_y) or 11 (the planes feed SSIM)
static int luma_region(const char* who, int N, int C, int H, int W, int shave, int min_side, int* h, int* w) {
  DSR_REQUIRE(N >= 1, "%s: %d images", who, N);
  DSR_REQUIRE(C == 3, "%s: %d channels, RGB needs 3", who, C);
  DSR_REQUIRE(H >= 1 && W >= 1, "%s: image %dx%d", who, H, W);
  DSR_REQUIRE(shave >= 0, "%s: shave %d is negative", who, shave);
  DSR_REQUIRE((long long)H - 2ll * shave >= min_side && (long long)W - 2ll * shave >= min_side,
              "%s: shave %d leaves less than %dx%d of a %dx%d image", who, shave, min_side, min_side, H, W);
  *h = H - 2 * shave;
  *w = W - 2 * shave;
  DSR_REQUIRE((long long)*h * *w < (1ll << 31), "%s: more than 2^31 pixels per image", who);
  return 0;
}

static long long luma_blocks_per_image(int h, int w) { return ((long long)h * w + LUMA_CHUNK - 1) / LUMA_CHUNK; }

extern "C" int dsr_luma_blocks(int N, int H, int W, int shave) {
  if (N < 1 || H < 1 || W < 1 || shave < 0 || (long long)H - 2ll * shave < 1 || (long long)W - 2ll * shave < 1) return 0;
  const int h = H - 2 * shave, w = W - 2 * shave;
  if ((long long)h * w >= (1ll << 31)) return 0;
  const long long b = (long long)N * luma_blocks_per_image(h, w);
  return b < (1ll << 31) ? (int)b : 0;
}

template <int DP, bool PAIR>
static void luma_launch_t(int dt_t, int blocks, dsr_stream_t st, const void* p, const void* t, int H, int W, int s, int w,
                          unsigned hw, int B, int quantize, float* yp, float* yt, float* partial) {
#define LUMA_GO(DT)                                                                                                          \
  hipLaunchKernelGGL((luma_kernel<DP, DT, PAIR>), dim3(blocks), dim3(256), 0, st, p, t, H, W, s, w, hw, B, quantize, yp, yt, \
                     partial)
  if constexpr (!PAIR) {
    LUMA_GO(DSR_F32);                   // no second image: its type is not instantiated over
  } else {
    if (dt_t == DSR_F32)
      LUMA_GO(DSR_F32);
    else if (dt_t == DSR_F16)
      LUMA_GO(DSR_F16);
    else
      LUMA_GO(DSR_BF16);
  }
#undef LUMA_GO
}

template <bool PAIR>
static void luma_launch(int dt_p, int dt_t, int blocks, dsr_stream_t st, const void* p, const void* t, int H, int W, int s,
                        int w, unsigned hw, int B, int quantize, float* yp, float* yt, float* partial) {
  if (dt_p == DSR_F32)
    luma_launch_t<DSR_F32, PAIR>(dt_t, blocks, st, p, t, H, W, s, w, hw, B, quantize, yp, yt, partial);
  else if (dt_p == DSR_F16)
    luma_launch_t<DSR_F16, PAIR>(dt_t, blocks, st, p, t, H, W, s, w, hw, B, quantize, yp, yt, partial);
  else
    luma_launch_t<DSR_BF16, PAIR>(dt_t, blocks, st, p, t, H, W, s, w, hw, B, quantize, yp, yt, partial);
}

extern "C" int dsr_luma_sse_stats(int dtype_preds, const void* preds, int dtype_target, const void* target, int N, int C, int H,
                                  int W, int shave, int quantize, float* partial_sse, dsr_stream_t st) {
  DSR_REQUIRE(preds && target && partial_sse, "luma_sse_stats: null pointer");
  DSR_REQUIRE(luma_dtype_ok(dtype_preds) && luma_dtype_ok(dtype_target), "luma_sse_stats: dtype %d / %d (0 bf16, 1 f16, 2 f32)",
              dtype_preds, dtype_target);
  int h, w;
  const int rc = luma_region("luma_sse_stats", N, C, H, W, shave, 1, &h, &w);
  if (rc) return rc;
  const int blocks = dsr_luma_blocks(N, H, W, shave);
  DSR_REQUIRE(blocks > 0, "luma_sse_stats: too many pixels for one launch");
  luma_launch<true>(dtype_preds, dtype_target, blocks, st, preds, target, H, W, shave, w, (unsigned)h * (unsigned)w, blocks / N,
                    quantize ? 1 : 0, nullptr, nullptr, partial_sse);
  return dsr_launch_status("dsr_luma_sse_stats");
}

extern "C" int dsr_luma_pair(int dtype_preds, const void* preds, int dtype_target, const void* target, int N, int C, int H, int W,
                             int shave, int quantize, float* y_preds, float* y_target, float* partial_sse, dsr_stream_t st) {
  DSR_REQUIRE(preds && target && y_preds && y_target, "luma_pair: null pointer");
  DSR_REQUIRE(luma_dtype_ok(dtype_preds) && luma_dtype_ok(dtype_target), "luma_pair: dtype %d / %d (0 bf16, 1 f16, 2 f32)",
              dtype_preds, dtype_target);
  int h, w;
  const int rc = luma_region("luma_pair", N, C, H, W, shave, LUMA_WIN, &h, &w);
  if (rc) return rc;
  const int blocks = dsr_luma_blocks(N, H, W, shave);
  DSR_REQUIRE(blocks > 0, "luma_pair: too many pixels for one launch");
  luma_launch<true>(dtype_preds, dtype_target, blocks, st, preds, target, H, W, shave, w, (unsigned)h * (unsigned)w, blocks / N,
                    quantize ? 1 : 0, y_preds, y_target, partial_sse);
  return dsr_launch_status("dsr_luma_pair");
}

extern "C" int dsr_rgb_to_y(int dtype, const void* x, int N, int C, int H, int W, int shave, int quantize, float* y,
                            dsr_stream_t st) {
  DSR_REQUIRE(x && y, "rgb_to_y: null pointer");
  DSR_REQUIRE(luma_dtype_ok(dtype), "rgb_to_y: dtype %d (0 bf16, 1 f16, 2 f32)", dtype);
  int h, w;
  const int rc = luma_region("rgb_to_y", N, C, H, W, shave, 1, &h, &w);
  if (rc) return rc;
  const int blocks = dsr_luma_blocks(N, H, W, shave);
  DSR_REQUIRE(blocks > 0, "rgb_to_y: too many pixels for one launch");
  luma_launch<false>(dtype, DSR_F32, blocks, st, x, nullptr, H, W, shave, w, (unsigned)h * (unsigned)w, blocks / N,
                     quantize ? 1 : 0, y, nullptr, nullptr);
  return dsr_launch_status("dsr_rgb_to_y");
}

extern "C" int dsr_luma_psnr_finalize(const float* partial_sse, int N, int H, int W, int shave, float* per_image, float* value,
                                      float value_scale, double* state, dsr_stream_t st) {
  DSR_REQUIRE(partial_sse, "luma_psnr_finalize: null pointer");
  DSR_REQUIRE(per_image || value || state, "luma_psnr_finalize: neither per-image values, a value nor a state are asked for");
  int h, w;
  const int rc = luma_region("luma_psnr_finalize", N, 3, H, W, shave, 1, &h, &w);
  if (rc) return rc;
  const int blocks = dsr_luma_blocks(N, H, W, shave);
  DSR_REQUIRE(blocks > 0, "luma_psnr_finalize: too many pixels for one launch");
  hipLaunchKernelGGL(luma_psnr_finalize_kernel, dim3(1), dim3(1024), 0, st, partial_sse, N, blocks / N, (double)h * (double)w,
                     per_image, value, value_scale, state);
  return dsr_launch_status("dsr_luma_psnr_finalize");
}
