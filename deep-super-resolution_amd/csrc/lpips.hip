// LPIPS (Zhang, Isola, Efros, Shechtman, Wang 2018) with the AlexNet trunk, as the reference's scripts log it: torchmetrics
// LearnedPerceptualImagePatchSimilarity(net_type='alex') at train_GAN.py:32,112, eval_GAN.py:32,49, DIP.py:75,159,185.
// torchmetrics and lpips are not installed here: "parity unpinned"; lpips.py restates the definition and the tests compare
// against a float64 restatement built from torch.nn.functional.
//
// The five convolutions run on dsr_conv_fwd (bias + ReLU epilogue).  This file holds the rest of the path:
//   * stem preparation: scaling layer + zero padding 2 + 4x4 space-to-depth of BOTH images into one [2N][BH][BW][64] 16-bit
//     NHWC tensor (48 channels + 16 zero channels), so that the 11x11 / stride-4 stem is an exact 3x3 / stride-1 / pad-0 conv
//     over 64 channels (its weight: the 11x11 kernel zero-padded to 12x12 and regrouped on the host, lpips.py).  64 rather
//     than 48 channels: the gather kernels' fast path wants whole 64-channel K slices (dsr_conv_gemm_fast); with 48 the
//     launch falls back to the per-element loader.
//     The same pass folds min / max of the raw inputs into a 2-word range buffer (order-preserving integer keys, one atomic
//     per wave and word, grid capped), which the host reads once to reject values outside the accepted range.
//   * MaxPool2d(3, stride 2), floor mode, forward only, on 16-byte channel vectors.
//   * the distance: per pixel the two channel norms (torchmetrics' form f / sqrt(eps + sum f^2), eps = 1e-8), then
//     sum_c w[c] * (n1 - n2)^2 -- the difference is taken after both norms are known, so identical inputs give exactly 0 and
//     swapping the images changes nothing -- one partial sum per block for all five taps in one launch, then one finalise
//     launch (per-tap 1/(h*w), sum over taps, batch mean or sum).  Deterministic: no float atomics.
//
// The backward (LPIPS as a training loss) runs the five input gradients on dsr_conv_dgrad / dsr_conv_dgrad_masked and adds three
// streaming passes, all gather form (no atomics, deterministic), 16-bit gradients carrying the caller's static loss scale:
//   * dsr_lpips_distance_bwd: the closed-form derivative of the distance for all five taps in one launch, times the ReLU mask
//     of the tap, for the image-1 half, the image-2 half or both.
//   * dsr_maxpool3s2_bwd: each 2x2 block of input pixels recomputes the arg-max of the four windows that touch it (torch's
//     tie rule: row-major scan, first maximum), sums the dy it wins in fp32, applies the ReLU mask of the pool's input and adds
//     the distance part of that tap: relu1 / relu2 get their whole gradient in one pass.
//   * dsr_lpips_stem_prep_bwd: 16-bit gradient of the space-to-depth stem input -> fp32 NCHW image gradient.
#include <string.h>

#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define LPIPS_S2D_CP 64        // channels of the stem input: 4 x 4 x 3 = 48 real, 16 zero
#define LPIPS_MAX_TAPS 5
#define LPIPS_PIX_PER_BLOCK 256
#define LPIPS_MAXV 6           // 16-byte channel vectors per lane and image in the distance kernel: Cp <= 8 lanes x 6 x 8 = 384
#define LPIPS_GRID_CAP 4096

#define LPIPS_DT_SWITCH(dtype, CALL)     \
  if ((dtype) == DSR_BF16) {             \
    constexpr int DT = DSR_DTYPE_BF16;   \
    CALL;                                \
  } else {                               \
    constexpr int DT = DSR_DTYPE_F16;    \
    CALL;                                \
  }

static inline unsigned lp_grid(size_t n) {
  const size_t b = (n + 255) / 256;
  return (unsigned)(b < LPIPS_GRID_CAP ? (b > 0 ? b : 1) : LPIPS_GRID_CAP);
}

// ---------------------------------------------------------------------------------------------------- stem preparation
template <int DT>
__global__ __launch_bounds__(256) void lpips_stem_prep_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                              int N, int H, int W, int BH, int BW, int normalize,
                                                              unsigned short* __restrict__ out, unsigned* __restrict__ range) {
  const size_t total = (size_t)2 * N * BH * BW * (LPIPS_S2D_CP / 8);
  unsigned kmin = 0xffffffffu, kmax = 0u;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int q = (int)(idx & 7);                       // 8-channel vector of the pixel
    const size_t pix = idx >> 3;
    const int bx = (int)(pix % BW);
    const int by = (int)((pix / BW) % BH);
    const int n2 = (int)(pix / ((size_t)BW * BH));
    const float* img = n2 < N ? img1 + (size_t)n2 * 3 * H * W : img2 + (size_t)(n2 - N) * 3 * H * W;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = q * 8 + j;                          // channel k = (py * 4 + px) * 3 + c
      float r = 0.f;
      if (k < 48) {
        const int t = k / 3, c = k - 3 * t;
        const int y = 4 * by + (t >> 2) - 2, x = 4 * bx + (t & 3) - 2;      // padded coordinate - 2 = image coordinate
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
          const float raw = img[((size_t)c * H + y) * W + x];
          const unsigned key = order_key(raw);           // a NaN lands outside [-inf, +inf], so it fails the range test
          kmin = key < kmin ? key : kmin;
          kmax = key > kmax ? key : kmax;
          // the scaling layer: (x - shift) / scale, shift (-.030, -.088, -.188), scale (.458, .448, .450)
          const float sh = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
          const float sc = c == 0 ? .458f : (c == 1 ? .448f : .450f);
          const float xin = normalize ? 2.f * raw - 1.f : raw;
          r = (xin - sh) / sc;
        }
      }
      v[j] = r;
    }
    *reinterpret_cast<U4*>(out + idx * 8) = pack8<DT>(v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned a = __shfl_xor(kmin, o, 64), b = __shfl_xor(kmax, o, 64);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(range, kmin);
    atomicMax(range + 1, kmax);
  }
}

static int lpips_sizes(int H, int W, int* hw) {
  // conv1 11x11/4 pad 2 -> pool 3/2 -> conv2 5x5 pad 2 -> pool 3/2 -> conv3..5 3x3 pad 1
  const int s[2] = {H, W};
  for (int d = 0; d < 2; ++d) {
    const int c1 = s[d] + 4 >= 11 ? (s[d] + 4 - 11) / 4 + 1 : 0;
    const int p1 = c1 >= 3 ? (c1 - 3) / 2 + 1 : 0;
    const int p2 = p1 >= 3 ? (p1 - 3) / 2 + 1 : 0;
    if (p2 < 1)
      return dsr_fail(DSR_E_ARG, "lpips: a %dx%d image is too small for the AlexNet trunk (its second max-pool output would be empty)",
                      H, W);
    hw[0 + d] = c1;
    hw[2 + d] = p1;
    hw[4 + d] = hw[6 + d] = hw[8 + d] = p2;
  }
  return DSR_OK;
}

extern "C" int dsr_lpips_tap_sizes(int H, int W, int* hw) {
  DSR_REQUIRE(hw, "lpips_tap_sizes: null output");
  DSR_REQUIRE(H > 0 && W > 0, "lpips_tap_sizes: empty image %dx%d", H, W);
  return lpips_sizes(H, W, hw);
}

extern "C" int dsr_lpips_stem_prep(int dtype, const float* img1, const float* img2, int N, int H, int W, int normalize, void* out,
                                   unsigned* range, dsr_stream_t st) {
  DSR_REQUIRE(img1 && img2 && out && range && DSR_DTYPE_OK(dtype), "lpips_stem_prep: null pointer or bad dtype");
  DSR_REQUIRE(N > 0 && H > 0 && W > 0, "lpips_stem_prep: empty batch or image");
  int hw[10];
  const int rc = lpips_sizes(H, W, hw);
  if (rc) return rc;
  const int BH = hw[0] + 2, BW = hw[1] + 2;             // a 3x3 stride-1 valid conv over the blocks gives the 11x11/4 output
  DSR_REQUIRE((long long)2 * N * BH * BW * LPIPS_S2D_CP * 2 < (1ll << 31),
              "lpips_stem_prep: output of 2 GiB or more (%d image pairs of %dx%d): split the batch", N, H, W);
  const size_t total = (size_t)2 * N * BH * BW * (LPIPS_S2D_CP / 8);
  LPIPS_DT_SWITCH(dtype, hipLaunchKernelGGL((lpips_stem_prep_kernel<DT>), dim3(lp_grid(total)), dim3(256), 0, st, img1, img2, N, H,
                                            W, BH, BW, normalize ? 1 : 0, (unsigned short*)out, range));
  return dsr_launch_status("dsr_lpips_stem_prep");
}

// The inverse gather of lpips_stem_prep_kernel: image pixel (c, y, x) sits at channel ((y+2)%4 * 4 + (x+2)%4) * 3 + c of block
// ((y+2)/4, (x+2)/4); padding rows / columns and channels 48..63 have no image pixel and are dropped.  One lane per pixel and
// its three channels (three neighbouring 16-bit values), stores coalesced along x in each of the three planes.
template <int DT>
__global__ __launch_bounds__(256) void lpips_stem_prep_bwd_kernel(const unsigned short* __restrict__ dx, int N, int H, int W, int BH,
                                                                  int BW, float m0, float m1, float m2, float* __restrict__ dimg) {
  const size_t total = (size_t)N * H * W;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int x = (int)(idx % W);
    const int y = (int)((idx / W) % H);
    const size_t n = idx / ((size_t)W * H);
    const int by = (y + 2) >> 2, bx = (x + 2) >> 2;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (by < BH && bx < BW) {                             // (a padded pixel past the last block never reached the stem)
      const unsigned short* p = dx + ((n * BH + by) * BW + bx) * LPIPS_S2D_CP + ((((y + 2) & 3) << 2) + ((x + 2) & 3)) * 3;
      g0 = h2f<DT>(p[0]) * m0;
      g1 = h2f<DT>(p[1]) * m1;
      g2 = h2f<DT>(p[2]) * m2;
    }
    float* o = dimg + (n * 3 * H + y) * W + x;
    o[0] = g0;
    o[(size_t)H * W] = g1;
    o[(size_t)2 * H * W] = g2;
  }
}

extern "C" int dsr_lpips_stem_prep_bwd(int dtype, const void* dx, int N, int H, int W, int normalize, float scale, float* dimg,
                                       dsr_stream_t st) {
  DSR_REQUIRE(dx && dimg && DSR_DTYPE_OK(dtype), "lpips_stem_prep_bwd: null pointer or bad dtype");
  DSR_REQUIRE(N > 0 && H > 0 && W > 0, "lpips_stem_prep_bwd: empty batch or image");
  DSR_REQUIRE(scale > 0.f && scale < INFINITY, "lpips_stem_prep_bwd: the loss scale must be positive and finite");
  int hw[10];
  const int rc = lpips_sizes(H, W, hw);
  if (rc) return rc;
  const int BH = hw[0] + 2, BW = hw[1] + 2;
  if ((long long)N * BH * BW * LPIPS_S2D_CP * 2 >= (1ll << 31) || (long long)N * 3 * H * W * 4 >= (1ll << 31))
    return dsr_fail(DSR_E_UNSUPPORTED, "lpips_stem_prep_bwd: tensor of 2 GiB or more (%d images of %dx%d): split the batch", N, H, W);
  // d/d raw of ((2 raw - 1 | raw) - shift) / scale_c, and the static loss scale taken out again
  const double k = (normalize ? 2.0 : 1.0) / (double)scale;
  const size_t total = (size_t)N * H * W;
  LPIPS_DT_SWITCH(dtype, hipLaunchKernelGGL((lpips_stem_prep_bwd_kernel<DT>), dim3(lp_grid(total)), dim3(256), 0, st,
                                            (const unsigned short*)dx, N, H, W, BH, BW, (float)(k / .458), (float)(k / .448),
                                            (float)(k / .450), dimg));
  return dsr_launch_status("dsr_lpips_stem_prep_bwd");
}

// ---------------------------------------------------------------------------------------------------- MaxPool2d(3, 2)
template <int DT>
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                             int N, int H, int W, int Cp, int OH, int OW) {
  const int cpr = Cp / 8;
  const size_t total = (size_t)N * OH * OW * cpr;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int ch = (int)(idx % cpr);
    const size_t pix = idx / cpr;
    const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), n = (int)(pix / ((size_t)OW * OH));
    float m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = -INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float f[8];
        unpack8<DT>(*reinterpret_cast<const U4*>(x + (((size_t)n * H + 2 * oy + i) * W + 2 * ox + j) * Cp + ch * 8), f);
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = (f[k] > m[k] || f[k] != f[k]) ? f[k] : m[k];    // a NaN propagates, as in torch
      }
    *reinterpret_cast<U4*>(y + pix * Cp + ch * 8) = pack8<DT>(m);
  }
}

extern "C" int dsr_maxpool3s2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int Cp, dsr_stream_t st) {
  DSR_REQUIRE(x && y && DSR_DTYPE_OK(dtype) && N > 0 && H > 0 && W > 0 && Cp >= 8 && Cp % 8 == 0,
              "maxpool3s2_fwd: null pointer or bad shape");
  DSR_REQUIRE(H >= 3 && W >= 3, "maxpool3s2_fwd: a %dx%d input is smaller than the 3x3 window (empty output)", H, W);
  const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
  const size_t total = (size_t)N * OH * OW * (Cp / 8);
  LPIPS_DT_SWITCH(dtype, hipLaunchKernelGGL((maxpool3s2_fwd_kernel<DT>), dim3(lp_grid(total)), dim3(256), 0, st,
                                            (const unsigned short*)x, (unsigned short*)y, N, H, W, Cp, OH, OW));
  return dsr_launch_status("dsr_maxpool3s2_fwd");
}

// One lane = a 2x2 block of input pixels (rows 2a, 2a+1, columns 2b, 2b+1) x 8 channels.  The windows that contain one of them
// are (a-1 | a, b-1 | b); window (a, b) holds all four (positions 0, 1, 3, 4 of its row-major scan), (a-1, b) the upper two
// (6, 7), (a, b-1) the left two (2, 5) and (a-1, b-1) the corner (8).  A window's arg-max is torch's: row-major scan, a value
// replaces the running maximum if it is greater or NaN, so the first of equal maxima keeps the gradient.
template <int DT>
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
                                                             const unsigned short* __restrict__ addend, unsigned short* __restrict__ dx,
                                                             int N, int H, int W, int Cp, int OH, int OW, int relu_mask) {
  const int cpr = Cp / 8, AH = (H + 1) / 2, AW = (W + 1) / 2;
  const size_t total = (size_t)N * AH * AW * cpr;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int ch = (int)(idx % cpr);
    const size_t blk = idx / cpr;
    const int b = (int)(blk % AW), a = (int)((blk / AW) % AH);
    const size_t n = blk / ((size_t)AW * AH);
    float acc[4][8];                                    // pixel (2a + (q >> 1), 2b + (q & 1))
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[q][k] = 0.f;
#pragma unroll
    for (int wy = 0; wy < 2; ++wy)
#pragma unroll
      for (int wx = 0; wx < 2; ++wx) {
        const int oy = a - 1 + wy, ox = b - 1 + wx;
        if (oy < 0 || ox < 0 || oy >= OH || ox >= OW) continue;
        float m[8];
        int am[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          m[k] = -INFINITY;
          am[k] = 0;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {                 // (rows 2oy .. 2oy+2 <= H-1 by the definition of OH: always inside x)
            float f[8];
            unpack8<DT>(*reinterpret_cast<const U4*>(x + ((n * H + 2 * oy + i) * W + 2 * ox + j) * Cp + ch * 8), f);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const bool take = f[k] > m[k] || f[k] != f[k];
              m[k] = take ? f[k] : m[k];
              am[k] = take ? i * 3 + j : am[k];
            }
          }
        float g[8];
        unpack8<DT>(*reinterpret_cast<const U4*>(dy + ((n * OH + oy) * OW + ox) * Cp + ch * 8), g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // position of block pixel q in this window, -1 if outside: row 2a + qy - 2oy = qy + 2 (1 - wy), likewise the column
          const int ry = (q >> 1) + 2 * (1 - wy), rx = (q & 1) + 2 * (1 - wx);
          if (ry > 2 || rx > 2) continue;               // (compile-time after unrolling)
          const int pos = ry * 3 + rx;
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[q][k] += am[k] == pos ? g[k] : 0.f;
        }
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int iy = 2 * a + (q >> 1), ix = 2 * b + (q & 1);
      if (iy >= H || ix >= W) continue;
      const size_t off = ((n * H + iy) * W + ix) * Cp + ch * 8;
      if (relu_mask) {
        float f[8];
        unpack8<DT>(*reinterpret_cast<const U4*>(x + off), f);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[q][k] = f[k] > 0.f ? acc[q][k] : 0.f;
      }
      if (addend) {
        float e[8];
        unpack8<DT>(*reinterpret_cast<const U4*>(addend + off), e);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[q][k] += e[k];
      }
      *reinterpret_cast<U4*>(dx + off) = pack8<DT>(acc[q]);
    }
  }
}

extern "C" int dsr_maxpool3s2_bwd(int dtype, const void* x, const void* dy, const void* addend, void* dx, int N, int H, int W, int Cp,
                                  int relu_mask, dsr_stream_t st) {
  DSR_REQUIRE(x && dy && dx && DSR_DTYPE_OK(dtype) && N > 0 && H > 0 && W > 0 && Cp >= 8 && Cp % 8 == 0,
              "maxpool3s2_bwd: null pointer or bad shape");
  DSR_REQUIRE(H >= 3 && W >= 3, "maxpool3s2_bwd: a %dx%d input is smaller than the 3x3 window (empty output)", H, W);
  if ((long long)N * H * W * Cp * 2 >= (1ll << 31))
    return dsr_fail(DSR_E_UNSUPPORTED, "maxpool3s2_bwd: tensor of 2 GiB or more: split the batch");
  const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
  const size_t total = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (Cp / 8);
  LPIPS_DT_SWITCH(dtype, hipLaunchKernelGGL((maxpool3s2_bwd_kernel<DT>), dim3(lp_grid(total)), dim3(256), 0, st,
                                            (const unsigned short*)x, (const unsigned short*)dy, (const unsigned short*)addend,
                                            (unsigned short*)dx, N, H, W, Cp, OH, OW, relu_mask ? 1 : 0));
  return dsr_launch_status("dsr_maxpool3s2_bwd");
}

// ---------------------------------------------------------------------------------------------------- distance
struct LpipsTap {
  const unsigned short* f;   // [2N][hw][Cp]: images 0..N-1 against N..2N-1
  const float* w;            // [C] lin weights
  int hw, Cp, C;
  int blk0, nblk;            // first block of the tap, blocks per image
};
struct LpipsTaps {
  LpipsTap t[LPIPS_MAX_TAPS];
  int ntaps, N;
};

// block table of a launch; returns the block count, or -1 if it does not fit an int
static int lpips_table(LpipsTaps& a, int ntaps, const int* hw, int N) {
  memset(&a, 0, sizeof(a));
  a.ntaps = ntaps;
  a.N = N;
  long long blk = 0;
  for (int i = 0; i < ntaps; ++i) {
    a.t[i].hw = hw[i];
    a.t[i].blk0 = (int)blk;
    a.t[i].nblk = (hw[i] + LPIPS_PIX_PER_BLOCK - 1) / LPIPS_PIX_PER_BLOCK;
    blk += (long long)N * a.t[i].nblk;
    if (blk >= (1ll << 30)) return -1;
  }
  return (int)blk;
}

// One block = LPIPS_PIX_PER_BLOCK pixels of one image of one tap; 8 lanes per pixel, lane j holds channel vectors j, j+8, ...
template <int DT>
__global__ __launch_bounds__(256) void lpips_distance_kernel(LpipsTaps a, float* __restrict__ partial) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  LpipsTap tp = a.t[0];
#pragma unroll
  for (int i = 1; i < LPIPS_MAX_TAPS; ++i)
    if (i < a.ntaps && b >= a.t[i].blk0) tp = a.t[i];
  const int local = b - tp.blk0;
  const int n = local / tp.nblk, chunk = local - n * tp.nblk;
  const int g = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int nv = tp.Cp / 8;
  const unsigned short* f1 = tp.f + (size_t)n * tp.hw * tp.Cp;
  const unsigned short* f2 = tp.f + (size_t)(n + a.N) * tp.hw * tp.Cp;
  float acc = 0.f;
  for (int it = 0; it < LPIPS_PIX_PER_BLOCK / 32; ++it) {
    const int p = chunk * LPIPS_PIX_PER_BLOCK + it * 32 + g;
    const bool ok = p < tp.hw;                          // uniform over the 8 lanes of a pixel
    U4 va[LPIPS_MAXV], vb[LPIPS_MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < LPIPS_MAXV; ++i) {
      const int v = j + 8 * i;
      const bool in = ok && v < nv;
      const size_t off = in ? (size_t)p * tp.Cp + v * 8 : 0;
      va[i] = load16_or_zero(f1, off, in);
      vb[i] = load16_or_zero(f2, off, in);
      float x1[8], x2[8];
      unpack8<DT>(va[i], x1);
      unpack8<DT>(vb[i], x2);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s1 += x1[k] * x1[k];
        s2 += x2[k] * x2[k];
      }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {                   // over the pixel's 8 lanes: every one ends with the full sums
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    const float r1 = 1.f / sqrtf(1e-8f + s1), r2 = 1.f / sqrtf(1e-8f + s2);
#pragma unroll
    for (int i = 0; i < LPIPS_MAXV; ++i) {
      const int v = j + 8 * i;
      if (ok && v < nv) {
        float x1[8], x2[8];
        unpack8<DT>(va[i], x1);
        unpack8<DT>(vb[i], x2);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          // no fma here: n1 and n2 are each rounded once, so (n1 - n2)^2 is the same number with the images swapped
#pragma clang fp contract(off)
          const int c = v * 8 + k;
          const float d = x1[k] * r1 - x2[k] * r2;
          acc += (c < tp.C ? tp.w[c] : 0.f) * (d * d);
        }
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// per_image[n] = sum_t (1 / hw_t) * (tap t's partials of image n);  total (+)= total_scale * sum_n per_image[n]
__global__ __launch_bounds__(1024) void lpips_finalize_kernel(LpipsTaps a, const float* __restrict__ partial,
                                                              float* __restrict__ per_image, float* __restrict__ total,
                                                              float total_scale, int accumulate) {
  __shared__ float wsum[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float mine = 0.f;                                     // this wave's images n = wave, wave + 16, ...
  for (int n = wave; n < a.N; n += 16) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LPIPS_MAX_TAPS; ++i) {
      if (i < a.ntaps) {
        const LpipsTap& tp = a.t[i];
        float t = 0.f;
        for (int k = lane; k < tp.nblk; k += 64) t += partial[tp.blk0 + n * tp.nblk + k];
        s += wave_sum(t) / (float)tp.hw;
      }
    }
    if (lane == 0) per_image[n] = s;
    mine += s;
  }
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int w = 0; w < 16; ++w) acc += wsum[w];
    const float v = acc * total_scale;
    total[0] = accumulate ? total[0] + v : v;
  }
}

static bool lpips_taps_ok(int ntaps, const int* hw, const int* cp, const int* c) {
  for (int i = 0; i < ntaps; ++i) {
    if (hw[i] < 1) return false;
    if (cp && (cp[i] < 8 || cp[i] % 8 || cp[i] > 8 * 8 * LPIPS_MAXV)) return false;
    if (c && cp && (c[i] < 1 || c[i] > cp[i])) return false;
  }
  return true;
}

extern "C" int dsr_lpips_distance_blocks(int ntaps, const int* hw, int N) {
  if (!hw || ntaps < 1 || ntaps > LPIPS_MAX_TAPS || N < 1 || !lpips_taps_ok(ntaps, hw, nullptr, nullptr)) return 0;
  LpipsTaps a;
  const int blocks = lpips_table(a, ntaps, hw, N);
  return blocks > 0 ? blocks : 0;
}

extern "C" int dsr_lpips_distance(int dtype, int ntaps, const void* const* feats, const float* const* lin_w, const int* hw,
                                  const int* cp, const int* c, int N, float* partial, dsr_stream_t st) {
  DSR_REQUIRE(feats && lin_w && hw && cp && c && partial && DSR_DTYPE_OK(dtype), "lpips_distance: null pointer or bad dtype");
  DSR_REQUIRE(ntaps >= 1 && ntaps <= LPIPS_MAX_TAPS && N >= 1, "lpips_distance: %d taps (1..%d), %d images", ntaps, LPIPS_MAX_TAPS,
              N);
  DSR_REQUIRE(lpips_taps_ok(ntaps, hw, cp, c), "lpips_distance: bad tap table (hw >= 1, Cp %% 8 == 0, Cp <= %d, 1 <= C <= Cp)",
              8 * 8 * LPIPS_MAXV);
  LpipsTaps a;
  const int blocks = lpips_table(a, ntaps, hw, N);
  DSR_REQUIRE(blocks > 0, "lpips_distance: too many pixels");
  for (int i = 0; i < ntaps; ++i) {
    DSR_REQUIRE(feats[i] && lin_w[i], "lpips_distance: null feature map or weight of tap %d", i);
    a.t[i].f = (const unsigned short*)feats[i];
    a.t[i].w = lin_w[i];
    a.t[i].Cp = cp[i];
    a.t[i].C = c[i];
  }
  LPIPS_DT_SWITCH(dtype, hipLaunchKernelGGL((lpips_distance_kernel<DT>), dim3(blocks), dim3(256), 0, st, a, partial));
  return dsr_launch_status("dsr_lpips_distance");
}

extern "C" int dsr_lpips_finalize(int ntaps, const int* hw, int N, const float* partial, float* per_image, float* total,
                                  float total_scale, int accumulate, dsr_stream_t st) {
  DSR_REQUIRE(hw && partial && per_image && total, "lpips_finalize: null pointer");
  DSR_REQUIRE(ntaps >= 1 && ntaps <= LPIPS_MAX_TAPS && N >= 1, "lpips_finalize: %d taps (1..%d), %d images", ntaps, LPIPS_MAX_TAPS,
              N);
  DSR_REQUIRE(lpips_taps_ok(ntaps, hw, nullptr, nullptr), "lpips_finalize: empty tap");
  LpipsTaps a;
  DSR_REQUIRE(lpips_table(a, ntaps, hw, N) > 0, "lpips_finalize: too many pixels");
  hipLaunchKernelGGL(lpips_finalize_kernel, dim3(1), dim3(1024), 0, st, a, partial, per_image, total, total_scale,
                     accumulate ? 1 : 0);
  return dsr_launch_status("dsr_lpips_finalize");
}

// ---------------------------------------------------------------------------------------------------- distance backward
// With s = sqrt(1e-8 + sum_c f_c^2), n = f / s and u_c = 2 w_c (n1_c - n2_c) coef, coef = g[image] * scale / hw:
//   d/df1 = (u - n1 <u, n1>) / s1,   d/df2 = -(u - n2 <u, n2>) / s2
// (the eps sits inside the root, so ds/df = n exactly: this is the whole derivative).  Every tap is a ReLU output, so what is
// stored is that gradient times (f > 0): the gradient at the pre-activation, ready to be added to what the deeper layers send.
// Same block table and lane layout as lpips_distance_kernel; d1 / d2 are [N][hw][Cp] (either may be absent).
struct LpipsBwdOut {
  unsigned short* d1[LPIPS_MAX_TAPS];
  unsigned short* d2[LPIPS_MAX_TAPS];
};

template <int DT>
__global__ __launch_bounds__(256) void lpips_distance_bwd_kernel(LpipsTaps a, LpipsBwdOut o, const float* __restrict__ g, float scale) {
  const int b = blockIdx.x;
  LpipsTap tp = a.t[0];
  unsigned short *o1 = o.d1[0], *o2 = o.d2[0];
#pragma unroll
  for (int i = 1; i < LPIPS_MAX_TAPS; ++i)
    if (i < a.ntaps && b >= a.t[i].blk0) {
      tp = a.t[i];
      o1 = o.d1[i];
      o2 = o.d2[i];
    }
  const int local = b - tp.blk0;
  const int n = local / tp.nblk, chunk = local - n * tp.nblk;
  const int grp = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int nv = tp.Cp / 8;
  const unsigned short* f1 = tp.f + (size_t)n * tp.hw * tp.Cp;
  const unsigned short* f2 = tp.f + (size_t)(n + a.N) * tp.hw * tp.Cp;
  const float coef = 2.f * (g[n] * scale / (float)tp.hw);
  for (int it = 0; it < LPIPS_PIX_PER_BLOCK / 32; ++it) {
    const int p = chunk * LPIPS_PIX_PER_BLOCK + it * 32 + grp;
    const bool ok = p < tp.hw;                          // uniform over the 8 lanes of a pixel
    U4 va[LPIPS_MAXV], vb[LPIPS_MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < LPIPS_MAXV; ++i) {
      const int v = j + 8 * i;
      const bool in = ok && v < nv;
      const size_t off = in ? (size_t)p * tp.Cp + v * 8 : 0;
      va[i] = load16_or_zero(f1, off, in);
      vb[i] = load16_or_zero(f2, off, in);
      float x1[8], x2[8];
      unpack8<DT>(va[i], x1);
      unpack8<DT>(vb[i], x2);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s1 += x1[k] * x1[k];
        s2 += x2[k] * x2[k];
      }
    }
#pragma unroll
    for (int sh = 1; sh < 8; sh <<= 1) {
      s1 += __shfl_xor(s1, sh, 64);
      s2 += __shfl_xor(s2, sh, 64);
    }
    const float r1 = 1.f / sqrtf(1e-8f + s1), r2 = 1.f / sqrtf(1e-8f + s2);
    float a1 = 0.f, a2 = 0.f;                           // <u, n1>, <u, n2>
#pragma unroll
    for (int i = 0; i < LPIPS_MAXV; ++i) {
      const int v = j + 8 * i;
      if (ok && v < nv) {
        float x1[8], x2[8];
        unpack8<DT>(va[i], x1);
        unpack8<DT>(vb[i], x2);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = v * 8 + k;
          const float n1 = x1[k] * r1, n2 = x2[k] * r2;
          const float u = (c < tp.C ? tp.w[c] : 0.f) * (n1 - n2) * coef;
          a1 += u * n1;
          a2 += u * n2;
        }
      }
    }
#pragma unroll
    for (int sh = 1; sh < 8; sh <<= 1) {
      a1 += __shfl_xor(a1, sh, 64);
      a2 += __shfl_xor(a2, sh, 64);
    }
#pragma unroll
    for (int i = 0; i < LPIPS_MAXV; ++i) {
      const int v = j + 8 * i;
      if (ok && v < nv) {
        float x1[8], x2[8], d1[8], d2[8];
        unpack8<DT>(va[i], x1);
        unpack8<DT>(vb[i], x2);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = v * 8 + k;
          const float n1 = x1[k] * r1, n2 = x2[k] * r2;
          const float u = (c < tp.C ? tp.w[c] : 0.f) * (n1 - n2) * coef;
          d1[k] = x1[k] > 0.f ? (u - n1 * a1) * r1 : 0.f;
          d2[k] = x2[k] > 0.f ? (n2 * a2 - u) * r2 : 0.f;
          if constexpr (DT == DSR_DTYPE_F16) {          // 1 / s reaches 1e4 on a near-zero feature vector: saturate, never inf
            d1[k] = fminf(fmaxf(d1[k], -65504.f), 65504.f);
            d2[k] = fminf(fmaxf(d2[k], -65504.f), 65504.f);
          }
        }
        const size_t off = ((size_t)n * tp.hw + p) * tp.Cp + v * 8;
        if (o1) *reinterpret_cast<U4*>(o1 + off) = pack8<DT>(d1);
        if (o2) *reinterpret_cast<U4*>(o2 + off) = pack8<DT>(d2);
      }
    }
  }
}

extern "C" int dsr_lpips_distance_bwd(int dtype, int ntaps, const void* const* feats, const float* const* lin_w, const int* hw,
                                      const int* cp, const int* c, int N, const float* g, float scale, void* const* d1,
                                      void* const* d2, dsr_stream_t st) {
  DSR_REQUIRE(feats && lin_w && hw && cp && c && g && DSR_DTYPE_OK(dtype), "lpips_distance_bwd: null pointer or bad dtype");
  DSR_REQUIRE(d1 || d2, "lpips_distance_bwd: neither half's gradient is asked for");
  DSR_REQUIRE(ntaps >= 1 && ntaps <= LPIPS_MAX_TAPS && N >= 1, "lpips_distance_bwd: %d taps (1..%d), %d images", ntaps,
              LPIPS_MAX_TAPS, N);
  DSR_REQUIRE(lpips_taps_ok(ntaps, hw, cp, c), "lpips_distance_bwd: bad tap table (hw >= 1, Cp %% 8 == 0, Cp <= %d, 1 <= C <= Cp)",
              8 * 8 * LPIPS_MAXV);
  DSR_REQUIRE(scale > 0.f && scale < INFINITY, "lpips_distance_bwd: the loss scale must be positive and finite");
  LpipsTaps a;
  const int blocks = lpips_table(a, ntaps, hw, N);
  DSR_REQUIRE(blocks > 0, "lpips_distance_bwd: too many pixels");
  LpipsBwdOut o;
  memset(&o, 0, sizeof(o));
  for (int i = 0; i < ntaps; ++i) {
    DSR_REQUIRE(feats[i] && lin_w[i] && (!d1 || d1[i]) && (!d2 || d2[i]),
                "lpips_distance_bwd: null feature map, weight or gradient of tap %d", i);
    if ((long long)2 * N * hw[i] * cp[i] * 2 >= (1ll << 31))
      return dsr_fail(DSR_E_UNSUPPORTED, "lpips_distance_bwd: tap %d of 2 GiB or more: split the batch", i);
    a.t[i].f = (const unsigned short*)feats[i];
    a.t[i].w = lin_w[i];
    a.t[i].Cp = cp[i];
    a.t[i].C = c[i];
    o.d1[i] = d1 ? (unsigned short*)d1[i] : nullptr;
    o.d2[i] = d2 ? (unsigned short*)d2[i] : nullptr;
  }
  LPIPS_DT_SWITCH(dtype, hipLaunchKernelGGL((lpips_distance_bwd_kernel<DT>), dim3(blocks), dim3(256), 0, st, a, o, g, scale));
  return dsr_launch_status("dsr_lpips_distance_bwd");
}
