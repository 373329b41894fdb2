// Image-quality metric on the device: SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) as the reference's scripts use it --
// torchmetrics StructuralSimilarityIndexMeasure(data_range=1.0) at train_GAN.py:31,111, DIP.py:74,158,184, eval_GAN.py:31,48:
// Gaussian 11x11 window, sigma 1.5, K1 = 0.01, K2 = 0.03, per channel, mean over all window positions that lie inside the
// image (torchmetrics pads by reflection and crops that border again, which is the same set of positions).
// torchmetrics is not installed here and cannot be fetched: "parity unpinned"; the oracle (oracle/metrics.py) restates
// the published formula with F.conv2d and is what the GPU test compares against.
//
// One forward kernel serves every caller (metrics.py's SSIM, MS-SSIM and SSIM_Y modules and evaluate.ssim): ssim_img_kernel,
// fp32 NCHW in, one partial sum per block out, folded by a one-block launch (deterministic, no atomics).  With it in this file:
// the SSIM and MS-SSIM input gradients, the 2x2 mean pool of the multi-scale pyramid, the PSNR statistics and the device-side
// running state of the metric modules.
// Every moment is accumulated the same way -- the product of the two pixels formed once, then one explicit fma per tap -- and
// the position's value comes from ssim_of_moments: with `r += g * x * y` left to the compiler, hipcc packs some moments into
// v_pk_fma_f32 and others into v_pk_mul_f32 + v_add_f32, so E[ab] and E[a^2] of IDENTICAL images differ in the last bit and
// their SSIM is 1 - 1e-6 instead of 1 (the cancellation in the variances amplifies by 1 / (va + vb + c2)).
#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define SSIM_K 11

struct SsimWindow {
  float g[SSIM_K];   // separable 1-D Gaussian, normalised to sum 1
};

// SSIM of one window position from its raw moments.  No contraction and the products a*b formed once: swapping the images
// gives the same bits, and identical images give exactly 1 (2 mab == maa + mbb and 2 cab == va + vb then hold exactly).
__device__ __forceinline__ float ssim_of_moments(float ma, float mb, float saa, float sbb, float sab, float c1, float c2) {
#pragma clang fp contract(off)
  const float maa = ma * ma, mbb = mb * mb, mab = ma * mb;
  const float va = saa - maa, vb = sbb - mbb, cab = sab - mab;
  return ((2.f * mab + c1) * (2.f * cab + c2)) / ((maa + mbb + c1) * (va + vb + c2));
}

// ================================================================================ metrics.StructuralSimilarityIndexMeasure
// Per-image SSIM, its input gradient, PSNR statistics and the device-side running state of the two metric modules
// (metrics.py).  The formula is unclamped; c1 = (k1 range)^2, c2 = (k2 range)^2 are arguments.
// Reductions are deterministic: one partial per block (plain stores), folded in a fixed order by a one-block finalise launch.

static SsimWindow ssim_gauss_window() {
  SsimWindow win;
  double s = 0.0, g[SSIM_K];
  for (int i = 0; i < SSIM_K; ++i) {
    const double d = i - (SSIM_K - 1) / 2.0;
    g[i] = exp(-d * d / (2.0 * 1.5 * 1.5));
    s += g[i];
  }
  for (int i = 0; i < SSIM_K; ++i) win.g[i] = (float)(g[i] / s);
  return win;
}

// The same position as its two factors: the contrast-structure term cs = (2 cab + c2) / (va + vb + c2) and
// ssim = cs * (2 mab + c1) / (maa + mbb + c1) (torchmetrics' return_contrast_sensitivity pair, which multi-scale SSIM
// folds per scale).  Same rules as above: no contraction, products formed once, so swapped images give the same bits
// and identical images give exactly cs = 1 and ssim = 1 * 1.
__device__ __forceinline__ void ssim_cs_of_moments(float ma, float mb, float saa, float sbb, float sab, float c1, float c2,
                                                   float& ssim, float& cs) {
#pragma clang fp contract(off)
  const float maa = ma * ma, mbb = mb * mb, mab = ma * mb;
  const float va = saa - maa, vb = sbb - mbb, cab = sab - mab;
  cs = (2.f * cab + c2) / (va + vb + c2);
  ssim = cs * ((2.f * mab + c1) / (maa + mbb + c1));
}

// ---- forward: a block owns SF_TH x SF_TW window positions of one plane; separable passes over a (SF_TH+10) x (SF_TW+10)
// tile of both images in LDS (11 row taps x 5 moments per staged row, then 11 column taps x 5 moments per position).
// CS = false: one partial per block, the SSIM sum (partial[block]).  CS = true: two, the SSIM sum and the sum of the
// contrast-structure term (partial[2 block], partial[2 block + 1]).
#define SF_TW 64
#define SF_TH 16
template <bool CS>
__global__ __launch_bounds__(256) void ssim_img_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                       int tiles_x, int tiles_y, float c1, float c2, SsimWindow win,
                                                       float* __restrict__ partial) {
  constexpr int SR = SF_TH + SSIM_K - 1, SC = SF_TW + SSIM_K - 1;
  __shared__ float sa[SR][SC + 1], sb[SR][SC + 1];
  __shared__ float hm[5][SR][SF_TW + 1];
  __shared__ float red[CS ? 8 : 4];
  const int plane = blockIdx.x / (tiles_x * tiles_y);
  const int t = blockIdx.x % (tiles_x * tiles_y);
  const int y0 = (t / tiles_x) * SF_TH, x0 = (t % tiles_x) * SF_TW;
  const float* pa = a + (size_t)plane * H * W;
  const float* pb = b + (size_t)plane * H * W;
  for (int i = threadIdx.x; i < SR * SC; i += 256) {
    const int ly = i / SC, lx = i % SC;
    const int y = y0 + ly, x = x0 + lx;
    const bool ok = y < H && x < W;
    sa[ly][lx] = ok ? pa[(size_t)y * W + x] : 0.f;
    sb[ly][lx] = ok ? pb[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SR * SF_TW; i += 256) {
    const int r = i / SF_TW, c = i % SF_TW;
    float ra = 0.f, rb = 0.f, raa = 0.f, rbb = 0.f, rab = 0.f;
#pragma unroll
    for (int dx = 0; dx < SSIM_K; ++dx) {
      const float xa = sa[r][c + dx], xb = sb[r][c + dx], g = win.g[dx];
      const float paa = xa * xa, pbb = xb * xb, pab = xa * xb;
      ra = fmaf(g, xa, ra);
      rb = fmaf(g, xb, rb);
      raa = fmaf(g, paa, raa);
      rbb = fmaf(g, pbb, rbb);
      rab = fmaf(g, pab, rab);
    }
    hm[0][r][c] = ra;
    hm[1][r][c] = rb;
    hm[2][r][c] = raa;
    hm[3][r][c] = rbb;
    hm[4][r][c] = rab;
  }
  __syncthreads();
  const int OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  const int c = threadIdx.x % SF_TW;
  float v = 0.f, vcs = 0.f;
  for (int r = threadIdx.x / SF_TW; r < SF_TH; r += 256 / SF_TW) {
    if (y0 + r < OH && x0 + c < OW) {
      float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dy = 0; dy < SSIM_K; ++dy) {
        const float g = win.g[dy];
#pragma unroll
        for (int k = 0; k < 5; ++k) m[k] = fmaf(g, hm[k][r + dy][c], m[k]);
      }
      if constexpr (CS) {
        float s, q;
        ssim_cs_of_moments(m[0], m[1], m[2], m[3], m[4], c1, c2, s, q);
        v += s;
        vcs += q;
      } else {
        v += ssim_of_moments(m[0], m[1], m[2], m[3], m[4], c1, c2);
      }
    }
  }
  v = wave_sum(v);
  if constexpr (CS) vcs = wave_sum(vcs);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = v;
    if constexpr (CS) red[4 + (threadIdx.x >> 6)] = vcs;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if constexpr (CS) {
      partial[2 * (size_t)blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
      partial[2 * (size_t)blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    } else {
      partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
  }
}

// per_image[n] = inv_count * (the nblk partials of image n, folded in a fixed order); total (+)= total_scale * sum_n per_image
__global__ __launch_bounds__(1024) void ssim_img_finalize_kernel(const float* __restrict__ partial, int N, int nblk,
                                                                 float inv_count, float* __restrict__ per_image,
                                                                 float* __restrict__ total, float total_scale, int accumulate) {
  __shared__ float wsum[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float mine = 0.f;
  for (int n = wave; n < N; n += 16) {
    float s = 0.f;
    for (int k = lane; k < nblk; k += 64) s += partial[(size_t)n * nblk + k];
    s = wave_sum(s) * inv_count;
    if (lane == 0 && per_image) per_image[n] = s;
    mine += s;
  }
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0 && total) {
    float acc = 0.f;
    for (int w = 0; w < 16; ++w) acc += wsum[w];
    const float v = acc * total_scale;
    total[0] = accumulate ? total[0] + v : v;
  }
}

static long long ssim_img_tiles(int H, int W) {
  const int OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  return (long long)((OH + SF_TH - 1) / SF_TH) * ((OW + SF_TW - 1) / SF_TW);
}

static bool ssim_consts_ok(float c1, float c2) {
  return c1 > 0.f && c1 < INFINITY && c2 > 0.f && c2 < INFINITY;     // false for NaN too
}

extern "C" int dsr_ssim_img_blocks(int N, int C, int H, int W) {
  if (N < 1 || C < 1 || H < SSIM_K || W < SSIM_K) return 0;
  const long long b = (long long)N * C * ssim_img_tiles(H, W);
  return b < (1ll << 31) ? (int)b : 0;
}

extern "C" int dsr_ssim_img_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2,
                                float* partial, float* per_image, float* total, float total_scale, int accumulate,
                                dsr_stream_t st) {
  DSR_REQUIRE(img1 && img2 && partial, "ssim_img: null pointer");
  DSR_REQUIRE(per_image || total, "ssim_img: neither per-image values nor a total are asked for");
  DSR_REQUIRE(N >= 1 && C >= 1, "ssim_img: %d images of %d planes", N, C);
  DSR_REQUIRE(H >= SSIM_K && W >= SSIM_K, "ssim_img: image %dx%d smaller than the 11x11 window", H, W);
  DSR_REQUIRE(ssim_consts_ok(c1, c2), "ssim_img: c1 and c2 must be positive and finite (data_range > 0)");
  const int blocks = dsr_ssim_img_blocks(N, C, H, W);
  DSR_REQUIRE(blocks > 0, "ssim_img: too many window tiles");
  const int OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  const int tiles_y = (OH + SF_TH - 1) / SF_TH, tiles_x = (OW + SF_TW - 1) / SF_TW;
  hipLaunchKernelGGL(ssim_img_kernel<false>, dim3(blocks), dim3(256), 0, st, img1, img2, H, W, tiles_x, tiles_y, c1, c2,
                     ssim_gauss_window(), partial);
  const int rc = dsr_launch_status("dsr_ssim_img_f32");
  if (rc) return rc;
  const float inv_count = (float)(1.0 / ((double)C * OH * OW));
  hipLaunchKernelGGL(ssim_img_finalize_kernel, dim3(1), dim3(1024), 0, st, partial, N, blocks / N, inv_count, per_image,
                     total, total_scale, accumulate ? 1 : 0);
  return dsr_launch_status("dsr_ssim_img_f32");
}

// ---- backward.  A block owns a SB_T x SB_T tile of gradient pixels of one plane.  The window positions that reach it are the
// tile plus 10 on the top / left (a position p covers pixels p .. p+10), whose windows need the images over the tile plus 10
// on every side.  Passes (LDS):
//   1. stage a, b over (T+20)^2;                               2. row taps: 5 moments of every staged row, (T+20) x (T+10);
//   3. column taps -> moments of the (T+10)^2 positions -> the coefficient maps dS/dmu_a, dS/dmu_b, dS/dE[a^2] (= dS/dE[b^2]),
//      dS/dE[ab], zero at positions outside the image's OH x OW (the plain transposed valid correlation at the border);
//   4. transposed row taps, (T+10) x T;                        5. transposed column taps per pixel, and
//   da = k (W'cmu_a + 2 a W'cE2 + b W'cEab),  db = k (W'cmu_b + 2 b W'cE2 + a W'cEab),  k = g[n] / (C OH OW).
// Buffers of passes 1 / 3 and 2 / 4 share LDS (each is dead before its partner is written): 73.6 KB, two blocks per CU.
//
// MS = true is one scale of the multi-scale backward (dsr_msssim_bwd_f32).  Each image carries two upstream weights,
// k_sim = g[n] w_sim[n] / (C OH OW) for its SSIM mean and k_cs = g[n] w_cs[n] / (C OH OW) for its contrast-structure mean
// (a null weight array is 0).  With l = A1 / B1, cs = A2 / B2, S = l cs, the maps of pass 3 are those of k_sim S + k_cs cs
//   = u d cs + t d l,   u = k_sim l + k_cs,  t = k_sim cs:
//   d/dmu_a = 2 u (mu_a cs - mu_b) / B2 + 2 t (mu_b - l mu_a) / B1,   d/dE[a^2] = -u cs / B2,   d/dE[ab] = 2 u / B2,
// so pass 5 multiplies by nothing more; its epilogue adds the gradient that arrived at the next coarser scale spread back
// through the 2x2 mean pool, 0.25 coarse[y/2][x/2] for pixels inside the pooled extent (a dropped odd row / column gets none).
#define SB_T 32
#define SB_SR (SB_T + 2 * (SSIM_K - 1))        // staged rows / columns
#define SB_PR (SB_T + SSIM_K - 1)              // window positions per row / column
#define SB_R1 (4 * SB_PR * (SB_PR + 1))        // >= 2 * SB_SR * (SB_SR + 1): stage, then the coefficient maps
#define SB_R2 (5 * SB_SR * (SB_PR + 1))        // >= 4 * SB_PR * (SB_T + 1): row moments, then transposed row sums
static_assert(SB_R1 >= 2 * SB_SR * (SB_SR + 1), "ssim_bwd LDS layout");
static_assert(SB_R2 >= 4 * SB_PR * (SB_T + 1), "ssim_bwd LDS layout");

template <bool MS>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int C, int H,
                                                       int W, int tiles_x, int tiles_y, float c1, float c2, SsimWindow win,
                                                       const float* __restrict__ g, float inv_count, float* __restrict__ ga,
                                                       float* __restrict__ gb, const float* __restrict__ w_sim,
                                                       const float* __restrict__ w_cs, const float* __restrict__ coarse_a,
                                                       const float* __restrict__ coarse_b) {
  __shared__ float r1[SB_R1];
  __shared__ float r2[SB_R2];
  // r1 as the stage [2][SB_SR][SB_SR+1], then as the coefficient maps [4][SB_PR][SB_PR+1]
  // r2 as the row moments [5][SB_SR][SB_PR+1], then as the transposed row sums [4][SB_PR][SB_T+1]
#define STG(i, y, x) r1[((i) * SB_SR + (y)) * (SB_SR + 1) + (x)]
#define CF(m, y, x) r1[((m) * SB_PR + (y)) * (SB_PR + 1) + (x)]
#define HM(k, y, x) r2[((k) * SB_SR + (y)) * (SB_PR + 1) + (x)]
#define TH(m, y, x) r2[((m) * SB_PR + (y)) * (SB_T + 1) + (x)]
  const bool want_a = ga != nullptr, want_b = gb != nullptr;
  const int nm = (want_a && want_b) ? 4 : 3;        // maps: [0] dS/dmu of the (first) wanted image, [1] dS/dE2, [2] dS/dEab, [3] dS/dmu_b
  const int plane = blockIdx.x / (tiles_x * tiles_y);
  const int t = blockIdx.x % (tiles_x * tiles_y);
  const int y0 = (t / tiles_x) * SB_T, x0 = (t % tiles_x) * SB_T;
  const int OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  const float* pa = a + (size_t)plane * H * W;
  const float* pb = b + (size_t)plane * H * W;
  const float k = g[plane / C] * inv_count;
  const float k_sim = (MS && w_sim) ? k * w_sim[plane / C] : 0.f, k_cs = (MS && w_cs) ? k * w_cs[plane / C] : 0.f;
  // 1. stage pixel (y0 - 10 + sy, x0 - 10 + sx); zero outside the image (those only feed positions that do not exist)
  for (int i = threadIdx.x; i < SB_SR * SB_SR; i += 256) {
    const int sy = i / SB_SR, sx = i % SB_SR;
    const int y = y0 - (SSIM_K - 1) + sy, x = x0 - (SSIM_K - 1) + sx;
    const bool ok = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    STG(0, sy, sx) = ok ? pa[(size_t)y * W + x] : 0.f;
    STG(1, sy, sx) = ok ? pb[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();
  // 2. row taps: position column px covers staged columns px .. px+10
  for (int i = threadIdx.x; i < SB_SR * SB_PR; i += 256) {
    const int sy = i / SB_PR, px = i % SB_PR;
    float ra = 0.f, rb = 0.f, raa = 0.f, rbb = 0.f, rab = 0.f;
#pragma unroll
    for (int dx = 0; dx < SSIM_K; ++dx) {
      const float xa = STG(0, sy, px + dx), xb = STG(1, sy, px + dx), w = win.g[dx];
      const float paa = xa * xa, pbb = xb * xb, pab = xa * xb;
      ra = fmaf(w, xa, ra);
      rb = fmaf(w, xb, rb);
      raa = fmaf(w, paa, raa);
      rbb = fmaf(w, pbb, rbb);
      rab = fmaf(w, pab, rab);
    }
    HM(0, sy, px) = ra;
    HM(1, sy, px) = rb;
    HM(2, sy, px) = raa;
    HM(3, sy, px) = rbb;
    HM(4, sy, px) = rab;
  }
  __syncthreads();
  // 3. column taps and the coefficient maps (every thread finishes its reads of r2 before anyone writes r1: the stage in r1 is
  //    dead after pass 2, and CF only overwrites r1)
  for (int i = threadIdx.x; i < SB_PR * SB_PR; i += 256) {
    const int py = i / SB_PR, px = i % SB_PR;
    const int qy = y0 - (SSIM_K - 1) + py, qx = x0 - (SSIM_K - 1) + px;
    float cma = 0.f, cmb = 0.f, ce2 = 0.f, ceab = 0.f;
    if ((unsigned)qy < (unsigned)OH && (unsigned)qx < (unsigned)OW) {
      float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dy = 0; dy < SSIM_K; ++dy) {
        const float w = win.g[dy];
#pragma unroll
        for (int j = 0; j < 5; ++j) m[j] = fmaf(w, HM(j, py + dy, px), m[j]);
      }
      const float ma = m[0], mb = m[1];
      const float maa = ma * ma, mbb = mb * mb, mab = ma * mb;
      const float A1 = 2.f * mab + c1, A2 = 2.f * (m[4] - mab) + c2;
      const float B1 = maa + mbb + c1, B2 = (m[2] - maa) + (m[3] - mbb) + c2;
      if constexpr (MS) {
        const float i1 = 1.f / B1, i2 = 1.f / B2;
        const float l = A1 * i1, cs = A2 * i2;
        const float u2 = 2.f * (k_sim * l + k_cs) * i2, t2 = 2.f * (k_sim * cs) * i1;
        cma = u2 * (ma * cs - mb) + t2 * (mb - l * ma);
        cmb = u2 * (mb * cs - ma) + t2 * (ma - l * mb);
        ce2 = -0.5f * u2 * cs;
        ceab = u2;
      } else {
        const float inv = 1.f / (B1 * B2);
        const float S = A1 * A2 * inv;
        const float d = 2.f * (A2 - A1) * inv, e = 2.f * S * (1.f / B1 - 1.f / B2);
        cma = mb * d - ma * e;                      // dS/dmu_a
        cmb = ma * d - mb * e;                      // dS/dmu_b
        ce2 = -S / B2;                              // dS/dE[a^2] = dS/dE[b^2]
        ceab = 2.f * A1 * inv;                      // dS/dE[ab]
      }
    }
    CF(0, py, px) = want_a ? cma : cmb;
    CF(1, py, px) = ce2;
    CF(2, py, px) = ceab;
    if (nm == 4) CF(3, py, px) = cmb;
  }
  __syncthreads();
  // 4. transposed row taps: pixel column tx receives position columns tx .. tx+10 (position px = tx + 10 - dx, weight g[dx])
  for (int i = threadIdx.x; i < nm * SB_PR * SB_T; i += 256) {
    const int m = i / (SB_PR * SB_T), r = i % (SB_PR * SB_T);
    const int py = r / SB_T, tx = r % SB_T;
    float s = 0.f;
#pragma unroll
    for (int dx = 0; dx < SSIM_K; ++dx) s = fmaf(win.g[dx], CF(m, py, tx + (SSIM_K - 1) - dx), s);
    TH(m, py, tx) = s;
  }
  __syncthreads();
  // 5. transposed column taps and the image gradients
  for (int i = threadIdx.x; i < SB_T * SB_T; i += 256) {
    const int ty = i / SB_T, tx = i % SB_T;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    float G[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < SSIM_K; ++dy) {
      const float w = win.g[dy];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (m < nm) G[m] = fmaf(w, TH(m, ty + (SSIM_K - 1) - dy, tx), G[m]);
    }
    const size_t o = (size_t)plane * H * W + (size_t)y * W + x;
    const float va = pa[(size_t)y * W + x], vb = pb[(size_t)y * W + x];
    if constexpr (MS) {
      const int Hc = H >> 1, Wc = W >> 1;
      const bool pooled = (y >> 1) < Hc && (x >> 1) < Wc;
      const size_t oc = ((size_t)plane * Hc + (y >> 1)) * Wc + (x >> 1);
      if (want_a) ga[o] = (G[0] + 2.f * va * G[1] + vb * G[2]) + ((coarse_a && pooled) ? 0.25f * coarse_a[oc] : 0.f);
      if (want_b)
        gb[o] = ((want_a ? G[3] : G[0]) + 2.f * vb * G[1] + va * G[2]) + ((coarse_b && pooled) ? 0.25f * coarse_b[oc] : 0.f);
    } else {
      if (want_a) ga[o] = k * (G[0] + 2.f * va * G[1] + vb * G[2]);
      if (want_b) gb[o] = k * ((want_a ? G[3] : G[0]) + 2.f * vb * G[1] + va * G[2]);
    }
  }
#undef STG
#undef CF
#undef HM
#undef TH
}

extern "C" int dsr_ssim_bwd_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2,
                                const float* g, float* grad1, float* grad2, dsr_stream_t st) {
  DSR_REQUIRE(img1 && img2 && g, "ssim_bwd: null pointer");
  DSR_REQUIRE(grad1 || grad2, "ssim_bwd: neither image's gradient is asked for");
  DSR_REQUIRE(N >= 1 && C >= 1, "ssim_bwd: %d images of %d planes", N, C);
  DSR_REQUIRE(H >= SSIM_K && W >= SSIM_K, "ssim_bwd: image %dx%d smaller than the 11x11 window", H, W);
  DSR_REQUIRE(ssim_consts_ok(c1, c2), "ssim_bwd: c1 and c2 must be positive and finite (data_range > 0)");
  const int tiles_y = (H + SB_T - 1) / SB_T, tiles_x = (W + SB_T - 1) / SB_T;
  const long long blocks = (long long)N * C * tiles_y * tiles_x;
  DSR_REQUIRE(blocks < (1ll << 31), "ssim_bwd: too many tiles");
  const int OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  const float inv_count = (float)(1.0 / ((double)C * OH * OW));
  hipLaunchKernelGGL(ssim_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, img1, img2, C, H, W, tiles_x, tiles_y,
                     c1, c2, ssim_gauss_window(), g, inv_count, grad1, grad2, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr);
  return dsr_launch_status("dsr_ssim_bwd_f32");
}

// ================================================================================ metrics.MultiScaleStructuralSimilarityIndexMeasure
// Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) as torchmetrics' MultiScaleStructuralSimilarityIndexMeasure states it: per
// scale the per-image means of SSIM and of its contrast-structure term, both images halved by a 2x2 mean between scales, and
// out[n] = prod_s v_s[n]^betas[s] over v = (cs_0 .. cs_{L-2}, ssim_{L-1}).  torchmetrics is absent here: PARITY UNPINNED.

// sim[n], cs[n] (either nullable) = inv_count * (the nblk partial pairs of image n, folded in a fixed order)
__global__ __launch_bounds__(1024) void ssim_cs_finalize_kernel(const float* __restrict__ partial, int N, int nblk,
                                                                float inv_count, float* __restrict__ sim,
                                                                float* __restrict__ cs) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int n = wave; n < N; n += 16) {
    float s = 0.f, q = 0.f;
    for (int k = lane; k < nblk; k += 64) {
      const float2 p = reinterpret_cast<const float2*>(partial)[(size_t)n * nblk + k];
      s += p.x;
      q += p.y;
    }
    s = wave_sum(s) * inv_count;
    q = wave_sum(q) * inv_count;
    if (lane == 0) {
      if (sim) sim[n] = s;
      if (cs) cs[n] = q;
    }
  }
}

extern "C" int dsr_ssim_cs_img_blocks(int N, int C, int H, int W) { return dsr_ssim_img_blocks(N, C, H, W); }

extern "C" int dsr_ssim_cs_img_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2,
                                   float* partial, float* sim, float* cs, dsr_stream_t st) {
  DSR_REQUIRE(img1 && img2 && partial, "ssim_cs_img: null pointer");
  DSR_REQUIRE(sim || cs, "ssim_cs_img: neither the SSIM nor the contrast-structure means are asked for");
  DSR_REQUIRE(((uintptr_t)partial & 7) == 0, "ssim_cs_img: partial must be 8-byte aligned");
  DSR_REQUIRE(N >= 1 && C >= 1, "ssim_cs_img: %d images of %d planes", N, C);
  DSR_REQUIRE(H >= SSIM_K && W >= SSIM_K, "ssim_cs_img: image %dx%d smaller than the 11x11 window", H, W);
  DSR_REQUIRE(ssim_consts_ok(c1, c2), "ssim_cs_img: c1 and c2 must be positive and finite (data_range > 0)");
  const int blocks = dsr_ssim_img_blocks(N, C, H, W);
  DSR_REQUIRE(blocks > 0, "ssim_cs_img: too many window tiles");
  const int OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  const int tiles_y = (OH + SF_TH - 1) / SF_TH, tiles_x = (OW + SF_TW - 1) / SF_TW;
  hipLaunchKernelGGL(ssim_img_kernel<true>, dim3(blocks), dim3(256), 0, st, img1, img2, H, W, tiles_x, tiles_y, c1, c2,
                     ssim_gauss_window(), partial);
  const int rc = dsr_launch_status("dsr_ssim_cs_img_f32");
  if (rc) return rc;
  const float inv_count = (float)(1.0 / ((double)C * OH * OW));
  hipLaunchKernelGGL(ssim_cs_finalize_kernel, dim3(1), dim3(1024), 0, st, partial, N, blocks / N, inv_count, sim, cs);
  return dsr_launch_status("dsr_ssim_cs_img_f32");
}

// ---- both images to half size in one launch: out[y][x] = mean of in[2y .. 2y+1][2x .. 2x+1], F.avg_pool2d(x, 2) (an odd last
// row / column is dropped).  Bandwidth-bound.  V4 (W % 4 == 0, 16-byte aligned planes): a thread loads one float4 of two
// input rows and stores two outputs as a float2; otherwise one output per thread from four scalar loads.  blockIdx.y picks
// the image.
template <bool V4>
__global__ __launch_bounds__(256) void avgpool2_pair_kernel(const float* __restrict__ in1, const float* __restrict__ in2,
                                                            float* __restrict__ out1, float* __restrict__ out2, int H, int W,
                                                            long long work) {
  const float* __restrict__ in = blockIdx.y ? in2 : in1;
  float* __restrict__ out = blockIdx.y ? out2 : out1;
  const int Ho = H >> 1, Wo = W >> 1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= work) return;
  if constexpr (V4) {
    const int W4 = W >> 2;
    const int x4 = (int)(i % W4);
    const long long r = i / W4;                               // plane * Ho + yo
    const int yo = (int)(r % Ho);
    const long long plane = r / Ho;
    const float* row = in + ((size_t)plane * H + 2 * (size_t)yo) * W + 4 * (size_t)x4;
    const float4 t = *reinterpret_cast<const float4*>(row), u = *reinterpret_cast<const float4*>(row + W);
    float2 o;
    o.x = 0.25f * ((t.x + t.y) + (u.x + u.y));
    o.y = 0.25f * ((t.z + t.w) + (u.z + u.w));
    *reinterpret_cast<float2*>(out + (size_t)r * Wo + 2 * (size_t)x4) = o;
  } else {
    const int xo = (int)(i % Wo);
    const long long r = i / Wo;
    const int yo = (int)(r % Ho);
    const long long plane = r / Ho;
    const float* row = in + ((size_t)plane * H + 2 * (size_t)yo) * W + 2 * (size_t)xo;
    out[(size_t)r * Wo + xo] = 0.25f * ((row[0] + row[1]) + (row[W] + row[W + 1]));
  }
}

extern "C" int dsr_avgpool2_pair_f32(const float* in1, const float* in2, float* out1, float* out2, int planes, int H, int W,
                                     dsr_stream_t st) {
  DSR_REQUIRE(in1 && in2 && out1 && out2, "avgpool2_pair: null pointer");
  DSR_REQUIRE(planes >= 1 && H >= 2 && W >= 2, "avgpool2_pair: %d planes of %dx%d", planes, H, W);
  const int Ho = H / 2, Wo = W / 2;
  const bool v4 = W % 4 == 0 && (((uintptr_t)in1 | (uintptr_t)in2) & 15) == 0 && (((uintptr_t)out1 | (uintptr_t)out2) & 7) == 0;
  const long long work = (long long)planes * Ho * (v4 ? W / 4 : Wo);
  const long long blocks = (work + 255) / 256;
  DSR_REQUIRE((long long)planes * H * W < (1ll << 40) && blocks < (1ll << 31), "avgpool2_pair: too many elements");
  if (v4)
    hipLaunchKernelGGL(avgpool2_pair_kernel<true>, dim3((unsigned)blocks, 2), dim3(256), 0, st, in1, in2, out1, out2, H, W, work);
  else
    hipLaunchKernelGGL(avgpool2_pair_kernel<false>, dim3((unsigned)blocks, 2), dim3(256), 0, st, in1, in2, out1, out2, H, W, work);
  return dsr_launch_status("dsr_avgpool2_pair_f32");
}

// ---- the pyramid's sizes (host queries)
extern "C" int dsr_msssim_min_size(int L) { return (L >= 1 && L <= DSR_MSSSIM_MAX_SCALES) ? SSIM_K << (L - 1) : 0; }

static bool msssim_shape_ok(int N, int C, int H, int W, int L) {
  const int m = dsr_msssim_min_size(L);
  return N >= 1 && C >= 1 && m > 0 && H >= m && W >= m;
}

// floats of one image's pooled levels 1 .. L-1, each [N][C][H >> s][W >> s], level 1 first (0: bad sizes, or L == 1)
extern "C" size_t dsr_msssim_pyramid_floats(int N, int C, int H, int W, int L) {
  if (!msssim_shape_ok(N, C, H, W, L)) return 0;
  size_t t = 0;
  for (int s = 1; s < L; ++s) t += (size_t)N * C * (H >> s) * (W >> s);
  return t;
}

// ---- combine: raw[s][n] = the cs mean of scale s < L-1, the SSIM mean of scale L-1.  One block; thread n strides the images.
//   v = raw, max(raw, 0) (relu) or (raw + 1) / 2 (simple);  out[n] = prod_s v_s^betas[s] (double, s ascending);
//   factors[s][n] = d out[n] / d raw[s][n] = betas[s] out / v_s (x 1/2 under simple); under relu 0 where v_s <= 0 -- the
//   image's out is 0 there, and so are all its factors (torch autograd has 0 * inf = NaN at that point).
struct MsssimBetas {
  float b[DSR_MSSSIM_MAX_SCALES];
};

__global__ __launch_bounds__(256) void msssim_combine_kernel(const float* __restrict__ raw, int N, int L, MsssimBetas betas,
                                                             int normalize, float* __restrict__ vals,
                                                             float* __restrict__ per_image, float* __restrict__ total,
                                                             float total_scale, float* __restrict__ factors) {
  __shared__ double wsum[4];
  double mine = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    double v[DSR_MSSSIM_MAX_SCALES];
    double out = 1.0;
#pragma unroll
    for (int s = 0; s < DSR_MSSSIM_MAX_SCALES; ++s) {
      if (s < L) {
        const float r = raw[(size_t)s * N + n];
        const float x = normalize == 1 ? fmaxf(r, 0.f) : normalize == 2 ? (r + 1.f) * 0.5f : r;
        if (vals) vals[(size_t)s * N + n] = x;
        v[s] = (double)x;
        out *= pow(v[s], (double)betas.b[s]);
      }
    }
    if (per_image) per_image[n] = (float)out;
    if (factors) {
#pragma unroll
      for (int s = 0; s < DSR_MSSSIM_MAX_SCALES; ++s) {
        if (s < L) {
          double f = (double)betas.b[s] * out / v[s];
          if (normalize == 1 && !(v[s] > 0.0)) f = 0.0;
          if (normalize == 2) f *= 0.5;
          factors[(size_t)s * N + n] = (float)f;
        }
      }
    }
    mine += (double)(float)out;
  }
  mine = wave_sum(mine);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0 && total) total[0] = (float)((double)total_scale * ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])));
}

extern "C" int dsr_msssim_combine(const float* raw, int N, int L, const float* betas, int normalize, float* vals,
                                  float* per_image, float* total, float total_scale, float* factors, dsr_stream_t st) {
  DSR_REQUIRE(raw && betas, "msssim_combine: null pointer");
  DSR_REQUIRE(per_image || total, "msssim_combine: neither per-image values nor a total are asked for");
  DSR_REQUIRE(N >= 1, "msssim_combine: %d images", N);
  DSR_REQUIRE(L >= 1 && L <= DSR_MSSSIM_MAX_SCALES, "msssim_combine: %d scales (1 .. %d)", L, DSR_MSSSIM_MAX_SCALES);
  DSR_REQUIRE(normalize >= 0 && normalize <= 2, "msssim_combine: normalize %d (0 none, 1 relu, 2 simple)", normalize);
  MsssimBetas bt;
  for (int s = 0; s < DSR_MSSSIM_MAX_SCALES; ++s) {
    bt.b[s] = s < L ? betas[s] : 1.f;
    DSR_REQUIRE(bt.b[s] > 0.f && bt.b[s] < INFINITY, "msssim_combine: betas[%d] must be positive and finite", s);
  }
  hipLaunchKernelGGL(msssim_combine_kernel, dim3(1), dim3(256), 0, st, raw, N, L, bt, normalize, vals, per_image, total,
                     total_scale, factors);
  return dsr_launch_status("dsr_msssim_combine");
}

// ---- one scale of the backward (ssim_bwd_kernel<true>, see there)
extern "C" int dsr_msssim_bwd_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2,
                                  const float* g, const float* w_sim, const float* w_cs, const float* coarse1,
                                  const float* coarse2, float* grad1, float* grad2, dsr_stream_t st) {
  DSR_REQUIRE(img1 && img2 && g, "msssim_bwd: null pointer");
  DSR_REQUIRE(w_sim || w_cs, "msssim_bwd: neither the SSIM nor the contrast-structure weights are given");
  DSR_REQUIRE(grad1 || grad2, "msssim_bwd: neither image's gradient is asked for");
  DSR_REQUIRE((!coarse1 || grad1) && (!coarse2 || grad2), "msssim_bwd: a coarse gradient without its image's gradient");
  DSR_REQUIRE(N >= 1 && C >= 1, "msssim_bwd: %d images of %d planes", N, C);
  DSR_REQUIRE(H >= SSIM_K && W >= SSIM_K, "msssim_bwd: image %dx%d smaller than the 11x11 window", H, W);
  DSR_REQUIRE(ssim_consts_ok(c1, c2), "msssim_bwd: c1 and c2 must be positive and finite (data_range > 0)");
  const int tiles_y = (H + SB_T - 1) / SB_T, tiles_x = (W + SB_T - 1) / SB_T;
  const long long blocks = (long long)N * C * tiles_y * tiles_x;
  DSR_REQUIRE(blocks < (1ll << 31), "msssim_bwd: too many tiles");
  const int OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  const float inv_count = (float)(1.0 / ((double)C * OH * OW));
  hipLaunchKernelGGL(ssim_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, img1, img2, C, H, W, tiles_x, tiles_y,
                     c1, c2, ssim_gauss_window(), g, inv_count, grad1, grad2, w_sim, w_cs, coarse1, coarse2);
  return dsr_launch_status("dsr_msssim_bwd_f32");
}

extern "C" int dsr_msssim_bwd_blocks(int N, int C, int H, int W) {
  if (N < 1 || C < 1 || H < SSIM_K || W < SSIM_K) return 0;
  const long long b = (long long)N * C * ((H + SB_T - 1) / SB_T) * ((W + SB_T - 1) / SB_T);
  return b < (1ll << 31) ? (int)b : 0;
}

// ================================================================================ metrics.PeakSignalNoiseRatio
// One pass over preds and target: per block (PSNR_CHUNK elements of one image, 64 per thread, then tree sums) the sum of
// squared errors and the target's (min, max) as order-preserving keys (order_key).  The finalise folds them per image / per
// batch in double, in a fixed order.
#define PSNR_CHUNK 16384

template <bool V4>
__global__ __launch_bounds__(256) void psnr_stats_kernel(const float* __restrict__ p, const float* __restrict__ t, int E, int B,
                                                         float* __restrict__ partial_sse, unsigned* __restrict__ partial_keys) {
  __shared__ float red[4];
  __shared__ unsigned rmin[4], rmax[4];
  const int n = blockIdx.x / B, blk = blockIdx.x % B;
  const float* pn = p + (size_t)n * E;
  const float* tn = t + (size_t)n * E;
  float s = 0.f;
  unsigned kmin = 0xffffffffu, kmax = 0u;
  if constexpr (V4) {
    const int e4 = E / 4;
    const int base = blk * (PSNR_CHUNK / 4);
#pragma unroll 4
    for (int i = 0; i < PSNR_CHUNK / 4 / 256; ++i) {
      const int e = base + i * 256 + threadIdx.x;
      if (e < e4) {
        const float4 x = reinterpret_cast<const float4*>(pn)[e], y = reinterpret_cast<const float4*>(tn)[e];
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        s = fmaf(d0, d0, s);
        s = fmaf(d1, d1, s);
        s = fmaf(d2, d2, s);
        s = fmaf(d3, d3, s);
        const unsigned k0 = order_key(y.x), k1 = order_key(y.y), k2 = order_key(y.z), k3 = order_key(y.w);
        kmin = min(kmin, min(min(k0, k1), min(k2, k3)));
        kmax = max(kmax, max(max(k0, k1), max(k2, k3)));
      }
    }
  } else {
    const int base = blk * PSNR_CHUNK;
#pragma unroll 4
    for (int i = 0; i < PSNR_CHUNK / 256; ++i) {
      const int e = base + i * 256 + threadIdx.x;
      if (e < E) {
        const float y = tn[e], d = pn[e] - y;
        s = fmaf(d, d, s);
        const unsigned key = order_key(y);
        kmin = min(kmin, key);
        kmax = max(kmax, key);
      }
    }
  }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor(kmin, o, 64));
    kmax = max(kmax, (unsigned)__shfl_xor(kmax, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = s;
    rmin[threadIdx.x >> 6] = kmin;
    rmax[threadIdx.x >> 6] = kmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial_sse[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    partial_keys[2 * blockIdx.x] = min(min(rmin[0], rmin[1]), min(rmin[2], rmin[3]));
    partial_keys[2 * blockIdx.x + 1] = max(max(rmax[0], rmax[1]), max(rmax[2], rmax[3]));
  }
}

// per_image mode (per_image != null): per[n] = log_scale (2 ln range - ln(SSE_n / E)); value = value_scale * sum_n per[n];
//   state[0] += sum_n per[n], state[1] += N.
// batch mode: value = log_scale (2 ln r - ln(SSE / (N E))), r = range, or max(target max, 0) - min(target min, 0);
//   state[0] += SSE, state[1] += N E, state[2] = min(state[2], target min), state[3] = max(state[3], target max).
__global__ __launch_bounds__(1024) void psnr_finalize_kernel(const float* __restrict__ partial_sse,
                                                             const unsigned* __restrict__ partial_keys, int N, int B, int E,
                                                             int infer_range, float range, float log_scale,
                                                             float* __restrict__ per_image, float* __restrict__ value,
                                                             float value_scale, double* __restrict__ state) {
  __shared__ double wsum[16];
  __shared__ unsigned wmin[16], wmax[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double mine = 0.0;
  unsigned kmin = 0xffffffffu, kmax = 0u;
  for (int n = wave; n < N; n += 16) {
    double s = 0.0;
    for (int k = lane; k < B; k += 64) {
      const size_t j = (size_t)n * B + k;
      s += (double)partial_sse[j];
      kmin = min(kmin, partial_keys[2 * j]);
      kmax = max(kmax, partial_keys[2 * j + 1]);
    }
    s = wave_sum(s);
    if (per_image) {
      const double v = (double)log_scale * (2.0 * log((double)range) - log(s / (double)E));
      if (lane == 0) per_image[n] = (float)v;
      mine += v;
    } else {
      mine += s;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor(kmin, o, 64));
    kmax = max(kmax, (unsigned)__shfl_xor(kmax, o, 64));
  }
  if (lane == 0) {
    wsum[wave] = mine;
    wmin[wave] = kmin;
    wmax[wave] = kmax;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double acc = 0.0;
  unsigned mn = 0xffffffffu, mx = 0u;
  for (int w = 0; w < 16; ++w) {
    acc += wsum[w];
    mn = min(mn, wmin[w]);
    mx = max(mx, wmax[w]);
  }
  if (per_image) {
    if (value) value[0] = (float)((double)value_scale * acc);
    if (state) {
      state[0] += acc;
      state[1] += (double)N;
    }
    return;
  }
  const double lo = (double)order_unkey(mn), hi = (double)order_unkey(mx), cnt = (double)N * (double)E;
  const double r = infer_range ? fmax(hi, 0.0) - fmin(lo, 0.0) : (double)range;
  if (value) value[0] = (float)((double)log_scale * (2.0 * log(r) - log(acc / cnt)));
  if (state) {
    state[0] += acc;
    state[1] += cnt;
    state[2] = fmin(state[2], lo);
    state[3] = fmax(state[3], hi);
  }
}

// state[0] += sum_n per[n] (fixed order, double), state[1] += N
__global__ __launch_bounds__(64) void metric_accumulate_kernel(const float* __restrict__ per, int N, double* __restrict__ state) {
  double s = 0.0;
  for (int n = threadIdx.x; n < N; n += 64) s += (double)per[n];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    state[0] += s;
    state[1] += (double)N;
  }
}

// mode 0: state[0]; 1: state[0] / state[1]; 2: PSNR of the running (SSE, count, min, max)
__global__ void metric_compute_kernel(const double* __restrict__ state, int mode, int infer_range, float range, float log_scale,
                                      float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double v;
  if (mode == 0) {
    v = state[0];
  } else if (mode == 1) {
    v = state[0] / state[1];
  } else {
    const double r = infer_range ? state[3] - state[2] : (double)range;
    v = (double)log_scale * (2.0 * log(r) - log(state[0] / state[1]));
  }
  out[0] = (float)v;
}

static bool metric_range_ok(int infer_range, float range) {
  return infer_range || (range > 0.f && range < INFINITY);     // false for NaN too
}

extern "C" int dsr_psnr_blocks(int N, int E) {
  if (N < 1 || E < 1) return 0;
  const long long b = (long long)N * ((E + PSNR_CHUNK - 1) / PSNR_CHUNK);
  return b < (1ll << 30) ? (int)b : 0;
}

extern "C" int dsr_psnr_stats_f32(const float* preds, const float* target, int N, int E, float* partial_sse,
                                  unsigned* partial_keys, dsr_stream_t st) {
  DSR_REQUIRE(preds && target && partial_sse && partial_keys, "psnr_stats: null pointer");
  DSR_REQUIRE(N >= 1 && E >= 1, "psnr_stats: %d images of %d elements", N, E);
  const int blocks = dsr_psnr_blocks(N, E);
  DSR_REQUIRE(blocks > 0, "psnr_stats: too many elements");
  const int B = blocks / N;
  const bool v4 = E % 4 == 0 && ((uintptr_t)preds & 15) == 0 && ((uintptr_t)target & 15) == 0;
  if (v4)
    hipLaunchKernelGGL(psnr_stats_kernel<true>, dim3(blocks), dim3(256), 0, st, preds, target, E, B, partial_sse, partial_keys);
  else
    hipLaunchKernelGGL(psnr_stats_kernel<false>, dim3(blocks), dim3(256), 0, st, preds, target, E, B, partial_sse, partial_keys);
  return dsr_launch_status("dsr_psnr_stats_f32");
}

extern "C" int dsr_psnr_finalize(const float* partial_sse, const unsigned* partial_keys, int N, int E, int infer_range,
                                 float data_range, float log_scale, float* per_image, float* value, float value_scale,
                                 double* state, dsr_stream_t st) {
  DSR_REQUIRE(partial_sse && partial_keys, "psnr_finalize: null pointer");
  DSR_REQUIRE(per_image || value, "psnr_finalize: neither per-image values nor a value are asked for");
  DSR_REQUIRE(N >= 1 && E >= 1, "psnr_finalize: %d images of %d elements", N, E);
  DSR_REQUIRE(metric_range_ok(infer_range, data_range), "psnr_finalize: data_range must be positive and finite");
  DSR_REQUIRE(!(per_image && infer_range), "psnr_finalize: per-image values need a given data_range");
  DSR_REQUIRE(log_scale != 0.f && fabsf(log_scale) < INFINITY, "psnr_finalize: bad log scale (base must be positive, not 1)");
  const int blocks = dsr_psnr_blocks(N, E);
  DSR_REQUIRE(blocks > 0, "psnr_finalize: too many elements");
  hipLaunchKernelGGL(psnr_finalize_kernel, dim3(1), dim3(1024), 0, st, partial_sse, partial_keys, N, blocks / N, E,
                     infer_range ? 1 : 0, data_range, log_scale, per_image, value, value_scale, state);
  return dsr_launch_status("dsr_psnr_finalize");
}

extern "C" int dsr_metric_accumulate(const float* per_image, int N, double* state, dsr_stream_t st) {
  DSR_REQUIRE(per_image && state, "metric_accumulate: null pointer");
  DSR_REQUIRE(N >= 1, "metric_accumulate: %d images", N);
  hipLaunchKernelGGL(metric_accumulate_kernel, dim3(1), dim3(64), 0, st, per_image, N, state);
  return dsr_launch_status("dsr_metric_accumulate");
}

extern "C" int dsr_metric_compute(const double* state, int mode, int infer_range, float data_range, float log_scale, float* out,
                                  dsr_stream_t st) {
  DSR_REQUIRE(state && out, "metric_compute: null pointer");
  DSR_REQUIRE(mode >= 0 && mode <= 2, "metric_compute: mode %d (0 sum, 1 mean, 2 psnr)", mode);
  DSR_REQUIRE(mode != 2 || metric_range_ok(infer_range, data_range), "metric_compute: data_range must be positive and finite");
  DSR_REQUIRE(mode != 2 || (log_scale != 0.f && fabsf(log_scale) < INFINITY), "metric_compute: bad log scale (base must be positive, not 1)");
  hipLaunchKernelGGL(metric_compute_kernel, dim3(1), dim3(64), 0, st, state, mode, infer_range ? 1 : 0, data_range, log_scale,
                     out);
  return dsr_launch_status("dsr_metric_compute");
}

// ---- measurement aid: (shader-clock cycles, 100 MHz real-time ticks) pairs, one per XCD.  Two samples around a region give
// the clock the chip actually held there: MI355X lowers its shader clock under load (tools/clock_probe.hip: a register-only
// MFMA loop on every CU runs at 1.22-1.28 GHz, not 2.4), which is what a fraction "of the 2.5 PFLOP/s peak" is really
// measured against.  s_memtime counters of different XCDs are not synchronised with each other, so every block files its
// pair under its own XCD (HW_REG_XCC_ID) and the host differences samples of the SAME XCD only.
__global__ void clock_sample_kernel(unsigned long long* __restrict__ out) {
  if (threadIdx.x == 0) {
    const unsigned xcc = __builtin_amdgcn_s_getreg((20 /* HW_REG_XCC_ID */) | (0 << 6) | ((4 - 1) << 11)) & 7u;
    out[2 * xcc] = __builtin_amdgcn_s_memtime();
    out[2 * xcc + 1] = __builtin_amdgcn_s_memrealtime();
  }
}
extern "C" int dsr_clock_sample(unsigned long long* out16, dsr_stream_t st) {
  DSR_REQUIRE(out16, "clock_sample: null pointer");
  hipLaunchKernelGGL(clock_sample_kernel, dim3(64), dim3(64), 0, st, out16);     // 64 blocks: every XCD gets some
  return dsr_launch_status("dsr_clock_sample");
}
