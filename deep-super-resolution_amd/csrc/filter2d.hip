// Per-sample 2-D filter of an fp32 batch (BasicSR's filter2D): the blur of the second-order Real-ESRGAN degradation.
//   y[b][c][Y][X] = sum_{i,j} k[b][i][j] * x[b][c][refl(Y + i - r)][refl(X + j - r)],   r = ks / 2
// a correlation; refl is torch's 'reflect' (-1 -> 1, H -> H - 2: reflect_index of degrade.hip).  Per output, in this order:
//   acc = 0;  for i, for j:  acc = fmaf(k[b][i][j], x[b][c][refl(Y + i - r)][refl(X + j - r)], acc)
// i.e. the chain of degrade_kernel at scale 1 on floats.  The chain does not depend on the tile, so a tile equals that region
// of any other tiling bit for bit.  A tap whose weight is 0 leaves a finite chain as it is (fmaf(0, v, acc) == acc: acc starts
// at +0 and a sum that is exactly zero rounds to +0), which is what the two shortcuts below rest on; an image with Inf / NaN in
// it is outside the definition.  No atomics, nothing that depends on the order blocks run in.
//
// filter2d_kernel: a block of 256 threads owns a 32 x 32 tile of up to three planes of one sample.  Thread (ty, tx) = (tid / 8,
// tid % 8) owns the 4 pixels 4 tx .. 4 tx + 3 of row ty in each plane: 12 accumulators.
//   * The weights go into an LDS table wl[21][24], zero beyond ks x ks, read back as 16-byte broadcasts.  21 threads then mark
//     the tap rows and columns that hold a non-zero weight: the tap loops run over rows [i0, i1) and the columns [jc0, jc1),
//     jc0 rounded down and jc1 up to a multiple of 4 (the added taps have weight 0).  A 7 x 7 kernel padded to 21 x 21, the
//     common case of the pipeline, costs 7 x 8 taps.
//   * Only the footprint those taps read is staged: rows [i0, th - 1 + i1), columns [jc0, jc1 + 32), as fp32, planar, 64
//     floats per row.  Columns past the last one a real tap of the tile reads are written as 0, not read from the image.
//   * Per tap row a thread slides a window over its footprint row: it keeps the previous 16-byte vector of each plane, loads
//     the next, and does 4 taps x 4 pixels = 16 fmaf per 16-byte LDS read (window floats p + q, pixel p, tap q).
//   * A wave's 16-byte reads touch 8 rows of 8 vectors.  With 64-float rows every row would start on bank 0 and the 16-lane
//     groups of a 16-byte read (lanes of two or four neighbouring rows) would meet on the same 8 slots; odd footprint rows
//     are therefore stored with their column XORed by 32, which puts them on the other half of the 64 banks.
// LDS: 3 x 52 x 64 x 4 B = 39 KB of footprint + 2 KB of weights, under the 64 KB a block gets without asking.
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int KS_MAX = 21;
constexpr int WL_PITCH = 24;                  // KS_MAX rounded up to the 4-tap chunks
constexpr int TH = 32, TW = 32, PX = 4;       // tile; pixels per thread along a row
constexpr int NT = TH * (TW / PX);            // 256
constexpr int CP = 3;                         // planes per block
constexpr int FH = TH + KS_MAX - 1;           // 52 footprint rows
constexpr int PITCH = 64;                     // floats per footprint row: TW + WL_PITCH = 56 are used

__device__ __forceinline__ int reflect_index(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
  return min(max(i, 0), n - 1);
}
// where column fx of footprint row fy lives in its plane
__device__ __forceinline__ int fp_at(int fy, int fx) { return fy * PITCH + (fx ^ ((fy & 1) << 5)); }

__global__ __launch_bounds__(NT) void filter2d_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      const float* __restrict__ kernels, int C, int H, int W, int ks, int shared,
                                                      int tiles_x, int tiles_y, int groups) {
  __shared__ __attribute__((aligned(16))) float wl[KS_MAX * WL_PITCH];
  __shared__ __attribute__((aligned(16))) float fp[CP * FH * PITCH];
  __shared__ int row_on[KS_MAX], col_on[KS_MAX];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tile_x = bid % tiles_x;
  bid /= tiles_x;
  const int tile_y = bid % tiles_y;
  bid /= tiles_y;
  const int g = bid % groups, b = bid / groups;
  const int c0 = g * CP, nc = min(CP, C - c0);
  const int Y0 = tile_y * TH, X0 = tile_x * TW;
  const int th = min(TH, H - Y0), tw = min(TW, W - X0);
  const int r = ks >> 1;

  const float* __restrict__ kb = kernels + (shared ? 0 : (size_t)b * ks * ks);
  for (int n = tid; n < KS_MAX * WL_PITCH; n += NT) {
    const int i = n / WL_PITCH, j = n - i * WL_PITCH;
    wl[n] = (i < ks && j < ks) ? kb[i * ks + j] : 0.0f;
  }
  __syncthreads();
  if (tid < ks) {
    int ro = 0, co = 0;
    for (int t = 0; t < ks; ++t) {
      ro |= wl[tid * WL_PITCH + t] != 0.0f;
      co |= wl[t * WL_PITCH + tid] != 0.0f;
    }
    row_on[tid] = ro;
    col_on[tid] = co;
  }
  __syncthreads();
  int i0 = ks, i1 = 0, j0 = ks, j1 = 0;
  for (int t = 0; t < ks; ++t) {
    if (row_on[t]) i0 = min(i0, t), i1 = t + 1;
    if (col_on[t]) j0 = min(j0, t), j1 = t + 1;
  }
  if (i1 == 0) i0 = 0, j0 = 0;                 // an all-zero kernel: no taps, the output is 0
  const int jc0 = j0 & ~3, jc1 = (j1 + 3) & ~3;

  // the footprint: row fy is image row refl(Y0 - r + fy), column fx image column refl(X0 - r + fx)
  const int fy_end = th - 1 + i1, fx_end = jc1 + TW, fx_real = tw - 1 + ks;
  const int lane = tid & 63, wave = tid >> 6;
  for (int c = 0; c < nc; ++c) {
    const float* __restrict__ xp = x + ((size_t)b * C + c0 + c) * H * W;
    float* __restrict__ fpc = fp + c * FH * PITCH;
    for (int fy = i0 + wave; fy < fy_end; fy += NT / 64) {
      const float* __restrict__ srow = xp + (size_t)reflect_index(Y0 - r + fy, H) * W;
      const int fx = jc0 + lane;
      if (fx < fx_end) fpc[fp_at(fy, fx)] = fx < fx_real ? srow[reflect_index(X0 - r + fx, W)] : 0.0f;
    }
  }
  __syncthreads();

  const int ty = tid / (TW / PX), tx = tid % (TW / PX);
  if (ty >= th || PX * tx >= tw) return;
  float acc[CP][PX];
#pragma unroll
  for (int c = 0; c < CP; ++c)
#pragma unroll
    for (int p = 0; p < PX; ++p) acc[c][p] = 0.0f;
  for (int i = i0; i < i1; ++i) {
    const int fy = ty + i;
    const float* __restrict__ frow = fp + fy * PITCH;
    const int sw = (fy & 1) << 5;
    f32x4 prev[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < nc) prev[c] = *reinterpret_cast<const f32x4*>(frow + c * FH * PITCH + ((PX * tx + jc0) ^ sw));
    for (int m = jc0; m < jc1; m += 4) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + i * WL_PITCH + m);
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        if (c < nc) {
          const f32x4 next = *reinterpret_cast<const f32x4*>(frow + c * FH * PITCH + ((PX * tx + m + 4) ^ sw));
          const float win[8] = {prev[c].x, prev[c].y, prev[c].z, prev[c].w, next.x, next.y, next.z, next.w};
          const float wq[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int p = 0; p < PX; ++p) acc[c][p] = fmaf(wq[q], win[p + q], acc[c][p]);
          prev[c] = next;
        }
      }
    }
  }
  const int Y = Y0 + ty, X = X0 + PX * tx;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    if (c < nc) {
      float* __restrict__ out = y + (((size_t)b * C + c0 + c) * H + Y) * W + X;
#pragma unroll
      for (int p = 0; p < PX; ++p)
        if (X + p < W) out[p] = acc[c][p];
    }
  }
}
}  // namespace

extern "C" int dsr_filter2d_f32(const float* x, float* y, const float* kernels, int B, int C, int H, int W, int ks, int shared,
                                dsr_stream_t st) {
  if (!x || !y || !kernels) return dsr_fail(DSR_E_ARG, "filter2d_f32: null pointer");
  if (B < 1 || C < 1 || H < 1 || W < 1) return dsr_fail(DSR_E_ARG, "filter2d_f32: bad shape %dx%dx%dx%d", B, C, H, W);
  if (ks < 1 || ks > KS_MAX || !(ks & 1)) return dsr_fail(DSR_E_ARG, "filter2d_f32: kernel size %d is not an odd number in 1..%d", ks, KS_MAX);
  if (ks / 2 >= (H < W ? H : W)) return dsr_fail(DSR_E_ARG, "filter2d_f32: a %dx%d kernel cannot be reflected in a %dx%d image", ks, ks, H, W);
  const long long total = (long long)B * C * H * W;
  if (total >= (1ll << 31)) return dsr_fail(DSR_E_ARG, "filter2d_f32: B*C*H*W = %lld does not fit 31 bits", total);
  const char *xb = (const char*)x, *yb = (const char*)y;
  if (xb < yb + total * 4 && yb < xb + total * 4) return dsr_fail(DSR_E_ARG, "filter2d_f32: y overlaps x");
  if (shared != 0 && shared != 1) return dsr_fail(DSR_E_ARG, "filter2d_f32: shared flag %d", shared);
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH, groups = (C + CP - 1) / CP;
  const long long blocks = (long long)tiles_x * tiles_y * groups * B;      // <= B*C*H*W < 2^31
  hipLaunchKernelGGL(filter2d_kernel, dim3((unsigned)blocks), dim3(NT), 0, st, x, y, kernels, C, H, W, ks, shared, tiles_x, tiles_y,
                     groups);
  return dsr_launch_status("dsr_filter2d_f32");
}
