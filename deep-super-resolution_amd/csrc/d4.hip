// The eight flips / quarter turns of an image (the dihedral group D4) as coalesced tile kernels: training augmentation of the
// uint8 patch bank and geometric self-ensemble at inference (EDSR "+", Lim et al. 2017).
//   code k in 0..7, r = k % 4, m = k >= 4:   T_k(x) = rot90(flip(x, W) if m else x, r)
//   T_k(x)[i][j] = x[a][b] of an H x W source:  r = 0: (i, j)   1: (j, W-1-i)   2: (H-1-i, W-1-j)   3: (H-1-j, i);
//   with m the column is mirrored afterwards, b = W-1-b.  The result is H x W for even r and W x H for odd r.
//
//   d4_expand_kernel   T_k(src) for every k of a mask, one launch: a block stages one 64 x 64 source tile in LDS (row-wise
//                      read) and writes the tile's image under each code row-wise
//   d4_mean_kernel     dst = (sum over k of the mask, ascending, of T_k^-1(src_k)) * (1 / count): a block owns a 64 x 64 tile
//                      of dst, keeps it in registers (16 per thread) over the codes and stores it once.  The four codes that
//                      keep the axes are read straight from global memory (a row of dst is a row of src_k, forwards or
//                      backwards); the four that swap them are read row-wise into LDS and turned there.
//   patch_batch_d4_kernel   patch_batch_kernel (data.hip) with a code per patch: the tile scheme over 3-byte pixels
// Every global access has consecutive lanes on consecutive addresses.  The LDS row is padded to an odd number of dwords
// (65 floats; 196 bytes = 49 dwords for the pixels), so the transposed read -- lane l in row l -- falls on 32 different banks
// in each 32-lane group, and so does the row-wise store.  fp32 sums only: adds in a fixed order and one multiply, nothing
// that could contract -- the result of d4_mean_kernel is defined bit for bit.
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int TILE = 64;
constexpr int PITCH = TILE + 1;            // floats per LDS row
constexpr int PIX_PITCH = TILE * 3 + 4;    // bytes per LDS row of RGB pixels: 49 dwords

// source position (a, b) of T_k(x)[i][j]; H, W are the SOURCE sizes
__device__ __forceinline__ void d4_source(int k, int H, int W, int i, int j, int& a, int& b) {
  const int r = k & 3;
  a = r == 0 ? i : (r == 1 ? j : (r == 2 ? H - 1 - i : H - 1 - j));
  b = r == 0 ? j : (r == 1 ? W - 1 - i : (r == 2 ? W - 1 - j : i));
  if (k & 4) b = W - 1 - b;
}

// The image under T_k of the source tile rows [a0, a0 + ah) x columns [b0, b0 + bw): origin (i0, j0) and extent eh x ew of
// that rectangle in the result
__device__ __forceinline__ void d4_image_tile(int k, int H, int W, int a0, int ah, int b0, int bw, int& i0, int& j0, int& eh, int& ew) {
  const int r = k & 3;
  const bool m = (k & 4) != 0;
  const int a_rev = H - a0 - ah, b_rev = W - b0 - bw;       // where the range starts once its axis is mirrored
  if (r == 0) {
    i0 = a0, j0 = m ? b_rev : b0;
  } else if (r == 1) {
    i0 = m ? b0 : b_rev, j0 = a0;
  } else if (r == 2) {
    i0 = a_rev, j0 = m ? b0 : b_rev;
  } else {
    i0 = m ? b_rev : b0, j0 = a_rev;
  }
  eh = (r & 1) ? bw : ah;
  ew = (r & 1) ? ah : bw;
}

// slot of code k among the codes of its parity (even r / odd r) that are set in mask, ascending
__device__ __forceinline__ int d4_slot(unsigned mask, int k) {
  const unsigned same = (k & 1) ? 0xAAu : 0x55u;
  return __popc(mask & same & ((1u << k) - 1u));
}

__global__ __launch_bounds__(256) void d4_expand_kernel(const float* __restrict__ src, int h, int w, unsigned mask,
                                                        float* __restrict__ dst_even, float* __restrict__ dst_odd, int planes) {
  __shared__ float tile[TILE * PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b0 = blockIdx.x * TILE, a0 = blockIdx.y * TILE, p = blockIdx.z;
  const int ah = min(TILE, h - a0), bw = min(TILE, w - b0);
  const size_t plane = (size_t)h * w;
  const float* __restrict__ s = src + (size_t)p * plane;
  for (int y = wave; y < ah; y += 4)
    if (lane < bw) tile[y * PITCH + lane] = s[(size_t)(a0 + y) * w + b0 + lane];
  __syncthreads();
  for (int k = 0; k < 8; ++k) {
    if (!(mask >> k & 1)) continue;
    int i0, j0, eh, ew;
    d4_image_tile(k, h, w, a0, ah, b0, bw, i0, j0, eh, ew);
    const int ow = (k & 1) ? h : w;                                  // row length of the result
    float* __restrict__ d = ((k & 1) ? dst_odd : dst_even) + ((size_t)d4_slot(mask, k) * planes + p) * plane;
    for (int y = wave; y < eh; y += 4) {
      if (lane < ew) {
        int a, b;
        d4_source(k, h, w, i0 + y, j0 + lane, a, b);
        d[(size_t)(i0 + y) * ow + j0 + lane] = tile[(a - a0) * PITCH + (b - b0)];
      }
    }
  }
}

// All loads of a tile are issued before the first one is used (8 codes x 16 values per thread in registers): the kernel is a
// pure stream, and with one tile-code in flight at a time it ran at half the rate (3.2 against 5+ TB/s at 3 x 2048 x 2048).
// Loads stay in flight across the barriers of the LDS turns; each use waits only for the loads issued before it.
__global__ __launch_bounds__(256) void d4_mean_kernel(const float* __restrict__ src_even, const float* __restrict__ src_odd, int planes,
                                                      int H, int W, unsigned mask, float scale, float* __restrict__ dst) {
  __shared__ float tile[2][TILE * PITCH];
  constexpr int RPT = TILE / 4;            // rows per thread
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b0 = blockIdx.x * TILE, a0 = blockIdx.y * TILE, p = blockIdx.z;
  const int ah = min(TILE, H - a0), bw = min(TILE, W - b0);
  const size_t plane = (size_t)H * W;
  float v[8][RPT];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!(mask >> k & 1)) continue;                                  // (block-uniform)
    const float* __restrict__ s = ((k & 1) ? src_odd : src_even) + ((size_t)d4_slot(mask, k) * planes + p) * plane;
    if (!(k & 1)) {
      // rows stay rows: dst[a][b] = src_k[i][j] with i = a or H-1-a, j = b or W-1-b -- each thread loads its own elements
      const int r = k & 3;
      const bool rev_j = ((k & 4) != 0) != (r == 2);
      const int bb = min(b0 + lane, W - 1);          // (threads off the edge load a clamped position and never store)
      const int j = rev_j ? W - 1 - bb : bb;
#pragma unroll
      for (int t = 0; t < RPT; ++t) {
        const int a = min(a0 + wave + 4 * t, H - 1);
        const int i = r == 0 ? a : H - 1 - a;
        v[k][t] = s[(size_t)i * W + j];
      }
    } else {
      // this block's tile of dst is the "source tile" of T_k and src_k (W x H: rows of H) holds its image: read that row-wise
      int i0, j0, eh, ew;
      d4_image_tile(k, H, W, a0, ah, b0, bw, i0, j0, eh, ew);
      const int j = j0 + min(lane, ew - 1);
#pragma unroll
      for (int t = 0; t < RPT; ++t) {
        const int i = i0 + min(wave + 4 * t, eh - 1);
        v[k][t] = s[(size_t)i * H + j];
      }
    }
  }
  float acc[RPT] = {};
  bool first = true;
  int buf = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!(mask >> k & 1)) continue;
    if (k & 1) {
      // turn the tile in LDS.  Two buffers, one barrier per code: whoever fills a buffer again has passed the barrier of the
      // code in between, which every thread reaches only after its reads of that buffer
      float* __restrict__ tl = tile[buf];
      buf ^= 1;
      int i0, j0, eh, ew;
      d4_image_tile(k, H, W, a0, ah, b0, bw, i0, j0, eh, ew);
#pragma unroll
      for (int t = 0; t < RPT; ++t) tl[(wave + 4 * t) * PITCH + lane] = v[k][t];
      __syncthreads();
#pragma unroll
      for (int t = 0; t < RPT; ++t) {
        // the position (i, j) of src_k that lands on dst[a][bb]: d4_source inverted for odd r
        const int y = wave + 4 * t;
        const int a = min(a0 + y, H - 1), bb = min(b0 + lane, W - 1);          // (clamped: lanes off the edge read, not use)
        const int b = (k & 4) ? W - 1 - bb : bb;
        const int i = (k & 3) == 1 ? W - 1 - b : b;
        const int j = (k & 3) == 1 ? a : H - 1 - a;
        v[k][t] = tl[(i - i0) * PITCH + (j - j0)];
      }
    }
#pragma unroll
    for (int t = 0; t < RPT; ++t) acc[t] = first ? v[k][t] : acc[t] + v[k][t];
    first = false;
  }
  float* __restrict__ d = dst + (size_t)p * plane;
#pragma unroll
  for (int t = 0; t < RPT; ++t) {
    const int y = wave + 4 * t;
    if (y < ah && lane < bw) d[(size_t)(a0 + y) * W + b0 + lane] = acc[t] * scale;
  }
}

struct PatchBatchD4 {
  const unsigned char* img[DSR_PATCH_BATCH_MAX];
  int width[DSR_PATCH_BATCH_MAX];       // row pitch of the source image in pixels
  int top[DSR_PATCH_BATCH_MAX], left[DSR_PATCH_BATCH_MAX];
  unsigned char xform[DSR_PATCH_BATCH_MAX];
};

// the arithmetic of patch_batch_kernel (data.hip), statement for statement: both round alike
__device__ __forceinline__ float patch_scale(unsigned char u, int mode) {
  float v = (float)u / 255.0f;                                // torchvision ToTensor (dataset.py:59-60)
  if (mode == DSR_PATCH_LR_REF) {
    v = v / 255.0f;                                           // dataset.py:152
  } else if (mode == DSR_PATCH_HR_REF) {
    v = v / 255.0f;                                           // :155
    v = v * 2.0f;                                             // :156
    v = v - 1.0f;                                             // :157
  } else if (mode == DSR_PATCH_HR_UNIT) {
    v = v * 2.0f;
    v = v - 1.0f;
  }
  return v;
}

// out[b][c] = T_k(patch_b[c]): a block stages a 64 x 64 pixel tile of the patch as bytes (consecutive lanes = consecutive bytes
// of an image row) and writes its image, channel by channel, with consecutive lanes on consecutive floats of an output row
__global__ __launch_bounds__(256) void patch_batch_d4_kernel(const PatchBatchD4 t, int ph, int pw, int mode, float* __restrict__ out) {
  __shared__ unsigned char tile[TILE * PIX_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (pw + TILE - 1) / TILE;
  const int b0 = (blockIdx.x % tiles_x) * TILE, a0 = (blockIdx.x / tiles_x) * TILE, pb = blockIdx.y;
  const int ah = min(TILE, ph - a0), bw = min(TILE, pw - b0);
  const int k = t.xform[pb];
  const unsigned char* __restrict__ s = t.img[pb] + ((size_t)(t.top[pb] + a0) * t.width[pb] + t.left[pb] + b0) * 3;
  const size_t pitch = (size_t)t.width[pb] * 3;
  for (int y = wave; y < ah; y += 4)
    for (int x = lane; x < bw * 3; x += 64) tile[y * PIX_PITCH + x] = s[y * pitch + x];
  __syncthreads();
  int i0, j0, eh, ew;
  d4_image_tile(k, ph, pw, a0, ah, b0, bw, i0, j0, eh, ew);
  const int ow = (k & 1) ? ph : pw;                                  // == pw: odd r only with ph == pw
  const size_t plane = (size_t)ph * pw;
  float* __restrict__ o = out + (size_t)pb * 3 * plane;
  for (int c = 0; c < 3; ++c) {
    for (int y = wave; y < eh; y += 4) {
      if (lane < ew) {
        int a, b;
        d4_source(k, ph, pw, i0 + y, j0 + lane, a, b);
        o[c * plane + (size_t)(i0 + y) * ow + j0 + lane] = patch_scale(tile[(a - a0) * PIX_PITCH + (b - b0) * 3 + c], mode);
      }
    }
  }
}

int popcount8(int mask) {
  int n = 0;
  for (int k = 0; k < 8; ++k) n += mask >> k & 1;
  return n;
}
}  // namespace

extern "C" int dsr_d4_expand_f32(const float* src, int planes, int h, int w, int mask, float* dst_even, float* dst_odd,
                                 dsr_stream_t st) {
  DSR_REQUIRE(src && planes > 0 && h > 0 && w > 0, "d4_expand_f32: null source or non-positive size");
  DSR_REQUIRE(mask > 0 && mask <= 0xFF, "d4_expand_f32: mask 0x%x is not a non-empty set of the codes 0..7", mask);
  DSR_REQUIRE((!(mask & 0x55) || dst_even) && (!(mask & 0xAA) || dst_odd), "d4_expand_f32: null destination for a code of mask 0x%x", mask);
  const int ty = (h + TILE - 1) / TILE;
  if (planes > 65535 || ty > 65535) return dsr_fail(DSR_E_UNSUPPORTED, "d4_expand_f32: %d planes of %d rows exceed the grid", planes, h);
  hipLaunchKernelGGL(d4_expand_kernel, dim3((w + TILE - 1) / TILE, ty, planes), dim3(256), 0, st, src, h, w, (unsigned)mask, dst_even,
                     dst_odd, planes);
  return dsr_launch_status("dsr_d4_expand_f32");
}

extern "C" int dsr_d4_mean_f32(const float* src_even, const float* src_odd, int planes, int H, int W, int mask, float* dst,
                               dsr_stream_t st) {
  DSR_REQUIRE(dst && planes > 0 && H > 0 && W > 0, "d4_mean_f32: null destination or non-positive size");
  DSR_REQUIRE(mask > 0 && mask <= 0xFF, "d4_mean_f32: mask 0x%x is not a non-empty set of the codes 0..7", mask);
  DSR_REQUIRE((!(mask & 0x55) || src_even) && (!(mask & 0xAA) || src_odd), "d4_mean_f32: null source for a code of mask 0x%x", mask);
  const int ty = (H + TILE - 1) / TILE;
  if (planes > 65535 || ty > 65535) return dsr_fail(DSR_E_UNSUPPORTED, "d4_mean_f32: %d planes of %d rows exceed the grid", planes, H);
  const float scale = 1.0f / (float)popcount8(mask);
  hipLaunchKernelGGL(d4_mean_kernel, dim3((W + TILE - 1) / TILE, ty, planes), dim3(256), 0, st, src_even, src_odd, planes, H, W,
                     (unsigned)mask, scale, dst);
  return dsr_launch_status("dsr_d4_mean_f32");
}

extern "C" int dsr_patch_batch_u8_d4(int count, const unsigned char* const* images, const int* heights, const int* widths,
                                     const int* tops, const int* lefts, const int* xforms, int ph, int pw, int mode, float* out,
                                     dsr_stream_t st) {
  if (count <= 0 || !images || !heights || !widths || !tops || !lefts || !xforms || !out || ph <= 0 || pw <= 0)
    return dsr_fail(DSR_E_ARG, "patch_batch_u8_d4: null table or bad shape");
  if (mode < DSR_PATCH_UNIT || mode > DSR_PATCH_HR_UNIT) return dsr_fail(DSR_E_ARG, "patch_batch_u8_d4: mode %d", mode);
  for (int i = 0; i < count; ++i) {
    if (!images[i]) return dsr_fail(DSR_E_ARG, "patch_batch_u8_d4: null image %d", i);
    if (tops[i] < 0 || lefts[i] < 0 || tops[i] + ph > heights[i] || lefts[i] + pw > widths[i])
      return dsr_fail(DSR_E_ARG, "patch_batch_u8_d4: patch %d (%d,%d)+(%d,%d) leaves its %dx%d image", i, tops[i], lefts[i], ph, pw,
                      heights[i], widths[i]);
    if (xforms[i] < 0 || xforms[i] > 7) return dsr_fail(DSR_E_ARG, "patch_batch_u8_d4: transform code %d of patch %d is not in 0..7", xforms[i], i);
    if ((xforms[i] & 1) && ph != pw)
      return dsr_fail(DSR_E_ARG, "patch_batch_u8_d4: code %d of patch %d turns a %dx%d patch by a quarter", xforms[i], i, ph, pw);
  }
  const size_t per = (size_t)3 * ph * pw;
  const unsigned tiles = (unsigned)((ph + TILE - 1) / TILE) * (unsigned)((pw + TILE - 1) / TILE);
  for (int i0 = 0; i0 < count; i0 += DSR_PATCH_BATCH_MAX) {
    PatchBatchD4 t;
    const int n = count - i0 < DSR_PATCH_BATCH_MAX ? count - i0 : DSR_PATCH_BATCH_MAX;
    for (int j = 0; j < n; ++j) {
      t.img[j] = images[i0 + j];
      t.width[j] = widths[i0 + j];
      t.top[j] = tops[i0 + j];
      t.left[j] = lefts[i0 + j];
      t.xform[j] = (unsigned char)xforms[i0 + j];
    }
    hipLaunchKernelGGL(patch_batch_d4_kernel, dim3(tiles, n), dim3(256), 0, st, t, ph, pw, mode, out + (size_t)i0 * per);
  }
  return dsr_launch_status("dsr_patch_batch_u8_d4");
}
