// Blind degradation of device-resident uint8 RGB images: LR = quant(clip((HR (*) k) sampled every s-th pixel + sigma * z)),
// with a different blur kernel k and noise level sigma per sample (SRMD, IKC, KernelGAN, BSRGAN's classical degradation, the
// first-order stage of Real-ESRGAN).  The degrading counterpart of patch_batch_d4_kernel (d4.hip): LR training patches are
// cut from the HR images of the bank with a fresh degradation per sample per step, in one launch.
//
// LR pixel (Y, X) of the LR grid, channel c, r = ks / 2, taps in row-major order, one fused multiply-add each:
//   acc = 0;  for i, for j:  acc = fmaf(k[i][j], (float)HR[refl(s*Y + offset + i - r, H)][refl(s*X + offset + j - r, W)][c], acc)
//   if noise:    acc = fmaf(noise_std[b], z[b][c][y][x], acc)          z at the OUTPUT position (after the D4 code)
//   acc = min(max(acc, 0), 255);  if quantise: acc = rintf(acc)        (half to even, as torch.round)
//   v = acc / 255.0f, then the `mode` statements of patch_batch_kernel (data.hip)
// refl reflects at the borders of the WHOLE image without repeating the edge (-1 -> 1, H -> H - 2: torch's 'reflect').  The
// tap order does not depend on the tile or on where a patch lies, so a patch equals the same region of the whole-image
// result (dsr_degrade_image_u8, the same kernel with a byte store) bit for bit.
//
// degrade_kernel<S>: a block owns a TH x 16 tile of LR pixels of one sample (TH = 16 up to scale 4, 8 above: the footprint
// of 16 x 16 at s = 8, ks = 21 is 148 x 148 x 3 = 65.7 KB, more than the 64 KB a block gets without asking), one thread per
// pixel.  The uint8 HR footprint (S*TH + ks - 1) x (S*16 + ks - 1) x 3 is staged in LDS once, consecutive lanes reading
// consecutive bytes of an image row, and so are the ks * ks weights (read back as a broadcast).  In LDS the three channels
// are planar and the columns of a row are split by their phase x % S:
//     byte (c, fy, x) at  c * FH * PITCH + fy * PITCH + (x % S) * QP + x / S
// Tap j of the 16 lanes of a tile row (columns S*tx + j) is then 16 CONSECUTIVE bytes (4-5 dwords, lanes on one dword
// broadcast) instead of 16 bytes 3*S apart -- at S = 8 interleaved pixels would put the 16 lanes on 8 banks.  QP is padded
// so that the next tile row (S rows = S * PITCH bytes on) starts 5..27 dwords further round the 32 banks: the two tile rows
// of a 32-lane group do not meet.  Each thread runs the tap loop from LDS into three fp32 accumulators; the D4 code only
// moves the store (and the noise read), which for a quarter turn writes columns -- 3 stores against 3 * ks * ks LDS reads.
// No atomics, no scratch, nothing that depends on the order blocks run in.
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int KS_MAX = 21;
constexpr int TW = 16;
constexpr int tile_rows(int S) { return S <= 4 ? 16 : 8; }
constexpr int phase_cols(int S) { return TW + (KS_MAX - 1 + S - 1) / S; }       // columns of one phase: x / S < this
// columns per phase in LDS: the smallest count >= phase_cols(S) that puts S image rows 5..27 dwords (20..108 bytes) round the banks
constexpr int phase_pitch(int S) {
  int qp = phase_cols(S);
  while ((S * S * qp) % 128 < 20 || (S * S * qp) % 128 > 108) ++qp;
  return qp;
}

struct DegradeBatch {
  const unsigned char* img[DSR_PATCH_BATCH_MAX];
  int height[DSR_PATCH_BATCH_MAX], width[DSR_PATCH_BATCH_MAX];
  int top[DSR_PATCH_BATCH_MAX], left[DSR_PATCH_BATCH_MAX];       // in LR pixels
  unsigned char xform[DSR_PATCH_BATCH_MAX];
};

// the arithmetic of patch_batch_kernel (data.hip) after its first division, statement for statement: both round alike
__device__ __forceinline__ float degrade_scale(float v, int mode) {
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

// torch's 'reflect' for an index at most n - 1 outside [0, n); clamped, so that no index can leave the image
__device__ __forceinline__ int reflect_index(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
  return min(max(i, 0), n - 1);
}

// where T_k puts element (a, b) of an H x W source: the gather table of d4.hip (d4_source) solved for (i, j)
__device__ __forceinline__ void d4_dest(int k, int H, int W, int a, int b, int& i, int& j) {
  const int r = k & 3;
  if (k & 4) b = W - 1 - b;
  i = r == 0 ? a : (r == 1 ? W - 1 - b : (r == 2 ? H - 1 - a : b));
  j = r == 0 ? b : (r == 1 ? a : (r == 2 ? W - 1 - b : H - 1 - a));
}

// out_f: fp32 [count][3][ph][pw] (scaled by `mode`) or, when null, out_u8: uint8 [ph][pw][3] of sample 0 (always rounded)
template <int S>
__global__ __launch_bounds__(tile_rows(S) * TW) void degrade_kernel(const DegradeBatch t, int ph, int pw, int offset,
                                                                    const float* __restrict__ kernels, int ks,
                                                                    const float* __restrict__ noise, const float* __restrict__ noise_std,
                                                                    int quantise, int mode, float* __restrict__ out_f,
                                                                    unsigned char* __restrict__ out_u8) {
  constexpr int TH = tile_rows(S), NT = TH * TW;
  constexpr int FH = S * TH + KS_MAX - 1;                      // footprint rows at ks = 21
  constexpr int QP = phase_pitch(S), PITCH = S * QP;           // bytes per footprint row of one channel
  __shared__ float wl[KS_MAX * KS_MAX];
  __shared__ unsigned char fp[3 * FH * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (pw + TW - 1) / TW;
  const int a0 = (blockIdx.x / tiles_x) * TH, b0 = (blockIdx.x % tiles_x) * TW, pb = blockIdx.y;
  const int ah = min(TH, ph - a0), bw = min(TW, pw - b0);      // the LR pixels of this tile that exist
  const int H = t.height[pb], W = t.width[pb];
  const int r = ks >> 1;
  const int rows = S * (ah - 1) + ks, cols = S * (bw - 1) + ks;        // the footprint that those pixels read
  const int y0 = S * (t.top[pb] + a0) + offset - r, x0 = S * (t.left[pb] + b0) + offset - r;
  const unsigned char* __restrict__ img = t.img[pb];
  for (int n = tid; n < ks * ks; n += NT) wl[n] = kernels[(size_t)pb * ks * ks + n];
  for (int fy = wave; fy < rows; fy += NT / 64) {
    const unsigned char* __restrict__ srow = img + (size_t)reflect_index(y0 + fy, H) * W * 3;
    unsigned char* __restrict__ drow = fp + fy * PITCH;
    for (int fb = lane; fb < cols * 3; fb += 64) {             // consecutive lanes = consecutive bytes of the image row
      const int x = fb / 3, c = fb - 3 * x;
      drow[c * FH * PITCH + (x % S) * QP + x / S] = srow[(size_t)reflect_index(x0 + x, W) * 3 + c];
    }
  }
  __syncthreads();
  const int ty = tid / TW, tx = tid % TW;
  if (ty >= ah || tx >= bw) return;
  float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
  const unsigned char* __restrict__ p = fp + S * ty * PITCH + tx;
  const float* __restrict__ w = wl;
  for (int i = 0; i < ks; ++i) {
    int phase = 0, q = 0;                                      // j % S, j / S
    for (int j = 0; j < ks; ++j) {
      const float k = w[j];
      const unsigned char* __restrict__ e = p + phase * QP + q;
      acc0 = fmaf(k, (float)e[0], acc0);
      acc1 = fmaf(k, (float)e[FH * PITCH], acc1);
      acc2 = fmaf(k, (float)e[2 * FH * PITCH], acc2);
      if (++phase == S) phase = 0, ++q;
    }
    p += PITCH;
    w += ks;
  }
  const int a = a0 + ty, b = b0 + tx;                          // position in the patch
  int i = a, j = b;
  if (out_f) d4_dest(t.xform[pb], ph, pw, a, b, i, j);
  const size_t plane = (size_t)ph * pw;
  const size_t o = (size_t)i * pw + j;                         // (a quarter turn only with ph == pw)
  float acc[3] = {acc0, acc1, acc2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = acc[c];
    if (noise) v = fmaf(noise_std[pb], noise[((size_t)pb * 3 + c) * plane + o], v);
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    if (out_f) {
      if (quantise) v = rintf(v);
      out_f[((size_t)pb * 3 + c) * plane + o] = degrade_scale(v / 255.0f, mode);
    } else {
      out_u8[o * 3 + c] = (unsigned char)rintf(v);
    }
  }
}

template <int S>
void launch_one(const DegradeBatch& t, int n, int ph, int pw, int offset, const float* kernels, int ks, const float* noise,
                const float* noise_std, int quantise, int mode, float* out_f, unsigned char* out_u8, dsr_stream_t st) {
  constexpr int TH = tile_rows(S);
  const unsigned tiles = (unsigned)((ph + TH - 1) / TH) * (unsigned)((pw + TW - 1) / TW);
  hipLaunchKernelGGL(degrade_kernel<S>, dim3(tiles, n), dim3(TH * TW), 0, st, t, ph, pw, offset, kernels, ks, noise, noise_std,
                     quantise, mode, out_f, out_u8);
}

void launch(int scale, const DegradeBatch& t, int n, int ph, int pw, int offset, const float* kernels, int ks, const float* noise,
            const float* noise_std, int quantise, int mode, float* out_f, unsigned char* out_u8, dsr_stream_t st) {
#define DSR_DEGRADE_CASE(S) \
  case S: launch_one<S>(t, n, ph, pw, offset, kernels, ks, noise, noise_std, quantise, mode, out_f, out_u8, st); break;
  switch (scale) {
    DSR_DEGRADE_CASE(1) DSR_DEGRADE_CASE(2) DSR_DEGRADE_CASE(3) DSR_DEGRADE_CASE(4)
    DSR_DEGRADE_CASE(5) DSR_DEGRADE_CASE(6) DSR_DEGRADE_CASE(7) DSR_DEGRADE_CASE(8)
  }
#undef DSR_DEGRADE_CASE
}

// what both entry points ask of the blur kernel and the sampling grid; 0 when fine
int check_sampling(const char* who, int ks, int scale, int offset) {
  if (ks < 1 || ks > KS_MAX || !(ks & 1)) return dsr_fail(DSR_E_ARG, "%s: kernel size %d is not an odd number in 1..%d", who, ks, KS_MAX);
  if (scale < 1 || scale > 8) return dsr_fail(DSR_E_ARG, "%s: scale %d is not in 1..8", who, scale);
  if (offset < 0 || offset >= scale) return dsr_fail(DSR_E_ARG, "%s: offset %d is not in 0..scale-1 = %d", who, offset, scale - 1);
  return 0;
}
}  // namespace

extern "C" int dsr_degrade_batch_u8(int count, const unsigned char* const* images, const int* heights, const int* widths,
                                    const int* tops, const int* lefts, const int* xforms, int ph, int pw, int scale, int offset,
                                    const float* kernels, int ks, const float* noise, const float* noise_std, int quantise, int mode,
                                    float* out, dsr_stream_t st) {
  if (count <= 0 || !images || !heights || !widths || !tops || !lefts || !kernels || !out || ph <= 0 || pw <= 0)
    return dsr_fail(DSR_E_ARG, "degrade_batch_u8: null table or pointer, or bad shape");
  if (int rc = check_sampling("degrade_batch_u8", ks, scale, offset)) return rc;
  if (mode < DSR_PATCH_UNIT || mode > DSR_PATCH_HR_UNIT) return dsr_fail(DSR_E_ARG, "degrade_batch_u8: mode %d", mode);
  if ((noise != nullptr) != (noise_std != nullptr))
    return dsr_fail(DSR_E_ARG, "degrade_batch_u8: noise and noise_std go together (one of them is null)");
  for (int i = 0; i < count; ++i) {
    if (!images[i]) return dsr_fail(DSR_E_ARG, "degrade_batch_u8: null image %d", i);
    if (heights[i] <= 0 || widths[i] <= 0 || ks / 2 >= (heights[i] < widths[i] ? heights[i] : widths[i]))
      return dsr_fail(DSR_E_ARG, "degrade_batch_u8: a %dx%d kernel cannot be reflected in the %dx%d image %d", ks, ks, heights[i], widths[i], i);
    if (tops[i] < 0 || lefts[i] < 0 || (long long)scale * ((long long)tops[i] + ph - 1) + offset >= heights[i] ||
        (long long)scale * ((long long)lefts[i] + pw - 1) + offset >= widths[i])
      return dsr_fail(DSR_E_ARG, "degrade_batch_u8: patch %d (%d,%d)+(%d,%d) at scale %d, offset %d leaves its %dx%d image", i, tops[i],
                      lefts[i], ph, pw, scale, offset, heights[i], widths[i]);
    if (xforms) {
      if (xforms[i] < 0 || xforms[i] > 7) return dsr_fail(DSR_E_ARG, "degrade_batch_u8: transform code %d of patch %d is not in 0..7", xforms[i], i);
      if ((xforms[i] & 1) && ph != pw)
        return dsr_fail(DSR_E_ARG, "degrade_batch_u8: code %d of patch %d turns a %dx%d patch by a quarter", xforms[i], i, ph, pw);
    }
  }
  const size_t per = (size_t)3 * ph * pw;
  for (int i0 = 0; i0 < count; i0 += DSR_PATCH_BATCH_MAX) {
    DegradeBatch t;
    const int n = count - i0 < DSR_PATCH_BATCH_MAX ? count - i0 : DSR_PATCH_BATCH_MAX;
    for (int j = 0; j < n; ++j) {
      t.img[j] = images[i0 + j];
      t.height[j] = heights[i0 + j];
      t.width[j] = widths[i0 + j];
      t.top[j] = tops[i0 + j];
      t.left[j] = lefts[i0 + j];
      t.xform[j] = (unsigned char)(xforms ? xforms[i0 + j] : 0);
    }
    launch(scale, t, n, ph, pw, offset, kernels + (size_t)i0 * ks * ks, ks, noise ? noise + (size_t)i0 * per : nullptr,
           noise_std ? noise_std + i0 : nullptr, quantise, mode, out + (size_t)i0 * per, nullptr, st);
  }
  return dsr_launch_status("dsr_degrade_batch_u8");
}

extern "C" int dsr_degrade_image_u8(const unsigned char* image, int H, int W, int scale, int offset, const float* kernel, int ks,
                                    const float* noise, const float* noise_std, unsigned char* out, dsr_stream_t st) {
  if (!image || !kernel || !out || H <= 0 || W <= 0) return dsr_fail(DSR_E_ARG, "degrade_image_u8: null pointer or bad shape");
  if (int rc = check_sampling("degrade_image_u8", ks, scale, offset)) return rc;
  if ((noise != nullptr) != (noise_std != nullptr))
    return dsr_fail(DSR_E_ARG, "degrade_image_u8: noise and noise_std go together (one of them is null)");
  if (ks / 2 >= (H < W ? H : W)) return dsr_fail(DSR_E_ARG, "degrade_image_u8: a %dx%d kernel cannot be reflected in a %dx%d image", ks, ks, H, W);
  DegradeBatch t;
  t.img[0] = image;
  t.height[0] = H;
  t.width[0] = W;
  t.top[0] = t.left[0] = 0;
  t.xform[0] = 0;
  const int h = (H - offset + scale - 1) / scale, w = (W - offset + scale - 1) / scale;
  launch(scale, t, 1, h, w, offset, kernel, ks, noise, noise_std, 1, DSR_PATCH_UNIT, nullptr, out, st);
  return dsr_launch_status("dsr_degrade_image_u8");
}
