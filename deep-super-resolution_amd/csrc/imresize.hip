// MATLAB-style separable resampler (utils/imresize.py): y = W_h . x . W_w^T per plane, the two passes in ONE launch.
//   tables (host-built in float64, rounded to fp32 once, device resident), per axis:  idx [out][taps] 0-based source
//   index, already mirrored;  w [out][taps] fp32;  a padding entry carries weight 0 and a valid index.
//   forward : dsr_imresize_f32(x, y, ..., forward tables)      backward: the same entry point on dy with the TRANSPOSED
//   tables (for source i the (o, w) pairs that read it, padded to the longest list): dx = W_h^T . dy . W_w is a gather too.
// Tile scheme: a block owns IMR_TH x IMR_TW outputs of one plane.  It reduces its slice of idx_w to the column range
// [c0, c0 + sw) its W taps reference, runs the H pass straight from global memory into an LDS strip [IMR_TH][sw] (lanes
// along x: every source row is read contiguously; the row index and weight of a tap are wave-uniform), then the W pass out
// of the LDS.  The intermediate never reaches HBM and stays fp32.  Per output and pass: one fmaf per tap, in tap order, from
// 0 -- no atomics, no reassociation: the result is defined bit for bit.  A tile whose strip is wider than the LDS the launch
// was given computes the same chains straight from global memory (H chain per W tap): slower, same bits, never truncated.
// Every table index is clamped to its axis before use, so no table content can make the kernel read out of bounds.
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

#define IMR_TH 16
#define IMR_TW 32
#define IMR_THREADS 256
#define IMR_MAX_TAPS 64
#define IMR_LDS_BYTES 65536   // static + dynamic LDS of a block without an opt-in; a x1/4 bicubic strip takes 9 KB of it

struct ImrArgs {
  const void* x;
  void* y;
  int H, W, OH, OW;
  int x_ps, x_rs, x_cs;   // element strides of a plane, a row and a pixel of x
  int y_ps, y_rs, y_cs;
  const int* idx_h;
  const float* w_h;
  int taps_h;
  const int* idx_w;
  const float* w_w;
  int taps_w;
  int tiles_x, tiles_y;
  int cap;                // columns per strip row the launch's LDS holds
};

__device__ __forceinline__ float imr_load(const float* p) { return *p; }
__device__ __forceinline__ float imr_load(const unsigned char* p) { return (float)*p; }
__device__ __forceinline__ void imr_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void imr_store(unsigned char* p, float v) {
  *p = (unsigned char)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
}
__device__ __forceinline__ int imr_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

template <typename T>
__global__ __launch_bounds__(IMR_THREADS) void imresize_kernel(const ImrArgs a) {
  extern __shared__ float strip[];   // [IMR_TH][a.cap]
  __shared__ int s_lo, s_hi;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y, plane = b / a.tiles_y;
  const int ox0 = tx * IMR_TW, oy0 = ty * IMR_TH;
  const int tw = min(IMR_TW, a.OW - ox0), th = min(IMR_TH, a.OH - oy0);
  const int taps_h = a.taps_h, taps_w = a.taps_w;

  // column range of the tile's W taps
  if (tid == 0) {
    s_lo = a.W - 1;
    s_hi = 0;
  }
  __syncthreads();
  {
    int lo = a.W - 1, hi = 0;
    const int* iw = a.idx_w + (size_t)ox0 * taps_w;
    for (int i = tid; i < tw * taps_w; i += IMR_THREADS) {
      const int c = imr_clamp(iw[i], a.W);
      lo = min(lo, c);
      hi = max(hi, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((tid & 63) == 0) {
      atomicMin(&s_lo, lo);
      atomicMax(&s_hi, hi);
    }
  }
  __syncthreads();
  const int c0 = s_lo, sw = s_hi - s_lo + 1;   // tw * taps_w >= 1 entries were seen: 1 <= sw <= W

  const T* xp = (const T*)a.x + (size_t)plane * a.x_ps;
  T* yp = (T*)a.y + (size_t)plane * a.y_ps;
  const int ox = tid & (IMR_TW - 1), r0 = tid / IMR_TW;   // this thread's outputs: column ox, rows r0 and r0 + 8
  const int* iwo = a.idx_w + (size_t)(ox0 + min(ox, tw - 1)) * taps_w;
  const float* wwo = a.w_w + (size_t)(ox0 + min(ox, tw - 1)) * taps_w;

  if (sw <= a.cap) {
    // H pass: wave v owns strip rows v, v + 4, ...; a lane runs four columns 64 apart through the tap loop together
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int r = wave; r < th; r += IMR_THREADS / 64) {
      const int* ih = a.idx_h + (size_t)(oy0 + r) * taps_h;
      const float* wh = a.w_h + (size_t)(oy0 + r) * taps_h;
      float* srow = strip + (size_t)r * a.cap;
      for (int cb = 0; cb < sw; cb += 256) {
        const T* col[4];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) col[k] = xp + (size_t)(c0 + min(cb + lane + 64 * k, sw - 1)) * a.x_cs;
        for (int t = 0; t < taps_h; ++t) {
          const size_t roff = (size_t)imr_clamp(ih[t], a.H) * a.x_rs;
          const float w = wh[t];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = fmaf(w, imr_load(col[k] + roff), acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (cb + lane + 64 * k < sw) srow[cb + lane + 64 * k] = acc[k];
      }
    }
    __syncthreads();
    // W pass out of the strip
    if (ox < tw) {
      const float* s0 = strip + (size_t)r0 * a.cap;
      const float* s1 = strip + (size_t)(r0 + IMR_TH / 2) * a.cap;
      float acc0 = 0.f, acc1 = 0.f;
      for (int t = 0; t < taps_w; ++t) {
        const int c = imr_clamp(iwo[t], a.W) - c0;
        const float w = wwo[t];
        acc0 = fmaf(w, s0[c], acc0);
        acc1 = fmaf(w, s1[c], acc1);
      }
      T* out = yp + (size_t)(ox0 + ox) * a.y_cs;
      if (r0 < th) imr_store(out + (size_t)(oy0 + r0) * a.y_rs, acc0);
      if (r0 + IMR_TH / 2 < th) imr_store(out + (size_t)(oy0 + r0 + IMR_TH / 2) * a.y_rs, acc1);
    }
  } else if (ox < tw) {
    // the strip does not fit: the same two chains per output, the H chain recomputed from global memory for every W tap
    for (int r = r0; r < th; r += IMR_TH / 2) {
      const int* ih = a.idx_h + (size_t)(oy0 + r) * taps_h;
      const float* wh = a.w_h + (size_t)(oy0 + r) * taps_h;
      float acc = 0.f;
      for (int t = 0; t < taps_w; ++t) {
        const T* col = xp + (size_t)imr_clamp(iwo[t], a.W) * a.x_cs;
        float hacc = 0.f;
        for (int u = 0; u < taps_h; ++u) hacc = fmaf(wh[u], imr_load(col + (size_t)imr_clamp(ih[u], a.H) * a.x_rs), hacc);
        acc = fmaf(wwo[t], hacc, acc);
      }
      imr_store(yp + (size_t)(oy0 + r) * a.y_rs + (size_t)(ox0 + ox) * a.y_cs, acc);
    }
  }
}

// ================================================================== C ABI
template <typename T>
static int imr_launch(const char* what, const void* x, void* y, int planes, int H, int W, int OH, int OW, int pix_stride,
                      const int* idx_h, const float* w_h, int taps_h, const int* idx_w, const float* w_w, int taps_w,
                      dsr_stream_t st) {
  if (!(x && y && idx_h && w_h && idx_w && w_w)) return dsr_fail(DSR_E_ARG, "%s: null pointer", what);
  if (planes < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return dsr_fail(DSR_E_ARG, "%s: a size is < 1", what);
  if (taps_h < 1 || taps_h > IMR_MAX_TAPS || taps_w < 1 || taps_w > IMR_MAX_TAPS)
    return dsr_fail(DSR_E_UNSUPPORTED, "%s: %d x %d taps, 1..%d per axis are supported", what, taps_h, taps_w, IMR_MAX_TAPS);
  const long long in_px = (long long)H * W, out_px = (long long)OH * OW;
  if ((long long)planes * (in_px > out_px ? in_px : out_px) >= (1ll << 31))
    return dsr_fail(DSR_E_ARG, "%s: planes * max(H*W, OH*OW) does not fit 31 bits", what);
  ImrArgs a;
  a.x = x;
  a.y = y;
  a.H = H, a.W = W, a.OH = OH, a.OW = OW;
  if (pix_stride == 1) {   // planar fp32 [planes][H][W]
    a.x_ps = H * W, a.x_rs = W, a.x_cs = 1;
    a.y_ps = OH * OW, a.y_rs = OW, a.y_cs = 1;
  } else {                 // interleaved [H][W][planes]
    a.x_ps = 1, a.x_rs = W * planes, a.x_cs = planes;
    a.y_ps = 1, a.y_rs = OW * planes, a.y_cs = planes;
  }
  a.idx_h = idx_h, a.w_h = w_h, a.taps_h = taps_h;
  a.idx_w = idx_w, a.w_w = w_w, a.taps_w = taps_w;
  a.tiles_x = (OW + IMR_TW - 1) / IMR_TW;
  a.tiles_y = (OH + IMR_TH - 1) / IMR_TH;
  // what a tile of a resampling table references: IMR_TW outputs W / OW apart plus one support; the tables live on the
  // device, so this is an estimate -- the kernel measures each tile and takes its direct path where the strip is wider
  long long est = ((long long)IMR_TW * W + (OW > 1 ? OW - 2 : 0)) / (OW > 1 ? OW - 1 : 1) + taps_w + 4;
  if (est > W) est = W;
  const int cap_max = (IMR_LDS_BYTES - 64) / (IMR_TH * (int)sizeof(float));   // 64 B: the kernel's static LDS
  a.cap = est > cap_max ? cap_max : (int)est;
  const size_t lds = (size_t)IMR_TH * a.cap * sizeof(float);
  const long long blocks = (long long)a.tiles_x * a.tiles_y * planes;   // <= planes * OH * OW < 2^31
  hipLaunchKernelGGL((imresize_kernel<T>), dim3((unsigned)blocks), dim3(IMR_THREADS), lds, st, a);
  return dsr_launch_status(what);
}

extern "C" int dsr_imresize_f32(const float* x, float* y, int planes, int H, int W, int OH, int OW, const int* idx_h,
                                const float* w_h, int taps_h, const int* idx_w, const float* w_w, int taps_w,
                                dsr_stream_t st) {
  return imr_launch<float>("dsr_imresize_f32", x, y, planes, H, W, OH, OW, 1, idx_h, w_h, taps_h, idx_w, w_w, taps_w, st);
}

extern "C" int dsr_imresize_u8(const unsigned char* x, unsigned char* y, int H, int W, int C, int OH, int OW,
                               const int* idx_h, const float* w_h, int taps_h, const int* idx_w, const float* w_w,
                               int taps_w, dsr_stream_t st) {
  if (C < 1) return dsr_fail(DSR_E_ARG, "dsr_imresize_u8: C %d < 1", C);
  return imr_launch<unsigned char>("dsr_imresize_u8", x, y, C, H, W, OH, OW, C, idx_h, w_h, taps_h, idx_w, w_w, taps_w, st);
}
