// JPEG compress-and-decompress round trip of device-resident RGB images (uint8 in, uint8 out, no bitstream: entropy coding is
// lossless), a quality per sample, 4:4:4 or 4:2:0 chroma: the last stage of the BSRGAN / Real-ESRGAN degradation, on the
// device.  The baseline codec with libjpeg's default "islow" DCT is integer arithmetic from end to end, so the result is
// defined -- and tested -- bit for bit; the definition is in include/dsr_hip.h, the numpy yardstick in tests/jpeg_ref.py.
//
// One 8x8 block of one component is transformed by EIGHT lanes: in each 1-D pass a lane owns one row (or column) of the block
// and runs jfdctint / jidctint on its eight values in registers, so a wave transforms eight blocks at a time and a 256-thread
// block 32.  Between the row and the column passes the block is turned through the LDS: int32 [8 rows][RS = 9] per block,
// blocks BS = 72 dwords apart.  Lane (g, r) -- block g, row r -- writes row r at g * 72 + r * 9 + k and reads column r at
// g * 72 + k * 9 + r: for a fixed k the 32 lanes of a half wave (ds_write_b32 / ds_read_b32 bank = dword % 32) sit on
// 8 g + 9 r and 8 g + r (mod 32), both 32 different banks (9 is odd: 9 r covers 8 residues that differ mod 8).
//   codec_block: -128, FDCT rows | LDS | FDCT columns, quantise, dequantise, IDCT columns | LDS | IDCT rows, +128, clip
// The quantiser (|c| + d/2) / d is a multiply by a float reciprocal kept beside the table, corrected by one step either way
// (numerator < 2^17, exact in fp32), not an integer division.  The tables are derived from quality[b] in the kernel (128
// threads, once per thread block): no host table, no host read of the qualities.
//
// 4:4:4, jpeg444_kernel, one launch: lane (g, r) loads the 8 pixels of row r of pixel block g, keeps Y, Cb, Cr of them in
// registers, runs codec_block three times and converts and stores the same 8 pixels.
// 4:2:0, two launches, because the triangle filter of the decoder reads decoded chroma of neighbouring MCUs:
//   jpeg420_planes_kernel: thread blocks of 32 luma blocks (one codec_block each), then thread blocks of 32 chroma positions
//       (lane (g, r): 2 x 16 pixels -> 8 downsampled Cb and Cr, two codec_block) -> decoded uint8 planes in the workspace,
//       whole blocks, 8-byte stores;
//   jpeg420_finish_kernel: a thread per 4 output pixels: Y as one dword, 2 x 4 chroma samples per plane, "fancy" upsampling
//       (or replication for a chroma width <= 2), YCbCr -> RGB, store.
// IO: U8Image (interleaved uint8 [count][H][W][3]) reads and writes whole dwords where a run of pixels lies inside the row
// and starts on a 4-byte boundary, single bytes otherwise; F32Batch (fp32 [count][3][h][w], the patch batches) uses 16-byte
// vectors likewise.  Edge replication is a clamp of the pixel coordinate.  No atomics, no scratch, no allocation, no host
// synchronisation: both entry points can be captured into a graph.
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int NT = 256, GROUPS = NT / 8;                       // 8 lanes per 8x8 block
constexpr int RS = 9, BS = 72;                                 // LDS dwords per block row / per block

__device__ const unsigned char BASE_TABLE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// jdct.h, CONST_BITS = 13
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }

struct QuantTables {
  int t[2][64];                                                // luminance, chrominance
  float rcp[2][64];                                            // 1 / (8 t)
};

// the two tables of sample `q` (clamped to 1..100, so that a bad device value cannot divide by zero); needs NT >= 128
__device__ __forceinline__ void make_tables(QuantTables& qt, int q) {
  const int tid = threadIdx.x;
  if (tid < 128) {
    q = min(max(q, 1), 100);
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int t = min(max(((int)BASE_TABLE[tid >> 6][tid & 63] * s + 50) / 100, 1), 255);
    qt.t[tid >> 6][tid & 63] = t;
    qt.rcp[tid >> 6][tid & 63] = 1.0f / (float)(t << 3);
  }
}

// jfdctint.c on eight values; FIRST: pass 1 (rows, out scaled by 4) or pass 2 (columns, the scale removed)
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  constexpr int N = FIRST ? 11 : 15;
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * F_0_541;
  d[2] = descale(z1 + t13 * F_0_765, N);
  d[6] = descale(z1 - t12 * F_1_847, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F_1_175;
  t4 *= F_0_298, t5 *= F_2_053, t6 *= F_3_072, t7 *= F_1_501;
  z1 *= -F_0_899, z2 *= -F_2_562;
  z3 = z3 * -F_1_961 + z5, z4 = z4 * -F_0_390 + z5;
  d[7] = descale(t4 + z1 + z3, N);
  d[5] = descale(t5 + z2 + z4, N);
  d[3] = descale(t6 + z2 + z3, N);
  d[1] = descale(t7 + z1 + z4, N);
}

// jidctint.c on eight values, descaled by N (11: pass 1, columns; 18: pass 2, rows)
template <int N>
__device__ __forceinline__ void idct8(int (&c)[8]) {
  int z1 = (c[2] + c[6]) * F_0_541;
  int t2 = z1 - c[6] * F_1_847, t3 = z1 + c[2] * F_0_765;
  int t0 = (c[0] + c[4]) << 13, t1 = (c[0] - c[4]) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = c[7], t1 = c[5], t2 = c[3], t3 = c[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * F_1_175;
  t0 *= F_0_298, t1 *= F_2_053, t2 *= F_3_072, t3 *= F_1_501;
  z1 *= -F_0_899, z2 *= -F_2_562;
  z3 = z3 * -F_1_961 + z5, z4 = z4 * -F_0_390 + z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  c[0] = descale(t10 + t3, N), c[7] = descale(t10 - t3, N);
  c[1] = descale(t11 + t2, N), c[6] = descale(t11 - t2, N);
  c[2] = descale(t12 + t1, N), c[5] = descale(t12 - t1, N);
  c[3] = descale(t13 + t0, N), c[4] = descale(t13 - t0, N);
}

// v: the samples 0..255 of row r of a block -> its decoded samples.  blk: the block's BS dwords of LDS; table 0 or 1.  EVERY
// thread of the thread block has to come here (two barriers).  A lane writes only its own row before the first barrier and
// reads only its own row after the second, so consecutive calls need no barrier between them.
__device__ __forceinline__ void codec_block(int (&v)[8], int* __restrict__ blk, const QuantTables& qt, int table, int r) {
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] -= 128;
  fdct8<true>(v);
#pragma unroll
  for (int k = 0; k < 8; ++k) blk[r * RS + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = blk[k * RS + r];         // column r
  fdct8<false>(v);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int t = qt.t[table][k * 8 + r], d = t << 3;
    const int c = v[k], num = abs(c) + (d >> 1);               // < 2^17
    int q = (int)((float)num * qt.rcp[table][k * 8 + r]);      // floor(num / d), one off at the most
    const int rem = num - q * d;
    q += rem >= d ? 1 : (rem < 0 ? -1 : 0);
    v[k] = (c < 0 ? -q : q) * t;
  }
  idct8<11>(v);
#pragma unroll
  for (int k = 0; k < 8; ++k) blk[k * RS + r] = v[k];         // back into the column this lane alone has read
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = blk[r * RS + k];
  idct8<18>(v);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = min(max(v[k] + 128, 0), 255);
}

__device__ __forceinline__ int rgb_y(int r, int g, int b) { return (fix16(.299) * r + fix16(.587) * g + fix16(.114) * b + 32768) >> 16; }
__device__ __forceinline__ int rgb_cb(int r, int g, int b) {
  return (-fix16(.16874) * r - fix16(.33126) * g + fix16(.5) * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int rgb_cr(int r, int g, int b) {
  return (fix16(.5) * r - fix16(.41869) * g - fix16(.08131) * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ void ycc_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
  cb -= 128, cr -= 128;
  r = min(max(y + ((fix16(1.402) * cr + 32768) >> 16), 0), 255);
  g = min(max(y + ((-fix16(.34414) * cb + 32768 - fix16(.71414) * cr) >> 16), 0), 255);
  b = min(max(y + ((fix16(1.772) * cb + 32768) >> 16), 0), 255);
}

// the scaling of patch_batch_kernel (data.hip) after its first division, statement for statement
__device__ __forceinline__ float patch_scale(float v, int mode) {
  if (mode == DSR_PATCH_LR_REF) {
    v = v / 255.0f;
  } else if (mode == DSR_PATCH_HR_REF) {
    v = v / 255.0f;
    v = v * 2.0f;
    v = v - 1.0f;
  } else if (mode == DSR_PATCH_HR_UNIT) {
    v = v * 2.0f;
    v = v - 1.0f;
  }
  return v;
}

// uint8 [count][H][W][3].  load / store: N pixels of row y (inside the image) of sample b from column x0 (x0 < W); columns
// past the row's end are read as the last one and not written.
struct U8Image {
  const unsigned char* __restrict__ in;
  unsigned char* __restrict__ out;
  int H, W;
  template <int N>
  __device__ __forceinline__ void load(int b, int y, int x0, int (&R)[N], int (&G)[N], int (&B)[N]) const {
    const unsigned char* __restrict__ row = in + ((size_t)b * H + y) * W * 3;
    const unsigned char* __restrict__ p = row + (size_t)x0 * 3;
    if (x0 + N <= W && ((uintptr_t)p & 3) == 0) {
      unsigned d[N * 3 / 4];
#pragma unroll
      for (int k = 0; k < N * 3 / 4; ++k) d[k] = reinterpret_cast<const unsigned*>(p)[k];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        R[k] = (d[(3 * k) >> 2] >> (8 * ((3 * k) & 3))) & 255;
        G[k] = (d[(3 * k + 1) >> 2] >> (8 * ((3 * k + 1) & 3))) & 255;
        B[k] = (d[(3 * k + 2) >> 2] >> (8 * ((3 * k + 2) & 3))) & 255;
      }
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const unsigned char* __restrict__ q = row + (size_t)min(x0 + k, W - 1) * 3;
        R[k] = q[0], G[k] = q[1], B[k] = q[2];
      }
    }
  }
  template <int N>
  __device__ __forceinline__ void store(int b, int y, int x0, const int (&R)[N], const int (&G)[N], const int (&B)[N]) const {
    unsigned char* __restrict__ p = out + (((size_t)b * H + y) * W + x0) * 3;
    if (x0 + N <= W && ((uintptr_t)p & 3) == 0) {
      unsigned d[N * 3 / 4] = {};
#pragma unroll
      for (int k = 0; k < N; ++k) {
        d[(3 * k) >> 2] |= (unsigned)R[k] << (8 * ((3 * k) & 3));
        d[(3 * k + 1) >> 2] |= (unsigned)G[k] << (8 * ((3 * k + 1) & 3));
        d[(3 * k + 2) >> 2] |= (unsigned)B[k] << (8 * ((3 * k + 2) & 3));
      }
#pragma unroll
      for (int k = 0; k < N * 3 / 4; ++k) reinterpret_cast<unsigned*>(p)[k] = d[k];
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (x0 + k < W) p[3 * k] = (unsigned char)R[k], p[3 * k + 1] = (unsigned char)G[k], p[3 * k + 2] = (unsigned char)B[k];
    }
  }
};

// fp32 [count][3][H][W]: in in DSR_PATCH_UNIT scaling, out scaled by `mode`
struct F32Batch {
  const float* __restrict__ in;
  float* __restrict__ out;
  int H, W, mode;
  static __device__ __forceinline__ int level(float v) { return (int)rintf(fminf(fmaxf(255.0f * v, 0.0f), 255.0f)); }
  template <int N>
  __device__ __forceinline__ void load(int b, int y, int x0, int (&R)[N], int (&G)[N], int (&B)[N]) const {
    const size_t plane = (size_t)H * W;
    const float* __restrict__ row = in + (size_t)b * 3 * plane + (size_t)y * W;
    if (x0 + N <= W && ((uintptr_t)(row + x0) & 15) == 0 && (plane & 3) == 0) {
#pragma unroll
      for (int k = 0; k < N; k += 4) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(row + x0 + k);
        const f32x4 g = *reinterpret_cast<const f32x4*>(row + plane + x0 + k);
        const f32x4 bl = *reinterpret_cast<const f32x4*>(row + 2 * plane + x0 + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) R[k + j] = level(r[j]), G[k + j] = level(g[j]), B[k + j] = level(bl[j]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const float* __restrict__ q = row + min(x0 + k, W - 1);
        R[k] = level(q[0]), G[k] = level(q[plane]), B[k] = level(q[2 * plane]);
      }
    }
  }
  template <int N>
  __device__ __forceinline__ void store(int b, int y, int x0, const int (&R)[N], const int (&G)[N], const int (&B)[N]) const {
    const size_t plane = (size_t)H * W;
    float* __restrict__ row = out + (size_t)b * 3 * plane + (size_t)y * W;
    if (x0 + N <= W && ((uintptr_t)(row + x0) & 15) == 0 && (plane & 3) == 0) {
#pragma unroll
      for (int k = 0; k < N; k += 4) {
        f32x4 r, g, bl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          r[j] = patch_scale((float)R[k + j] / 255.0f, mode);
          g[j] = patch_scale((float)G[k + j] / 255.0f, mode);
          bl[j] = patch_scale((float)B[k + j] / 255.0f, mode);
        }
        *reinterpret_cast<f32x4*>(row + x0 + k) = r;
        *reinterpret_cast<f32x4*>(row + plane + x0 + k) = g;
        *reinterpret_cast<f32x4*>(row + 2 * plane + x0 + k) = bl;
      }
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (x0 + k < W) {
          row[x0 + k] = patch_scale((float)R[k] / 255.0f, mode);
          row[plane + x0 + k] = patch_scale((float)G[k] / 255.0f, mode);
          row[2 * plane + x0 + k] = patch_scale((float)B[k] / 255.0f, mode);
        }
    }
  }
};

// the decoded planes of one 4:2:0 image in the workspace: whole blocks, so every size is a multiple of 8
struct Planes420 {
  int hy, wy, ch, cw, hc, wc;                                  // luma plane; real chroma samples; chroma plane
  size_t per_image;
  __host__ __device__ Planes420(int H, int W) {
    hy = (H + 7) / 8 * 8, wy = (W + 7) / 8 * 8;
    ch = (H + 1) / 2, cw = (W + 1) / 2;
    hc = (ch + 7) / 8 * 8, wc = (cw + 7) / 8 * 8;
    per_image = (size_t)hy * wy + 2 * (size_t)hc * wc;
  }
};

template <class IO>
__global__ __launch_bounds__(NT) void jpeg444_kernel(const IO io, const int* __restrict__ quality) {
  __shared__ QuantTables qt;
  __shared__ int tile[GROUPS * BS];
  const int b = blockIdx.y, g = threadIdx.x >> 3, r = threadIdx.x & 7;
  const int H = io.H, W = io.W, bw = (W + 7) >> 3, nblk = ((H + 7) >> 3) * bw;
  make_tables(qt, quality[b]);
  __syncthreads();
  const int want = blockIdx.x * GROUPS + g;
  const int blk = min(want, nblk - 1);                         // a group past the end repeats the last block and stores nothing
  const int y = (blk / bw) * 8 + r, x0 = (blk % bw) * 8;
  int R[8], G[8], B[8], Y[8], Cb[8], Cr[8];
  io.template load<8>(b, min(y, H - 1), x0, R, G, B);
#pragma unroll
  for (int k = 0; k < 8; ++k) Y[k] = rgb_y(R[k], G[k], B[k]), Cb[k] = rgb_cb(R[k], G[k], B[k]), Cr[k] = rgb_cr(R[k], G[k], B[k]);
  int* __restrict__ mine = tile + g * BS;
  codec_block(Y, mine, qt, 0, r);
  codec_block(Cb, mine, qt, 1, r);
  codec_block(Cr, mine, qt, 1, r);
  if (want >= nblk || y >= H) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) ycc_rgb(Y[k], Cb[k], Cr[k], R[k], G[k], B[k]);
  io.template store<8>(b, y, x0, R, G, B);
}

// grid.x: luma_groups thread blocks of 32 luma blocks, then thread blocks of 32 chroma positions (Cb and Cr of each)
template <class IO>
__global__ __launch_bounds__(NT) void jpeg420_planes_kernel(const IO io, const int* __restrict__ quality, int luma_groups,
                                                            unsigned char* __restrict__ ws) {
  __shared__ QuantTables qt;
  __shared__ int tile[GROUPS * BS];
  const int b = blockIdx.y, g = threadIdx.x >> 3, r = threadIdx.x & 7;
  const int H = io.H, W = io.W;
  const Planes420 pl(H, W);
  make_tables(qt, quality[b]);
  __syncthreads();
  int* __restrict__ mine = tile + g * BS;
  unsigned char* __restrict__ yp = ws + (size_t)b * pl.per_image;
  if ((int)blockIdx.x < luma_groups) {                         // uniform over the thread block
    const int bw = pl.wy >> 3, nblk = (pl.hy >> 3) * bw;
    const int want = blockIdx.x * GROUPS + g, blk = min(want, nblk - 1);
    const int y = (blk / bw) * 8 + r, x0 = (blk % bw) * 8;
    int R[8], G[8], B[8], Y[8];
    io.template load<8>(b, min(y, H - 1), x0, R, G, B);
#pragma unroll
    for (int k = 0; k < 8; ++k) Y[k] = rgb_y(R[k], G[k], B[k]);
    codec_block(Y, mine, qt, 0, r);
    if (want >= nblk) return;
    uint2 o;
    o.x = Y[0] | (Y[1] << 8) | (Y[2] << 16) | (Y[3] << 24);
    o.y = Y[4] | (Y[5] << 8) | (Y[6] << 16) | (Y[7] << 24);
    *reinterpret_cast<uint2*>(yp + (size_t)y * pl.wy + x0) = o;
    return;
  }
  const int bw = pl.wc >> 3, nblk = (pl.hc >> 3) * bw;
  const int want = ((int)blockIdx.x - luma_groups) * GROUPS + g, blk = min(want, nblk - 1);
  const int cy = (blk / bw) * 8 + r, cx0 = (blk % bw) * 8;
  // a chroma row at or below ch repeats the last downsampled row; a pixel row or column past the image repeats the last one
  const int sy = 2 * min(cy, pl.ch - 1), sx = min(2 * cx0, W - 1);
  int R[16], G[16], B[16], Cb[8], Cr[8];
  io.template load<16>(b, sy, sx, R, G, B);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // columns 2 (cx0 + k), + 1 clamped to W - 1: load() clamps from sx on, which is 2 cx0 or (past the image) W - 1 itself
    Cb[k] = rgb_cb(R[2 * k], G[2 * k], B[2 * k]) + rgb_cb(R[2 * k + 1], G[2 * k + 1], B[2 * k + 1]);
    Cr[k] = rgb_cr(R[2 * k], G[2 * k], B[2 * k]) + rgb_cr(R[2 * k + 1], G[2 * k + 1], B[2 * k + 1]);
  }
  io.template load<16>(b, min(sy + 1, H - 1), sx, R, G, B);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int bias = 1 + (k & 1);                              // cx0 is even: 1 in even output columns, 2 in odd ones
    Cb[k] = (Cb[k] + rgb_cb(R[2 * k], G[2 * k], B[2 * k]) + rgb_cb(R[2 * k + 1], G[2 * k + 1], B[2 * k + 1]) + bias) >> 2;
    Cr[k] = (Cr[k] + rgb_cr(R[2 * k], G[2 * k], B[2 * k]) + rgb_cr(R[2 * k + 1], G[2 * k + 1], B[2 * k + 1]) + bias) >> 2;
  }
  codec_block(Cb, mine, qt, 1, r);
  codec_block(Cr, mine, qt, 1, r);
  if (want >= nblk) return;
  unsigned char* __restrict__ cbp = yp + (size_t)pl.hy * pl.wy;
  unsigned char* __restrict__ crp = cbp + (size_t)pl.hc * pl.wc;
  uint2 o;
  o.x = Cb[0] | (Cb[1] << 8) | (Cb[2] << 16) | (Cb[3] << 24);
  o.y = Cb[4] | (Cb[5] << 8) | (Cb[6] << 16) | (Cb[7] << 24);
  *reinterpret_cast<uint2*>(cbp + (size_t)cy * pl.wc + cx0) = o;
  o.x = Cr[0] | (Cr[1] << 8) | (Cr[2] << 16) | (Cr[3] << 24);
  o.y = Cr[4] | (Cr[5] << 8) | (Cr[6] << 16) | (Cr[7] << 24);
  *reinterpret_cast<uint2*>(crp + (size_t)cy * pl.wc + cx0) = o;
}

// four chroma values of output row y at columns x .. x + 3 (x % 4 == 0) from the decoded plane c (pitch wc, ch x cw real samples)
__device__ __forceinline__ void upsample4(const unsigned char* __restrict__ c, int wc, int ch, int cw, int y, int x, int (&out)[4]) {
  const int cy = y >> 1, i0 = x >> 1;
  if (cw <= 2) {                                               // plain replication
    const unsigned char* __restrict__ row = c + (size_t)cy * wc;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = row[min(i0 + (k >> 1), cw - 1)];
    return;
  }
  const int ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);   // the nearer neighbour row, replicated at the edges
  const unsigned char* __restrict__ row = c + (size_t)cy * wc;
  const unsigned char* __restrict__ nrow = c + (size_t)ny * wc;
  int cs[4];                                                   // columns i0 - 1 .. i0 + 2, replicated at the edges
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = min(max(i0 - 1 + k, 0), cw - 1);
    cs[k] = 3 * (int)row[i] + (int)nrow[i];
  }
  // the first and the last column of the row are (4 cs + 8) >> 4 and (4 cs + 7) >> 4: the general taps with a replicated neighbour
  out[0] = (3 * cs[1] + cs[0] + 8) >> 4;
  out[1] = (3 * cs[1] + cs[2] + 7) >> 4;
  out[2] = (3 * cs[2] + cs[1] + 8) >> 4;
  out[3] = (3 * cs[2] + cs[3] + 7) >> 4;
}

template <class IO>
__global__ __launch_bounds__(NT) void jpeg420_finish_kernel(const IO io, const unsigned char* __restrict__ ws) {
  const int H = io.H, W = io.W, b = blockIdx.y;
  const Planes420 pl(H, W);
  const int quads = (W + 3) >> 2;
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (size_t)quads * H) return;
  const int y = (int)(idx / quads), x = (int)(idx - (size_t)y * quads) * 4;
  const unsigned char* __restrict__ yp = ws + (size_t)b * pl.per_image;
  const unsigned char* __restrict__ cbp = yp + (size_t)pl.hy * pl.wy;
  const unsigned char* __restrict__ crp = cbp + (size_t)pl.hc * pl.wc;
  const unsigned yy = *reinterpret_cast<const unsigned*>(yp + (size_t)y * pl.wy + x);     // wy % 8 == 0, x % 4 == 0
  int cb[4], cr[4], R[4], G[4], B[4];
  upsample4(cbp, pl.wc, pl.ch, pl.cw, y, x, cb);
  upsample4(crp, pl.wc, pl.ch, pl.cw, y, x, cr);
#pragma unroll
  for (int k = 0; k < 4; ++k) ycc_rgb((yy >> (8 * k)) & 255, cb[k], cr[k], R[k], G[k], B[k]);
  io.template store<4>(b, y, x, R, G, B);
}

constexpr int DIM_MAX = 65536, COUNT_MAX = 65535;

int check_common(const char* who, const void* in, const void* out, int count, int H, int W, const int* quality, int subsampling,
                 const void* workspace) {
  if (!in || !out || !quality) return dsr_fail(DSR_E_ARG, "%s: null pointer", who);
  if (in == out) return dsr_fail(DSR_E_ARG, "%s: out must not be in", who);
  if (count < 1 || count > COUNT_MAX) return dsr_fail(DSR_E_ARG, "%s: count %d is not in 1..%d", who, count, COUNT_MAX);
  if (H < 1 || W < 1 || H > DIM_MAX || W > DIM_MAX) return dsr_fail(DSR_E_ARG, "%s: size %dx%d is not in 1..%d", who, H, W, DIM_MAX);
  if (subsampling != 0 && subsampling != 2)
    return dsr_fail(DSR_E_ARG, "%s: subsampling %d is neither 0 (4:4:4) nor 2 (4:2:0)", who, subsampling);
  if (subsampling == 2 && (!workspace || ((uintptr_t)workspace & 15)))
    return dsr_fail(DSR_E_ARG, "%s: 4:2:0 needs a 16-byte aligned workspace of dsr_jpeg_workspace() bytes", who);
  return 0;
}

template <class IO>
void launch(const IO& io, int count, const int* quality, int subsampling, void* workspace, dsr_stream_t st) {
  const int H = io.H, W = io.W;
  if (subsampling == 0) {
    const int nblk = ((H + 7) / 8) * ((W + 7) / 8);
    hipLaunchKernelGGL(jpeg444_kernel<IO>, dim3((nblk + GROUPS - 1) / GROUPS, count), dim3(NT), 0, st, io, quality);
    return;
  }
  const Planes420 pl(H, W);
  const int luma = ((pl.hy / 8) * (pl.wy / 8) + GROUPS - 1) / GROUPS, chroma = ((pl.hc / 8) * (pl.wc / 8) + GROUPS - 1) / GROUPS;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  hipLaunchKernelGGL(jpeg420_planes_kernel<IO>, dim3(luma + chroma, count), dim3(NT), 0, st, io, quality, luma, ws);
  const size_t quads = (size_t)((W + 3) / 4) * H;
  hipLaunchKernelGGL(jpeg420_finish_kernel<IO>, dim3((unsigned)((quads + NT - 1) / NT), count), dim3(NT), 0, st, io, ws);
}
}  // namespace

extern "C" size_t dsr_jpeg_workspace(int count, int H, int W, int subsampling) {
  if (count < 1 || count > COUNT_MAX || H < 1 || W < 1 || H > DIM_MAX || W > DIM_MAX || subsampling != 2) return 0;
  return (size_t)count * Planes420(H, W).per_image;
}

extern "C" int dsr_jpeg_u8(const unsigned char* in, unsigned char* out, int count, int H, int W, const int* quality, int subsampling,
                           void* workspace, dsr_stream_t st) {
  if (int rc = check_common("jpeg_u8", in, out, count, H, W, quality, subsampling, workspace)) return rc;
  launch(U8Image{in, out, H, W}, count, quality, subsampling, workspace, st);
  return dsr_launch_status("dsr_jpeg_u8");
}

extern "C" int dsr_jpeg_batch_f32(const float* in, float* out, int count, int h, int w, const int* quality, int subsampling, int mode,
                                  void* workspace, dsr_stream_t st) {
  if (int rc = check_common("jpeg_batch_f32", in, out, count, h, w, quality, subsampling, workspace)) return rc;
  if (mode < DSR_PATCH_UNIT || mode > DSR_PATCH_HR_UNIT) return dsr_fail(DSR_E_ARG, "jpeg_batch_f32: mode %d", mode);
  launch(F32Batch{in, out, h, w, mode}, count, quality, subsampling, workspace, st);
  return dsr_launch_status("dsr_jpeg_batch_f32");
}
