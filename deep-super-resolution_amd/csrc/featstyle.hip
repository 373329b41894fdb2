// Style (Gram-matrix) term of the feature loss (perceptual.VggFeatureLoss(style_weight=), functional.FeatureStyleTap) for gfx950.
//
// For a tapped 16-bit NHWC map f[n][p][c] (p over the HW pixels of image n, Cp = round_up(C, 8) channels, pad channels zero)
//   gram_fwd : gram[n][i][j] = scale * sum_p f[n][p][i] f[n][p][j], fp32.  Pixels are the contraction index and both MFMA
//              operands come from the same staged tile through the transposing ds_read_b64_tr_b16 (the operand path of
//              conv_wgrad_tile.hip).  A block owns one 64 x 64 channel-tile pair ON OR ABOVE the diagonal and one chunk of
//              GRAM_CHUNK pixels of one image and writes its accumulators to that chunk's fp32 slab; a fold kernel then sums the
//              slabs in chunk order and writes gram[i][j] and gram[j][i] from the same sum, so gram[n] is bit-symmetric.  The
//              chunk size is a constant: the summation order depends on the shape only, never on the grid or the CU count.
//   gram_loss: up to 32 blocks per image over its C x C entries (a split that depends on C alone), double accumulation in a
//              fixed order: the sums of |G - Gt| (L1) or (G - Gt)^2 (MSE) and the largest magnitude per image; then the
//              16-bit operand of the backward GEMM, s16[n][Cp][Cp]: sign(G - Gt) for L1,
//              (G - Gt) / max|G - Gt| for MSE with that divisor in s_scale[n] (1 for L1, 1 for an all-zero difference).  Its
//              entries are of order one whatever the normalisation, so fp16 can neither overflow nor underflow; every scalar
//              factor stays in fp32 and enters in the backward's epilogue.  A one-block launch folds the sums into the mean.
//              A NaN or an Inf in G - Gt (an overflow upstream) is not hidden from a loss scaler that reads gradients: it makes
//              the value non-finite, it leaves a non-finite entry in s16 in BOTH modes (L1 stores it as it is, never as the
//              sign of an Inf), and for MSE it is the image's s_scale, so tap_bwd writes non-finite values into df of that
//              image and of no other.
//   tap_bwd  : df = (dnext ? dnext * m : 0) + g_content * coef_content * d + g_style * coef_style * s_scale[n] * (f[n] . s16[n])
//              a per-image [HW x Cp] . [Cp x Cp] GEMM (f read row-wise, s16 through the transposing read) with the pointwise
//              terms of featloss_tap_bwd in its epilogue: one launch, one rounding per element, and no 16-bit image of the
//              style gradient ever exists in memory.
// No atomics anywhere: every value is written by one thread with a plain store, two calls give the same bits.
#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define GRAM_CHUNK 1024   // pixels per partial slab (dsr_gram_chunks); a multiple of GRAM_KP
#define GRAM_KP 128       // pixels staged per step: 4 MFMA k-steps of 32
#define STYLE_MAX_CP 512

// LDS image of a tile: row r (a pixel, or a row of s16) is 128 bytes = 64 channels; its 16-byte chunk c sits at c ^ (r & 7)
__device__ __forceinline__ unsigned char* style_slot(unsigned char* base, int r, int c) { return base + r * 128 + ((c ^ (r & 7)) << 4); }

__device__ __forceinline__ s16x4 style_tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}
// rows r1 .. r1 + 3 and r2 .. r2 + 3 (each lane names its own row of the block) of columns 8 * chunk + within / 2 ..: the lane
// ends up with its column's 8 values, rows r1.. first
__device__ __forceinline__ U4 style_tr_frag(const unsigned char* base, int r1, int r2, int chunk, int within) {
  s16x4 lo = style_tr_read(base + r1 * 128 + ((chunk ^ (r1 & 7)) << 4) + within);
  s16x4 hi = style_tr_read(base + r2 * 128 + ((chunk ^ (r2 & 7)) << 4) + within);
  return __builtin_bit_cast(U4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// grid: x = n * chunks + chunk, y = tile pair (ti <= tj, row-major over the upper triangle).  4 waves = 2 x 2, 2 x 2 MFMA tiles each.
template <int DT>
__global__ __launch_bounds__(256) void gram_fwd_kernel(const unsigned short* __restrict__ f, int HW, int Cp, int tiles, int chunks,
                                                       float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char sA[GRAM_KP * 128];
  __shared__ __attribute__((aligned(16))) unsigned char sB[GRAM_KP * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int g = lane >> 4, l16 = lane & 15, q4 = l16 >> 2, cc = 4 * (l16 & 3);
  const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
  int ti = 0, rem = blockIdx.y;
  while (rem >= tiles - ti) {       // block-uniform
    rem -= tiles - ti;
    ++ti;
  }
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const int ca0 = ti * 64, cb0 = tj * 64;
  const unsigned char* sBr = diag ? sA : sB;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int c = tid & 7, pbase = tid >> 3;
  const bool a_ok = ca0 + c * 8 < Cp, b_ok = cb0 + c * 8 < Cp;
  const int px0 = chunk * GRAM_CHUNK;
  const int px1 = px0 + GRAM_CHUNK < HW ? px0 + GRAM_CHUNK : HW;
  const size_t img = (size_t)n * (size_t)HW;

  for (int k0 = px0; k0 < px1; k0 += GRAM_KP) {      // block-uniform trip count: EXEC stays full for the transposing reads
    __syncthreads();                                  // the previous step's fragment reads are done
#pragma unroll
    for (int u = 0; u < GRAM_KP / 32; ++u) {
      const int p = pbase + 32 * u;
      const bool in = k0 + p < px1;                   // a ragged last step is zero-filled, never read out of bounds
      const size_t row = (img + (size_t)(k0 + p)) * (size_t)Cp;
      *reinterpret_cast<U4*>(style_slot(sA, p, c)) = load16_or_zero(f, row + ca0 + c * 8, in && a_ok);
      if (!diag) *reinterpret_cast<U4*>(style_slot(sB, p, c)) = load16_or_zero(f, row + cb0 + c * 8, in && b_ok);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GRAM_KP / 32; ++kk) {
      const int r1 = kk * 32 + 4 * g + q4, r2 = r1 + 16;
      U4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ch = wr * 32 + i * 16 + cc;
        fa[i] = style_tr_frag(sA, r1, r2, ch >> 3, (ch & 7) * 2);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ch = wc * 32 + j * 16 + cc;
        fb[j] = style_tr_frag(sBr, r1, r2, ch >> 3, (ch & 7) * 2);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16<DT>(fa[i], fb[j], acc[i][j]);
    }
  }

  float* slab = ws + (size_t)blockIdx.x * (size_t)Cp * (size_t)Cp;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ca0 + wr * 32 + i * 16 + 4 * g + r, col = cb0 + wc * 32 + j * 16 + l16;
        if (row < Cp && col < Cp) slab[(size_t)row * Cp + col] = acc[i][j][r];
      }
}

// gram[n][i][j] and gram[n][j][i] are the same sum of the same slab entries (the one above the diagonal), in chunk order
__global__ __launch_bounds__(256) void gram_fold_kernel(const float* __restrict__ ws, int C, int Cp, int chunks, float scale,
                                                        size_t total, float* __restrict__ gram) {
  const size_t cc = (size_t)C * (size_t)C, slab = (size_t)Cp * (size_t)Cp;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t n = e / cc, ij = e - n * cc;
    const int i = (int)(ij / (size_t)C), j = (int)(ij - (size_t)i * (size_t)C);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const float* src = ws + n * (size_t)chunks * slab + (size_t)lo * Cp + hi;
    float s = 0.f;
    for (int k = 0; k < chunks; ++k) s += src[(size_t)k * slab];
    gram[e] = scale * s;
  }
}

// The C x C entries of one image are split over `slices` blocks (a function of C alone, style_loss_slices): slice b's sum and
// largest magnitude go to partial[(n * slices + b) * 2 + {0, 1}].
__global__ __launch_bounds__(256) void gram_loss_reduce_kernel(const float* __restrict__ gf, const float* __restrict__ gt, int C,
                                                               int mode, int slices, double* __restrict__ partial) {
  __shared__ double ssum[256];
  __shared__ float smax[256];
  const int n = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const int cc = C * C;
  const int per = (cc + slices - 1) / slices;
  const int e0 = b * per, e1 = e0 + per < cc ? e0 + per : cc;
  const float* x = gf + (size_t)n * cc;
  const float* y = gt + (size_t)n * cc;
  double s = 0.0;
  float mx = 0.f;
  for (int e = e0 + tid; e < e1; e += 256) {
    const double d = (double)x[e] - (double)y[e];
    s += mode == DSR_FEAT_L1 ? fabs(d) : d * d;
    const float m = fabsf((float)d);
    mx = (m > mx || m != m) ? m : mx;                 // a NaN sticks: an overflow upstream is not hidden from a loss scaler
  }
  ssum[tid] = s;
  smax[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      ssum[tid] += ssum[tid + o];
      const float m = smax[tid + o], cur = smax[tid];
      smax[tid] = (m > cur || m != m) ? m : cur;
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* out = partial + ((size_t)n * slices + b) * 2;
    out[0] = ssum[0];
    out[1] = (double)smax[0];
  }
}

// grid (blocks over the Cp x Cp entries, N): every block folds its image's slice maxima in slice order (the same value in all)
template <int DT>
__global__ __launch_bounds__(256) void gram_loss_operand_kernel(const float* __restrict__ gf, const float* __restrict__ gt, int C, int Cp,
                                                                int mode, int slices, const double* __restrict__ partial,
                                                                unsigned short* __restrict__ s16, float* __restrict__ s_scale) {
  const int n = blockIdx.y;
  float mx = 0.f;
  for (int b = 0; b < slices; ++b) {
    const float m = (float)partial[((size_t)n * slices + b) * 2 + 1];
    mx = (m > mx || m != m) ? m : mx;
  }
  const bool zero = mx == 0.f;
  const float div = (mode == DSR_FEAT_L1 || zero) ? 1.f : mx;
  if (blockIdx.x == 0 && threadIdx.x == 0) s_scale[n] = div;
  const float* x = gf + (size_t)n * C * C;
  const float* y = gt + (size_t)n * C * C;
  unsigned short* out = s16 + (size_t)n * Cp * Cp;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < Cp * Cp; e += gridDim.x * 256) {
    const int i = e / Cp, j = e - i * Cp;
    float v = 0.f;
    if (i < C && j < C) {
      const float d = (float)((double)x[i * C + j] - (double)y[i * C + j]);
      // L1: the sign, but a non-finite d as it is -- sign(Inf) = 1 would hand a finite gradient on after an overflow upstream
      v = mode == DSR_FEAT_L1 ? ((d > 0.f && d <= __FLT_MAX__) ? 1.f : ((d < 0.f && d >= -__FLT_MAX__) ? -1.f : d)) : (zero ? 0.f : d / div);
    }
    out[e] = f2h<DT>(v);
  }
}

// one block: the N * slices sums in a fixed order (strided per thread, then a tree), in double
__global__ __launch_bounds__(256) void gram_loss_fold_kernel(const double* __restrict__ partial, int terms, double count,
                                                             float* __restrict__ value) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < terms; i += 256) s += partial[(size_t)i * 2];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) value[0] = (float)(sh[0] / count);
}

struct StyleBwdArgs {
  const unsigned short *f, *t, *dnext, *s16;
  const float *g_content, *g_style, *s_scale;
  unsigned short* df;
  float coef_content, coef_style;
  int mode, masked, HW, Cp, tilesP;
};

// grid: x = n * tilesP + pixel tile (64 pixels of ONE image), y = 64-channel tile of the output.  4 waves = 2 (pixel halves) x 2
// (channel halves), 2 x 2 MFMA tiles each; K = the Cp input channels in steps of 64.
template <int DT>
__global__ __launch_bounds__(256) void featstyle_tap_bwd_kernel(const StyleBwdArgs a) {
  constexpr int OLD = 68;                              // fp32 row stride of the output tile (64 + 4: no 4-way write conflict)
  __shared__ __attribute__((aligned(16))) unsigned char smem[64 * OLD * 4];   // 17408 B >= the two 8 KB operand tiles
  unsigned char* sF = smem;
  unsigned char* sS = smem + 64 * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int g = lane >> 4, l16 = lane & 15, q4 = l16 >> 2, cc = 4 * (l16 & 3);
  const int n = blockIdx.x / a.tilesP, p0 = (blockIdx.x - n * a.tilesP) * 64, c0 = blockIdx.y * 64;
  const int HW = a.HW, Cp = a.Cp;
  const int c = tid & 7, pbase = tid >> 3;
  const size_t img = (size_t)n * (size_t)HW;
  const unsigned short* S = a.s16 + (size_t)n * (size_t)Cp * (size_t)Cp;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < Cp; k0 += 64) {                // block-uniform trip count
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = pbase + 32 * u;
      const bool fok = p0 + r < HW && k0 + c * 8 < Cp;
      *reinterpret_cast<U4*>(style_slot(sF, r, c)) = load16_or_zero(a.f, (img + (size_t)(p0 + r)) * (size_t)Cp + k0 + c * 8, fok);
      const bool sok = k0 + r < Cp && c0 + c * 8 < Cp;
      *reinterpret_cast<U4*>(style_slot(sS, r, c)) = load16_or_zero(S, (size_t)(k0 + r) * (size_t)Cp + c0 + c * 8, sok);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      U4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {                    // A[m = pixel][k = 8g .. 8g + 7]: one 16-byte row read
        const int row = wr * 32 + i * 16 + l16;
        fa[i] = *reinterpret_cast<const U4*>(style_slot(sF, row, kk * 4 + g));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {                    // B[k = 8g .. 8g + 7][n = channel]: rows of s16 through the transposing read
        const int ch = wc * 32 + j * 16 + cc;
        fb[j] = style_tr_frag(sS, kk * 32 + 8 * g + q4, kk * 32 + 8 * g + 4 + q4, ch >> 3, (ch & 7) * 2);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16<DT>(fa[i], fb[j], acc[i][j]);
    }
  }
  __syncthreads();                                     // the operand tiles are dead: the fp32 output tile takes their place
  float* sO = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sO[(wr * 32 + i * 16 + 4 * g + r) * OLD + wc * 32 + j * 16 + l16] = acc[i][j][r];
  __syncthreads();

  const bool content = a.t != nullptr && a.g_content != nullptr;
  const float sc = content ? a.g_content[0] * a.coef_content : 0.f;
  const float ks = a.g_style[0] * a.coef_style * a.s_scale[n];
  const bool next = a.dnext != nullptr, mask = next && a.masked != 0;
  if (c0 + c * 8 < Cp) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = pbase + 32 * u;
      if (p0 + p >= HW) continue;
      const size_t off = (img + (size_t)(p0 + p)) * (size_t)Cp + c0 + c * 8;
      float fv[8], tv[8], dn[8], o[8];
      unpack8<DT>(*reinterpret_cast<const U4*>(a.f + off), fv);
      if (content) unpack8<DT>(*reinterpret_cast<const U4*>(a.t + off), tv);
      if (next) unpack8<DT>(*reinterpret_cast<const U4*>(a.dnext + off), dn);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float r = ks * sO[p * OLD + c * 8 + k];
        if (content) {
          const float x = fv[k] - tv[k];
          const float d = a.mode == DSR_FEAT_L1 ? (x > 0.f ? 1.f : (x < 0.f ? -1.f : x)) : 2.f * x;
          r += sc * d;
        }
        if (next) r += (mask && !(fv[k] > 0.f)) ? 0.f : dn[k];
        o[k] = r;
      }
      *reinterpret_cast<U4*>(a.df + off) = pack8<DT>(o);
    }
  }
}

static inline bool style_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool style_shape_ok(int N, int HW, int Cp) {
  return N >= 1 && HW >= 1 && Cp >= 8 && Cp % 8 == 0 && Cp <= STYLE_MAX_CP && (long long)N * (long long)HW < (1LL << 31);
}

// blocks per image of the loss reduction: a function of C alone (8192 entries per block, at most DSR_GRAM_LOSS_SLICES)
static inline int style_loss_slices(int C) {
  const int s = (C * C + 8191) / 8192;
  return s < 1 ? 1 : (s > DSR_GRAM_LOSS_SLICES ? DSR_GRAM_LOSS_SLICES : s);
}

extern "C" int dsr_gram_chunks(int HW) { return HW < 1 ? 0 : (HW + GRAM_CHUNK - 1) / GRAM_CHUNK; }

extern "C" size_t dsr_gram_workspace(int N, int HW, int Cp) {
  if (!style_shape_ok(N, HW, Cp)) return 0;
  return (size_t)N * (size_t)dsr_gram_chunks(HW) * (size_t)Cp * (size_t)Cp;
}

extern "C" int dsr_gram_fwd(int dtype, const void* f, int N, int HW, int C, int Cp, float scale, float* workspace, float* gram,
                            hipStream_t st) {
  DSR_REQUIRE(f && workspace && gram, "gram_fwd: null pointer");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype), "gram_fwd: dtype %d is neither bf16 nor f16", dtype);
  DSR_REQUIRE(style_shape_ok(N, HW, Cp), "gram_fwd: N = %d images of HW = %d pixels and Cp = %d channels (Cp a multiple of 8 up to %d, "
              "HW >= 1, N HW < 2^31)", N, HW, Cp, STYLE_MAX_CP);
  DSR_REQUIRE(C >= 1 && C <= Cp, "gram_fwd: C = %d real channels of Cp = %d", C, Cp);
  DSR_REQUIRE(style_aligned(f) && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)gram & 3) == 0,
              "gram_fwd: the map must be 16-byte aligned, workspace and gram 4-byte aligned");
  const int chunks = dsr_gram_chunks(HW), tiles = (Cp + 63) / 64;
  DSR_REQUIRE((long long)N * chunks < (1LL << 31), "gram_fwd: %d images x %d chunks exceed the grid", N, chunks);
  const dim3 grid((unsigned)(N * chunks), (unsigned)(tiles * (tiles + 1) / 2));
  if (dtype == DSR_DTYPE_BF16)
    hipLaunchKernelGGL((gram_fwd_kernel<DSR_DTYPE_BF16>), grid, dim3(256), 0, st, (const unsigned short*)f, HW, Cp, tiles, chunks, workspace);
  else
    hipLaunchKernelGGL((gram_fwd_kernel<DSR_DTYPE_F16>), grid, dim3(256), 0, st, (const unsigned short*)f, HW, Cp, tiles, chunks, workspace);
  if (int rc = dsr_launch_status("dsr_gram_fwd")) return rc;
  const size_t total = (size_t)N * (size_t)C * (size_t)C;
  const size_t want = (total + 255) / 256;
  hipLaunchKernelGGL(gram_fold_kernel, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(256), 0, st, workspace, C, Cp, chunks, scale,
                     total, gram);
  return dsr_launch_status("dsr_gram_fwd (fold)");
}

extern "C" int dsr_gram_loss(int dtype, const float* gram_f, const float* gram_t, int N, int C, int Cp, int mode, double* partial,
                             float* value, void* s16, float* s_scale, hipStream_t st) {
  DSR_REQUIRE(gram_f && gram_t && partial && value && s16 && s_scale, "gram_loss: null pointer");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype), "gram_loss: dtype %d is neither bf16 nor f16", dtype);
  DSR_REQUIRE(N >= 1 && N <= 65535 && Cp >= 8 && Cp % 8 == 0 && Cp <= STYLE_MAX_CP && C >= 1 && C <= Cp,
              "gram_loss: N = %d Gram matrices of C = %d, Cp = %d (Cp a multiple of 8 up to %d, 1 <= C <= Cp)", N, C, Cp, STYLE_MAX_CP);
  DSR_REQUIRE(mode == DSR_FEAT_L1 || mode == DSR_FEAT_MSE, "gram_loss: unknown mode %d", mode);
  DSR_REQUIRE(((uintptr_t)gram_f & 3) == 0 && ((uintptr_t)gram_t & 3) == 0 && ((uintptr_t)partial & 7) == 0 && ((uintptr_t)value & 3) == 0 &&
              style_aligned(s16) && ((uintptr_t)s_scale & 3) == 0, "gram_loss: misaligned pointer");
  const int slices = style_loss_slices(C);
  hipLaunchKernelGGL(gram_loss_reduce_kernel, dim3(slices, N), dim3(256), 0, st, gram_f, gram_t, C, mode, slices, partial);
  if (int rc = dsr_launch_status("dsr_gram_loss (reduce)")) return rc;
  const int oblocks = (Cp * Cp + 2047) / 2048;          // 8 entries per thread
  if (dtype == DSR_DTYPE_BF16)
    hipLaunchKernelGGL((gram_loss_operand_kernel<DSR_DTYPE_BF16>), dim3(oblocks, N), dim3(256), 0, st, gram_f, gram_t, C, Cp, mode, slices,
                       partial, (unsigned short*)s16, s_scale);
  else
    hipLaunchKernelGGL((gram_loss_operand_kernel<DSR_DTYPE_F16>), dim3(oblocks, N), dim3(256), 0, st, gram_f, gram_t, C, Cp, mode, slices,
                       partial, (unsigned short*)s16, s_scale);
  if (int rc = dsr_launch_status("dsr_gram_loss (operand)")) return rc;
  hipLaunchKernelGGL(gram_loss_fold_kernel, dim3(1), dim3(256), 0, st, partial, N * slices, (double)N * (double)C * (double)C, value);
  return dsr_launch_status("dsr_gram_loss (fold)");
}

extern "C" int dsr_featstyle_tap_bwd(int dtype, const void* f, const void* t, const void* dnext, const float* g_content,
                                     float coef_content, int mode, int masked, const void* s16, const float* s_scale,
                                     const float* g_style, float coef_style, void* df, int N, int HW, int Cp, hipStream_t st) {
  DSR_REQUIRE(f && s16 && s_scale && g_style && df, "featstyle_tap_bwd: null pointer");
  DSR_REQUIRE((t == nullptr) == (g_content == nullptr), "featstyle_tap_bwd: t and g_content come together (both null: a style-only tap)");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype), "featstyle_tap_bwd: dtype %d is neither bf16 nor f16", dtype);
  DSR_REQUIRE(style_shape_ok(N, HW, Cp), "featstyle_tap_bwd: N = %d images of HW = %d pixels and Cp = %d channels (Cp a multiple of 8 "
              "up to %d, HW >= 1, N HW < 2^31)", N, HW, Cp, STYLE_MAX_CP);
  DSR_REQUIRE(mode == DSR_FEAT_L1 || mode == DSR_FEAT_MSE, "featstyle_tap_bwd: unknown mode %d", mode);
  DSR_REQUIRE(style_aligned(f) && style_aligned(t) && style_aligned(dnext) && style_aligned(s16) && style_aligned(df) &&
              (((uintptr_t)g_content | (uintptr_t)g_style | (uintptr_t)s_scale) & 3) == 0,
              "featstyle_tap_bwd: maps and s16 must be 16-byte aligned, the scalars 4-byte aligned");
  const int tilesP = (HW + 63) / 64;
  DSR_REQUIRE((long long)N * tilesP < (1LL << 31), "featstyle_tap_bwd: %d images x %d pixel tiles exceed the grid", N, tilesP);
  StyleBwdArgs a;
  a.f = (const unsigned short*)f, a.t = (const unsigned short*)t, a.dnext = (const unsigned short*)dnext, a.s16 = (const unsigned short*)s16;
  a.g_content = g_content, a.g_style = g_style, a.s_scale = s_scale;
  a.df = (unsigned short*)df;
  a.coef_content = coef_content, a.coef_style = coef_style;
  a.mode = mode, a.masked = masked, a.HW = HW, a.Cp = Cp, a.tilesP = tilesP;
  const dim3 grid((unsigned)(N * tilesP), (unsigned)((Cp + 63) / 64));
  if (dtype == DSR_DTYPE_BF16)
    hipLaunchKernelGGL((featstyle_tap_bwd_kernel<DSR_DTYPE_BF16>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((featstyle_tap_bwd_kernel<DSR_DTYPE_F16>), grid, dim3(256), 0, st, a);
  return dsr_launch_status("dsr_featstyle_tap_bwd");
}
