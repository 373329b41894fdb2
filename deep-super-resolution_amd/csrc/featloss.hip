// Feature-space loss taps (perceptual.VggFeatureLoss, functional.FeatureTap) for gfx950.
//
// A tap compares two 16-bit NHWC feature maps f (generated image) and t (target) where they already live -- no fp32 NCHW copy
// of the map is made.  Pad channels are zero in both maps, so a map is simply P * Cp / 8 16-byte vectors.
//   tap_fwd : per-block fp32 partial of sum |f - t| (L1) or sum (f - t)^2 (MSE), and optionally relu_out = max(f, 0) in the same
//             pass (a pre-activation tap feeds the next layer without a second read of the map)
//   fold    : one block sums a tap's partials in a fixed order (double) and writes value[0] = (float)sum / count
//   tap_bwd : df = (dnext ? (masked ? dnext * (f > 0) : dnext) : 0) + g[0] * coef * d,  d = sign(f - t) | 2 (f - t): the next
//             layer's gradient, the ReLU mask and the tap's own term in one launch, one rounding per element
//   relu    : out = max(x, 0) (the target's trunk behind a pre-activation tap, which has no f / t pair to ride on)
//   combine : out[0] = sum_k w[k] * v_k[0] over up to 32 one-element device scalars; combine_bwd: gout[k] = g[0] * w[k]
// Streaming kernels: 16-byte vector loads and stores, the grid of the other pointwise reductions (dsr_pw_reduce_blocks), wave
// reduction + one LDS step per block.  Every partial is written by one thread with a plain store and every sum runs in a
// fixed order: no atomics, the same bits on every run.
#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define DSR_FEAT_MAX_TERMS 32

// sum of the block's 256 per-thread values, valid in thread 0 (fixed order: xor tree inside a wave, then waves 0..3)
__device__ __forceinline__ float featloss_block_sum(float v) {
  __shared__ float wsum[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// block b owns vectors [b * vpb, min((b + 1) * vpb, nvec))
template <int DT, int MODE, bool RELU>
__global__ __launch_bounds__(256) void featloss_tap_fwd_kernel(const U4* __restrict__ f, const U4* __restrict__ t,
                                                               U4* __restrict__ relu_out, size_t nvec, size_t vpb,
                                                               float* __restrict__ partial) {
  const size_t v0 = (size_t)blockIdx.x * vpb;
  const size_t v1 = v0 + vpb < nvec ? v0 + vpb : nvec;
  float acc = 0.f;
#pragma unroll 2
  for (size_t i = v0 + threadIdx.x; i < v1; i += 256) {
    const U4 fv = f[i], tv = t[i];
    float a[8], b[8];
    unpack8<DT>(fv, a);
    unpack8<DT>(tv, b);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = a[k] - b[k];
      s += MODE == DSR_FEAT_L1 ? fabsf(d) : d * d;
    }
    acc += s;
    if constexpr (RELU) {
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = a[k] > 0.f ? a[k] : 0.f;     // (NaN becomes 0, as the fused conv + ReLU epilogue has it)
      relu_out[i] = pack8<DT>(a);
    }
  }
  const float tot = featloss_block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void featloss_fold_kernel(const float* __restrict__ partial, int blocks, float count,
                                                            float* __restrict__ value) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < blocks; i += 256) s += (double)partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) value[0] = (float)sh[0] / count;
}

template <int DT, int MODE, bool MASK, bool NEXT>
__global__ __launch_bounds__(256) void featloss_tap_bwd_kernel(const U4* __restrict__ f, const U4* __restrict__ t,
                                                               const U4* __restrict__ dnext, const float* __restrict__ g,
                                                               float coef, U4* __restrict__ df, size_t nvec) {
  const float s = g[0] * coef;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    const U4 fv = f[i], tv = t[i];
    float a[8], b[8], dn[8];
    unpack8<DT>(fv, a);
    unpack8<DT>(tv, b);
    if constexpr (NEXT) {
      const U4 nv = dnext[i];
      unpack8<DT>(nv, dn);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float x = a[k] - b[k];
      // sign(0) = 0; a NaN difference stays NaN, so an overflow upstream is not hidden from a loss scaler
      const float d = MODE == DSR_FEAT_L1 ? (x > 0.f ? 1.f : (x < 0.f ? -1.f : x)) : 2.f * x;
      float r = s * d;
      if constexpr (NEXT) r += (MASK && !(a[k] > 0.f)) ? 0.f : dn[k];
      a[k] = r;
    }
    df[i] = pack8<DT>(a);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void featloss_relu_kernel(const U4* __restrict__ x, U4* __restrict__ out, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    float a[8];
    unpack8<DT>(x[i], a);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = a[k] > 0.f ? a[k] : 0.f;
    out[i] = pack8<DT>(a);
  }
}

struct FeatTerms {
  const float* v[DSR_FEAT_MAX_TERMS];
  float w[DSR_FEAT_MAX_TERMS];
  int n;
};
__global__ void featloss_combine_kernel(const FeatTerms c, float* __restrict__ out) {
  float s = 0.f;
  for (int k = 0; k < c.n; ++k) s += c.w[k] * c.v[k][0];
  out[0] = s;
}
__global__ void featloss_combine_bwd_kernel(const FeatTerms c, const float* __restrict__ g, float* __restrict__ gout) {
  if ((int)threadIdx.x < c.n) gout[threadIdx.x] = g[0] * c.w[threadIdx.x];
}

static inline bool feat_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool feat_shape_ok(size_t P, int Cp) { return P > 0 && Cp >= 8 && Cp % 8 == 0 && P < ((size_t)1 << 40) / (size_t)Cp; }
// grid of the element-wise kernels: one vector per thread up to 2048 blocks, grid-stride beyond
static inline unsigned feat_stream_grid(size_t nvec) {
  const size_t want = (nvec + 255) / 256;
  return (unsigned)(want > 2048 ? 2048 : want);
}

#define FEAT_DT_SWITCH(dtype, ...)          \
  do {                                      \
    if ((dtype) == DSR_DTYPE_BF16) {        \
      constexpr int DT = DSR_DTYPE_BF16;    \
      __VA_ARGS__;                          \
    } else {                                \
      constexpr int DT = DSR_DTYPE_F16;     \
      __VA_ARGS__;                          \
    }                                       \
  } while (0)
#define FEAT_MODE_SWITCH(mode, ...)         \
  do {                                      \
    if ((mode) == DSR_FEAT_L1) {            \
      constexpr int MD = DSR_FEAT_L1;       \
      __VA_ARGS__;                          \
    } else {                                \
      constexpr int MD = DSR_FEAT_MSE;      \
      __VA_ARGS__;                          \
    }                                       \
  } while (0)
#define FEAT_BOOL_SWITCH(flag, NAME, ...)   \
  do {                                      \
    if (flag) {                             \
      constexpr bool NAME = true;           \
      __VA_ARGS__;                          \
    } else {                                \
      constexpr bool NAME = false;          \
      __VA_ARGS__;                          \
    }                                       \
  } while (0)

extern "C" int dsr_featloss_blocks(size_t P) {
  if (P == 0) return 0;
  int rpb = 0;
  return dsr_pw_reduce_blocks(P, &rpb);
}

extern "C" int dsr_featloss_tap_fwd(int dtype, const void* f, const void* t, void* relu_out, size_t P, int Cp, int mode,
                                    float* partial, hipStream_t st) {
  DSR_REQUIRE(f && t && partial, "featloss_tap_fwd: null pointer");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype), "featloss_tap_fwd: dtype %d is neither bf16 nor f16", dtype);
  DSR_REQUIRE(feat_shape_ok(P, Cp), "featloss_tap_fwd: P = %zu pixels of Cp = %d channels (Cp must be a positive multiple of 8, P > 0)", P, Cp);
  DSR_REQUIRE(mode == DSR_FEAT_L1 || mode == DSR_FEAT_MSE, "featloss_tap_fwd: unknown mode %d", mode);
  DSR_REQUIRE(feat_aligned(f) && feat_aligned(t) && feat_aligned(relu_out), "featloss_tap_fwd: maps must be 16-byte aligned");
  int rpb = 0;
  const int blocks = dsr_pw_reduce_blocks(P, &rpb);
  const size_t nvec = P * (size_t)(Cp / 8), vpb = (size_t)rpb * (size_t)(Cp / 8);
  FEAT_DT_SWITCH(dtype, FEAT_MODE_SWITCH(mode, FEAT_BOOL_SWITCH(relu_out != nullptr, RL,
      hipLaunchKernelGGL((featloss_tap_fwd_kernel<DT, MD, RL>), dim3(blocks), dim3(256), 0, st, (const U4*)f, (const U4*)t,
                         (U4*)relu_out, nvec, vpb, partial))));
  return dsr_launch_status("dsr_featloss_tap_fwd");
}

extern "C" int dsr_featloss_fold(const float* partial, int blocks, float count, float* value, hipStream_t st) {
  DSR_REQUIRE(partial && value, "featloss_fold: null pointer");
  DSR_REQUIRE(blocks > 0 && count > 0.f, "featloss_fold: %d partials over %g elements", blocks, (double)count);
  hipLaunchKernelGGL(featloss_fold_kernel, dim3(1), dim3(256), 0, st, partial, blocks, count, value);
  return dsr_launch_status("dsr_featloss_fold");
}

extern "C" int dsr_featloss_tap_bwd(int dtype, const void* f, const void* t, const void* dnext, const float* g, float coef,
                                    int mode, int masked, void* df, size_t P, int Cp, hipStream_t st) {
  DSR_REQUIRE(f && t && g && df, "featloss_tap_bwd: null pointer");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype), "featloss_tap_bwd: dtype %d is neither bf16 nor f16", dtype);
  DSR_REQUIRE(feat_shape_ok(P, Cp), "featloss_tap_bwd: P = %zu pixels of Cp = %d channels (Cp must be a positive multiple of 8, P > 0)", P, Cp);
  DSR_REQUIRE(mode == DSR_FEAT_L1 || mode == DSR_FEAT_MSE, "featloss_tap_bwd: unknown mode %d", mode);
  DSR_REQUIRE(feat_aligned(f) && feat_aligned(t) && feat_aligned(dnext) && feat_aligned(df) && ((uintptr_t)g & 3) == 0,
              "featloss_tap_bwd: maps must be 16-byte aligned, g 4-byte aligned");
  const size_t nvec = P * (size_t)(Cp / 8);
  const bool mask = masked != 0 && dnext != nullptr;
  FEAT_DT_SWITCH(dtype, FEAT_MODE_SWITCH(mode, FEAT_BOOL_SWITCH(mask, MK, FEAT_BOOL_SWITCH(dnext != nullptr, NX,
      hipLaunchKernelGGL((featloss_tap_bwd_kernel<DT, MD, MK, NX>), dim3(feat_stream_grid(nvec)), dim3(256), 0, st, (const U4*)f,
                         (const U4*)t, (const U4*)dnext, g, coef, (U4*)df, nvec)))));
  return dsr_launch_status("dsr_featloss_tap_bwd");
}

extern "C" int dsr_featloss_relu(int dtype, const void* x, void* out, size_t P, int Cp, hipStream_t st) {
  DSR_REQUIRE(x && out, "featloss_relu: null pointer");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype), "featloss_relu: dtype %d is neither bf16 nor f16", dtype);
  DSR_REQUIRE(feat_shape_ok(P, Cp), "featloss_relu: P = %zu pixels of Cp = %d channels (Cp must be a positive multiple of 8, P > 0)", P, Cp);
  DSR_REQUIRE(feat_aligned(x) && feat_aligned(out), "featloss_relu: maps must be 16-byte aligned");
  const size_t nvec = P * (size_t)(Cp / 8);
  FEAT_DT_SWITCH(dtype, hipLaunchKernelGGL((featloss_relu_kernel<DT>), dim3(feat_stream_grid(nvec)), dim3(256), 0, st,
                                           (const U4*)x, (U4*)out, nvec));
  return dsr_launch_status("dsr_featloss_relu");
}

static int feat_terms(const char* what, int n, const float* const* values, const float* weights, FeatTerms* c) {
  if (n < 1 || n > DSR_FEAT_MAX_TERMS) return dsr_fail(DSR_E_ARG, "%s: %d terms (1 .. %d)", what, n, DSR_FEAT_MAX_TERMS);
  if (!weights) return dsr_fail(DSR_E_ARG, "%s: null weight table", what);
  c->n = n;
  for (int k = 0; k < DSR_FEAT_MAX_TERMS; ++k) {
    c->v[k] = nullptr;
    c->w[k] = 0.f;
  }
  for (int k = 0; k < n; ++k) {
    if (values && (!values[k] || ((uintptr_t)values[k] & 3))) return dsr_fail(DSR_E_ARG, "%s: term %d is null or misaligned", what, k);
    c->v[k] = values ? values[k] : nullptr;
    c->w[k] = weights[k];
  }
  return 0;
}

extern "C" int dsr_featloss_combine(int n, const float* const* values, const float* weights, float* out, hipStream_t st) {
  DSR_REQUIRE(values && out, "featloss_combine: null pointer");
  FeatTerms c;
  if (int rc = feat_terms("featloss_combine", n, values, weights, &c)) return rc;
  hipLaunchKernelGGL(featloss_combine_kernel, dim3(1), dim3(1), 0, st, c, out);
  return dsr_launch_status("dsr_featloss_combine");
}

extern "C" int dsr_featloss_combine_bwd(int n, const float* weights, const float* g, float* gout, hipStream_t st) {
  DSR_REQUIRE(g && gout, "featloss_combine_bwd: null pointer");
  FeatTerms c;
  if (int rc = feat_terms("featloss_combine_bwd", n, nullptr, weights, &c)) return rc;
  hipLaunchKernelGGL(featloss_combine_bwd_kernel, dim3(1), dim3(64), 0, st, c, g, gout);
  return dsr_launch_status("dsr_featloss_combine_bwd");
}
