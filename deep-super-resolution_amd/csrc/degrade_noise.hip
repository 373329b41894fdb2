// The pointwise pieces of the second-order Real-ESRGAN degradation on fp32 [B][3][H][W] batches in [0, 1] scaling: applying
// Gaussian or Poisson noise whose draws are inputs, and the two pointwise steps of the unsharp mask.  One thread per pixel
// position (all three channels: the grey Poisson term needs them together), consecutive lanes on consecutive pixels.
//
// noise_kernel, per sample b and pixel, in this statement order (every operation a single fp32 rounding):
//   Gaussian:  s = sigma[b] / 255.0f;                      n_c = gray[b] ? zg : z_c
//              y_c = min(max(fmaf(s, n_c, x_c), 0), 1)
//   Poisson:   q_c = rintf(min(max(255.0f * x_c, 0), 255)) / 255.0f          (half to even, as torch.round)
//              colour:  n_c = z_c / vals[b] - q_c
//              grey:    g = 0.2989f * q_0;  g = fmaf(0.587f, q_1, g);  g = fmaf(0.114f, q_2, g);  n_c = zg / vals[b] - g
//              y_c = min(max(fmaf(scale[b], n_c, x_c), 0), 1)
// usm_mask_kernel:     res = x - blur;  mask = fabsf(res) * 255.0f > threshold ? 1 : 0
// usm_combine_kernel:  res = x - blur;  sharp = min(max(fmaf(weight, res, x), 0), 1);  y = fmaf(soft, sharp - x, x)
//                      (= soft * sharp + (1 - soft) * x; in this form weight == 0 returns x itself for x in [0, 1])
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int NT = 256;

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

template <bool POISSON>
__global__ __launch_bounds__(NT) void noise_kernel(const float* __restrict__ x, const float* __restrict__ z, const float* __restrict__ zg,
                                                   const float* __restrict__ amount, const float* __restrict__ vals,
                                                   const unsigned char* __restrict__ gray, float* __restrict__ y, int plane,
                                                   unsigned total) {
  const unsigned n = blockIdx.x * NT + threadIdx.x;              // over B * plane pixel positions
  if (n >= total) return;
  const unsigned b = n / (unsigned)plane, p = n - b * (unsigned)plane;
  const size_t o = (size_t)b * 3 * plane + p;
  const bool grey = gray[b] != 0;
  const float x0 = x[o], x1 = x[o + plane], x2 = x[o + 2 * (size_t)plane];
  float n0, n1, n2, s;
  if constexpr (POISSON) {
    const float q0 = rintf(fminf(fmaxf(255.0f * x0, 0.0f), 255.0f)) / 255.0f;
    const float q1 = rintf(fminf(fmaxf(255.0f * x1, 0.0f), 255.0f)) / 255.0f;
    const float q2 = rintf(fminf(fmaxf(255.0f * x2, 0.0f), 255.0f)) / 255.0f;
    const float v = vals[b];
    s = amount[b];
    if (grey) {
      float g = 0.2989f * q0;
      g = fmaf(0.587f, q1, g);
      g = fmaf(0.114f, q2, g);
      n0 = n1 = n2 = zg[n] / v - g;
    } else {
      n0 = z[o] / v - q0;
      n1 = z[o + plane] / v - q1;
      n2 = z[o + 2 * (size_t)plane] / v - q2;
    }
  } else {
    s = amount[b] / 255.0f;
    if (grey) {
      n0 = n1 = n2 = zg[n];
    } else {
      n0 = z[o];
      n1 = z[o + plane];
      n2 = z[o + 2 * (size_t)plane];
    }
  }
  y[o] = clamp01(fmaf(s, n0, x0));
  y[o + plane] = clamp01(fmaf(s, n1, x1));
  y[o + 2 * (size_t)plane] = clamp01(fmaf(s, n2, x2));
}

__global__ __launch_bounds__(NT) void usm_mask_kernel(const float* __restrict__ x, const float* __restrict__ blur, float threshold,
                                                      float* __restrict__ mask, unsigned n) {
  const unsigned i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float res = x[i] - blur[i];
  mask[i] = fabsf(res) * 255.0f > threshold ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(NT) void usm_combine_kernel(const float* __restrict__ x, const float* __restrict__ blur,
                                                         const float* __restrict__ soft, float weight, float* __restrict__ y,
                                                         unsigned n) {
  const unsigned i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  const float res = v - blur[i];
  const float sharp = clamp01(fmaf(weight, res, v));
  y[i] = fmaf(soft[i], sharp - v, v);
}

// the shape checks of the two noise entry points; 0 when fine
int check_noise(const char* who, const void* x, const void* z, const void* zg, const void* amount, const void* gray, const void* y,
                int B, int H, int W) {
  if (!x || !z || !zg || !amount || !gray || !y) return dsr_fail(DSR_E_ARG, "%s: null pointer", who);
  if (B < 1 || H < 1 || W < 1) return dsr_fail(DSR_E_ARG, "%s: bad shape %dx3x%dx%d", who, B, H, W);
  if ((long long)B * 3 * H * W >= (1ll << 31)) return dsr_fail(DSR_E_ARG, "%s: B*3*H*W does not fit 31 bits", who);
  return 0;
}
int check_usm(const char* who, size_t n) {
  if (n == 0 || n >= ((size_t)1 << 31)) return dsr_fail(DSR_E_ARG, "%s: %zu elements, 1..2^31-1 are supported", who, n);
  return 0;
}
}  // namespace

extern "C" int dsr_noise_gaussian_f32(const float* x, const float* z, const float* zg, const float* sigma, const unsigned char* gray,
                                      float* y, int B, int H, int W, dsr_stream_t st) {
  if (int rc = check_noise("noise_gaussian_f32", x, z, zg, sigma, gray, y, B, H, W)) return rc;
  const unsigned total = (unsigned)B * H * W;
  hipLaunchKernelGGL(noise_kernel<false>, dim3((total + NT - 1) / NT), dim3(NT), 0, st, x, z, zg, sigma, (const float*)nullptr, gray, y,
                     H * W, total);
  return dsr_launch_status("dsr_noise_gaussian_f32");
}

extern "C" int dsr_noise_poisson_f32(const float* x, const float* z, const float* zg, const float* vals, const float* scale,
                                     const unsigned char* gray, float* y, int B, int H, int W, dsr_stream_t st) {
  if (!vals) return dsr_fail(DSR_E_ARG, "noise_poisson_f32: null pointer");
  if (int rc = check_noise("noise_poisson_f32", x, z, zg, scale, gray, y, B, H, W)) return rc;
  const unsigned total = (unsigned)B * H * W;
  hipLaunchKernelGGL(noise_kernel<true>, dim3((total + NT - 1) / NT), dim3(NT), 0, st, x, z, zg, scale, vals, gray, y, H * W, total);
  return dsr_launch_status("dsr_noise_poisson_f32");
}

extern "C" int dsr_usm_mask(const float* x, const float* blur, float threshold, float* mask, size_t n, dsr_stream_t st) {
  if (!x || !blur || !mask) return dsr_fail(DSR_E_ARG, "usm_mask: null pointer");
  if (int rc = check_usm("usm_mask", n)) return rc;
  hipLaunchKernelGGL(usm_mask_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, x, blur, threshold, mask, (unsigned)n);
  return dsr_launch_status("dsr_usm_mask");
}

extern "C" int dsr_usm_combine(const float* x, const float* blur, const float* soft, float weight, float* y, size_t n,
                               dsr_stream_t st) {
  if (!x || !blur || !soft || !y) return dsr_fail(DSR_E_ARG, "usm_combine: null pointer");
  if (int rc = check_usm("usm_combine", n)) return rc;
  hipLaunchKernelGGL(usm_combine_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, x, blur, soft, weight, y, (unsigned)n);
  return dsr_launch_status("dsr_usm_combine");
}
