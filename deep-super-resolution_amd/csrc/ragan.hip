// Relativistic average GAN loss on logits (ESRGAN; BasicSR ESRGANModel.optimize_parameters), gfx950.
//
//   mu = mean(other);  z_i = x_i - mu;  loss = mean_i l(z_i),  l = the per-element term of dsr_gan_loss (pointwise.hip)
//   grad_x[i] = l'(z_i) / n;  grad_other[j] = -(sum_i l'(z_i)) / (n m)
//
// Reduction plan: every sum is a thread-strided double sum, folded over the wave, the block's four waves and then
// the blocks in block order, exactly as gan_loss_kernel / gan_loss_fold_kernel do -- no atomics, no host read.
//   1. rel_sum_kernel        partials of `other`, one double per block
//   2. rel_elem_kernel       every block folds those partials in block order (the same adds in every block, so the same mu),
//                            rounds mu to fp32 once and hands it to its threads through LDS; then the element pass: z, l(z),
//                            l'(z), grad_x, one partial of l and one of l' per block
//   3. rel_finish_kernel     block 0 folds the loss; with grad_other, every block folds the partials of l' to the one value
//                            -(sum l') / (n m), rounded once, and stores it to its share of grad_other
// A block-order fold is one thread adding up to 1024 doubles one after the other.  Read from global memory that is a chain of
// dependent load latencies (measured: ~50 us for 768 partials); here the block first copies the table to LDS with all its
// threads, and the one thread then adds from LDS -- the same adds in the same order.
// The workspace holds, in doubles: blocks(m) partials of other, blocks(n) of l, blocks(n) of l'.
#include <math.h>

#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define REL_MAX_BLOCKS 1024          // dsr_gan_loss_blocks never answers more

__device__ __forceinline__ double rel_block_sum(double s, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[0] + partial[1] + ... in that order, by one thread, from the block's LDS copy (call after the __syncthreads that
// follows rel_stage)
__device__ __forceinline__ void rel_stage(const double* __restrict__ partial, int blocks, double* stage) {
  for (int b = threadIdx.x; b < blocks; b += blockDim.x) stage[b] = partial[b];
}
__device__ __forceinline__ double rel_fold(const double* stage, int blocks) {
  double t = 0.0;
#pragma unroll 8
  for (int b = 0; b < blocks; ++b) t += stage[b];
  return t;
}

__global__ __launch_bounds__(256) void rel_sum_kernel(const float* __restrict__ other, size_t m, double* __restrict__ partial) {
  __shared__ double red[4];
  double s = 0.0;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) s += (double)other[j];
  s = rel_block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__device__ __forceinline__ float rel_sigmoid(float z) {      // gan_sigmoid of pointwise.hip: no overflow on either side
  if (z >= 0.f) return 1.f / (1.f + expf(-z));
  const float e = expf(z);
  return e / (1.f + e);
}

// part_g may be null (no grad_other wanted): the sum of l' is then not formed.  grad_x may be null.
__global__ __launch_bounds__(256) void rel_elem_kernel(const float* __restrict__ x, size_t n, const double* __restrict__ part_o,
                                                       int blocks_o, size_t m, int kind, int real, int is_disc,
                                                       float* __restrict__ grad_x, double* __restrict__ part_l,
                                                       double* __restrict__ part_g) {
  __shared__ double stage[REL_MAX_BLOCKS];
  __shared__ double red[4];
  __shared__ float mu_s;
  rel_stage(part_o, blocks_o, stage);
  __syncthreads();
  if (threadIdx.x == 0) mu_s = (float)(rel_fold(stage, blocks_o) / (double)m);
  __syncthreads();
  const float mu = mu_s;
  const float fn = (float)n;
  const float sgn = real ? -1.f : 1.f;
  double s = 0.0, sg = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float xi = x[i] - mu;
    float val, g;
    if (kind == DSR_GAN_VANILLA) {
      const float z = sgn * xi;
      val = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
      g = sgn * rel_sigmoid(z);
    } else if (kind == DSR_GAN_LSGAN) {
      const float d = xi - (real ? 1.f : 0.f);
      val = d * d;
      g = 2.f * d;
    } else if (is_disc) {
      const float h = 1.f + sgn * xi;
      val = fmaxf(h, 0.f);
      g = h > 0.f ? sgn : 0.f;
    } else {
      val = -xi;
      g = -1.f;
    }
    s += (double)val;
    sg += (double)g;
    if (grad_x) grad_x[i] = g / fn;
  }
  s = rel_block_sum(s, red);
  if (threadIdx.x == 0) part_l[blockIdx.x] = s;
  if (part_g) {
    __syncthreads();                                         // red is reused
    sg = rel_block_sum(sg, red);
    if (threadIdx.x == 0) part_g[blockIdx.x] = sg;
  }
}

// Block 0: loss[0].  grad_other given (then part_g is too): every block folds part_g to the same word and stores it to its
// grid-strided share of grad_other.  In block 0 the two folds run side by side on threads 0 and 64 (two waves).
__global__ __launch_bounds__(256) void rel_finish_kernel(const double* __restrict__ part_l, const double* __restrict__ part_g,
                                                         int blocks, size_t n, size_t m, float* __restrict__ loss,
                                                         float* __restrict__ grad_other) {
  __shared__ double stage_l[REL_MAX_BLOCKS];
  __shared__ double stage_g[REL_MAX_BLOCKS];
  __shared__ float g_s;
  if (blockIdx.x == 0) rel_stage(part_l, blocks, stage_l);
  if (grad_other) rel_stage(part_g, blocks, stage_g);
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 64) loss[0] = (float)(rel_fold(stage_l, blocks) / (double)n);
  if (!grad_other) return;
  if (threadIdx.x == 0) g_s = (float)(-rel_fold(stage_g, blocks) / ((double)n * (double)m));
  __syncthreads();
  const float g = g_s;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) grad_other[j] = g;
}

extern "C" size_t dsr_rel_gan_loss_workspace(size_t n, size_t m) {
  if (n == 0 || m == 0) return 0;
  return sizeof(double) * ((size_t)dsr_gan_loss_blocks(m) + 2 * (size_t)dsr_gan_loss_blocks(n));
}

extern "C" int dsr_rel_gan_loss(const float* x, size_t n, const float* other, size_t m, int kind, int target_is_real, int is_disc,
                                float* grad_x, float* grad_other, void* ws, float* loss, hipStream_t st) {
  DSR_REQUIRE(x && other && ws && loss, "rel_gan_loss: null pointer");
  DSR_REQUIRE(n > 0 && m > 0, "rel_gan_loss: empty tensor (n %zu, m %zu)", n, m);
  DSR_REQUIRE(kind == DSR_GAN_VANILLA || kind == DSR_GAN_LSGAN || kind == DSR_GAN_HINGE, "rel_gan_loss: unknown kind %d", kind);
  DSR_REQUIRE((((uintptr_t)x | (uintptr_t)other | (uintptr_t)grad_x | (uintptr_t)grad_other | (uintptr_t)loss) & 3) == 0 &&
                  ((uintptr_t)ws & 7) == 0,
              "rel_gan_loss: misaligned pointer");
  const int bo = dsr_gan_loss_blocks(m), bx = dsr_gan_loss_blocks(n);
  DSR_REQUIRE(bo >= 1 && bo <= REL_MAX_BLOCKS && bx >= 1 && bx <= REL_MAX_BLOCKS, "rel_gan_loss: partial table of %d / %d blocks", bo, bx);
  double* part_o = (double*)ws;
  double* part_l = part_o + bo;
  double* part_g = grad_other ? part_l + bx : nullptr;
  hipLaunchKernelGGL(rel_sum_kernel, dim3(bo), dim3(256), 0, st, other, m, part_o);
  hipLaunchKernelGGL(rel_elem_kernel, dim3(bx), dim3(256), 0, st, x, n, (const double*)part_o, bo, m, kind, target_is_real ? 1 : 0,
                     is_disc ? 1 : 0, grad_x, part_l, part_g);
  hipLaunchKernelGGL(rel_finish_kernel, dim3(grad_other ? bo : 1), dim3(256), 0, st, (const double*)part_l, (const double*)part_g,
                     bx, n, m, loss, grad_other);
  return dsr_launch_status("dsr_rel_gan_loss");
}
