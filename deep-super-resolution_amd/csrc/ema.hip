// Exponential moving average of a model's weights (optim.WeightEMA) and the exact exchange of two tensor sets (gfx950).
//
// Reference semantics: torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay) (first update copies, later
// ones lerp with 1 - decay), and the warm-up rule of timm / torch-ema, decay_k = min(decay, (1 + k) / (10 + k)).
//
// Streaming kernels, two reads and one write per element (swap: two and two).  The layout is multi_tensor.h's: up to 64
// tensors per launch, each an aligned span in chunks of DSR_EMA_CHUNK elements with 16-byte vector accesses in the body.
// Alignment is taken from the first operand; when the second one sits at another offset from a 16-byte boundary that
// tensor is cut into plain chunks from element 0 and runs on 4-byte accesses instead (DSR_EMA_VEC, decided per tensor).
// Every element is written by exactly one thread with a plain store: no atomics, the same bits on every run.  The
// averaged-step counter is only read here; ema_tick_kernel, one thread, launched on the same stream after every update
// launch of a step, is its only writer.
#include <math.h>

#include "dsr_common.h"
#include "dsr_kernels.h"
#include "multi_tensor.h"
#include "../../include/dsr_hip.h"

#define DSR_EMA_CHUNK 4096   // body elements per block: 4 16-byte vectors per thread
#define DSR_EMA_COPY 1       // flags: exact copy whatever the counter says
#define DSR_EMA_VEC 2        // flags: both operands share their offset from a 16-byte boundary
struct EmaGroup {
  float* a[DSR_MT_MAX];            // update: the shadow (written); swap: one side
  float* b[DSR_MT_MAX];            // update: the parameter (read only); swap: the other side
  size_t n[DSR_MT_MAX];
  unsigned char flags[DSR_MT_MAX];
  MtTable tb;
};
static_assert(sizeof(EmaGroup) <= 4096, "kernel arguments are limited to 4 KB");

// s + w * (p - s) on raw bits; w == 1 with COPY set never reaches the arithmetic, so a copy keeps NaN payloads and -0
__device__ __forceinline__ unsigned ema_mix(unsigned s, unsigned p, float w, bool copy) {
  const float sf = __uint_as_float(s), pf = __uint_as_float(p);
  return copy ? p : __float_as_uint(sf + w * (pf - sf));
}

// SWAP = false: a <- mix(a, b); SWAP = true: a <-> b
template <bool SWAP>
__device__ __forceinline__ void ema_chunk(const EmaGroup& g, float w, bool copy_all) {
  unsigned blk;
  const int t = mt_locate(g.tb, blk);
  unsigned* __restrict__ a = reinterpret_cast<unsigned*>(g.a[t]);
  unsigned* __restrict__ b = reinterpret_cast<unsigned*>(g.b[t]);
  const size_t n = g.n[t];
  const bool copy = copy_all || (g.flags[t] & DSR_EMA_COPY);
  const bool vec = g.flags[t] & DSR_EMA_VEC;
  auto one = [&](size_t i) {                       // one element on 4-byte accesses
    const unsigned x = a[i], y = b[i];
    if constexpr (SWAP) {
      a[i] = y;
      b[i] = x;
    } else {
      a[i] = ema_mix(x, y, w, copy);
    }
  };
  if (vec) {
    const MtSpan sp = mt_span(a, n, blk, DSR_EMA_CHUNK);
    U4* __restrict__ av = reinterpret_cast<U4*>(a + sp.head);
    U4* __restrict__ bv = reinterpret_cast<U4*>(b + sp.head);
#pragma unroll 4
    for (size_t i = sp.v0 + threadIdx.x; i < sp.v1; i += 256) {
      const U4 x = av[i], y = bv[i];
      if constexpr (SWAP) {
        av[i] = y;
        bv[i] = x;
      } else {
        U4 r;
        r.x = ema_mix(x.x, y.x, w, copy);
        r.y = ema_mix(x.y, y.y, w, copy);
        r.z = ema_mix(x.z, y.z, w, copy);
        r.w = ema_mix(x.w, y.w, w, copy);
        av[i] = r;
      }
    }
    if (blk == 0) {                               // at most 3 head elements on threads 0..2, 3 tail elements on 64..66
      size_t i = n;
      if (threadIdx.x < sp.head) i = threadIdx.x;
      else if (threadIdx.x >= 64 && sp.tail0 + (threadIdx.x - 64) < n) i = sp.tail0 + (threadIdx.x - 64);
      if (i < n) one(i);
    }
  } else {
    const size_t e0 = (size_t)blk * DSR_EMA_CHUNK;
    const size_t e1 = e0 + DSR_EMA_CHUNK < n ? e0 + DSR_EMA_CHUNK : n;
#pragma unroll 4
    for (size_t i = e0 + threadIdx.x; i < e1; i += 256) one(i);
  }
}

__global__ __launch_bounds__(256) void ema_update_kernel(const EmaGroup g, float decay, int mode,
                                                         const int* __restrict__ n_averaged,
                                                         const float* __restrict__ found_inf) {
  if (found_inf && found_inf[0] != 0.f) return;          // the optimiser skipped this step: nothing moves
  const int n = n_averaged[0];
  float d = decay;
  if (mode == DSR_EMA_WARMUP) {
    const float k = (float)n + 1.f;
    d = fminf(decay, (1.f + k) / (10.f + k));
  }
  ema_chunk<false>(g, 1.f - d, mode == DSR_EMA_TORCH && n == 0);
}
__global__ __launch_bounds__(256) void ema_swap_kernel(const EmaGroup g) { ema_chunk<true>(g, 0.f, false); }
__global__ void ema_tick_kernel(int* n_averaged, const float* found_inf) {
  if (!found_inf || found_inf[0] == 0.f) n_averaged[0] += 1;
}

// every entry is checked before the first launch; 0: fine, < 0: dsr_fail's code.  A tensor holds fewer than 2^42 elements
// (2^30 blocks of DSR_EMA_CHUNK).
static int ema_check_tables(const char* what, int count, float* const* a, const float* const* b, const size_t* n) {
  if (count < 0) return dsr_fail(DSR_E_ARG, "%s: count %d is negative", what, count);
  if (count && (!a || !b || !n)) return dsr_fail(DSR_E_ARG, "%s: null table", what);
  for (int i = 0; i < count; ++i) {
    if (!n[i] || (!a[i] && !b[i])) continue;             // skipped
    if (!a[i] || !b[i]) return dsr_fail(DSR_E_ARG, "%s: tensor %d has %zu elements and one null pointer", what, i, n[i]);
    if (n[i] >= ((size_t)1 << 42) || (((uintptr_t)a[i] | (uintptr_t)b[i]) & 3))
      return dsr_fail(DSR_E_ARG, "%s: tensor %d is too large or not 4-byte aligned", what, i);
  }
  return 0;
}

// the number of launches made (0: every entry was one of the skipped kinds)
template <class Launch>
static int ema_for_groups(int count, float* const* a, const float* const* b, const size_t* n, const unsigned char* copy,
                           Launch launch) {
  auto vec = [&](int i) { return (((uintptr_t)a[i] ^ (uintptr_t)b[i]) & 15) == 0; };
  return mt_for_groups<EmaGroup>(
      count, DSR_MT_MAX, [&](int i) { return !n[i] || !a[i] || a[i] == b[i]; },         // (a tensor against itself: nothing to do)
      [&](int i) { return vec(i) ? mt_span_blocks(a[i], n[i], DSR_EMA_CHUNK) : mt_blocks(n[i], DSR_EMA_CHUNK); },
      [&](EmaGroup& g, int j, int i) {
        g.a[j] = a[i];
        g.b[j] = const_cast<float*>(b[i]);
        g.n[j] = n[i];
        g.flags[j] = (unsigned char)((copy && copy[i] ? DSR_EMA_COPY : 0) | (vec(i) ? DSR_EMA_VEC : 0));
      },
      launch);
}

extern "C" int dsr_ema_update_multi(int count, float* const* shadow, const float* const* p, const size_t* n,
                                    const unsigned char* copy, float decay, int mode, const int* n_averaged,
                                    const float* found_inf, hipStream_t st) {
  if (int rc = ema_check_tables("ema_update_multi", count, shadow, p, n)) return rc;
  DSR_REQUIRE(n_averaged && ((uintptr_t)n_averaged & 3) == 0, "ema_update_multi: null or misaligned n_averaged");
  DSR_REQUIRE(((uintptr_t)found_inf & 3) == 0, "ema_update_multi: misaligned found_inf");
  DSR_REQUIRE(decay >= 0.f && decay <= 1.f, "ema_update_multi: decay %g is outside [0, 1]", (double)decay);   // (NaN fails too)
  DSR_REQUIRE(mode == DSR_EMA_TORCH || mode == DSR_EMA_WARMUP, "ema_update_multi: unknown mode %d", mode);
  const int launches = ema_for_groups(count, shadow, p, n, copy, [&](const EmaGroup& g, unsigned blocks) {
    hipLaunchKernelGGL(ema_update_kernel, dim3(blocks), dim3(256), 0, st, g, decay, mode, n_averaged, found_inf);
  });
  return launches ? dsr_launch_status("dsr_ema_update_multi") : 0;
}

extern "C" int dsr_ema_tick(int* n_averaged, const float* found_inf, hipStream_t st) {
  DSR_REQUIRE(n_averaged && ((uintptr_t)n_averaged & 3) == 0, "ema_tick: null or misaligned n_averaged");
  DSR_REQUIRE(((uintptr_t)found_inf & 3) == 0, "ema_tick: misaligned found_inf");
  hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(1), 0, st, n_averaged, found_inf);
  return dsr_launch_status("dsr_ema_tick");
}

extern "C" int dsr_ema_swap_multi(int count, float* const* a, float* const* b, const size_t* n, hipStream_t st) {
  if (int rc = ema_check_tables("ema_swap_multi", count, a, b, n)) return rc;
  const int launches = ema_for_groups(count, a, b, n, nullptr, [&](const EmaGroup& g, unsigned blocks) {
    hipLaunchKernelGGL(ema_swap_kernel, dim3(blocks), dim3(256), 0, st, g);
  });
  return launches ? dsr_launch_status("dsr_ema_swap_multi") : 0;
}
