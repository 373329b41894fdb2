// Exponential moving average of a model's weights (optim.WeightEMA) and the exact exchange of two tensor sets (gfx950).
//
// Reference semantics: torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay) (first update copies, later
// ones lerp with 1 - decay), and the warm-up rule of timm / torch-ema, decay_k = min(decay, (1 + k) / (10 + k)).
//
// Streaming kernels, two reads and one write per element (swap: two and two).  The layout is amp_check_kernel's
// (pointwise.hip): up to 64 tensors per launch behind a block-to-tensor table, the 16-byte aligned body of a tensor cut
// into chunks of DSR_EMA_CHUNK elements, one block each, 16-byte vector accesses in the body; the tensor's first block
// also does the scalar head (a view may start 4, 8 or 12 bytes off a 16-byte boundary) and the tail.  Alignment is taken
// from the first operand; when the second one sits at another offset from a 16-byte boundary the body of that tensor runs
// on 4-byte accesses instead.  Every element is written by exactly one thread with a plain store: no atomics, the same
// bits on every run.  The averaged-step counter is only read here; ema_tick_kernel, one thread, launched on the same
// stream after every update launch of a step, is its only writer.
#include <math.h>

#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define DSR_EMA_GROUP 64
#define DSR_EMA_CHUNK 4096   // body elements per block: 4 16-byte vectors per thread
#define DSR_EMA_COPY 1       // flags: exact copy whatever the counter says
#define DSR_EMA_VEC 2        // flags: both operands share their offset from a 16-byte boundary
struct EmaGroup {
  float* a[DSR_EMA_GROUP];         // update: the shadow (written); swap: one side
  float* b[DSR_EMA_GROUP];         // update: the parameter (read only); swap: the other side
  size_t n[DSR_EMA_GROUP];
  unsigned first_block[DSR_EMA_GROUP + 1];
  unsigned char flags[DSR_EMA_GROUP];
  int count;
};
static_assert(sizeof(EmaGroup) <= 4096, "kernel arguments are limited to 4 KB");

static __host__ __device__ inline size_t ema_head(const void* a, size_t n) {
  const size_t h = ((16 - ((size_t)(uintptr_t)a & 15)) & 15) / 4;
  return h < n ? h : n;
}

// s + w * (p - s) on raw bits; w == 1 with COPY set never reaches the arithmetic, so a copy keeps NaN payloads and -0
__device__ __forceinline__ unsigned ema_mix(unsigned s, unsigned p, float w, bool copy) {
  const float sf = __uint_as_float(s), pf = __uint_as_float(p);
  return copy ? p : __float_as_uint(sf + w * (pf - sf));
}

// SWAP = false: a <- mix(a, b); SWAP = true: a <-> b
template <bool SWAP>
__device__ __forceinline__ void ema_chunk(const EmaGroup& g, float w, bool copy_all) {
  int t = 0;
  while (t + 1 < g.count && blockIdx.x >= g.first_block[t + 1]) ++t;      // wave-uniform scan of <= 64 entries
  const unsigned blk = blockIdx.x - g.first_block[t];
  unsigned* __restrict__ a = reinterpret_cast<unsigned*>(g.a[t]);
  unsigned* __restrict__ b = reinterpret_cast<unsigned*>(g.b[t]);
  const size_t n = g.n[t];
  const bool copy = copy_all || (g.flags[t] & DSR_EMA_COPY);
  const bool vec = g.flags[t] & DSR_EMA_VEC;
  const size_t head = vec ? ema_head(a, n) : 0;
  const size_t nvec = vec ? (n - head) / 4 : 0;
  const size_t body = vec ? nvec * 4 : n;        // elements handled in chunks, as vectors or one by one
  const size_t e0 = (size_t)blk * DSR_EMA_CHUNK;
  const size_t e1 = e0 + DSR_EMA_CHUNK < body ? e0 + DSR_EMA_CHUNK : body;
  if (vec) {
    U4* __restrict__ av = reinterpret_cast<U4*>(a + head);
    U4* __restrict__ bv = reinterpret_cast<U4*>(b + head);
#pragma unroll 4
    for (size_t i = e0 / 4 + threadIdx.x; i < e1 / 4; i += 256) {
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
  } else {
#pragma unroll 4
    for (size_t i = e0 + threadIdx.x; i < e1; i += 256) {
      const unsigned x = a[i], y = b[i];
      if constexpr (SWAP) {
        a[i] = y;
        b[i] = x;
      } else {
        a[i] = ema_mix(x, y, w, copy);
      }
    }
  }
  if (blk == 0 && vec) {                          // at most 3 head and 3 tail elements
    const size_t tail0 = head + body;
    size_t i = n;
    if (threadIdx.x < head) i = threadIdx.x;
    else if (threadIdx.x >= 64 && tail0 + (threadIdx.x - 64) < n) i = tail0 + (threadIdx.x - 64);
    if (i < n) {
      const unsigned x = a[i], y = b[i];
      if constexpr (SWAP) {
        a[i] = y;
        b[i] = x;
      } else {
        a[i] = ema_mix(x, y, w, copy);
      }
    }
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

// every entry is checked before the first launch; 0: fine, < 0: dsr_fail's code
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
  EmaGroup g;
  g.count = 0;
  size_t blocks = 0;
  int launches = 0;
  auto flush = [&]() {
    if (!g.count) return;
    g.first_block[g.count] = (unsigned)blocks;
    launch(g, (unsigned)blocks);
    ++launches;
    g.count = 0;
    blocks = 0;
  };
  for (int i = 0; i < count; ++i) {
    if (!n[i] || !a[i] || a[i] == b[i]) continue;          // (a tensor against itself: nothing to do)
    const bool vec = (((uintptr_t)a[i] ^ (uintptr_t)b[i]) & 15) == 0;
    const size_t body = vec ? (n[i] - ema_head(a[i], n[i])) / 4 * 4 : n[i];
    const size_t nb = body ? (body + DSR_EMA_CHUNK - 1) / DSR_EMA_CHUNK : 1;      // (a block for head / tail alone)
    if (g.count == DSR_EMA_GROUP || blocks + nb > 0x7fffffffull) flush();
    g.a[g.count] = a[i];
    g.b[g.count] = const_cast<float*>(b[i]);
    g.n[g.count] = n[i];
    g.flags[g.count] = (unsigned char)((copy && copy[i] ? DSR_EMA_COPY : 0) | (vec ? DSR_EMA_VEC : 0));
    g.first_block[g.count] = (unsigned)blocks;
    blocks += nb;
    ++g.count;
  }
  flush();
  return launches;
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
