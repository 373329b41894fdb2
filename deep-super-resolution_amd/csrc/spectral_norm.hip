// Spectral normalisation of up to 64 weight matrices per call (gfx950): torch.nn.utils.spectral_norm with one power
// iteration, and its backward.
//
//   W [Cout][K] row-major fp32 (a conv weight viewed as Cout x Cin KH KW), u [Cout], v [K]
//   train:  t = W^T u;  v = t / max(|t|, eps);  s = W v;  u = s / max(|s|, eps);  sigma = u . s;  W_sn = W / sigma
//   eval:   s = W v;  sigma = u . s;  W_sn = W / sigma                        (u and v are only read)
//   bwd:    dW = (G - <G, W_sn> u v^T) / sigma                                 (u, v: constants, as torch detaches them)
//
// The phases depend on each other across the whole matrix, so each is a launch of its own -- no cooperative launch, no
// flag another block waits for, no atomics.  All layers of a call share every launch through multi_tensor.h's block table:
//   1. sn_wtu_kernel    partial[chunk][k] = sum over SN_ROWS rows of W[r][k] u[r]         (train only)
//   2. sn_v_kernel      t[k] = sum of the partials over chunks; v = t / max(|t|, eps)       (train only; one block per layer)
//   3. sn_wv_kernel     s[r] = W[r] . v, one wave per row
//   4. sn_apply_kernel  every block derives the layer's sigma from s (Cout values, the same arithmetic in every block, hence
//                       the same bits); the layer's first block also writes u and sigma; W_sn = W / sigma on its chunk
// and the backward is sn_bwd_dot_kernel (one partial per chunk of <G, W_sn>) + sn_bwd_apply_kernel (every block folds its
// layer's partials, then its chunk).  A training forward therefore reads W three times and writes W_sn once.
// Every sum has a fixed shape: a thread adds its strided elements in index order, a wave folds by the xor butterfly (the same
// value on every lane), a block adds its waves' values in wave order; partials are folded in chunk order.  Two runs from the
// same state give the same bits.
// Rows are read as 16-byte vectors when K % 4 == 0 and every pointer of the layer is 16-byte aligned (then every row start
// is); otherwise that layer runs on 4-byte accesses (decided per layer).
#include <math.h>

#include "dsr_common.h"
#include "dsr_kernels.h"
#include "multi_tensor.h"
#include "../../include/dsr_hip.h"

#define SN_ROWS 32       // rows of W behind one W^T u partial
#define SN_COLS 256      // scalar path: columns per block of sn_wtu_kernel (the vector path takes 4 per thread: 1024)
#define SN_CHUNK 4096    // elements of W per block of the streaming kernels
#define SN_THREADS 256
#define SN_VTHREADS 1024  // sn_v_kernel: one block per layer

typedef __attribute__((ext_vector_type(4))) float F4;

struct SnFwd {
  const float* w[DSR_MT_MAX];
  float* u[DSR_MT_MAX];
  float* v[DSR_MT_MAX];
  float* out[DSR_MT_MAX];
  int cout[DSR_MT_MAX];
  int k[DSR_MT_MAX];
  unsigned off[DSR_MT_MAX];          // floats into the workspace: s [round_up(Cout, 4)], then (train) the partials [chunks][K]
  unsigned char vec[DSR_MT_MAX];
};
struct SnBwd {
  const float* g[DSR_MT_MAX];
  const float* wsn[DSR_MT_MAX];
  const float* u[DSR_MT_MAX];
  const float* v[DSR_MT_MAX];
  float* dw[DSR_MT_MAX];
  int cout[DSR_MT_MAX];
  int k[DSR_MT_MAX];
  unsigned off[DSR_MT_MAX];          // floats into the workspace: one partial per chunk
  unsigned char vec[DSR_MT_MAX];
};
static_assert(sizeof(SnFwd) + sizeof(MtTable) + 64 <= 4096, "kernel arguments are limited to 4 KB");
static_assert(sizeof(SnBwd) + sizeof(MtTable) + 64 <= 4096, "kernel arguments are limited to 4 KB");

// the sum of v over the block, the same bits on every thread; `red` holds one float per wave and may be reused at once
__device__ __forceinline__ float sn_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
  for (unsigned w = 1; w < (blockDim.x >> 6); ++w) t += red[w];
  return t;
}

__global__ __launch_bounds__(SN_THREADS) void sn_wtu_kernel(const SnFwd g, const MtTable tb, float* __restrict__ ws) {
  unsigned blk;
  const int t = mt_locate(tb, blk);
  const int K = g.k[t], C = g.cout[t];
  const float* __restrict__ w = g.w[t];
  const float* __restrict__ u = g.u[t];
  float* __restrict__ part = ws + g.off[t] + ((C + 3) & ~3);
  const bool vec = g.vec[t];
  const unsigned tiles = vec ? (K + 4 * SN_COLS - 1) / (4 * SN_COLS) : (K + SN_COLS - 1) / SN_COLS;
  const unsigned chunk = blk / tiles, tile = blk % tiles;
  const int r0 = chunk * SN_ROWS, r1 = r0 + SN_ROWS < C ? r0 + SN_ROWS : C;
  if (vec) {
    const int col = (tile * SN_COLS + threadIdx.x) * 4;
    if (col >= K) return;
    F4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; ++r) {
      const F4 x = *reinterpret_cast<const F4*>(w + (size_t)r * K + col);
      const float ur = u[r];
      acc.x = fmaf(x.x, ur, acc.x);
      acc.y = fmaf(x.y, ur, acc.y);
      acc.z = fmaf(x.z, ur, acc.z);
      acc.w = fmaf(x.w, ur, acc.w);
    }
    *reinterpret_cast<F4*>(part + (size_t)chunk * K + col) = acc;      // (off, Cout and K are multiples of 4 here)
  } else {
    const int col = tile * SN_COLS + threadIdx.x;
    if (col >= K) return;
    float acc = 0.f;
    for (int r = r0; r < r1; ++r) acc = fmaf(w[(size_t)r * K + col], u[r], acc);
    part[(size_t)chunk * K + col] = acc;
  }
}

__global__ __launch_bounds__(SN_VTHREADS) void sn_v_kernel(const SnFwd g, const float* __restrict__ ws, float eps) {
  // one block per layer: a thread folds the partials of its columns in chunk order (independent loads, one chain of adds per
  // column), the block forms |t|, each thread normalises the columns it folded
  __shared__ float red[SN_VTHREADS / 64];
  const int t = blockIdx.x;
  const int K = g.k[t], C = g.cout[t];
  const float* __restrict__ part = ws + g.off[t] + ((C + 3) & ~3);
  float* __restrict__ v = g.v[t];
  const int chunks = (C + SN_ROWS - 1) / SN_ROWS;
  float ss = 0.f;
  if (g.vec[t]) {
    for (int k = threadIdx.x * 4; k < K; k += SN_VTHREADS * 4) {
      F4 tk = *reinterpret_cast<const F4*>(part + k);
#pragma unroll 8
      for (int c = 1; c < chunks; ++c) {
        const F4 x = *reinterpret_cast<const F4*>(part + (size_t)c * K + k);
        tk.x += x.x;
        tk.y += x.y;
        tk.z += x.z;
        tk.w += x.w;
      }
      *reinterpret_cast<F4*>(v + k) = tk;
      ss = fmaf(tk.x, tk.x, ss);
      ss = fmaf(tk.y, tk.y, ss);
      ss = fmaf(tk.z, tk.z, ss);
      ss = fmaf(tk.w, tk.w, ss);
    }
  } else {
    for (int k = threadIdx.x; k < K; k += SN_VTHREADS) {
      float tk = part[k];
#pragma unroll 8
      for (int c = 1; c < chunks; ++c) tk += part[(size_t)c * K + k];
      v[k] = tk;
      ss = fmaf(tk, tk, ss);
    }
  }
  const float d = fmaxf(sqrtf(sn_block_sum(ss, red)), eps);
  // (each thread re-reads what it wrote itself)
  if (g.vec[t]) {
    for (int k = threadIdx.x * 4; k < K; k += SN_VTHREADS * 4) {
      F4 x = *reinterpret_cast<const F4*>(v + k);
      x.x = x.x / d;
      x.y = x.y / d;
      x.z = x.z / d;
      x.w = x.w / d;
      *reinterpret_cast<F4*>(v + k) = x;
    }
  } else {
    for (int k = threadIdx.x; k < K; k += SN_VTHREADS) v[k] = v[k] / d;
  }
}

__global__ __launch_bounds__(SN_THREADS) void sn_wv_kernel(const SnFwd g, const MtTable tb, float* __restrict__ ws) {
  unsigned blk;
  const int t = mt_locate(tb, blk);
  const int K = g.k[t], C = g.cout[t];
  const int row = blk * (SN_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= C) return;
  const int lane = threadIdx.x & 63;
  const float* __restrict__ w = g.w[t] + (size_t)row * K;
  const float* __restrict__ v = g.v[t];
  float acc = 0.f;
  if (g.vec[t]) {
    for (int j = lane; j < K / 4; j += 64) {
      const F4 x = reinterpret_cast<const F4*>(w)[j], y = reinterpret_cast<const F4*>(v)[j];
      acc = fmaf(x.x, y.x, acc);
      acc = fmaf(x.y, y.y, acc);
      acc = fmaf(x.z, y.z, acc);
      acc = fmaf(x.w, y.w, acc);
    }
  } else {
    for (int j = lane; j < K; j += 64) acc = fmaf(w[j], v[j], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) ws[g.off[t] + row] = acc;
}

__global__ __launch_bounds__(SN_THREADS) void sn_apply_kernel(const SnFwd g, const MtTable tb, const float* __restrict__ ws,
                                                              int training, float eps, float* __restrict__ sigma_out) {
  __shared__ float red[SN_THREADS / 64];
  unsigned blk;
  const int t = mt_locate(tb, blk);
  const int K = g.k[t], C = g.cout[t];
  const float* __restrict__ s = ws + g.off[t];
  float* __restrict__ u = g.u[t];
  float sigma;
  if (training) {
    float ss = 0.f;
    for (int c = threadIdx.x; c < C; c += SN_THREADS) ss = fmaf(s[c], s[c], ss);
    const float d = fmaxf(sqrtf(sn_block_sum(ss, red)), eps);
    float dot = 0.f;
    for (int c = threadIdx.x; c < C; c += SN_THREADS) {
      const float uc = s[c] / d;
      dot = fmaf(uc, s[c], dot);
      if (blk == 0) u[c] = uc;
    }
    sigma = sn_block_sum(dot, red);
  } else {
    float dot = 0.f;
    for (int c = threadIdx.x; c < C; c += SN_THREADS) dot = fmaf(u[c], s[c], dot);
    sigma = sn_block_sum(dot, red);
  }
  if (blk == 0 && threadIdx.x == 0) sigma_out[t] = sigma;
  const size_t n = (size_t)C * K;
  const size_t e0 = (size_t)blk * SN_CHUNK, e1 = e0 + SN_CHUNK < n ? e0 + SN_CHUNK : n;
  const float* __restrict__ w = g.w[t];
  float* __restrict__ out = g.out[t];
  if (g.vec[t]) {                                   // (n is a multiple of 4)
    for (size_t i = e0 / 4 + threadIdx.x; i < e1 / 4; i += SN_THREADS) {
      const F4 x = reinterpret_cast<const F4*>(w)[i];
      F4 y;
      y.x = x.x / sigma;
      y.y = x.y / sigma;
      y.z = x.z / sigma;
      y.w = x.w / sigma;
      reinterpret_cast<F4*>(out)[i] = y;
    }
  } else {
    for (size_t i = e0 + threadIdx.x; i < e1; i += SN_THREADS) out[i] = w[i] / sigma;
  }
}

__global__ __launch_bounds__(SN_THREADS) void sn_bwd_dot_kernel(const SnBwd g, const MtTable tb, float* __restrict__ ws) {
  __shared__ float red[SN_THREADS / 64];
  unsigned blk;
  const int t = mt_locate(tb, blk);
  const size_t n = (size_t)g.cout[t] * g.k[t];
  const size_t e0 = (size_t)blk * SN_CHUNK, e1 = e0 + SN_CHUNK < n ? e0 + SN_CHUNK : n;
  const float* __restrict__ a = g.g[t];
  const float* __restrict__ b = g.wsn[t];
  float acc = 0.f;
  if (g.vec[t]) {
    for (size_t i = e0 / 4 + threadIdx.x; i < e1 / 4; i += SN_THREADS) {
      const F4 x = reinterpret_cast<const F4*>(a)[i], y = reinterpret_cast<const F4*>(b)[i];
      acc = fmaf(x.x, y.x, acc);
      acc = fmaf(x.y, y.y, acc);
      acc = fmaf(x.z, y.z, acc);
      acc = fmaf(x.w, y.w, acc);
    }
  } else {
    for (size_t i = e0 + threadIdx.x; i < e1; i += SN_THREADS) acc = fmaf(a[i], b[i], acc);
  }
  acc = sn_block_sum(acc, red);
  if (threadIdx.x == 0) ws[g.off[t] + blk] = acc;
}

__global__ __launch_bounds__(SN_THREADS) void sn_bwd_apply_kernel(const SnBwd g, const MtTable tb, const float* __restrict__ ws,
                                                                  const float* __restrict__ sigma_in) {
  __shared__ float red[SN_THREADS / 64];
  unsigned blk;
  const int t = mt_locate(tb, blk);
  const int K = g.k[t];
  const size_t n = (size_t)g.cout[t] * K;
  const unsigned nb = tb.first_block[t + 1] - tb.first_block[t];
  const float* __restrict__ part = ws + g.off[t];
  float acc = 0.f;
  for (unsigned j = threadIdx.x; j < nb; j += SN_THREADS) acc += part[j];
  const float d = sn_block_sum(acc, red);
  const float sigma = sigma_in[t];
  const size_t e0 = (size_t)blk * SN_CHUNK, e1 = e0 + SN_CHUNK < n ? e0 + SN_CHUNK : n;
  const float* __restrict__ a = g.g[t];
  const float* __restrict__ u = g.u[t];
  const float* __restrict__ v = g.v[t];
  float* __restrict__ dw = g.dw[t];
  if (g.vec[t]) {                                   // K % 4 == 0: the four elements share their row
    for (size_t i = e0 / 4 + threadIdx.x; i < e1 / 4; i += SN_THREADS) {
      const size_t e = i * 4;
      const int c = (int)(e / K), k = (int)(e % K);
      const F4 x = reinterpret_cast<const F4*>(a)[i];
      const F4 y = *reinterpret_cast<const F4*>(v + k);
      const float du = d * u[c];
      F4 r;
      r.x = (x.x - du * y.x) / sigma;
      r.y = (x.y - du * y.y) / sigma;
      r.z = (x.z - du * y.z) / sigma;
      r.w = (x.w - du * y.w) / sigma;
      reinterpret_cast<F4*>(dw)[i] = r;
    }
  } else {
    for (size_t i = e0 + threadIdx.x; i < e1; i += SN_THREADS) {
      const int c = (int)(i / K), k = (int)(i % K);
      dw[i] = (a[i] - d * u[c] * v[k]) / sigma;
    }
  }
}

// ---- host side
static inline bool sn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline size_t sn_chunks(int cout, int k) { return mt_blocks((size_t)cout * k, SN_CHUNK); }
static inline size_t sn_r4(size_t x) { return (x + 3) & ~(size_t)3; }
// floats of workspace of one layer (a multiple of 4, so that every layer's slice starts 16-byte aligned)
static inline size_t sn_fwd_floats(int cout, int k) { return sn_r4((size_t)cout) + sn_r4(mt_blocks(cout, SN_ROWS) * (size_t)k); }

static int sn_check_shapes(const char* what, int count, const int* cout, const int* k) {
  if (count < 1 || count > DSR_MT_MAX) return dsr_fail(DSR_E_ARG, "%s: count %d is outside 1..%d", what, count, DSR_MT_MAX);
  if (!cout || !k) return dsr_fail(DSR_E_ARG, "%s: null shape table", what);
  size_t blocks = 0;
  for (int i = 0; i < count; ++i) {
    if (cout[i] < 1 || k[i] < 1) return dsr_fail(DSR_E_ARG, "%s: layer %d is %d x %d", what, i, cout[i], k[i]);
    if ((size_t)cout[i] * k[i] >= ((size_t)1 << 31)) return dsr_fail(DSR_E_ARG, "%s: layer %d has 2^31 elements or more", what, i);
    blocks += sn_chunks(cout[i], k[i]) + mt_blocks(cout[i], SN_ROWS) * mt_blocks(k[i], SN_COLS);
  }
  if (blocks >= ((size_t)1 << 31)) return dsr_fail(DSR_E_ARG, "%s: too many blocks", what);
  return 0;
}

extern "C" size_t dsr_spectral_norm_workspace(int count, const int* cout, const int* k) {
  if (sn_check_shapes("spectral_norm_workspace", count, cout, k)) return 0;
  size_t fl = 0;
  for (int i = 0; i < count; ++i) fl += sn_fwd_floats(cout[i], k[i]);
  return fl * sizeof(float);
}

extern "C" size_t dsr_spectral_norm_bwd_workspace(int count, const int* cout, const int* k) {
  if (sn_check_shapes("spectral_norm_bwd_workspace", count, cout, k)) return 0;
  size_t fl = 0;
  for (int i = 0; i < count; ++i) fl += sn_r4(sn_chunks(cout[i], k[i]));
  return fl * sizeof(float);
}

extern "C" int dsr_spectral_norm_fwd(int count, const float* const* w, float* const* u, float* const* v, const int* cout,
                                     const int* k, int training, float eps, float* sigma, float* const* w_sn, float* ws,
                                     size_t ws_bytes, hipStream_t st) {
  if (int rc = sn_check_shapes("spectral_norm_fwd", count, cout, k)) return rc;
  DSR_REQUIRE(w && u && v && w_sn && sigma && ws, "spectral_norm_fwd: null table, sigma or workspace");
  DSR_REQUIRE(((uintptr_t)sigma & 3) == 0 && ((uintptr_t)ws & 15) == 0, "spectral_norm_fwd: misaligned sigma or workspace");
  DSR_REQUIRE(eps >= 0.f, "spectral_norm_fwd: eps %g is negative", (double)eps);
  DSR_REQUIRE(ws_bytes >= dsr_spectral_norm_workspace(count, cout, k), "spectral_norm_fwd: workspace of %zu bytes is too small",
              ws_bytes);
  SnFwd g;
  MtTable wtu, wv, ap;
  size_t off = 0, b_wtu = 0, b_wv = 0, b_ap = 0;
  for (int i = 0; i < count; ++i) {
    DSR_REQUIRE(w[i] && u[i] && v[i] && w_sn[i], "spectral_norm_fwd: layer %d has a null pointer", i);
    DSR_REQUIRE((((uintptr_t)w[i] | (uintptr_t)u[i] | (uintptr_t)v[i] | (uintptr_t)w_sn[i]) & 3) == 0,
                "spectral_norm_fwd: layer %d is not 4-byte aligned", i);
    DSR_REQUIRE(w[i] != w_sn[i], "spectral_norm_fwd: layer %d would be normalised in place", i);
    g.w[i] = w[i];
    g.u[i] = u[i];
    g.v[i] = v[i];
    g.out[i] = w_sn[i];
    g.cout[i] = cout[i];
    g.k[i] = k[i];
    g.off[i] = (unsigned)off;
    const bool vec = k[i] % 4 == 0 && sn_al16(w[i]) && sn_al16(v[i]) && sn_al16(w_sn[i]);
    g.vec[i] = vec;
    off += sn_fwd_floats(cout[i], k[i]);
    wtu.first_block[i] = (unsigned)b_wtu;
    wv.first_block[i] = (unsigned)b_wv;
    ap.first_block[i] = (unsigned)b_ap;
    b_wtu += mt_blocks(cout[i], SN_ROWS) * mt_blocks(k[i], vec ? 4 * SN_COLS : SN_COLS);
    b_wv += mt_blocks(cout[i], SN_THREADS / 64);
    b_ap += sn_chunks(cout[i], k[i]);
  }
  DSR_REQUIRE(off < ((size_t)1 << 32), "spectral_norm_fwd: the workspace passes 2^32 floats");
  wtu.first_block[count] = (unsigned)b_wtu;
  wv.first_block[count] = (unsigned)b_wv;
  ap.first_block[count] = (unsigned)b_ap;
  wtu.count = wv.count = ap.count = count;
  if (training) {
    hipLaunchKernelGGL(sn_wtu_kernel, dim3((unsigned)b_wtu), dim3(SN_THREADS), 0, st, g, wtu, ws);
    hipLaunchKernelGGL(sn_v_kernel, dim3(count), dim3(SN_VTHREADS), 0, st, g, ws, eps);
  }
  hipLaunchKernelGGL(sn_wv_kernel, dim3((unsigned)b_wv), dim3(SN_THREADS), 0, st, g, wv, ws);
  hipLaunchKernelGGL(sn_apply_kernel, dim3((unsigned)b_ap), dim3(SN_THREADS), 0, st, g, ap, ws, training ? 1 : 0, eps, sigma);
  return dsr_launch_status("dsr_spectral_norm_fwd");
}

extern "C" int dsr_spectral_norm_bwd(int count, const float* const* gr, const float* const* w_sn, const float* const* u,
                                     const float* const* v, const int* cout, const int* k, const float* sigma,
                                     float* const* dw, float* ws, size_t ws_bytes, hipStream_t st) {
  if (int rc = sn_check_shapes("spectral_norm_bwd", count, cout, k)) return rc;
  DSR_REQUIRE(gr && w_sn && u && v && dw && sigma && ws, "spectral_norm_bwd: null table, sigma or workspace");
  DSR_REQUIRE(((uintptr_t)sigma & 3) == 0 && ((uintptr_t)ws & 15) == 0, "spectral_norm_bwd: misaligned sigma or workspace");
  DSR_REQUIRE(ws_bytes >= dsr_spectral_norm_bwd_workspace(count, cout, k),
              "spectral_norm_bwd: workspace of %zu bytes is too small", ws_bytes);
  SnBwd g;
  MtTable tb;
  size_t off = 0, blocks = 0;
  for (int i = 0; i < count; ++i) {
    DSR_REQUIRE(gr[i] && w_sn[i] && u[i] && v[i] && dw[i], "spectral_norm_bwd: layer %d has a null pointer", i);
    DSR_REQUIRE((((uintptr_t)gr[i] | (uintptr_t)w_sn[i] | (uintptr_t)u[i] | (uintptr_t)v[i] | (uintptr_t)dw[i]) & 3) == 0,
                "spectral_norm_bwd: layer %d is not 4-byte aligned", i);
    g.g[i] = gr[i];
    g.wsn[i] = w_sn[i];
    g.u[i] = u[i];
    g.v[i] = v[i];
    g.dw[i] = dw[i];
    g.cout[i] = cout[i];
    g.k[i] = k[i];
    g.off[i] = (unsigned)off;
    g.vec[i] = k[i] % 4 == 0 && sn_al16(gr[i]) && sn_al16(w_sn[i]) && sn_al16(v[i]) && sn_al16(dw[i]);
    tb.first_block[i] = (unsigned)blocks;
    off += sn_r4(sn_chunks(cout[i], k[i]));
    blocks += sn_chunks(cout[i], k[i]);
  }
  tb.first_block[count] = (unsigned)blocks;
  tb.count = count;
  hipLaunchKernelGGL(sn_bwd_dot_kernel, dim3((unsigned)blocks), dim3(SN_THREADS), 0, st, g, tb, ws);
  hipLaunchKernelGGL(sn_bwd_apply_kernel, dim3((unsigned)blocks), dim3(SN_THREADS), 0, st, g, tb, ws, sigma);
  return dsr_launch_status("dsr_spectral_norm_bwd");
}
