// LDL artifact-map loss ("Details or Artifacts: A Locally Discriminative Learning Approach", CVPR 2022; BasicSR's ldl_opt /
// get_refined_artifact_map), gfx950.  Definition: include/dsr_hip.h; float64 statement: tests/ldl_ref.py.
//
//   r = sum_c |gt - x|, re = sum_c |gt - e|;  mu, v = mean / unbiased variance of r over the k x k window of the reflect-padded
//   plane;  V_n = unbiased variance of r[n] over the image, g_n = V_n^(1/5);  m = (r < re) ? 0 : 1;  w = g_n v m
//   loss = (1 / M) sum_n g_n S_n,  S_n = sum m r v
//
// Launch plan: two launches forward, one backward.
//   1. ldl_tile_kernel<K>   one 16 x 64 tile of one image per block.  r of the tile and its reflected halo of p goes to LDS; each
//                           thread owns four pixels and forms mu and v from the k x k LDS window in TWO passes (mean shifted by
//                           the centre pixel, then the squared deviations from that mean) -- never sum r^2 - (sum r)^2 / K.  It
//                           writes the planes r, m r, mu, m v and three double partials per block: sum (r - r0), sum (r - r0)^2
//                           (r0 = r[n, 0, 0], so a constant r gives exact zeros) and sum m r v.
//   2. ldl_finalize_kernel  a wave folds an image's partials in a fixed order (lane-strided, then the butterfly) and forms
//                           rbar_n, V_n, g_n (double, rounded to fp32 once), S_n and the coefficient of the backward's third
//                           term; the four waves of block (0, 0) take the images in turn, write the statistics, and wave 0
//                           adds the N products g_n S_n to the loss.  With a map, block (n, j) also stores chunk j of
//                           w[n] = g_n (m v).
//   3. ldl_bwd_kernel<K>    stages m r and mu of a tile plus halo (zero outside the image) in LDS and gathers, per pixel s,
//                           sum over the preimages u of s under the reflection and the window of u:  (m r)[q] (r[s] - mu[q]),
//                           which is r Adj(m r) - Adj(m r mu) of the definition with the subtraction made before the sum.
// The window passes are direct k x k LDS reads, not separable running sums: a separable sum cannot be shifted by the centre
// pixel, and at 49 reads per pixel the pass is far below the cost of reading the three images.
#include <math.h>

#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define LDL_TH 16
#define LDL_TW 64
#define LDL_PMAX 5
#define LDL_STATS 5                  // doubles per image: rbar, V, g (the fp32 value), the third term's coefficient, g S

static inline int ldl_tiles_y(int H) { return (H + LDL_TH - 1) / LDL_TH; }
static inline int ldl_tiles_x(int W) { return (W + LDL_TW - 1) / LDL_TW; }

static bool ldl_shape_ok(int N, int C, int H, int W, int k) {
  if (N < 1 || C < 1 || H < 1 || W < 1) return false;
  if (k < 3 || k > 2 * LDL_PMAX + 1 || (k & 1) == 0) return false;
  if (H <= k / 2 || W <= k / 2) return false;
  return (long long)N * C * H * W < (1ll << 31);
}

__device__ __forceinline__ double ldl_block_sum(double s, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();                                           // red may still be read from the sum before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// a coordinate of the padded plane -> the image (F.pad(mode='reflect'): the edge is not repeated); coordinates past the pad,
// which only pixels outside the image ask for, are clamped into the image
__device__ __forceinline__ int ldl_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

__device__ __forceinline__ float ldl_residual(const float* __restrict__ a, const float* __restrict__ b, size_t off, size_t plane,
                                              int C) {
  float r = 0.f;
  for (int c = 0; c < C; ++c) r += fabsf(a[off + (size_t)c * plane] - b[off + (size_t)c * plane]);
  return r;
}

template <int K>
__global__ __launch_bounds__(256) void ldl_tile_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                       const float* __restrict__ e, int C, int H, int W, int tiles_x, int tiles_y,
                                                       float* __restrict__ pr, float* __restrict__ pmr, float* __restrict__ pmu,
                                                       float* __restrict__ pmv, double* __restrict__ partial) {
  constexpr int P = K / 2, LW = LDL_TW + 2 * P, LH = LDL_TH + 2 * P;
  __shared__ float tile[LH * LW];
  __shared__ double red[4];
  const int b = blockIdx.x;
  const int tx = b % tiles_x, ty = (b / tiles_x) % tiles_y, n = b / (tiles_x * tiles_y);
  const int x0 = tx * LDL_TW, y0 = ty * LDL_TH;
  const size_t plane = (size_t)H * W;
  const float* xn = x + (size_t)n * C * plane;
  const float* gn = gt + (size_t)n * C * plane;
  const float* en = e + (size_t)n * C * plane;
  for (int i = threadIdx.x; i < LH * LW; i += 256) {
    const int yy = ldl_reflect(y0 - P + i / LW, H), xx = ldl_reflect(x0 - P + i % LW, W);
    tile[i] = ldl_residual(gn, xn, (size_t)yy * W + xx, plane, C);
  }
  const float r0 = ldl_residual(gn, xn, 0, plane, C);          // the image's first pixel: the shift of the per-image sums
  __syncthreads();
  const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
  double t1 = 0.0, t2 = 0.0, ts = 0.0;
#pragma unroll
  for (int j = 0; j < LDL_TH / 4; ++j) {
    const int ly = ly0 + 4 * j;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const float* win = tile + ly * LW + lx;
    const float rq = win[P * LW + P];
    float s1 = 0.f;
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
      for (int dx = 0; dx < K; ++dx) s1 += win[dy * LW + dx] - rq;
    const float mu = rq + s1 / (float)(K * K);
    float s2 = 0.f;
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
      for (int dx = 0; dx < K; ++dx) {
        const float d = win[dy * LW + dx] - mu;
        s2 = fmaf(d, d, s2);
      }
    const float v = s2 / (float)(K * K - 1);
    const size_t off = (size_t)gy * W + gx;
    const float re = ldl_residual(gn, en, off, plane, C);
    const bool drop = rq < re;                                 // false for a NaN: it stays in the loss
    const float mr = drop ? 0.f : rq, mv = drop ? 0.f : v;
    const size_t o = (size_t)n * plane + off;
    pr[o] = rq;
    pmr[o] = mr;
    pmu[o] = mu;
    pmv[o] = mv;
    const double d0 = (double)rq - (double)r0;
    t1 += d0;
    t2 += d0 * d0;
    ts += (double)mr * (double)mv;
  }
  t1 = ldl_block_sum(t1, red);
  t2 = ldl_block_sum(t2, red);
  ts = ldl_block_sum(ts, red);
  if (threadIdx.x == 0) {
    partial[3 * (size_t)b + 0] = t1;
    partial[3 * (size_t)b + 1] = t2;
    partial[3 * (size_t)b + 2] = ts;
  }
}

struct LdlStats {
  double rbar, V, g, S, c3;
};

// every lane of the wave returns the same bits: lane-strided sums over the image's tiles, then the wave butterfly.  No LDS and
// no barrier, so the waves of a block can take an image each
__device__ __forceinline__ LdlStats ldl_image_stats(const float* __restrict__ x, const float* __restrict__ gt,
                                                    const double* __restrict__ partial, int n, int tiles, int C, int H, int W) {
  const size_t plane = (size_t)H * W;
  double t1 = 0.0, t2 = 0.0, ts = 0.0;
  for (int t = threadIdx.x & 63; t < tiles; t += 64) {
    const double* p = partial + 3 * ((size_t)n * tiles + t);
    t1 += p[0];
    t2 += p[1];
    ts += p[2];
  }
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
  ts = wave_sum(ts);
  const size_t base = (size_t)n * C * plane;
  const double r0 = (double)ldl_residual(gt + base, x + base, 0, plane, C);
  const double hw = (double)plane;
  LdlStats s;
  s.rbar = r0 + t1 / hw;
  const double V = (t2 - t1 * t1 / hw) / (hw - 1.0);
  s.V = V < 0.0 ? 0.0 : V;                                     // (a NaN stays a NaN)
  s.S = ts;
  if (s.V == 0.0) {                                            // r constant: torch's 0 * inf; here the image adds nothing
    s.g = 0.0;
    s.S = 0.0;
    s.c3 = 0.0;
  } else {
    s.g = (double)(float)pow(s.V, 0.2);
    s.c3 = ts * 0.2 * pow(s.V, -0.8) * 2.0 / (hw - 1.0);
  }
  return s;
}

// grid (N, chunks) with a map, (1, 1) without.  Block (0, 0): its four waves take the images in turn (wave w: w, w + 4, ...) and
// write their statistics; after the barrier wave 0 adds the N products g_n S_n lane-strided in image order and folds them by the
// butterfly -- a fixed order.  With a map every wave of block (n, j) forms image n's statistics again (the same adds, the same
// bits) and the block stores chunk j of w[n].
__global__ __launch_bounds__(256) void ldl_finalize_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                           const double* __restrict__ partial, int N, int C, int H, int W,
                                                           int tiles, const float* __restrict__ pmv, double* __restrict__ stats,
                                                           float* __restrict__ loss, float* __restrict__ map) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    for (int n = wave; n < N; n += 4) {
      const LdlStats s = ldl_image_stats(x, gt, partial, n, tiles, C, H, W);
      if (lane == 0) {
        stats[LDL_STATS * n + 0] = s.rbar;
        stats[LDL_STATS * n + 1] = s.V;
        stats[LDL_STATS * n + 2] = s.g;
        stats[LDL_STATS * n + 3] = s.c3;
        stats[LDL_STATS * n + 4] = s.g * s.S;
      }
    }
    __threadfence_block();
    __syncthreads();
    if (wave == 0) {
      double total = 0.0;
      for (int n = lane; n < N; n += 64) total += stats[LDL_STATS * n + 4];
      total = wave_sum(total);
      if (lane == 0) loss[0] = (float)(total / ((double)N * C * H * W));
    }
  }
  if (!map) return;
  const int n = blockIdx.x;
  const LdlStats s = ldl_image_stats(x, gt, partial, n, tiles, C, H, W);
  const float g = (float)s.g;
  const bool flat = s.V == 0.0;
  const size_t plane = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < plane; i += (size_t)gridDim.y * 256)
    map[(size_t)n * plane + i] = flat ? 0.f : g * pmv[(size_t)n * plane + i];
}

// the preimages of image coordinate s under the reflection of a pad of P: s itself (not listed), -s for 1 <= s <= P, and
// 2 (n - 1) - s for n - 1 - P <= s <= n - 2
template <int P>
__device__ __forceinline__ int ldl_preimages(int s, int n, int* u) {
  int c = 0;
  if (s >= 1 && s <= P) u[c++] = -s;
  if (s >= n - 1 - P && s <= n - 2) u[c++] = 2 * (n - 1) - s;
  return c;
}

template <int K>
__global__ __launch_bounds__(256) void ldl_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                      const float* __restrict__ pr, const float* __restrict__ pmr,
                                                      const float* __restrict__ pmu, const float* __restrict__ pmv,
                                                      const double* __restrict__ stats, const float* __restrict__ upstream, int C,
                                                      int H, int W, int tiles_x, int tiles_y, double inv_m, int detach,
                                                      float* __restrict__ dx) {
  constexpr int P = K / 2, LW = LDL_TW + 2 * P, LH = LDL_TH + 2 * P;
  __shared__ float tc[LH * LW];
  __shared__ float tm[LH * LW];
  const int b = blockIdx.x;
  const int tx = b % tiles_x, ty = (b / tiles_x) % tiles_y, n = b / (tiles_x * tiles_y);
  const int x0 = tx * LDL_TW, y0 = ty * LDL_TH;
  const size_t plane = (size_t)H * W;
  if (!detach) {
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
      const int yy = y0 - P + i / LW, xx = x0 - P + i % LW;
      const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
      const size_t o = (size_t)n * plane + (in ? (size_t)yy * W + xx : 0);
      tc[i] = in ? pmr[o] : 0.f;
      tm[i] = in ? pmu[o] : 0.f;
    }
    __syncthreads();
  }
  const double rbar = stats[LDL_STATS * n + 0], V = stats[LDL_STATS * n + 1], c3 = stats[LDL_STATS * n + 3];
  const float g = (float)stats[LDL_STATS * n + 2];
  const float scale = (float)((double)upstream[0] * inv_m);
  const bool flat = V == 0.0;
  const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
  const float* xn = x + (size_t)n * C * plane;
  const float* gn = gt + (size_t)n * C * plane;
  float* dn = dx + (size_t)n * C * plane;
#pragma unroll
  for (int j = 0; j < LDL_TH / 4; ++j) {
    const int ly = ly0 + 4 * j;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const size_t off = (size_t)gy * W + gx;
    float dr = 0.f;
    if (!flat) {
      const float w = g * pmv[(size_t)n * plane + off];
      float sum = w;
      if (!detach) {
        const float rs = pr[(size_t)n * plane + off];
        float acc = 0.f;
        {                                                     // u = s: the whole window, zeros outside the image
          const float* wc = tc + ly * LW + lx;
          const float* wm = tm + ly * LW + lx;
#pragma unroll
          for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dxx = 0; dxx < K; ++dxx) acc = fmaf(wc[dy * LW + dxx], rs - wm[dy * LW + dxx], acc);
        }
        int uy[3], ux[3];
        uy[0] = gy;
        ux[0] = gx;
        const int ny = 1 + ldl_preimages<P>(gy, H, uy + 1), nx = 1 + ldl_preimages<P>(gx, W, ux + 1);
        if (ny + nx > 2) {                                     // a pixel that the pad reflects: the windows of its other preimages
          for (int a = 0; a < ny; ++a)
            for (int c = 0; c < nx; ++c) {
              if (a == 0 && c == 0) continue;
              const int ylo = max(uy[a] - P, 0), yhi = min(uy[a] + P, H - 1);
              const int xlo = max(ux[c] - P, 0), xhi = min(ux[c] + P, W - 1);
              for (int yy = ylo; yy <= yhi; ++yy)
                for (int xx = xlo; xx <= xhi; ++xx) {
                  const int i = (yy - (y0 - P)) * LW + (xx - (x0 - P));
                  acc = fmaf(tc[i], rs - tm[i], acc);
                }
            }
        }
        const float t3 = (float)(c3 * ((double)rs - rbar));
        sum = w + (2.f / (float)(K * K - 1)) * g * acc + t3;
      }
      dr = sum * scale;
    }
    for (int c = 0; c < C; ++c) {
      const float d = xn[off + (size_t)c * plane] - gn[off + (size_t)c * plane];
      const float sg = (float)(d > 0.f) - (float)(d < 0.f);
      dn[off + (size_t)c * plane] = flat ? 0.f : sg * dr;
    }
  }
}

struct LdlWs {
  float *r, *mr, *mu, *mv;
  double *partial, *stats;
};
static LdlWs ldl_carve(void* ws, int N, int H, int W) {
  const size_t px = (size_t)N * H * W;
  const size_t blocks = (size_t)N * ldl_tiles_y(H) * ldl_tiles_x(W);
  LdlWs w;
  w.partial = (double*)ws;                                     // the doubles first: ws is 8-byte aligned
  w.stats = w.partial + 3 * blocks;
  w.r = (float*)(w.stats + (size_t)LDL_STATS * N);
  w.mr = w.r + px;
  w.mu = w.mr + px;
  w.mv = w.mu + px;
  return w;
}

extern "C" size_t dsr_ldl_workspace(int N, int C, int H, int W, int k) {
  if (!ldl_shape_ok(N, C, H, W, k)) return 0;
  const size_t px = (size_t)N * H * W;
  const size_t blocks = (size_t)N * ldl_tiles_y(H) * ldl_tiles_x(W);
  const size_t bytes = sizeof(double) * (3 * blocks + (size_t)LDL_STATS * N) + sizeof(float) * 4 * px;
  return (bytes + 7) & ~(size_t)7;
}

#define LDL_DISPATCH(k, CALL)        \
  switch (k) {                       \
    case 3: CALL(3); break;          \
    case 5: CALL(5); break;          \
    case 7: CALL(7); break;          \
    case 9: CALL(9); break;          \
    default: CALL(11); break;        \
  }

extern "C" int dsr_ldl_fwd(const float* x, const float* gt, const float* e, int N, int C, int H, int W, int k, void* ws,
                           float* loss, float* map, hipStream_t st) {
  DSR_REQUIRE(x && gt && e && ws && loss, "ldl_fwd: null pointer");
  DSR_REQUIRE(k >= 3 && k <= 2 * LDL_PMAX + 1 && (k & 1), "ldl_fwd: window %d (odd, 3 .. %d)", k, 2 * LDL_PMAX + 1);
  DSR_REQUIRE(N >= 1 && C >= 1 && H > k / 2 && W > k / 2, "ldl_fwd: %d x %d x %d x %d under a window of %d (H, W > %d)", N, C, H, W,
              k, k / 2);
  DSR_REQUIRE(ldl_shape_ok(N, C, H, W, k), "ldl_fwd: %d x %d x %d x %d is 2^31 elements or more", N, C, H, W);
  DSR_REQUIRE((((uintptr_t)x | (uintptr_t)gt | (uintptr_t)e | (uintptr_t)loss | (uintptr_t)map) & 3) == 0 && ((uintptr_t)ws & 7) == 0,
              "ldl_fwd: misaligned pointer");
  const int tiles_x = ldl_tiles_x(W), tiles_y = ldl_tiles_y(H), tiles = tiles_x * tiles_y;
  const LdlWs w = ldl_carve(ws, N, H, W);
#define LDL_FWD(KK)                                                                                                          \
  hipLaunchKernelGGL(ldl_tile_kernel<KK>, dim3(N * tiles), dim3(256), 0, st, x, gt, e, C, H, W, tiles_x, tiles_y, w.r, w.mr, \
                     w.mu, w.mv, w.partial)
  LDL_DISPATCH(k, LDL_FWD);
#undef LDL_FWD
  const int rc = dsr_launch_status("dsr_ldl_fwd");
  if (rc) return rc;
  const long long chunks = ((long long)H * W + 256 * 8 - 1) / (256 * 8);
  const dim3 grid = map ? dim3(N, (unsigned)(chunks < 1024 ? chunks : 1024)) : dim3(1, 1);
  hipLaunchKernelGGL(ldl_finalize_kernel, grid, dim3(256), 0, st, x, gt, (const double*)w.partial, N, C, H, W, tiles,
                     (const float*)w.mv, w.stats, loss, map);
  return dsr_launch_status("dsr_ldl_fwd");
}

extern "C" int dsr_ldl_bwd(const float* x, const float* gt, const void* ws, const float* upstream, int N, int C, int H, int W,
                           int k, int detach_weight, float* dx, hipStream_t st) {
  DSR_REQUIRE(x && gt && ws && upstream && dx, "ldl_bwd: null pointer");
  DSR_REQUIRE(k >= 3 && k <= 2 * LDL_PMAX + 1 && (k & 1), "ldl_bwd: window %d (odd, 3 .. %d)", k, 2 * LDL_PMAX + 1);
  DSR_REQUIRE(N >= 1 && C >= 1 && H > k / 2 && W > k / 2, "ldl_bwd: %d x %d x %d x %d under a window of %d (H, W > %d)", N, C, H, W,
              k, k / 2);
  DSR_REQUIRE(ldl_shape_ok(N, C, H, W, k), "ldl_bwd: %d x %d x %d x %d is 2^31 elements or more", N, C, H, W);
  DSR_REQUIRE((((uintptr_t)x | (uintptr_t)gt | (uintptr_t)upstream | (uintptr_t)dx) & 3) == 0 && ((uintptr_t)ws & 7) == 0,
              "ldl_bwd: misaligned pointer");
  const int tiles_x = ldl_tiles_x(W), tiles_y = ldl_tiles_y(H), tiles = tiles_x * tiles_y;
  const LdlWs w = ldl_carve(const_cast<void*>(ws), N, H, W);
  const double inv_m = 1.0 / ((double)N * C * H * W);
#define LDL_BWD(KK)                                                                                                             \
  hipLaunchKernelGGL(ldl_bwd_kernel<KK>, dim3(N * tiles), dim3(256), 0, st, x, gt, (const float*)w.r, (const float*)w.mr,        \
                     (const float*)w.mu, (const float*)w.mv, (const double*)w.stats, upstream, C, H, W, tiles_x, tiles_y, inv_m, \
                     detach_weight ? 1 : 0, dx)
  LDL_DISPATCH(k, LDL_BWD);
#undef LDL_BWD
  return dsr_launch_status("dsr_ldl_bwd");
}
