// NIQE, the no-reference quality score of Mittal, Soundararajan and Bovik 2013 as BasicSR's calculate_niqe computes it
// (metrics.NaturalnessImageQualityEvaluator, metrics.niqe_features).  PARITY UNPINNED: BasicSR, OpenCV and its parameter file
// are not at hand; the float64 statement of the definition is tests/niqe_ref.py.  Three launches of this file and one of
// imresize.hip give the [blocks][36] feature table of a batch:
//   dsr_niqe_plane     the rounded 8-bit BT.601 luma, shaved and cropped to whole 96 x 96 blocks, as fp32 integers;
//   dsr_niqe_moments   per block the MSCN image v = (x - mu) / (sigma + 1) under a 7 x 7 window with replicated borders, and
//                      of v and its four products with a neighbour rolled INSIDE the block the five sums the fit needs;
//   dsr_niqe_features  the asymmetric generalised Gaussian fit of each of those maps from the sums and three Gamma tables.
//
// From the fp32 plane onward everything is fp64: w * x^2 - mu^2 cancels (x^2 reaches 55 225) and an fp32 window sum would
// leave 1e-3 in the variance, enough to move alpha across grid steps.  mu and w * x^2 are formed with a separately rounded
// multiply and add per tap (contraction off), in row-major order of the window as given: the sign of v on a flat
// neighbourhood is rounding residue (BasicSR has the same problem), and this way it is the yardstick's residue, bit for bit.
// Sums run in a fixed order without atomics: two runs give equal bits.
#include "dsr_common.h"
#include "dsr_kernels.h"
#include "../../include/dsr_hip.h"

#define NIQE_BLOCK 96            // the block of scale 1; scale 2 runs on the half-size plane with 48
#define NIQE_GRID 9801           // arange(0.2, 10.001, 0.001)
#define NIQE_FEATS 36

template <int D>
__device__ __forceinline__ int niqe_code(const void* __restrict__ p, size_t i) {
  float x;
  if constexpr (D == DSR_F32) {
    x = reinterpret_cast<const float*>(p)[i];
  } else {
    x = h2f<D>(reinterpret_cast<const unsigned short*>(p)[i]);
  }
  return (int)rintf(fminf(fmaxf(x, 0.f), 1.f) * 255.0f);
}

// plane[n][y][x] = 16 + round_half_even((65481 r + 128553 g + 24966 b) / 255000) of the 8-bit codes at (y + s, x + s)
template <int D>
__global__ __launch_bounds__(256) void niqe_plane_kernel(const void* __restrict__ x, int H, int W, int s, int hc, int wc,
                                                         unsigned total, float* __restrict__ plane) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned per = (unsigned)hc * (unsigned)wc;
  const unsigned n = i / per, r = i - n * per;
  const unsigned y = r / (unsigned)wc, c = r - y * (unsigned)wc;
  const size_t hw = (size_t)H * W;
  const size_t o = (size_t)n * 3 * hw + (size_t)(y + s) * W + (c + s);
  const int t = 65481 * niqe_code<D>(x, o) + 128553 * niqe_code<D>(x, o + hw) + 24966 * niqe_code<D>(x, o + 2 * hw);
  int q = t / 255000;
  const int rem = t - q * 255000;
  if (rem > 127500 || (rem == 127500 && (q & 1))) ++q;
  plane[i] = (float)(16 + q);
}

// One workgroup per block of B x B pixels.  LDS: v [B][B] fp64, the plane's tile with a 3-pixel halo [B + 6][B + 6] fp32, the
// waves' partial sums and the window -- 118 KB at B = 96 (the opt-in), 31 KB at B = 48.
template <int B, int T>
__global__ __launch_bounds__(T) void niqe_moments_kernel(const float* __restrict__ plane, int hc, int wc, int nby, int nbx,
                                                         const double* __restrict__ window, double* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int TW = B + 6;
  extern __shared__ __attribute__((aligned(16))) char niqe_smem[];
  double* v = reinterpret_cast<double*>(niqe_smem);
  float* xt = reinterpret_cast<float*>(niqe_smem + (size_t)B * B * 8);
  double* red = reinterpret_cast<double*>(niqe_smem + (size_t)B * B * 8 + (size_t)TW * TW * 4);
  double* win = red + (T / 64) * 25;
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby, n = blockIdx.x / (nbx * nby);
  const float* img = plane + (size_t)n * hc * wc;
  for (int i = tid; i < TW * TW; i += T) {
    const int ty = i / TW, tx = i - ty * TW;
    const int gy = min(max(by * B - 3 + ty, 0), hc - 1), gx = min(max(bx * B - 3 + tx, 0), wc - 1);
    xt[i] = img[(size_t)gy * wc + gx];
  }
  if (tid < 49) win[tid] = window[tid];
  __syncthreads();
  for (int i = tid; i < B * B; i += T) {
    const int r = i / B, c = i - r * B;
    double mu = 0.0, ex2 = 0.0;
    for (int a = 0; a < 7; ++a) {
#pragma unroll
      for (int b = 0; b < 7; ++b) {     // a convolution: window element (a, b) meets the pixel at (r + 3 - a, c + 3 - b)
        const double x = (double)xt[(r + 6 - a) * TW + (c + 6 - b)];
        const double w = win[a * 7 + b];
        mu = mu + w * x;
        ex2 = ex2 + w * (x * x);
      }
    }
    const double x0 = (double)xt[(r + 3) * TW + (c + 3)];
    v[i] = (x0 - mu) / (sqrt(fabs(ex2 - mu * mu)) + 1.0);
  }
  __syncthreads();
  double acc[5][5];
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[k][j] = 0.0;
  for (int i = tid; i < B * B; i += T) {
    const int r = i / B, c = i - r * B;
    const int rm = r == 0 ? B - 1 : r - 1, cm = c == 0 ? B - 1 : c - 1, cp = c == B - 1 ? 0 : c + 1;
    const double v0 = v[i];
    double m[5];
    m[0] = v0;
    m[1] = v0 * v[r * B + cm];          // roll (0, 1)
    m[2] = v0 * v[rm * B + c];          // roll (1, 0)
    m[3] = v0 * v[rm * B + cm];         // roll (1, 1)
    m[4] = v0 * v[rm * B + cp];         // roll (1, -1)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double sq = m[k] * m[k];
      const bool neg = m[k] < 0.0, pos = m[k] > 0.0;
      acc[k][0] += neg ? 1.0 : 0.0;
      acc[k][1] += pos ? 1.0 : 0.0;
      acc[k][2] += neg ? sq : 0.0;
      acc[k][3] += pos ? sq : 0.0;
      acc[k][4] += fabs(m[k]);
    }
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const double s = wave_sum(acc[k][j]);
      if (lane == 0) red[wave * 25 + k * 5 + j] = s;
    }
  __syncthreads();
  if (tid < 25) {
    double s = 0.0;
    for (int w = 0; w < T / 64; ++w) s += red[w * 25 + tid];
    out[(size_t)blockIdx.x * 25 + tid] = s;
  }
}

template <int B, int T>
constexpr int niqe_moments_lds() {
  return B * B * 8 + (B + 6) * (B + 6) * 4 + ((T / 64) * 25 + 49) * 8;
}

// One thread per (image, block, scale, map): the AGGD fit from the map's five sums.  tables: [0] r(alpha) =
// Gamma(2/alpha)^2 / (Gamma(1/alpha) Gamma(3/alpha)), strictly increasing over the grid; [1] sqrt(Gamma(1/alpha) /
// Gamma(3/alpha)); [2] Gamma(2/alpha) / Gamma(1/alpha).  np.argmin((r - rn)^2) = the nearer of the two grid points around rn,
// the lower one on a tie; a rn that is not finite gives index 0 like argmin of an all-NaN row.
__global__ __launch_bounds__(256) void niqe_features_kernel(const double* __restrict__ m1, const double* __restrict__ m2,
                                                            unsigned total, const double* __restrict__ tables,
                                                            double* __restrict__ feat) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned row = i / 10u, j = i - row * 10u;
  const unsigned scale = j / 5u, k = j - scale * 5u;
  const double* m = (scale ? m2 : m1) + (size_t)row * 25 + k * 5;
  const double b2 = scale ? (double)(NIQE_BLOCK / 2 * (NIQE_BLOCK / 2)) : (double)(NIQE_BLOCK * NIQE_BLOCK);
  const double nneg = m[0], npos = m[1], sneg = m[2], spos = m[3], sabs = m[4];
  const double ls = sqrt(sneg / nneg), rs = sqrt(spos / npos);
  const double gh = ls / rs;
  const double ma = sabs / b2;
  const double rhat = ma * ma / ((sneg + spos) / b2);
  const double g2 = gh * gh + 1.0;
  const double rn = rhat * (gh * gh * gh + 1.0) * (gh + 1.0) / (g2 * g2);
  int idx = 0;
  if (isfinite(rn)) {
    int lo = 0, hi = NIQE_GRID;                       // the first index whose r is >= rn
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tables[mid] < rn) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) {
      idx = 0;
    } else if (lo == NIQE_GRID) {
      idx = NIQE_GRID - 1;
    } else {
      const double dl = tables[lo - 1] - rn, dh = tables[lo] - rn;
      idx = dl * dl <= dh * dh ? lo - 1 : lo;
    }
  }
  const double alpha = 0.2 + 0.001 * (double)idx;
  const double bscale = tables[NIQE_GRID + idx];
  const double bl = ls * bscale, br = rs * bscale;
  double* f = feat + (size_t)row * NIQE_FEATS + scale * 18;
  if (k == 0) {
    f[0] = alpha;
    f[1] = (bl + br) / 2.0;
  } else {
    f += 2 + (k - 1) * 4;
    f[0] = alpha;
    f[1] = (br - bl) * tables[2 * NIQE_GRID + idx];
    f[2] = bl;
    f[3] = br;
  }
}

// ---- host side
static bool niqe_dtype_ok(int dt) { return dt == DSR_BF16 || dt == DSR_F16 || dt == DSR_F32; }

extern "C" int dsr_niqe_plane(int dtype, const void* x, int N, int C, int H, int W, int shave, float* plane, dsr_stream_t st) {
  DSR_REQUIRE(x && plane, "niqe_plane: null pointer");
  DSR_REQUIRE(niqe_dtype_ok(dtype), "niqe_plane: dtype %d (0 bf16, 1 f16, 2 f32)", dtype);
  DSR_REQUIRE(N >= 1, "niqe_plane: %d images", N);
  DSR_REQUIRE(C == 3, "niqe_plane: %d channels, RGB needs 3", C);
  DSR_REQUIRE(H >= 1 && W >= 1, "niqe_plane: image %dx%d", H, W);
  DSR_REQUIRE(shave >= 0, "niqe_plane: shave %d is negative", shave);
  const long long h = (long long)H - 2ll * shave, w = (long long)W - 2ll * shave;
  const long long nby = h > 0 ? h / NIQE_BLOCK : 0, nbx = w > 0 ? w / NIQE_BLOCK : 0;
  DSR_REQUIRE(nby * nbx >= 2, "niqe_plane: shave %d leaves %lldx%lld of a %dx%d image, fewer than two 96x96 blocks", shave,
              h > 0 ? h : 0, w > 0 ? w : 0, H, W);
  const long long hc = nby * NIQE_BLOCK, wc = nbx * NIQE_BLOCK;
  DSR_REQUIRE((long long)N * hc * wc < (1ll << 31), "niqe_plane: more than 2^31 pixels");
  const unsigned total = (unsigned)((long long)N * hc * wc);
  const unsigned blocks = (total + 255u) / 256u;
#define NIQE_GO(D) \
  hipLaunchKernelGGL((niqe_plane_kernel<D>), dim3(blocks), dim3(256), 0, st, x, H, W, shave, (int)hc, (int)wc, total, plane)
  if (dtype == DSR_F32)
    NIQE_GO(DSR_F32);
  else if (dtype == DSR_F16)
    NIQE_GO(DSR_F16);
  else
    NIQE_GO(DSR_BF16);
#undef NIQE_GO
  return dsr_launch_status("dsr_niqe_plane");
}

extern "C" int dsr_niqe_moments(const float* plane, int N, int hc, int wc, int block, const double* window, double* out,
                                dsr_stream_t st) {
  DSR_REQUIRE(plane && window && out, "niqe_moments: null pointer");
  DSR_REQUIRE(block == NIQE_BLOCK || block == NIQE_BLOCK / 2, "niqe_moments: block %d, 96 (scale 1) or 48 (scale 2)", block);
  DSR_REQUIRE(N >= 1, "niqe_moments: %d images", N);
  DSR_REQUIRE(hc >= block && wc >= block && hc % block == 0 && wc % block == 0,
              "niqe_moments: a plane of %dx%d is not whole blocks of %d", hc, wc, block);
  DSR_REQUIRE((long long)N * hc * wc < (1ll << 31), "niqe_moments: more than 2^31 pixels");
  const int nby = hc / block, nbx = wc / block;
  const int blocks = N * nby * nbx;
  if (block == NIQE_BLOCK) {
    constexpr int T = 1024, lds = niqe_moments_lds<NIQE_BLOCK, T>();
    static LdsOptIn opt;
    opt.ensure(reinterpret_cast<const void*>(&niqe_moments_kernel<NIQE_BLOCK, T>), lds);
    hipLaunchKernelGGL((niqe_moments_kernel<NIQE_BLOCK, T>), dim3(blocks), dim3(T), lds, st, plane, hc, wc, nby, nbx, window,
                       out);
  } else {
    constexpr int T = 256, lds = niqe_moments_lds<NIQE_BLOCK / 2, T>();
    hipLaunchKernelGGL((niqe_moments_kernel<NIQE_BLOCK / 2, T>), dim3(blocks), dim3(T), lds, st, plane, hc, wc, nby, nbx, window,
                       out);
  }
  return dsr_launch_status("dsr_niqe_moments");
}

extern "C" int dsr_niqe_features(const double* m1, const double* m2, int N, int nb, const double* tables, double* feat,
                                 dsr_stream_t st) {
  DSR_REQUIRE(m1 && m2 && tables && feat, "niqe_features: null pointer");
  DSR_REQUIRE(N >= 1 && nb >= 1, "niqe_features: %d images of %d blocks", N, nb);
  DSR_REQUIRE((long long)N * nb * 10 < (1ll << 31), "niqe_features: %d images of %d blocks are too many fits", N, nb);
  const unsigned total = (unsigned)N * (unsigned)nb * 10u;
  hipLaunchKernelGGL(niqe_features_kernel, dim3((total + 255u) / 256u), dim3(256), 0, st, m1, m2, total, tables, feat);
  return dsr_launch_status("dsr_niqe_features");
}
