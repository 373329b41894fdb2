// Dense (learnable) Downsampler: ReplicationPad2d(p) + Conv2d(C, C, k, stride=f) + bias on fp32 NCHW, C <= 4
// (utils/downsampler.py:44-71 with every filter live, which is what get_params('down') optimises).
//   y[n][co][oy][ox] = b[co] + sum_ci sum_ij w[co][ci][i][j] x[n][ci][clamp(oy f + i - p)][clamp(ox f + j - p)]
// All arithmetic is fp32 FMA on the vector ALU.  The three kernels share one arithmetic shape: one LDS read feeds C FMAs
// whose other operand is wave-uniform (a scalar load), so the inner loops hold no address arithmetic and no branches.
//   forward : a block owns 64 outputs of one output row; its 4 waves split the kernel rows, each staging its input row
//             phase-split ([col mod f][col div f]) so that lanes stride-f apart read consecutive LDS words
//   wgrad   : a thread owns one tap (ci, i, j) and C accumulators; lanes run along j, dy is the uniform operand;
//             a block walks a slab of output rows and writes its partial to the workspace, a second launch sums the
//             slabs in index order (no float atomics: two calls give the same bits) and forms db
//   dgrad   : sub-pixel form: the lanes of a wave share the phase (y+p mod f, x+p mod f), so the taps they need are
//             uniform and each pixel costs (k/f)^2 C terms from a staged dy tile; a second small launch adds what the
//             replicate pad folded onto the border pixels
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {

constexpr int DSD_MAXC = 4;
constexpr size_t DSD_LDS_MAX = 64 * 1024;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ------------------------------------------------------------------ forward
// grid (ceil(OW/64), OH, N), 256 threads.  LDS: 4 wave-private row images of f*S floats + 4*C*64 floats of partials.
template <int C>
__global__ __launch_bounds__(256) void dsd_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ y, int H, int W,
                                                      int OH, int OW, int k, int f, int p, int S, int fshift) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ox0 = blockIdx.x * 64, oy = blockIdx.y, n = blockIdx.z;
  const int nox = OW - ox0 < 64 ? OW - ox0 : 64;
  const int PW = (nox - 1) * f + k;           // input columns this block's outputs touch
  const int cb = ox0 * f - p;
  float* buf = lds + wave * f * S;
  float* red = lds + 4 * f * S;
  const size_t wco = (size_t)C * k * k;       // weight stride between output channels
  float acc[C];
#pragma unroll
  for (int co = 0; co < C; ++co) acc[co] = 0.f;
  const int trips = (k + 3) / 4;              // the same trip count in every wave: the barrier below is block-wide
  for (int ci = 0; ci < C; ++ci) {
    const float* xp = x + ((size_t)n * C + ci) * H * W;
    for (int r = 0; r < trips; ++r) {
      const int i = r * 4 + wave;
      if (i < k) {
        const float* xr = xp + (size_t)clampi(oy * f + i - p, H - 1) * W;
        for (int c = lane; c < PW; c += 64) {
          int q, ph;
          if (fshift >= 0) {
            q = c >> fshift;
            ph = c & (f - 1);
          } else {
            q = c / f;
            ph = c - q * f;
          }
          buf[ph * S + q] = xr[clampi(cb + c, W - 1)];
        }
      }
      __syncthreads();   // the image is wave-private; LDS executes a wave's accesses in order, so one barrier per row is enough
      if (i < k) {
        const float* wr = w + ((size_t)ci * k + i) * k;
        const float* rp = buf + lane;
        int ph = 0, q = 0;
#pragma unroll 4
        for (int j = 0; j < k; ++j) {
          const float xv = rp[ph * S + q];
#pragma unroll
          for (int co = 0; co < C; ++co) acc[co] = fmaf(wr[co * wco + j], xv, acc[co]);
          if (++ph == f) {
            ph = 0;
            ++q;
          }
        }
      }
    }
  }
#pragma unroll
  for (int co = 0; co < C; ++co) red[(wave * C + co) * 64 + lane] = acc[co];
  __syncthreads();
  if (wave == 0 && lane < nox) {
#pragma unroll
    for (int co = 0; co < C; ++co) {
      float s = red[co * 64 + lane];
      for (int wv = 1; wv < 4; ++wv) s += red[(wv * C + co) * 64 + lane];
      if (b) s += b[co];
      y[(((size_t)n * C + co) * OH + oy) * OW + ox0 + lane] = s;
    }
  }
}

// ------------------------------------------------------------------ weight gradient
struct WgPlan {
  int JW, JSH, RPW, IB, NI, NJ, RS, NSX, RB, NRB;
  int slabs, groups;
};

WgPlan wg_plan(int N, int C, int H, int W, int k, int f, int p) {
  WgPlan P;
  const int OH = (H + 2 * p - k) / f + 1, OW = (W + 2 * p - k) / f + 1;
  P.JW = k > 32 ? 64 : (k > 16 ? 32 : (k > 8 ? 16 : 8));   // lanes along j; 64 / JW kernel rows share a wave
  P.JSH = P.JW == 64 ? 6 : (P.JW == 32 ? 5 : (P.JW == 16 ? 4 : 3));
  P.RPW = 64 / P.JW;
  P.IB = 4 * P.RPW;
  P.NI = (k + P.IB - 1) / P.IB;
  P.NJ = (k + 63) / 64;
  // a 32-lane group of an LDS read holds 32 / JW rows: a row stride of JW (mod 32) words keeps them on different banks
  int rs = 63 * f + P.NJ * 64 + P.JW;
  if (P.JW < 32) rs += ((P.JW - rs % 32) + 32) % 32;
  P.RS = rs;
  P.NSX = (OW + 63) / 64;
  P.groups = C * P.NI * P.NJ;
  int target = 2048 / P.groups;
  target = target < 1 ? 1 : (target > 256 ? 256 : target);
  int per = target / (N * P.NSX);             // row blocks per (image, column strip)
  per = per < 1 ? 1 : per;
  int rb = (OH + per - 1) / per;
  if (rb < 1) rb = 1;
  P.RB = rb;
  P.NRB = (OH + P.RB - 1) / P.RB;
  P.slabs = N * P.NSX * P.NRB;
  return P;
}

// grid (groups, slabs), 256 threads.  LDS: IB rows of RS floats.
template <int C>
__global__ __launch_bounds__(256) void dsd_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        float* __restrict__ ws, int H, int W, int OH, int OW, int k,
                                                        int f, int p, WgPlan P) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int g = blockIdx.x;
  const int jc = g % P.NJ;
  g /= P.NJ;
  const int ig = g % P.NI, ci = g / P.NI;
  int s = blockIdx.y;
  const int rb = s % P.NRB;
  s /= P.NRB;
  const int sx = s % P.NSX, n = s / P.NSX;
  const int ox0 = sx * 64;
  const int nox = OW - ox0 < 64 ? OW - ox0 : 64;
  const int PW = (nox - 1) * f + k;
  const int cb = ox0 * f - p;
  const int il = lane >> P.JSH, jl = lane & (P.JW - 1);
  const int rl = wave * P.RPW + il;           // this thread's row of the staged block
  const int i = ig * P.IB + rl, j = jc * 64 + jl;
  const float* xp = x + ((size_t)n * C + ci) * H * W;
  const float* xs = lds + rl * P.RS + (j < k ? j : k - 1);
  const size_t plane = (size_t)OH * OW;
  float acc[C];
#pragma unroll
  for (int co = 0; co < C; ++co) acc[co] = 0.f;
  const int oy1 = (rb + 1) * P.RB < OH ? (rb + 1) * P.RB : OH;
  for (int oy = rb * P.RB; oy < oy1; ++oy) {
    __syncthreads();
    for (int r = 0; r < P.RPW; ++r) {
      const int row = wave * P.RPW + r;
      const float* xr = xp + (size_t)clampi(oy * f + ig * P.IB + row - p, H - 1) * W;
      float* dst = lds + row * P.RS;
      for (int c = lane; c < PW; c += 64) dst[c] = xr[clampi(cb + c, W - 1)];
    }
    __syncthreads();
    const float* dp = dy + ((size_t)n * C * OH + oy) * OW + ox0;
#pragma unroll 8
    for (int t = 0; t < nox; ++t) {
      const float xv = xs[t * f];
#pragma unroll
      for (int co = 0; co < C; ++co) acc[co] = fmaf(dp[co * plane + t], xv, acc[co]);
    }
  }
  if (i < k && j < k) {
#pragma unroll
    for (int co = 0; co < C; ++co)
      ws[(((size_t)blockIdx.y * C + co) * C + ci) * k * k + (size_t)i * k + j] = acc[co];
  }
}

// dw = sum of the slabs in index order; the last C blocks form db[co] = sum dy with a fixed-shape tree
__global__ __launch_bounds__(256) void dsd_wgrad_finalize_kernel(const float* __restrict__ ws,
                                                                 const float* __restrict__ dy, float* __restrict__ dw,
                                                                 float* __restrict__ db, int slabs, int taps, int wblocks,
                                                                 int N, int C, int plane) {
  __shared__ float red[256];
  if ((int)blockIdx.x < wblocks) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= taps) return;
    float s = 0.f;
    for (int sl = 0; sl < slabs; ++sl) s += ws[(size_t)sl * taps + idx];
    dw[idx] = s;
    return;
  }
  const int co = blockIdx.x - wblocks;
  float s = 0.f;
  for (int n = 0; n < N; ++n) {
    const float* dp = dy + ((size_t)n * C + co) * plane;
    for (int e = threadIdx.x; e < plane; e += 256) s += dp[e];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[co] = red[0];
}

// ------------------------------------------------------------------ input gradient
// Padded coordinates u = a + p, v = b + p; u = my f + ry, v = mx f + rx.  The gradient at (u, v) is
//   G[ci] = sum_co sum_{dy,dx} w[co][ci][ry + dy f][rx + dx f] * dY[co][my - dy][mx - dx]
// grid (tiles_x, tiles_y, N * PS), 256 threads; a block owns an 8 x 8 tile of (my, mx) and its waves walk the phases
// (ry, rx).  This launch writes every pixel's own term u = y + p, v = x + p; dsd_dgrad_border_kernel adds the folded ones.
template <int C>
__global__ __launch_bounds__(256) void dsd_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                        float* __restrict__ dx, int H, int W, int OH, int OW, int k,
                                                        int f, int p, int D, int TS, int PS, int my_lo, int mx_lo) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.z / PS, ps = blockIdx.z % PS;
  const int my0 = my_lo + blockIdx.y * 8, mx0 = mx_lo + blockIdx.x * 8;
  const int TH = 7 + D;                       // tile rows / columns: oy in [my0 - D + 1, my0 + 7]
  const size_t plane = (size_t)OH * OW;
  for (int e = threadIdx.x; e < C * TH * TS; e += 256) {
    const int c = e % TS, r = (e / TS) % TH, co = e / (TS * TH);
    const int oy = my0 - D + 1 + r, ox = mx0 - D + 1 + c;
    float v = 0.f;
    if (c < TH && oy >= 0 && oy < OH && ox >= 0 && ox < OW) v = dy[((size_t)n * C + co) * plane + (size_t)oy * OW + ox];
    lds[e] = v;
  }
  __syncthreads();
  const int ly = lane >> 3, lx = lane & 7;
  const float* tp = lds + (ly + D - 1) * TS + lx + D - 1;
  const size_t kk = (size_t)k * k;
  for (int ph = ps * 4 + wave; ph < f * f; ph += 4 * PS) {
    const int ry = ph / f, rx = ph - ry * f;
    float acc[C];
#pragma unroll
    for (int ci = 0; ci < C; ++ci) acc[ci] = 0.f;
    for (int co = 0; co < C; ++co) {
      const float* tc = tp + co * TH * TS;
      const float* wc = w + (size_t)co * C * kk;
      for (int dyi = 0, i = ry; i < k; ++dyi, i += f) {
        for (int dxi = 0, j = rx; j < k; ++dxi, j += f) {
          const float dv = tc[-dyi * TS - dxi];
#pragma unroll
          for (int ci = 0; ci < C; ++ci) acc[ci] = fmaf(wc[ci * kk + (size_t)i * k + j], dv, acc[ci]);
        }
      }
    }
    const int yy = (my0 + ly) * f + ry - p, xx = (mx0 + lx) * f + rx - p;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
#pragma unroll
      for (int ci = 0; ci < C; ++ci) dx[(((size_t)n * C + ci) * H + yy) * W + xx] = acc[ci];
    }
  }
}

// One wave per border pixel (n, y, x): its lanes share out the padded coordinates that ReplicationPad2d folded onto it
// (its own one excepted), each lane gathers (k/f)^2 C terms per channel, a fixed butterfly sums them, lane 0 adds to dx.
template <int C>
__global__ __launch_bounds__(256) void dsd_dgrad_border_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                               float* __restrict__ dx, int N, int H, int W, int OH, int OW,
                                                               int k, int f, int p) {
  const int lane = threadIdx.x & 63;
  const int per = W >= 2 ? 2 * W + (H > 2 ? 2 * (H - 2) : 0) : H;   // border pixels of one image plane
  const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (long long)N * per) return;
  const int n = (int)(wid / per);
  int e = (int)(wid % per), yy, xx;
  if (W < 2) {
    yy = e;
    xx = 0;
  } else if (e < W) {
    yy = 0;
    xx = e;
  } else if (e < 2 * W) {
    if (H < 2) return;      // a single row is its own top and bottom border: already covered
    yy = H - 1;
    xx = e - W;
  } else {
    e -= 2 * W;
    yy = 1 + (e >> 1);
    xx = (e & 1) ? W - 1 : 0;
  }
  // padded coordinates (unpadded frame) that fold onto this pixel
  const int ya0 = yy == 0 ? -p : yy, ya1 = yy == H - 1 ? H - 1 + p : yy;
  const int xa0 = xx == 0 ? -p : xx, xa1 = xx == W - 1 ? W - 1 + p : xx;
  const int na = ya1 - ya0 + 1, nbx = xa1 - xa0 + 1;
  const size_t plane = (size_t)OH * OW, kk = (size_t)k * k;
  float acc[C];
#pragma unroll
  for (int ci = 0; ci < C; ++ci) acc[ci] = 0.f;
  for (int t = lane; t < na * nbx; t += 64) {
    const int a = ya0 + t / nbx, bq = xa0 + t % nbx;
    if (a == yy && bq == xx) continue;        // the pixel's own term is dsd_dgrad_kernel's
    const int u = a + p, v = bq + p;
    int oyl = (u - k + f) / f;                // ceil((u - k + 1) / f) for u - k + 1 > 0
    if (u - k + 1 <= 0) oyl = 0;
    int oyh = u / f;
    if (oyh > OH - 1) oyh = OH - 1;
    int oxl = (v - k + f) / f;
    if (v - k + 1 <= 0) oxl = 0;
    int oxh = v / f;
    if (oxh > OW - 1) oxh = OW - 1;
    for (int co = 0; co < C; ++co) {
      const float* dp = dy + ((size_t)n * C + co) * plane;
      const float* wc = w + (size_t)co * C * kk;
      for (int oy = oyl; oy <= oyh; ++oy) {
        const int i = u - oy * f;
        for (int ox = oxl; ox <= oxh; ++ox) {
          const int j = v - ox * f;
          const float dv = dp[(size_t)oy * OW + ox];
#pragma unroll
          for (int ci = 0; ci < C; ++ci) acc[ci] = fmaf(wc[ci * kk + (size_t)i * k + j], dv, acc[ci]);
        }
      }
    }
  }
#pragma unroll
  for (int ci = 0; ci < C; ++ci) {
    float s = acc[ci];
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) dx[(((size_t)n * C + ci) * H + yy) * W + xx] += s;
  }
}

int pow2_shift(int f) {
  for (int s = 0; s < 31; ++s)
    if ((1 << s) == f) return s;
  return -1;
}

}  // namespace

#define DSD_C_SWITCH(C, CALL)   \
  switch (C) {                  \
    case 1: { constexpr int CC = 1; CALL; } break; \
    case 2: { constexpr int CC = 2; CALL; } break; \
    case 3: { constexpr int CC = 3; CALL; } break; \
    default: { constexpr int CC = 4; CALL; } break; \
  }

#define DSD_SHAPE_CHECK(what)                                                                                          \
  DSR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && k > 0 && f > 0 && p >= 0, what ": bad shape");                       \
  if (C > DSD_MAXC) return dsr_fail(DSR_E_UNSUPPORTED, what ": C %d > %d", C, DSD_MAXC);                               \
  DSR_REQUIRE(H + 2 * p >= k && W + 2 * p >= k, what ": empty output");                                                \
  DSR_REQUIRE(N <= 16384 && (long long)H * W <= (1 << 28) && k <= 4096 && f <= 4096 && p <= 4096,                    \
              what ": shape out of range");                                                                            \
  const int OH = (H + 2 * p - k) / f + 1, OW = (W + 2 * p - k) / f + 1;                                                \
  DSR_REQUIRE(OH <= 65535, what ": more than 65535 output rows")

extern "C" int dsr_downsample_dense_fwd(const float* x, const float* w, const float* b, float* y, int N, int C, int H,
                                        int W, int k, int f, int p, dsr_stream_t st) {
  DSR_REQUIRE(x && w && y, "downsample_dense_fwd: null pointer");
  DSD_SHAPE_CHECK("downsample_dense_fwd");
  const int S = 64 + (k + f - 1) / f;
  const size_t lds = ((size_t)4 * f * S + (size_t)4 * C * 64) * sizeof(float);
  if (lds > DSD_LDS_MAX) return dsr_fail(DSR_E_UNSUPPORTED, "downsample_dense_fwd: k %d at stride %d needs %zu B of LDS", k, f, lds);
  dim3 grid((OW + 63) / 64, OH, N);
  DSD_C_SWITCH(C, hipLaunchKernelGGL((dsd_fwd_kernel<CC>), grid, dim3(256), lds, st, x, w, b, y, H, W, OH, OW, k, f, p,
                                     S, pow2_shift(f)));
  return dsr_launch_status("dsr_downsample_dense_fwd");
}

extern "C" int dsr_downsample_dense_dgrad(const float* dy, const float* w, float* dx, int N, int C, int H, int W, int k,
                                          int f, int p, dsr_stream_t st) {
  DSR_REQUIRE(dy && w && dx, "downsample_dense_dgrad: null pointer");
  DSD_SHAPE_CHECK("downsample_dense_dgrad");
  const int D = (k + f - 1) / f;
  int TS = 7 + D;
  TS += ((8 - TS % 32) + 32) % 32;            // 8 (mod 32): the four tile rows of a 32-lane group sit on different banks
  const size_t lds = (size_t)C * (7 + D) * TS * sizeof(float);
  if (lds > DSD_LDS_MAX) return dsr_fail(DSR_E_UNSUPPORTED, "downsample_dense_dgrad: k %d at stride %d needs %zu B of LDS", k, f, lds);
  // pixels y in [0, H) have u = y + p in [p, H - 1 + p]
  const int my_lo = p / f, my_hi = (H - 1 + p) / f, mx_lo = p / f, mx_hi = (W - 1 + p) / f;
  const int ty = (my_hi - my_lo) / 8 + 1, tx = (mx_hi - mx_lo) / 8 + 1;
  DSR_REQUIRE(ty <= 65535, "downsample_dense_dgrad: too many tile rows");
  const long long tiles = (long long)ty * tx * N;
  const int phase_groups = (f * f + 3) / 4;   // 4 waves take 4 phases at a time
  int PS = (int)((1024 + tiles - 1) / tiles);
  PS = PS < 1 ? 1 : (PS > phase_groups ? phase_groups : PS);
  DSR_REQUIRE((long long)N * PS <= 65535, "downsample_dense_dgrad: batch too large");
  DSD_C_SWITCH(C, hipLaunchKernelGGL((dsd_dgrad_kernel<CC>), dim3(tx, ty, N * PS), dim3(256), lds, st, dy, w, dx, H, W,
                                     OH, OW, k, f, p, D, TS, PS, my_lo, mx_lo));
  if (p > 0) {
    const long long per = W >= 2 ? 2LL * W + (H > 2 ? 2LL * (H - 2) : 0) : H;
    const long long blocks = (N * per + 3) / 4;
    DSD_C_SWITCH(C, hipLaunchKernelGGL((dsd_dgrad_border_kernel<CC>), dim3((unsigned)blocks), dim3(256), 0, st, dy, w,
                                       dx, N, H, W, OH, OW, k, f, p));
  }
  return dsr_launch_status("dsr_downsample_dense_dgrad");
}

extern "C" size_t dsr_downsample_dense_wgrad_workspace(int N, int C, int H, int W, int k, int f, int p) {
  if (N <= 0 || C <= 0 || C > DSD_MAXC || H <= 0 || W <= 0 || k <= 0 || f <= 0 || p < 0 || H + 2 * p < k ||
      W + 2 * p < k || N > 16384 || (long long)H * W > (1 << 28) || k > 4096 || f > 4096 || p > 4096)
    return 0;
  const WgPlan P = wg_plan(N, C, H, W, k, f, p);
  return (size_t)P.slabs * C * C * k * k * sizeof(float);
}

extern "C" int dsr_downsample_dense_wgrad(const float* x, const float* dy, float* dw, float* db, void* workspace,
                                          size_t workspace_bytes, int N, int C, int H, int W, int k, int f, int p,
                                          dsr_stream_t st) {
  DSR_REQUIRE(x && dy && dw && workspace, "downsample_dense_wgrad: null pointer");
  DSD_SHAPE_CHECK("downsample_dense_wgrad");
  const WgPlan P = wg_plan(N, C, H, W, k, f, p);
  const size_t need = (size_t)P.slabs * C * C * k * k * sizeof(float);
  if (workspace_bytes < need)
    return dsr_fail(DSR_E_WORKSPACE, "downsample_dense_wgrad: workspace %zu B < %zu B", workspace_bytes, need);
  const size_t lds = (size_t)P.IB * P.RS * sizeof(float);
  if (lds > DSD_LDS_MAX) return dsr_fail(DSR_E_UNSUPPORTED, "downsample_dense_wgrad: k %d at stride %d needs %zu B of LDS", k, f, lds);
  DSR_REQUIRE(P.slabs <= 65535, "downsample_dense_wgrad: too many slabs");
  float* ws = (float*)workspace;
  DSD_C_SWITCH(C, hipLaunchKernelGGL((dsd_wgrad_kernel<CC>), dim3(P.groups, P.slabs), dim3(256), lds, st, x, dy, ws, H, W,
                                     OH, OW, k, f, p, P));
  const int taps = C * C * k * k, wblocks = (taps + 255) / 256;
  hipLaunchKernelGGL(dsd_wgrad_finalize_kernel, dim3(wblocks + (db ? C : 0)), dim3(256), 0, st, ws, dy, dw, db, P.slabs,
                     taps, wblocks, N, C, OH * OW);
  return dsr_launch_status("dsr_downsample_dense_wgrad");
}
