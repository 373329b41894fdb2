// Pointwise pieces of SRVGGNetCompact's composed (training) form, models/GAN/srvgg.py:
//   dsr_pw_prelu_c_fwd / _bwd   nn.PReLU(num_parameters=C) on a 16-bit NHWC tensor.  The backward takes the branch from the
//                               STORED PRE-ACTIVATION z, never from the output, so every slope (negative, zero) is exact:
//                                   dz = r16(dy * (z > 0 ? 1 : slope[c])),  dslope[c] = sum dy * z * [z <= 0]   (torch's rules at 0)
//                               The slope gradient: block r sums its pixel range into row r of `partial` (per thread in pixel
//                               order, then across the block's pixel lanes in lane order), the fold kernel adds the rows of a
//                               channel (thread t: rows t, t + FOLD_W, ... in order; then a fixed butterfly).  No atomics: two
//                               runs give equal bits.
//   dsr_shuffle_add_f32 / _bwd  out[n][c][s y + i][s x + j] = t[n][c s^2 + i s + j][y][x] + base[n][c][y][x] on fp32 NCHW, and its
//                               transpose (dbase sums the s^2 sub-pixels in i-then-j order).
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int PC_FOLD_W = 64;        // threads of the fold that share a channel's rows
constexpr int PC_MAX_ROWS = 1024;
constexpr int PC_MIN_PIX = 64;       // pixels per partial row, at least
}   // namespace

template <int DT>
__global__ __launch_bounds__(256) void prelu_c_fwd_kernel(const U4* __restrict__ z, const float* __restrict__ slope, U4* __restrict__ y,
                                                          size_t nvec, int C, int chunks) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += step) {
    const int c0 = (int)(i % (size_t)chunks) * 8;
    float f[8];
    unpack8<DT>(z[i], f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float sl = c0 + k < C ? slope[c0 + k] : 0.f;
      f[k] = f[k] > 0.f ? f[k] : f[k] * sl;
    }
    y[i] = pack8<DT>(f);
  }
}

// block r: pixels [r ppr, min(P, (r + 1) ppr)); thread = (pixel lane, 8-channel chunk)
template <int DT>
__global__ __launch_bounds__(256) void prelu_c_bwd_kernel(const U4* __restrict__ dy, const U4* __restrict__ z,
                                                          const float* __restrict__ slope, U4* __restrict__ dz, size_t P, size_t ppr,
                                                          int C, int chunks, float* __restrict__ partial) {
  extern __shared__ float s_part[];                     // [npl][chunks * 8]
  const int npl = 256 / chunks;                         // pixel lanes
  const int pl = threadIdx.x / chunks, chunk = threadIdx.x - pl * chunks;
  const size_t p0 = (size_t)blockIdx.x * ppr;
  const size_t p1 = p0 + ppr < P ? p0 + ppr : P;
  float sl[8], acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    sl[k] = chunk * 8 + k < C ? slope[chunk * 8 + k] : 0.f;
    acc[k] = 0.f;
  }
  if (pl < npl) {
    for (size_t p = p0 + pl; p < p1; p += npl) {
      const size_t i = p * chunks + chunk;
      float g[8], v[8];
      unpack8<DT>(dy[i], g);
      unpack8<DT>(z[i], v);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool pos = v[k] > 0.f;
        if (!pos) acc[k] += g[k] * v[k];
        g[k] = g[k] * (pos ? 1.f : sl[k]);
      }
      dz[i] = pack8<DT>(g);
    }
  }
  if (!partial) return;
  const int Cp = chunks * 8;
  if (pl < npl) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s_part[pl * Cp + chunk * 8 + k] = acc[k];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < Cp; c += 256) {
    float s = 0.f;
    for (int l = 0; l < npl; ++l) s += s_part[l * Cp + c];
    partial[(size_t)blockIdx.x * Cp + c] = s;
  }
}

// one wave per channel
__global__ __launch_bounds__(PC_FOLD_W) void prelu_c_fold_kernel(const float* __restrict__ partial, int rows, int Cp, float* __restrict__ dslope) {
  const int c = blockIdx.x;
  float s = 0.f;
  for (int r = threadIdx.x; r < rows; r += PC_FOLD_W) s += partial[(size_t)r * Cp + c];
  s = wave_sum(s);
  if (threadIdx.x == 0) dslope[c] = s;
}

template <int S>
__global__ __launch_bounds__(256) void shuffle_add_kernel(const float* __restrict__ t, const float* __restrict__ base, float* __restrict__ out,
                                                          size_t total, int C, int H, int W) {
  // one thread per OUTPUT element (coalesced stores)
  const size_t step = (size_t)gridDim.x * blockDim.x;
  const size_t OW = (size_t)S * W, OH = (size_t)S * H;
  for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += step) {
    const size_t ox = o % OW, r1 = o / OW;
    const size_t oy = r1 % OH, nc = r1 / OH;
    const size_t c = nc % C, n = nc / C;
    const size_t x = ox / S, j = ox - x * S, y = oy / S, i = oy - y * S;
    float v = t[((n * C * S * S + c * S * S + i * S + j) * H + y) * W + x];
    if (base) v += base[(nc * H + y) * W + x];
    out[o] = v;
  }
}

template <int S>
__global__ __launch_bounds__(256) void shuffle_add_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dt, float* __restrict__ dbase,
                                                              size_t total, int C, int H, int W) {
  // one thread per LR pixel of a colour plane: its s^2 sub-pixels, i then j
  const size_t step = (size_t)gridDim.x * blockDim.x;
  const size_t OW = (size_t)S * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    const size_t x = p % W, r1 = p / W;
    const size_t y = r1 % H, nc = r1 / H;
    const size_t c = nc % C, n = nc / C;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const float g = dout[(nc * S * H + S * y + i) * OW + S * x + j];
        dt[((n * C * S * S + c * S * S + i * S + j) * H + y) * W + x] = g;
        s += g;
      }
    if (dbase) dbase[p] = s;
  }
}

// ---- host side
static unsigned pc_grid(size_t n) {
  const size_t want = (n + 255) / 256;
  return (unsigned)(want > 8192 ? 8192 : (want ? want : 1));
}

extern "C" int dsr_pw_prelu_c_fwd(int dtype, const void* z, const float* slope, void* y, size_t P, int C, int Cp, hipStream_t st) {
  DSR_REQUIRE(z && slope && y, "pw_prelu_c_fwd: null pointer");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype) && P > 0 && DSR_CP_OK(Cp) && C >= 1 && C <= Cp, "pw_prelu_c_fwd: bad dtype, P = 0, Cp %d or C %d", Cp, C);
  const size_t nvec = P * (Cp / 8);
  if (dtype == DSR_DTYPE_BF16)
    hipLaunchKernelGGL((prelu_c_fwd_kernel<DSR_DTYPE_BF16>), dim3(pc_grid(nvec)), dim3(256), 0, st, (const U4*)z, slope, (U4*)y, nvec, C, Cp / 8);
  else
    hipLaunchKernelGGL((prelu_c_fwd_kernel<DSR_DTYPE_F16>), dim3(pc_grid(nvec)), dim3(256), 0, st, (const U4*)z, slope, (U4*)y, nvec, C, Cp / 8);
  return dsr_launch_status("dsr_pw_prelu_c_fwd");
}

extern "C" int dsr_pw_prelu_c_rows(size_t P) {
  if (P == 0) return 0;
  const size_t rows = (P + PC_MIN_PIX - 1) / PC_MIN_PIX;
  return (int)(rows > PC_MAX_ROWS ? PC_MAX_ROWS : rows);
}

extern "C" int dsr_pw_prelu_c_fold_width(void) { return PC_FOLD_W; }

extern "C" int dsr_pw_prelu_c_bwd(int dtype, const void* dy, const void* z, const float* slope, void* dz, size_t P, int C, int Cp,
                                  float* partial, float* dslope, hipStream_t st) {
  DSR_REQUIRE(dy && z && slope && dz, "pw_prelu_c_bwd: null pointer");
  DSR_REQUIRE(DSR_DTYPE_OK(dtype) && P > 0 && DSR_CP_OK(Cp) && C >= 1 && C <= Cp, "pw_prelu_c_bwd: bad dtype, P = 0, Cp %d or C %d", Cp, C);
  DSR_REQUIRE((partial != nullptr) == (dslope != nullptr), "pw_prelu_c_bwd: partial and dslope go together");
  const int rows = dsr_pw_prelu_c_rows(P);
  const size_t ppr = (P + rows - 1) / rows;
  const int chunks = Cp / 8;
  const int npl = 256 / chunks;
  const size_t lds = partial ? (size_t)npl * Cp * sizeof(float) : 0;
  // (a row whose range is empty -- P not a multiple of ppr near the cap -- writes zeros)
  if (dtype == DSR_DTYPE_BF16)
    hipLaunchKernelGGL((prelu_c_bwd_kernel<DSR_DTYPE_BF16>), dim3(rows), dim3(256), lds, st, (const U4*)dy, (const U4*)z, slope, (U4*)dz, P, ppr, C,
                       chunks, partial);
  else
    hipLaunchKernelGGL((prelu_c_bwd_kernel<DSR_DTYPE_F16>), dim3(rows), dim3(256), lds, st, (const U4*)dy, (const U4*)z, slope, (U4*)dz, P, ppr, C,
                       chunks, partial);
  int rc = dsr_launch_status("dsr_pw_prelu_c_bwd");
  if (rc != 0 || !partial) return rc;
  hipLaunchKernelGGL(prelu_c_fold_kernel, dim3(C), dim3(PC_FOLD_W), 0, st, partial, rows, Cp, dslope);
  return dsr_launch_status("dsr_pw_prelu_c_bwd (fold)");
}

static const char* shuffle_error(int N, int C, int s, int H, int W) {
  if (N < 1 || C < 1 || H < 1 || W < 1) return "N, C, H, W must be positive";
  if (s < 1 || s > 4) return "s must be in 1..4";
  if ((size_t)N * C * H * W * s * s >= 0x7FFFFFFFull) return "2^31 elements or more";
  return nullptr;
}

extern "C" int dsr_shuffle_add_f32(const float* t, const float* base, float* out, int N, int C, int s, int H, int W, hipStream_t st) {
  DSR_REQUIRE(t && out, "shuffle_add_f32: null pointer");
  const char* err = shuffle_error(N, C, s, H, W);
  DSR_REQUIRE(!err, "shuffle_add_f32: %s", err);
  const size_t total = (size_t)N * C * H * W * s * s;
#define SA_LAUNCH(S) hipLaunchKernelGGL((shuffle_add_kernel<S>), dim3(pc_grid(total)), dim3(256), 0, st, t, base, out, total, C, H, W)
  switch (s) {
    case 1: SA_LAUNCH(1); break;
    case 2: SA_LAUNCH(2); break;
    case 3: SA_LAUNCH(3); break;
    default: SA_LAUNCH(4); break;
  }
#undef SA_LAUNCH
  return dsr_launch_status("dsr_shuffle_add_f32");
}

extern "C" int dsr_shuffle_add_bwd_f32(const float* dout, float* dt, float* dbase, int N, int C, int s, int H, int W, hipStream_t st) {
  DSR_REQUIRE(dout && dt, "shuffle_add_bwd_f32: null pointer");
  const char* err = shuffle_error(N, C, s, H, W);
  DSR_REQUIRE(!err, "shuffle_add_bwd_f32: %s", err);
  const size_t total = (size_t)N * C * H * W;
#define SB_LAUNCH(S) hipLaunchKernelGGL((shuffle_add_bwd_kernel<S>), dim3(pc_grid(total)), dim3(256), 0, st, dout, dt, dbase, total, C, H, W)
  switch (s) {
    case 1: SB_LAUNCH(1); break;
    case 2: SB_LAUNCH(2); break;
    case 3: SB_LAUNCH(3); break;
    default: SB_LAUNCH(4); break;
  }
#undef SB_LAUNCH
  return dsr_launch_status("dsr_shuffle_add_bwd_f32");
}
