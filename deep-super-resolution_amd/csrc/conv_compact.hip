// SRVGGNetCompact (Real-ESRGAN's compact generator, models/GAN/srvgg.py): the two launches the network is made of.
//
//   dsr_conv_prelu_c_fwd      a body layer: 3x3 / stride 1 / zero-pad 1, 64 -> 64 channels of a 16-bit NHWC tensor, with a
//                             PER-CHANNEL PReLU (nn.PReLU(num_parameters=64)) in the epilogue.  The slope vector is read from the
//                             parameter's own storage by every launch, and the branch is taken on the fp32 pre-activation in the
//                             accumulators, so any sign of slope is exact (the one-element, output-masked conv + PReLU launches
//                             of conv_api.hip are right for a positive slope only).
//   dsr_conv_shuffle_add_fwd  the tail: 64 -> C s^2 channels, stored through PixelShuffle(s) as fp32 NCHW [N][C][sH][sW] with the
//                             network's own fp32 input added per LR pixel (nearest x s of the input is the input pixel itself for
//                             all s^2 sub-pixels).  No 16-bit rounding anywhere behind the accumulators.
//
// Tiling: conv_rdb.hip's (read conv_halo64.hip's header, then that file's) with ldx = Cin = 64, i.e. two 32-channel K-blocks
// per 8 x 64 pixel tile, the halo and the weight slice of a K-block brought in by LDS-DMA one stage ahead, 8 waves = 4 column
// strips of 16 pixels x 2 halves of the output channels, persistent blocks.  The main loop is that kernel's, restated here
// because this file may not change how that one compiles.  What differs:
//   * body: the epilogue reads slope[c] for the lane's 4 channels (c = chb + 16 nt + 4 g + r) once per launch;
//   * tail: COUT is the MFMA width the C s^2 outputs are padded to (32 or 64).  The packed image is [9][r8(C s^2)][64]; stage
//     rows beyond r8(C s^2) are requested out of range and land as zeros, rows in [C s^2, r8(C s^2)) are the image's pad rows
//     and are never stored.  The accumulators are staged as fp32, transposed to [row][q][column], RP = 128 / COUT tile rows at
//     a time in the halo stage just consumed; the store loop then walks an OUTPUT row: consecutive lanes write consecutive
//     floats out[n][c][s y + i][s x0 ..], the s sub-pixels of a source pixel side by side, as plain dword vector stores.
// No atomics, no hand-off between blocks: a block reads x and writes only its own tile of the output, and the entry points
// refuse overlapping ranges.
#include <stdlib.h>

#include <type_traits>

#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int CP_TR = 8, CP_TC = 64;                    // pixel tile
constexpr int CP_HR = CP_TR + 2, CP_HP = CP_TC + 2;     // halo rows, halo row pitch in pixels
constexpr int CP_SLOTS = CP_HR * CP_HP;                 // 660 pixel slots of 64 B
constexpr int CP_HPIECES = (CP_SLOTS + 15) / 16;        // 42 DMA pieces of 16 slots (1 KB)
constexpr int CP_HALO = CP_HPIECES * 1024;              // 43,008 B per halo stage
constexpr int CP_CIN = 64;                              // input channels = pixel stride of x
constexpr int CP_PITCH = CP_TC + 1;                     // floats per staged (row, q) line of the tail

struct CompactArgs {
  const void* x;
  const void* w;
  const float* bias;
  const float* slope;      // body: [64] or null
  void* y;                 // body: [N][H][W][64] 16-bit
  const float* base;       // tail: [N][C][H][W] fp32 or null
  float* out;              // tail: [N][C][sH][sW] fp32
  int H, W;
  int C, s, Q, R8;         // tail: Q = C s^2 real outputs, R8 = rows per tap of the weight image
  int tiles_y, tiles_x, ntiles;
  unsigned w_bytes, x_img, y_img;
};

template <int COUT>
constexpr int compact_lds() {
  return 2 * CP_HALO + 2 * (9 * COUT / 16) * 1024;      // 159,744 B (64 outputs) | 122,880 B (32)
}
}   // namespace

template <int DT, int COUT, bool TAIL>
__global__ __launch_bounds__(512, 2) void conv_compact_kernel(const CompactArgs a) {
  constexpr int NT = COUT / 32;                         // 16-channel MFMA row blocks per wave
  constexpr int WPIECES = 9 * COUT / 16;                // 36 | 18 pieces: 9 taps x COUT output channels x 64 B
  constexpr int WTS = WPIECES * 1024;
  constexpr int CSTRIDE = COUT * 2 + 16;                // body: staged C pixel pitch
  constexpr int VPP = COUT / 8;                         // body: 16-byte vectors per stored pixel
  constexpr int NIT = 4 * CP_TC * VPP / 512;            // body: store iterations per 4-row half tile
  constexpr int RP = 128 / COUT;                        // tail: tile rows staged per pass (2 | 4)
  static_assert(4 * CP_TC * CSTRIDE <= CP_HALO, "half a 16-bit C tile is staged in one halo stage");
  static_assert(RP * COUT * CP_PITCH * 4 <= CP_HALO, "RP fp32 rows are staged in one halo stage");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const sHalo = smem;
  unsigned char* const sWts = smem + 2 * CP_HALO;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave & 3, wc = wave >> 2;              // 16-column strip, half of the output channels
  const int g = lane >> 4, r16 = lane & 15;
  const int chb = (COUT / 2) * wc;                      // this wave's first output channel
  constexpr unsigned OOB = 0xFFFFFFF0u;
  constexpr int FAR = 0x7FFFFF00;

  // ---- loader, halo: wave w issues the pieces w, w + 8, ... (< 42); lane l of piece p fills slot 16 p + l / 4, chunk l % 4
  constexpr int NHU = (CP_HPIECES + 7) / 8;             // 6
  int h_part[NHU];                                      // ((hr * W + hc) * 64 + chunk * 8) * 2 of this lane's slot, FAR if none
  unsigned long long hc_pack = 0;                       // its halo column, 7 bits per piece
#pragma unroll
  for (int u = 0; u < NHU; ++u) {
    const int slot = 16 * (wave + 8 * u) + (lane >> 2);
    const int hr = slot / CP_HP, hc = slot - hr * CP_HP;
    h_part[u] = slot < CP_SLOTS ? ((hr * a.W + hc) * CP_CIN + (lane & 3) * 8) * 2 : FAR;
    hc_pack |= (unsigned long long)hc << (7 * u);
  }
  // ---- loader, weights: piece q = rows 16 q .. 16 q + 15 of the [9 * COUT] x 32 K-block slice (row = tap * COUT + channel)
  constexpr int NWU = (WPIECES + 7) / 8;                // 5 | 3
  int w_part[NWU];
#pragma unroll
  for (int v = 0; v < NWU; ++v) {
    const int row = 16 * (wave + 8 * v) + (lane >> 2);
    if constexpr (TAIL) {
      // row tap * COUT + c of the stage is row tap * R8 + c of the image [9][R8][64]; c >= R8 does not exist: zeros
      const int tap = row / COUT, c = row - tap * COUT;
      w_part[v] = c < a.R8 ? ((tap * a.R8 + c) * CP_CIN + (lane & 3) * 8) * 2 : FAR;
    } else {
      w_part[v] = (row * CP_CIN + (lane & 3) * 8) * 2;
    }
  }
  const BufSrd wsrd = make_srd(a.w, a.w_bytes);
  const int per_img = a.tiles_y * a.tiles_x;

  struct TileXY {
    int n, ty, tx;
  };
  auto decomp = [&](int t) {
    TileXY c;
    c.n = t / per_img;
    const int rem = t - c.n * per_img;
    c.ty = rem / a.tiles_x;
    c.tx = rem - c.ty * a.tiles_x;
    return c;
  };
  auto fetch = [&](const TileXY& tc, int kb, int buf) {
    const int oy0 = tc.ty * CP_TR - 1, ox0 = tc.tx * CP_TC - 1;
    // per-image resource: halo rows above / below the image fall outside it and read as zeros
    const BufSrd xsrd = make_srd(reinterpret_cast<const unsigned char*>(a.x) + (size_t)tc.n * a.x_img, a.x_img);
    const int sbase = (oy0 * a.W + ox0) * CP_CIN * 2 + kb * 64;
    const bool interior = ox0 >= 0 && ox0 + CP_HP <= a.W;
    unsigned char* hdst = sHalo + buf * CP_HALO;
#pragma unroll
    for (int u = 0; u < NHU; ++u) {
      if (wave + 8 * u >= CP_HPIECES) continue;         // (wave-uniform; only the last round is partial)
      unsigned off = (unsigned)(h_part[u] + sbase);
      if (!interior) {
        const int ix = ox0 + (int)((hc_pack >> (7 * u)) & 127);
        if ((unsigned)ix >= (unsigned)a.W) off = OOB;
      }
      lds_dma16(xsrd, hdst + (wave + 8 * u) * 1024, off);
    }
    unsigned char* wdst = sWts + buf * WTS;
#pragma unroll
    for (int v = 0; v < NWU; ++v) {
      if (wave + 8 * v >= WPIECES) continue;
      lds_dma16(wsrd, wdst + (wave + 8 * v) * 1024, (unsigned)(w_part[v] + kb * 64));
    }
  };

  // fragment addresses: A (pixels) at halo slot (h, 16 wq + tx + r16), chunk g; B (weights) at row tap * COUT + chb + 16 nt + r16
  const int a_off = ((16 * wq + r16) * 64) + 16 * g;
  const int b_off = ((chb + r16) * 64) + 16 * g;
  const int cw_base = (16 * wq + r16) * CSTRIDE + (chb + 4 * g) * 2;      // body: + (row & 3) * 64 * CSTRIDE + nt * 32

  const int tstep = gridDim.x;
  int t = blockIdx.x;
  if (t >= a.ntiles) return;
  TileXY cur = decomp(t);
  constexpr int KB = CP_CIN / 32;
  fetch(cur, 0, 0);
  int buf = 0;

  // per-launch constants of the lane's channels: bias (rows beyond the real outputs have none) and, body, the PReLU slopes
  float bv[NT][4], sl[NT][4];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = chb + 16 * nt + 4 * g + r;
      const bool real = TAIL ? c < a.Q : true;
      bv[nt][r] = (a.bias && real) ? a.bias[c] : 0.f;
      sl[nt][r] = (!TAIL && a.slope) ? a.slope[c] : 1.f;            // (slope == null: v * 1 = v, no activation)
    }

  for (; t < a.ntiles; t += tstep) {
    const bool has_next = t + tstep < a.ntiles;
    const TileXY nxt = has_next ? decomp(t + tstep) : cur;
    f32x4 acc[CP_TR][NT];
#pragma unroll
    for (int i = 0; i < CP_TR; ++i)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[i][nt] = f32x4{bv[nt][0], bv[nt][1], bv[nt][2], bv[nt][3]};
    for (int kb = 0; kb < KB; ++kb, buf ^= 1) {
      // my DMA of this K-block has landed; after the barrier everyone's has, and every wave is done with the other stage
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // (waves 4..7 issue their DMA pieces after their first tap column: one wave's issue runs under its SIMD partner's MFMAs)
      auto prefetch = [&]() {
        if (kb + 1 < KB)
          fetch(cur, kb + 1, buf ^ 1);
        else if (has_next)
          fetch(nxt, 0, buf ^ 1);
      };
      const bool late = wave >= 4;
      if (!late) prefetch();
      const unsigned char* sX = sHalo + buf * CP_HALO + a_off;
      const unsigned char* sW = sWts + buf * WTS + b_off;
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        U4 fb[3][NT];
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) {
          const int tap = ty * 3 + tx;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) fb[ty][nt] = *reinterpret_cast<const U4*>(sW + tap * COUT * 64 + nt * 16 * 64);
        }
        // halo rows as a software pipeline: fragment h + 2 requested before the MFMAs of fragment h
        U4 fa[3];
        auto load = [&](int h) { return *reinterpret_cast<const U4*>(sX + (h * CP_HP + tx) * 64); };
        fa[0] = load(0);
        fa[1] = load(1);
#pragma unroll
        for (int h = 0; h < CP_HR; ++h) {
          if (h + 2 < CP_HR) fa[(h + 2) % 3] = load(h + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ty = 0; ty < 3; ++ty) {
            const int i = h - ty;
            if (i < 0 || i >= CP_TR) continue;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[i][nt] = mfma16<DT>(fb[ty][nt], fa[h % 3], acc[i][nt]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (tx == 0 && late) prefetch();
      }
    }
    // ---- epilogue: the stage just consumed (buf ^ 1 after the loop's flip) becomes the C staging area; the DMA in flight
    // targets the other stage.
    unsigned char* sC = sHalo + (buf ^ 1) * CP_HALO;
    const int oy0 = cur.ty * CP_TR, ox0 = cur.tx * CP_TC;
    if constexpr (!TAIL) {
      unsigned char* const yimg = reinterpret_cast<unsigned char*>(a.y) + (size_t)cur.n * a.y_img;
      const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(yimg, 0, a.y_img, 0x00020000);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        __builtin_amdgcn_s_barrier();          // every wave is done reading the stage (half 0) / the staged half (half 1)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          const int i = half * 4 + ii;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float s = acc[i][nt][r];
              v[r] = s > 0.f ? s : s * sl[nt][r];       // torch's PReLU: the branch of the fp32 pre-activation, any slope
            }
            uint2 pk;
            pk.x = (unsigned)f2h<DT>(v[0]) | ((unsigned)f2h<DT>(v[1]) << 16);
            pk.y = (unsigned)f2h<DT>(v[2]) | ((unsigned)f2h<DT>(v[3]) << 16);
            *reinterpret_cast<uint2*>(sC + cw_base + ii * 64 * CSTRIDE + nt * 32) = pk;
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int vec = tid + 512 * it;
          const int pl = vec / VPP, chunk = vec - pl * VPP;
          const int row = pl >> 6, col = pl & 63;
          const U4 v = *reinterpret_cast<const U4*>(sC + (row * 64 + col) * CSTRIDE + chunk * 16);
          const int sy = oy0 + half * 4 + row, sx = ox0 + col;
          unsigned off = (unsigned)(((sy * a.W + sx) * COUT) * 2 + chunk * 16);
          if (!(sy < a.H && sx < a.W)) off = OOB;      // (the buffer resource drops the store)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), yrsrc, off, 0, 0);
        }
      }
    } else {
      float* const sF = reinterpret_cast<float*>(sC);
      const int fw_base = (chb + 4 * g) * CP_PITCH + 16 * wq + r16;       // + (rr * COUT + 16 nt + r) * CP_PITCH
      const size_t HW = (size_t)a.H * a.W;
      const float* const bimg = a.base ? a.base + (size_t)cur.n * a.C * HW : nullptr;
      float* const oimg = a.out + (size_t)cur.n * a.C * HW * a.s * a.s;
#pragma unroll
      for (int pass = 0; pass < CP_TR / RP; ++pass) {
        __builtin_amdgcn_s_barrier();          // every wave is done reading the stage / the rows staged by the last pass
        asm volatile("" ::: "memory");
#pragma unroll
        for (int rr = 0; rr < RP; ++rr)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sF[fw_base + (rr * COUT + 16 * nt + r) * CP_PITCH] = acc[pass * RP + rr][nt][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // one (tile row, colour plane) at a time: its s output rows of 64 s floats, element e = (i, s col + j) on thread e
        auto store = [&](auto s_tag) {
          constexpr int S = decltype(s_tag)::value;
          const size_t sW_ = (size_t)S * a.W;
          for (int rr = 0; rr < RP; ++rr) {
            const int py = oy0 + pass * RP + rr;
            if (py >= a.H) break;                       // (block-uniform)
            for (int c = 0; c < a.C; ++c) {
              const float* const brow = bimg ? bimg + (size_t)c * HW + (size_t)py * a.W : nullptr;
              float* const oplane = oimg + (size_t)c * HW * S * S;
              for (int e = tid; e < S * S * CP_TC; e += 512) {
                const int i = e / (S * CP_TC), rem = e - i * (S * CP_TC);
                const int col = rem / S, j = rem - col * S;
                const int px = ox0 + col;
                if (px >= a.W) continue;
                float v = sF[(rr * COUT + c * S * S + i * S + j) * CP_PITCH + col];
                if (brow) v += brow[px];
                oplane[((size_t)S * py + i) * sW_ + (size_t)S * px + j] = v;
              }
            }
          }
        };
        switch (a.s) {
          case 1: store(std::integral_constant<int, 1>{}); break;
          case 2: store(std::integral_constant<int, 2>{}); break;
          case 3: store(std::integral_constant<int, 3>{}); break;
          default: store(std::integral_constant<int, 4>{}); break;
        }
      }
    }
    cur = nxt;
  }
}

// ---- host side
static bool ranges_overlap(const void* p, size_t pb, const void* q, size_t qb) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qb && b < a + pb;
}

// shape fields only (no pointers): 0 = fine; `unsupported` tells DSR_E_UNSUPPORTED from DSR_E_ARG
static const char* compact_shape_error(int dtype, int N, int H, int W, size_t out_img_bytes, bool* unsupported) {
  *unsupported = false;
  if (!DSR_DTYPE_OK(dtype)) return "dtype is neither DSR_BF16 nor DSR_F16";
  if (N < 1 || H < 1 || W < 1) return "N, H, W must be positive";
  const size_t pix = (size_t)H * W;
  const size_t img = pix * CP_CIN * 2 > out_img_bytes ? pix * CP_CIN * 2 : out_img_bytes;
  if (img >= 0x7FFFFF00ull) return "a tensor of 2^31 bytes or more per image";
  if (img * N >= 0x100000000ull) return "a tensor of 2^32 bytes or more";
  return nullptr;
}

static void compact_fill(CompactArgs& a, int N, int H, int W) {
  a.H = H;
  a.W = W;
  a.tiles_y = (H + CP_TR - 1) / CP_TR;
  a.tiles_x = (W + CP_TC - 1) / CP_TC;
  a.ntiles = N * a.tiles_y * a.tiles_x;
  a.x_img = (unsigned)((size_t)H * W * CP_CIN * 2);
}

extern "C" int dsr_conv_prelu_c_supported(const dsr_compact_conv* c) {
  if (!c) return 0;
  bool uns;
  return compact_shape_error(c->dtype, c->N, c->H, c->W, 0, &uns) == nullptr ? 1 : 0;
}

extern "C" int dsr_conv_prelu_c_fwd(const dsr_compact_conv* c, hipStream_t st) {
  DSR_REQUIRE(c, "conv_prelu_c_fwd: null descriptor");
  DSR_REQUIRE(c->x && c->w && c->y, "conv_prelu_c_fwd: null pointer (x, w or y)");
  bool uns;
  const char* err = compact_shape_error(c->dtype, c->N, c->H, c->W, 0, &uns);
  if (err && uns) return dsr_fail(DSR_E_UNSUPPORTED, "conv_prelu_c_fwd: %s", err);
  DSR_REQUIRE(!err, "conv_prelu_c_fwd: %s", err);
  const size_t bytes = (size_t)c->N * c->H * c->W * CP_CIN * 2;
  DSR_REQUIRE(!ranges_overlap(c->x, bytes, c->y, bytes), "conv_prelu_c_fwd: the output overlaps the input");
  CompactArgs a{};
  a.x = c->x;
  a.w = c->w;
  a.bias = c->bias;
  a.slope = c->slope;
  a.y = c->y;
  compact_fill(a, c->N, c->H, c->W);
  a.y_img = a.x_img;
  a.w_bytes = (unsigned)(9 * 64 * CP_CIN * 2);
  const int cap = c->max_blocks > 0 ? c->max_blocks : 256;    // persistent: one 8-wave block per CU
  const int blocks = a.ntiles < cap ? a.ntiles : cap;
  static LdsOptIn optin[2];
  if (c->dtype == DSR_DTYPE_BF16) {
    optin[0].ensure((const void*)conv_compact_kernel<DSR_DTYPE_BF16, 64, false>, compact_lds<64>());
    hipLaunchKernelGGL((conv_compact_kernel<DSR_DTYPE_BF16, 64, false>), dim3(blocks), dim3(512), compact_lds<64>(), st, a);
  } else {
    optin[1].ensure((const void*)conv_compact_kernel<DSR_DTYPE_F16, 64, false>, compact_lds<64>());
    hipLaunchKernelGGL((conv_compact_kernel<DSR_DTYPE_F16, 64, false>), dim3(blocks), dim3(512), compact_lds<64>(), st, a);
  }
  return dsr_launch_status("dsr_conv_prelu_c_fwd");
}

static const char* tail_shape_error(const dsr_compact_tail* c, bool* unsupported) {
  *unsupported = false;
  if (c->s < 1 || c->s > 4 || c->C < 1 || c->C > 4) {
    *unsupported = DSR_DTYPE_OK(c->dtype) && c->N >= 1 && c->H >= 1 && c->W >= 1 && c->s >= 1 && c->C >= 1;
    return "s and C must be in 1..4";
  }
  return compact_shape_error(c->dtype, c->N, c->H, c->W, (size_t)c->H * c->W * c->C * c->s * c->s * 4, unsupported);
}

extern "C" int dsr_conv_shuffle_add_supported(const dsr_compact_tail* c) {
  if (!c) return 0;
  bool uns;
  return tail_shape_error(c, &uns) == nullptr ? 1 : 0;
}

extern "C" int dsr_conv_shuffle_add_fwd(const dsr_compact_tail* c, hipStream_t st) {
  DSR_REQUIRE(c, "conv_shuffle_add_fwd: null descriptor");
  DSR_REQUIRE(c->x && c->w && c->out, "conv_shuffle_add_fwd: null pointer (x, w or out)");
  bool uns;
  const char* err = tail_shape_error(c, &uns);
  if (err && uns) return dsr_fail(DSR_E_UNSUPPORTED, "conv_shuffle_add_fwd: %s", err);
  DSR_REQUIRE(!err, "conv_shuffle_add_fwd: %s", err);
  const size_t pix = (size_t)c->N * c->H * c->W;
  const size_t xb = pix * CP_CIN * 2, bb = pix * c->C * 4, ob = bb * c->s * c->s;
  DSR_REQUIRE(!ranges_overlap(c->x, xb, c->out, ob), "conv_shuffle_add_fwd: the output overlaps the input");
  DSR_REQUIRE(!c->base || !ranges_overlap(c->base, bb, c->out, ob), "conv_shuffle_add_fwd: the output overlaps base");
  CompactArgs a{};
  a.x = c->x;
  a.w = c->w;
  a.bias = c->bias;
  a.base = c->base;
  a.out = c->out;
  a.C = c->C;
  a.s = c->s;
  a.Q = c->C * c->s * c->s;
  a.R8 = (a.Q + 7) / 8 * 8;
  compact_fill(a, c->N, c->H, c->W);
  a.w_bytes = (unsigned)(9 * a.R8 * CP_CIN * 2);
  const int cap = c->max_blocks > 0 ? c->max_blocks : 256;
  const int blocks = a.ntiles < cap ? a.ntiles : cap;
  static LdsOptIn optin[4];
#define TAIL_LAUNCH(I, DTV, COUTV)                                                                                       \
  do {                                                                                                                   \
    optin[I].ensure((const void*)conv_compact_kernel<DTV, COUTV, true>, compact_lds<COUTV>());                           \
    hipLaunchKernelGGL((conv_compact_kernel<DTV, COUTV, true>), dim3(blocks), dim3(512), compact_lds<COUTV>(), st, a);   \
  } while (0)
  if (c->dtype == DSR_DTYPE_BF16) {
    if (a.Q > 32) TAIL_LAUNCH(0, DSR_DTYPE_BF16, 64);
    else TAIL_LAUNCH(1, DSR_DTYPE_BF16, 32);
  } else {
    if (a.Q > 32) TAIL_LAUNCH(2, DSR_DTYPE_F16, 64);
    else TAIL_LAUNCH(3, DSR_DTYPE_F16, 32);
  }
#undef TAIL_LAUNCH
  return dsr_launch_status("dsr_conv_shuffle_add_fwd");
}
