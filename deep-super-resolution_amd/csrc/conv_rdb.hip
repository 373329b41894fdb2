// Residual dense block (ESRGAN / Real-ESRGAN, models/GAN/rrdbnet.py) on a GROWTH BUFFER: one 3x3 / stride 1 / zero-pad 1
// convolution whose input is the channel prefix [0, Cin) of a 16-bit NHWC tensor [N][H][W][ldx] (ldx = 192 for the default
// model: the block input in [0, 64), x_k in [64 + 32 (k - 1), 64 + 32 k)) and whose 32 or 64 outputs are stored at a channel
// offset of a tensor with its own pixel stride.  conv1..4 of a block write the next 32 channels of the buffer they read --
// torch.cat((x, x1, ...)) costs nothing -- and conv5 writes the first 64 channels of the next block's buffer with
// x5 * 0.2 + x (and, for the third block of an RRDB, (...) * 0.2 + x_rrdb) folded into its epilogue, in fp32, one rounding.
//
// Structure of conv_halo64.hip (read that file's header first), with three changes:
//   * the halo addressing splits conv_halo64's CinP into the pixel stride ldx (addresses) and Cin / 32 (K-blocks);
//   * COUT is a template parameter: 64 = conv_halo64's wave layout (4 column strips of 16 pixels x 2 halves of 32 channels,
//     two 16-channel MFMA row blocks per wave); 32 = the same strips x 2 halves of 16 channels, ONE row block per wave (8
//     accumulators, 30 + 9 fragment reads for 72 MFMAs per K-block) and an 18 KB weight stage.  Other splits of the 32-output
//     form (over tile rows: 18 + 18 reads) have not been measured;
//   * the epilogue applies the residuals in the accumulators' register layout (a lane holds 4 consecutive channels of one
//     pixel: one 8-byte buffer load per residual), rounds once, and stores 64-byte (COUT = 32) or 128-byte (COUT = 64) pixel
//     segments at ldy pitch through the consumed halo stage.
// In place: halo reads touch bytes of channels [0, Cin) only, stores bytes of [y_off, y_off + COUT) only, and the entry point
// refuses y_off < Cin in the same tensor -- no byte is read and written by one launch, so there is no hand-off between blocks
// and no fence in here.  A 64-byte segment written next to segments other XCDs read leaves its L2 through byte-masked
// write-back; the next launch on the stream sees it by the ordinary kernel-boundary visibility ("Residual dense
// block on a growth buffer").
//
// INPUT-GRADIENT FORM (conv_rdb_kernel<DT, COUT, true>, dsr_conv_rdb_dgrad; the forward instantiations are the parent's
// code: `if constexpr` keeps every addition out of them).  A 3x3 / stride-1 input gradient is the same convolution with the
// mirrored taps and the transposed weights, so the kernel runs unchanged on the dgrad image [9][Cout][K] of
// dsr_conv_pack_weight (tap 8 - t in the loader's address), with
//   * an input channel OFFSET: the K = 32 | 64 channels [x_off, x_off + K) of dy (one or two K-blocks);
//   * Cout = 64 .. 192 outputs as Cout / COUT work items per tile (COUT = 64 where 64 divides Cout, else 32): the slices of
//     a tile are consecutive work items, so its halo is fetched from L2 again, not from HBM.  Staging the halo once and
//     looping over the slices inside a work item has not been measured;
//   * the epilogue  v = acc * gscale;  v += dx (the 16-bit value already in the range, `self_acc`);  below channel r1_lim
//     v = fmaf(g, beta1, v);  from channel mask_lo on  v *= (B >= 0 ? 1 : slope)  with B the block's forward buffer at the
//     same pixel and channel -- the LeakyReLU mask of the slice whose LAST contribution this launch stores (for a positive
//     slope the stored output carries the sign of its pre-activation; ConvAct's convention).  All of it in fp32 on fp32
//     accumulations of products of 16-bit operands; every store is ONE rounding to nearest even.
// In place, the rule that replaces "no byte is read and written by one launch": the OUTPUT bytes of a (tile, slice) are read
// (the addend) and then written by the one block that owns that work item, in its epilogue; halo reads -- the only reads of
// other blocks' pixels -- touch the other channel range [x_off, x_off + K) only, which no block writes (the entry point
// refuses dy == dx with x_off < Cout).  So there is still no hand-off between blocks and no fence.  No atomics anywhere.
#include <stdlib.h>

#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int RDB_TR = 8, RDB_TC = 64;                  // pixel tile
constexpr int RDB_HR = RDB_TR + 2, RDB_HP = RDB_TC + 2;  // halo rows, halo row pitch in pixels
constexpr int RDB_SLOTS = RDB_HR * RDB_HP;              // 660 pixel slots of 64 B
constexpr int RDB_HPIECES = (RDB_SLOTS + 15) / 16;      // 42 DMA pieces of 16 slots (1 KB)
constexpr int RDB_HALO = RDB_HPIECES * 1024;            // 43,008 B per halo stage

struct RdbArgs {
  const void* x;
  const void* w;
  const float* bias;
  void* y;
  const void* res1;
  const void* res2;
  int H, W, Cin, ldx, kblocks;
  int ldy, y_off, ldr1, r1_off, ldr2, r2_off;
  int act;
  float slope, beta1, beta2;
  int tiles_y, tiles_x, ntiles;
  unsigned w_bytes, x_img, y_img, r1_img, r2_img;       // bytes of the weight image and of ONE image of each tensor
  // input-gradient form only (BWD): the input is the channel range [x_off, x_off + Cin) and a work item is one of `nslices`
  // COUT-channel slices of one tile's output; rows of the dgrad image per tap; channels below r1_lim take res1; channels from
  // mask_lo on are multiplied by the LeakyReLU mask read from res2; `self_acc`: the output range is also the addend
  int x_off, nslices, w_rows, r1_lim, mask_lo, self_acc;
  float gscale;
};

template <int COUT>
constexpr int rdb_lds() {
  return 2 * RDB_HALO + 2 * (9 * COUT / 16) * 1024;     // 159,744 B (64 outputs) | 122,880 B (32)
}
}   // namespace

template <int DT, int COUT, bool BWD = false>
__global__ __launch_bounds__(512, 2) void conv_rdb_kernel(const RdbArgs a) {
  constexpr int NT = COUT / 32;                         // 16-channel MFMA row blocks per wave
  constexpr int WPIECES = 9 * COUT / 16;                // 36 | 18 pieces: 9 taps x COUT output channels x 64 B
  constexpr int WTS = WPIECES * 1024;
  constexpr int CSTRIDE = COUT * 2 + 16;                // staged C pixel pitch
  constexpr int VPP = COUT / 8;                         // 16-byte vectors per stored pixel segment
  constexpr int NIT = 4 * RDB_TC * VPP / 512;           // store iterations per 4-row half tile: 4 | 2
  static_assert(4 * RDB_TC * CSTRIDE <= RDB_HALO, "half a C tile is staged in one halo stage");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const sHalo = smem;
  unsigned char* const sWts = smem + 2 * RDB_HALO;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave & 3, wc = wave >> 2;              // 16-column strip, half of the output channels
  const int g = lane >> 4, r16 = lane & 15;
  const int chb = (COUT / 2) * wc;                      // this wave's first output channel
  constexpr unsigned OOB = 0xFFFFFFF0u;
  constexpr int FAR = 0x7FFFFF00;

  // ---- loader, halo: wave w issues the pieces w, w + 8, ... (< 42); lane l of piece p fills slot 16 p + l / 4, chunk l % 4
  constexpr int NHU = (RDB_HPIECES + 7) / 8;            // 6
  int h_part[NHU];                                      // ((hr * W + hc) * ldx + chunk * 8) * 2 of this lane's slot, FAR if none
  unsigned long long hc_pack = 0;                       // its halo column, 7 bits per piece
#pragma unroll
  for (int u = 0; u < NHU; ++u) {
    const int slot = 16 * (wave + 8 * u) + (lane >> 2);
    const int hr = slot / RDB_HP, hc = slot - hr * RDB_HP;
    h_part[u] = slot < RDB_SLOTS ? ((hr * a.W + hc) * a.ldx + (lane & 3) * 8) * 2 : FAR;
    hc_pack |= (unsigned long long)hc << (7 * u);
  }
  // ---- loader, weights: piece q = rows 16 q .. 16 q + 15 of the [9 * COUT] x 32 K-block slice (row = tap * COUT + channel)
  constexpr int NWU = (WPIECES + 7) / 8;                // 5 | 3
  int w_part[NWU];
#pragma unroll
  for (int v = 0; v < NWU; ++v) {
    const int row = 16 * (wave + 8 * v) + (lane >> 2);
    if constexpr (BWD) {
      // row tap * COUT + c of the stage is row (8 - tap) * w_rows + slice * COUT + c of the dgrad image [9][w_rows][Cin]: the
      // input gradient is the correlation with the mirrored kernel
      const int tap = row / COUT, c = row - tap * COUT;
      w_part[v] = (((8 - tap) * a.w_rows + c) * a.Cin + (lane & 3) * 8) * 2;
    } else {
      w_part[v] = (row * a.Cin + (lane & 3) * 8) * 2;
    }
  }
  const BufSrd wsrd = make_srd(a.w, a.w_bytes);
  const int per_img = a.tiles_y * a.tiles_x;

  struct TileXY {
    int n, ty, tx, sl;
  };
  auto decomp = [&](int t) {
    TileXY c;
    c.sl = 0;
    if constexpr (BWD) {                                // slices of one tile are consecutive work items: its halo stays in L2
      const int tile = t / a.nslices;
      c.sl = t - tile * a.nslices;
      t = tile;
    }
    c.n = t / per_img;
    const int rem = t - c.n * per_img;
    c.ty = rem / a.tiles_x;
    c.tx = rem - c.ty * a.tiles_x;
    return c;
  };
  auto fetch = [&](const TileXY& tc, int kb, int buf) {
    const int oy0 = tc.ty * RDB_TR - 1, ox0 = tc.tx * RDB_TC - 1;
    // per-image resource: halo rows above / below the image fall outside it and read as zeros
    const BufSrd xsrd = make_srd(reinterpret_cast<const unsigned char*>(a.x) + (size_t)tc.n * a.x_img, a.x_img);
    const int sbase = (oy0 * a.W + ox0) * a.ldx * 2 + kb * 64 + (BWD ? a.x_off * 2 : 0);
    const bool interior = ox0 >= 0 && ox0 + RDB_HP <= a.W;
    unsigned char* hdst = sHalo + buf * RDB_HALO;
#pragma unroll
    for (int u = 0; u < NHU; ++u) {
      if (wave + 8 * u >= RDB_HPIECES) continue;        // (wave-uniform; only the last round is partial)
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
      lds_dma16(wsrd, wdst + (wave + 8 * v) * 1024, (unsigned)(w_part[v] + kb * 64 + (BWD ? tc.sl * COUT * a.Cin * 2 : 0)));
    }
  };

  // fragment addresses: A (pixels) at halo slot (h, 16 wq + tx + r16), chunk g; B (weights) at row tap * COUT + chb + 16 nt + r16
  const int a_off = ((16 * wq + r16) * 64) + 16 * g;
  const int b_off = ((chb + r16) * 64) + 16 * g;

  // staged C: a lane writes its 4 channels of pixel (row, 16 wq + r16); thread tid then moves the 16-byte vectors tid + 512 it
  const int cw_base = (16 * wq + r16) * CSTRIDE + (chb + 4 * g) * 2;      // + (row & 3) * 64 * CSTRIDE + nt * 32

  const int tstep = gridDim.x;
  int t = blockIdx.x;
  if (t >= a.ntiles) return;
  TileXY cur = decomp(t);
  const int KB = a.kblocks;
  fetch(cur, 0, 0);
  int buf = 0;
  const float slope = a.slope;
  const bool leaky = !BWD && a.act == DSR_ACT_LEAKY;

  for (; t < a.ntiles; t += tstep) {
    const bool has_next = t + tstep < a.ntiles;
    const TileXY nxt = has_next ? decomp(t + tstep) : cur;
    f32x4 acc[RDB_TR][NT];
#pragma unroll
    for (int i = 0; i < RDB_TR; ++i)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (!BWD && a.bias) {
#pragma unroll
          for (int r = 0; r < 4; ++r) bv[r] = a.bias[chb + 16 * nt + 4 * g + r];
        }
        acc[i][nt] = f32x4{bv[0], bv[1], bv[2], bv[3]};
      }
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
      const unsigned char* sX = sHalo + buf * RDB_HALO + a_off;
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
        auto load = [&](int h) { return *reinterpret_cast<const U4*>(sX + (h * RDB_HP + tx) * 64); };
        fa[0] = load(0);
        fa[1] = load(1);
#pragma unroll
        for (int h = 0; h < RDB_HR; ++h) {
          if (h + 2 < RDB_HR) fa[(h + 2) % 3] = load(h + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ty = 0; ty < 3; ++ty) {
            const int i = h - ty;
            if (i < 0 || i >= RDB_TR) continue;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[i][nt] = mfma16<DT>(fb[ty][nt], fa[h % 3], acc[i][nt]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (tx == 0 && late) prefetch();
      }
    }
    // ---- epilogue: the stage just consumed (buf ^ 1 after the loop's flip) becomes the C staging area; the DMA in flight
    // targets the other stage.  Two halves of 4 rows x 64 pixels.
    unsigned char* sC = sHalo + (buf ^ 1) * RDB_HALO;
    const int oy0 = cur.ty * RDB_TR, ox0 = cur.tx * RDB_TC;
    unsigned char* const yimg = reinterpret_cast<unsigned char*>(a.y) + (size_t)cur.n * a.y_img;
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(yimg, 0, a.y_img, 0x00020000);
    const void* const r1p = a.res1 ? a.res1 : a.y;      // (never dereferenced without its flag)
    const void* const r2p = a.res2 ? a.res2 : a.y;
    const __amdgpu_buffer_rsrc_t r1rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(r1p)) + (size_t)cur.n * a.r1_img, 0, a.r1_img, 0x00020000);
    const __amdgpu_buffer_rsrc_t r2rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(r2p)) + (size_t)cur.n * a.r2_img, 0, a.r2_img, 0x00020000);
    const int px = ox0 + 16 * wq + r16;                 // this lane's pixel column
    const int ych = a.y_off + (BWD ? cur.sl * COUT : 0);  // first channel of the stored range
    auto residual = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned off, float beta, float* v) {
      typedef __attribute__((ext_vector_type(2))) unsigned U2;
      const U2 rv = __builtin_bit_cast(U2, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
      v[0] = fmaf(v[0], beta, h2f<DT>((unsigned short)(rv.x & 0xffff)));
      v[1] = fmaf(v[1], beta, h2f<DT>((unsigned short)(rv.x >> 16)));
      v[2] = fmaf(v[2], beta, h2f<DT>((unsigned short)(rv.y & 0xffff)));
      v[3] = fmaf(v[3], beta, h2f<DT>((unsigned short)(rv.y >> 16)));
    };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      __builtin_amdgcn_s_barrier();          // every wave is done reading the stage (half 0) / the staged half (half 1)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int i = half * 4 + ii;
        const int py = oy0 + i;
        const bool inside = py < a.H && px < a.W;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float s = acc[i][nt][r];
            v[r] = leaky ? (s >= 0.f ? s : s * slope) : s;
          }
          const int c0 = chb + 16 * nt + 4 * g;
          if constexpr (BWD) {
            // v = acc * gscale (+ what the range holds) (+ beta1 * res1 below channel r1_lim), times the mask from mask_lo on:
            // all in fp32, one rounding below.  The addend is read by the block that owns the tile, before it stores it.
            typedef __attribute__((ext_vector_type(2))) unsigned U2;
            const unsigned pix = inside ? (unsigned)(py * a.W + px) : 0u;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= a.gscale;
            if (a.self_acc) {
              const unsigned off = inside ? (pix * a.ldy + ych + c0) * 2 : OOB;
              const U2 rv = __builtin_bit_cast(U2, __builtin_amdgcn_raw_buffer_load_b64(yrsrc, off, 0, 0));
              v[0] += h2f<DT>((unsigned short)(rv.x & 0xffff));
              v[1] += h2f<DT>((unsigned short)(rv.x >> 16));
              v[2] += h2f<DT>((unsigned short)(rv.y & 0xffff));
              v[3] += h2f<DT>((unsigned short)(rv.y >> 16));
            }
            const int cabs = ych + c0;
            if (a.res1 && cabs < a.r1_lim) {
              const unsigned off = inside ? (pix * a.ldr1 + a.r1_off + cabs) * 2 : OOB;
              const U2 rv = __builtin_bit_cast(U2, __builtin_amdgcn_raw_buffer_load_b64(r1rsrc, off, 0, 0));
              v[0] = fmaf(h2f<DT>((unsigned short)(rv.x & 0xffff)), a.beta1, v[0]);
              v[1] = fmaf(h2f<DT>((unsigned short)(rv.x >> 16)), a.beta1, v[1]);
              v[2] = fmaf(h2f<DT>((unsigned short)(rv.y & 0xffff)), a.beta1, v[2]);
              v[3] = fmaf(h2f<DT>((unsigned short)(rv.y >> 16)), a.beta1, v[3]);
            }
            if (a.res2 && cabs >= a.mask_lo) {
              const unsigned off = inside ? (pix * a.ldr2 + a.r2_off + cabs) * 2 : OOB;
              const U2 rv = __builtin_bit_cast(U2, __builtin_amdgcn_raw_buffer_load_b64(r2rsrc, off, 0, 0));
              // (the stored activation carries the sign of its pre-activation for a positive slope; -0.0 counts as >= 0)
              v[0] *= h2f<DT>((unsigned short)(rv.x & 0xffff)) >= 0.f ? 1.f : slope;
              v[1] *= h2f<DT>((unsigned short)(rv.x >> 16)) >= 0.f ? 1.f : slope;
              v[2] *= h2f<DT>((unsigned short)(rv.y & 0xffff)) >= 0.f ? 1.f : slope;
              v[3] *= h2f<DT>((unsigned short)(rv.y >> 16)) >= 0.f ? 1.f : slope;
            }
          }
          if (!BWD && a.res1) {
            const unsigned off = inside ? (unsigned)(((py * a.W + px) * a.ldr1 + a.r1_off + c0) * 2) : OOB;
            residual(r1rsrc, off, a.beta1, v);
          }
          if (!BWD && a.res2) {
            const unsigned off = inside ? (unsigned)(((py * a.W + px) * a.ldr2 + a.r2_off + c0) * 2) : OOB;
            residual(r2rsrc, off, a.beta2, v);
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
        unsigned off = (unsigned)(((sy * a.W + sx) * a.ldy + ych) * 2 + chunk * 16);
        if (!(sy < a.H && sx < a.W)) off = OOB;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), yrsrc, off, 0, 0);
      }
    }
    cur = nxt;
  }
}

template <int DT>
__global__ __launch_bounds__(256) void scale_add16_kernel(const U4* __restrict__ a, float beta, const U4* __restrict__ b,
                                                          U4* __restrict__ out, size_t nvec) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += step) {
    float fa[8], fb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unpack8<DT>(a[i], fa);
    if (b) unpack8<DT>(b[i], fb);
#pragma unroll
    for (int k = 0; k < 8; ++k) fa[k] = fmaf(fa[k], beta, fb[k]);
    out[i] = pack8<DT>(fa);
  }
}

// ---- host side
static bool rdb_mult32(int v) { return v > 0 && v % 32 == 0; }

// shape fields only (no pointers): 0 = fine, else the reason
static const char* rdb_shape_error(const dsr_rdb_conv* c) {
  if (!DSR_DTYPE_OK(c->dtype)) return "dtype is neither DSR_BF16 nor DSR_F16";
  if (c->N < 1 || c->H < 1 || c->W < 1) return "N, H, W must be positive";
  if (c->Cout != 32 && c->Cout != 64) return "Cout must be 32 or 64";
  if (!rdb_mult32(c->Cin) || c->Cin > 1024) return "Cin must be a multiple of 32 in 32..1024";
  if (!rdb_mult32(c->ldx) || c->Cin > c->ldx) return "ldx must be a multiple of 32 and >= Cin";
  if (!rdb_mult32(c->ldy) || c->y_off < 0 || c->y_off % 32) return "ldy / y_off must be multiples of 32 channels";
  if (c->y_off + c->Cout > c->ldy) return "y_off + Cout > ldy";
  if (c->act != DSR_ACT_NONE && !(c->act == DSR_ACT_LEAKY && c->slope > 0.f)) return "act must be none or LeakyReLU with slope > 0";
  const size_t pix = (size_t)c->H * c->W;
  int ld_max = c->ldx > c->ldy ? c->ldx : c->ldy;
  if (c->res1 && c->ldr1 > ld_max) ld_max = c->ldr1;
  if (c->res2 && c->ldr2 > ld_max) ld_max = c->ldr2;
  if (pix * ld_max * 2 >= 0x7FFFFF00ull) return "a tensor of 2^31 bytes or more per image";
  if (pix * ld_max * 2 * c->N >= 0x100000000ull) return "a tensor of 2^32 bytes or more";
  return nullptr;
}

extern "C" int dsr_conv_rdb_supported(const dsr_rdb_conv* c) {
  if (!c) return 0;
  return rdb_shape_error(c) == nullptr ? 1 : 0;
}

static const char* rdb_residual_error(const dsr_rdb_conv* c, const void* res, int ldr, int r_off) {
  if (!res) return nullptr;
  if (!rdb_mult32(ldr) || r_off < 0 || r_off % 32) return "residual stride / offset must be multiples of 32 channels";
  if (r_off + c->Cout > ldr) return "residual offset + Cout > its stride";
  if (res == c->y && r_off < c->y_off + c->Cout && c->y_off < r_off + c->Cout) return "the output range overlaps a residual range of the same tensor";
  return nullptr;
}

extern "C" int dsr_conv_rdb_fwd(const dsr_rdb_conv* c, hipStream_t st) {
  DSR_REQUIRE(c, "conv_rdb_fwd: null descriptor");
  DSR_REQUIRE(c->x && c->w && c->y, "conv_rdb_fwd: null pointer (x, w or y)");
  const char* err = rdb_shape_error(c);
  DSR_REQUIRE(!err, "conv_rdb_fwd: %s", err);
  err = rdb_residual_error(c, c->res1, c->ldr1, c->r1_off);
  if (!err) err = rdb_residual_error(c, c->res2, c->ldr2, c->r2_off);
  DSR_REQUIRE(!err, "conv_rdb_fwd: %s", err);
  DSR_REQUIRE(!(c->y == c->x && c->y_off < c->Cin), "conv_rdb_fwd: the output range overlaps the input prefix (y == x and y_off %d < Cin %d)",
              c->y_off, c->Cin);
  RdbArgs a{};
  a.x = c->x;
  a.w = c->w;
  a.bias = c->bias;
  a.y = c->y;
  a.res1 = c->res1;
  a.res2 = c->res2;
  a.H = c->H;
  a.W = c->W;
  a.Cin = c->Cin;
  a.ldx = c->ldx;
  a.kblocks = c->Cin / 32;
  a.ldy = c->ldy;
  a.y_off = c->y_off;
  a.ldr1 = c->res1 ? c->ldr1 : 0;
  a.r1_off = c->res1 ? c->r1_off : 0;
  a.ldr2 = c->res2 ? c->ldr2 : 0;
  a.r2_off = c->res2 ? c->r2_off : 0;
  a.act = c->act;
  a.slope = c->slope;
  a.beta1 = c->beta1;
  a.beta2 = c->beta2;
  a.tiles_y = (c->H + RDB_TR - 1) / RDB_TR;
  a.tiles_x = (c->W + RDB_TC - 1) / RDB_TC;
  a.ntiles = c->N * a.tiles_y * a.tiles_x;
  const size_t pix = (size_t)c->H * c->W;
  a.w_bytes = (unsigned)(9 * c->Cout * c->Cin * 2);
  a.x_img = (unsigned)(pix * c->ldx * 2);
  a.y_img = (unsigned)(pix * c->ldy * 2);
  a.r1_img = (unsigned)(pix * a.ldr1 * 2);
  a.r2_img = (unsigned)(pix * a.ldr2 * 2);
  int cap = c->max_blocks > 0 ? c->max_blocks : 256;    // persistent: one 8-wave block per CU
  const int blocks = a.ntiles < cap ? a.ntiles : cap;
  static LdsOptIn optin[4];
#define RDB_LAUNCH(I, DTV, COUTV)                                                                             \
  do {                                                                                                        \
    optin[I].ensure((const void*)conv_rdb_kernel<DTV, COUTV>, rdb_lds<COUTV>());                              \
    hipLaunchKernelGGL((conv_rdb_kernel<DTV, COUTV>), dim3(blocks), dim3(512), rdb_lds<COUTV>(), st, a);      \
  } while (0)
  if (c->dtype == DSR_DTYPE_BF16) {
    if (c->Cout == 64) RDB_LAUNCH(0, DSR_DTYPE_BF16, 64);
    else RDB_LAUNCH(1, DSR_DTYPE_BF16, 32);
  } else {
    if (c->Cout == 64) RDB_LAUNCH(2, DSR_DTYPE_F16, 64);
    else RDB_LAUNCH(3, DSR_DTYPE_F16, 32);
  }
#undef RDB_LAUNCH
  return dsr_launch_status("dsr_conv_rdb_fwd");
}

// ---- input gradient on growth buffers
static const char* rdb_dgrad_shape_error(const dsr_rdb_dgrad* c) {
  if (!DSR_DTYPE_OK(c->dtype)) return "dtype is neither DSR_BF16 nor DSR_F16";
  if (c->N < 1 || c->H < 1 || c->W < 1) return "N, H, W must be positive";
  if (c->K != 32 && c->K != 64) return "K must be 32 or 64";
  if (!rdb_mult32(c->Cout) || c->Cout > 1024) return "Cout must be a multiple of 32 in 32..1024";
  if (!rdb_mult32(c->lddy) || c->dy_off < 0 || c->dy_off % 32 || c->dy_off + c->K > c->lddy) return "lddy / dy_off: multiples of 32 with dy_off + K <= lddy";
  if (!rdb_mult32(c->lddx) || c->Cout > c->lddx) return "lddx must be a multiple of 32 and >= Cout";
  if (c->g_limit < 0 || c->g_limit % 32 || c->g_limit > c->Cout) return "g_limit must be a multiple of 32 in 0..Cout";
  if (c->g_limit && (!rdb_mult32(c->ldg) || c->g_limit > c->ldg)) return "ldg must be a multiple of 32 and >= g_limit";
  if (c->mask_lo < 0 || c->mask_lo % 32 || c->mask_lo > c->Cout) return "mask_lo must be a multiple of 32 in 0..Cout";
  if (c->mask_lo < c->Cout && (!rdb_mult32(c->ldact) || c->Cout > c->ldact || !(c->slope > 0.f))) return "ldact must be a multiple of 32 and >= Cout, slope > 0";
  const size_t pix = (size_t)c->H * c->W;
  int ld_max = c->lddy > c->lddx ? c->lddy : c->lddx;
  if (c->g_limit && c->ldg > ld_max) ld_max = c->ldg;
  if (c->mask_lo < c->Cout && c->ldact > ld_max) ld_max = c->ldact;
  if (pix * ld_max * 2 >= 0x7FFFFF00ull) return "a tensor of 2^31 bytes or more per image";
  if (pix * ld_max * 2 * c->N >= 0x100000000ull) return "a tensor of 2^32 bytes or more";
  return nullptr;
}

extern "C" int dsr_conv_rdb_dgrad_supported(const dsr_rdb_dgrad* c) {
  if (!c) return 0;
  return rdb_dgrad_shape_error(c) == nullptr ? 1 : 0;
}

extern "C" int dsr_conv_rdb_dgrad(const dsr_rdb_dgrad* c, hipStream_t st) {
  DSR_REQUIRE(c, "conv_rdb_dgrad: null descriptor");
  DSR_REQUIRE(c->dy && c->wd && c->dx, "conv_rdb_dgrad: null pointer (dy, wd or dx)");
  const char* err = rdb_dgrad_shape_error(c);
  DSR_REQUIRE(!err, "conv_rdb_dgrad: %s", err);
  DSR_REQUIRE(!c->g_limit || c->g, "conv_rdb_dgrad: g_limit > 0 without g");
  DSR_REQUIRE(c->mask_lo >= c->Cout || c->act_out, "conv_rdb_dgrad: mask_lo < Cout without act_out");
  DSR_REQUIRE(!(c->dy == c->dx && c->dy_off < c->Cout), "conv_rdb_dgrad: the output range overlaps the input range (dy == dx and dy_off %d < Cout %d)",
              c->dy_off, c->Cout);
  DSR_REQUIRE(!(c->g_limit && c->g == c->dx) && !(c->mask_lo < c->Cout && c->act_out == c->dx), "conv_rdb_dgrad: g / act_out must not be the output tensor");
  const int cout = c->Cout % 64 == 0 ? 64 : 32;         // channels per work item
  RdbArgs a{};
  a.x = c->dy;
  a.w = c->wd;
  a.y = c->dx;
  a.res1 = c->g_limit ? c->g : nullptr;
  a.res2 = c->mask_lo < c->Cout ? c->act_out : nullptr;
  a.H = c->H;
  a.W = c->W;
  a.Cin = c->K;
  a.ldx = c->lddy;
  a.kblocks = c->K / 32;
  a.ldy = c->lddx;
  a.y_off = 0;
  a.ldr1 = a.res1 ? c->ldg : 0;
  a.ldr2 = a.res2 ? c->ldact : 0;
  a.act = DSR_ACT_NONE;
  a.slope = c->slope;
  a.beta1 = c->g_scale;
  a.tiles_y = (c->H + RDB_TR - 1) / RDB_TR;
  a.tiles_x = (c->W + RDB_TC - 1) / RDB_TC;
  a.nslices = c->Cout / cout;
  a.ntiles = c->N * a.tiles_y * a.tiles_x * a.nslices;
  const size_t pix = (size_t)c->H * c->W;
  a.w_bytes = (unsigned)(9 * c->Cout * c->K * 2);
  a.x_img = (unsigned)(pix * c->lddy * 2);
  a.y_img = (unsigned)(pix * c->lddx * 2);
  a.r1_img = (unsigned)(pix * a.ldr1 * 2);
  a.r2_img = (unsigned)(pix * a.ldr2 * 2);
  a.x_off = c->dy_off;
  a.w_rows = c->Cout;
  a.r1_lim = c->g_limit;
  a.mask_lo = c->mask_lo;
  a.self_acc = c->accumulate ? 1 : 0;
  a.gscale = c->scale;
  int cap = c->max_blocks > 0 ? c->max_blocks : 256;
  const int blocks = a.ntiles < cap ? a.ntiles : cap;
  static LdsOptIn optin[4];
#define RDB_LAUNCH(I, DTV, COUTV)                                                                                   \
  do {                                                                                                              \
    optin[I].ensure((const void*)conv_rdb_kernel<DTV, COUTV, true>, rdb_lds<COUTV>());                              \
    hipLaunchKernelGGL((conv_rdb_kernel<DTV, COUTV, true>), dim3(blocks), dim3(512), rdb_lds<COUTV>(), st, a);      \
  } while (0)
  if (c->dtype == DSR_DTYPE_BF16) {
    if (cout == 64) RDB_LAUNCH(0, DSR_DTYPE_BF16, 64);
    else RDB_LAUNCH(1, DSR_DTYPE_BF16, 32);
  } else {
    if (cout == 64) RDB_LAUNCH(2, DSR_DTYPE_F16, 64);
    else RDB_LAUNCH(3, DSR_DTYPE_F16, 32);
  }
#undef RDB_LAUNCH
  return dsr_launch_status("dsr_conv_rdb_dgrad");
}

extern "C" int dsr_scale_add16(int dtype, const void* a, float beta, const void* b, void* out, size_t nvec, hipStream_t st) {
  DSR_REQUIRE(a && out && DSR_DTYPE_OK(dtype) && nvec > 0, "scale_add16: null pointer, bad dtype or empty");
  const size_t want = (nvec + 255) / 256;
  const unsigned blocks = (unsigned)(want > 8192 ? 8192 : want);
  if (dtype == DSR_DTYPE_BF16)
    hipLaunchKernelGGL((scale_add16_kernel<DSR_DTYPE_BF16>), dim3(blocks), dim3(256), 0, st, (const U4*)a, beta, (const U4*)b, (U4*)out, nvec);
  else
    hipLaunchKernelGGL((scale_add16_kernel<DSR_DTYPE_F16>), dim3(blocks), dim3(256), 0, st, (const U4*)a, beta, (const U4*)b, (U4*)out, nvec);
  return dsr_launch_status("dsr_scale_add16");
}
