// Backward of a residual dense block ON ITS GROWTH BUFFERS (models/GAN/rrdbnet.py with fused_training; forward and the
// input-gradient kernel: conv_rdb.hip).  This file: the weight and bias gradients of the five convolutions of one block.
//
// When dgrad_2 has run, channels [64, 192) of the gradient buffer G hold the final dY_1 .. dY_4 (already multiplied by the
// LeakyReLU masks, conv_rdb.hip) and the block's buffer B holds every convolution's input as a channel prefix.  So
//   * launch A forms dW_1..4 as ONE block-triangular problem, 128 output x 192 input channels: conv_wgrad_dma_body
//     (conv_wgrad_tile.hip: pixels are the contraction index, ds_read_b64_tr_b16 fragments, all nine taps from one staged halo)
//     with pixel strides and channel offsets of its own, over the five 64 x 64 channel pairs that hold a weight -- the pair
//     (dY_1..2, B[128:192]) holds none and gets no block.  Entries of a computed pair that belong to no weight (dY_1 against
//     B[64:128], say) are formed and never read;
//   * launch B forms dW_5 from the dense dL/dout (three pairs); dY_5 = gscale * g enters as a factor of the fold;
//   * rdb_colsum_kernel sums dY_1..4 and g over the pixels (the bias gradients: a pass of its own, 192 columns);
//   * rdb_wgrad_fold_kernel adds the per-chunk slabs and the column-sum rows IN CHUNK ORDER and writes the ten fp32
//     gradients in PyTorch's layouts.  Nothing outside them is written: a structurally zero (co, ci) pair has no address.
// The pixel range is cut into chunks of at least RDB_WGRAD_MIN_TILES tiles (2 rows x 32 columns each); products of 16-bit
// operands are accumulated in fp32, every cross-chunk sum is a loop in a fixed order, there is no atomic: two runs give the
// same bits.
#include "../../include/dsr_hip.h"
#include "dsr_common.h"
#include "dsr_kernels.h"

namespace {
constexpr int RDB_F = 64, RDB_G = 32, RDB_LD = RDB_F + 4 * RDB_G;   // the only channel counts taken
constexpr int RDB_WGRAD_MIN_TILES = 8;                              // tiles per chunk below which the pixel range is not split
constexpr int RDB_WGRAD_WANT = 64;                                  // chunks aimed at: 8 pairs x 64 = two 4-wave blocks per CU
constexpr int RDB_COLSUM_ROWS = 256, RDB_COLSUM_PHASES = 4;

struct RdbWgradPlan {
  int tiles_y, tiles_x, ntiles, tiles_per_block, chunks;
  int cs_rows, cs_ppb;                                              // column sums: rows of the partial, pixels per block
  size_t off_b, off_cs, bytes;                                      // byte offsets of launch B's slabs and the column-sum rows
};

RdbWgradPlan rdb_wgrad_plan(int N, int H, int W) {
  RdbWgradPlan p;
  p.tiles_y = (H + 1) / 2;
  p.tiles_x = (W + 31) / 32;
  p.ntiles = N * p.tiles_y * p.tiles_x;
  int tpb = (p.ntiles + RDB_WGRAD_WANT - 1) / RDB_WGRAD_WANT;
  if (tpb < RDB_WGRAD_MIN_TILES) tpb = RDB_WGRAD_MIN_TILES;
  p.tiles_per_block = tpb;
  p.chunks = (p.ntiles + tpb - 1) / tpb;
  const size_t pix = (size_t)N * H * W;
  p.cs_ppb = (int)((pix + RDB_COLSUM_ROWS - 1) / RDB_COLSUM_ROWS);
  if (p.cs_ppb < 64) p.cs_ppb = 64;
  p.cs_rows = (int)((pix + p.cs_ppb - 1) / p.cs_ppb);
  p.off_b = (size_t)p.chunks * 9 * (4 * RDB_G) * RDB_LD * sizeof(float);
  p.off_cs = p.off_b + (size_t)p.chunks * 9 * RDB_F * RDB_LD * sizeof(float);
  p.bytes = p.off_cs + (size_t)p.cs_rows * RDB_LD * sizeof(float);
  return p;
}

struct RdbFoldArgs {
  const float* pa;      // [chunks][9][128][192]
  const float* pb;      // [chunks][9][64][192]
  const float* cs;      // [cs_rows][192]: columns 0..127 = dY_1..4, 128..191 = g
  float* dw[5];
  float* db[5];
  int chunks, cs_rows;
  float gscale;
};
}   // namespace

// part[b][c] = sum over the pixels of block b of dY_1..4 (c < 128: channel 64 + c of dy) or g (channel c - 128); four pixel
// phases per block, folded through LDS in phase order.
template <int DT>
__global__ __launch_bounds__(RDB_LD* RDB_COLSUM_PHASES) void rdb_colsum_kernel(const unsigned short* __restrict__ dy, int lddy,
                                                                               const unsigned short* __restrict__ g, int ldg,
                                                                               size_t pix, int ppb, float* __restrict__ part) {
  __shared__ float s[RDB_COLSUM_PHASES][RDB_LD];
  const int c = threadIdx.x % RDB_LD, q = threadIdx.x / RDB_LD;
  const unsigned short* src = c < 4 * RDB_G ? dy + RDB_F + c : g + (c - 4 * RDB_G);
  const size_t ld = c < 4 * RDB_G ? (size_t)lddy : (size_t)ldg;
  const size_t p0 = (size_t)blockIdx.x * ppb;
  size_t p1 = p0 + ppb;
  if (p1 > pix) p1 = pix;
  float acc = 0.f;
  for (size_t p = p0 + q; p < p1; p += RDB_COLSUM_PHASES) acc += h2f<DT>(src[p * ld]);
  s[q][c] = acc;
  __syncthreads();
  if (q == 0) {
    float v = s[0][c];
#pragma unroll
    for (int i = 1; i < RDB_COLSUM_PHASES; ++i) v += s[i][c];
    part[(size_t)blockIdx.x * RDB_LD + c] = v;
  }
}

// One thread per element of the slabs' [9][192 rows][192] index space (rows 0..127: launch A, 128..191: launch B); the last
// block folds the column sums.
__global__ __launch_bounds__(256) void rdb_wgrad_fold_kernel(const RdbFoldArgs a) {
  constexpr int ROWS = 4 * RDB_G + RDB_F;
  constexpr int TOTAL = 9 * ROWS * RDB_LD;
  if (blockIdx.x == gridDim.x - 1) {
    const int c = threadIdx.x;
    if (c >= ROWS) return;
    const int k = c < 4 * RDB_G ? c / RDB_G : 4;
    float* const db = a.db[k];
    if (!db) return;
    float v = 0.f;
    for (int r = 0; r < a.cs_rows; ++r) v += a.cs[(size_t)r * RDB_LD + c];
    if (k == 4) db[c - 4 * RDB_G] = v * a.gscale;
    else db[c - k * RDB_G] = v;
    return;
  }
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= TOTAL) return;
  const int ci = idx % RDB_LD;
  const int row = (idx / RDB_LD) % ROWS;
  const int t = idx / (RDB_LD * ROWS);
  if (row < 4 * RDB_G) {
    const int k = row / RDB_G, cin = RDB_F + k * RDB_G;
    float* const dw = a.dw[k];
    if (ci >= cin || !dw) return;                       // (no weight lives here)
    const size_t slab = (size_t)9 * 4 * RDB_G * RDB_LD;
    const float* p = a.pa + ((size_t)t * 4 * RDB_G + row) * RDB_LD + ci;
    float v = 0.f;
    for (int c = 0; c < a.chunks; ++c) v += p[c * slab];
    dw[((size_t)(row - k * RDB_G) * cin + ci) * 9 + t] = v;
  } else {
    float* const dw = a.dw[4];
    if (!dw) return;
    const int co = row - 4 * RDB_G;
    const size_t slab = (size_t)9 * RDB_F * RDB_LD;
    const float* p = a.pb + ((size_t)t * RDB_F + co) * RDB_LD + ci;
    float v = 0.f;
    for (int c = 0; c < a.chunks; ++c) v += p[c * slab];
    dw[((size_t)co * RDB_LD + ci) * 9 + t] = v * a.gscale;
  }
}

// ---- host side
static const char* rdb_wgrad_shape_error(const dsr_rdb_wgrad* c) {
  if (!DSR_DTYPE_OK(c->dtype)) return "dtype is neither DSR_BF16 nor DSR_F16";
  if (c->N < 1 || c->H < 1 || c->W < 1) return "N, H, W must be positive";
  if (c->ldx != RDB_LD || c->lddy != RDB_LD) return "the buffers of x and dy must have 192 channels (num_feat 64, num_grow_ch 32)";
  if (c->ldg < RDB_F || c->ldg % 32) return "ldg must be a multiple of 32 and >= 64";
  const size_t pix = (size_t)c->H * c->W;
  const int ld_max = c->ldg > RDB_LD ? c->ldg : RDB_LD;
  if (pix * ld_max * 2 >= 0x7FFFFF00ull) return "a tensor of 2^31 bytes or more per image";
  if (pix * ld_max * 2 * c->N >= 0x100000000ull) return "a tensor of 2^32 bytes or more";
  return nullptr;
}

extern "C" int dsr_conv_rdb_wgrad_supported(const dsr_rdb_wgrad* c) {
  if (!c) return 0;
  return rdb_wgrad_shape_error(c) == nullptr ? 1 : 0;
}

extern "C" size_t dsr_conv_rdb_wgrad_workspace(const dsr_rdb_wgrad* c) {
  if (!c || rdb_wgrad_shape_error(c)) return 0;
  return rdb_wgrad_plan(c->N, c->H, c->W).bytes;
}

extern "C" int dsr_conv_rdb_wgrad_chunks(const dsr_rdb_wgrad* c) {
  if (!c || rdb_wgrad_shape_error(c)) return 0;
  return rdb_wgrad_plan(c->N, c->H, c->W).chunks;
}

extern "C" int dsr_conv_rdb_wgrad(const dsr_rdb_wgrad* c, void* workspace, size_t workspace_bytes, hipStream_t st) {
  DSR_REQUIRE(c, "conv_rdb_wgrad: null descriptor");
  DSR_REQUIRE(c->x && c->dy && c->g, "conv_rdb_wgrad: null pointer (x, dy or g)");
  const char* err = rdb_wgrad_shape_error(c);
  DSR_REQUIRE(!err, "conv_rdb_wgrad: %s", err);
  const RdbWgradPlan p = rdb_wgrad_plan(c->N, c->H, c->W);
  DSR_REQUIRE(workspace && ((size_t)workspace & 15) == 0, "conv_rdb_wgrad: the workspace must be a 16-byte aligned device pointer");
  if (workspace_bytes < p.bytes) return dsr_fail(DSR_E_WORKSPACE, "conv_rdb_wgrad: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
  for (int k = 0; k < 5; ++k)
    DSR_REQUIRE(((size_t)c->dw[k] & 3) == 0 && ((size_t)c->db[k] & 3) == 0, "conv_rdb_wgrad: dw / db must be 4-byte aligned");
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  const size_t pix = (size_t)c->N * c->H * c->W;

  WgradRdbArgs a{};
  a.x = c->x;
  a.N = c->N;
  a.OH = a.IH = c->H;
  a.OW = a.IW = c->W;
  a.CinP = RDB_LD;
  a.pad = 1;
  a.pad_mode = DSR_PAD_ZERO;
  a.tiles_ci = RDB_LD / 64;
  a.tiles_y = p.tiles_y;
  a.tiles_x = p.tiles_x;
  a.ntiles = p.ntiles;
  a.tiles_per_block = p.tiles_per_block;
  a.ldx = RDB_LD;
  a.x_off = 0;
  a.x_bytes = (unsigned)(pix * RDB_LD * 2);
  const bool any14 = c->dw[0] || c->dw[1] || c->dw[2] || c->dw[3];
  if (any14) {
    // launch A: dY_1..4 = channels [64, 192) of dy against B's prefix; pairs (co tile, ci tile) = (0,0) (0,1) (1,0) (1,1) (1,2)
    a.dy = c->dy;
    a.partial = reinterpret_cast<float*>(ws);
    a.CoutP = 4 * RDB_G;
    a.tiles_co = 2;
    a.ldy = RDB_LD;
    a.y_off = RDB_F;
    a.dy_bytes = a.x_bytes;
    a.pair_map = 0x54310u;
    dsr_launch_wgrad_rdb(a, 5, p.chunks, c->dtype, st);
  }
  if (c->dw[4]) {
    a.dy = c->g;
    a.partial = reinterpret_cast<float*>(ws + p.off_b);
    a.CoutP = RDB_F;
    a.tiles_co = 1;
    a.ldy = c->ldg;
    a.y_off = 0;
    a.dy_bytes = (unsigned)(pix * c->ldg * 2);
    a.pair_map = 0x210u;
    dsr_launch_wgrad_rdb(a, 3, p.chunks, c->dtype, st);
  }
  const bool any_db = c->db[0] || c->db[1] || c->db[2] || c->db[3] || c->db[4];
  float* const cs = reinterpret_cast<float*>(ws + p.off_cs);
  if (any_db) {
    const dim3 block(RDB_LD * RDB_COLSUM_PHASES);
    if (c->dtype == DSR_DTYPE_BF16)
      hipLaunchKernelGGL((rdb_colsum_kernel<DSR_DTYPE_BF16>), dim3(p.cs_rows), block, 0, st, (const unsigned short*)c->dy, c->lddy,
                         (const unsigned short*)c->g, c->ldg, pix, p.cs_ppb, cs);
    else
      hipLaunchKernelGGL((rdb_colsum_kernel<DSR_DTYPE_F16>), dim3(p.cs_rows), block, 0, st, (const unsigned short*)c->dy, c->lddy,
                         (const unsigned short*)c->g, c->ldg, pix, p.cs_ppb, cs);
  }
  if (any14 || c->dw[4] || any_db) {
    RdbFoldArgs f{};
    f.pa = reinterpret_cast<const float*>(ws);
    f.pb = reinterpret_cast<const float*>(ws + p.off_b);
    f.cs = cs;
    for (int k = 0; k < 5; ++k) {
      f.dw[k] = c->dw[k];
      f.db[k] = c->db[k];
    }
    f.chunks = p.chunks;
    f.cs_rows = p.cs_rows;
    f.gscale = c->gscale;
    const int blocks = (9 * RDB_LD * RDB_LD + 255) / 256 + 1;
    hipLaunchKernelGGL(rdb_wgrad_fold_kernel, dim3(blocks), dim3(256), 0, st, f);
  }
  return dsr_launch_status("dsr_conv_rdb_wgrad");
}
