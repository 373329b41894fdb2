// Many small tensors behind one launch: the scheme of the multi-tensor Adam, weight repack, overflow check, gradient norm,
// EMA and L-BFGS gather / combine kernels.  A launch carries a by-value group struct (kernel arguments are limited to 4 KB,
// hence at most DSR_MT_MAX tensors): the family's own payload arrays (pointers, sizes, flags) plus one MtTable.  Every tensor
// is cut into chunks of a fixed number of elements, one block each, the blocks of a tensor are consecutive, and first_block[t]
// is the first block of tensor t (first_block[count] = the grid).  mt_for_groups cuts a longer table into such groups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DSR_MT_MAX 64
struct MtTable {
  unsigned first_block[DSR_MT_MAX + 1];
  int count;
};

// blockIdx.x -> tensor t (returned) and the block's index within that tensor (blk).  The table sits in kernel-argument
// (scalar) memory and blockIdx.x is wave-uniform, so a linear scan is at most 64 scalar compares with no divergence and no
// vector register; a binary search would save nothing that shows next to the streaming loop behind it.
__device__ __forceinline__ int mt_locate(const MtTable& tb, unsigned& blk) {
  int t = 0;
  while (t + 1 < tb.count && blockIdx.x >= tb.first_block[t + 1]) ++t;
  blk = blockIdx.x - tb.first_block[t];
  return t;
}

// blocks of a tensor of n elements cut into chunks of `chunk` elements from element 0 (an empty tensor has none)
static inline size_t mt_blocks(size_t n, size_t chunk) { return (n + chunk - 1) / chunk; }

// ---- aligned spans: a tensor of 4-byte elements that may start 4, 8 or 12 bytes off a 16-byte boundary (a view) is read
// as a scalar head (<= 3 elements), a body of nvec 16-byte vectors, and a scalar tail (<= 3 elements).  The body is cut
// into chunks of `chunk` elements (chunk / 4 vectors), one block each; the tensor's first block also owns head and tail,
// and a tensor with no body still gets that block.  mt_span_blocks (host) and mt_span (device) must agree.
static __host__ __device__ inline size_t mt_head(const void* p, size_t n) {
  const size_t h = ((16 - ((size_t)(uintptr_t)p & 15)) & 15) / 4;
  return h < n ? h : n;
}
static inline size_t mt_span_blocks(const void* p, size_t n, size_t chunk) {
  const size_t nvec = (n - mt_head(p, n)) / 4;
  return nvec ? mt_blocks(nvec, chunk / 4) : 1;
}
struct MtSpan {   // head scalars, nvec body vectors of which [v0, v1) are this block's, tail from element tail0 on
  size_t head, nvec, v0, v1, tail0;
};
__device__ __forceinline__ MtSpan mt_span(const void* p, size_t n, unsigned blk, size_t chunk) {
  MtSpan s;
  s.head = mt_head(p, n);
  s.nvec = (n - s.head) / 4;
  s.v0 = (size_t)blk * (chunk / 4);
  s.v1 = s.v0 + chunk / 4 < s.nvec ? s.v0 + chunk / 4 : s.nvec;
  s.tail0 = s.head + s.nvec * 4;
  return s;
}

// ---- the host loop.  Walks table entries 0 .. count - 1: skip(i) drops an entry (it takes no slot), blocks_of(i) is its
// block count (0 is allowed: the entry keeps its slot and gets no block), fill(g, slot, i) writes the payload of entry i
// into slot `slot` of the group.  A group is launched -- launch(g, grid) -- when it holds group_max entries or before it
// would pass 2^31 - 1 blocks; a group without blocks launches nothing.  With a skip that never fires the groups are the
// fixed slices [0, group_max), [group_max, 2 group_max), ...  Returns the number of launches made.
template <class Group, class Skip, class Blocks, class Fill, class Launch>
static int mt_for_groups(int count, int group_max, Skip skip, Blocks blocks_of, Fill fill, Launch launch) {
  Group g;
  g.tb.count = 0;
  size_t blocks = 0;
  int launches = 0;
  auto flush = [&]() {
    g.tb.first_block[g.tb.count] = (unsigned)blocks;
    if (blocks) {
      launch(g, (unsigned)blocks);
      ++launches;
    }
    g.tb.count = 0;
    blocks = 0;
  };
  for (int i = 0; i < count; ++i) {
    if (skip(i)) continue;
    const size_t nb = blocks_of(i);
    if (g.tb.count == group_max || blocks + nb > 0x7fffffffull) flush();
    fill(g, g.tb.count, i);
    g.tb.first_block[g.tb.count++] = (unsigned)blocks;
    blocks += nb;
  }
  flush();
  return launches;
}
