// L-BFGS with fixed step (torch.optim.LBFGS, line_search_fn=None) for the LBFGS branch of utils/DIP.optimize
// (reference utils/DIP.py:19-31), in the vector-free form of Chen, Wang & Zhou, "Large-scale L-BFGS using MapReduce"
// (NIPS 2014): the search direction is a combination of the basis {s_i, y_i, g}, so the two-loop recursion runs on
// scalar coefficients and needs only the dot products between basis vectors (the Gram matrix).
//
// Per inner iteration (all state on the device, no host read):
//   gather   g <- the .grad tensors (null = zeros), pending y = g - g_prev, max|g| and sum|g|          one pass over g
//   dots     pending s, pending y, g against every live history vector and each other, fp64         one read of the history
//   scalar   one wave: commit the pending pair if ys > 1e-10, two-loop on coefficients, t, gtd, every stop rule of
//            torch/optim/lbfgs.py (lines 463, 510-526) -> device flag
//   combine  d = sum_j coef_j b_j, pending s = t d into the free ring slot, p += s                      one read of the history
//
// The layout of `vecs` (S slot j at j, Y slot j at m+1+j, gradient buffer b at 2(m+1)+b, n_pad floats each), the ring of
// m + 1 slots with its pending pair, and the five public header ints are part of the state contract: include/dsr_hip.h.
// Gram indices are the vector indices of the S / Y slots; the current gradient is Gram index 2(m+1).
// Every reduction has a fixed order (per-thread fp64 sums, butterfly within a wave, waves in order, blocks in order):
// results are bitwise deterministic.
#include "dsr_common.h"
#include "dsr_kernels.h"
#include "multi_tensor.h"
#include "../../include/dsr_hip.h"

#define LB_GATHER_CHUNK 4096     // elements per gather block
#define LB_COMBINE_CHUNK 1024    // elements per combine block (4 per thread)
#define LB_DOT_E 8               // elements per thread of the dot pass (multiple of 4)
#define LB_MAX_HISTORY 1024      // the scalar kernel keeps its coefficient vectors in LDS

struct LbfgsHdr {
  int n_iter, func_evals;        // state["n_iter"], state["func_evals"] of torch's optimizer
  int n_iter_step, cur_evals;    // n_iter and current_evals of the running step()
  int count, free_slot, gprev;   // live pairs, ring slot of the pending pair, gradient buffer holding prev_flat_grad
  int mode;                      // what the combine pass does: 0 nothing, 1 write the pending s, 2 and update the parameters
  int nlive, gather_blocks, combine_blocks, reserved;
  double h_diag, t, prev_loss;
};

struct LbLayout {                // byte offsets into the workspace
  size_t slot_of, ro, al, idx, coef, dots, gram, dpart, gsum, gmax, cmax, total;
  size_t n_pad;
  int m, nb;
  unsigned bdot;
};

static size_t lb_al256(size_t x) { return (x + 255) & ~(size_t)255; }

static bool lb_layout(int m, size_t n, int ntensors, LbLayout& L) {
  if (m < 1 || m > LB_MAX_HISTORY || n == 0 || ntensors < 1 || n > ((size_t)1 << 40)) return false;
  L.m = m;
  L.nb = 2 * (m + 1) + 1;
  L.n_pad = (n + 3) & ~(size_t)3;
  L.bdot = (unsigned)((L.n_pad + 256 * LB_DOT_E - 1) / (256 * LB_DOT_E));
  const size_t bg = n / LB_GATHER_CHUNK + ntensors, bc = n / LB_COMBINE_CHUNK + ntensors;   // >= sum of ceil(n_i / chunk)
  size_t o = lb_al256(sizeof(LbfgsHdr));
  L.slot_of = o; o = lb_al256(o + sizeof(int) * m);
  L.ro = o;      o = lb_al256(o + sizeof(double) * (m + 1));
  L.al = o;      o = lb_al256(o + sizeof(double) * m);
  L.idx = o;     o = lb_al256(o + sizeof(int) * L.nb);
  L.coef = o;    o = lb_al256(o + sizeof(double) * L.nb);
  L.dots = o;    o = lb_al256(o + sizeof(double) * 6 * (m + 2));
  L.gram = o;    o = lb_al256(o + sizeof(double) * (size_t)L.nb * L.nb);
  L.dpart = o;   o = lb_al256(o + sizeof(double) * 6 * (size_t)(m + 2) * L.bdot);
  L.gsum = o;    o = lb_al256(o + sizeof(double) * bg);
  L.gmax = o;    o = lb_al256(o + sizeof(unsigned) * bg);
  L.cmax = o;    o = lb_al256(o + sizeof(unsigned) * bc);
  L.total = o;
  return true;
}

template <typename T>
static T* lb_at(void* ws, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

__device__ __forceinline__ unsigned lb_wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}

// up to 64 tensors of one flat vector per gather / combine launch (multi_tensor.h)
struct LbGroup {
  float* ptr[DSR_MT_MAX];
  size_t off[DSR_MT_MAX];              // the tensor's offset in the flat vector
  size_t n[DSR_MT_MAX];
  MtTable tb;
  unsigned block_base, total_blocks;   // blocks of the launches before this one; blocks of the whole table
};
static_assert(sizeof(LbGroup) <= 4096, "kernel arguments are limited to 4 KB");

// max|x| is taken on the bit patterns of |x| (order-preserving for non-negative floats; a NaN beats every number, so it
// survives the reduction and fails the `<=` tests like torch's max does)
__global__ __launch_bounds__(256) void lbfgs_gather_kernel(const LbGroup a, LbfgsHdr* __restrict__ hdr, float* __restrict__ vecs,
                                                           size_t n_pad, int m, double* __restrict__ gsum,
                                                           unsigned* __restrict__ gmax) {
  __shared__ double ss[4];
  __shared__ unsigned sx[4];
  unsigned blk;
  const int t = mt_locate(a.tb, blk);
  const size_t base = (size_t)blk * LB_GATHER_CHUNK;
  const size_t nt = a.n[t];
  const float* __restrict__ gr = a.ptr[t];
  const int gprev = hdr->gprev, slot = hdr->free_slot;
  const float* __restrict__ gp = vecs + (size_t)(2 * (m + 1) + gprev) * n_pad + a.off[t];
  float* __restrict__ gc = vecs + (size_t)(2 * (m + 1) + 1 - gprev) * n_pad + a.off[t];
  float* __restrict__ y = vecs + (size_t)(m + 1 + slot) * n_pad + a.off[t];
  unsigned mx = 0;
  double sm = 0.0;
  for (size_t i = base + threadIdx.x; i < base + LB_GATHER_CHUNK && i < nt; i += 256) {
    const float g = gr ? gr[i] : 0.f;
    y[i] = g - gp[i];
    gc[i] = g;
    const float ag = fabsf(g);
    mx = max(mx, __float_as_uint(ag));
    sm += (double)ag;
  }
  sm = wave_sum(sm);
  mx = lb_wave_max(mx);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    ss[w] = sm;
    sx[w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned b = a.block_base + blockIdx.x;
    gsum[b] = ((ss[0] + ss[1]) + ss[2]) + ss[3];
    gmax[b] = max(max(sx[0], sx[1]), max(sx[2], sx[3]));
    if (blockIdx.x == 0) hdr->gather_blocks = a.total_blocks;
  }
}

// one block = 256 x LB_DOT_E consecutive elements; the pending s, y and g of those elements stay in registers while the
// block walks the live slots, so the history is read once and the three pending vectors once.  Per slot j six dots
// (s.s_j, s.y_j, y.s_j, y.y_j, g.s_j, g.y_j), per block one partial of each: dpart[(j * 6 + c) * bdot + block]; row
// m + 1 holds the six dots among the pending vectors themselves (s.s, s.y, y.y, g.s, g.y, g.g).
__global__ __launch_bounds__(256) void lbfgs_dot_kernel(const LbfgsHdr* __restrict__ hdr, const int* __restrict__ slot_of,
                                                        const float* __restrict__ vecs, size_t n_pad, int m,
                                                        double* __restrict__ dpart, unsigned bdot) {
  constexpr int Q = LB_DOT_E / 4;
  __shared__ double red[2][4][6];
  const int count = hdr->count, p = hdr->free_slot, gcur = 1 - hdr->gprev;
  const float* sp = vecs + (size_t)p * n_pad;
  const float* yp = vecs + (size_t)(m + 1 + p) * n_pad;
  const float* gg = vecs + (size_t)(2 * (m + 1) + gcur) * n_pad;
  const size_t e0 = (size_t)blockIdx.x * 256 * LB_DOT_E;
  double s[4 * Q], yv[4 * Q], g[4 * Q];
  size_t off[Q];
  bool ok[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    off[q] = e0 + ((size_t)q * 256 + threadIdx.x) * 4;
    ok[q] = off[q] < n_pad;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 a = ok[q] ? *reinterpret_cast<const float4*>(sp + off[q]) : z;
    const float4 b = ok[q] ? *reinterpret_cast<const float4*>(yp + off[q]) : z;
    const float4 c = ok[q] ? *reinterpret_cast<const float4*>(gg + off[q]) : z;
    s[4 * q] = a.x; s[4 * q + 1] = a.y; s[4 * q + 2] = a.z; s[4 * q + 3] = a.w;
    yv[4 * q] = b.x; yv[4 * q + 1] = b.y; yv[4 * q + 2] = b.z; yv[4 * q + 3] = b.w;
    g[4 * q] = c.x; g[4 * q + 1] = c.y; g[4 * q + 2] = c.z; g[4 * q + 3] = c.w;
  }
  const int w = threadIdx.x >> 6;
  int par = 0;
  auto emit = [&](double* v, int row) {
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) red[par][w][c] = v[c];
    }
    __syncthreads();      // red[] is double-buffered: a wave that runs ahead writes the other half
    if (threadIdx.x < 6) {
      const int c = threadIdx.x;
      dpart[((size_t)row * 6 + c) * bdot + blockIdx.x] = ((red[par][0][c] + red[par][1][c]) + red[par][2][c]) + red[par][3][c];
    }
    par ^= 1;
  };
  {
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4 * Q; ++k) {
      v[0] = fma(s[k], s[k], v[0]);
      v[1] = fma(s[k], yv[k], v[1]);
      v[2] = fma(yv[k], yv[k], v[2]);
      v[3] = fma(g[k], s[k], v[3]);
      v[4] = fma(g[k], yv[k], v[4]);
      v[5] = fma(g[k], g[k], v[5]);
    }
    emit(v, m + 1);
  }
  for (int i = 0; i < count; ++i) {
    const int j = slot_of[i];
    const float* sj = vecs + (size_t)j * n_pad;
    const float* yj = vecs + (size_t)(m + 1 + j) * n_pad;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 a = ok[q] ? *reinterpret_cast<const float4*>(sj + off[q]) : z;
      const float4 b = ok[q] ? *reinterpret_cast<const float4*>(yj + off[q]) : z;
      const double as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 4 * q + u;
        v[0] = fma(s[k], as[u], v[0]);
        v[1] = fma(s[k], bs[u], v[1]);
        v[2] = fma(yv[k], as[u], v[2]);
        v[3] = fma(yv[k], bs[u], v[3]);
        v[4] = fma(g[k], as[u], v[4]);
        v[5] = fma(g[k], bs[u], v[5]);
      }
    }
    emit(v, j);
  }
}

// dots[row * 6 + c] = sum over the dot blocks in order; one wave per row (live slots and the pending row m + 1)
__global__ __launch_bounds__(64) void lbfgs_dot_reduce_kernel(const LbfgsHdr* __restrict__ hdr, const int* __restrict__ slot_of,
                                                              const double* __restrict__ dpart, unsigned bdot, int m,
                                                              double* __restrict__ dots) {
  const int row = blockIdx.x;
  if (row <= m) {
    const int count = hdr->count;
    bool live = false;
    for (int i = 0; i < count; ++i) live |= slot_of[i] == row;
    if (!live) return;
  }
  for (int c = 0; c < 6; ++c) {
    const double* src = dpart + ((size_t)row * 6 + c) * bdot;
    double v = 0.0;
    for (unsigned b = threadIdx.x; b < bdot; b += 64) v += src[b];
    v = wave_sum(v);
    if (threadIdx.x == 0) dots[row * 6 + c] = v;
  }
}

struct LbScalarArgs {
  LbfgsHdr* hdr;
  int* slot_of;
  double* ro;
  int* idx;
  double* coef;
  const double* dots;
  double* gram;
  const double* gsum;
  const unsigned* gmax;
  const unsigned* cmax;
  const float* loss;
  int* stop;
  int first, m, max_iter, max_eval;
  double lr, tol_grad, tol_change;
};

// One wave.  LDS: coefficient vector q / r over the Gram indices [nb], al [m], the live Gram indices [nb].
__global__ __launch_bounds__(64) void lbfgs_scalar_kernel(const LbScalarArgs a) {
  extern __shared__ double lds[];
  const int m = a.m, nb = 2 * (m + 1) + 1, G = 2 * (m + 1);
  double* q = lds;
  double* al = lds + nb;
  int* lst = reinterpret_cast<int*>(lds + nb + m);
  const int lane = threadIdx.x;
  LbfgsHdr h = *a.hdr;

  double gs = 0.0;
  unsigned gm = 0;
  for (int b = lane; b < h.gather_blocks; b += 64) {
    gs += a.gsum[b];
    gm = max(gm, a.gmax[b]);
  }
  gs = wave_sum(gs);
  gm = lb_wave_max(gm);
  const float loss = *a.loss;
  const bool opt_cond = (double)__uint_as_float(gm) <= a.tol_grad;

  bool stop = false;
  if (a.first) {                           // lbfgs.py:364-374: the step's first closure
    h.n_iter_step = 0;
    h.cur_evals = 1;
    h.func_evals += 1;
    stop = opt_cond;
  } else {                                 // lbfgs.py:497-526: the closure after an update, then the break tests
    h.cur_evals += 1;
    h.func_evals += 1;
    unsigned cm = 0;
    for (int b = lane; b < h.combine_blocks; b += 64) cm = max(cm, a.cmax[b]);
    cm = lb_wave_max(cm);
    const double dt_max = (double)__uint_as_float(cm);       // max |d t| of the update just made
    stop = h.cur_evals >= a.max_eval || opt_cond || dt_max <= a.tol_change ||
           fabs((double)loss - h.prev_loss) < a.tol_change;
  }
  if (!stop && h.n_iter_step >= a.max_iter) stop = true;
  if (stop) {
    if (lane == 0) {
      h.mode = 0;
      *a.hdr = h;
      *a.stop = 1;
    }
    return;
  }
  h.n_iter_step += 1;
  h.n_iter += 1;
  const double* pend = a.dots + (m + 1) * 6;     // s.s, s.y, y.y, g.s, g.y, g.g of the pending pair and the gradient
  const int p = h.free_slot;
  bool committed = false;
  if (h.n_iter == 1) {                           // lbfgs.py:396-401
    h.count = 0;
    h.free_slot = 0;
    h.h_diag = 1.0;
  } else if (pend[1] > 1e-10) {                  // lbfgs.py:404-421
    committed = true;
    for (int i = lane; i < h.count; i += 64) {
      const int j = a.slot_of[i];
      const double* dj = a.dots + j * 6;
      const int sp = p, yp = m + 1 + p, sj = j, yj = m + 1 + j;
      a.gram[(size_t)sp * nb + sj] = dj[0]; a.gram[(size_t)sj * nb + sp] = dj[0];
      a.gram[(size_t)sp * nb + yj] = dj[1]; a.gram[(size_t)yj * nb + sp] = dj[1];
      a.gram[(size_t)yp * nb + sj] = dj[2]; a.gram[(size_t)sj * nb + yp] = dj[2];
      a.gram[(size_t)yp * nb + yj] = dj[3]; a.gram[(size_t)yj * nb + yp] = dj[3];
    }
    if (lane == 0) {
      const int sp = p, yp = m + 1 + p;
      a.gram[(size_t)sp * nb + sp] = pend[0];
      a.gram[(size_t)sp * nb + yp] = pend[1];
      a.gram[(size_t)yp * nb + sp] = pend[1];
      a.gram[(size_t)yp * nb + yp] = pend[2];
      a.ro[p] = 1.0 / pend[1];
    }
    h.h_diag = pend[1] / pend[2];
    __syncthreads();                             // every lane has read slot_of before lane 0 rotates it
    if (h.count == m) {                          // full: the oldest pair leaves, its slot becomes the free one
      const int ev = a.slot_of[0];
      if (lane == 0) {
        for (int i = 0; i + 1 < m; ++i) a.slot_of[i] = a.slot_of[i + 1];
        a.slot_of[m - 1] = p;
      }
      h.free_slot = ev;
    } else {                                     // filling: slots are taken in order
      if (lane == 0) a.slot_of[h.count] = p;
      h.count += 1;
      h.free_slot = h.count;
    }
    __syncthreads();
  }
  // Gram row of the new gradient against the live slots
  const int k = h.count, L = 2 * k + 1;
  for (int i = lane; i < k; i += 64) {
    const int j = a.slot_of[i];
    const double gsj = committed && j == p ? pend[3] : a.dots[j * 6 + 4];
    const double gyj = committed && j == p ? pend[4] : a.dots[j * 6 + 5];
    a.gram[(size_t)G * nb + j] = gsj; a.gram[(size_t)j * nb + G] = gsj;
    a.gram[(size_t)G * nb + m + 1 + j] = gyj; a.gram[(size_t)(m + 1 + j) * nb + G] = gyj;
    lst[i] = j;
    lst[k + i] = m + 1 + j;
  }
  for (int i = lane; i < nb; i += 64) q[i] = 0.0;
  __syncthreads();
  if (lane == 0) {
    a.gram[(size_t)G * nb + G] = pend[5];
    lst[2 * k] = G;
    q[G] = -1.0;                                 // q = -g
  }
  __syncthreads();
  // lbfgs.py:432-435: al[i] = (s_i . q) ro[i]; q -= al[i] y_i
  for (int i = k - 1; i >= 0; --i) {
    const double* row = a.gram + (size_t)lst[i] * nb;
    double acc = 0.0;
    for (int l = lane; l < L; l += 64) acc = fma(q[lst[l]], row[lst[l]], acc);
    const double ali = wave_sum(acc) * a.ro[lst[i]];
    __syncthreads();
    if (lane == 0) {
      al[i] = ali;
      q[lst[k + i]] -= ali;
    }
    __syncthreads();
  }
  // lbfgs.py:439-442: r = q H_diag; be = (y_i . r) ro[i]; r += (al[i] - be) s_i
  for (int l = lane; l < L; l += 64) q[lst[l]] *= h.h_diag;
  __syncthreads();
  for (int i = 0; i < k; ++i) {
    const double* row = a.gram + (size_t)lst[k + i] * nb;
    double acc = 0.0;
    for (int l = lane; l < L; l += 64) acc = fma(q[lst[l]], row[lst[l]], acc);
    const double be = wave_sum(acc) * a.ro[lst[i]];
    __syncthreads();
    if (lane == 0) q[lst[i]] += al[i] - be;
    __syncthreads();
  }
  // lbfgs.py:460: gtd = g . d;  the direction's coefficients go to the combine pass
  double acc = 0.0;
  const double* grow = a.gram + (size_t)G * nb;
  for (int l = lane; l < L; l += 64) acc = fma(q[lst[l]], grow[lst[l]], acc);
  const double gtd = wave_sum(acc);
  const int gvec = 2 * (m + 1) + 1 - h.gprev;    // vector index of the current gradient buffer
  for (int l = lane; l < L; l += 64) {
    const int c = lst[l];
    a.idx[l] = c == G ? gvec : c;
    a.coef[l] = q[c];
  }
  h.nlive = L;
  h.gprev = 1 - h.gprev;                         // prev_flat_grad = flat_grad (lbfgs.py:444-448)
  h.prev_loss = (double)loss;
  if (h.n_iter == 1) {                           // lbfgs.py:454-457
    const double x = 1.0 / gs;
    h.t = (x < 1.0 ? x : 1.0) * a.lr;
  } else {
    h.t = a.lr;
  }
  int fin = 0;
  if (gtd > -a.tol_change) {                     // lbfgs.py:463: no update, but d and t are kept for the next pair
    h.mode = 1;
    fin = 1;
  } else {
    h.mode = 2;
    fin = h.n_iter_step == a.max_iter;           // lbfgs.py:493,511: the last iteration evaluates no closure
  }
  if (lane == 0) {
    *a.hdr = h;
    *a.stop = fin;
  }
}

// d = sum_l coef[l] vecs[idx[l]] (fp64), pending s = t d into the free slot, and (mode 2) p += s through the table
__global__ __launch_bounds__(256) void lbfgs_combine_kernel(const LbGroup a, LbfgsHdr* __restrict__ hdr, const int* __restrict__ idx,
                                                            const double* __restrict__ coef, float* __restrict__ vecs,
                                                            size_t n_pad, unsigned* __restrict__ cmax) {
  __shared__ unsigned sx[4];
  unsigned blk;
  const int t = mt_locate(a.tb, blk);
  const size_t base = (size_t)blk * LB_COMBINE_CHUNK;
  const size_t nt = a.n[t], off = a.off[t];
  const int mode = hdr->mode;
  unsigned mx = 0;
  if (mode != 0) {
    const int nl = hdr->nlive;
    const double tt = hdr->t;
    float* __restrict__ s_out = vecs + (size_t)hdr->free_slot * n_pad + off;
    float* __restrict__ prm = a.ptr[t];
    const size_t i0 = base + threadIdx.x;
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ok[u] = i0 + 256 * u < nt;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int l = 0; l < nl; ++l) {
      const float* v = vecs + (size_t)idx[l] * n_pad + off + i0;
      const double c = coef[l];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fma(c, (double)(ok[u] ? v[256 * u] : 0.f), acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!ok[u]) continue;
      const float s = (float)(tt * acc[u]);
      s_out[i0 + 256 * u] = s;
      if (mode == 2) prm[i0 + 256 * u] += s;
      mx = max(mx, __float_as_uint(fabsf(s)));
    }
  }
  mx = lb_wave_max(mx);
  if ((threadIdx.x & 63) == 0) sx[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    cmax[a.block_base + blockIdx.x] = max(max(sx[0], sx[1]), max(sx[2], sx[3]));
    if (blockIdx.x == 0) hdr->combine_blocks = a.total_blocks;
  }
}

// ------------------------------------------------------------------ C ABI
extern "C" size_t dsr_lbfgs_workspace(int history, size_t n, int ntensors) {
  LbLayout L;
  return lb_layout(history, n, ntensors, L) ? L.total : 0;
}

extern "C" size_t dsr_lbfgs_vector_floats(int history, size_t n) {
  LbLayout L;
  return lb_layout(history, n, 1, L) ? (size_t)(2 * (history + 1) + 2) * L.n_pad : 0;
}

// validates a tensor table against n; returns the total block count (0 on error, after dsr_fail)
static unsigned lb_blocks(const char* what, int count, const void* const* ptrs, bool null_ok, const size_t* numel, size_t n,
                          size_t chunk) {
  size_t tot = 0, blocks = 0;
  for (int i = 0; i < count; ++i) {
    if (numel[i] == 0 || (!null_ok && !ptrs[i])) {
      dsr_fail(DSR_E_ARG, "%s: tensor %d is empty or null", what, i);
      return 0;
    }
    tot += numel[i];
    blocks += mt_blocks(numel[i], chunk);
  }
  if (tot != n) {
    dsr_fail(DSR_E_ARG, "%s: tensor sizes add up to %zu, not n = %zu", what, tot, n);
    return 0;
  }
  return (unsigned)blocks;
}

template <typename K>
static void lb_launch_groups(int count, const void* const* ptrs, const size_t* numel, size_t chunk, unsigned total, K launch) {
  size_t off = 0;
  unsigned block_base = 0;
  mt_for_groups<LbGroup>(
      count, DSR_MT_MAX, [](int) { return false; },                        // fixed slices (lb_blocks refused empty tensors)
      [&](int i) { return mt_blocks(numel[i], chunk); },
      [&](LbGroup& g, int j, int i) {
        g.ptr[j] = const_cast<float*>(static_cast<const float*>(ptrs[i]));
        g.off[j] = off;
        g.n[j] = numel[i];
        off += numel[i];
      },
      [&](LbGroup& g, unsigned blocks) {
        g.block_base = block_base;
        g.total_blocks = total;
        launch(g, blocks);
        block_base += blocks;
      });
}

extern "C" int dsr_lbfgs_gather(int count, const float* const* grads, const size_t* numel, void* ws, size_t ws_bytes,
                                float* vecs, int history, size_t n, hipStream_t st) {
  LbLayout L;
  DSR_REQUIRE(count > 0 && grads && numel && ws && vecs, "lbfgs_gather: null pointer or empty table");
  DSR_REQUIRE(lb_layout(history, n, count, L) && ws_bytes >= L.total, "lbfgs_gather: bad history / size or workspace too small");
  const unsigned total = lb_blocks("lbfgs_gather", count, reinterpret_cast<const void* const*>(grads), true, numel, n,
                                   LB_GATHER_CHUNK);
  if (!total) return DSR_E_ARG;
  lb_launch_groups(count, reinterpret_cast<const void* const*>(grads), numel, LB_GATHER_CHUNK, total,
                   [&](const LbGroup& g, unsigned blocks) {
                     hipLaunchKernelGGL(lbfgs_gather_kernel, dim3(blocks), dim3(256), 0, st, g, lb_at<LbfgsHdr>(ws, 0), vecs,
                                        L.n_pad, L.m, lb_at<double>(ws, L.gsum), lb_at<unsigned>(ws, L.gmax));
                   });
  return dsr_launch_status("dsr_lbfgs_gather");
}

extern "C" int dsr_lbfgs_dots(void* ws, size_t ws_bytes, const float* vecs, int history, size_t n, int ntensors,
                              hipStream_t st) {
  LbLayout L;
  DSR_REQUIRE(ws && vecs, "lbfgs_dots: null pointer");
  DSR_REQUIRE(lb_layout(history, n, ntensors, L) && ws_bytes >= L.total, "lbfgs_dots: bad history / size or workspace too small");
  hipLaunchKernelGGL(lbfgs_dot_kernel, dim3(L.bdot), dim3(256), 0, st, lb_at<const LbfgsHdr>(ws, 0),
                     lb_at<const int>(ws, L.slot_of), vecs, L.n_pad, L.m, lb_at<double>(ws, L.dpart), L.bdot);
  hipLaunchKernelGGL(lbfgs_dot_reduce_kernel, dim3(L.m + 2), dim3(64), 0, st, lb_at<const LbfgsHdr>(ws, 0),
                     lb_at<const int>(ws, L.slot_of), lb_at<const double>(ws, L.dpart), L.bdot, L.m, lb_at<double>(ws, L.dots));
  return dsr_launch_status("dsr_lbfgs_dots");
}

extern "C" int dsr_lbfgs_scalar(void* ws, size_t ws_bytes, int history, size_t n, int ntensors, const float* loss, int first,
                                int* stop, double lr, int max_iter, int max_eval, double tolerance_grad, double tolerance_change,
                                hipStream_t st) {
  LbLayout L;
  DSR_REQUIRE(ws && loss && stop, "lbfgs_scalar: null pointer");
  DSR_REQUIRE(lb_layout(history, n, ntensors, L) && ws_bytes >= L.total, "lbfgs_scalar: bad history / size or workspace too small");
  DSR_REQUIRE(lr >= 0.0, "lbfgs_scalar: learning rate must be >= 0");
  LbScalarArgs a;
  a.hdr = lb_at<LbfgsHdr>(ws, 0);
  a.slot_of = lb_at<int>(ws, L.slot_of);
  a.ro = lb_at<double>(ws, L.ro);
  a.idx = lb_at<int>(ws, L.idx);
  a.coef = lb_at<double>(ws, L.coef);
  a.dots = lb_at<const double>(ws, L.dots);
  a.gram = lb_at<double>(ws, L.gram);
  a.gsum = lb_at<const double>(ws, L.gsum);
  a.gmax = lb_at<const unsigned>(ws, L.gmax);
  a.cmax = lb_at<const unsigned>(ws, L.cmax);
  a.loss = loss;
  a.stop = stop;
  a.first = first ? 1 : 0;
  a.m = L.m;
  a.max_iter = max_iter;
  a.max_eval = max_eval;
  a.lr = lr;
  a.tol_grad = tolerance_grad;
  a.tol_change = tolerance_change;
  const size_t lds = sizeof(double) * (L.nb + L.m) + sizeof(int) * L.nb;
  hipLaunchKernelGGL(lbfgs_scalar_kernel, dim3(1), dim3(64), lds, st, a);
  return dsr_launch_status("dsr_lbfgs_scalar");
}

extern "C" int dsr_lbfgs_combine(int count, float* const* params, const size_t* numel, void* ws, size_t ws_bytes, float* vecs,
                                 int history, size_t n, hipStream_t st) {
  LbLayout L;
  DSR_REQUIRE(count > 0 && params && numel && ws && vecs, "lbfgs_combine: null pointer or empty table");
  DSR_REQUIRE(lb_layout(history, n, count, L) && ws_bytes >= L.total, "lbfgs_combine: bad history / size or workspace too small");
  const unsigned total = lb_blocks("lbfgs_combine", count, reinterpret_cast<const void* const*>(params), false, numel, n,
                                   LB_COMBINE_CHUNK);
  if (!total) return DSR_E_ARG;
  lb_launch_groups(count, reinterpret_cast<const void* const*>(params), numel, LB_COMBINE_CHUNK, total,
                   [&](const LbGroup& g, unsigned blocks) {
                     hipLaunchKernelGGL(lbfgs_combine_kernel, dim3(blocks), dim3(256), 0, st, g, lb_at<LbfgsHdr>(ws, 0),
                                        lb_at<const int>(ws, L.idx), lb_at<const double>(ws, L.coef), vecs, L.n_pad,
                                        lb_at<unsigned>(ws, L.cmax));
                   });
  return dsr_launch_status("dsr_lbfgs_combine");
}
