"""Float64 references, operand generators and case tables of the dense-head sweep (csrc/linear.hip through the raw C ABI):
test_host_linear.py proves the references and the tables on the CPU, test_gpu_linear.py runs the kernels against them.

Every reference is written from the contract in include/dsr_hip.h; nothing is imported from the package.

Regime A (exact): integer operands (dyadic where stated) small enough that every product and every partial sum, in any order, is
an integer (or a dyadic rational) below 2^24 in magnitude -- bounded by sum |a||b|, not by the signed sum -- so fp32 accumulation,
split-K order, MFMA shape and the fp64 reduce cannot change a bit, and every 16-bit output is representable in bf16 AND fp16.
Regime B (rounded once): the same with larger operands, so that 16-bit outputs need rounding; the expected value is
round-to-nearest-even of the exact value, to16(): float64 -> fp32 -> 16 bits on the CPU.  The exact values are integers (or
multiples of 1/64) below 2^24, so the first step is exact and the double rounding is harmless (the host test shows it).
Zeros: a sum that starts from +0 cannot end in -0, so every accumulated reference is normalised with `+ 0.0` and compared bit for
bit.  The one place where -0 == +0 is allowed is dense2_bwd's 16-bit dh (dy16, dyT16): the value is an element-wise product whose
IEEE sign is that of its factors, but the sign of a ZERO gradient is not part of the contract -- the compiler may fuse the
multiply with the conversion to fp16 (v_fma_mixlo_f16 with a +0 addend, which is what hipcc emits on gfx950: (-0) + (+0) = +0)
while the bf16 form keeps -0, and no consumer (an MFMA operand) can tell the two apart.  Non-zero values are bit-exact there too.

dense2_fwd is the one entry point without an exact regime: out = 1 / (1 + expf(-v)) with v an exact integer.  ROCm's table of
device-function ulp errors is not among the documents this project can read offline, so the bound is a measured
one: with d = the largest deviation, in fp32 ulp of the float64 result, of torch's fp32 CPU sigmoid from float64 sigmoid on the
same sums, a result must be within max(4 d, 2) ulp (sigmoid_bar()).  Sums of magnitude >= SATURATED (expf overflows or 1 + e
rounds to 1) are only required to be finite, inside [0, 1], and exactly 1 for v >= 20."""
import functools

import torch

BF16, F16 = 0, 1
DTYPES = {BF16: torch.bfloat16, F16: torch.float16}
ACT_NONE, ACT_LEAKY = 0, 1
F64 = torch.float64
EXACT = float(1 << 24)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, a, seed):
    """Uniform integers in [-a, a] as float64."""
    return torch.randint(-a, a + 1, tuple(shape), generator=gen(seed)).to(F64)


def to16(t, dtype):
    """Round-to-nearest-even of an exact float64 value to the storage type: float64 -> fp32 -> 16 bits."""
    return t.to(torch.float32).to(DTYPES[dtype])


def fits16(t):
    """True when every value survives the trip through bf16 and through fp16."""
    return all(bool((to16(t, d).to(F64) == t).all()) for d in (BF16, F16))


def unique(rows, cols):
    """The impulse cases' second operand: a value in [-125, 125] (exact in both storage types) that differs between
    neighbouring rows and neighbouring columns, so a misplaced element shows as the wrong number."""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    return (((r * 7 + c * 3 + c % 5) % 251) - 125).to(F64)


def ties16(exact, dtype):
    """Number of values that lie exactly half way between two neighbours of the storage type."""
    r = to16(exact, dtype).to(F64)
    fin = r.isfinite()
    bits = to16(exact, dtype).view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(DTYPES[dtype]).to(F64)
    dn = (bits - 1).to(torch.int16).view(DTYPES[dtype]).to(F64)
    other = torch.where(exact.abs() > r.abs(), up, dn)
    tie = fin & other.isfinite() & (exact != r) & ((exact - r).abs() == (other - exact).abs())
    return int(tie.sum())


IMPULSE_MAX = 1 << 21          # the impulse form runs where the weight has at most this many elements (its table is slow to build)


# ----------------------------------------------------------------------------- linear forward
FWD_B = (1, 16, 17, 32, 33, 64)
FWD_O = (1, 8, 255, 256, 257, 1032)
FWD_K = (8, 64, 72, 128, 136, 264, 7168, 8192, 9224, 33000)
SLOPES = ((ACT_NONE, 0.0), (ACT_LEAKY, 0.25), (ACT_LEAKY, 0.2))


def fwd_shapes(K):
    """(B, O) pairs run at this K: every B, the O rotating so that every (O, K) pair and every (B, K) pair of the three sets is in
    the table (the largest weight, 1032 x 33000, once)."""
    i = FWD_K.index(K)
    return [(B, FWD_O[(i + j) % len(FWD_O)]) for j, B in enumerate(FWD_B)]


def linear_pre(x, w):
    """sum_k x[b][k] w[o][k]"""
    return x @ w.t() + 0.0


def linear_fwd(x, w, bias, act, slope, pre=None):
    """out[b][o] = act(sum_k x[b][k] w[o][k] + bias[o]); LeakyReLU keeps v >= 0 and multiplies the rest by the fp32 slope.
    `pre`: linear_pre(x, w) when the caller already has it."""
    v = linear_pre(x, w) if pre is None else pre
    if bias is not None:
        v = v + bias[None, :]
    if act == ACT_LEAKY:
        s = float(torch.tensor(slope, dtype=torch.float32))                  # the slope as the kernel holds it
        v = torch.where(v >= 0, v, (v * s).to(torch.float32).to(F64))        # ONE fp32 product, rounded once
    return v


def fwd_case(B, O, K, impulse=False):
    """x [B][K], w [O][K] in [-2, 2] (sum |x||w| <= 4 K <= 132000), bias [O] in [-8, 8].  Output column 0 has a zero weight row
    and bias -0.0, column 1 (O > 1) a zero row and bias +0: pre-activations of exactly -0 + 0 and 0; column 2 has its bias set
    so that row 0 cancels to 0.  Impulse form: x[b] is one-hot at a position from the k-tile edges, w = unique()."""
    seed = B * 1000003 + O * 1009 + K
    if impulse:
        x = torch.zeros(B, K, dtype=F64)
        pos = sorted({k for k in (0, 7, 8, 63, 64, 71, 127, 128, 1023, 1024, 1151, 1152, K // 2, K - 9, K - 8, K - 1) if 0 <= k < K})
        for b in range(B):
            x[b, pos[(b * 5 + b // 3) % len(pos)]] = 1.0
        w = unique(O, K)
    else:
        x, w = ints((B, K), 2, seed), ints((O, K), 2, seed + 1)
    bias = ints((O,), 8, seed + 2)
    if not impulse:
        w[0] = 0.0
        bias[0] = -0.0
        if O > 1:
            w[1] = 0.0
            bias[1] = 0.0
        if O > 2:
            bias[2] = -float(x[0] @ w[2])
    return x, w, bias


# ----------------------------------------------------------------------------- linear input gradient
DG_B = FWD_B
DG_O = (8, 24, 32, 40, 1032)
DG_K = (8, 120, 128, 136, 264, 33000)
DG_WIDE_K = (131064, 131072, 131080)      # below, at and above the 256 * 512 switch to 256-column blocks
DG_WIDE_O = 16


def dgrad_shapes(K):
    i = DG_K.index(K)
    return [(B, DG_O[(i + j) % len(DG_O)]) for j, B in enumerate(DG_B)]


def amp_b(dtype, O):
    """Operand magnitudes (dy, w) of regime B: the sums reach a few times 2^8 (bf16) resp. 2^11 (fp16), where odd integers are
    exact ties, and stay finite in fp16."""
    if dtype == BF16:
        return (3, 8) if O > 40 else (7, 31)
    return (7, 31) if O > 40 else (15, 127)


def linear_dgrad(dy, w):
    """dx[b][k] = sum_o dy[b][o] w[o][k]"""
    return dy @ w + 0.0


def dgrad_case(B, O, K, regime="A", dtype=BF16, impulse=False):
    """dy [B][O], w [O][K].  A: dy in [-1, 1], w in [-2, 2]; B: amp_b().  Impulse: dy[b] one-hot in o, w = unique()."""
    seed = 77 + B * 1000003 + O * 1009 + K
    if impulse:
        dy = torch.zeros(B, O, dtype=F64)
        pos = sorted({o for o in (0, 7, 8, 15, 16, 23, 31, 32, 39, O // 2, O - 9, O - 8, O - 1) if 0 <= o < O})
        for b in range(B):
            dy[b, pos[(b * 3 + b // 4) % len(pos)]] = 1.0
        return dy, unique(O, K)
    ay, aw = (1, 2) if regime == "A" else amp_b(dtype, O)
    return ints((B, O), ay, seed), ints((O, K), aw, seed + 1)


# ----------------------------------------------------------------------------- weight gradient, plain and gathered
WG_BP = (32, 64)
WG_O = (1, 63, 64, 65, 255, 257)
WG_K = (4, 36, 508, 512, 516, 1160)
WG_RS = ((1, 1.0), (2, 0.5), (3, 1.0 / 3.0), (4, 0.25), (3, 1.0), (2, 0.25))      # (R, scale); 1/3 is the one inexact scale


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def linear_wgrad(dyT, xT, scale=1.0):
    """dw[o][k] = fl32(scale) * sum_r sum_b dyT[r][o][b] xT[r][k][b], the product with the scale rounded ONCE to fp32
    (exact when the scale is a power of two)."""
    s = torch.einsum("rob,rkb->ok", dyT, xT) + 0.0
    return (s * f32(scale)).to(torch.float32).to(F64)


@functools.lru_cache(maxsize=16)
def wgrad_case(Bp, O, K, R=1, impulse=False, a=3):
    """dyT [R][O][Bp], xT [R][K][Bp] in [-a, a]; the batch is B = Bp - 5 wide, columns b >= B are zero.
    Impulse: dyT[r][o] one-hot at b = (o + r) % B with value r + 1, xT = unique() per r."""
    seed = 991 + Bp * 1000003 + O * 1009 + K * 7 + R
    B = Bp - 5
    if impulse:
        dyT = torch.zeros(R, O, Bp, dtype=F64)
        for r in range(R):
            dyT[r, torch.arange(O), (torch.arange(O) + r) % B] = float(r + 1)
        xT = torch.stack([unique(K, Bp) * (1 if r % 2 == 0 else -1) for r in range(R)])
    else:
        dyT, xT = ints((R, O, Bp), a, seed), ints((R, K, Bp), a, seed + 1)
    dyT[:, :, B:] = 0.0
    xT[:, :, B:] = 0.0
    return dyT, xT


# ----------------------------------------------------------------------------- fused weight gradient + Adam
WA_R = (1, 2, 3)
WA_O = (1, 63, 64, 65, 130)
WA_K = (64, 192, 256, 320)
WA_KPB = (None, "2", "3")
WA_STEPS = (1, 2, 1000)
WA_SCALE = {1: 1.0, 2: 0.5, 3: 1.0 / 3.0}
ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)


def wa_cases():
    """(R, O, K, step, grad_scale, kpb): every (O, K) pair, with R, the step, DSR_WGRAD_ADAM_KPB and a power-of-two gradient scale
    rotating so that every (R, kpb) and (R, step) pair occurs and K = 320 (a block whose later k tiles are past K) meets every kpb."""
    out = []
    for O in WA_O:
        for K in WA_K:
            i = len(out)
            out.append((WA_R[i % 3], O, K, WA_STEPS[(i + i // 3) % 3], (1.0, 0.5)[(i // 2) % 2], WA_KPB[(i // 3) % 3]))
    return out


@functools.lru_cache(maxsize=None)
def adam_state(O, K):
    """p ~ N(0, 1), m ~ 0.1 N(0, 1), v ~ 0.5 + U(0, 1) (fp32 values): a state in the middle of a run."""
    g = gen(4242 + O * 1009 + K)
    p = torch.randn(O, K, generator=g, dtype=torch.float32)
    m = 0.1 * torch.randn(O, K, generator=g, dtype=torch.float32)
    v = 0.5 + torch.rand(O, K, generator=g, dtype=torch.float32)
    return p, m, v


def adam_torch_fp32(p, m, v, g, step, lr, b1, b2, eps):
    """torch.optim.Adam in fp32 on the CPU, continued from (p, m, v) at `step` - 1: the floor of the Adam bar."""
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    q.grad = g.to(torch.float32)
    opt.step()
    st = opt.state[q]
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def rel(a, b):
    a, b = torch.as_tensor(a).to(F64), torch.as_tensor(b).to(F64)
    return float((a - b).norm() / b.norm())


# ----------------------------------------------------------------------------- Gram norm of the factored gradient
GRAM_N = {32: (32, 1), 64: (64, 1), 96: (32, 3), 128: (64, 2), 160: (32, 5), 256: (64, 4), 480: (32, 15), 512: (64, 8)}   # N: (Bp, R)
GRAM_O = (8, 31, 33, 1024)
GRAM_K = (64, 1000, 4104)


def gram_cases():
    """(Bp, R, O, K, scale): every N at every K, O and the scale rotating."""
    out = []
    for i, (n, (bp, r)) in enumerate(GRAM_N.items()):
        for j, K in enumerate(GRAM_K):
            out.append((bp, r, GRAM_O[(i + j) % 4], K, (1.0, 0.5)[(i + j) % 2]))
    return out


def gram_norm2(dyT, xT):
    """|sum_r dyT[r]^T-contracted-with xT[r]|_F^2 of the materialised product, as a Python integer (int64 arithmetic on an
    exact float64 matmul: every entry is an integer far below 2^53)."""
    dw = torch.einsum("rob,rkb->ok", dyT, xT)
    assert float(dw.abs().max()) < 2.0 ** 31
    dw = dw.to(torch.int64)
    return int((dw * dw).sum())


def gram_identity(dyT, xT):
    """The same number from the two N x N Gram matrices: sum_ij Gx[i][j] Gdy[i][j], i = (r, b)."""
    X = xT.permute(1, 0, 2).reshape(xT.shape[1], -1)
    Y = dyT.permute(1, 0, 2).reshape(dyT.shape[1], -1)
    return float(((X.t() @ X) * (Y.t() @ Y)).sum())


# ----------------------------------------------------------------------------- dense2: Linear(K1, 1) + Sigmoid
D2_SLOPE = 0.25
D2B_B = (1, 5, 32, 33, 64)
D2B_BP = (32, 40, 64)
D2B_K1 = (1, 127, 128, 129, 1024)
D2F_B = (1, 64)
D2F_K1 = (1, 255, 256, 257, 1024)
D2F_TARGETS = (0, 100, -100, 200, -200, 20, -20, 1, -1, 2, -3, 5, -7, 10, -12, 15, -17, 19, 4, -5, 8, -9)
SATURATED = 20


def dense2_bwd(dout, out, h, w2, Bp, slope):
    """dz[b] = dout[b] out[b] (1 - out[b]);  dw2[k] = sum_b dz[b] h[b][k];  db2 = sum_b dz[b];
    dh[b][k] = dz[b] w2[k] (1 if h[b][k] >= 0 else slope) -- the project's convention: derivative 1 AT 0, +0 and -0 alike
    (torch's leaky_relu backward gives `slope` there; they differ nowhere else);  db1[k] = sum_b dh[b][k];
    dy = dh [B][K1];  dyT = dh^T [K1][Bp], columns b >= B zero."""
    B, K1 = h.shape
    dz = dout * out * (1.0 - out)
    dh = dz[:, None] * w2[None, :] * torch.where(h >= 0, 1.0, slope)
    dyT = torch.zeros(K1, Bp, dtype=F64)
    dyT[:, :B] = dh.t()
    return {"dw2": (dz[:, None] * h).sum(0) + 0.0, "db2": dz.sum().reshape(1) + 0.0, "db1": dh.sum(0) + 0.0, "dy": dh, "dyT": dyT}


@functools.lru_cache(maxsize=8)
def dense2_bwd_case(B, K1, regime="A"):
    """out in {1/4, 1/2, 3/4}; dout, h, w2 integers -- |.| <= 4 (A: every dh a multiple of 1/64 with a numerator <= 256) or
    dout, w2 up to 63 (B: numerators up to 11907, rounded in both types).  h carries +0 and -0."""
    seed = 313 + B * 1009 + K1
    a = 4 if regime == "A" else 63
    dout, w2, h = ints((B,), a, seed), ints((K1,), a, seed + 1), ints((B, K1), 4, seed + 2)
    out = torch.randint(1, 4, (B,), generator=gen(seed + 3)).to(F64) / 4.0
    zero = (torch.arange(B)[:, None] * 5 + torch.arange(K1)[None, :]) % 7
    h = torch.where(zero == 0, torch.zeros(()).to(F64), h)
    h = torch.where(zero == 3, -torch.zeros(()).to(F64), h)
    return dout, out, h, w2


def dense2_fwd_sum(h, w2, b2):
    return h @ w2 + b2


@functools.lru_cache(maxsize=None)
def dense2_fwd_case(B, K1, offset=0):
    """Integer h [B][K1], w2 [K1] (w2[0] = 1), b2; h[b][0] is set so that row b's sum is D2F_TARGETS[(b + offset) % len]."""
    seed = 555 + B * 1009 + K1
    h, w2 = ints((B, K1), 4, seed), ints((K1,), 4, seed + 1)
    w2[0] = 1.0
    b2 = 3.0
    tgt = torch.tensor([D2F_TARGETS[(b + offset) % len(D2F_TARGETS)] for b in range(B)], dtype=F64)
    h[:, 0] = 0.0
    h[:, 0] = tgt - dense2_fwd_sum(h, w2, b2)
    return h, w2, b2, tgt


def ulp32(t):
    """The fp32 ulp at |t| (float64 tensor), the smallest subnormal below the normal range."""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 23).clamp_min(2.0 ** -149)


def sigmoid_bar(sums):
    """(d, bar) in fp32 ulp: torch's fp32 CPU sigmoid against float64 on these sums, and max(4 d, 2)."""
    ref = torch.sigmoid(sums)
    got = torch.sigmoid(sums.to(torch.float32)).to(F64)
    d = float(((got - ref).abs() / ulp32(ref)).max())
    return d, max(4.0 * d, 2.0)


# ----------------------------------------------------------------------------- cast16
CAST_N = (8, 2040, 2048, 2056)
CAST_GRID_CAP = 8 * 256 * 8192            # elements one pass of the capped grid covers


def cast_specials():
    """fp32 values at the edges of both 16-bit types: ties both ways, signed zeros, subnormals of fp32 / bf16 / fp16, infinities,
    NaN, the fp16 overflow edge and the bf16 one (largest finite, the next fp32 above it, the tie that rounds to infinity)."""
    bits = [0x3F808000, 0x3F818000, 0x3F80C000, 0x3F804000,                 # bf16 ties to even / to odd + 1, above and below a tie
            0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001,                 # fp16 ties (13 dropped bits) and their neighbours
            0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00010000, 0x007FFFFF, 0x00008000, 0x00018000,
            0x33800000, 0x33800001, 0x33000000, 0x387FC000, 0x38800000, 0x387FE000,   # around fp16's smallest subnormal / normal
            0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
            0x7F7F0000, 0x7F7F0001, 0x7F7F7FFF, 0x7F7F8000, 0xFF7F8000, 0x7F7FFFFF]
    t = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)
    edge = torch.tensor([65504.0, 65519.99, 65520.0, -65504.0, -65519.99, -65520.0, 65535.0, 1e5], dtype=torch.float32)
    return torch.cat([t, edge])


def cast_case(n):
    """N(0, 1) scaled over many binades with the specials planted at evenly spread positions (n = 8: the first eight)."""
    sp = cast_specials()
    g = gen(n)
    x = torch.randn(n, generator=g, dtype=torch.float32) * torch.pow(2.0, torch.randint(-30, 18, (n,), generator=g).float())
    if n >= len(sp):
        x[torch.arange(len(sp)) * (n // len(sp))] = sp
    else:
        x[:] = sp[:n]
    return x


# ----------------------------------------------------------------------------- flatten
FL_B = (1, 5, 33, 64)
FL_HW = (1, 6, 8, 63, 64, 72, 200)
FL_CP = (8, 24, 64, 72, 128)
FL_BP = (32, 64)


def flatten_shapes():
    """(B, HW, C, Cp): every (HW, Cp) pair with C = Cp and C = Cp - 3, B rotating."""
    out = []
    for i, hw in enumerate(FL_HW):
        for j, cp in enumerate(FL_CP):
            for c in (cp, cp - 3):
                out.append((FL_B[(i + j) % 4], hw, c, cp))
    return out


def takes_tile_form(mode, HW, Cp, Bp, switch=None):
    """The launcher's rule for the LDS-tiled kernel (test_host_linear.py reads it from the source)."""
    return switch != "0" and Cp % 64 == 0 and (Bp % 8 == 0 if mode == 1 else HW % 8 == 0)


def counter(shape, start=0):
    """16-bit counter pattern (int16 bits): consecutive elements differ, and so do elements one row apart."""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, dtype=torch.int64) + start) % 65521 - 32768).to(torch.int16).reshape(shape)


def flatten0(act, C):
    """flat[b][c * HW + p] = act[b][p][c], c < C"""
    B, HW, Cp = act.shape
    b, c, p = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(HW), indexing="ij")
    flat = torch.zeros(B, C * HW, dtype=act.dtype)
    flat[b, c * HW + p] = act[b, p, c]
    return flat


def flatten1(act, C, Bp):
    """flatT[c * HW + p][b] = act[b][p][c], c < C; columns b >= B zero"""
    B, HW, Cp = act.shape
    b, c, p = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(HW), indexing="ij")
    flatT = torch.zeros(C * HW, Bp, dtype=act.dtype)
    flatT[c * HW + p, b] = act[b, p, c]
    return flatT


def flatten2(flat, C, HW, Cp):
    """act[b][p][c] = flat[b][c * HW + p], c < C; pad channels zero"""
    B = flat.shape[0]
    b, c, p = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(HW), indexing="ij")
    act = torch.zeros(B, HW, Cp, dtype=flat.dtype)
    act[b, p, c] = flat[b, c * HW + p]
    return act


# ----------------------------------------------------------------------------- what the launchers choose (host test: == the source)
DG_WIDE_MIN_K = 256 * 512
GRAM_MAX_N = 512


def fwd_mt(B):
    return 2 if B <= 32 else 4


def gram_nsub(N):
    return min(8, 512 // N)
