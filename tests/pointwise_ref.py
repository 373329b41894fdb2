"""Float64 reference of the pointwise BatchNorm / activation family of csrc/pointwise.hip, and the case table of its sweep.

Every entry point of the family is restated from its contract (include/dsr_hip.h and the kernel comments) as plain float64
torch on [pixels, channels] arrays: the per-block partial rows of the two-stage reductions, the two finalize steps, the three
streaming kernels, the activation backward (plain and pixel-unshuffling), `add`, `sum_rows` and the eval-mode affine.  Nothing
is imported from the package under test: the constants below are restated, and tests/test_host_pointwise.py shows that they
are the ones in the source and the binding.  The functions work on whatever device their arguments live on, so that the two
large cases (capped grid, non-temporal instantiation) can be generated and referenced on the GPU.

Two data regimes, as in the convolution sweep (conv_exact_ref.py):
  exact    small integers for y / dout / residual, powers of two for scale / shift / slopes / rstd / c2, small integers for
           mean / c1: every product and partial sum is a dyadic rational that fp32 holds exactly and every stored 16-bit value
           is representable in bf16 and fp16.  The expected value then does not depend on summation order, FMA contraction or
           the instantiation that ran: the comparison is equality.
  rounded  real-valued data (channels with mean 16 and unit spread beside zero-mean ones) and general fp32 parameters, for the
           toleranced checks; the bounds are derived in tests/test_gpu_pointwise.py from the arithmetic.

Conventions of the kernels that the reference follows:
  z = y * scale + shift;  out = act(z) + residual
  g = dout * act'(.)      LeakyReLU / PReLU: 1 for z >= 0, slope below (read off z in the BatchNorm kernels, off the stored
                          OUTPUT in act_bwd: the same for slope > 0); ReLU: out > 0; ELU: out > 0 ? 1 : out + 1;
                          tanh: 1 - out^2; sigmoid: out (1 - out)
  bn_act_bwd_reduce rows  [blocks][3][Cp] = (sum g, sum g*y, sum dout*z*[z<0] (PReLU only)); slice 1 is sum g*y, NOT sum g*xhat
  act_bwd rows            [blocks][2][CyP] = (sum g, sum dout*(out/slope)*[out<0] (PReLU only))
  block b                 covers pixel rows [b*rpb, min(P, (b+1)*rpb))
"""
import functools
import math

import torch

BF16, F16 = 0, 1
ACT_NONE, ACT_LEAKY, ACT_PRELU, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_ELU = range(7)
DTYPES = {BF16: torch.bfloat16, F16: torch.float16}
ACT_NAMES = {ACT_NONE: "none", ACT_LEAKY: "leaky", ACT_PRELU: "prelu", ACT_RELU: "relu", ACT_TANH: "tanh", ACT_SIGMOID: "sigmoid",
             ACT_ELU: "elu"}
EXACT_LIMIT = float(2 ** 24)

# ---- the launchers' thresholds (csrc/pointwise.hip), cross-checked against the source by tests/test_host_pointwise.py
SCRATCH_ROWS = 64                 # dsr_pw_scratch_rows() == DSR_COMPACT_ROWS: rows every partial buffer keeps behind its own
SERIAL_ROWS = 32                  # up to here the finalize kernels walk the rows themselves (compact_rows: rows <= 32)
FINALIZE_PAR16_ROWS = 128         # bn_finalize: above, and Cp % 16 == 0, the 16-channel form of the parallel kernel
FINALIZE_PAR_ROWS = 512           # DSR_FINALIZE_PAR_ROWS: the parallel forward finalize / sum_rows up to here
FINALIZE_PAR_ROWS_BWD = 64        # DSR_FINALIZE_PAR_ROWS_BWD
COMPACT_WIDE_ROWS = 4096          # compact_rows: from here on 64 chunks instead of 16
NT_BYTES = 192 << 20              # DSR_PW_NT_BYTES: operand tensors of at least this size take the non-temporal instantiation
GRID_CAP = 4096                   # pw_grid: blocks of the cached instantiation of bn_act_fwd / bn_act_bwd_apply
CP_MAX = 2048                     # DSR_CP_OK


def r8(c):
    return (c + 7) // 8 * 8


def rpi_of(cp):
    """Pixel rows one block of a row-walking kernel covers per iteration: 256 threads, one per 8-channel chunk."""
    return 256 // (cp // 8)


def n_blocks(p, rpb):
    return (p + rpb - 1) // rpb


# ----------------------------------------------------------------------------- number formats
def _dt(dtype):
    return dtype if isinstance(dtype, torch.dtype) else DTYPES[dtype]


def r16(t, dtype):
    """float64 -> fp32 -> the 16-bit storage type (round to nearest even) -> float64."""
    return t.to(torch.float32).to(_dt(dtype)).to(torch.float64)


def representable(t, dtype):
    return bool(torch.equal(r16(t, dtype), t.to(torch.float64)))


def exact_f32(t):
    return bool(torch.equal(t.to(torch.float32).to(torch.float64), t.to(torch.float64)))


def ulp32(t):
    """Spacing of fp32 at |t| (float64 tensor); the smallest normal's spacing below it."""
    a = t.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def ulp16(t, dtype):
    """Spacing of the storage type at |t|."""
    mant, emin = (7, -126) if _dt(dtype) == torch.bfloat16 else (10, -14)
    a = t.abs().clamp_min(2.0 ** emin)
    return torch.exp2(torch.floor(torch.log2(a)) - mant)


def neighbours(ref, dtype):
    """The two values of the storage type that enclose the float64 `ref` (equal where ref is representable)."""
    near = ref.to(torch.float32).to(_dt(dtype))
    n64 = near.to(torch.float64)
    bits = near.view(torch.int16).to(torch.int32) & 0xFFFF
    mag, sign = bits & 0x7FFF, bits & 0x8000
    up = ref.abs() > n64.abs()
    other_mag = torch.where(up, mag + 1, (mag - 1).clamp_min(0))
    other_sign = torch.where(mag == 0, torch.where(ref < 0, 0x8000, 0), sign)
    ob = (other_mag | other_sign)
    ob = torch.where(ob >= 0x8000, ob - 0x10000, ob).to(torch.int16)
    other = ob.view(_dt(dtype)).to(torch.float64)
    return n64, torch.where(n64 == ref, n64, other)


# ----------------------------------------------------------------------------- activations
def act_fwd(z, act, slope=0.0):
    if act == ACT_NONE:
        return z
    if act == ACT_RELU:
        return z.clamp_min(0)
    if act in (ACT_LEAKY, ACT_PRELU):
        return torch.where(z >= 0, z, z * slope)
    if act == ACT_TANH:
        return torch.tanh(z)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    if act == ACT_ELU:
        return torch.where(z > 0, z, torch.expm1(z.clamp_max(0)))
    raise ValueError(act)


def act_grad_from_out(o, act, slope=0.0):
    """act' expressed through the activation's output (LeakyReLU / PReLU: through any value of z's sign; slope > 0)."""
    if act == ACT_NONE:
        return torch.ones_like(o)
    if act == ACT_RELU:
        return (o > 0).to(o.dtype)
    if act in (ACT_LEAKY, ACT_PRELU):
        return torch.where(o >= 0, torch.ones_like(o), torch.full_like(o, float(slope)))
    if act == ACT_TANH:
        return 1 - o * o
    if act == ACT_SIGMOID:
        return o * (1 - o)
    if act == ACT_ELU:
        return torch.where(o > 0, torch.ones_like(o), o + 1)
    raise ValueError(act)


# ----------------------------------------------------------------------------- per-block partial rows
def block_sums(t, rpb):
    """t [P, ...] -> [blocks, ...]: block b sums rows [b*rpb, min(P, (b+1)*rpb))."""
    p = t.shape[0]
    full = p // rpb
    parts = []
    if full:
        parts.append(t[:full * rpb].reshape(full, rpb, *t.shape[1:]).sum(1))
    if p % rpb:
        parts.append(t[full * rpb:].sum(0, keepdim=True))
    return torch.cat(parts)


def channel_stats(x, rpb):
    """[blocks][2][Cp] = (sum x, sum x^2)."""
    return torch.stack([block_sums(x, rpb), block_sums(x * x, rpb)], 1)


def colsum(x, rpb):
    """[blocks][1][Cp]."""
    return block_sums(x, rpb)[:, None]


def bn_act_fwd(y, scale, shift, residual, act, slope=0.0):
    z = y if scale is None else y * scale + shift
    out = act_fwd(z, act, slope)
    return out if residual is None else out + residual


def bn_act_g(dout, y, scale, shift, act, slope=0.0):
    """(g, z): the gradient at the BatchNorm output, g = dout * act'(z)."""
    z = y * scale + shift
    arg = z if act in (ACT_LEAKY, ACT_PRELU) else act_fwd(z, act, slope)
    return dout * act_grad_from_out(arg, act, slope), z


def kink_ambiguous(y, scale, shift, act):
    """Elements whose pre-activation is so close to the kink of ReLU / LeakyReLU / PReLU that its fp32 value z = fl(y*scale + shift)
    (two roundings, or one fused; scale / shift themselves within a few ulp of the reference's) may carry the other sign than the
    float64 one: |z| <= 8 * 2^-24 * (|y*scale| + |shift|).  For these the derivative may legitimately be either branch's."""
    if act not in (ACT_RELU, ACT_LEAKY, ACT_PRELU):
        return torch.zeros_like(y, dtype=torch.bool)
    bound = 8 * 2.0 ** -24 * ((y * scale).abs() + shift.abs() + torch.zeros_like(y))
    return ((y * scale + shift).abs() <= bound) & (bound > 0)          # (an exact 0 + 0, as in a pad channel, is no doubt)


def bn_act_bwd_reduce(dout, y, scale, shift, act, slope, rpb):
    """[blocks][3][Cp] = (sum g, sum g*y, PReLU slope terms)."""
    g, z = bn_act_g(dout, y, scale, shift, act, slope)
    sp = dout * z * (z < 0) if act == ACT_PRELU else torch.zeros_like(g)
    return torch.stack([block_sums(g, rpb), block_sums(g * y, rpb), block_sums(sp, rpb)], 1)


def bn_act_bwd_reduce_abs(dout, y, scale, shift, act, slope, rpb):
    """The same rows over |terms| (what the summation-chain bounds scale with)."""
    g, z = bn_act_g(dout, y, scale, shift, act, slope)
    sp = (dout * z * (z < 0)).abs() if act == ACT_PRELU else torch.zeros_like(g)
    return torch.stack([block_sums(g.abs(), rpb), block_sums((g * y).abs(), rpb), block_sums(sp, rpb)], 1)


def bn_finalize(partial, c, cp, count, gamma, beta, running_mean, running_var, num_batches, momentum, eps, updates):
    """partial [rows][2][stride] (stride >= Cp; columns past C are ignored), gamma / beta [C] -> dict of float64 arrays: mean, var
    (biased), rstd, scale, shift [Cp] with zero pad channels; running_mean / running_var [C] after `updates` applications
    with the unbiased variance (count == 1 keeps the biased one); num_batches + updates.  momentum and eps are the fp32 values
    the kernel receives."""
    momentum = float(torch.tensor(momentum, dtype=torch.float32))
    eps = float(torch.tensor(eps, dtype=torch.float32))
    s = partial.to(torch.float64).sum(0)
    mean = s[0, :c] / count
    var = (s[1, :c] / count - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.to(torch.float64) * rstd
    shift = beta.to(torch.float64) - mean * scale
    out = {}
    for k, v in (("mean", mean), ("var", var), ("rstd", rstd), ("scale", scale), ("shift", shift)):
        out[k] = torch.zeros(cp, dtype=torch.float64, device=partial.device)
        out[k][:c] = v
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        rm, rv = running_mean.to(torch.float64).clone(), running_var.to(torch.float64).clone()
        for _ in range(updates):
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * unbiased
        out["running_mean"], out["running_var"] = rm, rv
    out["num_batches"] = None if num_batches is None else num_batches + updates
    return out


def bn_bwd_finalize(partial, c, cp, count, mean, rstd):
    """partial [rows][3][Cp] -> dgamma, dbeta [C]; dprelu (scalar, real channels only); c1 = dbeta / count, c2 = dgamma / count
    [Cp] with zero pad channels."""
    s = partial.to(torch.float64).sum(0)
    sg, sgy, sp = s[0, :c], s[1, :c], s[2, :c]
    dgamma = rstd[:c].to(torch.float64) * (sgy - mean[:c].to(torch.float64) * sg)
    c1 = torch.zeros(cp, dtype=torch.float64, device=partial.device)
    c2 = torch.zeros_like(c1)
    c1[:c], c2[:c] = sg / count, dgamma / count
    return dict(dgamma=dgamma, dbeta=sg, dprelu=sp.sum(), c1=c1, c2=c2)


def bn_act_bwd_apply(dout, y, scale, shift, mean, rstd, c1, c2, act, slope, train):
    """dy = scale * (g - c1 - xhat * c2), xhat = (y - mean) * rstd; eval mode: dy = scale * g."""
    g, _ = bn_act_g(dout, y, scale, shift, act, slope)
    if not train:
        return scale * g
    return scale * (g - c1 - (y - mean) * rstd * c2)


def bn_act_bwd_apply_terms(dout, y, scale, shift, mean, rstd, c1, c2, act, slope):
    """|A g| + |B y| + |C| of the kernel's folded form dy = A g + B y + C (A = scale, B = -scale c2 rstd,
    C = scale (c2 mean rstd - c1))."""
    g, _ = bn_act_g(dout, y, scale, shift, act, slope)
    return (scale * g).abs() + (scale * c2 * rstd * y).abs() + (scale * (c2 * mean * rstd - c1)).abs() + torch.zeros_like(g)


def unshuffle_nhwc(t, cyp):
    """PixelShuffle(2) backward gather: t [N][2H][2W][CoP] -> [N][H][W][CyP], channel 4c + 2i + j <- pixel (2h+i, 2w+j) of
    channel c; conv channels whose shuffle channel lies past CoP read as zero."""
    n, h2, w2, cop = t.shape
    u = t.view(n, h2 // 2, 2, w2 // 2, 2, cop).permute(0, 1, 3, 5, 2, 4).reshape(n, h2 // 2, w2 // 2, 4 * cop)
    if 4 * cop >= cyp:
        return u[..., :cyp].contiguous()
    out = torch.zeros(n, h2 // 2, w2 // 2, cyp, dtype=t.dtype, device=t.device)
    out[..., :4 * cop] = u
    return out


def act_bwd(dout, out, act, slope, rpb):
    """dout / out [P][CyP] (already un-shuffled for the pixshuf form) -> dy [P][CyP], partial [blocks][2][CyP].  A PReLU slope
    that is not positive poisons everything with NaN."""
    g = dout * act_grad_from_out(out, act, slope)
    sp = dout * (out / slope) * (out < 0) if act == ACT_PRELU else torch.zeros_like(g)
    if act == ACT_PRELU and not slope > 0:
        g, sp = torch.full_like(g, math.nan), torch.full_like(g, math.nan)
    return g, torch.stack([block_sums(g, rpb), block_sums(sp, rpb)], 1)


def act_bwd_nchw(dout, out, act, cp):
    """fp32 NCHW dout / out (tanh / sigmoid / none) -> dy [N][H][W][Cp], pad channels zero."""
    n, c, h, w = dout.shape
    dy = torch.zeros(n, h, w, cp, dtype=torch.float64, device=dout.device)
    dy[..., :c] = (dout * act_grad_from_out(out, act, 0.0)).permute(0, 2, 3, 1)
    return dy


def add(a, b):
    return a + b


def sum_rows(partial, row_stride, col_offset, c, scale, out0, accumulate):
    """partial: flat, rows * row_stride floats.  out[c] (+)= scale * sum_r partial[r * row_stride + col_offset + c]."""
    rows = partial.numel() // row_stride
    v = partial.to(torch.float64).view(rows, row_stride)[:, col_offset:col_offset + c].sum(0) * scale
    return out0.to(torch.float64) + v if accumulate else v


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, c, cp):
    eps = float(torch.tensor(eps, dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(running_var.to(torch.float64) + eps)
    scale = gamma.to(torch.float64) * rstd
    vals = dict(rstd=rstd, scale=scale, shift=beta.to(torch.float64) - running_mean.to(torch.float64) * scale,
                mean=running_mean.to(torch.float64))
    out = {}
    for k, v in vals.items():
        out[k] = torch.zeros(cp, dtype=torch.float64, device=gamma.device)
        out[k][:c] = v
    return out


# ----------------------------------------------------------------------------- BatchNorm(train) + activation, composed
def bn_train_act(y, c, gamma, beta, eps, act, slope, dout, residual=None, rpb=64):
    """The three-launch forward and the three-launch backward, composed from the per-entry-point references above.
    y / dout / residual [P][Cp] float64 with zero pad channels; gamma / beta [C].  Returns out, dx, dgamma, dbeta, dprelu and
    the intermediate per-channel arrays."""
    p, cp = y.shape
    fin = bn_finalize(channel_stats(y, rpb), c, cp, float(p), gamma, beta, None, None, None, 0.1, eps, 0)
    out = bn_act_fwd(y, fin["scale"], fin["shift"], residual, act, slope)
    rows = bn_act_bwd_reduce(dout, y, fin["scale"], fin["shift"], act, slope, rpb)
    bw = bn_bwd_finalize(rows, c, cp, float(p), fin["mean"], fin["rstd"])
    dx = bn_act_bwd_apply(dout, y, fin["scale"], fin["shift"], fin["mean"], fin["rstd"], bw["c1"], bw["c2"], act, slope, True)
    return dict(out=out, dx=dx, dgamma=bw["dgamma"], dbeta=bw["dbeta"], dprelu=bw["dprelu"], fin=fin, bw=bw)


# ----------------------------------------------------------------------------- the case table
EXACT_ACTS = [(ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LEAKY, 0.25), (ACT_PRELU, 0.25), (ACT_PRELU, 0.5)]
CP_LIST = [8, 24, 64, 136, 2048]      # rpi 256 | cpr 3, rpi 85, one idle thread | rpi 32 | cpr 17, rpi 15, one idle thread | rpi 1
C_OF_CP = {8: 3, 24: 23, 64: 64, 136: 135, 2048: 2048}
PRIME_P = 997


def stream_case(cp, p, rpb, name=None):
    return dict(name=name or f"cp{cp}_p{p}_rpb{rpb}", cp=cp, c=C_OF_CP[cp], p=p, rpb=rpb, rpi=rpi_of(cp))


def _stream_cases():
    out = []
    for cp in CP_LIST:
        rpi = rpi_of(cp)
        out.append(stream_case(cp, 1, 64))                              # one pixel
        if rpi > 2:
            out.append(stream_case(cp, rpi - 1, max(1, rpi // 3)))      # no thread sees a second row; several short blocks
        out.append(stream_case(cp, rpi + 1, rpi + 1))                   # one block: the tail iteration alone
        out.append(stream_case(cp, 2 * rpi + 1, 2 * rpi + 1))           # one block: one trip of the two-row loop, then the tail
        out.append(stream_case(cp, PRIME_P, 100))                       # ten blocks, the last one shorter than rpb
    return out


STREAM_CASES = _stream_cases()
STREAM_IDS = [c["name"] for c in STREAM_CASES]
# grid cap of the cached instantiation: 4096 blocks of 32 rows, two rows in flight per trip, then 33 tail rows
CAPPED = dict(name="capped_grid", cp=64, c=64, p=GRID_CAP * 32 * 2 + 32 + 1, rpi=32)
# just over DSR_PW_NT_BYTES: the non-temporal instantiation (the size is the only way in without an environment override)
NONTEMPORAL = dict(name="nontemporal", cp=64, c=64, p=6 * 512 * 512 + 1, rpi=32)

# (rows, Cp, stride, updates): dsr_pw_bn_finalize
FINALIZE_CASES = [(1, 8, 8, 1), (7, 24, 24, 0), (8, 64, 64, 2), (32, 136, 136, 1), (33, 24, 24, 1), (33, 64, 80, 2), (128, 64, 64, 1),
                  (129, 64, 64, 1), (129, 24, 24, 2), (512, 136, 136, 1), (512, 64, 64, 0), (513, 24, 40, 1), (513, 64, 64, 2),
                  (4095, 8, 8, 1), (4096, 24, 24, 1), (4200, 8, 8, 1)]
# (rows, Cp, with dprelu): dsr_pw_bn_bwd_finalize; rows 40 at Cp 136 with dprelu is forced onto the serial kernel
BWD_FINALIZE_CASES = [(1, 8, True), (3, 24, True), (4, 64, False), (32, 136, True), (33, 64, True), (33, 136, False), (40, 64, True),
                      (40, 64, False), (40, 136, True), (64, 24, True), (64, 136, False), (65, 64, True), (65, 136, False),
                      (700, 24, True)]
# (rows, row_stride, col_offset, C, compact, accumulate, scale): dsr_pw_sum_rows
SUM_ROWS_CASES = [(1, 8, 0, 8, 1, 0, 1.0), (7, 24, 3, 20, 0, 1, 0.5), (8, 1, 0, 1, 1, 0, 0.25), (32, 48, 24, 23, 1, 0, 2.0),
                  (33, 48, 24, 23, 1, 1, 0.5), (33, 1, 0, 1, 1, 0, 1.0), (300, 1, 0, 1, 0, 1, 0.5), (512, 136, 1, 135, 0, 0, 0.25),
                  (513, 136, 1, 135, 1, 0, 0.25), (513, 64, 0, 64, 0, 1, 1.0), (4095, 16, 8, 8, 1, 1, 0.5), (4096, 16, 0, 16, 1, 0, 0.125),
                  (4096, 1, 0, 1, 1, 0, 0.125)]
# (N, H, W, shuffle channels C): act_bwd with pixshuf; CyP = r8(4 C), CoP = r8(C): 3 and 9 give CyP != 4 CoP
PIXSHUF_CASES = [(1, 1, 1, 2), (2, 3, 5, 3), (1, 7, 11, 9), (2, 9, 13, 16), (1, 5, 3, 64)]
# (N, C, H, W, act): act_bwd_nchw
NCHW_CASES = [(1, 3, 1, 1, ACT_NONE), (2, 3, 7, 9, ACT_TANH), (1, 1, 17, 31, ACT_SIGMOID), (2, 9, 5, 3, ACT_TANH)]
ADD_NVEC = [1, 255, 257, 997]
# (Cp, P, rpb) of the rounded-regime and end-to-end cases
REAL_CASES = [stream_case(8, 4099, 512), stream_case(8, 515, 64), stream_case(24, PRIME_P, 100), stream_case(64, 2500, 64), stream_case(136, 301, 64),
              stream_case(2048, 67, 64)]
REAL_IDS = [c["name"] for c in REAL_CASES]
# End to end the statistics pass through fp32 partial rows (sum y, sum y^2): one rounding each, which the ABI fixes.  For a channel
# with mean / sigma = m those leave about 3 * 2^-24 * m^2 / sqrt(blocks) in the variance, half of it in rstd, and an element of dx
# at the 2^-6 floor of the relative check carries 64 times the relative error of its terms.  With m = 16, one fp16 ulp (2^-11)
# for this part of the budget asks for sqrt(blocks) >= 64 * 1.5 * 2^-24 * 256 / 2^-11 ~ 3, i.e. about 16 blocks of 64 rows or
# more.  So the end-to-end cases start at 997 pixels in 16 blocks -- the case at which the sweep found channel_stats' fp32
# chain of y^2 (16 of its 23,928 fp16 dx elements beyond the bound before the fix) -- and the others have 1291 (a prime, 21 blocks,
# the last one short) or more.  The 67- and 301-pixel shapes of REAL_CASES (2 and 5 rows) are left out of the end-to-end check
# for that reason alone: with so few fp32 rows the row format itself, not a kernel, puts dx up to 1.1 times the bound.
E2E_P = 1291
E2E_CASES = [stream_case(8, E2E_P, 64), stream_case(24, PRIME_P, 100), stream_case(24, E2E_P, 64), stream_case(64, 2500, 64),
             stream_case(136, E2E_P, 64), stream_case(2048, E2E_P, 64)]
E2E_IDS = [c["name"] for c in E2E_CASES]
_f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # slopes as the fp32 values the kernels receive
REAL_ACTS = [(ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LEAKY, _f32(0.2)), (ACT_PRELU, _f32(0.3)), (ACT_ELU, 0.0), (ACT_TANH, 0.0), (ACT_SIGMOID, 0.0)]
LARGE_MEAN = 16.0


def partial_row_thresholds():
    """Per finalize entry point: (the row counts of its cases, the thresholds t its launcher branches on: the table must hold
    t and t + 1)."""
    fwd = [r for r, *_ in FINALIZE_CASES]
    bwd = [r for r, *_ in BWD_FINALIZE_CASES]
    srw = [r for r, *_ in SUM_ROWS_CASES]
    return {"bn_finalize": (fwd, [SERIAL_ROWS, FINALIZE_PAR16_ROWS, FINALIZE_PAR_ROWS, COMPACT_WIDE_ROWS - 1]),
            "bn_bwd_finalize": (bwd, [SERIAL_ROWS, FINALIZE_PAR_ROWS_BWD]),
            "sum_rows": (srw, [SERIAL_ROWS, FINALIZE_PAR_ROWS, COMPACT_WIDE_ROWS - 1])}


# ----------------------------------------------------------------------------- data
def _gen(name, salt, device="cpu"):
    return torch.Generator(device=device).manual_seed(1000 * sum(ord(ch) for ch in name) + salt)


def ints(gen, shape, amp, device="cpu"):
    return torch.randint(-amp, amp + 1, shape, generator=gen, device=device).to(torch.float64)


def pow2(gen, shape, lo, hi, device="cpu", signed=False):
    v = torch.exp2(torch.randint(lo, hi + 1, shape, generator=gen, device=device).to(torch.float64))
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=gen, device=device) * 2 - 1)
    return v


def _zero_pad(t, c):
    t[..., c:] = 0
    return t


def exact_stream(case, device="cpu"):
    """Exact-regime operands of a streaming case: y, dout, residual [P][Cp] (integers in [-3, 3], pad channels zero), and the
    per-channel arrays [Cp] with zero pad channels: scale in {1/2, 1, 2}, shift in +-{1/2, 1, 2}, mean in {-1, 0, 1},
    rstd in {1/2, 1}, c1 in {-1, 0, 1}, c2 in {1/2, 1}."""
    gen = _gen(case["name"], 1, device)
    p, cp, c = case["p"], case["cp"], case["c"]
    d = dict(case=case)
    for k in ("y", "dout", "residual"):
        d[k] = _zero_pad(ints(gen, (p, cp), 3, device), c)
    d["scale"] = _zero_pad(pow2(gen, (cp,), -1, 1, device), c)
    d["shift"] = _zero_pad(pow2(gen, (cp,), -1, 1, device, signed=True), c)
    d["mean"] = _zero_pad(ints(gen, (cp,), 1, device), c)
    d["rstd"] = _zero_pad(pow2(gen, (cp,), -1, 0, device), c)
    d["c1"] = _zero_pad(ints(gen, (cp,), 1, device), c)
    d["c2"] = _zero_pad(pow2(gen, (cp,), -1, 0, device), c)
    return d


@functools.lru_cache(maxsize=None)
def exact_stream_cpu(name):
    """Shared, computed once; callers must not modify it."""
    return exact_stream(STREAM_CASES[STREAM_IDS.index(name)])


def exact_act_out(gen, shape, c, slope, device="cpu"):
    """A stored activation output for act_bwd in the exact regime: integers where positive, slope * integer where negative."""
    z = _zero_pad(ints(gen, shape, 3, device), c)
    return torch.where(z >= 0, z, z * (slope if slope > 0 else 0.25))


def finalize_rows(rows, cp, stride, c):
    """Integer partial rows [rows][2][stride] of a tensor with one pixel per row (what channel_stats writes with rpb = 1):
    x in offset_c + [-3, 3] with offset 16 on every third channel; the columns past C hold junk that must be ignored."""
    gen = _gen(f"fin{rows}_{cp}_{stride}", 2)
    x = ints(gen, (rows, c), 3) + (torch.arange(c) % 3 == 1) * LARGE_MEAN
    part = ints(gen, (rows, 2, stride), 50)
    part[:, 0, :c], part[:, 1, :c] = x, x * x
    return part


def bwd_finalize_rows(rows, cp, c):
    """Integer partial rows [rows][3][Cp] (junk in the pad columns) and exact mean / rstd: everything the finalize computes is a
    dyadic rational fp32 holds."""
    gen = _gen(f"bwd{rows}_{cp}", 3)
    part = ints(gen, (rows, 3, cp), 8)
    mean = ints(gen, (cp,), 2)
    rstd = pow2(gen, (cp,), -2, 1)
    return part, mean, rstd


def real_stream(case, dtype):
    """Rounded-regime operands: 16-bit-rounded real data (every third channel with mean 16, unit spread), general fp32 parameters."""
    gen = _gen(case["name"], 5 + dtype)
    p, cp, c = case["p"], case["cp"], case["c"]
    big = (torch.arange(cp) % 3 == 1).to(torch.float64) * LARGE_MEAN
    d = dict(case=case)
    d["y"] = _zero_pad(r16(torch.randn(p, cp, generator=gen, dtype=torch.float64) + big, dtype), c)
    d["dout"] = _zero_pad(r16(torch.randn(p, cp, generator=gen, dtype=torch.float64), dtype), c)
    d["residual"] = _zero_pad(r16(torch.randn(p, cp, generator=gen, dtype=torch.float64), dtype), c)
    # the end-to-end case's upstream gradient: one-signed, so that no large share of dx cancels to nothing
    # (own generator; its seed is one for which under 5 % of the reference dx lies below the end-to-end check's floor, a property of
    # the reference inputs alone that test_host_pointwise.py asserts)
    gen_e = _gen(case["name"], 53 + dtype)
    d["dout_e2e"] = _zero_pad(r16(0.5 + torch.rand(p, cp, generator=gen_e, dtype=torch.float64), dtype), c)
    f32 = lambda t: t.to(torch.float32).to(torch.float64)
    d["gamma"] = f32(0.5 + torch.rand(c, generator=gen, dtype=torch.float64))
    d["beta"] = f32(0.5 * torch.randn(c, generator=gen, dtype=torch.float64))
    return d


@functools.lru_cache(maxsize=None)
def real_stream_cached(name, dtype):
    return real_stream(next(c for c in REAL_CASES + E2E_CASES if c["name"] == name), dtype)


def real_params(d, act, slope, rpb=64):
    """The fp32 per-channel arrays a kernel of the BatchNorm chain receives for rounded-regime operands d: float64 finalize
    results rounded to fp32 (as float64 tensors), for the forward and -- with this activation -- the backward."""
    c, cp, p, eps = d["case"]["c"], d["case"]["cp"], d["case"]["p"], 1e-5
    f32 = lambda t: t.to(torch.float32).to(torch.float64)
    fin = bn_finalize(channel_stats(d["y"], rpb), c, cp, float(p), d["gamma"], d["beta"], None, None, None, 0.1, eps, 0)
    q = {k: f32(fin[k]) for k in ("scale", "shift", "mean", "rstd")}
    rows = bn_act_bwd_reduce(d["dout"], d["y"], q["scale"], q["shift"], act, slope, rpb)
    bw = bn_bwd_finalize(rows, c, cp, float(p), q["mean"], q["rstd"])
    q["c1"], q["c2"] = f32(bw["c1"]), f32(bw["c2"])
    return q
