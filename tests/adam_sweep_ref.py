"""Reference, error bands and case tables of the elementwise sweep of the Adam kernels (test_host_adam_sweep.py,
test_gpu_adam_sweep.py): dsr_pw_adam and dsr_pw_adam_multi against one float64 statement of the step.

The checks are SINGLE STEPS FROM A GIVEN STATE.  A step counter written to the device and arbitrary m, v >= 0 give a state in
the middle of a run, so no error accumulates across steps and the bands below are those of one pass through adam_update
(csrc/dsr_common.h).

Reference.  adam_step() takes the fp32 inputs and the fp32 VALUES of the hyper-parameters (F32(0.9), not 0.9) and evaluates
in float64, on torch's elementwise ops so that it runs on either device:

    gk = g gs       m' = b1 m + (1 - b1) gk      v' = b2 v + (1 - b2) gk^2
    D  = sqrt(v') / sqrt(1 - b2^t) + eps         U  = lr / (1 - b1^t) m' / D         p' = p - U

gs is the multiplier as adam_resolve forms it: grad_scale (host mode), 1 / S (scaler mode, S a power of two), and with a hyper
block the fp32 product fl(gs hyper[1]) -- one rounding, taken here too -- with lr = hyper[0].  Float64 carries 29 more bits
than fp32, so the reference's own error (a few 2^-53) is 2^-27 of the smallest band below and is not added to them.

Bands, per element, u = 2^-24.  adam_update and adam_coef run with contraction off, so every fp32 operation is one rounding
fl(x) = x (1 + e), |e| <= u / (1 + u) (round to nearest, no intermediate subnormal: test_host_adam_sweep.py checks that none
occurs in these tables).  Products of k such factors stay below 1 + k u for k <= 3 because (1 + u/(1+u))^3 < 1 + 3u.

  gk~ = fl(g gs): one rounding, e1 (none when gs is a power of two).
  m~  = fl(fl(b1 m) + fl(w1 gk~)), w1 = fl(1 - b1) exact by Sterbenz (1/2 <= b1 <= 2).  The first term carries two roundings
        (product, sum), the second three (gk, product, sum):
            |m~ - m'| <= 3u (b1 |m| + (1 - b1) |gk|)                                                     =: 3u A
  v~  = fl(fl(b2 v) + fl(fl(w2 gk~) gk~)): the second term carries e1 twice, two products and the sum, 5 roundings, the first
        term two; all terms are non-negative, so with one u for the second-order terms
            |v~ - v'| <= 6u v'
  coefficients (adam_coef).  (float)t is exact for t < 2^24.  Device powf is allowed a relative error of K u (K = 16, a stated
        condition: no accuracy table for it was at hand, a worse powf would be a finding of its own).  c_i = fl(1 - powf(b_i,
        t)) has the absolute error K u b_i^t of the power plus its own rounding, at most u, hence the relative error
            d_i = (K u b_i^t + u) / (1 - b_i^t)
        -- the cancellation of 1 - b^t at small t is what the d terms carry.  step_size~ = fl(lr / c_1): d_1 + u.
        rbc2~ = fl(1 / fl(sqrt(c_2))): d_2 / 2 + 2u  (sqrtf and the division are correctly rounded: hipcc's default).
  D~  = fl(fl(sqrt~(v~) rbc2~) + eps): sqrt of v~ (6u) gives 3u, its rounding u, rbc2~ d_2/2 + 2u, the product u: 7u + d_2/2 on
        the first summand; eps is an fp32 value, both summands are positive, the sum rounds once: 8u + d_2/2.
  U~  = fl(step_size~ fl(m~ / D~)): beside the error of m~, D~ gives 8u + d_2/2, the division u, step_size~ d_1 + u, the
        product u: 11u + d_1 + d_2/2, 12u with one u for every second-order term (d_i <= 154u at t = 1):
            |U~ - U| <= |U| (12u + d_1 + d_2/2) + lr / (1 - b1^t) 3u A / D
  p~  = fl(p - U~): one rounding of the result,
            |p~ - p'| <= u |p'| + |U| (12u + d_1 + d_2/2) + lr / (1 - b1^t) 3u A / D

The all-zero regime (g = m = v = 0) has no band: p must come back bit for bit and m' = v' = +0.  The bf16 shadow has none
either: it must equal, bit for bit, round-to-nearest-even of the device's OWN new p at every element, tail included.

An fp32 op-by-op emulation (emulate(), powf modelled as float64 pow rounded to fp32) stays inside these bands for every case
of the tables, and each of the wrong variants listed in VARIANTS leaves them (test_host_adam_sweep.py)."""
import numpy as np
import torch

U24 = 2.0 ** -24
K_POWF = 16


def F32(x):
    """The float64 value of the fp32 number nearest to x."""
    return float(np.float32(x))


# ----------------------------------------------------------------------------- hyper-parameters, modes, steps
SETS = ((1e-2, 0.9, 0.999, 1e-8), (1e-4, 0.9, 0.99, 1e-8))          # (lr, b1, b2, eps)
STEPS = (1, 2, 7, 1000, 100000)
COEF = 0.37                                                          # hyper[1] of the hyper mode
# name, S (raw gradients are the true ones times S), and what goes into dsr_adam_args
MODES = (
    dict(name="host", S=1.0, grad_scale=1.0),
    dict(name="host_gs", S=1024.0, grad_scale=2.0 ** -10),
    dict(name="scaler", S=65536.0, grad_scale=3.0, loss_scale=65536.0),            # grad_scale must NOT be read
    dict(name="hyper", S=1024.0, grad_scale=2.0 ** -10, hyper=True),               # {lr, COEF}; the block's own lr is not read
    dict(name="found0", S=1.0, grad_scale=1.0, found_inf=0.0),
)


def multiplier(mode):
    """gs as adam_resolve forms it, as a float64 holding an fp32 value."""
    gs = np.float32(mode["grad_scale"])
    if "loss_scale" in mode:
        gs = np.float32(1.0) / np.float32(mode["loss_scale"])
    if mode.get("hyper"):
        gs = np.float32(gs * np.float32(COEF))                      # ONE fp32 product
    return float(gs)


class Case:
    """One launch: sizes (one for dsr_pw_adam, a table for dsr_pw_adam_multi), byte offsets of p, g, m, v from a 16-byte
    boundary per tensor, shadow or not, and the rotated mode / step / hyper-parameter set."""

    def __init__(self, name, sizes, k, shadow=False, offs=None, seed=0):
        self.name, self.sizes, self.shadow, self.seed = name, list(sizes), shadow, seed
        self.offs = offs or [(0, 0, 0, 0)] * len(self.sizes)
        self.mode = MODES[k % 5]
        self.t = STEPS[(k // 5) % 5]
        self.lr, self.b1, self.b2, self.eps = (F32(x) for x in SETS[k % 2])
        self.gs = multiplier(self.mode)

    def hyp(self):
        return dict(t=self.t, lr=self.lr, b1=self.b1, b2=self.b2, eps=self.eps, gs=self.gs)

    def __repr__(self):
        return f"{self.name}[{self.mode['name']},t={self.t},lr={self.lr:.0e}]"


# ----------------------------------------------------------------------------- dsr_pw_adam: sizes and their launch geometry
PW_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1028, 2047, 2048, 2052, 4099, 13317, (1 << 20) + 3)
PW_CASES = [Case(f"pw{n}{'+sh' if sh else ''}", [n], 2 * i + sh, shadow=bool(sh), seed=1000 + 2 * i + sh)
            for i, n in enumerate(PW_SIZES) for sh in (0, 1)]
BIG_N = 65536 * 2048 + 2048 + 1024 + 4 + 3          # 134 220 807: past the grid cap
BIG_CASE = Case("pw_big+sh", [BIG_N], 18, shadow=True, seed=77)      # k = 18: t = 1000, mode hyper, set 0


def pw_geometry(n):
    """dsr_pw_adam / adam_stream restated: (blocks, passes of the grid-stride loop, vectors of the LAST pass handled as u = 0
    and as u = 1 per block, tail length).  A block handles 512 vectors per pass, two halves of 256."""
    n4 = n // 4
    want = (n4 + 511) // 512
    blocks = min(max(want, 1), 65536)
    per_pass = blocks * 512
    passes = -(-n4 // per_pass)
    last = n4 - (passes - 1) * per_pass if passes else 0
    halves = []                                       # (u0 vectors, u1 vectors) of each block with work in the last pass
    for b in range(-(-last // 512)):
        left = last - 512 * b
        halves.append((min(left, 256), min(max(left - 256, 0), 256)))
    return dict(blocks=blocks, passes=passes, halves=halves, tail=n % 4, n4=n4)


# ----------------------------------------------------------------------------- dsr_pw_adam_multi: tables and their groups
MT_CHUNK, MT_MAX = 4096, 64
MT_SIZES = (1, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8192, 8193, 40961)
MT_BIG = 40961                                       # 11 blocks; at slots 0, 63, 64: both sides of a group boundary
MT_COUNTS = (1, 64, 65, 129)


def _mt_table(count):
    sizes = [MT_SIZES[(5 * i + 3) % 11] for i in range(count)]       # every size but the last, in a stride-5 cycle
    for slot in (0, 63, 64):
        if slot < count:
            sizes[slot] = MT_BIG
    # independently for p, g, m, v: 0, 4, 8 or 12 bytes off a 16-byte boundary (base-4 digits of the index, v skewed)
    offs = [(4 * (i % 4), 4 * ((i // 4) % 4), 4 * ((i // 16) % 4), 4 * ((3 * i + 1) % 4)) for i in range(count)]
    return sizes, offs


MT_CASES = []
for _j, _c in enumerate(MT_COUNTS):
    _s, _o = _mt_table(_c)
    MT_CASES.append(Case(f"mt{_c}", _s, (6, 13, 22, 9)[_j], offs=_o, seed=2000 + _j))


def mt_groups(sizes):
    """mt_for_groups restated for dsr_pw_adam_multi: [(first_block list of the group, grid)], 64 tensors per launch."""
    out = []
    for s in range(0, len(sizes), MT_MAX):
        first, blocks = [], 0
        for n in sizes[s:s + MT_MAX]:
            first.append(blocks)
            blocks += -(-n // MT_CHUNK)
        out.append((first, blocks))
    return out


# ----------------------------------------------------------------------------- data: six regimes drawn per element
NORMAL, P_ZERO, P_SMALL, TINY, ALL_ZERO, G_ZERO, LARGE = range(7)
REGIMES = ("normal", "p=0", "p small", "tiny g", "all zero", "g=0", "large g")


def draw(n, seed, S, device="cpu"):
    """(p, raw g, m, v, regime) for n elements, fp32, each element's regime drawn from a seeded generator so that every
    position class (head, tail, block edge) meets every regime.  raw g = true g * S (S a power of two: exact)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    kw = dict(generator=gen, device=device, dtype=torch.float32)
    r = torch.randint(0, 7, (n,), generator=gen, device=device)
    sign = lambda: torch.rand(n, **kw).lt(0.5).to(torch.float32) * 2.0 - 1.0
    unif = lambda lo, hi: torch.rand(n, **kw) * (hi - lo) + lo
    p = torch.randn(n, **kw)
    p = torch.where(r == P_ZERO, torch.zeros_like(p), p)
    p = torch.where(r == P_SMALL, p * 1e-3, p)
    g = (1e-2 * torch.randn(n, **kw)).abs().clamp_min(1e-6) * sign()          # (no normal-regime gradient below the tiny ones)
    g = torch.where(r == TINY, sign() * torch.pow(10.0, unif(-9.0, -6.0)), g)
    g = torch.where(r == LARGE, sign() * 1e12 * unif(1.0, 2.0), g)
    m = g * unif(0.2, 2.0) * sign()
    v = (g * unif(0.2, 2.0)) ** 2
    zero = torch.zeros_like(g)
    g = torch.where((r == G_ZERO) | (r == ALL_ZERO), zero, g)
    m = torch.where(r == ALL_ZERO, zero, m)
    v = torch.where(r == ALL_ZERO, zero, v)
    return p, g * S, m, v, r


def case_data(case, device="cpu"):
    """[(p, g, m, v, regime)] per tensor of the case."""
    return [draw(n, case.seed * 131 + i, case.mode["S"], device) for i, n in enumerate(case.sizes)]


# ----------------------------------------------------------------------------- the reference and its bands
def adam_step(p, g, m, v, t, lr, b1, b2, eps, gs, K=K_POWF, bands=False):
    """One Adam step in float64: (p', m', v'), and with bands=True also (band_p, band_m, band_v).  Inputs of any float dtype
    on any device; hyper-parameters are the float64 values of the fp32 numbers the kernel is given."""
    p, g, m, v = (x.to(torch.float64) for x in (p, g, m, v))
    gk = g * gs
    A = b1 * m.abs() + (1.0 - b1) * gk.abs()
    m1 = b1 * m + (1.0 - b1) * gk
    v1 = b2 * v + (1.0 - b2) * gk * gk
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    D = v1.sqrt() / bc2 ** 0.5 + eps
    step = lr / bc1
    Uu = step * m1 / D
    p1 = p - Uu
    if not bands:
        return p1, m1, v1
    d1 = (K * U24 * b1 ** t + U24) / bc1
    d2 = (K * U24 * b2 ** t + U24) / bc2
    band_p = U24 * p1.abs() + Uu.abs() * (12 * U24 + d1 + d2 / 2) + step * 3 * U24 * A / D
    return p1, m1, v1, band_p, 3 * U24 * A, 6 * U24 * v1


def _ratio(got, ref, band):
    err = (got.to(torch.float64) - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))      # a NaN is outside every band
    return torch.where(err == 0, err, err / band)                                        # (0 / 0: inside; x / 0: outside)


def compare(got, inputs, regime, hyp):
    """got = (p, m, v) fp32 after the step, inputs = (p, g, m, v) before it.  Returns the per-element ratios |delta| / band of
    p, m, v (the all-zero regime's elements set to 0) and whether the all-zero regime came back bit for bit (p unchanged,
    m' = v' = +0)."""
    p1, m1, v1, bp, bm, bv = adam_step(*inputs, bands=True, **hyp)
    z = regime == ALL_ZERO
    zero_ok = bool((got[0].view(torch.int32)[z] == inputs[0].view(torch.int32)[z]).all()) and \
        bool((got[1].view(torch.int32)[z] == 0).all()) and bool((got[2].view(torch.int32)[z] == 0).all())
    out = []
    for x, ref, band in zip(got, (p1, m1, v1), (bp, bm, bv)):
        r = _ratio(x, ref, band)
        out.append(torch.where(z, torch.zeros_like(r), r))
    return out[0], out[1], out[2], zero_ok


def bf16_bits(x):
    """Round-to-nearest-even bf16 image of an fp32 tensor, as int16 (torch's own cast)."""
    return x.to(torch.bfloat16).view(torch.int16)


# ----------------------------------------------------------------------------- fp32 emulation of adam_coef / adam_update, and wrong variants
VARIANTS = ("eps_in_root", "eps_before_bc", "t+1", "t-1", "swap_betas", "v_g_gk", "old_m", "tail_skipped", "tail_twice",
            "shadow_truncated", "shadow_old_p")


def emulate(p, g, m, v, t, lr, b1, b2, eps, gs, variant=None):
    """One np.float32 operation per operation of the kernel; powf is float64 pow rounded to fp32.  numpy arrays in, (p, m, v)
    out.  `variant`: one of the arithmetic mistakes of VARIANTS."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    lr, b1, b2, eps, gs = f(lr), f(b1), f(b2), f(eps), f(gs)
    if variant == "t+1":
        t += 1
    if variant == "t-1":
        t -= 1
    if variant == "swap_betas":
        b1, b2 = b2, b1
    with np.errstate(all="ignore"):
        powf = lambda b: f(float(b) ** float(f(t)))
        step_size = lr / (f(1) - powf(b1))
        c2 = f(1) - powf(b2)
        rbc2 = f(1) / np.sqrt(c2)
        gk = g * gs
        m1 = b1 * m + (f(1) - b1) * gk
        v1 = b2 * v + (f(1) - b2) * (g if variant == "v_g_gk" else gk) * gk
        if variant == "eps_in_root":
            D = np.sqrt(v1 / c2 + eps)
        elif variant == "eps_before_bc":
            D = (np.sqrt(v1) + eps) * rbc2
        else:
            D = np.sqrt(v1) * rbc2 + eps
        p1 = p - step_size * ((m if variant == "old_m" else m1) / D)
    assert p1.dtype == m1.dtype == v1.dtype == f
    return p1, m1, v1


def emulate_launch(p, g, m, v, hyp, variant=None):
    """emulate() with the launch's structure: vector body and scalar tail (n % 4 elements), and the shadow.  Returns
    (p, m, v, shadow bits as int16)."""
    n = p.shape[0]
    arith = variant if variant not in ("tail_skipped", "tail_twice", "shadow_truncated", "shadow_old_p") else None
    p1, m1, v1 = emulate(p, g, m, v, variant=arith, **hyp)
    tail = slice(n - n % 4, n)
    if variant == "tail_skipped":
        p1[tail], m1[tail], v1[tail] = p[tail], m[tail], v[tail]
    if variant == "tail_twice":
        p1[tail], m1[tail], v1[tail] = emulate(p1[tail], g[tail], m1[tail], v1[tail], **hyp)
    src = np.asarray(p, dtype=np.float32) if variant == "shadow_old_p" else p1
    bits = src.view(np.uint32)
    if variant == "shadow_truncated":
        sh = bits >> 16
    else:
        sh = (bits + np.uint32(0x7FFF) + ((bits >> 16) & 1)) >> 16
    return p1, m1, v1, sh.astype(np.uint16).view(np.int16)


# ----------------------------------------------------------------------------- guarded buffers
GUARD32, GUARD16 = 0x7FC0BEEF, 0x7FCE


class Arena:
    """One buffer holding the given 1-D tensors (all fp32, or all 16-bit) between guard words, 16 bytes of them on each side of
    every tensor; tensor i starts offs[i] bytes after a 16-byte boundary.  Built on `dev` from data that may live anywhere."""

    def __init__(self, datas, offs, dev):
        es = datas[0].element_size()
        self.itype = torch.int32 if es == 4 else torch.int16
        self.guard_word = GUARD32 if es == 4 else GUARD16
        per16 = 16 // es
        pos, cur = [], 0
        for d, off in zip(datas, offs):
            assert off % es == 0 and 0 <= off < 16
            start = cur + per16
            start += (off // es - start) % per16
            pos.append(start)
            cur = start + d.numel()
        total = cur + per16
        self.buf = torch.full((total,), self.guard_word, dtype=self.itype, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.mask = torch.ones(total, dtype=torch.bool, device=dev)
        self.views = []
        for d, s, off in zip(datas, pos, offs):
            self.buf[s:s + d.numel()].copy_(d.view(self.itype))
            self.mask[s:s + d.numel()] = False
            view = self.buf[s:s + d.numel()].view(d.dtype)
            assert view.data_ptr() % 16 == off
            self.views.append(view)

    def guards_intact(self):
        return bool(((self.buf == self.guard_word) | ~self.mask).all())

    def snapshot(self):
        return self.buf.clone()

    def unchanged(self, snap):
        return bool((self.buf == snap).all())
