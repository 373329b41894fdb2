"""GPU: direct float64 / exact sweep of the metric kernels of csrc/metrics.hip through the raw C ABI (references, operand
generators, case tables and floors: metrics_ref.py; the references against the suite's restatements, the exactness of the
regimes, the branches the tables reach and the floors on the CPU: test_host_metrics_sweep.py).

A  forward tiles: every partial[block] of dsr_ssim_img_f32 and dsr_ssim_cs_img_f32 against the float64 sum of that
   tile, bar 4 x max(F(n), 1e-6 n) for a tile of n positions (F(n): the float32 CPU restatement's largest deviation on tiles of
   that size); the finalisers against the read-back partials folded in float64, within the summation-chain bound.
B  exact regime, no tolerance: identical images give partial == the tile's position count; an impulse changes exactly the tiles
   that hold a window position covering it; swapped images give the same bits.
C  backward per pixel: dsr_ssim_bwd_f32 and dsr_msssim_bwd_f32 against float64 autograd of metrics_ref.one_scale_loss, relative L2
   and largest per-pixel error over max|ref|, each 4 x max(its float32 CPU floor, 1e-6).
D  PSNR by equality on integer-valued operands; the finalise values within 1 fp32 ulp of float64; the running state exactly.
E  dsr_avgpool2_pair_f32 by equality on dyadic operands.        F  dsr_msssim_combine: vals by equality, the rest within 1 ulp.

Every output and every partial buffer of every call sits inside a sentinel-filled buffer (canaries.py) whose margins are checked
after the calls; outputs whose contract is "every element written" are pre-filled with NaN and none may survive.  The measured
figures (floors, the kernels' ratios) are printed before they are asserted."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import metrics_ref as R
from canaries import Canaries

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
F64, F32 = torch.float64, torch.float32
NAN = float("nan")
IMG = (R.SF_TH, R.SF_TW)
SHAPE_ID = lambda s: "x".join(map(str, s))


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits32(t):
    return t.contiguous().view(torch.int32)


class Calls:
    """The entry points, every output inside a canary buffer.  Operands stay alive until the canaries are checked."""

    def __init__(self, dev):
        self.L = P("_lib")
        self.lib = self.L.lib()
        self.dev, self.can, self.keep = dev, Canaries(dev), []

    def up(self, t, offset=0):
        """float64 tensor / float32 array -> float32 on the device, `offset` floats past a 16-byte boundary; None stays None."""
        if t is None:
            return None
        t = torch.as_tensor(t)
        out = t.to(F32)
        if t.dtype == F64:
            assert bool((out.to(F64) == t).all()), "operand not representable in float32"
        buf = torch.empty(out.numel() + offset, dtype=F32, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[offset:].view(out.shape)
        view.copy_(out)
        self.keep.append(buf)
        return view

    def out(self, shape, what, fill=NAN, dtype=F32):
        o = self.can.alloc(shape, dtype, what)
        if fill is not None:
            o.fill_(fill)
        return o

    def call(self, name, *args):
        self.L.check(getattr(self.lib, "dsr_" + name)(*args, stream()))

    # ---- the forward entry points
    def ssim_img(self, a, b, shape, per=True, total=None, scale=1.0, accumulate=0):
        n, c, h, w = shape
        blocks = self.lib.dsr_ssim_img_blocks(n, c, h, w)
        assert blocks == n * R.blocks_per_image(shape, *IMG)
        partial = self.out((blocks,), "ssim_img partial")
        per = self.out((n,), "ssim_img per_image") if per else None
        self.call("ssim_img_f32", ptr(a), ptr(b), n, c, h, w, R.C1, R.C2, ptr(partial), ptr(per), ptr(total), scale, accumulate)
        return partial, per

    def ssim_cs(self, a, b, shape, sim=True, cs=True):
        n, c, h, w = shape
        blocks = self.lib.dsr_ssim_cs_img_blocks(n, c, h, w)
        assert blocks == n * R.blocks_per_image(shape, *IMG)
        partial = self.out((2 * blocks,), "ssim_cs_img partial")
        sim = self.out((n,), "ssim_cs_img sim") if sim else None
        cs = self.out((n,), "ssim_cs_img cs") if cs else None
        self.call("ssim_cs_img_f32", ptr(a), ptr(b), n, c, h, w, R.C1, R.C2, ptr(partial), ptr(sim), ptr(cs))
        return partial, sim, cs


def cpu64(t):
    return t.detach().cpu().to(F64).numpy()


def no_nan(t, what):
    assert not bool(t.isnan().any()), what + ": an element was not written (NaN pre-fill survived)"


class Ratios:
    """The kernel's worst error over max(F(n), 1e-6 n) per tile size n, printed with F(n)."""

    def __init__(self, tile, what):
        self.tile, self.what, self.worst = tile, what, {}

    def add(self, got, ref, cnt, where, only=None):
        """got, ref: float64 arrays per block; cnt: positions per block; asserts the bar after recording the ratio."""
        err = np.abs(got - ref)
        bar = R.fwd_bar(cnt, *self.tile)
        ratio = err / (bar / R.MARGIN)
        sel = np.ones(len(cnt), dtype=bool) if only is None else only
        for n in np.unique(cnt[sel]):
            self.worst[int(n)] = max(self.worst.get(int(n), 0.0), float(ratio[sel & (cnt == n)].max()))
        bad = np.nonzero(sel & ~(err <= bar))[0]
        if len(bad):
            self.report()
        assert len(bad) == 0, (f"{where}: {len(bad)} tiles over the bar; first block {bad[0]} (n = {cnt[bad[0]]}): got {got[bad[0]]!r} "
                               f"ref {ref[bad[0]]!r} err {err[bad[0]]:.3e} bar {bar[bad[0]]:.3e}")

    def report(self):
        fl = R.fwd_floor(*self.tile)
        print(f"\n{self.what}: " + "; ".join(f"n {n}: F {fl[n]:.3e}, bar {R.MARGIN * max(fl[n], R.REL_FLOOR * n):.3e}, worst err / max(F, 1e-6 n) "
                                              f"{r:.3f}" for n, r in sorted(self.worst.items())))


# ============================================================================= A: forward tiles against float64
@pytest.mark.parametrize("shape", R.FWD_SHAPES, ids=SHAPE_ID)
def test_forward_tiles_vs_float64(dev, shape):
    """dsr_ssim_img_f32 and dsr_ssim_cs_img_f32: EVERY partial against the float64 sum of its tile (bar 4 x max(F(n), 1e-6 n)),
    then per_image / total (accumulate 0 and 1) / sim / cs against the read-back partials folded in float64, within
    (nblk + 8) 2^-24 sum |partial| inv_count (total: see metrics_ref.total_tolerance).  A null per_image, sim or cs leaves the
    other outputs the same bits.  Measured on the MI355X (printed by this test): F(1) 1.7e-5, F(4) 9.6e-6, F(16) 1.2e-4, F(64)
    1.8e-4, F(128) 5.6e-5, F(1024) 9.8e-4; the kernels' worst error over max(F(n), 1e-6 n): 0.52, 0.57, 0.29, 0.40, 0.24, 0.25."""
    n, c, h, w = shape
    k = Calls(dev)
    a, b = R.fwd_case(shape)
    ad, bd = k.up(a), k.up(b)
    ref = R.fwd_reference(shape, *IMG)
    cnt = ref["cnt"].numpy()
    nblk = R.blocks_per_image(shape, *IMG)
    tot0 = k.out((1,), "ssim_img total", 3.0)
    tot1 = k.out((1,), "ssim_img total", 3.0)
    part, per = k.ssim_img(ad, bd, shape, total=tot0, scale=0.5, accumulate=0)
    part1, _ = k.ssim_img(ad, bd, shape, per=False, total=tot1, scale=0.5, accumulate=1)
    pcs, sim, cs = k.ssim_cs(ad, bd, shape)
    pcs_s, sim_only, _ = k.ssim_cs(ad, bd, shape, cs=False)
    pcs_c, _, cs_only = k.ssim_cs(ad, bd, shape, sim=False)
    k.can.check()
    for t, what in ((part, "partial"), (per, "per_image"), (pcs, "cs partial"), (sim, "sim"), (cs, "cs")):
        no_nan(t, f"{shape} {what}")
    assert torch.equal(bits32(part), bits32(part1)) and torch.equal(bits32(pcs), bits32(pcs_s)) and torch.equal(bits32(pcs), bits32(pcs_c))
    assert torch.equal(bits32(sim), bits32(sim_only)) and torch.equal(bits32(cs), bits32(cs_only))
    got, gcs = cpu64(part), cpu64(pcs).reshape(-1, 2)
    rat = Ratios(IMG, f"forward {shape}")
    rat.add(got, ref["sim"].numpy(), cnt, f"ssim_img {shape}")
    rat.add(gcs[:, 0], ref["sim"].numpy(), cnt, f"ssim_cs_img {shape} ssim sums")
    rat.add(gcs[:, 1], ref["cs"].numpy(), cnt, f"ssim_cs_img {shape} cs sums")
    rat.report()
    # the finalisers against the partials they read
    inv = R.f32(1.0 / (c * (h - 10) * (w - 10)))
    for out, parts, what in ((per, got, "per_image"), (sim, gcs[:, 0], "sim"), (cs, gcs[:, 1], "cs")):
        o = cpu64(out)
        for i in range(n):
            p = parts[i * nblk:(i + 1) * nblk]
            want, tol = p.sum() * inv, R.fold_tolerance(p, nblk, inv)
            assert abs(o[i] - want) <= tol, f"{shape} {what}[{i}]: got {o[i]!r} want {want!r} tol {tol:.3e}"
    want = 0.5 * got.sum() * inv
    for tot, base in ((tot0, 0.0), (tot1, 3.0)):
        tol = R.total_tolerance(got, n, nblk, inv, 0.5, base + want)
        assert abs(float(tot[0]) - (base + want)) <= tol, f"{shape} total (held {base}): got {float(tot[0])!r} want {base + want!r} tol {tol:.3e}"


# ============================================================================= B: the exact regime
@pytest.mark.parametrize("shape", R.FWD_SHAPES, ids=SHAPE_ID)
def test_identical_and_swapped_images_exact(dev, shape):
    """Identical images: every partial of dsr_ssim_img_f32 and both partials of dsr_ssim_cs_img_f32 EQUAL the number of in-image
    positions of their tile (an exact test of the masks and the grid), for both images of the pair.  Swapped images: the same
    bits."""
    k = Calls(dev)
    a, b = R.fwd_case(shape)
    ad, bd = k.up(a), k.up(b)
    cnt = R.tile_counts(shape, *IMG).to(F32)
    outs = []
    for x in (ad, bd):
        outs.append((k.ssim_img(x, x, shape)[0], cnt))
        outs.append((k.ssim_cs(x, x, shape)[0], cnt.repeat_interleave(2)))
    ab, ba = k.ssim_img(ad, bd, shape)[0], k.ssim_img(bd, ad, shape)[0]
    cab, cba = k.ssim_cs(ad, bd, shape)[0], k.ssim_cs(bd, ad, shape)[0]
    k.can.check()
    for got, want in outs:
        bad = (got.cpu() != want).nonzero()
        assert len(bad) == 0, f"{shape}: {len(bad)} partials differ from their tile's count; first {bad[:4].flatten().tolist()}: " \
                              f"got {got.cpu()[bad[0]].tolist()} want {want[bad[0]].tolist()}"
    assert torch.equal(bits32(ab), bits32(ba)), f"{shape}: ssim_img(a, b) and (b, a) differ"
    assert torch.equal(bits32(cab), bits32(cba)), f"{shape}: ssim_cs_img(a, b) and (b, a) differ"
    assert not torch.equal(bits32(ab), bits32(outs[0][0]))


@pytest.mark.parametrize("shape", R.FWD_SHAPES, ids=SHAPE_ID)
def test_impulse_changes_exactly_its_tiles(dev, shape):
    """b = a except one pixel of the last plane (+0.25), at both image corners and at the four pixels around an interior tile
    corner: exactly the tiles that hold a window position covering the pixel may differ from their count -- each of them does,
    and meets the bar of A against float64 -- and every other tile equals its count bit for bit."""
    cnt = R.tile_counts(shape, *IMG)
    rat = Ratios(IMG, f"impulse {shape}")
    for y, x in R.impulse_pixels(shape, *IMG):
        k = Calls(dev)
        a, b, _ = R.impulse_case(shape, y, x)
        ad, bd = k.up(a), k.up(b)
        part = k.ssim_img(ad, bd, shape)[0]
        pcs = k.ssim_cs(ad, bd, shape)[0]
        k.can.check()
        hit = R.impulse_tiles(shape, y, x, *IMG)
        assert 1 <= int(hit.sum()) <= 4
        sim, cs = R.fwd_maps(a, b)
        got, gcs = part.cpu(), pcs.cpu().view(-1, 2)
        for g, m, what in ((got, sim, "ssim_img"), (gcs[:, 0], sim, "ssim_cs_img ssim"), (gcs[:, 1], cs, "ssim_cs_img cs")):
            same = g == cnt.to(F32)
            assert bool(same[~hit].all()), f"{shape} impulse {(y, x)} {what}: tiles {(~same & ~hit).nonzero().flatten().tolist()} changed, " \
                                           f"only {hit.nonzero().flatten().tolist()} may"
            rat.add(g.to(F64).numpy(), R.tile_sums(m, *IMG)[0].numpy(), cnt.numpy(), f"{what} {shape} impulse {(y, x)}", only=hit.numpy())
    rat.report()


# ============================================================================= C: backward, per pixel
def _bwd(k, shape, which, ops, ms):
    """One launch: (grad1, grad2) in NaN-filled canary buffers (None where not asked for)."""
    n, c, h, w = shape
    a, b, g, ws, wc, ca, cb = ops
    ad, bd, gd = k.up(a), k.up(b), k.up(g)
    g1 = k.out(shape, "grad1") if which & 1 else None
    g2 = k.out(shape, "grad2") if which & 2 else None
    if ms:
        k.call("msssim_bwd_f32", ptr(ad), ptr(bd), n, c, h, w, R.C1, R.C2, ptr(gd), ptr(k.up(ws)), ptr(k.up(wc)), ptr(k.up(ca)), ptr(k.up(cb)),
               ptr(g1), ptr(g2))
    else:
        k.call("ssim_bwd_f32", ptr(ad), ptr(bd), n, c, h, w, R.C1, R.C2, ptr(gd), ptr(g1), ptr(g2))
    return g1, g2


class Worst:
    def __init__(self):
        self.v = [0.0, 0.0, 0.0, 0.0]           # floor l2, ratio l2, floor max, ratio max

    def check(self, got, ref, what):
        r64, fl2, fmx = ref
        no_nan(got, what)
        g = got.cpu()
        e2, em = R.rel_l2(g, r64), R.rel_max(g, r64)
        b2, bm = R.bwd_bars(fl2, fmx)
        r2, rm = e2 / (b2 / R.MARGIN), em / (bm / R.MARGIN)
        self.v = [max(self.v[0], fl2), max(self.v[1], r2), max(self.v[2], fmx), max(self.v[3], rm)]
        line = (f"{what}: rel L2 {e2:.3e} floor {fl2:.3e} bar {b2:.3e} ratio {r2:.3f}; per pixel / max|ref| {em:.3e} floor {fmx:.3e} "
                f"bar {bm:.3e} ratio {rm:.3f}")
        print(line)
        assert e2 <= b2 and em <= bm, line
        return bm * float(r64.abs().max())

    def report(self, what):
        print(f"\n{what}: largest float32 floor rel L2 {self.v[0]:.3e}, per pixel {self.v[2]:.3e}; worst err / max(floor, 1e-6): rel L2 "
              f"{self.v[1]:.3f}, per pixel {self.v[3]:.3f}")


@pytest.mark.parametrize("shape", R.BWD_SHAPES, ids=SHAPE_ID)
def test_ssim_bwd_vs_float64_autograd(dev, shape):
    """dsr_ssim_bwd_f32 with grad1 only, grad2 only and both (3 and 4 coefficient maps), g differing per image with both signs:
    relative L2 within 4 x max(floor, 1e-6) and the largest per-pixel error over max|ref| within 4 x max(its floor, 1e-6), the
    floors being float32 CPU autograd of the same loss against float64; every element written.  Measured on the MI355X, this
    test and the multi-scale one: relative-L2 floors 2.3e-7 .. 1.7e-5, kernels at 0.35 .. 0.57 of max(floor, 1e-6); per-pixel
    floors 2.2e-7 .. 6.0e-5, kernels at 0.35 .. 0.81."""
    worst = Worst()
    for which in R.WHICH:
        k = Calls(dev)
        grads = _bwd(k, shape, which, R.bwd_operands(shape, which, None, "none"), ms=False)
        k.can.check()
        for i, (got, ref) in enumerate(zip(grads, R.bwd_reference(shape, which, None, "none"))):
            assert (got is None) == (ref is None)
            if got is not None:
                worst.check(got, ref, f"ssim_bwd {shape} grad{i + 1} of {which}")
    worst.report(f"ssim_bwd {shape}")


@pytest.mark.parametrize("shape", R.BWD_SHAPES, ids=SHAPE_ID)
def test_msssim_bwd_vs_float64_autograd(dev, shape):
    """dsr_msssim_bwd_f32 at every (which, weights, coarse) of ms_cases(): w_sim only, w_cs only, both; no coarse gradient, one
    per asked image, and one for only one of two asked images; odd H and W leave the dropped row and column without a coarse
    share (the float64 avg_pool2d reference has none there).  The two bars of test_ssim_bwd_vs_float64_autograd."""
    worst = Worst()
    for s, which, weights, coarse in R.ms_cases():
        if s != shape:
            continue
        k = Calls(dev)
        grads = _bwd(k, shape, which, R.bwd_operands(shape, which, weights, coarse), ms=True)
        k.can.check()
        for i, (got, ref) in enumerate(zip(grads, R.bwd_reference(shape, which, weights, coarse))):
            assert (got is None) == (ref is None)
            if got is not None:
                worst.check(got, ref, f"msssim_bwd {shape} grad{i + 1} of {which} weights {weights} coarse {coarse}")
    worst.report(f"msssim_bwd {shape}")


@pytest.mark.parametrize("shape", R.BWD_SHAPES, ids=SHAPE_ID)
def test_bwd_impulse_is_local(dev, shape):
    """b = a except one pixel (+0.25): outside the 21 x 21 pixels around it -- and in every other plane -- the float64 gradient
    is zero.  The kernels' values there are float32 rounding of a vanishing derivative, NOT exactly zero; they are required to
    stay within the per-pixel bar (4 x max(floor, 1e-6) x max|ref|), as is every pixel.  At an image corner one window position
    reaches the pixel with weight 1e-6, the floor exceeds 1 and the bar says little; at a tile corner the floor is 1e-3."""
    worst = Worst()
    for y, x in R.bwd_impulse_pixels(shape):
        far = R.far_from_impulse(shape, y, x)
        for ms, weights in ((False, None), (True, "both")):
            k = Calls(dev)
            grads = _bwd(k, shape, 3, R.bwd_operands(shape, 3, weights, "none", (y, x)), ms=ms)
            k.can.check()
            for i, (got, ref) in enumerate(zip(grads, R.bwd_reference(shape, 3, weights, "none", (y, x)))):
                what = f"{'msssim' if ms else 'ssim'}_bwd {shape} impulse {(y, x)} grad{i + 1}"
                bar_abs = worst.check(got, ref, what)
                if bool(far.any()):
                    out = float(got.cpu()[far].abs().max())
                    print(f"{what}: largest |value| away from the impulse {out:.3e} (float64: 0), bar {bar_abs:.3e}")
                    assert out <= bar_abs + 1e-15, what
    worst.report(f"bwd impulse {shape}")


# ============================================================================= D: PSNR, by equality
def _stats(k, p, t, offset=0):
    n, e = t.shape
    blocks = k.lib.dsr_psnr_blocks(n, e)
    assert blocks == n * -(-e // R.PSNR_CHUNK)
    sse = k.out((blocks,), "psnr partial_sse")
    keys = k.out((2 * blocks,), "psnr partial_keys", fill=None, dtype=torch.int32)
    pd, td = k.up(p, offset), k.up(t, offset)
    assert (pd.data_ptr() % 16 == 0) == (offset % 4 == 0)
    k.call("psnr_stats_f32", ptr(pd), ptr(td), n, e, ptr(sse), ptr(keys))
    return sse, keys


def _keys_np(keys):
    return keys.cpu().numpy().view(np.uint32).reshape(-1, 2)


@pytest.mark.parametrize("e", R.PSNR_E)
def test_psnr_stats_exact(dev, e):
    """dsr_psnr_stats_f32 at every (N, E, offset) of psnr_cases(): integer-valued errors |d| <= 15, so partial_sse EQUALS the
    float64 sum of its chunk; both keys of every block EQUAL the ordered keys of the chunk's target min and max, with -0.0, +0.0,
    +-subnormals and negatives in the target (also across the chunk edges).  The vectorised form (E % 4 == 0, aligned) and the
    scalar form reached two ways (E % 4 != 0; E % 4 == 0 with both inputs one float off alignment) give the same reference."""
    for n, ee, off in R.psnr_cases():
        if ee != e:
            continue
        k = Calls(dev)
        p, t = R.psnr_case(n, e)
        sse, keys = _stats(k, p, t, off)
        k.can.check()
        no_nan(sse, f"psnr N {n} E {e} partial_sse")
        want_sse, want_keys = R.psnr_partials(p, t)
        got, gk = cpu64(sse), _keys_np(keys)
        what = f"psnr_stats N {n} E {e} offset {off} ({R.psnr_form(e, off)})"
        bad = np.nonzero(got != want_sse)[0]
        assert len(bad) == 0, f"{what}: partial_sse of blocks {bad[:6].tolist()}: got {got[bad[:6]].tolist()} want {want_sse[bad[:6]].tolist()}"
        bad = np.nonzero((gk != want_keys).any(axis=1))[0]
        assert len(bad) == 0, (f"{what}: keys of blocks {bad[:6].tolist()}: got {[hex(v) for v in gk[bad[0]]]} (floats {R.metric_unkey(gk[bad[0]]).tolist()}) "
                               f"want {[hex(v) for v in want_keys[bad[0]]]} (floats {R.metric_unkey(want_keys[bad[0]]).tolist()})")


FIN_CASES = [(1, 5), (2, 16385), (17, 32772), (33, 16388), (1, 65 * 16384 + 4), (17, 4)]


@pytest.mark.parametrize("n,e", FIN_CASES)
def test_psnr_finalize_values(dev, n, e):
    """dsr_psnr_finalize on the partials of dsr_psnr_stats_f32, base 10 and 2: per-image mode (per_image[n], value = value_scale
    x their sum, state[0..1]) and batch mode with the range given and inferred -- every value within 1 fp32 ulp of the float64
    formula; the batch state EQUALS (SSE, N E, min, max); the per-image state counts N exactly and leaves words 2, 3 alone."""
    k = Calls(dev)
    p, t = R.psnr_case(n, e)
    sse, keys = _stats(k, p, t)
    rs, rk = R.psnr_partials(p, t)
    todo = []
    for ls in R.LOG_SCALES:
        per, val = k.out((n,), "psnr per_image"), k.out((1,), "psnr value")
        st = k.out((4,), "psnr state", fill=None, dtype=F64)
        st[:2] = 0.0
        k.call("psnr_finalize", ptr(sse), ptr(keys), n, e, 0, 2.5, ls, ptr(per), ptr(val), 1.0 / n, ptr(st))
        ref = R.psnr_per_image(rs, n, e, 2.5, ls)
        todo.append(("per", per, val, st, ref, None))
        for infer in (0, 1):
            val, st = k.out((1,), "psnr value"), k.out((4,), "psnr state", 0.0, dtype=F64)
            k.call("psnr_finalize", ptr(sse), ptr(keys), n, e, infer, 0.0 if infer else 2.5, ls, None, ptr(val), 1.0, ptr(st))
            todo.append(("batch", None, val, st, R.psnr_batch(rs, rk, n, e, infer, 2.5, ls), infer))
    k.can.check()
    for mode, per, val, st, ref, infer in todo:
        what = f"psnr_finalize N {n} E {e} {mode} infer {infer}"
        state = st.cpu().tolist()
        if mode == "per":
            assert R.within_ulp32(per.cpu().numpy(), ref), f"{what}: per_image {per.cpu().tolist()[:4]} want {ref[:4].tolist()}"
            assert R.within_ulp32(val.cpu().numpy(), np.array([R.f32(1.0 / n) * ref.sum()])), what
            assert state[1] == float(n) and abs(state[0] - ref.sum()) <= 1e-12 * np.abs(ref).sum() and k.can.untouched(st[2:]), (what, state)
        else:
            assert R.within_ulp32(val.cpu().numpy(), np.array([ref[0]])), f"{what}: value {float(val[0])!r} want {ref[0]!r}"
            assert state == R.psnr_state_after([0.0, 0.0, 0.0, 0.0], ref), (what, state)


def test_psnr_running_state_and_compute(dev):
    """Three batch-mode finalises whose targets move the running minimum (shift -30), then the maximum (+40): state[0..3] EQUAL
    the float64 fold after every call; dsr_metric_compute mode 2 on it within 1 fp32 ulp (range inferred and given, base 10 and
    2), modes 0 and 1 by equality (a float64 value rounded once)."""
    n, e = 2, 32772
    k = Calls(dev)
    st = k.out((4,), "psnr state", 0.0, dtype=F64)
    want = [0.0, 0.0, 0.0, 0.0]
    outs = []
    for shift in (0, -30, 40):
        p, t = R.psnr_case(n, e, shift)
        sse, keys = _stats(k, p, t)
        k.call("psnr_finalize", ptr(sse), ptr(keys), n, e, 1, 0.0, R.LOG_SCALES[0], None, ptr(k.out((1,), "psnr value")), 1.0, ptr(st))
        rs, rk = R.psnr_partials(p, t)
        moved = want[2:]
        want = R.psnr_state_after(want, R.psnr_batch(rs, rk, n, e, 1, 0.0, R.LOG_SCALES[0]))
        assert shift == 0 or moved != want[2:]
        assert st.cpu().tolist() == want, (shift, st.cpu().tolist(), want)
        for mode in (0, 1, 2):
            for infer in ((0, 1) if mode == 2 else (0,)):
                for ls in (R.LOG_SCALES if mode == 2 else R.LOG_SCALES[:1]):
                    o = k.out((1,), "metric_compute out")
                    k.call("metric_compute", ptr(st), mode, infer, 2.5, ls, ptr(o))
                    ref = want[0] if mode == 0 else want[0] / want[1] if mode == 1 else R.psnr_of_state(want, infer, 2.5, ls)
                    outs.append((o, mode, ref, (shift, mode, infer, ls)))
    k.can.check()
    assert want[2] < -30 and want[3] > 40
    for o, mode, ref, what in outs:
        if mode == 2:
            assert R.within_ulp32(o.cpu().numpy(), np.array([ref])), (what, float(o[0]), ref)
        else:
            assert float(o[0]) == R.f32(ref), (what, float(o[0]), ref)


@pytest.mark.parametrize("n", R.ACC_N)
def test_metric_accumulate_exact(dev, n):
    """dsr_metric_accumulate on multiples of 1/1024 (every partial sum exact in double): state EQUALS (s0 + sum, s1 + N) after
    one call and after a second one."""
    k = Calls(dev)
    v = R.acc_case(n)
    st = k.out((2,), "metric state", fill=None, dtype=F64)
    st.copy_(torch.tensor([1.5, 3.0], dtype=F64))
    vd = k.up(v)
    s = float(v.astype(np.float64).sum())
    k.call("metric_accumulate", ptr(vd), n, ptr(st))
    once = st.cpu().tolist()
    k.call("metric_accumulate", ptr(vd), n, ptr(st))
    k.can.check()
    assert once == [1.5 + s, 3.0 + n] and st.cpu().tolist() == [1.5 + 2 * s, 3.0 + 2 * n], (once, st.cpu().tolist(), s)


# ============================================================================= E: the 2 x 2 mean pool of a pair
@pytest.mark.parametrize("planes,h,w,offset", R.POOL_CASES)
def test_avgpool2_pair_exact(dev, planes, h, w, offset):
    """dsr_avgpool2_pair_f32 on dyadic inputs (in1 != in2, so a wrong image pick shows): out1, out2 EQUAL float64 avg_pool2d; an
    odd last row / column is dropped; inputs one float off alignment take the scalar form on a V4 shape."""
    k = Calls(dev)
    x1, x2 = R.pool_case(planes, h, w)
    o1, o2 = k.out((planes, h // 2, w // 2), "pool out1"), k.out((planes, h // 2, w // 2), "pool out2")
    k.call("avgpool2_pair_f32", ptr(k.up(x1, offset)), ptr(k.up(x2, offset)), ptr(o1), ptr(o2), planes, h, w)
    k.can.check()
    for got, x, what in ((o1, x1, "out1"), (o2, x2, "out2")):
        no_nan(got, what)
        want = R.pool_ref(x)
        bad = (got.cpu().to(F64) != want).nonzero()
        assert len(bad) == 0, f"avgpool2_pair {(planes, h, w)} offset {offset} ({R.pool_form(w, offset)}) {what}: {len(bad)} differ, first {bad[0].tolist()}"


# ============================================================================= F: combine
def _combine(k, raw_d, n, L, normalize, vals=True, factors=True, total=True, per=True):
    bt = (C.c_float * L)(*R.BETAS8[:L])
    v = k.out((L, n), "combine vals") if vals else None
    f = k.out((L, n), "combine factors") if factors else None
    t = k.out((1,), "combine total") if total else None
    p = k.out((n,), "combine per_image") if per else None
    k.call("msssim_combine", ptr(raw_d), n, L, bt, normalize, ptr(v), ptr(p), ptr(t), 0.25, ptr(f))
    return v, p, t, f


@pytest.mark.parametrize("normalize", R.NORMALIZE)
def test_msssim_combine(dev, normalize):
    """dsr_msssim_combine at N = 1, 255, 256, 257, 600 x L = 1, 3, 5, 8, raw values with exact +0, -0 and negatives: vals EQUAL the
    float32 operation (a zero's sign is free: max(-0, +0) may return either, an arithmetic freedom of fmaxf, not a defect);
    per_image, factors and total within 1 fp32 ulp of float64 (NaN exactly where the plain arithmetic has NaN: normalize 0 at a
    negative or zero value); under relu an image with a non-positive scale has value exactly 0 and all factors exactly 0; null
    vals / factors / total / per_image each leave the other outputs the same bits."""
    for n in R.COMBINE_N:
        for L in R.COMBINE_L:
            k = Calls(dev)
            raw = R.combine_case(n, L)
            rd = k.up(raw)
            full = _combine(k, rd, n, L, normalize)
            variants = [(_combine(k, rd, n, L, normalize, vals=False), 0), (_combine(k, rd, n, L, normalize, factors=False), 3),
                        (_combine(k, rd, n, L, normalize, total=False), 2), (_combine(k, rd, n, L, normalize, per=False), 1)]
            k.can.check()
            what = f"combine N {n} L {L} normalize {normalize}"
            for t in full:
                assert t is not None
            for outs, dropped in variants:
                for i, (x, y) in enumerate(zip(outs, full)):
                    if i != dropped:
                        assert torch.equal(bits32(x), bits32(y)), f"{what}: output {i} changed when output {dropped} was null"
            vals, per, tot, fac = (t.cpu().numpy() for t in full)
            out, rv, rf = R.combine(raw, R.BETAS8[:L], normalize)
            assert not np.isnan(vals).any() and np.array_equal(vals, rv), f"{what}: vals"
            assert R.within_ulp32(per, out), f"{what}: per_image"
            assert R.within_ulp32(fac, rf), f"{what}: factors"
            # total = total_scale x the sum of the ROUNDED per-image values, in double, rounded once
            assert R.within_ulp32(tot, np.array([0.25 * per.astype(np.float64).sum()])), f"{what}: total {tot} per-image sum {per.sum()}"
            if normalize == 1:
                dead = (raw <= 0).any(axis=0)
                assert n == 1 or (dead.any() and not dead.all())
                assert not per[dead].any() and not fac[:, dead].any() and bool((per[~dead] > 0).all()) and bool((fac[:, ~dead] > 0).all()), what
            if normalize == 0 and n > 1:
                assert np.isnan(per).any() and not np.isnan(per).all()
