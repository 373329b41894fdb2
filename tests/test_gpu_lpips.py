"""GPU: LPIPS (AlexNet) on the HIP path (deep-super-resolution_amd/lpips.py, csrc/lpips.hip) against the float64 restatement
of tests/lpips_ref.py -- the three new kernels one by one, then the whole metric, its launches, the evaluation loop and the
error paths."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as TF

import lpips_ref

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _prep(dev, a, b, normalize):
    L = P("_lib")
    m = P("lpips")
    n, _, h, w = a.shape
    (oh, ow) = m.LPIPS().tap_sizes(h, w)[0]
    out = torch.empty((2 * n, oh + 2, ow + 2, 64), dtype=torch.float16, device=dev)
    rng = torch.tensor([-1, 0], dtype=torch.int32, device=dev)
    L.check(L.lib().dsr_lpips_stem_prep(L.F16, _ptr(a), _ptr(b), n, h, w, int(normalize), _ptr(out), _ptr(rng), _st()))
    torch.cuda.synchronize()
    return out.cpu(), [m._decode_key(k) for k in rng.tolist()]


def _cpu_prep(x, normalize, bh, bw):
    return lpips_ref.space_to_depth(TF.pad(lpips_ref.scale_input(x, normalize), (2, 2, 2, 2)), bh, bw)


SIZES = [(31, 31), (64, 64), (97, 131), (130, 66)]


@pytest.mark.parametrize("normalize", [False, True])
def test_stem_prep_matches_cpu(dev, normalize):
    """Scaling + pad + 4x4 space-to-depth within one fp16 ulp of the float64 value; the range pair is the inputs' min / max."""
    g = torch.Generator().manual_seed(11)
    for h, w in SIZES + [(33, 35)]:
        lo = 0.0 if normalize else -1.0
        a = torch.rand(2, 3, h, w, generator=g) * (1 - lo) + lo
        b = torch.rand(2, 3, h, w, generator=g) * (1 - lo) + lo
        got, (mn, mx) = _prep(dev, a.to(dev), b.to(dev), normalize)
        ref = torch.cat([_cpu_prep(a, normalize, got.shape[1], got.shape[2]), _cpu_prep(b, normalize, got.shape[1], got.shape[2])])
        ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))) - 10)
        assert bool(((got.double() - ref).abs() <= ulp).all()), (h, w)
        assert bool((got[..., 48:] == 0).all())
        both = torch.cat([a, b])
        assert (mn, mx) == (float(both.min()), float(both.max())), (h, w)


def test_stem_conv_through_prep(dev):
    """The 3x3 conv over the prepared tensor with the regrouped weight == conv2d(stride 4, pad 2) of the same fp16-rounded
    scaled input, + bias, ReLU (fp32 reference, the conv's own fp16 weights)."""
    L, m = P("_lib"), P("lpips")
    mod = m.LPIPS()
    g = torch.Generator().manual_seed(12)
    for h, w in SIZES:
        a = (torch.rand(1, 3, h, w, generator=g) * 2 - 1).to(dev)
        b = (torch.rand(1, 3, h, w, generator=g) * 2 - 1).to(dev)
        oh, ow = mod.tap_sizes(h, w)[0]
        x = torch.empty((2, oh + 2, ow + 2, 64), dtype=torch.float16, device=dev)
        rng = torch.tensor([-1, 0], dtype=torch.int32, device=dev)
        lib = L.lib()
        L.check(lib.dsr_lpips_stem_prep(L.F16, _ptr(a), _ptr(b), 1, h, w, 0, _ptr(x), _ptr(rng), _st()))
        wf = mod._weights(dev)[0]
        d = L.ConvDesc(L.F16, 2, oh + 2, ow + 2, 64, 64, 3, 3, 1, 0, L.PAD_ZERO)
        y = torch.empty((2, oh, ow, 64), dtype=torch.float16, device=dev)
        ep = L.Epilogue(L.ACT_RELU, 0.0, None, _ptr(mod.b1), None, 0, None)
        L.check(lib.dsr_conv_fwd(ctypes.byref(d), _ptr(x), _ptr(wf), ctypes.byref(ep), _ptr(y), _st()))
        torch.cuda.synchronize()
        xin = lpips_ref.scale_input(torch.cat([a, b]).cpu()).half().float()
        w11 = m._standin_alex_state()["0.weight"].half().float()
        ref = TF.relu(TF.conv2d(xin, w11, m._standin_alex_state()["0.bias"], stride=4, padding=2)).permute(0, 2, 3, 1)
        err = float((y.cpu().float() - ref).abs().max() / ref.abs().max())
        assert err < 4e-3, (h, w, err)


@pytest.mark.parametrize("h,w", [(63, 63), (64, 80), (127, 255)])
@pytest.mark.parametrize("cp", [64, 192])
def test_maxpool3s2_bit_exact(dev, h, w, cp):
    L = P("_lib")
    g = torch.Generator().manual_seed(h + w + cp)
    x = torch.randn(2, h, w, cp, generator=g).half()
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    xd = x.to(dev)
    y = torch.empty((2, oh, ow, cp), dtype=torch.float16, device=dev)
    L.check(L.lib().dsr_maxpool3s2_fwd(L.F16, _ptr(xd), _ptr(y), 2, h, w, cp, _st()))
    ref = TF.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).half()
    assert torch.equal(y.cpu(), ref)


def test_maxpool3s2_rejects_empty_output(dev):
    L = P("_lib")
    x = torch.zeros((1, 2, 9, 64), dtype=torch.float16, device=dev)
    assert L.lib().dsr_maxpool3s2_fwd(L.F16, _ptr(x), _ptr(x), 1, 2, 9, 64, _st()) == -1
    assert b"smaller than the 3x3 window" in L.lib().dsr_last_error()


def _distance(dev, feats, lins, n):
    """[N] per-image distances of the device kernels for NHWC fp16 maps [2N][h][w][C] (one per tap)."""
    L = P("_lib")
    lib = L.lib()
    k = len(feats)
    hw = (ctypes.c_int * k)(*[f.shape[1] * f.shape[2] for f in feats])
    cp = (ctypes.c_int * k)(*[f.shape[3] for f in feats])
    blocks = lib.dsr_lpips_distance_blocks(k, hw, n)
    part = torch.empty(blocks, dtype=torch.float32, device=dev)
    fp = (ctypes.c_void_p * k)(*[f.data_ptr() for f in feats])
    lw = (ctypes.c_void_p * k)(*[w.data_ptr() for w in lins])
    L.check(lib.dsr_lpips_distance(L.F16, k, fp, lw, hw, cp, cp, n, _ptr(part), _st()))
    per = torch.empty(n, dtype=torch.float32, device=dev)
    tot = torch.empty(1, dtype=torch.float32, device=dev)
    L.check(lib.dsr_lpips_finalize(k, hw, n, _ptr(part), _ptr(per), _ptr(tot), 1.0 / n, 0, _st()))
    torch.cuda.synchronize()
    return per.cpu(), float(tot)


def test_distance_kernel_vs_float64(dev):
    """Random ReLU-like features (a quarter of the pixels all zero, as dead ReLUs give) against float64; exactly 0 for
    identical maps; bit-identical when the images are swapped."""
    g = torch.Generator().manual_seed(21)
    n = 3
    shapes = [(37, 41, 64), (18, 20, 192), (8, 9, 384), (8, 9, 256), (8, 9, 256)]
    f1, f2, lins = [], [], []
    for h, w, c in shapes:
        a = TF.relu(torch.randn(n, h, w, c, generator=g)).half()
        b = TF.relu(torch.randn(n, h, w, c, generator=g)).half()
        a[:, ::2, ::2] = 0
        b[:, ::2, ::2] = 0
        f1.append(a)
        f2.append(b)
        lins.append(torch.rand(c, generator=g))
    ref = lpips_ref.distance_from_features([a.permute(0, 3, 1, 2) for a in f1], [b.permute(0, 3, 1, 2) for b in f2], lins)
    lw = [w.to(dev) for w in lins]
    ab = [torch.cat([a, b]).to(dev) for a, b in zip(f1, f2)]
    ba = [torch.cat([b, a]).to(dev) for a, b in zip(f1, f2)]
    aa = [torch.cat([a, a]).to(dev) for a in f1]
    per, tot = _distance(dev, ab, lw, n)
    assert float(((per.double() - ref).abs() / ref).max()) < 1e-4
    assert abs(tot - float(ref.mean())) < 1e-4 * float(ref.mean())
    per_ba, _ = _distance(dev, ba, lw, n)
    assert torch.equal(per, per_ba)
    per_aa, tot_aa = _distance(dev, aa, lw, n)
    assert bool((per_aa == 0).all()) and tot_aa == 0.0


def _ref_per_image(mod_net, mod_lin, a, b, normalize):
    return lpips_ref.lpips_per_image(a, b, mod_net, mod_lin, normalize)


@pytest.mark.parametrize("seed", [0, 1])
def test_end_to_end_vs_float64(dev, seed):
    """Whole metric vs the float64 restatement, stand-in weights (a second weight seed for seed 1), close pairs (noise-perturbed
    copies) and unrelated pairs.  Bar: 3 % relative per image.  Measured on the MI355X: at most 0.015 % (close pairs) and
    0.003 % (unrelated pairs)."""
    m = P("lpips")
    net = m._standin_alex_state(4321 + 17 * seed)
    lin_sd = m._standin_lin_state(4322 + 17 * seed)
    lins = m.load_lin_state(lin_sd)
    g = torch.Generator().manual_seed(100 + seed)
    worst = {}
    for normalize in (False, True):
        mods = {r: m.LPIPS(reduction=r, normalize=normalize, net_weights=net, lin_weights=lin_sd) for r in ("mean", "sum")}
        for shape in [(2, 3, 64, 64), (1, 3, 97, 131), (3, 3, 256, 256), (1, 3, 512, 512)]:
            lo = 0.0 if normalize else -1.0
            a = torch.rand(shape, generator=g) * (1 - lo) + lo
            close = (a + 0.05 * (1 - lo) * torch.randn(shape, generator=g)).clamp(lo, 1.0)
            far = torch.rand(shape, generator=g) * (1 - lo) + lo
            for kind, b in (("close", close), ("far", far)):
                ref = _ref_per_image(net, lins, a, b, normalize)
                ad, bd = a.to(dev), b.to(dev)
                per = mods["mean"].per_image(ad, bd).cpu().double()
                rel = float(((per - ref).abs() / ref).max())
                worst[kind] = max(worst.get(kind, 0.0), rel)
                assert rel <= 0.03, (normalize, shape, kind, rel)
                assert abs(float(mods["mean"](ad, bd)) - float(ref.mean())) <= 0.03 * float(ref.mean())
                assert abs(float(mods["sum"](ad, bd)) - float(ref.sum())) <= 0.03 * float(ref.sum())
    print("worst relative error per image:", worst)


def test_chunked_matches_unchunked_and_running_state(dev):
    m = P("lpips")
    g = torch.Generator().manual_seed(5)
    a = (torch.rand(5, 3, 96, 80, generator=g) * 2 - 1).to(dev)
    b = (torch.rand(5, 3, 96, 80, generator=g) * 2 - 1).to(dev)
    mod = m.LPIPS()
    whole, tot = mod.per_image(a, b), float(mod(a, b))
    mod.max_pairs_per_launch = 2                      # three trunk passes: 2 + 2 + 1 pairs
    chunked, tot_c = mod.per_image(a, b), float(mod(a, b))
    assert torch.allclose(chunked, whole, rtol=1e-5, atol=0), (chunked, whole)
    assert abs(tot_c - tot) <= 1e-5 * tot
    assert abs(tot - float(whole.double().mean())) <= 1e-6 * tot
    mod.max_pairs_per_launch = None
    mod.reset()
    mod.update(a[:2], b[:2])
    mod.update(a[2:], b[2:])
    assert abs(float(mod.compute()) - tot) <= 1e-5 * tot
    assert float(mod.total) == 5.0
    s = m.LPIPS(reduction="sum")
    s.update(a, b)
    assert abs(float(s.compute()) - float(whole.double().sum())) <= 1e-5 * float(whole.sum())


def test_identical_inputs_give_zero_and_swap_is_symmetric(dev):
    m = P("lpips")
    g = torch.Generator().manual_seed(6)
    a = (torch.rand(2, 3, 64, 72, generator=g) * 2 - 1).to(dev)
    b = (torch.rand(2, 3, 64, 72, generator=g) * 2 - 1).to(dev)
    mod = m.LPIPS()
    assert float(mod(a, a)) == 0.0
    assert torch.equal(mod.per_image(a, b), mod.per_image(b, a))


def test_launch_log_of_one_call(dev):
    L, m = P("_lib"), P("lpips")
    mod = m.LPIPS()
    a = (torch.rand(1, 3, 64, 64) * 2 - 1).to(dev)
    mod(a, a)                                          # packs the weights outside the log
    L.LAUNCH_LOG = []
    try:
        mod(a, a * 0.5)
        torch.cuda.synchronize()
        names = [e[0] for e in L.LAUNCH_LOG]
    finally:
        L.LAUNCH_LOG = None
    assert names.count("dsr_lpips_stem_prep") == 1
    assert names.count("dsr_maxpool3s2_fwd") == 2
    assert names.count("dsr_conv_fwd") == 5
    assert names.count("dsr_lpips_distance") == 1 and names.count("dsr_lpips_finalize") == 1


def test_evaluate_generator_with_lpips(dev):
    from oracle import filler, gan
    ev, Gm, m = P("evaluate"), P("models.GAN.generator"), P("lpips")
    sd = filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2)))
    g = Gm.Generator(4, 2)
    g.load_state_dict(sd)
    g.to(dev)
    pairs = []
    for i, (h, w) in enumerate([(12, 16), (10, 12), (8, 8)]):
        lr = filler.tensor(f"evl:lr{i}", (1, 3, h, w), 0.5, 0.5)
        hr = filler.tensor(f"evl:hr{i}", (1, 3, 4 * h, 4 * w), 0.5, 0.5).clamp(-1, 1)
        pairs.append((lr.to(dev), hr.to(dev), [f"img{i}"]))
    base = ev.evaluate_generator(g, pairs)
    lp = m.LPIPS()
    res = ev.evaluate_generator(g, pairs, lpips_model=lp)
    for k, v in base.items():
        assert res[k] == v, k
    assert list(res["lpips"]) == ["img0", "img1", "img2"]
    assert res["avg_lpips"] == sum(res["lpips"].values()) / 3
    assert all(v > 0 for v in res["lpips"].values())
    assert ev.lpips(pairs[0][1], pairs[0][1], lp) == 0.0


def test_error_paths(dev):
    m = P("lpips")
    mod = m.LPIPS()
    a = torch.rand(1, 3, 64, 64, device=dev)
    with pytest.raises(ValueError, match="got values in"):
        mod(a * 3 - 1, a)                              # outside [-1, 1]
    with pytest.raises(ValueError):
        m.LPIPS(normalize=True)(a * 2 - 1, a)          # outside [0, 1]
    bad = a.clone()
    bad[0, 1, 5, 7] = float("nan")
    with pytest.raises(ValueError):
        mod(bad, a)
    with pytest.raises(ValueError):
        mod(a, a[:, :, :, :63])
    with pytest.raises(ValueError):
        mod(a[:, :1], a[:, :1])
    with pytest.raises(RuntimeError, match="30x64"):
        mod(a[:, :, :30], a[:, :, :30])
    mod.reset()
    with pytest.raises(ValueError):
        mod.update(a * 3 - 1, a)
    assert mod._count == 0                             # a rejected batch leaves the running state alone
    assert float(m.LPIPS(normalize=True)(a, a)) == 0.0
