"""GPU: the multi-layer VGG feature loss on the HIP path (perceptual.VggFeatureLoss, functional.FeatureTap, csrc/featloss.hip).

1. the kernels through the C ABI on small-integer maps, where every fp32 sum and every 16-bit result is exact: equality
2. the module against the fp32 yardstick tests/vggfeat_ref.py by the rule of test_gpu_models.py::test_vgg_loss
3. consistency with utils.GAN.Vgg19Loss on the one configuration both express, and Vgg19Loss's bits unmoved
4. the trunk stops at the deepest tap
5. wiring: precomputed target features, PerceptualLoss(vgg_loss=), gen_perceptual_step under GraphedStep"""
import ctypes as C
import importlib

import pytest
import torch

import vggfeat_ref
from oracle import filler, gan, lowp

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


def cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-30))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ============================================================================= 1. exact kernels
EXACT = [((2, 5, 7, 64), 64, torch.bfloat16),        # a partial last block
         ((1, 3, 3, 8), 3, torch.bfloat16),          # 5 zero pad channels on both sides
         ((3, 37, 41, 128), 128, torch.bfloat16),    # many blocks, more than one row per block
         ((2, 5, 7, 64), 64, torch.float16)]


def _int_maps(shape, c, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randint(-4, 5, shape, generator=g).float()
    t = torch.randint(-4, 5, shape, generator=g).float()
    dn = torch.randint(-3, 4, shape, generator=g).float()
    f[..., c:] = 0
    t[..., c:] = 0
    dn[..., c:] = 0
    return f.to(dtype), t.to(dtype), dn.to(dtype)


@pytest.mark.parametrize("mode", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("shape,c,dtype", EXACT, ids=["2x5x7x64", "1x3x3x8pad", "3x37x41x128", "2x5x7x64f16"])
def test_tap_kernels_are_exact_on_small_integers(dev, shape, c, dtype, mode):
    L = P("_lib")
    lib = L.lib()
    dt = L.BF16 if dtype == torch.bfloat16 else L.F16
    f, t, dn = _int_maps(shape, c, dtype, 7 + mode)
    n, h, w, cp = shape
    p = n * h * w
    d = f.double() - t.double()
    elem = d.abs() if mode == 0 else d * d
    total = float(elem.sum())
    assert total < 2 ** 24 and bool((d == 0).any()) and bool((f <= 0).any())
    fg, tg, dng = f.to(dev), t.to(dev), dn.to(dev)
    rpb = C.c_int()
    blocks = lib.dsr_featloss_blocks(p)
    assert blocks == lib.dsr_pw_reduce_blocks(p, C.byref(rpb)) and blocks == -(-p // rpb.value)
    if shape == (2, 5, 7, 64):
        assert blocks == 2 and p % rpb.value != 0
    if shape == (3, 37, 41, 128):
        assert blocks > 64 and rpb.value > 1

    # ---- forward: per-block partials, the folded mean, relu_out; and the same bits from a second call
    part = torch.full((blocks,), float("nan"), device=dev)
    part2 = torch.full((blocks,), float("nan"), device=dev)
    relu = torch.full(shape, 9.0, dtype=dtype, device=dev)
    plain = torch.full((blocks,), float("nan"), device=dev)
    assert lib.dsr_featloss_tap_fwd(dt, _ptr(fg), _ptr(tg), _ptr(relu), p, cp, mode, _ptr(part), _stream()) == 0
    assert lib.dsr_featloss_tap_fwd(dt, _ptr(fg), _ptr(tg), _ptr(relu), p, cp, mode, _ptr(part2), _stream()) == 0
    assert lib.dsr_featloss_tap_fwd(dt, _ptr(fg), _ptr(tg), None, p, cp, mode, _ptr(plain), _stream()) == 0
    value = torch.full((1,), float("nan"), device=dev)
    assert lib.dsr_featloss_fold(_ptr(part), blocks, float(p * c), _ptr(value), _stream()) == 0
    torch.cuda.synchronize()
    rows = elem.reshape(p, cp).sum(1)
    want_part = torch.stack([rows[b * rpb.value:(b + 1) * rpb.value].sum() for b in range(blocks)])
    assert torch.equal(part.cpu().double(), want_part)
    assert float(part.cpu().double().sum()) == total
    assert torch.equal(part, part2) and torch.equal(part, plain)
    want_value = torch.tensor(total, dtype=torch.float32) / torch.tensor(float(p * c), dtype=torch.float32)
    assert torch.equal(value.cpu(), want_value.reshape(1)), (value.item(), want_value.item())
    assert torch.equal(relu.cpu(), torch.relu(f.float()).to(dtype))

    # ---- backward: g = 1, coef = 2^-4: every df is exactly representable in 16 bits
    coef = 2.0 ** -4
    term = coef * (torch.sign(d) if mode == 0 else 2.0 * d)
    mask = (f.double() > 0).double()
    one = torch.ones(1, device=dev)
    cases = [("masked", dng, 1, dn.double() * mask + term),
             ("post-activation", dng, 0, dn.double() + term),
             ("deepest tap, relu written", None, 1, term),
             ("deepest tap", None, 0, term)]
    for name, dnext, masked, want in cases:
        assert torch.equal(want.to(dtype).double(), want), name              # the expectation is exact in 16 bits
        df = torch.full(shape, 9.0, dtype=dtype, device=dev)
        assert lib.dsr_featloss_tap_bwd(dt, _ptr(fg), _ptr(tg), _ptr(dnext), _ptr(one), coef, mode, masked, _ptr(df), p, cp,
                                        _stream()) == 0, name
        torch.cuda.synchronize()
        assert torch.equal(df.cpu().double(), want), name
    # g scales the tap's own term only
    half = torch.full((1,), 0.5, device=dev)
    df = torch.empty(shape, dtype=dtype, device=dev)
    assert lib.dsr_featloss_tap_bwd(dt, _ptr(fg), _ptr(tg), _ptr(dng), _ptr(half), coef, mode, 1, _ptr(df), p, cp, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(df.cpu().double(), dn.double() * mask + 0.5 * term)


def test_relu_and_weighted_sum_are_exact(dev):
    F = P("functional")
    x, _, _ = _int_maps((2, 5, 7, 64), 64, torch.bfloat16, 3)
    assert torch.equal(F.relu16(x.to(dev)).cpu(), torch.relu(x.float()).bfloat16())
    vals = [torch.tensor([v], device=dev, requires_grad=True) for v in (1.5, -2.0, 0.25)]
    out = F.weighted_sum(vals, [2.0, 0.5, 4.0])
    assert out.shape == () and out.item() == 3.0 - 1.0 + 1.0
    (out * 3.0).backward()
    assert [v.grad.item() for v in vals] == [6.0, 1.5, 12.0]


def test_feature_tap_function_matches_the_formula(dev):
    """functional.FeatureTap end to end on integer maps: value, x_next, and the gradient of sum(x_next * probe) + 8 * value."""
    F = P("functional")
    shape = (2, 5, 7, 64)
    f, t, probe = _int_maps(shape, 64, torch.bfloat16, 11)
    count = f.numel()
    for mode in (F.FEAT_L1, F.FEAT_MSE):
        for want_relu in (True, False):
            fg = f.to(dev).requires_grad_(True)
            x_next, value = F.FeatureTap.apply(fg, t.to(dev), mode, want_relu)
            d = f.double() - t.double()
            total = float((d.abs() if mode == F.FEAT_L1 else d * d).sum())
            assert value.shape == (1,) and value.item() == (torch.tensor(total) / torch.tensor(float(count))).item()
            if want_relu:
                assert torch.equal(x_next.detach().cpu(), torch.relu(f.float()).bfloat16())
            else:
                assert x_next.data_ptr() == fg.data_ptr()                    # f itself, nothing written
            scale = float(count) / 16.0                                      # g * coef = 2^-4
            (x_next.float() * probe.to(dev).float()).sum().backward(retain_graph=True)
            only_next = fg.grad.clone()
            fg.grad = None
            ((x_next.float() * probe.to(dev).float()).sum() + (value * scale).sum()).backward()
            m = (f.double() > 0).double() if want_relu else 1.0
            term = (torch.sign(d) if mode == F.FEAT_L1 else 2.0 * d) / 16.0
            assert torch.equal(only_next.cpu().double(), probe.double() * m)
            assert torch.equal(fg.grad.cpu().double(), probe.double() * m + term)


# ============================================================================= 2. the module against the yardstick
CONFIGS = {
    "a_conv5_4_l1": dict(lw={"conv5_4": 1.0}, crit="l1", range_norm=False),
    "b_five_taps_l1_range_norm": dict(lw={"conv1_2": .1, "conv2_2": .1, "conv3_4": 1.0, "conv4_4": 1.0, "conv5_4": 1.0},
                                      crit="l1", range_norm=True),
    "c_relu2_2_conv4_4_mse": dict(lw={"relu2_2": 1.0, "conv4_4": 0.5}, crit="mse", range_norm=False),
}


@pytest.fixture(scope="module")
def images():
    return filler.tensor("vggfeat:a", (2, 3, 48, 32)), filler.tensor("vggfeat:b", (2, 3, 48, 32))


@pytest.fixture(scope="module")
def standin():
    return P("utils.GAN")._standin_vgg_state()


_REF = {}


def _reference(tag, sd, a, b):
    """fp32 yardstick (loss, per-tap means, image gradient) and the gradient of its bf16-storage restatement, once per config."""
    if tag not in _REF:
        cfg = CONFIGS[tag]
        ar = a.clone().requires_grad_(True)
        terms = vggfeat_ref.ref_terms(sd, ar, b, cfg["lw"], cfg["crit"], True, cfg["range_norm"], None, None)
        loss = sum(float(w) * terms[k] for k, w in cfg["lw"].items())
        loss.backward()
        an = a.clone().requires_grad_(True)
        with lowp.storage(torch.bfloat16):
            vggfeat_ref.ref_loss(sd, an, b, cfg["lw"], cfg["crit"], True, cfg["range_norm"], None, None).backward()
        _REF[tag] = (loss.item(), {k: v.item() for k, v in terms.items()}, ar.grad, an.grad)
    return _REF[tag]


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_module_against_the_yardstick(dev, images, standin, tag):
    """The rule of test_vgg_loss: loss and per-tap means within 3e-2 of the fp32 yardstick, 1 - cos(grad) <= 3 * floor + 0.01 with
    the floor from the yardstick under lowp.storage(bfloat16) (0.050, 0.027, 0.014 for a, b, c on the CPU), gradient norm within
    10 %.  Every figure is printed before it is asserted."""
    pc = P("perceptual")
    cfg = CONFIGS[tag]
    a, b = images
    lref, tref, gref, gfloor = _reference(tag, standin, a, b)
    m = pc.VggFeatureLoss(cfg["lw"], cfg["crit"], range_norm=cfg["range_norm"]).to(dev)
    ag = a.to(dev).requires_grad_(True)
    loss = m(ag, b.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    floor = 1 - cos(gfloor, gref)
    got = 1 - cos(ag.grad.cpu(), gref)
    ratio = float(ag.grad.norm().cpu() / gref.norm())
    print(f"vggfeat {tag}: loss hip={loss.item():.6g} ref={lref:.6g} rel={abs(loss.item() - lref) / abs(lref):.3e}; "
          f"1-cos={got:.3e} floor={floor:.3e}; |g| ratio={ratio:.4f}")
    assert loss.shape == () and abs(loss.item() - lref) < 3e-2 * abs(lref), (loss.item(), lref)
    assert set(m.last_terms) == set(cfg["lw"])
    for k, v in m.last_terms.items():
        assert v.is_cuda and abs(v.item() - tref[k]) < 3e-2 * abs(tref[k]), (k, v.item(), tref[k])
    assert got <= 3.0 * floor + 0.01, f"1 - cos(grad) = {got:.4e}, bf16-storage floor of the yardstick = {floor:.4e}"
    assert abs(ratio - 1) < 0.1, ratio


# ============================================================================= 3. consistency with Vgg19Loss
def test_same_as_vgg19loss_on_its_configuration_and_its_bits_do_not_move(dev):
    G, pc = P("utils.GAN"), P("perceptual")
    a = filler.tensor("vgg:a", (2, 3, 64, 64)).to(dev)
    b = filler.tensor("vgg:b", (2, 3, 64, 64)).to(dev)
    old = G.Vgg19Loss(resize_to=48, crop=40).to(dev)

    def run(mod):
        ag = a.clone().requires_grad_(True)
        loss = mod(ag, b)
        loss.backward()
        return loss.detach().clone(), ag.grad.clone()

    l0, g0 = run(old)
    new = pc.VggFeatureLoss({"relu5_4": 1.0}, "mse", resize_to=48, crop=40).to(dev)
    l1, g1 = run(new)
    assert new.target_features(b)[0].numel() == 4096                      # both reduce the same 4096 bf16 values in fp32
    l2, g2 = run(old)
    torch.cuda.synchronize()
    assert abs(l1.item() - l0.item()) <= 1e-5 * abs(l0.item()), (l1.item(), l0.item())
    assert 1 - cos(g1.cpu(), g0.cpu()) <= 1e-5, 1 - cos(g1.cpu(), g0.cpu())
    assert torch.equal(l0, l2) and torch.equal(g0, g2)                    # Vgg19Loss before and after `perceptual` was used


# ============================================================================= 4. trunk truncation
def test_trunk_stops_at_the_deepest_tap(dev, images):
    pc = P("perceptual")
    m = pc.VggFeatureLoss({"conv2_2": 1.0}).to(dev)
    poisoned = 0
    with torch.no_grad():
        for k, p_ in m.named_parameters():
            if int(k.split(".")[2]) > 7:
                p_.fill_(float("nan"))
                poisoned += 1
    assert poisoned == 24
    a, b = images
    ag = a.to(dev).requires_grad_(True)
    loss = m(ag, b.to(dev))
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(ag.grad).all()) and float(ag.grad.abs().sum()) > 0
    assert m.depth == 4 and m.target_features(b.to(dev))[0].shape == (2, 24, 16, 128)


# ============================================================================= 5. wiring
def test_precomputed_target_features_give_the_same_bits(dev, images):
    pc = P("perceptual")
    cfg = CONFIGS["b_five_taps_l1_range_norm"]
    m = pc.VggFeatureLoss(cfg["lw"], cfg["crit"], range_norm=True).to(dev)
    a, b = images[0].to(dev), images[1].to(dev)
    a1 = a.clone().requires_grad_(True)
    l1 = m(a1, b)
    l1.backward()
    feats = m.target_features(b)
    assert len(feats) == 5 and all(t.dtype == torch.bfloat16 and not t.requires_grad for t in feats)
    assert [tuple(t.shape) for t in feats] == [(2, 48, 32, 64), (2, 24, 16, 128), (2, 12, 8, 256), (2, 6, 4, 512), (2, 3, 2, 512)]
    a2 = a.clone().requires_grad_(True)
    l2 = m(a2, None, feats)
    l2.backward()
    assert torch.equal(l1, l2) and torch.equal(a1.grad, a2.grad)
    with pytest.raises(ValueError, match="image2"):
        m(a1, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="features2"):
        m(a1, None, feats[:2])


def _gan_parts(dev):
    Gm, Dm, optim = P("models.GAN.generator"), P("models.GAN.discriminator"), P("optim")
    gsd = filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2)))
    dsd = filler.fill_state_dict(gan.template(gan.discriminator_shapes((64, 64))))
    g, d = Gm.Generator(4, 2), Dm.Discriminator((64, 64))
    g.load_state_dict(gsd), d.load_state_dict(dsd)
    g.to(dev).train(), d.to(dev).train()
    return g, d, optim.FusedAdam(g.parameters(), lr=1e-3), optim.FusedAdam(d.parameters(), lr=1e-3)


@pytest.mark.parametrize("overlap", [True, False])
def test_gan_step_with_a_supplied_content_loss(dev, overlap):
    """PerceptualLoss(vgg_loss=VggFeatureLoss(...)) through steps.gan_step on the configuration of the existing GAN-step tests
    (stand-in VGG behind resize 32 / crop 28): finite losses, and the generator moves."""
    G, pc, steps = P("utils.GAN"), P("perceptual"), P("steps")
    g, d, og, od = _gan_parts(dev)
    feat = pc.VggFeatureLoss({"conv3_4": 1.0, "relu4_4": 0.5, "conv5_4": 1.0}, "l1", range_norm=True, resize_to=32, crop=28)
    perc = G.PerceptualLoss(vgg_loss=feat).to(dev)
    assert perc.vgg_loss is feat
    lr = filler.tensor("in:gs_lr", (4, 3, 16, 16), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:gs_hr", (4, 3, 64, 64)).to(dev)
    before = {k: v.detach().clone() for k, v in g.named_parameters()}
    ld, lg, fake = steps.gan_step(g, d, perc, og, od, lr, hr, overlap=overlap)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ld)) and bool(torch.isfinite(lg)) and bool(torch.isfinite(fake).all())
    moved = [k for k, v in g.named_parameters() if not torch.equal(v, before[k])]
    assert len(moved) > len(before) // 2, moved
    assert all(bool(torch.isfinite(v).all()) for v in g.parameters())


def test_gen_perceptual_step_graphed_equals_eager(dev):
    """steps.gen_perceptual_step: three replays from a HIP graph leave bit for bit the losses and weights that the same number
    of eager steps from the same start leaves (2 warm-up steps + 3 replays against 5 eager steps)."""
    pc, steps, Gm, optim = P("perceptual"), P("steps"), P("models.GAN.generator"), P("optim")
    sd = filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2)))
    lr = filler.tensor("in:lp_lr", (2, 3, 16, 16), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:lp_hr", (2, 3, 64, 64)).clamp(-1, 1).to(dev)
    cfg = CONFIGS["b_five_taps_l1_range_norm"]

    def make():
        g = Gm.Generator(4, 2)
        g.load_state_dict(sd)
        g.to(dev).train()
        opt = optim.FusedAdam(g.parameters(), lr=1e-3)
        feat = pc.VggFeatureLoss(cfg["lw"], cfg["crit"], range_norm=True).to(dev)
        return g, (lambda: steps.gen_perceptual_step(g, opt, feat, lr, hr, l1_weight=1.0))

    g_e, step_e = make()
    for _ in range(5):
        out_e = step_e()
    g_g, step_g = make()
    graphed = steps.GraphedStep(step_g, warmup=2)         # 2 eager warm-up steps; capture itself executes nothing
    for _ in range(3):
        out_g = graphed()
    torch.cuda.synchronize()
    assert len(out_e) == len(out_g) == 3
    for p, q in zip(out_e, out_g):
        assert bool(torch.isfinite(p).all()) and torch.equal(p, q)
    for (k, p), (_, q) in zip(g_e.state_dict().items(), g_g.state_dict().items()):
        assert torch.equal(p, q), k
    moved = [k for k, v in g_e.state_dict().items() if v.dtype == torch.float32 and not torch.equal(v.cpu(), sd[k])]
    assert len(moved) > len(sd) // 2                      # ... and the steps did move the generator
