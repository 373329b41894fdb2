"""GPU: UNetDiscriminatorSN (models/GAN/unet_discriminator.py) and steps.realesrgan_step against tests/unetd_ref.py.

1. the 4x4 stride-2 pad-1 convolution (a shape nothing else here runs) on exact-integer operands through F.ConvAct: forward,
   input gradient and weight gradient bit for bit against float64 F.conv2d, bf16 and fp16;
2. the whole network against the float64 network with the storage-model network as the floor; u and v after the forward;
3. every parameter gradient and the image gradient (parity_util.compare_grads), plain and inside F.batched_wgrad(): same bits;
4. a frozen discriminator: the image gradient still arrives, no weight-gradient launch, no .grad;
5. the pack cache does not grow with the per-forward W_sn tensors;
6. steps.realesrgan_step against the float64 restatement of the step, and eager = HIP-graph replay bit for bit."""
import contextlib
import importlib

import pytest
import torch
import torch.nn.functional as TF

import parity_util
import rrdb_ref as R
import spectral_ref as SR
import unetd_ref as U
import vggfeat_ref
from oracle import filler, lowp
from test_gpu_spectral_norm import EPS32, forward_bound

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


DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]


# ----------------------------------------------------------------------------- 1. the 4x4 stride-2 convolution, exactly
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 8, 16, 8, 8), (1, 64, 128, 16, 16), (2, 8, 16, 6, 10)],
                         ids=["8to16-8x8", "64to128-16x16", "8to16-6x10"])
def test_conv4x4_stride2_exact(dev, dtype, n, cin, cout, h, w):
    """Ternary x, w and dy (density 0.3), LeakyReLU 0.25: every product, partial sum and stored value is a quarter-integer far
    below 2^8, so nothing rounds and the summation order cannot show -- torch.equal against float64 F.conv2d and its autograd
    (activation gradient read off the output, o >= 0 -> 1, as the kernels document)."""
    F = P("functional")
    g = torch.Generator().manual_seed(n * 1000 + cin + h)
    x = R.ternary(g, (n, cin, h, w), 0.3)
    wt = R.ternary(g, (cout, cin, 4, 4), 0.3)
    x64, w64 = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    z = TF.conv2d(x64, w64, None, 2, 1)
    assert z.shape[-2:] == (h // 2, w // 2)
    y = torch.where(z >= 0, z, z * 0.25).detach()
    dy = R.ternary(g, tuple(y.shape), 0.3)
    gz = dy * torch.where(y >= 0, 1.0, 0.25)
    dx, dw = torch.autograd.grad(z, (x64, w64), gz)
    assert R.representable(y, dtype) and R.representable(gz, dtype) and R.representable(dx, dtype)
    assert float(y.abs().max()) > 4 and float(dx.abs().max()) > 2                         # (not a degenerate case)
    t16 = R.DTYPES[dtype]
    xd = x.permute(0, 2, 3, 1).contiguous().to(t16).to(dev).requires_grad_(True)
    wd = wt.float().to(dev).requires_grad_(True)
    yd = F.ConvAct.apply(xd, wd, None, None, dict(stride=2, pad=1, act=F.ACT_LEAKY, slope=0.25))
    yd.backward(dy.permute(0, 2, 3, 1).contiguous().to(t16).to(dev))
    nchw = lambda t: t.double().permute(0, 3, 1, 2).cpu()
    assert tuple(yd.shape) == (n, h // 2, w // 2, cout)
    assert torch.equal(nchw(yd.detach()), y)
    assert torch.equal(nchw(xd.grad), dx)
    assert torch.equal(wd.grad.double().cpu(), dw)


# ----------------------------------------------------------------------------- the network
def _state(num_feat, salt=0):
    """A closed-form state dict: unit-gain uniform weights, small biases, normalised u and v."""
    sd = {}
    for k, shape in U.key_table(num_feat=num_feat):
        if k.endswith(("weight_u", "weight_v")):
            t = filler.tensor(k, shape, salt=salt)
            sd[k] = (t.double() / t.double().norm()).float()
        elif k.endswith("bias"):
            sd[k] = filler.tensor(k, shape, 0.1, 0.0, salt)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            sd[k] = filler.tensor(k, shape, (3.0 / fan_in) ** 0.5, 0.0, salt)
    return sd


def _net(dev, sd, num_feat, dtype=torch.bfloat16, skip=True, training=True):
    net = P("models.GAN").UNetDiscriminatorSN(num_feat=num_feat, skip_connection=skip)
    net.load_state_dict(sd, strict=True)
    net.to(dev).train(training)
    net.compute_dtype = dtype
    return net


def _vector_check(tag, net, sd, vec, training):
    """u and v as the forward left them: the bound of test_gpu_spectral_norm.test_float_data (train), untouched (eval)."""
    for name in U.SN:
        m = getattr(net, name)
        if not training:
            assert torch.equal(m.weight_u.cpu(), sd[name + ".weight_u"]) and torch.equal(m.weight_v.cpu(), sd[name + ".weight_v"])
            continue
        du, dv, _, _ = forward_bound(sd[name + ".weight_orig"], sd[name + ".weight_u"])
        for got, ref, b in ((m.weight_u, vec[name][0], du), (m.weight_v, vec[name][1], dv)):
            err = float((got.double().cpu() - ref).abs().max())
            bound = float(b.max()) + EPS32 * float(ref.abs().max())
            assert err <= bound, (tag, name, err, bound)


NETS = [pytest.param(8, (2, 3, 16, 24), id="nf8-2x3x16x24"), pytest.param(64, (1, 3, 16, 16), id="nf64-1x3x16x16")]


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("nf,shape", NETS)
def test_network_forward(dev, nf, shape, dtype, training, skip):
    """The acceptance rule of tests/test_gpu_rrdb.py's whole-network test: max|y_hip - y_f64| <= 2 E_floor + 1e-3 max|y_f64|,
    E_floor = max|y_sim - y_f64| with y_sim the storage-model network of the same 16-bit type.

    Measured on the MI355X, E_floor / bound / error, max|y_f64| (train, skip; the other variants are printed):
        num_feat=8,  2x3x16x24  bf16 3.68e-3 / 7.90e-3 / 3.68e-3   fp16 3.92e-4 / 1.33e-3 / 4.33e-4,  0.547
        num_feat=64, 1x3x16x16  bf16 3.67e-3 / 7.75e-3 / 4.02e-3   fp16 3.71e-4 / 1.14e-3 / 4.89e-4,  0.401
    over all sixteen variants the error is between 0.8 and 1.35 of E_floor."""
    sd = _state(nf)
    if not training:
        # eval mode reads the stored vectors: as in a trained checkpoint they are iterated ones (sigma from the random initial
        # pair is a random projection, orders of magnitude below the spectral norm: logits of 1e9 and fp16 overflow)
        for name in U.SN:
            u, v = sd[name + ".weight_u"], sd[name + ".weight_v"]
            for _ in range(3):
                u, v, _, _ = SR.iterate(sd[name + ".weight_orig"], u, v)
            sd[name + ".weight_u"], sd[name + ".weight_v"] = u.float(), v.float()
    x = filler.tensor("in:unetd" + str(shape), shape, 0.5, 0.5)
    y64, vec = U.network(sd, x, None, training, skip)
    ysim, _ = U.network(sd, x, dtype, training, skip)
    floor = float((ysim - y64).abs().max())
    bound = 2.0 * floor + 1e-3 * float(y64.abs().max())
    net = _net(dev, sd, nf, R.DTYPES[dtype], skip, training)
    with torch.no_grad():
        y = net(x.to(dev))
    assert tuple(y.shape) == (shape[0], 1, shape[2], shape[3]) and y.dtype == torch.float32
    err = float((y.double().cpu() - y64).abs().max())
    print(f"unetd nf={nf} {shape} dtype={dtype} train={training} skip={skip}: E_floor {floor:.3e} bound {bound:.3e} error {err:.3e} "
          f"max|y| {float(y64.abs().max()):.3e}")
    assert err <= bound, (err, bound)
    _vector_check("forward", net, sd, vec, training)


def _ref_grads(sd, x, dtype, real=True):
    leaves = {k: v.double().clone().requires_grad_(not k.endswith(("weight_u", "weight_v"))) for k, v in sd.items()}
    xi = x.double().clone().requires_grad_(True)
    y, _ = U.network(leaves, xi, dtype, True, True)
    U.gan_loss(y, real).backward()
    out = {k: v.grad for k, v in leaves.items() if v.requires_grad}
    out["input"] = xi.grad
    return out


def _hip_grads(net, xd, batched, frozen=False):
    F = P("functional")
    loss = F.gan_loss(net(xd), True)
    with F.batched_wgrad(batched):
        loss.backward()
    out = {k: p.grad for k, p in net.named_parameters()}
    out["input"] = xd.grad
    return out


def test_gradients_plain_and_batched(dev):
    """Every parameter gradient and the image gradient of gan_loss(D(x), real): parity_util.compare_grads as it stands, float64
    network as the oracle, bf16 storage-model network as the floor.  The backward inside F.batched_wgrad() gives the same bits:
    a derived weight that joined the batch would hand its backward node an unwritten placeholder."""
    shape, nf = (2, 3, 16, 24), 8
    sd = _state(nf)
    x = filler.tensor("in:unetd_grad", shape, 0.5, 0.5)
    ref, sim = _ref_grads(sd, x, None), _ref_grads(sd, x, R.BF16)
    got = []
    for batched in (False, True):
        net = _net(dev, sd, nf)
        xd = x.to(dev).requires_grad_(True)
        got.append(_hip_grads(net, xd, batched))
    plain, batched = got
    assert set(plain) == set(ref) and all(g is not None for g in plain.values())
    for k in plain:
        assert torch.equal(plain[k], batched[k]), k
    bad, table = parity_util.compare_grads(plain, ref, sim)
    worst = sorted(table.items(), key=lambda kv: kv[1][0])[:5]
    print("unetd gradients, lowest cosines (cos_hip, cos_floor, ratio_hip, ratio_floor, numel):", worst)
    assert len(table) == len(ref) - 1 and not bad, bad             # (conv9.bias has one element: not a direction)
    b9 = float(plain["conv9.bias"].cpu())
    assert abs(b9 - float(ref["conv9.bias"])) <= 2 * abs(float(sim["conv9.bias"]) - float(ref["conv9.bias"])) + 1e-3 * abs(float(ref["conv9.bias"]))


def test_frozen_discriminator(dev):
    """The generator half of the step: D's parameters frozen, the image gradient still matches, no weight-gradient launch (and
    so no spectral-norm backward: nothing could feed it), every .grad stays None."""
    F, L = P("functional"), P("_lib")
    shape, nf = (2, 3, 16, 24), 8
    sd = _state(nf)
    x = filler.tensor("in:unetd_grad", shape, 0.5, 0.5)
    ref, sim = _ref_grads(sd, x, None), _ref_grads(sd, x, R.BF16)
    net = _net(dev, sd, nf)
    for p in net.parameters():
        p.requires_grad_(False)
    xd = x.to(dev).requires_grad_(True)
    F.KERNEL_LOG, L.LAUNCH_LOG = klog, llog = [], []
    try:
        with F.batched_wgrad():
            F.gan_loss(net(xd), True).backward()
        torch.cuda.synchronize()
    finally:
        F.KERNEL_LOG = L.LAUNCH_LOG = None
    kinds = [e[0] for e in klog]
    names = [e[0] for e in llog]
    assert "fwd" in kinds and "dgrad" in kinds and not [k for k in kinds if k.startswith("wgrad")], kinds
    assert names.count("dsr_spectral_norm_fwd") == 1 and "dsr_spectral_norm_bwd" not in names
    assert not [nm for nm in names if "wgrad" in nm or "first_bwd" in nm], names
    assert all(p.grad is None for p in net.parameters())
    bad, table = parity_util.compare_grads({"input": xd.grad}, ref, sim)
    print("frozen D, image gradient (cos_hip, cos_floor, ratio_hip, ratio_floor, numel):", table)
    assert len(table) == 1 and not bad, bad


def test_pack_cache_does_not_grow(dev):
    """50 train-mode forwards: only conv0 / conv9 (the two plain weights) may enter the pack cache; W_sn's images die with it."""
    F = P("functional")
    net = _net(dev, _state(8), 8)
    x = filler.tensor("in:unetd_cache", (1, 3, 16, 16), 0.5, 0.5).to(dev)
    before = len(F._pack_cache)
    with torch.no_grad():
        for _ in range(50):
            net(x)
    torch.cuda.synchronize()
    assert len(F._pack_cache) - before <= 2, (before, len(F._pack_cache))


# ----------------------------------------------------------------------------- 6. the step
LW = {"conv1_2": 0.5, "relu2_2": 1.0}
STEP_NF = 8


def _step_inputs():
    lq = filler.tensor("in:resr_lq", (2, 3, 8, 8), 0.5, 0.5)
    gt = filler.tensor("in:resr_gt", (2, 3, 32, 32), 0.5, 0.5)
    return lq, gt


def _gen_state():
    M = P("models.GAN.rrdbnet")
    return filler.fill_state_dict(M.RRDBNet(num_block=1).state_dict())


def _step_reference(gsd, dsd, vsd, lq, gt, dtype, gan_weight):
    """The step in float64 (dtype=None) or under the storage model: the five losses, the generator's gradients, D's vectors."""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in gsd.items()}
    gt64 = gt.double()
    fake = R.network(leaves, lq, 4, dtype=dtype, fused=False)
    l_pix = (fake - gt64).abs().mean()
    ctx = lowp.storage(torch.bfloat16) if dtype is not None else contextlib.nullcontext()
    with ctx:
        l_percep = vggfeat_ref.ref_loss({k: v.double() for k, v in vsd.items()}, fake, gt64, LW, "l1", True, False)
    d = {k: v.double().clone() for k, v in dsd.items()}

    def disc(img):
        y, vec = U.network(d, img, dtype, True, True)
        for name, (u, v) in vec.items():
            d[name + ".weight_u"], d[name + ".weight_v"] = u, v
        return y

    l_g_gan = U.gan_loss(disc(fake), True)
    (1.0 * l_pix + l_percep + gan_weight * l_g_gan).backward()
    grads = {k: v.grad for k, v in leaves.items()}
    with torch.no_grad():
        l_d_real = U.gan_loss(disc(gt64), True, "vanilla", True)
        l_d_fake = U.gan_loss(disc(fake.detach()), False, "vanilla", True)
    losses = [float(v.detach()) for v in (l_pix, l_percep, l_g_gan, l_d_real, l_d_fake)]
    return losses, grads, d


def _step_parts(dev, gsd, dsd, lr=1e-3):
    M, O, pc = P("models.GAN.rrdbnet"), P("optim"), P("perceptual")
    gen = M.RRDBNet(num_block=1)
    gen.load_state_dict(gsd)
    gen.to(dev).train()
    disc = _net(dev, dsd, STEP_NF)
    feat = pc.VggFeatureLoss(LW, "l1").to(dev)
    opt_g = O.FusedAdam(gen.parameters(), lr=torch.tensor(lr))
    opt_d = O.FusedAdam(disc.parameters(), lr=torch.tensor(lr))
    return gen, disc, feat, opt_g, opt_d


def test_realesrgan_step_against_the_restatement(dev):
    """One step.  Losses: |hip - f64| <= 2 |sim - f64| + 1e-3 |f64| (sim: the storage-model restatement).  The generator's
    gradients: parity_util.compare_grads -- they contain the adversarial gradient that flowed through D, and doubling gan_weight
    changes them (under steps.gan_step's detached form it would not).  D's u after the step = three reference iterations on
    the weights the step started from, within the first-order propagation of test_float_data's per-iteration bound:
    e_i <= a_i e_(i-1) + |du_i|_2, a_i = |W|_2^2 / (|W^T u_(i-1)| |W v_i|), the norm of the normalised iteration's derivative."""
    S, G = P("steps"), P("utils.GAN")
    lq, gt = _step_inputs()
    gsd, dsd, vsd = _gen_state(), _state(STEP_NF, salt=1), G._standin_vgg_state()
    ref_l, ref_g, ref_d = _step_reference(gsd, dsd, vsd, lq, gt, None, 0.1)
    sim_l, sim_g, _ = _step_reference(gsd, dsd, vsd, lq, gt, R.BF16, 0.1)
    gen, disc, feat, opt_g, opt_d = _step_parts(dev, gsd, dsd)
    before_d = {k: v.detach().clone() for k, v in disc.named_parameters()}
    out = S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq.to(dev), gt.to(dev), gan_weight=0.1)
    torch.cuda.synchronize()
    assert len(out) == 6 and all(not t.requires_grad and t.is_cuda for t in out) and tuple(out[5].shape) == (2, 3, 32, 32)
    for name, h, r, s in zip(("l_pix", "l_percep", "l_g_gan", "l_d_real", "l_d_fake"), out, ref_l, sim_l):
        print(f"realesrgan_step {name}: hip {float(h):.6g} f64 {r:.6g} sim {s:.6g}")
        assert abs(float(h) - r) <= 2 * abs(s - r) + 1e-3 * abs(r), (name, float(h), r, s)
    hip_g = {k: p.grad for k, p in gen.named_parameters()}
    assert all(g is not None for g in hip_g.values())
    bad, table = parity_util.compare_grads(hip_g, ref_g, sim_g)
    worst = sorted(table.items(), key=lambda kv: kv[1][0])[:5]
    print("realesrgan_step generator gradients, lowest cosines:", worst)
    assert len(table) == len(ref_g) and not bad, bad
    # D moved, stayed trainable, and its vectors advanced three times
    assert all(p.requires_grad for p in disc.parameters())
    assert all(not torch.equal(p, before_d[k]) for k, p in disc.named_parameters())
    for name in U.SN:
        W, u, v = dsd[name + ".weight_orig"], dsd[name + ".weight_u"].double(), dsd[name + ".weight_v"].double()
        smax = float(torch.linalg.matrix_norm(SR.mat(W), 2))
        e = 0.0
        for _ in range(3):
            du, _, _, _ = forward_bound(W, u)
            t = SR.mat(W).t() @ u
            u, v, _, _ = SR.iterate(W, u, v)
            e = smax ** 2 / (float(t.norm()) * float((SR.mat(W) @ v).norm())) * e + float(du.norm())
        assert float((u - ref_d[name + ".weight_u"]).abs().max()) == 0.0
        got = getattr(disc, name).weight_u.double().cpu()
        err = float((got - u).norm())
        assert err <= e + EPS32, (name, err, e)
    # the adversarial gradient arrives: another gan_weight, other generator gradients
    gen2, disc2, feat2, og2, od2 = _step_parts(dev, gsd, dsd)
    S.realesrgan_step(gen2, disc2, feat2, og2, od2, lq.to(dev), gt.to(dev), gan_weight=0.2)
    changed = [k for k, p in gen2.named_parameters() if not torch.equal(p.grad, hip_g[k])]
    assert len(changed) == len(hip_g), set(hip_g) - set(changed)


def test_realesrgan_step_graphed_equals_eager(dev):
    """One eager step, then two more: eager against two replays of a HIP graph captured after the same first step (GraphedStep's
    warm-up): losses, every parameter of G and D, u and v bit for bit; opt.lr.fill_() between the replays takes effect."""
    S = P("steps")
    lq, gt = _step_inputs()
    lq, gt = lq.to(dev), gt.to(dev)
    gsd, dsd = _gen_state(), _state(STEP_NF, salt=1)

    def make():
        gen, disc, feat, opt_g, opt_d = _step_parts(dev, gsd, dsd)
        return gen, disc, opt_g, opt_d, (lambda: S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt))

    gen_e, disc_e, og_e, od_e, step_e = make()
    gen_g, disc_g, og_g, od_g, step_g = make()
    step_e()
    graphed = S.GraphedStep(step_g, warmup=1)
    for i in range(2):
        if i == 1:
            for o in (og_e, od_e, og_g, od_g):
                o.lr.fill_(5e-3)
        out_e = [t.clone() for t in step_e()]
        out_g = graphed()
        torch.cuda.synchronize()
        for a, b in zip(out_e, out_g):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        for me, mg in ((gen_e, gen_g), (disc_e, disc_g)):
            for (k, a), (_, b) in zip(me.state_dict().items(), mg.state_dict().items()):
                assert torch.equal(a, b), (i, k)
        if i == 0:
            mid = {k: v.clone() for k, v in gen_e.state_dict().items()}
            step_small = {k: (v - gsd[k].to(dev)).abs().max() for k, v in mid.items()}
    # the larger lr of the second replay shows: Adam's first steps move every weight by about lr
    moved = max(float((v - mid[k]).abs().max()) for k, v in gen_g.state_dict().items())
    assert moved > 2.5e-3, moved
    assert max(float(v) for v in step_small.values()) < 2.5e-3
