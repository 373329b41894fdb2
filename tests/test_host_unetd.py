"""CPU: the yardsticks of the Real-ESRGAN discriminator path against torch itself, the module's state-dict surface, and the
argument checks of the new entry points.

1. tests/spectral_ref.py equals torch.nn.utils.spectral_norm in float64 (weight, u, v after one and three train-mode forwards,
   eval mode, the weight_orig gradient);
2. UNetDiscriminatorSN's state dict is that of a copy built from nn.Conv2d + spectral_norm, and loads it strictly;
3. tests/unetd_ref.network in float64 equals that copy's forward (train mode with the updated vectors, and eval mode);
4. ValueError for a 12 x 12 input, a loud failure without a GPU, DSR_E_ARG from the new entry points on bad arguments."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF
from torch.nn.utils import spectral_norm

import spectral_ref as SR
import unetd_ref as U

PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


class TorchUNetD(nn.Module):
    """The published definition with torch's own layers (the reference copy of items 2 and 3)."""

    def __init__(self, num_in_ch=3, num_feat=64, skip_connection=True):
        super().__init__()
        nf, norm = num_feat, spectral_norm
        self.skip_connection = skip_connection
        self.conv0 = nn.Conv2d(num_in_ch, nf, 3, 1, 1)
        self.conv1 = norm(nn.Conv2d(nf, nf * 2, 4, 2, 1, bias=False))
        self.conv2 = norm(nn.Conv2d(nf * 2, nf * 4, 4, 2, 1, bias=False))
        self.conv3 = norm(nn.Conv2d(nf * 4, nf * 8, 4, 2, 1, bias=False))
        self.conv4 = norm(nn.Conv2d(nf * 8, nf * 4, 3, 1, 1, bias=False))
        self.conv5 = norm(nn.Conv2d(nf * 4, nf * 2, 3, 1, 1, bias=False))
        self.conv6 = norm(nn.Conv2d(nf * 2, nf, 3, 1, 1, bias=False))
        self.conv7 = norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv8 = norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(nf, 1, 3, 1, 1)

    def forward(self, x):
        act = lambda v: TF.leaky_relu(v, negative_slope=0.2)
        up = lambda v: TF.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)
        x0 = act(self.conv0(x))
        x1 = act(self.conv1(x0))
        x2 = act(self.conv2(x1))
        x3 = act(self.conv3(x2))
        x4 = act(self.conv4(up(x3)))
        if self.skip_connection:
            x4 = x4 + x2
        x5 = act(self.conv5(up(x4)))
        if self.skip_connection:
            x5 = x5 + x1
        x6 = act(self.conv6(up(x5)))
        if self.skip_connection:
            x6 = x6 + x0
        return self.conv9(act(self.conv8(act(self.conv7(x6)))))


# ----------------------------------------------------------------------------- 1. the spectral-norm formulas
@pytest.mark.parametrize("k,stride", [(4, 2), (3, 1)])
def test_spectral_ref_equals_torch(k, stride):
    torch.manual_seed(k)
    conv = spectral_norm(nn.Conv2d(8, 16, k, stride, 1, bias=False).double())
    w = conv.weight_orig.detach().clone()
    u, v = conv.weight_u.detach().clone(), conv.weight_v.detach().clone()
    x = torch.randn(2, 8, 8, 8, dtype=torch.float64)
    conv.train()
    for step in range(3):
        y = conv(x)
        u, v, sigma, w_sn = SR.iterate(w, u, v)
        if step in (0, 2):
            assert float((conv.weight.detach() - w_sn).abs().max()) <= 1e-12
            assert float((conv.weight_u - u).abs().max()) <= 1e-12 and float((conv.weight_v - v).abs().max()) <= 1e-12
    # the gradient of weight_orig through that last forward
    probe = torch.randn_like(y)
    conv.weight_orig.grad = None
    (y * probe).sum().backward()
    g = torch.autograd.grad((TF.conv2d(x, w_sn.requires_grad_(True), None, stride, 1) * probe).sum(), w_sn)[0]
    want = SR.backward(g, w_sn.detach(), u, v, sigma)
    got = conv.weight_orig.grad
    assert float((got - want).abs().max()) <= 1e-12 * float(got.abs().max())
    # eval mode: sigma from the stored vectors, which stay
    conv.eval()
    conv(x)
    sig_e, w_e = SR.evaluate(w, u, v)
    assert float((conv.weight.detach() - w_e).abs().max()) <= 1e-12
    assert torch.equal(conv.weight_u, u) and torch.equal(conv.weight_v, v)


# ----------------------------------------------------------------------------- 2. state dict
def test_state_dict_is_torch_spectral_norm_layout(tmp_path):
    M = P("models.GAN")
    net, ref = M.UNetDiscriminatorSN(), TorchUNetD()
    sd, rsd = net.state_dict(), ref.state_dict()
    assert len(sd) == 28 and list(sd) == list(rsd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == U.key_table()
    assert U.param_count() == 4376897 == sum(p.numel() for p in net.parameters())
    assert {k for k, _ in net.named_parameters()} == {k for k, _ in ref.named_parameters()}
    net.load_state_dict(rsd, strict=True)
    assert all(torch.equal(v, rsd[k]) for k, v in net.state_dict().items())
    # BasicSR's wrapping, through evaluate.load_model
    path = tmp_path / "netD.pth"
    torch.save({"params": rsd}, path)
    net2 = P("evaluate").load_model(M.UNetDiscriminatorSN(), str(path))
    assert all(torch.equal(v, rsd[k]) for k, v in net2.state_dict().items())
    # u and v start normalised
    fresh = M.UNetDiscriminatorSN(num_feat=8)
    for name in U.SN:
        m = getattr(fresh, name)
        assert abs(float(m.weight_u.norm()) - 1) < 1e-5 and abs(float(m.weight_v.norm()) - 1) < 1e-5
    assert [(k, tuple(v.shape)) for k, v in fresh.state_dict().items()] == U.key_table(num_feat=8)


# ----------------------------------------------------------------------------- 3. the float64 network
@pytest.mark.parametrize("skip", [True, False])
def test_unetd_ref_equals_torch_copy(skip):
    torch.manual_seed(3)
    ref = TorchUNetD(num_feat=8, skip_connection=skip).double()
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    x = torch.randn(2, 3, 16, 24, dtype=torch.float64)
    ref.train()
    with torch.no_grad():
        want = ref(x)
    got, vec = U.network(sd, x, training=True, skip=skip)
    assert float((got - want).abs().max()) <= 1e-10
    after = ref.state_dict()
    for name in U.SN:
        assert float((vec[name][0] - after[name + ".weight_u"]).abs().max()) <= 1e-10
        assert float((vec[name][1] - after[name + ".weight_v"]).abs().max()) <= 1e-10
    ref.eval()
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    with torch.no_grad():
        want = ref(x)
    got, vec = U.network(sd, x, training=False, skip=skip)
    assert float((got - want).abs().max()) <= 1e-10
    assert all(torch.equal(vec[name][0], sd[name + ".weight_u"]) for name in U.SN)


def test_gan_loss_ref_equals_torch():
    x = torch.randn(3, 1, 8, 8, dtype=torch.float64) * 3
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    assert abs(float(U.gan_loss(x, True) - TF.binary_cross_entropy_with_logits(x, one))) < 1e-12
    assert abs(float(U.gan_loss(x, False) - TF.binary_cross_entropy_with_logits(x, zero))) < 1e-12
    assert abs(float(U.gan_loss(x, True, "lsgan") - TF.mse_loss(x, one))) < 1e-12
    assert abs(float(U.gan_loss(x, False, "hinge", True) - torch.relu(1 + x).mean())) < 1e-12
    assert abs(float(U.gan_loss(x, True, "hinge", True) - torch.relu(1 - x).mean())) < 1e-12
    assert abs(float(U.gan_loss(x, True, "hinge", False) + x.mean())) < 1e-12


# ----------------------------------------------------------------------------- 4. errors and the ABI
def test_input_size_must_be_a_multiple_of_8():
    net = P("models.GAN").UNetDiscriminatorSN(num_feat=8)
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 12, 12))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 16, 20))
    with pytest.raises(RuntimeError):          # torch's own verdict on such an input
        TorchUNetD(num_feat=8)(torch.zeros(1, 3, 12, 12))


def test_new_ops_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    F = P("functional")
    net = P("models.GAN").UNetDiscriminatorSN(num_feat=8)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError):
        F.gan_loss(torch.zeros(4), True)
    m = net.conv1
    with pytest.raises(RuntimeError):
        F.SpectralNormWeight.apply(m.weight_orig, m.weight_u, m.weight_v, True)
    with pytest.raises(ValueError):
        F.gan_loss(torch.zeros(4), True, kind="wgan")


def test_bad_arguments_return_codes():
    L = P("_lib")
    lib = L.lib()
    E_ARG = -1
    ints = lambda *v: (C.c_int * len(v))(*v)
    buf = (C.c_float * 128)()                      # host memory stands in for device pointers: nothing may be launched
    p = (C.cast(buf, C.c_void_p).value + 63) & ~63
    tab = lambda *v: (C.c_void_p * len(v))(*v)
    ok = dict(count=1, w=tab(p), u=tab(p + 16), v=tab(p + 32), cout=ints(2), k=ints(2), sigma=p + 48, out=tab(p + 64), ws=p + 128)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.dsr_spectral_norm_fwd(a["count"], a["w"], a["u"], a["v"], a["cout"], a["k"], 1, 1e-12, a["sigma"], a["out"],
                                         a["ws"], 1 << 20, None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.dsr_spectral_norm_bwd(a["count"], a["w"], a["out"], a["u"], a["v"], a["cout"], a["k"], a["sigma"], a["out"],
                                         a["ws"], 1 << 20, None)

    for call in (fwd, bwd):
        assert call(count=0) == E_ARG and b"count" in lib.dsr_last_error()
        assert call(count=65) == E_ARG
        assert call(count=-1) == E_ARG
        assert call(w=None) == E_ARG
        assert call(u=None) == E_ARG
        assert call(v=None) == E_ARG
        assert call(out=None) == E_ARG
        assert call(cout=None) == E_ARG and call(k=None) == E_ARG
        assert call(sigma=None) == E_ARG and call(ws=None) == E_ARG
        assert call(w=tab(None)) == E_ARG and call(u=tab(None)) == E_ARG and call(v=tab(None)) == E_ARG
        assert call(out=tab(None)) == E_ARG
        assert call(cout=ints(0)) == E_ARG and call(k=ints(0)) == E_ARG and call(cout=ints(-3)) == E_ARG
        assert call(w=tab(p + 2)) == E_ARG                       # off its 4-byte alignment
    assert lib.dsr_spectral_norm_fwd(1, ok["w"], ok["u"], ok["v"], ok["cout"], ok["k"], 1, 1e-12, ok["sigma"], ok["out"], ok["ws"],
                                     8, None) == E_ARG           # workspace too small
    assert lib.dsr_spectral_norm_workspace(0, ok["cout"], ok["k"]) == 0
    assert lib.dsr_spectral_norm_workspace(1, ints(0), ints(4)) == 0
    assert lib.dsr_spectral_norm_bwd_workspace(65, ok["cout"], ok["k"]) == 0
    # [512, 4096]: s, then 16 partial rows of 4096; the backward: one partial per 4096 elements
    assert lib.dsr_spectral_norm_workspace(1, ints(512), ints(4096)) == 4 * (512 + 16 * 4096)
    assert lib.dsr_spectral_norm_bwd_workspace(1, ints(512), ints(4096)) == 4 * 512
    assert lib.dsr_gan_loss_blocks(0) == 0 and lib.dsr_gan_loss_blocks(1) == 1 and lib.dsr_gan_loss_blocks(1 << 30) == 1024
    assert lib.dsr_gan_loss(None, 4, 0, 1, 0, p, p + 64, p + 128, None) == E_ARG
    assert lib.dsr_gan_loss(p, 0, 0, 1, 0, p, p + 64, p + 128, None) == E_ARG
    assert lib.dsr_gan_loss(p, 4, 3, 1, 0, p, p + 64, p + 128, None) == E_ARG and b"kind" in lib.dsr_last_error()
    assert lib.dsr_gan_loss(p, 4, 0, 1, 0, None, p + 64, p + 128, None) == E_ARG
    assert lib.dsr_gan_loss(p, 4, 0, 1, 0, p, None, p + 128, None) == E_ARG
    assert lib.dsr_gan_loss(p, 4, 0, 1, 0, p, p + 64, None, None) == E_ARG
    assert lib.dsr_abi_version() == L.ABI_VERSION == 9


def test_spectral_norm_wide_and_full_table_cases():
    """The cases of tests/test_gpu_spectral_norm.py past one turn of sn_v_kernel's column loops and at the table's limit:
    the regime each is meant to reach (SR.v_turns, restated from csrc/spectral_norm.hip), the workspace formulas of
    tests/spectral_ref.py against the library's, and the refusal of a 65th layer by all four entry points."""
    L = P("_lib")
    lib = L.lib()
    ints = lambda v: (C.c_int * len(v))(*v)
    cout, k = SR.WIDE_VECTOR
    print(f"vector path {SR.WIDE_VECTOR}: {SR.v_turns(k, True)} turns; scalar path {SR.WIDE_SCALAR}: {SR.v_turns(SR.WIDE_SCALAR[1], False)}")
    assert k > 4096 and k % 4 == 0 and SR.v_turns(k, True) == 2 and SR.v_turns(4096, True) == 1
    assert SR.WIDE_SCALAR[1] > 1024 and SR.v_turns(SR.WIDE_SCALAR[1], False) == 2 and SR.v_turns(576, False) == 1
    conv4 = {name: (co, ci * kk * kk) for name, co, ci, kk, _, _ in U.layer_table(num_feat=64)}["conv4"]
    assert conv4 == SR.WIDE_VECTOR                                 # the widest normalised layer of the default discriminator
    for shapes in ([SR.WIDE_VECTOR], [SR.WIDE_SCALAR], SR.FULL_TABLE, [(512, 4096)], [(8, 27), (130, 52)]):
        c, kk = ints([s[0] for s in shapes]), ints([s[1] for s in shapes])
        assert lib.dsr_spectral_norm_workspace(len(shapes), c, kk) == SR.fwd_workspace_bytes(shapes), shapes
        assert lib.dsr_spectral_norm_bwd_workspace(len(shapes), c, kk) == SR.bwd_workspace_bytes(shapes), shapes
    assert len(SR.FULL_TABLE) == SR.MAX_LAYERS == 64
    assert any(kk % 4 for _, kk in SR.FULL_TABLE) and any(c % 32 for c, _ in SR.FULL_TABLE)
    # 65 layers: refused by the size queries (0 bytes) and, before any pointer is looked at, by the forward and the backward
    shapes = SR.FULL_TABLE + [(8, 27)]
    c, kk = ints([s[0] for s in shapes]), ints([s[1] for s in shapes])
    assert lib.dsr_spectral_norm_workspace(65, c, kk) == 0 and lib.dsr_spectral_norm_bwd_workspace(65, c, kk) == 0
    buf = (C.c_float * 64)()
    p = (C.cast(buf, C.c_void_p).value + 63) & ~63
    tab = (C.c_void_p * 65)(*([p] * 65))
    assert lib.dsr_spectral_norm_fwd(65, tab, tab, tab, c, kk, 1, 1e-12, p, tab, p, 1 << 30, None) == -1
    assert b"count 65" in lib.dsr_last_error()
    assert lib.dsr_spectral_norm_bwd(65, tab, tab, tab, tab, c, kk, p, tab, p, 1 << 30, None) == -1
    assert b"count 65" in lib.dsr_last_error()
    assert all(v == 0.0 for v in buf)
