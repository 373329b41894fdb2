"""CPU: the float64 yardstick of BasicSR's VGGStyleDiscriminator and of its dense logit head (tests/vggd_ref.py) against torch
itself.  The module and its HIP head are not in the package yet; this file pins the yardstick they will be held to.

1. vggd_ref.key_table / param_count are the state dict of a copy built from torch.nn layers, for input_size 128 and 256;
2. vggd_ref.network in float64 equals that copy's forward to 1e-12, train mode (with the running statistics it leaves) and
   eval mode; the storage model's hand-written BatchNorm equals F.batch_norm;
3. vggd_ref.head (values and gradients) equals torch's autograd, and the NHWC layout helpers invert each other;
4. evaluate.vgg_discriminator_layout is that copy's state dict too, and evaluate.inspect_vgg_discriminator reads the three
   constructor arguments off a checkpoint (plain, wrapped, prefixed) and names the key of every defect."""
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

import vggd_ref as V


class TorchVGGD(nn.Module):
    """The published definition with torch's own layers."""

    def __init__(self, num_in_ch=3, num_feat=64, input_size=128):
        super().__init__()
        nf = num_feat
        self.input_size = input_size
        self.conv0_0 = nn.Conv2d(num_in_ch, nf, 3, 1, 1, bias=True)
        self.conv0_1 = nn.Conv2d(nf, nf, 4, 2, 1, bias=False)
        self.bn0_1 = nn.BatchNorm2d(nf, affine=True)
        self.conv1_0 = nn.Conv2d(nf, nf * 2, 3, 1, 1, bias=False)
        self.bn1_0 = nn.BatchNorm2d(nf * 2, affine=True)
        self.conv1_1 = nn.Conv2d(nf * 2, nf * 2, 4, 2, 1, bias=False)
        self.bn1_1 = nn.BatchNorm2d(nf * 2, affine=True)
        self.conv2_0 = nn.Conv2d(nf * 2, nf * 4, 3, 1, 1, bias=False)
        self.bn2_0 = nn.BatchNorm2d(nf * 4, affine=True)
        self.conv2_1 = nn.Conv2d(nf * 4, nf * 4, 4, 2, 1, bias=False)
        self.bn2_1 = nn.BatchNorm2d(nf * 4, affine=True)
        self.conv3_0 = nn.Conv2d(nf * 4, nf * 8, 3, 1, 1, bias=False)
        self.bn3_0 = nn.BatchNorm2d(nf * 8, affine=True)
        self.conv3_1 = nn.Conv2d(nf * 8, nf * 8, 4, 2, 1, bias=False)
        self.bn3_1 = nn.BatchNorm2d(nf * 8, affine=True)
        self.conv4_0 = nn.Conv2d(nf * 8, nf * 8, 3, 1, 1, bias=False)
        self.bn4_0 = nn.BatchNorm2d(nf * 8, affine=True)
        self.conv4_1 = nn.Conv2d(nf * 8, nf * 8, 4, 2, 1, bias=False)
        self.bn4_1 = nn.BatchNorm2d(nf * 8, affine=True)
        if input_size == 256:
            self.conv5_0 = nn.Conv2d(nf * 8, nf * 8, 3, 1, 1, bias=False)
            self.bn5_0 = nn.BatchNorm2d(nf * 8, affine=True)
            self.conv5_1 = nn.Conv2d(nf * 8, nf * 8, 4, 2, 1, bias=False)
            self.bn5_1 = nn.BatchNorm2d(nf * 8, affine=True)
        self.linear1 = nn.Linear(nf * 8 * 4 * 4, 100)
        self.linear2 = nn.Linear(100, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)

    def forward(self, x):
        assert x.size(2) == self.input_size
        feat = self.lrelu(self.conv0_0(x))
        feat = self.lrelu(self.bn0_1(self.conv0_1(feat)))
        for s in range(1, 6 if self.input_size == 256 else 5):
            feat = self.lrelu(getattr(self, f"bn{s}_0")(getattr(self, f"conv{s}_0")(feat)))
            feat = self.lrelu(getattr(self, f"bn{s}_1")(getattr(self, f"conv{s}_1")(feat)))
        feat = feat.view(feat.size(0), -1)
        return self.linear2(self.lrelu(self.linear1(feat)))


# ----------------------------------------------------------------------------- 1. state dict
@pytest.mark.parametrize("size", [128, 256])
def test_key_table_is_the_torch_copys_state_dict(size):
    ref = TorchVGGD(input_size=size)
    rsd = ref.state_dict()
    print(f"input_size {size}: {len(rsd)} keys, {sum(p.numel() for p in ref.parameters())} parameters")
    assert [(k, tuple(v.shape)) for k, v in rsd.items()] == V.key_table(input_size=size)
    assert sum(p.numel() for p in ref.parameters()) == V.param_count(input_size=size)
    small = TorchVGGD(num_in_ch=1, num_feat=8, input_size=size)
    assert [(k, tuple(v.shape)) for k, v in small.state_dict().items()] == V.key_table(1, 8, size)


# ----------------------------------------------------------------------------- 2. the float64 network and head
@pytest.mark.parametrize("size", [128, 256])
def test_vggd_ref_equals_torch_copy(size):
    torch.manual_seed(size)
    ref = TorchVGGD(num_feat=4, input_size=size).double()
    with torch.no_grad():
        for k, v in ref.named_parameters():
            if k.startswith("bn"):
                v.add_(torch.randn_like(v) * 0.2)
    x = torch.randn(2, 3, size, size, dtype=torch.float64)
    for training in (True, False):
        ref.train(training)
        sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
        with torch.no_grad():
            want = ref(x)
        got, stats = V.network(sd, x, None, training, input_size=size)
        assert tuple(got.shape) == (2, 1)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        after = ref.state_dict()
        assert set(stats) == {k for k in after if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
        for k, v in stats.items():
            assert float((v.double() - after[k].double()).abs().max()) <= 1e-12 * max(1.0, float(after[k].double().abs().max())), k
            assert training or torch.equal(v.double(), sd[k].double())
        assert int(stats["bn0_1.num_batches_tracked"]) == int(sd["bn0_1.num_batches_tracked"]) + int(training)


def test_storage_model_batchnorm_is_batch_norm(monkeypatch):
    """The storage model writes the BatchNorm out by hand (it takes the statistics from the unrounded sums): with the rounding
    switched off it must be F.batch_norm."""
    torch.manual_seed(5)
    ref = TorchVGGD(num_feat=4).double()
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    x = torch.randn(2, 3, 128, 128, dtype=torch.float64)
    monkeypatch.setattr(V, "_store", lambda t, dtype: t)
    for training in (True, False):
        want, wstats = V.network(sd, x, None, training)
        for folded in (False, True):
            got, stats = V.network(sd, x, V.BF16, training, folded)
            assert float((got - want).abs().max()) <= 1e-12
            for k in wstats:
                assert float((stats[k].double() - wstats[k].double()).abs().max()) <= 1e-12, k


def test_head_ref_equals_autograd():
    torch.manual_seed(6)
    b, k, o = 3, 48, 7
    x = torch.randn(b, k, dtype=torch.float64, requires_grad=True)
    lin1, lin2 = nn.Linear(k, o).double(), nn.Linear(o, 1).double()
    out = lin2(TF.leaky_relu(lin1(x), 0.2))
    dout = torch.randn(b, dtype=torch.float64)
    out.backward(dout[:, None])
    r = V.head(x.detach(), lin1.weight.detach(), lin1.bias.detach(), lin2.weight.detach(), lin2.bias.detach(), 0.2, dout)
    assert float((r["out"] - out.detach().reshape(-1)).abs().max()) <= 1e-12
    for name, want in (("dx", x.grad), ("dw1", lin1.weight.grad), ("db1", lin1.bias.grad), ("dw2", lin2.weight.grad),
                       ("db2", lin2.bias.grad)):
        assert tuple(r[name].shape) == tuple(want.shape) and float((r[name] - want).abs().max()) <= 1e-12, name
    # the layout helpers are each other's inverse on representable values, and the pad pattern stays out of the data
    xi = torch.randint(-3, 4, (2, 5 * 4)).double()
    t = V.nhwc(xi, 5, 8, 4, V.BF16, pad_bits=0x7FC0)
    assert tuple(t.shape) == (2, 4, 8) and bool(torch.isnan(t[:, :, 5:].float()).all()) and torch.equal(V.from_nhwc(t, 5), xi)


# ----------------------------------------------------------------------------- 4. the checkpoint surface in the package
def E():
    return importlib.import_module("deep-super-resolution_amd.evaluate")


@pytest.mark.parametrize("size", [128, 256])
def test_layout_is_the_torch_copys_state_dict(size):
    for cin, nf in ((3, 64), (1, 8)):
        rsd = TorchVGGD(cin, nf, size).state_dict()
        assert E().vgg_discriminator_layout(cin, nf, size) == [(k, tuple(v.shape)) for k, v in rsd.items()]
        assert E().vgg_discriminator_layout(cin, nf, size) == V.key_table(cin, nf, size)
    assert len(E().vgg_discriminator_layout(input_size=size)) == {128: 60, 256: 72}[size]
    for bad in (64, 512, 0):
        with pytest.raises(ValueError):
            E().vgg_discriminator_layout(input_size=bad)
    with pytest.raises(ValueError):
        E().vgg_discriminator_layout(num_feat=0)


def test_inspect_reads_the_constructor_arguments(tmp_path):
    ref = TorchVGGD()
    got = E().inspect_vgg_discriminator(ref.state_dict())
    assert got == {"num_in_ch": 3, "num_feat": 64, "input_size": 128, "parameters": 14499401}
    assert got["parameters"] == sum(p.numel() for p in ref.parameters())
    small = TorchVGGD(1, 8, 256)
    sd = small.state_dict()
    want = {"num_in_ch": 1, "num_feat": 8, "input_size": 256, "parameters": sum(p.numel() for p in small.parameters())}
    assert E().inspect_vgg_discriminator(sd) == want
    assert E().inspect_vgg_discriminator({"params": dict(sd)}) == want
    assert E().inspect_vgg_discriminator({"params_ema": dict(sd), "params": {}}) == want
    assert E().inspect_vgg_discriminator({"module." + k: v for k, v in sd.items()}) == want
    path = tmp_path / "net_d.pth"                       # as a file: what torch.load(..., weights_only=True) hands back
    torch.save({"params": sd}, path)
    assert E().inspect_vgg_discriminator(torch.load(path, map_location="cpu", weights_only=True)) == want


def test_inspect_names_the_key_of_every_defect():
    sd = TorchVGGD(3, 8, 128).state_dict()
    ins = E().inspect_vgg_discriminator
    with pytest.raises(ValueError, match="'bn2_1.running_var' is missing"):
        ins({k: v for k, v in sd.items() if k != "bn2_1.running_var"})
    with pytest.raises(ValueError, match="'conv0_1.bias'"):               # BasicSR's blocks carry no conv bias
        ins(dict(sd, **{"conv0_1.bias": torch.zeros(8)}))
    with pytest.raises(ValueError, match="'conv3_1.weight' has shape"):   # a 3x3 where the stride-2 4x4 belongs
        ins(dict(sd, **{"conv3_1.weight": torch.zeros(64, 64, 3, 3)}))
    with pytest.raises(ValueError, match="'linear1.weight' has shape"):
        ins(dict(sd, **{"linear1.weight": torch.zeros(100, 64 * 8 * 8)}))
    with pytest.raises(ValueError, match="'bn5_0.weight' is missing"):    # a sixth stage begun and not finished
        ins(dict(sd, **{"conv5_0.weight": torch.zeros(64, 64, 3, 3)}))
    with pytest.raises(ValueError, match="'conv0_0.weight'"):
        ins({k: v for k, v in sd.items() if k != "conv0_0.weight"})
    with pytest.raises(ValueError, match="'conv0_0.weight'"):             # the U-Net discriminator's checkpoint is another net
        ins({"conv0.weight": torch.zeros(64, 3, 3, 3), "conv0.bias": torch.zeros(64)})
