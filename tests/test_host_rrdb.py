"""CPU: the RRDBNet surface (models/GAN/rrdbnet.py) -- keys, shapes, parameter counts, checkpoint round trips, the
yardstick's two forms of a convolution, receptive field, argument errors -- and the host-side refusals of dsr_conv_rdb_fwd,
which validates before it launches and therefore runs without a device (as tests/test_abi.py does for the other entry points)."""
import ctypes as C
import importlib

import pytest
import torch

import rrdb_ref as R

PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


def test_keys_shapes_and_parameter_counts():
    M = P("models.GAN.rrdbnet")
    for kw in (dict(), dict(scale=2, num_block=2), dict(scale=1, num_block=1), dict(num_feat=32, num_grow_ch=16, num_block=1),
               dict(num_in_ch=1, num_out_ch=1, num_block=1)):
        sd = M.RRDBNet(**kw).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.key_table(**kw), kw
    assert len(R.key_table()) == 702
    assert R.param_count(scale=4) == 16_697_987
    assert R.param_count(scale=2) == 16_703_171
    assert R.param_count(scale=1) == 16_723_907
    assert sum(p.numel() for p in M.RRDBNet().parameters()) == 16_697_987          # the module itself, default arguments
    for scale in (4, 2, 1):
        net = M.RRDBNet(scale=scale, num_block=1)
        assert sum(p.numel() for p in net.parameters()) == R.param_count(scale=scale, num_block=1)
        assert net.scale == scale and net.unshuffle == {4: 1, 2: 2, 1: 4}[scale]


def test_initialisation_of_the_dense_block_convs():
    M = P("models.GAN.rrdbnet")
    torch.manual_seed(0)
    blk = M.ResidualDenseBlock()
    for conv in blk._convs():
        assert float(conv.bias.detach().abs().max()) == 0.0
        fan_in = conv.weight.shape[1] * 9
        std = float(conv.weight.detach().std())
        assert abs(std / (0.1 * (2.0 / fan_in) ** 0.5) - 1.0) < 0.05, std        # Kaiming-normal x 0.1


def test_state_dict_round_trips_bare_and_wrapped(tmp_path):
    M, E = P("models.GAN.rrdbnet"), P("evaluate")
    torch.manual_seed(1)
    src = M.RRDBNet(num_block=2)
    path = E.save_model(src, "rrdb", str(tmp_path))
    a = E.load_model(M.RRDBNet(num_block=2), path)
    sd = src.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in a.state_dict().items())
    # BasicSR's wrapping; params_ema wins over params
    other = {k: v + 1 for k, v in sd.items()}
    for name, wrapped, want in (("ema", {"params": other, "params_ema": dict(sd)}, sd), ("plain", {"params": other}, other),
                                ("module", {"params_ema": {"module." + k: v for k, v in sd.items()}}, sd)):
        p = str(tmp_path / (name + ".pth"))
        torch.save(wrapped, p)
        b = E.load_model(M.RRDBNet(num_block=2), p)
        assert all(torch.equal(v, want[k]) for k, v in b.state_dict().items()), name
    # a file that loads today loads the same way: the SRGAN generator, bare and with the DataParallel prefix
    G = P("models.GAN.generator")
    g = G.Generator(2, 1)
    p = E.save_model(g, "srgan", str(tmp_path))
    g2 = E.load_model(G.Generator(2, 1), p)
    assert all(torch.equal(v, g.state_dict()[k]) for k, v in g2.state_dict().items())


def test_yardstick_tap_sum_equals_conv2d():
    g = torch.Generator().manual_seed(2)
    buf, w, b, res = R.exact_operands(3, 2, 9, 11, 96, 32, res=2)
    args = (buf[:, :96], w, b)
    kw = dict(slope=0.25, res1=res[0][:, :32], beta1=0.25, res2=res[1][:, 32:64], beta2=0.25)
    assert torch.equal(R.prefix_conv(*args, **kw), R.prefix_conv(*args, taps=True, **kw))       # integers: exact both ways
    x = torch.randn(1, 64, 5, 7, generator=g, dtype=torch.float64)
    wf = torch.randn(32, 64, 3, 3, generator=g, dtype=torch.float64) * 0.05
    a, t = R.prefix_conv(x, wf, None, slope=0.2), R.prefix_conv(x, wf, None, slope=0.2, taps=True)
    assert float((a - t).abs().max()) <= 1e-13 * float(R.prefix_conv_bound(x, wf, None, 64).max())


def test_exact_sweep_stays_in_its_regime():
    """x in [-3, 3], ternary weights of density 0.25, bias in [-4, 4], slope and betas 0.25, residuals in [-3, 3].  An output
    is acc or acc / 4 (LeakyReLU), then (acc + 4 r1) / 4, then (acc + 4 r1 + 16 r2) / 16: representable in bf16's 8 bits when the
    numerator stays below 2^8.  |acc| <= 176 would be sufficient on its own (176 + 12 + 48 < 256); the largest |acc| of these
    operands is printed and may lie above that (a 4.5-sigma tail over 133 k sums of ~430 terms), so representability of every
    output is checked directly, value by value -- and the GPU sweep rounds its yardstick with r16 either way, so it stays
    exact even if a value were not."""
    worst = 0.0
    for n, h, w, _ in R.EXACT_SHAPES:
        for cin, cout in R.EXACT_CASES:
            for nres in ((0,) if cout == 32 else (1, 2)):
                buf, wt, b, _, kw = R.exact_launch(n, h, w, cin, cout, nres)
                worst = max(worst, float(R.prefix_conv(buf[:, :cin], wt, b).abs().max()))
                y = R.prefix_conv(buf[:, :cin], wt, b, **kw)
                assert R.representable(y, R.BF16) and R.representable(y, R.F16), (n, h, w, cin, cout, nres)
    print("largest |acc| of the sweep:", worst)
    assert worst < 256, worst
    # the rounding cases: x in [-15, 15] leaves bf16's 8 bits (and stays exact in fp32, so r16 of it is defined)
    for cin, cout, nres in ((160, 32, 0), (192, 64, 2)):
        buf, wt, b, _, kw = R.exact_launch(2, 9, 65, cin, cout, nres, amp=15)
        y = R.prefix_conv(buf[:, :cin], wt, b, **kw)
        assert not R.representable(y, R.BF16) and float(y.abs().max()) < 2 ** 11
        R.r16(y, R.BF16)


def test_forward_cases_take_several_items_per_block():
    """The launcher's partition (R.fwd_plan, restated from csrc/conv_rdb.hip) of the multi-item forward cases of
    tests/test_gpu_rrdb.py, and that the case at the natural cap stays exact."""
    n, h, w = R.CAP_SHAPE
    items, blocks = R.fwd_plan(n, h, w)
    print(f"forward at {R.CAP_SHAPE} without max_blocks: {items} items on {blocks} blocks")
    assert (items, blocks) == (260, 256) and items > blocks
    assert R.fwd_plan(1, 16, 130, 2) == (6, 2)                     # the one multi-item case of R.EXACT_SHAPES: three a block
    assert all(R.fwd_plan(n_, h_, w_, mb)[0] <= 256 for n_, h_, w_, mb in R.EXACT_SHAPES)
    plans = [R.fwd_plan(2, 9, 65, mb) for mb in R.FLOAT_PARTITIONS]
    print("float forward partitions at (2, 9, 65), (items, blocks):", plans)
    assert plans == [(8, 8), (8, 1), (8, 3)]
    assert sorted({cin // 32 % 2 for cin, _, _ in R.FLOAT_PARTITION_CASES}) == [0, 1]       # K-block counts of both parities
    assert {cout for _, cout, _ in R.FLOAT_PARTITION_CASES} == {32, 64}
    # exact at the cap: |acc| <= 27 Cin + 4, the residual steps make it a multiple of 1/16 -- far below 2^24 in any order;
    # the stored value is r16 of it (the operands are checked where they are uploaded, the values here for one case)
    assert (27 * 192 + 4 + 12 + 48) * 16 < 2 ** 24
    buf, wt, b, res2, kw = R.exact_launch(n, h, w, 64, 32, 0)
    assert all(R.representable(t, d) for t in (buf, wt, b) for d in (R.BF16, R.F16))
    y = R.prefix_conv(buf[:, :64], wt, b, **kw)
    assert torch.equal(y * 4, (y * 4).round())
    R.r16(y, R.BF16)                                               # (asserts that the value is exact in fp32)


def test_receptive_halo_and_scale_errors():
    M, I = P("models.GAN.rrdbnet"), P("infer")
    assert M.RRDBNet(num_block=1).receptive_halo() == 19
    assert M.RRDBNet().receptive_halo() == 2 + 15 * 23 + 2 == 349
    assert M.RRDBNet(scale=2, num_block=2).receptive_halo() == 2 * 34
    assert M.RRDBNet(scale=1, num_block=1).receptive_halo() == 4 * 19
    net = M.RRDBNet(scale=2, num_block=1)
    assert I.receptive_halo(net) == 38 and I._factor(net) == 2
    g = P("models.GAN.generator").Generator(4, 3)
    assert I.receptive_halo(g) == 4 + 6 + 1 + 2 + 1 and I._factor(g) == 4        # the SRGAN generator: as before
    for bad in (3, 8, 0):
        with pytest.raises(ValueError):
            M.RRDBNet(scale=bad)
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 9, 8))                      # 9 is no multiple of the unshuffle factor (raised before any launch)
    with pytest.raises(ValueError):
        M.RRDBNet(scale=1, num_block=1)(torch.zeros(1, 3, 8, 6))
    with pytest.raises(ValueError):
        I._run(net, torch.zeros(1, 3, 16, 16), 7, 38)     # tile
    with pytest.raises(ValueError):
        I._run(net, torch.zeros(1, 3, 16, 16), 8, 37)     # halo


def _desc(L, **kw):
    one = 4096                      # a non-null "pointer" that is never dereferenced: validation fails first
    base = dict(dtype=L.BF16, N=1, H=8, W=8, Cin=64, Cout=32, x=one, ldx=192, w=one, bias=one, act=L.ACT_LEAKY, slope=0.2,
                res1=None, ldr1=0, r1_off=0, beta1=0.0, res2=None, ldr2=0, r2_off=0, beta2=0.0, y=one, ldy=192, y_off=64,
                max_blocks=0)
    base.update(kw)
    return L.RdbConv(**base)


def test_rdb_conv_refusals_before_any_launch():
    L = P("_lib")
    lib = L.lib()
    good = _desc(L)
    assert lib.dsr_conv_rdb_supported(C.byref(good)) == 1
    assert lib.dsr_conv_rdb_supported(None) == 0
    other = 8192
    bad = {
        "overlaps the input prefix": _desc(L, y_off=32),                                  # y == x and y_off < Cin
        "multiples of 32": _desc(L, y_off=72),                                            # misaligned offset
        "y_off + Cout > ldy": _desc(L, y_off=192),
        "null pointer": _desc(L, x=None),
        "null pointer ": _desc(L, y=None),
        "null pointer  ": _desc(L, w=None),
        "dtype": _desc(L, dtype=2),
        "Cout must be": _desc(L, Cout=16),
        "Cin must be": _desc(L, Cin=48),
        "ldx must be": _desc(L, Cin=96, ldx=64, y=other),
        "slope": _desc(L, slope=0.0),
        "residual range": _desc(L, Cin=192, Cout=64, y=other, y_off=0, res1=other, ldr1=192, r1_off=32, beta1=0.2, act=L.ACT_NONE),
        "residual stride": _desc(L, Cin=192, Cout=64, y=other, y_off=0, res2=4096, ldr2=192, r2_off=8, beta2=0.2, act=L.ACT_NONE),
        "its stride": _desc(L, Cin=192, Cout=64, y=other, y_off=0, res1=4096, ldr1=64, r1_off=32, beta1=0.2, act=L.ACT_NONE),
        "per image": _desc(L, H=4096, W=4096, y=other),
        "2^32": _desc(L, N=64, H=1024, W=1024, y=other),
    }
    for what, d in bad.items():
        rc = lib.dsr_conv_rdb_fwd(C.byref(d), None)
        assert rc == -1, (what, rc)                                                       # DSR_E_ARG
        assert what.strip() in lib.dsr_last_error().decode(), (what, lib.dsr_last_error())
    assert lib.dsr_conv_rdb_fwd(None, None) == -1
    assert lib.dsr_conv_rdb_supported(C.byref(_desc(L, Cout=16))) == 0
    assert lib.dsr_scale_add16(L.BF16, None, 0.2, None, None, 8, None) == -1
    assert lib.dsr_scale_add16(2, 4096, 0.2, None, 4096, 8, None) == -1
    assert lib.dsr_scale_add16(L.BF16, 4096, 0.2, None, 4096, 0, None) == -1


def test_rrdb_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        return                      # (with a device the same call is the GPU file's business)
    with pytest.raises(RuntimeError):
        P("models.GAN.rrdbnet").RRDBNet(num_block=1)(torch.zeros(1, 3, 8, 8))
