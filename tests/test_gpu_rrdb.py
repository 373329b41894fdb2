"""GPU: RRDBNet on the HIP path (models/GAN/rrdbnet.py, csrc/conv_rdb.hip) against the float64 yardstick tests/rrdb_ref.py.

1. one dsr_conv_rdb_fwd launch on exact-integer operands: bit for bit, every byte outside the output range untouched, also
   with 260 work items on the launcher's cap of 256 blocks;
2. one launch on float data: a derived per-element bound, and the same bits under every partition (max_blocks);
3. whole networks, fused and composed, against the float64 network with the storage-model network as the floor;
4. gradients of the composed path (tests/parity_util.compare_grads);
5. the training recipe, HIP-graph replay and the refreshed weight images;
6. the inference surface (tiles, self-ensemble, evaluate_generator), and the SRGAN generator's unchanged tiling."""
import ctypes as C
import importlib

import pytest
import torch

import parity_util
import rrdb_ref as R
from oracle import filler

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
MARGIN = 1024         # sentinel elements on each side of a raw buffer
SENTINEL = 7777.0


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]


# ----------------------------------------------------------------------------- raw launches
class Raw:
    """NHWC 16-bit device tensors inside sentinel-filled allocations; check() asserts the margins came back untouched."""

    def __init__(self, dev):
        self.dev, self.flats = dev, []

    def put(self, nchw64, dtype):
        n, c, h, w = nchw64.shape
        t = nchw64.permute(0, 2, 3, 1).contiguous().to(R.DTYPES[dtype])
        assert torch.equal(t.double(), nchw64.permute(0, 2, 3, 1)), "operand not representable"
        flat = torch.full((t.numel() + 2 * MARGIN,), SENTINEL, dtype=t.dtype, device=self.dev)
        flat[MARGIN:MARGIN + t.numel()] = t.reshape(-1).to(self.dev)
        self.flats.append(flat)
        return flat[MARGIN:MARGIN + t.numel()].view(n, h, w, c)

    def check(self):
        torch.cuda.synchronize()
        for flat in self.flats:
            assert bool((flat[:MARGIN] == SENTINEL).all()) and bool((flat[-MARGIN:] == SENTINEL).all()), "write outside a tensor"


def _packed(wt64, n, h, w, dtype, dev):
    F, L = P("functional"), P("_lib")
    weight = wt64.float().to(dev)
    cout, cin = weight.shape[:2]
    wf, _ = F.packed_weights(weight, L.ConvDesc(dtype, n, h, w, cin, cout, 3, 3, 1, 1, 0), R.DTYPES[dtype])
    return wf, weight


def _nchw64(t, c0, c):
    return t[..., c0:c0 + c].double().permute(0, 3, 1, 2).contiguous().cpu()


def _launch(dev, dtype, n, h, w, cin, cout, nres, max_blocks, buf, wt, bias, res2, kw, y_off64=64, exact=True, bits=False):
    """Issue the launch as the model does (Cout = 32 in place; Cout = 64 into a second 192-channel tensor at channel offset
    y_off64) and return (y [N, Cout, H, W] float64, the untouched-bytes verdict) -- with `bits` the stored 16-bit patterns
    [N, H, W, Cout] (int16, on the host) instead of the float64 values."""
    F = P("functional")
    raw = Raw(dev)
    put = raw.put if exact else (lambda t, d: t.permute(0, 2, 3, 1).contiguous().to(R.DTYPES[d]).to(dev))
    xb = put(buf, dtype)
    before = xb.clone()
    wf, keep = _packed(wt, n, h, w, dtype, dev)
    b = bias.float().to(dev)
    slope = kw.get("slope")
    args = dict(act=F.ACT_NONE if slope is None else F.ACT_LEAKY, slope=slope or 0.0, max_blocks=max_blocks)
    if cout == 32:
        yb, y_off, ybefore = xb, cin, before
    else:
        pattern = torch.arange(n * h * w * 192, dtype=torch.float64).remainder(17).sub(8).view(n, 192, h, w)
        yb = put(pattern, dtype)
        y_off, ybefore = y_off64, yb.clone()
        args.update(res1=xb, r1_off=0, beta1=kw["beta1"])
        if nres == 2:
            args.update(res2=put(res2, dtype), r2_off=R.R2_OFF, beta2=kw["beta2"])
    F.rdb_conv(xb, cin, wf, b, yb, y_off, cout, **args)
    raw.check()
    # every byte outside [y_off, y_off + Cout) of the written tensor, and all of the input tensor, unchanged
    i16 = lambda t: t.view(torch.int16)
    keep_mask = torch.ones(192, dtype=torch.bool, device=dev)
    keep_mask[y_off:y_off + cout] = False
    untouched = torch.equal(i16(yb)[..., keep_mask], i16(ybefore)[..., keep_mask])
    if cout == 64:
        untouched = untouched and torch.equal(i16(xb), i16(before))
    if bits:
        return i16(yb)[..., y_off:y_off + cout].cpu(), untouched
    return _nchw64(yb, y_off, cout), untouched


EXACT = [pytest.param(n, h, w, mb, cin, cout, nres, id=f"{n}x{h}x{w}-{cin}to{cout}-res{nres}")
         for n, h, w, mb in R.EXACT_SHAPES for cin, cout in R.EXACT_CASES for nres in ((0,) if cout == 32 else (1, 2))]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,h,w,mb,cin,cout,nres", EXACT)
def test_single_launch_exact(dev, dtype, n, h, w, mb, cin, cout, nres):
    """Integers in [-3, 3], ternary weights, slope = beta = 0.25: nothing to round, torch.equal."""
    buf, wt, bias, res2, kw = R.exact_launch(n, h, w, cin, cout, nres)
    want = R.r16(R.prefix_conv(buf[:, :cin], wt, bias, **kw), dtype)
    got, untouched = _launch(dev, dtype, n, h, w, cin, cout, nres, mb, buf, wt, bias, res2, kw, y_off64=64 if nres == 1 else 0)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert untouched


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cin,cout,nres", [(64, 32, 0), (96, 32, 0), (128, 32, 0), (160, 32, 0), (192, 64, 2)])
def test_single_launch_exact_natural_cap(dev, dtype, cin, cout, nres):
    """No max_blocks: the launcher's own cap of 256 blocks.  (65, 9, 65) is 65 images x 2 x 2 ragged tiles = 260 work items on
    256 blocks, so blocks 0..3 take a second item (tile 256 + b: the four tiles of the last image) after the hand-over under
    their last K-block -- with 2, 3, 4, 5 and 6 K-blocks, both parities of the stage index at that point.  Operands and
    assertions of test_single_launch_exact."""
    n, h, w = R.CAP_SHAPE
    items, blocks = R.fwd_plan(n, h, w)
    assert (items, blocks) == (260, R.RDB_GRID_CAP)
    if (cin, nres) not in _CAP_REF:                # operands and the float64 value: once for both types, never modified
        case = R.exact_launch(n, h, w, cin, cout, nres)
        _CAP_REF[(cin, nres)] = (case, R.prefix_conv(case[0][:, :cin], case[1], case[2], **case[4]))
    (buf, wt, bias, res2, kw), y64 = _CAP_REF[(cin, nres)]
    want = R.r16(y64, dtype)
    got, untouched = _launch(dev, dtype, n, h, w, cin, cout, nres, 0, buf, wt, bias, res2, kw, y_off64=0)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert untouched


_CAP_REF = {}


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cin,cout,nres", [(160, 32, 0), (192, 64, 2)])
def test_single_launch_exact_rounded(dev, dtype, cin, cout, nres):
    """x in [-15, 15]: the sums leave bf16's 8 bits, the one rounding (to nearest even) is the yardstick's r16."""
    n, h, w = 2, 9, 65
    buf, wt, bias, res2, kw = R.exact_launch(n, h, w, cin, cout, nres, amp=15)
    exact = R.prefix_conv(buf[:, :cin], wt, bias, **kw)
    want = R.r16(exact, dtype)
    got, untouched = _launch(dev, dtype, n, h, w, cin, cout, nres, 0, buf, wt, bias, res2, kw, y_off64=0)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert untouched
    if dtype == R.BF16:
        assert not torch.equal(want, exact)


def _float_case(dtype, cin, cout, nres, n=2, h=9, w=65):
    """The float operands of one launch: (buf, wt, bias, res2 buffer or None, keyword arguments of prefix_conv)."""
    g = torch.Generator().manual_seed(cin + nres)
    t16 = lambda t: t.to(R.DTYPES[dtype]).double()
    buf = t16(torch.randn(n, 192, h, w, generator=g, dtype=torch.float64))
    wt = t16(torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.05)
    bias = (torch.randn(cout, generator=g, dtype=torch.float64) * 0.1).float().double()
    res2 = t16(torch.randn(n, 192, h, w, generator=g, dtype=torch.float64)) if nres == 2 else None
    kw = dict(slope=R.F32(0.2) if cout == 32 else None)
    if nres >= 1:
        kw.update(res1=buf[:, :cout], beta1=R.F32(0.2))
    if nres == 2:
        kw.update(res2=res2[:, R.R2_OFF:R.R2_OFF + cout], beta2=R.F32(0.2))
    return buf, wt, bias, res2, kw


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cin,cout,nres", R.FLOAT_PARTITION_CASES)
def test_single_launch_partition_independent_float(dev, dtype, cin, cout, nres):
    """The operands of test_single_launch_float under max_blocks = 0, 1, 3: the partition assigns tiles to blocks and enters
    no sum, so the stored output is the same bits for all three.  (2, 9, 65) is 8 tiles: 8 blocks of one item, one block of 8,
    three blocks of 3, 3 and 2.  Cin = 96, 128, 192 are 3, 4 and 6 K-blocks: the hand-over to the next item happens on
    either halo stage; Cout = 32 in place and Cout = 64 with one and two residuals.  The max_blocks = 0 result is the one
    test_single_launch_float holds to its bound."""
    n, h, w = 2, 9, 65
    buf, wt, bias, res2, kw = _float_case(dtype, cin, cout, nres)
    runs = {}
    for mb in R.FLOAT_PARTITIONS:
        items, blocks = R.fwd_plan(n, h, w, mb)
        assert (items, blocks) == (8, mb or 8)
        runs[mb], untouched = _launch(dev, dtype, n, h, w, cin, cout, nres, mb, buf, wt, bias, res2, kw, y_off64=0, exact=False,
                                      bits=True)
        assert untouched, mb
    for mb in R.FLOAT_PARTITIONS[1:]:
        diff = runs[mb] != runs[0]
        assert not bool(diff.any()), (mb, int(diff.sum()))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cin,cout,nres", [(64, 32, 0), (96, 32, 0), (128, 32, 0), (160, 32, 0), (192, 64, 1), (192, 64, 2)])
def test_single_launch_float(dev, dtype, cin, cout, nres):
    """N(0, 1) data, N(0, 0.05) weights, slope = beta = 0.2.  Per element, none excluded:
        |y - y64| <= u |y64| + (9 Cin + 4) 2^-24 A,   u = one ulp of the type, A = conv(|x|, |w|) + |b| (+ |residuals|):
    9 Cin + 4 fp32 operations of relative error 2^-24 each on magnitudes bounded by A, then one rounding to 16 bits.
    Measured on the MI355X: the largest (error - bound) over all twelve cases is -1.2e-4 (192 -> 64 with both residuals)."""
    n, h, w = 2, 9, 65
    buf, wt, bias, res2, kw = _float_case(dtype, cin, cout, nres)
    y64 = R.prefix_conv(buf[:, :cin], wt, bias, **kw)
    bkw = {k: v for k, v in kw.items() if k != "slope"}
    A = R.prefix_conv_bound(buf[:, :cin], wt, bias, cin, **bkw)
    got, untouched = _launch(dev, dtype, n, h, w, cin, cout, nres, 0, buf, wt, bias, res2, kw, y_off64=0, exact=False)
    u = 2.0 ** -8 if dtype == R.BF16 else 2.0 ** -10
    bound = u * y64.abs() + (9 * cin + 4) * 2.0 ** -24 * A
    excess = ((got - y64).abs() - bound).max()
    print(f"float launch {cin}->{cout} res{nres}: max err {float((got - y64).abs().max()):.3e}, max (err - bound) {float(excess):.3e}")
    assert float(excess) <= 0.0
    assert untouched


# ----------------------------------------------------------------------------- networks
def _net(dev, dtype=torch.bfloat16, salt=0, **kw):
    M = P("models.GAN.rrdbnet")
    net = M.RRDBNet(**kw)
    sd = filler.fill_state_dict(net.state_dict(), salt=salt)
    net.load_state_dict(sd)
    net.to(dev)
    net.compute_dtype = dtype
    return net, sd


def _count(fn):
    """Run fn with the launch log on; returns (result, {entry point: launches})."""
    L = P("_lib")
    L.LAUNCH_LOG = log = []
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.LAUNCH_LOG = None
    counts = {}
    for name, _, _ in log:
        counts[name] = counts.get(name, 0) + 1
    return out, counts


NETS = [pytest.param(dict(num_block=1), (1, 3, 12, 20), id="b1-12x20"),
        pytest.param(dict(num_block=1), (2, 3, 9, 65), id="b1-9x65"),
        pytest.param(dict(num_block=2), (1, 3, 12, 20), id="b2-12x20"),
        pytest.param(dict(num_block=2), (2, 3, 9, 65), id="b2-9x65"),
        pytest.param(dict(num_block=1, scale=2), (1, 3, 16, 24), id="b1-scale2"),
        pytest.param(dict(num_block=1, num_feat=32, num_grow_ch=16), (1, 3, 12, 20), id="f32g16-composed-only")]


@pytest.mark.parametrize("kw,shape", NETS)
def test_network_forward(dev, monkeypatch, kw, shape):
    """max|y_hip - y_f64| <= 2 E_floor + 1e-3 max|y_f64|, E_floor = max|y_sim - y_f64| (storage-model yardstick), for the
    fused no-grad forward, the composed forward, and their mutual difference; the fused path is 15 launches of the new
    kernel per RRDB and one box copy (conv_first's output into the first buffer), none inside the body.

    Measured on the MI355X (bf16), E_floor / bound / fused / composed / mutual, max|y_f64|:
        num_block=1, 1x3x12x20   8.95e-3 / 1.98e-2 / 8.76e-3 / 9.70e-3 / 7.12e-3,  1.93
        num_block=1, 2x3x9x65    9.80e-3 / 2.16e-2 / 1.07e-2 / 9.39e-3 / 9.72e-3,  2.01
        num_block=2, 1x3x12x20   1.04e-2 / 2.31e-2 / 1.01e-2 / 9.99e-3 / 8.43e-3,  2.25
        num_block=2, 2x3x9x65    1.14e-2 / 2.51e-2 / 1.04e-2 / 1.13e-2 / 8.37e-3,  2.27
        scale=2,     1x3x16x24   6.19e-3 / 1.35e-2 / 5.86e-3 / 6.37e-3 / 3.69e-3,  1.09
        num_feat=32, 1x3x12x20   1.04e-2 / 2.18e-2 / 1.01e-2 / 1.01e-2 / 0 (one path), 0.90"""
    net, sd = _net(dev, **kw)
    x = filler.tensor("in:rrdb" + str(shape), shape, 0.5, 0.5)
    scale = kw.get("scale", 4)
    y64 = R.network(sd, x, scale)
    ysim = R.network(sd, x, scale, dtype=R.BF16)
    floor = float((ysim - y64).abs().max())
    bound = 2.0 * floor + 1e-3 * float(y64.abs().max())
    xd = x.to(dev)
    with torch.no_grad():
        fused, counts = _count(lambda: net(xd))
    composed, ccounts = _count(lambda: net(xd))                      # grad mode on, parameters require grad
    monkeypatch.setenv("DSR_RRDB_FUSED", "0")
    with torch.no_grad():
        off, ocounts = _count(lambda: net(xd))
    monkeypatch.delenv("DSR_RRDB_FUSED")
    nb = kw["num_block"]
    if kw.get("num_feat", 64) == 64:
        assert counts.get("dsr_conv_rdb_fwd", 0) == 15 * nb and counts.get("dsr_box_copy", 0) == 1, counts
        assert counts.get("dsr_scale_add16", 0) == 1                 # the global skip only
    else:
        assert counts.get("dsr_conv_rdb_fwd", 0) == 0 and counts.get("dsr_box_copy", 0) == 42 * nb, counts
    for c in (ccounts, ocounts):
        # composed: 2 + 3 + 4 + 5 concatenation copies per dense block, one scale-add per dense block, RRDB and global skip
        assert c.get("dsr_conv_rdb_fwd", 0) == 0 and c.get("dsr_box_copy", 0) == 42 * nb, c
        assert c.get("dsr_scale_add16", 0) == 4 * nb + 1
    assert torch.equal(off, composed.detach())
    e_f = float((fused.double().cpu() - y64).abs().max())
    e_c = float((composed.detach().double().cpu() - y64).abs().max())
    e_m = float((fused - composed.detach()).abs().max())
    print(f"network {kw} {shape}: E_floor {floor:.3e} bound {bound:.3e} fused {e_f:.3e} composed {e_c:.3e} mutual {e_m:.3e} "
          f"max|y| {float(y64.abs().max()):.3e}")
    assert tuple(fused.shape) == (shape[0], 3, shape[2] * scale, shape[3] * scale) and fused.dtype == torch.float32
    assert e_f <= bound and e_c <= bound and e_m <= bound, (e_f, e_c, e_m, bound)


def test_composed_gradients(dev):
    """Every parameter gradient and the input gradient of the composed path against the float64 network's, with the
    storage-model network (composed rounding points) as the floor: parity_util.compare_grads as it stands."""
    shape = (2, 3, 12, 20)
    net, sd = _net(dev, num_block=1)
    x = filler.tensor("in:rrdb_grad", shape, 0.5, 0.5)
    probe = filler.tensor("in:rrdb_probe", (2, 3, 48, 80))

    def ref_grads(dtype):
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
        xi = x.double().clone().requires_grad_(True)
        y = R.network(leaves, xi, 4, dtype=dtype, fused=False)
        (y * probe.double()).sum().backward()
        out = {k: v.grad for k, v in leaves.items()}
        out["input"] = xi.grad
        return out

    ref, sim = ref_grads(None), ref_grads(R.BF16)
    xd = x.to(dev).requires_grad_(True)
    y, counts = _count(lambda: net(xd))
    assert counts.get("dsr_conv_rdb_fwd", 0) == 0
    (y * probe.to(dev)).sum().backward()
    hip = {k: p.grad for k, p in net.named_parameters()}
    hip["input"] = xd.grad
    assert all(g is not None for g in hip.values())
    bad, table = parity_util.compare_grads(hip, ref, sim)
    worst = sorted(table.items(), key=lambda kv: kv[1][0])[:5]
    print("composed gradients, lowest cosines (cos_hip, cos_floor, ratio_hip, ratio_floor, numel):", worst)
    assert len(table) == len(ref) and not bad, bad


def _batch(dev):
    lr = filler.tensor("in:rrdb_lr", (16, 3, 8, 8), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:rrdb_hr", (16, 3, 32, 32), 0.5, 0.5).to(dev)
    return lr, hr


def _params(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def test_l1_step_lowers_the_loss_and_replays_from_a_graph(dev):
    O, S = P("optim"), P("steps")
    lr, hr = _batch(dev)

    def setup():
        net, _ = _net(dev, num_block=1)
        net.train()
        opt = O.FusedAdam(net.parameters(), lr=1e-3)
        ema = O.WeightEMA(net, decay=0.9)
        return net, opt, ema

    net, opt, ema = setup()
    losses = []
    for _ in range(5):
        loss, fake = S.gen_l1_step(net, opt, lr, hr, ema=ema)
        losses.append(loss.clone())
    losses = [float(v) for v in losses]
    print("L1 over 5 steps:", losses)
    assert losses[-1] < losses[0] and all(v == v for v in losses)
    assert int(ema.n_averaged.item()) == 5

    # the same five steps, two eager and three replayed from a HIP graph: bit for bit
    net2, opt2, ema2 = setup()
    out = []
    graphed = S.GraphedStep(lambda: S.gen_l1_step(net2, opt2, lr, hr, ema=ema2), warmup=2)
    for _ in range(3):
        loss2, fake2 = graphed()
        out.append(loss2.clone())
    torch.cuda.synchronize()
    assert float(out[-1]) == losses[-1]
    assert torch.equal(fake2, fake)
    a, b = _params(net), _params(net2)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_fused_forward_graph_capture_and_updated_weights(dev):
    O, S, M = P("optim"), P("steps"), P("models.GAN.rrdbnet")
    net, _ = _net(dev, num_block=1)
    x = filler.tensor("in:rrdb_cap", (1, 3, 12, 20), 0.5, 0.5).to(dev)
    with torch.no_grad():
        eager = net(x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = net(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)
    # an optimiser step rewrites the weights through raw pointers and refreshes their packed images (repack_cached): the
    # fused forward must see them -- compare with a freshly constructed model loaded from the state_dict
    lr, hr = _batch(dev)
    opt = O.FusedAdam(net.parameters(), lr=1e-3)
    S.gen_l1_step(net, opt, lr, hr)
    with torch.no_grad():
        after, counts = _count(lambda: net(x))
    assert counts.get("dsr_conv_rdb_fwd", 0) == 15
    assert not torch.equal(after, eager)
    fresh = M.RRDBNet(num_block=1)
    fresh.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    fresh.to(dev)
    with torch.no_grad():
        assert torch.equal(fresh(x), after)


# ----------------------------------------------------------------------------- inference surface
def test_super_resolve_tiles_ensemble_and_evaluate(dev):
    I, E = P("infer"), P("evaluate")
    net, _ = _net(dev, num_block=1)
    lr = filler.tensor("in:rrdb_sr", (1, 3, 24, 40), 0.5, 0.5).to(dev)
    whole = I.super_resolve(net, lr)
    assert tuple(whole.shape) == (1, 3, 96, 160) and net.compute_dtype == torch.bfloat16
    tiled = I.super_resolve(net, lr, tile=8, halo=net.receptive_halo())
    assert torch.equal(tiled, whole)
    ens = I.super_resolve(net, lr, self_ensemble=True)
    singles = [I.d4_inverse(I.super_resolve(net, I.d4(lr, k)), k) for k in range(8)]
    mean = torch.stack(singles).double().mean(0).float()
    assert float((ens - mean).abs().max()) <= 1e-6
    pairs = [(filler.tensor(f"in:rrdb_ev{i}", (1, 3, 12, 16), 0.5, 0.5).to(dev),
              filler.tensor(f"in:rrdb_evhr{i}", (1, 3, 48, 64), 0.5, 0.5).to(dev), f"img{i}") for i in range(2)]
    res = E.evaluate_generator(net, pairs, with_ssim=False, y_channel=True)
    for key in ("psnr", "psnr_y"):
        assert len(res[key]) == 2 and all(v == v and abs(v) != float("inf") for v in res[key].values()), res
    # an unshuffling model tiles on its grid
    net2, _ = _net(dev, num_block=1, scale=2)
    lr2 = filler.tensor("in:rrdb_sr2", (1, 3, 16, 24), 0.5, 0.5).to(dev)
    whole2 = I.super_resolve(net2, lr2)
    assert tuple(whole2.shape) == (1, 3, 32, 48)
    assert torch.equal(I.super_resolve(net2, lr2, tile=8, halo=net2.receptive_halo()), whole2)
    with pytest.raises(ValueError):
        I.super_resolve(net2, lr2, tile=7, halo=38)


def test_srgan_generator_tiling_is_unchanged(dev):
    """super_resolve of the SRGAN generator against the tiling loop as it was before RRDBNet (factor from the shuffle
    blocks, halo = 4 + 2 blocks + 1 + 2 + 1), restated here."""
    I, G = P("infer"), P("models.GAN.generator")
    g = G.Generator(4, 2)
    g.load_state_dict(filler.fill_state_dict(g.state_dict()))
    g.to(dev)
    lr = filler.tensor("in:srgan_tiles", (1, 3, 24, 40), 0.5, 0.5).to(dev)
    got = I.super_resolve(g, lr, tile=8)
    halo, f, tile = 4 + 2 * 2 + 1 + 2 + 1, 4, 8
    g.eval()
    g.compute_dtype = torch.float16
    want = torch.empty((1, 3, 96, 160), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for y0 in range(0, 24, tile):
            for x0 in range(0, 40, tile):
                y1, x1 = min(y0 + tile, 24), min(x0 + tile, 40)
                ya, xa, yb, xb = max(y0 - halo, 0), max(x0 - halo, 0), min(y1 + halo, 24), min(x1 + halo, 40)
                sr = g(lr[:, :, ya:yb, xa:xb].contiguous())
                want[:, :, y0 * f:y1 * f, x0 * f:x1 * f] = sr[:, :, (y0 - ya) * f:(y1 - ya) * f, (x0 - xa) * f:(x1 - xa) * f]
    assert torch.equal(got, want)
    assert I.receptive_halo(g) == halo
