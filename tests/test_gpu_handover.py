"""GPU: functional.Handover at the functional level -- two-node chains built by hand in bf16, one per kind, each run plain, with
a second consumer of the linked activation, and with a hook on it.  The single-consumer precondition is checked by the link
itself: "bn" falls back to the producer's own reduce pass, the other kinds raise before the producer launches anything.  Also
the version guards of the two recompute paths (weight AND bias) and a second backward over a retained graph."""
import importlib

import pytest
import torch
import torch.nn.functional as TF

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


def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-20))


def cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-30))


def rnd(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) - 0.5) * 2 * scale).to(torch.bfloat16).float()


def logged(fn):
    """Ordered names of the launches fn makes (_lib.LAUNCH_LOG)."""
    L = P("_lib")
    L.LAUNCH_LOG = []
    try:
        fn()
        torch.cuda.synchronize()
        return [e[0] for e in L.LAUNCH_LOG]
    finally:
        L.LAUNCH_LOG = None


SPOILERS = ("consumer", "hook")


def probe_of(shape):
    return rnd(90, shape) * 0.5 + 0.5            # (one sign: the one-element PReLU gradient below is then no cancelling sum)


def spoil(z, how, loss):
    """The linked activation z gets a second consumer, or a hook that returns a new tensor."""
    if how == "consumer":
        return loss + (z.float() * probe_of(tuple(z.shape)).to(z.device)).sum()
    if how == "hook":
        z.register_hook(lambda g: g.clone())
    return loss


# ----------------------------------------------------------------------------- "bn"
def bn_chain(F, dev, how, retain=False):
    """ConvBNAct (64 -> 64, stride 1, LeakyReLU, train) into ConvBNAct (64 -> 64, stride 2), N = 2, 32 x 32.  Returns the launch
    names and the gradients (x, then both layers' weight / gamma / beta)."""
    x = rnd(1, (2, 32, 32, 64)).to(torch.bfloat16).to(dev).requires_grad_(True)
    ps = []
    for i in range(2):
        ps += [rnd(10 + i, (64, 64, 3, 3), 0.06).to(dev).requires_grad_(True), (1 + rnd(20 + i, (64,), 0.3)).to(dev).requires_grad_(True),
               rnd(30 + i, (64,), 0.3).to(dev).requires_grad_(True)]
    bias = [rnd(35 + i, (64,), 0.1).to(dev) for i in range(2)]      # (in front of a train-mode BatchNorm: no gradient)
    stats = [torch.zeros(64, device=dev), torch.ones(64, device=dev), torch.zeros((), dtype=torch.long, device=dev)]
    link = F.Handover()

    def run():
        z = F.ConvBNAct.apply(x, ps[0], bias[0], ps[1], ps[2], *[s.clone() for s in stats], None, None,
                              dict(stride=1, pad=1, act=F.ACT_LEAKY, slope=0.2, train=True, out_link=link))
        out = F.ConvBNAct.apply(z, ps[3], bias[1], ps[4], ps[5], *[s.clone() for s in stats], None, None,
                                dict(stride=2, pad=1, act=F.ACT_LEAKY, slope=0.2, train=True, in_link=link))
        loss = spoil(z, how, (out.float() * rnd(2, tuple(out.shape)).to(dev)).sum())
        if not retain:
            loss.backward()
            return
        loss.backward(retain_graph=True)
        torch.cuda.synchronize()
        first.extend(t.grad.clone() for t in [x] + ps)
        loss.backward()

    first = []
    names = logged(run)
    return names, [t.grad.clone() for t in [x] + ps], first


@pytest.mark.parametrize("how", SPOILERS)
def test_bn_handover_recomputes_its_sums_when_the_gradient_was_touched(dev, how, monkeypatch):
    """The plain chain takes dsr_conv_dgrad_bn (asserted) and the producer skips its reduce pass.  With a second consumer or a
    hook the consumer still deposits, the producer sees another tensor and runs its own reduce over the complete gradient: one
    dsr_pw_bn_act_bwd_reduce more than the plain chain, and every gradient equal to the DGRAD_BN = False run of the same graph
    (tolerances of test_discriminator_batchnorm_sums_in_the_next_layers_input_gradient: fp32 summation order, 2e-3; the bf16
    input gradient 1e-2 and cosine 0.99999)."""
    F = P("functional")
    plain, _, _ = bn_chain(F, dev, None)
    assert plain.count("dsr_conv_dgrad_bn") == 1 and plain.count("dsr_pw_bn_act_bwd_reduce") == 1, plain
    names, got, _ = bn_chain(F, dev, how)
    assert names.count("dsr_conv_dgrad_bn") == 1 and names.count("dsr_pw_bn_act_bwd_reduce") == 2, names
    monkeypatch.setattr(F, "DGRAD_BN", False)
    names_off, ref, _ = bn_chain(F, dev, how)
    assert names_off.count("dsr_conv_dgrad_bn") == 0 and names_off.count("dsr_pw_bn_act_bwd_reduce") == 2, names_off
    assert rel_err(got[0], ref[0]) < 1e-2 and cos(got[0], ref[0]) > 0.99999
    for a, b in zip(got[1:], ref[1:]):
        assert torch.isfinite(a).all() and rel_err(a, b) < 2e-3, rel_err(a, b)


def test_second_backward_over_a_retained_graph_takes_the_separate_launches(dev):
    """The "bn" chain, backward(retain_graph=True) and backward again: the first pass spends the link, the second finds no
    offer and runs the plain input gradient and the producer's reduce pass; the accumulated gradients are twice the first
    pass's (same tolerances as above)."""
    F = P("functional")
    names, total, first = bn_chain(F, dev, None, retain=True)
    assert names.count("dsr_conv_dgrad_bn") == 1 and names.count("dsr_pw_bn_act_bwd_reduce") == 1 + 2, names
    assert rel_err(total[0], 2 * first[0]) < 1e-2 and cos(total[0], first[0]) > 0.99999
    for a, b in zip(total[1:], first[1:]):
        assert torch.isfinite(a).all() and rel_err(a, 2 * b) < 2e-3, rel_err(a, 2 * b)


# ----------------------------------------------------------------------------- "act"
def act_chain(F, dev, consumer, how):
    """ConvAct (ReLU, 64 -> 64) into a ConvAct or into MaxPool2, N = 1, 16 x 16."""
    x = rnd(3, (1, 16, 16, 64)).to(torch.bfloat16).to(dev).requires_grad_(True)
    w0, w1 = (rnd(40 + i, (64, 64, 3, 3), 0.06).to(dev).requires_grad_(True) for i in range(2))
    link = F.Handover()
    res = {}

    def run():
        z = F.ConvAct.apply(x, w0, None, None, dict(stride=1, pad=1, act=F.ACT_RELU, out_link=link))
        if consumer == "conv":
            out = F.ConvAct.apply(z, w1, None, None, dict(stride=1, pad=1, act=F.ACT_NONE, in_link=link))
        else:
            out = F.MaxPool2.apply(z, link)
        loss = spoil(z, how, (out.float() * rnd(4, tuple(out.shape)).to(dev)).sum())
        res["out"] = out.detach().clone()
        loss.backward()

    names = logged(run)
    return names, [res["out"], x.grad.clone(), w0.grad.clone()] + ([w1.grad.clone()] if consumer == "conv" else [])


@pytest.mark.parametrize("consumer", ["conv", "pool"])
def test_act_handover_raises_when_the_gradient_was_touched(dev, consumer):
    """The plain chain folds the ReLU mask into its consumer's launch (asserted: no dsr_pw_act_bwd) and is bit-identical to
    ACT_LINKS = False.  A premasked gradient with anything added cannot be repaired: a second consumer or a hook raises."""
    F = P("functional")
    taken = "dsr_conv_dgrad_masked" if consumer == "conv" else "dsr_maxpool2_relu_bwd"
    names, got = act_chain(F, dev, consumer, None)
    assert names.count(taken) == 1 and names.count("dsr_pw_act_bwd") == 0, names
    try:
        F.ACT_LINKS = False
        names_off, ref = act_chain(F, dev, consumer, None)
    finally:
        F.ACT_LINKS = True
    assert names_off.count(taken) == 0 and names_off.count("dsr_pw_act_bwd") == 1, names_off
    assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref))
    for how in SPOILERS:
        with pytest.raises(RuntimeError, match="Handover 'act'.*second consumer or a hook.*ACT_LINKS"):
            act_chain(F, dev, consumer, how)


# ----------------------------------------------------------------------------- "ps"
def ps_tensors(dev):
    return dict(x=rnd(5, (1, 8, 8, 64)), w=rnd(50, (256, 64, 3, 3), 0.06), b=rnd(51, (256,), 0.1), a=torch.tensor([0.25]),
                w3=rnd(52, (3, 64, 9, 9), 0.02), b3=rnd(53, (3,), 0.1), probe=rnd(6, (1, 3, 16, 16)), probe_z=probe_of((1, 16, 16, 64)))


def ps_chain(F, dev, how):
    """The shuffle block (3x3 64 -> 256, PixelShuffle, PReLU) on 8 x 8 into the 9x9 tail on 16 x 16, N = 1: the smallest tail the
    kernel sweeps cover (test_dgrad_ps_exact).  dsr_conv_dgrad_ps_supported itself accepts down to 2 x 2, where the generic
    kernels around it (a 3x3 convolution of a 1 x 1 map) have no test of their own."""
    t = ps_tensors(dev)
    x = t["x"].to(torch.bfloat16).to(dev).requires_grad_(True)
    ps = [t[k].to(dev).requires_grad_(True) for k in ("w", "b", "a", "w3", "b3")]
    link = F.Handover()

    def run():
        z = F.ConvAct.apply(x, ps[0], ps[1], ps[2], dict(stride=1, pad=1, act=F.ACT_PRELU, pixel_shuffle=True, out_link=link))
        out = F.ConvOutNCHW.apply(z, ps[3], ps[4], dict(stride=1, pad=4, act=F.ACT_TANH, in_link=link))
        spoil(z, how, (out * t["probe"].to(dev)).sum()).backward()

    names = logged(run)
    return names, [x.grad.clone()] + [p.grad.clone() for p in ps]


def test_ps_handover_raises_when_the_gradient_was_touched(dev, monkeypatch):
    """The tail's launch accepts the shape (asserted) and the plain chain takes it.  A second consumer or a hook on the shuffled
    activation raises.  With DGRAD_PS = False the two-consumer graph runs, and its gradients match a float64 torch restatement
    (bf16 storage against float64: cosine 0.98 as in test_tail_backward_with_the_pixel_shuffle_prelu_backward_inside, 15 % on
    the one-element PReLU gradient)."""
    F = P("functional")
    desc = F.make_desc(torch.empty(1, 16, 16, 64, dtype=torch.bfloat16, device=dev), 3, 9, 9, 1, 4, F.PAD_ZERO, 64)
    import ctypes
    assert P("_lib").lib().dsr_conv_dgrad_ps_supported(ctypes.byref(desc)) == 1
    names, _ = ps_chain(F, dev, None)
    assert names.count("dsr_conv_dgrad_ps") == 1 and names.count("dsr_pw_act_bwd") == 0, names
    for how in SPOILERS:
        with pytest.raises(RuntimeError, match="Handover 'ps'.*second consumer or a hook.*DGRAD_PS"):
            ps_chain(F, dev, how)
    monkeypatch.setattr(F, "DGRAD_PS", False)
    names, got = ps_chain(F, dev, "consumer")
    assert names.count("dsr_conv_dgrad_ps") == 0 and names.count("dsr_pw_act_bwd") == 1, names
    t = {k: v.double() for k, v in ps_tensors(dev).items()}
    leaves = [t[k].requires_grad_(True) for k in ("x", "w", "b", "a", "w3", "b3")]
    z = TF.prelu(TF.pixel_shuffle(TF.conv2d(leaves[0].permute(0, 3, 1, 2), leaves[1], leaves[2], padding=1), 2), leaves[3])
    out = torch.tanh(TF.conv2d(z, leaves[4], leaves[5], padding=4))
    ((out * t["probe"]).sum() + (z.permute(0, 2, 3, 1) * t["probe_z"]).sum()).backward()
    for a, r in zip(got, leaves):
        if r.numel() == 1:
            assert abs(float(a) - float(r.grad)) < 0.15 * abs(float(r.grad)), (float(a), float(r.grad))
        else:
            assert torch.isfinite(a).all() and cos(a.cpu(), r.grad) > 0.98, cos(a.cpu(), r.grad)


# ----------------------------------------------------------------------------- "first2" and the version guards
def first2_chain(F, dev, how, edit_bias=False):
    """The deferred image layer (3 -> 64, LeakyReLU) into ConvBNAct (64 -> 64, stride 2, train) on 16 x 512, N = 2 (a tile of
    the fused backward is 256 gradient pixels of one row); the image needs no gradient."""
    img = torch.zeros(2, 16, 512, 8)
    img[..., :3] = rnd(7, (2, 16, 512, 3))
    img = img.to(torch.bfloat16).to(dev)
    w0, b0 = rnd(60, (64, 3, 3, 3), 0.3).to(dev).requires_grad_(True), rnd(61, (64,), 0.1).to(dev).requires_grad_(True)
    w1, b1 = rnd(62, (64, 64, 3, 3), 0.06).to(dev).requires_grad_(True), rnd(65, (64,), 0.1).to(dev)
    gamma, beta = (1 + rnd(63, (64,), 0.3)).to(dev).requires_grad_(True), rnd(64, (64,), 0.3).to(dev).requires_grad_(True)
    assert F.first2_supported(img, w0, w1, 2)
    link = F.Handover()

    def run():
        z = F.ConvAct.apply(img, w0, b0, None, dict(stride=1, pad=1, act=F.ACT_LEAKY, slope=0.2, defer=True, out_link=link))
        out = F.ConvBNAct.apply(z, w1, b1, gamma, beta, torch.zeros(64, device=dev), torch.ones(64, device=dev),
                                torch.zeros((), dtype=torch.long, device=dev), None, None,
                                dict(stride=2, pad=1, act=F.ACT_LEAKY, slope=0.2, train=True, in_link=link))
        loss = spoil(z, how, (out.float() * rnd(8, tuple(out.shape)).to(dev)).sum())
        if edit_bias:
            with torch.no_grad():
                b0.add_(1.0)
        loss.backward()

    names = logged(run)
    return names, [p.grad.clone() for p in (w0, b0, w1, gamma, beta)]


def test_first2_handover_raises_when_the_gradient_was_touched(dev):
    """The plain chain runs the image layer's backward inside the second layer's input gradient (asserted); a second consumer
    of the deferred activation (or a hook on it) raises: the image layer's gradients went through the link."""
    F = P("functional")
    names, _ = first2_chain(F, dev, None)
    assert names.count("dsr_conv_dgrad_first_bwd") == 1 and not any(n.startswith("dsr_conv_first_bwd") for n in names), names
    for how in SPOILERS:
        with pytest.raises(RuntimeError, match="Handover 'first2'.*second consumer or a hook.*FIRST2_BACKWARD"):
            first2_chain(F, dev, how)


def test_first2_backward_needs_the_bias_it_saw_in_the_forward(dev, monkeypatch):
    """b0 edited in place between forward and backward: the fused backward would rebuild the activation's sign from the new
    bias, so it is not taken -- the separate launches run on the stored activation, bit-identical to FIRST2_BACKWARD = False
    with the same edit."""
    F = P("functional")
    names, got = first2_chain(F, dev, None, edit_bias=True)
    assert "dsr_conv_dgrad_first_bwd" not in names and "dsr_conv_first_bwd_recompute" not in names, names
    assert names.count("dsr_conv_first_bwd") == 1, names
    monkeypatch.setattr(F, "FIRST2_BACKWARD", False)
    names_off, ref = first2_chain(F, dev, None, edit_bias=True)
    assert names_off == names
    assert all(torch.equal(a, b) for a, b in zip(got, ref))


def test_first_layer_recompute_needs_the_bias_it_saw_in_the_forward(dev, monkeypatch):
    """The image layer alone (the shape of test_first_layer_fused_backward, 3 x 37 x 70, LeakyReLU): with the bias edited in
    place between forward and backward the pass reads the stored activation (dsr_conv_first_bwd, not ..._recompute), and dw, db
    are bit-equal to FIRST_BWD_RECOMPUTE = False with the same edit; without the edit the recompute launch is taken."""
    F = P("functional")

    def run(edit):
        img = torch.zeros(3, 37, 70, 8)
        img[..., :3] = rnd(9, (3, 37, 70, 3))
        img = img.to(torch.bfloat16).to(dev)
        w, b = rnd(70, (64, 3, 3, 3), 0.3).to(dev).requires_grad_(True), rnd(71, (64,), 0.1).to(dev).requires_grad_(True)

        def go():
            y = F.ConvAct.apply(img, w, b, None, dict(stride=1, pad=1, act=F.ACT_LEAKY, slope=0.2))
            if edit:
                with torch.no_grad():
                    b.add_(1.0)
            y.backward(rnd(10, tuple(y.shape)).to(torch.bfloat16).to(dev))

        return logged(go), w.grad.clone(), b.grad.clone()

    names, _, _ = run(False)
    assert "dsr_conv_first_bwd_recompute" in names and "dsr_conv_first_bwd" not in names, names
    names, dw, db = run(True)
    assert "dsr_conv_first_bwd" in names and "dsr_conv_first_bwd_recompute" not in names, names
    monkeypatch.setattr(F, "FIRST_BWD_RECOMPUTE", False)
    names_off, dw_off, db_off = run(True)
    assert names_off == names and torch.equal(dw, dw_off) and torch.equal(db, db_off)
