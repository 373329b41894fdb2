"""GPU: steps.realesrgan_step with the LDL artifact term (ldl_weight, gen_ema, ldl_detach) against the float64 restatement of
tests/ldl_ref.py, at the shapes of tests/test_gpu_esrgan_step.py: RRDBNet(num_block=1), UNetDiscriminatorSN(num_feat=8),
lq 2x3x8x8, gt 2x3x32x32, a two-tap VggFeatureLoss on stand-in weights.

1. ldl_weight=0: outputs and the generator's weights after two steps are bit-equal to a call without the keywords;
2. ldl_weight=1: the seven values and the generator's gradients against the restatement, within the bounds of that file;
3. gen_ema holds the EMA's average after the step and held the previous one during it;
4. eager steps equal HIP-graph replays bit for bit;
5. a missing gen_ema raises."""
import importlib

import pytest
import torch

import ldl_ref as LR
import parity_util
import rrdb_ref as R
import unetd_ref as U
from oracle import filler

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
LW = {"conv1_2": 0.5, "relu2_2": 1.0}
STEP_NF = 8
L1_WEIGHT, GAN_WEIGHT, LDL_WEIGHT = 1.0, 0.1, 1.0


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _disc_state(num_feat, salt=0):
    """The closed-form discriminator state of tests/test_gpu_unetd.py: unit-gain weights, small biases, normalised u and v."""
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


def _inputs():
    lq = filler.tensor("in:resr_lq", (2, 3, 8, 8), 0.5, 0.5)
    gt = filler.tensor("in:resr_gt", (2, 3, 32, 32), 0.5, 0.5)
    return lq, gt


def _gen_state(salt=0):
    return filler.fill_state_dict(P("models.GAN.rrdbnet").RRDBNet(num_block=1).state_dict(), salt=salt)


def _generator(dev, sd, train=True):
    gen = P("models.GAN.rrdbnet").RRDBNet(num_block=1)
    gen.load_state_dict(sd)
    gen.to(dev)
    return gen.train() if train else gen.eval()


def _parts(dev, gsd, dsd, lr=1e-3):
    O, pc = P("optim"), P("perceptual")
    gen = _generator(dev, gsd)
    disc = P("models.GAN").UNetDiscriminatorSN(num_feat=STEP_NF)
    disc.load_state_dict(dsd, strict=True)
    disc.to(dev).train()
    disc.compute_dtype = torch.bfloat16
    vgg = pc.VggFeatureLoss(LW, "l1").to(dev)
    opt_g = O.FusedAdam(gen.parameters(), lr=torch.tensor(lr))
    opt_d = O.FusedAdam(disc.parameters(), lr=torch.tensor(lr))
    return gen, disc, vgg, opt_g, opt_d


def test_ldl_weight_zero_changes_no_bit(dev):
    """Two steps with ldl_weight=0 (a gen_ema given, and ignored) against two steps without the keywords: the six outputs and
    every generator weight bit for bit; gen_ema is left alone."""
    S = P("steps")
    lq, gt = _inputs()
    lq, gt = lq.to(dev), gt.to(dev)
    gsd, dsd, esd = _gen_state(), _disc_state(STEP_NF, salt=1), _gen_state(salt=3)
    runs = []
    for kw in (False, True):
        gen, disc, feat, opt_g, opt_d = _parts(dev, gsd, dsd)
        gen_ema = _generator(dev, esd, train=False)
        extra = dict(ldl_weight=0.0, gen_ema=gen_ema, ldl_detach=True) if kw else {}
        outs = []
        for _ in range(2):
            out = S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt, gan_weight=GAN_WEIGHT, **extra)
            assert len(out) == 6
            outs += [t.clone() for t in out]
        runs.append((outs, {k: v.clone() for k, v in gen.state_dict().items()}))
        for k, v in gen_ema.state_dict().items():
            assert torch.equal(v.cpu(), esd[k]), k
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k


@pytest.mark.parametrize("detach", [False, True], ids=["through-the-map", "detached"])
def test_step_with_the_term_against_the_restatement(dev, detach):
    """One step with ldl_weight = 1.  Losses: |hip - f64| <= 2 |sim - f64| + 1e-3 |f64| (sim: the bf16 storage-model
    restatement); the generator's gradients: parity_util.compare_grads -- the bounds of tests/test_gpu_esrgan_step.py.  The
    term takes the L1 term's target and the EMA generator's output as it stood before the step; the gradients differ from a step
    without the term in every parameter."""
    S, G = P("steps"), P("utils.GAN")
    lq, gt = _inputs()
    gsd, dsd, esd, vsd = _gen_state(), _disc_state(STEP_NF, salt=1), _gen_state(salt=3), G._standin_vgg_state()
    ref_l, ref_g, _ = LR.step_reference(gsd, esd, dsd, vsd, lq, gt, None, LW, L1_WEIGHT, GAN_WEIGHT, LDL_WEIGHT, 7, detach)
    sim_l, sim_g, _ = LR.step_reference(gsd, esd, dsd, vsd, lq, gt, R.BF16, LW, L1_WEIGHT, GAN_WEIGHT, LDL_WEIGHT, 7, detach)
    gen, disc, feat, opt_g, opt_d = _parts(dev, gsd, dsd)
    gen_ema = _generator(dev, esd, train=False)
    out = S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq.to(dev), gt.to(dev), l1_weight=L1_WEIGHT, gan_weight=GAN_WEIGHT,
                            ldl_weight=LDL_WEIGHT, gen_ema=gen_ema, ldl_detach=detach)
    torch.cuda.synchronize()
    assert len(out) == 7 and all(not t.requires_grad and t.is_cuda for t in out) and tuple(out[5].shape) == (2, 3, 32, 32)
    vals = list(out[:5]) + [out[6]]
    assert all(t.dim() == 0 and t.dtype == torch.float32 for t in vals)
    for name, h, r, s in zip(("l_pix", "l_percep", "l_g_gan", "l_d_real", "l_d_fake", "l_g_ldl"), vals, ref_l, sim_l):
        print(f"realesrgan_step+ldl detach={detach} {name}: hip {float(h):.6g} f64 {r:.6g} sim {s:.6g}")
        assert abs(float(h) - r) <= 2 * abs(s - r) + 1e-3 * abs(r), (name, float(h), r, s)
    assert ref_l[5] > 0
    hip_g = {k: p.grad for k, p in gen.named_parameters()}
    assert all(g is not None for g in hip_g.values())
    bad, table = parity_util.compare_grads(hip_g, ref_g, sim_g)
    worst = sorted(table.items(), key=lambda kv: kv[1][0])[:5]
    print("realesrgan_step+ldl generator gradients, lowest cosines:", worst)
    assert len(table) == len(ref_g) and not bad, bad
    # without an EMA object nothing is written into gen_ema
    for k, v in gen_ema.state_dict().items():
        assert torch.equal(v.cpu(), esd[k]), k
    # the term arrives in the gradients
    gen2, disc2, feat2, og2, od2 = _parts(dev, gsd, dsd)
    S.realesrgan_step(gen2, disc2, feat2, og2, od2, lq.to(dev), gt.to(dev), l1_weight=L1_WEIGHT, gan_weight=GAN_WEIGHT)
    changed = [k for k, p in gen2.named_parameters() if not torch.equal(p.grad, hip_g[k])]
    assert len(changed) == len(hip_g), set(hip_g) - set(changed)


def test_gen_ema_follows_the_average_one_step_behind(dev):
    """After a step gen_ema holds ema's average bit for bit; during the step the term read the average of the step before:
    l_g_ldl of step 2 is ldl_loss(fake, gt, gen_ema(lq)) with gen_ema as it stood between the steps."""
    S, O, F = P("steps"), P("optim"), P("functional")
    lq, gt = _inputs()
    lq, gt = lq.to(dev), gt.to(dev)
    gsd, dsd = _gen_state(), _disc_state(STEP_NF, salt=1)
    gen, disc, feat, opt_g, opt_d = _parts(dev, gsd, dsd, lr=1e-2)
    gen_ema = _generator(dev, _gen_state(salt=3), train=False)
    ema = O.WeightEMA(gen, decay=0.5)
    step = lambda: S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt, gan_weight=GAN_WEIGHT, ema=ema, ldl_weight=LDL_WEIGHT,
                                     gen_ema=gen_ema)
    with torch.no_grad():
        before = gen_ema(lq).clone()
    out = step()
    assert int(ema.n_averaged.item()) == 1
    assert torch.equal(out[6], F.ldl_loss(out[5], gt, before))
    avg = ema.module_state_dict()
    for k, v in gen_ema.state_dict().items():
        assert torch.equal(v, avg[k]), k
    with torch.no_grad():
        between = gen_ema(lq).clone()
    assert not torch.equal(between, before)
    out = step()
    assert int(ema.n_averaged.item()) == 2
    assert torch.equal(out[6], F.ldl_loss(out[5], gt, between))
    avg2 = ema.module_state_dict()
    assert any(not torch.equal(avg2[k], avg[k]) for k in avg)
    for k, v in gen_ema.state_dict().items():
        assert torch.equal(v, avg2[k]), k
    with torch.no_grad():
        assert not torch.equal(gen_ema(lq), between)            # the packed weight images followed the copy


def test_step_with_the_term_graphed_equals_eager(dev):
    """One eager step, then two more: eager against two replays of a HIP graph captured after the same first step: the seven
    outputs and every entry of G's, gen_ema's and D's state_dict bit for bit.  Each variant has modules, optimisers and EMA of
    its own."""
    S, O = P("steps"), P("optim")
    lq, gt = _inputs()
    lq, gt = lq.to(dev), gt.to(dev)
    gsd, dsd, esd = _gen_state(), _disc_state(STEP_NF, salt=1), _gen_state(salt=3)

    def make():
        gen, disc, feat, opt_g, opt_d = _parts(dev, gsd, dsd)
        gen_ema = _generator(dev, esd, train=False)
        ema = O.WeightEMA(gen, decay=0.5)
        return gen, gen_ema, disc, (lambda: S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt, gan_weight=GAN_WEIGHT, ema=ema,
                                                              ldl_weight=LDL_WEIGHT, gen_ema=gen_ema))

    gen_e, ema_e, disc_e, step_e = make()
    gen_g, ema_g, disc_g, step_g = make()
    step_e()
    graphed = S.GraphedStep(step_g, warmup=1)
    for i in range(2):
        out_e = [t.clone() for t in step_e()]
        out_g = graphed()
        torch.cuda.synchronize()
        assert len(out_e) == 7 and len(out_g) == 7
        for a, b in zip(out_e, out_g):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        for me, mg in ((gen_e, gen_g), (ema_e, ema_g), (disc_e, disc_g)):
            sd_e, sd_g = me.state_dict(), mg.state_dict()
            assert list(sd_e) == list(sd_g)
            for k in sd_e:
                assert torch.equal(sd_e[k], sd_g[k]), (i, k)
    assert any(not torch.equal(v, esd[k].to(dev)) for k, v in ema_g.state_dict().items())


def test_a_missing_gen_ema_raises(dev):
    S = P("steps")
    lq, gt = _inputs()
    gen, disc, feat, opt_g, opt_d = _parts(dev, _gen_state(), _disc_state(STEP_NF, salt=1))
    before = {k: v.clone() for k, v in gen.state_dict().items()}
    with pytest.raises(ValueError, match="gen_ema"):
        S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq.to(dev), gt.to(dev), ldl_weight=1.0)
    for k, v in gen.state_dict().items():
        assert torch.equal(v, before[k]), k
