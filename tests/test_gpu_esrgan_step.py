"""GPU: steps.esrgan_step against the float64 restatement of tests/ragan_ref.py, at the shapes of the Real-ESRGAN step tests
(tests/test_gpu_unetd.py): RRDBNet(num_block=1), UNetDiscriminatorSN(num_feat=8), lq 2x3x8x8, gt 2x3x32x32, a two-tap
VggFeatureLoss on stand-in weights.

1. the five losses, the generator's gradients, D's movement and its five power iterations per step;
2. the relativistic coupling: the generator's adversarial gradient depends on the ground truth;
3. eager steps equal HIP-graph replays bit for bit, state dicts (u, v included) and losses; a tensor lr takes effect;
4. ema= is updated once per step."""
import importlib

import pytest
import torch

import parity_util
import ragan_ref as RG
import rrdb_ref as R
import spectral_ref as SR
import unetd_ref as U
from oracle import filler
from test_gpu_spectral_norm import EPS32, forward_bound

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
LW = {"conv1_2": 0.5, "relu2_2": 1.0}
STEP_NF = 8
L1_WEIGHT, GAN_WEIGHT = 1.0, 0.1      # (the recipe's 1e-2 / 5e-3 would leave the adversarial gradient a rounding error of L1's)


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


def _inputs(tag=""):
    lq = filler.tensor("in:resr_lq", (2, 3, 8, 8), 0.5, 0.5)
    gt = filler.tensor("in:resr_gt" + tag, (2, 3, 32, 32), 0.5, 0.5)
    return lq, gt


def _gen_state():
    return filler.fill_state_dict(P("models.GAN.rrdbnet").RRDBNet(num_block=1).state_dict())


def _parts(dev, gsd, dsd, lr=1e-3, feat=True):
    M, O, pc = P("models.GAN.rrdbnet"), P("optim"), P("perceptual")
    gen = M.RRDBNet(num_block=1)
    gen.load_state_dict(gsd)
    gen.to(dev).train()
    disc = P("models.GAN").UNetDiscriminatorSN(num_feat=STEP_NF)
    disc.load_state_dict(dsd, strict=True)
    disc.to(dev).train()
    disc.compute_dtype = torch.bfloat16
    vgg = pc.VggFeatureLoss(LW, "l1").to(dev) if feat else None
    opt_g = O.FusedAdam(gen.parameters(), lr=torch.tensor(lr))
    opt_d = O.FusedAdam(disc.parameters(), lr=torch.tensor(lr))
    return gen, disc, vgg, opt_g, opt_d


@pytest.fixture(scope="module")
def reference():
    """The float64 restatement and its bf16 storage-model run: computed once, read only."""
    G = P("utils.GAN")
    lq, gt = _inputs()
    gsd, dsd, vsd = _gen_state(), _disc_state(STEP_NF, salt=1), G._standin_vgg_state()
    ref = RG.step_reference(gsd, dsd, vsd, lq, gt, None, LW, L1_WEIGHT, GAN_WEIGHT)
    sim = RG.step_reference(gsd, dsd, vsd, lq, gt, R.BF16, LW, L1_WEIGHT, GAN_WEIGHT)
    return gsd, dsd, ref, sim


def test_esrgan_step_against_the_restatement(dev, reference):
    """One step.  Losses: |hip - f64| <= 2 |sim - f64| + 1e-3 |f64| (sim: the storage-model restatement).  The generator's
    gradients: parity_util.compare_grads.  D stays trainable and moves.  D's u after the step = FIVE reference iterations on the
    weights the step started from, within the first-order propagation of test_float_data's per-iteration bound that the
    Real-ESRGAN step test uses for three: e_i <= a_i e_(i-1) + |du_i|_2, a_i = |W|_2^2 / (|W^T u_(i-1)| |W v_i|)."""
    S = P("steps")
    lq, gt = _inputs()
    gsd, dsd, (ref_l, ref_g, ref_d), (sim_l, sim_g, _) = reference
    gen, disc, feat, opt_g, opt_d = _parts(dev, gsd, dsd)
    before_d = {k: v.detach().clone() for k, v in disc.named_parameters()}
    out = S.esrgan_step(gen, disc, feat, opt_g, opt_d, lq.to(dev), gt.to(dev), l1_weight=L1_WEIGHT, gan_weight=GAN_WEIGHT)
    torch.cuda.synchronize()
    assert len(out) == 6 and all(not t.requires_grad and t.is_cuda for t in out) and tuple(out[5].shape) == (2, 3, 32, 32)
    assert all(t.dim() == 0 and t.dtype == torch.float32 for t in out[:5])
    for name, h, r, s in zip(("l_pix", "l_percep", "l_g_gan", "l_d_real", "l_d_fake"), out, ref_l, sim_l):
        print(f"esrgan_step {name}: hip {float(h):.6g} f64 {r:.6g} sim {s:.6g}")
        assert abs(float(h) - r) <= 2 * abs(s - r) + 1e-3 * abs(r), (name, float(h), r, s)
    hip_g = {k: p.grad for k, p in gen.named_parameters()}
    assert all(g is not None for g in hip_g.values())
    bad, table = parity_util.compare_grads(hip_g, ref_g, sim_g)
    worst = sorted(table.items(), key=lambda kv: kv[1][0])[:5]
    print("esrgan_step generator gradients, lowest cosines:", worst)
    assert len(table) == len(ref_g) and not bad, bad
    assert all(p.requires_grad for p in disc.parameters())
    assert all(not torch.equal(p, before_d[k]) for k, p in disc.named_parameters())
    for name in U.SN:
        W, u, v = dsd[name + ".weight_orig"], dsd[name + ".weight_u"].double(), dsd[name + ".weight_v"].double()
        smax = float(torch.linalg.matrix_norm(SR.mat(W), 2))
        e = 0.0
        for _ in range(5):
            du, _, _, _ = forward_bound(W, u)
            t = SR.mat(W).t() @ u
            u, v, _, _ = SR.iterate(W, u, v)
            e = smax ** 2 / (float(t.norm()) * float((SR.mat(W) @ v).norm())) * e + float(du.norm())
        assert float((u - ref_d[name + ".weight_u"]).abs().max()) == 0.0      # the restatement ran five forwards of D too
        got = getattr(disc, name).weight_u.double().cpu()
        err = float((got - u).norm())
        print(f"esrgan_step {name}.weight_u after five iterations: |hip - f64|_2 {err:.3e}, bound {e + EPS32:.3e}")
        assert err <= e + EPS32, (name, err, e)


def test_without_a_content_term(dev):
    """vggfeat=None: l_percep is a zero scalar on the device, everything else runs."""
    S = P("steps")
    lq, gt = _inputs()
    gen, disc, _, opt_g, opt_d = _parts(dev, _gen_state(), _disc_state(STEP_NF, salt=1), feat=False)
    out = S.esrgan_step(gen, disc, None, opt_g, opt_d, lq.to(dev), gt.to(dev))
    assert out[1].is_cuda and out[1].dim() == 0 and float(out[1]) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in out)


def test_the_relativistic_coupling_reaches_the_generator(dev):
    """l1_weight = 0 and no content term: what is left of the generator's gradient is adversarial.  Under the relativistic
    average form it depends on D(gt) through the batch mean, so another ground truth gives another gradient for every
    generator parameter (with realesrgan_step's constant label the two would be equal); and it scales with gan_weight."""
    S = P("steps")
    gsd, dsd = _gen_state(), _disc_state(STEP_NF, salt=1)
    lq, gt_a = _inputs()
    _, gt_b = _inputs("_other")
    assert not torch.equal(gt_a, gt_b)
    grads = []
    for gt, gw in ((gt_a, 0.1), (gt_b, 0.1), (gt_a, 0.2)):
        gen, disc, _, opt_g, opt_d = _parts(dev, gsd, dsd, feat=False)
        S.esrgan_step(gen, disc, None, opt_g, opt_d, lq.to(dev), gt.to(dev), l1_weight=0.0, gan_weight=gw)
        grads.append({k: p.grad.clone() for k, p in gen.named_parameters()})
    first, other_gt, doubled = grads
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in first.values())
    same = [k for k in first if torch.equal(first[k], other_gt[k])]
    assert not same, same
    same = [k for k in first if torch.equal(first[k], doubled[k])]
    assert not same, same


def test_esrgan_step_graphed_equals_eager(dev):
    """One eager step, then two more: eager against two replays of a HIP graph captured after the same first step (GraphedStep's
    warm-up): losses and every entry of G's and D's state_dict (u and v included) bit for bit; opt.lr.fill_() between the
    replays takes effect."""
    S = P("steps")
    lq, gt = _inputs()
    lq, gt = lq.to(dev), gt.to(dev)
    gsd, dsd = _gen_state(), _disc_state(STEP_NF, salt=1)

    def make():
        gen, disc, feat, opt_g, opt_d = _parts(dev, gsd, dsd)
        return gen, disc, opt_g, opt_d, (lambda: S.esrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt, l1_weight=L1_WEIGHT,
                                                               gan_weight=GAN_WEIGHT))

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
            sd_e, sd_g = me.state_dict(), mg.state_dict()
            assert list(sd_e) == list(sd_g)
            for k in sd_e:
                assert torch.equal(sd_e[k], sd_g[k]), (i, k)
        assert any(k.endswith("weight_u") for k in disc_e.state_dict())
        if i == 0:
            mid = {k: v.clone() for k, v in gen_e.state_dict().items()}
            step_small = {k: (v - gsd[k].to(dev)).abs().max() for k, v in mid.items()}
    # the larger lr of the second replay shows: Adam's first steps move every weight by about lr
    moved = max(float((v - mid[k]).abs().max()) for k, v in gen_g.state_dict().items())
    assert moved > 2.5e-3, moved
    assert max(float(v) for v in step_small.values()) < 2.5e-3


def test_ema_is_updated_once_per_step(dev):
    S, O = P("steps"), P("optim")
    lq, gt = _inputs()
    gen, disc, feat, opt_g, opt_d = _parts(dev, _gen_state(), _disc_state(STEP_NF, salt=1))
    ema = O.WeightEMA(gen, decay=0.5)
    for want in (1, 2):
        S.esrgan_step(gen, disc, feat, opt_g, opt_d, lq.to(dev), gt.to(dev), ema=ema)
        assert int(ema.n_averaged.item()) == want
