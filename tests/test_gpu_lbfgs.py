"""GPU: optim.FusedLBFGS (csrc/lbfgs.hip) against torch.optim.LBFGS.

The floor is torch.optim.LBFGS itself: the same closure (a torch fp32 function on the device) run by torch.optim.LBFGS in fp32
on the device, and in float64 on the CPU.  Bar: ||x_fused - x_f64|| / ||x_f64|| <= 2 x (that of torch's fp32 run), closure
calls equal to torch's, the returned loss the first closure value bit for bit.  The fused form accumulates its dots in fp64,
so it should be no worse than torch's fp32 recursion; any slack beyond 2x would hide a recursion error.  Each test prints
its measured ratio (tools/microbench_lbfgs.py records them in profiles/microbench_lbfgs.txt)."""
import importlib

import numpy as np
import pytest
import torch

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


def quadratic(n=5000, seed=0):
    rng = np.random.default_rng(seed)
    ev, b = np.logspace(0, 3, n), rng.standard_normal(n)
    x0 = rng.standard_normal(n)

    def make(device, dtype):
        e, bb = torch.tensor(ev, dtype=dtype, device=device), torch.tensor(b, dtype=dtype, device=device)
        return lambda x: 0.5 * (e * x * x).sum() - (bb * x).sum()
    return make, x0


def rosenbrock(n=1000):
    x0 = np.tile([-1.2, 1.0], n // 2)

    def make(device, dtype):
        def f(x):
            a, b = x[0::2], x[1::2]
            return (100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2).sum()
        return f
    return make, x0


def tiny_quadratic():
    ev, b, x0 = np.array([1.0, 10 ** 0.5, 10.0]), np.array([1.0, -2.0, 0.5]), np.array([0.3, -0.7, 1.1])

    def make(device, dtype):
        e, bb = torch.tensor(ev, dtype=dtype, device=device), torch.tensor(b, dtype=dtype, device=device)
        return lambda x: 0.5 * (e * x * x).sum() - (bb * x).sum()
    return make, x0


def linear(n=300):
    rng = np.random.default_rng(1)
    c, x0 = rng.standard_normal(n), rng.standard_normal(n)

    def make(device, dtype):
        cc = torch.tensor(c, dtype=dtype, device=device)
        return lambda x: (cc * x).sum()
    return make, x0


def run(opt_cls, problem, splits, device, dtype, steps=1, unused=0, **kw):
    """Parameters = x0 split into tensors of `splits` sizes (+ one tensor of `unused` elements the loss never touches, so
    its gradient stays None).  Returns (flat x, closure calls, step() return values, optimizer)."""
    make, x0 = problem
    f = make(device, dtype)
    params, o = [], 0
    for s in splits:
        params.append(torch.tensor(x0[o:o + s], dtype=dtype, device=device).requires_grad_(True))
        o += s
    extra = [torch.full((unused,), 0.5, dtype=dtype, device=device, requires_grad=True)] if unused else []
    opt = opt_cls(params[:1] + extra + params[1:], **kw)
    calls = [0]

    def closure():
        opt.zero_grad()
        calls[0] += 1
        loss = f(torch.cat(params))
        loss.backward()
        return loss

    rets = [opt.step(closure) for _ in range(steps)]
    x = torch.cat([p.detach() for p in params] + [e.detach() for e in extra]).double().cpu().numpy()
    return x, calls[0], rets, opt


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def compare(problem, splits, dev, steps=1, unused=0, **kw):
    F = P("optim").FusedLBFGS
    x64, c64, _, _ = run(torch.optim.LBFGS, problem, splits, "cpu", torch.float64, steps, unused, **kw)
    x32, c32, _, _ = run(torch.optim.LBFGS, problem, splits, dev, torch.float32, steps, unused, **kw)
    xf, cf, rets, opt = run(F, problem, splits, dev, torch.float32, steps, unused, **kw)
    floor, err = rel(x32, x64), rel(xf, x64)
    print(f"\n{kw} steps={steps}: calls fused {cf} torch fp32 {c32} fp64 {c64}; rel err fused {err:.3e} torch fp32 floor "
          f"{floor:.3e} ratio {err / floor:.3f}")
    return dict(x64=x64, x32=x32, xf=xf, c64=c64, c32=c32, cf=cf, floor=floor, err=err, rets=rets, opt=opt)


@pytest.mark.parametrize("history", [100, 5, 40])
def test_fused_lbfgs_quadratic_vs_torch(dev, history):
    """f = 1/2 sum ev x^2 - b x, ev logspaced over [1, 1e3], n = 5000 in tensors of 7, 1000, 3993 + one whose gradient stays
    None; lr 1, 30 iterations, tolerances off; x0 and b drawn N(0, 1).  History 40 runs 80 iterations instead: the live list
    passes 64 entries (L = 2k + 1 > 64 from k = 32) and the ring wraps at m = 40.  Measured on an MI355X: history 100 fused
    1.496e-4 against torch's fp32 floor 1.500e-4 (ratio 0.998), history 5 3.008e-4 against 3.022e-4 (0.995), history 40
    2.475e-3 against 9.122e-3 (0.271)."""
    r = compare(quadratic(), [7, 1000, 3993], dev, unused=3, lr=1, max_iter=80 if history == 40 else 30,
                history_size=history, tolerance_grad=-1, tolerance_change=-1)
    assert r["cf"] == r["c32"] == r["c64"]
    assert r["err"] <= 2 * r["floor"]


def test_fused_lbfgs_table_crosses_64_tensors(dev):
    """The quadratic of the test above at history 5, n = 5000 in 70 tensors + one whose gradient stays None: 68 ragged small
    ones (1 + 7 i mod 13 elements), one of 4097 (one element past a gather chunk of 4096, four combine chunks of 1024 and one
    element) and the remaining 437 -- gather and combine take 64 tensors per launch, so each is two launches, the second
    with a running block base and a tensor of several blocks.  Same bar as above.  Measured on an MI355X: fused 3.008e-4
    against torch's fp32 floor 3.028e-4 (ratio 0.994)."""
    small = [1 + (7 * i) % 13 for i in range(68)]
    splits = small + [4097, 5000 - 4097 - sum(small)]
    assert len(splits) == 70 and splits[-1] > 0
    r = compare(quadratic(), splits, dev, unused=3, lr=1, max_iter=30, history_size=5, tolerance_grad=-1, tolerance_change=-1)
    assert r["cf"] == r["c32"] == r["c64"]
    assert r["err"] <= 2 * r["floor"]


def test_fused_lbfgs_rosenbrock_vs_torch(dev):
    """Extended Rosenbrock, 1000 elements split 1 / 499 / 500, lr 0.1, 30 iterations from (-1.2, 1, ...).  Measured on an
    MI355X: fused 3.418e-6 against torch's fp32 floor 3.241e-6 (ratio 1.054)."""
    r = compare(rosenbrock(), [1, 499, 500], dev, lr=0.1, max_iter=30, tolerance_grad=-1, tolerance_change=-1)
    assert r["cf"] == r["c32"] == r["c64"]
    assert r["err"] <= 2 * r["floor"]


def test_fused_lbfgs_returns_the_first_closure_value(dev):
    F = P("optim").FusedLBFGS
    make, x0 = quadratic()
    f = make(dev, torch.float32)
    x = torch.tensor(x0, dtype=torch.float32, device=dev).requires_grad_(True)
    opt = F([x], max_iter=4)
    seen = []

    def closure():
        opt.zero_grad()
        loss = f(x)
        loss.backward()
        seen.append(loss)
        return loss

    ret = opt.step(closure)
    assert ret is seen[0]
    assert torch.equal(ret, seen[0]) and len(seen) == 4


@pytest.mark.parametrize("case", ["grad", "change", "max_eval", "linear"])
def test_fused_lbfgs_stops_where_torch_stops(dev, case):
    """3-element quadratic (cond 10, split 1 / 2, max_iter 50): tolerance_grad 1e-5 alone, tolerance_change 1e-9 alone, max_eval
    7 < max_iter 20; and a linear function on which every pair is skipped (y = 0)."""
    kws = {"grad": dict(tolerance_grad=1e-5, tolerance_change=-1), "change": dict(tolerance_grad=-1, tolerance_change=1e-9),
           "max_eval": dict(max_iter=20, max_eval=7, tolerance_grad=-1, tolerance_change=-1),
           "linear": dict(max_iter=12, tolerance_grad=-1, tolerance_change=-1)}
    kw = dict(dict(lr=1, max_iter=50), **kws[case])
    problem, splits = (linear(), [100, 200]) if case == "linear" else (tiny_quadratic(), [1, 2])
    r = compare(problem, splits, dev, **kw)
    assert r["cf"] == r["c32"]
    assert r["cf"] < 50
    # a run that converges can end within rounding of the optimum, where torch's own fp32 error may be ~0: one fp32
    # epsilon is the least a float32 result can be asked for
    assert r["err"] <= 2 * max(r["floor"], 2.0 ** -23)
    if case == "linear":
        assert r["opt"].state_counts()["history"] == 0


def test_fused_lbfgs_state_persists_across_steps(dev):
    """Two step() calls of max_iter 5 against torch's two calls (each torch step() starts with a closure call, so this is
    not one call of 10: it checks what step() carries over)."""
    r = compare(quadratic(seed=3), [7, 1000, 3993], dev, steps=2, lr=1, max_iter=5, history_size=100,
                tolerance_grad=-1, tolerance_change=-1)
    assert r["cf"] == r["c32"] == r["c64"] == 10
    assert r["err"] <= 2 * r["floor"]
    st = r["opt"].state_counts()
    assert st["n_iter"] == 10 and st["func_evals"] == 10


def test_fused_lbfgs_is_deterministic(dev):
    F = P("optim").FusedLBFGS
    a, _, _, _ = run(F, quadratic(), [7, 1000, 3993], dev, torch.float32, lr=1, max_iter=30, history_size=10,
                     tolerance_grad=-1, tolerance_change=-1)
    b, _, _, _ = run(F, quadratic(), [7, 1000, 3993], dev, torch.float32, lr=1, max_iter=30, history_size=10,
                     tolerance_grad=-1, tolerance_change=-1)
    assert np.array_equal(a, b)


def test_fused_lbfgs_launches_do_not_grow_with_history(dev):
    L = P("_lib")
    per_call = {}
    for h in (5, 50):
        L.LAUNCH_LOG = []
        try:
            _, calls, _, _ = run(P("optim").FusedLBFGS, quadratic(), [7, 1000, 3993], dev, torch.float32, lr=1, max_iter=20,
                                 history_size=h, tolerance_grad=-1, tolerance_change=-1)
            torch.cuda.synchronize()
            per_call[h] = len(L.LAUNCH_LOG) / calls
        finally:
            L.LAUNCH_LOG = None
    assert per_call[5] == per_call[50] == 4, per_call


def _small_dip(dev):
    M = P("models.DIP")
    torch.manual_seed(0)
    net = M.get_net(8, "skip", "reflection", upsample_mode="bilinear", skip_n33d=16, skip_n33u=16, skip_n11=4, num_scales=3)
    net.to(dev).train()
    for m in net.modules():
        if hasattr(m, "compute_dtype"):
            m.compute_dtype = torch.bfloat16
    return net


def test_fused_lbfgs_keeps_packed_weights_current(dev):
    """After FusedLBFGS updates a DIP net through raw pointers, its forward equals bit for bit that of a fresh net loaded with
    the updated state_dict (fails if bump() or the repack is missing: the old 16-bit weight images would be used)."""
    F = P("functional")
    net = _small_dip(dev)
    g = torch.Generator().manual_seed(5)
    z = (0.1 * torch.rand(1, 8, 32, 32, generator=g)).to(dev)
    target = torch.rand(1, 3, 32, 32, generator=g).to(dev)
    opt = P("optim").FusedLBFGS(list(net.parameters()), lr=0.01, max_iter=4, tolerance_grad=-1, tolerance_change=-1)

    def closure():
        opt.zero_grad()
        loss = F.mse_loss(net(z), target)
        loss.backward()
        return loss

    opt.step(closure)
    with torch.no_grad():
        got = net(z)
        fresh = _small_dip(dev)
        fresh.load_state_dict(net.state_dict())
        want = fresh(z)
    assert torch.equal(got, want)


def test_optimize_fused_lbfgs_over_hip_closure(dev):
    """utils.DIP.optimize('LBFGS', ..., fused_lbfgs=True) over the HIP DIP closure of
    test_gpu_surface.py::test_optimize_lbfgs_over_hip_closure, next to the default path: the same closure count, LBFGS keeps
    descending, and the window means of the LBFGS phase agree within the 35 % that test uses (chaotic amplification of
    rounding over 100 Adam steps on a 3-scale net at batch 1, test_gpu_surface.py:246-251)."""
    from oracle import dip, downsampler, filler, gan
    M, Dn, U, F = P("models.DIP"), P("utils.downsampler"), P("utils.DIP"), P("functional")
    kw = dict(skip_n33d=16, skip_n33u=16, skip_n11=4, num_scales=3)
    cfg = dip.SkipConfig(input_depth=8, **kw)
    sd = filler.fill_state_dict(gan.template(dip.skip_shapes(cfg)))
    hr = filler.tensor("in:lb_hr", (1, 3, 32, 32), 0.5, 0.5)
    lr_img = downsampler.downsampler_forward(hr, 2, "lanczos2", phase=0.5, preserve_size=True)
    zin = filler.tensor("in:lb_z", (1, 8, 32, 32), 0.05, 0.05)
    num_iter = 12

    def fit(fused):
        net = M.get_net(8, "skip", "reflection", upsample_mode="bilinear", **kw)
        net.load_state_dict(sd)
        net.to(dev).train()
        for m in net.modules():
            if hasattr(m, "compute_dtype"):
                m.compute_dtype = torch.bfloat16
        down = Dn.Downsampler(3, 2, "lanczos2", phase=0.5, preserve_size=True).to(dev)
        zd, lrd = zin.to(dev), lr_img.to(dev)
        hist = []

        def closure():
            loss = F.mse_loss(down(net(zd)), lrd)
            loss.backward()
            hist.append(loss.detach())
            return loss

        U.optimize("LBFGS", U.get_params("net", net, zd), closure, 0.01, num_iter, fused_lbfgs=fused)
        torch.cuda.synchronize()
        return [float(v) for v in hist]

    base, fused = fit(False), fit(True)
    print(f"\nclosure calls {len(base)} / {len(fused)}; loss[99] {base[99]:.5g} / {fused[99]:.5g}; last {base[-1]:.5g} / "
          f"{fused[-1]:.5g}")
    assert len(fused) == len(base) >= 100 + num_iter
    assert fused[-1] < fused[99] * 1.001

    def window(v, lo, hi):
        return sum(v[lo:hi]) / (hi - lo)

    h, b = window(fused, 100, len(fused)), window(base, 100, len(base))
    assert abs(h - b) < 0.35 * b, (h, b)


def test_fused_lbfgs_rejects_bad_arguments_on_the_device(dev):
    O = P("optim")
    x = torch.zeros(8, device=dev, requires_grad=True)
    with pytest.raises(ValueError):
        O.FusedLBFGS([x], history_size=0)
    with pytest.raises(ValueError):
        O.FusedLBFGS([x], history_size=-4)
    with pytest.raises(NotImplementedError, match="strong_wolfe"):
        O.FusedLBFGS([x], line_search_fn="strong_wolfe")
    with pytest.raises(TypeError):
        O.FusedLBFGS([torch.zeros(8, device=dev, dtype=torch.float16)])
    with pytest.raises(TypeError):
        O.FusedLBFGS([torch.zeros(4, 4, device=dev).t()])
    with pytest.raises(TypeError):
        O.FusedLBFGS([torch.zeros(8, device=dev).to_sparse()])
    L = P("_lib")
    lib = L.lib()
    assert lib.dsr_lbfgs_scalar(None, 0, 5, 8, 1, None, 1, None, 1.0, 20, 25, 1e-7, 1e-9, None) == -1
    assert lib.dsr_lbfgs_dots(None, 0, None, 0, 8, 1, None) == -1
