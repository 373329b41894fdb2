"""CPU: the vector-free L-BFGS recursion of csrc/lbfgs.hip (its float64 model, tests/lbfgs_ref.py) against torch.optim.LBFGS in
float64, the C-ABI symbols of the fused optimizer, its argument checks, and the Python surface that needs no device.

Bound of the model comparison: 1e-10 relative.  torch's fp32 floor on the quadratic (1.8e-6) is about 30 fp32 epsilons; the
same amplification of the fp64 epsilon gives about 1e-14, so 1e-10 leaves four orders of magnitude and still catches any
recursion error (a wrong coefficient moves the result by the size of a step)."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import lbfgs_ref

PKG = "deep-super-resolution_amd"
REL = 1e-10


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def so():
    return P("_build").build()


def quadratic(n=5000, seed=0):
    rng = np.random.default_rng(seed)
    ev = torch.tensor(np.logspace(0, 3, n))
    b = torch.tensor(rng.standard_normal(n))
    return (lambda x: 0.5 * (ev * x * x).sum() - (b * x).sum()), torch.tensor(rng.standard_normal(n))


def linear(n=300, seed=1):
    rng = np.random.default_rng(seed)
    c = torch.tensor(rng.standard_normal(n))
    return (lambda x: (c * x).sum()), torch.tensor(rng.standard_normal(n))


def torch_run(f, x0, steps=1, **kw):
    x = x0.clone().requires_grad_(True)
    opt = torch.optim.LBFGS([x], **kw)
    calls = [0]

    def closure():
        opt.zero_grad()
        calls[0] += 1
        loss = f(x)
        loss.backward()
        return loss

    firsts = [float(opt.step(closure).detach()) for _ in range(steps)]
    return x.detach().numpy(), calls[0], firsts


def model_run(f, x0, steps=1, **kw):
    x = x0.numpy().copy()
    opt = lbfgs_ref.GramLBFGS(len(x), **kw)

    def closure(xv):
        t = torch.tensor(xv, requires_grad=True)
        loss = f(t)
        loss.backward()
        return float(loss), t.grad.numpy()

    calls, firsts = 0, []
    for _ in range(steps):
        first, c = opt.step(x, closure)
        calls += c
        firsts.append(first)
    return x, calls, firsts


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("history", [100, 5])
def test_gram_recursion_matches_torch_lbfgs_quadratic(history):
    """30 iterations, tolerances off; history 5 wraps the ring six times."""
    f, x0 = quadratic()
    kw = dict(lr=1, max_iter=30, tolerance_grad=-1, tolerance_change=-1, history_size=history)
    xt, ct, ft = torch_run(f, x0, **kw)
    xm, cm, fm = model_run(f, x0, **kw)
    err = rel(xm, xt)
    print(f"history {history}: relative difference {err:.3e}, calls {cm} / {ct}")
    assert cm == ct == 30
    assert fm == ft
    assert err <= REL


def test_gram_recursion_skips_every_pair_on_a_linear_function():
    """y = 0 for every pair: ys = 0 fails the 1e-10 test each time and the direction stays -g (H_diag 1)."""
    f, x0 = linear()
    kw = dict(lr=1, max_iter=30, tolerance_grad=-1, tolerance_change=-1, history_size=10)
    xt, ct, _ = torch_run(f, x0, **kw)
    xm, cm, _ = model_run(f, x0, **kw)
    assert cm == ct == 30
    assert rel(xm, xt) <= REL


@pytest.mark.parametrize("kw", [dict(tolerance_grad=1e-5, tolerance_change=-1), dict(tolerance_grad=-1, tolerance_change=1e-9),
                                dict(max_iter=20, max_eval=7, tolerance_grad=-1, tolerance_change=-1)])
def test_gram_recursion_stops_where_torch_stops(kw):
    ev = torch.tensor([1.0, 10 ** 0.5, 10.0], dtype=torch.float64)
    b = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    x0 = torch.tensor([0.3, -0.7, 1.1], dtype=torch.float64)

    def f(x):
        return 0.5 * (ev * x * x).sum() - (b * x).sum()

    kw = dict(dict(lr=1, max_iter=50, history_size=100), **kw)
    xt, ct, _ = torch_run(f, x0, **kw)
    xm, cm, _ = model_run(f, x0, **kw)
    print(kw, "closure calls", ct, cm)
    assert cm == ct < kw["max_iter"]
    assert rel(xm, xt) <= REL


def test_gram_recursion_carries_state_across_steps():
    f, x0 = quadratic(seed=3)
    kw = dict(lr=1, max_iter=5, tolerance_grad=-1, tolerance_change=-1, history_size=4)
    xt, ct, ft = torch_run(f, x0, steps=3, **kw)
    xm, cm, fm = model_run(f, x0, steps=3, **kw)
    assert cm == ct == 3 * 5        # each step: its first closure + one after each of the first 4 updates
    assert fm[0] == ft[0] and np.allclose(fm, ft, rtol=REL, atol=0)    # later steps start from the rounded iterate
    assert rel(xm, xt) <= REL


NEW = ("dsr_lbfgs_workspace", "dsr_lbfgs_vector_floats", "dsr_lbfgs_gather", "dsr_lbfgs_dots", "dsr_lbfgs_scalar",
       "dsr_lbfgs_combine")


def test_lbfgs_symbols_declared_and_bound(so):
    abi = importlib.import_module("test_abi")
    decl = abi.declared()
    L = P("_lib")
    for name in NEW:
        assert name in decl and name in L.SIGNATURES, name
        assert len(L.SIGNATURES[name][1]) == decl[name], name
        assert hasattr(ctypes.CDLL(so), name)
    assert {"dsr_lbfgs_workspace", "dsr_lbfgs_vector_floats"} <= set(L._NO_LAUNCH)
    assert L.ABI_VERSION == 9


def test_lbfgs_entry_points_reject_bad_arguments(so):
    """Null pointers, empty or inconsistent sizes and history < 1 return DSR_E_ARG before anything is launched."""
    L = P("_lib")
    lib = L.lib()
    one = ctypes.c_void_p(16)                 # never dereferenced: validation fails first
    n = 1000
    ws = lib.dsr_lbfgs_workspace(5, n, 2)
    assert ws > 0 and lib.dsr_lbfgs_vector_floats(5, n) == (2 * 6 + 2) * 1000
    assert lib.dsr_lbfgs_workspace(0, n, 2) == 0 and lib.dsr_lbfgs_workspace(-3, n, 2) == 0
    assert lib.dsr_lbfgs_workspace(5, 0, 2) == 0 and lib.dsr_lbfgs_workspace(5, n, 0) == 0
    assert lib.dsr_lbfgs_vector_floats(0, n) == 0 and lib.dsr_lbfgs_workspace(2000, n, 1) == 0
    ptrs = (ctypes.c_void_p * 2)(16, 16)
    sizes = (ctypes.c_size_t * 2)(400, 600)
    bad_sizes = (ctypes.c_size_t * 2)(400, 500)
    zero_sizes = (ctypes.c_size_t * 2)(0, 1000)
    nulls = (ctypes.c_void_p * 2)(16, None)
    st = None
    calls = [
        lambda: lib.dsr_lbfgs_gather(2, None, sizes, one, ws, one, 5, n, st),
        lambda: lib.dsr_lbfgs_gather(2, ptrs, None, one, ws, one, 5, n, st),
        lambda: lib.dsr_lbfgs_gather(2, ptrs, sizes, None, ws, one, 5, n, st),
        lambda: lib.dsr_lbfgs_gather(2, ptrs, sizes, one, ws, None, 5, n, st),
        lambda: lib.dsr_lbfgs_gather(0, ptrs, sizes, one, ws, one, 5, n, st),
        lambda: lib.dsr_lbfgs_gather(-1, ptrs, sizes, one, ws, one, 5, n, st),
        lambda: lib.dsr_lbfgs_gather(2, ptrs, sizes, one, ws, one, 0, n, st),          # history < 1
        lambda: lib.dsr_lbfgs_gather(2, ptrs, sizes, one, ws - 1, one, 5, n, st),      # workspace too small
        lambda: lib.dsr_lbfgs_gather(2, ptrs, bad_sizes, one, ws, one, 5, n, st),      # sizes do not add up to n
        lambda: lib.dsr_lbfgs_gather(2, ptrs, zero_sizes, one, ws, one, 5, n, st),     # empty tensor
        lambda: lib.dsr_lbfgs_dots(None, ws, one, 5, n, 2, st),
        lambda: lib.dsr_lbfgs_dots(one, ws, None, 5, n, 2, st),
        lambda: lib.dsr_lbfgs_dots(one, ws, one, 0, n, 2, st),
        lambda: lib.dsr_lbfgs_dots(one, ws, one, 5, 0, 2, st),
        lambda: lib.dsr_lbfgs_scalar(None, ws, 5, n, 2, one, 1, one, 1.0, 20, 25, 1e-7, 1e-9, st),
        lambda: lib.dsr_lbfgs_scalar(one, ws, 5, n, 2, None, 1, one, 1.0, 20, 25, 1e-7, 1e-9, st),
        lambda: lib.dsr_lbfgs_scalar(one, ws, 5, n, 2, one, 1, None, 1.0, 20, 25, 1e-7, 1e-9, st),
        lambda: lib.dsr_lbfgs_scalar(one, ws, -1, n, 2, one, 1, one, 1.0, 20, 25, 1e-7, 1e-9, st),
        lambda: lib.dsr_lbfgs_scalar(one, ws, 5, n, 2, one, 1, one, -1.0, 20, 25, 1e-7, 1e-9, st),   # lr < 0
        lambda: lib.dsr_lbfgs_combine(2, nulls, sizes, one, ws, one, 5, n, st),        # a null parameter
        lambda: lib.dsr_lbfgs_combine(2, ptrs, sizes, one, 16, one, 5, n, st),
        lambda: lib.dsr_lbfgs_combine(2, ptrs, sizes, one, ws, one, 5, n + 1, st),
    ]
    for i, call in enumerate(calls):
        rc = call()
        assert rc == -1, f"call #{i} returned {rc}"
        assert lib.dsr_last_error(), i


def test_fused_lbfgs_constructor_matches_torch_and_rejects_what_it_cannot_run():
    O = P("optim")
    got = inspect.signature(O.FusedLBFGS.__init__).parameters
    want = inspect.signature(torch.optim.LBFGS.__init__).parameters
    assert list(got) == list(want)
    for k in want:
        assert got[k].default == want[k].default, k
    x = torch.zeros(4, requires_grad=True)
    with pytest.raises(NotImplementedError, match="strong_wolfe"):
        O.FusedLBFGS([x], line_search_fn="strong_wolfe")
    with pytest.raises(ValueError):
        O.FusedLBFGS([x], history_size=0)
    with pytest.raises(ValueError):
        O.FusedLBFGS([x], lr=-1)
    with pytest.raises(ValueError):
        O.FusedLBFGS([])
    with pytest.raises(TypeError, match="fp32"):
        O.FusedLBFGS([torch.zeros(4, dtype=torch.float64)])
    with pytest.raises(TypeError, match="contiguous"):
        O.FusedLBFGS([torch.zeros(4, 4).t()])
    with pytest.raises(TypeError, match="device"):
        O.FusedLBFGS([x])                     # a CPU tensor: the optimizer runs on the MI355X only
    sig = inspect.signature(P("utils.DIP").optimize).parameters
    assert sig["fused_lbfgs"].kind == inspect.Parameter.KEYWORD_ONLY and sig["fused_lbfgs"].default is False
