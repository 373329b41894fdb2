"""CPU: what optim.WeightEMA and the dsr_ema_* entry points of csrc/ema.hip promise without a device -- tests/ema_ref.py itself
against torch.optim.swa_utils.AveragedModel in float64, the argument checks of the three C-ABI symbols, the constructor's
refusals, the checkpoint keys, and the optional `ema` keyword of the step recipes."""
import ctypes
import importlib
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import ema_ref

PKG = "deep-super-resolution_amd"
E_ARG = -1                     # DSR_E_ARG: refused by the host-side validation (DSR_E_LAUNCH = -2 would be a launch that failed)


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def so():
    return P("_build").build()


def test_ema_symbols_declared_and_bound(so):
    abi = importlib.import_module("test_abi")
    decl = abi.declared()
    L = P("_lib")
    for name, nargs in (("dsr_ema_update_multi", 10), ("dsr_ema_tick", 3), ("dsr_ema_swap_multi", 5)):
        assert decl.get(name) == nargs and len(L.SIGNATURES[name][1]) == nargs, name
        assert hasattr(ctypes.CDLL(so), name)
        assert name not in L._NO_LAUNCH
    assert L.ABI_VERSION == 9 and L.lib().dsr_abi_version() == 9


# ----------------------------------------------------------------------------- 1: the yardstick is torch's AveragedModel
def _small():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.PReLU()).double()


def _tensors(model):
    out = {k: v.detach().numpy().copy() for k, v in model.named_parameters()}
    out.update({k: v.detach().numpy().copy() for k, v in model.named_buffers()})
    return out


def _perturb(model, gen):
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3)
        for name, b in model.named_buffers():
            if b.is_floating_point():
                b.add_(torch.rand(b.shape, generator=gen, dtype=torch.float64))
            else:
                b.add_(3)


@pytest.mark.parametrize("use_buffers", [False, True])
def test_ema_ref_equals_averaged_model(use_buffers):
    model = _small()
    buffers = [k for k, _ in model.named_buffers()]
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9), use_buffers=use_buffers)
    ref = ema_ref.EmaRef(_tensors(model), buffers, decay=0.9, use_buffers=use_buffers)
    gen = torch.Generator().manual_seed(11)
    for step in range(6):
        _perturb(model, gen)
        avg.update_parameters(model)
        ref.update(_tensors(model))
        theirs = _tensors(avg.module)
        for name, want in theirs.items():
            got = ref.shadow[name]
            if np.issubdtype(want.dtype, np.integer):
                # use_buffers=True: torch truncates the lerp of the counter; the yardstick (and WeightEMA) copy it
                assert np.array_equal(got, _tensors(model)[name]), (step, name)
                if not use_buffers:
                    assert np.array_equal(got, want), (step, name)
                continue
            assert np.abs(got - want).max() <= 1e-12, (step, name, np.abs(got - want).max())
    assert ref.n_averaged == int(avg.n_averaged) == 6
    moved = _tensors(model)
    assert max(np.abs(ref.shadow[k] - moved[k]).max() for k, _ in model.named_parameters()) > 1e-2     # an average, not a copy
    if use_buffers:
        assert int(_tensors(avg.module)["1.num_batches_tracked"]) != int(moved["1.num_batches_tracked"])   # torch's truncation


def test_warmup_closed_form_and_skips():
    """d_k = min(decay, (1 + k) / (10 + k)), k = 1..12 at decay = 0.5: the crossover (2/11 ... 8/17 < 1/2 <= 9/18) lies inside.
    shadow_K = prod(d_k) s_0 + sum_k (1 - d_k) prod_{j > k}(d_j) p_k, in exact rationals."""
    ds = [ema_ref.decay_at(0.5, n, True) for n in range(12)]
    assert ds[:7] == [Fraction(1 + k, 10 + k) for k in range(1, 8)] and all(d < Fraction(1, 2) for d in ds[:7])
    assert ds[7:] == [Fraction(1, 2)] * 5 and Fraction(1 + 8, 10 + 8) == Fraction(1, 2) < Fraction(1 + 9, 10 + 9)
    assert ema_ref.decay_at(0.5, 0, False) is None and ema_ref.decay_at(0.5, 1, False) == Fraction(1, 2)
    rng = np.random.default_rng(2)
    s0 = Fraction(int(rng.integers(-1000, 1000)), 64)
    ps = [Fraction(int(v), 64) for v in rng.integers(-1000, 1000, size=12)]
    shadows, n = ema_ref.run({"w": np.array([float(s0)])}, [{"w": np.array([float(p)])} for p in ps], decay=0.5, warmup=True)
    assert n == 12
    for K in range(1, 13):
        want = s0
        for k in range(K):
            want = ds[k] * want + (1 - ds[k]) * ps[k]
        closed = s0 * math.prod(ds[:K]) + sum((1 - ds[k]) * math.prod(ds[k + 1:K]) * ps[k] for k in range(K))
        assert closed == want
        assert abs(shadows[K - 1]["w"][0] - float(want)) <= 1e-12 * 16
    # a skipped step moves nothing and is not counted: the run equals the run over the other snapshots
    snaps = [{"w": np.array([float(p)])} for p in ps]
    for warm in (False, True):
        a, na = ema_ref.run({"w": np.array([1.0])}, snaps, decay=0.5, warmup=warm, skipped={0, 4})
        b, nb = ema_ref.run({"w": np.array([1.0])}, [s for i, s in enumerate(snaps) if i not in (0, 4)], decay=0.5, warmup=warm)
        assert na == nb == 10 and a[-1]["w"][0] == b[-1]["w"][0]
        assert a[0]["w"][0] == 1.0 and a[4]["w"][0] == a[3]["w"][0]


# ----------------------------------------------------------------------------- 2: bad arguments
def test_ema_entry_points_reject_bad_arguments(so):
    """Every pattern is refused by the host-side validation (DSR_E_ARG, not a failed launch: there is no GPU here) with a
    message that names the entry point; count == 0 is fine and does nothing."""
    lib = P("_lib").lib()
    N, st = None, None
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)       # never dereferenced: validation fails first
    a = (ctypes.c_void_p * 2)(64, 128)
    b = (ctypes.c_void_p * 2)(1024, 2048)
    oddp = (ctypes.c_void_p * 2)(64, 130)
    holes = (ctypes.c_void_p * 2)(1024, None)
    sizes = (ctypes.c_size_t * 2)(400, 600)
    huge = (ctypes.c_size_t * 2)(400, 1 << 42)
    flags = (ctypes.c_ubyte * 2)(0, 1)
    up = lib.dsr_ema_update_multi
    calls = [
        ("ema_update_multi", lambda: up(-1, a, b, sizes, flags, 0.9, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, N, b, sizes, flags, 0.9, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, N, sizes, flags, 0.9, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, N, flags, 0.9, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, 0.9, 0, N, N, st)),                # no counter
        ("ema_update_multi", lambda: up(0, a, b, sizes, flags, 0.9, 0, N, N, st)),                # ... whatever the count
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, 0.9, 0, odd, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, 0.9, 0, one, odd, st)),
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, -0.1, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, 1.5, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, float("nan"), 1, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, 0.9, 2, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, sizes, flags, 0.9, -1, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, holes, sizes, flags, 0.9, 0, one, N, st)),          # a parameter without a shadow's partner
        ("ema_update_multi", lambda: up(2, holes, b, sizes, N, 0.9, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, oddp, b, sizes, flags, 0.9, 0, one, N, st)),           # not 4-byte aligned
        ("ema_update_multi", lambda: up(2, a, oddp, sizes, flags, 0.9, 0, one, N, st)),
        ("ema_update_multi", lambda: up(2, a, b, huge, flags, 0.9, 0, one, N, st)),
        ("ema_tick", lambda: lib.dsr_ema_tick(N, N, st)),
        ("ema_tick", lambda: lib.dsr_ema_tick(N, one, st)),
        ("ema_tick", lambda: lib.dsr_ema_tick(odd, N, st)),
        ("ema_tick", lambda: lib.dsr_ema_tick(one, odd, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(-1, a, b, sizes, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(2, N, b, sizes, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(2, a, N, sizes, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(2, a, b, N, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(2, a, holes, sizes, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(2, holes, b, sizes, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(2, a, oddp, sizes, st)),
        ("ema_swap_multi", lambda: lib.dsr_ema_swap_multi(2, a, b, huge, st)),
    ]
    for i, (who, call) in enumerate(calls):
        rc = call()
        assert rc == E_ARG, f"call #{i} returned {rc}: {lib.dsr_last_error()}"
        assert who.encode() in lib.dsr_last_error(), (i, lib.dsr_last_error())
    assert up(0, a, b, sizes, flags, 0.9, 0, one, N, st) == 0
    assert up(0, N, N, N, N, 1.0, 1, one, one, st) == 0
    assert lib.dsr_ema_swap_multi(0, N, N, N, st) == 0 and lib.dsr_ema_swap_multi(0, a, b, sizes, st) == 0
    # the documented "skip" entries are not errors: with nothing but those a call validates and launches nothing
    empty = (ctypes.c_size_t * 2)(0, 600)
    nulls = (ctypes.c_void_p * 2)(64, None)
    assert up(2, nulls, nulls, empty, N, 0.9, 0, one, N, st) == 0
    assert lib.dsr_ema_swap_multi(2, nulls, nulls, empty, st) == 0
    assert lib.dsr_ema_swap_multi(2, a, a, sizes, st) == 0            # a tensor against itself


# ----------------------------------------------------------------------------- 3: constructor refusals
def test_weight_ema_refusals():
    O = P("optim")
    lin = nn.Linear(3, 2)
    for bad in (-0.1, 1.0001, float("nan"), True, "0.9", None, [0.9]):
        with pytest.raises(ValueError, match="decay"):
            O.WeightEMA(lin, decay=bad)
    for ok in (0, 0.0, 1, 1.0, 0.999):
        assert O.WeightEMA(lin, decay=ok).decay == float(ok)
    with pytest.raises(ValueError, match="without parameters"):
        O.WeightEMA(nn.Tanh())
    with pytest.raises(ValueError, match="without parameters"):
        O.WeightEMA(nn.Sequential())
    with pytest.raises(TypeError, match=r"1\.weight is torch\.float64"):
        O.WeightEMA(nn.Sequential(nn.Linear(3, 2), nn.Linear(2, 2).double()))
    with pytest.raises(TypeError, match=r"0\.weight is torch\.float16"):
        O.WeightEMA(nn.Sequential(nn.Linear(3, 2).half()))
    strided = nn.Linear(3, 2)
    strided.weight = nn.Parameter(torch.zeros(3, 2).t())
    assert not strided.weight.is_contiguous()
    with pytest.raises(TypeError, match="weight is torch.float32, contiguous=False"):
        O.WeightEMA(strided)
    bn = nn.BatchNorm2d(4)
    bn.running_mean = bn.running_mean.double()
    O.WeightEMA(bn)                                              # copied: any dtype of 4n bytes
    with pytest.raises(TypeError, match="running_mean is torch.float64"):
        O.WeightEMA(bn, use_buffers=True)
    flag = nn.Linear(3, 2)
    flag.register_buffer("on", torch.ones(3, dtype=torch.bool))
    with pytest.raises(TypeError, match="on is torch.bool"):
        O.WeightEMA(flag)


def test_weight_ema_needs_the_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    O = P("optim")
    model = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.PReLU())
    ema = O.WeightEMA(model, decay=0.9)
    assert ema.n_averaged.dtype == torch.int32 and ema.n_averaged.shape == (1,) and ema.n_averaged.item() == 0
    for op in (ema.update, ema.swap, ema.copy_to, lambda: ema.copy_to(nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.PReLU()))):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            op()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        with ema.average_parameters():
            raise AssertionError("the block must not run")
    with pytest.raises(RuntimeError, match="copy_to"):
        ema.restore()
    sc = O.DynamicLossScaler()
    assert sc._checked is False


def test_ema_keyword_is_optional_everywhere():
    S, E, O = P("steps"), P("evaluate"), P("optim")
    for fn in (S.gen_l1_step, S.gen_lpips_step, S.gen_msssim_step):
        p = inspect.signature(fn).parameters["ema"]
        assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    assert inspect.signature(S.gan_step).parameters["ema"].default is None
    assert inspect.signature(S._backward_and_step).parameters["ema"].default is None
    assert inspect.signature(E.evaluate_generator).parameters["ema"].default is None
    sig = inspect.signature(O.WeightEMA.__init__).parameters
    assert (sig["decay"].default, sig["warmup"].default, sig["use_buffers"].default) == (0.999, False, False)
    assert list(inspect.signature(O.WeightEMA.update).parameters) == ["self", "scaler"]
    with pytest.raises(ValueError, match="another module"):
        E.evaluate_generator(nn.Linear(2, 2), [], ema=O.WeightEMA(nn.Linear(2, 2)))


# ----------------------------------------------------------------------------- 4: checkpoint keys
def test_module_state_dict_is_the_modules_own_format():
    O, G = P("optim"), P("models.GAN.generator")
    torch.manual_seed(0)
    gen = G.Generator(factor=2, residual_blocks_count=1)
    ema = O.WeightEMA(gen, decay=0.5)
    before = {k: v.clone() for k, v in gen.state_dict().items()}
    with torch.no_grad():
        for p in gen.parameters():
            p.add_(1.0)                                         # the average is the copy taken at construction, not a view
    want, got = gen.state_dict(), ema.module_state_dict()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert got[k].data_ptr() != want[k].data_ptr(), k
    assert all(torch.equal(got[k], before[k]) for k in want)
    assert not any(torch.equal(got[k], want[k]) for k, _ in gen.named_parameters())
    fresh = G.Generator(factor=2, residual_blocks_count=1)
    assert fresh.load_state_dict(got, strict=True).missing_keys == []
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, got[k]), k
    # the EMA's own state: every tensor once, the counter, the three settings; it round-trips
    sd = ema.state_dict()
    assert set(sd) == {"shadow", "n_averaged", "decay", "warmup", "use_buffers"}
    assert set(sd["shadow"]) == set(want.keys()) and sd["n_averaged"] == 0 and sd["decay"] == 0.5
    other = O.WeightEMA(gen, decay=0.25, warmup=True)
    sd["n_averaged"] = 7
    other.load_state_dict(sd)
    assert other.decay == 0.5 and other.warmup is False and other.n_averaged.item() == 7
    assert all(torch.equal(a, b) for a, b in zip(other._shadow, ema._shadow))
    bad = dict(sd, shadow={k: v for k, v in list(sd["shadow"].items())[1:]})
    with pytest.raises(RuntimeError, match="names differ"):
        other.load_state_dict(bad)
    with pytest.raises(ValueError, match="decay"):
        other.load_state_dict(dict(sd, decay=2.0))
