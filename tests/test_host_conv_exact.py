"""CPU: the exact-integer convolution sweep's reference, regime conditions and dispatch coverage (tests/conv_exact_ref.py).

Nothing here launches a kernel: the reference is checked against float64 torch.nn.functional.conv2d + autograd (both are exact
on these operands, so that is equality), every case is shown to stay inside the exact regime for both storage types, and the
case table is shown to reach every kernel name the dispatcher can report -- planning only (dsr_conv_kernel_name)."""
import importlib

import pytest
import torch
import torch.nn.functional as TF

import conv_exact_ref as R

PKG = "deep-super-resolution_amd"


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + "._lib").lib()


def _torch_pad(x, pad, mode):
    if pad == 0:
        return x
    return TF.pad(x, (pad,) * 4, mode={R.PAD_ZERO: "constant", R.PAD_REFLECT: "reflect", R.PAD_REPLICATE: "replicate"}[mode])


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_reference_equals_float64_autograd(name):
    r = R.layer_a(name)
    c = r["case"]
    x = r["x"].clone().requires_grad_(True)
    w = r["w"].clone().requires_grad_(True)
    y = TF.conv2d(_torch_pad(x, c["pad"], c["mode"]), w, None, stride=c["stride"])
    assert torch.equal(y.detach(), R.conv_fwd(r["x"], r["w"], c["stride"], c["pad"], c["mode"]))
    y.backward(r["g"])
    assert torch.equal(x.grad, R.conv_dgrad(r["g"], r["w"], c["h"], c["w"], c["stride"], c["pad"], c["mode"]))
    assert torch.equal(w.grad, R.conv_wgrad(r["x"], r["g"], c["k"], c["stride"], c["pad"], c["mode"]))
    if c["dgrad"] is not None:
        assert torch.equal(x.grad, r["dx_plain"])
    # the epilogue against torch's own activation / shuffle on the same exact values (away from the kink the two agree)
    z = r["inter"][-2]
    want = {R.ACT_NONE: z, R.ACT_RELU: torch.relu(z)}.get(c["act"], TF.leaky_relu(z, c["slope"]))
    assert torch.equal(r["inter"][-1], want)
    if c["ps"]:
        assert torch.equal(R.pixel_shuffle2(r["y"]), TF.pixel_shuffle(r["y"], 2))
        assert torch.equal(R.pixel_unshuffle2(TF.pixel_shuffle(r["y"], 2)), r["y"])


@pytest.mark.parametrize("dtype", [R.BF16, R.F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_regime_a_is_exact(name, dtype):
    """Every partial sum stays below 2^24 whatever the summation order (bounded by sum |x| |w|), and every stored 16-bit
    tensor -- operands, folded intermediates, y, g, dx -- is representable in the storage type: no rounding anywhere."""
    r = R.layer_a(name)
    c = r["case"]
    for key in ("bound_fwd", "bound_stats", "bound_db", "bound_dgrad", "bound_wgrad", "bound_dprelu"):
        if key in r:
            assert r[key] < R.EXACT_LIMIT, (key, r[key])
    for key in ("x", "w", "dy", "g", "residual", "addend"):
        if r.get(key) is not None:
            assert R.representable(r[key], dtype), key
    for t in r["inter"]:
        assert R.representable(t, dtype)
    if not c["nchw"]:
        assert R.representable(r["y"], dtype)
    if c["dgrad"] is not None:
        assert R.representable(r["dx_plain"], dtype) and R.representable(r["dx"], dtype)
    # the case exercises what it is there for: both branches of its activation, non-trivial outputs
    if c["act"] != R.ACT_NONE:
        assert int((r["inter"][-2] < 0).sum()) > 10 and int((r["inter"][-2] > 0).sum()) > 10
    assert int((r["y"] != 0).sum()) > r["y"].numel() // 4
    if "dw" in r:
        assert int((r["dw"] != 0).sum()) > r["dw"].numel() // 4


@pytest.mark.parametrize("dtype", [R.BF16, R.F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["regime_b"]])
def test_regime_b_rounds(name, dtype):
    """Partial sums still exact (< 2^24), operands representable, and the outputs leave the representable range: at least a
    few hundred exact ties, rounded both ways (kept bit even below and even above), forward and input gradient."""
    r = R.layer_b(name, dtype)
    assert r["bound_fwd"] < R.EXACT_LIMIT and r["bound_dgrad"] < R.EXACT_LIMIT
    for key in ("x", "w", "g"):
        assert R.representable(r[key], dtype), key
    for key in ("y_exact", "dx_exact"):
        down, up = R.tie_counts(r[key], dtype)
        assert down >= 100 and up >= 100 and down + up >= 300, (key, down, up, r["amps"])
        assert not R.representable(r[key], dtype)


def test_case_table_reaches_every_kernel(lib, monkeypatch):
    """Each case names the kernels it is there for; dsr_conv_kernel_name must report exactly those (planning launches
    nothing), and the union over the table must be every name the dispatcher can return: a dispatch change that drops a
    kernel out of the sweep fails here, on any machine."""
    seen, slabs = set(), {}
    for c in R.CASES:
        with monkeypatch.context() as m:
            for k, v in c["env"].items():
                m.setenv(k, v)
            for dtype in (R.BF16, R.F16):
                got = R.kernel_names(lib, c, dtype)
                want = tuple(w if w is not None else g for w, g in zip(c["names"], got))
                assert got == want, (c["name"], got, c["names"])
        seen.update(n for n in c["names"] if n is not None)
        if c["names"][2] not in (None, R.W_RGB9):
            slabs.setdefault(c["names"][2], []).append(R.wgrad_slabs(lib, c))
    # every weight-gradient kernel has a case whose result is reduced over at least two partial slabs
    assert all(max(v) >= 2 for v in slabs.values()), slabs
    assert seen == R.ALL_KERNEL_NAMES, (R.ALL_KERNEL_NAMES - seen, seen - R.ALL_KERNEL_NAMES)


def test_kernel_name_list_matches_the_dispatcher_source():
    """ALL_KERNEL_NAMES is the full list plan_name() and the weight-gradient branch of dsr_conv_kernel_name can return."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PKG, "csrc", "conv_api.hip")).read()
    body = src[src.index("static const char* plan_name("):src.index("// ---- input gradient of a 3x3 stride-2 layer + the BatchNorm")]
    assert set(re.findall(r'"(conv_[^"]+)"', body)) == R.ALL_KERNEL_NAMES


def test_r16_rounds_to_nearest_even():
    t = torch.tensor([256.0, 257.0, 258.0, 259.0, 513.0, 514.0, 518.0, -257.0, 0.25, 32.25, 64.25])
    assert R.r16(t, R.BF16).tolist() == [256.0, 256.0, 258.0, 260.0, 512.0, 512.0, 520.0, -256.0, 0.25, 32.25, 64.0]
    t = torch.tensor([2048.0, 2049.0, 2051.0, 4098.0, 4102.0, -2049.0, 1024.5, 1025.5])
    assert R.r16(t, R.F16).tolist() == [2048.0, 2048.0, 2052.0, 4096.0, 4104.0, -2048.0, 1024.0, 1026.0]
    assert R.representable(torch.tensor([255.0, -256.0, 0.75]), R.BF16) and not R.representable(torch.tensor([257.0]), R.BF16)
    assert R.tie_counts(torch.tensor([257.0, 259.0, 258.0, 513.0, 514.0, 518.0]), R.BF16) == (2, 2)
