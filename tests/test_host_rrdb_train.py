"""CPU: the host side of training RRDBNet on its growth buffers -- argument checks of dsr_conv_rdb_dgrad / dsr_conv_rdb_wgrad
(nothing is launched), the size queries, the module switch, and the yardstick tests/rrdb_train_ref.py against autograd."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as TF

import rrdb_train_ref as T

PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def lib():
    P("_build").build()
    return P("_lib").lib()


def _dgrad(L, **kw):
    one = 16                                # a non-null "pointer" that is never dereferenced: validation fails first
    f = dict(dtype=L.BF16, N=2, H=9, W=65, K=32, Cout=96, dy=one, lddy=192, dy_off=96, wd=one, scale=1.0, dx=one, lddx=192,
             accumulate=1, g=None, ldg=0, g_limit=0, g_scale=1.0, act_out=32, ldact=192, mask_lo=64, slope=0.2, max_blocks=0)
    f.update(kw)
    return L.RdbDgrad(**f)


def test_dgrad_arguments_are_checked_on_the_host(lib):
    L = P("_lib")
    assert lib.dsr_conv_rdb_dgrad_supported(C.byref(_dgrad(L))) == 1
    assert lib.dsr_conv_rdb_dgrad_supported(None) == 0
    bad = [dict(dy=None), dict(wd=None), dict(dx=None), dict(dtype=2), dict(K=48), dict(K=128), dict(Cout=80), dict(Cout=0),
           dict(dy_off=64),                                   # dy == dx and the ranges overlap
           dict(dy_off=176),                                  # dy_off + K > lddy
           dict(lddx=64),                                     # Cout > lddx
           dict(g_limit=64),                                  # g_limit without g
           dict(g=16, g_limit=64, ldg=64),                    # g is the output tensor
           dict(g=48, g_limit=128, ldg=192),                  # g_limit > Cout
           dict(act_out=None),                                # mask_lo < Cout without act_out
           dict(act_out=16),                                  # act_out is the output tensor
           dict(mask_lo=48), dict(mask_lo=128), dict(slope=0.0), dict(slope=-0.2), dict(ldact=64),
           dict(H=1 << 12, W=1 << 12)]                        # 2^31 bytes per image
    for i, kw in enumerate(bad):
        assert lib.dsr_conv_rdb_dgrad(C.byref(_dgrad(L, **kw)), None) == -1, (i, kw)
        assert lib.dsr_last_error(), i
    assert lib.dsr_conv_rdb_dgrad(None, None) == -1
    for kw in (dict(K=48), dict(Cout=80), dict(H=1 << 12, W=1 << 12), dict(slope=0.0)):
        assert lib.dsr_conv_rdb_dgrad_supported(C.byref(_dgrad(L, **kw))) == 0, kw


def test_wgrad_arguments_sizes_and_chunks(lib):
    L, F = P("_lib"), P("functional")

    def desc(n=2, h=9, w=65, x=16, dy=32, g=48, ldx=192, lddy=192, ldg=64, dt=L.BF16):
        tab = (C.c_void_p * 5)(*([64] * 5))
        return L.RdbWgrad(dt, n, h, w, x, ldx, dy, lddy, g, ldg, 0.2, tab, tab)

    ok = desc()
    assert lib.dsr_conv_rdb_wgrad_supported(C.byref(ok)) == 1 and lib.dsr_conv_rdb_wgrad_supported(None) == 0
    need = lib.dsr_conv_rdb_wgrad_workspace(C.byref(ok))
    chunks = lib.dsr_conv_rdb_wgrad_chunks(C.byref(ok))
    assert chunks == 4 and need >= chunks * 9 * 192 * 192 * 4
    assert (need, chunks) == F.rdb_wgrad_workspace(2, 9, 65, torch.bfloat16)
    for d in (desc(x=None), desc(dy=None), desc(g=None), desc(ldx=128), desc(lddy=256), desc(ldg=32), desc(dt=2), desc(n=0),
              desc(h=1 << 12, w=1 << 12)):
        assert lib.dsr_conv_rdb_wgrad(C.byref(d), C.c_void_p(256), 1 << 40, None) == -1
    assert lib.dsr_conv_rdb_wgrad(None, C.c_void_p(256), 1 << 40, None) == -1
    assert lib.dsr_conv_rdb_wgrad(C.byref(ok), None, 1 << 40, None) == -1
    assert lib.dsr_conv_rdb_wgrad(C.byref(ok), C.c_void_p(256), need - 1, None) == -3          # DSR_E_WORKSPACE
    assert lib.dsr_conv_rdb_wgrad_workspace(C.byref(desc(ldx=128))) == 0 and lib.dsr_conv_rdb_wgrad_chunks(None) == 0
    # the split threshold: chunks of at least RDB_WGRAD_MIN_TILES tiles, at most 64 chunks
    assert F.RDB_WGRAD_MIN_TILES == 8
    for n, h, w in ((1, 4, 128), (1, 4, 129), (1, 5, 33), (2, 1, 1), (16, 32, 32), (12, 64, 64), (3, 100, 300)):
        tiles = T.wgrad_tiles(n, h, w)
        per = max(F.RDB_WGRAD_MIN_TILES, -(-tiles // 64))
        assert F.rdb_wgrad_workspace(n, h, w, torch.float16)[1] == -(-tiles // per), (n, h, w)


def test_module_switch_is_an_attribute_only():
    M = P("models.GAN.rrdbnet")
    net = M.RRDBNet(num_block=1)
    assert net.fused_training is False
    keys = set(net.state_dict())
    assert net.set_fused_training() is net and net.fused_training is True
    assert set(net.state_dict()) == keys and "fused_training" not in keys
    net.set_fused_training(False)
    assert net.fused_training is False
    import inspect
    assert "fused_training" not in inspect.signature(M.RRDBNet.__init__).parameters


def test_yardstick_equals_autograd_of_the_block():
    """The chain of dgrad_value launches and block_param_grads reproduces torch.autograd on a float64 dense block.  Bar: 1e-7
    of the largest magnitude of each tensor -- a structural mistake (a tap, a mask, a channel range) is of order 1, and the
    yardstick is only ever held against fp32 sums (2^-24 = 6e-8 per operation) rounded to 16 bits.  Measured: 7e-9 absolute
    between torch's two float64 convolution-gradient routes."""
    close = lambda got, want: float((got - want).abs().max()) <= 1e-7 * float(want.abs().max())
    torch.manual_seed(3)
    n, h, w, slope, beta = 2, 5, 7, 0.2, 0.2
    x = torch.randn(n, 64, h, w, dtype=torch.float64, requires_grad=True)
    a = torch.randn(n, 64, h, w, dtype=torch.float64, requires_grad=True)
    ws = [(torch.randn(32 if k < 4 else 64, 64 + 32 * k, 3, 3, dtype=torch.float64) * 0.05).requires_grad_(True) for k in range(5)]
    bs = [torch.randn(32 if k < 4 else 64, dtype=torch.float64, requires_grad=True) for k in range(5)]
    xs = [x]
    for k in range(4):
        v = TF.conv2d(torch.cat(xs, 1), ws[k], bs[k], 1, 1)
        xs.append(torch.where(v >= 0, v, v * slope))
    B = torch.cat(xs, 1)
    out = (TF.conv2d(B, ws[4], bs[4], 1, 1) * beta + x) * beta + a          # the third block of an RRDB
    g = torch.randn_like(out)
    out.backward(g)
    Bd = B.detach()
    G = T.dgrad_value(g, ws[4].detach(), None, scale=beta * beta, g=g, g_scale=beta, act=Bd, mask_lo=160, slope=slope)
    for k in (4, 3, 2, 1):
        K, off, cout, mask_lo = T.launch_geometry(k)
        head = T.dgrad_value(G[:, off:off + K], ws[k - 1].detach(), G[:, :cout], act=Bd[:, :cout], mask_lo=mask_lo, slope=slope)
        if k == 2:
            dws, dbs = T.block_param_grads(Bd, torch.cat([head, G[:, cout:]], 1), g, beta * beta)
        G = torch.cat([head, G[:, cout:]], 1)
    assert close(G[:, :64], x.grad) and torch.equal(a.grad, g)
    for k in range(5):
        assert close(dws[k], ws[k].grad), (k, float((dws[k] - ws[k].grad).abs().max()))
        assert close(dbs[k], bs[k].grad), k
