"""Autograd functions over the C ABI (include/dsr_hip.h): the device work behind the
reference's nn.Module surface.

Internal activation format: torch tensor [N, H, W, Cp] (NHWC, Cp = channels rounded up to 8),
dtype bfloat16 (training) or float16 (inference).  Parameters stay fp32 in the reference's
layouts, so state_dicts interchange with the reference.

PyTorch is only plumbing here: it owns device memory, the stream and the autograd tape; every
FLOP is a HIP kernel from csrc/.  Nothing in this file can run without the extension.
"""
import ctypes as C
import os
import weakref

import torch

from . import _lib
from ._lib import (ACT_ELU, ACT_LEAKY, ACT_NONE, ACT_PRELU, ACT_RELU, ACT_SIGMOID, ACT_TANH, BF16, F16,  # noqa: F401
                   FEAT_L1, FEAT_MSE, PAD_REFLECT, PAD_REPLICATE, PAD_ZERO, ConvDesc, Epilogue, _ptr, _stream, check)

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def r8(c):
    return (c + 7) // 8 * 8


def _dt(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"activation dtype must be bfloat16 or float16, got {t.dtype}")


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("deep-super-resolution_amd: tensors must live on the MI355X (cuda device); "
                           "there is no CPU implementation of this path")


# ----------------------------------------------------------------------------- per-launch timing (bench.py roofline leg)
KERNEL_LOG = None          # set to a list to record (kind, desc-tuple, start_event, end_event) per conv launch


_OPS = {"fwd": 0, "dgrad": 1, "wgrad": 2}


def _timed(kind, desc, fn, ep=None, name=None):
    """Run one C-ABI conv call; when KERNEL_LOG is a list, bracket it with HIP events on the launch stream."""
    if KERNEL_LOG is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn()
    e1.record()
    if name is None:
        name = _lib.lib().dsr_conv_kernel_name(C.byref(desc), _OPS[kind], C.byref(ep) if ep is not None else None).decode()
    KERNEL_LOG.append((kind, (desc.N, desc.H, desc.W, desc.Cin, desc.Cout, desc.KH, desc.KW, desc.stride, desc.pad), e0, e1, name))
    return rc


# ----------------------------------------------------------------------------- weight images
_pack_cache = {}


def _version(p):
    return (p._version, getattr(p, "_dsr_version", 0), p.data_ptr())


def bump(p):
    """Called by the fused optimiser after it rewrote a parameter through its raw pointer."""
    p._dsr_version = getattr(p, "_dsr_version", 0) + 1


def clear_pack_cache():
    _pack_cache.clear()


def check_prelu_slopes(module):
    """Raise if a one-parameter nn.PReLU of `module` that feeds a fused conv+PReLU launch (generator.py:48,34: the head
    and the PixelShuffle blocks) holds a slope <= 0: those launches keep only the activation OUTPUT, from which the
    backward can tell the branch for a positive slope only (see ConvAct).  One host sync; call it between steps."""
    import torch.nn as nn
    bad = [(name, float(m.weight.detach().min())) for name, m in module.named_modules()
           if isinstance(m, nn.PReLU) and not float(m.weight.detach().min()) > 0.0]
    if bad:
        raise RuntimeError("PReLU slope(s) not positive: " + ", ".join(f"{n}.weight={v:g}" for n, v in bad) +
                           " -- conv+PReLU launches that store only the activation output cannot back-propagate "
                           "through them (their gradients are NaN by construction)")


def packed_weights(weight, desc, dtype):
    """16-bit [T][Cout_p][Cin_p] (forward) and [T][Cin_p][Cout_p] (dgrad) images of an OIHW fp32 weight."""
    derived = getattr(weight, "_dsr_derived", False)
    if not derived:
        key = (id(weight), dtype, tuple(weight.shape))
        ver = _version(weight)
        hit = _pack_cache.get(key)
        # ids (and allocator addresses) are recycled once a tensor dies: a hit must be THIS tensor object
        if hit is not None and hit[0] == ver and hit[3]() is weight:
            return hit[1], hit[2]
    lib = _lib.lib()
    nf = lib.dsr_conv_packed_elems(C.byref(desc), 0)
    nd = lib.dsr_conv_packed_elems(C.byref(desc), 1)
    wf = torch.empty(nf, dtype=dtype, device=weight.device)
    wd = torch.empty(nd, dtype=dtype, device=weight.device)
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    check(lib.dsr_conv_pack_weight(C.byref(desc), _ptr(w), _ptr(wf), _ptr(wd), _stream()))
    if derived:
        # a weight computed anew by every forward (SpectralNormWeight): its images belong to that one call -- they never enter
        # the cache, which would otherwise pin them until 4096 dead entries have piled up
        return wf, wd
    _pack_cache[key] = (ver, wf, wd, weakref.ref(weight))
    if len(_pack_cache) > 4096:          # dead entries of short-lived tensors (tests); live models are far smaller
        for k in [k for k, v in _pack_cache.items() if v[3]() is None]:
            del _pack_cache[k]
    return wf, wd


def repack_cached(params):
    """Refresh, in one launch per 48 tensors, the packed images of every conv weight in `params` that has some (called by
    the fused optimiser right after it rewrote them; the images are rewritten in place, on the current stream)."""
    by_dtype = {}
    for p in params:
        if p.dim() != 4 or not p.is_contiguous():
            continue
        for dtype in (torch.bfloat16, torch.float16):
            key = (id(p), dtype, tuple(p.shape))
            hit = _pack_cache.get(key)
            if hit is not None and hit[3]() is p and hit[0] != _version(p):
                by_dtype.setdefault(dtype, []).append((key, p, hit))
    lib = _lib.lib()
    for dtype, items in by_dtype.items():
        k = len(items)
        ints = lambda vals: (C.c_int * k)(*vals)
        check(lib.dsr_conv_pack_weight_multi(
            BF16 if dtype == torch.bfloat16 else F16, k, _lib.ptr_table([p for _, p, _ in items]),
            _lib.ptr_table([h[1] for _, _, h in items]), _lib.ptr_table([h[2] for _, _, h in items]),
            ints([p.shape[0] for _, p, _ in items]), ints([p.shape[1] for _, p, _ in items]),
            ints([p.shape[2] * p.shape[3] for _, p, _ in items]), _stream()))
        for key, p, hit in items:
            _pack_cache[key] = (_version(p), hit[1], hit[2], hit[3])


def make_desc(x, cout, kh, kw, stride, pad, pad_mode, cin):
    n, h, w, cp = x.shape
    assert cp == r8(cin), (cp, cin)
    return ConvDesc(_dt(x), n, h, w, cin, cout, kh, kw, stride, pad, pad_mode)


def first2_supported(img, w0, w1, stride1):
    """The image layer + the stride-2 64 -> 64 layer behind it as one forward kernel (dsr_conv_first2_fwd)?"""
    if not (img.is_cuda and img.dim() == 4 and img.shape[-1] == 8 and tuple(w0.shape[2:]) == (3, 3) and tuple(w1.shape) == (64, 64, 3, 3)
            and w0.shape[0] == 64 and w0.shape[1] <= 8 and stride1 == 2):
        return False
    n, h, w, _ = img.shape
    d0 = ConvDesc(_dt(img), n, h, w, w0.shape[1], 64, 3, 3, 1, 1, PAD_ZERO)
    d1 = ConvDesc(_dt(img), n, h, w, 64, 64, 3, 3, 2, 1, PAD_ZERO)
    return bool(_lib.lib().dsr_conv_first2_supported(C.byref(d0), C.byref(d1)))


def _out_hw(desc):
    oh, ow = C.c_int(), C.c_int()
    check(_lib.lib().dsr_conv_out_size(C.byref(desc), C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def _conv_prologue(x, weight, cfg):
    """What every conv node's forward starts from: (contiguous x, desc, oh, ow, forward image, dgrad image)."""
    _need_gpu(x)
    x = x.contiguous()
    cout, cin, kh, kw = weight.shape
    desc = make_desc(x, cout, kh, kw, cfg["stride"], cfg["pad"], cfg.get("pad_mode", PAD_ZERO), cin)
    oh, ow = _out_hw(desc)
    wf, wd = packed_weights(weight, desc, x.dtype)
    return x, desc, oh, ow, wf, wd


def _scr():
    return _lib.lib().dsr_pw_scratch_rows()


def _partials(rows, width, device):
    """fp32 scratch for `rows` partial rows of `width` floats, with the tail rows that compact_rows (csrc/pointwise.hip)
    writes behind them when it folds the table."""
    return torch.empty((rows + _scr()) * width, dtype=torch.float32, device=device)


def _reduce_blocks(p):
    rpb = C.c_int()
    blocks = _lib.lib().dsr_pw_reduce_blocks(p, C.byref(rpb))
    return blocks, rpb.value


_BN_BWD_BLOCKS = int(os.environ.get("DSR_PW_BN_REDUCE_BLOCKS", "1280"))


def _bn_bwd_blocks(p, act):
    """Grid of dsr_pw_bn_act_bwd_reduce.  Without the PReLU slope gradient the kernel fits five waves per SIMD: 1280 blocks
    (five per CU, all resident at once) stream 10-20 % faster than the 1024 of the other row reductions
    (tools/microbench_pw.py); the PReLU form (four waves per SIMD) keeps the common grid."""
    if act == ACT_PRELU:
        return _reduce_blocks(p)
    rpb = max(64, -(-p // _BN_BWD_BLOCKS))
    return -(-p // rpb), rpb


_wgrad_batch = None      # the open batched_wgrad context (per process: backward passes are issued from one thread here)


class batched_wgrad:
    """``with batched_wgrad(): loss.backward()`` -- every 3x3 stride-1 weight gradient of that backward pass is formed by ONE
    grouped contraction launch and one reduction launch when the block exits (dsr_conv_wgrad_batched), instead of one
    contraction + two reduction launches per layer.  The SRGAN trunk is 33 such layers with a single 64x64 output tile
    each (generator.py:7-25,52): alone, a layer can only fill the chip by cutting its pixels into ~256 chunks and
    reducing 37 MB of partials; together ~30 chunks per layer do.  A weight that appears twice in the graph (the
    discriminator on the real and the generated batch, train_GAN.py:44-47) gets both contributions summed inside the
    reduction, which also replaces autograd's elementwise accumulation.

    Inside the block a layer's backward returns its (still unwritten) gradient tensor, so nothing may READ a weight's
    .grad before the block exits: hooks on those parameters, and accumulation into an existing .grad -- a weight whose
    .grad is already set is therefore computed at once, unbatched.  On exit each parameter's .grad is checked to be the
    tensor the launch wrote (autograd may have cloned it) and repaired if not."""

    MAX_PROBLEMS = 256           # kMaxBatchProblems of dsr_conv_wgrad_batched: larger groups are split in flush()

    def __init__(self, enabled=True, early_stream=None, early_every=0):
        """early_stream / early_every: every `early_every` collected problems are launched AT ONCE on `early_stream` (behind an
        event of the stream the backward pass runs on) instead of at the exit: the grouped launch of a long chain of layers
        (the generator's trunk) then runs beside the rest of that chain's input gradients instead of after them.  Only for
        weights used once inside the block; the exit waits for the early launches."""
        self.enabled = enabled
        self.items = {}          # id(weight) -> [weight, returned tensor, alias of it, [(desc, x, dy), ...], [extra addends]]
        self.unbatched = set()   # id(weight) of weights that already returned a REAL gradient inside this block
        self.early_stream = early_stream if early_every > 0 else None
        self.early_every = int(early_every)
        self.done = []           # entries whose launch is already on early_stream
        self.early_ids = set()
        self.reused = set()      # ... and which were used again afterwards

    def __enter__(self):
        global _wgrad_batch
        self.outer = _wgrad_batch
        if self.enabled and self.outer is None:
            _wgrad_batch = self
        return self

    def __exit__(self, et, ev, tb):
        global _wgrad_batch
        if _wgrad_batch is self:
            _wgrad_batch = None
            if et is None:
                self.flush()
                self._finish_early()
            else:
                if self.done:
                    torch.cuda.current_stream().wait_stream(self.early_stream)
                # backward raised: the launch never ran, so a .grad that autograd already pointed at one of the placeholder
                # tensors holds uninitialised memory -- drop it rather than leave garbage behind
                for weight, _, alias, _, _ in self.items.values():
                    g = weight.grad
                    if g is not None and g.data_ptr() == alias.data_ptr():
                        weight.grad = None
            self.items = {}
            self.unbatched = set()
            self.done = []
            self.early_ids = set()
            self.reused = set()
        return False

    def add(self, weight, desc, x, dy, wshape):
        """The gradient tensor to return for this use of `weight` (None for a second use: its contribution joins the first)."""
        ent = self.items.get(id(weight))
        if ent is not None:
            ent[3].append((desc, x, dy))
            return None
        dw = torch.empty(wshape, dtype=torch.float32, device=x.device)
        # (the alias shares dw's storage through a tensor object of its own: autograd takes over a gradient only while
        # nobody else holds the very tensor it was handed)
        self.items[id(weight)] = [weight, None, dw.detach(), [(desc, x, dy)], []]
        if self.early_stream is not None and sum(len(e[3]) for e in self.items.values()) >= self.early_every:
            self._launch_early()
        return dw

    def batchable(self, weight):
        """False for a weight whose gradient launch is already under way on the early stream: a second use of it inside the
        block is computed on its own, after that launch (the caller's stream is made to wait for it here)."""
        if id(weight) in self.early_ids:
            torch.cuda.current_stream().wait_stream(self.early_stream)
            self.reused.add(id(weight))      # autograd now sums a real tensor onto the finished placeholder: .grad is that sum
            return False
        return id(weight) not in self.unbatched

    def _launch_early(self):
        cur = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(cur)                       # every dy collected so far was enqueued on `cur` before this point
        self.early_stream.wait_event(ev)
        ents = list(self.items.values())
        with torch.cuda.stream(self.early_stream):
            self._launch(ents)
        for weight, _, alias, uses, _ in ents:
            alias.record_stream(self.early_stream)
            for _, x, dy in uses:            # (allocated on `cur`: not to be handed out again before the early launch has read them)
                x.record_stream(self.early_stream)
                dy.record_stream(self.early_stream)
            self.early_ids.add(id(weight))
        self.done.extend(ents)
        self.items = {}

    def _finish_early(self):
        if not self.done:
            return
        torch.cuda.current_stream().wait_stream(self.early_stream)
        self._settle([e for e in self.done if id(e[0]) not in self.reused])

    def add_unbatchable(self, weight, dw):
        """A use of `weight` that the grouped launch cannot take (other stride / padding ...), computed at once as `dw`.  If an
        earlier use of the same weight joined the batch, autograd already holds its PLACEHOLDER: summing a real tensor into it
        would add garbage, and the later launch would overwrite the sum.  The real contribution is therefore kept here and
        added to the launch's result in flush(); the caller returns None for this use.  Returns True when that happened."""
        ent = self.items.get(id(weight))
        if ent is None:
            self.unbatched.add(id(weight))       # later batchable uses of this weight must not join the batch either
            return False
        ent[4].append(dw)
        return True

    def flush(self):
        if not self.items:
            return
        ents = list(self.items.values())
        self._launch(ents)
        self._settle(ents)

    def _launch(self, ents):
        lib = _lib.lib()
        by_dtype = {}
        for ent in ents:
            by_dtype.setdefault(ent[3][0][0].dtype, []).append(ent)
        groups = []
        for group in by_dtype.values():      # at most MAX_PROBLEMS problems per launch; the uses of one weight stay together
            cur, ncur = [], 0
            for ent in group:
                if cur and ncur + len(ent[3]) > self.MAX_PROBLEMS:
                    groups.append(cur)
                    cur, ncur = [], 0
                cur.append(ent)
                ncur += len(ent[3])
            if cur:
                groups.append(cur)
        for group in groups:
            descs, xs, dys, dws = [], [], [], []
            for weight, _, alias, uses, _ in group:
                for desc, x, dy in uses:
                    descs.append(desc)
                    xs.append(x.data_ptr())
                    dys.append(dy.data_ptr())
                    dws.append(alias.data_ptr())
            n = len(descs)
            darr = (_lib.ConvDesc * n)(*descs)
            xa, ya, wa = (C.c_void_p * n)(*xs), (C.c_void_p * n)(*dys), (C.c_void_p * n)(*dws)
            wsz = lib.dsr_conv_wgrad_batched_workspace(n, darr, wa)
            ws = torch.empty(max(wsz, 16), dtype=torch.uint8, device=group[0][2].device)
            if KERNEL_LOG is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            check(lib.dsr_conv_wgrad_batched(n, darr, xa, ya, wa, _ptr(ws), wsz, _stream()))
            if KERNEL_LOG is not None:
                e1.record()
                KERNEL_LOG.append(("wgrad_batch", [(d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad) for d in descs],
                                   e0, e1, "conv_wgrad_dma_batch_kernel"))

    @staticmethod
    def _settle(ents):
        for weight, _, alias, uses, extra in ents:
            for e in extra:                               # contributions of uses the grouped launch could not take
                alias.add_(e)
            g = weight.grad
            if g is None:
                continue                                  # (nobody kept the gradient: e.g. torch.autograd.grad)
            if g.data_ptr() != alias.data_ptr():
                g.copy_(alias)                            # autograd stored a copy made before the launch: refresh it


FIRST_BWD_RECOMPUTE = os.environ.get("DSR_FIRST_BWD_RECOMPUTE", "1") != "0"   # 0: the first-layer backward reads the stored activation

ACT_LINKS = True      # development switch: False makes every layer run its own activation-backward pass (A/B of kind "act")
FIRST2_BACKWARD = os.environ.get("DSR_FIRST2_BACKWARD", "1") != "0"   # 0: the first two layers' backward as separate launches
DGRAD_BN = os.environ.get("DSR_DGRAD_BN_LINK", "1") != "0"             # 0: BatchNorm-backward sums always by their own reduce pass
DGRAD_PS = os.environ.get("DSR_DGRAD_PS_LINK", "1") != "0"             # 0: the PixelShuffle-PReLU backward always as its own pass


def _identity(t):
    return (t.data_ptr(), t._version, tuple(t.shape))


def zero_placeholder(shape, dtype, device):
    """The gradient a consumer returns to autograd when the real one went through a Handover: zeros of `shape` over ONE
    element (stride 0), so that a reader the link did not foresee adds zero.  Allocated per use (a captured backward pass
    replays the fill)."""
    return torch.zeros(1, dtype=dtype, device=device).expand(shape)


class Handover:
    """Part of one node's backward done by its neighbour: the node that CONSUMES an activation x runs some of the backward
    of the node that PRODUCED x inside its own input-gradient launch, and the producer skips that work.  The model makes one
    empty Handover per activation and forward call and gives it to the producer as cfg["out_link"] and to the consumer as
    cfg["in_link"] (MaxPool2: the second argument).

      offer   (producer, forward)   `kind` and the payload the consumer's kernel needs -- only when the producer will be able
                                    to use what comes back:
                "act"     act, slope                           the consumer multiplies dx by act'(x): dsr_conv_dgrad_masked,
                                                               dsr_maxpool2_relu_bwd; deposits True
                "bn"      y, scale, shift, act, slope          the consumer also forms the BatchNorm-backward sums:
                                                               dsr_conv_dgrad_bn; deposits (part, rows)
                "ps"      prelu                                the consumer also runs the PixelShuffle + PReLU backward:
                                                               dsr_conv_dgrad_ps; deposits (dy, part, rows), dx a placeholder
                "first2"  img, w0, b0, slope, versions of w0, b0   the consumer runs the image layer's whole backward:
                                                               dsr_conv_dgrad_first_bwd; deposits (dw0, db0), dx a placeholder
      deposit (consumer, backward)  the result, with the identity (data_ptr, _version, shape) of the dx it returns to autograd
      collect (producer, backward)  the deposit, if `dout` IS that dx.

    The precondition of every kind is that x has exactly one consumer and no hook: autograd then hands the producer the very
    tensor the consumer returned.  Anything summed into it on the way -- a second consumer, a hook -- changes its address or
    its version.  The sums of "bn" are then recomputed by the producer from the complete `dout`; for the other kinds the
    link's contribution cannot be recovered and collect raises.  collect spends the link and drops everything it holds: a
    second backward over a retained graph finds it without an offer and takes the separate launches, whatever the kind.
    (offer starts the link afresh: a forward that is recomputed may reuse it.)"""
    __slots__ = ("kind", "payload", "_deposit", "_dx")
    _SWITCH = {"act": "functional.ACT_LINKS = False", "bn": "DSR_DGRAD_BN_LINK=0 (functional.DGRAD_BN)",
               "ps": "DSR_DGRAD_PS_LINK=0 (functional.DGRAD_PS)", "first2": "DSR_FIRST2_BACKWARD=0 (functional.FIRST2_BACKWARD)"}

    def __init__(self):
        self.kind = self.payload = self._deposit = self._dx = None

    def offer(self, kind, *payload):
        assert kind in self._SWITCH
        self.kind, self.payload, self._deposit, self._dx = kind, payload, None, None

    def deposit(self, dx, result=True):
        if self.kind is None:
            raise RuntimeError("Handover.deposit: the link holds no offer (never made, or spent by an earlier backward pass)")
        self._deposit, self._dx = result, _identity(dx)

    def collect(self, dout):
        kind, got, dx = self.kind, self._deposit, self._dx
        self.kind = self.payload = self._deposit = self._dx = None
        if got is None or dx == _identity(dout):
            return got
        if kind == "bn":
            return None
        raise RuntimeError(
            f"Handover '{kind}': the gradient that reached the producer is not the tensor its consumer returned -- the "
            "activation has a second consumer or a hook, and the part of the backward that went through the link cannot be "
            f"separated from what was added.  Turn the fusion off for such a graph: {self._SWITCH[kind]}")


def _conv_backward(desc, x, dy, wd, need_dx, need_dw, weight_shape, weight=None, addend=None, in_link=None):
    """dx (+ `addend`: the gradient that reaches x along a skip path, summed in the dgrad epilogue where the kernel can; or
    `in_link`, the Handover of the layer that produced x -- "act": its activation's backward mask is folded into the dgrad
    stores, "bn": the dgrad launch also forms its BatchNorm-backward sums -- where the kernel can) and dw."""
    lib = _lib.lib()
    dx = dw = None
    kind = in_link.kind if (in_link is not None and addend is None) else None
    if need_dx:
        dx = torch.empty_like(x)
        if (kind == "bn" and DGRAD_BN and in_link.payload[3] in (ACT_NONE, ACT_LEAKY) and in_link.payload[0].shape == x.shape
                and lib.dsr_conv_dgrad_bn_supported(C.byref(desc))):
            y0, scale0, shift0, act0, slope0 = in_link.payload
            rows = lib.dsr_conv_dgrad_bn_rows(C.byref(desc))
            cp = x.shape[-1]
            part = _partials(rows, 3 * cp, x.device)
            check(_timed("dgrad", desc, lambda: lib.dsr_conv_dgrad_bn(
                C.byref(desc), _ptr(dy), _ptr(wd), _ptr(dx), _ptr(y0), _ptr(scale0), _ptr(shift0), act0, slope0, _ptr(part),
                _stream()), name="conv_dgrad_s2_kernel<bn>"))
            in_link.deposit(dx, (part, rows))
        elif kind == "act" and ACT_LINKS and lib.dsr_conv_dgrad_masked_supported(C.byref(desc)):
            act0, slope0 = in_link.payload
            check(_timed("dgrad", desc, lambda: lib.dsr_conv_dgrad_masked(C.byref(desc), _ptr(dy), _ptr(wd), _ptr(x), act0, slope0,
                                                                            _ptr(dx), _stream())))
            in_link.deposit(dx)
        elif addend is not None and lib.dsr_conv_dgrad_add_supported(C.byref(desc)):
            addend = addend.contiguous()
            check(_timed("dgrad", desc, lambda: lib.dsr_conv_dgrad_add(C.byref(desc), _ptr(dy), _ptr(wd), _ptr(addend), _ptr(dx),
                                                                         _stream()), name="conv_c64_kernel<3>"))
            addend = None
        else:
            wsz = lib.dsr_conv_dgrad_workspace(C.byref(desc))
            ws = torch.empty(max(wsz, 16), dtype=torch.uint8, device=x.device)
            check(_timed("dgrad", desc, lambda: lib.dsr_conv_dgrad(C.byref(desc), _ptr(dy), _ptr(wd), _ptr(dx), _ptr(ws), wsz,
                                                                     _stream())))
    if addend is not None:
        dx = addend if dx is None else dx + addend
    if (need_dw and _wgrad_batch is not None and weight is not None and weight.is_leaf and weight.grad is None
            # (a derived weight -- SpectralNormWeight's -- has a backward node that reads its gradient at once: no placeholder)
            and _wgrad_batch.batchable(weight)                               # (an earlier use returned a real gradient / was launched early)
            and not getattr(weight, "_post_accumulate_grad_hooks", None)      # (a hook would read the gradient at once)
            and lib.dsr_conv_wgrad_batchable(C.byref(desc))):
        return dx, _wgrad_batch.add(weight, desc, x, dy, weight_shape)
    if need_dw:
        dw = torch.empty(weight_shape, dtype=torch.float32, device=x.device)
        wsz = lib.dsr_conv_wgrad_workspace(C.byref(desc))
        ws = torch.empty(wsz, dtype=torch.uint8, device=x.device)
        check(_timed("wgrad", desc, lambda: lib.dsr_conv_wgrad(C.byref(desc), _ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), wsz,
                                                                 _stream())))
        if _wgrad_batch is not None and weight is not None and _wgrad_batch.add_unbatchable(weight, dw):
            dw = None            # joins the batched contribution of the same weight when the block exits
    return dx, dw


def _colsum(dy, c):
    """fp32 [c] column sums of an NHWC tensor (bias gradient)."""
    lib = _lib.lib()
    p = dy.numel() // dy.shape[-1]
    cp = dy.shape[-1]
    blocks, rpb = _reduce_blocks(p)
    part = _partials(blocks, cp, dy.device)
    check(lib.dsr_pw_colsum(_dt(dy), _ptr(dy), p, cp, blocks, rpb, _ptr(part), _stream()))
    out = torch.empty(c, dtype=torch.float32, device=dy.device)
    check(lib.dsr_pw_sum_rows(_ptr(part), blocks, cp, 0, c, 1.0, _ptr(out), 0, 1, _stream()))
    return out


def _fold_bias_prelu(part, blocks, cout, cyp, has_bias, has_prelu):
    """(db, dprelu) of a conv + activation backward from its `blocks` partial rows [bias sums (cyp) | slope sums (cyp)]:
    fp32 [cout] and [1], each None unless asked for."""
    lib = _lib.lib()
    db = dprelu = None
    if has_bias:
        db = torch.empty(cout, dtype=torch.float32, device=part.device)
        check(lib.dsr_pw_sum_rows(_ptr(part), blocks, 2 * cyp, 0, cout, 1.0, _ptr(db), 0, 1, _stream()))
    if has_prelu:
        chan = torch.empty(cyp, dtype=torch.float32, device=part.device)
        check(lib.dsr_pw_sum_rows(_ptr(part), blocks, 2 * cyp, cyp, cyp, 1.0, _ptr(chan), 0, 1, _stream()))
        dprelu = torch.empty(1, dtype=torch.float32, device=part.device)
        check(lib.dsr_pw_sum_rows(_ptr(chan), cyp, 1, 0, 1, 1.0, _ptr(dprelu), 0, 0, _stream()))
    return db, dprelu


# ----------------------------------------------------------------------------- layout edges
class ToNHWC(torch.autograd.Function):
    """fp32 NCHW [N,C,H,W] -> 16-bit NHWC [N,H,W,r8(C)] (pad channels are zero)."""

    @staticmethod
    def forward(ctx, x, dtype):
        _need_gpu(x)
        x = x.contiguous().float()
        n, c, h, w = x.shape
        out = torch.empty((n, h, w, r8(c)), dtype=dtype, device=x.device)
        check(_lib.lib().dsr_pw_nchw_to_nhwc(_dt(out), _ptr(x), _ptr(out), n, c, h, w, r8(c), _stream()))
        ctx.c = c
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        n, h, w, cp = g.shape
        out = torch.empty((n, ctx.c, h, w), dtype=torch.float32, device=g.device)
        check(_lib.lib().dsr_pw_nhwc_to_nchw(_dt(g), _ptr(g), _ptr(out), n, ctx.c, h, w, cp, _stream()))
        return out, None


class ToNCHW(torch.autograd.Function):
    """16-bit NHWC -> fp32 NCHW with the first `c` channels.  `net_output`: this is where a network hands its result back
    (a net that ends without an activation), so its backward is where an ambient loss scale enters (ambient_loss_scale)."""

    @staticmethod
    def forward(ctx, x, c, net_output=False):
        x = x.contiguous()
        n, h, w, cp = x.shape
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        check(_lib.lib().dsr_pw_nhwc_to_nchw(_dt(x), _ptr(x), _ptr(out), n, c, h, w, cp, _stream()))
        ctx.dtype = x.dtype
        ctx.net_output = net_output
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().float()
        if ctx.net_output:
            g = _ambient_scaled(g)
        n, c, h, w = g.shape
        out = torch.empty((n, h, w, r8(c)), dtype=ctx.dtype, device=g.device)
        check(_lib.lib().dsr_pw_nchw_to_nhwc(_dt(out), _ptr(g), _ptr(out), n, c, h, w, r8(c), _stream()))
        return out, None, None


# ----------------------------------------------------------------------------- conv + bias + activation
class ConvAct(torch.autograd.Function):
    """y = act(conv(x, W) + b), optionally stored through PixelShuffle(2).

    generator.py:47-48 (9x9 + PReLU), :30-39 (3x3 64->256 + PixelShuffle + PReLU: a one-parameter
    PReLU commutes with the shuffle permutation), discriminator.py:25-27 (3x3 + LeakyReLU),
    utils/GAN.py:19-57 (VGG 3x3 + ReLU), plain convs (act none).
    Backward derives act' from the stored OUTPUT (the pre-activation is never written to HBM), which identifies the
    branch only for a POSITIVE slope.  A LeakyReLU slope is a host constant and is checked here; a learned PReLU slope
    lives on the device: if it has crossed zero the backward kernel turns every gradient of the launch into NaN (never
    a silently wrong number) and ``check_prelu_slopes(module)`` names the parameter.  ConvBNAct has no such
    restriction (it re-derives the sign from the saved conv output)."""

    @staticmethod
    def forward(ctx, x, weight, bias, prelu, cfg):
        _need_gpu(x)
        if cfg.get("act", ACT_NONE) == ACT_LEAKY and not float(cfg.get("slope", 0.0)) > 0.0:
            raise ValueError(f"ConvAct: LeakyReLU slope {cfg.get('slope', 0.0)} must be > 0 (the activation gradient is "
                             "derived from the stored output)")
        x, desc, oh, ow, wf, wd = _conv_prologue(x, weight, cfg)
        cout = desc.Cout
        ps = bool(cfg.get("pixel_shuffle", False))
        n = x.shape[0]
        if ps:
            y = torch.empty((n, 2 * oh, 2 * ow, r8(cout // 4)), dtype=x.dtype, device=x.device)
        else:
            y = torch.empty((n, oh, ow, r8(cout)), dtype=x.dtype, device=x.device)
        act = cfg.get("act", ACT_NONE)
        ep = Epilogue(act, float(cfg.get("slope", 0.0)), _ptr(prelu), _ptr(bias), None, int(ps), None)
        if not cfg.get("defer", False):
            check(_timed("fwd", desc, lambda: _lib.lib().dsr_conv_fwd(C.byref(desc), _ptr(x), _ptr(wf), C.byref(ep), _ptr(y),
                                                                        _stream()), ep))
        # (defer: nothing is launched here -- the layer that consumes y computes this layer inside its own forward kernel and
        #  fills y only if a backward pass will need it: ConvBNAct whose in_link offers "first2", the discriminator's first two
        #  layers)
        ctx.desc, ctx.cfg, ctx.ps, ctx.act = desc, cfg, ps, act
        ctx.wshape = tuple(weight.shape)
        ctx.weight_ref = weight
        ctx.weight_version = _version(weight)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.bias_version = _version(bias) if bias is not None else None
        out_link = cfg.get("out_link")
        if out_link is not None:
            # what the consumer of y may do of this layer's backward inside its own launch (Handover)
            slope = float(cfg.get("slope", 0.0))
            if cfg.get("defer", False):
                out_link.offer("first2", x, weight, bias, slope, ctx.weight_version, ctx.bias_version)
            elif ps:
                if act == ACT_PRELU and prelu is not None and cout == 256:
                    out_link.offer("ps", prelu.detach())
            elif (prelu is None and act in (ACT_RELU, ACT_LEAKY) and not (ctx.has_bias and ctx.needs_input_grad[2])
                    and (ctx.needs_input_grad[0] or not ctx.needs_input_grad[1])):
                # (a bias gradient needs this layer's own pass over the unmasked gradient; an image layer -- weight gradient and
                #  no input gradient -- applies the mask inside its one-pass backward, dsr_conv_first_bwd)
                out_link.offer("act", act, slope)
        ctx.save_for_backward(x, y, wd, prelu if prelu is not None else torch.empty(0, device=x.device))
        return y

    @staticmethod
    def backward(ctx, dout):
        x, y, wd, prelu = ctx.saved_tensors
        prelu = prelu if prelu.numel() else None
        lib = _lib.lib()
        desc = ctx.desc
        out_link = ctx.cfg.get("out_link")
        kind = out_link.kind if out_link is not None else None
        got = out_link.collect(dout) if out_link is not None else None
        if kind == "first2" and got is not None:
            # the layer on top of this one (ConvBNAct) ran this layer's whole backward inside its own input-gradient kernel
            # (dsr_conv_dgrad_first_bwd) and left the results in the link; `dout` is a placeholder
            return None, got[0], got[1], None, None
        if got is None:
            dout = dout.contiguous()     # (otherwise premasked and contiguous already, or a placeholder: see below)
        cout = desc.Cout
        n = x.shape[0]
        oh, ow = _out_hw(desc)
        cyp = r8(cout)
        need_partial = ctx.has_bias or prelu is not None
        if (not ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and not ctx.ps and prelu is None
                and lib.dsr_conv_first_bwd_supported(C.byref(desc), ctx.act)):
            # first layer on an image (discriminator.py:22): activation mask, bias gradient and weight gradient in ONE
            # pass over dout and y -- g = dout * act'(y) is never materialised
            dw = torch.empty(ctx.wshape, dtype=torch.float32, device=x.device)
            db = torch.empty(cout, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            wsz = lib.dsr_conv_first_bwd_workspace(C.byref(desc))
            ws = torch.empty(wsz, dtype=torch.uint8, device=x.device)
            w0 = getattr(ctx, "weight_ref", None)
            b0 = ctx.bias_ref
            if (FIRST_BWD_RECOMPUTE and w0 is not None and w0.dtype == torch.float32 and w0.is_contiguous()
                    and _version(w0) == ctx.weight_version and (b0 is None or _version(b0) == ctx.bias_version)):
                # the activation output y is not read: the sign of the pre-activation is recomputed inside the pass from the
                # image and the layer's own weight and bias (unchanged since the forward: same versions) -- 1.07 GB less per
                # pass at 512^2
                check(_timed("wgrad", desc, lambda: lib.dsr_conv_first_bwd_recompute(
                    C.byref(desc), _ptr(x), _ptr(dout), _ptr(w0.detach()), _ptr(b0.detach() if b0 is not None else None), ctx.act,
                    float(ctx.cfg.get("slope", 0.0)), _ptr(dw), _ptr(db), _ptr(ws), wsz, _stream()), name="conv_first_bwd_kernel"))
            else:
                check(_timed("wgrad", desc, lambda: lib.dsr_conv_first_bwd(
                    C.byref(desc), _ptr(x), _ptr(dout), _ptr(y), ctx.act, float(ctx.cfg.get("slope", 0.0)), _ptr(dw), _ptr(db),
                    _ptr(ws), wsz, _stream()), name="conv_first_bwd_kernel"))
            return None, dw, db, None, None
        if kind == "ps" and got is not None:
            # the tail's input-gradient launch (dsr_conv_dgrad_ps) already produced the masked, un-shuffled gradient of this
            # layer's conv output and the partial sums; `dout` is a placeholder
            dy, part, blocks = got
            db, dprelu = _fold_bias_prelu(part, blocks, cout, cyp, ctx.has_bias, True)
        elif kind == "act" and got is not None:
            # the consumer of this layer's output already multiplied dout by act'(y): nothing left to do here
            dy = dout
            db = dprelu = None
        elif ctx.act == ACT_NONE and not ctx.ps:
            dy = dout
            db = _colsum(dy, cout) if (ctx.has_bias and ctx.needs_input_grad[2]) else None   # (a frozen trunk's bias: no pass)
            dprelu = None
        else:
            dy = torch.empty((n, oh, ow, cyp), dtype=x.dtype, device=x.device)
            p = n * oh * ow
            blocks, rpb = _reduce_blocks(p)
            part = _partials(blocks, 2 * cyp, x.device) if need_partial else None
            check(lib.dsr_pw_act_bwd(_dt(x), _ptr(dout), _ptr(y), _ptr(dy), n, oh, ow, cyp, y.shape[-1], int(ctx.ps),
                                     ctx.act, float(ctx.cfg.get("slope", 0.0)), _ptr(prelu), blocks, rpb, _ptr(part),
                                     _stream()))
            db, dprelu = _fold_bias_prelu(part, blocks, cout, cyp, ctx.has_bias, prelu is not None)
        dx, dw = _conv_backward(desc, x, dy, wd, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.wshape,
                                 getattr(ctx, "weight_ref", None), in_link=ctx.cfg.get("in_link"))
        return dx, dw, db, dprelu, None


def _first2_backward(ctx, desc, x, dy, wd):
    """discriminator.py:25-29 in a step that needs no image gradient (the discriminator's own update): this layer's input
    gradient and the image layer's whole backward (mask, bias and weight gradient) as one launch, dsr_conv_dgrad_first_bwd --
    the gradient of the 64-channel activation between the two (1.07 GB at 512x512, batch 32) is never written.  Returns the
    placeholder to hand to autograd as that gradient (the image layer's gradients are left in the link its ConvAct node
    reads), or None when the pair does not qualify: then the caller takes the separate launches."""
    link = ctx.cfg.get("in_link")
    if not FIRST2_BACKWARD or link is None or link.kind != "first2" or not ctx.train or not ctx.needs_input_grad[0]:
        return None
    img, w0, b0, slope0, w0_version, b0_version = link.payload
    # (the kernel rebuilds the activation's sign from the live w0 and b0: both must be what the forward used)
    if (img.requires_grad or not w0.requires_grad or w0.dtype != torch.float32 or not w0.is_contiguous()
            or _version(w0) != w0_version or (b0 is not None and (not b0.requires_grad or _version(b0) != b0_version))):
        return None
    lib = _lib.lib()
    d0 = make_desc(img, w0.shape[0], 3, 3, 1, 1, PAD_ZERO, w0.shape[1])
    if not lib.dsr_conv_dgrad_first_bwd_supported(C.byref(d0), C.byref(desc), ACT_LEAKY):
        return None
    dw0 = torch.empty(tuple(w0.shape), dtype=torch.float32, device=x.device)
    db0 = torch.empty(w0.shape[0], dtype=torch.float32, device=x.device) if b0 is not None else None
    wsz = lib.dsr_conv_dgrad_first_bwd_workspace(C.byref(desc))
    ws = torch.empty(wsz, dtype=torch.uint8, device=x.device)
    check(_timed("dgrad", desc, lambda: lib.dsr_conv_dgrad_first_bwd(
        C.byref(d0), C.byref(desc), _ptr(dy), _ptr(wd), _ptr(img), _ptr(w0.detach()), _ptr(b0.detach() if b0 is not None else None),
        ACT_LEAKY, float(slope0), _ptr(dw0), _ptr(db0), _ptr(ws), wsz, _stream()), name="conv_dgrad_s2_kernel<first_bwd>"))
    dx = zero_placeholder(x.shape, x.dtype, x.device)
    link.deposit(dx, (dw0, db0))
    return dx


# ----------------------------------------------------------------------------- the BatchNorm recipe of ConvBNAct and BNAct
def _bn_vectors(cp, dev):
    """Uninitialised (scale, shift, mean, rstd), fp32 [cp] each."""
    return tuple(torch.empty(cp, dtype=torch.float32, device=dev) for _ in range(4))


def _bn_finalize(part, rows, cout, cp, count, gamma, beta, running_mean, running_var, nbt, cfg, vectors):
    """Train mode: `rows` partial rows of per-channel sum / sum of squares over `count` pixels -> the affine map and the batch
    statistics in `vectors` (scale, shift, mean, rstd), and the running statistics advanced like nn.BatchNorm2d's."""
    scale, shift, mean, rstd = vectors
    check(_lib.lib().dsr_pw_bn_finalize(_ptr(part), rows, cp, cout, cp, float(count), _ptr(gamma), _ptr(beta),
                                        _ptr(running_mean), _ptr(running_var), _ptr(nbt), BN_MOMENTUM, BN_EPS,
                                        int(cfg.get("bn_updates", 1)),
                                        _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd), _stream()))
    bump(running_mean)       # rewritten through their raw pointers: whatever is keyed on them (the inference
    bump(running_var)        # affine map ConvBNAct keeps with running_mean) must see a new version


def _bn_eval_affine(gamma, beta, running_mean, running_var, cout, cp, vectors):
    """Eval mode: the fixed affine map of the running statistics into `vectors` (scale, shift, mean, rstd)."""
    scale, shift, mean, rstd = vectors
    check(_lib.lib().dsr_pw_bn_eval_affine(_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), BN_EPS,
                                           cout, cp, _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd), _stream()))


def _bn_act_backward(dout, y, scale, shift, mean, rstd, p, c, cp, act, slope, prelu, train, part_rows=None):
    """Backward of act(BN(y)) over p pixels: (dy, dgamma, dbeta, dprelu).  `part_rows` = (part, rows): the partial sums that
    another launch already formed (Handover "bn"); without it they come from this recipe's own reduce pass."""
    lib = _lib.lib()
    dev, dt = y.device, _dt(y)
    c1 = torch.empty(cp, dtype=torch.float32, device=dev)
    c2 = torch.empty(cp, dtype=torch.float32, device=dev)
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    dprelu = torch.empty(1, dtype=torch.float32, device=dev) if prelu is not None else None
    if part_rows is not None:
        part, blocks = part_rows
    else:
        blocks, rpb = _bn_bwd_blocks(p, act)
        part = _partials(blocks, 3 * cp, dev)
        check(lib.dsr_pw_bn_act_bwd_reduce(dt, _ptr(dout), _ptr(y), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd), p, cp,
                                           blocks, rpb, act, slope, _ptr(prelu), _ptr(part), _stream()))
    check(lib.dsr_pw_bn_bwd_finalize(_ptr(part), blocks, c, cp, float(p), _ptr(mean), _ptr(rstd), _ptr(dgamma), _ptr(dbeta),
                                     _ptr(dprelu), _ptr(c1), _ptr(c2), _stream()))
    dy = torch.empty_like(y)
    check(lib.dsr_pw_bn_act_bwd_apply(dt, _ptr(dout), _ptr(y), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd), _ptr(c1),
                                      _ptr(c2), _ptr(dy), p, cp, act, slope, _ptr(prelu), int(train), _stream()))
    return dy, dgamma, dbeta, dprelu


# ----------------------------------------------------------------------------- conv + BatchNorm + activation (+ residual)
class ConvBNAct(torch.autograd.Function):
    """out = act(BN(conv(x, W) + b)) [+ residual]   (train or eval mode BatchNorm2d).

    generator.py:14-25,71-74 (conv3x3 -> BN -> PReLU | + skip), discriminator.py:14-19
    (conv3x3 s1|s2 -> BN -> LeakyReLU), models/DIP/skip.py:54-88 (reflect conv -> BN -> LeakyReLU).
    The conv epilogue emits per-channel sum / sum-of-squares partial rows from its fp32
    accumulators; a tiny finalize kernel turns them into the affine map and updates the running
    statistics (momentum 0.1, unbiased variance) exactly like nn.BatchNorm2d."""

    @classmethod
    def apply(cls, *args):
        # forward() runs with grad mode off whatever the caller's mode is: note the caller's here ("infer" selects the
        # single-kernel inference epilogue, which saves nothing for a backward pass)
        cfg = dict(args[-1], infer=not torch.is_grad_enabled())
        return super().apply(*args[:-1], cfg)

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, nbt, prelu, residual, cfg):
        x, desc, oh, ow, wf, wd = _conv_prologue(x, weight, cfg)
        lib = _lib.lib()
        cout = desc.Cout
        n = x.shape[0]
        cp = r8(cout)
        train = bool(cfg["train"])
        dev = x.device
        y = torch.empty((n, oh, ow, cp), dtype=x.dtype, device=dev)
        scale, shift, mean, rstd = vectors = _bn_vectors(cp, dev)
        count = n * oh * ow
        in_link = cfg.get("in_link")
        if train and in_link is not None and in_link.kind == "first2":
            # x is the (not yet computed) output of the image layer in front of this one: both convolutions run in ONE kernel
            # that recomputes that activation per tile in LDS (dsr_conv_first2_fwd) and writes it to x only when a backward
            # pass will read it (this layer's weight gradient); the forward itself never reads it back from HBM
            img, w0, b0, slope0 = in_link.payload[:4]
            d0 = make_desc(img, w0.shape[0], 3, 3, 1, 1, PAD_ZERO, w0.shape[1])
            wf0, _ = packed_weights(w0, d0, x.dtype)
            rows = lib.dsr_conv_first2_stats_rows(C.byref(d0))
            part = _partials(rows, 2 * cp, dev)
            keep = not cfg.get("infer", False)
            check(_timed("fwd", desc, lambda: lib.dsr_conv_first2_fwd(
                C.byref(d0), C.byref(desc), _ptr(img), _ptr(wf0), _ptr(b0.detach() if b0 is not None else None), float(slope0),
                _ptr(wf), _ptr(bias), _ptr(x) if keep else None, _ptr(y), _ptr(part), _stream()), name="conv_first2_kernel"))
        elif train:
            rows = lib.dsr_conv_stats_rows(C.byref(desc))
            part = _partials(rows, 2 * cp, dev)
            ep = Epilogue(ACT_NONE, 0.0, None, _ptr(bias), _ptr(part), 0, None)
            check(_timed("fwd", desc, lambda: lib.dsr_conv_fwd(C.byref(desc), _ptr(x), _ptr(wf), C.byref(ep), _ptr(y),
                                                                 _stream()), ep))
        if train:
            _bn_finalize(part, rows, cout, cp, count, gamma, beta, running_mean, running_var, nbt, cfg, vectors)
        else:
            infer = cfg.get("infer", False) and lib.dsr_conv_fwd_affine_supported(C.byref(desc))
            # inference: the affine map of an eval-mode BatchNorm changes only when its four tensors do -- keep it with the
            # running mean, keyed by their version counters (33 launches of ~3 us per x8 forward otherwise)
            # (_version(p) = torch's counter + the counter bump() advances when a HIP launch rewrites p through its raw
            #  pointer -- FusedAdam for gamma / beta, the train-mode _bn_finalize for the running statistics -- + the address)
            key = (_version(gamma), _version(beta), _version(running_mean), _version(running_var), str(dev))
            capturing = torch.cuda.is_current_stream_capturing()
            # a capture never takes the kept map: the graph would replay yesterday's scale / shift whatever the statistics
            # are by then -- inside a graph the affine launch is part of every replay
            hit = getattr(running_mean, "_dsr_affine", None) if (infer and not capturing) else None
            if hit is not None and hit[0] == key:
                scale, shift = hit[1], hit[2]
                if hit[4] != torch.cuda.current_stream(dev).cuda_stream:
                    torch.cuda.current_stream(dev).wait_event(hit[3])      # computed on another stream
            else:
                _bn_eval_affine(gamma, beta, running_mean, running_var, cout, cp, vectors)
                if infer and not capturing:
                    ev = torch.cuda.Event()
                    ev.record()
                    running_mean._dsr_affine = (key, scale, shift, ev, torch.cuda.current_stream(dev).cuda_stream)
            if infer:
                # inference (eval_GAN.py:44,94; called under torch.no_grad(), see apply() below): eval-mode BatchNorm
                # is a fixed per-channel affine map, so it, the activation and the skip connection all ride in the conv
                # epilogue -- one kernel, one pass
                res = residual.contiguous() if residual is not None else None
                ep = Epilogue(cfg.get("act", ACT_NONE), float(cfg.get("slope", 0.0)), _ptr(prelu), _ptr(bias), None, 0,
                              None, _ptr(scale), _ptr(shift), _ptr(res))
                check(_timed("fwd", desc, lambda: lib.dsr_conv_fwd(C.byref(desc), _ptr(x), _ptr(wf), C.byref(ep), _ptr(y),
                                                                     _stream()), ep))
                return (y, x) if cfg.get("carry_input", False) else y
            ep = Epilogue(ACT_NONE, 0.0, None, _ptr(bias), None, 0, None)
            check(_timed("fwd", desc, lambda: lib.dsr_conv_fwd(C.byref(desc), _ptr(x), _ptr(wf), C.byref(ep), _ptr(y),
                                                                 _stream()), ep))
        act = cfg.get("act", ACT_NONE)
        out = torch.empty_like(y)
        res = residual.contiguous() if residual is not None else None
        check(lib.dsr_pw_bn_act_fwd(_dt(x), _ptr(y), _ptr(scale), _ptr(shift), _ptr(res), _ptr(out), count, cp, act,
                                    float(cfg.get("slope", 0.0)), _ptr(prelu), _stream()))
        ctx.desc, ctx.cfg, ctx.act, ctx.train, ctx.count = desc, cfg, act, train, count
        out_link = cfg.get("out_link")
        if out_link is not None and train and residual is None and prelu is None and not cfg.get("infer", False):
            # the layer that consumes `out` may form this layer's BatchNorm-backward sums inside its input-gradient launch
            out_link.offer("bn", y, scale, shift, act, float(cfg.get("slope", 0.0)))
        ctx.wshape = tuple(weight.shape)
        ctx.weight_ref = weight
        ctx.has_res = residual is not None
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, y, wd, scale, shift, mean, rstd,
                              prelu if prelu is not None else torch.empty(0, device=dev))
        if cfg.get("carry_input", False):
            # the input comes back as a second output: a residual block hands THAT to its skip connection, so both gradients
            # of the block input arrive at this node and are summed in its dgrad epilogue (dsr_conv_dgrad_add) instead of by
            # an elementwise pass of autograd's
            return out, x
        return out

    @staticmethod
    def backward(ctx, dout, dcarry=None):
        x, y, wd, scale, shift, mean, rstd, prelu = ctx.saved_tensors
        prelu = prelu if prelu.numel() else None
        desc = ctx.desc
        dout = dout.contiguous()
        cout = desc.Cout
        out_link = ctx.cfg.get("out_link")
        # (a deposit: the launch that produced `dout` -- the next layer's input gradient, dsr_conv_dgrad_bn -- formed the
        #  BatchNorm-backward sums already, and the reduce pass is skipped)
        got = out_link.collect(dout) if out_link is not None else None
        dy, dgamma, dbeta, dprelu = _bn_act_backward(dout, y, scale, shift, mean, rstd, ctx.count, cout, y.shape[-1], ctx.act,
                                                     float(ctx.cfg.get("slope", 0.0)), prelu, ctx.train, got)
        fused = _first2_backward(ctx, desc, x, dy, wd) if dcarry is None else None
        if fused is not None:
            # the input gradient (of the image layer's activation) was consumed where it was formed: autograd gets a
            # placeholder of the right shape, and the image layer's ConvAct node finds its gradients in the link
            dx = fused
            _, dw = _conv_backward(desc, x, dy, wd, False, ctx.needs_input_grad[1], ctx.wshape, getattr(ctx, "weight_ref", None))
        else:
            dx, dw = _conv_backward(desc, x, dy, wd, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.wshape,
                                     getattr(ctx, "weight_ref", None), dcarry, in_link=ctx.cfg.get("in_link"))
        db = None
        if ctx.has_bias and not ctx.train:
            # a bias in front of a train-mode BatchNorm has an analytically zero gradient (the reference holds ~1e-9
            # rounding noise there): no gradient is produced for it at all -- Adam leaves such a parameter exactly where
            # a zero gradient would (m = v = 0 => no update), and 47 zero-fill launches per GAN step disappear.
            # In eval mode it is the column sum of dy.
            db = _colsum(dy, cout)
        dres = dout if ctx.has_res else None
        return dx, dw, db, dgamma, dbeta, None, None, None, dprelu, dres, None


# ----------------------------------------------------------------------------- last layer: conv + act -> fp32 NCHW
class ConvOutNCHW(torch.autograd.Function):
    """fp32 NCHW output of the last conv (+Tanh: generator.py:78-80; +Sigmoid: models/DIP/skip.py:92-94)."""

    @staticmethod
    def forward(ctx, x, weight, bias, cfg):
        x, desc, oh, ow, wf, wd = _conv_prologue(x, weight, cfg)
        out = torch.empty((x.shape[0], desc.Cout, oh, ow), dtype=torch.float32, device=x.device)
        act = cfg.get("act", ACT_NONE)
        ep = Epilogue(act, 0.0, None, _ptr(bias), None, 0, _ptr(out))
        check(_timed("fwd", desc, lambda: _lib.lib().dsr_conv_fwd(C.byref(desc), _ptr(x), _ptr(wf), C.byref(ep), None,
                                                                    _stream()), ep))
        ctx.desc, ctx.act = desc, act
        ctx.in_link = cfg.get("in_link")
        ctx.wshape = tuple(weight.shape)
        ctx.weight_ref = weight
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, out, wd)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, wd = ctx.saved_tensors
        desc = ctx.desc
        dout = _ambient_scaled(dout.contiguous().float())
        n, c, h, w = out.shape
        dy = torch.empty((n, h, w, r8(c)), dtype=x.dtype, device=x.device)
        check(_lib.lib().dsr_pw_act_bwd_nchw(_dt(x), _ptr(dout), _ptr(out), _ptr(dy), n, c, h, w, r8(c), ctx.act,
                                             _stream()))
        lib = _lib.lib()
        link = ctx.in_link
        if (link is not None and link.kind == "ps" and DGRAD_PS and ctx.needs_input_grad[0]
                and lib.dsr_conv_dgrad_ps_supported(C.byref(desc))):
            # x is PReLU(PixelShuffle(conv)) (generator.py:37-39 in front of :78): that activation's backward rides in this
            # layer's input-gradient launch (dsr_conv_dgrad_ps) -- the 64-channel gradient at the high resolution is never
            # written; the shuffle conv's node finds the un-shuffled, masked gradient and the partial sums in the link
            n_, h_, w_, _ = x.shape
            rows = lib.dsr_conv_dgrad_ps_rows(C.byref(desc))
            dyu = torch.empty((n_, h_ // 2, w_ // 2, 256), dtype=x.dtype, device=x.device)
            part = _partials(rows, 2 * 256, x.device)
            check(_timed("dgrad", desc, lambda: lib.dsr_conv_dgrad_ps(C.byref(desc), _ptr(dy), _ptr(wd), _ptr(x), _ptr(link.payload[0]),
                                                                       _ptr(dyu), _ptr(part), _stream()),
                         name="conv_dgrad_toeplitz9_kernel<ps>"))
            dx = zero_placeholder(x.shape, x.dtype, x.device)
            link.deposit(dx, (dyu, part, rows))
            _, dw = _conv_backward(desc, x, dy, wd, False, ctx.needs_input_grad[1], ctx.wshape, getattr(ctx, "weight_ref", None))
        else:
            dx, dw = _conv_backward(desc, x, dy, wd, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.wshape,
                                     getattr(ctx, "weight_ref", None))
        db = _colsum(dy, c) if ctx.has_bias else None
        return dx, dw, db, None


# ----------------------------------------------------------------------------- losses
def axpby(x, y=None, a=1.0, b=1.0, g=None):
    """(a * x + b * y) * g on fp32 tensors (y optional, g an optional 0-dim / 1-element device tensor): dsr_pw_axpby_f32."""
    x = x.contiguous()
    out = torch.empty_like(x)
    if y is not None:
        y = y.contiguous()
        assert y.shape == x.shape and y.dtype == torch.float32
    if g is not None:
        g = g.contiguous().float()
    check(_lib.lib().dsr_pw_axpby_f32(_ptr(x), _ptr(y), float(a), float(b), _ptr(g), _ptr(out), x.numel(), _stream()))
    return out


class DiffLoss(torch.autograd.Function):
    """mean |a-b| (mode 0, BASELINE config 2) or mean (a-b)^2 (mode 1, nn.MSELoss: DIP.py:26,65;
    utils/GAN.py:74,90) over fp32 tensors.  Both arguments are differentiable (nn.MSELoss / nn.L1Loss are):
    d/d target = - d/d pred."""

    @staticmethod
    def forward(ctx, pred, target, mode):
        _need_gpu(pred)
        pred = pred.contiguous().float()
        target = target.contiguous().float()
        if pred.shape != target.shape:
            raise RuntimeError(f"loss operands differ in shape: {tuple(pred.shape)} vs {tuple(target.shape)}")
        n = pred.numel()
        blocks = max(1, min(1024, (n + 1023) // 1024))
        part = torch.empty(blocks, dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        lib = _lib.lib()
        check(lib.dsr_pw_diff_loss(_ptr(pred), _ptr(target), _ptr(grad), n, mode, _ptr(part), blocks, _stream()))
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        check(lib.dsr_pw_sum_rows(_ptr(part), blocks, 1, 0, 1, 1.0 / n, _ptr(loss), 0, 0, _stream()))
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        gp = axpby(grad, None, 1.0, 0.0, g) if ctx.needs_input_grad[0] else None
        gt = axpby(grad, None, -1.0, 0.0, g) if ctx.needs_input_grad[1] else None
        return gp, gt, None


def l1_loss(pred, target):
    return DiffLoss.apply(pred, target, 0)


def mse_loss(pred, target):
    return DiffLoss.apply(pred, target, 1)


class BCEConst(torch.autograd.Function):
    """nn.BCELoss()(p, full_like(p, target)) with the log clamp at -100 (utils/GAN.py:96-105)."""

    @staticmethod
    def forward(ctx, p, target):
        _need_gpu(p)
        p = p.contiguous().float()
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        check(_lib.lib().dsr_pw_bce_const(_ptr(p), p.numel(), float(target), _ptr(loss), _ptr(grad), 0, _stream()))
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return axpby(grad, None, 1.0, 0.0, g), None


def bce_const(p, target):
    return BCEConst.apply(p, target)


_GAN_KINDS = {"vanilla": _lib.GAN_VANILLA, "lsgan": _lib.GAN_LSGAN, "hinge": _lib.GAN_HINGE}


class GanLoss(torch.autograd.Function):
    """BasicSR's GANLoss on logits against a constant label, mean over all elements (dsr_gan_loss): one pass writes the
    per-element gradient and the block partials, a fixed-order fold makes the mean; nothing is read on the host."""

    @staticmethod
    def forward(ctx, logits, target_is_real, kind, is_disc):
        _need_gpu(logits)
        x = logits.contiguous().float()
        n = x.numel()
        if n == 0:
            raise ValueError("gan_loss: empty logits")
        lib = _lib.lib()
        part = torch.empty(lib.dsr_gan_loss_blocks(n), dtype=torch.float64, device=x.device)
        grad = torch.empty_like(x)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        check(lib.dsr_gan_loss(_ptr(x), n, kind, int(bool(target_is_real)), int(bool(is_disc)), _ptr(grad), _ptr(part),
                               _ptr(loss), _stream()))
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return axpby(grad, None, 1.0, 0.0, g), None, None, None


def gan_loss(logits, target_is_real, kind="vanilla", is_disc=False):
    """GANLoss(gan_type=kind)(logits, target_is_real, is_disc) of BasicSR, unweighted: 'vanilla' = BCEWithLogits against a
    constant 1 / 0, 'lsgan' = (x - t)^2, 'hinge' = relu(1 -+ x) for the discriminator and -x for the generator."""
    if kind not in _GAN_KINDS:
        raise ValueError(f"gan_loss: kind must be one of {sorted(_GAN_KINDS)}, got {kind!r}")
    return GanLoss.apply(logits, target_is_real, _GAN_KINDS[kind], is_disc)


class RelGanLoss(torch.autograd.Function):
    """The relativistic average GAN term of ESRGAN (dsr_rel_gan_loss): gan_loss(pred - mean(other)), with the mean, the loss and
    both gradients formed by fixed-order sums on the device.  A gradient is written only for the operand that requires one:
    grad_pred in the element pass, grad_other (one value for all its elements) by a broadcast store."""

    @staticmethod
    def forward(ctx, pred, other, target_is_real, kind, is_disc):
        _need_gpu(pred)
        _need_gpu(other)
        x = pred.contiguous().float()
        o = other.contiguous().float()
        n, m = x.numel(), o.numel()
        if n == 0 or m == 0:
            raise ValueError("relativistic_gan_loss: empty logits")
        lib = _lib.lib()
        ws = torch.empty(lib.dsr_rel_gan_loss_workspace(n, m) // 8, dtype=torch.float64, device=x.device)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        go = torch.empty_like(o) if ctx.needs_input_grad[1] else None
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        check(lib.dsr_rel_gan_loss(_ptr(x), n, _ptr(o), m, kind, int(bool(target_is_real)), int(bool(is_disc)), _ptr(gx),
                                   _ptr(go), _ptr(ws), _ptr(loss), _stream()))
        ctx.save_for_backward(gx, go)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        gx, go = ctx.saved_tensors
        return (axpby(gx, None, 1.0, 0.0, g) if gx is not None else None,
                axpby(go, None, 1.0, 0.0, g) if go is not None else None, None, None, None)


def relativistic_gan_loss(pred, other, target_is_real, kind="vanilla", is_disc=False):
    """BasicSR's GANLoss(gan_type=kind)(pred - mean(other), target_is_real, is_disc), unweighted: the relativistic average
    form of ESRGAN.  `pred` and `other` are logits of any shapes (their sizes are independent); the gradient goes to whichever
    of them requires one.  Returns an fp32 scalar on the device."""
    if kind not in _GAN_KINDS:
        raise ValueError(f"relativistic_gan_loss: kind must be one of {sorted(_GAN_KINDS)}, got {kind!r}")
    return RelGanLoss.apply(pred, other, target_is_real, _GAN_KINDS[kind], is_disc)


# ----------------------------------------------------------------------------- LDL artifact-map loss
def _ldl_forward(pred, target, pred_ema, ksize, want_map):
    """The two forward launches of csrc/ldl.hip: (x, gt, ws, loss, map or None)."""
    for t in (pred, target, pred_ema):
        _need_gpu(t)
        if t.dtype != torch.float32:
            raise TypeError(f"ldl_loss takes fp32 tensors, got {t.dtype}")
    if pred.dim() != 4 or pred.shape != target.shape or pred.shape != pred_ema.shape:
        raise RuntimeError(f"ldl_loss operands must be [N, C, H, W] of one shape: {tuple(pred.shape)}, {tuple(target.shape)}, "
                           f"{tuple(pred_ema.shape)}")
    if isinstance(ksize, bool) or not isinstance(ksize, int) or ksize < 3 or ksize > 11 or ksize % 2 == 0:
        raise ValueError(f"ldl_loss: ksize must be an odd int in 3..11, got {ksize!r}")
    n, c, h, w = pred.shape
    if h <= ksize // 2 or w <= ksize // 2:
        raise ValueError(f"ldl_loss: a {h}x{w} image cannot be reflect-padded by {ksize // 2}")
    x, gt, e = pred.detach().contiguous(), target.detach().contiguous(), pred_ema.detach().contiguous()
    lib = _lib.lib()
    nbytes = lib.dsr_ldl_workspace(n, c, h, w, ksize)
    if nbytes == 0:
        raise ValueError(f"ldl_loss: shape {tuple(pred.shape)} is empty or has 2^31 elements or more")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    amap = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device) if want_map else None
    check(lib.dsr_ldl_fwd(_ptr(x), _ptr(gt), _ptr(e), n, c, h, w, ksize, _ptr(ws), _ptr(loss), _ptr(amap), _stream()))
    return x, gt, ws, loss, amap


class LdlLoss(torch.autograd.Function):
    """The LDL artifact-map term (dsr_ldl_fwd / dsr_ldl_bwd, csrc/ldl.hip): mean |w pred - w target| with the refined artifact
    map w of ldl_artifact_map.  Two launches forward, one backward; the backward reads the incoming gradient on the device.
    Gradient for `pred` only.  Like DiffLoss it has nothing to do under an ambient loss scale: the scale enters the backward pass
    at the net's output, after this op."""

    @staticmethod
    def forward(ctx, pred, target, pred_ema, ksize, detach_weight):
        x, gt, ws, loss, _ = _ldl_forward(pred, target, pred_ema, ksize, False)
        ctx.save_for_backward(x, gt, ws)
        ctx.ksize, ctx.detach_weight = ksize, bool(detach_weight)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        x, gt, ws = ctx.saved_tensors
        n, c, h, w = x.shape
        g = g.reshape(1).float().contiguous()
        dx = torch.empty_like(x)
        check(_lib.lib().dsr_ldl_bwd(_ptr(x), _ptr(gt), _ptr(ws), _ptr(g), n, c, h, w, ctx.ksize, int(ctx.detach_weight), _ptr(dx),
                                     _stream()))
        return dx, None, None, None, None


def ldl_loss(pred, target, pred_ema, ksize=7, detach_weight=False):
    """BasicSR's LDL term (ldl_opt; "Details or Artifacts", CVPR 2022), unweighted: L1(w * pred, w * target) with
    w = get_refined_artifact_map(target, pred, pred_ema, ksize).  fp32 [N, C, H, W] operands on the device; returns an fp32
    scalar.  ``detach_weight=False`` (BasicSR's behaviour) lets the gradient flow through the map as well; ``True`` treats the
    map as a constant.  Where an image's residual is constant (its map is all zero) the image adds 0 to the loss and its
    gradient is 0, where torch's own autograd gives 0 * inf = NaN.  Parity with BasicSR is unpinned (tests/ldl_ref.py)."""
    return LdlLoss.apply(pred, target, pred_ema, ksize, detach_weight)


def ldl_artifact_map(pred, target, pred_ema, ksize=7):
    """BasicSR's get_refined_artifact_map(target, pred, pred_ema, ksize), without a gradient: [N, 1, H, W] fp32,
    var(r[n])^(1/5) * (the k x k local variance of r = sum_c |target - pred|), zero where r < sum_c |target - pred_ema|."""
    with torch.no_grad():
        return _ldl_forward(pred, target, pred_ema, ksize, True)[4]


# ----------------------------------------------------------------------------- spectral normalisation
SN_EPS = 1e-12           # torch.nn.utils.spectral_norm's default
_sn_pending = {}         # id(weight_orig) -> results of a group launch that SpectralNormWeight.forward picks up


def _sn_check(weight, u, v):
    _need_gpu(weight)
    cout = weight.shape[0]
    k = weight.numel() // max(cout, 1)
    for name, t, n in (("weight_orig", weight, cout * k), ("u", u, cout), ("v", v, k)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or t.device != weight.device or n == 0:
            raise ValueError(f"spectral norm: {name} must be a contiguous fp32 tensor of {n} elements beside the weight, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")
    return cout, k


def _sn_forward(weights, us, vs, training):
    """W_sn (a new tensor per weight) and sigma ([len] fp32) of a list of layers, 64 per launch group; in train mode u and v
    advance in place."""
    lib = _lib.lib()
    outs, sigmas = [], []
    for i0 in range(0, len(weights), 64):
        ws, uu, vv = weights[i0:i0 + 64], us[i0:i0 + 64], vs[i0:i0 + 64]
        n = len(ws)
        shapes = [_sn_check(w, u, v) for w, u, v in zip(ws, uu, vv)]
        ci, ki = (C.c_int * n)(*[s[0] for s in shapes]), (C.c_int * n)(*[s[1] for s in shapes])
        out = [torch.empty_like(w) for w in ws]
        sigma = torch.empty(n, dtype=torch.float32, device=ws[0].device)
        nbytes = lib.dsr_spectral_norm_workspace(n, ci, ki)
        work = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=ws[0].device)
        check(lib.dsr_spectral_norm_fwd(n, _lib.ptr_table(ws), _lib.ptr_table(uu), _lib.ptr_table(vv), ci, ki, int(bool(training)),
                                        SN_EPS, _ptr(sigma), _lib.ptr_table(out), _ptr(work), nbytes, _stream()))
        outs += out
        sigmas += [sigma[j:j + 1] for j in range(n)]
    return outs, sigmas


class SpectralNormWeight(torch.autograd.Function):
    """W_sn = weight_orig / sigma of torch.nn.utils.spectral_norm (one power iteration, eps 1e-12; csrc/spectral_norm.hip).
    In train mode `u` and `v` advance in place; in eval mode they are only read.  The backward treats the iterated vectors
    as constants, as torch does: dW = (G - <G, W_sn> u v^T) / sigma, on copies of u and v taken by this forward (a later
    forward may move them on before this one's backward runs).  A frozen weight_orig has no backward node at all.  The
    result is marked as a derived weight: its packed conv images are not cached (packed_weights) and its weight gradient
    never joins a batched_wgrad group (_conv_backward)."""

    @staticmethod
    def forward(ctx, weight_orig, u, v, training):
        pend = _sn_pending.pop(id(weight_orig), None)
        need = ctx.needs_input_grad[0]
        if pend is None:
            w = weight_orig.detach()
            (w_sn,), (sigma,) = _sn_forward([w], [u], [v], training)
            us, vs = (u.clone(), v.clone()) if need else (None, None)
        else:
            w_sn, sigma, us, vs = pend
        if need:
            ctx.save_for_backward(w_sn, sigma, us, vs)
        w_sn._dsr_derived = True
        return w_sn

    @staticmethod
    def backward(ctx, g):
        w_sn, sigma, u, v = ctx.saved_tensors
        lib = _lib.lib()
        g = g.contiguous().float()
        cout = w_sn.shape[0]
        ci, ki = (C.c_int * 1)(cout), (C.c_int * 1)(w_sn.numel() // cout)
        dw = torch.empty_like(w_sn)
        nbytes = lib.dsr_spectral_norm_bwd_workspace(1, ci, ki)
        work = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=g.device)
        check(lib.dsr_spectral_norm_bwd(1, _lib.ptr_table([g]), _lib.ptr_table([w_sn]), _lib.ptr_table([u]), _lib.ptr_table([v]),
                                        ci, ki, _ptr(sigma), _lib.ptr_table([dw]), _ptr(work), nbytes, _stream()))
        return dw, None, None, None


def spectral_norm_weights(weights, us, vs, training):
    """[SpectralNormWeight(w, u, v, training) for every layer], with the iterations of all layers in ONE launch group
    (dsr_spectral_norm_fwd takes 64 layers a call) instead of one group per layer."""
    weights, us, vs = list(weights), list(us), list(vs)
    outs, sigmas = _sn_forward([w.detach() for w in weights], us, vs, training)
    saved = {}
    need = [i for i, w in enumerate(weights) if w.requires_grad and torch.is_grad_enabled()]
    if need:
        # this forward's vectors for the backward passes: one copy launch for all of them
        flat = torch.cat([us[i].reshape(-1) for i in need] + [vs[i].reshape(-1) for i in need])
        sizes = [us[i].numel() for i in need] + [vs[i].numel() for i in need]
        parts = flat.split(sizes)
        for j, i in enumerate(need):
            saved[i] = (parts[j], parts[len(need) + j])
    res = []
    for i, w in enumerate(weights):
        _sn_pending[id(w)] = (outs[i], sigmas[i]) + saved.get(i, (None, None))
        try:
            w_sn = SpectralNormWeight.apply(w, us[i], vs[i], training)
        finally:
            _sn_pending.pop(id(w), None)
        w_sn._dsr_derived = True
        res.append(w_sn)
    return res


class AddScalars(torch.autograd.Function):
    """a + b for two scalar losses (utils/GAN.py:105 BCE(real,1) + BCE(fake,0); :122 content + adversarial)."""

    @staticmethod
    def forward(ctx, a, b):
        return axpby(a.reshape(1), b.reshape(1), 1.0, 1.0).reshape(())

    @staticmethod
    def backward(ctx, g):
        return g, g


def add_losses(a, b):
    return AddScalars.apply(a, b)


class OneMinus(torch.autograd.Function):
    """1 - x for a scalar similarity (1 - SSIM, 1 - MS-SSIM as a loss term)."""

    @staticmethod
    def forward(ctx, x):
        one = torch.ones(1, dtype=torch.float32, device=x.device)
        return axpby(x.reshape(1).float(), one, -1.0, 1.0).reshape(())

    @staticmethod
    def backward(ctx, g):
        return axpby(g.reshape(1), None, -1.0, 0.0).reshape(())


def one_minus(x):
    return OneMinus.apply(x)


class ScaleLoss(torch.autograd.Function):
    """s * loss for a host constant s (the static loss scale of the fp16 DIP path)."""

    @staticmethod
    def forward(ctx, loss, s):
        ctx.s = float(s)
        return axpby(loss.reshape(1), None, ctx.s, 0.0).reshape(())

    @staticmethod
    def backward(ctx, g):
        return axpby(g.reshape(1), None, ctx.s, 0.0).reshape(()), None


def scale_loss(loss, s):
    return loss if s == 1.0 else ScaleLoss.apply(loss, s)


class ScaleLossDevice(torch.autograd.Function):
    """scale[0] * loss for a one-element device tensor (optim.DynamicLossScaler): nothing is read on the host.  Backward
    reads the live tensor, which is correct because the scaler's update() runs after backward()."""

    @staticmethod
    def forward(ctx, loss, scale):
        ctx.scale = scale
        return axpby(loss.reshape(1), None, 1.0, 0.0, scale).reshape(())

    @staticmethod
    def backward(ctx, g):
        return axpby(g.reshape(1), None, 1.0, 0.0, ctx.scale).reshape(()), None


# ----------------------------------------------------------------------------- feature-space loss taps
def _content_forward(f, t, p, cp, mode, want_relu, count):
    """The content term of a tap: (x_next, value) with value = sum |f - t| or (f - t)^2 over the p x cp map, divided by
    `count`; x_next = max(f, 0), a new tensor written by the same pass, when want_relu and None otherwise."""
    lib = _lib.lib()
    blocks = lib.dsr_featloss_blocks(p)
    part = torch.empty(max(blocks, 1), dtype=torch.float32, device=f.device)
    x_next = torch.empty_like(f) if want_relu else None
    check(lib.dsr_featloss_tap_fwd(_dt(f), _ptr(f), _ptr(t), _ptr(x_next), p, cp, mode, _ptr(part), _stream()))
    value = torch.empty(1, dtype=torch.float32, device=f.device)
    check(lib.dsr_featloss_fold(_ptr(part), blocks, float(count), _ptr(value), _stream()))
    return x_next, value


def _scalar_grad(g, device):
    """The gradient of a one-element value as the contiguous fp32 [1] tensor the backward launches read; zeros for None."""
    return torch.zeros(1, dtype=torch.float32, device=device) if g is None else g.reshape(1).contiguous().float()


class FeatureTap(torch.autograd.Function):
    """One tap of a feature-space loss on the 16-bit NHWC map where it lives (csrc/featloss.hip).

    forward(f, t, mode, want_relu, c=None) -> (x_next, value): value = mean |f - t| (mode FEAT_L1) or mean (f - t)^2
    (FEAT_MSE) over the N * c * H * W real elements (c defaults to the padded channel count; pad channels are zero in both
    maps), a 1-element fp32 tensor.  want_relu: f is a PRE-activation map -- x_next is a new tensor max(f, 0), written by the
    same pass, for the next layer; otherwise x_next is f itself and nothing is written.  Whatever consumes the map next must
    consume x_next: the tap is then f's only consumer in the graph and its backward, ONE launch with one rounding per element,
    adds the gradient arriving through x_next (times the ReLU mask when want_relu) to the tap's own term.  Either incoming
    gradient may be None (the deepest tap has no next layer).  t gets no gradient."""

    @staticmethod
    def forward(ctx, f, t, mode, want_relu, c=None):
        _need_gpu(f)
        if mode not in (FEAT_L1, FEAT_MSE):
            raise ValueError(f"FeatureTap: mode {mode!r} is neither FEAT_L1 nor FEAT_MSE")
        if f.dim() != 4 or f.shape != t.shape or f.dtype != t.dtype:
            raise RuntimeError(f"FeatureTap: maps differ: {tuple(f.shape)} {f.dtype} vs {tuple(t.shape)} {t.dtype}")
        f, t = f.contiguous(), t.contiguous()
        n, h, w, cp = f.shape
        p = n * h * w
        count = p * (cp if c is None else int(c))
        x_next, value = _content_forward(f, t, p, cp, mode, want_relu, count)
        ctx.mode, ctx.masked, ctx.coef, ctx.pc = mode, bool(want_relu), 1.0 / count, (p, cp)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(f, t)
        return (x_next if want_relu else f), value

    @staticmethod
    def backward(ctx, d_next, g_value):
        f, t = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (d_next is None and g_value is None):
            return None, None, None, None, None
        if g_value is None and not ctx.masked:
            return d_next, None, None, None, None
        g = _scalar_grad(g_value, f.device)      # (None: only the mask is left to apply)
        if d_next is not None:
            d_next = d_next.contiguous()
        p, cp = ctx.pc
        df = torch.empty_like(f)
        check(_lib.lib().dsr_featloss_tap_bwd(_dt(f), _ptr(f), _ptr(t), _ptr(d_next), _ptr(g), ctx.coef, ctx.mode,
                                              int(ctx.masked), _ptr(df), p, cp, _stream()))
        return df, None, None, None, None


def _gram(x, c):
    n, h, w, cp = x.shape
    lib = _lib.lib()
    ws = torch.empty(max(lib.dsr_gram_workspace(n, h * w, cp), 1), dtype=torch.float32, device=x.device)
    gram = torch.empty((n, c, c), dtype=torch.float32, device=x.device)
    check(lib.dsr_gram_fwd(_dt(x), _ptr(x), n, h * w, c, cp, 1.0 / (c * h * w), _ptr(ws), _ptr(gram), _stream()))
    return gram


def gram16(x, c):
    """Gram matrices of a 16-bit NHWC map, no gradient: fp32 [N, c, c], gram[n][i][j] = sum_p x[n][p][i] x[n][p][j] / (c H W) over
    the c real channels (dsr_gram_fwd).  What FeatureStyleTap takes as ``gram_t`` for the target."""
    _need_gpu(x)
    if x.dim() != 4 or not 1 <= int(c) <= x.shape[3]:
        raise ValueError(f"gram16: an NHWC map and 1 <= c <= Cp, got {tuple(x.shape)} and c = {c!r}")
    return _gram(x.detach().contiguous(), int(c))


class FeatureStyleTap(torch.autograd.Function):
    """FeatureTap with the style (Gram-matrix) term on the same map (csrc/featstyle.hip).

    forward(f, t, gram_t, mode, want_relu, c, with_content) -> (x_next, content_value, style_value).  style_value is the mean
    of |G - gram_t| (FEAT_L1) or (G - gram_t)^2 (FEAT_MSE) over the N c c entries of G = gram16(f, c); content_value is
    FeatureTap's value when with_content is set and None otherwise (t may then be None: no content launch runs).  x_next and
    the single-consumer contract are FeatureTap's.  The backward is ONE launch with one rounding per element: the gradient
    arriving through x_next (masked when want_relu), the content term and the style term, a per-image GEMM of f with the
    16-bit order-one matrix that the forward left, every scalar factor applied in fp32 in its epilogue.  t and gram_t get no
    gradient."""

    @staticmethod
    def forward(ctx, f, t, gram_t, mode, want_relu, c, with_content):
        _need_gpu(f)
        if mode not in (FEAT_L1, FEAT_MSE):
            raise ValueError(f"FeatureStyleTap: mode {mode!r} is neither FEAT_L1 nor FEAT_MSE")
        if f.dim() != 4:
            raise RuntimeError(f"FeatureStyleTap: the map is NHWC, got {tuple(f.shape)}")
        f = f.contiguous()
        n, h, w, cp = f.shape
        c = int(c)
        p = n * h * w
        if gram_t.shape != (n, c, c) or gram_t.dtype != torch.float32:
            raise RuntimeError(f"FeatureStyleTap: gram_t must be fp32 {(n, c, c)}, got {gram_t.dtype} {tuple(gram_t.shape)}")
        gram_t = gram_t.contiguous()
        lib = _lib.lib()
        content, x_next = None, None
        if with_content:
            if t is None or f.shape != t.shape or f.dtype != t.dtype:
                raise RuntimeError("FeatureStyleTap: with_content needs a target map of f's shape and dtype")
            t = t.contiguous()
            x_next, content = _content_forward(f, t, p, cp, mode, want_relu, p * c)
        else:
            t = None
            if want_relu:
                x_next = torch.empty_like(f)
                check(lib.dsr_featloss_relu(_dt(f), _ptr(f), _ptr(x_next), p, cp, _stream()))
        gram = _gram(f, c)
        sums = torch.empty(_lib.GRAM_LOSS_PARTIALS * n, dtype=torch.float64, device=f.device)
        style = torch.empty(1, dtype=torch.float32, device=f.device)
        s16 = torch.empty((n, cp, cp), dtype=f.dtype, device=f.device)
        s_scale = torch.empty(n, dtype=torch.float32, device=f.device)
        check(lib.dsr_gram_loss(_dt(f), _ptr(gram), _ptr(gram_t), n, c, cp, mode, _ptr(sums), _ptr(style), _ptr(s16), _ptr(s_scale),
                                _stream()))
        # d value / d f = [2 for MSE] * (D + D^T) f * scale / (N c c), D symmetric because both Gram matrices are
        ctx.coef_style = (2.0 if mode == FEAT_L1 else 4.0) / (c * h * w) / (n * c * c)
        ctx.mode, ctx.masked, ctx.coef, ctx.dims = mode, bool(want_relu), 1.0 / (p * c), (n, h * w, cp)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(f, t, s16, s_scale)
        return (x_next if want_relu else f), content, style

    @staticmethod
    def backward(ctx, d_next, g_content, g_style):
        f, t, s16, s_scale = ctx.saved_tensors
        none = (None,) * 7
        if not ctx.needs_input_grad[0] or (d_next is None and g_content is None and g_style is None):
            return none
        if g_content is None and g_style is None and not ctx.masked:
            return (d_next,) + none[1:]
        gs = _scalar_grad(g_style, f.device)
        gc = None if t is None else _scalar_grad(g_content, f.device)
        if d_next is not None:
            d_next = d_next.contiguous()
        n, hw, cp = ctx.dims
        df = torch.empty_like(f)
        check(_lib.lib().dsr_featstyle_tap_bwd(_dt(f), _ptr(f), _ptr(t), _ptr(d_next), _ptr(gc), ctx.coef, ctx.mode, int(ctx.masked),
                                               _ptr(s16), _ptr(s_scale), _ptr(gs), ctx.coef_style, _ptr(df), n, hw, cp, _stream()))
        return (df,) + none[1:]


class WeightedSum(torch.autograd.Function):
    """sum_k w_k * v_k over one-element device scalars with host weights, one launch each way (dsr_featloss_combine): the
    weighted sum of a multi-tap loss without a chain of scale_loss / add_losses launches.  forward(weights, *values)."""

    @staticmethod
    def forward(ctx, weights, *values):
        k = len(values)
        vals = [v.reshape(1).contiguous().float() for v in values]
        out = torch.empty(1, dtype=torch.float32, device=vals[0].device)
        ctx.w = (C.c_float * k)(*[float(w) for w in weights])
        check(_lib.lib().dsr_featloss_combine(k, (C.c_void_p * k)(*[v.data_ptr() for v in vals]), ctx.w, _ptr(out), _stream()))
        ctx.shapes = [tuple(v.shape) for v in values]
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        k = len(ctx.shapes)
        g = g.reshape(1).contiguous().float()
        gout = torch.empty(k, dtype=torch.float32, device=g.device)
        check(_lib.lib().dsr_featloss_combine_bwd(k, ctx.w, _ptr(g), _ptr(gout), _stream()))
        return (None,) + tuple(gout[i:i + 1].reshape(s) for i, s in enumerate(ctx.shapes))


def weighted_sum(values, weights):
    if len(values) != len(weights) or not values:
        raise ValueError("weighted_sum: one weight per value, at least one")
    return WeightedSum.apply(tuple(float(w) for w in weights), *values)


def relu16(x):
    """max(x, 0) on a 16-bit NHWC map, no gradient (the target's trunk behind a pre-activation tap): dsr_featloss_relu."""
    x = x.detach().contiguous()
    n, h, w, cp = x.shape
    out = torch.empty_like(x)
    check(_lib.lib().dsr_featloss_relu(_dt(x), _ptr(x), _ptr(out), n * h * w, cp, _stream()))
    return out


_ambient_scale = None    # the open ambient_loss_scale context's device scalar (per process, like _wgrad_batch)


class ambient_loss_scale:
    """While open, the backward of a network's fp32 output op (ConvOutNCHW; ToNCHW where a net ends without an activation)
    multiplies the incoming gradient by scale[0] before it is rounded to 16 bits.  For callers whose loss this package
    never sees (utils.DIP.optimize: the closure calls backward() itself); everything downstream is then identical to a
    scaled loss, because a power of two commutes with the fp32 arithmetic in front of that op.  `scale`: a one-element
    fp32 device tensor, or None (no-op)."""

    def __init__(self, scale):
        self.scale = scale

    def __enter__(self):
        global _ambient_scale
        self.prev, _ambient_scale = _ambient_scale, self.scale
        return self

    def __exit__(self, *exc):
        global _ambient_scale
        _ambient_scale = self.prev
        return False


def _ambient_scaled(g):
    """The fp32 gradient entering 16-bit storage, times the ambient loss scale when one is set."""
    return g if _ambient_scale is None else axpby(g, None, 1.0, 0.0, _ambient_scale)


# ----------------------------------------------------------------------------- discriminator dense head
_shadow_cache = {}


def shadow16(weight, dtype):
    """16-bit copy of an fp32 matrix in its own layout, refreshed when the parameter changes."""
    key = (id(weight), dtype, tuple(weight.shape))
    ver = _version(weight)
    hit = _shadow_cache.get(key)
    same = hit is not None and hit[2]() is weight
    if same and hit[0] == ver:
        return hit[1]
    w = weight.detach().contiguous()
    out = hit[1] if same else torch.empty(w.shape, dtype=dtype, device=w.device)
    check(_lib.lib().dsr_cast16(_dt(out), _ptr(w), _ptr(out), w.numel(), _stream()))
    _shadow_cache[key] = (ver, out, weakref.ref(weight))
    return out


def shadow_for_update(weight):
    """The bf16 shadow tensor of `weight` if one exists (so the optimiser can refresh it in its own pass)."""
    hit = _shadow_cache.get((id(weight), torch.bfloat16, tuple(weight.shape)))
    if hit is not None and hit[2]() is weight and weight.is_contiguous():
        return hit[1]
    return None


def mark_shadow_current(weight):
    key = (id(weight), torch.bfloat16, tuple(weight.shape))
    hit = _shadow_cache.get(key)
    if hit is not None:
        _shadow_cache[key] = (_version(weight), hit[1], hit[2])


def _awaits_allreduce(param):
    """True when a data-parallel run will average `param`.grad with a collective after backward (dist.GradSync) -- such a
    gradient has to exist as a tensor; the dense head's matrix is exempt when its factors are gathered instead."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return False
    return not getattr(param, "_dsr_grad_global", False)


def dp_world_for(param):
    """World size when `param`'s gradient is produced already averaged over the ranks by its own backward
    (`param._dsr_grad_global`, set by dist.GradSync.attach for the dense head's big matrix), else 0."""
    if not getattr(param, "_dsr_grad_global", False):
        return 0
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 0


def _gather_factors(xt, dyt, world):
    """Asynchronous all-gather of the rank-local wgrad factors; returns the [R][...] buffers and the work handles."""
    import torch.distributed as dist
    xt_all = torch.empty((world,) + tuple(xt.shape), dtype=xt.dtype, device=xt.device)
    dyt_all = torch.empty((world,) + tuple(dyt.shape), dtype=dyt.dtype, device=dyt.device)
    if dist.get_backend() == "gloo":        # (rehearsal on one GPU) no all_gather_into_tensor for device tensors
        works = [dist.all_gather(list(xt_all.unbind(0)), xt, async_op=True),
                 dist.all_gather(list(dyt_all.unbind(0)), dyt, async_op=True)]
    else:
        works = [dist.all_gather_into_tensor(xt_all, xt, async_op=True),
                 dist.all_gather_into_tensor(dyt_all, dyt, async_op=True)]
    return xt_all, dyt_all, works


class DenseHead(torch.autograd.Function):
    """sigmoid(Linear(1024,1)(leaky_relu(Linear(K,1024)(flatten_CHW(x)), 0.2)))  -- discriminator.py:65-72.

    x is the NHWC 16-bit output of the last conv block; the C,H,W flatten order of ``x.view(N,-1)`` on an
    NCHW tensor (:65) is reproduced by a small transposing copy, so dense1.weight keeps the reference layout."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, c):
        _need_gpu(x)
        lib = _lib.lib()
        x = x.contiguous()
        n, h, w, cp = x.shape
        hw = h * w
        k = c * hw
        o = w1.shape[0]
        if w1.shape[1] != k:
            raise RuntimeError(f"dense1 expects {w1.shape[1]} features, the conv stack produced {k}")   # torch raises too
        dev = x.device
        st = _stream()
        flat = torch.empty((n, k), dtype=x.dtype, device=dev)
        check(lib.dsr_flatten(_dt(x), _ptr(x), _ptr(flat), n, hw, c, cp, 0, 0, st))
        w16 = shadow16(w1, x.dtype)
        wsz = lib.dsr_linear_fwd_workspace(n, k, o)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        h1 = torch.empty((n, o), dtype=torch.float32, device=dev)
        check(lib.dsr_linear_fwd(_dt(x), _ptr(flat), _ptr(w16), _ptr(b1), ACT_LEAKY, 0.2, _ptr(h1), n, k, o, _ptr(ws),
                                 wsz, st))
        out = torch.empty((n, 1), dtype=torch.float32, device=dev)
        check(lib.dsr_dense2_fwd(_ptr(h1), _ptr(w2), _ptr(b2), n, o, _ptr(out), st))
        ctx.c = c
        ctx.dp_world = dp_world_for(w1)
        ctx.w1 = w1                     # (the Parameter itself: backward may hand its gradient over in factored form)
        ctx.save_for_backward(x, h1, out, w16, w2)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, h1, out, w16, w2 = ctx.saved_tensors
        lib = _lib.lib()
        n, h, w, cp = x.shape
        hw, c = h * w, ctx.c
        k = c * hw
        o = h1.shape[1]
        dev = x.device
        st = _stream()
        bp = 32 if n <= 32 else 64
        dout = dout.contiguous().float()
        dw2 = torch.empty((1, o), dtype=torch.float32, device=dev)
        db2 = torch.empty(1, dtype=torch.float32, device=dev)
        db1 = torch.empty(o, dtype=torch.float32, device=dev)
        dy16 = torch.empty((n, o), dtype=x.dtype, device=dev)
        dyt16 = torch.empty((o, bp), dtype=x.dtype, device=dev)
        check(lib.dsr_dense2_bwd(_dt(x), _ptr(dout), _ptr(out), _ptr(h1), _ptr(w2), n, o, bp, 0.2, _ptr(dw2), _ptr(db2),
                                 _ptr(db1), _ptr(dy16), _ptr(dyt16), st))
        dx = dw1 = None
        gather = None
        if ctx.needs_input_grad[1]:
            xt = torch.empty((k, bp), dtype=x.dtype, device=dev)
            check(lib.dsr_flatten(_dt(x), _ptr(x), _ptr(xt), n, hw, c, cp, bp, 1, st))
            if ctx.dp_world >= 1:     # (1 only under DSR_DIST_FORCE=1: the RCCL path rehearsed on a single rank)
                # data parallel: the averaged dW1 = (1/R) sum_r dyT_r xT_r is formed from the all-gathered rank-local factors
                # (67 MB + 128 KB per rank) instead of all-reducing the 2.1 GB gradient; dist.GradSync skips this tensor
                gather = _gather_factors(xt, dyt16, ctx.dp_world)
        if ctx.needs_input_grad[0]:          # issued before the gather is waited for: it runs under the exchange
            dflat = torch.empty((n, k), dtype=x.dtype, device=dev)
            check(lib.dsr_linear_dgrad(_dt(x), _ptr(dy16), _ptr(w16), _ptr(dflat), n, o, k, st))
            dx = torch.empty_like(x)
            check(lib.dsr_flatten(_dt(x), _ptr(dflat), _ptr(dx), n, hw, c, cp, 0, 2, st))
        if ctx.needs_input_grad[1]:
            works = ()
            if gather is not None:
                xt, dyt16, works = gather
            ranks = max(ctx.dp_world, 1) if gather is not None else 1
            fac = GradFactors(_dt(x), dyt16, xt, bp, o, k, ranks, 1.0 / ranks, works)
            if getattr(ctx.w1, "_dsr_defer_wgrad", False) and k % 64 == 0 and not _awaits_allreduce(ctx.w1):
                # optim.FusedAdam(fuse_dense_head=True): dW1 = dyT x is a rank-(64 R) product -- hand the two factors to
                # the optimiser, whose dsr_linear_wgrad_adam launch forms each tile of it in registers and applies Adam
                # there; the 2.1 GB gradient (config 3) is neither written nor read back
                pending = getattr(ctx.w1, "_dsr_grad_factors", None)
                if pending is None:
                    pending = ctx.w1._dsr_grad_factors = []
                pending.append(fac)
            else:
                dw1 = fac.materialize()
        return dx, dw1, db1, dw2, db2, None


class GradFactors:
    """The gradient of a Linear weight as its two 16-bit factors: dW[o][k] = scale * sum_r sum_b dyT[r][o][b] xT[r][k][b]
    (R rank-local pairs, all-gathered under data parallelism -- `works` are the pending gathers)."""

    def __init__(self, dt, dyt, xt, bp, o, k, ranks, scale, works):
        self.dt, self.dyt, self.xt, self.bp, self.o, self.k = dt, dyt, xt, bp, o, k
        self.ranks, self.scale, self.works = ranks, scale, tuple(works)

    def wait(self):
        for wk in self.works:
            wk.wait()
        self.works = ()

    def materialize(self):
        """The fp32 [o][k] gradient (what Tensor.grad would have held)."""
        lib = _lib.lib()
        self.wait()
        dw = torch.empty((self.o, self.k), dtype=torch.float32, device=self.xt.device)
        if self.ranks > 1 or self.scale != 1.0:
            check(lib.dsr_linear_wgrad_gathered(self.dt, _ptr(self.dyt), _ptr(self.xt), _ptr(dw), self.bp, self.o, self.k,
                                                self.ranks, self.scale, _stream()))
        else:
            check(lib.dsr_linear_wgrad(self.dt, _ptr(self.dyt), _ptr(self.xt), _ptr(dw), self.bp, self.o, self.k, _stream()))
        return dw


# ----------------------------------------------------------------------------- pooling / resampling
class MaxPool2(torch.autograd.Function):
    """nn.MaxPool2d(2, 2) on NHWC (VGG19 trunk, utils/GAN.py:24-47)."""

    @staticmethod
    def forward(ctx, x, *rest):
        in_link = rest[0] if rest else None               # (optional second argument: the Handover of the ReLU that produced x)
        ctx.nin = 1 + len(rest)
        x = x.contiguous()
        n, h, w, cp = x.shape
        y = torch.empty((n, h // 2, w // 2, cp), dtype=x.dtype, device=x.device)
        check(_lib.lib().dsr_maxpool2_fwd(_dt(x), _ptr(x), _ptr(y), n, h, w, cp, _stream()))
        ctx.in_link = in_link
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        n, h, w, cp = x.shape
        dx = torch.empty_like(x)
        link = ctx.in_link
        if link is not None and link.kind == "act" and ACT_LINKS and link.payload[0] == ACT_RELU:
            # x is a ReLU output with this pool as its only consumer: the ReLU's backward rides in the routing (Handover "act")
            check(_lib.lib().dsr_maxpool2_relu_bwd(_dt(x), _ptr(x), _ptr(dy.contiguous()), _ptr(dx), n, h, w, cp, _stream()))
            link.deposit(dx)
        else:
            check(_lib.lib().dsr_maxpool2_bwd(_dt(x), _ptr(x), _ptr(dy.contiguous()), _ptr(dx), n, h, w, cp, _stream()))
        return (dx, None) if ctx.nin == 2 else dx


def _resample2x(name, fwd, bwd, up, doc):
    """The autograd Function `name` of a 2x resampler on NHWC that needs nothing but the input's shape for its backward.
    `fwd`, `bwd`: its entry points, both (dt, src, dst, n, h, w, cp, stream) with the INPUT's h and w; `up`: the output is
    2h x 2w, otherwise h/2 x w/2."""

    def forward(ctx, x):
        x = x.contiguous()
        n, h, w, cp = x.shape
        y = torch.empty((n, 2 * h, 2 * w, cp) if up else (n, h // 2, w // 2, cp), dtype=x.dtype, device=x.device)
        check(getattr(_lib.lib(), fwd)(_dt(x), _ptr(x), _ptr(y), n, h, w, cp, _stream()))
        ctx.shape = (n, h, w, cp)
        return y

    def backward(ctx, dy):
        n, h, w, cp = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((n, h, w, cp), dtype=dy.dtype, device=dy.device)
        check(getattr(_lib.lib(), bwd)(_dt(dy), _ptr(dy), _ptr(dx), n, h, w, cp, _stream()))
        return dx

    return type(name, (torch.autograd.Function,),
                {"__doc__": doc, "forward": staticmethod(forward), "backward": staticmethod(backward)})


AvgPool2 = _resample2x("AvgPool2", "dsr_avgpool2_fwd", "dsr_avgpool2_bwd", False,
                       """nn.AvgPool2d(2, 2) on NHWC: conv(..., downsample_mode='avg') of models/DIP/utils.py:86-94.""")
Nearest2x = _resample2x("Nearest2x", "dsr_nearest2x_fwd", "dsr_nearest2x_bwd", True,
                        """nn.Upsample(scale_factor=2, mode='nearest') on NHWC (models/DIP/skip.py:77, skip()'s default mode).""")
Bilinear2x = _resample2x("Bilinear2x", "dsr_bilinear2x_fwd", "dsr_bilinear2x_bwd", True,
                         """nn.Upsample(scale_factor=2, mode='bilinear') (align_corners=False) on NHWC (models/DIP/skip.py:77).""")


class ResizeNorm(torch.autograd.Function):
    """torchvision ImageClassification preset on an fp32 NCHW batch -> NHWC 16-bit [N, crop, crop, 8].

    ``tab`` is a ResampleTables object (utils/GAN.py mirror) holding the device-resident forward and
    transposed weight tables of the separable antialiased resize + centre crop."""

    @staticmethod
    def forward(ctx, img, tab, dtype):
        _need_gpu(img)
        img = img.contiguous().float()
        n, c, h, w = img.shape
        assert (h, w) == (tab.in_h, tab.in_w), ((h, w), (tab.in_h, tab.in_w))
        out = torch.empty((n, tab.out_h, tab.out_w, 8), dtype=dtype, device=img.device)
        check(_lib.lib().dsr_resize_norm_fwd(_dt(out), _ptr(img), _ptr(out), n, c, h, w, tab.out_h, tab.out_w,
                                             _ptr(tab.ys), _ptr(tab.yc), _ptr(tab.yw), _ptr(tab.xs), _ptr(tab.xc),
                                             _ptr(tab.xw), tab.kt, tab.mean_c, tab.std_c, _stream()))
        ctx.tab, ctx.shape = tab, (n, c, h, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        tab = ctx.tab
        n, c, h, w = ctx.shape
        dout = dout.contiguous()
        dimg = torch.empty((n, c, h, w), dtype=torch.float32, device=dout.device)
        check(_lib.lib().dsr_resize_norm_bwd(_dt(dout), _ptr(dout), _ptr(dimg), n, c, h, w, tab.out_h, tab.out_w,
                                             _ptr(tab.tys), _ptr(tab.tyc), _ptr(tab.tyw), _ptr(tab.txs), _ptr(tab.txc),
                                             _ptr(tab.txw), tab.kt, tab.std_c, _stream()))
        return dimg, None, None


def _box_copy(src, dst, n, bh, bw, c, sy0, sx0, cs0, dy0, dx0, cd0):
    check(_lib.lib().dsr_box_copy(_ptr(src), _ptr(dst), n, bh, bw, c, src.shape[1], src.shape[2], src.shape[3], sy0, sx0,
                                  cs0, dst.shape[1], dst.shape[2], dst.shape[3], dy0, dx0, cd0, _stream()))


class ConcatCrop(torch.autograd.Function):
    """torch.cat([a, b], dim=1) after centre-cropping both to the smaller H, W (models/DIP/utils.py:18-38)."""

    @staticmethod
    def forward(ctx, a, b, ca, cb):
        a, b = a.contiguous(), b.contiguous()
        n = a.shape[0]
        h, w = min(a.shape[1], b.shape[1]), min(a.shape[2], b.shape[2])
        out = torch.zeros((n, h, w, r8(ca + cb)), dtype=a.dtype, device=a.device)
        offs = []
        c0 = 0
        for t, c in ((a, ca), (b, cb)):
            d2, d3 = (t.shape[1] - h) // 2, (t.shape[2] - w) // 2
            _box_copy(t, out, n, h, w, c, d2, d3, 0, 0, 0, c0)
            offs.append((d2, d3, c0, c, tuple(t.shape)))
            c0 += c
        ctx.offs, ctx.hw = offs, (h, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        n = dout.shape[0]
        h, w = ctx.hw
        grads = []
        for d2, d3, c0, c, shape in ctx.offs:
            g = torch.zeros(shape, dtype=dout.dtype, device=dout.device)
            _box_copy(dout, g, n, h, w, c, 0, 0, c0, d2, d3, 0)
            grads.append(g)
        return grads[0], grads[1], None, None


class ConcatChannels(torch.autograd.Function):
    """torch.cat(tensors, dim=1) on NHWC tensors of one N, H, W: ``ConcatChannels.apply((c0, c1, ...), t0, t1, ...)`` with
    the real channel count of each input (ConcatCrop for n inputs, without the crop; one dsr_box_copy per input)."""

    @staticmethod
    def forward(ctx, channels, *tensors):
        tensors = [t.contiguous() for t in tensors]
        n, h, w, _ = tensors[0].shape
        if len(channels) != len(tensors) or any(t.shape[:3] != (n, h, w) or t.dtype != tensors[0].dtype for t in tensors):
            raise ValueError("ConcatChannels: one channel count per input, inputs of one N, H, W and dtype")
        total = sum(channels)
        make = torch.empty if total == r8(total) else torch.zeros        # pad channels are zero
        out = make((n, h, w, r8(total)), dtype=tensors[0].dtype, device=tensors[0].device)
        c0 = 0
        for t, c in zip(tensors, channels):
            _box_copy(t, out, n, h, w, c, 0, 0, 0, 0, 0, c0)
            c0 += c
        ctx.channels, ctx.shapes = tuple(channels), [tuple(t.shape) for t in tensors]
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        n, h, w, _ = dout.shape
        grads, c0 = [], 0
        for i, (c, shape) in enumerate(zip(ctx.channels, ctx.shapes)):
            g = None
            if ctx.needs_input_grad[1 + i]:
                g = (torch.empty if c == shape[3] else torch.zeros)(shape, dtype=dout.dtype, device=dout.device)
                _box_copy(dout, g, n, h, w, c, 0, 0, c0, 0, 0, 0)
            grads.append(g)
            c0 += c
        return (None,) + tuple(grads)


def scale_add16(a, beta, b=None):
    """r16(fmaf(a, beta, b)) on two 16-bit tensors of one shape (b=None: r16(a * beta)): dsr_scale_add16."""
    a = a.contiguous()
    if b is not None:
        b = b.contiguous()
        if b.shape != a.shape or b.dtype != a.dtype:
            raise ValueError(f"scale_add16: operands of {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
    if a.numel() % 8:
        raise ValueError("scale_add16: the element count must be a multiple of 8")
    out = torch.empty_like(a)
    check(_lib.lib().dsr_scale_add16(_dt(a), _ptr(a), float(beta), _ptr(b), _ptr(out), a.numel() // 8, _stream()))
    return out


class ScaleAdd(torch.autograd.Function):
    """a * beta + b on 16-bit NHWC tensors, one rounding (the residual scalings of a dense block on the composed path)."""

    @staticmethod
    def forward(ctx, a, beta, b):
        _need_gpu(a)
        ctx.beta = float(beta)
        return scale_add16(a, beta, b)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        da = scale_add16(g, ctx.beta) if ctx.needs_input_grad[0] else None
        return da, None, (g if ctx.needs_input_grad[2] else None)


# ----------------------------------------------------------------------------- residual dense block on a growth buffer
def rrdb_fused_enabled():
    """DSR_RRDB_FUSED (read per call): 0 = the no-grad forward of a dense block also takes the composed launches."""
    return os.environ.get("DSR_RRDB_FUSED", "1") != "0"


def rdb_conv_desc(x, cin, cout, y, y_off, act=ACT_NONE, slope=0.0, res1=None, r1_off=0, beta1=0.0, res2=None, r2_off=0,
                  beta2=0.0, wf=None, bias=None, max_blocks=0):
    """The dsr_rdb_conv of one prefix convolution: x [N,H,W,ldx] read in channels [0, cin), y written in [y_off, y_off + cout)."""
    n, h, w, ldx = x.shape
    return _lib.RdbConv(_dt(x), n, h, w, cin, cout, x.data_ptr(), ldx, None if wf is None else wf.data_ptr(),
                        None if bias is None else bias.data_ptr(), act, float(slope),
                        None if res1 is None else res1.data_ptr(), 0 if res1 is None else res1.shape[3], r1_off, float(beta1),
                        None if res2 is None else res2.data_ptr(), 0 if res2 is None else res2.shape[3], r2_off, float(beta2),
                        y.data_ptr(), y.shape[3], y_off, int(max_blocks))


def rdb_conv(x, cin, wf, bias, y, y_off, cout, **kw):
    """One dsr_conv_rdb_fwd launch (see rdb_conv_desc; wf: the packed forward image [9][cout][cin] of packed_weights)."""
    _need_gpu(x)
    for t in (x, y, kw.get("res1"), kw.get("res2")):
        if t is not None and not (t.is_contiguous() and t.dim() == 4 and t.dtype == x.dtype and t.shape[:3] == x.shape[:3]):
            raise ValueError("rdb_conv: contiguous NHWC tensors of one N, H, W and dtype are expected")
    d = rdb_conv_desc(x, cin, cout, y, y_off, wf=wf, bias=bias, **kw)
    if KERNEL_LOG is None:
        return check(_lib.lib().dsr_conv_rdb_fwd(C.byref(d), _stream()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = check(_lib.lib().dsr_conv_rdb_fwd(C.byref(d), _stream()))
    e1.record()
    KERNEL_LOG.append(("fwd", (d.N, d.H, d.W, cin, cout, 3, 3, 1, 1), e0, e1, "conv_rdb_kernel"))
    return rc


def rdb_supported(x_shape, dtype, num_feat, num_grow_ch):
    """Does dsr_conv_rdb_fwd take all five launches of a dense block on [N,H,W,*] growth buffers (and is the switch on)?"""
    if not rrdb_fused_enabled() or dtype not in (torch.bfloat16, torch.float16):
        return False
    n, h, w = x_shape[:3]
    key = (n, h, w, dtype, num_feat, num_grow_ch)
    hit = _rdb_supported_cache.get(key)
    if hit is None:
        if len(_rdb_supported_cache) > 1024:
            _rdb_supported_cache.clear()
        hit = _rdb_supported_cache[key] = _rdb_supported(n, h, w, dtype, num_feat, num_grow_ch)
    return hit


_rdb_supported_cache = {}


def _rdb_supported(n, h, w, dtype, num_feat, num_grow_ch):
    ld = num_feat + 4 * num_grow_ch
    dt = BF16 if dtype == torch.bfloat16 else F16
    lib = _lib.lib()
    for k in range(5):
        cin = num_feat + k * num_grow_ch
        cout, ldy, y_off = (num_grow_ch, ld, cin) if k < 4 else (num_feat, ld, 0)
        d = _lib.RdbConv(dt, n, h, w, cin, cout, None, ld, None, None, ACT_LEAKY if k < 4 else ACT_NONE, 0.2, None, 0, 0, 0.0,
                         None, 0, 0, 0.0, None, ldy, y_off, 0)
        if not lib.dsr_conv_rdb_supported(C.byref(d)):
            return False
    return True


def rdb_forward(buf_in, weights, biases, buf_out, res2=None, slope=0.2, beta=0.2):
    """One residual dense block on growth buffers, no autograd: five dsr_conv_rdb_fwd launches, no concatenation copy.

    buf_in [N,H,W,F + 4 G] holds the block input in channels [0, F); conv1..4 (LeakyReLU(slope)) append G channels each in
    place; conv5 writes r16(x5 * beta + x) -- with `res2` r16((x5 * beta + x) * beta + res2[..., :F]) -- into channels
    [0, F) of buf_out, which may have any pixel stride >= F (the next block's buffer, or a dense [N,H,W,F] tensor).
    weights / biases: the five fp32 OIHW weights and [Cout] biases (None entries: no bias)."""
    if not rdb_supported(buf_in.shape, buf_in.dtype, weights[4].shape[0], weights[0].shape[0]):
        raise RuntimeError("rdb_forward: dsr_conv_rdb_fwd does not take this block (shape, or DSR_RRDB_FUSED=0); "
                           "the composed path (ConvAct / ConcatChannels / ScaleAdd) does")
    n, h, w, ld = buf_in.shape
    nf, gc = weights[4].shape[0], weights[0].shape[0]
    if ld != nf + 4 * gc or buf_out.data_ptr() == buf_in.data_ptr():
        raise ValueError("rdb_forward: buf_in must have num_feat + 4 num_grow_ch channels and differ from buf_out")
    dt = _dt(buf_in)
    for k in range(5):
        wk, bk = weights[k], biases[k]
        cin = nf + k * gc
        if tuple(wk.shape) != (gc if k < 4 else nf, cin, 3, 3):
            raise ValueError(f"rdb_forward: conv{k + 1} weight of shape {tuple(wk.shape)}")
        wf, _ = packed_weights(wk, ConvDesc(dt, n, h, w, cin, wk.shape[0], 3, 3, 1, 1, PAD_ZERO), buf_in.dtype)
        bk = None if bk is None else bk.detach()
        if k < 4:
            rdb_conv(buf_in, cin, wf, bk, buf_in, cin, gc, act=ACT_LEAKY, slope=slope)
        elif res2 is None:
            rdb_conv(buf_in, cin, wf, bk, buf_out, 0, nf, res1=buf_in, beta1=beta)
        else:
            rdb_conv(buf_in, cin, wf, bk, buf_out, 0, nf, res1=buf_in, beta1=beta, res2=res2, beta2=beta)


# ----------------------------------------------------------------------------- ... and its backward on the same buffers
RDB_WGRAD_MIN_TILES = 8      # csrc/conv_rdb_bwd.hip: the pixel range is split into chunks of at least this many 2 x 32 tiles


def rdb_dgrad(dy, dy_off, k, wd, dx, cout, scale=1.0, accumulate=False, g=None, g_limit=0, g_scale=1.0, act_out=None,
              mask_lo=None, slope=0.0, max_blocks=0):
    """One dsr_conv_rdb_dgrad launch: channels [dy_off, dy_off + k) of dy against the dgrad image wd [9][cout][k] into
    channels [0, cout) of dx (see include/dsr_hip.h for the epilogue).  mask_lo=None: no mask."""
    _need_gpu(dy)
    for t in (dy, dx, g, act_out):
        if t is not None and not (t.is_contiguous() and t.dim() == 4 and t.dtype == dy.dtype and t.shape[:3] == dy.shape[:3]):
            raise ValueError("rdb_dgrad: contiguous NHWC tensors of one N, H, W and dtype are expected")
    n, h, w, lddy = dy.shape
    d = _lib.RdbDgrad(_dt(dy), n, h, w, k, cout, dy.data_ptr(), lddy, dy_off, wd.data_ptr(), float(scale), dx.data_ptr(),
                      dx.shape[3], int(bool(accumulate)), None if g is None else g.data_ptr(), 0 if g is None else g.shape[3],
                      g_limit if g is not None else 0, float(g_scale), None if act_out is None else act_out.data_ptr(),
                      0 if act_out is None else act_out.shape[3], cout if mask_lo is None else mask_lo, float(slope),
                      int(max_blocks))
    return check(_lib.lib().dsr_conv_rdb_dgrad(C.byref(d), _stream()))


def _rdb_wgrad_desc(n, h, w, dt, x=None, dy=None, g=None, ldg=64, gscale=1.0, dws=None, dbs=None):
    tab = lambda ts: (C.c_void_p * 5)(*[None if t is None else t.data_ptr() for t in (ts or [None] * 5)])
    p = lambda t: None if t is None else t.data_ptr()
    return _lib.RdbWgrad(dt, n, h, w, p(x), 192, p(dy), 192, p(g), ldg, float(gscale), tab(dws), tab(dbs))


def rdb_wgrad_workspace(n, h, w, dtype):
    """Bytes of workspace of dsr_conv_rdb_wgrad on [n, h, w, 192] buffers, and the number of pixel chunks it sums over."""
    d = _rdb_wgrad_desc(n, h, w, BF16 if dtype == torch.bfloat16 else F16)
    return _lib.lib().dsr_conv_rdb_wgrad_workspace(C.byref(d)), _lib.lib().dsr_conv_rdb_wgrad_chunks(C.byref(d))


def rdb_wgrad(x, dy, g, gscale, dws, dbs, ws=None):
    """dsr_conv_rdb_wgrad: the weight / bias gradients of one dense block into the fp32 tensors dws / dbs (five entries each,
    None: not computed) from its forward buffer x, the gradient buffer dy (channels [64, 192) final) and dL/dout g."""
    _need_gpu(x)
    n, h, w, ld = x.shape
    if not (x.is_contiguous() and dy.is_contiguous() and g.is_contiguous() and dy.shape == x.shape and ld == 192
            and g.shape[:3] == x.shape[:3] and dy.dtype == x.dtype and g.dtype == x.dtype):
        raise ValueError("rdb_wgrad: contiguous [N,H,W,192] buffers and a g of the same N, H, W and dtype are expected")
    for k, (dw, db) in enumerate(zip(dws, dbs)):
        cout, cin = (32, 64 + 32 * k) if k < 4 else (64, 192)
        if dw is not None and not (dw.is_contiguous() and dw.dtype == torch.float32 and tuple(dw.shape) == (cout, cin, 3, 3)):
            raise ValueError(f"rdb_wgrad: dw[{k}] must be a contiguous fp32 [{cout},{cin},3,3] tensor")
        if db is not None and not (db.is_contiguous() and db.dtype == torch.float32 and tuple(db.shape) == (cout,)):
            raise ValueError(f"rdb_wgrad: db[{k}] must be a contiguous fp32 [{cout}] tensor")
    d = _rdb_wgrad_desc(n, h, w, _dt(x), x, dy, g, g.shape[3], gscale, dws, dbs)
    lib = _lib.lib()
    need = lib.dsr_conv_rdb_wgrad_workspace(C.byref(d))
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    return check(lib.dsr_conv_rdb_wgrad(C.byref(d), _ptr(ws), ws.numel(), _stream()))


def rdb_train_supported(x_shape, dtype, num_feat, num_grow_ch):
    """rdb_supported(...) and do dsr_conv_rdb_dgrad / dsr_conv_rdb_wgrad take the backward of such a block?"""
    if not rdb_supported(x_shape, dtype, num_feat, num_grow_ch) or (num_feat, num_grow_ch) != (64, 32):
        return False
    n, h, w = x_shape[:3]
    key = (n, h, w, dtype)
    hit = _rdb_train_cache.get(key)
    if hit is None:
        if len(_rdb_train_cache) > 1024:
            _rdb_train_cache.clear()
        lib = _lib.lib()
        dt = BF16 if dtype == torch.bfloat16 else F16
        hit = bool(lib.dsr_conv_rdb_wgrad_supported(C.byref(_rdb_wgrad_desc(n, h, w, dt))))
        for k in range(5):
            kk, cout = (32, 64 + 32 * k) if k < 4 else (64, 192)
            d = _lib.RdbDgrad(dt, n, h, w, kk, cout, None, 192 if k < 4 else 64, cout if k < 4 else 0, None, 1.0, None, 192, 1, None,
                              64, 64, 1.0, None, 192, max(cout - 32, 0) if k else cout, 0.2, 0)
            hit = hit and bool(lib.dsr_conv_rdb_dgrad_supported(C.byref(d)))
        _rdb_train_cache[key] = hit
    return hit


_rdb_train_cache = {}


class RRDBBody(torch.autograd.Function):
    """The whole body of an RRDBNet (every RRDB, three dense blocks each) as ONE autograd node on growth buffers:
    ``RRDBBody.apply(feat, cfg, w, b, w, b, ...)`` with feat [N,H,W,64], cfg = dict(slope=, beta=) and the weight and bias of
    conv1..5 of every dense block in network order (30 tensors per RRDB).

    Forward: one [N,H,W,192] buffer per dense block and the five dsr_conv_rdb_fwd launches of rdb_forward on each -- the bits
    of the no-grad forward; the buffers are the saved activations (192 channels per block: x, x1..x4), with the forward-time
    dgrad images of the weights.  Backward, per dense block in reverse order, on a gradient buffer G of the same shape (three
    of them rotate): dgrad5 fills G from g = dL/dout, dgrad4..1 accumulate into channel prefixes of G in place, each applying
    the LeakyReLU mask of the slice it completes (dsr_conv_rdb_dgrad); one dsr_conv_rdb_wgrad forms the block's ten
    parameter gradients from (buffer, G, g).  No concatenation or split copy, no activation-backward pass, nothing read on
    the host; the only box copies are feat into the first buffer and G[..., :64] of the first block out as dL/dfeat."""

    @staticmethod
    def forward(ctx, feat, cfg, *params):
        _need_gpu(feat)
        feat = feat.contiguous()
        n, h, w, nf = feat.shape
        nd = len(params) // 10
        if nf != 64 or nd == 0 or nd % 3 or len(params) != 10 * nd:
            raise ValueError("RRDBBody: feat [N,H,W,64] and ten parameters per dense block, three blocks per RRDB")
        if not rdb_train_supported(feat.shape, feat.dtype, 64, 32):
            raise RuntimeError("RRDBBody: the growth-buffer kernels do not take this shape (or DSR_RRDB_FUSED=0)")
        slope, beta = float(cfg["slope"]), float(cfg["beta"])
        if not slope > 0.0:
            raise ValueError("RRDBBody: the LeakyReLU slope must be > 0 (the mask is derived from the stored output)")
        dt = _dt(feat)
        bufs = [torch.empty((n, h, w, 192), dtype=feat.dtype, device=feat.device) for _ in range(nd)]
        out = torch.empty((n, h, w, 64), dtype=feat.dtype, device=feat.device)
        _box_copy(feat, bufs[0], n, h, w, 64, 0, 0, 0, 0, 0, 0)
        wds = []
        for d in range(nd):
            buf, dst = bufs[d], (bufs[d + 1] if d + 1 < nd else out)
            for k in range(5):
                wk, bk = params[10 * d + 2 * k], params[10 * d + 2 * k + 1]
                cin, cout = 64 + 32 * k, (32 if k < 4 else 64)
                if tuple(wk.shape) != (cout, cin, 3, 3):
                    raise ValueError(f"RRDBBody: conv{k + 1} weight of shape {tuple(wk.shape)}")
                wf, wd = packed_weights(wk, ConvDesc(dt, n, h, w, cin, cout, 3, 3, 1, 1, PAD_ZERO), feat.dtype)
                wds.append(wd)
                bk = None if bk is None else bk.detach()
                if k < 4:
                    rdb_conv(buf, cin, wf, bk, buf, cin, 32, act=ACT_LEAKY, slope=slope)
                elif d % 3 < 2:
                    rdb_conv(buf, cin, wf, bk, dst, 0, 64, res1=buf, beta1=beta)
                else:
                    rdb_conv(buf, cin, wf, bk, dst, 0, 64, res1=buf, beta1=beta, res2=bufs[d - 2], beta2=beta)
        ctx.nd, ctx.slope, ctx.beta = nd, slope, beta
        ctx.shapes = [None if p is None else tuple(p.shape) for p in params]
        ctx.save_for_backward(*bufs, *wds)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        nd = ctx.nd
        saved = ctx.saved_tensors
        bufs, wds = saved[:nd], saved[nd:]
        g = gout.contiguous()
        n, h, w, _ = g.shape
        dev = g.device
        need_feat = ctx.needs_input_grad[0]
        need_p = ctx.needs_input_grad[2:]
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
        beta = f32(ctx.beta)
        beta_sq = float(torch.tensor(ctx.beta, dtype=torch.float32) * torch.tensor(ctx.beta, dtype=torch.float32))
        grads = [None] * (10 * nd)
        free, ws = [], None
        take = lambda: free.pop() if free else torch.empty((n, h, w, 192), dtype=g.dtype, device=dev)
        g_rrdb = g               # dL/d(output of the RRDB being walked): its input receives it too
        for d in range(nd - 1, -1, -1):
            j = d % 3
            buf, G = bufs[d], take()
            if j == 2:
                g_rrdb = g
            bp = beta_sq if j == 2 else beta
            wd = wds[5 * d:5 * d + 5]
            # G[..., 0:192] = bp * dgrad5(g), channels [0, 64) + g (third block: + beta * g), channels [160, 192) masked by x4
            rdb_dgrad(g, 0, 64, wd[4], G, 192, scale=bp, g=g, g_limit=64, g_scale=(beta if j == 2 else 1.0), act_out=buf,
                      mask_lo=160, slope=ctx.slope)
            for k in (3, 2, 1):
                c = 64 + 32 * k          # slice [c, c + 32) = dY_{k+1} is final; its input gradient goes to [0, c)
                rdb_dgrad(G, c, 32, wd[k], G, c, accumulate=True, act_out=buf, mask_lo=c - 32, slope=ctx.slope)
            if any(need_p[10 * d:10 * d + 10]):
                dws = [torch.empty(ctx.shapes[10 * d + 2 * k], dtype=torch.float32, device=dev)
                       if need_p[10 * d + 2 * k] else None for k in range(5)]
                dbs = [torch.empty(ctx.shapes[10 * d + 2 * k + 1], dtype=torch.float32, device=dev)
                       if ctx.shapes[10 * d + 2 * k + 1] is not None and need_p[10 * d + 2 * k + 1] else None for k in range(5)]
                if ws is None:
                    ws = torch.empty(max(rdb_wgrad_workspace(n, h, w, g.dtype)[0], 16), dtype=torch.uint8, device=dev)
                rdb_wgrad(buf, G, g, bp, dws, dbs, ws)
                for k in range(5):
                    grads[10 * d + 2 * k], grads[10 * d + 2 * k + 1] = dws[k], dbs[k]
            if d > 0 or need_feat:
                # the first block of an RRDB also hands the RRDB's own dL/dout to its input (the outer residual)
                rdb_dgrad(G, 64, 32, wd[0], G, 64, accumulate=True, g=g_rrdb if j == 0 else None, g_limit=64, g_scale=1.0)
            # g of this block is dead now; a G buffer goes back to the pool unless the RRDB still needs it as g_rrdb
            if g.shape[3] == 192 and not (j != 0 and g is g_rrdb):
                free.append(g)
            if j == 0 and g_rrdb is not g and g_rrdb.shape[3] == 192:
                free.append(g_rrdb)
            g = G
        dfeat = None
        if need_feat:
            dfeat = torch.empty((n, h, w, 64), dtype=g.dtype, device=dev)
            _box_copy(g, dfeat, n, h, w, 64, 0, 0, 0, 0, 0, 0)
        return (dfeat, None) + tuple(grads)


class BNAct(torch.autograd.Function):
    """act(BatchNorm2d(x)) on a tensor that does not come straight out of a conv (DIP: BN after Concat,
    models/DIP/skip.py:51)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, nbt, c, cfg):
        _need_gpu(x)
        lib = _lib.lib()
        x = x.contiguous()
        cp = x.shape[-1]
        p = x.numel() // cp
        dev = x.device
        train = bool(cfg["train"])
        scale, shift, mean, rstd = vectors = _bn_vectors(cp, dev)
        if train:
            blocks, rpb = _reduce_blocks(p)
            part = _partials(blocks, 2 * cp, dev)
            check(lib.dsr_pw_channel_stats(_dt(x), _ptr(x), p, cp, blocks, rpb, _ptr(part), _stream()))
            _bn_finalize(part, blocks, c, cp, p, gamma, beta, running_mean, running_var, nbt, cfg, vectors)
        else:
            _bn_eval_affine(gamma, beta, running_mean, running_var, c, cp, vectors)
        act = cfg.get("act", ACT_NONE)
        out = torch.empty_like(x)
        check(lib.dsr_pw_bn_act_fwd(_dt(x), _ptr(x), _ptr(scale), _ptr(shift), None, _ptr(out), p, cp, act,
                                    float(cfg.get("slope", 0.0)), None, _stream()))
        ctx.cfg, ctx.act, ctx.train, ctx.p, ctx.c = cfg, act, train, p, c
        ctx.save_for_backward(x, scale, shift, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, scale, shift, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta, _ = _bn_act_backward(dout.contiguous(), x, scale, shift, mean, rstd, ctx.p, ctx.c, x.shape[-1], ctx.act,
                                                float(ctx.cfg.get("slope", 0.0)), None, ctx.train)
        return dx, dgamma, dbeta, None, None, None, None, None


class Downsample(torch.autograd.Function):
    """Fixed-kernel strided depthwise correlation with ReplicationPad2d on fp32 NCHW (utils/downsampler.py:65-71)."""

    @staticmethod
    def forward(ctx, x, kern, factor, pad):
        _need_gpu(x)
        x = x.contiguous().float()
        n, c, h, w = x.shape
        k = kern.shape[0]
        oh, ow = (h + 2 * pad - k) // factor + 1, (w + 2 * pad - k) // factor + 1
        y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
        check(_lib.lib().dsr_downsample_fwd(_ptr(x), _ptr(kern), _ptr(y), n * c, h, w, k, factor, pad, _stream()))
        ctx.args = (n, c, h, w, k, factor, pad)
        ctx.save_for_backward(kern)
        return y

    @staticmethod
    def backward(ctx, dy):
        (kern,) = ctx.saved_tensors
        n, c, h, w, k, factor, pad = ctx.args
        dy = dy.contiguous().float()
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
        check(_lib.lib().dsr_downsample_bwd(_ptr(dy), _ptr(kern), _ptr(dx), n * c, h, w, k, factor, pad, _stream()))
        return dx, None, None, None


class DownsampleDense(torch.autograd.Function):
    """The Downsampler as the dense layer it is in the reference: ReplicationPad2d(pad) + Conv2d(C, C, k, stride=factor)
    + bias on fp32 NCHW with every filter live (csrc/downsample_dense.hip).  Gradients for x, weight and bias, each
    computed only when asked for.  Under an ambient loss scale (utils.DIP.optimize(loss_scale=...)) the scale enters
    the backward pass at the net's output, i.e. after this op: dx passes on unscaled and gets scaled there, so dw and db
    are multiplied by the scale here to arrive at the optimiser scaled like every other gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, factor, pad):
        _need_gpu(x)
        x = x.contiguous().float()
        w = weight.detach().contiguous().float()
        b = None if bias is None else bias.detach().contiguous().float()
        n, c, h, wd = x.shape
        if w.dim() != 4 or w.shape[0] != c or w.shape[1] != c or w.shape[2] != w.shape[3]:
            raise RuntimeError(f"DownsampleDense: weight {tuple(w.shape)} does not fit an input of {c} planes")
        k = w.shape[2]
        oh, ow = (h + 2 * pad - k) // factor + 1, (wd + 2 * pad - k) // factor + 1
        y = torch.empty((n, c, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=x.device)
        check(_lib.lib().dsr_downsample_dense_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), n, c, h, wd, k, factor, pad,
                                                  _stream()))
        ctx.args = (n, c, h, wd, k, factor, pad, bias is not None)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        n, c, h, wd, k, factor, pad, has_bias = ctx.args
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_db = has_bias and ctx.needs_input_grad[2]
        dy = dy.contiguous().float()
        lib = _lib.lib()
        dx = dw = db = None
        if need_dx:
            dx = torch.empty_like(x)
            check(lib.dsr_downsample_dense_dgrad(_ptr(dy), _ptr(w), _ptr(dx), n, c, h, wd, k, factor, pad, _stream()))
        if need_dw or need_db:
            nbytes = lib.dsr_downsample_dense_wgrad_workspace(n, c, h, wd, k, factor, pad)
            ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x.device)
            dw = torch.empty_like(w)
            db = torch.empty(c, dtype=torch.float32, device=x.device) if need_db else None
            check(lib.dsr_downsample_dense_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws), nbytes, n, c, h, wd, k,
                                                 factor, pad, _stream()))
            if _ambient_scale is not None:
                dw = axpby(dw, None, 1.0, 0.0, _ambient_scale)
                db = None if db is None else axpby(db, None, 1.0, 0.0, _ambient_scale)
            if not need_dw:
                dw = None
        return dx, dw, db, None, None


def imresize_check(rc):
    """`check` for the imresize entry points: DSR_E_UNSUPPORTED (more than 64 taps on an axis) is a NotImplementedError."""
    if rc == -4:
        raise NotImplementedError("dsr_hip: " + _lib.lib().dsr_last_error().decode())
    return check(rc)


def _imresize_launch(src, dst, planes, h, w, oh, ow, idx_h, w_h, taps_h, idx_w, w_w, taps_w):
    imresize_check(_lib.lib().dsr_imresize_f32(_ptr(src), _ptr(dst), planes, h, w, oh, ow, _ptr(idx_h), _ptr(w_h), taps_h,
                                               _ptr(idx_w), _ptr(w_w), taps_w, _stream()))


class Imresize(torch.autograd.Function):
    """MATLAB-style separable resampling of fp32 NCHW (csrc/imresize.hip; the tables: utils.imresize.imresize_tables of the
    H and the W axis).  One launch forward; one launch backward, the same kernel on dy with the transposed tables (a gather:
    deterministic, no atomics).  Gradient for x only.  Like Downsample it has nothing to do under an ambient loss scale: the
    scale enters the backward pass at the net's output, after this op, and there is no parameter gradient to scale here.
    The tables are cached device tensors, so a call reads nothing on the host and allocates its output only."""

    @staticmethod
    def forward(ctx, x, th, tw):
        _need_gpu(x)
        x = x.contiguous().float()
        n, c, h, w = x.shape
        if (h, w) != (th.n_in, tw.n_in):
            raise RuntimeError(f"Imresize: tables for {th.n_in}x{tw.n_in}, input {h}x{w}")
        y = torch.empty((n, c, th.n_out, tw.n_out), dtype=torch.float32, device=x.device)
        _imresize_launch(x, y, n * c, h, w, th.n_out, tw.n_out, th.idx, th.w, th.taps, tw.idx, tw.w, tw.taps)
        ctx.tables = (th, tw)
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        th, tw = ctx.tables
        n, c, h, w = ctx.shape
        dy = dy.contiguous().float()
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
        _imresize_launch(dy, dx, n * c, th.n_out, tw.n_out, h, w, th.t_idx, th.t_w, th.q, tw.t_idx, tw.t_w, tw.q)
        return dx, None, None


# ----------------------------------------------------------------------------- SRVGGNetCompact (csrc/conv_compact.hip, pw_compact.hip)
def compact_fused_enabled():
    """DSR_COMPACT_FUSED (read per call): 0 = the no-grad forward of SRVGGNetCompact also takes the composed launches."""
    return os.environ.get("DSR_COMPACT_FUSED", "1") != "0"


def compact_supported(x_shape, dtype, num_feat, num_ch, upscale):
    """Do dsr_conv_prelu_c_fwd and dsr_conv_shuffle_add_fwd take the body and the tail of an SRVGGNetCompact on an
    [N,H,W,*] input (and is the switch on)?  The kernels are 64-channel ones: any other width is the composed form's."""
    if not compact_fused_enabled() or dtype not in (torch.bfloat16, torch.float16) or num_feat != 64:
        return False
    n, h, w = (int(v) for v in x_shape[:3])
    dt = BF16 if dtype == torch.bfloat16 else F16
    lib = _lib.lib()
    body = _lib.CompactConv(dt, n, h, w, None, None, None, None, None, 0)
    tail = _lib.CompactTail(dt, n, h, w, int(num_ch), int(upscale), None, None, None, None, None, 0)
    return bool(lib.dsr_conv_prelu_c_supported(C.byref(body))) and bool(lib.dsr_conv_shuffle_add_supported(C.byref(tail)))


def _compact_check(x):
    _need_gpu(x)
    if not (x.dim() == 4 and x.shape[3] == 64 and x.is_contiguous()):
        raise ValueError(f"compact conv: a contiguous 16-bit NHWC tensor with 64 channels is expected, got {tuple(x.shape)}")
    return _dt(x)


def compact_conv(x, weight, bias, slope, max_blocks=0):
    """One dsr_conv_prelu_c_fwd launch, no autograd: r16(prelu_c(conv3x3(x, weight) + bias, slope)) on [N,H,W,64].

    weight: fp32 OIHW [64,64,3,3]; bias, slope: fp32 [64] device tensors or None (slope None: no activation).  The slope is
    read from the tensor's own storage by the launch."""
    dt = _compact_check(x)
    if tuple(weight.shape) != (64, 64, 3, 3):
        raise ValueError(f"compact_conv: weight of shape {tuple(weight.shape)}, expected (64, 64, 3, 3)")
    for name, t in (("bias", bias), ("slope", slope)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 64 and t.is_contiguous()):
            raise ValueError(f"compact_conv: {name} must be a contiguous fp32 device tensor of 64 elements")
    n, h, w, _ = x.shape
    wf, _ = packed_weights(weight, ConvDesc(dt, n, h, w, 64, 64, 3, 3, 1, 1, PAD_ZERO), x.dtype)
    y = torch.empty_like(x)
    d = _lib.CompactConv(dt, n, h, w, x.data_ptr(), wf.data_ptr(), None if bias is None else bias.data_ptr(),
                         None if slope is None else slope.data_ptr(), y.data_ptr(), int(max_blocks))
    check(_lib.lib().dsr_conv_prelu_c_fwd(C.byref(d), _stream()))
    return y


def compact_tail(x, weight, bias, base, upscale, max_blocks=0):
    """One dsr_conv_shuffle_add_fwd launch, no autograd: pixel_shuffle(conv3x3(x, weight) + bias, s) + nearest_s(base) as
    fp32 NCHW [N,C,sH,sW].  weight: fp32 OIHW [C s^2,64,3,3]; bias [C s^2] or None; base fp32 [N,C,H,W] or None."""
    dt = _compact_check(x)
    s = int(upscale)
    q = weight.shape[0]
    if tuple(weight.shape[1:]) != (64, 3, 3) or s < 1 or q % (s * s):
        raise ValueError(f"compact_tail: weight of shape {tuple(weight.shape)} for upscale {s}")
    c = q // (s * s)
    n, h, w, _ = x.shape
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.numel() == q and bias.is_contiguous()):
        raise ValueError(f"compact_tail: bias must be a contiguous fp32 device tensor of {q} elements")
    if base is not None:
        if not (base.is_cuda and base.dtype == torch.float32 and tuple(base.shape) == (n, c, h, w)):
            raise ValueError(f"compact_tail: base of shape {tuple(base.shape)} {base.dtype}, expected fp32 {(n, c, h, w)}")
        base = base.contiguous()
    wf, _ = packed_weights(weight, ConvDesc(dt, n, h, w, 64, q, 3, 3, 1, 1, PAD_ZERO), x.dtype)
    out = torch.empty((n, c, s * h, s * w), dtype=torch.float32, device=x.device)
    d = _lib.CompactTail(dt, n, h, w, c, s, x.data_ptr(), wf.data_ptr(), None if bias is None else bias.data_ptr(),
                         None if base is None else base.data_ptr(), out.data_ptr(), int(max_blocks))
    check(_lib.lib().dsr_conv_shuffle_add_fwd(C.byref(d), _stream()))
    return out


def prelu_channel(z, slope):
    """r16(z > 0 ? z : z * slope[c]) on a 16-bit NHWC tensor, no autograd: dsr_pw_prelu_c_fwd."""
    _need_gpu(z)
    z = z.contiguous()
    cp = z.shape[-1]
    y = torch.empty_like(z)
    check(_lib.lib().dsr_pw_prelu_c_fwd(_dt(z), _ptr(z), _ptr(slope), _ptr(y), z.numel() // cp, slope.numel(), cp, _stream()))
    return y


class PReLUChannel(torch.autograd.Function):
    """nn.PReLU(num_parameters=C) on a 16-bit NHWC tensor [N,H,W,r8(C)]; slope: fp32 [C] on the device, any sign.

    Saves the PRE-ACTIVATION z: the backward takes its branch from z (torch's rules at 0: dz = dy * slope and the slope
    gradient gets dy * 0 there), so -- unlike the output-masked conv + PReLU launches of ConvAct -- a negative or zero slope
    is exact and check_prelu_slopes has nothing to check.  The slope gradient is a fixed-order fold of fp32 partial rows
    (no atomics; scratch from torch's allocator)."""

    @staticmethod
    def forward(ctx, z, slope):
        if not (slope.dtype == torch.float32 and slope.dim() == 1 and slope.is_contiguous() and slope.numel() <= z.shape[-1]):
            raise ValueError(f"PReLUChannel: slope of shape {tuple(slope.shape)} {slope.dtype} for {z.shape[-1]} stored channels")
        z = z.contiguous()
        ctx.save_for_backward(z, slope)
        return prelu_channel(z, slope.detach())

    @staticmethod
    def backward(ctx, dy):
        z, slope = ctx.saved_tensors
        dy = dy.contiguous()
        lib = _lib.lib()
        cp = z.shape[-1]
        p = z.numel() // cp
        c = slope.numel()
        dz = torch.empty_like(z)
        part = dslope = None
        if ctx.needs_input_grad[1]:
            part = torch.empty(lib.dsr_pw_prelu_c_rows(p) * cp, dtype=torch.float32, device=z.device)
            dslope = torch.empty(c, dtype=torch.float32, device=z.device)
        check(lib.dsr_pw_prelu_c_bwd(_dt(z), _ptr(dy), _ptr(z), _ptr(slope.detach()), _ptr(dz), p, c, cp, _ptr(part), _ptr(dslope),
                                     _stream()))
        return dz, dslope


class ShuffleAdd(torch.autograd.Function):
    """pixel_shuffle(t, s) + nearest_upsample(base, s) on fp32 NCHW: t [N,C s^2,H,W], base [N,C,H,W] -> [N,C,sH,sW]
    (dsr_shuffle_add_f32).  Backward: the un-shuffle of the gradient and, where the image wants one, its s^2-pixel sums."""

    @staticmethod
    def forward(ctx, t, base, s):
        _need_gpu(t)
        t = t.contiguous().float()
        base = base.contiguous().float()
        n, q, h, w = t.shape
        s = int(s)
        c = q // (s * s)
        if q != c * s * s or tuple(base.shape) != (n, c, h, w):
            raise ValueError(f"ShuffleAdd: t {tuple(t.shape)} and base {tuple(base.shape)} for upscale {s}")
        out = torch.empty((n, c, s * h, s * w), dtype=torch.float32, device=t.device)
        check(_lib.lib().dsr_shuffle_add_f32(_ptr(t), _ptr(base), _ptr(out), n, c, s, h, w, _stream()))
        ctx.dims = (n, c, s, h, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, c, s, h, w = ctx.dims
        dout = dout.contiguous().float()
        dt = torch.empty((n, c * s * s, h, w), dtype=torch.float32, device=dout.device)
        dbase = torch.empty((n, c, h, w), dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[1] else None
        check(_lib.lib().dsr_shuffle_add_bwd_f32(_ptr(dout), _ptr(dt), _ptr(dbase), n, c, s, h, w, _stream()))
        return dt, dbase, None
