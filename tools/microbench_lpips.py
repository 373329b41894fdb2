"""Time of one LPIPS call (lpips.LPIPS, AlexNet trunk) for a [1,3,2048,2048] pair (config 5's output size) and a
[32,3,512,512] pair (the train-log batch), with per-launch times from _lib.LAUNCH_LOG.

    python tools/microbench_lpips.py [--iters 20] [--warmup 5] [--backward]

Prints one JSON line per size: median wall time of a call (HIP events around it, the one host read included) and the
median time of each launch, summed per entry point.  --backward times forward + backward with only img1 requiring a gradient
(the training case, steps.gen_lpips_step) on the [32,3,512,512] pair, next to the forward-only call of the same process."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "deep-super-resolution_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--backward", action="store_true", help="also time forward + backward (img1.requires_grad) at 32 x 512 x 512")
    args = ap.parse_args()
    L = importlib.import_module(PKG + "._lib")
    m = importlib.import_module(PKG + ".lpips")
    dev = torch.device("cuda:0")
    mod = m.LPIPS()
    for shape in [(1, 3, 2048, 2048), (32, 3, 512, 512)]:
        g = torch.Generator().manual_seed(0)
        a = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
        b = (a + 0.1 * torch.randn(shape, generator=g).to(dev)).clamp(-1, 1)
        for _ in range(args.warmup):
            mod(a, b)
        torch.cuda.synchronize()
        calls, launches = [], {}
        for _ in range(args.iters):
            L.LAUNCH_LOG = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            v = mod(a, b)
            e1.record()
            torch.cuda.synchronize()
            calls.append(e0.elapsed_time(e1))
            per = {}
            for name, s, e in L.LAUNCH_LOG:
                per[name] = per.get(name, 0.0) + s.elapsed_time(e)
            for name, t in per.items():
                launches.setdefault(name, []).append(t)
            L.LAUNCH_LOG = None
        # trunk FLOPs of the pair (both images): the stem as run (3x3 over 64 channels), conv2..5 as defined
        sizes = mod.tap_sizes(shape[2], shape[3])
        flops = 0
        for (h, w), (_, cout, cin, k, _, _) in zip(sizes, m.ALEX_CONVS):
            cin, k = (m.STEM_CP, 3) if k == 11 else (cin, k)
            flops += 2 * 2 * shape[0] * h * w * cout * cin * k * k
        conv_ms = statistics.median(launches["dsr_conv_fwd"])
        print(json.dumps({"shape": list(shape), "lpips": float(v), "call_ms": round(statistics.median(calls), 4),
                          "trunk_gflop": round(flops / 1e9, 1), "conv_tflops": round(flops / conv_ms / 1e9, 1),
                          "launch_ms": {k: round(statistics.median(t), 4) for k, t in launches.items()}}), flush=True)
    if args.backward:
        backward(args, L, mod, dev)


def backward(args, L, mod, dev):
    shape = (32, 3, 512, 512)
    g = torch.Generator().manual_seed(0)
    a = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
    b = (a + 0.1 * torch.randn(shape, generator=g).to(dev)).clamp(-1, 1)
    x = a.clone().requires_grad_()

    def fwd_bwd():
        x.grad = None
        v = mod(x, b)
        v.backward()
        return v

    for _ in range(args.warmup):
        fwd_bwd()
    torch.cuda.synchronize()
    calls, fwd_only, launches = [], [], {}
    for _ in range(args.iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        mod(a, b)                                   # forward only, alternating with the differentiated call
        ev[1].record()
        torch.cuda.synchronize()
        L.LAUNCH_LOG = []
        ev[2].record()
        v = fwd_bwd()
        ev[3].record()
        torch.cuda.synchronize()
        fwd_only.append(ev[0].elapsed_time(ev[1]))
        calls.append(ev[2].elapsed_time(ev[3]))
        per = {}
        for name, s, e in L.LAUNCH_LOG:
            per[name] = per.get(name, 0.0) + s.elapsed_time(e)
        for name, t in per.items():
            launches.setdefault(name, []).append(t)
        L.LAUNCH_LOG = None
    gx = x.grad
    print(json.dumps({"shape": list(shape), "mode": "forward+backward(img1)", "lpips": float(v.detach()),
                      "fwd_bwd_ms": round(statistics.median(calls), 4), "fwd_only_ms": round(statistics.median(fwd_only), 4),
                      "grad_scale": mod._grad_scale(shape[0], mod.tap_sizes(shape[2], shape[3])),
                      "grad_absmax": float(gx.abs().max()), "grad_finite": bool(torch.isfinite(gx).all()),
                      "launch_ms": {k: round(statistics.median(t), 4) for k, t in launches.items()}}), flush=True)


if __name__ == "__main__":
    main()
