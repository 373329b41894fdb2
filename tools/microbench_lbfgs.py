"""optim.FusedLBFGS (csrc/lbfgs.hip) against torch.optim.LBFGS, in one process on one device:

  optimizer   time per inner iteration of the optimizer alone, on the reference-size DIP parameter set (get_net(32, 'skip',
              skip_n33d=128, skip_n33u=128, skip_n11=4, num_scales=5): 112 tensors, 2,217,831 elements) with a full history
              of 100 pairs.  The closure writes the gradient of a fixed quadratic into .grad (one addcmul per tensor); its
              own time, measured alone, is subtracted.
  dip_x2      one whole LBFGS iteration (closure + optimizer) with the HIP DIP closure at the dip_x2 size (HR 128 x 128,
              bench.py's config 1 net), default torch.optim.LBFGS path against FusedLBFGS.
  passes      HIP-event time of the dot pass (dsr_lbfgs_dots) and the combine pass (dsr_lbfgs_combine) at full history and
              the bandwidth they reach, against the streaming ceiling in profiles/r02_stream_probe.txt.
  accuracy    the GPU test problems' ||x - x_f64|| / ||x_f64|| for FusedLBFGS and torch's fp32 run (the floor) and the ratio.

    python tools/microbench_lbfgs.py [--out profiles/microbench_lbfgs.txt]"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


def stream_ceiling():
    """Best streaming rate of the 537 MB rows (larger than the Infinity Cache) of the recorded probe."""
    txt = open(os.path.join(ROOT, "profiles", "r02_stream_probe.txt")).read()
    big = txt[txt.index("== tensor 537 MB"):]
    return max(float(v) for v in re.findall(r":\s+([\d.]+) TB/s", big))


def ref_params(dev):
    net = P("models.DIP").get_net(32, "skip", "reflection", upsample_mode="bilinear", skip_n33d=128, skip_n33u=128,
                                  skip_n11=4, num_scales=5)
    return [torch.zeros(p.shape, device=dev).normal_(0, 0.05).requires_grad_(True) for p in net.parameters()]


def optimizer_only(dev, out, iters):
    params = ref_params(dev)
    n = sum(p.numel() for p in params)
    g = torch.Generator(device=dev).manual_seed(0)
    A = [torch.rand(p.shape, device=dev, generator=g) * 999 + 1 for p in params]
    B = [torch.randn(p.shape, device=dev, generator=g) for p in params]
    x0 = [p.detach().clone() for p in params]

    def make_closure(opt):
        def closure():
            opt.zero_grad()
            loss = torch.zeros((), device=dev)
            for p, a, b in zip(params, A, B):
                p.grad = torch.addcmul(-b, a, p.detach())          # gradient of 1/2 a p^2 - b p
            return loss
        return closure

    res = {"tensors": len(params), "elements": n}
    for name, cls in (("torch", torch.optim.LBFGS), ("fused", P("optim").FusedLBFGS)):
        with torch.no_grad():
            for p, x in zip(params, x0):
                p.copy_(x)
        opt = cls(params, lr=1, max_iter=101, history_size=100, tolerance_grad=-1, tolerance_change=-1)
        closure = make_closure(opt)
        opt.step(closure)                                  # fills the history: 100 pairs
        torch.cuda.synchronize()
        hist = opt.state_counts()["history"] if name == "fused" else len(opt.state[opt._params[0]]["old_dirs"])
        if name == "fused":
            opt.max_iter, opt.max_eval = iters, iters * 5 // 4
        else:
            opt.param_groups[0].update(max_iter=iters, max_eval=iters * 5 // 4)
        t0 = time.perf_counter()
        opt.step(closure)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        t0 = time.perf_counter()
        for _ in range(iters):
            closure()
        torch.cuda.synchronize()
        clos = time.perf_counter() - t0
        res[name] = {"history": hist, "ms_per_iter": round((total - clos) / iters * 1e3, 3),
                     "closure_ms": round(clos / iters * 1e3, 3)}
        if name == "fused":
            res["passes"] = passes(opt)
        del opt
        torch.cuda.empty_cache()
    res["speedup"] = round(res["torch"]["ms_per_iter"] / res["fused"]["ms_per_iter"], 2)
    out(dict(leg="optimizer", **res))


def passes(opt, reps=20):
    """Time the dot and combine passes on the optimizer's own (full) state."""
    L = P("_lib")
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    k, h, n = len(opt._flat), opt.history_size, opt.n
    ws, vecs = C.c_void_p(opt._ws.data_ptr()), C.c_void_p(opt._vecs.data_ptr())
    ptrs = (C.c_void_p * k)(*[p.data_ptr() for p in opt._flat])
    count = opt.state_counts()["history"]
    npad = (n + 3) // 4 * 4

    def dots():
        L.check(lib.dsr_lbfgs_dots(ws, opt._ws_bytes, vecs, h, n, k, st))

    def combine():
        L.check(lib.dsr_lbfgs_combine(k, ptrs, opt._numel, ws, opt._ws_bytes, vecs, h, n, st))

    with torch.no_grad():
        saved = [p.detach().clone() for p in opt._flat]
    out = {}
    byts = {"dots": 4 * npad * (2 * count + 3), "combine": 4 * n * (2 * count + 1) + 4 * n * 3}
    for name, f in (("dots", dots), ("combine", combine)):
        for _ in range(3):
            f()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        med = statistics.median(ts)
        out[name] = {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "gbyte": round(byts[name] / 1e9, 3),
                     "tbs": round(byts[name] / med / 1e9, 3)}
    with torch.no_grad():
        for p, s in zip(opt._flat, saved):
            p.copy_(s)
    out["stream_ceiling_tbs"] = stream_ceiling()
    for name in ("dots", "combine"):
        out[name]["share_of_ceiling"] = round(out[name]["tbs"] / out["stream_ceiling_tbs"], 3)
    return out


def dip_iteration(dev, out, iters):
    M, Dn, F = P("models.DIP"), P("utils.downsampler"), P("functional")
    hr_sz = 128
    gcpu = torch.Generator().manual_seed(1)
    hr_img = torch.rand(1, 3, hr_sz, hr_sz, generator=gcpu).to(dev)
    z = (torch.rand(1, 32, hr_sz, hr_sz, generator=gcpu) * 0.1).to(dev)
    torch.manual_seed(0)
    net0 = M.get_net(32, "skip", "reflection", upsample_mode="bilinear")
    sd = {k: v.clone() for k, v in net0.state_dict().items()}
    res = {}
    for name, fused in (("torch", False), ("fused", True)):
        net = M.get_net(32, "skip", "reflection", upsample_mode="bilinear")
        net.load_state_dict(sd)
        net.to(dev).train()
        down = Dn.Downsampler(3, 2, "lanczos2", phase=0.5, preserve_size=True).to(dev)
        with torch.no_grad():
            lr_img = down(hr_img)
        params = list(net.parameters())
        cls = P("optim").FusedLBFGS if fused else torch.optim.LBFGS
        opt = cls(params, lr=0.01, max_iter=iters, tolerance_grad=-1, tolerance_change=-1)
        calls = [0]

        def closure():
            opt.zero_grad()
            calls[0] += 1
            loss = F.mse_loss(down(net(z)), lr_img)
            loss.backward()
            return loss

        opt.step(closure)                                   # warm-up (allocations, weight images)
        torch.cuda.synchronize()
        calls[0] = 0
        t0 = time.perf_counter()
        opt.step(closure)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = {"closure_calls": calls[0], "ms_per_iter": round(dt / calls[0] * 1e3, 3)}
    res["speedup"] = round(res["torch"]["ms_per_iter"] / res["fused"]["ms_per_iter"], 2)
    out(dict(leg="dip_x2", max_iter=iters, **res))


def accuracy(dev, out):
    import test_gpu_lbfgs as T
    cases = [("quadratic h100", T.quadratic(), [7, 1000, 3993], dict(lr=1, max_iter=30, history_size=100), 3),
             ("quadratic h5", T.quadratic(), [7, 1000, 3993], dict(lr=1, max_iter=30, history_size=5), 3),
             ("rosenbrock", T.rosenbrock(), [1, 499, 500], dict(lr=0.1, max_iter=30), 0)]
    for name, prob, splits, kw, unused in cases:
        r = T.compare(prob, splits, dev, unused=unused, tolerance_grad=-1, tolerance_change=-1, **kw)
        out(dict(leg="accuracy", case=name, calls=r["cf"], fused_rel_err=r["err"], torch_fp32_floor=r["floor"],
                 ratio=round(r["err"] / r["floor"], 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_lbfgs.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dip-iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P("_lib").lib()
    lines = []

    def out(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    out({"device": torch.cuda.get_device_name(0), "torch": torch.__version__})
    accuracy(dev, out)
    optimizer_only(dev, out, args.iters)
    dip_iteration(dev, out, args.dip_iters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
