#!/usr/bin/env python3
"""Timing of the second-order Real-ESRGAN degradation (csrc/filter2d.hip, csrc/degrade_noise.hip, the torch-convention resize
and the unsharp mask on csrc/imresize.hip) at batch 12, ground truth 256 x 256, x4 (GPU box only; development aid).  One GPU
step:

    timeout -k 10 600 python tools/microbench_realesrgan_degrade.py [--repeats 30] [--warmup 3] [--out profiles/microbench_realesrgan_degrade.txt]

Each op is timed beside the same arithmetic out of torch device ops: F.pad(reflect) + a grouped F.conv2d for the filter,
F.interpolate for the resize, elementwise tensor expressions for the noise and the unsharp mask, and the stages composed from
those for the whole pipeline (with this project's jpeg_batch in both columns: torch has no JPEG).

Every call is warmed up, then timed between a pair of HIP events with a synchronise after it; median, min and max in ms."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "deep-super-resolution_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_realesrgan_degrade.txt"))
    args = ap.parse_args()
    D = importlib.import_module(PKG + ".utils.degradation")
    I = importlib.import_module(PKG + ".utils.imresize")
    R = importlib.import_module(PKG + ".utils.realesrgan")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def timed(section, calls):
        for f in calls.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = {}
        for k, ts in times.items():
            med[k] = statistics.median(ts)
            emit({"section": section, "call": k, "median_ms": round(med[k], 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)})
        if "hip" in med and "torch" in med:
            emit({"section": section, "torch_over_hip": round(med["torch"] / med["hip"], 2)})
        return med

    # ---- the torch-op column
    def t_filter2d(x, k):
        b, c, h, w = x.shape
        ks = k.shape[-1]
        xp = TF.pad(x, (ks // 2,) * 4, mode="reflect")
        wt = k[:, None].expand(b, c, ks, ks).reshape(b * c, 1, ks, ks)
        return TF.conv2d(xp.reshape(1, b * c, h + ks - 1, w + ks - 1), wt, groups=b * c).reshape(b, c, h, w)

    def t_interpolate(x, mode, **kw):
        return TF.interpolate(x, mode=mode, **({} if mode == "area" else {"align_corners": False}), **kw)

    def t_gaussian(x, sigma, gray, z, zg):
        n = torch.where(gray.bool()[:, None, None, None], zg[:, None].expand_as(z), z)
        return torch.clamp(x + (sigma / 255.0)[:, None, None, None] * n, 0.0, 1.0)

    def t_poisson(x, scale, gray, z, zg, vals):
        q = torch.round(torch.clamp(x * 255.0, 0.0, 255.0)) / 255.0
        g = 0.2989 * q[:, 0] + 0.587 * q[:, 1] + 0.114 * q[:, 2]
        v = vals[:, None, None, None]
        n = torch.where(gray.bool()[:, None, None, None], (zg / v[:, 0] - g)[:, None].expand_as(z), z / v - q)
        return torch.clamp(x + scale[:, None, None, None] * n, 0.0, 1.0)

    usm_g = torch.from_numpy(D.usm_kernel()).float().to(dev)

    def t_blur51(x):
        b, c, h, w = x.shape
        x = x.reshape(b * c, 1, h, w)
        x = TF.conv2d(TF.pad(x, (0, 0, 25, 25), mode="reflect"), usm_g.reshape(1, 1, -1, 1))
        x = TF.conv2d(TF.pad(x, (25, 25, 0, 0), mode="reflect"), usm_g.reshape(1, 1, 1, -1))
        return x.reshape(b, c, h, w)

    def t_usm(x, weight=0.5, threshold=10.0):
        res = x - t_blur51(x)
        soft = t_blur51((res.abs() * 255.0 > threshold).float())
        return soft * torch.clamp(x + weight * res, 0.0, 1.0) + (1.0 - soft) * x

    emit({"repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "batch": 12, "gt": 256, "scale": 4})
    B, H = 12, 256
    rng = np.random.RandomState(0)
    gt = torch.rand((B, 3, H, H), generator=torch.Generator().manual_seed(0)).to(dev)

    # ---- filter2d: full 21 x 21 kernels, 7 x 7 padded to 21 x 21, at the ground-truth size and at 1.5 x (the largest first resize)
    k21 = torch.from_numpy(D.random_mixed_kernels(B, size=21, rng=rng)).to(dev)
    k7 = torch.from_numpy(D.random_mixed_kernels(B, size=7, rng=rng)).to(dev)
    big = I.interpolate(gt, scale_factor=1.5, mode="bilinear")
    for name, x in (("256", gt), ("384", big)):
        for kname, k in (("21x21", k21), ("7x7_in_21x21", k7)):
            err = float((D.filter2d(x, k) - t_filter2d(x, k)).abs().max())
            emit({"section": f"filter2d_{kname}_{name}", "max_abs_diff_vs_torch": err})
            timed(f"filter2d_{kname}_{name}", {"hip": lambda x=x, k=k: D.filter2d(x, k), "torch": lambda x=x, k=k: t_filter2d(x, k)})

    # ---- the resizes of the chain
    for mode in R.RESIZE_MODES:
        timed(f"interpolate_{mode}_256_x0.5", {"hip": lambda mode=mode: I.interpolate(gt, scale_factor=0.5, mode=mode),
                                               "torch": lambda mode=mode: t_interpolate(gt, mode, scale_factor=0.5)})
        timed(f"interpolate_{mode}_256_x1.5", {"hip": lambda mode=mode: I.interpolate(gt, scale_factor=1.5, mode=mode),
                                               "torch": lambda mode=mode: t_interpolate(gt, mode, scale_factor=1.5)})

    # ---- the noise kernels (draws given: the kernels alone)
    z, zg = torch.randn_like(gt), torch.randn((B, H, H), device=dev)
    amount = torch.from_numpy(rng.uniform(1, 30, B).astype(np.float32)).to(dev)
    gray = torch.from_numpy((rng.uniform(0, 1, B) < 0.4).astype(np.uint8)).to(dev)
    timed("noise_gaussian_256", {"hip": lambda: D.add_gaussian_noise_batch(gt, amount, gray, z=z, zg=zg),
                                 "torch": lambda: t_gaussian(gt, amount, gray, z, zg)})
    q, g, vals = D.poisson_levels(gt, gray)
    pz, pzg = torch.poisson(q * vals[:, None, None, None]), torch.poisson(g * vals[:, None, None])
    scale = torch.from_numpy(rng.uniform(0.05, 3, B).astype(np.float32)).to(dev)
    timed("noise_poisson_256", {"hip": lambda: D.add_poisson_noise_batch(gt, scale, gray, z=pz, zg=pzg, vals=vals),
                                "torch": lambda: t_poisson(gt, scale, gray, pz, pzg, vals)})
    timed("noise_with_draws_256", {"gaussian": lambda: D.add_gaussian_noise_batch(gt, amount, gray),
                                   "poisson": lambda: D.add_poisson_noise_batch(gt, scale, gray)})

    # ---- the unsharp mask
    emit({"section": "usm_sharp_256", "max_abs_diff_vs_torch": float((D.usm_sharp(gt) - t_usm(gt)).abs().max())})
    timed("usm_sharp_256", {"hip": lambda: D.usm_sharp(gt), "torch": lambda: t_usm(gt)})

    # ---- the whole pipeline on fixed plans (host draws and kernel uploads included in both columns)
    deg = R.RealESRGANDegradation(scale=4)
    plans = [deg.plan(B, H, H, np.random.RandomState(s)) for s in range(8)]

    def t_noise(x, kind, amount, gray):
        amount, gray = torch.from_numpy(amount).to(dev), torch.from_numpy(gray.astype(np.uint8)).to(dev)
        if kind == "gaussian":
            return t_gaussian(x, amount, gray, torch.randn_like(x), torch.randn((x.shape[0],) + tuple(x.shape[2:]), device=dev))
        q, g, vals = D.poisson_levels(x, gray)
        return t_poisson(x, amount, gray, torch.poisson(q * vals[:, None, None, None]), torch.poisson(g * vals[:, None, None]), vals)

    def t_pipeline(p):
        up = lambda k: torch.from_numpy(k).to(dev)
        t = t_filter2d(gt, up(p.kernel1))
        t = t_interpolate(t, p.mode1, scale_factor=p.scale1)
        t = D.jpeg_batch(t_noise(t, p.noise1, p.amount1, p.gray1), p.quality1)
        if p.second_blur:
            t = t_filter2d(t, up(p.kernel2))
        t = t_noise(t_interpolate(t, p.mode2, size=p.size2), p.noise2, p.amount2, p.gray2)
        tail = lambda v: t_filter2d(t_interpolate(v, p.mode3, size=p.size3), up(p.sinc_kernel))
        t = D.jpeg_batch(tail(t), p.quality2) if p.jpeg_last else tail(D.jpeg_batch(t, p.quality2))
        return torch.round(torch.clamp(t, 0.0, 1.0) * 255.0) / 255.0

    state = {"hip": 0, "torch": 0}

    def run(which):
        p = plans[state[which] % len(plans)]
        state[which] += 1
        return deg(gt, plan=p) if which == "hip" else t_pipeline(p)

    timed("pipeline_12x3x256x256_x4", {"hip": lambda: run("hip"), "torch": lambda: run("torch")})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
