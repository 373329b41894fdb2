#!/usr/bin/env python3
"""Timing of the blind-degradation kernel (csrc/degrade.hip) and of PatchBank(degradation=...) (GPU box only; development
aid).  One GPU step:

    timeout -k 10 600 python tools/microbench_degrade.py [--repeats 20] [--warmup 3] [--out profiles/microbench_degrade.txt]

  1. dsr_degrade_batch_u8 at batch 32, LR 128 x 128, x4, ks = 21 (32 HR crops of 532 x 532 read through 21 x 21 kernels: 0.69
     G fused multiply-adds), with and without noise, identity code against a quarter turn, and ks = 7 and x2 / x8 beside it --
     against the same arithmetic assembled from torch ops on the device: crop with halo, F.pad(reflect), a grouped F.conv2d
     with a different 21 x 21 kernel per sample at stride 4, noise, clamp, round, / 255.
  2. PatchBank.sample(32) of the bank of tools/microbench_data.py: plain (LR patches of the pre-shrunk images) against
     degradation=BlindDegradation() with and without a noise range -- host draws and uploads included.

Every call is warmed up, then timed between a pair of HIP events with a synchronise after it; median, min and max in ms."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "deep-super-resolution_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_degrade.txt"))
    args = ap.parse_args()
    DS = importlib.import_module(PKG + ".dataset")
    D = importlib.import_module(PKG + ".utils.degradation")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def timed(section, calls, work=None):
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
            row = {"section": section, "call": k, "median_ms": round(med[k], 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
            if work and k in work:
                row["Gfma_per_s"] = round(work[k] / (med[k] * 1e-3) / 1e9, 1)
            emit(row)
        return med

    emit({"repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)})
    rng = np.random.RandomState(0)
    pairs = []
    for i in range(100):
        lr = torch.from_numpy(rng.randint(0, 256, (170, 255, 3), dtype=np.uint8)).to(dev)
        pairs.append((lr, D.resize(lr, 255 * 4, 170 * 4)))

    # ---- 1. the kernel
    B, P = 32, 128
    imgs = [pairs[i][1] for i in range(B)]
    z = torch.randn((B, 3, P, P), device=dev)
    std = torch.linspace(0.0, 25.0, B, device=dev)

    def case(s, ks):
        k = torch.from_numpy(D.random_kernels(B, ks, rng=np.random.RandomState(ks))).to(dev)
        p = min(P, 680 // s - 4)
        tops, lefts = [(3 * i) % (680 // s - p) for i in range(B)], [(7 * i) % (1020 // s - p) for i in range(B)]
        return k, p, tops, lefts

    k21, _, tops, lefts = case(4, 21)
    fma = lambda p, ks: B * 3 * p * p * ks * ks
    calls = {"x4_ks21": lambda: D.degrade_batch(imgs, tops, lefts, P, P, 4, k21),
             "x4_ks21_noise": lambda: D.degrade_batch(imgs, tops, lefts, P, P, 4, k21, noise=z, noise_std=std),
             "x4_ks21_code1": lambda: D.degrade_batch(imgs, tops, lefts, P, P, 4, k21, transforms=[1] * B)}
    work = {k: fma(P, 21) for k in calls}
    for s, ks in [(4, 7), (2, 21), (8, 21)]:
        kk, p, tt, ll = case(s, ks)
        calls[f"x{s}_ks{ks}_lr{p}"] = (lambda s, kk, p, tt, ll: lambda: D.degrade_batch(imgs, tt, ll, p, p, s, kk))(s, kk, p, tt, ll)
        work[f"x{s}_ks{ks}_lr{p}"] = fma(p, ks)

    def torch_ops(noise):
        # the HR footprint of every patch (positions chosen inside the image: no reflection needed here), one grouped conv
        r, n = 10, 4 * (P - 1) + 21
        crops = []
        for b in range(B):
            t, l = 4 * tops[b] - r, 4 * lefts[b] - r
            pad = (max(0, -l), max(0, l + n - 1020), max(0, -t), max(0, t + n - 680))
            c = imgs[b][max(t, 0):t + n, max(l, 0):l + n].permute(2, 0, 1).float()
            crops.append(F.pad(c[None], pad, mode="reflect")[0] if any(pad) else c)
        x = torch.stack(crops).reshape(1, B * 3, n, n)
        w = k21[:, None].expand(B, 3, 21, 21).reshape(B * 3, 1, 21, 21)
        acc = F.conv2d(x, w, stride=4, groups=B * 3).reshape(B, 3, P, P)
        if noise:
            acc = acc + std[:, None, None, None] * z
        return torch.round(acc.clamp(0.0, 255.0)) / 255.0

    calls["torch_ops_x4_ks21"] = lambda: torch_ops(False)
    calls["torch_ops_x4_ks21_noise"] = lambda: torch_ops(True)
    work["torch_ops_x4_ks21"] = work["torch_ops_x4_ks21_noise"] = fma(P, 21)
    diff = float((torch_ops(True) - D.degrade_batch(imgs, tops, lefts, P, P, 4, k21, noise=z, noise_std=std)).abs().max())
    emit({"section": "kernel_b32_lr128", "max_abs_diff_torch_ops_vs_kernel": diff})
    med = timed("kernel_b32_lr128", calls, work)
    emit({"section": "kernel_b32_lr128", "torch_over_hip": round(med["torch_ops_x4_ks21"] / med["x4_ks21"], 2),
          "torch_over_hip_noise": round(med["torch_ops_x4_ks21_noise"] / med["x4_ks21_noise"], 2)})

    # ---- 2. PatchBank
    plain = DS.PatchBank(pairs, 4, (P, P), rng=np.random.RandomState(1))
    blind = DS.PatchBank(pairs, 4, (P, P), rng=np.random.RandomState(1), degradation=DS.BlindDegradation())
    noisy = DS.PatchBank(pairs, 4, (P, P), rng=np.random.RandomState(1), degradation=DS.BlindDegradation(noise_std=(0.0, 25.0)))
    med = timed("patch_bank", {"sample32_plain": lambda: plain.sample(B), "sample32_degradation": lambda: blind.sample(B),
                               "sample32_degradation_noise": lambda: noisy.sample(B)})
    emit({"section": "patch_bank", "degradation_over_plain": round(med["sample32_degradation"] / med["sample32_plain"], 3),
          "degradation_noise_over_plain": round(med["sample32_degradation_noise"] / med["sample32_plain"], 3)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
