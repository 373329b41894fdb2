#!/usr/bin/env python3
"""Timing of the D4 kernels (csrc/d4.hip) and of what is built on them (GPU box only; development aid).  One GPU step:

    timeout -k 10 600 python tools/microbench_d4.py [--repeats 20] [--warmup 3] [--out profiles/microbench_d4.txt]

  1. PatchBank.sample(32) at LR 128 x 128 / x4 (config-3 patches, the bank of tools/microbench_data.py): augment=False --
     the launches of dsr_patch_batch_u8, which this feature leaves as they were, so this IS the parent's figure -- against
     augment=True, and against what augmentation costs without the kernel: augment=False followed by torch.flip / torch.rot90
     of both batches.  Also the bare kernels, identity code against each of the eight, on the HR batch.
  2. dsr_d4_mean_f32 at 3 x 2048 x 2048: mask 0xFF (9 x 50.3 MB moved) as bytes/s, every single code on its own (2 x 50.3 MB:
     the axis-swapping codes against the axis-preserving ones), dsr_d4_expand_f32 likewise, and the naive baseline
     torch.stack([inverse of each copy with torch.rot90 / torch.flip]).mean(0).
  3. x8 inference 256 x 256 -> 2048 x 2048, Generator(8, 16) in fp16: plain, self-ensemble with ensemble_batch=1, 2 and None
     (all eight copies in one batch, where the conv kernels accept a tensor of that size), and the same at 128 x 128 -> 1024 x 1024.

Every call is warmed up, then timed between a pair of HIP events with a synchronise after it; median, min and max in ms."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "deep-super-resolution_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_d4.txt"))
    ap.add_argument("--skip-inference", action="store_true")
    args = ap.parse_args()
    import d4_ref
    L = importlib.import_module(PKG + "._lib")
    DS = importlib.import_module(PKG + ".dataset")
    D = importlib.import_module(PKG + ".utils.degradation")
    inf = importlib.import_module(PKG + ".infer")
    lib = L.lib()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def P(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def timed(section, calls, extra=None):
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
            if extra and k in extra:
                row["TB_per_s"] = round(extra[k] / (med[k] * 1e-3) / 1e12, 3)
            emit(row)
        return med

    emit({"repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)})

    # ---- 1. PatchBank
    rng = np.random.RandomState(0)
    pairs = []
    for i in range(100):
        lr = torch.from_numpy(rng.randint(0, 256, (170, 255, 3), dtype=np.uint8)).to(dev)
        pairs.append((lr, D.resize(lr, 255 * 4, 170 * 4)))
    plain = DS.PatchBank(pairs, 4, (128, 128), rng=np.random.RandomState(1))
    augmented = DS.PatchBank(pairs, 4, (128, 128), rng=np.random.RandomState(1), augment=True)
    code_rng = np.random.RandomState(2)

    def torch_augment():
        lr, hr = plain.sample(32)
        codes = [int(code_rng.randint(0, 8)) for _ in range(32)]
        return (torch.stack([d4_ref.T(lr[b], codes[b]) for b in range(32)]), torch.stack([d4_ref.T(hr[b], codes[b]) for b in range(32)]))

    med = timed("patch_bank", {"sample32_plain": lambda: plain.sample(32), "sample32_augment": lambda: augmented.sample(32),
                               "sample32_plain_then_torch_rot_flip": torch_augment})
    emit({"section": "patch_bank", "augment_over_plain": round(med["sample32_augment"] / med["sample32_plain"], 3),
          "torch_over_augment": round(med["sample32_plain_then_torch_rot_flip"] / med["sample32_augment"], 3)})
    idx = [i % 100 for i in range(32)]
    imgs, tops, lefts = [pairs[i][1] for i in idx], [7 * (i % 20) for i in range(32)], [11 * (i % 40) for i in range(32)]
    hr_bytes = 32 * 3 * 512 * 512 * 5                   # a byte read and a float written per element
    calls = {"hr_kernel_plain": lambda: DS.patch_batch(imgs, tops, lefts, 512, 512, DS.PATCH_HR_REF)}
    for k in range(8):
        calls[f"hr_kernel_code{k}"] = (lambda k: lambda: DS.patch_batch(imgs, tops, lefts, 512, 512, DS.PATCH_HR_REF, transforms=[k] * 32))(k)
    timed("patch_kernel_32x3x512x512", calls, {k: hr_bytes for k in calls})

    # ---- 2. the reduction at 3 x 2048 x 2048
    planes, H, W = 3, 2048, 2048
    n = planes * H * W
    plane_bytes = 4 * n
    g = torch.Generator().manual_seed(0)
    even = torch.randn((4, planes, H, W), generator=g).to(dev)
    odd = torch.randn((4, planes, W, H), generator=g).to(dev)
    dst = torch.empty((planes, H, W), dtype=torch.float32, device=dev)
    src = torch.randn((planes, H, W), generator=g).to(dev)

    def mean(mask):
        return lambda: L.check(lib.dsr_d4_mean_f32(P(even), P(odd), planes, H, W, mask, P(dst), st))

    def expand(mask):
        return lambda: L.check(lib.dsr_d4_expand_f32(P(src), planes, H, W, mask, P(even), P(odd), st))

    def torch_mean():
        copies = [even[k // 2] if k % 2 == 0 else odd[k // 2] for k in range(8)]
        return torch.stack([d4_ref.T_inv(copies[k], k) for k in range(8)]).mean(0)

    calls, moved = {"mean_0xFF": mean(0xFF), "torch_stack_mean": torch_mean}, {"mean_0xFF": 9 * plane_bytes, "torch_stack_mean": 9 * plane_bytes}
    for k in range(8):
        calls[f"mean_code{k}"], moved[f"mean_code{k}"] = mean(1 << k), 2 * plane_bytes
    med = timed("mean_3x2048x2048", calls, moved)
    swap = statistics.mean(med[f"mean_code{k}"] for k in (1, 3, 5, 7))
    keep = statistics.mean(med[f"mean_code{k}"] for k in (0, 2, 4, 6))
    emit({"section": "mean_3x2048x2048", "axis_swapping_over_axis_preserving": round(swap / keep, 3),
          "torch_over_hip": round(med["torch_stack_mean"] / med["mean_0xFF"], 2)})
    calls, moved = {"expand_0xFF": expand(0xFF)}, {"expand_0xFF": 9 * plane_bytes}
    for k in range(8):
        calls[f"expand_code{k}"], moved[f"expand_code{k}"] = expand(1 << k), 2 * plane_bytes
    timed("expand_3x2048x2048", calls, moved)
    del even, odd, dst

    # ---- 3. x8 inference 256 -> 2048
    if not args.skip_inference:
        gen_mod = importlib.import_module(PKG + ".models.GAN.generator")
        torch.manual_seed(0)
        gen = gen_mod.Generator(8, 16).to(dev)
        lr = torch.rand((1, 3, 256, 256), generator=g).to(dev)
        calls = {"plain": lambda: inf.super_resolve(gen, lr),
                 "self_ensemble_batch_1": lambda: inf.super_resolve(gen, lr, self_ensemble=True, ensemble_batch=1),
                 "self_ensemble_batch_2": lambda: inf.super_resolve(gen, lr, self_ensemble=True, ensemble_batch=2)}
        try:        # eight 64-channel 2048 x 2048 fp16 activations are 4.3 GB: beyond the conv kernels' 2 GiB tensor limit
            inf.super_resolve(gen, lr, self_ensemble=True)
            calls["self_ensemble_batch_all"] = lambda: inf.super_resolve(gen, lr, self_ensemble=True)
        except RuntimeError as e:
            emit({"section": "infer_x8_256_to_2048", "call": "self_ensemble_batch_all", "refused": str(e)})
        med = timed("infer_x8_256_to_2048", calls)
        emit({"section": "infer_x8_256_to_2048", **{k + "_over_plain": round(v / med["plain"], 2) for k, v in med.items() if k != "plain"}})
        lr = torch.rand((1, 3, 128, 128), generator=g).to(dev)      # a size at which all eight copies fit one batch
        calls = {"plain": lambda: inf.super_resolve(gen, lr),
                 "self_ensemble_batch_1": lambda: inf.super_resolve(gen, lr, self_ensemble=True, ensemble_batch=1),
                 "self_ensemble_batch_all": lambda: inf.super_resolve(gen, lr, self_ensemble=True)}
        med = timed("infer_x8_128_to_1024", calls)
        emit({"section": "infer_x8_128_to_1024", **{k + "_over_plain": round(v / med["plain"], 2) for k, v in med.items() if k != "plain"}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
