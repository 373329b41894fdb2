#!/usr/bin/env python3
"""Timing of the MATLAB-style imresize (csrc/imresize.hip, utils/imresize.py) (GPU box only; development aid).  One GPU step:

    timeout -k 10 600 python tools/microbench_imresize.py [--repeats 30] [--warmup 3] [--out profiles/microbench_imresize.txt]

Forward and forward + backward of ``imresize(x, 1 / s)`` (bicubic, antialiased) on fp32 NCHW at
    1 x 3 x 2040 x 1356, x1/4 and x1/8   (one DIV2K image: the Deep-Image-Prior forward model at HR size)
    32 x 3 x 512 x 512, x1/4             (a training batch)
beside, on the same tensors,
    ``torch.nn.functional.interpolate(mode='bicubic', antialias=True)`` forward and backward on the device, and
    ``utils.downsampler.Downsampler(3, s, 'lanczos2', phase=0.5, preserve_size=True)`` (functional.Downsample), the operator it
    replaces in Deep Image Prior.
Every call is warmed up, then timed between a pair of HIP events with a synchronise after it; median, min and max in ms.  The
forward rows carry the achieved bytes per second -- input read once plus output written once -- and their share of the 6.29
TB/s copy ceiling measured on the MI355X."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "deep-super-resolution_amd"
COPY_CEILING = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_imresize.txt"))
    args = ap.parse_args()
    I = importlib.import_module(PKG + ".utils.imresize")
    D = importlib.import_module(PKG + ".utils.downsampler")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def timed(section, calls, nbytes):
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
            if k.endswith("_fwd"):
                row["TB_per_s"] = round(nbytes / (med[k] * 1e-3) / 1e12, 3)
                row["of_copy_ceiling"] = round(nbytes / (med[k] * 1e-3) / COPY_CEILING, 3)
            emit(row)
        return med

    emit({"repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)})
    gen = torch.Generator(device=dev).manual_seed(0)
    for shape, factor in (((1, 3, 2040, 1356), 4), ((1, 3, 2040, 1356), 8), ((32, 3, 512, 512), 4)):
        x = torch.rand(shape, device=dev, generator=gen).requires_grad_()
        y = I.imresize(x, scale=1.0 / factor)
        dy = torch.rand(y.shape, device=dev, generator=gen)
        oh, ow = y.shape[2], y.shape[3]
        lanczos = D.Downsampler(3, factor, "lanczos2", phase=0.5, preserve_size=True).to(dev)
        dl = torch.rand(lanczos(x).shape, device=dev, generator=gen)
        ops = {"imresize": (lambda: I.imresize(x, scale=1.0 / factor), dy),
               "torch_interpolate": (lambda: TF.interpolate(x, size=(oh, ow), mode="bicubic", antialias=True), dy),
               "downsample_lanczos2": (lambda: lanczos(x), dl)}
        calls = {}
        for name, (fwd, g) in ops.items():
            calls[name + "_fwd"] = (lambda fwd: lambda: fwd().detach())(fwd)
            calls[name + "_fwd_bwd"] = (lambda fwd, g: lambda: torch.autograd.grad(fwd(), x, g))(fwd, g)
        section = "x".join(map(str, shape)) + f"_x1/{factor}"
        ref = TF.interpolate(x, size=(oh, ow), mode="bicubic", antialias=True)
        emit({"section": section, "out": [oh, ow],
              "max_abs_diff_interior_vs_torch": float((y - ref)[..., 3:-3, 3:-3].abs().max()),
              "max_abs_diff_border_vs_torch": float((y - ref).abs().max())})
        med = timed(section, calls, 4 * (x.numel() + y.numel()))
        emit({"section": section,
              "torch_over_imresize_fwd": round(med["torch_interpolate_fwd"] / med["imresize_fwd"], 2),
              "torch_over_imresize_fwd_bwd": round(med["torch_interpolate_fwd_bwd"] / med["imresize_fwd_bwd"], 2),
              "lanczos2_over_imresize_fwd": round(med["downsample_lanczos2_fwd"] / med["imresize_fwd"], 2),
              "lanczos2_over_imresize_fwd_bwd": round(med["downsample_lanczos2_fwd_bwd"] / med["imresize_fwd_bwd"], 2)})
        del x, y, dy, dl, ref
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
