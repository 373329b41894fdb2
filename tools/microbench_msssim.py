"""Device-event time per call of metrics.MultiScaleStructuralSimilarityIndexMeasure (five scales, csrc/metrics.hip) at
[32,3,512,512], [32,3,192,192] (the reference's HR patches) and [1,3,2048,2048] fp32, next to two yardsticks measured in the
same run:
  msssim_fwd        the module's forward under no_grad (per scale: tiles + fold, pool; one combine launch)
  msssim_fwd_bwd    forward with a graph + backward to the gradient of preds (one launch per scale, coarse to fine)
  ssim_img          (a) dsr_ssim_img_f32, the single-scale forward, at the same shape
  ssim_img_bwd1     (a) dsr_ssim_img_f32 + dsr_ssim_bwd_f32 for img1: a five-scale pyramid touches 1.33 x these pixels
  torch_fwd         (b) tests/msssim_ref.py in fp32 on the same device (torch ops), forward under no_grad
  torch_fwd_bwd     (b) the same with autograd backward to the gradient of preds

    python tools/microbench_msssim.py [--repeats 30] [--warmup 5] [--out profiles/microbench_msssim.txt]

Every shape is warmed up first; the timed repeats then run the six calls in turn (so drift hits all alike), each between its
own pair of HIP events with a synchronise after it.  Reported per call: median, min and max over the repeats.  Per shape a
summary line gives the ratios and whether the HIP path beats (b) by more than the run-to-run spread of both
(max - min of each, added)."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "deep-super-resolution_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_msssim.txt"))
    ap.add_argument("--shapes", default="32x3x512x512,32x3x192x192,1x3x2048x2048")
    ap.add_argument("--only-hip", action="store_true", help="time the HIP calls alone (for a kernel trace)")
    args = ap.parse_args()
    import msssim_ref
    L = importlib.import_module(PKG + "._lib")
    metrics = importlib.import_module(PKG + ".metrics")
    lib = L.lib()
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def P(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    emit({"repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "scales": 5})
    for shape in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        n, c, h, w = shape
        g = torch.Generator().manual_seed(0)
        a = torch.rand(shape, generator=g).to(dev)
        b = (a + 0.1 * torch.randn(shape, generator=g).to(dev)).clamp(0, 1)
        ar = a.clone().requires_grad_()
        ms = metrics.MS_SSIM()
        c1, c2 = 1e-4, 9e-4
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        part = torch.empty(lib.dsr_ssim_img_blocks(n, c, h, w), dtype=torch.float32, device=dev)
        per = torch.empty(n, dtype=torch.float32, device=dev)
        tot = torch.empty(1, dtype=torch.float32, device=dev)
        up = torch.full((n,), 1.0 / n, dtype=torch.float32, device=dev)
        g1 = torch.empty_like(a)

        def msssim_fwd():
            with torch.no_grad():
                return ms(a, b)

        def msssim_fwd_bwd():
            (gx,) = torch.autograd.grad(ms(ar, b), [ar])
            return gx

        def ssim_img():
            L.check(lib.dsr_ssim_img_f32(P(a), P(b), n, c, h, w, c1, c2, P(part), P(per), P(tot), 1.0 / n, 0, st))

        def ssim_img_bwd1():
            ssim_img()
            L.check(lib.dsr_ssim_bwd_f32(P(a), P(b), n, c, h, w, c1, c2, P(up), P(g1), None, st))

        def torch_fwd():
            with torch.no_grad():
                return msssim_ref.msssim_per_image(a, b)[0].mean()

        def torch_fwd_bwd():
            (gx,) = torch.autograd.grad(msssim_ref.msssim_per_image(ar, b)[0].mean(), [ar])
            return gx

        calls = {"msssim_fwd": msssim_fwd, "msssim_fwd_bwd": msssim_fwd_bwd, "ssim_img": ssim_img,
                 "ssim_img_bwd1": ssim_img_bwd1}
        if not args.only_hip:
            calls.update({"torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd})
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
        ms.reset()
        med = {k: statistics.median(ts) for k, ts in times.items()}
        spread = {k: max(ts) - min(ts) for k, ts in times.items()}
        for k, ts in times.items():
            emit({"shape": list(shape), "call": k, "median_ms": round(med[k], 4), "min_ms": round(min(ts), 4),
                  "max_ms": round(max(ts), 4)})
        summary = {"shape": list(shape), "hip_value": float(msssim_fwd()),
                   "fwd_over_ssim_img": round(med["msssim_fwd"] / med["ssim_img"], 2),
                   "fwd_bwd_over_ssim_img_bwd1": round(med["msssim_fwd_bwd"] / med["ssim_img_bwd1"], 2)}
        if not args.only_hip:
            summary.update({
                "torch_value": float(torch_fwd()),
                "torch_over_hip_fwd": round(med["torch_fwd"] / med["msssim_fwd"], 2),
                "torch_over_hip_fwd_bwd": round(med["torch_fwd_bwd"] / med["msssim_fwd_bwd"], 2),
                "hip_fwd_faster_beyond_spread":
                    med["msssim_fwd"] + spread["msssim_fwd"] + spread["torch_fwd"] < med["torch_fwd"],
                "hip_fwd_bwd_faster_beyond_spread":
                    med["msssim_fwd_bwd"] + spread["msssim_fwd_bwd"] + spread["torch_fwd_bwd"] < med["torch_fwd_bwd"]})
        emit(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
