"""Device-event time per call of the metric kernels (csrc/metrics.hip) at [32,3,512,512] fp32 (the train_GAN.py:110-111 logging
batch) and [1,3,2048,2048]:
  ssim_img     dsr_ssim_img_f32: per-image SSIM (tile launch + one-block fold; what the SSIM modules and evaluate.ssim launch)
  ssim_bwd1    dsr_ssim_bwd_f32 writing the gradient of img1 only
  ssim_bwd2    dsr_ssim_bwd_f32 writing both gradients
  psnr         dsr_psnr_stats_f32 + dsr_psnr_finalize (whole batch, inferred range, running state)

    python tools/microbench_metrics.py [--repeats 30] [--warmup 5]

Every shape is warmed up first; the timed repeats then run the four calls in turn,
each between its own pair of HIP events with a synchronise after it.  Reported per call: median, min and max over the repeats;
the FLOPs and bytes of the formulas below over the median time; and the share of the larger of the two lower bounds
(FLOPs / FP32 vector peak, bytes / HBM peak: MI355X_MICROARCH.md, 157.3 TFLOP/s and 8.0 TB/s), which names what bounds the
kernel.  The FLOP counts are what each kernel's arithmetic executes (multiplies and adds, an FMA counting 2); the bytes are one
read of every input and one write of every output (halo re-reads, which the caches serve, are not counted)."""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "deep-super-resolution_amd"
PEAK_FP32 = 157.3e12          # FP32 vector, spec
PEAK_HBM = 8.0e12             # HBM3E, spec
K = 11
TAP = 3 + 5 * 2               # per window tap of a moment pass: the products a^2, b^2, ab, then 5 FMAs
SSIM_FORMULA = 20             # the SSIM of one position from its 5 moments
COEF = 30                     # the four coefficient maps of one position


def flops_ssim_img(n, c, h, w):
    """Separable: row taps over (16 + 10) staged rows per 16 position rows, 11 x 5 column FMAs, the formula."""
    pos = n * c * (h - 10) * (w - 10)
    return pos * (K * TAP * (16 + 10) / 16 + K * 5 * 2 + SSIM_FORMULA)


def flops_ssim_bwd(n, c, h, w, maps):
    """Per 32 x 32 tile: row taps over 52 x 42, column taps + coefficients over 42 x 42, transposed row taps (maps x 42 x 32)
    and column taps (maps x 32 x 32), 2 FMAs per map tap; the gradient formula (~6 per output)."""
    px = n * c * h * w
    per_tile = 52 * 42 * K * TAP + 42 * 42 * (K * 5 * 2 + COEF) + maps * (42 * 32 + 32 * 32) * K * 2
    return px * (per_tile / (32 * 32) + 6 * (1 if maps == 3 else 2))


def bytes_io(n, c, h, w, reads, writes):
    return 4 * n * c * h * w * (reads + writes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    L = importlib.import_module(PKG + "._lib")
    lib = L.lib()
    dev = torch.device("cuda:0")

    def P(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(json.dumps({"peaks": {"fp32_vector_tflops": PEAK_FP32 / 1e12, "hbm_tbs": PEAK_HBM / 1e12},
                      "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}), flush=True)
    for shape in [(32, 3, 512, 512), (1, 3, 2048, 2048)]:
        n, c, h, w = shape
        g = torch.Generator().manual_seed(0)
        a = torch.rand(shape, generator=g).to(dev)
        b = (a + 0.1 * torch.randn(shape, generator=g).to(dev)).clamp(0, 1)
        c1, c2 = 1e-4, 9e-4
        nb = lib.dsr_ssim_img_blocks(n, c, h, w)
        npart = torch.empty(nb, dtype=torch.float32, device=dev)
        per = torch.empty(n, dtype=torch.float32, device=dev)
        tot = torch.empty(1, dtype=torch.float32, device=dev)
        up = torch.full((n,), 1.0 / n, dtype=torch.float32, device=dev)
        g1, g2 = torch.empty_like(a), torch.empty_like(a)
        e = c * h * w
        pb = lib.dsr_psnr_blocks(n, e)
        sse = torch.empty(pb, dtype=torch.float32, device=dev)
        keys = torch.empty(2 * pb, dtype=torch.int32, device=dev)
        state = torch.zeros(4, dtype=torch.float64, device=dev)
        pval = torch.empty(1, dtype=torch.float32, device=dev)

        def ssim_img():
            L.check(lib.dsr_ssim_img_f32(P(a), P(b), n, c, h, w, c1, c2, P(npart), P(per), P(tot), 1.0 / n, 0, st))

        def ssim_bwd1():
            L.check(lib.dsr_ssim_bwd_f32(P(a), P(b), n, c, h, w, c1, c2, P(up), P(g1), None, st))

        def ssim_bwd2():
            L.check(lib.dsr_ssim_bwd_f32(P(a), P(b), n, c, h, w, c1, c2, P(up), P(g1), P(g2), st))

        def psnr():
            L.check(lib.dsr_psnr_stats_f32(P(b), P(a), n, e, P(sse), P(keys), st))
            L.check(lib.dsr_psnr_finalize(P(sse), P(keys), n, e, 1, 1.0, 10 / math.log(10), None, P(pval), 1.0, P(state), st))

        calls = {"ssim_img": ssim_img, "ssim_bwd1": ssim_bwd1, "ssim_bwd2": ssim_bwd2, "psnr": psnr}
        work = {"ssim_img": (flops_ssim_img(*shape), bytes_io(*shape, 2, 0)),
                "ssim_bwd1": (flops_ssim_bwd(*shape, 3), bytes_io(*shape, 2, 1)),
                "ssim_bwd2": (flops_ssim_bwd(*shape, 4), bytes_io(*shape, 2, 2)),
                "psnr": (3 * n * e, bytes_io(*shape, 2, 0))}
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
        for k, ts in times.items():
            med = statistics.median(ts)
            fl, by = work[k]
            t_f, t_b = fl / PEAK_FP32, by / PEAK_HBM
            print(json.dumps({"shape": list(shape), "call": k, "median_ms": round(med, 4), "min_ms": round(min(ts), 4),
                              "max_ms": round(max(ts), 4), "gflop": round(fl / 1e9, 2), "gbyte": round(by / 1e9, 3),
                              "tflops": round(fl / med / 1e9, 2), "tbs": round(by / med / 1e9, 3),
                              "bound": "fp32" if t_f >= t_b else "hbm",
                              "share_of_bound": round(max(t_f, t_b) * 1e3 / med, 3)}), flush=True)


if __name__ == "__main__":
    main()
