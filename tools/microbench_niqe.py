"""Device-event time of NIQE (csrc/niqe.hip, metrics.NaturalnessImageQualityEvaluator) at [1,3,2048,2048] (one evaluation frame,
441 blocks) and [8,3,512,512] (25 blocks per image), fp32 inputs, shave 0, the published window and stand-in mu / cov:
  plane        dsr_niqe_plane
  imresize     dsr_imresize_f32, the half-size plane of scale 2
  moments_96   dsr_niqe_moments on the plane, 96 x 96 blocks
  moments_48   dsr_niqe_moments on the half-size plane, 48 x 48 blocks
  features     dsr_niqe_features
  statistics   metrics.niqe_statistics (float64 torch ops on the device)
  update       NIQE.update: all of the above, nothing read on the host
  forward      NIQE.forward: update + one transfer of N (36 + 36^2 + 1) numbers + the pseudo-inverse in numpy -- the whole metric
               (a host clock around it: its last step runs on the host)
  yardstick_cpu  tests/niqe_ref.py (float64 numpy) on ONE image of the shape, once: what a BasicSR user pays per image

    python tools/microbench_niqe.py [--repeats 30] [--warmup 5] [--out profiles/microbench_niqe.txt] [--no-cpu]

Every shape is warmed up first; the timed repeats run the calls in turn, each between its own pair of HIP events with a
synchronise after it.  Reported per call: median, min and max over the repeats.  The compiler's figures of the moments kernel
(VGPRs, scratch, LDS) are read from a -Rpass-analysis=kernel-resource-usage compile of csrc/niqe.hip when hipcc is on the path;
its LDS is dynamic, so the launch's own byte count is printed beside them.  A table of what was measured; there is no pass bar."""
import argparse
import importlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "deep-super-resolution_amd"
SHAPES = [(1, 3, 2048, 2048), (8, 3, 512, 512)]


def moments_lds(block, threads):
    """The dynamic LDS of niqe_moments_kernel<block, threads> (niqe_moments_lds in csrc/niqe.hip)."""
    return block * block * 8 + (block + 6) * (block + 6) * 4 + ((threads // 64) * 25 + 49) * 8


def compiler_figures():
    """{kernel: {vgprs, sgprs, scratch_bytes_per_lane, occupancy_waves_per_simd}} of the moments kernels, or a reason."""
    if shutil.which("hipcc") is None:
        return {"not_measured": "hipcc is not on the path"}
    b = importlib.import_module(PKG + "._build")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["hipcc"] + b.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(b.CSRC, "niqe.hip"), "-o",
                                     os.path.join(tmp, "niqe.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return {"not_measured": "the compile failed"}
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1) if "niqe_moments_kernel" in m.group(1) else None
            if name:
                out[name] = {}
            continue
        if name is None:
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("static_lds_bytes", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="leave the yardstick's CPU time out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_niqe.txt"))
    args = ap.parse_args()
    M = importlib.import_module(PKG + ".metrics")
    F = importlib.import_module(PKG + ".functional")
    R = importlib.import_module(PKG + ".utils.imresize")
    L = importlib.import_module(PKG + "._lib")
    lib = L.lib()
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit({"repeats": args.repeats, "warmup": args.warmup, "shave": 0, "device": torch.cuda.get_device_name(0),
          "moments_kernel_compiler_figures": compiler_figures(),
          "moments_kernel_dynamic_lds_bytes": {"block 96, 1024 threads": moments_lds(96, 1024),
                                               "block 48, 256 threads": moments_lds(48, 256)}})
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mod = M.NIQE(reduction="none")
    for shape in SHAPES:
        n, _, hh, ww = shape
        x = torch.rand(shape, generator=torch.Generator().manual_seed(0)).to(dev)
        hc, wc = hh // 96 * 96, ww // 96 * 96
        nb = (hc // 96) * (wc // 96)
        win = M._niqe_window(None, dev)
        tables = M._niqe_device_tables(dev)
        th, tw = R.imresize_tables(hc, hc // 2, 0.5, "bicubic", True, dev), R.imresize_tables(wc, wc // 2, 0.5, "bicubic", True, dev)
        plane = torch.empty(n, hc, wc, dtype=torch.float32, device=dev)
        half = torch.empty(n, hc // 2, wc // 2, dtype=torch.float32, device=dev)
        m1 = torch.empty(n, nb, 5, 5, dtype=torch.float64, device=dev)
        m2 = torch.empty_like(m1)
        feat = torch.empty(n, nb, 36, dtype=torch.float64, device=dev)
        keep = {}
        p = lambda t: t.data_ptr()

        def k_plane():
            L.check(lib.dsr_niqe_plane(L.F32, p(x), n, 3, hh, ww, 0, p(plane), None))

        def k_resize():
            F._imresize_launch(plane, half, n, hc, wc, hc // 2, wc // 2, th.idx, th.w, th.taps, tw.idx, tw.w, tw.taps)

        def k_m96():
            L.check(lib.dsr_niqe_moments(p(plane), n, hc, wc, 96, p(win), p(m1), None))

        def k_m48():
            L.check(lib.dsr_niqe_moments(p(half), n, hc // 2, wc // 2, 48, p(win), p(m2), None))

        def k_feat():
            L.check(lib.dsr_niqe_features(p(m1), p(m2), n, nb, p(tables), p(feat), None))

        def k_stats():
            keep["stats"] = M.niqe_statistics(feat)

        def k_update():
            mod.reset()
            mod.update(x)

        def k_forward():
            mod.reset()
            keep["score"] = mod(x)

        calls = {"plane": k_plane, "imresize": k_resize, "moments_96": k_m96, "moments_48": k_m48, "features": k_feat,
                 "statistics": k_stats, "update": k_update, "forward": k_forward}
        for f in calls.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                host = (time.perf_counter() - t0) * 1e3
                times[k].append(host if k == "forward" else e0.elapsed_time(e1))
        for k, ts in times.items():
            emit({"shape": list(shape), "blocks_per_image": nb, "call": k, "clock": "host" if k == "forward" else "device events",
                  "median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)})
        emit({"shape": list(shape), "score_of_image_0": float(keep["score"][0])})
        if not args.no_cpu:
            import niqe_ref
            import numpy as np
            one = x[:1].cpu().numpy()
            t0 = time.perf_counter()
            ref = niqe_ref.niqe(one, np.zeros((1, 36)), np.eye(36))
            emit({"shape": [1] + list(shape[1:]), "call": "yardstick_cpu", "clock": "host, one run",
                  "ms": round((time.perf_counter() - t0) * 1e3, 1), "score": float(ref[0]),
                  "relative_difference_to_device": float(abs(ref[0] - float(keep["score"][0])) / ref[0])})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
