#!/usr/bin/env python3
"""Timing of SRVGGNetCompact and of its two kernels (csrc/conv_compact.hip) against the composed form on the same commit's
existing kernels, in the same run (GPU box only; development aid).  One GPU step:

    timeout -k 10 600 python tools/microbench_compact.py [--repeats 30] [--inner 10] [--out profiles/microbench_compact.txt]

bf16.  Every measurement is a HIP graph (`inner` copies of the launch sequence for the single-launch rows, 1 for the others),
warmed up, then replayed `repeats` times between a pair of HIP events with a synchronise after each; the variants of one row
alternate replay by replay.  Reported: median / min / max per sequence in ms.  Every row times the fused form TWICE (fused,
fused_again: two variants of the same form) -- their difference is the run-to-run spread the comparison is read against.
EVERY TIMED VARIANT OWNS ITS MODULES, OPTIMISER, TENSORS AND GRAPH, all kept alive until the run ends (the rule written down
in tools/microbench_ldl.py): no two graphs share a module or an optimiser.
  * SRVGGNetCompact(upscale=4) inference at 1 x 3 x 256 x 256 and 1 x 3 x 720 x 1280, num_conv 16 and 32: the fused form
    against DSR_COMPACT_FUSED=0 (the variable is read per call, i.e. at capture);
  * one body layer at 1 x 256 x 256 x 64 and 1 x 720 x 1280 x 64: dsr_conv_prelu_c_fwd against dsr_conv_fwd (no activation) +
    dsr_pw_prelu_c_fwd, with the achieved TFLOP/s (2 * 9 * 64 * 64 * H * W);
  * the tail (x4, 48 outputs) at both sizes: dsr_conv_shuffle_add_fwd against dsr_conv_fwd (fp32 NCHW) + dsr_shuffle_add_f32;
  * one steps.gen_l1_step (FusedAdam) at 16 x 3 x 64 x 64 -> 256 x 256 (the composed, differentiable form), timed twice."""
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
ALIVE = []            # everything a graph refers to, until the run ends


def P(sub):
    return importlib.import_module(PKG + "." + sub)


def graph_of(fn, inner, warmup=2):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            keep = fn()
    g.keep = keep
    ALIVE.append((g, fn, keep))
    return g


def alternate(graphs, repeats, inner):
    """{name: (median, min, max) ms per sequence}; the graphs take turns, replay by replay."""
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(repeats):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return {k: (statistics.median(t), min(t), max(t)) for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_compact.txt"))
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    F, M, O, S = P("functional"), P("models.GAN.srvgg"), P("optim"), P("steps")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def row(res, digits=4):
        out = {k + "_ms": [round(v, digits) for v in t] for k, t in res.items()}
        f, f2, c = res["fused"][0], res["fused_again"][0], res["composed"][0]
        out["spread"] = round(abs(f - f2) / min(f, f2), 4)
        out["composed_over_fused"] = round(c / max(f, f2), 3)
        return out

    emit({"repeats": args.repeats, "inner": args.inner, "device": torch.cuda.get_device_name(0), "dtype": "bfloat16"})
    torch.manual_seed(0)
    cfg = dict(stride=1, pad=1, act=F.ACT_NONE)
    sizes = ((256, 256), (720, 1280))

    # ---- one body layer, one tail
    for h, w in sizes:
        def body_variant(fused):
            x = torch.randn(1, h, w, 64, device=dev).to(dtype)
            weight = torch.randn(64, 64, 3, 3, device=dev) * 0.05
            bias = torch.randn(64, device=dev) * 0.1
            slope = torch.rand(64, device=dev) - 0.5
            ALIVE.append((x, weight, bias, slope))
            if fused:
                return lambda: F.compact_conv(x, weight, bias, slope)

            def composed():
                with torch.no_grad():
                    return F.prelu_channel(F.ConvAct.apply(x, weight, bias, None, cfg), slope)
            return composed

        graphs = {"fused": graph_of(body_variant(True), args.inner), "composed": graph_of(body_variant(False), args.inner),
                  "fused_again": graph_of(body_variant(True), args.inner)}
        res = alternate(graphs, args.repeats, args.inner)
        out = {"section": "body layer 64 -> 64 + per-channel PReLU", "shape": [1, h, w]}
        out.update(row(res))
        out["fused_TFLOPs"] = round(2.0 * 9 * 64 * 64 * h * w / res["fused"][0] / 1e9, 1)
        emit(out)

        def tail_variant(fused):
            x = torch.randn(1, h, w, 64, device=dev).to(dtype)
            weight = torch.randn(48, 64, 3, 3, device=dev) * 0.05
            bias = torch.randn(48, device=dev) * 0.1
            base = torch.rand(1, 3, h, w, device=dev)
            ALIVE.append((x, weight, bias, base))
            if fused:
                return lambda: F.compact_tail(x, weight, bias, base, 4)

            def composed():
                with torch.no_grad():
                    return F.ShuffleAdd.apply(F.ConvOutNCHW.apply(x, weight, bias, cfg), base, 4)
            return composed

        graphs = {"fused": graph_of(tail_variant(True), args.inner), "composed": graph_of(tail_variant(False), args.inner),
                  "fused_again": graph_of(tail_variant(True), args.inner)}
        res = alternate(graphs, args.repeats, args.inner)
        out = {"section": "tail 64 -> 48 + PixelShuffle(4) + input image", "shape": [1, h, w]}
        out.update(row(res))
        emit(out)

    # ---- whole networks
    if not args.skip_network:
        for h, w in sizes:
            for num_conv in (16, 32):
                def net_variant(env):
                    net = M.SRVGGNetCompact(num_conv=num_conv, upscale=4).to(dev).eval()
                    with torch.no_grad():
                        for m in net.body:
                            if isinstance(m, torch.nn.PReLU):
                                m.weight.uniform_(-0.25, 0.5)
                    net.compute_dtype = dtype
                    x = torch.rand(1, 3, h, w, device=dev)
                    ALIVE.append((net, x))

                    def infer():
                        with torch.no_grad():
                            return net(x)
                    os.environ["DSR_COMPACT_FUSED"] = env
                    try:
                        return graph_of(infer, 1)
                    finally:
                        os.environ.pop("DSR_COMPACT_FUSED")

                graphs = {"fused": net_variant("1"), "composed": net_variant("0"), "fused_again": net_variant("1")}
                res = alternate(graphs, args.repeats, 1)
                out = {"section": "SRVGGNetCompact(upscale=4) inference", "shape": [1, 3, h, w], "num_conv": num_conv}
                out.update(row(res, 3))
                emit(out)

    # ---- one training step (the composed form is the only differentiable one): the same form twice
    if not args.skip_step:
        def step_variant():
            net = M.SRVGGNetCompact(num_conv=16, upscale=4).to(dev).train()
            opt = O.FusedAdam(net.parameters(), lr=1e-4)
            lr, hr = torch.rand(16, 3, 64, 64, device=dev), torch.rand(16, 3, 256, 256, device=dev)
            ALIVE.append((net, opt, lr, hr))
            return graph_of(lambda: S.gen_l1_step(net, opt, lr, hr), 1)

        graphs = {"step": step_variant(), "step_again": step_variant()}
        res = alternate(graphs, args.repeats, 1)
        emit({"section": "gen_l1_step SRVGGNetCompact(num_conv=16) batch 16, 64x64 -> 256x256 (bf16, composed form)",
              "step_ms": [round(v, 3) for v in res["step"]], "step_again_ms": [round(v, 3) for v in res["step_again"]],
              "loss": float(graphs["step"].keep[0])})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
