#!/usr/bin/env python3
"""Timing of the residual-dense-block kernel (csrc/conv_rdb.hip) and of RRDBNet (GPU box only; development aid).  One GPU step:

    timeout -k 10 600 python tools/microbench_rrdb.py [--repeats 30] [--inner 20] [--out profiles/microbench_rrdb.txt]

fp16 and bf16.  Every measurement is a HIP graph that holds `inner` copies of the launch sequence (1 for the whole-network
rows), warmed up, then replayed `repeats` times between a pair of HIP events with a synchronise after each; the two forms of
one row alternate replay by replay.  Reported: median / min / max per sequence in ms.
  * per launch shape of a dense block (Cin 64, 96, 128, 160 -> 32 and 192 -> 64) at 1 x 256 x 256 and 32 x 64 x 64:
      fused     one dsr_conv_rdb_fwd on the growth buffer (in place; conv5 with its residual)          + achieved TFLOP/s
      composed  the same layer as it runs without that kernel: the dsr_box_copy launches that build the dense concatenated
                input, dsr_conv_fwd on it, and the dsr_scale_add16 pass behind conv5
    FLOPs = 2 * 9 * Cin * Cout * N * H * W (the convolution alone).
  * RRDBNet(scale=4) inference at 1 x 3 x 256 x 256: the fused body against DSR_RRDB_FUSED=0;
  * one steps.gen_l1_step (FusedAdam) of RRDBNet at batch 16, 32 x 32 -> 128 x 128 (the composed, differentiable path)."""
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
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_rrdb.txt"))
    ap.add_argument("--skip-network", action="store_true")
    args = ap.parse_args()
    F, L, M, O, S = P("functional"), P("_lib"), P("models.GAN.rrdbnet"), P("optim"), P("steps")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit({"repeats": args.repeats, "inner": args.inner, "device": torch.cuda.get_device_name(0)})
    torch.manual_seed(0)
    nf, gc, ld = 64, 32, 192
    for dtype in (torch.float16, torch.bfloat16):
        dt = L.F16 if dtype == torch.float16 else L.BF16
        for n, h, w in ((1, 256, 256), (32, 64, 64)):
            buf = torch.randn(n, h, w, ld, device=dev).to(dtype)
            nxt = torch.empty(n, h, w, ld, device=dev, dtype=dtype)
            pieces = [buf[..., :nf].contiguous()] + [buf[..., nf + gc * k:nf + gc * (k + 1)].contiguous() for k in range(4)]
            for k in range(5):
                cin, cout = nf + gc * k, (gc if k < 4 else nf)
                weight = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
                bias = torch.randn(cout, device=dev) * 0.1
                wf, _ = F.packed_weights(weight, L.ConvDesc(dt, n, h, w, cin, cout, 3, 3, 1, 1, 0), dtype)
                if k < 4:
                    fused = lambda: F.rdb_conv(buf, cin, wf, bias, buf, cin, cout, act=F.ACT_LEAKY, slope=0.2)
                else:
                    fused = lambda: F.rdb_conv(buf, cin, wf, bias, nxt, 0, cout, res1=buf, beta1=0.2)
                cfg = dict(stride=1, pad=1, act=F.ACT_LEAKY if k < 4 else F.ACT_NONE, slope=0.2)

                def composed():
                    with torch.no_grad():
                        x = pieces[0] if k == 0 else F.ConcatChannels.apply((nf,) + (gc,) * k, *pieces[:k + 1])
                        y = F.ConvAct.apply(x, weight, bias, None, cfg)
                        return F.ScaleAdd.apply(y, 0.2, pieces[0]) if k == 4 else y

                graphs = {"fused": graph_of(fused, args.inner), "composed": graph_of(composed, args.inner)}
                res = alternate(graphs, args.repeats, args.inner)
                flops = 2.0 * 9 * cin * cout * n * h * w
                d = L.ConvDesc(dt, n, h, w, cin, cout, 3, 3, 1, 1, 0)
                emit({"section": "launch", "dtype": str(dtype).split(".")[1], "shape": [n, h, w], "Cin": cin, "Cout": cout,
                      "fused_ms": [round(v, 4) for v in res["fused"]], "fused_TFLOPs": round(flops / res["fused"][0] / 1e9, 1),
                      "composed_ms": [round(v, 4) for v in res["composed"]],
                      "composed_conv_kernel": L.lib().dsr_conv_kernel_name(d, 0, None).decode(),
                      "composed_launches": (k + 1 if k else 0) + 1 + (1 if k == 4 else 0),
                      "composed_over_fused": round(res["composed"][0] / res["fused"][0], 2)})
                del graphs
            del buf, nxt, pieces
    if not args.skip_network:
        for dtype in (torch.float16, torch.bfloat16):
            net = M.RRDBNet().to(dev).eval()
            net.compute_dtype = dtype
            x = torch.rand(1, 3, 256, 256, device=dev)

            def infer():
                with torch.no_grad():
                    return net(x)

            graphs = {}
            for name, env in (("fused", "1"), ("composed", "0")):
                os.environ["DSR_RRDB_FUSED"] = env
                graphs[name] = graph_of(infer, 1)
            os.environ.pop("DSR_RRDB_FUSED")
            diff = float((graphs["fused"].keep - graphs["composed"].keep).abs().max())
            res = alternate(graphs, args.repeats, 1)
            emit({"section": "RRDBNet(scale=4) inference 1x3x256x256", "dtype": str(dtype).split(".")[1],
                  "fused_ms": [round(v, 3) for v in res["fused"]], "composed_ms": [round(v, 3) for v in res["composed"]],
                  "composed_over_fused": round(res["composed"][0] / res["fused"][0], 3), "max_abs_diff": diff})
            del graphs, net
        net = M.RRDBNet().to(dev).train()
        opt = O.FusedAdam(net.parameters(), lr=1e-4)
        lr, hr = torch.rand(16, 3, 32, 32, device=dev), torch.rand(16, 3, 128, 128, device=dev)
        step = graph_of(lambda: S.gen_l1_step(net, opt, lr, hr), 1)
        res = alternate({"step": step}, args.repeats, 1)
        emit({"section": "gen_l1_step RRDBNet batch 16, 32x32 -> 128x128 (bf16, composed path)",
              "step_ms": [round(v, 3) for v in res["step"]], "loss": float(step.keep[0])})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
