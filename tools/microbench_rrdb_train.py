#!/usr/bin/env python3
"""Training RRDBNet on its growth buffers against the composed form, in the same run (GPU box only; development aid).
One GPU step:

    timeout -k 10 900 python tools/microbench_rrdb_train.py [--repeats 30] [--out profiles/microbench_rrdb_train.txt]

Every measurement is a HIP graph, warmed up, then replayed `repeats` times between a pair of HIP events with a synchronise
after each; the composed and the fused form of one row alternate replay by replay (the GAN step: one after the other,
twice).  bf16.  Reported: median / min / max in ms.
  * steps.gen_l1_step at batch 16, 32 x 32 -> 128 x 128, 23 blocks (FusedAdam);
  * steps.realesrgan_step at batch 12, 64 x 64 -> 256 x 256 with the five-tap VggFeatureLoss on stand-in weights;
  * each launch of the new kernels at 16 x 32 x 32 and 12 x 64 x 64 pixels: time and TFLOP/s of the useful products
    (2 * 9 * pixels * K * Cout for an input gradient; 2 * 9 * pixels * sum Cin_k Cout_k for the weight gradients of a block);
  * torch.cuda.max_memory_allocated of one forward + backward of the 23-block net at both sizes, both forms."""
import argparse
import gc
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


def graph_of(fn, warmup=2):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    g.keep = keep
    return g


def alternate(graphs, repeats):
    """{name: (median, min, max) ms}; the graphs take turns, replay by replay."""
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
            times[k].append(e0.elapsed_time(e1))
    return {k: [round(v, 4) for v in (statistics.median(t), min(t), max(t))] for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_rrdb_train.txt"))
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--skip-gan", action="store_true")
    args = ap.parse_args()
    F, G, M, O, S, pc = P("functional"), P("models.GAN"), P("models.GAN.rrdbnet"), P("optim"), P("steps"), P("perceptual")
    L = P("_lib")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit({"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "num_block": args.blocks})

    # ---- per-launch times of the new kernels
    for n, h, w in ((16, 32, 32), (12, 64, 64)):
        pix = n * h * w
        B = torch.randn(n, h, w, 192, device=dev).to(torch.bfloat16)
        Gb = torch.randn(n, h, w, 192, device=dev).to(torch.bfloat16)
        g = torch.randn(n, h, w, 64, device=dev).to(torch.bfloat16)
        graphs, flops = {}, {}
        for k in (5, 4, 3, 2, 1):
            kk, cout = (64, 192) if k == 5 else (32, 64 + 32 * (k - 1))
            weight = torch.randn(kk, cout, 3, 3, device=dev) * 0.05
            _, wd = F.packed_weights(weight, L.ConvDesc(L.BF16, n, h, w, cout, kk, 3, 3, 1, 1, 0), torch.bfloat16)
            if k == 5:
                fn = (lambda wd=wd: F.rdb_dgrad(g, 0, 64, wd, Gb, 192, scale=0.04, g=g, g_limit=64, g_scale=0.2, act_out=B,
                                                mask_lo=160, slope=0.2))
            else:
                fn = (lambda wd=wd, cout=cout, k=k: F.rdb_dgrad(Gb, cout, 32, wd, Gb, cout, accumulate=True, act_out=B if k > 1 else None,
                                                                mask_lo=cout - 32 if k > 1 else None, slope=0.2))
            graphs[f"dgrad{k}"] = graph_of(fn)
            flops[f"dgrad{k}"] = 2.0 * 9 * pix * kk * cout
        dws = [torch.empty((32 if k < 4 else 64, 64 + 32 * k, 3, 3), device=dev) for k in range(5)]
        dbs = [torch.empty((32 if k < 4 else 64,), device=dev) for k in range(5)]
        ws_bytes, chunks = F.rdb_wgrad_workspace(n, h, w, torch.bfloat16)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        graphs["wgrad"] = graph_of(lambda: F.rdb_wgrad(B, Gb, g, 0.2, dws, dbs, ws))
        flops["wgrad"] = 2.0 * 9 * pix * (32 * (64 + 96 + 128 + 160) + 64 * 192)
        res = alternate(graphs, args.repeats)
        emit({"section": f"launches at {n}x{h}x{w} pixels (bf16)", "wgrad_chunks": chunks, "wgrad_workspace_MB": round(ws_bytes / 1e6, 1),
              "ms": res, "TFLOPs": {k: round(flops[k] / res[k][0] / 1e9, 1) for k in res}})
        del graphs, B, Gb, g, ws

    # ---- memory of one forward + backward
    def peak(fused, shape):
        gc.collect()
        F.clear_pack_cache()
        torch.manual_seed(0)
        net = M.RRDBNet(num_block=args.blocks).to(dev).train().set_fused_training(fused)
        x = torch.rand(*shape, device=dev)
        net(x).sum().backward()
        for p in net.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        net(x).sum().backward()
        torch.cuda.synchronize()
        out = torch.cuda.max_memory_allocated()
        del net
        return out, base

    for shape in ((16, 3, 32, 32), (12, 3, 64, 64)):
        c, f = peak(False, shape), peak(True, shape)
        emit({"section": f"max_memory_allocated of forward + backward, input {shape}", "composed_MB": round(c[0] / 1e6, 1),
              "fused_MB": round(f[0] / 1e6, 1), "resident_before_MB": [round(c[1] / 1e6, 1), round(f[1] / 1e6, 1)],
              "fused_over_composed": round(f[0] / c[0], 3)})

    # ---- gen_l1_step
    def l1_setup(fused):
        torch.manual_seed(0)
        net = M.RRDBNet(num_block=args.blocks).to(dev).train().set_fused_training(fused)
        opt = O.FusedAdam(net.parameters(), lr=1e-4)
        return lambda: S.gen_l1_step(net, opt, lr, hr)

    gc.collect()
    F.clear_pack_cache()
    lr, hr = torch.rand(16, 3, 32, 32, device=dev), torch.rand(16, 3, 128, 128, device=dev)
    graphs = {"composed": graph_of(l1_setup(False)), "fused": graph_of(l1_setup(True))}
    res = alternate(graphs, args.repeats)
    emit({"section": "gen_l1_step batch 16, 32x32 -> 128x128 (bf16)", "composed_ms": res["composed"], "fused_ms": res["fused"],
          "composed_over_fused": round(res["composed"][0] / res["fused"][0], 2),
          "loss": [float(graphs["composed"].keep[0]), float(graphs["fused"].keep[0])]})
    del graphs

    # ---- realesrgan_step
    if not args.skip_gan:
        def gan_setup(fused):
            torch.manual_seed(0)
            gen = M.RRDBNet(num_block=args.blocks).to(dev).train().set_fused_training(fused)
            disc = G.UNetDiscriminatorSN().to(dev).train()
            feat = pc.VggFeatureLoss({"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1.0, "conv4_4": 1.0, "conv5_4": 1.0}, "l1").to(dev)
            opt_g, opt_d = O.FusedAdam(gen.parameters(), lr=1e-4), O.FusedAdam(disc.parameters(), lr=1e-4)
            with torch.no_grad():
                for _ in range(30):      # D's power iterations start from random vectors: let sigma settle before it trains G
                    disc(gt)
            return lambda: S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt)

        gc.collect()
        F.clear_pack_cache()
        lq, gt = torch.rand(12, 3, 64, 64, device=dev), torch.rand(12, 3, 256, 256, device=dev)
        # (one graph at a time here: two captured GAN steps alive together returned NaN losses in BOTH forms, while the same
        #  steps issued eagerly, and either graph alone, stay finite -- not looked into further; the two forms therefore run
        #  one after the other in this section, twice, in the order composed, fused, composed, fused)
        res, losses = {"composed": [], "fused": []}, {}
        for rnd in range(2):
            for name, fused in (("composed", False), ("fused", True)):
                gc.collect()
                F.clear_pack_cache()
                graph = graph_of(gan_setup(fused), warmup=1)
                res[name].append(alternate({name: graph}, args.repeats)[name])
                losses[name] = [float(v) for v in graph.keep[:5]]
                del graph
        best = {k: min(v, key=lambda t: t[0]) for k, v in res.items()}
        emit({"section": "realesrgan_step batch 12, 64x64 -> 256x256 (bf16)", "composed_ms": res["composed"], "fused_ms": res["fused"],
              "composed_over_fused": round(best["composed"][0] / best["fused"][0], 2),
              "losses": [losses["composed"], losses["fused"]]})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
