#!/usr/bin/env python3
"""Timing of functional.ldl_loss and of steps.realesrgan_step with the LDL term (GPU box only; development aid).  One GPU step:

    timeout -k 10 900 python tools/microbench_ldl.py [--repeats 30] [--out profiles/microbench_ldl.txt]

Every measurement is a HIP graph, warmed up, then replayed `repeats` times between a pair of HIP events with a synchronise
after each; the forms of one row alternate replay by replay.  Reported: median / min / max in ms.
  * the primitive at 12 x 3 x 256^2 and 16 x 3 x 128^2, forward alone (two launches) and forward + backward (three), in both
    detach_weight modes, beside the literal form assembled from torch device ops (F.pad, two unfolds, var, masked_fill in place
    of the index-assign, which reads the host and cannot be captured, l1_loss) and torch's autograd in the same run;
  * one steps.realesrgan_step (FusedAdam twice, WeightEMA) at batch 12, 64 x 64 -> 256 x 256, 23-block RRDBNet,
    UNetDiscriminatorSN, VggFeatureLoss({'conv5_4': 1.0}) on stand-in weights, with the term on (ldl_weight=1, a second RRDBNet as
    gen_ema: one more generator forward and a copy of the average per step) and off.  Each variant has modules, optimisers, EMA and
    graph of its own, kept alive beside the graph that trains them."""
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


def torch_ldl(x, gt, e, k=7, detach_weight=False):
    """The literal form from torch device ops (fp32 throughout)."""
    p = (k - 1) // 2
    re = (gt - e).abs().sum(1, keepdim=True)
    r = (gt - x).abs().sum(1, keepdim=True)
    patch = r.var(dim=(-1, -2, -3), keepdim=True) ** (1 / 5)
    win = TF.pad(r, [p, p, p, p], mode="reflect").unfold(2, k, 1).unfold(3, k, 1)
    w = (patch * win.var(dim=(-1, -2), unbiased=True)).masked_fill(r < re, 0.0)
    if detach_weight:
        w = w.detach()
    return TF.l1_loss(w * x, w * gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_ldl.txt"))
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    F, G, M, O, S, pc = P("functional"), P("models.GAN"), P("models.GAN.rrdbnet"), P("optim"), P("steps"), P("perceptual")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit({"repeats": args.repeats, "device": torch.cuda.get_device_name(0)})
    torch.manual_seed(0)
    for shape in ((12, 3, 256, 256), (16, 3, 128, 128)):
        gt = torch.rand(shape, device=dev)
        e = gt + 0.1 * torch.randn(shape, device=dev)
        x = (gt + 0.1 * torch.randn(shape, device=dev)).requires_grad_(True)

        def fwd(loss_fn):
            with torch.no_grad():
                return loss_fn(x, gt, e)

        def both(loss_fn, detach):
            x.grad = None
            loss = loss_fn(x, gt, e, 7, detach)
            loss.backward()
            return loss.detach(), x.grad

        graphs = {"hip_fwd": graph_of(lambda: fwd(F.ldl_loss)), "torch_fwd": graph_of(lambda: fwd(torch_ldl))}
        for detach in (False, True):
            tag = "_detached" if detach else ""
            graphs["hip_fwd_bwd" + tag] = graph_of(lambda d=detach: both(F.ldl_loss, d))
            graphs["torch_fwd_bwd" + tag] = graph_of(lambda d=detach: both(torch_ldl, d))
        res = alternate(graphs, args.repeats)
        lh, gh = graphs["hip_fwd_bwd"].keep
        lt, gtt = graphs["torch_fwd_bwd"].keep
        row = {"section": "ldl_loss, k = 7", "shape": list(shape)}
        for name in ("fwd", "fwd_bwd", "fwd_bwd_detached"):
            row["hip_" + name + "_ms"] = res["hip_" + name]
            row["torch_ops_" + name + "_ms"] = res["torch_" + name]
            row["torch_over_hip_" + name] = round(res["torch_" + name][0] / res["hip_" + name][0], 2)
        row.update({"loss_hip": float(lh), "loss_torch": float(lt), "max_abs_grad_diff": float((gh - gtt).abs().max()),
                    "max_abs_grad": float(gtt.abs().max())})
        emit(row)
        del graphs
    if not args.skip_step:
        lq, gt = torch.rand(12, 3, 64, 64, device=dev), torch.rand(12, 3, 256, 256, device=dev)

        def variant(ldl):
            torch.manual_seed(1)
            disc = G.UNetDiscriminatorSN().to(dev).train()
            gen = M.RRDBNet().to(dev).train()
            feat = pc.VggFeatureLoss({"conv5_4": 1.0}, "l1").to(dev)
            opt_g, opt_d = O.FusedAdam(gen.parameters(), lr=1e-4), O.FusedAdam(disc.parameters(), lr=1e-4)
            ema = O.WeightEMA(gen, decay=0.999)
            kw = {}
            if ldl:
                gen_ema = M.RRDBNet().to(dev).eval()
                gen_ema.load_state_dict(gen.state_dict())
                kw = dict(ldl_weight=1.0, gen_ema=gen_ema)
            g = graph_of(lambda: S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt, ema=ema, **kw), warmup=1)
            # a captured graph holds raw addresses and no references: the modules, optimiser state and EMA it trains must live as
            # long as it is replayed, or the next variant is handed their freed blocks and the two graphs train the same memory
            g.alive = (gen, disc, feat, opt_g, opt_d, ema, kw)
            return g

        graphs = {"off": variant(False), "on": variant(True)}
        res = alternate(graphs, args.repeats)
        for name, g in graphs.items():
            bad = [i for i, v in enumerate(g.keep) if not bool(torch.isfinite(v).all())]
            if bad:
                raise SystemExit(f"microbench_ldl: the '{name}' step produced non-finite outputs {bad}; its time is not reported")
        emit({"section": "one realesrgan_step with ema, batch 12, 64x64 -> 256x256, RRDBNet 23 blocks, UNetDiscriminatorSN, VGG conv5_4 (bf16)",
              "ldl_off_ms": res["off"], "ldl_on_ms": res["on"], "on_over_off": round(res["on"][0] / res["off"][0], 3),
              "losses_off": [float(v) for v in graphs["off"].keep[:5]],
              "losses_on": [float(v) for v in graphs["on"].keep[:5]] + [float(graphs["on"].keep[6])]})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
