"""What optim.DynamicLossScaler costs per DIP iteration, and where its scale settles, on one device:

  cost     HIP-graph replay of one DIP iteration at the config-1 shapes (HR 128 x 128, x2, default 5-scale fp16 skip net),
           (b) DipRunner at static 1024 against (c) DipRunner under a scaler at rest (init_scale 1024, never growing): blocks
           of replays of the two alternate in one process, device events around each replay, the median over all of them.
           --parent-tree DIR adds (a): the same static-1024 measurement by a checkout of the parent commit (built there),
           run as a child process before and after; (b) must equal (a) within the spread the repeats show.
  settle   the scale a scaler started at 2**16 holds after --settle-iters iterations (growth_interval --interval), the steps it
           skipped on the way, at config 1 and (--ref-size) at a reference-sized case: x8, a synthetic HR image of 1024 x 672
           (a 2040 x 1356 DIV2K image as dataset.py hands it to DIP.py is 1016 x 672; the width is rounded to the net's 32).

    python tools/microbench_amp.py [--out profiles/microbench_amp.txt] [--parent-tree DIR] [--ref-size]"""
import argparse
import importlib
import json
import math
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep-super-resolution_amd"


IMPORT_ROOT = ROOT        # --child-static: the tree whose package is measured


def P(sub):
    if IMPORT_ROOT not in sys.path:
        sys.path.insert(0, IMPORT_ROOT)
    return importlib.import_module(PKG + "." + sub)


def runner(dev, loss_scale, hr_hw=(128, 128), factor=2, seed=0):
    M, D, S = P("models.DIP"), P("utils.downsampler"), P("steps")
    g = torch.Generator(device="cpu").manual_seed(seed)
    net = M.get_net(32, "skip", "reflection", upsample_mode="bilinear").to(dev).train()
    down = D.Downsampler(3, factor, "lanczos2", phase=0.5, preserve_size=True).to(dev)
    h, w = hr_hw
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    hr = torch.stack([0.5 + 0.4 * torch.sin(12 * xx + 3 * yy), 0.5 + 0.4 * torch.cos(9 * yy), xx * yy])[None]
    hr = (hr + 0.02 * torch.randn(hr.shape, generator=g)).clamp(0, 1).to(dev)
    with torch.no_grad():
        lr_img = down(hr).detach()
    zin = (torch.rand((1, 32, h, w), generator=g) * 0.1).to(dev)
    return S.DipRunner(net, down, zin, lr_img, 0.01, 0.05, loss_scale=loss_scale)


def graphed(dev, loss_scale):
    S = P("steps")
    run = runner(dev, loss_scale)
    noise = torch.randn((1, 32, 128, 128), device=dev)
    return S.GraphedStep(lambda: run.step(noise)), run


def time_block(step, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def static_only(dev, replays, warm):
    """(a) / child mode: median replay time of the static-1024 step of whatever tree this file sits in."""
    step, _ = graphed(dev, 1024.0)
    time_block(step, warm)
    t = time_block(step, replays)
    return {"median_ms": statistics.median(t), "p10_ms": sorted(t)[len(t) // 10], "p90_ms": sorted(t)[len(t) * 9 // 10]}


def parent_static(tree, replays, warm):
    """A fresh process that imports the package from `tree` (this file only supplies the measuring code)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-static", os.path.abspath(tree), "--replays",
                        str(replays), "--warm", str(warm)], capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError("parent-tree run failed:\n" + r.stdout + r.stderr)
    return json.loads(r.stdout.strip().splitlines()[-1])


def cost(dev, out, replays, warm, blocks, parent_tree):
    O = P("optim")
    res = {}
    if parent_tree:
        res["a_parent_static_before"] = parent_static(parent_tree, replays, warm)
    sb, _ = graphed(dev, 1024.0)
    sc, rc = graphed(dev, O.DynamicLossScaler(init_scale=1024.0, growth_interval=10 ** 9))
    time_block(sb, warm)
    time_block(sc, warm)
    tb, tc, mb, mc = [], [], [], []
    for _ in range(blocks):
        b, c = time_block(sb, replays // blocks), time_block(sc, replays // blocks)
        tb += b
        tc += c
        mb.append(statistics.median(b))
        mc.append(statistics.median(c))
    if parent_tree:
        res["a_parent_static_after"] = parent_static(parent_tree, replays, warm)
    res.update(b_static_ms=statistics.median(tb), c_scaler_at_rest_ms=statistics.median(tc), replays_each=len(tb),
               b_block_medians_ms=mb, c_block_medians_ms=mc, c_over_b=statistics.median(tc) / statistics.median(tb),
               scaler_counts=rc.scaler.counts())
    if parent_tree:
        a = [res["a_parent_static_before"]["median_ms"], res["a_parent_static_after"]["median_ms"]]
        res["a_parent_static_ms"] = sum(a) / 2
        res["b_over_a"] = res["b_static_ms"] / res["a_parent_static_ms"]
        res["c_over_a"] = res["c_scaler_at_rest_ms"] / res["a_parent_static_ms"]
    out["cost"] = res


def settle(dev, out, name, hr_hw, factor, iters, interval):
    O = P("optim")
    sc = O.DynamicLossScaler(growth_interval=interval)
    run = runner(dev, sc, hr_hw, factor)
    first = last = None
    for it in range(iters):
        loss, _ = run.step()
        if it == 0:
            first = loss.item()
    last = loss.item()
    taken, skipped = sc.counts()
    out["settle_" + name] = {"hr": list(hr_hw), "factor": factor, "iterations": iters, "growth_interval": interval,
                             "scale_log2": math.log2(sc.get_scale()), "taken": taken, "skipped": skipped,
                             "loss_first": first, "loss_last": last}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_amp.txt"))
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--settle-iters", type=int, default=1500)
    ap.add_argument("--interval", type=int, default=50)
    ap.add_argument("--ref-size", action="store_true")
    ap.add_argument("--ref-iters", type=int, default=300)
    ap.add_argument("--child-static", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_amp needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    if a.child_static:
        global IMPORT_ROOT
        IMPORT_ROOT = a.child_static
        print(json.dumps(static_only(dev, a.replays, a.warm)))
        return
    out = {"device": torch.cuda.get_device_name(0)}
    cost(dev, out, a.replays, a.warm, a.blocks, a.parent_tree)
    settle(dev, out, "config1", (128, 128), 2, a.settle_iters, a.interval)
    if a.ref_size:
        settle(dev, out, "reference_x8", (672, 1024), 8, a.ref_iters, 20)
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(__doc__.split("\n\n")[0] + "\n\n" + txt + "\n")


if __name__ == "__main__":
    main()
