#!/usr/bin/env python3
"""Timing of the spectral-norm launch group, UNetDiscriminatorSN and steps.realesrgan_step (GPU box only; development aid).
One GPU step:

    timeout -k 10 600 python tools/microbench_unetd.py [--repeats 30] [--out profiles/microbench_unetd.txt]

Every measurement is a HIP graph, warmed up, then replayed `repeats` times between a pair of HIP events with a synchronise
after each; the two forms of one row alternate replay by replay.  Reported: median / min / max in ms.
  * the spectral-norm launch group for the eight normalised layers of the default discriminator (4.4 M weights, 17.6 MB),
    train mode (4 launches) and eval mode (2), and its backward (2 launches), beside the same arithmetic in torch ops on the
    device (mv / norm / div per layer);
  * UNetDiscriminatorSN forward (no grad) and forward + backward of gan_loss at 12 x 3 x 256 x 256, bf16;
  * one steps.realesrgan_step (FusedAdam twice) at batch 12, 64 x 64 -> 256 x 256, 23-block RRDBNet, stand-in VGG weights."""
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


def torch_sn(ws, us, vs, training, eps=1e-12):
    """The same arithmetic in torch ops (u, v in place), one layer after the other."""
    outs = []
    for w, u, v in zip(ws, us, vs):
        m = w.reshape(w.shape[0], -1)
        if training:
            t = torch.mv(m.t(), u)
            v.copy_(t / t.norm().clamp_min(eps))
            s = torch.mv(m, v)
            u.copy_(s / s.norm().clamp_min(eps))
        sigma = torch.dot(u, torch.mv(m, v))
        outs.append(w / sigma)
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_unetd.txt"))
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
    disc = G.UNetDiscriminatorSN().to(dev).train()
    layers = [getattr(disc, f"conv{i}") for i in range(1, 9)]
    ws = [m.weight_orig.detach() for m in layers]
    us, vs = [m.weight_u for m in layers], [m.weight_v for m in layers]
    nbytes = 4 * sum(w.numel() for w in ws)
    for training in (True, False):
        graphs = {"hip": graph_of(lambda: F._sn_forward(ws, us, vs, training)[0]),
                  "torch": graph_of(lambda: torch_sn(ws, us, vs, training))}
        res = alternate(graphs, args.repeats)
        emit({"section": "spectral norm, 8 default layers", "mode": "train" if training else "eval", "weight_MB": round(nbytes / 1e6, 1),
              "hip_ms": res["hip"], "torch_ops_ms": res["torch"], "torch_over_hip": round(res["torch"][0] / res["hip"][0], 2),
              "hip_GBps_of_weights": round(nbytes / res["hip"][0] / 1e6, 1)})
        del graphs
    outs, sigmas = F._sn_forward(ws, us, vs, True)
    gs = [torch.randn_like(w) for w in ws]
    L = P("_lib")
    import ctypes as C
    n = len(ws)
    ci = (C.c_int * n)(*[w.shape[0] for w in ws])
    ki = (C.c_int * n)(*[w.numel() // w.shape[0] for w in ws])
    dws = [torch.empty_like(w) for w in ws]
    sigma = torch.cat(sigmas)
    wsz = L.lib().dsr_spectral_norm_bwd_workspace(n, ci, ki)
    work = torch.empty(wsz // 4, dtype=torch.float32, device=dev)

    def hip_bwd():
        L.check(L.lib().dsr_spectral_norm_bwd(n, L.ptr_table(gs), L.ptr_table(outs), L.ptr_table(us), L.ptr_table(vs), ci, ki,
                                              C.c_void_p(sigma.data_ptr()), L.ptr_table(dws), C.c_void_p(work.data_ptr()), wsz,
                                              F._stream()))
        return dws

    def torch_bwd():
        return [(g - (g * o).sum() * torch.outer(u, v).reshape(g.shape)) / s for g, o, u, v, s in zip(gs, outs, us, vs, sigmas)]

    res = alternate({"hip": graph_of(hip_bwd), "torch": graph_of(torch_bwd)}, args.repeats)
    emit({"section": "spectral norm backward, 8 default layers", "hip_ms": res["hip"], "torch_ops_ms": res["torch"],
          "torch_over_hip": round(res["torch"][0] / res["hip"][0], 2)})

    x = torch.rand(12, 3, 256, 256, device=dev)

    def fwd():
        with torch.no_grad():
            return disc(x)

    def fwd_bwd():
        for p in disc.parameters():
            p.grad = None
        loss = F.gan_loss(disc(x), True, is_disc=True)
        with F.batched_wgrad():
            loss.backward()
        return loss.detach()

    res = alternate({"fwd": graph_of(fwd), "fwd_bwd": graph_of(fwd_bwd)}, args.repeats)
    emit({"section": "UNetDiscriminatorSN 12x3x256x256 bf16", "forward_ms": res["fwd"], "forward_backward_ms": res["fwd_bwd"]})
    if not args.skip_step:
        gen = M.RRDBNet().to(dev).train()
        feat = pc.VggFeatureLoss({"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1.0, "conv4_4": 1.0, "conv5_4": 1.0}, "l1").to(dev)
        opt_g, opt_d = O.FusedAdam(gen.parameters(), lr=1e-4), O.FusedAdam(disc.parameters(), lr=1e-4)
        lq, gt = torch.rand(12, 3, 64, 64, device=dev), torch.rand(12, 3, 256, 256, device=dev)
        step = graph_of(lambda: S.realesrgan_step(gen, disc, feat, opt_g, opt_d, lq, gt), warmup=1)
        res = alternate({"step": step}, args.repeats)
        emit({"section": "realesrgan_step batch 12, 64x64 -> 256x256, RRDBNet 23 blocks (bf16)", "step_ms": res["step"],
              "losses": [float(v) for v in step.keep[:5]]})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
