"""What optim.WeightEMA costs, on one device:

  update   one ema.update() over the tensors of Generator(factor=4, residual_blocks_count=16) (parameters averaged, buffers
           copied), against torch.optim.swa_utils.AveragedModel.update_parameters with get_ema_multi_avg_fn on the same
           module and against a bare torch._foreach_lerp_ over the parameters alone, in alternating blocks; the bytes an
           update moves (two reads and one write per averaged element, one and one per copied one) over its time as GB/s.
  config2  HIP-graph replay of gen_l1_step (generator x4, batch 16, 32 x 32 -> 128 x 128) without and with ema=, two graphs
           in one process, in alternating blocks.

    python tools/microbench_ema.py [--out profiles/microbench_ema.txt]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep-super-resolution_amd"


def P(sub):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(PKG + "." + sub)


def timed(fn, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def summary(t):
    s = sorted(t)
    return {"median_ms": statistics.median(t), "p10_ms": s[len(s) // 10], "p90_ms": s[len(s) * 9 // 10], "n": len(t)}


def update(dev, out, reps, blocks):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    O = P("optim")
    gen = P("models.GAN.generator").Generator(4, 16).to(dev).train()
    ema = O.WeightEMA(gen, decay=0.999)
    avg = AveragedModel(gen, multi_avg_fn=get_ema_multi_avg_fn(0.999), use_buffers=False)
    params = [p.detach() for p in gen.parameters()]
    mirror = [p.clone() for p in params]
    runs = {"weight_ema_update": ema.update, "averaged_model_update_parameters": lambda: avg.update_parameters(gen),
            "foreach_lerp_parameters_only": lambda: torch._foreach_lerp_(mirror, params, 0.001)}
    for fn in runs.values():
        timed(fn, 10)                                # (also takes both past their copy-on-first-update step)
    times = {k: [] for k in runs}
    for _ in range(blocks):
        for k, fn in runs.items():
            times[k] += timed(fn, reps // blocks)
    res = {k: summary(v) for k, v in times.items()}
    n_par = sum(p.numel() for p in params)
    buf_bytes = sum(b.numel() * b.element_size() for b in gen.buffers())
    res.update(tensors=len(params) + len(list(gen.buffers())), parameter_elements=n_par,
               update_bytes=12 * n_par + 2 * buf_bytes)
    res["weight_ema_GBps"] = res["update_bytes"] / (res["weight_ema_update"]["median_ms"] * 1e-3) / 1e9
    res["averaged_model_over_weight_ema"] = (res["averaged_model_update_parameters"]["median_ms"] /
                                             res["weight_ema_update"]["median_ms"])
    res["foreach_lerp_over_weight_ema"] = (res["foreach_lerp_parameters_only"]["median_ms"] /
                                           res["weight_ema_update"]["median_ms"])
    out["update_generator_x4_16"] = res


def config2(dev, with_ema):
    O, S = P("optim"), P("steps")
    gen = P("models.GAN.generator").Generator(4, 16).to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(1)
    lr_in = torch.rand((16, 3, 32, 32), generator=g).to(dev)
    hr = (torch.rand((16, 3, 128, 128), generator=g) * 2 - 1).to(dev)
    opt = O.FusedAdam(gen.parameters(), lr=1e-4)
    ema = O.WeightEMA(gen, decay=0.999) if with_ema else None
    return S.GraphedStep(lambda: S.gen_l1_step(gen, opt, lr_in, hr, ema=ema))


def config2_cost(dev, out, replays, warm, blocks):
    sa, sb = config2(dev, False), config2(dev, True)
    timed(sa, warm)
    timed(sb, warm)
    ta, tb, ma, mb = [], [], [], []
    for _ in range(blocks):
        a, b = timed(sa, replays // blocks), timed(sb, replays // blocks)
        ta += a
        tb += b
        ma.append(statistics.median(a))
        mb.append(statistics.median(b))
    out["config2_graph_replay"] = dict(a_without_ema=summary(ta), b_with_ema=summary(tb), a_block_medians_ms=ma,
                                       b_block_medians_ms=mb, b_over_a=statistics.median(tb) / statistics.median(ta),
                                       ema_extra_ms=statistics.median(tb) - statistics.median(ta))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_ema.txt"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_ema needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    update(dev, out, a.reps, a.blocks)
    config2_cost(dev, out, a.replays, a.warm, a.blocks)
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(__doc__.split("\n\n")[0] + "\n\n" + txt + "\n")


if __name__ == "__main__":
    main()
