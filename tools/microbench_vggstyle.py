"""Device-event time of the five-tap Real-ESRGAN perceptual loss with and without its style (Gram-matrix) term, bf16, at
[12, 3, 256, 256] and [16, 3, 128, 128], forward alone and forward + backward to the image:
  off            perceptual.VggFeatureLoss(LAYERS, 'l1', range_norm=True): the content term alone (csrc/featloss.hip)
  on             the same with style_weight = 1: Gram matrices by MFMA on the 16-bit NHWC maps, the style gradient inside the
                 tap's one backward launch (functional.FeatureStyleTap, csrc/featstyle.hip)
  assembled_off  the content term from the pieces that existed before either module: per tapped layer the convolution without
                 its activation -> functional.ToNCHW (an fp32 NCHW copy of the map) -> functional.l1_loss, torch's ReLU
  assembled_on   assembled_off plus the style term from that fp32 NCHW copy: torch.bmm each way and torch's l1_loss
All four share the trunk's weights; the target's taps and Gram matrices are computed ahead of the timed window and handed in.
Per tap, the Gram matrix alone is also timed both ways: functional.gram16 against ToNCHW + torch.bmm.

    python tools/microbench_vggstyle.py [--repeats 30] [--warmup 3] [--out profiles/microbench_vggstyle.txt]

Every shape is warmed up first; the timed repeats run the calls in turn (they alternate within one run), each between its own
pair of HIP events with a synchronise after it.  Reported per call: median, min and max over the repeats.  A table of what
was measured; there is no pass bar."""
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
LAYERS = {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1.0, "conv4_4": 1.0, "conv5_4": 1.0}
SHAPES = [(12, 3, 256, 256), (16, 3, 128, 128)]


def timed(calls, repeats, warmup):
    for f in calls.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_vggstyle.txt"))
    args = ap.parse_args()
    pc = importlib.import_module(PKG + ".perceptual")
    F = importlib.import_module(PKG + ".functional")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit({"layers": LAYERS, "criterion": "l1", "range_norm": True, "dtype": "bfloat16", "style_weight": 1.0,
          "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)})
    for shape in SHAPES:
        g = torch.Generator().manual_seed(0)
        hr = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
        fake = (hr.cpu() + 0.1 * torch.randn(shape, generator=g)).clamp(-1, 1).to(dev)
        off = pc.VggFeatureLoss(LAYERS, "l1", range_norm=True).to(dev)
        on = pc.VggFeatureLoss(LAYERS, "l1", range_norm=True, style_weight=1.0).to(dev)
        feats = on.target_features(hr)
        grams = on.target_grams(feats)
        feats_nchw = [F.ToNCHW.apply(t, t.shape[-1]) for t in feats]
        convs = on._convs()
        tap_of = {o: i for i, (o, _, _, _) in enumerate(on.taps)}
        pools = pc._POOL_AFTER
        keep = {}

        def fused(mod, name, backward):
            def run():
                x = fake.detach().requires_grad_(backward)
                loss = mod(x, None, feats, grams) if mod is on else mod(x, None, feats)
                if backward:
                    loss.backward()
                    keep[name] = (loss.detach(), x.grad)
            return run

        def assembled(style, name, backward):
            def run():
                x = fake.detach().requires_grad_(backward)
                h = on._input(x)
                link = None
                loss = None
                for k, conv in enumerate(convs):
                    i = tap_of.get(k)
                    if i is None:
                        out_link = F.Handover()
                        h = F.ConvAct.apply(h, conv.weight, conv.bias, None,
                                            dict(stride=1, pad=1, act=F.ACT_RELU, in_link=link, out_link=out_link))
                        link = out_link
                    else:
                        y = F.ConvAct.apply(h, conv.weight, conv.bias, None, dict(stride=1, pad=1, act=F.ACT_NONE, in_link=link))
                        c = conv.out_channels
                        y32 = F.ToNCHW.apply(y, c)
                        term = F.scale_loss(F.l1_loss(y32, feats_nchw[i]), on.taps[i][3])
                        loss = term if loss is None else F.add_losses(loss, term)
                        if style:
                            m = y32.reshape(y32.shape[0], c, -1)
                            gram = torch.bmm(m, m.transpose(1, 2)) / float(c * m.shape[2])
                            loss = loss + on.taps[i][3] * torch.nn.functional.l1_loss(gram, grams[i])
                        h = torch.relu(y)
                        link = None
                    if k in pools and k != len(convs) - 1:
                        h = F.MaxPool2.apply(h, link)
                        link = None
                if backward:
                    loss.backward()
                    keep[name] = (loss.detach(), x.grad)
            return run

        for backward in (False, True):
            calls = {"off": fused(off, "off", backward), "on": fused(on, "on", backward),
                     "assembled_off": assembled(False, "assembled_off", backward),
                     "assembled_on": assembled(True, "assembled_on", backward)}
            times = timed(calls, args.repeats, args.warmup)
            med = {k: statistics.median(ts) for k, ts in times.items()}
            for k, ts in times.items():
                emit({"shape": list(shape), "pass": "fwd+bwd" if backward else "fwd", "call": k, "median_ms": round(med[k], 4),
                      "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)})
            emit({"shape": list(shape), "pass": "fwd+bwd" if backward else "fwd",
                  "style_cost_fused_ms": round(med["on"] - med["off"], 4),
                  "style_cost_assembled_ms": round(med["assembled_on"] - med["assembled_off"], 4)})
        (lf, gf), (la, ga) = keep["on"], keep["assembled_on"]
        cosv = float((gf.double().flatten() @ ga.double().flatten()) / (gf.double().norm() * ga.double().norm()))
        emit({"shape": list(shape), "loss_on": float(lf), "loss_assembled_on": float(la),
              "loss_rel_diff": abs(float(lf) - float(la)) / abs(float(la)), "grad_one_minus_cos": 1.0 - cosv,
              "grad_norm_ratio": float(gf.norm() / ga.norm())})
        # the Gram matrix alone, per tap
        for t, (o, _, name, _) in zip(feats, on.taps):
            c = convs[o].out_channels

            def ours(t=t, c=c):
                F.gram16(t, c)

            def torchs(t=t, c=c):
                m = F.ToNCHW.apply(t, c).reshape(t.shape[0], c, -1)
                torch.bmm(m, m.transpose(1, 2)) / float(c * m.shape[2])

            times = timed({"gram16": ours, "tonchw_bmm": torchs}, args.repeats, args.warmup)
            emit({"shape": list(shape), "tap": name, "map": list(t.shape),
                  "gram16_median_ms": round(statistics.median(times["gram16"]), 4),
                  "tonchw_bmm_median_ms": round(statistics.median(times["tonchw_bmm"]), 4)})
        del feats, grams, feats_nchw, keep
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
