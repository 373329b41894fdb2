"""Device-event time of the five-tap Real-ESRGAN content loss, forward + backward to the image, at [32, 3, 128, 128] (bf16):
  fused      perceptual.VggFeatureLoss({conv1_2: .1, conv2_2: .1, conv3_4: 1, conv4_4: 1, conv5_4: 1}, 'l1', range_norm=True):
             one tap pass per layer on the 16-bit NHWC map (csrc/featloss.hip), ReLU written / masked inside the tap launches
  assembled  the same loss from the pieces that existed before that module: per tapped layer the convolution without its
             activation -> functional.ToNCHW (an fp32 NCHW copy of the map) -> functional.l1_loss; the ReLU in front of the
             next layer, its backward pass and the add of the two gradients that meet at the tapped map are torch's;
             scale_loss / add_losses for the weighted sum
Both share the trunk's weights, the target's taps are computed ahead of the timed window (as steps.gan_step does on its side
stream) and handed in; the timed call is loss forward + backward down to image1.grad.

    python tools/microbench_vggfeat.py [--repeats 30] [--warmup 5] [--out profiles/microbench_vggfeat.txt]

The shape is warmed up first; the timed repeats run the two calls in turn (they alternate within one run), each between its
own pair of HIP events with a synchronise after it.  Reported per call: median, min and max over the repeats, and how far the
two losses and image gradients are apart.  A table of what was measured; there is no pass bar."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=4, default=[32, 3, 128, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microbench_vggfeat.txt"))
    args = ap.parse_args()
    pc = importlib.import_module(PKG + ".perceptual")
    F = importlib.import_module(PKG + ".functional")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    shape = tuple(args.shape)
    emit({"shape": list(shape), "layers": LAYERS, "criterion": "l1", "range_norm": True, "dtype": "bfloat16",
          "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)})
    g = torch.Generator().manual_seed(0)
    hr = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
    fake = (hr.cpu() + 0.1 * torch.randn(shape, generator=g)).clamp(-1, 1).to(dev)
    m = pc.VggFeatureLoss(LAYERS, "l1", range_norm=True).to(dev)
    feats = m.target_features(hr)
    feats_nchw = [F.ToNCHW.apply(t, t.shape[-1]) for t in feats]      # the assembled form compares fp32 NCHW copies
    convs = m._convs()
    tap_of = {o: i for i, (o, _, _, _) in enumerate(m.taps)}
    pools = pc._POOL_AFTER
    keep = {}

    def fused():
        x = fake.detach().requires_grad_(True)
        loss = m(x, None, feats)
        loss.backward()
        keep["fused"] = (loss.detach(), x.grad)

    def assembled():
        x = fake.detach().requires_grad_(True)
        h = m._input(x)
        link = None
        loss = None
        for k, conv in enumerate(convs):
            i = tap_of.get(k)
            if i is None:
                out_link = F.Handover()
                h = F.ConvAct.apply(h, conv.weight, conv.bias, None, dict(stride=1, pad=1, act=F.ACT_RELU, in_link=link, out_link=out_link))
                link = out_link
            else:
                y = F.ConvAct.apply(h, conv.weight, conv.bias, None, dict(stride=1, pad=1, act=F.ACT_NONE, in_link=link))
                term = F.scale_loss(F.l1_loss(F.ToNCHW.apply(y, conv.out_channels), feats_nchw[i]), m.taps[i][3])
                loss = term if loss is None else F.add_losses(loss, term)
                h = torch.relu(y)
                link = None
            if k in pools and k != len(convs) - 1:
                h = F.MaxPool2.apply(h, link)
                link = None
        loss.backward()
        keep["assembled"] = (loss.detach(), x.grad)

    calls = {"fused": fused, "assembled": assembled}
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
        emit({"call": k, "median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)})
    emit({"fused_over_assembled_median": round(statistics.median(times["fused"]) / statistics.median(times["assembled"]), 4)})
    (lf, gf), (la, ga) = keep["fused"], keep["assembled"]
    cosv = float((gf.double().flatten() @ ga.double().flatten()) / (gf.double().norm() * ga.double().norm()))
    emit({"loss_fused": float(lf), "loss_assembled": float(la), "loss_rel_diff": abs(float(lf) - float(la)) / abs(float(la)),
          "grad_one_minus_cos": 1.0 - cosv, "grad_norm_ratio": float(gf.norm() / ga.norm())})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
