"""Yardstick for optim.WeightEMA: the averaging recurrence in float64 over a list of snapshots of a model's tensors.

The weight of every step is an exact rational (fractions.Fraction of the decay's own binary value) rounded once to float64:
    warmup=False  torch.optim.swa_utils.AveragedModel + get_ema_multi_avg_fn(decay): the first update copies, later ones
                  do  shadow += (1 - decay) * (p - shadow)
    warmup=True   timm / torch-ema: update number k = n_averaged + 1 uses d_k = min(decay, (1 + k) / (10 + k)); no copy step,
                  the shadow starts as the copy of the tensors handed to the constructor
Buffers: use_buffers=False copies every buffer from the snapshot at each update (torch); use_buffers=True averages the
floating-point ones like parameters and COPIES the integer ones (WeightEMA's documented departure from torch, which truncates
the lerp to an integer).  A step flagged skipped moves nothing, the count of averaged steps included.
tests/test_host_ema.py pins this file to torch's AveragedModel."""
from fractions import Fraction

import numpy as np


def decay_at(decay, n_averaged, warmup):
    """The decay d of the update that finds `n_averaged` earlier ones, as a Fraction (the update is s += (1 - d) * (p - s));
    None where the update is the plain copy."""
    d = Fraction(decay)
    if not warmup:
        return None if n_averaged == 0 else d
    k = n_averaged + 1
    return min(d, Fraction(1 + k, 10 + k))


def _is_int(a):
    return np.issubdtype(np.asarray(a).dtype, np.integer)


class EmaRef:
    def __init__(self, start, buffers=(), decay=0.999, warmup=False, use_buffers=False):
        """`start`: {name: array}, the tensors at construction; `buffers`: the names that are buffers."""
        self.decay, self.warmup, self.use_buffers = decay, bool(warmup), bool(use_buffers)
        self.buffers = set(buffers)
        self.shadow = {k: (np.array(v) if _is_int(v) else np.array(v, dtype=np.float64)) for k, v in start.items()}
        self.n_averaged = 0

    def copied(self, name):
        return name in self.buffers and not (self.use_buffers and not _is_int(self.shadow[name]))

    def update(self, snapshot, skipped=False):
        if skipped:
            return
        d = decay_at(self.decay, self.n_averaged, self.warmup)
        for name, s in self.shadow.items():
            p = np.asarray(snapshot[name])
            if d is None or self.copied(name):
                self.shadow[name] = np.array(p) if _is_int(p) else np.array(p, dtype=np.float64)
            else:
                self.shadow[name] = s + float(1 - d) * (p.astype(np.float64) - s)
        self.n_averaged += 1


def run(start, snapshots, buffers=(), decay=0.999, warmup=False, use_buffers=False, skipped=()):
    """The shadow after every snapshot (a list of {name: array}) and the final count; `skipped`: indices of skipped steps."""
    ref = EmaRef(start, buffers, decay, warmup, use_buffers)
    out = []
    for i, snap in enumerate(snapshots):
        ref.update(snap, skipped=i in skipped)
        out.append({k: v.copy() for k, v in ref.shadow.items()})
    return out, ref.n_averaged
