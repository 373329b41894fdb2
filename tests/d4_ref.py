"""Yardstick of the D4 kernels (csrc/d4.hip): the eight flips / quarter turns with torch on the CPU, and the self-ensemble mean.

Code k in 0..7, r = k % 4, m = k >= 4:  T_k(x) = rot90(flip(x, [-1]) if m else x, r, [-2, -1]) on [..., H, W];
T_k^-1(y) = flip(rot90(y, -r, [-2, -1]), [-1]) if m else rot90(y, -r, [-2, -1])."""
import numpy as np
import torch


def T(x, k):
    r, m = k % 4, k >= 4
    return torch.rot90(torch.flip(x, [-1]) if m else x, r, [-2, -1]).contiguous()


def T_inv(y, k):
    r, m = k % 4, k >= 4
    y = torch.rot90(y, -r, [-2, -1])
    return (torch.flip(y, [-1]) if m else y).contiguous()


def gather(x, k):
    """T_k by the index table: T_k(x)[i, j] = x[a, b], H and W the source's sizes (an independent restatement of T)."""
    H, W = x.shape[-2:]
    r, m = k % 4, k >= 4
    oh, ow = (H, W) if r % 2 == 0 else (W, H)
    out = torch.empty(tuple(x.shape[:-2]) + (oh, ow), dtype=x.dtype)
    for i in range(oh):
        for j in range(ow):
            a, b = [(i, j), (j, W - 1 - i), (H - 1 - i, W - 1 - j), (H - 1 - j, i)][r]
            if m:
                b = W - 1 - b
            out[..., i, j] = x[..., a, b]
    return out


def ensemble_mean(outputs, codes):
    """fp32 sum of `outputs` (already turned back; outputs[n] belongs to codes[n]) in ASCENDING code order, times the fp32
    value of 1 / len -- the order and the single multiply are the contract of dsr_d4_mean_f32."""
    order = sorted(range(len(codes)), key=lambda n: codes[n])
    assert len(set(codes)) == len(codes) == len(outputs)
    acc = outputs[order[0]].to(torch.float32).clone()
    for n in order[1:]:
        acc = acc + outputs[n].to(torch.float32)
    return acc * float(np.float32(1.0) / np.float32(len(codes)))


def codes_of(mask):
    return [k for k in range(8) if mask >> k & 1]
