#!/usr/bin/env python3
"""Golden vectors for the top-n_min branch of ``OhemCELoss`` behind the final upsample at the reference's real threshold,
produced by running the REFERENCE (src/utils/loss.py:11-83, weights from src/utils/class_weights.py:77-90) in float64 on the
materialised ``F.interpolate`` output (cabinet.py:240-245).

Needs a checkout of the reference:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ohem_topk.py REFERENCE_ROOT
Writes g7_ohem_topk.npz, data only.  Every head is shaped like late training: low-resolution logits that are SCALE x one-hot of a
class map of vertical stripes (plus, where NOISE > 0, a little noise), labels = that class map at full resolution with a small
share of pixels flipped to a wrong class (the hard pixels) and ~10 % ignored; thresh = 0.7, n_min = B*H*W/16.  Bilinear
upsampling of such logits gives a discrete ladder of losses at the stripe borders (x8, scale 40: e^-35, e^-25, 3e-7, 7e-3, 5, ...)
and 0 or SCALE elsewhere, so fewer than n_min pixels are above the threshold and the n_min-th hardest sits among saturated ones.

  a   8 classes, unweighted, x8 with Wl = 64 (the row kernel's shape)
  b   19 classes, ENet weights (scaled to a maximum of 1) with one occurring class at weight 0, x4 (the segment kernel, general ratio)
  c   a pair over the same labels: head 0 late training (top-n_min branch), head 1 random logits (n_min above thresh)
  d   the tie at zero: exact one-hot logits, fewer than k non-zero losses

Per head ``<case>.h<i>``: low, weight (absent = unweighted), loss, dlow, n_valid, n_above, t (the k-th largest loss), branch
("topk" | "sel").  Asserted before anything is written (tests/test_ohem_topk.py re-checks them on the stored data):
  (i)   no valid pixel has |l - thresh| < 1e-5;
  (ii)  topk heads, DELTA = 1e-4: every valid pixel other than the k-th itself with |l - t| <= DELTA has l <= 1e-6 -- what is near
        the k-th value is saturated, its softmax - onehot is ~1e-6, and which of those pixels an fp32 kernel keeps cannot move a
        gradient element by 1e-3;
  (iii) DELTA >= 10 x the largest |l_fp32 - l_fp64| over the valid pixels (per-pixel loss evaluated in fp32 on the CPU);
  (iv)  case d: in fp32 the k-th largest loss is exactly 0 and more than one pixel equals it.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
from src.utils.class_weights import compute_class_weights  # noqa: E402
from src.utils.loss import OhemCELoss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
IGNORE, THRESH, GAP, DELTA, SAT = 255, 0.7, 1e-5, 1e-4, 1e-6
# name: (B, C, Hl, Wl, H, W), seed, logit scale, noise sd, share of flipped labels, stripe width (source columns), weighted
CASES = {
    "a": ((1, 8, 8, 64, 64, 512), 11, 40.0, 0.25, 0.01, 4, False),
    "b": ((2, 19, 12, 40, 48, 160), 12, 24.0, 0.25, 0.01, 10, True),
    "c": ((1, 8, 4, 64, 32, 512), 13, 40.0, 0.25, 0.01, 4, False),
    "d": ((1, 8, 4, 64, 32, 512), 14, 40.0, 0.0, 0.002, 8, False),
}


def px_loss(low, labels, size, w, dtype):
    up = F.interpolate(low.to(dtype), size=size, mode="bilinear", align_corners=False)
    return F.cross_entropy(up, labels, weight=None if w is None else w.to(dtype), ignore_index=IGNORE, reduction="none")


def late_training_head(shape, g, scale, noise, stripe):
    B, C, Hl, Wl, H, W = shape
    cls_low = ((torch.arange(Wl) // stripe) * 5 % C).view(1, 1, Wl).expand(B, Hl, Wl)        # vertical stripes of classes
    low = scale * F.one_hot(cls_low, C).permute(0, 3, 1, 2).float()
    if noise > 0:
        low = low + noise * torch.randn(B, C, Hl, Wl, generator=g)
    cls_full = ((torch.arange(W) * Wl // W // stripe) * 5 % C).view(1, 1, W).expand(B, H, W).contiguous()
    return low.contiguous(), cls_full


out = dict(ignore_lb=np.int64(IGNORE), thresh=np.float64(THRESH), gap=np.float64(GAP), delta=np.float64(DELTA),
           sat=np.float64(SAT), cases=np.array(sorted(CASES)))
for name, (shape, seed, scale, noise, flip, stripe, weighted) in sorted(CASES.items()):
    B, C, Hl, Wl, H, W = shape
    g = torch.Generator().manual_seed(seed)
    low, cls_full = late_training_head(shape, g, scale, noise, stripe)
    labels = cls_full.clone()
    hard = torch.rand(B, H, W, generator=g) < flip
    labels[hard] = (cls_full[hard] + 1 + torch.randint(0, C - 1, (int(hard.sum()),), generator=g)) % C
    labels[torch.rand(B, H, W, generator=g) < 0.10] = IGNORE
    n_min = B * H * W // 16
    heads = [("topk", low)]
    if name == "c":
        heads.append(("sel", (torch.randn(B, C, Hl, Wl, generator=g) * 2.0).contiguous()))
    weight = None
    if weighted:
        counts = np.bincount(labels[labels != IGNORE].numpy(), minlength=C)
        # divided by their maximum: the reference's weights are >= 1 (up to 7), and w * 24 evaluated in fp32 would be off by
        # more than DELTA / 10 (condition iii); the kernels take any non-negative table
        weight = compute_class_weights(counts, 0.5)
        weight = (weight / weight.max()).astype(np.float32)
        zero = int(cls_full[0, 0, W // 2])                       # a class that occurs and weighs nothing
        assert counts[zero] > 0
        weight[zero] = 0.0
        out[f"{name}.weight"] = weight
    w64 = None if weight is None else torch.from_numpy(weight).double()
    out.update({f"{name}.labels": labels.numpy().astype(np.uint8), f"{name}.size": np.array([H, W], dtype=np.int64),
                f"{name}.n_min": np.int64(n_min), f"{name}.n_heads": np.int64(len(heads))})
    valid = labels != IGNORE
    n_valid = int(valid.sum())
    k = min(n_min, n_valid)
    for hi, (branch, lw) in enumerate(heads):
        x = lw.double().requires_grad_(True)
        up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
        loss = OhemCELoss(THRESH, n_min, IGNORE, weight=w64)(up, labels)
        loss.backward()
        l64 = px_loss(lw, labels, (H, W), w64, torch.float64)[valid]
        l32 = px_loss(lw, labels, (H, W), None if weight is None else torch.from_numpy(weight), torch.float32)[valid]
        err32 = float((l32.double() - l64).abs().max())
        n_above = int((l64 > THRESH).sum())
        gap = float((l64 - THRESH).abs().min())
        assert gap >= GAP, (name, hi, gap)                                              # (i)
        assert (n_above >= k) == (branch == "sel"), (name, hi, n_above, k)
        assert DELTA >= 10 * err32, (name, hi, err32)                                   # (iii)
        srt = torch.sort(l64, descending=True).values
        t = float(srt[k - 1])
        line = f"case {name} head {hi} {branch}: loss {loss.item():.9f} n_valid {n_valid} n_above {n_above} k {k} gap {gap:.3e} " \
               f"fp32 err {err32:.3e}"
        if branch == "topk":
            near = (l64 - t).abs() <= DELTA
            n_near = int(near.sum())
            # the k-th itself is one of them; all others must be saturated
            unsat = int((near & (l64 > SAT)).sum()) - (1 if t > SAT else 0)
            assert unsat <= 0, (name, hi, t, n_near, unsat)                            # (ii)
            s32 = torch.sort(l32, descending=True).values
            t32, n_eq32 = float(s32[k - 1]), int((l32 == s32[k - 1]).sum())
            line += f" t {t:.3e} near {n_near} n(l > 1e-6) {int((l64 > SAT).sum())} fp32: t {t32:.3e} n_eq {n_eq32}"
            if name == "d":
                assert t32 == 0.0 and n_eq32 > 1 and int((l32 != 0).sum()) < k, (t32, n_eq32)   # (iv)
        print(line)
        out.update({f"{name}.h{hi}.low": lw.numpy(), f"{name}.h{hi}.loss": np.float64(loss.item()),
                    f"{name}.h{hi}.dlow": x.grad.numpy().astype(np.float32), f"{name}.h{hi}.n_valid": np.int64(n_valid),
                    f"{name}.h{hi}.n_above": np.int64(n_above), f"{name}.h{hi}.t": np.float64(t),
                    f"{name}.h{hi}.branch": np.array(branch)})
path = os.path.join(HERE, "g7_ohem_topk.npz")
np.savez_compressed(path, **out)
print("wrote g7_ohem_topk.npz", os.path.getsize(path))
