#!/usr/bin/env python3
"""Golden vectors for the class-weighted ``OhemCELoss`` behind the final upsample, produced by running the REFERENCE
(src/utils/loss.py:11-83 with ``weight=``, src/utils/class_weights.py:77-90) in float64 on the materialised
``F.interpolate`` output (cabinet.py:240-245).

Build container only (needs /root/reference):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ohem_weighted.py
Writes g6_ohem_weighted.npz, data only.  Per case ``c<i>``: low-resolution logits, labels (uint8, 255 = ignored) drawn from
a skewed class distribution, ``weight`` = compute_class_weights(pixel counts, 0.5) rounded to fp32 with one occurring class
set to 0, ``n_min``, and for ``sel`` (thresh 0.7: "at least n_min pixels above thresh") and ``topk`` (a threshold nothing
exceeds: the n_min hardest) the loss, dlow, n_valid, n_above and thresh.

Conditions asserted before anything is written (tests/test_ohem_weighted.py re-checks them on the stored data): no valid
pixel has |w * ce - thresh| < 1e-5 (an fp32 kernel selects the float64 reference's set), and n_above >= n_min for ``sel``.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
from src.utils.class_weights import compute_class_weights  # noqa: E402
from src.utils.loss import OhemCELoss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(2, 19, 12, 20, 96, 160), (2, 8, 16, 16, 128, 128)]
SEED, IGNORE, GAP = 0, 255, 1e-5
BRANCHES = (("sel", 0.7), ("topk", 1e4))

out = dict(ignore_lb=np.int64(IGNORE), gap=np.float64(GAP), n_cases=np.int64(len(CASES)))
for ci, (B, C, Hl, Wl, H, W) in enumerate(CASES):
    g = torch.Generator().manual_seed(SEED + ci)
    low = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    prior = 0.7 ** torch.arange(C, dtype=torch.float64)          # skewed: class k is 0.7 x as frequent as class k - 1
    labels = torch.multinomial(prior / prior.sum(), B * H * W, replacement=True, generator=g).view(B, H, W)
    labels[torch.rand(B, H, W, generator=g) < 0.15] = IGNORE
    counts = np.bincount(labels[labels != IGNORE].numpy(), minlength=C)
    weight = compute_class_weights(counts, 0.5).astype(np.float32)
    assert counts[1] > 0
    weight[1] = 0.0                                               # a class that occurs and weighs nothing
    w64 = torch.from_numpy(weight).double()
    n_min = B * H * W // 16
    out.update({f"c{ci}.low": low.numpy(), f"c{ci}.labels": labels.numpy().astype(np.uint8), f"c{ci}.weight": weight,
                f"c{ci}.size": np.array([H, W], dtype=np.int64), f"c{ci}.n_min": np.int64(n_min),
                f"c{ci}.counts": counts.astype(np.int64)})
    for tag, thresh in BRANCHES:
        x = low.double().requires_grad_(True)
        up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
        loss = OhemCELoss(thresh, n_min, IGNORE, weight=w64)(up, labels)
        loss.backward()
        px = F.cross_entropy(up.detach(), labels, weight=w64, ignore_index=IGNORE, reduction="none")
        valid = labels != IGNORE
        n_valid, n_above = int(valid.sum()), int(((px > thresh) & valid).sum())
        gap = float((px[valid] - thresh).abs().min())
        assert gap >= GAP, (ci, tag, gap)
        assert (n_above >= n_min) == (tag == "sel"), (ci, tag, n_above, n_min)
        print(f"case {ci} {tag}: loss {loss.item():.9f} n_valid {n_valid} n_above {n_above} n_min {n_min} min gap {gap:.3e}")
        out.update({f"c{ci}.{tag}.loss": np.float64(loss.item()), f"c{ci}.{tag}.dlow": x.grad.numpy(),
                    f"c{ci}.{tag}.n_valid": np.int64(n_valid), f"c{ci}.{tag}.n_above": np.int64(n_above),
                    f"c{ci}.{tag}.thresh": np.float64(thresh)})
path = os.path.join(HERE, "g6_ohem_weighted.npz")
np.savez_compressed(path, **out)
print("wrote g6_ohem_weighted.npz", os.path.getsize(path))
