#!/usr/bin/env python3
"""Golden vectors for ``SoftmaxFocalLoss`` behind the final upsample, produced by running the REFERENCE
(src/utils/loss.py:86-127, src/utils/class_weights.py:77-90) in float64 on the materialised ``F.interpolate`` output
(cabinet.py:240-245).

Build container only (needs /root/reference):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_focal_up.py
Writes g11_focal_up.npz, data only.  Per case ``c<i>``: low-resolution logits, labels (uint8, 255 = ignored: 15 % of the
pixels) drawn from a skewed class distribution, ``weight`` = compute_class_weights(pixel counts, 0.5) rounded to fp32 with one
occurring class set to 0, and for every weight mode ``nw`` (none) / ``w`` and every gamma ``g<k>`` of ``gammas`` the loss
(float64) and dlow (stored as fp32: the file stays small).

The last case (``conf`` = its index) has constant low-logit blocks: a column band whose class 0 logit towers 30 above the
others, labelled 0 in its upper and 1 in its lower half -- pixels with p_t > 1 - 1e-6 (q = 1 - p_t loses every digit in a naive
fp32 ``1 - exp(-l)``) and with p_t < 1e-6.  Both counts are asserted >= 64 before anything is written
(tests/test_focal_up.py re-checks them on the stored data).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
from src.utils.class_weights import compute_class_weights  # noqa: E402
from src.utils.loss import SoftmaxFocalLoss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(1, 5, 7, 9, 40, 50),        # general ratio
         (2, 19, 12, 20, 96, 160),    # x8: segment kernel + y8
         (1, 8, 2, 64, 16, 512),      # x8: whole-row kernel
         (1, 4, 6, 8, 48, 64)]        # confident / hopeless pixels (constant blocks)
CONF = 3
GAMMAS = (0.0, 0.5, 2.0, 5.0)
SEED, IGNORE, NEED = 0, 255, 64

out = dict(ignore_lb=np.int64(IGNORE), n_cases=np.int64(len(CASES)), gammas=np.array(GAMMAS, dtype=np.float64),
           conf=np.int64(CONF))
for ci, (B, C, Hl, Wl, H, W) in enumerate(CASES):
    g = torch.Generator().manual_seed(SEED + ci)
    low = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    prior = 0.7 ** torch.arange(C, dtype=torch.float64)          # skewed: class k is 0.7 x as frequent as class k - 1
    labels = torch.multinomial(prior / prior.sum(), B * H * W, replacement=True, generator=g).view(B, H, W)
    if ci == CONF:
        low[:, :, :, :3] = 0.0
        low[:, 0, :, :3] = 30.0
        labels[:, :H // 2, :16] = 0
        labels[:, H // 2:, :16] = 1
    labels[torch.rand(B, H, W, generator=g) < 0.15] = IGNORE
    valid = labels != IGNORE
    counts = np.bincount(labels[valid].numpy(), minlength=C)
    weight = compute_class_weights(counts, 0.5).astype(np.float32)
    zero_cls = 2 if ci == CONF else 1
    assert counts[zero_cls] > 0
    weight[zero_cls] = 0.0                                        # a class that occurs and weighs nothing
    w64 = torch.from_numpy(weight).double()
    up = F.interpolate(low.double(), size=(H, W), mode="bilinear", align_corners=False)
    p_t = torch.softmax(up, 1).gather(1, labels.clamp(max=C - 1).unsqueeze(1)).squeeze(1)
    n_conf, n_hopeless = int(((p_t > 1 - 1e-6) & valid).sum()), int(((p_t < 1e-6) & valid).sum())
    if ci == CONF:
        assert n_conf >= NEED and n_hopeless >= NEED, (n_conf, n_hopeless)
    out.update({f"c{ci}.low": low.numpy(), f"c{ci}.labels": labels.numpy().astype(np.uint8), f"c{ci}.weight": weight,
                f"c{ci}.size": np.array([H, W], dtype=np.int64), f"c{ci}.counts": counts.astype(np.int64),
                f"c{ci}.n_conf": np.int64(n_conf), f"c{ci}.n_hopeless": np.int64(n_hopeless)})
    for wtag, w in (("nw", None), ("w", w64)):
        for gi, gamma in enumerate(GAMMAS):
            x = low.double().requires_grad_(True)
            upx = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
            loss = SoftmaxFocalLoss(gamma, weight=w, ignore_lb=IGNORE)(upx, labels)
            loss.backward()
            assert torch.isfinite(loss) and torch.isfinite(x.grad).all(), (ci, wtag, gamma)
            print(f"case {ci} {wtag} gamma {gamma}: loss {loss.item():.12f} |dlow|max {x.grad.abs().max().item():.3e} "
                  f"n_conf {n_conf} n_hopeless {n_hopeless}")
            out.update({f"c{ci}.{wtag}.g{gi}.loss": np.float64(loss.item()),
                        f"c{ci}.{wtag}.g{gi}.dlow": x.grad.numpy().astype(np.float32)})
path = os.path.join(HERE, "g11_focal_up.npz")
np.savez_compressed(path, **out)
print("wrote g11_focal_up.npz", os.path.getsize(path))
