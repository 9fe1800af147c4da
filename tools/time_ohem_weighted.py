#!/usr/bin/env python3
"""Pair forward + backward of the fused OHEM head, unweighted / class-weighted / composite weighted, in one process.

    python tools/time_ohem_weighted.py [--rounds 5] [--replays 100] [--configs 3,5] [--json OUT]
    python tools/time_ohem_weighted.py --package-root DIR      # import cabinet_amd from another checkout (A/B against a
                                                               # build without the weighted entry points: unweighted only)
    python tools/time_ohem_weighted.py --variants unweighted   # the same sequence of work as such a build runs: what ran just
                                                               # before a variant (the composite moves GBs) shifts it by a few %

Configurations: 3 = 8 x 8 x 128 x 128 -> 1024^2, 5 = 2 x 19 x 256 x 128 -> 2048 x 1024.  Per configuration the
variants alternate round by round (clock and cache state drift alike for all of them):
  unweighted  ohem_up_pair_fwd_hip / ohem_up_pair_bwd_hip, forward group and backward group each captured in a hipGraph
  weighted    the same with one ENet-style weight table per head
  composite   what weighted criteria ran before the kernels took weights: F.interpolate of both heads + OhemCELoss.forward +
              backward.  Its branch decision reads the device (a host sync), so it cannot be captured: timed eagerly (its
              kernels take milliseconds, launch overhead does not show).
Device events around `replays` replays after a warm-up; the median over rounds and the min .. max spread are printed in us.
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replays", type=int, default=100)
ap.add_argument("--configs", default="3,5")
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--variants", default="unweighted,weighted,composite")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cabinet_amd import _lib, functional as Fn  # noqa: E402
from cabinet_amd.loss import OhemCELoss  # noqa: E402

CONFIGS = {"3": (8, 8, 128, 128, 1024, 1024), "5": (2, 19, 256, 128, 2048, 1024)}
HAS_WEIGHTS = "cabinet_ohem_up_pair_w_fwd" in _lib.SIGNATURES
WANT = set(args.variants.split(",")) if HAS_WEIGHTS else {"unweighted"}


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def graphed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, keep


def enet_weights(C, seed):
    p = 0.7 ** np.random.RandomState(seed).permutation(C)
    p = p / p.sum()
    return torch.tensor((1.0 / np.log(1.02 + p)) ** 0.5, dtype=torch.float32, device="cuda")


results = {"package_root": os.path.abspath(args.package_root), "weighted_entry_points": HAS_WEIGHTS, "variants": sorted(WANT),
           "rounds": args.rounds, "replays": args.replays, "device": torch.cuda.get_device_name(0), "configs": {}}
for key in args.configs.split(","):
    B, C, Hl, Wl, H, W = CONFIGS[key]
    g = torch.Generator().manual_seed(0)
    la = (torch.randn(B, C, Hl, Wl, generator=g) * 2).cuda()
    lb = (torch.randn(B, C, Hl, Wl, generator=g) * 2).cuda()
    lab = torch.randint(0, C, (B, H, W), generator=g).cuda()
    size, n_min = (H, W), B * H * W // 16
    variants = {}

    def fused(wa, wb):
        kw = dict(weight_a=wa, weight_b=wb) if HAS_WEIGHTS else {}
        gf, (loss_px, stats) = graphed(lambda: Fn.ohem_up_pair_fwd_hip(la, lb, lab, size, 0.7, 255, **kw))
        gb, _ = graphed(lambda: Fn.ohem_up_pair_bwd_hip(la, lb, lab, loss_px, size, 0.7, 255, 1e-6, **kw))
        return gf, gb

    if "unweighted" in WANT:
        variants["unweighted"] = fused(None, None)
    if HAS_WEIGHTS:
        wa, wb = enet_weights(C, 1), enet_weights(C, 2)
    if "weighted" in WANT:
        variants["weighted"] = fused(wa, wb)
    if "composite" in WANT:
        ca, cb = OhemCELoss(0.7, n_min, 255, weight=wa.clone()).cuda(), OhemCELoss(0.7, n_min, 255, weight=wb.clone()).cuda()
        xa, xb = la.clone().requires_grad_(True), lb.clone().requires_grad_(True)

        def composite():
            xa.grad = xb.grad = None
            up_a = F.interpolate(xa, size=size, mode="bilinear", align_corners=False)
            up_b = F.interpolate(xb, size=size, mode="bilinear", align_corners=False)
            (ca.forward(up_a, lab) + cb.forward(up_b, lab)).backward()

        for _ in range(3):
            composite()
    times = {}
    for r in range(args.rounds):
        for name, (gf, gb) in variants.items():
            times.setdefault(name + ".fwd", []).append(events(gf.replay, args.replays))
            times.setdefault(name + ".bwd", []).append(events(gb.replay, args.replays))
        if "composite" in WANT:
            times.setdefault("composite.fwd+bwd", []).append(events(composite, max(10, args.replays // 10)))
    print(f"config {key}: B={B} C={C} {Hl}x{Wl} -> {H}x{W}   ({args.rounds} rounds x {args.replays} replays, us)")
    out = {}
    for name, ts in times.items():
        out[name] = dict(median=round(statistics.median(ts), 2), min=round(min(ts), 2), max=round(max(ts), 2))
        print(f"  {name:22s} median {out[name]['median']:10.2f}   min {out[name]['min']:10.2f}   max {out[name]['max']:10.2f}")
    for name in variants:
        tot = [f + b for f, b in zip(times[name + ".fwd"], times[name + ".bwd"])]
        out[name + ".fwd+bwd"] = dict(median=round(statistics.median(tot), 2), min=round(min(tot), 2), max=round(max(tot), 2))
        print(f"  {name + '.fwd+bwd':22s} median {out[name + '.fwd+bwd']['median']:10.2f}")
    results["configs"][key] = out
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
