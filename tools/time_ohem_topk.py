#!/usr/bin/env python3
"""The OHEM top-n_min branch: device selection + backward on the HIP kernels against the composite path, in one process.

    python tools/time_ohem_topk.py [--rounds 5] [--replays 50] [--configs 3,5] [--json OUT] [--no-step]
    python tools/time_ohem_topk.py --package-root DIR     # import cabinet_amd from another checkout (one without the
                                                          # selection entry points times the composite path and the floor only)

Configurations: 3 = 8 x 8 x 128 x 128 -> 1024^2, 5 = 2 x 19 x 256 x 128 -> 2048 x 1024.  Inputs shaped like late
training: low-resolution logits = 12 x one-hot of a blocky class map + noise, labels = that map with 1 % of the pixels flipped
and 10 % ignored, thresh 0.7, n_min = B*H*W/16: both heads are on the top-n_min branch.  Per configuration the variants
alternate round by round (clock and cache state drift alike for all of them):
  select       cabinet_ohem_select for both heads (init, 3 x (histogram, scan), sum, final), captured in a hipGraph
  bwd_sel      cabinet_ohem_up_pair_w_bwd_sel (threshold and tie factor read on the device), captured
  bwd_floor    cabinet_ohem_up_pair_w_bwd on first-branch inputs (random logits): what the backward costs on the other branch
  composite    F.interpolate of both heads + OhemCELoss.forward (cross_entropy, topk) + backward, eager (its branch decision
               reads the device, it cannot be captured; its kernels take milliseconds, launch overhead does not show)
and, unless --no-step, the whole GraphedTrainStep (CABiNet large, the configuration's batch) on a batch whose main head is on
the top-n_min branch (labels = the net's own prediction, thresh = ln C), no optimizer so that the batch keeps its branch:
  step_on      device_select=True: graph A + graph B-any
  step_off     device_select=False: graph A, restore of the BatchNorm buffers, the eager step (the behaviour without the option)
  step_first   a first-branch batch through graph A + graph B, for scale
Device events around `replays` calls after a warm-up; the median over rounds and the min .. max spread are printed in us.
"""
import argparse
import json
import math
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replays", type=int, default=50)
ap.add_argument("--configs", default="3,5")
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--step-calls", type=int, default=10)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cabinet_amd import _lib, functional as Fn  # noqa: E402
from cabinet_amd.loss import OhemCELoss  # noqa: E402

CONFIGS = {"3": (8, 8, 128, 128, 1024, 1024), "5": (2, 19, 256, 128, 2048, 1024)}
HAS_SELECT = "cabinet_ohem_select" in _lib.SIGNATURES


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


def late_training(B, C, Hl, Wl, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    cls_low = torch.randint(0, C, (B, Hl // 8, Wl // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    low = 12.0 * F.one_hot(cls_low, C).permute(0, 3, 1, 2).float() + 0.5 * torch.randn(B, C, Hl, Wl, generator=g)
    lab = cls_low.repeat_interleave(H // Hl, 1).repeat_interleave(W // Wl, 2).clone()
    flip = torch.rand(B, H, W, generator=g) < 0.01
    lab[flip] = torch.randint(0, C, (int(flip.sum()),), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.10] = 255
    return low.contiguous().cuda(), lab.cuda()


def summarise(times):
    return {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()}


results = {"package_root": os.path.abspath(args.package_root), "select_entry_points": HAS_SELECT, "rounds": args.rounds,
           "replays": args.replays, "device": torch.cuda.get_device_name(0), "configs": {}}
for key in args.configs.split(","):
    B, C, Hl, Wl, H, W = CONFIGS[key]
    size, n_min = (H, W), B * H * W // 16
    la, lab = late_training(B, C, Hl, Wl, H, W, 1)
    lb = (la + 0.25 * torch.randn_like(la)).contiguous()
    g = torch.Generator().manual_seed(0)
    ra, rb = ((torch.randn(B, C, Hl, Wl, generator=g) * 2).cuda() for _ in range(2))
    rlab = torch.randint(0, C, (B, H, W), generator=g).cuda()
    variants = {}
    loss_px, stats = Fn.ohem_up_pair_fwd_hip(la, lb, lab, size, 0.7, 255)
    host = stats.tolist()
    assert all(h[1] < min(n_min, h[0]) for h in host), ("inputs not on the top-n_min branch", host)
    if HAS_SELECT:
        gs, sel = graphed(lambda: Fn.ohem_select_hip(loss_px, lab, stats, 0.7, [n_min, n_min], 255, C))
        variants["select"] = gs
        variants["bwd_sel"] = graphed(lambda: Fn.ohem_up_pair_bwd_sel_hip(la, lb, lab, loss_px, size, sel, 255, 1.0))[0]
        print(f"config {key}: stats {host} sel {sel.tolist()}")
    rloss_px, rstats = Fn.ohem_up_pair_fwd_hip(ra, rb, rlab, size, 0.7, 255)
    assert all(h[1] >= n_min for h in rstats.tolist())
    variants["bwd_floor"] = graphed(lambda: Fn.ohem_up_pair_bwd_hip(ra, rb, rlab, rloss_px, size, 0.7, 255, 1.0))[0]
    ca, cb = OhemCELoss(0.7, n_min, 255).cuda(), OhemCELoss(0.7, n_min, 255).cuda()
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
        for name, gr in variants.items():
            times.setdefault(name, []).append(events(gr.replay, args.replays))
        times.setdefault("composite", []).append(events(composite, max(5, args.replays // 10)))
    out = summarise(times)
    del variants, xa, xb, loss_px, rloss_px
    torch.cuda.empty_cache()

    if not args.no_step:
        from cabinet_amd.train import GraphedTrainStep, build_model, make_criteria, synthetic_batch

        steps = {}
        im, lb_rand = synthetic_batch(B, H, W, C, "cuda", seed=1)
        own = None
        for name, ds in (("step_on", True), ("step_off", False)):
            if ds and not HAS_SELECT:
                continue
            net = build_model("large", n_classes=C, seed=0, gamma=0.5, device="cuda").train()
            crit = make_criteria(B, H, W, "cuda", thresh=math.log(C), **({"device_select": True} if ds else {}))
            step = GraphedTrainStep(net, crit, warmup=2, **({"device_select": True} if ds else {}))
            for _ in range(3):
                step(im, lb_rand)       # two eager steps, capture on the first-branch batch, one replay
            if own is None:
                with torch.no_grad():
                    low, _ = net.forward_lowres(im)
                    own = F.interpolate(low.float(), size=size, mode="bilinear", align_corners=False).argmax(1)
                    del low
            steps[name] = (step, own)
            if "step_first" not in steps:
                steps["step_first"] = (step, lb_rand)
        stimes = {}
        for name, (step, lbl) in steps.items():
            step(im, lbl)
        for r in range(args.rounds):
            for name, (step, lbl) in steps.items():
                stimes.setdefault(name, []).append(events(lambda: step(im, lbl), args.step_calls))
        out.update(summarise(stimes))
        for name, (step, _) in steps.items():
            out[name]["fallbacks"] = step.fallbacks
            out[name]["device_selected"] = getattr(step, "device_selected", 0)
        del steps
        torch.cuda.empty_cache()
    print(f"config {key}: B={B} C={C} {Hl}x{Wl} -> {H}x{W}   ({args.rounds} rounds, us)")
    for name, v in out.items():
        print(f"  {name:12s} median {v['median']:11.2f}   min {v['min']:11.2f}   max {v['max']:11.2f}"
              + (f"   fallbacks {v['fallbacks']} device_selected {v['device_selected']}" if "fallbacks" in v else ""))
    if "select" in out:
        print(f"  select / bwd_floor = {out['select']['median'] / out['bwd_floor']['median']:.2f}, "
              f"(select + bwd_sel) / composite = {(out['select']['median'] + out['bwd_sel']['median']) / out['composite']['median']:.3f}")
    results["configs"][key] = out
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
