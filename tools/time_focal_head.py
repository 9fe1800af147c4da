#!/usr/bin/env python3
"""The fused focal head against the composite SoftmaxFocalLoss and against the OHEM head, and the focal train step, in one process.

    python tools/time_focal_head.py [--rounds 7] [--replays 500] [--configs a,5] [--json profiles/focal_head.json] [--no-step]

Configurations: a = 8 x 19 x 128 x 128 -> 1024^2, 5 = 2 x 19 x 256 x 128 -> 2048 x 1024.  Random logits
(sigma 2), labels uniform over the classes with 10 % ignored, ENet-style class weights on both heads, gamma = 2.  Per
configuration the variants alternate round by round (clock and cache state drift alike for all of them):
  focal_fwd / focal_bwd    cabinet_focal_up_fwd + cabinet_focal_stats / cabinet_focal_up_bwd for BOTH heads, each captured in a
                           hipGraph (kernel time without launch overhead)
  ohem_fwd / ohem_bwd      the same groups of the weighted OHEM pair (thresh 0.7), the yardstick
  focal_pair               focal_upsampled_pair + backward through autograd, eager (what TrainStep runs)
  composite_pair           2 x (F.interpolate + SoftmaxFocalLoss.forward) + backward, eager: the composite path
and, unless --no-step, whole steps of CABiNet large on the configuration's batch with SGD:
  step_focal_graph         GraphedTrainStep, focal criteria: one graph + the eager optimizer step
  step_focal_eager         TrainStep, focal criteria
  step_ohem_graph          GraphedTrainStep, OHEM criteria: two graphs around one host read
Device events around `replays` calls after a warm-up (50-100 ms of kernels per sample; steps: a host clock around
`step-calls` calls, 0.6-1 s per sample, ending in a synchronise);
the median over rounds and the min .. max spread are reported in us.  Before anything is timed the fused pair's loss and
gradients are compared with the composite's on the timed inputs and the differences are reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--replays", type=int, default=500)
ap.add_argument("--configs", default="a,5")
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--step-calls", type=int, default=50)
ap.add_argument("--gamma", type=float, default=2.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cabinet_amd import functional as Fn  # noqa: E402
from cabinet_amd.loss import OhemCELoss, SoftmaxFocalLoss, focal_upsampled_pair  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_focal_head.py measures on a GPU; none found")

CONFIGS = {"a": (8, 19, 128, 128, 1024, 1024), "5": (2, 19, 256, 128, 2048, 1024)}
IGNORE = 255


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def graphed(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def summary(samples):
    return dict(median_us=round(statistics.median(samples), 1), min_us=round(min(samples), 1), max_us=round(max(samples), 1))


def head_times(key):
    B, C, Hl, Wl, H, W = CONFIGS[key]
    g = torch.Generator().manual_seed(7)
    la, lb_ = (torch.randn(B, C, Hl, Wl, generator=g).mul_(2.0).cuda() for _ in range(2))
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    lab = lab.cuda()
    w = (1.0 / torch.log(1.02 + torch.rand(C, generator=g))).cuda()
    gam = [args.gamma, args.gamma]
    fa, fb = (SoftmaxFocalLoss(args.gamma, weight=w.clone(), ignore_lb=IGNORE).cuda() for _ in range(2))

    def fused_pair():
        xa, xb = la.clone().requires_grad_(True), lb_.clone().requires_grad_(True)
        loss = focal_upsampled_pair(fa, xa, fb, xb, lab, (H, W))
        loss.backward()
        return loss.detach(), xa.grad, xb.grad

    def composite_pair():
        xa, xb = la.clone().requires_grad_(True), lb_.clone().requires_grad_(True)
        loss = fa(F.interpolate(xa, size=(H, W), mode="bilinear", align_corners=False), lab) + \
            fb(F.interpolate(xb, size=(H, W), mode="bilinear", align_corners=False), lab)
        loss.backward()
        return loss.detach(), xa.grad, xb.grad

    (lf, gfa, gfb), (lc, gca, gcb) = fused_pair(), composite_pair()
    parity = dict(loss_fused=float(lf), loss_composite=float(lc),
                  dlow_rel_diff=[float((x - y).norm() / y.norm()) for x, y in ((gfa, gca), (gfb, gcb))])
    loss_px, _ = Fn.focal_up_fwd_hip([la, lb_], lab, (H, W), gam, IGNORE, [w, w])
    o_px, _ = Fn.ohem_up_pair_fwd_hip(la, lb_, lab, (H, W), 0.7, IGNORE, w, w)
    variants = {
        "focal_fwd": graphed(lambda: Fn.focal_up_fwd_hip([la, lb_], lab, (H, W), gam, IGNORE, [w, w])),
        "focal_bwd": graphed(lambda: Fn.focal_up_bwd_hip([la, lb_], lab, loss_px, (H, W), gam, IGNORE, 1.0, [w, w])),
        "ohem_fwd": graphed(lambda: Fn.ohem_up_pair_fwd_hip(la, lb_, lab, (H, W), 0.7, IGNORE, w, w)),
        "ohem_bwd": graphed(lambda: Fn.ohem_up_pair_bwd_hip(la, lb_, lab, o_px, (H, W), 0.7, IGNORE, 1.0, w, w)),
        "focal_pair": fused_pair,
        "composite_pair": composite_pair,
    }
    samples = {k: [] for k in variants}
    for fn in variants.values():
        events(fn, 3)
    for _ in range(args.rounds):
        for k, fn in variants.items():
            samples[k].append(events(fn, args.replays if k != "composite_pair" else max(3, args.replays // 5)))
    out = {k: summary(v) for k, v in samples.items()}
    out["parity_on_timed_inputs"] = parity
    return out


def step_times(key):
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria, synthetic_batch

    B, C, _, _, H, W = CONFIGS[key]
    batches = [synthetic_batch(B, H, W, C, "cuda", seed=50 + i) for i in range(3)]
    w = (1.0 / torch.log(1.02 + torch.rand(C, generator=torch.Generator().manual_seed(1))))
    steps = {}
    for name, kind, gr in (("step_focal_graph", "focal", True), ("step_focal_eager", "focal", False), ("step_ohem_graph", "ohem", True)):
        net = build_model("large", n_classes=C, seed=0, device="cuda").train()
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-3, momentum=0.9)
        crit = make_criteria(B, H, W, "cuda", weight=w, loss=kind, gamma=args.gamma)
        step = GraphedTrainStep(net, crit, optimizer=opt, warmup=2) if gr else TrainStep(net, crit, optimizer=opt)
        for i in range(4):
            step(*batches[i % 3])
        torch.cuda.synchronize()
        steps[name] = step
    samples = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.step_calls):
                step(*batches[i % 3])
            torch.cuda.synchronize()
            samples[k].append((time.perf_counter() - t0) / args.step_calls * 1e6)
    out = {k: summary(v) for k, v in samples.items()}
    out["fallbacks"] = {k: getattr(s, "fallbacks", None) for k, s in steps.items()}
    return out


result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, gamma=args.gamma, rounds=args.rounds,
              replays=args.replays, step_calls=args.step_calls, configs={})
for key in args.configs.split(","):
    B, C, Hl, Wl, H, W = CONFIGS[key]
    entry = dict(shape=f"{B}x{C}x{Hl}x{Wl} -> {H}x{W}", heads=head_times(key))
    torch.cuda.empty_cache()
    if not args.no_step:
        entry["steps"] = step_times(key)
        torch.cuda.empty_cache()
    result["configs"][key] = entry
    print(json.dumps({key: entry}), flush=True)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
