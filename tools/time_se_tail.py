"""Backward of the squeeze-excite tail (functional.se_tail) per production shape, SE_MLP_FUSED off and on.

    python tools/time_se_tail.py [--rounds 5] [--configs 3,5] [--json FILE]

The eight `BatchNorm -> SELayer -> act` runs of the large backbone (features.4-6, 11-15) at BASELINE config 3 (B = 8,
1024 x 1024) and config 5 (B = 2, 2048 x 1024).  For each shape three hipGraphs are captured: the forward alone, and forward +
backward once with the MLP's adjoint as the chain of torch ops and once as cabinet_se_act_bwd_mlp; they are replayed alternately
in one process and timed with events on the stream the kernels run on.  The backward (reduce, the MLP's adjoint, dx) is a step's
time minus the median of the forward alone; the figure is the median over the rounds (min - max beside it).  The forward is the
same in both steps, so the difference of the two columns is what the MLP's adjoint costs between the streaming passes."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import cabinet_amd.functional as Fh
from cabinet_amd.models.mobilenetv3 import SELayer

# (C, plane divisor, act) of the BatchNorm input
BLOCKS = [(72, 8, "relu"), (120, 8, "relu"), (120, 8, "relu"), (480, 16, "hardswish"), (672, 16, "hardswish"),
          (672, 32, "hardswish"), (960, 32, "hardswish"), (960, 32, "hardswish")]
CONFIGS = {"3": ("config 3", 8, 1024, 1024), "5": ("config 5", 2, 2048, 1024)}
REPLAYS = 5


def capture(fn, fused):
    """fn under hipGraph capture.  Forward and backward are captured together: autograd runs a node's backward on the stream its
    forward ran on, so a backward captured alone would leave the capturing stream for the one an earlier, uncaptured forward used."""
    Fh.SE_MLP_FUSED = fused
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph, out


def replay_us(graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPLAYS):
        graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / REPLAYS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for cfg in a.configs.split(","):
        name, B, H, W = CONFIGS[cfg]
        print(f"--- {name}: B = {B}, {H} x {W}")
        total = {"chain": 0.0, "fused": 0.0}
        for C, div, act in BLOCKS:
            h, w = H // div, W // div
            torch.manual_seed(C + div)
            bn, se = nn.BatchNorm2d(C).cuda().train(), SELayer(C).cuda().train()
            z = torch.randn(B, C, h, w, device="cuda", requires_grad=True)
            g = torch.randn(B, C, h, w, device="cuda")
            inputs = [z] + list(bn.parameters()) + list(se.parameters())

            def forward():
                with torch.no_grad():
                    return Fh.se_tail(z, bn, se, act)

            def step():
                return torch.autograd.grad(Fh.se_tail(z, bn, se, act), inputs, g)

            graphs = [("fwd", capture(forward, True)), ("chain", capture(step, False)), ("fused", capture(step, True))]
            raw = {side: [] for side, _ in graphs}
            for _ in range(a.rounds):
                for side, (graph, _) in graphs:
                    raw[side].append(replay_us(graph))
            fwd = statistics.median(raw["fwd"])
            times = {side: [t - fwd for t in raw[side]] for side in ("chain", "fused")}  # the backward: step minus forward
            med = {side: statistics.median(t) for side, t in times.items()}
            print(f"C={C:4d} @{h:4d}x{w:4d} forward alone: {fwd:7.1f} us ({min(raw['fwd']):7.1f} - {max(raw['fwd']):7.1f})")
            for side, t in times.items():
                total[side] += med[side]
                print(f"C={C:4d} Cs={se.fc[0].out_features:4d} @{h:4d}x{w:4d} {side:5s}: {med[side]:7.1f} us ({min(t):7.1f} - {max(t):7.1f})")
                rows.append({"config": name, "C": C, "Cs": se.fc[0].out_features, "h": h, "w": w, "side": side,
                             "median_us": round(med[side], 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)})
            del graphs, z, g
        print(f"{name}: eight blocks chain {total['chain']:7.1f} us  fused {total['fused']:7.1f} us  "
              f"gain {total['chain'] - total['fused']:6.1f} us")
        rows.append({"config": name, "chain_total_us": round(total["chain"], 1), "fused_total_us": round(total["fused"], 1)})
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
