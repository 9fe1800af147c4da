#!/usr/bin/env python3
"""Time single-image inference on one GPU: the reference's sequence (plain) against the fused tail, eager and as one hipGraph.

    python tools/time_predict.py [--reps 20] [--mode large] [--height 1024 --width 2048] [--profile] [--out FILE]

One 1 x 3 x 1024 x 2048 image, 19 classes, two cases: (a) scales (1.0,) without flip -- what visualize_predictions runs -- and
(b) scales (0.75, 1.0, 1.25) with flip.  Three paths:
  plain     cabinet_amd.predict.infer_image(fused=False): model(x)[0] at full resolution, softmax, flip, resize, +=, /=, argmax,
            int64 labels to the host -- the reference's sequence, which is all the package offered before this tail existed
  fused     infer_image(fused=True): forward_lowres + the HIP tail, uint8 labels to the host (widened to int64 there)
  graphed   Predictor(fused=True, graph=True).predict(x).cpu(): the same work replayed from one hipGraph
Every repetition ends with the label map on the host and a device synchronise; the host clock is read on both sides.  Per path:
  whole   the call as a user makes it
  model   the same forwards alone (model(x)[0] for plain, forward_lowres for fused), nothing after them
  tail    everything after the model, measured directly: the same call with the model replaced by a replay of its recorded
          outputs (plain and fused eager only; inside a graph the two cannot be separated: not measured)
After warm-up of every shape the paths ALTERNATE within one process; median [min, max] over --reps repetitions.  One JSON line
(also written to --out), with the algorithmic bytes of each tail from the shapes and their time at the 8 TB/s roof.

--profile runs each case's fused eager path (labels, then labels + render) a few times and exits
(for `rocprofv3 --kernel-trace --stats -- python tools/time_predict.py --profile`).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CASES = {"a_scales_1.0_noflip": ((1.0,), False), "b_scales_0.75_1.0_1.25_flip": ((0.75, 1.0, 1.25), True)}
C = 19
HBM_TBPS = 8.0


class _Replay(torch.nn.Module):
    """Stands in for the model: records what the real model returns for each call of one image, then replays it."""

    def __init__(self, real):
        super().__init__()
        self.real, self.lo, self.hi, self.i, self.recording = [real], [], [], 0, True   # in a list: not a submodule
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=next(real.parameters()).device))  # names the device

    def _next(self, store, fn, x):
        if self.recording:
            store.append(fn(x)[0])
            return (store[-1], None)
        self.i += 1
        return (store[self.i - 1], None)

    def forward_lowres(self, x):
        return self._next(self.lo, self.real[0].forward_lowres, x)

    def forward(self, x):
        return self._next(self.hi, self.real[0], x)


def _model_only(net, x, scales, flip, lowres):
    run = (lambda t: net.forward_lowres(t)[0]) if lowres else (lambda t: net(t)[0])
    H, W = x.shape[2:]
    for s in scales:
        t = x if s == 1.0 else F.interpolate(x, [int(H * s), int(W * s)], mode="bilinear", align_corners=False)
        run(t)
        if flip:
            run(torch.flip(t, dims=(3,)))


def _timed(fn, *a, **k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*a, **k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def tail_bytes(H, W, scales, flip):
    """Algorithmic bytes each tail moves in device memory (every tensor read or written once per operation that touches it)."""
    f = 4
    full = C * H * W * f
    plain = full                                      # zeros(probs)
    fused = 0
    single = len(scales) == 1 and scales[0] == 1.0 and not flip
    for s in scales:
        h, w = int(H * s), int(W * s)
        low, sc = C * (h // 8) * (w // 8) * f, C * h * w * f
        n = 2 if flip else 1
        plain += n * (low + sc) + n * 2 * sc          # the model's x8 upsample, softmax
        if flip:
            plain += 2 * sc + 3 * sc + 2 * sc         # flip of the logits, prob + flipped, / 2
        if s != 1.0:
            plain += sc + full                        # resize back
        plain += 3 * full                             # probs += prob
        if single:
            fused += low + H * W                      # predict_up_argmax: low logits in, uint8 labels out
        elif (h, w) == (H, W):
            fused += n * low + 2 * full               # eval_chip_accum straight into total
        else:
            fused += sc + n * low + 2 * sc + sc + 2 * full   # zeros, eval_chip_accum, eval_scale_merge
    plain += 2 * full + full + H * W * 8              # /= len(scales), argmax (int64 out)
    if not single:
        fused += full + full + H * W                  # zeros(total), predict_argmax
    return {"plain_MB": round(plain / 1e6, 1), "fused_MB": round(fused / 1e6, 1),
            "plain_us_at_roof": round(plain / (HBM_TBPS * 1e6), 1), "fused_us_at_roof": round(fused / (HBM_TBPS * 1e6), 2),
            "plain_d2h_MB": round(H * W * 8 / 1e6, 1), "fused_d2h_MB": round(H * W / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="large")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_predict.py measures on a GPU; there is no CPU fallback"
    from cabinet_amd.predict import Predictor, infer_image
    from cabinet_amd.train import build_model

    dev = torch.device("cuda", 0)
    H, W = a.height, a.width
    net = build_model(a.mode, n_classes=C, seed=0, gamma=0.5).to(dev).eval()
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(0)).to(dev)
    out = {"tool": "time_predict", "device": torch.cuda.get_device_name(0), "mode": a.mode, "image": [1, 3, H, W], "classes": C,
           "reps": a.reps, "unit": "ms", "cases": {}}
    with torch.no_grad():
        for name, (scales, flip) in CASES.items():
            kw = dict(num_classes=C, scales=list(scales), flip=flip, device=dev)
            if a.profile:
                renderer = Predictor(net, C, scales=scales, flip=flip, fused=True)
                for _ in range(4):
                    infer_image(net, x, fused=True, **kw)
                    renderer.render(x)
                torch.cuda.synchronize()
                continue
            graphed = Predictor(net, C, scales=scales, flip=flip, fused=True, graph=True)
            whole = {"plain": lambda: infer_image(net, x, fused=False, **kw), "fused": lambda: infer_image(net, x, fused=True, **kw),
                     "graphed": lambda: graphed.predict(x).cpu().numpy()[0]}
            replays, tails = {}, {}
            for p in ("plain", "fused"):   # record the model's outputs for this image once per path
                replays[p] = _Replay(net).eval()
                infer_image(replays[p], x, fused=(p == "fused"), **kw)
                replays[p].recording = False

                def tail(p=p):
                    replays[p].i = 0
                    return infer_image(replays[p], x, fused=(p == "fused"), **kw)
                tails[p] = tail
            for _ in range(a.warmup):
                for p in whole:
                    whole[p]()
                for p in tails:
                    tails[p]()
                    _model_only(net, x, scales, flip, lowres=(p == "fused"))
            t = {p: {"whole": [], "model": [], "tail": []} for p in whole}
            labels, differ = {}, {p: 0 for p in tails}
            for _ in range(a.reps):
                for p in whole:   # plain, fused, graphed, plain, ...
                    ms, labels[p] = _timed(whole[p])
                    t[p]["whole"].append(ms)
                    if p in tails:
                        t[p]["model"].append(_timed(_model_only, net, x, scales, flip, p == "fused")[0])
                        ms, lab = _timed(tails[p])
                        t[p]["tail"].append(ms)
                        differ[p] = max(differ[p], int((lab != labels[p]).sum()))
            case = {"scales": list(scales), "flip": flip,
                    "pixels_plain_and_fused_label_differently": int((labels["plain"] != labels["fused"]).sum()),
                    "pixels_graphed_and_fused_label_differently": int((labels["graphed"] != labels["fused"]).sum()),
                    "pixels_replayed_tail_and_whole_call_label_differently_max": differ,
                    "tail_bytes": tail_bytes(H, W, scales, flip)}
            for p in whole:
                case[p] = {k: (_stats(v) if v else "not measured") for k, v in t[p].items()}
            case["whole_ratio_plain_over_fused"] = round(case["plain"]["whole"]["median"] / case["fused"]["whole"]["median"], 2)
            case["whole_ratio_plain_over_graphed"] = round(case["plain"]["whole"]["median"] / case["graphed"]["whole"]["median"], 2)
            case["tail_ratio_plain_over_fused"] = round(case["plain"]["tail"]["median"] / case["fused"]["tail"]["median"], 2)
            case["fused_whole_median_below_plain_min"] = bool(case["fused"]["whole"]["median"] < case["plain"]["whole"]["min"])
            out["cases"][name] = case
    if not a.profile:
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
