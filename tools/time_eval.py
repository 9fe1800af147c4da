#!/usr/bin/env python3
"""Time the multi-scale evaluator on one GPU: the model forwards and everything after the model, plain path against fused path.

    python tools/time_eval.py [--reps 20] [--mode large] [--profile]

Two cases at BASELINE config 5's shape (batch 2, 3 x 2048 x 1024, 19 classes, crop 1024, flip on): (a) scales (1.0,) and
(b) scales (0.75, 1.0, 1.25).  Per case and path two things are timed, each with a device synchronise on both sides of a host clock:
  whole   MscEvalV0's summed probability map + argmax + confusion matrix of one batch (labels upload and, on the plain path, the
          predictions' trip to the host and numpy.bincount included),
  model   the same sequence of chips through the model alone (model(x)[0] for the plain path, forward_lowres for the fused one),
  tail    "everything after the model", measured directly: the same batch with the model replaced by a replay of its recorded
          outputs (so a noisy forward does not leak into the difference of two large numbers).
After warm-up of every shape the two paths ALTERNATE within one process; medians over --reps repetitions, and the spread (min,
max) of each so that a difference can be judged.  One JSON line.

--profile runs each case's fused path a few times and exits (for `rocprofv3 --kernel-trace --stats -- python tools/time_eval.py --profile`).
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

CASES = {"a_scales_1.0": (1.0,), "b_scales_0.75_1.0_1.25": (0.75, 1.0, 1.25)}
N, H, W, C, CROP = 2, 2048, 1024, 19, 1024


class _ModelOnly:
    """Replays the chips an evaluator cuts, through the model alone."""

    def __init__(self, ev, lowres):
        self.ev, self.lowres = ev, lowres

    def __call__(self, images):
        from cabinet_amd.evaluate import EVAL_STRIDE_RATE, _window_starts

        ev, crop = self.ev, self.ev.cropsize
        run = (lambda x: ev.model.forward_lowres(x)[0]) if self.lowres else (lambda x: ev.model(x)[0])
        for scale in ev.scales:
            h, w = images.shape[2:]
            x = F.interpolate(images, [int(h * scale), int(w * scale)], mode="bilinear", align_corners=False)
            target = ev._target_size(*x.shape[2:])
            if target is not None:
                x, _ = ev.pad_tensor(x, target)
            stride = int(crop * EVAL_STRIDE_RATE)
            for y in _window_starts(x.shape[2], crop, stride):
                for x0 in _window_starts(x.shape[3], crop, stride):
                    chip = x[:, :, y:y + crop, x0:x0 + crop].contiguous()
                    run(chip)
                    if ev.flip:
                        run(torch.flip(chip, dims=(3,)))


class _Replay(torch.nn.Module):
    """Stands in for the model: records what the real model returns for each chip of one batch, then replays it."""

    def __init__(self, real):
        super().__init__()
        self.real, self.lo, self.hi, self.i, self.recording = [real], [], [], 0, True   # in a list: not a submodule

    def _next(self, store, fn, x):
        if self.recording:
            store.append(fn(x)[0])
            return (store[-1],)
        self.i += 1
        return (store[self.i - 1],)

    def forward_lowres(self, x):
        return self._next(self.lo, self.real[0].forward_lowres, x)

    def forward(self, x):
        return self._next(self.hi, self.real[0], x)


def _tail(ev, replay, images, labels):
    replay.i = 0
    return _whole(ev, images, labels)


def _whole(ev, images, labels):
    """One batch of MscEvalV0.evaluate(), without the metrics."""
    from cabinet_amd import functional as fn

    probs, fused = ev._summed_probs(images)
    if fused:
        hist = torch.zeros((C, C), dtype=torch.int64, device=images.device)
        fn.eval_argmax_hist(probs, labels.to(device=images.device, dtype=torch.int64), hist, ev.ignore_label)
        return hist.cpu().numpy()
    preds = torch.argmax(probs, dim=1).cpu().numpy()
    lab = labels.numpy()
    return sum(ev.compute_hist(preds[i], lab[i], C, ev.ignore_label) for i in range(lab.shape[0]))


def _timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="large")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_eval.py measures on a GPU; there is no CPU fallback"
    from cabinet_amd.evaluate import MscEvalV0
    from cabinet_amd.train import build_model

    dev = torch.device("cuda", 0)
    net = build_model(a.mode, n_classes=C, seed=0, gamma=0.5).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    images = torch.randn(N, 3, H, W, generator=g).to(dev)
    labels = torch.randint(0, C, (N, H, W), generator=g)
    labels[torch.rand(N, H, W, generator=g) < 0.1] = 255
    out = {"tool": "time_eval", "device": torch.cuda.get_device_name(0), "mode": a.mode, "batch": N, "image": [H, W], "classes": C,
           "cropsize": CROP, "flip": True, "reps": a.reps, "unit": "ms", "cases": {}}
    with torch.no_grad():
        for name, scales in CASES.items():
            evs = {p: MscEvalV0(net, [], C, scales=scales, flip=True, cropsize=CROP, fused=(p == "fused")) for p in ("plain", "fused")}
            if a.profile:
                for _ in range(3):
                    _whole(evs["fused"], images, labels)
                torch.cuda.synchronize()
                continue
            model_only = {p: _ModelOnly(evs[p], lowres=(p == "fused")) for p in evs}
            replays, tails = {}, {}
            for p in evs:   # record the model's outputs for this batch once per path
                replays[p] = _Replay(net)
                tails[p] = MscEvalV0(replays[p], [], C, scales=scales, flip=True, cropsize=CROP, fused=(p == "fused"))
                _whole(tails[p], images, labels)
                replays[p].recording = False
            for _ in range(a.warmup):
                for p in evs:
                    _whole(evs[p], images, labels)
                    model_only[p](images)
                    _tail(tails[p], replays[p], images, labels)
            t = {p: {"whole": [], "model": [], "tail": []} for p in evs}
            hists = {}
            for _ in range(a.reps):
                for p in evs:   # plain, fused, plain, fused, ...
                    ms, hists[p] = _timed(_whole, evs[p], images, labels)
                    t[p]["whole"].append(ms)
                    t[p]["model"].append(_timed(model_only[p], images)[0])
                    ms, h = _timed(_tail, tails[p], replays[p], images, labels)
                    t[p]["tail"].append(ms)
                    assert np.array_equal(h, hists[p]), "the replayed batch must give the batch's own confusion matrix"
            case = {"scales": list(scales), "confusion_cells_differing_by": float(np.abs(hists["plain"] - hists["fused"]).sum())}
            for p in evs:
                case[p] = {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                           for k, v in t[p].items()}
            case["tail_ratio_plain_over_fused"] = round(case["plain"]["tail"]["median"] / case["fused"]["tail"]["median"], 2)
            case["whole_ratio_plain_over_fused"] = round(case["plain"]["whole"]["median"] / case["fused"]["whole"]["median"], 2)
            out["cases"][name] = case
    if not a.profile:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
