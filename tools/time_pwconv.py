"""Thin pointwise layers of the backbone (K10, csrc/pwconv.hip): forward, input gradient and weight gradient, per layer shape.

    python tools/time_pwconv.py [--other PATH/libcabinet_hip.so] [--wide] [--rounds 5] [--configs 3,5] [--json FILE]
    python tools/time_pwconv.py --once [--other-only --other PATH]     one eager call of every kernel at config 3 (for counters)

The six layers K10 serves at BASELINE config 3 (B = 8, 1024 x 1024) and config 5 (B = 2, 2048 x 1024).  Every operator is
captured into a hipGraph (four calls, each on its own copy of its operands and results, so that the planes do not sit in the
256 MB last-level cache between calls); with `--other` (another build of the library, e.g. the parent commit's) the graphs of
the two libraries are replayed alternately in one process.  The figure is the median over the rounds (min - max beside it),
timed with events on the stream the kernels run on.  `--wide` adds cabinet_pwconv_wide_wgrad (K14) at the same shapes.
Bytes are algorithmic: operands read once, results written once (dW itself is negligible); shares are of the 6.3 TB/s a
float4 copy reaches and of the 8 TB/s peak."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cabinet_amd import _lib
from cabinet_amd.functional import _ptr, _stream_handle, _workspace

NBUF = 4
COPY_TBS, PEAK_TBS = 6.3, 8.0
# (Ci, Co, plane divisor of the input)
LAYERS = [(16, 16, 2), (16, 64, 2), (64, 24, 4), (24, 72, 4), (72, 24, 4), (24, 72, 4)]
CONFIGS = {"3": ("config 3", 8, 1024, 1024), "5": ("config 5", 2, 2048, 1024)}
NAMES = ("cabinet_pwconv_fwd", "cabinet_pwconv_bwd", "cabinet_pwconv_bwd_workspace_bytes", "cabinet_pwconv_wide_wgrad",
         "cabinet_pwconv_wide_wgrad_workspace_bytes", "cabinet_last_error")


def other_library(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def capture(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def replay_us(graph, n=3):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / (n * NBUF) * 1e3


def operators(lib, B, ci, co, P, xs, gs, ys, dxs, wt, dw, wide):
    """-> {name: (callable running the operator on every buffer set, algorithmic bytes of one call)}"""
    def ok(rc, who):
        if rc != 0:
            raise RuntimeError(f"{who}: rc {rc}: {lib.cabinet_last_error().decode()}")

    ws, nb = _workspace(lib.cabinet_pwconv_bwd_workspace_bytes(B, ci, co, P), wt.device)
    plane = 4.0 * B * P

    def fwd():
        st = _stream_handle(wt.device)
        for x, y in zip(xs, ys):
            ok(lib.cabinet_pwconv_fwd(_ptr(x), _ptr(wt), B, ci, co, P, _ptr(y), st), "fwd")

    def dgrad():
        st = _stream_handle(wt.device)
        for x, g, dx in zip(xs, gs, dxs):
            ok(lib.cabinet_pwconv_bwd(_ptr(g), _ptr(x), _ptr(wt), B, ci, co, P, _ptr(dx), None, _ptr(ws), nb, st), "dx")

    def wgrad():
        st = _stream_handle(wt.device)
        for x, g in zip(xs, gs):
            ok(lib.cabinet_pwconv_bwd(_ptr(g), _ptr(x), _ptr(wt), B, ci, co, P, None, _ptr(dw), _ptr(ws), nb, st), "dW")

    ops = {"fwd": (fwd, plane * (ci + co)), "dx": (dgrad, plane * (ci + co)), "dW": (wgrad, plane * (ci + co))}
    if wide:
        ws2, nb2 = _workspace(lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, ci, co, P), wt.device)

        def wide_wgrad():
            st = _stream_handle(wt.device)
            for x, g in zip(xs, gs):
                ok(lib.cabinet_pwconv_wide_wgrad(_ptr(g), _ptr(x), B, ci, co, P, _ptr(dw), _ptr(ws2), nb2, st), "K14 dW")

        ops["dW(K14)"] = (wide_wgrad, plane * (ci + co))
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None, help="another build of libcabinet_hip.so to alternate with")
    ap.add_argument("--other-only", action="store_true", help="with --once: run the other library's kernels instead of this one's")
    ap.add_argument("--wide", action="store_true", help="also time cabinet_pwconv_wide_wgrad (K14) at these shapes")
    ap.add_argument("--once", action="store_true", help="one eager call of every kernel at the first config; no timing")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    this = _lib.load()
    other = other_library(a.other) if a.other else None
    rows = []
    for cfg in a.configs.split(","):
        name, B, H, W = CONFIGS[cfg]
        print(f"--- {name}: B = {B}, {H} x {W}")
        total = {}
        for ci, co, div in LAYERS:
            h, w = H // div, W // div
            P = h * w
            nbuf = 1 if a.once else NBUF
            xs = [torch.randn(B, ci, P, device="cuda") for _ in range(nbuf)]
            gs = [torch.randn(B, co, P, device="cuda") for _ in range(nbuf)]
            ys, dxs = [torch.empty_like(g) for g in gs], [torch.empty_like(x) for x in xs]
            wt, dw = torch.randn(co, ci, device="cuda") * ci ** -0.5, torch.empty(co, ci, device="cuda")
            if a.once:
                lib = other if a.other_only else this
                for fn, _ in operators(lib, B, ci, co, P, xs, gs, ys, dxs, wt, dw, False).values():
                    fn()
                torch.cuda.synchronize()
                continue
            sides = [("this", operators(this, B, ci, co, P, xs, gs, ys, dxs, wt, dw, a.wide))]
            if other is not None:
                sides.append(("other", operators(other, B, ci, co, P, xs, gs, ys, dxs, wt, dw, False)))
            for op in sides[0][1]:
                graphs = [(side, capture(ops[op][0])) for side, ops in sides if op in ops]
                times = {side: [] for side, _ in graphs}
                for _ in range(a.rounds):
                    for side, g in graphs:
                        times[side].append(replay_us(g))
                nbytes = sides[0][1][op][1]
                for side, t in times.items():
                    med = statistics.median(t)
                    tbs = nbytes / med * 1e-6
                    total[(side, op)] = total.get((side, op), 0.0) + med
                    print(f"{ci:3d}->{co:3d} @{h:4d}x{w:4d} {op:8s} {side:5s}: {med:7.1f} us ({min(t):7.1f} - {max(t):7.1f})  "
                          f"{nbytes / 1e6:6.1f} MB  {tbs * 1e3:6.0f} GB/s  {tbs / COPY_TBS:4.2f} of copy  {tbs / PEAK_TBS:4.2f} of peak")
                    rows.append({"config": name, "ci": ci, "co": co, "h": h, "w": w, "op": op, "side": side, "median_us": round(med, 2),
                                 "min_us": round(min(t), 2), "max_us": round(max(t), 2), "mbytes": round(nbytes / 1e6, 2),
                                 "gbs": round(tbs * 1e3, 1)})
                del graphs
        for (side, op), t in sorted(total.items()):
            print(f"{name}: six layers {op:8s} {side:5s}: {t:7.1f} us")
            rows.append({"config": name, "op": op, "side": side, "total_us": round(t, 1)})
        if a.once:
            break
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
