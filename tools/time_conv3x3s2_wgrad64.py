"""The 64 -> 64 weight gradient of the 3x3 stride-2 convolutions (K15, cabinet_conv3x3s2_wgrad), operator alone: this build and
other builds of libcabinet_hip.so against the stock operator, at sb.conv2's and sb.conv3's planes.

    python tools/time_conv3x3s2_wgrad64.py [--other PATH/libcabinet_hip.so ...] [--rounds 5] [--json FILE]
    python tools/time_conv3x3s2_wgrad64.py --launch 3 [--lib PATH/libcabinet_hip.so]

`--other` (repeatable) is another build of the library: the parent commit's.  BASELINE config 3 (B = 8, 1024 x 1024) and config 5
(B = 2, 2048 x 1024).  Each side is captured into a hipGraph (NBUF calls, each on its own copy of x and dy, so that the operands do
not sit in the last-level cache between calls) and the graphs are replayed alternately in one process; the figure is the median
over the rounds (min and max beside it), timed with events on the stream the kernels run on.  The stock side is the whole
aten.convolution_backward call with mask [False, True, False]: its NCHW <-> NHWC copies of x, dy and dw are part of what it
costs.  dW of every build is compared bit for bit with this build's before anything is timed.  TFLOP/s = 2 B Ho Wo 64 64 9 / time
against the 157.3 of the fp32 MFMA.  The table decides _conv3x3s2_native_wgrad64 in functional.py.

`--launch N` only launches the entry point N times per layer at config 3, eagerly and alone, for a counter pass of rocprofv3
(`rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES -- python tools/time_conv3x3s2_wgrad64.py --launch 3`)."""
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

PEAK_TFLOPS = 157.3
NBUF = 4
CONFIGS = [("config 3", 8, 1024, 1024), ("config 5", 2, 2048, 1024)]
LAYERS = [("sb.conv2", 2), ("sb.conv3", 4)]  # (name, plane divisor of the image)
NAMES = ["cabinet_conv3x3s2_wgrad", "cabinet_conv3x3s2_wgrad_workspace_bytes", "cabinet_last_error"]


def load_other(path):
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
    return start.elapsed_time(stop) * 1e3 / (n * NBUF)


def wgrad(lib, g, x, dw, ws, nb, st):
    B, _, h, w = x.shape
    if lib.cabinet_conv3x3s2_wgrad(_ptr(g), _ptr(x), B, 64, 64, h, w, _ptr(dw), _ptr(ws), nb, st) != 0:
        raise RuntimeError(lib.cabinet_last_error().decode())


def launch(a):
    lib = load_other(a.lib) if a.lib else _lib.load()
    dev = torch.device("cuda")
    _, B, H, W = CONFIGS[0]
    for _, div in LAYERS:
        h, w = H // div, W // div
        x, g = torch.randn(B, 64, h, w, device=dev), torch.randn(B, 64, h // 2, w // 2, device=dev)
        dw = torch.empty(64, 64, 3, 3, device=dev)
        ws, nb = _workspace(lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, 64, 64, h, w), dev)
        for _ in range(a.launch):
            wgrad(lib, g, x, dw, ws, nb, _stream_handle(dev))
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", action="append", default=[])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--launch", type=int, default=0)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.launch:
        return launch(a)
    libs = [("this", _lib.load())] + [(os.path.basename(os.path.dirname(os.path.abspath(p))), load_other(p)) for p in a.other]
    dev = torch.device("cuda")
    cb = torch.ops.aten.convolution_backward
    rows = []
    for cfg, B, H, W in CONFIGS:
        for layer, div in LAYERS:
            h, w = H // div, W // div
            ho, wo = h // 2, w // 2
            xs = [torch.randn(B, 64, h, w, device=dev) for _ in range(NBUF)]
            gs = [torch.randn(B, 64, ho, wo, device=dev) for _ in range(NBUF)]
            wt = torch.randn(64, 64, 3, 3, device=dev)

            def stock():
                for x, g in zip(xs, gs):
                    cb(g, x, wt, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])
            sides = [("stock", capture(stock), None)]
            keep = []  # the workspaces the graphs write to: a capture empties the allocator's cache, a dropped one would be unmapped
            for label, lib in libs:
                dws = [torch.empty(64, 64, 3, 3, device=dev) for _ in range(NBUF)]
                ws, nb = _workspace(lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, 64, 64, h, w), dev)
                keep.append(ws)

                def run(lib=lib, dws=dws, ws=ws, nb=nb):
                    st = _stream_handle(dev)
                    for x, g, dw in zip(xs, gs, dws):
                        wgrad(lib, g, x, dw, ws, nb, st)
                sides.append((label, capture(run), dws))
            row = {"config": cfg, "layer": layer, "h": h, "w": w}
            for label, _, dws in sides[2:]:
                same = all(torch.equal(p, q) for p, q in zip(sides[1][2], dws))
                row[f"{label}_bit_equal_to_this"] = same
                print(f"{cfg}: {layer}: dW of {label} vs this: {'bit-equal' if same else 'DIFFER'}")
            times = {label: [] for label, _, _ in sides}
            for _ in range(a.rounds):
                for label, graph, _ in sides:
                    times[label].append(replay_us(graph))
            flop = 2.0 * B * ho * wo * 64 * 64 * 9
            for label, t in times.items():
                med = statistics.median(t)
                tf = flop / med * 1e-6
                row[label] = {"us": round(med, 1), "min": round(min(t), 1), "max": round(max(t), 1), "tflops": round(tf, 1)}
                print(f"{cfg}: {layer} dw @{h:4d}x{w:4d} {label:8s} {med:8.1f} us (min {min(t):.1f}, max {max(t):.1f})  {tf:5.1f} TF/s "
                      f"{tf / PEAK_TFLOPS:4.2f}", flush=True)
            rows.append(row)
            del xs, gs, sides, keep
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
