"""The 64 -> 64 forward of the 3x3 stride-2 convolutions (K15, cabinet_conv3x3s2_fwd), operator alone: this build and other
builds of libcabinet_hip.so against the stock operator, at sb.conv2's and sb.conv3's planes.

    python tools/time_conv3x3s2_fwd64.py [--other PATH/libcabinet_hip.so ...] [--rounds 5] [--json FILE]
    python tools/time_conv3x3s2_fwd64.py --launch 3 [--lib PATH/libcabinet_hip.so]

The shapes are tests/fwd64_cases.py::BENCH_SHAPES: BASELINE config 3 (B = 8, 1024 x 1024), config 5 (B = 2, 2048 x 1024) and one
1024 x 2048 image.  `--other` (repeatable) is another build of the library (another tile width).  Each side is captured into a
hipGraph (NBUF calls, each on its own copy of x and y, so that the operands do not sit in the last-level cache between calls) and
the graphs are replayed alternately in one process; the figure is the median over the rounds (min and max beside it), timed with
events on the stream the kernels run on.  The stock side is the whole F.conv2d call: its NCHW <-> NHWC copies of x, w and y are
part of what it costs.  y of every build is compared bit for bit with this build's, and with the stock operator's by distance,
before anything is timed.  TFLOP/s = 2 B Ho Wo 64 64 9 / time against the 157.3 of the fp32 MFMA.  The table decides
_conv3x3s2_native_fwd64 in functional.py: a shape class is routed only where this build's maximum is below the stock minimum.

`--launch N` only launches the entry point N times per layer at config 3, eagerly and alone, for a counter pass of rocprofv3
(`rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES -- python tools/time_conv3x3s2_fwd64.py --launch 3`)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as F

import fwd64_cases as fc
from cabinet_amd import _lib
from cabinet_amd.functional import _ptr, _stream_handle

PEAK_TFLOPS = 157.3
NBUF = 4
NAMES = ["cabinet_conv3x3s2_fwd", "cabinet_conv3x3s2_fwd_supported", "cabinet_last_error"]


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


def fwd(lib, x, w, y, st):
    B, _, h, w_ = x.shape
    if lib.cabinet_conv3x3s2_fwd(_ptr(x), _ptr(w), B, 64, 64, h, w_, _ptr(y), st) != 0:
        raise RuntimeError(lib.cabinet_last_error().decode())


def launch(a):
    lib = load_other(a.lib) if a.lib else _lib.load()
    dev = torch.device("cuda")
    for name in ("sb.conv2 config 3", "sb.conv3 config 3"):
        B, h, w = fc.BENCH_SHAPES[name]
        x, wt = torch.randn(B, 64, h, w, device=dev), torch.randn(64, 64, 3, 3, device=dev) * 0.05
        y = torch.empty((B, 64) + fc.out_hw(h, w), device=dev)
        for _ in range(a.launch):
            fwd(lib, x, wt, y, _stream_handle(dev))
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
    rows = []
    for name, (B, h, w) in fc.BENCH_SHAPES.items():
        ho, wo = fc.out_hw(h, w)
        xs = [torch.randn(B, 64, h, w, device=dev) for _ in range(NBUF)]
        wt = torch.randn(64, 64, 3, 3, device=dev) * 0.05
        outs = []

        def stock():
            outs[:] = [F.conv2d(x, wt, None, 2, 1) for x in xs]
        with torch.no_grad():
            sides = [("stock", capture(stock), None)]
        ref = [o.clone() for o in outs]
        for label, lib in libs:
            ys = [torch.empty(B, 64, ho, wo, device=dev) for _ in range(NBUF)]

            def run(lib=lib, ys=ys):
                st = _stream_handle(dev)
                for x, y in zip(xs, ys):
                    fwd(lib, x, wt, y, st)
            sides.append((label, capture(run), ys))
        row = {"shape": name, "B": B, "h": h, "w": w}
        dist = max(float((p - q).norm() / q.norm()) for p, q in zip(sides[1][2], ref))
        row["this_vs_stock_rel"] = dist
        print(f"{name}: y of this vs stock: {dist:.3e}")
        for label, _, ys in sides[2:]:
            same = all(torch.equal(p, q) for p, q in zip(sides[1][2], ys))
            row[f"{label}_bit_equal_to_this"] = same
            print(f"{name}: y of {label} vs this: {'bit-equal' if same else 'DIFFER'}")
        times = {label: [] for label, _, _ in sides}
        for _ in range(a.rounds):
            for label, graph, _ in sides:
                times[label].append(replay_us(graph))
        flop = 2.0 * B * ho * wo * 64 * 64 * 9
        for label, t in times.items():
            med = statistics.median(t)
            tf = flop / med * 1e-6
            row[label] = {"us": round(med, 1), "min": round(min(t), 1), "max": round(max(t), 1), "tflops": round(tf, 1)}
            print(f"{name} @{B}x{h:4d}x{w:4d} {label:8s} {med:8.1f} us (min {min(t):.1f}, max {max(t):.1f})  {tf:5.1f} TF/s "
                  f"{tf / PEAK_TFLOPS:4.2f}", flush=True)
        rows.append(row)
        del xs, sides, outs, ref
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
