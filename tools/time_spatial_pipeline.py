"""The two pipelined matrix kernels of the spatial branch, operators alone: cabinet_stem_conv_fwd (K9) and
cabinet_conv3x3s2_dgrad (K15, at sb.conv2's and sb.conv3's planes), this build against other builds of libcabinet_hip.so.

    python tools/time_spatial_pipeline.py [--other PATH/libcabinet_hip.so ...] [--rounds 5] [--json FILE]

`--other` (repeatable) is another build of the library: the parent commit's, or a variant of a kernel under measurement.  BASELINE
config 3 (B = 8, 1024 x 1024) and config 5 (B = 2, 2048 x 1024).  Each side is captured into a hipGraph (NBUF calls, each on its
own copy of the operands and of the output, so that one call's output does not sit in the last-level cache for the next) and the
graphs are replayed alternately in one process; the figure is the median over the rounds (min and max beside it), timed with
events on the stream the kernels run on.  The outputs of every side are compared bit for bit before anything is timed.
TFLOP/s = executed FLOP / time against the 157.3 of the fp32 MFMA; the stem executes K = 148 of 147."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cabinet_amd import _lib
from cabinet_amd.functional import _ptr, _stream_handle

PEAK_TFLOPS = 157.3
NBUF = 4
CONFIGS = [("config 3", 8, 1024, 1024), ("config 5", 2, 2048, 1024)]
NAMES = ["cabinet_stem_conv_fwd", "cabinet_conv3x3s2_dgrad", "cabinet_last_error"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", action="append", default=[])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    libs = [("this", _lib.load())] + [(os.path.basename(os.path.dirname(os.path.abspath(p))), load_other(p)) for p in a.other]
    dev = torch.device("cuda")
    rows = []
    for cfg, B, H, W in CONFIGS:
        # (operator, input tensors per buffer, output shape, call, executed FLOP)
        ops = []
        Ho, Wo = H // 2, W // 2
        ops.append(("stem_conv_fwd", [(B, 3, H, W)], (B, 64, Ho, Wo), 2.0 * B * Ho * Wo * 64 * 148,
                    lambda lib, ins, w, out, st: lib.cabinet_stem_conv_fwd(_ptr(ins[0]), _ptr(w), B, H, W, _ptr(out), st),
                    (64, 3, 7, 7)))
        for layer, div in (("sb.conv2", 2), ("sb.conv3", 4)):
            h, w_ = H // div, W // div
            ho, wo = h // 2, w_ // 2
            ops.append((f"conv3x3s2_dgrad {layer}", [(B, 64, ho, wo)], (B, 64, h, w_), 2.0 * B * ho * wo * 64 * 64 * 9,
                        (lambda h, w_: lambda lib, ins, w, out, st: lib.cabinet_conv3x3s2_dgrad(_ptr(ins[0]), _ptr(w), B, 64, 64, h, w_,
                                                                                                 _ptr(out), st))(h, w_),
                        (64, 64, 3, 3)))
        for op, in_shapes, out_shape, flop, call, w_shape in ops:
            ins = [[torch.randn(s, device=dev) for s in in_shapes] for _ in range(NBUF)]
            wt = torch.randn(w_shape, device=dev) * 0.1
            sides = []
            for label, lib in libs:
                outs = [torch.empty(out_shape, device=dev) for _ in range(NBUF)]

                def run(lib=lib, outs=outs):
                    st = _stream_handle(dev)
                    for i, o in zip(ins, outs):
                        if call(lib, i, wt, o, st) != 0:
                            raise RuntimeError(lib.cabinet_last_error().decode())
                sides.append((label, capture(run), outs))
            for label, _, outs in sides[1:]:
                same = all(torch.equal(p, q) for p, q in zip(sides[0][2], outs))
                print(f"{cfg}: {op}: {label} vs {sides[0][0]}: outputs {'bit-equal' if same else 'DIFFER'}")
            times = {label: [] for label, _, _ in sides}
            for _ in range(a.rounds):
                for label, graph, _ in sides:
                    times[label].append(replay_us(graph))
            row = {"config": cfg, "op": op}
            for label, t in times.items():
                med = statistics.median(t)
                tf = flop / med * 1e-6
                row[label] = {"us": round(med, 1), "min": round(min(t), 1), "max": round(max(t), 1), "tflops": round(tf, 1)}
                print(f"{cfg}: {op:26s} {label:12s} {med:8.1f} us (min {min(t):.1f}, max {max(t):.1f})  {tf:5.1f} TF/s "
                      f"{tf / PEAK_TFLOPS:4.2f}", flush=True)
            rows.append(row)
            del ins, sides
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
