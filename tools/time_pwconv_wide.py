"""Weight gradient of the wide pointwise layers: cabinet_pwconv_wide_wgrad (K14) vs the stock operator, per layer shape.

    python tools/time_pwconv_wide.py [--rounds 7] [--json FILE]

The 25 layers the stock operator served at BASELINE config 3 (B = 8, 1024 x 1024) and the same layers at config 5 (B = 2,
2048 x 1024).  Each side is captured into a hipGraph (four calls, each on its own copy of x and dy so that the operands of
the big planes do not sit in the 256 MB last-level cache between calls) and the two graphs are replayed alternately in one
process; the figure is the median over the rounds, timed with events on the stream the kernels run on, as
bench.py::time_kernel does.  The stock side is the whole aten.convolution_backward call with mask [False, True, False]:
its NCHW -> NHWC copies of x and dy are part of what it costs.  TFLOP/s = 2 B P Ci Co / time; peak 157.3 (fp32 MFMA)."""
import argparse
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
# (Ci, Co, plane divisor of the input, how many layers of the model have this shape)
LAYERS = [(72, 40, 8, 1), (40, 120, 8, 2), (120, 40, 8, 2), (40, 240, 8, 1), (64, 128, 8, 1),
          (240, 80, 16, 1), (80, 200, 16, 1), (200, 80, 16, 1), (80, 184, 16, 2), (184, 80, 16, 2), (80, 480, 16, 1),
          (480, 112, 16, 1), (112, 672, 16, 2), (672, 112, 16, 1),
          (672, 160, 32, 1), (160, 960, 32, 3), (960, 160, 32, 2)]
CONFIGS = [("config 3", 8, 1024, 1024), ("config 5", 2, 2048, 1024)]


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


def replay_ms(graph, n=3):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / (n * NBUF)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    cb = torch.ops.aten.convolution_backward
    rows = []
    for name, B, H, W in CONFIGS:
        tot0 = tot1 = 0.0
        print(f"--- {name}: B = {B}, {H} x {W}")
        for ci, co, div, count in LAYERS:
            h, w = H // div, W // div
            P = h * w
            xs = [torch.randn(B, ci, h, w, device="cuda") for _ in range(NBUF)]
            gs = [torch.randn(B, co, h, w, device="cuda") for _ in range(NBUF)]
            wt = torch.randn(co, ci, 1, 1, device="cuda")
            dw = torch.empty(co, ci, device="cuda")
            ws, nb = _workspace(lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, ci, co, P), wt.device)

            def native():
                st = _stream_handle(wt.device)
                for x, g in zip(xs, gs):
                    _lib.check(lib.cabinet_pwconv_wide_wgrad(_ptr(g), _ptr(x), B, ci, co, P, _ptr(dw), _ptr(ws), nb, st),
                               "cabinet_pwconv_wide_wgrad")

            def stock():
                for x, g in zip(xs, gs):
                    cb(g, x, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False])

            g1, g0 = capture(native), capture(stock)
            t1, t0 = [], []
            for _ in range(a.rounds):
                t0.append(replay_ms(g0))
                t1.append(replay_ms(g1))
            m0, m1 = statistics.median(t0) * 1e3, statistics.median(t1) * 1e3  # us
            flop = 2.0 * B * P * ci * co
            tf0, tf1 = flop / m0 * 1e-6, flop / m1 * 1e-6
            tot0, tot1 = tot0 + count * m0, tot1 + count * m1
            print(f"{ci:4d}->{co:4d} @{h:3d}x{w:3d} x{count}: stock {m0:7.1f} us {tf0:5.1f} TF/s {tf0 / PEAK_TFLOPS:4.2f} | "
                  f"native {m1:7.1f} us {tf1:5.1f} TF/s {tf1 / PEAK_TFLOPS:4.2f} | x{m0 / m1:4.2f}")
            rows.append({"config": name, "ci": ci, "co": co, "h": h, "w": w, "count": count, "stock_us": round(m0, 2),
                         "native_us": round(m1, 2), "stock_tflops": round(tf0, 2), "native_tflops": round(tf1, 2)})
            del g0, g1
        print(f"{name}: all 25 layers: stock {tot0:7.1f} us, native {tot1:7.1f} us per step")
        rows.append({"config": name, "total_stock_us": round(tot0, 1), "total_native_us": round(tot1, 1)})
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
