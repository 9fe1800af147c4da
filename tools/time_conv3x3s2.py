"""Backward of the 3x3 stride-2 convolutions: cabinet_conv3x3s2_wgrad / _dgrad (K15) vs the stock operator, per layer.

    python tools/time_conv3x3s2.py [--rounds 5] [--json FILE]

The three layers (spatial branch conv2 and conv3, 64 -> 64; backbone features.0, 3 -> 16) at BASELINE config 3 (B = 8,
1024 x 1024) and config 5 (B = 2, 2048 x 1024).  Each side is captured into a hipGraph (four calls, each on its own copy of x
and dy so that the operands do not sit in the 256 MB last-level cache between calls) and the two graphs are replayed
alternately in one process; the figure is the median over the rounds, timed with events on the stream the kernels run on.
The stock side is the whole aten.convolution_backward call with mask [False, True, False]: its NCHW <-> NHWC copies of x, dy
and dw are part of what it costs.  The input gradient of conv2 / conv3 is the call with mask [True, False, False] (MIOpen reads
NCHW there: no copies) against cabinet_conv3x3s2_dgrad; its four calls write four copies of dx.  The last line times
cabinet_stem_conv_wrw (K9), whose slab sum changed.  TFLOP/s = 2 B Ho Wo Ci Co 9 / time; peak 157.3 (fp32 MFMA).  The table
decides the routing in functional.py::_Conv3x3S2 (an operator is routed where native beats stock at both configurations)."""
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
# (name, Ci, Co, plane divisor of the image)
LAYERS = [("sb.conv2", 64, 64, 2), ("sb.conv3", 64, 64, 4), ("features.0", 3, 16, 1)]
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


def alternate(fns, rounds):
    graphs = [capture(f) for f in fns]
    times = [[] for _ in fns]
    for _ in range(rounds):
        for g, t in zip(graphs, times):
            t.append(replay_ms(g))
    return [statistics.median(t) * 1e3 for t in times]  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    cb = torch.ops.aten.convolution_backward
    rows = []
    for name, B, H, W in CONFIGS:
        print(f"--- {name}: B = {B}, {H} x {W}")
        for layer, ci, co, div in LAYERS:
            h, w = H // div, W // div
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            xs = [torch.randn(B, ci, h, w, device="cuda") for _ in range(NBUF)]
            gs = [torch.randn(B, co, ho, wo, device="cuda") for _ in range(NBUF)]
            wt = torch.randn(co, ci, 3, 3, device="cuda")
            dw = torch.empty(co, ci, 3, 3, device="cuda")
            ws, nb = _workspace(lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, ci, co, h, w), wt.device)

            def native():
                st = _stream_handle(wt.device)
                for x, g in zip(xs, gs):
                    _lib.check(lib.cabinet_conv3x3s2_wgrad(_ptr(g), _ptr(x), B, ci, co, h, w, _ptr(dw), _ptr(ws), nb, st),
                               "cabinet_conv3x3s2_wgrad")

            def stock():
                for x, g in zip(xs, gs):
                    cb(g, x, wt, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])

            def stock_dx():
                for x, g in zip(xs, gs):
                    cb(g, x, wt, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])

            m0, m1 = alternate([stock, native], a.rounds)
            flop = 2.0 * B * ho * wo * ci * co * 9
            tf0, tf1 = flop / m0 * 1e-6, flop / m1 * 1e-6
            print(f"{layer:10s} wgrad {ci:2d}->{co:2d} @{h:4d}x{w:4d}: stock {m0:7.1f} us {tf0:5.1f} TF/s {tf0 / PEAK_TFLOPS:4.2f} | "
                  f"native {m1:7.1f} us {tf1:5.1f} TF/s {tf1 / PEAK_TFLOPS:4.2f} | x{m0 / m1:4.2f}")
            row = {"config": name, "layer": layer, "op": "wgrad", "ci": ci, "co": co, "h": h, "w": w, "stock_us": round(m0, 2),
                   "native_us": round(m1, 2), "stock_tflops": round(tf0, 2), "native_tflops": round(tf1, 2)}
            rows.append(row)
            if ci == 64:
                dxs = [torch.empty_like(x) for x in xs]

                def native_dx():
                    st = _stream_handle(wt.device)
                    for g, dx in zip(gs, dxs):
                        _lib.check(lib.cabinet_conv3x3s2_dgrad(_ptr(g), _ptr(wt), B, ci, co, h, w, _ptr(dx), st),
                                   "cabinet_conv3x3s2_dgrad")

                d0, d1 = alternate([stock_dx, native_dx], a.rounds)
                tf0, tf1 = flop / d0 * 1e-6, flop / d1 * 1e-6
                print(f"{layer:10s} dgrad {ci:2d}->{co:2d} @{h:4d}x{w:4d}: stock {d0:7.1f} us {tf0:5.1f} TF/s {tf0 / PEAK_TFLOPS:4.2f} | "
                      f"native {d1:7.1f} us {tf1:5.1f} TF/s {tf1 / PEAK_TFLOPS:4.2f} | x{d0 / d1:4.2f}")
                rows.append({"config": name, "layer": layer, "op": "dgrad", "ci": ci, "co": co, "h": h, "w": w,
                             "stock_us": round(d0, 2), "native_us": round(d1, 2), "stock_tflops": round(tf0, 2),
                             "native_tflops": round(tf1, 2)})
                del dxs
            del xs, gs
        # K9's weight gradient, for its slab sum
        ho, wo = H // 2, W // 2
        xs = [torch.randn(B, 3, H, W, device="cuda") for _ in range(NBUF)]
        gs = [torch.randn(B, 64, ho, wo, device="cuda") for _ in range(NBUF)]
        dw = torch.empty(64, 3, 7, 7, device="cuda")
        ws, nb = _workspace(lib.cabinet_stem_conv_wrw_workspace_bytes(B, H, W), dw.device)

        def stem():
            st = _stream_handle(dw.device)
            for x, g in zip(xs, gs):
                _lib.check(lib.cabinet_stem_conv_wrw(_ptr(g), _ptr(x), B, H, W, _ptr(dw), _ptr(ws), nb, st), "cabinet_stem_conv_wrw")

        (s1,) = alternate([stem], a.rounds)
        print(f"sb.conv1   wgrad  3->64 @{H:4d}x{W:4d}: native {s1:7.1f} us (K9 with its slab sum)")
        rows.append({"config": name, "layer": "sb.conv1", "op": "wgrad", "native_us": round(s1, 2)})
        del xs, gs
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
