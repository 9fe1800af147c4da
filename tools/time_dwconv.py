"""Depthwise convolutions (K8): cabinet_dwconv_fwd / cabinet_dwconv_bwd of TWO builds of the library, per backbone layer.

    python tools/time_dwconv.py --other PATH/libcabinet_hip.so [--rounds 5] [--json FILE]

`--other` is a second build of libcabinet_hip.so (the parent commit's, say); the package's own library is "this".  The 15
depthwise layers of the MobileNetV3 backbone at BASELINE config 3 (B = 8, 1024 x 1024) and config 5 (B = 2, 2048 x 1024).  Each side
is captured into a hipGraph (four calls, each on its own copy of the operands so that they do not sit in the 256 MB last-level
cache between calls) and the two graphs are replayed alternately in one process; the figure is the median over the rounds, timed
with events on the stream the kernels run on.  The backward figure includes dwconv_dw_finalize_kernel.  TB/s = algorithmic bytes
(forward: x + y; backward: dy + x + dx) / time; HBM peak 8 TB/s.  The plain entry points are timed: the fused form runs the same
kernels with the BatchNorm expression in their loaders.  An instantiation (K, S, direction) keeps its strip kernel only if it is
faster than the one-tile kernel at some layer of the workload."""
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
# (name, channels, K, S, plane divisor of the image): torchvision mobilenet_v3_large features.1 .. features.15
LAYERS = [("features.1", 16, 3, 1, 2), ("features.2", 64, 3, 2, 2), ("features.3", 72, 3, 1, 4), ("features.4", 72, 5, 2, 4),
          ("features.5", 120, 5, 1, 8), ("features.6", 120, 5, 1, 8), ("features.7", 240, 3, 2, 8), ("features.8", 200, 3, 1, 16),
          ("features.9", 184, 3, 1, 16), ("features.10", 184, 3, 1, 16), ("features.11", 480, 3, 1, 16),
          ("features.12", 672, 3, 1, 16), ("features.13", 672, 5, 2, 16), ("features.14", 960, 5, 1, 32),
          ("features.15", 960, 5, 1, 32)]
CONFIGS = [("config 3", 8, 1024, 1024), ("config 5", 2, 2048, 1024)]
NAMES = ["cabinet_dwconv_fwd", "cabinet_dwconv_bwd", "cabinet_dwconv_bwd_workspace_bytes", "cabinet_last_error"]


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
    ap.add_argument("--other", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    this, other = _lib.load(), load_other(a.other)
    rows = []
    for name, B, H, W in CONFIGS:
        print(f"--- {name}: B = {B}, {H} x {W}   (us: other -> this)")
        for layer, C, K, S, div in LAYERS:
            h, w = H // div, W // div
            ho, wo = (h - 1) // S + 1, (w - 1) // S + 1
            xs = [torch.randn(B, C, h, w, device="cuda") for _ in range(NBUF)]
            gs = [torch.randn(B, C, ho, wo, device="cuda") for _ in range(NBUF)]
            ys = [torch.empty_like(g) for g in gs]
            dxs = [torch.empty_like(x) for x in xs]
            wt = torch.randn(C, 1, K, K, device="cuda")
            dw = torch.empty_like(wt)
            nbytes = this.cabinet_dwconv_bwd_workspace_bytes(B, C, h, w, K, S)
            assert nbytes == other.cabinet_dwconv_bwd_workspace_bytes(B, C, h, w, K, S)
            ws, nb = _workspace(nbytes, wt.device)

            def fwd(lib):
                def run():
                    st = _stream_handle(wt.device)
                    for x, y in zip(xs, ys):
                        if lib.cabinet_dwconv_fwd(_ptr(x), _ptr(wt), B, C, h, w, K, S, _ptr(y), st) != 0:
                            raise RuntimeError(lib.cabinet_last_error().decode())
                return run

            def bwd(lib):
                def run():
                    st = _stream_handle(wt.device)
                    for x, g, dx in zip(xs, gs, dxs):
                        if lib.cabinet_dwconv_bwd(_ptr(g), _ptr(x), _ptr(wt), B, C, h, w, K, S, _ptr(dx), _ptr(dw), _ptr(ws), nb, st) != 0:
                            raise RuntimeError(lib.cabinet_last_error().decode())
                return run

            f0, f1 = alternate([fwd(other), fwd(this)], a.rounds)
            b0, b1 = alternate([bwd(other), bwd(this)], a.rounds)
            fb, bb = 4.0 * B * C * (h * w + ho * wo), 4.0 * B * C * (2 * h * w + ho * wo)
            print(f"{layer:12s} K{K} S{S} {C:4d} x {h:4d} x {w:4d}: fwd {f0:7.1f} -> {f1:7.1f} us ({fb / f0 * 1e-6:4.2f} -> {fb / f1 * 1e-6:4.2f} TB/s)"
                  f" | bwd {b0:7.1f} -> {b1:7.1f} us ({bb / b0 * 1e-6:4.2f} -> {bb / b1 * 1e-6:4.2f} TB/s)", flush=True)
            rows.append({"config": name, "layer": layer, "C": C, "K": K, "S": S, "h": h, "w": w, "fwd_other_us": round(f0, 2),
                         "fwd_this_us": round(f1, 2), "bwd_other_us": round(b0, 2), "bwd_this_us": round(b1, 2),
                         "fwd_bytes": fb, "bwd_bytes": bb})
            del xs, gs, ys, dxs
        for K, S in ((3, 1), (3, 2), (5, 1), (5, 2)):
            sel = [r for r in rows if r["config"] == name and (r["K"], r["S"]) == (K, S)]
            print(f"    K{K} S{S} total: fwd {sum(r['fwd_other_us'] for r in sel):7.1f} -> {sum(r['fwd_this_us'] for r in sel):7.1f} us"
                  f" | bwd {sum(r['bwd_other_us'] for r in sel):7.1f} -> {sum(r['bwd_this_us'] for r in sel):7.1f} us")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
