"""The stem's backward behind relu(bn(stem_conv(image))) (K9 + K7), operator alone: the pair cabinet_bn_act_bwd +
cabinet_stem_conv_wrw against the one call cabinet_stem_conv_bn_bwd, which never writes the BatchNorm's input gradient.

    python tools/time_stem_bwd.py [--other PATH/libcabinet_hip.so] [--rounds 5] [--json FILE]

`--other` is a second build of libcabinet_hip.so (the parent commit's, say): its pair is timed as well.  BASELINE config 3
(B = 8, 1024 x 1024) and config 5 (B = 2, 2048 x 1024).  Each side is captured into a hipGraph (NBUF calls, each on its own copy of
g and z: the 537 MB planes do not fit the 256 MB last-level cache, the copies only keep one call's tail out of the next one's
head) and the graphs are replayed alternately in one process; the figure is the median over the rounds, timed with events on the
stream the kernels run on.  The three gradients of every side are compared bit for bit before anything is timed."""
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

NBUF = 2
CONFIGS = [("config 3", 8, 1024, 1024), ("config 5", 2, 2048, 1024)]
PAIR = ["cabinet_bn_act_bwd", "cabinet_bn_act_workspace_bytes", "cabinet_stem_conv_wrw", "cabinet_stem_conv_wrw_workspace_bytes",
        "cabinet_last_error"]


def load_other(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in PAIR:
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
    ap.add_argument("--other", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    this = _lib.load()
    other = load_other(a.other) if a.other else None
    rows = []
    for name, B, H, W in CONFIGS:
        Ho, Wo = H // 2, W // 2
        P = Ho * Wo
        dev = torch.device("cuda")
        x = torch.randn(B, 3, H, W, device=dev)
        zs = [torch.randn(B, 64, Ho, Wo, device=dev) for _ in range(NBUF)]
        gs = [torch.randn(B, 64, Ho, Wo, device=dev) for _ in range(NBUF)]
        dz = torch.empty(B, 64, Ho, Wo, device=dev)
        gam, bet = torch.randn(64, device=dev), torch.randn(64, device=dev) * 0.5
        mean, invstd = zs[0].mean((0, 2, 3)), torch.rsqrt(zs[0].var((0, 2, 3), unbiased=False) + 1e-5)

        def outs():
            return torch.empty(64, 3, 7, 7, device=dev), torch.empty(64, device=dev), torch.empty(64, device=dev)

        def pair(lib):
            dw, dgam, dbet = outs()
            nb1, nb2 = lib.cabinet_bn_act_workspace_bytes(B, 64, P), lib.cabinet_stem_conv_wrw_workspace_bytes(B, H, W)
            ws1, ws2 = torch.empty(nb1, dtype=torch.uint8, device=dev), torch.empty(nb2, dtype=torch.uint8, device=dev)

            def run():
                st = _stream_handle(dev)
                for g, z in zip(gs, zs):
                    rc = lib.cabinet_bn_act_bwd(_ptr(g), _ptr(z), _ptr(gam), _ptr(bet), _ptr(mean), _ptr(invstd), B, 64, P, 1, 1,
                                                _ptr(dz), _ptr(dgam), _ptr(dbet), _ptr(ws1), nb1, st)
                    rc = rc or lib.cabinet_stem_conv_wrw(_ptr(dz), _ptr(x), B, H, W, _ptr(dw), _ptr(ws2), nb2, st)
                    if rc != 0:
                        raise RuntimeError(lib.cabinet_last_error().decode())
            return run, (dw, dgam, dbet)

        def fused(lib):
            dw, dgam, dbet = outs()
            nb = lib.cabinet_stem_conv_bn_bwd_workspace_bytes(B, H, W)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)

            def run():
                st = _stream_handle(dev)
                for g, z in zip(gs, zs):
                    if lib.cabinet_stem_conv_bn_bwd(_ptr(g), _ptr(z), _ptr(x), _ptr(gam), _ptr(bet), _ptr(mean), _ptr(invstd), B, H,
                                                    W, 1, _ptr(dw), _ptr(dgam), _ptr(dbet), _ptr(ws), nb, st) != 0:
                        raise RuntimeError(lib.cabinet_last_error().decode())
            return run, (dw, dgam, dbet)

        sides = ([("other pair", pair(other))] if other else []) + [("this pair", pair(this)), ("this fused", fused(this))]
        graphs = [(label, capture(run), out) for label, (run, out) in sides]
        for label, _, out in graphs[1:]:
            same = all(torch.equal(p, q) for p, q in zip(graphs[0][2], out))
            print(f"{name}: {label} vs {graphs[0][0]}: gradients {'bit-equal' if same else 'DIFFER'}")
        times = {label: [] for label, _, _ in graphs}
        for _ in range(a.rounds):
            for label, graph, _ in graphs:
                times[label].append(replay_us(graph))
        row = {"config": name, "B": B, "H": H, "W": W}
        for label, t in times.items():
            row[label.replace(" ", "_") + "_us"] = round(statistics.median(t), 1)
            print(f"{name}: {label:11s} {statistics.median(t):8.1f} us  (min {min(t):.1f}, max {max(t):.1f})", flush=True)
        rows.append(row)
        del zs, gs, dz, graphs, sides
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
