"""Backward of the six thin 1x1 convolutions of features.1 - features.4 TOGETHER with the BatchNorm behind each: the fused entry
points (cabinet_pw_bn_act_bwd, cabinet_pw_bn_dwconv_bwd; csrc/pwconv_wide.hip "BN form") against the chain they replace
(cabinet_bn_act_bwd / cabinet_bn_dwconv_bwd, then cabinet_pwconv_bwd on the stored dz).

    python tools/time_pw_bn_bwd.py [--other PATH/libcabinet_hip.so] [--rounds 5] [--configs 3,5] [--json FILE]
    python tools/time_pw_bn_bwd.py --once [--chain]      one eager call per layer at config 3 (for counters / a kernel trace)

As tools/time_pwconv.py: every operator is captured into a hipGraph of four calls, each on its own copy of the operands and
results (cold operands: the planes do not sit in the last-level cache between calls), and the graphs are replayed alternately;
with `--other` the chain runs from that build of the library (the parent commit's).  Median, min - max over the rounds, events on
the stream.  Bytes are algorithmic, T = the tensor on the convolution's output side, t = the one on its input side:
closing form   chain 2 T (reduce) + 5 T + 2 t      fused 2 T + 2 T + 2 t
depthwise form chain dy + 2 T (K8: z, da) + 5 T + 2 t   fused dy + 2 T + 2 T + 2 t
A layer is routed to the fused call where its maximum is below the chain's minimum (the K10 rule)."""
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
# (name, Ci, Co, plane divisor, depthwise (K, stride) or None, act of the BatchNorm)
LAYERS = [("features.2 expand", 16, 64, 2, (3, 2), 1), ("features.3 expand", 24, 72, 4, (3, 1), 1),
          ("features.4 expand", 24, 72, 4, (5, 2), 1), ("features.1 project", 16, 16, 2, None, 0),
          ("features.2 project", 64, 24, 4, None, 0), ("features.3 project", 72, 24, 4, None, 0)]
CONFIGS = {"3": ("config 3", 8, 1024, 1024), "5": ("config 5", 2, 2048, 1024)}
CHAIN_NAMES = ("cabinet_bn_act_bwd", "cabinet_bn_act_workspace_bytes", "cabinet_bn_dwconv_bwd", "cabinet_bn_dwconv_bwd_workspace_bytes",
               "cabinet_pwconv_bwd", "cabinet_pwconv_bwd_workspace_bytes", "cabinet_last_error")


def other_library(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in CHAIN_NAMES:
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


def replay_us(graph, nbuf, n=3):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / (n * nbuf) * 1e3


def layer_ops(this, chain_lib, B, ci, co, h, w, dwc, act, nbuf):
    """-> {"fused": (callable, bytes), "chain": (callable, bytes)} on `nbuf` sets of operands"""
    P, dev = h * w, torch.device("cuda")
    xs = [torch.randn(B, ci, P, device=dev) for _ in range(nbuf)]
    zs = [torch.randn(B, co, P, device=dev) for _ in range(nbuf)]
    dxs = [torch.empty_like(x) for x in xs]
    wt, dw = torch.randn(co, ci, device=dev) * ci ** -0.5, torch.empty(co, ci, device=dev)
    gam, bet = torch.randn(co, device=dev), torch.randn(co, device=dev) * 0.3
    mean, invstd = torch.zeros(co, device=dev), torch.ones(co, device=dev)
    dgam, dbet = torch.empty_like(gam), torch.empty_like(bet)
    dz = torch.empty(B, co, P, device=dev)  # the chain's intermediate (one: it is written and read back at once, as in the step)
    T, t = 4.0 * B * co * P, 4.0 * B * ci * P

    def ok(lib, rc, who):
        if rc != 0:
            raise RuntimeError(f"{who}: rc {rc}: {lib.cabinet_last_error().decode()}")

    ws_pw, nb_pw = _workspace(chain_lib.cabinet_pwconv_bwd_workspace_bytes(B, ci, co, P), dev)
    if dwc is None:
        gs = [torch.randn(B, co, P, device=dev) for _ in range(nbuf)]
        ws_f, nb_f = _workspace(this.cabinet_pw_bn_act_bwd_workspace_bytes(B, ci, co, P), dev)
        ws_c, nb_c = _workspace(chain_lib.cabinet_bn_act_workspace_bytes(B, co, P), dev)

        def fused():
            st = _stream_handle(dev)
            for x, z, g, dx in zip(xs, zs, gs, dxs):
                ok(this, this.cabinet_pw_bn_act_bwd(_ptr(g), _ptr(z), _ptr(x), _ptr(wt), _ptr(gam), _ptr(bet), _ptr(mean), _ptr(invstd),
                                                    B, ci, co, P, act, 1, _ptr(dx), _ptr(dw), _ptr(dgam), _ptr(dbet), _ptr(ws_f), nb_f,
                                                    st), "pw_bn_act_bwd")

        def chain():
            st = _stream_handle(dev)
            for x, z, g, dx in zip(xs, zs, gs, dxs):
                ok(chain_lib, chain_lib.cabinet_bn_act_bwd(_ptr(g), _ptr(z), _ptr(gam), _ptr(bet), _ptr(mean), _ptr(invstd), B, co, P,
                                                           act, 1, _ptr(dz), _ptr(dgam), _ptr(dbet), _ptr(ws_c), nb_c, st), "bn_act_bwd")
                ok(chain_lib, chain_lib.cabinet_pwconv_bwd(_ptr(dz), _ptr(x), _ptr(wt), B, ci, co, P, _ptr(dx), _ptr(dw), _ptr(ws_pw),
                                                           nb_pw, st), "pwconv_bwd")

        return {"fused": (fused, 4 * T + 2 * t), "chain": (chain, 7 * T + 2 * t)}

    K, s = dwc
    ho, wo = (h + 2 * (K // 2) - K) // s + 1, (w + 2 * (K // 2) - K) // s + 1
    gs = [torch.randn(B, co, ho, wo, device=dev) for _ in range(nbuf)]
    cw, dcw = torch.randn(co, 1, K, K, device=dev) / K, torch.empty(co, 1, K, K, device=dev)
    ws_f, nb_f = _workspace(this.cabinet_pw_bn_dwconv_bwd_workspace_bytes(B, ci, co, h, w, K, s), dev)
    ws_c, nb_c = _workspace(chain_lib.cabinet_bn_dwconv_bwd_workspace_bytes(B, co, h, w, K, s), dev)
    dy = 4.0 * B * co * ho * wo

    def fused():
        st = _stream_handle(dev)
        for x, z, g, dx in zip(xs, zs, gs, dxs):
            ok(this, this.cabinet_pw_bn_dwconv_bwd(_ptr(g), _ptr(z), _ptr(x), _ptr(wt), _ptr(gam), _ptr(bet), _ptr(mean), _ptr(invstd),
                                                   _ptr(cw), B, ci, co, h, w, K, s, act, 1, _ptr(dx), _ptr(dw), _ptr(dgam), _ptr(dbet),
                                                   _ptr(dcw), _ptr(ws_f), nb_f, st), "pw_bn_dwconv_bwd")

    def chain():
        st = _stream_handle(dev)
        for x, z, g, dx in zip(xs, zs, gs, dxs):
            ok(chain_lib, chain_lib.cabinet_bn_dwconv_bwd(_ptr(g), _ptr(z), _ptr(gam), _ptr(bet), _ptr(mean), _ptr(invstd), _ptr(cw), B,
                                                          co, h, w, K, s, act, 1, _ptr(dz), _ptr(dgam), _ptr(dbet), _ptr(dcw), _ptr(ws_c),
                                                          nb_c, st), "bn_dwconv_bwd")
            ok(chain_lib, chain_lib.cabinet_pwconv_bwd(_ptr(dz), _ptr(x), _ptr(wt), B, ci, co, P, _ptr(dx), _ptr(dw), _ptr(ws_pw), nb_pw,
                                                       st), "pwconv_bwd")

    return {"fused": (fused, dy + 4 * T + 2 * t), "chain": (chain, dy + 7 * T + 2 * t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None, help="another build of libcabinet_hip.so (the parent's) to run the chain from")
    ap.add_argument("--once", action="store_true", help="one eager call per layer at the first config; no timing")
    ap.add_argument("--chain", action="store_true", help="with --once: the chain instead of the fused call")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    this = _lib.load()
    chain_lib = other_library(a.other) if a.other else this
    rows = []
    for cfg in a.configs.split(","):
        name, B, H, W = CONFIGS[cfg]
        print(f"--- {name}: B = {B}, {H} x {W}")
        for lname, ci, co, div, dwc, act in LAYERS:
            h, w = H // div, W // div
            nbuf = 1 if a.once else NBUF
            ops = layer_ops(this, chain_lib, B, ci, co, h, w, dwc, act, nbuf)
            if a.once:
                ops["chain" if a.chain else "fused"][0]()
                torch.cuda.synchronize()
                continue
            graphs = {side: capture(fn) for side, (fn, _) in ops.items()}
            times = {side: [] for side in graphs}
            for _ in range(a.rounds):
                for side, g in graphs.items():
                    times[side].append(replay_us(g, nbuf))
            routed = max(times["fused"]) < min(times["chain"])
            for side, ts in times.items():
                med, nbytes = statistics.median(ts), ops[side][1]
                print(f"{lname:19s} {ci:3d}->{co:3d} @{h:4d}x{w:4d} {side:5s}: {med:7.1f} us ({min(ts):7.1f} - {max(ts):7.1f})  "
                      f"{nbytes / 1e6:7.1f} MB  {nbytes / med * 1e-6:5.2f} TB/s" + (f"  fused max < chain min: {routed}" if side == "fused" else ""))
                rows.append({"config": name, "layer": lname, "ci": ci, "co": co, "h": h, "w": w, "side": side,
                             "median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                             "mbytes": round(nbytes / 1e6, 2), "tbs": round(nbytes / med * 1e-6, 3), "fused_routed": routed})
            del graphs, ops
            torch.cuda.empty_cache()
        if a.once:
            break
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
