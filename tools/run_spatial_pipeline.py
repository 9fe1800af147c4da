#!/usr/bin/env python3
"""Launch cabinet_stem_conv_fwd (K9) and cabinet_conv3x3s2_dgrad (K15, sb.conv2's and sb.conv3's planes) `iters` times each, alone,
for counter passes of rocprofv3 (bench.py has no kernel group for the input gradient):

    rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES -- python tools/run_spatial_pipeline.py 3 [--lib PATH]

`--lib` is another build of libcabinet_hip.so (the parent commit's).  Shapes: CAB_B x 3 x CAB_H x CAB_W as tools/run_kernels.py
(defaults = BASELINE config 3: 8 x 3 x 1024 x 1024)."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from cabinet_amd import _lib  # noqa: E402
from cabinet_amd.functional import _ptr, _stream_handle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("iters", type=int, nargs="?", default=3)
ap.add_argument("--lib", default=None)
a = ap.parse_args()
lib = _lib.load()
if a.lib:
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    for name in ("cabinet_stem_conv_fwd", "cabinet_conv3x3s2_dgrad"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
B = int(os.environ.get("CAB_B", "8"))
H = int(os.environ.get("CAB_H", os.environ.get("CAB_SIZE", "1024")))
W = int(os.environ.get("CAB_W", os.environ.get("CAB_SIZE", "1024")))
dev = torch.device("cuda")
st = _stream_handle(dev)
x, w7 = torch.randn(B, 3, H, W, device=dev), torch.randn(64, 3, 7, 7, device=dev) * 0.1
y = torch.empty(B, 64, H // 2, W // 2, device=dev)
for _ in range(a.iters):
    assert lib.cabinet_stem_conv_fwd(_ptr(x), _ptr(w7), B, H, W, _ptr(y), st) == 0
torch.cuda.synchronize()
w3 = torch.randn(64, 64, 3, 3, device=dev) * 0.05
for div in (2, 4):
    h, w = H // div, W // div
    dy, dx = torch.randn(B, 64, h // 2, w // 2, device=dev), torch.empty(B, 64, h, w, device=dev)
    for _ in range(a.iters):
        assert lib.cabinet_conv3x3s2_dgrad(_ptr(dy), _ptr(w3), B, 64, 64, h, w, _ptr(dx), st) == 0
    torch.cuda.synchronize()
