#!/usr/bin/env python3
"""What cabinet_conv3x3s2_wgrad (K15, 64 -> 64) computed BEFORE its staging was pipelined, for
tests/test_gpu_conv3x3s2_wgrad64.py.

Run on a GPU with the library of the commit in front of that change:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wgrad64.py [--lib PATH/libcabinet_hip.so]
(`--lib`: a build of that commit kept beside the working tree; without it the package's own library is used, i.e. run it on that
commit.)  The cases and their seeded inputs are those of tests/wgrad64_cases.py.  Writes g12_wgrad64.npz, data only: per case
`<key>/sha256` (the digest of the whole dW, 32 bytes) and `<key>/sample` (a fixed strided sample of it)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wgrad64_cases as wc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "g12_wgrad64.npz"))
a = ap.parse_args()
lib = wc.load_library(a.lib)
rec = {}
for shape in wc.SHAPES:
    x, dy = wc.inputs(*shape)
    dw = wc.run_wgrad(lib, dy.cuda(), x.cuda(), torch.full((64, 64, 3, 3), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw).all()), shape
    rec[wc.key(shape) + "/sha256"] = np.frombuffer(bytes.fromhex(wc.digest(dw)), dtype=np.uint8)
    rec[wc.key(shape) + "/sample"] = wc.sample(dw).numpy()
np.savez_compressed(a.out, **rec)
print(f"{len(rec) // 2} cases; {os.path.getsize(a.out)} B")
assert os.path.getsize(a.out) < 2 ** 17
