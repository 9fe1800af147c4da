#!/usr/bin/env python3
"""What cabinet_stem_conv_fwd (K9) and cabinet_conv3x3s2_dgrad (K15) computed BEFORE their staging was pipelined, for
tests/test_gpu_spatial_pipeline.py.

Run on a GPU with the library of the commit in front of that change:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spatial_pipeline.py [--lib PATH/libcabinet_hip.so]
(`--lib`: a build of that commit kept beside the working tree; without it the package's own library is used, i.e. run it on that
commit.)  The cases and their seeded inputs are those of tests/spatial_pipeline_cases.py.  Writes g9_spatial_pipeline.npz, data
only: per case `<key>/sha256` (the digest of the whole output, 32 bytes) and `<key>/sample` (a fixed strided sample of it)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import spatial_pipeline_cases as sp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "g9_spatial_pipeline.npz"))
a = ap.parse_args()
lib = sp.load_library(a.lib)
rec = {}


def keep(k, t):
    assert bool(torch.isfinite(t).all()), k
    rec[k + "/sha256"] = np.frombuffer(bytes.fromhex(sp.digest(t)), dtype=np.uint8)
    rec[k + "/sample"] = sp.sample(t).numpy()


for shape in sp.STEM:
    x, w = sp.stem_inputs(*shape)
    y = torch.full(sp.stem_out(*shape), float("nan"), device="cuda")
    keep(sp.key("stem", shape), sp.run_stem(lib, x.cuda(), w.cuda(), y))
for shape in sp.DGRAD:
    dy, w = sp.dgrad_inputs(*shape)
    dx = torch.full((shape[0], 64, shape[1], shape[2]), float("nan"), device="cuda")
    keep(sp.key("dgrad", shape), sp.run_dgrad(lib, dy.cuda(), w.cuda(), dx))
torch.cuda.synchronize()
np.savez_compressed(a.out, **rec)
print(f"{len(rec) // 2} cases; {os.path.getsize(a.out)} B")
assert os.path.getsize(a.out) < 2 ** 19
