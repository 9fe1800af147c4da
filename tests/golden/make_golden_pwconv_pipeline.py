#!/usr/bin/env python3
"""What cabinet_pwconv_fwd / cabinet_pwconv_bwd (K10) computed BEFORE their kernels were pipelined, for
tests/test_gpu_pwconv_pipeline.py.

Run on a GPU with the library of the commit in front of that change:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pwconv_pipeline.py [--lib PATH/libcabinet_hip.so]
(`--lib`: a build of that commit kept beside the working tree; without it the package's own library is used, i.e. run it on that
commit.)  The cases and their seeded inputs are those of tests/pwconv_pipeline_cases.py.  Writes g10_pwconv_pipeline.npz, data
only: per case `<key>/y/sha256`, `<key>/dx/sha256` (the digest of the whole output, 32 bytes), `<key>/y/sample`, `<key>/dx/sample`
(a fixed strided sample), `<key>/dw/sha256` and `<key>/dw/dist`, the relative distance of that commit's dW from the fp64 product."""
import argparse
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pwconv_pipeline_cases as pc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "g10_pwconv_pipeline.npz"))
a = ap.parse_args()
lib = pc.load_library(a.lib)
rec = {}
for case in pc.CASES:
    B, Ci, Co, P, mis = case
    x, w, g = pc.inputs(B, Ci, Co, P)
    y, dx, dw = pc.run(lib, pc.on_device(x, mis), pc.on_device(w, False), pc.on_device(g, mis), mis)
    torch.cuda.synchronize()
    k = pc.key(case)
    for name, t in (("y", y), ("dx", dx)):
        assert bool(torch.isfinite(t).all()), (k, name)
        rec[f"{k}/{name}/sha256"] = np.frombuffer(bytes.fromhex(pc.digest(t)), dtype=np.uint8)
        rec[f"{k}/{name}/sample"] = pc.sample(t).numpy()
    assert bool(torch.isfinite(dw).all()), k
    rec[f"{k}/dw/sha256"] = np.frombuffer(bytes.fromhex(pc.digest(dw)), dtype=np.uint8)
    rec[f"{k}/dw/dist"] = np.float64(pc.dist(dw, pc.dw_ref(x, g)))
    print(f"{k}: dW distance from fp64 {float(rec[f'{k}/dw/dist']):.3e}")
np.savez_compressed(a.out, **rec)
print(f"{len(pc.CASES)} cases; {os.path.getsize(a.out)} B")
assert os.path.getsize(a.out) < 2 ** 19
