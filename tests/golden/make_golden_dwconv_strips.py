#!/usr/bin/env python3
"""What the depthwise kernels (K8) computed BEFORE the strip-walking rewrite, for tests/test_gpu_dwconv_strips.py.

Run on a GPU, on the commit in front of the rewrite:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dwconv_strips.py
The cases and their inputs are those of tests/dwconv_strips_cases.py.  Writes, data only:
  g8_dwconv_strips.json   per case the SHA-256 of the bytes of every tensor whose arithmetic the rewrite must not change (plain
                          form: y, dx; fused form: y, and dz in eval mode, where it does not depend on the batch sums) and that
                          commit's own relative distance ||a - b|| / ||b|| from the fp64 oracle for the regrouped sums (dw; fused:
                          dconv_weight, dbn_weight, dbn_bias and the training-mode dz)
  g8_dwconv_strips.npz    the same tensors in full for the shapes below FULL_NUMEL elements (a digest says that bits differ,
                          a tensor says where)
"""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from conftest import rel_err  # noqa: E402

import dwconv_strips_cases as dc  # noqa: E402
from test_gpu_backbone_edges import _dw_dev  # noqa: E402

rec, full = {}, {}


def keep(k, name, t, shape):
    assert bool(torch.isfinite(t).all()), (k, name)
    rec[k][name] = dc.digest(t)
    if shape[0] * shape[1] * shape[2] * shape[3] <= dc.FULL_NUMEL:
        full[f"{k}/{name}"] = t.detach().cpu().numpy()


for shape, K, S in dc.plain_cases():
    k = dc.key(shape, K, S)
    x, w, g, (yo, dxo, dwo) = dc.plain_case(shape, K, S)
    y, dx, dw = _dw_dev(x, w, g, S)
    torch.cuda.synchronize()
    rec[k] = {}
    keep(k, "y", y, shape)
    keep(k, "dx", dx, shape)
    rec[k]["err"] = {"dw": rel_err(dw, dwo)}
    assert rel_err(y, yo) < 1e-5 and rel_err(dx, dxo) < 1e-5 and rec[k]["err"]["dw"] < 1e-5, k

for shape, K, S, act, training in dc.fused_cases():
    k = dc.key(shape, K, S, act, training)
    ref, run = dc.fused_case(shape, K, S, act, training)
    out = run()
    torch.cuda.synchronize()
    rec[k] = {}
    keep(k, "y", out["y"], shape)
    names = ["dconv_weight", "dbn_weight", "dbn_bias"]
    if training:
        names.append("dz")
    else:
        keep(k, "dz", out["dz"], shape)
    rec[k]["err"] = {n: rel_err(out[n], ref[n]) for n in names}
    assert all(rel_err(out[n], ref[n]) < 1e-3 for n in ref), k

with open(os.path.join(HERE, "g8_dwconv_strips.json"), "w") as f:
    json.dump(rec, f, indent=0, sort_keys=True)
path = os.path.join(HERE, "g8_dwconv_strips.npz")
np.savez_compressed(path, **full)
print(f"{len(rec)} cases; json {os.path.getsize(os.path.join(HERE, 'g8_dwconv_strips.json'))} B, npz {os.path.getsize(path)} B")
assert os.path.getsize(path) < 2 ** 20
