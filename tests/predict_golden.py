"""Loader of the inference fixture tests/golden/g7_predict.npz (written by tests/golden/make_golden_predict.py), and the render
contract in numpy.  Shared by tests/test_predict.py and tests/test_gpu_predict.py.

Per case k = 1..5 the file holds the image as uint8 (image = (u8 - 128) / 64, exact in fp32), the stub's weights, the reference's
fp32 predictions as uint8, ref32_vs_f64_maxabs, the bit-packed mask of the undecided pixels (float64 top-two margin below
TIE_FACTOR x ref32_vs_f64_maxabs) and their share; and one render block (see ``load_render``).
"""
import os

import numpy as np
import torch

from eval_golden import GOLDEN, MAX_UNDECIDED_SHARE, StubNet, image_from_u8

CASES = (1, 2, 3, 4, 5)
_cache = {}


def _file():
    if "z" not in _cache:
        with np.load(os.path.join(GOLDEN, "g7_predict.npz")) as z:
            _cache["z"] = {n: z[n] for n in z.files}
    return _cache["z"]


def load_case(k):
    """One case, loaded once and shared (treat as read-only; the model is fresh on every call)."""
    z = _file()
    g = {n[len(f"c{k}_"):]: z[n] for n in z if n.startswith(f"c{k}_")}
    C = int(g["n_classes"])
    H, W = g["image_u8"].shape[2:]
    net = StubNet(C)
    with torch.no_grad():
        net.conv.weight.copy_(torch.from_numpy(g["weight"]))
        net.conv.bias.copy_(torch.from_numpy(g["bias"]))
    undecided = np.unpackbits(g["undecided_bits"])[:H * W].reshape(H, W).astype(bool)
    share = float(g["undecided_share"])
    assert abs(float(undecided.mean()) - share) < 1e-12 and share <= MAX_UNDECIDED_SHARE
    return {"n_classes": C, "scales": tuple(float(s) for s in g["scales"]), "flip": bool(g["flip"]),
            "image": image_from_u8(g["image_u8"]), "model": net.eval(), "pred": g["pred"].astype(np.int64),
            "ref32_vs_f64_maxabs": float(g["ref32_vs_f64_maxabs"]), "undecided": undecided, "undecided_share": share}


def load_render():
    """image (3, H, W) normalised fp32, labels (H, W) uint8 (with values >= 19 and 255), mean / std fp32 (3,), alpha, and the
    reference's three (H, W, 3) uint8 arrays: input, pred, overlay."""
    z = _file()
    return {n[len("render_"):]: z[n] for n in z if n.startswith("render_")}


def render_contract(labels, image, palette, mean, std, alpha):
    """numpy statement of cabinet_predict_render: fp32 throughout, every product and sum rounded on its own, truncation toward
    zero.  labels (..., H, W) integer, image (..., 3, H, W) or None, palette (n_colors, 3) uint8."""
    palette = np.asarray(palette, dtype=np.uint8)
    pred = palette[np.minimum(np.asarray(labels).astype(np.int64), len(palette) - 1)]
    if image is None:
        return {"pred": pred}
    x = np.moveaxis(np.asarray(image, dtype=np.float32), -3, -1)
    v = x * np.asarray(std, dtype=np.float32) + np.asarray(mean, dtype=np.float32)
    inp = (np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    diff = (pred.astype(np.int32) - inp.astype(np.int32)).astype(np.float32)
    overlay = (inp.astype(np.float32) + np.float32(alpha) * diff).astype(np.uint8)
    assert v.dtype == np.float32 and overlay.dtype == np.uint8
    return {"pred": pred, "input": inp, "overlay": overlay}
