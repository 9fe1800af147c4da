"""Shared by tests/test_aerial_augment.py and tests/test_gpu_aerial_augment.py: the cases of tests/golden/g13_aerial.npz (the
reference's own output for the aerial datasets' train pipeline, tests/golden/make_golden_aerial.py) and the augmenter that goes
with them."""
import os
import random

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_aerial.npz")

_cache = {}


def fixture():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def pillow_version():
    return str(fixture()["pillow_version"])


class Case(object):
    def __init__(self, i):
        g = fixture()
        H, W, tw, th, seed, noisy = [int(v) for v in g[f"c{i}_meta"]]
        self.index, self.size, self.crop, self.seed = i, (H, W), (tw, th), seed
        self.image, self.label = g[f"image_{H}x{W}"], g[f"label_{H}x{W}"]
        self.noise = g[f"c{i}_noise"] if noisy else None
        self.u8, self.lb, self.f32 = g[f"c{i}_u8"], g[f"c{i}_label"].astype(np.int64), g[f"c{i}_f32"]


def cases():
    return [Case(i) for i in range(int(fixture()["n_cases"]))]


def crops():
    return sorted({c.crop for c in cases()})


def augmenter(crop):
    from cabinet_amd.augment import DeviceAugment

    g = fixture()
    return DeviceAugment.uavid(cropsize=crop, cutout_size=int(g["cutout_size"]), mean=[float(v) for v in g["mean"]],
                               std=[float(v) for v in g["std"]])


def batch(crop, device="cpu"):
    """Every case of one crop size as one batch (sources of different sizes, resized and not): augmenter, cases, images, labels,
    the parameters drawn as the reference draws them -- random.Random(seed) per case -- and the noise."""
    aug = augmenter(crop)
    cs = [c for c in cases() if c.crop == crop]
    params = [aug.draw([c.size], random.Random(c.seed))[0] for c in cs]
    images = [torch.from_numpy(c.image).to(device) for c in cs]
    labels = [torch.from_numpy(c.label).to(device) for c in cs]
    tw, th = crop
    noise = np.zeros((len(cs), th, tw, 3), dtype=np.float32)
    for j, c in enumerate(cs):
        if c.noise is not None:
            noise[j] = c.noise
    return aug, cs, images, labels, params, torch.from_numpy(noise).to(device)
