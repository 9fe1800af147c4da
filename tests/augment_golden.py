"""Shared by tests/test_augment.py and tests/test_gpu_augment.py: the cases of tests/golden/g10_augment.npz (the reference's own
output, tests/golden/make_golden_augment.py) and the augmenter that goes with them."""
import os
import random

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_augment.npz")
GOLDEN_CONT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_augment_continuous.npz")

_cache = {}


def fixture():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def n_cases():
    return int(fixture()["n_cases"])


class Case(object):
    def __init__(self, i):
        g = fixture()
        H, W, tw, th, seed, noisy = [int(v) for v in g[f"c{i}_meta"]]
        self.index, self.size, self.crop, self.seed = i, (H, W), (tw, th), seed
        self.image, self.label = g[f"image_{H}x{W}"], g[f"label_{H}x{W}"]
        self.noise = g[f"c{i}_noise"] if noisy else None
        self.u8, self.lb, self.f32 = g[f"c{i}_u8"], g[f"c{i}_label"].astype(np.int64), g[f"c{i}_f32"]


def cases():
    return [Case(i) for i in range(n_cases())]


def crops():
    return sorted({c.crop for c in cases()})


def augmenter(crop):
    from cabinet_amd.augment import DeviceAugment

    g = fixture()
    return DeviceAugment.cityscapes(cropsize=crop, ignore_label=255, label_map=g["label_map"], cutout_size=int(g["cutout_size"]),
                                    mean=[float(v) for v in g["mean"]], std=[float(v) for v in g["std"]])


def batch(crop, device="cpu"):
    """Every case of one crop size as one batch (the sources differ in size): augmenter, cases, images, labels, the parameters
    drawn as the reference draws them -- random.Random(seed) per case, since the fixture seeds per sample -- and the noise."""
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


def continuous_fixture():
    if "c" not in _cache:
        with np.load(GOLDEN_CONT) as z:
            _cache["c"] = {k: z[k] for k in z.files}
    return _cache["c"]


class ContinuousCase(object):
    """A case of g10_augment_continuous.npz: RandomScale(continuous=True) over (0.4, 0.6) in a partly configured pipeline."""

    def __init__(self, i):
        g = continuous_fixture()
        H, W, tw, th, seed = [int(v) for v in g[f"c{i}_meta"]]
        self.index, self.size, self.crop, self.seed = i, (H, W), (tw, th), seed
        self.image, self.label = g[f"image_{H}x{W}"], g[f"label_{H}x{W}"]
        self.u8, self.lb = g[f"c{i}_u8"], g[f"c{i}_label"].astype(np.int64)


def continuous_cases():
    return [ContinuousCase(i) for i in range(int(continuous_fixture()["n_cases"]))]


def continuous_augmenter(crop):
    from cabinet_amd.augment import DeviceAugment

    g = continuous_fixture()
    return DeviceAugment(crop, scales=tuple(float(v) for v in g["scales"]), continuous=True, flip_p=float(g["flip_p"]),
                         contrast=float(g["contrast"]), grayscale_p=float(g["grayscale_p"]),
                         gamma_range=tuple(float(v) for v in g["gamma_range"]), gamma_p=float(g["gamma_p"]),
                         cutout_p=float(g["cutout_p"]), cutout_size=int(g["cutout_size"]))


def continuous_batch(crop, device="cpu"):
    aug = continuous_augmenter(crop)
    cs = [c for c in continuous_cases() if c.crop == crop]
    params = [aug.draw([c.size], random.Random(c.seed))[0] for c in cs]
    return (aug, cs, [torch.from_numpy(c.image).to(device) for c in cs], [torch.from_numpy(c.label).to(device) for c in cs], params)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in numpy: counter (..., 4) and key (..., 2) uint32 -> (..., 4) uint32."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[..., 0], dtype=np.uint64), np.asarray(key[..., 1], dtype=np.uint64)
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & lo]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & lo, (k1 + np.uint64(0xBB67AE85)) & lo
    return np.stack(c, axis=-1).astype(np.uint32)


def ulp_distance(a, b):
    """Largest distance in units of the last place between two fp32 arrays of equal sign pattern (bit patterns as integers)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max())
