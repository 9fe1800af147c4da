#!/usr/bin/env python3
"""Generate the augmentation fixtures tests/golden/g10_augment.npz and g10_augment_continuous.npz (described where it is made,
below) by running the REFERENCE's transform classes.

Run where a checkout of the reference exists (it never travels to the GPU box); CABINET_REFERENCE names it, the default is a
directory `reference` beside this repository:

    PYTHONDONTWRITEBYTECODE=1 [CABINET_REFERENCE=/path/to/CABiNet] python tests/golden/make_golden_augment.py

Per case: a random uint8 image and label, a seed k, and what the reference's default Cityscapes train pipeline
(src/datasets/cityscapes.py:114-136, with cutout_size = 8 for the small crops) makes of them after random.seed(k): the final
bytes, the final labels (through the stored id -> trainId table) and the normalised fp32 tensor.  torchvision is not needed: its
ToTensor / Normalize are restated as u8.float().div(255).sub(mean).div(std).  numpy.random.normal is replaced for the run by
stored float32-valued noise (multiples of 1/16, so the file stays small), which makes the noise step exact as well.

The seeds are chosen by a set cover over the parameters cabinet_amd.augment.DeviceAugment.draw predicts for them, and the
generator FAILS unless the chosen set holds every scale, flip on and off, padding in x only / y only / both / none, a blend
factor inside [0, 1] and one above it for each of the three blends, gray, gamma, noise, a cutout touching row 0 and one touching
the last row, both source sizes under one crop size, a flipped sample padded in x, and the 130-wide crop flipped and at scale 0.75.  That the prediction is right is what tests/test_augment.py proves: it
reproduces every case byte for byte from draw(random.Random(k)).

Only data is written: inputs, expected outputs, seeds.  No reference source text.
"""

import os
import random
import sys

import numpy as np
import torch
from PIL import Image

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("CABINET_REFERENCE", os.path.normpath(os.path.join(ROOT, "..", "reference")))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "src", "datasets"))   # transform.py alone: the package's __init__ pulls torchvision in

import transform as T  # noqa: E402

from cabinet_amd.augment import DeviceAugment, resample_taps  # noqa: E402

OUT = os.path.join(HERE, "g10_augment.npz")
SCALES = (0.75, 1.0, 1.25, 1.5, 1.75, 2.0)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CUTOUT = 8
SIGMA = 0.03
# (source H, W), cropsize (tw, th)
GROUPS = [((33, 61), (48, 40)), ((40, 72), (48, 40)), ((33, 61), (64, 64)), ((40, 72), (64, 64)),
          ((33, 61), (45, 37)), ((40, 72), (45, 37)), ((97, 200), (130, 70)),
          # the sources above are all wider than tall, so none of them is ever padded in x alone: an upright one is
          ((72, 40), (48, 40))]
SEEDS = range(400)


def features(size, crop, p):
    tw, th = crop
    f = {f"scale{p.scale}", f"flip{int(p.flip)}", f"pad_x{int(p.w < tw)}_y{int(p.h < th)}"}
    for name, r in (("b", p.brightness), ("c", p.contrast), ("s", p.saturation)):
        f.add(f"{name}_{'in' if np.float32(r) <= 1 else 'above'}")
    f |= {"gray"} if p.gray else set()
    f |= {"gamma"} if p.gamma is not None else set()
    f |= {"noise"} if p.noise else set()
    if p.cutout is not None:
        f |= {"cut_top"} if p.cutout[0] == 0 else set()
        f |= {"cut_bottom"} if p.cutout[0] + CUTOUT == th else set()
    f.add(f"src{size}_crop{crop}")
    # combinations that meet in one table entry or one workgroup: a mirrored walk through a reflected column, and the widest
    # taps (scale 0.75) and a mirrored walk across tile seams
    f |= {"flip1_pad_x"} if p.flip and p.w < tw else set()
    f |= {"seams_scale0.75"} if tw > 64 and p.scale == 0.75 else set()
    f |= {"seams_flip1"} if tw > 64 and p.flip else set()
    return f


WANTED = ({f"scale{s}" for s in SCALES} | {"flip0", "flip1", "pad_x1_y0", "pad_x0_y1", "pad_x1_y1", "pad_x0_y0", "b_in", "b_above",
          "c_in", "c_above", "s_in", "s_above", "gray", "gamma", "noise", "cut_top", "cut_bottom", "flip1_pad_x",
          "seams_scale0.75", "seams_flip1"}
          | {f"src{s}_crop{c}" for s, c in GROUPS})


def choose():
    cands = []
    for size, crop in GROUPS:
        aug = DeviceAugment.cityscapes(cropsize=crop, cutout_size=CUTOUT)
        for k in SEEDS:
            p = aug.draw([size], random.Random(k))[0]
            if aug.supported(size, p):
                cands.append((size, crop, k, features(size, crop, p)))
    left, picked = set(WANTED), []
    while left:
        best = max(cands, key=lambda c: (len(c[3] & left), -c[0][0] * c[1][0]))
        if not best[3] & left:
            raise SystemExit(f"no seed in {SEEDS} gives {sorted(left)}")
        picked.append(best)
        left -= best[3]
    got = set().union(*[c[3] for c in picked])
    assert WANTED <= got, sorted(WANTED - got)
    return picked


def run_reference(image, label, crop, k, noise, lut):
    pipeline = T.Compose([
        T.RandomHorizontalFlip(p=0.5), T.RandomScale(SCALES), T.RandomCrop(size=crop, pad_if_needed=True, ignore_label=255),
        T.RandomColorJitter(brightness=0.5, contrast=0.5, saturation=0.5), T.RandomGrayscale(p=0.2),
        T.RandomGamma(gamma_range=(0.8, 1.2), p=0.3), T.RandomNoise(mode="gaussian", sigma=SIGMA, p=0.3),
        T.RandomCutout(p=0.3, size=CUTOUT)])
    used = []

    def stored_normal(loc, scale, shape):
        assert loc == 0 and tuple(shape) == noise.shape
        used.append(True)
        return noise.astype(np.float64)

    keep = np.random.normal
    np.random.normal = stored_normal
    try:
        random.seed(k)
        res = pipeline(dict(im=Image.fromarray(image), lb=Image.fromarray(label)))
    finally:
        np.random.normal = keep
    u8 = np.array(res["im"])
    lb = lut[np.array(res["lb"], dtype=np.int64)]
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    f32 = torch.from_numpy(u8).permute(2, 0, 1).contiguous().float().div(255).sub(mean).div(std)
    return u8, lb, f32.numpy(), bool(used)


# The second file, g10_augment_continuous.npz: RandomScale(continuous=True) over (0.4, 0.6) in a pipeline that configures only
# some of the steps (no brightness, no saturation, no noise; gamma always).  It holds what the first cannot: the uniform draw of
# the scale and the jitter factors that are skipped, and resize ratios between 2 and the kernels' limit of 2.5, where a tile of
# 16 output rows reads more than 40 source rows.
OUT_CONT = os.path.join(HERE, "g10_augment_continuous.npz")
CONT = dict(scales=(0.4, 0.6), continuous=True, flip_p=0.5, contrast=0.5, grayscale_p=0.5, gamma_range=(0.7, 1.5), gamma_p=1.0,
            cutout_p=0.5, cutout_size=CUTOUT)
# (source H, W), cropsize (tw, th), seeds
CONT_GROUPS = [((200, 97), (36, 70), (15, 31, 9, 16, 0)), ((97, 200), (70, 36), (15, 7))]


def run_reference_continuous(image, label, crop, k):
    pipeline = T.Compose([
        T.RandomHorizontalFlip(p=CONT["flip_p"]), T.RandomScale(CONT["scales"], continuous=True),
        T.RandomCrop(size=crop, pad_if_needed=True, ignore_label=255), T.RandomColorJitter(contrast=CONT["contrast"]),
        T.RandomGrayscale(p=CONT["grayscale_p"]), T.RandomGamma(gamma_range=CONT["gamma_range"], p=CONT["gamma_p"]),
        T.RandomNoise(mode="gaussian", sigma=SIGMA, p=0.0), T.RandomCutout(p=CONT["cutout_p"], size=CUTOUT)])
    random.seed(k)
    res = pipeline(dict(im=Image.fromarray(image), lb=Image.fromarray(label)))
    return np.array(res["im"]), np.array(res["lb"])


def main_continuous():
    gen = np.random.RandomState(20242)
    out = {"cutout_size": np.int64(CUTOUT), "scales": np.asarray(CONT["scales"]), "contrast": np.float64(CONT["contrast"]),
           "grayscale_p": np.float64(CONT["grayscale_p"]), "gamma_range": np.asarray(CONT["gamma_range"]),
           "gamma_p": np.float64(CONT["gamma_p"]), "cutout_p": np.float64(CONT["cutout_p"]), "flip_p": np.float64(CONT["flip_p"])}
    seen, i = set(), 0
    for size, crop, seeds in CONT_GROUPS:
        image, label = gen.randint(0, 256, size=size + (3,)).astype(np.uint8), gen.randint(0, 256, size=size).astype(np.uint8)
        out[f"image_{size[0]}x{size[1]}"], out[f"label_{size[0]}x{size[1]}"] = image, label
        aug = DeviceAugment(crop, **CONT)
        for k in seeds:
            p = aug.draw([size], random.Random(k))[0]
            assert aug.supported(size, p)
            first, n, _ = resample_taps(size[0], p.h)
            rows = np.arange(p.sh, p.sh + crop[1])
            span = max(int((first[r[-1]] + n[r[-1]]) - first[r[0]]) for r in (rows[j:j + 16] for j in range(0, crop[1], 16)))
            ratio = max(size[0] / p.h, size[1] / p.w)
            seen |= {f"flip{int(p.flip)}", "below_half" if p.scale < 0.5 else "above_half", f"gray{int(p.gray)}",
                     f"cutout{int(p.cutout is not None)}"}
            seen |= {"rows_past_40"} if span > 40 else set()
            seen |= {"ratio_2.5"} if ratio == 2.5 else set()
            seen |= {"just_below_half"} if 0.49 <= p.scale < 0.5 else set()
            u8, lb = run_reference_continuous(image, label, crop, k)
            assert u8.shape == (crop[1], crop[0], 3) and lb.shape == (crop[1], crop[0])
            out[f"c{i}_meta"] = np.asarray([size[0], size[1], crop[0], crop[1], k], dtype=np.int64)
            out[f"c{i}_u8"], out[f"c{i}_label"] = u8, lb.astype(np.uint8)
            print(f"continuous case {i}: source {size} crop {crop} seed {k}: scale {p.scale:.4f}, ratio {ratio:.3f}, {span} source rows per tile")
            i += 1
    want = {"flip0", "flip1", "below_half", "above_half", "gray0", "gray1", "cutout0", "cutout1", "rows_past_40", "ratio_2.5",
            "just_below_half"}
    assert want <= seen, sorted(want - seen)
    out["n_cases"] = np.int64(i)
    np.savez_compressed(OUT_CONT, **out)
    print(f"wrote {OUT_CONT}: {os.path.getsize(OUT_CONT)} bytes, {i} cases")
    assert os.path.getsize(OUT_CONT) <= 1 << 20


def main():
    gen = np.random.RandomState(20241)
    lut = np.full(256, 255, dtype=np.int64)
    lut[:34] = gen.randint(0, 19, size=34)
    lut[:7] = 255
    picked = choose()
    out = {"label_map": lut, "mean": np.asarray(MEAN, dtype=np.float32), "std": np.asarray(STD, dtype=np.float32),
           "cutout_size": np.int64(CUTOUT), "noise_sigma": np.float64(SIGMA), "n_cases": np.int64(len(picked))}
    sources = {}
    for size, _ in GROUPS:
        if size not in sources:
            sources[size] = (gen.randint(0, 256, size=size + (3,)).astype(np.uint8), gen.randint(0, 34, size=size).astype(np.uint8))
            out[f"image_{size[0]}x{size[1]}"], out[f"label_{size[0]}x{size[1]}"] = sources[size]
    seen = set()
    for i, (size, crop, k, feats) in enumerate(picked):
        tw, th = crop
        noise = (np.round(gen.normal(0, SIGMA * 255, size=(th, tw, 3)) * 16) / 16).astype(np.float32)
        u8, lb, f32, noisy = run_reference(*sources[size], crop, k, noise, lut)
        assert u8.shape == (th, tw, 3) and lb.shape == (th, tw) and noisy == ("noise" in feats)
        assert lb.min() >= 0 and lb.max() <= 255
        out[f"c{i}_meta"] = np.asarray([size[0], size[1], tw, th, k, int(noisy)], dtype=np.int64)
        out[f"c{i}_u8"], out[f"c{i}_label"], out[f"c{i}_f32"] = u8, lb.astype(np.uint8), f32
        if noisy:
            out[f"c{i}_noise"] = noise
        seen |= feats
        print(f"case {i}: source {size} crop {crop} seed {k}: {sorted(feats)}")
    assert WANTED <= seen
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(picked)} cases")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
    main_continuous()
