#!/usr/bin/env python3
"""Generate tests/golden/g13_aerial.npz by running the REFERENCE's transform classes in the train pipeline its aerial datasets
share (src/datasets/uavid.py:192-230; vdd.py and aeroscapes.py hold the same span).

Run where a checkout of the reference exists (it never travels to the GPU box); CABINET_REFERENCE names it, the default is a
directory `reference` beside this repository:

    PYTHONDONTWRITEBYTECODE=1 [CABINET_REFERENCE=/path/to/CABiNet] python tests/golden/make_golden_aerial.py

Per case: a random uint8 image and label, a seed k, and what the UAVid pipeline with its default augmentation (cutout_size = 8 for
the small crops, the cap of ResizeIfLarger 2 max(cropsize) as the dataset sets it) makes of them after random.seed(k): the final
bytes, the final labels (class ids, no lookup) and the normalised fp32 tensor (ToTensor / Normalize restated as
u8.float().div(255).sub(mean).div(std) with UAVid's constants).  numpy.random.normal is replaced for the run by stored
float32-valued noise (multiples of 1/16), which makes the noise step exact as well.

Every candidate (source, crop, seed) is run through the reference first, with RandomHSV watched for whether its saturation and
value tables clip a byte that is really there; the seeds are then chosen by a set cover over those observations and the
parameters cabinet_amd.augment.DeviceAugment.draw predicts, and the generator FAILS unless the chosen set holds everything in
WANTED below.  That the prediction is right is what tests/test_aerial_augment.py proves: it reproduces every case byte for byte
from draw(random.Random(k)).

Only data is written: inputs, expected outputs, seeds, the Pillow version.  No reference source text.
"""

import io
import os
import random
import sys
import zipfile

import numpy as np
import PIL
import torch
from PIL import Image

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("CABINET_REFERENCE", os.path.normpath(os.path.join(ROOT, "..", "reference")))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "src", "datasets"))   # transform.py alone: the package's __init__ pulls torchvision in

import transform as T  # noqa: E402

from cabinet_amd.augment import DeviceAugment  # noqa: E402

OUT = os.path.join(HERE, "g13_aerial.npz")
MEAN, STD = (0.480, 0.499, 0.457), (0.225, 0.208, 0.228)   # UAVid's
AUG = DeviceAugment.AERIAL_DEFAULTS
CUTOUT = 8
SIGMA = 0.03
IGNORE = 255
SOURCES = [(33, 61), (72, 40), (97, 200), (200, 97)]      # (H, W)
CROPS = [(48, 40), (64, 64), (130, 70)]                   # cropsize (tw, th)
SEEDS = range(200)


class WatchedHSV(T.RandomHSV):
    """The reference's step, unchanged; notes the largest S and V byte of the crop it is given."""
    seen = None

    def __call__(self, im_lb):
        hsv = np.array(im_lb["im"].convert("HSV"))
        WatchedHSV.seen = (int(hsv[..., 1].max()), int(hsv[..., 2].max()))
        return super().__call__(im_lb)


def pipeline(crop):
    d, s = float(AUG["degrees"]), float(AUG["scale"])
    return T.Compose([
        T.ResizeIfLarger(max_size=2 * max(crop)), T.RandomHorizontalFlip(p=float(AUG["fliplr"])),
        T.RandomVerticalFlip(p=float(AUG["flipud"])), T.RandomTranslate(translate=float(AUG["translate"]), ignore_label=IGNORE),
        T.RandomRotate(degrees=(-d, d), ignore_label=IGNORE), T.RandomScale((1.0 - s, 1.0 + s), continuous=True),
        T.RandomCrop(size=crop, pad_if_needed=True, ignore_label=IGNORE),
        WatchedHSV(hgain=float(AUG["hsv_h"]), sgain=float(AUG["hsv_s"]), vgain=float(AUG["hsv_v"])),
        T.RandomColorJitter(contrast=0.5), T.RandomGamma(gamma_range=(0.8, 1.2), p=0.3),
        T.RandomNoise(mode="gaussian", sigma=SIGMA, p=0.3), T.RandomCutout(p=0.3, size=CUTOUT)])


def run_reference(image, label, crop, k, noise):
    used = []

    def stored_normal(loc, scale, shape):
        assert loc == 0 and tuple(shape) == noise.shape
        used.append(True)
        return noise.astype(np.float64)

    keep = np.random.normal
    np.random.normal = stored_normal
    try:
        random.seed(k)
        res = pipeline(crop)(dict(im=Image.fromarray(image), lb=Image.fromarray(label)))
    finally:
        np.random.normal = keep
    u8 = np.array(res["im"])
    lb = np.array(res["lb"], dtype=np.int64)
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    f32 = torch.from_numpy(u8).permute(2, 0, 1).contiguous().float().div(255).sub(mean).div(std)
    return u8, lb, f32.numpy(), bool(used)


def augmenter(crop):
    return DeviceAugment.uavid(cropsize=crop, cutout_size=CUTOUT)


def features(size, crop, p, s_max, v_max):
    tw, th = crop
    f = {f"hflip{int(p.flip)}", f"vflip{int(p.vflip)}", "dx_neg" if p.dx < 0 else "dx_pos", "dy_neg" if p.dy < 0 else "dy_pos",
         "rot_neg" if p.angle < 0 else "rot_pos", "scale_below" if p.scale < 1 else "scale_above",
         f"pad_x{int(p.w < tw)}_y{int(p.h < th)}"}
    f |= {"both_flips"} if p.flip and p.vflip else set()
    shift = round(p.hsv[0] * 255)
    f.add("hue_neg" if shift < 0 else ("hue_pos" if shift > 0 else "hue_zero"))
    f.add("sat_below" if p.hsv[1] < 0 else "sat_above")
    f.add("val_below" if p.hsv[2] < 0 else "val_above")
    f |= {"sat_clips"} if s_max * (p.hsv[1] + 1) > 255 else set()
    f |= {"val_clips"} if v_max * (p.hsv[2] + 1) > 255 else set()
    f |= {"gamma"} if p.gamma is not None else set()
    f |= {"noise"} if p.noise else set()
    if p.cutout is not None:
        f |= {"cut_top"} if p.cutout[0] == 0 else set()
        f |= {"cut_bottom"} if p.cutout[0] + CUTOUT == th else set()
    f.add(f"resized{int(p.resized is not None)}_crop{crop}")
    f |= {"seams_rotated"} if tw > 64 and p.angle % 360.0 != 0 else set()
    return f


WANTED = {"hflip0", "hflip1", "vflip0", "vflip1", "both_flips", "dx_neg", "dx_pos", "dy_neg", "dy_pos", "rot_neg", "rot_pos",
          "scale_below", "scale_above", "pad_x0_y0", "pad_x1_y0", "pad_x0_y1", "pad_x1_y1", "hue_neg", "hue_zero", "hue_pos",
          "sat_below", "sat_above", "sat_clips", "val_below", "val_above", "val_clips", "gamma", "noise", "cut_top", "cut_bottom",
          "resized1_crop(48, 40)", "resized0_crop(48, 40)", "seams_rotated"}


def choose(sources):
    cands = []
    for crop in CROPS:
        aug = augmenter(crop)
        tw, th = crop
        zero = np.zeros((th, tw, 3), dtype=np.float32)
        for size in SOURCES:
            for k in SEEDS:
                p = aug.draw([size], random.Random(k))[0]
                if not aug.supported(size, p):
                    continue
                run_reference(*sources[size], crop, k, zero)
                cands.append((size, crop, k, features(size, crop, p, *WatchedHSV.seen)))
    left, picked = set(WANTED), []
    while left:
        best = max(cands, key=lambda c: (len(c[3] & left), -c[1][0] * c[1][1], -c[0][0] * c[0][1], -c[2]))
        if not best[3] & left:
            raise SystemExit(f"no seed in {SEEDS} gives {sorted(left)}")
        picked.append(best)
        left -= best[3]
    got = set().union(*[c[3] for c in picked])
    assert WANTED <= got, sorted(WANTED - got)
    return picked


def save_npz(path, arrays):
    """numpy's .npz layout with fixed member timestamps, so that a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, arr in arrays.items():
            raw = io.BytesIO()
            np.lib.format.write_array(raw, np.asanyarray(arr), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), raw.getvalue(), zipfile.ZIP_DEFLATED, 9)


def main():
    gen = np.random.RandomState(20243)
    sources = {size: (gen.randint(0, 256, size=size + (3,)).astype(np.uint8), gen.randint(0, 19, size=size).astype(np.uint8))
               for size in SOURCES}
    picked = choose(sources)
    out = {"mean": np.asarray(MEAN, dtype=np.float32), "std": np.asarray(STD, dtype=np.float32), "cutout_size": np.int64(CUTOUT),
           "noise_sigma": np.float64(SIGMA), "n_cases": np.int64(len(picked)), "pillow_version": np.asarray(PIL.__version__)}
    for size in sorted({c[0] for c in picked}):
        out[f"image_{size[0]}x{size[1]}"], out[f"label_{size[0]}x{size[1]}"] = sources[size]
    seen = set()
    for i, (size, crop, k, feats) in enumerate(picked):
        tw, th = crop
        noise = (np.round(gen.normal(0, SIGMA * 255, size=(th, tw, 3)) * 16) / 16).astype(np.float32)
        u8, lb, f32, noisy = run_reference(*sources[size], crop, k, noise)
        assert u8.shape == (th, tw, 3) and lb.shape == (th, tw) and noisy == ("noise" in feats)
        assert lb.min() >= 0 and lb.max() <= 255
        out[f"c{i}_meta"] = np.asarray([size[0], size[1], tw, th, k, int(noisy)], dtype=np.int64)
        out[f"c{i}_u8"], out[f"c{i}_label"], out[f"c{i}_f32"] = u8, lb.astype(np.uint8), f32
        if noisy:
            out[f"c{i}_noise"] = noise
        seen |= feats
        print(f"case {i}: source {size} crop {crop} seed {k}: {sorted(feats)}")
    assert WANTED <= seen
    save_npz(OUT, out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(picked)} cases, Pillow {PIL.__version__}")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
