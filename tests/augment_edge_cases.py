"""Shapes, launch rules, seeded inputs and oracle helpers of the device-side augmentation -- K18 csrc/augment.hip, K20
csrc/augment_warp.hip and the shared csrc/augment_taps.hpp -- shared by the tests of tests/test_gpu_augment_edges.py.

The plan functions restate the host rules of the launchers (the function each restates is named in its docstring) so that the
tables below can say which branch a shape reaches; test_augment_plan_cases_reach_their_branches keeps the tables and, through the
library's queries and the constants read back from the sources, the restatement honest.  The oracle of every GPU test is the
project's numpy route (DeviceAugment on host tensors, affine_image / affine_label, _host_warp, _apply_taps); the pillow_*
helpers compose the same operations from Pillow's own calls, and test_edge_oracle_against_pillow holds the numpy route against
them at the shapes of these tables.  Everything here runs on the CPU."""
import dataclasses
import os
import random
import re

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the kernels' constants, restated; source_constants() reads the originals back
AUG_TX, AUG_TY, AUG_RS, AUG_TAPS = 64, 16, 48, 5
WARP_TX, WARP_TY = 32, 8
PHOTO_THREADS, PHOTO_PX = 256, 4       # augment_photo_kernel: lanes of a workgroup (and of its prologue's stride), pixels of a lane
RESTATED = dict(AUG_TX=AUG_TX, AUG_TY=AUG_TY, AUG_RS=AUG_RS, AUG_TAPS=AUG_TAPS, WARP_TX=WARP_TX, WARP_TY=WARP_TY)
LABEL_MAP = (np.arange(256) * 7) % 19
FILL = 255


def source_constants():
    """The same constants as csrc/augment_taps.hpp and csrc/augment_warp.hip spell them."""
    def text(name):
        with open(os.path.join(ROOT, "cabinet_amd", "csrc", name)) as f:
            return f.read()

    def define(src, name):
        m = re.search(r"#define %s\s+(\d+)" % name, src)
        assert m is not None, name
        return int(m.group(1))

    taps, warp, k18 = text("augment_taps.hpp"), text("augment_warp.hip"), text("augment.hip")
    assert re.search(r"for \(int i = t; i < tiles; i \+= %d\)" % PHOTO_THREADS, k18)          # the prologue's stride
    assert re.search(r"\(\(size_t\)blockIdx\.x \* %d \+ t\) \* %d;" % (PHOTO_THREADS, PHOTO_PX), k18)   # p0 of a lane
    out = {k: define(taps, k) for k in ("AUG_TX", "AUG_TY", "AUG_RS", "AUG_TAPS")}
    out.update({k: define(warp, k) for k in ("WARP_TX", "WARP_TY")})
    return out


# ------------------------------------------------------------------------------------------------ the host rules, restated
def _cdiv(a, b):
    return -(-a // b)


def _align(v, a):
    return _cdiv(v, a) * a


def tiles(th, tw):
    """augment_tiles: workgroups of augment_geom_kernel per sample, one 64-bit partial each."""
    return _cdiv(th, AUG_TY) * _cdiv(tw, AUG_TX)


def geom_grid(th, tw):
    """augment_run: (x, y) of augment_geom_kernel's grid."""
    return _cdiv(tw, AUG_TX), _cdiv(th, AUG_TY)


def crop_stride(th, tw):
    """augment_crop_stride: bytes between the uint8 crops of two samples in the workspace."""
    return _align(th * tw * 3, 16)


def workspace_bytes(N, th, tw):
    """augment_workspace."""
    return _align(N * crop_stride(th, tw), 256) + N * tiles(th, tw) * 8


def tiles_from_workspace(N, th, tw, nbytes):
    """The tile count cabinet_augment_workspace_bytes' answer holds."""
    rest = nbytes - _align(N * crop_stride(th, tw), 256)
    assert rest % (8 * N) == 0
    return rest // (8 * N)


def photo_grid(th, tw, N):
    """augment_run: grid of augment_photo_kernel, four pixels per lane."""
    return _cdiv(_cdiv(th * tw, PHOTO_PX), PHOTO_THREADS), N


def group_counts(P):
    """The `cnt` values the lanes of augment_photo_kernel see at P pixels: 4 for full groups, P % 4 for a last ragged one."""
    return ({4} if P >= 4 else set()) | ({P % 4} if P % 4 else set())


def store_pairings(P, N, f32_off=0, u8_off=0):
    """{(f32x4 store?, packed out_u8 store?)} over the full groups of every (sample, channel), for out_image `f32_off` elements
    and out_u8 `u8_off` bytes past a 16-byte aligned address: p0 % 4 == 0, so `(dst & 15) == 0` is ((f32_off + (3 n + ch) P) % 4
    == 0) and `(d & 3) == 0` is ((u8_off + 3 n P) % 4 == 0).  A ragged last group stores element by element either way."""
    if P < 4:
        return set()
    return {((f32_off + (3 * n + ch) * P) % 4 == 0, (u8_off + 3 * n * P) % 4 == 0) for n in range(N) for ch in range(3)}


def tile_spans(rt, th, H):
    """tap_rows_span per tile of AUG_TY output rows, from the row taps `rt` of _sample_tables (step = 1 on rows)."""
    first = np.clip(rt["first"], 0, H - 1)
    last = np.clip(first + np.maximum(np.clip(rt["n"], 0, AUG_TAPS), 1) - 1, 0, H - 1)
    return [int(last[y:y + AUG_TY].max() - first[y:y + AUG_TY].min() + 1) for y in range(0, th, AUG_TY)]


def k18_supported(th, tw, taps, pad_y, pad_x, min_h, min_w):
    """cabinet_augment_supported."""
    return bool(1 <= th <= 32768 and 1 <= tw <= 32768 and 1 <= taps <= AUG_TAPS and min_h >= 1 and min_w >= 1
                and 0 <= pad_y <= min_h - 1 and 0 <= pad_x <= min_w - 1)


def warp_supported(H, W, oh, ow, angle, ratio):
    """cabinet_augment_warp_supported for |angle| < 180."""
    return bool(all(1 <= v <= 32768 for v in (H, W, oh, ow)) and abs(angle) <= 45.0 and 0.0 <= ratio <= 2.5)


def warp_outside(items, tx, ty):
    """Workgroups of one launch over `items` that leave at `x0 >= ow || y0 >= oh`: the grid covers the largest output."""
    gx, gy = _cdiv(max(it["out_w"] for it in items), tx), _cdiv(max(it["out_h"] for it in items), ty)
    own = sum(_cdiv(it["out_w"], tx) * _cdiv(it["out_h"], ty) for it in items)
    return gx * gy * len(items) - own, gx * gy * len(items)


# ------------------------------------------------------------------------------------------------ seeded inputs
def source(size, seed=0):
    """uint8 image (H, W, 3) and label (H, W) with ids below 34 of one (H, W)."""
    gen = np.random.RandomState(size[0] * 1000 + size[1] + 7919 * seed)
    return gen.randint(0, 256, size=tuple(size) + (3,)).astype(np.uint8), gen.randint(0, 34, size=tuple(size)).astype(np.uint8)


def noise_for(N, th, tw, seed):
    gen = np.random.RandomState(seed)
    return (gen.standard_normal((N, th, tw, 3)) * (0.03 * 255)).astype(np.float32)


def ramp(n):
    """A gray ramp of n pixels, dark (0) to bright (255), whose offset is searched so that the rounded mean (int)(sum / n + 0.5)
    drops by one when the last pixel's luma is left out of the sum."""
    x = np.arange(n, dtype=np.int64)
    for off in range(n - 1):
        v = (x * 255 + off) // (n - 1)
        s = int(v.sum())
        if v[-1] == 255 and int(s / n + 0.5) != int((s - 255) / n + 0.5):
            return v.astype(np.uint8)
    raise AssertionError(n)


# ------------------------------------------------------------------------------------------------ K18: tables
NEUTRAL = dict(flip=False, brightness=1.0, contrast=1.0, saturation=1.0, gray=False, gamma=None, noise=False, cutout=None)
TINY_CROPS = [(1, 1), (2, 1), (3, 1), (1, 2), (5, 1), (3, 3), (2, 17), (6, 7), (7, 9)]      # (tw, th)
_RICH = dict(brightness=0.9, contrast=0.7, saturation=1.2, gamma=0.9, noise=True)
_J = [0.0, 1.0, 0.5, 1.5]


def _tiny(crop):
    tw, th = crop
    return dict(crop=crop, branch="cnt", samples=[dict(size=(th + 3, tw + 4), sw=2, sh=1, **_RICH), dict(size=(th + 1, tw + 2), sw=1, sh=0, flip=True, **_RICH)])


# name -> dict(crop=(tw, th), branch, samples=[dict(size=(H, W), scale, sw, sh, overrides of NEUTRAL ...)], aug=constructor
# keywords, src="random" | "vramp" | "hramp").  `branch` is what test_augment_plan_cases_reach_their_branches asserts of the row.
K18_CASES = {
    # tiles > 256: the second trip of the photo prologue's loop.  The 257th tile of these two crops is ONE pixel, so leaving it
    # out moves the mean by at most 255 / P < 1; ramp() places the sum where that still changes the rounded mean
    "tall-257-tiles": dict(crop=(1, 4097), branch="tiles>256", src="vramp", samples=[dict(size=(4097, 1), contrast=0.6)]),
    "wide-257-tiles": dict(crop=(16385, 1), branch="tiles>256", src="hramp", samples=[dict(size=(1, 16385), contrast=0.6)]),
    # 512 tiles: the first 256 are the dark half, their mean luma is far (>= 2) from the whole crop's
    "tall-512-tiles": dict(crop=(1, 8177), branch="tiles>256 by 2", src="vramp", samples=[dict(size=(8177, 1), contrast=0.6)]),
    "wide-512-tiles": dict(crop=(32705, 1), branch="tiles>256 by 2", src="hramp", samples=[dict(size=(1, 32705), contrast=0.6)]),
    "grid-3x5-N3": dict(crop=(130, 70), branch="grid", samples=[dict(size=(80, 140), sw=7, sh=9, contrast=0.6), dict(size=(72, 150), sw=20, sh=2, contrast=1.3),
                                                                 dict(size=(90, 131), sw=1, sh=20, contrast=0.85)]),
    **{"tiny-%dx%d" % c: _tiny(c) for c in TINY_CROPS},
    # ratio exactly 2.5 (120 -> 48 rows: 40 source rows per tile of 16; 320 -> 128 columns: 160 per tile of 64) at three offsets
    "ratio-2.5-phase-0": dict(crop=(64, 16), branch="span>=40", aug=dict(scales=(0.4,)), samples=[dict(size=(120, 320), scale=0.4, sw=0, sh=0, contrast=0.8)]),
    "ratio-2.5-phase-mid": dict(crop=(64, 16), branch="span>=40", aug=dict(scales=(0.4,)), samples=[dict(size=(120, 320), scale=0.4, sw=31, sh=15, contrast=0.8)]),
    "ratio-2.5-phase-last": dict(crop=(64, 16), branch="span>=40", aug=dict(scales=(0.4,)), samples=[dict(size=(120, 320), scale=0.4, sw=64, sh=32, contrast=0.8)]),
    "upscale-2-reversed": dict(crop=(67, 33), branch="step=-1", aug=dict(scales=(2.0,)), samples=[dict(size=(20, 37), scale=2.0, sw=5, sh=3, flip=True, saturation=0.5),
                                                                                                  dict(size=(19, 40), scale=2.0, sw=0, sh=5, flip=True)]),
    "reflect-maximal": dict(crop=(21, 17), branch="maxpad", samples=[dict(size=(9, 11), contrast=0.7), dict(size=(9, 11), flip=True)]),
    "source-h1": dict(crop=(5, 1), branch="H=1", aug=dict(scales=(1.0, 2.0)), samples=[dict(size=(1, 9), sw=2), dict(size=(1, 4), scale=2.0, sw=1, sh=1, flip=True)]),
    "source-w1": dict(crop=(1, 5), branch="W=1", aug=dict(scales=(1.0, 2.0)), samples=[dict(size=(9, 1), sh=3), dict(size=(4, 1), scale=2.0, sw=1, sh=2, flip=True)]),
    "flags-all-16": dict(crop=(45, 37), branch="flags", aug=dict(cutout_size=8), samples=[
        dict(size=((40, 72), (33, 61))[k & 1], sw=k & 1, sh=0, contrast=0.8, gray=bool(k & 1), gamma=1.15 if k & 2 else None, noise=bool(k & 4),
             cutout=(3 + k, 30 - k) if k & 8 else None) for k in range(16)]),
    "cutout-corners": dict(crop=(45, 37), branch="cutout", aug=dict(cutout_size=8), samples=[dict(size=(40, 72), sw=3, sh=1, cutout=c)
                                                                                            for c in ((0, 0), (0, 37), (29, 0), (29, 37))]),
    "cutout-size-1": dict(crop=(45, 37), branch="cutout", aug=dict(cutout_size=1), samples=[dict(size=(40, 72), sw=3, sh=1, cutout=c)
                                                                                           for c in ((0, 0), (36, 44), (17, 20), (0, 44))]),
    "cutout-whole-crop": dict(crop=(24, 24), branch="cutout", aug=dict(cutout_size=24), samples=[dict(size=(40, 72), sw=3, sh=1, cutout=(0, 0)),
                                                                                                 dict(size=(33, 61), sw=0, sh=2)]),
    "jitter-0-1-0.5-1.5": dict(crop=(45, 37), branch="jitter", samples=[
        dict(size=(40, 72), sw=k, sh=1, **{**dict(brightness=0.8, contrast=1.2, saturation=0.8), which: v})
        for k, (which, v) in enumerate((w, v) for w in ("brightness", "contrast", "saturation") for v in _J)]),
    "hsv-mixed-batch": dict(crop=(45, 37), branch="hsv", aug=dict(hsv=(0.01, 0.4, 0.3)), samples=[
        dict(size=(40, 72), sw=2, sh=1, contrast=0.6, hsv=(0.004, 0.2, -0.3)), dict(size=(33, 61), contrast=0.6, hsv=None),
        dict(size=(40, 72), sw=5, sh=0, contrast=0.6, hsv=(-0.009, -0.31, 0.25)), dict(size=(33, 61), sw=1, contrast=1.4, hsv=None)]),
}


@dataclasses.dataclass
class Batch:
    aug: object
    images: list      # numpy uint8 (H, W, 3)
    labels: list      # numpy uint8 (H, W)
    sizes: list
    params: list
    noise: object     # numpy fp32 (N, th, tw, 3) or None

    def tensors(self, dev="cpu"):
        return [torch.from_numpy(a).to(dev) for a in self.images], [torch.from_numpy(a).to(dev) for a in self.labels]

    def noise_tensor(self, dev="cpu"):
        return None if self.noise is None else torch.from_numpy(self.noise).to(dev)

    def host(self, params=None, noise="own"):
        """(fp32 (N, 3, th, tw), labels (N, th, tw), bytes (N, th, tw, 3)) of the numpy route, as numpy arrays."""
        im, lb = self.tensors()
        nz = self.noise_tensor() if isinstance(noise, str) else noise
        return tuple(t.numpy() for t in self.aug(im, lb, params=self.params if params is None else params, noise=nz, return_uint8=True))


def k18_aug(crop, **kw):
    from cabinet_amd.augment import DeviceAugment

    base = dict(scales=(1.0,), flip_p=0.5, brightness=0.5, contrast=0.5, saturation=0.5, grayscale_p=0.2, gamma_p=0.3, noise_p=0.3,
                cutout_p=0.3, cutout_size=1, label_map=LABEL_MAP)
    base.update(kw)
    return DeviceAugment(crop, **base)


_cases = {}


def k18_case(name):
    """The Batch of one row of K18_CASES: params from draw(), then dataclasses.replace with the row's values."""
    if name in _cases:
        return _cases[name]
    row = K18_CASES[name]
    tw, th = row["crop"]
    aug = k18_aug(row["crop"], **row.get("aug", {}))
    sizes = [s["size"] for s in row["samples"]]
    drawn = aug.draw(sizes, random.Random(len(name) + tw + th))
    params, images, labels = [], [], []
    for k, (p, (H, W), s) in enumerate(zip(drawn, sizes, row["samples"])):
        scale = s.get("scale", 1.0)
        over = dict(NEUTRAL, scale=scale, w=int(round(W * scale)), h=int(round(H * scale)), sw=s.get("sw", 0), sh=s.get("sh", 0), hsv=None)
        over.update({f: v for f, v in s.items() if f not in ("size", "scale", "sw", "sh")})
        params.append(dataclasses.replace(p, **over))
        image, label = source((H, W), k)
        if row.get("src") in ("vramp", "hramp"):
            image = np.repeat(ramp(H * W).reshape(H, W, 1), 3, axis=2)
        images.append(image), labels.append(label)
    noise = noise_for(len(sizes), th, tw, tw * 100 + th) if any(p.noise for p in params) else None
    _cases[name] = Batch(aug, images, labels, sizes, params, noise)
    return _cases[name]


def k18_plan(b):
    """What the launch of one Batch reaches, by the restated rules and the tables of _sample_tables."""
    aug = b.aug
    P = aug.th * aug.tw
    spans, steps = [], set()
    for size, p in zip(b.sizes, b.params):
        ct, rt, lc, lr = aug._sample_tables(size, p)
        spans += tile_spans(rt, aug.th, size[0])
        steps |= set(int(v) for v in ct["step"])
    return dict(tiles=tiles(aug.th, aug.tw), grid=geom_grid(aug.th, aug.tw), photo=photo_grid(aug.th, aug.tw, len(b.sizes)), P=P, cnt=group_counts(P),
                pairings=store_pairings(P, len(b.sizes)), span=max(spans), steps=steps,
                pad=[(max(aug.tw - p.w, 0), max(aug.th - p.h, 0), p.w, p.h) for p in b.params])


def wrong_mean_bytes(b, drop_from=PHOTO_THREADS):
    """(true m, m of a sum over the first `drop_from` tiles only, whether the contrast blend against the second gives other
    bytes) for a one-sample Batch with no step but the contrast blend: the device of test_contrast_mean_is_taken_after_hsv."""
    from cabinet_amd.augment import DeviceAugment

    aug, p = b.aug, b.params[0]
    crop = b.host(params=[dataclasses.replace(p, contrast=1.0)])[2][0]          # the brightened crop: what augment_geom writes
    luma = DeviceAugment._luma(crop).astype(np.int64)
    gx, gy = geom_grid(aug.th, aug.tw)
    part = np.array([luma[y:y + AUG_TY, x:x + AUG_TX].sum() for y in range(0, aug.th, AUG_TY) for x in range(0, aug.tw, AUG_TX)])
    assert part.size == gx * gy == tiles(aug.th, aug.tw)
    m = int(int(part.sum()) / (aug.th * aug.tw) + 0.5)
    m_wrong = int(int(part[:drop_from].sum()) / (aug.th * aug.tw) + 0.5)
    right = DeviceAugment._blend(np.full_like(crop, m), crop, p.contrast)
    wrong = DeviceAugment._blend(np.full_like(crop, m_wrong), crop, p.contrast)
    assert np.array_equal(right, b.host()[2][0])
    return m, m_wrong, not np.array_equal(right, wrong)


def first_tiles_mean(b, count=PHOTO_THREADS):
    """(mean luma of the first `count` tiles' own pixels, mean luma of the whole crop) of a one-sample Batch."""
    from cabinet_amd.augment import DeviceAugment

    aug, p = b.aug, b.params[0]
    luma = DeviceAugment._luma(b.host(params=[dataclasses.replace(p, contrast=1.0)])[2][0]).astype(np.float64)
    boxes = [luma[y:y + AUG_TY, x:x + AUG_TX] for y in range(0, aug.th, AUG_TY) for x in range(0, aug.tw, AUG_TX)][:count]
    return sum(float(t.sum()) for t in boxes) / sum(t.size for t in boxes), float(luma.mean())


# ------------------------------------------------------------------------------------------------ K18: the residue sweeps
SWEEP_TW = list(range(1, 68)) + list(range(126, 132))
SWEEP_TH = list(range(1, 19)) + list(range(31, 35))
SWEEP_TH_BLOCKS = [list(range(1, 7)), list(range(7, 13)), list(range(13, 19)), list(range(31, 35))]
SWEEP_SOURCES = [(40, 72), (33, 61)]
SWEEP_SEEDS = 20
POISON_CROPS = {0: (6, 6), 1: (5, 5), 2: (6, 7), 3: (7, 9)}      # P % 4 -> (tw, th); every P holds full groups and, but 0, a tail

_sweep_images = {}
_sweep = {}


def sweep_case(tw, th):
    """The Batch of one sweep shape under the Cityscapes preset with cutout_size 1, and the seed that gave it: the params are
    drawn from random.Random(seed) for seed = 1000 tw + th, then the next, until supported() takes both samples; None after
    SWEEP_SEEDS seeds."""
    from cabinet_amd.augment import DeviceAugment

    if (tw, th) in _sweep:
        return _sweep[(tw, th)]
    if not _sweep_images:
        for k, s in enumerate(SWEEP_SOURCES):
            _sweep_images[s] = source(s, k)
    aug = DeviceAugment.cityscapes(cropsize=(tw, th), cutout_size=1, label_map=LABEL_MAP)
    found = None
    for k in range(SWEEP_SEEDS):
        seed = 1000 * tw + th + k
        params = aug.draw(SWEEP_SOURCES, random.Random(seed))
        if all(aug.supported(s, p) for s, p in zip(SWEEP_SOURCES, params)):
            noise = noise_for(2, th, tw, seed) if any(p.noise for p in params) else None
            found = (Batch(aug, [_sweep_images[s][0] for s in SWEEP_SOURCES], [_sweep_images[s][1] for s in SWEEP_SOURCES],
                           list(SWEEP_SOURCES), params, noise), seed)
            break
    _sweep[(tw, th)] = found
    return found


def poison_case(res):
    """The Batch of the second sweep at P % 4 == res: every photometric step on, noise given."""
    tw, th = POISON_CROPS[res]
    aug = k18_aug((tw, th), cutout_size=2)
    sizes = [(th + 5, tw + 3), (th + 2, tw + 6)]
    drawn = aug.draw(sizes, random.Random(res))
    params = [dataclasses.replace(p, **dict(NEUTRAL, scale=1.0, w=W, h=H, sw=1 + k, sh=2 - k, flip=bool(k), cutout=(1, k), **_RICH))
              for k, (p, (H, W)) in enumerate(zip(drawn, sizes))]
    pairs = [source(s, 3 + k) for k, s in enumerate(sizes)]
    return Batch(aug, [a for a, _ in pairs], [b for _, b in pairs], sizes, params, noise_for(2, th, tw, 50 + res))


# ------------------------------------------------------------------------------------------------ K20: the passes' tables
RESIZE_OH = list(range(1, 19)) + [31, 32, 33]
RESIZE_OW = [1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129]
RESIZE_GROUPS = [RESIZE_OH[0:5], RESIZE_OH[5:9], RESIZE_OH[9:13], RESIZE_OH[13:17], RESIZE_OH[17:21]]
RATIO_NAMES = ["just above 1", "1.5", "2.0", "2.5"]


def ratio_in(n_out, k):
    """The source extent of an axis of n_out outputs at ratio RATIO_NAMES[k]: n_out + 1, floor(1.5 n_out), 2 n_out,
    floor(2.5 n_out) (2.5 exactly at even n_out), never below n_out."""
    return max((n_out + 1, (3 * n_out) // 2, 2 * n_out, (5 * n_out) // 2)[k], n_out)


def resize_item(oh, ow, ky, kx, seed=0):
    H, W = ratio_in(oh, ky), ratio_in(ow, kx)
    image, label = source((H, W), seed)
    return dict(image=image, label=label, H=H, W=W, out_h=oh, out_w=ow, resize=True, ratios=(ky, kx))


def resize_group(ohs):
    """One launch: every ow of RESIZE_OW at each oh of `ohs`; the ratio indices (i + j + 1, i + 2 j) mod 4 of (oh, ow) at table
    positions (i, j) take all 16 pairs, (2.5, 2.5) at even extents (6 x 2, 10 x 128, ...) where it is exact."""
    return [resize_item(oh, ow, (RESIZE_OH.index(oh) + j + 1) % 4, (RESIZE_OH.index(oh) + 2 * j) % 4) for oh in ohs for j, ow in enumerate(RESIZE_OW)]


def resize_mixed():
    """A 1 x 1 output beside a 47 x 96 one: five of the six workgroups of the small item leave at once."""
    big = dict(zip(("image", "label"), source((97, 200))), H=97, W=200, out_h=47, out_w=96, resize=True, ratios=None)
    one = dict(zip(("image", "label"), source((2, 2))), H=2, W=2, out_h=1, out_w=1, resize=True, ratios=None)
    return [one, big]


def resize_oracle(it):
    """The numpy route of the resize pass: _apply_taps along x then y with the tables warp_descs sends, the label by index."""
    from cabinet_amd.augment import DeviceAugment, _resize_axis

    (ct, lc), (rt, lr) = _resize_axis(it["W"], it["out_w"]), _resize_axis(it["H"], it["out_h"])
    return DeviceAugment._apply_taps(DeviceAugment._apply_taps(it["image"], ct, 1), rt, 0), it["label"][lr[:, None], lc[None, :]]


WARP_OH, WARP_OW = [7, 8, 9], [31, 32, 33, 63, 64, 65]
WARP_SHAPES = [(oh, ow) for oh in WARP_OH for ow in WARP_OW]
WARP_ANGLES = [0.01, -0.01, 44.99, -44.99, 45.0, -45.0]
EXPAND_SOURCES = [(8, 32), (9, 65), (7, 31)]


def warp_matrices(H, W):
    """[(kind, six coefficients)] for a source of H x W: the translates, the rotations (Image.rotate's matrix of this source,
    onto an output of the source's size) and the general matrices."""
    from cabinet_amd.augment import rotate_matrix

    shifts = [(0.3, -0.7), (3.0, -2.0), (-1.5, 2.25), (-4.0, 1.0), (0.25, 0.25), (-0.25, -0.25), (0.25, -0.25), (-0.25, 0.25),
              (float(W), 0.0), (-float(W), 0.0), (0.0, float(H)), (0.0, -float(H))]
    out = [("translate", (1, 0, dx, 0, 1, dy)) for dx, dy in shifts]
    out += [("rotate", rotate_matrix(W, H, a)[0]) for a in WARP_ANGLES]
    out += [("scale", (0.5, 0, 0.0, 0, 0.5, 0.0)), ("scale", (1.7, 0, -3.1, 0, 1.7, -0.4)),                      # per-axis label tables with a step
            ("shear", (1, 0.3, 0.0, 0, 1, 0.0)), ("scale-shear", (0.5, 0.3, 0.2, 0, 0.5, 1.1)), ("scale-shear", (1.7, 0, -3.0, 0.3, 1.7, -2.0))]
    return out


def warp_group(shape):
    """One launch: every matrix of warp_matrices x all four flips, source and output of `shape` = (oh, ow)."""
    H, W = shape
    image, label = source(shape)
    return [dict(image=image, label=label, H=H, W=W, out_h=H, out_w=W, a=a, flip=flip, fill=FILL, kind=kind)
            for kind, a in warp_matrices(H, W) for flip in range(4)]


def expand_group(size):
    """Image.rotate(expand=True) of one source at WARP_ANGLES x all four flips: outputs of the rotation's own sizes."""
    from cabinet_amd.augment import rotate_matrix

    H, W = size
    image, label = source(size, 1)
    items = []
    for angle in WARP_ANGLES:
        m, nw, nh = rotate_matrix(W, H, angle)
        items += [dict(image=image, label=label, H=H, W=W, out_h=nh, out_w=nw, a=m, flip=flip, fill=FILL, kind="expand", angle=angle) for flip in range(4)]
    return items


def warp_mixed():
    """A 1 x 1 output beside a 97 x 200 one, both label modes in one launch."""
    image, label = source((97, 200))
    tiny = source((3, 2))
    return [dict(image=tiny[0], label=tiny[1], H=3, W=2, out_h=1, out_w=1, a=(1, 0, 0.5, 0, 1, 1.25), flip=3, fill=FILL, kind="translate"),
            dict(image=image, label=label, H=97, W=200, out_h=97, out_w=200, a=(1.7, 0.3, -40.0, -0.3, 1.7, 5.0), flip=1, fill=FILL, kind="scale-shear")]


def label_mode(it):
    """warp_descs' choice, restated: Pillow takes per-axis tables where a[1] == a[3] == 0 and 16.16 fixed point elsewhere."""
    from cabinet_amd.augment import LABEL_FIXED, LABEL_TABLES

    return LABEL_TABLES if float(it["a"][1]) == 0 and float(it["a"][3]) == 0 else LABEL_FIXED


def warp_oracle(it):
    from cabinet_amd.augment import affine_image, affine_label

    return (affine_image(it["image"], it["a"], it["out_w"], it["out_h"], it["flip"]),
            affine_label(it["label"], it["a"], it["out_w"], it["out_h"], it["fill"], it["flip"]))


# ------------------------------------------------------------------------------------------------ K20: composition
COMPOSE_CROP, COMPOSE_CAP = (48, 40), 96
SMALL_SOURCES = [(60, 80), (72, 90), (50, 64), (33, 61)]          # none above the cap
LARGE_SOURCES = [(97, 200), (200, 97), (120, 110), (150, 180)]    # all above it: ratios 2.08, 2.08, 1.25, 1.875


def compose_aug():
    from cabinet_amd.augment import DeviceAugment

    return DeviceAugment.uavid(cropsize=COMPOSE_CROP, max_size=COMPOSE_CAP, cutout_size=8, label_map=LABEL_MAP)


def reparam(aug, size, p, **changes):
    """`p` with `changes` and everything draw() derives from them recomputed: resized, warped, (w, h), the crop offset clamped."""
    from cabinet_amd.augment import resize_if_larger, rotate_matrix

    p = dataclasses.replace(p, **changes)
    resized = resize_if_larger(size[0], size[1], aug.max_size)
    H, W = resized if resized is not None else size
    rot = rotate_matrix(W, H, p.angle)
    if rot is not None:
        H, W = rot[2], rot[1]
    w, h = int(round(W * p.scale)), int(round(H * p.scale))
    return dataclasses.replace(p, resized=resized, warped=(H, W), w=w, h=h, sw=min(p.sw, max(w, aug.tw) - aug.tw), sh=min(p.sh, max(h, aug.th) - aug.th))


def compose_batch(sizes, seed, angles=None):
    """A Batch of the aerial pipeline over `sizes` with drawn params (the first of SWEEP_SEEDS seeds from `seed` that
    supported() takes whole) and, with `angles`, each sample's angle replaced (0.0: no rotate pass for it)."""
    aug = compose_aug()
    for k in range(SWEEP_SEEDS):
        params = aug.draw(sizes, random.Random(seed + k))
        if angles is not None:
            params = [reparam(aug, s, p, angle=a) for s, p, a in zip(sizes, params, angles)]
        if all(aug.supported(s, p) for s, p in zip(sizes, params)):
            pairs = [source(s, i) for i, s in enumerate(sizes)]
            noise = noise_for(len(sizes), aug.th, aug.tw, seed) if any(p.noise for p in params) else None
            return Batch(aug, [a for a, _ in pairs], [b for _, b in pairs], list(sizes), params, noise)
    raise AssertionError((sizes, seed))


# ------------------------------------------------------------------------------------------------ Pillow's own calls
def _pil_flip(Image, im, flip):
    im = im.transpose(Image.FLIP_LEFT_RIGHT) if flip & 1 else im
    return im.transpose(Image.FLIP_TOP_BOTTOM) if flip & 2 else im


def pillow_resize(Image, it):
    return (np.array(Image.fromarray(it["image"]).resize((it["out_w"], it["out_h"]), Image.BILINEAR)),
            np.array(Image.fromarray(it["label"]).resize((it["out_w"], it["out_h"]), Image.NEAREST)))


def pillow_affine(Image, it):
    """Image.transform(AFFINE) of the flipped source (tests/test_aerial_augment.py's call)."""
    im, lb = _pil_flip(Image, Image.fromarray(it["image"]), it["flip"]), _pil_flip(Image, Image.fromarray(it["label"]), it["flip"])
    size, a = (it["out_w"], it["out_h"]), tuple(float(v) for v in it["a"])
    return (np.array(im.transform(size, Image.AFFINE, a, resample=Image.BILINEAR)),
            np.array(lb.transform(size, Image.AFFINE, a, resample=Image.NEAREST, fillcolor=it["fill"])))


def pillow_rotate(Image, it):
    im, lb = _pil_flip(Image, Image.fromarray(it["image"]), it["flip"]), _pil_flip(Image, Image.fromarray(it["label"]), it["flip"])
    return (np.array(im.rotate(it["angle"], resample=Image.BILINEAR, expand=True)),
            np.array(lb.rotate(it["angle"], resample=Image.NEAREST, expand=True, fillcolor=it["fill"])))


def pillow_k18(Image, aug, image, label, p):
    """The non-aerial pipeline in Pillow's and numpy's own calls, in the reference's order, with the values of `p` (no noise):
    (bytes (th, tw, 3), labels (th, tw) after the id map)."""
    from PIL import ImageEnhance

    im, lab = _pil_flip(Image, Image.fromarray(image), int(p.flip)), _pil_flip(Image, Image.fromarray(label), int(p.flip))
    im, lab = im.resize((p.w, p.h), Image.BILINEAR), lab.resize((p.w, p.h), Image.NEAREST)
    pw, ph = max(aug.tw - p.w, 0), max(aug.th - p.h, 0)
    if pw or ph:
        im = Image.fromarray(np.pad(np.array(im), ((0, ph), (0, pw), (0, 0)), mode="reflect"))
        lab = Image.fromarray(np.pad(np.array(lab), ((0, ph), (0, pw)), constant_values=aug.ignore_label).astype(np.uint8))
    box = (p.sw, p.sh, p.sw + aug.tw, p.sh + aug.th)
    im, lab = im.crop(box), lab.crop(box)
    if p.hsv is not None:
        hsv = np.array(im.convert("HSV"), dtype=np.int16)
        hsv[..., 0] = (hsv[..., 0] + round(p.hsv[0] * 255)) % 255
        hsv[..., 1] = np.clip(hsv[..., 1] * (p.hsv[1] + 1), 0, 255)
        hsv[..., 2] = np.clip(hsv[..., 2] * (p.hsv[2] + 1), 0, 255)
        hsv = hsv.astype(np.uint8)
        im = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(hsv[..., c])) for c in range(3)]).convert("RGB")
    im = ImageEnhance.Color(ImageEnhance.Contrast(ImageEnhance.Brightness(im).enhance(p.brightness)).enhance(p.contrast)).enhance(p.saturation)
    if p.gray:
        im = im.convert("L").convert("RGB")
    a = np.array(im)
    if p.gamma is not None:
        a = (np.clip((a.astype(np.float32) / 255.0) ** p.gamma, 0, 1) * 255).astype(np.uint8)
    if p.cutout is not None:
        a[p.cutout[0]:p.cutout[0] + aug.cutout_size, p.cutout[1]:p.cutout[1] + aug.cutout_size, :] = 0
    lab = np.array(lab)
    return a, np.where(lab == aug.ignore_label, aug.ignore_label, aug.label_lut[lab.astype(np.int64)])


def pillow_batch(Image, b):
    """[(bytes, labels)] of a Batch through pillow_k18, and the same Batch's numpy route, both with the noise step off."""
    params = [dataclasses.replace(p, noise=False) for p in b.params]
    want = [pillow_k18(Image, b.aug, im, lb, p) for im, lb, p in zip(b.images, b.labels, params)]
    got = b.host(params=params, noise=None)
    return want, got
