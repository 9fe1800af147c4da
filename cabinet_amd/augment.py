"""Training augmentation on the device: the reference's Cityscapes transform (src/datasets/cityscapes.py:114-136 with
src/datasets/transform.py) as two HIP launches per batch (csrc/augment.hip, K18).

    aug = DeviceAugment.cityscapes(cropsize=(1024, 1024), ignore_label=255, label_map=lut256)
    params = aug.draw(sizes=[(H, W), ...], rng=random.Random(seed))
    im, lb = aug(images, labels, params=params)          # im fp32 (N, 3, th, tw), lb int64 (N, th, tw)

The sequence is the reference's: horizontal flip, RandomScale (Pillow BILINEAR for the image, NEAREST for the label), RandomCrop
with reflect padding of the image and ``ignore_label`` padding of the label, the three ImageEnhance blends, grayscale, gamma,
Gaussian noise, cutout, ToTensor / Normalize and the id -> trainId lookup.  Everything but the VALUES of the noise is reproduced
byte for byte (tests/golden/g10_augment.npz is the reference's own output).

How: everything geometric is folded, on the host, into small integer tables -- per output column and per output row the source
taps of Pillow's antialiased resample with their 22-bit integer coefficients, and the label's source index.  The tables of a
(source size, scale) pair are built once and cached; the flip (taps walk backwards), the crop window (only its entries are sent)
and the reflection (a padded column takes the taps of its mirror column) are applied per sample.  The kernels then only walk
tables and do per-pixel integer and fp32 arithmetic.

The aerial datasets (src/datasets/uavid.py:192-230, vdd.py, aeroscapes.py; K20, csrc/augment_warp.hip) put ResizeIfLarger, a
vertical flip, RandomTranslate and RandomRotate(expand=True) ahead of the scale and RandomHSV behind the crop:

    aug = DeviceAugment.uavid(cropsize=(1024, 1024))     # or .vdd / .aeroscapes / .aerial(cropsize, augmentation={...})
    im, lb = aug(images, labels, rng=random.Random(seed))
    im, lb = DeviceAugment.mixup(im_a, lb_a, im_b, lb_b, r)

Those steps run as uint8 -> uint8 passes (Pillow truncates to bytes between them): resize where the source is larger than the
cap, translate with both flips folded into its source read, rotate; their output is the `image` / `label` of the two launches
above, whose geometry kernel also applies the HSV tables.

Routing: device tensors take the kernels and never fall back (a shape the kernels refuse raises); host tensors take the numpy
path below, which uses the same tables and the same arithmetic.
"""

from __future__ import annotations

import ctypes as _ct
import functools as _functools
import math as _math
import random as _random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["DeviceAugment", "SampleParams", "resample_taps", "nearest_index", "MAX_TAPS", "resize_if_larger", "rotate_matrix",
           "affine_image", "affine_label", "rgb_to_hsv", "hsv_to_rgb", "hsv_tables", "warp_descs"]

MAX_TAPS = 5
MAX_RATIO = 2.5                  # resize ratio in/out per axis: five taps at most, and fewer than 17 * 2.5 + 1 source rows per tile
TILE_ROWS, TILE_SPAN = 16, 48    # csrc/augment.hip: output rows of a workgroup tile, source rows it stages
_TABLE_CACHE = 32                # axis tables kept (Cityscapes' six scales need twelve); continuous scales evict the oldest
_PRECISION_BITS = 22
FLAG_GRAY, FLAG_GAMMA, FLAG_NOISE, FLAG_CUTOUT, FLAG_HSV = 1, 2, 4, 8, 16
MAX_ANGLE = 45.0                 # csrc/augment_warp.hip: the rotation pass covers 0 < |angle| <= 45 degrees (and 0, a copy)
MAX_SIDE = 32768
LABEL_TABLES, LABEL_FIXED = 0, 1
FLIP_X, FLIP_Y = 1, 2

# One table entry per sample; mirrors `cabinet_augment_sample` in include/cabinet_hip.h (2400 bytes)
SAMPLE_DTYPE = np.dtype([
    ("image", "<u8"), ("label", "<u8"), ("H", "<i4"), ("W", "<i4"),
    ("col_taps", "<u8"), ("row_taps", "<u8"), ("lab_col", "<u8"), ("lab_row", "<u8"),
    ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("flags", "<i4"),
    ("noise_scale", "<f4"), ("cut_y", "<i4"), ("cut_x", "<i4"), ("cut_size", "<i4"),
    ("ignore_label", "<i4"), ("reserved", "<i4"),
    ("gamma_lut", "u1", (256,)), ("label_lut", "<i8", (256,)),
])
TAP_DTYPE = np.dtype([("first", "<i4"), ("step", "<i4"), ("n", "<i4"), ("coef", "<i4", (MAX_TAPS,))])  # 32 bytes
# One descriptor per sample and pass; mirrors `cabinet_augment_warp_desc` in include/cabinet_hip.h (192 bytes)
WARP_DTYPE = np.dtype([
    ("src_image", "<u8"), ("src_label", "<u8"), ("dst_image", "<u8"), ("dst_label", "<u8"),
    ("H", "<i4"), ("W", "<i4"), ("out_h", "<i4"), ("out_w", "<i4"), ("a", "<f8", (6,)), ("fix", "<i8", (6,)),
    ("lab_col", "<u8"), ("lab_row", "<u8"), ("col_taps", "<u8"), ("row_taps", "<u8"),
    ("flip", "<i4"), ("label_mode", "<i4"), ("fill", "<i4"), ("reserved", "<i4"),
])
assert SAMPLE_DTYPE.itemsize == 2400 and TAP_DTYPE.itemsize == 32 and WARP_DTYPE.itemsize == 192


# --------------------------------------------------------------------------- tables

def resample_taps(n_in: int, n_out: int):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the BILINEAR filter along one axis, vectorised in double:
    (first (n_out,), n (n_out,), coef (n_out, kmax)) int32.  Output ``xx`` is clip8((2^21 + sum_k coef[k] * in[first + k]) >> 22)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    xx = np.arange(n_out, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = xmax - xmin
    kmax = int(n.max())
    k = np.arange(kmax, dtype=np.float64)[None, :]
    w = (k + xmin[:, None] - center[:, None] + 0.5) * ss
    w = np.abs(w)
    w = np.where(w < 1.0, 1.0 - w, 0.0)
    w = np.where(k < n[:, None], w, 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for j in range(kmax):  # the sum runs in tap order, as Pillow's loop does
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    coef = (0.5 + w * float(1 << _PRECISION_BITS)).astype(np.int64)
    coef = np.where(k < n[:, None], coef, 0)
    return xmin.astype(np.int32), n.astype(np.int32), coef.astype(np.int32)


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """Source index of every output position of Pillow's ``resize(NEAREST)`` along one axis: ``(int) xo`` with ``xo`` starting at
    half a step and ACCUMULATED by repeated addition in double (the closed form differs at hundreds of columns of a 2048-wide
    image), clamped into the source."""
    step = n_in / n_out
    xo = np.empty(n_out, dtype=np.float64)
    xo[0] = step * 0.5
    if n_out > 1:
        steps = np.full(n_out, step, dtype=np.float64)
        steps[0] = xo[0]
        xo = np.cumsum(steps)  # a running sum in index order: xo[i] = xo[i - 1] + step
    return np.clip(xo.astype(np.int64), 0, n_in - 1).astype(np.int32)


class _AxisTables(object):
    __slots__ = ("first", "n", "coef", "label")

    def __init__(self, n_in, n_out):
        self.first, self.n, self.coef = resample_taps(n_in, n_out)
        if self.coef.shape[1] < MAX_TAPS:
            self.coef = np.pad(self.coef, ((0, 0), (0, MAX_TAPS - self.coef.shape[1])))
        self.label = nearest_index(n_in, n_out)


@_functools.lru_cache(maxsize=8)
def _resize_axis(n_in: int, n_out: int):
    """(taps, label index) of a whole resized axis, unflipped: ResizeIfLarger meets a handful of sizes per dataset."""
    tab = _AxisTables(n_in, n_out)
    taps = np.zeros(n_out, dtype=TAP_DTYPE)
    taps["first"], taps["step"], taps["n"], taps["coef"] = tab.first, 1, tab.n, tab.coef
    return taps, tab.label


# --------------------------------------------------------------------------- aerial geometry (K20): Pillow's arithmetic, restated

def resize_if_larger(H: int, W: int, cap) -> Optional[Tuple[int, int]]:
    """ResizeIfLarger's target (h, w), or None where it does not act."""
    if cap is None or max(W, H) <= cap:
        return None
    scale = cap / max(W, H)
    return max(1, round(H * scale)), max(1, round(W * scale))


def rotate_matrix(W: int, H: int, angle: float):
    """Image.rotate(angle, expand=True): (the six coefficients, nw, nh), or None for an angle that is a copy."""
    angle = angle % 360.0
    if angle == 0:
        return None
    r = -_math.radians(angle)
    m = [round(_math.cos(r), 15), round(_math.sin(r), 15), 0.0, round(-_math.sin(r), 15), round(_math.cos(r), 15), 0.0]

    def T(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = T(-(W / 2.0), -(H / 2.0))
    m[2] += W / 2.0
    m[5] += H / 2.0
    xs, ys = zip(*[T(x, y) for x, y in ((0, 0), (W, 0), (W, H), (0, H))])
    nw = _math.ceil(max(xs)) - _math.floor(min(xs))
    nh = _math.ceil(max(ys)) - _math.floor(min(ys))
    m[2], m[5] = T(-(nw - W) / 2.0, -(nh - H) / 2.0)
    return tuple(m), int(nw), int(nh)


def _flipped(src, flip):
    src = src[:, ::-1] if flip & FLIP_X else src
    return src[::-1] if flip & FLIP_Y else src


def affine_image(src: np.ndarray, a, out_w: int, out_h: int, flip: int = 0) -> np.ndarray:
    """Image.transform((out_w, out_h), AFFINE, a, BILINEAR) of uint8 (H, W, 3), read through ``flip``: double, every operation
    rounded on its own, the byte by truncation; outside the source 0."""
    src = _flipped(src, flip)
    H, W = src.shape[:2]
    a = [float(v) for v in a]
    out = np.zeros((out_h, out_w, 3), dtype=np.uint8)
    xh = np.arange(out_w, dtype=np.float64) + 0.5
    ax0, ax3 = a[0] * xh, a[3] * xh
    for y0 in range(0, out_h, 128):
        yh = np.arange(y0, min(out_h, y0 + 128), dtype=np.float64) + 0.5
        xin = (ax0[None, :] + (a[1] * yh)[:, None]) + a[2]
        yin = (ax3[None, :] + (a[4] * yh)[:, None]) + a[5]
        ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
        if not ok.any():
            continue
        xs, ys = np.where(ok, xin, 0.5) - 0.5, np.where(ok, yin, 0.5) - 0.5
        xf, yf = np.floor(xs), np.floor(ys)
        dx, dy = (xs - xf)[..., None], (ys - yf)[..., None]
        xf, yf = xf.astype(np.int64), yf.astype(np.int64)
        c0, c1 = np.clip(xf, 0, W - 1), np.clip(xf + 1, 0, W - 1)
        r0, r1 = np.clip(yf, 0, H - 1), np.clip(yf + 1, 0, H - 1)
        below = ((yf + 1 >= 0) & (yf + 1 < H))[..., None]
        p00, p01 = src[r0, c0].astype(np.float64), src[r0, c1].astype(np.float64)
        p10, p11 = src[r1, c0].astype(np.float64), src[r1, c1].astype(np.float64)
        v1 = p00 + (p01 - p00) * dx
        v2 = np.where(below, p10 + (p11 - p10) * dx, v1)
        v = v1 + (v2 - v1) * dy
        out[y0:y0 + yh.size] = np.where(ok[..., None], v.astype(np.uint8), 0)
    return out


def _fix16(v: float) -> int:
    return int(_math.floor(v * 65536.0 + 0.5))


def affine_fixed(a) -> Tuple[int, ...]:
    """Pillow's 16.16 coefficients of a general affine NEAREST transform."""
    a = [float(v) for v in a]
    return (_fix16(a[0]), _fix16(a[1]), _fix16(a[2] + a[0] * 0.5 + a[1] * 0.5),
            _fix16(a[3]), _fix16(a[4]), _fix16(a[5] + a[3] * 0.5 + a[4] * 0.5))


def affine_axis_table(offset: float, step: float, n_out: int, n_in: int) -> np.ndarray:
    """Pillow's per-axis table of an axis-aligned NEAREST transform: xo from offset + step / 2 by a running sum in double; the
    entry is (int) xo, -1 where xo < 0 or the index is past the source."""
    steps = np.full(n_out, float(step), dtype=np.float64)
    steps[0] = float(offset) + float(step) * 0.5
    xo = np.cumsum(steps)   # a running sum in index order
    idx = np.where(xo < 0, -1.0, np.trunc(np.clip(xo, -1.0, float(n_in)))).astype(np.int64)
    return np.where(idx >= n_in, -1, idx).astype(np.int32)


def affine_label(src: np.ndarray, a, out_w: int, out_h: int, fill: int, flip: int = 0) -> np.ndarray:
    """Image.transform((out_w, out_h), AFFINE, a, NEAREST, fillcolor=fill) of uint8 (H, W), read through ``flip``: per-axis
    tables where a[1] == a[3] == 0, Pillow's 16.16 fixed point otherwise."""
    src = _flipped(src, flip)
    H, W = src.shape
    a = [float(v) for v in a]
    if a[1] == 0 and a[3] == 0:
        lc, lr = affine_axis_table(a[2], a[0], out_w, W)[None, :], affine_axis_table(a[5], a[4], out_h, H)[:, None]
    else:
        A = affine_fixed(a)
        x, y = np.arange(out_w, dtype=np.int64)[None, :], np.arange(out_h, dtype=np.int64)[:, None]
        lc, lr = (A[2] + y * A[1] + x * A[0]) >> 16, (A[5] + y * A[4] + x * A[3]) >> 16
    ok = (lc >= 0) & (lc < W) & (lr >= 0) & (lr < H)
    return np.where(ok, src[np.clip(lr, 0, H - 1), np.clip(lc, 0, W - 1)], fill).astype(np.uint8)


def rgb_to_hsv(a: np.ndarray) -> np.ndarray:
    """Pillow's convert("HSV") of uint8 (..., 3): fp32 divisions, the hue's sum and wrap in double."""
    r, g, b = [a[..., i].astype(np.int32) for i in range(3)]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    ok = mx != mn
    cr = np.where(ok, mx - mn, 1).astype(np.float32)
    s = cr / np.where(ok, mx, 1).astype(np.float32)
    rc, gc, bc = [(mx - c).astype(np.float32) / cr for c in (r, g, b)]
    rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    h = np.where(r == mx, bc - gc, np.where(g == mx, ((2.0 + rc64) - bc64).astype(np.float32), ((4.0 + gc64) - rc64).astype(np.float32)))
    h = np.fmod(h.astype(np.float32).astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(ok, H, 0), np.where(ok, S, 0), mx], axis=-1).astype(np.uint8)


def hsv_to_rgb(a: np.ndarray) -> np.ndarray:
    """Pillow's HSV -> RGB of uint8 (..., 3): f and S / 255 rounded to fp32, the products in double, C's round."""
    H, S, V = [a[..., i].astype(np.float64) for i in range(3)]
    hh = H * 6.0 / 255.0
    i = np.floor(hh)
    f = (hh - i).astype(np.float32).astype(np.float64)
    fs = (S / 255.0).astype(np.float32).astype(np.float64)
    cround = lambda v: np.clip(np.floor(v + 0.5), 0, 255)  # noqa: E731  (C's round of a non-negative value)
    p, q, t = cround(V * (1.0 - fs)), cround(V * (1.0 - fs * f)), cround(V * (1.0 - fs * (1.0 - f)))
    k = i.astype(np.int64) % 6
    R, G, B = np.choose(k, [V, q, p, p, t, V]), np.choose(k, [t, V, V, q, p, p]), np.choose(k, [p, p, t, V, V, q])
    out = np.stack([R, G, B], axis=-1)
    return np.where((a[..., 1] == 0)[..., None], V[..., None], out).astype(np.uint8)


def hsv_tables(r_h: float, r_s: float, r_v: float) -> np.ndarray:
    """RandomHSV's three byte tables (3, 256), by the reference's numpy expressions on every byte value."""
    hsv = np.repeat(np.arange(256, dtype=np.int16)[:, None], 3, axis=1)
    hsv[..., 0] = (hsv[..., 0] + round(r_h * 255)) % 255
    hsv[..., 1] = np.clip(hsv[..., 1] * (r_s + 1), 0, 255)
    hsv[..., 2] = np.clip(hsv[..., 2] * (r_v + 1), 0, 255)
    return np.ascontiguousarray(hsv.astype(np.uint8).T)


def apply_hsv(im: np.ndarray, tables: np.ndarray) -> np.ndarray:
    hsv = rgb_to_hsv(im)
    return hsv_to_rgb(np.stack([tables[0][hsv[..., 0]], tables[1][hsv[..., 1]], tables[2][hsv[..., 2]]], axis=-1))


def warp_descs(items) -> np.ndarray:
    """The device block of cabinet_augment_warp_batch / cabinet_augment_resize_batch as host bytes: one cabinet_augment_warp_desc
    per item, then the tables they name.  An item is a dict with src_image, src_label, dst_image, dst_label (device addresses),
    H, W, out_h, out_w and either ``a`` (six coefficients; optional ``flip`` and ``fill``) for the affine pass -- the label
    route follows Pillow's choice -- or ``resize=True`` for the resize pass."""
    a16 = lambda v: (v + 15) & ~15  # noqa: E731
    head = a16(len(items) * WARP_DTYPE.itemsize)
    tables, off = [], head
    entries = np.zeros(len(items), dtype=WARP_DTYPE)
    for e, it in zip(entries, items):
        for k in ("src_image", "src_label", "dst_image", "dst_label", "H", "W", "out_h", "out_w"):
            e[k] = it[k]
        H, W, oh, ow = int(it["H"]), int(it["W"]), int(it["out_h"]), int(it["out_w"])
        named = []
        if it.get("resize"):
            (ct, lc), (rt, lr) = _resize_axis(W, ow), _resize_axis(H, oh)
            named += [("col_taps", ct), ("row_taps", rt), ("lab_col", lc), ("lab_row", lr)]
        else:
            a = [float(v) for v in it["a"]]
            e["a"], e["flip"], e["fill"] = a, int(it.get("flip", 0)), int(it.get("fill", 0))
            if a[1] == 0 and a[3] == 0:
                e["label_mode"] = LABEL_TABLES
                named += [("lab_col", affine_axis_table(a[2], a[0], ow, W)), ("lab_row", affine_axis_table(a[5], a[4], oh, H))]
            else:
                e["label_mode"], e["fix"] = LABEL_FIXED, affine_fixed(a)
        for name, arr in named:
            raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            e[name] = off
            tables.append((off, raw))
            off += a16(raw.size)
    blob = np.zeros(off, dtype=np.uint8)
    blob[:entries.nbytes] = entries.view(np.uint8)
    for o, raw in tables:
        blob[o:o + raw.size] = raw
    return blob


@dataclass
class SampleParams:
    """What the reference's Compose draws for one sample, in its order."""
    flip: bool
    scale: float
    w: int            # resized size
    h: int
    sw: int           # crop offset inside the padded resized image
    sh: int
    brightness: float
    contrast: float
    saturation: float
    gray: bool
    gamma: Optional[float]
    noise: bool
    cutout: Optional[Tuple[int, int]]   # (y, x)
    # the aerial steps (K20); the defaults are "the step is absent"
    vflip: bool = False
    dx: float = 0.0                               # RandomTranslate, in pixels of the (resized) source
    dy: float = 0.0
    angle: float = 0.0                            # RandomRotate, degrees
    hsv: Optional[Tuple[float, float, float]] = None   # RandomHSV's r_h, r_s, r_v (gain times uniform(-1, 1))
    resized: Optional[Tuple[int, int]] = None     # (H, W) after ResizeIfLarger, None where it does not act
    warped: Optional[Tuple[int, int]] = None      # (H, W) entering RandomScale, None without the aerial geometry


class DeviceAugment(object):
    """The reference's train-time transform for batches; see the module docstring.  ``cropsize`` is (target_w, target_h), the
    order of the reference's RandomCrop.  ``brightness`` / ``contrast`` / ``saturation`` are the reference's jitter widths
    (``v`` -> uniform(max(1 - v, 0), 1 + v)) or None.  ``label_map``: 256 entries id -> trainId, or None for the identity.

    The aerial datasets' steps, each absent at None: ``max_size`` (ResizeIfLarger's cap), ``vflip_p``, ``translate`` (fraction of
    the size), ``degrees`` (RandomRotate over (-degrees, degrees), expand=True) -- any of these four runs the whole chain
    resize, flips, translate, rotate ahead of the scale, as the reference's pipeline holds all of them -- and ``hsv`` =
    (hgain, sgain, vgain) of RandomHSV behind the crop.  ``grayscale_p=None``: a pipeline without the grayscale step."""

    def __init__(self, cropsize, ignore_label=255, label_map=None, scales=(1.0,), continuous=False, flip_p=0.5, brightness=None,
                 contrast=None, saturation=None, grayscale_p=0.0, gamma_range=(0.7, 1.5), gamma_p=0.0, noise_sigma=0.05,
                 noise_p=0.0, cutout_p=0.0, cutout_size=64, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), seed=None,
                 max_size=None, vflip_p=None, translate=None, degrees=None, hsv=None):
        self.tw, self.th = int(cropsize[0]), int(cropsize[1])
        if self.tw < 1 or self.th < 1:
            raise ValueError(f"DeviceAugment: cropsize {cropsize} must be positive")
        self.ignore_label = int(ignore_label)
        lut = np.arange(256, dtype=np.int64) if label_map is None else np.asarray(label_map, dtype=np.int64).reshape(-1)
        if lut.shape != (256,):
            raise ValueError("DeviceAugment: label_map must have 256 entries (id -> trainId)")
        self.label_lut = lut.copy()
        self.continuous = bool(continuous)
        self.scales = tuple(float(s) for s in scales)
        if self.continuous and len(self.scales) != 2:
            raise ValueError("DeviceAugment: continuous=True takes scales=(low, high)")
        self.flip_p = float(flip_p)
        jit = lambda v: None if v is None else (max(1 - v, 0), 1 + v)  # noqa: E731  (RandomColorJitter._check)
        self.brightness, self.contrast, self.saturation = jit(brightness), jit(contrast), jit(saturation)
        # grayscale_p=None: the pipeline has no RandomGrayscale step at all (the aerial datasets'), so nothing is drawn for it
        self.grayscale_p = None if grayscale_p is None else float(grayscale_p)
        self.gamma_range, self.gamma_p = tuple(gamma_range), float(gamma_p)
        self.noise_sigma, self.noise_p = float(noise_sigma), float(noise_p)
        self.cutout_p, self.cutout_size = float(cutout_p), int(cutout_size)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self._seed = _random.SystemRandom().getrandbits(63) if seed is None else int(seed)
        self._calls = 0
        self._tables = {}
        # the aerial steps: any of the four geometric keywords puts the whole chain ResizeIfLarger, flips, RandomTranslate,
        # RandomRotate ahead of RandomScale, each with "never" / zero width where its own keyword is None, drawn as the reference draws
        self.aerial = any(v is not None for v in (max_size, vflip_p, translate, degrees))
        self.max_size = None if max_size is None else int(max_size)
        self.vflip_p = 0.0 if vflip_p is None else float(vflip_p)
        self.translate = 0.0 if translate is None else float(translate)
        self.degrees = 0.0 if degrees is None else float(degrees)
        self.hsv = None if hsv is None else tuple(float(v) for v in hsv)
        if self.hsv is not None and len(self.hsv) != 3:
            raise ValueError("DeviceAugment: hsv takes (hgain, sgain, vgain)")
        self.mixup_p = 0.0
        self._buffers = {}

    @classmethod
    def cityscapes(cls, cropsize=(1024, 1024), ignore_label=255, label_map=None, **overrides):
        """The reference's default Cityscapes train pipeline (src/datasets/cityscapes.py:114-136)."""
        kw = dict(scales=(0.75, 1.0, 1.25, 1.5, 1.75, 2.0), flip_p=0.5, brightness=0.5, contrast=0.5, saturation=0.5,
                  grayscale_p=0.2, gamma_range=(0.8, 1.2), gamma_p=0.3, noise_sigma=0.03, noise_p=0.3, cutout_p=0.3, cutout_size=64)
        kw.update(overrides)
        return cls(cropsize, ignore_label=ignore_label, label_map=label_map, **kw)

    AERIAL_DEFAULTS = dict(degrees=10.0, translate=0.05, scale=0.3, flipud=0.2, fliplr=0.5, hsv_h=0.01, hsv_s=0.4, hsv_v=0.3, mixup=0.1)

    @classmethod
    def aerial(cls, cropsize=(1024, 1024), augmentation=None, ignore_label=255, label_map=None, **overrides):
        """The train pipeline the reference's aerial datasets share (src/datasets/uavid.py:192-230); ``augmentation`` takes the
        reference's ``augmentation:`` keys over its defaults.  Its ``mixup`` probability is kept as ``mixup_p`` for the caller."""
        unknown = set(augmentation or {}) - set(cls.AERIAL_DEFAULTS)
        if unknown:
            raise ValueError(f"DeviceAugment.aerial: unknown augmentation keys {sorted(unknown)}")
        a = {**cls.AERIAL_DEFAULTS, **(augmentation or {})}
        scale = float(a["scale"])
        kw = dict(max_size=2 * max(cropsize), flip_p=float(a["fliplr"]), vflip_p=float(a["flipud"]), translate=float(a["translate"]),
                  degrees=float(a["degrees"]), scales=(1.0 - scale, 1.0 + scale), continuous=True,
                  hsv=(float(a["hsv_h"]), float(a["hsv_s"]), float(a["hsv_v"])), contrast=0.5, grayscale_p=None,
                  gamma_range=(0.8, 1.2), gamma_p=0.3, noise_sigma=0.03, noise_p=0.3, cutout_p=0.3, cutout_size=64)
        kw.update(overrides)
        aug = cls(cropsize, ignore_label=ignore_label, label_map=label_map, **kw)
        aug.mixup_p = float(a["mixup"])
        return aug

    @classmethod
    def uavid(cls, cropsize=(1024, 1024), augmentation=None, **overrides):
        """src/datasets/uavid.py: its normalisation constants."""
        kw = dict(mean=(0.480, 0.499, 0.457), std=(0.225, 0.208, 0.228))
        kw.update(overrides)
        return cls.aerial(cropsize, augmentation, **kw)

    @classmethod
    def vdd(cls, cropsize=(1024, 1024), augmentation=None, **overrides):
        """src/datasets/vdd.py."""
        kw = dict(mean=(0.486, 0.487, 0.441), std=(0.190, 0.178, 0.214))
        kw.update(overrides)
        return cls.aerial(cropsize, augmentation, **kw)

    @classmethod
    def aeroscapes(cls, cropsize=(640, 640), augmentation=None, **overrides):
        """src/datasets/aeroscapes.py."""
        kw = dict(mean=(0.439, 0.508, 0.460), std=(0.176, 0.157, 0.194))
        kw.update(overrides)
        return cls.aerial(cropsize, augmentation, **kw)

    @staticmethod
    def mixup(im_a, lb_a, im_b, lb_b, r):
        """The reference's MixUp (src/datasets/uavid.py:256-269) of two normalised fp32 tensors: im_a r + im_b (1 - r), each
        product and the sum an operation of its own, and the whole label of whichever sample holds the larger share."""
        r = float(r)
        return im_a * r + im_b * (1.0 - r), (lb_a if r >= 0.5 else lb_b)

    # ------------------------------------------------------------------ parameters

    def draw(self, sizes: Sequence[Tuple[int, int]], rng=None) -> List[SampleParams]:
        """One SampleParams per (H, W) of ``sizes``, consuming ``rng`` (a ``random.Random``; None: the module-level generator)
        exactly as the reference's Compose consumes ``random``."""
        rng = _random if rng is None else rng
        out = []
        for H, W in sizes:
            flip = not (rng.random() > self.flip_p)
            extra = {}
            if self.aerial:
                resized = resize_if_larger(H, W, self.max_size)
                H, W = resized if resized is not None else (H, W)
                vflip = not (rng.random() > self.vflip_p)
                dx = rng.uniform(-self.translate, self.translate) * W
                dy = rng.uniform(-self.translate, self.translate) * H
                angle = rng.uniform(-self.degrees, self.degrees)
                rot = rotate_matrix(W, H, angle)
                if rot is not None:
                    H, W = rot[2], rot[1]
                extra = dict(vflip=vflip, dx=dx, dy=dy, angle=angle, resized=resized, warped=(H, W))
            scale = rng.uniform(*self.scales) if self.continuous else rng.choice(self.scales)
            w, h = int(round(W * scale)), int(round(H * scale))
            pw, ph = max(w, self.tw), max(h, self.th)
            sw = rng.randint(0, pw - self.tw) if pw > self.tw else 0
            sh = rng.randint(0, ph - self.th) if ph > self.th else 0
            if self.hsv is not None and any(self.hsv):
                extra["hsv"] = tuple(rng.uniform(-1, 1) * g for g in self.hsv)
            rb = rng.uniform(*self.brightness) if self.brightness else 1.0
            rc = rng.uniform(*self.contrast) if self.contrast else 1.0
            rs = rng.uniform(*self.saturation) if self.saturation else 1.0
            gray = False if self.grayscale_p is None else rng.random() < self.grayscale_p
            gamma = rng.uniform(*self.gamma_range) if rng.random() < self.gamma_p else None
            noise = rng.random() < self.noise_p
            cutout = None
            if rng.random() < self.cutout_p:
                y = rng.randint(0, self.th - self.cutout_size)
                x = rng.randint(0, self.tw - self.cutout_size)
                cutout = (y, x)
            out.append(SampleParams(flip, scale, w, h, sw, sh, rb, rc, rs, gray, gamma, noise, cutout, **extra))
        return out

    def supported(self, size: Tuple[int, int], p: SampleParams) -> bool:
        """Whether the kernels cover this sample: a resize ratio in/out of at most 2.5 per axis (scale >= 0.4), which is what
        bounds both the taps per output pixel (five) and the source rows a tile of the geometry kernel stages, and a reflect pad
        below the resized size.  Both routes refuse the same samples."""
        return self._limits(size, p)[0]

    def _limits(self, size, p: SampleParams):
        """(covered, taps, pad_y, pad_x) of one sample; the tap count is 0 where the ratio already rules the sample out."""
        H, W = self._scale_source(size, p)
        pad_y, pad_x = max(self.th - p.h, 0), max(self.tw - p.w, 0)
        if self._warp_refusal(size, p) is not None:
            return False, 0, pad_y, pad_x
        if p.w < 1 or p.h < 1 or W > MAX_RATIO * p.w or H > MAX_RATIO * p.h:
            return False, 0, pad_y, pad_x
        taps = int(max(self._axis(W, p.w).n.max(), self._axis(H, p.h).n.max()))
        return bool(taps <= MAX_TAPS and pad_x <= p.w - 1 and pad_y <= p.h - 1), taps, pad_y, pad_x

    def _scale_source(self, size, p: SampleParams):
        """(H, W) of what RandomScale resizes: the source itself, or the output of the aerial geometry."""
        if not self.aerial:
            return size
        if p.warped is None:
            raise ValueError("DeviceAugment: the aerial steps need SampleParams from draw() (resized / warped sizes)")
        return p.warped

    def _warp_refusal(self, size, p: SampleParams) -> Optional[str]:
        """The aerial step that refuses this sample, in words, or None."""
        if not self.aerial:
            return None
        H, W = size
        if max(H, W) > MAX_SIDE:
            return f"the source side {max(H, W)} is above {MAX_SIDE}"
        if p.resized is not None and (H > MAX_RATIO * p.resized[0] or W > MAX_RATIO * p.resized[1]):
            return (f"ResizeIfLarger({self.max_size}) of {H}x{W} to {p.resized[0]}x{p.resized[1]}: ratio in/out above {MAX_RATIO} "
                    f"(at most {MAX_TAPS} taps)")
        a = p.angle % 360.0
        if not (a == 0 or a <= MAX_ANGLE or a >= 360.0 - MAX_ANGLE):
            return f"RandomRotate by {p.angle:.3f} degrees: |angle| above {MAX_ANGLE:g}"
        return None

    def warp_plan(self, size, p: SampleParams):
        """The passes of the aerial geometry for one sample, in order: a list of dicts with ``H``, ``W`` (the pass's source),
        ``out_h``, ``out_w`` and ``resize=True`` or ``a`` / ``flip`` / ``fill`` (see warp_descs)."""
        H, W = size
        plan = []
        if p.resized is not None:
            if tuple(p.resized) != resize_if_larger(H, W, self.max_size):
                raise ValueError(f"DeviceAugment: SampleParams.resized {p.resized} is not ResizeIfLarger({self.max_size}) of {H}x{W}")
            plan.append(dict(H=H, W=W, out_h=p.resized[0], out_w=p.resized[1], resize=True))
            H, W = p.resized
        flip = (FLIP_X if p.flip else 0) | (FLIP_Y if p.vflip else 0)
        plan.append(dict(H=H, W=W, out_h=H, out_w=W, a=(1, 0, p.dx, 0, 1, p.dy), flip=flip, fill=self.ignore_label))
        rot = rotate_matrix(W, H, p.angle)
        if rot is not None:
            plan.append(dict(H=H, W=W, out_h=rot[2], out_w=rot[1], a=rot[0], flip=0, fill=self.ignore_label))
            H, W = rot[2], rot[1]
        if (H, W) != tuple(p.warped):
            raise ValueError(f"DeviceAugment: SampleParams.warped {p.warped} does not follow from the sample's geometry ({H}, {W})")
        return plan

    # ------------------------------------------------------------------ tables

    def _axis(self, n_in, n_out) -> _AxisTables:
        key = (int(n_in), int(n_out))
        t = self._tables.pop(key, None)
        if t is None:
            t = _AxisTables(*key)
            while len(self._tables) >= _TABLE_CACHE:
                del self._tables[next(iter(self._tables))]   # the least recently used: a hit moves its entry to the end
        self._tables[key] = t
        return t

    @staticmethod
    def _window(tab: _AxisTables, n_in, n_res, start, count, flip):
        """Tap and label tables of ``count`` output positions from ``start`` of the padded axis."""
        pos = start + np.arange(count)
        pad = pos >= n_res
        src = np.where(pad, 2 * (n_res - 1) - pos, pos)
        taps = np.zeros(count, dtype=TAP_DTYPE)
        first = tab.first[src]
        taps["first"] = (n_in - 1 - first) if flip else first
        taps["step"] = -1 if flip else 1
        taps["n"] = tab.n[src]
        taps["coef"] = tab.coef[src]
        lab = tab.label[src]
        lab = np.where(pad, -1, (n_in - 1 - lab) if flip else lab).astype(np.int32)
        return taps, lab

    def gamma_lut(self, gamma: Optional[float]) -> np.ndarray:
        if gamma is None:
            return np.arange(256, dtype=np.uint8)
        im = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0   # the reference's expression (transform.py RandomGamma)
        im = np.clip(im ** gamma, 0, 1)
        return (im * 255).astype(np.uint8)

    def _sample_tables(self, size, p: SampleParams):
        """``size``: what RandomScale resizes (_scale_source).  With the aerial geometry the flip is already in the translate pass."""
        H, W = size
        flip = p.flip and not self.aerial
        if p.cutout is not None and not (0 <= p.cutout[0] <= self.th - self.cutout_size and 0 <= p.cutout[1] <= self.tw - self.cutout_size):
            raise ValueError("DeviceAugment: cutout square outside the crop")
        ct, lc = self._window(self._axis(W, p.w), W, p.w, p.sw, self.tw, flip)
        rt, lr = self._window(self._axis(H, p.h), H, p.h, p.sh, self.th, False)
        tile = np.arange(0, self.th, TILE_ROWS)
        span = np.maximum.reduceat(rt["first"] + np.maximum(rt["n"], 1) - 1, tile) - np.minimum.reduceat(rt["first"], tile) + 1
        if int(span.max()) > TILE_SPAN:   # cannot happen inside coverage (MAX_RATIO); the kernel would read the wrong rows
            raise RuntimeError(f"DeviceAugment: a tile of {TILE_ROWS} output rows needs {int(span.max())} source rows, more than {TILE_SPAN}")
        return ct, rt, lc, lr

    def _check(self, sizes, params):
        """Raises for a sample outside coverage; returns what the batch asks of cabinet_augment_supported: its largest tap count
        and pads, its smallest resized size."""
        taps = pad_y = pad_x = 0
        for i, (s, p) in enumerate(zip(sizes, params)):
            ok, t, py, px = self._limits(s, p)
            why = self._warp_refusal(s, p)
            if why is not None:
                raise RuntimeError(f"DeviceAugment: sample {i} (source {s[0]}x{s[1]}) is outside coverage: {why}")
            if not ok:
                s = self._scale_source(s, p)
                step = "padding: RandomCrop's reflect pad >= the resized size" if t and t <= MAX_TAPS else "RandomScale: ratio above 2.5"
                raise RuntimeError(f"DeviceAugment: sample {i} (source {s[0]}x{s[1]}, resized {p.h}x{p.w}, crop {self.th}x{self.tw}) is "
                                   f"outside coverage ({step}): a resize ratio in/out <= {MAX_RATIO} per axis (scale >= 0.4, at most "
                                   f"{MAX_TAPS} taps) and padding <= resized size - 1")
            taps, pad_y, pad_x = max(taps, t), max(pad_y, py), max(pad_x, px)
        return taps, pad_y, pad_x, min(p.h for p in params), min(p.w for p in params)

    # ------------------------------------------------------------------ call

    def __call__(self, images, labels, params=None, rng=None, seed=None, noise=None, out=None, return_uint8=False):
        """``images``: list of uint8 (H_i, W_i, 3); ``labels``: list of uint8 (H_i, W_i).  Returns (im fp32 (N, 3, th, tw),
        lb int64 (N, th, tw)) and, with ``return_uint8``, the final bytes uint8 (N, th, tw, 3).

        ``params`` replays recorded parameters, otherwise they are drawn from ``rng``.  ``noise``: fp32 (N, th, tw, 3) values
        already scaled by sigma * 255, used as given for the samples whose noise step applies; None: standard normals from the
        counter-based generator keyed by (``seed``, sample, pixel) times sigma * 255 (``seed=None``: the object's own seed plus a
        call counter; the host path draws from numpy's generator seeded with (seed, sample) instead: its values differ from the
        device's, as both differ from the reference's).  ``out=(im, lb)``: caller-owned dense tensors, e.g. the static inputs of a graphed step."""
        images, labels = list(images), list(labels)
        N = len(images)
        if N == 0 or len(labels) != N:
            raise ValueError("DeviceAugment: needs as many labels as images, at least one")
        dev = images[0].device
        sizes = []
        for im, lb in zip(images, labels):
            if not (im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and lb.dtype == torch.uint8
                    and tuple(lb.shape) == tuple(im.shape[:2]) and im.device == dev and lb.device == dev):
                raise ValueError("DeviceAugment: images are uint8 (H, W, 3), labels uint8 (H, W), all on one device")
            sizes.append((int(im.shape[0]), int(im.shape[1])))
        if params is None:
            params = self.draw(sizes, rng)
        if len(params) != N:
            raise ValueError("DeviceAugment: one SampleParams per sample")
        limits = self._check(sizes, params)
        if seed is None:
            seed = (self._seed + self._calls) & ((1 << 64) - 1)
        self._calls += 1
        if noise is not None and (tuple(noise.shape) != (N, self.th, self.tw, 3) or noise.dtype != torch.float32 or noise.device != dev
                                  or not noise.is_contiguous()):
            raise ValueError(f"DeviceAugment: noise must be dense fp32 {(N, self.th, self.tw, 3)} on the images' device")
        im_out, lb_out = out if out is not None else (None, None)
        im_out = self._out(im_out, (N, 3, self.th, self.tw), torch.float32, dev)
        lb_out = self._out(lb_out, (N, self.th, self.tw), torch.int64, dev)
        if dev.type == "cuda":
            u8 = self._run_device(images, labels, sizes, params, limits, int(seed), noise, im_out, lb_out, return_uint8)
        else:
            u8 = self._run_host(images, labels, sizes, params, int(seed), noise, im_out, lb_out)
        return (im_out, lb_out, u8) if return_uint8 else (im_out, lb_out)

    @staticmethod
    def _out(t, shape, dtype, dev):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if not (tuple(t.shape) == shape and t.dtype == dtype and t.device == dev and t.is_contiguous()):
            raise ValueError(f"DeviceAugment: out tensor must be dense {dtype} {shape} on {dev}")
        return t

    # ------------------------------------------------------------------ device path

    def _run_device(self, images, labels, sizes, params, limits, seed, noise, im_out, lb_out, return_uint8):
        lib = _lib.load()
        N, th, tw = len(images), self.th, self.tw
        dev = images[0].device
        images = [t.contiguous() for t in images]
        labels = [t.contiguous() for t in labels]
        im_ptrs, lb_ptrs = [t.data_ptr() for t in images], [t.data_ptr() for t in labels]
        if self.aerial:
            with torch.cuda.device(dev):
                im_ptrs, lb_ptrs = self._device_warp(lib, dev, im_ptrs, lb_ptrs, sizes, params)
            sizes = [self._scale_source(s, p) for s, p in zip(sizes, params)]
        if not lib.cabinet_augment_supported(th, tw, *limits):   # the batch's own figures: the library's word on coverage
            _lib.check(-2, "cabinet_augment_supported")
        table = torch.from_numpy(self.build_table(im_ptrs, lb_ptrs, sizes, params)).to(dev)
        need = int(lib.cabinet_augment_workspace_bytes(N, th, tw))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)  # from torch's stream-ordered cache: no device allocation per call
        u8 = torch.empty((N, th, tw, 3), dtype=torch.uint8, device=dev) if return_uint8 else None
        m3, s3 = (_ct.c_float * 3)(*self.mean), (_ct.c_float * 3)(*self.std)
        with torch.cuda.device(dev):
            rc = lib.cabinet_augment_batch(table.data_ptr(), N, th, tw, noise.data_ptr() if noise is not None else None, seed,
                                           _ct.addressof(m3), _ct.addressof(s3), im_out.data_ptr(), lb_out.data_ptr(),
                                           u8.data_ptr() if u8 is not None else None, ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "cabinet_augment_batch")
        return u8

    def _buffer(self, dev, name, nbytes):
        """A cached, grow-only uint8 device buffer: the passes of consecutive calls on one stream reuse it in stream order."""
        buf = self._buffers.get((dev, name))
        if buf is None or buf.numel() < nbytes:
            buf = self._buffers[(dev, name)] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        return buf

    def warp_stages(self, dev, im_ptrs, lb_ptrs, sizes, params):
        """The launches of the aerial geometry for a batch: resize where ResizeIfLarger acts, translate with the flips, rotate
        where the angle is no copy -- at most one launch per pass for the whole batch, into cached device buffers.  Returns
        ([(pass name, entry point name, descriptor block on the device, count, max_out_h, max_out_w, items)], image addresses,
        label addresses): the addresses of each sample's warped image and label."""
        plans = [self.warp_plan(s, p) for s, p in zip(sizes, params)]
        im_ptrs, lb_ptrs = list(im_ptrs), list(lb_ptrs)
        translate = lambda st: "a" in st and st["a"][1] == 0 and st["a"][3] == 0  # noqa: E731
        passes = (("resize", lambda st: st.get("resize"), "cabinet_augment_resize_batch"), ("translate", translate, "cabinet_augment_warp_batch"),
                  ("rotate", lambda st: "a" in st and not translate(st), "cabinet_augment_warp_batch"))
        stages = []
        for name, mine, entry in passes:
            todo = [(i, st) for i, plan in enumerate(plans) for st in plan if mine(st)]
            if not todo:
                continue
            base = self._buffer(dev, name, sum(4 * st["out_h"] * st["out_w"] for _, st in todo)).data_ptr()
            items, off = [], 0
            for i, st in todo:
                px = st["out_h"] * st["out_w"]
                items.append(dict(st, src_image=im_ptrs[i], src_label=lb_ptrs[i], dst_image=base + off, dst_label=base + off + 3 * px))
                im_ptrs[i], lb_ptrs[i] = base + off, base + off + 3 * px
                off += 4 * px
            descs = torch.from_numpy(warp_descs(items)).to(dev)
            stages.append((name, entry, descs, len(items), max(st["out_h"] for _, st in todo), max(st["out_w"] for _, st in todo), items))
        return stages, im_ptrs, lb_ptrs

    def _device_warp(self, lib, dev, im_ptrs, lb_ptrs, sizes, params):
        """Runs warp_stages on the current stream; the library's word on coverage first."""
        for s, p in zip(sizes, params):
            ratio = max(s[0] / p.resized[0], s[1] / p.resized[1]) if p.resized is not None else 0.0
            if not lib.cabinet_augment_warp_supported(s[0], s[1], p.warped[0], p.warped[1], float(p.angle), float(ratio)):
                _lib.check(-2, "cabinet_augment_warp_supported")
        stages, im_ptrs, lb_ptrs = self.warp_stages(dev, im_ptrs, lb_ptrs, sizes, params)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for _, entry, descs, n, max_h, max_w, _ in stages:
            _lib.check(getattr(lib, entry)(descs.data_ptr(), n, max_h, max_w, stream), entry)
        return im_ptrs, lb_ptrs

    def build_table(self, image_ptrs, label_ptrs, sizes, params) -> np.ndarray:
        """The batch's device table as host bytes (include/cabinet_hip.h, cabinet_augment_batch): N entries, then each sample's
        column taps, row taps, label column and label row indices, 16-byte aligned, named by byte offset."""
        N, th, tw = len(sizes), self.th, self.tw
        a16 = lambda v: (v + 15) & ~15  # noqa: E731
        per = a16(tw * 32) + a16(th * 32) + a16(tw * 4) + a16(th * 4)
        head = a16(N * SAMPLE_DTYPE.itemsize)
        hsv_at = head + N * per   # the 768-byte H, S, V tables of the samples with RandomHSV, behind everything else
        n_hsv = sum(p.hsv is not None for p in params)
        blob = np.zeros(hsv_at + n_hsv * 768, dtype=np.uint8)
        entries = blob[:N * SAMPLE_DTYPE.itemsize].view(SAMPLE_DTYPE)
        for i, (size, p) in enumerate(zip(sizes, params)):
            ct, rt, lc, lr = self._sample_tables(size, p)
            off = head + i * per
            e = entries[i]
            e["image"], e["label"], e["H"], e["W"] = image_ptrs[i], label_ptrs[i], size[0], size[1]
            for name, arr in (("col_taps", ct), ("row_taps", rt), ("lab_col", lc), ("lab_row", lr)):
                raw = arr.view(np.uint8).reshape(-1)
                blob[off:off + raw.size] = raw
                e[name] = off
                off += a16(raw.size)
            self._fill_entry(e, p)
            if p.hsv is not None:
                blob[hsv_at:hsv_at + 768] = hsv_tables(*p.hsv).reshape(-1)
                e["flags"] |= FLAG_HSV
                e["reserved"] = hsv_at
                hsv_at += 768
        return blob

    def _fill_entry(self, e, p: SampleParams):
        e["brightness"], e["contrast"], e["saturation"] = p.brightness, p.contrast, p.saturation
        flags = (FLAG_GRAY if p.gray else 0) | (FLAG_GAMMA if p.gamma is not None else 0) | (FLAG_NOISE if p.noise else 0)
        if p.cutout is not None:
            flags |= FLAG_CUTOUT
            e["cut_y"], e["cut_x"] = p.cutout
        e["cut_size"] = self.cutout_size
        e["flags"] = flags
        e["noise_scale"] = self.noise_sigma * 255
        e["ignore_label"] = self.ignore_label
        e["gamma_lut"] = self.gamma_lut(p.gamma)
        e["label_lut"] = self.label_lut

    # ------------------------------------------------------------------ host path (numpy; same tables, same arithmetic)

    @staticmethod
    def _apply_taps(src, taps, axis):
        """One pass of the resample along ``axis`` of uint8 ``src``: clip8((2^21 + sum coef * pixel) >> 22)."""
        n_in = src.shape[axis]
        acc = None
        for k in range(MAX_TAPS):
            idx = np.clip(taps["first"] + taps["step"] * k, 0, n_in - 1)
            coef = np.where(k < taps["n"], taps["coef"][:, k], 0).astype(np.int64)
            shape = [1, 1, 1]
            shape[axis] = -1
            term = np.take(src, idx, axis=axis).astype(np.int64) * coef.reshape(shape)
            acc = term if acc is None else acc + term
        return np.clip((acc + (1 << (_PRECISION_BITS - 1))) >> _PRECISION_BITS, 0, 255).astype(np.uint8)

    @staticmethod
    def _luma(a):
        a = a.astype(np.int64)
        return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)

    @staticmethod
    def _blend(deg, src, r):
        """Pillow's Image.blend(deg, src, r) in fp32, every operation rounded on its own."""
        r32 = np.float32(r)
        d, s = deg.astype(np.float32), src.astype(np.float32)
        t = d + r32 * (s - d)
        if 0.0 <= r32 <= 1.0:
            return t.astype(np.uint8)
        return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.uint8))).astype(np.uint8)

    def _host_warp(self, image, label, size, p: SampleParams):
        """The aerial geometry in numpy, pass by pass as the device runs it (warp_plan)."""
        for st in self.warp_plan(size, p):
            if st.get("resize"):
                (ct, lc), (rt, lr) = _resize_axis(st["W"], st["out_w"]), _resize_axis(st["H"], st["out_h"])
                image = self._apply_taps(self._apply_taps(image, ct, 1), rt, 0)
                label = label[lr[:, None], lc[None, :]]
            else:
                image, label = (affine_image(image, st["a"], st["out_w"], st["out_h"], st["flip"]),
                                affine_label(label, st["a"], st["out_w"], st["out_h"], st["fill"], st["flip"]))
        return image, label

    def _host_sample(self, image, label, size, p: SampleParams, noise, seed, index):
        if self.aerial:
            image, label = self._host_warp(image, label, size, p)
            size = self._scale_source(size, p)
        ct, rt, lc, lr = self._sample_tables(size, p)
        used = np.zeros(size[0], dtype=bool)   # the horizontal pass runs over the source rows the vertical one reads
        for k in range(MAX_TAPS):
            used[np.clip(rt["first"] + rt["step"] * k, 0, size[0] - 1)[k < rt["n"]]] = True
        rows = np.flatnonzero(used)
        remap = np.zeros(size[0], dtype=np.int64)
        remap[rows] = np.arange(rows.size)
        hor = self._apply_taps(image[rows], ct, 1)
        rt2 = rt.copy()
        # taps of one output row are consecutive source rows, all of them used: their positions in `rows` are consecutive too
        rt2["first"] = remap[np.clip(rt["first"], 0, size[0] - 1)]
        im = self._apply_taps(hor, rt2, 0)
        if p.hsv is not None:
            im = apply_hsv(im, hsv_tables(*p.hsv))
        lb = np.where((lr[:, None] < 0) | (lc[None, :] < 0), -1, 0)
        src_lb = label[np.clip(lr, 0, None)[:, None], np.clip(lc, 0, None)[None, :]]
        lb = np.where(lb < 0, self.ignore_label, self.label_lut[src_lb]).astype(np.int64)
        im = self._blend(np.zeros_like(im), im, p.brightness)
        L = self._luma(im)
        m = int(int(L.astype(np.int64).sum()) / (self.th * self.tw) + 0.5)
        im = self._blend(np.full_like(im, m), im, p.contrast)
        im = self._blend(np.repeat(self._luma(im)[..., None], 3, axis=2), im, p.saturation)
        if p.gray:
            im = np.repeat(self._luma(im)[..., None], 3, axis=2)
        if p.gamma is not None:
            im = self.gamma_lut(p.gamma)[im]
        if p.noise:
            if noise is None:
                nz = np.random.default_rng([seed, index]).standard_normal(im.shape).astype(np.float32) * np.float32(self.noise_sigma * 255)
            else:
                nz = noise
            im = np.clip(im.astype(np.float64) + nz.astype(np.float64), 0, 255).astype(np.uint8)
        if p.cutout is not None:
            y, x = p.cutout
            im = im.copy()
            im[y:y + self.cutout_size, x:x + self.cutout_size, :] = 0
        return im, lb

    def _run_host(self, images, labels, sizes, params, seed, noise, im_out, lb_out):
        N = len(images)
        u8 = np.empty((N, self.th, self.tw, 3), dtype=np.uint8)
        mean, std = np.asarray(self.mean, dtype=np.float32), np.asarray(self.std, dtype=np.float32)
        for i in range(N):
            nz = noise[i].numpy() if noise is not None else None
            u8[i], lb = self._host_sample(images[i].numpy(), labels[i].numpy(), sizes[i], params[i], nz, seed, i)
            lb_out[i].copy_(torch.from_numpy(lb))
        f = (u8.astype(np.float32) / np.float32(255.0) - mean) / std
        im_out.copy_(torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2))))
        return torch.from_numpy(u8)
