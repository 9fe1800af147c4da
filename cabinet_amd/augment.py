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

Routing: device tensors take the kernels and never fall back (a shape the kernels refuse raises); host tensors take the numpy
path below, which uses the same tables and the same arithmetic.
"""

from __future__ import annotations

import ctypes as _ct
import random as _random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["DeviceAugment", "SampleParams", "resample_taps", "nearest_index", "MAX_TAPS"]

MAX_TAPS = 5
MAX_RATIO = 2.5                  # resize ratio in/out per axis: five taps at most, and fewer than 17 * 2.5 + 1 source rows per tile
TILE_ROWS, TILE_SPAN = 16, 48    # csrc/augment.hip: output rows of a workgroup tile, source rows it stages
_TABLE_CACHE = 32                # axis tables kept (Cityscapes' six scales need twelve); continuous scales evict the oldest
_PRECISION_BITS = 22
FLAG_GRAY, FLAG_GAMMA, FLAG_NOISE, FLAG_CUTOUT = 1, 2, 4, 8

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
assert SAMPLE_DTYPE.itemsize == 2400 and TAP_DTYPE.itemsize == 32


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


class DeviceAugment(object):
    """The reference's train-time transform for batches; see the module docstring.  ``cropsize`` is (target_w, target_h), the
    order of the reference's RandomCrop.  ``brightness`` / ``contrast`` / ``saturation`` are the reference's jitter widths
    (``v`` -> uniform(max(1 - v, 0), 1 + v)) or None.  ``label_map``: 256 entries id -> trainId, or None for the identity."""

    def __init__(self, cropsize, ignore_label=255, label_map=None, scales=(1.0,), continuous=False, flip_p=0.5, brightness=None,
                 contrast=None, saturation=None, grayscale_p=0.0, gamma_range=(0.7, 1.5), gamma_p=0.0, noise_sigma=0.05,
                 noise_p=0.0, cutout_p=0.0, cutout_size=64, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), seed=None):
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
        self.grayscale_p, self.gamma_range, self.gamma_p = float(grayscale_p), tuple(gamma_range), float(gamma_p)
        self.noise_sigma, self.noise_p = float(noise_sigma), float(noise_p)
        self.cutout_p, self.cutout_size = float(cutout_p), int(cutout_size)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self._seed = _random.SystemRandom().getrandbits(63) if seed is None else int(seed)
        self._calls = 0
        self._tables = {}

    @classmethod
    def cityscapes(cls, cropsize=(1024, 1024), ignore_label=255, label_map=None, **overrides):
        """The reference's default Cityscapes train pipeline (src/datasets/cityscapes.py:114-136)."""
        kw = dict(scales=(0.75, 1.0, 1.25, 1.5, 1.75, 2.0), flip_p=0.5, brightness=0.5, contrast=0.5, saturation=0.5,
                  grayscale_p=0.2, gamma_range=(0.8, 1.2), gamma_p=0.3, noise_sigma=0.03, noise_p=0.3, cutout_p=0.3, cutout_size=64)
        kw.update(overrides)
        return cls(cropsize, ignore_label=ignore_label, label_map=label_map, **kw)

    # ------------------------------------------------------------------ parameters

    def draw(self, sizes: Sequence[Tuple[int, int]], rng=None) -> List[SampleParams]:
        """One SampleParams per (H, W) of ``sizes``, consuming ``rng`` (a ``random.Random``; None: the module-level generator)
        exactly as the reference's Compose consumes ``random``."""
        rng = _random if rng is None else rng
        out = []
        for H, W in sizes:
            flip = not (rng.random() > self.flip_p)
            scale = rng.uniform(*self.scales) if self.continuous else rng.choice(self.scales)
            w, h = int(round(W * scale)), int(round(H * scale))
            pw, ph = max(w, self.tw), max(h, self.th)
            sw = rng.randint(0, pw - self.tw) if pw > self.tw else 0
            sh = rng.randint(0, ph - self.th) if ph > self.th else 0
            rb = rng.uniform(*self.brightness) if self.brightness else 1.0
            rc = rng.uniform(*self.contrast) if self.contrast else 1.0
            rs = rng.uniform(*self.saturation) if self.saturation else 1.0
            gray = rng.random() < self.grayscale_p
            gamma = rng.uniform(*self.gamma_range) if rng.random() < self.gamma_p else None
            noise = rng.random() < self.noise_p
            cutout = None
            if rng.random() < self.cutout_p:
                y = rng.randint(0, self.th - self.cutout_size)
                x = rng.randint(0, self.tw - self.cutout_size)
                cutout = (y, x)
            out.append(SampleParams(flip, scale, w, h, sw, sh, rb, rc, rs, gray, gamma, noise, cutout))
        return out

    def supported(self, size: Tuple[int, int], p: SampleParams) -> bool:
        """Whether the kernels cover this sample: a resize ratio in/out of at most 2.5 per axis (scale >= 0.4), which is what
        bounds both the taps per output pixel (five) and the source rows a tile of the geometry kernel stages, and a reflect pad
        below the resized size.  Both routes refuse the same samples."""
        return self._limits(size, p)[0]

    def _limits(self, size, p: SampleParams):
        """(covered, taps, pad_y, pad_x) of one sample; the tap count is 0 where the ratio already rules the sample out."""
        H, W = size
        pad_y, pad_x = max(self.th - p.h, 0), max(self.tw - p.w, 0)
        if p.w < 1 or p.h < 1 or W > MAX_RATIO * p.w or H > MAX_RATIO * p.h:
            return False, 0, pad_y, pad_x
        taps = int(max(self._axis(W, p.w).n.max(), self._axis(H, p.h).n.max()))
        return bool(taps <= MAX_TAPS and pad_x <= p.w - 1 and pad_y <= p.h - 1), taps, pad_y, pad_x

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
        H, W = size
        if p.cutout is not None and not (0 <= p.cutout[0] <= self.th - self.cutout_size and 0 <= p.cutout[1] <= self.tw - self.cutout_size):
            raise ValueError("DeviceAugment: cutout square outside the crop")
        ct, lc = self._window(self._axis(W, p.w), W, p.w, p.sw, self.tw, p.flip)
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
            if not ok:
                raise RuntimeError(f"DeviceAugment: sample {i} (source {s[0]}x{s[1]}, resized {p.h}x{p.w}, crop {self.th}x{self.tw}) is "
                                   f"outside coverage: a resize ratio in/out <= {MAX_RATIO} per axis (scale >= 0.4, at most "
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
        if not lib.cabinet_augment_supported(th, tw, *limits):   # the batch's own figures: the library's word on coverage
            _lib.check(-2, "cabinet_augment_supported")
        table = torch.from_numpy(self.build_table([t.data_ptr() for t in images], [t.data_ptr() for t in labels], sizes, params)).to(dev)
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

    def build_table(self, image_ptrs, label_ptrs, sizes, params) -> np.ndarray:
        """The batch's device table as host bytes (include/cabinet_hip.h, cabinet_augment_batch): N entries, then each sample's
        column taps, row taps, label column and label row indices, 16-byte aligned, named by byte offset."""
        N, th, tw = len(sizes), self.th, self.tw
        a16 = lambda v: (v + 15) & ~15  # noqa: E731
        per = a16(tw * 32) + a16(th * 32) + a16(tw * 4) + a16(th * 4)
        head = a16(N * SAMPLE_DTYPE.itemsize)
        blob = np.zeros(head + N * per, dtype=np.uint8)
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

    def _host_sample(self, image, label, size, p: SampleParams, noise, seed, index):
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
