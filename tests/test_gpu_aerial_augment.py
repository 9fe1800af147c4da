"""The aerial datasets' train transform (K20) on the GPU: csrc/augment_warp.hip and the HSV epilogue of csrc/augment.hip against
the reference's own output (tests/golden/g13_aerial.npz) through DeviceAugment, and each pass alone through the raw C ABI against
the numpy route, which tests/test_aerial_augment.py holds against the reference and against Pillow.  All comparisons are exact."""
import dataclasses
import random

import numpy as np
import pytest
import torch

import aerial_golden as ag
from augment_golden import ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _check(cs, im, lb, u8, who):
    """The judgement of tests/test_gpu_augment.py::_check."""
    im, lb, u8 = im.cpu().numpy(), lb.cpu().numpy(), u8.cpu().numpy()
    for j, c in enumerate(cs):
        db, dl = int((u8[j] != c.u8).sum()), int((lb[j] != c.lb).sum())
        ulp = ulp_distance(im[j], c.f32)
        print(f"{who} case {c.index} source {c.size} crop {c.crop}: {db} differing bytes, {dl} differing labels, fp32 max {ulp} ulp")
        assert db == 0 and dl == 0, (who, c.index, db, dl)
        assert ulp <= 1, (who, c.index, ulp)   # bit equality is expected (two correctly rounded operations on both sides)


@pytest.mark.parametrize("crop", ag.crops())
def test_fixture_through_device_augment(crop):
    """One batch per crop size: sources of different sizes, resized and unresized, in one batch.  Twice, so that the second
    call runs in the cached pass buffers the first one left full."""
    aug, cs, images, labels, params, noise = ag.batch(crop, DEV)
    for rep in range(2):
        im, lb, u8 = aug(images, labels, params=params, noise=noise, return_uint8=True)
        assert im.is_cuda and im.dtype == torch.float32 and lb.dtype == torch.int64
        _check(cs, im, lb, u8, f"DeviceAugment call {rep}")


def _run_pass(entry, items):
    """One launch of cabinet_augment_warp_batch / _resize_batch for ``items`` (dicts of warp_descs without addresses, plus the
    host arrays ``image`` and ``label``): every output at an ODD byte offset inside one 0xFF-filled allocation.  Returns the
    outputs [(image, label)] and asserts that no byte outside them moved."""
    from cabinet_amd import _lib
    from cabinet_amd.augment import warp_descs

    lib = _lib.load()
    keep, descs, spans, off = [], [], [], 1
    for it in items:
        src_im, src_lb = torch.from_numpy(it["image"]).to(DEV), torch.from_numpy(it["label"]).to(DEV)
        keep.append((src_im, src_lb))
        px = it["out_h"] * it["out_w"]
        a, b = off, (off + 3 * px + 6) | 1
        spans.append((a, b, px))
        off = (b + px + 4) | 1
        descs.append(dict({k: v for k, v in it.items() if k not in ("image", "label")}, src_image=src_im.data_ptr(), src_label=src_lb.data_ptr()))
    big = torch.full((off + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    for d, (a, b, px) in zip(descs, spans):
        d["dst_image"], d["dst_label"] = big.data_ptr() + a, big.data_ptr() + b
    table = torch.from_numpy(warp_descs(descs)).to(DEV)
    rc = getattr(lib, entry)(table.data_ptr(), len(items), max(it["out_h"] for it in items), max(it["out_w"] for it in items),
                             torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    owned = np.zeros(got.size, dtype=bool)
    outs = []
    for it, (a, b, px) in zip(items, spans):
        owned[a:a + 3 * px] = True
        owned[b:b + px] = True
        outs.append((got[a:a + 3 * px].reshape(it["out_h"], it["out_w"], 3), got[b:b + px].reshape(it["out_h"], it["out_w"])))
    assert bool((got[~owned] == 0xFF).all()), "a byte outside the outputs moved"
    return outs


SOURCES = [(1, 7), (7, 1), (5, 1), (1, 5), (33, 61), (72, 40), (97, 200)]   # (H, W)
FILL = 255


def _source(size):
    gen = np.random.RandomState(size[0] * 1000 + size[1])
    return gen.randint(0, 256, size=size + (3,)).astype(np.uint8), gen.randint(0, 200, size=size).astype(np.uint8)


def _compare(items, outs, what):
    from cabinet_amd.augment import affine_image, affine_label

    bad = 0
    for it, (gi, gl) in zip(items, outs):
        wi = affine_image(it["image"], it["a"], it["out_w"], it["out_h"], it["flip"])
        wl = affine_label(it["label"], it["a"], it["out_w"], it["out_h"], it["fill"], it["flip"])
        db, dl = int((gi != wi).sum()), int((gl != wl).sum())
        if db or dl:
            bad += 1
            print(f"{what} a={it['a']} flip={it['flip']}: {db} differing bytes, {dl} differing labels")
    assert bad == 0, (what, bad, len(items))


@pytest.mark.parametrize("size", SOURCES)
def test_translate_pass_alone(size):
    """dx, dy in {0, an exact integer, +-0.05 size, +-size (everything fill)} x all four flips, one launch.  The allocation is
    0xFF beforehand, so the zero fill of the image is the kernel's own."""
    H, W = size
    image, label = _source(size)
    items = [dict(image=image, label=label, H=H, W=W, out_h=H, out_w=W, a=(1, 0, dx, 0, 1, dy), flip=flip, fill=FILL)
             for flip in range(4) for dx in (0.0, 3.0, 0.05 * W, -0.05 * W, float(W), -float(W))
             for dy in (0.0, 3.0, 0.05 * H, -0.05 * H, float(H), -float(H))]
    outs = _run_pass("cabinet_augment_warp_batch", items)
    _compare(items, outs, f"translate {size}")
    whole = [o for it, o in zip(items, outs) if abs(it["a"][2]) == W or abs(it["a"][5]) == H]
    assert whole and all(not gi.any() and bool((gl == FILL).all()) for gi, gl in whole)


@pytest.mark.parametrize("size", SOURCES)
def test_rotate_pass_alone(size):
    """Angles +-0.5, +-10, 30, +-45 x all four flips, expand=True: outputs of different sizes in one launch."""
    from cabinet_amd.augment import rotate_matrix

    H, W = size
    image, label = _source(size)
    items = []
    for flip in range(4):
        for angle in (0.5, -0.5, 10.0, -10.0, 30.0, 45.0, -45.0):
            m, nw, nh = rotate_matrix(W, H, angle)
            items.append(dict(image=image, label=label, H=H, W=W, out_h=nh, out_w=nw, a=m, flip=flip, fill=FILL))
    assert len({(it["out_h"], it["out_w"]) for it in items}) > 1
    _compare(items, _run_pass("cabinet_augment_warp_batch", items), f"rotate {size}")


def test_resize_pass_alone():
    """97 x 200 -> 47 x 96 and 200 x 97 -> 96 x 47 (ResizeIfLarger(96), ratio 2.08), and 120 x 50 -> 48 x 20, the 2.5 edge, whose
    tiles of 16 output rows stage 42-43 source rows; one launch."""
    from cabinet_amd.augment import DeviceAugment, resample_taps

    first, n, _ = resample_taps(120, 48)
    spans = [int(first[min(j + 15, 47)] + n[min(j + 15, 47)] - first[j]) for j in range(0, 48, 16)]
    assert max(spans) in (42, 43), spans
    items, want = [], []
    aug = DeviceAugment.uavid(cropsize=(8, 8), cutout_size=8)
    for (H, W), (oh, ow) in (((97, 200), (47, 96)), ((200, 97), (96, 47)), ((120, 50), (48, 20))):
        image, label = _source((H, W))
        items.append(dict(image=image, label=label, H=H, W=W, out_h=oh, out_w=ow, resize=True))
        aug.max_size = max(oh, ow)
        p = dataclasses.replace(aug.draw([(H, W)], random.Random(0))[0], flip=False, vflip=False, dx=0.0, dy=0.0, angle=0.0, warped=(oh, ow))
        assert p.resized == (oh, ow)
        want.append(aug._host_warp(image, label, (H, W), p))   # the resize, then an identity translate
    outs = _run_pass("cabinet_augment_resize_batch", items)
    for it, (gi, gl), (wi, wl) in zip(items, outs, want):
        db, dl = int((gi != wi).sum()), int((gl != wl).sum())
        print(f"resize {it['H']}x{it['W']} -> {it['out_h']}x{it['out_w']}: {db} differing bytes, {dl} differing labels")
        assert db == 0 and dl == 0


_colour_cache = {}


def _all_colours():
    """All 2^24 colours as (16, 1024, 1024, 3), and their HSV bytes by the numpy route (computed once)."""
    if not _colour_cache:
        from cabinet_amd.augment import rgb_to_hsv

        v = np.arange(1 << 24, dtype=np.uint32)
        rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(16, 1024, 1024, 3)
        _colour_cache["rgb"] = rgb
        _colour_cache["hsv"] = np.concatenate([rgb_to_hsv(rgb[i:i + 4]) for i in range(0, 16, 4)])
    return _colour_cache["rgb"], _colour_cache["hsv"]


@pytest.mark.parametrize("gains", [(-0.009, 0.31, -0.2), (0.0071, -0.4, 0.3)])
def test_hsv_on_every_colour(gains):
    """All 2^24 colours as 16 samples of 1024 x 1024, crop 1024 x 1024, no geometry and no other photometric step: the final
    bytes equal the numpy route's RGB -> HSV -> tables -> RGB on every colour."""
    from cabinet_amd.augment import DeviceAugment, hsv_tables, hsv_to_rgb

    rgb, hsv = _all_colours()
    aug = DeviceAugment((1024, 1024), scales=(1.0,), flip_p=0.0, hsv=(0.01, 0.4, 0.3))
    params = [dataclasses.replace(p, hsv=gains) for p in aug.draw([(1024, 1024)] * 16, random.Random(0))]
    assert all(not p.flip and (p.w, p.h, p.sw, p.sh) == (1024, 1024, 0, 0) and (p.brightness, p.contrast, p.saturation) == (1.0, 1.0, 1.0)
               and not p.gray and p.gamma is None and not p.noise and p.cutout is None for p in params)
    images = [torch.from_numpy(rgb[i]).to(DEV) for i in range(16)]
    label = torch.zeros((1024, 1024), dtype=torch.uint8, device=DEV)
    got = aug(images, [label] * 16, params=params, return_uint8=True)[2].cpu().numpy()
    t = hsv_tables(*gains)
    diff = 0
    for i in range(0, 16, 4):
        h = hsv[i:i + 4]
        want = hsv_to_rgb(np.stack([t[0][h[..., 0]], t[1][h[..., 1]], t[2][h[..., 2]]], axis=-1))
        diff += int((got[i:i + 4] != want).any(axis=-1).sum())
    print(f"gains {gains}: {diff} of {1 << 24} colours differ")
    assert diff == 0


def test_contrast_mean_is_taken_after_hsv():
    """A value gain of -0.3 moves the mean luma of the crop by far more than 1, and the contrast blend (factor 0.6) pulls every
    byte toward that mean: device equals host, and a mean taken from the unconverted crop would give other bytes."""
    from cabinet_amd.augment import DeviceAugment, apply_hsv, hsv_tables

    gen = np.random.RandomState(9)
    image = gen.randint(0, 256, size=(80, 96, 3)).astype(np.uint8)
    label = gen.randint(0, 19, size=(80, 96)).astype(np.uint8)
    aug = DeviceAugment((96, 80), scales=(1.0,), flip_p=0.0, contrast=0.5, hsv=(0.01, 0.4, 0.3))
    p = dataclasses.replace(aug.draw([(80, 96)], random.Random(1))[0], hsv=(0.004, 0.2, -0.3), contrast=0.6)
    luma = lambda a: float(DeviceAugment._luma(a).astype(np.float64).mean())  # noqa: E731
    before, after = luma(image), luma(apply_hsv(image, hsv_tables(*p.hsv)))
    assert abs(before - after) >= 1, (before, after)
    want = aug([torch.from_numpy(image)], [torch.from_numpy(label)], params=[p], return_uint8=True)
    got = aug([torch.from_numpy(image).to(DEV)], [torch.from_numpy(label).to(DEV)], params=[p], return_uint8=True)
    assert int((got[2].cpu() != want[2]).sum()) == 0 and int((got[1].cpu() != want[1]).sum()) == 0
    assert ulp_distance(got[0].cpu().numpy(), want[0].numpy()) <= 1
    # the same blend against the mean of the UNCONVERTED crop differs, so the comparison above can tell the two apart
    m_wrong = int(DeviceAugment._luma(image).astype(np.int64).sum() / (80 * 96) + 0.5)
    conv = apply_hsv(image, hsv_tables(*p.hsv))
    assert not np.array_equal(DeviceAugment._blend(np.full_like(conv, m_wrong), conv, p.contrast), want[2][0].numpy())


def test_mixup_on_the_device_is_bit_equal_to_the_cpu():
    from cabinet_amd.augment import DeviceAugment

    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((2, 3, 70, 130), generator=g), torch.randn((2, 3, 70, 130), generator=g)
    la, lb = torch.zeros((2, 70, 130), dtype=torch.int64), torch.ones((2, 70, 130), dtype=torch.int64)
    for r in (0.37, 0.5, 0.61):
        want_im, want_lb = a * r + b * (1.0 - r), (la if r >= 0.5 else lb)
        im, lab = DeviceAugment.mixup(a.to(DEV), la.to(DEV), b.to(DEV), lb.to(DEV), r)
        assert im.is_cuda and torch.equal(im.cpu().view(torch.int32), want_im.view(torch.int32))
        assert torch.equal(lab.cpu(), want_lb)


def test_device_path_refuses_what_the_host_path_refuses():
    from cabinet_amd.augment import DeviceAugment

    im, lb = torch.zeros((40, 300, 3), dtype=torch.uint8, device=DEV), torch.zeros((40, 300), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="outside coverage: ResizeIfLarger"):
        DeviceAugment.uavid(cropsize=(16, 16), max_size=100, cutout_size=8)([im], [lb], rng=random.Random(0))
