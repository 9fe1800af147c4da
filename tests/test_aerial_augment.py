"""The aerial datasets' train transform (K20) on the CPU tier: cabinet_amd.augment's numpy route against the reference's own output
(tests/golden/g13_aerial.npz), its restatements of Pillow's affine transform and HSV conversions against Pillow itself, the
order in which draw() consumes the generator, compatibility with K18, and the argument checks of the new entry points."""
import math
import random

import numpy as np
import pytest
import torch

import aerial_golden as ag


def _pil():
    Image = pytest.importorskip("PIL.Image")
    return Image


@pytest.mark.parametrize("i", range(len(ag.cases())))
def test_host_path_reproduces_the_reference(i):
    """From draw(random.Random(k)) alone: 0 differing bytes, 0 differing labels, the fp32 tensor bit for bit."""
    c = ag.cases()[i]
    aug = ag.augmenter(c.crop)
    noise = None if c.noise is None else torch.from_numpy(c.noise)[None]
    im, lb, u8 = aug([torch.from_numpy(c.image)], [torch.from_numpy(c.label)], rng=random.Random(c.seed), noise=noise, return_uint8=True)
    db, dl = int((u8[0].numpy() != c.u8).sum()), int((lb[0].numpy() != c.lb).sum())
    print(f"case {i} source {c.size} crop {c.crop} seed {c.seed}: {db} differing bytes, {dl} differing labels")
    assert db == 0 and dl == 0
    assert np.array_equal(im[0].numpy().view(np.int32), c.f32.view(np.int32))


@pytest.mark.parametrize("crop", ag.crops())
def test_host_batch_mixes_sources_and_replays_params(crop):
    aug, cs, images, labels, params, noise = ag.batch(crop)
    im, lb, u8 = aug(images, labels, params=params, noise=noise, return_uint8=True)
    for j, c in enumerate(cs):
        assert np.array_equal(u8[j].numpy(), c.u8) and np.array_equal(lb[j].numpy(), c.lb)
        assert np.array_equal(im[j].numpy().view(np.int32), c.f32.view(np.int32))


def test_fixture_holds_every_branch_and_names_its_pillow():
    assert ag.pillow_version().split(".")[0].isdigit()
    seen = set()
    for c in ag.cases():
        aug = ag.augmenter(c.crop)
        p = aug.draw([c.size], random.Random(c.seed))[0]
        assert aug.supported(c.size, p)
        tw, th = c.crop
        seen |= {f"h{int(p.flip)}", f"v{int(p.vflip)}", f"dx{int(p.dx > 0)}", f"dy{int(p.dy > 0)}", f"rot{int(p.angle > 0)}",
                 f"scale{int(p.scale > 1)}", f"pad{int(p.w < tw)}{int(p.h < th)}", f"hue{np.sign(round(p.hsv[0] * 255)):+.0f}",
                 f"sat{int(p.hsv[1] > 0)}", f"val{int(p.hsv[2] > 0)}", f"resized{int(p.resized is not None)}_{c.crop}"}
        seen |= {"both"} if p.flip and p.vflip else set()
        seen |= {"gamma"} if p.gamma is not None else set()
        seen |= {"noise"} if p.noise else set()
        seen |= {"seams_rotated"} if tw > 64 and p.angle != 0 else set()
        if p.cutout is not None:
            seen |= {"cut_top"} if p.cutout[0] == 0 else set()
            seen |= {"cut_bottom"} if p.cutout[0] + 8 == th else set()
    want = {"h0", "h1", "v0", "v1", "both", "dx0", "dx1", "dy0", "dy1", "rot0", "rot1", "scale0", "scale1", "pad00", "pad10", "pad01",
            "pad11", "hue-1", "hue+0", "hue+1", "sat0", "sat1", "val0", "val1", "gamma", "noise", "seams_rotated", "cut_top",
            "cut_bottom", "resized1_(48, 40)", "resized0_(48, 40)"}
    assert want <= seen, sorted(want - seen)


def test_draw_consumes_the_generator_in_the_references_order():
    from cabinet_amd.augment import DeviceAugment, resize_if_larger, rotate_matrix

    aug = DeviceAugment.uavid(cropsize=(48, 40), cutout_size=8)
    r = random.Random(11)
    p = aug.draw([(97, 200)], r)[0]
    q = random.Random(11)
    H, W = resize_if_larger(97, 200, 96)
    assert (H, W) == (47, 96) == p.resized
    flip, vflip = not (q.random() > 0.5), not (q.random() > 0.2)
    dx, dy = q.uniform(-0.05, 0.05) * W, q.uniform(-0.05, 0.05) * H
    angle = q.uniform(-10.0, 10.0)
    _, nw, nh = rotate_matrix(W, H, angle)
    scale = q.uniform(0.7, 1.3)
    w, h = int(round(nw * scale)), int(round(nh * scale))
    sw = q.randint(0, max(w, 48) - 48) if max(w, 48) > 48 else 0
    sh = q.randint(0, max(h, 40) - 40) if max(h, 40) > 40 else 0
    hsv = tuple(q.uniform(-1, 1) * g for g in (0.01, 0.4, 0.3))
    rc = q.uniform(0.5, 1.5)
    gamma = q.uniform(0.8, 1.2) if q.random() < 0.3 else None
    noise = q.random() < 0.3
    cut = (q.randint(0, 40 - 8), q.randint(0, 48 - 8)) if q.random() < 0.3 else None
    assert (p.flip, p.vflip, p.dx, p.dy, p.angle, p.warped, p.scale, p.w, p.h, p.sw, p.sh, p.hsv, p.contrast, p.gamma, p.noise, p.cutout) \
        == (flip, vflip, dx, dy, angle, (nh, nw), scale, w, h, sw, sh, hsv, rc, gamma, noise, cut)
    assert (p.brightness, p.saturation, p.gray) == (1.0, 1.0, False)
    assert r.random() == q.random()
    # all-zero HSV gains: the reference draws nothing for the step
    r, q = random.Random(3), random.Random(3)
    a0 = DeviceAugment.uavid(cropsize=(48, 40), cutout_size=8, augmentation=dict(hsv_h=0.0, hsv_s=0.0, hsv_v=0.0))
    a1 = DeviceAugment.uavid(cropsize=(48, 40), cutout_size=8)
    p0, p1 = a0.draw([(33, 61)], r)[0], a1.draw([(33, 61)], q)[0]
    assert p0.hsv is None and p1.hsv is not None and (p0.sw, p0.sh) == (p1.sw, p1.sh) and p0.contrast != p1.contrast


def test_cityscapes_configuration_draws_exactly_as_before():
    """K18's draws, written out by hand: the state of the generator after draw() is the state after these."""
    from cabinet_amd.augment import SAMPLE_DTYPE, DeviceAugment, SampleParams

    aug = DeviceAugment.cityscapes(cropsize=(48, 40), cutout_size=8)
    assert not aug.aerial and aug.hsv is None
    r, q = random.Random(21), random.Random(21)
    ps = aug.draw([(40, 72), (33, 61)], r)
    for (H, W), p in zip([(40, 72), (33, 61)], ps):
        flip = not (q.random() > 0.5)
        scale = q.choice((0.75, 1.0, 1.25, 1.5, 1.75, 2.0))
        w, h = int(round(W * scale)), int(round(H * scale))
        sw = q.randint(0, max(w, 48) - 48) if max(w, 48) > 48 else 0
        sh = q.randint(0, max(h, 40) - 40) if max(h, 40) > 40 else 0
        rb, rc, rs = q.uniform(0.5, 1.5), q.uniform(0.5, 1.5), q.uniform(0.5, 1.5)
        gray = q.random() < 0.2
        gamma = q.uniform(0.8, 1.2) if q.random() < 0.3 else None
        noise = q.random() < 0.3
        cut = (q.randint(0, 32), q.randint(0, 40)) if q.random() < 0.3 else None
        assert p == SampleParams(flip, scale, w, h, sw, sh, rb, rc, rs, gray, gamma, noise, cut)
    assert r.getstate() == q.getstate()
    assert SAMPLE_DTYPE.itemsize == 2400
    table = aug.build_table([0x1000, 0x2000], [0x3000, 0x4000], [(40, 72), (33, 61)], ps)
    entries = table[:2 * 2400].view(SAMPLE_DTYPE)
    assert not (entries["flags"] & 16).any() and not entries["reserved"].any()


def test_presets_carry_each_datasets_constants():
    from cabinet_amd.augment import DeviceAugment

    u, v, a = DeviceAugment.uavid(), DeviceAugment.vdd(), DeviceAugment.aeroscapes()
    assert (u.mean, u.std) == ((0.480, 0.499, 0.457), (0.225, 0.208, 0.228))
    assert (v.mean, v.std) == ((0.486, 0.487, 0.441), (0.190, 0.178, 0.214))
    assert (a.mean, a.std) == ((0.439, 0.508, 0.460), (0.176, 0.157, 0.194))
    assert (a.tw, a.th, a.max_size) == (640, 640, 1280) and u.max_size == 2048
    for x in (u, v, a):
        assert (x.flip_p, x.vflip_p, x.translate, x.degrees, x.scales, x.hsv, x.mixup_p) == (0.5, 0.2, 0.05, 10.0, (0.7, 1.3), (0.01, 0.4, 0.3), 0.1)
        assert x.grayscale_p is None and x.contrast == (0.5, 1.5) and x.brightness is None and x.saturation is None
    b = DeviceAugment.aerial((64, 64), augmentation=dict(degrees=30.0, flipud=0.0, mixup=0.0))
    assert (b.degrees, b.vflip_p, b.mixup_p, b.max_size) == (30.0, 0.0, 0.0, 128)
    with pytest.raises(ValueError, match="unknown"):
        DeviceAugment.aerial((64, 64), augmentation=dict(mosaic=1.0))


def test_refusals_name_the_step():
    from cabinet_amd.augment import DeviceAugment

    im, lb = torch.zeros((40, 300, 3), dtype=torch.uint8), torch.zeros((40, 300), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="outside coverage: ResizeIfLarger"):     # 300 -> 100: ratio 3
        DeviceAugment.uavid(cropsize=(16, 16), max_size=100, cutout_size=8)([im], [lb], rng=random.Random(0))
    aug = DeviceAugment.uavid(cropsize=(16, 16), augmentation=dict(degrees=90.0), cutout_size=8)
    k = next(k for k in range(100) if abs(aug.draw([(40, 72)], random.Random(k))[0].angle) > 45)
    with pytest.raises(RuntimeError, match="outside coverage: RandomRotate"):
        aug([im[:, :72]], [lb[:, :72]], rng=random.Random(k))
    assert not aug.supported((40, 72), aug.draw([(40, 72)], random.Random(k))[0])
    with pytest.raises(RuntimeError, match="padding"):                               # 40 rows padded to 200
        DeviceAugment.uavid(cropsize=(16, 200), cutout_size=8)([im[:, :72]], [lb[:, :72]], rng=random.Random(0))


# --------------------------------------------------------------------------- against Pillow itself

def _pillow_affine(Image, img, lab, a, size, fill):
    return (np.array(Image.fromarray(img).transform(size, Image.AFFINE, a, resample=Image.BILINEAR)),
            np.array(Image.fromarray(lab).transform(size, Image.AFFINE, a, resample=Image.NEAREST, fillcolor=fill)))


SMALL = [(7, 1), (1, 5), (1, 7), (5, 1), (33, 61), (72, 40), (97, 200)]      # (H, W); 1 x 7 and 5 x 1 read either way round


@pytest.mark.parametrize("size", SMALL)
def test_translate_and_rotate_against_pillow_small(size):
    Image = _pil()
    from cabinet_amd.augment import affine_image, affine_label, rotate_matrix

    H, W = size
    gen = np.random.RandomState(H * 1000 + W)
    img, lab = gen.randint(0, 256, size=(H, W, 3)).astype(np.uint8), gen.randint(0, 200, size=(H, W)).astype(np.uint8)
    rnd = random.Random(H)
    shifts = [(0.0, 0.0), (3.0, -2.0), (0.05 * W, -0.05 * H), (-0.05 * W, 0.05 * H), (float(W), 0.0), (0.0, -float(H))]
    shifts += [(rnd.uniform(-0.05, 0.05) * W, rnd.uniform(-0.05, 0.05) * H) for _ in range(20)]
    for dx, dy in shifts:
        a = (1, 0, dx, 0, 1, dy)
        want = _pillow_affine(Image, img, lab, a, (W, H), 255)
        assert np.array_equal(affine_image(img, a, W, H), want[0]), (size, dx, dy)
        assert np.array_equal(affine_label(lab, a, W, H, 255), want[1]), (size, dx, dy)
    for angle in [0.5, -0.5, 10.0, -10.0, 30.0, 45.0, -45.0] + [rnd.uniform(-45, 45) for _ in range(20)]:
        m, nw, nh = rotate_matrix(W, H, angle)
        pim = Image.fromarray(img).rotate(angle, resample=Image.BILINEAR, expand=True)
        plb = Image.fromarray(lab).rotate(angle, resample=Image.NEAREST, expand=True, fillcolor=255)
        assert pim.size == (nw, nh), (size, angle)
        assert np.array_equal(affine_image(img, m, nw, nh), np.array(pim)), (size, angle)
        assert np.array_equal(affine_label(lab, m, nw, nh, 255), np.array(plb)), (size, angle)
    assert rotate_matrix(W, H, 0.0) is None and rotate_matrix(W, H, 360.0) is None


@pytest.mark.parametrize("size,angle", [((1152, 2048), -10.0), ((1536, 2048), 45.0), ((720, 1280), 7.3190245)])
def test_translate_and_rotate_against_pillow_at_working_sizes(size, angle):
    """The sizes the aerial datasets warp at: UAVid's 2160 x 3840 and VDD's 3000 x 4000 under the 2048 cap, AeroScapes' 720 x 1280."""
    Image = _pil()
    from cabinet_amd.augment import affine_image, affine_label, rotate_matrix

    H, W = size
    gen = np.random.RandomState(W + int(angle))
    img, lab = gen.randint(0, 256, size=(H, W, 3)).astype(np.uint8), gen.randint(0, 200, size=(H, W)).astype(np.uint8)
    a = (1, 0, 0.0371 * W, 0, 1, -0.0123 * H)
    want = _pillow_affine(Image, img, lab, a, (W, H), 255)
    assert np.array_equal(affine_image(img, a, W, H), want[0])
    assert np.array_equal(affine_label(lab, a, W, H, 255), want[1])
    m, nw, nh = rotate_matrix(W, H, angle)
    pim = Image.fromarray(img).rotate(angle, resample=Image.BILINEAR, expand=True)
    plb = Image.fromarray(lab).rotate(angle, resample=Image.NEAREST, expand=True, fillcolor=255)
    assert pim.size == (nw, nh)
    assert np.array_equal(affine_image(img, m, nw, nh), np.array(pim))
    assert np.array_equal(affine_label(lab, m, nw, nh, 255), np.array(plb))


def _colours():
    """Every colour with R in a stride-of-8 subset plus 255: (34, 65536, 3)."""
    r = np.asarray(list(range(0, 256, 8)) + [255], dtype=np.uint8)
    g = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack(np.meshgrid(r, g, g, indexing="ij"), axis=-1).reshape(r.size, 65536, 3))


def test_hsv_conversions_against_pillow():
    Image = _pil()
    from cabinet_amd.augment import apply_hsv, hsv_tables, hsv_to_rgb, rgb_to_hsv

    col = _colours()
    assert np.array_equal(rgb_to_hsv(col), np.array(Image.fromarray(col).convert("HSV")))
    as_hsv = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(col[..., c])) for c in range(3)])
    assert np.array_equal(hsv_to_rgb(col), np.array(as_hsv.convert("RGB")))
    for r_h, r_s, r_v in ((-0.009, 0.31, -0.2), (0.0, -0.4, 0.3), (0.0071, 0.0, 0.0)):
        # the reference's RandomHSV, step by step, on Pillow's own conversions
        hsv = np.array(Image.fromarray(col).convert("HSV"), dtype=np.int16)
        hsv[..., 0] = (hsv[..., 0] + round(r_h * 255)) % 255
        hsv[..., 1] = np.clip(hsv[..., 1] * (r_s + 1), 0, 255)
        hsv[..., 2] = np.clip(hsv[..., 2] * (r_v + 1), 0, 255)
        hsv = hsv.astype(np.uint8)
        want = np.array(Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(hsv[..., c])) for c in range(3)]).convert("RGB"))
        assert np.array_equal(apply_hsv(col, hsv_tables(r_h, r_s, r_v)), want), (r_h, r_s, r_v)


def _pillow_pipeline(Image, aug, image, label, p):
    """The aerial train pipeline in Pillow calls, with the parameters of ``p`` in place of the draws (no noise)."""
    from PIL import ImageEnhance

    im, lb = Image.fromarray(image), Image.fromarray(label)
    if p.resized is not None:
        im, lb = im.resize(p.resized[::-1], Image.BILINEAR), lb.resize(p.resized[::-1], Image.NEAREST)
    if p.flip:
        im, lb = im.transpose(Image.FLIP_LEFT_RIGHT), lb.transpose(Image.FLIP_LEFT_RIGHT)
    if p.vflip:
        im, lb = im.transpose(Image.FLIP_TOP_BOTTOM), lb.transpose(Image.FLIP_TOP_BOTTOM)
    a = (1, 0, p.dx, 0, 1, p.dy)
    im = im.transform(im.size, Image.AFFINE, a, resample=Image.BILINEAR)
    lb = lb.transform(lb.size, Image.AFFINE, a, resample=Image.NEAREST, fillcolor=aug.ignore_label)
    im = im.rotate(p.angle, resample=Image.BILINEAR, expand=True)
    lb = lb.rotate(p.angle, resample=Image.NEAREST, expand=True, fillcolor=aug.ignore_label)
    im, lb = im.resize((p.w, p.h), Image.BILINEAR), lb.resize((p.w, p.h), Image.NEAREST)
    pad_w, pad_h = max(aug.tw - p.w, 0), max(aug.th - p.h, 0)
    if pad_w or pad_h:
        im = Image.fromarray(np.pad(np.array(im), ((0, pad_h), (0, pad_w), (0, 0)), mode="reflect"))
        lb = Image.fromarray(np.pad(np.array(lb), ((0, pad_h), (0, pad_w)), constant_values=aug.ignore_label).astype(np.uint8))
    box = (p.sw, p.sh, p.sw + aug.tw, p.sh + aug.th)
    im, lb = im.crop(box), lb.crop(box)
    if p.hsv is not None:
        hsv = np.array(im.convert("HSV"), dtype=np.int16)
        hsv[..., 0] = (hsv[..., 0] + round(p.hsv[0] * 255)) % 255
        hsv[..., 1] = np.clip(hsv[..., 1] * (p.hsv[1] + 1), 0, 255)
        hsv[..., 2] = np.clip(hsv[..., 2] * (p.hsv[2] + 1), 0, 255)
        hsv = hsv.astype(np.uint8)
        im = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(hsv[..., c])) for c in range(3)]).convert("RGB")
    im = ImageEnhance.Contrast(im).enhance(p.contrast)
    out = np.array(im)
    if p.gamma is not None:
        out = (np.clip((out.astype(np.float32) / 255.0) ** p.gamma, 0, 1) * 255).astype(np.uint8)
    if p.cutout is not None:
        y, x = p.cutout
        out[y:y + aug.cutout_size, x:x + aug.cutout_size, :] = 0
    return out, np.array(lb)


def test_one_full_size_sample_against_pillow():
    """A UAVid-sized source (2160 x 3840, resized to 1152 x 2048) to a 1024 x 1024 crop with the dataset's defaults, noise off."""
    Image = _pil()
    from cabinet_amd.augment import DeviceAugment

    gen = np.random.RandomState(5)
    # blocks of 3 x 3 pixels: texture fine enough that a wrong tap or a wrong rounding shows, a label with regions
    image = np.repeat(np.repeat(gen.randint(0, 256, size=(720, 1280, 3)).astype(np.uint8), 3, axis=0), 3, axis=1)
    label = np.repeat(np.repeat(gen.randint(0, 19, size=(720, 1280)).astype(np.uint8), 3, axis=0), 3, axis=1)
    aug = DeviceAugment.uavid(cropsize=(1024, 1024), noise_p=0.0)
    p = aug.draw([(2160, 3840)], random.Random(2))[0]
    assert p.resized == (1152, 2048) and p.angle != 0 and aug.supported((2160, 3840), p)
    im, lb, u8 = aug([torch.from_numpy(image)], [torch.from_numpy(label)], params=[p], return_uint8=True)
    want_u8, want_lb = _pillow_pipeline(Image, aug, image, label, p)
    db, dl = int((u8[0].numpy() != want_u8).sum()), int((lb[0].numpy() != want_lb).sum())
    print(f"full size: {db} differing bytes, {dl} differing labels")
    assert db == 0 and dl == 0


def test_mixup_is_the_references_expression():
    from cabinet_amd.augment import DeviceAugment

    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((3, 40, 48), generator=g), torch.randn((3, 40, 48), generator=g)
    la, lb = torch.zeros((40, 48), dtype=torch.int64), torch.ones((40, 48), dtype=torch.int64)
    for r in (0.37, 0.5, 0.61):
        im, lab = DeviceAugment.mixup(a, la, b, lb, r)
        r32, s32 = np.float32(r), np.float32(1.0 - r)
        want = a.numpy() * r32 + b.numpy() * s32        # fp32 products and sum, each rounded on its own
        assert np.array_equal(im.numpy().view(np.int32), want.view(np.int32))
        assert lab is (la if r >= 0.5 else lb)


# --------------------------------------------------------------------------- the C ABI without a GPU

def test_symbols_abi_and_sources():
    import os

    from cabinet_amd import _lib, build
    from cabinet_amd.augment import SAMPLE_DTYPE, WARP_DTYPE

    assert "augment_warp.hip" in build.SOURCES and "augment_taps.hpp" in build.HEADERS
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.cabinet_abi_version() == 8 and _lib.ABI_VERSION == 8
    for name in ("cabinet_augment_warp_supported", "cabinet_augment_warp_batch", "cabinet_augment_resize_batch"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cabinet_hip.h")).read()
    assert "#define CABINET_ABI_VERSION 8" in header and "#define CABINET_AUGMENT_HSV 16" in header
    assert SAMPLE_DTYPE.itemsize == 2400 and WARP_DTYPE.itemsize == 192


@pytest.mark.parametrize("entry", ["cabinet_augment_warp_batch", "cabinet_augment_resize_batch"])
def test_argument_errors_need_no_gpu(entry):
    """Checked before any HIP call: the address below is never touched."""
    from cabinet_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    fn = getattr(lib, entry)
    A = 0x10000
    assert fn(None, 2, 40, 48, None) == -1 and b"null" in lib.cabinet_last_error()
    assert fn(A, 0, 40, 48, None) == -1 and fn(A, 2, 0, 48, None) == -1 and fn(A, 2, 40, -1, None) == -1
    assert b"non-positive" in lib.cabinet_last_error()
    assert fn(A + 4, 2, 40, 48, None) == -1 and b"aligned" in lib.cabinet_last_error()
    assert fn(A, 2, 32769, 48, None) == -2 and b"32768" in lib.cabinet_last_error()
    assert fn(A, 2, 40, 40000, None) == -2
    assert fn(A, 70000, 40, 48, None) == -2


def test_warp_supported_names_the_refusing_step():
    from cabinet_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    q = lib.cabinet_augment_warp_supported
    assert q(2160, 3840, 1500, 2300, -10.0, 1.875) == 1 and q(97, 200, 60, 110, 45.0, 2.5) == 1 and q(40, 72, 40, 72, 0.0, 0.0) == 1
    assert q(40, 72, 40, 72, 350.0, 0.0) == 1        # -10 degrees as Pillow normalises it
    assert q(40, 72, 80, 80, 45.5, 0.0) == 0 and b"RandomRotate" in lib.cabinet_last_error()
    assert q(40, 72, 80, 80, math.nan, 0.0) == 0
    assert q(97, 200, 38, 79, 0.0, 2.53) == 0 and b"ResizeIfLarger" in lib.cabinet_last_error()
    assert q(40, 40000, 40, 72, 0.0, 0.0) == 0 and b"32768" in lib.cabinet_last_error()
    assert q(40, 72, 0, 72, 0.0, 0.0) == 0
