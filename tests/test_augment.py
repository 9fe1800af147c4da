"""Device-side training augmentation (K18), CPU tier: the host path of cabinet_amd.augment.DeviceAugment against the
reference's own output (tests/golden/g10_augment.npz, and g10_augment_continuous.npz for continuous scales up to the coverage
limit), its table builders and a whole sample against Pillow, the coverage boundary, and the C ABI's argument checks."""
import os
import random

import numpy as np
import pytest
import torch

import augment_golden as ag

SCALES = (0.75, 1.0, 1.25, 1.5, 1.75, 2.0)


def test_fixture_holds_every_branch():
    """What the generator asserted when it chose the seeds, read back from the parameters draw() gives for them."""
    seen = set()
    for c in ag.cases():
        p = ag.augmenter(c.crop).draw([c.size], random.Random(c.seed))[0]
        tw, th = c.crop
        seen |= {("scale", p.scale), ("flip", p.flip), ("pad", p.w < tw, p.h < th), ("gray", p.gray), ("gamma", p.gamma is not None),
                 ("noise", p.noise), ("b", np.float32(p.brightness) <= 1), ("c", np.float32(p.contrast) <= 1),
                 ("s", np.float32(p.saturation) <= 1)}
        if p.cutout is not None:
            seen |= {("cut_top", p.cutout[0] == 0), ("cut_bottom", p.cutout[0] + 8 == th)}
        assert (c.noise is not None) == p.noise
    want = {("scale", s) for s in SCALES} | {("flip", f) for f in (False, True)} | {("pad", x, y) for x in (False, True) for y in (False, True)}
    want |= {(k, v) for k in "bcs" for v in (False, True)} | {("gray", True), ("gamma", True), ("noise", True), ("cut_top", True),
                                                               ("cut_bottom", True)}
    assert want <= seen, sorted(map(str, want - seen))
    assert os.path.getsize(ag.GOLDEN) <= 1 << 20


@pytest.mark.parametrize("i", range(ag.n_cases()))
def test_host_path_reproduces_the_reference(i):
    """Parameters drawn by draw(random.Random(k)) -- so the draw order is the reference's -- and 0 differing bytes and labels."""
    c = ag.Case(i)
    aug = ag.augmenter(c.crop)
    noise = torch.from_numpy(c.noise)[None] if c.noise is not None else None
    im, lb, u8 = aug([torch.from_numpy(c.image)], [torch.from_numpy(c.label)], rng=random.Random(c.seed), noise=noise, return_uint8=True)
    assert im.dtype == torch.float32 and tuple(im.shape) == (1, 3, c.crop[1], c.crop[0])
    assert lb.dtype == torch.int64 and tuple(lb.shape) == (1, c.crop[1], c.crop[0])
    assert int((u8[0].numpy() != c.u8).sum()) == 0
    assert int((lb[0].numpy() != c.lb).sum()) == 0
    assert ag.ulp_distance(im[0].numpy(), c.f32) <= 1


@pytest.mark.parametrize("crop", ag.crops())
def test_host_batch_mixes_source_sizes_and_replays_params(crop):
    aug, cs, images, labels, params, noise = ag.batch(crop)
    im = torch.full((len(cs), 3, crop[1], crop[0]), float("nan"))
    lb = torch.full((len(cs), crop[1], crop[0]), -1, dtype=torch.int64)
    res = aug(images, labels, params=params, noise=noise, out=(im, lb), return_uint8=True)
    assert res[0] is im and res[1] is lb
    for j, c in enumerate(cs):
        assert np.array_equal(res[2][j].numpy(), c.u8) and np.array_equal(lb[j].numpy(), c.lb)
    if crop == (48, 40):
        assert len({c.size for c in cs}) >= 2


def test_unsupported_samples_raise():
    from cabinet_amd.augment import DeviceAugment

    im, lb = torch.zeros((40, 72, 3), dtype=torch.uint8), torch.zeros((40, 72), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="outside coverage"):   # scale 0.3: more than five taps
        DeviceAugment((16, 16), scales=(0.3,))([im], [lb], rng=random.Random(0))
    with pytest.raises(RuntimeError, match="outside coverage"):   # 40 rows padded to 100: more than one reflection
        DeviceAugment((16, 100))([im], [lb], rng=random.Random(0))
    with pytest.raises(ValueError):
        DeviceAugment((16, 16))([im], [lb[:, :5]], rng=random.Random(0))


def test_draw_consumes_the_generator_only_for_configured_steps():
    from cabinet_amd.augment import DeviceAugment

    r = random.Random(5)
    p = DeviceAugment((16, 16), scales=(0.5, 2.0), continuous=True, contrast=0.5, gamma_p=1.0).draw([(40, 72)], r)[0]
    q = random.Random(5)
    flip = not (q.random() > 0.5)
    scale = q.uniform(0.5, 2.0)
    w, h = int(round(72 * scale)), int(round(40 * scale))
    sw = q.randint(0, w - 16) if w > 16 else 0
    sh = q.randint(0, h - 16) if h > 16 else 0
    rc = q.uniform(0.5, 1.5)
    gray = q.random() < 0.0
    gamma = q.uniform(0.7, 1.5) if q.random() < 1.0 else None
    noise, cut = q.random() < 0.0, q.random() < 0.0
    assert (p.flip, p.scale, p.w, p.h, p.sw, p.sh, p.brightness, p.contrast, p.saturation, p.gray, p.gamma, p.noise, p.cutout) == \
        (flip, scale, w, h, sw, sh, 1.0, rc, 1.0, gray, gamma, noise, None) and not cut
    assert r.random() == q.random()


@pytest.mark.parametrize("scale", SCALES)
def test_tables_against_pillow_at_cityscapes_size(scale):
    """Column and row tables of a 1024 x 2048 source against Pillow itself: a strip of full width resized in x only, a strip of
    full height resized in y only, image (BILINEAR) and label (NEAREST)."""
    Image = pytest.importorskip("PIL.Image")
    from cabinet_amd.augment import TAP_DTYPE, DeviceAugment, _AxisTables

    H, W = 1024, 2048
    w, h = int(round(W * scale)), int(round(H * scale))
    gen = np.random.RandomState(int(scale * 100))
    for n_in, n_out, axis in ((W, w, 1), (H, h, 0)):
        tab = _AxisTables(n_in, n_out)
        assert tab.n.max() <= 5
        shape = (6, n_in) if axis == 1 else (n_in, 6)
        img = gen.randint(0, 256, size=shape + (3,)).astype(np.uint8)
        lab = gen.randint(0, 256, size=shape).astype(np.uint8)
        size = (n_out, 6) if axis == 1 else (6, n_out)
        want_img = np.array(Image.fromarray(img).resize(size, Image.BILINEAR))
        want_lab = np.array(Image.fromarray(lab).resize(size, Image.NEAREST))
        taps = np.zeros(n_out, dtype=TAP_DTYPE)
        taps["first"], taps["step"], taps["n"], taps["coef"] = tab.first, 1, tab.n, tab.coef
        assert np.array_equal(DeviceAugment._apply_taps(img, taps, axis), want_img)
        assert np.array_equal(np.take(lab, tab.label, axis=axis), want_lab)


def test_symbols_abi_and_sources():
    from cabinet_amd import _lib, build

    assert "augment.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 8
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.cabinet_abi_version() == 8
    for name in ("cabinet_augment_supported", "cabinet_augment_workspace_bytes", "cabinet_augment_batch"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cabinet_hip.h")).read()
    assert "#define CABINET_ABI_VERSION 8" in header and "cabinet_augment_batch(" in header


def test_argument_errors_need_no_gpu():
    """Checked before any HIP call: the addresses below are never touched."""
    from cabinet_amd import _lib, build
    from cabinet_amd.augment import SAMPLE_DTYPE, TAP_DTYPE

    build.build(verbose=False)
    lib = _lib.load()
    A = 0x10000
    need = lib.cabinet_augment_workspace_bytes(2, 40, 48)
    assert need >= 2 * 40 * 48 * 3 + 2 * 3 * 8 and lib.cabinet_augment_workspace_bytes(0, 40, 48) == 0
    assert lib.cabinet_augment_supported(40, 48, 5, 7, 2, 33, 46) == 1
    args = dict(samples=A, N=2, th=40, tw=48, noise=None, seed=1, mean=A, std=A, im=A, lb=A, u8=None, ws=A, ws_bytes=need)

    def call(**kw):
        a = dict(args, **kw)
        return lib.cabinet_augment_batch(a["samples"], a["N"], a["th"], a["tw"], a["noise"], a["seed"], a["mean"], a["std"], a["im"],
                                         a["lb"], a["u8"], a["ws"], a["ws_bytes"], None)

    for name in ("samples", "mean", "std", "im", "lb"):     # a null pointer: -1
        assert call(**{name: None}) == -1 and b"null" in lib.cabinet_last_error(), name
    assert call(ws_bytes=need - 1) == -1 and b"workspace" in lib.cabinet_last_error()   # a short workspace: -1
    assert call(ws=None) == -1
    assert call(N=0) == -1
    # six taps (a resize ratio above 2.5): outside coverage, with the reason as text; the batch call cannot see the tables, which are
    # in device memory, so the tap count is refused where it is stated and the batch call refuses the shapes it is given
    assert lib.cabinet_augment_supported(40, 48, 6, 0, 0, 33, 46) == 0 and b"taps" in lib.cabinet_last_error()
    assert lib.cabinet_augment_supported(40, 48, 5, 33, 0, 33, 46) == 0 and b"padding" in lib.cabinet_last_error()
    assert call(th=40000) == -2 and b"32768" in lib.cabinet_last_error()
    with pytest.raises(RuntimeError, match="code -2"):
        _lib.check(-2, "cabinet_augment_batch")
    assert SAMPLE_DTYPE.itemsize == 2400 and TAP_DTYPE.itemsize == 32


@pytest.mark.parametrize("i", range(len(ag.continuous_cases())))
def test_host_path_reproduces_the_reference_at_continuous_scales(i):
    """The reference's own output for RandomScale(continuous=True) over (0.4, 0.6) with only contrast, gray, gamma and cutout
    configured: the uniform draw of the scale, the jitter draws that are skipped, and resize ratios up to the limit of 2.5."""
    c = ag.ContinuousCase(i)
    aug = ag.continuous_augmenter(c.crop)
    im, lb, u8 = aug([torch.from_numpy(c.image)], [torch.from_numpy(c.label)], rng=random.Random(c.seed), return_uint8=True)
    assert int((u8[0].numpy() != c.u8).sum()) == 0
    assert int((lb[0].numpy() != c.lb).sum()) == 0


def test_continuous_fixture_reaches_the_limit():
    """What its generator asserted: a scale just under 0.5, the ratio 2.5 itself, and tiles of 16 output rows that read more
    than 40 source rows (at most 43 inside coverage; the geometry kernel stages 48)."""
    from cabinet_amd.augment import MAX_RATIO, TILE_ROWS, TILE_SPAN

    spans, ratios, scales = [], [], []
    for c in ag.continuous_cases():
        aug = ag.continuous_augmenter(c.crop)
        p = aug.draw([c.size], random.Random(c.seed))[0]
        assert aug.supported(c.size, p)
        rt = aug._sample_tables(c.size, p)[1]
        tile = np.arange(0, aug.th, TILE_ROWS)
        spans.append(int((np.maximum.reduceat(rt["first"] + rt["n"] - 1, tile) - np.minimum.reduceat(rt["first"], tile) + 1).max()))
        ratios.append(max(c.size[0] / p.h, c.size[1] / p.w))
        scales.append(p.scale)
    assert max(ratios) == MAX_RATIO and 40 < max(spans) <= 43 < TILE_SPAN
    assert any(0.49 <= s < 0.5 for s in scales) and any(s >= 0.5 for s in scales)
    assert os.path.getsize(ag.GOLDEN_CONT) <= 1 << 20


def test_coverage_is_the_resize_ratio():
    """Five taps do not bound the rows a tile reads: the ratio in/out <= 2.5 does (fewer than 17 * 2.5 + 1 rows), and both routes
    refuse what is past it, whatever its tap count."""
    from cabinet_amd.augment import TILE_ROWS, TILE_SPAN, DeviceAugment, resample_taps

    im, lb = torch.zeros((1024, 1024, 3), dtype=torch.uint8), torch.zeros((1024, 1024), dtype=torch.uint8)
    for n_out, ok in ((410, True), (409, False)):     # 1024 / 410 = 2.4976 (43 rows per tile), 1024 / 409 = 2.5037
        aug = DeviceAugment((32, 64), scales=(n_out / 1024,), flip_p=0.0)
        p = aug.draw([(1024, 1024)], random.Random(0))[0]
        assert p.h == n_out and aug.supported((1024, 1024), p) == ok
        if ok:
            first, n, _ = resample_taps(1024, n_out)
            assert n.max() == 5
            assert max(first[j + TILE_ROWS - 1] + n[j + TILE_ROWS - 1] - first[j] for j in range(n_out - TILE_ROWS + 1)) == 43 <= TILE_SPAN
            aug([im], [lb], params=[p])
        else:
            with pytest.raises(RuntimeError, match="outside coverage"):
                aug([im], [lb], params=[p])
    # a tiny output clamps its taps at the borders: three taps at ratio 3, refused all the same
    aug = DeviceAugment((1, 1), scales=(1 / 3,), flip_p=0.0)
    p = aug.draw([(3, 3)], random.Random(0))[0]
    assert (p.h, p.w) == (1, 1) and resample_taps(3, 1)[1].max() == 3 and not aug.supported((3, 3), p)


def test_batch_limits_are_the_batchs_own():
    """What DeviceAugment states to cabinet_augment_supported: the largest tap count and pads and the smallest resized size of
    the samples at hand, not constants, and the library accepts them."""
    from cabinet_amd import _lib, build

    aug, cs, images, labels, params, noise = ag.batch((48, 40))
    sizes = [c.size for c in cs]
    taps, pad_y, pad_x, min_h, min_w = aug._check(sizes, params)
    assert taps == max(max(aug._axis(s[0], p.h).n.max(), aug._axis(s[1], p.w).n.max()) for s, p in zip(sizes, params))
    assert (pad_y, pad_x) == (max(max(40 - p.h, 0) for p in params), max(max(48 - p.w, 0) for p in params))
    assert (min_h, min_w) == (min(p.h for p in params), min(p.w for p in params)) and pad_y > 0 and pad_x > 0
    build.build(verbose=False)
    assert _lib.load().cabinet_augment_supported(40, 48, taps, pad_y, pad_x, min_h, min_w) == 1


def test_table_cache_is_bounded():
    from cabinet_amd.augment import _TABLE_CACHE, DeviceAugment

    aug = DeviceAugment((8, 8), scales=(0.5, 2.0), continuous=True)
    first = aug._axis(64, 64)
    for n_out in range(32, 32 + 3 * _TABLE_CACHE):
        aug._axis(64, n_out)
        assert aug._axis(64, 64) is first          # in use: kept
    assert len(aug._tables) == _TABLE_CACHE


def test_philox_restatement_known_answers():
    """The numpy Philox4x32-10 that tests/test_gpu_augment.py holds the kernel's generator against, on the known-answer vectors
    of the Random123 distribution (kat_vectors: zeros, ones, digits of pi)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    ctr = np.array([k[0] for k in kat], dtype=np.uint32)
    key = np.array([k[1] for k in kat], dtype=np.uint32)
    assert np.array_equal(ag.philox4x32_10(ctr, key), np.array([k[2] for k in kat], dtype=np.uint32))


@pytest.mark.parametrize("scale,seed", [(0.75, 3), (2.0, 4)])
def test_host_path_against_pillow_at_cityscapes_size(scale, seed):
    """A whole 1024 x 2048 sample to a 1024 x 1024 crop through Pillow's and numpy's own calls, in the reference's order, with
    the parameters draw() gives (noise off): equal bytes and labels.  Scale 0.75 is the widest filter of the default pipeline,
    2.0 the largest image."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance

    from cabinet_amd.augment import DeviceAugment

    gen = np.random.RandomState(seed)
    image = gen.randint(0, 256, size=(1024, 2048, 3)).astype(np.uint8)
    label = gen.randint(0, 34, size=(1024, 2048)).astype(np.uint8)
    aug = DeviceAugment.cityscapes(scales=(scale,), noise_p=0.0, gamma_p=1.0, cutout_p=1.0, label_map=(np.arange(256) * 7) % 19)
    p = aug.draw([(1024, 2048)], random.Random(seed))[0]
    _, lb, u8 = aug([torch.from_numpy(image)], [torch.from_numpy(label)], params=[p], return_uint8=True)

    im, lab = Image.fromarray(image), Image.fromarray(label)
    if p.flip:
        im, lab = im.transpose(Image.FLIP_LEFT_RIGHT), lab.transpose(Image.FLIP_LEFT_RIGHT)
    im, lab = im.resize((p.w, p.h), Image.BILINEAR), lab.resize((p.w, p.h), Image.NEAREST)
    pw, ph = max(1024 - p.w, 0), max(1024 - p.h, 0)
    if pw or ph:
        im = Image.fromarray(np.pad(np.array(im), ((0, ph), (0, pw), (0, 0)), mode="reflect"))
        lab = Image.fromarray(np.pad(np.array(lab), ((0, ph), (0, pw)), constant_values=255).astype(np.uint8))
    box = (p.sw, p.sh, p.sw + 1024, p.sh + 1024)
    im, lab = im.crop(box), lab.crop(box)
    im = ImageEnhance.Color(ImageEnhance.Contrast(ImageEnhance.Brightness(im).enhance(p.brightness)).enhance(p.contrast)).enhance(p.saturation)
    if p.gray:
        im = im.convert("L").convert("RGB")
    a = np.array(im)
    a = (np.clip((a.astype(np.float32) / 255.0) ** p.gamma, 0, 1) * 255).astype(np.uint8)
    a[p.cutout[0]:p.cutout[0] + 64, p.cutout[1]:p.cutout[1] + 64, :] = 0
    want_lb = np.where(np.array(lab) == 255, 255, aug.label_lut[np.array(lab, dtype=np.int64)])
    assert int((u8[0].numpy() != a).sum()) == 0
    assert int((lb[0].numpy() != want_lb).sum()) == 0
