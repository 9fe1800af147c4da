"""Device-side training augmentation (K18) on the GPU: csrc/augment.hip against the reference's own output
(tests/golden/g10_augment.npz) through DeviceAugment and through the raw C ABI, the call's independence of what the workspace
held, the bytes around its outputs, resize ratios up to the coverage limit of 2.5, and the in-kernel noise: its statistics and
its bytes against a numpy restatement of the generator."""
import ctypes

import numpy as np
import pytest
import torch

import augment_golden as ag

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _raw(aug, images, labels, params, noise, seed, im, lb, u8, ws=None):
    """cabinet_augment_batch itself: table from DeviceAugment.build_table, everything else by hand."""
    from cabinet_amd import _lib

    lib = _lib.load()
    N, th, tw = len(images), aug.th, aug.tw
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
    table = torch.from_numpy(aug.build_table([t.data_ptr() for t in images], [t.data_ptr() for t in labels], sizes, params)).to(DEV)
    need = lib.cabinet_augment_workspace_bytes(N, th, tw)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert ws.numel() >= need
    m3, s3 = (ctypes.c_float * 3)(*aug.mean), (ctypes.c_float * 3)(*aug.std)
    rc = lib.cabinet_augment_batch(table.data_ptr(), N, th, tw, noise.data_ptr() if noise is not None else None, seed,
                                   ctypes.addressof(m3), ctypes.addressof(s3), im.data_ptr(), lb.data_ptr(),
                                   u8.data_ptr() if u8 is not None else None, ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cabinet_augment_batch")
    torch.cuda.synchronize()
    return ws


def _check(cs, im, lb, u8, who):
    im, lb, u8 = im.cpu().numpy(), lb.cpu().numpy(), u8.cpu().numpy()
    for j, c in enumerate(cs):
        db, dl = int((u8[j] != c.u8).sum()), int((lb[j] != c.lb).sum())
        ulp = ag.ulp_distance(im[j], c.f32)
        print(f"{who} case {c.index} source {c.size} crop {c.crop}: {db} differing bytes, {dl} differing labels, fp32 max {ulp} ulp")
        assert db == 0 and dl == 0, (who, c.index, db, dl)
        assert ulp <= 1, (who, c.index, ulp)   # bit equality is expected (two correctly rounded operations on both sides)


@pytest.mark.parametrize("crop", ag.crops())
def test_fixture_through_device_augment(crop):
    """One batch per crop size: the sources differ in size within a batch."""
    aug, cs, images, labels, params, noise = ag.batch(crop, DEV)
    im, lb, u8 = aug(images, labels, params=params, noise=noise, return_uint8=True)
    assert im.is_cuda and im.dtype == torch.float32 and lb.dtype == torch.int64
    _check(cs, im, lb, u8, "DeviceAugment")


@pytest.mark.parametrize("crop", ag.crops())
def test_fixture_through_the_c_abi_twice_into_one_workspace(crop):
    """The raw entry point; then the same call again into the same workspace, which now holds the first call's sums and crop:
    identical output (a sum the call did not start from zero itself would double the contrast mean)."""
    aug, cs, images, labels, params, noise = ag.batch(crop, DEV)
    N, (tw, th) = len(cs), crop
    outs = []
    ws = None
    for rep in range(2):
        im = torch.full((N, 3, th, tw), float("nan"), device=DEV)
        lb = torch.full((N, th, tw), -1, dtype=torch.int64, device=DEV)
        u8 = torch.full((N, th, tw, 3), 0xFF, dtype=torch.uint8, device=DEV)
        if ws is None:
            from cabinet_amd import _lib
            ws = torch.full((_lib.load().cabinet_augment_workspace_bytes(N, th, tw),), 0xFF, dtype=torch.uint8, device=DEV)
        _raw(aug, images, labels, params, noise, 0, im, lb, u8, ws)
        _check(cs, im, lb, u8, f"C ABI call {rep}")
        outs.append((im, lb, u8))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("crop,offset", [((45, 37), 3), ((45, 37), 4), ((48, 40), 1), ((130, 70), 8)])
def test_outputs_inside_poisoned_allocations(crop, offset):
    """out tensors `offset` elements into larger NaN / 0xFF allocations (offsets that do and do not leave 16-byte alignment, a
    crop whose pixel count is no multiple of four): the results are right and no neighbouring byte moves."""
    aug, cs, images, labels, params, noise = ag.batch(crop, DEV)
    N, (tw, th) = len(cs), crop
    n_im, n_lb, n_u8, pad = N * 3 * th * tw, N * th * tw, N * th * tw * 3, 64
    big_im = torch.full((n_im + 2 * pad,), float("nan"), device=DEV)
    big_lb = torch.full((n_lb + 2 * pad,), -1, dtype=torch.int64, device=DEV)
    big_u8 = torch.full((n_u8 + 2 * pad,), 0xFF, dtype=torch.uint8, device=DEV)
    im = big_im[offset:offset + n_im].view(N, 3, th, tw)
    lb = big_lb[offset:offset + n_lb].view(N, th, tw)
    u8 = big_u8[offset:offset + n_u8].view(N, th, tw, 3)
    _raw(aug, images, labels, params, noise, 0, im, lb, u8)
    _check(cs, im, lb, u8, "poisoned")
    assert bool(torch.isnan(big_im[:offset]).all()) and bool(torch.isnan(big_im[offset + n_im:]).all())
    assert bool((big_lb[:offset] == -1).all()) and bool((big_lb[offset + n_lb:] == -1).all())
    assert bool((big_u8[:offset] == 0xFF).all()) and bool((big_u8[offset + n_u8:] == 0xFF).all())
    # the same through out= of DeviceAugment
    big_im.fill_(float("nan")), big_lb.fill_(-1)
    res = aug(images, labels, params=params, noise=noise, out=(im, lb), return_uint8=True)
    assert res[0] is im and res[1] is lb
    _check(cs, im, lb, res[2], "out=")
    assert bool(torch.isnan(big_im[:offset]).all()) and bool(torch.isnan(big_im[offset + n_im:]).all())
    assert bool((big_lb[:offset] == -1).all()) and bool((big_lb[offset + n_lb:] == -1).all())


def test_in_kernel_noise_statistics():
    """A 256 x 256 constant-128 image, every other step the identity: out - 128 is floor of N(0, sigma^2), sigma = 0.03 * 255 =
    7.65 (128 is sixteen sigma from either end of the byte range: nothing clips), over N = 196 608 values.  Bounds are six
    standard errors of each statistic: the mean of floor(x) is -1/2 with standard error sigma / sqrt(N); the variance is
    sigma^2 + 1/12 with relative standard error sqrt(2 / N); the lag-1 correlation of independent values has standard error
    1 / sqrt(N)."""
    from cabinet_amd.augment import DeviceAugment

    aug = DeviceAugment((256, 256), scales=(1.0,), flip_p=0.0, noise_sigma=0.03, noise_p=1.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    image = torch.full((256, 256, 3), 128, dtype=torch.uint8, device=DEV)
    label = torch.zeros((256, 256), dtype=torch.uint8, device=DEV)
    params = aug.draw([(256, 256)] * 2)
    assert all(p.noise and not p.flip and p.gamma is None and p.cutout is None and not p.gray for p in params)

    def run(seed):
        return aug([image, image], [label, label], params=params, seed=seed, return_uint8=True)[2].cpu().numpy()

    a, b, c = run(1234), run(1234), run(1235)
    assert np.array_equal(a, b)                       # the same key: the same bytes
    assert not np.array_equal(a, c)                   # another seed
    assert not np.array_equal(a[0], a[1])             # another sample index
    sigma, N = 0.03 * 255, 256 * 256 * 3
    for name, u8 in (("seed 1234 sample 0", a[0]), ("seed 1234 sample 1", a[1]), ("seed 1235 sample 0", c[0])):
        d = u8.astype(np.float64).reshape(-1) - 128.0
        assert d.size == N
        mean, var = d.mean(), d.var()
        e = d - mean
        lag1 = float((e[:-1] * e[1:]).sum() / (e * e).sum())
        print(f"{name}: mean {mean:+.4f} (want -0.5 +- {6 * sigma / np.sqrt(N):.4f}), var {var:.4f} (want {sigma ** 2 + 1 / 12:.4f} "
              f"+- {600 * np.sqrt(2 / N):.2f} %), lag-1 {lag1:+.5f} (+- {6 / np.sqrt(N):.5f})")
        assert abs(mean + 0.5) <= 6 * sigma / np.sqrt(N)
        assert abs(var / (sigma ** 2 + 1 / 12) - 1) <= 6 * np.sqrt(2 / N)
        assert abs(lag1) <= 6 / np.sqrt(N)


@pytest.mark.parametrize("crop", sorted({c.crop for c in ag.continuous_cases()}))
def test_continuous_fixture_up_to_the_ratio_limit(crop):
    """The reference's output for continuous scales in (0.4, 0.6): a scale just under 0.5, ratios up to 2.5 itself, where a tile
    of 16 output rows reads up to 43 source rows (tests/test_augment.py asserts the fixture holds them)."""
    aug, cs, images, labels, params = ag.continuous_batch(crop, DEV)
    im, lb, u8 = aug(images, labels, params=params, return_uint8=True)
    host = aug([t.cpu() for t in images], [t.cpu() for t in labels], params=params, return_uint8=True)
    u8, lb = u8.cpu().numpy(), lb.cpu().numpy()
    for j, c in enumerate(cs):
        db, dl = int((u8[j] != c.u8).sum()), int((lb[j] != c.lb).sum())
        print(f"continuous case {c.index} source {c.size} crop {c.crop} scale {params[j].scale:.4f}: {db} differing bytes, {dl} differing labels")
        assert db == 0 and dl == 0, (c.index, db, dl)
    assert ag.ulp_distance(im.cpu().numpy(), host[0].numpy()) <= 1   # the numpy path's own tensor; bit equality is expected


def test_device_equals_host_at_the_widest_ratio_over_many_tiles():
    """1024 source rows to 410 (ratio 2.4976, five taps, 43 source rows under the worst of 26 row tiles) and to 502 (scale just
    under 0.5), every photometric step on: the kernels against the numpy path, which the CPU tier holds against the reference."""
    import random

    from cabinet_amd.augment import DeviceAugment

    gen = np.random.RandomState(7)
    image = torch.from_numpy(gen.randint(0, 256, size=(1024, 160, 3)).astype(np.uint8))
    label = torch.from_numpy(gen.randint(0, 256, size=(1024, 160)).astype(np.uint8))
    for n_out in (410, 502):
        aug = DeviceAugment.cityscapes(cropsize=(64, n_out), scales=(n_out / 1024,), noise_p=0.0, cutout_size=8)
        params = aug.draw([(1024, 160)] * 2, random.Random(n_out))
        assert all(p.h == n_out and aug.supported((1024, 160), p) for p in params)
        want = aug([image, image], [label, label], params=params, return_uint8=True)
        got = aug([image.to(DEV)] * 2, [label.to(DEV)] * 2, params=params, return_uint8=True)
        for name, g, w in zip(("label", "bytes"), got[1:], want[1:]):
            diff = int((g.cpu() != w).sum())
            print(f"{n_out} rows, {name}: {diff} differing")
            assert diff == 0, (n_out, name, diff)
        ulp = ag.ulp_distance(got[0].cpu().numpy(), want[0].numpy())
        print(f"{n_out} rows, fp32: max {ulp} ulp")
        assert ulp <= 1


def test_in_kernel_noise_is_the_documented_philox_stream():
    """The bytes of a constant-128 image against a numpy restatement of the contract: Philox4x32-10 (tests/test_augment.py holds
    the restatement against the known-answer vectors) with key (seed low, seed high) and counter (pixel low, pixel high, sample,
    0); uniforms ((c >> 8) + 0.5) 2^-24 in fp32; Box-Muller, r0 from word 0 with the angle of word 1 giving R (cos) and G (sin),
    r1 from word 2 with the angle of word 3 giving B (cos); times fp32 sigma * 255; (uint8)(128 + noise).  The device's logf /
    sinf / cosf differ from double by a few fp32 units in the last place of values below 5.5 sigma = 42 (4e-6 each) and the angle
    2 pi u is rounded to fp32 (3e-7 times r sigma <= 42): under 1e-4 in all.  So every byte must equal floor of the double value
    wherever that value is further than 1e-3 from an integer, and be one of its two neighbours elsewhere."""
    from cabinet_amd.augment import DeviceAugment

    th = tw = 96
    seed = 0x9E3779B97F4A7C15
    aug = DeviceAugment((tw, th), scales=(1.0,), flip_p=0.0, noise_sigma=0.03, noise_p=1.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    image = torch.full((th, tw, 3), 128, dtype=torch.uint8, device=DEV)
    label = torch.zeros((th, tw), dtype=torch.uint8, device=DEV)
    params = aug.draw([(th, tw)] * 3)
    got = aug([image] * 3, [label] * 3, params=params, seed=seed, return_uint8=True)[2].cpu().numpy().astype(np.int64)

    P = th * tw
    ctr = np.zeros((3, P, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(P, dtype=np.uint32)[None, :]
    ctr[..., 2] = np.arange(3, dtype=np.uint32)[:, None]
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), (3, P, 2))
    words = ag.philox4x32_10(ctr, key)
    u = ((words >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u = u.astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    z = np.stack([r0 * np.cos(2 * np.pi * u[..., 1]), r0 * np.sin(2 * np.pi * u[..., 1]), r1 * np.cos(2 * np.pi * u[..., 3])], axis=-1)
    value = 128.0 + z * float(np.float32(0.03 * 255))
    want = np.floor(value).astype(np.int64).reshape(3, th, tw, 3)
    near = (np.abs(value - np.round(value)) < 1e-3).reshape(3, th, tw, 3)
    print(f"{int((got != want).sum())} of {want.size} bytes differ from floor of the double value, {int(near.sum())} values within 1e-3 of an integer")
    assert value.min() > 1 and value.max() < 254                  # nothing clips
    assert np.array_equal(got[~near], want[~near])
    assert int(np.abs(got - want).max()) <= 1
    assert near.mean() < 0.01


def test_device_path_raises_on_unsupported_shapes():
    import random

    from cabinet_amd.augment import DeviceAugment

    im, lb = torch.zeros((40, 72, 3), dtype=torch.uint8, device=DEV), torch.zeros((40, 72), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="outside coverage"):
        DeviceAugment((16, 16), scales=(0.3,))([im], [lb], rng=random.Random(0))
