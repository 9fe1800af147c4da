"""The device-side augmentation -- K18 csrc/augment.hip, K20 csrc/augment_warp.hip, the shared csrc/augment_taps.hpp and the host
code of cabinet_amd/augment.py that composes them -- where its launch rules branch and where its tiles, pixel groups and
buffers end.  The oracle of every case is the project's numpy route on the same parameters (tests/augment_edge_cases.py), which
test_edge_oracle_against_pillow holds against Pillow's own calls at the shapes of these tables.  All comparisons are exact:
final bytes and labels 0 differing, the fp32 tensor at most 1 ulp (augment_golden.ulp_distance); no tolerance anywhere.

1. `test_augment_plan_cases_reach_their_branches` (no kernel launched): AUG_TX / AUG_TY / AUG_RS / AUG_TAPS / WARP_TX / WARP_TY as
   the sources spell them, the tile count, the crop stride, the photo grid, `cnt`, the two store-alignment predicates and the
   per-tile span restated and held against cabinet_augment_workspace_bytes (the tile count decoded from its answer),
   cabinet_augment_supported, cabinet_augment_warp_supported and TILE_ROWS / TILE_SPAN / MAX_RATIO of augment.py; then every
   row of the tables asserted to reach the branch it is listed for, and each table's row count.
2. A, K18 through DeviceAugment with explicit SampleParams: the rows of K18_CASES, the residue sweep of 73 x 22 crops in four
   blocks of th, and 64 placements of the outputs inside poisoned allocations through the raw C ABI.
3. B, the K20 passes through the raw C ABI: every output at an odd byte offset inside one 0xFF allocation whose other bytes
   must not move.
4. C, the composition: passes only some samples take, buffers that grow and are reused oversized, two calls queued on one
   stream, `out=` reused -- against the numpy route and bit for bit against a fresh DeviceAugment.
5. D, the caller contract: non-contiguous and offset inputs give the dense call's bits; refused inputs leave `out=` unchanged
   and name the step.

The 257-tile rows: the issue's crops (1, 4097) and (16385, 1) have a 257th tile of ONE pixel, which moves the mean luma by at
most 255 / P < 1, never by 2; their sources are ramps placed so that leaving that pixel out still moves the rounded mean by one
(the blend at 0.6 then gives other bytes), and the two 512-tile rows carry the difference of at least 2.
"""
import dataclasses
import random

import numpy as np
import pytest
import torch

import augment_edge_cases as E
from augment_golden import ulp_distance

gpu = pytest.mark.gpu
DEV = "cuda"
PAD = 64


# ------------------------------------------------------------------------------------------------ 1. the plan tables
def _all_resize_items():
    return [it for g in E.RESIZE_GROUPS for it in E.resize_group(g)]


def _all_warp_items():
    return [it for s in E.WARP_SHAPES for it in E.warp_group(s)]


def test_augment_plan_cases_reach_their_branches():
    """Every row of the tables of augment_edge_cases.py reaches the branch it is there for: the restated launch rules against
    the library's queries and the sources' constants, then the tables against the restated rules."""
    from cabinet_amd import _lib
    from cabinet_amd import augment as A

    lib = _lib.load()
    assert E.source_constants() == E.RESTATED
    assert (A.TILE_ROWS, A.TILE_SPAN, A.MAX_RATIO, A.MAX_TAPS) == (E.AUG_TY, E.AUG_RS, 2.5, E.AUG_TAPS)
    assert (E.AUG_TY + 1) * A.MAX_RATIO + 1 < E.AUG_RS and E.AUG_TX * E.AUG_TY == 4 * E.PHOTO_THREADS
    crops = [row["crop"] for row in E.K18_CASES.values()] + [(tw, th) for tw in E.SWEEP_TW for th in E.SWEEP_TH] + list(E.POISON_CROPS.values())
    for tw, th in crops:
        for N in (1, 2, 3, 16):
            got = lib.cabinet_augment_workspace_bytes(N, th, tw)
            assert got == E.workspace_bytes(N, th, tw) and E.tiles_from_workspace(N, th, tw, got) == E.tiles(th, tw), (tw, th, N)
        assert E.crop_stride(th, tw) % 16 == 0 and E.photo_grid(th, tw, 2) == ((th * tw + 1023) // 1024, 2)
    for th, tw in ((1, 1), (0, 5), (5, 0), (32768, 1), (32769, 1), (1, 32769)):
        for taps in (0, 1, 5, 6):
            for mh, py in ((1, 0), (9, 8), (9, 9), (0, 0), (4, -1)):
                args = (th, tw, taps, py, 0, mh, 7)
                assert lib.cabinet_augment_supported(*args) == int(E.k18_supported(*args)), args
                args = (th, tw, taps, 0, py, 7, mh)
                assert lib.cabinet_augment_supported(*args) == int(E.k18_supported(*args)), args
    for dims in ((1, 1, 1, 1), (0, 1, 1, 1), (32768, 32768, 32768, 32768), (1, 32769, 1, 1), (1, 1, 0, 1), (1, 1, 1, 32769)):
        for angle in (0.0, 45.0, -45.0, 45.01, -45.01, 0.01):
            for ratio in (0.0, 1.0, 2.5, 2.51, -0.1):
                assert lib.cabinet_augment_warp_supported(*dims, angle, ratio) == int(E.warp_supported(*dims, angle, ratio)), (dims, angle, ratio)

    # K18 rows
    assert len(E.K18_CASES) == 27 and len(E.TINY_CROPS) == 9                                        # no row may leave unnoticed
    plans = {}
    for name, row in E.K18_CASES.items():
        b = E.k18_case(name)
        assert all(b.aug.supported(s, p) for s, p in zip(b.sizes, b.params)), name
        assert b.noise is not None or not any(p.noise for p in b.params)
        plan = plans[name] = E.k18_plan(b)
        branch = row["branch"]
        if branch.startswith("tiles>256"):
            assert plan["tiles"] == (512 if branch.endswith("by 2") else 257) > E.PHOTO_THREADS, (name, plan["tiles"])
            m, m_wrong, differs = E.wrong_mean_bytes(b)
            first, whole = E.first_tiles_mean(b)
            print(f"{name}: m {m}, over the first 256 tiles only {m_wrong}; mean luma of those tiles {first:.3f}, of the crop {whole:.3f}")
            assert m != m_wrong and differs, name
            if branch.endswith("by 2"):
                assert abs(first - whole) >= 2 and abs(m - m_wrong) >= 2, (name, first, whole)
            else:   # one pixel in the 257th tile: 255 / P is all it can move the mean by
                P = plan["P"]
                assert P - 256 * (E.AUG_TY if b.aug.tw == 1 else E.AUG_TX) == 1 and abs(m - m_wrong) == 1
        elif branch == "grid":
            assert plan["grid"] == (3, 5) and len(b.params) == 3 and len({p.contrast for p in b.params}) == 3
        elif branch == "cnt":
            assert plan["cnt"] == ({plan["P"] % 4} if plan["P"] < 4 else {4, plan["P"] % 4}), name
        elif branch == "span>=40":
            assert 40 <= plan["span"] <= E.AUG_RS and all(p.h * 2.5 == s[0] and p.w * 2.5 == s[1] for s, p in zip(b.sizes, b.params)), (name, plan["span"])
        elif branch == "step=-1":
            assert plan["steps"] == {-1} and all(p.scale == 2.0 and p.flip for p in b.params)
        elif branch == "maxpad":
            assert all((px, py) == (w - 1, h - 1) and px > 0 and py > 0 for px, py, w, h in plan["pad"])
            lb = b.host()[1]
            assert bool((lb[:, 9:, :] == 255).all()) and bool((lb[:, :, 11:] == 255).all()) and bool((lb[:, :9, :11] != 255).all())
        elif branch in ("H=1", "W=1"):
            assert all(s[0 if branch == "H=1" else 1] == 1 for s in b.sizes)
        elif branch == "flags":
            flags = [(p.gray, p.gamma is not None, p.noise, p.cutout is not None) for p in b.params]
            assert len(set(flags)) == 16 == len(flags)
        elif branch == "cutout":
            assert any(p.cutout is not None for p in b.params)
        elif branch == "jitter":
            assert sorted((p.brightness, p.contrast, p.saturation) for p in b.params) == sorted(
                tuple(v if k == j else (0.8, 1.2, 0.8)[j] for j in range(3)) for k in range(3) for v in (0.0, 1.0, 0.5, 1.5))
        elif branch == "hsv":
            blob = b.aug.build_table([0] * 4, [0] * 4, b.sizes, b.params)
            e = blob[:4 * A.SAMPLE_DTYPE.itemsize].view(A.SAMPLE_DTYPE)
            assert [bool(f & A.FLAG_HSV) for f in e["flags"]] == [True, False, True, False]
            at = [int(e["reserved"][0]), int(e["reserved"][2])]
            assert at[1] == at[0] + 768 == blob.size - 768 and int(e["reserved"][1]) == 0 == int(e["reserved"][3])
            for k, i in zip(at, (0, 2)):
                assert np.array_equal(blob[k:k + 768], A.hsv_tables(*b.params[i].hsv).reshape(-1))
            assert not np.array_equal(blob[at[0]:at[0] + 768], blob[at[1]:at[1] + 768])
        else:
            raise AssertionError(branch)
    corners = {p.cutout for p in E.k18_case("cutout-corners").params}
    assert corners == {(0, 0), (0, 37), (29, 0), (29, 37)} and E.k18_case("cutout-whole-crop").aug.cutout_size == 24
    assert not E.k18_case("cutout-whole-crop").host()[2][0].any()
    tiny = [plans["tiny-%dx%d" % c]["P"] for c in E.TINY_CROPS]
    assert {P % 4 for P in tiny if P < 4} == {1, 2, 3} == {P % 4 for P in tiny if P > 4}
    phases = [E.k18_case(n).params[0] for n in plans if n.startswith("ratio-2.5")]     # 2 output rows step over 5 source rows
    assert [(p.sh, p.sh % 2, p.sh + 16 == p.h) for p in phases] == [(0, 0, False), (15, 1, False), (32, 0, True)]

    # the sweeps: the whole seed table, every cnt, every store pairing
    assert len(E.SWEEP_TW) == 73 and len(E.SWEEP_TH) == 22 and sum(E.SWEEP_TH_BLOCKS, []) == E.SWEEP_TH
    cnts, pairs, later = set(), set(), 0
    for tw in E.SWEEP_TW:
        for th in E.SWEEP_TH:
            found = E.sweep_case(tw, th)
            assert found is not None, f"crop {(tw, th)}: no seed of {E.SWEEP_SEEDS} gives params that supported() takes"
            later += found[1] != 1000 * tw + th
            cnts |= E.group_counts(tw * th)
            pairs |= E.store_pairings(tw * th, 2)
    print(f"sweep: {later} of {73 * 22} shapes redrawn from a later seed")
    assert cnts == {1, 2, 3, 4} and pairs == {(True, True), (True, False), (False, True), (False, False)}
    assert {(tw % 64 == 0, th % 16 == 0) for tw in E.SWEEP_TW for th in E.SWEEP_TH} == {(a, b) for a in (False, True) for b in (False, True)}
    seen = set()
    for res, (tw, th) in E.POISON_CROPS.items():
        assert (tw * th) % 4 == res and tw * th > 4
        for f in range(4):
            for u in range(4):
                seen |= {(res, f, u, pair) for pair in E.store_pairings(tw * th, 2, f, u)}
    assert {s[3] for s in seen} == {(True, True), (True, False), (False, True), (False, False)}
    assert all({s[3][0] for s in seen if s[0] == res} == {True, False} for res in range(4))

    # K20 resize
    items = _all_resize_items()
    assert len(items) == 21 * 11 == 231 and all(32 <= len(E.resize_group(g)) <= 64 for g in E.RESIZE_GROUPS)
    assert sum(E.RESIZE_GROUPS, []) == E.RESIZE_OH and {it["ratios"] for it in items} == {(a, b) for a in range(4) for b in range(4)}
    spans = []
    for it in items + E.resize_mixed():
        (ct, _), (rt, _) = A._resize_axis(it["W"], it["out_w"]), A._resize_axis(it["H"], it["out_h"])
        assert int(max(ct["n"].max(), rt["n"].max())) <= E.AUG_TAPS and it["H"] <= 2.5 * it["out_h"] and it["W"] <= 2.5 * it["out_w"]
        spans += E.tile_spans(rt, it["out_h"], it["H"])
    assert 40 <= max(spans) <= E.AUG_RS and min(spans) == 1, (min(spans), max(spans))
    assert any(it["ratios"] == (3, 3) and it["H"] == 2.5 * it["out_h"] and it["W"] == 2.5 * it["out_w"] for it in items)
    assert E.warp_outside(E.resize_mixed(), E.AUG_TX, E.AUG_TY) == (5, 12)
    assert all(E.warp_outside(E.resize_group(g), E.AUG_TX, E.AUG_TY)[0] > 0 for g in E.RESIZE_GROUPS)

    # K20 warp
    assert len(E.WARP_SHAPES) == 18 and all(len(E.warp_group(s)) == 23 * 4 for s in E.WARP_SHAPES)
    modes = {}
    for it in E.warp_group((8, 33)) + E.warp_mixed() + E.expand_group(E.EXPAND_SOURCES[0]):
        d = A.warp_descs([dict({k: v for k, v in it.items() if k not in ("image", "label")}, src_image=0, src_label=0, dst_image=0, dst_label=0)])
        mode = int(d[:A.WARP_DTYPE.itemsize].view(A.WARP_DTYPE)["label_mode"][0])
        assert mode == E.label_mode(it)
        modes.setdefault(it["kind"], set()).add(mode)
    assert modes == {"translate": {A.LABEL_TABLES}, "scale": {A.LABEL_TABLES}, "rotate": {A.LABEL_FIXED}, "shear": {A.LABEL_FIXED},
                     "scale-shear": {A.LABEL_FIXED}, "expand": {A.LABEL_FIXED}}, modes
    assert {A.LABEL_TABLES, A.LABEL_FIXED} == {E.label_mode(it) for it in E.warp_mixed()}
    assert E.warp_outside(E.warp_mixed(), E.WARP_TX, E.WARP_TY) == (90, 182)
    assert all(E.warp_outside(E.expand_group(s), E.WARP_TX, E.WARP_TY)[0] > 0 for s in E.EXPAND_SOURCES)
    # +-0.25: column 0 reads xf = -1, the last row reads yf + 1 == H
    assert np.floor((0 + 0.5) - 0.25 - 0.5) == -1 and np.floor((8 - 1 + 0.5) + 0.25 - 0.5) + 1 == 8


def test_edge_oracle_against_pillow():
    """The numpy route against Pillow's own calls at the new shapes: every row of K18_CASES, the mixed and expand=True launches
    of part B, and every tenth shape or item of the sweeps.  Noise is left out: it is an addition of given values."""
    Image = pytest.importorskip("PIL.Image")

    bad = []

    def cmp(what, want, got):
        db, dl = int((want[0] != got[0]).sum()), int((want[1] != got[1]).sum())
        if db or dl:
            bad.append(f"{what}: {db} differing bytes, {dl} differing labels")

    batches = [(n, E.k18_case(n)) for n in E.K18_CASES]
    shapes = [(tw, th) for tw in E.SWEEP_TW for th in E.SWEEP_TH][::10]
    batches += [(f"sweep {s}", E.sweep_case(*s)[0]) for s in shapes] + [(f"poison {r}", E.poison_case(r)) for r in range(4)]
    for name, b in batches:
        want, got = E.pillow_batch(Image, b)
        for i, w in enumerate(want):
            cmp(f"{name} sample {i} {b.params[i]}", w, (got[2][i], got[1][i]))
    for it in E.resize_mixed() + _all_resize_items()[::10]:
        cmp(f"resize {it['H']}x{it['W']} -> {it['out_h']}x{it['out_w']}", E.pillow_resize(Image, it), E.resize_oracle(it))
    for it in E.warp_mixed() + _all_warp_items()[::10]:
        cmp(f"warp {it['kind']} {it['H']}x{it['W']} a={it['a']} flip={it['flip']}", E.pillow_affine(Image, it), E.warp_oracle(it))
    for s in E.EXPAND_SOURCES:
        for it in E.expand_group(s):
            want = E.pillow_rotate(Image, it)
            assert want[1].shape == (it["out_h"], it["out_w"]), (s, it["angle"])
            cmp(f"rotate(expand) {s} by {it['angle']} flip={it['flip']}", want, E.warp_oracle(it))
    print(f"{len(batches)} batches; {len(bad)} disagreements")
    assert not bad, "\n".join(bad[:20])


MIXED_SOURCES = [(60, 80), (97, 200), (50, 64), (150, 180)]
MIXED_ANGLES = [0.0, 7.3, 0.0, -9.1]


def test_warp_stages_and_buffer_cache_on_the_host():
    """warp_stages on host addresses: which samples each pass holds, how each pass's outputs are laid out in its cached buffer
    and chained into the next pass, and the grow-only rule of _buffer."""
    from cabinet_amd import augment as A

    cpu = torch.device("cpu")
    aug = E.compose_aug()
    b = E.compose_batch(MIXED_SOURCES, 11, MIXED_ANGLES)
    assert [p.resized is not None for p in b.params] == [False, True, False, True]
    ims, lbs = b.tensors()
    ip0, lp0 = [t.data_ptr() for t in ims], [t.data_ptr() for t in lbs]
    stages, ip, lp = aug.warp_stages(cpu, ip0, lp0, b.sizes, b.params)
    assert [(s[0], s[1], s[3]) for s in stages] == [("resize", "cabinet_augment_resize_batch", 2), ("translate", "cabinet_augment_warp_batch", 4),
                                                    ("rotate", "cabinet_augment_warp_batch", 2)]
    last = {}
    for name, entry, descs, n, max_h, max_w, items in stages:
        buf = aug._buffers[(cpu, name)]
        need = sum(4 * it["out_h"] * it["out_w"] for it in items)
        assert buf.numel() >= need and (max_h, max_w) == (max(it["out_h"] for it in items), max(it["out_w"] for it in items))
        off = buf.data_ptr()
        for it in items:                                   # image then label of each item, items back to back
            px = it["out_h"] * it["out_w"]
            assert (it["dst_image"], it["dst_label"]) == (off, off + 3 * px)
            off += 4 * px
        e = descs.numpy()[:n * A.WARP_DTYPE.itemsize].view(A.WARP_DTYPE)
        assert [int(v) for v in e["dst_image"]] == [it["dst_image"] for it in items] and [int(v) for v in e["src_image"]] == [it["src_image"] for it in items]
        last[name] = items
    rs, tr, ro = last["resize"], last["translate"], last["rotate"]
    assert [it["src_image"] for it in rs] == [ip0[1], ip0[3]]
    assert [it["src_image"] for it in tr] == [ip0[0], rs[0]["dst_image"], ip0[2], rs[1]["dst_image"]]
    assert [it["src_label"] for it in ro] == [tr[1]["dst_label"], tr[3]["dst_label"]]
    assert ip == [tr[0]["dst_image"], ro[0]["dst_image"], tr[2]["dst_image"], ro[1]["dst_image"]]
    assert lp == [tr[0]["dst_label"], ro[0]["dst_label"], tr[2]["dst_label"], ro[1]["dst_label"]]
    # grow-only: a smaller batch runs in the same buffers, a larger one replaces them
    before = {k: (v.data_ptr(), v.numel()) for k, v in aug._buffers.items()}
    small = E.compose_batch([(33, 61)], 5)
    aug.warp_stages(cpu, [0], [0], small.sizes, small.params)
    assert {k: (v.data_ptr(), v.numel()) for k, v in aug._buffers.items()} == before
    big = E.compose_batch(MIXED_SOURCES + MIXED_SOURCES, 12)
    aug.warp_stages(cpu, [0] * 8, [0] * 8, big.sizes, big.params)
    assert all(aug._buffers[k].numel() >= before[k][1] for k in before) and aug._buffers[(cpu, "translate")].numel() > before[(cpu, "translate")][1]
    # no pass without a taker
    none = E.compose_batch(E.SMALL_SOURCES, 1, [0.0] * 4)
    assert [s[0] for s in E.compose_aug().warp_stages(cpu, [0] * 4, [0] * 4, none.sizes, none.params)[0]] == ["translate"]


# ------------------------------------------------------------------------------------------------ shared pieces
def _report(fails, ran, want):
    assert ran == want, (ran, want)
    assert not fails, f"{len(fails)} of {ran}:\n" + "\n".join(fails[:12])


def _judge(fails, who, got, want):
    """The judgement of tests/test_gpu_augment.py::_check on (fp32, labels, bytes) of a whole batch."""
    im, lb, u8 = (t.cpu().numpy() for t in got)
    db, dl = int((u8 != want[2]).sum()), int((lb != want[1]).sum())
    ulp = ulp_distance(im, want[0]) if np.isfinite(im).all() else -1
    if db or dl or not 0 <= ulp <= 1:
        fails.append(f"{who}: {db} differing bytes, {dl} differing labels, fp32 max {ulp} ulp")


def _guarded(numel, dtype, fill, offset=0):
    """A dense 1-d view of `numel` elements, PAD + offset elements into an allocation filled with `fill`, and the allocation."""
    big = torch.full((numel + 2 * PAD + 4,), fill, dtype=dtype, device=DEV)
    assert big.data_ptr() % 16 == 0
    return big[PAD + offset:PAD + offset + numel], big


def _untouched(big, offset, numel, fill):
    head, tail = big[:PAD + offset], big[PAD + offset + numel:]
    same = (lambda t: bool(torch.isnan(t).all())) if isinstance(fill, float) else (lambda t: bool((t == fill).all()))
    return same(head) and same(tail)


def _through_device_augment(fails, who, b, aug=None):
    """DeviceAugment on the device into NaN / -1 outputs inside poisoned allocations; judged against the numpy route."""
    aug = b.aug if aug is None else aug
    N, th, tw = len(b.sizes), aug.th, aug.tw
    im, big_im = _guarded(N * 3 * th * tw, torch.float32, float("nan"))
    lb, big_lb = _guarded(N * th * tw, torch.int64, -1)
    images, labels = b.tensors(DEV)
    got = aug(images, labels, params=b.params, noise=b.noise_tensor(DEV), out=(im.view(N, 3, th, tw), lb.view(N, th, tw)), return_uint8=True)
    _judge(fails, who, got, b.host())
    if not (_untouched(big_im, 0, im.numel(), float("nan")) and _untouched(big_lb, 0, lb.numel(), -1)):
        fails.append(f"{who}: a value outside the outputs moved")
    return got


def _raw_k18(b, im, lb, u8):
    """cabinet_augment_batch itself: the table from build_table, a 0xFF workspace, the outputs as given."""
    import ctypes

    from cabinet_amd import _lib

    lib, aug = _lib.load(), b.aug
    N, th, tw = len(b.sizes), aug.th, aug.tw
    images, labels = b.tensors(DEV)
    table = torch.from_numpy(aug.build_table([t.data_ptr() for t in images], [t.data_ptr() for t in labels], b.sizes, b.params)).to(DEV)
    ws = torch.full((lib.cabinet_augment_workspace_bytes(N, th, tw),), 0xFF, dtype=torch.uint8, device=DEV)
    noise = b.noise_tensor(DEV)
    m3, s3 = (ctypes.c_float * 3)(*aug.mean), (ctypes.c_float * 3)(*aug.std)
    rc = lib.cabinet_augment_batch(table.data_ptr(), N, th, tw, noise.data_ptr() if noise is not None else None, 0, ctypes.addressof(m3),
                                   ctypes.addressof(s3), im.data_ptr(), lb.data_ptr(), u8.data_ptr(), ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cabinet_augment_batch")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. A: K18 on the GPU
@gpu
@pytest.mark.parametrize("name", list(E.K18_CASES))
def test_k18_plan_case_equals_the_host_route(name):
    fails = []
    _through_device_augment(fails, name, E.k18_case(name))
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("block", range(len(E.SWEEP_TH_BLOCKS)), ids=["th%d-%d" % (b[0], b[-1]) for b in E.SWEEP_TH_BLOCKS])
def test_k18_residue_sweep(block):
    """tw = 1..67 and 126..131 at each th of the block, two sources of different sizes under the Cityscapes preset: every
    residue of th mod 16 and tw mod 64 around one and two tiles, every `cnt`, noise given."""
    fails, ran = [], 0
    for th in E.SWEEP_TH_BLOCKS[block]:
        for tw in E.SWEEP_TW:
            found = E.sweep_case(tw, th)
            assert found is not None, f"crop {(tw, th)}: no seed of {E.SWEEP_SEEDS} gives params that supported() takes"
            _through_device_augment(fails, f"crop {(tw, th)} seed {found[1]}", found[0])
            ran += 1
    _report(fails, ran, 73 * len(E.SWEEP_TH_BLOCKS[block]))


@gpu
@pytest.mark.parametrize("res", range(4))
def test_k18_every_store_pairing_inside_poisoned_allocations(res):
    """P % 4 == res with out_image 0..3 elements and out_u8 0..3 bytes past a 16-byte boundary, through the raw C ABI: the
    f32x4 / scalar plane store with the packed / byte-wise store of the final bytes in all four pairings, and no value around
    an output moves."""
    b = E.poison_case(res)
    want = b.host()
    N, th, tw = 2, b.aug.th, b.aug.tw
    fails, ran, seen = [], 0, set()
    for f in range(4):
        for u in range(4):
            im, big_im = _guarded(N * 3 * th * tw, torch.float32, float("nan"), f)
            lb, big_lb = _guarded(N * th * tw, torch.int64, -1, f)
            u8, big_u8 = _guarded(N * th * tw * 3, torch.uint8, 0xFF, u)
            assert im.data_ptr() % 16 == 4 * f and u8.data_ptr() % 4 == u
            _raw_k18(b, im, lb, u8)
            who = f"P % 4 = {res}, out_image + {f}, out_u8 + {u}"
            _judge(fails, who, (im.view(N, 3, th, tw), lb.view(N, th, tw), u8.view(N, th, tw, 3)), want)
            if not (_untouched(big_im, f, im.numel(), float("nan")) and _untouched(big_lb, f, lb.numel(), -1) and _untouched(big_u8, u, u8.numel(), 0xFF)):
                fails.append(f"{who}: a value outside the outputs moved")
            seen |= E.store_pairings(th * tw, N, f, u)
            ran += 1
    assert seen == {(a, c) for a in (False, True) for c in (False, True)}
    _report(fails, ran, 16)


# ------------------------------------------------------------------------------------------------ 3. B: the K20 passes
def _run_pass(entry, items):
    """One launch of cabinet_augment_warp_batch / _resize_batch for `items`: every output at an ODD byte offset inside one
    0xFF-filled allocation.  Returns [(image, label)] and whether every byte outside them is still 0xFF."""
    from cabinet_amd import _lib
    from cabinet_amd.augment import warp_descs

    lib = _lib.load()
    keep, descs, spans, off = {}, [], [], 1
    for it in items:
        key = id(it["image"])
        if key not in keep:
            keep[key] = (torch.from_numpy(it["image"]).to(DEV), torch.from_numpy(it["label"]).to(DEV))
        px = it["out_h"] * it["out_w"]
        a, b = off, (off + 3 * px + 6) | 1
        spans.append((a, b, px))
        off = (b + px + 4) | 1
        descs.append(dict({k: v for k, v in it.items() if k in ("H", "W", "out_h", "out_w", "a", "flip", "fill", "resize")},
                          src_image=keep[key][0].data_ptr(), src_label=keep[key][1].data_ptr()))
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
    return outs, bool((got[~owned] == 0xFF).all())


def _pass_check(entry, items, oracle, what):
    outs, clean = _run_pass(entry, items)
    fails = [] if clean else [f"{what}: a byte outside the outputs moved"]
    for it, (gi, gl) in zip(items, outs):
        wi, wl = oracle(it)
        db, dl = int((gi != wi).sum()), int((gl != wl).sum())
        if db or dl:
            fails.append(f"{what} {it['H']}x{it['W']} -> {it['out_h']}x{it['out_w']} {it.get('kind', '')} a={it.get('a')} flip={it.get('flip')}: "
                         f"{db} differing bytes, {dl} differing labels")
    _report(fails, len(outs), len(items))


@gpu
@pytest.mark.parametrize("group", range(len(E.RESIZE_GROUPS)), ids=["oh%d-%d" % (g[0], g[-1]) for g in E.RESIZE_GROUPS])
def test_resize_pass_residue_sweep(group):
    """44 or 55 items of different extents in one launch: oh over the block, ow in 1..3, 62..66, 127..129, the ratio of each
    axis on its own from just above 1 to 2.5 exactly."""
    _pass_check("cabinet_augment_resize_batch", E.resize_group(E.RESIZE_GROUPS[group]), E.resize_oracle, "resize")


@gpu
def test_resize_pass_one_pixel_beside_a_large_output():
    items = E.resize_mixed()
    assert E.warp_outside(items, E.AUG_TX, E.AUG_TY)[0] == 5
    _pass_check("cabinet_augment_resize_batch", items, E.resize_oracle, "resize 1x1 beside 47x96")


@gpu
@pytest.mark.parametrize("shape", E.WARP_SHAPES, ids=["%dx%d" % s for s in E.WARP_SHAPES])
def test_warp_pass_around_its_tile(shape):
    """92 items in one launch at an output one under, on and one over the 32 x 8 tile (and two tiles wide): translates by
    fractions, integers, +-0.25 and +- the size, rotations by +-0.01, +-44.99 and +-45 degrees, scales 0.5 and 1.7 alone (label
    tables with a step) and with a shear of 0.3 (fixed point), each under all four flips."""
    _pass_check("cabinet_augment_warp_batch", E.warp_group(shape), E.warp_oracle, "warp")


@gpu
@pytest.mark.parametrize("size", E.EXPAND_SOURCES, ids=["%dx%d" % s for s in E.EXPAND_SOURCES])
def test_rotate_pass_with_expanded_outputs(size):
    _pass_check("cabinet_augment_warp_batch", E.expand_group(size), E.warp_oracle, "rotate(expand)")


@gpu
def test_warp_pass_one_pixel_beside_a_large_output():
    """A 1 x 1 output (label tables) beside a 97 x 200 one (fixed point): 90 of the small item's 91 workgroups leave at once."""
    items = E.warp_mixed()
    assert E.warp_outside(items, E.WARP_TX, E.WARP_TY)[0] == 90
    _pass_check("cabinet_augment_warp_batch", items, E.warp_oracle, "warp 1x1 beside 97x200")


# ------------------------------------------------------------------------------------------------ 4. C: the composition
def _call(aug, b, out=None):
    images, labels = b.tensors(DEV)
    return aug(images, labels, params=b.params, noise=b.noise_tensor(DEV), out=out, return_uint8=True)


def _compose_check(fails, who, b, got):
    """`got` against the numpy route and, bit for bit, against a fresh object's result."""
    _judge(fails, who, got, b.host())
    fresh = _call(E.compose_aug(), b)
    if not all(torch.equal(g, f) for g, f in zip(got, fresh)):
        fails.append(f"{who}: not the bits of a fresh DeviceAugment")


@gpu
@pytest.mark.parametrize("name,sizes,angles,passes", [
    ("no-sample-resizes", E.SMALL_SOURCES, None, ["translate", "rotate"]),
    ("all-resize", E.LARGE_SOURCES, None, ["resize", "translate", "rotate"]),
    ("only-1-and-3-rotate", MIXED_SOURCES, MIXED_ANGLES, ["resize", "translate", "rotate"]),
    ("nothing-rotates", E.SMALL_SOURCES, [0.0] * 4, ["translate"])])
def test_composition_of_passes_some_samples_take(name, sizes, angles, passes):
    b = E.compose_batch(sizes, 21, angles)
    aug = E.compose_aug()
    plans = [[("resize" if st.get("resize") else "rotate" if st["a"][1] != 0 else "translate") for st in aug.warp_plan(s, p)] for s, p in zip(b.sizes, b.params)]
    assert [n for n in ("resize", "translate", "rotate") if any(n in pl for pl in plans)] == passes
    if angles is not None:
        assert [("rotate" in pl) for pl in plans] == [a != 0.0 for a in angles]
    fails = []
    _compose_check(fails, name, b, _call(aug, b))
    _compose_check(fails, name + " again", b, _call(aug, b))
    _report(fails, 1, 1)


@gpu
def test_composition_buffers_grow_and_are_reused_oversized():
    """One object: a batch of 1, then 6 large sources, then 1 again -- the cached pass buffers grow, then hold a smaller batch."""
    aug = E.compose_aug()
    one = E.compose_batch([(97, 200)], 31)
    six = E.compose_batch(E.LARGE_SOURCES + [(200, 190), (190, 200)], 32)
    fails, sizes = [], []
    for who, b in (("1", one), ("6", six), ("1 again", one)):
        _compose_check(fails, who, b, _call(aug, b))
        sizes.append({k[1]: (v.numel(), v.data_ptr()) for k, v in aug._buffers.items()})
    assert set(sizes[0]) == {"resize", "translate", "rotate"}
    assert all(sizes[1][k][0] > sizes[0][k][0] for k in sizes[0]) and sizes[2] == sizes[1], sizes
    _report(fails, 1, 1)


@gpu
def test_composition_two_calls_queued_on_one_stream():
    """Two calls with different batches queued back to back on a non-default stream, no synchronisation between them, each
    into its own `out=`: the second call's passes run in the buffers the first call's launches still read."""
    aug = E.compose_aug()
    a, b = E.compose_batch(E.LARGE_SOURCES, 41), E.compose_batch(MIXED_SOURCES, 42, MIXED_ANGLES)
    th, tw = aug.th, aug.tw
    ins = [(x.tensors(DEV), x.noise_tensor(DEV)) for x in (a, b)]
    outs = [(torch.full((4, 3, th, tw), float("nan"), device=DEV), torch.full((4, th, tw), -1, dtype=torch.int64, device=DEV)) for _ in range(2)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    got = []
    with torch.cuda.stream(stream):
        for x, ((images, labels), noise), out in zip((a, b), ins, outs):
            got.append(aug(images, labels, params=x.params, noise=noise, out=out, return_uint8=True))
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    fails = []
    for who, x, g, out in zip(("first", "second"), (a, b), got, outs):
        assert g[0] is out[0] and g[1] is out[1]
        _compose_check(fails, who, x, g)
    _report(fails, 1, 1)


@gpu
def test_composition_out_tensors_reused_across_calls():
    aug = E.compose_aug()
    th, tw = aug.th, aug.tw
    out = (torch.full((4, 3, th, tw), float("nan"), device=DEV), torch.full((4, th, tw), -1, dtype=torch.int64, device=DEV))
    fails = []
    for who, b in (("small", E.compose_batch(E.SMALL_SOURCES, 51)), ("large", E.compose_batch(E.LARGE_SOURCES, 52)), ("small again", E.compose_batch(E.SMALL_SOURCES, 51))):
        got = _call(aug, b, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _compose_check(fails, who, b, tuple(t.clone() for t in got))
    _report(fails, 1, 1)


# ------------------------------------------------------------------------------------------------ 5. D: caller contract
@gpu
@pytest.mark.parametrize("name", ["upscale-2-reversed", "hsv-mixed-batch"])
def test_inputs_as_views_give_the_dense_calls_bits(name):
    """Image and label as a column slice of a wider tensor and as a tensor one byte into its storage."""
    b = E.k18_case(name)
    images, labels = b.tensors(DEV)
    noise = b.noise_tensor(DEV)
    base = b.aug(images, labels, params=b.params, noise=noise, return_uint8=True)

    def sliced(t):
        wide = torch.zeros((t.shape[0], t.shape[1] + 5) + tuple(t.shape[2:]), dtype=t.dtype, device=DEV)
        wide[:, 3:3 + t.shape[1]] = t
        v = wide[:, 3:3 + t.shape[1]]
        assert not v.is_contiguous() or t.shape[0] == 1
        return v

    def one_byte_in(t):
        v = torch.empty(t.numel() + 1, dtype=torch.uint8, device=DEV)[1:].view(t.shape).copy_(t)
        assert v.data_ptr() % 2 == 1 and v.is_contiguous()
        return v

    for what, form in (("a column slice", sliced), ("one byte into the storage", one_byte_in)):
        got = b.aug([form(t) for t in images], [form(t) for t in labels], params=b.params, noise=noise, return_uint8=True)
        assert all(torch.equal(g, w) for g, w in zip(got, base)), what
    fails = []
    _judge(fails, name, base, b.host())
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("name,crop,kw,change,error,match", [
    ("ratio-above-2.5", (16, 16), dict(scales=(0.3,)), dict(scale=0.3, w=22, h=12), RuntimeError, "RandomScale: ratio above 2.5"),
    ("pad-at-resized-size", (45, 80), {}, {}, RuntimeError, "padding: RandomCrop's reflect pad >= the resized size"),
    ("cutout-outside-the-crop", (45, 37), dict(cutout_size=8), dict(cutout=(30, 0)), ValueError, "cutout square outside the crop")])
def test_refused_inputs_leave_out_unchanged_and_name_the_step(name, crop, kw, change, error, match):
    aug = E.k18_aug(crop, **kw)
    image, label = E.source((40, 72))
    p = dataclasses.replace(aug.draw([(40, 72)], random.Random(3))[0], **dict(E.NEUTRAL, **change))
    tw, th = crop
    im, big_im = _guarded(3 * th * tw, torch.float32, float("nan"))
    lb, big_lb = _guarded(th * tw, torch.int64, -1)
    with pytest.raises(error, match=match):
        aug([torch.from_numpy(image).to(DEV)], [torch.from_numpy(label).to(DEV)], params=[p], out=(im.view(1, 3, th, tw), lb.view(1, th, tw)))
    with pytest.raises(error, match=match):                         # the host route refuses the same sample
        aug([torch.from_numpy(image)], [torch.from_numpy(label)], params=[p])
    torch.cuda.synchronize()
    assert bool(torch.isnan(big_im).all()) and bool((big_lb == -1).all()), "a refused call changed out="
