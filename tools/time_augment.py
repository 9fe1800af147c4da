#!/usr/bin/env python3
"""Time the device-side training augmentation (K18, csrc/augment.hip) on one GPU.

    python tools/time_augment.py [--reps 30] [--bench-json FILE] [--cpu-samples 2] [--out profiles/augment_time.json]

Batches of 8 crops of 1024 x 1024 from device-resident 1024 x 2048 uint8 sources (random bytes, labels 0..33), the reference's
default Cityscapes pipeline: one case per scale (every sample of the batch at that scale, every photometric step switched on, so
that each case does the most work a batch can ask for) and `mix`, whose parameters are drawn as the reference draws them.

Per case:
  kernels_us   device time of the two launches of cabinet_augment_batch: the call captured into a hipGraph with its table already
               on the device, events around --reps replays, median [min, max]
  call_us      DeviceAugment.__call__ as a user makes it: the per-sample tables assembled on the host, one host-to-device copy of
               them, the two launches; host clock around a call that ends in a device synchronise
  bytes        what the two kernels must move, from the shapes: the source rows and columns the crop window covers (image and
               label), the uint8 crop written and read back, int64 labels and fp32 planes written
  hbm_fraction bytes / kernels_us over the 8 TB/s of BASELINE.md
Where Pillow is importable the same sequence runs through Pillow / numpy calls on one core for --cpu-samples samples per case
(`cpu_pillow_ms_per_sample`, a CPU baseline, not the reference's loader: decoding and worker processes are not in it).

--bench-json names a file whose last line is the JSON line of `python bench.py --gpus 1 ...` taken in the same session: the
structural condition is that one batch costs less than the step it feeds (`batch_below_step`), reported as measured.
One JSON line (also written to --out).

--aerial times the aerial datasets' pipeline instead (K20, csrc/augment_warp.hip; written to profiles/augment_aerial_time.json
with --out): batches of 8 crops of 1024 x 1024 from device-resident 2160 x 3840 sources with the UAVid defaults -- `mix`, drawn
as the reference draws, and `widest`, every sample at the largest rotation and scale with every photometric step on.  Per case
each launch (resize, translate, rotate, and the two of cabinet_augment_batch together) is replayed from a graph of its own
between events, with the bytes its shapes move against 8 TB/s; call_us is the whole DeviceAugment call on the host clock.

--profile CASE launches that case's batch twenty times and exits: the split between the two kernels comes from
`rocprofv3 --kernel-trace --stats -- python tools/time_augment.py --profile CASE`, a run of its own.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SCALES = (0.75, 1.0, 1.25, 1.5, 1.75, 2.0)
H, W, TH, TW, N = 1024, 2048, 1024, 1024, 8
HBM_TBPS = 8.0


def _stats(v, nd=1):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def batch_bytes(params):
    """Algorithmic bytes of the two kernels for these samples."""
    total = 0
    for p in params:
        cols, rows = min(TW, p.w) / p.w * W, min(TH, p.h) / p.h * H       # the part of the source under the crop window
        total += cols * rows * (3 + 1)                                     # image and label bytes read
        total += 2 * TH * TW * 3 + TH * TW * 8 + 3 * TH * TW * 4           # crop out and back in, labels, planes
    return int(total)


def worst_case_params(aug, scale, rng):
    """Every sample at `scale`, every photometric step on."""
    from cabinet_amd.augment import SampleParams

    out = []
    for _ in range(N):
        w, h = int(round(W * scale)), int(round(H * scale))
        out.append(SampleParams(flip=rng.random() < 0.5, scale=scale, w=w, h=h, sw=rng.randint(0, max(w - TW, 0)),
                                sh=rng.randint(0, max(h - TH, 0)), brightness=rng.uniform(0.5, 1.5), contrast=rng.uniform(0.5, 1.5),
                                saturation=rng.uniform(0.5, 1.5), gray=False, gamma=rng.uniform(0.8, 1.2), noise=True,
                                cutout=(rng.randint(0, TH - 64), rng.randint(0, TW - 64))))
    return out


def pillow_sample(image, label, p, aug, gen):
    """The reference's sequence for one sample with the drawn parameters, through Pillow and numpy calls."""
    from PIL import Image, ImageEnhance

    im, lb = Image.fromarray(image), Image.fromarray(label)
    if p.flip:
        im, lb = im.transpose(Image.FLIP_LEFT_RIGHT), lb.transpose(Image.FLIP_LEFT_RIGHT)
    im, lb = im.resize((p.w, p.h), Image.BILINEAR), lb.resize((p.w, p.h), Image.NEAREST)
    pw, ph = max(TW - p.w, 0), max(TH - p.h, 0)
    if pw or ph:
        im = Image.fromarray(np.pad(np.array(im), ((0, ph), (0, pw), (0, 0)), mode="reflect"))
        lb = Image.fromarray(np.pad(np.array(lb), ((0, ph), (0, pw)), constant_values=255).astype(np.uint8))
    box = (p.sw, p.sh, p.sw + TW, p.sh + TH)
    im, lb = im.crop(box), lb.crop(box)
    im = ImageEnhance.Brightness(im).enhance(p.brightness)
    im = ImageEnhance.Contrast(im).enhance(p.contrast)
    im = ImageEnhance.Color(im).enhance(p.saturation)
    if p.gray:
        im = im.convert("L").convert("RGB")
    a = np.array(im)
    if p.gamma is not None:
        a = (np.clip((a.astype(np.float32) / 255.0) ** p.gamma, 0, 1) * 255).astype(np.uint8)
    if p.noise:
        a = np.clip(a.astype(np.float32) + gen.normal(0, aug.noise_sigma * 255, a.shape), 0, 255).astype(np.uint8)
    if p.cutout is not None:
        a[p.cutout[0]:p.cutout[0] + 64, p.cutout[1]:p.cutout[1] + 64, :] = 0
    t = torch.from_numpy(a).permute(2, 0, 1).contiguous().float().div(255)
    t = t.sub(torch.tensor(aug.mean).view(3, 1, 1)).div(torch.tensor(aug.std).view(3, 1, 1))
    return t, torch.from_numpy(aug.label_lut[np.array(lb, dtype=np.int64)])


def pillow_aerial_sample(image, label, p, aug, gen):
    """The aerial datasets' sequence for one sample with the drawn parameters, through Pillow and numpy calls."""
    from PIL import Image, ImageEnhance

    im, lb = Image.fromarray(image), Image.fromarray(label)
    if p.resized is not None:
        im, lb = im.resize(p.resized[::-1], Image.BILINEAR), lb.resize(p.resized[::-1], Image.NEAREST)
    if p.flip:
        im, lb = im.transpose(Image.FLIP_LEFT_RIGHT), lb.transpose(Image.FLIP_LEFT_RIGHT)
    if p.vflip:
        im, lb = im.transpose(Image.FLIP_TOP_BOTTOM), lb.transpose(Image.FLIP_TOP_BOTTOM)
    m = (1, 0, p.dx, 0, 1, p.dy)
    im = im.transform(im.size, Image.AFFINE, m, resample=Image.BILINEAR)
    lb = lb.transform(lb.size, Image.AFFINE, m, resample=Image.NEAREST, fillcolor=255)
    im = im.rotate(p.angle, resample=Image.BILINEAR, expand=True)
    lb = lb.rotate(p.angle, resample=Image.NEAREST, expand=True, fillcolor=255)
    im, lb = im.resize((p.w, p.h), Image.BILINEAR), lb.resize((p.w, p.h), Image.NEAREST)
    pw, ph = max(TW - p.w, 0), max(TH - p.h, 0)
    if pw or ph:
        im = Image.fromarray(np.pad(np.array(im), ((0, ph), (0, pw), (0, 0)), mode="reflect"))
        lb = Image.fromarray(np.pad(np.array(lb), ((0, ph), (0, pw)), constant_values=255).astype(np.uint8))
    box = (p.sw, p.sh, p.sw + TW, p.sh + TH)
    im, lb = im.crop(box), lb.crop(box)
    hsv = np.array(im.convert("HSV"), dtype=np.int16)
    hsv[..., 0] = (hsv[..., 0] + round(p.hsv[0] * 255)) % 255
    hsv[..., 1] = np.clip(hsv[..., 1] * (p.hsv[1] + 1), 0, 255)
    hsv[..., 2] = np.clip(hsv[..., 2] * (p.hsv[2] + 1), 0, 255)
    hsv = hsv.astype(np.uint8)
    im = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(hsv[..., c])) for c in range(3)]).convert("RGB")
    im = ImageEnhance.Contrast(im).enhance(p.contrast)
    a = np.array(im)
    if p.gamma is not None:
        a = (np.clip((a.astype(np.float32) / 255.0) ** p.gamma, 0, 1) * 255).astype(np.uint8)
    if p.noise:
        a = np.clip(a.astype(np.float32) + gen.normal(0, aug.noise_sigma * 255, a.shape), 0, 255).astype(np.uint8)
    if p.cutout is not None:
        a[p.cutout[0]:p.cutout[0] + 64, p.cutout[1]:p.cutout[1] + 64, :] = 0
    t = torch.from_numpy(a).permute(2, 0, 1).contiguous().float().div(255)
    t = t.sub(torch.tensor(aug.mean).view(3, 1, 1)).div(torch.tensor(aug.std).view(3, 1, 1))
    return t, torch.from_numpy(np.array(lb, dtype=np.int64))


AH, AW = 2160, 3840


def _graph_times(launch, reps, warmup):
    """Device time of `launch` replayed from a graph of its own between events, per replay, in microseconds."""
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        launch()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main_aerial(a):
    import ctypes
    import dataclasses

    from cabinet_amd import _lib
    from cabinet_amd.augment import DeviceAugment, rotate_matrix

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    gen = np.random.RandomState(0)
    aug = DeviceAugment.uavid(cropsize=(TW, TH))
    host_images = [gen.randint(0, 256, size=(AH, AW, 3)).astype(np.uint8) for _ in range(N)]
    host_labels = [gen.randint(0, 8, size=(AH, AW)).astype(np.uint8) for _ in range(N)]
    images = [torch.from_numpy(x).to(dev) for x in host_images]
    labels = [torch.from_numpy(x).to(dev) for x in host_labels]
    im = torch.empty((N, 3, TH, TW), device=dev)
    lb = torch.empty((N, TH, TW), dtype=torch.int64, device=dev)
    ws = torch.empty(lib.cabinet_augment_workspace_bytes(N, TH, TW), dtype=torch.uint8, device=dev)
    m3, s3 = (ctypes.c_float * 3)(*aug.mean), (ctypes.c_float * 3)(*aug.std)
    sizes = [(AH, AW)] * N
    rng = random.Random(0)
    cases = {"mix": aug.draw(sizes, rng)}
    widest = []
    for j, p in enumerate(aug.draw(sizes, rng)):   # the largest rotated size and scale, every photometric step on
        angle = 10.0 if j % 2 else -10.0
        _, nw, nh = rotate_matrix(p.resized[1], p.resized[0], angle)
        w, h = int(round(nw * 1.3)), int(round(nh * 1.3))
        widest.append(dataclasses.replace(p, angle=angle, warped=(nh, nw), scale=1.3, w=w, h=h, sw=rng.randint(0, w - TW),
                                          sh=rng.randint(0, h - TH), gamma=rng.uniform(0.8, 1.2), noise=True,
                                          cutout=(rng.randint(0, TH - 64), rng.randint(0, TW - 64))))
    cases["widest"] = widest
    try:
        import PIL  # noqa: F401
        have_pillow = True
    except ImportError:
        have_pillow = False
    out = {"tool": "time_augment --aerial", "device": torch.cuda.get_device_name(0), "batch": N, "source": [AH, AW], "crop": [TH, TW],
           "reps": a.reps, "hbm_tbps": HBM_TBPS, "pipeline": "DeviceAugment.uavid defaults", "cases": {}}
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731  (asked per launch: a capture runs on a stream of its own)
    for name, params in cases.items():
        stages, im_ptrs, lb_ptrs = aug.warp_stages(dev, [t.data_ptr() for t in images], [t.data_ptr() for t in labels], sizes, params)
        ksizes = [p.warped for p in params]
        table = torch.from_numpy(aug.build_table(im_ptrs, lb_ptrs, ksizes, params)).to(dev)

        def launch_batch():
            rc = lib.cabinet_augment_batch(table.data_ptr(), N, TH, TW, None, 7, ctypes.addressof(m3), ctypes.addressof(s3), im.data_ptr(),
                                           lb.data_ptr(), None, ws.data_ptr(), ws.numel(), stream())
            _lib.check(rc, "cabinet_augment_batch")

        launches = []
        for sname, entry, descs, n, mh, mw, items in stages:
            nbytes = sum(4 * (it["H"] * it["W"] + it["out_h"] * it["out_w"]) for it in items)   # image + label read once, written once
            launches.append((sname, (lambda e=entry, d=descs, n=n, mh=mh, mw=mw: _lib.check(getattr(lib, e)(d.data_ptr(), n, mh, mw, stream()), e)), nbytes))
        kbytes = 0
        for p in params:
            cols, rows = min(TW, p.w) / p.w * p.warped[1], min(TH, p.h) / p.h * p.warped[0]
            kbytes += int(cols * rows * 4 + 2 * TH * TW * 3 + TH * TW * 8 + 3 * TH * TW * 4)
        launches.append(("scale_crop_photo", launch_batch, kbytes))
        if a.profile:
            if name == a.profile:
                for _ in range(20):
                    for _, fn, _ in launches:
                        fn()
                torch.cuda.synchronize()
            continue
        case = {"angles": [round(p.angle, 2) for p in params], "scales": [round(p.scale, 3) for p in params],
                "warped": [list(p.warped) for p in params], "launches": {}}
        total_us = total_bytes = 0.0
        for sname, fn, nbytes in launches:   # in pipeline order: each launch reads what the one before it left
            us = _graph_times(fn, a.reps, a.warmup)
            med = statistics.median(us)
            case["launches"][sname] = {"us": _stats(us), "bytes_MB": round(nbytes / 1e6, 1), "us_at_hbm_rate": round(nbytes / (HBM_TBPS * 1e6), 1),
                                       "hbm_fraction": round(nbytes / (HBM_TBPS * 1e6) / med, 3)}
            total_us, total_bytes = total_us + med, total_bytes + nbytes
        case["sum_of_medians_us"] = round(total_us, 1)
        case["bytes_MB"] = round(total_bytes / 1e6, 1)
        case["hbm_fraction"] = round(total_bytes / (HBM_TBPS * 1e6) / total_us, 3)
        calls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            aug(images, labels, params=params, seed=7, out=(im, lb))
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e6)
        case["call_us"] = _stats(calls)
        if have_pillow and a.cpu_samples > 0:
            torch.set_num_threads(1)
            ms = []
            for j in range(min(a.cpu_samples, N)):
                t0 = time.perf_counter()
                pillow_aerial_sample(host_images[j], host_labels[j], params[j], aug, gen)
                ms.append((time.perf_counter() - t0) * 1e3)
            case["cpu_pillow_ms_per_sample"] = _stats(ms, 1)
            case["cpu_pillow_what"] = "CPU baseline: the same sequence through Pillow / numpy calls on one core, no decoding"
        else:
            case["cpu_pillow_ms_per_sample"] = "not measured"
        out["cases"][name] = case
    if a.profile:
        return
    if a.bench_json:
        with open(a.bench_json) as f:
            line = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")][-1]
        step_ms = float(json.loads(line)["ms_per_step"])
        worst_k = max(c["sum_of_medians_us"] for c in out["cases"].values())
        worst_c = max(c["call_us"]["median"] for c in out["cases"].values())
        out["step"] = {"ms_per_step": step_ms, "what": "bench.py --gpus 1 (BASELINE config 3, 8 x 3 x 1024 x 1024) in the same session; the "
                       "step's code is the parent commit's", "slowest_batch_kernels_us": worst_k, "slowest_batch_call_us": worst_c,
                       "batch_below_step": bool(worst_c < step_ms * 1e3), "kernels_share_of_step": round(worst_k / (step_ms * 1e3), 4)}
    else:
        out["step"] = "not measured"
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-samples", type=int, default=2)
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--profile", default=None, metavar="CASE", help="only launch this case's batch (scale_0.75 ... scale_2.0, mix) a few "
                    "times and exit, for rocprofv3 --kernel-trace --stats -- python tools/time_augment.py --profile mix")
    ap.add_argument("--out", default=None)
    ap.add_argument("--aerial", action="store_true", help="the aerial datasets' pipeline (K20) instead of the Cityscapes one")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_augment.py measures on a GPU; there is no CPU fallback"
    if a.aerial:
        return main_aerial(a)
    import ctypes

    from cabinet_amd import _lib
    from cabinet_amd.augment import DeviceAugment

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    gen = np.random.RandomState(0)
    lut = np.full(256, 255, dtype=np.int64)
    lut[:34] = gen.randint(0, 19, size=34)
    aug = DeviceAugment.cityscapes(cropsize=(TW, TH), label_map=lut)
    host_images = [gen.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(N)]
    host_labels = [gen.randint(0, 34, size=(H, W)).astype(np.uint8) for _ in range(N)]
    images = [torch.from_numpy(x).to(dev) for x in host_images]
    labels = [torch.from_numpy(x).to(dev) for x in host_labels]
    im = torch.empty((N, 3, TH, TW), device=dev)
    lb = torch.empty((N, TH, TW), dtype=torch.int64, device=dev)
    ws = torch.empty(lib.cabinet_augment_workspace_bytes(N, TH, TW), dtype=torch.uint8, device=dev)
    m3, s3 = (ctypes.c_float * 3)(*aug.mean), (ctypes.c_float * 3)(*aug.std)
    try:
        import PIL  # noqa: F401
        have_pillow = True
    except ImportError:
        have_pillow = False

    rng = random.Random(0)
    cases = {f"scale_{s}": worst_case_params(aug, s, rng) for s in SCALES}
    cases["mix"] = aug.draw([(H, W)] * N, rng)
    out = {"tool": "time_augment", "device": torch.cuda.get_device_name(0), "batch": N, "source": [H, W], "crop": [TH, TW],
           "reps": a.reps, "hbm_tbps": HBM_TBPS, "cases": {}}
    for name, params in cases.items():
        table = torch.from_numpy(aug.build_table([t.data_ptr() for t in images], [t.data_ptr() for t in labels], [(H, W)] * N, params)).to(dev)

        def launch():
            rc = lib.cabinet_augment_batch(table.data_ptr(), N, TH, TW, None, 7, ctypes.addressof(m3), ctypes.addressof(s3), im.data_ptr(),
                                           lb.data_ptr(), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "cabinet_augment_batch")

        if a.profile:
            if name == a.profile:
                for _ in range(20):
                    launch()
                torch.cuda.synchronize()
            continue
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            launch()
        kernels, calls = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            kernels.append(e0.elapsed_time(e1) * 1e3)
            t0 = time.perf_counter()
            aug(images, labels, params=params, seed=7, out=(im, lb))
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e6)
        nbytes = batch_bytes(params)
        case = {"scales": sorted({p.scale for p in params}), "kernels_us": _stats(kernels), "call_us": _stats(calls),
                "bytes_MB": round(nbytes / 1e6, 1), "us_at_hbm_rate": round(nbytes / (HBM_TBPS * 1e6), 1),
                "hbm_fraction": round(nbytes / (HBM_TBPS * 1e6) / statistics.median(kernels), 3)}
        if have_pillow and a.cpu_samples > 0:
            torch.set_num_threads(1)
            ms = []
            for j in range(min(a.cpu_samples, N)):
                t0 = time.perf_counter()
                pillow_sample(host_images[j], host_labels[j], params[j], aug, gen)
                ms.append((time.perf_counter() - t0) * 1e3)
            case["cpu_pillow_ms_per_sample"] = _stats(ms, 1)
            case["cpu_pillow_what"] = "CPU baseline: the same sequence through Pillow / numpy calls on one core, no decoding"
        else:
            case["cpu_pillow_ms_per_sample"] = "not measured"
        out["cases"][name] = case
    if a.profile:
        return
    if a.bench_json:
        with open(a.bench_json) as f:
            line = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")][-1]
        step_ms = float(json.loads(line)["ms_per_step"])
        worst_k = max(c["kernels_us"]["median"] for c in out["cases"].values())
        worst_c = max(c["call_us"]["median"] for c in out["cases"].values())
        out["step"] = {"ms_per_step": step_ms, "what": "bench.py --gpus 1 (BASELINE config 3, 8 x 3 x 1024 x 1024) in the same session; the "
                       "step's code is the parent commit's", "slowest_batch_kernels_us": worst_k, "slowest_batch_call_us": worst_c,
                       "batch_below_step": bool(worst_c < step_ms * 1e3), "kernels_share_of_step": round(worst_k / (step_ms * 1e3), 4)}
    else:
        out["step"] = "not measured"
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
