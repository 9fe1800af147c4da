"""cabinet_amd.predict on the CPU: the plain path against the reference's infer_image / colorize_mask (fixture g7_predict.npz,
tests/golden/make_golden_predict.py), the render contract in numpy against the reference's numpy / Pillow lines, and the
declarations of the three K17 entry points.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from predict_golden import CASES, load_case, load_render, render_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K17 = ("cabinet_predict_up_argmax_supported", "cabinet_predict_up_argmax", "cabinet_predict_argmax", "cabinet_predict_render")


@pytest.mark.parametrize("case", CASES)
def test_plain_infer_image_is_the_reference_bit_for_bit(case):
    from cabinet_amd.predict import infer_image

    g = load_case(case)
    pred = infer_image(g["model"], g["image"], num_classes=g["n_classes"], scales=list(g["scales"]), flip=g["flip"], device="cpu")
    assert isinstance(pred, np.ndarray) and pred.dtype == np.int64 and pred.shape == g["pred"].shape
    assert np.array_equal(pred, g["pred"])
    # `fused=False` is the same path, and the automatic choice on a CPU model is the plain path too
    again = infer_image(g["model"], g["image"], num_classes=g["n_classes"], scales=list(g["scales"]), flip=g["flip"], device="cpu",
                        fused=False)
    assert np.array_equal(again, g["pred"])


def test_infer_image_input_forms():
    from cabinet_amd.predict import infer_image

    g = load_case(2)
    chw = infer_image(g["model"], g["image"][0], num_classes=g["n_classes"], device="cpu")
    assert np.array_equal(chw, g["pred"])
    with pytest.raises(ValueError, match="batch size 1"):
        infer_image(g["model"], torch.cat([g["image"], g["image"]]), num_classes=g["n_classes"], device="cpu")
    with pytest.raises(RuntimeError, match="not on a GPU"):
        infer_image(g["model"], g["image"], num_classes=g["n_classes"], device="cpu", fused=True)


def test_colorize_mask_equals_the_reference():
    from cabinet_amd.predict import CITYSCAPES_COLORS, colorize_mask

    r = load_render()
    img = colorize_mask(r["labels"])
    assert img.mode == "RGB" and img.size == (r["labels"].shape[1], r["labels"].shape[0])
    assert np.array_equal(np.asarray(img), r["pred"])
    assert (r["labels"] == 255).any() and (r["labels"] >= 19).sum() > (r["labels"] == 255).sum()
    assert np.array_equal(np.asarray(colorize_mask(r["labels"].astype(np.int64)))[r["labels"] == 255][0], CITYSCAPES_COLORS[18])
    # a shorter palette clips at its own end
    short = np.asarray(colorize_mask(r["labels"], CITYSCAPES_COLORS[:7]))
    assert np.array_equal(short, CITYSCAPES_COLORS[np.minimum(r["labels"], 6)])


def test_render_contract_in_numpy_equals_the_reference():
    from cabinet_amd.predict import CITYSCAPES_COLORS, IMAGENET_MEAN, IMAGENET_STD

    r = load_render()
    assert np.array_equal(np.asarray(IMAGENET_MEAN, dtype=np.float32), r["mean"])
    assert np.array_equal(np.asarray(IMAGENET_STD, dtype=np.float32), r["std"])
    out = render_contract(r["labels"], r["image"], CITYSCAPES_COLORS, r["mean"], r["std"], float(r["alpha"]))
    for name in ("pred", "input", "overlay"):
        assert out[name].dtype == np.uint8 and np.array_equal(out[name], r[name]), name
    # the fixture exercises the clip on both sides and the truncation
    assert (r["input"] == 0).any() and (r["input"] == 255).any()
    # the arithmetic type is part of the contract: the same formula in double gives other bytes somewhere in this block
    d = r["input"].astype(np.float64) + 0.6 * (r["pred"].astype(np.float64) - r["input"].astype(np.float64))
    assert (d.astype(np.uint8) != r["overlay"]).any()


def test_predictor_plain_on_the_cpu_matches_the_contract():
    from cabinet_amd.predict import CITYSCAPES_COLORS, Predictor

    g, r = load_case(2), load_render()
    p = Predictor(g["model"], g["n_classes"])
    labels = p.predict(torch.cat([g["image"], g["image"].flip(3)]))
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (2, *g["pred"].shape)
    assert np.array_equal(labels[0].numpy(), g["pred"])
    out = p.render(torch.from_numpy(r["image"]), torch.from_numpy(r["labels"]))
    for name in ("pred", "input", "overlay"):
        assert out[name].dtype == torch.uint8 and np.array_equal(out[name][0].numpy(), r[name]), name
    own = p.render(g["image"])
    assert np.array_equal(own["pred"][0].numpy(), CITYSCAPES_COLORS[g["pred"]])
    g["model"].train()
    with pytest.raises(RuntimeError, match="training mode"):
        p.predict(g["image"])


def test_predictor_graph_on_a_cpu_model_raises():
    from cabinet_amd.predict import Predictor

    g = load_case(5)
    with pytest.raises(RuntimeError, match=r"graph=True.*GPU"):
        Predictor(g["model"], g["n_classes"], graph=True)


def test_visualize_predictions_writes_the_four_files(tmp_path):
    from PIL import Image

    from cabinet_amd.predict import CITYSCAPES_COLORS, visualize_predictions

    g = load_case(2)
    gt = torch.from_numpy(g["pred"]).clone()
    gt[:4] = 255
    n = visualize_predictions(g["model"], [(g["image"], gt[None]), (g["image"],)], tmp_path / "vis", "cpu",
                              num_classes=g["n_classes"])
    assert n == 2
    first = tmp_path / "vis" / "sample_0000"
    assert sorted(p.name for p in first.iterdir()) == ["gt.png", "input.png", "overlay.png", "pred.png"]
    assert sorted(p.name for p in (tmp_path / "vis" / "sample_0001").iterdir()) == ["input.png", "overlay.png", "pred.png"]
    want = render_contract(g["pred"], g["image"][0].numpy(), CITYSCAPES_COLORS, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 0.6)
    for name in ("pred", "input", "overlay"):
        assert np.array_equal(np.asarray(Image.open(first / f"{name}.png")), want[name]), name
    assert np.array_equal(np.asarray(Image.open(first / "gt.png")), CITYSCAPES_COLORS[np.minimum(gt.numpy(), 18)])


def test_the_three_entry_points_are_declared_and_typed():
    from cabinet_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "cabinet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in K17:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "visualize.py:50-61" in header and "visualize.py:113-114" in header and ":165-177" in header
    assert int(re.search(r"#define\s+CABINET_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == _lib.ABI_VERSION
    assert "predict_tail.hip" in build.SOURCES
    assert len(_lib.SIGNATURES["cabinet_predict_render"][1]) == 14 and len(_lib.SIGNATURES["cabinet_predict_up_argmax"][1]) == 9


def test_argument_errors_need_no_gpu():
    from cabinet_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    assert lib.cabinet_abi_version() == 8
    # LDS budget: every enlarging resize of up to 32 classes is taken; a strongly shrinking one of many classes is refused
    assert lib.cabinet_predict_up_argmax_supported(19, 128, 256, 1024, 2048) == 1
    assert lib.cabinet_predict_up_argmax_supported(32, 24, 40, 24, 40) == 1
    assert lib.cabinet_predict_up_argmax_supported(8, 40, 60, 25, 33) == 1
    assert lib.cabinet_predict_up_argmax_supported(33, 8, 8, 64, 64) == 0
    assert lib.cabinet_predict_up_argmax_supported(32, 64, 4096, 64, 512) == 0
    A = 0x10000
    assert lib.cabinet_predict_up_argmax(A, 1, 32, 64, 4096, 64, 512, A, None) == -2 and b"LDS" in lib.cabinet_last_error()
    assert lib.cabinet_predict_up_argmax(None, 1, 8, 4, 4, 32, 32, A, None) == -1 and b"null" in lib.cabinet_last_error()
    assert lib.cabinet_predict_argmax(A, 1, 40, 8, 8, A, None) == -2 and b"max 32" in lib.cabinet_last_error()
    assert lib.cabinet_predict_argmax(A + 4, 1, 8, 8, 8, A, None) == -1 and b"16-byte aligned" in lib.cabinet_last_error()
    assert lib.cabinet_predict_render(A, None, A, 19, None, None, 0.6, 1, 8, 8, A, A, None, None) == -1
    assert b"need the image" in lib.cabinet_last_error()
    assert lib.cabinet_predict_render(A, None, A, 300, None, None, 0.6, 1, 8, 8, A, None, None, None) == -1
    assert b"n_colors" in lib.cabinet_last_error()
    assert lib.cabinet_predict_render(A, None, A, 19, None, None, 1.5, 1, 8, 8, A, None, None, None) == -1
    assert b"alpha" in lib.cabinet_last_error()
