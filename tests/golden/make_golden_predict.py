#!/usr/bin/env python3
"""Generate the inference fixture tests/golden/g7_predict.npz by running the REFERENCE's infer_image and colorize_mask.

Run where a checkout of the reference exists (it never travels to the GPU box); CABINET_REFERENCE names it, the default is a
directory `reference` beside this repository:

    PYTHONDONTWRITEBYTECODE=1 [CABINET_REFERENCE=/path/to/CABiNet] python tests/golden/make_golden_predict.py

Per case: a stub model (tests/eval_golden.py: StubNet, weights stored), a random uint8 image, the reference's fp32 predictions,
and three things derived from the probability map the predictions are the argmax of, computed here in fp32 (its argmax must BE
the reference's predictions) and in float64: ref32_vs_f64_maxabs, the bit-packed mask of the undecided pixels (float64 top-two
margin below TIE_FACTOR x that distance) and their share.  The generator FAILS when that share exceeds 0.2 % of a case, when a
class does not occur, or when fp32 and float64 disagree on a decided pixel.

Render block: a normalised float32 image some of whose values de-normalise outside [0, 1], a label map with values >= 19 and
255, and the three uint8 arrays that the reference's colorize_mask, its de-normalisation arithmetic and PIL.Image.blend produce
at alpha 0.6.

Only data is written: inputs, expected outputs, seeds.  No reference source text.
"""

import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CABINET_REFERENCE", os.path.normpath(os.path.join(HERE, "..", "..", "..", "reference")))
sys.path.insert(0, os.path.dirname(HERE))   # tests/: eval_golden
sys.path.insert(0, REF)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules.setdefault(name, m)


# the reference's visualize.py imports its command-line stack, its dataset (which needs torchvision) and a progress bar at
# module level; none of them is needed to run the two functions
_stub("hydra", main=lambda *a, **k: (lambda fn: fn))
_stub("omegaconf", DictConfig=dict, OmegaConf=type("OmegaConf", (), {}))
_stub("src.datasets.cityscapes", CityScapes=object)
try:
    import tqdm  # noqa: F401
except ImportError:
    _stub("tqdm", tqdm=lambda it, **k: it)

from eval_golden import MAX_UNDECIDED_SHARE, TIE_FACTOR, StubNet, image_from_u8  # noqa: E402
from src.scripts.visualize import colorize_mask, infer_image  # noqa: E402

torch.set_num_threads(8)

#        C   H    W   scales            flip
CASES = {
    1: (19, 96, 136, (1.0,), False),            # the deployment setting
    2: (8, 70, 93, (1.0,), False),              # ragged: W % 4 = 1, H and W no multiple of 8
    3: (19, 96, 128, (0.5, 1.0, 1.5), True),
    4: (5, 64, 72, (0.75, 1.0), False),         # a class count without a compiled form
    5: (8, 40, 52, (1.0, 1.25), True),
}
SEED0 = 700


def summed_map(net, image, C, scales, flip):
    """The map infer_image takes the argmax of, in the default dtype."""
    H, W = image.shape[2:]
    probs = torch.zeros((1, C, H, W))
    with torch.no_grad():
        for s in scales:
            x = image if s == 1.0 else F.interpolate(image, size=[int(H * s), int(W * s)], mode="bilinear", align_corners=False)
            p = F.softmax(net(x)[0], dim=1)
            if flip:
                q = F.softmax(torch.flip(net(torch.flip(x, dims=(3,)))[0], dims=(3,)), dim=1)
                p = (p + q) / 2
            if s != 1.0:
                p = F.interpolate(p, size=(H, W), mode="bilinear", align_corners=False)
            probs += p
        probs /= len(scales)
    return probs


def render_block(out):
    g = torch.Generator().manual_seed(SEED0 + 99)
    H, W = 70, 93
    mean = np.array([0.485, 0.456, 0.406], dtype=np.float32)
    std = np.array([0.229, 0.224, 0.225], dtype=np.float32)
    rgb = torch.rand(3, H, W, generator=g).numpy().astype(np.float32) * 1.3 - 0.15     # some values leave [0, 1]
    image = ((rgb - mean[:, None, None]) / std[:, None, None]).astype(np.float32)
    labels = torch.randint(0, 19, (H, W), generator=g).numpy().astype(np.uint8)
    r = torch.rand(H, W, generator=g).numpy()
    labels[r < 0.05] = 255
    labels[(r >= 0.05) & (r < 0.08)] = 19
    labels[(r >= 0.08) & (r < 0.10)] = 37
    # the reference's lines: de-normalise, clip, * 255, astype(uint8); colorize_mask; Image.blend at alpha 0.6
    img_np = np.transpose(image, (1, 2, 0))
    img_np = (img_np * std + mean).clip(0.0, 1.0)
    img_np = (img_np * 255).astype(np.uint8)
    img_pil = Image.fromarray(img_np)
    color = colorize_mask(labels)
    overlay = Image.blend(img_pil, color, alpha=0.6)
    assert img_np.min() == 0 and img_np.max() == 255
    out.update(render_image=image, render_labels=labels, render_input=img_np, render_pred=np.asarray(color),
               render_overlay=np.asarray(overlay), render_alpha=np.float32(0.6), render_mean=mean, render_std=std)


def main():
    out = {}
    for k, (C, H, W, scales, flip) in CASES.items():
        g = torch.Generator().manual_seed(SEED0 + k)
        u8 = torch.randint(0, 256, (1, 3, H, W), generator=g, dtype=torch.uint8).numpy()
        image = image_from_u8(u8)
        net = StubNet(C)
        with torch.no_grad():
            net.conv.weight.copy_(torch.randn(net.conv.weight.shape, generator=g) * 0.19)
            net.conv.bias.copy_(torch.randn(C, generator=g) * 0.5)
        net.eval()
        pred = infer_image(net, image, num_classes=C, scales=list(scales), flip=flip, device="cpu")
        assert pred.shape == (H, W) and pred.dtype == np.int64
        assert np.array_equal(infer_image(net, image[0], num_classes=C, scales=list(scales), flip=flip, device="cpu"), pred)
        p32 = summed_map(net, image, C, scales, flip)
        assert np.array_equal(torch.argmax(p32, dim=1).numpy()[0], pred), "the restated map is not the reference's"
        torch.set_default_dtype(torch.float64)
        try:
            p64 = summed_map(copy.deepcopy(net).double(), image.double(), C, scales, flip)
        finally:
            torch.set_default_dtype(torch.float32)
        assert p64.dtype == torch.float64
        p32, p64 = p32.numpy()[0], p64.numpy()[0]
        maxabs = float(np.abs(p32.astype(np.float64) - p64).max())
        top2 = np.sort(p64, axis=0)[-2:]
        undecided = (top2[1] - top2[0]) < TIE_FACTOR * maxabs
        share = float(undecided.mean())
        wrong = int(((np.argmax(p64, axis=0) != pred) & ~undecided).sum())
        classes = np.unique(pred)
        print(f"case {k}: C={C} {H}x{W} scales={scales} flip={flip}  ref32_vs_f64_maxabs {maxabs:.3e}  undecided "
              f"{int(undecided.sum())} px ({share:.3e})  decided fp32/f64 disagreements {wrong}  classes seen {len(classes)}")
        assert share <= MAX_UNDECIDED_SHARE, f"case {k}: {share:.3e} of the pixels are undecided"
        assert wrong == 0 and len(classes) == C
        out.update({f"c{k}_{n}": v for n, v in dict(
            n_classes=C, scales=np.array(scales), flip=flip, seed=SEED0 + k, image_u8=u8, weight=net.conv.weight.detach().numpy(),
            bias=net.conv.bias.detach().numpy(), pred=pred.astype(np.uint8), ref32_vs_f64_maxabs=maxabs,
            undecided_bits=np.packbits(undecided), undecided_share=share).items()})
    render_block(out)
    path = os.path.join(HERE, "g7_predict.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 20
    print(f"wrote g7_predict.npz: {os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
