#!/usr/bin/env python3
"""Generate the evaluator fixture tests/golden/g5_eval*.npz by running the REFERENCE's MscEvalV0 itself.

Run where a checkout of the reference exists (it never travels to the GPU box); CABINET_REFERENCE names it, the default is the
place the sibling generators use:

    PYTHONDONTWRITEBYTECODE=1 [CABINET_REFERENCE=/path/to/CABiNet] python tests/golden/make_golden_eval.py

Per case: a stub model (tests/eval_golden.py: StubNet, weights stored), a random uint8 image, random labels with about 10 %
ignore_label and a few out-of-range values; the reference's summed probability map in fp32 and in float64 (default dtype
switched around a double copy of the stub), its predictions, confusion matrix, mIoU and accuracy, and two scalars derived from
the maps: ref32_vs_f64_maxabs and the share of pixels whose float64 top-two margin is below 5 x that (the tie margin of the
tests).  The generator FAILS when that share exceeds 0.2 % of a case.  Storage layout: tests/eval_golden.py.

Only data is written: inputs, expected outputs, seeds.  No reference source text.
"""

import copy
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("CABINET_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/: eval_golden
sys.path.insert(0, REF)

# the reference's evaluate.py imports its command-line stack and its dataset registry (which needs torchvision) at module
# level; none of them is needed to run the class
_registry = types.ModuleType("src.datasets.registry")
_registry.DATASET_KWARGS_BUILDERS, _registry.DATASET_REGISTRY = {}, {}
sys.modules.setdefault("src.datasets.registry", _registry)
_hydra = types.ModuleType("hydra")
_hydra.main = lambda *a, **k: (lambda fn: fn)
_omega = types.ModuleType("omegaconf")
_omega.DictConfig = dict
_omega.OmegaConf = type("OmegaConf", (), {})
sys.modules.setdefault("hydra", _hydra)
sys.modules.setdefault("omegaconf", _omega)

from eval_golden import MAX_UNDECIDED_SHARE, TIE_FACTOR, StubNet, image_from_u8  # noqa: E402
from src.scripts.evaluate import MscEvalV0  # noqa: E402

torch.set_num_threads(8)
IGNORE = 255
MAX_VALUES_PER_FILE = 160_000  # x (4 + 2) bytes: below 1 MiB

#        C   H    W   crop  scales             flip
CASES = {
    1: (8, 160, 224, 128, (0.75, 1.0, 1.5), True),    # several windows per axis, clamped last window, overlap counts 1, 2, 4
    2: (19, 96, 128, 128, (0.5, 1.0), False),         # padding branch; scaled image smaller than the crop in both axes
    3: (19, 160, 192, 128, (1.0, 1.25), True),
    4: (8, 96, 200, 128, (1.0, 0.75), True),          # H < crop <= W: the target-size rule
}


def summed_map(ev, image):
    """What evaluate() takes the argmax of (reference evaluate.py:213-218)."""
    with torch.no_grad():
        probs = torch.zeros((image.size(0), ev.n_classes, *image.shape[-2:]))
        for s in ev.scales:
            probs += ev.scale_crop_eval(image, s)
    return probs


def main():
    small = {}
    for k, (C, H, W, crop, scales, flip) in CASES.items():
        g = torch.Generator().manual_seed(500 + k)
        u8 = torch.randint(0, 256, (1, 3, H, W), generator=g, dtype=torch.uint8).numpy()
        image = image_from_u8(u8)
        labels = torch.randint(0, C, (1, H, W), generator=g)
        r = torch.rand(1, H, W, generator=g)
        labels[r < 0.10] = IGNORE
        labels[(r >= 0.10) & (r < 0.104)] = 200          # out of range: counted as class C - 1
        labels[(r >= 0.104) & (r < 0.108)] = C + 3
        net = StubNet(C)
        with torch.no_grad():
            net.conv.weight.copy_(torch.randn(net.conv.weight.shape, generator=g) * 0.19)   # logits spread over ~3 units
            net.conv.bias.copy_(torch.randn(C, generator=g) * 0.5)
        net.eval()
        ev = MscEvalV0(net, [(image, labels)], C, ignore_label=IGNORE, scales=scales, flip=flip, cropsize=crop,
                       device=torch.device("cpu"))
        prob32 = summed_map(ev, image)
        res = ev.evaluate()
        pred = torch.argmax(prob32, dim=1).numpy()
        assert np.array_equal(MscEvalV0.compute_hist(pred[0], labels[0].numpy(), C, IGNORE), res["confusion_matrix"])
        torch.set_default_dtype(torch.float64)
        try:
            ev64 = MscEvalV0(copy.deepcopy(net).double(), [], C, ignore_label=IGNORE, scales=scales, flip=flip, cropsize=crop,
                             device=torch.device("cpu"))
            prob64 = summed_map(ev64, image.double())
        finally:
            torch.set_default_dtype(torch.float32)
        assert prob64.dtype == torch.float64
        p32, p64 = prob32.numpy(), prob64.numpy()
        maxabs = float(np.abs(p32.astype(np.float64) - p64).max())
        top2 = np.sort(p64, axis=1)[:, -2:]
        share = float(((top2[:, 1] - top2[:, 0]) < TIE_FACTOR * maxabs).mean())
        disagree = float((np.argmax(p64, axis=1) != pred).mean())
        print(f"case {k}: ref32_vs_f64_maxabs {maxabs:.3e}  undecided share {share:.3e}  fp32/fp64 argmax disagree {disagree:.3e}  "
              f"mIoU {res['mIoU']:.6f}  acc {res['accuracy']:.6f}")
        assert share <= MAX_UNDECIDED_SHARE, f"case {k}: {share:.3e} of the pixels are undecided"
        q64 = np.rint((p64 - p32.astype(np.float64)) / (maxabs / 32767.0)).astype(np.int16)
        per = max(1, MAX_VALUES_PER_FILE // (H * W))
        for j, c0 in enumerate(range(0, C, per)):
            path = os.path.join(HERE, f"g5_eval_maps_c{k}_{j}.npz")
            np.savez_compressed(path, prob32=p32[:, c0:c0 + per], q64=q64[:, c0:c0 + per])
            assert os.path.getsize(path) < 2 ** 20, path
        small.update({f"c{k}_{n}": v for n, v in dict(
            n_classes=C, cropsize=crop, scales=np.array(scales), flip=flip, ignore_label=IGNORE, seed=500 + k, image_u8=u8,
            labels=labels.numpy().astype(np.uint8), weight=net.conv.weight.detach().numpy(), bias=net.conv.bias.detach().numpy(),
            pred=pred.astype(np.uint8), confusion_matrix=res["confusion_matrix"], mIoU=res["mIoU"], accuracy=res["accuracy"],
            ref32_vs_f64_maxabs=maxabs, undecided_share=share).items()})
    path = os.path.join(HERE, "g5_eval.npz")
    np.savez_compressed(path, **small)
    assert os.path.getsize(path) < 2 ** 20
    print(f"wrote g5_eval.npz: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
