"""Single-image inference: label maps and overlay images out of a trained model (the reference's src/scripts/visualize.py).

``infer_image`` and ``colorize_mask`` keep the reference's contracts (visualize.py:50-61, :64-140); ``visualize_predictions``
writes the reference's four files per sample (:143-195); ``Predictor`` is the same computation for repeated use: batches, labels
that stay on the device, rendering on the device and, opt-in, one hipGraph per input shape.

Two paths, as in ``cabinet_amd.evaluate``:

* plain (``fused=False``, and always for a model on the CPU): the reference's sequence of torch operations -- ``model(x)[0]``
  at full resolution, softmax, flip, resize, sum over scales, argmax.  It runs on any model and any device and is the yardstick
  of the fused path.
* fused (``fused=True``; ``None`` = whenever the model is on a GPU, the library is loaded, there are at most 32 classes and the
  kernels take the shapes): the model runs through ``forward_lowres`` when it has one (else ``model(x)[0]``, "low resolution at
  factor 1") and everything behind it runs in HIP kernels (csrc/predict_tail.hip, csrc/eval_tail.hip).  For ``scales=[1.0]``
  without flip -- the deployment setting -- the labels are the argmax of the resized logits (softmax does not move an argmax),
  computed from the H/8 x W/8 logits in one kernel; the full-resolution class tensor never exists.  Otherwise every scale's
  probabilities are accumulated by ``eval_chip_accum`` (the whole scaled image as one chip) and ``eval_scale_merge``, and one
  kernel takes the argmax.  The reference's division by ``len(scales)`` is skipped: it does not move the argmax either.

Both paths compute the same labels; only pixels whose two best classes are within rounding of each other may differ
(tests/test_predict.py, tests/test_gpu_predict.py).
"""

from __future__ import annotations

from collections import OrderedDict
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import functional as _fn
from .models.constants import CITYSCAPES_NUM_CLASSES, VISUALIZATION_SAMPLE_LIMIT

__all__ = ["CITYSCAPES_COLORS", "IMAGENET_MEAN", "IMAGENET_STD", "Predictor", "colorize_mask", "infer_image",
           "visualize_predictions"]

# Colours of the 19 Cityscapes train ids (the dataset's public label table, cityscapesScripts helpers/labels.py)
CITYSCAPES_COLORS = np.array([
    [128, 64, 128], [244, 35, 232], [70, 70, 70], [102, 102, 156], [190, 153, 153], [153, 153, 153], [250, 170, 30],
    [220, 220, 0], [107, 142, 35], [152, 251, 152], [70, 130, 180], [220, 20, 60], [255, 0, 0], [0, 0, 142], [0, 0, 70],
    [0, 60, 100], [0, 80, 100], [0, 0, 230], [119, 11, 32],
], dtype=np.uint8)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# What ``fused=None`` selects on a GPU.  Set by measurement (profiles/predict_time.json).
FUSED_BY_DEFAULT = True


class _Unsupported(Exception):
    pass


def colorize_mask(mask, palette: np.ndarray = CITYSCAPES_COLORS):
    """(H, W) integer label map -> PIL RGB image; labels are clipped into the palette (255 takes the last colour)."""
    from PIL import Image

    mask = np.asarray(mask)
    h, w = mask.shape
    palette = np.asarray(palette, dtype=np.uint8)
    idx = np.clip(mask, 0, len(palette) - 1).astype(np.int64)
    return Image.fromarray(palette[idx.ravel()].reshape(h, w, 3))


def _resize(x: torch.Tensor, size) -> torch.Tensor:
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


def _plain_probs(model, x: torch.Tensor, n_classes: int, scales: Sequence[float], flip: bool) -> torch.Tensor:
    """The reference's sequence (visualize.py:97-136) for a batch: class probabilities averaged over the scales."""
    N, _, H, W = x.shape
    probs = torch.zeros((N, n_classes, H, W), device=x.device)
    for scale in scales:
        scaled = x if scale == 1.0 else _resize(x, [int(H * scale), int(W * scale)])
        prob = F.softmax(model(scaled)[0], dim=1)
        if flip:
            mirrored = model(torch.flip(scaled, dims=(3,)))[0]
            prob = (prob + F.softmax(torch.flip(mirrored, dims=(3,)), dim=1)) / 2
        if scale != 1.0:
            prob = _resize(prob, (H, W))
        probs += prob
    probs /= len(scales)
    return probs


def _low(model, x: torch.Tensor) -> torch.Tensor:
    lowres = getattr(model, "forward_lowres", None)
    return lowres(x)[0] if lowres is not None else model(x)[0]


def _fused_labels(model, x: torch.Tensor, n_classes: int, scales: Sequence[float], flip: bool, strict: bool) -> torch.Tensor:
    """(N, H, W) uint8 labels of ``x`` with everything behind the model in HIP kernels.  ``strict``: shapes the kernels refuse
    raise with the library's message; otherwise ``_Unsupported``."""
    N, _, H, W = x.shape
    if len(scales) == 1 and float(scales[0]) == 1.0 and not flip:
        low = _low(model, x)
        if low.shape[1] != n_classes:
            raise ValueError(f"the model returns {low.shape[1]} classes, not {n_classes}")
        if not strict and not _fn.predict_up_argmax_supported(low, (H, W)):
            raise _Unsupported()
        return _fn.predict_up_argmax(low, (H, W))
    total = torch.zeros((N, n_classes, H, W), device=x.device)
    for scale in scales:
        scaled = x if scale == 1.0 else _resize(x, [int(H * scale), int(W * scale)])
        size = tuple(scaled.shape[2:])
        a = _low(model, scaled)
        b = _low(model, torch.flip(scaled, dims=(3,))) if flip else None
        if a.shape[1] != n_classes:
            raise ValueError(f"the model returns {a.shape[1]} classes, not {n_classes}")
        if not strict and not (_fn.eval_chip_accum_supported(a, size, flip) and _fn.eval_scale_merge_supported(total)):
            raise _Unsupported()
        if size == (H, W):
            _fn.eval_chip_accum(total, a, b, size, (0, 0))
        else:
            dst = torch.zeros((N, n_classes, *size), device=x.device)
            _fn.eval_chip_accum(dst, a, b, size, (0, 0))
            _fn.eval_scale_merge(total, dst)
    return _fn.predict_argmax(total)


def _wants_fused(fused: Optional[bool], x: torch.Tensor, n_classes: int, who: str) -> bool:
    if fused:
        if not x.is_cuda:
            raise RuntimeError(f"{who}(fused=True): the model is not on a GPU; the fused inference tail is HIP only")
        _fn._lib.load()  # raises when the library is missing or of another ABI version; shapes are refused by the library itself
        return True
    if fused is None:
        return bool(FUSED_BY_DEFAULT and x.is_cuda and n_classes <= 32 and _fn._lib.available())
    return False


def _labels(model, x: torch.Tensor, n_classes: int, scales: Sequence[float], flip: bool, fused: Optional[bool], who: str) -> torch.Tensor:
    """(N, H, W) labels on x's device: uint8 from the fused path, int64 from the plain one."""
    if _wants_fused(fused, x, n_classes, who):
        try:
            return _fused_labels(model, x, n_classes, scales, flip, strict=bool(fused))
        except _Unsupported:  # shapes the kernels do not take, met under `fused=None`: the plain path
            pass
    return torch.argmax(_plain_probs(model, x, n_classes, scales, flip), dim=1)


@torch.no_grad()
def infer_image(model: torch.nn.Module, img_tensor: torch.Tensor, num_classes: int = CITYSCAPES_NUM_CLASSES,
                scales: Sequence[float] = [1.0], flip: bool = False, device="cuda", fused: Optional[bool] = None) -> np.ndarray:
    """Multi-scale + flip inference on one image tensor (C, H, W) or (1, C, H, W); returns the (H, W) int64 label map as a
    numpy array (reference visualize.py:64-140).  ``fused``: see the module docstring."""
    model.eval()
    if img_tensor.dim() == 3:
        img_tensor = img_tensor.unsqueeze(0)
    img_tensor = img_tensor.to(device)
    B = img_tensor.shape[0]
    if B != 1:
        raise ValueError(f"infer_image only supports batch size 1, got {B}")
    pred = _labels(model, img_tensor, num_classes, scales, flip, fused, "infer_image")
    return pred.cpu().numpy()[0].astype(np.int64, copy=False)


def _render_plain(labels: torch.Tensor, images: Optional[torch.Tensor], palette: torch.Tensor, mean, std, alpha: float) -> Dict[str, torch.Tensor]:
    """The render contract in torch operations (any device): one rounding per product and sum, truncation toward zero."""
    idx = labels.long().clamp(0, palette.shape[0] - 1)
    out = {"pred": palette[idx]}
    if images is not None:
        m = torch.tensor(mean, dtype=torch.float32, device=images.device).view(1, 1, 1, 3)
        s = torch.tensor(std, dtype=torch.float32, device=images.device).view(1, 1, 1, 3)
        x = images.float().permute(0, 2, 3, 1)
        inp = ((x * s + m).clamp(0.0, 1.0) * 255).to(torch.uint8)
        a = torch.tensor(alpha, dtype=torch.float32, device=images.device)
        diff = (out["pred"].to(torch.int16) - inp.to(torch.int16)).float()
        out["input"] = inp
        out["overlay"] = (inp.float() + a * diff).to(torch.uint8)
    return out


class Predictor(object):
    """Labels and rendered images for batches of one model, on the model's device.

    ``predict(images)`` -> uint8 (N, H, W) labels; ``render(images, labels=None)`` -> dict of ``input``, ``pred`` and ``overlay``,
    each uint8 (N, H, W, 3) (reference visualize.py:50-61, :165-177, byte for byte).  ``scales``, ``flip`` and ``fused`` as for
    ``infer_image``.

    ``graph=True`` (GPU only, opt-in: it pins memory per input shape): the first call with a shape runs once eagerly, so that
    lazy initialisation (MIOpen's solver choice) happens outside capture, and then records one hipGraph holding the resizes and
    flips, every forward, the zeroing of the probability sum, the tail kernels and the render.  Later calls copy the images into
    the graph's static input and replay.  The tensors returned are the graph's static outputs: READ THEM BEFORE THE NEXT CALL
    with the same shape (clone to keep).  At most ``max_graphs`` shapes are kept, the least recently used is dropped.  The
    graph holds the parameters' addresses, so weights updated in place (``load_state_dict``, ``copy_``) are seen by replays;
    parameters REPLACED by new tensors are not -- build a new Predictor.  The model must be in ``eval()`` mode: BatchNorm in
    training mode would update its statistics on every replay.
    """

    def __init__(self, model: torch.nn.Module, n_classes: int, scales: Sequence[float] = (1.0,), flip: bool = False,
                 fused: Optional[bool] = None, graph: bool = False, palette=None, mean: Sequence[float] = IMAGENET_MEAN,
                 std: Sequence[float] = IMAGENET_STD, alpha: float = 0.6, max_graphs: int = 4):
        self.model, self.n_classes = model, int(n_classes)
        self.scales, self.flip, self.fused, self.graph = tuple(float(s) for s in scales), bool(flip), fused, bool(graph)
        self.mean, self.std, self.alpha = tuple(float(v) for v in mean), tuple(float(v) for v in std), float(alpha)
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError(f"Predictor: alpha={alpha} outside [0, 1]")
        self.max_graphs = max(1, int(max_graphs))
        self.device = next(model.parameters()).device
        if self.graph and self.device.type != "cuda":
            raise RuntimeError("Predictor(graph=True) needs a model on a GPU: a hipGraph records device work only "
                               f"(the model is on '{self.device}')")
        pal = np.asarray(CITYSCAPES_COLORS if palette is None else palette, dtype=np.uint8)
        if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
            raise ValueError("Predictor: palette must be (n_colors <= 256, 3) uint8")
        self.palette = torch.from_numpy(pal.copy()).to(self.device)
        self._graphs: "OrderedDict[tuple, dict]" = OrderedDict()

    # ------------------------------------------------------------------ eager

    def _prepare(self, images: torch.Tensor) -> torch.Tensor:
        if self.model.training:
            raise RuntimeError("Predictor: the model is in training mode; call model.eval() first")
        if images.dim() == 3:
            images = images.unsqueeze(0)
        return images.to(self.device)

    def _labels_u8(self, x: torch.Tensor) -> torch.Tensor:
        return _labels(self.model, x, self.n_classes, self.scales, self.flip, self.fused, "Predictor").to(torch.uint8)

    def _render(self, x: Optional[torch.Tensor], labels: torch.Tensor) -> Dict[str, torch.Tensor]:
        if labels.is_cuda and self.fused is not False and _fn._lib.available():
            return _fn.predict_render(labels.contiguous(), x, self.palette, self.mean, self.std, self.alpha)
        return _render_plain(labels, x, self.palette, self.mean, self.std, self.alpha)

    # ------------------------------------------------------------------ graphs

    def _replay(self, x: torch.Tensor) -> dict:
        key = (tuple(x.shape), x.dtype)
        entry = self._graphs.get(key)
        if entry is None:
            static_in = x.clone()
            self._labels_u8(static_in)  # eager warm-up of this shape, outside capture
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                labels = self._labels_u8(static_in)
                rendered = self._render(static_in, labels)
            entry = {"graph": g, "input": static_in, "labels": labels, "rendered": rendered}
            while len(self._graphs) >= self.max_graphs:
                self._graphs.popitem(last=False)
            self._graphs[key] = entry
        else:
            self._graphs.move_to_end(key)
            entry["input"].copy_(x)
        entry["graph"].replay()
        return entry

    # ------------------------------------------------------------------ public

    @torch.no_grad()
    def predict(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 (N, H, W) labels of ``images`` (N, 3, H, W) or (3, H, W), on the model's device."""
        x = self._prepare(images)
        if self.graph:
            return self._replay(x)["labels"]
        return self._labels_u8(x)

    @torch.no_grad()
    def render(self, images: torch.Tensor, labels: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """``input``, ``pred`` and ``overlay`` of ``images``, each uint8 (N, H, W, 3) on the device.  ``labels`` (N, H, W): colour
        these (ground truth, say) instead of the model's prediction; the model is not run then."""
        x = self._prepare(images)
        if labels is not None:
            labels = labels.to(self.device)
            if labels.dim() == 2:
                labels = labels.unsqueeze(0)
            return self._render(x, labels.clamp(0, 255).to(torch.uint8))
        if self.graph:
            return dict(self._replay(x)["rendered"])
        return self._render(x, self._labels_u8(x))


def visualize_predictions(model: torch.nn.Module, dataloader, output_dir, device, show_gt: bool = True,
                          use_gt_for_overlay: bool = False, num_classes: int = CITYSCAPES_NUM_CLASSES, fused: Optional[bool] = None,
                          palette=None, limit: int = VISUALIZATION_SAMPLE_LIMIT) -> int:
    """For every batch of ``dataloader`` ((image, label) or (image,)), write ``sample_XXXX/{input,pred,overlay}.png`` of its
    first image, and ``gt.png`` when there is a label and ``show_gt`` (reference visualize.py:143-195; single scale, no flip,
    alpha 0.6).  ``use_gt_for_overlay`` blends the ground truth's colours instead of the prediction's.  Returns the number of
    samples written."""
    from PIL import Image

    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    model = model.to(device).eval()
    pred = Predictor(model, num_classes, scales=(1.0,), flip=False, fused=fused, palette=palette)
    written = 0
    for i, data in enumerate(dataloader):
        img, lb = (data[0], data[1]) if len(data) == 2 else (data[0], None)
        img = img[:1]
        out = pred.render(img)
        gt = None
        if lb is not None:
            lb0 = lb[0]
            gt = lb0[0] if lb0.dim() == 3 else lb0
        if gt is not None and use_gt_for_overlay:
            out["overlay"] = pred.render(img, gt)["overlay"]
        save_dir = output_dir / f"sample_{i:04d}"
        save_dir.mkdir(parents=True, exist_ok=True)
        for name in ("input", "pred", "overlay"):
            Image.fromarray(out[name][0].cpu().numpy()).save(save_dir / f"{name}.png")
        if gt is not None and show_gt:
            colorize_mask(gt.cpu().numpy(), pred.palette.cpu().numpy()).save(save_dir / "gt.png")
        written += 1
        if i > limit:
            break
    return written
