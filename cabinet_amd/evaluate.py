"""Multi-scale, sliding-window, flip-averaged evaluation: the number the reference publishes (mIoU).

``MscEvalV0`` keeps the constructor, the methods and the result dictionary of the reference's evaluator
(src/scripts/evaluate.py:32-247) and adds one keyword, ``fused``:

* plain (``fused=False``, and always for a model on the CPU): the reference's sequence of torch operations.  It needs nothing
  from the model but ``model(x)[0]`` and is the yardstick of the fused path.
* fused (``fused=True``; ``None`` = whenever the model is on a GPU, the library is loaded and the shapes are supported): the
  model runs through ``forward_lowres`` when it has one (else ``model(x)[0]``, "low resolution at factor 1") and everything
  behind it runs in three HIP kernels (csrc/eval_tail.hip): labels go to the device once per batch, predictions never come
  back, and the C x C confusion matrix is copied to the host once per ``evaluate()``.

Both paths compute the same thing; only rounding differs (tests/test_evaluate.py, tests/test_gpu_evaluate.py).
"""

from __future__ import annotations

import math
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import functional as _fn
from .models.constants import EVAL_STRIDE_RATE

__all__ = ["MscEvalV0"]


def _window_starts(full: int, crop: int, stride: int) -> List[int]:
    """Start of every window along one axis: a step of ``stride``, the last window pulled back to end at the image edge."""
    n = math.ceil((full - crop) / stride) + 1
    return [min(full, stride * i + crop) - crop for i in range(n)]


class _Unsupported(Exception):
    pass


class MscEvalV0(object):
    """Multi-scale crop evaluation of a segmentation model (flip, scales, overlapping windows)."""

    def __init__(self, model: torch.nn.Module, dataloader: Iterable, n_classes: int, ignore_label: int = 255,
                 scales: Sequence[float] = (1.0,), flip: bool = False, cropsize: int = 1024,
                 device: Optional[torch.device] = None, fused: Optional[bool] = None):
        self.model = model
        self.dl = dataloader
        self.n_classes = n_classes
        self.ignore_label = ignore_label
        self.scales = scales
        self.flip = flip
        self.cropsize = cropsize
        self.device = device or torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.fused = fused

    # ------------------------------------------------------------------ shared geometry

    def _target_size(self, H: int, W: int) -> Optional[Tuple[int, int]]:
        """Size the image is zero-padded to before windows are cut, None when it already holds a whole crop.  An image
        shorter than the crop on both axes becomes crop x crop; otherwise only the SHORTER axis is raised to the crop and
        the other keeps its length (so H < crop <= W gives crop x W)."""
        crop = self.cropsize
        if H >= crop and W >= crop:
            return None
        if max(H, W) < crop:
            return crop, crop
        return (crop if H < W else H), (crop if W < H else W)

    def pad_tensor(self, tensor: torch.Tensor, size: tuple) -> Tuple[torch.Tensor, list]:
        """Centre ``tensor`` in a zero tensor of ``size``; returns it with [hst, hed, wst, wed] of the original inside it."""
        N, C, H, W = tensor.shape
        hst, wst = max(size[0] - H, 0) // 2, max(size[1] - W, 0) // 2
        hed, wed = hst + H, wst + W
        out = torch.zeros(N, C, size[0], size[1], device=tensor.device)
        out[:, :, hst:hed, wst:wed] = tensor
        return out, [hst, hed, wst, wed]

    # ------------------------------------------------------------------ plain path

    def eval_chip(self, crop: torch.Tensor) -> torch.Tensor:
        """Class probabilities of one chip, averaged with those of its mirror image when ``flip`` is on."""
        with torch.no_grad():
            prob = F.softmax(self.model(crop)[0], dim=1)
            if self.flip:
                mirrored = self.model(torch.flip(crop, dims=(3,)))[0]
                prob = (prob + F.softmax(torch.flip(mirrored, dims=(3,)), dim=1)) * 0.5
        return prob

    def crop_eval(self, image: torch.Tensor) -> torch.Tensor:
        """Probabilities (N, n_classes, H, W) of ``image`` (N, 3, H, W) from overlapping crop-sized windows, every pixel
        weighted equally (the sum over windows divided by the number of windows that cover the pixel)."""
        crop = self.cropsize
        N, _, H, W = image.shape
        target = self._target_size(H, W)
        indices = None
        if target is not None:
            image, indices = self.pad_tensor(image, target)
        FH, FW = image.shape[2:]
        prob = torch.zeros((N, self.n_classes, FH, FW), device=image.device)
        count = torch.zeros((1, 1, FH, FW), device=image.device)
        if FH < crop or FW < crop:
            prob += self.eval_chip(image)
            count += 1
        else:
            stride = int(crop * EVAL_STRIDE_RATE)
            for y in _window_starts(FH, crop, stride):
                for x in _window_starts(FW, crop, stride):
                    prob[:, :, y:y + crop, x:x + crop] += self.eval_chip(image[:, :, y:y + crop, x:x + crop])
                    count[:, :, y:y + crop, x:x + crop] += 1
        prob = prob / count.clamp(min=1)
        if indices is not None:
            hst, hed, wst, wed = indices
            prob = prob[:, :, hst:hed, wst:wed]
        return prob

    def scale_crop_eval(self, image: torch.Tensor, scale: float) -> torch.Tensor:
        """``crop_eval`` of the image resized by ``scale``, resized back to the image's own size."""
        H, W = image.shape[2:]
        scaled = F.interpolate(image, [int(H * scale), int(W * scale)], mode="bilinear", align_corners=False)
        return F.interpolate(self.crop_eval(scaled), (H, W), mode="bilinear", align_corners=False)

    @staticmethod
    def compute_hist(pred, label, n_classes: int, ignore_label: int) -> np.ndarray:
        """Confusion matrix (n_classes, n_classes) indexed [pred, label].  Pixels labelled ``ignore_label`` are dropped;
        every other label, and every prediction, is clipped into [0, n_classes - 1]."""
        pred = pred.cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)
        label = label.cpu().numpy() if isinstance(label, torch.Tensor) else np.asarray(label)
        keep = label != ignore_label
        p = np.clip(pred[keep].astype(np.int64), 0, n_classes - 1)
        t = np.clip(label[keep].astype(np.int64), 0, n_classes - 1)
        return np.bincount(p * n_classes + t, minlength=n_classes ** 2).reshape(n_classes, n_classes)

    # ------------------------------------------------------------------ fused path

    def _low(self, x: torch.Tensor) -> torch.Tensor:
        lowres = getattr(self.model, "forward_lowres", None)
        return lowres(x)[0] if lowres is not None else self.model(x)[0]

    def _fused_supported(self, images: torch.Tensor) -> bool:
        return bool(images.is_cuda and self.n_classes <= 32 and _fn._lib.available())

    def _fused_scale(self, image: torch.Tensor, scale: float, total: torch.Tensor, use_shortcut: bool = True) -> None:
        """``total += scale_crop_eval(image, scale)`` with everything behind the model in the HIP kernels.  When the scaled and
        padded image has the size of ``total`` the chips accumulate straight into it (``use_shortcut``), otherwise into a
        buffer of this scale that one merge kernel resizes into ``total``."""
        crop = self.cropsize
        N, _, H, W = image.shape
        scaled = F.interpolate(image, [int(H * scale), int(W * scale)], mode="bilinear", align_corners=False)
        sh, sw = scaled.shape[2:]
        target = self._target_size(sh, sw)
        indices = [0, sh, 0, sw]
        if target is not None:
            scaled, indices = self.pad_tensor(scaled, target)
        FH, FW = scaled.shape[2:]
        direct = use_shortcut and target is None and (FH, FW) == (H, W)
        dst = total if direct else torch.zeros((N, self.n_classes, FH, FW), device=image.device)
        if FH < crop or FW < crop:
            ys, xs, ch, cw = [0], [0], FH, FW
        else:
            stride = int(crop * EVAL_STRIDE_RATE)
            ys, xs, ch, cw = _window_starts(FH, crop, stride), _window_starts(FW, crop, stride), crop, crop
        # the reference's count map is the outer product of these two vectors
        cy, cx = torch.zeros(FH), torch.zeros(FW)
        for y in ys:
            cy[y:y + ch] += 1
        for x in xs:
            cx[x:x + cw] += 1
        rcp_y, rcp_x = (1.0 / cy.clamp(min=1)).to(image.device), (1.0 / cx.clamp(min=1)).to(image.device)
        for y in ys:
            for x in xs:
                chip = scaled[:, :, y:y + ch, x:x + cw].contiguous()
                a = self._low(chip)
                b = self._low(torch.flip(chip, dims=(3,))) if self.flip else None
                if self.fused is None and not _fn.eval_chip_accum_supported(a, (ch, cw), self.flip):
                    raise _Unsupported()  # `fused=True` goes on and raises with the library's message
                _fn.eval_chip_accum(dst, a, b, (ch, cw), (y, x), rcp_y, rcp_x)
        if not direct:
            _fn.eval_scale_merge(total, dst, indices)

    def _check_fused(self, images: torch.Tensor) -> None:
        """``fused=True`` on a case the kernels do not take: raise with the library's message."""
        if not images.is_cuda:
            raise RuntimeError("MscEvalV0(fused=True): the model is not on a GPU; the fused evaluation tail is HIP only")
        _fn._lib.load()  # raises when the library is missing or of another ABI version; shapes are refused by the library itself

    # ------------------------------------------------------------------ driver

    def _summed_probs(self, images: torch.Tensor, use_shortcut: bool = True) -> Tuple[torch.Tensor, bool]:
        """Sum over ``self.scales`` of ``scale_crop_eval`` and whether the fused path computed it."""
        fused = self.fused
        if fused:
            self._check_fused(images)
        elif fused is None:
            fused = self._fused_supported(images)
        N, _, H, W = images.shape
        probs = torch.zeros((N, self.n_classes, H, W), device=images.device)
        if fused:
            try:
                for scale in self.scales:
                    self._fused_scale(images, scale, probs, use_shortcut)
                return probs, True
            except _Unsupported:  # chip logits the kernels do not take, met under `fused=None`: the plain path
                probs.zero_()
        for scale in self.scales:
            probs += self.scale_crop_eval(images, scale)
        return probs, False

    def summed_probabilities(self, images: torch.Tensor) -> torch.Tensor:
        """The (N, n_classes, H, W) map whose argmax is the prediction: class probabilities summed over the scales."""
        self.model.eval()
        with torch.no_grad():
            return self._summed_probs(images.to(next(self.model.parameters()).device))[0]

    def evaluate(self) -> Dict[str, Any]:
        """Evaluate every batch of the dataloader; returns mIoU, accuracy, per-class IoU and the confusion matrix on rank 0
        (of an initialised process group, else of this process) and {} on the other ranks."""
        self.model.eval()
        device = next(self.model.parameters()).device
        C = self.n_classes
        hist = np.zeros((C, C), dtype=np.float64)
        hist_dev = None
        is_dist = dist.is_available() and dist.is_initialized()
        rank = dist.get_rank() if is_dist else 0
        with torch.no_grad():
            for images, labels in self.dl:
                images = images.to(device, non_blocking=True)
                if labels.dim() == 4:
                    labels = labels.squeeze(1)
                probs, fused = self._summed_probs(images)
                if fused:
                    if hist_dev is None:
                        hist_dev = torch.zeros((C, C), dtype=torch.int64, device=device)
                    _fn.eval_argmax_hist(probs, labels.to(device=device, dtype=torch.int64), hist_dev, self.ignore_label)
                    continue
                preds = torch.argmax(probs, dim=1).cpu().numpy()
                labels_np = labels.cpu().numpy()
                for i in range(labels_np.shape[0]):
                    hist += self.compute_hist(preds[i], labels_np[i], C, self.ignore_label)
        if hist_dev is not None:
            hist += hist_dev.cpu().numpy().astype(np.float64)  # the one device-to-host copy of the fused path
        if is_dist:
            t = torch.from_numpy(hist).to(device)
            dist.reduce(t, dst=0, op=dist.ReduceOp.SUM)
            if rank == 0:
                hist = t.cpu().numpy()
        if rank != 0:
            return {}
        diag = np.diag(hist)
        ious = diag / (hist.sum(axis=0) + hist.sum(axis=1) - diag + 1e-8)
        return {
            "mIoU": np.nanmean(ious),
            "accuracy": diag.sum() / hist.sum(),
            "iou_per_class": {f"class_{i}": ious[i] for i in range(len(ious))},
            "confusion_matrix": hist,
        }

    def __call__(self):
        return self.evaluate()
