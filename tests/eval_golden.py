"""Loader of the evaluator fixture tests/golden/g5_eval*.npz (written by tests/golden/make_golden_eval.py) and the stub model
whose weights travel in it.  Shared by tests/test_evaluate.py and tests/test_gpu_evaluate.py.

Storage (no file above 1 MiB): g5_eval.npz holds, per case, the image as uint8 (image = (u8 - 128) / 64, exact in fp32), labels
and the reference's predictions as uint8, the stub's weights, the reference's confusion matrix, mIoU, accuracy and the scalars
derived from its two probability maps; g5_eval_maps_c<case>_<part>.npz hold class ranges of the reference's fp32 summed
probability map and of its float64 map, the latter as int16 steps of ref32_vs_f64_maxabs / 32767 away from the fp32 map
(reconstruction error below 4e-10, five orders under the tie margin).
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = (1, 2, 3, 4)
TIE_FACTOR = 5.0            # undecided: float64 top-two margin below TIE_FACTOR x ref32_vs_f64_maxabs (from the fixture)
MAX_UNDECIDED_SHARE = 2e-3  # of the pixels of any case


class StubNet(torch.nn.Module):
    """Conv2d(3, C, 8, stride=8): ``forward_lowres`` returns its output, ``forward`` the x8 align_corners=False upsample, so one
    stub exercises the plain path (``model(x)[0]``) and the fused path (``forward_lowres``)."""

    def __init__(self, n_classes):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, n_classes, 8, stride=8)

    def forward_lowres(self, x):
        y = self.conv(x)
        return y, y

    def forward(self, x):
        y = F.interpolate(self.conv(x), size=x.shape[2:], mode="bilinear", align_corners=False)
        return y, y


def image_from_u8(u8):
    return (torch.from_numpy(np.asarray(u8)).float() - 128.0) / 64.0


def load_case(k):
    z = np.load(os.path.join(GOLDEN, "g5_eval.npz"))
    g = {n[len(f"c{k}_"):]: z[n] for n in z.files if n.startswith(f"c{k}_")}
    parts = sorted(glob.glob(os.path.join(GOLDEN, f"g5_eval_maps_c{k}_*.npz")))
    maps = [np.load(p) for p in parts]
    prob32 = np.concatenate([m["prob32"] for m in maps], axis=1)
    step = float(g["ref32_vs_f64_maxabs"]) / 32767.0
    prob64 = prob32.astype(np.float64) + np.concatenate([m["q64"] for m in maps], axis=1).astype(np.float64) * step
    C = int(g["n_classes"])
    assert prob32.shape[1] == C
    net = StubNet(C)
    with torch.no_grad():
        net.conv.weight.copy_(torch.from_numpy(g["weight"]))
        net.conv.bias.copy_(torch.from_numpy(g["bias"]))
    top2 = np.sort(prob64, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    tie = TIE_FACTOR * float(g["ref32_vs_f64_maxabs"])
    return {
        "n_classes": C, "cropsize": int(g["cropsize"]), "scales": tuple(float(s) for s in g["scales"]), "flip": bool(g["flip"]),
        "ignore_label": int(g["ignore_label"]), "image": image_from_u8(g["image_u8"]),
        "labels": torch.from_numpy(g["labels"].astype(np.int64)), "model": net.eval(), "prob32": prob32, "prob64": prob64,
        "pred": g["pred"].astype(np.int64), "confusion_matrix": g["confusion_matrix"], "mIoU": float(g["mIoU"]),
        "accuracy": float(g["accuracy"]), "ref32_vs_f64_maxabs": float(g["ref32_vs_f64_maxabs"]),
        "undecided_share": float(g["undecided_share"]), "tie": tie, "undecided": margin < tie,
    }


def hist_of(pred, labels, undecided, n_classes, ignore_label):
    """Confusion matrix [pred, label] over the decided pixels only (numpy; ignore and clip rules of the evaluator)."""
    keep = (labels != ignore_label) & ~undecided
    p = np.clip(pred[keep].astype(np.int64), 0, n_classes - 1)
    t = np.clip(labels[keep].astype(np.int64), 0, n_classes - 1)
    return np.bincount(p * n_classes + t, minlength=n_classes ** 2).reshape(n_classes, n_classes)


def check_against_case(g, probs, pred, result, tag, record=None):
    """The fixture rules for one case.  probs: summed probability map (N,C,H,W) of the code under test, pred: its predictions,
    result: its evaluate() dictionary.  Prints every figure before asserting; returns the max-abs distance from the float64 map."""
    from parity_rules import TOL

    probs = probs.detach().double().cpu().numpy()
    pred = np.asarray(pred).astype(np.int64)
    labels = g["labels"].numpy()
    C, ign, und = g["n_classes"], g["ignore_label"], g["undecided"]
    rel = float(np.linalg.norm(probs - g["prob32"]) / np.linalg.norm(g["prob32"].astype(np.float64)))
    maxabs64 = float(np.abs(probs - g["prob64"]).max())
    share = float(und.mean())
    wrong = int(((pred != g["pred"]) & ~und).sum())
    print(f"[{tag}] rel vs ref fp32 {rel:.3e} (tol {TOL:g})  max|.-f64| {maxabs64:.3e} = {maxabs64 / g['ref32_vs_f64_maxabs']:.2f} x "
          f"ref32_vs_f64 {g['ref32_vs_f64_maxabs']:.3e}  tie {g['tie']:.3e}  undecided {int(und.sum())} px ({share:.3e})  "
          f"decided pixels predicted differently: {wrong}")
    if record is not None:
        record[tag] = {"rel_vs_ref32": rel, "maxabs_vs_f64": maxabs64, "ref32_vs_f64_maxabs": g["ref32_vs_f64_maxabs"],
                       "undecided_px": int(und.sum()), "decided_px_differing": wrong}
    assert rel <= TOL, f"{tag}: probability map {rel:.3e} from the reference's"
    assert share <= MAX_UNDECIDED_SHARE and abs(share - g["undecided_share"]) < 1e-12
    assert wrong == 0, f"{tag}: {wrong} decided pixels differ from the reference's predictions"
    mine, ref = hist_of(pred, labels, und, C, ign), hist_of(g["pred"], labels, und, C, ign)
    assert np.array_equal(mine, ref), f"{tag}: confusion matrix over the decided pixels differs"
    # the matrix evaluate() returned is the histogram of these very predictions, and (fixture self-check) so is the reference's
    none = np.zeros_like(und)
    assert np.array_equal(hist_of(g["pred"], labels, none, C, ign), g["confusion_matrix"])
    cm = result["confusion_matrix"]
    assert cm.dtype == np.float64 and cm.shape == (C, C)
    assert np.array_equal(cm, hist_of(pred, labels, none, C, ign).astype(np.float64)), f"{tag}: evaluate() matrix is not the histogram of its predictions"
    # mIoU / accuracy: within what k undecided (valid) pixels can move them.  accuracy = trace / total moves by at most k / total;
    # an IoU I/U with I and U each moved by at most k changes by at most 2k / (U - k)
    k = int((und & (labels != ign)).sum())
    refm = g["confusion_matrix"].astype(np.float64)
    union = refm.sum(0) + refm.sum(1) - np.diag(refm)
    bound_miou = float(np.mean(2.0 * k / np.maximum(union - k, 1.0))) + 1e-9
    bound_acc = k / refm.sum() + 1e-12
    print(f"[{tag}] mIoU {result['mIoU']:.8f} vs {g['mIoU']:.8f} (allowed {bound_miou:.2e})  accuracy {result['accuracy']:.8f} vs "
          f"{g['accuracy']:.8f} (allowed {bound_acc:.2e})")
    assert abs(result["mIoU"] - g["mIoU"]) <= bound_miou
    assert abs(result["accuracy"] - g["accuracy"]) <= bound_acc
    return maxabs64


def write_record(record, name):
    """Figures of a run go to the file CABINET_EVAL_PARITY_JSON names (merged), when set; the committed copy lives in profiles/."""
    import json

    path = os.environ.get("CABINET_EVAL_PARITY_JSON")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[name] = record
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
