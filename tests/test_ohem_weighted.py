"""Class-weighted OHEM-CE (reference src/utils/loss.py:38-80 with ``weight=``, the reference's default training configuration)
on the host: the composite path of ``cabinet_amd.loss.OhemCELoss`` against vectors the reference produced in float64
(tests/golden/make_golden_ohem_weighted.py), ``make_criteria(weight=...)``, and the C header's new entry points.
The device kernels are covered by tests/test_gpu_ohem_weighted.py."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g6_ohem_weighted.npz")
BRANCHES = ("sel", "topk")


def load_case(d, ci):
    low = torch.from_numpy(d[f"c{ci}.low"])
    labels = torch.from_numpy(d[f"c{ci}.labels"].astype(np.int64))
    weight = torch.from_numpy(d[f"c{ci}.weight"])
    size = tuple(int(v) for v in d[f"c{ci}.size"])
    return low, labels, weight, size, int(d[f"c{ci}.n_min"])


def fixture_cases():
    d = np.load(FIXTURE)
    return d, range(int(d["n_cases"]))


def test_fixture_meets_the_conditions_the_comparisons_rely_on():
    """Not a measurement: the stored inputs are such that an fp32 implementation selects the float64 reference's set (no valid
    pixel within 1e-5 of the threshold), the ``sel`` cases take the 'n_min above thresh' branch and the ``topk`` cases do not,
    a class of weight 0 occurs, and roughly 10-20 % of the pixels are ignored."""
    d, cases = fixture_cases()
    shapes = []
    for ci in cases:
        low, labels, weight, size, n_min = load_case(d, ci)
        shapes.append(tuple(low.shape) + size)
        ignored = float((labels == 255).double().mean())
        assert 0.10 <= ignored <= 0.20
        zero = [c for c in range(low.shape[1]) if float(weight[c]) == 0.0]
        assert len(zero) == 1 and int((labels == zero[0]).sum()) > 0
        assert float(weight.min()) >= 0.0 and weight.dtype == torch.float32
        up = F.interpolate(low.double(), size=size, mode="bilinear", align_corners=False)
        px = F.cross_entropy(up, labels, weight=weight.double(), ignore_index=255, reduction="none")
        valid = labels != 255
        for tag in BRANCHES:
            thresh = float(d[f"c{ci}.{tag}.thresh"])
            assert float((px[valid] - thresh).abs().min()) >= 1e-5
            n_above = int(((px > thresh) & valid).sum())
            assert n_above == int(d[f"c{ci}.{tag}.n_above"]) and int(valid.sum()) == int(d[f"c{ci}.{tag}.n_valid"])
            assert (n_above >= n_min) == (tag == "sel")
    assert shapes == [(2, 19, 12, 20, 96, 160), (2, 8, 16, 16, 128, 128)]


@pytest.mark.parametrize("tag", BRANCHES)
@pytest.mark.parametrize("dtype,ltol,gtol", [(torch.float64, 1e-10, 1e-9), (torch.float32, 1e-5, 1e-3)])
@pytest.mark.parametrize("entry", ["forward", "forward_upsampled", "pair"])
def test_host_composite_path_matches_the_reference(entry, dtype, ltol, gtol, tag):
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    d, cases = fixture_cases()
    for ci in cases:
        low, labels, weight, size, n_min = load_case(d, ci)
        thresh = float(d[f"c{ci}.{tag}.thresh"])
        ref_loss, ref_dlow = float(d[f"c{ci}.{tag}.loss"]), torch.from_numpy(d[f"c{ci}.{tag}.dlow"])
        crit = OhemCELoss(thresh, n_min, 255, weight=weight.to(dtype))
        x = low.to(dtype).clone().requires_grad_(True)
        if entry == "forward":
            loss = crit(F.interpolate(x, size=size, mode="bilinear", align_corners=False), labels)
            heads = [x]
        elif entry == "forward_upsampled":
            loss = crit.forward_upsampled(x, labels, size)
            heads = [x]
        else:
            x2 = low.to(dtype).clone().requires_grad_(True)
            crit2 = OhemCELoss(thresh, n_min, 255, weight=weight.to(dtype))
            loss = ohem_upsampled_pair(crit, x, crit2, x2, labels, size)
            heads = [x, x2]
        loss.backward()
        want = len(heads) * ref_loss
        assert abs(float(loss.detach()) - want) <= ltol * max(1.0, abs(want)), (ci, float(loss.detach()), want)
        for h in heads:
            assert_close(h.grad, ref_dlow, gtol, f"dlow case {ci} {tag} {entry}", atol=1e-12)


def test_a_pair_of_differently_weighted_heads_is_the_sum_of_the_heads():
    """One weighted and one unweighted criterion (and two different weight tables) through ``ohem_upsampled_pair``."""
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    d, cases = fixture_cases()
    low, labels, weight, size, n_min = load_case(d, 1)
    for wa, wb in ((weight, None), (weight, weight.flip(0))):
        ca, cb = OhemCELoss(0.7, n_min, 255, weight=wa), OhemCELoss(0.7, n_min, 255, weight=wb)
        xa, xb = low.clone().requires_grad_(True), (low * 0.5).requires_grad_(True)
        ohem_upsampled_pair(ca, xa, cb, xb, labels, size).backward()
        ya, yb = low.clone().requires_grad_(True), (low * 0.5).requires_grad_(True)
        (ca.forward_upsampled(ya, labels, size) + cb.forward_upsampled(yb, labels, size)).backward()
        assert torch.equal(xa.grad, ya.grad) and torch.equal(xb.grad, yb.grad)
        assert not torch.equal(xa.grad, xb.grad)


def test_make_criteria_hands_the_weights_to_both_criteria():
    from cabinet_amd.train import make_criteria

    w = [1.5, 0.0, 2.25, 3.0, 1.0, 1.0, 4.5, 2.0]
    for given in (w, torch.tensor(w, dtype=torch.float64), np.asarray(w)):
        crit_p, crit_16 = make_criteria(2, 64, 64, "cpu", weight=given)
        for crit in (crit_p, crit_16):
            assert "weight" in dict(crit.named_buffers())
            assert crit.weight.dtype == torch.float32 and crit.weight.tolist() == w
            assert crit.n_min == 2 * 64 * 64 // 16
        assert crit_p.weight.data_ptr() != crit_16.weight.data_ptr()   # separate buffers, as after the reference's .to()
        crit_p.to(torch.float64)
        assert crit_p.weight.dtype == torch.float64 and crit_16.weight.dtype == torch.float32   # buffers follow .to()
        assert "weight" in crit_p.state_dict()
    plain_p, plain_16 = make_criteria(2, 64, 64, "cpu")
    assert plain_p.weight is None and plain_16.weight is None


def _declared(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(cabinet_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_header_declares_the_weighted_entry_points_under_abi_8():
    from cabinet_amd import _lib

    text = open(os.path.join(ROOT, "include", "cabinet_hip.h")).read()
    assert "#define CABINET_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8
    decl = _declared(text)
    pairs = [("cabinet_ohem_up_fwd", "cabinet_ohem_up_w_fwd", 1), ("cabinet_ohem_up_bwd", "cabinet_ohem_up_w_bwd", 1),
             ("cabinet_ohem_up_pair_fwd", "cabinet_ohem_up_pair_w_fwd", 2), ("cabinet_ohem_up_pair_bwd", "cabinet_ohem_up_pair_w_bwd", 2)]
    for plain, weighted, ntab in pairs:
        assert plain in decl and weighted in decl, weighted
        a, b = decl[plain].split(","), decl[weighted].split(",")
        # the existing argument list plus one `const float*` table per head in front of the stream
        assert len(b) == len(a) + ntab and b[:len(a) - 1] == a[:-1] and b[-1] == a[-1]
        assert all(t.strip().startswith("const float* class_weight") for t in b[len(a) - 1:-1])
        assert weighted in _lib.SIGNATURES and len(_lib.SIGNATURES[weighted][1]) == len(b)
