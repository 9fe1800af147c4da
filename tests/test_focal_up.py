"""SoftmaxFocalLoss behind the final upsample, CPU tier: the reference's float64 vectors (tests/golden/g11_focal_up.npz, written
by tests/golden/make_golden_focal_up.py) against the closed form the kernels implement (tests/focal_golden.py) and against the
composite route that CPU tensors take; and the Python plumbing around the fused head (criteria, pair dispatch)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from focal_golden import focal_up_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_focal_up.npz")
IGNORE = 255
WTAGS = ("nw", "w")


@functools.lru_cache(maxsize=None)
def fixture():
    d = np.load(GOLDEN)
    assert int(d["ignore_lb"]) == IGNORE
    return d, int(d["n_cases"]), [float(g) for g in d["gammas"]]


def load_case(d, ci):
    low = torch.from_numpy(d[f"c{ci}.low"])
    lab = torch.from_numpy(d[f"c{ci}.labels"].astype(np.int64))
    w = torch.from_numpy(d[f"c{ci}.weight"])
    size = tuple(int(s) for s in d[f"c{ci}.size"])
    return low, lab, w, size


def combos():
    _, n, gammas = fixture()
    return [(ci, wtag, gi) for ci in range(n) for wtag in WTAGS for gi in range(len(gammas))]


def test_fixture_layout_and_confident_case():
    d, n, gammas = fixture()
    assert n == 4 and gammas == [0.0, 0.5, 2.0, 5.0]
    shapes = [tuple(d[f"c{ci}.low"].shape) + tuple(int(s) for s in d[f"c{ci}.size"]) for ci in range(n)]
    assert shapes[:3] == [(1, 5, 7, 9, 40, 50), (2, 19, 12, 20, 96, 160), (1, 8, 2, 64, 16, 512)]
    for ci in range(n):
        low, lab, w, size = load_case(d, ci)
        valid = lab != IGNORE
        assert 0.10 < 1.0 - float(valid.double().mean()) < 0.20          # 15 % ignored
        counts = np.bincount(lab[valid].numpy(), minlength=low.shape[1])
        assert np.array_equal(counts, d[f"c{ci}.counts"])
        zero = (w == 0).nonzero().flatten().tolist()
        assert len(zero) == 1 and counts[zero[0]] > 0                    # a class that occurs and weighs nothing
        assert d[f"c{ci}.w.g0.dlow"].dtype == np.float32
    # the confident case, re-asserted on the stored data
    ci = int(d["conf"])
    low, lab, _, size = load_case(d, ci)
    up = F.interpolate(low.double(), size=size, mode="bilinear", align_corners=False)
    p_t = torch.softmax(up, 1).gather(1, lab.clamp(max=low.shape[1] - 1).unsqueeze(1)).squeeze(1)
    valid = lab != IGNORE
    n_conf, n_hopeless = int(((p_t > 1 - 1e-6) & valid).sum()), int(((p_t < 1e-6) & valid).sum())
    assert n_conf >= 64 and n_hopeless >= 64
    assert (n_conf, n_hopeless) == (int(d[f"c{ci}.n_conf"]), int(d[f"c{ci}.n_hopeless"]))
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("ci,wtag,gi", combos())
def test_closed_form_reproduces_the_reference(ci, wtag, gi):
    """tests/focal_golden.py (the formulas the kernels implement) against the reference's own autograd in float64."""
    d, _, gammas = fixture()
    low, lab, w, size = load_case(d, ci)
    loss, dlow, _ = focal_up_ref(low, lab, size, gammas[gi], w if wtag == "w" else None, IGNORE)
    ref_loss, ref_dlow = float(d[f"c{ci}.{wtag}.g{gi}.loss"]), torch.from_numpy(d[f"c{ci}.{wtag}.g{gi}.dlow"])
    assert abs(loss - ref_loss) <= 1e-12 * abs(ref_loss)
    # dlow is stored as fp32: half an ulp per element.  The absolute floor covers the REFERENCE's own error: it forms q as
    # 1 - prob, 2^-53 absolute, which is 4e-4 of q at the confident pixels of the last case (q ~ 3e-13); everything those pixels
    # send into dlow is below 64 * 8 * q^(1 + gamma) / D < 1e-19 for gamma >= 0.5 (and exact for gamma = 0), so the error they
    # carry is below 1e-22 -- and fp32 denormals round at 2^-150.
    err = (dlow - ref_dlow.double()).abs()
    assert bool((err <= 2.0 ** -24 * ref_dlow.double().abs() + 1e-22).all()), float(err.max())


@pytest.mark.parametrize("ci,wtag,gi", combos())
def test_forward_upsampled_on_cpu_is_the_composite(ci, wtag, gi):
    """For CPU tensors the composite route is the contract: it equals the fixture (fp32 composite against float64)."""
    from cabinet_amd.loss import SoftmaxFocalLoss

    d, _, gammas = fixture()
    low, lab, w, size = load_case(d, ci)
    crit = SoftmaxFocalLoss(gammas[gi], weight=w.clone() if wtag == "w" else None, ignore_lb=IGNORE)
    x = low.clone().requires_grad_(True)
    loss = crit.forward_upsampled(x, lab, size)
    loss.backward()
    x2 = low.clone().requires_grad_(True)
    direct = crit(F.interpolate(x2, size=size, mode="bilinear", align_corners=False), lab)
    direct.backward()
    assert torch.equal(loss.detach(), direct.detach()) and torch.allclose(x.grad, x2.grad, rtol=0, atol=0, equal_nan=True)
    ref_loss = float(d[f"c{ci}.{wtag}.g{gi}.loss"])
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    if not (ci == int(d["conf"]) and 0 < gammas[gi] < 1):   # the composite's fp32 autograd is NaN at q = 0 for 0 < gamma < 1
        assert_close(x.grad, torch.from_numpy(d[f"c{ci}.{wtag}.g{gi}.dlow"]), 1e-3, "dlow", atol=1e-9)
    # size defaults to the labels' size
    assert torch.equal(crit.forward_upsampled(low, lab).detach(), direct.detach())


def test_composite_autograd_is_nan_where_the_fused_head_pins_zero():
    """The deviation the fused head documents: fp32, 0 < gamma < 1, q = 0 -> the composite's gradient is NaN."""
    from cabinet_amd.loss import SoftmaxFocalLoss

    x = torch.tensor([[40.0, 0.0]]).view(1, 2, 1, 1).requires_grad_(True)
    SoftmaxFocalLoss(0.5)(x, torch.zeros(1, 1, 1, dtype=torch.long)).backward()
    assert bool(torch.isnan(x.grad).any())
    _, dlow, _ = focal_up_ref(x.detach(), torch.zeros(1, 1, 1, dtype=torch.long), (1, 1), 0.5)
    assert bool(torch.isfinite(dlow).all())


def test_edge_semantics_of_the_restatement_and_the_composite():
    """No valid pixel: NaN loss (0 / 0) and a gradient of exactly 0, in the composite and in the restatement.  Only classes of
    weight 0: NaN loss in both; the restatement (and the fused head) pin the gradient to 0, the composite's nll_loss backward
    divides 0 by the zero total weight at every valid pixel and returns NaN."""
    from cabinet_amd.loss import SoftmaxFocalLoss

    low = torch.randn(1, 4, 3, 3, generator=torch.Generator().manual_seed(0))
    cases = ((torch.full((1, 12, 12), IGNORE), None, True),
             (torch.ones(1, 12, 12, dtype=torch.long), torch.tensor([1.0, 0, 1, 1]), False))
    for lab, w, composite_zero in cases:
        x = low.clone().requires_grad_(True)
        loss = SoftmaxFocalLoss(2.0, weight=w, ignore_lb=IGNORE).forward_upsampled(x, lab)
        loss.backward()
        assert bool(torch.isnan(loss))
        if composite_zero:
            assert float(x.grad.abs().max()) == 0.0
        else:
            assert bool(torch.isnan(x.grad).all())
        rl, rd, st = focal_up_ref(low, lab, (12, 12), 2.0, w, IGNORE)
        assert rl != rl and float(rd.abs().max()) == 0.0 and st[1] == 0.0


def test_make_criteria_focal():
    from cabinet_amd.loss import OhemCELoss, SoftmaxFocalLoss
    from cabinet_amd.train import make_criteria

    w = torch.tensor([1.0, 2.0, 0.0, 4.0])
    a, b = make_criteria(2, 64, 64, "cpu", weight=w, loss="focal", gamma=1.5)
    assert type(a) is SoftmaxFocalLoss and type(b) is SoftmaxFocalLoss
    assert a.gamma == b.gamma == 1.5 and a.ignore_lb == b.ignore_lb == 255
    assert torch.equal(a.weight, w) and torch.equal(b.weight, w)
    assert a.weight.data_ptr() != b.weight.data_ptr() and a.weight.data_ptr() != w.data_ptr()   # each its own buffer
    a, b = make_criteria(2, 64, 64, "cpu", loss="focal")
    assert a.gamma == 2.0 and a.weight is None and b.weight is None
    assert all(type(c) is OhemCELoss for c in make_criteria(2, 64, 64, "cpu"))                  # defaults change nothing
    with pytest.raises(ValueError):
        make_criteria(2, 64, 64, "cpu", loss="dice")


def test_upsampled_pair_dispatch_on_cpu():
    from cabinet_amd.loss import OhemCELoss, SoftmaxFocalLoss, ohem_upsampled_pair, upsampled_pair

    g = torch.Generator().manual_seed(3)
    la, lb_ = torch.randn(1, 5, 4, 4, generator=g), torch.randn(1, 5, 4, 4, generator=g)
    lab = torch.randint(0, 5, (1, 32, 32), generator=g)
    lab[0, :3] = IGNORE
    oa, ob = OhemCELoss(0.7, 16, IGNORE), OhemCELoss(0.7, 16, IGNORE, weight=torch.rand(5, generator=g) + 0.5)
    assert torch.equal(upsampled_pair(oa, la, ob, lb_, lab, (32, 32)), ohem_upsampled_pair(oa, la, ob, lb_, lab, (32, 32)))
    fa, fb = SoftmaxFocalLoss(2.0, ignore_lb=IGNORE), SoftmaxFocalLoss(0.5, weight=torch.rand(5, generator=g) + 0.5, ignore_lb=IGNORE)
    want = fa.forward_upsampled(la, lab, (32, 32)) + fb.forward_upsampled(lb_, lab, (32, 32))
    assert torch.equal(upsampled_pair(fa, la, fb, lb_, lab, (32, 32)), want)
    mixed = oa.forward_upsampled(la, lab, (32, 32)) + fb.forward_upsampled(lb_, lab, (32, 32))
    assert torch.equal(upsampled_pair(oa, la, fb, lb_, lab, (32, 32)), mixed)


def test_train_step_with_focal_criteria_on_cpu():
    """TrainStep goes through upsampled_pair: fused_loss=True no longer needs OHEM criteria."""
    from cabinet_amd.train import TrainStep, build_model, make_criteria, synthetic_batch

    net = build_model("small", n_classes=5, seed=0, device="cpu").train()
    im, lb = synthetic_batch(1, 64, 64, 5, "cpu", seed=1)
    losses = []
    for fused in (True, False):
        loss = TrainStep(net, make_criteria(1, 64, 64, "cpu", loss="focal", gamma=2.0), fused_loss=fused)(im, lb)
        losses.append(float(loss))
    assert losses[0] == losses[0] and abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[1]))
