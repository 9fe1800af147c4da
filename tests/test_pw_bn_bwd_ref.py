"""No device: (1) the fp64 formulas the GPU tests of the fused thin-convolution + BatchNorm backward compare with
(tests/pw_bn_bwd_cases.py) equal autograd through conv2d + batch_norm (+ activation, shortcut, depthwise convolution) in float64;
(2) the Python linkage leaves host tensors and frozen parameters on the path they took before."""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pw_bn_bwd_cases as pc  # noqa: E402

EPS = 1e-5


def _act(u, act):
    return {"none": lambda t: t, "relu": F.relu, "hardswish": F.hardswish}[act](u)


def _autograd(d, act, training, shortcut, dw=None):
    """float64 autograd of act(bn(conv1x1(x))) [+ x] or conv_dw(act(bn(conv1x1(x)))) with batch (training) or given statistics."""
    x = d["x"].double().requires_grad_(True)
    w, gam, bet = (d[k].double().requires_grad_(True) for k in ("w", "gamma", "beta"))
    z = F.conv2d(x, w[:, :, None, None])
    if training:
        rm, rv = torch.zeros_like(gam).detach(), torch.ones_like(gam).detach()
    else:
        rm, rv = d["mean"].double(), 1.0 / d["invstd"].double() ** 2 - EPS
    y = _act(F.batch_norm(z, rm, rv, gam, bet, training, 0.1, EPS), act)
    if shortcut:
        y = y + x
    cw = None
    if dw is not None:
        cw = d["cw"].double().requires_grad_(True)
        y = F.conv2d(y, cw, None, dw[1], dw[0] // 2, 1, cw.shape[0])
    y.backward(d["g"].double().reshape(y.shape))
    return z.detach(), dict(dx=x.grad, dw=w.grad, dgamma=gam.grad, dbeta=bet.grad, dcw=None if cw is None else cw.grad)


@pytest.mark.parametrize("shape", [(2, 16, 16, 5, 7), (3, 24, 72, 9, 4), (1, 64, 24, 13, 3)], ids=str)
@pytest.mark.parametrize("act", ["none", "relu", "hardswish"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_formulas_equal_float64_autograd(shape, act, training):
    B, Ci, Co, H, W = shape
    d = pc.dw_inputs(B, Ci, Co, H, W, 3, 1)
    d["g"] = torch.randn(B, Co, H, W, generator=torch.Generator().manual_seed(3))
    shortcut = Ci == Co
    z, auto = _autograd(d, act, training, shortcut)
    if training:  # the statistics the BatchNorm used
        d["mean"], d["invstd"] = z.mean((0, 2, 3)), 1.0 / (z.var((0, 2, 3), unbiased=False) + EPS).sqrt()
    ref = pc.bn_pw_ref(d["g"], z, d["x"], d["w"], d["gamma"], d["beta"], d["mean"], d["invstd"], act, training)
    want_dx = auto["dx"].flatten(2) - (d["g"].double().flatten(2) if shortcut else 0.0)  # the shortcut's gradient is g itself
    for k, a in (("dx", want_dx), ("dw", auto["dw"]), ("dgamma", auto["dgamma"]), ("dbeta", auto["dbeta"])):
        assert pc.dist(ref[k].reshape(a.shape), a) < 1e-11, k


@pytest.mark.parametrize("shape", [(2, 16, 64, 5, 7, 3, 2), (3, 24, 72, 9, 4, 5, 1), (2, 8, 8, 1, 1, 3, 1)], ids=str)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_depthwise_formulas_equal_float64_autograd(shape, training):
    B, Ci, C, H, W, K, stride = shape
    act = "relu" if K == 3 else "hardswish"
    d = pc.dw_inputs(B, Ci, C, H, W, K, stride)
    z, auto = _autograd(d, act, training, False, dw=(K, stride))
    d["z"] = z
    if training:
        d["mean"], d["invstd"] = z.mean((0, 2, 3)), 1.0 / (z.var((0, 2, 3), unbiased=False) + EPS).sqrt()
    ref = pc.dw_ref(d, K, stride, act, training)
    for k in ("dx", "dw", "dgamma", "dbeta", "dcw"):
        assert pc.dist(ref[k].reshape(auto[k].shape), auto[k]) < 1e-11, k


def test_case_tables_cover_what_the_kernel_branches_on():
    shapes = {(c[1], c[2]) for c in pc.ACT_CASES}
    assert shapes >= {(8, 8), (16, 16), (16, 64), (64, 24), (24, 72), (72, 24), (96, 96)}
    assert {c[0] for c in pc.ACT_CASES} == {1, 2, 3}
    assert {c[3] for c in pc.ACT_CASES} >= {1, 5, 63, 64, 65, 127, 129, 449, 1000, 4099}
    assert {(c[4], c[5]) for c in pc.ACT_CASES} == {(a, t) for a in pc.ACTS for t in (True, False)}
    assert {c[6] for c in pc.ACT_CASES} == {0, 1, 2} and any(not c[7] for c in pc.ACT_CASES) and any(not c[8] for c in pc.ACT_CASES)
    assert {(c[5], c[6]) for c in pc.DW_CASES} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    assert {(c[3], c[4]) for c in pc.DW_CASES} == {(1, 1), (7, 9), (33, 65)}
    B, _, _, P = pc.LOADED_CASE[:4]
    assert B * ((P + 63) // 64) >= 4 * 512  # the full grid, four chunks or more per workgroup


def test_linkage_leaves_host_tensors_and_frozen_parameters_alone(monkeypatch):
    import cabinet_amd.functional as fn
    from cabinet_amd.models.mobilenetv3 import InvertedResidual

    def never(*a):
        raise AssertionError("the fused node was taken")

    monkeypatch.setattr(fn._PwBnAct, "apply", staticmethod(never))
    monkeypatch.setattr(fn._PwBnActDwConv, "apply", staticmethod(never))
    monkeypatch.setattr(fn, "PW_BN_BWD_FUSED", True)
    mod = InvertedResidual(16, 64, 24, 3, 2, False, False)
    x = torch.randn(2, 16, 8, 8, requires_grad=True)
    mod(x).sum().backward()  # host tensors: the stock modules
    assert x.grad is not None and all(p.grad is not None for p in mod.parameters())

    bn, conv = nn.BatchNorm2d(8), nn.Conv2d(8, 8, 1, bias=False)
    z = torch.randn(2, 8, 4, 4, requires_grad=True)
    assert fn._pw_bn_source(z, bn) is None                      # not a pwconv output
    z._pw_src = (torch.randn(2, 8, 4, 4), conv.weight)
    for frozen in (conv.weight, bn.weight, bn.bias):
        frozen.requires_grad_(False)
        assert fn._pw_bn_source(z, bn) is None, "a frozen parameter must fall back to the two nodes"
        frozen.requires_grad_(True)
    extra = nn.Parameter(torch.randn(8, 1, 3, 3), requires_grad=False)
    assert fn._pw_bn_source(z, bn, extra) is None               # the depthwise weight frozen
    with torch.no_grad():
        assert fn._pw_bn_source(z, bn) is None                  # nothing is being recorded
    monkeypatch.setattr(fn, "PW_BN_BWD_FUSED", False)
    assert fn._pw_bn_source(z, bn) is None                      # the flag
