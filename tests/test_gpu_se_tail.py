"""The squeeze-excite tail `BatchNorm -> SELayer -> act` of the MBConv blocks as one operator (functional.se_tail):
against the stock modules in fp64 (output, dz, BatchNorm and SE-MLP parameter gradients, running buffers) in train and
eval mode; forward bitwise equal to the composed operators it replaces; two runs bitwise equal.
Shapes: the squeeze-excite blocks of the large backbone at the 1024 x 1024 benchmark size, B = 2, and ragged planes
(H*W % 4 != 0, planes that are not a multiple of the 8192-element chunk)."""
import copy

import pytest
import torch
import torch.nn as nn

from conftest import assert_close

pytestmark = pytest.mark.gpu
TOL = 1e-3  # as tests/test_gpu_bn_act.py: 1e-3 relative per tensor for outputs and gradients; 1e-5 for running statistics

# (C, H, W, act) of the BatchNorm input: blocks 4-6 (ReLU) and 11-15 (HardSwish), then ragged planes
SHAPES = [(72, 128, 128, "relu"), (120, 128, 128, "relu"), (480, 64, 64, "hardswish"), (672, 64, 64, "hardswish"),
          (672, 32, 32, "hardswish"), (960, 32, 32, "hardswish"),
          (24, 37, 29, "relu"), (16, 23, 7, "hardswish"), (40, 90, 91, None), (8, 1, 1, "relu")]


def _case(shape, training, seed=7):
    from cabinet_amd.models.mobilenetv3 import HardSwish, SELayer

    C, H, W, act = shape
    g0 = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    se = SELayer(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g0) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=g0) - 0.5)
        bn.running_mean.copy_(torch.rand(C, generator=g0) - 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g0) + 0.5)
        for m in (se.fc[0], se.fc[2]):  # spread the gate over the whole hard-sigmoid range (both clamps are hit)
            m.weight.copy_(torch.randn(m.weight.shape, generator=g0) * (3.0 / m.in_features ** 0.5))
            m.bias.copy_(torch.randn(m.bias.shape, generator=g0))
    z = torch.randn(2, C, H, W, generator=g0) * 1.3 + 0.4
    g = torch.randn(2, C, H, W, generator=g0)
    mods = nn.ModuleList([bn, se, {"relu": nn.ReLU(), "hardswish": HardSwish(), None: nn.Identity()}[act]]).train(training)
    return mods, z, g, act


def _device_run(mods, z, g, act):
    from cabinet_amd.functional import se_tail

    zd = z.cuda().requires_grad_(True)
    y = se_tail(zd, mods[0], mods[1], act)
    y.backward(g.cuda())
    torch.cuda.synchronize()
    return y, zd.grad


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_se_tail_vs_stock_modules_fp64(shape, training):
    mods, z, g, act = _case(shape, training)
    ref = copy.deepcopy(mods).double()
    zo = z.double().requires_grad_(True)
    yo = zo
    for m in ref:
        yo = m(yo)
    yo.backward(g.double())
    dev = mods.cuda()
    y, dz = _device_run(dev, z, g, act)
    assert_close(y, yo, TOL, "y")
    assert_close(dz, zo.grad, TOL, "dz")
    for (k, p), (_, q) in zip(dev.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, TOL, k)
    for (k, p), (_, q) in zip(dev.named_buffers(), ref.named_buffers()):
        if p.is_floating_point():
            assert_close(p, q, 1e-5, k)
        else:
            assert int(p) == int(q), k


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", [(480, 64, 64, "hardswish"), (24, 37, 29, "relu")])
def test_se_tail_forward_is_the_composed_forward_bitwise(shape, training):
    """Same kernels as bn_act -> SELayer.gate -> gate_act: y and the running buffers are bit for bit the composed form's;
    the gradients agree to TOL."""
    from cabinet_amd.functional import bn_act, gate_act

    mods, z, g, act = _case(shape, training, seed=3)
    a, b = mods.cuda(), copy.deepcopy(mods).cuda()
    y, dz = _device_run(a, z, g, act)
    zb = z.cuda().requires_grad_(True)
    x = bn_act(zb, b[0], None)
    yb = gate_act(x, b[1].gate(x), act)
    yb.backward(g.cuda())
    assert torch.equal(y, yb)
    assert torch.equal(a[0].running_mean, b[0].running_mean) and torch.equal(a[0].running_var, b[0].running_var)
    assert_close(dz, zb.grad, TOL, "dz")
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert_close(p.grad, q.grad, TOL, k)


@pytest.mark.parametrize("training", [True, False])
def test_se_tail_is_deterministic(training):
    runs = []
    for _ in range(2):
        mods, z, g, act = _case((672, 64, 64, "hardswish"), training, seed=9)
        dev = mods.cuda()
        y, dz = _device_run(dev, z, g, act)
        runs.append([y, dz] + [p.grad for p in dev.parameters()] + list(dev.buffers()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
