"""The BatchNorm finalize in its consumer kernel's prologue (K7 apply and dx, also behind K8's folded backward) against the two-launch plan
that CABINET_BN_PROLOGUE=0 restores: every workgroup of the consumer merges its channel's partials with the code of the
stand-alone finalize kernel, in the same order, so every output is the same bits -- outputs, saved statistics, running buffers,
parameter gradients.  Every buffer the wrappers allocate is pre-filled with NaN, so a channel whose writer workgroup did not run
shows up.  Shapes are the smallest that reach each branch: one value (the unbiased-variance guard), one chunk, a ragged last
chunk (scalar loads), several aligned chunks, an aligned plane whose last chunk is short (the unbranched loads of apply and dx
clamp their addresses there), partials per channel just below and just above the plan's cap, partials from the 3x3
convolution's epilogue with ragged tile blocks in both directions, and the depthwise backward's per-tile partials.

What the cap cases can and cannot show: nothing visible from Python tells which plan a call took, and both plans give the same
bits by construction, so the case above the cap shows that a call with more partials than the cap is still right -- not that it
took the stand-alone finalize.  MAX_NT mirrors BA_PROLOGUE_MAX_NT by hand; the launch counts on either side of it are read off
the kernel trace (profiles/bn_prologue_summary.md)."""
import contextlib

import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

CHUNK = 8192      # elements one workgroup streams (bn_finalize.hpp: BA_CHUNK)
MAX_NT = 1024     # partials per channel up to which the consumer merges them itself (bn_act.hip: BA_PROLOGUE_MAX_NT)
ACTS = [None, "relu", "hardswish"]


@contextlib.contextmanager
def _nan_buffers():
    """Everything the wrappers allocate with torch.empty / empty_like starts as NaN (byte workspaces stay as they are)."""
    real_empty, real_like = torch.empty, torch.empty_like

    def _fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t

    torch.empty = lambda *a, **k: _fill(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: _fill(real_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def _bn(C, training, seed=3):
    g0 = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g0) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=g0) - 0.5)
        bn.running_mean.copy_(torch.rand(C, generator=g0) - 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g0) + 0.5)
    return bn.cuda().train(training)


def _bn_act_once(monkeypatch, plan, x, g, bn0, act, residual, conv_part=None):
    """forward + backward of bn_act under CABINET_BN_PROLOGUE=plan on a copy of bn0 (fresh running buffers)."""
    import copy

    from cabinet_amd.functional import bn_act

    monkeypatch.setenv("CABINET_BN_PROLOGUE", plan)
    bn = copy.deepcopy(bn0)
    xd = x.clone().requires_grad_(True)
    with _nan_buffers():
        y = bn_act(xd, bn, act, residual, conv_part)
        mean, invstd = y.grad_fn.saved_tensors[3:5]
        y.backward(g)
    torch.cuda.synchronize()
    return {"y": y.detach(), "save_mean": mean, "save_invstd": invstd, "running_mean": bn.running_mean, "running_var": bn.running_var,
            "dx": xd.grad, "dweight": bn.weight.grad, "dbias": bn.bias.grad}


def _assert_same_bits(a, b):
    for k in a:
        assert not torch.isnan(a[k]).any(), f"{k}: NaN left in the default plan's result"
        assert torch.equal(a[k], b[k]), f"{k}: default plan differs from CABINET_BN_PROLOGUE=0 in {int((a[k] != b[k]).sum())} elements"


SHAPES = [(1, 1, 1), (2, 5, CHUNK), (3, 7, 2 * CHUNK + 5), (2, 16, 3 * CHUNK),
          (2, 3, CHUNK + 4),                      # aligned loads, a last chunk of four elements: clamped addresses
          (2, 1, (MAX_NT // 2) * CHUNK),          # nt = 1024: the last count the plan gives to the prologue
          (2, 1, (MAX_NT // 2) * CHUNK + 5)]      # nt = 1026: above the cap (and ragged loads)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bn_act_prologue_same_bits_as_two_launch_plan(monkeypatch, shape, act, with_residual, training):
    B, C, P = shape
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(B, C, 1, P, device="cuda", generator=gen) * 1.7 + 0.6
    g = torch.randn(B, C, 1, P, device="cuda", generator=gen)
    r = torch.randn(B, C, 1, P, device="cuda", generator=gen) if with_residual else None
    bn0 = _bn(C, training)
    res = [_bn_act_once(monkeypatch, plan, x, g, bn0, act, r) for plan in ("1", "0")]
    _assert_same_bits(*res)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("H,W", [(9, 70), (4, 32)])
def test_bn_act_from_conv_partials_same_bits(monkeypatch, H, W, act, training):
    """bn_act fed by the partials of the 3x3 convolution's epilogue: 4 x 32 tile blocks, ragged in both directions at 9 x 70."""
    import cabinet_amd.functional as Fh

    gen = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.randn(2, 64, H, W, device="cuda", generator=gen)
    w3 = torch.randn(64, 64, 3, 3, device="cuda", generator=gen) * 0.05
    part = Fh.conv3x3_bn_part(x0, 64)
    z = Fh.conv3x3(x0, w3, None, part).detach()
    g = torch.randn(2, 64, H, W, device="cuda", generator=gen)
    r = torch.randn(2, 64, H, W, device="cuda", generator=gen)
    bn0 = _bn(64, training)
    res = [_bn_act_once(monkeypatch, plan, z, g, bn0, act, r, part) for plan in ("1", "0")]
    _assert_same_bits(*res)


def _bn_dw_once(monkeypatch, plan, z, g, bn0, conv0, act):
    import copy

    from cabinet_amd.functional import bn_act_dwconv

    monkeypatch.setenv("CABINET_BN_PROLOGUE", plan)
    bn, conv = copy.deepcopy(bn0), copy.deepcopy(conv0)
    zd = z.clone().requires_grad_(True)
    with _nan_buffers():
        y = bn_act_dwconv(zd, bn, act, conv)
        mean, invstd = y.grad_fn.saved_tensors[4:6]
        y.backward(g)
    torch.cuda.synchronize()
    return {"y": y.detach(), "save_mean": mean, "save_invstd": invstd, "running_mean": bn.running_mean, "running_var": bn.running_var,
            "dz": zd.grad, "dbn_weight": bn.weight.grad, "dbn_bias": bn.bias.grad, "dconv_weight": conv.weight.grad}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", ["relu", "hardswish"])
@pytest.mark.parametrize("S", [1, 2])
def test_bn_act_dwconv_same_bits(monkeypatch, S, act, training):
    """BatchNorm folded into the depthwise convolution: the backward's dx pass merges the per-tile partials the convolution's
    backward wrote (33 x 34: two tiles per plane, ragged); the forward keeps the stand-alone finalize under either plan."""
    B, C, H, W = 2, 5, 33, 34
    gen = torch.Generator(device="cuda").manual_seed(7 + S)
    conv0 = torch.nn.Conv2d(C, C, 3, S, 1, groups=C, bias=False).cuda()
    z = torch.randn(B, C, H, W, device="cuda", generator=gen) * 1.5 + 0.3
    Ho, Wo = (H - 1) // S + 1, (W - 1) // S + 1
    g = torch.randn(B, C, Ho, Wo, device="cuda", generator=gen)
    bn0 = _bn(C, training)
    res = [_bn_dw_once(monkeypatch, plan, z, g, bn0, conv0, act) for plan in ("1", "0")]
    _assert_same_bits(*res)


def test_bn_act_prologue_vs_fp64_oracle():
    """The default plan against fp64 F.batch_norm + HardSwish (the oracle and the bounds of test_gpu_bn_act.py)."""
    from cabinet_amd.functional import bn_act
    from test_gpu_bn_act import TOL, _oracle

    B, C, P = 3, 7, 2 * CHUNK + 5
    g0 = torch.Generator().manual_seed(4)
    bn = _bn(C, True).cpu()
    x = torch.randn(B, C, 1, P, generator=g0) * 1.7 + 0.6
    g = torch.randn(B, C, 1, P, generator=g0)
    ref = _oracle(x, g, bn, "hardswish", True)
    bn = bn.cuda().train()
    xd = x.cuda().requires_grad_(True)
    y = bn_act(xd, bn, "hardswish")
    y.backward(g.cuda())
    torch.cuda.synchronize()
    assert_close(y, ref[0], TOL, "y")
    assert_close(xd.grad, ref[1], TOL, "dx")
    assert_close(bn.weight.grad, ref[2], TOL, "dweight")
    assert_close(bn.bias.grad, ref[3], TOL, "dbias")
    assert_close(bn.running_mean, ref[4], 1e-5, "running_mean")
    assert_close(bn.running_var, ref[5], 1e-5, "running_var")


def test_bn_prologue_graph_replay_same_bits_as_eager():
    """forward + backward of one bn_act and one bn_act_dwconv captured in a graph and replayed twice: the same bits as the eager
    calls from the same running buffers -- nothing in the prologue path depends on what ran before.  Captured the way
    GraphedTrainStep captures the model's step: after an eager step, in the thread-local capture mode (autograd's worker thread
    enqueues the backward; under the global mode its event calls are errors while a capture is open)."""
    from cabinet_amd.functional import bn_act, bn_act_dwconv

    gen = torch.Generator(device="cuda").manual_seed(2)
    B, C, H, W = 2, 6, 90, 97          # 8730 elements: two chunks, the second ragged; two depthwise tiles per plane
    x = torch.randn(B, C, H, W, device="cuda", generator=gen).requires_grad_(True)
    g = torch.randn(B, C, H, W, device="cuda", generator=gen)
    bn1, bn2 = _bn(C, True, 1), _bn(C, True, 2)
    conv = torch.nn.Conv2d(C, C, 3, 1, 1, groups=C, bias=False).cuda()
    params = [x, bn1.weight, bn1.bias, bn2.weight, bn2.bias, conv.weight]
    buffers = [bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var]
    start = [b.clone() for b in buffers]

    def step():
        for p in params:
            p.grad = None
        y = bn_act_dwconv(bn_act(x, bn1, "hardswish"), bn2, "relu", conv)
        y.backward(g)
        return [y.detach()] + [p.grad for p in params]

    def reset():
        with torch.no_grad():
            for b, s in zip(buffers, start):
                b.copy_(s)

    eager = [t.clone() for t in step()] + [b.clone() for b in buffers]
    reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = step()
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(outs + buffers, eager)):
            assert torch.equal(a, b), f"replayed tensor {i} differs from the eager result"
