"""HIP weight and input gradient of the 3x3 stride-2 convolutions (K15, through the C ABI) and the chip-wide slab sum of the stem's weight
gradient (K9) vs the oracle: fp64 F.conv2d(...).backward on the CPU, the call oracle/model_ref.py makes for cabinet.py:111-113
and mobilenetv3.py:173.

Two bounds on every gradient, both asserted: the suite's 1e-3 (||a-b|| / ||b||), and no worse than twice the stock operator's
own distance to the same fp64 result on the same inputs (the two differ only in summation order).  Both distances are printed."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3  # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32

# (B, H, W): one tile; both odd; Wo = 35 crosses a 32-wide tile; odd x even; fewer rows than a strip; conv3's plane at B = 1
CASES_64 = [(1, 8, 8), (2, 9, 11), (1, 16, 70), (3, 33, 34), (2, 7, 64), (1, 256, 256)]
CASES_3_16 = [(2, 18, 18), (1, 17, 19), (1, 64, 66)]


def _native_dw(g, x, Ci, Co):
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    lib = _lib.load()
    B, H, W = x.shape[0], x.shape[2], x.shape[3]
    dw = torch.full((Co, Ci, 3, 3), float("nan"), dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, Ci, Co, H, W), x.device)
    rc = lib.cabinet_conv3x3s2_wgrad(_ptr(g), _ptr(x), B, Ci, Co, H, W, _ptr(dw), _ptr(ws), nbytes, _stream_handle(x.device))
    _lib.check(rc, "cabinet_conv3x3s2_wgrad")
    return dw


def _native_dx(g, w, B, H, W):
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle

    dx = torch.full((B, 64, H, W), float("nan"), dtype=torch.float32, device=g.device)  # NaN: every element must be written
    rc = _lib.load().cabinet_conv3x3s2_dgrad(_ptr(g), _ptr(w), B, 64, 64, H, W, _ptr(dx), _stream_handle(g.device))
    _lib.check(rc, "cabinet_conv3x3s2_dgrad")
    return dx


def _stock_dw(g, x, w, stride, pad):
    return torch.ops.aten.convolution_backward(g, x, w, None, [stride] * 2, [pad] * 2, [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


def _inputs(B, Ci, Co, H, W, k, stride, pad):
    g0 = torch.Generator().manual_seed(B * 100003 + H * 1009 + W * 17 + Ci)
    x = torch.randn(B, Ci, H, W, generator=g0)
    w = torch.randn(Co, Ci, k, k, generator=g0)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = torch.randn(B, Co, Ho, Wo, generator=g0)
    wo, xo = w.double().requires_grad_(True), x.double().requires_grad_(True)
    F.conv2d(xo, wo, None, stride, pad).backward(g.double())
    return x, w, g, wo.grad, xo.grad


def _check(name, native, stock, ref):
    assert torch.isfinite(native).all()
    e_native, e_stock = rel_err(native, ref), rel_err(stock, ref)
    print(f"{name}: native {e_native:.3e}  stock {e_stock:.3e}")
    assert e_native <= TOL, f"{name}: {e_native:.3e} > {TOL}"
    assert e_native <= 2.0 * e_stock, f"{name}: native {e_native:.3e} > 2 x stock {e_stock:.3e}"


@pytest.mark.parametrize("Ci,Co,B,H,W", [(64, 64) + c for c in CASES_64] + [(3, 16) + c for c in CASES_3_16])
def test_conv3x3s2_wgrad_vs_oracle(Ci, Co, B, H, W):
    from cabinet_amd import _lib

    assert _lib.load().cabinet_conv3x3s2_supported(Ci, Co) == 1
    x, w, g, ref, _ = _inputs(B, Ci, Co, H, W, 3, 2, 1)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    dw = _native_dw(gd, xd, Ci, Co)
    stock = _stock_dw(gd, xd, wd, 2, 1)
    torch.cuda.synchronize()
    _check(f"conv3x3s2 dw B={B} {Ci}->{Co} {H}x{W}", dw, stock, ref)


@pytest.mark.parametrize("B,H,W", CASES_64)
def test_conv3x3s2_dgrad_vs_oracle(B, H, W):
    x, w, g, _, ref = _inputs(B, 64, 64, H, W, 3, 2, 1)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    dx = _native_dx(gd, wd, B, H, W)
    stock = torch.ops.aten.convolution_backward(gd, xd, wd, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1,
                                                [True, False, False])[0]
    torch.cuda.synchronize()
    assert dx.shape == stock.shape
    _check(f"conv3x3s2 dx B={B} 64->64 {H}x{W}", dx, stock, ref)


def test_conv3x3s2_argument_checks():
    from cabinet_amd import _lib

    lib = _lib.load()
    A = 0x10000
    assert lib.cabinet_conv3x3s2_supported(64, 64) == 1 and lib.cabinet_conv3x3s2_supported(3, 16) == 1
    for ci, co in [(64, 128), (32, 64), (3, 64), (16, 16), (0, 0)]:
        assert lib.cabinet_conv3x3s2_supported(ci, co) == 0
    assert lib.cabinet_conv3x3s2_wgrad_workspace_bytes(8, 64, 128, 64, 64) == 0
    assert lib.cabinet_conv3x3s2_wgrad(A, A, 8, 64, 128, 64, 64, A, A, 1 << 30, None) == -2
    assert lib.cabinet_conv3x3s2_wgrad(A, A, 8, 3, 64, 64, 64, A, A, 1 << 30, None) == -2
    assert lib.cabinet_conv3x3s2_wgrad(A, None, 8, 64, 64, 64, 64, A, A, 1 << 30, None) == -1
    assert lib.cabinet_conv3x3s2_wgrad(None, A, 8, 3, 16, 64, 64, A, A, 1 << 30, None) == -1
    assert lib.cabinet_conv3x3s2_wgrad(A, A, 8, 64, 64, 64, 64, None, A, 1 << 30, None) == -1
    assert lib.cabinet_conv3x3s2_wgrad(A, A, 0, 64, 64, 64, 64, A, A, 1 << 30, None) == -1
    for ci, co in [(64, 64), (3, 16)]:
        need = lib.cabinet_conv3x3s2_wgrad_workspace_bytes(8, ci, co, 64, 64)
        assert need > 0
        rc = lib.cabinet_conv3x3s2_wgrad(A, A, 8, ci, co, 64, 64, A, A, need - 1, None)
        assert rc == -3 and b"workspace" in lib.cabinet_last_error()
        rc = lib.cabinet_conv3x3s2_wgrad(A, A, 8, ci, co, 64, 64, A, None, need, None)
        assert rc == -3 and b"workspace" in lib.cabinet_last_error()
    assert lib.cabinet_conv3x3s2_dgrad(A, A, 8, 3, 16, 64, 64, A, None) == -2  # the image has no gradient
    assert lib.cabinet_conv3x3s2_dgrad(A, A, 8, 64, 128, 64, 64, A, None) == -2
    assert lib.cabinet_conv3x3s2_dgrad(A, A, 0, 64, 64, 64, 64, A, None) == -1
    assert lib.cabinet_conv3x3s2_dgrad(None, A, 8, 64, 64, 64, 64, A, None) == -1
    assert lib.cabinet_conv3x3s2_dgrad(A, None, 8, 64, 64, 64, 64, A, None) == -1
    assert lib.cabinet_conv3x3s2_dgrad(A, A, 8, 64, 64, 64, 64, None, None) == -1


@pytest.mark.parametrize("B,H,W", [(2, 9, 11), (1, 256, 256)])
def test_conv3x3s2_bit_reproducible_eager_and_graph(B, H, W):
    x = torch.randn(B, 64, H, W, device="cuda")
    g = torch.randn(B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device="cuda")
    w = torch.randn(64, 64, 3, 3, device="cuda")

    def both():
        return _native_dw(g, x, 64, 64), _native_dx(g, w, B, H, W)

    a, b = both(), both()
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()  # the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = both()
    for _ in range(2):
        c[0].fill_(float("nan"))
        c[1].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


def test_conv3x3s2_function_matches_stock_autograd():
    """Conv2dS2 against nn.Conv2d with the same weight: the forward is the stock operator's (bit for bit), dx the kernel's; dw the
    kernel's where it is routed (the 3 -> 16 layer on a plane of the model's size), else the stock operator's.  Forward hooks
    on the layer fire."""
    from cabinet_amd.functional import Conv2dS2, conv3x3s2_supported

    def conv3x3s2(x, conv):
        routed = Conv2dS2(conv.in_channels, conv.out_channels, 3, 2, 1, bias=False).cuda()
        routed.weight = conv.weight
        seen = []
        routed.register_forward_hook(lambda m, i, o: seen.append(o.dtype))
        y = routed(x)
        assert seen == [torch.float32] and type(y.grad_fn).__name__ == "_Conv3x3S2Backward"
        return y

    conv = torch.nn.Conv2d(64, 64, 3, 2, 1, bias=False).cuda()
    x = torch.randn(2, 64, 24, 21, device="cuda", requires_grad=True)
    g = torch.randn(2, 64, 12, 11, device="cuda")
    assert conv3x3s2_supported(conv, x)
    y0 = conv(x)
    y0.backward(g)
    dx0, dw0 = x.grad.clone(), conv.weight.grad.clone()
    x.grad = None
    conv.zero_grad()
    y1 = conv3x3s2(x, conv)
    y1.backward(g)
    assert torch.equal(y0, y1)
    assert x.grad.shape == dx0.shape and rel_err(x.grad, dx0) <= TOL
    assert conv.weight.grad.shape == dw0.shape and rel_err(conv.weight.grad, dw0) <= TOL
    first = torch.nn.Conv2d(3, 16, 3, 2, 1, bias=False).cuda()
    im = torch.randn(8, 3, 1024, 64, device="cuda")
    assert conv3x3s2_supported(first, im)
    y0 = first(im)
    g = torch.randn_like(y0)
    y0.backward(g)
    dw0 = first.weight.grad.clone()
    first.zero_grad()
    y1 = conv3x3s2(im, first)
    y1.backward(g)
    assert torch.equal(y0, y1) and rel_err(first.weight.grad, dw0) <= TOL
    from cabinet_amd.functional import _conv3x3s2_native_wgrad

    assert _conv3x3s2_native_wgrad(3, 8, 1024) and not _conv3x3s2_native_wgrad(3, 2, 2048)  # config 3 / config 5: as measured
    assert not _conv3x3s2_native_wgrad(64, 8, 512)
    # what keeps the stock path
    with torch.no_grad():
        assert not conv3x3s2_supported(conv, x)
    assert not conv3x3s2_supported(torch.nn.Conv2d(64, 64, 3, 2, 1, bias=True).cuda(), x)
    assert not conv3x3s2_supported(torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False).cuda(), x)
    assert not conv3x3s2_supported(torch.nn.Conv2d(64, 64, 3, 2, 0, bias=False).cuda(), x)
    assert not conv3x3s2_supported(torch.nn.Conv2d(64, 128, 3, 2, 1, bias=False).cuda(), x)
    assert not conv3x3s2_supported(torch.nn.Conv2d(64, 64, 3, 2, 1, bias=False), x.detach().cpu())
    assert not conv3x3s2_supported(torch.nn.Conv2d(64, 64, 3, 2, 1, bias=False).cuda().requires_grad_(False), x)
    with torch.autocast("cuda"):
        assert not conv3x3s2_supported(conv, x)


def _backward_nodes(outputs, name):
    seen, stack, n = set(), [o.grad_fn for o in outputs if o.grad_fn is not None], 0
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        n += type(fn).__name__ == name
        stack.extend(f for f, _ in fn.next_functions)
    return n


def test_model_step_routes_the_three_layers(monkeypatch):
    """A CABiNet training step with the route on and off: the forward is the stock operator's either way (the loss is bit-equal),
    the routed weight gradients agree, and the autograd graph holds one _Conv3x3S2Backward per routed layer."""
    from cabinet_amd import functional as Fh
    from cabinet_amd.train import TrainStep, build_model, make_criteria, synthetic_batch

    im, lb = synthetic_batch(2, 64, 64, 8, "cuda", seed=5)
    names = ["sb.conv1.conv.weight", "sb.conv2.conv.weight", "sb.conv3.conv.weight", "mobile.features.0.0.weight"]
    losses, grads, nodes = [], [], []
    for on in (True, False):
        monkeypatch.setattr(Fh, "CONV3X3S2_ENABLED", on)
        net = build_model("large", n_classes=8, seed=0, device="cuda").train()
        params = dict(net.named_parameters())
        assert all(n in params for n in names)
        nodes.append(_backward_nodes(net.forward_lowres(im), "_Conv3x3S2Backward"))
        net = build_model("large", n_classes=8, seed=0, device="cuda").train()  # fresh running statistics
        params = dict(net.named_parameters())
        step = TrainStep(net, make_criteria(2, 64, 64, "cuda"))
        losses.append(step(im, lb).clone())
        grads.append([params[n].grad.clone() for n in names])
    assert nodes == [3, 0]
    assert torch.equal(losses[0], losses[1])
    for n, a, b in zip(names, grads[0], grads[1]):
        e = rel_err(a, b)
        print(f"{n}: route on vs off {e:.3e}")
        assert torch.isfinite(a).all() and e <= TOL, f"{n}: {e:.3e}"


@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 33, 70)])
def test_stem_conv_wrw_slab_sum(B, H, W):
    """dw of cabinet_stem_conv_wrw (the slabs now summed by slab lanes on the whole chip) vs fp64; bit-reproducible."""
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    lib = _lib.load()
    x, w, g, ref, _ = _inputs(B, 3, 64, H, W, 7, 2, 3)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    outs = []
    for _ in range(2):
        dw = torch.full((64, 3, 7, 7), float("nan"), dtype=torch.float32, device="cuda")
        ws, nbytes = _workspace(lib.cabinet_stem_conv_wrw_workspace_bytes(B, H, W), xd.device)
        rc = lib.cabinet_stem_conv_wrw(_ptr(gd), _ptr(xd), B, H, W, _ptr(dw), _ptr(ws), nbytes, _stream_handle(xd.device))
        _lib.check(rc, "cabinet_stem_conv_wrw")
        outs.append(dw)
    stock = _stock_dw(gd, xd, wd, 2, 3)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    _check(f"stem dw B={B} {H}x{W}", outs[0], stock, ref)
