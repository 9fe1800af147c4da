"""The native NCHW forward of the 64 -> 64 3x3 stride-2 convolutions (K15, cabinet_conv3x3s2_fwd): the entry point called directly,
whatever the routing rule says, over tests/fwd64_cases.py (every branch of cv_plan, and the edge sweep B x H x W around the tile
width T):

  accuracy     against fp64 F.conv2d on the CPU under the two bounds of test_gpu_conv3x3s2.py::_check (1e-3, and no worse than
               twice the stock operator's own distance, the stock forward computed on the device in the same test)
  neighbours   x and w inside NaN-filled allocations, y inside a sentinel-filled one, all at an odd element offset: the same
               bits, every element written, sentinels intact (a clamped load that leaks into a sum, a mask applied by
               multiplication, a store past the tensor)
  reproducible two calls give equal bits; an image gives the same bits at b = 0 and at b = 2 of a batch of 3
  captured     two replays of one captured graph give the eager call's bits

and the routing: the rule (functional.py::_conv3x3s2_native_fwd64), _Conv3x3S2.forward, Conv2dS2 under no_grad, the error codes."""
import functools

import pytest
import torch
import torch.nn.functional as F

import fwd64_cases as fc
from conftest import rel_err

gpu = pytest.mark.gpu
TOL = 1e-3  # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32
PAD = 1031  # elements of NaN / sentinel on either side of a tensor (odd: the tensors sit at 4-byte, not 16-byte, alignment)
SENTINEL = -12345.5
IDS = ["x".join(map(str, s)) for s in fc.SHAPES]
EDGE_BH = [(b, h) for b in fc.EDGE_B for h in fc.EDGE_H]


def test_plans_match_the_table():
    """The Python restatement of cv_plan gives the plans the cases were chosen for, and the table reaches every branch (CPU only)."""
    from cabinet_amd.functional import _conv3x3s2_fwd64_plan

    for shape, want in fc.PLANS.items():
        assert fc.plan(*shape) == want, (shape, fc.plan(*shape))
        tiles, strips, rows_per = want
        assert _conv3x3s2_fwd64_plan(*shape) == (shape[0] * tiles * strips, rows_per)  # the routing rule reads the same plan
    plans = list(fc.PLANS.items())
    assert any(p[1] == 1 for _, p in plans), "one strip per image"
    assert any(p[1] > 1 for _, p in plans), "several strips"
    assert any(p[2] >= 2 and fc.out_hw(s[1], s[2])[0] % p[2] != 0 for s, p in plans), "a last strip shorter than the others"
    assert any(p[2] >= 2 and s[0] * p[0] * fc.out_hw(s[1], s[2])[0] > fc.TARGET_WG for s, p in plans), "rows_per >= 2 past the target"
    assert fc.plan(4, 300, 2 * fc.T)[2] == 2
    assert any(p[0] > 1 for _, p in plans), "more than one column tile"
    # the benchmark's layers: 512 workgroups each
    for shape, want in {(8, 512, 512): (8, 8, 32), (8, 256, 256): (4, 16, 8), (2, 1024, 512): (8, 32, 16),
                        (2, 512, 256): (4, 64, 4)}.items():
        assert fc.plan(*shape) == want, shape


def test_rule_routes_the_measured_shapes_only():
    """The rule of the summary's table: at least one workgroup per CU, each with a strip of at least two rows.  The measured
    layers (config 3, config 5, one 1024 x 2048 image) are routed; the shapes other tests pin to the stock forward are not."""
    from cabinet_amd import functional as Fh

    assert (Fh._CV_TILE, Fh._CV_MIN_WORKGROUPS, Fh._CV_MIN_ROWS) == (fc.T, 256, 2)
    for name, shape in fc.BENCH_SHAPES.items():
        assert Fh._conv3x3s2_native_fwd64(*shape), name
        tiles, strips, rows_per = fc.plan(*shape)
        assert shape[0] * tiles * strips == fc.TARGET_WG and rows_per >= 2
    assert min(fc.plan(*s)[2] for s in fc.BENCH_SHAPES.values()) == Fh._CV_MIN_ROWS  # the threshold is the shortest strip measured
    for shape in fc.STOCK_SHAPES:
        assert not Fh._conv3x3s2_native_fwd64(*shape), shape
    assert Fh._conv3x3s2_native_fwd64(*ROUTED) and not Fh._conv3x3s2_native_fwd64(*UNROUTED)
    assert not Fh._conv3x3s2_native_fwd64(255, 4, 8) and not Fh._conv3x3s2_native_fwd64(1, 512, 16)  # 510 and 256 one-row strips


@functools.lru_cache(maxsize=None)
def _fwd(shape):
    """-> x, w on the device and the plain result (computed once, shared, never written again)."""
    x, w = fc.inputs(*shape)
    x, w = x.cuda(), w.cuda()
    y = fc.run_fwd(x, w)
    torch.cuda.synchronize()
    return x, w, y


def _check(name, x, w, y):
    assert bool(torch.isfinite(y).all()), f"{name}: an element was not written, or is not finite"
    ref = F.conv2d(x.double().cpu(), w.double().cpu(), None, 2, 1)
    stock = F.conv2d(x, w, None, 2, 1)
    assert y.shape == ref.shape
    e_native, e_stock = rel_err(y, ref), rel_err(stock, ref)
    print(f"{name}: native {e_native:.3e}  stock {e_stock:.3e}")
    assert e_native <= TOL, f"{name}: {e_native:.3e} > {TOL}"
    assert e_native <= 2.0 * e_stock, f"{name}: native {e_native:.3e} > 2 x stock {e_stock:.3e}"


@gpu
@pytest.mark.parametrize("shape", fc.SHAPES, ids=IDS)
def test_fwd64_vs_fp64(shape):
    x, w, y = _fwd(shape)
    _check(f"fwd64 {shape}", x, w, y)


@gpu
@pytest.mark.parametrize("B,H", EDGE_BH)
def test_fwd64_edge_sweep_vs_fp64(B, H):
    for W in fc.EDGE_W:
        x, w = fc.inputs(B, H, W)
        x, w = x.cuda(), w.cuda()
        _check(f"fwd64 edge {(B, H, W)}", x, w, fc.run_fwd(x, w))


def _inside(t, pad, fill):
    """A contiguous copy of t in the middle of a larger allocation filled with `fill` -> (view, whole buffer)."""
    buf = torch.full((t.numel() + 2 * pad,), fill, device="cuda")
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _neighbours(x, w, y):
    xv, _ = _inside(x, PAD, float("nan"))
    wv, _ = _inside(w, PAD, float("nan"))
    yv, ybuf = _inside(torch.full_like(y, float("nan")), PAD, SENTINEL)
    assert xv.data_ptr() % 8 == 4 and yv.data_ptr() % 8 == 4  # 4-byte alignment only
    fc.run_fwd(xv, wv, yv)
    torch.cuda.synchronize()
    assert torch.equal(yv, y), "a NaN beside x or w reached a sum, or an element of y was not written"
    assert bool((ybuf[:PAD] == SENTINEL).all()) and bool((ybuf[-PAD:] == SENTINEL).all()), "y: written outside the tensor"


@gpu
@pytest.mark.parametrize("shape", fc.SHAPES, ids=IDS)
def test_fwd64_neighbours(shape):
    _neighbours(*_fwd(shape))


@gpu
@pytest.mark.parametrize("B,H", EDGE_BH)
def test_fwd64_edge_sweep_neighbours(B, H):
    for W in fc.EDGE_W:
        x, w = fc.inputs(B, H, W)
        x, w = x.cuda(), w.cuda()
        y = fc.run_fwd(x, w)
        assert bool(torch.isfinite(y).all())
        _neighbours(x, w, y)


@gpu
@pytest.mark.parametrize("shape", fc.SHAPES, ids=IDS)
def test_fwd64_twice_same_bits(shape):
    x, w, y = _fwd(shape)
    again = fc.run_fwd(x, w)
    torch.cuda.synchronize()
    assert torch.equal(again, y)


@gpu
@pytest.mark.parametrize("H,W", [(9, 2 * fc.T + 7), (41, 11), (400, 8)])
def test_fwd64_same_bits_at_any_batch_index(H, W):
    """The same image at b = 0 and b = 2 of a batch of 3, and alone: the plan differs at (400, 8) (two-row strips at B 3, one-row strips at B 1), the bits do not."""
    x, w = fc.inputs(3, H, W)
    x[2] = x[0]
    x, w = x.cuda(), w.cuda()
    y = fc.run_fwd(x, w)
    alone = fc.run_fwd(x[:1].contiguous(), w)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y[0], y[2]) and not torch.equal(y[0], y[1])
    assert torch.equal(alone[0], y[0])


@gpu
@pytest.mark.parametrize("shape", fc.SHAPES, ids=IDS)
def test_fwd64_captured_matches_eager(shape):
    x, w, y = _fwd(shape)
    out = torch.empty_like(y)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        fc.run_fwd(x, w, out)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, y)


# (B, H, W) of x: a plane the rule routes (260 workgroups of 4 rows) and one it leaves to the stock operator
ROUTED, UNROUTED = (260, 8, 8), (2, 24, 21)


def _layer(shape, seed):
    from cabinet_amd import functional as Fh

    B, H, W = shape
    g0 = torch.Generator().manual_seed(seed)
    conv = Fh.Conv2dS2(64, 64, 3, 2, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 64, 3, 3, generator=g0) * 0.05)
    x = torch.randn(B, 64, H, W, generator=g0).cuda()
    g = torch.randn(B, 64, *fc.out_hw(H, W), generator=g0).cuda()
    return conv.cuda(), x, g


def _count(fn, name="_Conv3x3S2Backward"):
    seen, todo, n = set(), [fn], 0
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        n += type(f).__name__ == name
        todo += [nf for nf, _ in f.next_functions]
    return n


@gpu
def test_training_forward_routes_by_the_rule(monkeypatch):
    """A Conv2dS2 that records a graph gives the entry point's bits at a routed shape and the stock operator's at an unrouted
    one, builds one _Conv3x3S2Backward node either way, and its gradients do not depend on which forward ran."""
    from cabinet_amd import functional as Fh

    assert Fh.CONV3X3S2_FWD64_ENABLED and Fh._conv3x3s2_native_fwd64(*ROUTED) and not Fh._conv3x3s2_native_fwd64(*UNROUTED)
    for shape, native in ((ROUTED, True), (UNROUTED, False)):
        conv, x, g = _layer(shape, 4100 + shape[0])
        xr = x.clone().requires_grad_(True)
        y = conv(xr)
        assert type(y.grad_fn).__name__ == "_Conv3x3S2Backward" and _count(y.grad_fn) == 1
        want = fc.run_fwd(x, conv.weight.detach()) if native else F.conv2d(x, conv.weight.detach(), None, 2, 1)
        assert torch.equal(y.detach(), want), shape
        y.backward(g)
        dx, dw = xr.grad.clone(), conv.weight.grad.clone()
        conv.weight.grad = None
        with monkeypatch.context() as m:
            m.setattr(Fh, "CONV3X3S2_FWD64_ENABLED", False)
            assert not Fh._conv3x3s2_native_fwd64(*shape)
            xs = x.clone().requires_grad_(True)
            ys = conv(xs)
            assert torch.equal(ys.detach(), F.conv2d(x, conv.weight.detach(), None, 2, 1))
            ys.backward(g)
        e_y, e_dx, e_dw = rel_err(y, ys), rel_err(dx, xs.grad), rel_err(dw, conv.weight.grad)
        print(f"{shape}: y {e_y:.3e}  dx {e_dx:.3e}  dw {e_dw:.3e}")
        assert e_y <= TOL and e_dx <= TOL and e_dw <= TOL


@gpu
def test_no_grad_forward_routes_by_the_rule():
    """Under no_grad (evaluation, inference) the layer calls the entry point directly at a routed shape -- its bits, no autograd
    node, conv3x3s2_supported still false -- and its forward hook fires; an unrouted shape keeps the stock operator."""
    from cabinet_amd import functional as Fh

    for shape, native in ((ROUTED, True), (UNROUTED, False)):
        conv, x, _ = _layer(shape, 4200 + shape[0])
        conv.eval()
        fired = []
        handle = conv.register_forward_hook(lambda m, a, out: fired.append(tuple(out.shape)))
        with torch.no_grad():
            assert not Fh.conv3x3s2_supported(conv, x)
            y = conv(x)
        handle.remove()
        assert fired == [tuple(y.shape)] and y.grad_fn is None and not y.requires_grad
        want = fc.run_fwd(x, conv.weight.detach()) if native else F.conv2d(x, conv.weight.detach(), None, 2, 1)
        assert torch.equal(y, want), shape
    conv, x, _ = _layer(ROUTED, 4300)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert conv(x).dtype == torch.bfloat16  # autocast keeps the stock operator


@gpu
def test_entry_point_error_codes():
    """Null pointers and (Ci, Co) != (64, 64) are refused before any HIP call: the pointers given here are not device memory."""
    from cabinet_amd import _lib

    lib = _lib.load()
    assert lib.cabinet_abi_version() == 8
    assert lib.cabinet_conv3x3s2_fwd_supported(64, 64) == 1
    for ci, co in ((3, 16), (64, 32), (32, 64), (16, 16), (64, 128)):
        assert lib.cabinet_conv3x3s2_fwd_supported(ci, co) == 0
    assert lib.cabinet_conv3x3s2_supported(64, 64) == 1 and lib.cabinet_conv3x3s2_supported(3, 16) == 1  # not widened, not narrowed
    bad = 4096  # never dereferenced
    invalid, unsupported = lib.cabinet_conv3x3s2_fwd(None, bad, 1, 64, 64, 4, 4, bad, None), \
        lib.cabinet_conv3x3s2_fwd(bad, bad, 1, 3, 16, 4, 4, bad, None)
    assert invalid != 0 and unsupported != 0 and invalid != unsupported
    assert b"Ci=3" in lib.cabinet_last_error()
    assert lib.cabinet_conv3x3s2_fwd(bad, None, 1, 64, 64, 4, 4, bad, None) == invalid
    assert lib.cabinet_conv3x3s2_fwd(bad, bad, 1, 64, 64, 4, 4, None, None) == invalid
    assert lib.cabinet_conv3x3s2_fwd(bad, bad, 0, 64, 64, 4, 4, bad, None) == invalid
    assert lib.cabinet_conv3x3s2_fwd(bad, bad, 1, 64, 64, 0, 4, bad, None) == invalid
    assert lib.cabinet_conv3x3s2_fwd(bad, bad, 1, 64, 128, 4, 4, bad, None) == unsupported
