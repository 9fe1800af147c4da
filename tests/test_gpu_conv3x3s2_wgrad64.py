"""The pipelined staging of the 64 -> 64 weight gradient of the 3x3 stride-2 convolutions (K15, cabinet_conv3x3s2_wgrad): whole-wave,
clamped, zero-selected row-segment loads, the next step's rows in registers under the MFMAs, the three-slot ring of input rows.
The arithmetic of the kernel is frozen, so per shape (tests/wgrad64_cases.py: every edge of the new staging):

  bits       dW is bit for bit what the commit before the change computed (tests/golden/g12_wgrad64.npz, written by
             tests/golden/make_golden_wgrad64.py on that commit's library: SHA-256 of dW and a strided sample)
  accuracy   against fp64 F.conv2d(...).backward on the CPU under the two bounds of test_gpu_conv3x3s2.py (1e-3, and no worse than
             twice the stock operator's own distance)
  neighbours x and dy inside NaN-filled allocations, dW inside a sentinel-filled one: the same bits, sentinel intact (a clamped
             load that leaks into a sum, a mask applied by multiplication, a store past the tensor)
  captured   two replays of one captured graph give the eager call's bits

and the routing of _Conv3x3S2.backward (functional.py::_conv3x3s2_native_wgrad64)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad64_cases as wc
from conftest import GOLDEN, rel_err

gpu = pytest.mark.gpu
TOL = 1e-3  # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32
PAD = 1031  # elements of NaN / sentinel on either side of a tensor (odd: the tensors sit at 4-byte, not 16-byte, alignment)
SENTINEL = -12345.5
IDS = ["x".join(map(str, s)) for s in wc.SHAPES]


def test_plans_match_the_table():
    """The Python restatement of cw_plan gives the plans the cases were chosen for (CPU only)."""
    for shape, want in wc.PLANS.items():
        assert wc.plan(*shape) == want, shape
    rows = {p[2] for p in wc.PLANS.values()}
    assert {1, 2, 3, 4, 7, 9} <= rows
    B, H, W = 1, 1025, 6
    assert wc.out_hw(H, W)[0] % wc.plan(B, H, W)[2] == 1  # a one-row last strip
    # the benchmark's layers: 512 workgroups each
    for shape, want in {(8, 512, 512): (8, 8, 32), (8, 256, 256): (4, 16, 8), (2, 1024, 512): (8, 32, 16),
                        (2, 512, 256): (4, 64, 4)}.items():
        assert wc.plan(*shape) == want, shape


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(os.path.join(GOLDEN, "g12_wgrad64.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _wgrad(shape):
    """-> x, dy on the device and the plain result (computed once, shared, never written again)."""
    x, dy = wc.inputs(*shape)
    x, dy = x.cuda(), dy.cuda()
    dw = wc.run_wgrad(wc.load_library(), dy, x, torch.full((64, 64, 3, 3), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    return x, dy, dw


@gpu
@pytest.mark.parametrize("shape", wc.SHAPES, ids=IDS)
def test_wgrad64_bits_match_parent(shape):
    dw = _wgrad(shape)[2]
    assert bool(torch.isfinite(dw).all()), "an element was not written, or is not finite"
    g = _golden()
    k = wc.key(shape)
    want = torch.from_numpy(g[k + "/sample"])
    got = wc.sample(dw)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"{k}: {int((got != want).sum())} of {got.numel()} sampled elements differ from the parent's"
    assert wc.digest(dw) == bytes(g[k + "/sha256"]).hex(), f"{k}: the sample agrees, the whole dW does not"


@gpu
@pytest.mark.parametrize("shape", wc.SHAPES, ids=IDS)
def test_wgrad64_vs_fp64(shape):
    x, dy, dw = _wgrad(shape)
    w64 = torch.zeros(64, 64, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().cpu(), w64, None, 2, 1).backward(dy.double().cpu())
    stock = torch.ops.aten.convolution_backward(dy, x, torch.zeros(64, 64, 3, 3, device="cuda"), None, [2, 2], [1, 1], [1, 1], False,
                                                [0, 0], 1, [False, True, False])[1]
    e_native, e_stock = rel_err(dw, w64.grad), rel_err(stock, w64.grad)
    print(f"wgrad64 {shape}: native {e_native:.3e}  stock {e_stock:.3e}")
    assert e_native <= TOL, f"{e_native:.3e} > {TOL}"
    assert e_native <= 2.0 * e_stock, f"native {e_native:.3e} > 2 x stock {e_stock:.3e}"


def _inside(t, pad, fill):
    """A contiguous copy of t in the middle of a larger allocation filled with `fill` -> (view, whole buffer)."""
    buf = torch.full((t.numel() + 2 * pad,), fill, device="cuda")
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


@gpu
@pytest.mark.parametrize("shape", wc.SHAPES, ids=IDS)
def test_wgrad64_neighbours(shape):
    x, dy, dw = _wgrad(shape)
    xv, _ = _inside(x, PAD, float("nan"))
    gv, _ = _inside(dy, PAD, float("nan"))
    dv, dbuf = _inside(torch.full_like(dw, float("nan")), PAD, SENTINEL)
    wc.run_wgrad(wc.load_library(), gv, xv, dv)
    torch.cuda.synchronize()
    assert torch.equal(dv, dw)
    assert bool((dbuf[:PAD] == SENTINEL).all()) and bool((dbuf[-PAD:] == SENTINEL).all()), "dw: written outside the tensor"


@gpu
@pytest.mark.parametrize("shape", wc.SHAPES, ids=IDS)
def test_wgrad64_captured_matches_eager(shape):
    x, dy, dw = _wgrad(shape)  # the workspace exists before the capture
    out = torch.empty_like(dw)
    lib = wc.load_library()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        wc.run_wgrad(lib, dy, x, out)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, dw)


# (B, H, W) of x: a plane the 64 -> 64 rule routes (256 workgroups of 4 rows: both thresholds) and one it leaves to the stock
# operator (6 workgroups)
ROUTED, UNROUTED = (32, 64, 64), (2, 24, 21)


@gpu
def test_backward_routes_by_the_rule(monkeypatch):
    """_Conv3x3S2.backward calls cabinet_conv3x3s2_wgrad for dw at a routed shape and the stock operator at an unrouted one; the two
    routes' gradients agree."""
    from cabinet_amd import _lib
    from cabinet_amd import functional as Fh

    assert Fh._conv3x3s2_native_wgrad64(*ROUTED) and not Fh._conv3x3s2_native_wgrad64(*UNROUTED)
    assert Fh._conv3x3s2_native_wgrad64(8, 512, 512) == Fh._conv3x3s2_native_wgrad64(8, 256, 256)  # decided per configuration
    assert Fh._conv3x3s2_native_wgrad64(2, 1024, 512) == Fh._conv3x3s2_native_wgrad64(2, 512, 256)
    lib = _lib.load()
    calls = {"native": 0, "stock": 0}
    native, stock = lib.cabinet_conv3x3s2_wgrad, torch.ops.aten.convolution_backward

    def count_native(*a):
        calls["native"] += 1
        return native(*a)

    def count_stock(*a):
        calls["stock"] += bool(a[-1][1])  # the weight-gradient mask
        return stock(*a)

    for shape, want in ((ROUTED, {"native": 1, "stock": 0}), (UNROUTED, {"native": 0, "stock": 1})):
        B, H, W = shape
        g0 = torch.Generator().manual_seed(B * 1009 + H)
        x = torch.randn(B, 64, H, W, generator=g0).cuda().requires_grad_(True)
        w = (torch.randn(64, 64, 3, 3, generator=g0) * 0.05).cuda().requires_grad_(True)
        g = torch.randn(B, 64, *wc.out_hw(H, W), generator=g0).cuda()
        calls.update(native=0, stock=0)
        with monkeypatch.context() as m:
            m.setattr(lib, "cabinet_conv3x3s2_wgrad", count_native)
            m.setattr(torch.ops.aten, "convolution_backward", count_stock)
            Fh._Conv3x3S2.apply(x, w).backward(g)
        assert calls == want, (shape, calls)
        ref = stock(g, x.detach(), w.detach(), None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [True, True, False])
        e_dx, e_dw = rel_err(x.grad, ref[0]), rel_err(w.grad, ref[1])
        print(f"{shape}: dx {e_dx:.3e}  dw {e_dw:.3e}")
        assert e_dx <= TOL and e_dw <= TOL
