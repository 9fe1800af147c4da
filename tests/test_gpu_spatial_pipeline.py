"""The pipelined staging of the stem forward (K9, cabinet_stem_conv_fwd) and of the 3x3 stride-2 input gradient (K15,
cabinet_conv3x3s2_dgrad): prefetched, clamped, zero-selected row-segment loads; the patch of the stem's next tile in registers
under the MFMAs; the three-slot dy row ring of the input gradient.  The arithmetic of both kernels is frozen, so per shape
(tests/spatial_pipeline_cases.py: every plan branch and every edge of the new staging):

  bits       the output is bit for bit what the commit before the change computed (tests/golden/g9_spatial_pipeline.npz, written
             by tests/golden/make_golden_spatial_pipeline.py on that commit's library: SHA-256 of the output and a strided sample)
  accuracy   against fp64 F.conv2d / its input gradient under the bounds of test_gpu_stem.py (1e-3) and test_gpu_conv3x3s2.py
             (1e-3 and no worse than twice the stock operator's own distance)
  neighbours operands inside NaN-filled allocations, the output inside a sentinel-filled one: the same bits, sentinel intact (a
             clamped load that leaks into a sum, a mask applied by multiplication, a store past the tensor)
  captured   two replays of one captured graph give the eager call's bits
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatial_pipeline_cases as sp
from conftest import GOLDEN, assert_close, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3  # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32
PAD = 1031  # elements of NaN / sentinel on either side of a tensor (odd: the tensors sit at 4-byte, not 16-byte, alignment ...)
PAD_DX = 1030  # ... except dx, which the entry point wants 8-byte aligned
SENTINEL = -12345.5


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(os.path.join(GOLDEN, "g9_spatial_pipeline.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _stem(shape):
    """-> x, w on the device and the plain result (computed once, shared, never written again)."""
    x, w = sp.stem_inputs(*shape)
    x, w = x.cuda(), w.cuda()
    y = sp.run_stem(sp.load_library(), x, w, torch.full(sp.stem_out(*shape), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    return x, w, y


@functools.lru_cache(maxsize=None)
def _dgrad(shape):
    dy, w = sp.dgrad_inputs(*shape)
    dy, w = dy.cuda(), w.cuda()
    dx = sp.run_dgrad(sp.load_library(), dy, w, torch.full((shape[0], 64, shape[1], shape[2]), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    return dy, w, dx


def _assert_bits(kind, shape, out):
    assert bool(torch.isfinite(out).all()), "an element was not written, or is not finite"
    g = _golden()
    k = sp.key(kind, shape)
    want = torch.from_numpy(g[k + "/sample"])
    got = sp.sample(out)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"{k}: {int((got != want).sum())} of {got.numel()} sampled elements differ from the parent's"
    assert sp.digest(out) == bytes(g[k + "/sha256"]).hex(), f"{k}: the sample agrees, the whole output does not"


def test_plans_cover_every_branch():
    tiles = {sp.stem_plan(*s)[1] for s in sp.STEM}
    assert {1, 2, 3} <= tiles and max(tiles) >= 6
    assert any(sp.stem_plan(*s)[0] >= 512 for s in sp.STEM)
    rows = {sp.dgrad_plan(*s)[2] for s in sp.DGRAD}
    assert {1, 2, 4} <= rows
    assert any(sp.dgrad_plan(*s)[2] >= 4 and ((s[1] - 1) // 2 + 1) % sp.dgrad_plan(*s)[2] == 1 for s in sp.DGRAD)  # a one-row last strip


@pytest.mark.parametrize("shape", sp.STEM, ids=lambda s: "x".join(map(str, s)))
def test_stem_fwd_bits_match_parent(shape):
    _assert_bits("stem", shape, _stem(shape)[2])


@pytest.mark.parametrize("shape", sp.DGRAD, ids=lambda s: "x".join(map(str, s)))
def test_dgrad_bits_match_parent(shape):
    _assert_bits("dgrad", shape, _dgrad(shape)[2])


@pytest.mark.parametrize("shape", sp.STEM, ids=lambda s: "x".join(map(str, s)))
def test_stem_fwd_vs_fp64(shape):
    x, w, y = _stem(shape)
    ref = F.conv2d(x.double().cpu(), w.double().cpu(), None, 2, 3)
    e = rel_err(y, ref)
    print(f"stem fwd {shape}: {e:.3e}")
    assert_close(y, ref, TOL, "y")


@pytest.mark.parametrize("shape", sp.DGRAD, ids=lambda s: "x".join(map(str, s)))
def test_dgrad_vs_fp64(shape):
    dy, w, dx = _dgrad(shape)
    B, H, W = shape
    ref = torch.ops.aten.convolution_backward(dy.double().cpu(), torch.zeros(B, 64, H, W, dtype=torch.float64), w.double().cpu(), None,
                                              [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])[0]
    stock = torch.ops.aten.convolution_backward(dy, torch.zeros(B, 64, H, W, device="cuda"), w, None, [2, 2], [1, 1], [1, 1], False,
                                                [0, 0], 1, [True, False, False])[0]
    e_native, e_stock = rel_err(dx, ref), rel_err(stock, ref)
    print(f"dgrad {shape}: native {e_native:.3e}  stock {e_stock:.3e}")
    assert e_native <= TOL, f"{e_native:.3e} > {TOL}"
    assert e_native <= 2.0 * e_stock, f"native {e_native:.3e} > 2 x stock {e_stock:.3e}"


def _inside(t, pad, fill):
    """A contiguous copy of t in the middle of a larger allocation filled with `fill` -> (view, whole buffer)."""
    buf = torch.full((t.numel() + 2 * pad,), fill, device="cuda")
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _assert_intact(buf, pad, what):
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all()), f"{what}: written outside the tensor"


@pytest.mark.parametrize("shape", sp.STEM, ids=lambda s: "x".join(map(str, s)))
def test_stem_fwd_neighbours(shape):
    x, w, y = _stem(shape)
    xv, _ = _inside(x, PAD, float("nan"))
    wv, _ = _inside(w, PAD, float("nan"))
    yv, ybuf = _inside(torch.full_like(y, float("nan")), PAD, SENTINEL)
    sp.run_stem(sp.load_library(), xv, wv, yv)
    torch.cuda.synchronize()
    assert torch.equal(yv, y)
    _assert_intact(ybuf, PAD, "y")


@pytest.mark.parametrize("shape", sp.DGRAD, ids=lambda s: "x".join(map(str, s)))
def test_dgrad_neighbours(shape):
    dy, w, dx = _dgrad(shape)
    gv, _ = _inside(dy, PAD, float("nan"))
    wv, _ = _inside(w, PAD, float("nan"))
    dv, dbuf = _inside(torch.full_like(dx, float("nan")), PAD_DX, SENTINEL)
    sp.run_dgrad(sp.load_library(), gv, wv, dv)
    torch.cuda.synchronize()
    assert torch.equal(dv, dx)
    _assert_intact(dbuf, PAD_DX, "dx")


def _captured(run, out):
    """Two replays of one captured graph of `run`, the output cleared in between -> the two results."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run()
    got = []
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got.append(out.clone())
    return got


def test_stem_fwd_captured_matches_eager():
    shape = (1, 17, 449)
    x, w, y = _stem(shape)
    out = torch.empty_like(y)
    lib = sp.load_library()
    for r in _captured(lambda: sp.run_stem(lib, x, w, out), out):
        assert torch.equal(r, y)


def test_dgrad_captured_matches_eager():
    shape = (3, 1025, 6)
    dy, w, dx = _dgrad(shape)
    out = torch.empty_like(dx)
    lib = sp.load_library()
    for r in _captured(lambda: sp.run_dgrad(lib, dy, w, out), out):
        assert torch.equal(r, dx)
