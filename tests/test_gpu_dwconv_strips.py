"""Strip-walking depthwise kernels (K8, csrc/dwconv.hip): a workgroup walks a run of 1024-pixel blocks of one column strip,
prefetching block i+1 while it computes block i, carrying the K-1 halo rows in LDS, and reduces its weight-gradient sums once.
The arithmetic of every output ELEMENT and the grouping of the BatchNorm sums are what the one-tile kernels did; only the grouping
of the weight-gradient sums moved.

Cases: tests/dwconv_strips_cases.py (each row names the branch of the plan it reaches; `test_table_reaches_its_branches` holds the
table to that).  Per case:
  * bits: y and dx (plain form), y and the eval-mode dz (fused form: dz does not depend on the batch sums there, coef = 0 in
    bn_act_bwd_finalize) equal what the commit in front of the rewrite computed, recorded by tests/golden/
    make_golden_dwconv_strips.py on that commit as SHA-256 digests of the bytes (all shapes) and in full (small shapes);
  * fp64 oracle, the calls of test_gpu_dwconv.py: every output within 1e-3, running statistics within 1e-5; the regrouped sums
    (dw, dbn_weight, dbn_bias, training-mode dz) no further from fp64 than 2 x that commit's own recorded distance
    (`test_regrouped_sums_within_twice_the_one_tile_kernels`, all cases in one verdict);
  * two runs bit-equal; every buffer the wrappers allocate -- outputs and workspaces -- starts as NaN / 0xFF bytes, so an output
    element that is not written, or a partial beyond the new count that is read, shows up as a non-finite value;
  * one hipGraph capture, two replays: equal to the eager result.
"""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import dwconv_strips_cases as dc
from conftest import GOLDEN, rel_err

gpu = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "g8_dwconv_strips.json")) as f:
        rec = json.load(f)
    return rec, np.load(os.path.join(GOLDEN, "g8_dwconv_strips.npz"))


@contextlib.contextmanager
def _poisoned_buffers():
    """torch.empty / empty_like of the wrappers give NaN (floating point) or 0xFF bytes (workspaces: NaN when read as fp32)."""
    real_empty, real_like = torch.empty, torch.empty_like

    def _fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(255) if t.dtype == torch.uint8 else t

    torch.empty = lambda *a, **k: _fill(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: _fill(real_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def _ids(case):
    return dc.key(*case).replace("/", "-")


def test_table_reaches_its_branches():
    """The rows of dwconv_strips_cases.SHAPES are what their comments say, by the plan restated in strip_plan."""
    plans = {sh: dc.strip_plan(sh[0] * sh[1], sh[2], sh[3]) for sh in dc.SHAPES}
    p = plans[(2, 3, 70, 130)]
    assert (p["strips"], p["runs"], p["nb"], p["last"]) == (3, 2, 3, 2) and 130 % 4 == 2 and 130 - 2 * p["TW"] == 2
    p = plans[(1, 2, 41, 67)]
    assert (p["runs"], p["nb"]) == (1, 3) and 41 % 2 == 1 and 67 % 2 == 1
    p = plans[(2, 2, 5, 200)]
    assert (p["strips"], p["blocks"]) == (4, 1) and 200 % 4 == 0 and 5 < p["TH"]
    p = plans[(1, 2, 200, 5)]
    assert (p["TW"], p["TH"], p["nb"]) == (8, 128, 2) and p["TH"] * 4 > 256 >= p["TH"] * 2   # K = 5 fills the second halo slot
    assert plans[(1, 5, 1, 1)]["blocks"] == 1
    p = plans[(1, 4, 128, 128)]
    assert (p["strips"], p["runs"], p["nb"]) == (2, 2, 4) and 128 % 4 == 0
    p = plans[(1, 2, 330, 36)]
    assert (p["blocks"], p["nb"], p["runs"], p["last"]) == (21, 4, 6, 1) and 36 % 4 == 0 and 36 < p["TW"]
    p = plans[(1, 2, 2, 9)]
    assert p["TW"] == 16 and 2 < 3
    p = plans[(1, 3, 100, 24)]
    assert (p["TW"], p["TH"], p["nb"], p["runs"]) == (32, 32, 4, 1) and 100 - 3 * 32 == 4
    p = plans[(2, 1, 3, 8300)]
    assert 2 * p["strips"] * p["runs"] == 260 > 256
    for sh, p in plans.items():  # a run is never shorter than one tile: the partials are a prefix of the per-tile workspace
        assert p["strips"] * p["runs"] <= p["strips"] * p["blocks"] and p["nb"] >= 1
    # the stride-2 forward keeps its one-tile kernel; the stride-1 forward plans on the output plane, which has the input's size


def _same_bits(rec, full, k, name, t):
    assert bool(torch.isfinite(t).all()), f"{k} {name}: non-finite values (an element not written, or a stale partial read)"
    if f"{k}/{name}" in full.files:
        want = torch.from_numpy(full[f"{k}/{name}"])
        assert torch.equal(t.cpu(), want), f"{k} {name}: {int((t.cpu() != want).sum())} elements differ from the recorded tensor"
    assert dc.digest(t) == rec[k][name], f"{k} {name}: bits differ from what the one-tile kernels computed"


_DIST = {}   # case key -> {tensor: distance from fp64}, filled by the per-case tests, read by the test of the 2 x bound


def _distance(k, name, got, ref):
    _DIST.setdefault(k, {})[name] = rel_err(got, ref)


@gpu
@pytest.mark.parametrize("case", dc.plain_cases(), ids=_ids)
def test_plain_strips(case, golden):
    from test_gpu_backbone_edges import _dw_dev

    rec, full = golden
    shape, K, S = case
    k = dc.key(shape, K, S)
    x, w, g, (yo, dxo, dwo) = dc.plain_case(shape, K, S)
    runs = []
    for _ in range(2):
        with _poisoned_buffers():
            runs.append(_dw_dev(x, w, g, S))
        torch.cuda.synchronize()
    y, dx, dw = runs[0]
    for a, b, name in zip(runs[0], runs[1], ("y", "dx", "dw")):
        assert torch.equal(a, b), f"{k} {name}: two runs differ"
    _same_bits(rec, full, k, "y", y)
    _same_bits(rec, full, k, "dx", dx)
    assert bool(torch.isfinite(dw).all()), f"{k} dw: non-finite"
    for name, got, ref in (("y", y, yo), ("dx", dx, dxo), ("dw", dw, dwo)):
        e = rel_err(got, ref)
        assert got.shape == ref.shape and e <= TOL, f"{k} {name}: rel {e:.2e}"
    _distance(k, "dw", dw, dwo)


@gpu
@pytest.mark.parametrize("case", dc.fused_cases(), ids=_ids)
def test_fused_strips(case, golden):
    rec, full = golden
    shape, K, S, act, training = case
    k = dc.key(*case)
    ref, run = dc.fused_case(*case)
    runs = []
    for _ in range(2):
        with _poisoned_buffers():
            runs.append(run())
        torch.cuda.synchronize()
    out = runs[0]
    for name in out:
        assert bool(torch.isfinite(out[name]).all()), f"{k} {name}: non-finite"
        assert torch.equal(out[name], runs[1][name]), f"{k} {name}: two runs differ"
    _same_bits(rec, full, k, "y", out["y"])
    if not training:
        _same_bits(rec, full, k, "dz", out["dz"])
    for name in ref:
        e = rel_err(out[name], ref[name])
        assert e <= (1e-5 if name.startswith("running") else TOL), f"{k} {name}: rel {e:.2e}"
    for name in rec[k]["err"]:
        _distance(k, name, out[name], ref[name])


@gpu
def test_regrouped_sums_within_twice_the_one_tile_kernels(golden):
    """dw, dbn_weight, dbn_bias and the training-mode dz of EVERY case above: no further from the fp64 oracle than 2 x the distance
    the one-tile kernels had on the same inputs (recorded with the bits).  Every figure is printed; all misses are reported at once.
    Cases the per-case tests of this session did not run are run here.


    The strip kernels keep the one-tile kernels' grouping of the two BatchNorm sums (one partial per 1024-pixel block, the same
    per-thread chains and tree), so dbn_weight, dbn_bias and the training-mode dz are the one-tile kernels' numbers; only dw is
    grouped per workgroup.  A first version summed the BatchNorm terms per workgroup (in fp32, then in double): 19 of the 568 sums,
    all dbn_weight / dbn_bias of 1 to 4 numbers at 6e-8 ... 6e-7 from fp64, were then past twice the one-tile kernels' distance,
    which for so few numbers is at or below one fp32 rounding."""
    from test_gpu_backbone_edges import _dw_dev

    rec, _ = golden
    for case in dc.plain_cases():
        k = dc.key(*case)
        if k not in _DIST:
            x, w, g, (_, _, dwo) = dc.plain_case(*case)
            _distance(k, "dw", _dw_dev(x, w, g, case[2])[2], dwo)
    for case in dc.fused_cases():
        k = dc.key(*case)
        if k not in _DIST:
            ref, run = dc.fused_case(*case)
            out = run()
            for name in rec[k]["err"]:
                _distance(k, name, out[name], ref[name])
    misses, n = [], 0
    for k in sorted(_DIST):
        for name, e in _DIST[k].items():
            e0, n = rec[k]["err"][name], n + 1
            print(f"{k} {name}: distance from fp64 {e:.3e}, one-tile kernels {e0:.3e}")
            if not e <= 2.0 * e0:
                misses.append(f"{k} {name}: {e:.3e} from fp64, one-tile kernels {e0:.3e}")
    assert n == sum(len(rec[dc.key(*c)]["err"]) for c in dc.plain_cases() + dc.fused_cases())
    assert not misses, f"{len(misses)} of {n} sums further from fp64 than twice the one-tile kernels:\n" + "\n".join(misses)


GRAPH_SHAPES = [(2, 3, 70, 130), (1, 4, 128, 128)]   # ragged and 16-byte form, several runs and strips each


@gpu
@pytest.mark.parametrize("K,S", dc.KS)
@pytest.mark.parametrize("shape", GRAPH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_capture_and_replay(shape, K, S):
    """Plain and fused (hardswish, eval: the running buffers do not move between replays) forward + backward in one hipGraph,
    captured the way GraphedTrainStep captures the model's step and tests/test_gpu_bn_prologue.py its operators: after an eager
    step, in the thread-local capture mode (autograd's worker thread enqueues the backward; under the global mode its event
    calls are errors while a capture is open)."""
    from cabinet_amd.functional import bn_act_dwconv, dwconv
    from test_gpu_backbone_edges import _set_bn

    B, C, H, W = shape
    gen = torch.Generator().manual_seed(dc.seed(shape, K, S) + 1)
    conv0 = torch.nn.Conv2d(C, C, K, S, K // 2, groups=C, bias=False)
    conv1 = torch.nn.Conv2d(C, C, K, S, K // 2, groups=C, bias=False)
    with torch.no_grad():
        conv0.weight.copy_(torch.randn(C, 1, K, K, generator=gen))
        conv1.weight.copy_(torch.randn(C, 1, K, K, generator=gen))
    bn = _set_bn(torch.nn.BatchNorm2d(C), gen).cuda().eval()
    conv0, conv1 = conv0.cuda(), conv1.cuda()
    x0 = (torch.randn(B, C, H, W, generator=gen) * 1.5 + 0.3).cuda().requires_grad_(True)
    x1 = (torch.randn(B, C, H, W, generator=gen) * 1.5 + 0.3).cuda().requires_grad_(True)
    Ho, Wo = (H - 1) // S + 1, (W - 1) // S + 1
    g = torch.randn(B, C, Ho, Wo, generator=gen).cuda()
    params = [x0, conv0.weight, x1, bn.weight, bn.bias, conv1.weight]

    def step():
        for p in params:
            p.grad = None
        y0 = dwconv(x0, conv0)
        y0.backward(g)
        y1 = bn_act_dwconv(x1, bn, "hardswish", conv1)
        y1.backward(g)
        return [y0.detach(), y1.detach()] + [p.grad for p in params]

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = step()
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(outs, eager)):
            assert torch.equal(a, b), f"replay {rep}: output {i} differs from the eager result"
