"""K10 (csrc/pwconv.hip) after its kernels were pipelined: the forward and the input gradient are bit for bit what the commit
before computed (tests/golden/g10_pwconv_pipeline.npz, written by make_golden_pwconv_pipeline.py on that commit's library); the
weight gradient, whose sums are grouped differently now, is deterministic, within the project's bound of the fp64 product and
no further from it than twice what that commit was.  Everything goes through the C ABI (tests/pwconv_pipeline_cases.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pwconv_pipeline_cases as pc  # noqa: E402

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_pwconv_pipeline.npz")
TOL = 1e-3            # the project's bound on the relative distance from fp64
ROUNDING = 2.0 ** -23  # one fp32 rounding: the floor of the comparison with the parent's distance


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _ids(case):
    return pc.key(case)


def test_plan_reaches_every_branch():
    """The cases, against the launch plan restated in pwconv_pipeline_cases.stream_plan: every vector width, walks of 1, 2 and 3
    blocks per wave at the full grid, every residue of P the issue names, both batch sizes, one misaligned case.  Pure Python
    (no device work), so it also runs in the CPU tier.  A walk of 0 blocks cannot be launched: the grid is min(blocks, cap)."""
    plans = [pc.stream_plan(B, Co, Ci, P, not mis) for B, Ci, Co, P, mis in pc.CASES]
    plans += [pc.stream_plan(B, Ci, Co, P, not mis) for B, Ci, Co, P, mis in pc.CASES]
    assert {p[0] for p in plans} == {0, 1, 2, 4}  # 0: the products that keep the plain walk
    for v in (1, 2, 4):
        walks = {p[4] for p in plans if p[0] == v and p[3] == pc.GRID_CAP}
        assert 3 in walks, (v, walks)  # 4203 blocks on 2048 waves: 107 waves walk 3 blocks, the others 2
        assert 1 in {p[4] for p in plans if p[0] == v}
    assert {c[3] % 64 for c in pc.CASES} >= {0, 1, 37, 63} and {c[3] % 4 for c in pc.CASES} == {0, 1, 2, 3}
    assert {c[0] for c in pc.CASES} == {1, 3} and any(c[4] for c in pc.CASES)
    assert {(c[1], c[2]) for c in pc.CASES} >= {(16, 16), (16, 64), (64, 24), (24, 72), (72, 24), (8, 8), (104, 56)}
    assert any(pc.stream_plan(c[0], c[2], c[1], c[3], False)[0] == 1 for c in pc.CASES if c[4])


@gpu
@pytest.mark.parametrize("case", pc.CASES, ids=_ids)
def test_pwconv_pipeline(case):
    """y and dx: the parent's SHA-256 and its strided sample.  dW: two calls equal; within 1e-3 of the fp64 product; at most
    twice the parent's distance from it (floor: one fp32 rounding)."""
    B, Ci, Co, P, mis = case
    gold, k = _golden(), pc.key(case)
    x, w, g = pc.inputs(B, Ci, Co, P)
    xd, wd, gd = pc.on_device(x, mis), pc.on_device(w, False), pc.on_device(g, mis)
    y, dx, dw = pc.run(pc.load_library(), xd, wd, gd, mis)
    y2, dx2, dw2 = pc.run(pc.load_library(), xd, wd, gd, mis)
    torch.cuda.synchronize()
    for name, t, t2 in (("y", y, y2), ("dx", dx, dx2)):
        assert bool(torch.isfinite(t).all()), name
        assert torch.equal(pc.sample(t), torch.from_numpy(gold[f"{k}/{name}/sample"])), f"{name}: the strided sample differs"
        assert pc.digest(t) == bytes(gold[f"{k}/{name}/sha256"]).hex(), f"{name}: not bit for bit the parent's"
        assert torch.equal(t, t2), name
    assert bool(torch.isfinite(dw).all()) and torch.equal(dw, dw2), "dW is not deterministic"
    d, d0 = pc.dist(dw, pc.dw_ref(x, g)), float(gold[f"{k}/dw/dist"])
    print(f"pwconv pipeline {k}: dW distance from fp64 {d:.3e}, parent {d0:.3e}")
    assert d <= TOL, f"dW: {d:.3e} > {TOL}"
    assert d <= 2.0 * max(d0, ROUNDING), f"dW: {d:.3e} from fp64, the parent was {d0:.3e}"


@gpu
def test_pwconv_pipeline_captured():
    """Forward + backward captured in a graph and replayed twice: bit for bit the eager result."""
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    B, Ci, Co, P = 3, 24, 72, 64 * 9 + 38
    lib = pc.load_library()
    x, w, g = pc.inputs(B, Ci, Co, P)
    xd, wd, gd = x.cuda(), w.cuda(), g.cuda()
    eager = pc.run(lib, xd, wd, gd)
    torch.cuda.synchronize()
    nan = float("nan")
    y, dx, dw = torch.full_like(gd, nan), torch.full_like(xd, nan), torch.full_like(wd, nan)
    ws, nbytes = _workspace(lib.cabinet_pwconv_bwd_workspace_bytes(B, Ci, Co, P), xd.device)

    def step():
        st = _stream_handle(xd.device)
        assert lib.cabinet_pwconv_fwd(_ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(y), st) == 0
        assert lib.cabinet_pwconv_bwd(_ptr(gd), _ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes, st) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for t in (y, dx, dw):
            t.fill_(nan)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("y", "dx", "dw"), (y, dx, dw), eager):
            assert torch.equal(a, b), f"{name}: the replay differs from the eager call"
