"""The three kernel families without autograd -- K13 csrc/eval_tail.hip (evaluation), K17 csrc/predict_tail.hip (inference), K16
csrc/opt_tail.hip (optimizer) -- where their host-side launch plans branch and where their rows, segments and chunks end: every
case through the public wrappers of cabinet_amd.functional or cabinet_amd.optim.FusedSGDTail, against float64 on the CPU
(tests/tail_cases.py) or, for K16, against the class's own composite host path.

1. `test_tail_plan_cases_reach_their_branches` (no kernel launched): eval_span / eval_chip_threads, predict_span /
   predict_up_threads, the (VEC, CFIX) choice and the 512-workgroup cap of eval_argmax_hist_run, the grids of eval_scale_merge_run
   and predict_argmax_run and build_chunks with the grid rule of sgd_tail_run restated, cross-checked against
   cabinet_eval_chip_accum_supported / cabinet_predict_up_argmax_supported over a few thousand (C, wl, W) triples around the
   boundaries, against cabinet_sgd_tail_workspace_bytes and against the constants as the sources spell them; then every row of
   the tables asserted to reach the branch it is listed for.
2. K13: every row of CHIP_CASES (T = 256, 128, 64 for CMAX = 0, 19, 8, one and two sources, the 64 KB boundary) at four corner
   origins and an interior one: bytes outside the window bit-equal, a second run bit-equal, ||got - ref|| <= 1e-4 ||ref|| and
   element by element |got - ref| <= max(4 E32, 2e-6), E32 the distance of the fp32 composite on the CPU from float64 on the
   same inputs; refused rows raise before any launch; a dense sweep of 540 shapes.  eval_scale_merge with more than one workgroup
   in x, vector and scalar, element by element max(4 E32, 5e-7 max(1, |ref|)); eval_argmax_hist at every (VEC, CFIX) pair and at
   every pixel count 1..40, exact.
3. K17: predict_up_argmax on rows of two to five segments (ox_lo > 0, a_lo > 0, ragged last segments), T = 128 and 64, packed and
   byte stores, under the decision rule of test_up_argmax_vs_float64 with the seed searched on the float64 reference alone;
   guard bands one byte into a 0xA5-filled buffer; planted ties; predict_argmax's byte-wise form over three workgroups;
   predict_render over four-pixel groups that straddle images.
4. K16: momentum 0, no EMA, no clipping, no warm-up, past max_iter, no weight decay, a non-finite norm with and without the
   skip, NaN-poisoned momentum buffers (a first step overwrites its buffer and never reads it), each of the four pointers of
   ptr_aligned16 misaligned, a size sweep aligned and misaligned, and 2051 chunks on the kernels' own cap of 2048 workgroups.
5. Caller contract: channels_last, offset and half-precision inputs give the dense call's bits; a misaligned `total` raises.

NaN ordering is out of scope: torch.argmax treats NaN as the maximum, the kernels' `>` does not; no input here holds a NaN.

Measured on an MI355X, largest elementwise distance from float64 as (E32, kernel) on the same inputs:
  eval_chip_accum   table rows (1.780e-5, 1.780e-5) at 512 -> 130 with T = 64, the other rows (1.5e-7 .. 4.5e-7, kernel and E32 the
                    same to three digits; 1.473e-7 against 1.564e-7 at T = 128, C = 8); sweep (2.296e-5, 2.290e-5) at 220 -> 513
  eval_scale_merge  table rows (2.328e-5, 2.328e-5) at 300 -> 1030; sweep (3.011e-5, 3.011e-5) at 772 -> 1027
The kernels form their source indices in fp32 by the formula torch's CPU resize uses, so kernel / E32 is 1.0 wherever that index error
dominates and at most 1.2 elsewhere (8.9e-8 against 7.5e-8 on one pixel); nothing exceeds a bound, and no seam or last
column stands out at T = 128 or T = 64.

One defect was found, in K16: a gradient 4 bytes into its storage changed the bits of every result.  sgd_tail_norm summed the
squares of such a chunk in another order than those of an aligned one, so the norm, the clip coefficient and with them every
parameter differed in their last bits (test_tail_each_pointer_of_an_entry_misaligned, forms `grad` and `all`).  The scalar
form now reads the elements of each float4 with four dword loads and adds them in the float4 form's order.
"""
import numpy as np
import pytest
import torch

import tail_cases as T
from conftest import assert_close
from eval_golden import MAX_UNDECIDED_SHARE
from predict_golden import render_contract
from test_gpu_backbone_edges import _all_equal, _cmp, _report

gpu = pytest.mark.gpu
GUARD = 0xA5
_DIST = {}   # tag -> (E32, kernel distance), printed by the tests that fill it


# ------------------------------------------------------------------------------------------------ 1. the plan tables
def _boundary_triples():
    """(C, wl, W) around the LDS boundaries of both kernels: a few thousand triples."""
    out = []
    for C in (1, 5, 8, 19, 31, 32):
        for W in (64, 100, 128, 130, 256, 257, 512, 513, 862, 863, 1000, 1024, 1025, 2048):
            ws = {W, W + 1, 2 * W, 2 * W + 3, 3 * W, 4 * W, 4 * W - 1, 4 * W + 2, 5 * W, 8 * W, 8 * W + 1, 16 * W, 20 * W,
                  max(W // 2, 1), max(W // 8, 1), 16384 // C, 16384 // C + 1, 8192 // C, 8192 // C + 1, 32768 // C}
            out += [(C, wl, W) for wl in sorted(ws)]
    return out


def test_tail_plan_cases_reach_their_branches():
    """Every row of the tables of tail_cases.py reaches the branch it is there for: the restated host rules against the
    library's queries and the sources' constants, then the tables against the restated rules."""
    from cabinet_amd import _lib
    from cabinet_amd import optim

    lib = _lib.load()
    assert T.source_constants() == T.RESTATED
    assert optim.CHUNK == T.TAIL_CHUNK
    tables = (T.CHIP_CASES, T.CHIP_REFUSED, T.MERGE_CASES, T.HIST_CASES, T.UP_CASES, T.UP_REFUSED, T.UP_TIES, T.ARGMAX_CASES)
    assert [len(t) for t in tables] == [8, 2, 6, 6, 12, 2, 2, 2]     # no row may leave unnoticed
    triples = _boundary_triples()
    assert len(triples) > 1500
    seen = {"chip1": set(), "chip2": set(), "up": set()}
    for C, wl, W in triples:
        for flip in (0, 1):
            t = T.eval_chip_threads(C, wl, W, 1 + flip)
            assert lib.cabinet_eval_chip_accum_supported(C, 2, wl, 3, W, flip) == int(t > 0), (C, wl, W, flip)
            assert T.eval_chip_supported(C, 2, wl, 3, W, flip) == (t > 0)
            seen["chip2" if flip else "chip1"].add(t)
        t = T.predict_up_threads(C, wl, W)
        assert lib.cabinet_predict_up_argmax_supported(C, 2, wl, 3, W) == int(t > 0) == int(T.predict_up_supported(C, 2, wl, 3, W))
        seen["up"].add(t)
    assert all(s == {0, 64, 128, 256} for s in seen.values()), seen
    for args in ((33, 2, 8, 3, 8), (0, 2, 8, 3, 8), (8, 2, 8, 65536, 8)):
        assert lib.cabinet_eval_chip_accum_supported(*args, 0) == 0 and not T.eval_chip_supported(*args, False)
        assert lib.cabinet_predict_up_argmax_supported(*args) == 0 and not T.predict_up_supported(*args)

    # K13 eval_chip_accum
    for name, (C, low, chip, flip, want, N) in T.CHIP_CASES.items():
        assert lib.cabinet_eval_chip_accum_supported(C, *low, *chip, int(flip)) == 1, name
        assert T.eval_chip_plan(C, low, chip, flip)[:3] == want, (name, T.eval_chip_plan(C, low, chip, flip))
    plan = {n: T.eval_chip_plan(*c[:4]) for n, c in T.CHIP_CASES.items()}
    assert {(p[0], p[3]) for p in plan.values()} == {(256, 0), (128, 0), (64, 0), (128, 19), (64, 19), (128, 8)}
    assert 2 * 32 * 256 * 4 == T.EVAL_LDS_MAX and plan["lds-at-64KB"][2] == 256 == plan["lds-at-64KB-T64"][2]
    assert 2 * 32 * T.eval_span(256, 257, 257) * 4 == 65792 > T.EVAL_LDS_MAX        # one column over the limit
    assert T.eval_chip_plan(32, (2, 260), (3, 260), True)[0] == 128                 # the same width with two sources
    assert sorted(c[5] for c in T.CHIP_CASES.values()).count(3) == 2
    assert all(p[1] >= 2 for n, p in plan.items() if n != "lds-at-64KB")            # more than one row segment
    for name, (case, neighbour) in T.CHIP_REFUSED.items():
        assert lib.cabinet_eval_chip_accum_supported(case[0], *case[1], *case[2], int(case[3])) == 0, name
        assert T.eval_chip_plan(*case)[0] == 0 and neighbour in T.CHIP_CASES, name
    for C in T.CHIP_SWEEP_C:
        for hh in T.CHIP_SWEEP_HH:
            shapes = T.chip_sweep_shapes(C, hh)
            assert len(shapes) == 90 and all(T.eval_chip_plan(*s)[0] == 256 for s in shapes)
            assert {T.eval_chip_plan(*s)[1] for s in shapes} == {1, 2, 3}

    # K13 eval_scale_merge, eval_argmax_hist
    for name, (C, src, crop, out, want) in T.MERGE_CASES.items():
        assert T.scale_merge_plan(out[1]) == want, name
    assert T.scale_merge_plan(1024) == (4, 1) and T.scale_merge_plan(256) == (4, 1) and T.scale_merge_plan(257) == (1, 2)
    assert {T.scale_merge_plan(W) for W in T.MERGE_W} == {(1, 1), (4, 1), (1, 2), (1, 4), (1, 5), (4, 2)}
    assert T.MERGE_MAX_PLANES[0] == 65535 and len(T.merge_sweep_shapes()) == 66
    assert all(c[2] % 2 == 1 for _, c, _ in T.merge_sweep_shapes() if c is not None)     # wst is odd
    for name, (C, N, H, W, want) in T.HIST_CASES.items():
        assert T.argmax_hist_plan(C, N, H, W)[:2] == want, name
    assert T.argmax_hist_plan(19, 2, 728, 728)[2] == T.EVAL_HIST_BLOCKS == 512
    assert {T.argmax_hist_plan(C, 1, 1, P)[:2] for C in T.HIST_SWEEP_C for P in range(1, 41)} == {(1, 0), (4, 0), (4, 8), (4, 19)}

    # K17
    for name, (C, low, out, want, seed) in T.UP_CASES.items():
        assert lib.cabinet_predict_up_argmax_supported(C, *low, *out) == 1, name
        assert T.predict_up_plan(C, low, out)[:2] == want, (name, T.predict_up_plan(C, low, out))
        found = T.find_up_seed(C, low, out)
        assert found is not None and found[0] == seed and found[1][4] <= MAX_UNDECIDED_SHARE, (name, found and found[0])
    up = {n: T.predict_up_plan(*c[:3]) for n, c in T.UP_CASES.items()}
    assert {(p[0], p[3]) for p in up.values()} == {(256, 19), (256, 8), (256, 0), (128, 0), (64, 0), (128, 19), (64, 8)}
    assert up["production-width-2048"][:2] == (256, 2) and up["two-segments-packed"][4] and not up["second-segment-one-pixel"][4]
    assert 1025 - 4 * 256 == 1 and 2049 - 2 * 4 * 256 == 1 and 513 - 2 * 4 * 64 == 1    # ragged last segments of one pixel
    assert 19 * 862 * 4 <= T.PREDICT_LDS_MAX < 19 * 863 * 4 and 32 * 512 * 4 == T.PREDICT_LDS_MAX
    for name, c in T.UP_REFUSED.items():
        assert lib.cabinet_predict_up_argmax_supported(c[0], *c[1], *c[2]) == 0 and T.predict_up_plan(*c)[0] == 0, name
    for name, (C, low, out, _) in T.UP_TIES.items():
        assert T.predict_up_plan(C, low, out)[1] >= 2, name
    for C in T.UP_SWEEP_C:
        shapes = T.up_sweep_shapes(C)
        assert len(shapes) == 66 and all(lib.cabinet_predict_up_argmax_supported(c, *lo, *o) == 1 for c, lo, o in shapes)
        assert {T.predict_up_plan(*s)[1] for s in shapes} >= {1, 2, 3}
    assert {T.predict_up_plan(*s)[0] for s in T.up_sweep_shapes(19)} == {64, 128, 256}
    assert max(T.predict_up_plan(*s)[1] for s in T.up_sweep_shapes(19)) == 5
    for name, c in T.ARGMAX_CASES.items():
        assert T.predict_argmax_plan(*c) == (False, 0, 3, 3), name
    assert T.predict_argmax_plan(19, 1, 1, 40) == (True, 19, 1, 4) and T.predict_argmax_plan(19, 1, 1, 40, aligned=False)[0] is False

    # K16
    for numels in ([1], [4096], [4097], [3 * 4096 + 5, 1], T.TAIL_SIZES, [2049 * 4096 + 5, 1]):
        n = T.tail_chunks(numels)
        assert len(optim.build_chunks(numels)) == n
        assert lib.cabinet_sgd_tail_workspace_bytes(n) == T.tail_workspace_bytes(n), numels
    n = T.tail_chunks([2049 * 4096 + 5, 1])
    assert n == 2051 and T.tail_grid(n) == T.TAIL_GRID_CAP == 2048 and n - T.tail_grid(n) == 3 and T.tail_grid(n, 64) == 64
    assert T.tail_grid(T.tail_chunks([3 * 4096 + 5, 1]), 2) == 2 and T.tail_grid(5) == 5
    assert len(T.TAIL_SIZES) == 25 and T.tail_chunks(T.TAIL_SIZES) == 25 + 3 + 2 + 2   # 4097..4099, 8191, 8192; 8193 is three


# ------------------------------------------------------------------------------------------------ shared pieces
def _elementwise(fails, tag, got, want, e32, floor):
    """|got - want| <= max(4 E32, floor) element by element; floor a number or a tensor.  The first miss is located."""
    g = got.detach().double().cpu()
    if tuple(g.shape) != tuple(want.shape) or not bool(torch.isfinite(g).all()):
        fails.append(f"{tag}: shape {tuple(g.shape)} or not finite")
        return
    err = (g - want).abs()
    bound = torch.clamp(torch.as_tensor(floor, dtype=torch.float64).expand_as(err), min=4.0 * e32)
    _DIST[tag] = (e32, float(err.max()))
    over = err - bound
    if bool((over > 0).any()):
        where = np.unravel_index(int(over.argmax()), tuple(err.shape))
        fails.append(f"{tag}: {int((over > 0).sum())} elements beyond the bound, the worst |d| = {float(err[where]):.3e} (bound "
                     f"{float(bound[where]):.3e}, E32 {e32:.3e}) at {tuple(int(i) for i in where)} of {tuple(err.shape)}")


def _print_distances(what):
    if _DIST:
        worst = max(_DIST, key=lambda k: _DIST[k][1])
        print(f"{what}: {len(_DIST)} maps, largest E32 {max(v[0] for v in _DIST.values()):.3e}, largest kernel distance "
              f"{_DIST[worst][1]:.3e} (E32 there {_DIST[worst][0]:.3e}, {worst})")
    _DIST.clear()


def _guarded(shape, offset, pad=64):
    """A dense uint8 view of `shape`, `offset` bytes into a buffer filled with GUARD, and the buffer."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + pad,), GUARD, dtype=torch.uint8, device="cuda")
    return buf[offset:offset + n].view(*shape), buf


def _guard_ok(buf, offset, n):
    b = buf.cpu().numpy()
    return bool((b[:offset] == GUARD).all() and (b[offset + n:] == GUARD).all())


def _off4(t):
    """The same values in a dense tensor that starts 4 bytes into its storage."""
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape).copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------ 2. K13 on the GPU
def _chip_run(fails, tag, C, low, chip, flip, N, seed, origins=None):
    from cabinet_amd.functional import eval_chip_accum, eval_chip_accum_supported

    a, b, rcy, rcx, (FH, FW) = T.chip_inputs(C, low, chip, flip, N, seed)
    ad, bd, (ch, cw) = a.cuda(), (b.cuda() if flip else None), chip
    assert eval_chip_accum_supported(ad, chip, flip), tag
    g = torch.Generator().manual_seed(seed + 100)
    all_origins = T.chip_origins(chip, (FH, FW))
    for i in (range(5) if origins is None else origins):
        origin = all_origins[i]
        dst0 = torch.rand(N, C, FH, FW, generator=g)
        ry, rx = (rcy, rcx) if i < 4 else (None, None)
        runs = []
        for _ in range(2):
            dst = dst0.cuda()
            eval_chip_accum(dst, ad, bd, chip, origin, None if ry is None else ry.cuda(), None if rx is None else rx.cuda())
            runs.append(dst)
        got = runs[0].cpu()
        otag = f"{tag} origin {origin}"
        if not torch.equal(runs[0], runs[1]):
            fails.append(f"{otag}: a second run differs")
        outside = torch.ones(FH, FW, dtype=torch.bool)
        outside[origin[0]:origin[0] + ch, origin[1]:origin[1] + cw] = False
        if not torch.equal(got[:, :, outside], dst0[:, :, outside]):
            fails.append(f"{otag}: a value outside the window changed")
        want, e32 = T.chip_refs(dst0, a, b, chip, origin, ry, rx)
        _cmp(fails, otag, "dst", got, want, tol=1e-4, atol=0.0)
        _elementwise(fails, otag, got, want, e32, 2e-6)


@gpu
@pytest.mark.parametrize("name", list(T.CHIP_CASES))
def test_chip_accum_plan_case_vs_float64(name):
    """T = 256 | 128 | 64 for CMAX = 0 | 19 | 8, one and two sources, the 64 KB boundary itself: the bounds of the module
    docstring at the four corner origins and an interior origin without the reciprocal vectors."""
    C, low, chip, flip, want, N = T.CHIP_CASES[name]
    assert T.eval_chip_plan(C, low, chip, flip)[:3] == want
    fails = []
    _DIST.clear()
    _chip_run(fails, name, C, low, chip, flip, N, seed=C * 1000 + chip[1])
    torch.cuda.synchronize()
    _print_distances(f"chip_accum {name} T={want[0]}")
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("name", list(T.CHIP_REFUSED))
def test_chip_accum_refused_before_any_launch(name):
    from cabinet_amd.functional import eval_chip_accum, eval_chip_accum_supported

    (C, low, chip, flip), neighbour = T.CHIP_REFUSED[name]
    a, b, rcy, rcx, (FH, FW) = T.chip_inputs(C, low, chip, flip, 1, 3)
    ad, bd = a.cuda(), b.cuda()
    assert eval_chip_accum_supported(ad, chip, flip) is False
    dst0 = torch.rand(1, C, FH, FW)
    dst = dst0.cuda()
    with pytest.raises(RuntimeError, match="LDS"):
        eval_chip_accum(dst, ad, bd, chip, (1, 2), rcy.cuda(), rcx.cuda())
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), dst0), "a refused call changed dst"
    nC, nlow, nchip, nflip = T.CHIP_CASES[neighbour][:4]
    fails = []
    _chip_run(fails, neighbour, nC, nlow, nchip, nflip, 1, seed=4, origins=[3])
    _DIST.clear()
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("hh", T.CHIP_SWEEP_HH, ids=[f"{a}to{b}" for a, b in T.CHIP_SWEEP_HH])
@pytest.mark.parametrize("C", T.CHIP_SWEEP_C)
def test_chip_accum_residue_sweep(C, hh):
    """cw at 1, 2, 3 and either side of 64, 128, 256, 512 (the segment seams of T = 256 and the wave), wl = cw, ceil(cw / 8),
    ceil(3 cw / 7), one and two sources; the window in the far corner of a larger destination."""
    fails, ran = [], 0
    _DIST.clear()
    for _, low, chip, flip in T.chip_sweep_shapes(C, hh):
        _chip_run(fails, f"C={C} {low}->{chip} flip={flip}", C, low, chip, flip, 1, seed=chip[1] + low[1], origins=[3])
        ran += 1
    torch.cuda.synchronize()
    _print_distances(f"chip_accum sweep C={C} {hh}")
    _report(fails, ran, 90)


def _merge_run(fails, tag, N, C, src, crop, out, seed):
    from cabinet_amd.functional import eval_scale_merge

    prob, total0 = T.merge_inputs(N, C, src, out, seed)
    want, e32 = T.merge_refs(total0, prob, crop, out)
    runs = []
    for _ in range(2):
        total = total0.cuda()
        eval_scale_merge(total, prob.cuda(), crop)
        runs.append(total)
    if not torch.equal(runs[0], runs[1]):
        fails.append(f"{tag}: a second run differs")
    _cmp(fails, tag, "total", runs[0], want, tol=1e-5, atol=0.0)
    _elementwise(fails, tag, runs[0], want, e32, 5e-7 * want.abs().clamp_min(1.0))
    return runs[0].cpu(), prob, total0


@gpu
@pytest.mark.parametrize("name", list(T.MERGE_CASES))
def test_scale_merge_plan_case_vs_float64(name):
    C, src, crop, out, want = T.MERGE_CASES[name]
    assert T.scale_merge_plan(out[1]) == want
    fails = []
    _DIST.clear()
    got, prob, total0 = _merge_run(fails, name, 2, C, src, crop, out, seed=C + out[1])
    if name == "one-pixel-crop":   # every output equals the one value (the two lerp weights of a pixel sum to 1 +- an ulp)
        one = (total0.double() + prob.double()[:, :, 2:3, 4:5]).expand_as(total0)
        assert float((got.double() - one).abs().max()) <= 5e-7 * float(one.abs().max().clamp_min(1.0))
    torch.cuda.synchronize()
    _print_distances(f"scale_merge {name}")
    _report(fails, 1, 1)


@gpu
def test_scale_merge_at_the_grid_limit_of_planes():
    """N * C = 65535 planes of one pixel: the last z index of the grid."""
    from cabinet_amd.functional import eval_scale_merge, eval_scale_merge_supported

    NC = T.MERGE_MAX_PLANES[0]
    g = torch.Generator().manual_seed(7)
    prob, total0 = torch.rand(1, NC, 1, 1, generator=g), torch.rand(1, NC, 1, 1, generator=g)
    total = total0.cuda()
    assert eval_scale_merge_supported(total)
    eval_scale_merge(total, prob.cuda())
    assert torch.equal(total.cpu(), total0 + prob)


@gpu
def test_scale_merge_residue_sweep():
    """W = 1..9 and either side of 256, 1024 and 1028 (the workgroup seams of the scalar and the vector form) at H = 2."""
    fails, ran = [], 0
    _DIST.clear()
    for src, crop, out in T.merge_sweep_shapes():
        _merge_run(fails, f"{src}{crop}->{out}", 1, 2, src, crop, out, seed=out[1] + src[1])
        ran += 1
    torch.cuda.synchronize()
    _print_distances("scale_merge sweep")
    _report(fails, ran, 66)


def _hist_run(fails, tag, C, N, H, W, seed):
    from cabinet_amd.functional import eval_argmax_hist

    total, labels, tie, lo = T.hist_inputs(C, N, H, W, seed)
    want_pred, want = T.hist_ref(total, labels, C)
    assert bool((want_pred[tie] == lo).all()), tag      # the plant: the lowest of the equal classes, exactly
    td, ld = total.cuda(), labels.cuda()
    hist = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    pred = eval_argmax_hist(td, ld, hist, 255, want_pred=True)
    if pred.dtype != torch.uint8 or not torch.equal(pred.cpu().long(), want_pred):
        fails.append(f"{tag}: the prediction differs from torch.argmax")
    if not np.array_equal(hist.cpu().numpy(), want):
        fails.append(f"{tag}: the matrix differs from numpy.bincount")
    if eval_argmax_hist(td, ld, hist, 255) is not None or not np.array_equal(hist.cpu().numpy(), 2 * want):
        fails.append(f"{tag}: a second call without the prediction does not accumulate")
    return want


@gpu
@pytest.mark.parametrize("name", list(T.HIST_CASES))
def test_argmax_hist_plan_case_exact(name):
    """Every (VEC, CFIX) pair, the Cityscapes instantiation <4, 19> among them: planted ties, labels 255, 200 and -3, with and
    without the prediction, a second call that accumulates."""
    C, N, H, W, want = T.HIST_CASES[name]
    assert T.argmax_hist_plan(C, N, H, W)[:2] == want
    fails = []
    for seed in (1, 2, 3):
        _hist_run(fails, f"{name} seed {seed}", C, N, H, W, seed)
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("C", T.HIST_SWEEP_C)
def test_argmax_hist_pixel_count_sweep(C):
    """N = 1 and 3 at every pixel count 1..40 (H = 1): VEC = 4 where P % 4 == 0 and 1 elsewhere, one ragged workgroup."""
    fails, ran = [], 0
    for N in (1, 3):
        for P in range(1, 41):
            _hist_run(fails, f"C={C} N={N} P={P}", C, N, 1, P, seed=P)
            ran += 1
    _report(fails, ran, 80)


# ------------------------------------------------------------------------------------------------ 3. K17 on the GPU
def _up_run(fails, tag, C, low, out, N, seed, case=None, offsets=(1,)):
    """The decision rule of test_up_argmax_vs_float64 on a seed whose float64 reference alone meets the share; then the same
    call with `out=` `offset` bytes into a guarded buffer."""
    from cabinet_amd.functional import predict_up_argmax, predict_up_argmax_supported

    a, want, undecided, e32, share = case if case is not None else T.up_case(C, low, out, N, seed)
    assert share <= MAX_UNDECIDED_SHARE, (tag, seed, share)
    ad = a.cuda()
    assert predict_up_argmax_supported(ad, out), tag
    got = predict_up_argmax(ad, out)
    if got.dtype != torch.uint8 or tuple(got.shape) != (N, *out):
        fails.append(f"{tag}: dtype or shape")
        return
    bad = (got.cpu().long() != want) & ~undecided
    if bool(bad.any()):
        n, y, x = (int(v[0]) for v in torch.nonzero(bad, as_tuple=True))
        fails.append(f"{tag} seed {seed}: {int(bad.sum())} decided pixels differ from the float64 argmax, the first at (n, y, x) = "
                     f"({n}, {y}, {x}); x of all of them {sorted(set(torch.nonzero(bad)[:, 2].tolist()))[:12]}")
    for offset in offsets:
        view, buf = _guarded((N, *out), offset)
        if predict_up_argmax(ad, out, out=view) is not view or not _guard_ok(buf, offset, view.numel()):
            fails.append(f"{tag} offset {offset}: a byte outside the tensor changed")
        if not torch.equal(view, got):
            fails.append(f"{tag} offset {offset}: the bytes differ from the ordinary call's")


@gpu
@pytest.mark.parametrize("name", list(T.UP_CASES))
def test_up_argmax_plan_case_vs_float64(name):
    C, low, out, want, seed = T.UP_CASES[name]
    assert T.predict_up_plan(C, low, out)[:2] == want
    fails = []
    _up_run(fails, name, C, low, out, 2, seed, offsets=(0, 1))
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("name", list(T.UP_TIES))
def test_up_argmax_planted_ties_over_several_segments(name):
    """Two equal planes above the rest stay equal under any resize: the lower index everywhere, in every segment."""
    from cabinet_amd.functional import predict_up_argmax

    C, low, out, (lo, hi) = T.UP_TIES[name]
    g = torch.Generator().manual_seed(5)
    a = torch.randn(2, C, *low, generator=g)
    a[:, lo] = a.max(dim=1).values + 1.0
    a[:, hi] = a[:, lo]
    rest = [c for c in range(C) if c not in (lo, hi)]
    assert lo < hi and torch.equal(a[:, lo], a[:, hi]) and bool((a[:, rest].max(dim=1).values + 1.0 <= a[:, lo]).all())   # no near-tie
    got = predict_up_argmax(a.cuda(), out)
    assert tuple(got.shape) == (2, *out) and bool((got == lo).all())


@gpu
@pytest.mark.parametrize("name", list(T.UP_REFUSED))
def test_up_argmax_refused_before_any_launch(name):
    from cabinet_amd.functional import predict_up_argmax, predict_up_argmax_supported

    C, low, out = T.UP_REFUSED[name]
    a = torch.randn(1, C, *low).cuda()
    assert predict_up_argmax_supported(a, out) is False
    view, buf = _guarded((1, *out), 0)
    with pytest.raises(RuntimeError, match="LDS"):
        predict_up_argmax(a, out, out=view)
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all()), "a refused call changed out"


@gpu
@pytest.mark.parametrize("C", T.UP_SWEEP_C)
def test_up_argmax_residue_sweep(C):
    """W = 1..9 and either side of 256, 512, 1024, 1028 and 2048 (the segment seams of T = 64, 128, 256), wl = W, ceil(W / 8),
    ceil(3 W / 7), the output at byte offsets 0 and 1; the seed searched per shape on the float64 reference."""
    fails, ran = [], 0
    for _, low, out in T.up_sweep_shapes(C):
        found = T.find_up_seed(C, low, out, N=1)
        assert found is not None, f"{(C, low, out)}: no seed of {T.SEEDS} meets the undecided share on the float64 reference"
        _up_run(fails, f"C={C} {low}->{out}", C, low, out, 1, found[0], case=found[1], offsets=(0, 1))
        ran += 1
    _report(fails, ran, 66)


def _argmax_run(fails, tag, C, N, H, W, seed, offsets):
    from cabinet_amd.functional import predict_argmax

    t = T.argmax_inputs(C, N, H, W, seed)
    want = torch.argmax(t, dim=1)
    td = t.cuda()
    got = predict_argmax(td)
    if got.dtype != torch.uint8 or not torch.equal(got.cpu().long(), want):
        fails.append(f"{tag}: differs from torch.argmax")
    for offset in offsets:
        view, buf = _guarded((N, H, W), offset)
        predict_argmax(td, out=view)
        if not _guard_ok(buf, offset, view.numel()) or not torch.equal(view.cpu().long(), want):
            fails.append(f"{tag} offset {offset}: guard band or bytes")


@gpu
@pytest.mark.parametrize("name", list(T.ARGMAX_CASES))
def test_argmax_bytewise_form_over_three_workgroups(name):
    C, N, H, W = T.ARGMAX_CASES[name]
    assert T.predict_argmax_plan(C, N, H, W) == (False, 0, 3, 3)
    fails = []
    _argmax_run(fails, name, C, N, H, W, 3, offsets=(0, 1, 2, 3))
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("C", T.ARGMAX_SWEEP_C)
def test_argmax_pixel_count_sweep(C):
    fails, ran = [], 0
    for P in range(1, 41):
        _argmax_run(fails, f"C={C} P={P}", C, 2, 1, P, P, offsets=(0, 1))
        ran += 1
    _report(fails, ran, 40)


@gpu
@pytest.mark.parametrize("with_image", [False, True], ids=["labels-only", "with-image"])
def test_render_groups_straddling_images(with_image):
    """N = 1, 2, 3 images of 1..13 pixels, every output 0..3 bytes into a guarded buffer: four-pixel groups that straddle
    images, img_vec on (H W % 4 == 0) and off, byte for byte predict_golden.render_contract."""
    from cabinet_amd.functional import predict_render
    from cabinet_amd.predict import CITYSCAPES_COLORS

    pal = torch.from_numpy(CITYSCAPES_COLORS.copy()).cuda()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    fails, ran = [], 0
    for N in (1, 2, 3):
        for P in range(1, 14):
            g = torch.Generator().manual_seed(100 * N + P)
            labels = torch.randint(0, 24, (N, 1, P), generator=g).to(torch.uint8)    # beyond the palette: clipped
            image = torch.randn(N, 3, 1, P, generator=g) if with_image else None
            want = render_contract(labels.numpy(), None if image is None else image.numpy(), CITYSCAPES_COLORS, mean, std, 0.6)
            for offset in range(4):
                lab, _ = _guarded((N, 1, P), offset)
                lab.copy_(labels)
                views = {k: _guarded((N, 1, P, 3), offset) for k in want}
                res = predict_render(lab, None if image is None else image.cuda(), pal, mean, std, 0.6,
                                     out={k: v[0] for k, v in views.items()})
                for k, (view, buf) in views.items():
                    if res[k] is not view or not _guard_ok(buf, offset, view.numel()):
                        fails.append(f"N={N} P={P} offset {offset} {k}: a byte outside the tensor changed")
                    if not np.array_equal(view.cpu().numpy(), want[k]):
                        fails.append(f"N={N} P={P} offset {offset} {k}: bytes differ from the contract")
                ran += 1
    _report(fails, ran, 3 * 13 * 4)


# ------------------------------------------------------------------------------------------------ 4. K16 on the GPU
def _two(device, g):
    return [torch.randn(3 * 4096 + 5, generator=g).to(device), torch.randn(1, generator=g).to(device)]


def _mixed(device, g):
    return [torch.randn(n, generator=g).to(device) for n in (4097, 7, 300, 1)]


def _plant_inf(step_no):
    def hook(s, net, opt):
        if s == step_no:
            net.p[0].grad.view(-1)[11] = float("inf")
    return hook


def _poison(net, opt):
    for p in net.p:
        opt.optim.state[p]["momentum_buffer"].fill_(float("nan"))


@gpu
@pytest.mark.parametrize("name,over,steps", [
    ("momentum-0", dict(momentum=0.0), 3), ("no-ema", dict(ema=False), 3), ("no-clip", dict(max_grad_norm=0.0), 3),
    ("no-warmup", dict(warmup_steps=0), 3), ("past-max-iter", dict(max_iter=2), 4), ("no-weight-decay", dict(wd=0.0), 3)])
def test_tail_configurations_against_the_composite(name, over, steps):
    """The configurations no device test launched: has_buf false, has_ema false, max_norm <= 0, warmup_steps = 0, `it` past
    max_iter (the rate reaches exactly 0 and the parameters stop), wd = 0."""
    host, oh, dev, od = T.against_composite(_mixed, steps=steps, over=over)
    if name == "momentum-0":
        assert not any("momentum_buffer" in od.optim.state.get(p, {}) for p in dev.p)
    if name == "no-ema":
        assert od.ema is None and od.ema_updates == steps
    if name == "no-clip":
        assert float(od._scalars[1]) == 1.0
    if name == "past-max-iter":
        before = [p.detach().clone() for p in dev.p]
        assert od.lr.cpu().tolist() == [0.0] * 4 and oh.lr.tolist() == [0.0] * 4
        for p in dev.p:
            p.grad = torch.ones_like(p)
        od.step()
        assert od.it == steps + 1 and all(torch.equal(a, p.detach()) for a, p in zip(before, dev.p))


@gpu
def test_tail_nonfinite_norm_without_the_skip():
    """One inf gradient element with skip_nonfinite=False: the clip coefficient is 0, inf * 0 = NaN at that element on host and
    device alike, every other element within the bound."""
    host, oh, dev, od = T.against_composite(_mixed, over=dict(skip_nonfinite=False), hook=_plant_inf(2), finite=False)
    assert od.skipped == 0 and od.it == 3
    assert int((~torch.isfinite(dev.p[0].detach())).sum()) == 1 and all(bool(torch.isfinite(p).all()) for p in list(dev.p)[1:])


@gpu
def test_tail_nonfinite_norm_skips_the_step():
    before = {}

    def hook(s, net, opt):
        _plant_inf(1)(s, net, opt)
        before[net.p[0].device.type] = T.tail_state(net, opt)

    host, oh, dev, od = T.against_composite(_mixed, steps=1, hook=hook)
    assert od.skipped == 1 and od.it == 0 and od.ema_updates == 0 and int(od._flags[0]) == 1 and int(od._flags[1]) == 0
    after = T.tail_state(dev, od)
    assert all(torch.equal(after[k], before["cuda"][k]) for k in after), "a skipped step changed a tensor"


@gpu
def test_tail_first_step_overwrites_a_poisoned_buffer():
    """Every momentum buffer NaN before the first step; step 1 carries an inf gradient and is skipped, step 2 is the first that
    runs: it must write its buffers without reading them (`first`), and `valid` must not have been set by the skipped step."""
    host, oh, dev, od = T.against_composite(_mixed, steps=3, setup=_poison, hook=_plant_inf(1))
    assert od.skipped == 1 and od.it == 2


@gpu
def test_tail_first_step_of_a_late_gradient():
    """One parameter has no gradient at step 1 (its entry is EMA-only) and one from step 2 on; its buffer is NaN until then."""
    def hook(s, net, opt):
        if s == 1:
            net.p[2].grad = None

    host, oh, dev, od = T.against_composite(_mixed, steps=3, setup=_poison, hook=hook)
    assert od.it == 3 and bool(torch.isfinite(od.optim.state[dev.p[2]]["momentum_buffer"]).all())


_MISALIGNED = ["param", "grad", "buf", "ema", "all"]


def _misaligned_run(which):
    """-> the device state after three steps with the named tensors of entry 0 starting 4 bytes into their storage."""
    forms = ("param", "grad", "buf", "ema") if which == "all" else (which,) if which else ()

    def tensors_of(device, g):
        big, one = _two(device, g)
        return [T.offset_tensor(big, device) if "param" in forms else big, one]

    def setup(net, opt):
        p = net.p[0]
        if "buf" in forms:
            opt.optim.state[p]["momentum_buffer"] = T.offset_tensor(opt.optim.state[p]["momentum_buffer"], p.device)
        if "ema" in forms:
            opt.ema.p[0].data = T.offset_tensor(opt.ema.p[0].data, p.device)

    def hook(s, net, opt):
        if "grad" in forms:
            net.p[0].grad = T.offset_tensor(net.p[0].grad, net.p[0].device)
        if net.p[0].is_cuda:
            p = net.p[0]
            ptrs = dict(param=p, grad=p.grad, buf=opt.optim.state[p]["momentum_buffer"], ema=opt.ema.p[0])
            assert {k for k, t in ptrs.items() if t.data_ptr() % 16 == 4} == set(forms) and \
                all(t.data_ptr() % 16 in (0, 4) for t in ptrs.values())

    host, oh, dev, od = T.against_composite(tensors_of, setup=setup, hook=hook)
    return T.tail_state(dev, od), od.last_grad_norm.clone()


@gpu
def test_tail_each_pointer_of_an_entry_misaligned():
    """ptr_aligned16 joins four pointers: each alone 4 bytes into its storage, then all four, sends the chunks of a 3 * 4096 + 5
    tensor down the scalar path.  Within the composite bound, and the bits of the all-aligned run."""
    base, base_norm = _misaligned_run(None)
    bad = []
    for which in _MISALIGNED:
        got, norm = _misaligned_run(which)
        bad += [f"{which}: {k}" for k in base if not torch.equal(got[k], base[k])]
        if not torch.equal(norm, base_norm):
            bad.append(f"{which}: the norm {float(norm):.9g} vs {float(base_norm):.9g}")
    assert not bad, f"not the bits of the all-aligned run: {bad}"


@gpu
def test_tail_size_sweep_aligned_and_misaligned():
    """One tensor of every size 1..9 and either side of 256, 1024, 4096 (4093..4099) and 8192, aligned and with every
    parameter 4 bytes into its storage."""
    res = []
    for off in (False, True):
        def tensors_of(device, g):
            vals = [torch.randn(n, generator=g) for n in T.TAIL_SIZES]
            return [T.offset_tensor(v, device) if off else v.to(device) for v in vals]

        host, oh, dev, od = T.against_composite(tensors_of)
        assert len(od._chunks_host) == T.tail_chunks(T.TAIL_SIZES)
        assert all(p.data_ptr() % 16 == (4 if off else 0) for p in dev.p)
        res.append(T.tail_state(dev, od))
    assert all(torch.equal(res[0][k], res[1][k]) for k in res[0])


@gpu
def test_tail_more_chunks_than_the_kernels_own_cap():
    """2049 * 4096 + 5 elements and a scalar in the second group: 2051 chunks on 2048 workgroups, three of which take two
    chunks.  Against the composite, and the bits of the same run on 64 workgroups."""
    def tensors_of(device, g):
        return [torch.randn(2049 * 4096 + 5, generator=g).to(device), torch.randn(1, generator=g).to(device)]

    host, oh, dev0, o0 = T.against_composite(tensors_of, steps=2, max_grid=0)
    n = len(o0._chunks_host)
    assert n == 2051 and T.tail_grid(n) == 2048
    a = T.tail_state(dev0, o0)
    del host, oh
    # the second run needs no composite: same seeds, same gradients
    g = torch.Generator().manual_seed(5)
    from optim_tail_model import make_tail
    dev = T.Bag(tensors_of("cuda", torch.Generator().manual_seed(6)))
    od = make_tail(dev, lr0=0.05, wd=5e-4, warmup_steps=1, max_iter=10, ema_tau=4)
    od.max_grid = 64
    for _ in range(2):
        for p in dev.p:
            p.grad = (torch.randn(p.shape, generator=g) * 0.05).cuda()
        od.step()
    b = T.tail_state(dev, od)
    assert all(torch.equal(a[k], b[k]) for k in a) and torch.equal(o0.last_grad_norm, od.last_grad_norm)


# ------------------------------------------------------------------------------------------------ 5. caller contract
def _logit_layouts(x):
    """name -> the same values (a half can hold them) channels_last, 4 bytes into the storage, in half precision."""
    out = {"channels_last": x.contiguous(memory_format=torch.channels_last), "4 bytes into the storage": _off4(x), "fp16": x.half()}
    assert not out["channels_last"].is_contiguous() and all(torch.equal(v.float(), x) for v in out.values())
    return out


@gpu
def test_chip_accum_accepts_any_layout():
    from cabinet_amd.functional import eval_chip_accum

    C, low, chip, N = 19, (3, 40), (5, 300), 2
    a, b, rcy, rcx, (FH, FW) = T.chip_inputs(C, low, chip, True, N, 9)
    a, b = a.half().float().cuda(), b.half().float().cuda()
    dst0 = torch.rand(N, C, FH, FW).cuda()
    base = eval_chip_accum(dst0.clone(), a, b, chip, (2, 3), rcy.cuda(), rcx.cuda())
    la, lb_ = _logit_layouts(a), _logit_layouts(b)
    for what in la:
        got = eval_chip_accum(dst0.clone(), la[what], lb_[what], chip, (2, 3), rcy.cuda(), rcx.cuda())
        assert torch.equal(got, base), what
    assert torch.equal(eval_chip_accum(dst0.clone(), a.half(), b.half(), chip, (2, 3)),
                       eval_chip_accum(dst0.clone(), a.half().float(), b.half().float(), chip, (2, 3)))
    off = _off4(dst0)
    assert eval_chip_accum(off, a, b, chip, (2, 3), rcy.cuda(), rcx.cuda()) is off and torch.equal(off, base)   # scalar on dst


@gpu
def test_merge_and_hist_refuse_a_misaligned_total():
    """Both kernels move `total` in 16-byte pieces: a `total` 4 bytes into its storage is refused, naming the alignment, before
    any launch."""
    from cabinet_amd.functional import eval_argmax_hist, eval_scale_merge

    g = torch.Generator().manual_seed(3)
    total0 = torch.rand(2, 8, 3, 8, generator=g).cuda()
    prob = torch.rand(2, 8, 3, 8, generator=g).cuda()
    total = _off4(total0)
    with pytest.raises(RuntimeError, match="aligned"):
        eval_scale_merge(total, prob)
    labels = torch.randint(0, 8, (2, 3, 8), generator=g).cuda()
    hist = torch.zeros(8, 8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="aligned"):
        eval_argmax_hist(total, labels, hist, 255)
    torch.cuda.synchronize()
    assert torch.equal(total, total0) and int(hist.abs().sum()) == 0


@gpu
def test_argmax_hist_accepts_any_label_layout():
    from cabinet_amd.functional import eval_argmax_hist

    C, N, H, W = 19, 2, 6, 10
    total, labels, _, _ = T.hist_inputs(C, N, H, W, 4)
    _, want = T.hist_ref(total, labels, C)
    td, ld = total.cuda(), labels.cuda()
    wide = torch.zeros(N, H, W + 3, dtype=torch.int64, device="cuda")
    wide[:, :, 1:W + 1] = ld
    lab8 = torch.empty(ld.numel() + 1, dtype=torch.int64, device="cuda")[1:].view(ld.shape).copy_(ld)
    assert lab8.data_ptr() % 16 == 8 and not wide[:, :, 1:W + 1].is_contiguous()
    for what, lab in (("dense", ld), ("a slice", wide[:, :, 1:W + 1]), ("8 bytes into the storage", lab8)):
        hist = torch.zeros(C, C, dtype=torch.int64, device="cuda")
        eval_argmax_hist(td, lab, hist, 255)
        assert np.array_equal(hist.cpu().numpy(), want), what


@gpu
def test_predict_wrappers_accept_any_layout():
    from cabinet_amd.functional import predict_argmax, predict_up_argmax

    g = torch.Generator().manual_seed(8)
    low = (torch.randn(2, 19, 3, 130, generator=g) * 3.0).half().float().cuda()
    full = torch.randn(2, 19, 5, 8, generator=g).half().float().cuda()
    base_up, base_arg = predict_up_argmax(low, (5, 1040)), predict_argmax(full)
    lows, fulls = _logit_layouts(low), _logit_layouts(full)
    for what in lows:
        assert torch.equal(predict_up_argmax(lows[what], (5, 1040)), base_up), what
        assert torch.equal(predict_argmax(fulls[what]), base_arg), what
