"""Backbone kernels (K7 BatchNorm + activation / gate / SE tail, K8 depthwise, K9 stem, K10 thin pointwise, K14 wide pointwise
weight gradient, K15 3x3 stride-2 backward) where their host-side launch plans branch and where their tiles end -- every case
through the C ABI, against the fp64 CPU oracle of the kernel's own test file.

1. Plan-branch cases: one shape per branch of a launch plan that no other operator test reaches (the second trip of the
   `t += 256` finalize loops, the grid-stride walk of K10 over ragged image borders, `rows_per > 1` in the K15 data gradient,
   both forms of the slab sum either side of 128 slabs, uneven K14 splits).  Criteria as in the per-kernel files: per tensor
   ||a-b|| <= 1e-3 ||b||, running statistics at 1e-5, two runs bit-equal, the 2x-stock bound where the file has it (both
   distances printed), NaN-prefilled outputs for the kernels that are called directly.
2. `test_plan_branch_cases_reach_their_branches` (no GPU): reads every plan back through the `*_workspace_bytes` entry points
   and asserts that the shapes of part 1 are what they claim.  A retuned plan constant turns it red instead of letting the
   coverage lapse.
3. Dense residue sweeps: every (H, W) / P of a grid around the tile sizes, all failing shapes collected into one message, the
   number of shapes run asserted.  Per tensor the 1e-3 rule; for the maps (y, dx, dz) also max|a-b| <= 1e-3 max|b|, so that a
   single wrong pixel cannot hide in a large plane.
4. Caller contract of the backbone wrappers: channels_last inputs, inputs 4 bytes into their storage, non-contiguous and
   stride-0 output gradients give bit for bit the results of the dense, aligned call.
"""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_bn_act as t_bn
import test_gpu_conv3x3s2 as t_c3
import test_gpu_pwconv_wide as t_pww
from conftest import assert_close, rel_err

gpu = pytest.mark.gpu
TOL = 1e-3  # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32; the sweeps apply the same 1e-3 in the max norm to the maps

KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
ACTS = [None, "relu", "hardswish"]

# ------------------------------------------------------------------------------------------------ the plan-branch table
K7_SHAPE = (3, 2, 841, 839)                                    # 87 chunks x 3 images = 261 partials per channel (> 256); P odd
K8_SHAPE = (3, 2, 330, 330)                                    # 6 x 21 tiles x 3 images = 378 partials per channel (> 256)
K10_SHAPES = [(5, 16, 40, 255, 257), (5, 8, 16, 255, 257)]     # 5 x 1024 blocks on the 2048 grid; P % 64 = 63
K15_SHAPES = [(64, 65, 8), (64, 65, 9)]                        # dgrad rows_per = 5 (see _cd_plan); wgrad 64 x 7 = 448 slabs
SLAB_SHAPES = [((1, 1015, 10), 127), ((1, 1024, 10), 128), ((1, 1026, 10), 129)]   # K9 and K15 3 -> 16: slabs = ceil(Ho / 4)
K14_SHAPE = (3, 40, 24, 150, 151)                              # 3 x 354 = 1062 chunks over 512 splits; P % 64 = 58


def _a256(n):
    return (n + 255) // 256 * 256


def _cd_plan(B, H, W):
    """cd_plan of conv3x3_s2.hip restated (the data gradient has no workspace to query): strips = min(512 / (B * tiles), Ho)
    with tiles = ceil(Wo / 64), rows_per = ceil(Ho / strips), strips = ceil(Ho / rows_per) -> (rows_per, strips, Ho)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    strips = max(1, min(512 // (B * -(-Wo // 64)), Ho))
    rows_per = -(-Ho // strips)
    return rows_per, -(-Ho // rows_per), Ho


def test_plan_branch_cases_reach_their_branches():
    """Every row of the table above reaches the branch it is there for, read back from the library's own plans."""
    from cabinet_amd import _lib

    lib = _lib.load()
    # K7: more than 256 (mean, M2) / (sum du, sum du xhat) partials per channel, and a plane that ends in a scalar tail
    B, C, H, W = K7_SHAPE
    P = H * W
    ws = lib.cabinet_bn_act_workspace_bytes(B, C, P)
    assert P % 2 == 1 and ws == _a256(2 * C * B * 87 * 4) + _a256(2 * C * 4)
    assert ws - _a256(2 * C * 4) > _a256(2 * C * 256 * 4) and B * 87 == 261
    # K8: more than 256 tile partials per channel in dwconv_dw_finalize_kernel and in the fused form's bn_bwd_tail_run
    B, C, H, W = K8_SHAPE
    for K, S in KS:
        ws = lib.cabinet_dwconv_bwd_workspace_bytes(B, C, H, W, K, S)
        assert ws == _a256(C * 378 * K * K * 4) and (ws - 255) / (C * K * K * 4) > 256
        fused = lib.cabinet_bn_dwconv_bwd_workspace_bytes(B, C, H, W, K, S)
        assert fused == (lib.cabinet_bn_act_workspace_bytes(B, C, H * W) + _a256(C * 378 * K * K * 4) + _a256(2 * C * 378 * 4)
                         + _a256(2 * C * 4) + _a256(B * C * H * W * 4))
    # K10: the grid is capped at 2048 one-wave workgroups and every one of them walks more than two blocks; ragged last block
    for B, Ci, Co, H, W in K10_SHAPES:
        P = H * W
        assert lib.cabinet_pwconv_supported(Ci, Co, P) == 1
        assert lib.cabinet_pwconv_bwd_workspace_bytes(B, Ci, Co, P) == 2048 * Co * Ci * 4
        assert B * -(-P // 64) == 5120 > 2 * 2048 and P % 64 == 63
    # the slab sum switches form at 128 slabs: K9 (64 x 147 floats per slab) and K15 3 -> 16 (432 floats per slab)
    for (B, H, W), n in SLAB_SHAPES:
        assert lib.cabinet_stem_conv_wrw_workspace_bytes(B, H, W) == n * 64 * 147 * 4
        assert lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, 3, 16, H, W) == _a256(n * 432 * 4)
    # K14: 512 splits that do not divide the chunks (two or three each), image borders inside a split, a ragged last chunk
    B, Ci, Co, H, W = K14_SHAPE
    P = H * W
    assert lib.cabinet_pwconv_wide_supported(Ci, Co, P) == 1
    assert lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, Ci, Co, P) == 512 * Co * Ci * 4
    nchunks = B * -(-P // 64)
    assert nchunks == 1062 and nchunks % 512 != 0 and 2 * 512 < nchunks < 3 * 512 and P % 64 == 58
    # K15 64 -> 64: the weight gradient's strips are bound by 512 / (B * tiles) = 8, not by ceil(Ho / 4) = 9 -> 64 x 7 slabs;
    # the data gradient walks rows_per = 5 row pairs per workgroup, 7 strips, the last one 3 rows
    for B, H, W in K15_SHAPES:
        assert lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, 64, 64, H, W) == 448 * 64 * 64 * 9 * 4
        assert _cd_plan(B, H, W) == (5, 7, 33)
    assert all(_cd_plan(*c)[0] == 1 for c in t_c3.CASES_64)  # what the per-kernel file runs: one row pair per workgroup


# ------------------------------------------------------------------------------------------------ shared pieces
def _cmp(fails, tag, name, a, b, maxnorm=False, tol=TOL, atol=1e-6):
    """conftest.assert_close's rule (||a-b|| <= tol ||b|| + atol sqrt(numel)); maxnorm: also max|a-b| <= tol max|b|.
    A miss is appended to ``fails`` instead of raised."""
    if a is None or tuple(a.shape) != tuple(b.shape):
        fails.append(f"{tag} {name}: shape {None if a is None else tuple(a.shape)} vs {tuple(b.shape)}")
        return
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if not bool(torch.isfinite(a).all()):
        fails.append(f"{tag} {name}: not finite")
        return
    err, den = float((a - b).norm()), float(b.norm())
    if not err <= tol * den + atol * (b.numel() ** 0.5):
        fails.append(f"{tag} {name}: rel {err / max(den, 1e-300):.2e}")
    if maxnorm:
        m, top = float((a - b).abs().max()), float(b.abs().max())
        if not m <= tol * top:
            fails.append(f"{tag} {name}: max|a-b| {m:.2e} vs max|b| {top:.2e}")


def _report(fails, ran, expected):
    assert ran == expected, f"{ran} shapes run, {expected} expected"
    assert not fails, f"{len(fails)} misses, the first of them:\n" + "\n".join(fails[:40])


def _set_bn(bn, gen):
    C = bn.num_features
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=gen) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=gen) - 0.5)
        bn.running_mean.copy_(torch.rand(C, generator=gen) - 0.5)
        bn.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
    return bn


KINKS = {None: (), "relu": (0.0,), "hardswish": (-3.0, 3.0)}


def _clear_of_kinks(x, pre, act, step, margin=2e-4):
    """Moves, in place, the elements of ``x`` whose pre-activation ``pre(x.double())`` (same shape, fp64) lies within ``margin``
    of a kink of ``act``.  There the derivative of the activation jumps, so an fp32 pre-activation that lands on the other side
    (its error here is up to ~2e-5) turns one pixel of the gradient, and through the batch sums every pixel of a small plane,
    into another function's: the comparison with fp64 would measure the input, not the kernel."""
    for _ in range(50):
        u = pre(x.double())
        near = torch.zeros(u.shape, dtype=torch.bool)
        for k in KINKS[act]:
            near |= (u - k).abs() < margin
        if not bool(near.any()):
            return x
        x[near] += step
    raise AssertionError("the inputs could not be moved clear of the activation's kinks")


def _bn_pre(bn, training):
    """fp64 BatchNorm of the module ``bn`` (CPU) as a function of the input; the running buffers are left alone."""
    w, b = bn.weight.detach().double(), bn.bias.detach().double()
    rm, rv = bn.running_mean.double(), bn.running_var.double()
    return lambda t: F.batch_norm(t, rm.clone(), rv.clone(), w, b, training, 0.1, bn.eps)


def _dw_case(B, C, H, W, K, S, gen):
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(C, 1, K, K, generator=gen)
    xo, wo = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yo = F.conv2d(xo, wo, None, S, K // 2, 1, C)
    g = torch.randn(yo.shape, generator=gen)
    yo.backward(g.double())
    return x, w, g, (yo.detach(), xo.grad, wo.grad)


def _dw_dev(x, w, g, S):
    from cabinet_amd.functional import dwconv, dwconv_supported

    C, K = w.shape[0], w.shape[-1]
    conv = torch.nn.Conv2d(C, C, K, S, K // 2, groups=C, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    conv = conv.cuda()
    assert dwconv_supported(conv)
    xd = x.cuda().requires_grad_(True)
    y = dwconv(xd, conv)
    y.backward(g.cuda())
    return y.detach(), xd.grad, conv.weight.grad


def _bndw_case(B, C, H, W, K, S, act, training, gen, spread=1.5, mean=0.3):
    """conv(act(bn(z))): inputs, the fp64 result and a function that runs the fused operator on the device."""
    from oracle.model_ref import _hswish

    bn = _set_bn(torch.nn.BatchNorm2d(C), gen)
    cw = torch.randn(C, 1, K, K, generator=gen)
    z = _clear_of_kinks(torch.randn(B, C, H, W, generator=gen) * spread + mean, _bn_pre(bn, training), act, 0.37 * spread)
    zo = z.double().requires_grad_(True)
    wo, bo = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    cwo = cw.double().requires_grad_(True)
    rm, rv = bn.running_mean.double().clone(), bn.running_var.double().clone()
    a = {"relu": F.relu, "hardswish": _hswish}[act](F.batch_norm(zo, rm, rv, wo, bo, training, 0.1, 1e-5))
    yo = F.conv2d(a, cwo, None, S, K // 2, 1, C)
    g = torch.randn(yo.shape, generator=gen)
    yo.backward(g.double())
    ref = {"y": yo.detach(), "dz": zo.grad, "dbn_weight": wo.grad, "dbn_bias": bo.grad, "dconv_weight": cwo.grad,
           "running_mean": rm, "running_var": rv}

    def run():
        from cabinet_amd.functional import bn_act_dwconv

        conv = torch.nn.Conv2d(C, C, K, S, K // 2, groups=C, bias=False)
        with torch.no_grad():
            conv.weight.copy_(cw)
        conv, dbn = conv.cuda(), copy.deepcopy(bn).cuda().train(training)
        zd = z.cuda().requires_grad_(True)
        y = bn_act_dwconv(zd, dbn, act, conv)
        y.backward(g.cuda())
        return {"y": y.detach(), "dz": zd.grad, "dbn_weight": dbn.weight.grad, "dbn_bias": dbn.bias.grad,
                "dconv_weight": conv.weight.grad, "running_mean": dbn.running_mean, "running_var": dbn.running_var}

    return ref, run


def _pw_ref(x, w, g):
    """fp64 1x1 convolution on (B, Ci, P), (Co, Ci), (B, Co, P): y, dx, dw."""
    xo, wo, go = x.double(), w.double(), g.double()
    return (torch.einsum("oc,bcp->bop", wo, xo), torch.einsum("oc,bop->bcp", wo, go), torch.einsum("bop,bcp->oc", go, xo))


def _pw_direct(xd, wd, gd):
    """cabinet_pwconv_fwd / cabinet_pwconv_bwd on device tensors (B, Ci, P), (Co, Ci), (B, Co, P), every output NaN before the call."""
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    lib = _lib.load()
    (B, Ci, P), Co = xd.shape, wd.shape[0]
    nan = float("nan")
    y, dx, dw = torch.full_like(gd, nan), torch.full_like(xd, nan), torch.full_like(wd, nan)
    _lib.check(lib.cabinet_pwconv_fwd(_ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(y), _stream_handle(xd.device)), "cabinet_pwconv_fwd")
    ws, nbytes = _workspace(lib.cabinet_pwconv_bwd_workspace_bytes(B, Ci, Co, P), xd.device)
    rc = lib.cabinet_pwconv_bwd(_ptr(gd), _ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes, _stream_handle(xd.device))
    _lib.check(rc, "cabinet_pwconv_bwd")
    return y, dx, dw


def _stem_wrw(gd, xd):
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    lib = _lib.load()
    B, H, W = xd.shape[0], xd.shape[2], xd.shape[3]
    dw = torch.full((64, 3, 7, 7), float("nan"), dtype=torch.float32, device=xd.device)
    ws, nbytes = _workspace(lib.cabinet_stem_conv_wrw_workspace_bytes(B, H, W), xd.device)
    rc = lib.cabinet_stem_conv_wrw(_ptr(gd), _ptr(xd), B, H, W, _ptr(dw), _ptr(ws), nbytes, _stream_handle(xd.device))
    _lib.check(rc, "cabinet_stem_conv_wrw")
    return dw


def _all_equal(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. plan-branch cases
@gpu
@pytest.mark.parametrize("act", ACTS)
def test_bn_act_more_than_256_partials(act):
    """K7 forward + backward in training mode where both finalize loops take a second trip (261 partials per channel)."""
    from cabinet_amd.functional import bn_act

    B, C, H, W = K7_SHAPE
    g0 = torch.Generator().manual_seed(11)
    bn0 = _set_bn(torch.nn.BatchNorm2d(C), g0)
    x = _clear_of_kinks(torch.randn(B, C, H, W, generator=g0) * 1.7 + 0.6, _bn_pre(bn0, True), act, 0.6)
    g = torch.randn(B, C, H, W, generator=g0)
    ref = t_bn._oracle(x, g, bn0, act, True)
    runs = []
    for _ in range(2):
        bn = copy.deepcopy(bn0).cuda().train()
        xd = x.cuda().requires_grad_(True)
        y = bn_act(xd, bn, act)
        y.backward(g.cuda())
        runs.append([y.detach(), xd.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var])
    torch.cuda.synchronize()
    out = runs[0]
    assert_close(out[0], ref[0], TOL, "y")
    assert_close(out[1], ref[1], TOL, "dx")
    assert_close(out[2], ref[2], TOL, "dweight")
    assert_close(out[3], ref[3], TOL, "dbias")
    assert_close(out[4], ref[4], 1e-5, "running_mean")
    assert_close(out[5], ref[5], 1e-5, "running_var")
    assert _all_equal(*runs)


@gpu
@pytest.mark.parametrize("K,S", KS)
def test_dwconv_more_than_256_tile_partials(K, S):
    """K8, plain and with the BatchNorm folded in (training mode), where the per-channel tile partials exceed one trip of the
    finalize loops (378 per channel)."""
    B, C, H, W = K8_SHAPE
    g0 = torch.Generator().manual_seed(100 * K + S)
    x, w, g, ref = _dw_case(B, C, H, W, K, S, g0)
    runs = [_dw_dev(x, w, g, S) for _ in range(2)]
    torch.cuda.synchronize()
    for name, a, b in zip(("y", "dx", "dw"), runs[0], ref):
        assert_close(a, b, TOL, name)
    assert _all_equal(*runs)
    ref, run = _bndw_case(B, C, H, W, K, S, "relu" if K == 3 else "hardswish", True, g0)
    outs = [run() for _ in range(2)]
    torch.cuda.synchronize()
    for name, b in ref.items():
        assert_close(outs[0][name], b, 1e-5 if name.startswith("running") else TOL, name)
    assert _all_equal(list(outs[0].values()), list(outs[1].values()))


@gpu
@pytest.mark.parametrize("B,Ci,Co,H,W", K10_SHAPES)
def test_pwconv_grid_stride_over_ragged_images(B, Ci, Co, H, W):
    """K10 forward, input gradient and weight gradient where the 2048 workgroups walk 5120 blocks across image borders whose
    last block holds 63 pixels, and the weight gradient leaves 2048 slabs."""
    P = H * W
    g0 = torch.Generator().manual_seed(Ci * 1000 + Co)
    x, w, g = torch.randn(B, Ci, P, generator=g0), torch.randn(Co, Ci, generator=g0) * Ci ** -0.5, torch.randn(B, Co, P, generator=g0)
    ref = _pw_ref(x, w, g)
    xd, wd, gd = x.cuda(), w.cuda(), g.cuda()
    runs = [_pw_direct(xd, wd, gd) for _ in range(2)]
    torch.cuda.synchronize()
    for name, a, b in zip(("y", "dx", "dw"), runs[0], ref):
        assert torch.isfinite(a).all(), name
        e = rel_err(a, b)
        print(f"pwconv B={B} {Ci}->{Co} P={P} {name}: {e:.3e}")
        assert e <= TOL, f"{name}: {e:.3e} > {TOL}"
    assert _all_equal(*runs)


@gpu
@pytest.mark.parametrize("B,H,W", K15_SHAPES)
def test_conv3x3s2_dgrad_several_row_pairs_per_workgroup(B, H, W):
    """K15 data gradient with rows_per = 5: the dy tile in LDS is staged again behind the barrier for every row pair; W = 9
    takes the scalar stores."""
    x, w, g, _, ref = t_c3._inputs(B, 64, 64, H, W, 3, 2, 1)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    runs = [t_c3._native_dx(gd, wd, B, H, W) for _ in range(2)]
    stock = torch.ops.aten.convolution_backward(gd, xd, wd, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])[0]
    torch.cuda.synchronize()
    assert runs[0].shape == stock.shape
    t_c3._check(f"conv3x3s2 dx B={B} 64->64 {H}x{W}", runs[0], stock, ref)
    assert torch.equal(runs[0], runs[1])


@gpu
@pytest.mark.parametrize("B,H,W", K15_SHAPES)
def test_conv3x3s2_wgrad_strips_bound_by_the_grid_target(B, H, W):
    """K15 64 -> 64 weight gradient with 7 strips of 5 rows (the last one 3) per image: 448 slabs into the 32-lane slab sum."""
    x, w, g, ref, _ = t_c3._inputs(B, 64, 64, H, W, 3, 2, 1)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    runs = [t_c3._native_dw(gd, xd, 64, 64) for _ in range(2)]
    stock = t_c3._stock_dw(gd, xd, wd, 2, 1)
    torch.cuda.synchronize()
    t_c3._check(f"conv3x3s2 dw B={B} 64->64 {H}x{W}", runs[0], stock, ref)
    assert torch.equal(runs[0], runs[1])


@gpu
@pytest.mark.parametrize("shape,nslab", SLAB_SHAPES)
def test_slab_sum_either_side_of_128_slabs(shape, nslab):
    """K9's and K15's (3 -> 16) weight gradients with 127, 128 and 129 slabs: the 8-lane form, the switch, the 32-lane form."""
    B, H, W = shape
    x, w, g, ref, _ = t_c3._inputs(B, 3, 64, H, W, 7, 2, 3)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    runs = [_stem_wrw(gd, xd) for _ in range(2)]
    stock = t_c3._stock_dw(gd, xd, wd, 2, 3)
    torch.cuda.synchronize()
    t_c3._check(f"stem dw {nslab} slabs B={B} {H}x{W}", runs[0], stock, ref)
    assert torch.equal(runs[0], runs[1])
    x, w, g, ref, _ = t_c3._inputs(B, 3, 16, H, W, 3, 2, 1)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    runs = [t_c3._native_dw(gd, xd, 3, 16) for _ in range(2)]
    stock = t_c3._stock_dw(gd, xd, wd, 2, 1)
    torch.cuda.synchronize()
    t_c3._check(f"conv3x3s2 dw {nslab} slabs B={B} 3->16 {H}x{W}", runs[0], stock, ref)
    assert torch.equal(runs[0], runs[1])


@gpu
def test_pwconv_wide_uneven_splits():
    """K14 with 1062 chunks over 512 splits: two or three chunks per split, image borders inside a split, a 58-pixel last chunk."""
    B, Ci, Co, H, W = K14_SHAPE
    t_pww.test_pwconv_wide_wgrad_vs_oracle(B, Ci, Co, H, W)  # NaN-prefilled dw, 1e-3 and the 2x-stock bound, distances printed
    g0 = torch.Generator().manual_seed(3)
    x, g = torch.randn(B, Ci, H, W, generator=g0).cuda(), torch.randn(B, Co, H, W, generator=g0).cuda()
    a, b = t_pww._native_dw(g, x, Ci, Co), t_pww._native_dw(g, x, Ci, Co)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. dense residue sweeps
DW_H = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130]
DW_W = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 66, 67, 129]
C3_H = list(range(1, 11)) + [17, 33]
C3_W = list(range(1, 11)) + list(range(31, 36)) + list(range(63, 71)) + list(range(127, 132))
PW_P = list(range(1, 201))
BN_P = list(range(1, 71)) + list(range(8189, 8196)) + list(range(16381, 16388))
# BatchNorm inputs of the sweeps: mean 0.6, spread 0.01.  The narrow spread makes the variance a small difference of large
# numbers (a sum-of-squares formula would lose it), and it keeps the two-sample planes (B P = 2, training) within reach of
# fp32: there dx = gamma invstd (du1 - du2) / 2 * eps / (d^2 + eps), d the half distance of the two samples, is what is left
# of a cancellation with condition number 1 + d^2 / eps.  With unit-spread inputs that is ~1e5, and the stock fp32 operator
# itself lands up to 1.1e-1 (max norm, relative) from fp64; with d ~ 0.01 it is ~10.  (Training mode only.)
BN_MEAN, BN_SPREAD = 0.6, 0.01
BN_SPREAD_EVAL = 1.7  # eval mode has no such cancellation; the wide spread puts pre-activations on both sides of every kink


@gpu
@pytest.mark.parametrize("K,S", KS)
def test_dwconv_residue_sweep(K, S):
    """K8 on 23 x 19 = 437 planes (B = 2, C = 3): y, dx, dw; the fused BatchNorm form on every third, training and eval."""
    gen = torch.Generator().manual_seed(7000 + 10 * K + S)
    fails, ran, fused = [], 0, 0
    for i, (H, W) in enumerate(itertools.product(DW_H, DW_W)):
        tag = f"dwconv K={K} S={S} {H}x{W}"
        x, w, g, ref = _dw_case(2, 3, H, W, K, S, gen)
        out = _dw_dev(x, w, g, S)
        _cmp(fails, tag, "y", out[0], ref[0], maxnorm=True)
        _cmp(fails, tag, "dx", out[1], ref[1], maxnorm=True)
        _cmp(fails, tag, "dw", out[2], ref[2])
        ran += 1
        if i % 3:
            continue
        act = ("relu", "hardswish")[(i // 3) % 2]
        for training in (True, False):
            ref, run = _bndw_case(2, 3, H, W, K, S, act, training, gen, BN_SPREAD if training else BN_SPREAD_EVAL, BN_MEAN)
            out = run()
            for name, b in ref.items():
                _cmp(fails, f"bn_{tag} {act} training={training}", name, out[name], b, maxnorm=name in ("y", "dz"),
                     tol=1e-5 if name.startswith("running") else TOL)
            fused += 1
    assert fused == 2 * 146
    _report(fails, ran, len(DW_H) * len(DW_W))


@gpu
def test_stem_conv_residue_sweep():
    """K9 forward and weight gradient on 12 x 28 = 336 images (B = 2)."""
    from cabinet_amd.functional import stem_conv, stem_conv_supported

    gen = torch.Generator().manual_seed(9000)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    wo = conv.weight.detach().double().requires_grad_(True)
    conv = conv.cuda()
    assert stem_conv_supported(conv)
    fails, ran = [], 0
    for H, W in itertools.product(C3_H, C3_W):
        x = torch.randn(2, 3, H, W, generator=gen)
        yo = F.conv2d(x.double(), wo, None, 2, 3)
        g = torch.randn(yo.shape, generator=gen)
        wo.grad = None
        yo.backward(g.double())
        conv.zero_grad()
        y = stem_conv(x.cuda(), conv)
        y.backward(g.cuda())
        _cmp(fails, f"stem {H}x{W}", "y", y, yo, maxnorm=True)
        _cmp(fails, f"stem {H}x{W}", "dw", conv.weight.grad, wo.grad)
        ran += 1
    _report(fails, ran, len(C3_H) * len(C3_W))


@pytest.fixture(scope="module")
def conv3x3s2_64_sweep():
    """Both 64 -> 64 kernels of K15 on the 336 planes against one fp64 backward per plane: {"dw": misses, "dx": misses, "ran": n}."""
    res = {"dw": [], "dx": [], "ran": 0}
    for H, W in itertools.product(C3_H, C3_W):
        x, w, g, dw_ref, dx_ref = t_c3._inputs(2, 64, 64, H, W, 3, 2, 1)
        xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
        _cmp(res["dw"], f"conv3x3s2 64->64 {H}x{W}", "dw", t_c3._native_dw(gd, xd, 64, 64), dw_ref, atol=0.0)
        _cmp(res["dx"], f"conv3x3s2 64->64 {H}x{W}", "dx", t_c3._native_dx(gd, wd, 2, H, W), dx_ref, maxnorm=True, atol=0.0)
        res["ran"] += 1
    return res


@gpu
def test_conv3x3s2_wgrad64_residue_sweep(conv3x3s2_64_sweep):
    """K15 64 -> 64 weight gradient on 12 x 28 = 336 planes (B = 2), NaN-prefilled."""
    _report(conv3x3s2_64_sweep["dw"], conv3x3s2_64_sweep["ran"], len(C3_H) * len(C3_W))


@gpu
def test_conv3x3s2_dgrad64_residue_sweep(conv3x3s2_64_sweep):
    """K15 64 -> 64 data gradient on the same planes, NaN-prefilled: every pixel is written, none is wrong."""
    _report(conv3x3s2_64_sweep["dx"], conv3x3s2_64_sweep["ran"], len(C3_H) * len(C3_W))


@gpu
def test_conv3x3s2_wgrad_3_16_residue_sweep():
    """K15 3 -> 16 weight gradient on the 336 planes (B = 2), NaN-prefilled."""
    fails, ran = [], 0
    for H, W in itertools.product(C3_H, C3_W):
        x, w, g, ref, _ = t_c3._inputs(2, 3, 16, H, W, 3, 2, 1)
        _cmp(fails, f"conv3x3s2 3->16 {H}x{W}", "dw", t_c3._native_dw(g.cuda(), x.cuda(), 3, 16), ref, atol=0.0)
        ran += 1
    _report(fails, ran, len(C3_H) * len(C3_W))


@gpu
@pytest.mark.parametrize("Ci,Co", [(8, 8), (16, 40), (72, 24), (104, 56)])
def test_pwconv_residue_sweep(Ci, Co):
    """K10 on planes of 1..200 pixels, B = 1 and 3: y, dx, dw through the C ABI, NaN-prefilled."""
    gen = torch.Generator().manual_seed(10000 + Ci * 200 + Co)
    fails, ran = [], 0
    for P, B in itertools.product(PW_P, (1, 3)):
        x, w, g = torch.randn(B, Ci, P, generator=gen), torch.randn(Co, Ci, generator=gen), torch.randn(B, Co, P, generator=gen)
        ref = _pw_ref(x, w, g)
        out = _pw_direct(x.cuda(), w.cuda(), g.cuda())
        tag = f"pwconv {Ci}->{Co} B={B} P={P}"
        _cmp(fails, tag, "y", out[0], ref[0], maxnorm=True, atol=0.0)
        _cmp(fails, tag, "dx", out[1], ref[1], maxnorm=True, atol=0.0)
        _cmp(fails, tag, "dw", out[2], ref[2], atol=0.0)
        ran += 1
    _report(fails, ran, len(PW_P) * 2)


@gpu
@pytest.mark.parametrize("Ci,Co", [(8, 8), (40, 120), (200, 80)])
def test_pwconv_wide_residue_sweep(Ci, Co):
    """K14 on planes of 1..200 pixels, B = 1 and 3, NaN-prefilled."""
    gen = torch.Generator().manual_seed(14000 + Ci * 200 + Co)
    fails, ran = [], 0
    for P, B in itertools.product(PW_P, (1, 3)):
        x, g = torch.randn(B, Ci, 1, P, generator=gen), torch.randn(B, Co, 1, P, generator=gen)
        ref = torch.einsum("bop,bcp->oc", g[:, :, 0].double(), x[:, :, 0].double())
        _cmp(fails, f"pwconv_wide {Ci}->{Co} B={B} P={P}", "dw", t_pww._native_dw(g.cuda(), x.cuda(), Ci, Co), ref, atol=0.0)
        ran += 1
    _report(fails, ran, len(PW_P) * 2)


def _bn_cases():
    """(P, B, act, training) of the K7 sweeps; B P = 1 in training mode has no batch statistics (the stock module rejects it)."""
    return [c for c in itertools.product(BN_P, (1, 3), ACTS, (True, False)) if not (c[0] * c[1] == 1 and c[3])]


@gpu
def test_bn_act_residue_sweep():
    """K7 on planes of 1..70, 8189..8195 and 16381..16387 pixels (one, two and three chunks; P % 4 of every kind), B = 1 and 3,
    C = 3, every activation, training and eval."""
    from cabinet_amd.functional import bn_act

    gen = torch.Generator().manual_seed(7700)
    bn0 = _set_bn(torch.nn.BatchNorm2d(3), gen)
    fails, ran, data = [], 0, {}
    for P, B, act, training in _bn_cases():
        if (P, B) not in data:
            data = {(P, B): (torch.randn(B, 3, 1, P, generator=gen), torch.randn(B, 3, 1, P, generator=gen))}
        x, g = data[(P, B)]
        spread = BN_SPREAD if training else BN_SPREAD_EVAL
        x = _clear_of_kinks(x * spread + BN_MEAN, _bn_pre(bn0, training), act, 0.37 * spread)
        ref = t_bn._oracle(x, g, bn0, act, training)
        bn = copy.deepcopy(bn0).cuda().train(training)
        xd = x.cuda().requires_grad_(True)
        y = bn_act(xd, bn, act)
        y.backward(g.cuda())
        tag = f"bn_act P={P} B={B} {act} training={training}"
        _cmp(fails, tag, "y", y, ref[0], maxnorm=True)
        _cmp(fails, tag, "dx", xd.grad, ref[1], maxnorm=True)
        _cmp(fails, tag, "dweight", bn.weight.grad, ref[2])
        _cmp(fails, tag, "dbias", bn.bias.grad, ref[3])
        _cmp(fails, tag, "running_mean", bn.running_mean, ref[4], tol=1e-5)
        _cmp(fails, tag, "running_var", bn.running_var, ref[5], tol=1e-5)
        if int(bn.num_batches_tracked) != int(training):
            fails.append(f"{tag}: num_batches_tracked {int(bn.num_batches_tracked)}")
        ran += 1
    _report(fails, ran, len(BN_P) * 2 * 3 * 2 - 3)


@gpu
def test_gate_act_residue_sweep():
    """gate_act on the same planes, B = 1 and 3, C = 3, every activation."""
    from cabinet_amd.functional import gate_act
    from oracle.model_ref import _hswish

    gen = torch.Generator().manual_seed(7800)
    fails, ran = [], 0
    for P, B in itertools.product(BN_P, (1, 3)):
        x, gate, g = torch.randn(B, 3, 1, P, generator=gen) * 2, torch.rand(B, 3, generator=gen), torch.randn(B, 3, 1, P, generator=gen)
        for act in ACTS:
            x = _clear_of_kinks(x.clone(), lambda t: t * gate.double()[:, :, None, None], act, 0.37)
            xo, go = x.double().requires_grad_(True), gate.double().requires_grad_(True)
            yo = {"relu": F.relu, "hardswish": _hswish, None: lambda t: t}[act](xo * go[:, :, None, None])
            yo.backward(g.double())
            xd, gd = x.cuda().requires_grad_(True), gate.cuda().requires_grad_(True)
            y = gate_act(xd, gd, act)
            y.backward(g.cuda())
            tag = f"gate_act P={P} B={B} {act}"
            _cmp(fails, tag, "y", y, yo, maxnorm=True)
            _cmp(fails, tag, "dx", xd.grad, xo.grad, maxnorm=True)
            _cmp(fails, tag, "dgate", gd.grad, go.grad)
            ran += 1
    _report(fails, ran, len(BN_P) * 2 * 3)


@gpu
def test_se_tail_residue_sweep():
    """se_tail (BatchNorm -> SELayer -> act) on the same planes against the stock modules in fp64: y, dz, the BatchNorm's and
    the SE MLP's parameter gradients, the running buffers."""
    from cabinet_amd.functional import se_tail
    from cabinet_amd.models.mobilenetv3 import HardSwish, SELayer

    gen = torch.Generator().manual_seed(7900)
    bn0, se0 = _set_bn(torch.nn.BatchNorm2d(3), gen), SELayer(3)
    with torch.no_grad():
        for m in (se0.fc[0], se0.fc[2]):  # as tests/test_gpu_se_tail.py: the gate spread over the whole hard-sigmoid range
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (3.0 / m.in_features ** 0.5))
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen))
    fails, ran, data = [], 0, {}
    for P, B, act, training in _bn_cases():
        if (P, B) not in data:
            data = {(P, B): (torch.randn(B, 3, 1, P, generator=gen), torch.randn(B, 3, 1, P, generator=gen))}
        z, g = data[(P, B)]
        spread = BN_SPREAD if training else BN_SPREAD_EVAL
        tail = {"relu": torch.nn.ReLU(), "hardswish": HardSwish(), None: torch.nn.Identity()}[act]
        mods = torch.nn.ModuleList([copy.deepcopy(bn0), copy.deepcopy(se0), tail]).train(training)
        ref = copy.deepcopy(mods).double()
        probe = copy.deepcopy(ref)  # its running buffers move with every call; those of ref do not

        def pre(t):
            """The value whose distance to a kink counts.  ReLU: gate >= 0, so the sign of gate * bn(z) is that of bn(z); where the
            gate is exactly 0 (the hard sigmoid's lower clamp) the product is 0 in every precision and there is no side to miss."""
            with torch.no_grad():
                u = probe[0](t)
                gt = probe[1].gate(u).view(B, 3, 1, 1)
                return torch.where(gt > 0, u, torch.full_like(u, float("nan"))) if act == "relu" else u * gt

        z = _clear_of_kinks(z * spread + BN_MEAN, pre, act, 0.37 * spread)
        zo = z.double().requires_grad_(True)
        yo = zo
        for m in ref:
            yo = m(yo)
        yo.backward(g.double())
        dev = mods.cuda()
        zd = z.cuda().requires_grad_(True)
        y = se_tail(zd, dev[0], dev[1], act)
        y.backward(g.cuda())
        tag = f"se_tail P={P} B={B} {act} training={training}"
        _cmp(fails, tag, "y", y, yo, maxnorm=True)
        _cmp(fails, tag, "dz", zd.grad, zo.grad, maxnorm=True)
        for (k, p), (_, q) in zip(dev.named_parameters(), ref.named_parameters()):
            _cmp(fails, tag, k, p.grad, q.grad)
        for (k, p), (_, q) in zip(dev.named_buffers(), ref.named_buffers()):
            if p.is_floating_point():
                _cmp(fails, tag, k, p, q, tol=1e-5)
            elif int(p) != int(q):
                fails.append(f"{tag} {k}: {int(p)} vs {int(q)}")
        ran += 1
    _report(fails, ran, len(BN_P) * 2 * 3 * 2 - 3)


# ------------------------------------------------------------------------------------------------ 4. caller contract
def _contract_bn_act():
    from cabinet_amd.functional import bn_act

    bn = _set_bn(torch.nn.BatchNorm2d(5), torch.Generator().manual_seed(1)).cuda().train()
    return (lambda x: bn_act(x, bn, "relu")), list(bn.parameters()), [bn.running_mean, bn.running_var]


def _contract_gate_act():
    from cabinet_amd.functional import gate_act

    gate = torch.rand(2, 5, generator=torch.Generator().manual_seed(2)).cuda().requires_grad_(True)
    return (lambda x: gate_act(x, gate, "hardswish")), [gate], []


def _contract_se_tail():
    from cabinet_amd.functional import se_tail
    from cabinet_amd.models.mobilenetv3 import SELayer

    torch.manual_seed(3)
    bn, se = _set_bn(torch.nn.BatchNorm2d(8), torch.Generator().manual_seed(3)).cuda().train(), SELayer(8).cuda()
    return (lambda x: se_tail(x, bn, se, "hardswish")), list(bn.parameters()) + list(se.parameters()), [bn.running_mean, bn.running_var]


def _contract_dwconv():
    from cabinet_amd.functional import dwconv

    torch.manual_seed(4)
    conv = torch.nn.Conv2d(4, 4, 3, 2, 1, groups=4, bias=False).cuda()
    return (lambda x: dwconv(x, conv)), [conv.weight], []


def _contract_bn_act_dwconv():
    from cabinet_amd.functional import bn_act_dwconv

    torch.manual_seed(5)
    conv = torch.nn.Conv2d(4, 4, 5, 1, 2, groups=4, bias=False).cuda()
    bn = _set_bn(torch.nn.BatchNorm2d(4), torch.Generator().manual_seed(5)).cuda().train()
    return (lambda x: bn_act_dwconv(x, bn, "relu", conv)), [conv.weight] + list(bn.parameters()), [bn.running_mean, bn.running_var]


def _contract_stem_conv():
    from cabinet_amd.functional import stem_conv

    torch.manual_seed(6)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False).cuda()
    return (lambda x: stem_conv(x, conv)), [conv.weight], []


def _contract_pwconv():
    from cabinet_amd.functional import pwconv

    torch.manual_seed(7)
    conv = torch.nn.Conv2d(16, 24, 1, bias=False).cuda()
    return (lambda x: pwconv(x, conv)), [conv.weight], []


def _contract_pwconv_wide():
    from cabinet_amd.functional import pwconv_wide, pwconv_wide_supported

    torch.manual_seed(8)
    conv = torch.nn.Conv2d(40, 24, 1, bias=False).cuda()

    def fn(x):
        assert pwconv_wide_supported(conv, x)
        return pwconv_wide(x, conv)

    return fn, [conv.weight], []


def _contract_conv2d_s2():
    from cabinet_amd.functional import Conv2dS2

    torch.manual_seed(9)
    conv = Conv2dS2(64, 64, 3, 2, 1, bias=False).cuda()

    def fn(x):
        y = conv(x)
        assert type(y.grad_fn).__name__ == "_Conv3x3S2Backward"
        return y

    return fn, [conv.weight], []


CONTRACT = {"bn_act": (_contract_bn_act, (2, 5, 7, 9)), "gate_act": (_contract_gate_act, (2, 5, 7, 9)),
            "se_tail": (_contract_se_tail, (2, 8, 7, 9)), "dwconv": (_contract_dwconv, (2, 4, 9, 11)),
            "bn_act_dwconv": (_contract_bn_act_dwconv, (2, 4, 9, 11)), "stem_conv": (_contract_stem_conv, (2, 3, 12, 14)),
            "pwconv": (_contract_pwconv, (2, 16, 5, 7)), "pwconv_wide": (_contract_pwconv_wide, (2, 40, 5, 7)),
            "Conv2dS2": (_contract_conv2d_s2, (2, 64, 6, 10))}


@gpu
@pytest.mark.parametrize("name", list(CONTRACT))
def test_backbone_wrappers_accept_any_layout(name):
    """A channels_last input, an input that starts 4 bytes into its storage, a non-contiguous output gradient (backward through a
    transposed view) and a stride-0 one (y.sum().backward()): the wrappers copy such operands and the kernels are
    bit-reproducible, so outputs, gradients and running buffers are bit for bit those of the dense, aligned call."""
    build, shape = CONTRACT[name]
    gen = torch.Generator().manual_seed(40)
    x = (torch.randn(*shape, generator=gen) * 1.3 + 0.2).cuda()
    x_cl = x.contiguous(memory_format=torch.channels_last)
    x_off = torch.empty(x.numel() + 1, device="cuda")[1:].view(shape).copy_(x)
    assert not x_cl.is_contiguous() and x_off.is_contiguous() and x_off.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    assert torch.equal(x_cl, x) and torch.equal(x_off, x)
    g = None

    def run(xv, mode):
        nonlocal g
        fn, params, buffers = build()  # fresh, identically seeded parameters and running buffers
        xv = xv.detach().requires_grad_(True)
        y = fn(xv)
        if g is None:
            g = torch.randn(y.shape, generator=gen).cuda()
        if mode == "dense":
            y.backward(g)
        elif mode == "transposed":
            y.transpose(2, 3).backward(g.transpose(2, 3).contiguous())  # y receives a transposed view: not contiguous
        elif mode == "ones":
            y.backward(torch.ones_like(y))
        else:
            y.sum().backward()  # y receives an expanded scalar: every stride 0
        assert xv.grad is not None and all(p.grad is not None for p in params)
        return [y.detach(), xv.grad] + [p.grad for p in params] + [b.clone() for b in buffers]

    base = run(x, "dense")
    for what, got in (("channels_last input", run(x_cl, "dense")), ("input 4 bytes into its storage", run(x_off, "dense")),
                      ("non-contiguous grad_output", run(x, "transposed"))):
        bad = [i for i, (a, b) in enumerate(zip(got, base)) if not torch.equal(a, b)]
        assert len(got) == len(base) and not bad, f"{name}, {what}: tensors {bad} differ from the dense, aligned call"
    ones, summed = run(x, "ones"), run(x, "sum")
    bad = [i for i, (a, b) in enumerate(zip(summed, ones)) if not torch.equal(a, b)]
    assert not bad, f"{name}, stride-0 grad_output: tensors {bad} differ from the dense call"
