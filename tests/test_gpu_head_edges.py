"""Head kernels (K11 Winograd 3x3 convolution, K12 BatchNorm + ReLU + classifier, K5 CAB local branch, K6 q/k/v producers and the
plain 1x1 convolution) where their host-side launch plans branch and where their tiles end -- every case through the C ABI or the
public wrapper, against the fp64 CPU oracle of the kernel's own test file.

1. Plan-branch cases: one shape per branch of a launch plan that no other operator test reaches (`wino_conv_kernel<false, 2>`,
   weight-gradient ranges of several chunks, K11's own routing rules either side of their thresholds, the big-plane path of
   `conv1x1`, the tiled K5 form on small planes in large batches, the combinations of K6's three predicates, `sd_plan`'s corners,
   more than 256 ragged tile-block partials into K7 / K12).  Criteria as in the per-kernel files: per tensor
   ||a-b|| <= 1e-3 ||b||, the tighter bound the file asserts (1e-5 for K11, 2e-5 for y / dw_cls of K12, 1e-5 for running
   statistics), two runs bit-equal, the 2x-stock bound for the big-plane `conv1x1` (both distances printed), NaN-prefilled outputs
   for the kernels that are called directly.
2. `test_head_plan_cases_reach_their_branches` (no GPU): reads every plan back through the library's queries, or restates the host
   rule where no query exists, and asserts that the shapes of part 1 are what they claim.  A retuned plan constant turns it red
   instead of letting the coverage lapse.
3. Dense residue sweeps: every (H, W) / P of a grid around the tile sizes, all failing shapes collected into one message, the
   number of shapes run asserted.  Per tensor the 1e-3 rule; for the maps also max|a-b| <= 1e-3 max|b|.
4. Caller contract of the head wrappers: channels_last (3-D: transposed) inputs, inputs 4 bytes into their storage,
   non-contiguous and stride-0 output gradients give bit for bit the results of the dense, aligned call.
"""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_bn_cls as t_cls
import test_gpu_conv3x3 as t_k11
import test_gpu_local as t_loc
import test_gpu_qkv as t_qkv
from conftest import assert_close, rel_err
from test_gpu_backbone_edges import _all_equal, _bn_pre, _clear_of_kinks, _cmp, _report, _set_bn

gpu = pytest.mark.gpu
TOL = 1e-3  # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32; the sweeps apply the same 1e-3 in the max norm to the maps

# ------------------------------------------------------------------------------------------------ the plan-branch table
# K11 (B, C0, C1, K, H, W) -> the kernel of the forward, of the data gradient, weight-gradient (chunks, ranges); see _wino_route
K11_CASES = {
    "odd-243-blocks": ((3, 64, 0, 64, 33, 257), "odd2", "odd2", (867, 256)),        # three or four chunks per range, ranges cross images
    "odd-fwd2-dgrad1": ((2, 64, 0, 128, 29, 225), "odd2", "odd1", (450, 128)),
    "odd-two-inputs": ((2, 64, 64, 64, 29, 225), "odd1", "odd2", (450, 128)),       # dx0 and dx1 from <false, 2>
    "even-K192": ((1, 64, 0, 192, 36, 256), "pair2", "pair1", (288, 85)),           # <true, 2> because K % 128 != 0, 72 x 3 blocks
    "small-at-200": ((8, 64, 0, 64, 20, 160), "pair1", "pair1", (800, 256)),        # ntb * nkb = 200: 32-channel blocks
    "small-at-225": ((9, 64, 0, 64, 20, 160), "pair2", "pair2", (900, 256)),        # the next reachable value: 64-channel blocks
    "k128-at-511": ((511, 64, 0, 128, 2, 30), "pair2", "pair2", (1022, 128)),       # wgs = 511: 64-channel blocks
    "k128-at-512": ((512, 64, 0, 128, 2, 30), "k128", "pair2", (1024, 128)),        # wgs = 512: the 128-channel kernel by its own rule
    "nsplit-272-units": ((1, 1088, 0, 1024, 2, 2), "pair1", "pair1", (1, 1)),       # units > 256: two rounds, one range per unit
    "nsplit-272-units-2-chunks": ((1, 1088, 0, 1024, 4, 4), "pair1", "pair1", (2, 1)),   # ... with two chunks: the rule itself, not the cut
    "nsplit-cut-to-chunks": ((1, 64, 0, 64, 5, 9), "odd1", "odd1", (3, 3)),         # 256 ranges wanted, three chunks there
}
K11_K128_RULE = (128, 64, 64, 256, 3, 34)    # two inputs, 256 ragged tile blocks (3 of 4 rows, 2 of 32 columns) x 2 = 512 workgroups
# conv1x1 (B, Ci, Co, H, W) -> ceil(P / 128) * B * ceil(max(Ci, Co) / 128); >= 400 is the big-plane path (cab_qkv.hip:894-896)
C1_CASES = [((4, 24, 72, 101, 127), 404), ((4, 24, 72, 100, 127), 400), ((2, 128, 256, 100, 128), 400), ((4, 24, 72, 99, 128), 396)]
# K5 (B, C, H, W) -> form, (TR, tiles per plane) of the tiled form
K5_CASES = {
    (2, 3, 64, 32): ("resident", None), (4, 3, 32, 64): ("resident", None),          # n == 2 * LOC_T: cab_local_*_kernel<2>
    (3, 3, 32, 32): ("resident", None), (7, 3, 32, 32): ("resident", None),          # n == LOC_T, odd B: <1>
    (512, 2, 4, 4): ("tiled", (4, 1)), (2048, 2, 1, 3): ("tiled", (1, 1)),           # B*H*W <= 8192, local_lds_bwd > 160 KB
    (5, 2, 2100, 1): ("tiled", (2100, 1)),                                          # W = 1
    (1, 2, 5, 2049): ("tiled", (1, 5)),                                             # TR = 1
    (1, 2, 129, 64): ("tiled", (64, 3)),                                            # the last tile is one row
}
# (B, C, H, W, training) -> seed where the default (3) leaves a ReLU input within 2e-6 of zero in the fp64 oracle (checked on the CPU)
K5_SEEDS = {(7, 3, 32, 32, False): 4, (512, 2, 4, 4, False): 5, (2048, 2, 1, 3, False): 4, (1, 2, 129, 64, False): 4}
# K6 (B, C, Kc, Vc, H, W, sizes) -> (BatchNorm partials in the GEMM's epilogue, one-kernel output stage, LDS-free dx); see _qkv_plan
K6_CASES = [
    ((2, 64, 64, 64, 8, 8, (1, 3, 6, 8)), (True, False, False)),      # P % 64 == 0, P % 256 != 0
    ((1, 64, 64, 64, 8, 24, (1, 3, 6, 8)), (True, False, False)),
    ((2, 48, 64, 64, 16, 16, (1, 3, 6, 8)), (False, True, False)),    # P % 256 == 0, C % 32 != 0
    ((2, 64, 64, 64, 16, 16, (1, 9)), (True, False, True)),           # s^2 = 81 > 64
    ((2, 32, 32, 48, 6, 10, (1, 3)), (False, False, False)),          # Kc != Vc, P % 64 != 0
    ((2, 32, 32, 32, 16, 16, (1, 3, 6, 8)), (False, False, True)),    # P % 256 == 0, Kc % 64 != 0: only the LDS-free dx
]
# conv1x1_bwd on the small path (B, Ci, Co, H, W) -> sd_plan's (total chunks, chunks per split, splits); see _sd_plan
SD_CASES = [((1, 16, 32, 5, 7), (2, 2, 1)), ((3, 16, 32, 8, 25), (21, 7, 3)), ((4, 16, 32, 64, 64), (512, 8, 64)),
            ((2, 24, 72, 25, 32), (50, 8, 7))]
# K11's partials into K12 and K7: 324 tile blocks (> 256: second trip of `t += BA_T`), ragged in both directions (count_of)
PART_CLS = (4, 64, 0, 64, 34, 258)
PART_BN = (4, 64, 0, 64, 33, 257)


def _a256(n):
    return (n + 255) // 256 * 256


def _th(n):
    return (n + 1) // 2


def _tile_blocks(B, H, W):
    """conv3x3_tile_blocks (conv3x3_wino.hip:1032): blocks of 2 x 16 Winograd tiles = 4 x 32 pixels."""
    return B * ((_th(H) + 1) // 2) * ((_th(W) + 15) // 16)


def _wino_route(ntb, Kout, K0, W):
    """wino_conv_run (conv3x3_wino.hip:1041-1082) with CABINET_WINO_128 unset and 8-byte aligned operands; the data
    gradient calls it with Kout = C0 + C1 and K0 = C0 (conv3x3_dgrad_run, :1102)."""
    if W % 2 == 0 and Kout % 128 == 0 and K0 % 64 == 0 and ntb * (Kout // 128) >= 512:   # :1055-1057
        return "k128"
    small = ntb * (Kout // 64) <= 200                                                    # :1066
    return ("pair" if W % 2 == 0 else "odd") + ("1" if small else "2")                   # :1050, :1076-1079


def _wgrad_plan(B, C, K, H, W):
    """wino_wgrad_nchunks / wino_wgrad_nsplit (conv3x3_wino.hip:1108-1114): chunks of 8 tiles of one tile row."""
    nchunks = B * _th(H) * ((_th(W) + 7) // 8)
    units = (K // 64) * (C // 64)
    ns = max(1, 256 * (-(-units // 256)) // units)
    return nchunks, min(ns, nchunks)


def _conv1x1_product(B, Ci, Co, P):
    """conv1x1_small (cab_qkv.hip:894-896): the small-tile path below 400."""
    return -(-P // 128) * B * -(-max(Ci, Co) // 128)


def _k16(n):
    return (n + 15) // 16 * 16


def _sd_plan(B, M, N, P):
    """sd_plan of small_gemm.hip:506-535 for ONE job (tiles_total = its own tiles) -> (total chunks, chunks per split, splits)."""
    tiles = -(-M // 64) * -(-N // 64)
    total = B * -(-P // 32)
    nsplit = max(1, min(-(-total // 8), -(-1024 // tiles), 64))
    cps = -(-total // nsplit)
    return total, cps, -(-total // cps)


def _dw_nsplit(B, Co, Ci, P):
    """dw_nsplit / dw_part_floats of ffm.hip:535-539, :1399-1402 (the big-plane weight gradient's slabs)."""
    return min(-(-768 // (-(-Co // 128) * -(-Ci // 128))), B * -(-P // 32), 128)


def _tiled_geom(B, H, W):
    """tiled_geom of cab_local_tiled.hip:28-37 -> (TR, tiles per plane, workgroups per channel)."""
    TR = min(max(4096 // W, 1), H)
    nT = -(-H // TR)
    return TR, nT, B * nT


def _local_lds_bwd(B, H, W):
    """local_lds_bwd of cab_local.hip:354-356, LOC_T = 1024."""
    return (4 * B * (H + 2) * (W + 2) + 2 + 4 * 16 + 9 * 16 + 16) * 4


def _qkv_plan(B, C, Kc, Vc, H, W, sizes):
    """The three independent predicates of K6 for training mode and 16-byte aligned operands."""
    P = H * W
    # sg_gemm (small_gemm.hip:350-375) returns `fast` for the three projection jobs: whole 64 x 64 tiles and whole 32-deep chunks;
    # qkv_fwd_run (cab_qkv.hip:742-746) then takes the BatchNorm partials from the GEMM's epilogue
    stats_in_gemm = P % 4 == 0 and Kc % 64 == 0 and Vc % 64 == 0 and P % 64 == 0 and C % 32 == 0 and C % 4 == 0
    # qkv_fused_fwd_supported (cab_qkv_fused.hip:259-266); the LDS bound does not bind at these sizes
    fused = Kc % 32 == 0 and Vc % 32 == 0 and P % 256 == 0 and Kc == Vc and Kc in (64, 128, 256) and all(s * s <= 64 for s in sizes)
    # qkv_dx_supported (cab_qkv_fused.hip:280-283)
    dx = C % 32 == 0 and Kc % 32 == 0 and Vc % 32 == 0 and P % 256 == 0 and B * (2 * Kc + Vc) * P < (1 << 29)
    return stats_in_gemm, fused, dx


def test_head_plan_cases_reach_their_branches():
    """Every row of the table above reaches the branch it is there for, read back from the library's own plans where it has a
    query and from the restated host rule where it has none."""
    from cabinet_amd import _lib
    from cabinet_amd.functional import _sizes_arg

    lib = _lib.load()
    # K11: tile blocks and weight-gradient ranges from the library, the routing from the restated rule
    for name, (shape, fwd, dgrad, (nchunks, nsplit)) in K11_CASES.items():
        B, C0, C1, K, H, W = shape
        C = C0 + C1
        assert lib.cabinet_conv3x3_supported(C0, C1, K) == 1, name
        ntb = lib.cabinet_conv3x3_tile_blocks(B, H, W)
        assert ntb == _tile_blocks(B, H, W), name
        slabs = lib.cabinet_conv3x3_bwd_workspace_bytes(*shape) - lib.cabinet_conv3x3_fwd_workspace_bytes(*shape)
        assert slabs == nsplit * K * C * 9 * 4 and _wgrad_plan(B, C, K, H, W) == (nchunks, nsplit), (name, slabs, _wgrad_plan(B, C, K, H, W))
        assert (_wino_route(ntb, K, K, W), _wino_route(ntb, C, C0, W)) == (fwd, dgrad), name
    ntb = {n: _tile_blocks(s[0], s[4], s[5]) for n, (s, *_) in K11_CASES.items()}
    assert ntb["odd-243-blocks"] == 243 and ntb["odd-fwd2-dgrad1"] == 128 and ntb["even-K192"] == 72
    assert (ntb["small-at-200"], ntb["small-at-225"]) == (200, 225) and (ntb["k128-at-511"], ntb["k128-at-512"]) == (511, 512)
    assert (1024 // 64) * (1088 // 64) == 272                                   # units of "nsplit-272-units"
    for s in t_k11.SHAPES:   # what the per-kernel file runs at odd W: one chunk per range
        nchunks, nsplit = _wgrad_plan(s[0], s[1] + s[2], s[3], s[4], s[5])
        assert s[5] % 2 == 0 or nchunks == nsplit, s
    B, C0, C1, K, H, W = K11_K128_RULE
    ntb_r = lib.cabinet_conv3x3_tile_blocks(B, H, W)
    assert ntb_r == 256 and _wino_route(ntb_r, K, K, W) == "k128" and H % 4 and W % 32 and C1
    # conv1x1: cabinet_conv1x1_bias_supported IS conv1x1_small; the workspace of the big path holds its slabs and the padded weight
    for (B, Ci, Co, H, W), prod in C1_CASES:
        P = H * W
        assert _conv1x1_product(B, Ci, Co, P) == prod
        assert lib.cabinet_conv1x1_bias_supported(B, Ci, Co, P) == (1 if prod < 400 else 0)
        big = _a256(_dw_nsplit(B, Co, Ci, P) * Co * Ci * 4) + (_a256(_k16(Co) * Ci * 4) if Co % 16 else 0)
        total, cps, ns = _sd_plan(B, Co, Ci, P)
        small = _a256(_a256(-(-ns * Co * Ci // 64) * 64 * 4))
        assert lib.cabinet_conv1x1_bwd_workspace_bytes(B, Ci, Co, P) == max(small, big)
        assert lib.cabinet_conv1x1_fwd_workspace_bytes(Ci, Co) == _a256(_k16(Ci) * Co * 4)
    assert (101 * 127) % 2 == 1 and (100 * 127) % 4 == 0 and 24 % 16 and 72 % 16 and not 128 % 16 and not 256 % 16
    for (B, Ci, Co, H, W), plan in SD_CASES:
        assert lib.cabinet_conv1x1_bias_supported(B, Ci, Co, H * W) == 1 and _sd_plan(B, Co, Ci, H * W) == plan
    (_, c0, n0), (_, c1, n1), (_, c2, n2), (t3, c3, n3) = (p for _, p in SD_CASES)
    assert n0 == 1 and n1 % 4 and n2 == 64 and n3 % 4 and c3 * n3 != t3
    # K5: a zero workspace is the resident form; the tiled form's workspace carries nblk partials per channel
    for (B, C, H, W), (form, geom) in K5_CASES.items():
        assert lib.cabinet_cab_local_supported(B, C, H, W) == 1
        ws = lib.cabinet_cab_local_bwd_workspace_bytes(B, C, H, W)
        if form == "resident":
            assert ws == 0 and lib.cabinet_cab_local_fwd_workspace_bytes(B, C, H, W) == 0 and H * W in (1024, 2048)
            continue
        TR, nT, nblk = _tiled_geom(B, H, W)
        n64 = -(-B * C * H * W // 64) * 64
        assert (TR, nT) == geom and ws == _a256(5 * n64 * 4 + C * nblk * 36 * 8)
        assert lib.cabinet_cab_local_fwd_workspace_bytes(B, C, H, W) == _a256(3 * n64 * 4 + 3 * C * nblk * 2 * 8)
    assert all(B * H * W <= 8192 and _local_lds_bwd(B, H, W) > 160 * 1024 for B, _, H, W in [(512, 2, 4, 4), (2048, 2, 1, 3)])
    assert 129 % 64 == 1 and _tiled_geom(512, 4, 4)[2] == 512 and _tiled_geom(2048, 1, 3)[2] == 2048
    # K6: supported, the statistics workspace counts 64-position tiles; the predicates from the restated rules
    seen = set()
    for (B, C, Kc, Vc, H, W, sizes), plan in K6_CASES:
        sz = _sizes_arg(sizes)
        assert lib.cabinet_cab_qkv_supported(B, C, Kc, Vc, H, W, len(sizes), sz) == 1
        nbp = lib.cabinet_cab_qkv_padded_bins(len(sizes), sz)
        assert nbp == -(-sum(s * s for s in sizes) // 4) * 4
        want = _a256(4 * Kc * B * -(-H * W // 64) * 4) + _a256(B * Kc * nbp * 4) + _a256(B * Vc * nbp * 4)
        assert lib.cabinet_cab_qkv_fwd_workspace_bytes(B, C, Kc, Vc, H, W, len(sizes), sz) == want
        assert _qkv_plan(B, C, Kc, Vc, H, W, sizes) == plan
        seen.add(plan)
    have = {_qkv_plan(*c[:7]) for c in [(2, 256, 128, 128, 16, 16, (1, 3, 6, 8)), (8, 256, 128, 128, 32, 32, (1, 3, 6, 8)),
                                         (1, 64, 32, 48, 5, 7, (1, 3, 6, 8)), (2, 32, 16, 16, 8, 20, (2, 5)),
                                         (1, 512, 256, 128, 32, 64, (1, 3, 6, 8)), (2, 256, 128, 128, 64, 32, (1, 3, 6, 8)),
                                         (3, 96, 64, 64, 16, 32, (2, 5)), (1, 320, 256, 256, 16, 16, (1, 3, 6, 8))]}   # test_gpu_qkv.py
    # (True, True, False) and (False, True, True) cannot occur: the one-kernel output stage with either of the others implies the third
    assert seen - have == {(True, False, False), (False, True, False), (False, False, True)} and len(seen | have) == 6
    # K11 partials -> K12 / K7: more than 256 tile blocks AND ragged ones
    for B, _, _, K, H, W in (PART_CLS, PART_BN):
        assert lib.cabinet_conv3x3_tile_blocks(B, H, W) == 324 > 256 and H % 4 and W % 32
    assert lib.cabinet_bn_cls_supported(64, 8, 34 * 258) == 1 and lib.cabinet_bn_cls_supported(64, 8, 33 * 257) == 0


# ------------------------------------------------------------------------------------------------ shared pieces
def _no_wino_env(monkeypatch):
    monkeypatch.delenv("CABINET_WINO_128", raising=False)


def _k11_dev(x0, x1, w, dy, with_part=False):
    """Forward (optionally with a NaN-prefilled statistics buffer) and backward of K11 through the C ABI wrappers."""
    from cabinet_amd.functional import conv3x3_bn_part, conv3x3_bwd_hip, conv3x3_fwd_hip

    d = lambda t: t.cuda() if t is not None else None  # noqa: E731
    part = conv3x3_bn_part(d(x0), w.shape[0]).fill_(float("nan")) if with_part else None
    y = conv3x3_fwd_hip(d(x0), d(x1), d(w), bn_part=part)
    dx0, dx1, dw = conv3x3_bwd_hip(d(dy), d(x0), d(x1), d(w))
    out = {"y": y, "dx0": dx0, "dw": dw}
    if x1 is not None:
        out["dx1"] = dx1
    if with_part:
        out["bn_part"] = part
    return out


def _k11_ref(x0, x1, w, dy):
    y, dx, dw = t_k11._oracle(x0, x1, w, dy)
    C0 = x0.shape[1]
    ref = {"y": y, "dx0": dx[:, :C0], "dw": dw}
    if x1 is not None:
        ref["dx1"] = dx[:, C0:]
    return ref


def _c1_direct(xd, wd, gd, need_dx=True, need_dw=True):
    """cabinet_conv1x1_fwd / _bwd on device tensors (B, Ci, H, W), (Co, Ci), (B, Co, H, W), every output NaN before the call."""
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    lib = _lib.load()
    B, Ci, P, Co = xd.shape[0], xd.shape[1], xd[0, 0].numel(), wd.shape[0]
    nan, st = float("nan"), _stream_handle(xd.device)
    y = torch.full_like(gd, nan)
    dx = torch.full_like(xd, nan) if need_dx else None
    dw = torch.full_like(wd, nan) if need_dw else None
    # the workspaces are NaN bit patterns before the calls: the K tail of the staged W^T and of the padded weight must be zeroed by
    # the library, whatever the allocator hands back
    ws, nbytes = _workspace(lib.cabinet_conv1x1_fwd_workspace_bytes(Ci, Co), xd.device)
    ws.fill_(255)
    _lib.check(lib.cabinet_conv1x1_fwd(_ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(y), _ptr(ws), nbytes, st), "cabinet_conv1x1_fwd")
    ws, nbytes = _workspace(lib.cabinet_conv1x1_bwd_workspace_bytes(B, Ci, Co, P), xd.device)
    ws.fill_(255)
    rc = lib.cabinet_conv1x1_bwd(_ptr(gd), _ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes, st)
    _lib.check(rc, "cabinet_conv1x1_bwd")
    return y, dx, dw


def _c1_case(B, Ci, Co, H, W, gen):
    x, w, g = torch.randn(B, Ci, H, W, generator=gen), torch.randn(Co, Ci, generator=gen) * Ci ** -0.5, torch.randn(B, Co, H, W, generator=gen)
    xo, wo, go = x.double(), w.double(), g.double()
    ref = (torch.einsum("oc,bchw->bohw", wo, xo), torch.einsum("oc,bohw->bchw", wo, go), torch.einsum("bohw,bchw->oc", go, xo))
    return x, w, g, ref


def _k5_case(B, C, H, W, training, with_glob, seed):
    """Inputs, the fp64 oracle (test_gpu_local._oracle) and the fragile-channel mask of one K5 case, all on the CPU."""
    m0 = t_loc._make(C, 7 + seed)
    gen = torch.Generator().manual_seed(1000 * seed + 17 * H + W + B)
    x, g = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    glob = torch.randn(B, C, H, W, generator=gen) if with_glob else None
    gamma = torch.tensor([0.37]) if with_glob else None
    out, dx, grads, bufs, extra = t_loc._oracle(m0, x, g, training, glob, gamma)
    ref = {"out": out, "dx": dx, **{f"grad {k}": v for k, v in grads.items()}, **{k: v for k, v in bufs.items()}}
    if with_glob:
        ref.update(dglob=extra["dglob"], dgamma=extra["dgamma"])
    return m0, x, g, glob, gamma, ref, t_loc._fragile_channels(m0, x, training)


def _k5_dev(m0, x, g, glob, gamma, training):
    from cabinet_amd.functional import cab_local

    m = copy.deepcopy(m0).cuda().train(training)
    xd = x.cuda().requires_grad_(True)
    gd, gm = (glob.cuda().requires_grad_(True), gamma.cuda().requires_grad_(True)) if glob is not None else (None, None)
    out = cab_local(xd, m.refine, gd, gm)
    out.backward(g.cuda())
    res = {"out": out.detach(), "dx": xd.grad, **{f"grad {k}": p.grad for k, p in m.named_parameters()},
           **{k: b.clone() for k, b in m.named_buffers()}}
    if glob is not None:
        res.update(dglob=gd.grad, dgamma=gm.grad)
    return res


def _k5_compare(fails, tag, res, ref, frag, maxnorm=True):
    """Per tensor the 1e-3 rule (running statistics 1e-5) on the channels without a fragile ReLU unit (test_gpu_local's rule)."""
    keep = ~frag
    for name, b in ref.items():
        a = res[name]
        if name.endswith("num_batches_tracked"):
            if int(a) != int(b):
                fails.append(f"{tag} {name}: {int(a)} vs {int(b)}")
            continue
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        if name == "dgamma":   # one scalar over every channel
            if bool(keep.all()):
                _cmp(fails, tag, name, a.reshape(-1), b.reshape(-1))
            continue
        dim = 1 if b.dim() == 4 and name in ("out", "dx", "dglob") else 0
        a, b = a.movedim(dim, 0)[keep], b.movedim(dim, 0)[keep]
        stat = "running" in name
        _cmp(fails, tag, name, a, b, maxnorm=maxnorm and b.dim() == 4 and not name.startswith("grad"), tol=1e-5 if stat else TOL)


def _qkv_dev(m0, x, grads, training):
    from cabinet_amd.functional import cab_qkv

    m = copy.deepcopy(m0).cuda().train(training)
    xd = x.cuda().requires_grad_(True)
    q, k, v = cab_qkv(xd, m)
    torch.autograd.backward([q, k, v], [g.cuda() for g in grads])
    named = {n: p.grad for n, p in m.named_parameters() if not n.startswith("project_out")}
    return m, {"q": q.detach(), "k": k.detach(), "v": v.detach(), "dx": xd.grad, **{f"grad {n}": t for n, t in named.items()}}


# ------------------------------------------------------------------------------------------------ 1. plan-branch cases
@gpu
@pytest.mark.parametrize("name", list(K11_CASES))
def test_conv3x3_plan_branches(name, monkeypatch):
    """K11 forward, data gradient and weight gradient by the library's own routing (CABINET_WINO_128 unset): `<false, 2>`, `<true, 2>`
    by K % 128 != 0, either side of ntb * nkb = 200 and of wgs = 512, weight-gradient ranges of several chunks, nsplit of 1 over
    272 units and nsplit cut to the chunk count.  1e-5 against the fp64 oracle, two runs bit-equal."""
    _no_wino_env(monkeypatch)
    shape = K11_CASES[name][0]
    x0, x1, w, dy = t_k11._case(*shape, seed=41)
    ref = _k11_ref(x0, x1, w, dy)
    runs = [_k11_dev(x0, x1, w, dy) for _ in range(2)]
    torch.cuda.synchronize()
    errs = {k: rel_err(runs[0][k], ref[k]) for k in ref}
    print(f"conv3x3 {name} {shape}: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0].values())
    assert all(e <= TOL for e in errs.values()), errs
    assert max(errs.values()) < 1e-5, errs
    assert _all_equal(list(runs[0].values()), list(runs[1].values()))


@gpu
def test_conv3x3_128_channel_kernel_by_its_own_rule_equals_64_channel_kernel(monkeypatch):
    """wino_conv128_kernel chosen by `wgs >= 512` (no environment switch) on two inputs and ragged tile blocks: 1e-5 against fp64,
    and outputs, gradients and BatchNorm partials bit for bit those of the 64-channel kernel (CABINET_WINO_128=0)."""
    _no_wino_env(monkeypatch)
    x0, x1, w, dy = t_k11._case(*K11_K128_RULE, seed=43)
    ref = _k11_ref(x0, x1, w, dy)
    own = [_k11_dev(x0, x1, w, dy, with_part=True) for _ in range(2)]
    monkeypatch.setenv("CABINET_WINO_128", "0")
    k64 = _k11_dev(x0, x1, w, dy, with_part=True)
    torch.cuda.synchronize()
    errs = {k: rel_err(own[0][k], ref[k]) for k in ref}
    print(f"conv3x3 128-channel rule {K11_K128_RULE}: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert bool(torch.isfinite(own[0]["bn_part"]).all())
    assert max(errs.values()) < 1e-5, errs
    assert _all_equal(list(own[0].values()), list(own[1].values()))
    for k in own[0]:
        assert torch.equal(own[0][k], k64[k]), f"{k}: the 128-channel kernel differs from the 64-channel kernel's bits (rel {rel_err(own[0][k], k64[k]):.2e})"


@gpu
@pytest.mark.parametrize("shape,prod", C1_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv1x1_big_plane_path(shape, prod):
    """`conv1x1` forward, dx and dw either side of the 400-workgroup bound: gemm_kmajor / dw_product of ffm.hip with the K tail of
    the staged W^T (Ci % 16) and the padded weight copy for dx (Co % 16), and the small-tile neighbour at 396.  The 1e-3 rule and
    distance to fp64 <= max(2 x the distance of torch's own fp32 convolution on the same device tensors, 1e-6); dx only and dw only
    give the bits of the full call; two runs bit-equal."""
    B, Ci, Co, H, W = shape
    x, w, g, ref = _c1_case(B, Ci, Co, H, W, torch.Generator().manual_seed(prod + Ci))
    xd, wd, gd = x.cuda(), w.cuda(), g.cuda()
    runs = [_c1_direct(xd, wd, gd) for _ in range(2)]
    only_dx, only_dw = _c1_direct(xd, wd, gd, need_dw=False), _c1_direct(xd, wd, gd, need_dx=False)
    xs, ws = xd.clone().requires_grad_(True), wd.clone().view(Co, Ci, 1, 1).requires_grad_(True)
    ys = F.conv2d(xs, ws)
    ys.backward(gd)
    torch.cuda.synchronize()
    stock = (ys.detach(), xs.grad, ws.grad.view(Co, Ci))
    fails = []
    for name, a, s, b in zip(("y", "dx", "dw"), runs[0], stock, ref):
        assert bool(torch.isfinite(a).all()), name
        e, e_stock = rel_err(a, b), rel_err(s, b)
        print(f"conv1x1 {shape} product {prod} {name}: native {e:.3e}  stock {e_stock:.3e}")
        if not e <= TOL:
            fails.append(f"{name}: {e:.3e} > {TOL}")
        if not e <= max(2.0 * e_stock, 1e-6):
            fails.append(f"{name}: native {e:.3e} > max(2 x stock {e_stock:.3e}, 1e-6)")
    assert not fails, fails
    assert _all_equal(runs[0], runs[1])
    assert only_dx[2] is None and only_dw[1] is None
    assert torch.equal(only_dx[1], runs[0][1]) and torch.equal(only_dw[2], runs[0][2])
    assert torch.equal(only_dx[0], runs[0][0]) and torch.equal(only_dw[0], runs[0][0])


@gpu
@pytest.mark.parametrize("shape,plan", SD_CASES, ids=lambda v: "x".join(map(str, v)))
def test_conv1x1_bwd_small_path_split_plans(shape, plan):
    """`sd_plan` through cabinet_conv1x1_bwd: one split, a split count that is no multiple of 4, the cap of 64, and a last split
    shorter than the others.  NaN-prefilled, 1e-3 and the 2e-5 the per-kernel file asserts on this path, bit-equal runs."""
    B, Ci, Co, H, W = shape
    x, w, g, ref = _c1_case(B, Ci, Co, H, W, torch.Generator().manual_seed(sum(plan)))
    xd, wd, gd = x.cuda(), w.cuda(), g.cuda()
    runs = [_c1_direct(xd, wd, gd) for _ in range(2)]
    torch.cuda.synchronize()
    for name, a, b in zip(("y", "dx", "dw"), runs[0], ref):
        assert bool(torch.isfinite(a).all()), name
        print(f"conv1x1 small {shape} splits {plan} {name}: {rel_err(a, b):.3e}")
        assert_close(a, b, TOL, name)
        assert_close(a, b, 2e-5, name)
    assert _all_equal(runs[0], runs[1])


@gpu
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_glob", [False, True])
@pytest.mark.parametrize("B,C,H,W", list(K5_CASES))
def test_cab_local_plan_branches(B, C, H, W, with_glob, training):
    """K5: the resident form's n == 2048 and n == 1024 specialisations, and the tiled form where LDS (not B*H*W) selects it, with
    W = 1, with TR = 1 and with a one-row last tile.  No ReLU input of the fp64 oracle lies within 2e-6 of zero (asserted), so every
    channel is held to 1e-3 (running statistics 1e-5); two runs bit-equal."""
    seed = K5_SEEDS.get((B, C, H, W, training), 3)
    m0, x, g, glob, gamma, ref, frag = _k5_case(B, C, H, W, training, with_glob, seed)
    assert not bool(frag.any()), f"seed {seed}: channels {frag.nonzero().flatten().tolist()} hold a ReLU input within 2e-6 of zero"
    runs = [_k5_dev(m0, x, g, glob, gamma, training) for _ in range(2)]
    torch.cuda.synchronize()
    fails = []
    _k5_compare(fails, f"cab_local {(B, C, H, W)} glob={with_glob} training={training}", runs[0], ref, frag, maxnorm=False)
    assert not fails, "\n".join(fails)
    assert list(runs[0]) == list(runs[1]) and _all_equal(list(runs[0].values()), list(runs[1].values()))


@gpu
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case,plan", K6_CASES, ids=lambda v: "-".join(map(str, v)).replace(" ", ""))
def test_qkv_predicate_combinations(case, plan, training):
    """K6 at the combinations of (statistics in the GEMM's epilogue, one-kernel output stage, LDS-free dx) that test_gpu_qkv.py has
    no shape for; criteria of that file (1e-3 per tensor, running statistics 1e-5), two runs bit-equal."""
    B, C, Kc, Vc, H, W, sizes = case
    m0 = t_qkv._make(C, Kc, Vc, sizes, 5)
    g0 = torch.Generator().manual_seed(19)
    x = torch.randn(B, C, H, W, generator=g0)
    grads = [torch.randn(B, ch, H * W, generator=g0) for ch in (Kc, Kc, Vc)]
    (oq, ok, ov), o_dx, o_grads, o_buf = t_qkv._oracle_qkv(m0, x, grads, training, sizes)
    (m, res), (m2, res2) = _qkv_dev(m0, x, grads, training), _qkv_dev(m0, x, grads, training)
    torch.cuda.synchronize()
    ref = {"q": oq, "k": ok, "v": ov, "dx": o_dx, **{n: o_grads[n[5:]] for n in res if n.startswith("grad ")}}
    for name, b in ref.items():
        print(f"qkv {case} {plan} training={training} {name}: {rel_err(res[name], b):.3e}")
        assert_close(res[name], b, TOL, name)
    for name, b in m.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(o_buf[name]), name
        else:
            assert_close(b, o_buf[name], 1e-5, name)
    assert _all_equal(list(res.values()), list(res2.values()))
    assert _all_equal([b for _, b in m.named_buffers()], [b for _, b in m2.named_buffers()])


@gpu
def test_conv3x3_partials_into_bn_relu_cls_more_than_256_ragged_blocks():
    """conv3x3 -> bn_relu_cls with 324 ragged tile-block partials (bn_finalize_channel's count_of on the second trip of its loops):
    against the chain with K12's own statistics pass (2e-5, test_gpu_bn_cls.py) and against fp64 BatchNorm -> ReLU -> classifier on
    the same z (2e-5 for y and dw_cls, 1e-3 for the rest, 1e-5 for the running statistics)."""
    from cabinet_amd.functional import bn_relu_cls, conv3x3, conv3x3_bn_part

    B, C0, _, Co, H, W = PART_CLS
    K = 8
    gen = torch.Generator().manual_seed(51)
    x0 = (torch.randn(B, C0, H, W, generator=gen) + 0.5).cuda()
    w3 = (torch.randn(Co, C0, 3, 3, generator=gen) * (9 * C0) ** -0.5).cuda()
    g = torch.randn(B, K, H, W, generator=gen).cuda()
    res, mods = [], []
    for with_part in (True, False, True):
        bn, cls = t_cls._modules(Co, K, True, torch.Generator().manual_seed(9))
        mods.append((copy.deepcopy(bn), copy.deepcopy(cls)))
        bn, cls = bn.cuda().train(), cls.cuda()
        part = conv3x3_bn_part(x0, Co).fill_(float("nan")) if with_part else None
        z = conv3x3(x0, w3, None, part).requires_grad_(True)
        y = bn_relu_cls(z, bn, cls, conv_part=part)
        assert type(y.grad_fn).__name__ == "_BnClsBackward"
        y.backward(g)
        res.append((y.detach(), z.grad, bn.weight.grad, bn.bias.grad, cls.weight.grad, cls.bias.grad, bn.running_mean, bn.running_var, z.detach()))
    torch.cuda.synchronize()
    names = ("y", "dz", "dgamma", "dbeta", "dw", "dbias", "running_mean", "running_var", "z")
    for name, a, b in zip(names, res[0], res[1]):
        assert rel_err(a, b) < 2e-5, (name, rel_err(a, b))
    assert _all_equal(res[0], res[2])
    ref = t_cls._oracle(res[0][8], g, *mods[0], True)
    for name, a, tol in (("y", 0, 2e-5), ("dz", 1, TOL), ("dgw", 2, TOL), ("dgb", 3, TOL), ("dw", 4, 2e-5), ("db", 5, 2e-5), ("rm", 6, 1e-5),
                         ("rv", 7, 1e-5)):
        print(f"conv3x3 -> bn_relu_cls {PART_CLS} {name}: {rel_err(res[0][a], ref[name]):.3e}")
        assert_close(res[0][a], ref[name], tol, name)


@gpu
def test_conv3x3_partials_into_bn_act_more_than_256_ragged_blocks():
    """conv3x3 -> bn_act(conv_part=) with 324 ragged tile-block partials (P odd): against bn_act with its own statistics pass (1e-6)
    and against torch's BatchNorm2d in fp64 (1e-5), the criteria of test_gpu_conv3x3.py's partials test."""
    from cabinet_amd.functional import bn_act, conv3x3, conv3x3_bn_part

    B, C, _, K, H, W = PART_BN
    x0, _, w, _ = t_k11._case(B, C, 0, K, H, W, seed=53)
    xd, wd = (x0 + 0.5).cuda(), w.cuda()
    outs = []
    for with_part in (True, False, True):
        bn = torch.nn.BatchNorm2d(K)
        _set_bn(bn, torch.Generator().manual_seed(5))
        bn0 = copy.deepcopy(bn)
        bn = bn.cuda().train()
        part = conv3x3_bn_part(xd, K).fill_(float("nan")) if with_part else None
        y = conv3x3(xd, wd, None, part)
        outs.append((bn_act(y, bn, "relu", conv_part=part), bn.running_mean, bn.running_var, y))
        assert int(bn.num_batches_tracked) == 1
    torch.cuda.synchronize()
    for name, a, b in zip(("out", "running_mean", "running_var"), outs[0], outs[1]):
        assert rel_err(a, b) < 1e-6, (name, rel_err(a, b))
    assert _all_equal(outs[0], outs[2])
    ref_bn = bn0.double().train()
    ref = torch.relu(ref_bn(outs[0][3].double().cpu()))
    print(f"conv3x3 -> bn_act {PART_BN}: out {rel_err(outs[0][0], ref):.3e}  running_var {rel_err(outs[0][2], ref_bn.running_var):.3e}")
    assert rel_err(outs[0][0], ref) < 1e-5
    assert rel_err(outs[0][1], ref_bn.running_mean) < 1e-5 and rel_err(outs[0][2], ref_bn.running_var) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. dense residue sweeps
K11_SWEEPS = {
    "1x64+0->64": ((1, 64, 0, 64), list(range(1, 11)), list(range(1, 37))),
    "2x64+64->64": ((2, 64, 64, 64), [1, 2, 3, 4, 5, 8, 9], [1, 2, 7, 8, 15, 16, 17, 18, 31, 32, 33, 34, 35, 36]),
    "1x64+0->128": ((1, 64, 0, 128), [1, 2, 3, 4, 5, 8, 9], [1, 2, 7, 8, 15, 16, 17, 18, 31, 32, 33, 34, 35, 36]),
}
CLS_P = list(range(4, 601, 4)) + [2052, 4100, 6148]   # BC_TPW = 2048 positions per wave of the reduce kernel
CLS_K = [1, 8, 9, 20, 21, 32]
TILED_W = [1, 2, 3, 63, 64, 65, 255, 257]
C1_SWEEP = [(16, 32), (24, 72)]


@gpu
@pytest.mark.parametrize("name", list(K11_SWEEPS))
def test_conv3x3_residue_sweep(name, monkeypatch):
    """K11 on every plane of a grid that covers both W parities, every residue of the 4 x 32 tile block and of the 8-tile (16-pixel)
    weight-gradient chunk: y, dx0 (dx1), dw."""
    _no_wino_env(monkeypatch)
    (B, C0, C1, K), hs, ws = K11_SWEEPS[name]
    fails, ran = [], 0
    for H, W in itertools.product(hs, ws):
        x0, x1, w, dy = t_k11._case(B, C0, C1, K, H, W, seed=61)
        ref, out = _k11_ref(x0, x1, w, dy), _k11_dev(x0, x1, w, dy)
        for k, b in ref.items():
            _cmp(fails, f"conv3x3 {name} {H}x{W}", k, out[k], b, maxnorm=k != "dw", atol=0.0)
        ran += 1
    _report(fails, ran, len(hs) * len(ws))


@gpu
@pytest.mark.parametrize("K", CLS_K)
def test_bn_relu_cls_residue_sweep(K):
    """K12 on planes of 4, 8, ..., 600 pixels and just above one, two and three 2048-position reduce tiles, B = 1 and 3, C = 64,
    training and eval alternating; inputs within 2e-4 of the ReLU kink are moved off it."""
    from cabinet_amd.functional import bn_relu_cls

    gen = torch.Generator().manual_seed(1200 + K)
    bn0, cls0 = t_cls._modules(64, K, K % 2 == 0, gen)
    fails, ran = [], 0
    for i, (P, B) in enumerate(itertools.product(CLS_P, (1, 3))):
        training = (i // 2 + i) % 2 == 0
        z = torch.randn(B, 64, 1, P, generator=gen) * 1.3 + 0.4
        z = _clear_of_kinks(z, _bn_pre(bn0, training), "relu", 0.37)
        g = torch.randn(B, K, 1, P, generator=gen)
        ref = t_cls._oracle(z, g, bn0, cls0, training)
        bn, cls = copy.deepcopy(bn0).cuda().train(training), copy.deepcopy(cls0).cuda()
        zd = z.cuda().requires_grad_(True)
        y = bn_relu_cls(zd, bn, cls)
        if type(y.grad_fn).__name__ != "_BnClsBackward":
            fails.append(f"P={P}: K12 did not take the shape")
        y.backward(g.cuda())
        tag = f"bn_relu_cls K={K} P={P} B={B} training={training}"
        _cmp(fails, tag, "y", y, ref["y"], maxnorm=True)
        _cmp(fails, tag, "dz", zd.grad, ref["dz"], maxnorm=True)
        _cmp(fails, tag, "dgamma", bn.weight.grad, ref["dgw"])
        _cmp(fails, tag, "dbeta", bn.bias.grad, ref["dgb"])
        _cmp(fails, tag, "dw_cls", cls.weight.grad, ref["dw"])
        if cls.bias is not None:
            _cmp(fails, tag, "dbias", cls.bias.grad, ref["db"])
        _cmp(fails, tag, "running_mean", bn.running_mean, ref["rm"], tol=1e-5)
        _cmp(fails, tag, "running_var", bn.running_var, ref["rv"], tol=1e-5)
        ran += 1
    _report(fails, ran, len(CLS_P) * 2)


def _k5_sweep(shapes, seed):
    fails, ran, fragile = [], 0, 0
    for i, (B, C, H, W) in enumerate(shapes):
        # training-mode statistics over fewer than 32 samples per channel make the three stacked normalisations an ill-conditioned
        # function of the input (test_gpu_backbone_edges.py, BN_SPREAD): such planes run in eval mode, the others alternate
        training = B * H * W >= 32 and i % 2 == 0
        with_glob = (i // 2) % 2 == 0
        m0, x, g, glob, gamma, ref, frag = _k5_case(B, C, H, W, training, with_glob, seed)
        fragile += int(frag.sum())
        res = _k5_dev(m0, x, g, glob, gamma, training)
        _k5_compare(fails, f"cab_local {(B, C, H, W)} glob={with_glob} training={training}", res, ref, frag)
        ran += 1
    return fails, ran, fragile


@gpu
@pytest.mark.parametrize("B", [1, 2, 3])
def test_cab_local_resident_residue_sweep(B):
    """K5's resident form on every plane of 1..12 x 1..12 pixels, C = 3, with and without the gamma * glob term.  Training mode starts
    at 32 samples per channel (B*H*W >= 32, every other plane); smaller planes run in eval mode only."""
    from cabinet_amd import _lib

    lib = _lib.load()
    shapes = [(B, 3, H, W) for H, W in itertools.product(range(1, 13), range(1, 13))]
    assert all(lib.cabinet_cab_local_bwd_workspace_bytes(*s) == 0 for s in shapes)
    fails, ran, fragile = _k5_sweep(shapes, 70 + B)
    assert fragile <= 4, f"{fragile} channels with a ReLU input within 2e-6 of zero"
    _report(fails, ran, 144)


def _tiled_shapes():
    """W of TILED_W; H so that the tile count (1, 2, 3) and the last tile's height (1, 2, TR - 1, TR) take every small value; B the
    smallest batch for which the library chooses the tiled form."""
    shapes = []
    for W in TILED_W:
        TR = 4096 // W
        hs = [1, 2, 3, 5] if W <= 3 else sorted({1, 2, TR - 1, TR, TR + 1, TR + 2, 2 * TR - 1, 2 * TR, 2 * TR + 1})
        for H in hs:
            B = 1
            while B * H * W <= 8192 and _local_lds_bwd(B, H, W) <= 160 * 1024:
                B += 1
            shapes.append((B, 2, H, W))
    return shapes


@gpu
def test_cab_local_tiled_residue_sweep():
    """K5's tiled form at W in {1, 2, 3, 63, 64, 65, 255, 257} with one, two and three row tiles per plane whose last tile holds
    1, 2, TR - 1 or TR rows.  Every plane has more than 32 samples per channel: training and eval alternate."""
    from cabinet_amd import _lib

    lib = _lib.load()
    shapes = _tiled_shapes()
    assert all(lib.cabinet_cab_local_supported(*s) == 1 and lib.cabinet_cab_local_bwd_workspace_bytes(*s) > 0 for s in shapes)
    geoms = {_tiled_geom(B, H, W)[:2] for B, _, H, W in shapes}
    assert {nT for _, nT in geoms} == {1, 2, 3}
    fails, ran, fragile = _k5_sweep(shapes, 80)
    assert fragile <= 4, f"{fragile} channels with a ReLU input within 2e-6 of zero"
    _report(fails, ran, 3 * 4 + 5 * 9)


@gpu
@pytest.mark.parametrize("Ci,Co", C1_SWEEP)
def test_conv1x1_small_path_residue_sweep(Ci, Co):
    """`conv1x1` on planes of 1..200 pixels (B = 2): y, dx, dw through the C ABI, NaN-prefilled."""
    gen = torch.Generator().manual_seed(6000 + Ci)
    fails, ran = [], 0
    for P in range(1, 201):
        x, w, g, ref = _c1_case(2, Ci, Co, 1, P, gen)
        out = _c1_direct(x.cuda(), w.cuda(), g.cuda())
        tag = f"conv1x1 {Ci}->{Co} P={P}"
        _cmp(fails, tag, "y", out[0], ref[0], maxnorm=True, atol=0.0)
        _cmp(fails, tag, "dx", out[1], ref[1], maxnorm=True, atol=0.0)
        _cmp(fails, tag, "dw", out[2], ref[2], atol=0.0)
        ran += 1
    _report(fails, ran, 200)


# ------------------------------------------------------------------------------------------------ 4. caller contract
def _contract_conv3x3():
    from cabinet_amd.functional import conv3x3, conv3x3_bn_part

    w = (torch.randn(64, 128, 3, 3, generator=torch.Generator().manual_seed(1)) * 0.05).cuda().requires_grad_(True)
    buffers = []

    def fn(x, x1):
        part = conv3x3_bn_part(x, 64).fill_(float("nan"))
        buffers.append(part)
        return conv3x3(x, w, x1, part)

    return fn, [w], buffers


def _contract_conv1x1():
    from cabinet_amd.functional import conv1x1

    w = torch.randn(24, 16, 1, 1, generator=torch.Generator().manual_seed(2)).cuda().requires_grad_(True)
    return (lambda x: conv1x1(x, w)), [w], []


def _contract_conv1x1_bias():
    from cabinet_amd.functional import conv1x1, conv1x1_bias_supported

    torch.manual_seed(3)
    conv = torch.nn.Conv2d(16, 24, 1, bias=True).cuda()

    def fn(x):
        assert conv1x1_bias_supported(x, conv)
        return conv1x1(x, conv.weight, conv.bias)

    return fn, [conv.weight, conv.bias], []


def _contract_cab_local():
    from cabinet_amd.functional import cab_local

    m = t_loc._make(4, 4).cuda().train()
    gamma = torch.tensor([0.37]).cuda().requires_grad_(True)
    return (lambda x, glob: cab_local(x, m.refine, glob, gamma)), list(m.parameters()) + [gamma], [b for b in m.buffers() if b.is_floating_point()]


def _contract_cab_qkv():
    from cabinet_amd.functional import cab_qkv

    m = t_qkv._make(32, 16, 16, (2, 5), 5).cuda().train()
    params = [p for n, p in m.named_parameters() if not n.startswith("project_out")]
    return (lambda x: cab_qkv(x, m)), params, [b for b in m.buffers() if b.is_floating_point()]


def _contract_bn_relu_cls():
    from cabinet_amd.functional import bn_relu_cls

    bn, cls = t_cls._modules(64, 8, True, torch.Generator().manual_seed(6))
    bn, cls = bn.cuda().train(), cls.cuda()

    def fn(z):
        y = bn_relu_cls(z, bn, cls)
        assert type(y.grad_fn).__name__ == "_BnClsBackward"
        return y

    return fn, list(bn.parameters()) + list(cls.parameters()), [bn.running_mean, bn.running_var]


def _contract_cab_attention():
    from cabinet_amd.functional import cab_attention, cab_attention_supported

    assert cab_attention_supported(128, 128)
    return (lambda q, k, v: cab_attention(q, k, v, 128 ** -0.5)), [], []


def _contract_cab_attention_proj():
    from cabinet_amd.functional import cab_attention_proj, cab_attention_proj_supported

    w = (torch.randn(256, 128, generator=torch.Generator().manual_seed(8)) * 128 ** -0.5).cuda().requires_grad_(True)

    def fn(q, k, v):
        assert cab_attention_proj_supported(q, v, w)
        return cab_attention_proj(q, k, v, w, 128 ** -0.5)

    return fn, [w], []


def _ffm_params(seed):
    gen = torch.Generator().manual_seed(seed)
    ws = [torch.randn(256, 384, 1, 1, generator=gen) * 0.07, torch.randn(64, 256, 1, 1, generator=gen) * 0.1, torch.randn(256, 64, 1, 1, generator=gen) * 0.1]
    bn = _set_bn(torch.nn.BatchNorm2d(256), gen).cuda().train()
    return [w.cuda().requires_grad_(True) for w in ws], bn


def _contract_ffm_fused():
    from cabinet_amd.functional import ffm_fused

    (wb, w1, w2), bn = _ffm_params(9)
    return (lambda fsp, fcp: ffm_fused(fsp, fcp, wb, bn, w1, w2)), [wb, w1, w2] + list(bn.parameters()), [bn.running_mean, bn.running_var]


def _contract_ffm_fused_upsampled():
    from cabinet_amd.functional import ffm_fused_upsampled

    (wb, w1, w2), bn = _ffm_params(10)
    return (lambda fsp, low: ffm_fused_upsampled(fsp, low, wb, bn, w1, w2)), [wb, w1, w2] + list(bn.parameters()), [bn.running_mean, bn.running_var]


HEAD_CONTRACT = {
    "conv3x3": (_contract_conv3x3, [(2, 64, 6, 10), (2, 64, 6, 10)]),
    "conv1x1": (_contract_conv1x1, [(2, 16, 5, 7)]),
    "conv1x1_bias": (_contract_conv1x1_bias, [(2, 16, 5, 7)]),
    "cab_local": (_contract_cab_local, [(2, 4, 6, 5), (2, 4, 6, 5)]),
    "cab_qkv": (_contract_cab_qkv, [(2, 32, 8, 20)]),
    "bn_relu_cls": (_contract_bn_relu_cls, [(2, 64, 6, 10)]),
    "cab_attention": (_contract_cab_attention, [(2, 128, 40), (2, 128, 40), (2, 128, 40)]),
    "cab_attention_proj": (_contract_cab_attention_proj, [(8, 128, 256), (8, 128, 256), (8, 128, 256)]),
    "ffm_fused": (_contract_ffm_fused, [(2, 128, 12, 10), (2, 256, 12, 10)]),
    "ffm_fused_upsampled": (_contract_ffm_fused_upsampled, [(2, 128, 32, 64), (2, 256, 8, 16)]),
}


def _restrided(x):
    """The values of ``x`` in another memory order: channels_last for a 4-D tensor, the last two dimensions swapped in storage for a
    3-D one."""
    if x.dim() == 4:
        return x.contiguous(memory_format=torch.channels_last)
    return x.transpose(1, 2).contiguous().transpose(1, 2)


def _offset(x):
    return torch.empty(x.numel() + 1, device=x.device)[1:].view(x.shape).copy_(x)


@gpu
@pytest.mark.parametrize("name", list(HEAD_CONTRACT))
def test_head_wrappers_accept_any_layout(name):
    """Channels_last (3-D: transposed) inputs, inputs that start 4 bytes into their storage, a non-contiguous output gradient
    (backward through a transposed view) and a stride-0 one (y.sum().backward()): the wrappers copy such operands and the kernels
    are bit-reproducible, so outputs, every gradient and the running buffers are bit for bit those of the dense, aligned call."""
    build, shapes = HEAD_CONTRACT[name]
    gen = torch.Generator().manual_seed(44)
    xs = [(torch.randn(*s, generator=gen) * 1.3 + 0.2).cuda() for s in shapes]
    xs_cl, xs_off = [_restrided(x) for x in xs], [_offset(x) for x in xs]
    for x, c, o in zip(xs, xs_cl, xs_off):
        assert not c.is_contiguous() and o.is_contiguous() and o.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
        assert torch.equal(c, x) and torch.equal(o, x)
    gs = None

    def run(inputs, mode):
        nonlocal gs
        fn, params, buffers = build()  # fresh, identically seeded parameters and running buffers
        inputs = [x.detach().requires_grad_(True) for x in inputs]
        ys = fn(*inputs)
        ys = list(ys) if isinstance(ys, (tuple, list)) else [ys]
        if gs is None:
            gs = [torch.randn(y.shape, generator=gen).cuda() for y in ys]
        if mode == "dense":
            torch.autograd.backward(ys, gs)
        elif mode == "transposed":   # every output receives a transposed view: not contiguous
            torch.autograd.backward([y.transpose(-1, -2) for y in ys], [g.transpose(-1, -2).contiguous() for g in gs])
        elif mode == "ones":
            torch.autograd.backward(ys, [torch.ones_like(y) for y in ys])
        else:
            sum(y.sum() for y in ys).backward()  # every output receives an expanded scalar: every stride 0
        assert all(x.grad is not None for x in inputs) and all(p.grad is not None for p in params)
        return [y.detach() for y in ys] + [x.grad for x in inputs] + [p.grad for p in params] + [b.clone() for b in buffers]

    base = run(xs, "dense")
    for what, got in (("channels_last / transposed inputs", run(xs_cl, "dense")), ("inputs 4 bytes into their storage", run(xs_off, "dense")),
                      ("non-contiguous grad_output", run(xs, "transposed"))):
        bad = [i for i, (a, b) in enumerate(zip(got, base)) if not torch.equal(a, b)]
        assert len(got) == len(base) and not bad, f"{name}, {what}: tensors {bad} differ from the dense, aligned call"
    ones, summed = run(xs, "ones"), run(xs, "sum")
    bad = [i for i, (a, b) in enumerate(zip(summed, ones)) if not torch.equal(a, b)]
    assert not bad, f"{name}, stride-0 grad_output: tensors {bad} differ from the dense call"
