"""Attention core (K1 / K2) and Feature Fusion Module (K3 / K4) where their host-side launch plans branch and where their tiles
end -- every case through the public wrapper or the C ABI, against the fp64 CPU oracle (oracle/cab_math.py, and for the fused
upsample F.interpolate(mode="bilinear", align_corners=False) in fp64, as in test_gpu_ffm.py).

1. Plan-branch cases, one shape per branch that no other operator test reaches.  Attention: `launch_dq_direct`'s NCB either side
   of each threshold, every value of `dq_ksplit` with its alignment decrement and a longer last segment, the recompute kernels
   with a query split and at n % 4 == 0 (dS above DS_MAX_BYTES, next to the largest batch that still stores dS), the generic pair,
   the forward key split at 64/64 and 256/128 (4-wave kernel), with the split-bf16 forms, and in the rounds regime.  FFM:
   `gemm_kmajor_kernel<2 | 3, guarded | interior, 0 | 1 | 2>`, more than 16 per-image BatchNorm partials (the tree of the folded
   finalize), a ragged 4096-pixel chunk, the guarded weight gradient on whole chunks, shrinking and mixed resizes
   (`upsample_adjoint_kernel<false>`), (lin_adj, fused_xw) = (1, 0), de-interleave factors 2, 3 and 8, three bands with a one-row
   last band, a band of 122 KB of LDS after a small one, odd unit counts of both persistent kernels, the low-resolution side off
   `small_grid`, and the geometry the backward refuses.  Attention calls go through the C ABI with outputs and workspace
   NaN-prefilled; FFM calls go through the public wrappers.  Every case runs twice and must give the same bits.
   Criteria (the per-kernel files' own): ctx 2e-5, lse 1e-5, dq / dk / dv 5e-5 against fp64 (conftest.assert_close's rule);
   bf16x6 <= max(2 x the fp32 kernel's distance on the same inputs, 1e-6), bf16x3 < 5e-5; FFM 1e-3 per tensor, for the maps also
   max|a-b| <= 1e-3 max|b|, running statistics 1e-5.
2. `test_attn_ffm_plan_cases_reach_their_branches` (no GPU): restates every host rule with its file:line, cross-checks the
   restatement against the library's workspace queries wherever one discriminates (the forward key split and the backward's
   nsplit, both decoded from the library's answers, for every B in 1..64 and n in {32k, 32k+1} below 20000 -- the splits seen are
   exactly {1, 2, 4}: the loops' s = 8 is dead
   under the present charges, and a retuned charge that makes it reachable turns this test red and asks for a split-8 case), and
   asserts that every row of part 1 reaches the branch it names.
3. Dense sweeps, all failing shapes collected into one message, the number of shapes run asserted: attention at n = 1..136 and
   around the split thresholds, `cab_attention_proj` at n = 4, 8, .. 136, the plain FFM around the 128-pixel tile and the 32-pixel
   chunk, the fused-upsample FFM over Hl = 1..10 at the x4 ratio and at non-integer ratios.
4. Caller contract of `cab_attention`, `cab_attention_proj`, `ffm_fused`, `ffm_fused_upsampled` at shapes that take the ragged /
   guarded kernels: transposed (3-D) and channels_last (4-D) inputs, inputs 4 bytes into their storage, non-contiguous and stride-0
   output gradients give bit for bit the results of the dense, aligned call.
5. Findings.  `cabinet_ffm_up_bwd` refused a geometry whose staged band exceeds the LDS with a bare "invalid argument" AFTER it
   had launched the reduction kernels; it now refuses before any launch and says which geometry and why
   (`test_ffm_up_bwd_refuses_a_band_above_the_lds_cap`).  K1 with the projection in its epilogue prefetched the weight rows of
   output block `wave` in all eight waves, whatever Co: below Co = 256 the waves without a block read up to 256 rows of a shorter
   w_out, and at (128, 128) with Co = 96 that read left the allocation and faulted (`test_attn_proj_residue_sweep[128-128]`; the
   rows were never used, so results did not change).  The prefetch is now guarded by `wave * 32 < Co`.

`check_ffm_shape` (capi.hip) admits only Cs, Cc, Co that are multiples of 32, so the guarded forms are reached with Co = 192 and 288,
Cs | Cc = 96 | 192 and 160 | 224.  Unreachable through the wrappers, hence without a test: `lda % 4 != 0` in `gemm_kmajor` from the
FFM (lda is Co or Cs + Cc) and a source split at a channel that is no multiple of 32; and the last clause of
`ffm_bwd_fused_supported` cannot fail at the x4 ratio (P = 16 Pl gives (16 + Cc / 128) B Pl / 32 units, and ceil(that / 256) <=
B Pl / 32 always).

ReLU units near the kink: the FFM re-decides borderline pre-activations in double (ffm.hip, ffm_pool_kernel), so it follows the
fp64 oracle's mask; still every FFM input set is checked on the CPU before the device runs.  The margin of `_clear_of_kinks`
(2e-4) cannot be met by choosing seeds at most shapes here -- a tensor of N unit-variance pre-activations holds about 1.6e-4 N units
within it: one at N = 6000, twenty at the sweeps' 256-channel planes, a thousand at the largest cases -- so one margin serves
every shape: the one the head file uses for K5, 2e-6 (ten times the rounding error of an fp32 pre-activation of size one).  No
BatchNorm output and no squeeze unit of the fp64 oracle lies within it, by the seeds of FFM_SEEDS.  The seven cases of more than
2^21 units (FFM_BIG) hold several such units under any seed: with gamma >= 0.5 the density of a pre-activation at zero is at most
0.8, so at most m = 3.2e-6 N of N units are expected inside the margin, and the count is asserted to stay below m + 5 sqrt(m);
those units are left to the re-decision itself, which smoke() asserts on its own.

Two samples per channel in training mode (B = 2 on a one-pixel plane): the normalised values are +-1 whatever z is, and
dz = gamma invstd (dy1 - dy2) / 2 * eps / (var + eps) is the difference of numbers that agree to five digits, so the gradients that
flow through dz (dfsp, dfcp, dw_blk) lose those digits in ANY fp32 evaluation.  There, and only there, these three are held to
max(1e-3, 2 x the distance of the oracle's own formulas evaluated in fp32 on the same inputs), in the tensor norm and for the
maps in the max norm; both distances are printed (the fp32 evaluation lies 1e-5 .. 3e-5 from fp64 on these inputs, so the bound in
force is the 1e-3 rule).  Output, BatchNorm and squeeze gradients and running statistics keep their bounds.
"""
import copy
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_attn as t_attn
import test_gpu_ffm as t_ffm
from conftest import rel_err
from oracle.cab_math import attn_core_bwd, attn_core_fwd, ffm_bwd, ffm_fwd
from test_gpu_backbone_edges import _all_equal, _cmp, _report, _set_bn
from test_gpu_head_edges import _offset, _restrided

gpu = pytest.mark.gpu
TOL = 1e-3       # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32; the maps also in the max norm
KINK = 2e-6      # see the module docstring
PAIRS = [(64, 64), (128, 128), (256, 128)]
BF16_PAIRS = [(64, 64), (128, 128)]   # attn_bf16_supported (cab_attn_bf16.hip:425)

# ------------------------------------------------------------------------------------------------ the plan-branch tables
# attention (B, Kc, Vc, n) -> what the case is there for; every entry is checked by _attn_plan in part 2.
#   ncb: channel blocks per workgroup of cab_attn_bwd_dq_ds_kernel; ks: dq_ksplit; ds: stored-dS form; nsplit: bwd_nsplit;
#   split: attn_fwd_kvsplit; fwd: the fp32 forward kernel ("w8" two waves per SIMD, "w4" the 4-wave kernel)
ATTN_CASES = {
    (49, 128, 128, 128): dict(ncb=2), (50, 128, 128, 128): dict(ncb=4),
    (24, 128, 128, 128): dict(ncb=1), (25, 128, 128, 128): dict(ncb=2),
    (49, 64, 64, 128): dict(ncb=1), (50, 64, 64, 128): dict(ncb=2),
    (12, 256, 128, 128): dict(ncb=1, ks=1), (13, 256, 128, 128): dict(ncb=2, ks=1),
    (24, 256, 128, 128): dict(ncb=2, ks=1), (25, 256, 128, 128): dict(ncb=4, ks=1),
    (1, 256, 128, 512): dict(ks=2, ds=True, nsplit=2, split=2, fwd="w4"),
    (1, 256, 128, 516): dict(ks=1, ds=True, nsplit=2),                       # 516 / 2 = 258: no 16-byte rows -> one segment
    (1, 256, 128, 780): dict(ks=3, ds=True, nsplit=2),
    (1, 256, 128, 1040): dict(ks=4, ds=True, nsplit=4),
    (1, 256, 128, 1044): dict(ks=3, ds=True, nsplit=4),                      # 1044 / 4 = 261 -> three segments of 348
    (1, 256, 128, 1300): dict(ks=5, ds=True, nsplit=4),
    (1, 256, 128, 1540): dict(ks=6, ds=True, nsplit=4, last=260),            # five segments of 256 and one of 260
    (1, 256, 128, 1796): dict(ks=7, ds=True, nsplit=4, last=260),
    (1, 256, 128, 2052): dict(ks=8, ds=True, nsplit=2, last=260),
    (1, 64, 64, 485): dict(ds=False, nsplit=2, split=2, fwd="w4"),            # recompute kernels with a split at 64/64; x6 / x3 ragged
    (1, 128, 128, 997): dict(ds=False, nsplit=4, split=4, fwd="w4"),
    (1, 256, 128, 485): dict(ds=False, nsplit=1, split=2, fwd="w4", generic=True),
    (1, 256, 128, 484): dict(ds=True, split=2, fwd="w4"),
    (1, 128, 128, 485): dict(ds=False, split=2, fwd="w4"),
    (1, 64, 64, 484): dict(ds=True, split=2, fwd="w8"),
    (1, 64, 64, 997): dict(ds=False, split=4, fwd="w4"),
    (17, 128, 128, 484): dict(ds=True, split=2, nsplit=2, fwd="w8", wgs=272),  # the rounds regime: 272 query tiles
}
# the recompute kernels at n % 4 == 0: dS of 129 images is 541 MB (> DS_MAX_BYTES), of 128 images exactly 512 MB
ATTN_DS_CAP = {(129, 128, 128, 1024): dict(ds=False, nsplit=1, split=1, fwd="w8"), (128, 128, 128, 1024): dict(ds=True, ncb=4, split=1)}
ATTN_SWEEP_N = list(range(1, 137))
ATTN_EDGE_N = [476, 477, 480, 481, 484, 485, 509, 512, 513, 516, 988, 989, 992, 993, 996, 997]

# FFM plain (B, Cs, Cc, Co, Cm, H, W) -> G1 (forward product) and G2 (data gradient) as (WM, interior, UP), and what else it is for
FFM_PLAIN = {
    (2, 128, 256, 256, 64, 100, 128): dict(g1=(2, True, 0), g2=(3, True, 0), cpr=4, prod=(200, 200)),
    (2, 128, 256, 256, 64, 99, 128): dict(g1=(1, True, 0), g2=(1, True, 0), cpr=4, prod=(198, 198)),
    (2, 32, 64, 192, 24, 5, 7): dict(g1=(2, False, 0)),
    (2, 32, 64, 288, 24, 5, 7): dict(g1=(3, False, 0)),
    (2, 96, 192, 96, 24, 5, 7): dict(g2=(3, False, 0)),                                # lda = 288
    (17, 32, 64, 96, 24, 3, 5): dict(tree=True),                                       # more than 16 per-image partials
    (1, 128, 256, 256, 64, 65, 64): dict(cpr=2, g1=(1, False, 0)),                     # P = 4160: a 64-pixel second chunk, P % 128 = 64
    (1, 160, 224, 256, 64, 16, 16): dict(dw=(False, False), g2=(1, True, 0)),          # guarded gemm_dw_kernel with P % 32 == 0
}
FFM_PLAIN_EVAL = [(17, 32, 64, 96, 24, 3, 5)]
# FFM fused-upsample (B, Cs, Cc, Co, Cm, H, W, Hl, Wl) -> see _up_plan; only the keys a row is there for are listed
FFM_UP = {
    (2, 128, 256, 256, 64, 4, 8, 8, 16): dict(fuse_dz=False, R=1, bands=1),             # shrinking: upsample_adjoint_kernel<false>
    (1, 64, 96, 96, 24, 3, 5, 7, 9): dict(fuse_dz=False, R=1, bands=1),
    (1, 64, 96, 96, 24, 8, 5, 4, 9): dict(fuse_dz=True, lin=False, R=1),                # H >= Hl, W < Wl
    (2, 64, 96, 96, 24, 16, 16, 4, 4): dict(lin=True, xw=False),
    (2, 128, 512, 256, 64, 16, 16, 4, 4): dict(lin=True, xw=False, segs=5),             # five segments > XW_MAXSEG
    (1, 128, 256, 256, 64, 68, 64, 17, 16): dict(lin=True, xw=False, fz=(68, 1), cpr=2),   # Pl % 32 != 0
    (1, 128, 256, 256, 64, 4, 256, 2, 32): dict(gz=(1, True, 1), lin=False, xw=True, R=8),   # row form UP = 1
    (2, 128, 256, 128, 32, 8, 128, 2, 32): dict(gz=(1, True, 1), lin=True, xw=False),
    (1, 128, 256, 256, 64, 6, 20, 3, 10): dict(lin=False, R=2),
    (1, 128, 256, 256, 64, 9, 24, 3, 8): dict(lin=False, R=3),
    (1, 128, 256, 256, 64, 65, 64, 17, 16): dict(lin=False, bands=3, last_band=1, R=4),
    (2, 32, 64, 288, 24, 5, 7, 2, 3): dict(gz=(3, False, 2)),
    (2, 64, 256, 256, 64, 100, 128, 25, 32): dict(gz=(2, True, 1)),
    (2, 64, 256, 256, 64, 200, 64, 50, 16): dict(gz=(2, True, 2)),
    (3, 128, 256, 256, 64, 88, 64, 22, 16): dict(lin=True, xw=True, fz=(132, 2), xw_units=(594, 3)),
    (2, 128, 256, 256, 64, 8, 512, 2, 128): dict(lin=False, xw=True, R=4, lds=125408),  # 122 KB of the 160 KB
    (2, 64, 256, 256, 64, 100, 128, 100, 128): dict(small_low=False, small=False, ylow=(2, True, 0), dlow=(2, True, 0)),
    (2, 64, 256, 256, 64, 99, 128, 99, 128): dict(small_low=True, small=True),
}
FFM_REFUSED = (1, 128, 256, 256, 64, 32, 256, 2, 16)     # the band of the two-pass adjoint would stage 197 KB
FFM_SMALL_BEFORE_CAP = (1, 128, 256, 256, 64, 6, 20, 3, 10)
# more than 2^21 BatchNorm outputs: several within KINK of zero under any seed (module docstring)
FFM_BIG = {(2, 128, 256, 256, 64, 100, 128), (2, 128, 256, 256, 64, 99, 128), (2, 64, 256, 256, 64, 100, 128, 25, 32),
           (2, 64, 256, 256, 64, 200, 64, 50, 16), (2, 64, 256, 256, 64, 100, 128, 100, 128), (2, 64, 256, 256, 64, 99, 128, 99, 128),
           (3, 128, 256, 256, 64, 88, 64, 22, 16)}
# (shape, training) -> seed where the default (0) leaves a ReLU input of the fp64 oracle within KINK of zero (checked on the CPU)
FFM_SEEDS = {
    ((1, 128, 256, 256, 64, 65, 64), True): 1, ((2, 64, 96, 96, 24, 16, 16, 4, 4), True): 1,
    ((1, 128, 256, 256, 64, 68, 64, 17, 16), True): 6, ((2, 128, 256, 128, 32, 8, 128, 2, 32), True): 2,
    ((1, 128, 256, 256, 64, 65, 64, 17, 16), True): 9, ((2, 128, 256, 256, 64, 8, 512, 2, 128), True): 12,
    ((2, 32, 64, 96, 24, 1, 20), True): 1, ((2, 32, 64, 192, 24, 1, 132), False): 1, ((2, 32, 64, 192, 24, 1, 133), True): 1,
    ((2, 32, 64, 192, 24, 4, 31), False): 1, ((2, 128, 256, 256, 64, 4, 16, 1, 4), False): 1,
    ((2, 128, 256, 256, 64, 4, 32, 1, 8), False): 1, ((2, 128, 256, 256, 64, 12, 16, 3, 4), False): 1,
    ((2, 128, 256, 256, 64, 12, 32, 3, 8), False): 1, ((2, 128, 256, 256, 64, 12, 64, 3, 16), True): 3,
    ((2, 128, 256, 256, 64, 12, 64, 3, 16), False): 1, ((2, 128, 256, 256, 64, 16, 64, 4, 16), True): 1,
    ((2, 128, 256, 256, 64, 16, 64, 4, 16), False): 2, ((2, 128, 256, 256, 64, 20, 64, 5, 16), True): 2,
    ((2, 128, 256, 256, 64, 24, 16, 6, 4), False): 2, ((2, 128, 256, 256, 64, 24, 64, 6, 16), False): 2,
    ((2, 128, 256, 256, 64, 28, 16, 7, 4), False): 1, ((2, 128, 256, 256, 64, 28, 32, 7, 8), True): 4,
    ((2, 128, 256, 256, 64, 28, 32, 7, 8), False): 3, ((2, 128, 256, 256, 64, 28, 64, 7, 16), False): 3,
    ((2, 128, 256, 256, 64, 32, 16, 8, 4), True): 3, ((2, 128, 256, 256, 64, 32, 16, 8, 4), False): 1,
    ((2, 128, 256, 256, 64, 32, 32, 8, 8), False): 1, ((2, 128, 256, 256, 64, 32, 64, 8, 16), True): 4,
    ((2, 128, 256, 256, 64, 32, 64, 8, 16), False): 10, ((2, 128, 256, 256, 64, 36, 16, 9, 4), True): 1,
    ((2, 128, 256, 256, 64, 36, 32, 9, 8), True): 4, ((2, 128, 256, 256, 64, 36, 64, 9, 16), True): 6,
    ((2, 128, 256, 256, 64, 36, 64, 9, 16), False): 1, ((2, 128, 256, 256, 64, 40, 32, 10, 8), False): 8,
    ((2, 128, 256, 256, 64, 40, 64, 10, 16), True): 1, ((2, 128, 256, 256, 64, 40, 64, 10, 16), False): 1,
    ((2, 128, 256, 256, 64, 7, 22, 3, 5), False): 1, ((2, 128, 256, 256, 64, 9, 14, 4, 3), True): 1,
}

FFM_SWEEP_CO = [96, 192]
FFM_SWEEP_HW = [(1, P) for P in list(range(1, 41)) + list(range(120, 137))] + list(itertools.product((3, 4, 5), (31, 32, 33, 43)))
FFM_UP_SWEEP = ([(4 * Hl, 4 * Wl, Hl, Wl) for Hl in range(1, 11) for Wl in (4, 8, 16)]
                + [(H, 4 * Wl + 2, Hl, Wl) for (H, Hl) in ((7, 3), (9, 4), (30, 7)) for Wl in (3, 5)])


def _a256(n):
    return (n + 255) // 256 * 256


def _a64(n):
    return (n + 63) // 64 * 64


def _cd(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the host rules, restated
def _rounds_split(B, n, charge):
    """attn_fwd_kvsplit (cab_attn_fwd.hip:594-610, charge 0.04) and bwd_nsplit (cab_attn_bwd.hip:871-884, charge 0.05)."""
    nt = _cd(n, 32)
    wgs = nt * B
    best, best_cost, cost1 = 1, 1e30, 0.0
    for s in (1, 2, 4, 8):
        if s > 1 and s * 8 > nt:
            break
        cost = _cd(wgs * s, 256) / s + (charge * s if s > 1 else 0.0)
        if s == 1:
            cost1 = cost
        if cost < best_cost - 1e-9:
            best, best_cost = s, cost
    return 1 if best > 1 and best_cost > 0.85 * cost1 else best


def _fwd_split(B, n):
    return _rounds_split(B, n, 0.04)


def _bwd_nsplit(B, n):
    return _rounds_split(B, n, 0.05)


def _dq_ksplit(n):
    """cab_attn_bwd.hip:1045-1050."""
    s = min(max(n // 256, 1), 8)
    while s > 1 and (n // s) % 4:
        s -= 1
    return s


def _use_ds(B, n):
    """use_ds_path (cab_attn_bwd.hip:1077-1078): DS_MAX_BYTES = 512 MB."""
    return n % 4 == 0 and B * n * n * 4 <= 512 << 20


def _ncb(B, Kc, n):
    """launch_dq_direct (cab_attn_bwd.hip:1035-1041)."""
    tiles, blocks = _cd(n, 32) * B, Kc // 32
    if blocks % 4 == 0 and tiles * (blocks // 4) >= 200:
        return 4
    if blocks % 2 == 0 and tiles * (blocks // 2) >= 200:
        return 2
    return 1


def _attn_fwd_ws(B, Vc, n):
    """attn_fwd_split_bytes (capi.hip:234-237) at precision 0."""
    s = _fwd_split(B, n)
    return 0 if s == 1 else _a256(s * B * Vc * n * 4) + _a256(s * B * n * 4)


def _attn_bwd_ws(B, Kc, Vc, n, ns=None):
    """attn_bwd_workspace (cab_attn_bwd.hip:1175-1184); ``ns``: the bytes for that nsplit instead of bwd_nsplit's."""
    nbytes = (_a64(B * n) + _a64(B * Kc)) * 4
    fast = (Kc <= 128 and Kc + Vc <= 256) or (Kc == 256 and Vc == 128 and _use_ds(B, n))
    ns = ns if ns is not None else _bwd_nsplit(B, n) if fast else 1
    if ns > 1:
        nbytes += ns * B * (Kc + Vc) * n * 4
    if _use_ds(B, n):
        ks = _dq_ksplit(n)
        nbytes += (B * n * n + (ks * B * Kc * n if Kc == 256 and ks > 1 else 0)) * 4
    return _a256(nbytes)


SPLITS = (1, 2, 4, 8, 16)


def _lib_fwd_split(lib, B, n):
    """attn_fwd_kvsplit as the library's workspace query encodes it (distinct splits give distinct sizes)."""
    got = lib.cabinet_cab_attn_fwd_workspace_bytes(B, 128, 128, n, 0)
    match = [s for s in SPLITS if got == (0 if s == 1 else _a256(s * B * 128 * n * 4) + _a256(s * B * n * 4))]
    assert len(match) == 1, (B, n, got)
    return match[0]


def _lib_bwd_nsplit(lib, B, n):
    """bwd_nsplit as cabinet_cab_attn_bwd_workspace_bytes encodes it at (128, 128): nsplit slabs of B * 256 * n floats."""
    got = lib.cabinet_cab_attn_bwd_workspace_bytes(B, 128, 128, n)
    match = [s for s in SPLITS if got == _attn_bwd_ws(B, 128, 128, n, s)]
    assert len(match) == 1, (B, n, got)
    return match[0]


def _attn_plan(B, Kc, Vc, n):
    """What attn_fwd_dispatch / attn_bwd_dispatch (cab_attn_fwd.hip:561-588, cab_attn_bwd.hip:1186-1199) run for a shape."""
    ds = _use_ds(B, n)
    generic = Kc == 256 and not ds
    plan = dict(split=_fwd_split(B, n), fwd="w8" if Kc <= 128 and n % 4 == 0 else "w4", ds=ds, generic=generic,
                nsplit=1 if generic else _bwd_nsplit(B, n), wgs=_cd(n, 32) * B)
    if ds:
        plan["ncb"] = _ncb(B, Kc, n)
        if Kc == 256:
            ks = _dq_ksplit(n)
            plan["ks"], plan["last"] = ks, n - (ks - 1) * ((n // ks + 3) & ~3)
    return plan


def _small_grid(B, M, P):
    """blocks.hpp:112."""
    return _cd(P, 128) * B * _cd(M, 128) < 400


def _gk(M, P, B, lda, up=False, W=0, Wl=0):
    """gemm_kmajor and launch_gemm_k_wm (ffm.hip:232-250) -> (WM, INTERIOR, UP)."""
    wm = 1 if M <= 128 else (3 if 256 < M <= 384 else 2)
    if wm > 1 and M % 128 == 0 and _cd(P, 128) * B * _cd(M, 128 * wm) < 200:
        wm = 1
    interior = P % 128 == 0 and M % (128 * wm) == 0 and lda % 4 == 0
    return wm, interior, (0 if not up else 1 if interior and W % 128 == 0 and Wl == 32 else 2)


def _gk_product(M, P, B):
    wm = 1 if M <= 128 else (3 if 256 < M <= 384 else 2)
    return _cd(P, 128) * B * _cd(M, 128 * wm)


def _dw_nsplit(B, Co, Cx, P):
    """dw_nsplit (ffm.hip:535-539) as dw_product calls it (:1405-1409)."""
    return min(_cd(768, _cd(Co, 128) * _cd(Cx, 128)), B * _cd(P, 32), 128)


def _dw_interior(Co, Cx, P):
    """dw_product (ffm.hip:1414)."""
    return P % 32 == 0 and Co % 128 == 0 and Cx % 128 == 0


def _fz_supported(Cs, Co, H, W, Hl, Wl):
    """ffm_fwd_fused_supported (ffm_fwd_fused.hip:344-348): FZ_CO = 256, FZ_CS = 128, FZ_PX = 64, FZ_WL = 32."""
    return Co == 256 and Cs == 128 and W % 64 == 0 and 4 <= Wl <= 32 and Wl % 4 == 0 and W == 4 * Wl and Hl >= 1 and 256 * H * W * 4 < 0x7fffffff


def _fz_nwg(B, P):
    """ffm_fwd_fused_nwg (ffm_fwd_fused.hip:349-352) -> (workgroups, units per workgroup)."""
    units = B * (P // 64)
    upw = _cd(units, 256)
    return _cd(units, upw), upw


def _xw_units(B, Cc, P, Pl):
    """xw_units / xw_units_per_wg (ffm_bwd_fused.hip:394-395): XW_CX = 128, XW_PX = 32."""
    total = B * (P // 32) + (Cc // 128) * B * (Pl // 32)
    return total, _cd(total, 256)


def _xw_supported(B, Cs, Cc, Co, P, Pl):
    """ffm_bwd_fused_supported (ffm_bwd_fused.hip:397-400): XW_CO = 256, XW_MAXSEG = 4."""
    if not (Co == 256 and Cs == 128 and Cc > 0 and Cc % 128 == 0 and Cc // 128 + 1 <= 4 and P % 32 == 0 and Pl % 32 == 0 and B > 0):
        return False
    return _xw_units(B, Cc, P, Pl)[1] <= B * (Pl // 32)


def _xw_slab_floats(B, Cc, P, Pl):
    """ffm_bwd_fused_slab_floats (ffm_bwd_fused.hip:402-406)."""
    total, upw = _xw_units(B, Cc, P, Pl)
    return (_cd(total, upw) + 4) * 256 * 128


def _adj_supported(H, W, Hl, Wl):
    """ffm_bwd_adj_supported (ffm_bwd_adj.hip:168-170): the x4 ratio and a power-of-two width of 4..64."""
    return Hl > 0 and 4 <= Wl <= 64 and Wl & (Wl - 1) == 0 and H == 4 * Hl and W == 4 * Wl


def _adj_geom(H, W, Hl, Wl):
    """adj_geom (ffm.hip): ADJ_BAND = 8 -> (R, bands, rows of the last band, LDS bytes)."""
    f = lambda x: torch.tensor(float(x), dtype=torch.float32)  # noqa: E731  (the host evaluates both in fp32)
    max_rows, XT = int(f(10) * (f(H) / f(Hl))) + 6, int(f(2) * f(W) / f(Wl)) + 4
    R = W // Wl if W % Wl == 0 and W // Wl <= 32 else 1
    plane = _cd(W, R)
    want = 32 // R if R & (R - 1) == 0 else 1
    plane += (want - plane % 32 + 32) % 32
    lds = (max_rows * W + 8 * R * plane + 8 * max_rows + 2 * Wl * XT + 8) * 4
    return R, _cd(Hl, 8), Hl - 8 * (_cd(Hl, 8) - 1), lds


def _plain_plan(B, Cs, Cc, Co, Cm, H, W):
    """ffm_fwd_run / ffm_bwd_run (ffm.hip:1210-1230, :1427-1453) and the tail (:1191-1208, :745)."""
    P, Cin = H * W, Cs + Cc
    return dict(g1=_gk(Co, P, B, Co), g2=_gk(Cin, P, B, Cin), cpr=_cd(P, 4096), tree=B > 16,
                dw=(_dw_interior(Co, Cs, P), _dw_interior(Co, Cc, P)), prod=(_gk_product(Co, P, B), _gk_product(Cin, P, B)))


def _up_plan(B, Cs, Cc, Co, Cm, H, W, Hl, Wl):
    """ffm_up_fwd_run / ffm_up_bwd_run (ffm.hip:1232-1293, ffm_up_bwd_run) with no environment switch set."""
    P, Pl, Cin = H * W, Hl * Wl, Cs + Cc
    plan = dict(small_low=_small_grid(B, Co, Pl) and Cin % 4 == 0 and Cc % 4 == 0, cpr=_cd(P, 4096), segs=1 + Cc // 128)
    if not plan["small_low"]:
        plan["ylow"] = _gk(Co, Pl, B, Co)
    if Cin % 4 == 0 and _fz_supported(Cs, Co, H, W, Hl, Wl):
        plan["fz"] = _fz_nwg(B, P)
    else:
        plan["gz"] = _gk(Co, P, B, Co, True, W, Wl)
    fuse_dz = H >= Hl
    plan.update(fuse_dz=fuse_dz, lin=fuse_dz and _adj_supported(H, W, Hl, Wl), xw=fuse_dz and _xw_supported(B, Cs, Cc, Co, P, Pl))
    if not plan["lin"]:
        plan["R"], plan["bands"], plan["last_band"], plan["lds"] = _adj_geom(H, W, Hl, Wl)
    if plan["xw"]:
        plan["xw_units"] = _xw_units(B, Cc, P, Pl)
    else:
        plan["small"] = _small_grid(B, Cc, Pl) and Cin % 4 == 0 and Cc % 4 == 0 and Co % 4 == 0
        plan["dfsp"] = _gk(Cs, P, B, Cin)
        if not plan["small"]:
            plan["dlow"] = _gk(Cc, Pl, B, Cin)
    return plan


def _ffm_fwd_ws(B, Cs, Cc, Co, Hl=0, Wl=0):
    """ffm_fwd_workspace / ffm_up_fwd_workspace (ffm.hip:1168-1184): W^T, the BatchNorm partials, y_low, the bf16x6 weight images."""
    nbytes = _a256((Cs + Cc) * Co * 4) + _a256(max(B, 256) * 2 * Co * 8)
    return nbytes + (_a256(B * Co * Hl * Wl * 4) + _a256(3 * Co * Cs * 2) if Hl else 0)


def _ffm_bwd_ws(B, Cs, Cc, Co, Cm, H, W, Hl=0, Wl=0):
    """bwd_layout (ffm.hip:1322-1351)."""
    P = H * W
    part = 128 * Co * max(Cs, Cc)
    if Hl and _xw_supported(B, Cs, Cc, Co, P, Hl * Wl):
        part = max(part, _xw_slab_floats(B, Cc, P, Hl * Wl))
    sizes = [B * Co * 5, B * Co, B * Co, Co, Co, B * Co * Cm, B * Co * Cm, B * 2 * Co, B * Co * P, part, B * Co * Hl * Wl]
    return sum(_a256(4 * s) for s in sizes)


def _ffm_shapes_of(fn):
    """The shapes a parametrised test of test_gpu_ffm.py runs."""
    return [mark.args[1] for mark in fn.pytestmark if mark.name == "parametrize"][0]


# ------------------------------------------------------------------------------------------------ 2. the plans, without a GPU
def test_attn_ffm_plan_cases_reach_their_branches():
    """Every row of the tables above reaches the branch it names: the host rules restated, cross-checked against the library's
    workspace queries where one discriminates."""
    from cabinet_amd import _lib

    lib = _lib.load()
    # attention: the forward's key split and the backward's nsplit over the whole grid of B and n
    fwd_seen, bwd_seen = set(), set()
    for B in range(1, 65):
        for n0 in range(32, 20000, 32):
            for n in (n0, n0 + 1):   # both splits are read from the library's answers; the restatement must agree with them
                fs, bs = _lib_fwd_split(lib, B, n), _lib_bwd_nsplit(lib, B, n)
                assert (fs, bs) == (_fwd_split(B, n), _bwd_nsplit(B, n)), (B, n, fs, bs)
                fwd_seen.add(fs)
                bwd_seen.add(bs)
    assert fwd_seen == {1, 2, 4} and bwd_seen == {1, 2, 4}, (fwd_seen, bwd_seen)   # a reachable 8 asks for a split-8 case
    for shape, want in {**ATTN_CASES, **ATTN_DS_CAP}.items():
        B, Kc, Vc, n = shape
        assert lib.cabinet_cab_attn_supported(Kc, Vc) == 1
        assert lib.cabinet_cab_attn_fwd_workspace_bytes(B, Kc, Vc, n, 0) == _attn_fwd_ws(B, Vc, n), shape
        assert lib.cabinet_cab_attn_bwd_workspace_bytes(B, Kc, Vc, n) == _attn_bwd_ws(B, Kc, Vc, n), shape
        plan = _attn_plan(*shape)
        assert {k: plan.get(k) for k in want} == want, (shape, plan)
    # either side of each NCB threshold, and of DS_MAX_BYTES
    for lo, hi in (((49, 128, 128, 128), (50, 128, 128, 128)), ((24, 128, 128, 128), (25, 128, 128, 128)), ((49, 64, 64, 128), (50, 64, 64, 128)),
                   ((12, 256, 128, 128), (13, 256, 128, 128)), ((24, 256, 128, 128), (25, 256, 128, 128))):
        assert hi[0] == lo[0] + 1 and _attn_plan(*lo)["ncb"] * 2 == _attn_plan(*hi)["ncb"] and _attn_plan(*lo)["ds"]
    assert 128 * 1024 * 1024 * 4 == 512 << 20 and 129 * 1024 * 1024 * 4 > 512 << 20
    assert {_attn_plan(1, 256, 128, n)["ks"] for n in (512, 516, 780, 1040, 1044, 1300, 1540, 1796, 2052)} | {
        _attn_plan(*s).get("ks") for s in ((1, 256, 128, 2048), (2, 256, 128, 1000), (1, 256, 128, 66))} == {None, 1, 2, 3, 4, 5, 6, 7, 8}
    # the forward's split edges: nt = 16 key tiles at n = 481 (the last tile holds one key), split 4 from n = 993
    assert [_fwd_split(1, n) for n in (480, 481, 992, 993)] == [1, 2, 2, 4] and [_bwd_nsplit(1, n) for n in (480, 481, 992, 993)] == [1, 2, 2, 4]
    assert all(n in ATTN_EDGE_N for n in (480, 481, 992, 993))
    for Kc, Vc in PAIRS:
        assert lib.cabinet_cab_attn_precision_supported(Kc, Vc, 2) == (1 if (Kc, Vc) in BF16_PAIRS else 0)

    # FFM: the plans from the restated rules, the workspaces from the library
    for shape, want in FFM_PLAIN.items():
        B, Cs, Cc, Co, Cm, H, W = shape
        plan = _plain_plan(*shape)
        assert {k: plan[k] for k in want} == want, (shape, plan)
        assert lib.cabinet_ffm_fwd_workspace_bytes(*shape) == _ffm_fwd_ws(B, Cs, Cc, Co), shape
        assert lib.cabinet_ffm_bwd_workspace_bytes(*shape) == _ffm_bwd_ws(*shape), shape
    assert 4160 % 4096 == 64 and 4160 % 128 == 64 and _dw_interior(256, 128, 4160)
    # dw_nsplit: the chunk count binds on the guarded 16 x 16 plane (8 chunks), the cap of 128 slabs -- what `part` holds -- on the
    # low-resolution side off small_grid (800 chunks, 192 and 384 wanted); no row asks for more than 128
    assert (_dw_nsplit(1, 256, 160, 256), _dw_nsplit(1, 256, 224, 256)) == (8, 8)
    assert (_dw_nsplit(2, 256, 64, 12800), _dw_nsplit(2, 256, 256, 12800)) == (128, 128) and _cd(768, 4) == 192 and _cd(768, 2) == 384
    assert all(_dw_nsplit(s[0], s[3], c, p) <= 128 for s in list(FFM_PLAIN) + list(FFM_UP) for c in s[1:3] for p in (s[5] * s[6], s[-2] * s[-1]))
    for shape, want in FFM_UP.items():
        B, Cs, Cc, Co, Cm, H, W, Hl, Wl = shape
        plan = _up_plan(*shape)
        assert {k: plan.get(k) for k in want} == want, (shape, plan)
        assert plan.get("lds", 0) <= 160 * 1024, shape
        assert lib.cabinet_ffm_up_fwd_workspace_bytes(*shape) == _ffm_fwd_ws(B, Cs, Cc, Co, Hl, Wl), shape
        assert lib.cabinet_ffm_up_bwd_workspace_bytes(*shape) == _ffm_bwd_ws(*shape), shape
    seen = {(p["lin"], p["xw"]) for p in map(lambda s: _up_plan(*s), FFM_UP)}
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert {_up_plan(*s).get("R") for s in FFM_UP} >= {1, 2, 3, 4, 8}
    plan = _up_plan(*FFM_REFUSED)
    assert plan["fuse_dz"] and not plan["lin"] and plan["lds"] == 197344 > 160 * 1024
    assert _up_plan(*FFM_SMALL_BEFORE_CAP)["lds"] < 16 * 1024 and not _up_plan(*FFM_SMALL_BEFORE_CAP)["lin"]
    # the persistent kernels' unit counts of the odd-count row: 264 forward units over 132 workgroups, 594 backward units
    assert 3 * (88 * 64 // 64) == 264 and _fz_nwg(3, 88 * 64) == (132, 2) and _xw_units(3, 256, 88 * 64, 22 * 16) == (594, 3)
    # the slabs of the fused backward outgrow the 128 worst-case dw_product slabs only above 252 workgroups: 255 units of one chunk
    slabby = (1, 128, 128, 256, 64, 120, 64, 30, 16)
    assert _xw_supported(1, 128, 128, 256, 120 * 64, 30 * 16) and _xw_slab_floats(1, 128, 120 * 64, 30 * 16) == 259 * 256 * 128 > 128 * 256 * 128
    assert _xw_slab_floats(3, 256, 88 * 64, 22 * 16) == (198 + 4) * 256 * 128 < 128 * 256 * 256
    assert lib.cabinet_ffm_up_bwd_workspace_bytes(*slabby) == _ffm_bwd_ws(*slabby)
    # the last clause of ffm_bwd_fused_supported cannot fail at the x4 ratio
    assert all(_xw_units(B, Cc, 16 * Pl, Pl)[1] <= B * (Pl // 32) for B in range(1, 70) for Cc in (128, 256, 384) for Pl in range(32, 4097, 32))
    # what motivates this file: every plain and fused-upsample shape of test_gpu_ffm.py runs gemm_kmajor with WM = 1, fuse_dz = 1,
    # R in {1, 4}, and (lin_adj, fused_xw) = (1, 0) nowhere against the oracle
    old_plain = [s[:7] for s in _ffm_shapes_of(t_ffm.test_ffm_vs_oracle)]
    old_up = [s[:9] for s in _ffm_shapes_of(t_ffm.test_ffm_upsampled_vs_oracle)]
    assert all(_plain_plan(*s)[k][0] == 1 for s in old_plain for k in ("g1", "g2"))
    plans = [_up_plan(*s) for s in old_up]
    assert all(p.get(k, (1,))[0] == 1 for p in plans for k in ("gz", "ylow", "dfsp", "dlow")) and all(p["fuse_dz"] for p in plans)
    assert {p["R"] for p in plans if "R" in p} <= {1, 4} and (True, False) not in {(p["lin"], p["xw"]) for p in plans}
    assert all(not p["tree"] and p["cpr"] == 1 for p in map(lambda s: _plain_plan(*s), old_plain))
    # the sweeps: every residue of the 128-pixel tile's 32-pixel chunks, both guarded widths of G1
    assert {(H * W) % 32 for H, W in FFM_SWEEP_HW} == set(range(32)) and len(FFM_SWEEP_HW) == 69 and len(FFM_UP_SWEEP) == 36
    assert [_gk(Co, 35, 2, Co)[0] for Co in FFM_SWEEP_CO] == [1, 2]
    up_plans = [_up_plan(2, 128, 256, 256, 64, *g) for g in FFM_UP_SWEEP]
    assert {p["lin"] for p in up_plans} == {True, False} and {p["xw"] for p in up_plans} == {True, False}
    assert {"fz" in p for p in up_plans} == {True, False} and max(p.get("lds", 0) for p in up_plans) <= 160 * 1024


# ------------------------------------------------------------------------------------------------ shared pieces: attention
def _attn_inputs(nb, Kc, Vc, n, seed):
    """The inputs of test_attn_autograd_vs_oracle: non-negative queries, as the model's ReLU leaves them."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(nb, Kc, n, generator=gen).relu()
    k, v, g = (torch.randn(nb, c, n, generator=gen) for c in (Kc, Vc, Vc))
    return q, k, v, g


def _attn_oracle(q, k, v, g, scale):
    q, k, v, g = (t.double() for t in (q, k, v, g))
    ctx, lse = attn_core_fwd(q, k, v, scale)
    dq, dk, dv = attn_core_bwd(g, q, k, v, ctx, lse, scale)
    return dict(ctx=ctx, lse=lse, dq=dq, dk=dk, dv=dv)


def _nan_ws(nbytes, dev):
    """A workspace whose every float is a NaN bit pattern: the wrappers hand over torch.empty memory, so the kernels may assume
    nothing about it."""
    return (torch.full((nbytes,), 255, dtype=torch.uint8, device=dev), nbytes) if nbytes else (None, 0)


def _attn_direct(q, k, v, g, scale, prec=0, backward=True):
    """cabinet_cab_attn_fwd (and _bwd on its results) on device tensors, every output and the workspaces NaN before the call."""
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle

    lib = _lib.load()
    B, Kc, n = q.shape
    Vc, nan, st = v.shape[1], float("nan"), _stream_handle(q.device)
    ctx, lse = torch.full_like(v, nan), torch.full((B, n), nan, device=q.device)
    ws, nbytes = _nan_ws(lib.cabinet_cab_attn_fwd_workspace_bytes(B, Kc, Vc, n, prec), q.device)
    _lib.check(lib.cabinet_cab_attn_fwd(_ptr(q), _ptr(k), _ptr(v), float(scale), B, Kc, Vc, n, prec, _ptr(ctx), _ptr(lse), _ptr(ws), nbytes, st),
               "cabinet_cab_attn_fwd")
    out = dict(ctx=ctx, lse=lse)
    if backward:
        dq, dk, dv = torch.full_like(q, nan), torch.full_like(k, nan), torch.full_like(v, nan)
        ws, nbytes = _nan_ws(lib.cabinet_cab_attn_bwd_workspace_bytes(B, Kc, Vc, n), q.device)
        _lib.check(lib.cabinet_cab_attn_bwd(_ptr(g), _ptr(q), _ptr(k), _ptr(v), _ptr(ctx), _ptr(lse), float(scale), B, Kc, Vc, n, _ptr(dq),
                                            _ptr(dk), _ptr(dv), _ptr(ws), nbytes, st), "cabinet_cab_attn_bwd")
        out.update(dq=dq, dk=dk, dv=dv)
    return out


ATTN_TOL = dict(ctx=2e-5, lse=1e-5, dq=5e-5, dk=5e-5, dv=5e-5)   # test_attn_autograd_vs_oracle / test_attn_fwd_golden


def _attn_check(fails, tag, dev, ref, precs=()):
    """fp32 results against fp64 by conftest.assert_close's rule; the split-bf16 forwards by test_attn_fwd_split_bf16_vs_fp64's."""
    for name, tol in ATTN_TOL.items():
        if name in dev[0]:
            _cmp(fails, tag, name, dev[0][name], ref[name], tol=tol)
    for prec, res in precs:
        for name in ("ctx", "lse"):
            if not bool(torch.isfinite(res[name]).all()):
                fails.append(f"{tag} precision {prec} {name}: not finite")
                continue
            e32, e = rel_err(dev[0][name], ref[name]), rel_err(res[name], ref[name])
            if prec == 2 and not e <= max(2 * e32, 1e-6):
                fails.append(f"{tag} bf16x6 {name}: {e:.2e} > max(2 x fp32 {e32:.2e}, 1e-6)")
            if prec == 1 and not e < 5e-5:
                fails.append(f"{tag} bf16x3 {name}: {e:.2e} >= 5e-5 (fp32 {e32:.2e})")


def _attn_case(fails, shape, seed, backward=True, bf16=True, twice=False):
    B, Kc, Vc, n = shape
    scale = Kc ** -0.5
    cpu = _attn_inputs(B, Kc, Vc, n, seed)
    ref = _attn_oracle(*cpu, scale)
    t = [x.cuda() for x in cpu]
    dev = [_attn_direct(*t, scale, 0, backward) for _ in range(2 if twice else 1)]
    precs = [(p, _attn_direct(*t, scale, p, False)) for p in (2, 1)] if bf16 and (Kc, Vc) in BF16_PAIRS else []
    _attn_check(fails, f"attention {shape}", dev, ref, precs)
    if twice and not _all_equal(list(dev[0].values()), list(dev[1].values())):
        fails.append(f"attention {shape}: two runs differ")
    return dev[0], ref


# ------------------------------------------------------------------------------------------------ shared pieces: FFM
FFM_MAPS = ("out", "dfsp", "dxc")


@functools.lru_cache(maxsize=4)
def _ffm_case(shape, training, seed=None):
    """Inputs (test_gpu_ffm.py's distributions), the fp64 oracle and the number of ReLU inputs of the oracle within KINK of zero."""
    B, Cs, Cc, Co, Cm, H, W = shape[:7]
    up = len(shape) == 9
    seed = FFM_SEEDS.get((shape, training), 0) if seed is None else seed
    gen = torch.Generator().manual_seed(100003 * seed + 7 * sum(shape) + H + int(training))
    fsp = torch.randn(B, Cs, H, W, generator=gen)
    xc = torch.randn(B, Cc, *(shape[7:] if up else (H, W)), generator=gen)
    wb = torch.randn(Co, Cs + Cc, 1, 1, generator=gen) * (2.0 / (Cs + Cc)) ** 0.5
    w1, w2 = torch.randn(Cm, Co, 1, 1, generator=gen) * 0.1, torch.randn(Co, Cm, 1, 1, generator=gen) * 0.1
    g = torch.randn(B, Co, H, W, generator=gen)
    bn = _set_bn(torch.nn.BatchNorm2d(Co), gen).train(training)
    d = lambda t: t.detach().double()  # noqa: E731
    x64 = xc.double().requires_grad_(up)
    fcp = F.interpolate(x64, size=(H, W), mode="bilinear", align_corners=False) if up else x64
    fw = ffm_fwd(fsp.double(), fcp.detach(), d(wb).flatten(1), d(bn.weight), d(bn.bias), d(bn.running_mean), d(bn.running_var),
                 d(w1).flatten(1), d(w2).flatten(1), training)
    gr = ffm_bwd(g.double(), fw, d(wb).flatten(1), d(bn.weight), d(w1).flatten(1), d(w2).flatten(1), training, Cs)
    if up:
        fcp.backward(gr["dfcp"])
    ref = dict(out=fw["out"], dfsp=gr["dfsp"], dxc=x64.grad if up else gr["dfcp"], dw_blk=gr["dw_blk"].view_as(wb), dbn_w=gr["dbn_w"],
               dbn_b=gr["dbn_b"], dw1=gr["dw1"].view_as(w1), dw2=gr["dw2"].view_as(w2), running_mean=fw["new_running_mean"],
               running_var=fw["new_running_var"])
    pre = (fw["z"] - fw["mean"].view(1, -1, 1)) * (fw["invstd"] * d(bn.weight)).view(1, -1, 1) + d(bn.bias).view(1, -1, 1)
    near = int((pre.abs() < KINK).sum()) + int((fw["u"].abs() < KINK).sum())
    return dict(inputs=(fsp, xc, wb, w1, w2), g=g, bn=bn, ref=ref, near=near, up=up, training=training)


def _ffm_dev(case):
    from cabinet_amd.functional import ffm_fused, ffm_fused_upsampled

    bn = copy.deepcopy(case["bn"]).cuda().train(case["training"])
    t = [x.cuda().requires_grad_(True) for x in case["inputs"]]
    out = (ffm_fused_upsampled if case["up"] else ffm_fused)(t[0], t[1], t[2], bn, t[3], t[4])
    out.backward(case["g"].cuda())
    return dict(out=out.detach(), dfsp=t[0].grad, dxc=t[1].grad, dw_blk=t[2].grad, dbn_w=bn.weight.grad, dbn_b=bn.bias.grad, dw1=t[3].grad,
                dw2=t[4].grad, running_mean=bn.running_mean, running_var=bn.running_var)


def _ffm_compare(fails, tag, res, ref):
    for name, b in ref.items():
        _cmp(fails, tag, name, res[name], b, maxnorm=name in FFM_MAPS, tol=1e-5 if name.startswith("running") else TOL)


def _ffm_check_kinks(shape, case):
    if shape in FFM_BIG:
        m = 3.2e-6 * shape[0] * shape[3] * shape[5] * shape[6]
        print(f"ffm {shape}: {case['near']} ReLU inputs of the fp64 oracle within {KINK} of zero (left to the double re-decision)")
        assert case["near"] <= m + 5 * m ** 0.5, f"ffm {shape}: {case['near']} ReLU inputs within {KINK} of zero, {m:.1f} expected at the most"
    else:
        assert case["near"] == 0, f"ffm {shape} training={case['training']}: {case['near']} ReLU inputs within {KINK} of zero: another seed"


def _ffm_run_case(shape, training):
    case = _ffm_case(shape, training)
    _ffm_check_kinks(shape, case)
    runs = [_ffm_dev(case) for _ in range(2)]
    torch.cuda.synchronize()
    fails = []
    _ffm_compare(fails, f"ffm {shape} training={training}", runs[0], case["ref"])
    print(f"ffm {shape} training={training}: " + "  ".join(f"{k} {rel_err(runs[0][k], b):.1e}" for k, b in case["ref"].items()))
    assert not fails, "\n".join(fails)
    assert _all_equal(list(runs[0].values()), list(runs[1].values())), "two runs differ"
    return runs[0]


# ------------------------------------------------------------------------------------------------ 1. plan-branch cases
@gpu
@pytest.mark.parametrize("shape", list(ATTN_CASES), ids=lambda s: "x".join(map(str, s)))
def test_attn_plan_branches(shape):
    """K1 and K2 through the C ABI at one shape per branch of `launch_dq_direct`, `dq_ksplit`, `bwd_nsplit`, the stored-dS decision
    and the forward's split and kernel choice (ATTN_CASES): NaN-prefilled outputs and workspaces, fp64 oracle, two runs bit-equal;
    the split-bf16 forwards where the pair has them."""
    fails = []
    _attn_case(fails, shape, 4000 + shape[0] + shape[3], twice=True)
    assert not fails, "\n".join(fails)


@gpu
@pytest.mark.parametrize("shape", list(ATTN_DS_CAP), ids=lambda s: "x".join(map(str, s)))
def test_attn_bwd_either_side_of_the_ds_cap(shape):
    """The recompute kernels at n % 4 == 0 (129 images: dS would be 541 MB) and the stored-dS form at exactly DS_MAX_BYTES (128
    images).  The batch repeats three distinct images (image b = pattern b % 3), so three fp64 evaluations check every image."""
    B, Kc, Vc, n = shape
    scale = Kc ** -0.5
    cpu = _attn_inputs(3, Kc, Vc, n, 77)
    ref = _attn_oracle(*cpu, scale)
    idx = torch.arange(B) % 3
    t = [x[idx].contiguous().cuda() for x in cpu]
    runs = [_attn_direct(*t, scale) for _ in range(2)]
    torch.cuda.synchronize()
    fails = []
    for name, tol in ATTN_TOL.items():
        a = runs[0][name]
        if not bool(torch.isfinite(a).all()):
            fails.append(f"{name}: not finite")
        for p in range(3):   # conftest.assert_close's rule per pattern, over all its images at once
            b = ref[name][p].cuda()
            diff = a[p::3].double() - b
            err, den, cnt = float(diff.norm()), float(b.norm()) * (diff.shape[0] ** 0.5), diff.numel()
            print(f"attention {shape} {name} pattern {p}: rel {err / den:.2e}")
            if not err <= tol * den + 1e-6 * cnt ** 0.5:
                fails.append(f"{name} pattern {p}: rel {err / den:.2e} > {tol}")
    assert not fails, "\n".join(fails)
    assert _all_equal(list(runs[0].values()), list(runs[1].values()))


@gpu
@pytest.mark.parametrize("shape", list(FFM_PLAIN), ids=lambda s: "x".join(map(str, s)))
def test_ffm_plain_plan_branches(shape):
    """`ffm_fused` at one shape per branch of FFM_PLAIN, training mode."""
    _ffm_run_case(shape, True)


@gpu
@pytest.mark.parametrize("shape", FFM_PLAIN_EVAL, ids=lambda s: "x".join(map(str, s)))
def test_ffm_plain_plan_branches_eval(shape):
    _ffm_run_case(shape, False)


@gpu
@pytest.mark.parametrize("shape", list(FFM_UP), ids=lambda s: "x".join(map(str, s)))
def test_ffm_upsampled_plan_branches(shape):
    """`ffm_fused_upsampled` at one shape per branch of FFM_UP, training mode; the 122 KB band runs after a band of a few KB in the
    same process (the LDS attribute is set once per device)."""
    if _up_plan(*shape).get("lds", 0) > 100 * 1024:
        _ffm_run_case(FFM_SMALL_BEFORE_CAP, True)
    _ffm_run_case(shape, True)


@gpu
def test_ffm_up_bwd_refuses_a_band_above_the_lds_cap():
    """A x16 resize of a 256-pixel row: one band of the two-pass adjoint would stage 197 KB.  The forward runs; the backward raises
    and names the geometry (it used to report a bare `invalid argument` after launching its reduction kernels); an ordinary call
    before and after gives the same bits."""
    before = _ffm_dev(_ffm_case(FFM_SMALL_BEFORE_CAP, True))
    case = _ffm_case(FFM_REFUSED, True)
    # (the message travels in the exception: cabinet_last_error is per thread, and autograd runs the backward on its own)
    with pytest.raises(RuntimeError, match=r"cabinet_ffm_up_bwd failed.*resize 2x16 -> 32x256 is refused.*197344 bytes of LDS"):
        _ffm_dev(case)
    torch.cuda.synchronize()
    after = _ffm_dev(_ffm_case(FFM_SMALL_BEFORE_CAP, True))
    assert _all_equal(list(before.values()), list(after.values()))


# ------------------------------------------------------------------------------------------------ 3. dense sweeps
@gpu
@pytest.mark.parametrize("Kc,Vc", PAIRS)
def test_attn_residue_sweep(Kc, Vc):
    """n = 1 .. 136, B = 2: every residue of the 32-key tile and of 4, up to just past the point where all eight waves of the
    two-waves-per-SIMD kernels own a tile; forward (fp32 and both split-bf16 forms) and backward against fp64."""
    fails, ran = [], 0
    for n in ATTN_SWEEP_N:
        _attn_case(fails, (2, Kc, Vc, n), 9000 + n)
        ran += 1
    _report(fails, ran, 136)


@gpu
@pytest.mark.parametrize("Kc,Vc", PAIRS)
def test_attn_split_threshold_sweep(Kc, Vc):
    """B = 1 either side of every n at which the forward's key split, the backward's query split or the kernel choice changes:
    nt = 15 | 16 key tiles (n = 480 | 481), 31 | 32 (992 | 993), n % 4 and n % 32 around them, and the 512 / 516 pair of `dq_ksplit`."""
    fails, ran = [], 0
    for n in ATTN_EDGE_N:
        _attn_case(fails, (1, Kc, Vc, n), 9500 + n)
        ran += 1
    _report(fails, ran, 16)


@gpu
@pytest.mark.parametrize("Kc,Vc", BF16_PAIRS)
def test_attn_proj_residue_sweep(Kc, Vc):
    """`cab_attention_proj` (K1 with the projection in its epilogue) at Co = 96 and n = 4, 8, .. 136, B = 2: 2e-5 forward, 1e-4
    gradients against the fp64 composite of test_gpu_attn.py."""
    from cabinet_amd.functional import cab_attention_proj, cab_attention_proj_supported

    fails, ran, scale = [], 0, Kc ** -0.5
    for n in range(4, 137, 4):
        gen = torch.Generator().manual_seed(9900 + n)
        q = torch.randn(2, Kc, n, generator=gen).relu()
        k, v, g = torch.randn(2, Kc, n, generator=gen), torch.randn(2, Vc, n, generator=gen), torch.randn(2, 96, n, generator=gen)
        w = torch.randn(96, Vc, 1, 1, generator=gen) * Vc ** -0.5
        ref = t_attn._proj_reference(q, k, v, w.flatten(1), g, scale)
        t = [x.cuda().requires_grad_(True) for x in (q, k, v, w)]
        if not cab_attention_proj_supported(t[0], t[2], t[3]):
            fails.append(f"n={n}: the fused form did not take the shape")
        glob = cab_attention_proj(*t[:3], t[3], scale)
        glob.backward(g.cuda())
        tag = f"attention + projection ({Kc}, {Vc}) n={n}"
        _cmp(fails, tag, "glob", glob, ref[0], tol=2e-5)
        for name, a, b in zip(("dq", "dk", "dv", "dw_out"), (t[0].grad, t[1].grad, t[2].grad, t[3].grad.flatten(1)), ref[2:]):
            _cmp(fails, tag, name, a, b, tol=1e-4)
        ran += 1
    _report(fails, ran, 34)


def _sweep_modes(shapes):
    """Every shape in training and in eval mode."""
    return [(s, training) for s in shapes for training in (True, False)]


DZ_GRADS = ("dfsp", "dxc", "dw_blk")


def _two_sample_bounds(case):
    """For a training-mode case with two samples per channel: per gradient that flows through dz, 2 x the distance (tensor norm,
    max norm) of the oracle's formulas evaluated in fp32 from the fp64 result (module docstring).  Plain form only."""
    f = lambda t: t.detach().float()  # noqa: E731
    fsp, xc, wb, w1, w2 = (f(t) for t in case["inputs"])
    bn, Cs = case["bn"], fsp.shape[1]
    fw = ffm_fwd(fsp, xc, wb.flatten(1), f(bn.weight), f(bn.bias), f(bn.running_mean), f(bn.running_var), w1.flatten(1), w2.flatten(1), True)
    gr = ffm_bwd(f(case["g"]), fw, wb.flatten(1), f(bn.weight), w1.flatten(1), w2.flatten(1), True, Cs)
    got = dict(dfsp=gr["dfsp"], dxc=gr["dfcp"], dw_blk=gr["dw_blk"].view_as(wb))
    out = {}
    for name in DZ_GRADS:
        a, b = got[name].double(), case["ref"][name]
        out[name] = (2 * float((a - b).norm() / b.norm()), 2 * float((a - b).abs().max() / b.abs().max()))
    return out


def _plain_sweep_shapes(Co):
    return [(2, 32, 64, Co, 24, H, W) for H, W in FFM_SWEEP_HW]


def _up_sweep_shapes():
    return [(2, 128, 256, 256, 64, *g) for g in FFM_UP_SWEEP]


def _ffm_sweep(shapes):
    fails, ran = [], 0
    for shape, training in _sweep_modes(shapes):
        case = _ffm_case(shape, training)
        tag = f"ffm {shape} training={training}"
        if case["near"]:
            fails.append(f"{tag}: {case['near']} ReLU inputs within {KINK} of zero: another seed")
        res, ref = _ffm_dev(case), case["ref"]
        if training and shape[0] * shape[5] * shape[6] == 2:   # two samples per channel: see the module docstring
            for name, (e2, m2) in _two_sample_bounds(case).items():
                a, b = res[name].double().cpu(), ref[name]
                e, m = float((a - b).norm() / b.norm()), float((a - b).abs().max() / b.abs().max())
                print(f"{tag} {name}: kernel {e:.2e} (max norm {m:.2e}), 2 x the fp32 evaluation {e2:.2e} ({m2:.2e})")
                if not (bool(torch.isfinite(a).all()) and e <= max(TOL, e2) and (name == "dw_blk" or m <= max(TOL, m2))):
                    fails.append(f"{tag} {name}: {e:.2e} / max norm {m:.2e} against max(1e-3, {e2:.2e} / {m2:.2e})")
            ref = {k: v for k, v in ref.items() if k not in DZ_GRADS}
        _ffm_compare(fails, tag, res, ref)
        ran += 1
    return fails, ran


@gpu
@pytest.mark.parametrize("Co", FFM_SWEEP_CO)
def test_ffm_plain_residue_sweep(Co):
    """`ffm_fused` (32 | 64 -> Co, B = 2) on planes of 1..40 and 120..136 pixels and on (3, 4, 5) x (31, 32, 33, 43): every residue of
    the 128-pixel tile's 32-pixel chunks, vector and scalar rows, `gemm_kmajor_kernel<1>` (Co = 96) and `<2, guarded>` (Co = 192);
    every plane in training and in eval mode."""
    fails, ran = _ffm_sweep(_plain_sweep_shapes(Co))
    _report(fails, ran, 2 * 69)


@gpu
def test_ffm_upsampled_residue_sweep():
    """`ffm_fused_upsampled` (128 | 256 -> 256, B = 2) at the x4 ratio for Hl = 1..10 and Wl in {4, 8, 16} -- band edges of the
    linear adjoint, of the two-pass adjoint and of the fused forward (W = 64) -- and at the non-integer ratios 7/3, 9/4, 30/7 with
    Wl in {3, 5}; every geometry in training and in eval mode."""
    fails, ran = _ffm_sweep(_up_sweep_shapes())
    _report(fails, ran, 2 * 36)


# ------------------------------------------------------------------------------------------------ 4. caller contract
def _ffm_modules(Cs, Cc, Co, Cm, seed):
    gen = torch.Generator().manual_seed(seed)
    ws = [torch.randn(Co, Cs + Cc, 1, 1, generator=gen) * 0.07, torch.randn(Cm, Co, 1, 1, generator=gen) * 0.1, torch.randn(Co, Cm, 1, 1, generator=gen) * 0.1]
    bn = _set_bn(torch.nn.BatchNorm2d(Co), gen).cuda().train()
    return [w.cuda().requires_grad_(True) for w in ws], bn


def _contract_attention():
    from cabinet_amd.functional import cab_attention

    return (lambda q, k, v: cab_attention(q, k, v, 64 ** -0.5)), [], []


def _contract_attention_proj():
    from cabinet_amd.functional import cab_attention_proj, cab_attention_proj_supported

    w = (torch.randn(96, 64, generator=torch.Generator().manual_seed(8)) * 64 ** -0.5).cuda().requires_grad_(True)

    def fn(q, k, v):
        assert cab_attention_proj_supported(q, v, w)
        return cab_attention_proj(q, k, v, w, 64 ** -0.5)

    return fn, [w], []


def _contract_ffm():
    from cabinet_amd.functional import ffm_fused

    (wb, w1, w2), bn = _ffm_modules(32, 64, 192, 24, 9)
    return (lambda fsp, fcp: ffm_fused(fsp, fcp, wb, bn, w1, w2)), [wb, w1, w2] + list(bn.parameters()), [bn.running_mean, bn.running_var]


def _contract_ffm_up():
    from cabinet_amd.functional import ffm_fused_upsampled

    (wb, w1, w2), bn = _ffm_modules(64, 96, 96, 24, 10)
    return (lambda fsp, low: ffm_fused_upsampled(fsp, low, wb, bn, w1, w2)), [wb, w1, w2] + list(bn.parameters()), [bn.running_mean, bn.running_var]


CONTRACT = {
    "cab_attention": (_contract_attention, [(1, 64, 485)] * 3),                       # ragged n, key split, recompute backward
    "cab_attention_proj": (_contract_attention_proj, [(2, 64, 36)] * 3),              # a ragged second tile in the fused epilogue
    "ffm_fused": (_contract_ffm, [(2, 32, 5, 7), (2, 64, 5, 7)]),                      # gemm_kmajor_kernel<2, guarded>, odd P
    "ffm_fused_upsampled": (_contract_ffm_up, [(1, 64, 3, 5), (1, 96, 7, 9)]),         # a shrinking resize
}


@gpu
@pytest.mark.parametrize("name", list(CONTRACT))
def test_attn_ffm_wrappers_accept_any_layout(name):
    """Transposed (3-D) / channels_last (4-D) inputs, inputs that start 4 bytes into their storage, a non-contiguous output gradient
    (backward through a transposed view) and a stride-0 one (y.sum().backward()): the wrappers copy such operands and the kernels
    are bit-reproducible, so outputs, every gradient and the running buffers are bit for bit those of the dense, aligned call
    (the precedent: test_backbone_wrappers_accept_any_layout)."""
    build, shapes = CONTRACT[name]
    gen = torch.Generator().manual_seed(45)
    xs = [(torch.randn(*s, generator=gen) * 1.3 + 0.2).cuda() for s in shapes]
    xs_cl, xs_off = [_restrided(x) for x in xs], [_offset(x) for x in xs]
    for x, c, o in zip(xs, xs_cl, xs_off):
        assert not c.is_contiguous() and o.is_contiguous() and o.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
        assert torch.equal(c, x) and torch.equal(o, x)
    g = None

    def run(inputs, mode):
        nonlocal g
        fn, params, buffers = build()   # fresh, identically seeded parameters and running buffers
        inputs = [x.detach().requires_grad_(True) for x in inputs]
        y = fn(*inputs)
        if g is None:
            g = torch.randn(y.shape, generator=gen).cuda()
        if mode == "dense":
            y.backward(g)
        elif mode == "transposed":
            y.transpose(-1, -2).backward(g.transpose(-1, -2).contiguous())
        elif mode == "ones":
            y.backward(torch.ones_like(y))
        else:
            y.sum().backward()
        assert all(x.grad is not None for x in inputs) and all(p.grad is not None for p in params)
        return [y.detach()] + [x.grad for x in inputs] + [p.grad for p in params] + [b.clone() for b in buffers]

    base = run(xs, "dense")
    for what, got in (("transposed / channels_last inputs", run(xs_cl, "dense")), ("inputs 4 bytes into their storage", run(xs_off, "dense")),
                      ("non-contiguous grad_output", run(xs, "transposed"))):
        bad = [i for i, (a, b) in enumerate(zip(got, base)) if not torch.equal(a, b)]
        assert len(got) == len(base) and not bad, f"{name}, {what}: tensors {bad} differ from the dense, aligned call"
    ones, summed = run(xs, "ones"), run(xs, "sum")
    bad = [i for i, (a, b) in enumerate(zip(summed, ones)) if not torch.equal(a, b)]
    assert not bad, f"{name}, stride-0 grad_output: tensors {bad} differ from the dense call"
