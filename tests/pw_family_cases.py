"""Case tables, plan readers and fp64 formulas for the tests of the thin 1x1 convolution family: K10's stream kernels
(csrc/pwconv.hip), K14's weight gradient and the BN form (csrc/pwconv_wide.hip), the SE MLP adjoint (csrc/se_mlp.hip).
Shared by tests/test_pw_family_plans.py (no GPU) and tests/test_gpu_pw_family_edges.py.  No device work at import.

The kernels are templates and the host picks the instantiation from the shape and the pointer alignment.  Every table below is
written so that the library's own plan queries (cabinet_pwconv_stream_plan, cabinet_pwconv_wide_plan, cabinet_pw_bn_bwd_plan)
put its cases on the instantiations named beside them; test_pw_family_plans.py holds the tables against those queries, so a
retuned plan constant turns that file red instead of letting the coverage lapse."""
import ctypes


CHANNELS = tuple(range(8, 129, 8))  # the sweep of both channel counts; the library says which pairs it takes
EPS32 = 2.0 ** -23


def load_library():
    from cabinet_amd import _lib

    return _lib.load()


# ================================================================================================ K10: the stream kernels
# An instantiation is ("pipe", MB, KQ, V) = pw_stream_kernel<MB, KQ, V> or ("plain", MB, 0, 1) = pw_stream_plain_kernel<MB>, for the
# M x K product of one direction: forward M = Co, K = Ci; input gradient M = Ci, K = Co.  MB = ceil(M / 32), KQ = ceil(K / 16).
K10_B = 2
K10_PLANES = (196, 194, 193)  # 16-byte form where it fits, else 8-byte (last 128- / 64-pixel block partial) | 8-byte form, 2 live
#                               pixels in the last block | dword form
K10_FORM_P = 260              # P % 4 == 0, two full 128-pixel blocks and 4 pixels
K10_FORM_OFFSETS = (0, 8, 4)  # bytes from 16-byte alignment of x and y: V = 4 (where it fits, else 2), 2, 1
K10_LOADED_B = 3
K10_LOADED_BLOCKS = 4203      # 3 x 1401 blocks on the 2048-workgroup grid: walks of 2 and 3 across image borders, ragged last block
K10_LOADED_P = {4: 128 * 1400 + 36, 2: 64 * 1400 + 38, 1: 64 * 1400 + 37}
K10_PLAIN_LOADED_P = 64 * 1364 + 38  # 3 x 1365 = 4095 blocks of 64 pixels: the last count at which <1,5,*> keeps the plain walk
GRID_CAP = 2048               # 256 CUs x 8 one-wave workgroups (pwconv_pipeline_cases.GRID_CAP: the documented restatement)


def mbkq(M, K):
    return -(-M // 32), -(-K // 16)


def k10_pairs(lib, P=K10_PLANES[0]):
    """Every (Ci, Co) in multiples of 8 up to 128 that cabinet_pwconv_supported takes."""
    return [(ci, co) for ci in CHANNELS for co in CHANNELS if lib.cabinet_pwconv_supported(ci, co, P) == 1]


def stream_plan(lib, B, M, K, P, x_off=0, y_off=0):
    """cabinet_pwconv_stream_plan -> (pipelined, V, pixels per block, blocks)."""
    out = (ctypes.c_int * 4)()
    rc = lib.cabinet_pwconv_stream_plan(B, M, K, P, x_off, y_off, out)
    assert rc == 0, lib.cabinet_last_error()
    return tuple(out)


def k10_inst(lib, B, M, K, P, x_off=0, y_off=0):
    """-> (instantiation, blocks)."""
    pipelined, v, px, nblocks = stream_plan(lib, B, M, K, P, x_off, y_off)
    mb, kq = mbkq(M, K)
    assert px == (128 if v == 4 else 64) and nblocks == B * -(-P // px)
    return (("pipe", mb, kq, v) if pipelined else ("plain", mb, 0, 1)), nblocks


def k10_rep_product(mb, kq):
    """One (M, K) per (MB, KQ): M = 32 MB - 8 (the last row block has 8 rows past M), K alternately 16 KQ - 8 (the last four slots
    of the walk lie past K and their MFMAs are skipped) and 16 KQ; 128 channels are past the operator's LDS limit."""
    return 32 * mb - 8, min(16 * kq - (8 if (mb + kq) % 2 else 0), 120)


def k10_mbkq(lib):
    """The (MB, KQ) the operator's shapes give, from the library's own support rule."""
    return sorted({mbkq(co, ci) for ci, co in k10_pairs(lib)})


def k10_sweep_products(lib):
    """Table (a): (B, M, K, P, x_off, y_off) of every product tests (a) launch: both directions of every pair, aligned."""
    out = []
    for ci, co in k10_pairs(lib):
        for P in K10_PLANES:
            out += [(K10_B, co, ci, P, 0, 0), (K10_B, ci, co, P, 0, 0)]
    return out


def k10_form_cases(lib):
    """Table (b): (Ci, Co) = (K, M) of k10_rep_product per (MB, KQ); the test runs y (M = Co) and dx (M = Ci) at the three offsets."""
    return [(k, m) for m, k in (k10_rep_product(mb, kq) for mb, kq in k10_mbkq(lib))]


def k10_form_products(lib):
    out = []
    for ci, co in k10_form_cases(lib):
        for off in K10_FORM_OFFSETS:
            out += [(K10_B, co, ci, K10_FORM_P, off, off), (K10_B, ci, co, K10_FORM_P, off, off)]
    return out


def k10_loaded_cases(lib):
    """Table (c): (Ci, Co, P) -- the forward of Ci -> Co is the M = Co, K = Ci product -- one per pipelined instantiation at 4203
    blocks, and the plain walks: <1> at 4095 blocks of the product that is pipelined past 4096, <2> at 4203."""
    out = []
    for mb, kq in k10_mbkq(lib):
        m, k = k10_rep_product(mb, kq)
        for v in (4, 2, 1):
            P = K10_LOADED_P[v]
            inst, nblocks = k10_inst(lib, K10_LOADED_B, m, k, P)
            if inst == ("pipe", mb, kq, v):
                assert nblocks == K10_LOADED_BLOCKS
                out.append((k, m, P))
    out.append((k10_rep_product(1, 5)[1], k10_rep_product(1, 5)[0], K10_PLAIN_LOADED_P))
    out.append((k10_rep_product(2, 2)[1], k10_rep_product(2, 2)[0], K10_LOADED_P[2]))
    return out


def k10_loaded_products(lib):
    return [(K10_LOADED_B, co, ci, P, 0, 0) for ci, co, P in k10_loaded_cases(lib)]


# The input gradient under the same load: A = W^T, read through the strides (sm, sk) = (1, Ci), M = Ci, K = Co.  (Ci, Co, P) and the
# instantiation of the dx product, one per vector form.
K10_LOADED_DX_CASES = [((16, 24, K10_LOADED_P[4]), ("pipe", 1, 2, 4)), ((120, 56, K10_LOADED_P[2]), ("pipe", 4, 4, 2)),
                       ((24, 88, K10_LOADED_P[1]), ("pipe", 1, 6, 1))]


def k10_expected_instantiations():
    """The instantiations pwconv.hip can launch, restated from its templates: MB x ceil(KQ / 2) <= 8 row-block products; the plain
    walk owns <2,2> (and <1,5> up to 4096 blocks); the 16-byte form where 4 (32 MB + 8 KQ) registers stay within 224."""
    out = {("plain", 1, 0, 1), ("plain", 2, 0, 1)}
    for mb in range(1, 5):
        for kq in range(1, 9):
            if mb * ((kq + 1) // 2) > 8 or (mb, kq) == (2, 2):
                continue
            out |= {("pipe", mb, kq, 2), ("pipe", mb, kq, 1)}
            if 4 * (32 * mb + 8 * kq) <= 224:
                out.add(("pipe", mb, kq, 4))
    return out


def pw_ref(w, x):
    """fp64 product y[b][m][p] = sum_k w[m][k] x[b][k][p] and the product of the absolute values (the bound's scale)."""
    import torch

    w, x = w.double(), x.double()
    return torch.einsum("mk,bkp->bmp", w, x), torch.einsum("mk,bkp->bmp", w.abs(), x.abs())


def dot_bound_ratio(a, ref, scale, K):
    """max over elements of |a - ref| / (K 2^-23 (|A| |X|)): the textbook bound of a K-term fp32 dot product, doubled because the
    order of the two products inside the MFMA is undocumented.  <= 1 passes.  An element whose scale is 0 must be exactly ref."""
    import torch

    err = (a.double() - ref).abs()
    lim = K * EPS32 * scale
    ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(ratio.max())


# ================================================================================================ K14: pww_wgrad_kernel<BM, BN>
K14_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 2), (1, 4), (4, 1), (2, 4), (4, 2), (3, 3)]
K14_NEW_PAIRS = [(40, 40), (40, 72), (104, 8), (8, 104)]            # (Ci, Co): the tile shapes (2,2), (3,2), (1,4), (4,1)
# The same shapes with more than one tile, as the plan query confirms (K14_LARGE_PLANS): (3,2) x 3, (1,4) x 2, (4,1) x 2.  The
# plan never lays (2,2) tiles side by side (two of them cost more than one (2,4), (4,2) or two (2,3)): a sweep of the query over
# 1..16 row blocks either side finds none, so (40, 40) is all of that instantiation.  (136, 136), (136, 264) and (264, 40) -- first
# guesses -- are (3,3) and (2,3) plans, which test_gpu_pwconv_wide.py already launches.
K14_LARGE_PAIRS = [(40, 264), (200, 8), (8, 200)]
K14_LARGE_PLANS = {(40, 264): (3, 2, 3, 1), (200, 8): (1, 4, 1, 2), (8, 200): (4, 1, 2, 1)}  # (bm, bn, tiles_m, tiles_n)
K14_OTHER_PAIRS = [(8, 8), (40, 8), (8, 40), (72, 8), (8, 72), (72, 40), (104, 40), (40, 104), (96, 96)]  # the other nine
K14_PLANES = [(1, 323), (3, 64 * 65)]  # (B, P): ragged, one image | 3 x 65 chunks that split unevenly
K14_SWEEP_MAX = 512                    # the plan depends on the 32-row block counts only: up to 16 blocks either side


def wide_plan(lib, B, Ci, Co, P):
    """cabinet_pwconv_wide_plan -> (bm, bn, tiles_m, tiles_n, nsplit)."""
    out = (ctypes.c_int * 5)()
    rc = lib.cabinet_pwconv_wide_plan(B, Ci, Co, P, out)
    assert rc == 0, lib.cabinet_last_error()
    return tuple(out)


def k14_cases():
    """(B, Ci, Co, P): the seven pairs of the four new tile shapes at both planes, the other nine shapes at the first."""
    out = [(B, ci, co, P) for ci, co in K14_NEW_PAIRS + K14_LARGE_PAIRS for B, P in K14_PLANES]
    return out + [(K14_PLANES[0][0], ci, co, K14_PLANES[0][1]) for ci, co in K14_OTHER_PAIRS]


# ================================================================================================ BN form: pw_bn_bwd_kernel<BM, BN>
BN_SHAPES = [(bm, bn) for bm in (1, 2, 3) for bn in (1, 2, 3)]
BN_PAIRS = [(72, 40), (40, 72), (96, 64), (64, 96), (96, 40), (88, 24), (24, 88)]  # (Ci, Co): <2,3> <3,2> <2,3> <3,2> <2,3> <1,3> <3,1>
BN_SMALL_PAIRS = [(8, 8), (64, 24), (16, 64), (64, 64), (96, 96)]  # <1,1> <1,2> <2,1> <2,2> <3,3>: this table alone reaches all nine
BN_PS, BN_BS = (5, 129, 1000), (1, 3)
_ROT = [(a, t) for t in (True, False) for a in ("relu", "hardswish", "none")]  # the rotation of pw_bn_bwd_cases.ACT_CASES


def bn_plan(lib, B, Ci, Co, P, dx_off=0):
    """cabinet_pw_bn_bwd_plan -> (bm, bn, nsplit, vec, lds bytes)."""
    out = (ctypes.c_int * 5)()
    rc = lib.cabinet_pw_bn_bwd_plan(B, Ci, Co, P, dx_off, out)
    assert rc == 0, lib.cabinet_last_error()
    return tuple(out)


def bn_act_cases():
    """Rows in the form of pw_bn_bwd_cases.ACT_CASES: (B, Ci, Co, P, act, training, misalign, want_dx, want_dw)."""
    out, n = [], 0
    for ci, co in BN_PAIRS:
        for P in BN_PS:
            for B in BN_BS:
                act, training = _ROT[n % len(_ROT)]
                out.append((B, ci, co, P, act, training, 0, True, True))
                n += 1
    for ci, co in BN_SMALL_PAIRS:
        act, training = _ROT[n % len(_ROT)]
        out.append((1, ci, co, 129, act, training, 0, True, True))
        n += 1
    out.append((2, 72, 40, 1000, "relu", True, 1, True, True))        # x and dx 4 bytes off: dword stores on a P % 4 == 0 plane
    out.append((2, 40, 72, 129, "hardswish", True, 0, False, True))   # dX not requested
    out.append((2, 96, 64, 129, "relu", True, 0, True, False))        # dW not requested
    return out


BN_IDENTITY_CASES = [(2, 40, 72, 129, "relu", True), (3, 72, 40, 1000, "hardswish", True), (2, 96, 96, 65, "none", False)]
# (B, Ci, Co, P, act, training) with W = eye(Co, Ci): rows < min(Ci, Co) of dx are the chain's dz, the others exact zeros

# depthwise form: (B, Ci, C, H, W, K, stride, act, training), the K / stride mix of pw_bn_bwd_cases.DW_CASES
BN_DW_CASES = [
    (1, 16, 72, 1, 1, 3, 1, "relu", True),
    (2, 24, 88, 7, 9, 5, 2, "hardswish", True),
    (3, 40, 96, 7, 9, 3, 2, "none", False),
    (1, 16, 72, 33, 65, 5, 1, "relu", False),
    (2, 24, 88, 33, 65, 3, 2, "relu", True),
    (1, 40, 96, 33, 65, 3, 1, "hardswish", True),
    (2, 40, 96, 33, 65, 5, 2, "relu", True),
]

# the full 512-workgroup grid with four or five chunks each (pw_bn_bwd_cases.LOADED_CASE), for the two instantiations that run one
# workgroup per CU on more than 64 KB of LDS and had never been launched
BN_LOADED_CASES = [(1, 72, 40, 64 * 2103 + 36, "relu", True, 0, True, True),        # <2,3>
                   (1, 40, 72, 64 * 2103 + 36, "relu", True, 0, True, True)]        # <3,2>
# ReLU in both: with mean 0.5 and invstd 2 exact, the fp32 pre-activation is the rounded exact one and has its sign, so no unit
# decides differently in fp64 and the per-element check of the loaded test is sharp.  (hardswish's t = u + 3 rounds once more: on
# 9.7 million elements one or two land on the kink, in the fused form and the chain alike, 1.4e-4 from fp64 in the 2-norm.)


def bn_table_products():
    """(B, Ci, Co, P, dx_off) of every BN-form launch of the tables."""
    out = [(c[0], c[1], c[2], c[3], 4 if c[6] else 0) for c in bn_act_cases() + BN_LOADED_CASES]
    out += [(c[0], c[1], c[2], c[3], 0) for c in BN_IDENTITY_CASES]
    out += [(c[0], c[1], c[2], c[3] * c[4], 0) for c in BN_DW_CASES]
    return out


# ================================================================================================ SE MLP adjoint
# (B, C, Cs): Cs = 1; no multiples of 8 (the q < Q / cc < C guards, short last row slabs); image counts either side of a pass of
# eight (9, 16, 17); Cs > 256: the second column tile of launch A; the limit 1024 x 1024 (48 KB of LDS); C > 256 with Cs = 1000
SE_SHAPES = [(2, 8, 1), (3, 12, 5), (2, 100, 30), (9, 40, 16), (16, 72, 24), (17, 72, 24), (2, 520, 264), (1, 1024, 1024),
             (2, 1024, 256), (2, 257, 1000)]
SE_PS = (1, 1024)
# test_gpu_se_mlp_bwd._inputs zeroes the hidden activation of the last image: with one image nothing behind the ReLU would be live, so
# B = 1 keeps its image; and under seed 0 the single hidden unit of (2, 8, 1) is dead in image 0, under seed 1 it is alive.  The
# test asserts that dw1 and dw2 are nonzero in fp64 for every case.
SE_SEEDS = {(2, 8, 1): 1}


def se_input_args(shape):
    """-> keyword arguments of test_gpu_se_mlp_bwd._inputs for a shape of SE_SHAPES."""
    return dict(seed=SE_SEEDS.get(shape, 0), zero_image=shape[0] > 1)

SE_POISON_SHAPES = [(17, 72, 24), (2, 520, 264), (1, 1024, 1024)]
