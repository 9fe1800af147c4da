"""The tables of tests/pw_family_cases.py against the library's own launch plans (cabinet_pwconv_stream_plan,
cabinet_pwconv_wide_plan, cabinet_pw_bn_bwd_plan: the functions the launches themselves read).  No GPU: the queries are host-only.

Per kernel family: the instantiations the supported shapes can reach are enumerated by sweeping the query, and the tables of
tests/test_gpu_pw_family_edges.py must reach exactly that set -- which must also be the set restated from the templates.  A
retuned plan constant (the register budget of the 16-byte form, the plain / pipelined rule, a tile cost, the split target) moves
cases onto other instantiations and turns this file red; before it, every test stayed green while coverage lapsed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pw_bn_bwd_cases as bnc  # noqa: E402
import pw_family_cases as fc  # noqa: E402
import pwconv_pipeline_cases as k10  # noqa: E402


def _a256(n):
    return (n + 255) // 256 * 256


def _k10_configs():
    """(B, P, offset) of every plane and alignment the K10 tables use."""
    out = [(fc.K10_B, P, 0) for P in fc.K10_PLANES] + [(fc.K10_B, fc.K10_FORM_P, o) for o in fc.K10_FORM_OFFSETS]
    return out + [(fc.K10_LOADED_B, P, 0) for P in sorted(set(fc.K10_LOADED_P.values()) | {fc.K10_PLAIN_LOADED_P})]


def test_k10_tables_reach_every_stream_instantiation():
    lib = fc.load_library()
    pairs = fc.k10_pairs(lib)
    # the operator's shapes: 128 channels are past its LDS limit (32 x 4 x 129 floats > 64 KB), so 176 pairs, not 16 x 16 less the
    # row-block products above 8
    assert len(pairs) == 176 and all(max(p) <= 120 for p in pairs) and len(fc.k10_mbkq(lib)) == 24
    reachable, small_reachable = set(), set()
    for ci, co in pairs:
        for B, P, off in _k10_configs():
            for M, K in ((co, ci), (ci, co)):
                inst, nblocks = fc.k10_inst(lib, B, M, K, P, off, off)
                reachable.add(inst)
                if nblocks <= fc.GRID_CAP:
                    small_reachable.add(inst)
    expected = fc.k10_expected_instantiations()
    assert len(expected) == 51 and reachable == expected, (sorted(reachable - expected), sorted(expected - reachable))

    small = {fc.k10_inst(lib, *p) for p in fc.k10_sweep_products(lib) + fc.k10_form_products(lib)}
    loaded = {fc.k10_inst(lib, *p) for p in fc.k10_loaded_products(lib)}
    assert {i for i, _ in small} | {i for i, _ in loaded} == reachable
    # a small case (every block has a wave of its own: prologue and drain only) and a loaded one (4203 blocks on the 2048 grid: walks
    # of 2 and 3) for every pipelined instantiation.  <1,5,*> is pipelined only past 4096 blocks: no small case can exist.
    pipelined = {i for i in reachable if i[0] == "pipe"}
    assert len(pipelined) == 49
    assert all(n <= fc.GRID_CAP for _, n in small) and {i for i, _ in small} == small_reachable
    assert pipelined - small_reachable == {("pipe", 1, 5, 2), ("pipe", 1, 5, 1)}
    assert {i for i, n in loaded if i[0] == "pipe" and n == fc.K10_LOADED_BLOCKS} == pipelined
    assert fc.K10_LOADED_BLOCKS > 2 * fc.GRID_CAP and fc.K10_LOADED_BLOCKS % fc.GRID_CAP != 0
    assert all(P % px != 0 for v, P in fc.K10_LOADED_P.items() for px in (128 if v == 4 else 64,))  # ragged last block
    # the plain walks under load: <1> at the last block count that keeps it (one more image row of blocks is pipelined), <2>
    assert (("plain", 1, 0, 1), 4095) in loaded and (("plain", 2, 0, 1), fc.K10_LOADED_BLOCKS) in loaded
    m, k = fc.k10_rep_product(1, 5)
    assert fc.k10_inst(lib, fc.K10_LOADED_B, m, k, fc.K10_PLAIN_LOADED_P + 128)[0][0] == "pipe"
    assert len(fc.k10_loaded_cases(lib)) == 51
    for (ci, co, P), inst in fc.K10_LOADED_DX_CASES:  # the input gradient of Ci -> Co is the M = Ci, K = Co product
        assert fc.k10_inst(lib, fc.K10_LOADED_B, ci, co, P) == (inst, fc.K10_LOADED_BLOCKS)
    assert {inst[3] for _, inst in fc.K10_LOADED_DX_CASES} == {4, 2, 1}


def test_k10_planes_and_offsets_give_the_forms_they_are_there_for():
    lib = fc.load_library()
    for ci, co in fc.k10_pairs(lib):
        for M, K in ((co, ci), (ci, co)):
            mb, kq = fc.mbkq(M, K)
            got = [fc.stream_plan(lib, fc.K10_B, M, K, P) for P in fc.K10_PLANES]
            if all(g[0] for g in got):
                fits = 4 * (32 * mb + 8 * kq) <= 224
                assert [g[1] for g in got] == [4 if fits else 2, 2, 1], (M, K, got)
                # the last block of each plane is partial: 68 of 128 or 4 of 64 pixels | 2 of 64 | 1 of 64
                assert [P % g[2] for P, g in zip(fc.K10_PLANES, got)] == [68 if fits else 4, 2, 1]
            else:
                assert (mb, kq) in ((2, 2), (1, 5)) and not any(g[0] for g in got)
    for ci, co in fc.k10_form_cases(lib):
        for M, K in ((co, ci), (ci, co)):
            mb, kq = fc.mbkq(M, K)
            got = [fc.stream_plan(lib, fc.K10_B, M, K, fc.K10_FORM_P, o, o) for o in fc.K10_FORM_OFFSETS]
            if got[0][0]:
                assert [g[1] for g in got] == [4 if 4 * (32 * mb + 8 * kq) <= 224 else 2, 2, 1], (M, K, got)
    # one offset alone (x or y) decides as both do
    assert fc.stream_plan(lib, 2, 16, 16, 260, 0, 8)[1] == 2 and fc.stream_plan(lib, 2, 16, 16, 260, 4, 0)[1] == 1
    assert fc.stream_plan(lib, 2, 16, 16, 260, 16, 16)[1] == 4  # an alignment of 16 reads as offset 0
    out = (fc.ctypes.c_int * 4)()
    assert lib.cabinet_pwconv_stream_plan(2, 128, 16, 260, 0, 0, out) == -2  # unsupported
    assert lib.cabinet_pwconv_stream_plan(0, 16, 16, 260, 0, 0, out) == -1 and lib.cabinet_pwconv_stream_plan(2, 16, 16, 260, 0, 0, None) == -1


def test_k10_restatements_agree_with_the_query():
    """pwconv_pipeline_cases.stream_plan / vec_width / plain_form (what test_gpu_pwconv_pipeline.py's plan test reads) and the K10
    rows of test_gpu_backbone_edges.py, on their own cases."""
    import test_gpu_backbone_edges as be

    lib = fc.load_library()
    for B, Ci, Co, P, mis in k10.CASES:
        for M, K in ((Co, Ci), (Ci, Co)):
            v, px, nblocks, grid, walk = k10.stream_plan(B, M, K, P, not mis)
            pipelined, qv, qpx, qblocks = fc.stream_plan(lib, B, M, K, P, 4 if mis else 0, 4 if mis else 0)
            assert (v != 0, v if v else 1, px, nblocks) == (bool(pipelined), qv, qpx, qblocks), (B, M, K, P, mis)
            assert grid == min(qblocks, fc.GRID_CAP) and walk == -(-qblocks // grid)
    assert fc.GRID_CAP == k10.GRID_CAP
    for B, Ci, Co, H, W in be.K10_SHAPES:
        for M, K in ((Co, Ci), (Ci, Co)):
            assert fc.stream_plan(lib, B, M, K, H * W)[3] == 5120
    B, Ci, Co, H, W = be.K14_SHAPE
    assert fc.wide_plan(lib, B, Ci, Co, H * W)[4] == 512


def test_k14_tables_reach_every_tile_shape():
    lib = fc.load_library()
    reachable = set()
    for ci in range(8, fc.K14_SWEEP_MAX + 1, 8):
        for co in range(8, fc.K14_SWEEP_MAX + 1, 8):
            reachable.add(fc.wide_plan(lib, 1, ci, co, 323)[:2])
    assert reachable == set(fc.K14_SHAPES) and len(reachable) == 13
    reached = {}
    for B, ci, co, P in fc.k14_cases():
        assert lib.cabinet_pwconv_wide_supported(ci, co, P) == 1
        bm, bn, tm, tn, nsplit = fc.wide_plan(lib, B, ci, co, P)
        reached.setdefault((bm, bn), []).append((ci, co, tm, tn))
        assert tm == -(-co // (32 * bm)) and tn == -(-ci // (32 * bn))
        assert lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, ci, co, P) == _a256(nsplit * co * ci * 4)
        nchunks = B * -(-P // 64)
        assert nsplit == max(1, min(512 // (tm * tn), nchunks // 2))
    assert set(reached) == reachable
    assert [fc.wide_plan(lib, 1, ci, co, 323)[:2] for ci, co in fc.K14_NEW_PAIRS] == [(2, 2), (3, 2), (1, 4), (4, 1)]
    for pair, plan in fc.K14_LARGE_PLANS.items():
        assert fc.wide_plan(lib, 1, *pair, 323)[:4] == plan and plan[2] * plan[3] > 1
    assert set(fc.K14_LARGE_PLANS) == set(fc.K14_LARGE_PAIRS)
    # no plan lays (2,2) tiles side by side
    assert not any(fc.wide_plan(lib, 1, 32 * a, 32 * b, 323)[:2] == (2, 2) for a in range(1, 17) for b in range(1, 17) if (a, b) != (2, 2))
    # the second plane: 195 chunks over 97 splits (85 with six tiles): two or three chunks each, image borders inside a split
    B, P = fc.K14_PLANES[1]
    assert B * -(-P // 64) == 195 and {fc.wide_plan(lib, B, ci, co, P)[4] for ci, co in fc.K14_NEW_PAIRS} == {97}
    # K10's weight gradient is this kernel on this plan: its workspace holds the slabs
    for ci, co in fc.K14_NEW_PAIRS[:2]:
        assert lib.cabinet_pwconv_bwd_workspace_bytes(1, ci, co, 323) >= lib.cabinet_pwconv_wide_wgrad_workspace_bytes(1, ci, co, 323)


def test_bn_form_tables_reach_every_instantiation():
    lib = fc.load_library()
    reachable, big_lds = set(), set()
    for ci in range(8, 97, 8):
        for co in range(8, 97, 8):
            for P in fc.BN_PS:
                for off in (0, 4):
                    assert lib.cabinet_pw_bn_bwd_supported(ci, co, P) == 1
                    bm, bn, nsplit, vec, lds = fc.bn_plan(lib, 1, ci, co, P, off)
                    assert (bm, bn) == (-(-co // 32), -(-ci // 32))
                    assert lds == 4 * (32 * (bm + bn) * 68 + 32 * bm * (32 * bn + 4) + 32 * bm * 8)
                    assert vec == int(P % 4 == 0 and off == 0)
                    reachable.add((bm, bn))
                    if lds > 64 * 1024:  # the opt-in to more than 64 KB of dynamic LDS, one workgroup per CU
                        big_lds.add((bm, bn))
    assert reachable == set(fc.BN_SHAPES) and len(reachable) == 9
    assert big_lds == {(2, 3), (3, 2), (3, 3)}
    reached, vecs = set(), set()
    for B, ci, co, P, off in fc.bn_table_products():
        assert lib.cabinet_pw_bn_bwd_supported(ci, co, P) == 1
        bm, bn, nsplit, vec, lds = fc.bn_plan(lib, B, ci, co, P, off)
        reached.add((bm, bn))
        vecs.add((P % 4 == 0, vec))
        nchunks = B * -(-P // 64)
        assert nsplit == max(1, min(512, nchunks // 2))
        slabs = lib.cabinet_pw_bn_act_bwd_workspace_bytes(B, ci, co, P) - lib.cabinet_bn_act_workspace_bytes(B, co, P)
        assert slabs == _a256(nsplit * co * ci * 4)
    assert reached == reachable
    assert vecs == {(True, 1), (True, 0), (False, 0)}  # 16-byte stores, dwords on an aligned-size plane (dx 4 bytes off), dwords
    # the closing-BN table of the GPU file alone reaches all nine; the pairs named for <2,3> and <3,2> are what they claim
    assert {fc.bn_plan(lib, c[0], c[1], c[2], c[3])[:2] for c in fc.bn_act_cases()} == reachable
    assert [fc.bn_plan(lib, 1, ci, co, 129)[:2] for ci, co in fc.BN_PAIRS] == [(2, 3), (3, 2), (2, 3), (3, 2), (2, 3), (1, 3), (3, 1)]
    assert {fc.bn_plan(lib, c[0], c[1], c[2], c[3] * c[4])[:2] for c in fc.BN_DW_CASES} == {(3, 1), (3, 2)}
    for case, shape in zip(fc.BN_LOADED_CASES, [(2, 3), (3, 2)]):
        B, ci, co, P = case[:4]
        bm, bn, nsplit, vec, lds = fc.bn_plan(lib, B, ci, co, P)
        nchunks = B * -(-P // 64)
        assert (bm, bn) == shape and nsplit == 512 and lds > 64 * 1024 and 4 * 512 < nchunks < 5 * 512 and P % 64 == 36
    # the rotation: every activation with training on and off, both batch sizes, every plane
    rows = fc.bn_act_cases()
    assert {(r[4], r[5]) for r in rows} == {(a, t) for a in bnc.ACTS for t in (True, False)}
    assert {r[0] for r in rows} >= {1, 3} and {r[3] for r in rows} >= set(fc.BN_PS)
    assert sum(r[6] == 1 for r in rows) == 1 and sum(not r[7] for r in rows) == 1 and sum(not r[8] for r in rows) == 1
    out = (fc.ctypes.c_int * 5)()
    assert lib.cabinet_pw_bn_bwd_plan(1, 104, 56, 129, 0, out) == -2 and lib.cabinet_pwconv_wide_plan(1, 20, 16, 129, out) == -2
    assert lib.cabinet_pw_bn_bwd_plan(1, 16, 16, 0, 0, out) == -1 and lib.cabinet_pwconv_wide_plan(1, 16, 16, 129, None) == -1


def test_se_mlp_shapes_reach_the_launch_branches():
    """se_act_bwd_mlp_run has no plan beyond four ceil-divisions (SM_CT = 8 columns per contraction workgroup, SM_RT = 8 rows and
    SM_T = 256 columns per outer-product tile, SM_NB = 8 images per pass, C and Cs <= 1024): restated here on the table."""
    lib = fc.load_library()
    shapes = fc.SE_SHAPES
    for B, C, Cs in shapes:
        assert lib.cabinet_se_act_bwd_mlp_supported(C, Cs) == 1
        assert lib.cabinet_se_act_bwd_mlp_workspace_bytes(B, C, Cs) == _a256(B * Cs * 4)
    assert lib.cabinet_se_act_bwd_mlp_supported(1032, 8) == 0 and lib.cabinet_se_act_bwd_mlp_supported(8, 1032) == 0
    assert any(-(-Cs // 256) > 1 for _, _, Cs in shapes) and any(-(-C // 256) > 1 for _, C, _ in shapes)  # second column tiles, A and B
    assert any(C % 8 for _, C, _ in shapes) and any(Cs % 8 for _, _, Cs in shapes)  # short last slabs, the q < Q / cc < C guards
    assert any(Cs % 256 and Cs > 256 for _, _, Cs in shapes) and (1, 1024, 1024) in shapes and any(Cs == 1 for _, _, Cs in shapes)
    assert {B for B, _, _ in shapes} >= {1, 2, 9, 16, 17}  # one pass, a pass and one image, two full passes, two and one image
    assert set(fc.SE_POISON_SHAPES) <= set(shapes)
