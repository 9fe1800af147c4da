"""cabinet_se_act_bwd_mlp (csrc/se_mlp.hip) on the CPU tier: its symbols are declared, exported and bound; the workspace
query and the argument checks answer before any HIP call (there is no GPU here, so no launch is made)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cabinet_se_act_bwd_mlp", "cabinet_se_act_bwd_mlp_workspace_bytes", "cabinet_se_act_bwd_mlp_supported")
# every SELayer of the two backbones
PAIRS = [(16, 8), (72, 24), (96, 24), (120, 32), (144, 40), (240, 64), (288, 72), (480, 120), (576, 144), (672, 168), (960, 240)]


@pytest.fixture(scope="module")
def lib():
    from cabinet_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _args(B=2, C=16, Cs=8, P=64, ptr=0x10000, ws=0x10000, nbytes=1 << 20):
    """Positional arguments of cabinet_se_act_bwd_mlp; the addresses are never touched by a call that is rejected."""
    return [ptr] * 7 + [B, C, Cs, P, 1] + [ptr] * 9 + [ws, nbytes, None]


def test_symbols_are_declared_exported_and_bound(lib):
    from cabinet_amd import _lib, build

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cabinet_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["cabinet_se_act_bwd_mlp"][1]) == len(_args())
    assert "se_mlp.hip" in build.SOURCES
    assert lib.cabinet_abi_version() == 8  # additive change
    assert hasattr(lib, "cabinet_se_act_bwd_coef")  # the separate tail stays


@pytest.mark.parametrize("B", [1, 2, 8, 19])
def test_workspace_query(lib, B):
    for C, Cs in PAIRS + [(8, 8), (1024, 1024)]:
        assert lib.cabinet_se_act_bwd_mlp_workspace_bytes(B, C, Cs) >= 4 * B * Cs
    for bad in [(0, 16, 8), (2, 0, 8), (2, 16, 0), (-1, 16, 8), (2, -16, 8), (2, 16, -8)]:
        assert lib.cabinet_se_act_bwd_mlp_workspace_bytes(*bad) == 0


def test_null_pointers_are_rejected_before_any_hip_call(lib):
    for i in list(range(7)) + list(range(12, 21)):  # each tensor pointer in turn
        a = _args()
        a[i] = None
        assert lib.cabinet_se_act_bwd_mlp(*a) == -1, i
        assert b"null" in lib.cabinet_last_error()


def test_non_positive_dimensions_are_rejected_before_any_hip_call(lib):
    for kw in ({"B": 0}, {"C": 0}, {"Cs": 0}, {"P": 0}, {"B": -2}, {"C": -16}, {"Cs": -8}, {"P": -1}):
        assert lib.cabinet_se_act_bwd_mlp(*_args(**kw)) == -1, kw
        assert b"non-positive" in lib.cabinet_last_error()
    # and with null pointers as well: the dimensions are looked at first, nothing is dereferenced
    assert lib.cabinet_se_act_bwd_mlp(*_args(B=0, ptr=None, ws=None, nbytes=0)) == -1


def test_size_limit_and_workspace_errors(lib):
    """C or Cs beyond what the kernels stage in LDS: CABINET_ERR_UNSUPPORTED (the caller keeps the chain of torch ops there);
    a missing or short workspace: CABINET_ERR_WORKSPACE.  Both before any launch.  cabinet_se_act_bwd_mlp_supported is the query the
    caller routes by: every SELayer of the two backbones is inside."""
    assert all(lib.cabinet_se_act_bwd_mlp_supported(C, Cs) == 1 for C, Cs in PAIRS + [(8, 8), (1024, 1024)])
    assert [lib.cabinet_se_act_bwd_mlp_supported(*p) for p in [(1025, 8), (16, 1025), (0, 8), (16, -1)]] == [0, 0, 0, 0]
    assert lib.cabinet_se_act_bwd_mlp(*_args(C=1025, Cs=8)) == -2 and b"se_act_bwd_mlp" in lib.cabinet_last_error()
    assert lib.cabinet_se_act_bwd_mlp(*_args(C=16, Cs=1025)) == -2
    need = lib.cabinet_se_act_bwd_mlp_workspace_bytes(2, 16, 8)
    assert lib.cabinet_se_act_bwd_mlp(*_args(nbytes=need - 1)) == -3
    assert lib.cabinet_se_act_bwd_mlp(*_args(ws=None)) == -3


def test_flag_follows_the_environment():
    import cabinet_amd.functional as Fh

    assert Fh.SE_MLP_FUSED is (os.environ.get("CABINET_SE_MLP_FUSED", "1") != "0")
