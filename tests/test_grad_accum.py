"""GradAccumulator on the CPU tier: the composite path (same semantics as csrc/grad_accum.hip) against a Python loop, bit for bit,
the counter, the validation of the pairs, and the ABI surface of cabinet_grad_accum / cabinet_grad_accum_reset."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from cabinet_amd.optim import GradAccumulator


def _bits(t):
    return t.contiguous().view(torch.int32)


def _special(shape, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    flat = t.view(-1)
    vals = [float("inf"), -float("inf"), -0.0, 0.0, 1e-40, -1e-40]
    for i in range(min(flat.numel(), len(vals))):
        flat[(i * 7 + seed) % flat.numel()] = vals[(i + seed) % len(vals)]
    return t


def test_composite_path_is_bit_equal_to_a_python_loop():
    shapes = [(1,), (3,), (5, 7), (4097,), (6, 4, 3, 3)]
    grads = [torch.empty(s) for s in shapes]
    accs = [torch.full(s, float("nan")) for s in shapes]
    acc = GradAccumulator(list(zip(accs, grads)))
    steps = [[_special(s, 10 * k + i) for i, s in enumerate(shapes)] for k in range(4)]
    steps[0][1][0] = -0.0  # a copied -0.0 stays -0.0
    want = None
    for k in range(3):
        for g, new in zip(grads, steps[k]):
            g.copy_(new)
        acc.add()
        want = [s.clone() for s in steps[0]] if k == 0 else [w + s for w, s in zip(want, steps[k])]
        assert acc.micro == k + 1
        for a, w in zip(accs, want):
            assert torch.equal(_bits(a), _bits(w))
        if k == 0:
            assert _bits(accs[1])[0].item() == -2 ** 31 and not any(torch.isnan(a).all() for a in accs)  # -0.0 copied, no stale NaN
    acc.reset()
    assert acc.micro == 0
    for g, new in zip(grads, steps[3]):
        g.copy_(new)
    acc.add()
    for a, w in zip(accs, steps[3]):
        assert torch.equal(_bits(a), _bits(w))
    assert acc.micro == 1


def test_micro_counts_and_can_be_set():
    a, g = torch.zeros(5), torch.ones(5)
    acc = GradAccumulator([(a, g)])
    assert acc.micro == 0 and acc.max_grid == 0
    acc.add()
    acc.add()
    assert acc.micro == 2 and torch.equal(a, torch.full((5,), 2.0))
    acc.micro = 0  # the next add() copies
    a.fill_(float("nan"))
    acc.add()
    assert acc.micro == 1 and torch.equal(a, torch.ones(5))
    acc.micro = 7  # any other value adds
    acc.add()
    assert acc.micro == 8 and torch.equal(a, torch.full((5,), 2.0))


def test_open_accumulator_binds_once():
    a, g = torch.zeros(4), torch.ones(4)
    acc = GradAccumulator([(a, None)])
    with pytest.raises(RuntimeError, match="no gradients bound"):
        acc.add()
    acc.bind([g])
    acc.add()
    assert torch.equal(a, g)
    with pytest.raises(RuntimeError, match="already bound"):
        acc.bind([g])
    with pytest.raises(ValueError, match="every pair"):
        GradAccumulator([(a, g), (torch.zeros(2), None)])


def test_mismatched_pairs_raise():
    a = torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="dense fp32 with equal strides"):  # dtype
        GradAccumulator([(a, torch.zeros(4, 6, dtype=torch.float64))])
    with pytest.raises(RuntimeError, match="dense fp32 with equal strides"):  # dtype of acc
        GradAccumulator([(a.double(), torch.zeros(4, 6))])
    with pytest.raises(RuntimeError, match="dense fp32 with equal strides"):  # shape
        GradAccumulator([(a, torch.zeros(6, 4))])
    w = torch.zeros(2, 3, 4, 5)
    with pytest.raises(RuntimeError, match="dense fp32 with equal strides"):  # strides
        GradAccumulator([(w, torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))])
    with pytest.raises(RuntimeError, match="dense fp32 with equal strides"):  # not dense
        GradAccumulator([(torch.zeros(4, 12)[:, ::2], torch.zeros(4, 12)[:, ::2])])
    with pytest.raises(RuntimeError, match="same memory"):
        GradAccumulator([(a, a)])
    with pytest.raises(ValueError):
        GradAccumulator([])
    # equal strides of a permuted layout are fine
    cl = torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    GradAccumulator([(cl, torch.ones_like(cl))]).add()
    assert torch.equal(cl, torch.ones_like(cl))


def test_header_and_signatures_list_the_new_symbols_at_abi_8():
    from cabinet_amd import _lib, build

    text = open(os.path.join(ROOT, "include", "cabinet_hip.h")).read()
    assert re.search(r"#define CABINET_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    for s in ("cabinet_grad_accum_state_bytes", "cabinet_grad_accum", "cabinet_grad_accum_reset"):
        assert re.search(rf"\b{s}\s*\(", text) and s in _lib.SIGNATURES
    assert re.search(r"\}\s*cabinet_grad_accum_entry;", text)
    assert "grad_accum.hip" in build.SOURCES
    build.build(verbose=False)
    assert _lib.load().cabinet_abi_version() == 8


def test_argument_errors_are_codes_not_faults():
    """Refused before any HIP call: the addresses below are never touched."""
    from cabinet_amd import _lib, build
    from cabinet_amd.optim import _ACCUM_ENTRY, _ACCUM_STATE_BYTES

    build.build(verbose=False)
    lib = _lib.load()
    assert _ACCUM_ENTRY.itemsize == 24
    need = lib.cabinet_grad_accum_state_bytes()
    assert need == _ACCUM_STATE_BYTES and need >= 4
    A, add, reset = 0x10000, lib.cabinet_grad_accum, lib.cabinet_grad_accum_reset
    assert add(None, 4, A, 4, A, need, 0, None) == -1 and b"null table" in lib.cabinet_last_error()
    assert add(A, 4, None, 4, A, need, 0, None) == -1 and b"null table" in lib.cabinet_last_error()
    assert add(A, 4, A, 4, None, need, 0, None) == -1 and b"null state" in lib.cabinet_last_error()
    assert add(A, -1, A, 4, A, need, 0, None) == -1 and b"non-positive" in lib.cabinet_last_error()
    assert add(A, 4, A, -2, A, need, 0, None) == -1 and b"non-positive" in lib.cabinet_last_error()
    assert add(A, 4, A, 0, A, need, 0, None) == -1 and b"non-positive" in lib.cabinet_last_error()
    assert add(A, 4, A, 4, A, need, -3, None) == -1 and b"max_grid" in lib.cabinet_last_error()
    assert add(A + 4, 4, A, 4, A, need, 0, None) == -1 and b"8-byte aligned" in lib.cabinet_last_error()
    assert add(A, 4, A, 4, A, need - 1, 0, None) == -3 and b"state block" in lib.cabinet_last_error()
    assert add(A, 4, A, 4, A, 0, 0, None) == -3
    assert reset(None, need, None) == -1 and b"null state" in lib.cabinet_last_error()
    assert reset(A, 3, None) == -3 and b"state block" in lib.cabinet_last_error()
    with pytest.raises(RuntimeError, match="code -3"):
        _lib.check(reset(A, 0, None), "cabinet_grad_accum_reset")
    assert ctypes.sizeof(ctypes.c_void_p) == 8
