"""FusedSGDTail on the CPU tier: the composite path (same semantics as the kernels of csrc/opt_tail.hip) against the reference's
own clip_grad_norm_ + Optimizer + ModelEMA run stored in tests/golden/g6_optim_tail*.npz, the host logic around it (resume,
checkpoint interchange, skipped steps, EMA-only entries), and the ABI surface.

Rule for fixture comparisons (optim_tail_model.fixture_rule): per tensor, on the change since the initial state,
||d - d64|| <= max(parity_rules.ALLOW_FACTOR x the fp32 reference's own ||d32 - d64||, 4 K 2^-24 ||x64||).
Norms: within 1e-6 relative of the fp64 norm.  Learning rates: equal to the fixture's float32 value during warm-up, within one
float ulp in the poly phase (two pow implementations may differ in the last bit of a double)."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from optim_tail_model import (HYPER, SNAPSHOTS, STEPS, Fixture, TailNet, buffers_of, check_scalars, check_snapshot, drive,
                              make_tail)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_composite_path_matches_the_reference_run(fx):
    net = TailNet(seed=0)
    opt = make_tail(net)
    assert opt.capturable is True and not opt.ema.training and not any(p.requires_grad for p in opt.ema.parameters())

    def each(s):
        check_scalars(fx, opt, s)
        if s in SNAPSHOTS:
            check_snapshot(fx, net, opt, s)

    drive(fx, net, opt, 1, STEPS, each)
    assert opt.skipped == 1 and opt.it == STEPS - 1


def test_skipped_step_changes_nothing_and_counts(fx):
    net = TailNet(seed=0)
    opt = make_tail(net)
    drive(fx, net, opt, 1, fx.inf_step - 1)
    before = ({k: v.clone() for k, v in net.state_dict().items()}, {k: v.clone() for k, v in buffers_of(opt, net).items()},
              {k: v.clone() for k, v in opt.ema.state_dict().items()}, opt.it, opt.ema_updates, opt.lr.clone())
    fx.set_grads(net, fx.inf_step)
    opt.step()
    after = (net.state_dict(), buffers_of(opt, net), opt.ema.state_dict())
    for a, b in zip(before[:3], after):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert (opt.it, opt.ema_updates, opt.skipped) == (before[3], before[4], 1) and torch.equal(opt.lr, before[5])
    # skip_nonfinite=False steps as torch would: the inf reaches the weights
    net2 = TailNet(seed=0)
    opt2 = make_tail(net2, skip_nonfinite=False)
    fx.set_grads(net2, fx.inf_step)
    opt2.step()
    assert opt2.skipped == 0 and opt2.it == 1 and not all(torch.isfinite(p).all() for p in net2.parameters())


def test_resume_from_step_5_equals_the_straight_run(fx):
    net = TailNet(seed=0)
    opt = make_tail(net)
    drive(fx, net, opt, 1, 5)
    ckpt = dict(model=net.state_dict(), optimizer_state=opt.state_dict(), ema_state=opt.ema.state_dict(), it=opt.it,
                updates=opt.ema_updates)
    ckpt = {k: (v if isinstance(v, int) else copy.deepcopy(v)) for k, v in ckpt.items()}
    drive(fx, net, opt, 6, STEPS)
    net2 = TailNet(seed=3)                      # other weights: everything must come from the checkpoint
    net2.load_state_dict(ckpt["model"])
    opt2 = make_tail(net2)
    opt2.load_state_dict(ckpt["optimizer_state"])
    opt2.ema.load_state_dict(ckpt["ema_state"])
    opt2.it, opt2.ema_updates = ckpt["it"], ckpt["updates"]
    drive(fx, net2, opt2, 6, STEPS)
    for a, b in ((net.state_dict(), net2.state_dict()), (buffers_of(opt, net), buffers_of(opt2, net2)),
                 (opt.ema.state_dict(), opt2.ema.state_dict())):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert (opt2.it, opt2.ema_updates) == (opt.it, opt.ema_updates) and torch.equal(opt.lr, opt2.lr)


def test_checkpoint_interchange_with_the_reference_layout(fx):
    """The reference's ``optimizer_state`` is ``torch.optim.SGD.state_dict()`` over its four groups: the fixture's step-5 state in
    that layout loads here, steps 6-8 land on the fixture's step-8 state under the rule, and a plain SGD over the same groups
    loads what this class writes."""
    z = fx.z
    net = TailNet(seed=3)
    sd = {k: torch.from_numpy(z[f"s5.f32.param.{k}"]) for k in (str(n) for n in z["names"])}
    sd["bn.num_batches_tracked"] = torch.tensor(5)
    net.load_state_dict(sd)
    opt = make_tail(net)
    name_of = {id(p): k for k, p in net.named_parameters()}
    ref = torch.optim.SGD([dict(g, params=list(g["params"])) for g in opt.param_groups], lr=HYPER["lr0"], momentum=HYPER["momentum"])
    for g in ref.param_groups:
        for p in g["params"]:
            if p.requires_grad:
                ref.state[p]["momentum_buffer"] = torch.from_numpy(z[f"s5.f32.buf.{name_of[id(p)]}"]).reshape(p.shape).clone()
    opt.load_state_dict(ref.state_dict())        # the frozen parameter has no state there: it gets a zero, not-yet-valid buffer
    esd = {k: torch.from_numpy(z[f"s5.f32.ema.{k}"]) for k in (str(n) for n in z["names"])}
    esd["bn.num_batches_tracked"] = torch.tensor(0)
    opt.ema.load_state_dict(esd)
    opt.it, opt.ema_updates = int(z["s5.it"]), int(z["s5.updates"])
    drive(fx, net, opt, 6, STEPS, lambda s: check_scalars(fx, opt, s))
    check_snapshot(fx, net, opt, STEPS)
    ref.load_state_dict(opt.state_dict())
    for p in ref.param_groups[0]["params"]:
        assert torch.equal(ref.state[p]["momentum_buffer"], opt.optim.state[p]["momentum_buffer"])


def test_frozen_parameter_and_int_buffers(fx):
    net = TailNet(seed=0)
    frozen0 = net.frozen.detach().clone()
    opt = make_tail(net)
    drive(fx, net, opt, 1, STEPS)
    assert torch.equal(net.frozen, frozen0) and net.frozen.grad is None       # the optimizer never touches it
    assert "momentum_buffer" in opt.optim.state[net.frozen] and not opt.optim.state[net.frozen]["momentum_buffer"].any()
    # its average folds the same value every step: d*e + (1-d)*p is two products and a sum, <= 2 ulp per step
    assert float((opt.ema.frozen - frozen0).abs().max()) <= 2 * (STEPS - 1) * 2.0 ** -24 * float(frozen0.abs().max())
    # integer buffers: the live counter counts, the averaged module's stays as copied (ema.py:61-65)
    assert int(net.bn.num_batches_tracked) == STEPS and int(opt.ema.bn.num_batches_tracked) == 0


def test_gradless_parameter_is_skipped_and_strides_are_checked(fx):
    net = TailNet(seed=0)
    opt = make_tail(net)
    fx.set_grads(net, 1)
    net.vecs[5].grad = None
    v5 = net.vecs[5].detach().clone()
    opt.step()
    assert torch.equal(net.vecs[5], v5) and not opt.optim.state[net.vecs[5]]["momentum_buffer"].any()
    fx.set_grads(net, 2)
    net.conv.weight.grad = net.conv.weight.grad.contiguous()                # NCHW gradient for a channels_last weight
    with pytest.raises(RuntimeError, match="dense fp32 with equal strides"):
        opt.step()


def test_optimizer_segment_accepts_a_capturable_object():
    from cabinet_amd.train import _OptimizerSegment

    opt = make_tail(TailNet(seed=0))
    seg = _OptimizerSegment(opt, capture=True)
    assert seg.capture and seg.graph is None

    class Wrapper:
        param_groups = opt.param_groups

        def step(self):
            pass

    with pytest.raises(RuntimeError, match="wrapper"):
        _OptimizerSegment(Wrapper(), capture=True)
    with pytest.raises(RuntimeError, match="before_optimizer"):
        _OptimizerSegment(opt, capture=True, before=lambda: None)


def test_header_and_signatures_list_the_new_symbols_at_abi_8():
    from cabinet_amd import _lib, build

    text = open(os.path.join(ROOT, "include", "cabinet_hip.h")).read()
    assert re.search(r"#define CABINET_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    for s in ("cabinet_sgd_tail_workspace_bytes", "cabinet_sgd_tail_state_bytes", "cabinet_sgd_tail_step"):
        assert re.search(rf"\b{s}\s*\(", text) and s in _lib.SIGNATURES
    assert "opt_tail.hip" in build.SOURCES
    build.build(verbose=False)
    assert _lib.load().cabinet_abi_version() == 8


def test_argument_errors_are_codes_not_faults():
    """Refused before any HIP call: the addresses below are never touched."""
    from cabinet_amd import _lib, build
    from cabinet_amd.optim import _CHUNK, _ENTRY, _Config, build_chunks

    build.build(verbose=False)
    lib = _lib.load()
    assert _ENTRY.itemsize == 48 and _CHUNK.itemsize == 16
    assert lib.cabinet_sgd_tail_workspace_bytes(0) == 0 and lib.cabinet_sgd_tail_workspace_bytes(2600) >= 2600 * 4
    assert lib.cabinet_sgd_tail_state_bytes(343) >= 128 + 2 * 4 * 343 and lib.cabinet_sgd_tail_state_bytes(-1) == 0
    cfg = _Config(lr0=0.05, max_iter=10.0, power=0.9, ema_decay=0.9999, ema_tau=2000.0, warmup_steps=3)
    c, A = ctypes.addressof(cfg), 0x10000
    big = 1 << 20
    step = lib.cabinet_sgd_tail_step
    assert step(None, 4, A, 4, c, A, big, 0, A, big, None) == -1 and b"null table" in lib.cabinet_last_error()
    assert step(A, 4, None, 4, c, A, big, 0, A, big, None) == -1 and b"null table" in lib.cabinet_last_error()
    assert step(A, 0, A, 4, c, A, big, 0, A, big, None) == -1 and b"non-positive" in lib.cabinet_last_error()
    assert step(A, 4, A, -2, c, A, big, 0, A, big, None) == -1 and b"non-positive" in lib.cabinet_last_error()
    assert step(A, 4, A, 4, None, A, big, 0, A, big, None) == -1
    assert step(A, 4, A, 4, c, A, big, 0, A, 8, None) == -3 and b"workspace" in lib.cabinet_last_error()
    assert step(A, 4, A, 4, c, A, big, 0, None, 0, None) == -3
    assert step(A, 4, A, 4, c, A, 64, 0, A, big, None) == -3 and b"state block" in lib.cabinet_last_error()
    bad = _Config(lr0=0.05, max_iter=3.0, power=0.9, ema_decay=0.9999, ema_tau=2000.0, warmup_steps=3)
    assert step(A, 4, A, 4, ctypes.addressof(bad), A, big, 0, A, big, None) == -1 and b"max_iter" in lib.cabinet_last_error()
    # the chunk list: every tensor cut at multiples of 4096, a small tensor one chunk
    ch = build_chunks([1, 4096, 4097, 3 * 4096 + 5])
    assert [(int(r["tensor"]), int(r["start"]), int(r["length"])) for r in ch] == \
        [(0, 0, 1), (1, 0, 4096), (2, 0, 4096), (2, 4096, 1), (3, 0, 4096), (3, 4096, 4096), (3, 8192, 4096), (3, 12288, 5)]
