"""Gradient accumulation in the graphed train step (K21, csrc/grad_accum.hip, ``GradAccumulator``,
``GraphedTrainStep(accum_steps=k)``).

(a)-(c) the kernel against torch on the device, bit for bit: a copy on a window's first micro-step (NaN-prefilled ``acc``), one
fp32 add afterwards, over edge sizes, a misaligned view, a channels_last weight and 300 tiny tensors, every tensor seated between
guard elements that must come back unchanged; the grid-stride loop; one recorded ``add()`` replayed over a window.
(d) inside the step, independent of any stock kernel's run-to-run noise: ``p.grad`` is the in-order torch sum of the clones of the
static per-micro-step gradients of the current window, OHEM (graph B) and focal (one graph).
(e) against ``TrainStep(accum_steps=3)`` driving its own ``FusedSGDTail`` eagerly, with the graphed-vs-eager bounds of
tests/test_gpu_optim_tail.py (3e-3 on losses and norms; ``assert_close(..., 2e-3, atol=1e-5)`` per tensor).  Those bounds were
derived for single-batch steps, so the eager side runs twice: where its own run-to-run distance exceeds a third of a bound, that
bound becomes three times the measured distance (printed, never silent).
(f) branches inside windows (tests/test_gpu_ohem_topk.py section 6): first-branch, other-branch and all-ignored batches, with and
without ``device_select``.
(g) ``accum_steps=1`` is the object it was."""
import numpy as np
import pytest
import torch

from conftest import assert_close
from test_gpu_ohem_topk import IGNORE, LN8, _compare, _own_argmax_labels

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Seats:
    """Tensors seated inside larger allocations: ``views`` and, per allocation, the mask of its guard elements."""

    def __init__(self, grad_side):
        self.views, self.stores = [], []
        for n in SIZES:
            # both tensors of a pair 16-byte aligned, except 4097: its gradient starts 12 bytes into the allocation
            off = 3 if (grad_side and n == 4097) else 4
            self._seat(n + 8, off, (n,))
        self._seat(2 * 4096 + 10, 1, (2 * 4096 + 9,))                     # a view starting 4 bytes into its storage
        shape = (16, 24, 3, 3)                                             # a channels_last 4-D weight
        store, mask = self._store(16 * 24 * 9 + 8)
        v = store[4:4 + 16 * 24 * 9].view(16, 3, 3, 24).permute(0, 3, 1, 2)
        assert v.shape == shape and v.is_contiguous(memory_format=torch.channels_last)
        mask[4:4 + 16 * 24 * 9] = False
        self.views.append(v)
        store, mask = self._store(300 * 12 + 16)                           # 300 one- to seven-element tensors, any alignment
        for i in range(300):
            n, lo = i % 7 + 1, 12 * i + 3
            mask[lo:lo + n] = False
            self.views.append(store[lo:lo + n])
        assert self.views[len(SIZES)].data_ptr() % 16 == 4

    def _store(self, numel):
        store = torch.full((numel,), SENTINEL, device="cuda")
        mask = torch.ones(numel, dtype=torch.bool, device="cuda")
        self.stores.append((store, mask))
        return store, mask

    def _seat(self, numel, off, shape):
        store, mask = self._store(numel)
        n = int(np.prod(shape))
        mask[off:off + n] = False
        self.views.append(store[off:off + n].view(shape))

    def guards_intact(self):
        return all(bool((s[m] == SENTINEL).all()) for s, m in self.stores)


def _values(views, seed):
    """Random values with -0.0, +-inf and denormals sprinkled in, one tensor per view (contiguous, on the device)."""
    g = torch.Generator().manual_seed(seed)
    special = [-0.0, float("inf"), -float("inf"), 1e-40, -3e-42, 0.0]
    out = []
    for i, v in enumerate(views):
        t = torch.randn(v.numel(), generator=g)
        for j in range(0, v.numel(), 5 if v.numel() < 64 else 97):
            t[(j + seed + i) % v.numel()] = special[(i + j + seed) % len(special)]
        out.append(t.view(v.shape).cuda())
    return out


def _write(views, vals):
    for v, x in zip(views, vals):
        v.copy_(x)


def _accumulator(max_grid=0):
    from cabinet_amd.optim import GradAccumulator

    acc, grad = Seats(False), Seats(True)
    for a in acc.views:
        a.fill_(float("nan"))
    ga = GradAccumulator(list(zip(acc.views, grad.views)))
    ga.max_grid = max_grid
    return ga, acc, grad


@pytest.fixture(scope="module")
def gs():
    views = Seats(False).views
    return [_values(views, 100 + k) for k in range(4)]


def _run_window(ga, acc, grad, gs):
    for g in gs[:3]:
        _write(grad.views, g)
        ga.add()
    three = [a.clone() for a in acc.views]
    assert ga.micro == 3
    ga.reset()
    assert ga.micro == 0
    _write(grad.views, gs[3])
    ga.add()
    assert ga.micro == 1
    return three, [a.clone() for a in acc.views]


def test_kernel_against_torch_bitwise(gs):
    """(a)"""
    ga, acc, grad = _accumulator()
    assert len(ga._chunks_host) == 6 + 2 + 3 + 3 + 1 + 300
    three, one = _run_window(ga, acc, grad, gs)
    torch.cuda.synchronize()
    for i, (t, o) in enumerate(zip(three, one)):
        want = (gs[0][i] + gs[1][i]) + gs[2][i]
        assert torch.equal(_bits(t), _bits(want)), (i, tuple(t.shape))
        assert torch.equal(_bits(o), _bits(gs[3][i])), (i, tuple(o.shape))
        assert not bool(torch.isnan(o).any())  # no stale NaN of the prefilled acc survived the copy
    for v, x in zip(grad.views, gs[3]):  # the gradients are read only
        assert torch.equal(_bits(v), _bits(x))
    assert acc.guards_intact() and grad.guards_intact()


def test_grid_stride_loop_gives_the_same_bits(gs):
    """(b)"""
    a3, b3 = _accumulator(max_grid=3), _accumulator()
    ra, rb = _run_window(*a3, gs), _run_window(*b3, gs)
    for x, y in zip(ra[0] + ra[1], rb[0] + rb[1]):
        assert torch.equal(_bits(x), _bits(y))
    assert a3[1].guards_intact() and a3[2].guards_intact()


def test_one_recorded_add_serves_a_window(gs):
    """(c)"""
    eager = _accumulator()
    want3, want1 = _run_window(*eager, gs)  # also the kernels' first launch, outside capture
    ga, acc, grad = _accumulator()
    torch.cuda.synchronize()
    g_add, g_reset = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_add):
        ga.add()
    with torch.cuda.graph(g_reset, pool=g_add.pool()):
        ga.reset()
    assert ga.micro == 0 and ga._entries_captured  # recording executes nothing
    for g in gs[:3]:
        _write(grad.views, g)
        g_add.replay()
    assert ga.micro == 3
    for a, w in zip(acc.views, want3):
        assert torch.equal(_bits(a), _bits(w))
    g_reset.replay()
    assert ga.micro == 0
    _write(grad.views, gs[3])
    g_add.replay()
    for a, w in zip(acc.views, want1):
        assert torch.equal(_bits(a), _bits(w))
    assert ga.micro == 1 and acc.guards_intact() and grad.guards_intact()


# ---- inside the step ----------------------------------------------------------------------------------------------------------

def _batches(n=10):
    from cabinet_amd.train import synthetic_batch

    return [synthetic_batch(2, 256, 256, 8, "cuda", seed=60 + i) for i in range(n)]


@pytest.mark.parametrize("loss,k", [("ohem", 3), ("focal", 2)])
def test_grad_is_the_in_order_sum_of_the_window(loss, k):
    """(d)"""
    from cabinet_amd.train import GraphedTrainStep, build_model, make_criteria

    net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
    step = GraphedTrainStep(net, make_criteria(2, 256, 256, "cuda", loss=loss), warmup=2, accum_steps=k)
    window, graphed = [], 0
    for im, lb in _batches():
        replayed = step.g_fwd is not None  # the call that records the graphs still runs eagerly
        step(im, lb)
        if not replayed:
            continue
        graphed += 1
        clones = [g.clone() for _, g in step.s_grads]
        if len(window) == k:
            window = []  # the window closed with the call before: this call's gradients alone
        window.append(clones)
        want = window[0]
        for more in window[1:]:
            want = [w + m for w, m in zip(want, more)]
        for (p, _), w in zip(step.s_grads, want):
            assert p.grad is not None and torch.equal(_bits(p.grad), _bits(w)), len(window)
        assert step.accum.micro == len(window) % k
    step.flush()
    assert step.accum.micro == 0 and step._micro == 0
    first_graphed = {3: 4, 2: 3}[k]  # capture behind the first call >= warmup that closes a window
    assert graphed == 10 - first_graphed + 1 and step.fallbacks == 0
    if loss == "focal":
        assert step.g_bwd is None and step.g_any is None
    else:
        assert step.g_bwd is not None


HYPER = dict(lr0=2e-2, momentum=0.9, wd=5e-4, warmup_steps=2, warmup_start_lr=1e-5, max_iter=10, power=0.9, lr_multiplier=10.0)


def _run_e(graphed, batches):
    from cabinet_amd.optim import FusedSGDTail
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria

    net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
    opt = FusedSGDTail(net, **HYPER, max_grad_norm=1.0, ema_decay=0.9999, ema_tau=4)
    crit = make_criteria(2, 256, 256, "cuda")
    if graphed:
        step = GraphedTrainStep(net, crit, optimizer=opt, capture_optimizer=True, warmup=2, accum_steps=3)
    else:
        step = TrainStep(net, crit, optimizer=opt, accum_steps=3)
    losses, norms = [], []
    for b in batches:
        losses.append(float(step(*b)))
        norms.append(float(opt.last_grad_norm.cpu()[0]))
    step.flush()
    norms.append(float(opt.last_grad_norm.cpu()[0]))
    assert (opt.it, opt.ema_updates, opt.skipped) == (4, 4, 0)
    if graphed:
        assert step.opt_seg.graph is not None and step.fallbacks == 0 and step.accum.micro == 0
    state = {k: v.clone() for k, v in net.state_dict().items()}
    state.update({"ema." + k: v.clone() for k, v in opt.ema.state_dict().items()})
    return losses + norms, state


def test_windows_of_three_against_the_eager_step():
    """(e) Bounds of tests/test_gpu_optim_tail.py: 3e-3 on losses and norms, 2e-3 (atol 1e-5) per tensor; the eager side's own
    run-to-run distance is measured in the same session and a bound it exceeds a third of becomes three times that distance.
    Measured on one MI355X (also in DESIGN.md, K21): eager-vs-eager distance exactly 0 on all 21 losses and norms and on
    every tensor; graphed-vs-eager the same, exactly 0 -- at these shapes the runs are bit-reproducible and the
    accumulate kernel adds what autograd adds -- so no bound was replaced (third of a bound: 1e-3 and 6.7e-4 x ||tensor||)."""
    batches = _batches()
    sa, ta = _run_e(False, batches)
    sb, tb = _run_e(False, batches)
    sg, tg = _run_e(True, batches)
    widened, worst_ee, worst_ge = [], 0.0, 0.0
    for i, (a, b, g) in enumerate(zip(sa, sb, sg)):
        bound, ee = 3e-3 * max(1.0, abs(a)), abs(a - b)
        if ee > bound / 3:
            widened.append(("scalar", i, ee, bound))
            bound = 3 * ee
        worst_ee, worst_ge = max(worst_ee, ee / max(1.0, abs(a))), max(worst_ge, abs(g - a) / max(1.0, abs(a)))
        assert abs(g - a) <= bound, (i, a, b, g)
    print(f"scalars: eager-vs-eager {worst_ee:.3e}, graphed-vs-eager {worst_ge:.3e} (bound 3e-3)")
    worst_ee = worst_ge = 0.0
    for k in ta:
        if not ta[k].dtype.is_floating_point:
            assert torch.equal(ta[k], tg[k]), k
            continue
        a, b, g = ta[k].double(), tb[k].double(), tg[k].double()
        bound = 2e-3 * float(a.norm()) + 1e-5 * a.numel() ** 0.5
        ee, ge = float((b - a).norm()), float((g - a).norm())
        worst_ee, worst_ge = max(worst_ee, ee / bound), max(worst_ge, ge / bound)
        if ee > bound / 3:
            widened.append((k, ee, bound))
            assert ge <= 3 * ee, (k, ge, ee, bound)
        else:
            assert_close(g, a, 2e-3, k, atol=1e-5)
    print(f"tensors, as a share of the bound: eager-vs-eager {worst_ee:.3e}, graphed-vs-eager {worst_ge:.3e}")
    print("bounds replaced by 3 x eager-vs-eager:", widened)


KINDS = ["F", "F", "F", "O", "I", "F", "O", "F", "F"]   # F F | F O | I F | O F | F, then flush()


def _build_f(device_select, graphed):
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria

    net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-2, momentum=0.9)
    crit = make_criteria(2, 256, 256, "cuda", thresh=LN8, device_select=device_select)
    if graphed:
        return net, GraphedTrainStep(net, crit, optimizer=opt, warmup=1, device_select=device_select, accum_steps=2)
    return net, TrainStep(net, crit, optimizer=opt, accum_steps=2)


@pytest.fixture(scope="module")
def branch_batches():
    """The eager reference run (criteria with ``device_select=True``, as section 6 of tests/test_gpu_ohem_topk.py) makes the
    batches: the labels of an 'O' batch are the net's own argmax in its state at that call."""
    from cabinet_amd.train import synthetic_batch

    net, step = _build_f(True, False)
    batches, losses = [], []
    for i, kind in enumerate(KINDS):
        im, lb = synthetic_batch(2, 256, 256, 8, "cuda", seed=60 + i)
        if kind == "O":
            lb = _own_argmax_labels(net, im)
        elif kind == "I":
            lb = torch.full_like(lb, IGNORE)
        batches.append((im, lb))
        losses.append(float(step(im, lb)))
    step.flush()
    return batches, losses, {k: v.clone() for k, v in net.state_dict().items()}


def _run_f(device_select, graphed, batches):
    net, step = _build_f(device_select, graphed)
    losses = [float(step(*b)) for b in batches]
    step.flush()
    return step, losses, {k: v.clone() for k, v in net.state_dict().items()}


def test_branches_inside_windows_with_device_select(branch_batches):
    """(f) the two graphed 'O' batches replay graph B-any, the all-ignored batch falls back (loss 0.0, a contribution of zeros)."""
    batches, ref_losses, ref_state = branch_batches
    step, losses, state = _run_f(True, True, batches)
    print("eager  ", ref_losses, "\ngraphed", losses)
    assert step.g_any is not None and step.device_selected == 2 and step.fallbacks == 1
    assert losses[4] == 0.0 and ref_losses[4] == 0.0
    _compare(ref_losses, losses, ref_state, state)


def test_branches_inside_windows_without_device_select(branch_batches):
    """(f) without the option the two 'O' batches and the 'I' batch fall back inside their windows.  Compared against
    ``TrainStep(accum_steps=2)`` with the same criteria (``device_select=False``) over the same batches: as section 6 explains,
    one set of criteria run two ways is what that section's tolerances price."""
    batches, _, _ = branch_batches
    _, ref_losses, ref_state = _run_f(False, False, batches)
    step, losses, state = _run_f(False, True, batches)
    print("eager  ", ref_losses, "\ngraphed", losses)
    assert step.g_any is None and step.device_selected == 0 and step.fallbacks == 3
    assert losses[4] == 0.0 and ref_losses[4] == 0.0
    _compare(ref_losses, losses, ref_state, state)


def test_default_is_unchanged():
    """(g)"""
    from cabinet_amd.train import GraphedTrainStep, build_model, make_criteria

    net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-2, momentum=0.9)
    step = GraphedTrainStep(net, make_criteria(2, 256, 256, "cuda"), optimizer=opt)
    assert step.accum_steps == 1 and step.accum is None and step.opt_seg.after is None
    step.flush()  # before capture: nothing to flush
    for b in _batches(4):
        step(*b)
    assert step.g_bwd is not None and step.accum is None and step.fallbacks == 0
    before = {k: v.clone() for k, v in net.state_dict().items()}
    step.flush()
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert all(p.grad is g for p, g in step.s_grads)
