"""The optimizer-tail kernels (csrc/opt_tail.hip behind cabinet_amd.optim.FusedSGDTail) on the GPU: against the reference's
run stored in tests/golden/g6_optim_tail*.npz under the rule of tests/test_optim_tail.py, bit-reproducibility, hipGraph capture
with a live schedule, the scalar and grid-stride paths, and the whole graphed train step with the tail captured."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import assert_close
from optim_tail_model import (HYPER, SNAPSHOTS, STEPS, Fixture, TailNet, buffers_of, check_scalars, check_snapshot, drive,
                              forward_side_effects, make_tail)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def everything(net, opt):
    out = {f"param.{k}": v for k, v in net.state_dict().items()}
    out.update({f"buf.{k}": v for k, v in buffers_of(opt, net).items()})
    out.update({f"ema.{k}": v for k, v in opt.ema.state_dict().items()})
    return {k: v.detach().clone() for k, v in out.items()}


def run_fixture(fx, each=None, **over):
    net = TailNet(seed=0).cuda()
    opt = make_tail(net, **over)
    drive(fx, net, opt, 1, STEPS, None if each is None else (lambda s: each(s, net, opt)))
    return net, opt


def test_kernels_match_the_reference_run(fx):
    """(a)"""
    def each(s, net, opt):
        check_scalars(fx, opt, s)
        if s in SNAPSHOTS:
            check_snapshot(fx, net, opt, s)

    net, opt = run_fixture(fx, each)
    assert opt.skipped == 1 and opt.it == STEPS - 1 and opt.ema_updates == STEPS - 1
    assert net.conv.weight.is_contiguous(memory_format=torch.channels_last)
    assert int(net.bn.num_batches_tracked) == STEPS and int(opt.ema.bn.num_batches_tracked) == 0


def test_two_runs_are_bit_identical(fx):
    """(b) no atomics, fixed summation order: the same state and gradients give the same bits, norms included."""
    norms = ([], [])
    runs = [everything(*run_fixture(fx, lambda s, net, opt, n=n: n.append(opt.last_grad_norm.clone()))) for n in norms]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert all(torch.equal(a, b) or (not torch.isfinite(a).all() and not torch.isfinite(b).all()) for a, b in zip(*norms))


def _finite_gradients(fx):
    """(STEPS, ...) stacked gradients per parameter with the inf element left out: eight real steps."""
    per_step = [fx.gradients(s) for s in range(1, STEPS + 1)]
    g = {k: torch.stack([per_step[s][k] for s in range(STEPS)]) for k in fx.names}
    g[str(fx.z["inf_name"])][fx.inf_step - 1].view(-1)[int(fx.z["inf_index"])] = 0.0
    return g


def test_eight_steps_in_one_graph_equal_eight_eager_steps(fx):
    """(c) capture does not freeze the schedule: eight steps recorded into ONE graph -- static gradients refilled between them
    inside the graph -- replay to the same bits as eight eager kernel steps, eight different learning rates included."""
    stacked = {k: v.cuda() for k, v in _finite_gradients(fx).items()}
    res = []
    for graphed in (False, True):
        net = TailNet(seed=0).cuda()
        opt = make_tail(net)
        params = dict(net.named_parameters())
        for k in fx.names:
            params[k].grad = torch.zeros_like(params[k])
        lrs, norms = torch.zeros(STEPS, 4, device="cuda"), torch.zeros(STEPS, device="cuda")

        def eight():
            for s in range(STEPS):
                forward_side_effects(net, s + 1)
                for k in fx.names:
                    params[k].grad.copy_(stacked[k][s].reshape(params[k].shape))
                opt.step()
                lrs[s].copy_(opt.lr)
                norms[s].copy_(opt.last_grad_norm[0])

        if graphed:
            opt.prepare_capture()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                eight()
            assert opt.it == 0                   # recording executed nothing
            graph.replay()
        else:
            eight()
        torch.cuda.synchronize()
        assert opt.it == STEPS and opt.ema_updates == STEPS and opt.skipped == 0
        res.append((everything(net, opt), lrs.cpu(), norms.cpu()))
    (ea, lra, na), (eb, lrb, nb) = res
    assert torch.equal(lra, lrb) and torch.equal(na, nb)
    assert len({float(x) for x in lrb[:, 0]}) == STEPS and len({float(x) for x in lrb[:, 3]}) == STEPS
    for k in ea:
        assert torch.equal(ea[k], eb[k]), k


def test_address_change_during_capture_raises(fx):
    """A gradient at a new address cannot be uploaded while the stream is capturing: step() raises instead of recording a
    stale table; after prepare_capture() outside the capture the same step records."""
    net = TailNet(seed=0).cuda()
    opt = make_tail(net)
    fx.set_grads(net, 1)
    opt.step()                                   # eager: uploads the table for these gradient tensors
    fx.set_grads(net, 2)                         # new gradient tensors
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="during stream capture"):
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            opt.step()
    opt.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        opt.step()
    assert opt.it == 1
    graph.replay()
    assert opt.it == 2


class _Bag(nn.Module):
    """Parameters handed in ready-made; two groups."""

    def __init__(self, tensors):
        super().__init__()
        self.p = nn.ParameterList([nn.Parameter(t) for t in tensors])

    def get_params(self):
        return list(self.p)[0::2], list(self.p)[1::2]


def _against_composite(tensors_of, steps=3, max_grid=0, seed=5):
    """The kernels on cuda against the composite path on the host, same parameters and gradients.  Per element both do the same
    fp32 operations in the same order; the norm (and with it the clip coefficient) is summed in another order, so the bound is
    the fixture rule's floor, 4 K 2^-24 ||x|| per tensor, on parameters, buffers and EMA."""
    g = torch.Generator().manual_seed(seed)
    host = _Bag(tensors_of("cpu", torch.Generator().manual_seed(seed + 1)))
    dev = _Bag(tensors_of("cuda", torch.Generator().manual_seed(seed + 1)))
    kw = dict(lr0=0.05, wd=5e-4, warmup_steps=1, max_iter=10, ema_tau=4)
    oh, od = make_tail(host, **kw), make_tail(dev, **kw)
    od.max_grid = max_grid
    for _ in range(steps):
        for ph, pd in zip(host.p, dev.p):
            gr = torch.randn(ph.shape, generator=g) * 0.05
            ph.grad, pd.grad = gr.clone(), gr.cuda()
        oh.step()
        od.step()
    assert od.it == oh.it == steps
    assert abs(float(od.last_grad_norm.cpu()[0]) - float(oh.last_grad_norm[0])) <= 1e-6 * float(oh.last_grad_norm[0])
    a, b = everything(host, oh), everything(dev, od)
    for k in a:
        err, floor = float((b[k].cpu().double() - a[k].double()).norm()), 4 * steps * 2.0 ** -24 * float(a[k].double().norm())
        assert err <= floor, (k, err, floor)
    return dev, od


def test_misaligned_view_and_300_tiny_tensors():
    """(d) a parameter that starts 4 bytes into its storage (its chunks take the scalar path; the EMA copy and the gradient are
    aligned) between 300 tensors of 1..7 elements: no limit on the table, one chunk per tiny tensor."""
    def tensors_of(device, g):
        out = [(torch.randn(n % 7 + 1, generator=g)).to(device) for n in range(300)]
        store = torch.zeros(2 * 4096 + 10, device=device)
        store[1:].copy_(torch.randn(2 * 4096 + 9, generator=g))
        out.insert(150, store[1:])
        return out

    dev, od = _against_composite(tensors_of)
    assert dev.p[150].data_ptr() % 16 == 4 and dev.p[150].storage_offset() == 1
    assert len(od._chunks_host) == 300 + 3


def test_grid_stride_over_chunks():
    """(e) one tensor of 3 * 4096 + 5 elements (and a second group's scalar) with the grid forced to 2 workgroups: each strides
    over several chunks; the result has the same bits as the default grid's."""
    def tensors_of(device, g):
        return [torch.randn(3 * 4096 + 5, generator=g).to(device), torch.randn(1, generator=g).to(device)]

    dev2, o2 = _against_composite(tensors_of, max_grid=2)
    dev0, o0 = _against_composite(tensors_of, max_grid=0)
    a, b = everything(dev2, o2), everything(dev0, o0)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _reference_tail(net, ema_net, sgd, state, hyper, max_norm, decay, tau):
    """train.py:411-427 with the formulas of optimizer.py:124-156 and ema.py:51-62, eagerly (test-local)."""
    import math

    norm = float(torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm))
    it, w = state["it"], hyper["warmup_steps"]
    if it < w:
        lr = hyper["warmup_start_lr"] + it / w * (hyper["lr0"] - hyper["warmup_start_lr"])
    else:
        lr = hyper["lr0"] * (1 - max((it - w) / (hyper["max_iter"] - w), 0.0)) ** hyper["power"]
    for pg in sgd.param_groups:
        pg["lr"] = lr * pg.get("lr_scale", 1.0)
    sgd.step()
    state["it"] += 1
    state["updates"] += 1
    d = decay * (1 - math.exp(-state["updates"] / tau))
    msd = net.state_dict()
    with torch.no_grad():
        for k, v in ema_net.state_dict().items():
            if v.dtype.is_floating_point:
                v.mul_(d).add_(msd[k].detach(), alpha=1 - d)
    state["norms"].append(norm)
    state["lrs"].append([pg["lr"] for pg in sgd.param_groups])


def test_graphed_train_step_with_the_tail_captured():
    """(f) GraphedTrainStep with FusedSGDTail recorded into its optimizer graph against TrainStep driving the eager
    reference-semantics tail: losses, norms, learning rates, weights, BatchNorm buffers and the EMA agree within the bounds the
    graphed-vs-eager tests of tests/test_gpu_model.py use (3e-3 on losses and norms, 2e-3 per tensor: MIOpen's backward atomics
    move the gradients run to run and SGD carries that along)."""
    import copy

    from cabinet_amd.optim import FusedSGDTail
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria, synthetic_batch

    hyper = dict(lr0=2e-2, momentum=0.9, wd=5e-4, warmup_steps=2, warmup_start_lr=1e-5, max_iter=10, power=0.9, lr_multiplier=10.0)
    batches = [synthetic_batch(2, 256, 256, 8, "cuda", seed=60 + i) for i in range(6)]
    # eager: the reference's sequence
    net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
    ema_net = copy.deepcopy(net).eval()
    wd_p, nowd_p, lr_wd_p, lr_nowd_p = net.get_params()
    groups = [dict(params=wd_p, weight_decay=hyper["wd"]), dict(params=nowd_p, weight_decay=0.0),
              dict(params=lr_wd_p, weight_decay=hyper["wd"], lr_scale=hyper["lr_multiplier"]),
              dict(params=lr_nowd_p, weight_decay=0.0, lr_scale=hyper["lr_multiplier"])]
    sgd = torch.optim.SGD(groups, lr=hyper["lr0"], momentum=hyper["momentum"], weight_decay=0.0)
    state = dict(it=0, updates=0, norms=[], lrs=[])

    class Tail:
        param_groups = sgd.param_groups

        def step(self):
            _reference_tail(net, ema_net, sgd, state, hyper, 1.0, 0.9999, 4)

    step = TrainStep(net, make_criteria(2, 256, 256, "cuda"), optimizer=Tail())
    la = [float(step(*b)) for b in batches]
    sa, ema_a = {k: v.clone() for k, v in net.state_dict().items()}, {k: v.clone() for k, v in ema_net.state_dict().items()}
    # graphed, the tail in its own hipGraph
    net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
    opt = FusedSGDTail(net, **hyper, max_grad_norm=1.0, ema_decay=0.9999, ema_tau=4)
    step = GraphedTrainStep(net, make_criteria(2, 256, 256, "cuda"), optimizer=opt, capture_optimizer=True, warmup=2)
    lb_, nb, lrb = [], [], []
    for b in batches:
        lb_.append(float(step(*b)))
        nb.append(float(opt.last_grad_norm.cpu()[0]))
        lrb.append(opt.lr.cpu().tolist())
    assert step.opt_seg.graph is not None and step.fallbacks == 0 and step.g_bwd is not None
    assert (opt.it, opt.ema_updates, opt.skipped) == (6, 6, 0)
    print("losses", la, lb_, "\nnorms", state["norms"], nb, "\nlr", state["lrs"], lrb)
    for x, y in zip(la + state["norms"], lb_ + nb):
        assert abs(x - y) <= 3e-3 * max(1.0, abs(x)), (la, lb_, state["norms"], nb)
    want = np.array(state["lrs"], dtype=np.float64).astype(np.float32)
    assert np.all(np.abs(np.array(lrb, dtype=np.float32).astype(np.float64) - want) <= np.spacing(want)), (lrb, state["lrs"])
    assert len({r[0] for r in lrb}) == 6          # six different learning rates: the captured schedule moves
    sb, ema_b = net.state_dict(), opt.ema.state_dict()
    for k in sa:
        assert_close(sb[k].double(), sa[k].double(), 2e-3, k, atol=1e-5)
        assert_close(ema_b[k].double(), ema_a[k].double(), 2e-3, "ema." + k, atol=1e-5)
