"""The synthetic module and the fixture access shared by tests/golden/make_golden_optim_tail.py, tests/test_optim_tail.py and
tests/test_gpu_optim_tail.py (data layout of tests/golden/g6_optim_tail*.npz: see the generator's docstring)."""
import os

import numpy as np
import torch
import torch.nn as nn

from parity_rules import ALLOW_FACTOR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
HYPER = dict(lr0=0.05, momentum=0.9, wd=5e-4, warmup_steps=3, warmup_start_lr=1e-5, max_iter=8, power=0.9, lr_multiplier=10.0)
MAX_NORM, EMA_DECAY, EMA_TAU = 1.0, 0.9999, 4
STEPS, SNAPSHOTS = 8, (5, 8)


class TailNet(nn.Module):
    """Fourteen vectors of the edge sizes, a channels_last convolution weight, a BatchNorm (float buffers and an int counter)
    and one frozen parameter; ``get_params`` deals them over the reference's four groups (the frozen one included, as the real
    model's frozen parameters are)."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.vecs = nn.ParameterList([nn.Parameter(torch.randn(n, generator=g)) for n in SIZES])
        self.conv = nn.Conv2d(6, 10, 3, bias=False)
        self.conv.weight.data = torch.randn(10, 6, 3, 3, generator=g).contiguous(memory_format=torch.channels_last)
        self.bn = nn.BatchNorm2d(10)
        self.bn.weight.data = torch.rand(10, generator=g) + 0.5
        self.bn.bias.data = torch.randn(10, generator=g)
        self.bn.running_mean.copy_(torch.randn(10, generator=g))
        self.bn.running_var.copy_(torch.rand(10, generator=g) + 0.5)
        self.frozen = nn.Parameter(torch.randn(7, generator=g), requires_grad=False)

    def get_params(self):
        v = list(self.vecs)
        return [self.conv.weight] + v[0::4], [self.bn.weight, self.frozen] + v[1::4], v[2::4], [self.bn.bias] + v[3::4]


def trainable_names(net):
    return [k for k, p in net.named_parameters() if p.requires_grad]


def forward_side_effects(net, step):
    """What a forward pass would do to the BatchNorm buffers before optimizer step `step` (1-based): the EMA-only entries move."""
    with torch.no_grad():
        net.bn.running_mean.add_(0.01 * step)
        net.bn.running_var.mul_(1.0 + 0.01 * step)
        net.bn.num_batches_tracked.add_(1)


def fixture_rule(x, x64, x0, ref_dist, steps, factor):
    """The rule for fixture comparisons, on the CHANGE since the initial state: ||d - d64|| <= max(factor x the fp32 reference's
    own ||d32 - d64|| on this tensor, 4 K 2^-24 ||x64||) with K the number of steps -- the floor is four fp32 roundings per element
    and step (g*coef, the momentum update, the parameter update, the EMA fold), derived, not tuned.  -> (distance, bound)"""
    x, x64, x0 = (t.detach().double().cpu().reshape(-1) for t in (x, x64, x0))
    dist = float(((x - x0) - (x64 - x0)).norm())
    return dist, max(factor * float(ref_dist), 4 * steps * 2.0 ** -24 * float(x64.norm()))


class Fixture:
    def __init__(self):
        self.z = dict(np.load(os.path.join(GOLDEN, "g6_optim_tail.npz")))
        for s in SNAPSHOTS:
            self.z.update(np.load(os.path.join(GOLDEN, f"g6_optim_tail_f64_s{s}.npz")))
        self.names = [str(n) for n in self.z["grad_names"]]
        self.inf_step = int(self.z["inf_step"])  # 1-based

    def gradients(self, step, dtype=torch.float32):
        """{name: gradient} of step `step` (1-based): int8 values x a power-of-two scale, exact in fp32; the inf step carries
        one inf element."""
        out = {}
        for k in self.names:
            g = torch.from_numpy(self.z[f"grad.{k}"][step - 1].astype(np.float64) * float(self.z["grad_scale"][step - 1]))
            out[k] = g.to(dtype)
        if step == self.inf_step:
            out[str(self.z["inf_name"])].view(-1)[int(self.z["inf_index"])] = float("inf")
        return out

    def set_grads(self, net, step):
        params = dict(net.named_parameters())
        for k, g in self.gradients(step, next(iter(params.values())).dtype).items():
            p = params[k]
            p.grad = torch.empty_like(p).copy_(g.reshape(p.shape))  # the parameter's own strides (channels_last weight)


def make_tail(net, **over):
    from cabinet_amd.optim import FusedSGDTail

    kw = dict(HYPER, max_grad_norm=MAX_NORM, ema=True, ema_decay=EMA_DECAY, ema_tau=EMA_TAU)
    kw.update(over)
    return FusedSGDTail(net, **kw)


def buffers_of(opt, net):
    return {k: opt.optim.state[p]["momentum_buffer"] for k, p in net.named_parameters() if p.requires_grad}


def check_scalars(fx, opt, step):
    """norm and learning rates after step `step` against the fixture (module docstring)."""
    z = fx.z
    norm = float(opt.last_grad_norm.cpu()[0])
    if step == fx.inf_step:
        assert not np.isfinite(norm)
        return
    want = float(z["norm64"][step - 1])
    print(f"step {step}: norm {norm:.9g} (fp64 {want:.9g}, rel {abs(norm - want) / want:.2e})  lr {opt.lr.cpu().tolist()}")
    assert abs(norm - want) <= 1e-6 * want
    got, ref = opt.lr.cpu().numpy().astype(np.float32), z["lr32"][step - 1]
    it = step - 1 - (1 if step > fx.inf_step else 0)
    if it < HYPER["warmup_steps"]:
        assert np.array_equal(got, ref), (step, got, ref)
    else:
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(ref).astype(np.float64)), (step, got, ref)


def check_snapshot(fx, net, opt, step):
    """Every parameter, momentum buffer and EMA entry after `step` steps under the fixture rule; prints each figure."""
    z, bad = fx.z, []
    kinds = dict(param=dict(net.state_dict()), buf=buffers_of(opt, net), ema=dict(opt.ema.state_dict()))
    for kind, tensors in kinds.items():
        names = fx.names if kind == "buf" else [str(n) for n in z["names"]]
        for k in names:
            x64 = torch.from_numpy(z[f"s{step}.f64.{kind}.{k}"])
            x0 = torch.zeros_like(x64) if kind == "buf" else torch.from_numpy(z[f"init.{k}"]).double()
            dist, bound = fixture_rule(tensors[k], x64, x0, z[f"s{step}.dist.{kind}.{k}"], step, ALLOW_FACTOR)
            print(f"s{step} {kind:5s} {k:22s} dist {dist:.3e} bound {bound:.3e} ref32 {float(z[f's{step}.dist.{kind}.{k}']):.3e}")
            if not dist <= bound:
                bad.append((kind, k, dist, bound))
    assert not bad, bad
    assert opt.it == int(z[f"s{step}.it"]) and opt.ema_updates == int(z[f"s{step}.updates"])


def drive(fx, net, opt, first, last, each=None):
    for s in range(first, last + 1):
        forward_side_effects(net, s)
        fx.set_grads(net, s)
        opt.step()
        if each is not None:
            each(s)
