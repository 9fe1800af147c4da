#!/usr/bin/env python3
"""Golden vectors for the optimizer tail (cabinet_amd.optim.FusedSGDTail, csrc/opt_tail.hip), produced by running the REFERENCE's
own step tail -- torch.nn.utils.clip_grad_norm_, src/utils/optimizer.py:Optimizer, src/utils/ema.py:ModelEMA, in the order of
src/scripts/train.py:411-427 -- on the synthetic module of tests/optim_tail_model.py, once in fp32 and once with everything in
double.

Needs a checkout of the reference:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_optim_tail.py REFERENCE_ROOT
Writes, data only:
  g6_optim_tail.npz           hyper-parameters; names (floating-point state_dict entries) and grad_names (trainable parameters);
                              init.<name> (every state_dict entry); grad.<name> (STEPS, numel) int8 with grad_scale (STEPS,), the
                              gradient of step s being int8 x scale -- exact in fp32 --, in the parameter's logical element order;
                              inf_step / inf_name / inf_index: that step's gradient has one inf element (no step, no EMA update,
                              as scaler.step and the `optim.it != prev_it` gate of train.py:419-427 leave it);
                              lr64 / lr32 (STEPS, groups) and norm64 / norm32 (STEPS,) per step (nan lr on the skipped step);
                              s<K>.it, s<K>.updates and s<K>.f32.{param,buf,ema}.<name> after K = 5 and K = 8 steps;
                              s<K>.dist.{param,buf,ema}.<name> = ||d32 - d64||, the fp32 reference's own distance from the fp64
                              run on the CHANGE d = x_after - x_0 of that tensor.
  g6_optim_tail_f64_s<K>.npz  s<K>.f64.{param,buf,ema}.<name>: the double run (one file per snapshot: size limit per file).
Before every step s the BatchNorm buffers move as optim_tail_model.forward_side_effects(net, s) says (a stand-in for the forward
pass, so that the EMA-only entries have something to average).

Asserted before anything is written: the steps never pass max_iter (where the reference's (1 - k) ** power leaves the reals), the
warm-up boundary is crossed, at least two steps clip and two do not, and the fp32 reference itself passes the rule the tests apply
(tests/optim_tail_model.py::fixture_rule) with factor 1.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    sys.exit(__doc__)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, sys.argv[1])
from src.utils.ema import ModelEMA  # noqa: E402
from src.utils.optimizer import Optimizer  # noqa: E402

from optim_tail_model import (EMA_DECAY, EMA_TAU, HYPER, MAX_NORM, SNAPSHOTS, STEPS, TailNet, fixture_rule,  # noqa: E402
                              forward_side_effects, trainable_names)

INF_STEP = 4
# norms: int8 values uniform in [-127, 127] have rms 73.3; x sqrt(22,014 elements) = 10,880; 2^-13 -> 1.33 (clipped), 2^-14 -> 0.66
SCALES = [2.0 ** -13, 2.0 ** -14, 2.0 ** -13, 2.0 ** -13, 2.0 ** -14, 2.0 ** -13, 2.0 ** -14, 2.0 ** -12]

proto = TailNet(seed=0)
grad_names = trainable_names(proto)
names = [k for k, v in proto.state_dict().items() if v.dtype.is_floating_point]
g = torch.Generator().manual_seed(1)
grads_q = {k: torch.randint(-127, 128, (STEPS, p.numel()), generator=g, dtype=torch.int8)
           for k, p in proto.named_parameters() if p.requires_grad}
inf_name, inf_index = "vecs.12", 4096  # the one element of the 4097-vector past its first chunk


def gradients(step, dtype):
    out = {k: (q[step - 1].double() * SCALES[step - 1]).to(dtype) for k, q in grads_q.items()}
    if step == INF_STEP:
        out[inf_name][inf_index] = float("inf")
    return out


def run(dtype):
    net = TailNet(seed=0).to(dtype)
    optim = Optimizer(net, **HYPER)
    ema = ModelEMA(net, decay=EMA_DECAY, tau=EMA_TAU)
    params = dict(net.named_parameters())
    x0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    lrs, norms, snaps = [], [], {}
    for step in range(1, STEPS + 1):
        forward_side_effects(net, step)
        for k, gr in gradients(step, dtype).items():
            params[k].grad = torch.empty_like(params[k]).copy_(gr.reshape(params[k].shape))
        # train.py:411-427 without a GradScaler: clip, step unless a gradient is inf / nan, EMA only behind a real step
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), MAX_NORM)
        norms.append(float(norm))
        if torch.isfinite(norm):
            assert optim.it < optim.max_iter, "the schedule must not pass max_iter"
            lrs.append([optim.get_lr(i, pg) for i, pg in enumerate(optim.optim.param_groups)])
            optim.step()
            ema.update(net)
        else:
            lrs.append([float("nan")] * len(optim.optim.param_groups))
        optim.zero_grad()
        if step in SNAPSHOTS:
            esd = ema.ema.state_dict()
            snaps[step] = dict(it=optim.it, updates=ema.updates,
                               param={k: net.state_dict()[k].detach().clone() for k in names},
                               buf={k: optim.optim.state[params[k]]["momentum_buffer"].detach().clone() for k in grad_names},
                               ema={k: esd[k].detach().clone() for k in names})
            for k, v in esd.items():
                if not v.dtype.is_floating_point:
                    assert torch.equal(v, x0[k]), "integer buffers stay as copied"
    return x0, lrs, norms, snaps


x0, lr32, norm32, snap32 = run(torch.float32)
x0_64, lr64, norm64, snap64 = run(torch.float64)
assert all(torch.equal(x0[k].double(), x0_64[k].double()) for k in x0)
finite = [n for n in norm64 if np.isfinite(n)]
assert sum(n > MAX_NORM for n in finite) >= 2 and sum(n < MAX_NORM for n in finite) >= 2, norm64
assert not np.isfinite(norm64[INF_STEP - 1]) and len(finite) == STEPS - 1
assert snap64[STEPS]["it"] == STEPS - 1 > HYPER["warmup_steps"] and snap64[STEPS]["it"] <= HYPER["max_iter"]
assert snap32[5]["it"] == snap64[5]["it"] == 4 and snap32[5]["updates"] == 4

out = dict(names=np.array(names), grad_names=np.array(grad_names), grad_scale=np.array(SCALES), inf_step=np.int64(INF_STEP),
           inf_name=np.array(inf_name), inf_index=np.int64(inf_index), max_norm=np.float64(MAX_NORM), ema_decay=np.float64(EMA_DECAY),
           ema_tau=np.float64(EMA_TAU), lr64=np.array(lr64, dtype=np.float64), lr32=np.array(lr64, dtype=np.float64).astype(np.float32),
           norm64=np.array(norm64), norm32=np.array(norm32), **{f"hyper.{k}": np.float64(v) for k, v in HYPER.items()})
# the fp32 run's host schedule is the same Python arithmetic as the double run's
assert np.array_equal(np.array(lr32), np.array(lr64), equal_nan=True)
for k, v in x0.items():
    out[f"init.{k}"] = v.numpy()
for k, q in grads_q.items():
    out[f"grad.{k}"] = q.numpy()
f64 = {s: {} for s in SNAPSHOTS}
worst = 0.0
for s in SNAPSHOTS:
    out[f"s{s}.it"], out[f"s{s}.updates"] = np.int64(snap32[s]["it"]), np.int64(snap32[s]["updates"])
    for kind in ("param", "buf", "ema"):
        for k, v32 in snap32[s][kind].items():
            v64 = snap64[s][kind][k]
            start = torch.zeros_like(v64) if kind == "buf" else x0[k].double()
            dist = float(((v32.double() - start) - (v64 - start)).norm())
            out[f"s{s}.f32.{kind}.{k}"] = v32.numpy()
            out[f"s{s}.dist.{kind}.{k}"] = np.float64(dist)
            f64[s][f"s{s}.f64.{kind}.{k}"] = v64.numpy()
            # the tests' rule, applied to the fp32 reference itself with factor 1 (so it is known to be satisfiable); how far the
            # reference's own distance is from the derived floor is printed
            got, bound = fixture_rule(v32, v64, start, dist, s, 1.0)
            assert got <= bound, (s, kind, k, got, bound)
            floor = 4 * s * 2.0 ** -24 * float(v64.norm())
            worst = max(worst, dist / floor if floor > 0 else 0.0)
print(f"norms {['%.4f' % n for n in norm64]}")
print(f"lr (group 0) {['%.6g' % r[0] for r in lr64]}")
print(f"largest fp32-reference distance / derived floor over all tensors: {worst:.3f}")
path = os.path.join(HERE, "g6_optim_tail.npz")
np.savez_compressed(path, **out)
total = os.path.getsize(path)
print("wrote g6_optim_tail.npz", total)
for s in SNAPSHOTS:
    p = os.path.join(HERE, f"g6_optim_tail_f64_s{s}.npz")
    np.savez_compressed(p, **f64[s])
    print(f"wrote g6_optim_tail_f64_s{s}.npz", os.path.getsize(p))
    total += os.path.getsize(p)
    assert os.path.getsize(p) < 2 ** 20
assert os.path.getsize(path) < 2 ** 20 and total < 2e6, total
