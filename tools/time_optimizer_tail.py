"""What the optimizer tail of the step costs, and what the fused kernels change (needs an MI355X; fails without one).

The tail is everything the reference does between backward and the next forward (src/scripts/train.py:411-427):
clip_grad_norm_, Optimizer.step() (host-side warm-up / poly schedule + SGD with momentum and weight decay), ModelEMA.update().

Part 1 -- the tail alone, on the parameter set of build_model("large", 19) with seeded gradients, 10 warm-up steps then
REPEATS x STEPS steps each of
    A  the eager reference-semantics tail (clip_grad_norm_, host schedule, torch SGD, per-entry EMA loop)
    B  cabinet_amd.optim.FusedSGDTail, eager (three launches + the host's address check)
    C  the same from a hipGraph
reported as host wall time around a final synchronise and as device-event time, with the spread over the repeats; the bytes the
update has to move and the resulting share of the element-wise HBM ceiling; and the outputs of A and C after 8 steps from the same
state compared under the fixture rule of tests/optim_tail_model.py against the same tail in double.

Part 2 -- the whole GraphedTrainStep at BASELINE config 3 (8 x 3 x 1024 x 1024, 19 classes), alternating in one process:
    P  the step bench.py times (plain SGD, eager, no clipping, no EMA): the parent's step
    A  with the eager reference-semantics tail
    C  with FusedSGDTail captured (capture_optimizer=True)

    python tools/time_optimizer_tail.py [--steps 200] [--repeats 5] [--rounds 4] [--skip-step]
"""
import argparse
import atexit
import copy
import math
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
# the committed MIOpen database on a private copy and FAST find mode, as bench.py and tests/conftest.py run
_db_src = os.path.join(ROOT, "cabinet_amd", "miopen_db")
if os.path.isdir(_db_src) and "MIOPEN_USER_DB_PATH" not in os.environ:
    _tmp = tempfile.mkdtemp(prefix="cabinet_miopen_tail_")
    shutil.copytree(_db_src, os.path.join(_tmp, "db"), copy_function=shutil.copyfile)
    for _dir, _, _ in os.walk(_tmp):
        os.chmod(_dir, 0o700)
    atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    os.environ["MIOPEN_USER_DB_PATH"] = os.path.join(_tmp, "db")
    os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", os.path.join(_tmp, "db", "cache"))
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402

from cabinet_amd.optim import FusedSGDTail  # noqa: E402
from cabinet_amd.train import GraphedTrainStep, build_model, make_criteria, synthetic_batch  # noqa: E402

HBM_CEILING = 6.3e12  # bytes/s an element-wise kernel reaches on MI355X (the HIP guide's Appendix B figure)
# the reference's defaults (configs/*.yaml: max_grad_norm 1.0, warmup_steps 4000, ema_decay 0.9999); lr0 as bench.py's SGD
HYPER = dict(lr0=1e-4, momentum=0.9, wd=5e-4, warmup_steps=4000, warmup_start_lr=1e-5, max_iter=100000, power=0.9, lr_multiplier=10.0)
MAX_NORM, EMA_DECAY, EMA_TAU = 1.0, 0.9999, 2000


class ReferenceTail:
    """Tail A: the reference's sequence, eagerly, with its formulas (optimizer.py:124-156, ema.py:51-62)."""

    def __init__(self, net, hyper=HYPER):
        self.net, self.h, self.it, self.updates = net, hyper, 0, 0
        wd_p, nowd_p, lr_wd_p, lr_nowd_p = net.get_params()
        groups = [dict(params=wd_p, weight_decay=hyper["wd"]), dict(params=nowd_p, weight_decay=0.0),
                  dict(params=lr_wd_p, weight_decay=hyper["wd"], lr_scale=hyper["lr_multiplier"]),
                  dict(params=lr_nowd_p, weight_decay=0.0, lr_scale=hyper["lr_multiplier"])]
        self.optim = torch.optim.SGD([g for g in groups if g["params"]], lr=hyper["lr0"], momentum=hyper["momentum"], weight_decay=0.0)
        self.ema = copy.deepcopy(net).eval()
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self.last_grad_norm = None

    @property
    def param_groups(self):
        return self.optim.param_groups

    def step(self):
        h = self.h
        self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self.net.parameters(), MAX_NORM)
        if self.it < h["warmup_steps"]:
            lr = h["warmup_start_lr"] + self.it / h["warmup_steps"] * (h["lr0"] - h["warmup_start_lr"])
        else:
            lr = h["lr0"] * (1 - max((self.it - h["warmup_steps"]) / (h["max_iter"] - h["warmup_steps"]), 0.0)) ** h["power"]
        for pg in self.optim.param_groups:
            pg["lr"] = lr * pg.get("lr_scale", 1.0)
        self.optim.step()
        self.it += 1
        self.updates += 1
        d = EMA_DECAY * (1 - math.exp(-self.updates / EMA_TAU))
        msd = self.net.state_dict()
        with torch.no_grad():
            for k, v in self.ema.state_dict().items():
                if v.dtype.is_floating_point:
                    v.mul_(d).add_(msd[k].detach(), alpha=1 - d)


def seeded_gradients(net, seed=7, scale=1e-3):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for p in net.parameters():
        if p.requires_grad:
            p.grad = torch.empty_like(p).copy_(torch.randn(p.shape, generator=g) * scale)


def spread(xs):
    return f"median {statistics.median(xs):8.1f}  min {min(xs):8.1f}  max {max(xs):8.1f}"


def time_tail(label, fn, steps, repeats, warmup=10):
    """us per step: host wall time around a final synchronise, and device-event time, per repeat."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0) / steps)
        dev.append(1e3 * e0.elapsed_time(e1) / steps)
    print(f"{label:44s} wall us/step: {spread(wall)}   device events us/step: {spread(dev)}   ({repeats} x {steps} steps)", flush=True)
    return statistics.median(wall), statistics.median(dev)


def tail_bytes(opt):
    """Bytes one step has to move: an owned entry is read for the norm (g) and read (p, g, buf, ema) and written (p, buf, ema)
    by the apply pass = 8 passes of 4 bytes; an EMA-only entry is read twice and written once."""
    owned = sum(t.numel() for t, gi in zip(opt._live, opt._group) if gi >= 0 and t.grad is not None)
    ema_only = sum(t.numel() for t in opt._live) - owned
    return 4 * (8 * owned + 3 * ema_only), owned, ema_only


def part1(steps, repeats):
    print("== part 1: the tail alone, parameter set of build_model('large', 19) ==", flush=True)
    nets = {k: build_model("large", n_classes=19, device="cuda", seed=0, gamma=0.5).train() for k in "ABC"}
    for net in nets.values():
        seeded_gradients(net)
    a = ReferenceTail(nets["A"])
    b = FusedSGDTail(nets["B"], **HYPER, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY, ema_tau=EMA_TAU)
    c = FusedSGDTail(nets["C"], **HYPER, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY, ema_tau=EMA_TAU)
    nbytes, owned, ema_only = tail_bytes(c)
    n_float = len(c._live)
    print(f"entries {n_float} ({sum(1 for g in c._group if g >= 0)} in param groups), chunks {len(c._chunks_host)}, owned elements "
          f"{owned}, EMA-only elements {ema_only}; bytes per step 4 * (8 * owned + 3 * ema_only) = {nbytes / 1e6:.1f} MB; at the "
          f"element-wise HBM ceiling of {HBM_CEILING / 1e12:.1f} TB/s: {1e6 * nbytes / HBM_CEILING:.1f} us", flush=True)
    c.step()  # first launch outside capture
    c.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        c.step()
    res = {"A": time_tail("A eager reference tail", a.step, steps, repeats),
           "B": time_tail("B FusedSGDTail eager", b.step, steps, repeats),
           "C": time_tail("C FusedSGDTail from a hipGraph", graph.replay, steps, repeats)}
    for k in "BC":
        print(f"{k}: device time {res[k][1]:.1f} us/step = {100 * (1e6 * nbytes / HBM_CEILING) / res[k][1]:.0f} % of the HBM ceiling "
              f"({nbytes / res[k][1] / 1e6:.2f} TB/s; the four arrays, 167 MB, also fit the 256 MB Infinity Cache, so this is a share "
              "of the HBM ceiling by name, not proof of HBM traffic)")
    print(f"A / C: wall {res['A'][0] / res['C'][0]:.1f}x, device {res['A'][1] / res['C'][1]:.1f}x", flush=True)
    del nets, a, b, c, graph
    torch.cuda.empty_cache()


def compare_outputs(k_steps=8):
    """Outputs of A and C on the timed tensors after k_steps from the same state, against tail A in double, per tensor under the
    fixture rule: ||d_C - d_64|| <= max(3 x ||d_A - d_64||, 4 K 2^-24 ||x_64||) on the change d of parameters, buffers and EMA."""
    from optim_tail_model import fixture_rule
    from parity_rules import ALLOW_FACTOR

    print(f"== outputs of A and C after {k_steps} steps from the same state, vs the tail in double ==", flush=True)
    hyper = dict(HYPER, lr0=0.05, warmup_steps=3, max_iter=k_steps + 2)  # updates far above the parameters' fp32 rounding
    base = build_model("large", n_classes=19, device="cuda", seed=0, gamma=0.5).train()
    x0 = {k: v.detach().clone() for k, v in base.state_dict().items()}
    na, nc, n64 = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base).double()
    a, a64 = ReferenceTail(na, hyper), ReferenceTail(n64, hyper)
    c = FusedSGDTail(nc, **hyper, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY, ema_tau=EMA_TAU)
    for s in range(k_steps):
        for net in (na, nc, n64):
            seeded_gradients(net, seed=100 + s, scale=1e-3 if s % 2 else 2e-4)
        a.step(), a64.step(), c.step()
    torch.cuda.synchronize()
    worst, fails, count = 0.0, [], 0
    def bufs_of(net, sgd):
        names = {id(p): k for k, p in net.named_parameters()}
        return {names[id(p)]: st["momentum_buffer"] for p, st in sgd.state.items() if st.get("momentum_buffer") is not None}

    sets = [(dict(nc.state_dict()), dict(na.state_dict()), dict(n64.state_dict()), x0, "param"),
            (dict(c.ema.state_dict()), dict(a.ema.state_dict()), dict(a64.ema.state_dict()), x0, "ema"),
            (bufs_of(nc, c.optim), bufs_of(na, a.optim), bufs_of(n64, a64.optim), None, "buf")]
    for got, ref32, ref64, start, kind in sets:
        for k, x64 in ref64.items():
            if not x64.dtype.is_floating_point:
                continue
            s0 = torch.zeros_like(x64) if start is None else start[k].double()
            ref_dist, _ = fixture_rule(ref32[k], x64, s0, 0.0, k_steps, 1.0)
            dist, bound = fixture_rule(got[k], x64, s0, ref_dist, k_steps, ALLOW_FACTOR)
            count += 1
            worst = max(worst, dist / bound if bound > 0 else 0.0)
            if not dist <= bound:
                fails.append((kind, k, dist, bound))
    print(f"{count} tensors; worst distance / bound {worst:.3f}; outside the rule: {len(fails)} {fails[:5]}")
    print(f"norm of the last step: A {float(a.last_grad_norm):.9g}  C {float(c.last_grad_norm.cpu()[0]):.9g}  double {float(a64.last_grad_norm):.12g}",
          flush=True)
    assert not fails
    del base, na, nc, n64, a, a64, c
    torch.cuda.empty_cache()


def part2(steps, rounds):
    print("== part 2: GraphedTrainStep at config 3 (8 x 3 x 1024 x 1024, 19 classes), alternating ==", flush=True)
    im, lb = synthetic_batch(8, 1024, 1024, 19, "cuda", seed=1)
    variants = {}
    for name in "PAC":
        net = build_model("large", n_classes=19, device="cuda", seed=0, gamma=0.5).train()
        crit = make_criteria(8, 1024, 1024, "cuda")
        if name == "P":
            opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4, momentum=0.9, weight_decay=5e-4)
            step = GraphedTrainStep(net, crit, optimizer=opt)
        elif name == "A":
            step = GraphedTrainStep(net, crit, optimizer=ReferenceTail(net))
        else:
            opt = FusedSGDTail(net, **HYPER, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY, ema_tau=EMA_TAU)
            step = GraphedTrainStep(net, crit, optimizer=opt, capture_optimizer=True)
        for _ in range(5):
            step(im, lb)
        torch.cuda.synchronize()
        variants[name] = step
    assert variants["C"].opt_seg.graph is not None
    label = {"P": "P parent's step (plain SGD, eager)", "A": "A eager reference tail", "C": "C FusedSGDTail captured"}
    times = {k: [] for k in variants}
    for r in range(rounds):
        for name, step in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(im, lb)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / steps
            times[name].append(ms)
            print(f"round {r} {label[name]:38s} {ms:8.3f} ms/step   fallbacks {step.fallbacks}", flush=True)
    for name in variants:
        print(f"{label[name]:38s} median {statistics.median(times[name]):8.3f} ms/step  min {min(times[name]):8.3f}  max {max(times[name]):8.3f} "
              f"over {rounds} runs of {steps} steps")
    print(f"C - A: {statistics.median(times['C']) - statistics.median(times['A']):+.3f} ms/step;  "
          f"C - P: {statistics.median(times['C']) - statistics.median(times['P']):+.3f} ms/step", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--skip-step", action="store_true", help="part 1 and the output comparison only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_optimizer_tail.py measures on an MI355X: no GPU in this process")
    if args.steps < 200:
        print(f"NOTE: --steps {args.steps} is below the 200 steps the documented numbers were taken with")
    print(torch.cuda.get_device_name(0), flush=True)
    part1(args.steps, args.repeats)
    compare_outputs()
    if not args.skip_step:
        part2(args.steps, args.rounds)
