"""What gradient accumulation in the graphed step costs (K21; needs an MI355X, fails without one).  Writes profiles/grad_accum.md.

Part 1 -- the accumulate pass alone, on the gradient set of build_model("large", 19) with seeded gradients, replayed from
hipGraphs and alternated in one process, REPEATS rounds of STEPS replays each:
    K later   [cabinet_grad_accum]                         acc += grad            12 bytes per element
    F later   [torch._foreach_add_(accs, grads)]           the same update as stock multi-tensor kernels
    K first   [cabinet_grad_accum, cabinet_grad_accum_reset]   acc = grad         8 bytes per element; the reset keeps every
                                                           replay a window's first micro-step, and is timed alone (K reset)
    F first   [torch._foreach_copy_(accs, grads)]
reported as device-event time per replay with the spread over the rounds, the bytes moved and the share of the element-wise HBM
ceiling.

Part 2 -- the whole GraphedTrainStep at BASELINE config 3 (8 x 3 x 1024 x 1024, 19 classes) at accum_steps=1, this tree against
a checkout of the parent commit (--parent-tree DIR, built), alternating: one child process per run, each under its own timeout.
These are the same graphs, so a difference beyond the spread is a finding.  With --accum K a third row times this tree at
accum_steps=K (per micro-step).

    python tools/time_grad_accum.py [--steps 200] [--repeats 5] [--rounds 3] [--parent-tree DIR] [--accum 4] [--out FILE]
"""
import argparse
import atexit
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_CEILING = 6.3e12  # bytes/s an element-wise kernel reaches on MI355X (the figure tools/time_optimizer_tail.py uses for K16)
CHILD_TIMEOUT = 240   # seconds, each child process


def _setup(root):
    """The tree to import from, and the committed MIOpen database on a private copy with FAST find mode, as bench.py runs."""
    sys.path[:0] = [root]
    db_src = os.path.join(root, "cabinet_amd", "miopen_db")
    if os.path.isdir(db_src) and "MIOPEN_USER_DB_PATH" not in os.environ:
        tmp = tempfile.mkdtemp(prefix="cabinet_miopen_accum_")
        shutil.copytree(db_src, os.path.join(tmp, "db"), copy_function=shutil.copyfile)
        for d, _, _ in os.walk(tmp):
            os.chmod(d, 0o700)
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        os.environ["MIOPEN_USER_DB_PATH"] = os.path.join(tmp, "db")
        os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", os.path.join(tmp, "db", "cache"))
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")


def _stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


# ---- children ---------------------------------------------------------------------------------------------------------------------
def child_kernel(steps, repeats):
    _setup(HERE)
    import torch

    from cabinet_amd.optim import GradAccumulator
    from cabinet_amd.train import build_model

    net = build_model("large", n_classes=19, device="cuda", seed=0, gamma=0.5).train()
    g = torch.Generator(device="cpu").manual_seed(7)
    grads = [torch.empty_like(p).copy_(torch.randn(p.shape, generator=g) * 1e-3) for p in net.parameters() if p.requires_grad]
    accs = [torch.zeros_like(x) for x in grads]
    accs_f = [torch.zeros_like(x) for x in grads]
    ga = GradAccumulator(list(zip(accs, grads)))
    ga.add(), ga.reset()  # first launches outside capture
    torch._foreach_add_(accs_f, grads), torch._foreach_copy_(accs_f, grads)
    torch.cuda.synchronize()

    def graph_of(fn):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode="thread_local"):
            fn()
        return gr

    graphs = {"K later": graph_of(ga.add), "F later": graph_of(lambda: torch._foreach_add_(accs_f, grads)),
              "K first": graph_of(lambda: (ga.add(), ga.reset())), "F first": graph_of(lambda: torch._foreach_copy_(accs_f, grads)),
              "K reset": graph_of(ga.reset)}
    times = {k: [] for k in graphs}
    for r in range(repeats + 1):  # round 0 warms up
        for name, gr in graphs.items():
            if name == "K later":
                ga.micro = 1
            elif name == "K first":
                ga.micro = 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(1e3 * e0.elapsed_time(e1) / steps)
        for a in accs + accs_f:  # keep the sums small: thousands of adds of the same gradient
            a.zero_()
    numel = sum(x.numel() for x in grads)
    print("RESULT " + json.dumps(dict(device=torch.cuda.get_device_name(0), tensors=len(grads), chunks=len(ga._chunks_host),
                                      numel=numel, steps=steps, repeats=repeats, us={k: _stats(v) for k, v in times.items()})))


def child_step(tree, accum, steps):
    _setup(tree)
    import torch

    from cabinet_amd.train import GraphedTrainStep, build_model, make_criteria, synthetic_batch

    im, lb = synthetic_batch(8, 1024, 1024, 19, "cuda", seed=1)
    net = build_model("large", n_classes=19, device="cuda", seed=0, gamma=0.5).train()
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4, momentum=0.9, weight_decay=5e-4)
    kw = dict(accum_steps=accum) if accum > 1 else {}  # the parent's step does not take the argument
    step = GraphedTrainStep(net, make_criteria(8, 1024, 1024, "cuda"), optimizer=opt, **kw)
    for _ in range(2 * max(accum, 2) + accum):
        step(im, lb)
    assert step.g_bwd is not None
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            step(im, lb)
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    print("RESULT " + json.dumps(dict(ms=out, fallbacks=step.fallbacks)))


# ---- driver -------------------------------------------------------------------------------------------------------------------------
def run_child(args):
    """One child process under its own time limit; returns its RESULT record, raises on any other end."""
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), *args]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} ended with {r.returncode}; nothing further is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def fmt(s, digits=1):
    return f"{s['median']:.{digits}f} [{s['min']:.{digits}f}, {s['max']:.{digits}f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit; without it part 2 is skipped")
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grad_accum.md"))
    ap.add_argument("--child", default=None, choices=["kernel", "step"])
    ap.add_argument("--tree", default=HERE)
    a = ap.parse_args()
    if a.child == "kernel":
        return child_kernel(a.steps, a.repeats)
    if a.child == "step":
        return child_step(os.path.abspath(a.tree), a.accum, a.steps)

    k = run_child(["--child", "kernel", "--steps", str(a.steps), "--repeats", str(a.repeats)])
    print(json.dumps(k), flush=True)
    us, n = k["us"], k["numel"]
    lines = ["# Gradient accumulation in the graphed step: the accumulate pass (K21) and the step around it", "",
             f"{k['device']}, `python tools/time_grad_accum.py --steps {a.steps} --repeats {a.repeats} --rounds {a.rounds}`"
             + (" --parent-tree <checkout of the parent commit>" if a.parent_tree else "") + ".", "",
             "## The accumulate pass alone", "",
             f"Gradient set of `build_model(\"large\", 19)`: {k['tensors']} tensors, {k['chunks']} chunks, {n:,} elements. Each row is a "
             f"hipGraph replayed {a.steps} times between two events; the rows alternate in one process, {a.repeats} rounds after "
             "one warm-up round; µs per replay, median [min, max] over the rounds.", "",
             "| graph | µs per replay | bytes | share of the 6.3 TB/s element-wise HBM ceiling |", "|---|---|---|---|"]
    # K first includes the reset launch; K reset alone is the floor of replaying a graph of one tiny kernel, not that launch's
    # share of a longer graph, so it is shown beside the row and NOT subtracted: the share of K first is a lower bound
    for name, per, what in (("K later", 12, "`cabinet_grad_accum`, `acc += grad`"), ("F later", 12, "captured `torch._foreach_add_`"),
                            ("K first", 8, "`cabinet_grad_accum` + `cabinet_grad_accum_reset`, `acc = grad`"),
                            ("F first", 8, "captured `torch._foreach_copy_`")):
        t = us[name]["median"]
        lines.append(f"| {name}: {what} | {fmt(us[name])} | {per} B × {n:,} = {per * n / 1e6:.1f} MB | "
                     f"{'at least ' if name == 'K first' else ''}{100 * (1e6 * per * n / HBM_CEILING) / t:.0f} % |")
    lines += [f"| K reset: `cabinet_grad_accum_reset` alone (the floor of a one-kernel graph) | {fmt(us['K reset'])} | | |", ""]
    if a.parent_tree:
        rows = {"this tree, accum_steps=1": (HERE, 1), "parent commit": (os.path.abspath(a.parent_tree), 1),
                f"this tree, accum_steps={a.accum} (per micro-step)": (HERE, a.accum)}
        ms = {name: [] for name in rows}
        for r in range(a.rounds):
            for name, (tree, accum) in rows.items():
                res = run_child(["--child", "step", "--tree", tree, "--accum", str(accum), "--steps", str(a.steps)])
                ms[name] += res["ms"]
                print(r, name, res, flush=True)
        lines += ["## The whole step", "",
                  f"`GraphedTrainStep` at config 3 (8 × 3 × 1024², CABiNet-Large, 19 classes, plain eager SGD as `bench.py`), one child "
                  f"process per run under its own time limit, the rows alternating, {a.rounds} rounds of 3 × {a.steps} steps; ms per "
                  "call (host wall time around a synchronise), median [min, max] over all runs.", "",
                  "| step | ms per call |", "|---|---|"]
        lines += [f"| {name} | {fmt(_stats(v), 3)} |" for name, v in ms.items()] + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
