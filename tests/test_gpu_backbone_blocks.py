"""The code that COMPOSES the backbone and spatial-branch kernels -- `_FusedSequential.forward` (cabinet_amd/models/mobilenetv3.py),
`ConvBNReLU.forward` / `_conv3x3_bn_relu` (cabinet_amd/models/cabinet.py), `Conv2dS2` / `_Conv3x3S2` (cabinet_amd/functional.py) --
module by module against the fp64 CPU copy of the same module (tables, oracle and kink predicate: tests/backbone_block_cases.py).

1. Every block configuration of both backbones (21 distinct rows) plus `conv_3x3_bn(3, 16, 2)`, `conv_1x1_bn(160, 960)` and
   `conv_1x1_bn(96, 576)`, training mode, B = 2, planes 13 x 19 and 20 x 12, forward and backward: output, dx and every parameter
   gradient by ||a-b|| <= 1e-3 ||b|| (the maps also max|a-b| <= 1e-3 max|b|), running buffers at 1e-5, `num_batches_tracked`
   exactly, two device runs bit-equal, and the sequence of routes the state machine took against the table's claim.
2. The routes production takes and small planes do not: K10 inside a block either side of P = 65536; the spatial branch's four
   ConvBNReLU modules and the backbone's first layer alone, either side of the K15 weight-gradient thresholds, the stem as one node
   and as two; frozen parameters, eval mode in a grad-recording forward, `torch.no_grad()`, channels_last and offset inputs.
3. The whole chain (`mobilenetv3_large`, `mobilenetv3_small`, `SpatialBranch`), a `torch.no_grad()` forward (so the 1x1 and
   stride-2 convolutions are the stock operator and the stem is two nodes; the routes of a recording forward are parts 1 and 2's),
   at ragged image sizes, training and eval: output and every running buffer within max(10 d32, 1e-5) (never above 1e-3) of fp64, d32 the fp32 CPU copy's own distance.

No-GPU tests: the configuration count, the kink predicate for every row of every table, the K15 plan restatements, and that the
claimed routes cover every route of the state machine.
"""
import contextlib
import copy
import functools

import pytest
import torch
import torch.nn as nn

import backbone_block_cases as bc
from test_gpu_backbone_edges import _all_equal, _cmp, _report

gpu = pytest.mark.gpu
TOL = 1e-3      # north_star: 1e-3 relative per tensor; the maps also in the max norm
TOL_STAT = 1e-5  # running statistics

PART1 = bc.part1_cases()
K10 = bc.k10_cases()
S2 = bc.s2_cases()
CONV1 = bc.conv1_cases()
CONV_OUT = bc.conv_out_cases()
FAMILY_MODES = [(n, t) for n in bc.FAMILIES for t in (True, False)]


def _ids(cases):
    return [bc.case_id(c) for c in cases]


# ------------------------------------------------------------------------------------------------ no GPU: the tables hold
def test_block_rows_are_the_21_distinct_configurations():
    from cabinet_amd.models.constants import MOBILENETV3_CFGS

    rows = bc.block_rows()
    assert len(rows) == 21 and len(set(rows)) == 21
    assert sum(len(v) for v in MOBILENETV3_CFGS.values()) == 26
    assert len(PART1) == (21 + 3) * 2
    for row in list(bc.K10_BLOCKS) + list(bc.FAMILIES.values()):
        assert row in rows, row
    fam = bc.FAMILIES  # one block of each family: no expansion; expansion without SE; SE + ReLU; SE + HardSwish with the shortcut
    assert fam["no-expansion"][0] == fam["no-expansion"][1]
    assert fam["expansion"][0] != fam["expansion"][1] and not fam["expansion"][5]
    assert fam["se-relu"][5:] == (True, False)
    r = fam["se-hardswish-shortcut"]
    assert r[5:] == (True, True) and r[4] == 1 and r[0] == r[2]


@pytest.mark.parametrize("c", bc.all_gradient_cases(), ids=_ids(bc.all_gradient_cases()))
def test_every_case_is_clear_of_kinks(c):
    """No fp64 pre-activation of the case within m = max(10 e32, 2e-5) of a kink of its activation (recomputed, not recorded)."""
    mod, x, _ = bc.build(c)
    rep = bc.kink_report(mod, x, c["training"])
    print(f"KINK {bc.case_id(c)} e32 {rep['e32']:.2e} margin {rep['margin']:.2e} nearest {rep['worst']:.2e}")
    assert rep["margin"] >= bc.MIN_MARGIN and rep["margin"] < 1e-3, rep["margin"]
    assert not any(rep["near"].values()), f"{bc.case_id(c)}: units within {rep['margin']:.2e} of a kink: {rep['near']}"
    if c["bn"] == "pm3":  # the mask is not trivial: channels passed and channels zeroed (behind a depthwise convolution the
        for name, p in rep["pre64"].items():  # zero-padded border of a channel can sit 8 sigma out and cross over: < 5 % of it)
            if p.dim() == 4:
                passed = (p > 0).flatten(2).double().mean(2)
                assert bool(((passed < 0.05) | (passed > 0.95)).all()) and 0.25 < float(passed.mean()) < 0.75, name


def test_k15_shapes_sit_either_side_of_their_thresholds():
    """The weight-gradient routes of part 2b, restated: 64 -> 64 native from 256 workgroups of >= 4 rows, 3 -> 16 from 1024."""
    from cabinet_amd.functional import (_CW_MIN_ROWS, _CW_MIN_WORKGROUPS, _conv3x3s2_native_wgrad, _conv3x3s2_native_wgrad64,
                                        _conv3x3s2_wgrad64_plan)

    assert (_CW_MIN_WORKGROUPS, _CW_MIN_ROWS) == (256, 4)
    plans = {s: _conv3x3s2_wgrad64_plan(s[0], s[2], s[3]) for s, _ in bc.CONV23_SHAPES}
    assert plans[(4, 64, 255, 126)] == (256, 4) and plans[(4, 64, 248, 128)] == (248, 4) and plans[(2, 64, 33, 21)] == (10, 4)
    for (B, _, H, W), native in bc.CONV23_SHAPES:
        assert _conv3x3s2_native_wgrad64(B, H, W) is native
        assert not _conv3x3s2_native_wgrad(64, B, H)
    groups = {s: s[0] * (((s[2] - 1) // 2 + 1 + 3) // 4) for s, _ in bc.FIRST_SHAPES}
    assert groups == {(8, 3, 1023, 34): 1024, (8, 3, 1015, 34): 1016}
    for (B, Ci, H, W), native in bc.FIRST_SHAPES:
        assert _conv3x3s2_native_wgrad(Ci, B, H) is native
    for c in PART1:
        if c["spec"][0] == "conv_3x3_bn":
            assert not _conv3x3s2_native_wgrad(3, c["shape"][0], c["shape"][2])


def test_claimed_routes_cover_the_state_machine():
    """The union of the routes the tables claim (and the GPU tests assert case by case) holds every route of
    `_FusedSequential.forward`, `bn_act` with and without the residual, and the stock fall-through; the written-out K10 table
    agrees with the restated rule."""
    for c in K10:
        assert c["routes"] == bc.claimed_routes(c["spec"][1:], c["shape"][2:]), bc.case_id(c)
        assert ("pwconv" in c["routes"]) == (c["shape"][2] == 256 and c["spec"][1:] != (16, 16, 16, 3, 2, True, False))
    union = set()
    for c in PART1 + K10:
        union.update(bc.case_routes(c))
    assert union >= set(bc.ROUTES), set(bc.ROUTES) - union
    frozen = set()
    for n in bc.FAMILIES:
        frozen.update(bc.case_routes(bc.family_case(n), trainable=False))
    assert "stock" in frozen and "pwconv_wide" not in frozen
    assert bc.claimed_routes((24, 72, 40, 5, 2, True, False), (256, 257)) == ("pwconv", "bn_act_dwconv", "se_tail", "pwconv_wide", "bn_act")


# ------------------------------------------------------------------------------------------------ device side
@contextlib.contextmanager
def _routes(mod):
    """Records the sequence of routes `mod` takes: the names `_FusedSequential.forward` imports from cabinet_amd.functional (and
    cabinet.py holds), the `_Conv3x3S2` / `_StemConvBnRelu` entry points, the K15 weight-gradient rules as the backward asks them,
    and "stock" / "stock:<Class>" for every direct layer of a `_FusedSequential` / `ConvBNReLU` that is called as a module."""
    import cabinet_amd.functional as fn
    import cabinet_amd.models.cabinet as cab
    from cabinet_amd.models.mobilenetv3 import _FusedSequential

    log, undo, hooks = [], [], []

    def patch(obj, name, new):
        own = name in vars(obj)
        old = getattr(obj, name)
        setattr(obj, name, new)
        undo.append((lambda: setattr(obj, name, old)) if own else (lambda: delattr(obj, name)))
        return old

    def named(name):
        old = getattr(fn, name)

        def wrapper(*a, **k):
            residual = k.get("residual", a[3] if len(a) > 3 else None)
            log.append("bn_act+res" if name == "bn_act" and residual is not None else name)
            return old(*a, **k)

        patch(fn, name, wrapper)
        if hasattr(cab, name):
            patch(cab, name, wrapper)

    def entry(cls, name):
        old = cls.apply

        def apply(*a):
            log.append(name)
            return old(*a)

        patch(cls, "apply", staticmethod(apply))

    def rule(name):
        old = getattr(fn, name)

        def wrapper(*a):
            native = old(*a)  # `_Conv3x3S2.backward` asks the one rule of the layer's form, once
            log.append("wgrad:native" if native else "wgrad:stock")
            return native

        patch(fn, name, wrapper)

    try:
        for name in ("bn_act", "bn_act_dwconv", "dwconv", "gate_act", "pwconv", "pwconv_wide", "se_tail", "stem_conv", "conv3x3"):
            named(name)
        entry(fn._Conv3x3S2, "conv3x3s2")
        entry(fn._StemConvBnRelu, "stem_conv_bn_relu")
        rule("_conv3x3s2_native_wgrad64")
        rule("_conv3x3s2_native_wgrad")
        for box in mod.modules():
            if isinstance(box, (_FusedSequential, cab.ConvBNReLU)):
                for layer in box.children():
                    if isinstance(layer, nn.Identity):
                        continue
                    tag = "stock" if isinstance(layer, nn.Conv2d) else f"stock:{type(layer).__name__}"
                    mark = []
                    hooks.append(layer.register_forward_pre_hook(lambda _m, _a, mark=mark: mark.append(len(log))))
                    hooks.append(layer.register_forward_hook(
                        lambda _m, _a, _o, mark=mark, tag=tag: log.append(tag) if mark.pop() == len(log) else None))
        yield log
    finally:
        for h in hooks:
            h.remove()
        for u in reversed(undo):
            u()


def _device_run(c, x=None, grad=True, x_grad=True, freeze=False, backward=True):
    """One forward (+ backward) of a fresh device copy of the case's module -> dict(y, dx, grads, buffers, routes)."""
    mod0, x0, g = bc.build(c)
    mod = copy.deepcopy(mod0).cuda()
    if freeze:
        mod.requires_grad_(False)
    xd = (x0.cuda() if x is None else x).detach().requires_grad_(x_grad and grad)
    with _routes(mod) as log, torch.set_grad_enabled(grad):
        y = mod(xd)
        if grad and backward:
            y.backward(g.cuda())
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xd.grad, "grads": {k: p.grad for k, p in mod.named_parameters()},
            "buffers": {k: b.detach().clone() for k, b in mod.named_buffers()}, "routes": tuple(log)}


def _flat(out):
    return [out["y"]] + ([out["dx"]] if out["dx"] is not None else []) + [g for g in out["grads"].values() if g is not None] + \
        list(out["buffers"].values())


def _compare(fails, tag, out, ref, grads=True, dx=True, buffers=True, bias_floor=False):
    """The criteria of part 1 against the fp64 reference; prints the worst distance per tensor kind.  `bias_floor`: part 2a only."""
    worst = {"y": bc.rel(out["y"], ref["y"])}
    _cmp(fails, tag, "y", out["y"], ref["y"], maxnorm=True, atol=0.0)
    if dx:
        _cmp(fails, tag, "dx", out["dx"], ref["dx"], maxnorm=True, atol=0.0)
        worst["dx"] = bc.rel(out["dx"], ref["dx"]) if out["dx"] is not None else float("nan")
    if grads:
        assert set(out["grads"]) == set(ref["grads"])
        for k, q in ref["grads"].items():
            # A BatchNorm's bias gradient is sum_p du, and in front of `[SE,] 1x1 conv, training-mode BatchNorm` that sum CANCELS:
            # the closing BatchNorm's dz sums to zero per channel, the 1x1 convolution is linear, so for a channel the ReLU passes
            # whole (part 2a's construction) the true value is 0 and the fp64 run itself holds rounding noise (1e-11 beside a
            # weight gradient of 1e3).  A relative rule alone would compare noise with noise; the floor is one fp32 ulp (2^-23) of
            # sum_p |du|, the error of a sum whose every partial is rounded once -- per tensor, in the same norm.  Part 2a alone:
            # everywhere else the rule is the plain relative one, and it is part 1 that tests these gradients.
            floor = 2.0 ** -23 * float(ref["sum_abs_du"][k].norm()) if bias_floor and k in ref["sum_abs_du"] else 0.0
            _cmp(fails, tag, f"d {k}", out["grads"][k], q, atol=floor / q.numel() ** 0.5)
            if out["grads"][k] is not None and float(q.norm()) > 1e-3 * floor * 2.0 ** 23:
                worst["dparam"] = max(worst.get("dparam", 0.0), bc.rel(out["grads"][k], q))
            elif out["grads"][k] is not None and floor > 0:
                worst["dbias/sum|du|"] = max(worst.get("dbias/sum|du|", 0.0), float((out["grads"][k].double().cpu() - q).norm())
                                             / max(float(ref["sum_abs_du"][k].norm()), 1e-300))
    if buffers:
        assert set(out["buffers"]) == set(ref["buffers"])
        for k, q in ref["buffers"].items():
            p = out["buffers"][k]
            if q.is_floating_point():
                _cmp(fails, tag, k, p, q, tol=TOL_STAT, atol=0.0)
                worst["buffer"] = max(worst.get("buffer", 0.0), bc.rel(p, q))
            elif int(p) != int(q):
                fails.append(f"{tag} {k}: {int(p)} vs {int(q)}")
    print(f"DIST {tag} " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def _check_case(c, routes):
    ref = bc.reference(c)
    runs = [_device_run(c) for _ in range(2)]
    fails = []
    _compare(fails, bc.case_id(c), runs[0], ref, bias_floor=c["bn"] == "pm3")
    assert runs[0]["routes"] == routes, f"routes taken {runs[0]['routes']}, the table claims {routes}"
    assert all(g is not None for g in runs[0]["grads"].values())
    assert _all_equal(_flat(runs[0]), _flat(runs[1])), "two device runs differ"
    _report(fails, 1, 1)


# ------------------------------------------------------------------------------------------------ 1. every block configuration
@gpu
@pytest.mark.parametrize("c", PART1, ids=_ids(PART1))
def test_block_forward_backward_vs_fp64(c):
    """Part 1: the module in training mode against its fp64 CPU copy, and the routes it took against the table."""
    _check_case(c, bc.case_routes(c))


# ------------------------------------------------------------------------------------------------ 2a. K10 inside a block
@gpu
@pytest.mark.parametrize("c", K10, ids=_ids(K10))
def test_k10_block_either_side_of_its_plane_threshold(c):
    """Six ReLU blocks at 256 x 257 (P = 65792: the thin 1x1 convolutions in front of the stride run K10) and 255 x 257 (65535: K14's
    weight gradient instead), cleared of kinks by construction."""
    _check_case(c, c["routes"])


# ------------------------------------------------------------------------------------------------ 2b. spatial branch, first layer
@gpu
@pytest.mark.parametrize("c", CONV1, ids=_ids(CONV1))
def test_stem_module_as_one_node_and_as_two(c):
    """`sb.conv1` on an image without gradient (`stem_conv_bn_relu`, one node) and on the same image with `requires_grad_()`
    (`stem_conv` + `bn_act`, dx from ATen): both right, parameter gradients and buffers of the two bit-equal."""
    ref = bc.reference(c)
    one, two = _device_run(c, x_grad=False), _device_run(c, x_grad=True)
    fails = []
    _compare(fails, bc.case_id(c) + " one node", one, ref, dx=False)
    _compare(fails, bc.case_id(c) + " two nodes", two, ref)
    assert one["routes"] == ("stem_conv_bn_relu",) and two["routes"] == ("stem_conv", "bn_act")
    assert one["dx"] is None and torch.equal(one["y"], two["y"])
    assert _all_equal(list(one["grads"].values()), list(two["grads"].values())), "parameter gradients of the two forms differ"
    assert _all_equal(list(one["buffers"].values()), list(two["buffers"].values()))
    again = _device_run(c, x_grad=False)
    assert _all_equal(_flat(one), _flat(again))
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("c", S2 + CONV_OUT, ids=_ids(S2 + CONV_OUT))
def test_spatial_module_vs_fp64(c):
    """`sb.conv2` / `sb.conv3` (K15: native weight gradient at 256 workgroups, stock at 248 and on a small plane), the backbone's
    first layer (native at 1024 workgroups, stock at 1016) and `sb.conv_out` (K14), each module alone."""
    _check_case(c, c["routes"])


# ------------------------------------------------------------------------------------------------ 2c. conditions that switch routes
@gpu
@pytest.mark.parametrize("name", list(bc.FAMILIES))
def test_frozen_parameters(name):
    """Every parameter frozen, x requiring a gradient: dx against fp64, no parameter gets a `.grad`, the running buffers still move;
    the 1x1 convolutions fall through to the stock operator (K14 is a weight gradient)."""
    c = bc.family_case(name)
    ref = bc.reference(c)
    runs = [_device_run(c, freeze=True) for _ in range(2)]
    fails = []
    _compare(fails, bc.case_id(c) + " frozen", runs[0], ref, grads=False)
    assert all(g is None for g in runs[0]["grads"].values())
    assert runs[0]["routes"] == bc.case_routes(c, trainable=False), runs[0]["routes"]
    mod0 = bc.build(c)[0]
    assert not any(torch.equal(runs[0]["buffers"][k].cpu(), b) for k, b in mod0.named_buffers())
    assert _all_equal(_flat(runs[0]), _flat(runs[1]))
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("name", list(bc.FAMILIES))
def test_eval_mode_in_a_recording_forward(name):
    """`eval()` with autograd recording: the running statistics are used, the buffers stay bit-unchanged, output, dx and every
    parameter gradient against the fp64 copy in eval mode (the seed clears both modes)."""
    c = bc.family_case(name, training=False)
    ref = bc.reference(c)
    runs = [_device_run(c) for _ in range(2)]
    fails = []
    _compare(fails, bc.case_id(c), runs[0], ref)
    assert runs[0]["routes"] == bc.case_routes(c), runs[0]["routes"]
    for k, b in bc.build(c)[0].named_buffers():
        assert torch.equal(runs[0]["buffers"][k].cpu(), b), f"{k} moved in eval mode"
    assert _all_equal(_flat(runs[0]), _flat(runs[1]))
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("name,training", FAMILY_MODES)
def test_no_grad_forward(name, training):
    """`torch.no_grad()` in both modes: output and buffers against fp64; no K14 / K15 route (they exist for their gradients)."""
    c = bc.family_case(name, training=training)
    ref = bc.reference(c)
    runs = [_device_run(c, grad=False) for _ in range(2)]
    fails = []
    _compare(fails, bc.case_id(c) + " no_grad", runs[0], ref, grads=False, dx=False)
    assert runs[0]["routes"] == bc.case_routes(c, grad=False), runs[0]["routes"]
    assert not runs[0]["y"].requires_grad
    if not training:
        for k, b in bc.build(c)[0].named_buffers():
            assert torch.equal(runs[0]["buffers"][k].cpu(), b), f"{k} moved in eval mode"
    assert _all_equal(_flat(runs[0]), _flat(runs[1]))
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("name", list(bc.FAMILIES))
def test_block_accepts_any_input_layout(name):
    """A channels_last x and an x that is a view 4 bytes into its storage: bit for bit the dense call, forward and backward."""
    c = bc.family_case(name)
    x = bc.build(c)[1].cuda()
    x_cl = x.contiguous(memory_format=torch.channels_last)
    x_off = torch.empty(x.numel() + 1, device="cuda")[1:].view(x.shape).copy_(x)
    assert not x_cl.is_contiguous() and x_off.is_contiguous() and x_off.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    base = _device_run(c, x=x)
    for what, xv in (("channels_last", x_cl), ("4 bytes into its storage", x_off)):
        got = _device_run(c, x=xv)
        assert got["routes"] == base["routes"]
        assert _all_equal(_flat(got), _flat(base)), f"{name}: an x that is {what} differs from the dense call"


# ------------------------------------------------------------------------------------------------ 3. the whole chain, forward only
@functools.lru_cache(maxsize=None)
def _chain_module(name):
    return bc.chain_module(name)


def _chain_bound(key, d32):
    return min(max(bc.CHAIN_FACTOR.get(key, 10) * d32, bc.CHAIN_FLOOR), bc.CHAIN_CEIL)


@gpu
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("image", bc.CHAIN_IMAGES, ids=["x".join(map(str, s)) for s in bc.CHAIN_IMAGES])
@pytest.mark.parametrize("name", bc.CHAIN_MODULES)
def test_whole_chain_forward_vs_fp64(name, image, training):
    """Part 3: how one layer hands its plane and statistics to the next.  Output and every running mean / variance within
    max(10 d32, 1e-5) <= 1e-3 of the fp64 CPU copy (relative, per tensor), d32 the fp32 CPU copy's distance on the same case."""
    mod = _chain_module(name)
    x = torch.randn(*image, generator=torch.Generator().manual_seed(sum(image)))
    y64, b64 = bc.chain_run(mod, x, training, torch.float64)
    y32, b32 = bc.chain_run(mod, x, training, torch.float32)
    runs = [bc.chain_run(mod, x, training, None, "cuda") for _ in range(2)]
    torch.cuda.synchronize()
    yd, bd = runs[0]
    tag = f"{name} {'x'.join(map(str, image))} {'train' if training else 'eval'}"
    fails = []
    stats = [k for k, b in b64.items() if b.is_floating_point()]
    assert len(stats) == 2 * sum(isinstance(m, nn.BatchNorm2d) for m in mod.modules()) and set(bd) == set(b64)
    d32 = {"y": bc.rel(y32, y64), "buffer": max(bc.rel(b32[k], b64[k]) for k in stats)}
    dev = {"y": bc.rel(yd, y64), "buffer": max(bc.rel(bd[k], b64[k]) for k in stats)}
    bound = {k: _chain_bound((name, image, training, k), d32[k]) for k in d32}
    print(f"CHAIN {tag} y dev {dev['y']:.2e} d32 {d32['y']:.2e} bound {bound['y']:.2e} buffer dev {dev['buffer']:.2e} "
          f"d32 {d32['buffer']:.2e} bound {bound['buffer']:.2e}")
    assert tuple(yd.shape) == tuple(y64.shape) and bool(torch.isfinite(yd).all())
    if not dev["y"] <= bound["y"]:
        fails.append(f"{tag} y: {dev['y']:.2e} > {bound['y']:.2e} (d32 {d32['y']:.2e})")
    for k in stats:
        e = bc.rel(bd[k], b64[k])
        if not e <= bound["buffer"]:
            fails.append(f"{tag} {k}: {e:.2e} > {bound['buffer']:.2e}")
    for k, b in b64.items():
        if not b.is_floating_point() and int(bd[k]) != int(b):
            fails.append(f"{tag} {k}: {int(bd[k])} vs {int(b)}")
    if not training:
        fails += [f"{tag} {k}: moved in eval mode" for k, b in mod.named_buffers() if not torch.equal(bd[k].cpu(), b)]
    assert torch.equal(yd, runs[1][0]) and _all_equal(list(bd.values()), list(runs[1][1].values())), "two device runs differ"
    _report(fails, 1, 1)
