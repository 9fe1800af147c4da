"""Case tables, the fp64 CPU oracle and the kink predicate of tests/test_gpu_backbone_blocks.py: the code that COMPOSES the
backbone and spatial-branch kernels (`_FusedSequential.forward`, `ConvBNReLU.forward` / `_conv3x3_bn_relu`, `Conv2dS2`).  Imports
without a GPU.

The oracle: on a host tensor `_FusedSequential` and `ConvBNReLU` fall through to the plain `nn.Sequential` /
`relu(bn(conv(x)))`, so a deep copy of the module, `.double()`, on the CPU is a plain high-precision reference of the same
operation.

Kinks: the oracle may not sit on a derivative jump.  Per case the margin is m = max(10 e32, 2e-5): e32 is the largest
pre-activation distance between the fp32 CPU run and the fp64 CPU run of the same module (both are the reference), 2e-5 the
pre-activation error stated for K7 (`_clear_of_kinks` in test_gpu_backbone_edges.py).  No fp64 pre-activation of a ReLU (0), a
HardSwish (+-3), an SE ReLU (0) or an SE HardSigmoid (+-3) may lie within m of its kink.  A case gets there
 * by seed (`seed` of the row; the blocks of parts 1 and 2c; `search` keeps a seed only if it is clear of 3 m, since e32 -- an
   fp32 run's error -- moves with the CPU's summation order),
 * by construction (`bn="pm3"`: every BatchNorm in front of a ReLU has gamma = 0.4, beta = +-3 alternating per channel, so whole
   channels pass or are zeroed: the 65792-pixel planes of part 2a, where no seed can clear millions of ReLU units), or
 * by nudging x (`nudge=True`: the centre-tap input pixel of every unit within 4 m of a kink is moved, as `_clear_of_kinks` does
   for pointwise operators; the single-activation modules of part 2b).
`test_every_case_is_clear_of_kinks` (no GPU) recomputes the predicate for every row, so the table cannot rot.
"""
import copy
import functools

import torch
import torch.nn as nn

from test_gpu_backbone_edges import _set_bn

ROUTES = ("se_tail", "bn_act_dwconv", "bn_act", "bn_act+res", "gate_act", "pwconv", "dwconv", "pwconv_wide")
PLANES = [(13, 19), (20, 12)]  # odd and even in both directions: the stride-2 blocks end on ragged tiles
MIN_MARGIN = 2e-5
K10_MIN_P, K10_MAX_C = 65536, 96  # pwconv_supported's rule (cabinet_amd/functional.py), restated


def block_rows():
    """The distinct (inp, hidden, oup, k, s, SE, HS) of both backbones, in order of first appearance (MobileNetV3.__init__)."""
    from cabinet_amd.models.constants import MOBILENETV3_CFGS
    from cabinet_amd.models.mobilenetv3 import _make_divisible

    rows = []
    for mode in ("large", "small"):
        cin = _make_divisible(16, 8)
        for k, t, c, se, hs, s in MOBILENETV3_CFGS[mode]:
            cout, exp = _make_divisible(c, 8), _make_divisible(cin * t, 8)
            row = (cin, exp, cout, k, s, bool(se), bool(hs))
            if row not in rows:
                rows.append(row)
            cin = cout
    return rows


# ------------------------------------------------------------------------------------------------ the case tables
# spec: ("block", inp, hidden, oup, k, s, SE, HS) | ("conv_3x3_bn", 3, 16, 2) | ("conv_1x1_bn", ci, co) | ("cbr", ci, co, k, s, p)
def _case(spec, shape, seed, training=True, bn="random", se_scale=0.3, nudge=False, routes=None):
    return {"spec": spec, "shape": shape, "seed": seed, "training": training, "bn": bn, "se_scale": se_scale, "nudge": nudge,
            "routes": routes}


# part 1: seeds per (row, plane) for which the kink predicate holds (found by tests/backbone_block_cases.py's search())
BLOCK_SEEDS = {  # (spec, plane) -> seed, from search(); every row not listed is clear of 3 m with seed 0
    (('block', 16, 16, 16, 3, 1, False, False), (20, 12)): 1,
    (('block', 16, 64, 24, 3, 2, False, False), (13, 19)): 17,
    (('block', 16, 64, 24, 3, 2, False, False), (20, 12)): 4,
    (('block', 24, 72, 24, 3, 1, False, False), (13, 19)): 39,
    (('block', 24, 72, 24, 3, 1, False, False), (20, 12)): 22,
    (('block', 24, 72, 40, 5, 2, True, False), (13, 19)): 11,
    (('block', 24, 72, 40, 5, 2, True, False), (20, 12)): 13,
    (('block', 40, 120, 40, 5, 1, True, False), (13, 19)): 2808,  # clear of 2 m: no seed below 40000 is clear of 3 m
    (('block', 40, 120, 40, 5, 1, True, False), (20, 12)): 2411,
    (('block', 40, 240, 80, 3, 2, False, True), (13, 19)): 2,
    (('block', 80, 184, 80, 3, 1, False, True), (13, 19)): 2,
    (('block', 80, 184, 80, 3, 1, False, True), (20, 12)): 2,
    (('block', 80, 480, 112, 3, 1, True, True), (13, 19)): 1,
    (('block', 80, 480, 112, 3, 1, True, True), (20, 12)): 1,
    (('block', 112, 672, 112, 3, 1, True, True), (13, 19)): 3,
    (('block', 112, 672, 112, 3, 1, True, True), (20, 12)): 48,
    (('block', 112, 672, 160, 5, 2, True, True), (13, 19)): 17,
    (('block', 112, 672, 160, 5, 2, True, True), (20, 12)): 2,
    (('block', 160, 960, 160, 5, 1, True, True), (13, 19)): 307,
    (('block', 160, 960, 160, 5, 1, True, True), (20, 12)): 19,
    (('block', 16, 16, 16, 3, 2, True, False), (20, 12)): 1,
    (('block', 16, 72, 24, 3, 2, False, False), (13, 19)): 20,
    (('block', 16, 72, 24, 3, 2, False, False), (20, 12)): 5,
    (('block', 24, 88, 24, 3, 1, False, False), (13, 19)): 47,
    (('block', 24, 88, 24, 3, 1, False, False), (20, 12)): 5,
    (('block', 48, 288, 96, 5, 2, True, True), (20, 12)): 3,
    (('block', 96, 576, 96, 5, 1, True, True), (13, 19)): 11,
    (('block', 96, 576, 96, 5, 1, True, True), (20, 12)): 9,
    (('conv_1x1_bn', 160, 960), (13, 19)): 1,
    (('conv_1x1_bn', 160, 960), (20, 12)): 4,
    (('conv_1x1_bn', 96, 576), (13, 19)): 3,
    (('conv_1x1_bn', 96, 576), (20, 12)): 1,
}
EXTRA_SPECS = [("conv_3x3_bn", 3, 16, 2), ("conv_1x1_bn", 160, 960), ("conv_1x1_bn", 96, 576)]


def spec_id(spec):
    if spec[0] == "block":
        return "blk" + "-".join(str(int(v)) for v in spec[1:])
    return spec[0] + "-" + "-".join(str(v) for v in spec[1:])


def case_id(c):
    return f"{spec_id(c['spec'])}@" + "x".join(map(str, c["shape"])) + ("" if c["training"] else "-eval")


def part1_cases():
    out = []
    for spec in [("block",) + r for r in block_rows()] + EXTRA_SPECS:
        for hw in PLANES:
            out.append(_case(spec, (2, spec[1]) + hw, BLOCK_SEEDS.get((spec, hw), 0)))
    return out


# part 2a: K10 inside a block, both sides of P >= 65536; the route sequence each case must take, written out
K10_PLANES = [(256, 257), (255, 257)]  # P = 65792 (K10) and 65535 (K14 instead)
K10_BLOCKS = {
    # row -> routes at 256 x 257; at 255 x 257 every "pwconv" is "pwconv_wide"
    (16, 16, 16, 3, 1, False, False): ("dwconv", "bn_act", "pwconv", "bn_act+res"),
    (16, 64, 24, 3, 2, False, False): ("pwconv", "bn_act_dwconv", "bn_act", "pwconv_wide", "bn_act"),
    (24, 72, 24, 3, 1, False, False): ("pwconv", "bn_act_dwconv", "bn_act", "pwconv", "bn_act+res"),
    (24, 72, 40, 5, 2, True, False): ("pwconv", "bn_act_dwconv", "se_tail", "pwconv_wide", "bn_act"),
    (16, 16, 16, 3, 2, True, False): ("dwconv", "bn_act", "gate_act", "pwconv_wide", "bn_act"),  # its 1x1 sits behind the stride
    (16, 72, 24, 3, 2, False, False): ("pwconv", "bn_act_dwconv", "bn_act", "pwconv_wide", "bn_act"),
}
K10_SEEDS = {((24, 72, 40, 5, 2, True, False), (256, 257)): 1}  # the SE MLP's two activations, by seed; the others: 0


def k10_cases():
    out = []
    for row, routes in K10_BLOCKS.items():
        for hw in K10_PLANES:
            r = routes if hw[0] * hw[1] >= K10_MIN_P else tuple("pwconv_wide" if v == "pwconv" else v for v in routes)
            # SE weights of order 0.05 here: behind beta = +-3 the pooled values are +-3, and 0.3 would saturate every gate
            out.append(_case(("block",) + row, (1, row[0]) + hw, K10_SEEDS.get((row, hw), 0), bn="pm3", se_scale=0.05, routes=r))
    return out


# part 2b: the spatial branch's modules and the backbone's first layer, each alone (one activation per module)
CONV1 = ("cbr", 3, 64, 7, 2, 3)
CONV23 = ("cbr", 64, 64, 3, 2, 1)
CONV_OUT = ("cbr", 64, 128, 1, 1, 0)
FIRST = ("conv_3x3_bn", 3, 16, 2)
CONV1_SHAPES = [(2, 3, 97, 131), (2, 3, 130, 66)]
# (shape, native weight gradient?): K15 64 -> 64 is native from 256 workgroups of >= 4 rows, 3 -> 16 from 1024 workgroups
CONV23_SHAPES = [((4, 64, 255, 126), True), ((4, 64, 248, 128), False), ((2, 64, 33, 21), False)]
FIRST_SHAPES = [((8, 3, 1023, 34), True), ((8, 3, 1015, 34), False)]
CONV_OUT_SHAPE = (2, 64, 13, 17)


def conv1_cases():
    return [_case(CONV1, s, 11, nudge=True) for s in CONV1_SHAPES]


def s2_cases():
    out = [_case(CONV23, s, 12, nudge=True, routes=("conv3x3s2", "bn_act", "wgrad:native" if nat else "wgrad:stock"))
           for s, nat in CONV23_SHAPES]
    out += [_case(FIRST, s, 13, nudge=True, routes=("conv3x3s2", "bn_act", "wgrad:native" if nat else "wgrad:stock"))
            for s, nat in FIRST_SHAPES]
    return out


def conv_out_cases():
    return [_case(CONV_OUT, CONV_OUT_SHAPE, 14, nudge=True, routes=("pwconv_wide", "bn_act"))]


# part 2c: the conditions that switch routes, one block of each family; seeds clear in training AND in eval mode
FAMILIES = {
    "no-expansion": (16, 16, 16, 3, 1, False, False),
    "expansion": (16, 64, 24, 3, 2, False, False),
    "se-relu": (24, 72, 40, 5, 2, True, False),
    "se-hardswish-shortcut": (40, 240, 40, 5, 1, True, True),
}
FAMILY_SEEDS = {"no-expansion": 4, "expansion": 77, "se-relu": 5, "se-hardswish-shortcut": 0}


FAMILY_PLANES = {"se-relu": (9, 11)}  # 3 m in both modes at once: no seed below 2000 clears its 72 x 494 ReLU units on 13 x 19


def family_case(name, training=True):
    row = FAMILIES[name]
    return _case(("block",) + row, (2, row[0]) + FAMILY_PLANES.get(name, PLANES[0]), FAMILY_SEEDS.get(name, 0), training=training)


def all_gradient_cases():
    """Every case whose gradients are compared with fp64, i.e. that must be clear of kinks."""
    fam = [family_case(n, t) for n in FAMILIES for t in (True, False)]
    return part1_cases() + k10_cases() + conv1_cases() + s2_cases() + conv_out_cases() + fam


def claimed_routes(row, hw, grad=True, trainable=True):
    """The route sequence of `_FusedSequential.forward` for a block row, restated from the row alone (not from the module's layer
    list): `grad` = the forward records a graph, `trainable` = the convolution weights require a gradient."""
    inp, hidden, oup, k, s, se, hs = row
    P = hw[0] * hw[1]
    Po = ((hw[0] - 1) // s + 1) * ((hw[1] - 1) // s + 1)

    def pw(ci, co, p):
        if p >= K10_MIN_P and ci <= K10_MAX_C and co <= K10_MAX_C:
            return "pwconv"
        return "pwconv_wide" if grad and trainable else "stock"

    if inp == hidden:
        r = ["dwconv", "bn_act"] + (["gate_act"] if se else [])
    else:
        r = [pw(inp, hidden, P), "bn_act_dwconv", "se_tail" if se else "bn_act"]
    return tuple(r + [pw(hidden, oup, Po), "bn_act+res" if s == 1 and inp == oup else "bn_act"])


def case_routes(c, grad=True, trainable=True):
    """What the table claims for a case: the written-out tuple where the row has one, else the restated rule."""
    if c["routes"] is not None:
        return c["routes"]
    spec = c["spec"]
    if spec[0] == "block":
        return claimed_routes(spec[1:], c["shape"][2:], grad, trainable)
    if spec[0] == "conv_1x1_bn":
        return ("pwconv_wide" if grad and trainable else "stock", "bn_act")
    if spec[0] == "conv_3x3_bn":
        return ("conv3x3s2", "bn_act", "wgrad:stock") if grad and trainable else ("stock", "bn_act")
    raise KeyError(spec)


# part 3: the whole chain, forward only
CHAIN_MODULES = ("mobilenetv3_large", "mobilenetv3_small", "SpatialBranch")
CHAIN_IMAGES = [(2, 3, 97, 131), (2, 3, 130, 66), (3, 3, 65, 225)]
CHAIN_FACTOR = {}  # (module, image, training, kind) -> factor on d32 where a correct kernel needs more than 10; none so far
CHAIN_FLOOR, CHAIN_CEIL = 1e-5, 1e-3


# ------------------------------------------------------------------------------------------------ modules and inputs
def _new_module(spec):
    from cabinet_amd.models.cabinet import ConvBNReLU
    from cabinet_amd.models.mobilenetv3 import InvertedResidual, conv_1x1_bn, conv_3x3_bn

    kind = spec[0]
    if kind == "block":
        return InvertedResidual(*spec[1:])
    return {"conv_3x3_bn": conv_3x3_bn, "conv_1x1_bn": conv_1x1_bn, "cbr": ConvBNReLU}[kind](*spec[1:])


def _owned_hsig(mod):
    from cabinet_amd.models.mobilenetv3 import HardSwish

    return {id(m.sigmoid) for m in mod.modules() if isinstance(m, HardSwish)}


def activations(mod):
    """[(name, module, kinks)] of every activation with a derivative jump; HardSwish's inner HardSigmoid is HardSwish's own."""
    from cabinet_amd.models.mobilenetv3 import HardSigmoid, HardSwish

    owned, out = _owned_hsig(mod), []
    for name, m in mod.named_modules():
        if isinstance(m, nn.ReLU):
            out.append((name, m, (0.0,)))
        elif isinstance(m, HardSwish) or (isinstance(m, HardSigmoid) and id(m) not in owned):
            out.append((name, m, (-3.0, 3.0)))
    return out


def prepare(mod, gen, bn="random", se_scale=0.3):
    """BatchNorm affine and running buffers from `_set_bn`; SE linear layers of order `se_scale` (not the 0.01 initialisation), so
    that the gate moves.  bn="pm3": the BatchNorms in front of a ReLU get gamma = 0.4, beta = +-3 alternating per channel."""
    from cabinet_amd.models.mobilenetv3 import SELayer

    for m in mod.modules():
        if isinstance(m, nn.BatchNorm2d):
            _set_bn(m, gen)
        elif isinstance(m, nn.Linear):
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * se_scale)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.3)
    if bn == "pm3":  # blocks only: the layer list of the block, placeholders dropped
        layers = [m for m in mod.conv if not isinstance(m, nn.Identity)] + [None, None]
        for m, n1, n2 in zip(layers, layers[1:], layers[2:]):
            if isinstance(m, nn.BatchNorm2d) and (isinstance(n1, nn.ReLU) or (isinstance(n1, SELayer) and isinstance(n2, nn.ReLU))):
                with torch.no_grad():
                    m.weight.fill_(0.4)
                    m.bias.copy_(3.0 - 6.0 * (torch.arange(m.num_features) % 2))
    return mod


def forward_with_preacts(mod, x):
    """mod(x) on the CPU -> (y, {activation name: its input, detached})."""
    pre, hooks = {}, []
    for name, m, _ in activations(mod):
        hooks.append(m.register_forward_pre_hook(lambda _m, args, name=name: pre.__setitem__(name, args[0].detach().clone())))
    try:
        y = mod(x)
    finally:
        for h in hooks:
            h.remove()
    return y, pre


def kink_report(mod, x, training, slack=1.0):
    """-> dict(e32, margin, near, worst): e32 = max pre-activation distance of the fp32 and fp64 CPU runs, margin = max(10 e32,
    2e-5), near = {activation: number of fp64 pre-activations within the margin of a kink}, pre64 = the fp64 pre-activations."""
    m64, m32 = copy.deepcopy(mod).double().train(training), copy.deepcopy(mod).float().train(training)
    with torch.no_grad():
        _, p64 = forward_with_preacts(m64, x.double())
        _, p32 = forward_with_preacts(m32, x.float())
    e32 = max(float((p32[k].double() - p64[k]).abs().max()) for k in p64)
    margin = max(10 * e32, MIN_MARGIN)
    near, worst = {}, float("inf")
    for name, _, kinks in activations(m64):
        d = torch.stack([(p64[name] - k).abs() for k in kinks]).amin(0)
        near[name] = int((d < margin).sum())
        worst = min(worst, float(d.min()))
    return {"e32": e32, "margin": margin, "near": near, "worst": worst, "pre64": p64, "clear": worst >= slack * margin}


def _nudge(mod, x, training, rounds=60):
    """Moves x (training mode) until no pre-activation of the module's single activation lies within 4 m of a kink.  For every
    such unit (b, co, oy, ox) the input pixel under the kernel's centre tap -- (s oy, s ox) for a k x k / s convolution with
    padding k // 2 --, in the input channel with the largest centre weight for co, moves by what carries the unit 16 m further
    from the kink.  Small steps on purpose: every moved pixel shifts the batch mean of all output channels, and a large shift
    would carry as many new units into the band as the step carries out of it."""
    conv = next(m for m in mod.modules() if isinstance(m, nn.Conv2d))
    bn = next(m for m in mod.modules() if isinstance(m, nn.BatchNorm2d))
    s, kc = conv.stride[0], conv.kernel_size[0] // 2
    wc = conv.weight.detach().double()[:, :, kc, kc]
    ci_of = wc.abs().argmax(1)
    w_of = wc.gather(1, ci_of[:, None])[:, 0]
    (name, _, kinks), = activations(mod)
    m64 = copy.deepcopy(mod).double().train(training)
    state = copy.deepcopy(m64.state_dict())
    want = 4 * kink_report(mod, x, training)["margin"]  # 4 m, not m: e32 moves with the CPU's summation order
    with torch.no_grad():
        z = torch.nn.functional.conv2d(x.double(), conv.weight.detach().double(), None, conv.stride, conv.padding)
        slope = bn.weight.detach().double() / (z.var((0, 2, 3), unbiased=False) + bn.eps).sqrt() * w_of  # d u / d pixel
    del z
    for _ in range(rounds):
        m64.load_state_dict(state)  # the running buffers move with every training-mode call
        with torch.no_grad():
            _, p = forward_with_preacts(m64, x.double())
        u = p[name]
        dist = torch.stack([u - k for k in kinks])
        dist = dist.gather(0, dist.abs().argmin(0, keepdim=True))[0]  # signed distance to the nearest kink
        near = dist.abs() < want
        if not bool(near.any()):
            return x
        b, co, oy, ox = near.nonzero(as_tuple=True)
        step = torch.where(dist[near] >= 0, 1.0, -1.0) * 4 * want / slope[co]
        x.index_put_((b, ci_of[co], oy * s, ox * s), step.float(), accumulate=True)
    raise AssertionError("the input could not be moved clear of the activation's kinks")


@functools.lru_cache(maxsize=None)
def _built(key):
    spec, shape, seed, training, bn, se_scale, nudge = key
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    mod = prepare(_new_module(spec), gen, bn, se_scale).train(training)
    x = torch.randn(*shape, generator=gen)
    if nudge:
        x = _nudge(mod, x, training)
    with torch.no_grad():
        y = copy.deepcopy(mod)(x.clone())
    g = torch.randn(y.shape, generator=gen)
    return mod, x, g


def build(c):
    """-> (module (fp32, CPU; deep-copy it before use), x, upstream gradient g), deterministic in the case."""
    return _built((c["spec"], c["shape"], c["seed"], c["training"], c["bn"], c["se_scale"], c["nudge"]))


@functools.lru_cache(maxsize=8)
def _reference(key):
    mod, x, g = _built(key)
    m64 = copy.deepcopy(mod).double()
    x64 = x.double().requires_grad_(True)
    sum_abs_du, hooks = {}, []
    for name, m in m64.named_modules():
        if isinstance(m, nn.BatchNorm2d):  # a hook on the BatchNorm's output, set before an in-place ReLU rewrites it: du
            hooks.append(m.register_forward_hook(lambda _m, _a, out, key=name + ".bias": out.register_hook(
                lambda du: sum_abs_du.__setitem__(key, du.abs().sum((0, 2, 3)))) and None))
    y = m64(x64)
    y.backward(g.double())
    for h in hooks:
        h.remove()
    return {"y": y.detach(), "dx": x64.grad, "grads": {k: p.grad for k, p in m64.named_parameters()},
            "buffers": {k: b.clone() for k, b in m64.named_buffers()}, "sum_abs_du": sum_abs_du}


def reference(c):
    """The fp64 CPU copy's forward + backward: y, dx, parameter gradients and buffers after the call; `sum_abs_du`: per BatchNorm
    bias, sum_p |du| per channel (du the gradient at the BatchNorm's output), the scale of the terms its gradient sum_p du adds
    up.  Shared, never modified."""
    return _reference((c["spec"], c["shape"], c["seed"], c["training"], c["bn"], c["se_scale"], c["nudge"]))


def search(specs_shapes, seeds=range(30000), both_modes=False, slack=3.0, **kw):
    """Table maintenance: the first seed per (spec, shape) for which the kink predicate holds (in training and eval mode if
    `both_modes`) with `slack` times the margin.  The rule is 3 m: e32 is an fp32 run's error and moves with the CPU's summation
    order, and the predicate the tests recompute (1 m) has to hold on any host."""
    found = {}
    for spec, shape in specs_shapes:
        for seed in seeds:
            ok = True
            for training in ((True, False) if both_modes else (True,)):
                c = _case(spec, shape, seed, training=training, **kw)
                mod, x, _ = build(c)
                ok = ok and kink_report(mod, x, training, slack)["clear"]
            _built.cache_clear()
            if ok:
                found[(spec, shape)] = seed
                break
        else:
            raise AssertionError(f"no seed for {spec} {shape}")
    return found


# ------------------------------------------------------------------------------------------------ the whole chain (part 3)
def chain_module(name, seed=5):
    from cabinet_amd.models.cabinet import SpatialBranch
    from cabinet_amd.models.mobilenetv3 import mobilenetv3_large, mobilenetv3_small

    torch.manual_seed(seed)
    mod = {"mobilenetv3_large": mobilenetv3_large, "mobilenetv3_small": mobilenetv3_small, "SpatialBranch": SpatialBranch}[name]()
    return prepare(mod, torch.Generator().manual_seed(seed))  # `_set_bn` on every BatchNorm; SE gates that move


def chain_run(mod, x, training, dtype=None, device="cpu"):
    """A deep copy of `mod` in `dtype` on `device`, one forward without autograd -> (y, {buffer name: value after the call})."""
    m = copy.deepcopy(mod)
    m = (m.to(dtype) if dtype is not None else m).to(device).train(training)
    with torch.no_grad():
        y = m(x.to(device=device, dtype=dtype if dtype is not None else x.dtype))
    return y, dict(m.named_buffers())


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
