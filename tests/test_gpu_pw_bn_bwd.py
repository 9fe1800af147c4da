"""The fused backward of a thin 1x1 convolution and the BatchNorm behind it (csrc/pwconv_wide.hip "BN form"; entry points
cabinet_pw_bn_act_bwd and cabinet_pw_bn_dwconv_bwd) against the parent's chain -- cabinet_bn_act_bwd / cabinet_bn_dwconv_bwd, then
cabinet_pwconv_bwd on the stored dz -- and against fp64 formulas on the same inputs (tests/pw_bn_bwd_cases.py):

* dgamma, dbeta and the depthwise weight gradient equal the chain's (torch.equal); two runs of every case are bit-equal;
* with W = I, dx equals the dz the chain's dx pass writes: the loader's expression and its tail handling, bit for bit;
* dX and the convolution's dW are no further from fp64 than twice the chain (floor where the chain is exact: one fp32 rounding)
  and under 1e-3;
* through the modules, flag on and off: outputs and buffers exactly, gradients under the same bound, the same routes.

A shortcut does not reach the C call (its gradient is g itself, returned by the autograd node): the module tests cover it."""
import contextlib
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_block_cases as bc  # noqa: E402
import pw_bn_bwd_cases as pc  # noqa: E402

gpu = pytest.mark.gpu


def _check_pair(tag, fused, chain, ref, names):
    fails = []
    for name in names:
        if fused[name] is None:
            continue
        assert bool(torch.isfinite(fused[name]).all()), f"{tag} {name}: not finite (a NaN of the prefill was left or read)"
        d, d0 = pc.dist(fused[name], ref[name]), pc.dist(chain[name], ref[name])
        print(f"PWBN {tag} {name}: fused {d:.3e} chain {d0:.3e} from fp64")
        if d > pc.TOL:
            fails.append(f"{name}: {d:.3e} > {pc.TOL}")
        if d > pc.bound(d0):
            fails.append(f"{name}: {d:.3e} from fp64, the chain {d0:.3e}")
    assert not fails, f"{tag}: " + "; ".join(fails)


@gpu
@pytest.mark.parametrize("case", pc.ACT_CASES, ids=pc.key)
def test_closing_bn_form(case):
    B, Ci, Co, P, act, training, mis, want_dx, want_dw = case
    lib = pc.load_library()
    assert lib.cabinet_pw_bn_bwd_supported(Ci, Co, P) == 1
    cpu = pc.act_inputs(B, Ci, Co, P)
    dev = {k: pc.on_device(v, mis == 2 or (mis == 1 and k == "x")) for k, v in cpu.items()}
    runs = [pc.run_act_fused(lib, dev, B, Ci, Co, P, act, training, want_dx, want_dw, mis == 1, mis == 2) for _ in range(2)]
    chain = pc.run_act_chain(lib, dev, B, Ci, Co, P, act, training)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(a, b), "two runs differ"
    dx, dw, dgam, dbet = runs[0]
    assert (dx is None) == (not want_dx) and (dw is None) == (not want_dw)
    assert torch.equal(dgam, chain[2]) and torch.equal(dbet, chain[3]), "dgamma / dbeta are not the chain's bits"
    ref = pc.bn_pw_ref(cpu["g"], cpu["z"], cpu["x"], cpu["w"], cpu["gamma"], cpu["beta"], cpu["mean"], cpu["invstd"], act, training)
    assert pc.dist(dgam, ref["dgamma"]) <= pc.TOL and pc.dist(dbet, ref["dbeta"]) <= pc.TOL
    _check_pair(pc.key(case), {"dx": dx, "dw": dw}, {"dx": chain[0], "dw": chain[1]}, ref, ("dx", "dw"))


@gpu
@pytest.mark.parametrize("case", pc.IDENTITY_CASES, ids=pc.key)
def test_identity_weight_gives_the_chains_dz(case):
    """W = I: every dx element is one dz element plus exact zeros, so dx is the dz of bn_act_bwd_dx_kernel bit for bit -- the
    staged expression, its per-channel scalars, and zeros (not the dz of zero operands) past P and Co."""
    B, C, P, act, training = case
    lib = pc.load_library()
    cpu = pc.act_inputs(B, C, C, P, identity=True)
    dev = {k: pc.on_device(v) for k, v in cpu.items()}
    dx, dw, _, _ = pc.run_act_fused(lib, dev, B, C, C, P, act, training)
    chain = pc.run_act_chain(lib, dev, B, C, C, P, act, training)
    torch.cuda.synchronize()
    assert torch.equal(dx, chain[4]), f"dx differs from the chain's dz in {int((dx != chain[4]).sum())} elements"
    assert torch.equal(dw, chain[1]), "dW (same staged dz, same plan) differs from the chain's"


@gpu
@pytest.mark.parametrize("case", pc.DW_CASES, ids=pc.key)
def test_depthwise_form(case):
    B, Ci, C, H, W, K, stride, act, training = case
    lib = pc.load_library()
    cpu = pc.dw_inputs(B, Ci, C, H, W, K, stride)
    dev = {k: pc.on_device(v) for k, v in cpu.items()}
    runs = [pc.run_dw_fused(lib, dev, B, Ci, C, H, W, K, stride, act, training) for _ in range(2)]
    chain = pc.run_dw_chain(lib, dev, B, Ci, C, H, W, K, stride, act, training)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    dx, dw, dgam, dbet, dcw = runs[0]
    assert torch.equal(dgam, chain[2]) and torch.equal(dbet, chain[3]) and torch.equal(dcw, chain[4]), \
        "dgamma / dbeta / the depthwise dW are not the chain's bits"
    ref = pc.dw_ref(cpu, K, stride, act, training)
    assert pc.dist(dcw, ref["dcw"]) <= pc.TOL
    _check_pair(pc.key(case), {"dx": dx, "dw": dw}, {"dx": chain[0], "dw": chain[1]}, ref, ("dx", "dw"))


@gpu
def test_loaded_chip_digest():
    """The full grid with several chunks per workgroup (see pw_bn_bwd_cases.LOADED_CASE): two runs have one digest, and dx / dW keep
    the bound against the chain.  Store data taken straight from accumulator registers failed only under such load."""
    B, Ci, Co, P, act, training = pc.LOADED_CASE[:6]
    lib = pc.load_library()
    cpu = pc.act_inputs(B, Ci, Co, P)
    dev = {k: pc.on_device(v) for k, v in cpu.items()}
    runs = [pc.run_act_fused(lib, dev, B, Ci, Co, P, act, training) for _ in range(2)]
    chain = pc.run_act_chain(lib, dev, B, Ci, Co, P, act, training)
    torch.cuda.synchronize()
    assert pc.digest(runs[0][0]) == pc.digest(runs[1][0]) and pc.digest(runs[0][1]) == pc.digest(runs[1][1])
    ref = pc.bn_pw_ref(cpu["g"], cpu["z"], cpu["x"], cpu["w"], cpu["gamma"], cpu["beta"], cpu["mean"], cpu["invstd"], act, training)
    _check_pair("loaded", {"dx": runs[0][0], "dw": runs[0][1]}, {"dx": chain[0], "dw": chain[1]}, ref, ("dx", "dw"))
    worst = float((runs[0][0].double().cpu().flatten(1) - ref["dx"].flatten(1)).abs().max())
    assert worst <= 1e-4 * float(ref["dx"].abs().max()), f"a dx element is off by {worst:.3e}: a row stored from the wrong registers?"


@gpu
def test_captured_replay_equals_eager():
    """No allocation or synchronisation inside: the call captured in a graph and replayed twice gives the eager bits."""
    from cabinet_amd.functional import _ptr, _stream_handle

    B, Ci, Co, P, act, training = 2, 24, 72, 64 * 9 + 38, "hardswish", True
    lib = pc.load_library()
    dev = {k: pc.on_device(v) for k, v in pc.act_inputs(B, Ci, Co, P).items()}
    eager = pc.run_act_fused(lib, dev, B, Ci, Co, P, act, training)
    torch.cuda.synchronize()
    outs = [pc.nan_like(dev[k]) for k in ("x", "w", "gamma", "beta")]
    nbytes = lib.cabinet_pw_bn_act_bwd_workspace_bytes(B, Ci, Co, P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def step():
        rc = lib.cabinet_pw_bn_act_bwd(_ptr(dev["g"]), _ptr(dev["z"]), _ptr(dev["x"]), _ptr(dev["w"]), _ptr(dev["gamma"]),
                                       _ptr(dev["beta"]), _ptr(dev["mean"]), _ptr(dev["invstd"]), B, Ci, Co, P, pc.ACTS[act],
                                       int(training), *[_ptr(t) for t in outs], _ptr(ws), nbytes, _stream_handle(ws.device))
        assert rc == 0, lib.cabinet_last_error()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a, b), "the replay differs from the eager call"


@gpu
def test_unsupported_shapes_are_refused():
    lib = pc.load_library()
    assert lib.cabinet_pw_bn_bwd_supported(104, 56, 4096) == 0 and lib.cabinet_pw_bn_bwd_supported(16, 128, 4096) == 0
    assert lib.cabinet_pw_bn_bwd_supported(20, 16, 4096) == 0 and lib.cabinet_pw_bn_bwd_supported(16, 16, (1 << 21) + 4) == 0
    assert lib.cabinet_pw_bn_act_bwd_workspace_bytes(2, 104, 56, 4096) == 0
    assert lib.cabinet_pw_bn_dwconv_bwd_workspace_bytes(2, 16, 64, 8, 8, 4, 1) == 0


# ------------------------------------------------------------------------------------------------ through the modules
FAMILY_ROWS = {  # the three block forms of features.1 - features.3, with the routes once the plane threshold is lifted
    "project+shortcut": ((16, 16, 16, 3, 1, False, False), ("dwconv", "bn_act", "pwconv", "bn_act+res")),
    "expand/s2+project": ((16, 64, 24, 3, 2, False, False), ("pwconv", "bn_act_dwconv", "bn_act", "pwconv", "bn_act")),
    "expand+project+shortcut": ((24, 72, 24, 3, 1, False, False), ("pwconv", "bn_act_dwconv", "bn_act", "pwconv", "bn_act+res")),
}


@contextlib.contextmanager
def _module_setup(flag):
    """K10 on a 64 x 64 plane (its rule without the P >= 65536 threshold, which is a speed rule) and the fused-backward flag."""
    import cabinet_amd.functional as fn
    from cabinet_amd import _lib

    def supported(conv, x):
        return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.groups == 1 and conv.bias is None
                and bool(_lib.load().cabinet_pwconv_supported(conv.in_channels, conv.out_channels, x.shape[2] * x.shape[3])))

    old = fn.pwconv_supported, fn.PW_BN_BWD_FUSED
    fn.pwconv_supported, fn.PW_BN_BWD_FUSED = supported, flag
    try:
        yield
    finally:
        fn.pwconv_supported, fn.PW_BN_BWD_FUSED = old


def _module_run(c, flag, nodes):
    import test_gpu_backbone_blocks as tb
    import cabinet_amd.functional as fn

    counted = []
    for cls in (fn._PwBnAct, fn._PwBnActDwConv, fn._PwConv):
        old = cls.backward

        def backward(ctx, *g, _old=old, _name=cls.__name__):
            nodes.append(_name)
            return _old(ctx, *g)

        cls.backward = staticmethod(backward)
        counted.append((cls, old))
    try:
        with _module_setup(flag):
            return tb._device_run(c)
    finally:
        for cls, old in counted:
            cls.backward = staticmethod(old)


@gpu
@pytest.mark.parametrize("name", list(FAMILY_ROWS), ids=list(FAMILY_ROWS))
def test_block_flag_on_and_off(name):
    row, routes = FAMILY_ROWS[name]
    c = bc._case(("block",) + row, (2, row[0], 64, 64), 0)
    ref = bc.reference(c)
    nodes_on, nodes_off = [], []
    on, off = _module_run(c, True, nodes_on), _module_run(c, False, nodes_off)
    assert on["routes"] == off["routes"] == routes, (on["routes"], off["routes"])
    assert "_PwConv" not in nodes_on and nodes_on and set(nodes_off) == {"_PwConv"}, (nodes_on, nodes_off)
    assert torch.equal(on["y"], off["y"]), "the output changed"
    for k in off["buffers"]:
        assert torch.equal(on["buffers"][k], off["buffers"][k]), f"buffer {k} changed"
    fails = []
    pairs = [("dx", on["dx"], off["dx"], ref["dx"])] + [(k, on["grads"][k], off["grads"][k], ref["grads"][k]) for k in ref["grads"]]
    for k, a, b, q in pairs:
        assert a is not None and b is not None, k
        d, d0 = pc.dist(a, q), pc.dist(b, q)
        print(f"PWBN block {name} {k}: on {d:.3e} off {d0:.3e} from fp64")
        if d > pc.TOL or d > pc.bound(d0):
            fails.append(f"{k}: on {d:.3e}, off {d0:.3e}")
    assert not fails, "; ".join(fails)


@gpu
def test_frozen_parameters_and_no_grad_keep_todays_nodes():
    """A frozen parameter anywhere in the pair, or a forward that records nothing, leaves the two separate nodes (the parent's)."""
    row, _ = FAMILY_ROWS["expand/s2+project"]
    c = bc._case(("block",) + row, (2, row[0], 64, 64), 0)
    mod0, x0, g = bc.build(c)
    import cabinet_amd.functional as fn

    def nodes_of(freeze=None, grad=True):
        mod = copy.deepcopy(mod0).cuda()
        for n, p in mod.named_parameters():
            if freeze and n.endswith(freeze):
                p.requires_grad_(False)
        seen = []
        old = fn._PwBnAct.apply, fn._PwBnActDwConv.apply
        fn._PwBnAct.apply = staticmethod(lambda *a: (seen.append("act"), old[0](*a))[1])
        fn._PwBnActDwConv.apply = staticmethod(lambda *a: (seen.append("dw"), old[1](*a))[1])
        try:
            with _module_setup(True), torch.set_grad_enabled(grad):
                y = mod(x0.cuda().requires_grad_(grad))
                if grad:
                    y.backward(g.cuda())
        finally:
            del fn._PwBnAct.apply, fn._PwBnActDwConv.apply  # the inherited classmethod shows again
        torch.cuda.synchronize()
        return seen, mod

    assert nodes_of()[0] == ["dw", "act"]
    assert nodes_of(grad=False)[0] == []
    seen, mod = nodes_of(freeze="conv.0.weight")  # the expand convolution frozen: its pair falls back, the other stays
    assert seen == ["act"] and mod.conv[0].weight.grad is None and mod.conv[1].weight.grad is not None
    seen, mod = nodes_of(freeze="conv.1.bias")    # its BatchNorm's beta frozen
    assert seen == ["act"] and mod.conv[1].bias.grad is None and mod.conv[0].weight.grad is not None
