"""Class weights on the fused upsample + OHEM-CE kernels (cabinet_ohem_up[_pair]_w_fwd/bwd): the reference's default training
configuration (configs/train.yaml ``cls_pw: 0.5`` -> ``OhemCELoss(thresh, n_min, ignore_lb, weight=w)`` on both heads,
src/scripts/train.py:332-349) against the reference's own float64 vectors (tests/golden/g6_ohem_weighted.npz) and against a
float64 restatement of src/utils/loss.py:38-80 on the materialised F.interpolate output.

Every comparison input satisfies, checked here in float64 on the host before anything is compared: no valid pixel has
|w * ce - thresh| < 1e-5 (the fp32 kernels and the float64 computation select the same set, no pixel is excluded from any
comparison) and at least n_min pixels are above the threshold (the branch the kernels implement)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from test_ohem_weighted import fixture_cases, load_case

pytestmark = pytest.mark.gpu
TOL = 1e-3          # the project's gradient tolerance (tests/test_gpu_ohem.py)
GAP = 1e-5
IGNORE = 255


def ref64(low, lab, w, size, thresh, n_min, upstream=1.0):
    """loss.py:38-80 in float64 for the 'at least n_min above thresh' branch -> loss, dlow, n_valid, n_above; asserts the
    conditions on the input (module docstring)."""
    x = low.detach().double().cpu().requires_grad_(True)
    lab = lab.cpu()
    up = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    px = F.cross_entropy(up, lab, weight=None if w is None else w.detach().double().cpu(), ignore_index=IGNORE, reduction="none")
    valid = lab != IGNORE
    above = valid & (px > thresh)
    n_valid, n_above = int(valid.sum()), int(above.sum())
    assert float((px.detach()[valid] - thresh).abs().min()) >= GAP, "test input: a pixel sits on the threshold"
    assert n_above >= min(n_min, n_valid) > 0, "test input: not on the selected branch"
    loss = (px * above).sum() / n_above
    (upstream * loss).backward()
    return float(loss.detach()), x.grad, n_valid, n_above


def make_case(B, C, Hl, Wl, H, W, seed, zero_class=None):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    low2 = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    w = 0.5 + 3.0 * torch.rand(C, generator=g)
    if zero_class is not None:
        w[zero_class] = 0.0
    return low, low2, lab, w


class kernel_choice:
    """CABINET_OHEM_SEGMENT_KERNEL for the duration of a block (the library reads it per call)."""

    def __init__(self, var):
        self.var = var

    def __enter__(self):
        if self.var:
            os.environ[self.var] = "1"

    def __exit__(self, *exc):
        if self.var:
            del os.environ[self.var]


def run_single(low, lab, w, size, thresh, n_min, upstream=1.0):
    from cabinet_amd.loss import OhemCELoss

    crit = OhemCELoss(thresh, n_min, IGNORE, weight=None if w is None else w.clone()).cuda()
    x = low.cuda().requires_grad_(True)
    loss = crit.forward_upsampled(x, lab.cuda(), size)
    (upstream * loss).backward()
    torch.cuda.synchronize()
    return loss, x.grad


def run_pair(low_a, w_a, low_b, w_b, lab, size, thresh, n_min):
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    ca = OhemCELoss(thresh, n_min, IGNORE, weight=None if w_a is None else w_a.clone()).cuda()
    cb = OhemCELoss(thresh, n_min, IGNORE, weight=None if w_b is None else w_b.clone()).cuda()
    xa, xb = low_a.cuda().requires_grad_(True), low_b.cuda().requires_grad_(True)
    loss = ohem_upsampled_pair(ca, xa, cb, xb, lab.cuda(), size)
    loss.backward()
    torch.cuda.synchronize()
    return loss, xa.grad, xb.grad


def device_counts(low, lab, w, size, thresh):
    from cabinet_amd.functional import ohem_up_fwd_hip

    stats = ohem_up_fwd_hip(low.cuda(), lab.cuda(), size, thresh, IGNORE, None if w is None else w.cuda())[1].tolist()
    return int(stats[0]), int(stats[1])


# ---- 1. parity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", [0, 1])
def test_fixture_parity_single_and_pair(ci):
    from cabinet_amd.functional import ohem_up_pair_fwd_hip

    d, _ = fixture_cases()
    low, lab, w, size, n_min = load_case(d, ci)
    thresh = float(d[f"c{ci}.sel.thresh"])
    ref_loss, ref_dlow = float(d[f"c{ci}.sel.loss"]), torch.from_numpy(d[f"c{ci}.sel.dlow"])
    ref_counts = (int(d[f"c{ci}.sel.n_valid"]), int(d[f"c{ci}.sel.n_above"]))
    loss, grad = run_single(low, lab, w, size, thresh, n_min)
    assert "_OhemUpSelected" in type(loss.grad_fn).__name__
    print(f"fixture {ci} single: loss {loss.item():.9f} ref {ref_loss:.9f}")
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert_close(grad, ref_dlow, TOL, "dlow", atol=1e-9)
    assert device_counts(low, lab, w, size, thresh) == ref_counts
    loss2, ga, gb = run_pair(low, w, low, w, lab, size, thresh, n_min)
    assert "_OhemUpSelectedPair" in type(loss2.grad_fn).__name__
    assert abs(float(loss2) - 2 * ref_loss) <= 1e-5 * max(1.0, abs(2 * ref_loss))
    assert_close(ga, ref_dlow, TOL, "dlow a", atol=1e-9)
    assert_close(gb, ref_dlow, TOL, "dlow b", atol=1e-9)
    stats = ohem_up_pair_fwd_hip(low.cuda(), low.cuda(), lab.cuda(), size, thresh, IGNORE, w.cuda(), w.cuda())[1].tolist()
    assert [(int(s[0]), int(s[1])) for s in stats] == [ref_counts, ref_counts]


ROW = [(1, 8, 4, 64, 32, 512), (2, 19, 3, 128, 24, 1024), (1, 5, 2, 256, 16, 2048), (1, 27, 2, 64, 16, 512)]   # IPL 1 / 2 / 4 / 1
OTHER = [
    (1, 19, 4, 40, 32, 320),     # x8, Wl not a multiple of 64: segment kernel, FR = 8
    (1, 27, 6, 6, 48, 48),       # x8, 27 classes (widest class bucket)
    (1, 8, 3, 136, 24, 1088),    # x8, three column segments (64 + 64 + 8)
    (1, 8, 9, 7, 61, 50),        # non-integer ratio: general forward, FR = 0
    (2, 5, 10, 6, 20, 48),       # x2 rows, x8 columns, 5 classes (predicated bucket of 8)
    (1, 19, 16, 24, 64, 96),     # x4: general column pass, 19 classes
]
CASES = [(s, None) for s in ROW + OTHER] + [(s, "CABINET_OHEM_SEGMENT_KERNEL") for s in ROW]


@pytest.mark.parametrize("shape,env", CASES)
def test_weighted_kernels_vs_float64(shape, env):
    """Every kernel form, single head and pair (two different logits, two different weight tables)."""
    B, C, Hl, Wl, H, W = shape
    low, low2, lab, w = make_case(*shape, seed=H + C)
    w2 = w.flip(0).contiguous()
    size, thresh, n_min = (H, W), 0.7, B * H * W // 16
    ra = ref64(low, lab, w, size, thresh, n_min)
    rb = ref64(low2, lab, w2, size, thresh, n_min)
    with kernel_choice(env):
        loss, grad = run_single(low, lab, w, size, thresh, n_min)
        lossp, ga, gb = run_pair(low, w, low2, w2, lab, size, thresh, n_min)
        counts = device_counts(low, lab, w, size, thresh)
    assert "_OhemUpSelected" in type(loss.grad_fn).__name__ and "_OhemUpSelectedPair" in type(lossp.grad_fn).__name__
    print(f"{shape} {env}: loss {loss.item():.9f} ref {ra[0]:.9f}; pair {lossp.item():.9f} ref {ra[0] + rb[0]:.9f}")
    assert abs(float(loss) - ra[0]) <= 1e-5 * max(1.0, abs(ra[0]))
    assert abs(float(lossp) - (ra[0] + rb[0])) <= 1e-5 * max(1.0, abs(ra[0] + rb[0]))
    assert counts == (ra[2], ra[3])
    assert_close(grad, ra[1], TOL, "dlow", atol=1e-9)
    assert_close(ga, ra[1], TOL, "pair dlow a", atol=1e-9)
    assert_close(gb, rb[1], TOL, "pair dlow b", atol=1e-9)


# ---- 2. the fused path is taken, and nothing of full resolution times C is allocated ----------------------------------------

@pytest.mark.parametrize("pair", [False, True])
def test_weighted_criteria_stay_on_the_fused_head(pair):
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    B, C, Hl, Wl, H, W = 2, 19, 128, 128, 1024, 1024
    g = torch.Generator().manual_seed(5)
    w = (1.0 + 2.0 * torch.rand(C, generator=g))
    n_min = B * H * W // 16
    ca, cb = OhemCELoss(0.7, n_min, IGNORE, weight=w.clone()).cuda(), OhemCELoss(0.7, n_min, IGNORE, weight=w.flip(0)).cuda()
    xa = (torch.randn(B, C, Hl, Wl, generator=g) * 2.0).cuda().requires_grad_(True)
    xb = (torch.randn(B, C, Hl, Wl, generator=g) * 2.0).cuda().requires_grad_(True)
    lab = torch.randint(0, C, (B, H, W), generator=g).cuda()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    loss = ohem_upsampled_pair(ca, xa, cb, xb, lab, (H, W)) if pair else ca.forward_upsampled(xa, lab, (H, W))
    name = type(loss.grad_fn).__name__
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - start
    one_full_res_logits = B * C * H * W * 4
    print(f"pair={pair}: grad_fn {name}, {extra / 2 ** 20:.1f} MiB on top of the inputs (one (B,C,H,W) fp32 tensor: "
          f"{one_full_res_logits / 2 ** 20:.1f} MiB)")
    assert name == ("_OhemUpSelectedPairBackward" if pair else "_OhemUpSelectedBackward")
    assert extra < one_full_res_logits
    assert bool(torch.isfinite(xa.grad).all()) and float(xa.grad.abs().sum()) > 0


# ---- 3. the graphed steps take weighted criteria ----------------------------------------------------------------------------

def enet_weights(n_classes, cls_pw=0.5):
    """ENet inverse-log weights (Paszke et al. 2016) of a skewed class distribution: (1 / ln(1.02 + p)) ** cls_pw, all >= 1."""
    p = 0.6 ** np.arange(n_classes)
    p = p / p.sum()
    return torch.tensor((1.0 / np.log(1.02 + p)) ** cls_pw, dtype=torch.float32)


def test_graphed_train_step_with_class_weights_equals_eager():
    """tests/test_gpu_model.py::test_graphed_train_step_equals_eager with weighted criteria (its tolerances: the stock backward
    kernels' atomics are explained there), plus: the losses are far from those of the unweighted run of the same batches."""
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria, synthetic_batch

    w = enet_weights(8)
    assert float(w.min()) >= 1.0
    batches = [synthetic_batch(2, 256, 256, 8, "cuda", seed=20 + i) for i in range(4)]
    ign = (batches[0][0], torch.full_like(batches[0][1], 255))
    res = []
    for mode in ("eager", "graphed", "unweighted"):
        net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-2, momentum=0.9)
        crit = make_criteria(2, 256, 256, "cuda", weight=None if mode == "unweighted" else w)
        if mode != "unweighted":
            assert all(c.weight.is_cuda and torch.equal(c.weight.cpu(), w) for c in crit)
        step = GraphedTrainStep(net, crit, optimizer=opt, warmup=1) if mode == "graphed" else TrainStep(net, crit, optimizer=opt)
        losses = [float(step(*b)) for b in batches]
        losses.append(float(step(*ign)))
        losses.append(float(step(*batches[1])))
        if mode == "graphed":
            assert step.g_bwd is not None and step.fallbacks == 1   # only the all-ignored batch left the graphs
        res.append((losses, {k: v.clone() for k, v in net.state_dict().items()}))
    (la, sa), (lb_, sb), (lu, _) = res
    print("eager", la, "graphed", lb_, "unweighted", lu)
    assert la[4] == 0.0 and lb_[4] == 0.0
    for x, y in zip(la, lb_):
        assert abs(x - y) <= 1e-4 * max(1.0, abs(x)), (la, lb_)
    for k in sa:
        assert_close(sb[k].double(), sa[k].double(), 2e-3, k, atol=1e-5)
    for i in (0, 1, 2, 3, 5):   # weights dropped anywhere on the way would give the unweighted losses
        assert abs(lb_[i] - lu[i]) > 100 * 1e-4 * max(1.0, abs(lu[i])), (lb_, lu)


def test_graphed_step_sees_in_place_weight_updates():
    """The captured graphs hold the weight buffers' addresses: ``crit.weight.copy_()`` reaches the next replay."""
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria, synthetic_batch

    w = enet_weights(8)
    batches = [synthetic_batch(2, 256, 256, 8, "cuda", seed=40 + i) for i in range(3)]
    out = []
    for graphed in (False, True):
        net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
        crit = make_criteria(2, 256, 256, "cuda", weight=w)
        step = GraphedTrainStep(net, crit, warmup=1) if graphed else TrainStep(net, crit)
        losses = [float(step(*batches[0])), float(step(*batches[1]))]
        for c in crit:
            c.weight.copy_(2.0 * w.cuda())
        losses.append(float(step(*batches[2])))
        if graphed:
            assert step.g_bwd is not None and step.fallbacks == 0
        out.append(losses)
    for x, y in zip(*out):
        assert abs(x - y) <= 1e-4 * max(1.0, abs(x)), out


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_graphed_ddp_step_world1_with_class_weights():
    """tests/test_gpu_ddp_single.py::test_graphed_ddp_step_world1_matches_graphed_single with weighted criteria."""
    import torch.distributed as dist

    from cabinet_amd.train import GraphedDDPStep, GraphedTrainStep, build_model, make_criteria, synthetic_batch

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    assert not dist.is_initialized()
    w = enet_weights(8)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", world_size=1, rank=0,
                            device_id=torch.device("cuda", 0))
    try:
        batches = [synthetic_batch(2, 256, 256, 8, "cuda", seed=30 + i) for i in range(4)]
        res = []
        for mode in ("single", "ddp", "unweighted"):
            net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
            opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-2)
            crit = make_criteria(2, 256, 256, "cuda", weight=None if mode == "unweighted" else w)
            step = (GraphedDDPStep(net, crit, optimizer=opt, warmup=1, always_reduce=True, bucket_mb=4.0) if mode == "ddp"
                    else GraphedTrainStep(net, crit, optimizer=opt, warmup=1))
            losses = [float(step(*b)) for b in batches] + [float(step(*batches[1]))]
            if mode == "ddp":
                assert step.graphs is not None and step.fallbacks == 0
            res.append((losses, {k: v.clone() for k, v in net.state_dict().items()}))
        (la, sa), (lb_, sb), (lu, _) = res
        print("single", la, "ddp", lb_, "unweighted", lu)
        for x, y in zip(la, lb_):
            assert abs(x - y) <= 1e-5 * max(1.0, abs(x)), (la, lb_)
        for k in sa:
            err, den = float((sb[k].double() - sa[k].double()).norm()), float(sa[k].double().norm())
            assert err <= 2e-3 * den + 1e-5 * sa[k].numel() ** 0.5, (k, err, den)
        for x, y in zip(lb_, lu):
            assert abs(x - y) > 100 * 1e-4 * max(1.0, abs(y)), (lb_, lu)
    finally:
        dist.destroy_process_group()


# ---- 4. unit weights are the unweighted kernels' bits -----------------------------------------------------------------------

@pytest.mark.parametrize("shape,env", [(s, None) for s in ROW[:3] + OTHER[:1] + OTHER[3:4]] + [(ROW[1], "CABINET_OHEM_SEGMENT_KERNEL")])
def test_unit_weights_are_bitwise_the_unweighted_result(shape, env):
    B, C, Hl, Wl, H, W = shape
    low, low2, lab, w = make_case(*shape, seed=H + C + 1)
    ones = torch.ones(C)
    size, thresh, n_min = (H, W), 0.7, B * H * W // 16
    with kernel_choice(env):
        l0, g0 = run_single(low, lab, None, size, thresh, n_min)
        l1, g1 = run_single(low, lab, ones, size, thresh, n_min)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)
        p0 = run_pair(low, None, low2, None, lab, size, thresh, n_min)
        p1 = run_pair(low, ones, low2, ones, lab, size, thresh, n_min)
        assert all(torch.equal(a, b) for a, b in zip(p0, p1))
        # one weighted and one unweighted head in ONE pair launch = the two single heads
        lw, gw = run_single(low, lab, w, size, thresh, n_min)
        l2, g2 = run_single(low2, lab, None, size, thresh, n_min)
        lp, ga, gb = run_pair(low, w, low2, None, lab, size, thresh, n_min)
        assert "_OhemUpSelectedPair" in type(lp.grad_fn).__name__
        assert torch.equal(ga, gw) and torch.equal(gb, g2)
        # (the pair forms its sum in float64 before the one rounding to fp32, the single heads round first)
        assert abs(float(lp) - (float(lw) + float(l2))) <= 1e-6 * abs(float(lp))
        assert not torch.equal(gw, g0)


# ---- 5. weight 0 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,env", [(ROW[1], None), (ROW[1], "CABINET_OHEM_SEGMENT_KERNEL"), (OTHER[3], None)])
def test_a_class_of_weight_zero(shape, env):
    B, C, Hl, Wl, H, W = shape
    low, _, lab, w = make_case(*shape, seed=H + C + 2, zero_class=2)
    assert int((lab == 2).sum()) > 0
    size, thresh, n_min = (H, W), 0.7, B * H * W // 16
    ref_loss, ref_dlow, n_valid, n_above = ref64(low, lab, w, size, thresh, n_min)
    with kernel_choice(env):
        loss, grad = run_single(low, lab, w, size, thresh, n_min)
        counts = device_counts(low, lab, w, size, thresh)
        counts_unweighted = device_counts(low, lab, None, size, thresh)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert counts == (n_valid, n_above) and counts_unweighted[0] == n_valid == int((lab != IGNORE).sum())
    assert counts[1] < counts_unweighted[1]          # the class' pixels are valid but never selected
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert_close(grad, ref_dlow, TOL, "dlow", atol=1e-9)
    # no contribution from the class' pixels: relabelling them as ignored changes neither #above nor the gradient's bits
    lab_ign = lab.clone()
    lab_ign[lab == 2] = IGNORE
    with kernel_choice(env):
        loss_i, grad_i = run_single(low, lab_ign, w, size, thresh, n_min)
    assert torch.equal(grad_i, grad) and torch.equal(loss_i, loss)


# ---- 6. determinism, linearity in the upstream gradient ---------------------------------------------------------------------

@pytest.mark.parametrize("shape", [ROW[1], OTHER[0], OTHER[3]])
def test_weighted_head_is_bit_reproducible_and_linear_in_the_upstream_gradient(shape):
    B, C, Hl, Wl, H, W = shape
    low, low2, lab, w = make_case(*shape, seed=H + C + 3)
    size, thresh, n_min = (H, W), 0.7, B * H * W // 16
    l0, g0 = run_single(low, lab, w, size, thresh, n_min)
    l1, g1 = run_single(low, lab, w, size, thresh, n_min)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    p0 = run_pair(low, w, low2, w.flip(0), lab, size, thresh, n_min)
    p1 = run_pair(low, w, low2, w.flip(0), lab, size, thresh, n_min)
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    # the upstream gradient is one fp32 factor on the kernels' output: 3 g differs from g(3) by two roundings at most
    _, g3 = run_single(low, lab, w, size, thresh, n_min, upstream=3.0)
    assert_close(g3, 3.0 * g0, 1e-6, "3 x upstream", atol=0.0)


# ---- 7. half-precision buffers never reach the C ABI ------------------------------------------------------------------------

def test_half_precision_weight_buffer_under_autocast(monkeypatch):
    from cabinet_amd import functional as Fn
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    shape = ROW[1]
    B, C, Hl, Wl, H, W = shape
    low, low2, lab, w = make_case(*shape, seed=H + C + 4)
    w = w.half().float()            # the values a half buffer can hold
    size, n_min = (H, W), B * H * W // 16
    seen = []
    real_ptr = Fn._ptr

    def spy(t):
        if t is not None:
            seen.append(t.dtype)
        return real_ptr(t)

    monkeypatch.setattr(Fn, "_ptr", spy)
    out = {}
    for tag in ("fp32", "half"):
        ca, cb = OhemCELoss(0.7, n_min, IGNORE, weight=w.clone()).cuda(), OhemCELoss(0.7, n_min, IGNORE, weight=w.flip(0)).cuda()
        if tag == "half":
            ca, cb = ca.half(), cb.half()
            assert ca.weight.dtype == torch.float16 and cb.weight.dtype == torch.float16
        xa, xb, xs = (t.cuda().requires_grad_(True) for t in (low, low2, low))
        seen.clear()
        with torch.autocast("cuda", dtype=torch.float16, enabled=(tag == "half")):
            lp = ohem_upsampled_pair(ca, xa, cb, xb, lab.cuda(), size)
            ls = ca.forward_upsampled(xs, lab.cuda(), size)
            (lp + ls).backward()
        torch.cuda.synchronize()
        assert "_OhemUpSelectedPair" in type(lp.grad_fn).__name__ and "_OhemUpSelected" in type(ls.grad_fn).__name__
        floating = [dt for dt in seen if dt.is_floating_point]
        assert len(seen) > 20 and set(floating) <= {torch.float32, torch.float64}, set(seen)   # float64: the (n,3) statistics
        out[tag] = (lp.detach(), ls.detach(), xa.grad, xb.grad, xs.grad)
    assert all(torch.equal(a, b) for a, b in zip(out["fp32"], out["half"]))


# ---- 8. the rare branch keeps the composite path, weights included ----------------------------------------------------------

@pytest.mark.parametrize("pair", [False, True])
def test_weighted_top_n_min_branch_takes_the_composite_path(pair):
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    d, _ = fixture_cases()
    low, lab, w, size, n_min = load_case(d, 0)
    thresh = float(d["c0.topk.thresh"])
    ref_loss, ref_dlow = float(d["c0.topk.loss"]), torch.from_numpy(d["c0.topk.dlow"])
    ca, cb = OhemCELoss(thresh, n_min, IGNORE, weight=w.clone()).cuda(), OhemCELoss(thresh, n_min, IGNORE, weight=w.clone()).cuda()
    x, x2, y = (low.cuda().requires_grad_(True) for _ in range(3))
    labc = lab.cuda()
    if pair:
        loss = ohem_upsampled_pair(ca, x, cb, x2, labc, size)
    else:
        loss = ca.forward_upsampled(x, labc, size)
    assert "_OhemUpSelected" not in type(loss.grad_fn).__name__
    loss.backward()
    want = ca.forward(F.interpolate(y, size=size, mode="bilinear", align_corners=False), labc)
    want.backward()
    torch.cuda.synchronize()
    nh = 2 if pair else 1
    # the same operators on the same inputs (forward kernels without atomics); the upsample's backward adds with atomics
    assert abs(float(loss) - nh * float(want)) <= 1e-6 * abs(nh * float(want))
    assert_close(x.grad, y.grad, 1e-5, "dlow vs composite", atol=1e-9)
    assert abs(float(loss) - nh * ref_loss) <= 1e-5 * max(1.0, abs(nh * ref_loss))
    assert_close(x.grad, ref_dlow, TOL, "dlow vs reference", atol=1e-9)
