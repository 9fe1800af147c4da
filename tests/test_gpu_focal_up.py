"""SoftmaxFocalLoss on the fused upsample + loss kernels (cabinet_focal_up_fwd/bwd, the focal mode of the OHEM kernels): the
reference's own float64 vectors (tests/golden/g11_focal_up.npz), every kernel form against the float64 closed form of
tests/focal_golden.py, the pinned edge values, and the eager and one-graph train steps.

Tolerances are the project's own (tests/test_gpu_ohem_weighted.py): loss within 1e-5 * max(1, |ref|), gradients through
assert_close(..., 1e-3, atol=1e-9)."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from focal_golden import focal_up_ref
from test_focal_up import IGNORE, fixture, load_case
from test_gpu_ohem_weighted import kernel_choice

pytestmark = pytest.mark.gpu
TOL = 1e-3


def loss_close(got, ref, what=""):
    print(f"{what}: loss {got:.9f} ref {ref:.9f}")
    assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (what, got, ref)


def run_single(low, lab, w, size, gamma, upstream=1.0):
    from cabinet_amd.loss import SoftmaxFocalLoss

    crit = SoftmaxFocalLoss(gamma, weight=None if w is None else w.clone(), ignore_lb=IGNORE).cuda()
    x = low.cuda().requires_grad_(True)
    loss = crit.forward_upsampled(x, lab.cuda(), size)
    (upstream * loss).backward()
    torch.cuda.synchronize()
    return loss, x.grad


def run_pair(low_a, w_a, g_a, low_b, w_b, g_b, lab, size):
    from cabinet_amd.loss import SoftmaxFocalLoss, focal_upsampled_pair

    ca = SoftmaxFocalLoss(g_a, weight=None if w_a is None else w_a.clone(), ignore_lb=IGNORE).cuda()
    cb = SoftmaxFocalLoss(g_b, weight=None if w_b is None else w_b.clone(), ignore_lb=IGNORE).cuda()
    xa, xb = low_a.cuda().requires_grad_(True), low_b.cuda().requires_grad_(True)
    loss = focal_upsampled_pair(ca, xa, cb, xb, lab.cuda(), size)
    loss.backward()
    torch.cuda.synchronize()
    return loss, xa.grad, xb.grad


def fused(loss):
    return "_FocalUp" in type(loss.grad_fn).__name__


# ---- 1. the reference's vectors ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_fixture_parity_single_and_pair(ci):
    d, _, gammas = fixture()
    low, lab, w, size = load_case(d, ci)
    singles = {}
    for wtag in ("nw", "w"):
        for gi, gamma in enumerate(gammas):
            loss, grad = run_single(low, lab, w if wtag == "w" else None, size, gamma)
            assert fused(loss)
            loss_close(float(loss), float(d[f"c{ci}.{wtag}.g{gi}.loss"]), f"fixture {ci} {wtag} gamma {gamma}")
            assert bool(torch.isfinite(grad).all())
            assert_close(grad, torch.from_numpy(d[f"c{ci}.{wtag}.g{gi}.dlow"]), TOL, f"dlow {wtag} g{gi}", atol=1e-9)
            singles[(wtag, gi)] = (float(loss), grad)
    # two different (gamma, weight) combinations in one launch = the sum of the singles
    (la, ga), (lb_, gb) = singles[("w", 2)], singles[("nw", 1)]
    loss, xa, xb = run_pair(low, w, gammas[2], low, None, gammas[1], lab, size)
    assert fused(loss)
    assert abs(float(loss) - (la + lb_)) <= 1e-6 * max(1.0, abs(la + lb_))
    assert_close(xa, ga, 1e-6, "pair dlow a", atol=1e-12)
    assert_close(xb, gb, 1e-6, "pair dlow b", atol=1e-12)
    assert_close(xa, torch.from_numpy(d[f"c{ci}.w.g2.dlow"]), TOL, "pair dlow a vs fixture", atol=1e-9)
    assert_close(xb, torch.from_numpy(d[f"c{ci}.nw.g1.dlow"]), TOL, "pair dlow b vs fixture", atol=1e-9)


# ---- 2. every kernel form against the float64 closed form ----------------------------------------------------------------

def make_case(B, C, Hl, Wl, H, W, seed, zero_class=1):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    low2 = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.15] = IGNORE
    w = 0.5 + 3.0 * torch.rand(C, generator=g)
    w[zero_class] = 0.0
    return low, low2, lab, w


SWEEP = [((1, 32, 3, 5, 24, 40), None),                              # C = 32, Wl % 4 != 0
         ((1, 19, 1, 128, 8, 1024), None),                           # whole-row kernel, IPL = 2
         ((1, 3, 4, 64, 32, 512), None),                             # C < 8
         ((1, 19, 1, 128, 8, 1024), "CABINET_OHEM_SEGMENT_KERNEL"),  # the same rows through the segment kernel
         ((1, 18, 5, 6, 23, 31), None)]                              # general ratio, 17..20 classes (the 20-slot forward)


@pytest.mark.parametrize("shape,env", SWEEP)
def test_kernel_forms_vs_float64(shape, env):
    B, C, Hl, Wl, H, W = shape
    low, low2, lab, w = make_case(*shape, seed=sum(shape))
    with kernel_choice(env):
        loss, grad = run_single(low, lab, w, (H, W), 2.0)
        pl, ga, gb = run_pair(low, w, 0.5, low2, None, 5.0, lab, (H, W))
    assert fused(loss) and fused(pl)
    ref, rgrad, _ = focal_up_ref(low, lab, (H, W), 2.0, w, IGNORE)
    loss_close(float(loss), ref, f"{shape} single")
    assert_close(grad, rgrad, TOL, "dlow", atol=1e-9)
    ra, rga, _ = focal_up_ref(low, lab, (H, W), 0.5, w, IGNORE)
    rb, rgb, _ = focal_up_ref(low2, lab, (H, W), 5.0, None, IGNORE)
    loss_close(float(pl), ra + rb, f"{shape} pair")
    assert_close(ga, rga, TOL, "pair dlow a", atol=1e-9)
    assert_close(gb, rgb, TOL, "pair dlow b", atol=1e-9)


def test_more_than_32_classes_and_unsupported_gamma_take_the_composite():
    from cabinet_amd.loss import SoftmaxFocalLoss

    low, _, lab, w = make_case(1, 33, 3, 5, 24, 40, seed=5)
    for C, gamma in ((33, 2.0), (8, -1.0), (8, float("inf"))):
        x = low[:, :C].cuda().requires_grad_(True)
        lb = lab.clamp(max=C - 1).cuda() if C < 33 else lab.cuda()
        lb = torch.where(lab.cuda() == IGNORE, lab.cuda(), lb)
        crit = SoftmaxFocalLoss(gamma, weight=w[:C].clone(), ignore_lb=IGNORE).cuda()
        loss = crit.forward_upsampled(x, lb, (24, 40))
        assert not fused(loss)
        want = crit(F.interpolate(x.detach(), size=(24, 40), mode="bilinear", align_corners=False), lb)
        assert torch.allclose(loss.detach(), want, rtol=0, atol=0, equal_nan=True)
        if C == 33:
            loss.backward()
            ref, rgrad, _ = focal_up_ref(low, lab, (24, 40), 2.0, w, IGNORE)
            loss_close(float(loss), ref, "C = 33 composite")
            assert_close(x.grad, rgrad, TOL, "dlow", atol=1e-9)


def test_label_checks_raise_like_the_ohem_head():
    from cabinet_amd.loss import SoftmaxFocalLoss

    crit = SoftmaxFocalLoss(2.0).cuda()
    low = torch.randn(1, 5, 4, 4, device="cuda")
    with pytest.raises(RuntimeError, match=r"labels must be int64 \(torch.long\), got torch.int32"):
        crit.forward_upsampled(low, torch.zeros(1, 32, 32, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="do not match logits batch"):
        crit.forward_upsampled(low, torch.zeros(2, 32, 32, dtype=torch.long, device="cuda"), (32, 32))
    with pytest.raises(RuntimeError, match="do not match logits batch"):
        crit.forward_upsampled(low, torch.zeros(1, 32, 32, dtype=torch.long), (32, 32))


# ---- 3. pinned edges ----------------------------------------------------------------------------------------------------------

EDGE = (1, 8, 4, 8, 32, 64)   # x8, segment kernel


def test_gamma_zero_is_the_weighted_cross_entropy_mean():
    B, C, Hl, Wl, H, W = EDGE
    low, _, lab, w = make_case(*EDGE, seed=1)
    for shape_low, size in ((low, (H, W)), (low[:, :5, :3, :7].contiguous(), (20, 50))):   # and the general ratio
        lb = lab[:, :size[0], :size[1]].clamp(max=shape_low.shape[1] - 1)
        lb = torch.where(lab[:, :size[0], :size[1]] == IGNORE, torch.full_like(lb, IGNORE), lb)
        ww = w[:shape_low.shape[1]]
        loss, grad = run_single(shape_low, lb, ww, size, 0.0)
        x = shape_low.double().requires_grad_(True)
        ce = F.cross_entropy(F.interpolate(x, size=size, mode="bilinear", align_corners=False), lb, weight=ww.double(),
                             ignore_index=IGNORE, reduction="mean")
        ce.backward()
        assert fused(loss)
        loss_close(float(loss), float(ce), "gamma 0 vs weighted CE")
        assert_close(grad, x.grad, TOL, "dlow", atol=1e-9)


def test_confident_pixels_have_finite_gradients_below_gamma_one():
    d, _, gammas = fixture()
    ci = int(d["conf"])
    low, lab, w, size = load_case(d, ci)
    assert gammas[1] == 0.5 and int(d[f"c{ci}.n_conf"]) >= 64
    for wtag in ("nw", "w"):
        loss, grad = run_single(low, lab, w if wtag == "w" else None, size, 0.5)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
        ref, rgrad, _ = focal_up_ref(low, lab, size, 0.5, w if wtag == "w" else None, IGNORE)
        loss_close(float(loss), ref, f"confident {wtag}")
        assert_close(grad, rgrad, TOL, "dlow", atol=1e-9)


def test_no_weight_in_the_batch_gives_nan_loss_and_zero_gradient():
    B, C, Hl, Wl, H, W = EDGE
    low, low2, lab, w = make_case(*EDGE, seed=2)
    only_zero = torch.where(lab == IGNORE, lab, torch.ones_like(lab))     # class 1 weighs 0
    for lb, ww in ((torch.full_like(lab, IGNORE), w), (torch.full_like(lab, IGNORE), None), (only_zero, w)):
        for gamma in (0.0, 0.5, 2.0):
            loss, grad = run_single(low, lb, ww, (H, W), gamma)
            assert fused(loss) and bool(torch.isnan(loss)) and float(grad.abs().max()) == 0.0
        loss, ga, gb = run_pair(low, ww, 2.0, low2, ww, 0.5, lb, (H, W))
        assert bool(torch.isnan(loss)) and float(ga.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0


def test_one_valid_pixel():
    B, C, Hl, Wl, H, W = EDGE
    low, _, lab, w = make_case(*EDGE, seed=3)
    for size, lw in (((H, W), low), ((20, 50), low[:, :, :3, :7].contiguous())):
        lb = torch.full((1,) + size, IGNORE, dtype=torch.long)
        lb[0, size[0] - 3, size[1] - 2] = 4
        for gamma in (0.0, 0.5, 2.0):
            loss, grad = run_single(lw, lb, w, size, gamma)
            ref, rgrad, st = focal_up_ref(lw, lb, size, gamma, w, IGNORE)
            assert st[0] == 1
            loss_close(float(loss), ref, f"one pixel gamma {gamma}")
            assert_close(grad, rgrad, TOL, "dlow", atol=1e-9)


def test_out_of_range_label_gives_nan_and_a_poisoned_count():
    from cabinet_amd.functional import focal_up_fwd_hip

    B, C, Hl, Wl, H, W = EDGE
    low, _, lab, w = make_case(*EDGE, seed=4)
    for size, lw in (((H, W), low), ((20, 50), low[:, :, :3, :7].contiguous())):
        for bad in (C, 254, -3, 2 ** 40):
            lb = lab[:, :size[0], :size[1]].clone()
            lb[0, 5, 7] = bad
            loss, grad = run_single(lw, lb, w, size, 2.0)
            assert fused(loss) and bool(torch.isnan(loss))
            loss_px, stats = focal_up_fwd_hip([lw.cuda()], lb.cuda(), size, [2.0], IGNORE, [w.cuda()])
            torch.cuda.synchronize()
            assert float(stats[0, 0]) < 0 and bool(torch.isfinite(loss_px).all())
    # the clean labels of the same case: a count, not a flag
    _, stats = focal_up_fwd_hip([low.cuda()], lab.cuda(), (H, W), [2.0], IGNORE, [w.cuda()])
    assert int(stats[0, 0]) == int((lab != IGNORE).sum())


def test_bit_reproducible_linear_in_upstream_and_out_fully_written():
    from cabinet_amd.functional import focal_up_bwd_hip, focal_up_fwd_hip

    for shape in (EDGE, (1, 19, 1, 128, 8, 1024), (1, 5, 7, 9, 40, 50)):
        B, C, Hl, Wl, H, W = shape
        low, low2, lab, w = make_case(*shape, seed=7)
        l1, g1 = run_single(low, lab, w, (H, W), 0.5)
        l2, g2 = run_single(low, lab, w, (H, W), 0.5)
        assert torch.equal(l1.detach(), l2.detach()) and torch.equal(g1, g2)
        p1, p2 = run_pair(low, w, 2.0, low2, None, 0.5, lab, (H, W)), run_pair(low, w, 2.0, low2, None, 0.5, lab, (H, W))
        assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(p1, p2))
        _, g3 = run_single(low, lab, w, (H, W), 0.5, upstream=3.0)
        assert_close(g3, 3.0 * g1, 1e-6, "3 g upstream", atol=1e-12)
        lows, lb, ws = [low.cuda(), low2.cuda()], lab.cuda(), [w.cuda(), None]
        loss_px, _ = focal_up_fwd_hip(lows, lb, (H, W), [2.0, 0.5], IGNORE, ws)
        out = torch.full((2, B, C, Hl, Wl), float("nan"), device="cuda")
        got = focal_up_bwd_hip(lows, lb, loss_px, (H, W), [2.0, 0.5], IGNORE, 1.0, ws, out=out)
        assert got is out and bool(torch.isfinite(out).all())
        assert torch.equal(out, focal_up_bwd_hip(lows, lb, loss_px, (H, W), [2.0, 0.5], IGNORE, 1.0, ws))


def test_backward_is_linear_in_coef_whatever_its_sign():
    """``coef`` is a free argument of cabinet_focal_up_bwd (dlogits_low = coef * U^T[...]): the on / off test of a pixel must not
    see it.  A general-ratio shape and an x8 shape off the whole-row form (segment x pass), a whole-row shape, and the whole-row
    shape forced through the segment kernel."""
    from cabinet_amd.functional import focal_up_bwd_hip, focal_up_fwd_hip

    for shape, env in (((1, 5, 7, 9, 40, 50), None), (EDGE, None), ((1, 19, 1, 128, 8, 1024), None),
                       ((1, 19, 1, 128, 8, 1024), "CABINET_OHEM_SEGMENT_KERNEL")):
        B, C, Hl, Wl, H, W = shape
        low, low2, lab, w = make_case(*shape, seed=11)
        lows, lb, ws = [low.cuda(), low2.cuda()], lab.cuda(), [w.cuda(), None]
        loss_px, _ = focal_up_fwd_hip(lows, lb, (H, W), [2.0, 0.5], IGNORE, ws)
        with kernel_choice(env):
            one = focal_up_bwd_hip(lows, lb, loss_px, (H, W), [2.0, 0.5], IGNORE, 1.0, ws)
            neg = focal_up_bwd_hip(lows, lb, loss_px, (H, W), [2.0, 0.5], IGNORE, -2.0, ws)
            single = focal_up_bwd_hip(lows[:1], lb, loss_px[:1], (H, W), [2.0], IGNORE, -2.0, ws[:1])
        assert float(one.abs().max()) > 0
        assert_close(neg, -2.0 * one, 1e-6, f"coef -2 {shape} {env}", atol=1e-12)
        assert_close(single[0], -2.0 * one[0], 1e-6, f"coef -2 single {shape} {env}", atol=1e-12)


def test_weight_of_the_wrong_length_names_the_criterion():
    from cabinet_amd.loss import SoftmaxFocalLoss

    crit = SoftmaxFocalLoss(2.0, weight=torch.ones(4)).cuda()
    with pytest.raises(RuntimeError, match="SoftmaxFocalLoss: weight of shape"):
        crit.forward_upsampled(torch.randn(1, 5, 4, 4, device="cuda"), torch.zeros(1, 32, 32, dtype=torch.long, device="cuda"))


# ---- 4. the train steps -------------------------------------------------------------------------------------------------------

def _sync_debug_mode_is_honoured():
    """Whether this torch build raises on a synchronising call under set_sync_debug_mode("error")."""
    t = torch.ones(1, device="cuda")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def test_focal_train_steps_eager_and_one_graph():
    """The model and batches of test_graphed_train_step_with_class_weights_equals_eager (and its bounds: 1e-4 on the losses,
    2e-3 / 1e-5 on the parameters) with focal criteria: TrainStep through upsampled_pair, GraphedTrainStep as ONE graph.  The
    all-ignored batch in the middle replays like any other: NaN loss, zero gradients, no fallback, nothing read on the host."""
    from cabinet_amd.loss import SoftmaxFocalLoss
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria, synthetic_batch
    from test_gpu_ohem_weighted import enet_weights

    w = enet_weights(8)
    batches = [synthetic_batch(2, 256, 256, 8, "cuda", seed=20 + i) for i in range(4)]
    ign = (batches[0][0], torch.full_like(batches[0][1], 255))
    seq = batches + [ign, batches[1]]
    honoured = _sync_debug_mode_is_honoured()
    print("sync debug mode honoured:", honoured)
    res = []
    for mode in ("eager", "graphed"):
        net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-2, momentum=0.9)
        crit = make_criteria(2, 256, 256, "cuda", weight=w, loss="focal")
        assert all(type(c) is SoftmaxFocalLoss and c.weight.is_cuda for c in crit)
        if mode == "eager":
            step = TrainStep(net, crit, optimizer=opt)
            losses = [float(step(*b)) for b in seq]
        else:
            step = GraphedTrainStep(net, crit, optimizer=opt, warmup=1)
            losses = [float(step(*seq[0]))]          # the eager warm-up step; the graph is recorded after it
            assert step.g_fwd is not None and step.g_bwd is None and step.focal
            kept = []
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error" if honoured else prev)
            try:
                for b in seq[1:]:
                    kept.append((step(*b).clone(), step.last_stats.clone()))
            finally:
                torch.cuda.set_sync_debug_mode(prev)
            losses += [float(l) for l, _ in kept]
            assert step.fallbacks == 0
            assert tuple(step.last_stats.shape) == (2, 3) and step.last_stats.dtype == torch.float64
            n_valid = [int((b[1] != 255).sum()) for b in seq[1:]]
            assert [int(s[0, 0]) for _, s in kept] == n_valid and [int(s[1, 0]) for _, s in kept] == n_valid
        res.append((losses, {k: v.clone() for k, v in net.state_dict().items()}))
    (la, sa), (lb_, sb) = res
    print("eager", la, "graphed", lb_)
    assert math.isnan(la[4]) and math.isnan(lb_[4])
    for i, (x, y) in enumerate(zip(la, lb_)):
        if i != 4:
            assert abs(x - y) <= 1e-4 * max(1.0, abs(x)), (la, lb_)
    for k in sa:
        assert bool(torch.isfinite(sa[k].double()).all()), k
        assert_close(sb[k].double(), sa[k].double(), 2e-3, k, atol=1e-5)


def test_graphed_ddp_step_with_focal_criteria():
    """With graphs it refuses at construction, with a text that says so; use_graphs=False runs through upsampled_pair and
    gives the eager TrainStep's loss."""
    import os

    import torch.distributed as dist

    from cabinet_amd.train import GraphedDDPStep, TrainStep, build_model, make_criteria, synthetic_batch
    from test_gpu_ohem_weighted import _free_port, enet_weights

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    assert not dist.is_initialized()
    w = enet_weights(8)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", world_size=1, rank=0,
                            device_id=torch.device("cuda", 0))
    try:
        batch = synthetic_batch(2, 256, 256, 8, "cuda", seed=30)
        losses = []
        for mode in ("single", "ddp"):
            net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
            crit = make_criteria(2, 256, 256, "cuda", weight=w, loss="focal")
            if mode == "ddp":
                with pytest.raises(RuntimeError, match="needs two OhemCELoss criteria"):
                    GraphedDDPStep(net, crit, use_graphs=True)
                step = GraphedDDPStep(net, crit, use_graphs=False, always_reduce=True, bucket_mb=4.0)
            else:
                step = TrainStep(net, crit)
            losses.append(float(step(*batch)))
        print("single", losses[0], "ddp", losses[1])
        assert abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[0]))
    finally:
        dist.destroy_process_group()
