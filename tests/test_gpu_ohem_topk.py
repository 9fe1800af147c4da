"""The top-n_min branch of OHEM-CE on the HIP kernels (``device_select=True``): cabinet_ohem_select (radix select of the k-th
largest per-pixel loss, on the device) and the backward kernels that read their threshold from it -- reference
src/utils/loss.py:67-80, both branches -- against ``torch.sort``, against the reference's own float64 vectors
(tests/golden/g7_ohem_topk.npz at the real thresh = 0.7, and the two ``topk`` cases of g6_ohem_weighted.npz), against the
composite path, and inside GraphedTrainStep (graph B-any).

What the stored inputs guarantee (tests/test_ohem_topk.py checks it on the host): no pixel within 1e-5 of thresh, and whatever
lies within 1e-4 of the k-th largest loss is saturated (loss <= 1e-6), so an fp32 kernel cannot keep a different set that
moves a gradient element."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from test_ohem_topk import case_names, fixture, load_head
from test_ohem_weighted import fixture_cases as g6_cases, load_case as g6_load

pytestmark = pytest.mark.gpu
TOL = 1e-3          # the project's gradient tolerance (tests/test_gpu_ohem.py)
IGNORE = 255


class segment_kernel:
    """CABINET_OHEM_SEGMENT_KERNEL=1 for the duration of a block (the library reads it per call)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["CABINET_OHEM_SEGMENT_KERNEL"] = "1"

    def __exit__(self, *exc):
        if self.on:
            del os.environ["CABINET_OHEM_SEGMENT_KERNEL"]


def crit_of(thresh, n_min, w, device_select=True):
    from cabinet_amd.loss import OhemCELoss

    return OhemCELoss(thresh, n_min, IGNORE, weight=None if w is None else w.clone(), device_select=device_select).cuda()


def run_single(low, lab, w, size, thresh, n_min, device_select=True):
    x = low.cuda().requires_grad_(True)
    loss = crit_of(thresh, n_min, w, device_select).forward_upsampled(x, lab.cuda(), size)
    loss.backward()
    torch.cuda.synchronize()
    return loss, x.grad


def run_pair(low_a, w_a, low_b, w_b, lab, size, thresh, n_min, device_select=True):
    from cabinet_amd.loss import ohem_upsampled_pair

    xa, xb = low_a.cuda().requires_grad_(True), low_b.cuda().requires_grad_(True)
    loss = ohem_upsampled_pair(crit_of(thresh, n_min, w_a, device_select), xa, crit_of(thresh, n_min, w_b, device_select), xb,
                               lab.cuda(), size)
    loss.backward()
    torch.cuda.synchronize()
    return loss, xa.grad, xb.grad


# ---- 1. the selection alone against torch.sort ------------------------------------------------------------------------------

def select_reference(loss_px, lab, w, thresh, n_min):
    """-> [t, tie, denom, value] from a sort of the same fp32 l = w[label] * loss_px (value summed in float64), or the
    first-branch row; None where the head has no valid pixel."""
    valid = lab != IGNORE
    l = loss_px[valid]
    if w is not None:
        l = w[lab[valid]] * l
    n_valid = int(valid.sum())
    if n_valid == 0:
        return None
    k = min(n_min, n_valid)
    n_above = int((l > thresh).sum())
    if n_above >= k:
        return [float(np.float32(thresh)), 0.0, float(n_above), float(l[l > thresh].double().sum()) / n_above]
    s = torch.sort(l, descending=True).values
    t = s[k - 1]
    n_gt, n_eq = int((l > t).sum()), int((l == t).sum())
    value = (float(l[l > t].double().sum()) + (k - n_gt) * float(t)) / k
    return [float(t) + 0.0, (k - n_gt) / n_eq, float(k), value]


def device_select_rows(loss_px, lab, ws, thresh, n_mins):
    """loss_px (nheads,B,H,W) on the device -> sel rows, through cabinet_ohem_stats-shaped statistics built with torch."""
    from cabinet_amd.functional import ohem_select_hip

    nheads = loss_px.shape[0]
    stats = torch.zeros((nheads, 3), dtype=torch.float64, device="cuda")
    valid = lab != IGNORE
    for i in range(nheads):
        l = loss_px[i][valid]
        if ws[i] is not None:
            l = ws[i][lab[valid]] * l
        above = l > thresh
        stats[i] = torch.stack([valid.sum().double(), above.sum().double(), l[above].double().sum()])
    C = 32 if ws[0] is None else ws[0].numel()
    sel = ohem_select_hip(loss_px, lab, stats, thresh, n_mins, IGNORE, C, ws)
    again = ohem_select_hip(loss_px, lab, stats, thresh, n_mins, IGNORE, C, ws)
    torch.cuda.synchronize()
    assert torch.equal(sel, again), "two calls of the selection differ"
    return sel.cpu()


def check_rows(sel, loss_px, lab, ws, thresh, n_mins, what):
    for i in range(loss_px.shape[0]):
        ref = select_reference(loss_px[i], lab, ws[i], thresh, n_mins[i])
        row = [float(v) for v in sel[i]]
        print(f"{what} head {i}: device {row} reference {ref}")
        if ref is None:
            assert row[1] == 0.0 and row[2] == 1.0 and row[3] == 0.0      # a finite row: value 0, 1 / denom finite
            continue
        t_dev, t_ref = np.float32(row[0]), np.float32(ref[0])
        assert row[0] == float(t_dev) and t_dev.tobytes() == t_ref.tobytes(), (what, i, row[0], ref[0])   # bit-equal fp32
        assert row[1] == ref[1] and row[2] == ref[2], (what, i, row, ref)                               # n_gt, n_eq exact
        assert abs(row[3] - ref[3]) <= 1e-6 * abs(ref[3]) + 1e-300, (what, i, row[3], ref[3])


SELECT_CASES = [
    # name, (B, H, W), heads, classes weighted?, share ignored, n_min as a share of B*H*W (or an int), value scale
    ("one pixel", (1, 1, 1), 1, False, 0.0, 1, 3.0),
    ("small", (2, 37, 53), 2, False, 0.1, 1 / 16, 3.0),
    ("weighted pair", (2, 64, 96), 2, True, 0.1, 1 / 16, 3.0),
    ("k == n_valid", (1, 40, 40), 1, False, 0.25, "n_valid", 3.0),
    ("n_min > n_valid", (1, 40, 40), 2, False, 0.5, 5000, 3.0),
    ("config 3", (8, 1024, 1024), 2, False, 0.1, 1 / 16, 1e-3),
]


@pytest.mark.parametrize("case", SELECT_CASES, ids=[c[0] for c in SELECT_CASES])
def test_select_against_sort(case):
    name, (B, H, W), nheads, weighted, ign, n_min, scale = case
    g = torch.Generator().manual_seed(B * H + W)
    # any finite fp32 is a legal key: mostly tiny positive losses (late training), some negative ones (an fp32 forward can
    # produce -1e-8), exact zeros of both signs, and a thin tail of hard pixels
    loss_px = torch.rand(nheads, B, H, W, generator=g).pow(8) * scale
    loss_px[torch.rand(nheads, B, H, W, generator=g) < 0.02] *= -1e-3
    loss_px[torch.rand(nheads, B, H, W, generator=g) < 0.05] = 0.0
    loss_px[torch.rand(nheads, B, H, W, generator=g) < 0.05] = -0.0
    hard = torch.rand(nheads, B, H, W, generator=g) < 0.01
    loss_px[hard] = 5.0 + 10.0 * torch.rand(int(hard.sum()), generator=g)
    lab = torch.randint(0, 19, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < ign] = IGNORE
    ws = [None] * nheads
    if weighted:
        ws = [0.5 + 2.0 * torch.rand(19, generator=g) for _ in range(nheads)]
        ws[0][3] = 0.0
    n_valid = int((lab != IGNORE).sum())
    n_min = n_valid if n_min == "n_valid" else (n_min if isinstance(n_min, int) else max(1, int(B * H * W * n_min)))
    thresh = 4.0                                                   # 1 % of the pixels above it: the top-n_min branch
    loss_px, lab, ws = loss_px.cuda(), lab.cuda(), [None if w is None else w.cuda() for w in ws]
    sel = device_select_rows(loss_px, lab, ws, thresh, [n_min] * nheads)
    check_rows(sel, loss_px, lab, ws, thresh, [n_min] * nheads, name)
    assert all(float(sel[i, 2]) == min(n_min, n_valid) for i in range(nheads))      # every head took the order statistic


def test_select_first_branch_row_all_ignored_and_signed_zeros():
    g = torch.Generator().manual_seed(7)
    B, H, W = 2, 48, 64
    lab = torch.randint(0, 8, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    # head 0 on the first branch (half of its pixels above thresh), head 1 on the other one
    loss_px = torch.stack([torch.rand(B, H, W, generator=g) * 2.0, torch.rand(B, H, W, generator=g) * 0.5]).cuda()
    n_min = B * H * W // 16
    sel = device_select_rows(loss_px, lab.cuda(), [None, None], 0.7, [n_min, n_min])
    check_rows(sel, loss_px, lab.cuda(), [None, None], 0.7, [n_min, n_min], "mixed pair")
    assert float(sel[0, 0]) == float(np.float32(0.7)) and float(sel[0, 1]) == 0.0       # the row of stats, copied
    assert float(sel[0, 2]) == float(((loss_px[0] > 0.7) & (lab.cuda() != IGNORE)).sum())
    assert float(sel[1, 2]) == n_min
    # every pixel ignored: a finite row, nothing selected
    allign = torch.full((B, H, W), IGNORE).cuda()
    sel = device_select_rows(loss_px, allign, [None, None], 0.7, [n_min, n_min])
    check_rows(sel, loss_px, allign, [None, None], 0.7, [n_min, n_min], "all ignored")
    # the k-th value among zeros of both signs: one bucket, t reported as +0.0, the tie spread over all of them
    z = torch.zeros(1, 1, 32, 32)
    z[0, 0, ::2] = -0.0
    z[0, 0, 0, :10] = torch.arange(1, 11).float()                                        # 10 non-zero losses
    z[0, 0, 1, :5] = -1.0                                                                # and 5 below zero
    labz = torch.zeros(1, 32, 32, dtype=torch.int64)
    sel = device_select_rows(z.cuda(), labz.cuda(), [None], 100.0, [64])
    row = [float(v) for v in sel[0]]
    assert row[0] == 0.0 and np.signbit(row[0]) == False  # noqa: E712
    assert row[1] == (64 - 10) / (1024 - 15) and row[2] == 64.0 and abs(row[3] - 55.0 / 64) <= 1e-12


# ---- 2. loss and gradient against the reference's vectors --------------------------------------------------------------------

def topk_heads():
    """(id, low, labels, weight, size, n_min, thresh, loss, dlow) of every stored head on the top-n_min branch."""
    out = []
    d = fixture()
    for name in case_names(d):
        for hi in range(int(d[f"{name}.n_heads"])):
            if str(d[f"{name}.h{hi}.branch"]) == "topk":
                out.append((f"g7.{name}.h{hi}",) + load_head(d, name, hi) +
                           (float(d[f"{name}.h{hi}.loss"]), torch.from_numpy(d[f"{name}.h{hi}.dlow"])))
    d6, cases = g6_cases()
    for ci in cases:
        low, lab, w, size, n_min = g6_load(d6, ci)
        out.append((f"g6.c{ci}.topk", low, lab, w, size, n_min, float(d6[f"c{ci}.topk.thresh"]), float(d6[f"c{ci}.topk.loss"]),
                    torch.from_numpy(d6[f"c{ci}.topk.dlow"])))
    return out


@pytest.mark.parametrize("segment", [False, True], ids=["default-kernel", "segment-kernel"])
def test_top_n_min_branch_matches_the_reference(segment):
    """Single head and pair (the same head twice), weighted and not, row-kernel and segment-kernel shapes; with ``segment`` the
    row-kernel shapes run through the generic segment kernel as well."""
    for name, low, lab, w, size, n_min, thresh, ref_loss, ref_dlow in topk_heads():
        with segment_kernel(segment):
            loss, grad = run_single(low, lab, w, size, thresh, n_min)
            lossp, ga, gb = run_pair(low, w, low, w, lab, size, thresh, n_min)
        print(f"{name} segment={segment}: loss {loss.item():.9f} pair {lossp.item():.9f} ref {ref_loss:.9f}")
        assert type(loss.grad_fn).__name__ == "_OhemUpDeviceSelectedBackward"
        assert type(lossp.grad_fn).__name__ == "_OhemUpDeviceSelectedPairBackward"
        assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), name
        assert abs(lossp.item() - 2 * ref_loss) <= 1e-5 * max(1.0, abs(2 * ref_loss)), name
        assert_close(grad, ref_dlow, TOL, f"{name} dlow", atol=1e-9)
        assert_close(ga, ref_dlow, TOL, f"{name} pair dlow a", atol=1e-9)
        assert_close(gb, ref_dlow, TOL, f"{name} pair dlow b", atol=1e-9)


def test_mixed_pair_matches_the_reference_head_by_head():
    """Case c: head 0 on the top-n_min branch, head 1 on 'n_min above thresh' -- one selection sequence, one backward pair.
    The first-branch head, now through the `_sel` kernels with t = thresh and tie = 0, equals its own ``device_select=False``
    single-head result."""
    d = fixture()
    low_a, lab, w, size, n_min, thresh = load_head(d, "c", 0)
    low_b = load_head(d, "c", 1)[0]
    refs = [(float(d[f"c.h{i}.loss"]), torch.from_numpy(d[f"c.h{i}.dlow"])) for i in range(2)]
    loss, ga, gb = run_pair(low_a, w, low_b, w, lab, size, thresh, n_min)
    assert type(loss.grad_fn).__name__ == "_OhemUpDeviceSelectedPairBackward"
    total = refs[0][0] + refs[1][0]
    print(f"mixed pair: loss {loss.item():.9f} ref {total:.9f}")
    assert abs(loss.item() - total) <= 1e-5 * max(1.0, abs(total))
    assert_close(ga, refs[0][1], TOL, "c.h0 dlow", atol=1e-9)
    assert_close(gb, refs[1][1], TOL, "c.h1 dlow", atol=1e-9)
    plain_loss, plain_grad = run_single(low_b, lab, w, size, thresh, n_min, device_select=False)
    assert type(plain_loss.grad_fn).__name__ == "_OhemUpSelectedBackward"
    single_a, _ = run_single(low_a, lab, w, size, thresh, n_min)
    assert abs(loss.item() - (single_a.item() + plain_loss.item())) <= 1e-6 * abs(loss.item())
    assert_close(gb, plain_grad, 1e-6, "first-branch head through the _sel kernels", atol=1e-12)
    print("first-branch head through the _sel kernels bit-equal to the host-threshold kernels:", torch.equal(gb, plain_grad))


# ---- 3. against the composite path: the same numbers, and the composite path did NOT run ------------------------------------

@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("ci", [0, 1])
def test_device_selection_replaces_the_composite_path(ci, pair):
    """The g6 ``topk`` cases have a clean gap at the k-th value (1.1e-2 and 3.2e-4): both paths keep the same pixels."""
    from cabinet_amd.loss import ohem_upsampled_pair

    d6, _ = g6_cases()
    low, lab, w, size, n_min = g6_load(d6, ci)
    thresh = float(d6[f"c{ci}.topk.thresh"])
    ca, cb = crit_of(thresh, n_min, w), crit_of(thresh, n_min, w)
    x, x2, y = (low.cuda().requires_grad_(True) for _ in range(3))
    labc = lab.cuda()
    loss = ohem_upsampled_pair(ca, x, cb, x2, labc, size) if pair else ca.forward_upsampled(x, labc, size)
    assert type(loss.grad_fn).__name__ == ("_OhemUpDeviceSelectedPairBackward" if pair else "_OhemUpDeviceSelectedBackward")
    loss.backward()
    want = ca.forward(F.interpolate(y, size=size, mode="bilinear", align_corners=False), labc)     # the composite path
    want.backward()
    torch.cuda.synchronize()
    nh = 2 if pair else 1
    print(f"g6.c{ci} pair={pair}: loss {loss.item():.9f} composite {nh * want.item():.9f} "
          f"grad rel {float((x.grad - y.grad).norm() / y.grad.norm()):.3e}")
    assert abs(loss.item() - nh * want.item()) <= 1e-6 * abs(nh * want.item())
    assert_close(x.grad, y.grad, 1e-5, "dlow vs composite", atol=1e-9)
    if pair:
        assert_close(x2.grad, y.grad, 1e-5, "dlow b vs composite", atol=1e-9)


# ---- 4. the common case is untouched ----------------------------------------------------------------------------------------

def test_first_branch_inputs_are_bit_identical_with_the_option_on():
    """With at least n_min pixels above thresh the host read still picks today's Functions: same bits, loss and gradient."""
    d6, cases = g6_cases()
    for ci in cases:
        low, lab, w, size, n_min = g6_load(d6, ci)
        thresh = float(d6[f"c{ci}.sel.thresh"])
        res = []
        for ds in (False, True):
            ls, gs = run_single(low, lab, w, size, thresh, n_min, device_select=ds)
            lp, ga, gb = run_pair(low, w, low.flip(0).contiguous(), None, lab, size, thresh, n_min, device_select=ds)
            assert type(ls.grad_fn).__name__ == "_OhemUpSelectedBackward" and type(lp.grad_fn).__name__ == "_OhemUpSelectedPairBackward"
            res.append((ls.detach(), gs, lp.detach(), ga, gb))
        assert all(torch.equal(a, b) for a, b in zip(*res))


# ---- 5. reproducible ----------------------------------------------------------------------------------------------------------

def test_backward_twice_is_bit_identical():
    """No float atomics anywhere on the branch (the composite path's upsample backward adds with atomics)."""
    for name, low, lab, w, size, n_min, thresh, _, _ in topk_heads():
        a = run_pair(low, w, low.flip(0).contiguous(), w, lab, size, thresh, n_min)
        b = run_pair(low, w, low.flip(0).contiguous(), w, lab, size, thresh, n_min)
        s1, s2 = run_single(low, lab, w, size, thresh, n_min), run_single(low, lab, w, size, thresh, n_min)
        assert all(torch.equal(u.detach(), v.detach()) for u, v in zip(a + s1, b + s2)), name


# ---- 6. GraphedTrainStep: graph B-any ----------------------------------------------------------------------------------------

LN8 = float(np.log(8.0))   # -log(max softmax) < ln 8 for 8 classes: a threshold no pixel labelled with the net's own argmax reaches


def _build(device_select, graphed, capture_optimizer=False):
    from cabinet_amd.train import GraphedTrainStep, TrainStep, build_model, make_criteria

    net = build_model("small", n_classes=8, seed=0, gamma=0.5, device="cuda").train()
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-2, momentum=0.9)
    crit = make_criteria(2, 256, 256, "cuda", thresh=LN8, device_select=device_select)
    if graphed:
        return net, GraphedTrainStep(net, crit, optimizer=opt, warmup=1, capture_optimizer=capture_optimizer,
                                     device_select=device_select)
    return net, TrainStep(net, crit, optimizer=opt)


def _own_argmax_labels(net, im):
    """Labels = the main head's own prediction on this batch in the net's CURRENT state (a throw-away copy: no BatchNorm side
    effect): every pixel of that head then has loss < ln 8, n_above = 0, the top-n_min branch -- while the auxiliary head, for
    which these labels are as good as random, stays on 'n_min above thresh': a mixed pair."""
    with torch.no_grad():
        low, _ = copy.deepcopy(net).forward_lowres(im)
        return F.interpolate(low.float(), size=im.shape[2:], mode="bilinear", align_corners=False).argmax(1)


def _eager_reference(kinds):
    """TrainStep with the SAME criteria as the graphed step (``device_select=True``: the eager step gets the feature through
    the criteria) over batches of the given kinds, as test_graphed_train_step_equals_eager compares one set of criteria run two
    ways: what then differs between the runs is what differs there (capture and replay, stock kernels with atomics), and that
    test's tolerances are the ones derived for it.  The kernels against the composite path are compared directly above (3.);
    through SGD steps on own-argmax labels, which reinforce themselves, their 1e-5 difference would be a second, amplified
    source of divergence that those tolerances do not price.  The labels of the 'O' batches are made on the fly and handed to
    the graphed runs."""
    from cabinet_amd.train import synthetic_batch

    from cabinet_amd.loss import fused_pair_launch

    net, step = _build(True, False)
    batches, losses = [], []
    for i, kind in enumerate(kinds):
        im, lb = synthetic_batch(2, 256, 256, 8, "cuda", seed=60 + i)
        if kind == "O":
            lb = _own_argmax_labels(net, im)
        elif kind == "I":
            lb = torch.full_like(lb, IGNORE)
        if kind != "I":   # the batch is of its kind: the forward statistics of a throw-away copy of the net in this state
            with torch.no_grad():
                low, low16 = copy.deepcopy(net).forward_lowres(im)
                host = fused_pair_launch(step.crit_p, low, step.crit_16, low16, lb, tuple(im.shape[2:])).stats.tolist()
            on_first = [int(h[1]) >= min(step.crit_p.n_min, int(h[0])) for h in host]
            print(f"batch {i} kind {kind}: [n_valid, n_above, sum] per head {host}")
            assert on_first == ([True, True] if kind == "F" else [False, True]), (kind, host)
        batches.append((im, lb))
        losses.append(float(step(im, lb)))
    return batches, losses, {k: v.clone() for k, v in net.state_dict().items()}


def _compare(la, lb_, sa, sb):
    # the tolerances of test_graphed_train_step_equals_eager (stock backward kernels with atomics differ run to run); a
    # capture bug -- a stale buffer, gradients accumulated across the two backward graphs, a wrong branch -- is an O(1) error
    for x, y in zip(la, lb_):
        assert abs(x - y) <= 1e-4 * max(1.0, abs(x)), (la, lb_)
    for k in sa:
        assert_close(sb[k].double(), sa[k].double(), 2e-3, k, atol=1e-5)


@pytest.mark.parametrize("capture_optimizer", [False, True])
def test_graphed_train_step_with_device_select_equals_eager(capture_optimizer):
    kinds = ["F", "O", "F", "O", "I", "O", "F"]           # first-branch, other-branch (mixed pair), all-ignored
    batches, ref_losses, ref_state = _eager_reference(kinds)
    net, step = _build(True, True, capture_optimizer)
    losses = [float(step(*b)) for b in batches]
    print("eager  ", ref_losses)
    print("graphed", losses)
    assert step.g_any is not None and step.g_bwd is not None
    assert step.fallbacks == 1                             # the all-ignored batch only
    assert step.device_selected == 3                       # the three other-branch batches went through graph B-any
    assert losses[4] == 0.0 and ref_losses[4] == 0.0
    _compare(ref_losses, losses, ref_state, {k: v for k, v in net.state_dict().items()})


def test_capture_on_an_other_branch_batch():
    """Recording executes nothing, so the branch of the capture batch does not matter with the option on; without it the
    capture still refuses such a batch."""
    kinds = ["O", "F", "O"]
    batches, ref_losses, ref_state = _eager_reference(kinds)
    net, step = _build(True, True)
    losses = [float(step(*b)) for b in batches]
    assert step.g_any is not None and step.fallbacks == 0 and step.device_selected == 1   # the first step ran eagerly
    _compare(ref_losses, losses, ref_state, {k: v for k, v in net.state_dict().items()})
    _, plain = _build(False, True)
    with pytest.raises(RuntimeError, match="capture batch does not take"):
        plain(*batches[0])


# ---- 7. half precision / autocast computes in fp32 ----------------------------------------------------------------------------

def test_half_precision_under_autocast_computes_in_fp32(monkeypatch):
    from cabinet_amd import functional as Fn
    from cabinet_amd.loss import ohem_upsampled_pair

    d = fixture()
    low, lab, w, size, n_min, thresh = load_head(d, "b", 0)
    low = low.half().float()         # the values a half tensor can hold
    w = w.half().float()
    seen = []
    real_ptr = Fn._ptr

    def spy(t):
        if t is not None:
            seen.append(t.dtype)
        return real_ptr(t)

    monkeypatch.setattr(Fn, "_ptr", spy)
    out = {}
    for tag in ("fp32", "half"):
        ca, cb = crit_of(thresh, n_min, w), crit_of(thresh, n_min, w)
        xa, xb, xs = (low.cuda().requires_grad_(True) for _ in range(3))
        if tag == "half":
            ca, cb = ca.half(), cb.half()
            assert ca.weight.dtype == torch.float16 and ca.device_select
        seen.clear()
        with torch.autocast("cuda", dtype=torch.float16, enabled=(tag == "half")):
            lp = ohem_upsampled_pair(ca, xa, cb, xb, lab.cuda(), size)
            ls = ca.forward_upsampled(xs, lab.cuda(), size)
            (lp + ls).backward()
        torch.cuda.synchronize()
        assert "_OhemUpDeviceSelectedPair" in type(lp.grad_fn).__name__ and "_OhemUpDeviceSelected" in type(ls.grad_fn).__name__
        floating = [dt for dt in seen if dt.is_floating_point]
        assert len(seen) > 20 and set(floating) <= {torch.float32, torch.float64}, set(seen)
        assert lp.dtype == torch.float32 and xa.grad.dtype == torch.float32
        out[tag] = (lp.detach(), ls.detach(), xa.grad, xb.grad, xs.grad)
    assert all(torch.equal(a, b) for a, b in zip(out["fp32"], out["half"]))
