"""The fused evaluation tail (csrc/eval_tail.hip) on the GPU: each kernel through the C ABI against a float64 torch computation
of its contract, then cabinet_amd.evaluate.MscEvalV0(fused=True) against the reference's evaluator (fixture g5_eval*.npz) and
against the plain path on the real network.  Near-tie rule: tests/test_evaluate.py.  Every test runs once."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from eval_golden import CASES, MAX_UNDECIDED_SHARE, check_against_case, hist_of, load_case, write_record

pytestmark = pytest.mark.gpu


def _up(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


def _chip_oracle(dst0, a, b, size, origin, rcy, rcx):
    """float64: dst[window] += rcp_y (x) rcp_x * mean over {chip, mirrored chip} of softmax(upsample(logits))."""
    (ch, cw), (y0, x0) = size, origin
    p = torch.softmax(_up(a.double(), size), dim=1)
    if b is not None:
        p = (p + torch.softmax(torch.flip(_up(b.double(), size), dims=(3,)), dim=1)) * 0.5
    ry = rcy.double()[y0:y0 + ch] if rcy is not None else torch.ones(ch, dtype=torch.float64)
    rx = rcx.double()[x0:x0 + cw] if rcx is not None else torch.ones(cw, dtype=torch.float64)
    out = dst0.double().clone()
    out[:, :, y0:y0 + ch, x0:x0 + cw] += p * ry.view(1, 1, -1, 1) * rx.view(1, 1, 1, -1)
    return out


# C, (hl, wl), (ch, cw): factor 1, the model's x8, a non-integer ratio, a 1024-wide row (four segments), a shrinking resize
_CHIP_SHAPES = [
    (1, (24, 40), (24, 40)), (8, (24, 40), (24, 40)), (19, (20, 300), (20, 300)), (32, (24, 40), (24, 40)),
    (1, (4, 6), (32, 48)), (8, (16, 16), (128, 128)), (19, (3, 128), (24, 1024)), (32, (6, 40), (48, 320)),
    (1, (13, 17), (100, 131)), (8, (13, 17), (100, 131)), (19, (13, 17), (100, 131)), (32, (13, 17), (100, 131)),
    (5, (13, 17), (100, 131)), (8, (40, 60), (25, 33)),
]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("C,low,chip", _CHIP_SHAPES)
def test_chip_accum_vs_float64(C, low, chip, flip):
    from cabinet_amd.functional import eval_chip_accum, eval_chip_accum_supported

    g = torch.Generator().manual_seed(C * 1000 + chip[1])
    N, (ch, cw) = 2, chip
    FH, FW = ch + 37, cw + 23
    a = torch.randn(N, C, *low, generator=g) * 3.0
    b = torch.randn(N, C, *low, generator=g) * 3.0 if flip else None
    rcy = 1.0 / torch.randint(1, 4, (FH,), generator=g).float()
    rcx = 1.0 / torch.randint(1, 4, (FW,), generator=g).float()
    assert eval_chip_accum_supported(a.cuda(), chip, flip)
    worst = 0.0
    # the four corners of the larger destination, then an interior window without the reciprocal vectors
    for i, origin in enumerate([(0, 0), (0, FW - cw), (FH - ch, 0), (FH - ch, FW - cw), (17, 11)]):
        dst0 = torch.rand(N, C, FH, FW, generator=g)
        ry, rx = (rcy, rcx) if i < 4 else (None, None)
        dst = dst0.cuda()
        eval_chip_accum(dst, a.cuda(), b.cuda() if flip else None, chip, origin, ry.cuda() if ry is not None else None,
                        rx.cuda() if rx is not None else None)
        torch.cuda.synchronize()
        want = _chip_oracle(dst0, a, b, chip, origin, ry, rx)
        got = dst.cpu()
        outside = torch.ones(FH, FW, dtype=torch.bool)
        outside[origin[0]:origin[0] + ch, origin[1]:origin[1] + cw] = False
        assert torch.equal(got[:, :, outside], dst0[:, :, outside]), "a value outside the window changed"
        err = float((got.double() - want).abs().max())
        worst = max(worst, err)
        # fp32 source indices carry ~1e-5 of a pixel at these sizes: 1e-4 per tensor; at factor 1 nothing is interpolated
        assert_close(got, want, 1e-4, f"chip_accum C={C} {low}->{chip} flip={flip} origin={origin}", atol=0)
        if low == chip:
            assert err < 2e-6
    print(f"chip_accum C={C} {low}->{chip} flip={flip}: max abs error {worst:.3e}")


@pytest.mark.parametrize("C,src,crop,out", [
    (1, (40, 56), None, (40, 56)),                       # same size: exact
    (8, (128, 200), (16, 112, 0, 200), (96, 200)),       # the padding branch: crop rows, same size
    (19, (120, 168), None, (160, 224)),                  # scale 0.75 back up
    (8, (240, 336), None, (160, 224)),                   # scale 1.5 back down
    (32, (50, 67), (3, 47, 5, 60), (61, 131)),           # odd sizes, W % 4 != 0
    (19, (128, 128), (40, 88, 32, 96), (96, 128)),       # scaled image smaller than the crop in both axes
])
def test_scale_merge_vs_float64(C, src, crop, out):
    from cabinet_amd.functional import eval_scale_merge

    g = torch.Generator().manual_seed(C + out[1])
    N = 2
    prob = torch.rand(N, C, *src, generator=g)
    total0 = torch.rand(N, C, *out, generator=g) * 2
    hst, hed, wst, wed = crop if crop is not None else (0, src[0], 0, src[1])
    want = total0.double() + _up(prob.double()[:, :, hst:hed, wst:wed], out)
    total = total0.cuda()
    eval_scale_merge(total, prob.cuda(), crop)
    torch.cuda.synchronize()
    err = float((total.cpu().double() - want).abs().max())
    print(f"scale_merge C={C} {src}{crop}->{out}: max abs error {err:.3e}")
    assert_close(total, want, 1e-5, "scale_merge", atol=0)
    if (hed - hst, wed - wst) == out:
        assert err < 5e-7


def _argmax_hist_plan(N, H, W):
    """eval_argmax_hist_run (eval_tail.hip:290-311) -> (VEC, groups, workgroups): VEC pixels per thread, at most 512 workgroups of
    256 threads that stride over the groups."""
    vec = 4 if (H * W) % 4 == 0 else 1
    groups = N * (H * W // vec)
    return vec, groups, min(-(-groups // 256), 512)


# the last two cross the cap of 512 workgroups (more than 512 * 256 groups): the second trip of the kernel's strided loop, with
# VEC = 4 and -- P odd -- with VEC = 1
@pytest.mark.parametrize("C,H,W", [(1, 16, 24), (8, 96, 200), (19, 61, 131), (32, 64, 64), (8, 728, 728), (19, 363, 363)])
def test_argmax_hist_ties_clip_ignore(C, H, W):
    from cabinet_amd.functional import eval_argmax_hist

    g = torch.Generator().manual_seed(C + W)
    N = 2
    if H >= 363:
        vec, groups, wgs = _argmax_hist_plan(N, H, W)
        assert vec == (4 if H == 728 else 1) and groups > 512 * 256 and wgs == 512
        assert _argmax_hist_plan(1, H, W)[1] == (132496 if H == 728 else 131769) > 512 * 256   # one image alone crosses it
    total = torch.rand(N, C, H, W, generator=g)
    if C >= 8:  # exact ties: the same maximal value in two (three) classes, the lowest index must win
        tie = torch.rand(N, H, W, generator=g) < 0.2
        top = total.max(dim=1).values + 1.0
        total[:, 5][tie] = top[tie]
        total[:, 2][tie] = top[tie]
        tie3 = tie & (torch.rand(N, H, W, generator=g) < 0.3)
        total[:, 7][tie3] = top[tie3]
    labels = torch.randint(0, C, (N, H, W), generator=g)
    r = torch.rand(N, H, W, generator=g)
    labels[r < 0.1] = 255
    labels[(r >= 0.1) & (r < 0.12)] = 200
    labels[(r >= 0.12) & (r < 0.13)] = -3
    hist = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    pred = eval_argmax_hist(total.cuda(), labels.cuda(), hist, 255, want_pred=True)
    torch.cuda.synchronize()
    want_pred = torch.argmax(total, dim=1)
    if C >= 8:
        assert bool((want_pred[tie] == 2).all())
    assert pred.dtype == torch.uint8 and torch.equal(pred.cpu().long(), want_pred)
    keep = labels != 255
    idx = pred.cpu().long()[keep].numpy() * C + labels[keep].clamp(0, C - 1).numpy()
    want = np.bincount(idx, minlength=C * C).reshape(C, C)
    assert np.array_equal(hist.cpu().numpy(), want)
    # a second call accumulates; without the prediction pointer nothing else changes
    assert eval_argmax_hist(total.cuda(), labels.cuda(), hist, 255) is None
    assert np.array_equal(hist.cpu().numpy(), 2 * want)
    # all labels ignored: the matrix stays zero
    zero = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    eval_argmax_hist(total.cuda(), torch.full((N, H, W), 255, dtype=torch.int64, device="cuda"), zero, 255)
    assert int(zero.abs().sum()) == 0


_RECORD = {"fused": {}, "plain_gpu": {}}


def _gpu_evaluator(g, fused):
    from cabinet_amd.evaluate import MscEvalV0

    return MscEvalV0(g["model"].cuda(), [(g["image"], g["labels"])], g["n_classes"], ignore_label=g["ignore_label"],
                     scales=g["scales"], flip=g["flip"], cropsize=g["cropsize"], fused=fused)


@pytest.mark.parametrize("case", CASES)
def test_fused_evaluator_matches_the_reference(case):
    from cabinet_amd import functional as fn

    g = load_case(case)
    ev = _gpu_evaluator(g, True)
    probs = ev.summed_probabilities(g["image"])
    hist = torch.zeros(g["n_classes"], g["n_classes"], dtype=torch.int64, device="cuda")
    pred = fn.eval_argmax_hist(probs, g["labels"].cuda(), hist, g["ignore_label"], want_pred=True)
    res = ev.evaluate()
    assert np.array_equal(res["confusion_matrix"], hist.cpu().numpy().astype(np.float64))
    check_against_case(g, probs, pred.cpu().numpy(), res, f"fused_case{case}", _RECORD["fused"])
    write_record(_RECORD["fused"], "fused_gpu")


@pytest.mark.parametrize("case", CASES)
def test_plain_path_on_the_gpu_matches_the_reference(case):
    g = load_case(case)
    ev = _gpu_evaluator(g, False)
    probs = ev.summed_probabilities(g["image"])
    res = ev.evaluate()
    check_against_case(g, probs, torch.argmax(probs, dim=1).cpu().numpy(), res, f"plain_gpu_case{case}", _RECORD["plain_gpu"])
    write_record(_RECORD["plain_gpu"], "plain_gpu")


class _TupleOut(torch.nn.Module):
    """Any model is served: only ``model(x)[0]`` is required (no ``forward_lowres``)."""

    def __init__(self, n_classes):
        super().__init__()
        self.net = torch.nn.Conv2d(3, n_classes, 3, padding=1)

    def forward(self, x):
        return (self.net(x),)


def test_auto_mode_takes_the_fused_path_and_true_raises_on_unsupported(monkeypatch):
    from cabinet_amd import functional as fn
    from cabinet_amd.evaluate import MscEvalV0

    g = load_case(4)
    calls = []
    real = fn.eval_chip_accum
    monkeypatch.setattr(fn, "eval_chip_accum", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    auto = _gpu_evaluator(g, None).evaluate()
    assert calls, "fused=None on a GPU model with supported shapes must run the HIP kernels"
    assert np.array_equal(auto["confusion_matrix"], _gpu_evaluator(g, True).evaluate()["confusion_matrix"])
    # a model without forward_lowres: its full-resolution logits are "low resolution at factor 1"
    torch.manual_seed(3)
    data = [(torch.randn(1, 3, 40, 56), torch.randint(0, 8, (1, 40, 56)))]
    m8 = _TupleOut(8).cuda()
    n = len(calls)
    f1 = MscEvalV0(m8, data, 8, cropsize=32, flip=True, fused=True).evaluate()
    assert len(calls) > n
    p1 = MscEvalV0(m8, data, 8, cropsize=32, flip=True, fused=False).evaluate()
    assert np.abs(f1["confusion_matrix"] - p1["confusion_matrix"]).sum() <= 4   # random logits: a near-tie or two at most
    # 40 classes: outside the kernels' coverage.  None falls back to the plain path, True raises.
    m40 = _TupleOut(40).cuda()
    data = [(torch.randn(1, 3, 32, 32), torch.randint(0, 40, (1, 32, 32)))]
    n = len(calls)
    res = MscEvalV0(m40, data, 40, cropsize=32).evaluate()
    assert len(calls) == n and res["confusion_matrix"].sum() == 32 * 32
    with pytest.raises(RuntimeError, match="32"):
        MscEvalV0(m40, data, 40, cropsize=32, fused=True).evaluate()


def _real_net(weight_scale):
    from cabinet_amd.train import build_model

    net = build_model("small", n_classes=8, seed=0, gamma=0.5)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2, generator=gen)
                m.running_var.uniform_(0.5, 1.5, generator=gen)
        net.conv_out.conv_out.weight.mul_(weight_scale)
    return net.cuda().eval()


def test_fused_vs_plain_on_the_real_network():
    """Plain-on-GPU fp32 is the yardstick here.  Undecided pixels: plain's own top-two margin below the TIE of fixture case 4 (the
    same class count, scales and flip).  A freshly initialised network has flat logits, so the classifier's weights are scaled
    (x1, x4, x16, ...) until the PLAIN path alone leaves at most 0.2 % of the pixels undecided; the fused path is run once."""
    from cabinet_amd import functional as fn
    from cabinet_amd.evaluate import MscEvalV0

    tie = load_case(4)["tie"]
    g = torch.Generator().manual_seed(21)
    image = torch.randn(2, 3, 320, 448, generator=g)
    labels = torch.randint(0, 8, (2, 320, 448), generator=g)
    labels[torch.rand(2, 320, 448, generator=g) < 0.1] = 255
    kw = dict(scales=(0.75, 1.0), flip=True, cropsize=256)
    for scale in (1.0, 4.0, 16.0, 64.0, 256.0):
        net = _real_net(scale)
        plain = MscEvalV0(net, [(image, labels)], 8, fused=False, **kw)
        p = plain.summed_probabilities(image)
        top2 = torch.topk(p, 2, dim=1).values
        undecided = (top2[:, 0] - top2[:, 1]) < tie
        share = float(undecided.float().mean())
        print(f"classifier weights x{scale:g}: plain path leaves {share:.3e} of the pixels undecided (tie {tie:.3e})")
        if share <= MAX_UNDECIDED_SHARE:
            break
    assert share <= MAX_UNDECIDED_SHARE
    fused = MscEvalV0(net, [(image, labels)], 8, fused=True, **kw)
    q = fused.summed_probabilities(image)
    rel = float((q - p).double().norm() / p.double().norm())
    maxabs = float((q - p).abs().max())
    hist = torch.zeros(8, 8, dtype=torch.int64, device="cuda")
    pred_f = fn.eval_argmax_hist(q, labels.cuda(), hist, 255, want_pred=True).long()
    pred_p = torch.argmax(p, dim=1)
    wrong = int(((pred_f != pred_p) & ~undecided).sum())
    print(f"fused vs plain on CABiNet-Small: rel {rel:.3e}  max abs {maxabs:.3e}  decided pixels differing {wrong}")
    assert rel <= 1e-3
    assert wrong == 0
    rp, rf = plain.evaluate(), fused.evaluate()
    und, lab = undecided.cpu().numpy(), labels.numpy()
    assert np.array_equal(hist_of(pred_f.cpu().numpy(), lab, und, 8, 255), hist_of(pred_p.cpu().numpy(), lab, und, 8, 255))
    assert np.array_equal(rf["confusion_matrix"], hist.cpu().numpy().astype(np.float64))
    assert np.abs(rp["confusion_matrix"] - rf["confusion_matrix"]).sum() <= 2 * int((und & (lab != 255)).sum())
    # integer accumulation: a second run gives the identical matrix
    assert np.array_equal(fused.evaluate()["confusion_matrix"], rf["confusion_matrix"])


def test_direct_accumulation_and_merge_route_agree():
    """At scale 1.0 without padding the chips accumulate straight into the total; the same map through a per-scale buffer and
    the merge kernel (a same-size resize: every weight is 0 or 1) differs by fp32 rounding of the sums only."""
    g = load_case(3)
    ev = _gpu_evaluator(g, True)
    ev.scales = (1.0,)
    with torch.no_grad():
        direct = ev._summed_probs(g["image"].cuda(), use_shortcut=True)[0]
        merged = ev._summed_probs(g["image"].cuda(), use_shortcut=False)[0]
    err = float((direct - merged).abs().max())
    print(f"direct vs merge route: max abs difference {err:.3e}")
    assert err <= 4 * 2 ** -24   # probabilities <= 1 summed in another order: a few ulp of 1
    assert float(direct.sum(dim=1).sub(1).abs().max()) < 1e-5   # one scale: every pixel's probabilities sum to one
