"""The inference tail (csrc/predict_tail.hip) on the GPU: each kernel through the C ABI against a torch / numpy computation of its
contract, guard bands around every byte output, then cabinet_amd.predict (infer_image, Predictor eager and graphed) against the
reference's infer_image (fixture g7_predict.npz) and against the plain path on the real network.  Every test runs once."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eval_golden import MAX_UNDECIDED_SHARE, TIE_FACTOR
from eval_golden import load_case as load_eval_case
from predict_golden import CASES, load_case, load_render, render_contract

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _guarded(shape, offset, pad=64):
    """A dense uint8 view of `shape`, `offset` bytes into a buffer filled with GUARD, and the buffer."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + pad,), GUARD, dtype=torch.uint8, device="cuda")
    return buf[offset:offset + n].view(*shape), buf


def _assert_guard(buf, offset, n, what):
    b = buf.cpu().numpy()
    assert (b[:offset] == GUARD).all() and (b[offset + n:] == GUARD).all(), f"{what}: a byte outside the tensor changed"


# C, (hl, wl), (H, W): factor 1, the model's x8, non-integer ratios, a 1024-wide row, a shrinking resize, degenerate sizes
_UP_SHAPES = [
    (1, (24, 40), (24, 40)), (8, (24, 40), (24, 40)), (19, (20, 300), (20, 300)), (32, (24, 40), (24, 40)),
    (5, (4, 6), (32, 48)), (8, (16, 16), (128, 128)), (19, (3, 128), (24, 1024)), (32, (6, 40), (48, 320)),
    (2, (13, 17), (100, 131)), (8, (13, 17), (100, 131)), (19, (13, 17), (100, 131)), (32, (13, 17), (100, 131)),
    (5, (13, 17), (100, 130)), (8, (40, 60), (25, 33)), (19, (1, 1), (1, 3)), (19, (2, 3), (5, 1)), (8, (5, 9), (33, 70)),
]


@pytest.mark.parametrize("C,low,out", _UP_SHAPES)
def test_up_argmax_vs_float64(C, low, out):
    """Reference: float64 F.interpolate + argmax.  e32 = max-abs distance of torch's CPU fp32 resize from the float64 one (the
    reference's own error); a pixel is undecided when its float64 top-two margin is below TIE_FACTOR x e32 (at ratio 1 e32 = 0:
    exact match).  Every decided pixel must match; at most 0.2 % may be undecided."""
    from cabinet_amd.functional import predict_up_argmax, predict_up_argmax_supported

    g = torch.Generator().manual_seed(C * 1000 + out[1])
    N = 2
    a = torch.randn(N, C, *low, generator=g) * 3.0
    up64 = F.interpolate(a.double(), size=out, mode="bilinear", align_corners=False)
    up32 = F.interpolate(a, size=out, mode="bilinear", align_corners=False)
    e32 = float((up32.double() - up64).abs().max())
    want = torch.argmax(up64, dim=1)
    if C > 1:
        top2 = torch.topk(up64, 2, dim=1).values
        undecided = (top2[:, 0] - top2[:, 1]) < TIE_FACTOR * e32
    else:
        undecided = torch.zeros_like(want, dtype=torch.bool)
    share = float(undecided.float().mean())
    ref_wrong = int(((torch.argmax(up32, dim=1) != want) & ~undecided).sum())
    assert predict_up_argmax_supported(a.cuda(), out)
    got = predict_up_argmax(a.cuda(), out)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, *out)
    wrong = int(((got.cpu().long() != want) & ~undecided).sum())
    print(f"up_argmax C={C} {low}->{out}: e32 {e32:.3e}  undecided {int(undecided.sum())} px ({share:.3e})  decided pixels "
          f"differing: kernel {wrong}, torch fp32 {ref_wrong}")
    if low == out:
        assert e32 == 0.0 and not undecided.any()
    assert share <= MAX_UNDECIDED_SHARE
    assert wrong == 0


def test_up_argmax_ties_take_the_lowest_index():
    from cabinet_amd.functional import predict_up_argmax

    a = torch.zeros(1, 19, 5, 7)
    a[:, 3] = 1.0
    a[:, 11] = 1.0   # equal planes stay equal under any resize: class 3 everywhere
    assert (predict_up_argmax(a.cuda(), (40, 56)).cpu() == 3).all()
    assert (predict_up_argmax(torch.zeros(2, 6, 4, 4).cuda(), (9, 13)).cpu() == 0).all()


@pytest.mark.parametrize("C", [1, 5, 8, 19, 32])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 131, 1024])
def test_argmax_equals_torch(C, W):
    from cabinet_amd.functional import predict_argmax

    g = torch.Generator().manual_seed(C * 10000 + W)
    N, H = 2, 5 if W < 1024 else 3
    t = torch.randn(N, C, H, W, generator=g)
    if C > 1:
        # planted ties: the maximum copied into 2-3 classes, class 0 and class C - 1 among them
        mx = t.max(dim=1).values
        r = torch.rand(N, H, W, generator=g)
        for lo, hi, classes in ((0.0, 0.15, (0, C - 1)), (0.15, 0.3, (C - 1, C // 2)), (0.3, 0.45, (0, C // 2, C - 1))):
            m = (r >= lo) & (r < hi)
            for c in classes:
                t[:, c][m] = mx[m]
    t = t.cuda()
    got = predict_argmax(t)
    want = torch.argmax(t, dim=1)
    assert got.dtype == torch.uint8 and torch.equal(got.long(), want)


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
def test_render_equals_the_reference(alpha):
    from cabinet_amd.functional import predict_render
    from cabinet_amd.predict import CITYSCAPES_COLORS

    r = load_render()
    pal = torch.from_numpy(CITYSCAPES_COLORS.copy()).cuda()
    labels = torch.from_numpy(r["labels"])[None].cuda()
    image = torch.from_numpy(r["image"])[None].cuda()
    out = predict_render(labels, image, pal, r["mean"], r["std"], alpha)
    want = render_contract(r["labels"], r["image"], CITYSCAPES_COLORS, r["mean"], r["std"], alpha)
    if alpha == 0.6:   # the reference's own bytes (tests/test_predict.py ties render_contract to them as well)
        want = {k: r[k] for k in ("pred", "input", "overlay")}
    for name in ("pred", "input", "overlay"):
        assert out[name].dtype == torch.uint8 and np.array_equal(out[name][0].cpu().numpy(), want[name]), name
    if alpha == 0.0:
        assert torch.equal(out["overlay"], out["input"])
    if alpha == 1.0:
        assert torch.equal(out["overlay"], out["pred"])


def test_render_optional_outputs_and_short_palette():
    from cabinet_amd.functional import predict_render
    from cabinet_amd.predict import CITYSCAPES_COLORS

    r = load_render()
    labels = torch.from_numpy(r["labels"])[None].cuda()
    image = torch.from_numpy(r["image"])[None].cuda()
    pal = torch.from_numpy(CITYSCAPES_COLORS.copy()).cuda()
    only = predict_render(labels, None, pal)
    assert sorted(only) == ["pred"] and np.array_equal(only["pred"][0].cpu().numpy(), r["pred"])
    no_overlay = predict_render(labels, image, pal, want_overlay=False)
    assert sorted(no_overlay) == ["input", "pred"] and np.array_equal(no_overlay["input"][0].cpu().numpy(), r["input"])
    no_input = predict_render(labels, image, pal, want_input=False)
    assert sorted(no_input) == ["overlay", "pred"] and np.array_equal(no_input["overlay"][0].cpu().numpy(), r["overlay"])
    # n_colors below the largest label: clipped to the palette's last colour; a batch of two (the vector path: H * W % 4 == 0)
    short = CITYSCAPES_COLORS[:7]
    lab2 = torch.from_numpy(np.stack([r["labels"][:, :92], r["labels"][::-1, :92]]).copy()).cuda()
    img2 = torch.from_numpy(np.stack([r["image"][:, :, :92], r["image"][:, ::-1, 1:]]).copy()).cuda()
    out = predict_render(lab2, img2, torch.from_numpy(short.copy()).cuda(), r["mean"], r["std"], 0.3)
    want = render_contract(lab2.cpu().numpy(), img2.cpu().numpy(), short, r["mean"], r["std"], 0.3)
    for name in ("pred", "input", "overlay"):
        assert np.array_equal(out[name].cpu().numpy(), want[name]), name


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_guard_bands(offset):
    """Every uint8 output sits `offset` bytes into a larger buffer filled with 0xA5: nothing outside it may change, and the
    bytes inside equal those of an ordinary call.  Widths 1, 3, 93, 131 (rows that start off a dword) and 4-multiples."""
    from cabinet_amd.functional import predict_argmax, predict_render, predict_up_argmax
    from cabinet_amd.predict import CITYSCAPES_COLORS

    g = torch.Generator().manual_seed(offset)
    pal = torch.from_numpy(CITYSCAPES_COLORS.copy()).cuda()
    for C, low, (H, W) in [(19, (2, 3), (5, 1)), (8, (3, 2), (7, 3)), (19, (9, 12), (70, 93)), (5, (13, 17), (100, 131)),
                           (8, (4, 6), (32, 48))]:
        N = 2
        a = (torch.randn(N, C, *low, generator=g) * 3.0).cuda()
        out, buf = _guarded((N, H, W), offset)
        assert predict_up_argmax(a, (H, W), out=out) is out
        _assert_guard(buf, offset, N * H * W, f"up_argmax {W=}")
        assert torch.equal(out, predict_up_argmax(a, (H, W)))
        t = torch.randn(N, C, H, W, generator=g).cuda()
        out2, buf2 = _guarded((N, H, W), offset)
        predict_argmax(t, out=out2)
        _assert_guard(buf2, offset, N * H * W, f"argmax {W=}")
        assert torch.equal(out2.long(), torch.argmax(t, dim=1))
        image = torch.randn(N, 3, H, W, generator=g).cuda()
        views = {k: _guarded((N, H, W, 3), offset) for k in ("pred", "input", "overlay")}
        res = predict_render(out, image, pal, alpha=0.6, out={k: v[0] for k, v in views.items()})   # labels off a dword, too
        plain = predict_render(out.clone(), image, pal, alpha=0.6)
        for k, (view, vbuf) in views.items():
            _assert_guard(vbuf, offset, N * H * W * 3, f"render {k} {W=}")
            assert res[k] is view and torch.equal(view, plain[k])
        want = render_contract(out.cpu().numpy(), image.cpu().numpy(), CITYSCAPES_COLORS, (0.485, 0.456, 0.406),
                               (0.229, 0.224, 0.225), 0.6)
        for k in views:
            assert np.array_equal(plain[k].cpu().numpy(), want[k]), k


# --------------------------------------------------------------------------- end to end on the stub model


def _decided_equal(pred, g, tag):
    pred = np.asarray(pred).astype(np.int64)
    wrong = int(((pred != g["pred"]) & ~g["undecided"]).sum())
    print(f"[{tag}] undecided {int(g['undecided'].sum())} px ({g['undecided_share']:.3e})  decided pixels predicted differently: {wrong}")
    assert pred.shape == g["pred"].shape and wrong == 0, tag


@pytest.mark.parametrize("case", CASES)
def test_fused_paths_match_the_reference(case):
    from cabinet_amd.predict import Predictor, infer_image

    g = load_case(case)
    net = g["model"].cuda()
    kw = dict(scales=g["scales"], flip=g["flip"])
    pred = infer_image(net, g["image"], num_classes=g["n_classes"], scales=list(g["scales"]), flip=g["flip"], device="cuda", fused=True)
    assert pred.dtype == np.int64
    _decided_equal(pred, g, f"case {case} infer_image(fused=True)")
    plain = infer_image(net, g["image"], num_classes=g["n_classes"], scales=list(g["scales"]), flip=g["flip"], device="cuda", fused=False)
    _decided_equal(plain, g, f"case {case} infer_image(fused=False) on the GPU")
    eager = Predictor(net, g["n_classes"], fused=True, **kw).predict(g["image"])
    assert eager.dtype == torch.uint8 and eager.is_cuda and np.array_equal(eager[0].cpu().numpy(), pred)
    graphed = Predictor(net, g["n_classes"], fused=True, graph=True, **kw)
    first = graphed.predict(g["image"]).clone()
    assert torch.equal(first, eager), "graphed output is not bit-identical to eager fused"
    # a second image through the same graph, then the first again: each replay answers for its own image
    other = torch.flip(g["image"], dims=(2,)).contiguous()
    want_other = Predictor(net, g["n_classes"], fused=True, **kw).predict(other)
    assert torch.equal(graphed.predict(other), want_other)
    assert torch.equal(graphed.predict(g["image"]), eager)
    assert len(graphed._graphs) == 1
    assert not torch.equal(want_other, eager)


def test_graph_follows_in_place_weight_updates_and_evicts():
    from cabinet_amd.predict import CITYSCAPES_COLORS, Predictor

    g = load_case(3)
    net = g["model"].cuda()
    kw = dict(scales=g["scales"], flip=g["flip"], fused=True)
    p = Predictor(net, g["n_classes"], graph=True, max_graphs=1, **kw)
    before = p.predict(g["image"]).clone()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    state["conv.weight"] = torch.roll(state["conv.weight"], 1, dims=0)   # class c takes class c-1's filter
    state["conv.bias"] = torch.roll(state["conv.bias"], 1, dims=0)
    net.load_state_dict(state)
    after = p.predict(g["image"]).clone()
    assert torch.equal(after, Predictor(net, g["n_classes"], **kw).predict(g["image"]))
    decided = torch.from_numpy(~g["undecided"])[None]   # the softmax sums run in another order: near-ties may fall either way
    assert torch.equal(after.cpu().long()[decided], ((before.cpu().long() + 1) % g["n_classes"])[decided])
    assert not torch.equal(after, before)
    # a sixth, distinct shape with room for one graph: the first is dropped, both still answer
    small = g["image"][:, :, :64, :88].contiguous()
    got = p.predict(small).clone()
    assert len(p._graphs) == 1 and next(iter(p._graphs))[0] == tuple(small.shape)
    assert torch.equal(got, Predictor(net, g["n_classes"], **kw).predict(small))
    assert torch.equal(p.predict(g["image"]), after)
    r = p.render(g["image"])
    assert torch.equal(r["pred"].cpu(), torch.from_numpy(CITYSCAPES_COLORS)[after.cpu().long()])
    net.train()
    with pytest.raises(RuntimeError, match="training mode"):
        p.predict(g["image"])


class _Net40(torch.nn.Module):
    """40 classes at full resolution, no forward_lowres: "low resolution at factor 1"."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 40, 1)

    def forward(self, x):
        y = self.conv(x)
        return y, y


def test_auto_mode_and_unsupported_shapes():
    from cabinet_amd import predict
    from cabinet_amd.predict import infer_image

    net40 = _Net40().cuda().eval()
    x = torch.randn(1, 3, 16, 24)
    auto = infer_image(net40, x, num_classes=40, device="cuda")          # more than 32 classes: the plain path, silently
    assert np.array_equal(auto, infer_image(net40, x, num_classes=40, device="cuda", fused=False))
    with pytest.raises(RuntimeError, match="32"):
        infer_image(net40, x, num_classes=40, device="cuda", fused=True)
    g = load_case(1)
    calls = []
    real = predict._fn.predict_up_argmax
    try:
        predict._fn.predict_up_argmax = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        infer_image(g["model"].cuda(), g["image"], num_classes=19, device="cuda")
        assert len(calls) == (1 if predict.FUSED_BY_DEFAULT else 0)
        infer_image(g["model"], g["image"], num_classes=19, device="cuda", fused=True)
        assert len(calls) == (2 if predict.FUSED_BY_DEFAULT else 1)
    finally:
        predict._fn.predict_up_argmax = real


# --------------------------------------------------------------------------- the real network


def _real_net(weight_scale):
    from cabinet_amd.train import build_model

    net = build_model("small", n_classes=19, seed=0, gamma=0.5)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2, generator=gen)
                m.running_var.uniform_(0.5, 1.5, generator=gen)
        net.conv_out.conv_out.weight.mul_(weight_scale)
    return net.cuda().eval()


def test_fused_vs_plain_on_the_real_network():
    """Plain-on-GPU fp32 is the yardstick, with the near-tie rule of tests/test_gpu_evaluate.py's real-network test: undecided =
    plain's own top-two probability margin below the TIE of evaluator fixture case 4; the classifier's weights are scaled until
    the PLAIN path alone leaves at most 0.2 % of the pixels undecided; the fused path is then run once per setting."""
    from cabinet_amd.predict import CITYSCAPES_COLORS, Predictor, _plain_probs

    tie = load_eval_case(4)["tie"]
    g = torch.Generator().manual_seed(23)
    image = torch.randn(1, 3, 256, 320, generator=g).cuda()
    settings = [((1.0,), False), ((0.75, 1.0), True)]
    with torch.no_grad():
        for scale in (1.0, 4.0, 16.0, 64.0, 256.0):
            net = _real_net(scale)
            probs = [_plain_probs(net, image, 19, s, f) for s, f in settings]
            shares = []
            for (s, _), p in zip(settings, probs):
                top2 = torch.topk(p * len(s), 2, dim=1).values   # the evaluator's map is the SUM over the scales
                shares.append(float(((top2[:, 0] - top2[:, 1]) < tie).float().mean()))
            print(f"classifier weights x{scale:g}: plain path leaves {shares} of the pixels undecided (tie {tie:.3e})")
            if max(shares) <= MAX_UNDECIDED_SHARE:
                break
    assert max(shares) <= MAX_UNDECIDED_SHARE
    assert float(net.ab.a2block.gamma.detach().abs().min()) > 0
    for (scales, flip), p in zip(settings, probs):
        top2 = torch.topk(p * len(scales), 2, dim=1).values
        undecided = (top2[:, 0] - top2[:, 1]) < tie
        want = torch.argmax(p, dim=1)
        pr = Predictor(net, 19, scales=scales, flip=flip, fused=True)
        got = pr.predict(image)
        wrong = int(((got.long() != want) & ~undecided).sum())
        print(f"CABiNet-Small scales={scales} flip={flip}: classes predicted {int(want.unique().numel())}  undecided "
              f"{int(undecided.sum())} px  decided pixels differing {wrong}")
        assert wrong == 0
        r = pr.render(image)
        for name in ("input", "pred", "overlay"):
            assert r[name].dtype == torch.uint8 and tuple(r[name].shape) == (1, 256, 320, 3) and r[name].is_cuda
        assert torch.equal(r["pred"].cpu(), torch.from_numpy(CITYSCAPES_COLORS)[got.cpu().long()])
