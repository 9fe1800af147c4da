"""HIP weight gradient of the wide pointwise convolutions (K14, through the C ABI) vs the oracle: fp64 F.conv2d with a 1x1
weight, the call oracle/model_ref.py::_mobilenet makes for mobilenetv3.py:128-131,144-151,193 and cabinet.py:114 -- every
(Ci, Co) pair the stock operator served at BASELINE config 3 / 5, ragged planes, B = 1 and 3, three layers at production size.

Two bounds on dw, both asserted: the suite's 1e-3 (||a-b|| / ||b||), and no worse than twice the stock operator's own distance
to the same fp64 result on the same inputs (the two differ only in summation order).  Both distances are printed."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3  # north_star: 1e-3 relative (||a-b||/||b|| per tensor), fp32

# (Ci, Co) of the 25 layers K10 leaves alone at config 3 (17 distinct pairs), by plane
PAIRS_128 = [(72, 40), (40, 120), (120, 40), (40, 240), (64, 128)]
PAIRS_64 = [(240, 80), (80, 200), (200, 80), (80, 184), (184, 80), (80, 480), (480, 112), (112, 672), (672, 112)]
PAIRS_32 = [(672, 160), (160, 960), (960, 160)]
ALL_PAIRS = PAIRS_128 + PAIRS_64 + PAIRS_32

CASES = ([(2, ci, co, 32, 32) for ci, co in ALL_PAIRS]
         + [(1, ci, co, 17, 19) for ci, co in ALL_PAIRS]                       # ragged: P = 323, B = 1
         + [(3, ci, co, 64, 65) for ci, co in [(72, 40), (40, 240), (200, 80), (112, 672), (960, 160)]]  # ragged, B = 3
         + [(1, 8, 8, 3, 5), (3, 104, 56, 17, 19), (1, 256, 256, 16, 16)]      # one block; odd block counts; square tile grid
         + [(8, 40, 240, 128, 128), (8, 112, 672, 64, 64), (8, 160, 960, 32, 32)])  # production size


def _native_dw(g, x, Ci, Co):
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    lib = _lib.load()
    B, P = x.shape[0], x.shape[2] * x.shape[3]
    dw = torch.full((Co, Ci), float("nan"), dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, Ci, Co, P), x.device)
    rc = lib.cabinet_pwconv_wide_wgrad(_ptr(g), _ptr(x), B, Ci, Co, P, _ptr(dw), _ptr(ws), nbytes, _stream_handle(x.device))
    _lib.check(rc, "cabinet_pwconv_wide_wgrad")
    return dw


def _stock_dw(g, x, w):
    return torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


@pytest.mark.parametrize("B,Ci,Co,H,W", CASES)
def test_pwconv_wide_wgrad_vs_oracle(B, Ci, Co, H, W):
    from cabinet_amd import _lib

    assert _lib.load().cabinet_pwconv_wide_supported(Ci, Co, H * W) == 1
    g0 = torch.Generator().manual_seed(Ci * 1000 + Co)
    x = torch.randn(B, Ci, H, W, generator=g0)
    g = torch.randn(B, Co, H, W, generator=g0)
    w = torch.randn(Co, Ci, 1, 1, generator=g0)
    wo = w.double().requires_grad_(True)
    F.conv2d(x.double(), wo).backward(g.double())
    ref = wo.grad.view(Co, Ci)
    xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
    dw = _native_dw(gd, xd, Ci, Co)
    stock = _stock_dw(gd, xd, wd).view(Co, Ci)
    torch.cuda.synchronize()
    assert torch.isfinite(dw).all()
    e_native, e_stock = rel_err(dw, ref), rel_err(stock, ref)
    print(f"pwconv_wide dw B={B} {Ci}->{Co} {H}x{W}: native {e_native:.3e}  stock {e_stock:.3e}")
    assert e_native <= TOL, f"dw: {e_native:.3e} > {TOL}"
    assert e_native <= 2.0 * e_stock, f"dw: native {e_native:.3e} > 2 x stock {e_stock:.3e}"


def test_pwconv_wide_argument_checks():
    from cabinet_amd import _lib

    lib = _lib.load()
    A = 0x10000
    assert lib.cabinet_pwconv_wide_supported(160, 960, 1024) == 1
    assert lib.cabinet_pwconv_wide_supported(20, 16, 4096) == 0      # channels not a multiple of 8
    assert lib.cabinet_pwconv_wide_supported(8192, 16, 4096) == 0    # past the channel limit
    assert lib.cabinet_pwconv_wide_wgrad_workspace_bytes(8, 20, 16, 4096) == 0
    assert lib.cabinet_pwconv_wide_wgrad(A, A, 8, 20, 16, 4096, A, A, 1 << 30, None) == -2
    assert lib.cabinet_pwconv_wide_wgrad(A, None, 8, 160, 960, 1024, A, A, 1 << 30, None) == -1
    assert lib.cabinet_pwconv_wide_wgrad(A, A, 0, 160, 960, 1024, A, A, 1 << 30, None) == -1
    need = lib.cabinet_pwconv_wide_wgrad_workspace_bytes(8, 160, 960, 1024)
    assert need > 0
    rc = lib.cabinet_pwconv_wide_wgrad(A, A, 8, 160, 960, 1024, A, A, need - 1, None)
    assert rc != 0 and b"workspace" in lib.cabinet_last_error()


@pytest.mark.parametrize("B,Ci,Co,H,W", [(8, 160, 960, 32, 32), (2, 40, 120, 64, 65), (3, 200, 80, 17, 19)])
def test_pwconv_wide_bit_reproducible_eager_and_graph(B, Ci, Co, H, W):
    x = torch.randn(B, Ci, H, W, device="cuda")
    g = torch.randn(B, Co, H, W, device="cuda")
    a = _native_dw(g, x, Ci, Co)
    b = _native_dw(g, x, Ci, Co)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _native_dw(g, x, Ci, Co)  # the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = _native_dw(g, x, Ci, Co)
    outs = []
    for _ in range(2):
        c.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        outs.append(c.clone())
    assert torch.equal(outs[0], a) and torch.equal(outs[1], a)


def test_pwconv_wide_function_matches_stock_autograd():
    """The Function: forward and dx are the stock operator's (bit for bit), dw the kernel's."""
    from cabinet_amd.functional import pwconv_wide, pwconv_wide_supported

    conv = torch.nn.Conv2d(80, 184, 1, bias=False).cuda()
    x = torch.randn(2, 80, 24, 20, device="cuda", requires_grad=True)
    g = torch.randn(2, 184, 24, 20, device="cuda")
    assert pwconv_wide_supported(conv, x)
    y0 = conv(x)
    y0.backward(g)
    dx0, dw0 = x.grad.clone(), conv.weight.grad.clone()
    x.grad = None
    conv.zero_grad()
    y1 = pwconv_wide(x, conv)
    y1.backward(g)
    assert torch.equal(y0, y1) and torch.equal(dx0, x.grad)
    assert conv.weight.grad.shape == dw0.shape and rel_err(conv.weight.grad, dw0) <= TOL
    # what keeps the stock path
    with torch.no_grad():
        assert not pwconv_wide_supported(conv, x)
    assert not pwconv_wide_supported(torch.nn.Conv2d(80, 184, 1, bias=True).cuda(), x)
    assert not pwconv_wide_supported(torch.nn.Conv2d(80, 184, 1, stride=2, bias=False).cuda(), x)
    assert not pwconv_wide_supported(torch.nn.Conv2d(80, 184, 3, padding=1, bias=False).cuda(), x)
    assert not pwconv_wide_supported(torch.nn.Conv2d(80, 180, 1, bias=False).cuda(), x)  # channels not a multiple of 8
    assert not pwconv_wide_supported(torch.nn.Conv2d(80, 184, 1, bias=False), x.detach().cpu())
    frozen = torch.nn.Conv2d(80, 184, 1, bias=False).cuda().requires_grad_(False)
    assert not pwconv_wide_supported(frozen, x)


def _expected(h, w):
    """(Ci, Co, pixels per image) of every layer of the table for an h x w input."""
    return sorted([(ci, co, (h // 8) * (w // 8)) for ci, co in PAIRS_128 + [(120, 40), (40, 120)]]
                  + [(ci, co, (h // 16) * (w // 16)) for ci, co in PAIRS_64 + [(184, 80), (80, 184), (112, 672)]]
                  + [(ci, co, (h // 32) * (w // 32)) for ci, co in PAIRS_32 + [(160, 960), (960, 160), (160, 960)]])


@pytest.mark.parametrize("h,w,classes", [(1024, 1024, 8), (2048, 1024, 19)])
def test_model_routes_the_wide_pointwise_layers(h, w, classes, monkeypatch):
    from cabinet_amd import functional as Fh
    from cabinet_amd.models.cabinet import CABiNet
    from cabinet_amd.models.constants import MOBILENETV3_CFGS

    wide, thin = [], []
    wide_apply, thin_apply = Fh._PwConvWide.apply, Fh._PwConv.apply

    def rec_wide(x, weight):
        wide.append((weight.shape[1], weight.shape[0], x.shape[2] * x.shape[3]))
        return wide_apply(x, weight)

    def rec_thin(x, weight):
        thin.append((weight.shape[1], weight.shape[0], x.shape[2] * x.shape[3]))
        return thin_apply(x, weight)

    monkeypatch.setattr(Fh._PwConvWide, "apply", rec_wide)
    monkeypatch.setattr(Fh._PwConv, "apply", rec_thin)
    torch.manual_seed(0)
    net = CABiNet(n_classes=classes, cfgs=MOBILENETV3_CFGS["large"], mode="large").cuda().train()
    x = torch.randn(1, 3, h, w, device="cuda")
    net(x)
    assert len(_expected(h, w)) == 25
    assert sorted(wide) == _expected(h, w)
    assert thin and all(ci <= 96 and co <= 96 and p >= 65536 for ci, co, p in thin)  # K10's layers are still K10's
    n_thin = len(thin)
    del wide[:], thin[:]
    with torch.no_grad():
        net(x)
    assert not wide and len(thin) == n_thin
    del wide[:], thin[:]
    net.eval()
    with torch.no_grad():
        net(x)
    assert not wide and len(thin) == n_thin
