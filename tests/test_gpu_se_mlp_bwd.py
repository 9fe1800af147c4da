"""The squeeze-excite MLP's backward between the two streaming passes of the SE tail in two HIP launches
(cabinet_se_act_bwd_mlp, csrc/se_mlp.hip) against the chain of torch ops it replaces (functional.SE_MLP_FUSED off):

* operator level, on planted inputs: every output against the formulas written out in fp64 -- at most ALLOW_FACTOR x as far
  from fp64 as the chain is on the same tensor, exactly zero where the tensor is analytically zero; the coefficient tail bit
  for bit what cabinet_se_act_bwd_coef gives for the same ds; two runs bit-equal; NaN-filled outputs and workspace change nothing;
* module level (se_tail): flag on against flag off, eager and replayed from a captured graph; the size limit's other side."""
import pytest
import torch

from conftest import assert_close, rel_err
from parity_rules import ALLOW_FACTOR
from test_gpu_se_tail import TOL, _case

pytestmark = pytest.mark.gpu

# (B, C, Cs): one image, odd B, C / Cs that are no multiples of 32 or 64, one slab, the largest block
SHAPES = [(1, 8, 8), (3, 16, 8), (8, 24, 8), (5, 40, 16), (2, 72, 24), (2, 120, 32), (2, 144, 40), (2, 672, 168), (8, 960, 240)]
PS = [1, 1024, 16384]
OUT = ("dw1", "db1", "dw2", "db2", "ds", "ds_over_p", "dbn_weight", "dbn_bias", "coef")


def _inputs(B, C, Cs, seed=0, zero_image=True):
    """Planted edges: h1 from a real relu (exact zeros) with image B-1 all zero, da2 with exact zeros and channel 1 zero in every
    image, gate entries exactly 0 and exactly 1, sums of both signs."""
    g = torch.Generator().manual_seed(1000 * B + C + Cs + seed)
    pooled = torch.randn(B, C, generator=g)
    w1 = torch.randn(Cs, C, generator=g) / C ** 0.5
    w2 = torch.randn(C, Cs, generator=g) / Cs ** 0.5
    h1 = torch.relu(pooled @ w1.t() + 0.5 * torch.randn(Cs, generator=g))
    if zero_image:
        h1[B - 1] = 0
    da2 = torch.randn(B, C, generator=g)
    da2[torch.rand(B, C, generator=g) < 0.2] = 0
    da2[:, 1] = 0
    gate = torch.rand(B, C, generator=g)
    gate[0, 0], gate[B - 1, C - 1] = 0.0, 1.0
    sums = torch.randn(3, B, C, generator=g) * 8
    t = dict(sums=sums, da2=da2, gate=gate, h1=h1, pooled=pooled, w1=w1, w2=w2)
    assert (h1 == 0).any() and (sums < 0).any() and (da2 == 0).any()
    return {k: v.cuda() for k, v in t.items()}


def _fp64(t, P, training):
    d = {k: v.double() for k, v in t.items()}
    B, C = d["da2"].shape
    o = {}
    o["dw2"] = torch.einsum("bc,bj->cj", d["da2"], d["h1"])
    o["db2"] = d["da2"].sum(0)
    da1 = torch.einsum("bc,cj->bj", d["da2"], d["w2"]) * (d["h1"] > 0)
    o["db1"] = da1.sum(0)
    o["dw1"] = torch.einsum("bj,bc->jc", da1, d["pooled"])
    o["ds"] = torch.einsum("bj,jc->bc", da1, d["w1"])
    o["ds_over_p"] = o["ds"] / P
    A, X, S = d["sums"]
    o["dbn_bias"] = (d["gate"] * A + o["ds"]).sum(0)
    o["dbn_weight"] = (d["gate"] * X + o["ds_over_p"] * S).sum(0)
    o["coef"] = torch.stack([o["dbn_bias"], o["dbn_weight"]]) / (B * P) * (1.0 if training else 0.0)
    return o


def _coef(t, ds, P, training):
    from cabinet_amd import _lib

    B, C = ds.shape
    o = dict(dbn_weight=torch.empty(C), dbn_bias=torch.empty(C), coef=torch.empty(2, C), ds_over_p=torch.empty(B, C))
    o = {k: v.cuda() for k, v in o.items()}
    rc = _lib.load().cabinet_se_act_bwd_coef(t["sums"].data_ptr(), t["gate"].data_ptr(), ds.data_ptr(), B, C, P, int(training),
                                             o["dbn_weight"].data_ptr(), o["dbn_bias"].data_ptr(), o["coef"].data_ptr(),
                                             o["ds_over_p"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cabinet_se_act_bwd_coef")
    return o


def _chain(t, P, training):
    """The MLP backward of _SeTail.backward with SE_MLP_FUSED off, op for op."""
    da2, h1, pooled, w1, w2 = t["da2"], t["h1"], t["pooled"], t["w1"], t["w2"]
    o = {}
    o["dw2"], o["db2"] = da2.t().mm(h1), da2.sum(0)
    da1 = da2.mm(w2) * (h1 > 0)
    o["dw1"], o["db1"] = da1.t().mm(pooled), da1.sum(0)
    o["ds"] = da1.mm(w1)
    o.update(_coef(t, o["ds"], P, training))
    return o


def _fused(t, P, training, poison=False):
    from cabinet_amd import _lib

    lib = _lib.load()
    B, C = t["da2"].shape
    Cs = t["h1"].shape[1]
    shapes = dict(dw1=(Cs, C), db1=(Cs,), dw2=(C, Cs), db2=(C,), ds=(B, C), dbn_weight=(C,), dbn_bias=(C,), coef=(2, C),
                  ds_over_p=(B, C))
    fill = float("nan") if poison else 0.0
    o = {k: torch.full(s, fill, dtype=torch.float32, device="cuda") for k, s in shapes.items()}
    nbytes = lib.cabinet_se_act_bwd_mlp_workspace_bytes(B, C, Cs)
    ws = torch.full((nbytes // 4,), fill, dtype=torch.float32, device="cuda")
    rc = lib.cabinet_se_act_bwd_mlp(*[t[k].data_ptr() for k in ("sums", "da2", "gate", "h1", "pooled", "w1", "w2")], B, C, Cs, P,
                                    int(training), *[o[k].data_ptr() for k in ("dw1", "db1", "dw2", "db2", "ds", "dbn_weight",
                                                                               "dbn_bias", "coef", "ds_over_p")],
                                    ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cabinet_se_act_bwd_mlp")
    torch.cuda.synchronize()
    return o


def _check_case(t, P, training):
    ref = _fp64(t, P, training)
    old, new = _chain(t, P, training), _fused(t, P, training)
    rows = []
    for k in OUT:
        assert new[k].shape == ref[k].shape and torch.isfinite(new[k]).all(), k
        if not ref[k].any():
            assert not new[k].any(), f"{k}: analytically zero"
            continue
        d_old, d_new = rel_err(old[k], ref[k]), rel_err(new[k], ref[k])
        rows.append((k, d_old, d_new))
        print(f"{k:11s} chain {d_old:.3e}  fused {d_new:.3e}")
    for k, d_old, d_new in rows:
        assert d_new <= ALLOW_FACTOR * d_old, f"{k}: fused {d_new:.3e} vs chain {d_old:.3e} from fp64"
    # the coefficient tail: this entry point's own ds through the separate kernel, bit for bit
    tail = _coef(t, new["ds"], P, training)
    for k in tail:
        assert torch.equal(tail[k], new[k]), k
    return new


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_mlp_bwd_vs_fp64_and_chain(shape, P, training):
    _check_case(_inputs(*shape), P, training)


def test_mlp_bwd_single_image_with_live_hidden_units():
    """(1, 8, 8) above has its only image's h1 zeroed (everything behind the ReLU is analytically zero); here it is live."""
    _check_case(_inputs(1, 8, 8, zero_image=False), 1024, 1)


def test_mlp_bwd_more_images_than_one_pass():
    """B beyond the 8 images a contraction pass stages: further passes, the tail's image order carried across them."""
    _check_case(_inputs(19, 40, 16), 1024, 1)


@pytest.mark.parametrize("shape", [(3, 16, 8), (2, 672, 168), (8, 960, 240), (19, 40, 16)])
def test_mlp_bwd_is_deterministic_and_owns_its_outputs(shape):
    """Two runs are bit-equal; with the workspace and every output pre-filled with NaN the bits are the same and all finite:
    every element is written and nothing stale is read."""
    t = _inputs(*shape)
    a, b, c = _fused(t, 1024, 1), _fused(t, 1024, 1), _fused(t, 1024, 1, poison=True)
    for k in OUT:
        assert torch.equal(a[k], b[k]), k
        assert torch.isfinite(c[k]).all() and torch.equal(a[k], c[k]), k


def _tail_run(shape, fused, monkeypatch, training=True, seed=5):
    import cabinet_amd.functional as Fh

    monkeypatch.setattr(Fh, "SE_MLP_FUSED", fused)
    mods, z, g, act = _case(shape, training, seed=seed)
    dev = mods.cuda()
    zd = z.cuda().requires_grad_(True)
    y = Fh.se_tail(zd, dev[0], dev[1], act)
    y.backward(g.cuda())
    torch.cuda.synchronize()
    return y, zd.grad, dev


@pytest.mark.parametrize("shape", [(72, 16, 16, "relu"), (24, 37, 29, "hardswish")])
def test_se_tail_flag_on_vs_off(shape, monkeypatch):
    y0, dz0, m0 = _tail_run(shape, False, monkeypatch)
    y1, dz1, m1 = _tail_run(shape, True, monkeypatch)
    assert torch.equal(y0, y1)
    for (k, p), (_, q) in zip(m1.named_buffers(), m0.named_buffers()):
        assert torch.equal(p, q), k
    assert_close(dz1, dz0, TOL, "dz")
    grads = [(k, p.grad, q.grad) for (k, p), (_, q) in zip(m1.named_parameters(), m0.named_parameters())]
    assert len(grads) == 6 and all(a is not None for _, a, _ in grads)  # BatchNorm weight / bias, fc1 and fc2 weight / bias
    for k, a, b in grads:
        assert_close(a, b, TOL, k)


def test_se_tail_beyond_the_size_limit_keeps_the_chain(monkeypatch):
    """C = 1032 > 1024: the entry point answers CABINET_ERR_UNSUPPORTED and the torch chain runs -- the same bits as flag off."""
    from cabinet_amd import _lib

    lib = _lib.load()
    t = _inputs(2, 1032, 8)
    with pytest.raises(RuntimeError, match="code -2"):
        _fused(t, 16, 1)
    shape = (1032, 4, 4, "relu")
    y0, dz0, m0 = _tail_run(shape, False, monkeypatch)
    y1, dz1, m1 = _tail_run(shape, True, monkeypatch)
    assert torch.equal(y0, y1) and torch.equal(dz0, dz1)
    for p, q in zip(m1.parameters(), m0.parameters()):
        assert torch.equal(p.grad, q.grad)
    assert lib.cabinet_se_act_bwd_mlp_workspace_bytes(2, 1024, 256) >= 4 * 2 * 256  # the last supported width


def test_se_tail_fused_under_graph_capture(monkeypatch):
    """Forward and backward captured in a hipGraph and replayed twice: the gradients equal the eager run's -- no allocation
    outside the graph's pool and no synchronisation in the new path."""
    import cabinet_amd.functional as Fh

    shape = (72, 16, 16, "relu")
    _, dz_e, m_e = _tail_run(shape, True, monkeypatch)
    mods, z, g, act = _case(shape, True, seed=5)
    dev = mods.cuda()
    zd = z.cuda().requires_grad_(True)
    gd = g.cuda()
    params = list(dev.parameters())
    buffers = [b.clone() for b in dev.buffers()]

    def step():
        y = Fh.se_tail(zd, dev[0], dev[1], act)
        return torch.autograd.grad(y, [zd] + params, gd)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for b, b0 in zip(dev.buffers(), buffers):  # the eager run saw the initial running statistics; they do not feed gradients
            b.copy_(b0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], dz_e)
        for o, p in zip(outs[1:], m_e.parameters()):
            assert torch.equal(o, p.grad)
