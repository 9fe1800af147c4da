"""The top-n_min branch of OHEM-CE (reference src/utils/loss.py:76-79) on the host: the conditions the stored vectors of
tests/golden/g7_ohem_topk.npz (tests/golden/make_golden_ohem_topk.py: the reference in float64 at its real thresh = 0.7) must
meet for the device comparisons to be decided by the reference alone, the composite path against them, the ``device_select``
keyword (off by default everywhere, no effect on CPU tensors), and the C header's new entry points.
The device kernels are covered by tests/test_gpu_ohem_topk.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g7_ohem_topk.npz")
IGNORE = 255
NEW_SYMBOLS = ("cabinet_ohem_select_workspace_bytes", "cabinet_ohem_select", "cabinet_ohem_up_w_bwd_sel",
               "cabinet_ohem_up_pair_w_bwd_sel")


def fixture():
    return np.load(FIXTURE)


def case_names(d):
    return [str(c) for c in d["cases"]]


def load_head(d, name, hi=0):
    """-> low, labels (int64), weight | None, size, n_min, thresh"""
    low = torch.from_numpy(d[f"{name}.h{hi}.low"])
    labels = torch.from_numpy(d[f"{name}.labels"].astype(np.int64))
    weight = torch.from_numpy(d[f"{name}.weight"]) if f"{name}.weight" in d.files else None
    size = tuple(int(v) for v in d[f"{name}.size"])
    return low, labels, weight, size, int(d[f"{name}.n_min"]), float(d["thresh"])


def px64(low, labels, weight, size):
    up = F.interpolate(low.double(), size=size, mode="bilinear", align_corners=False)
    return F.cross_entropy(up, labels, weight=None if weight is None else weight.double(), ignore_index=IGNORE, reduction="none")


def test_fixture_meets_the_conditions_the_comparisons_rely_on():
    """Not a measurement.  (i) no valid pixel within 1e-5 of thresh; (ii) on a top-n_min head every valid pixel other than the
    k-th itself within delta = 1e-4 of the k-th value has a loss of at most 1e-6 (what an fp32 kernel may rank differently is
    saturated); (iii) delta is at least 10x the fp32 evaluation error of the per-pixel loss; (iv) case d ties at zero in fp32.
    And the cases are what the module docstring of the generator says: branch per head, ~10 % ignored, a zero-weight class."""
    d = fixture()
    assert case_names(d) == ["a", "b", "c", "d"]
    gap, delta, sat = float(d["gap"]), float(d["delta"]), float(d["sat"])
    assert (gap, delta, sat, float(d["thresh"])) == (1e-5, 1e-4, 1e-6, 0.7)
    shapes, branches = {}, {}
    for name in case_names(d):
        nh = int(d[f"{name}.n_heads"])
        branches[name] = [str(d[f"{name}.h{hi}.branch"]) for hi in range(nh)]
        for hi in range(nh):
            low, labels, weight, size, n_min, thresh = load_head(d, name, hi)
            shapes[name] = tuple(low.shape) + size
            assert low.dtype == torch.float32 and n_min == labels.numel() // 16
            valid = labels != IGNORE
            assert 0.05 <= 1.0 - float(valid.double().mean()) <= 0.15
            l64 = px64(low, labels, weight, size)[valid]
            w32 = None if weight is None else weight.float()
            up32 = F.interpolate(low, size=size, mode="bilinear", align_corners=False)
            l32 = F.cross_entropy(up32, labels, weight=w32, ignore_index=IGNORE, reduction="none")[valid]
            n_valid, n_above = int(valid.sum()), int((l64 > thresh).sum())
            k = min(n_min, n_valid)
            assert (n_valid, n_above) == (int(d[f"{name}.h{hi}.n_valid"]), int(d[f"{name}.h{hi}.n_above"]))
            assert float((l64 - thresh).abs().min()) >= gap                                        # (i)
            assert delta >= 10 * float((l32.double() - l64).abs().max())                           # (iii)
            assert (n_above >= k) == (branches[name][hi] == "sel")
            if branches[name][hi] == "topk":
                t = float(torch.sort(l64, descending=True).values[k - 1])
                assert t == float(d[f"{name}.h{hi}.t"])
                near = (l64 - t).abs() <= delta
                assert int((near & (l64 > sat)).sum()) - (1 if t > sat else 0) <= 0                # (ii)
                if name == "d":
                    t32 = torch.sort(l32, descending=True).values[k - 1]
                    assert float(t32) == 0.0 and int((l32 == t32).sum()) > 1 and int((l32 != 0).sum()) < k   # (iv)
        if f"{name}.weight" in d.files:
            w = d[f"{name}.weight"]
            zero = [c for c in range(len(w)) if w[c] == 0.0]
            assert w.dtype == np.float32 and float(w.min()) >= 0.0 and len(zero) == 1
            assert int((d[f"{name}.labels"] == zero[0]).sum()) > 0
    assert branches == {"a": ["topk"], "b": ["topk"], "c": ["topk", "sel"], "d": ["topk"]}
    assert shapes["a"] == (1, 8, 8, 64, 64, 512) and shapes["a"][3] % 64 == 0 and shapes["a"][5] == 8 * shapes["a"][3]
    assert shapes["b"][1] == 19 and shapes["b"][5] != 8 * shapes["b"][3] and "b.weight" in d.files
    assert "a.weight" not in d.files


@pytest.mark.parametrize("device_select", [False, True])
@pytest.mark.parametrize("dtype,ltol,gtol", [(torch.float64, 1e-10, 1e-9), (torch.float32, 1e-5, 1e-3)])
def test_host_path_matches_the_reference_with_and_without_device_select(dtype, ltol, gtol, device_select):
    """CPU tensors take the composite path whatever ``device_select`` says; it reproduces the reference's loss and gradient on
    both branches (float64 to rounding, fp32 within the project's tolerances)."""
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    d = fixture()
    for name in case_names(d):
        nh = int(d[f"{name}.n_heads"])
        xs, crits, total = [], [], 0.0
        for hi in range(nh):
            low, labels, weight, size, n_min, thresh = load_head(d, name, hi)
            crit = OhemCELoss(thresh, n_min, IGNORE, weight=None if weight is None else weight.to(dtype),
                              device_select=device_select)
            x = low.to(dtype).clone().requires_grad_(True)
            loss = crit.forward_upsampled(x, labels, size)
            loss.backward()
            ref = float(d[f"{name}.h{hi}.loss"])
            assert abs(float(loss.detach()) - ref) <= ltol * max(1.0, abs(ref)), (name, hi)
            assert_close(x.grad, torch.from_numpy(d[f"{name}.h{hi}.dlow"]).to(dtype), max(gtol, 1e-6), f"{name}.h{hi} dlow", atol=1e-9)
            xs.append(low.to(dtype).clone().requires_grad_(True))
            crits.append(crit)
            total += ref
        if nh == 2:
            loss = ohem_upsampled_pair(crits[0], xs[0], crits[1], xs[1], labels, size)
            assert abs(float(loss.detach()) - total) <= ltol * max(1.0, abs(total))


def test_device_select_is_a_keyword_after_the_references_four_and_off_by_default():
    from cabinet_amd.loss import OhemCELoss
    from cabinet_amd.train import GraphedTrainStep, make_criteria

    params = list(inspect.signature(OhemCELoss.__init__).parameters)
    assert params[1:] == ["thresh", "n_min", "ignore_lb", "weight", "device_select"]
    for fn in (OhemCELoss.__init__, make_criteria, GraphedTrainStep.__init__):
        assert inspect.signature(fn).parameters["device_select"].default is False
    plain, on = OhemCELoss(0.7, 10, 255, weight=[1.0, 2.0]), OhemCELoss(0.7, 10, 255, weight=[1.0, 2.0], device_select=True)
    assert plain.device_select is False and on.device_select is True
    assert list(plain.state_dict()) == list(on.state_dict()) == ["weight"]          # a plain attribute, not a buffer
    assert "device_select" not in repr(plain) and "device_select=True" in repr(on)
    ca, cb = make_criteria(2, 64, 64, "cpu")
    assert not ca.device_select and not cb.device_select
    ca, cb = make_criteria(2, 64, 64, "cpu", weight=[1.0] * 8, device_select=True)
    assert ca.device_select and cb.device_select and ca.weight is not cb.weight


def test_device_select_changes_nothing_on_host_tensors():
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    g = torch.Generator().manual_seed(3)
    low, low2 = torch.randn(2, 5, 6, 7, generator=g), torch.randn(2, 5, 6, 7, generator=g)
    lab = torch.randint(0, 5, (2, 24, 28), generator=g)
    lab[torch.rand(2, 24, 28, generator=g) < 0.1] = IGNORE
    for thresh in (0.7, 1e4):                                                          # both branches
        res = []
        for ds in (False, True):
            ca, cb = OhemCELoss(thresh, 84, IGNORE, device_select=ds), OhemCELoss(thresh, 84, IGNORE, device_select=ds)
            xa, xb = low.clone().requires_grad_(True), low2.clone().requires_grad_(True)
            single = ca.forward_upsampled(xa, lab, (24, 28))
            pair = ohem_upsampled_pair(ca, xa, cb, xb, lab, (24, 28))
            (single + pair).backward()
            res.append((single.detach(), pair.detach(), xa.grad, xb.grad))
        for a, b in zip(*res):
            assert torch.equal(a, b)
    allign = torch.full((2, 24, 28), IGNORE)
    for ds in (False, True):
        z = OhemCELoss(0.7, 84, IGNORE, device_select=ds).forward_upsampled(low.clone().requires_grad_(True), allign, (24, 28))
        assert float(z) == 0.0 and z.requires_grad


def test_header_and_binding_declare_the_new_entry_points_under_abi_8():
    from cabinet_amd import _lib

    text = open(os.path.join(ROOT, "include", "cabinet_hip.h")).read()
    assert re.search(r"#define\s+CABINET_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", code), sym
        assert sym in _lib.SIGNATURES, sym
    # the `_bwd_sel` lists are the `_w_bwd` lists with the device pointer in the place of `float thresh`
    for a, b in (("cabinet_ohem_up_w_bwd", "cabinet_ohem_up_w_bwd_sel"), ("cabinet_ohem_up_pair_w_bwd", "cabinet_ohem_up_pair_w_bwd_sel")):
        (ra, aa), (rb, ab) = _lib.SIGNATURES[a], _lib.SIGNATURES[b]
        assert ra is rb and len(aa) == len(ab)
        diff = [i for i, (x, y) in enumerate(zip(aa, ab)) if x is not y]
        assert len(diff) == 1 and aa[diff[0]] is _lib._FLT and ab[diff[0]] is _lib._PTR
    assert "loss.py:67-80" in text


def test_select_argument_checks_need_no_gpu():
    from cabinet_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    assert lib.cabinet_ohem_select_workspace_bytes(2, 8, 1024, 1024) > lib.cabinet_ohem_select_workspace_bytes(1, 8, 1024, 1024) > 0
    assert lib.cabinet_ohem_select_workspace_bytes(3, 8, 1024, 1024) == 0
    A, M = 0x10000, 0x10004   # never dereferenced: every check below fails before any HIP call
    rc = lib.cabinet_ohem_select(A, A, A, 3, 1, 8, 32, 32, 0.7, 64, 64, 255, None, None, A, A, 1 << 20, None)
    assert rc == -1 and b"nheads" in lib.cabinet_last_error()
    rc = lib.cabinet_ohem_select(A, A, None, 1, 1, 8, 32, 32, 0.7, 64, 64, 255, None, None, A, A, 1 << 20, None)
    assert rc == -1 and b"null" in lib.cabinet_last_error()
    rc = lib.cabinet_ohem_select(M, A, A, 1, 1, 8, 32, 32, 0.7, 64, 64, 255, None, None, A, A, 1 << 20, None)
    assert rc == -1 and b"16-byte aligned" in lib.cabinet_last_error()
    rc = lib.cabinet_ohem_select(A, A, A, 1, 1, 8, 32, 32, 0.7, 64, 64, 255, None, None, A, A, 16, None)
    assert rc == -3 and b"workspace" in lib.cabinet_last_error()
    rc = lib.cabinet_ohem_select(A, A, A, 1, 1, 40, 32, 32, 0.7, 64, 64, 255, None, None, A, A, 1 << 20, None)
    assert rc == -2
    rc = lib.cabinet_ohem_up_w_bwd_sel(A, A, A, 1, 8, 4, 4, 32, 32, None, 255, 1.0, A, A, 1 << 30, None, None)
    assert rc == -1 and b"null" in lib.cabinet_last_error()
    rc = lib.cabinet_ohem_up_pair_w_bwd_sel(A, A, A, A, 1, 8, 4, 4, 32, 32, M, 255, 1.0, A, A, 1 << 30, None, None, None)
    assert rc == -1 and b"16-byte aligned" in lib.cabinet_last_error()
