"""The thin 1x1 convolution family -- K10's stream kernels (csrc/pwconv.hip), K14's weight gradient and the BN form
(csrc/pwconv_wide.hip), the SE MLP adjoint (csrc/se_mlp.hip) -- at every instantiation its launch plans can pick, through the C
ABI, on NaN-prefilled outputs and workspaces.  The tables are tests/pw_family_cases.py; tests/test_pw_family_plans.py holds them
against the library's own plan queries (no GPU), this file runs them:

a. K10, every supported (Ci, Co) in multiples of 8: y, dx, dW on three planes whose last block is ragged in each vector form,
   against fp64 on the CPU.  y and dx per ELEMENT: |a - ref| <= K 2^-23 (|A| |X|), the bound of a K-term fp32 dot product (K the
   contracted length), doubled because the order of the two products inside the MFMA is undocumented -- derived, not measured.
   dW: 1e-3 in the 2-norm and the max-norm, bit-equal to cabinet_pwconv_wide_wgrad (same kernel, same plan), two calls equal.
b. K10, the 16-byte, 8-byte and dword forms on the same data (pointers 0, 8 and 4 bytes off): the three results are torch.equal.
c. K10, every pipelined instantiation (and both plain walks) on a loaded chip: 4203 blocks on the 2048-workgroup grid, the bound
   of (a) per element against an fp64 einsum on the device, two runs with one SHA-256, finite everywhere.  The store hazard
   recorded in DESIGN.md (K10) showed under load only and differently per instantiation.  Three input gradients (A = W^T through
   its strides, one per vector form) run under the same load.
d. The small backbone's features.1 expand (16 -> 72 on a 256 x 256 plane) through functional.pwconv.
e. The BN form at its nine instantiations, with the criteria of test_gpu_pw_bn_bwd.py; <2,3> and <3,2> -- more than 64 KB of
   LDS, one workgroup per CU -- also on the full grid.
f. K14 at the tile shapes no other file launches, with the criteria of test_gpu_pwconv_wide.py.
g. The SE MLP adjoint off the multiples of 8, past one column tile, at its size limit, either side of a pass of eight images,
   with the check of test_gpu_se_mlp_bwd.py unchanged.

Every distance is printed (profiles/pw_family_test_distances.txt is the record of one run); misses are collected into one message
per test and the number of cases run is asserted."""
import hashlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pw_bn_bwd_cases as bnc  # noqa: E402
import pw_family_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3  # the project's bound on the relative distance from fp64


def _report(fails, ran, expected):
    assert ran == expected, f"{ran} cases run, {expected} expected"
    assert not fails, f"{len(fails)} misses, the first of them:\n" + "\n".join(fails[:40])


def _at_offset(shape, off_bytes, src=None):
    """A dense device tensor `off_bytes` past 16-byte alignment: a copy of src, or NaN."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0 and off_bytes % 4 == 0
    v = flat[off_bytes // 4:off_bytes // 4 + n].view(shape)
    if src is None:
        v.fill_(float("nan"))
    else:
        v.copy_(src)
    assert v.data_ptr() % 16 == off_bytes
    return v


def _nan_ws(nbytes):
    return torch.full((max(nbytes, 4) // 4 + 1,), float("nan"), dtype=torch.float32, device="cuda")


def _k10_fwd(lib, x, w, y):
    from cabinet_amd.functional import _ptr, _stream_handle

    (B, Ci, P), Co = x.shape, w.shape[0]
    rc = lib.cabinet_pwconv_fwd(_ptr(x), _ptr(w), B, Ci, Co, P, _ptr(y), _stream_handle(x.device))
    assert rc == 0, lib.cabinet_last_error()
    return y


def _k10_bwd(lib, g, x, w, dx, dw):
    from cabinet_amd.functional import _ptr, _stream_handle

    (B, Ci, P), Co = x.shape, w.shape[0]
    nbytes = lib.cabinet_pwconv_bwd_workspace_bytes(B, Ci, Co, P)
    ws = _nan_ws(nbytes)
    rc = lib.cabinet_pwconv_bwd(_ptr(g), _ptr(x), _ptr(w), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes, _stream_handle(x.device))
    assert rc == 0, lib.cabinet_last_error()
    return dx, dw


def _wide_dw(lib, g, x, Ci, Co):
    from cabinet_amd.functional import _ptr, _stream_handle

    B, P = x.shape[0], x.shape[2]
    dw = torch.full((Co, Ci), float("nan"), dtype=torch.float32, device="cuda")
    nbytes = lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, Ci, Co, P)
    ws = _nan_ws(nbytes)
    rc = lib.cabinet_pwconv_wide_wgrad(_ptr(g), _ptr(x), B, Ci, Co, P, _ptr(dw), _ptr(ws), nbytes, _stream_handle(x.device))
    assert rc == 0, lib.cabinet_last_error()
    return dw


def _k10_inputs(B, Ci, Co, P):
    gen = torch.Generator().manual_seed(100003 * Ci + 1009 * Co + P)
    return (torch.randn(B, Ci, P, generator=gen), torch.randn(Co, Ci, generator=gen) * Ci ** -0.5,
            torch.randn(B, Co, P, generator=gen))


# ================================================================================================ a. K10, every channel pair
_MB_COUNT = {1: 4, 2: 4, 3: 4, 4: 3}  # channel counts per row-block count: 8..32, 40..64, 72..96, 104..120 (128 is past the LDS limit)
MB_GROUPS = [(a, b) for a in range(1, 5) for b in range(1, 5) if a * b <= 8]


@pytest.mark.parametrize("mbo,mbi", MB_GROUPS, ids=[f"co{a}x32-ci{b}x32" for a, b in MB_GROUPS])
def test_k10_every_channel_pair(mbo, mbi):
    lib = fc.load_library()
    pairs = [(ci, co) for ci, co in fc.k10_pairs(lib) if -(-co // 32) == mbo and -(-ci // 32) == mbi]
    fails, ran, worst = [], 0, 0.0
    for ci, co in pairs:
        for P in fc.K10_PLANES:
            B = fc.K10_B
            x, w, g = _k10_inputs(B, ci, co, P)
            xd, wd, gd = x.cuda(), w.cuda(), g.cuda()
            y = _k10_fwd(lib, xd, wd, torch.full_like(gd, float("nan")))
            dx, dw = _k10_bwd(lib, gd, xd, wd, torch.full_like(xd, float("nan")), torch.full_like(wd, float("nan")))
            _, dw2 = _k10_bwd(lib, gd, xd, wd, None, torch.full_like(wd, float("nan")))
            dw_wide = _wide_dw(lib, gd, xd, ci, co)
            torch.cuda.synchronize()
            tag = f"{ci}->{co} P={P}"
            y_ref, y_scale = fc.pw_ref(w, x)
            dx_ref, dx_scale = fc.pw_ref(w.t(), g)
            ry = fc.dot_bound_ratio(y.cpu(), y_ref, y_scale, ci)
            rdx = fc.dot_bound_ratio(dx.cpu(), dx_ref, dx_scale, co)
            dw_ref = torch.einsum("bop,bip->oi", g.double(), x.double())
            e = dw.double().cpu() - dw_ref
            d2, dmax = float(e.norm() / dw_ref.norm()), float(e.abs().max() / dw_ref.abs().max())
            fy, fdx = fc.k10_inst(lib, B, co, ci, P)[0], fc.k10_inst(lib, B, ci, co, P)[0]
            print(f"PWFAM k10 {tag}: y {fy} ratio {ry:.3f}  dx {fdx} ratio {rdx:.3f}  dW 2-norm {d2:.3e} max-norm {dmax:.3e}")
            worst = max(worst, ry, rdx)
            for name, t in (("y", y), ("dx", dx), ("dw", dw)):
                if not bool(torch.isfinite(t).all()):
                    fails.append(f"{tag} {name}: not finite (a NaN of the prefill was left or read)")
            if not ry <= 1.0:
                fails.append(f"{tag} y {fy}: an element is {ry:.3f} x the dot-product bound off")
            if not rdx <= 1.0:
                fails.append(f"{tag} dx {fdx}: an element is {rdx:.3f} x the dot-product bound off")
            if not (d2 <= TOL and dmax <= TOL):
                fails.append(f"{tag} dW: 2-norm {d2:.3e}, max-norm {dmax:.3e}")
            if not torch.equal(dw, dw2):
                fails.append(f"{tag} dW: two calls differ")
            if not torch.equal(dw, dw_wide):
                fails.append(f"{tag} dW: not cabinet_pwconv_wide_wgrad's bits")
            ran += 1
    print(f"PWFAM k10 group co{mbo} ci{mbi}: worst |a - ref| / (K 2^-23 |A||X|) = {worst:.3f}")
    _report(fails, ran, 3 * _MB_COUNT[mbo] * _MB_COUNT[mbi])


# ================================================================================================ b. K10, the three forms
@pytest.mark.parametrize("mb", [1, 2, 3, 4])
def test_k10_three_vector_forms_agree(mb):
    """The chain of an output element is the same whatever V (the kernel's header): accumulator from 0, k ascending in pairs."""
    lib = fc.load_library()
    cases = [(ci, co) for ci, co in fc.k10_form_cases(lib) if -(-co // 32) == mb]
    fails, ran = [], 0
    B, P = fc.K10_B, fc.K10_FORM_P
    for ci, co in cases:
        x, w, g = _k10_inputs(B, ci, co, P)
        wd = w.cuda()
        ys, dxs, forms = [], [], []
        for off in fc.K10_FORM_OFFSETS:
            xd, gd = _at_offset(x.shape, off, x), _at_offset(g.shape, off, g)
            ys.append(_k10_fwd(lib, xd, wd, _at_offset(g.shape, off)))
            dxs.append(_k10_bwd(lib, gd, xd, wd, _at_offset(x.shape, off), None)[0])
            forms.append((fc.k10_inst(lib, B, co, ci, P, off, off)[0], fc.k10_inst(lib, B, ci, co, P, off, off)[0]))
        torch.cuda.synchronize()
        print(f"PWFAM k10 forms {ci}->{co}: " + "  ".join(f"+{o}: y {f[0]} dx {f[1]}" for o, f in zip(fc.K10_FORM_OFFSETS, forms)))
        for name, ts in (("y", ys), ("dx", dxs)):
            if not all(bool(torch.isfinite(t).all()) for t in ts):
                fails.append(f"{ci}->{co} {name}: not finite")
            for i in (1, 2):
                if not torch.equal(ts[0], ts[i]):
                    fails.append(f"{ci}->{co} {name}: offset {fc.K10_FORM_OFFSETS[i]} differs from the aligned call in "
                                 f"{int((ts[0] != ts[i]).sum())} elements")
        y_ref, y_scale = fc.pw_ref(w, x)
        r = fc.dot_bound_ratio(ys[0].cpu(), y_ref, y_scale, ci)
        if not r <= 1.0:
            fails.append(f"{ci}->{co} y: {r:.3f} x the dot-product bound")
        ran += 1
    _report(fails, ran, {1: 8, 2: 8, 3: 4, 4: 4}[mb])


# ================================================================================================ c. K10, loaded walks
_LOADED = sorted(fc.k10_expected_instantiations())


def _sha(t):
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("inst", _LOADED, ids=["-".join(str(v) for v in i) for i in _LOADED])
def test_k10_loaded_walks(inst):
    lib = fc.load_library()
    form, mb, kq, v = inst
    if form == "pipe":
        (m, k), P = fc.k10_rep_product(mb, kq), fc.K10_LOADED_P[v]
    else:
        (m, k), P = (fc.k10_rep_product(1, 5), fc.K10_PLAIN_LOADED_P) if mb == 1 else (fc.k10_rep_product(2, 2), fc.K10_LOADED_P[2])
    ci, co, B = k, m, fc.K10_LOADED_B
    assert (ci, co, P) in fc.k10_loaded_cases(lib)
    got, nblocks = fc.k10_inst(lib, B, co, ci, P)
    assert got == inst and nblocks == (fc.K10_LOADED_BLOCKS if (form, mb) != ("plain", 1) else 4095)
    gen = torch.Generator(device="cuda").manual_seed(7919 * ci + 31 * co + v)
    x = torch.randn(B, ci, P, device="cuda", generator=gen)
    w = torch.randn(co, ci, device="cuda", generator=gen) * ci ** -0.5
    assert x.data_ptr() % 16 == 0
    y1 = _k10_fwd(lib, x, w, torch.full((B, co, P), float("nan"), device="cuda"))
    y2 = _k10_fwd(lib, x, w, torch.full((B, co, P), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y1).all()), "not finite (a NaN of the prefill was left or read)"
    ref, scale = fc.pw_ref(w, x)  # fp64 einsum on the device: independent of every kernel here
    ratio = fc.dot_bound_ratio(y1, ref, scale, ci)
    dist = float((y1.double() - ref).norm() / ref.norm())
    del ref, scale
    print(f"PWFAM k10 loaded {inst} {ci}->{co} P={P} blocks={nblocks}: worst |a - ref| / (K 2^-23 |A||X|) = {ratio:.3f}, "
          f"2-norm distance {dist:.3e}")
    h1, h2 = _sha(y1), _sha(y2)
    del x, w, y1, y2
    torch.cuda.empty_cache()
    assert ratio <= 1.0, f"an element is {ratio:.3f} x the dot-product bound off: a row stored from the wrong registers?"
    assert h1 == h2, "two runs differ"


@pytest.mark.parametrize("case,inst", fc.K10_LOADED_DX_CASES, ids=["-".join(str(v) for v in i) for _, i in fc.K10_LOADED_DX_CASES])
def test_k10_loaded_walks_input_gradient(case, inst):
    """cabinet_pwconv_bwd's dx under the same load: A = W^T read through its strides, one case per vector form."""
    lib = fc.load_library()
    (ci, co, P), B = case, fc.K10_LOADED_B
    assert fc.k10_inst(lib, B, ci, co, P) == (inst, fc.K10_LOADED_BLOCKS)
    gen = torch.Generator(device="cuda").manual_seed(104729 * ci + 37 * co)
    g = torch.randn(B, co, P, device="cuda", generator=gen)
    x = torch.randn(B, ci, P, device="cuda", generator=gen)  # read by the weight gradient only, which is not requested
    w = torch.randn(co, ci, device="cuda", generator=gen) * ci ** -0.5
    dx1 = _k10_bwd(lib, g, x, w, torch.full_like(x, float("nan")), None)[0]
    dx2 = _k10_bwd(lib, g, x, w, torch.full_like(x, float("nan")), None)[0]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx1).all()), "not finite (a NaN of the prefill was left or read)"
    ref, scale = fc.pw_ref(w.t(), g)
    ratio = fc.dot_bound_ratio(dx1, ref, scale, co)
    dist = float((dx1.double() - ref).norm() / ref.norm())
    del ref, scale
    print(f"PWFAM k10 loaded dx {inst} {ci}->{co} P={P}: worst |a - ref| / (K 2^-23 |A||X|) = {ratio:.3f}, 2-norm distance {dist:.3e}")
    h1, h2 = _sha(dx1), _sha(dx2)
    del g, x, w, dx1, dx2
    torch.cuda.empty_cache()
    assert ratio <= 1.0, f"an element is {ratio:.3f} x the dot-product bound off: a row stored from the wrong registers?"
    assert h1 == h2, "two runs differ"


# ================================================================================================ d. the routed small-backbone layer
@pytest.mark.parametrize("Ci,Co", [(16, 72), (16, 16)])
def test_small_backbone_expand_through_functional(Ci, Co):
    """MOBILENETV3_CFGS["small"], features.1: 16 -> 72 on the 256 x 256 plane of a 1024 x 1024 input (forward <3,1,2>, which no
    other shape of the suite launches) and the 16 -> 16 of the same plane."""
    import cabinet_amd.functional as Fh

    lib = fc.load_library()
    H = W = 256
    assert fc.k10_inst(lib, 1, Co, Ci, H * W)[0] == ("pipe", -(-Co // 32), 1, 2 if Co == 72 else 4)
    gen = torch.Generator().manual_seed(Ci + Co)
    conv = torch.nn.Conv2d(Ci, Co, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(Co, Ci, 1, 1, generator=gen) * Ci ** -0.5)
    x, g = torch.randn(1, Ci, H, W, generator=gen), torch.randn(1, Co, H, W, generator=gen)
    w = conv.weight.detach().clone().view(Co, Ci)
    conv = conv.cuda()
    xd = x.cuda().requires_grad_(True)
    assert Fh.pwconv_supported(conv, xd)
    y = Fh.pwconv(xd, conv)
    y.backward(g.cuda())
    torch.cuda.synchronize()
    y_ref, y_scale = fc.pw_ref(w, x.flatten(2))
    dx_ref, dx_scale = fc.pw_ref(w.t(), g.flatten(2))
    ry = fc.dot_bound_ratio(y.detach().cpu().flatten(2), y_ref, y_scale, Ci)
    rdx = fc.dot_bound_ratio(xd.grad.cpu().flatten(2), dx_ref, dx_scale, Co)
    dw_ref = torch.einsum("bop,bip->oi", g.flatten(2).double(), x.flatten(2).double())
    e = conv.weight.grad.double().cpu().view(Co, Ci) - dw_ref
    d2, dmax = float(e.norm() / dw_ref.norm()), float(e.abs().max() / dw_ref.abs().max())
    print(f"PWFAM routed {Ci}->{Co} 256x256: y ratio {ry:.3f} dx ratio {rdx:.3f} dW 2-norm {d2:.3e} max-norm {dmax:.3e}")
    assert torch.isfinite(y).all() and torch.isfinite(xd.grad).all() and torch.isfinite(conv.weight.grad).all()
    assert ry <= 1.0 and rdx <= 1.0, (ry, rdx)
    assert d2 <= TOL and dmax <= TOL, (d2, dmax)


# ================================================================================================ e. the BN form
def _bn_pairs():
    seen = []
    for c in fc.bn_act_cases():
        if (c[1], c[2]) not in seen:
            seen.append((c[1], c[2]))
    return seen


def _bn_case(lib, case, fails, tag=None):
    """One closing-BN case with the criteria of test_gpu_pw_bn_bwd.py::test_closing_bn_form; misses appended."""
    import test_gpu_pw_bn_bwd as tb

    B, Ci, Co, P, act, training, mis, want_dx, want_dw = case
    tag = tag or bnc.key(case)
    cpu = bnc.act_inputs(B, Ci, Co, P)
    dev = {k: bnc.on_device(v, mis == 2 or (mis == 1 and k == "x")) for k, v in cpu.items()}
    runs = [bnc.run_act_fused(lib, dev, B, Ci, Co, P, act, training, want_dx, want_dw, mis == 1, mis == 2) for _ in range(2)]
    chain = bnc.run_act_chain(lib, dev, B, Ci, Co, P, act, training)
    torch.cuda.synchronize()
    for name, a, b in zip(("dx", "dw", "dgamma", "dbeta"), *runs):
        if not ((a is None and b is None) or torch.equal(a, b)):
            fails.append(f"{tag} {name}: two runs differ")
    dx, dw, dgam, dbet = runs[0]
    if (dx is None) != (not want_dx) or (dw is None) != (not want_dw):
        fails.append(f"{tag}: an output that was not requested came back, or the reverse")
    if not (torch.equal(dgam, chain[2]) and torch.equal(dbet, chain[3])):
        fails.append(f"{tag}: dgamma / dbeta are not the chain's bits")
    ref = bnc.bn_pw_ref(cpu["g"], cpu["z"], cpu["x"], cpu["w"], cpu["gamma"], cpu["beta"], cpu["mean"], cpu["invstd"], act, training)
    if not (bnc.dist(dgam, ref["dgamma"]) <= bnc.TOL and bnc.dist(dbet, ref["dbeta"]) <= bnc.TOL):
        fails.append(f"{tag}: dgamma / dbeta off fp64")
    try:
        tb._check_pair("PWFAM " + tag, {"dx": dx, "dw": dw}, {"dx": chain[0], "dw": chain[1]}, ref, ("dx", "dw"))
    except AssertionError as e:
        fails.append(str(e))
    return runs[0], chain, ref


@pytest.mark.parametrize("Ci,Co", _bn_pairs(), ids=[f"{a}-{b}" for a, b in _bn_pairs()])
def test_bn_form_closing_cases(Ci, Co):
    lib = fc.load_library()
    cases = [c for c in fc.bn_act_cases() if (c[1], c[2]) == (Ci, Co)]
    fails = []
    for case in cases:
        assert lib.cabinet_pw_bn_bwd_supported(Ci, Co, case[3]) == 1
        _bn_case(lib, case, fails)
    expected = (6 if (Ci, Co) in fc.BN_PAIRS else 1) + sum((Ci, Co) == p for p in ((72, 40), (40, 72), (96, 64)))
    _report(fails, len(cases), expected)


@pytest.mark.parametrize("case", fc.BN_IDENTITY_CASES, ids=bnc.key)
def test_bn_form_rectangular_identity_gives_the_chains_dz(case):
    """W = eye(Co, Ci): row i < min(Ci, Co) of dx is row i of the dz the chain's dx pass writes, bit for bit; further rows of dx (Ci >
    Co) are exact zeros -- the staged expression, its scalars, and zeros (not the dz of zero operands) past P and Co."""
    B, Ci, Co, P, act, training = case
    lib = fc.load_library()
    cpu = bnc.act_inputs(B, Ci, Co, P, identity=True)
    assert torch.equal(cpu["w"], torch.eye(Co, Ci))
    dev = {k: bnc.on_device(v) for k, v in cpu.items()}
    dx, dw, _, _ = bnc.run_act_fused(lib, dev, B, Ci, Co, P, act, training)
    chain = bnc.run_act_chain(lib, dev, B, Ci, Co, P, act, training)
    torch.cuda.synchronize()
    m, dz = min(Ci, Co), chain[4]
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all()
    assert torch.equal(dx[:, :m], dz[:, :m]), f"dx differs from the chain's dz in {int((dx[:, :m] != dz[:, :m]).sum())} elements"
    assert not dx[:, m:].any(), "rows of dx past Co are not exact zeros"
    assert torch.equal(dw, chain[1]), "dW (same staged dz, same plan) differs from the chain's"
    ref = bnc.bn_pw_ref(cpu["g"], cpu["z"], cpu["x"], cpu["w"], cpu["gamma"], cpu["beta"], cpu["mean"], cpu["invstd"], act, training)
    d, d0 = bnc.dist(dw, ref["dw"]), bnc.dist(chain[1], ref["dw"])
    print(f"PWFAM identity {bnc.key(case)} dw: fused {d:.3e} chain {d0:.3e} from fp64")
    assert d <= bnc.TOL and d <= bnc.bound(d0)


def test_bn_form_depthwise_cases():
    import test_gpu_pw_bn_bwd as tb

    lib = fc.load_library()
    fails, ran = [], 0
    for case in fc.BN_DW_CASES:
        B, Ci, C, H, W, K, stride, act, training = case
        tag = "PWFAM " + bnc.key(case)
        cpu = bnc.dw_inputs(B, Ci, C, H, W, K, stride)
        dev = {k: bnc.on_device(v) for k, v in cpu.items()}
        runs = [bnc.run_dw_fused(lib, dev, B, Ci, C, H, W, K, stride, act, training) for _ in range(2)]
        chain = bnc.run_dw_chain(lib, dev, B, Ci, C, H, W, K, stride, act, training)
        torch.cuda.synchronize()
        if not all(torch.equal(a, b) for a, b in zip(*runs)):
            fails.append(f"{tag}: two runs differ")
        dx, dw, dgam, dbet, dcw = runs[0]
        if not (torch.equal(dgam, chain[2]) and torch.equal(dbet, chain[3]) and torch.equal(dcw, chain[4])):
            fails.append(f"{tag}: dgamma / dbeta / the depthwise dW are not the chain's bits")
        ref = bnc.dw_ref(cpu, K, stride, act, training)
        if not bnc.dist(dcw, ref["dcw"]) <= bnc.TOL:
            fails.append(f"{tag}: depthwise dW off fp64")
        try:
            tb._check_pair(tag, {"dx": dx, "dw": dw}, {"dx": chain[0], "dw": chain[1]}, ref, ("dx", "dw"))
        except AssertionError as e:
            fails.append(str(e))
        ran += 1
    _report(fails, ran, 7)


@pytest.mark.parametrize("case", fc.BN_LOADED_CASES, ids=["2-3", "3-2"])
def test_bn_form_big_lds_instantiations_loaded(case):
    """<2,3> and <3,2> on the full grid, as test_gpu_pw_bn_bwd.py::test_loaded_chip_digest runs <2,1>: one digest for two runs, the
    bound against the chain, and no dx element further off than 1e-4 of the largest."""
    lib = fc.load_library()
    fails = []
    (dx, dw, _, _), chain, ref = _bn_case(lib, case, fails, tag="loaded " + bnc.key(case))
    assert not fails, "\n".join(fails)
    worst = float((dx.double().cpu().flatten(1) - ref["dx"].flatten(1)).abs().max())
    assert worst <= 1e-4 * float(ref["dx"].abs().max()), f"a dx element is off by {worst:.3e}: a row stored from the wrong registers?"


# ================================================================================================ f. K14
_K14_PAIRS = fc.K14_NEW_PAIRS + fc.K14_LARGE_PAIRS + fc.K14_OTHER_PAIRS


@pytest.mark.parametrize("Ci,Co", _K14_PAIRS, ids=[f"{a}-{b}" for a, b in _K14_PAIRS])
def test_k14_tile_shapes(Ci, Co):
    """The criteria of test_gpu_pwconv_wide.py: 1e-3 from fp64 and at most twice the stock operator's distance; two calls equal."""
    import test_gpu_pwconv_wide as tw
    from conftest import rel_err

    lib = fc.load_library()
    cases = [c for c in fc.k14_cases() if (c[1], c[2]) == (Ci, Co)]
    fails = []
    for B, _, _, P in cases:
        H, W = {323: (17, 19), 64 * 65: (64, 65)}[P]
        g0 = torch.Generator().manual_seed(Ci * 1000 + Co + P)
        x, g, w = torch.randn(B, Ci, H, W, generator=g0), torch.randn(B, Co, H, W, generator=g0), torch.randn(Co, Ci, 1, 1, generator=g0)
        ref = torch.einsum("bop,bip->oi", g.flatten(2).double(), x.flatten(2).double())
        xd, gd, wd = x.cuda(), g.cuda(), w.cuda()
        dw, dw2 = tw._native_dw(gd, xd, Ci, Co), tw._native_dw(gd, xd, Ci, Co)
        stock = tw._stock_dw(gd, xd, wd).view(Co, Ci)
        torch.cuda.synchronize()
        e_native, e_stock = rel_err(dw, ref), rel_err(stock, ref)
        plan = fc.wide_plan(lib, B, Ci, Co, P)
        print(f"PWFAM k14 B={B} {Ci}->{Co} P={P} plan {plan}: native {e_native:.3e}  stock {e_stock:.3e}")
        if not bool(torch.isfinite(dw).all()):
            fails.append(f"B={B} P={P}: not finite")
        if not e_native <= TOL:
            fails.append(f"B={B} P={P}: {e_native:.3e} > {TOL}")
        if not e_native <= 2.0 * e_stock:
            fails.append(f"B={B} P={P}: native {e_native:.3e} > 2 x stock {e_stock:.3e}")
        if not torch.equal(dw, dw2):
            fails.append(f"B={B} P={P}: two calls differ")
    _report(fails, len(cases), 1 if (Ci, Co) in fc.K14_OTHER_PAIRS else 2)


# ================================================================================================ g. SE MLP adjoint
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("P", fc.SE_PS)
@pytest.mark.parametrize("shape", fc.SE_SHAPES, ids=["-".join(map(str, s)) for s in fc.SE_SHAPES])
def test_se_mlp_bwd_off_the_production_shapes(shape, P, training):
    import test_gpu_se_mlp_bwd as ts

    print(f"PWFAM se {shape} P={P} training={training}")
    t = ts._inputs(*shape, **fc.se_input_args(shape))
    ref = ts._fp64(t, P, training)
    assert ref["dw1"].any() and ref["dw2"].any() and ref["ds"].any(), "no live hidden unit: the contractions would multiply zeros"
    ts._check_case(t, P, training)


@pytest.mark.parametrize("shape", fc.SE_POISON_SHAPES, ids=["-".join(map(str, s)) for s in fc.SE_POISON_SHAPES])
def test_se_mlp_bwd_owns_its_outputs(shape):
    """Two runs bit-equal; NaN-filled outputs and workspace change nothing and nothing stays NaN."""
    import test_gpu_se_mlp_bwd as ts

    t = ts._inputs(*shape, **fc.se_input_args(shape))
    a, b, c = ts._fused(t, 1024, 1), ts._fused(t, 1024, 1), ts._fused(t, 1024, 1, poison=True)
    assert a["dw1"].any() and a["dw2"].any() and a["ds"].any(), "no live hidden unit"
    for k in ts.OUT:
        assert torch.equal(a[k], b[k]), k
        assert torch.isfinite(c[k]).all() and torch.equal(a[k], c[k]), k
