"""Cases, inputs, fp64 formulas and C-ABI drivers for the fused backward of a thin 1x1 convolution and the BatchNorm behind it
(cabinet_pw_bn_act_bwd / cabinet_pw_bn_dwconv_bwd, csrc/pwconv_wide.hip "BN form").  No device work at import.

The C entry points take z, save_mean and save_invstd as inputs, so the tests choose them: mean 0.5 and invstd 2 are exact, a z
element equal to the mean has xhat = 0 and its pre-activation is beta, and beta = 0, -3, +3 in channels 0, 1, 2 puts those
elements on the ReLU boundary (u = 0) and on hardswish's t = u + 3 = 0 and t = 6.  gamma has a zero and negative entries."""
import hashlib

import torch
import torch.nn.functional as F

ACTS = {"none": 0, "relu": 1, "hardswish": 2}
ROUNDING = 2.0 ** -23  # one fp32 rounding: the K10 tests' floor where the chain's own distance is 0
TOL = 1e-3

# closing-BN form: (B, Ci, Co, P, act, training, misalign, want_dx, want_dw)
#   misalign: 0 none | 1 x and dx start 4 bytes into their allocation (P % 4 == 0: the dword store path on an aligned-size plane)
#           | 2 every tensor does (odd P only: the BatchNorm reduce reads 16 bytes at a time where P % 4 == 0)
ACT_CASES = [
    (1, 8, 8, 1, "relu", True, 0, True, True),          # one chunk, one split
    (2, 8, 8, 5, "hardswish", True, 0, True, True),
    (3, 16, 16, 63, "none", True, 0, True, True),
    (1, 16, 16, 64, "relu", False, 0, True, True),
    (2, 16, 64, 65, "hardswish", False, 0, True, True),
    (3, 64, 24, 127, "none", False, 0, True, True),
    (1, 24, 72, 129, "relu", True, 0, True, True),
    (2, 72, 24, 449, "hardswish", True, 0, True, True),
    (3, 96, 96, 1000, "relu", True, 0, True, True),     # <3,3>: W in 38 KB of LDS, one workgroup per CU
    (1, 16, 64, 4099, "none", True, 0, True, True),
    (2, 96, 96, 64, "hardswish", True, 0, True, True),
    (3, 24, 72, 4099, "hardswish", True, 0, True, True),
    (1, 72, 24, 1000, "relu", False, 0, True, True),
    (2, 64, 24, 129, "relu", True, 0, True, True),
    (2, 16, 64, 449, "relu", True, 0, True, True),
    (2, 16, 64, 449, "none", True, 0, True, True),
    (2, 16, 64, 449, "hardswish", False, 0, True, True),
    (2, 24, 72, 127, "relu", True, 0, False, True),     # dX not requested
    (2, 24, 72, 127, "relu", True, 0, True, False),     # dW not requested
    (3, 72, 24, 1000, "hardswish", True, 0, False, True),
    (2, 16, 16, 1000, "relu", True, 1, True, True),     # base pointers of x and dx offset by 4 bytes
    (2, 16, 64, 129, "hardswish", True, 2, True, True),  # every base pointer offset by 4 bytes
]
IDENTITY_CASES = [(2, 16, 65, "relu", True), (3, 64, 1000, "hardswish", True), (1, 16, 4099, "none", False),
                  (2, 64, 129, "relu", False)]  # (B, C, P, act, training): W = I, dx must be the chain's dz

# depthwise form: (B, Ci, C, H, W, K, stride, act, training)
DW_CASES = [
    (1, 16, 64, 1, 1, 3, 1, "relu", True),
    (2, 24, 72, 1, 1, 5, 2, "hardswish", True),
    (3, 8, 8, 1, 1, 3, 2, "none", False),
    (1, 16, 16, 1, 1, 5, 1, "relu", False),
    (2, 16, 64, 7, 9, 3, 2, "relu", True),
    (3, 24, 72, 7, 9, 3, 1, "relu", True),
    (1, 24, 72, 7, 9, 5, 2, "hardswish", True),
    (2, 96, 96, 7, 9, 5, 1, "none", True),
    (3, 16, 64, 33, 65, 3, 2, "relu", True),
    (1, 24, 72, 33, 65, 3, 1, "hardswish", False),
    (2, 72, 24, 33, 65, 5, 2, "relu", True),
    (1, 64, 24, 33, 65, 5, 1, "hardswish", True),
]

# one launch of the full grid (512 workgroups, every one resident: two per CU) with four or five chunks each: the store hazard of
# DESIGN.md K10 showed on a loaded chip only.  The plan never launches more than 512 workgroups, so "more than the resident
# workgroups" cannot be had from one launch; this is the launch that backs the memory pipeline up as the production layers do.
LOADED_CASE = (1, 16, 64, 64 * 2103 + 36, "relu", True, 0, True, True)


def key(case):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case)


def _params(C, gen):
    gamma = torch.randn(C, generator=gen)
    gamma[3 % C] = 0.0
    gamma[5 % C] = -abs(gamma[5 % C]) - 0.1
    beta = torch.randn(C, generator=gen) * 0.5
    beta[0], beta[1 % C], beta[2 % C] = 0.0, -3.0, 3.0
    if C > 2:
        assert (beta[:3] == torch.tensor([0.0, -3.0, 3.0])).all()
    return gamma, beta, torch.full((C,), 0.5), torch.full((C,), 2.0)


def _on_boundary(z):
    zf = z.reshape(z.shape[0], z.shape[1], -1)
    zf[:, :3, ::7] = 0.5  # xhat = 0: the pre-activation is beta exactly
    return z


def act_inputs(B, Ci, Co, P, seed=0, identity=False):
    """-> dict of CPU fp32 tensors: x (B,Ci,P), w (Co,Ci), z = W x (rounded), g, gamma, beta, mean, invstd."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * Ci + 13 * Co + P + B)
    x = torch.randn(B, Ci, P, generator=gen)
    w = torch.eye(Co, Ci) if identity else torch.randn(Co, Ci, generator=gen) / Ci ** 0.5
    z = _on_boundary(torch.einsum("oi,bip->bop", w, x) * 0.5 + 0.5)
    g = torch.randn(B, Co, P, generator=gen)
    gamma, beta, mean, invstd = _params(Co, gen)
    return dict(x=x, w=w, z=z, g=g, gamma=gamma, beta=beta, mean=mean, invstd=invstd)


def dw_inputs(B, Ci, C, H, W, K, stride, seed=0):
    d = act_inputs(B, Ci, C, H * W, seed)
    gen = torch.Generator().manual_seed(seed + 99)
    Ho, Wo = (H + 2 * (K // 2) - K) // stride + 1, (W + 2 * (K // 2) - K) // stride + 1
    d["cw"] = torch.randn(C, 1, K, K, generator=gen) / K
    d["g"] = torch.randn(B, C, Ho, Wo, generator=gen)
    for k in ("x", "z"):
        d[k] = d[k].reshape(B, -1, H, W)
    return d


# ------------------------------------------------------------------------------------------------ fp64 formulas
def act_grad64(u, act):
    """The derivative conventions of csrc/act.hpp: ReLU' = [u > 0]; hardswish with relu6' = 1 on the open interval (0, 6)."""
    if act == "relu":
        return (u > 0).to(u.dtype)
    if act == "hardswish":
        t = u + 3.0
        return t.clamp(0.0, 6.0) / 6.0 + torch.where((t > 0) & (t < 6), u / 6.0, torch.zeros_like(u))
    return torch.ones_like(u)


def act_fwd64(u, act):
    if act == "relu":
        return u.clamp_min(0.0)
    if act == "hardswish":
        return u * (u + 3.0).clamp(0.0, 6.0) / 6.0
    return u


def bn_pw_ref(g, z, x, w, gamma, beta, mean, invstd, act, training):
    """fp64 backward of act(bn(z)) and of z = W x at the given statistics -> dict(dx, dw, dgamma, dbeta, dz).  Tensors (B, C, ...)."""
    g, z, x, w = g.double().flatten(2), z.double().flatten(2), x.double().flatten(2), w.double()
    c = lambda t: t.double().view(1, -1, 1)  # noqa: E731
    xh = (z - c(mean)) * c(invstd)
    du = g * act_grad64(xh * c(gamma) + c(beta), act)
    dbeta, dgamma = du.sum((0, 2)), (du * xh).sum((0, 2))
    n = z.shape[0] * z.shape[2]
    m1, m2 = (dbeta / n, dgamma / n) if training else (torch.zeros_like(dbeta), torch.zeros_like(dgamma))
    dz = c(gamma) * c(invstd) * (du - m1.view(1, -1, 1) - xh * m2.view(1, -1, 1))
    return dict(dx=torch.einsum("oi,bop->bip", w, dz), dw=torch.einsum("bop,bip->oi", dz, x), dgamma=dgamma, dbeta=dbeta, dz=dz)


def dw_ref(d, K, stride, act, training):
    """fp64 backward of conv_dw(act(bn(z))), z = W x, at the given statistics -> dict(dx, dw, dgamma, dbeta, dcw)."""
    z, cw = d["z"].double(), d["cw"].double()
    c = lambda t: t.double().view(1, -1, 1, 1)  # noqa: E731
    a = act_fwd64((z - c(d["mean"])) * c(d["invstd"]) * c(d["gamma"]) + c(d["beta"]), act).requires_grad_(True)
    cw = cw.requires_grad_(True)
    F.conv2d(a, cw, None, stride, K // 2, 1, z.shape[1]).backward(d["g"].double())
    out = bn_pw_ref(a.grad, z, d["x"], d["w"], d["gamma"], d["beta"], d["mean"], d["invstd"], act, training)
    out["dcw"] = cw.grad
    return out


def dist(a, ref):
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def bound(d_chain):
    """The issue's rule: twice the chain's own distance from fp64; where that is 0, twice one fp32 rounding."""
    return 2.0 * (d_chain if d_chain > 0 else ROUNDING)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ device side
def load_library():
    from cabinet_amd import _lib

    return _lib.load()


def on_device(t, misaligned=False):
    """A dense device copy; `misaligned`: it starts 4 bytes into its allocation."""
    if not misaligned:
        return t.cuda().contiguous()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def nan_like(t, misaligned=False):
    return on_device(torch.full(t.shape, float("nan"), dtype=t.dtype), misaligned)


def _ws(nbytes):
    return torch.full((max(nbytes, 4) // 4 + 1,), float("nan"), dtype=torch.float32, device="cuda"), nbytes


def run_act_fused(lib, dev, B, Ci, Co, P, act, training, want_dx=True, want_dw=True, mis_x=False, mis_all=False):
    """cabinet_pw_bn_act_bwd on NaN-prefilled outputs and workspace -> (dx, dw, dgamma, dbeta)."""
    from cabinet_amd.functional import _ptr, _stream_handle

    dx = nan_like(dev["x"], mis_x or mis_all) if want_dx else None
    dw = nan_like(dev["w"], mis_all) if want_dw else None
    dgam, dbet = nan_like(dev["gamma"]), nan_like(dev["beta"])
    ws, nbytes = _ws(lib.cabinet_pw_bn_act_bwd_workspace_bytes(B, Ci, Co, P))
    rc = lib.cabinet_pw_bn_act_bwd(_ptr(dev["g"]), _ptr(dev["z"]), _ptr(dev["x"]), _ptr(dev["w"]), _ptr(dev["gamma"]),
                                   _ptr(dev["beta"]), _ptr(dev["mean"]), _ptr(dev["invstd"]), B, Ci, Co, P, ACTS[act],
                                   int(training), _ptr(dx), _ptr(dw), _ptr(dgam), _ptr(dbet), _ptr(ws), nbytes,
                                   _stream_handle(dgam.device))
    assert rc == 0, lib.cabinet_last_error()
    return dx, dw, dgam, dbet


def pw_bwd_chain(lib, dz, x, w, B, Ci, Co, P):
    """The parent's backward of the 1x1 convolution on a stored dz: cabinet_pwconv_bwd where K10 takes the shape, else (96 x 96)
    what the model runs for such a layer: K14's weight gradient and the stock product for dx."""
    from cabinet_amd.functional import _ptr, _stream_handle

    dx, dw = nan_like(x), nan_like(w)
    if lib.cabinet_pwconv_supported(Ci, Co, P):
        ws, nbytes = _ws(lib.cabinet_pwconv_bwd_workspace_bytes(B, Ci, Co, P))
        rc = lib.cabinet_pwconv_bwd(_ptr(dz), _ptr(x), _ptr(w), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes,
                                    _stream_handle(x.device))
        assert rc == 0, lib.cabinet_last_error()
    else:
        ws, nbytes = _ws(lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, Ci, Co, P))
        rc = lib.cabinet_pwconv_wide_wgrad(_ptr(dz), _ptr(x), B, Ci, Co, P, _ptr(dw), _ptr(ws), nbytes, _stream_handle(x.device))
        assert rc == 0, lib.cabinet_last_error()
        dx = torch.einsum("oi,bop->bip", w, dz.reshape(B, Co, P)).reshape(x.shape)
    return dx, dw


def run_act_chain(lib, dev, B, Ci, Co, P, act, training):
    """cabinet_bn_act_bwd, then the convolution's backward on the dz it stored -> (dx, dw, dgamma, dbeta, dz).  Aligned copies."""
    from cabinet_amd.functional import _ptr, _stream_handle

    a = {k: v.clone() for k, v in dev.items()}  # clone(): a fresh, aligned allocation
    dz, dgam, dbet = nan_like(a["z"]), nan_like(a["gamma"]), nan_like(a["beta"])
    ws, nbytes = _ws(lib.cabinet_bn_act_workspace_bytes(B, Co, P))
    rc = lib.cabinet_bn_act_bwd(_ptr(a["g"]), _ptr(a["z"]), _ptr(a["gamma"]), _ptr(a["beta"]), _ptr(a["mean"]), _ptr(a["invstd"]),
                                B, Co, P, ACTS[act], int(training), _ptr(dz), _ptr(dgam), _ptr(dbet), _ptr(ws), nbytes,
                                _stream_handle(dz.device))
    assert rc == 0, lib.cabinet_last_error()
    dx, dw = pw_bwd_chain(lib, dz, a["x"], a["w"], B, Ci, Co, P)
    return dx, dw, dgam, dbet, dz


def run_dw_fused(lib, dev, B, Ci, C, H, W, K, stride, act, training):
    from cabinet_amd.functional import _ptr, _stream_handle

    dx, dw, dgam, dbet, dcw = (nan_like(dev[k]) for k in ("x", "w", "gamma", "beta", "cw"))
    ws, nbytes = _ws(lib.cabinet_pw_bn_dwconv_bwd_workspace_bytes(B, Ci, C, H, W, K, stride))
    rc = lib.cabinet_pw_bn_dwconv_bwd(_ptr(dev["g"]), _ptr(dev["z"]), _ptr(dev["x"]), _ptr(dev["w"]), _ptr(dev["gamma"]),
                                      _ptr(dev["beta"]), _ptr(dev["mean"]), _ptr(dev["invstd"]), _ptr(dev["cw"]), B, Ci, C, H, W,
                                      K, stride, ACTS[act], int(training), _ptr(dx), _ptr(dw), _ptr(dgam), _ptr(dbet), _ptr(dcw),
                                      _ptr(ws), nbytes, _stream_handle(dx.device))
    assert rc == 0, lib.cabinet_last_error()
    return dx, dw, dgam, dbet, dcw


def run_dw_chain(lib, dev, B, Ci, C, H, W, K, stride, act, training):
    from cabinet_amd.functional import _ptr, _stream_handle

    dz, dgam, dbet, dcw = (nan_like(dev[k]) for k in ("z", "gamma", "beta", "cw"))
    ws, nbytes = _ws(lib.cabinet_bn_dwconv_bwd_workspace_bytes(B, C, H, W, K, stride))
    rc = lib.cabinet_bn_dwconv_bwd(_ptr(dev["g"]), _ptr(dev["z"]), _ptr(dev["gamma"]), _ptr(dev["beta"]), _ptr(dev["mean"]),
                                   _ptr(dev["invstd"]), _ptr(dev["cw"]), B, C, H, W, K, stride, ACTS[act], int(training),
                                   _ptr(dz), _ptr(dgam), _ptr(dbet), _ptr(dcw), _ptr(ws), nbytes, _stream_handle(dz.device))
    assert rc == 0, lib.cabinet_last_error()
    dx, dw = pw_bwd_chain(lib, dz, dev["x"], dev["w"], B, Ci, C, H * W)
    return dx, dw, dgam, dbet, dcw
