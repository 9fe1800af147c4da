"""Autograd operators of the hot path, backed by libcabinet_hip.so on HIP tensors.

``cab_attention``   replaces reference src/models/cab.py:149-154          (K1 / K2)
``cab_qkv``         cab.py:137-146 (projections, BN, PSP)                 (K6)     ``conv1x1``  cab.py:155
``cab_local``       cab.py:182-184 and :213-216                           (K5)
``ffm_fused``       src/models/cabinet.py:142-153                         (K3 / K4; ``ffm_fused_upsampled`` + :228-230)
``bn_act``          cabinet.py:42-44 and every BatchNorm2d(+act) pair     (K7)     ``gate_act``  mobilenetv3.py:79-83
``se_tail``         mobilenetv3.py:146-149 (BatchNorm -> SELayer -> act: K7 + gate_act forward, two-pass backward)
``bn_relu_cls``     cabinet.py:90-92, :161-172 (BN -> ReLU -> 1x1 classifier)  (K12)   ``conv3x3``  cabinet.py:59, :88-89, :160 (K11)
``dwconv`` / ``bn_act_dwconv``   mobilenetv3.py:118-126,135-143           (K8)
``stem_conv``       cabinet.py:111                                        (K9)     ``pwconv``   mobilenetv3.py:128-131
``stem_conv_bn_relu``  cabinet.py:111 + :42-44 (the stem's conv -> BN -> ReLU as one node: K9 + K7, no BatchNorm dx pass)
OHEM head           src/utils/loss.py:51-80 + cabinet.py:240-245          (``ohem_up_*``, used by cabinet_amd.loss)
evaluation tail     src/scripts/evaluate.py:69-159, :193-226              (K13: ``eval_chip_accum`` / ``eval_scale_merge`` /
                    ``eval_argmax_hist``, no autograd; used by cabinet_amd.evaluate)
inference tail      src/scripts/visualize.py:50-61, :113-139, :165-177    (K17: ``predict_up_argmax`` / ``predict_argmax`` /
                    ``predict_render``, no autograd; used by cabinet_amd.predict)

ONE dispatch rule for every operator here:
  * device tensor, shape inside the kernel family's coverage (each family exports ``*_supported``): the hand-written
    HIP kernels run; a missing / mismatching library or a failing launch raises RuntimeError -- nothing is caught and
    retried on another path;
  * device tensor, shape outside the coverage (attention channel pairs other than (128,128) (256,128) (64,64); producers
    with channel counts that are not multiples of 16; depthwise kernels other than 3 / 5; the local branch only for planes
    wider than its LDS tile, > ~1800 columns -- every B*H*W is served: channel-resident kernel up to 8192 positions per
    channel, tiled multi-workgroup form above; the loss heads beyond 32 classes, a 60 KB row of C * Wl logits or a resize ratio
    whose segment buffers leave the LDS): the module's composite ATen forward, on the device -- the reference API accepts any
    channel count, so must this one;
  * host (CPU) tensors: the composite ATen forward, so modules stay usable for checkpoint surgery, EMA copies and CPU
    unit tests, exactly like any nn.Module.
"""

from __future__ import annotations

import ctypes as _ct

import torch
import torch.nn.functional as F

from . import _lib


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream_handle(device):
    return torch.cuda.current_stream(device).cuda_stream


def _workspace(nbytes, device):
    if nbytes == 0:
        return None, 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws, nbytes


def _aligned(t):
    """A dense tensor of any dtype at a 16-byte aligned address (labels, internal slices such as ``loss_px[1]``)."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() & 15 else t


def _f32c(t):
    """Borrowed inputs must be dense fp32 and 16-byte aligned (the rules the C ABI documents): a contiguous VIEW that starts
    4 or 8 bytes into its allocation (``x[1:]``, ``x.flatten()[1:]``) is copied."""
    if t.dtype != torch.float32:
        t = t.float()
    t = t.contiguous()
    if t.data_ptr() & 15:
        t = t.clone()
    return t


# --------------------------------------------------------------------------- attention core


PREC_FP32, PREC_BF16X3, PREC_BF16X6 = 0, 1, 2  # include/cabinet_hip.h: CABINET_PREC_*
_PRECISIONS = {"fp32": PREC_FP32, "bf16x3": PREC_BF16X3, "bf16x6": PREC_BF16X6}


def attn_fwd_hip(q, k, v, scale, precision=PREC_FP32):
    """q,k (B,Kc,n), v (B,Vc,n) fp32 device tensors -> ctx (B,Vc,n), lse (B,n)."""
    lib = _lib.load()
    B, Kc, n = q.shape
    Vc = v.shape[1]
    ctx = torch.empty((B, Vc, n), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, n), dtype=torch.float32, device=q.device)
    ws, nbytes = _workspace(lib.cabinet_cab_attn_fwd_workspace_bytes(B, Kc, Vc, n, int(precision)), q.device)
    with torch.cuda.device(q.device):
        rc = lib.cabinet_cab_attn_fwd(_ptr(q), _ptr(k), _ptr(v), float(scale), B, Kc, Vc, n, int(precision), _ptr(ctx),
                                      _ptr(lse), _ptr(ws), nbytes, _stream_handle(q.device))
    _lib.check(rc, "cabinet_cab_attn_fwd")
    return ctx, lse


def attn_bwd_hip(g, q, k, v, ctx, lse, scale):
    lib = _lib.load()
    B, Kc, n = q.shape
    Vc = v.shape[1]
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws, nbytes = _workspace(lib.cabinet_cab_attn_bwd_workspace_bytes(B, Kc, Vc, n), q.device)
    with torch.cuda.device(q.device):
        rc = lib.cabinet_cab_attn_bwd(_ptr(g), _ptr(q), _ptr(k), _ptr(v), _ptr(ctx), _ptr(lse), float(scale),
                                      B, Kc, Vc, n, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), nbytes,
                                      _stream_handle(q.device))
    _lib.check(rc, "cabinet_cab_attn_bwd")
    return dq, dk, dv


class _CabAttention(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, q, k, v, scale, precision):
        q, k, v = _f32c(q), _f32c(k), _f32c(v)
        out, lse = attn_fwd_hip(q, k, v, scale, precision)
        fn_ctx.save_for_backward(q, k, v, out, lse)
        fn_ctx.scale = scale
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        q, k, v, out, lse = fn_ctx.saved_tensors
        dq, dk, dv = attn_bwd_hip(_f32c(g), q, k, v, out, lse, fn_ctx.scale)
        return dq, dk, dv, None, None


def cab_attention_supported(Kc, Vc):
    """True for the (key, value) channel pairs K1 / K2 are instantiated for."""
    return bool(_lib.load().cabinet_cab_attn_supported(int(Kc), int(Vc)))


# Matrix arithmetic of K1's two contractions (include/cabinet_hip.h, CABINET_PREC_*): "fp32" = exact fp32 MFMA (default),
# "bf16x6" = fp32 operands as three bf16 pieces each, six bf16 MFMA products per fp32 product (fp32-level accuracy, 2.7x the
# matrix rate), "bf16x3" = two pieces, three products (~1e-5 per tensor; a measured variant).  Set per call, or process-wide
# through this module attribute / the environment variable CABINET_ATTN_PRECISION; channel pairs without a split-bf16
# instantiation always run fp32.
import os as _os  # noqa: E402

ATTN_PRECISION = _os.environ.get("CABINET_ATTN_PRECISION", "fp32")
# the same switch for the FFM's big forward product z = W_s . fsp + U(W_c . low) (cabinet_ffm_up_fwd); shapes without a
# split-bf16 instantiation run fp32 whatever is set
FFM_PRECISION = _os.environ.get("CABINET_FFM_PRECISION", "fp32")


def _ffm_precision():
    """``FFM_PRECISION`` -> CABINET_PREC_*; an unknown name raises (a typo such as ``bf16_6`` must not silently measure
    fp32), exactly as ``_resolve_precision`` does for the attention switch."""
    if FFM_PRECISION not in _PRECISIONS:
        raise RuntimeError(f"ffm_fused_upsampled: unknown CABINET_FFM_PRECISION {FFM_PRECISION!r} "
                           f"(one of {sorted(_PRECISIONS)})")
    return _PRECISIONS[FFM_PRECISION]


def _resolve_precision(precision, Kc, Vc):
    name = ATTN_PRECISION if precision is None else precision
    if name not in _PRECISIONS:
        raise RuntimeError(f"cab_attention: unknown precision {name!r} (one of {sorted(_PRECISIONS)})")
    code = _PRECISIONS[name]
    if code != PREC_FP32 and not _lib.load().cabinet_cab_attn_precision_supported(int(Kc), int(Vc), code):
        if precision is not None:
            raise RuntimeError(f"cab_attention: precision {name!r} is not built for (Kc={Kc}, Vc={Vc})")
        code = PREC_FP32
    return code


def cab_attention(q, k, v, scale, precision=None):
    """ctx[b,c,i] = sum_j softmax_j(scale * <q[b,:,i], k[b,:,j]>) v[b,c,j].

    q,k: (B,Kc,n)  v: (B,Vc,n)  ->  (B,Vc,n).   Reference: cab.py:149-154.
    ``precision``: None (module default ``ATTN_PRECISION``) | "fp32" | "bf16x6" | "bf16x3" -- forward contractions only; the
    backward (K2) is fp32 MFMA in every case.
    """
    if q.dim() != 3 or k.shape != q.shape or v.dim() != 3 or v.shape[0] != q.shape[0] or v.shape[2] != q.shape[2]:
        raise RuntimeError(f"cab_attention: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)}")
    if q.is_cuda and cab_attention_supported(q.shape[1], v.shape[1]):
        return _CabAttention.apply(q, k, v, float(scale), _resolve_precision(precision, q.shape[1], v.shape[1]))
    # host tensors, and channel pairs without a gfx950 instantiation: composite ATen ops (module docstring: one rule)
    attn = torch.bmm(q.transpose(1, 2), k) * scale
    attn = F.softmax(attn, dim=-1)
    return torch.bmm(v, attn.transpose(1, 2))


def attn_proj_fwd_hip(q, k, v, w2, scale, need_ctx=True):
    """q,k (B,Kc,n), v (B,Vc,n), w2 (Co,Vc) fp32 device tensors -> glob (B,Co,n), ctx (B,Vc,n) or None, lse (B,n): K1 with the output
    projection in its epilogue (cabinet_cab_attn_proj_fwd)."""
    lib = _lib.load()
    B, Kc, n = q.shape
    Vc, Co = v.shape[1], w2.shape[0]
    ctx = torch.empty((B, Vc, n), dtype=torch.float32, device=q.device) if need_ctx else None
    glob = torch.empty((B, Co, n), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, n), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        rc = lib.cabinet_cab_attn_proj_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(w2), float(scale), B, Kc, Vc, Co, n, _ptr(ctx),
                                           _ptr(glob), _ptr(lse), _stream_handle(q.device))
    _lib.check(rc, "cabinet_cab_attn_proj_fwd")
    return glob, ctx, lse


class _CabAttentionProj(torch.autograd.Function):
    """K1 with the CAB's output projection in its epilogue: ``project_out(attention(q, k, v))`` in ONE launch
    (cabinet_cab_attn_proj_fwd).  Backward = the projection's backward (cabinet_conv1x1_bwd: dctx, dw) + K2."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, q, k, v, w_out, scale):
        q, k, v = _f32c(q), _f32c(k), _f32c(v)
        w2 = _f32c(w_out.detach()).reshape(w_out.shape[0], -1)
        need_ctx = any(fn_ctx.needs_input_grad[:4])
        glob, ctx, lse = attn_proj_fwd_hip(q, k, v, w2, scale, need_ctx)
        if need_ctx:
            fn_ctx.save_for_backward(q, k, v, ctx, lse, w2)
        fn_ctx.scale, fn_ctx.w_shape = scale, w_out.shape
        return glob

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        q, k, v, ctx, lse, w2 = fn_ctx.saved_tensors
        g = _f32c(g)
        B, Vc, n = ctx.shape
        Co = w2.shape[0]
        need_attn, need_w = any(fn_ctx.needs_input_grad[:3]), fn_ctx.needs_input_grad[3]
        dctx = torch.empty_like(ctx) if need_attn else None
        dw = torch.empty_like(w2) if need_w else None
        ws, nbytes = _workspace(lib.cabinet_conv1x1_bwd_workspace_bytes(B, Vc, Co, n), g.device)
        with torch.cuda.device(g.device):
            rc = lib.cabinet_conv1x1_bwd(_ptr(g), _ptr(ctx), _ptr(w2), B, Vc, Co, n, _ptr(dctx), _ptr(dw), _ptr(ws), nbytes,
                                         _stream_handle(g.device))
        _lib.check(rc, "cabinet_conv1x1_bwd")
        dq = dk = dv = None
        if need_attn:
            dq, dk, dv = attn_bwd_hip(dctx, q, k, v, ctx, lse, fn_ctx.scale)
        return dq, dk, dv, (dw.reshape(fn_ctx.w_shape) if need_w else None), None


def cab_attention_proj_supported(q, v, w_out):
    """True when ``project_out(cab_attention(q, k, v))`` runs as ONE kernel (K1 with the projection in its epilogue): device
    tensors, the 8-wave kernel's channel pairs, n % 4 == 0, Co % 32 == 0, a batch the forward runs without a key split, fp32 MFMA
    (the split-bf16 precisions keep the two-launch form)."""
    if not (q.is_cuda and q.dim() == 3 and v.dim() == 3 and w_out.dim() in (2, 4)) or ATTN_PRECISION != "fp32" or not PROJ_FUSED:
        return False
    if w_out.dim() == 4 and tuple(w_out.shape[2:]) != (1, 1):
        return False
    B, Kc, n = q.shape
    return bool(_lib.load().cabinet_cab_attn_proj_supported(int(B), int(Kc), int(v.shape[1]), int(w_out.shape[0]), int(n)))


# CABINET_ATTN_PROJ_FUSED=0 keeps the round-4 pair of launches (K1, then the projection as a small GEMM): A/B timing
PROJ_FUSED = _os.environ.get("CABINET_ATTN_PROJ_FUSED", "1") != "0"


def cab_attention_proj(q, k, v, w_out, scale):
    """``conv1x1(cab_attention(q, k, v, scale), w_out)`` -> (B, Co, n).  Reference: cab.py:149-155.  ONE launch where
    :func:`cab_attention_proj_supported`, the two operators otherwise."""
    if cab_attention_proj_supported(q, v, w_out) and k.shape == q.shape and v.shape[0] == q.shape[0] and v.shape[2] == q.shape[2] \
            and w_out.shape[1] == v.shape[1]:
        return _CabAttentionProj.apply(q, k, v, w_out, float(scale))
    ctx = cab_attention(q, k, v, scale)
    B, Vc, n = ctx.shape
    return conv1x1(ctx.reshape(B, Vc, n, 1), w_out).reshape(B, -1, n)


# --------------------------------------------------------------------------- FFM


def _ffm_dims(fsp, fcp, w_blk, w1):
    B, Cs, H, W = fsp.shape
    Cc = fcp.shape[1]
    Co = w_blk.shape[0]
    Cm = w1.shape[0]
    return B, Cs, Cc, Co, Cm, H, W


def ffm_fwd_hip(fsp, fcp, w_blk, bn_w, bn_b, run_mean, run_var, w1, w2, training, momentum, eps):
    lib = _lib.load()
    dims = _ffm_dims(fsp, fcp, w_blk, w1)
    B, Cs, Cc, Co, Cm, H, W = dims
    dev = fsp.device
    out = torch.empty((B, Co, H, W), dtype=torch.float32, device=dev)
    z = torch.empty((B, Co, H, W), dtype=torch.float32, device=dev)
    save_mean = torch.empty(Co, dtype=torch.float32, device=dev)
    save_invstd = torch.empty(Co, dtype=torch.float32, device=dev)
    pooled = torch.empty((B, Co), dtype=torch.float32, device=dev)
    gate = torch.empty((B, Co), dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(lib.cabinet_ffm_fwd_workspace_bytes(*dims), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ffm_fwd(_ptr(fsp), _ptr(fcp), _ptr(w_blk), _ptr(bn_w), _ptr(bn_b), _ptr(run_mean),
                                 _ptr(run_var), _ptr(w1), _ptr(w2), *dims, int(training), float(momentum),
                                 float(eps), _ptr(out), _ptr(z), _ptr(save_mean), _ptr(save_invstd),
                                 _ptr(pooled), _ptr(gate), _ptr(ws), nbytes, _stream_handle(dev))
    _lib.check(rc, "cabinet_ffm_fwd")
    return out, z, save_mean, save_invstd, pooled, gate


def ffm_bwd_hip(g, fsp, fcp, w_blk, bn_w, bn_b, w1, w2, z, save_mean, save_invstd, pooled, gate, training):
    lib = _lib.load()
    dims = _ffm_dims(fsp, fcp, w_blk, w1)
    dev = fsp.device
    dfsp, dfcp = torch.empty_like(fsp), torch.empty_like(fcp)
    dw_blk = torch.empty_like(w_blk)
    dbn_w, dbn_b = torch.empty_like(bn_w), torch.empty_like(bn_b)
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    ws, nbytes = _workspace(lib.cabinet_ffm_bwd_workspace_bytes(*dims), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ffm_bwd(_ptr(g), _ptr(fsp), _ptr(fcp), _ptr(w_blk), _ptr(bn_w), _ptr(bn_b), _ptr(w1),
                                 _ptr(w2), _ptr(z), _ptr(save_mean), _ptr(save_invstd), _ptr(pooled),
                                 _ptr(gate), *dims, int(training), _ptr(dfsp), _ptr(dfcp), _ptr(dw_blk),
                                 _ptr(dbn_w), _ptr(dbn_b), _ptr(dw1), _ptr(dw2), _ptr(ws), nbytes,
                                 _stream_handle(dev))
    _lib.check(rc, "cabinet_ffm_bwd")
    return dfsp, dfcp, dw_blk, dbn_w, dbn_b, dw1, dw2


class _FfmFused(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, fsp, fcp, w_blk, bn_w, bn_b, w1, w2, run_mean, run_var, training, momentum, eps):
        fsp, fcp = _f32c(fsp), _f32c(fcp)
        w_blk2 = _f32c(w_blk).view(w_blk.shape[0], -1)
        w1_2 = _f32c(w1).view(w1.shape[0], -1)
        w2_2 = _f32c(w2).view(w2.shape[0], -1)
        bn_w, bn_b = _f32c(bn_w), _f32c(bn_b)
        out, z, mean, invstd, pooled, gate = ffm_fwd_hip(fsp, fcp, w_blk2, bn_w, bn_b, run_mean, run_var,
                                                         w1_2, w2_2, training, momentum, eps)
        fn_ctx.save_for_backward(fsp, fcp, w_blk2, bn_w, bn_b, w1_2, w2_2, z, mean, invstd, pooled, gate)
        fn_ctx.training = training
        fn_ctx.w_shapes = (w_blk.shape, w1.shape, w2.shape)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        fsp, fcp, w_blk, bn_w, bn_b, w1, w2, z, mean, invstd, pooled, gate = fn_ctx.saved_tensors
        dfsp, dfcp, dw_blk, dbn_w, dbn_b, dw1, dw2 = ffm_bwd_hip(
            _f32c(g), fsp, fcp, w_blk, bn_w, bn_b, w1, w2, z, mean, invstd, pooled, gate, fn_ctx.training)
        s_blk, s1, s2 = fn_ctx.w_shapes
        return (dfsp, dfcp, dw_blk.view(s_blk), dbn_w, dbn_b, dw1.view(s1), dw2.view(s2),
                None, None, None, None, None)


def ffm_up_fwd_hip(fsp, low, w_blk, bn_w, bn_b, run_mean, run_var, w1, w2, training, momentum, eps, precision=0):
    lib = _lib.load()
    B, Cs, H, W = fsp.shape
    Cc, Hl, Wl = low.shape[1:]
    Co, Cm = w_blk.shape[0], w1.shape[0]
    dims = (B, Cs, Cc, Co, Cm, H, W, Hl, Wl)
    dev = fsp.device
    out = torch.empty((B, Co, H, W), dtype=torch.float32, device=dev)
    z = torch.empty((B, Co, H, W), dtype=torch.float32, device=dev)
    save_mean = torch.empty(Co, dtype=torch.float32, device=dev)
    save_invstd = torch.empty(Co, dtype=torch.float32, device=dev)
    pooled = torch.empty((B, Co), dtype=torch.float32, device=dev)
    gate = torch.empty((B, Co), dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(lib.cabinet_ffm_up_fwd_workspace_bytes(*dims), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ffm_up_fwd(_ptr(fsp), _ptr(low), _ptr(w_blk), _ptr(bn_w), _ptr(bn_b), _ptr(run_mean),
                                    _ptr(run_var), _ptr(w1), _ptr(w2), *dims, int(training), float(momentum),
                                    float(eps), int(precision), _ptr(out), _ptr(z), _ptr(save_mean), _ptr(save_invstd),
                                    _ptr(pooled), _ptr(gate), _ptr(ws), nbytes, _stream_handle(dev))
    _lib.check(rc, "cabinet_ffm_up_fwd")
    return out, z, save_mean, save_invstd, pooled, gate


def ffm_up_bwd_hip(g, fsp, low, w_blk, bn_w, bn_b, w1, w2, z, save_mean, save_invstd, pooled, gate, training):
    lib = _lib.load()
    B, Cs, H, W = fsp.shape
    Cc, Hl, Wl = low.shape[1:]
    dims = (B, Cs, Cc, w_blk.shape[0], w1.shape[0], H, W, Hl, Wl)
    dev = fsp.device
    dfsp, dlow = torch.empty_like(fsp), torch.empty_like(low)
    dw_blk = torch.empty_like(w_blk)
    dbn_w, dbn_b = torch.empty_like(bn_w), torch.empty_like(bn_b)
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    ws, nbytes = _workspace(lib.cabinet_ffm_up_bwd_workspace_bytes(*dims), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ffm_up_bwd(_ptr(g), _ptr(fsp), _ptr(low), _ptr(w_blk), _ptr(bn_w), _ptr(bn_b), _ptr(w1),
                                    _ptr(w2), _ptr(z), _ptr(save_mean), _ptr(save_invstd), _ptr(pooled),
                                    _ptr(gate), *dims, int(training), _ptr(dfsp), _ptr(dlow), _ptr(dw_blk),
                                    _ptr(dbn_w), _ptr(dbn_b), _ptr(dw1), _ptr(dw2), _ptr(ws), nbytes,
                                    _stream_handle(dev))
    _lib.check(rc, "cabinet_ffm_up_bwd")
    return dfsp, dlow, dw_blk, dbn_w, dbn_b, dw1, dw2


class _FfmUpFused(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, fsp, low, w_blk, bn_w, bn_b, w1, w2, run_mean, run_var, training, momentum, eps):
        fsp, low = _f32c(fsp), _f32c(low)
        w_blk2 = _f32c(w_blk).view(w_blk.shape[0], -1)
        w1_2 = _f32c(w1).view(w1.shape[0], -1)
        w2_2 = _f32c(w2).view(w2.shape[0], -1)
        bn_w, bn_b = _f32c(bn_w), _f32c(bn_b)
        out, z, mean, invstd, pooled, gate = ffm_up_fwd_hip(fsp, low, w_blk2, bn_w, bn_b, run_mean, run_var,
                                                            w1_2, w2_2, training, momentum, eps,
                                                            _ffm_precision())
        fn_ctx.save_for_backward(fsp, low, w_blk2, bn_w, bn_b, w1_2, w2_2, z, mean, invstd, pooled, gate)
        fn_ctx.training = training
        fn_ctx.w_shapes = (w_blk.shape, w1.shape, w2.shape)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        fsp, low, w_blk, bn_w, bn_b, w1, w2, z, mean, invstd, pooled, gate = fn_ctx.saved_tensors
        dfsp, dlow, dw_blk, dbn_w, dbn_b, dw1, dw2 = ffm_up_bwd_hip(
            _f32c(g), fsp, low, w_blk, bn_w, bn_b, w1, w2, z, mean, invstd, pooled, gate, fn_ctx.training)
        s_blk, s1, s2 = fn_ctx.w_shapes
        return (dfsp, dlow, dw_blk.view(s_blk), dbn_w, dbn_b, dw1.view(s1), dw2.view(s2),
                None, None, None, None, None)


_NBT_PENDING = None  # list of num_batches_tracked buffers while batched_bn_counters() is open


class batched_bn_counters:
    """Within this context the ``num_batches_tracked += 1`` of every BatchNorm2d served by the HIP ops is deferred
    and applied as ONE multi-tensor add on exit (the model has 59 BatchNorms: 59 one-element kernels per step
    otherwise).  Values after the context are identical; nesting is a no-op."""

    def __enter__(self):
        global _NBT_PENDING
        self.owner = _NBT_PENDING is None
        if self.owner:
            _NBT_PENDING = []
        return self

    def __exit__(self, *exc):
        global _NBT_PENDING
        if self.owner:
            pending, _NBT_PENDING = _NBT_PENDING, None
            if pending:
                # a module applied twice inside the context appears twice: a multi-tensor add with a repeated tensor is a
                # read-modify-write race, so each distinct counter is added its own count
                counts = {}
                for t in pending:
                    counts.setdefault(id(t), [t, 0])[1] += 1
                by_count = {}
                for t, c in counts.values():
                    by_count.setdefault(c, []).append(t)
                for c, ts in by_count.items():
                    torch._foreach_add_(ts, c)
        return False


def _bn_step(bn):
    if not (bn.affine and bn.track_running_stats):
        raise RuntimeError("ffm_fused: BatchNorm2d must be affine with running statistics")
    if bn.training:
        if _NBT_PENDING is not None and bn.momentum is not None:
            _NBT_PENDING.append(bn.num_batches_tracked)
            return True, bn.momentum
        bn.num_batches_tracked.add_(1)
        return True, (bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked))
    return False, 0.0


def ffm_fused_upsampled(fsp, low, conv_w, bn, w1, w2):
    """FFM(fsp, bilinear_upsample(low -> fsp's H x W)) with the upsample fused into the kernels
    (reference cabinet.py:228-230 + :236).  ``low`` is the attention branch's (B,Cc,H/32,W/32) output."""
    if fsp.dim() != 4 or low.dim() != 4 or fsp.shape[0] != low.shape[0]:
        raise RuntimeError(f"ffm_fused_upsampled: bad shapes fsp{tuple(fsp.shape)} low{tuple(low.shape)}")
    training, momentum = _bn_step(bn)
    return _FfmUpFused.apply(fsp, low, conv_w, bn.weight, bn.bias, w1, w2, bn.running_mean, bn.running_var,
                             training, momentum, bn.eps)


def ffm_fused(fsp, fcp, conv_w, bn, w1, w2):
    """FeatureFusionModule.forward on HIP tensors (reference cabinet.py:142-153).

    ``bn`` is the nn.BatchNorm2d that owns the affine parameters and running buffers;
    its buffers are updated in place in training mode like nn.BatchNorm2d would.
    """
    training, momentum = _bn_step(bn)
    return _FfmFused.apply(fsp, fcp, conv_w, bn.weight, bn.bias, w1, w2, bn.running_mean, bn.running_var,
                           training, momentum, bn.eps)


# --------------------------------------------------------------------------- OHEM-CE fused with the final upsample


def _class_weight(weight, logits, criterion="OhemCELoss"):
    """A criterion's class-weight buffer as the C ABI wants it: dense fp32 (C,) on the logits' device, or None.  The buffer of
    a criterion under ``.half()`` / AMP may be half precision; no such pointer reaches the library.  A buffer that already is
    fp32, contiguous and on the device is passed as it is (its ADDRESS is what a captured graph replays)."""
    if weight is None:
        return None
    if weight.dim() != 1 or weight.shape[0] != logits.shape[1]:
        raise RuntimeError(f"{criterion}: weight of shape {tuple(weight.shape)} for {logits.shape[1]} classes")
    return _f32c(weight.detach().to(logits.device))


def ohem_up_supported(logits_low, size):
    """The fused OHEM head takes these logits: HIP, (B,C,Hl,Wl) with C <= 32, a row of C * Wl floats and the segment buffers
    of the resize ratio inside the kernels' LDS, B and H inside the grid.  The library's own rule (``check_ohem``: the focal
    query with gamma = 0 is exactly that check for one image), asked before anything is launched."""
    if not logits_low.is_cuda or logits_low.dim() != 4 or len(size) != 2:
        return False
    B, C, Hl, Wl = logits_low.shape
    if B > 65535:  # the query is per image; check_ohem also bounds the batch (grid.y)
        return False
    return bool(_lib.load().cabinet_focal_up_supported(C, Hl, Wl, int(size[0]), int(size[1]), 0.0))


def ohem_up_fwd_hip(logits_low, labels, size, thresh, ignore_lb, weight=None):
    """Per-pixel CE of bilinear_upsample(logits_low -> size) vs labels, never materialising the upsample.
    Returns loss_px (B,H,W) and the three reduced statistics as ONE device tensor [n_valid, n_above, sum_above].
    ``weight`` (C,): per-class weights; the statistics are then over w[label] * CE while loss_px stays the unweighted CE (it is
    the buffer the backward rebuilds the log-sum-exp from; hand ohem_up_bwd_hip the same weights)."""
    lib = _lib.load()
    logits_low, labels = _f32c(logits_low), _aligned(labels)
    weight = _class_weight(weight, logits_low)
    B, C, Hl, Wl = logits_low.shape
    H, W = size
    dev = logits_low.device
    nblk = lib.cabinet_ohem_up_blocks(B, H, W)
    loss_px = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    blk_sum = torch.empty(nblk, dtype=torch.float32, device=dev)
    blk_cnt = torch.empty((nblk, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ohem_up_w_fwd(_ptr(logits_low), _ptr(labels), B, C, Hl, Wl, H, W, float(thresh), int(ignore_lb),
                                       _ptr(loss_px), _ptr(blk_sum), _ptr(blk_cnt), _ptr(weight), _stream_handle(dev))
        _lib.check(rc, "cabinet_ohem_up_w_fwd")
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        rc = lib.cabinet_ohem_stats(_ptr(blk_sum), _ptr(blk_cnt), 1, nblk, _ptr(stats), _stream_handle(dev))
    _lib.check(rc, "cabinet_ohem_stats")
    return loss_px, stats


def ohem_up_bwd_hip(logits_low, labels, loss_px, size, thresh, ignore_lb, coef, weight=None):
    lib = _lib.load()
    logits_low, labels, loss_px = _f32c(logits_low), _aligned(labels), _f32c(loss_px)
    weight = _class_weight(weight, logits_low)
    B, C, Hl, Wl = logits_low.shape
    H, W = size
    dev = logits_low.device
    dlow = torch.empty_like(logits_low)
    ws, nbytes = _workspace(lib.cabinet_ohem_up_bwd_workspace_bytes(B, C, Hl, Wl, H, W), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ohem_up_w_bwd(_ptr(logits_low), _ptr(labels), _ptr(loss_px), B, C, Hl, Wl, H, W, float(thresh),
                                       int(ignore_lb), float(coef), _ptr(dlow), _ptr(ws), nbytes, _ptr(weight),
                                       _stream_handle(dev))
    _lib.check(rc, "cabinet_ohem_up_w_bwd")
    return dlow


class _OhemUpSelected(torch.autograd.Function):
    """loss = sum_above / n_above for the 'at least n_min pixels above thresh' branch (reference loss.py:74-75);
    forward statistics were produced by ohem_up_fwd_hip, backward runs the two adjoint kernels.  ``n_above`` is a DEVICE
    scalar: nothing of the step's data-dependent state is baked into a kernel argument, so the op can be replayed from a
    captured hipGraph (cabinet_amd.train.GraphedTrainStep); the host only reads it to pick the branch.
    ``weight``: the class weights the forward statistics were formed with (a buffer: no gradient), or None."""

    @staticmethod
    def forward(fn_ctx, logits_low, labels, loss_px, sum_above, n_above, size, thresh, ignore_lb, weight=None):
        fn_ctx.save_for_backward(logits_low, labels, loss_px, n_above)
        fn_ctx.meta = (size, thresh, ignore_lb)
        fn_ctx.weight = weight  # not through save_for_backward: an in-place update of the buffer is no autograd error
        return (sum_above / n_above).to(torch.float32)

    @staticmethod
    def backward(fn_ctx, g):
        logits_low, labels, loss_px, n_above = fn_ctx.saved_tensors
        size, thresh, ignore_lb = fn_ctx.meta
        # the kernels produce U^T[sel * w * (softmax - onehot)]; upstream gradient and 1/n_above are device scalars folded in after
        dlow = ohem_up_bwd_hip(logits_low, labels, loss_px, size, thresh, ignore_lb, 1.0, fn_ctx.weight)
        return dlow * (g / n_above).to(torch.float32), None, None, None, None, None, None, None, None


def ohem_up_pair_fwd_hip(low_a, low_b, labels, size, thresh, ignore_lb, weight_a=None, weight_b=None):
    """Both loss heads over the same labels in ONE launch (reference train.py:435 on the outputs of cabinet.py:240-245).
    Returns loss_px (2,B,H,W) and stats (2,3) = per head [n_valid, n_above, sum_above] as one device tensor.
    ``weight_a`` / ``weight_b``: each head's own class weights or None (see ohem_up_fwd_hip)."""
    lib = _lib.load()
    low_a, low_b, labels = _f32c(low_a), _f32c(low_b), _aligned(labels)
    weight_a, weight_b = _class_weight(weight_a, low_a), _class_weight(weight_b, low_b)
    B, C, Hl, Wl = low_a.shape
    H, W = size
    dev = low_a.device
    nblk = lib.cabinet_ohem_up_blocks(B, H, W)
    loss_px = torch.empty((2, B, H, W), dtype=torch.float32, device=dev)
    blk_sum = torch.empty((2, nblk), dtype=torch.float32, device=dev)
    blk_cnt = torch.empty((2, nblk, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ohem_up_pair_w_fwd(_ptr(low_a), _ptr(low_b), _ptr(labels), B, C, Hl, Wl, H, W, float(thresh),
                                            int(ignore_lb), _ptr(loss_px), _ptr(blk_sum), _ptr(blk_cnt), _ptr(weight_a),
                                            _ptr(weight_b), _stream_handle(dev))
        _lib.check(rc, "cabinet_ohem_up_pair_w_fwd")
        stats = torch.empty((2, 3), dtype=torch.float64, device=dev)
        rc = lib.cabinet_ohem_stats(_ptr(blk_sum), _ptr(blk_cnt), 2, nblk, _ptr(stats), _stream_handle(dev))
    _lib.check(rc, "cabinet_ohem_stats")
    return loss_px, stats


def ohem_up_pair_bwd_hip(low_a, low_b, labels, loss_px, size, thresh, ignore_lb, coef, weight_a=None, weight_b=None):
    lib = _lib.load()
    low_a, low_b, labels, loss_px = _f32c(low_a), _f32c(low_b), _aligned(labels), _f32c(loss_px)
    weight_a, weight_b = _class_weight(weight_a, low_a), _class_weight(weight_b, low_b)
    B, C, Hl, Wl = low_a.shape
    H, W = size
    dev = low_a.device
    dlow = torch.empty((2, B, C, Hl, Wl), dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(lib.cabinet_ohem_up_pair_bwd_workspace_bytes(B, C, Hl, Wl, H, W), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ohem_up_pair_w_bwd(_ptr(low_a), _ptr(low_b), _ptr(labels), _ptr(loss_px), B, C, Hl, Wl, H, W,
                                            float(thresh), int(ignore_lb), float(coef), _ptr(dlow), _ptr(ws), nbytes,
                                            _ptr(weight_a), _ptr(weight_b), _stream_handle(dev))
    _lib.check(rc, "cabinet_ohem_up_pair_w_bwd")
    return dlow


class _OhemUpSelectedPair(torch.autograd.Function):
    """loss = sum_above_a / n_above_a + sum_above_b / n_above_b: the two heads' 'at least n_min pixels above thresh' branches
    (reference loss.py:74-75) with ONE backward launch pair for both (see _OhemUpSelected for the single head)."""

    @staticmethod
    def forward(fn_ctx, low_a, low_b, labels, loss_px, stats, size, thresh, ignore_lb, weight_a=None, weight_b=None):
        fn_ctx.save_for_backward(low_a, low_b, labels, loss_px, stats)
        fn_ctx.meta = (size, thresh, ignore_lb)
        fn_ctx.weights = (weight_a, weight_b)
        return (stats[0, 2] / stats[0, 1] + stats[1, 2] / stats[1, 1]).to(torch.float32)

    @staticmethod
    def backward(fn_ctx, g):
        low_a, low_b, labels, loss_px, stats = fn_ctx.saved_tensors
        size, thresh, ignore_lb = fn_ctx.meta
        dlow = ohem_up_pair_bwd_hip(low_a, low_b, labels, loss_px, size, thresh, ignore_lb, 1.0, *fn_ctx.weights)
        scale = (g / stats[:, 1]).to(torch.float32)  # upstream gradient and 1 / n_above per head: device scalars
        dlow = dlow * scale.view(2, 1, 1, 1, 1)
        return dlow[0], dlow[1], None, None, None, None, None, None, None, None


# ---- the top-n_min branch with the selection on the device (reference loss.py:67-80, both branches)


def ohem_select_hip(loss_px, labels, stats, thresh, n_min, ignore_lb, n_classes, weights=None):
    """Per head ``[t, tie, denom, value]`` (a (nheads,4) float64 device tensor) from the forward's ``loss_px`` (nheads,B,H,W)
    and ``stats`` (nheads,3): the threshold the backward selects with, the factor of pixels exactly at it, the divisor of the
    mean, and the mean itself -- ``thresh, 0, n_above, sum_above / n_above`` for a head with at least
    ``min(n_min, n_valid)`` pixels above ``thresh``, else the order statistic of the ``n_min`` hardest pixels.
    ``n_min``: one integer per head; ``weights``: per head the class weights the forward used, or None.  No host read."""
    lib = _lib.load()
    loss_px, labels, stats = _f32c(loss_px), _aligned(labels), stats.contiguous()
    nheads = loss_px.shape[0]
    if loss_px.dim() != 4 or nheads not in (1, 2) or tuple(stats.shape) != (nheads, 3) or stats.dtype != torch.float64:
        raise RuntimeError(f"ohem_select_hip: loss_px {tuple(loss_px.shape)} / stats {tuple(stats.shape)} {stats.dtype}")
    _, B, H, W = loss_px.shape
    dev = loss_px.device
    n_min = [int(n) for n in n_min]
    weights = list(weights) if weights is not None else [None] * nheads
    wts = [None if w is None else _f32c(w.detach().to(dev)) for w in weights] + [None]
    for w in wts:
        if w is not None and (w.dim() != 1 or w.shape[0] != n_classes):
            raise RuntimeError(f"OhemCELoss: weight of shape {tuple(w.shape)} for {n_classes} classes")
    sel = torch.empty((nheads, 4), dtype=torch.float64, device=dev)
    ws, nbytes = _workspace(lib.cabinet_ohem_select_workspace_bytes(nheads, B, H, W), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ohem_select(_ptr(loss_px), _ptr(labels), _ptr(stats), nheads, B, int(n_classes), H, W, float(thresh),
                                     n_min[0], n_min[-1], int(ignore_lb), _ptr(wts[0]), _ptr(wts[1]), _ptr(sel), _ptr(ws),
                                     nbytes, _stream_handle(dev))
    _lib.check(rc, "cabinet_ohem_select")
    return sel


def ohem_up_bwd_sel_hip(logits_low, labels, loss_px, size, sel, ignore_lb, coef, weight=None):
    """ohem_up_bwd_hip with the threshold and the tie factor read on the device from ``sel`` (4,) (see ohem_select_hip)."""
    lib = _lib.load()
    logits_low, labels, loss_px = _f32c(logits_low), _aligned(labels), _f32c(loss_px)
    weight = _class_weight(weight, logits_low)
    B, C, Hl, Wl = logits_low.shape
    H, W = size
    dev = logits_low.device
    dlow = torch.empty_like(logits_low)
    ws, nbytes = _workspace(lib.cabinet_ohem_up_bwd_workspace_bytes(B, C, Hl, Wl, H, W), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ohem_up_w_bwd_sel(_ptr(logits_low), _ptr(labels), _ptr(loss_px), B, C, Hl, Wl, H, W, _ptr(sel),
                                           int(ignore_lb), float(coef), _ptr(dlow), _ptr(ws), nbytes, _ptr(weight),
                                           _stream_handle(dev))
    _lib.check(rc, "cabinet_ohem_up_w_bwd_sel")
    return dlow


def ohem_up_pair_bwd_sel_hip(low_a, low_b, labels, loss_px, size, sel, ignore_lb, coef, weight_a=None, weight_b=None):
    lib = _lib.load()
    low_a, low_b, labels, loss_px = _f32c(low_a), _f32c(low_b), _aligned(labels), _f32c(loss_px)
    weight_a, weight_b = _class_weight(weight_a, low_a), _class_weight(weight_b, low_b)
    B, C, Hl, Wl = low_a.shape
    H, W = size
    dev = low_a.device
    dlow = torch.empty((2, B, C, Hl, Wl), dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(lib.cabinet_ohem_up_pair_bwd_workspace_bytes(B, C, Hl, Wl, H, W), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_ohem_up_pair_w_bwd_sel(_ptr(low_a), _ptr(low_b), _ptr(labels), _ptr(loss_px), B, C, Hl, Wl, H, W,
                                                _ptr(sel), int(ignore_lb), float(coef), _ptr(dlow), _ptr(ws), nbytes,
                                                _ptr(weight_a), _ptr(weight_b), _stream_handle(dev))
    _lib.check(rc, "cabinet_ohem_up_pair_w_bwd_sel")
    return dlow


class _OhemUpDeviceSelected(torch.autograd.Function):
    """Either branch of reference loss.py:67-80 for one head, decided on the device: ``sel`` (4,) = [t, tie, denom, value]
    from ohem_select_hip.  loss = value; backward runs the adjoint kernels with the device threshold and scales by
    g / denom, a device scalar.  Nothing data-dependent is a kernel argument: replayable from a captured hipGraph whatever
    branch the replayed batch is on."""

    @staticmethod
    def forward(fn_ctx, logits_low, labels, loss_px, sel, size, ignore_lb, weight=None):
        fn_ctx.save_for_backward(logits_low, labels, loss_px, sel)
        fn_ctx.meta = (size, ignore_lb)
        fn_ctx.weight = weight
        return sel[3].to(torch.float32)

    @staticmethod
    def backward(fn_ctx, g):
        logits_low, labels, loss_px, sel = fn_ctx.saved_tensors
        size, ignore_lb = fn_ctx.meta
        dlow = ohem_up_bwd_sel_hip(logits_low, labels, loss_px, size, sel, ignore_lb, 1.0, fn_ctx.weight)
        return dlow * (g / sel[2]).to(torch.float32), None, None, None, None, None, None


class _OhemUpDeviceSelectedPair(torch.autograd.Function):
    """Both heads, any mix of branches: ``sel`` (2,4) from ONE selection sequence, ONE backward launch pair."""

    @staticmethod
    def forward(fn_ctx, low_a, low_b, labels, loss_px, sel, size, ignore_lb, weight_a=None, weight_b=None):
        fn_ctx.save_for_backward(low_a, low_b, labels, loss_px, sel)
        fn_ctx.meta = (size, ignore_lb)
        fn_ctx.weights = (weight_a, weight_b)
        return (sel[0, 3] + sel[1, 3]).to(torch.float32)

    @staticmethod
    def backward(fn_ctx, g):
        low_a, low_b, labels, loss_px, sel = fn_ctx.saved_tensors
        size, ignore_lb = fn_ctx.meta
        dlow = ohem_up_pair_bwd_sel_hip(low_a, low_b, labels, loss_px, size, sel, ignore_lb, 1.0, *fn_ctx.weights)
        scale = (g / sel[:, 2]).to(torch.float32)
        dlow = dlow * scale.view(2, 1, 1, 1, 1)
        return dlow[0], dlow[1], None, None, None, None, None, None, None


# ---- softmax focal loss on the same fused operator (reference loss.py:86-127; K19)


def focal_up_supported(logits_low, size, gamma):
    """The fused focal head takes these logits (C <= 32, the LDS row buffers) and this exponent (finite, >= 0)."""
    import math

    gamma = float(gamma)
    if not logits_low.is_cuda or logits_low.dim() != 4 or not math.isfinite(gamma) or gamma < 0.0:
        return False
    _, C, Hl, Wl = logits_low.shape
    return bool(_lib.load().cabinet_focal_up_supported(C, Hl, Wl, int(size[0]), int(size[1]), gamma))


def focal_up_fwd_hip(lows, labels, size, gammas, ignore_lb, weights=None, out=None):
    """Focal loss of bilinear_upsample(low -> size) vs labels for one or two heads (``lows``: a list of (B,C,Hl,Wl) tensors of
    one shape), never materialising the upsample.  Returns loss_px (nh,B,H,W), the UNWEIGHTED per-pixel l = lse - x_label
    (0 where ignored), and stats (nh,3) float64 = per head [n_valid, D, S] with D = sum w_t, S = sum w_t q^gamma l; n_valid < 0
    flags a label outside [0, C).  ``out``: an (nh,3) float64 device tensor to write the statistics into.  No host read."""
    lib = _lib.load()
    lows, labels = [_f32c(t) for t in lows], _aligned(labels)
    nh = len(lows)
    weights = list(weights) if weights is not None else [None] * nh
    wts = [_class_weight(w, lows[0], "SoftmaxFocalLoss") for w in weights] + [None]
    gam = [float(g) for g in gammas] + [0.0]
    B, C, Hl, Wl = lows[0].shape
    H, W = size
    dev = lows[0].device
    nblk = lib.cabinet_ohem_up_blocks(B, H, W)
    loss_px = torch.empty((nh, B, H, W), dtype=torch.float32, device=dev)
    blk_sum = torch.empty((nh, nblk, 2), dtype=torch.float32, device=dev)
    blk_cnt = torch.empty((nh, nblk), dtype=torch.int32, device=dev)
    stats = out if out is not None else torch.empty((nh, 3), dtype=torch.float64, device=dev)
    if tuple(stats.shape) != (nh, 3) or stats.dtype != torch.float64 or stats.device != dev or not stats.is_contiguous():
        raise RuntimeError(f"focal_up_fwd_hip: out must be a contiguous ({nh},3) float64 tensor on {dev}")
    with torch.cuda.device(dev):
        rc = lib.cabinet_focal_up_fwd(_ptr(lows[0]), _ptr(lows[1]) if nh == 2 else None, _ptr(labels), B, C, Hl, Wl, H, W,
                                      gam[0], gam[1], int(ignore_lb), _ptr(loss_px), _ptr(blk_sum), _ptr(blk_cnt),
                                      _ptr(wts[0]), _ptr(wts[1]), _stream_handle(dev))
        _lib.check(rc, "cabinet_focal_up_fwd")
        rc = lib.cabinet_focal_stats(_ptr(blk_sum), _ptr(blk_cnt), nh, nblk, _ptr(stats), _stream_handle(dev))
    _lib.check(rc, "cabinet_focal_stats")
    return loss_px, stats


def focal_up_bwd_hip(lows, labels, loss_px, size, gammas, ignore_lb, coef, weights=None, out=None):
    """(nh,B,C,Hl,Wl) = coef * U^T[w_t a(l) (softmax - onehot)] from the forward's ``loss_px`` (see focal_up_fwd_hip: the same
    gammas and weights).  ``out``: a buffer of that shape; every element is written."""
    lib = _lib.load()
    lows, labels, loss_px = [_f32c(t) for t in lows], _aligned(labels), _f32c(loss_px)
    nh = len(lows)
    weights = list(weights) if weights is not None else [None] * nh
    wts = [_class_weight(w, lows[0], "SoftmaxFocalLoss") for w in weights] + [None]
    gam = [float(g) for g in gammas] + [0.0]
    B, C, Hl, Wl = lows[0].shape
    H, W = size
    dev = lows[0].device
    dlow = out if out is not None else torch.empty((nh, B, C, Hl, Wl), dtype=torch.float32, device=dev)
    if tuple(dlow.shape) != (nh, B, C, Hl, Wl) or dlow.dtype != torch.float32 or dlow.device != dev \
            or not dlow.is_contiguous() or dlow.data_ptr() & 15:
        raise RuntimeError(f"focal_up_bwd_hip: out must be a contiguous, 16-byte aligned ({nh},{B},{C},{Hl},{Wl}) float32 "
                           f"tensor on {dev}")
    ws, nbytes = _workspace(lib.cabinet_focal_up_bwd_workspace_bytes(nh, B, C, Hl, Wl, H, W), dev)
    with torch.cuda.device(dev):
        rc = lib.cabinet_focal_up_bwd(_ptr(lows[0]), _ptr(lows[1]) if nh == 2 else None, _ptr(labels), _ptr(loss_px), B, C, Hl,
                                      Wl, H, W, gam[0], gam[1], int(ignore_lb), float(coef), _ptr(dlow), _ptr(ws), nbytes,
                                      _ptr(wts[0]), _ptr(wts[1]), _stream_handle(dev))
    _lib.check(rc, "cabinet_focal_up_bwd")
    return dlow


class _FocalUp(torch.autograd.Function):
    """Sum over one or two heads of SoftmaxFocalLoss behind the upsample: loss = sum_heads S / D.  The reference's semantics,
    all on the device: no valid pixel (or only classes of weight 0) -> NaN (0 / 0) and a gradient of exactly 0; a label out of
    range -> NaN (``stats[:, 0] < 0`` says why).  Nothing is read on the host and nothing data-dependent is a kernel argument:
    replayable from a captured hipGraph whatever the batch.  ``stats_out``: where the (nh,3) statistics go (a static tensor of
    a graphed step)."""

    @staticmethod
    def forward(fn_ctx, labels, size, ignore_lb, gammas, weights, stats_out, *lows):
        loss_px, stats = focal_up_fwd_hip([t.detach() for t in lows], labels, size, gammas, ignore_lb, weights, out=stats_out)
        fn_ctx.save_for_backward(labels, loss_px, stats, *lows)
        fn_ctx.meta = (size, ignore_lb, tuple(gammas))
        fn_ctx.weights = tuple(weights)  # not through save_for_backward: an in-place update of the buffer is no autograd error
        per_head = torch.where(stats[:, 0] < 0, torch.full_like(stats[:, 2], float("nan")), stats[:, 2] / stats[:, 1])
        return per_head.sum().to(torch.float32)

    @staticmethod
    def backward(fn_ctx, g):
        labels, loss_px, stats, *lows = fn_ctx.saved_tensors
        size, ignore_lb, gammas = fn_ctx.meta
        dlow = focal_up_bwd_hip(lows, labels, loss_px, size, gammas, ignore_lb, 1.0, fn_ctx.weights)
        D = stats[:, 1]
        scale = torch.where(D > 0, g / D, torch.zeros_like(D)).to(torch.float32)  # upstream gradient and 1 / D: device scalars
        dlow = dlow * scale.view(-1, 1, 1, 1, 1)
        return (None,) * 6 + tuple(dlow[i] for i in range(len(lows)))


def focal_up_loss(lows, labels, size, gammas, ignore_lb, weights=None, stats_out=None):
    """``sum_i SoftmaxFocalLoss(gammas[i], weights[i], ignore_lb)(interpolate(lows[i], size), labels)`` on the fused kernels; one
    or two heads of one shape, ONE forward launch and ONE backward launch pair."""
    lows = [_f32c(t) for t in lows]
    weights = list(weights) if weights is not None else [None] * len(lows)
    return _FocalUp.apply(_aligned(labels), tuple(int(s) for s in size), int(ignore_lb), tuple(float(g) for g in gammas),
                          tuple(weights), stats_out, *lows)


# --------------------------------------------------------------------------- CAB local branch + block output (K5)


def _ptr3(ts):
    return (_ct.c_void_p * 3)(*[t.data_ptr() for t in ts])


def cab_local_supported(x):
    return x.dim() == 4 and bool(_lib.load().cabinet_cab_local_supported(*x.shape))


def cab_local_fwd_hip(x, glob, gamma, dw_w, bn_w, bn_b, run_mean, run_var, training, momentum, eps):
    """out = [gamma*glob +] x*(1 + sigmoid(refine(x))); returns out and the (3,C) saved mean / invstd."""
    lib = _lib.load()
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    mean = torch.empty((3, C), dtype=torch.float32, device=x.device)
    invstd = torch.empty((3, C), dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(lib.cabinet_cab_local_fwd_workspace_bytes(B, C, H, W), x.device)  # 0 for the resident form
    with torch.cuda.device(x.device):
        rc = lib.cabinet_cab_local_fwd(_ptr(x), _ptr(glob), _ptr(gamma), _ptr3(dw_w), _ptr3(bn_w), _ptr3(bn_b),
                                       _ptr3(run_mean), _ptr3(run_var), B, C, H, W, int(training), float(momentum),
                                       float(eps), _ptr(out), _ptr(mean), _ptr(invstd), _ptr(ws), nbytes,
                                       _stream_handle(x.device))
    _lib.check(rc, "cabinet_cab_local_fwd")
    return out, mean, invstd


def cab_local_bwd_hip(g, x, glob, gamma, dw_w, bn_w, bn_b, mean, invstd, training):
    lib = _lib.load()
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    dglob = torch.empty_like(x) if glob is not None else None
    dgamma_part = torch.empty(C, dtype=torch.float32, device=x.device) if glob is not None else None
    ddw = [torch.empty_like(w) for w in dw_w]
    dbw = [torch.empty_like(w) for w in bn_w]
    dbb = [torch.empty_like(w) for w in bn_b]
    ws, nbytes = _workspace(lib.cabinet_cab_local_bwd_workspace_bytes(B, C, H, W), x.device)
    with torch.cuda.device(x.device):
        rc = lib.cabinet_cab_local_bwd(_ptr(g), _ptr(x), _ptr(glob), _ptr(gamma), _ptr3(dw_w), _ptr3(bn_w),
                                       _ptr3(bn_b), _ptr(mean), _ptr(invstd), B, C, H, W, int(training), _ptr(dx),
                                       _ptr(dglob), _ptr(dgamma_part), _ptr3(ddw), _ptr3(dbw), _ptr3(dbb),
                                       _ptr(ws), nbytes, _stream_handle(x.device))
    _lib.check(rc, "cabinet_cab_local_bwd")
    return dx, dglob, dgamma_part, ddw, dbw, dbb


class _CabLocal(torch.autograd.Function):
    """args: x, glob|None, gamma|None, 3 dw weights, 3 bn weights, 3 bn biases, 3 running means, 3 running vars,
    training, momentum, eps."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, glob, gamma, *rest):
        dw_w, bn_w, bn_b = [_f32c(t) for t in rest[0:3]], [_f32c(t) for t in rest[3:6]], [_f32c(t) for t in rest[6:9]]
        run_mean, run_var = list(rest[9:12]), list(rest[12:15])
        training, momentum, eps = rest[15:18]
        x = _f32c(x)
        glob = _f32c(glob) if glob is not None else None
        gamma = _f32c(gamma) if glob is not None else None
        out, mean, invstd = cab_local_fwd_hip(x, glob, gamma, dw_w, bn_w, bn_b, run_mean, run_var, training,
                                              momentum, eps)
        fn_ctx.save_for_backward(x, glob, gamma, mean, invstd, *dw_w, *bn_w, *bn_b)
        fn_ctx.training = bool(training)
        fn_ctx.w_shapes = [t.shape for t in rest[0:3]]
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        x, glob, gamma, mean, invstd, *params = fn_ctx.saved_tensors
        dw_w, bn_w, bn_b = params[0:3], params[3:6], params[6:9]
        dx, dglob, dgamma_part, ddw, dbw, dbb = cab_local_bwd_hip(_f32c(g), x, glob, gamma, dw_w, bn_w, bn_b, mean,
                                                                  invstd, fn_ctx.training)
        dgamma = dgamma_part.sum().reshape(gamma.shape) if glob is not None else None
        ddw = [d.view(s) for d, s in zip(ddw, fn_ctx.w_shapes)]
        return (dx, dglob, dgamma, *ddw, *dbw, *dbb) + (None,) * 9


def cab_local(x, refine, glob=None, gamma=None):
    """LocalAttention.forward (reference cab.py:182-184), plus ``gamma * glob +`` (cab.py:213-216) when given.

    ``refine`` is the nn.Sequential of three DWConv blocks (conv, BatchNorm2d, ReLU) that owns the parameters
    and running buffers; the buffers are updated in place in training mode like nn.BatchNorm2d would.
    """
    if not x.is_cuda:
        raise RuntimeError("cab_local: device tensors only (host tensors take the composite ATen path)")
    convs = [blk.block[0] for blk in refine]
    bns = [blk.block[1] for blk in refine]
    if len(convs) != 3 or any(c.kernel_size != (3, 3) or c.stride != (1, 1) or c.padding != (1, 1)
                              or c.groups != x.shape[1] or c.bias is not None for c in convs):
        raise RuntimeError("cab_local: expects three depthwise 3x3, stride 1, pad 1, bias-free convolutions")
    if len({(bn.eps, bn.momentum) for bn in bns}) != 1:
        raise RuntimeError("cab_local: the three BatchNorm2d must share eps and momentum")
    steps = [_bn_step(bn) for bn in bns]
    training, momentum = steps[0]
    if any(s[0] != training for s in steps):
        raise RuntimeError("cab_local: BatchNorm2d layers disagree on training mode")
    return _CabLocal.apply(x, glob, gamma, *[c.weight for c in convs], *[bn.weight for bn in bns],
                           *[bn.bias for bn in bns], *[bn.running_mean for bn in bns],
                           *[bn.running_var for bn in bns], training, momentum, bns[0].eps)


# --------------------------------------------------------------------------- q/k/v producers (K6) and 1x1 convolution


def _sizes_arg(sizes):
    return (_ct.c_int * len(sizes))(*[int(s) for s in sizes])


def cab_qkv_supported(x, Kc, Vc, sizes):
    if x.dim() != 4 or not 1 <= len(sizes) <= 4:
        return False
    B, C, H, W = x.shape
    return bool(_lib.load().cabinet_cab_qkv_supported(B, C, Kc, Vc, H, W, len(sizes), _sizes_arg(sizes)))


class _CabQkv(torch.autograd.Function):
    """args: x, wq, wk, wv, bnq_w, bnq_b, bnk_w, bnk_b, wpk, wpv, bnq_rm, bnq_rv, bnk_rm, bnk_rv, sizes, training,
    momentum, eps  ->  q (B,Kc,n), k (B,Kc,n), v (B,Vc,n)"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, wq, wk, wv, bnq_w, bnq_b, bnk_w, bnk_b, wpk, wpv, bnq_rm, bnq_rv, bnk_rm, bnk_rv, sizes,
                training, momentum, eps):
        lib = _lib.load()
        x = _f32c(x)
        B, C, H, W = x.shape
        Kc, Vc, n, ns = wq.shape[0], wv.shape[0], H * W, len(sizes)
        shapes = (wq.shape, wk.shape, wv.shape, wpk.shape, wpv.shape)
        wq2, wk2, wv2 = (_f32c(t).view(t.shape[0], C) for t in (wq, wk, wv))
        wpk2, wpv2 = _f32c(wpk).view(Kc, (ns + 1) * Kc), _f32c(wpv).view(Vc, (ns + 1) * Vc)
        bnq_w, bnq_b, bnk_w, bnk_b = _f32c(bnq_w), _f32c(bnq_b), _f32c(bnk_w), _f32c(bnk_b)
        sz = _sizes_arg(sizes)
        dims = (B, C, Kc, Vc, H, W, ns, sz)
        nbp = lib.cabinet_cab_qkv_padded_bins(ns, sz)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)  # noqa: E731
        q, k, v = new(B, Kc, n), new(B, Kc, n), new(B, Vc, n)
        zqk, vv, kk = new(B, 2 * Kc, n), new(B, Vc, n), new(B, Kc, n)
        pooled_k, pooled_v = new(B, ns * Kc, nbp), new(B, ns * Vc, nbp)
        mean, invstd = new(2 * Kc), new(2 * Kc)
        ws, nbytes = _workspace(lib.cabinet_cab_qkv_fwd_workspace_bytes(*dims), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_cab_qkv_fwd(_ptr(x), _ptr(wq2), _ptr(wk2), _ptr(wv2), _ptr(bnq_w), _ptr(bnq_b), _ptr(bnq_rm),
                                         _ptr(bnq_rv), _ptr(bnk_w), _ptr(bnk_b), _ptr(bnk_rm), _ptr(bnk_rv), _ptr(wpk2),
                                         _ptr(wpv2), *dims, int(training), float(momentum), float(eps), _ptr(q),
                                         _ptr(k), _ptr(v), _ptr(zqk), _ptr(vv), _ptr(kk), _ptr(pooled_k),
                                         _ptr(pooled_v), _ptr(mean), _ptr(invstd), _ptr(ws), nbytes,
                                         _stream_handle(x.device))
        _lib.check(rc, "cabinet_cab_qkv_fwd")
        fn_ctx.save_for_backward(x, wq2, wk2, wv2, bnq_w, bnq_b, bnk_w, bnk_b, wpk2, wpv2, zqk, vv, kk, pooled_k,
                                 pooled_v, mean, invstd)
        fn_ctx.sizes, fn_ctx.training, fn_ctx.shapes = tuple(sizes), bool(training), shapes
        return q, k, v

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, dq, dk, dv):
        lib = _lib.load()
        (x, wq, wk, wv, bnq_w, bnq_b, bnk_w, bnk_b, wpk, wpv, zqk, vv, kk, pooled_k, pooled_v, mean,
         invstd) = fn_ctx.saved_tensors
        B, C, H, W = x.shape
        Kc, Vc, ns = wq.shape[0], wv.shape[0], len(fn_ctx.sizes)
        sz = _sizes_arg(fn_ctx.sizes)
        dims = (B, C, Kc, Vc, H, W, ns, sz)
        dq = _f32c(dq) if dq is not None else torch.zeros(B, Kc, H * W, device=x.device)
        dk = _f32c(dk) if dk is not None else torch.zeros(B, Kc, H * W, device=x.device)
        dv = _f32c(dv) if dv is not None else torch.zeros(B, Vc, H * W, device=x.device)
        dx = torch.empty_like(x)
        dwqk, dwv = torch.empty(2 * Kc, C, device=x.device), torch.empty(Vc, C, device=x.device)
        dbn = [torch.empty(Kc, device=x.device) for _ in range(4)]
        dwpk, dwpv = torch.empty_like(wpk), torch.empty_like(wpv)
        ws, nbytes = _workspace(lib.cabinet_cab_qkv_bwd_workspace_bytes(*dims), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_cab_qkv_bwd(_ptr(dq), _ptr(dk), _ptr(dv), _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv),
                                         _ptr(bnq_w), _ptr(bnq_b), _ptr(bnk_w), _ptr(bnk_b), _ptr(wpk), _ptr(wpv),
                                         _ptr(zqk), _ptr(vv), _ptr(kk), _ptr(pooled_k), _ptr(pooled_v), _ptr(mean),
                                         _ptr(invstd), *dims, int(fn_ctx.training), _ptr(dx), _ptr(dwqk), _ptr(dwv),
                                         _ptr(dbn[0]), _ptr(dbn[1]), _ptr(dbn[2]), _ptr(dbn[3]), _ptr(dwpk),
                                         _ptr(dwpv), _ptr(ws), nbytes, _stream_handle(x.device))
        _lib.check(rc, "cabinet_cab_qkv_bwd")
        s_q, s_k, s_v, s_pk, s_pv = fn_ctx.shapes
        return (dx, dwqk[:Kc].view(s_q), dwqk[Kc:].view(s_k), dwv.view(s_v), dbn[0], dbn[1], dbn[2], dbn[3],
                dwpk.view(s_pk), dwpv.view(s_pv)) + (None,) * 8


def cab_qkv(x, gca):
    """q, k, v of GlobalContextAttention (reference cab.py:137-146) from its sub-modules, on device tensors.

    ``gca`` owns to_query / to_key (Conv2d 1x1, BatchNorm2d, ReLU), to_value (Conv2d 1x1), psp_key / psp_value
    (PSPModule); BatchNorm running buffers are updated in place in training mode."""
    bn_q, bn_k = gca.to_query[1], gca.to_key[1]
    sizes = [int(st.output_size[0]) for st in gca.psp_key.stages]
    if sizes != [int(st.output_size[0]) for st in gca.psp_value.stages]:
        raise RuntimeError("cab_qkv: psp_key and psp_value must use the same pyramid sizes")
    if (bn_q.eps, bn_q.momentum, bn_q.training) != (bn_k.eps, bn_k.momentum, bn_k.training):
        raise RuntimeError("cab_qkv: the two BatchNorm2d must share eps, momentum and training mode")
    training, momentum = _bn_step(bn_q)
    _bn_step(bn_k)
    return _CabQkv.apply(x, gca.to_query[0].weight, gca.to_key[0].weight, gca.to_value.weight, bn_q.weight, bn_q.bias,
                         bn_k.weight, bn_k.bias, gca.psp_key.project.weight, gca.psp_value.project.weight,
                         bn_q.running_mean, bn_q.running_var, bn_k.running_mean, bn_k.running_var, sizes, training,
                         momentum, bn_q.eps)


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, weight):
        lib = _lib.load()
        x = _f32c(x)
        Co, Ci = weight.shape[0], weight.shape[1]
        w2 = _f32c(weight).view(Co, Ci)
        B, P = x.shape[0], x[0, 0].numel()
        y = torch.empty((B, Co) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        ws, nbytes = _workspace(lib.cabinet_conv1x1_fwd_workspace_bytes(Ci, Co), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_conv1x1_fwd(_ptr(x), _ptr(w2), B, Ci, Co, P, _ptr(y), _ptr(ws), nbytes,
                                         _stream_handle(x.device))
        _lib.check(rc, "cabinet_conv1x1_fwd")
        fn_ctx.save_for_backward(x, w2)
        fn_ctx.w_shape = weight.shape
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, w2 = fn_ctx.saved_tensors
        g = _f32c(g)
        Co, Ci = w2.shape
        B, P = x.shape[0], x[0, 0].numel()
        dx = torch.empty_like(x) if fn_ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w2) if fn_ctx.needs_input_grad[1] else None
        ws, nbytes = _workspace(lib.cabinet_conv1x1_bwd_workspace_bytes(B, Ci, Co, P), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_conv1x1_bwd(_ptr(g), _ptr(x), _ptr(w2), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes,
                                         _stream_handle(x.device))
        _lib.check(rc, "cabinet_conv1x1_bwd")
        return dx, (dw.view(fn_ctx.w_shape) if dw is not None else None)


class _Conv1x1Bias(torch.autograd.Function):
    """1x1 convolution WITH bias on the small-grid path (``AttentionBranch.convb``, reference cabinet.py:65-66, :86)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, weight, bias):
        lib = _lib.load()
        x = _f32c(x)
        Co, Ci = weight.shape[0], weight.shape[1]
        w2 = _f32c(weight).view(Co, Ci)
        B, P = x.shape[0], x[0, 0].numel()
        y = torch.empty((B, Co) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        ws, nbytes = _workspace(lib.cabinet_conv1x1_fwd_workspace_bytes(Ci, Co), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_conv1x1_bias_fwd(_ptr(x), _ptr(w2), _ptr(_f32c(bias)), B, Ci, Co, P, _ptr(y), _ptr(ws), nbytes,
                                              _stream_handle(x.device))
        _lib.check(rc, "cabinet_conv1x1_bias_fwd")
        fn_ctx.save_for_backward(x, w2)
        fn_ctx.w_shape = weight.shape
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, w2 = fn_ctx.saved_tensors
        g = _f32c(g)
        Co, Ci = w2.shape
        B, P = x.shape[0], x[0, 0].numel()
        dx = torch.empty_like(x) if fn_ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w2) if fn_ctx.needs_input_grad[1] else None
        db = torch.empty(Co, dtype=torch.float32, device=x.device) if fn_ctx.needs_input_grad[2] else None
        ws, nbytes = _workspace(lib.cabinet_conv1x1_bwd_workspace_bytes(B, Ci, Co, P), x.device)
        with torch.cuda.device(x.device):
            if dx is not None or dw is not None:
                rc = lib.cabinet_conv1x1_bwd(_ptr(g), _ptr(x), _ptr(w2), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes,
                                             _stream_handle(x.device))
                _lib.check(rc, "cabinet_conv1x1_bwd")
            if db is not None:
                _lib.check(lib.cabinet_channel_sum(_ptr(g), B, Co, P, _ptr(db), _stream_handle(x.device)), "cabinet_channel_sum")
        return dx, (dw.view(fn_ctx.w_shape) if dw is not None else None), db


def conv1x1(x, weight, bias=None):
    """1x1 convolution of a (B,Ci,...) device tensor with a (Co,Ci[,1,1]) weight (reference cab.py:155; with ``bias``:
    cabinet.py:65-66, ``convb``).  The bias form exists on the small-grid path only (``conv1x1_bias_supported``)."""
    if not x.is_cuda:
        raise RuntimeError("conv1x1: device tensors only")
    if bias is not None:
        return _Conv1x1Bias.apply(x, weight, bias)
    return _Conv1x1.apply(x, weight)


def conv1x1_bias_supported(x, conv):
    """True when ``conv(x)`` -- a plain 1x1 nn.Conv2d with bias -- runs through the small-grid MFMA path (the CAB's resolution)."""
    if not (x.is_cuda and x.dim() == 4 and conv.bias is not None and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.in_channels == x.shape[1]):
        return False
    if conv.in_channels % 4 or conv.out_channels % 4:
        return False
    return bool(_lib.load().cabinet_conv1x1_bias_supported(int(x.shape[0]), int(conv.in_channels), int(conv.out_channels),
                                                           int(x.shape[2] * x.shape[3])))


# --------------------------------------------------------------------------- dense 3x3 convolution (K11, Winograd on the fp32 MFMA)


# CABINET_CONV3X3=0: the model's plain 3x3 convolutions go back to the stock (MIOpen) operator -- same-box A/B timing only
CONV3X3_ENABLED = _os.environ.get("CABINET_CONV3X3", "1") != "0"


def conv3x3_supported(C0, C1, Co, H=None, W=None):
    """True when K11 takes ``nn.Conv2d(C0 + C1, Co, 3, padding=1, bias=False)`` over inputs of C0 (+ C1) channels -- and, when the
    spatial size is given, over images of H x W: zero padding rides on the buffer range check, which keeps one image's tensors below
    1 GiB (conv3x3_wino.hip: WN_OOB).  A layer past that limit takes the stock convolution instead of raising."""
    if not _lib.load().cabinet_conv3x3_supported(int(C0), int(C1), int(Co)):
        return False
    if H is None or W is None:
        return True
    return 4 * max(int(C0), int(C1), int(Co)) * int(H) * int(W) < (1 << 30)


def conv3x3_fwd_hip(x0, x1, weight, bn_part=None):
    lib = _lib.load()
    B, C0, H, W = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    Co = weight.shape[0]
    y = torch.empty((B, Co, H, W), dtype=torch.float32, device=x0.device)
    ws, nbytes = _workspace(lib.cabinet_conv3x3_fwd_workspace_bytes(B, C0, C1, Co, H, W), x0.device)
    with torch.cuda.device(x0.device):
        rc = lib.cabinet_conv3x3_fwd(_ptr(x0), _ptr(x1), _ptr(weight), B, C0, C1, Co, H, W, _ptr(y), _ptr(bn_part), _ptr(ws), nbytes,
                                     _stream_handle(x0.device))
    _lib.check(rc, "cabinet_conv3x3_fwd")
    return y


def conv3x3_bwd_hip(g, x0, x1, weight, need_dx=True, need_dw=True):
    lib = _lib.load()
    B, C0, H, W = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    Co = weight.shape[0]
    dx0 = torch.empty_like(x0) if need_dx else None
    dx1 = torch.empty_like(x1) if need_dx and x1 is not None else None
    dw = torch.empty_like(weight) if need_dw else None
    ws, nbytes = _workspace(lib.cabinet_conv3x3_bwd_workspace_bytes(B, C0, C1, Co, H, W), x0.device)
    with torch.cuda.device(x0.device):
        rc = lib.cabinet_conv3x3_bwd(_ptr(g), _ptr(x0), _ptr(x1), _ptr(weight), B, C0, C1, Co, H, W, _ptr(dx0), _ptr(dx1), _ptr(dw),
                                     _ptr(ws), nbytes, _stream_handle(x0.device))
    _lib.check(rc, "cabinet_conv3x3_bwd")
    return dx0, dx1, dw


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x0, x1, weight, bn_part=None):
        x0, weight = _f32c(x0), _f32c(weight)
        x1 = _f32c(x1) if x1 is not None else None
        y = conv3x3_fwd_hip(x0, x1, weight, bn_part)
        fn_ctx.save_for_backward(x0, x1, weight)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        x0, x1, weight = fn_ctx.saved_tensors
        need = fn_ctx.needs_input_grad
        dx0, dx1, dw = conv3x3_bwd_hip(_f32c(g), x0, x1, weight, need_dx=need[0] or (x1 is not None and need[1]), need_dw=need[2])
        return (dx0, dx1, dw) + (None,) * (len(need) - 3)


def conv3x3_bn_part(x, out_channels):
    """The (2, Co, blocks) buffer K11's epilogue fills with per-block (mean, M2) of its output for ``bn_act(..., conv_part=)``."""
    B, _, H, W = x.shape
    return torch.empty((2, out_channels, _lib.load().cabinet_conv3x3_tile_blocks(B, H, W)), dtype=torch.float32, device=x.device)


def conv3x3(x, weight, x1=None, bn_part=None):
    """``F.conv2d(cat([x, x1], 1), weight, padding=1)`` (``x1`` optional) for a bias-free 3x3 stride-1 convolution of device
    tensors, without the concat: reference cabinet.py:59, :68 + :88-89, :160.  ``bn_part`` (from :func:`conv3x3_bn_part`) receives
    the statistics partials of the output for the training-mode BatchNorm that follows."""
    if not x.is_cuda:
        raise RuntimeError("conv3x3: device tensors only")
    if bn_part is not None:
        return _Conv3x3.apply(x, x1, weight, bn_part)
    return _Conv3x3.apply(x, x1, weight)


# --------------------------------------------------------------------------- BatchNorm2d + activation (K7)

_ACT_CODES = {None: 0, "none": 0, "relu": 1, "hardswish": 2}


class _BnAct(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, weight, bias, run_mean, run_var, act, training, momentum, eps, residual=None, conv_part=None):
        lib = _lib.load()
        x, weight, bias = _f32c(x), _f32c(weight), _f32c(bias)
        residual = _f32c(residual) if residual is not None else None
        B, C = x.shape[0], x.shape[1]
        P = x[0, 0].numel()
        y = torch.empty_like(x)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        if conv_part is not None and x.dim() == 4:
            # x comes straight out of K11 with its per-block (mean, M2) pairs: no statistics pass over x
            with torch.cuda.device(x.device):
                rc = lib.cabinet_bn_act_fwd_part(_ptr(x), _ptr(conv_part), _ptr(weight), _ptr(bias), _ptr(run_mean), _ptr(run_var),
                                                 _ptr(residual), B, C, x.shape[2], x.shape[3], act, int(training), float(momentum),
                                                 float(eps), _ptr(y), _ptr(mean), _ptr(invstd), _stream_handle(x.device))
            _lib.check(rc, "cabinet_bn_act_fwd_part")
        else:
            ws, nbytes = _workspace(lib.cabinet_bn_act_workspace_bytes(B, C, P), x.device)
            with torch.cuda.device(x.device):
                rc = lib.cabinet_bn_act_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(run_mean), _ptr(run_var), _ptr(residual), B, C, P,
                                            act, int(training), float(momentum), float(eps), _ptr(y), _ptr(mean), _ptr(invstd),
                                            _ptr(ws), nbytes, _stream_handle(x.device))
            _lib.check(rc, "cabinet_bn_act_fwd")
        fn_ctx.save_for_backward(x, weight, bias, mean, invstd)
        fn_ctx.act, fn_ctx.training = act, bool(training)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, weight, bias, mean, invstd = fn_ctx.saved_tensors
        g = _f32c(g)
        B, C = x.shape[0], x.shape[1]
        P = x[0, 0].numel()
        dx, dw, db = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(bias)
        ws, nbytes = _workspace(lib.cabinet_bn_act_workspace_bytes(B, C, P), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_bn_act_bwd(_ptr(g), _ptr(x), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(invstd), B, C, P,
                                        fn_ctx.act, int(fn_ctx.training), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws),
                                        nbytes, _stream_handle(x.device))
        _lib.check(rc, "cabinet_bn_act_bwd")
        grads = (dx, dw, db, None, None, None, None, None, None)
        if len(fn_ctx.needs_input_grad) > 9:  # called with the optional residual operand: d(residual) = dy
            grads += (g if fn_ctx.needs_input_grad[9] else None,)
        if len(fn_ctx.needs_input_grad) > 10:  # ... and the producer's statistics partials (a buffer, not a variable)
            grads += (None,)
        return grads


def bn_act(x, bn, act=None, residual=None, conv_part=None):
    """act(bn(x)) [+ residual] for a device tensor; ``bn`` is the nn.BatchNorm2d owning parameters and running
    buffers (updated in place in training mode), ``act`` one of None / "relu" / "hardswish"
    (reference cabinet.py:42-44, mobilenetv3.py:86-99); ``residual`` is the MBConv identity shortcut
    (mobilenetv3.py:158), added in the same pass.  ``conv_part``: the (2, C, blocks) statistics partials ``conv3x3`` wrote
    while it produced ``x`` -- the batch statistics then cost no pass over ``x``."""
    if not x.is_cuda:
        raise RuntimeError("bn_act: device tensors only (host tensors take the composite ATen path)")
    if act not in _ACT_CODES:
        raise RuntimeError(f"bn_act: unknown activation {act!r}")
    training, momentum = _bn_step(bn)
    if residual is not None and residual.shape != x.shape:
        raise RuntimeError(f"bn_act: residual {tuple(residual.shape)} does not match x {tuple(x.shape)}")
    if conv_part is not None:
        return _BnAct.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, _ACT_CODES[act], training, momentum,
                            bn.eps, residual, conv_part)
    src = _pw_bn_source(x, bn)
    if src is not None:  # x = pwconv(...): one backward for the convolution and this BatchNorm (same forward calls)
        args = (src[0], src[1], x.detach(), bn.weight, bn.bias, bn.running_mean, bn.running_var, _ACT_CODES[act], training,
                momentum, bn.eps)
        return _PwBnAct.apply(*args, residual) if residual is not None else _PwBnAct.apply(*args)
    return _BnAct.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, _ACT_CODES[act], training, momentum,
                        bn.eps, residual)


# --------------------------------------------------------------------------- BatchNorm + ReLU + 1x1 classifier (K12)

# CABINET_BN_CLS=0 keeps the round-4 pair (K7 BatchNorm + ReLU, then the stock 1x1 convolution): A/B timing
BN_CLS_ENABLED = _os.environ.get("CABINET_BN_CLS", "1") != "0"


class _BnCls(torch.autograd.Function):
    """``conv1x1(relu(bn(z)))`` as one streaming operator (cabinet_bn_cls_fwd / _bwd): the activation and its gradient are never
    written.  Saved for backward: z and the per-channel table (classifier column, mean, invstd, gamma, beta)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, z, bn_w, bn_b, run_mean, run_var, w_cls, bias, training, momentum, eps, conv_part=None):
        lib = _lib.load()
        z = _f32c(z)
        B, C, H, W = z.shape
        K = w_cls.shape[0]
        w2 = _f32c(w_cls.detach()).reshape(K, C)
        y = torch.empty((B, K, H, W), dtype=torch.float32, device=z.device)
        tab = torch.empty(lib.cabinet_bn_cls_table_floats(C, K), dtype=torch.float32, device=z.device)
        ws, nbytes = _workspace(lib.cabinet_bn_cls_fwd_workspace_bytes(B, C, H * W), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_bn_cls_fwd(_ptr(z), _ptr(conv_part), _ptr(bn_w), _ptr(bn_b), _ptr(run_mean), _ptr(run_var), _ptr(w2),
                                        _ptr(bias), B, C, K, H, W, int(training), float(momentum), float(eps), _ptr(y), _ptr(tab),
                                        _ptr(ws), nbytes, _stream_handle(z.device))
        _lib.check(rc, "cabinet_bn_cls_fwd")
        fn_ctx.save_for_backward(z, tab)
        fn_ctx.training, fn_ctx.w_shape, fn_ctx.has_bias = bool(training), w_cls.shape, bias is not None
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        z, tab = fn_ctx.saved_tensors
        g = _f32c(g)
        B, C, H, W = z.shape
        K = g.shape[1]
        dz = torch.empty_like(z)
        dbn_w = torch.empty(C, dtype=torch.float32, device=z.device)
        dbn_b = torch.empty(C, dtype=torch.float32, device=z.device)
        dw = torch.empty((K, C), dtype=torch.float32, device=z.device)
        db = torch.empty(K, dtype=torch.float32, device=z.device) if fn_ctx.has_bias else None
        ws, nbytes = _workspace(lib.cabinet_bn_cls_bwd_workspace_bytes(B, C, K, H * W), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_bn_cls_bwd(_ptr(g), _ptr(z), _ptr(tab), B, C, K, H, W, int(fn_ctx.training), _ptr(dz), _ptr(dbn_w),
                                        _ptr(dbn_b), _ptr(dw), _ptr(db), _ptr(ws), nbytes, _stream_handle(z.device))
        _lib.check(rc, "cabinet_bn_cls_bwd")
        grads = (dz, dbn_w, dbn_b, None, None, dw.view(fn_ctx.w_shape), db, None, None, None)
        if len(fn_ctx.needs_input_grad) > 10:  # called with the producer's statistics partials (a buffer, not a variable)
            grads += (None,)
        return grads


def bn_relu_cls_supported(z, bn, cls):
    """True when ``cls(relu(bn(z)))`` runs as K12: a device (B,C,H,W) tensor, ``cls`` a plain 1x1 nn.Conv2d (stride 1, no padding,
    one group; bias optional), C % 64 == 0, at most 32 classes, H*W % 4 == 0."""
    if not (BN_CLS_ENABLED and z.is_cuda and z.dim() == 4):
        return False
    if not (cls.kernel_size == (1, 1) and cls.stride == (1, 1) and cls.padding == (0, 0) and cls.dilation == (1, 1)
            and cls.groups == 1 and cls.in_channels == z.shape[1] and bn.num_features == z.shape[1] and bn.affine
            and bn.track_running_stats):
        return False
    return bool(_lib.load().cabinet_bn_cls_supported(int(z.shape[1]), int(cls.out_channels), int(z.shape[2] * z.shape[3])))


def bn_relu_cls(z, bn, cls, conv_part=None):
    """``cls(relu(bn(z)))`` for a device tensor: ``bn`` the nn.BatchNorm2d (running buffers updated in place in training mode),
    ``cls`` the 1x1 nn.Conv2d classifier behind it (reference cabinet.py:90-92 and :161-172).  ONE operator (K12) where
    :func:`bn_relu_cls_supported`, K7 + the stock convolution otherwise.  ``conv_part``: the statistics partials ``conv3x3`` wrote
    while it produced ``z``."""
    if not bn_relu_cls_supported(z, bn, cls):
        return cls(bn_act(z, bn, "relu", conv_part=conv_part))
    training, momentum = _bn_step(bn)
    args = (z, bn.weight, bn.bias, bn.running_mean, bn.running_var, cls.weight, cls.bias, training, momentum, bn.eps)
    return _BnCls.apply(*args, conv_part) if conv_part is not None else _BnCls.apply(*args)


# --------------------------------------------------------------------------- depthwise convolution (K8)


def dwconv_supported(conv):
    """True for the depthwise nn.Conv2d shapes the HIP kernels cover (reference mobilenetv3.py:118-126)."""
    k, s = conv.kernel_size, conv.stride
    return (conv.groups == conv.in_channels == conv.out_channels and conv.bias is None and k[0] == k[1]
            and s[0] == s[1] and conv.padding == (k[0] // 2, k[0] // 2) and conv.dilation == (1, 1)
            and conv.padding_mode == "zeros" and k[0] in (3, 5) and s[0] in (1, 2))


class _DwConv(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, weight, stride):
        lib = _lib.load()
        x, w = _f32c(x), _f32c(weight)
        B, C, H, W = x.shape
        K = w.shape[-1]
        Ho, Wo = (H + 2 * (K // 2) - K) // stride + 1, (W + 2 * (K // 2) - K) // stride + 1
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_dwconv_fwd(_ptr(x), _ptr(w), B, C, H, W, K, stride, _ptr(y), _stream_handle(x.device))
        _lib.check(rc, "cabinet_dwconv_fwd")
        fn_ctx.save_for_backward(x, w)
        fn_ctx.stride = stride
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, w = fn_ctx.saved_tensors
        g = _f32c(g)
        B, C, H, W = x.shape
        K, stride = w.shape[-1], fn_ctx.stride
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        ws, nbytes = _workspace(lib.cabinet_dwconv_bwd_workspace_bytes(B, C, H, W, K, stride), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_dwconv_bwd(_ptr(g), _ptr(x), _ptr(w), B, C, H, W, K, stride, _ptr(dx), _ptr(dw), _ptr(ws),
                                        nbytes, _stream_handle(x.device))
        _lib.check(rc, "cabinet_dwconv_bwd")
        return dx, dw, None


def dwconv(x, conv):
    """Depthwise convolution of a device tensor with the weights of ``conv`` (an nn.Conv2d, see dwconv_supported)."""
    if not x.is_cuda:
        raise RuntimeError("dwconv: device tensors only")
    return _DwConv.apply(x, conv.weight, conv.stride[0])


# --------------------------------------------------------------------------- channel gate + activation (SE tail)


class _GateAct(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, gate, act):
        lib = _lib.load()
        x, gate = _f32c(x), _f32c(gate)
        B, C = x.shape[0], x.shape[1]
        P = x[0, 0].numel()
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_gate_act_fwd(_ptr(x), _ptr(gate), B, C, P, act, _ptr(y), _stream_handle(x.device))
        _lib.check(rc, "cabinet_gate_act_fwd")
        fn_ctx.save_for_backward(x, gate)
        fn_ctx.act = act
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, gate = fn_ctx.saved_tensors
        g = _f32c(g)
        B, C = x.shape[0], x.shape[1]
        P = x[0, 0].numel()
        dx, dgate = torch.empty_like(x), torch.empty_like(gate)
        ws, nbytes = _workspace(lib.cabinet_gate_act_bwd_workspace_bytes(B, C, P), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_gate_act_bwd(_ptr(g), _ptr(x), _ptr(gate), B, C, P, fn_ctx.act, _ptr(dx), _ptr(dgate),
                                          _ptr(ws), nbytes, _stream_handle(x.device))
        _lib.check(rc, "cabinet_gate_act_bwd")
        return dx, dgate, None


def gate_act(x, gate, act=None):
    """act(x * gate[:, :, None, None]) for a device tensor x (B,C,H,W) and a (B,C) gate: the tail of SELayer.forward
    (reference mobilenetv3.py:79-83) fused with the activation that follows it in the MBConv block."""
    if not x.is_cuda:
        raise RuntimeError("gate_act: device tensors only")
    if act not in _ACT_CODES:
        raise RuntimeError(f"gate_act: unknown activation {act!r}")
    if gate.shape != x.shape[:2]:
        raise RuntimeError(f"gate_act: gate {tuple(gate.shape)} does not match x {tuple(x.shape)}")
    return _GateAct.apply(x, gate, _ACT_CODES[act])


# --------------------------------------------------------------------------- BatchNorm -> SELayer -> act (SE tail)

# CABINET_SE_MLP_FUSED=0: the MLP's backward between the two streaming passes goes back to the chain of torch ops followed by
# cabinet_se_act_bwd_coef -- same-box A/B timing and the equality tests
SE_MLP_FUSED = _os.environ.get("CABINET_SE_MLP_FUSED", "1") != "0"


class _SeTail(torch.autograd.Function):
    """``act(se(bn(z)))`` with ``se(x) = x * hsig(fc2(relu(fc1(avgpool(x)))))`` as ONE autograd node.  The forward runs the
    very kernels of the composed form (K7 BatchNorm, the stock pool, the MLP, gate_act_fwd: bitwise the same output); the
    backward replaces gate_act_bwd + the pool's broadcast gradient + autograd's add + K7's reduce and dx by two passes over
    (dy, z) (include/cabinet_hip.h: cabinet_se_act_bwd_*).  Between them the MLP's backward on (B, C) and the BatchNorm
    coefficients are two launches (cabinet_se_act_bwd_mlp; SE_MLP_FUSED off, or an MLP wider than its kernels stage: the chain
    of torch ops and cabinet_se_act_bwd_coef), with autograd's conventions at the clamp boundaries (ReLU: gradient where the
    output is > 0; ReLU6: where 0 < input < 6).  Saved for backward: z, not the BatchNorm output."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, z, bn_w, bn_b, run_mean, run_var, w1, b1, w2, b2, act, training, momentum, eps):
        lib = _lib.load()
        z, bn_w, bn_b = _f32c(z), _f32c(bn_w), _f32c(bn_b)
        B, C, H, W = z.shape
        P = H * W
        dev = z.device
        x = torch.empty_like(z)
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty(C, dtype=torch.float32, device=dev)
        ws, nbytes = _workspace(lib.cabinet_bn_act_workspace_bytes(B, C, P), dev)
        with torch.cuda.device(dev):
            rc = lib.cabinet_bn_act_fwd(_ptr(z), _ptr(bn_w), _ptr(bn_b), _ptr(run_mean), _ptr(run_var), None, B, C, P, 0,
                                        int(training), float(momentum), float(eps), _ptr(x), _ptr(mean), _ptr(invstd), _ptr(ws),
                                        nbytes, _stream_handle(dev))
        _lib.check(rc, "cabinet_bn_act_fwd")
        pooled = F.adaptive_avg_pool2d(x, 1).view(B, C)  # SELayer.gate (mobilenetv3.py:64-66), op for op
        h1 = torch.relu(F.linear(pooled, w1, b1))
        a2 = F.linear(h1, w2, b2)
        gate = F.relu6(a2 + 3) / 6  # HardSigmoid (mobilenetv3.py:38-50)
        y = torch.empty_like(z)
        with torch.cuda.device(dev):
            rc = lib.cabinet_gate_act_fwd(_ptr(x), _ptr(gate), B, C, P, act, _ptr(y), _stream_handle(dev))
        _lib.check(rc, "cabinet_gate_act_fwd")
        fn_ctx.save_for_backward(z, bn_w, bn_b, mean, invstd, pooled, h1, a2, gate, w1, w2)
        fn_ctx.act, fn_ctx.training = act, bool(training)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        z, bn_w, bn_b, mean, invstd, pooled, h1, a2, gate, w1, w2 = fn_ctx.saved_tensors
        g = _f32c(g)
        B, C, H, W = z.shape
        P = H * W
        dev = z.device
        stream = _stream_handle(dev)
        sums = torch.empty((3, B, C), dtype=torch.float32, device=dev)  # sum_p du, sum_p du * xhat, sum_p xhat
        da2 = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws, nbytes = _workspace(lib.cabinet_se_act_bwd_workspace_bytes(B, C, P), dev)
        with torch.cuda.device(dev):
            rc = lib.cabinet_se_act_bwd_reduce(_ptr(g), _ptr(z), _ptr(mean), _ptr(invstd), _ptr(bn_w), _ptr(bn_b), _ptr(gate), _ptr(a2),
                                               B, C, P, fn_ctx.act, _ptr(sums), _ptr(da2), _ptr(ws), nbytes, stream)
        _lib.check(rc, "cabinet_se_act_bwd_reduce")
        dweight, dbias = torch.empty_like(bn_w), torch.empty_like(bn_b)
        coef = torch.empty((2, C), dtype=torch.float32, device=dev)
        ds_p = torch.empty((B, C), dtype=torch.float32, device=dev)
        Cs = w1.shape[0]
        # the MLP's backward and the coefficients in two launches (csrc/se_mlp.hip); with CABINET_SE_MLP_FUSED=0, or for an MLP
        # wider than those kernels stage (no SELayer of the two backbones is), the chain of torch ops and the coefficient kernel
        if SE_MLP_FUSED and lib.cabinet_se_act_bwd_mlp_supported(C, Cs):
            pooled, h1, w1, w2 = _f32c(pooled), _f32c(h1), _f32c(w1), _f32c(w2)
            dw1, db1 = torch.empty_like(w1), torch.empty(Cs, dtype=torch.float32, device=dev)
            dw2, db2 = torch.empty_like(w2), torch.empty(C, dtype=torch.float32, device=dev)
            ds = torch.empty((B, C), dtype=torch.float32, device=dev)
            mlp_ws, mlp_nbytes = _workspace(lib.cabinet_se_act_bwd_mlp_workspace_bytes(B, C, Cs), dev)
            with torch.cuda.device(dev):
                rc = lib.cabinet_se_act_bwd_mlp(_ptr(sums), _ptr(da2), _ptr(gate), _ptr(h1), _ptr(pooled), _ptr(w1), _ptr(w2), B, C,
                                                Cs, P, int(fn_ctx.training), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(ds),
                                                _ptr(dweight), _ptr(dbias), _ptr(coef), _ptr(ds_p), _ptr(mlp_ws), mlp_nbytes, stream)
            _lib.check(rc, "cabinet_se_act_bwd_mlp")
        else:
            dw2, db2 = da2.t().mm(h1), da2.sum(0)
            da1 = da2.mm(w2) * (h1 > 0)
            dw1, db1 = da1.t().mm(pooled), da1.sum(0)
            ds = da1.mm(w1)  # gradient of the pooled input
            with torch.cuda.device(dev):
                rc = lib.cabinet_se_act_bwd_coef(_ptr(sums), _ptr(gate), _ptr(ds), B, C, P, int(fn_ctx.training), _ptr(dweight),
                                                 _ptr(dbias), _ptr(coef), _ptr(ds_p), stream)
            _lib.check(rc, "cabinet_se_act_bwd_coef")
        dz = torch.empty_like(z)
        with torch.cuda.device(dev):
            rc = lib.cabinet_se_act_bwd_dx(_ptr(g), _ptr(z), _ptr(mean), _ptr(invstd), _ptr(bn_w), _ptr(bn_b), _ptr(gate), _ptr(ds_p),
                                           _ptr(coef), B, C, P, fn_ctx.act, _ptr(dz), stream)
        _lib.check(rc, "cabinet_se_act_bwd_dx")
        return dz, dweight, dbias, None, None, dw1, db1, dw2, db2, None, None, None, None


def se_tail(z, bn, se, act=None):
    """``act(se(bn(z)))`` for a device tensor z (B,C,H,W): ``bn`` the nn.BatchNorm2d (running buffers updated in place in
    training mode), ``se`` the SELayer (its ``fc.0`` / ``fc.2`` Linear layers), ``act`` None / "relu" / "hardswish" -- the
    `BatchNorm, SELayer, act` run of the MBConv block (reference mobilenetv3.py:146-149, SELayer :68-83)."""
    if not z.is_cuda:
        raise RuntimeError("se_tail: device tensors only")
    if act not in _ACT_CODES:
        raise RuntimeError(f"se_tail: unknown activation {act!r}")
    fc1, fc2 = se.fc[0], se.fc[2]
    training, momentum = _bn_step(bn)
    return _SeTail.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, fc1.weight, fc1.bias, fc2.weight, fc2.bias,
                         _ACT_CODES[act], training, momentum, bn.eps)


# --------------------------------------------------------------------------- BatchNorm (+act) -> depthwise conv, fused


class _BnActDwConv(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, z, bn_w, bn_b, run_mean, run_var, conv_w, act, stride, training, momentum, eps):
        lib = _lib.load()
        z, bn_w, bn_b, cw = _f32c(z), _f32c(bn_w), _f32c(bn_b), _f32c(conv_w)
        B, C, H, W = z.shape
        K = cw.shape[-1]
        Ho, Wo = (H + 2 * (K // 2) - K) // stride + 1, (W + 2 * (K // 2) - K) // stride + 1
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=z.device)
        mean = torch.empty(C, dtype=torch.float32, device=z.device)
        invstd = torch.empty(C, dtype=torch.float32, device=z.device)
        ws, nbytes = _workspace(lib.cabinet_bn_dwconv_fwd_workspace_bytes(B, C, H, W), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_bn_dwconv_fwd(_ptr(z), _ptr(bn_w), _ptr(bn_b), _ptr(run_mean), _ptr(run_var), _ptr(cw), B, C,
                                           H, W, K, stride, act, int(training), float(momentum), float(eps), _ptr(y),
                                           _ptr(mean), _ptr(invstd), _ptr(ws), nbytes, _stream_handle(z.device))
        _lib.check(rc, "cabinet_bn_dwconv_fwd")
        fn_ctx.save_for_backward(z, bn_w, bn_b, cw, mean, invstd)
        fn_ctx.meta = (act, stride, bool(training))
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        z, bn_w, bn_b, cw, mean, invstd = fn_ctx.saved_tensors
        act, stride, training = fn_ctx.meta
        g = _f32c(g)
        B, C, H, W = z.shape
        K = cw.shape[-1]
        dz, dbw, dbb, dcw = torch.empty_like(z), torch.empty_like(bn_w), torch.empty_like(bn_b), torch.empty_like(cw)
        ws, nbytes = _workspace(lib.cabinet_bn_dwconv_bwd_workspace_bytes(B, C, H, W, K, stride), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_bn_dwconv_bwd(_ptr(g), _ptr(z), _ptr(bn_w), _ptr(bn_b), _ptr(mean), _ptr(invstd), _ptr(cw), B,
                                           C, H, W, K, stride, act, int(training), _ptr(dz), _ptr(dbw), _ptr(dbb),
                                           _ptr(dcw), _ptr(ws), nbytes, _stream_handle(z.device))
        _lib.check(rc, "cabinet_bn_dwconv_bwd")
        return dz, dbw, dbb, None, None, dcw, None, None, None, None, None


def bn_act_dwconv(z, bn, act, conv):
    """conv(act(bn(z))) for a depthwise ``conv`` (see dwconv_supported) on a device tensor, without materialising the
    normalised tensor (reference mobilenetv3.py:135-143)."""
    if not z.is_cuda:
        raise RuntimeError("bn_act_dwconv: device tensors only")
    if act not in _ACT_CODES:
        raise RuntimeError(f"bn_act_dwconv: unknown activation {act!r}")
    training, momentum = _bn_step(bn)
    src = _pw_bn_source(z, bn, conv.weight)
    if src is not None:  # z = pwconv(...): one backward for that convolution and this BatchNorm (same forward calls)
        return _PwBnActDwConv.apply(src[0], src[1], z.detach(), bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.weight,
                                    _ACT_CODES[act], conv.stride[0], training, momentum, bn.eps)
    return _BnActDwConv.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.weight, _ACT_CODES[act],
                              conv.stride[0], training, momentum, bn.eps)


# --------------------------------------------------------------------------- 7x7 stride-2 stem convolution (K9)


def stem_conv_supported(conv):
    """True for the spatial branch's first convolution (reference cabinet.py:111): 3 -> 64, 7x7, stride 2, pad 3."""
    return (conv.in_channels == 3 and conv.out_channels == 64 and conv.kernel_size == (7, 7) and conv.stride == (2, 2)
            and conv.padding == (3, 3) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.padding_mode == "zeros")


class _StemConv(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, weight):
        lib = _lib.load()
        x, w = _f32c(x), _f32c(weight)
        B, _, H, W = x.shape
        y = torch.empty((B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_stem_conv_fwd(_ptr(x), _ptr(w), B, H, W, _ptr(y), _stream_handle(x.device))
        _lib.check(rc, "cabinet_stem_conv_fwd")
        fn_ctx.save_for_backward(x, w)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, w = fn_ctx.saved_tensors
        g = _f32c(g)
        B, _, H, W = x.shape
        dx = None
        if fn_ctx.needs_input_grad[0]:  # not the training step (the input is the image); served by ATen when asked for
            dx = torch.ops.aten.convolution_backward(g, x, w, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0]
        dw = torch.empty_like(w)
        ws, nbytes = _workspace(lib.cabinet_stem_conv_wrw_workspace_bytes(B, H, W), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_stem_conv_wrw(_ptr(g), _ptr(x), B, H, W, _ptr(dw), _ptr(ws), nbytes,
                                           _stream_handle(x.device))
        _lib.check(rc, "cabinet_stem_conv_wrw")
        return dx, dw


def stem_conv(x, conv):
    """The spatial branch's 7x7/2 stem convolution on a device tensor (see stem_conv_supported)."""
    if not x.is_cuda:
        raise RuntimeError("stem_conv: device tensors only")
    return _StemConv.apply(x, conv.weight)


# CABINET_STEM_BN_FUSED=0: the stem goes back to the two nodes bn_act(stem_conv(...)) -- same-box A/B timing and the equality tests
STEM_BN_FUSED = _os.environ.get("CABINET_STEM_BN_FUSED", "1") != "0"


class _StemConvBnRelu(torch.autograd.Function):
    """relu(bn(stem_conv(image))) as one node: the forward is K9's and K7's, called in that order; the backward never writes the
    BatchNorm's input gradient (B, 64, H/2, W/2) -- its only reader, the weight-gradient kernel, forms it while staging."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, weight, bn_weight, bn_bias, run_mean, run_var, training, momentum, eps):
        lib = _lib.load()
        x, w, bn_weight, bn_bias = _f32c(x), _f32c(weight), _f32c(bn_weight), _f32c(bn_bias)
        B, _, H, W = x.shape
        z = torch.empty((B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
        y = torch.empty_like(z)
        mean = torch.empty(64, dtype=torch.float32, device=x.device)
        invstd = torch.empty(64, dtype=torch.float32, device=x.device)
        P = z.shape[2] * z.shape[3]
        with torch.cuda.device(x.device):
            rc = lib.cabinet_stem_conv_fwd(_ptr(x), _ptr(w), B, H, W, _ptr(z), _stream_handle(x.device))
            _lib.check(rc, "cabinet_stem_conv_fwd")
            ws, nbytes = _workspace(lib.cabinet_bn_act_workspace_bytes(B, 64, P), x.device)
            rc = lib.cabinet_bn_act_fwd(_ptr(z), _ptr(bn_weight), _ptr(bn_bias), _ptr(run_mean), _ptr(run_var), None, B, 64, P,
                                        _ACT_CODES["relu"], int(training), float(momentum), float(eps), _ptr(y), _ptr(mean),
                                        _ptr(invstd), _ptr(ws), nbytes, _stream_handle(x.device))
            _lib.check(rc, "cabinet_bn_act_fwd")
        fn_ctx.save_for_backward(x, z, w, bn_weight, bn_bias, mean, invstd)
        fn_ctx.training = bool(training)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, z, w, bn_weight, bn_bias, mean, invstd = fn_ctx.saved_tensors
        g = _f32c(g)
        B, _, H, W = x.shape
        dw, dgam, dbet = torch.empty_like(w), torch.empty_like(bn_weight), torch.empty_like(bn_bias)
        ws, nbytes = _workspace(lib.cabinet_stem_conv_bn_bwd_workspace_bytes(B, H, W), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_stem_conv_bn_bwd(_ptr(g), _ptr(z), _ptr(x), _ptr(bn_weight), _ptr(bn_bias), _ptr(mean), _ptr(invstd),
                                              B, H, W, int(fn_ctx.training), _ptr(dw), _ptr(dgam), _ptr(dbet), _ptr(ws), nbytes,
                                              _stream_handle(x.device))
        _lib.check(rc, "cabinet_stem_conv_bn_bwd")
        return None, dw, dgam, dbet, None, None, None, None, None


def stem_conv_bn_relu(x, conv, bn):
    """``relu(bn(conv(x)))`` for the stem (see stem_conv_supported) on an image that needs no gradient: the values, the running
    buffers and the three parameter gradients of ``bn_act(stem_conv(x, conv), bn, "relu")``, bit for bit, without the BatchNorm's
    dx pass (reference cabinet.py:111 with :42-44)."""
    if not x.is_cuda:
        raise RuntimeError("stem_conv_bn_relu: device tensors only")
    if x.requires_grad:
        raise RuntimeError("stem_conv_bn_relu: the image gets no gradient here; use bn_act(stem_conv(...))")
    training, momentum = _bn_step(bn)
    return _StemConvBnRelu.apply(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps)


# --------------------------------------------------------------------------- thin pointwise convolution (K10)


def pwconv_supported(conv, x):
    """True for the bias-free stride-1 1x1 convolutions the streaming kernels cover (thin channel counts on large
    planes, reference mobilenetv3.py:128-131,144-151); others stay with MIOpen, which is as fast there."""
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
            and conv.bias is None and conv.dilation == (1, 1)):
        return False
    P = x.shape[2] * x.shape[3]
    # measured on MI355X (tools/time_pwconv*.py): the streaming kernels win where the layer is HBM-bound -- planes of
    # >= 256 x 256 pixels with <= 96 channels either side (2.5x forward / input gradient, 1.3x weight gradient)
    return (P >= 65536 and conv.in_channels <= 96 and conv.out_channels <= 96
            and bool(_lib.load().cabinet_pwconv_supported(conv.in_channels, conv.out_channels, P)))


class _PwConv(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(fn_ctx, x, weight):
        lib = _lib.load()
        x = _f32c(x)
        Co, Ci = weight.shape[0], weight.shape[1]
        w2 = _f32c(weight).view(Co, Ci)
        B, P = x.shape[0], x.shape[2] * x.shape[3]
        y = torch.empty((B, Co) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_pwconv_fwd(_ptr(x), _ptr(w2), B, Ci, Co, P, _ptr(y), _stream_handle(x.device))
        _lib.check(rc, "cabinet_pwconv_fwd")
        fn_ctx.save_for_backward(x, w2)
        fn_ctx.w_shape = weight.shape
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, w2 = fn_ctx.saved_tensors
        g = _f32c(g)
        Co, Ci = w2.shape
        B, P = x.shape[0], x.shape[2] * x.shape[3]
        dx = torch.empty_like(x) if fn_ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w2) if fn_ctx.needs_input_grad[1] else None
        ws, nbytes = _workspace(lib.cabinet_pwconv_bwd_workspace_bytes(B, Ci, Co, P), x.device)
        with torch.cuda.device(x.device):
            rc = lib.cabinet_pwconv_bwd(_ptr(g), _ptr(x), _ptr(w2), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes,
                                        _stream_handle(x.device))
        _lib.check(rc, "cabinet_pwconv_bwd")
        return dx, (dw.view(fn_ctx.w_shape) if dw is not None else None)


def pwconv(x, conv):
    """Thin pointwise convolution of a device tensor with the weights of ``conv`` (see pwconv_supported)."""
    if not x.is_cuda:
        raise RuntimeError("pwconv: device tensors only")
    y = _PwConv.apply(x, conv.weight)
    if PW_BN_BWD_FUSED and y.requires_grad:
        y._pw_src = (x, conv.weight)  # for the BatchNorm that consumes y: see _pw_bn_source
    return y


# CABINET_PW_BN_BWD_FUSED=0: a thin 1x1 convolution and the BatchNorm behind it go back to their two backward nodes -- same-box A/B
# timing and the equality tests
PW_BN_BWD_FUSED = _os.environ.get("CABINET_PW_BN_BWD_FUSED", "1") != "0"


def _pw_bn_source(z, bn, *more_params):
    """``(x, weight)`` of the thin 1x1 convolution (:func:`pwconv`) that produced ``z`` when its backward can be taken together
    with the backward of the BatchNorm ``bn`` that consumes ``z`` (cabinet_pw_bn_*_bwd), else None: the flag is on, a graph is
    being recorded outside autocast, every parameter involved is trainable fp32 and the shape is one the kernel takes."""
    src = getattr(z, "_pw_src", None)
    if src is None or not PW_BN_BWD_FUSED or not torch.is_grad_enabled() or torch.is_autocast_enabled():
        return None
    x, w = src
    params = (w, bn.weight, bn.bias) + more_params
    if not all(p.requires_grad and p.dtype == torch.float32 for p in params):
        return None
    if not (z.dim() == 4 and z.dtype == torch.float32 and x.dtype == torch.float32 and z.is_contiguous() and x.is_contiguous()):
        return None
    if not _lib.load().cabinet_pw_bn_bwd_supported(w.shape[1], w.shape[0], z.shape[2] * z.shape[3]):
        return None
    return x, w


class _PwBnAct(torch.autograd.Function):
    """act(bn(z)) [+ residual] for z = pwconv(x, w), as the node of BOTH: the forward is K7's call on z (the convolution has run,
    its own node receives no gradient and never runs), the backward is cabinet_pw_bn_act_bwd -- the BatchNorm's input gradient
    (B, Co, H, W) is never written; the weight-gradient kernel forms it while staging and multiplies it by W^T as well."""

    @staticmethod
    def forward(fn_ctx, x, w, z, bn_w, bn_b, run_mean, run_var, act, training, momentum, eps, residual=None):
        lib = _lib.load()
        bn_w, bn_b = _f32c(bn_w), _f32c(bn_b)
        residual = _f32c(residual) if residual is not None else None
        B, C, P = z.shape[0], z.shape[1], z.shape[2] * z.shape[3]
        y = torch.empty_like(z)
        mean = torch.empty(C, dtype=torch.float32, device=z.device)
        invstd = torch.empty(C, dtype=torch.float32, device=z.device)
        ws, nbytes = _workspace(lib.cabinet_bn_act_workspace_bytes(B, C, P), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_bn_act_fwd(_ptr(z), _ptr(bn_w), _ptr(bn_b), _ptr(run_mean), _ptr(run_var), _ptr(residual), B, C, P,
                                        act, int(training), float(momentum), float(eps), _ptr(y), _ptr(mean), _ptr(invstd),
                                        _ptr(ws), nbytes, _stream_handle(z.device))
        _lib.check(rc, "cabinet_bn_act_fwd")
        fn_ctx.save_for_backward(x, _f32c(w).view(w.shape[0], w.shape[1]), z, bn_w, bn_b, mean, invstd)
        fn_ctx.meta = (act, bool(training), w.shape)
        return y

    @staticmethod
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, w2, z, bn_w, bn_b, mean, invstd = fn_ctx.saved_tensors
        act, training, w_shape = fn_ctx.meta
        need = fn_ctx.needs_input_grad
        g = _f32c(g)
        Co, Ci = w2.shape
        B, P = z.shape[0], z.shape[2] * z.shape[3]
        dx = torch.empty_like(x) if need[0] else None
        dw = torch.empty_like(w2) if need[1] else None
        dgam, dbet = torch.empty_like(bn_w), torch.empty_like(bn_b)
        ws, nbytes = _workspace(lib.cabinet_pw_bn_act_bwd_workspace_bytes(B, Ci, Co, P), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_pw_bn_act_bwd(_ptr(g), _ptr(z), _ptr(x), _ptr(w2), _ptr(bn_w), _ptr(bn_b), _ptr(mean), _ptr(invstd),
                                           B, Ci, Co, P, act, int(training), _ptr(dx), _ptr(dw), _ptr(dgam), _ptr(dbet),
                                           _ptr(ws), nbytes, _stream_handle(z.device))
        _lib.check(rc, "cabinet_pw_bn_act_bwd")
        grads = (dx, dw.view(w_shape) if dw is not None else None, None, dgam, dbet) + (None,) * 6
        if len(need) > 11:  # called with the shortcut: d(residual) = dy
            grads += (g if need[11] else None,)
        return grads


class _PwBnActDwConv(torch.autograd.Function):
    """conv(act(bn(z))) for z = pwconv(x, w) and a depthwise ``conv``, as the node of both: the forward is
    cabinet_bn_dwconv_fwd on z, the backward cabinet_pw_bn_dwconv_bwd (see _PwBnAct)."""

    @staticmethod
    def forward(fn_ctx, x, w, z, bn_w, bn_b, run_mean, run_var, conv_w, act, stride, training, momentum, eps):
        lib = _lib.load()
        bn_w, bn_b, cw = _f32c(bn_w), _f32c(bn_b), _f32c(conv_w)
        B, C, H, W = z.shape
        K = cw.shape[-1]
        Ho, Wo = (H + 2 * (K // 2) - K) // stride + 1, (W + 2 * (K // 2) - K) // stride + 1
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=z.device)
        mean = torch.empty(C, dtype=torch.float32, device=z.device)
        invstd = torch.empty(C, dtype=torch.float32, device=z.device)
        ws, nbytes = _workspace(lib.cabinet_bn_dwconv_fwd_workspace_bytes(B, C, H, W), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_bn_dwconv_fwd(_ptr(z), _ptr(bn_w), _ptr(bn_b), _ptr(run_mean), _ptr(run_var), _ptr(cw), B, C,
                                           H, W, K, stride, act, int(training), float(momentum), float(eps), _ptr(y),
                                           _ptr(mean), _ptr(invstd), _ptr(ws), nbytes, _stream_handle(z.device))
        _lib.check(rc, "cabinet_bn_dwconv_fwd")
        fn_ctx.save_for_backward(x, _f32c(w).view(w.shape[0], w.shape[1]), z, bn_w, bn_b, cw, mean, invstd)
        fn_ctx.meta = (act, stride, bool(training), w.shape)
        return y

    @staticmethod
    def backward(fn_ctx, g):
        lib = _lib.load()
        x, w2, z, bn_w, bn_b, cw, mean, invstd = fn_ctx.saved_tensors
        act, stride, training, w_shape = fn_ctx.meta
        need = fn_ctx.needs_input_grad
        g = _f32c(g)
        B, C, H, W = z.shape
        Ci, K = w2.shape[1], cw.shape[-1]
        dx = torch.empty_like(x) if need[0] else None
        dw = torch.empty_like(w2) if need[1] else None
        dgam, dbet, dcw = torch.empty_like(bn_w), torch.empty_like(bn_b), torch.empty_like(cw)
        ws, nbytes = _workspace(lib.cabinet_pw_bn_dwconv_bwd_workspace_bytes(B, Ci, C, H, W, K, stride), z.device)
        with torch.cuda.device(z.device):
            rc = lib.cabinet_pw_bn_dwconv_bwd(_ptr(g), _ptr(z), _ptr(x), _ptr(w2), _ptr(bn_w), _ptr(bn_b), _ptr(mean),
                                              _ptr(invstd), _ptr(cw), B, Ci, C, H, W, K, stride, act, int(training), _ptr(dx),
                                              _ptr(dw), _ptr(dgam), _ptr(dbet), _ptr(dcw), _ptr(ws), nbytes,
                                              _stream_handle(z.device))
        _lib.check(rc, "cabinet_pw_bn_dwconv_bwd")
        return (dx, dw.view(w_shape) if dw is not None else None, None, dgam, dbet, None, None, dcw) + (None,) * 5


# --------------------------------------------------------------------------- wide pointwise convolution: weight gradient (K14)


# CABINET_PWCONV_WIDE=0: the wide 1x1 convolutions go back to the stock operator entirely (MIOpen weight gradient with its
# NCHW -> NHWC copies) -- same-box A/B timing only
PWCONV_WIDE_ENABLED = _os.environ.get("CABINET_PWCONV_WIDE", "1") != "0"


def pwconv_wide_supported(conv, x):
    """True for the bias-free stride-1 1x1 convolutions whose WEIGHT GRADIENT K14 computes straight on NCHW (every such
    layer K10 does not take: reference mobilenetv3.py:128-131,144-151,193, cabinet.py:114) -- in a forward that records a
    graph for autograd only; fp32 device tensors outside autocast.  Forward and input gradient stay the stock operator's."""
    if not (PWCONV_WIDE_ENABLED and isinstance(conv, torch.nn.Conv2d) and x.is_cuda and x.dim() == 4):
        return False
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
            and conv.bias is None and conv.dilation == (1, 1)):
        return False
    if not (torch.is_grad_enabled() and conv.weight.requires_grad) or torch.is_autocast_enabled():
        return False
    if x.dtype != torch.float32 or conv.weight.dtype != torch.float32 or x.shape[0] < 1 or x.shape[2] * x.shape[3] < 1:
        return False
    return bool(_lib.load().cabinet_pwconv_wide_supported(conv.in_channels, conv.out_channels, x.shape[2] * x.shape[3]))


class _PwConvWide(torch.autograd.Function):
    """y = conv2d(x, weight) with the stock forward and input gradient; dw by cabinet_pwconv_wide_wgrad."""

    @staticmethod
    def forward(fn_ctx, x, weight):
        x = x.contiguous()  # dense NCHW for the stock operator too (a no-op in the model): a channels_last input sends it to another solver
        y = F.conv2d(x, weight)
        fn_ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(fn_ctx, g):
        x, w = fn_ctx.saved_tensors
        g = g.contiguous()
        dx = None
        if fn_ctx.needs_input_grad[0]:
            dx = torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0]
        dw = None
        if fn_ctx.needs_input_grad[1]:
            lib = _lib.load()
            xc, gc = _f32c(x), _f32c(g)
            Co, Ci = w.shape[0], w.shape[1]
            B, P = xc.shape[0], xc.shape[2] * xc.shape[3]
            dw = torch.empty((Co, Ci, 1, 1), dtype=torch.float32, device=x.device)
            ws, nbytes = _workspace(lib.cabinet_pwconv_wide_wgrad_workspace_bytes(B, Ci, Co, P), x.device)
            with torch.cuda.device(x.device):
                rc = lib.cabinet_pwconv_wide_wgrad(_ptr(gc), _ptr(xc), B, Ci, Co, P, _ptr(dw), _ptr(ws), nbytes,
                                                   _stream_handle(x.device))
            _lib.check(rc, "cabinet_pwconv_wide_wgrad")
        return dx, dw


def pwconv_wide(x, conv):
    """1x1 convolution of a device tensor with the weights of ``conv`` (see pwconv_wide_supported)."""
    if not x.is_cuda:
        raise RuntimeError("pwconv_wide: device tensors only")
    return _PwConvWide.apply(x, conv.weight)


# --------------------------------------------------------------------------- 3x3 stride-2 convolution: weight gradient (K15)


# CABINET_CONV3X3S2=0: the 3x3 stride-2 convolutions go back to the stock operator entirely (MIOpen input gradient, MIOpen
# weight gradient with its NCHW <-> NHWC copies for the first layer too) -- same-box A/B timing only
CONV3X3S2_ENABLED = _os.environ.get("CABINET_CONV3X3S2", "1") != "0"


def conv3x3s2_supported(conv, x):
    """True for the bias-free 3x3 stride-2 padding-1 convolutions whose BACKWARD K15 computes straight on NCHW (the spatial
    branch's conv2 / conv3, reference cabinet.py:112-113, and the backbone's first layer, mobilenetv3.py:173) -- in a forward
    that records a graph for autograd only; fp32 device tensors outside autocast.  Which part of which layer goes native is
    _Conv3x3S2's business (64 -> 64: the forward by _conv3x3s2_native_fwd64, dx always, dw by _conv3x3s2_native_wgrad64;
    3 -> 16: stock forward, dw by _conv3x3s2_native_wgrad)."""
    if not (CONV3X3S2_ENABLED and isinstance(conv, torch.nn.Conv2d) and x.is_cuda and x.dim() == 4):
        return False
    if not (conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.dilation == (1, 1) and conv.padding_mode == "zeros"):
        return False
    if not (torch.is_grad_enabled() and conv.weight.requires_grad) or torch.is_autocast_enabled():
        return False
    if x.dtype != torch.float32 or conv.weight.dtype != torch.float32 or x.shape[0] < 1 or x.shape[2] * x.shape[3] < 1:
        return False
    return x.shape[1] == conv.in_channels and bool(_lib.load().cabinet_conv3x3s2_supported(conv.in_channels, conv.out_channels))


def _conv3x3s2_native_wgrad(Ci, B, H):
    """The routing rule of the 3 -> 16 form of cabinet_conv3x3s2_wgrad, by measurement on MI355X (tools/time_conv3x3s2.py,
    profiles/conv3x3s2_summary.md): native where its one workgroup per four output rows fills the chip (>= 1024 of them: x1.5 at
    config 3; with the 512 of config 5 it only draws level with the stock call).  False for every other channel count: the
    64 -> 64 form has a rule of its own, _conv3x3s2_native_wgrad64."""
    return Ci == 3 and B * (((H - 1) // 2 + 1 + 3) // 4) >= 1024


# CABINET_CONV3X3S2_WGRAD64=0: the 64 -> 64 weight gradient alone goes back to the stock operator -- same-box A/B timing only
CONV3X3S2_WGRAD64_ENABLED = _os.environ.get("CABINET_CONV3X3S2_WGRAD64", "1") != "0"
_CW_MIN_WORKGROUPS = 256  # one per CU
_CW_MIN_ROWS = 4          # output rows a workgroup walks per 147 KB slab it writes: a full strip of cw_plan


def _conv3x3s2_wgrad64_plan(B, H, W):
    """cw_plan of csrc/conv3x3_s2.hip restated -> (workgroups, rows_per): 32-column tiles, strips of output rows."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tiles = -(-Wo // 32)
    strips = max(1, min(512 // (B * tiles), -(-Ho // 4)))
    rows_per = -(-Ho // strips)
    return B * tiles * -(-Ho // rows_per), rows_per


def _conv3x3s2_native_wgrad64(B, H, W):
    """The routing rule of the 64 -> 64 form of cabinet_conv3x3s2_wgrad, by measurement on MI355X
    (tools/time_conv3x3s2_wgrad64.py, profiles/conv3x3s2_wgrad64_summary.md): native where the plan gives every CU a workgroup
    and every workgroup a full strip of rows to pipeline over, which is where it was measured against the stock call with its
    layout copies (sb.conv2 and sb.conv3 at config 3 and 5: 512 workgroups of 32, 8, 16 and 4 rows).  Smaller planes were not
    measured and keep the stock operator."""
    if not CONV3X3S2_WGRAD64_ENABLED:
        return False
    workgroups, rows_per = _conv3x3s2_wgrad64_plan(B, H, W)
    return workgroups >= _CW_MIN_WORKGROUPS and rows_per >= _CW_MIN_ROWS


# CABINET_CONV3X3S2_FWD64=0: the 64 -> 64 forward alone goes back to the stock operator (MIOpen's NHWC implicit GEMM with its
# NCHW <-> NHWC copies) -- same-box A/B timing only
CONV3X3S2_FWD64_ENABLED = _os.environ.get("CABINET_CONV3X3S2_FWD64", "1") != "0"
_CV_TILE = 32             # output columns of a workgroup's tile (CV_TW of csrc/conv3x3_s2.hip)
_CV_MIN_WORKGROUPS = 256  # one per CU
_CV_MIN_ROWS = 2          # output rows a workgroup walks: the shortest strip measured (the ring's hand-over runs at least once)


def _conv3x3s2_fwd64_plan(B, H, W):
    """cv_plan of csrc/conv3x3_s2.hip restated -> (workgroups, rows_per): 32-column tiles, strips of output rows, 512 workgroups
    aimed at."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tiles = -(-Wo // _CV_TILE)
    strips = max(1, min(512 // (B * tiles), Ho))
    rows_per = -(-Ho // strips)
    return B * tiles * -(-Ho // rows_per), rows_per


def _conv3x3s2_native_fwd64(B, H, W):
    """The routing rule of cabinet_conv3x3s2_fwd, by measurement on MI355X (tools/time_conv3x3s2_fwd64.py,
    profiles/conv3x3s2_fwd64_summary.md): native where the plan gives every CU a workgroup and every workgroup a strip of at
    least two rows, which is where it was measured against the stock call with its layout copies (sb.conv2 and sb.conv3 at
    config 3 and 5 and of one 1024 x 2048 image: 512 workgroups of 32, 8, 16, 4, 8 and 2 rows).  Planes whose workgroups get a
    single row each were not measured and keep the stock operator."""
    if not CONV3X3S2_FWD64_ENABLED:
        return False
    workgroups, rows_per = _conv3x3s2_fwd64_plan(B, H, W)
    return workgroups >= _CV_MIN_WORKGROUPS and rows_per >= _CV_MIN_ROWS


def conv3x3s2_fwd64(x, weight):
    """y = conv2d(x, weight, stride 2, padding 1) of a 64 -> 64 layer by cabinet_conv3x3s2_fwd: dense fp32 NCHW device tensors,
    no autograd, no workspace; capturable.  Whatever the routing rule says: the callers ask it."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and weight.dtype == torch.float32
            and tuple(weight.shape) == (64, 64, 3, 3) and x.shape[1] == 64):
        raise RuntimeError("conv3x3s2_fwd64: fp32 device tensors, x (B, 64, H, W), weight (64, 64, 3, 3)")
    xc, wc = _f32c(x.detach()), _f32c(weight.detach())
    B, H, W = xc.shape[0], xc.shape[2], xc.shape[3]
    y = torch.empty((B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().cabinet_conv3x3s2_fwd(_ptr(xc), _ptr(wc), B, 64, 64, H, W, _ptr(y), _stream_handle(x.device))
    _lib.check(rc, "cabinet_conv3x3s2_fwd")
    return y


def _conv3x3s2_fwd64_nograd(conv, x, weight):
    """True where Conv2dS2 takes the native forward outside autograd (evaluation, inference): a bias-free 3x3 stride-2 padding-1
    64 -> 64 layer, dense-able fp32 device input, no graph being recorded, outside autocast, and the routing rule holds."""
    if not (CONV3X3S2_ENABLED and x.is_cuda and x.dim() == 4 and x.shape[0] >= 1 and x.shape[2] * x.shape[3] >= 1):
        return False
    if not (conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.dilation == (1, 1) and conv.padding_mode == "zeros"
            and conv.in_channels == 64 and conv.out_channels == 64 and x.shape[1] == 64):
        return False
    if torch.is_autocast_enabled() or x.dtype != torch.float32 or weight.dtype != torch.float32 or not weight.is_cuda:
        return False
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return False
    if not _conv3x3s2_native_fwd64(x.shape[0], x.shape[2], x.shape[3]):
        return False
    return bool(_lib.load().cabinet_conv3x3s2_fwd_supported(64, 64))


class _Conv3x3S2(torch.autograd.Function):
    """y = conv2d(x, weight, stride 2, padding 1): the forward of the 64 -> 64 layers by cabinet_conv3x3s2_fwd where
    _conv3x3s2_native_fwd64 says so, else (and for the 3 -> 16 layer always) the stock forward; dx of the 64 -> 64 layers by
    cabinet_conv3x3s2_dgrad (the 3 -> 16 layer reads the image and has none), dw by cabinet_conv3x3s2_wgrad where the form's
    rule says so (_conv3x3s2_native_wgrad64 for 64 -> 64, _conv3x3s2_native_wgrad for 3 -> 16), else by the stock operator.
    What is saved and the backward do not depend on which forward ran."""

    @staticmethod
    def forward(fn_ctx, x, weight):
        x = x.contiguous()  # dense NCHW for the stock operator too (a no-op in the model): a channels_last input sends it to another solver
        if weight.shape[0] == 64 and weight.shape[1] == 64 and _conv3x3s2_native_fwd64(x.shape[0], x.shape[2], x.shape[3]):
            y = conv3x3s2_fwd64(x, weight)
        else:
            y = F.conv2d(x, weight, None, 2, 1)
        fn_ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(fn_ctx, g):
        x, w = fn_ctx.saved_tensors
        g = g.contiguous()
        lib = _lib.load()
        xc, gc = _f32c(x), _f32c(g)
        Co, Ci = w.shape[0], w.shape[1]
        B, H, W = xc.shape[0], xc.shape[2], xc.shape[3]
        cb = torch.ops.aten.convolution_backward
        dx = None
        if fn_ctx.needs_input_grad[0] and Ci == 64:
            dx = torch.empty_like(xc)
            with torch.cuda.device(x.device):
                rc = lib.cabinet_conv3x3s2_dgrad(_ptr(gc), _ptr(_f32c(w)), B, Ci, Co, H, W, _ptr(dx), _stream_handle(x.device))
            _lib.check(rc, "cabinet_conv3x3s2_dgrad")
        elif fn_ctx.needs_input_grad[0]:
            dx = cb(g, x, w, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])[0]
        dw = None
        native_dw = _conv3x3s2_native_wgrad64(B, H, W) if Ci == 64 else _conv3x3s2_native_wgrad(Ci, B, H)
        if fn_ctx.needs_input_grad[1] and native_dw:
            dw = torch.empty((Co, Ci, 3, 3), dtype=torch.float32, device=x.device)
            ws, nbytes = _workspace(lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, Ci, Co, H, W), x.device)
            with torch.cuda.device(x.device):
                rc = lib.cabinet_conv3x3s2_wgrad(_ptr(gc), _ptr(xc), B, Ci, Co, H, W, _ptr(dw), _ptr(ws), nbytes,
                                                 _stream_handle(x.device))
            _lib.check(rc, "cabinet_conv3x3s2_wgrad")
        elif fn_ctx.needs_input_grad[1]:
            dw = cb(g, x, w, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        return dx, dw


class Conv2dS2(torch.nn.Conv2d):
    """``nn.Conv2d`` (same parameters, same ``state_dict``) whose convolution is ``_Conv3x3S2`` where conv3x3s2_supported says
    so (a forward that records a graph), cabinet_conv3x3s2_fwd called directly where _conv3x3s2_fwd64_nograd says so (the
    64 -> 64 layers in evaluation and inference) and the stock operator everywhere else.  The route sits inside the module's
    own call, so forward hooks and pre-hooks registered on the layer see it as they see any convolution.  The models build
    their stride-2 3x3 layers with it."""

    def _conv_forward(self, input, weight, bias):
        if bias is None and conv3x3s2_supported(self, input):
            return _Conv3x3S2.apply(input, weight)
        if bias is None and _conv3x3s2_fwd64_nograd(self, input, weight):
            return conv3x3s2_fwd64(input, weight)
        return super()._conv_forward(input, weight, bias)


# --------------------------------------------------------------------------- evaluation tail (K13; no autograd)


def eval_chip_accum_supported(logits, chip_size, flip=False):
    """True when the fused softmax + window accumulation takes these chip logits: a device tensor, at most 32 classes, and the
    source rows of one segment of chip pixels fit the LDS (every model-resolution-to-chip ratio <= 1 does)."""
    if not (logits.is_cuda and logits.dim() == 4 and _lib.available()):
        return False
    _, C, hl, wl = logits.shape
    return bool(_lib.load().cabinet_eval_chip_accum_supported(C, hl, wl, int(chip_size[0]), int(chip_size[1]), int(bool(flip))))


def eval_chip_accum(dst, logits, logits_flipped, chip_size, origin, rcp_y=None, rcp_x=None):
    """dst[:, :, y0:y0+ch, x0:x0+cw] += rcp_y (x) rcp_x * mean over {chip, flipped chip} of softmax(upsample(logits -> chip_size))
    -- reference evaluate.py:75-87 with the model's final upsample, and :133-137.  ``logits_flipped`` (or None) holds the logits
    of the horizontally flipped chip; ``rcp_y`` (FH) / ``rcp_x`` (FW) the reciprocal window counts per row / column of ``dst``
    (None: ones).  In place on ``dst`` (N, C, FH, FW), which must be dense fp32."""
    lib = _lib.load()
    if not (dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous()):
        raise RuntimeError("eval_chip_accum: dst must be a dense fp32 device tensor")
    a = _f32c(logits)
    b = _f32c(logits_flipped) if logits_flipped is not None else None
    if b is not None and b.shape != a.shape:
        raise RuntimeError("eval_chip_accum: the flipped chip's logits must have the shape of the chip's")
    N, C, hl, wl = a.shape
    if dst.shape[:2] != (N, C):
        raise RuntimeError(f"eval_chip_accum: dst {tuple(dst.shape)} does not match logits {tuple(a.shape)}")
    FH, FW = dst.shape[2:]
    ry = _f32c(rcp_y) if rcp_y is not None else None
    rx = _f32c(rcp_x) if rcp_x is not None else None
    if (ry is not None and ry.numel() != FH) or (rx is not None and rx.numel() != FW):
        raise RuntimeError("eval_chip_accum: rcp_y / rcp_x must have one entry per row / column of dst")
    dev = dst.device
    with torch.cuda.device(dev):
        rc = lib.cabinet_eval_chip_accum(_ptr(a), _ptr(b), N, C, hl, wl, int(chip_size[0]), int(chip_size[1]), _ptr(dst), FH, FW,
                                         int(origin[0]), int(origin[1]), _ptr(ry), _ptr(rx), _stream_handle(dev))
    _lib.check(rc, "cabinet_eval_chip_accum")
    return dst


def eval_scale_merge_supported(total):
    return bool(total.is_cuda and total.dim() == 4 and _lib.available() and total.shape[0] * total.shape[1] <= 65535
                and total.shape[2] <= 65535)


def eval_scale_merge(total, prob, crop=None):
    """total += F.interpolate(prob[:, :, hst:hed, wst:wed], total.shape[2:], mode="bilinear", align_corners=False) in one pass
    (reference evaluate.py:140-142, :156-158, :217).  ``crop`` = (hst, hed, wst, wed), None: all of ``prob``.  In place."""
    lib = _lib.load()
    if not (total.is_cuda and total.dtype == torch.float32 and total.is_contiguous()):
        raise RuntimeError("eval_scale_merge: total must be a dense fp32 device tensor")
    prob = _f32c(prob)
    N, C, H, W = total.shape
    if prob.shape[:2] != (N, C):
        raise RuntimeError(f"eval_scale_merge: prob {tuple(prob.shape)} does not match total {tuple(total.shape)}")
    FH, FW = prob.shape[2:]
    hst, hed, wst, wed = crop if crop is not None else (0, FH, 0, FW)
    dev = total.device
    with torch.cuda.device(dev):
        rc = lib.cabinet_eval_scale_merge(_ptr(prob), N, C, FH, FW, int(hst), int(hed), int(wst), int(wed), _ptr(total), H, W,
                                          _stream_handle(dev))
    _lib.check(rc, "cabinet_eval_scale_merge")
    return total


def eval_argmax_hist_supported(total):
    return bool(total.is_cuda and total.dim() == 4 and _lib.available() and total.shape[1] <= 32)


def eval_argmax_hist(total, labels, hist, ignore_label, want_pred=False):
    """hist[argmax_c total, clip(label)] += 1 over the pixels whose label != ignore_label (reference evaluate.py:218-224 with
    compute_hist, :161-191).  ``labels`` (N, H, W) int64 on the device; ``hist`` (C, C) int64 on the device, updated in place
    with integer atomics.  Returns the (N, H, W) uint8 predictions when ``want_pred``."""
    lib = _lib.load()
    if not (total.is_cuda and total.dtype == torch.float32 and total.is_contiguous()):
        raise RuntimeError("eval_argmax_hist: total must be a dense fp32 device tensor")
    N, C, H, W = total.shape
    if labels.dtype != torch.int64 or tuple(labels.shape) != (N, H, W) or labels.device != total.device:
        raise RuntimeError("eval_argmax_hist: labels must be (N, H, W) int64 on total's device")
    if hist.dtype != torch.int64 or tuple(hist.shape) != (C, C) or not hist.is_contiguous() or hist.device != total.device:
        raise RuntimeError("eval_argmax_hist: hist must be a dense (C, C) int64 tensor on total's device")
    labels = _aligned(labels)
    pred = torch.empty((N, H, W), dtype=torch.uint8, device=total.device) if want_pred else None
    dev = total.device
    with torch.cuda.device(dev):
        rc = lib.cabinet_eval_argmax_hist(_ptr(total), _ptr(labels), N, C, H, W, int(ignore_label), _ptr(hist), _ptr(pred),
                                          _stream_handle(dev))
    _lib.check(rc, "cabinet_eval_argmax_hist")
    return pred


# --------------------------------------------------------------------------- inference tail (K17; no autograd)


def _u8_out(out, shape, device, what):
    """The uint8 output of a K17 kernel: a fresh tensor, or the caller's (any byte offset into its storage; dense)."""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if not (out.dtype == torch.uint8 and out.device == device and tuple(out.shape) == tuple(shape) and out.is_contiguous()):
        raise RuntimeError(f"{what}: out must be a dense uint8 tensor of shape {tuple(shape)} on the input's device")
    return out


def predict_up_argmax_supported(logits, size):
    """True when ``predict_up_argmax`` takes these low-resolution logits: a device tensor, at most 32 classes, and the source
    rows of one row segment fit the LDS (every model-resolution-to-image ratio <= 1 does)."""
    if not (logits.is_cuda and logits.dim() == 4 and _lib.available()):
        return False
    N, C, hl, wl = logits.shape
    return bool(N <= 65535 and _lib.load().cabinet_predict_up_argmax_supported(C, hl, wl, int(size[0]), int(size[1])))


def predict_up_argmax(logits, size, out=None):
    """(N, H, W) uint8 argmax over classes of F.interpolate(logits, size, mode="bilinear", align_corners=False) -- reference
    visualize.py:113-114 and :139 with the model's final upsample (cabinet.py:240-245) for ``scales=[1.0]``, ``flip=False``:
    softmax does not move the argmax, and the full-resolution class tensor is never built.  Lowest index on equal values."""
    lib = _lib.load()
    if not (logits.is_cuda and logits.dim() == 4):
        raise RuntimeError("predict_up_argmax: logits must be a (N, C, h, w) device tensor")
    a = _f32c(logits)
    N, C, hl, wl = a.shape
    H, W = int(size[0]), int(size[1])
    labels = _u8_out(out, (N, H, W), a.device, "predict_up_argmax")
    dev = a.device
    with torch.cuda.device(dev):
        rc = lib.cabinet_predict_up_argmax(_ptr(a), N, C, hl, wl, H, W, _ptr(labels), _stream_handle(dev))
    _lib.check(rc, "cabinet_predict_up_argmax")
    return labels


def predict_argmax_supported(total):
    return bool(total.is_cuda and total.dim() == 4 and _lib.available() and total.shape[1] <= 32 and total.shape[0] <= 65535)


def predict_argmax(total, out=None):
    """(N, H, W) uint8 ``torch.argmax(total, 1)`` of a (N, C, H, W) fp32 device tensor (reference visualize.py:139 on the
    multi-scale / flip path), lowest index on equal values."""
    lib = _lib.load()
    if not (total.is_cuda and total.dim() == 4):
        raise RuntimeError("predict_argmax: total must be a (N, C, H, W) device tensor")
    t = _f32c(total)
    N, C, H, W = t.shape
    labels = _u8_out(out, (N, H, W), t.device, "predict_argmax")
    dev = t.device
    with torch.cuda.device(dev):
        rc = lib.cabinet_predict_argmax(_ptr(t), N, C, H, W, _ptr(labels), _stream_handle(dev))
    _lib.check(rc, "cabinet_predict_argmax")
    return labels


def predict_render(labels, image, palette, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), alpha=0.6,
                   want_input=True, want_overlay=True, out=None):
    """The reference's colouring and blending (visualize.py:50-61, :165-177) on the device, byte for byte.

    ``labels`` (N, H, W) uint8, ``image`` (N, 3, H, W) normalised fp32 or None, ``palette`` (n_colors, 3) uint8 on the device.
    Returns a dict of (N, H, W, 3) uint8 tensors: ``pred`` = palette[min(label, n_colors - 1)] always; with an image ``input`` =
    uint8(clip(image * std + mean, 0, 1) * 255) and ``overlay`` = Image.blend(input, pred, alpha), each unless switched off.
    ``out`` may name caller-owned tensors under the same keys."""
    lib = _lib.load()
    if not (labels.is_cuda and labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous()):
        raise RuntimeError("predict_render: labels must be a dense (N, H, W) uint8 device tensor")
    N, H, W = labels.shape
    dev = labels.device
    if not (palette.dtype == torch.uint8 and palette.dim() == 2 and palette.shape[1] == 3 and palette.device == dev
            and 1 <= palette.shape[0] <= 256):
        raise RuntimeError("predict_render: palette must be a (n_colors <= 256, 3) uint8 tensor on labels' device")
    palette = palette.contiguous()
    img = None
    if image is not None:
        if tuple(image.shape) != (N, 3, H, W) or image.device != dev:
            raise RuntimeError(f"predict_render: image {tuple(image.shape)} does not match labels {tuple(labels.shape)}")
        img = _f32c(image)
    want_input, want_overlay = bool(want_input and img is not None), bool(want_overlay and img is not None)
    out = out or {}
    res = {"pred": _u8_out(out.get("pred"), (N, H, W, 3), dev, "predict_render")}
    if want_input:
        res["input"] = _u8_out(out.get("input"), (N, H, W, 3), dev, "predict_render")
    if want_overlay:
        res["overlay"] = _u8_out(out.get("overlay"), (N, H, W, 3), dev, "predict_render")
    m3, s3 = (_ct.c_float * 3)(*[float(v) for v in mean]), (_ct.c_float * 3)(*[float(v) for v in std])
    with torch.cuda.device(dev):
        rc = lib.cabinet_predict_render(_ptr(labels), _ptr(img if (want_input or want_overlay) else None), _ptr(palette),
                                        int(palette.shape[0]), _ct.addressof(m3), _ct.addressof(s3), float(alpha), N, H, W,
                                        _ptr(res["pred"]), _ptr(res.get("input")), _ptr(res.get("overlay")), _stream_handle(dev))
    _lib.check(rc, "cabinet_predict_render")
    return res
