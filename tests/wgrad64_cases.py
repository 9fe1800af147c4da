"""Shapes, seeded inputs and the launch plan of the 64 -> 64 weight gradient of the 3x3 stride-2 convolutions (K15,
conv3x3s2_wgrad64_kernel in csrc/conv3x3_s2.hip), shared by tests/test_gpu_conv3x3s2_wgrad64.py and
tests/golden/make_golden_wgrad64.py (the generator runs on the library of the commit BEFORE the pipelined staging and records
what that commit computes)."""
import ctypes
import hashlib
import os

import torch

# (B, H, W) of x -> (tiles, strips, rows_per) of cw_plan.  A workgroup walks rows_per output rows of one 32-column tile.
PLANS = {
    (1, 1, 1): (1, 1, 1),       # one workgroup, one step: iy = -1, iy = H, ix = -1, ix = W and ox >= Wo at once; no prefetch
    (1, 4, 8): (1, 1, 2),       # the shortest ring hand-over
    (2, 9, 11): (1, 2, 3),      # strips of 3 and 2 rows: odd H (row iy = H is zero), odd W, a second strip that starts at oy > 0
    (1, 7, 64): (1, 1, 4),      # Wo = 32 exactly: the right halo column is inside x, the left one outside
    (1, 16, 70): (2, 2, 4),     # Wo 35: two tiles, the second 3 wide: clamped dy and x columns
    (1, 5, 130): (3, 1, 3),     # Wo 65: three tiles, the last one column wide
    (1, 1025, 6): (1, 129, 4),  # 129 strips of 4 rows, the last a single row: a strip without prefetch behind strips with it
    (3, 400, 16): (1, 50, 4),   # B > 1 image bases
    (260, 18, 8): (1, 1, 9),    # one strip of 9 rows: the ring wraps three times in one workgroup
    (130, 14, 70): (2, 1, 7),   # wrap with a ragged tile
}
SHAPES = list(PLANS)

SAMPLE = 1024  # elements of dW (36864) kept in the fixture, beside the SHA-256 of all of it


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def plan(B, H, W):
    """cw_plan of conv3x3_s2.hip restated -> (tiles, strips, rows_per); the kernel runs B * tiles * strips workgroups."""
    Ho, Wo = out_hw(H, W)
    tiles = -(-Wo // 32)
    strips = max(1, min(512 // (B * tiles), -(-Ho // 4)))
    rows_per = -(-Ho // strips)
    return tiles, -(-Ho // rows_per), rows_per


def _gen(shape):
    return torch.Generator().manual_seed(int(hashlib.sha256(f"wgrad64/{shape}".encode()).hexdigest()[:8], 16))


def inputs(B, H, W):
    """-> x [B, 64, H, W], dy [B, 64, Ho, Wo] (CPU, seeded)."""
    g = _gen((B, H, W))
    return torch.randn(B, 64, H, W, generator=g), torch.randn(B, 64, *out_hw(H, W), generator=g)


def load_library(path=None):
    """The package's library, or another build of it (the parent commit's) with the same signatures."""
    from cabinet_amd import _lib

    this = _lib.load()
    if path is None:
        return this
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("cabinet_conv3x3s2_wgrad", "cabinet_conv3x3s2_wgrad_workspace_bytes", "cabinet_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def run_wgrad(lib, dy, x, dw):
    """cabinet_conv3x3s2_wgrad on device tensors; dw [64, 64, 3, 3] is written in place and returned."""
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    B, _, H, W = x.shape
    assert tuple(dy.shape) == (B, 64) + out_hw(H, W) and tuple(dw.shape) == (64, 64, 3, 3)
    assert dy.is_contiguous() and x.is_contiguous() and dw.is_contiguous()
    ws, nbytes = _workspace(lib.cabinet_conv3x3s2_wgrad_workspace_bytes(B, 64, 64, H, W), x.device)
    rc = lib.cabinet_conv3x3s2_wgrad(_ptr(dy), _ptr(x), B, 64, 64, H, W, _ptr(dw), _ptr(ws), nbytes, _stream_handle(x.device))
    if rc != 0:
        raise RuntimeError(f"cabinet_conv3x3s2_wgrad: rc {rc}: {lib.cabinet_last_error().decode()}")
    return dw


def key(shape):
    return "wgrad64/" + "x".join(map(str, shape))


def digest(t):
    """SHA-256 over the bytes of a tensor: equal digests <=> torch.equal up to NaN payloads, which the tests exclude."""
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def sample(t):
    """A fixed strided sample of at most SAMPLE elements (an odd stride: it walks through taps, ci and co)."""
    flat = t.detach().cpu().contiguous().view(-1)
    stride = max(1, flat.numel() // SAMPLE) | 1
    return flat[::stride][:SAMPLE].clone()
