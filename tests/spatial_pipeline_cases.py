"""Shapes, seeded inputs and the launch plans of the pipelined stem forward (K9, csrc/stem_conv.hip) and 3x3 stride-2 input
gradient (K15, csrc/conv3x3_s2.hip), shared by tests/test_gpu_spatial_pipeline.py and
tests/golden/make_golden_spatial_pipeline.py (the generator runs on the library of the commit BEFORE the pipelined staging and
records what that commit computes)."""
import ctypes
import hashlib
import os

import torch

# ---- stem forward: (B, H, W).  Tile 8 x 32 outputs; a workgroup walks the tiles of one 8-row strip, left to right.
STEM = [
    (1, 15, 37),     # Ho 8, Wo 19: one tile, no prefetch at all
    (1, 16, 128),    # Wo 64: exactly two tiles: one prefetch
    (3, 29, 255),    # odd H and W; Ho 15 (Ho % 8 = 7); Wo 128: four tiles
    (3, 13, 190),    # Ho 7; Wo 95 (Wo % 32 = 31): three tiles, the middle one is prefetched into and from
    (1, 17, 449),    # Ho 9 (Ho % 8 = 1); Wo 225 (Wo % 32 = 1): eight tiles, the last one column wide
    (1, 33, 322),    # Wo 161: six tiles, three strips, the last a single row
    (64, 121, 131),  # 512 workgroups (two on every CU) of three tiles (Wo 66), the last two columns wide; Ho 61
]

# ---- input gradient: (B, H, W).  A workgroup walks rows_per row pairs of one 64-column tile of dy (cd_plan).
DGRAD = [
    (1, 1, 5),       # Ho 1, Wo 3: one step; odd H and W (unpaired stores); the halo column lies outside dy
    (1, 6, 128),     # Wo 64 (Wo % 64 = 0): one full tile, halo column outside; rows_per 1
    (3, 9, 129),     # Wo 65 (Wo % 64 = 1): the halo column of tile 0 is inside dy, tile 1 is one column wide; odd H, odd W; B 3
    (1, 8, 254),     # Wo 127 (Wo % 64 = 63)
    (3, 400, 16),    # Ho 200 in 100 strips: rows_per 2
    (3, 1025, 6),    # Ho 513 in 129 strips: rows_per 4, the last strip a single row: the ring wraps; odd H
    (8, 200, 130),   # Wo 65, two tiles; Ho 100 in 25 strips: rows_per 4 with the halo column inside dy
]

SAMPLE = 4096  # elements of an output kept in the fixture (a strided sample), beside the SHA-256 of all of it


def stem_out(B, H, W):
    return (B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


def stem_plan(B, H, W):
    """stem_conv_fwd_run restated -> (workgroups, tiles walked by each)."""
    _, _, Ho, Wo = stem_out(B, H, W)
    return B * -(-Ho // 8), -(-Wo // 32)


def dgrad_plan(B, H, W):
    """cd_plan of conv3x3_s2.hip restated -> (tiles, strips, rows_per); cabinet_conv3x3s2_dgrad_workgroups is B * tiles * strips."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tiles = -(-Wo // 64)
    strips = max(1, min(512 // (B * tiles), Ho))
    rows_per = -(-Ho // strips)
    return tiles, -(-Ho // rows_per), rows_per


def _gen(tag, shape):
    return torch.Generator().manual_seed(int(hashlib.sha256(f"{tag}/{shape}".encode()).hexdigest()[:8], 16))


def stem_inputs(B, H, W):
    """-> x [B, 3, H, W], w [64, 3, 7, 7] (CPU, seeded)."""
    g = _gen("stem", (B, H, W))
    return torch.randn(B, 3, H, W, generator=g), torch.randn(64, 3, 7, 7, generator=g) * 0.1


def dgrad_inputs(B, H, W):
    """-> dy [B, 64, Ho, Wo], w [64, 64, 3, 3] (CPU, seeded)."""
    g = _gen("dgrad", (B, H, W))
    return torch.randn(B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g), torch.randn(64, 64, 3, 3, generator=g) * 0.05


def load_library(path=None):
    """The package's library, or another build of it (the parent commit's) with the same signatures."""
    from cabinet_amd import _lib

    this = _lib.load()
    if path is None:
        return this
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("cabinet_stem_conv_fwd", "cabinet_conv3x3s2_dgrad", "cabinet_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def _check(lib, rc, who):
    if rc != 0:
        raise RuntimeError(f"{who}: rc {rc}: {lib.cabinet_last_error().decode()}")


def run_stem(lib, x, w, y):
    """cabinet_stem_conv_fwd on device tensors; y is written in place and returned."""
    from cabinet_amd.functional import _ptr, _stream_handle

    B, _, H, W = x.shape
    assert tuple(y.shape) == stem_out(B, H, W) and x.is_contiguous() and w.is_contiguous() and y.is_contiguous()
    _check(lib, lib.cabinet_stem_conv_fwd(_ptr(x), _ptr(w), B, H, W, _ptr(y), _stream_handle(x.device)), "cabinet_stem_conv_fwd")
    return y


def run_dgrad(lib, dy, w, dx):
    """cabinet_conv3x3s2_dgrad on device tensors; dx [B, 64, H, W] is written in place and returned."""
    from cabinet_amd.functional import _ptr, _stream_handle

    B, _, H, W = dx.shape
    assert tuple(dy.shape) == (B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert dy.is_contiguous() and w.is_contiguous() and dx.is_contiguous()
    _check(lib, lib.cabinet_conv3x3s2_dgrad(_ptr(dy), _ptr(w), B, 64, 64, H, W, _ptr(dx), _stream_handle(dy.device)),
           "cabinet_conv3x3s2_dgrad")
    return dx


def key(kind, shape):
    return f"{kind}/" + "x".join(map(str, shape))


def digest(t):
    """SHA-256 over the bytes of a tensor: equal digests <=> torch.equal up to NaN payloads, which the tests exclude."""
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def sample(t):
    """A fixed strided sample of at most SAMPLE elements (an odd stride, so that it walks through columns, rows and channels)."""
    flat = t.detach().cpu().contiguous().view(-1)
    stride = max(1, flat.numel() // SAMPLE) | 1
    return flat[::stride][:SAMPLE].clone()
