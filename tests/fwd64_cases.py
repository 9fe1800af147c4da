"""Shapes, seeded inputs and the launch plan of the 64 -> 64 forward of the 3x3 stride-2 convolutions (K15,
conv3x3s2_fwd64_kernel in csrc/conv3x3_s2.hip), shared by tests/test_gpu_conv3x3s2_fwd64.py and tools/time_conv3x3s2_fwd64.py."""
import hashlib

import torch

T = 32           # output columns of a workgroup's tile (CV_TW)
TARGET_WG = 512  # workgroups the plan aims at (CV_TARGET_WG)

# (B, H, W) of x -> (tiles, strips, rows_per) of cv_plan.  A workgroup walks rows_per output rows of one T-column tile.
PLANS = {
    (260, 6, 8): (1, 1, 3),            # one strip per image (B x tiles > TARGET_WG / 2): the ring's hand-over runs twice
    (2, 9, 11): (1, 5, 1),             # several strips of one row: every workgroup is a first step without prefetch
    (40, 30, 8): (1, 8, 2),            # B x tiles x Ho = 600 > TARGET_WG: rows_per 2, and a last strip of one row
    (4, 300, 2 * T): (1, 75, 2),       # the same branch at a full tile: Wo = T, the right halo inside x, the left outside
    (1, 5, 4 * T + 2): (3, 3, 1),      # Wo = 2 T + 1: three column tiles, the last one column wide
    (130, 14, 70): (2, 1, 7),          # two tiles, the second 3 wide; one strip of 7 rows: the ring wraps twice
    (3, 41, 2 * T + 7): (2, 21, 1),    # odd H and W, B > 1 image bases, a ragged second tile
    (70, 27, 2 * T + 1): (2, 3, 5),    # strips of 5, 5 and 4 rows over two tiles
}
SHAPES = list(PLANS)

# the edge sweep: every (B, H, W) of the product
EDGE_B = (1, 3)
EDGE_H = (1, 2, 3, 4, 5, 9)
EDGE_W = (1, 2, 3, 2 * T - 2, 2 * T - 1, 2 * T, 2 * T + 1, 4 * T + 1)

# operator-alone timing (tools/time_conv3x3s2_fwd64.py): sb.conv2 / sb.conv3 at config 3, at config 5, of one 1024 x 2048 image
BENCH_SHAPES = {
    "sb.conv2 config 3": (8, 512, 512), "sb.conv3 config 3": (8, 256, 256),
    "sb.conv2 config 5": (2, 1024, 512), "sb.conv3 config 5": (2, 512, 256),
    "sb.conv2 1x1024x2048": (1, 512, 1024), "sb.conv3 1x1024x2048": (1, 256, 512),
}
# shapes existing tests pin to the stock forward bit for bit: (2, 64, 32, 32) and (2, 64, 16, 16) are sb.conv2 / sb.conv3 of a
# 2 x 3 x 64 x 64 image
STOCK_SHAPES = [(2, 24, 21), (2, 6, 10), (2, 32, 32), (2, 16, 16), (2, 33, 21)]


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def plan(B, H, W):
    """cv_plan of conv3x3_s2.hip restated -> (tiles, strips, rows_per); the kernel runs B * tiles * strips workgroups."""
    Ho, Wo = out_hw(H, W)
    tiles = -(-Wo // T)
    strips = max(1, min(TARGET_WG // (B * tiles), Ho))
    rows_per = -(-Ho // strips)
    return tiles, -(-Ho // rows_per), rows_per


def _gen(shape):
    return torch.Generator().manual_seed(int(hashlib.sha256(f"fwd64/{shape}".encode()).hexdigest()[:8], 16))


def inputs(B, H, W):
    """-> x [B, 64, H, W], w [64, 64, 3, 3] (CPU, seeded); w at the scale of a trained layer."""
    g = _gen((B, H, W))
    return torch.randn(B, 64, H, W, generator=g), torch.randn(64, 64, 3, 3, generator=g) * 0.05


def run_fwd(x, w, y=None):
    """cabinet_conv3x3s2_fwd on device tensors, whatever the routing rule says; y [B, 64, Ho, Wo] is written in place (allocated
    NaN-filled when not given) and returned."""
    from cabinet_amd import _lib
    from cabinet_amd.functional import _ptr, _stream_handle

    lib = _lib.load()
    B, _, H, W = x.shape
    if y is None:
        y = torch.full((B, 64) + out_hw(H, W), float("nan"), device=x.device)
    assert tuple(x.shape) == (B, 64, H, W) and tuple(w.shape) == (64, 64, 3, 3) and tuple(y.shape) == (B, 64) + out_hw(H, W)
    assert x.is_contiguous() and w.is_contiguous() and y.is_contiguous()
    rc = lib.cabinet_conv3x3s2_fwd(_ptr(x), _ptr(w), B, 64, 64, H, W, _ptr(y), _stream_handle(x.device))
    if rc != 0:
        raise RuntimeError(f"cabinet_conv3x3s2_fwd: rc {rc}: {lib.cabinet_last_error().decode()}")
    return y
