"""Shapes, inputs and the launch plan of the strip-walking depthwise kernels (K8, csrc/dwconv.hip), shared by
tests/test_gpu_dwconv_strips.py and tests/golden/make_golden_dwconv_strips.py (the generator runs on the commit BEFORE the
strip kernels and records what that commit computes)."""
import hashlib

import torch

KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
FUSED = [("relu", True), ("relu", False), ("hardswish", True), ("hardswish", False)]
MIN_WG, MIN_BLOCKS = 4096, 4   # DW_MIN_WG, DW_MIN_BLOCKS of dwconv.hip


def strip_plan(planes, hp, wp):
    """dw_plan of dwconv.hip restated (it has no entry point to query): the tile of a (hp, wp) plane -- the INPUT plane for the
    backward kernels, the OUTPUT plane for the forward ones -- is TH x TW = 1024 pixels; a workgroup walks `nb` vertically
    adjacent tiles (blocks) of one strip: at least MIN_BLOCKS where the plane has them, more while MIN_WG workgroups remain.
    -> dict(TW, TH, strips, blocks, nb, runs, last) with last = blocks of the last run."""
    tw = 64 if wp > 32 else 32 if wp > 16 else 16 if wp > 8 else 8
    th = 1024 // tw
    strips, blocks = -(-wp // tw), -(-hp // th)
    nb = min(blocks, max(MIN_BLOCKS, planes * strips * blocks // MIN_WG))
    runs = -(-blocks // nb)
    nb = -(-blocks // runs)
    runs = -(-blocks // nb)
    return dict(TW=tw, TH=th, strips=strips, blocks=blocks, nb=nb, runs=runs, last=blocks - (runs - 1) * nb)


# (B, C, H, W) and the branch of the plan (input-space, i.e. the backward kernels and the stride-1 forward) the row is there for
SHAPES = [
    (2, 3, 70, 130),   # 3 strips (the last 2 columns wide) x 2 runs of 3 + 2 blocks: several partials per channel; W % 4 = 2: ragged form
    (1, 2, 41, 67),    # odd H and W (stride 2: odd quads at both borders); one run of 3 blocks: the halo is carried twice
    (2, 2, 5, 200),    # H < one block: 4 strips of a single short block; W % 4 = 0: 16-byte form
    (1, 2, 200, 5),    # W below the narrowest tile (TW = 8, TH = 128): 2 blocks of 128 rows, halo columns in both staging slots
    (1, 5, 1, 1),      # one pixel: every tap but the centre falls into the padding
    (1, 4, 128, 128),  # 16-byte form over 2 strips x 2 runs of 4 blocks: the prefetch wraps the double buffer twice
    (1, 2, 330, 36),   # 21 blocks in runs of 4: 6 runs, the last a single block; a strip 36 of 64 columns wide, 16-byte form
    (1, 2, 2, 9),      # H < K for both filters; TW = 16
    (1, 3, 100, 24),   # TW = 32 (TH = 32): one run of 4 blocks, the last 4 rows tall
    (2, 1, 3, 8300),   # 130 strips x 2 images = 260 partials per channel: the second trip of the finalize loops
]
FULL_NUMEL = 2048   # recorded in full below this size, as a SHA-256 of the bytes for every shape


def key(shape, K, S, act=None, training=None):
    k = "x".join(map(str, shape)) + f"/K{K}S{S}"
    return k if act is None else k + f"/{act}/{'train' if training else 'eval'}"


def seed(shape, K, S, act=None, training=None):
    return int(hashlib.sha256(key(shape, K, S, act, training).encode()).hexdigest()[:8], 16)


def plain_cases():
    return [(sh, K, S) for sh in SHAPES for K, S in KS]


def fused_cases():
    """Every shape x (K, S) x activation x mode; batch statistics need more than one value per channel."""
    return [(sh, K, S, act, tr) for sh in SHAPES for K, S in KS for act, tr in FUSED if not (tr and sh[0] * sh[2] * sh[3] == 1)]


def digest(t):
    """SHA-256 over the bytes of a tensor (dense, CPU copy): equal digests <=> torch.equal up to NaN payloads, which the
    tests exclude with isfinite."""
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def plain_case(shape, K, S):
    from test_gpu_backbone_edges import _dw_case

    return _dw_case(*shape, K, S, torch.Generator().manual_seed(seed(shape, K, S)))


def fused_case(shape, K, S, act, training):
    from test_gpu_backbone_edges import _bndw_case

    return _bndw_case(*shape, K, S, act, training, torch.Generator().manual_seed(seed(shape, K, S, act, training)))
