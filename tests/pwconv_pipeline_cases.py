"""Shapes, seeded inputs and the launch plan of the pipelined thin 1x1 convolutions (K10, csrc/pwconv.hip), shared by
tests/test_gpu_pwconv_pipeline.py and tests/golden/make_golden_pwconv_pipeline.py (the generator runs on the library of the
commit BEFORE the pipelined kernels and records what that commit computes)."""
import ctypes
import hashlib
import os

import torch

# One-wave workgroups of the stream kernel: 8 on each of the 256 CUs.  The library launches min(blocks, 256 x resident
# workgroups per CU, at most 8) and does not export that figure, so the plan below is a restatement that no test can hold
# against the launch: if the runtime reported fewer than 8 for an instantiation, the grid would be smaller and the walks of the
# big cases LONGER than stated (still prologue + steady state + drain); the bit comparison does not depend on it.  The grid is
# never larger than the number of blocks, so a wave that walks 0 blocks does not exist.
GRID_CAP = 2048

# (B, Ci, Co, P, misaligned).  The forward runs Ci -> Co, the input gradient its transpose Co -> Ci, the weight gradient both.
CASES = [
    # every row-block count the backbone uses, + 8 -> 8 and 104 -> 56; B in {1, 3}; P % 64 in {0, 1, 37, 63}; P % 4 in {0..3}
    (1, 16, 16, 64 * 5, False),        # P % 64 = 0, P % 4 = 0: 16-byte form, 3 blocks of 128 pixels, the last half empty
    (3, 16, 64, 64 * 7 + 1, False),    # P % 64 = 1, P % 4 = 1: dword form
    (1, 64, 24, 64 * 6 + 37, False),   # P % 64 = 37, P % 4 = 1
    (3, 24, 72, 64 * 4 + 63, False),   # P % 64 = 63, P % 4 = 3
    (1, 72, 24, 64 * 9 + 38, False),   # P % 4 = 2: 8-byte form
    (3, 72, 24, 64 * 2 + 4, False),    # P % 4 = 0 with 72 rows: 8-byte form by the register budget
    (3, 8, 8, 64 * 3 + 2, False),      # P % 4 = 2
    (1, 104, 56, 64 * 5 + 4, False),   # P % 4 = 0, 4 and 2 row blocks
    (1, 16, 64, 128 * 3, False),       # P % 128 = 0: 8-byte form (two row blocks, and 64 rows of dy for dx)
    (1, 16, 16, 60, False),            # less than one block: prologue only, nothing prefetched
    (1, 16, 64, 64 * 6 + 4, True),     # P % 4 = 0 but every pointer one float off 16-byte alignment: dword form
    # pipeline depth at the full grid: walks of 1..2 and 2..3 blocks per wave across image borders
    (3, 16, 16, 128 * 700 + 36, False),   # 16-byte form: 3 * 701 = 2103 blocks on 2048 waves
    (3, 16, 16, 128 * 1400 + 36, False),  # 16-byte form: 4203 blocks: more than twice the grid
    (3, 24, 72, 64 * 1400 + 38, False),   # 8-byte form: 4203 blocks (dx: 24 x 72 is pipelined only past twice the grid)
    (3, 16, 16, 64 * 1400 + 37, False),   # dword form: 4203 blocks
]

SAMPLE = 1024  # elements of an output kept in the fixture (a strided sample), beside the SHA-256 of all of it


def vec_width(M, K, P, aligned=True):
    """stream_launch of pwconv.hip restated: pixels per lane and load (4, 2 or 1) for an M x K product on planes of P pixels."""
    mb, kq = -(-M // 32), -(-K // 16)
    if aligned and P % 4 == 0 and 4 * (32 * mb + 8 * kq) <= 224:  # accumulator (twice) + operand registers of a lane
        return 4
    return 2 if aligned and P % 2 == 0 else 1


def plain_form(M, K, nblocks64):
    """stream_plain of pwconv.hip restated: the products that keep the walk without prefetch (64-pixel blocks, dword accesses)."""
    mb, kq = -(-M // 32), -(-K // 16)
    return (mb == 2 and kq == 2) or (mb == 1 and kq == 5 and nblocks64 <= 2 * GRID_CAP)


def stream_plan(B, M, K, P, aligned=True):
    """-> (vector width, pixels per block, blocks, grid, longest walk of one wave); vector width 0 is the plain form.  The grid is
    256 CUs x the one-wave workgroups resident on one, 8 wherever the instantiation leaves two waves on a SIMD (every case
    here; the library does not export it)."""
    v = 0 if plain_form(M, K, B * -(-P // 64)) else vec_width(M, K, P, aligned)
    px = 32 * max(v, 2)
    nblocks = B * -(-P // px)
    grid = min(nblocks, GRID_CAP)
    return v, px, nblocks, grid, -(-nblocks // grid)


def _gen(shape):
    return torch.Generator().manual_seed(int(hashlib.sha256(f"pwconv/{shape}".encode()).hexdigest()[:8], 16))


def inputs(B, Ci, Co, P, misaligned=False):
    """-> x [B, Ci, P], w [Co, Ci], g [B, Co, P] (CPU, seeded)."""
    g0 = _gen((B, Ci, Co, P))
    return torch.randn(B, Ci, P, generator=g0), torch.randn(Co, Ci, generator=g0) * Ci ** -0.5, torch.randn(B, Co, P, generator=g0)


def on_device(t, misaligned, fill=None):
    """A dense device copy of t (or a NaN-filled tensor of its shape) whose address is one float past 16-byte alignment if asked."""
    flat = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + t.numel()].view(t.shape) if misaligned else flat[:t.numel()].view(t.shape)
    if fill is None:
        v.copy_(t)
    else:
        v.fill_(fill)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 4) == bool(misaligned)
    return v


def load_library(path=None):
    """The package's library, or another build of it (the parent commit's) with the same signatures."""
    from cabinet_amd import _lib

    this = _lib.load()
    if path is None:
        return this
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("cabinet_pwconv_fwd", "cabinet_pwconv_bwd", "cabinet_pwconv_bwd_workspace_bytes", "cabinet_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def _check(lib, rc, who):
    if rc != 0:
        raise RuntimeError(f"{who}: rc {rc}: {lib.cabinet_last_error().decode()}")


def run(lib, xd, wd, gd, misaligned=False):
    """cabinet_pwconv_fwd / cabinet_pwconv_bwd on device tensors, every output NaN before the call -> y, dx, dw."""
    from cabinet_amd.functional import _ptr, _stream_handle, _workspace

    (B, Ci, P), Co = xd.shape, wd.shape[0]
    nan = float("nan")
    y, dx, dw = on_device(gd, misaligned, nan), on_device(xd, misaligned, nan), torch.full_like(wd, nan)
    st = _stream_handle(xd.device)
    _check(lib, lib.cabinet_pwconv_fwd(_ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(y), st), "cabinet_pwconv_fwd")
    ws, nbytes = _workspace(lib.cabinet_pwconv_bwd_workspace_bytes(B, Ci, Co, P), xd.device)
    _check(lib, lib.cabinet_pwconv_bwd(_ptr(gd), _ptr(xd), _ptr(wd), B, Ci, Co, P, _ptr(dx), _ptr(dw), _ptr(ws), nbytes, st),
           "cabinet_pwconv_bwd")
    return y, dx, dw


def dw_ref(x, g):
    """fp64 weight gradient (Co, Ci), one image at a time (the big cases would otherwise hold B fp64 copies)."""
    out = torch.zeros(g.shape[1], x.shape[1], dtype=torch.float64)
    for b in range(x.shape[0]):
        out += g[b].double() @ x[b].double().t()
    return out


def dist(a, ref):
    a, ref = a.detach().double().cpu(), ref.double()
    return float((a - ref).norm() / ref.norm())


def key(case):
    return "x".join(str(int(v)) for v in case)


def digest(t):
    """SHA-256 over the bytes of a tensor: equal digests <=> torch.equal up to NaN payloads, which the tests exclude."""
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def sample(t):
    """A fixed strided sample of at most SAMPLE elements (an odd stride, so that it walks through columns, rows and channels)."""
    flat = t.detach().cpu().contiguous().view(-1)
    stride = max(1, flat.numel() // SAMPLE) | 1
    return flat[::stride][:SAMPLE].clone()
