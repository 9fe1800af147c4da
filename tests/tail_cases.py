"""Shapes, launch plans, seeded inputs and float64 references of the three kernel families without autograd -- K13
csrc/eval_tail.hip, K17 csrc/predict_tail.hip, K16 csrc/opt_tail.hip -- shared by the tests of tests/test_gpu_tail_edges.py.

The plan functions restate the host rules of the launchers (the function each restates is named in its docstring) so that the
tables below can say which branch a shape reaches; test_tail_plan_cases_reach_their_branches keeps the tables and, through the
library's queries and the constants read back from the sources, the restatement honest.  Everything here runs on the CPU."""
import os
import re

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from eval_golden import MAX_UNDECIDED_SHARE, TIE_FACTOR
from test_gpu_evaluate import _argmax_hist_plan

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the launchers' constants, restated; source_constants() reads the originals back
EVAL_LDS_MAX = 64 * 1024
PREDICT_LDS_MAX = 64 * 1024
PREDICT_PX = 4
EVAL_HIST_BLOCKS = 512
TAIL_GRID_CAP = 2048
TAIL_CHUNK = 4096
RESTATED = dict(EVAL_LDS_MAX=EVAL_LDS_MAX, PREDICT_LDS_MAX=PREDICT_LDS_MAX, PREDICT_PX=PREDICT_PX, EVAL_HIST_BLOCKS=EVAL_HIST_BLOCKS,
                TAIL_GRID_CAP=TAIL_GRID_CAP, TAIL_CHUNK=TAIL_CHUNK)


def source_constants():
    """The same constants as the sources spell them (the library has no query for the two grid caps)."""
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    def product(src, pattern):
        m = re.search(pattern, src)
        assert m is not None, pattern
        return int(np.prod([int(x) for x in m.group(1).split("*")]))

    ev, pr, op = (text("cabinet_amd", "csrc", n) for n in ("eval_tail.hip", "predict_tail.hip", "opt_tail.hip"))
    assert re.search(r"TAIL_CHUNK\s*=\s*CABINET_SGD_TAIL_CHUNK;", op)
    return dict(EVAL_LDS_MAX=product(ev, r"EVAL_LDS_MAX\s*=\s*([\d\s*]+);"),
                PREDICT_LDS_MAX=product(pr, r"PREDICT_LDS_MAX\s*=\s*([\d\s*]+);"),
                PREDICT_PX=product(pr, r"#define PREDICT_PX\s+(\d+)"),
                EVAL_HIST_BLOCKS=product(ev, r"#define EVAL_HIST_BLOCKS\s+(\d+)"),
                TAIL_GRID_CAP=product(op, r"TAIL_GRID_CAP\s*=\s*(\d+);"),
                TAIL_CHUNK=product(text("include", "cabinet_hip.h"), r"#define CABINET_SGD_TAIL_CHUNK\s+(\d+)"))


# ------------------------------------------------------------------------------------------------ the host rules, restated
def _span(px, wl, w):
    """eval_span / predict_span: source columns `px` output pixels can touch, float32 with ceil as on the host."""
    rw = np.float32(wl) / np.float32(w)
    s = int(np.ceil(np.float32(px) * rw)) + 3
    return min(s, wl)


def eval_span(T, wl, cw):
    return _span(T, wl, cw)


def eval_chip_threads(C, wl, cw, nsrc):
    """eval_chip_threads: the largest of 256, 128, 64 whose staged rows fit the LDS, else 0."""
    for T in (256, 128, 64):
        if nsrc * C * eval_span(T, wl, cw) * 4 <= EVAL_LDS_MAX:
            return T
    return 0


def eval_chip_supported(C, hl, wl, ch, cw, flip):
    """cabinet_eval_chip_accum_supported."""
    if C < 1 or C > 32 or min(hl, wl, ch, cw) < 1 or ch > 65535:
        return False
    return eval_chip_threads(C, wl, cw, 2 if flip else 1) > 0


def eval_chip_plan(C, low, chip, flip):
    """eval_chip_accum_run -> (T, row segments, span, CMAX); T = 0: refused."""
    T = eval_chip_threads(C, low[1], chip[1], 2 if flip else 1)
    if T == 0:
        return 0, None, None, None
    return T, -(-chip[1] // T), eval_span(T, low[1], chip[1]), (C if C in (8, 19) else 0)


def predict_span(px, wl, W):
    return _span(px, wl, W)


def predict_up_threads(C, wl, W):
    """predict_up_threads: among the workgroups that fit the LDS the smallest that still covers the row, else the largest."""
    best = 0
    for T in (256, 128, 64):
        if C * predict_span(PREDICT_PX * T, wl, W) * 4 <= PREDICT_LDS_MAX and (best == 0 or PREDICT_PX * T >= W):
            best = T
    return best


def predict_up_supported(C, hl, wl, H, W):
    """cabinet_predict_up_argmax_supported."""
    if C < 1 or C > 32 or min(hl, wl, H, W) < 1 or H > 65535:
        return False
    return predict_up_threads(C, wl, W) > 0


def predict_up_plan(C, low, out):
    """predict_up_argmax_run -> (T, row segments, span, CMAX, packed for a dword-aligned output); T = 0: refused."""
    T = predict_up_threads(C, low[1], out[1])
    if T == 0:
        return 0, None, None, None, None
    return T, -(-out[1] // (PREDICT_PX * T)), predict_span(PREDICT_PX * T, low[1], out[1]), (C if C in (8, 19) else 0), out[1] % 4 == 0


def argmax_hist_plan(C, N, H, W):
    """eval_argmax_hist_run -> (VEC, CFIX, workgroups)."""
    vec, _, wgs = _argmax_hist_plan(N, H, W)
    assert wgs <= EVAL_HIST_BLOCKS
    return vec, (C if vec == 4 and C in (8, 19) else 0), wgs


def scale_merge_plan(W):
    """eval_scale_merge_run -> (VEC, workgroups in x)."""
    vec = 4 if W % 4 == 0 else 1
    return vec, -(-(W // vec) // 256)


def predict_argmax_plan(C, N, H, W, aligned=True):
    """predict_argmax_run -> (VEC, CFIX, workgroups in x, pixels of an image's last group)."""
    P = H * W
    groups = -(-P // PREDICT_PX)
    vec = P % 4 == 0 and aligned
    return vec, (C if vec and C in (8, 19) else 0), -(-groups // 256), P - (groups - 1) * PREDICT_PX


def tail_chunks(numels):
    """optim.build_chunks: every tensor cut at multiples of TAIL_CHUNK."""
    return sum(-(-n // TAIL_CHUNK) for n in numels)


def tail_grid(n_chunks, max_grid=0):
    """sgd_tail_run: workgroups of the norm and the apply pass."""
    cap = min(max_grid, TAIL_GRID_CAP) if max_grid > 0 else TAIL_GRID_CAP
    return min(n_chunks, cap)


def tail_workspace_bytes(n_chunks):
    return -(-n_chunks * 4 // 256) * 256


# ------------------------------------------------------------------------------------------------ K13 tables
# name -> (C, (hl, wl), (ch, cw), flip, (T, segments, span), N)
CHIP_CASES = {
    "lds-at-64KB": (32, (2, 256), (3, 256), True, (256, 1, 256), 2),
    "one-column-over": (32, (2, 257), (3, 257), True, (128, 3, 131), 2),
    "one-source-stays-256": (32, (2, 260), (3, 260), False, (256, 2, 259), 2),
    "shrink-x3-T64": (32, (2, 300), (3, 100), True, (64, 2, 195), 3),
    "lds-at-64KB-T64": (32, (2, 512), (3, 130), True, (64, 3, 256), 2),
    "c19-T128": (19, (2, 600), (3, 200), True, (128, 2, 387), 2),
    "c19-T64": (19, (2, 480), (3, 120), True, (64, 2, 259), 3),
    "c8-T128": (8, (2, 1152), (3, 256), True, (128, 2, 579), 2),
}
# name -> (C, (hl, wl), (ch, cw), flip), and the supported row of CHIP_CASES next to it
CHIP_REFUSED = {"c32-520-to-130": ((32, (2, 520), (3, 130), True), "lds-at-64KB-T64"),
                "c8-2000-to-100": ((8, (2, 2000), (3, 100), True), "c8-T128")}

# name -> (C, src (FH, FW), crop (hst, hed, wst, wed) or None, out (H, W), (VEC, workgroups in x))
MERGE_CASES = {
    "vec-2-blocks": (2, (3, 515), None, (2, 1028), (4, 2)),
    "vec-2-blocks-shrinking": (3, (4, 2056), None, (2, 1028), (4, 2)),
    "scalar-2-blocks-crop": (1, (5, 300), (1, 4, 7, 290), (3, 259), (1, 2)),
    "scalar-5-blocks": (2, (3, 300), None, (2, 1030), (1, 5)),
    "one-pixel-crop": (2, (6, 9), (2, 3, 4, 5), (5, 7), (1, 1)),
    "to-one-pixel": (1, (4, 4), None, (1, 1), (1, 1)),
}
MERGE_MAX_PLANES = (65535, (1, 1), None, (1, 1), (1, 1))   # N * C = 65535 at the grid's z limit, N = 1

# name -> (C, N, H, W, (VEC, CFIX))
HIST_CASES = {
    "cityscapes-vec4-c19": (19, 2, 6, 10, (4, 19)),
    "vec4-c8": (8, 2, 6, 10, (4, 8)),
    "vec4-any-c": (32, 2, 4, 4, (4, 0)),
    "fewer-classes-than-unroll": (3, 1, 2, 2, (4, 0)),
    "scalar-c19": (19, 2, 3, 5, (1, 0)),
    "one-pixel": (1, 1, 1, 1, (1, 0)),
}

# ------------------------------------------------------------------------------------------------ K17 tables
# name -> (C, (hl, wl), (H, W), (T, segments), seed).  The seed is the first of 1..40 for which the float64 reference alone
# leaves at most MAX_UNDECIDED_SHARE of the pixels undecided (found on the CPU by find_up_seed, asserted by the plan test).
UP_CASES = {
    "widest-single-segment": (19, (2, 128), (3, 1024), (256, 1), 1),
    "second-segment-one-pixel": (19, (2, 129), (3, 1025), (256, 2), 1),
    "two-segments-packed": (19, (2, 130), (3, 1040), (256, 2), 1),
    "production-width-2048": (19, (2, 256), (3, 2048), (256, 2), 1),
    "three-segments-c8": (8, (2, 257), (3, 2049), (256, 3), 1),
    "c32-T128": (32, (2, 512), (2, 512), (128, 1), 1),
    "c32-T64-513": (32, (2, 513), (2, 513), (64, 3), 1),
    "c32-T64-600": (32, (2, 600), (2, 600), (64, 3), 1),
    "c19-862-T256": (19, (2, 862), (2, 862), (256, 1), 1),
    "c19-863-T128": (19, (2, 863), (2, 863), (128, 2), 1),
    "shrink-x4-T64": (8, (2, 4000), (2, 1000), (64, 4), 1),
    "run-time-class-loop": (5, (3, 2100), (2, 2100), (256, 3), 1),
}
UP_REFUSED = {"c32-1030-to-512": (32, (2, 1030), (2, 512)), "c32-2048-to-1024": (32, (2, 2048), (2, 1024))}
# two equal planes: the lowest index wins everywhere -> C, low, out, the two classes
UP_TIES = {"w1040": (19, (2, 130), (3, 1040), (3, 11)), "c32-513": (32, (2, 513), (2, 513), (7, 30))}
# (C, N, H, W): P = 2055, the byte-wise form over three workgroups whose last group holds 3 pixels
ARGMAX_CASES = {"c19-p2055": (19, 2, 5, 411), "c5-p2055": (5, 2, 5, 411)}

SEEDS = range(1, 41)


# ------------------------------------------------------------------------------------------------ inputs and references
def _up(x, size):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)


def chip_inputs(C, low, chip, flip, N, seed):
    """-> a, b or None, rcp_y, rcp_x, (FH, FW): the destination is larger than the window."""
    g = torch.Generator().manual_seed(seed)
    FH, FW = chip[0] + 5, chip[1] + 9
    a = torch.randn(N, C, *low, generator=g) * 3.0
    b = torch.randn(N, C, *low, generator=g) * 3.0 if flip else None
    rcy = 1.0 / torch.randint(1, 4, (FH,), generator=g).float()
    rcx = 1.0 / torch.randint(1, 4, (FW,), generator=g).float()
    return a, b, rcy, rcx, (FH, FW)


def chip_origins(chip, full):
    """The four corners of the destination, then an interior window (run without the reciprocal vectors)."""
    (ch, cw), (FH, FW) = chip, full
    return [(0, 0), (0, FW - cw), (FH - ch, 0), (FH - ch, FW - cw), (2, 5)]


def chip_oracle(dst0, a, b, size, origin, rcy, rcx, dtype=torch.float64):
    """_chip_oracle of test_gpu_evaluate.py in `dtype`: float64 is the reference, float32 the yardstick E32."""
    (ch, cw), (y0, x0) = size, origin
    p = torch.softmax(_up(a.to(dtype), size), dim=1)
    if b is not None:
        p = (p + torch.softmax(torch.flip(_up(b.to(dtype), size), dims=(3,)), dim=1)) * 0.5
    ry = rcy.to(dtype)[y0:y0 + ch] if rcy is not None else torch.ones(ch, dtype=dtype)
    rx = rcx.to(dtype)[x0:x0 + cw] if rcx is not None else torch.ones(cw, dtype=dtype)
    out = dst0.to(dtype).clone()
    out[:, :, y0:y0 + ch, x0:x0 + cw] += p * ry.view(1, 1, -1, 1) * rx.view(1, 1, 1, -1)
    return out


def chip_refs(dst0, a, b, size, origin, rcy, rcx):
    """-> float64 reference, E32 (largest elementwise distance of the fp32 composite on the CPU from it)."""
    want = chip_oracle(dst0, a, b, size, origin, rcy, rcx)
    e32 = float((chip_oracle(dst0, a, b, size, origin, rcy, rcx, torch.float32).double() - want).abs().max())
    return want, e32


def merge_inputs(N, C, src, out, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, C, *src, generator=g), torch.rand(N, C, *out, generator=g) * 2


def merge_refs(total0, prob, crop, out):
    """total0 + resize(prob[crop] -> out) in float64, and E32 of the same in fp32 on the CPU."""
    FH, FW = prob.shape[2:]
    hst, hed, wst, wed = crop if crop is not None else (0, FH, 0, FW)
    want = total0.double() + _up(prob.double()[:, :, hst:hed, wst:wed], out)
    got32 = total0 + _up(prob[:, :, hst:hed, wst:wed], out)
    return want, float((got32.double() - want).abs().max())


def hist_inputs(C, N, H, W, seed):
    """-> total with planted exact ties (the lowest index must win), labels with 255 (ignored), 200 and -3 (clipped), the
    mask of the two-way ties and their lowest class."""
    g = torch.Generator().manual_seed(seed)
    total = torch.rand(N, C, H, W, generator=g)
    tie = torch.rand(N, H, W, generator=g) < 0.3
    lo, hi = (0, 0) if C == 1 else (C // 3, C - 1)
    if C > 1:
        top = total.max(dim=1).values + 1.0
        total[:, hi][tie] = top[tie]
        total[:, lo][tie] = top[tie]
    labels = torch.randint(0, C, (N, H, W), generator=g)
    r = torch.rand(N, H, W, generator=g)
    labels[r < 0.1] = 255
    labels[(r >= 0.1) & (r < 0.17)] = 200
    labels[(r >= 0.17) & (r < 0.24)] = -3
    return total, labels, tie, lo


def hist_ref(total, labels, C, ignore=255):
    pred = torch.argmax(total, dim=1)
    keep = labels != ignore
    idx = pred[keep].numpy() * C + labels[keep].clamp(0, C - 1).numpy()
    return pred, np.bincount(idx, minlength=C * C).reshape(C, C)


def up_case(C, low, out, N, seed):
    """Seeded logits and the decision rule of test_up_argmax_vs_float64 -> a, want, undecided, e32, share."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(N, C, *low, generator=g) * 3.0
    up64 = _up(a.double(), out)
    e32 = float((_up(a, out).double() - up64).abs().max())
    want = torch.argmax(up64, dim=1)
    if C > 1:
        top2 = torch.topk(up64, 2, dim=1).values
        undecided = (top2[:, 0] - top2[:, 1]) < TIE_FACTOR * e32
    else:
        undecided = torch.zeros_like(want, dtype=torch.bool)
    return a, want, undecided, e32, float(undecided.float().mean())


def find_up_seed(C, low, out, N=2, seeds=SEEDS):
    """The first seed whose float64 reference alone leaves at most MAX_UNDECIDED_SHARE undecided -> (seed, case) or None."""
    for seed in seeds:
        case = up_case(C, low, out, N, seed)
        if case[4] <= MAX_UNDECIDED_SHARE:
            return seed, case
    return None


def argmax_inputs(C, N, H, W, seed):
    """randn with the maximum copied into two or three classes, class 0 and class C - 1 among them (test_argmax_equals_torch)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(N, C, H, W, generator=g)
    if C > 1:
        mx = t.max(dim=1).values
        r = torch.rand(N, H, W, generator=g)
        for lo, hi, classes in ((0.0, 0.15, (0, C - 1)), (0.15, 0.3, (C - 1, C // 2)), (0.3, 0.45, (0, C // 2, C - 1))):
            m = (r >= lo) & (r < hi)
            for c in classes:
                t[:, c][m] = mx[m]
    return t


# ------------------------------------------------------------------------------------------------ sweeps
CHIP_CW = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 511, 512, 513]
CHIP_SWEEP_C = [5, 8, 19]
CHIP_SWEEP_HH = [(2, 3), (3, 1)]
MERGE_W = list(range(1, 10)) + [255, 256, 257, 1023, 1024, 1025, 1027, 1028, 1029]
UP_W = list(range(1, 10)) + [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1027, 1028, 2047, 2048, 2049]
UP_SWEEP_C = [5, 8, 19]
HIST_SWEEP_C = [1, 2, 3, 5, 8, 19, 32]
ARGMAX_SWEEP_C = [1, 3, 8, 19, 32]
TAIL_SIZES = list(range(1, 10)) + [255, 256, 257, 1023, 1024, 1025] + list(range(4093, 4100)) + [8191, 8192, 8193]


def _widths(w):
    return sorted({w, -(-w // 8), -(-w * 3 // 7)})


def chip_sweep_shapes(C, hh):
    """(C, (hl, wl), (ch, cw), flip) for cw in CHIP_CW, wl in {cw, ceil(cw / 8), ceil(3 cw / 7)}, both flips."""
    hl, ch = hh
    return [(C, (hl, wl), (ch, cw), flip) for cw in CHIP_CW for wl in _widths(cw) for flip in (False, True)]


def up_sweep_shapes(C):
    """(C, (2, wl), (3, W)) for W in UP_W, wl in {W, ceil(W / 8), ceil(3 W / 7)}."""
    return [(C, (2, wl), (3, W)) for W in UP_W for wl in _widths(W)]


def merge_sweep_shapes():
    """(src, crop, out) for W in MERGE_W at H = 2: a same-size and a x0.75 source, whole and through a crop whose wst is odd
    (the source is then three columns and a row larger than the window)."""
    out = []
    for W in MERGE_W:
        for sw in sorted({W, -(-W * 3 // 4)}):
            sh = 2 if sw == W else 3
            out.append(((sh, sw), None, (2, W)))
            out.append(((sh + 1, sw + 3), (1, 1 + sh, 1, 1 + sw), (2, W)))
    return out


# ------------------------------------------------------------------------------------------------ K16
class Bag(nn.Module):
    """Parameters handed in ready-made; two groups (the _Bag of test_gpu_optim_tail.py)."""

    def __init__(self, tensors):
        super().__init__()
        self.p = nn.ParameterList([nn.Parameter(t) for t in tensors])

    def get_params(self):
        return list(self.p)[0::2], list(self.p)[1::2]


def offset_tensor(values, device):
    """A dense 1-D tensor holding `values` that starts 4 bytes into its storage."""
    store = torch.zeros(values.numel() + 1, device=device)
    store[1:].copy_(values)
    return store[1:]


def tail_state(net, opt):
    """Every parameter, momentum buffer (where one exists) and EMA entry, cloned."""
    out = {f"param.{k}": v for k, v in net.state_dict().items()}
    for k, p in net.named_parameters():
        buf = opt.optim.state.get(p, {}).get("momentum_buffer")
        if buf is not None:
            out[f"buf.{k}"] = buf
    if opt.ema is not None:
        out.update({f"ema.{k}": v for k, v in opt.ema.state_dict().items()})
    return {k: v.detach().clone() for k, v in out.items()}


def against_composite(tensors_of, steps=3, max_grid=0, seed=5, over=None, setup=None, hook=None, device="cuda", finite=True):
    """_against_composite of test_gpu_optim_tail.py with constructor overrides (`over`), a hook after construction
    (`setup(net, opt)`) and one per step between the gradients and the step (`hook(step, net, opt)`, step 1-based), each
    applied to host and device alike.  The kernels on `device` against the class's own composite path on the host, the bounds
    derived there: 4 K 2^-24 ||x|| per tensor on parameters, buffers and EMA (over the finite elements; the non-finite masks
    must be equal, and empty when `finite`), the norm within 1e-6 relative or non-finite on both, the learning rates within one
    fp32 spacing, `it`, `ema_updates` and `skipped` equal.  -> (host net, host tail, device net, device tail)"""
    from optim_tail_model import make_tail

    g = torch.Generator().manual_seed(seed)
    host = Bag(tensors_of("cpu", torch.Generator().manual_seed(seed + 1)))
    dev = Bag(tensors_of(device, torch.Generator().manual_seed(seed + 1)))
    kw = dict(lr0=0.05, wd=5e-4, warmup_steps=1, max_iter=10, ema_tau=4)
    kw.update(over or {})
    oh, od = make_tail(host, **kw), make_tail(dev, **kw)
    od.max_grid = max_grid
    if setup is not None:
        setup(host, oh)
        setup(dev, od)
    for s in range(1, steps + 1):
        for ph, pd in zip(host.p, dev.p):
            gr = torch.randn(ph.shape, generator=g) * 0.05
            ph.grad, pd.grad = gr.clone(), gr.to(device)
        if hook is not None:
            hook(s, host, oh)
            hook(s, dev, od)
        oh.step()
        od.step()
        nh, nd = float(oh.last_grad_norm[0]), float(od.last_grad_norm.cpu()[0])
        assert (abs(nd - nh) <= 1e-6 * nh) if np.isfinite(nh) else not np.isfinite(nd), (s, nh, nd)
        if int(oh._flags[1]):   # the step ran: the schedule's rates of this step
            lh, ld = oh.lr.numpy().astype(np.float32), od.lr.cpu().numpy().astype(np.float32)
            assert np.all(np.abs(ld.astype(np.float64) - lh.astype(np.float64)) <= np.spacing(lh).astype(np.float64)), (s, lh, ld)
    assert (od.it, od.ema_updates, od.skipped) == (oh.it, oh.ema_updates, oh.skipped)
    a, b = tail_state(host, oh), tail_state(dev, od)
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k].double().reshape(-1), b[k].cpu().double().reshape(-1)
        fin = torch.isfinite(x)
        assert torch.equal(fin, torch.isfinite(y)), f"{k}: the non-finite elements of host and device differ"
        assert bool(fin.all()) or not finite, f"{k}: {int((~fin).sum())} non-finite elements"
        err, floor = float((y[fin] - x[fin]).norm()), 4 * steps * 2.0 ** -24 * float(x[fin].norm())
        assert err <= floor, (k, err, floor)
    return host, oh, dev, od
