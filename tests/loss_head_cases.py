"""Shapes, launch plans, seeded inputs and the float64 reference of the loss-head kernels (csrc/ohem.hip: the fused x8-upsample +
OHEM-CE head f3, its focal mode K19), shared by the tests of tests/test_gpu_loss_head_edges.py.

The plan functions restate the host rules of ohem.hip (line references in each) so that the table below can say which branch a
shape reaches; test_loss_head_plan_cases_reach_their_branches keeps the table and, through the library's queries, the
restatement honest.  Everything here runs on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

from focal_golden import focal_q_pow_a

IGNORE = 255
THRESH = 0.7       # the reference's OHEM threshold (train.py: OhemCELoss(0.7, ...))
COEF = 0.37
TIE_UNUSED = 0.625  # tie factor handed to the device-selected backward where the reference shows no pixel AT the threshold
LDS_SEG = 60 * 1024
LDS_ROW = 64 * 1024


# ------------------------------------------------------------------------------------------------ the host rules, restated
def bucket(C):
    """Class slots of the instantiation (ohem.hip:929-934, :1050-1055): 8 and 19 are exact, the others predicated."""
    if C in (8, 19):
        return C
    return 8 if C < 8 else 16 if C <= 16 else 20 if C <= 20 else 32


def segment_plan(C, Wl, W):
    """ohem_segment (ohem.hip:943-962) -> (SX, nox_max, R, gplane, lds bytes); SX = 0: no segment width fits 60 KB.
    rw and (SX + 2) / rw are formed in float32 as on the host."""
    rw = np.float32(Wl) / np.float32(W)
    R = max((W + Wl // 2) // Wl, 1)
    SX = 64
    while SX >= 1:
        nox_max = int(np.float32(SX + 2) / rw) + 8
        gplane = -(-nox_max // R)
        want = 32 // R if (R <= 32 and R & (R - 1) == 0) else 8
        gplane += (want - gplane % 32 + 32) % 32
        lds = (C * (SX + 4) + C * R * gplane) * 4
        if lds <= LDS_SEG:
            return SX, nox_max, R, gplane, lds
        SX >>= 1
    return 0, nox_max, R, gplane, lds


def supported(B, C, Hl, Wl, H, W):
    """check_ohem (capi.hip:465-474) with ohem_up_supported (ohem.hip:964-969)."""
    if min(B, C, Hl, Wl, H, W) <= 0 or C > 32 or B > 65535 or H > 65535:
        return False
    return segment_plan(C, Wl, W)[0] > 0 and C * Wl * 4 <= LDS_SEG


def fwd_plan(nh, C, Wl, W, weighted):
    """ohem_up_fwd_run (ohem.hip:886-938) for 16-byte aligned labels and losses -> (form, threads, trips of the pixel loop,
    launches).  `weighted`: any head with a table, or the focal mode (both add the 128-byte tables behind the rows)."""
    wlds = 128 if weighted else 0
    x8 = W == 8 * Wl                                                          # :894
    nt8 = 256 if Wl >= 256 else -(-Wl // 64) * 64                             # :896
    if not x8:
        return "general", 256, -(-W // 256), nh
    pair = nh == 2 and 2 * C * Wl * 4 + 2 * wlds <= LDS_SEG                   # :898
    return ("x8-pair" if pair else "x8"), nt8, -(-Wl // nt8), (1 if pair else nh)


def bwd_plan(nh, B, C, Hl, Wl, H, W, segment_env=False):
    """ohem_up_bwd_run (ohem.hip:979-1074) for 16-byte aligned operands -> a dict: the x pass (`x`: "row" with `ipl`, or
    "segment" with `FR`, `SX`, `nseg`), its grid and whether the grid holds padded workgroups, `fast_y` and the y pass."""
    SX, nox_max, R, gplane, lds = segment_plan(C, Wl, W)
    fast_y = H // Hl if (H % Hl == 0 and (H // Hl) % 2 == 0) else 0           # :993
    x8 = W == 8 * Wl and 8 * (SX + 3) <= nox_max and SX + 3 <= gplane         # :994
    ipl = Wl // 64 if (W == 8 * Wl and Wl % 64 == 0) else 0                   # :997
    lds_row = (4 * C * Wl + W) * 4                                            # :998
    plan = {"fast_y": fast_y, "lds_row": lds_row, "R": R}
    if ipl in (1, 2, 4) and lds_row <= LDS_ROW and not segment_env:           # :1003
        items = H * B
        plan.update(x="row", ipl=ipl, grid=8 * nh * -(-items // 8), padded=items % 8 != 0)   # :1004
    else:
        nseg = -(-Wl // SX)
        items = nseg * H * B
        plan.update(x="segment", FR=8 if x8 else 0, SX=SX, nseg=nseg, lds=lds, grid=8 * nh * -(-items // 8),
                    padded=items % 8 != 0)                                    # :995
    plane_floats = B * C * H * Wl
    slab = workspace_bytes(B, C, H, Wl) // 4                                  # :987
    together = nh == 1 or slab == plane_floats                                # :1062
    y8 = fast_y == 8 and Wl % 4 == 0                                          # :1061
    plan["y"] = "y8" if (y8 and together) else "y" if together else "y-per-head"
    return plan


def workspace_bytes(B, C, H, Wl):
    """ohem_up_bwd_workspace (ohem.hip:940): one T slab, rounded up to 256 bytes."""
    return -(-B * C * H * Wl * 4 // 256) * 256


def select_wgs(P):
    """ohem_select_wgs (ohem.hip:1348-1351): at least four strides of 256 pixels per workgroup, at most 2048 workgroups."""
    return max(1, min(2048, -(-P // (4 * 256))))


# ------------------------------------------------------------------------------------------------ the plan table
# name -> (B, C, Hl, Wl, H, W), seed, and what the shape is there for:
#   fwd   per number of heads (1, 2): (form, threads, trips, launches) of the unweighted forward
#   bwd   the x pass: ("row", ipl) or ("segment", FR, SX, nseg); then fast_y and the y pass of one head / of two heads
# The seed is the first of 1, 2, ... for which no pixel of the float64 reference lies inside the guard band of THRESH (in
# any of the head / weight combinations the modes use); found on the CPU, asserted again by the test that uses it.
PLAN_CASES = {
    "two-trips-5-segments": ((1, 8, 2, 320, 16, 2560), 2, ("x8", 256, 2, 1), ("x8-pair", 256, 2, 1), ("segment", 8, 64, 5), 8, "y8", "y8"),
    "pair-refused-by-60KB": ((1, 32, 1, 256, 8, 2048), 1, ("x8", 256, 1, 1), ("x8", 256, 1, 2), ("segment", 8, 32, 8), 8, "y8", "y8"),
    "192-threads": ((1, 8, 2, 192, 16, 1536), 2, ("x8", 192, 1, 1), ("x8-pair", 192, 1, 1), ("segment", 8, 64, 3), 8, "y8", "y8"),
    "row-lds-at-64KB-ipl2": ((1, 30, 1, 128, 8, 1024), 2, ("x8", 128, 1, 1), ("x8-pair", 128, 1, 1), ("row", 2), 8, "y8", "y8"),
    "row-lds-above-64KB-ipl2": ((1, 31, 1, 128, 8, 1024), 1, ("x8", 128, 1, 1), ("x8-pair", 128, 1, 1), ("segment", 8, 32, 4), 8, "y8", "y8"),
    "row-lds-at-64KB-ipl4": ((1, 14, 1, 256, 8, 2048), 2, ("x8", 256, 1, 1), ("x8-pair", 256, 1, 1), ("row", 4), 8, "y8", "y8"),
    "row-lds-above-64KB-ipl4": ((1, 15, 1, 256, 8, 2048), 1, ("x8", 256, 1, 1), ("x8-pair", 256, 1, 1), ("segment", 8, 64, 4), 8, "y8", "y8"),
    "segment-sx64-at-61200": ((1, 25, 2, 72, 16, 576), 1, ("x8", 128, 1, 1), ("x8-pair", 128, 1, 1), ("segment", 8, 64, 2), 8, "y8", "y8"),
    "segment-sx32-3-segments": ((1, 26, 2, 72, 16, 576), 1, ("x8", 128, 1, 1), ("x8-pair", 128, 1, 1), ("segment", 8, 32, 3), 8, "y8", "y8"),
    "row-ipl1-13-rows": ((1, 8, 3, 64, 13, 512), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("row", 1), 0, "y", "y"),
    "row-ipl1-39-rows": ((3, 8, 3, 64, 13, 512), 3, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("row", 1), 0, "y", "y"),
    "row-fast-y-4": ((1, 8, 3, 64, 12, 512), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("row", 1), 4, "y", "y"),
    "row-fast-y-2": ((1, 8, 3, 64, 6, 512), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("row", 1), 2, "y", "y"),
    "bucket-7": ((1, 7, 1, 5, 8, 40), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y", "y-per-head"),
    "bucket-9": ((1, 9, 1, 5, 8, 40), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y", "y-per-head"),
    "bucket-16": ((1, 16, 1, 5, 8, 40), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y", "y"),
    "bucket-17": ((1, 17, 1, 5, 8, 40), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y", "y-per-head"),
    "bucket-20": ((1, 20, 1, 5, 8, 40), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y", "y-per-head"),
    "bucket-21": ((1, 21, 1, 5, 8, 40), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y", "y-per-head"),
    "bucket-12-wl3": ((1, 12, 1, 3, 8, 24), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y", "y-per-head"),
    "per-head-y-at-fast-y-8": ((1, 5, 1, 4, 8, 32), 1, ("x8", 64, 1, 1), ("x8-pair", 64, 1, 1), ("segment", 8, 64, 1), 8, "y8", "y-per-head"),
    "general-ratio-3": ((1, 8, 3, 5, 9, 15), 1, ("general", 256, 1, 1), ("general", 256, 1, 2), ("segment", 0, 64, 1), 0, "y", "y-per-head"),
    "ratio-1": ((1, 8, 4, 4, 4, 4), 1, ("general", 256, 1, 1), ("general", 256, 1, 2), ("segment", 0, 64, 1), 0, "y", "y"),
    "ratio-16-sx16": ((1, 19, 2, 40, 4, 640), 1, ("general", 256, 3, 1), ("general", 256, 3, 2), ("segment", 0, 16, 3), 2, "y", "y-per-head"),
    "ratio-16-sx64": ((1, 8, 2, 40, 4, 640), 1, ("general", 256, 3, 1), ("general", 256, 3, 2), ("segment", 0, 64, 1), 2, "y", "y"),
    "ratio-64": ((1, 8, 2, 2, 2, 128), 1, ("general", 256, 1, 1), ("general", 256, 1, 2), ("segment", 0, 4, 1), 0, "y", "y-per-head"),
    "widest-row-808": ((1, 19, 1, 808, 8, 6464), 3, ("x8", 256, 4, 1), ("x8", 256, 4, 2), ("segment", 8, 64, 13), 8, "y8", "y8"),
}
# (C, Hl, Wl, H, W) the library refuses, and why; B = 1
REFUSED = {
    "row-19x809": (19, 1, 809, 8, 6472),      # C * Wl * 4 = 61484 > 60 KB
    "row-32x481": (32, 1, 481, 8, 3848),      # 61568 > 60 KB
    "ratio-300": (8, 1, 1, 1, 300),           # the segment buffers of one source column do not fit
    "ratio-64-32-classes": (32, 2, 2, 2, 128),
    # H exceeds the grid.  Hl = 8192 keeps the number of output pixels per source pixel at 16: the composite's upsample
    # backward adds them with fp32 atomics, and with one source pixel for all 65536 rows that sum alone misses 1e-3
    "H-65536": (8, 8192, 1, 65536, 1),
}
NEIGHBOURS = {"row-19x808": (19, 1, 808, 8, 6464), "row-32x480": (32, 1, 480, 8, 3840)}


# ------------------------------------------------------------------------------------------------ inputs and the reference
def make_inputs(shape, seed):
    """low_a, low_b = 2 randn; labels with 12 % ignored; class weights 0.5 + 3 rand with class 1 at 0 (make_case of
    test_gpu_focal_up.py)."""
    B, C, Hl, Wl, H, W = shape
    g = torch.Generator().manual_seed(seed)
    low_a = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    low_b = torch.randn(B, C, Hl, Wl, generator=g) * 2.0
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.12] = IGNORE
    w = 0.5 + 3.0 * torch.rand(C, generator=g)
    w[1] = 0.0
    return low_a, low_b, lab, w


class HeadRef:
    """One head in float64 on the CPU: up = interpolate(low), l = cross_entropy(up, labels) per pixel (0 where ignored), and
    U^T applied to any per-pixel factor times (softmax - onehot) -- the gradient of sum factor * l for a factor held constant.
    `e32` is the largest elementwise distance of the plain fp32 composite (interpolate + cross_entropy in fp32 on the CPU)
    from l: the yardstick of the per-pixel bound."""

    def __init__(self, low, lab, size):
        C = low.shape[1]
        self.z = low.double().requires_grad_(True)
        self.up = F.interpolate(self.z, size=tuple(size), mode="bilinear", align_corners=False)
        x = self.up.detach()
        self.lab, self.valid = lab, lab != IGNORE
        self.t = torch.where(self.valid, lab, torch.zeros_like(lab))
        self.l = F.cross_entropy(x, lab, ignore_index=IGNORE, reduction="none")
        self.smo = torch.softmax(x, dim=1) - F.one_hot(self.t, C).permute(0, 3, 1, 2).double()
        up32 = F.interpolate(low.float(), size=tuple(size), mode="bilinear", align_corners=False)
        l32 = F.cross_entropy(up32, lab, ignore_index=IGNORE, reduction="none")
        self.e32 = float((l32.double() - self.l).abs().max())

    def weighted(self, w):
        """w_t * l per pixel (0 where ignored), and w_t."""
        if w is None:
            return self.l, self.valid.double()
        wt = torch.where(self.valid, w.double()[self.t], torch.zeros_like(self.l))
        return wt * self.l, wt

    def dlow(self, factor):
        return torch.autograd.grad(self.up, self.z, factor.unsqueeze(1) * self.smo, retain_graph=True)[0]

    def focal(self, w, gamma):
        """-> (n_valid, D, S) and the backward's per-pixel factor w_t a(l)."""
        _, wt = self.weighted(w)
        _, qg, a = focal_q_pow_a(self.l, float(gamma))
        return (int(self.valid.sum()), float(wt.sum()), float((wt * qg * self.l).sum())), wt * a


def guard(t):
    """Half-width of the band around a threshold inside which a pixel could legitimately flip: four times the per-pixel bound."""
    return 4e-5 * max(1.0, abs(t))


def gap_to(wl, valid, t):
    """Distance of the nearest valid pixel's w_t l to t (inf without a valid pixel)."""
    v = wl[valid]
    return float((v - t).abs().min()) if v.numel() else float("inf")


def thresh_clear(ra, rb, w, pairs):
    """No valid pixel of the listed (head, weighted?) combinations lies inside the guard band of THRESH."""
    refs = {"a": ra, "b": rb}
    return all(gap_to(refs[h].weighted(w if wt else None)[0], refs[h].valid, THRESH) > guard(THRESH) for h, wt in pairs)


ALL_PAIRS = (("a", False), ("a", True), ("b", False), ("b", True))


def build_case(shape, seed, pairs=ALL_PAIRS):
    """-> (inputs, ra, rb, clear): the seeded inputs, both heads' references and whether the guard band of THRESH is empty."""
    inputs = make_inputs(shape, seed)
    size = shape[4:]
    ra, rb = HeadRef(inputs[0], inputs[2], size), HeadRef(inputs[1], inputs[2], size)
    return inputs, ra, rb, thresh_clear(ra, rb, inputs[3], pairs)


def find_seed(shape, seeds, pairs=ALL_PAIRS):
    """The first seed of `seeds` whose float64 reference alone keeps the guard band of THRESH empty -> (seed, inputs, ra, rb),
    or None."""
    for seed in seeds:
        inputs, ra, rb, clear = build_case(shape, seed, pairs)
        if clear:
            return seed, inputs, ra, rb
    return None


def gap_threshold(wl, valid, lo=1.0, hi=4.0):
    """A threshold for the device-selected modes: the middle (an fp32 value) of the widest gap that the valid pixels' w_t l
    leave inside [lo, hi] -- well above THRESH, so the selected set differs from the plain one."""
    v = wl[valid]
    v = v[(v > lo) & (v < hi)].sort().values
    pts = torch.cat([torch.tensor([lo], dtype=torch.float64), v, torch.tensor([hi], dtype=torch.float64)])
    i = int((pts[1:] - pts[:-1]).argmax())
    return float(np.float32(0.5 * (float(pts[i]) + float(pts[i + 1]))))
