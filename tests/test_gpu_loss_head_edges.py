"""Loss-head kernels (csrc/ohem.hip: the fused x8-upsample + OHEM-CE head f3, its focal mode K19, the device-side top-n_min
selection) where their host-side launch plans branch and where their rows, segments and chunks end -- every case through the
public wrappers of cabinet_amd.functional or the criteria of cabinet_amd.loss, against float64 on the CPU
(tests/loss_head_cases.py: interpolate + cross_entropy, autograd for the linear map U^T only).

1. `test_loss_head_plan_cases_reach_their_branches` (no kernel launched): the host rules of ohem_up_fwd_run, ohem_segment,
   ohem_up_supported and ohem_up_bwd_run restated, cross-checked against the library's queries, and every row of PLAN_CASES
   asserted to reach the branch it is listed for.  A retuned constant turns it red instead of letting the coverage lapse.
2. Every row in the five modes (plain, weighted, device-selected with and without weights, focal), one head and two, rows with
   Wl % 64 == 0 also with CABINET_OHEM_SEGMENT_KERNEL=1.  Per case:
     loss_px  element by element |got - ref| <= max(4 E32, 1e-5 max(1, |ref|)), E32 the distance of the fp32 composite
              (interpolate + cross_entropy on the CPU) from float64 on the same inputs, both distances printed; ignored pixels
              exactly 0;
     stats    n_valid, n_above exact, sums within 1e-6 relative (focal: [n_valid, D, S] alike);
     dlow     ||a-b|| <= 1e-3 ||b|| and max|a-b| <= 1e-3 max|b|;
     a second call bit-equal, NaN-prefilled outputs where the wrapper takes `out`, the pair bit-equal to the two single heads.
   The threshold is a condition, not a tolerance: the seed of each case is one for which the float64 reference alone has no
   pixel within 4e-5 max(1, t) of t (four times the per-pixel bound), stored in the table and asserted; the device-selected
   modes get t in the middle of the widest gap of the reference above 1.0.  Real ties (B = 2, image 1 a copy of image 0, odd
   k from ohem_select_hip) for one case per backward form.
3. Dense residue sweeps (x8: every Wl around the thread-count steps, the segment seams and the row-kernel widths; general: both
   directions shrinking and growing, fast_y 0, 2, 4, 8), plain single, weighted pair, focal pair; all misses collected into
   one message, the number of shapes asserted, the seed searched per shape on the CPU reference.
4. The radix select on crafted keys: the digit edges (all equal, only the lowest 10 bits differ, only the middle 11), a
   negative, signed-zero and denormal k-th value, k = 1, k = n_valid, at the chunk seams of ohem_select_wgs.
5. The support boundary: shapes the library refuses take the composite path through both OHEM entry points (they raised from
   the launch before `functional.ohem_up_supported` was asked first), their supported neighbours the fused nodes.
6. Caller contract: channels_last, offset, sliced and half-precision logits, offset labels and a strided upstream gradient
   give bit for bit the dense, aligned fp32 call.

Measured on an MI355X, largest elementwise distance of loss_px from float64, kernel against the fp32 composite (E32) on the
same inputs: table rows 1.9e-6 against 1.4e-6, x8 sweep 2.2e-6 against 1.7e-6, general sweep 6.4e-6 against 6.7e-6.  Per map
kernel / E32 lies between 0.8 and 3.5; it is larger (up to 14, on a single pixel) only on planes of at most 35 pixels, where E32
is a few 1e-7 and the 1e-5 floor governs.  Nothing exceeds the bound and no border column, segment seam or last row stands out: the distance is rounding
(summation order, the 1-ulp v_exp_f32 / v_log_f32).
"""
import itertools

import numpy as np
import pytest
import torch

import loss_head_cases as L
from loss_head_cases import COEF, IGNORE, NEIGHBOURS, PLAN_CASES, REFUSED, THRESH, TIE_UNUSED, HeadRef
from test_gpu_backbone_edges import _cmp, _report
from test_gpu_ohem_topk import check_rows, device_select_rows

gpu = pytest.mark.gpu
SEGMENT_ENV = "CABINET_OHEM_SEGMENT_KERNEL"
SWEEP_SEEDS = range(1, 41)
_DIST = {}   # tag -> (E32, kernel distance), printed by the tests that fill it


# ------------------------------------------------------------------------------------------------ 1. the plan table
def _bwd_x(plan):
    return ("row", plan["ipl"]) if plan["x"] == "row" else ("segment", plan["FR"], plan["SX"], plan["nseg"])


def test_loss_head_plan_cases_reach_their_branches():
    """Every row of PLAN_CASES reaches the branch it is there for: the restated host rules against the library's queries
    (cabinet_focal_up_supported with gamma = 0 is check_ohem; the backward workspace; the forward's partial count), then the
    table against the restated rules."""
    from cabinet_amd import _lib

    lib = _lib.load()
    plans = {}
    for name, (shape, seed, fwd1, fwd2, bx, fast_y, y1, y2) in PLAN_CASES.items():
        B, C, Hl, Wl, H, W = shape
        assert lib.cabinet_focal_up_supported(C, Hl, Wl, H, W, 0.0) == 1 and L.supported(*shape), name
        assert lib.cabinet_ohem_up_bwd_workspace_bytes(*shape) == L.workspace_bytes(B, C, H, Wl), name
        assert lib.cabinet_ohem_up_pair_bwd_workspace_bytes(*shape) == 2 * L.workspace_bytes(B, C, H, Wl), name
        assert lib.cabinet_ohem_up_blocks(B, H, W) == B * H, name
        p1, p2 = L.bwd_plan(1, *shape), L.bwd_plan(2, *shape)
        got = (L.fwd_plan(1, C, Wl, W, False), L.fwd_plan(2, C, Wl, W, False), _bwd_x(p1), p1["fast_y"], p1["y"], p2["y"])
        assert got == (fwd1, fwd2, bx, fast_y, y1, y2), (name, got)
        assert _bwd_x(p2) == bx and p2["grid"] == 2 * p1["grid"], name
        # the class tables of the weighted and focal modes (128 bytes per head) move no row of the table across the pair rule
        assert L.fwd_plan(2, C, Wl, W, True) == fwd2, name
        if Wl % 64 == 0 and W == 8 * Wl:   # the forced segment kernel is the x8 form of the segment kernel
            forced = L.bwd_plan(1, *shape, segment_env=True)
            assert forced["x"] == "segment" and forced["FR"] == 8, name
        plans[name] = (p1, p2)
    shape = {n: c[0] for n, c in PLAN_CASES.items()}
    # what each row is there for, in numbers
    assert PLAN_CASES["two-trips-5-segments"][2][2] == 2 and 320 // 64 == 5                      # second trip; ipl = 5: no row kernel
    assert 2 * 32 * 256 * 4 == 65536 > L.LDS_SEG and plans["pair-refused-by-60KB"][0]["lds_row"] == 139264
    assert plans["row-lds-at-64KB-ipl2"][0]["lds_row"] == L.LDS_ROW == plans["row-lds-at-64KB-ipl4"][0]["lds_row"]
    assert plans["row-lds-above-64KB-ipl2"][0]["lds_row"] == 67584 and plans["row-lds-above-64KB-ipl4"][0]["lds_row"] == 69632
    assert plans["segment-sx64-at-61200"][0]["lds"] == 61200 <= L.LDS_SEG < (26 * 68 + 26 * 8 * 68) * 4   # C = 26 at SX = 64
    assert plans["row-ipl1-13-rows"][0]["padded"] and plans["row-ipl1-39-rows"][0]["padded"] and 13 % 8 and 39 % 8
    assert plans["row-fast-y-4"][0]["padded"] and plans["row-fast-y-2"][0]["padded"]
    assert [L.bucket(shape[f"bucket-{c}"][1]) for c in (7, 9, 16, 17, 20, 21)] == [8, 16, 16, 20, 20, 32]
    assert L.bucket(12) == 16 and all(shape[n][3] % 4 for n in shape if n.startswith("bucket-"))   # scalar staging
    B, C, Hl, Wl, H, W = shape["per-head-y-at-fast-y-8"]
    assert Wl % 4 == 0 and (B * C * H * Wl * 4) % 256 != 0
    assert plans["ratio-16-sx16"][0]["R"] == 16 == plans["ratio-16-sx64"][0]["R"] and plans["ratio-64"][0]["R"] == 64
    assert plans["general-ratio-3"][0]["R"] == 3 and plans["ratio-1"][0]["R"] == 1
    assert 19 * 808 * 4 == 61408 <= L.LDS_SEG < 19 * 809 * 4 and 32 * 480 * 4 == L.LDS_SEG < 32 * 481 * 4
    # the refused rows and their supported neighbours: the restated rule and the library agree
    for name, s in REFUSED.items():
        assert lib.cabinet_focal_up_supported(*s, 0.0) == 0 and not L.supported(1, *s), name
    for name, s in NEIGHBOURS.items():
        assert lib.cabinet_focal_up_supported(*s, 0.0) == 1 and L.supported(1, *s), name
    assert L.segment_plan(8, 1, 300)[0] == 0 and L.segment_plan(32, 2, 128)[0] == 0 and L.segment_plan(8, 2, 128)[0] == 4
    # the sweeps of part 3 stay inside the coverage, and the x8 sweep crosses every step it is there for
    for s in _x8_shapes(27, 3) + _x8_shapes(19, 1) + [x for hh in GENERAL_HH for x in _general_shapes(19, hh)]:
        assert lib.cabinet_focal_up_supported(*s[1:], 0.0) == 1 and L.supported(*s), s
    assert {L.fwd_plan(2, 8, wl, 8 * wl, False)[1] for wl in X8_WL} == {64, 128, 192, 256}
    assert {L.fwd_plan(2, 8, wl, 8 * wl, False)[2] for wl in X8_WL} == {1, 2}
    assert {L.bwd_plan(1, 1, 27, 1, wl, 8, 8 * wl)["SX"] for wl in X8_WL if wl not in (64, 128, 256)} == {32}
    assert {L.bwd_plan(1, 1, 8, 1, wl, 8, 8 * wl)["x"] for wl in (64, 128, 256)} == {"row"}
    assert {L.bwd_plan(1, *s)["fast_y"] for hh in GENERAL_HH for s in _general_shapes(8, hh)} == {0, 2, 4, 8}
    # part 4: the pixel counts sit on the chunk seams of the selection's pixel passes
    assert [L.select_wgs(P) for P in SELECT_P] == [1, 1, 2, 4]


# ------------------------------------------------------------------------------------------------ shared pieces
def _dev(t):
    return None if t is None else t.cuda()


def _twice(fails, tag, fn):
    """fn() -> tuple of tensors, called twice: the second call must be bit-equal."""
    a, b = fn(), fn()
    if not all(torch.equal(x, y) for x, y in zip(a, b)):
        fails.append(f"{tag}: a second call differs")
    return a


def _px_check(fails, tag, got, ref):
    """Element by element against float64: max(4 E32, 1e-5 max(1, |ref|)); ignored pixels exactly 0."""
    g = got.detach().double().cpu()
    if tuple(g.shape) != tuple(ref.l.shape) or not bool(torch.isfinite(g).all()):
        fails.append(f"{tag} loss_px: shape {tuple(g.shape)} or not finite")
        return
    err = (g - ref.l).abs()
    bound = torch.clamp(1e-5 * ref.l.abs().clamp_min(1.0), min=4.0 * ref.e32)
    dist = float(err.max())
    _DIST[tag] = (ref.e32, dist)
    over = err - bound
    if bool((over > 0).any()):
        b, oy, ox = np.unravel_index(int(over.argmax()), tuple(err.shape))
        fails.append(f"{tag} loss_px: {int((over > 0).sum())} pixels beyond the bound, the worst |d| = {float(err[b, oy, ox]):.3e} "
                     f"(bound {float(bound[b, oy, ox]):.3e}, E32 {ref.e32:.3e}) at (b, oy, ox) = ({b}, {oy}, {ox}) of {tuple(err.shape)}")
    if bool((g[~ref.valid] != 0).any()):
        fails.append(f"{tag} loss_px: an ignored pixel is not 0")


def _rel_check(fails, tag, name, got, want):
    if not abs(got - want) <= 1e-6 * abs(want):
        fails.append(f"{tag} {name}: {got!r} vs {want!r} (rel {abs(got - want) / max(abs(want), 1e-300):.2e})")


def _ohem_stats_check(fails, tag, stats, ref, w, t):
    wl, _ = ref.weighted(w)
    above = ref.valid & (wl > t)
    nv, na, s = [float(v) for v in stats.cpu()]
    if nv != float(ref.valid.sum()) or na != float(above.sum()):
        fails.append(f"{tag} stats: n_valid {nv} n_above {na} vs {int(ref.valid.sum())} {int(above.sum())}")
    _rel_check(fails, tag, "sum_above", s, float(wl[above].sum()))


def _run_ohem(fails, tag, heads, lab, size, sel_ts=None):
    """heads: one or two (reference, low on the device, class weights on the CPU or None).  Every head through the single-head
    wrappers against its reference; two heads through the pair wrappers, bit-equal to the singles.  sel_ts: per head the
    threshold of the device-selected backward (a `sel` row supplied by the test), else the host-threshold backward."""
    from cabinet_amd import functional as Fn

    singles = []
    for i, (ref, low, w) in enumerate(heads):
        wd, t = _dev(w), (THRESH if sel_ts is None else sel_ts[i])
        wl, wt = ref.weighted(w)
        assert L.gap_to(wl, ref.valid, t) > L.guard(t), (tag, i, t)   # a condition on the reference alone
        htag = f"{tag} head {i} {'w' if w is not None else 'nw'}"
        px, st = _twice(fails, htag + " fwd", lambda: Fn.ohem_up_fwd_hip(low, lab, size, THRESH, IGNORE, wd))
        if sel_ts is None:
            (dl,) = _twice(fails, htag + " bwd", lambda: (Fn.ohem_up_bwd_hip(low, lab, px, size, THRESH, IGNORE, COEF, wd),))
        else:
            row = torch.tensor([t, TIE_UNUSED, 1.0, 0.0], dtype=torch.float64, device="cuda")
            (dl,) = _twice(fails, htag + " bwd_sel", lambda: (Fn.ohem_up_bwd_sel_hip(low, lab, px, size, row, IGNORE, COEF, wd),))
        _px_check(fails, htag, px, ref)
        _ohem_stats_check(fails, htag, st, ref, w, THRESH)
        factor = COEF * wt * (ref.valid & (wl > t)).double()
        _cmp(fails, htag, "dlow", dl, ref.dlow(factor), maxnorm=True, atol=0.0)
        singles.append((px, st, dl))
    if len(heads) == 2:
        (_, la, wa), (_, lb_, wb) = heads
        wa, wb = _dev(wa), _dev(wb)
        ppx, pst = _twice(fails, tag + " pair fwd", lambda: Fn.ohem_up_pair_fwd_hip(la, lb_, lab, size, THRESH, IGNORE, wa, wb))
        if sel_ts is None:
            bwd = lambda: (Fn.ohem_up_pair_bwd_hip(la, lb_, lab, ppx, size, THRESH, IGNORE, COEF, wa, wb),)   # noqa: E731
        else:
            sel = torch.tensor([[t, TIE_UNUSED, 1.0, 0.0] for t in sel_ts], dtype=torch.float64, device="cuda")
            bwd = lambda: (Fn.ohem_up_pair_bwd_sel_hip(la, lb_, lab, ppx, size, sel, IGNORE, COEF, wa, wb),)   # noqa: E731
        (pdl,) = _twice(fails, tag + " pair bwd", bwd)
        for i, (px, st, dl) in enumerate(singles):
            for what, a, b in (("loss_px", ppx[i], px), ("stats", pst[i], st), ("dlow", pdl[i], dl)):
                if not torch.equal(a, b):
                    fails.append(f"{tag} pair head {i} {what}: not bit-equal to the single-head call "
                                 f"(max |d| {float((a.double() - b.double()).abs().max()):.3e})")


def _run_focal(fails, tag, heads, lab, size):
    """heads: one or two (reference, low on the device, class weights or None, gamma); outputs NaN-prefilled."""
    from cabinet_amd import functional as Fn

    def call(lows, ws, gammas):
        nh = len(lows)
        st = torch.full((nh, 3), float("nan"), dtype=torch.float64, device="cuda")
        px, got = Fn.focal_up_fwd_hip(lows, lab, size, gammas, IGNORE, ws, out=st)
        buf = torch.full((nh,) + tuple(lows[0].shape), float("nan"), device="cuda")
        dl = Fn.focal_up_bwd_hip(lows, lab, px, size, gammas, IGNORE, COEF, ws, out=buf)
        assert got is st and dl is buf
        return px, st, dl

    singles = []
    for i, (ref, low, w, gamma) in enumerate(heads):
        htag = f"{tag} focal head {i} gamma {gamma} {'w' if w is not None else 'nw'}"
        px, st, dl = _twice(fails, htag, lambda: call([low], [_dev(w)], [gamma]))
        _px_check(fails, htag, px[0], ref)
        (nv, D, S), factor = ref.focal(w, gamma)
        got = [float(v) for v in st[0].cpu()]
        if got[0] != float(nv):
            fails.append(f"{htag} stats: n_valid {got[0]} vs {nv}")
        _rel_check(fails, htag, "D", got[1], D)
        _rel_check(fails, htag, "S", got[2], S)
        _cmp(fails, htag, "dlow", dl[0], ref.dlow(COEF * factor), maxnorm=True, atol=0.0)
        singles.append((px[0], st[0], dl[0]))
    if len(heads) == 2:
        ppx, pst, pdl = _twice(fails, tag + " focal pair", lambda: call([h[1] for h in heads], [_dev(h[2]) for h in heads],
                                                                         [h[3] for h in heads]))
        for i, (px, st, dl) in enumerate(singles):
            for what, a, b in (("loss_px", ppx[i], px), ("stats", pst[i], st), ("dlow", pdl[i], dl)):
                if not torch.equal(a, b):
                    fails.append(f"{tag} focal pair head {i} {what}: not bit-equal to the single-head call "
                                 f"(max |d| {float((a.double() - b.double()).abs().max()):.3e})")


def _print_distances(what):
    if _DIST:
        e32 = max(v[0] for v in _DIST.values())
        worst = max(_DIST, key=lambda k: _DIST[k][1] / max(_DIST[k][0], 1e-300))
        print(f"{what}: {len(_DIST)} loss maps, largest E32 {e32:.3e}, largest kernel distance {max(v[1] for v in _DIST.values()):.3e}, "
              f"largest kernel / E32 {_DIST[worst][1] / _DIST[worst][0]:.2f} ({worst})")
    _DIST.clear()


# ------------------------------------------------------------------------------------------------ 2. every row, every mode
@gpu
@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_case_every_mode_vs_float64(name, monkeypatch):
    shape, seed = PLAN_CASES[name][:2]
    B, C, Hl, Wl, H, W = shape
    (low_a, low_b, lab, w), ra, rb, clear = L.build_case(shape, seed)
    assert clear, f"{name}: seed {seed} leaves a pixel of the float64 reference inside the guard band of {THRESH}"
    la, lb_, labd, size = low_a.cuda(), low_b.cuda(), lab.cuda(), (H, W)
    # per head and weighting, the threshold of the device-selected modes: inside a gap of the reference, well above THRESH
    ts = {(h, wt): L.gap_threshold(r.weighted(w if wt else None)[0], r.valid) for h, r in (("a", ra), ("b", rb)) for wt in (False, True)}
    fails = []
    _DIST.clear()
    for forced in ([False, True] if Wl % 64 == 0 else [False]):
        if forced:
            monkeypatch.setenv(SEGMENT_ENV, "1")
        for nh in (1, 2):
            tag = f"{name}{' forced-segment' if forced else ''} nh={nh}"
            one = nh == 1
            _run_ohem(fails, tag + " plain", [(ra, la, None)] if one else [(ra, la, None), (rb, lb_, None)], labd, size)
            _run_ohem(fails, tag + " weighted", [(ra, la, w)] if one else [(ra, la, None), (rb, lb_, w)], labd, size)
            _run_ohem(fails, tag + " sel", [(ra, la, None)] if one else [(ra, la, None), (rb, lb_, None)], labd, size,
                      sel_ts=[ts["a", False], ts["b", False]][:nh])
            _run_ohem(fails, tag + " sel+w", [(ra, la, w)] if one else [(ra, la, w), (rb, lb_, w)], labd, size,
                      sel_ts=[ts["a", True], ts["b", True]][:nh])
            _run_focal(fails, tag, [(ra, la, w, 0.5)] if one else [(ra, la, w, 0.5), (rb, lb_, None, 2.0)], labd, size)
    monkeypatch.delenv(SEGMENT_ENV, raising=False)
    torch.cuda.synchronize()
    _print_distances(name)
    _report(fails, 1, 1)


TIE_CASES = {"row-ipl2": (8, 1, 128, 8, 1024), "segment-fr8": (8, 2, 192, 16, 1536), "general-fr0": (8, 3, 5, 9, 15)}


@gpu
@pytest.mark.parametrize("name", list(TIE_CASES))
def test_real_ties_spread_half_over_the_twins(name):
    """B = 2 with image 1 a copy of image 0: every loss has a bit-identical twin, so an odd k from the selection lands between
    the twins of one pixel -- tie = 1/2, and the backward gives both half the weight."""
    from cabinet_amd import functional as Fn

    C, Hl, Wl, H, W = TIE_CASES[name]
    plan = L.bwd_plan(1, 2, C, Hl, Wl, H, W)
    assert _bwd_x(plan)[:2] == {"row-ipl2": ("row", 2), "segment-fr8": ("segment", 8), "general-fr0": ("segment", 0)}[name]
    low, _, lab, _ = L.make_inputs((1, C, Hl, Wl, H, W), 5)
    low, lab = torch.cat([low, low]), torch.cat([lab, lab])
    ref = HeadRef(low, lab, (H, W))
    vals = ref.l[ref.valid].sort(descending=True).values
    k = t_ref = None
    for cand in range(vals.numel() // 8 | 1, vals.numel(), 2):   # the first odd k whose guard band holds the twins only
        t = float(vals[cand - 1])
        near = ((ref.l - t).abs() <= L.guard(t)) & ref.valid
        if int(near.sum()) == 2 and torch.equal(near[0], near[1]):
            k, t_ref = cand, t
            break
    assert k is not None, "no odd k with only the twins inside the guard band"
    lowd, labd = low.cuda(), lab.cuda()
    px, st = Fn.ohem_up_fwd_hip(lowd, labd, (H, W), 100.0, IGNORE)
    assert torch.equal(px[0], px[1]) and float(st[1]) == 0.0
    sel = Fn.ohem_select_hip(px.unsqueeze(0), labd, st.view(1, 3), 100.0, [k], IGNORE, C)
    t_dev, tie, denom, value = [float(v) for v in sel[0].cpu()]
    print(f"{name}: k {k} t {t_dev!r} (reference {t_ref!r}) tie {tie} value {value!r}")
    assert tie == 0.5 and denom == float(k)
    assert abs(t_dev - t_ref) <= max(4.0 * ref.e32, 1e-5 * max(1.0, abs(t_ref)))
    want = (float(vals[:k - 1].sum()) + t_ref) / k
    assert abs(value - want) <= 1e-5 * max(1.0, abs(want))
    fails = []
    (dl,) = _twice(fails, name, lambda: (Fn.ohem_up_bwd_sel_hip(lowd, labd, px, (H, W), sel[0], IGNORE, COEF),))
    factor = COEF * ((ref.valid & (ref.l > t_ref + L.guard(t_ref))).double() + 0.5 * near.double())
    _px_check(fails, name, px, ref)
    _cmp(fails, name, "dlow", dl, ref.dlow(factor), maxnorm=True, atol=0.0)
    _DIST.clear()
    _report(fails, 1, 1)


# ------------------------------------------------------------------------------------------------ 3. dense residue sweeps
X8_WL = list(range(1, 13)) + [31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257]
GENERAL_HH = [(1, 1), (1, 7), (3, 3), (3, 5), (3, 6), (3, 12), (3, 24), (5, 2)]


def _x8_shapes(C, Hl):
    return [(1, C, Hl, Wl, 8 * Hl, 8 * Wl) for Wl in X8_WL]


def _general_shapes(C, hh):
    Hl, H = hh
    return [(1, C, Hl, Wl, H, W) for Wl in range(1, 10)
            for W in sorted({1, 2, 3, 5, 13, Wl, 3 * Wl, 4 * Wl, 8 * Wl - 1, 8 * Wl + 1, 16 * Wl})]


def _sweep(shapes):
    """Plain single, weighted pair (head a without a table), focal pair on every shape; the seed is the first of SWEEP_SEEDS
    whose float64 reference keeps the guard band of THRESH empty for the combinations these modes threshold."""
    fails, ran = [], 0
    _DIST.clear()
    for shape in shapes:
        found = L.find_seed(shape, SWEEP_SEEDS, pairs=(("a", False), ("b", True)))
        assert found is not None, f"{shape}: no seed of {SWEEP_SEEDS} keeps the guard band of the float64 reference empty"
        seed, (low_a, low_b, lab, w), ra, rb = found
        la, lb_, labd, size, tag = low_a.cuda(), low_b.cuda(), lab.cuda(), shape[4:], f"{shape} seed {seed}"
        _run_ohem(fails, tag + " plain", [(ra, la, None)], labd, size)
        _run_ohem(fails, tag + " weighted", [(ra, la, None), (rb, lb_, w)], labd, size)
        _run_focal(fails, tag, [(ra, la, w, 0.5), (rb, lb_, None, 2.0)], labd, size)
        ran += 1
    torch.cuda.synchronize()
    return fails, ran


@gpu
@pytest.mark.parametrize("Hl", [1, 2, 3])
@pytest.mark.parametrize("C", [8, 19, 5, 27])
def test_x8_residue_sweep(C, Hl):
    """W = 8 Wl, H = 8 Hl at every Wl of 1..12 and either side of 32, 64, 128, 192, 256 (the forward's thread counts and second
    trip, the segment seams at 64 and -- C = 27 -- at 32, the whole-row widths 64, 128, 256)."""
    fails, ran = _sweep(_x8_shapes(C, Hl))
    _print_distances(f"x8 sweep C={C} Hl={Hl}")
    _report(fails, ran, 28)


@gpu
@pytest.mark.parametrize("hh", GENERAL_HH, ids=[f"{a}to{b}" for a, b in GENERAL_HH])
@pytest.mark.parametrize("C", [8, 19])
def test_general_ratio_residue_sweep(C, hh):
    """Wl = 1..9 against W in {1, 2, 3, 5, 13, Wl, 3 Wl, 4 Wl, 8 Wl - 1, 8 Wl + 1, 16 Wl}: shrinking, ratio 1, odd and even integer
    ratios, one off the x8 form on either side, and one source pixel; vertically fast_y = 0, 2, 4, 8 and shrinking."""
    fails, ran = _sweep(_general_shapes(C, hh))
    _print_distances(f"general sweep C={C} {hh}")
    _report(fails, ran, 94)


# ------------------------------------------------------------------------------------------------ 4. the radix select's digit edges
SELECT_P = [1023, 1024, 1025, 4 * 256 * 3 + 1]
SELECT_KINDS = ["all-equal", "low-10-bits", "middle-11-bits", "kth-negative", "kth-signed-zero", "k-1", "k-n_valid-unique-min",
                "kth-denormal"]


def _bits(base, ints):
    return (torch.full_like(ints, base, dtype=torch.int32) | ints.to(torch.int32)).view(torch.float32)


def _crafted(kind, n, g):
    """-> (n fp32 values in a random order, n_min of head 0, n_min of head 1)."""
    top = torch.arange(1, 11).float()   # ten values above everything else
    if kind == "all-equal":
        v, ks = torch.full((n,), 1.25), (n // 3, n - 1)
    elif kind == "low-10-bits":       # 1.5 | ten random low bits: every pass descends inside one bin of the two upper digits
        v, ks = _bits(0x3FC00000, torch.randint(0, 1024, (n,), generator=g)), (n // 2, n // 5)
    elif kind == "middle-11-bits":    # the upper and the lowest digit are the same for all
        v, ks = _bits(0x3FC00155, torch.randint(0, 2048, (n,), generator=g) << 10), (n // 2, n // 5)
    elif kind == "kth-negative":
        v, ks = torch.cat([top, -3.0 * torch.rand(n - 10, generator=g) - 1e-3]), (50, n // 2)
    elif kind == "kth-signed-zero":   # both zeros share a key: t comes back as +0.0
        z = torch.zeros(n - 30)
        z[::2] = -0.0
        v, ks = torch.cat([top, z, -1.0 - torch.rand(20, generator=g)]), (64, n - 25)
    elif kind == "k-1":
        v, ks = torch.cat([torch.tensor([100.0]), 3.0 * torch.rand(n - 1, generator=g)]), (1, 3)
    elif kind == "k-n_valid-unique-min":
        v, ks = torch.cat([torch.tensor([-50.0]), 3.0 * torch.rand(n - 1, generator=g) - 1.0]), (n, n - 1)
    else:                             # distinct denormals between ten normal values and the negatives
        m = n // 2
        den = (torch.randperm(0x7FFFF, generator=g)[:m] + 1).to(torch.int32).view(torch.float32)
        v, ks = torch.cat([top, den, -1.0 - torch.rand(n - 10 - m, generator=g)]), (10 + m // 2, 10 + m)
    assert v.numel() == n and v.dtype == torch.float32
    return v[torch.randperm(n, generator=g)], ks


@gpu
@pytest.mark.parametrize("kind", SELECT_KINDS)
def test_select_digit_edges_at_the_chunk_seams(kind):
    """Crafted keys at P = 1023, 1024, 1025 and 3073 pixels, one head and two heads with different n_min: t bit-equal to the
    sort, tie and denom exact, value within 1e-6 (check_rows of test_gpu_ohem_topk.py).  5 % of the pixels are ignored and hold
    1e30 -- above the threshold -- so a pixel that is not excluded by its LABEL shows."""
    thresh = 1e20
    for P, nheads in itertools.product(SELECT_P, (1, 2)):
        g = torch.Generator().manual_seed(P + nheads)
        lab = torch.randint(0, 19, (1, 1, P), generator=g)
        lab[torch.rand(1, 1, P, generator=g) < 0.05] = IGNORE
        valid = (lab != IGNORE).flatten()
        n = int(valid.sum())
        loss_px = torch.full((nheads, P), 1e30)
        n_mins = []
        for i in range(nheads):
            v, ks = _crafted(kind, n, g)
            loss_px[i, valid] = v
            n_mins.append(ks[i])
        loss_px = loss_px.view(nheads, 1, 1, P).cuda()
        what = f"{kind} P={P} nheads={nheads}"
        sel = device_select_rows(loss_px, lab.cuda(), [None] * nheads, thresh, n_mins)
        check_rows(sel, loss_px.cpu(), lab, [None] * nheads, thresh, n_mins, what)   # the sort on the CPU: denormals are kept
        rows = [[float(x) for x in r] for r in sel]
        assert all(r[2] == float(min(k, n)) for r, k in zip(rows, n_mins)), (what, rows)   # every head took the order statistic
        r0 = rows[0]
        if kind == "all-equal":
            assert r0[0] == 1.25 and r0[1] == n_mins[0] / n
        elif kind == "kth-negative":
            assert r0[0] < 0.0 and r0[1] == 1.0
        elif kind == "kth-signed-zero":
            assert r0[0] == 0.0 and not np.signbit(r0[0]) and r0[1] == (64 - 10) / (n - 30)
        elif kind == "k-1":
            assert r0[0] == 100.0 and r0[1] == 1.0 and r0[3] == 100.0
        elif kind == "k-n_valid-unique-min":
            assert r0[0] == -50.0 and r0[1] == 1.0
        elif kind == "kth-denormal":
            assert 0.0 < r0[0] < 1.1754944e-38 and r0[1] == 1.0


# ------------------------------------------------------------------------------------------------ 5. the support boundary
def _ohem_reference(ref, n_min):
    """OhemCELoss(THRESH, n_min) on the first branch in float64 -> loss, dlow."""
    above = ref.valid & (ref.l > THRESH)
    n_above = int(above.sum())
    assert n_above >= min(n_min, int(ref.valid.sum())) > 0
    return float(ref.l[above].sum()) / n_above, ref.dlow(above.double() / n_above)


def _boundary_case(shape):
    found = L.find_seed(shape, SWEEP_SEEDS, pairs=(("a", False), ("b", False)))
    assert found is not None, shape
    return found[1:]


def _boundary_run(name, dims, fused):
    from cabinet_amd.functional import ohem_up_supported
    from cabinet_amd.loss import OhemCELoss, ohem_upsampled_pair

    C, Hl, Wl, H, W = dims
    (low_a, low_b, lab, _), ra, rb = _boundary_case((1,) + dims)
    n_min = H * W // 16
    (loss_a, grad_a), (loss_b, grad_b) = _ohem_reference(ra, n_min), _ohem_reference(rb, n_min)
    labd = lab.cuda()
    fails = []
    assert ohem_up_supported(low_a.cuda(), (H, W)) is fused
    for device_select in (False, True):
        crit_a, crit_b = (OhemCELoss(THRESH, n_min, IGNORE, device_select=device_select).cuda() for _ in range(2))
        tag = f"{name} device_select={device_select}"
        x = low_a.cuda().requires_grad_(True)
        loss = crit_a.forward_upsampled(x, labd, (H, W))
        loss.backward()
        xa, xb = low_a.cuda().requires_grad_(True), low_b.cuda().requires_grad_(True)
        pair = ohem_upsampled_pair(crit_a, xa, crit_b, xb, labd, (H, W))
        pair.backward()
        nodes = type(loss.grad_fn).__name__, type(pair.grad_fn).__name__
        print(f"{tag}: loss {float(loss)!r} (reference {loss_a!r}) pair {float(pair)!r} (reference {loss_a + loss_b!r}) nodes {nodes}")
        if fused:
            assert nodes == ("_OhemUpSelectedBackward", "_OhemUpSelectedPairBackward"), (tag, nodes)
        else:
            assert not any("_OhemUp" in n for n in nodes), (tag, nodes)
        assert loss.is_cuda and pair.is_cuda
        assert abs(float(loss) - loss_a) <= 1e-5 * max(1.0, abs(loss_a)), tag
        assert abs(float(pair) - (loss_a + loss_b)) <= 1e-5 * max(1.0, abs(loss_a + loss_b)), tag
        _cmp(fails, tag, "dlow", x.grad, grad_a, maxnorm=True, atol=0.0)
        _cmp(fails, tag, "pair dlow a", xa.grad, grad_a, maxnorm=True, atol=0.0)
        _cmp(fails, tag, "pair dlow b", xb.grad, grad_b, maxnorm=True, atol=0.0)
    _report(fails, 1, 1)


@gpu
@pytest.mark.parametrize("name", list(REFUSED))
def test_shapes_the_library_refuses_take_the_composite_path(name):
    """Both OHEM entry points, device_select off and on: the composite's loss and gradient (against float64), no fused node in the
    graph, on the device.  Before `functional.ohem_up_supported` was asked first these calls raised RuntimeError from the launch."""
    from cabinet_amd import _lib

    assert _lib.load().cabinet_focal_up_supported(*REFUSED[name], 0.0) == 0
    _boundary_run(name, REFUSED[name], fused=False)


@gpu
@pytest.mark.parametrize("name", list(NEIGHBOURS))
def test_supported_neighbours_of_the_boundary_stay_fused(name):
    from cabinet_amd import _lib

    assert _lib.load().cabinet_focal_up_supported(*NEIGHBOURS[name], 0.0) == 1
    _boundary_run(name, NEIGHBOURS[name], fused=True)


# ------------------------------------------------------------------------------------------------ 6. caller contract
CONTRACT_SHAPES = {"x8-row": (2, 8, 2, 64, 16, 512), "general": (2, 5, 3, 5, 9, 15)}


def _layouts(low, lab):
    """name -> (logits, labels): the same values in another layout."""
    B, C, Hl, Wl = low.shape
    big = torch.zeros(B, C + 2, Hl, Wl + 3, device=low.device)
    big[:, 1:C + 1, :, 2:Wl + 2] = low
    off = torch.empty(low.numel() + 1, device=low.device)[1:].view(low.shape).copy_(low)
    lab8 = torch.empty(lab.numel() + 1, dtype=lab.dtype, device=lab.device)[1:].view(lab.shape).copy_(lab)
    out = {"channels_last": (low.contiguous(memory_format=torch.channels_last), lab), "4 bytes into the storage": (off, lab),
           "a slice": (big[:, 1:C + 1, :, 2:Wl + 2], lab), "labels 8 bytes into their storage": (low, lab8),
           "fp16": (low.half(), lab)}
    assert not out["channels_last"][0].is_contiguous() and off.data_ptr() % 16 == 4 and not out["a slice"][0].is_contiguous()
    assert lab8.data_ptr() % 16 == 8 and low.data_ptr() % 16 == 0 and lab.data_ptr() % 16 == 0
    assert all(torch.equal(a.float(), low) and torch.equal(b, lab) for a, b in out.values())
    return out


def _contract_wrappers(la, lb_, lab, size, w, n_mins):
    from cabinet_amd import functional as Fn

    C = la.shape[1]
    px, st = Fn.ohem_up_fwd_hip(la, lab, size, THRESH, IGNORE, w)
    row = torch.tensor([1.5, 0.5, 1.0, 0.0], dtype=torch.float64, device="cuda")
    ppx, pst = Fn.ohem_up_pair_fwd_hip(la, lb_, lab, size, THRESH, IGNORE, None, w)
    tpx, tst = Fn.ohem_up_pair_fwd_hip(la, lb_, lab, size, 100.0, IGNORE, None, w)   # no pixel above: the selection is active
    fpx, fst = Fn.focal_up_fwd_hip([la, lb_], lab, size, [0.5, 2.0], IGNORE, [w, None])
    return [px, st, Fn.ohem_up_bwd_hip(la, lab, px, size, THRESH, IGNORE, COEF, w),
            Fn.ohem_up_bwd_sel_hip(la, lab, px, size, row, IGNORE, COEF, w), ppx, pst,
            Fn.ohem_up_pair_bwd_hip(la, lb_, lab, ppx, size, THRESH, IGNORE, COEF, None, w),
            Fn.ohem_up_pair_bwd_sel_hip(la, lb_, lab, ppx, size, torch.stack([row, row]), IGNORE, COEF, None, w),
            tst, Fn.ohem_select_hip(tpx, lab, tst, 100.0, n_mins, IGNORE, C, [None, w]), fpx, fst,
            Fn.focal_up_bwd_hip([la, lb_], lab, fpx, size, [0.5, 2.0], IGNORE, COEF, [w, None])]


def _contract_criteria(la, lb_, lab, size, w, n_mins, upstream, autocast):
    from cabinet_amd.loss import OhemCELoss, SoftmaxFocalLoss, focal_upsampled_pair, ohem_upsampled_pair

    def ohem(thresh, n_min, ws):
        return OhemCELoss(thresh, n_min, IGNORE, weight=None if ws is None else ws.clone(), device_select=True).cuda()

    fa, fb = SoftmaxFocalLoss(0.5, weight=w.clone(), ignore_lb=IGNORE).cuda(), SoftmaxFocalLoss(2.0, ignore_lb=IGNORE).cuda()
    xa, xb = la.detach().requires_grad_(True), lb_.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        losses = [ohem(THRESH, n_mins[0], w).forward_upsampled(xa, lab, size),              # 'n_min above thresh'
                  ohem(100.0, n_mins[0], w).forward_upsampled(xb, lab, size),               # top-n_min through the device selection
                  fa.forward_upsampled(xa, lab, size),
                  ohem_upsampled_pair(ohem(THRESH, n_mins[0], None), xa, ohem(THRESH, n_mins[1], w), xb, lab, size),
                  ohem_upsampled_pair(ohem(100.0, n_mins[0], None), xa, ohem(100.0, n_mins[1], w), xb, lab, size),
                  focal_upsampled_pair(fa, xa, fb, xb, lab, size)]
    nodes = [type(v.grad_fn).__name__ for v in losses]
    assert nodes == ["_OhemUpSelectedBackward", "_OhemUpDeviceSelectedBackward", "_FocalUpBackward", "_OhemUpSelectedPairBackward",
                     "_OhemUpDeviceSelectedPairBackward", "_FocalUpBackward"], nodes
    grads = []   # per loss: a half leaf receives each fp32 gradient rounded once
    for v in losses:
        grads += [g for g in torch.autograd.grad(v, [xa, xb], grad_outputs=upstream, allow_unused=True) if g is not None]
    assert len(grads) == 9
    return [v.detach() for v in losses] + grads


@gpu
@pytest.mark.parametrize("name", list(CONTRACT_SHAPES))
def test_loss_head_wrappers_accept_any_layout(name):
    """channels_last logits, logits 4 bytes into their storage, a non-contiguous slice, labels 8 bytes into their storage and
    fp16 logits under autocast (values a half can hold) through every fused wrapper, both criteria and both pair functions: bit
    for bit the dense, aligned fp32 call (the wrappers copy such operands, the kernels are bit-reproducible).  A half leaf
    receives the fp32 call's gradient rounded to half.  The upstream gradient as a view into an expanded (stride-0) tensor
    gives the gradients of a dense one."""
    shape = CONTRACT_SHAPES[name]
    B, C, Hl, Wl, H, W = shape
    low_a, low_b, lab, w = L.make_inputs(shape, 9)
    la, lb_, labd, wd = low_a.half().float().cuda(), low_b.half().float().cuda(), lab.cuda(), w.cuda()
    n_mins, size = [H * W // 3, H * W // 5 | 1], (H, W)
    dense_up = torch.full((), 1.7, device="cuda")
    base_w = _contract_wrappers(la, lb_, labd, size, wd, n_mins)
    base_c = _contract_criteria(la, lb_, labd, size, wd, n_mins, dense_up, False)
    va, vb = _layouts(la, labd), _layouts(lb_, labd)
    for what in va:
        half = what == "fp16"
        (xa, lab_v), (xb, _) = va[what], vb[what]
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            got_w = _contract_wrappers(xa, xb, lab_v, size, wd, n_mins)
        got_c = _contract_criteria(xa, xb, lab_v, size, wd, n_mins, dense_up, half)
        want_c = base_c[:6] + [g.half() if half else g for g in base_c[6:]]
        bad = [i for i, (a, b) in enumerate(zip(got_w, base_w)) if not torch.equal(a, b)]
        assert len(got_w) == len(base_w) and not bad, f"{name}, {what}: wrapper results {bad} differ from the dense, aligned call"
        bad = [i for i, (a, b) in enumerate(zip(got_c, want_c)) if a.dtype != b.dtype or not torch.equal(a, b)]
        assert len(got_c) == len(want_c) and not bad, f"{name}, {what}: criterion results {bad} differ from the dense, aligned call"
    expanded = torch.full((1,), 1.7, device="cuda").expand(5)
    strided_up = expanded[3]
    assert strided_up.dim() == 0 and expanded.stride() == (0,) and strided_up.data_ptr() == expanded.data_ptr()
    got_c = _contract_criteria(la, lb_, labd, size, wd, n_mins, strided_up, False)
    bad = [i for i, (a, b) in enumerate(zip(got_c, base_c)) if not torch.equal(a, b)]
    assert not bad, f"{name}, stride-0 upstream gradient: results {bad} differ from the dense call"
