"""CPU: the references of tests/resize_reference.py are right, their bounds hold for a correct fp32 kernel and reject subtly wrong
ones, and the case tables of tests/resize_cases.py reach every regime the eval resize / crop / fused-mask kernels have.

torch is trusted where it can be: over the forward case list the float64 references agree with F.interpolate on float64 input
(antialias=True for mode 0, antialias=False for mode 2) within one fp32 ulp of the largest source coordinate times the input
range -- torch computes its coordinates in float64, the kernel in fp32 -- and the nearest restatement agrees exactly.

NOT everywhere: torch 2.10 on the CPU returns wrong anti-aliased values when the output width is 1 and the height is resized
(a 7x1 ramp resized to 16x1 comes back as all zeros; 500x3 -> 32x1 is off by 0.09).  Those geometries (aa_torch_excluded) are
checked from first principles instead: every weight row sums to 1 within n U, a constant image stays constant within the bound,
a ramp maps to the ramp sampled at the fp32 centres.  The kernel follows the contract of include/segk.h and ATen's documented
_compute_indices_min_size_weights_aa arithmetic there; do not "fix" it towards torch's output."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_cases as K
import resize_reference as R
import vit_reference
from resize_cases import FWD_CASES, REV_CASES, FwdCase

f32 = np.float32


def aa_torch_excluded(c):
    """output width 1 with a height that is resized or differs from the output height: torch is wrong there (module docstring)"""
    return c.nw == 1 and c.H != c.nh


def _within(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def _killed(ref, bound, mutant):
    """the mutant leaves the bound by 2x at some element (or is not finite)"""
    return not np.isfinite(mutant).all() or _within(mutant, ref, bound) >= 2


# ---- restated coordinates --------------------------------------------------------------------------------------------------
def test_coordinates_match_the_kernel_expressions():
    for n_out, n_in in ((224, 14), (5, 1), (63, 65), (1, 500), (64, 2000), (300, 64), (1200, 37), (16, 7)):
        i0, i1, lam = R.src_index(n_out, n_in)
        t0, t1, tl = vit_reference.src_index_f32(n_out, n_in)                 # the restatement the bilinear matrix already uses
        assert lam.dtype == f32 and np.array_equal(i0, t0.numpy()) and np.array_equal(i1, t1.numpy()) and np.array_equal(lam, tl.numpy())
        assert i1.max() <= n_in - 1 and i0.min() >= 0
    assert R.nearest_index(5, 7).tolist() == [0, 1, 2, 4, 5] and R.nearest_index(16, 7).max() == 6
    assert R.nearest_index(4, 2, "nearest_round").tolist() == [0, 1, 1, 1]
    a = R.Axis(4, 8)                                                           # scale 2: taps o*2 - 1 .. o*2 + 2, weights 1 3 3 1 / 8
    assert a.lo.tolist() == [0, 1, 3, 5] and a.n.tolist() == [3, 4, 4, 3]
    assert a.W[1, 1:5].tolist() == [0.125, 0.375, 0.375, 0.125] and a.W.dtype == f32
    assert np.allclose(a.W[0, :3], np.array([3, 3, 1]) / 7) and a.W[0, 0] == f32(0.75) / f32(1.75)          # clipped and renormalised
    up = R.Axis(16, 7)                                                         # up-scaling: support clamped to 1, at most 2 taps of weight
    assert int(up.n.max()) == 2 and up.lo[0] == 0 and up.lo[-1] + up.n[-1] == 7
    one = R.Axis(1, 500)
    assert (int(one.lo[0]), int(one.n[0])) == (0, 500)


# ---- agreement with torch where it can be trusted --------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_CASES, ids=K.fwd_id)
def test_references_agree_with_torch(case):
    c = case
    assert K.fwd_ref_cost(c) <= K.REF_BUDGET
    for design in ("dense01", "signed", "ramp"):
        x = R.dense_image(design, 3, c.H, c.W)
        # one ulp of the largest source coordinate x the input range.  The dense designs carry this check; on the ramp the range
        # grows with the image (about 0.06 allowed at 2000x3), so its row shows agreement in kind and settles little on its own
        tol = R.coord_ulp(c.H, c.W) * float(x.max() - x.min())
        xt = torch.from_numpy(x).double()[None]
        for mode in (0, 2):
            if mode == 0 and aa_torch_excluded(c):
                continue
            ref, bound = R.resize_f64(x, c.nh, c.nw, mode)
            want = F.interpolate(xt, size=(c.nh, c.nw), mode="bilinear", align_corners=False, antialias=mode == 0)[0].numpy()
            err = float(np.abs(ref - want).max())
            print(f"{K.fwd_id(c)} {design} mode {mode}: |ref - torch| = {err:.3e}, allowed {tol:.3e}")
            assert err <= tol, (design, mode, err, tol)
        near = R.resize_f32(x, c.nh, c.nw, 1)
        want = F.interpolate(torch.from_numpy(x)[None], size=(c.nh, c.nw), mode="nearest")[0].numpy()
        assert near.dtype == f32 and np.array_equal(near, want)
    lab = R.label_image(2, c.H, c.W, K.LABEL_VALUES)
    got = R.resize_f32(lab, c.nh, c.nw, 1)
    assert got.dtype == np.int64 and np.array_equal(got, lab[:, R.nearest_index(c.nh, c.H)][:, :, R.nearest_index(c.nw, c.W)])


@pytest.mark.parametrize("case", [c for c in FWD_CASES if aa_torch_excluded(c)], ids=K.fwd_id)
def test_first_principles_where_torch_is_wrong(case):
    c = case
    assert (c.H, c.W, c.nh, c.nw) in ((7, 1, 16, 1), (500, 375, 1, 1))
    ay, ax = R.Axis(c.nh, c.H), R.Axis(c.nw, c.W)
    for a in (ay, ax):
        s = a.W.astype(np.float64).sum(1)
        assert bool((np.abs(s - 1) <= a.n * R.U).all()) and bool((a.W >= 0).all())              # within n U, n the row's own taps
    x = R.dense_image("constant", 3, c.H, c.W)
    ref, bound = R.resize_f64(x, c.nh, c.nw, 0)
    assert bool((np.abs(ref - x[:, :1, :1].astype(np.float64)) <= bound).all())
    assert _within(R.resize_f32(x, c.nh, c.nw, 0), x[:, :1, :1].astype(np.float64) + 0 * ref, bound) <= 1
    # a ramp along y comes back sampled at the fp32 centres: at center - 0.5 wherever the window is whole and symmetric (every
    # output of the up-scaling whose two taps are inside; the single output that averages the whole 500-row image)
    ramp = np.broadcast_to(np.arange(c.H, dtype=np.float64)[None, :, None], (1, c.H, c.W)).astype(f32)
    ref, _ = R.resize_f64(ramp, c.nh, c.nw, 0)
    centre = np.array([float(R.scale_f32(c.H, c.nh) * (f32(o) + f32(0.5))) for o in range(c.nh)]) - 0.5
    whole = (centre >= 0) & (centre <= c.H - 1)
    assert whole.sum() >= max(1, c.nh - 4)
    tol = R.coord_ulp(c.H, c.W) * (c.H - 1)
    assert float(np.abs(ref[0, whole, 0] - centre[whole]).max()) <= tol
    assert float(np.abs(ref).max()) > 0                                        # not the all-zero image torch returns


# ---- the fp32 arithmetic stays inside each bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_CASES, ids=K.fwd_id)
def test_fp32_arithmetic_stays_inside_the_bounds(case):
    """mode 2: the restatement against the float64 blend of the same weights, 12 U sum |w| |x|; mode 0: the emulated fmaf chain
    (float64 multiply-add rounded to fp32: it can double-round, so the device is held to the bound, not to this) against
    (nx + ny + 2) U sum |wy| |wx| |t|; impulse images: the chain is fl32(wy * wx), exactly"""
    c = case
    for design in K.DESIGNS:
        x = R.dense_image(design, 3, c.H, c.W)
        for mode in (0, 2):
            ref, bound = R.resize_f64(x, c.nh, c.nw, mode)
            ratio = _within(R.resize_f32(x, c.nh, c.nw, mode), ref, bound)
            print(f"{K.fwd_id(c)} {design} mode {mode}: fp32 error / bound = {ratio:.4f}")
            assert ratio <= 1.0
    imp = R.impulse_image(c)
    assert imp.shape[0] == len(set(R.impulse_positions(c))) and bool((imp.sum((1, 2)) == 1).all())
    ay, ax = R.Axis(c.nh, c.H), R.Axis(c.nw, c.W)
    got = R.resize_f32(imp, c.nh, c.nw, 0)
    for k, (y, x_) in enumerate(R.impulse_positions(c)):
        want = (ay.W[:, y].astype(np.float64)[:, None] * ax.W[:, x_].astype(np.float64)[None, :]).astype(f32)   # 48 bits, one rounding
        assert np.array_equal(got[k], want)
    slot = R.resize_pad_f32(imp, c, 0)
    assert slot.shape == (imp.shape[0], c.T, c.T) and np.array_equal(slot[:, c.pt:c.pt + c.nh, c.pl:c.pl + c.nw], got)
    assert int((slot != 0).sum()) == int((got != 0).sum())


@pytest.mark.parametrize("case", REV_CASES + [K.STRADDLE_CASE], ids=K.rev_id)
def test_reverse_references(case):
    c = case
    slot = R.logits_slot(3, c.T)
    for mode in (0, 1):
        z = R.crop_resize_f32(slot, c, mode)
        ref, bound = R.crop_resize_f64(slot, c, mode)
        assert z.shape == (3, c.oh, c.ow) and z.dtype == f32 and _within(z, ref, bound) <= 1.0
        win = torch.from_numpy(slot[:, c.pt:c.pt + c.nh, c.pl:c.pl + c.nw].copy())[None]
        if mode == 1:
            assert np.array_equal(z, F.interpolate(win, size=(c.oh, c.ow), mode="nearest")[0].numpy())
        else:
            want = F.interpolate(win.double(), size=(c.oh, c.ow), mode="bilinear", align_corners=False)[0].numpy()
            assert float(np.abs(ref - want).max()) <= R.coord_ulp(c.nh, c.nw) * float(slot.max() - slot.min())
        lab = R.eval_labels(3, c.oh, c.ow)
        mask, color, counts, M = R.predict_mask_ref(slot, c, mode, R.PALETTE, lab)
        assert np.array_equal(mask, torch.from_numpy(z).argmax(0).numpy()) and np.array_equal(color, R.PALETTE[mask])
        assert int(counts.sum()) == c.oh * c.ow and int(counts[3:].sum()) == 0
        keep = (lab >= 0) & (lab < 3)
        assert int(M.sum()) == int(keep.sum()) and M[1, 2] == int(((mask == 1) & (lab == 2)).sum())
    nan = slot.copy()
    nan[1, c.pt, c.pl] = np.nan
    nan[2, c.pt, c.pl] = np.nan
    assert int(R.predict_mask_ref(nan, c, 1)[0][0, 0]) == 1                     # NaN is maximal, the first NaN wins
    assert 0xA5 not in R.PALETTE.tolist() and len({tuple(p) for p in R.PALETTE.tolist()}) == 8


# ---- mutants ---------------------------------------------------------------------------------------------------------------
def _forward_kills(c, mut):
    """does some run of forward case c (the runs the GPU test makes) tell the mutant from the reference?"""
    for design in K.DESIGNS:
        x = R.dense_image(design, 3, c.H, c.W)
        for mode in K.MODES:
            if mode == 0:
                ref, bound = R.resize_pad_f64(x, c, 0)
                if _killed(ref, bound, R.resize_pad_f64(x, c, 0, mut=mut)[0]):
                    return True
            elif not np.array_equal(R.resize_pad_f32(x, c, mode), R.resize_pad_f32(x, c, mode, mut=mut)):
                return True
    imp = R.impulse_image(c)
    return not np.array_equal(R.resize_pad_f32(imp, c, 0), R.resize_pad_f32(imp, c, 0, mut=mut))


def _flip_kills(c, mut):
    x = R.dense_image("dense01", 3, c.H, c.W)
    return any(not np.array_equal(R.resize_pad_f32(x, c, 2, flip), R.resize_pad_f32(x, c, 2, flip, mut=mut)) for flip in K.FLIPS)


def _reverse_kills(c, mut):
    for C in K.REV_CLASSES:
        slot = R.logits_slot(C, c.T)
        for mode in (0, 1):
            if not np.array_equal(R.crop_resize_f32(slot, c, mode), R.crop_resize_f32(slot, c, mode, mut)):
                return True
            if not np.array_equal(R.predict_mask_ref(slot, c, mode)[0], R.predict_mask_ref(slot, c, mode, mut=mut)[0]):
                return True
    return False


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_killed(mut):
    """a reference with one error -- the tap window shifted by one, the centre without its + 0.5, edge weights not renormalised,
    the support not clamped to 1 when up-scaling, i1 not clamped, round for floor, the window origin or the flip bits swapped,
    row taps not refreshed at a row end -- leaves the bound by 2x or differs in an exact check on at least one case"""
    if mut == "swap_flip":
        killers = [K.fwd_id(c) for c in K.FLIP_CASES if _flip_kills(c, mut)]
        assert len(killers) == len(K.FLIP_CASES), killers
        return
    if mut == "stale_row":
        killers = [K.rev_id(c) for c in REV_CASES if _reverse_kills(c, mut)]
        assert any(c.ow in (1, 2, 3) and K.rev_id(c) in killers for c in REV_CASES), killers
        return
    killers = [K.fwd_id(c) for c in FWD_CASES if _forward_kills(c, mut)]
    print(mut, "killed by", killers)
    assert killers, mut
    if mut in ("swap_pad", "i1_unclamped", "nearest_round"):
        assert any(_reverse_kills(c, mut) for c in REV_CASES), mut
    if mut == "swap_pad":                                    # only an off-centre window can tell
        assert K.fwd_id(FwdCase("inside", 37, 53, 24, 32, 48, 5, 11)) in killers
    if mut == "support_unclamped":                           # only up-scaling under mode 0 can tell
        assert all(c.nh > c.H or c.nw > c.W for c in FWD_CASES if K.fwd_id(c) in killers)


# ---- the tables ------------------------------------------------------------------------------------------------------------
def test_case_tables_reach_every_regime():
    ids = [K.fwd_id(c) for c in FWD_CASES] + [K.rev_id(c) for c in REV_CASES] + [K.wrap_id(c) for c in K.WRAP_CASES]
    assert len(ids) == len(set(ids))
    assert all(K.window_ok(c) for c in FWD_CASES + REV_CASES + K.WRAP_CASES + [K.STRADDLE_CASE, K.WRAP_PREDICT])
    assert {c.regime for c in FWD_CASES} == {"identity", "side1", "anisotropic", "near-identity", "ratio31", "inside", "pad00", "control"}
    shapes = {(c.H, c.W, c.nh, c.nw) for c in FWD_CASES}
    assert shapes >= {(16, 16, 16, 16), (1, 1, 1, 1), (1, 7, 1, 5), (7, 1, 16, 1), (1, 300, 1, 64), (500, 375, 1, 1), (97, 1200, 3, 37),
                      (5, 40, 64, 8), (2, 3, 64, 64), (33, 65, 32, 63), (13, 17, 12, 16), (2000, 3, 64, 2), (37, 53, 24, 32)}
    assert FwdCase("side1", 1, 1, 1, 1, 4, 3, 3) in FWD_CASES and FwdCase("inside", 37, 53, 24, 32, 48, 5, 11) in FWD_CASES
    assert FwdCase("pad00", 37, 53, 24, 32, 48, 0, 0) in FWD_CASES
    assert any(c.nh > c.H and c.nw < c.W for c in FWD_CASES)                                  # up on one axis, down on the other
    assert any(0 < c.pt and c.pt + c.nh < c.T and 0 < c.pl and c.pl + c.nw < c.T for c in FWD_CASES)   # strictly inside on both axes
    assert any(c.pt + c.nh == c.T and c.pt > 0 for c in FWD_CASES) and any(c.pl + c.nw == c.T and c.pl > 0 for c in FWD_CASES)
    assert any(c.H / c.nh > 19 for c in FWD_CASES) and any(c.W / c.nw > 19 for c in FWD_CASES)
    assert any(c.nh > c.H for c in FWD_CASES)                                                 # up-scaling under mode 0
    control = [c for c in FWD_CASES if c.regime == "control"]
    assert len(control) == 1 and max(control[0].nh, control[0].nw) == control[0].T            # aspect kept, centred
    c = control[0]
    assert (c.pt, c.pl) == ((c.T - c.nh) // 2, (c.T - c.nw) // 2) and abs(c.H / c.nh - c.W / c.nw) < 0.01
    assert len(K.FLIP_CASES) == 2 and all(c.H != c.W and c.nh != c.nw for c in K.FLIP_CASES) and len(K.I64_CASES) == 3
    assert len(K.U8_CASES) == 6 and set(K.U8_CHANNELS) == {1, 3, 4} and set(K.LABEL_VALUES) == {-1, 0, 3, 255, 2 ** 31, 2 ** 40 + 1, -(2 ** 63)}
    # no forward or reverse case of the small tables wraps a grid; each wrap case does, and is near the smallest that does
    assert all(K.resize_pad_trips(3, c.T) == 1 and K.resize_pad_u8_trips(c.T) == 1 for c in FWD_CASES)
    assert all(K.crop_resize_trips(8, c.oh, c.ow) == 1 and K.predict_mask_trips(c.oh, c.ow) == 1 for c in REV_CASES)
    for w in K.WRAP_CASES:
        trips = K.resize_pad_u8_trips(w.T) if w.entry == "resize_pad_u8" else K.resize_pad_trips(w.C, w.T)
        assert trips == 2 and (w.H, w.W) == (8, 8)
    assert K.resize_pad_trips(4, 1024) == 1 and K.resize_pad_u8_trips(2048) == 1
    p = K.WRAP_PREDICT
    assert K.predict_mask_trips(p.oh, p.ow) == 2 and K.predict_mask_trips(4096, 4096) == 1 and p.T == 16
    # the reverse table: the inverses of the forward windows, and what the four-pixel walk of predict_mask needs
    fwd_windows = {(c.T, c.pt, c.pl, c.nh, c.nw, c.H, c.W) for c in FWD_CASES}
    assert sum((c.T, c.pt, c.pl, c.nh, c.nw, c.oh, c.ow) in fwd_windows for c in REV_CASES) >= 13
    assert any(c.nh == 1 for c in REV_CASES) and any(c.nw == 1 for c in REV_CASES) and any(c.oh == 1 for c in REV_CASES)
    assert any(c.nh / c.oh > 16 for c in REV_CASES) and any(c.nw / c.ow > 16 for c in REV_CASES)
    assert {c.ow for c in REV_CASES} >= {1, 2, 3, 5} and {c.oh * c.ow for c in REV_CASES} >= {1, 3, 6, 7}
    assert {(c.oh * c.ow) % 4 for c in REV_CASES} == {0, 1, 2, 3}
    assert set().union(*(K.rows_of_a_thread(c) for c in REV_CASES)) == {1, 2, 3, 4}
    assert set(K.REV_CLASSES) == {1, 2, 3, 4, 5, 8}
    s = K.STRADDLE_CASE
    assert (s.nh, s.nw) == (s.oh, s.ow) and s.ow == 3 and K.rows_of_a_thread(s) == {2}
    assert np.array_equal(R.crop_resize_f32(R.logits_slot(2, s.T), s, 0), R.logits_slot(2, s.T)[:, s.pt:s.pt + s.nh, s.pl:s.pl + s.nw])


def test_every_gpu_case_fits_the_memory_budget():
    worst = max([K.fwd_bytes(c, 8) for c in FWD_CASES] + [K.rev_bytes(c, 8) for c in REV_CASES])
    assert worst <= K.MEM_BUDGET
    for w in K.WRAP_CASES:
        elem = 8 if w.entry == "resize_pad_i64" else 4
        assert K.fwd_bytes(w, w.C, elem, in_bytes=1 if w.entry == "resize_pad_u8" else None) <= K.MEM_BUDGET
    p = K.WRAP_PREDICT                                                       # the mask alone: no colour, counts or labels
    assert K.WRAP_PREDICT_C * p.T * p.T * 4 + p.oh * p.ow + 4096 <= K.MEM_BUDGET
