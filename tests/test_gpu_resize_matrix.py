"""GPU (-m gpu): the eval resize, crop and fused-mask entries (the second half of csrc/resize.hip: segk_resize_pad[_flip],
segk_resize_pad_u8[_flip], segk_crop_resize, segk_predict_mask) through the C ABI against the references of
tests/resize_reference.py, on the case tables of tests/resize_cases.py (tests/test_resize_cases_host.py proves on the CPU that the
tables reach every regime and that the checks made here tell subtly wrong kernels from right ones).

Every output buffer is pre-filled with a NaN or byte pattern and followed by a guard of the same pattern: after the call every
element of the slot [C, T, T] (exactly +0.0 outside the window), of [C, oh, ow], every mask and colour byte is overwritten and
the guard is untouched.

  modes 1 and 2, crop_resize, int64:  equal to the fp32 / integer restatement, bit for bit.
  mode 0 (anti-aliased):              impulse images equal fl32(wy * wx); dense, constant and ramp images within the derived bound
                                      (nx + ny + 2) U sum |wy| |wx| |t| of the float64 reference.
  u8 route, flips:                    the same checks, and the same bits as the float route on the converted / flipped image.
  predict_mask:                       mask, colour, counts and confusion counts exact; counts and M accumulate over two calls; the
                                      call with every option off gives the same mask; NaN and exact ties at a row straddle.
  grid-stride wraps:                  the whole output of one launch behind each capped grid.
  refusals:                           a window one past the far edge is refused before any launch.
Equality of fp32 outputs is equality of all 32 bits of every element (-0.0 is not +0.0), against the NumPy restatement as between
two device routes; only where the reference itself holds NaN (the NaN pixels of the straddle test) it is NaN at the same places and
numerical equality elsewhere.
Set SEGK_RESIZE_PARITY_OUT=<file> to record the worst error / bound per kernel, mode, design and regime
(profiles/eval_resize_matrix_parity.txt)."""
import os

import numpy as np
import pytest
import torch

import resize_cases as K
import resize_reference as R
from matrix_helpers import (NAN_BITS, assert_equal, assert_identical, assert_within, make_recorder, nan_buffer, ptr, stream, sync, take,
                            write_parity)
from resize_cases import FWD_CASES, REV_CASES

pytestmark = pytest.mark.gpu

_PARITY, record = make_recorder()


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_RESIZE_PARITY_OUT")
    if out and _PARITY:
        write_parity(out, _PARITY,
                     "# worst error / bound per kernel, mode, design and regime of tests/test_gpu_resize_matrix.py (references and bounds:\n"
                     "# tests/resize_reference.py); 0.0000 marks an exact run: every element equal to the fp32 / integer restatement\n"
                     "# mode 0 dense rows: |device - float64| / ((nx + ny + 2) U sum |wy| |wx| |t|), derived, not fitted\n", width=58)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def resize_pad(lib, img, c, mode, flip=None, elem=0, what=""):
    """segk_resize_pad[_flip] of img [C, H, W] (fp32, or int64 with elem = 1) -> the whole slot [C, T, T] on the CPU"""
    C, dt = img.shape[0], "i64" if elem else "fp32"
    d, n = dev(img), img.shape[0] * c.T * c.T
    out = nan_buffer(n, dt)
    if flip is None:
        lib.call("segk_resize_pad", ptr(d), ptr(out), C, c.H, c.W, c.nh, c.nw, c.T, c.pt, c.pl, mode, elem, stream())
    else:
        lib.call("segk_resize_pad_flip", ptr(d), ptr(out), C, c.H, c.W, c.nh, c.nw, c.T, c.pt, c.pl, mode, elem, flip, stream())
    sync(what)
    return take(out, n, dt, what).reshape(C, c.T, c.T)


def resize_pad_u8(lib, img_hwc, c, mode, flip=None, what=""):
    cin = img_hwc.shape[2]
    co = min(cin, 3)
    d, n = dev(img_hwc), co * c.T * c.T
    out = nan_buffer(n, "fp32")
    if flip is None:
        lib.call("segk_resize_pad_u8", ptr(d), ptr(out), cin, c.H, c.W, c.nh, c.nw, c.T, c.pt, c.pl, mode, stream())
    else:
        lib.call("segk_resize_pad_u8_flip", ptr(d), ptr(out), cin, c.H, c.W, c.nh, c.nw, c.T, c.pt, c.pl, mode, flip, stream())
    sync(what)
    return take(out, n, "fp32", what).reshape(co, c.T, c.T)


def padding_is_plus_zero(slot, c, what):
    """outside the window every element is +0.0: all bits clear, neither -0.0 nor NaN"""
    bits = slot.view(torch.int32 if slot.dtype == torch.float32 else slot.dtype).clone()
    bits[:, c.pt:c.pt + c.nh, c.pl:c.pl + c.nw] = 0
    assert int((bits != 0).sum()) == 0, f"{what}: {int((bits != 0).sum())} padding elements are not +0"


def assert_same_bits(got, want, what):
    """fp32 tensors whose reference holds no NaN: numerically equal (that message names the elements), then the same 32 bits of
    every element, which also tells -0.0 from +0.0"""
    assert_equal(got, want, what)
    same = torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    assert same, f"{what}: equal numbers but other bits (a signed zero)"


def check_float_slot(got, img, c, mode, flip, exact, name, what, cid):
    """got: the device slot of img under (mode, flip); exact: equal to the fp32 restatement, else within the mode-0 bound.
    name is "entry modeN design regime"; the exact runs of an entry, mode and regime share one row"""
    padding_is_plus_zero(got, c, what)
    if exact:
        assert_same_bits(got, t64(R.resize_pad_f32(img, c, mode, flip or 0)), what)
        entry, md, design, regime = name.split()
        record(f"{entry} {md} {'impulse' if mode == 0 else 'exact'} {regime}", 0.0, cid)
    else:
        ref, bound = R.resize_pad_f64(img, c, mode, flip or 0)
        record(name, assert_within(got, t64(ref), t64(bound), what), cid)


# ---- segk_resize_pad, float --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_CASES, ids=K.fwd_id)
def test_resize_pad_float(lib, case):
    c, cid = case, K.fwd_id(case)
    for mode in K.MODES:
        for C in K.CHANNELS:
            for design in K.DESIGNS:
                img = R.dense_image(design, C, c.H, c.W)
                what = f"resize_pad mode {mode} {design} C={C} {cid}"
                got = resize_pad(lib, img, c, mode, what=what)
                check_float_slot(got, img, c, mode, None, mode != 0, f"resize_pad mode{mode} {design} {c.regime}", what, cid)
                if (c.H, c.W) == (c.nh, c.nw):
                    assert_same_bits(got[:, c.pt:c.pt + c.nh, c.pl:c.pl + c.nw], t64(img), what + " (identity)")
        imp = R.impulse_image(c)
        what = f"resize_pad mode {mode} impulses {cid}"
        got = resize_pad(lib, imp, c, mode, what=what)
        check_float_slot(got, imp, c, mode, None, True, f"resize_pad mode{mode} impulse {c.regime}", what, cid)


@pytest.mark.parametrize("case", K.FLIP_CASES, ids=K.fwd_id)
def test_resize_pad_flips(lib, case):
    c, cid = case, K.fwd_id(case)
    img, imp = R.dense_image("signed", 3, c.H, c.W), R.impulse_image(c)
    u8, u8imp = R.u8_image(c, 3), R.u8_impulse_image(c, 3)
    labs = R.label_image(2, c.H, c.W, K.LABEL_VALUES)
    for flip in K.FLIPS:
        for mode in K.MODES:
            what = f"resize_pad_flip mode {mode} flip {flip} {cid}"
            got = resize_pad(lib, img, c, mode, flip=flip, what=what)
            check_float_slot(got, img, c, mode, flip, mode != 0, f"resize_pad_flip mode{mode} signed {c.regime}", what, cid)
            # the flipped image through the unflipped entry: the same bits
            same = resize_pad(lib, R.flip_image(img, flip), c, mode, what=what + " (flipped source)")
            assert torch.equal(got.view(torch.int32), same.view(torch.int32)), what + ": differs from the unflipped entry on the flipped image"
            got = resize_pad(lib, imp, c, mode, flip=flip, what=what + " impulses")
            check_float_slot(got, imp, c, mode, flip, True, f"resize_pad_flip mode{mode} impulse {c.regime}", what + " impulses", cid)
            for name, pic in (("dense", u8), ("impulse", u8imp)):
                conv = R.u8_to_float(pic)
                got = resize_pad_u8(lib, pic, c, mode, flip=flip, what=what + f" u8 {name}")
                check_float_slot(got, conv, c, mode, flip, mode != 0 or name == "impulse", f"resize_pad_u8_flip mode{mode} {name} {c.regime}",
                                 what + f" u8 {name}", cid)
                same = resize_pad(lib, conv, c, mode, flip=flip, what=what + " (float route)")
                assert torch.equal(got.view(torch.int32), same.view(torch.int32)), what + f" u8 {name}: differs from the float route"
        got = resize_pad(lib, labs, c, 1, flip=flip, elem=1, what=f"resize_pad_flip int64 flip {flip} {cid}")
        assert_identical(got, t64(R.resize_pad_f32(labs, c, 1, flip)), f"resize_pad_flip int64 flip {flip} {cid}")
        record(f"resize_pad_flip int64 {c.regime}", 0.0, cid)
    out = nan_buffer(3 * c.T * c.T, "fp32")                 # the size a launch would write: refused before any launch
    with pytest.raises(RuntimeError, match="flip is 0..3"):
        lib.call("segk_resize_pad_flip", ptr(dev(img)), ptr(out), 3, c.H, c.W, c.nh, c.nw, c.T, c.pt, c.pl, 0, 0, 4, stream())
    sync("flip refusal")
    assert bool((out.cpu() == NAN_BITS["fp32"]).all()), "the refused call wrote to its output"


# ---- segk_resize_pad_u8 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.U8_CASES, ids=K.fwd_id)
def test_resize_pad_u8(lib, case):
    c, cid = case, K.fwd_id(case)
    for cin in K.U8_CHANNELS:
        for mode in K.MODES:
            for name, pic in (("dense", R.u8_image(c, cin)), ("impulse", R.u8_impulse_image(c, cin))):
                what = f"resize_pad_u8 mode {mode} {name} Cin={cin} {cid}"
                conv = R.u8_to_float(pic)
                got = resize_pad_u8(lib, pic, c, mode, what=what)
                check_float_slot(got, conv, c, mode, None, mode != 0 or name == "impulse", f"resize_pad_u8 mode{mode} {name} {c.regime}", what, cid)
                same = resize_pad(lib, conv, c, mode, what=what + " (float route)")
                assert torch.equal(got.view(torch.int32), same.view(torch.int32)), what + ": differs from the float route"
                if cin == 4 and name == "dense":           # another alpha plane: the same slot
                    other = R.u8_image(c, 4, alpha_key=1)
                    assert np.array_equal(other[:, :, :3], pic[:, :, :3]) and not np.array_equal(other[:, :, 3], pic[:, :, 3])
                    again = resize_pad_u8(lib, other, c, mode, what=what + " (other alpha)")
                    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), what + ": the alpha byte is not ignored"


# ---- segk_resize_pad, int64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.I64_CASES, ids=K.fwd_id)
def test_resize_pad_int64(lib, case):
    c, cid = case, K.fwd_id(case)
    for C in K.CHANNELS:
        labs = R.label_image(C, c.H, c.W, K.LABEL_VALUES)
        assert set(np.unique(labs).tolist()) <= set(K.LABEL_VALUES) and NAN_BITS["i64"] not in K.LABEL_VALUES
        what = f"resize_pad int64 C={C} {cid}"
        got = resize_pad(lib, labs, c, 1, elem=1, what=what)
        padding_is_plus_zero(got, c, what)
        assert_identical(got, t64(R.resize_pad_f32(labs, c, 1)), what)
        record(f"resize_pad int64 {c.regime}", 0.0, cid)
    d, out = dev(labs), nan_buffer(C * c.T * c.T, "i64")    # the size a launch would write: refused before any launch
    for mode in (0, 2):
        with pytest.raises(RuntimeError, match="nearest only"):
            lib.call("segk_resize_pad", ptr(d), ptr(out), C, c.H, c.W, c.nh, c.nw, c.T, c.pt, c.pl, mode, 1, stream())
    sync("int64 refusal")
    assert bool((out.cpu() == NAN_BITS["i64"]).all()), "the refused call wrote to its output"


# ---- segk_crop_resize and segk_predict_mask --------------------------------------------------------------------------------
def crop_resize(lib, slot_d, C, c, mode, what):
    n = C * c.oh * c.ow
    out = nan_buffer(n, "fp32")
    lib.call("segk_crop_resize", ptr(slot_d), ptr(out), C, c.T, c.pt, c.pl, c.nh, c.nw, c.oh, c.ow, mode, stream())
    sync(what)
    return take(out, n, "fp32", what).reshape(C, c.oh, c.ow)


def predict_mask(lib, slot_d, C, c, mode, what, palette=None, labels=None, counts=None, M=None):
    """-> (mask [oh, ow] uint8, color [oh, ow, 3] uint8 or None) on the CPU, every byte written and the guards intact; counts
    and M are device buffers the call adds to"""
    total = c.oh * c.ow
    mask = nan_buffer(total, "u8")
    color = nan_buffer(3 * total, "u8") if palette is not None else None
    lib.call("segk_predict_mask", ptr(slot_d), ptr(mask), ptr(color), ptr(palette), ptr(counts), ptr(labels), ptr(M), C, c.T, c.pt, c.pl,
             c.nh, c.nw, c.oh, c.ow, mode, stream())
    sync(what)
    m = take(mask, total, "u8", what + " mask").reshape(c.oh, c.ow)
    return m, None if color is None else take(color, 3 * total, "u8", what + " color").reshape(c.oh, c.ow, 3)


def count_buffers():
    """counts [8] and M [8, 8] as patterned int64 buffers that start at 5 and 7: the entry adds to what is there"""
    counts, M = nan_buffer(8, "i64"), nan_buffer(64, "i64")
    counts[:8] = 5
    M[:64] = 7
    return counts, M


def assert_equal_nan(got, want, what):
    """assert_equal where the reference itself holds NaN: NaN at the same places, every other element equal"""
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN at {gn.nonzero().tolist()[:10]}, want NaN at {wn.nonzero().tolist()[:10]}"
    assert_equal(torch.where(gn, torch.zeros_like(got), got), torch.where(wn, torch.zeros_like(want), want), what)


def check_reverse(lib, c, cid, slot, C, modes, with_singles):
    slot_d, pal_d = dev(slot), dev(R.PALETTE)
    labs = R.eval_labels(C, c.oh, c.ow)
    labs_d = dev(labs)
    for mode in modes:
        what = f"mode {mode} C={C} {cid}"
        z = crop_resize(lib, slot_d, C, c, mode, "crop_resize " + what)
        want_z = t64(R.crop_resize_f32(slot, c, mode))
        (assert_equal_nan if bool(torch.isnan(want_z).any()) else assert_same_bits)(z, want_z, "crop_resize " + what)
        record(f"crop_resize mode{mode} {c.regime}", 0.0, cid)
        want_mask, want_color, want_counts, want_M = R.predict_mask_ref(slot, c, mode, R.PALETTE, labs)
        assert int(want_mask.max()) < C
        counts, M = count_buffers()
        for call in (1, 2):
            mask, color = predict_mask(lib, slot_d, C, c, mode, "predict_mask " + what, pal_d, labs_d, counts, M)
            assert_identical(mask, t64(want_mask), "predict_mask mask " + what)
            assert_identical(color, t64(want_color), "predict_mask color " + what)
            assert_identical(take(counts, 8, "i64", what + " counts"), t64(5 + call * want_counts), f"predict_mask counts after call {call} " + what)
            assert_identical(take(M, 64, "i64", what + " M").reshape(8, 8), t64(7 + call * want_M), f"predict_mask M after call {call} " + what)
        assert int(want_counts[C:].sum()) == 0 and int(want_M[C:].sum()) == 0 and int(want_M[:, C:].sum()) == 0
        # predict_mask == crop_resize + argmax on the device's own values (segk.h), and every option off: the same mask
        assert_identical(mask, t64(R.argmax_first_nan_max(z.numpy()).astype(np.uint8)), "predict_mask against crop_resize + argmax " + what)
        bare, none = predict_mask(lib, slot_d, C, c, mode, "predict_mask (options off) " + what)
        assert none is None
        assert_identical(bare, mask, "predict_mask (options off) " + what)
        if with_singles:
            m, col = predict_mask(lib, slot_d, C, c, mode, "predict_mask (colour only) " + what, palette=pal_d)
            assert_identical(m, mask, "predict_mask (colour only) " + what)
            assert_identical(col, t64(want_color), "predict_mask (colour only) color " + what)
            counts, M = count_buffers()
            m, _ = predict_mask(lib, slot_d, C, c, mode, "predict_mask (counts only) " + what, counts=counts)
            assert_identical(m, mask, "predict_mask (counts only) " + what)
            assert_identical(take(counts, 8, "i64", what + " counts"), t64(5 + want_counts), "predict_mask (counts only) counts " + what)
            m, _ = predict_mask(lib, slot_d, C, c, mode, "predict_mask (labels only) " + what, labels=labs_d, M=M)
            assert_identical(m, mask, "predict_mask (labels only) " + what)
            assert_identical(take(M, 64, "i64", what + " M").reshape(8, 8), t64(7 + want_M), "predict_mask (labels only) M " + what)
        record(f"predict_mask mode{mode} {c.regime}", 0.0, cid)


@pytest.mark.parametrize("case", REV_CASES, ids=K.rev_id)
def test_crop_resize_and_predict_mask(lib, case):
    c, cid = case, K.rev_id(case)
    for C in K.REV_CLASSES:
        check_reverse(lib, c, cid, R.logits_slot(C, c.T), C, (0, 1), with_singles=C in (3, 5))


@pytest.mark.parametrize("mode", [0, 1], ids=["bilinear", "nearest"])
def test_nan_and_ties_at_a_row_straddle(lib, mode):
    """ow = 3, identity geometry: a thread owns four flat pixels, thread 0 (0,0) (0,1) (0,2) (1,0), thread 2 (2,2) (3,0) (3,1) (3,2),
    thread 3 (4,0) (4,1) (4,2) (5,0).  NaN beats every number, of two NaNs the first wins, of an exact tie the lowest index -- also
    right behind a row end.  (Under bilinear a NaN also reaches the pixels above and left of it through their zero-weight taps,
    0 * NaN; the marked pixels are chosen clear of each other, and the reference restates the rest.)"""
    c, C = K.STRADDLE_CASE, 4
    slot = R.logits_slot(C, c.T, key="straddle")
    at = lambda k, y, x: (k, c.pt + y, c.pl + x)
    slot[at(2, 1, 0)] = np.nan                                         # the pixel behind thread 0's row end
    slot[at(1, 3, 0)] = np.nan; slot[at(3, 3, 0)] = np.nan             # behind thread 2's row end: two NaNs, the first
    slot[at(0, 1, 1)] = 5.0; slot[at(3, 1, 1)] = 5.0                   # exact tie above the fill range: the lowest index
    slot[at(1, 0, 2)] = 4.0; slot[at(2, 0, 2)] = 4.0                   # the last pixel of a row
    slot[at(3, 5, 0)] = np.nan; slot[at(0, 5, 0)] = 9.0                # thread 3's last pixel: NaN beats the largest number
    check_reverse(lib, c, K.rev_id(c), slot, C, (mode,), with_singles=True)
    mask, _ = predict_mask(lib, dev(slot), C, c, mode, "straddle")
    assert (int(mask[1, 0]), int(mask[3, 0]), int(mask[1, 1]), int(mask[0, 2]), int(mask[5, 0])) == (2, 1, 0, 1, 3)


# ---- the grid-stride wrap of each capped grid --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.WRAP_CASES, ids=K.wrap_id)
def test_grid_stride_wrap_forward(lib, case):
    c, cid = case, K.wrap_id(case)
    for mode in c.modes:
        what = f"{c.entry} wrap mode {mode} {cid}"
        if c.entry == "resize_pad_u8":
            assert K.resize_pad_u8_trips(c.T) == 2
            pic = R.u8_image(c, c.C)
            got = resize_pad_u8(lib, pic, c, mode, what=what)
            want = R.resize_pad_f32(R.u8_to_float(pic), c, mode)
        elif c.entry == "resize_pad_i64":
            assert K.resize_pad_trips(c.C, c.T) == 2
            img = R.label_image(c.C, c.H, c.W, K.LABEL_VALUES)
            got = resize_pad(lib, img, c, mode, elem=1, what=what)
            want = R.resize_pad_f32(img, c, mode)
        else:
            assert K.resize_pad_trips(c.C, c.T) == 2
            img = R.dense_image("signed", c.C, c.H, c.W)
            got = resize_pad(lib, img, c, mode, what=what)
            want = R.resize_pad_f32(img, c, mode)
        padding_is_plus_zero(got, c, what)
        if c.entry == "resize_pad_i64":
            assert_identical(got, t64(want), what)
        else:
            assert_same_bits(got, t64(want), what)
        record(f"{c.entry} mode{mode} exact wrap", 0.0, cid)


@pytest.mark.parametrize("mode", [0, 1], ids=["bilinear", "nearest"])
def test_grid_stride_wrap_predict_mask(lib, mode):
    c, C = K.WRAP_PREDICT, K.WRAP_PREDICT_C
    assert K.predict_mask_trips(c.oh, c.ow) == 2
    slot = R.logits_slot(C, c.T, key="wrap")
    mask, _ = predict_mask(lib, dev(slot), C, c, mode, f"predict_mask wrap mode {mode}")
    want = R.predict_mask_ref(slot, c, mode)[0]
    assert torch.equal(mask, t64(want)), f"predict_mask wrap mode {mode}: {int((mask != t64(want)).sum())} of {mask.numel()} pixels differ"
    record(f"predict_mask mode{mode} wrap", 0.0, K.rev_id(c))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_a_window_past_the_far_edge_is_refused(lib):
    """only the entries' own argument checks, before any launch: the outputs keep their pattern"""
    far = [c for c in FWD_CASES if K.flush_far(c)]
    assert len(far) >= 5
    for c in far:
        img, pic = dev(R.dense_image("dense01", 1, c.H, c.W)), dev(R.u8_image(c, 1))
        slot = torch.zeros((1, c.T, c.T), device="cuda")
        out, small, mask = nan_buffer(c.T * c.T, "fp32"), nan_buffer(c.H * c.W, "fp32"), nan_buffer(c.H * c.W, "u8")
        for dt, dl in ((1, 0), (0, 1)):
            if (dt and c.pt + c.nh != c.T) or (dl and c.pl + c.nw != c.T):
                continue
            pt, pl = c.pt + dt, c.pl + dl
            assert not K.window_ok(c._replace(pt=pt, pl=pl))
            with pytest.raises(RuntimeError, match="resize_pad: window outside the target"):
                lib.call("segk_resize_pad", ptr(img), ptr(out), 1, c.H, c.W, c.nh, c.nw, c.T, pt, pl, 2, 0, stream())
            with pytest.raises(RuntimeError, match="resize_pad: window outside the target"):
                lib.call("segk_resize_pad_flip", ptr(img), ptr(out), 1, c.H, c.W, c.nh, c.nw, c.T, pt, pl, 2, 0, 3, stream())
            with pytest.raises(RuntimeError, match="resize_pad_u8: window outside the target"):
                lib.call("segk_resize_pad_u8", ptr(pic), ptr(out), 1, c.H, c.W, c.nh, c.nw, c.T, pt, pl, 2, stream())
            with pytest.raises(RuntimeError, match="resize_pad_u8: window outside the target"):
                lib.call("segk_resize_pad_u8_flip", ptr(pic), ptr(out), 1, c.H, c.W, c.nh, c.nw, c.T, pt, pl, 2, 1, stream())
            with pytest.raises(RuntimeError, match="crop_resize: window outside the slot"):
                lib.call("segk_crop_resize", ptr(slot), ptr(small), 1, c.T, pt, pl, c.nh, c.nw, c.H, c.W, 0, stream())
            with pytest.raises(RuntimeError, match="predict_mask: window outside the slot"):
                lib.call("segk_predict_mask", ptr(slot), ptr(mask), 0, 0, 0, 0, 0, 1, c.T, pt, pl, c.nh, c.nw, c.H, c.W, 0, stream())
        sync("window refusals")
        assert bool((out.cpu() == NAN_BITS["fp32"]).all()) and bool((small.cpu() == NAN_BITS["fp32"]).all()) and bool((mask.cpu() == NAN_BITS["u8"]).all())
