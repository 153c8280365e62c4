"""CPU: the restatement of DESIGN.md 3.21 (tests/morph_reference.py) against scipy.ndimage where it is installed, against
hand-written cases and its own algebra; the numerical check of the kernel's two-pass argument; every refusal of
image_segmentation_amd.morph, which has no CPU path; the header's macros against the binding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases as MC                                                           # noqa: E402
import morph_reference as R                                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [c.name for c in MC.CASES]


def u8(rows):
    return np.asarray(rows, dtype=np.uint8)


def element(shape, r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return {"square": np.maximum(abs(yy), abs(xx)) <= r, "diamond": abs(yy) + abs(xx) <= r, "disk": yy * yy + xx * xx <= r * r}[shape]


# ------------------------------------------------------------------------------------------------ hand-written
def test_erode_and_dilate_5x5():
    m = u8([[0, 0, 0, 0, 0],
            [0, 1, 1, 1, 0],
            [0, 1, 1, 1, 0],
            [0, 1, 1, 1, 0],
            [0, 0, 0, 0, 0]])
    e = R.erode(m, (1,), 1, 0, "square")
    assert e.sum() == 1 and e[2, 2] == 1
    assert np.array_equal(R.dilate(e, (1,), 1, shape="square"), m)
    assert R.dilate(e, (1,), 1, shape="diamond").tolist() == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0],
                                                                  [0, 0, 0, 0, 0]]
    assert np.array_equal(R.dilate(e, (1,), 1, shape="disk"), R.dilate(e, (1,), 1, shape="diamond"))      # r = 1: the same element
    full = np.ones((5, 5), dtype=np.uint8)
    assert np.array_equal(R.erode(full, (1,), 2, 0), full)                 # nothing erodes from the image border
    assert (R.boundary_distance(full, 2) == R.FAR).all()


def test_open_removes_a_spur_and_close_a_crack_5x5():
    m = u8([[0, 0, 0, 0, 0],
            [1, 1, 1, 0, 0],
            [1, 1, 1, 1, 1],
            [1, 1, 1, 0, 0],
            [0, 0, 0, 0, 0]])
    o = R.open_mask(m, (1,), 1, 0, "square")
    assert o.tolist() == [[0, 0, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [0, 0, 0, 0, 0]]
    c = u8([[1, 1, 0, 1, 1]] * 5)
    assert (R.close_mask(c, (1,), 1, shape="square") == 1).all()
    two = u8([[2, 2, 2, 0, 0],
              [2, 1, 1, 0, 0],
              [2, 1, 1, 3, 3],
              [2, 2, 2, 0, 0],
              [2, 2, 2, 0, 0]])
    o = R.open_mask(two, (1, 2), 1, 0, "square")                          # a two-class set: every pixel gets its own value back
    assert o.tolist() == [[2, 2, 2, 0, 0], [2, 1, 1, 0, 0], [2, 1, 1, 3, 3], [2, 2, 2, 0, 0], [2, 2, 2, 0, 0]]


def test_band_distance_and_skip_5x5():
    m = u8([[0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0],
            [0, 0, 5, 0, 0],
            [0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0]])
    d = R.boundary_distance(m, 2, shape="disk")
    assert d.tolist() == [[R.FAR, R.FAR, 4, R.FAR, R.FAR], [R.FAR, 2, 1, 2, R.FAR], [4, 1, 1, 1, 4], [R.FAR, 2, 1, 2, R.FAR],
                          [R.FAR, R.FAR, 4, R.FAR, R.FAR]]
    assert R.boundary_distance(m, 2, shape="square")[0].tolist() == [2] * 5
    assert R.boundary_distance(m, 2, shape="diamond")[0].tolist() == [R.FAR, R.FAR, 2, R.FAR, R.FAR]
    b = R.label_band(m, 1, value=255, shape="diamond")
    assert (b == 255).sum() == 5 and b[2, 2] == 255 and b[0, 0] == 0
    assert np.array_equal(R.label_band(m, 1, skip=(5,)), m)               # a skipped value differs from nothing
    assert (R.boundary_distance(m, 2, skip=(5,)) == R.FAR).all()
    b = R.label_band(m, 1, classes=(0,), shape="diamond")
    assert b[2, 2] == 5 and (b == 255).sum() == 4


def test_disk_offsets_3_4_fire_and_4_4_do_not_at_r5():
    m = np.zeros((12, 12), dtype=np.uint8)
    m[1, 1] = 1
    d = R.boundary_distance(m, 5, shape="disk")
    assert d[4, 5] == 25 and d[5, 4] == 25 and d[1, 6] == 25 and d[5, 5] == R.FAR and d[1, 7] == R.FAR
    assert R.dilate(m, (1,), 5)[4, 5] == 1 and R.dilate(m, (1,), 5)[5, 5] == 0
    assert R.boundary_distance(m, 5, shape="square")[5, 5] == 4 and R.boundary_distance(m, 5, shape="diamond")[5, 5] == R.FAR


def test_fill_holes_by_hand():
    m = u8([[0, 0, 1, 0, 0],
            [0, 1, 0, 1, 0],
            [0, 0, 1, 0, 0]])
    out, num, filled = R.fill_holes(m, (1,))                # at 4 the outside falls in two and the centre is a hole
    assert (num, filled) == (3, 1) and out[1, 2] == 1 and (out != m).sum() == 1
    out8, num8, filled8 = R.fill_holes(m, (1,), connectivity=8)            # at 8 it joins the outside
    assert (num8, filled8) == (1, 0) and np.array_equal(out8, m)
    assert R.fill_holes(m, (1,), max_area=0)[2] == 0
    assert R.fill_holes(m, (1,), max_components=2)[2] == 0  # the hole is component 3 in raster order: it has no row and stays
    assert R.fill_holes(m, (1,), max_components=3)[2] == 1
    assert R.fill_holes(m, (1,), value=9)[0][1, 2] == 9


# ------------------------------------------------------------------------------------------------ scipy
@pytest.mark.parametrize("case", MC.CASES, ids=CASE_IDS)
def test_restatement_equals_scipy(case):
    ndi = pytest.importorskip("scipy.ndimage")
    m = case.mask
    S = R.byte_set(case.classes)[m]
    for shape in MC.SHAPES:
        for r in case.radii:
            el = element(shape, r)
            value = R._single(case.classes, case.value, "case")
            er = ndi.binary_erosion(S, el, border_value=1)
            di = ndi.binary_dilation(S, el)
            e = R.erode(m, case.classes, r, case.fill, shape)
            d = R.dilate(m, case.classes, r, value, None, shape)
            assert np.array_equal(R.byte_set(case.classes)[e], er), (shape, r)
            assert np.array_equal(R.byte_set(case.classes)[d], di), (shape, r)
            o = R.open_mask(m, case.classes, r, case.fill, shape)
            c = R.close_mask(m, case.classes, r, value, shape)
            assert np.array_equal(R.byte_set(case.classes)[o], ndi.binary_dilation(er, el)), (shape, r)
            assert np.array_equal(R.byte_set(case.classes)[c], ndi.binary_erosion(di, el, border_value=1)), (shape, r)
            assert np.array_equal(o[R.byte_set(case.classes)[o]], m[R.byte_set(case.classes)[o]])       # its own value back
            # the capped distance on both sides of the set
            D = R.boundary_distance(m, r, classes=case.classes, shape=shape).astype(np.int64)
            if S.all() or not S.any():
                assert (D == R.FAR).all()
                continue
            if shape == "disk":
                inside, outside = ndi.distance_transform_edt(S), ndi.distance_transform_edt(~S)
                want = np.rint(np.where(S, inside, outside) ** 2).astype(np.int64)
            else:
                met = "chessboard" if shape == "square" else "taxicab"
                want = np.where(S, ndi.distance_transform_cdt(S, met), ndi.distance_transform_cdt(~S, met)).astype(np.int64)
            want = np.where(want <= R.cap_of(shape, r), want, R.FAR)
            assert np.array_equal(D, want), (shape, r)


UNLIMITED = [h for h in MC.HOLE_CASES if "max_area" not in h.keywords and h.name != "overflow"]       # scipy has neither limit


@pytest.mark.parametrize("hc", UNLIMITED, ids=[h.name for h in UNLIMITED])
def test_fill_holes_equals_scipy(hc):
    ndi = pytest.importorskip("scipy.ndimage")
    kw = dict(hc.keywords)
    S = R.byte_set(kw["classes"])[hc.mask]
    conn = kw.get("connectivity", 4)
    st = ndi.generate_binary_structure(2, 1 if conn == 4 else 2)
    out, num, filled = R.fill_holes(hc.mask, **kw)
    assert np.array_equal(R.byte_set(kw["classes"])[out] | (out == kw.get("value", -1)), ndi.binary_fill_holes(S, st))
    assert num == ndi.label(~S, st)[1]


def test_fill_holes_limits():
    by = {h.name: h for h in MC.HOLE_CASES}
    at, below = R.fill_holes(by["area_at"].mask, **by["area_at"].keywords), R.fill_holes(by["area_below"].mask, **by["area_below"].keywords)
    assert at[2] == below[2] + 2 and at[0][4, 4] == 1 and below[0][4, 4] == 2     # both 5 x 6 holes have 30 pixels
    m4, m8 = R.fill_holes(by["mixed4"].mask, **by["mixed4"].keywords), R.fill_holes(by["mixed8"].mask, **by["mixed8"].keywords)
    assert m4[0][21, 34] == 1 and m8[0][21, 34] == 0                       # the diamond's centre: a hole at 4, outside at 8
    assert m4[0][12, 2] == 0                                               # open to the left border
    assert m4[0][16, 20] == 1 and m4[0][11, 13] == 1                       # nested: the outer hole fills with everything in it
    over, full = R.fill_holes(by["overflow"].mask, **by["overflow"].keywords), R.fill_holes(by["no_overflow"].mask, **by["no_overflow"].keywords)
    assert over[1] == full[1] == 169 and full[2] == 168 and over[2] == 49 and (over[0] == 0).sum() == 169 - 49


# ------------------------------------------------------------------------------------------------ algebra
@pytest.mark.parametrize("case", MC.CASES, ids=CASE_IDS)
def test_algebra(case):
    m, cs = case.mask, case.classes
    S = R.byte_set(cs)
    value = R._single(cs, case.value, "case")
    for shape in MC.SHAPES:
        for r in case.radii:
            o, c = R.open_mask(m, cs, r, case.fill, shape), R.close_mask(m, cs, r, value, shape)
            assert not (S[o] & ~S[m]).any() and not (S[m] & ~S[c]).any()                      # open in S in close
            assert np.array_equal(R.open_mask(o, cs, r, case.fill, shape), o)                 # idempotent
            assert np.array_equal(R.close_mask(c, cs, r, value, shape), c)
            # erosion of the complement is dilation: the same pixels change
            comp = [v for v in range(256) if not S[v]]
            d = R.dilate(m, cs, r, value, None, shape)
            e = R.erode(m, comp, r, value, shape)
            assert np.array_equal(d, e)
            band = R.label_band(m, r, case.band_value, case.band_classes, case.skip, shape)
            D = R.boundary_distance(m, r, None, case.skip, shape)
            C = np.ones(256, dtype=bool) if case.band_classes is None else R.byte_set(case.band_classes)
            assert np.array_equal(band != m, (D != R.FAR) & C[m] & (m != case.band_value))


# ------------------------------------------------------------------------------------------------ the two-pass argument
@pytest.mark.parametrize("case", MC.CASES, ids=CASE_IDS)
def test_two_pass_equals_brute_force(case):
    """DESIGN.md 3.21 "two passes": the column recurrence and the row minimum the kernel uses, restated in NumPy on a crop,
    equal the definition -- for binary keys, for keys = values and with wild cells inside the image"""
    m = np.ascontiguousarray(case.mask[:40, :44])
    keys = [R.set_keys(case.classes), R.value_keys(case.skip)]
    if case.skip:
        k = R.set_keys(case.classes); k[list(case.skip)] = R.WILD
        keys.append(k)
    for key in keys:
        for shape in MC.SHAPES:
            for r in case.radii:
                assert np.array_equal(R.two_pass(m, key, shape, r), R.distance(m, key, shape, r)), (shape, r)


# ------------------------------------------------------------------------------------------------ refusals, ABI
def test_refusals():
    import image_segmentation_amd as seg
    from image_segmentation_amd import morph as M
    m = torch.zeros((4, 4), dtype=torch.uint8)
    bad_plans = [
        lambda: M._erode_plan((1,), 0, 0), lambda: M._erode_plan((1,), 33, 0), lambda: M._erode_plan((1,), True, 0),
        lambda: M._erode_plan((1,), 1.5, 0), lambda: M._erode_plan((1,), 1, 0, shape="cross"), lambda: M._erode_plan((1,), 1, 0, shape=None),
        lambda: M._erode_plan((256,), 1, 0), lambda: M._erode_plan((-1,), 1, 0), lambda: M._erode_plan((True,), 1, 0),
        lambda: M._erode_plan(1, 1, 0), lambda: M._erode_plan((), 1, 0), lambda: M._erode_plan("12", 1, 0),
        lambda: M._erode_plan((1, 2), 1, 2), lambda: M._erode_plan((1,), 1, 256), lambda: M._erode_plan((1,), 1, None),
        lambda: M._dilate_plan((1, 2), 1), lambda: M._dilate_plan((1,), 1, value=300), lambda: M._dilate_plan((1,), 1, into=(1, 0)),
        lambda: M._open_plan((1,), 1, 1), lambda: M._open_plan((1,), 40, 0),
        lambda: M._close_plan((1, 2), 1), lambda: M._close_plan((1, 2), 1, value=0), lambda: M._close_plan((1,), 0),
        lambda: M._band_plan(0), lambda: M._band_plan(1, value=256), lambda: M._band_plan(1, skip=(300,)), lambda: M._band_plan(1, classes=()),
        lambda: M._band_plan(1, shape="round"), lambda: M._distance_plan(33), lambda: M._distance_plan(2, classes=(9.5,)),
        lambda: M._fill_plan((1, 2)), lambda: M._fill_plan((1,), connectivity=6), lambda: M._fill_plan((1,), max_area=-1),
        lambda: M._fill_plan((1,), max_components=0), lambda: M._fill_plan((1,), max_components=True), lambda: M._fill_plan((1,), connectivity=True),
        lambda: M._fill_plan((1,), value=-1),
    ]
    for k, f in enumerate(bad_plans):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"plan {k} was accepted")
    # tensors: all refused before any launch (no GPU here: a launch would raise something else)
    calls = [lambda t: seg.erode(t, (1,), 1, 0), lambda t: seg.dilate(t, (1,), 1), lambda t: seg.open_mask(t, (1,), 1, 0),
             lambda t: seg.close_mask(t, (1,), 1), lambda t: seg.label_band(t, 1), lambda t: seg.boundary_distance(t, 1),
             lambda t: seg.fill_holes(t, (1,))]
    for f in calls:
        for t in (m, m.numpy(), m.float(), m[0], m[None], torch.zeros((0, 4), dtype=torch.uint8)):
            with pytest.raises(ValueError):
                f(t)
    with pytest.raises(ValueError, match="2\\^28"):           # a meta tensor: the shape without its 256 MiB
        seg.erode(torch.empty((1 << 15, (1 << 13) + 1), dtype=torch.uint8, device="meta"), (1,), 1, 0)
    with pytest.raises(ValueError, match="radius"):         # argument errors come before the tensor is looked at
        seg.erode(m, (1,), 99, 0)


def test_morph_steps_and_segmenter_keyword():
    import image_segmentation_amd as seg
    from image_segmentation_amd import morph as M
    steps = M.as_morph([seg.MorphStep("open", classes=(1, 2), radius=2, fill=0), {"op": "fill_holes", "classes": (1,)},
                        dict(op="close", classes=(1,), radius=1, shape="square")])
    assert [s.op for s in steps] == ["open", "fill_holes", "close"] and len(steps[0].plan) == 2
    assert M.as_morph(None) is None and M.as_morph([]) == ()
    for bad in ("open", {"op": "open"}, [{"classes": (1,)}], [("open",)], [{"op": "sharpen"}], [{"op": "open", "classes": (1,), "radius": 2}],
                [{"op": "erode", "classes": (1,), "radius": 2, "fill": 0, "strength": 3}], 7):
        with pytest.raises(ValueError):
            M.as_morph(bad)
    assert "boundary_distance" not in M._OPS                # it returns no mask: not a Segmenter step
    import inspect
    assert inspect.signature(seg.Segmenter.__init__).parameters["morph"].default is None


def test_header_macros_and_binding():
    from image_segmentation_amd import _lib
    assert MC.macro("SEGK_ABI_VERSION") == _lib.ABI_VERSION >= 328 and MC.macro("SEGK_ENTRY_COUNT") == len(_lib.SIGNATURES) >= 116
    assert MC.macro("SEGK_MORPH_MAX_RADIUS") == _lib.MORPH_MAX_RADIUS == R.MAX_RADIUS == 32
    assert (MC.TH, MC.TW) == (_lib.MORPH_TILE_H, _lib.MORPH_TILE_W)
    assert MC.macro("SEGK_MORPH_WILD") == _lib.MORPH_WILD == R.WILD and MC.macro("SEGK_MORPH_FAR") == _lib.MORPH_FAR == R.FAR
    assert [MC.macro("SEGK_MORPH_" + s.upper()) for s in R.SHAPES] == [_lib.MORPH_METRICS[s] for s in R.SHAPES]
    for name in ("segk_morph", "segk_byte_lut", "segk_fill_holes"):
        assert name in _lib.SIGNATURES
    # two workgroups of the largest radius share a CU's 160 KiB of LDS, tables included
    r, th, tw = 32, MC.TH, MC.TW
    assert (th + 2 * r) * (tw + 2 * r) * 2 + th * (tw + 2 * r) + th * tw + 768 <= 80 * 1024
