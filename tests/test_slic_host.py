"""CPU: proofs about the case table of DESIGN.md 3.24 (tests/slic_cases.py) on the restatement (tests/slic_reference.py) --
that it holds the situations the kernels can get wrong, and that snapping does what it is for on clean edges; the integer
colour transform over all 2^24 colours; every refusal of image_segmentation_amd.superpixels, which has no CPU path; the
header's macros against the binding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_reference as BR                                                    # noqa: E402
import slic_cases as SC                                                            # noqa: E402
import slic_reference as R                                                         # noqa: E402


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_holds_the_shapes_the_kernel_can_get_wrong():
    shapes = {c.image.shape[:2] for c in SC.CASES}
    assert {(1, 1), (1, 7), (5, 3), (33, 65), (65, 129), (SC.TS, SC.TS)} <= shapes
    assert {c.image.shape[2] for c in SC.CASES if c.image.shape[:2] == (SC.TS, SC.TS)} == {1, 3, 4}
    assert {c.step for c in SC.CASES} >= {R.MIN_STEP, R.MAX_STEP} and {c.space for c in SC.CASES} == set(R.SPACES)
    assert {c.iterations for c in SC.CASES} >= {1, 10} and {c.compactness for c in SC.CASES} >= {1, 255}
    assert any(c.step > max(c.image.shape[:2]) and max(c.image.shape[:2]) > 8 for c in SC.CASES)
    for name in ("1x1", "1x7", "5x3", "33x40-step64"):
        assert SC.grid_k(SC.BY_NAME[name]) == 1
    assert any((3 * c.image.shape[1]) % 4 and c.image.shape[2] == 3 for c in SC.CASES)        # rows off the 4-byte grid
    for c in SC.CASES:
        lab, cen, n = SC.expected(c)
        K = SC.grid_k(c)
        assert lab.dtype == np.int32 and lab.min() >= 0 and lab.max() < K and cen.shape == (K, 5) and n.shape == (K,)
        assert np.array_equal(np.bincount(lab.ravel(), minlength=K), n) and int(n.sum()) == lab.size


def test_the_table_holds_an_empty_cluster():
    lab, cen, n = SC.expected(SC.BY_NAME["emptied"])
    assert (n == 0).any() and (n > 0).any()
    # ... that kept the centre it had when it last owned a pixel: it differs from its start centre or equals it, but is a centre
    f = R.features(SC.BY_NAME["emptied"].image, "rgb")
    start = R.start_centres(f, 4)
    k = int(np.flatnonzero(n == 0)[0])
    lab1 = R.assign(f, start, 4, 1)
    assert (lab1 == k).any(), "the cluster owns its seed pixel in the first round: it was emptied later"


def _tied_or_short(case):
    f = R.features(case.image, case.space)
    cen = R.start_centres(f, case.step)
    Ds, valids = [], []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            D, _, valid = R.distances(f, cen, case.step, case.compactness, di, dj)
            Ds.append(np.where(valid, D, np.iinfo(np.int64).max))
            valids.append(valid)
    Ds, n_valid = np.stack(Ds), np.stack(valids).sum(0)
    tied = (Ds == Ds.min(0)).sum(0) > 1
    return tied, n_valid


def test_the_table_holds_a_lowest_index_tie_and_a_pixel_with_fewer_than_nine_candidates():
    case = SC.BY_NAME["65x129-constant"]
    tied, n_valid = _tied_or_short(case)
    assert tied.any() and (n_valid < 9).any() and (n_valid == 9).any() and n_valid.min() == 4
    # the tie goes to the lowest index: the pixel midway between two seeds of a row belongs to the left one
    lab = SC.expected(case)[0]
    S = case.step
    ny, nx = R.grid_of(*case.image.shape[:2], S)
    y, x = S // 2, S // 2 + S // 2 + S                      # as far from the seed of cell (0, 1) as from that of (0, 2)
    assert tied[y, x] and lab[y, x] == 1
    assert n_valid[0, 0] == 4 and _tied_or_short(SC.BY_NAME["1x1"])[1][0, 0] == 1


def test_the_table_holds_a_share_test_that_passes_with_equality():
    case = SC.SNAP_BY_NAME["share-equal"]
    out, hist, win = SC.snap_expected(case)
    assert hist[0].tolist() == [0, 0, 8, 0, 0, 8, 0, 0] and 256 * 8 == case.min_share * int(hist[0].sum())
    assert win.tolist() == [2, 2] and (out == 2).all()                             # the lowest class of the tie, painted
    out2, _, win2 = SC.snap_expected(SC.SNAP_BY_NAME["share-just-missed"])
    assert win2.tolist() == [2, 2] and np.array_equal(out2, case.mask)             # one 256th more: nothing is painted


def test_the_snap_cases_hold_what_they_are_for():
    names = set(SC.SNAP_BY_NAME)
    assert {"slic-share0", "slic-share128", "slic-share256"} <= names
    assert {c.min_share for c in SC.SNAP_CASES} >= {0, 128, 256}
    c = SC.SNAP_BY_NAME["slic-weighted"]
    assert (c.weights == 0).any() and (c.weights == 255).any()
    c = SC.SNAP_BY_NAME["slic-void-band"]
    out, hist, win = SC.snap_expected(c)
    assert c.fill == (255,) and (c.mask == 255).any() and (c.mask == 3).any() and 3 not in c.classes
    assert (out[c.mask == 255] != 255).any(), "void pixels are filled from their segment"
    assert (out[c.mask == 3] == 3).all() and hist[:, 3].sum() == 0, "a class outside `classes` neither votes nor changes"
    out, _, _ = SC.snap_expected(SC.SNAP_BY_NAME["slic-void-band-nofill"])
    assert np.array_equal(out == 255, SC.SNAP_BY_NAME["slic-void-band-nofill"].mask == 255)
    c = SC.SNAP_BY_NAME["labels-outside"]
    out, hist, win = SC.snap_expected(c)
    outside = (c.labels < 0) | (c.labels >= c.k)
    assert (c.labels == -1).any() and (c.labels >= c.k).any() and np.array_equal(out[outside], c.mask[outside])
    assert (out != c.mask).any()
    c = SC.SNAP_BY_NAME["blocks"]
    assert (SC.snap_expected(c)[2] == -1).any()                                    # ids nobody holds have no winner
    c = SC.SNAP_BY_NAME["pixel-segments"]
    assert c.k > 2048 and np.array_equal(SC.snap_expected(c)[0], c.mask)           # one vote each: the winner is the pixel's own


# ------------------------------------------------------------------------------------------------ the colour transform
def test_ycc_stays_in_a_byte_over_all_colours():
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    lo, hi = 255, 0
    raw_lo, raw_hi = 0, 0
    for r in range(256):
        img = np.stack([np.full_like(g, r), g, b], axis=-1)
        f = R.features(img, "ycc")
        lo, hi = min(lo, int(f.min())), max(hi, int(f.max()))
        R_, G_, B_ = (img[..., a].astype(np.int64) for a in range(3))
        cb = ((-43 * R_ - 85 * G_ + 128 * B_ + 128) >> 8) + 128
        cr = ((128 * R_ - 107 * G_ - 21 * B_ + 128) >> 8) + 128
        raw_lo, raw_hi = min(raw_lo, int(cb.min()), int(cr.min())), max(raw_hi, int(cb.max()), int(cr.max()))
    assert (lo, hi) == (0, 255)
    assert raw_lo == 0 and raw_hi == 256, "the chroma reaches 256 before the clamp: the clamp is part of the definition"
    grey = np.stack([g, g, g], axis=-1)
    f = R.features(grey, "ycc")
    assert np.array_equal(f[..., 0], g) and (f[..., 1:] == 128).all()              # 77 + 150 + 29 = 256: grey keeps its luma


def test_grey_has_one_feature_in_either_space():
    img = SC.noise(9, 11, 1, 3)
    assert np.array_equal(R.features(img, "ycc"), R.features(img, "rgb"))
    assert (R.features(img, "ycc")[..., 1:] == 0).all()
    rgba = SC.noise(9, 11, 4, 3)
    assert np.array_equal(R.features(rgba, "ycc"), R.features(rgba[..., :3].copy(), "ycc"))


# ------------------------------------------------------------------------------------------------ what snapping is for
@pytest.mark.parametrize("kind", ["straight", "diagonal"])
def test_snapping_a_shifted_mask_gives_back_the_true_mask_and_raises_boundary_iou(kind):
    case = SC.BY_NAME[kind]
    assert case.compactness == 1
    image, true = SC.TWO_TONE[kind]
    lab = SC.expected(case)[0]
    moved = SC.shifted(true, 2)
    assert (moved != true).sum() > 0
    out, _, _ = R.snap(lab, moved, SC.grid_k(case), None, range(8), (), R.share_of(0.5))
    assert np.array_equal(out, true)
    for width in (1, 2, 3):
        before = BR.quality(BR.boundary_stats(moved, true, 2, width=width), 2)["mean_boundary_iou"]
        after = BR.quality(BR.boundary_stats(out, true, 2, width=width), 2)["mean_boundary_iou"]
        assert after > before and after == 1.0


# ------------------------------------------------------------------------------------------------ the public layer
def test_min_share_is_rounded_once_on_the_host():
    import importlib
    SP = importlib.import_module("image_segmentation_amd.superpixels")             # seg.superpixels is the function
    for f, want in ((0, 0), (0.0, 0), (1, 256), (1.0, 256), (0.5, 128), (0.6, 154), (0.001, 0), (0.002, 1), (0.998, 255), (0.9981, 256),
                    (np.float32(0.25), 64)):
        assert SP.share_of(f) == want == R.share_of(f), f
    for bad in (-0.01, 1.01, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="min_share"):
            SP.share_of(bad)


def test_the_tile_height_follows_the_image_size():
    import importlib
    from image_segmentation_amd import _lib
    SP = importlib.import_module("image_segmentation_amd.superpixels")
    assert _lib.SLIC_TILE_ROWS == (_lib.SLIC_TILE, 16, 4)
    groups = lambda H, W, rows: -(-H // rows) * -(-W // 64)
    for H, W, want in ((1, 1, 4), (256, 256, 4), (1024, 1024, 16), (1023, 1024, 16), (1008, 1024, 4), (2048, 2048, 64), (3000, 4000, 64),
                       (1984, 2048, 16), (1 << 20, 1, 64), (1, 1 << 20, 64), (4096, 64, 4), (16384, 64, 16), (65536, 64, 64)):
        assert SP.tile_rows(H, W) == want, (H, W)
        assert want == 4 or groups(H, W, want) >= 1024
        assert all(groups(H, W, taller) < 1024 for taller in _lib.SLIC_TILE_ROWS if taller > want)


def test_superpixels_refusals():
    import image_segmentation_amd as seg
    img = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        seg.superpixels(img)
    with pytest.raises(ValueError, match=r"uint8 \[H,W,C\]"):
        seg.superpixels(torch.zeros((3, 8, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match=r"uint8 \[H,W,C\]"):
        seg.superpixels(np.zeros((8, 8, 3), dtype=np.uint8))
    for shape in ((8, 8, 2), (8, 8, 5), (2, 8, 8, 3), (8,), (0, 8, 3)):
        with pytest.raises(ValueError, match="1, 3 or 4 channels"):
            seg.superpixels(torch.zeros(shape, dtype=torch.uint8))
    for kw, what in ((dict(step=3), "step"), (dict(step=65), "step"), (dict(step=True), "step"), (dict(step=16.0), "step"),
                     (dict(compactness=0), "compactness"), (dict(compactness=256), "compactness"), (dict(compactness=False), "compactness"),
                     (dict(iterations=0), "iterations"), (dict(iterations=21), "iterations"), (dict(iterations=True), "iterations"),
                     (dict(space="lab"), "space"), (dict(space=1), "space")):
        with pytest.raises(ValueError, match=what):
            seg.superpixels(img, **kw)


def test_snap_mask_refusals():
    import image_segmentation_amd as seg
    mask = torch.zeros((8, 8), dtype=torch.uint8)
    lab = torch.zeros((8, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU path"):
        seg.snap_mask(mask, lab, k=1)
    with pytest.raises(ValueError, match="k="):
        seg.snap_mask(mask, lab)
    for k in (0, True, 1.0, (1 << 28) + 1):
        with pytest.raises(ValueError, match="k:"):
            seg.snap_mask(mask, lab, k=k)
    with pytest.raises(ValueError, match=r"uint8 \[H,W\] mask"):
        seg.snap_mask(mask.float(), lab, k=1)
    with pytest.raises(ValueError, match=r"uint8 \[H,W\] mask"):
        seg.snap_mask(mask[None], lab, k=1)
    with pytest.raises(ValueError, match="int32"):
        seg.snap_mask(mask, lab.long(), k=1)
    with pytest.raises(ValueError, match="int32"):
        seg.snap_mask(mask, [[0]], k=1)
    with pytest.raises(ValueError, match="the label map is"):
        seg.snap_mask(mask, torch.zeros((8, 9), dtype=torch.int32), k=1)
    with pytest.raises(ValueError, match="weights"):
        seg.snap_mask(mask, lab, k=1, weights=torch.zeros((8, 8)))
    with pytest.raises(ValueError, match="weights"):
        seg.snap_mask(mask, lab, k=1, weights=torch.zeros((8, 7), dtype=torch.uint8))
    with pytest.raises(ValueError, match="fill: 2 is one of the classes"):
        seg.snap_mask(mask, lab, k=1, classes=(1, 2), fill=(2, 255))
    with pytest.raises(ValueError, match="fill: 7 is one of the classes"):
        seg.snap_mask(mask, lab, k=1, fill=(7,))                                   # the default is all eight
    for classes in ((8,), (), 3, "12", (True,), (1, 256)):
        with pytest.raises(ValueError, match="classes"):
            seg.snap_mask(mask, lab, k=1, classes=classes)
    for fill in (255, (256,), (-1,), None):
        with pytest.raises(ValueError, match="fill"):
            seg.snap_mask(mask, lab, k=1, fill=fill)
    with pytest.raises(ValueError, match="min_share"):
        seg.snap_mask(mask, lab, k=1, min_share=1.5)
    sp = seg.Superpixels(lab, None, None, (1, 1), 8, 1)
    with pytest.raises(ValueError, match="k:"):
        seg.snap_mask(mask, sp, k=2)
    with pytest.raises(ValueError, match="no CPU path"):
        seg.snap_mask(mask, sp)


def test_segmenter_snap_refusals():
    import image_segmentation_amd as seg
    model = torch.nn.Conv2d(3, 4, 1)
    for snap, what in ((dict(step=2), "step"), (dict(min_share=2), "min_share"), (dict(radius=3), "snap"), ([16], "snap"),
                       (dict(weighted=1), "weighted"), (dict(classes=(1,), fill=(1,)), "fill"), (dict(space="hsv"), "space")):
        with pytest.raises(ValueError, match=what):
            seg.Segmenter(model, snap=snap)
    with pytest.raises(ValueError, match="weighted=True"):
        seg.Segmenter(model, snap=dict(weighted=True))                             # the plain route writes no confidence map
    s = seg.Segmenter(model, snap=dict(step=8, min_share=0.6, weighted=True), tta=dict(flips=("", "h")))
    assert s.snap == seg.Snap(step=8, min_share=0.6, weighted=True) and s.snap._plan[2] == 154
    assert seg.Segmenter(model, snap=dict(weighted=True), tiles=dict(size=32)).snap.weighted
    assert seg.Segmenter(model).snap is None
    # a float image is refused before the forward (the model is on the host: the device check would come next)
    with pytest.raises(ValueError, match="uint8"):
        seg.Segmenter(model, snap=dict(step=8))([torch.zeros((3, 16, 16))])
    assert seg.Prediction(None, None, None, None, {}).superpixels is None


def test_header_macros_match_the_binding():
    from image_segmentation_amd import _lib
    for macro, value in (("SEGK_SLIC_TILE", _lib.SLIC_TILE), ("SEGK_SLIC_MAX_CELLS", _lib.SLIC_MAX_CELLS),
                         ("SEGK_SLIC_MIN_STEP", _lib.SLIC_MIN_STEP), ("SEGK_SLIC_MAX_STEP", _lib.SLIC_MAX_STEP),
                         ("SEGK_SLIC_MAX_COMPACTNESS", _lib.SLIC_MAX_COMPACTNESS), ("SEGK_SLIC_MAX_ITERATIONS", _lib.SLIC_MAX_ITERATIONS),
                         ("SEGK_SLIC_RGB", _lib.SLIC_SPACES["rgb"]), ("SEGK_SLIC_YCC", _lib.SLIC_SPACES["ycc"]),
                         ("SEGK_SLIC_CENTRE_WORDS", _lib.SLIC_CENTRE_WORDS), ("SEGK_SLIC_SUM_WORDS", _lib.SLIC_SUM_WORDS),
                         ("SEGK_SNAP_NONE", _lib.SNAP_NONE)):
        assert SC.macro(macro) == value, macro
    assert (R.MIN_STEP, R.MAX_STEP, R.MAX_COMPACTNESS, R.MAX_ITERATIONS) == (_lib.SLIC_MIN_STEP, _lib.SLIC_MAX_STEP,
                                                                             _lib.SLIC_MAX_COMPACTNESS, _lib.SLIC_MAX_ITERATIONS)
    # a tile and its ring never touch more cells than the staged table holds
    for S in range(_lib.SLIC_MIN_STEP, _lib.SLIC_MAX_STEP + 1):
        for t0 in range(0, 64 * 70, 64):
            assert (t0 + 63) // S - t0 // S + 3 <= _lib.SLIC_MAX_CELLS, (S, t0)


def test_c_entries_refuse_before_any_launch():
    import ctypes
    from image_segmentation_amd import _lib
    lib = _lib.load()
    err = lambda: lib.segk_last_error().decode()
    p = 4096
    ok = dict(C=3, space=1, S=8, H=16, W=24, K=6)
    start = lambda image=p, cen=p, sums=p, **kw: lib.segk_slic_start(image, cen, sums, *[{**ok, **kw}[k] for k in ("C", "space", "S", "H", "W", "K")], None)
    for kw, word in ((dict(image=None), "NULL"), (dict(cen=None), "NULL"), (dict(sums=None), "NULL"), (dict(C=2), "C 2"),
                     (dict(space=2), "space"), (dict(S=3), "step"), (dict(S=65), "step"), (dict(H=0), "shape"), (dict(W=-1), "shape"),
                     (dict(K=5), "grid"), (dict(K=7), "grid"), (dict(cen=p + 2), "aligned"), (dict(sums=p + 8), "aligned"),
                     (dict(H=1 << 15, W=1 << 14, K=0), "2^28"), (dict(H=(1 << 27) + 1, W=1, K=1), "sides")):
        assert start(**kw) == -2 and word in err(), (kw, err())
    okA = dict(ok, m=20, round=0, T=10, rows=64)
    assign = lambda image=p, cen=p, sums=2 * p, lab=3 * p, **kw: lib.segk_slic_assign(
        image, cen, sums, lab, *[{**okA, **kw}[k] for k in ("C", "space", "S", "m", "round", "T", "rows", "H", "W", "K")], None)
    for kw, word in ((dict(lab=None), "NULL"), (dict(m=0), "compactness"), (dict(m=256), "compactness"), (dict(T=0), "iterations"),
                     (dict(rows=0), "tile_rows"), (dict(rows=8), "tile_rows"), (dict(rows=128), "tile_rows"),
                     (dict(T=21), "iterations"), (dict(round=10), "round"), (dict(round=-1), "round"), (dict(C=5), "C 5"),
                     (dict(K=1), "grid"), (dict(lab=3 * p + 1), "aligned"), (dict(lab=p), "distinct"), (dict(sums=p), "distinct"),
                     (dict(S=2), "step"), (dict(space=-1), "space")):
        assert assign(**kw) == -2 and word in err(), (kw, err())
    update = lambda cen=p, sums=2 * p, cnt=3 * p, **kw: lib.segk_slic_update(cen, sums, cnt, *[{**ok, **kw}[k] for k in ("S", "H", "W", "K")], None)
    for kw, word in ((dict(cnt=None), "NULL"), (dict(S=100), "step"), (dict(K=600), "grid"), (dict(sums=2 * p + 4), "aligned"),
                     (dict(cnt=p), "distinct")):
        assert update(**kw) == -2 and word in err(), (kw, err())
    vote = lambda lab=p, mask=2 * p, w=None, hist=3 * p, bits=255, rows=16, H=16, W=24, K=6: lib.segk_snap_vote(lab, mask, w, hist, bits, rows,
                                                                                                          H, W, K, None)
    for kw, word in ((dict(lab=None), "NULL"), (dict(hist=None), "NULL"), (dict(bits=0), "classes_mask"), (dict(bits=256), "classes_mask"),
                     (dict(rows=5), "tile_rows"), (dict(rows=-4), "tile_rows"),
                     (dict(H=0), "shape"), (dict(K=0), "K 0"), (dict(K=(1 << 28) + 1), "K "), (dict(lab=p + 2), "aligned"),
                     (dict(hist=3 * p + 4), "aligned"), (dict(H=1 << 15, W=1 << 14), "2^28")):
        assert vote(**kw) == -2 and word in err(), (kw, err())
    paint = lambda lab=p, mask=2 * p, hist=3 * p, win=4 * p, pt=5 * p, out=6 * p, share=128, H=16, W=24, K=6: lib.segk_snap_paint(
        lab, mask, hist, win, pt, out, ctypes.c_long(255), ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(-1), share, H, W, K, None)
    for kw, word in ((dict(out=None), "NULL"), (dict(pt=None), "NULL"), (dict(share=-1), "min_share"), (dict(share=257), "min_share"),
                     (dict(out=2 * p), "neither"), (dict(out=5 * p), "neither"), (dict(W=0), "shape"), (dict(K=-3), "K -3"),
                     (dict(win=4 * p + 2), "aligned"), (dict(hist=3 * p + 1), "aligned")):
        assert paint(**kw) == -2 and word in err(), (kw, err())
