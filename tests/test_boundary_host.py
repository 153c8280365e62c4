"""CPU: the restatement of DESIGN.md 3.23 (tests/boundary_reference.py) against scipy.ndimage where it is installed and
against its own algebra; quality_from_boundary_stats on hand-made integers; every refusal of image_segmentation_amd.boundary,
which has no CPU path; the header's macros against the binding."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_cases as BC                                                        # noqa: E402
import boundary_reference as R                                                     # noqa: E402

SCIPY_CASES = [c for c in BC.CASES if c.name in ("one_tile", "tiles_plus_1", "eight_classes", "noise", "one_row", "int64_label",
                                                 "contour_on_tile_rows", "smaller_than_the_band")]


# ------------------------------------------------------------------------------------------------ against scipy
@pytest.mark.parametrize("case", SCIPY_CASES, ids=[c.name for c in SCIPY_CASES])
def test_published_band_equals_scipy_erosion(case):
    """shape="square", image_border=True is G & ~erode(G, 3 x 3, d iterations, zero border) -- the published Boundary IoU --
    where nothing is void; void pixels differ from nothing, which scipy states as eroding the mask united with the void"""
    ndi = pytest.importorskip("scipy.ndimage")
    P, G = R.class_maps(case.pred, case.label, case.C, case.ignore)
    sq = np.ones((3, 3), dtype=bool)
    for M in (G, P):
        for d in (1, 2, 7):
            band = R.band_mask(M, case.C, d, "square", True)
            for c in range(case.C):
                A = M == c
                grown = A | (M == R.VOID)
                want = A & ~ndi.binary_erosion(grown, sq, iterations=d, border_value=0)
                assert np.array_equal(band & A, want), (d, c)


@pytest.mark.parametrize("case", SCIPY_CASES, ids=[c.name for c in SCIPY_CASES])
def test_contour_bins_equal_the_ceiling_of_scipy_edt(case):
    ndi = pytest.importorskip("scipy.ndimage")
    P, G = R.class_maps(case.pred, case.label, case.C, case.ignore)
    for c in range(case.C):
        Kg, Kp = R.contour(G, c), R.contour(P, c)
        for src, dst in ((Kp, Kg), (Kg, Kp)):
            got = R.bins_of(src, dst, case.max_distance)
            want = np.zeros(R.BINS, dtype=np.int64)
            if dst.any():
                d2 = np.rint(ndi.distance_transform_edt(~dst) ** 2).astype(np.int64)[src]     # exact: squared integers
                t = np.ceil(np.sqrt(d2.astype(np.float64)) - 1e-9).astype(np.int64)
                assert ((t * t >= d2) & ((t - 1) * (t - 1) < d2) | (d2 == 0)).all()
                np.add.at(want, np.where(t <= case.max_distance, t, case.max_distance + 1), 1)
            else:
                want[case.max_distance + 1] = int(src.sum())
            assert np.array_equal(got, want), c


# ------------------------------------------------------------------------------------------------ the algebra
def test_equal_maps_give_boundary_iou_one_and_all_mass_in_bin_zero():
    for case in BC.CASES:
        lab = np.where((np.asarray(case.label) < 0) | (np.asarray(case.label) > 255), 255, case.label).astype(np.uint8)
        st = R.boundary_stats(lab, case.label, case.C, 2, case.max_distance, case.ignore)
        assert np.array_equal(st["band_g"], st["band_p"]) and np.array_equal(st["band_g"], st["band_i"])
        assert np.array_equal(st["band_conf"], np.diag(st["band_g"]))
        assert st["hist"][:, :, 1:].sum() == 0 and np.array_equal(st["hist"][0], st["hist"][1])
        assert st["hd_sum"].sum() == 0 and st["hd_capped"].sum() == 0
        assert np.array_equal(st["hd_images"], (st["hist"][0, :, 0] > 0).astype(np.int64))
        q = R.quality(st, case.C)
        assert all(v in (None, 1.0) for v in q["boundary_iou"]) and all(v in (None, 0.0) for v in q["hd95"])


@pytest.mark.parametrize("k", [1, 3, 6])
def test_a_map_moved_by_k_columns_puts_the_mass_at_bin_k(k):
    lab = np.zeros((24, 60), dtype=np.uint8)
    lab[:, 20:35] = 1                                      # a full-height bar: its contours are four columns
    pred = np.roll(lab, k, axis=1)
    st = R.boundary_stats(pred, lab, 2, 2, 32)
    for c in (0, 1):
        for d in (0, 1):
            assert st["hist"][d, c, k] == 2 * 24 and st["hist"][d, c].sum() == 2 * 24
    assert st["hd_sum"][:2].tolist() == [k, k] and st["hd_images"][:2].tolist() == [1, 1]


def test_a_constant_map_counts_nothing():
    m = np.full((9, 11), 2, dtype=np.uint8)
    st = R.boundary_stats(m, m, 3, 2, 32, image_border=False)
    assert all(int(v.sum()) == 0 for v in st.values())
    from image_segmentation_amd import quality_from_boundary_stats
    q = quality_from_boundary_stats(**{k: v.tolist() for k, v in st.items()}, num_classes=3)
    for key in ("boundary_iou", "band_iou", "hd95"):
        assert q[key] == [None] * 3
    assert q["mean_boundary_iou"] is None and q["band_accuracy"] is None and q["mean_hd95"] is None
    assert q["contour_f"] == {1: [None] * 3, 2: [None] * 3, 3: [None] * 3} and q["hd95_capped"] == [0, 0, 0]
    # the image border makes a band (every pixel within 2 of it), never a contour
    st = R.boundary_stats(m, m, 3, 2, 32, image_border=True)
    assert st["band_g"][2] == st["band_i"][2] == 9 * 11 - 5 * 7 and st["hist"].sum() == 0


def test_void_differs_from_nothing_and_is_counted_nowhere():
    lab = np.zeros((12, 20), dtype=np.uint8)
    lab[:, 8:12] = 3                                       # an ignored stripe between two halves of class 0 ...
    lab[:, 12:] = 1                                        # ... and class 1
    pred = lab.copy()
    pred[pred == 3] = 0
    pred[0, 0] = 9                                         # >= C: void in the prediction alone
    st = R.boundary_stats(pred, lab, 3, 2, 32, ignore=(3,), image_border=False)
    # across the 4-wide void stripe nothing is within 2: no band; the contours do not see each other through it either
    assert st["band_g"].sum() == 0 and st["band_p"].sum() == 0 and st["hist"].sum() == 0
    st = R.boundary_stats(pred, lab, 3, 5, 32, ignore=(3,), image_border=False)
    assert st["band_g"][:2].tolist() == [12, 12] and st["band_conf"].sum() == 24
    assert st["band_p"][0] == 12 - 0 and st["band_conf"][0, 0] == 12     # (0, 0) is 8 columns from the stripe: not in the band


def test_published_width_and_its_refusal():
    from image_segmentation_amd import boundary as B
    assert B.published_width(10, 10) == 1 == R.published_width(10, 10) and B.published_width(300, 400) == 10
    assert B.published_width(1280, 960) == 32 and B._width_for(None, 1280, 960) == 32
    for H, W in ((1, 1), (64, 128), (200, 300), (1000, 1300)):
        assert B.published_width(H, W) == R.published_width(H, W) == max(1, int(round(0.02 * math.hypot(H, W))))
    with pytest.raises(ValueError, match="width="):
        B._width_for(None, 3000, 4000)


# ------------------------------------------------------------------------------------------------ the host finish
def _stats(**kw):
    st = {k: v.tolist() for k, v in R.empty_stats().items()}
    for k, v in kw.items():
        st[k] = v
    return st


def test_quality_from_hand_made_integers():
    from image_segmentation_amd import quality_from_boundary_stats as Q
    st = _stats()
    st["band_g"][:2], st["band_p"][:2], st["band_i"][:2] = [10, 0], [6, 0], [4, 0]
    st["band_conf"][0][:2], st["band_conf"][1][:2] = [6, 2], [1, 3]
    st["hist"][0][0][:4] = [2, 1, 1, 0]
    st["hist"][0][0][33] = 4                               # overflow: never within a tolerance
    st["hist"][1][0][:4] = [1, 0, 3, 0]
    st["hd_sum"][0], st["hd_images"][0], st["hd_capped"][0] = 7, 2, 3
    q = Q(**st, num_classes=2, tolerances=(0, 1, 2), images=5)
    assert q["boundary_iou"] == [4 / 12, None] and q["mean_boundary_iou"] == 4 / 12
    assert q["band_iou"] == [6 / (8 + 7 - 6), 3 / (4 + 5 - 3)] and q["band_accuracy"] == 9 / 12
    assert q["mean_band_iou"] == (6 / 9 + 3 / 6) / 2
    assert q["contour_precision"] == {0: [2 / 8, None], 1: [3 / 8, None], 2: [4 / 8, None]}
    assert q["contour_recall"] == {0: [1 / 4, None], 1: [1 / 4, None], 2: [1.0, None]}
    p, r = 4 / 8, 1.0
    assert q["contour_f"][2] == [2 * p * r / (p + r), None] and q["mean_contour_f"][2] == 2 * p * r / (p + r)
    assert q["hd95"] == [3.5, None] and q["hd95_capped"] == [3, 0] and q["hd95_images"] == [2, 0] and q["mean_hd95"] == 3.5
    assert q["images"] == 5 and q["tolerances"] == [0, 1, 2] and q["max_distance"] == 32
    import json
    json.dumps(q)
    # one side without a contour pixel: F is 0, not None; a smaller cap moves the overflow bin
    st = _stats()
    st["hist"][0][1][6] = 5                                # max_distance 5: its overflow bin
    q = Q(**st, num_classes=2, tolerances=(5,), max_distance=5)
    assert q["contour_precision"][5] == [None, 0.0] and q["contour_recall"][5] == [None, None] and q["contour_f"][5] == [None, 0.0]
    for bad in (dict(num_classes=0), dict(num_classes=9), dict(num_classes=True), dict(num_classes=2, tolerances=(40,)),
                dict(num_classes=2, max_distance=33), dict(num_classes=2, tolerances=(1.5,))):
        with pytest.raises(ValueError):
            Q(**_stats(), **bad)
    # the restatement's own finish agrees on a real case
    case = next(c for c in BC.CASES if c.name == "one_tile")
    ref = R.boundary_stats(case.pred, case.label, case.C, 2, 32, case.ignore)
    assert Q(**{k: v.tolist() for k, v in ref.items()}, num_classes=case.C, images=1) == R.quality(ref, case.C, images=1)


@pytest.mark.parametrize("n", [1, 19, 20, 21])
def test_the_95_percent_rule_in_integers(n):
    """hd95 = the smallest t with 20 cum >= 19 n, i.e. cum >= ceil(0.95 n): n - 1 pixels at distance 1 and one at 9 give 9 up
    to n = 19 (ceil(0.95 n) = n) and 1 from n = 20 on (ceil(0.95 * 20) = 19)"""
    hist = np.zeros((2, R.BINS), dtype=np.int64)
    hist[0, 1], hist[1, 9] = n - 1, 1
    need = -(-19 * n // 20)
    assert need == math.ceil(0.95 * n - 1e-12) and need == (n if n < 20 else n - 1)
    assert R.hd95_of(hist, 32) == (9 if n < 20 else 1)
    hist[1, 9], hist[1, 33] = 0, 1                         # the far pixel past the cap instead: capped, or not reached
    assert R.hd95_of(hist, 32) == (33 if n < 20 else 1)
    assert R.hd95_of(np.zeros((2, R.BINS), dtype=np.int64), 32) is None


# ------------------------------------------------------------------------------------------------ refusals, ABI
def test_refusals():
    import image_segmentation_amd as seg
    m = torch.zeros((4, 6), dtype=torch.uint8)
    lab = torch.zeros((4, 6), dtype=torch.int64)
    meta = lambda *s, dtype=torch.uint8: torch.empty(s, dtype=dtype, device="meta")     # a device tensor as far as the checks go
    bad_settings = [dict(num_classes=0), dict(num_classes=9), dict(num_classes=True), dict(num_classes=2.0), dict(width=0), dict(width=33),
                    dict(width=True), dict(width=2.5), dict(max_distance=0), dict(max_distance=33), dict(max_distance=False),
                    dict(shape="round"), dict(shape=None), dict(image_border=1), dict(image_border=None), dict(ignore_index=True),
                    dict(ignore_index=256), dict(ignore_index=(1, -1)), dict(ignore_index="3"), dict(ignore_index=(2.5,))]
    for kw in bad_settings:
        full = dict(num_classes=3, width=2)
        full.update(kw)
        with pytest.raises(ValueError):                     # argument errors come before the tensors are looked at
            seg.boundary_stats(m, lab, **full)
        ctor = {k: v for k, v in full.items()}
        with pytest.raises(ValueError):
            seg.BoundaryQuality(ctor.pop("num_classes"), **ctor)
    for tol in ((40,), (-1,), (True,), 3, "12", (1.5,)):
        with pytest.raises(ValueError):
            seg.BoundaryQuality(3, tolerances=tol)
    # tensors: all refused before any launch (no GPU here: a launch would raise something else)
    for p in (m, m.numpy(), m.float(), m[0], m[None], torch.zeros((0, 4), dtype=torch.uint8), m.bool(), meta(4, 6, dtype=torch.int64),
              meta(4, 6, dtype=torch.float32), meta(6), meta(1, 4, 6)):
        with pytest.raises(ValueError):
            seg.boundary_stats(p, lab, 3, width=2)
        with pytest.raises(ValueError):
            seg.BoundaryQuality(3, width=2).update(p, lab)
    from image_segmentation_amd import boundary as B
    cpu = torch.device("cpu")
    for bad_label, why in ((lab.numpy(), "tensor"), (None, "tensor"), (lab.float(), "integer"), (lab.bool(), "integer"),
                           (lab[:, :5], "like the prediction"), (torch.stack([lab, lab]), "like the prediction"), (lab.t(), "like the prediction"),
                           (lab.reshape(-1), "like the prediction"), (lab, "no CPU path"), (lab[None], "no CPU path")):
        with pytest.raises(ValueError, match=why):
            B._check_label(bad_label, (4, 6), cpu)
        with pytest.raises(ValueError):
            seg.boundary_stats(m, bad_label, 3, width=2)
    with pytest.raises(ValueError, match="2\\^28"):
        seg.boundary_stats(meta(1 << 15, (1 << 13) + 1), lab, 3, width=2)
    with pytest.raises(ValueError, match="width="):         # the published width of a large image is past the primitive's radius
        seg.boundary_stats(meta(3000, 4000), meta(3000, 4000, dtype=torch.int64), 3)
    with pytest.raises(ValueError):
        seg.boundary_quality([m], [], 3)
    with pytest.raises(ValueError):
        seg.boundary_quality([m], [lab], 3, out=seg.BoundaryQuality(4))
    a = seg.BoundaryQuality(3, ignore_index=(2,), width=2)
    for other in (seg.BoundaryQuality(4, ignore_index=(2,), width=2), seg.BoundaryQuality(3, width=2), seg.BoundaryQuality(3, ignore_index=2),
                  seg.BoundaryQuality(3, ignore_index=2, width=2, shape="disk"), seg.PanopticQuality(3), None):
        with pytest.raises(ValueError):
            a.add_(other)
    assert a.add_(seg.BoundaryQuality(3, ignore_index=2, width=2)) is a and a.images == 0       # an int or an iterable: the same set
    assert a.compute()["boundary_iou"] == [None] * 3 and a.compute()["images"] == 0


def test_the_defaults_are_the_published_boundary_iou():
    import inspect
    import image_segmentation_amd as seg
    for f in (seg.boundary_stats, seg.BoundaryQuality.__init__):
        p = inspect.signature(f).parameters
        assert p["shape"].default == "square" and p["image_border"].default is True and p["width"].default is None
        assert p["max_distance"].default == 32
    assert inspect.signature(seg.BoundaryQuality.__init__).parameters["tolerances"].default == (1, 2, 3)


def test_header_macros_and_binding():
    from image_segmentation_amd import _lib, boundary as B
    assert BC.macro("SEGK_ABI_VERSION") == _lib.ABI_VERSION >= 330 and BC.macro("SEGK_ENTRY_COUNT") == len(_lib.SIGNATURES) >= 120
    assert (BC.TH, BC.TW) == (_lib.BOUNDARY_TILE_H, _lib.BOUNDARY_TILE_W)
    assert BC.macro("SEGK_BOUNDARY_MAX_WIDTH") == _lib.BOUNDARY_MAX_WIDTH == R.MAX_WIDTH == B.MAX_WIDTH == BC.macro("SEGK_MORPH_MAX_RADIUS")
    assert BC.macro("SEGK_BOUNDARY_BINS") == _lib.BOUNDARY_BINS == R.BINS == _lib.BOUNDARY_MAX_WIDTH + 2
    assert _lib.BOUNDARY_HIST_WORDS == 2 * _lib.MAX_CLASSES * _lib.BOUNDARY_BINS
    off = {k: BC.macro("SEGK_BOUNDARY_" + n) for k, n in (("band_g", "BAND_G"), ("band_p", "BAND_P"), ("band_i", "BAND_I"), ("conf", "CONF"),
                                                            ("hd_sum", "HD_SUM"), ("hd_images", "HD_IMAGES"), ("hd_capped", "HD_CAPPED"),
                                                            ("hist", "HIST"))}
    assert off == _lib.BOUNDARY_OFFSETS and _lib.BOUNDARY_STAT_WORDS == off["hist"] + _lib.BOUNDARY_HIST_WORDS
    sizes = dict(band_g=8, band_p=8, band_i=8, conf=64, hd_sum=8, hd_images=8, hd_capped=8, hist=_lib.BOUNDARY_HIST_WORDS)
    order = sorted(off, key=off.get)
    assert off[order[0]] == 0 and all(off[a] + sizes[a] == off[b] for a, b in zip(order, order[1:]))     # no gap, no overlap
    assert _lib.SIGNATURES["segk_boundary_stats"][1].count(_lib._i) == 8 and len(_lib.SIGNATURES["segk_boundary_finish"][1]) == 5
    # the largest launch (8 classes, halo 33) fits a CU's 160 KiB of LDS with the static tables; two of up to six classes do
    lds = lambda C, halo: (2 * C + 4) * (BC.TH + 2 * halo) * 32
    assert lds(8, 33) + 8192 <= 160 * 1024 and lds(6, 33) + 8192 <= 80 * 1024
    st = B.BoundaryStats.zeros(3, 32, "cpu")
    assert st.words.shape == (656,) and st.image_hist.shape == (544,) and st.hist.shape == (2, 8, 34) and st.band_conf.shape == (8, 8)
    st.hist[1, 2, 3] = 7
    assert st.words[off["hist"] + (8 + 2) * 34 + 3] == 7 and st.tolist()["hist"][1][2][3] == 7
