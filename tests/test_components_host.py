"""CPU: the restatement of DESIGN.md 3.3 (tests/components_reference.py) against hand-written cases and, where scipy is
installed, against scipy.ndimage.label per class; the argument checks of image_segmentation_amd.components, which has no
CPU path; the ABI's workspace size; the tools' new options."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as R                                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u8(rows):
    return np.asarray(rows, dtype=np.uint8)


def test_ring_with_a_hole():
    m = u8([[0, 0, 0, 0, 0],
            [0, 1, 1, 1, 0],
            [0, 1, 0, 1, 0],
            [0, 1, 1, 1, 0],
            [0, 0, 0, 0, 0]])
    r = R.components(m, 4)
    assert r["num"] == 3
    assert r["cls"].tolist() == [0, 1, 0] and r["area"].tolist() == [16, 8, 1] and r["first"].tolist() == [0, 6, 12]
    assert r["box"].tolist() == [[0, 0, 5, 5], [1, 1, 4, 4], [2, 2, 3, 3]]
    assert np.array_equal(r["mask"], m) and r["kept"].tolist() == [1, 1, 1] and r["new_cls"].tolist() == [0, 1, 0]
    r = R.components(m, 4, min_area=2)                     # the hole goes: its four neighbours are the ring
    assert r["kept"].tolist() == [1, 1, 0] and r["new_cls"].tolist() == [0, 1, 1] and r["mask"][2, 2] == 1
    assert (r["mask"] != m).sum() == 1
    r = R.components(m, 4, keep_largest=(0,))              # the same through keep_largest: the hole is the smaller class-0 part
    assert r["kept"].tolist() == [1, 1, 0] and r["mask"][2, 2] == 1
    r = R.components(m, 4, classes=(1,))                   # class 0 unlabelled: id 0, never changed, but it votes
    assert r["num"] == 1 and r["labels"][0, 0] == 0 and r["labels"][1, 1] == 1
    r = R.components(m, 4, classes=(1,), min_area=9)
    assert r["kept"].tolist() == [0] and r["new_cls"].tolist() == [0] and not r["mask"].any()


def test_tie_between_equal_blobs_goes_to_the_lowest_id():
    m = u8([[1, 1, 0, 1, 1],
            [0, 0, 0, 0, 0],
            [2, 0, 0, 0, 1]])
    r = R.components(m, 4, keep_largest=(1,))
    assert r["cls"].tolist() == [1, 0, 1, 2, 1] and r["area"].tolist() == [2, 9, 2, 1, 1]
    assert r["kept"].tolist() == [1, 1, 0, 1, 0]           # ids 1 and 3 tie at two pixels: id 1 stays
    assert r["mask"].tolist() == [[1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [2, 0, 0, 0, 0]]
    r = R.components(m, 4, keep_largest=True)               # every class: 2 has one component, 0 has one
    assert r["kept"].tolist() == [1, 1, 0, 1, 0]


def test_vote_tie_takes_the_lowest_class():
    m = u8([[3, 3, 3],
            [2, 1, 2],
            [3, 3, 3]])
    r = R.components(m, 4, min_area=2)                     # the centre: two votes for 2, two for 3 -- but both 2s go as well
    assert r["cls"].tolist() == [3, 2, 1, 2, 3]
    assert r["kept"].tolist() == [1, 0, 0, 0, 1]
    assert r["new_cls"].tolist() == [3, 3, 3, 3, 3]        # a removed neighbour does not stand: only the 3s vote
    m = u8([[3, 3, 3, 3],
            [2, 2, 1, 3],
            [2, 2, 3, 3]])
    r = R.components(m, 4, min_area=2)                     # the 1: left 2 stands, up 3, right 3, down 3 -> 3
    assert r["mask"][1, 2] == 3
    m = u8([[2, 2, 2],
            [3, 1, 2],
            [3, 3, 3]])
    r = R.components(m, 4, min_area=2)                     # two votes each for 2 and 3: the lower class
    assert r["mask"][1, 1] == 2 and r["new_cls"].tolist()[r["labels"][1, 1] - 1] == 2


def test_one_pass_votes_use_the_input_values():
    m = u8([[1, 2, 0, 0]])
    r = R.components(m, 4, min_area=2)                     # 1 and 2 both go; 1 sees only the removed 2: no votes, it stays 1
    assert r["kept"].tolist() == [0, 0, 1] and r["new_cls"].tolist() == [1, 0, 0]
    assert r["mask"].tolist() == [[1, 0, 0, 0]]


def test_no_vote_component_keeps_its_class():
    m = u8([[1]])
    r = R.components(m, 8, min_area=5)
    assert r["num"] == 1 and r["kept"].tolist() == [0] and r["new_cls"].tolist() == [1] and r["mask"].tolist() == [[1]]
    m = u8([[9, 1, 9],
            [9, 9, 9]])
    r = R.components(m, 4, min_area=5)                     # surrounded by values >= 8: they never vote
    assert r["mask"].tolist() == m.tolist() and r["kept"].tolist() == [0]


def test_values_of_eight_and_more_are_outside():
    m = u8([[8, 1, 1],
            [255, 0, 1],
            [1, 0, 200]])
    r = R.components(m, 4)
    assert r["labels"].tolist() == [[0, 1, 1], [0, 2, 1], [3, 2, 0]] and r["num"] == 3
    r = R.components(m, 4, min_area=2)                     # the lone 1 has a 255 above and a 0 right: one vote
    assert r["mask"].tolist() == [[8, 1, 1], [255, 0, 1], [0, 0, 200]]


def test_diagonal_contact():
    m = u8([[1, 0],
            [0, 1]])
    assert R.components(m, 4)["num"] == 4 and R.components(m, 4)["labels"].tolist() == [[1, 2], [3, 4]]
    r = R.components(m, 8)
    assert r["num"] == 2 and r["labels"].tolist() == [[1, 2], [2, 1]] and r["box"].tolist() == [[0, 0, 2, 2], [0, 0, 2, 2]]
    r = R.components(m, 8, min_area=3)                     # the vote neighbourhood stays 4: each sees the other class twice,
    assert r["kept"].tolist() == [0, 0]                    # but that class is removed too -> no votes, nothing moves
    assert r["mask"].tolist() == m.tolist()


def test_checkerboard_counts():
    m = R.pattern("checkerboard", 64, 64)
    assert R.components(m, 4)["num"] == 64 * 64 and R.components(m, 8)["num"] == 2
    assert R.components(m, 4, classes=(1,))["num"] == 64 * 64 // 2 and R.components(m, 8, classes=(1,))["num"] == 1


def test_patterns_are_what_they_claim():
    for H, W in ((65, 129), (130, 259), (200, 37)):
        for conn in (4, 8):
            for name in ("one_class", "spiral", "comb", "u_shape"):
                r = R.components(R.pattern(name, H, W), conn)
                assert (r["cls"] > 0).sum() == 1, (name, H, W)          # one component of the drawn class
            assert R.components(R.pattern("spiral", H, W), conn)["area"].max() > H + W
    assert 1024 < R.components(R.pattern("noise2", 200, 37), 4)["num"] < 4096
    assert 1024 < R.components(R.pattern("noise4", 200, 37), 4)["num"] < 4096
    b = R.pattern("blobs", 130, 259)
    assert set(np.unique(b)) == {0, 1, 2, 3} and (R.components(b, 4, min_area=20)["mask"] != b).any()


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", R.TALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tall_masks_have_a_root_on_most_rows(size, connectivity):
    H, W = size
    r = R.components(R.pattern("row_stripes", H, W), connectivity)
    assert r["num"] == H and np.array_equal(r["labels"], np.repeat(np.arange(1, H + 1), W).reshape(H, W))
    assert (r["area"] == W).all() and np.array_equal(r["first"], W * np.arange(H)) and r["cls"].tolist() == [1 + (y & 1) for y in range(H)]
    r = R.components(R.pattern("noise2", H, W), connectivity)
    roots_of_row = np.bincount(r["first"] // W, minlength=H)              # the noise: rows with no root, with one and with more
    assert H > 1024 and (roots_of_row > 0).sum() > H // 4 and roots_of_row[1024:].any() and (roots_of_row == 0).any()
    assert roots_of_row.max() > 1 or connectivity == 8


@pytest.mark.parametrize("connectivity", [4, 8])
def test_numbering_is_scipys(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for name in ("noise2", "noise4", "blobs", "rings", "spiral"):
        m = R.pattern(name, 65, 129)
        for c in np.unique(m):
            want, n = ndi.label(m == c, structure=structure)
            r = R.components(m, connectivity, classes=(int(c),))
            assert r["num"] == n and np.array_equal(r["labels"], want), (name, c)
            assert np.array_equal(r["area"], np.bincount(want.ravel())[1:])
            for k, sl in enumerate(ndi.find_objects(want)):
                assert r["box"][k].tolist() == [sl[0].start, sl[1].start, sl[0].stop, sl[1].stop]


# ---------------------------------------------------------------------------------------------- the Python surface
@pytest.fixture(scope="module")
def C():
    return importlib.import_module("image_segmentation_amd.components")


def test_exports(C):
    import image_segmentation_amd as seg
    assert seg.components is C.components and seg.Components is C.Components and seg.Clean is C.Clean
    import inspect
    sig = inspect.signature(seg.components)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == \
        [("connectivity", 4), ("classes", None), ("min_area", 0), ("keep_largest", False), ("max_components", 1024)]
    fields = list(seg.Prediction.__dataclass_fields__)
    assert fields[:5] == ["mask", "color", "counts", "confusion", "meta"] and fields[5:] == ["raw_mask", "components"]
    p = seg.Prediction(None, None, None, None, {})
    assert p.raw_mask is None and p.components is None


def test_has_no_cpu_path(C):
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.components(torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.mask_finish(torch.zeros((4, 4), dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match="uint8"):
        C.components(np.zeros((4, 4), dtype=np.uint8))


@pytest.mark.parametrize("kw, match", [
    (dict(connectivity=6), "connectivity"), (dict(connectivity=True), "connectivity"), (dict(classes=(8,)), "classes"),
    (dict(classes=3), "classes"), (dict(classes=(1.5,)), "classes"), (dict(min_area=-1), "min_area"),
    (dict(min_area=2.5), "min_area"), (dict(keep_largest=(9,)), "keep_largest"), (dict(keep_largest=2), "keep_largest"),
    (dict(max_components=0), "max_components"), (dict(max_components=1 << 25), "max_components")])
def test_argument_checks_come_first(C, kw, match):
    with pytest.raises(ValueError, match=match):           # before the device check: a CPU tensor gets this far
        C.components(torch.zeros((4, 4), dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match=match):
        C.Clean(**kw)


def test_masks_of_classes(C):
    assert C._check_args(4, None, 0, False, 1) == (255, 0)
    assert C._check_args(8, (1, 2), 0, True, 1) == (6, 6)
    assert C._check_args(8, (1, 2), 0, (2, 3), 1) == (6, 4)        # keep_largest only inside the labelled classes
    assert C._check_args(8, [0], 7, None, 1024) == (1, 0)


def test_segmenter_takes_clean(C):
    import image_segmentation_amd as seg
    m = seg.unet(3, 4)
    assert seg.Segmenter(m).clean is None
    s = seg.Segmenter(m, clean=dict(min_area=20, keep_largest=(1, 2)))
    assert s.clean == C.Clean(min_area=20, keep_largest=(1, 2)) and seg.Segmenter(m, clean=s.clean).clean is s.clean
    with pytest.raises(ValueError, match="connectivity"):
        seg.Segmenter(m, clean=dict(connectivity=5))
    with pytest.raises(TypeError):
        seg.Segmenter(m, clean=dict(area=5))
    with pytest.raises(ValueError, match="clean"):
        seg.Segmenter(m, clean=5)


def test_workspace_size_matches_the_header(C):
    import re
    txt = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert re.search(r"#define SEGK_CC_WS_INTS\(H, W\) \(16L \+ 11L \* \(long\)\(H\) \* \(long\)\(W\) \+ 2L \* \(long\)\(H\)\)", txt)
    assert C.ws_ints(7, 5) == 16 + 11 * 35 + 14


def test_new_entries_refuse_bad_arguments_before_any_launch():
    from image_segmentation_amd import _lib
    lib = _lib.load()
    err = lambda: lib.segk_last_error().decode()
    p = 256
    assert lib.segk_cc_label(p, p, p, p, p, p, p, p, 4, 4, 5, 255, 8, None) == -2 and "connectivity" in err()
    assert lib.segk_cc_label(p, p, p, p, p, p, p, None, 4, 4, 4, 255, 8, None) == -2 and "NULL" in err()
    assert lib.segk_cc_label(p, p, p, p, p, p, p, p, 4, 4, 4, 256, 8, None) == -2 and "class_mask" in err()
    assert lib.segk_cc_label(p, p, p, p, p, p, p, p, 1 << 15, 1 << 15, 4, 255, 8, None) == -2 and "2^28" in err()
    assert lib.segk_cc_label(p, p, p, p, p, p, p, p, 4, 4, 4, 255, 0, None) == -2 and "max_components" in err()
    assert lib.segk_cc_clean(p, 512, p, p, p, 4, 4, -1, 0, 8, None) == -2 and "min_area" in err()
    assert lib.segk_cc_clean(p, 512, p, p, p, 4, 4, 0, 256, 8, None) == -2 and "keep_mask" in err()
    assert lib.segk_cc_clean(p, p, p, p, p, 4, 4, 0, 0, 8, None) == -2 and "in place" in err()
    assert lib.segk_mask_finish(p, None, None, None, None, None, 4, 4, 4, None) == -2 and "no output" in err()
    assert lib.segk_mask_finish(p, p, None, p, None, None, 4, 4, 4, None) == -2 and "come together" in err()
    assert lib.segk_mask_finish(p + 1, None, None, p, None, None, 4, 4, 4, None) == -2 and "aligned" in err()
    assert lib.segk_mask_finish(p, None, None, p, None, None, 0, 4, 4, None) == -2 and "classes" in err()


def test_components_kernels_compiled_code():
    """no spills and no scratch in the unit (tools/spill_report.py) and in mask_finish_kernel (csrc/predict.hip), and every
    kernel is there"""
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    rows = tool.report("components") + [r for r in tool.report("predict") if "mask_finish_kernel" in r["name"]]
    names = " ".join(r["name"] for r in rows)
    for k in ("cc_tile_kernel", "cc_border_kernel", "cc_flatten_kernel", "cc_scan_kernel", "cc_rank_kernel", "cc_ids_kernel",
              "cc_clean_init_kernel", "cc_vote_kernel", "cc_apply_kernel", "mask_finish_kernel"):
        assert k in names, k
    for r in rows:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r


def test_tools_know_the_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--min-area", "--keep-largest", "--connectivity", "--boxes"):
        assert opt in r.stdout, opt
    assert "def components():" in open(os.path.join(ROOT, "tools", "kbench.py")).read()
