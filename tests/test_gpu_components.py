"""MI355X: mask clean-up (image_segmentation_amd/components.py, csrc/components.hip) against the restatement of DESIGN.md
3.3 in tests/components_reference.py -- EXACT equality of the labels, K, every statistics row, the removal flags, the new
classes and the cleaned mask, for both connectivities.  The sizes cover one tile, exact multiples of the 32-row x 64-column tile, one
past a multiple and three tiles and more in each direction; the patterns cover one component per pixel, one component winding
through every tile, components whose parts meet only in another tile, and the realistic speckled blob mask.  There is
nothing to tolerance: the arithmetic is integer and the definition makes the result unique."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as R                                                   # noqa: E402

pytestmark = pytest.mark.gpu
PALETTE = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (90, 160, 250)]
CLEAN_PATTERNS = R.PATTERNS
CLEAN_CASES = [dict(min_area=a, keep_largest=k) for a in (1, 2, 5, 50) for k in (False, True, (1, 2))] + \
              [dict(min_area=5, keep_largest=True, classes=(1, 2)), dict(min_area=0, keep_largest=(2, 3), classes=(1, 2))]


@pytest.fixture(scope="module")
def C():
    import importlib                 # the package exports the function components() under the module's name
    return importlib.import_module("image_segmentation_amd.components")


_masks, _labelled = {}, {}


def mask_of(name, H, W):
    if (name, H, W) not in _masks:
        m = R.pattern(name, H, W)
        m.setflags(write=False)
        _masks[name, H, W] = m
    return _masks[name, H, W]


def reference(name, H, W, connectivity, classes=None, **kw):
    """the restatement, its labelling computed once per (mask, connectivity, classes) and left unchanged"""
    key = (name, H, W, connectivity, classes)
    m = mask_of(name, H, W)
    if key not in _labelled:
        _labelled[key] = R.label(m, connectivity, classes)
    labels, rows = _labelled[key]
    out, kept, new_cls = R.clean(m, labels, rows, classes=classes, **kw)
    K = len(rows)
    i32 = lambda k, shape: np.asarray([r[k] for r in rows], dtype=np.int32).reshape(shape)
    return {"labels": labels, "num": K, "cls": i32("cls", K), "area": i32("area", K), "box": i32("box", (K, 4)),
            "first": i32("first", K), "kept": kept, "new_cls": new_cls, "mask": out}


def check(got, ref, cap, what):
    K, n = ref["num"], min(ref["num"], cap)
    assert got.n == K, f"{what}: K = {got.n}, expected {K}"
    lab = got.labels.cpu().numpy()
    assert lab.dtype == np.int32 and np.array_equal(lab, ref["labels"]), f"{what}: {int((lab != ref['labels']).sum())} labels differ"
    for name in ("cls", "area", "first", "box", "kept", "new_cls"):
        a = getattr(got, name).cpu().numpy()
        assert a.dtype == np.int32 and a.shape[0] == cap, (what, name, a.shape)
        assert np.array_equal(a[:n], ref[name][:n]), f"{what}: {name} differs in {int((a[:n] != ref[name][:n]).sum())} places"
        assert not a[n:].any(), f"{what}: {name} rows past min(K, cap) are not zero"
    out = got.mask.cpu().numpy()
    assert out.dtype == np.uint8 and np.array_equal(out, ref["mask"]), f"{what}: {int((out != ref['mask']).sum())} cleaned pixels differ"


def run(C, name, H, W, connectivity, cap, **kw):
    m = mask_of(name, H, W)
    dev = torch.from_numpy(m.copy()).cuda()
    got = C.components(dev, connectivity=connectivity, max_components=cap, **kw)
    ref = reference(name, H, W, connectivity, **kw)
    check(got, ref, cap, f"{name} {H}x{W} c{connectivity} {kw}")
    assert np.array_equal(dev.cpu().numpy(), m), "the input mask was modified"
    return got, ref


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelling_equals_the_restatement(C, size, connectivity):
    H, W = size
    for name in R.PATTERNS:
        _, ref = run(C, name, H, W, connectivity, H * W)           # a row for every component there can be
        if name == "checkerboard":                                  # diagonals join each colour where there are two rows and columns
            assert ref["num"] == (2 if connectivity == 8 and min(H, W) >= 2 else H * W)
        if name in ("one_class", "spiral", "comb", "u_shape"):
            assert (ref["cls"] > 0).sum() == 1, name                # one component of the drawn class across all tiles


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cleaning_equals_the_restatement(C, size, connectivity):
    H, W = size
    changed = 0
    for name in CLEAN_PATTERNS:
        for kw in CLEAN_CASES:
            got, ref = run(C, name, H, W, connectivity, H * W, **kw)
            changed += int((ref["mask"] != mask_of(name, H, W)).sum())
    if H * W >= 31 * 33:
        assert changed > 0                                          # the cases do remove something


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", R.TALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_scan_takes_more_than_one_trip(C, size, connectivity):
    """one workgroup scans the H row counts 1024 per trip (csrc/scan.hpp): two trips and three, a root on most rows"""
    H, W = size
    for name in R.TALL_PATTERNS:
        _, ref = run(C, name, H, W, connectivity, H * W)
        assert name != "row_stripes" or ref["num"] == H


def test_components_past_the_cap(C):
    H, W = 200, 37
    for name, lo in (("noise2", 1024), ("noise4", 1024)):
        K = reference(name, H, W, 4)["num"]
        assert lo < K < 4096, (name, K)                             # more than the default cap, inside the large one
        for kw in (dict(min_area=0), dict(min_area=3, keep_largest=(1, 2))):
            run(C, name, H, W, 4, 4096, **kw)                       # every row is checked
            got, ref = run(C, name, H, W, 4, 256, **kw)             # num is the true K, 256 equal rows, the mask exact
            assert got.n == K > 256 and got.cls.shape == (256,) and got.box.shape == (256, 4)


def test_repeatable_and_default_arguments(C):
    m = torch.from_numpy(mask_of("blobs", 130, 259).copy()).cuda()
    a = C.components(m, min_area=20, keep_largest=(1, 2))
    b = C.components(m, min_area=20, keep_largest=(1, 2))
    for name in ("labels", "num", "cls", "area", "box", "first", "kept", "new_cls", "mask"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.cls.shape == (1024,)
    plain = C.components(m)
    assert torch.equal(plain.mask, m) and plain.mask.data_ptr() != m.data_ptr()
    k = plain.n
    assert int(plain.kept[:k].sum()) == k and torch.equal(plain.new_cls[:k], plain.cls[:k])
    view = torch.from_numpy(mask_of("blobs", 130, 259).copy()).cuda()[3:, 5:]       # not contiguous, not aligned
    got = C.components(view, connectivity=8, min_area=4)
    ref = R.components(mask_of("blobs", 130, 259)[3:, 5:].copy(), 8, min_area=4)
    check(got, ref, 1024, "view")


def test_device_argument_errors(C):
    from image_segmentation_amd import _lib, ops
    m = torch.zeros((4, 5), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="uint8"):
        C.components(m.int())
    with pytest.raises(ValueError, match="uint8"):
        C.components(m[None])
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    ws = torch.zeros(C.ws_ints(4, 5), dtype=torch.int32, device="cuda")
    P, s = (lambda t: t.data_ptr()), ops._stream()
    with pytest.raises(RuntimeError, match="connectivity"):
        _lib.call("segk_cc_label", P(m), P(i), P(i), P(i), P(i), P(i), P(i), P(ws), 4, 5, 6, 255, 4, s)
    with pytest.raises(RuntimeError, match="NULL"):
        _lib.call("segk_cc_label", P(m), None, P(i), P(i), P(i), P(i), P(i), P(ws), 4, 5, 4, 255, 4, s)
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("segk_cc_label", P(m), P(i), P(i), P(i), P(i), P(i), P(i), P(ws), 0, 5, 4, 255, 4, s)
    with pytest.raises(RuntimeError, match="not in place"):
        _lib.call("segk_cc_clean", P(m), P(m), P(ws), P(i), P(i), 4, 5, 0, 0, 4, s)
    with pytest.raises(RuntimeError, match="come together"):
        _lib.call("segk_mask_finish", P(m), P(m), None, None, None, None, 4, 4, 5, s)
    with pytest.raises(RuntimeError, match="classes"):
        _lib.call("segk_mask_finish", P(m), None, None, P(ws), None, None, 9, 4, 5, s)
    torch.cuda.synchronize()


@pytest.mark.parametrize("size", [(1, 1), (1, 9), (7, 1), (2, 3), (31, 33), (65, 129), (130, 259), (200, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_finish_equals_the_lookups(C, size):
    """segk_mask_finish == palette[mask], bincount(mask, minlength=8) and the confusion counts of segk_confusion's rule
    (M[pred][label] += 1 for labels inside [0, C)), bit for bit"""
    H, W = size
    rng = np.random.default_rng(H * 1000 + W)
    pal = np.asarray(PALETTE, dtype=np.uint8)
    for ncls in (1, 3, 4, 8):
        m = rng.integers(0, ncls, size=(H, W), dtype=np.uint8)
        lab = rng.integers(0, ncls, size=(H, W)).astype(np.int64)
        lab[rng.random((H, W)) < 0.1] = 255                         # ignore pixels: skipped
        lab[rng.random((H, W)) < 0.05] = -1
        md, ld, pd = torch.from_numpy(m).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(pal).cuda()
        color, counts, M = C.mask_finish(md, ncls, palette=pd, labels=ld)
        assert np.array_equal(color.cpu().numpy(), pal[m])
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), np.bincount(m.ravel(), minlength=8))
        ok = (lab >= 0) & (lab < ncls)
        want = np.zeros((8, 8), dtype=np.int64)
        np.add.at(want, (m[ok].astype(np.int64), lab[ok]), 1)
        assert np.array_equal(M.cpu().numpy(), want)
        color2, counts2, M2 = C.mask_finish(md, ncls)               # counts alone
        assert color2 is None and M2 is None and torch.equal(counts2, counts)
        assert np.array_equal(md.cpu().numpy(), m)
