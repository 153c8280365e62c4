"""MI355X: boundary quality on the device (image_segmentation_amd/boundary.py, csrc/boundary.hip) against the
NumPy restatement (tests/boundary_reference.py) on the shared case table (tests/boundary_cases.py), bit for bit: every case x
width x shape x image_border, written inside a prefilled buffer whose slack must stay, run twice and on a side stream; label
dtypes, views and non-contiguous inputs; accumulation over images of different sizes with the per-image HD95 totals;
Segmenter(morph=...) into BoundaryQuality; the command-line tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_cases as BC                                                        # noqa: E402
import boundary_reference as R                                                     # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 12                                                 # int64 words on both sides
FILL = -0x0123456789ABCDEF
NAMES = ("band_g", "band_p", "band_i", "band_conf", "hist", "hd_sum", "hd_images", "hd_capped")


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as seg
    return seg


def stats_in_prefilled(B, C, R_):
    """a zeroed BoundaryStats inside a prefilled buffer with SLACK words before, between and after its two tensors"""
    buf = torch.full((3 * SLACK + B.STAT_WORDS + B.HIST_WORDS,), FILL, dtype=torch.int64, device="cuda")
    words = buf[SLACK:SLACK + B.STAT_WORDS]
    hist = buf[2 * SLACK + B.STAT_WORDS:2 * SLACK + B.STAT_WORDS + B.HIST_WORDS]
    words.zero_()
    hist.zero_()
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[SLACK:SLACK + B.STAT_WORDS] = False
    keep[2 * SLACK + B.STAT_WORDS:2 * SLACK + B.STAT_WORDS + B.HIST_WORDS] = False
    return B.BoundaryStats(words, hist, C, R_), buf, keep


def check(st, want, what):
    for name in NAMES:
        got = getattr(st, name).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, want[name]), (what, name, got.tolist(), want[name].tolist())
    assert int(st.image_hist.abs().sum()) == 0, what       # the finish cleared the image's histogram


def as_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", BC.CASES, ids=[c.name for c in BC.CASES])
def test_every_statistic_equals_the_restatement(seg, case):
    from image_segmentation_amd import boundary as B
    pred, label = as_device(case.pred), as_device(case.label)
    ignore = case.ignore or None
    side = torch.cuda.Stream()
    for width, shape, border in BC.settings(case):
        what = (width, shape, border)
        want = R.boundary_stats(case.pred, case.label, case.C, width, case.max_distance, case.ignore, shape, border)
        st, buf, keep = stats_in_prefilled(B, case.C, case.max_distance)
        got = seg.boundary_stats(pred, label, case.C, width, case.max_distance, ignore, shape, border, out=st)
        assert got is st
        check(st, want, what)
        assert bool((buf[keep] == FILL).all()), what
        again = seg.boundary_stats(pred, label, case.C, width, case.max_distance, ignore, shape, border)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            third = seg.boundary_stats(pred, label, case.C, width, case.max_distance, ignore, shape, border)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(again.words, st.words) and torch.equal(third.words, st.words), what
    assert np.array_equal(pred.cpu().numpy(), case.pred) and np.array_equal(label.cpu().numpy(), case.label)      # inputs as they were


def test_the_chosen_offsets_land_in_their_bins(seg):
    """the lone-pixel pairs of the case table: class 1's contours are the two pixels themselves, (dy, dx) apart, so the bin is
    the ceiling of hypot(dy, dx); (R, 1) and an empty label contour land in the overflow bin"""
    by = {c.name: c for c in BC.CASES}
    for name, t in (("offset_1_1", 2), ("offset_3_4", 5), ("offset_0_R", 32), ("offset_R_1", 33)):
        c = by[name]
        st = seg.boundary_stats(as_device(c.pred), as_device(c.label), 2, 1, 32, image_border=False)
        hist = st.hist.cpu().numpy()
        assert hist[0, 1, t] == 1 and hist[1, 1, t] == 1 and hist[0, 1].sum() == 1 and hist[1, 1].sum() == 1, name
        assert hist[0, 0].sum() == 4 and hist[1, 0].sum() == 4, name      # class 0's: the rings around the lone pixels
    c = by["offset_R_1"]
    hist = seg.boundary_stats(as_device(c.pred), as_device(c.label), 2, 1, 32).hist.cpu().numpy()
    assert hist[0, 1, 33] == 1 and hist[1, 1, 33] == 1     # 32^2 + 1 > 32^2: past the cap
    c = by["offset_R_1_small_cap"]
    st = seg.boundary_stats(as_device(c.pred), as_device(c.label), 2, 1, 5)
    assert st.hist.cpu().numpy()[0, 1, 6] == 1 and int(st.hd_capped[1]) + int(st.hd_images[1]) == 1
    c = by["empty_label_contour"]
    st = seg.boundary_stats(as_device(c.pred), as_device(c.label), 2, 2, 32)
    hist = st.hist.cpu().numpy()
    assert hist[0, :, 33].tolist()[:2] == [80, 80] and hist[0].sum() == 160 and hist[1].sum() == 0       # two contour rows per side and class
    assert st.hd_capped.cpu().tolist()[:2] == [1, 1] and int(st.hd_images.sum()) == 0 and int(st.hd_sum.sum()) == 0


def test_label_dtypes_views_and_non_contiguous_inputs(seg):
    case = next(c for c in BC.CASES if c.name == "tile_plus_column")
    H, W = case.pred.shape
    want = R.boundary_stats(case.pred, case.label, case.C, 2, 32)
    pred, label = as_device(case.pred), as_device(case.label)
    flat = torch.zeros((H * W + 7,), dtype=torch.uint8, device="cuda")
    flat[3:3 + H * W] = pred.reshape(-1)
    odd = flat[3:3 + H * W].view(H, W)                      # a view at an odd byte offset
    wide = torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")
    wide[:, ::2] = pred
    strided = wide[:, ::2]
    tr = as_device(case.pred.T).t()
    assert odd.data_ptr() % 2 == 1 and not strided.is_contiguous() and not tr.is_contiguous()
    labels = [label, label.long(), label.int(), label.short(), label.long()[None], as_device(case.label.T).t(), label.long().t().contiguous().t()]
    for p in (pred, odd, strided, tr):
        for lab in labels:
            check(seg.boundary_stats(p, lab, case.C, 2), want, (p.stride(), lab.dtype, lab.stride()))
    neg = label.long()
    neg[label == 255] = -7                                  # outside 0..255: void, as 255 is
    check(seg.boundary_stats(pred, neg, case.C, 2), want, "negative void")
    assert torch.equal(odd, pred) and torch.equal(strided, pred)

    class P:                                               # anything with a .mask, as a Prediction
        mask = pred
    check(seg.boundary_stats(P(), label, case.C, 2), want, "prediction")
    # pred == label through the device: Boundary IoU 1 and all mass in bin 0
    st = seg.boundary_stats(label, label, case.C, 2)
    assert torch.equal(st.band_g, st.band_i) and torch.equal(st.band_p, st.band_i) and int(st.hist[:, :, 1:].sum()) == 0
    with pytest.raises(ValueError, match="out"):
        seg.boundary_stats(pred, label, case.C, 2, out=seg.BoundaryStats.zeros(case.C + 1, 32, "cuda"))
    with pytest.raises(ValueError, match="out"):
        seg.boundary_stats(pred, label, case.C, 2, out=torch.zeros(656, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        seg.boundary_stats(pred, label.cpu(), case.C, 2)
    with pytest.raises(ValueError):
        seg.boundary_stats(pred.cpu(), label, case.C, 2)


def test_updates_of_different_sizes_add_up_with_their_hd95_totals(seg):
    by = {c.name: c for c in BC.CASES}
    group = [by["one_tile"], by["small_cap"], by["int64_label"], by["noise"], by["all_void_label"], by["one_row"]]
    C, ignore = 3, (2,)
    a, b = seg.BoundaryQuality(C, ignore_index=ignore, tolerances=(0, 1, 2, 5)), seg.BoundaryQuality(C, ignore_index=2, tolerances=(0, 1, 2, 5))
    want = R.empty_stats()
    for k, c in enumerate(group):
        H, W = c.pred.shape
        one = R.boundary_stats(c.pred, c.label, C, None, 32, ignore)      # width=None: the published width of each image
        assert R.published_width(H, W) in (1, 2, 3)
        want = R.add_stats(want, one)
        (a if k % 2 else b).update(as_device(c.pred), as_device(c.label))
    assert int(want["hd_images"].sum()) >= 6 and int(want["hd_sum"].sum()) > 0 and len({c.pred.shape for c in group}) == len(group)
    a.add_(b)
    assert a.images == len(group) and b.images == 3
    check(a.stats, want, "sum")
    got = a.compute()
    ref = R.quality(want, C, (0, 1, 2, 5), 32, len(group))
    assert got == ref and json.loads(json.dumps(got))["images"] == len(group)
    assert got["hd95"] == [want["hd_sum"][c] / want["hd_images"][c] if want["hd_images"][c] else None for c in range(C)]
    listed = seg.boundary_quality([as_device(c.pred) for c in group], [torch.from_numpy(np.asarray(c.label)) for c in group], C,
                                  ignore_index=ignore, tolerances=(0, 1, 2, 5))
    assert listed == ref
    a.reset()
    assert a.stats is None and a.images == 0 and a.compute()["boundary_iou"] == [None] * C


# ------------------------------------------------------------------------------------------------ Segmenter, the tool
SIZES = [(40, 56), (33, 61)]
T = 64
STEPS = [dict(op="open", classes=(1, 2, 3), radius=1, fill=0, shape="square"), dict(op="close", classes=(1,), radius=2)]


@pytest.fixture(scope="module")
def setup(seg):
    """a small random-weight U-Net, two ragged images and their label maps"""
    from oracle.fill import fill, labels, fill_module
    m = seg.unet(3, 4)
    fill_module(m, 1000)
    m.cuda().eval()
    images = [fill((3,) + s, 70 + i, 0, 1) for i, s in enumerate(SIZES)]
    labs = [labels(s, 80 + i, 4) for i, s in enumerate(SIZES)]
    return m, images, labs


def test_segmenter_with_morph_feeds_boundary_quality(seg, setup):
    m, images, labs = setup
    want = {}
    for morph in (None, STEPS):
        preds = seg.Segmenter(m, target_size=T, morph=morph)(images)
        bq = seg.BoundaryQuality(4, ignore_index=3, width=2)
        total = R.empty_stats()
        for p, lab in zip(preds, labs):
            bq.update(p, lab.cuda())
            total = R.add_stats(total, R.boundary_stats(p.mask.cpu().numpy(), lab.numpy(), 4, 2, 32, (3,)))
        check(bq.stats, total, morph)
        assert bq.compute() == R.quality(total, 4, (1, 2, 3), 32, 2)
        assert seg.boundary_quality(preds, labs, 4, ignore_index=3, width=2) == bq.compute()
        want[morph is None] = total
    assert int(want[True]["band_p"].sum()) > 0


def test_evaluate_boundaries_tool(seg, setup, tmp_path):
    from PIL import Image
    m, images, labs = setup
    torch.save({"model_state_dict": m.state_dict()}, tmp_path / "w.pt")
    os.makedirs(tmp_path / "images")
    os.makedirs(tmp_path / "labels")
    arrays = []
    for i, (img, lab) in enumerate(zip(images, labs)):
        arrays.append((img.permute(1, 2, 0).numpy() * 255).astype(np.uint8))
        Image.fromarray(arrays[-1], "RGB").save(tmp_path / "images" / f"im{i}.png")
        Image.fromarray(lab.numpy().astype(np.uint8), "L").save(tmp_path / "labels" / f"im{i}.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate_boundaries.py"), "--checkpoint", str(tmp_path / "w.pt"),
                        "--images", str(tmp_path / "images"), "--labels", str(tmp_path / "labels"), "--classes", "4", "--ignore-index", "3",
                        "--size", str(T), "--width", "2", "--tolerances", "1,4", "--open", "1", "--close", "2", "--morph-classes", "1,2",
                        "--morph-shape", "square", "--min-area", "3", "--out", str(tmp_path / "b.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.load(open(tmp_path / "b.json"))
    morph = [dict(op="open", classes=(1, 2), radius=1, fill=0, shape="square")] + [dict(op="close", classes=(c,), radius=2, shape="square")
                                                                                   for c in (1, 2)]
    preds = seg.Segmenter(m, target_size=T, palette=None, morph=morph, clean=dict(connectivity=4, min_area=3))(arrays)
    total = R.empty_stats()
    for p, lab in zip(preds, labs):
        total = R.add_stats(total, R.boundary_stats(p.mask.cpu().numpy(), lab.numpy(), 4, 2, 32, (3,)))
    ref = json.loads(json.dumps(R.quality(total, 4, (1, 4), 32, 2)))
    assert {k: got[k] for k in ref} == ref and got["open"] == 1 and got["close"] == 2 and got["min_area"] == 3 and got["width"] == 2
