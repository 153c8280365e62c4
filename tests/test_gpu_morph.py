"""MI355X: mask morphology on the device (image_segmentation_amd/morph.py, csrc/morph.hip) against the
NumPy restatement (tests/morph_reference.py) on the shared case table (tests/morph_cases.py), bit for bit: every case x
operation x shape x radius, written into a prefilled buffer whose slack must stay, run twice and on a side stream; views and
non-contiguous inputs; hole filling with its counts and its overflow regime; Segmenter(morph=...); the label band in front of
the training path; the two tools."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases as MC                                                           # noqa: E402
import morph_reference as R                                                        # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 96


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as seg
    return seg


def launch_into_prefilled(morph, x, stage, paint=None, want_dist=False):
    """One segk_morph launch whose output lies inside a 0xFF-prefilled buffer with SLACK bytes on both sides: -> (output,
    the buffer's slack).  The kernel writes every output byte once and nothing else."""
    from image_segmentation_amd import _lib, ops
    H, W = x.shape
    item = 2 if want_dist else 1
    buf = torch.full((SLACK + H * W * item + SLACK,), 0xFF, dtype=torch.uint8, device=x.device)
    inner = buf[SLACK:SLACK + H * W * item]
    s = ops._stream()
    tab = morph._tables_on(x.device, s, stage.tables)
    _lib.call("segk_morph", x.data_ptr(), ops._p(paint), 0 if want_dist else inner.data_ptr(), inner.data_ptr() if want_dist else 0,
              tab.data_ptr(), tab.data_ptr() + 512, stage.value, stage.metric, stage.radius, H, W, s)
    out = inner.view(torch.uint16).view(H, W) if want_dist else inner.view(H, W)
    return out, torch.cat([buf[:SLACK], buf[-SLACK:]])


@pytest.mark.parametrize("case", MC.CASES, ids=[c.name for c in MC.CASES])
def test_every_operation_equals_the_restatement(seg, case):
    from image_segmentation_amd import morph
    m = case.mask
    x = torch.from_numpy(m.copy()).cuda()
    side = torch.cuda.Stream()
    for shape in MC.SHAPES:
        for r in case.radii:
            for name, fn, kw in MC.operations(case, shape, r):
                want = getattr(R, fn)(m, **kw)
                got = getattr(seg, fn)(x, **kw)
                assert got.dtype == (torch.uint16 if fn == "boundary_distance" else torch.uint8) and got.shape == x.shape
                assert np.array_equal(got.cpu().numpy(), want), (name, shape, r)
                again = getattr(seg, fn)(x, **kw)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    third = getattr(seg, fn)(x, **kw)
                torch.cuda.current_stream().wait_stream(side)
                assert torch.equal(again, got) and torch.equal(third, got), (name, shape, r)
            # the launches themselves, into a prefilled buffer: erode (one stage), open's second stage (paint) and the distance
            plan = morph._open_plan(case.classes, r, case.fill, shape)
            e, slack = launch_into_prefilled(morph, x, plan[0])
            assert np.array_equal(e.cpu().numpy(), R.erode(m, case.classes, r, case.fill, shape)) and (slack == 0xFF).all()
            o, slack = launch_into_prefilled(morph, e.clone(), plan[1], paint=x)
            assert np.array_equal(o.cpu().numpy(), R.open_mask(m, case.classes, r, case.fill, shape)) and (slack == 0xFF).all()
            d, slack = launch_into_prefilled(morph, x, morph._distance_plan(r, None, case.skip, shape)[0], want_dist=True)
            assert np.array_equal(d.cpu().numpy(), R.boundary_distance(m, r, None, case.skip, shape)) and (slack == 0xFF).all()
    assert np.array_equal(x.cpu().numpy(), m)               # the input is left as it was


def test_views_and_non_contiguous_inputs(seg):
    case = next(c for c in MC.CASES if c.name == "corners_and_borders")
    m = case.mask
    H, W = m.shape
    flat = torch.zeros((H * W + 7,), dtype=torch.uint8, device="cuda")
    flat[3:3 + H * W] = torch.from_numpy(m.copy()).cuda().reshape(-1)
    odd = flat[3:3 + H * W].view(H, W)                      # a view at an odd byte offset
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    wide = torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")
    wide[:, ::2] = torch.from_numpy(m.copy()).cuda()
    strided = wide[:, ::2]                                  # not contiguous
    tr = torch.from_numpy(np.ascontiguousarray(m.T)).cuda().t()            # a transposed view
    assert not strided.is_contiguous() and not tr.is_contiguous()
    for x in (odd, strided, tr):
        before = x.clone()
        for shape in MC.SHAPES:
            for name, fn, kw in MC.operations(case, shape, 3):
                assert np.array_equal(getattr(seg, fn)(x, **kw).cpu().numpy(), getattr(R, fn)(m, **kw)), (name, shape)
        got = seg.fill_holes(x, (1, 2), value=2)
        assert np.array_equal(got.mask.cpu().numpy(), R.fill_holes(m, (1, 2), value=2)[0])
        assert torch.equal(x, before)


@pytest.mark.parametrize("hc", MC.HOLE_CASES, ids=[h.name for h in MC.HOLE_CASES])
def test_fill_holes_equals_the_restatement(seg, hc):
    want, num, filled = R.fill_holes(hc.mask, **hc.keywords)
    x = torch.from_numpy(hc.mask.copy()).cuda()
    side = torch.cuda.Stream()
    got = seg.fill_holes(x, **hc.keywords)
    again = seg.fill_holes(x, **hc.keywords)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = seg.fill_holes(x, **hc.keywords)
    torch.cuda.current_stream().wait_stream(side)
    for g in (got, again, third):
        assert np.array_equal(g.mask.cpu().numpy(), want)
        assert (int(g.num), int(g.filled)) == (num, filled)
        assert g.complete == (num <= hc.keywords.get("max_components", 65536))
    assert np.array_equal(x.cpu().numpy(), hc.mask)
    if hc.name == "overflow":
        assert not got.complete and filled == 49 and num == 169           # the rows ran out: the later holes stayed


# ------------------------------------------------------------------------------------------------ Segmenter(morph=...)
SIZES = [(40, 56), (97, 75), (33, 61)]
T = 64
STEPS = [dict(op="open", classes=(1, 2, 3), radius=1, fill=0, shape="square"), dict(op="close", classes=(1,), radius=2),
         dict(op="fill_holes", classes=(2,), connectivity=8), dict(op="dilate", classes=(3,), radius=1, into=(0,), shape="diamond")]
CLEAN = dict(min_area=20, keep_largest=(1, 2))


@pytest.fixture(scope="module")
def setup(seg):
    """the small random-weight U-Net of tests/test_gpu_components_segmenter.py, three ragged images and their label maps"""
    from oracle.fill import fill, labels, fill_module
    from oracle import resize_ref, unet_ref
    images = [fill((3,) + s, 70 + i, 0, 1) for i, s in enumerate(SIZES)]
    r = unet_ref.unet(3, 4)
    fill_module(r, 1000)
    Xb, _ = resize_ref.process_batch_forward(images, T)
    with torch.no_grad():
        r.train()
        for _ in range(20):
            r(Xb)
        r.eval()
        r.output.bias -= r(Xb).mean(dim=(0, 2, 3))
    m = seg.unet(3, 4)
    m.load_state_dict(r.state_dict())
    m.cuda().eval()
    labs = [labels(s, 80 + i, 4) for i, s in enumerate(SIZES)]
    return m, images, labs


def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


def by_hand(m):
    m = R.open_mask(m, (1, 2, 3), 1, 0, "square")
    m = R.close_mask(m, (1,), 2)
    m = R.fill_holes(m, (2,), connectivity=8)[0]
    return R.dilate(m, (3,), 1, into=(0,), shape="diamond")


def test_segmenter_morph_none_changes_nothing(seg, setup):
    m, images, labs = setup
    plain = seg.Segmenter(m, target_size=T)(images, labels=labs)
    for preds in (seg.Segmenter(m, target_size=T, morph=None)(images, labels=labs), seg.predict(m, images, labels=labs, target_size=T, morph=None)):
        for a, b in zip(preds, plain):
            assert same(a.mask, b.mask) and same(a.color, b.color) and same(a.counts, b.counts) and same(a.confusion, b.confusion)
            assert a.meta == b.meta and a.raw_mask is None and a.components is None
    cleaned = seg.Segmenter(m, target_size=T, clean=CLEAN)(images, labels=labs)
    for a, b in zip(seg.Segmenter(m, target_size=T, clean=CLEAN, morph=None)(images, labels=labs), cleaned):
        assert same(a.mask, b.mask) and same(a.raw_mask, b.raw_mask) and same(a.color, b.color) and same(a.counts, b.counts)
        assert same(a.confusion, b.confusion) and same(a.components.labels, b.components.labels)


def test_segmenter_morph_equals_the_operations_by_hand(seg, setup):
    import components_reference as CR
    m, images, labs = setup
    plain = seg.Segmenter(m, target_size=T)(images, labels=labs)
    pal = np.asarray([seg.COLOR_MAP[k] for k in range(4)], dtype=np.uint8)
    steps = [seg.MorphStep(**STEPS[0]), STEPS[1], STEPS[2], seg.MorphStep(**STEPS[3])]
    differ = 0
    for clean, vectors in ((None, None), (CLEAN, None), (CLEAN, True), (None, True)):
        preds = seg.Segmenter(m, target_size=T, morph=steps, clean=clean, vectors=vectors)(images, labels=labs)
        for p, q, lab in zip(preds, plain, labs):
            assert torch.equal(p.raw_mask, q.mask)           # the argmax, bit for bit
            raw = q.mask.cpu().numpy()
            want = by_hand(raw)
            differ += int((want != raw).sum())
            if clean is not None:
                ref = CR.components(want, 4, **clean)
                assert np.array_equal(p.components.labels.cpu().numpy(), ref["labels"]) and p.components.mask is p.mask
                want = ref["mask"]
            else:
                assert p.components is None
            mask = p.mask.cpu().numpy()
            assert np.array_equal(mask, want)
            assert np.array_equal(p.color.cpu().numpy(), pal[mask])
            assert np.array_equal(p.counts.cpu().numpy(), np.bincount(mask.ravel(), minlength=4))
            lab = lab.numpy()
            ok = (lab >= 0) & (lab < 4)
            conf = np.zeros((4, 4), dtype=np.int64)
            np.add.at(conf, (mask[ok].astype(np.int64), lab[ok]), 1)
            assert np.array_equal(p.confusion.cpu().numpy(), conf)
            if vectors:
                v = seg.vectorize(p.mask)
                V = max(int(v.totals[3]), 0)                 # -1: the default edge capacity overflowed, on both alike
                assert torch.equal(p.vectors.totals, v.totals) and torch.equal(p.vectors.xy[:V], v.xy[:V])
            else:
                assert p.vectors is None
    assert differ > 0                                        # the steps did change something


# ------------------------------------------------------------------------------------------------ the training side
def test_label_band_feeds_class_weights_and_a_loss_step(seg):
    H, W = 48, 64
    sq = np.asarray([[8, 6], [40, 6], [40, 30], [8, 30]], dtype=np.float64)
    tri = np.asarray([[30, 20], [60, 24], [44, 44]], dtype=np.float64)
    hard = seg.rasterize([seg.Shape(rings=[sq], value=1), seg.Shape(rings=[tri], value=2)], (H, W))
    lab = seg.label_band(hard, 2)
    ref = R.label_band(hard.cpu().numpy(), 2)
    assert np.array_equal(lab.cpu().numpy(), ref) and 0 < int((lab == 255).sum()) < H * W // 2
    assert set(np.unique(ref)) == {0, 1, 2, 255}
    w = seg.class_weights(lab, 3, ignore_index=255)
    w_hard = seg.class_weights(hard, 3, ignore_index=255)
    assert w.shape == w_hard.shape == (3,) and torch.isfinite(w).all() and not torch.equal(w, w_hard)
    logits = torch.randn((1, 3, H, W), device="cuda", requires_grad=True)
    loss = torch.nn.CrossEntropyLoss(weight=w.float().cuda(), ignore_index=255)(logits, lab.long()[None])
    loss.backward()
    assert torch.isfinite(loss) and (logits.grad[0][:, lab == 255] == 0).all() and (logits.grad[0][:, lab != 255] != 0).any()


# ------------------------------------------------------------------------------------------------ tools
def test_predict_tool_opens_closes_and_fills(seg, tmp_path):
    import subprocess
    from PIL import Image
    from oracle.fill import fill, fill_module
    m = seg.unet(3, 4)
    fill_module(m, 1000)
    torch.save({"model_state_dict": m.state_dict()}, tmp_path / "w.pt")
    paths = []
    for i, (h, w) in enumerate(((40, 56), (33, 61))):
        img = (fill((h, w, 3), 70 + i, 0, 1).numpy() * 255).astype(np.uint8)
        paths.append(str(tmp_path / f"im{i}.png"))
        Image.fromarray(img, "RGB").save(paths[-1])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--checkpoint", str(tmp_path / "w.pt"), "--size", "64",
                        "--out", str(tmp_path / "shaped"), "--open", "1", "--close", "2", "--fill-holes", "--morph-classes", "1,3",
                        "--morph-shape", "square", *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = seg.Segmenter(m.cuda(), target_size=64)([np.asarray(Image.open(p).convert("RGB")) for p in paths])
    for i, q in enumerate(plain):
        want = R.open_mask(q.mask.cpu().numpy(), (1, 3), 1, 0, "square")
        for c in (1, 3):
            want = R.close_mask(want, (c,), 2, shape="square")
        for c in (1, 3):
            want = R.fill_holes(want, (c,))[0]
        assert np.array_equal(np.asarray(Image.open(tmp_path / "shaped" / f"im{i}_mask.png")), want)


def test_rasterize_tool_void_band(seg, tmp_path):
    import json
    import subprocess
    from PIL import Image
    coco = {"categories": [{"id": 11, "name": "cat"}], "images": [{"id": 1, "file_name": "a.jpg", "height": 30, "width": 44}],
            "annotations": [{"id": 1, "image_id": 1, "category_id": 11, "iscrowd": 0, "segmentation": [[5, 4, 30, 4, 30, 22, 5, 22]]}]}
    json.dump(coco, open(tmp_path / "c.json", "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rasterize.py"), str(tmp_path / "c.json"), "--categories", "cat=1",
                        "--out", str(tmp_path / "band"), "--void-band", "2", "--void-value", "250"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    hard = seg.rasterize(seg.shapes_from_coco(coco["annotations"], {11: 1}), (30, 44)).cpu().numpy()
    assert (hard == 1).sum() == 25 * 18
    assert np.array_equal(np.asarray(Image.open(tmp_path / "band" / "a.png")), R.label_band(hard, 2, value=250))
