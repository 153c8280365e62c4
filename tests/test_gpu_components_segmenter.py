"""MI355X: mask clean-up inside the prediction surface (Segmenter(..., clean=), predict(..., clean=)): with clean=None
every output equals a plain Segmenter's; with a clean-up the raw mask is the plain mask bit for bit, the mask is the
restatement's cleaning of it (tests/components_reference.py), and colour, counts and confusion are those of the cleaned
mask."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle.fill import fill, labels
from oracle import resize_ref, unet_ref
from oracle.fill import fill_module

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as R                                                   # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(40, 56), (97, 75), (33, 61)]
T = 64
CLEAN = dict(min_area=20, keep_largest=(1, 2))


@pytest.fixture(scope="module")
def setup():
    """a small random-weight U-Net whose eval-mode argmax is not one class everywhere (settled BatchNorm buffers, centred
    head bias: the preparation of tests/test_gpu_inference.py), three ragged images and their label maps"""
    import image_segmentation_amd as seg
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
    labs[1][::3, ::4] = 255
    return seg, m, images, labs


def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


def test_clean_none_changes_nothing(setup):
    seg, m, images, labs = setup
    plain = seg.Segmenter(m, target_size=T)(images, labels=labs)
    for preds in (seg.Segmenter(m, target_size=T, clean=None)(images, labels=labs),
                  seg.predict(m, images, labels=labs, target_size=T, clean=None)):
        for a, b in zip(preds, plain):
            assert same(a.mask, b.mask) and same(a.color, b.color) and same(a.counts, b.counts) and same(a.confusion, b.confusion)
            assert a.meta == b.meta and a.raw_mask is None and a.components is None


def test_cleaned_prediction(setup):
    seg, m, images, labs = setup
    plain = seg.Segmenter(m, target_size=T)(images, labels=labs)
    s = seg.Segmenter(m, target_size=T, clean=CLEAN)
    preds = s(images, labels=labs)
    pal = np.asarray([seg.COLOR_MAP[k] for k in range(4)], dtype=np.uint8)
    differ = 0
    for p, q, lab in zip(preds, plain, labs):
        assert torch.equal(p.raw_mask, q.mask)                      # the argmax, bit for bit
        raw = q.mask.cpu().numpy()
        ref = R.components(raw, 4, **CLEAN)
        mask = p.mask.cpu().numpy()
        assert np.array_equal(mask, ref["mask"])
        differ += int((mask != raw).sum())
        assert p.components.n == ref["num"] and np.array_equal(p.components.labels.cpu().numpy(), ref["labels"])
        assert p.components.mask is p.mask
        k = min(ref["num"], 1024)
        assert np.array_equal(p.components.kept.cpu().numpy()[:k], ref["kept"][:k])
        # colour, counts and confusion are those of the cleaned mask
        assert np.array_equal(p.color.cpu().numpy(), pal[mask])
        assert p.counts.shape == (4,) and np.array_equal(p.counts.cpu().numpy(), np.bincount(mask.ravel(), minlength=4))
        lab = lab.numpy()
        ok = (lab >= 0) & (lab < 4)
        want = np.zeros((4, 4), dtype=np.int64)
        np.add.at(want, (mask[ok].astype(np.int64), lab[ok]), 1)
        assert p.confusion.shape == (4, 4) and np.array_equal(p.confusion.cpu().numpy(), want)
    assert differ > 0                                               # the clean-up did remove something
    again = s(images, labels=labs)                                  # a second call: identical tensors
    for a, b in zip(again, preds):
        assert same(a.mask, b.mask) and same(a.raw_mask, b.raw_mask) and same(a.color, b.color) and same(a.counts, b.counts)
        assert same(a.confusion, b.confusion) and same(a.components.labels, b.components.labels)
        assert same(a.components.area, b.components.area) and same(a.components.box, b.components.box)
    one = seg.predict(m, images, target_size=T, clean=seg.Clean(**CLEAN), palette=None)
    for a, b in zip(one, preds):
        assert same(a.mask, b.mask) and a.color is None and a.confusion is None and same(a.counts, b.counts)
