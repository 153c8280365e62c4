"""MI355X: device-side augmentation (image_segmentation_amd/augment.py, csrc/augment.hip) against the NumPy restatement of
its integer arithmetic (tests/augment_reference.py) -- EXACT equality of the uint8 image, the float image and the int64 label
for plain resize and each of the eight ops -- and against the reference's own outputs for the parts that are pinned
(tests/golden/augment_ref.npz: pair merge, colour -> class map, class weights).  No tolerance anywhere."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_reference as R                                                      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(375, 500), (500, 333), (256, 256), (17, 31), (1, 1)]
PALETTE = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 0], [255, 255, 255], [12, 200, 7]], np.uint8)
LUT = np.arange(256, dtype=np.uint8)
LUT[255] = 3


@pytest.fixture(scope="module")
def A():
    from image_segmentation_amd import augment
    return augment


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "augment_ref.npz"))


def sources(seed):
    """a ragged batch: the five sizes; sample 1 is RGBA; labels alternate between trimap values and colours"""
    rng = np.random.default_rng(seed)
    imgs, labs = [], []
    for k, (H, W) in enumerate(SIZES):
        c = 4 if k == 1 else 3
        smooth = np.kron(rng.integers(0, 256, (-(-H // 7), -(-W // 7), c)), np.ones((7, 7, 1), np.int64))[:H, :W]
        imgs.append(np.clip(smooth + rng.integers(-40, 41, (H, W, c)), 0, 255).astype(np.uint8))
        pick = np.kron(rng.integers(0, 5, (-(-H // 5), -(-W // 5))), np.ones((5, 5), np.int64))[:H, :W]
        labs.append(PALETTE[pick] if k % 2 else np.array([0, 1, 2, 255, 2], np.uint8)[pick])
    return imgs, labs


def plans_for(A, op, seed):
    rng = np.random.default_rng(1000 + seed)
    out = []
    for H, W in SIZES:
        kw = dict(seed=int(rng.integers(0, 1 << 32)))
        if op == A.RANDOM_CROP:
            s = max(1, int(min(H, W) * 2 / 3))
            kw.update(y1=int(rng.integers(0, H - s + 1)), x1=int(rng.integers(0, W - s + 1)))
        elif op == A.ROTATION:
            kw.update(theta=float(rng.uniform(45.0, 315.0)))
        elif op == A.LAPLACE:
            kw.update(b=float(rng.uniform(25.5, 76.5)))
        elif op == A.CONTRAST:
            kw.update(alpha=float(rng.uniform(0.2, 0.6)))
        out.append(A.make_plan(op, H, W, **kw))
    return out


def check_batch(A, aug, imgs, labs, plans, T, lut, fill):
    di = [torch.from_numpy(a).cuda() for a in imgs]
    dl = [torch.from_numpy(a).cuda() for a in labs]
    X, X8, y = aug.apply(di, dl, plans, out="both")
    torch.cuda.synchronize()
    assert X.shape == (len(imgs), 3, T, T) and X.dtype == torch.float32
    assert X8.shape == (len(imgs), T, T, 3) and X8.dtype == torch.uint8
    assert y.shape == (len(imgs), 1, T, T) and y.dtype == torch.int64
    X, X8, y = X.cpu().numpy(), X8.cpu().numpy(), y.cpu().numpy()
    for k, (im, lb, p) in enumerate(zip(imgs, labs, plans)):
        want8, wantl = R.augment(im, lb, p, T, lut, fill)
        what = f"{A.OP_NAMES[p.op]} sample {k} {im.shape} T={T}"
        bad = int((X8[k] != want8).sum())
        assert bad == 0, f"{what}: {bad} uint8 image bytes differ (max {np.abs(X8[k].astype(int) - want8.astype(int)).max()})"
        assert np.array_equal(X[k], R.to_float(want8)), f"{what}: float image"
        assert np.array_equal(y[k, 0], wantl), f"{what}: {int((y[k, 0] != wantl).sum())} labels differ"
    for t, a in zip(di + dl, imgs + labs):                      # the sources are unchanged
        assert np.array_equal(t.cpu().numpy(), a)
    return X8, y


@pytest.mark.parametrize("op", range(9), ids=lambda o: ["resize", "center_crop", "random_crop", "rotation", "masking",
                                                        "grayscale", "laplace", "blur", "contrast"][o])
def test_each_op_equals_the_restatement(A, op):
    imgs, labs = sources(op)
    for T, lut, fill in ((256, LUT, 0), (224, None, 255), (96, LUT, 2)):
        aug = A.Augmenter(target_size=T, label_lut=lut, label_fill=fill)
        plans = plans_for(A, op, T)
        X8, y = check_batch(A, aug, imgs, labs, plans, T, lut, fill)
        if op == A.MASKING:                                     # the op did something: a dropped cell zeroes image and label
            assert (X8[0].reshape(-1, 3).max(axis=1) == 0).sum() > 100
        if lut is not None:
            assert not (y == 255).any() and (y == 3).any()


def test_mixed_batch_and_determinism(A):
    imgs, labs = sources(77)
    aug = A.Augmenter(target_size=256, label_lut=LUT, seed=3)
    plans = aug.plan([a.shape[:2] for a in imgs] * 3)
    assert len({p.op for p in plans}) >= 4
    check_batch(A, aug, imgs * 3, labs * 3, plans, 256, LUT, 0)
    di = [torch.from_numpy(a).cuda() for a in imgs * 3]
    dl = [torch.from_numpy(a).cuda() for a in labs * 3]
    a1 = aug.apply(di, dl, plans, out="both")
    a2 = aug.apply(di, dl, plans, out="both")
    for u, v in zip(a1, a2):
        assert torch.equal(u, v)                                # the same plan twice: identical bytes
    Xf, yf = aug.apply(di, dl, plans)                           # the float-only form writes the same values
    assert torch.equal(Xf, a1[0]) and torch.equal(yf, a1[2])
    aug.reseed()
    X1, y1 = aug(di, dl)
    aug.reseed()
    X2, y2 = aug(di, dl)
    assert torch.equal(X1, X2) and torch.equal(y1, y2) and torch.equal(X1, Xf)


def test_one_batch_is_at_most_two_launches(A, monkeypatch):
    from image_segmentation_amd import _lib
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    imgs, labs = sources(5)
    di = [torch.from_numpy(a).cuda() for a in imgs] * 4
    dl = [torch.from_numpy(a).cuda() for a in labs] * 4
    aug = A.Augmenter(seed=0)
    plans = aug.plan([tuple(t.shape[:2]) for t in di])
    assert {A.ROTATION, A.BLUR} & {p.op for p in plans}
    aug.apply(di, dl, plans)
    assert sorted(calls) == ["segk_aug_prefilter", "segk_aug_resample"]
    calls.clear()
    A.Augmenter(ops=(A.RESIZE, A.GRAYSCALE, A.CONTRAST), seed=0)(di, dl)
    assert calls == ["segk_aug_resample"]
    calls.clear()
    A.merge_pairs(di[:1] * 3, dl[:1] * 3, di[:1] * 3, dl[:1] * 3)
    assert calls == ["segk_aug_merge"]
    torch.cuda.synchronize()


def test_merge_equals_the_reference_golden(A, gold):
    names = [n for n in gold["merge.names"] if not bool(gold[f"merge.{n}.skipped"])]
    a = [[torch.from_numpy(gold[f"merge.{n}.{k}"]).cuda() for n in names] for k in ("img1", "lab1", "img2", "lab2")]
    X, X8, y = A.merge_pairs(a[0], a[1], a[2], a[3], target_size=256, out="both")
    torch.cuda.synchronize()
    assert X.shape == (len(names), 3, 256, 256) and y.shape == (len(names), 1, 256, 256) and y.dtype == torch.int64
    for k, n in enumerate(names):
        want = gold[f"merge.{n}.image"]
        assert np.array_equal(X8[k].cpu().numpy(), want), n
        assert np.array_equal(X[k].cpu().numpy(), R.to_float(want)), n
        assert np.array_equal(y[k, 0].cpu().numpy(), gold[f"merge.{n}.label"].astype(np.int64)), n
    _, yl = A.merge_pairs(a[0], a[1], a[2], a[3], label_lut=LUT)
    assert torch.equal(yl, torch.where(y == 255, torch.full_like(y, 3), y))
    n = [m for m in gold["merge.names"] if bool(gold[f"merge.{m}.skipped"])][0]
    b = [[torch.from_numpy(gold[f"merge.{n}.{k}"]).cuda()] for k in ("img1", "lab1", "img2", "lab2")]
    with pytest.raises(ValueError, match="orientations"):
        A.merge_pairs(*b)


def test_class_weights_and_colour_map_equal_the_reference_golden(A, gold):
    got = A.convert_rgb_label_to_classes(torch.from_numpy(gold["rgb.in"]).cuda())
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), gold["rgb.out"])
    labs = [gold[f"cw.label{k}"] for k in range(int(gold["cw.nlabels"]))]
    dev = [torch.from_numpy(a).cuda() for a in labs]
    for n in gold["cw.names"]:
        kw = json.loads(str(gold[f"cw.{n}.args"]))
        want = gold[f"cw.{n}.weights"]
        w = A.class_weights(dev, **kw)
        assert w.dtype == torch.float32 and np.array_equal(w.numpy(), want), (n, w, want)
        # int64 labels, host labels and a loader of (image, label) batches count the same
        assert np.array_equal(A.class_weights([t.long() for t in dev], **kw).numpy(), want), n
        assert np.array_equal(A.class_weights([(None, [torch.from_numpy(a)]) for a in labs], **kw).numpy(), want), n
        counts = A.class_counts(dev, kw["num_classes"], kw.get("ignore_index")).cpu().numpy()
        assert np.array_equal(counts, R.class_weights(labs, kw["num_classes"], kw.get("ignore_index"))[0]), n
    big = torch.from_numpy(np.random.default_rng(0).integers(0, 256, 3_000_001).astype(np.uint8)).cuda()
    c = A.class_counts([big, big], 4, 7).cpu().numpy()           # the counter accumulates across calls, exactly
    assert np.array_equal(c, 2 * R.class_weights([big.cpu().numpy()], 4, 7)[0])


def test_augmented_batches_drive_train_loop(A):
    import image_segmentation_amd as seg
    from image_segmentation_amd import training
    from oracle.fill import fill_module
    training.VERBOSE = False
    imgs, labs = sources(9)
    loader = [([torch.from_numpy(a) for a in imgs[:4]], [torch.from_numpy(a) for a in labs[:4]]) for _ in range(2)]
    batches = A.AugmentedBatches(loader, A.Augmenter(target_size=64, label_lut=LUT, seed=1))
    assert len(batches) == 2
    for X, y in batches:
        assert X.shape == (4, 3, 64, 64) and X.dtype == torch.float32 and X.is_cuda
        assert y.shape == (4, 1, 64, 64) and y.dtype == torch.int64 and int(y.max()) <= 3 and int(y.min()) >= 0
        assert 0.0 <= float(X.min()) and float(X.max()) <= 1.0
    m = seg.unet(3, 4)
    fill_module(m, 1000)
    m.cuda()
    before = m.output.weight.detach().clone()
    loss = training.train_loop(batches, m, seg.CrossEntropyLoss(), torch.optim.AdamW(m.parameters(), weight_decay=0.01), 1,
                               torch.device("cuda"))
    assert np.isfinite(loss) and loss > 0
    assert torch.isfinite(m.output.weight).all() and not torch.equal(m.output.weight, before)
