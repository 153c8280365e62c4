"""CPU: the host half of image_segmentation_amd/augment.py -- table builders, planning, argument checks -- and the parts of
the NumPy restatement (tests/augment_reference.py) that are pinned against the reference's own code through
tests/golden/augment_ref.npz (tools/gen_golden_augment.py): the pair merge of cell 17, convert_rgb_label_to_classes and
calculate_class_weights.  No kernel is launched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_reference as R                                                      # noqa: E402
from image_segmentation_amd import augment as A                                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "augment_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---------------------------------------------------------------------------------------------- table builders
@pytest.mark.parametrize("S,T", [(500, 256), (375, 256), (256, 256), (31, 256), (1, 256), (8192, 224), (250, 96), (96, 96)])
def test_cubic_rows_sum_to_2048(S, T):
    idx, coef = A.cubic_table(S, T)
    assert idx.dtype == np.int32 and coef.dtype == np.int16 and idx.shape == (T,) and coef.shape == (T, 4)
    assert (coef.astype(np.int64).sum(axis=1) == 2048).all()
    assert np.abs(coef.astype(np.int64)).sum(axis=1).max() <= 2816          # the bound the 32-bit accumulator relies on
    assert idx.min() >= -1 and idx.max() <= S - 1
    assert not idx.flags.writeable and not coef.flags.writeable
    ridx, rcoef = R.cubic(S, T)
    assert np.array_equal(idx, ridx) and np.array_equal(coef, rcoef)


def test_cubic_identity():
    idx, coef = A.cubic_table(256, 256)
    assert np.array_equal(idx, np.arange(256))
    assert (coef == np.array([0, 2048, 0, 0])).all()


def test_contrast_lut_is_monotone():
    for alpha in (0.2, 0.37, 0.6, 1.0, 1.7):
        lut = A.contrast_lut(alpha)
        assert lut.dtype == np.uint8 and lut.shape == (256,) and (np.diff(lut.astype(int)) >= 0).all()
        assert lut[127] == 127
        assert np.array_equal(lut, R.contrast_table(alpha))
    assert np.array_equal(A.contrast_lut(1.0), np.arange(256))


def test_laplace_table_is_antisymmetric():
    for b in (25.5, 51.0, 76.5):
        t = A.laplace_table(b).astype(int)
        assert t.shape == (4096,) and np.array_equal(t, -t[::-1])
        assert (np.diff(t) >= 0).all() and t[2048] >= 0 and abs(t).max() < 700
        assert np.array_equal(t, R.laplace(b))


@pytest.mark.parametrize("H,W", [(375, 500), (500, 333), (17, 31), (1, 1), (64, 64)])
@pytest.mark.parametrize("theta", [90.0, 180.0, 270.0])
def test_rotation_by_right_angles_is_a_permutation(H, W, theta):
    Ha, Wa, Aq = A.rotation_plan(H, W, theta)
    assert (Ha, Wa) == ((W, H) if theta != 180.0 else (H, W))
    y, x = np.indices((Ha, Wa), dtype=np.int64)
    SX, SY = Aq[0] * x + Aq[1] * y + Aq[2], Aq[3] * x + Aq[4] * y + Aq[5]
    assert ((SX & 0xFFFF) == 0).all() and ((SY & 0xFFFF) == 0).all()          # no fraction: every output is one source pixel
    sx, sy = SX >> 16, SY >> 16
    assert sx.min() == 0 and sx.max() == W - 1 and sy.min() == 0 and sy.max() == H - 1
    assert len(np.unique(sy * W + sx)) == H * W                                # each source pixel exactly once
    if theta == 90.0:
        assert np.array_equal(sx, y) and np.array_equal(sy, H - 1 - x)
    elif theta == 180.0:
        assert np.array_equal(sx, W - 1 - x) and np.array_equal(sy, H - 1 - y)
    else:
        assert np.array_equal(sx, W - 1 - y) and np.array_equal(sy, x)
    # and the restatement moves the pixels accordingly
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    lab = rng.integers(0, 3, (H, W)).astype(np.uint8)
    oi, ol = R.rotate(img, lab, theta, 9)
    assert np.array_equal(oi, img[sy, sx]) and np.array_equal(ol, lab[sy, sx])
    assert R.rotation(H, W, theta) == (Ha, Wa, list(Aq))


def test_rotation_plan_fits_the_output():
    for theta in (45.0, 123.4, 315.0):
        Ha, Wa, Aq = A.rotation_plan(375, 500, theta)
        assert R.rotation(375, 500, theta) == (Ha, Wa, list(Aq))
        assert max(Ha, Wa) <= 626 and min(Ha, Wa) >= 375


# ---------------------------------------------------------------------------------------------- planning
SIZES = [(375, 500), (500, 333), (256, 256), (17, 31), (1, 1)] * 4


def test_plan_is_reproducible_and_reseed_rewinds():
    a, b = A.Augmenter(seed=11), A.Augmenter(seed=11)
    p1, p2 = a.plan(SIZES), a.plan(SIZES)
    assert p1 == b.plan(SIZES)
    assert p1 != p2                                   # the next epoch differs
    a.reseed()
    assert a.plan(SIZES) == p1 and a.plan(SIZES) == p2
    assert A.Augmenter(seed=12).plan(SIZES) != p1
    a.reseed(12)
    assert a.plan(SIZES) == A.Augmenter(seed=12).plan(SIZES)


def test_plan_draws_valid_parameters():
    plans = A.Augmenter(seed=5).plan([(375, 500)] * 400)
    assert {p.op for p in plans} == set(A.ALL_OPS)
    for p in plans:
        y, x, h, w = p.window
        if p.op == A.CENTER_CROP:
            assert p.window == (0, 62, 375, 375)
        elif p.op == A.RANDOM_CROP:
            assert h == w == 250 and 0 <= y <= 125 and 0 <= x <= 250
        elif p.op == A.ROTATION:
            assert 45.0 <= p.theta <= 315.0 and (h, w) == A.rotation_plan(375, 500, p.theta)[:2] and (y, x) == (0, 0)
        else:
            assert p.window == (0, 0, 375, 500)
        if p.op == A.CONTRAST:
            assert 0.2 <= p.alpha <= 0.6
        if p.op == A.LAPLACE:
            assert 25.5 <= p.b <= 76.5
        assert 0 <= p.seed < 1 << 32
    only = A.Augmenter(ops=(A.RESIZE, A.BLUR), probs=(0.0, 1.0), seed=1).plan([(8, 8)] * 20)
    assert {p.op for p in only} == {A.BLUR}


# ---------------------------------------------------------------------------------------------- pinned against the reference
@pytest.mark.parametrize("n_in,n_out", [(500, 103), (375, 154), (333, 102), (1, 5), (5, 1), (358, 81), (442, 163), (120, 256),
                                        (8192, 255), (97, 97)])
def test_merge_index_tables_equal_pil_nearest(n_in, n_out):
    Image = pytest.importorskip("PIL.Image")
    idx = np.arange(n_in)
    src = np.zeros((1, n_in, 3), np.uint8)
    src[0, :, 0], src[0, :, 1] = idx % 256, idx // 256
    for vertical in (False, True):
        s = np.ascontiguousarray(src.transpose(1, 0, 2)) if vertical else src
        size = (2, n_out) if vertical else (n_out, 2)
        got = np.array(Image.fromarray(s).resize(size, Image.Resampling.NEAREST)).astype(int)
        got = got[:, 0] if vertical else got[0]
        pil = got[:, 0] + 256 * got[:, 1]
        assert np.array_equal(A._pil_nearest(n_in, n_out), pil)
        assert np.array_equal(R.pil_nearest_index(n_in, n_out), pil)


def test_merge_plan_tables_against_pil_resize_and_paste():
    """the four tables of a plan, applied as a gather, equal PIL's resize + paste + paste of an index image"""
    Image = pytest.importorskip("PIL.Image")
    for sizes in (((120, 90), (100, 81)), ((375, 500), (333, 500)), ((40, 300), (30, 200)), ((31, 31), (17, 31))):
        tables, (fh1, fw1, fh2, fw2) = A.merge_plan(sizes, 256)
        canvas = Image.new("RGB", (256, 256), (0, 0, 0))
        ims = []
        for k, (h, w) in enumerate(sizes):
            a = np.zeros((h, w, 3), np.uint8)
            a[..., 0], a[..., 1], a[..., 2] = (np.arange(h) % 251)[:, None], (np.arange(w) % 251)[None, :], k + 1
            ims.append(a)
        r1 = Image.fromarray(ims[0]).resize((fw1, fh1), Image.Resampling.NEAREST)
        r2 = Image.fromarray(ims[1]).resize((fw2, fh2), Image.Resampling.NEAREST)
        portrait = sizes[0][0] > sizes[0][1]
        strip = Image.new("RGB", (256, max(fh1, fh2)) if portrait else (max(fw1, fw2), 256), (0, 0, 0))
        strip.paste(r1, (0, 0))
        strip.paste(r2, (fw1, 0) if portrait else (0, fh1))
        canvas.paste(strip, ((256 - strip.width) // 2, (256 - strip.height) // 2))
        want = np.array(canvas)
        got = np.zeros((256, 256, 3), np.uint8)
        for k in range(2):
            ys, xs = tables[2 * k], tables[2 * k + 1]
            hit = (ys >= 0)[:, None] & (xs >= 0)[None, :]
            got[hit] = ims[k][np.clip(ys, 0, None)][:, np.clip(xs, 0, None)][hit]
        assert np.array_equal(got, want), sizes


def test_restatement_equals_the_reference_golden(gold):
    assert np.array_equal(R.rgb_to_classes(gold["rgb.in"]), gold["rgb.out"])
    seen = 0
    for n in gold["merge.names"]:
        a = [gold[f"merge.{n}.{k}"] for k in ("img1", "lab1", "img2", "lab2")]
        if bool(gold[f"merge.{n}.skipped"]):
            with pytest.raises(ValueError):
                R.merge(*a)
            with pytest.raises(ValueError, match="orientations"):
                A.merge_plan((a[0].shape[:2], a[2].shape[:2]), 256)
            continue
        im, lb = R.merge(*a)
        assert np.array_equal(im, gold[f"merge.{n}.image"]), n
        assert np.array_equal(lb, gold[f"merge.{n}.label"]), n
        seen += 1
    assert seen >= 6
    labs = [gold[f"cw.label{k}"] for k in range(int(gold["cw.nlabels"]))]
    for n in gold["cw.names"]:
        kw = json.loads(str(gold[f"cw.{n}.args"]))
        counts, w = R.class_weights(labs, kw["num_classes"], kw.get("ignore_index"), kw.get("unimportant_class_indices"),
                                    kw.get("normalize_target_sum", -1.0))
        assert w.dtype == np.float32 and np.array_equal(w, gold[f"cw.{n}.weights"]), n
        # the host half of the package on the same counts
        got = A.weights_from_counts(counts, kw.get("unimportant_class_indices"), kw.get("normalize_target_sum", -1.0))
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), gold[f"cw.{n}.weights"]), n


# ---------------------------------------------------------------------------------------------- errors, compiled code
def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from image_segmentation_amd import _lib
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a kernel entry was reached"))
    with pytest.raises(ValueError):
        A.Augmenter(target_size=0)
    with pytest.raises(ValueError):
        A.Augmenter(ops=())
    with pytest.raises(ValueError):
        A.Augmenter(ops=(99,))
    with pytest.raises(ValueError):
        A.Augmenter(probs=(0.5, 0.5))
    with pytest.raises(ValueError):
        A.Augmenter(label_lut=np.zeros(10, np.uint8))
    with pytest.raises(ValueError):
        A.Augmenter(label_fill=300)
    with pytest.raises(ValueError):
        A.make_plan(A.RANDOM_CROP, 30, 30, y1=20, x1=0)
    with pytest.raises(ValueError):
        A.make_plan(A.RESIZE, 0, 5)
    with pytest.raises(ValueError):
        A.Augmenter().plan([(9000, 10)])
    aug = A.Augmenter(seed=0)
    img, lab = torch.zeros((8, 6, 3), dtype=torch.uint8), torch.zeros((8, 6), dtype=torch.uint8)
    plan = [A.make_plan(A.RESIZE, 8, 6)]
    with pytest.raises(TypeError):
        aug.apply([img.float()], [lab], plan)
    with pytest.raises(TypeError):
        aug.apply([img], [lab.long()], plan)
    with pytest.raises(TypeError):
        aug.apply([img.numpy()], [lab], plan)
    with pytest.raises(TypeError):
        aug.apply([img], [lab], ["resize"])
    with pytest.raises(ValueError):
        aug.apply([img], [lab[:4]], plan)
    with pytest.raises(ValueError):
        aug.apply([img[:, :, :2]], [lab], plan)
    with pytest.raises(ValueError):
        aug.apply([img], [lab], plan * 2)
    with pytest.raises(ValueError):
        aug.apply([img], [lab], [A.make_plan(A.RESIZE, 6, 8)])
    with pytest.raises(ValueError):
        aug.apply([img], [lab], plan, out="half")
    with pytest.raises(RuntimeError, match="no CPU path"):
        aug.apply([img], [lab], plan)                                   # host tensors: refused, not computed on the CPU
    tall, wide = torch.zeros((9, 6, 3), dtype=torch.uint8), torch.zeros((6, 9, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="orientations"):
        A.merge_pairs([tall], [tall], [wide], [wide])
    with pytest.raises(ValueError):
        A.merge_pairs([tall], [tall], [tall, tall], [tall, tall])
    with pytest.raises(TypeError):
        A.merge_pairs([tall.float()], [tall], [tall], [tall])
    with pytest.raises(ValueError):
        A.class_weights([lab], 0)
    with pytest.raises(TypeError):
        A.class_weights([lab.float()], 3)
    with pytest.raises(TypeError):
        A.class_weights([lab], 3, ignore_index=2.5)
    with pytest.raises(ValueError):
        A.class_weights([], 3)
    with pytest.raises(ValueError):
        A.convert_rgb_label_to_classes(lab)
    with pytest.raises(TypeError):
        A.convert_rgb_label_to_classes(img.float())


def test_augment_unit_has_no_spills_and_no_serialized_loads():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "spill_report.py"), "--all", "augment"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("augment")]
    assert len(rows) >= 5, r.stdout                                     # every kernel of the unit was reported
    for ln in rows:
        assert " spill    0 scratch     0 " in ln, ln
    assert "0 kernel(s) with spills or scratch" in r.stdout
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import serialized_loads
    rows = serialized_loads.scan("augment")
    assert len(rows) >= 5
    for ser, n, unit, name in rows:
        assert ser <= 2, f"{name}: {ser} of {n} loads wait for themselves"
