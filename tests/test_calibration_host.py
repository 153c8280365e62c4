"""CPU: the host side of confidence calibration -- bins / ECE / MCE, the temperature grid and the parabola,
the ABI rows, the refusals that need no GPU, and what the NumPy restatement (tests/calibration_reference.py) itself says
about the inputs tests/test_gpu_calibration.py uses.  No kernel runs."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import calibration_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as s
    return s


def rel_of(seg, entries, C=2):
    """Reliability from {(class, q): (count, correct)}"""
    h = np.zeros((C, 256, 2), dtype=np.int64)
    for (c, q), v in entries.items():
        h[c, q] = v
    return seg.Reliability(torch.from_numpy(h), C), h


def test_ece_mce_on_hand_made_histograms(seg):
    # perfectly calibrated: q / 255 is the accuracy of every occupied confidence (single-confidence bins: n = 256)
    r, h = rel_of(seg, {(0, 255): (40, 40), (1, 51): (10, 2), (0, 153): (5, 3), (1, 0): (7, 0)})
    assert r.ece(256) == 0.0 and r.mce(256) == 0.0
    assert r.ece(256) == CR.ece(h.sum(0), 256)
    # everything in q = 255 and all wrong
    r, h = rel_of(seg, {(0, 255): (12, 0), (1, 255): (3, 0)})
    for n in (1, 10, 15, 256):
        assert r.ece(n) == 1.0 and r.mce(n) == 1.0
    assert [c["ece"] for c in r.per_class()] == [1.0, 1.0] and [c["pixels"] for c in r.per_class()] == [12, 3]
    # empty: None, not a division by zero
    r, h = rel_of(seg, {})
    assert r.ece() is None and r.mce() is None and all(b["conf"] is None and b["acc"] is None for b in r.bins())
    assert [c["ece"] for c in r.per_class()] == [None, None] and CR.ece(h.sum(0)) is None
    # a mixed one against the restatement, every bin count; the per-class split adds up; JSON goes through
    rng = np.random.default_rng(5)
    h = rng.integers(0, 50, size=(3, 256, 2))
    h[:, :, 1] = np.minimum(h[:, :, 1], h[:, :, 0])
    r = seg.Reliability(torch.from_numpy(h), 3)
    for n in (1, 10, 15, 256):
        assert r.ece(n) == pytest.approx(CR.ece(h.sum(0), n), abs=1e-15) and r.mce(n) == pytest.approx(CR.mce(h.sum(0), n), abs=1e-15)
        for b, w in zip(r.bins(n), CR.bins(h.sum(0), n)):
            assert (b["lo"], b["hi"], b["count"], b["correct"]) == w[:4] and b["conf"] == pytest.approx(w[4], abs=1e-15)
    for c, row in enumerate(r.per_class(10)):
        assert row["ece"] == pytest.approx(CR.ece(h[c], 10), abs=1e-15)
    out = json.loads(json.dumps(r.to_json()))
    assert out["pixels"] == int(h[:, :, 0].sum()) and len(out["bins"]) == 15 and len(out["per_class"]) == 3
    both = r + r
    assert np.array_equal(both.counts(), 2 * h) and np.array_equal(r.counts(), h) and both.ece() == pytest.approx(r.ece(), abs=1e-15)
    with pytest.raises(ValueError, match="int64"):
        seg.Reliability(torch.zeros((3, 256, 2)), 3)
    with pytest.raises(ValueError, match="bins"):
        r.bins(257)


@pytest.mark.parametrize("n", [1, 10, 15, 256])
def test_bin_edges(seg, n):
    r, _ = rel_of(seg, {(0, q): (1, 0) for q in range(256)})
    rows = r.bins(n)
    assert len(rows) == n and rows[0]["lo"] == 0 and rows[-1]["hi"] == 255 and sum(b["count"] for b in rows) == 256
    for b, row in enumerate(rows):
        assert all(q * n // 256 == b for q in range(row["lo"], row["hi"] + 1)) and row["count"] == row["hi"] - row["lo"] + 1
        if b:
            assert row["lo"] == rows[b - 1]["hi"] + 1
        assert row["conf"] == pytest.approx(sum(q / 255 for q in range(row["lo"], row["hi"] + 1)) / row["count"], abs=1e-15)
    if n == 256:
        assert all(row["lo"] == row["hi"] for row in rows)
    if n == 10:                                                    # 256 is no multiple of 10: bin b starts at ceil(25.6 b)
        assert [row["lo"] for row in rows] == [0, 26, 52, 77, 103, 128, 154, 180, 205, 231]


def test_default_grid(seg):
    t = seg.default_temperatures()
    assert len(t) == 17 and t == sorted(t) and t[8] == 1.0 and t[0] == 0.25 and t[-1] == 4.0
    inv = seg.inverse_temperatures(t)
    assert inv.dtype == np.float32 and inv[8] == 1.0 and np.array_equal(inv, CR.inverse_temperatures(t))


def test_refine_temperature(seg):
    t = seg.default_temperatures()
    for T0 in (0.3, 1.0, 1.2345, 3.0):                             # a parabola in log T: the vertex comes back exactly
        nll = [0.7 + 0.4 * (math.log(x) - math.log(T0)) ** 2 for x in t]
        T, i, end = seg.refine_temperature(t, nll)
        assert not end and T == pytest.approx(T0, rel=1e-12) and i == int(np.argmin(nll))
        assert T == pytest.approx(CR.refine(t, nll)[0], rel=1e-9)
    assert seg.refine_temperature(t, [float(j) for j in range(17)]) == (0.25, 0, True)          # falling towards the low end
    assert seg.refine_temperature(t, [float(-j) for j in range(17)]) == (4.0, 16, True)
    assert seg.refine_temperature([1.0], [0.3]) == (1.0, 0, True)
    assert seg.refine_temperature(t, [None] * 17) == (None, None, False)
    flat = [1.0] * 17
    assert seg.refine_temperature(t, flat)[:2] == (0.25, 0)                                     # the first minimum
    # uneven spacing: the three-point formula, not the equal-step one
    tt, T0 = [0.5, 0.8, 2.0, 3.0], 1.1
    T, i, end = seg.refine_temperature(tt, [(math.log(x) - math.log(T0)) ** 2 for x in tt])
    assert (i, end) == (1, False) and T == pytest.approx(T0, rel=1e-12)
    with pytest.raises(ValueError):
        seg.refine_temperature([1.0, 2.0], [0.1])


def test_fit_record_from_counts(seg):
    t = seg.default_temperatures()
    hist = np.zeros((17, 256, 2), dtype=np.int64)
    hist[:, 200] = (100, 80)
    nll = [0.5 + 0.3 * (math.log(x) - math.log(1.5)) ** 2 for x in t]
    fx = [int(round(v * 65536 * 98)) for v in nll]
    fit = seg.fit_from_counts(t, hist, fx, [2] * 17, 100)
    assert fit.pixels == 100 and fit.index == int(np.argmin(nll)) and not fit.at_grid_end
    assert fit.temperature == pytest.approx(1.5, rel=1e-4) and fit.nll_at_1 == pytest.approx(nll[8], abs=1e-6)
    assert fit.ece_at_1 == pytest.approx(abs(0.8 - 200 / 255), abs=1e-15) and fit.nonfinite == [2] * 17
    assert json.loads(json.dumps(fit.to_json()))["temperatures"] == t
    none = seg.fit_from_counts(t, np.zeros((17, 256, 2)), [0] * 17, [0] * 17, 0)                 # no pixels: None, no division
    assert none.temperature is None and none.nll == [None] * 17 and none.ece == [None] * 17 and none.pixels == 0


def test_the_two_entries_in_header_and_binding(seg):
    from image_segmentation_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "segk.h")).read(), flags=re.S)
    for name, nargs in (("segk_calib_hist", 9), ("segk_calib_temps", 19)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
    assert int(re.search(r"#define\s+SEGK_MAX_TEMPS\s+(\d+)", txt).group(1)) == _lib.MAX_TEMPS == 32
    assert float(re.search(r"#define\s+SEGK_CALIB_NLL_MAX\s+([\d.]+)f", txt).group(1)) == CR.NLL_MAX


def test_refusals_without_a_gpu(seg):
    m = seg.unet(3, 4)
    for bad in (0, -1.0, float("nan"), float("inf"), (1.0, 2.0)):
        with pytest.raises(ValueError, match="temperature"):
            seg.Segmenter(m, temperature=bad)
    with pytest.raises(ValueError, match="temperature"):
        seg.Segmenter([m, seg.unet(3, 4)], temperature=(1.0, 2.0, 3.0))
    assert seg.Segmenter(m)._inv_T is None and seg.Segmenter(m, temperature=None, tta=seg.TTA())._inv_T is None
    assert seg.Segmenter(m, temperature=2.0)._inv_T == [0.5]
    assert seg.Segmenter([m, seg.unet(3, 4)], temperature=(3.0, 0.7))._inv_T == [float(np.float32(1 / 3.0)), float(np.float32(1 / 0.7))]
    assert seg.Segmenter(m, temperature=1.5, tiles=seg.Tiles(size=32))._inv_T == [float(np.float32(1 / 1.5))]
    p = seg.PromptModel(clip=seg.unet(3, 4))
    for kw in (dict(), dict(tta=seg.TTA()), dict(tiles=seg.Tiles(size=32))):
        with pytest.raises(ValueError, match='outputs="probs"'):
            seg.Segmenter(p, temperature=2.0, **kw)
    with pytest.raises(ValueError, match='outputs="probs"'):
        seg.Segmenter(m, temperature=2.0, tta=seg.TTA(), outputs="probs")
    # reliability: a Prediction without a confidence map, and the routes that set one
    pred = seg.Prediction(torch.zeros((4, 4), dtype=torch.uint8), None, torch.zeros(4), None, {})
    with pytest.raises(ValueError, match="tta=.*tiles=.*return_scores=True"):
        seg.reliability([pred], [torch.zeros((4, 4), dtype=torch.int64)], 4)
    pred.confidence = torch.zeros((4, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.reliability([pred], [torch.zeros((4, 4), dtype=torch.int64)], 4)
    with pytest.raises(ValueError, match="num_classes"):
        seg.reliability([pred], [None], 9)
    with pytest.raises(ValueError, match="label maps"):
        seg.reliability([pred], [], 4)
    # fit_temperature
    img, lab = [torch.zeros((3, 8, 8))], [torch.zeros((8, 8), dtype=torch.int64)]
    with pytest.raises(ValueError, match="returns probabilities"):
        seg.fit_temperature(p, img, lab)
    with pytest.raises(ValueError, match="one model"):
        seg.fit_temperature([m, m], img, lab)
    clip = seg.ClipUNet.__new__(seg.ClipUNet)                       # the size check reads encoder.config.image_size alone
    torch.nn.Module.__init__(clip)
    clip.encoder = types.SimpleNamespace(config=types.SimpleNamespace(image_size=224))
    with pytest.raises(ValueError, match="224 x 224 inputs only"):
        seg.fit_temperature(clip, img, lab, target_size=64)
    for temps in ([], [1.0] * 33, [1.0, 0.0], [float("nan")]):
        with pytest.raises(ValueError, match="temps"):
            seg.fit_temperature(m, img, lab, temps=temps)
    with pytest.raises(ValueError, match="label maps"):
        seg.fit_temperature(m, img, [], target_size=16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.fit_temperature(m, img, lab, target_size=16)


@pytest.mark.parametrize("h,w,C", [(64, 64, 4), (37, 53, 3), (20, 30, 2), (33, 65, 8)])
def test_synthetic_recovery(seg, h, w, C):
    """labels drawn from softmax(g), logits 2^0.75 g: the float64 restatement's grid argmin is 2^0.75 (identity resolution)"""
    rng = np.random.default_rng(h * w + C)
    T = max(h, w)
    g = rng.normal(scale=2, size=(C, T, T))
    p = np.exp(g - g.max(0))
    p /= p.sum(0)
    lab = (rng.random((T, T))[None] > np.cumsum(p, 0)).sum(0).clip(0, C - 1)[:h, :w]
    slot = (2 ** 0.75 * g).astype(np.float32)
    temps = seg.default_temperatures()
    geo = dict(pad_top=0, pad_left=0, nh=h, nw=w)
    s = CR.sweep(slot, geo, (h, w), lab, C, CR.inverse_temperatures(temps), -1, 0, np.float64)
    nll = [CR.mean_nll(s, j) for j in range(17)]
    assert temps[int(np.argmin(nll))] == 2 ** 0.75 == temps[11]
    # the package's host arithmetic on the float32 restatement's integer outputs finds the same point
    s32 = CR.sweep(slot, geo, (h, w), lab, C, CR.inverse_temperatures(temps), -1, 0, np.float32)
    fit = seg.fit_from_counts(temps, s32["hist"], s32["nll_fx"], s32["nonfinite"], s32["valid"])
    assert fit.index == 11 and not fit.at_grid_end and temps[10] < fit.temperature < temps[12]
    assert max(abs(a - b) for a, b in zip(fit.nll, nll)) < 1e-4 and fit.nll_best < fit.nll_at_1 and fit.pixels == h * w


def gpu_test_cases():
    """the small images in full; the large one (3 s per restatement) bilinear at two class counts"""
    for C in CR.CLASSES:
        for mode in (0, 1):
            for T in CR.SIZES:
                for n, shape in enumerate(CR.SHAPES):
                    if shape[0] * shape[1] <= 100000:
                        yield n, T, C, mode, 32
    for C in (2, 8):
        for T in CR.SIZES:
            yield 1, T, C, 0, 17


def test_inputs_of_the_gpu_test_keep_the_restatement_inside_the_caps(seg):
    """float32 restatement against float64 on the GPU test's inputs: at most 1 pixel in 20 ambiguous, its own histogram inside
    2 x ambiguous per column, its own mean NLL inside d_nll + 2^-17"""
    worst = 0.0
    for n, T, C, mode, K in gpu_test_cases():
        shape, geo, slot, lab, ign = CR.case(n, T, C)
        inv = seg.inverse_temperatures(CR.TABLE[:K])                  # the table the package uploads
        assert np.array_equal(inv, CR.inverse_temperatures(CR.TABLE[:K]))
        s64 = CR.sweep(slot, geo, shape, lab, C, inv, ign, mode, np.float64)
        s32 = CR.sweep(slot, geo, shape, lab, C, inv, ign, mode, np.float32)
        d_nll, d_p, d_z = CR.distances(s32, s64)
        amb = CR.ambiguous(s64, d_p, d_z).sum(axis=1)
        valid = s64["valid"]
        assert valid == s32["valid"] == int(CR.valid_labels(lab, C, ign).sum()) > 0 and s32["nonfinite"] == [0] * K
        assert (amb * 20 <= valid).all(), (n, T, C, mode, float(amb.max() / valid))
        worst = max(worst, float(amb.max() / valid))
        moved = np.abs(s32["hist"] - s64["hist"]).sum(axis=1)
        assert (moved <= 2 * amb[:, None]).all(), (n, T, C, mode)
        for j in range(K):
            assert abs(s32["nll_fx"][j] / 65536 / valid - CR.mean_nll(s64, j)) <= d_nll[j] + 2.0 ** -17
        if C == 1:
            assert (s32["hist"][:, 255, 0] == valid).all() and s32["nll_fx"] == [0] * K
        else:
            assert s64["hist"][0, 255, 0] > 0                             # the top bin is in use (at 1/T = 4)
    print(f"largest ambiguous share {worst:.4f}")
