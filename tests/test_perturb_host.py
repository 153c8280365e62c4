"""CPU: the host half of image_segmentation_amd/robustness.py -- levels, tables, plans, argument checks -- and the NumPy
restatement of the perturbation arithmetic (tests/perturb_reference.py): its blur pass against scipy's mirror correlation and
the identity the LDS kernel relies on (extend once by k, then k plain passes == k reflecting passes).  No kernel is launched."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perturb_reference as R                                                      # noqa: E402
from image_segmentation_amd import robustness as P                                 # noqa: E402

SMALL = [(1, 1), (1, 7), (2, 3), (5, 4), (13, 70)]
LUT_KINDS = ("contrast_increase", "contrast_decrease", "brightness_increase", "brightness_decrease")


def test_default_levels_are_eight_by_ten_and_start_at_the_identity():
    assert len(P.PERTURBATIONS) == 8 and set(P.DEFAULT_LEVELS) == set(P.PERTURBATIONS)
    sizes = [(5, 4), (13, 70)]
    for kind in P.PERTURBATIONS:
        lv = P.DEFAULT_LEVELS[kind]
        assert len(lv) == 10
        plan = P.perturb_plan(kind, lv[0], sizes, seed=3)
        assert plan.identity
        if plan.table is not None and plan.code == P.LUT:
            assert np.array_equal(plan.table, np.arange(256))
        if plan.table is not None and plan.code == P.GAUSS_NOISE:
            assert not plan.table.any()
        if kind == "gaussian_blur":
            assert plan.entry == "segk_perturb_blur" and plan.code == 0
        if kind == "salt_and_pepper":
            assert all(p[0] == 0 for p in plan.params)
        if kind == "occlusion":
            assert all(p[2] == 0 for p in plan.params)
        for x in lv[1:]:
            assert not P.perturb_plan(kind, x, sizes, seed=3).identity
    assert P.DEFAULT_LEVELS["gaussian_noise"] == tuple(range(0, 20, 2))
    assert P.DEFAULT_LEVELS["gaussian_blur"] == tuple(range(10))
    assert P.DEFAULT_LEVELS["contrast_increase"] == (1.0, 1.01, 1.02, 1.03, 1.04, 1.05, 1.10, 1.15, 1.20, 1.25)
    assert P.DEFAULT_LEVELS["contrast_decrease"] == (1.0, 0.95, 0.90, 0.85, 0.80, 0.60, 0.40, 0.30, 0.20, 0.10)
    for kind in ("brightness_increase", "brightness_decrease", "occlusion"):
        assert P.DEFAULT_LEVELS[kind] == tuple(range(0, 50, 5))
    assert np.allclose(P.DEFAULT_LEVELS["salt_and_pepper"], np.arange(10) * 0.02, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", LUT_KINDS)
def test_value_lut_is_monotone_clipped_and_equals_the_restatement(kind):
    for level in P.DEFAULT_LEVELS[kind]:
        t = P.value_lut(kind, level)
        assert t.dtype == np.uint8 and t.shape == (256,) and not t.flags.writeable
        assert (np.diff(t.astype(np.int64)) >= 0).all()
        assert np.array_equal(t, R.lut(kind, level))
    assert P.value_lut("brightness_increase", 45)[-1] == 255 and P.value_lut("brightness_increase", 45)[0] == 45
    assert P.value_lut("brightness_decrease", 45)[0] == 0 and P.value_lut("brightness_decrease", 45)[255] == 210
    assert P.value_lut("contrast_increase", 1.25)[255] == 255 and P.value_lut("contrast_increase", 1.25)[100] == 125
    assert P.value_lut("contrast_decrease", 0.1)[255] == 26       # rint(25.5) is 26 (half to even)


@pytest.mark.parametrize("std", [0, 2, 4, 10, 18, 3.7])
def test_gauss_table_is_antisymmetric_with_the_right_spread(std):
    t = P.gauss_table(std)
    assert t.dtype == np.int16 and t.shape == (4096,) and not t.flags.writeable
    assert np.array_equal(t, -t[::-1])
    assert (np.diff(t.astype(np.int64)) >= 0).all()
    assert np.array_equal(t, R.gauss_table(std))
    if std >= 2:
        assert abs(float(np.sqrt(np.mean(t.astype(np.float64) ** 2))) - std) <= 0.01 * std
    else:
        assert not t.any()


def test_one_blur_pass_equals_scipy_mirror_correlation():
    rng = np.random.default_rng(0)
    w = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.int32)
    for H, W in SMALL + [(64, 64), (37, 200)]:
        a = rng.integers(0, 256, (H, W), dtype=np.int32)
        want = (scipy.ndimage.correlate(a, w, mode="mirror") + 8) >> 4
        assert np.array_equal(R.blur_pass(a), want), (H, W)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    got = R.blur(img, 1)
    for c in range(3):
        assert np.array_equal(got[..., c], (scipy.ndimage.correlate(img[..., c].astype(np.int32), w, mode="mirror") + 8) >> 4)


@pytest.mark.parametrize("H,W", SMALL)
def test_extend_once_then_plain_passes_equals_reflecting_passes(H, W):
    rng = np.random.default_rng(H * 100 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    for k in (1, 2, 9):
        assert np.array_equal(R.blur_extend_once(img, k), R.blur(img, k)), k
    assert np.array_equal(R.blur(img, 0), img)


def test_occlusion_plans_stay_inside_the_image():
    sizes = SMALL + [(64, 64), (65, 129), (37, 200)]
    for edge in (0, 5, 45):
        for seed in range(20):
            plan = P.perturb_plan("occlusion", edge, sizes, seed=seed)
            assert plan.entry == "segk_perturb_point" and plan.code == P.OCCLUDE
            for (H, W), (y0, x0, e) in zip(sizes, plan.params):
                assert e == min(edge, H, W)
                assert 0 <= y0 <= H - e and 0 <= x0 <= W - e
    # the corner moves with the seed and with the image
    a = P.perturb_plan("occlusion", 5, [(37, 200)] * 8, seed=0).params
    assert len(set(a)) > 1


def test_plans_are_a_function_of_their_arguments():
    sizes = [(5, 4), (13, 70), (37, 200)]
    for kind in P.PERTURBATIONS:
        level = P.DEFAULT_LEVELS[kind][3]
        a, b = P.perturb_plan(kind, level, sizes, seed=11), P.perturb_plan(kind, level, sizes, seed=11)
        assert a.seeds == b.seeds and a.params == b.params and a.code == b.code and a.entry == b.entry
        assert (a.table is None) == (b.table is None) and (a.table is None or np.array_equal(a.table, b.table))
        c = P.perturb_plan(kind, level, sizes, seed=12)
        assert c.seeds != a.seeds
        assert len(set(a.seeds)) == len(sizes)
    assert P.cell_seed(0, 1, 2) == P.cell_seed(0, 1, 2)
    cells = {P.cell_seed(s, k, l) for s in range(3) for k in range(8) for l in range(10)}
    assert len(cells) == 240 and all(0 <= c < 1 << 64 for c in cells)
    assert P.perturb_plan("salt_and_pepper", 0.02, sizes).params[0][0] == int(np.floor(0.02 * (1 << 24)))


def test_bad_arguments_raise():
    sizes = [(5, 4)]
    with pytest.raises(ValueError, match="unknown perturbation"):
        P.perturb_plan("fog", 1, sizes)
    for kind, level in [("gaussian_blur", 10), ("gaussian_blur", 1.5), ("gaussian_blur", -1), ("gaussian_noise", -2),
                        ("gaussian_noise", float("nan")), ("contrast_increase", 0.5), ("contrast_decrease", 1.5),
                        ("brightness_increase", 300), ("brightness_decrease", 2.5), ("occlusion", -5),
                        ("salt_and_pepper", 1.5), ("salt_and_pepper", "much"), ("occlusion", None)]:
        with pytest.raises(ValueError, match="level"):
            P.perturb_plan(kind, level, sizes)
    with pytest.raises(ValueError):
        P.perturb_plan("occlusion", 5, [(0, 4)])
    with pytest.raises(ValueError):
        P.value_lut("occlusion", 5)
    with pytest.raises(TypeError, match="uint8"):
        P.perturb([np.zeros((5, 4, 3), np.float32)], "occlusion", 5)
    with pytest.raises(TypeError, match="uint8"):
        P.perturb([torch.zeros((5, 4, 3))], "occlusion", 5)
    with pytest.raises(ValueError, match=r"\[H,W,3\|4\]"):
        P.perturb([np.zeros((5, 4, 2), np.uint8)], "occlusion", 5)
    with pytest.raises(ValueError, match="unknown perturbation"):
        P.perturb([np.zeros((5, 4, 3), np.uint8)], "fog", 5)
    with pytest.raises(ValueError, match="level"):
        P.perturb([np.zeros((5, 4, 3), np.uint8)], "gaussian_blur", 10)
    with pytest.raises(TypeError):
        P.perturb([], "occlusion", 5)


def test_perturb_has_no_cpu_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.perturb([np.zeros((5, 4, 3), np.uint8)], "occlusion", 5)


def test_restatement_pointwise_properties():
    """The restatement itself: level-0 parameters are the identity, occlusion zeroes exactly its square, the hash is the
    splitmix64 finaliser (first outputs of the published generator for seed 0 after one increment)."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (13, 70, 3), dtype=np.uint8)
    assert np.array_equal(R.gaussian_noise(img, 0, 9), img)
    assert np.array_equal(R.salt_and_pepper(img, 0.0, 9), img)
    assert np.array_equal(R.occlude(img, 3, 4, 0), img)
    o = R.occlude(img, 3, 4, 5)
    assert not o[3:8, 4:9].any() and np.array_equal(o[:3], img[:3]) and np.array_equal(o[:, 9:], img[:, 9:])
    # splitmix64 with state 0: the first output is the finaliser of 0x9E3779B97F4A7C15 = hash(seed=1, i=0)
    assert int(R.splitmix(1, np.zeros(1, np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert P._mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF


def test_perturb_kernels_do_not_spill_and_keep_their_loads_in_flight():
    """Compiled-code check (hipcc cross-compiles here) with the project's own two tools: no register spills, no scratch, no
    load that waits for itself in any kernel of csrc/perturb.hip."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def tool(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    rows = tool("spill_report").report("perturb")
    assert len(rows) == 5, rows                                     # four pointwise instances and the blur
    for r in rows:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
    for n_ser, n_loads, _, name in tool("serialized_loads").scan("perturb"):
        assert n_ser == 0, f"{name}: {n_ser} of {n_loads} loads wait for themselves"


def test_command_line_tool_checks_its_arguments(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "robustness.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--only" in r.stdout and "--target-size" in r.stdout and "--out" in r.stdout
    r = subprocess.run([sys.executable, tool, "--checkpoint", "none.pt", "--images", str(tmp_path), "--labels", str(tmp_path),
                        "--out", str(tmp_path / "s.json"), "--only", "fog"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "unknown perturbation 'fog'" in r.stderr
    assert not (tmp_path / "s.json").exists()
