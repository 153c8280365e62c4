"""CPU: the host half of the point prompts (image_segmentation_amd/prompts.py, Segmenter(points=), tools/predict.py
--point) -- the two look-up tables against the fixture captured from the reference's own functions
(tests/golden/prompt_points.npz, tools/gen_golden_prompts.py), the label remap table, the argument errors raised before
any launch, and the compiled-code bar of csrc/prompt.hip (hipcc cross-compiles without a GPU): no spills, no scratch, at
most two loads that wait for themselves in the make and heat-map kernels -- the bar tests/test_inference_host.py sets."""
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.fill import fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as s
    return s


def test_heat_tables_against_the_reference(seg, golden):
    g = golden("prompt_points")
    w, q, R = seg.heat_tables(3.0, 256, 256)
    assert R == 27 and len(w) == len(q) == 2 * R * R + 1
    assert w.dtype == np.float64 and q.dtype == np.uint8
    d2 = np.arange(len(w))
    assert np.array_equal(w, np.exp(-d2 / 18.0))                    # bit for bit: the reference's expression
    assert np.count_nonzero(q) == 100 and np.all(q[:100] > 0) and not q[100:].any()
    assert math.floor(18.0 * math.log(255)) == 99
    ref = g["q_by_d2"]                                              # read back from the reference's heat-maps; -1: never seen
    seen = ref >= 0
    assert seen.sum() > 100
    n = min(len(ref), len(q))
    assert np.array_equal(q[:n][seen[:n]], ref[:n][seen[:n]].astype(np.uint8))
    assert not ref[n:][seen[n:]].any()


@pytest.mark.parametrize("sigma,H,W", [(1.5, 256, 256), (6.0, 512, 512), (3.0, 33, 47), (0.5, 1, 1)])
def test_heat_tables_defining_inequalities(seg, sigma, H, W):
    w, q, R = seg.heat_tables(sigma, H, W)
    assert H * W * math.exp(-R * R / (2 * sigma**2)) <= 1e-12
    assert R == 0 or H * W * math.exp(-(R - 1) ** 2 / (2 * sigma**2)) > 1e-12           # the smallest such radius
    assert len(w) == 2 * R * R + 1
    d2 = np.arange(len(w))
    assert np.array_equal(w, np.exp(-d2 / (2 * sigma**2)))
    assert np.array_equal(q, (w * 255).astype(np.uint8))
    last = math.floor(2 * sigma**2 * math.log(255))
    assert not q[last + 1:].any() and (last >= len(q) or q[last] >= 1)


def test_trimap_table(seg, golden):
    g = golden("prompt_points")
    raw = g["trimap96x128.labels"].astype(np.int64)
    assert set(np.unique(raw)) == {0, 1, 2, 255}
    assert np.array_equal(seg.TRIMAP_TO_PROMPT[raw], g["trimap96x128.remapped"])
    t = seg.TRIMAP_TO_PROMPT
    assert t.shape == (256,) and t.dtype == np.uint8
    assert [int(t[i]) for i in (0, 1, 2, 3, 255)] == [1, 2, 3, 1, 1] and int(t.astype(int).sum()) == 8


def test_sampler_argument_errors(seg):
    lab = torch.zeros((2, 16, 20), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.PromptSampler()(lab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.PromptSampler()([lab[0], lab[1, :8]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.PromptSampler()(lab, centers=np.zeros((2, 4, 2), dtype=np.int64))
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            seg.PromptSampler(sigma=bad)
    with pytest.raises(ValueError, match="sigma"):
        seg.heat_tables(0.0, 8, 8)
    with pytest.raises(ValueError, match="candidates"):
        seg.PromptSampler(candidates=0)
    for bad in (0, 8):
        with pytest.raises(ValueError, match="per_image"):
            seg.PromptSampler(per_image=bad)
    assert seg.PromptSampler(per_image=7).per_image == 7
    with pytest.raises(ValueError, match="lut"):
        seg.PromptSampler(lut=np.zeros(255, dtype=np.uint8))
    s = seg.PromptSampler()
    with pytest.raises(TypeError, match="int64"):
        s(lab.to(torch.uint8))
    with pytest.raises(ValueError, match=r"\[B,H,W\]"):
        s(lab[0])
    with pytest.raises(ValueError, match=r"expected integers \[2,K,2\]"):
        s(lab, centers=np.zeros((2, 4, 3), dtype=np.int64))
    with pytest.raises(ValueError, match=r"expected integers \[2,K,2\]"):
        s(lab, centers=np.zeros((1, 4, 2), dtype=np.int64))
    with pytest.raises(ValueError, match=r"expected integers \[2,K,2\]"):
        s(lab, centers=np.zeros((2, 4, 2)))
    for y, x in ((16, 0), (0, 20), (-1, 0)):
        c = np.zeros((2, 4, 2), dtype=np.int64)
        c[1, 3] = (y, x)
        with pytest.raises(ValueError, match="outside the 16 x 20 image"):
            s(lab, centers=c)
    with pytest.raises(ValueError, match=r"centers\[1\]: a centre lies outside the 8 x 20 image"):
        s([lab[0], lab[1, :8]], centers=[np.zeros((4, 2), dtype=np.int64), np.full((4, 2), 9)])
    with pytest.raises(ValueError, match="1 centre sets for 2"):
        s([lab[0], lab[1]], centers=[np.zeros((4, 2), dtype=np.int64)])


def test_segmenter_points_argument_errors(seg):
    img = fill((3, 20, 30), 1, 0, 1)
    u8 = np.zeros((20, 30, 3), dtype=np.uint8)
    pm = seg.PromptModel(clip=seg.unet(3, 4))
    with pytest.raises(ValueError, match="takes the image alone"):
        seg.Segmenter(seg.unet(3, 4))([img], points=[(3, 4)])
    with pytest.raises(ValueError, match="either heatmaps or points"):
        seg.Segmenter(pm)([img], heatmaps=[fill((1, 20, 30), 2, 0, 1)], points=[(3, 4)])
    with pytest.raises(ValueError, match="2 point sets for 1 images"):
        seg.Segmenter(pm)([img], points=[(3, 4), (5, 6)])
    for im in (img, u8):
        for bad in ((20, 0), (0, 30), (-1, 5), [(3, 4), (19, 30)]):
            with pytest.raises(ValueError, match=r"points\[0\]: a point lies outside the 20 x 30 image"):
                seg.Segmenter(pm)([im], points=[bad])
    with pytest.raises(ValueError, match="one integer"):
        seg.Segmenter(pm)([img], points=[(3.5, 4.0)])
    with pytest.raises(ValueError, match="one integer"):
        seg.Segmenter(pm)([img], points=[(3, 4, 5)])
    with pytest.raises(ValueError, match="sigma"):
        seg.Segmenter(pm, sigma=0)
    with pytest.raises(RuntimeError, match="no CPU path"):          # well-formed: reaches the device requirement
        seg.Segmenter(pm, target_size=32)([img], points=[[(3, 4), (19, 29)]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.predict(pm, [u8], points=[(0, 0)], target_size=32)
    with pytest.raises(ValueError, match="outside the 8 x 8 image"):
        seg.point_heatmap((8, 0), 8, 8, device="cpu")


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_prompt_kernels_compiled_code():
    rows = _load_tool("serialized_loads").scan("prompt")
    names = [r[3] for r in rows]
    assert sum("prompt_scores_kernel" in n for n in names) == 1
    assert sum("prompt_make_kernel" in n for n in names) == 2 and sum("prompt_heatmap_kernel" in n for n in names) == 2
    for n_ser, n_loads, _, name in rows:
        if "prompt_make_kernel" in name or "prompt_heatmap_kernel" in name:
            assert n_ser <= 2, f"{name}: {n_ser} of {n_loads} loads wait for themselves"
    rep = _load_tool("spill_report").report("prompt")
    assert len(rep) == 5
    for r in rep:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r


def test_abi_has_the_three_entries(seg):
    from image_segmentation_amd import _lib, build
    assert "prompt.hip" in build.SOURCES
    for name in ("segk_prompt_scores", "segk_prompt_make", "segk_prompt_heatmap"):
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib.C.c_int


def test_predict_tool_names_point():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--point" in r.stdout and "Y,X" in r.stdout
