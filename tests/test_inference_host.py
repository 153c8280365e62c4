"""CPU: the host half of the prediction surface (image_segmentation_amd/inference.py, tools/predict.py) -- checkpoint
handling (reference segmentation_webapp/app.py:65-84), the palette / class-name tables (app.py:187-208), the argument
errors Segmenter raises before any launch, and the compiled-code bar of the two prediction kernels (csrc/predict.hip, csrc/resize.hip)
(hipcc cross-compiles without a GPU): no spills, no scratch, at most two loads that wait for themselves -- the bar
tests/test_tools.py sets for the other streaming kernels."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

from oracle import unet_ref
from oracle.fill import fill, fill_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as s
    return s


def _reference_state():
    r = unet_ref.unet(3, 4)
    fill_module(r, 1000)
    return r.state_dict()


@pytest.mark.parametrize("form", ["model_state_dict", "state_dict", "bare_module_prefix"])
def test_load_checkpoint_formats(seg, tmp_path, form):
    from image_segmentation_amd.inference import load_checkpoint
    sd = _reference_state()
    if form == "bare_module_prefix":
        obj = {"module." + k: v for k, v in sd.items()}
    else:
        obj = {form: sd, "epoch": 3}
    path = str(tmp_path / "ckpt.pt")
    torch.save(obj, path)
    m = seg.unet(3, 4).train()
    out = load_checkpoint(m, path)
    assert out is m and not m.training and not any(c.training for c in m.modules())
    got = m.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k


def test_load_checkpoint_strict(seg, tmp_path):
    from image_segmentation_amd.inference import load_checkpoint
    sd = _reference_state()
    sd.pop("output.bias")
    path = str(tmp_path / "short.pt")
    torch.save({"model_state_dict": sd}, path)
    with pytest.raises(RuntimeError, match="output.bias"):
        load_checkpoint(seg.unet(3, 4), path)
    m = load_checkpoint(seg.unet(3, 4), path, strict=False)
    assert not m.training


def test_tables(seg):
    assert seg.COLOR_MAP == {0: (0, 0, 0), 1: (255, 0, 0), 2: (0, 255, 0), 3: (0, 0, 255)}
    assert seg.CLASS_NAMES == {"standard": {0: "Background", 1: "Cat", 2: "Dog", 3: "Boundary"},
                               "prompt_model": {0: "Deactivated", 1: "Background+Boundary", 2: "Cat", 3: "Dog"}}
    from image_segmentation_amd import inference
    assert inference.Segmenter is seg.Segmenter and inference.predict is seg.predict


def test_segmenter_has_no_cpu_path(seg):
    m = seg.unet(3, 4)
    s = seg.Segmenter(m, target_size=32)
    assert s.num_classes == 4
    with pytest.raises(RuntimeError, match="no CPU path"):
        s([fill((3, 20, 30), 1, 0, 1)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.predict(m, [fill((3, 20, 30), 1, 0, 1)], target_size=32)


def test_segmenter_argument_errors(seg):
    with pytest.raises(ValueError, match="palette has 3 rows, the model has 4 classes"):
        seg.Segmenter(seg.unet(3, 4), palette=[(0, 0, 0), (1, 1, 1), (2, 2, 2)])
    with pytest.raises(ValueError, match="at most 8"):
        seg.Segmenter(seg.unet(3, 9), palette=None)
    with pytest.raises(ValueError, match="palette"):
        seg.Segmenter(seg.unet(3, 2), palette=[(0, 0, 0, 0), (1, 1, 1, 1)])
    assert seg.Segmenter(seg.unet(3, 4), palette=None).num_classes == 4
    img = fill((3, 20, 30), 1, 0, 1)
    with pytest.raises(ValueError, match="takes the image alone"):
        seg.Segmenter(seg.unet(3, 4))([img], heatmaps=[fill((1, 20, 30), 2, 0, 1)])
    pm = seg.PromptModel(clip=seg.unet(3, 4))
    with pytest.raises(ValueError, match="pass heatmaps"):
        seg.Segmenter(pm)([img])
    with pytest.raises(ValueError, match="interpolation"):
        seg.Segmenter(seg.unet(3, 4), interpolation="bicubic")


def test_predict_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--checkpoint" in r.stdout and "--classes" in r.stdout and "IMG" in r.stdout


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_prediction_kernels_compiled_code():
    new = ("predict_mask_kernel", "resize_pad_u8_kernel")
    units = ("predict", "resize")          # predict_mask_kernel lives in csrc/predict.hip, resize_pad_u8_kernel in csrc/resize.hip
    rows = [r for u in units for r in _load_tool("serialized_loads").scan(u) if any(k in r[3] for k in new)]
    # 5 class counts x 2 modes x with/without labels, and 3 channel counts x 3 modes
    assert sum("predict_mask_kernel" in r[3] for r in rows) == 20 and sum("resize_pad_u8_kernel" in r[3] for r in rows) == 9
    for n_ser, n_loads, _, name in rows:
        assert n_ser <= 2, f"{name}: {n_ser} of {n_loads} loads wait for themselves"
    seen = 0
    for u in units:
        for r in _load_tool("spill_report").report(u):
            if any(k in r["name"] for k in new):
                seen += 1
                assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
    assert seen == 29
