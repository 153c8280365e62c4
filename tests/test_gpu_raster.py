"""MI355X: label rasterisation (image_segmentation_amd/raster.py, csrc/raster.hip) against the restatement of DESIGN.md 3.18 in
tests/raster_reference.py -- EXACT equality of every label map of every case of tests/raster_cases.py.  The output buffer
starts as 0xFF bytes and is larger than the plan needs: the gaps between the images and the slack behind them must still be
0xFF afterwards.  Every case runs twice and on a side stream with identical bytes.  Then the loop the feature closes, on the
device: rasterize(shapes_from_vectors(vectorize(mask))) is the mask again.  There is nothing to tolerance: the arithmetic is
integer and the definition makes the result unique."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_cases as RC                                                          # noqa: E402
import vector_cases as VC                                                          # noqa: E402
from test_raster_host import plan_of, to_shapes                                    # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 777


def run_plan(plan, fill, stream=None):
    """one launch into a 0xFF-filled buffer with slack -> the whole buffer as a NumPy array"""
    from image_segmentation_amd import raster as R
    dev = torch.device("cuda:0")
    out = torch.full((plan["out_bytes"] + SLACK,), 0xFF, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
        blob = R.launch(plan, out, fill, dev)
    torch.cuda.synchronize()
    del blob
    return out.cpu().numpy()


@pytest.mark.parametrize("name", RC.NAMES)
def test_every_case_equals_the_restatement(name):
    images, fill = RC.CASES[name]
    plan, refs = plan_of(name), RC.reference(name)
    want = np.full(plan["out_bytes"] + SLACK, 0xFF, np.uint8)
    for off, ref in zip(plan["out_off"], refs):
        want[off:off + ref.size] = ref.reshape(-1)
    got = run_plan(plan, fill)
    for i, (off, ref) in enumerate(zip(plan["out_off"], refs)):
        g = got[off:off + ref.size].reshape(ref.shape)
        bad = np.argwhere(g != ref)
        assert bad.size == 0, f"{name}: image {i}: {len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}: {g[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
    assert np.array_equal(got, want), f"{name}: bytes outside the images were written"
    again, side = run_plan(plan, fill), run_plan(plan, fill, torch.cuda.Stream())
    assert np.array_equal(again, got) and np.array_equal(side, got)


def test_public_calls_views_and_devices():
    import image_segmentation_amd as seg
    images, fill = RC.CASES["batch"]
    labs = seg.rasterize_batch([to_shapes(s) for s, _ in images], [hw for _, hw in images], fill=fill)
    assert [tuple(t.shape) for t in labs] == [hw for _, hw in images] and all(t.dtype == torch.uint8 and t.is_cuda for t in labs)
    assert labs[0].untyped_storage().data_ptr() == labs[2].untyped_storage().data_ptr()           # views of ONE buffer
    for t, ref in zip(labs, RC.reference("batch")):
        assert t.is_contiguous() and np.array_equal(t.cpu().numpy(), ref)
    shapes, hw = RC.CASES["mixed"][0][0]
    one = seg.rasterize(to_shapes(shapes), hw, fill=RC.CASES["mixed"][1], device="cuda:0")
    assert np.array_equal(one.cpu().numpy(), RC.reference("mixed")[0])
    assert (seg.rasterize([], (3, 5), fill=200).cpu().numpy() == 200).all()


@pytest.mark.parametrize("name", VC.MASK_NAMES)
@pytest.mark.parametrize("connectivity", [4, 8])
def test_rasterize_inverts_vectorize(name, connectivity):
    """on the device: the mask -> rings -> the mask, classes outside `classes` come back as fill"""
    import image_segmentation_amd as seg
    mask, classes = VC.MASKS[name]
    H, W = mask.shape
    full = VC.reference(name, connectivity)
    dev = torch.from_numpy(mask.copy()).cuda()
    vec = seg.vectorize(dev, connectivity=connectivity, classes=classes, max_components=1 << 15, max_edges=max(4, int(full["totals"][1])))
    assert vec.complete
    labelled = np.isin(mask, list(classes) if classes is not None else list(range(8)))
    for fill in (0, 255):
        lab = seg.rasterize(seg.shapes_from_vectors(vec), (H, W), fill=fill)
        assert np.array_equal(lab.cpu().numpy(), np.where(labelled, mask, fill).astype(np.uint8)), (name, connectivity, fill)


@pytest.mark.parametrize("name", ["hole_island", "nested3", "frame", "stripes70x130", "noise0.1_3c_120x77"])
def test_compressed_coco_round_trip(name):
    """to_coco(compressed=True) -> shapes_from_coco -> rasterize: objects with holes travel as RLE strings, the others as polygons"""
    import json
    import image_segmentation_amd as seg
    mask, classes = VC.MASKS[name]
    dev = torch.from_numpy(mask.copy()).cuda()
    vec = seg.vectorize(dev, classes=classes, max_edges=4 * mask.size)     # the stripes have more edges than the default holds
    cats = {c: 10 + c for c in classes}
    anns = json.loads(json.dumps(vec.to_coco(1, cats, compressed=True)))
    kinds = {type(a["segmentation"]) for a in anns}
    assert all(isinstance(a["segmentation"]["counts"], str) for a in anns if isinstance(a["segmentation"], dict))
    if name in ("hole_island", "nested3", "frame"):
        assert dict in kinds
    if name in ("hole_island", "stripes70x130", "noise0.1_3c_120x77"):
        assert list in kinds
    lab = seg.rasterize(seg.shapes_from_coco(anns, {10 + c: c for c in classes}), mask.shape)
    assert np.array_equal(lab.cpu().numpy(), mask)
    plain = seg.rasterize(seg.shapes_from_coco(vec.to_coco(1, cats), {10 + c: c for c in classes}), mask.shape)
    assert torch.equal(plain, lab)


def test_rasterize_tool_writes_label_pngs(tmp_path):
    """tools/rasterize.py: a COCO file written from two masks (polygons, RLE lists and RLE strings) comes back as their PNGs"""
    import json
    import subprocess
    from PIL import Image
    import image_segmentation_amd as seg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    coco = {"categories": [{"id": 11, "name": "cat"}, {"id": 12, "name": "dog"}, {"id": 13, "name": "edge"}], "images": [], "annotations": []}
    masks = {}
    for i, name in enumerate(("hole_island", "noise0.1_3c_120x77")):
        mask, classes = VC.MASKS[name]
        masks[f"im{i}"] = mask
        coco["images"].append({"id": i + 1, "file_name": f"dir/im{i}.jpg", "height": mask.shape[0], "width": mask.shape[1]})
        vec = seg.vectorize(torch.from_numpy(mask.copy()).cuda(), classes=classes)
        coco["annotations"] += vec.to_coco(i + 1, {1: 11, 2: 12, 3: 13}, first_id=len(coco["annotations"]) + 1, compressed=bool(i))
    json.dump(coco, open(tmp_path / "c.json", "w"))
    out = tmp_path / "labels"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "rasterize.py"), str(tmp_path / "c.json"), "--categories",
                        "cat=1,12=2,edge=3", "--out", str(out), "--batch", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for stem, mask in masks.items():
        assert np.array_equal(np.asarray(Image.open(out / f"{stem}.png")), mask), stem


def test_outputs_feed_augmenter_and_class_weights():
    """a rasterize_batch output is a label of the training path as it stands: no copy to the host in between"""
    import image_segmentation_amd as seg
    from image_segmentation_amd import augment as A
    images, fill = RC.CASES["batch"]
    sizes = [hw for _, hw in images]
    labs = seg.rasterize_batch([to_shapes(s) for s, _ in images], sizes, fill=1)
    rng = np.random.default_rng(5)
    imgs = [torch.from_numpy(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).cuda() for hw in sizes]
    aug = seg.Augmenter(target_size=32, ops=[A.RESIZE], seed=3)
    X, y = aug(imgs, labs)
    assert X.shape == (3, 3, 32, 32) and y.shape == (3, 1, 32, 32) and y.dtype == torch.int64 and y.is_cuda
    refs = [np.where(r == 8, 1, r) for r in RC.reference("batch")]             # the same shapes over fill 1
    for i, ((H, W), ref) in enumerate(zip(sizes, refs)):
        assert np.array_equal(labs[i].cpu().numpy(), ref)
        S = max(H, W)                                                           # pad to the square (centred, 0), nearest resize
        canvas = np.zeros((S, S), np.uint8)
        canvas[(S - H) // 2:(S - H) // 2 + H, (S - W) // 2:(S - W) // 2 + W] = ref
        idx = np.arange(32) * S // 32
        assert np.array_equal(y[i, 0].cpu().numpy(), canvas[idx][:, idx].astype(np.int64)), i
    w = seg.class_weights(labs, num_classes=5)
    hist = sum(np.bincount(r.reshape(-1), minlength=5)[:5] for r in refs)
    w2 = seg.class_weights([torch.from_numpy(r.copy()).cuda() for r in refs], num_classes=5)
    assert torch.equal(torch.as_tensor(w), torch.as_tensor(w2)) and hist.sum() == sum(h * w_ for h, w_ in sizes)
