"""GPU (-m gpu): what the whole prediction surface does, as a record -- every route of Segmenter (single view, merged
views, tiles; with labels, clean=, temperature=, heat-maps and points) and calibration.fit_temperature on three tiny
images, compared with tests/golden/segmenter_trace.json.

Per case the record holds
  * the launch trace: every _lib.call in order, as [entry, args...]; an argument whose argtype in _lib.SIGNATURES is
    c_void_p is recorded only as "ptr" / "null" (None or 0), every other argument as its value -- no address is recorded;
  * per Prediction the SHA-1 of the bytes of mask, raw_mask, color, counts, confusion and confidence (null where the field is
    None), meta, and whether scores / components are set; for fit_temperature its to_json().

The models are stock-torch stubs with literal weights, so no digest depends on a BLAS choice.  The fixture is a record of
the commit BEFORE the routes were folded into shared helpers: the Python that drives the kernels may be
rearranged, the launches and the bytes may not change.

Set SEGK_SEGMENTER_TRACE_OUT=<file> to write the record there instead of comparing."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_trace.json")
C = 3
W_A = [[1.0, -1.0, 0.25], [-1.0, 1.0, 0.25], [-0.25, -0.25, 1.0]]
W_B = [[0.5, 0.25, -0.75], [-0.5, 0.75, 0.0], [0.25, -0.5, 0.5]]
V_A = [0.5, -0.25, 1.0]
V_B = [-0.5, 0.75, 0.25]

_RECORD = {}


class Stub(torch.nn.Module):
    """y[n,c] = sum_k w[c,k] x[n,k]: a 1x1 convolution spelled with elementwise ops"""

    def __init__(self, w):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(w, dtype=torch.float32))
        self.batches = []

    def forward(self, x):
        self.batches.append(int(x.shape[0]))
        return (x.unsqueeze(1) * self.w.view(1, C, 3, 1, 1)).sum(2)


class Stub2(torch.nn.Module):
    """The two-input form: the heat-map h [n,1,T,T] adds h v[c]"""

    def __init__(self, w, v):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(w, dtype=torch.float32))
        self.v = torch.nn.Parameter(torch.tensor(v, dtype=torch.float32))

    def forward(self, x, h):
        return (x.unsqueeze(1) * self.w.view(1, C, 3, 1, 1)).sum(2) + h * self.v.view(1, C, 1, 1)


def _grid(H, W):
    return np.meshgrid(np.arange(H), np.arange(W), indexing="ij")


def _u8_image(H, W, cin):
    y, x = _grid(H, W)
    mul = [(37, 11, 5), (13, 53, 90), (7, 29, 170), (3, 5, 40)]
    return np.stack([(x * a + y * b + c) % 256 for a, b, c in mul[:cin]], axis=-1).astype(np.uint8)


def _float_image(H, W):
    y, x = _grid(H, W)
    return torch.from_numpy(np.stack([((x * 5 + y * 3 + c * 7) % 11) / 10.0 for c in range(3)]).astype(np.float32))


def _label(H, W):
    y, x = _grid(H, W)
    lab = (x + 2 * y) % 3
    lab[(x + y) % 5 == 0] = 255
    return lab.astype(np.int64)


def _heat_u8(H, W):
    y, x = _grid(H, W)
    return torch.from_numpy(((x * 19 + y * 41) % 256).astype(np.uint8))


def _heat_float(H, W):
    y, x = _grid(H, W)
    return torch.from_numpy((((x * 3 + y * 7) % 13) / 12.0).astype(np.float32)).unsqueeze(0)


SIZES = [(5, 7), (9, 20), (6, 6)]


def images():
    """uint8 [5,7,3], uint8 [9,20,4] (RGBA: the cin == 4 path), float [3,6,6]"""
    return [_u8_image(5, 7, 3), _u8_image(9, 20, 4), _float_image(6, 6)]


def labels():
    return [_label(5, 7), torch.from_numpy(_label(9, 20)), torch.from_numpy(_label(6, 6)).unsqueeze(0)]


POINTS = [(2, 3), [(1, 1), (4, 10)], (0, 5)]            # one click, two clicks, one click
TILE_ORDER = [0, 2, 1]                                  # [5x7, 6x6, 9x20]: 1, 1 and 6 tiles


def take(seq, order):
    return [seq[k] for k in order]


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import image_segmentation_amd as s
    from image_segmentation_amd import _lib
    _lib.load()
    yield s
    out = os.environ.get("SEGK_SEGMENTER_TRACE_OUT")
    if out and _RECORD:
        with open(out, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in _RECORD.items())
                    + "\n}\n")


@pytest.fixture
def trace(monkeypatch):
    from image_segmentation_amd import _lib
    calls, real = [], _lib.call

    def call(name, *args):
        types = _lib.SIGNATURES[name][1]
        assert len(types) == len(args), name
        row = [name]
        for t, a in zip(types, args):
            if t is ctypes.c_void_p:
                row.append("null" if a is None or a == 0 else "ptr")
            else:
                row.append(float(a) if isinstance(a, (float, np.floating)) else int(a))
        calls.append(row)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", call)
    return calls


def sha(t):
    return None if t is None else hashlib.sha1(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def describe(preds):
    return [{"mask": sha(p.mask), "raw_mask": sha(p.raw_mask), "color": sha(p.color), "counts": sha(p.counts),
             "confusion": sha(p.confusion), "confidence": sha(p.confidence), "meta": p.meta,
             "scores": p.scores is not None, "components": p.components is not None} for p in preds]


def check(name, calls, result):
    got = json.loads(json.dumps({"calls": calls, "result": result}))
    if os.environ.get("SEGK_SEGMENTER_TRACE_OUT"):
        _RECORD[name] = got
        return
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]], "the launch order changed"
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"launch {k}"
    assert got["result"] == want["result"]


def models(two_input, n=1):
    if two_input:
        return [Stub2(w, v).cuda() for w, v in ((W_A, V_A), (W_B, V_B))][:n]
    return [Stub(w).cuda() for w in (W_A, W_B)][:n]


def prompt_kw(prompt, order=(0, 1, 2)):
    if prompt == "heat_u8":
        return {"heatmaps": [_heat_u8(*SIZES[k]) for k in order]}
    if prompt == "heat_float":
        return {"heatmaps": [_heat_float(*SIZES[k]) for k in order]}
    if prompt == "points":
        return {"points": take(POINTS, order)}
    return {}


PROMPTS = [None, "heat_u8", "heat_float", "points"]
TTA = dict(flips=("", "h", "v"), sizes=(16, 24))


# ---- 1. single view -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,kw", [("bilinear", {}), ("nearest", {"interpolation": "nearest"}),
                                        ("clean", {"clean": dict(min_area=2)})])
def test_single_view(seg, trace, variant, kw):
    s = seg.Segmenter(models(False)[0], target_size=16, batch_size=2, **kw)
    preds = s(images(), labels=labels())
    assert all(p.confidence is None and p.scores is None for p in preds)
    if variant == "bilinear":       # the stub's weights separate the classes: no image is one class everywhere
        assert all(len(torch.unique(p.mask)) > 1 for p in preds)
    check(f"single/{variant}", trace, describe(preds))


@pytest.mark.parametrize("prompt", PROMPTS[1:])
def test_single_view_two_input(seg, trace, prompt):
    s = seg.Segmenter(models(True)[0], target_size=16, batch_size=2)
    preds = s(images(), labels=labels(), **prompt_kw(prompt))
    check(f"single/{prompt}", trace, describe(preds))


# ---- 2. merged views ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prompt,clean", [(None, None), (None, dict(min_area=2))] + [(p, None) for p in PROMPTS[1:]])
def test_merged(seg, trace, prompt, clean):
    s = seg.Segmenter(models(prompt is not None, 2), target_size=16, batch_size=2, tta=seg.TTA(**TTA), model_weights=(2, 1),
                      temperature=(0.5, 2.0), return_scores=True, clean=clean)
    preds = s(images(), labels=labels(), **prompt_kw(prompt))
    assert all(p.confidence is not None and p.scores is not None for p in preds)
    check(f"merged/{prompt}/{'clean' if clean else 'plain'}", trace, describe(preds))


def test_merged_one_view(seg, trace):
    s = seg.Segmenter(models(False)[0], target_size=16, batch_size=2, return_scores=True)
    assert s._merged and len(s._views) == 1
    preds = s(images())
    check("merged/one_view", trace, describe(preds))


# ---- 3. tiles -------------------------------------------------------------------------------------------------------------------

def test_tile_plan():
    from image_segmentation_amd import tiles
    counts = [len(tiles.tile_axis(H, 8, 2)) * len(tiles.tile_axis(W, 8, 2)) for H, W in take(SIZES, TILE_ORDER)]
    assert counts == [1, 1, 6]


@pytest.mark.parametrize("variant,kw", [("labels", {}), ("clean_temperature", {"clean": dict(min_area=2), "temperature": 1.5})])
def test_tiles(seg, trace, variant, kw):
    model = models(False)[0]
    s = seg.Segmenter(model, target_size=16, batch_size=4, tiles=dict(size=8, overlap=2), **kw)
    preds = s(take(images(), TILE_ORDER), labels=take(labels(), TILE_ORDER))
    assert model.batches == [2, 4, 2]       # the first two images share a forward, the third runs alone in two
    assert [p.meta["tiles"] for p in preds] == [(1, 1), (1, 1), (2, 3)]
    check(f"tiles/{variant}", trace, describe(preds))


@pytest.mark.parametrize("prompt", PROMPTS[1:])
def test_tiles_two_input(seg, trace, prompt):
    s = seg.Segmenter(models(True)[0], target_size=16, batch_size=4, tiles=dict(size=8, overlap=2))
    preds = s(take(images(), TILE_ORDER), labels=take(labels(), TILE_ORDER), **prompt_kw(prompt, TILE_ORDER))
    check(f"tiles/{prompt}", trace, describe(preds))


# ---- 5. fit_temperature -------------------------------------------------------------------------------------------------------

def test_fit_temperature(seg, trace):
    from image_segmentation_amd.calibration import fit_temperature
    fit = fit_temperature(models(False)[0], images(), labels(), target_size=16, temps=(0.5, 1.0, 2.0), batch_size=2)
    assert fit.pixels > 0
    check("fit_temperature", trace, fit.to_json())
