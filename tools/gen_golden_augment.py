#!/usr/bin/env python3
"""Generate tests/golden/augment_ref.npz by running THE REFERENCE'S OWN code for the three parts of its data preparation
that run without imgaug:

  * utils.utils.convert_rgb_label_to_classes and utils.utils.calculate_class_weights -- utils/utils.py is loaded as a module
    with an empty four-module `torchvision` stub in sys.modules (its import line is the only use this needs);
  * combine_images_preserve_aspect_ratio, cell 17 of utils/augmentation.ipynb -- the notebook is read as JSON, the cell is
    parsed with `ast`, and only that FunctionDef is compiled into a namespace that holds PIL.Image, math, os, np, a silent
    print and the reference's convert_rgb_label_to_classes.  It reads and writes files, so the inputs go through lossless PNG
    files in a temporary directory.

Nothing of the reference's text is written anywhere; the fixture holds numbers only (the inputs, so that the tests need no
generator of their own, and the reference's outputs).  The generator refuses to write a fixture that lacks what the tests rely
on: a portrait and a landscape pair, a pair that needs the exact-fit adjustment, a mismatched pair the cell skips, a
one-channel label, all five label colours, the value 255 and the ignore_index in the class-weight cases.

Usage: python tools/gen_golden_augment.py --reference DIR      (or SEG_REFERENCE=DIR; CPU only)"""
import argparse
import ast
import importlib.util
import json
import math
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "augment_ref.npz")
MAX_BYTES = 744 * 1024
T = 256
PALETTE = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 0], [255, 255, 255], [128, 128, 0], [0, 0, 128]], np.uint8)


def reference_utils(ref):
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.transforms.v2"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    sys.modules["torchvision.transforms"].InterpolationMode = types.SimpleNamespace(BILINEAR="bilinear", NEAREST="nearest")
    spec = importlib.util.spec_from_file_location("reference_utils_utils", os.path.join(ref, "utils", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_combine(ref, convert):
    from PIL import Image
    nb = json.load(open(os.path.join(ref, "utils", "augmentation.ipynb")))
    want = "combine_images_preserve_aspect_ratio"
    for cell in nb["cells"]:
        src = "".join(cell["source"])
        if cell["cell_type"] != "code" or "def " + want not in src:
            continue
        defs = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == want]
        ns = {"Image": Image, "math": math, "os": os, "np": np, "print": lambda *a, **k: None,
              "convert_rgb_label_to_classes": convert}
        exec(compile(ast.Module(body=defs, type_ignores=[]), "<reference cell>", "exec"), ns)
        return ns[want]
    raise SystemExit("cell 17 (combine_images_preserve_aspect_ratio) was not found")


def blocky(rng, h, w, block, values):
    """[h,w,...]: blocks of `block` pixels drawn from `values` (compresses well, still exercises every index of a gather)"""
    gh, gw = -(-h // block), -(-w // block)
    pick = rng.integers(0, len(values), (gh, gw))
    return np.ascontiguousarray(np.kron(pick, np.ones((block, block), np.int64))[:h, :w].astype(np.int64))


def image(rng, h, w):
    """random colours in blocks of 3 x 3 pixels: an index of a gather that is off by one shows at every third position, and
    the file still compresses"""
    gh, gw = -(-h // 3), -(-w // 3)
    tint = rng.integers(0, 256, (gh, gw, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(tint, np.ones((3, 3, 1), np.uint8))[:h, :w])


def colour_label(rng, h, w):
    return PALETTE[blocky(rng, h, w, 5, PALETTE)]


def merge_cases(rng):
    """name -> (img1, lab1, img2, lab2)"""
    c = {}
    c["portrait"] = (image(rng, 120, 90), colour_label(rng, 120, 90), image(rng, 100, 81), colour_label(rng, 100, 81))
    c["landscape"] = (image(rng, 90, 120), colour_label(rng, 90, 120), image(rng, 75, 110), colour_label(rng, 75, 110))
    c["fullsize"] = (image(rng, 375, 500), colour_label(rng, 375, 500), image(rng, 333, 500), colour_label(rng, 333, 500))
    c["tall"] = (image(rng, 500, 333), colour_label(rng, 500, 333), image(rng, 400, 300), colour_label(rng, 400, 300))
    c["square_small"] = (image(rng, 31, 31), colour_label(rng, 31, 31), image(rng, 17, 31), colour_label(rng, 17, 31))
    c["wide"] = (image(rng, 40, 300), colour_label(rng, 40, 300), image(rng, 30, 200), colour_label(rng, 30, 200))
    grey = np.array([0, 1, 2, 128, 255], np.uint8)[blocky(rng, 64, 48, 4, range(5))]            # a one-channel label file
    c["grey_label"] = (image(rng, 64, 48), grey, image(rng, 70, 50), colour_label(rng, 70, 50))
    c["mismatch"] = (image(rng, 60, 40), colour_label(rng, 60, 40), image(rng, 40, 60), colour_label(rng, 40, 60))
    return c


def main():
    from PIL import Image
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("SEG_REFERENCE"), help="checkout of the reference project")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or SEG_REFERENCE) is required")
    ru = reference_utils(args.reference)
    combine = reference_combine(args.reference, ru.convert_rgb_label_to_classes)
    rng = np.random.default_rng(20240517)
    out = {}

    # 1. convert_rgb_label_to_classes
    rgb = colour_label(rng, 48, 64)
    rgb[0, :8] = rng.integers(0, 256, (8, 3))                     # a few colours off the palette
    rgb[1, 0], rgb[1, 1], rgb[1, 2] = (128, 0, 1), (0, 128, 128), (255, 255, 254)
    out["rgb.in"] = rgb
    out["rgb.out"] = ru.convert_rgb_label_to_classes(rgb)
    assert set(np.unique(out["rgb.out"])) == {0, 1, 2, 255}

    # 2. cell 17
    names, adjusted = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, (i1, l1, i2, l2) in merge_cases(rng).items():
            paths = []
            for k, a in enumerate((i1, l1, i2, l2)):
                p = os.path.join(tmp, f"{name}_{k}.png")
                Image.fromarray(a).save(p)
                paths.append(p)
            img = combine(paths[0], paths[2], None, False)
            lab = combine(paths[1], paths[3], None, True)
            names.append(name)
            for k, a in zip(("img1", "lab1", "img2", "lab2"), (i1, l1, i2, l2)):
                out[f"merge.{name}.{k}"] = a
            out[f"merge.{name}.skipped"] = np.array(img is None)
            if img is None:
                assert lab is None
                continue
            out[f"merge.{name}.image"] = np.array(img)
            out[f"merge.{name}.label"] = np.array(lab)
            assert out[f"merge.{name}.image"].shape == (T, T, 3) and out[f"merge.{name}.label"].shape == (T, T)
            (h1, w1), (h2, w2) = i1.shape[:2], i2.shape[:2]
            s = T / ((w1 + w2) if h1 > w1 else (h1 + h2))
            a, b = ((w1, w2) if h1 > w1 else (h1, h2))
            adjusted += math.ceil(a * s) + math.ceil(b * s) > T
    assert adjusted >= 2, "no pair needs the exact-fit adjustment"
    assert bool(out["merge.mismatch.skipped"]) and sum(bool(out[f"merge.{n}.skipped"]) for n in names) == 1
    out["merge.names"] = np.array(names)

    # 3. calculate_class_weights (source_type='dataset': label_source[i] -> (image, label))
    labs = [np.array([0, 1, 2, 255, 3], np.uint8)[blocky(rng, h, w, 3, range(5))] for h, w in ((40, 50), (33, 47), (64, 64))]
    labs.append(np.zeros((16, 16), np.uint8))
    for k, a in enumerate(labs):
        out[f"cw.label{k}"] = a
    out["cw.nlabels"] = np.array(len(labs))
    cw_cases = {"c4": dict(num_classes=4), "c3_ignore255": dict(num_classes=3, ignore_index=255),
                "c3_clamp": dict(num_classes=3), "c4_unimportant0": dict(num_classes=4, unimportant_class_indices=[0]),
                "c4_ignore255_bg_sum1": dict(num_classes=4, ignore_index=255, unimportant_class_indices=[0, 3],
                                             normalize_target_sum=1.0),
                "c5_ignore0": dict(num_classes=5, ignore_index=0)}
    ds = [(None, torch.from_numpy(a)) for a in labs]
    stdout = sys.stdout
    for name, kw in cw_cases.items():
        sys.stdout = open(os.devnull, "w")
        try:
            w = ru.calculate_class_weights(ds, source_type="dataset", **kw)
        finally:
            sys.stdout.close()
            sys.stdout = stdout
        assert w.dtype == torch.float32 and w.shape == (kw["num_classes"],)
        out[f"cw.{name}.weights"] = w.numpy()
        out[f"cw.{name}.args"] = np.array(json.dumps(kw))
    out["cw.names"] = np.array(list(cw_cases))
    assert any((a == 255).any() for a in labs)

    import PIL
    out["pil_version"] = np.array(PIL.__version__)
    out["numpy_version"] = np.array(np.__version__)
    out["torch_version"] = np.array(torch.__version__)
    tmpf = OUT + ".tmp.npz"
    np.savez_compressed(tmpf, **out)
    size = os.path.getsize(tmpf)
    if size >= MAX_BYTES:
        os.remove(tmpf)
        raise SystemExit(f"fixture would be {size} bytes (limit {MAX_BYTES})")
    os.replace(tmpf, OUT)
    print(f"wrote {OUT}: {size} bytes, {len(names)} merge cases ({adjusted} adjusted), {len(cw_cases)} class-weight cases")


if __name__ == "__main__":
    main()
