#!/usr/bin/env python3
"""Generate tests/golden/prompt_points.npz by running THE REFERENCE'S OWN two functions of the "Prompt Augmentation" cell
of utils/augmentation.ipynb: the notebook is read as JSON, the cell that defines create_gaussian_heatmap and
select_dominant_class is parsed with `ast`, and only those two FunctionDefs are compiled into a namespace that holds `np`,
`random` and a silent `print`.  Nothing of the notebook's text is written anywhere; the fixture holds numbers only.

The loop around the two functions is script code of the cell, so it is restated in run_case() below: remap the labels
(255 -> 3, the reference's target_remap; then 3 -> 0 and + 1), skip a map with fewer than two target classes, draw a centre,
score it, take its class if it is non-zero and new, stop at two; heat-maps are stored as the cell writes them,
(heatmap * 255).astype(uint8).  The fixture records the first 64 draws of each case (the loop's decisions for draws behind
the second taken one are never made by the reference; the recorded scores and classes of those draws still are its own).

The generator asserts the fixture's fitness and refuses to write a file that fails it: every candidate's class choice must
be STABLE under the score bound of tests/test_gpu_prompt_points.py (largest sum clear of the 1e-9 threshold and of the
second largest sum), the 8-bit heat value must be a function of the squared distance alone, class 0 must be chosen somewhere
in the class-0 case, and the file must stay below 744 KB.

Usage: python tools/gen_golden_prompts.py --reference DIR      (or SEG_REFERENCE=DIR; CPU only)"""
import argparse
import ast
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.fill import labels as fill_labels        # noqa: E402

SIGMA = 3.0
DRAWS = 64
QLEN = 512               # squared distances recorded in q_by_d2 (-1: never seen)
OUT = os.path.join(ROOT, "tests", "golden", "prompt_points.npz")
MAX_BYTES = 744 * 1024
NCLS = 8


def reference_functions(ref):
    nb = json.load(open(os.path.join(ref, "utils", "augmentation.ipynb")))
    want = ("create_gaussian_heatmap", "select_dominant_class")
    for cell in nb["cells"]:
        src = "".join(cell["source"])
        if cell["cell_type"] != "code" or not all("def " + w in src for w in want):
            continue
        defs = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in want]
        ns = {"np": np, "random": random, "print": lambda *a, **k: None}
        exec(compile(ast.Module(body=defs, type_ignores=[]), "<reference cell>", "exec"), ns)
        return ns[want[0]], ns[want[1]]
    raise SystemExit("the Prompt Augmentation cell was not found")


def blocky(shape, seed, ncls, scale, crop=None):
    m = np.kron(fill_labels(shape, seed, ncls).numpy(), np.ones((scale, scale), dtype=np.int64))
    return m if crop is None else m[:crop[0], :crop[1]]


def cases():
    """name -> (label map as stored, raw trimap?)"""
    out = {}
    out["sq256"] = (blocky((8, 8), 101, 3, 32) + 1, False)                      # remapped classes 1..3
    out["odd33x47"] = (blocky((5, 6), 102, 3, 8, (33, 47)) + 1, False)          # non-square, H*W odd
    out["rect128x96"] = (blocky((8, 6), 103, 3, 16) + 1, False)
    out["single64"] = (np.full((64, 64), 2, dtype=np.int64), False)             # one class: the reference skips it
    m = blocky((8, 8), 104, 2, 16) + 1                                          # un-remapped: a 64 x 64 corner of class 0
    m[:64, :64] = 0
    out["zero128"] = (m, False)
    t = blocky((6, 8), 105, 4, 16)                                              # raw trimap 0 / 1 / 2 / 255
    t[t == 3] = 255
    out["trimap96x128"] = (t, True)
    return out


def run_case(idx, lab, raw, heat_fn, select_fn):
    if raw:                                            # the cell's two remaps
        m = lab.astype(np.uint8).copy()
        m[m == 255] = 3
        sw = m.copy()
        sw[m == 3] = 0
        remapped = sw + 1
    else:
        remapped = lab.astype(np.uint8)
    present = np.unique(remapped)
    skip_early = len(present[present > 0]) < 2
    random.seed(idx)
    centers = np.zeros((DRAWS, 2), np.int32)
    scores = np.zeros((DRAWS, NCLS), np.float64)
    cls = np.zeros(DRAWS, np.int32)
    heats = []
    for k in range(DRAWS):
        h, (cy, cx) = heat_fn(size=remapped.shape, sigma=SIGMA)
        c, sc = select_fn(h, remapped)
        centers[k] = (cy, cx)
        cls[k] = c
        for cv, s in sc.items():
            assert 1 <= int(cv) < NCLS
            scores[k, int(cv)] = s
        heats.append(h)
    taken, found = [], set()
    if not skip_early:
        for k in range(DRAWS):                         # the cell's while loop over the same draws
            if len(taken) == 2:
                break
            if cls[k] > 0 and int(cls[k]) not in found:
                taken.append(k)
                found.add(int(cls[k]))
    ok = len(taken) == 2
    H, W = remapped.shape
    heat8 = np.zeros((2, H, W), np.uint8)
    masks = np.zeros((2, H, W), np.uint8)
    if ok:
        for j, k in enumerate(taken):
            heat8[j] = (heats[k] * 255).astype(np.uint8)
            masks[j][remapped == cls[k]] = cls[k]
    return dict(labels=lab.astype(np.int16), remapped=remapped, centers=centers, scores=scores, cls=cls,
                taken=np.array(taken if ok else [-1, -1], np.int32), heat8=heat8, masks=masks, skipped=np.array(not ok))


def stable(scores):
    """per candidate: is the reference's class choice safe under |dev - ref| <= 2e-12 + 2e-12 ref on every sum?"""
    s = np.sort(scores[:, 1:], axis=1)
    top, second = s[:, -1], s[:, -2]
    return (top < 1e-9 - 4e-12) | ((top > 1e-9 + 4e-12) & (top - second > 4e-12 + 4e-12 * top))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("SEG_REFERENCE"), help="checkout of the reference project")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or SEG_REFERENCE) is required")
    heat_fn, select_fn = reference_functions(args.reference)
    out = {}
    q_by_d2 = np.full(QLEN, -1, np.int16)
    names = []
    total = unstable = zero_chosen = 0
    for idx, (name, (lab, raw)) in enumerate(cases().items()):
        r = run_case(idx, lab, raw, heat_fn, select_fn)
        names.append(name)
        for k, v in r.items():
            out[f"{name}.{k}"] = v
        st = stable(r["scores"])
        total += len(st)
        unstable += int((~st).sum())
        if name == "zero128":
            zero_chosen = int((r["cls"] == 0).sum())
        if not r["skipped"]:
            H, W = r["remapped"].shape
            yy, xx = np.indices((H, W))
            for j, k in enumerate(r["taken"]):
                cy, cx = r["centers"][k]
                d2 = (yy - cy) ** 2 + (xx - cx) ** 2
                assert (r["heat8"][j][d2 >= QLEN] == 0).all(), "a heat value beyond the recorded distances"
                for d, v in zip(d2[d2 < QLEN].ravel(), r["heat8"][j][d2 < QLEN].ravel()):
                    assert q_by_d2[d] in (-1, v), f"heat value at d2={d} is not a function of the distance"
                    q_by_d2[d] = v
        print(f"{name:14s} {r['remapped'].shape} classes chosen {np.bincount(r['cls'], minlength=4).tolist()} taken "
              f"{r['taken'].tolist()} skipped {bool(r['skipped'])} unstable {int((~st).sum())}")
    # fitness
    assert unstable == 0, f"{unstable} of {total} candidates have an unstable class choice: pick other maps"
    assert zero_chosen > 0, "class 0 is never chosen in the class-0 case"
    assert bool(out["single64.skipped"]) and sum(bool(out[f"{n}.skipped"]) for n in names) == 1
    seen = q_by_d2[q_by_d2 >= 0]
    assert (q_by_d2[:100][q_by_d2[:100] >= 0] > 0).all() and (q_by_d2[100:] <= 0).all() and len(seen) > 100
    out["q_by_d2"] = q_by_d2
    out["names"] = np.array(names)
    out["sigma"] = np.array(SIGMA)
    out["numpy_version"] = np.array(np.__version__)
    try:
        import torch
        out["torch_version"] = np.array(torch.__version__)
    except ImportError:
        out["torch_version"] = np.array("none")
    out["seed_rule"] = np.array("random.seed(case index)")
    tmp = OUT + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    size = os.path.getsize(tmp)
    if size >= MAX_BYTES:
        os.remove(tmp)
        raise SystemExit(f"fixture would be {size} bytes (limit {MAX_BYTES})")
    os.replace(tmp, OUT)
    print(f"wrote {OUT}: {size} bytes, {total} candidates, 0 unstable, class 0 chosen {zero_chosen} times")


if __name__ == "__main__":
    main()
