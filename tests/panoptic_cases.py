"""The case table the object-evaluation tests share: hand-made cases whose numbers are written here, blob and
noise masks, and the sizes that cross every constant csrc/panoptic.hip declares.  A case is a dict: pred / target uint8 [H,W],
things, stuff, ignore_index, target_objects (None or (labels int32 [H,W], classes list)) and, for the hand cases, `want`: the
rows {class: (TP, FP, FN)} and further facts the host test asserts.  The restatement's results are computed once per (case,
connectivity) and shared."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as CR                                                  # noqa: E402
import panoptic_reference as PR                                                    # noqa: E402

CASES = {}


def _add(name, pred, target, things=(1,), stuff=(), ignore_index=None, target_objects=None, want=None):
    CASES[name] = dict(pred=np.ascontiguousarray(pred, dtype=np.uint8), target=np.ascontiguousarray(target, dtype=np.uint8),
                       things=tuple(things), stuff=tuple(stuff), ignore_index=ignore_index, target_objects=target_objects, want=want)


def _z(H, W):
    return np.zeros((H, W), np.uint8)


def _box(H, W, boxes):
    m = _z(H, W)
    for y0, x0, y1, x1, v in boxes:
        m[y0:y1, x0:x1] = v
    return m


def _rng(*salt):
    return np.random.default_rng([20190501, *salt])


def noise(H, W, density, classes, seed, void=0.0):
    """a pixel is one of the classes 1..classes with probability `density`, else 0; `void` of the pixels become 255"""
    r = _rng(H, W, int(density * 100), classes, seed)
    m = np.where(r.random((H, W)) < density, r.integers(1, classes + 1, size=(H, W)), 0).astype(np.uint8)
    m[r.random((H, W)) < void] = 255
    return m


# ---- the smallest shapes
_add("1x1", [[1]], [[1]], want={1: (1, 0, 0)})
_add("1x7", [[1, 1, 0, 2, 2, 2, 0]], [[1, 1, 1, 0, 2, 2, 255]], things=(1, 2), want={1: (1, 0, 0), 2: (1, 0, 0)})
_add("7x1", [[1], [0], [1], [1], [0], [2], [2]], [[1], [1], [1], [1], [0], [0], [2]], things=(1, 2), stuff=(0,),
     want={0: (0, 1, 1), 1: (0, 2, 1), 2: (0, 1, 1)})
_add("all_void", noise(9, 11, 0.5, 2, 1), np.full((9, 11), 255, np.uint8), things=(1, 2), want={})
_add("all_nothing", _z(5, 6), _z(5, 6), things=(1, 2), want={})
_same = CR.blobs(64, 64, speckle=0.01, seed=3)
_add("identical", _same, _same, things=(1, 2), stuff=(0,), ignore_index=3)

# ---- the thresholds.  A 2 x 2 target of class 1 at (2..3, 2..3) of an 8 x 8 image
_t4 = _box(8, 8, [(2, 2, 4, 4, 1)])
_add("half_inside", _box(8, 8, [(2, 2, 3, 4, 1)]), _t4, want={1: (0, 1, 1)})                 # n 2, union 4: IoU exactly 0.5
_p5 = _t4.copy(); _p5[4, 2] = 1
_add("cover5", _p5, _t4, want={1: (1, 0, 0), "col3": {1: 3435973836}, "tp_at": {1: [1, 1, 1, 1, 1, 1, 1, 0, 0, 0]}})
_v = _z(8, 8); _v[1, 1:4] = 255
_add("void3of4", _box(8, 8, [(1, 1, 2, 5, 1)]), _v, want={1: (0, 0, 0)})                   # 3 of 4 pixels on void: no FP
_v = _z(8, 8); _v[1, 1:3] = 255
_add("void2of4", _box(8, 8, [(1, 1, 2, 5, 1)]), _v, want={1: (0, 1, 0)})                   # exactly half: an FP
_add("other_class", _box(8, 8, [(2, 2, 4, 4, 2)]), _t4, things=(1, 2), want={1: (0, 0, 1), 2: (0, 1, 0)})
_s = _box(9, 12, [(0, 0, 3, 3, 2), (6, 8, 9, 12, 2), (4, 4, 6, 6, 1)])
_add("stuff_two_blobs", _s, _s, things=(1,), stuff=(2,), want={1: (1, 0, 0), 2: (1, 0, 0)})
_one = _box(12, 30, [(2, 2, 10, 27, 1)])
_five = _one.copy(); _five[:, 6::5] = 0
_add("split5", _five, _one, want={1: (0, 5, 1)})
_add("merge5", _one, _five, want={1: (0, 1, 5)})
_ig = _box(10, 10, [(1, 1, 4, 4, 1), (5, 5, 9, 9, 3)])
_add("ignore_index", _box(10, 10, [(1, 1, 4, 4, 1), (4, 5, 9, 9, 2)]), _ig, things=(1, 2), stuff=(0,), ignore_index=3,
     want={0: (1, 0, 0), 1: (1, 0, 0), 2: (0, 0, 0)})                                       # class 2: 16 of its 20 pixels on void
# two touching instances of one class given as annotation ids; the prediction finds the left one and half of the right one
_inst = np.zeros((8, 12), np.int32); _inst[2:6, 1:6] = 1; _inst[2:6, 6:11] = 2
_add("instances", _box(8, 12, [(2, 1, 6, 6, 1), (2, 7, 4, 11, 1)]), (_inst > 0).astype(np.uint8), target_objects=(_inst, [1, 1]),
     want={1: (1, 1, 1)})
_add("instances_merged", (_inst > 0).astype(np.uint8), (_inst > 0).astype(np.uint8), target_objects=(_inst, [1, 1]),
     want={1: (0, 1, 2)})

# ---- blobs shifted by (1, 2), with a void frame; sizes around the tile, LDS-table, bitmap-word and scan-chunk constants
_b = CR.blobs(128, 160, speckle=0.02, seed=5)
_bt = CR.blobs(128, 160, speckle=0.0, seed=5); _bt[:2] = 255
_add("blobs_shift_128x160", np.roll(_b, (1, 2), (0, 1)), _bt, things=(1, 2), stuff=(0,), ignore_index=3)
for _H, _W in ((33, 65), (65, 33), (64, 129), (32, 64), (1, 2049)):
    _add(f"noise0.5_3c_{_H}x{_W}", noise(_H, _W, 0.5, 3, 1), noise(_H, _W, 0.5, 3, 2, void=0.02), things=(1, 2, 3), stuff=(0,))
for _d in (0.1, 0.5, 0.9):
    _add(f"noise{_d}_1c_120x77", noise(120, 77, _d, 1, 1), noise(120, 77, _d, 1, 2, void=0.01), things=(1,))
    _add(f"noise{_d}_3c_200x300", noise(200, 300, _d, 3, 1), noise(200, 300, _d, 3, 2, void=0.01), things=(1, 2), stuff=(3,))

NAMES = list(CASES)
HAND = [n for n in NAMES if CASES[n]["want"] is not None]


@functools.lru_cache(maxsize=None)
def labelled(name, connectivity):
    c = CASES[name]
    return PR.label_sides(c["pred"], c["target"], c["things"], connectivity, c["target_objects"])


@functools.lru_cache(maxsize=None)
def true_counts(name, connectivity):
    """(components of the larger side, at least 1; pairs)"""
    c = CASES[name]
    lab = labelled(name, connectivity)
    res = PR.evaluate(c["pred"], c["target"], lab, c["stuff"], c["ignore_index"], cap=max(len(lab[1]), len(lab[3]), 1))
    return max(len(lab[1]), len(lab[3]), 1), res["P"]


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, cap, max_pairs):
    c = CASES[name]
    return PR.evaluate(c["pred"], c["target"], labelled(name, connectivity), c["stuff"], c["ignore_index"], cap, max_pairs)


def regimes(name, connectivity):
    """{regime: (max_components, max_pairs)}: roomy; exactly the true counts; one too few of each where that is still >= 1"""
    K, P = true_counts(name, connectivity)
    out = {"roomy": (K + 13, P + 29), "exact": (K, P)}
    if P > 1:
        out["pairs-1"] = (K, P - 1)
    lab = labelled(name, connectivity)
    if max(len(lab[1]), len(lab[3])) > 1:
        out["components-1"] = (K - 1, P + 29)
    return out
