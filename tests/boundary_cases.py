"""The case table the boundary-quality tests share: the smallest image pairs at which csrc/boundary.hip can
still go wrong.  TH x TW is the kernel's tile (SEGK_BOUNDARY_TILE_H x SEGK_BOUNDARY_TILE_W of include/segk.h): shapes are named
relative to it, so a tile change moves the cases with it.  No image is larger than about 200 x 300."""
import os
import re
import sys
from dataclasses import dataclass
from typing import Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as CR                                                  # noqa: E402
import boundary_reference as R                                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def macro(name):
    txt = open(os.path.join(ROOT, "include", "segk.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\w+)", txt).group(1).rstrip("uUlL"), 0)


TH, TW = macro("SEGK_BOUNDARY_TILE_H"), macro("SEGK_BOUNDARY_TILE_W")
MAX_WIDTH = macro("SEGK_BOUNDARY_MAX_WIDTH")
SHAPES = R.SHAPES
ALL_WIDTHS = (1, 2, 7, MAX_WIDTH)


@dataclass
class Case:
    name: str
    pred: np.ndarray                         # uint8 [H,W]
    label: np.ndarray                        # uint8 or int64 [H,W]
    C: int
    ignore: Tuple[int, ...] = ()
    widths: Tuple[int, ...] = (1, 7)
    shapes: Tuple[str, ...] = SHAPES
    borders: Tuple[bool, ...] = (True, False)
    max_distance: int = MAX_WIDTH


def blob_pair(H, W, C, seed=0, shift=(2, 3), speckle=0.004, void=True):
    """a label of smooth blobs (classes folded into 0..C-1) and a prediction that is the label moved by `shift` with a few
    pixels redrawn: contours a few pixels apart, as a real prediction's; with void, a void blob beside a contour in the label
    and values >= C in the prediction"""
    rng = np.random.default_rng(1000003 * H + 7919 * W + seed)
    lab = (CR.blobs(H, W, speckle=speckle, seed=seed) % C).astype(np.uint8)
    pred = np.roll(lab, shift, axis=(0, 1))
    hit = rng.random((H, W)) < speckle
    pred[hit] = rng.integers(0, C, size=(H, W), dtype=np.uint8)[hit]
    if void:
        y, x = int(0.35 * H), int(0.5 * W)                 # on the right edge of the first blob
        lab[max(y - 3, 0):y + 4, max(x - 4, 0):x + 3] = 255
        pred[rng.random((H, W)) < 0.003] = C               # >= C: void in the prediction alone
        pred[H // 2:H // 2 + 2, W // 4:W // 4 + 9] = 200
    return np.ascontiguousarray(pred), np.ascontiguousarray(lab)


def _noise(H, W, C, seed):
    rng = np.random.default_rng(31 * H + 17 * W + seed)
    return rng.integers(0, C, size=(H, W), dtype=np.uint8), rng.integers(0, C, size=(H, W), dtype=np.uint8)


def _offset_pair(H, W, y, x, dy, dx):
    """one lone label pixel at (y, x) and one lone predicted pixel at (y + dy, x + dx), class 1 on class 0: their contour
    rings are the two pixels' 4-neighbourhoods, so the nearest-contour offsets are (dy, dx) moved by at most one"""
    lab = np.zeros((H, W), dtype=np.uint8)
    pred = np.zeros((H, W), dtype=np.uint8)
    lab[y, x] = 1
    pred[y + dy, x + dx] = 1
    return pred, lab


def _bars(H, W, at, thick=1):
    """class 1 bars whose contours lie on the given rows: with `at` on a tile edge the contour pixels sit in two tiles"""
    m = np.zeros((H, W), dtype=np.uint8)
    for y in at:
        m[y:y + thick] = 1
    return m


def cases():
    R32 = MAX_WIDTH
    out = [
        Case("one_pixel", np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8), 1, widths=(1, R32)),
        Case("one_row", *blob_pair(1, 150, 3, 1, shift=(0, 2), speckle=0.05, void=False), 3, widths=(1, 2, R32)),
        Case("one_column", *blob_pair(90, 1, 3, 2, shift=(3, 0), speckle=0.05, void=False), 3, widths=(1, 2, R32)),
        Case("smaller_than_the_band", *_noise(5, 7, 3, 3), 3, widths=(2, R32)),
        Case("one_tile", *blob_pair(TH, TW, 4, 4), 4, ignore=(3,), widths=ALL_WIDTHS),
        Case("tile_plus_row", *blob_pair(TH + 1, TW, 3, 5), 3, widths=(2, R32)),
        Case("tile_plus_column", *blob_pair(TH, TW + 1, 2, 6), 2, widths=(2, R32)),
        Case("tiles_plus_1", *blob_pair(TH + 1, 2 * TW + 1, 4, 7, shift=(3, 4)), 4, ignore=(3, 200), widths=ALL_WIDTHS),
        Case("eight_classes", *blob_pair(70, 90, 8, 8, speckle=0.02), 8, ignore=(6,), widths=(1, 7)),
        Case("one_class_of_one", *blob_pair(40, 50, 1, 9), 1, widths=(2,)),
        Case("all_void_label", blob_pair(30, 40, 3, 10)[0], np.full((30, 40), 255, np.uint8), 3, widths=(2,), shapes=("square",)),
        Case("constant", np.full((20, 30), 2, np.uint8), np.full((20, 30), 2, np.uint8), 3, widths=(3,)),
        Case("noise", *_noise(37, 45, 3, 11), 3, widths=(1, 7)),
        # contours on a tile edge, both ways: rows TH - 1 | TH and columns TW - 1 | TW
        Case("contour_on_tile_rows", _bars(TH + 20, 40, (TH - 3,), 3), _bars(TH + 20, 40, (TH,), 5), 2, widths=(1, 7, R32),
             shapes=("square", "disk")),
        Case("contour_on_tile_columns", _bars(TW + 20, 30, (TW - 2,), 2).T.copy(), _bars(TW + 20, 30, (TW,), 4).T.copy(), 2,
             widths=(1, 7, R32), shapes=("square", "diamond")),
        # nearest contour pixels at chosen offsets, the pair straddling the tile corner; (R, 1) is past the cap
        Case("offset_1_1", *_offset_pair(TH + 40, TW + 40, TH - 1, TW - 1, 1, 1), 2, widths=(1,), shapes=("square",), borders=(False,)),
        Case("offset_3_4", *_offset_pair(TH + 40, TW + 40, TH - 2, TW - 2, 3, 4), 2, widths=(1,), shapes=("square",), borders=(False,)),
        Case("offset_0_R", *_offset_pair(TH + 40, TW + 40, TH - 1, TW - 20, 0, R32), 2, widths=(1,), shapes=("square",), borders=(False,)),
        Case("offset_R_1", *_offset_pair(TH + 40, TW + 40, TH - 20, TW - 1, R32, 1), 2, widths=(1,), shapes=("square",), borders=(False,)),
        Case("offset_R_1_small_cap", *_offset_pair(30, 40, 8, 9, 5, 1), 2, widths=(1,), shapes=("square",), borders=(False,),
             max_distance=5),
        Case("small_cap", *blob_pair(50, 70, 3, 12, shift=(4, 6)), 3, widths=(2, 7), shapes=("disk",), max_distance=3),
        # an empty Kg(c) against a non-empty Kp(c): the label has no class 1 at all
        Case("empty_label_contour", _bars(30, 40, (10,), 4), np.zeros((30, 40), np.uint8), 2, widths=(2,), shapes=("square",)),
    ]
    # an int64 label with values outside 0..255, which are void
    p, lab = blob_pair(45, 60, 3, 13)
    wide = lab.astype(np.int64)
    wide[lab == 255] = -1
    wide[5:8, 5:9] = 1000
    out.append(Case("int64_label", p, wide, 3, widths=(2,), shapes=("square", "disk")))
    return out


CASES = cases()


def settings(case):
    """(width, shape, image_border) of every launch of a case"""
    return [(w, s, b) for w in case.widths for s in case.shapes for b in case.borders]
