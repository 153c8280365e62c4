"""The case table the morphology tests share: the smallest maps at which csrc/morph.hip can still go wrong.
TH x TW is the kernel's tile (SEGK_MORPH_TILE_H x SEGK_MORPH_TILE_W of include/segk.h): shapes are named relative to it, so
a tile change moves the cases with it."""
import os
import re
import sys
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as CR                                                  # noqa: E402
import morph_reference as R                                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def macro(name):
    txt = open(os.path.join(ROOT, "include", "segk.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\w+)", txt).group(1).rstrip("uUlL"), 0)


TH, TW = macro("SEGK_MORPH_TILE_H"), macro("SEGK_MORPH_TILE_W")
MAX_RADIUS = macro("SEGK_MORPH_MAX_RADIUS")
SHAPES = R.SHAPES


@dataclass
class Case:
    name: str
    mask: np.ndarray
    radii: Tuple[int, ...]
    classes: Tuple[int, ...] = (1,)          # the set of erode / dilate / open / close / boundary_distance(classes=)
    fill: int = 0
    value: Optional[int] = None              # dilate / close: None = the single class
    skip: Tuple[int, ...] = ()               # label_band / boundary_distance
    band_value: int = 255
    band_classes: Optional[Tuple[int, ...]] = None
    into: Optional[Tuple[int, ...]] = None
    extra: dict = field(default_factory=dict)


def noise(H, W, values=(0, 1, 2, 3), seed=0, blob=True):
    """seeded noise over `values`, with the smooth blobs of the component tests underneath on larger maps"""
    rng = np.random.default_rng(7919 * H + 104729 * W + seed)
    m = np.asarray(values, dtype=np.uint8)[rng.integers(0, len(values), size=(H, W))]
    if blob and H >= 16 and W >= 16:
        b = CR.blobs(H, W, speckle=0.03, seed=seed)
        keep = rng.random((H, W)) < 0.9
        m = np.where(keep, np.asarray(values, dtype=np.uint8)[b % len(values)], m)
    return np.ascontiguousarray(m, dtype=np.uint8)


def _lone(H, W, at, v=1):
    m = np.zeros((H, W), dtype=np.uint8)
    for y, x in at:
        m[y, x] = v
    return m


def _corners(H=40, W=50):
    m = np.zeros((H, W), dtype=np.uint8)
    m[:6, :7] = 1; m[:5, -6:] = 1; m[-7:, :5] = 1; m[-6:, -8:] = 1           # an object in every corner
    m[:4, 20:30] = 2; m[-3:, 18:27] = 2; m[15:25, :4] = 2; m[14:22, -5:] = 2  # and against every border
    m[17:23, 22:28] = 1                                                    # one that touches nothing
    return m


def _checker(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) & 1).astype(np.uint8)


def _with_255(H=30, W=40):
    m = noise(H, W, values=(0, 1, 255, 7), seed=5, blob=False)
    m[10:20, 12:30] = 255
    m[13:17, 5:35] = 7                                                     # a band of the skipped value through it
    m[2:6, 2:9] = 7
    return m


def cases():
    multi = dict(classes=(1, 2), fill=0, value=1)
    return [
        Case("one_pixel", np.ones((1, 1), dtype=np.uint8), (1, MAX_RADIUS)),
        Case("one_row", noise(1, 37, (0, 1, 2), 1), (1, 5), **multi),
        Case("one_column", noise(41, 1, (0, 1, 2), 2), (1, 5), **multi),
        Case("smaller_than_r", noise(5, 7, (0, 1, 2), 3), (2, MAX_RADIUS), **multi),
        Case("tile_plus_1", noise(TH + 1, TW + 1, (0, 1, 2, 3), 4), (1, 2, 5, MAX_RADIUS), **multi),
        Case("two_tiles_plus", noise(2 * TH + 3, 2 * TW + 5, (0, 1, 2), 5), (1, 2, 5, MAX_RADIUS), classes=(1, 2), fill=3, value=2,
             skip=(2,), band_value=9),
        Case("lone_pixel", _lone(20, 30, [(9, 14)]), (1, 5)),
        Case("constant", np.full((9, 11), 2, dtype=np.uint8), (3,), classes=(2,), fill=0),
        Case("checkerboard", _checker(17, 19), (1, 2)),
        Case("corners_and_borders", _corners(), (1, 3, 5), **multi),
        # a pixel whose only different neighbour lies in the next tile, across an edge and across the corner, at the radius
        # (r = 5: the offsets (0,5), (3,4) fire, (4,4) does not under the disk) and one past it (r = 4)
        Case("across_tile_corner", _lone(TH + 12, TW + 12, [(TH, TW)]), (4, 5)),
        Case("across_tile_edges", _lone(TH + 12, TW + 12, [(TH - 1, 20), (30, TW), (TH, TW - 40), (8, TW - 1)]), (4, 5)),
        Case("value_255_and_skip", _with_255(), (1, 3), classes=(255, 1), fill=0, value=255, skip=(7,), band_value=200,
             band_classes=(0, 255), into=(0,)),
    ]


CASES = cases()


def operations(case, shape, r):
    """(name, function name, keywords) of every operation of a case at one shape and radius"""
    c = case
    ops = [("erode", "erode", dict(classes=c.classes, radius=r, fill=c.fill, shape=shape)),
           ("dilate", "dilate", dict(classes=c.classes, radius=r, value=c.value, into=c.into, shape=shape)),
           ("open", "open_mask", dict(classes=c.classes, radius=r, fill=c.fill, shape=shape)),
           ("close", "close_mask", dict(classes=c.classes, radius=r, value=c.value, shape=shape)),
           ("band", "label_band", dict(width=r, value=c.band_value, classes=c.band_classes, skip=c.skip, shape=shape)),
           ("distance_values", "boundary_distance", dict(max_radius=r, skip=c.skip, shape=shape)),
           ("distance_set", "boundary_distance", dict(max_radius=r, classes=c.classes, skip=c.skip, shape=shape))]
    return ops


# ------------------------------------------------------------------------------------------------ holes
@dataclass
class HoleCase:
    name: str
    mask: np.ndarray
    keywords: dict


def _ring(m, y0, x0, y1, x1, v=1):
    m[y0:y1, x0:x1] = v
    m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = 0


def hole_cases():
    out = []
    m = np.zeros((24, 40), dtype=np.uint8)
    _ring(m, 2, 2, 9, 10)                                  # a plain hole of 5 x 6 = 30
    _ring(m, 0, 14, 7, 22)                                 # the ring touches the border, its hole does not: filled
    m[10:17, 0:7] = 1; m[11:16, 0:6] = 0                   # a "hole" open to the left border: not filled
    _ring(m, 10, 12, 22, 30); _ring(m, 13, 15, 19, 25)     # nested: the outer hole holds a ring with its own hole
    m[4:6, 4:6] = 2                                        # a hole holding two classes (0 and 2 are both outside the set)
    m[20, 34] = 1; m[21, 33] = 1; m[21, 35] = 1; m[22, 34] = 1     # a diamond: closed at 4, open at 8
    out.append(HoleCase("mixed4", m, dict(classes=(1,), connectivity=4)))
    out.append(HoleCase("mixed8", m, dict(classes=(1,), connectivity=8)))
    out.append(HoleCase("area_at", m, dict(classes=(1,), max_area=30)))            # the plain hole has 30 pixels: filled
    out.append(HoleCase("area_below", m, dict(classes=(1,), max_area=29)))         # not filled
    out.append(HoleCase("value_and_set", m, dict(classes=(1, 2), value=7)))
    g = np.ones((3 * 12 + 1, 3 * 14 + 1), dtype=np.uint8)  # more holes than rows: 12 x 14 one-pixel holes
    g[1::3, 1::3] = 0
    g[0, 5] = 0                                            # and a border component among them
    out.append(HoleCase("overflow", g, dict(classes=(1,), max_components=50)))
    out.append(HoleCase("no_overflow", g, dict(classes=(1,), max_components=169)))
    big = noise(TH + 9, TW + 7, (0, 1), 11)
    out.append(HoleCase("noise", big, dict(classes=(1,), connectivity=4, max_components=4096)))
    return out


HOLE_CASES = hole_cases()
