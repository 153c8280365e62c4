"""The case table tests/test_raster_host.py and tests/test_gpu_raster.py share.  Host-only.

A case is (images, fill): images a list of (shapes, (H, W)), one launch; a shape is the dict of tests/raster_reference.py.
The shapes are the smallest at which each mechanism can go wrong: the tile is 64 rows x 256 columns (SEGK_RAST_TILE_H / _W),
the bit plane has 8 words of 32 columns per tile row, the RLE search halves log2(runs) + 1 times."""
import functools

import numpy as np

import raster_reference as rref

TH, TW = 64, 256


def poly(rings, value=1):
    return {"rings": [np.asarray(r) for r in rings], "value": value}


def rle(H, W, counts, value=1):
    return {"rle": {"size": [H, W], "counts": counts}, "value": value}


def one(shapes, H, W, fill=0):
    return [(shapes, (H, W))], fill


def _spanning(H, W):
    """a quadrilateral off the 1/256 grid that reaches into every tile of an H x W image (where the image has an inside)"""
    return [(0.3, 0.2), (W - 0.3, H * 0.1), (W - 0.6, H - 0.2), (W * 0.1, H - 0.4)]


def _in_last_tile(H, W):
    """a triangle inside the last tile alone"""
    y0, x0 = (H - 1) // TH * TH, (W - 1) // TW * TW
    h, w = H - y0, W - x0
    return [(x0 + 0.2 * w, y0 + 0.1 * h), (x0 + 0.9 * w, y0 + 0.5 * h), (x0 + 0.3 * w, y0 + 0.95 * h)]


def _random_polygon(rng, H, W, on_grid):
    n = int(rng.integers(3, 41))
    v = rng.uniform(-0.2, 1.2, (n, 2)) * (W, H)
    if on_grid:
        return np.floor(v * 256) / 256               # exact multiples of 1/256: quantisation changes nothing
    return v + 1.0 / 1024                            # a quarter of a step off the grid


def _rle_runs(H, W, n, zero_first=False, seed=0):
    """n counts that sum to H*W, all > 0 but (zero_first) the first"""
    hw = H * W
    m = n - 1 if zero_first else n
    assert 1 <= m <= hw
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, hw), m - 1, replace=False)) if m > 1 else np.zeros(0, np.int64)
    counts = np.diff(np.concatenate([[0], cuts, [hw]])).tolist()
    return ([0] if zero_first else []) + [int(c) for c in counts]


def _cases():
    c = {}
    sq = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    # ---- basic
    c["unit_1x1"] = one([poly([sq(0, 0, 1, 1)])], 1, 1)
    c["no_shapes"] = one([], 5, 7, fill=3)
    c["value_is_fill"] = one([poly([sq(1, 1, 5, 5)], 2), poly([sq(3, 0, 6, 4)], 0)], 6, 6)
    # ---- out of bounds
    c["outside_left"] = one([poly([sq(-9, 2, -1, 8)])], 10, 12)
    c["outside_right"] = one([poly([sq(12, 2, 30, 8)])], 10, 12)
    c["outside_top"] = one([poly([sq(2, -7, 9, 0)])], 10, 12)
    c["outside_bottom"] = one([poly([sq(2, 10, 9, 19.5)])], 10, 12)
    c["overhang"] = one([poly([[(-5, -5), (20, -3), (18.5, 15), (-4, 14.25)]], 4)], 10, 12)
    # ---- the centre rule and the half-open row rule
    c["centre_triangle"] = one([poly([[(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)]])], 6, 6)
    c["scanline_rect"] = one([poly([sq(1.5, 1.5, 4.5, 3.5)])], 6, 6)
    # ---- topology
    c["bowtie"] = one([poly([[(1, 1), (11, 9), (11, 1), (1, 9)]], 5)], 10, 12)
    star = [(10 + 9 * np.sin(2 * np.pi * k * 2 / 5), 10 - 9 * np.cos(2 * np.pi * k * 2 / 5)) for k in range(5)]
    c["pentagram"] = one([poly([star], 6)], 20, 20)
    c["collinear"] = one([poly([[(1, 1), (6, 6), (3, 3)]]), poly([[(2, 7.5), (9, 7.5), (5, 7.5)]], 2)], 10, 12)
    c["sliver"] = one([poly([sq(5.4, -1, 5.6, 200)], 1), poly([sq(8.6, -1, 8.9, 200)], 2),
                       poly([[(11.6, 0), (11.9, 0), (15.9, 192), (15.6, 192)]], 3)], 192, 20)
    # ---- paint order, even-odd against union
    a, b = sq(1, 1, 8, 7), sq(5, 3, 11, 9)
    c["order_ab"] = one([poly([a], 1), poly([b], 2)], 10, 12)
    c["order_ba"] = one([poly([b], 2), poly([a], 1)], 10, 12)
    c["two_rings_one_shape"] = one([poly([a, b], 1)], 10, 12)
    c["two_rings_two_shapes"] = one([poly([a], 1), poly([b], 1)], 10, 12)
    # ---- tile borders
    for H, W in ((64, 256), (63, 255), (65, 257), (129, 513), (1, 300), (300, 1)):
        c[f"tiles_{H}x{W}"] = one([poly([_spanning(H, W)], 1), poly([_in_last_tile(H, W)], 2)], H, W, fill=7)
    # ---- arithmetic range: the longest edge an image admits, in both directions
    c["diag_8x8192"] = one([poly([[(0, 0), (8192, 8), (0, 8)]], 3)], 8, 8192)
    c["diag_8192x8"] = one([poly([[(0, 0), (8, 8192), (8, 0)]], 3)], 8192, 8)
    # ---- many shapes per tile
    rng = np.random.default_rng(1808)
    c["triangles200"] = one([poly([rng.uniform(-10, 140, (3, 2)) * (1, 80 / 150)], k % 8) for k in range(200)], 70, 130, fill=9)
    # ---- random float polygons, on the 1/256 grid and off it
    for on_grid in (True, False):
        rng = np.random.default_rng(77 + on_grid)
        H, W = (37, 53) if on_grid else (100, 300)
        c[f"random_{'grid' if on_grid else 'offgrid'}"] = one(
            [poly([_random_polygon(rng, H, W, on_grid)], 1 + k % 5) for k in range(6)], H, W)
    # ---- a ragged batch, the middle image empty
    c["batch"] = ([([poly([_spanning(70, 300)], 1), rle(70, 300, _rle_runs(70, 300, 40, seed=3), 2)], (70, 300)),
                   ([], (9, 5)),
                   ([poly([star], 3), poly([sq(-2, 5, 30, 8.5)], 4)], (20, 20))], 8)
    # ---- run-length codes
    c["rle_starts_with_0"] = one([rle(7, 9, [0, 5, 10, 48])], 7, 9)
    c["rle_all_background"] = one([rle(7, 9, [63], 2)], 7, 9, fill=1)                 # ONE run
    c["rle_all_foreground"] = one([rle(7, 9, [0, 63], 2)], 7, 9, fill=1)
    c["rle_two_runs"] = one([rle(7, 9, [20, 43], 2)], 7, 9)
    c["rle_h1"] = one([rle(1, 300, [3, 250, 40, 7], 5)], 1, 300)
    c["rle_across_columns"] = one([rle(5, 4, [3, 9, 2, 6])], 5, 4)                     # both foreground runs cross column ends
    c["rle_zero_counts"] = one([rle(5, 4, [3, 0, 2, 4, 0, 0, 0, 6, 5])], 5, 4)
    c["rle_1025_runs"] = one([rle(66, 260, _rle_runs(66, 260, 1025, seed=5), 3)], 66, 260)
    c["rle_1025_runs_zero_first"] = one([rle(40, 60, _rle_runs(40, 60, 1025, zero_first=True, seed=6), 3)], 40, 60)
    c["mixed"] = one([poly([_spanning(70, 300)], 1), rle(70, 300, _rle_runs(70, 300, 30, seed=8), 2),
                      poly([sq(100.5, 10, 290, 66)], 3), rle(70, 300, _rle_runs(70, 300, 7, zero_first=True, seed=9), 4),
                      poly([_in_last_tile(70, 300)], 0)], 70, 300, fill=5)
    return c


CASES = _cases()
NAMES = list(CASES)
RLE_NAMES = [n for n in NAMES if any("rle" in s for shapes, _ in CASES[n][0] for s in shapes)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the label maps of a case by the restatement: computed once, shared, never modified"""
    images, fill = CASES[name]
    out = []
    for shapes, (H, W) in images:
        lab = rref.render(shapes, H, W, fill)
        lab.setflags(write=False)
        out.append(lab)
    return out
