"""The shapes, plans and inputs the tiled-prediction tests share (tests/test_tiles_host.py, tests/test_gpu_tiles.py;
DESIGN.md 3.5).  Host-only.

The set holds both axes short (L < T), L = T, L = T + 1, the nine-cover case (65 x 65 at T = 32, overlap 16), odd widths (a
thread's four flat pixels straddle a row end) and, with the last plan, a tile side that is no multiple of 4 (the gather's
scalar stores and the partial last quad of a slot row)."""
import itertools

import numpy as np

import tiles_reference as R
from oracle.fill import fill

SHAPES = [(40, 56), (33, 70), (20, 90), (65, 65), (97, 50), (3, 1), (16, 16), (17, 31)]
PLANS = [(32, 8), (32, 16), (16, 0), (48, 24), (20, 5), (18, 4)]        # (T, overlap)
CLASSES = (1, 2, 3, 4, 5, 8)
WINDOWS = ("triangle", "flat")


def plans():
    """every shape under every plan: [(index, (H, W), T, overlap)]"""
    return [(i, shape, T, o) for i, (shape, (T, o)) in enumerate(itertools.product(SHAPES, PLANS))]


def tile_count(shape, T, o):
    return len(R.tile_axis(shape[0], T, o)) * len(R.tile_axis(shape[1], T, o))


def softmax_cases():
    """the cases of the float64 comparison: every shape under every plan, class counts and windows cycling over them"""
    return [dict(shape=shape, T=T, o=o, C=(2, 3, 4, 5, 8)[i % 5], window=WINDOWS[(i // 5) % 2], seed=1700 + i)
            for i, shape, T, o in plans()]


def logits(case):
    """Y [n, C, T, T] float32 in (-3, 3)"""
    n = tile_count(case["shape"], case["T"], case["o"])
    return fill((n, case["C"], case["T"], case["T"]), case["seed"], -3, 3).numpy()


def probabilities(case):
    """Y of a model that returns probabilities: the float64 softmax of such a field, rounded to float32"""
    y = logits(case).astype(np.float64)
    e = np.exp(y - y.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def poison(Y, case):
    """NaN at every position of Y that no pixel maps to"""
    Y = Y.copy()
    un = R.unmapped(*case["shape"], case["T"], case["o"])
    Y[np.broadcast_to(un[:, None], Y.shape)] = np.nan
    return Y
