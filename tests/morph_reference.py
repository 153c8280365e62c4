"""NumPy restatement of DESIGN.md 3.21 (mask morphology), written from the definition: D(p) is found by brute force over
every offset of the structuring element with shifted comparisons -- no column / row passes, so it shares no mistake with
csrc/morph.hip.  Hole filling uses the labelling of components_reference.py.  The device must equal every array here bit for
bit.  `two_pass` restates the kernel's decomposition instead and exists to be compared with the brute force."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as CR                                                  # noqa: E402

WILD = 0xFFFF
FAR = 0xFFFF
MAX_RADIUS = 32
SHAPES = ("square", "diamond", "disk")


def metric(shape, dx, dy):
    dx, dy = abs(dx), abs(dy)
    return {"square": max(dx, dy), "diamond": dx + dy, "disk": dx * dx + dy * dy}[shape]


def cap_of(shape, r):
    return r * r if shape == "disk" else r


def byte_set(classes):
    """-> bool [256]"""
    t = np.zeros(256, dtype=bool)
    t[[int(c) for c in classes]] = True
    return t


def set_keys(classes):
    return byte_set(classes).astype(np.int64)


def value_keys(skip=()):
    k = np.arange(256, dtype=np.int64)
    k[[int(c) for c in skip]] = WILD
    return k


_memo = {}


def distance(m, key, shape, r):
    """D(p) int64 [H,W] (squared for the disk), FAR where nothing differs within the radius.  Results are kept: the
    operations of one map share them."""
    m = np.asarray(m)
    assert m.dtype == np.uint8 and m.ndim == 2 and 1 <= r <= MAX_RADIUS and shape in SHAPES
    key = np.asarray(key, dtype=np.int64)
    memo = (m.shape, m.tobytes(), key.tobytes(), shape, r)
    if memo not in _memo:
        if len(_memo) > 512:
            _memo.clear()
        _memo[memo] = _distance(m, key, shape, r)
    return _memo[memo]


def _distance(m, key, shape, r):
    H, W = m.shape
    K = key[m].astype(np.int32)
    P = np.full((H + 2 * r, W + 2 * r), WILD, dtype=np.int32)      # outside the image: the wild key
    P[r:r + H, r:r + W] = K
    live_p = K != WILD
    D = np.full((H, W), FAR, dtype=np.int64)
    cap = cap_of(shape, r)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            d = metric(shape, dx, dy)
            if d > cap or (dy == 0 and dx == 0):
                continue
            Q = P[r + dy:r + dy + H, r + dx:r + dx + W]
            differs = (Q != K) & (Q != WILD) & live_p
            D[differs & (D > d)] = d
    D.setflags(write=False)
    return D


def fires(m, key, shape, r):
    return distance(m, key, shape, r) <= cap_of(shape, r)


def _single(classes, value, what):
    cs = sorted({int(c) for c in classes})
    if value is None:
        assert len(cs) == 1, f"{what}: value is required with several classes"
        return cs[0]
    return int(value)


def erode(m, classes, radius, fill, shape="disk"):
    S = byte_set(classes)
    assert not S[int(fill)]
    out = m.copy()
    out[S[m] & fires(m, S.astype(np.int64), shape, radius)] = fill
    return out


def dilate(m, classes, radius, value=None, into=None, shape="disk"):
    S = byte_set(classes)
    value = _single(classes, value, "dilate")
    T = ~S if into is None else byte_set(into)
    assert not (T & S).any()
    out = m.copy()
    out[T[m] & fires(m, S.astype(np.int64), shape, radius)] = value
    return out


def open_mask(m, classes, radius, fill, shape="disk"):
    S = byte_set(classes)
    e = erode(m, classes, radius, fill, shape)
    back = S[m] & ~S[e] & fires(e, S.astype(np.int64), shape, radius)      # of the original set, gone, and near what is left
    out = e.copy()
    out[back] = m[back]
    return out


def close_mask(m, classes, radius, value=None, shape="disk"):
    S = byte_set(classes)
    value = _single(classes, value, "close_mask")
    assert S[value]
    d = dilate(m, classes, radius, value, None, shape)
    back = ~S[m] & S[d] & fires(d, S.astype(np.int64), shape, radius)      # painted, and near what stayed outside
    out = d.copy()
    out[back] = m[back]
    return out


def label_band(m, width, value=255, classes=None, skip=(), shape="disk"):
    key = value_keys(skip)
    C = np.ones(256, dtype=bool) if classes is None else byte_set(classes)
    out = m.copy()
    out[C[m] & fires(m, key, shape, width)] = value
    return out


def boundary_distance(m, max_radius, classes=None, skip=(), shape="disk"):
    key = value_keys(skip) if classes is None else set_keys(classes)
    if classes is not None:
        key[[int(c) for c in skip]] = WILD
    return distance(m, key, shape, max_radius).astype(np.uint16)


def fill_holes(m, classes, value=None, connectivity=4, max_area=None, max_components=65536):
    """-> (mask, num, filled): a hole is a component of the complement of the set whose box touches no image border and
    whose area is <= max_area; only the first max_components components (raster order of the first pixel) can be filled"""
    S = byte_set(classes)
    value = _single(classes, value, "fill_holes")
    H, W = m.shape
    comp = np.where(S[m], 255, 0).astype(np.uint8)
    labels, rows = CR.label(comp, connectivity, classes=(0,))
    out = m.copy()
    filled = 0
    for k, row in enumerate(rows[:max_components], 1):
        y0, x0, y1, x1 = row["box"]
        if y0 > 0 and x0 > 0 and y1 < H and x1 < W and (max_area is None or row["area"] <= max_area):
            out[labels == k] = value
            filled += 1
    return out, len(rows), filled


def two_pass(m, key, shape, r):
    """The kernel's decomposition (DESIGN.md 3.21 "two passes"), on the whole image: g = the vertical distance to the nearest
    live key that differs from the cell's own (a wild cell: to the nearest live key), saturating at r + 1; then per pixel
    the minimum over dx of dist(dx, 0) where the key at x + dx differs, else dist(dx, g(x + dx)), a wild cell's column
    being walked from g to r."""
    m = np.asarray(m)
    H, W = m.shape
    K = np.asarray(key, dtype=np.int64)[m]
    sat = r + 1
    g = np.full((H, W), sat, dtype=np.int64)
    for x in range(W):
        for sweep in (range(H), range(H - 1, -1, -1)):
            a, da, db = WILD, sat, sat
            for y in sweep:
                k = K[y, x]
                v = da
                if k != WILD:
                    if a != k:
                        db, a = da, k
                    else:
                        v = db
                    da = 0
                g[y, x] = min(g[y, x], v)
                da, db = min(da + 1, sat), min(db + 1, sat)
    D = np.full((H, W), FAR, dtype=np.int64)
    cap = cap_of(shape, r)
    for y in range(H):
        for x in range(W):
            kp = K[y, x]
            if kp == WILD:
                continue
            best = FAR
            for dx in range(-r, r + 1):
                if not 0 <= x + dx < W:
                    continue
                kq, v = K[y, x + dx], g[y, x + dx]
                if kq == WILD:
                    dy = v
                    while dy <= r:
                        u = K[y - dy, x + dx] if y - dy >= 0 else WILD
                        d = K[y + dy, x + dx] if y + dy < H else WILD
                        if (u != WILD and u != kp) or (d != WILD and d != kp):
                            break
                        dy += 1
                    v = dy
                elif kq != kp:
                    v = 0
                best = min(best, metric(shape, dx, v))
            if best <= cap:
                D[y, x] = best
    return D
