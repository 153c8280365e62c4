"""NumPy / pure-Python restatement of DESIGN.md 3.3 (mask clean-up): breadth-first labelling in raster order, the
statistics, the removal flags, the one-pass neighbour vote and the cleaned mask.  The device (csrc/components.hip) must
equal every array here bit for bit.  Also the synthetic masks the component tests share."""
from collections import deque

import numpy as np

MAX_CLASSES = 8
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def class_set(classes):
    """classes=None: every class; else the classes of an iterable (each in 0..7)"""
    if classes is None:
        return set(range(MAX_CLASSES))
    return {int(c) for c in classes}


def keep_set(keep_largest, classes):
    """False: none; True: every labelled class; else the classes of an iterable -- always inside the labelled classes"""
    if keep_largest is False or keep_largest is None:
        return set()
    if keep_largest is True:
        return set(classes)
    return {int(c) for c in keep_largest} & set(classes)


def label(mask, connectivity=4, classes=None):
    """-> labels int32 [H,W] (0: unlabelled; ids 1..K in ascending order of the first pixel), rows: list of K dicts
    (cls, area, box, first)"""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2 and connectivity in (4, 8)
    H, W = mask.shape
    sel = class_set(classes)
    nbrs = N4 if connectivity == 4 else N8
    m = mask.tolist()
    labels = [[0] * W for _ in range(H)]
    rows = []
    for y in range(H):
        for x in range(W):
            v = m[y][x]
            if labels[y][x] or v >= MAX_CLASSES or v not in sel:
                continue
            k = len(rows) + 1                    # raster order: (y, x) is the component's smallest linear index
            labels[y][x] = k
            queue = deque([(y, x)])
            area, y0, x0, y1, x1 = 0, y, x, y, x
            while queue:
                cy, cx = queue.popleft()
                area += 1
                y0, x0, y1, x1 = min(y0, cy), min(x0, cx), max(y1, cy), max(x1, cx)
                for dy, dx in nbrs:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and not labels[ny][nx] and m[ny][nx] == v:
                        labels[ny][nx] = k
                        queue.append((ny, nx))
            rows.append({"cls": v, "area": area, "box": (y0, x0, y1 + 1, x1 + 1), "first": y * W + x})
    return np.asarray(labels, dtype=np.int32).reshape(H, W), rows


def clean(mask, labels, rows, min_area=0, keep_largest=False, classes=None):
    """-> cleaned mask uint8 [H,W], kept [K] (0/1), new_cls [K]"""
    mask = np.asarray(mask)
    H, W = mask.shape
    K = len(rows)
    keep = keep_set(keep_largest, class_set(classes))
    largest = {}                                  # class -> id of its largest component, the lowest id on a tie
    for k, r in enumerate(rows, 1):
        c = r["cls"]
        if c not in largest or r["area"] > rows[largest[c] - 1]["area"]:
            largest[c] = k
    removed = [False] * (K + 1)
    for k, r in enumerate(rows, 1):
        removed[k] = r["area"] < min_area or (r["cls"] in keep and largest[r["cls"]] != k)
    votes = np.zeros((K + 1, MAX_CLASSES), dtype=np.int64)
    m, lab = mask.tolist(), labels.tolist()
    for y in range(H):
        for x in range(W):
            k = lab[y][x]
            if not k or not removed[k]:
                continue
            for dy, dx in N4:                     # the vote neighbourhood is 4 whatever the connectivity
                ny, nx = y + dy, x + dx
                if not (0 <= ny < H and 0 <= nx < W):
                    continue
                kq, vq = lab[ny][nx], m[ny][nx]
                if kq == k:
                    continue
                stands = (vq < MAX_CLASSES) if kq == 0 else not removed[kq]
                if stands:
                    votes[k, vq] += 1
    new_cls = np.zeros(K, dtype=np.int32)
    kept = np.zeros(K, dtype=np.int32)
    for k, r in enumerate(rows, 1):
        c = r["cls"]
        if removed[k] and votes[k].max() > 0:
            c = int(np.argmax(votes[k]))          # first maximum: the lowest class on a tie
        new_cls[k - 1] = c
        kept[k - 1] = 0 if removed[k] else 1
    out = mask.copy()
    if K:
        lut = np.concatenate([[0], new_cls]).astype(np.uint8)
        sel = labels > 0
        out[sel] = lut[labels[sel]]
    return out, kept, new_cls


def components(mask, connectivity=4, classes=None, min_area=0, keep_largest=False):
    """Everything at once, as arrays: dict(labels, num, cls, area, box, first, kept, new_cls, mask)"""
    labels, rows = label(mask, connectivity, classes)
    out, kept, new_cls = clean(mask, labels, rows, min_area, keep_largest, classes)
    K = len(rows)
    return {"labels": labels, "num": K,
            "cls": np.asarray([r["cls"] for r in rows], dtype=np.int32).reshape(K),
            "area": np.asarray([r["area"] for r in rows], dtype=np.int32).reshape(K),
            "box": np.asarray([r["box"] for r in rows], dtype=np.int32).reshape(K, 4),
            "first": np.asarray([r["first"] for r in rows], dtype=np.int32).reshape(K),
            "kept": kept, "new_cls": new_cls, "mask": out}


# ---------------------------------------------------------------------------------------------- synthetic masks
SIZES = [(1, 1), (1, 9), (7, 1), (2, 3), (31, 33), (64, 64), (65, 129), (130, 259), (200, 37)]
PATTERNS = ["one_class", "checkerboard", "spiral", "comb", "u_shape", "rings", "noise2", "noise4", "blobs", "high_values"]
# more rows than the 1024 that the scan of the row counts takes per trip (csrc/scan.hpp): two trips and three, with a root on
# most rows.  Kept beside SIZES: the narrow masks need neither every pattern nor the cleaning cases
TALL_SIZES = [(1100, 3), (2049, 2)]
TALL_PATTERNS = ["row_stripes", "noise2"]


def _rng(H, W, salt):
    return np.random.default_rng(1000003 * H + 1009 * W + salt)


def blobs(H, W, speckle=0.02, seed=0):
    """A smooth blob mask (background 0, two animals 1 / 2 with a boundary ring 3) with `speckle` of the pixels redrawn:
    the realistic case"""
    rng = _rng(H, W, 17 + seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    m = np.zeros((H, W), dtype=np.uint8)
    for cls, (cy, cx, ry, rx) in ((1, (0.35, 0.3, 0.25, 0.2)), (2, (0.65, 0.7, 0.22, 0.25))):
        d = ((yy - cy * H) / max(ry * H, 1.0)) ** 2 + ((xx - cx * W) / max(rx * W, 1.0)) ** 2
        m[d <= 1.0] = cls
        m[(d > 1.0) & (d <= 1.25)] = 3
    hit = rng.random((H, W)) < speckle
    m[hit] = rng.integers(0, 4, size=(H, W), dtype=np.uint8)[hit]
    return m


def pattern(name, H, W):
    m = np.zeros((H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "one_class":
        m[:] = 2
    elif name == "checkerboard":
        m[:] = ((yy + xx) & 1).astype(np.uint8)          # class 1 where y + x is odd; classes=(1,) labels those alone
    elif name == "spiral":
        m[:] = _spiral(H, W)
    elif name == "comb":                                  # teeth two pixels apart hanging from a spine in the LAST row
        m[:, ::2] = 1
        m[H - 1, :] = 1
    elif name == "u_shape":                               # two arms in the first and last column, joined in the last row
        m[:, 0] = 2
        m[:, W - 1] = 2
        m[H - 1, :] = 2
    elif name == "rings":                                 # concentric rectangular rings of alternating classes 1, 2, 3
        d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
        m[:] = (1 + (d // 2) % 3).astype(np.uint8)
    elif name == "row_stripes":                           # rows of the classes 1, 2, 1, ...: every row is a component
        m[:] = (1 + (yy & 1)).astype(np.uint8)
    elif name == "noise2":
        m[:] = _rng(H, W, 2).integers(0, 2, size=(H, W), dtype=np.uint8)
    elif name == "noise4":
        m[:] = _rng(H, W, 4).integers(0, 4, size=(H, W), dtype=np.uint8)
    elif name == "blobs":
        m[:] = blobs(H, W)
    elif name == "high_values":                           # blobs with a tenth of the pixels at 8 / 200 / 255: never labelled
        rng = _rng(H, W, 8)
        m[:] = blobs(H, W)
        hit = rng.random((H, W)) < 0.1
        m[hit] = rng.choice(np.asarray([8, 200, 255], dtype=np.uint8), size=(H, W))[hit]
    else:
        raise KeyError(name)
    return m


def _spiral(H, W):
    """A one-pixel-wide path of class 1 that winds inwards with a one-pixel gap between its turns: one component whose
    pixels are far apart along the path although close in the image"""
    m = np.zeros((H, W), dtype=np.uint8)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W
    y = x = d = failed = 0
    m[0, 0] = 1
    while failed < 2:                                     # a step needs a free cell with a free (or no) cell behind it
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        ny, nx, by, bx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not m[ny, nx] and (not inside(by, bx) or not m[by, bx]):
            y, x, failed = ny, nx, 0
            m[y, x] = 1
        else:
            d, failed = (d + 1) % 4, failed + 1
    return m
