"""NumPy int64 restatement of DESIGN.md 3.18 (label rasterisation), shared by tests/test_raster_host.py and
tests/test_gpu_raster.py.  Written from the definition: per shape a crossing count per pixel, edge by edge, from the row rule
and the inequality as they are stated -- no toggles, no prefix XOR, no division.  The run-length form is expanded count by
count.  The string codec is a second, independent writing of COCO's.  Nothing here is imported by the package, and nothing
of the package is imported here.

A shape is a dict: {"rings": [xy, ...], "value": v} or {"rle": {"size": [H, W], "counts": [...] | str}, "value": v}."""
import numpy as np


def quantize(xy):
    """[n,2] pixel-corner coordinates -> int64 with 8 fractional bits: floor(v * 256 + 0.5)"""
    a = np.asarray(xy)
    if a.dtype.kind == "f":
        return np.floor(a.astype(np.float64) * 256 + 0.5).astype(np.int64)
    return a.astype(np.int64) * 256


def polygon_inside(rings, H, W):
    """bool [H,W]: an odd number of counting crossings over ALL rings (already quantised, int64 [n,2])"""
    Yc = 256 * np.arange(H, dtype=np.int64) + 128
    Xc = 256 * np.arange(W, dtype=np.int64) + 128
    ys = np.concatenate([r[:, 1] for r in rings])
    # rows a crossing can exist in (a window only to keep the count array small; the row rule below decides)
    lo = int(max(0, min(H, (int(ys.min()) - 128) // 256)))
    hi = int(max(lo, min(H, (int(ys.max()) - 128) // 256 + 2)))
    cnt = np.zeros((hi - lo, W), np.int64)
    for r in rings:
        n = len(r)
        for i in range(n):
            X0, Y0 = (int(v) for v in r[i])
            X1, Y1 = (int(v) for v in r[(i + 1) % n])
            if Y0 == Y1:
                continue                                   # horizontal edges never cross
            if Y0 > Y1:
                X0, Y0, X1, Y1 = X1, Y1, X0, Y0
            rows = np.flatnonzero((Y0 <= Yc[lo:hi]) & (Yc[lo:hi] < Y1))
            if rows.size == 0:
                continue
            lhs = (X1 - X0) * (Yc[lo:hi][rows] - Y0)
            rhs = (Xc - X0) * (Y1 - Y0)
            cnt[rows] += lhs[:, None] <= rhs[None, :]
    inside = np.zeros((H, W), bool)
    inside[lo:hi] = (cnt & 1).astype(bool)
    return inside


def string_to_counts(s):
    """COCO's compressed string -> counts: 5-bit groups, least significant first, bit 0x20 continues, sign from bit 0x10 of the
    last group; from the fourth count on the value is a difference to the count two before"""
    vals, groups = [], []
    for ch in s:
        g = ord(ch) - 48
        groups.append(g & 31)
        if not g & 32:
            v = sum(b << (5 * k) for k, b in enumerate(groups))
            if groups[-1] & 16:
                v -= 1 << (5 * len(groups))
            vals.append(v)
            groups = []
    assert not groups, "the string ends inside a count"
    for i in range(3, len(vals)):
        vals[i] += vals[i - 2]
    return vals


def counts_to_string(counts):
    """the shortest code of every value: n groups hold the two's complement range -2^(5n-1) .. 2^(5n-1) - 1"""
    counts = [int(c) for c in counts]
    out = []
    for i, c in enumerate(counts):
        v = c - counts[i - 2] if i > 2 else c
        n = 1
        while not -(1 << (5 * n - 1)) <= v < (1 << (5 * n - 1)):
            n += 1
        u = v % (1 << (5 * n))                             # two's complement in 5n bits
        for k in range(n):
            out.append(chr(((u >> (5 * k)) & 31) + (32 if k < n - 1 else 0) + 48))
    return "".join(out)


def rle_inside(rle, H, W):
    counts = rle["counts"]
    if isinstance(counts, str):
        counts = string_to_counts(counts)
    assert list(rle["size"]) == [H, W] and sum(counts) == H * W and min(counts, default=0) >= 0
    bits = np.repeat(np.arange(len(counts)) & 1, counts)
    return bits.reshape(W, H).T.astype(bool)


def shape_inside(shape, H, W):
    if "rings" in shape:
        return polygon_inside([quantize(r) for r in shape["rings"]], H, W)
    return rle_inside(shape["rle"], H, W)


def render(shapes, H, W, fill=0):
    """uint8 [H,W]: fill, then the shapes in list order, a later one over an earlier one"""
    lab = np.full((H, W), fill, np.uint8)
    for s in shapes:
        lab[shape_inside(s, H, W)] = s["value"]
    return lab


def mask_to_counts(inside):
    """bool [H,W] -> COCO's uncompressed counts (column-major, the first count is background)"""
    cm = np.ascontiguousarray(inside.T).reshape(-1).astype(np.int8)
    change = np.flatnonzero(np.diff(cm)) + 1
    counts = np.diff(np.concatenate([[0], change, [cm.size]])).tolist()
    return ([0] if cm[0] else []) + counts
