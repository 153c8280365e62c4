"""NumPy restatement of tiled prediction (segk_tile_gather / segk_tile_gather_u8 / segk_predict_tiles), in
float64 or in float32 with the kernel's expression order.  There is no reference code for this feature: the project defines
the result and this file pins it.  Host-only.

Tiles are numbered row-major, t = iy * nx + ix; Y is [ny * nx, C, T, T]."""
import numpy as np

from tta_reference import argmax_first_nan_max, softmax


def tile_axis(L, T, o):
    """origins of the tiles of an axis of length L: one centred tile when L <= T, else min(i s, L - T), s = T - o"""
    assert L >= 1 and T >= 1 and 0 <= o <= T // 2
    if L <= T:
        return [-((T - L) // 2)]
    s = T - o
    n = -(-(L - T) // s) + 1
    return [min(i * s, L - T) for i in range(n)]


def reflect_index(g, L):
    """r(g, L): reflection without repeating the edge pixel, as often as needed"""
    if L == 1:
        return 0
    m = 2 * L - 2
    j = g % m                                   # Python's %: non-negative
    return j if j < L else m - j


def source_index(origin, T, L, pad):
    """(index [T] into the axis, keep [T]) of a tile's coordinates origin .. origin + T - 1"""
    g = np.arange(origin, origin + T)
    inside = (g >= 0) & (g < L)
    if pad == "reflect":
        return np.asarray([reflect_index(int(v), L) for v in g]), np.ones(T, bool)
    return np.clip(g, 0, L - 1), inside


def gather(img, T, o, pad):
    """uint8 [H,W,Cin] (alpha dropped, (float32)u8 / 255.0f) or float [C,H,W] -> float32 [ny * nx, c, T, T]"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        if img.ndim == 2:
            img = img[:, :, None]
        chw = (img[:, :, :3].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    else:
        chw = img.astype(np.float32)
    _, H, W = chw.shape
    out = []
    for y0 in tile_axis(H, T, o):
        iy, ky = source_index(y0, T, H, pad)
        for x0 in tile_axis(W, T, o):
            ix, kx = source_index(x0, T, W, pad)
            tile = chw[:, iy[:, None], ix[None, :]]
            out.append(np.where((ky[:, None] & kx[None, :])[None], tile, np.float32(0)))
    return np.stack(out).astype(np.float32)


def window_axis(T, window):
    u = np.arange(T)
    return np.ones(T, np.int64) if window == "flat" else np.minimum(u, T - 1 - u) + 1


def tile_regions(H, W, T, o):
    """[(t, image rows slice, image cols slice, tile rows slice, tile cols slice)] in row-major tile order"""
    ys, xs = tile_axis(H, T, o), tile_axis(W, T, o)
    out = []
    for iy, y0 in enumerate(ys):
        ya, yb = max(y0, 0), min(y0 + T, H)
        for ix, x0 in enumerate(xs):
            xa, xb = max(x0, 0), min(x0 + T, W)
            out.append((iy * len(xs) + ix, slice(ya, yb), slice(xa, xb), slice(ya - y0, yb - y0), slice(xa - x0, xb - x0)))
    return out


def unmapped(H, W, T, o):
    """bool [ny * nx, T, T]: the positions of Y no pixel maps to (the padded border of a short axis)"""
    regions = tile_regions(H, W, T, o)
    m = np.ones((len(regions), T, T), bool)
    for t, _, _, ty, tx in regions:
        m[t, ty, tx] = False
    return m


def cover_count(H, W, T, o):
    n = np.zeros((H, W), np.int64)
    for _, gy, gx, _, _ in tile_regions(H, W, T, o):
        n[gy, gx] += 1
    return n


def device_candidates(g, L, T, o):
    """The covering tiles of coordinate g as the KERNEL finds them (csrc/tiles.hip: regular_range / candidate), ascending:
    [(tile, tile-local coordinate)].  tests/test_tiles_host.py holds it against tile_axis."""
    s = T - o
    n = 1 if L <= T else (L - T + s - 1) // s + 1
    last = -((T - L) // 2) if L <= T else L - T
    q = g // s
    ilo = q - 1 if (q >= 1 and (q - 1) * s + T - 1 >= g) else q
    ihi = min(q, n - 2)
    out = []
    for c in range(3):
        i = ilo + c if c < 2 else n - 1
        covers = (i <= ihi) if c < 2 else (g >= last)
        tile = min(i, n - 1)
        origin = last if tile == n - 1 else tile * s
        u = min(max(g - origin, 0), T - 1)
        if covers:
            out.append((tile, u))
    return out


def blend(Y, H, W, T, o, window="triangle", merge="prob", kind=0, dtype=np.float64):
    """-> (mask uint8 [H,W], confidence uint8 [H,W], scores dtype [C,H,W], a dtype [C,H,W]): a is acc ("prob") or acc / Wtot
    ("logit"), the array the argmax is taken of.  Per pixel the covering tiles are walked in row-major tile order:
    acc = acc + w * s, one rounding for the product and one for the sum in float32."""
    ft = np.dtype(dtype).type
    Y = np.asarray(Y)
    C = Y.shape[1]
    assert not (merge == "logit" and kind == 1)
    wa = window_axis(T, window)
    acc = np.zeros((C, H, W), dtype)
    wtot = np.zeros((H, W), dtype)
    with np.errstate(all="ignore"):
        for t, gy, gx, ty, tx in tile_regions(H, W, T, o):
            z = Y[t][:, ty, tx].astype(ft)
            s = softmax(z) if (merge == "prob" and kind == 0) else z
            w = (wa[ty][:, None] * wa[tx][None, :]).astype(ft)
            acc[:, gy, gx] = (acc[:, gy, gx] + (w[None] * s).astype(ft)).astype(ft)
            wtot[gy, gx] = wtot[gy, gx] + w
        if merge == "prob":
            a = acc
            total = np.zeros_like(acc[0])
            for k in range(C):
                total = total + acc[k]
            scores = acc / total[None]
        else:
            a = (acc / wtot[None]).astype(ft)
            scores = softmax(a)
        scores = scores.astype(ft)
        mask = argmax_first_nan_max(a)
        pb = np.take_along_axis(scores, mask[None], axis=0)[0]
        c = ft(255) * pb + ft(0.5)
        c = np.where(c >= 0, np.minimum(c, ft(255)), ft(0))       # a NaN confidence is stored as 0
    return mask.astype(np.uint8), c.astype(np.uint8), scores, a
