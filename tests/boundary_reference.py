"""NumPy restatement of DESIGN.md 3.23 (boundary quality), written from the definition by brute force: the band distance is
the primitive of 3.21 as morph_reference.py states it (shifted comparisons over every offset of the element), the nearest
contour pixel is an explicit minimum over all pairs -- no bit planes, no windows, so it shares no mistake with
csrc/boundary.hip.  The device must equal every integer here bit for bit."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_reference as MR                                                       # noqa: E402

MAX_CLASSES = 8
MAX_WIDTH = 32
BINS = 34
SHAPES = MR.SHAPES
VOID = 255


def published_width(H, W, ratio=0.02):
    """the rule of Cheng et al. 2021: 2 % of the image diagonal, at least one pixel"""
    return max(1, int(round(ratio * math.hypot(H, W))))


def class_maps(pred, label, C, ignore=()):
    """-> (P, G) uint8 maps of classes 0..C-1 and VOID: a label in `ignore`, >= C or outside 0..255 is void in both, a
    prediction >= C in P"""
    label = np.asarray(label).astype(np.int64)
    pred = np.asarray(pred).astype(np.int64)
    assert pred.shape == label.shape and pred.ndim == 2 and 1 <= C <= MAX_CLASSES
    void = (label < 0) | (label >= C)
    for v in ignore:
        void |= label == int(v)
    G = np.where(void, VOID, label).astype(np.uint8)
    P = np.where(void | (pred < 0) | (pred >= C), VOID, pred).astype(np.uint8)
    return P, G


def _keys(C):
    k = np.full(256, MR.WILD, dtype=np.int64)
    k[:C] = np.arange(C)
    return k


def band_mask(M, C, width, shape="square", image_border=True):
    """bool [H,W]: the non-void pixels of the class map M with D(p) <= width; D is 3.21's distance with key = class and
    void = wild, and with image_border the pixels outside the image differ from every class"""
    H, W = M.shape
    D = MR.distance(M, _keys(C), shape, width)
    inside = D <= MR.cap_of(shape, width)
    if image_border:
        yy, xx = np.mgrid[0:H, 0:W]
        b = np.minimum(np.minimum(yy + 1, xx + 1), np.minimum(H - yy, W - xx))
        inside = inside | (b <= width)                     # b^2 <= width^2 for the disk: the same test
    return inside & (M != VOID)


def contour(M, c):
    """bool [H,W]: pixels of class c with a 4-neighbour inside the image that is non-void and of another class"""
    H, W = M.shape
    other = (M != VOID) & (M != c)
    near = np.zeros((H, W), dtype=bool)
    near[1:] |= other[:-1]
    near[:-1] |= other[1:]
    near[:, 1:] |= other[:, :-1]
    near[:, :-1] |= other[:, 1:]
    return (M == c) & near


def bins_of(src, dst, max_distance):
    """for every pixel of the bool map src: the smallest t with t^2 >= the squared distance to the nearest pixel of dst, the
    overflow bin max_distance + 1 past max_distance or when dst is empty -> int64 [BINS] counts"""
    out = np.zeros(BINS, dtype=np.int64)
    ys, xs = np.nonzero(src)
    if len(ys) == 0:
        return out
    qy, qx = np.nonzero(dst)
    if len(qy) == 0:
        out[max_distance + 1] = len(ys)
        return out
    for k0 in range(0, len(ys), 512):                      # the explicit minimum, a slab of sources at a time
        dy = ys[k0:k0 + 512, None] - qy[None, :]
        dx = xs[k0:k0 + 512, None] - qx[None, :]
        d2 = (dy * dy + dx * dx).min(axis=1)
        for v in d2:
            t = 0
            while t * t < v:
                t += 1
            out[t if t <= max_distance else max_distance + 1] += 1
    return out


def hd95_of(hist_c, max_distance):
    """the pooled histogram [2][BINS] of one class and image -> None (no contour pixel) or the smallest bin whose cumulative
    count reaches 95 %, in integers"""
    pooled = hist_c[0] + hist_c[1]
    n = int(pooled.sum())
    if n == 0:
        return None
    cum = 0
    for t in range(max_distance + 2):
        cum += int(pooled[t])
        if 20 * cum >= 19 * n:
            return t
    raise AssertionError("unreachable")


def empty_stats():
    z = lambda *s: np.zeros(s, dtype=np.int64)
    return dict(band_g=z(MAX_CLASSES), band_p=z(MAX_CLASSES), band_i=z(MAX_CLASSES), band_conf=z(MAX_CLASSES, MAX_CLASSES),
                hist=z(2, MAX_CLASSES, BINS), hd_sum=z(MAX_CLASSES), hd_images=z(MAX_CLASSES), hd_capped=z(MAX_CLASSES))


_memo = {}


def boundary_stats(pred, label, C, width=None, max_distance=32, ignore=(), shape="square", image_border=True):
    """the statistics of one image pair: a dict of int64 arrays laid out as the device's (8 classes, BINS bins)"""
    pred, label = np.asarray(pred), np.asarray(label)
    H, W = label.shape
    if width is None:
        width = published_width(H, W)
    assert 1 <= width <= MAX_WIDTH and 1 <= max_distance <= MAX_WIDTH
    memo = (pred.shape, pred.dtype.str, pred.tobytes(), label.dtype.str, label.tobytes(), C, width, max_distance,
            tuple(sorted(int(v) for v in ignore)), shape, bool(image_border))
    if memo in _memo:
        return {k: v.copy() for k, v in _memo[memo].items()}
    P, G = class_maps(pred, label, C, ignore)
    Bg, Bp = band_mask(G, C, width, shape, image_border), band_mask(P, C, width, shape, image_border)
    st = empty_stats()
    for c in range(C):
        st["band_g"][c] = int(((G == c) & Bg).sum())
        st["band_p"][c] = int(((P == c) & Bp).sum())
        st["band_i"][c] = int(((G == c) & (P == c) & Bg & Bp).sum())
        for q in range(C):
            st["band_conf"][c, q] = int(((G == c) & (P == q) & Bg).sum())
        hkey = ("hist", P.shape, P.tobytes(), G.tobytes(), c, max_distance)     # the contours do not depend on the band
        if hkey not in _memo:
            Kg, Kp = contour(G, c), contour(P, c)
            _memo[hkey] = (bins_of(Kp, Kg, max_distance), bins_of(Kg, Kp, max_distance))
        st["hist"][0, c], st["hist"][1, c] = _memo[hkey]
        hd = hd95_of(st["hist"][:, c], max_distance)
        if hd is not None:
            if hd == max_distance + 1:
                st["hd_capped"][c] = 1
            else:
                st["hd_sum"][c], st["hd_images"][c] = hd, 1
    if len(_memo) > 4096:
        _memo.clear()
    _memo[memo] = {k: v.copy() for k, v in st.items()}
    return st


def add_stats(a, b):
    return {k: a[k] + b[k] for k in a}


def quality(st, C, tolerances=(1, 2, 3), max_distance=32, images=0):
    """the host finish of 3.23, restated on the reference's arrays (float64)"""
    div = lambda a, b: (a / b) if b else None
    mean = lambda v: (sum(x for x in v if x is not None) / len([x for x in v if x is not None])) if any(x is not None for x in v) else None
    out = {}
    bg, bp, bi = (st[k].tolist() for k in ("band_g", "band_p", "band_i"))
    conf = st["band_conf"].tolist()
    out["boundary_iou"] = [div(bi[c], bg[c] + bp[c] - bi[c]) for c in range(C)]
    out["mean_boundary_iou"] = mean(out["boundary_iou"])
    out["band_iou"] = [div(conf[c][c], sum(conf[c][:C]) + sum(conf[g][c] for g in range(C)) - conf[c][c]) for c in range(C)]
    out["mean_band_iou"] = mean(out["band_iou"])
    out["band_accuracy"] = div(sum(conf[c][c] for c in range(C)), sum(sum(conf[g][:C]) for g in range(C)))
    hist = st["hist"].tolist()
    out["contour_precision"], out["contour_recall"], out["contour_f"], out["mean_contour_f"] = {}, {}, {}, {}
    for th in tolerances:
        pr = [div(sum(hist[0][c][:th + 1]), sum(hist[0][c][:max_distance + 2])) for c in range(C)]
        rc = [div(sum(hist[1][c][:th + 1]), sum(hist[1][c][:max_distance + 2])) for c in range(C)]
        f = [None if p is None and r is None else (0.0 if not (p or 0.0) + (r or 0.0) else 2 * (p or 0.0) * (r or 0.0) / ((p or 0.0) + (r or 0.0)))
             for p, r in zip(pr, rc)]
        out["contour_precision"][th], out["contour_recall"][th], out["contour_f"][th] = pr, rc, f
        out["mean_contour_f"][th] = mean(f)
    out["hd95"] = [div(int(st["hd_sum"][c]), int(st["hd_images"][c])) for c in range(C)]
    out["mean_hd95"] = mean(out["hd95"])
    out["hd95_capped"] = [int(v) for v in st["hd_capped"][:C]]
    out["hd95_images"] = [int(v) for v in st["hd_images"][:C]]
    out["images"] = images
    out["tolerances"] = list(tolerances)
    out["max_distance"] = max_distance
    return out
