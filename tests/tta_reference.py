"""NumPy restatement of the multi-view merge (segk_predict_merge), in float64 or in float32 with the
kernel's expression order.  There is no reference code for this feature: the project defines the result and this file pins
it.  Host-only.

A view is a dict: slot [C,T,T] array, pad_top, pad_left, nh, nw (the window of the flipped image in the slot), flip (bit 0:
x, bit 1: y), kind (0 logits / 1 probabilities), weight (any positive number; normalised here as tta.view_table does)."""
import math

import numpy as np

FLIPS = {"": 0, "h": 1, "v": 2, "hv": 3}


def normalised_weights(weights):
    """w_v / sum w, computed in float64 and rounded once to float32 (what the device table holds)"""
    total = math.fsum(float(w) for w in weights)
    return np.asarray([float(w) / total for w in weights], dtype=np.float64).astype(np.float32)


def src_index(o, scale, n, ft):
    """ATen's area_pixel_compute_source_index, align_corners=False: taps i0, i1 and the weight of i1"""
    s = scale * (o.astype(ft) + ft(0.5)) - ft(0.5)
    s = np.where(s < 0, ft(0), s).astype(ft)
    i0 = np.minimum(s.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    return i0, i1, (s - i0.astype(ft)).astype(ft)


def nearest_index(o, scale, n, ft):
    return np.minimum(np.floor(o.astype(ft) * scale).astype(np.int64), n - 1)


def sample_view(view, oh, ow, mode, ft):
    """z [C,oh,ow]: the view's window resized to (oh, ow) (the arithmetic of segk_crop_resize) and read at the flipped pixel"""
    slot = np.asarray(view["slot"]).astype(ft)
    nh, nw, pt, pl = view["nh"], view["nw"], view["pad_top"], view["pad_left"]
    win = slot[:, pt:pt + nh, pl:pl + nw]
    sy = np.arange(oh)[::-1] if view["flip"] & 2 else np.arange(oh)
    sx = np.arange(ow)[::-1] if view["flip"] & 1 else np.arange(ow)
    sh, sw = ft(nh) / ft(oh), ft(nw) / ft(ow)
    if mode == 1:
        y, x = nearest_index(sy, sh, nh, ft), nearest_index(sx, sw, nw, ft)
        return win[:, y[:, None], x[None, :]]
    y0, y1, ly = src_index(sy, sh, nh, ft)
    x0, x1, lx = src_index(sx, sw, nw, ft)
    ly, lx = ly[:, None], lx[None, :]
    a, b = win[:, y0[:, None], x0[None, :]], win[:, y0[:, None], x1[None, :]]
    d, e = win[:, y1[:, None], x0[None, :]], win[:, y1[:, None], x1[None, :]]
    one = ft(1)
    return ((one - ly) * ((one - lx) * a + lx * b) + ly * ((one - lx) * d + lx * e)).astype(ft)


def softmax(z):
    """m = max z, e_k = exp(z_k - m), p_k = e_k / sum_k e_k, the sum in class order"""
    m = z[0]
    for k in range(1, len(z)):
        m = np.where(z[k] > m, z[k], m)
    e = np.exp(z - m[None])
    total = np.zeros_like(m)
    for k in range(len(z)):
        total = total + e[k]
    return e / total[None]


def argmax_first_nan_max(acc):
    """first maximum over axis 0, NaN maximal (torch.argmax; segk_predict_mask)"""
    best, bv = np.zeros(acc.shape[1:], dtype=np.int64), acc[0].copy()
    for k in range(1, len(acc)):
        take = (acc[k] > bv) | (np.isnan(acc[k]) & ~np.isnan(bv))
        bv = np.where(take, acc[k], bv)
        best = np.where(take, k, best)
    return best


def merge_views(views, oh, ow, merge="prob", mode=0, dtype=np.float64):
    """-> (mask uint8 [oh,ow], confidence uint8 [oh,ow], scores dtype [C,oh,ow], acc dtype [C,oh,ow])"""
    ft = np.dtype(dtype).type
    weights = normalised_weights([v["weight"] for v in views])
    acc = None
    with np.errstate(all="ignore"):
        for view, w in zip(views, weights):
            z = sample_view(view, oh, ow, mode, ft)
            s = softmax(z) if (merge == "prob" and view["kind"] == 0) else z
            acc = (np.zeros_like(s) if acc is None else acc) + ft(w) * s
            acc = acc.astype(ft)
        mask = argmax_first_nan_max(acc)
        if merge == "prob":
            total = np.zeros_like(acc[0])
            for k in range(len(acc)):
                total = total + acc[k]
            scores = acc / total[None]
        else:
            scores = softmax(acc)
        scores = scores.astype(ft)
        pb = np.take_along_axis(scores, mask[None], axis=0)[0]
        c = ft(255) * pb + ft(0.5)
        c = np.where(c >= 0, np.minimum(c, ft(255)), ft(0))       # a NaN confidence is stored as 0
    return mask.astype(np.uint8), c.astype(np.uint8), scores, acc


def flip_image(img, flip, axes=(-2, -1)):
    """the flipped image: bit 0 reverses x (axes[1]), bit 1 reverses y (axes[0])"""
    out = np.asarray(img)
    if flip & 2:
        out = np.flip(out, axes[0])
    if flip & 1:
        out = np.flip(out, axes[1])
    return out
