"""NumPy / pure-Python restatement of DESIGN.md 3.22 (mixed-sample augmentation): the geometry, the paste bit of the three
modes with their selection keys, the write rule, the seam and the pasted count.  The device (csrc/mix.hip behind
image_segmentation_amd/mix.py) must equal every array here bit for bit.  Component ids come from tests/components_reference.py;
splitmix is restated with Python integers.  Images are handled as raw integer bit patterns: copies move bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as CR                                                  # noqa: E402

NONE, BOX, CLASS, OBJECT = range(4)
M64 = (1 << 64) - 1
DEFAULTS = dict(exclude=(), n_classes=None, seam_value=None, things=(1, 2, 3, 4, 5, 6, 7), connectivity=4, min_area=64,
                max_area=None, max_objects=4, max_components=1024)


def splitmix(seed, i):
    """csrc/common.hpp: the splitmix64 finaliser of i + seed * 0x9E3779B97F4A7C15, modulo 2^64"""
    z = (i + seed * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, i):
    return (splitmix(seed, i) & (M64 ^ 0xFFFFFF)) | i


def smallest(seed, candidates, k):
    """the k candidates with the smallest keys"""
    return set(sorted(candidates, key=lambda i: key(seed, i))[:k])


def as_bytes(label):
    """int64 [H,W]: the value where it lies in 0..255, else -1 ("outside")"""
    v = np.asarray(label).astype(np.int64)
    return np.where((v < 0) | (v > 255), -1, v)


def candidate_classes(label_p, exclude=()):
    v = as_bytes(label_p)
    return sorted(set(int(c) for c in np.unique(v) if c >= 0) - set(int(e) for e in exclude))


def select_classes(label_p, seed, exclude=(), n_classes=None):
    """-> bool [256]"""
    cand = candidate_classes(label_p, exclude)
    n = len(cand)
    k = (n + 1) // 2 if n_classes is None else min(n, n_classes)
    sel = np.zeros(256, dtype=bool)
    for c in smallest(seed, cand, k):
        sel[c] = True
    return sel


_label_cache = {}


def object_ids(label_p, things, connectivity):
    """-> (ids int32 [H,W], rows) of the partner's byte map (outside -> 255) under components_reference.label"""
    v = as_bytes(label_p)
    mask = np.where(v < 0, 255, v).astype(np.uint8)
    k = (mask.tobytes(), mask.shape, tuple(sorted(things)), connectivity)
    if k not in _label_cache:
        _label_cache[k] = CR.label(mask, connectivity, things)
    return _label_cache[k]


def select_objects(label_p, seed, things=DEFAULTS["things"], connectivity=4, min_area=64, max_area=None, max_objects=4,
                   max_components=1024):
    """-> (ids int32 [H,W], the set of selected ids, K)"""
    ids, rows = object_ids(label_p, things, connectivity)
    K = len(rows)
    hi = (1 << 30) if max_area is None else max_area
    cand = [i for i in range(1, min(K, max_components) + 1)
            if rows[i - 1]["cls"] in set(things) and min_area <= rows[i - 1]["area"] <= hi]
    return ids, smallest(seed, cand, min(len(cand), max_objects)), K


def source(plan, H, W):
    """-> (ys, xs, inside): the partner pixel every output pixel looks at"""
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    ys = Y - plan.dy
    xr = X - plan.dx
    xs = W - 1 - xr if plan.flip else xr
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    return ys, xs, inside


def paste_bits(plan, labels, **opt):
    """m bool [H,W] of one sample: labels int [B,H,W]"""
    o = dict(DEFAULTS, **opt)
    B, H, W = labels.shape
    m = np.zeros((H, W), dtype=bool)
    if plan.mode == NONE:
        return m
    ys, xs, inside = source(plan, H, W)
    yc, xc = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    lab_p = labels[plan.partner]
    if plan.mode == BOX:
        y0, x0, y1, x1 = plan.box
        Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        m = (Y >= y0) & (Y < y1) & (X >= x0) & (X < x1)
    elif plan.mode == CLASS:
        sel = select_classes(lab_p, plan.seed, o["exclude"], o["n_classes"])
        v = as_bytes(lab_p)[yc, xc]
        m = (v >= 0) & sel[np.clip(v, 0, 255)]
    elif plan.mode == OBJECT:
        ids, chosen, _ = select_objects(lab_p, plan.seed, o["things"], o["connectivity"], o["min_area"], o["max_area"],
                                        o["max_objects"], o["max_components"])
        m = np.isin(ids[yc, xc], sorted(chosen)) if chosen else np.zeros((H, W), dtype=bool)
    else:
        raise ValueError(plan.mode)
    return m & inside


def seam_of(m):
    """bool [H,W]: a 4-neighbour inside the image has another paste bit"""
    s = np.zeros_like(m)
    s[1:, :] |= m[1:, :] != m[:-1, :]
    s[:-1, :] |= m[:-1, :] != m[1:, :]
    s[:, 1:] |= m[:, 1:] != m[:, :-1]
    s[:, :-1] |= m[:, :-1] != m[:, 1:]
    return s


def mix(X, y, plans, nhwc=False, **opt):
    """X: integer bit patterns [B,C,H,W] (or [B,H,W,C] with nhwc), y: labels [B,H,W] (or [B,1,H,W]) -> (X', y', pasted int32
    [B], bits bool [B,H,W])"""
    o = dict(DEFAULTS, **opt)
    X, y = np.asarray(X), np.asarray(y)
    shape = y.shape
    lab = y.reshape(shape[0], shape[-2], shape[-1])
    B, H, W = lab.shape
    Xo, yo = X.copy(), lab.copy()
    pasted = np.zeros(B, dtype=np.int32)
    bits = np.zeros((B, H, W), dtype=bool)
    for b, plan in enumerate(plans):
        m = paste_bits(plan, lab, **opt)
        bits[b] = m
        pasted[b] = int(m.sum())
        ys, xs, _ = source(plan, H, W)
        yc, xc = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
        p = plan.partner
        yo[b] = np.where(m, lab[p][yc, xc], lab[b])
        if nhwc:
            Xo[b] = np.where(m[:, :, None], X[p][yc, xc, :], X[b])
        else:
            Xo[b] = np.where(m[None], X[p][:, yc, xc], X[b])
        if o["seam_value"] is not None:
            yo[b][seam_of(m)] = o["seam_value"]
    return Xo, yo.reshape(shape), pasted, bits
