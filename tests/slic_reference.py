"""NumPy restatement of DESIGN.md 3.24 (superpixels), written from the definition: pixel-centric, the nine candidates of a
pixel evaluated as whole-image arrays in index order, the sums taken with np.add.at over the TRUE coordinates (no tiles, no
runs, no offsets from a home cell), so it shares no mistake with csrc/slic.hip.  Every value is an exact integer: int64
arrays whose largest entry stays below 2^43 (a distance), Python ints nowhere needed.  The device must equal every integer
here bit for bit."""
import numpy as np

MIN_STEP, MAX_STEP = 4, 64
MAX_COMPACTNESS, MAX_ITERATIONS = 255, 20
SPACES = ("rgb", "ycc")
MAX_CLASSES = 8
NONE = -1


def features(image, space):
    """uint8 [H,W,C], C in {1, 3, 4} -> int64 [H,W,3] of bytes: "rgb" the channels, "ycc" the integer transform with arithmetic
    shifts, each value clamped to 0..255; a fourth channel is ignored; grey has the one feature c0 in either space"""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] in (1, 3, 4) and space in SPACES
    H, W, C = image.shape
    f = np.zeros((H, W, 3), dtype=np.int64)
    if C == 1:
        f[..., 0] = image[..., 0]
        return f
    R, G, B = (image[..., a].astype(np.int64) for a in range(3))
    if space == "rgb":
        f[..., 0], f[..., 1], f[..., 2] = R, G, B
    else:
        f[..., 0] = (77 * R + 150 * G + 29 * B + 128) >> 8
        f[..., 1] = ((-43 * R - 85 * G + 128 * B + 128) >> 8) + 128
        f[..., 2] = ((128 * R - 107 * G - 21 * B + 128) >> 8) + 128
    return np.clip(f, 0, 255)


def grid_of(H, W, S):
    """-> (ny, nx)"""
    return -(-H // S), -(-W // S)


def start_centres(f, S):
    """int64 [K,5]: (Y, X, C0, C1, C2) in 1/16 units"""
    H, W = f.shape[:2]
    ny, nx = grid_of(H, W, S)
    cen = np.zeros((ny * nx, 5), dtype=np.int64)
    for i in range(ny):
        for j in range(nx):
            y, x = min(i * S + S // 2, H - 1), min(j * S + S // 2, W - 1)
            cen[i * nx + j] = (16 * y, 16 * x, *(16 * f[y, x]))
    return cen


def distances(f, cen, S, m, di, dj):
    """(D int64 [H,W], k int64 [H,W], valid bool [H,W]) of the candidate whose home cell is the pixel's cell moved by (di, dj)"""
    H, W = f.shape[:2]
    ny, nx = grid_of(H, W, S)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    gy, gx = yy // S + di, xx // S + dj
    valid = (gy >= 0) & (gy < ny) & (gx >= 0) & (gx < nx)
    k = np.where(valid, gy * nx + gx, 0)
    c = cen[k]                                                                     # [H,W,5]
    colour = ((16 * f - c[..., 2:]) ** 2).sum(-1)
    place = (16 * yy - c[..., 0]) ** 2 + (16 * xx - c[..., 1]) ** 2
    return S * S * colour + m * m * place, k, valid


def assign(f, cen, S, m):
    """int64 [H,W]: the candidate of smallest D, the lowest k on a tie"""
    H, W = f.shape[:2]
    best = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
    lab = np.full((H, W), -1, dtype=np.int64)
    for di in (-1, 0, 1):                                                          # k grows with (di, dj): a strict < keeps the lowest
        for dj in (-1, 0, 1):
            D, k, valid = distances(f, cen, S, m, di, dj)
            take = valid & (D < best)
            best = np.where(take, D, best)
            lab = np.where(take, k, lab)
    assert (lab >= 0).all()
    return lab


def update(f, lab, cen):
    """-> (the new centres int64 [K,5], n int64 [K])"""
    H, W = lab.shape
    K = cen.shape[0]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    n = np.zeros(K, dtype=np.int64)
    sums = np.zeros((K, 5), dtype=np.int64)
    flat = lab.ravel()
    np.add.at(n, flat, 1)
    for a, v in enumerate((yy, xx, f[..., 0], f[..., 1], f[..., 2])):
        np.add.at(sums[:, a], flat, v.ravel())
    new = cen.copy()
    live = n > 0
    new[live] = (32 * sums[live] + n[live, None]) // (2 * n[live, None])
    return new, n


def slic(image, step=16, compactness=20, iterations=10, space="ycc"):
    """-> (labels int32 [H,W] of the last assignment, centres int32 [K,5] after the last update, counts int32 [K] of the last
    assignment)"""
    S, m, T = int(step), int(compactness), int(iterations)
    assert MIN_STEP <= S <= MAX_STEP and 1 <= m <= MAX_COMPACTNESS and 1 <= T <= MAX_ITERATIONS
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[..., None]
    f = features(image, space)
    cen = start_centres(f, S)
    for _ in range(T):
        lab = assign(f, cen, S, m)
        cen, n = update(f, lab, cen)
    return lab.astype(np.int32), cen.astype(np.int32), n.astype(np.int32)


# ------------------------------------------------------------------------------------------------ vote and snap
def share_of(min_share):
    """the public layer's float in [0, 1] -> 0..256 of 256: floor(256 f + 1/2), rounded once"""
    return int(np.floor(256.0 * float(min_share) + 0.5))


def vote(labels, mask, K, weights=None, classes=range(MAX_CLASSES)):
    """int64 [K,8]: hist[k][c] += w(p) over the pixels with 0 <= labels[p] < K and mask[p] = c in classes"""
    labels, mask = np.asarray(labels).astype(np.int64), np.asarray(mask)
    assert labels.shape == mask.shape and mask.dtype == np.uint8
    w = np.ones(mask.shape, dtype=np.int64) if weights is None else np.asarray(weights).astype(np.int64)
    ok = (labels >= 0) & (labels < K) & np.isin(mask, [c for c in classes])
    assert all(0 <= c < MAX_CLASSES for c in classes)
    hist = np.zeros((K, MAX_CLASSES), dtype=np.int64)
    np.add.at(hist, (labels[ok], mask[ok].astype(np.int64)), w[ok])
    return hist


def winners(hist):
    """int32 [K]: the class of the largest entry, the lowest on a tie, -1 for a row of zeros"""
    w = np.argmax(hist, axis=1).astype(np.int32)                                   # argmax takes the first of equals
    w[hist.max(axis=1) == 0] = NONE
    return w


def snap(labels, mask, K, weights=None, classes=range(MAX_CLASSES), fill=(), min_share=128):
    """-> (out uint8 [H,W], hist int64 [K,8], winner int32 [K]); min_share in 0..256 of 256"""
    labels, mask = np.asarray(labels).astype(np.int64), np.asarray(mask)
    classes, fill = sorted(set(int(c) for c in classes)), sorted(set(int(v) for v in fill))
    assert not set(classes) & set(fill) and 0 <= min_share <= 256
    hist = vote(labels, mask, K, weights, classes)
    win = winners(hist)
    top = hist.max(axis=1)
    passes = (win >= 0) & (256 * top >= min_share * hist.sum(axis=1))
    inside = (labels >= 0) & (labels < K)
    k = np.where(inside, labels, 0)
    paint = inside & passes[k] & np.isin(mask, classes + fill)
    out = np.where(paint, win[k], mask).astype(np.uint8)
    return out, hist, win
