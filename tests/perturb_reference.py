"""NumPy restatement of the robustness perturbations (include/segk.h SEGK_PERTURB_*) -- a helper, not a
test.  It shares no code with image_segmentation_amd.robustness: its own hash, its own tables (the normal quantile comes from
the standard library), and a blur that reflects at EVERY pass.  What the host draws (per-image seeds, occlusion corners) are
inputs here."""
from statistics import NormalDist

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix(seed, idx):
    """splitmix64 finaliser of idx + seed * 0x9E3779B97F4A7C15 (idx: uint64 array), wrapping."""
    with np.errstate(over="ignore"):
        z = idx.astype(np.uint64) + np.uint64(seed & 0xFFFFFFFFFFFFFFFF) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def element_hash(seed, H, W):
    """uint64 [H,W,3]: the hash of element e = (y W + x) 3 + c."""
    return splitmix(seed, np.arange(H * W * 3, dtype=np.uint64)).reshape(H, W, 3)


def gauss_table(std):
    nd = NormalDist()
    z = np.array([nd.inv_cdf((j + 0.5) / 4096.0) for j in range(4096)], dtype=np.float64)
    return np.rint(float(std) * z).astype(np.int16)


def lut(kind, level):
    v = np.arange(256, dtype=np.float64)
    if kind in ("contrast_increase", "contrast_decrease"):
        t = np.rint(v * float(level))
    elif kind == "brightness_increase":
        t = v + float(level)
    elif kind == "brightness_decrease":
        t = v - float(level)
    else:
        raise ValueError(kind)
    return np.clip(t, 0, 255).astype(np.uint8)


def apply_lut(img, kind, level):
    return lut(kind, level)[img[..., :3]]


def gaussian_noise(img, std, seed):
    H, W = img.shape[:2]
    n = gauss_table(std)[(element_hash(seed, H, W) >> np.uint64(52)).astype(np.int64)].astype(np.int64)
    return np.clip(img[..., :3].astype(np.int64) + n, 0, 255).astype(np.uint8)


def salt_and_pepper(img, amount, seed):
    H, W = img.shape[:2]
    h = element_hash(seed, H, W)
    hit = (h >> np.uint64(40)).astype(np.int64) < int(np.floor(float(amount) * (1 << 24)))
    salt = ((h >> np.uint64(39)) & np.uint64(1)).astype(bool)
    return np.where(hit, np.where(salt, 255, 0), img[..., :3]).astype(np.uint8)


def occlude(img, y0, x0, e):
    out = img[..., :3].copy()
    out[y0:y0 + e, x0:x0 + e] = 0
    return out


def reflect101(i, n):
    """i mod 2 (n - 1), folded; 0 for n = 1 (i: integer array)."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def blur_plain(a):
    """One pass on an int array [H,W,...] WITHOUT borders: the result is [H-2, W-2, ...]."""
    a = a.astype(np.int64)
    h = a[:, :-2] + 2 * a[:, 1:-1] + a[:, 2:]
    return (h[:-2] + 2 * h[1:-1] + h[2:] + 8) >> 4


def extend(a, k):
    """Reflect-101 extension by k on every side (periodic: k may exceed the image)."""
    H, W = a.shape[:2]
    return a[reflect101(np.arange(-k, H + k), H)][:, reflect101(np.arange(-k, W + k), W)]


def blur_pass(a):
    """One pass with reflect-101 borders."""
    return blur_plain(extend(a, 1))


def blur(img, k):
    """k passes, each with its own reflection."""
    a = img[..., :3].astype(np.int64)
    for _ in range(int(k)):
        a = blur_pass(a)
    return a.astype(np.uint8)


def blur_extend_once(img, k):
    """Extend once by k, then k plain passes (what the kernel does in LDS)."""
    a = extend(img[..., :3].astype(np.int64), int(k))
    for _ in range(int(k)):
        a = blur_plain(a)
    return a.astype(np.uint8)
