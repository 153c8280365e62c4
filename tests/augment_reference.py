"""NumPy restatement of the augmentation arithmetic, written from its definition and not from the
package: it shares no code with image_segmentation_amd/augment.py and takes nothing from it but the VALUES of the AugPlan it is
handed (op, source size, window, theta, alpha, b, seed).  Float64 appears only where the definition builds a table (cubic
weights, contrast LUT, Laplace inverse CDF, the rotation matrix before its Q16 rounding, the masking grid, the merge scale);
every pixel is computed with integers.  Not a test module: tests/test_augment_host.py and tests/test_gpu_augment.py import it.

    image, label = augment(img_u8_hwc, label_u8, plan, T, label_lut, label_fill)      # uint8 [T,T,3], int64 [T,T]
    image, label = merge(img1, lab1, img2, lab2, T)
    counts, weights = class_weights(list_of_label_arrays, C, ignore_index, unimportant, normalize_target_sum)
    counts = label_hist(labels, C, ignore); classes = rgb_classes(rgb_u8_n3)       # the two class-count entries

The end of the file holds the launch arithmetic of label_hist_kernel and the case table of tests/test_gpu_label_count_matrix.py."""
import math

import numpy as np

from oracle.fill import u01

RESIZE, CENTER_CROP, RANDOM_CROP, ROTATION, MASKING, GRAYSCALE, LAPLACE, BLUR, CONTRAST = range(9)
U64 = np.uint64


def splitmix(seed, i):
    """finaliser of i + seed * 0x9E3779B97F4A7C15 (mod 2^64), two multiply-xorshift rounds; uint64 array"""
    with np.errstate(over="ignore"):
        z = np.asarray(i).astype(np.uint64) + U64((int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def rgb_to_classes(rgb):
    """black or white -> 0, (128,0,0) -> 1, (0,128,0) -> 2, else 255; integer [H,W,3] -> int64 [H,W]"""
    p = (rgb[..., 0].astype(np.int64) << 16) | (rgb[..., 1].astype(np.int64) << 8) | rgb[..., 2].astype(np.int64)
    out = np.full(p.shape, 255, np.int64)
    out[(p == 0) | (p == 0xFFFFFF)] = 0
    out[p == 0x800000] = 1
    out[p == 0x008000] = 2
    return out


def label_classes(label):
    return rgb_to_classes(label) if label.ndim == 3 else label.astype(np.int64)


# ---------------------------------------------------------------------------------------------- tables
def cubic(S, T):
    """idx [T], coef [T,4] (int64): Keys a = -0.75 at f = (i + 0.5) S / T - 0.5; float64 weights, rint to 11 bits, residual to
    the largest tap (first of equals)"""
    a = -0.75
    f = (np.arange(T, dtype=np.float64) + 0.5) * S / T - 0.5
    fl = np.floor(f)
    t = f - fl
    x0, x1, x2, x3 = 1.0 + t, t, 1.0 - t, 2.0 - t
    w = np.empty((T, 4))
    w[:, 0] = ((a * x0 - 5.0 * a) * x0 + 8.0 * a) * x0 - 4.0 * a
    w[:, 1] = ((a + 2.0) * x1 - (a + 3.0)) * x1 * x1 + 1.0
    w[:, 2] = ((a + 2.0) * x2 - (a + 3.0)) * x2 * x2 + 1.0
    w[:, 3] = ((a * x3 - 5.0 * a) * x3 + 8.0 * a) * x3 - 4.0 * a
    q = np.rint(w * 2048.0).astype(np.int64)
    for i in range(T):
        q[i, int(np.argmax(q[i]))] += 2048 - int(q[i].sum())
    return fl.astype(np.int64), q


def contrast_table(alpha):
    v = np.arange(256, dtype=np.float64)
    return np.clip(np.floor(127.0 + alpha * (v - 127.0) + 0.5), 0, 255).astype(np.int64)


def laplace(b):
    u = (np.arange(4096, dtype=np.float64) + 0.5) / 4096
    d = u - 0.5
    return np.rint(-b * np.sign(d) * np.log(1.0 - 2.0 * np.abs(d))).astype(np.int64)


def rotation(H, W, theta):
    """Ha, Wa and the Q16 inverse map (clockwise rotation on the screen, about the centres (size - 1) / 2)"""
    th = math.radians(theta)
    c, s = math.cos(th), math.sin(th)
    Wa = max(1, int(math.floor(abs(W * c) + abs(H * s) + 0.5)))
    Ha = max(1, int(math.floor(abs(W * s) + abs(H * c) + 0.5)))
    cxs, cys, cxo, cyo = (W - 1) / 2.0, (H - 1) / 2.0, (Wa - 1) / 2.0, (Ha - 1) / 2.0
    m = [c, s, cxs - c * cxo - s * cyo, -s, c, cys + s * cxo - c * cyo]
    return Ha, Wa, [int(np.rint(v * 65536.0)) for v in m]


# ---------------------------------------------------------------------------------------------- stage A
def rotate(img, lab, theta, label_fill):
    """-> uint8-valued int64 [Ha,Wa,3], int64 [Ha,Wa] (classes)"""
    H, W = img.shape[:2]
    Ha, Wa, A = rotation(H, W, theta)
    y, x = np.indices((Ha, Wa), dtype=np.int64)
    SX = A[0] * x + A[1] * y + A[2]
    SY = A[3] * x + A[4] * y + A[5]
    ix, iy = SX >> 16, SY >> 16
    fx, fy = (SX >> 8) & 255, (SY >> 8) & 255
    src = img[..., :3].astype(np.int64)
    acc = np.zeros((Ha, Wa, 3), np.int64)
    for dy, dx, w in ((0, 0, (256 - fx) * (256 - fy)), (0, 1, fx * (256 - fy)), (1, 0, (256 - fx) * fy), (1, 1, fx * fy)):
        yy, xx = iy + dy, ix + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        p = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        acc += np.where(inside[..., None], w[..., None] * p, 0)
    out = (acc + 32768) >> 16
    nx, ny = (SX + 32768) >> 16, (SY + 32768) >> 16
    inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
    cls = label_classes(lab)
    lo = np.where(inside, cls[np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)], label_fill)
    return out, lo


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def blur(img):
    """12 x 12 box over rows y-6..y+5, columns x-6..x+5, reflect-101 (repeated), (sum + 72) // 144"""
    H, W = img.shape[:2]
    src = img[..., :3].astype(np.int64)
    ys = reflect101(np.arange(-6, H + 5), H)
    xs = reflect101(np.arange(-6, W + 5), W)
    ext = src[ys][:, xs]
    acc = np.zeros((H, W, 3), np.int64)
    for dy in range(12):
        for dx in range(12):
            acc += ext[dy:dy + H, dx:dx + W]
    return (acc + 72) // 144


# ---------------------------------------------------------------------------------------------- pointwise + stage B
def masking_cells(H, W, seed):
    """bool [H,W]: pixel lies in a dropped cell"""
    gh = min(H, max(3, int(math.floor(0.02 * H + 0.5))))
    gw = min(W, max(3, int(math.floor(0.02 * W + 0.5))))
    cy = (np.arange(H, dtype=np.int64) * gh) // H
    cx = (np.arange(W, dtype=np.int64) * gw) // W
    cell = cy[:, None] * gw + cx[None, :]
    return (splitmix(seed, cell) >> U64(40)).astype(np.int64) < int(math.floor(0.15 * (1 << 24)))


def pointwise(img, plan):
    """the op's per-pixel part on a whole int64 [H,W,3] image (the device applies it to each tap it reads: same values)"""
    H, W = img.shape[:2]
    if plan.op == GRAYSCALE:
        g = (4899 * img[..., 0] + 9617 * img[..., 1] + 1868 * img[..., 2] + 8192) >> 14
        return np.stack([g, g, g], axis=-1)
    if plan.op == CONTRAST:
        return contrast_table(plan.alpha)[img]
    if plan.op == LAPLACE:
        i = np.arange(H * W * 3, dtype=np.uint64).reshape(H, W, 3)
        n = laplace(plan.b)[(splitmix(plan.seed, i) >> U64(52)).astype(np.int64)]
        return np.clip(img + n, 0, 255)
    if plan.op == MASKING:
        return np.where(masking_cells(H, W, plan.seed)[..., None], 0, img)
    return img


def pad_square(a, value=0):
    h, w = a.shape[:2]
    S = max(h, w)
    out = np.full((S, S) + a.shape[2:], value, a.dtype)
    py, px = (S - h) // 2, (S - w) // 2
    out[py:py + h, px:px + w] = a
    return out


def resize_cubic(sq, T):
    S = sq.shape[0]
    idx, coef = cubic(S, T)
    taps = np.clip(idx[:, None] + np.arange(-1, 3)[None, :], 0, S - 1)           # [T,4]
    rows = sq[taps]                                                                # [T,4,S,3]
    cols = rows[:, :, taps]                                                        # [T,4,T,4,3]: (oy, r, ox, c, ch)
    inner = (cols * coef[None, None, :, :, None]).sum(axis=3)                      # [T,4,T,3]
    acc = (inner * coef[:, :, None, None]).sum(axis=1)                             # [T,T,3]
    return np.clip((acc + (1 << 21)) >> 22, 0, 255)


def resize_nearest(sq, T):
    S = sq.shape[0]
    src = (np.arange(T, dtype=np.int64) * S) // T
    return sq[src][:, src]


def augment(img, label, plan, T=256, label_lut=None, label_fill=0):
    """-> (uint8 [T,T,3], int64 [T,T])"""
    im = img[..., :3].astype(np.int64)
    lab = label_classes(label)
    if plan.op == ROTATION:
        im, lab = rotate(img, label, plan.theta, label_fill)
    elif plan.op == BLUR:
        im = blur(img)
    else:
        im = pointwise(im, plan)
        if plan.op == MASKING:
            lab = np.where(masking_cells(*im.shape[:2], plan.seed), 0, lab)
    wy, wx, wh, ww = plan.window
    im, lab = im[wy:wy + wh, wx:wx + ww], lab[wy:wy + wh, wx:wx + ww]
    out = resize_cubic(pad_square(im), T).astype(np.uint8)
    lo = resize_nearest(pad_square(lab), T)
    if label_lut is not None:
        lo = np.asarray(label_lut).astype(np.int64)[lo]
    return out, lo


def to_float(u8_hwc):
    """uint8 [T,T,3] -> float32 [3,T,T] = u8 / 255.0f"""
    return (u8_hwc.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)


# ---------------------------------------------------------------------------------------------- merge (cell 17)
def pil_nearest_index(n_in, n_out):
    """PIL NEAREST n_in -> n_out: truncation of the running float64 sum a/2, a/2 + a, ... (a = n_in / n_out)"""
    a = n_in / n_out
    xo = a * 0.5
    out = []
    for _ in range(n_out):
        out.append(int(xo) if int(xo) < n_in else -1)
        xo += a
    return np.array(out, dtype=np.int64)


def gather_nearest(a, fh, fw):
    ys, xs = pil_nearest_index(a.shape[0], fh), pil_nearest_index(a.shape[1], fw)
    out = a[np.clip(ys, 0, None)][:, np.clip(xs, 0, None)].copy()
    out[ys < 0] = 0
    out[:, xs < 0] = 0
    return out


def paste(canvas, a, y, x):
    """PIL paste: clipped to the canvas"""
    H, W = canvas.shape[:2]
    h, w = a.shape[:2]
    y0, x0, y1, x1 = max(y, 0), max(x, 0), min(y + h, H), min(x + w, W)
    if y1 > y0 and x1 > x0:
        canvas[y0:y1, x0:x1] = a[y0 - y:y1 - y, x0 - x:x1 - x]


def merge_rgb(a1, a2, T=256):
    """uint8 [h,w,3] x 2 -> uint8 [T,T,3]"""
    (h1, w1), (h2, w2) = a1.shape[:2], a2.shape[:2]
    portrait = h1 > w1
    if portrait != (h2 > w2):
        raise ValueError("mismatched orientations")
    scale = T / (w1 + w2) if portrait else T / (h1 + h2)
    sw1, sh1 = max(1, math.ceil(w1 * scale)), max(1, math.ceil(h1 * scale))
    sw2, sh2 = max(1, math.ceil(w2 * scale)), max(1, math.ceil(h2 * scale))
    fw1, fh1, fw2, fh2 = sw1, sh1, sw2, sh2
    if portrait:
        diff = (sw1 + sw2) - T
        if diff > 0:
            fw1 -= diff if sw1 >= sw2 else 0
            fw2 -= diff if sw2 > sw1 else 0
    else:
        diff = (sh1 + sh2) - T
        if diff > 0:
            fh1 -= diff if sh1 >= sh2 else 0
            fh2 -= diff if sh2 > sh1 else 0
    fw1, fh1, fw2, fh2 = max(1, fw1), max(1, fh1), max(1, fw2), max(1, fh2)
    r1, r2 = gather_nearest(a1, fh1, fw1), gather_nearest(a2, fh2, fw2)
    if portrait:
        strip = np.zeros((max(fh1, fh2), T, 3), np.uint8)
        paste(strip, r1, 0, 0)
        paste(strip, r2, 0, fw1)
    else:
        strip = np.zeros((T, max(fw1, fw2), 3), np.uint8)
        paste(strip, r1, 0, 0)
        paste(strip, r2, fh1, 0)
    canvas = np.zeros((T, T, 3), np.uint8)
    paste(canvas, strip, (T - strip.shape[0]) // 2, (T - strip.shape[1]) // 2)
    return canvas


def as_rgb(a):
    a = a[..., :3] if a.ndim == 3 else np.stack([a, a, a], axis=-1)
    return np.ascontiguousarray(a.astype(np.uint8))


def merge(img1, lab1, img2, lab2, T=256, label_lut=None):
    """-> (uint8 [T,T,3], int64 [T,T])"""
    lo = rgb_to_classes(merge_rgb(as_rgb(lab1), as_rgb(lab2), T))
    if label_lut is not None:
        lo = np.asarray(label_lut).astype(np.int64)[lo]
    return merge_rgb(as_rgb(img1), as_rgb(img2), T), lo


# ---------------------------------------------------------------------------------------------- class weights
def label_hist(labels, C, ignore=None):
    """utils.py:168-173: drop the ignore value first, then clamp to 0..C-1, then count -> int64 [C]"""
    v = np.asarray(labels).astype(np.int64).ravel()
    if ignore is not None:
        v = v[v != ignore]
    return np.bincount(np.clip(v, 0, C - 1), minlength=C)


def rgb_classes(rgb):
    """uint8 [n,3] -> uint8 [n] (segk_rgb_label_to_classes)"""
    return rgb_to_classes(np.asarray(rgb)).astype(np.uint8)


def class_weights(labels, C, ignore_index=None, unimportant=None, normalize_target_sum=-1.0):
    """utils.py:166-198 -> (counts int64 [C], weights float32 [C])"""
    counts = np.zeros(C, np.int64)
    for lab in labels:
        counts += label_hist(lab, C, ignore_index)
    freq = counts.astype(np.float64) / float(counts.sum())
    w = 1.0 / (freq + 1e-6)
    if unimportant:
        for i in unimportant:
            w[i] = w.min()
    target = normalize_target_sum if normalize_target_sum > 0 else float(C)
    tot = 0.0
    for v in w:                                     # a plain left-to-right float64 sum
        tot += float(v)
    return counts, (w / tot * target).astype(np.float32)


# ---- class counts: launch arithmetic and the case table of tests/test_gpu_label_count_matrix.py ------------------------------
HIST_MAX_BLOCKS, HIST_PER_BLOCK, HIST_PER_PASS = 1024, 4096, 1024


def hist_launch(n):
    """label_hist_kernel -> (workgroups, passes of the longest-running workgroup's loop).  A workgroup takes 1024 labels per pass
    and the grid is sized for four passes, up to 1024 workgroups; beyond 1024 * 4096 labels a fifth pass begins."""
    blocks = min((n + HIST_PER_BLOCK - 1) // HIST_PER_BLOCK, HIST_MAX_BLOCKS)
    return blocks, (n + blocks * HIST_PER_PASS - 1) // (blocks * HIST_PER_PASS)


HIST_N = [1, 3, 4, 5, 1023, 1024, 1025, 4096, 4097, 1024 * 4096, 1024 * 4096 + 1, 1024 * 4096 + 4097]
HIST_CLASSES = [1, 2, 4, 21, 256]
HIST_BAD = [-5, None, 2 ** 40, -2 ** 63]            # None: the class count C itself, one past the last class


def hist_cases():
    """(elem_bytes, n, C, ignore | None): C and the ignore mode walk the n values with strides of their own -- none, a value inside
    0..C-1, 255 with C = 4, and -100 (int64 only; uint8 takes the inside value again)"""
    out = []
    for d, eb in enumerate((1, 8)):
        for i, n in enumerate(HIST_N):
            C = HIST_CLASSES[(i + 2 * d) % 5]
            mode = (i + i // 4 + d) % 4
            if mode == 2:
                C, ign = 4, 255
            elif mode == 3 and eb == 8:
                ign = -100
            else:
                ign = None if mode == 0 else (i + d) % C
            out.append((eb, n, C, ign))
    return out


def hist_labels(eb, n_max):
    """the master array every case is a prefix of: values 0..255; int64 also holds -100 and the values of HIST_BAD at strides of
    their own (the class count stands in as 300, above every C)"""
    v = np.minimum((u01(n_max, 77 + eb).astype(np.float64) * 256).astype(np.int64), 255)
    if eb == 1:
        return v.astype(np.uint8)
    v[2::29] = -100
    for i, bad in enumerate(HIST_BAD):
        v[1 + i::31 + 2 * i] = 300 if bad is None else bad
    return v


def hist_case_labels(master, n, C):
    """the first n labels of the master array with the stand-in 300 replaced by C"""
    v = master[:n]
    return v if v.dtype == np.uint8 else np.where(v == 300, C, v)


RGB_N =[1, 255, 256, 257, 65537]
RGB_COLOURS = [(0, 0, 0), (255, 255, 255), (128, 0, 0), (0, 128, 0),                       # the four named colours
               (0, 0, 128), (0, 128, 128), (255, 255, 254),                                # near misses
               (1, 0, 0), (0, 1, 0), (0, 0, 1), (254, 255, 255), (255, 254, 255), (129, 0, 0), (127, 0, 0), (128, 1, 0),
               (128, 0, 1), (0, 129, 0), (0, 127, 0), (1, 128, 0), (0, 128, 1), (128, 128, 0), (128, 128, 128)]


def rgb_pixels(n):
    """uint8 [n,3]: the colours above in a fixed shuffle"""
    idx = np.minimum((u01(n, 99).astype(np.float64) * len(RGB_COLOURS)).astype(np.int64), len(RGB_COLOURS) - 1)
    idx[:min(n, len(RGB_COLOURS))] = np.arange(min(n, len(RGB_COLOURS)))
    return np.array(RGB_COLOURS, dtype=np.uint8)[idx]
