"""Training augmentation and dataset preparation on the device -- the rest of the reference's utils/augmentation.ipynb (the
eight imgaug augmenters, each followed by "pad to square, resize to 256"; the pair merge of cell 17;
convert_rgb_label_to_classes) and utils/utils.py:117-198 calculate_class_weights.

    aug = Augmenter(target_size=256, label_lut=TARGET_REMAP, seed=0)
    X, y = aug(images, labels)                                # lists of uint8 [H,W,3|4] / [H,W] or [H,W,3] device tensors
    for X, y in AugmentedBatches(loader, aug): ...            # what train_loop / start iterate over
    X, y = merge_pairs(images_a, labels_a, images_b, labels_b)
    w = class_weights(loader, 4, unimportant_class_indices=[0])

The reference builds its `astrain/` set offline, one image at a time on the CPU.  Here a batch of differently sized images
costs at most two launches: segk_aug_prefilter (rotation, blur) and segk_aug_resample (window, pointwise op, pad, resize),
driven by one descriptor table that is uploaded once per batch from pinned memory together with the tables it points into.
Every value that decides a result comes from a table this module builds on the host (cubic coefficients, contrast LUT, Laplace
inverse CDF, Q16 rotation matrix, PIL-NEAREST index tables); the device combines them with integer arithmetic only, so the
outputs are bit-stable and equal the NumPy restatement of tests/augment_reference.py.  The arithmetic is DEFINED in DESIGN.md
section 3: it is modelled on what cv2 does for uint8, parity with imgaug itself is not pinned.  There is no CPU path."""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from . import _lib, ops

RESIZE, CENTER_CROP, RANDOM_CROP, ROTATION, MASKING, GRAYSCALE, LAPLACE, BLUR, CONTRAST = range(9)     # SEGK_AUG_*
OP_NAMES = ("resize", "center_crop", "random_crop", "rotation", "masking", "grayscale", "laplace", "blur", "contrast")
ALL_OPS = (CENTER_CROP, RANDOM_CROP, ROTATION, MASKING, GRAYSCALE, LAPLACE, BLUR, CONTRAST)           # the eight augmenters
MAX_SIDE = 8192
LAPLACE_ENTRIES = 4096

# utils/dataset.py target_remap: the ignore value 255 becomes class 3
TARGET_REMAP = np.arange(256, dtype=np.uint8)
TARGET_REMAP[255] = 3
TARGET_REMAP.setflags(write=False)

# segk_aug_desc / segk_merge_desc of include/segk.h
DESC = np.dtype([("img", "<u8"), ("lab", "<u8"), ("a_img", "<u8"), ("a_lab", "<u8"), ("A", "<i8", (6,)), ("seed", "<u8"),
                 ("H", "<i4"), ("W", "<i4"), ("img_c", "<i4"), ("lab_c", "<i4"), ("Ha", "<i4"), ("Wa", "<i4"), ("op", "<i4"),
                 ("wy", "<i4"), ("wx", "<i4"), ("wh", "<i4"), ("ww", "<i4"), ("tab", "<i4"), ("aux", "<i4"), ("gh", "<i4"),
                 ("gw", "<i4"), ("label_fill", "<i4"), ("pad_", "<i4", (2,))])
MERGE_DESC = np.dtype([("img", "<u8", (2,)), ("lab", "<u8", (2,)), ("H", "<i4", (2,)), ("W", "<i4", (2,)),
                       ("img_c", "<i4", (2,)), ("lab_c", "<i4", (2,))])
assert DESC.itemsize == 160 and MERGE_DESC.itemsize == 64


# ------------------------------------------------------------------------------------------------ host table builders
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@lru_cache(maxsize=512)
def cubic_table(S, T):
    """-> (idx int32 [T], coef int16 [T,4]): the separable cubic resize S -> T (Keys kernel, a = -0.75).  Output i reads the
    taps idx[i] - 1 .. idx[i] + 2 (clamped to [0, S-1] by the reader) at f = (i + 0.5) S / T - 0.5, idx = floor(f).  The
    weights are computed in float64, rounded (half to even) to 11 bits, and the residual goes to the largest tap (the first
    of equals), so every row sums to 2048.  Host only; the arrays are read-only."""
    S, T = int(S), int(T)
    if S < 1 or T < 1:
        raise ValueError(f"cubic_table: sizes {S} -> {T}")
    a = -0.75
    f = (np.arange(T, dtype=np.float64) + 0.5) * S / T - 0.5
    fl = np.floor(f)
    t = f - fl

    def near(x):
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0

    def far(x):
        return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    w = np.stack([far(1.0 + t), near(t), near(1.0 - t), far(2.0 - t)], axis=1)
    q = np.rint(w * 2048.0).astype(np.int64)
    q[np.arange(T), np.argmax(q, axis=1)] += 2048 - q.sum(axis=1)
    return _ro(fl.astype(np.int32), q.astype(np.int16))


@lru_cache(maxsize=512)
def contrast_lut(alpha):
    """uint8 [256]: clip(floor(127 + alpha (v - 127) + 0.5), 0, 255) (LinearContrast)."""
    alpha = float(alpha)
    if not math.isfinite(alpha):
        raise ValueError(f"contrast_lut: alpha {alpha}")
    v = np.arange(256, dtype=np.float64)
    return _ro(np.clip(np.floor(127.0 + alpha * (v - 127.0) + 0.5), 0, 255).astype(np.uint8))


@lru_cache(maxsize=512)
def laplace_table(b):
    """int16 [4096]: the inverse CDF of Laplace(0, b) at u = (k + 1/2) / 4096, rint(-b sgn(u - 1/2) ln(1 - 2 |u - 1/2|))."""
    b = float(b)
    if not (math.isfinite(b) and 0 <= b <= 3000):
        raise ValueError(f"laplace_table: scale {b} (0..3000)")
    u = (np.arange(LAPLACE_ENTRIES, dtype=np.float64) + 0.5) / LAPLACE_ENTRIES
    d = u - 0.5
    return _ro(np.rint(-b * np.sign(d) * np.log(1.0 - 2.0 * np.abs(d))).astype(np.int16))


@lru_cache(maxsize=512)
def rotation_plan(H, W, theta):
    """-> (Ha, Wa, A): rotation by theta degrees (clockwise on the screen) about the image centre with fit_output.  Ha, Wa:
    the output size, floor(|W cos| + |H sin| + 0.5) wide; A: the 2 x 3 inverse map output -> source about the centres
    (size - 1) / 2, as six Q16 integers (rint): SX = A[0] x + A[1] y + A[2], SY = A[3] x + A[4] y + A[5]."""
    H, W, theta = int(H), int(W), float(theta)
    if H < 1 or W < 1 or not math.isfinite(theta):
        raise ValueError(f"rotation_plan: {H} x {W}, theta {theta}")
    th = math.radians(theta)
    c, s = math.cos(th), math.sin(th)
    Wa = max(1, int(math.floor(abs(W * c) + abs(H * s) + 0.5)))
    Ha = max(1, int(math.floor(abs(W * s) + abs(H * c) + 0.5)))
    cxs, cys, cxo, cyo = (W - 1) / 2.0, (H - 1) / 2.0, (Wa - 1) / 2.0, (Ha - 1) / 2.0
    m = [c, s, cxs - c * cxo - s * cyo, -s, c, cys + s * cxo - c * cyo]
    return Ha, Wa, tuple(int(np.rint(v * 65536.0)) for v in m)


def _pil_nearest(n_in, n_out):
    """source index per output index of PIL's NEAREST resize n_in -> n_out: the running float64 sum a/2, a/2 + a, ... with
    a = n_in / n_out, truncated (libImaging's scale-only affine path); -1 where PIL would leave the pixel untouched."""
    a = n_in / n_out
    xo = np.cumsum(np.concatenate(([a * 0.5], np.full(n_out - 1, a))))      # cumsum adds left to right, as the C loop does
    t = xo.astype(np.int64)
    t[t >= n_in] = -1
    return t


@lru_cache(maxsize=1024)
def merge_plan(sizes, T=256):
    """sizes ((h1, w1), (h2, w2)) -> (tables int32 [4,T], (fh1, fw1, fh2, fw2)): cell 17 of utils/augmentation.ipynb statement
    for statement.  tables = source row of image 1 per canvas row, source column of image 1 per canvas column, then the same
    for image 2; -1 where the image does not reach.  Mismatched orientations raise ValueError (the cell prints and skips)."""
    (h1, w1), (h2, w2) = ((int(h), int(w)) for h, w in sizes)
    T = int(T)
    if min(h1, w1, h2, w2) < 1 or max(h1, w1, h2, w2) > MAX_SIDE or not 1 <= T <= 4096:
        raise ValueError(f"merge_plan: sizes {sizes} (sides 1..{MAX_SIDE}), target {T} (1..4096)")
    portrait = h1 > w1
    if portrait != (h2 > w2):
        raise ValueError(f"merge_plan: mismatched orientations ({h1} x {w1} is {'portrait' if portrait else 'landscape'}, "
                         f"{h2} x {w2} is not)")
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
    if portrait:
        cw, ch, off2 = T, max(fh1, fh2), (0, fw1)            # strip size; where image 2 is pasted (y, x)
    else:
        cw, ch, off2 = max(fw1, fw2), T, (fh1, 0)
    py, px = (T - ch) // 2, (T - cw) // 2
    tables = np.full((4, T), -1, dtype=np.int32)
    for k, (n_in, n_out, off, lim, pad) in enumerate(((h1, fh1, 0, ch, py), (w1, fw1, 0, cw, px),
                                                      (h2, fh2, off2[0], ch, py), (w2, fw2, off2[1], cw, px))):
        src = _pil_nearest(n_in, n_out)
        for j in range(n_out):
            sp = off + j                                     # position in the strip (pastes are clipped to it) ...
            cp = sp + pad                                    # ... and on the canvas
            if sp < lim and 0 <= cp < T:
                tables[k, cp] = src[j]
    return _ro(tables), (fh1, fw1, fh2, fw2)


def masking_grid(H, W):
    """(gh, gw) of the CoarseDropout cells: min(side, max(3, floor(0.02 side + 0.5)))."""
    return (min(H, max(3, int(math.floor(0.02 * H + 0.5)))), min(W, max(3, int(math.floor(0.02 * W + 0.5)))))


# ------------------------------------------------------------------------------------------------ plans
@dataclass(frozen=True)
class AugPlan:
    """What one sample gets: drawn by Augmenter.plan on the host, applied by Augmenter.apply on the device."""
    op: int                         # RESIZE .. CONTRAST
    H: int                          # source size
    W: int
    window: tuple                   # (y, x, h, w) of stage B in its input (the rotated image for ROTATION, else the source)
    theta: float = 0.0              # ROTATION: degrees
    alpha: float = 1.0              # CONTRAST
    b: float = 0.0                  # LAPLACE: scale
    seed: int = 0                   # per-image seed of the hash (MASKING, LAPLACE)


def make_plan(op, H, W, y1=0, x1=0, theta=0.0, alpha=1.0, b=0.0, seed=0):
    """An AugPlan with the op's window: the whole stage-B input, the centre square (CENTER_CROP) or the square of side
    int(min(H, W) 2 / 3) at (y1, x1) (RANDOM_CROP)."""
    op, H, W = int(op), int(H), int(W)
    if not 0 <= op < len(OP_NAMES):
        raise ValueError(f"unknown augmentation op {op}")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"image of {H} x {W}: sides 1..{MAX_SIDE}")
    if op == CENTER_CROP:
        s = min(H, W)
        win = ((H - s) // 2, (W - s) // 2, s, s)
    elif op == RANDOM_CROP:
        s = max(1, int(min(H, W) * 2 / 3))
        if not (0 <= y1 <= H - s and 0 <= x1 <= W - s):
            raise ValueError(f"random crop at ({y1}, {x1}) of side {s} leaves the {H} x {W} image")
        win = (int(y1), int(x1), s, s)
    elif op == ROTATION:
        Ha, Wa, _ = rotation_plan(H, W, float(theta))
        win = (0, 0, Ha, Wa)
    else:
        win = (0, 0, H, W)
    return AugPlan(op, H, W, win, float(theta), float(alpha), float(b), int(seed))


def _image_list(images, what):
    if isinstance(images, torch.Tensor):
        if images.ndim < 3:
            raise ValueError(f"{what}: a batch tensor is [B,H,W] or [B,H,W,C], got {tuple(images.shape)}")
        images = list(images)
    if not isinstance(images, (list, tuple)) or not images:
        raise TypeError(f"{what}: expected a non-empty list of tensors")
    return list(images)


def _check_image(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise TypeError(f"{what}: images are uint8, got {t.dtype}")
    if t.ndim == 3 and t.shape[0] in (3, 4) and t.shape[2] not in (3, 4):       # CHW, as a file decoder returns it
        t = t.permute(1, 2, 0)
    if t.ndim != 3 or t.shape[2] not in (3, 4):
        raise ValueError(f"{what}: expected uint8 [H,W,3|4], got {tuple(t.shape)}")
    if not (1 <= t.shape[0] <= MAX_SIDE and 1 <= t.shape[1] <= MAX_SIDE):
        raise ValueError(f"{what}: image of {t.shape[0]} x {t.shape[1]}: sides 1..{MAX_SIDE}")
    return t


def _check_label(t, H, W, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise TypeError(f"{what}: labels are uint8 class ids, trimap values or colours, got {t.dtype}")
    if t.ndim == 3 and t.shape[0] == 1 and t.shape[2] != 3:
        t = t[0]
    if not (t.ndim == 2 or (t.ndim == 3 and t.shape[2] == 3)) or tuple(t.shape[:2]) != (H, W):
        raise ValueError(f"{what}: expected uint8 [{H},{W}] or [{H},{W},3], got {tuple(t.shape)}")
    return t


def _lut_array(lut, what="label_lut"):
    if lut is None:
        return None
    t = np.asarray(lut)
    if t.shape != (256,) or t.dtype.kind not in "iu" or t.min() < 0 or t.max() > 255:
        raise ValueError(f"{what}: 256 integer entries in 0..255")
    return np.ascontiguousarray(t.astype(np.uint8))


def _upload(parts, dev):
    """Host arrays -> one pinned buffer -> one copy; returns the device buffer and each part's address in it."""
    offs, n = [], 0
    for a in parts:
        offs.append(n)
        n += (a.nbytes + 15) // 16 * 16
    host = torch.empty(max(n, 16), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    for a, o in zip(parts, offs):
        hv[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = host.to(dev, non_blocking=True)
    return buf, [buf.data_ptr() + o for o in offs]


class Augmenter:
    """(images, labels) -> (X float32 [B,3,T,T] = u8 / 255, y int64 [B,1,T,T]) with one of `ops` applied to every sample.

    ops: the ops to draw from (default: the eight augmenters; RESIZE is the plain "pad to square, resize"); probs: their
    probabilities (default uniform); label_lut: 256-entry table applied to the class map at the output (TARGET_REMAP: 255 ->
    3); label_fill: label value a rotation brings in from outside the image.

    plan(sizes) draws on the host from a NumPy Generator seeded with `seed`, per sample in this order: the op, then its
    parameters (RANDOM_CROP: y1, x1; ROTATION: theta ~ U(45, 315); LAPLACE: b ~ U(25.5, 76.5); CONTRAST: alpha ~ U(0.2, 0.6)),
    then the per-image seed (always).  Two augmenters with one seed draw the same plans; reseed() rewinds.  apply() is a pure
    function of (images, labels, plans): at most one prefilter and one resample launch per batch, no synchronisation."""

    def __init__(self, target_size=256, ops=ALL_OPS, probs=None, label_lut=None, label_fill=0, seed=None):
        self.T = int(target_size)
        if not 1 <= self.T <= 4096:
            raise ValueError(f"target_size must be in 1..4096, got {target_size}")
        self.ops = tuple(int(o) for o in ops)
        if not self.ops or any(not 0 <= o < len(OP_NAMES) for o in self.ops):
            raise ValueError(f"ops: a non-empty sequence of op codes 0..{len(OP_NAMES) - 1}, got {ops}")
        if probs is None:
            self.probs = None
        else:
            p = np.asarray(probs, dtype=np.float64)
            if p.shape != (len(self.ops),) or (p < 0).any() or not p.sum() > 0:
                raise ValueError(f"probs: {len(self.ops)} non-negative numbers with a positive sum")
            self.probs = p / p.sum()
        self._lut = _lut_array(label_lut)
        self.label_fill = int(label_fill)
        if not 0 <= self.label_fill <= 255:
            raise ValueError(f"label_fill must be in 0..255, got {label_fill}")
        self.seed = seed
        self._rng = None
        self._scratch = {}

    def reseed(self, seed=None):
        """Rewind the plan generator to its seed (or to a new one)."""
        if seed is not None:
            self.seed = seed
        self._rng = None

    def _generator(self):
        if self._rng is None:
            if self.seed is None:
                self.seed = int(np.random.SeedSequence().entropy & 0x7FFFFFFF)
            self._rng = np.random.default_rng(int(self.seed))
        return self._rng

    def plan(self, sizes):
        """sizes: (H, W) per sample -> list of AugPlan."""
        rng = self._generator()
        plans = []
        for H, W in sizes:
            H, W = int(H), int(W)
            if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                raise ValueError(f"image of {H} x {W}: sides 1..{MAX_SIDE}")
            op = self.ops[int(rng.choice(len(self.ops), p=self.probs))]
            kw = {}
            if op == RANDOM_CROP:
                s = max(1, int(min(H, W) * 2 / 3))
                kw["y1"] = int(rng.integers(0, H - s + 1))
                kw["x1"] = int(rng.integers(0, W - s + 1))
            elif op == ROTATION:
                kw["theta"] = float(rng.uniform(45.0, 315.0))
            elif op == LAPLACE:
                kw["b"] = float(rng.uniform(25.5, 76.5))
            elif op == CONTRAST:
                kw["alpha"] = float(rng.uniform(0.2, 0.6))
            kw["seed"] = int(rng.integers(0, 1 << 32))
            plans.append(make_plan(op, H, W, **kw))
        return plans

    def _scratch_on(self, dev, nbytes):
        s = self._scratch.get(dev)
        if s is None or s.numel() < nbytes:
            s = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
            self._scratch[dev] = s
        return s

    def apply(self, images, labels, plans, out="float"):
        """-> (X, y) for out="float", (X8 uint8 [B,T,T,3], y) for "uint8", (X, X8, y) for "both".  The sources are not
        modified.  Every argument is checked before the first launch."""
        if out not in ("float", "uint8", "both"):
            raise ValueError(f'out: "float", "uint8" or "both", got {out!r}')
        images, labels = _image_list(images, "images"), _image_list(labels, "labels")
        if not (len(images) == len(labels) == len(plans)):
            raise ValueError(f"{len(images)} images, {len(labels)} labels, {len(plans)} plans")
        B, T = len(images), self.T
        if B > 65535:
            raise ValueError(f"a batch of {B} samples (at most 65535)")
        imgs, labs = [], []
        for k in range(B):
            im = _check_image(images[k], f"images[{k}]")
            lb = _check_label(labels[k], im.shape[0], im.shape[1], f"labels[{k}]")
            p = plans[k]
            if not isinstance(p, AugPlan):
                raise TypeError(f"plans[{k}]: expected an AugPlan, got {type(p).__name__}")
            if (p.H, p.W) != tuple(im.shape[:2]):
                raise ValueError(f"plans[{k}] was drawn for {p.H} x {p.W}, images[{k}] is {im.shape[0]} x {im.shape[1]}")
            if not 0 <= p.op < len(OP_NAMES):
                raise ValueError(f"plans[{k}]: unknown op {p.op}")
            imgs.append(im)
            labs.append(lb)
        dev = imgs[0].device
        for k in range(B):
            ops._require_cuda(imgs[k], f"images[{k}]")
            ops._require_cuda(labs[k], f"labels[{k}]")
            if imgs[k].device != dev or labs[k].device != dev:
                raise ValueError(f"sample {k} is on another device than sample 0")
        imgs = [t.contiguous() for t in imgs]
        labs = [t.contiguous() for t in labs]

        # the tables the descriptors point into, and the scratch of stage A
        desc = np.zeros(B, dtype=DESC)
        cub, con, lap = {}, {}, {}
        a_off, nscratch, max_tiles = [], 0, 0
        for k, p in enumerate(plans):
            d = desc[k]
            H, W = p.H, p.W
            wy, wx, wh, ww = p.window
            Ha, Wa = H, W
            if p.op == ROTATION:
                Ha, Wa, A = rotation_plan(H, W, p.theta)
                d["A"] = A
            hb, wb = (Ha, Wa) if p.op == ROTATION else (H, W)
            if not (0 <= wy and 0 <= wx and wh >= 1 and ww >= 1 and wy + wh <= hb and wx + ww <= wb):
                raise ValueError(f"plans[{k}]: window {p.window} leaves the {hb} x {wb} input of stage B")
            d["img"], d["lab"] = imgs[k].data_ptr(), labs[k].data_ptr()
            d["H"], d["W"], d["img_c"], d["lab_c"] = H, W, imgs[k].shape[2], 3 if labs[k].ndim == 3 else 1
            d["Ha"], d["Wa"], d["op"] = Ha, Wa, p.op
            d["wy"], d["wx"], d["wh"], d["ww"] = wy, wx, wh, ww
            d["tab"] = cub.setdefault(max(wh, ww), len(cub))
            if p.op == CONTRAST:
                d["aux"] = con.setdefault(p.alpha, len(con))
            elif p.op == LAPLACE:
                d["aux"] = lap.setdefault(p.b, len(lap))
            elif p.op == MASKING:
                d["gh"], d["gw"] = masking_grid(H, W)
            d["seed"] = p.seed & 0xFFFFFFFFFFFFFFFF
            d["label_fill"] = self.label_fill
            if p.op in (ROTATION, BLUR):
                img_b = (Ha * Wa * 3 + 255) // 256 * 256
                lab_b = (Ha * Wa + 255) // 256 * 256 if p.op == ROTATION else 0
                a_off.append((k, nscratch, nscratch + img_b if lab_b else -1))
                nscratch += img_b + lab_b
                max_tiles = max(max_tiles, ((Ha + 15) // 16) * ((Wa + 15) // 16))
        if a_off:
            base = self._scratch_on(dev, nscratch).data_ptr()
            for k, oi, ol in a_off:
                desc[k]["a_img"] = base + oi
                desc[k]["a_lab"] = base + ol if ol >= 0 else 0
        parts = [desc, desc[[k for k, _, _ in a_off]] if a_off else desc[:0]]
        tabs = [cubic_table(S, T) for S in cub]                       # dicts keep insertion order: row = value
        parts += [np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])]
        parts.append(np.stack([contrast_lut(a) for a in con]) if con else np.zeros(0, np.uint8))
        parts.append(np.stack([laplace_table(b) for b in lap]) if lap else np.zeros(0, np.int16))
        parts.append(self._lut if self._lut is not None else np.zeros(0, np.uint8))
        X = torch.empty((B, 3, T, T), dtype=torch.float32, device=dev) if out != "uint8" else None
        X8 = torch.empty((B, T, T, 3), dtype=torch.uint8, device=dev) if out != "float" else None
        y = torch.empty((B, 1, T, T), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            buf, (p_desc, p_adesc, p_idx, p_coef, p_con, p_lap, p_lut) = _upload(parts, dev)
            s = ops._stream()
            launches = [("segk_aug_prefilter", (p_adesc, len(a_off), max_tiles, s))] if a_off else []
            launches.append(("segk_aug_resample", (p_desc, B, T, p_idx, p_coef, len(cub), p_con if con else 0, len(con),
                                                   p_lap if lap else 0, len(lap), p_lut if self._lut is not None else 0,
                                                   ops._p(X), ops._p(X8), y.data_ptr(), s)))
            for name, args in launches:
                _lib.call(name, *args)
        # of the last batch (tools/kbench.py replays them; valid while the batch's inputs and outputs are alive)
        self.last_launches, self._last_tables = launches, buf
        return (X, y) if out == "float" else (X8, y) if out == "uint8" else (X, X8, y)

    def __call__(self, images, labels, out="float"):
        images = _image_list(images, "images")
        sizes = [tuple(_check_image(t, f"images[{k}]").shape[:2]) for k, t in enumerate(images)]
        return self.apply(images, labels, self.plan(sizes), out=out)


def merge_pairs(images_a, labels_a, images_b, labels_b, target_size=256, label_lut=None, out="float"):
    """Cell 17 (combine_images_preserve_aspect_ratio) for a batch of pairs in one launch: image a and image b of every pair
    are resized (PIL NEAREST) so that they fill the target side by side (portrait pairs) or one above the other, the strip
    is centred on a black T x T canvas; the labels go the same way and through the colour -> class map (a one-channel label
    counts as grey, as the cell loads every file as RGB).  -> (X, y) as Augmenter.apply.  A pair of a portrait (h > w) and a
    non-portrait image raises ValueError."""
    if out not in ("float", "uint8", "both"):
        raise ValueError(f'out: "float", "uint8" or "both", got {out!r}')
    T = int(target_size)
    lists = [_image_list(v, n) for v, n in ((images_a, "images_a"), (labels_a, "labels_a"), (images_b, "images_b"),
                                            (labels_b, "labels_b"))]
    P = len(lists[0])
    if any(len(v) != P for v in lists):
        raise ValueError(f"merge_pairs: lists of {[len(v) for v in lists]} entries")
    if P > 65535:
        raise ValueError(f"a batch of {P} pairs (at most 65535)")
    lut = _lut_array(label_lut)
    desc = np.zeros(P, dtype=MERGE_DESC)
    tables = np.empty((P, 4, T), dtype=np.int32)
    keep = []
    for k in range(P):
        sizes = []
        for j, (il, ll) in enumerate(((lists[0], lists[1]), (lists[2], lists[3]))):
            im = _check_image(il[k], f"images_{'ab'[j]}[{k}]")
            lb = _check_label(ll[k], im.shape[0], im.shape[1], f"labels_{'ab'[j]}[{k}]")
            keep.append((im, lb))
            sizes.append((int(im.shape[0]), int(im.shape[1])))
        tables[k] = merge_plan(tuple(sizes), T)[0]
    dev = keep[0][0].device
    for im, lb in keep:
        ops._require_cuda(im, "merge_pairs")
        ops._require_cuda(lb, "merge_pairs")
        if im.device != dev or lb.device != dev:
            raise ValueError("merge_pairs: the tensors are on different devices")
    keep = [(im.contiguous(), lb.contiguous()) for im, lb in keep]
    for k in range(P):
        for j in range(2):
            im, lb = keep[2 * k + j]
            d = desc[k]
            d["img"][j], d["lab"][j] = im.data_ptr(), lb.data_ptr()
            d["H"][j], d["W"][j], d["img_c"][j], d["lab_c"][j] = im.shape[0], im.shape[1], im.shape[2], 3 if lb.ndim == 3 else 1
    X = torch.empty((P, 3, T, T), dtype=torch.float32, device=dev) if out != "uint8" else None
    X8 = torch.empty((P, T, T, 3), dtype=torch.uint8, device=dev) if out != "float" else None
    y = torch.empty((P, 1, T, T), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        buf, (p_desc, p_tab, p_lut) = _upload([desc, tables, lut if lut is not None else np.zeros(0, np.uint8)], dev)
        _lib.call("segk_aug_merge", p_desc, p_tab, P, T, p_lut if lut is not None else 0, ops._p(X), ops._p(X8), y.data_ptr(),
                  ops._stream())
    return (X, y) if out == "float" else (X8, y) if out == "uint8" else (X, X8, y)


class AugmentedBatches:
    """Iterable over augmented (X, y) batches made from a loader of (images, labels) batches -- lists of differently sized
    uint8 tensors as a ragged collate function returns them, or batch tensors [B,H,W,C] / [B,H,W] -- and an Augmenter: what
    train_loop and start take as their `dataloader`."""

    def __init__(self, loader, augmenter, device=None):
        self.loader, self.augmenter = loader, augmenter
        self.device = torch.device("cuda" if device is None else device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for X, y in self.loader:
            X = [t.to(self.device, non_blocking=True) for t in X]
            y = [t.to(self.device, non_blocking=True) for t in y]
            yield self.augmenter(X, y)


def convert_rgb_label_to_classes(label):
    """utils/utils.py:201-250 for a device tensor: uint8 [H,W,3] colours -> uint8 [H,W] classes (black or white 0, (128,0,0)
    1, (0,128,0) 2, anything else 255)."""
    if not isinstance(label, torch.Tensor):
        raise TypeError(f"convert_rgb_label_to_classes: expected a tensor, got {type(label).__name__}")
    if label.ndim != 3 or label.shape[2] != 3:
        raise ValueError(f"Input label must be 3-channel RGB (HxWx3), but got shape {tuple(label.shape)}")
    if label.dtype != torch.uint8:
        raise TypeError(f"convert_rgb_label_to_classes: labels are uint8, got {label.dtype}")
    ops._require_cuda(label, "convert_rgb_label_to_classes")
    label = label.contiguous()
    out = torch.empty(label.shape[:2], dtype=torch.uint8, device=label.device)
    if out.numel():
        with torch.cuda.device(label.device):
            _lib.call("segk_rgb_label_to_classes", label.data_ptr(), out.data_ptr(), out.numel(), ops._stream())
    return out


def _label_tensors(source):
    """label_source -> iterator over label tensors: a tensor, a list of tensors, or a loader / dataset of (image, label)"""
    if isinstance(source, torch.Tensor):
        yield source
        return
    for item in source:
        if isinstance(item, torch.Tensor):
            yield item
        elif isinstance(item, (list, tuple)) and len(item) == 2:
            lab = item[1]
            if isinstance(lab, torch.Tensor):
                yield lab
            else:
                yield from lab
        else:
            raise TypeError(f"class_weights: label_source yields {type(item).__name__}; expected label tensors or "
                            "(image, label) pairs")


def class_counts(label_source, num_classes, ignore_index=None, device=None):
    """int64 [num_classes] on the device: utils.py:166-177 over every label of the source (labels equal to ignore_index are
    dropped, the rest is clamped to 0..num_classes-1, so 255 lands in the last class).  Exact; no synchronisation."""
    num_classes = int(num_classes)
    if not 1 <= num_classes <= 256:
        raise ValueError(f"num_classes must be in 1..256, got {num_classes}")
    if ignore_index is not None and int(ignore_index) != ignore_index:
        raise TypeError(f"ignore_index must be an integer or None, got {ignore_index!r}")
    dev = torch.device("cuda" if device is None else device)
    counts = None
    for lab in _label_tensors(label_source):
        if not isinstance(lab, torch.Tensor) or lab.dtype not in (torch.uint8, torch.int64):
            raise TypeError(f"class_weights: labels are uint8 or int64 tensors, got {getattr(lab, 'dtype', type(lab).__name__)}")
        if not lab.is_cuda:
            lab = lab.to(dev, non_blocking=True)
        if counts is None:
            counts = torch.zeros(num_classes, dtype=torch.int64, device=lab.device)
        lab = lab.contiguous()
        if lab.numel():
            with torch.cuda.device(lab.device):
                _lib.call("segk_label_hist", lab.data_ptr(), lab.numel(), lab.element_size(), num_classes,
                          0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index),
                          counts.data_ptr(), ops._stream())
    if counts is None:
        raise ValueError("class_weights: label_source is empty")
    return counts


def weights_from_counts(counts, unimportant_class_indices=None, normalize_target_sum=-1.0):
    """utils.py:183-198 in float64 on the host: inverse frequencies with epsilon 1e-6, the unimportant classes get the smallest
    weight, the sum is normalised to num_classes (or normalize_target_sum) -> float32 [num_classes]."""
    c = torch.as_tensor(counts).detach().cpu().to(torch.float64)
    total = int(c.sum().item())
    if total <= 0:
        raise ValueError("class_weights: no valid pixel was counted")
    weights = 1.0 / (c / total + 1e-6)
    if unimportant_class_indices:
        for idx in unimportant_class_indices:
            weights[idx] = min(weights)
    target = normalize_target_sum if normalize_target_sum > 0 else float(len(c))
    return (weights / weights.sum() * target).float()


def class_weights(label_source, num_classes, ignore_index=None, unimportant_class_indices=None,
                  target_unimportant_weight=1.0, normalize_target_sum=-1.0):
    """calculate_class_weights of the reference (utils/utils.py:117-198), its arguments in its order without `source_type`:
    label_source is a label tensor, a list of them, or a loader / dataset of (image, label) -- uint8 or int64, on the device or
    not.  The counting runs on the device (segk_label_hist), exactly; the dozen float64 operations behind it run on the host.
    Reading the counts is the one synchronisation.  target_unimportant_weight is accepted and ignored, as the reference ignores
    it.  -> float32 [num_classes] on the host."""
    counts = class_counts(label_source, num_classes, ignore_index)
    return weights_from_counts(counts, unimportant_class_indices, normalize_target_sum)
