"""NumPy references, inputs and derived bounds for the eval resize / crop / fused-mask kernels (the second half of
csrc/resize.hip): what tests/test_gpu_resize_matrix.py compares the device with.  Host-only; nothing here is taken from what the
kernels return.  The contract is include/segk.h and the comment block above `struct AA` in resize.hip; the arithmetic restated is
that of aa_taps, aa_w, src_index, nearest_index, bilerp and resize_sample.  U = 2^-24 is the unit roundoff of fp32.  The library
is built with -ffp-contract=off and fp32 division is correctly rounded, so every fp32 expression below is restated in
np.float32 with one operation per rounding, in the kernel's order: indices, tap windows, lambdas and weights are integers and
bit-exact fp32 values with no tolerance.

  nearest (mode 1)     index = min(floor(f32(o) * scale), in - 1), scale = f32(in) / f32(out): an exact gather (int64 images
                       never pass through a float).
  bilinear (mode 2,    src_index: s = max(scale * (o + 0.5) - 0.5, 0), i0 = min(int(s), in - 1), i1 = min(i0 + 1, in - 1),
  crop_resize,         lambda = s - i0; the blend is bilerp's expression (1 - ly) * ((1 - lx) * a + lx * b) + ly * (...), which has
  predict_mask)        no fused operation: the whole result is restated in fp32 and the device must equal it.  The float64 blend of
                       the same fp32 lambdas bounds the restatement by 12 U sum |w| |x| (the form of
                       vit_reference.bilinear_fwd_bound): the host test holds the restatement to it, which shows it is an
                       interpolation and not a copy of a bug.
  anti-aliased         per axis: support = max(scale, 1), inv = 1 / support, center = scale * (o + 0.5),
  (mode 0)             lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), in),
                       x = |((j + lo) - center + 0.5) * inv|, w = 1 - x where x < 1 else 0, total = the sequential fp32 sum in tap
                       order, weight = w / total (w where total == 0).  float64 reference: Wy x Wx^T with these exact weights.
                       The kernel runs row = fmaf(wx, t, row) over the nx taps and v = fmaf(wy, row, v) over the ny rows: nx + ny
                       roundings along the longest path, 2 spare:   bound = (nx + ny + 2) U sum_y sum_x |wy| |wx| |t|
                       with nx, ny the pixel's own tap counts.  Derived, not fitted.  aa_emulate_f32 runs the chain with fmaf
                       emulated as a float64 multiply-add rounded to fp32; that can double-round (the float64 sum is itself
                       rounded before the rounding to fp32), which is why the device is held to the bound and not to the
                       emulation -- except on impulse inputs (a single 1.0 in a zero image), where the chain collapses to
                       fl32(wy * wx): a 48-bit product rounded once, exact in the emulation, and the device must equal it.  That
                       pins every tap position and every weight, clipped and renormalised edge taps included.
  u8 images            every tap is np.float32(u8) / np.float32(255); everything else as above on the converted image.
  flips                the reference flips the source image and calls the unflipped reference (segk.h: the flipped image's pixel
                       (y, x) is the image's (H - 1 - y, W - 1 - x)).
  predict_mask         mask = argmax over the classes of the fp32 restatement (first maximum, NaN maximal), color =
                       palette[mask], counts = bincount(mask), M[pred * 8 + label] over the labels inside [0, C): all exact.

Mutants (`mut`): the single errors tests/test_resize_cases_host.py shows the case list to catch -- MUTANTS below."""
import zlib

import numpy as np

f32 = np.float32
U = 2.0 ** -24
MAX_CLASSES = 8

MUTANTS = ("lo+1", "no_half", "no_renorm", "support_unclamped", "i1_unclamped", "nearest_round", "swap_pad", "swap_flip", "stale_row")


# ---- coordinates and weights -----------------------------------------------------------------------------------------------
def scale_f32(n_in, n_out):
    return f32(n_in) / f32(n_out)


def nearest_index(n_out, n_in, mut=None):
    v = np.arange(n_out, dtype=f32) * scale_f32(n_in, n_out)
    s = np.floor(v + f32(0.5)) if mut == "nearest_round" else np.floor(v)
    return np.minimum(s.astype(np.int64), n_in - 1)


def src_index(n_out, n_in, mut=None):
    """src_index of resize.hip for o = 0 .. n_out - 1: (i0, i1 int64, lambda float32)"""
    s = scale_f32(n_in, n_out) * (np.arange(n_out, dtype=f32) + f32(0.5)) - f32(0.5)
    s = np.where(s < 0, f32(0), s).astype(f32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + 1 if mut == "i1_unclamped" else i0 + (i0 < n_in - 1)
    return i0, i1, (s - i0.astype(f32)).astype(f32)


class Axis:
    """one axis of the anti-aliased filter: lo, n [out] and the weights, dense (W [out, in]) and by tap (wp [out, max n])"""

    def __init__(self, n_out, n_in, mut=None):
        scale = scale_f32(n_in, n_out)
        if scale >= 1 or mut == "support_unclamped":
            support, inv = scale, f32(1) / scale
        else:
            support, inv = f32(1), f32(1)
        self.lo, self.n, rows = np.zeros(n_out, dtype=np.int64), np.zeros(n_out, dtype=np.int64), []
        for o in range(n_out):
            center = scale * f32(o) if mut == "no_half" else scale * (f32(o) + f32(0.5))
            lo = int(center - support + f32(0.5)) + (1 if mut == "lo+1" else 0)
            lo = max(lo, 0)
            hi = min(int(center + support + f32(0.5)), n_in)
            n = max(hi - lo, 0)
            x = np.abs(((np.arange(n) + lo).astype(f32) - center + f32(0.5)) * inv)
            w = np.where(x < 1, f32(1) - x, f32(0)).astype(f32)
            total = np.add.accumulate(w, dtype=f32)[-1] if n else f32(0)       # sequential, in tap order
            if total != 0 and mut != "no_renorm":
                w = (w / total).astype(f32)
            self.lo[o], self.n[o] = lo, n
            rows.append(w)
        self.W = np.zeros((n_out, n_in), dtype=f32)
        self.wp = np.zeros((n_out, max(1, int(self.n.max()))), dtype=f32)
        for o, w in enumerate(rows):
            self.W[o, self.lo[o]:self.lo[o] + len(w)] = w
            self.wp[o, :len(w)] = w


def bilinear_matrix(n_out, n_in, mut=None):
    """[out, in (+ 1 for the unclamped mutant)] float64: (1 - lambda) at i0 plus lambda at i1, lambda the fp32 value"""
    i0, i1, lam = src_index(n_out, n_in, mut)
    W = np.zeros((n_out, n_in + (mut == "i1_unclamped")), dtype=np.float64)
    r = np.arange(n_out)
    np.add.at(W, (r, i0), 1.0 - lam.astype(np.float64))
    np.add.at(W, (r, i1), lam.astype(np.float64))
    return W


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def aa_emulate_f32(x, ay, ax):
    """the fmaf chains of resize_sample's anti-aliased branch on x [C, H, W] fp32 (see the docstring on double rounding).  Taps
    past a pixel's own count carry weight 0 and leave the accumulator as it is, as in the kernel, which never reads them."""
    C, H, W = x.shape
    row = np.zeros((C, H, len(ax.n)), dtype=f32)
    for j in range(ax.wp.shape[1]):
        row = _fma32(ax.wp[None, None, :, j], x[:, :, np.minimum(ax.lo + j, W - 1)], row)
    v = np.zeros((C, len(ay.n), len(ax.n)), dtype=f32)
    for j in range(ay.wp.shape[1]):
        v = _fma32(ay.wp[None, :, j, None], row[:, np.minimum(ay.lo + j, H - 1), :], v)
    return v


# ---- one resize ------------------------------------------------------------------------------------------------------------
def _padded(x, mut):
    return np.pad(x, ((0, 0), (0, 1), (0, 1))) if mut == "i1_unclamped" else x       # what the unclamped tap reads: not the edge


def resize_f32(x, nh, nw, mode, mut=None):
    """x [C, H, W] -> [C, nh, nw] in the dtype of x: the kernel's arithmetic in fp32 (mode 0: the emulated chain, exact on
    impulse inputs only; modes 1 and 2: what the device must return bit for bit)"""
    C, H, W = x.shape
    if mode == 1:
        return x[:, nearest_index(nh, H, mut)[:, None], nearest_index(nw, W, mut)[None, :]]
    x = x.astype(f32)
    if mode == 0:
        return aa_emulate_f32(x, Axis(nh, H, mut), Axis(nw, W, mut))
    y0, y1, ly = src_index(nh, H, mut)
    x0, x1, lx = src_index(nw, W, mut)
    x = _padded(x, mut)
    ly, lx, one = ly[:, None], lx[None, :], f32(1)
    a, b = x[:, y0[:, None], x0[None, :]], x[:, y0[:, None], x1[None, :]]
    d, e = x[:, y1[:, None], x0[None, :]], x[:, y1[:, None], x1[None, :]]
    with np.errstate(invalid="ignore"):
        return ((one - ly) * ((one - lx) * a + lx * b) + ly * ((one - lx) * d + lx * e)).astype(f32)


def resize_f64(x, nh, nw, mode, mut=None):
    """-> (float64 reference [C, nh, nw], bound): the exact fp32 weights applied in float64"""
    C, H, W = x.shape
    xd = x.astype(np.float64)
    if mode == 1:
        r = xd[:, nearest_index(nh, H, mut)[:, None], nearest_index(nw, W, mut)[None, :]]
        return r, np.zeros_like(r)
    if mode == 0:
        ay, ax = Axis(nh, H, mut), Axis(nw, W, mut)
        Wy, Wx = ay.W.astype(np.float64), ax.W.astype(np.float64)
        k = (ay.n[:, None] + ax.n[None, :] + 2).astype(np.float64)
    else:
        Wy, Wx = bilinear_matrix(nh, H, mut), bilinear_matrix(nw, W, mut)
        xd = _padded(xd, mut)
        k = 12.0
    ref = np.einsum("oi,cij,pj->cop", Wy, xd, Wx, optimize=True)
    mag = np.einsum("oi,cij,pj->cop", np.abs(Wy), np.abs(xd), np.abs(Wx), optimize=True)
    return ref, k * U * mag


def flip_image(img, flip, axes=(-2, -1)):
    """the flipped image: bit 0 reverses x (axes[1]), bit 1 reverses y (axes[0])"""
    out = np.asarray(img)
    if flip & 2:
        out = np.flip(out, axes[0])
    if flip & 1:
        out = np.flip(out, axes[1])
    return np.ascontiguousarray(out)


def _place(r, T, pt, pl):
    """[C, nh, nw] -> zero slot [C, T, T] with r at (pt, pl); a mutant's window is cut at the slot's edge"""
    C, nh, nw = r.shape
    out = np.zeros((C, T, T), dtype=r.dtype)
    ys, xs = pt + np.arange(nh), pl + np.arange(nw)
    ky, kx = ys < T, xs < T
    out[:, ys[ky][:, None], xs[kx][None, :]] = r[:, ky][:, :, kx]
    return out


def _mut_geometry(c, flip, mut):
    pt, pl = (c.pl, c.pt) if mut == "swap_pad" else (c.pt, c.pl)
    if mut == "swap_flip":
        flip = ((flip & 1) << 1) | ((flip >> 1) & 1)
    return pt, pl, flip


def resize_pad_f32(img, c, mode, flip=0, mut=None):
    """segk_resize_pad[_flip] of img [C, H, W] (fp32, or int64 with mode 1) -> the slot [C, T, T] in fp32 arithmetic"""
    pt, pl, flip = _mut_geometry(c, flip, mut)
    return _place(resize_f32(flip_image(img, flip), c.nh, c.nw, mode, mut), c.T, pt, pl)


def resize_pad_f64(img, c, mode, flip=0, mut=None):
    """-> (float64 slot, bound slot): zero, and bound zero, outside the window"""
    pt, pl, flip = _mut_geometry(c, flip, mut)
    ref, bound = resize_f64(flip_image(img, flip), c.nh, c.nw, mode, mut)
    return _place(ref, c.T, pt, pl), _place(bound, c.T, pt, pl)


def u8_to_float(img_hwc):
    """[H, W, Cin] uint8 -> [min(Cin, 3), H, W] fp32: (float)u8 / 255.0f, the alpha byte dropped"""
    chw = np.ascontiguousarray(np.transpose(img_hwc[:, :, :3], (2, 0, 1)))
    return (chw.astype(f32) / f32(255)).astype(f32)


# ---- the reverse direction -------------------------------------------------------------------------------------------------
def crop_resize_f32(slot, c, mode, mut=None):
    """segk_crop_resize: slot [C, T, T] -> [C, oh, ow]; mode 0 bilinear (bilerp), 1 nearest"""
    pt, pl, _ = _mut_geometry(c, 0, mut)
    big = np.pad(slot, ((0, 0), (0, c.T), (0, c.T)))                     # a mutant's window may leave the slot
    return resize_f32(big[:, pt:pt + c.nh, pl:pl + c.nw], c.oh, c.ow, 1 if mode == 1 else 2, mut)


def crop_resize_f64(slot, c, mode):
    return resize_f64(slot[:, c.pt:c.pt + c.nh, c.pl:c.pl + c.nw], c.oh, c.ow, 1 if mode == 1 else 2)


def argmax_first_nan_max(z):
    """first maximum over axis 0, NaN maximal (torch.argmax; segk_predict_mask)"""
    best, bv = np.zeros(z.shape[1:], dtype=np.int64), z[0].copy()
    for k in range(1, len(z)):
        take = (z[k] > bv) | (np.isnan(z[k]) & ~np.isnan(bv))
        bv = np.where(take, z[k], bv)
        best = np.where(take, k, best)
    return best


def predict_mask_ref(slot, c, mode, palette=None, labels=None, mut=None):
    """-> (mask uint8 [oh, ow], color uint8 [oh, ow, 3] or None, counts int64 [8], M int64 [8, 8] or None)"""
    z = crop_resize_f32(slot, c, mode, mut)
    if mut == "stale_row":            # a thread's four flat pixels all take the row taps of its first one
        p = np.arange(c.oh * c.ow)
        z = z[:, (p - p % 4) // c.ow, p % c.ow].reshape(z.shape)
    mask = argmax_first_nan_max(z)
    counts = np.bincount(mask.reshape(-1), minlength=MAX_CLASSES).astype(np.int64)
    color = None if palette is None else np.asarray(palette, dtype=np.uint8).reshape(-1, 3)[mask]
    M = None
    if labels is not None:
        lab, C = np.asarray(labels).reshape(-1), slot.shape[0]
        keep = (lab >= 0) & (lab < C)
        M = np.bincount(mask.reshape(-1)[keep] * MAX_CLASSES + lab[keep], minlength=MAX_CLASSES ** 2).reshape(MAX_CLASSES, MAX_CLASSES)
    return mask.astype(np.uint8), color, counts, M


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def dense_image(design, C, H, W, key=()):
    """[C, H, W] fp32 of a dense design: uniform [0, 1], uniform [-3, 3], one constant per channel, or a plane whose values
    (0.25 y + 0.5 x + c, below 2^11 with two fraction bits) are exact in fp32"""
    g = _rng("image", design, C, H, W, key)
    if design == "dense01":
        return g.random((C, H, W), dtype=f32)
    if design == "signed":
        return (g.random((C, H, W), dtype=f32) * f32(6) - f32(3)).astype(f32)
    if design == "constant":
        return np.broadcast_to((f32(0.3) + np.arange(C, dtype=f32))[:, None, None], (C, H, W)).copy()
    if design == "ramp":
        y, x, ch = np.arange(H, dtype=f32)[None, :, None], np.arange(W, dtype=f32)[None, None, :], np.arange(C, dtype=f32)[:, None, None]
        return (f32(0.25) * y + f32(0.5) * x + ch).astype(f32)
    raise ValueError(design)


def edge_taps(c):
    """the last tap the first output row / column reads under mode 0, and the first tap of the last one"""
    ay, ax = Axis(c.nh, c.H), Axis(c.nw, c.W)
    return (int(ay.lo[0] + ay.n[0] - 1), int(ax.lo[0] + ax.n[0] - 1)), (int(ay.lo[-1]), int(ax.lo[-1]))


def impulse_positions(c):
    """the four corners, an interior pixel, and the two edge taps"""
    pos = [(0, 0), (0, c.W - 1), (c.H - 1, 0), (c.H - 1, c.W - 1), (c.H // 2, c.W // 2), *edge_taps(c)]
    return sorted(set(pos))


def impulse_image(c):
    """[P, H, W] fp32: channel k is zero but for a single 1.0 at the k-th impulse position"""
    pos = impulse_positions(c)
    img = np.zeros((len(pos), c.H, c.W), dtype=f32)
    for k, (y, x) in enumerate(pos):
        img[k, y, x] = 1
    return img


def u8_image(c, cin, alpha_key=0):
    """[H, W, cin] uint8, random; the alpha byte of a 4-channel image follows alpha_key alone"""
    img = _rng("u8", c.H, c.W, cin).integers(0, 256, (c.H, c.W, cin), dtype=np.uint8)
    if cin == 4:
        img[:, :, 3] = _rng("alpha", alpha_key).integers(0, 256, (c.H, c.W), dtype=np.uint8)
    return img


def u8_impulse_image(c, cin):
    """[H, W, cin] uint8: one 255 (1.0 after the conversion) per colour channel, zero elsewhere.  An 8-bit image has at most
    three colour channels, so the positions are chosen, not all taken: the two edge taps first (the last tap the first output
    reads, the first tap of the last one: what a shifted or unnormalised edge window moves), then the corners; a 1-channel
    image carries the first edge tap alone.  The other impulse positions reach the u8 entries through the equality with the
    float route, which the GPU test asserts on the device."""
    pos = list(dict.fromkeys([*edge_taps(c), *impulse_positions(c)]))
    img = np.zeros((c.H, c.W, cin), dtype=np.uint8)
    for k, (y, x) in enumerate(pos[:min(cin, 3)]):
        img[y, x, k] = 255
    if cin == 4:
        img[:, :, 3] = 200
    return img


def label_image(C, H, W, values):
    """[C, H, W] int64 drawn from `values`, every value present when the image has room"""
    v = np.asarray(values, dtype=np.int64)
    img = v[_rng("labels", C, H, W).integers(0, len(v), (C, H, W))]
    flat = img.reshape(-1)
    flat[:min(len(v), len(flat))] = v[:len(flat)]
    return img


def logits_slot(C, T, key=()):
    """[C, T, T] fp32 uniform [-3, 3] over the WHOLE slot: a wrong window origin reads other numbers, not zeros"""
    return (_rng("slot", C, T, key).random((C, T, T), dtype=f32) * f32(6) - f32(3)).astype(f32)


def eval_labels(C, oh, ow):
    """[oh, ow] int64 in [0, C) with ignore values outside it: -1, C, 255 and 2^40 + 1"""
    g = _rng("eval-labels", C, oh, ow)
    lab = g.integers(0, C, (oh, ow)).astype(np.int64)
    pick = g.integers(0, 9, (oh, ow))
    for n, v in enumerate((-1, C, 255, 2 ** 40 + 1)):
        lab[pick == n] = v
    return lab


PALETTE = np.array([[0, 0, 0], [255, 1, 2], [3, 254, 4], [5, 6, 253], [250, 251, 7], [8, 120, 121], [122, 9, 123], [64, 65, 66]], dtype=np.uint8)


def coord_ulp(*sizes):
    """one fp32 ulp of the largest source coordinate of a geometry (the source sides bound the coordinates)"""
    return float(np.spacing(f32(max(sizes))))
