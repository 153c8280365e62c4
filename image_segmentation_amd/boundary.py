"""Boundary quality on the device: Boundary IoU (Cheng et al. 2021), band ("trimap") IoU and accuracy, the
contour precision / recall / F-measure at pixel tolerances and the 95 % Hausdorff distance -- what a `mask.cpu()` +
`scipy.ndimage` pass per image does on the host, in integers, without leaving the device or synchronising.

    bq = BoundaryQuality(4, ignore_index=3, width=None, tolerances=(1, 2, 3))
    for pred, label in zip(segmenter(images), labels):
        bq.update(pred, label)                       # no sync: adds into one int64 tensor on the device
    bq.compute()                                     # synchronises once: plain data, json.dump-able

    st = boundary_stats(pred.mask, label, 4, width=2)    # BoundaryStats: int64 device tensors

Everything is built on the primitive of 3.21 (the capped distance to the nearest non-void pixel of another class, radius <=
32) and nothing wider: distances past max_distance are reported as capped, never approximated.  The defaults, shape="square"
with image_border=True, are the published Boundary IoU (cv2.erode with a 3 x 3 element, `width` iterations, on a zero-padded
mask).  The kernels are csrc/boundary.hip (segk_boundary_stats, segk_boundary_finish); there is no CPU path."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops

MAX_WIDTH = _lib.BOUNDARY_MAX_WIDTH
BINS = _lib.BOUNDARY_BINS
STAT_WORDS, HIST_WORDS = _lib.BOUNDARY_STAT_WORDS, _lib.BOUNDARY_HIST_WORDS
_OFF = _lib.BOUNDARY_OFFSETS
_C8 = _lib.MAX_CLASSES


# ------------------------------------------------------------------------------------------------ argument checks
def _int_in(v, lo, hi, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def published_width(H, W, ratio=0.02):
    """the published rule: 2 % of the image diagonal, at least one pixel"""
    return max(1, int(round(ratio * math.hypot(H, W))))


def _width_for(width, H, W):
    if width is None:
        w = published_width(H, W)
        if w > MAX_WIDTH:
            raise ValueError(f"width=None gives {w} pixels for a {H} x {W} image, more than {MAX_WIDTH}: pass width= (1..{MAX_WIDTH})")
        return w
    return _int_in(width, 1, MAX_WIDTH, "width")


def _ignore_mask(ignore_index):
    """None, an int or an iterable of byte values -> the bits of the values below 8 (a label >= num_classes is void anyway)"""
    if ignore_index is None:
        return 0
    if isinstance(ignore_index, (bool, str, bytes)):
        raise ValueError(f"ignore_index: None, an integer or an iterable of values in 0..255, got {ignore_index!r}")
    values = [ignore_index] if isinstance(ignore_index, (int, np.integer)) else list(ignore_index)
    mask = 0
    for v in values:
        v = _int_in(v, 0, 255, "ignore_index")
        if v < _C8:
            mask |= 1 << v
    return mask


def _check_settings(num_classes, width, max_distance, ignore_index, shape, image_border):
    C = _int_in(num_classes, 1, _C8, "num_classes")
    if width is not None:
        _int_in(width, 1, MAX_WIDTH, "width")
    R = _int_in(max_distance, 1, MAX_WIDTH, "max_distance")
    if not isinstance(shape, str) or shape not in _lib.MORPH_METRICS:
        raise ValueError(f"shape: one of {tuple(_lib.MORPH_METRICS)}, got {shape!r}")
    if not isinstance(image_border, (bool, np.bool_)):
        raise ValueError(f"image_border: True or False, got {image_border!r}")
    return C, R, _ignore_mask(ignore_index), _lib.MORPH_METRICS[shape], int(bool(image_border))


def _mask_of(pred, what, on_gpu=True):
    mask = pred.mask if hasattr(pred, "mask") and not isinstance(pred, torch.Tensor) else pred
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{what}: a uint8 [H,W] mask or a Prediction, got {type(pred).__name__}")
    if mask.dtype != torch.uint8 or mask.ndim != 2 or mask.shape[0] < 1 or mask.shape[1] < 1:
        raise ValueError(f"{what}: expected a uint8 [H,W] mask, got {mask.dtype} {tuple(mask.shape)}")
    if mask.shape[0] * mask.shape[1] > 1 << 28:
        raise ValueError(f"{what}: {tuple(mask.shape)} has more than 2^28 pixels")
    if on_gpu:
        _on_gpu(mask, what)
    return mask


def _on_gpu(t, what):
    if not t.is_cuda:
        raise ValueError(f"{what}: expected a tensor on the GPU -- there is no CPU path, got one on {t.device}")


def _check_label(label, size, dev):
    if not isinstance(label, torch.Tensor):
        raise ValueError(f"label: expected an integer [H,W] tensor, got {type(label).__name__}")
    if torch.is_floating_point(label) or label.is_complex() or label.dtype == torch.bool:
        raise ValueError(f"label: expected an integer map, got {label.dtype}")
    if tuple(label.shape) not in (size, (1,) + size):
        raise ValueError(f"label: expected a map of {size} like the prediction, got {tuple(label.shape)}")
    _on_gpu(label, "label")
    if label.device != dev:
        raise ValueError(f"label lives on {label.device}, the prediction on {dev}")


def _label_u8(label, size):
    """a checked integer map -> uint8 [H,W]; a value outside 0..255 becomes 255, which is void at every class count"""
    t = label.reshape(size)
    if t.dtype != torch.uint8:
        t = torch.where((t < 0) | (t > 255), 255, t).to(torch.uint8)
    return t.contiguous()


# ------------------------------------------------------------------------------------------------ the statistics
@dataclass
class BoundaryStats:
    """The integer statistics of DESIGN.md 3.23 on the device: `words` (int64 [656], the layout of include/segk.h) and views
    into it.  Rows past num_classes stay zero."""
    words: torch.Tensor         # int64 [STAT_WORDS]
    image_hist: torch.Tensor    # int64 [HIST_WORDS]: scratch of one image, zero between calls
    num_classes: int
    max_distance: int

    @staticmethod
    def zeros(num_classes, max_distance, device):
        buf = torch.zeros((STAT_WORDS + HIST_WORDS,), dtype=torch.int64, device=device)
        return BoundaryStats(buf[:STAT_WORDS], buf[STAT_WORDS:], int(num_classes), int(max_distance))

    def _at(self, name, n, shape):
        return self.words[_OFF[name]:_OFF[name] + n].view(shape)

    band_g = property(lambda s: s._at("band_g", _C8, (_C8,)))            # #{G = c, Dg <= width}
    band_p = property(lambda s: s._at("band_p", _C8, (_C8,)))            # #{P = c, Dp <= width}
    band_i = property(lambda s: s._at("band_i", _C8, (_C8,)))            # #{G = c = P, both within width}
    band_conf = property(lambda s: s._at("conf", _C8 * _C8, (_C8, _C8)))    # [g][p]: #{G = g, P = p, Dg <= width}
    hd_sum = property(lambda s: s._at("hd_sum", _C8, (_C8,)))
    hd_images = property(lambda s: s._at("hd_images", _C8, (_C8,)))
    hd_capped = property(lambda s: s._at("hd_capped", _C8, (_C8,)))
    hist = property(lambda s: s._at("hist", HIST_WORDS, (2, _C8, BINS)))   # [0]: pred -> label, [1]: label -> pred

    def tolist(self):
        """synchronises -> the plain-int keywords of quality_from_boundary_stats"""
        w = self.words.cpu().tolist()
        cut = lambda name, n: w[_OFF[name]:_OFF[name] + n]
        rows = lambda flat, n: [flat[k * n:(k + 1) * n] for k in range(len(flat) // n)]
        hist = rows(cut("hist", HIST_WORDS), BINS)
        return dict(band_g=cut("band_g", _C8), band_p=cut("band_p", _C8), band_i=cut("band_i", _C8),
                    band_conf=rows(cut("conf", _C8 * _C8), _C8), hist=[hist[:_C8], hist[_C8:]], hd_sum=cut("hd_sum", _C8),
                    hd_images=cut("hd_images", _C8), hd_capped=cut("hd_capped", _C8))


def boundary_stats(pred_mask, label, num_classes, width=None, max_distance=32, ignore_index=None, shape="square",
                   image_border=True, out=None):
    """Add the boundary statistics of one image pair to `out` (default: a zeroed BoundaryStats) and return it.

    pred_mask     a uint8 [H,W] mask on the device, or a Prediction (its .mask); a value >= num_classes is void
    label         an integer [H,W] / [1,H,W] map on the same device; a value of ignore_index or outside 0..num_classes-1 is
                  void, in both maps
    width         the band half-width in pixels, 1..32; None: the published max(1, round(0.02 * diagonal)) of this image
    max_distance  the cap of the contour distances, 1..32; farther pixels land in the overflow bin max_distance + 1
    ignore_index  None, an integer or an iterable of byte values
    shape         "square" | "diamond" | "disk": the metric of the band distance; image_border: pixels outside the image
                  differ from every class (the published Boundary IoU: "square", True)

    Two launches, nothing synchronises with the host and the inputs are not modified."""
    C, R, ign, metric, border = _check_settings(num_classes, width, max_distance, ignore_index, shape, image_border)
    mask = _mask_of(pred_mask, "boundary_stats", on_gpu=False)
    H, W = (int(v) for v in mask.shape)
    w = _width_for(width, H, W)                            # a property of the shape: told before the device is looked at
    _on_gpu(mask, "boundary_stats")
    dev = mask.device
    _check_label(label, (H, W), dev)
    if out is None:
        out = BoundaryStats.zeros(C, R, dev)
    elif (not isinstance(out, BoundaryStats) or out.num_classes != C or out.max_distance != R or out.words.device != dev or
          out.words.dtype != torch.int64 or tuple(out.words.shape) != (STAT_WORDS,) or not out.words.is_contiguous() or
          out.image_hist.dtype != torch.int64 or tuple(out.image_hist.shape) != (HIST_WORDS,) or not out.image_hist.is_contiguous()):
        raise ValueError(f"out: a BoundaryStats of {C} classes and max_distance {R} on {dev}")
    with torch.cuda.device(dev):
        mask = mask.contiguous()
        lab = _label_u8(label, (H, W))
        s = ops._stream()
        _lib.call("segk_boundary_stats", mask.data_ptr(), lab.data_ptr(), out.words.data_ptr(), out.image_hist.data_ptr(), C, ign,
                  metric, w, R, border, H, W, s)
        _lib.call("segk_boundary_finish", out.words.data_ptr(), out.image_hist.data_ptr(), C, R, s)
    return out


# ------------------------------------------------------------------------------------------------ the host finish
def quality_from_boundary_stats(band_g, band_p, band_i, band_conf, hist, hd_sum, hd_images, hd_capped, num_classes,
                                tolerances=(1, 2, 3), max_distance=32, images=0):
    """The float64 host formulas of DESIGN.md 3.23 on plain Python ints (BoundaryStats.tolist()).  Lists hold num_classes
    entries, None for a class whose denominator is 0; means are over the classes that are not None.

    boundary_iou       band_i / (band_g + band_p - band_i)
    band_iou           band_conf[c][c] / (row c + column c - band_conf[c][c]); band_accuracy: trace / total
    contour_precision  {tolerance: per class}: the share of the prediction's contour pixels within the tolerance of the label's
    contour_recall     the same for the label's contour pixels; contour_f: 2 P R / (P + R), 0 when one side has no pixel
    hd95               hd_sum / hd_images: the mean over images of the per-image 95 % Hausdorff distance, rounded up to whole
                       pixels; hd95_capped: the images whose HD95 lies past max_distance (never folded into the mean)"""
    C = _int_in(num_classes, 1, _C8, "num_classes")
    R = _int_in(max_distance, 1, MAX_WIDTH, "max_distance")
    tolerances = [_int_in(t, 0, R, "tolerances") for t in tolerances]

    def ratio(a, b):
        return float(a) / float(b) if b else None

    def mean(values):
        seen = [v for v in values if v is not None]
        return sum(seen) / len(seen) if seen else None

    out = {"boundary_iou": [ratio(int(band_i[c]), int(band_g[c]) + int(band_p[c]) - int(band_i[c])) for c in range(C)]}
    out["mean_boundary_iou"] = mean(out["boundary_iou"])
    conf = [[int(band_conf[g][p]) for p in range(C)] for g in range(C)]
    out["band_iou"] = [ratio(conf[c][c], sum(conf[c]) + sum(conf[g][c] for g in range(C)) - conf[c][c]) for c in range(C)]
    out["mean_band_iou"] = mean(out["band_iou"])
    out["band_accuracy"] = ratio(sum(conf[c][c] for c in range(C)), sum(sum(row) for row in conf))
    out["contour_precision"], out["contour_recall"], out["contour_f"], out["mean_contour_f"] = {}, {}, {}, {}
    for th in tolerances:
        side = []
        for d in (0, 1):
            side.append([ratio(sum(int(v) for v in hist[d][c][:th + 1]), sum(int(v) for v in hist[d][c][:R + 2])) for c in range(C)])
        f = []
        for p, r in zip(*side):
            if p is None and r is None:
                f.append(None)
            elif not p or not r:
                f.append(0.0)
            else:
                f.append(2.0 * p * r / (p + r))
        out["contour_precision"][th], out["contour_recall"][th], out["contour_f"][th] = side[0], side[1], f
        out["mean_contour_f"][th] = mean(f)
    out["hd95"] = [ratio(int(hd_sum[c]), int(hd_images[c])) for c in range(C)]
    out["mean_hd95"] = mean(out["hd95"])
    out["hd95_capped"] = [int(hd_capped[c]) for c in range(C)]
    out["hd95_images"] = [int(hd_images[c]) for c in range(C)]
    out.update(images=int(images), tolerances=tolerances, max_distance=R)
    return out


class BoundaryQuality:
    """Running boundary quality over images: update() adds into one device tensor without a sync, compute() synchronises
    once.  The defaults are the published Boundary IoU: a square band of width=None (2 % of each image's diagonal) that the
    image border cuts."""

    def __init__(self, num_classes, ignore_index=None, width=None, max_distance=32, tolerances=(1, 2, 3), shape="square",
                 image_border=True):
        self.num_classes, self.max_distance = _check_settings(num_classes, width, max_distance, ignore_index, shape, image_border)[:2]
        if isinstance(tolerances, (bool, int, str, bytes)) or not hasattr(tolerances, "__iter__"):
            raise ValueError(f"tolerances: an iterable of integers in 0..max_distance, got {tolerances!r}")
        self.tolerances = tuple(_int_in(t, 0, self.max_distance, "tolerances") for t in tolerances)
        self.ignore_index = ignore_index if ignore_index is None or isinstance(ignore_index, (int, np.integer)) else tuple(ignore_index)
        self.width, self.shape, self.image_border = width, shape, bool(image_border)
        self.stats = None
        self.images = 0

    def _settings(self):
        return (self.num_classes, self.max_distance, _ignore_mask(self.ignore_index), self.width, self.shape, self.image_border)

    def update(self, pred, label):
        """add one image (no sync): pred a Prediction or a uint8 [H,W] mask, label an integer [H,W] / [1,H,W] map -> the
        running BoundaryStats"""
        mask = _mask_of(pred, "BoundaryQuality.update")
        if self.stats is not None and self.stats.words.device != mask.device:
            raise ValueError(f"update: the statistics live on {self.stats.words.device}, the prediction on {mask.device}")
        self.stats = boundary_stats(mask, label, self.num_classes, self.width, self.max_distance, self.ignore_index, self.shape,
                                    self.image_border, out=self.stats)
        self.images += 1
        return self.stats

    def reset(self):
        self.stats = None
        self.images = 0

    def add_(self, other):
        """add another BoundaryQuality's counts (merging ranks by hand: .stats.words is one int64 tensor a caller can reduce)"""
        if not isinstance(other, BoundaryQuality) or other._settings() != self._settings():
            raise ValueError("add_: a BoundaryQuality of the same settings")
        if other.stats is not None:
            if self.stats is None:
                self.stats = BoundaryStats.zeros(self.num_classes, self.max_distance, other.stats.words.device)
            self.stats.words += other.stats.words.to(self.stats.words.device)
        self.images += other.images
        return self

    def compute(self):
        """synchronises once -> plain data (json.dump-able), the keys of quality_from_boundary_stats"""
        st = self.stats.tolist() if self.stats is not None else BoundaryStats.zeros(self.num_classes, self.max_distance, "cpu").tolist()
        return quality_from_boundary_stats(**st, num_classes=self.num_classes, tolerances=self.tolerances,
                                           max_distance=self.max_distance, images=self.images)


def boundary_quality(predictions, labels, num_classes, ignore_index=None, out=None, **settings):
    """BoundaryQuality over Segmenter predictions (or uint8 masks) and their label maps at the images' own sizes: a list in,
    compute() out.  out: a BoundaryQuality to add to (its result is returned); further keywords are BoundaryQuality's."""
    from . import inference as I
    predictions = list(predictions)
    if len(labels) != len(predictions):
        raise ValueError(f"{len(labels)} label maps for {len(predictions)} predictions")
    bq = out if out is not None else BoundaryQuality(num_classes, ignore_index, **settings)
    if not isinstance(bq, BoundaryQuality) or bq.num_classes != num_classes:
        raise ValueError(f"out: a BoundaryQuality of {num_classes} classes")
    for k, p in enumerate(predictions):
        mask = _mask_of(p, f"prediction {k}")
        bq.update(mask, I._label_on(labels[k], tuple(mask.shape), mask.device, k))
    return bq.compute()
