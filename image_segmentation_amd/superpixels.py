"""Superpixels on the device: SLIC in the pixel-centric integer form, and snapping a mask to a segmentation
by a per-segment majority vote -- the image-aware refinement that an `image.cpu()` + `skimage.segmentation.slic` pass and a
Python loop over segments do on the host, without leaving the device or synchronising.

    sp = seg.superpixels(image, step=16, compactness=20, iterations=10, space="ycc")
    sp.labels, sp.centres, sp.counts          # int32 [H,W], [K,5], [K] on the device; sp.grid, sp.step, sp.k: host ints
    v = seg.snap_mask(pred.mask, sp, min_share=0.5, weights=pred.confidence, fill=(255,))
    v.mask, v.hist, v.winner                  # uint8 [H,W], int64 [K,8], int32 [K]
    v = seg.snap_mask(mask, labels, k=K)      # any int32 label map will do

Everything is integer arithmetic with ties broken by index, so results are unique and bit-stable.  Ids are home cells of the
grid: they are not dense, `counts` tells which are empty, and segments are not forced to be connected.  The kernels are
csrc/slic.hip; there is no CPU path."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .morph import _byte_set, _check_mask

MIN_STEP, MAX_STEP = _lib.SLIC_MIN_STEP, _lib.SLIC_MAX_STEP
MAX_COMPACTNESS, MAX_ITERATIONS = _lib.SLIC_MAX_COMPACTNESS, _lib.SLIC_MAX_ITERATIONS
SPACES = tuple(_lib.SLIC_SPACES)
_C8 = _lib.MAX_CLASSES


# ------------------------------------------------------------------------------------------------ argument checks
def _int_in(v, lo, hi, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def _slic_settings(step, compactness, iterations, space):
    S = _int_in(step, MIN_STEP, MAX_STEP, "step")
    m = _int_in(compactness, 1, MAX_COMPACTNESS, "compactness")
    T = _int_in(iterations, 1, MAX_ITERATIONS, "iterations")
    if not isinstance(space, str) or space not in _lib.SLIC_SPACES:
        raise ValueError(f"space: one of {SPACES}, got {space!r}")
    return S, m, T, _lib.SLIC_SPACES[space]


def tile_rows(H, W):
    """Rows of a kernel tile (64 columns wide) for an H x W image: the tallest of 64, 16, 4 that still gives 1024 workgroups
    -- four for each of the 256 CUs --, and 4 where none does.  The result of a kernel does not depend on it."""
    for rows in _lib.SLIC_TILE_ROWS:
        if -(-H // rows) * -(-W // _lib.SLIC_TILE) >= 1024:
            return rows
    return _lib.SLIC_TILE_ROWS[-1]


def share_of(min_share):
    """min_share, a number in [0, 1] -> 0..256 of 256: floor(256 min_share + 1/2), rounded once, here"""
    if isinstance(min_share, bool) or not isinstance(min_share, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(min_share) <= 1.0:                                    # a NaN fails the comparison too
        raise ValueError(f"min_share: a number in [0, 1], got {min_share!r}")
    return int(math.floor(256.0 * float(min_share) + 0.5))


def _class_set(classes):
    """None (all eight) or an iterable of values below 8 -> bool [256]"""
    if classes is None:
        t = np.zeros(256, dtype=bool)
        t[:_C8] = True
        return t
    t = _byte_set(classes, "classes")
    if not t.any():
        raise ValueError("classes: at least one value")
    if t[_C8:].any():
        raise ValueError(f"classes: values below {_C8} vote, got {int(np.flatnonzero(t)[-1])}")
    return t


def _snap_sets(classes, fill):
    """-> (the bits of classes, the four 64-bit words of classes | fill as signed ints)"""
    S, F = _class_set(classes), _byte_set(fill, "fill")
    if (S & F).any():
        raise ValueError(f"fill: {int(np.flatnonzero(S & F)[0])} is one of the classes that vote")
    allow = S | F
    words = []
    for j in range(4):
        w = sum(1 << b for b in range(64) if allow[64 * j + b])
        words.append(w - (1 << 64) if w >= 1 << 63 else w)
    return sum(1 << c for c in range(_C8) if S[c]), tuple(words)


def _check_image(image):
    if not isinstance(image, torch.Tensor):
        raise ValueError(f"superpixels: expected a uint8 [H,W,C] tensor, got {type(image).__name__}")
    if image.dtype != torch.uint8:
        raise ValueError(f"superpixels: expected a uint8 [H,W,C] image (1, 3 or 4 channels, or [H,W]), got {image.dtype} "
                         f"{tuple(image.shape)} -- a float image is not taken")
    if image.ndim == 2:
        image = image.unsqueeze(-1)
    if image.ndim != 3 or image.shape[2] not in (1, 3, 4) or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"superpixels: expected a uint8 [H,W,C] image with 1, 3 or 4 channels (or [H,W]), got {tuple(image.shape)}")
    if image.shape[0] * image.shape[1] > 1 << 28 or max(image.shape[:2]) > _lib.SLIC_MAX_SIDE:
        raise ValueError(f"superpixels: {tuple(image.shape[:2])} has more than 2^28 pixels or a side past 2^27")
    if not image.is_cuda:
        raise ValueError(f"superpixels: expected a tensor on the GPU -- there is no CPU path, got one on {image.device}")
    return image.contiguous()


# ------------------------------------------------------------------------------------------------ SLIC
@dataclass
class Superpixels:
    labels: torch.Tensor        # int32 [H,W]: the last assignment, values in 0..k-1 (ids are home cells: not dense)
    centres: torch.Tensor       # int32 [k,5]: (Y, X, C0, C1, C2) in 1/16 units, after the last update
    counts: torch.Tensor        # int32 [k]: pixels per id in `labels`; 0: the id is empty
    grid: Tuple[int, int]       # (ny, nx) cells; k = ny nx
    step: int
    k: int


def superpixels(image, step=16, compactness=20, iterations=10, space="ycc"):
    """SLIC superpixels of a uint8 [H,W,C] image (C of 1, 3 or 4, the alpha ignored; or [H,W]) on the device -> Superpixels.

    step         the grid spacing S in pixels, 4..64: k = ceil(H / S) ceil(W / S) segments of about S x S pixels
    compactness  m, 1..255: D = S^2 |colour|^2 + m^2 |position|^2; larger keeps segments square, 1 lets them follow colour
    iterations   rounds of assign and update, 1..20
    space        "ycc" (an integer luma / chroma transform) or "rgb"; a grey image has its one feature in either

    2 iterations + 1 launches in stream order; nothing synchronises with the host and the image is not modified."""
    S, m, T, sp = _slic_settings(step, compactness, iterations, space)
    image = _check_image(image)
    H, W, C = (int(v) for v in image.shape)
    ny, nx = -(-H // S), -(-W // S)
    K = ny * nx
    dev = image.device
    with torch.cuda.device(dev):
        s = ops._stream()
        i32 = dict(dtype=torch.int32, device=dev)
        labels = torch.empty((H, W), **i32)
        centres = torch.empty((K, _lib.SLIC_CENTRE_WORDS), **i32)
        counts = torch.empty((K,), **i32)
        sums = torch.empty((K, _lib.SLIC_SUM_WORDS), **i32)
        rows = tile_rows(H, W)
        _lib.call("segk_slic_start", image.data_ptr(), centres.data_ptr(), sums.data_ptr(), C, sp, S, H, W, K, s)
        for t in range(T):
            _lib.call("segk_slic_assign", image.data_ptr(), centres.data_ptr(), sums.data_ptr(), labels.data_ptr(), C, sp, S, m, t, T,
                      rows, H, W, K, s)
            _lib.call("segk_slic_update", centres.data_ptr(), sums.data_ptr(), counts.data_ptr(), S, H, W, K, s)
    return Superpixels(labels, centres, counts, (ny, nx), S, K)


# ------------------------------------------------------------------------------------------------ vote and snap
@dataclass
class Snapped:
    mask: torch.Tensor          # uint8 [H,W]
    hist: torch.Tensor          # int64 [k,8]: the votes per segment and class
    winner: torch.Tensor        # int32 [k]: the class of the largest entry, the lowest on a tie, -1 without a vote


def _labels_of(sp, k, size):
    if isinstance(sp, Superpixels):
        if k is not None and k != sp.k:
            raise ValueError(f"k: the Superpixels has {sp.k} ids, got k={k!r}")
        labels, k = sp.labels, sp.k
    else:
        labels = sp
        if k is None:
            raise ValueError("snap_mask: k= (the number of ids) is required with a label map")
        k = _int_in(k, 1, 1 << 28, "k")
    if not isinstance(labels, torch.Tensor):
        raise ValueError(f"snap_mask: expected a Superpixels or an int32 [H,W] label map, got {type(sp).__name__}")
    if labels.dtype != torch.int32 or labels.ndim != 2:
        raise ValueError(f"snap_mask: expected an int32 [H,W] label map, got {labels.dtype} {tuple(labels.shape)}")
    if tuple(labels.shape) != size:
        raise ValueError(f"snap_mask: the label map is {tuple(labels.shape)}, the mask {size}")
    return labels, k


def _snap(mask, sp, k, bits, words, share, weights):
    # types, ranks and sizes first, the devices last: what is wrong with the arguments themselves is told on any machine
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.ndim != 2 or mask.shape[0] < 1 or mask.shape[1] < 1:
        got = f"{mask.dtype} {tuple(mask.shape)}" if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise ValueError(f"snap_mask: expected a uint8 [H,W] mask, got {got}")
    H, W = (int(v) for v in mask.shape)
    labels, K = _labels_of(sp, k, (H, W))
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.uint8 or weights.ndim != 2:
            got = f"{weights.dtype} {tuple(weights.shape)}" if isinstance(weights, torch.Tensor) else type(weights).__name__
            raise ValueError(f"weights: expected a uint8 [H,W] tensor, got {got}")
        if tuple(weights.shape) != (H, W):
            raise ValueError(f"weights: {tuple(weights.shape)}, the mask is {(H, W)}")
    mask = _check_mask(mask, "snap_mask")
    dev = mask.device
    for t, what in ((labels, "the label map"), (weights, "weights")):
        if t is not None and not t.is_cuda:
            raise ValueError(f"snap_mask: expected a tensor on the GPU -- there is no CPU path, got {what} on {t.device}")
        if t is not None and t.device != dev:
            raise ValueError(f"snap_mask: {what} lives on {t.device}, the mask on {dev}")
    labels = labels.contiguous()
    weights = None if weights is None else weights.contiguous()
    with torch.cuda.device(dev):
        s = ops._stream()
        hist = torch.zeros((K, _C8), dtype=torch.int64, device=dev)
        winner = torch.empty((K,), dtype=torch.int32, device=dev)
        paint = torch.empty((K,), dtype=torch.uint8, device=dev)
        out = torch.empty_like(mask)
        _lib.call("segk_snap_vote", labels.data_ptr(), mask.data_ptr(), ops._p(weights), hist.data_ptr(), bits, tile_rows(H, W), H, W, K, s)
        _lib.call("segk_snap_paint", labels.data_ptr(), mask.data_ptr(), hist.data_ptr(), winner.data_ptr(), paint.data_ptr(),
                  out.data_ptr(), *words, share, H, W, K, s)
    return Snapped(out, hist, winner)


def snap_mask(mask, sp, classes=None, min_share=0.5, weights=None, fill=(), k=None):
    """Snap a uint8 [H,W] mask to a segmentation: every segment votes, and its pixels take the winning class -> Snapped.

    sp         a Superpixels, or an int32 [H,W] label map with k= ids; a pixel whose label is outside 0..k-1 neither votes
               nor changes
    classes    the values (below 8) that vote and may change; None: all eight
    min_share  a segment is painted when its winner holds at least this share of the segment's votes, a number in [0, 1]
               rounded once to floor(256 min_share + 1/2) of 256; ties between classes go to the lowest
    weights    None (a vote weighs 1) or a uint8 [H,W] map, as Prediction.confidence: a vote weighs weights[p]
    fill       byte values outside classes that never vote but are painted: a void class, the ring of label_band

    Three launches, nothing synchronises with the host and the inputs are not modified."""
    bits, words = _snap_sets(classes, fill)
    return _snap(mask, sp, k, bits, words, share_of(min_share), weights)


# ------------------------------------------------------------------------------------------------ Segmenter(snap=...)
@dataclass(frozen=True)
class Snap:
    """The settings of Segmenter(snap=...): superpixels of the input image (step, compactness, iterations, space), then
    snap_mask of the argmax (classes, min_share, fill; weighted: the votes weigh the route's confidence map).  Checked here,
    before any prediction runs."""
    step: int = 16
    compactness: int = 20
    iterations: int = 10
    space: str = "ycc"
    classes: Optional[Tuple[int, ...]] = None
    min_share: float = 0.5
    fill: Tuple[int, ...] = ()
    weighted: bool = False

    def __post_init__(self):
        _slic_settings(self.step, self.compactness, self.iterations, self.space)
        if not isinstance(self.weighted, (bool, np.bool_)):
            raise ValueError(f"weighted: True or False, got {self.weighted!r}")
        bits, words = _snap_sets(self.classes, self.fill)
        object.__setattr__(self, "_plan", (bits, words, share_of(self.min_share)))
        if self.classes is not None:
            object.__setattr__(self, "classes", tuple(int(c) for c in self.classes))
        object.__setattr__(self, "fill", tuple(int(v) for v in self.fill))

    def __call__(self, image, mask, confidence=None):
        """-> (the Superpixels of `image`, the Snapped mask)"""
        sp = superpixels(image, self.step, self.compactness, self.iterations, self.space)
        return sp, _snap(mask, sp, None, *self._plan, confidence if self.weighted else None)


def as_snap(snap):
    """None, a Snap or a dict of its keywords -> None or a Snap"""
    if snap is None or isinstance(snap, Snap):
        return snap
    if not isinstance(snap, dict):
        raise ValueError(f"snap: None, a Snap or a dict of its keywords, got {type(snap).__name__}")
    try:
        return Snap(**snap)
    except TypeError as e:                                   # an unknown keyword
        raise ValueError(f"snap: {e}") from None
