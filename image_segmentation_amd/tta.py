"""Test-time augmentation and ensembling: the host side of segk_predict_merge.

A VIEW of an image is (model, target size T, flip, weight): the network output for the flipped image resized and padded to
T x T.  TTA names the (size, flip) views of one model; Segmenter multiplies them by its models.  view_table builds the
device kernel's descriptor table on the host and refuses what the kernel itself cannot check (the table lives in device
memory).  Nothing here touches the GPU."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _lib

FLIPS = {"": 0, "h": 1, "v": 2, "hv": 3}       # bit 0 reverses x, bit 1 reverses y (the flip argument of the kernels)
MERGES = {"prob": 0, "logit": 1}               # SEGK_MERGE_PROB / SEGK_MERGE_LOGIT
KINDS = {"logits": 0, "probs": 1}
MAX_VIEWS = _lib.MAX_VIEWS

# segk_view_desc of include/segk.h
VIEW_DESC = np.dtype([("slot", "<u8"), ("T", "<i4"), ("pad_top", "<i4"), ("pad_left", "<i4"), ("nh", "<i4"), ("nw", "<i4"),
                      ("flip", "<i4"), ("kind", "<i4"), ("weight", "<f4"), ("pad_", "<i4", (2,))])
assert VIEW_DESC.itemsize == 48


def _positive(values, what):
    out = tuple(float(w) for w in values)
    if not out or any(not (w > 0 and math.isfinite(w)) for w in out):
        raise ValueError(f"{what}: positive finite numbers, got {tuple(values)}")
    return out


@dataclass(frozen=True)
class TTA:
    """The views of one model: every size in `sizes` (None: the Segmenter's target_size) times every flip in `flips`
    ("" none, "h" x reversed, "v" y reversed, "hv" both), sizes-major, in the order given -- the order is part of the
    result (fp32 sums in view order).  merge: "prob" (probabilities are averaged) or "logit".  weights: one positive number
    per (size, flip) view in that order, None for equal weights."""
    flips: Tuple[str, ...] = ("", "h")
    sizes: Optional[Tuple[int, ...]] = None
    merge: str = "prob"
    weights: Optional[Tuple[float, ...]] = None

    def __post_init__(self):
        flips = (self.flips,) if isinstance(self.flips, str) else tuple(self.flips)
        if not flips or any(f not in FLIPS for f in flips) or len(set(flips)) != len(flips):
            raise ValueError(f"flips: distinct entries of {tuple(FLIPS)}, got {self.flips!r}")
        object.__setattr__(self, "flips", flips)
        if self.sizes is not None:
            sizes = (self.sizes,) if isinstance(self.sizes, int) else tuple(self.sizes)
            if not sizes or any(int(t) != t or int(t) < 1 for t in sizes) or len(set(sizes)) != len(sizes):
                raise ValueError(f"sizes: distinct positive integers, got {self.sizes!r}")
            object.__setattr__(self, "sizes", tuple(int(t) for t in sizes))
        if self.merge not in MERGES:
            raise ValueError(f"merge: one of {tuple(MERGES)}, got {self.merge!r}")
        if self.weights is not None:
            weights = _positive(self.weights, "weights")
            n = len(flips) * (1 if self.sizes is None else len(self.sizes))
            if len(weights) != n:
                raise ValueError(f"weights: {len(weights)} entries for {n} (size, flip) views")
            object.__setattr__(self, "weights", weights)

    def views(self, target_size):
        """[(T, flip, weight)] in view order; target_size stands in for sizes=None."""
        sizes = (int(target_size),) if self.sizes is None else self.sizes
        pairs = [(T, f) for T in sizes for f in self.flips]
        weights = self.weights if self.weights is not None else (1.0,) * len(pairs)
        return [(T, f, w) for (T, f), w in zip(pairs, weights)]


def view_order(n_models, tta, target_size, model_weights=None):
    """[(model index, T, flip, weight)]: models-major, then sizes, then flips, each in the order given."""
    mw = (1.0,) * n_models if model_weights is None else _positive(model_weights, "model_weights")
    if len(mw) != n_models:
        raise ValueError(f"model_weights: {len(mw)} entries for {n_models} models")
    views = [(m, T, f, mw[m] * w) for m in range(n_models) for T, f, w in tta.views(target_size)]
    if len(views) > MAX_VIEWS:
        raise ValueError(f"{len(views)} views ({n_models} models x {len(views) // n_models}): at most {MAX_VIEWS}")
    return views


def view_table(views):
    """Descriptor table of one image for segk_predict_merge: a VIEW_DESC array, one row per view in the order given.
    views: rows of (slot address, T, pad_top, pad_left, nh, nw, flip, kind, weight) -- the slot's geometry as
    utils._geometry gives it, flip a key of FLIPS or its number, kind a key of KINDS or its number, weight > 0.  The weights
    are divided by their sum in float64 and rounded once to float32."""
    views = list(views)
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"{len(views)} views: 1..{MAX_VIEWS} supported")
    table = np.zeros(len(views), dtype=VIEW_DESC)
    weights = []
    for v, row in enumerate(views):
        slot, T, pt, pl, nh, nw, flip, kind, w = row
        flip = FLIPS.get(flip, flip) if isinstance(flip, str) else flip
        kind = KINDS.get(kind, kind) if isinstance(kind, str) else kind
        if flip not in (0, 1, 2, 3):
            raise ValueError(f"view {v}: unknown flip {row[6]!r} (one of {tuple(FLIPS)} or 0..3)")
        if kind not in (0, 1):
            raise ValueError(f"view {v}: unknown kind {row[7]!r} (one of {tuple(KINDS)} or 0 / 1)")
        if int(slot) <= 0 or int(slot) % 4:
            raise ValueError(f"view {v}: the slot address must be non-zero and 4-byte aligned")
        T, pt, pl, nh, nw = (int(a) for a in (T, pt, pl, nh, nw))
        if T < 1 or T * T >= 1 << 30:
            raise ValueError(f"view {v}: a slot side of {T} (1 <= T, T*T < 2^30)")
        if nh < 1 or nw < 1 or pt < 0 or pl < 0 or pt + nh > T or pl + nw > T:
            raise ValueError(f"view {v}: window {nh} x {nw} at ({pt}, {pl}) lies outside the {T} x {T} slot")
        if not (float(w) > 0 and math.isfinite(float(w))):
            raise ValueError(f"view {v}: weight must be positive and finite, got {w}")
        weights.append(float(w))
        table[v] = (int(slot), T, pt, pl, nh, nw, flip, kind, 0.0, (0, 0))
    total = math.fsum(weights)
    table["weight"] = np.asarray([w / total for w in weights], dtype=np.float64).astype(np.float32)
    return table
