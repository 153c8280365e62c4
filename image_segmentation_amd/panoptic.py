"""Object-level evaluation on the device: the overlap (contingency) table of a predicted and a target
segmentation, the unique IoU > 0.5 matching of their segments, and Panoptic Quality / object F1 per class -- what a
`mask.cpu()` + labelling + `np.unique` of combined ids does on the host, in integers, without leaving the device or
synchronising.

    pq = PanopticQuality(4, things=(1, 2), stuff=(0,), ignore_index=3)
    for pred, label in zip(segmenter(images), labels):
        pq.update(pred, label)                       # no sync: adds into one int64 [8,16] tensor on the device
    pq.compute()                                     # synchronises once: pq / sq / rq / f1 per class, their means

    m = match_objects(pred.mask, label, things=(1, 2))
    m.matches()                                      # synchronises: rows (target id, predicted id, inter, union)

The kernels are csrc/panoptic.hip (segk_pq_pairs, segk_pq_match) on top of segk_cc_label; there is no CPU path."""
import importlib
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, ops

_cc = importlib.import_module(".components", __package__)      # the module: the package's attribute of that name is its function

BLOCK_PIXELS, LDS_SLOTS, CHUNK, MIN_SLOTS = 2048, 256, 1024, 1024      # SEGK_PQ_* of include/segk.h
STAT_COLS = 16
MAX_PAIRS = 1 << 28
SEG_ARRAYS = ("area_g", "match_g", "inter_g", "union_g", "area_p", "void_p", "match_p")


def _r4(n):
    return (n + 3) // 4 * 4


def ws_ints(H, W, max_pairs, max_components):
    """32-bit words of workspace segk_pq_pairs needs (SEGK_PQ_WS_INTS of include/segk.h)"""
    words = (H * W + 31) // 32
    return 16 + 4 * (2 * max_pairs + MIN_SLOTS) + 2 * _r4(words) + _r4((words + CHUNK - 1) // CHUNK)


def default_max_pairs(H, W, max_components):
    return min(H * W, max(4096, 4 * max_components))


def _check_args(things, stuff, ignore_index, connectivity, max_components, max_pairs):
    """-> (things tuple, things mask, stuff mask, ignore word) after the argument checks (all before any launch)"""
    if things is None:
        raise ValueError("things: an iterable of classes (PanopticQuality(things=None) spells it out)")
    things = tuple(things) if not isinstance(things, (bool, int, str, bytes)) else things
    tmask, _ = _cc._check_args(connectivity, things, 0, False, max_components)
    smask = _cc._class_mask(stuff, "stuff")
    if tmask & smask:
        raise ValueError(f"things and stuff share classes: {sorted(set(things) & set(stuff))}")
    if not tmask and not smask:
        raise ValueError("things and stuff are both empty: nothing to evaluate")
    if ignore_index is None:
        ign = -1
    else:
        if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index:
            raise ValueError(f"ignore_index: an integer or None, got {ignore_index!r}")
        ign = int(ignore_index)
        if 0 <= ign < _lib.MAX_CLASSES and ((tmask | smask) >> ign) & 1:
            raise ValueError(f"ignore_index {ign} is one of things / stuff")
        if not 0 <= ign <= 255:
            ign = -1                                   # such a label is void already: _target_u8 maps it to 255
    if max_pairs is not None and (isinstance(max_pairs, bool) or int(max_pairs) != max_pairs or not 1 <= max_pairs <= MAX_PAIRS):
        raise ValueError(f"max_pairs: an integer in 1..2^28, got {max_pairs!r}")
    return tuple(sorted({int(c) for c in things})), tmask, smask, ign


def _check_target(target, size, dev):
    if not isinstance(target, torch.Tensor):
        raise ValueError(f"target: expected an integer [H,W] tensor, got {type(target).__name__}")
    ops._require_cuda(target, "match_objects")
    if torch.is_floating_point(target) or target.dtype == torch.bool or tuple(target.shape) not in (size, (1,) + size):
        raise ValueError(f"target: expected an integer map of {size}, got {target.dtype} {tuple(target.shape)}")
    if target.device != dev:
        raise ValueError(f"target lives on {target.device}, the prediction on {dev}")


def _target_u8(target, size):
    """a checked integer [H,W] / [1,H,W] map -> uint8 [H,W]; a value outside 0..255 becomes 255 (void)"""
    t = target.reshape(size)
    if t.dtype != torch.uint8:
        t = torch.where((t < 0) | (t > 255), 255, t).to(torch.uint8)
    return t.contiguous()


def _target_objects(target_objects, size, dev, cap):
    """(labels int32 [H,W], classes int32 [K]) on the device, K <= max_components -> (labels, classes padded to cap rows, K)"""
    if not isinstance(target_objects, (tuple, list)) or len(target_objects) != 2:
        raise ValueError("target_objects: a pair (labels int32 [H,W], classes int32 [K])")
    lab, cls = target_objects
    for t, what in ((lab, "labels"), (cls, "classes")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise ValueError(f"target_objects: {what} is an int32 tensor")
        ops._require_cuda(t, "match_objects")
        if t.device != dev:
            raise ValueError(f"target_objects: {what} live on {t.device}, the prediction on {dev}")
    if tuple(lab.shape) != size or cls.ndim != 1:
        raise ValueError(f"target_objects: labels {size} and classes [K], got {tuple(lab.shape)} and {tuple(cls.shape)}")
    K = int(cls.shape[0])
    if K > cap:
        raise ValueError(f"target_objects: {K} instances exceed max_components={cap}")
    return lab.contiguous(), cls.contiguous(), K


@dataclass
class ObjectMatch:
    pair_g: torch.Tensor        # int32 [max_pairs]   target segment of pair i (-1 void, 0 nothing), pairs in order of first pixel
    pair_p: torch.Tensor        # int32 [max_pairs]   predicted segment (0 nothing)
    pair_n: torch.Tensor        # int32 [max_pairs]   pixels the two share
    area_g: torch.Tensor        # int32 [cap + 8]     row r = segment r + 1; rows cap.. are the stuff classes
    match_g: torch.Tensor       # int32 [cap + 8]     matched predicted segment, 0: none
    inter_g: torch.Tensor       # int32 [cap + 8]
    union_g: torch.Tensor       # int32 [cap + 8]
    area_p: torch.Tensor        # int32 [cap + 8]
    void_p: torch.Tensor        # int32 [cap + 8]     pixels of the predicted segment on void
    match_p: torch.Tensor       # int32 [cap + 8]     matched target segment, 0: none
    totals: torch.Tensor        # int32 [4]           pairs, target segments, predicted segments, matches; all -1: overflow
    stats: torch.Tensor         # int64 [8,16]        the statistics this call was added to
    pred_num: torch.Tensor      # int32 [1]
    pred_cls: torch.Tensor      # int32 [cap]
    target_num: torch.Tensor    # int32 [1]
    target_cls: torch.Tensor    # int32 [cap]
    size: tuple
    max_components: int
    _h: dict = field(default_factory=dict, repr=False, compare=False)

    def _totals(self):
        if "totals" not in self._h:
            self._h["totals"] = [int(v) for v in self.totals.detach().cpu().numpy()]
        return self._h["totals"]

    @property
    def complete(self):
        """False when a capacity was exceeded (totals are -1 and nothing else was written).  Synchronises."""
        return self._totals()[0] >= 0

    def _need(self, what):
        if not self.complete:
            raise RuntimeError(f"{what}: max_pairs={self.pair_g.shape[0]} or max_components={self.max_components} was exceeded: "
                               "nothing was computed")
        return self._totals()[0]

    def pairs(self):
        """int64 [P,3]: rows (target segment, predicted segment, pixels) in order of first pixel"""
        P = self._need("pairs")
        if "pairs" not in self._h:
            self._h["pairs"] = torch.stack([self.pair_g[:P], self.pair_p[:P], self.pair_n[:P]], dim=1).cpu().numpy().astype(np.int64)
        return self._h["pairs"]

    def matches(self):
        """int64 [M,4]: rows (target segment, predicted segment, inter, union) in ascending target segment"""
        self._need("matches")
        if "matches" not in self._h:
            m, i, u = (getattr(self, n).cpu().numpy().astype(np.int64) for n in ("match_g", "inter_g", "union_g"))
            k = int(self.target_num.cpu().numpy()[0])
            rows = [r for r in list(range(k)) + list(range(self.max_components, self.max_components + 8)) if m[r] > 0]
            self._h["matches"] = np.asarray([(r + 1, m[r], i[r], u[r]) for r in rows], dtype=np.int64).reshape(-1, 4)
        return self._h["matches"]

    def contingency(self):
        """(table int64 [G,Q], target segment ids [G], predicted segment ids [Q]): the dense overlap table of the segments
        that occur (void -1 and nothing 0 included), for small cases"""
        pairs = self.pairs()
        gs, ps = np.unique(pairs[:, 0]), np.unique(pairs[:, 1])
        T = np.zeros((len(gs), len(ps)), np.int64)
        T[np.searchsorted(gs, pairs[:, 0]), np.searchsorted(ps, pairs[:, 1])] = pairs[:, 2]
        return T, gs, ps


def match_objects(pred, target, things, stuff=(), ignore_index=None, connectivity=4, max_components=1024, max_pairs=None,
                  target_objects=None, stats=None):
    """Match the objects of a predicted mask with those of a target map on their device.

    pred            a uint8 [H,W] mask or a Prediction (its .mask)
    target          an integer [H,W] / [1,H,W] map; a value equal to ignore_index or outside 0..7 is void
    things          the classes whose connected components are objects; stuff: the classes that are one segment each
    max_components  rows of the labellings; max_pairs: rows of the pair table (default min(H*W, max(4096, 4*max_components)));
                    if either is exceeded ObjectMatch.totals is all -1 and nothing else is written
    target_objects  (labels int32 [H,W], classes int32 [K]) on the device: the target's instances as given (annotation ids)
                    instead of its connected components
    stats           an int64 [8,16] device tensor to add to (default: a zeroed one)

    Nothing synchronises with the host and the inputs are not modified."""
    if hasattr(pred, "mask") and not isinstance(pred, torch.Tensor):
        pred = pred.mask
    things, tmask, smask, ign = _check_args(things, stuff, ignore_index, connectivity, max_components, max_pairs)
    pred = _cc._check_mask(pred, "match_objects")
    H, W = (int(v) for v in pred.shape)
    cap, dev = int(max_components), pred.device
    mp = default_max_pairs(H, W, cap) if max_pairs is None else int(max_pairs)
    _check_target(target, (H, W), dev)
    given = None if target_objects is None else _target_objects(target_objects, (H, W), dev, cap)
    if stats is None:
        stats = torch.zeros((_lib.MAX_CLASSES, STAT_COLS), dtype=torch.int64, device=dev)
    elif (not isinstance(stats, torch.Tensor) or stats.dtype != torch.int64 or tuple(stats.shape) != (_lib.MAX_CLASSES, STAT_COLS) or
          stats.device != dev or not stats.is_contiguous()):
        raise ValueError(f"stats: a contiguous int64 [{_lib.MAX_CLASSES},{STAT_COLS}] tensor on {dev}")
    with torch.cuda.device(dev):
        tgt = _target_u8(target, (H, W))
        i32 = dict(dtype=torch.int32, device=dev)
        labels = torch.empty((2, H, W), **i32)
        rows = torch.empty((6, cap), **i32)              # per side: cls, area, first
        box = torch.empty((2, cap, 4), **i32)
        num = torch.empty((2, 4), **i32)                 # one word per side, 16 bytes apart
        ws = torch.empty((max(_cc.ws_ints(H, W), ws_ints(H, W, mp, cap)),), **i32)
        pairs = torch.empty((3, mp), **i32)
        seg = torch.empty((7, cap + 8), **i32)
        totals = torch.empty((4,), **i32)
        s = ops._stream()
        _lib.call("segk_cc_label", pred.data_ptr(), labels[0].data_ptr(), num[0].data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(),
                  box[0].data_ptr(), rows[2].data_ptr(), ws.data_ptr(), H, W, int(connectivity), tmask, cap, s)
        if given is None:
            _lib.call("segk_cc_label", tgt.data_ptr(), labels[1].data_ptr(), num[1].data_ptr(), rows[3].data_ptr(),
                      rows[4].data_ptr(), box[1].data_ptr(), rows[5].data_ptr(), ws.data_ptr(), H, W, int(connectivity), tmask, cap, s)
            lab_g, cls_g, num_g = labels[1], rows[3], num[1]
        else:
            lab_g, cls_g = given[0], rows[3]
            cls_g[:given[2]].copy_(given[1])
            num_g = num[1]
            num_g.fill_(given[2])
        _lib.call("segk_pq_pairs", pred.data_ptr(), labels[0].data_ptr(), num[0].data_ptr(), tgt.data_ptr(), lab_g.data_ptr(),
                  num_g.data_ptr(), pairs[0].data_ptr(), pairs[1].data_ptr(), pairs[2].data_ptr(), totals.data_ptr(), ws.data_ptr(),
                  H, W, smask, ign, cap, mp, s)
        _lib.call("segk_pq_match", pairs[0].data_ptr(), pairs[1].data_ptr(), pairs[2].data_ptr(), totals.data_ptr(),
                  rows[0].data_ptr(), num[0].data_ptr(), cls_g.data_ptr(), num_g.data_ptr(), *(seg[k].data_ptr() for k in range(7)),
                  stats.data_ptr(), cap, mp, s)
    return ObjectMatch(pairs[0], pairs[1], pairs[2], *(seg[k] for k in range(7)), totals, stats, num[0, :1], rows[0], num_g[:1], cls_g,
                       (H, W), cap)


def quality_from_stats(stats, classes, num_classes):
    """The float64 host formulas of DESIGN.md 3.19 on stats [8][16] (nested lists or an array of integers) over `classes`:
    lists of num_classes entries, None for a class that is not evaluated or has TP + FP + FN == 0, and the means."""
    S = 4294967296.0
    C = int(num_classes)
    out = {k: [None] * C for k in ("pq", "sq", "rq", "f1", "tp", "fp", "fn")}
    seen = []
    for c in classes:
        tp, fp, fn, iou = (int(stats[c][k]) for k in (0, 1, 2, 3))
        out["tp"][c], out["fp"][c], out["fn"][c] = tp, fp, fn
        if tp + fp + fn == 0:
            continue
        seen.append(c)
        den = tp + fp / 2 + fn / 2
        out["pq"][c] = (iou / S) / den
        out["sq"][c] = (iou / S) / tp if tp else 0.0
        out["rq"][c] = tp / den
        f1 = []
        for k in range(10):         # a match below the threshold is a miss on both sides: FP and FN each gain tp - t
            t = int(stats[c][4 + k])
            f1.append(t / (t + (fp + tp - t) / 2 + (fn + tp - t) / 2))
        out["f1"][c] = f1
    mean = lambda v: (sum(v) / len(v)) if v else None
    for k in ("pq", "sq", "rq"):
        out["mean_" + k] = mean([out[k][c] for c in seen])
    out["mean_f1"] = [mean([out["f1"][c][k] for c in seen]) for k in range(10)]
    out["classes"] = list(classes)
    return out


class PanopticQuality:
    """Running Panoptic Quality / object F1 over images: update() adds into one device tensor without a sync, compute()
    synchronises once.  things=None: every class below num_classes but ignore_index.  Further keywords go to match_objects
    (connectivity, max_components, max_pairs)."""

    def __init__(self, num_classes, things=None, stuff=(), ignore_index=None, **match_kwargs):
        C = int(num_classes)
        if not 1 <= C <= _lib.MAX_CLASSES:
            raise ValueError(f"num_classes: 1..{_lib.MAX_CLASSES}, got {num_classes}")
        if set(match_kwargs) - {"connectivity", "max_components", "max_pairs"}:
            raise ValueError(f"unknown keywords {sorted(set(match_kwargs) - {'connectivity', 'max_components', 'max_pairs'})}")
        stuff = tuple(stuff)
        if things is None:
            things = tuple(c for c in range(C) if c != ignore_index and c not in stuff)
        self.num_classes, self.stuff, self.ignore_index, self.kwargs = C, stuff, ignore_index, dict(match_kwargs)
        self.things = _check_args(things, stuff, ignore_index, self.kwargs.get("connectivity", 4), self.kwargs.get("max_components", 1024),
                                  self.kwargs.get("max_pairs"))[0]
        if any(c >= C for c in self.things + tuple(self.stuff)):
            raise ValueError(f"things / stuff: classes below num_classes={C}")
        self.stats = self.incomplete = None
        self.images = 0

    def _state(self, dev):
        if self.stats is None:
            self.stats = torch.zeros((_lib.MAX_CLASSES, STAT_COLS), dtype=torch.int64, device=dev)
            self.incomplete = torch.zeros((1,), dtype=torch.int64, device=dev)
        return self.stats

    def update(self, pred, target, target_objects=None):
        """add one image (no sync) -> its ObjectMatch"""
        mask = pred.mask if hasattr(pred, "mask") and not isinstance(pred, torch.Tensor) else pred
        if not isinstance(mask, torch.Tensor):
            raise ValueError(f"pred: a uint8 [H,W] mask or a Prediction, got {type(pred).__name__}")
        ops._require_cuda(mask, "PanopticQuality.update")
        m = match_objects(mask, target, self.things, self.stuff, self.ignore_index, target_objects=target_objects,
                          stats=self._state(mask.device), **self.kwargs)
        self.incomplete += (m.totals[:1] < 0)
        self.images += 1
        return m

    def reset(self):
        self.stats = self.incomplete = None
        self.images = 0

    def add_(self, other):
        """add another PanopticQuality's counts (merging ranks by hand: .stats is one int64 tensor a caller can reduce)"""
        if (not isinstance(other, PanopticQuality) or (other.num_classes, other.things, other.stuff, other.ignore_index) !=
                (self.num_classes, self.things, self.stuff, self.ignore_index)):
            raise ValueError("add_: a PanopticQuality of the same classes")
        if other.stats is not None:
            self._state(other.stats.device)
            self.stats += other.stats.to(self.stats.device)
            self.incomplete += other.incomplete.to(self.stats.device)
        self.images += other.images
        return self

    def compute(self):
        """synchronises once -> plain data (json.dump-able): pq / sq / rq / f1 / tp / fp / fn per class, mean_pq / mean_sq /
        mean_rq / mean_f1 over the classes with TP + FP + FN > 0, incomplete_images, images, thresholds"""
        if self.stats is None:
            st, bad = [[0] * STAT_COLS for _ in range(_lib.MAX_CLASSES)], 0
        else:
            both = torch.cat([self.stats.reshape(-1), self.incomplete]).cpu().tolist()
            st, bad = [both[c * STAT_COLS:(c + 1) * STAT_COLS] for c in range(_lib.MAX_CLASSES)], both[-1]
        out = quality_from_stats(st, sorted(self.things + tuple(self.stuff)), self.num_classes)
        out.update(incomplete_images=int(bad), images=self.images, thresholds=[0.5 + 0.05 * k for k in range(10)])
        return out


def object_quality(predictions, labels, num_classes, things=None, stuff=(), ignore_index=None, out=None, **match_kwargs):
    """PanopticQuality over Segmenter predictions and their label maps at the images' own sizes: a list in, compute() out.
    out: a PanopticQuality to add to (its result is returned)."""
    from . import inference as I
    predictions = list(predictions)
    if len(labels) != len(predictions):
        raise ValueError(f"{len(labels)} label maps for {len(predictions)} predictions")
    pq = out if out is not None else PanopticQuality(num_classes, things, stuff, ignore_index, **match_kwargs)
    if not isinstance(pq, PanopticQuality) or pq.num_classes != int(num_classes):
        raise ValueError(f"out: a PanopticQuality of {num_classes} classes")
    for k, p in enumerate(predictions):
        mask = p.mask if hasattr(p, "mask") and not isinstance(p, torch.Tensor) else p
        if not isinstance(mask, torch.Tensor) or mask.ndim != 2:
            raise ValueError(f"prediction {k}: a uint8 [H,W] mask or a Prediction")
        ops._require_cuda(mask, "object_quality")
        pq.update(mask, I._label_on(labels[k], tuple(mask.shape), mask.device, k))
    return pq.compute()
