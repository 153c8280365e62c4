"""Mask morphology on the device: erode, dilate, open, close, hole filling, the void band around label
changes and the capped distance to the nearest different label -- the other half of a `mask.cpu()` + `scipy.ndimage` / `cv2`
post-process, without leaving the device or synchronising.

    m = seg.open_mask(pred.mask, classes=(1, 2), radius=2, fill=0)     # spurs and one-pixel bridges go
    m = seg.close_mask(m, classes=(1,), radius=3)                      # cracks close
    m = seg.fill_holes(m, classes=(1,)).mask
    label = seg.label_band(seg.rasterize(shapes, H, W), width=2)       # the 255 void band polygons do not have
    d = seg.boundary_distance(label, 8)                                # uint16, squared for the disk, 0xFFFF past the radius

Everything but the hole fill is one primitive (segk_morph): the distance D(p) from a pixel to the nearest pixel inside the
image whose key differs, under a metric ("square": max(|dx|,|dy|), "diamond": |dx|+|dy|, "disk": dx^2+dy^2 against r^2), plus
a per-pixel write rule.  Nothing erodes from the image border.  The kernels are csrc/morph.hip; there is no CPU path."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, components as _components, ops

MAX_RADIUS = _lib.MORPH_MAX_RADIUS
SHAPES = tuple(_lib.MORPH_METRICS)
_WILD = _lib.MORPH_WILD


# ------------------------------------------------------------------------------------------------ argument checks
def _byte(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255:
        raise ValueError(f"{what}: an integer in 0..255, got {v!r}")
    return int(v)


def _byte_set(classes, what):
    """an iterable of byte values -> bool [256]"""
    if isinstance(classes, (bool, int, np.integer, str, bytes)) or classes is None:
        raise ValueError(f"{what}: expected an iterable of values in 0..255, got {classes!r}")
    t = np.zeros(256, dtype=bool)
    for c in classes:
        t[_byte(c, what)] = True
    return t


def _classes(classes, what="classes"):
    t = _byte_set(classes, what)
    if not t.any():
        raise ValueError(f"{what}: at least one value")
    return t


def _radius(r, what="radius"):
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= int(r) <= MAX_RADIUS:
        raise ValueError(f"{what}: an integer in 1..{MAX_RADIUS}, got {r!r}")
    return int(r)


def _metric(shape):
    if not isinstance(shape, str) or shape not in _lib.MORPH_METRICS:
        raise ValueError(f"shape: one of {SHAPES}, got {shape!r}")
    return _lib.MORPH_METRICS[shape]


def _value_of(S, value, what):
    """value, or the single class of the set"""
    if value is None:
        if int(S.sum()) != 1:
            raise ValueError(f"{what}: value= is required with several classes")
        return int(np.flatnonzero(S)[0])
    return _byte(value, f"{what}: value")


def _check_mask(mask, what):
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{what}: expected a uint8 [H,W] tensor, got {type(mask).__name__}")
    if mask.dtype != torch.uint8 or mask.ndim != 2 or mask.shape[0] < 1 or mask.shape[1] < 1:
        raise ValueError(f"{what}: expected a uint8 [H,W] mask, got {mask.dtype} {tuple(mask.shape)}")
    if mask.shape[0] * mask.shape[1] > 1 << 28:
        raise ValueError(f"{what}: {tuple(mask.shape)} has more than 2^28 pixels")
    if not mask.is_cuda:
        raise ValueError(f"{what}: expected a tensor on the GPU -- there is no CPU path, got one on {mask.device}")
    return mask.contiguous()


# ------------------------------------------------------------------------------------------------ plans: one launch each
@dataclass(frozen=True)
class _Stage:
    """One segk_morph launch: the two tables as bytes (uint16 [256] keys, then uint8 [256] fire flags), the painted value,
    the metric and radius, whether the original map is the paint source."""
    tables: bytes
    value: int
    metric: int
    radius: int
    paint: bool = False


def _tables(key, fire):
    return np.asarray(key, dtype="<u2").tobytes() + np.asarray(fire, dtype=np.uint8).tobytes()


_table_cache = {}


def _tables_on(dev, stream, tables):
    """The tables on the device, uploaded once per (device, stream, content) without waiting for the device"""
    k = (dev.index, stream, tables)
    hit = _table_cache.get(k)
    if hit is None:
        if len(_table_cache) >= 256:
            _table_cache.clear()
        host = torch.from_numpy(np.frombuffer(tables, dtype=np.uint8).copy())
        hit = _table_cache[k] = (host.to(dev, non_blocking=True), host)
    return hit[0]


def _launch(mask, stage, paint=None, want_dist=False):
    H, W = mask.shape
    dev = mask.device
    with torch.cuda.device(dev):
        s = ops._stream()
        tab = _tables_on(dev, s, stage.tables)
        out = None if want_dist else torch.empty_like(mask)
        dist = torch.empty((H, W), dtype=torch.uint16, device=dev) if want_dist else None
        _lib.call("segk_morph", mask.data_ptr(), ops._p(paint), ops._p(out), ops._p(dist), tab.data_ptr(), tab.data_ptr() + 512,
                  stage.value, stage.metric, stage.radius, H, W, s)
    return dist if want_dist else out


def _erode_plan(classes, radius, fill, shape="disk"):
    S, r, m = _classes(classes), _radius(radius), _metric(shape)
    fill = _byte(fill, "fill")
    if S[fill]:
        raise ValueError(f"fill: {fill} is one of the classes that are eroded")
    return (_Stage(_tables(S, S), fill, m, r),)


def _dilate_plan(classes, radius, value=None, into=None, shape="disk"):
    S, r, m = _classes(classes), _radius(radius), _metric(shape)
    value = _value_of(S, value, "dilate")
    T = ~S if into is None else _byte_set(into, "into")
    if (T & S).any():
        raise ValueError("into: holds a value of classes (the set grows into other values only)")
    return (_Stage(_tables(S, T), value, m, r),)


def _open_plan(classes, radius, fill, shape="disk"):
    first, = _erode_plan(classes, radius, fill, shape)
    S = _classes(classes)
    # second stage on the eroded map: a pixel outside the set that fires against it and whose original value is in the set
    return (first, _Stage(_tables(S, ~S), 0, first.metric, first.radius, paint=True))


def _close_plan(classes, radius, value=None, shape="disk"):
    S = _classes(classes)
    value = _value_of(S, value, "close_mask")
    if not S[value]:
        raise ValueError(f"close_mask: value {value} is not one of classes")
    first, = _dilate_plan(classes, radius, value, None, shape)
    # second stage on the dilated map: a pixel of the set that fires against the outside and whose original value is outside
    return (first, _Stage(_tables(S, S), 0, first.metric, first.radius, paint=True))


def _value_keys(skip):
    key = np.arange(256, dtype=np.int64)
    key[_byte_set(skip, "skip")] = _WILD
    return key


def _band_plan(width, value=255, classes=None, skip=(), shape="disk"):
    r, m = _radius(width, "width"), _metric(shape)
    value = _byte(value, "value")
    C = np.ones(256, dtype=bool) if classes is None else _classes(classes)
    return (_Stage(_tables(_value_keys(skip), C), value, m, r),)


def _distance_plan(max_radius, classes=None, skip=(), shape="disk"):
    r, m = _radius(max_radius, "max_radius"), _metric(shape)
    key = _value_keys(skip)
    if classes is not None:
        key = np.where(key == _WILD, _WILD, _classes(classes).astype(np.int64))
    return (_Stage(_tables(key, np.ones(256, dtype=bool)), 0, m, r),)


def _fill_plan(classes, value=None, connectivity=4, max_area=None, max_components=65536):
    S = _classes(classes)
    value = _value_of(S, value, "fill_holes")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity: 4 or 8, got {connectivity!r}")
    if max_area is not None and (isinstance(max_area, bool) or not isinstance(max_area, (int, np.integer)) or max_area < 0):
        raise ValueError(f"max_area: None or a non-negative integer, got {max_area!r}")
    if isinstance(max_components, bool) or not isinstance(max_components, (int, np.integer)) or not 1 <= max_components <= 1 << 24:
        raise ValueError(f"max_components: an integer in 1..2^24, got {max_components!r}")
    lut = np.where(S, 255, 0).astype(np.uint8).tobytes()           # the complement becomes class 0, the set unlabelled
    return (lut, value, int(connectivity), (1 << 30) if max_area is None else int(min(max_area, 1 << 30)), int(max_components))


def _run(mask, plan, what):
    mask = _check_mask(mask, what)
    out = _launch(mask, plan[0])
    for stage in plan[1:]:
        out = _launch(out, stage, paint=mask)
    return out


# ------------------------------------------------------------------------------------------------ the operations
def erode(mask, classes, radius, fill, shape="disk"):
    """A pixel of `classes` within `radius` of a pixel inside the image that is not of `classes` becomes `fill` (a value
    outside classes).  scipy's binary_erosion(border_value=1) with the metric's structuring element; cv2's default border."""
    return _run(mask, _erode_plan(classes, radius, fill, shape), "erode")


def dilate(mask, classes, radius, value=None, into=None, shape="disk"):
    """A pixel not of `classes` (and of `into`, default every other value) within `radius` of a pixel of `classes` becomes
    `value` (default: the single class of classes)."""
    return _run(mask, _dilate_plan(classes, radius, value, into, shape), "dilate")


def open_mask(mask, classes, radius, fill, shape="disk"):
    """Erode, then every pixel of the original set that is in the eroded set or within `radius` of it gets its own original
    value back: spurs and bridges thinner than the element become `fill`.  Two launches."""
    return _run(mask, _open_plan(classes, radius, fill, shape), "open_mask")


def close_mask(mask, classes, radius, value=None, shape="disk"):
    """Dilate with `value` (one of classes), then every painted pixel within `radius` of a pixel the dilation left outside
    the set returns to its original value: cracks and pits narrower than the element become `value`.  Two launches."""
    return _run(mask, _close_plan(classes, radius, value, shape), "close_mask")


def label_band(label, width, value=255, classes=None, skip=(), shape="disk"):
    """The void band / trimap maker: a pixel whose value is in `classes` (default: all) and that lies within `width` of a
    pixel inside the image with a different value becomes `value`.  Values of `skip` differ from nothing and never change."""
    return _run(label, _band_plan(width, value, classes, skip, shape), "label_band")


def boundary_distance(mask, max_radius, classes=None, skip=(), shape="disk"):
    """uint16 [H,W]: the distance to the nearest pixel inside the image on the other side -- of `classes` or not, or, without
    classes, of a different value -- squared for the disk, 0xFFFF where it exceeds max_radius or nothing differs."""
    mask = _check_mask(mask, "boundary_distance")
    return _launch(mask, _distance_plan(max_radius, classes, skip, shape)[0], want_dist=True)


@dataclass
class Filled:
    mask: torch.Tensor          # uint8 [H,W]
    num: torch.Tensor           # int32 [1] on the device: components of the complement of the set
    filled: torch.Tensor        # int32 [1] on the device: how many of them were holes and took `value`
    max_components: int

    @property
    def complete(self):
        """every component had a row (synchronises); False: holes past max_components stayed unfilled"""
        return int(self.num.item()) <= self.max_components


def _fill(mask, plan):
    lut, value, conn, max_area, cap = plan
    mask = _check_mask(mask, "fill_holes")
    H, W = mask.shape
    dev = mask.device
    with torch.cuda.device(dev):
        s = ops._stream()
        i32 = dict(dtype=torch.int32, device=dev)
        table = _tables_on(dev, s, lut)
        comp, out = torch.empty_like(mask), torch.empty_like(mask)
        labels = torch.empty((H, W), **i32)
        rows = torch.empty((3, cap), **i32)                  # cls, area, first
        box = torch.empty((cap, 4), **i32)
        num, filled = torch.empty((1,), **i32), torch.zeros((1,), **i32)
        ws = torch.empty((_components.ws_ints(H, W),), **i32)
        _lib.call("segk_byte_lut", mask.data_ptr(), comp.data_ptr(), table.data_ptr(), H * W, s)
        _lib.call("segk_cc_label", comp.data_ptr(), labels.data_ptr(), num.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(),
                  box.data_ptr(), rows[2].data_ptr(), ws.data_ptr(), H, W, conn, 1, cap, s)
        _lib.call("segk_fill_holes", mask.data_ptr(), labels.data_ptr(), num.data_ptr(), rows[1].data_ptr(), box.data_ptr(),
                  rows[2].data_ptr(), out.data_ptr(), filled.data_ptr(), value, max_area, H, W, cap, s)
    return Filled(out, num, filled, cap)


def fill_holes(mask, classes, value=None, connectivity=4, max_area=None, max_components=65536):
    """Fill the holes of the set of `classes` with `value` (default: its single class).  A hole is a connected component
    (`connectivity` 4, scipy's binary_fill_holes default, or 8) of the complement of the set whose box does not touch the
    image border and whose area is <= max_area.  Components past max_components stay unfilled: Filled.complete tells."""
    return _fill(mask, _fill_plan(classes, value, connectivity, max_area, max_components))


# ------------------------------------------------------------------------------------------------ Segmenter(morph=[...])
_OPS = {"erode": _erode_plan, "dilate": _dilate_plan, "open": _open_plan, "close": _close_plan, "label_band": _band_plan,
        "fill_holes": _fill_plan}


class MorphStep:
    """One step of Segmenter(morph=[...]): an operation ("erode", "dilate", "open", "close", "fill_holes", "label_band") and
    the keywords of its function.  The arguments are checked here, before any prediction runs."""
    __slots__ = ("op", "keywords", "plan")

    def __init__(self, op, **keywords):
        if op not in _OPS:
            raise ValueError(f"morph: op is one of {tuple(_OPS)}, got {op!r}")
        try:
            self.plan = _OPS[op](**keywords)
        except TypeError as e:                               # an unknown or a missing keyword
            raise ValueError(f"morph: {op}: {e}") from None
        self.op, self.keywords = op, dict(keywords)

    def __repr__(self):
        return "MorphStep(" + ", ".join([repr(self.op)] + [f"{k}={v!r}" for k, v in self.keywords.items()]) + ")"

    def __eq__(self, other):
        return isinstance(other, MorphStep) and (self.op, self.plan) == (other.op, other.plan)

    def __hash__(self):
        return hash((self.op, self.plan))

    def __call__(self, mask):
        """the step applied to a uint8 [H,W] mask on the device -> the new mask"""
        return _fill(mask, self.plan).mask if self.op == "fill_holes" else _run(mask, self.plan, self.op)


def as_morph(morph):
    """None, or a sequence of MorphStep records / dicts {"op": ..., keywords} -> None or a tuple of MorphSteps"""
    if morph is None:
        return None
    if isinstance(morph, (MorphStep, dict, str, bytes)) or not hasattr(morph, "__iter__"):
        raise ValueError(f"morph: None or a sequence of MorphStep records or dicts, got {type(morph).__name__}")
    steps = []
    for st in morph:
        if isinstance(st, dict):
            if "op" not in st:
                raise ValueError(f"morph: a dict step names its op, got {st!r}")
            st = MorphStep(st["op"], **{k: v for k, v in st.items() if k != "op"})
        if not isinstance(st, MorphStep):
            raise ValueError(f"morph: a step is a MorphStep or a dict, got {type(st).__name__}")
        steps.append(st)
    return tuple(steps)
