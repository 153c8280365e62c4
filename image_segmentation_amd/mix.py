"""Mixed-sample augmentation on the device: CutMix, ClassMix and object copy-paste.  Where the Augmenter
gives every sample one single-image operation, a Mixer pastes a part of ANOTHER sample of the batch into it: a rectangle
("cutmix"), half of the partner's classes ("classmix", from its labels or from a teacher's pseudo-labels) or whole objects with a
shift and a flip ("copy_paste").

    mixer = Mixer(("cutmix", "classmix", "copy_paste"), p=0.5, seam_value=255, flip=True, max_shift=0.25, seed=0)
    X, y = mixer(X, y)                                         # fresh tensors of the inputs' shapes and dtypes
    mixer.last["pasted"]                                       # int32 [B] on the device: pixels pasted per sample
    for X, y in MixedBatches(AugmentedBatches(loader, aug), mixer): ...      # what train_loop / start / train_loop_distill take

Which classes or objects get pasted depends on the partner's labels, which live on the device: the selection is made there
(segk_mix_select), so a batch costs no synchronisation.  Every output value is a copy of one input value; the paste bit is
defined in integers and the device equals the NumPy restatement of tests/mix_reference.py bit for bit.  The kernels are
csrc/mix.hip; there is no CPU path."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from .components import _class_mask, ws_ints
from .augment import _upload

NONE, BOX, CLASS, OBJECT = _lib.MIX_NONE, _lib.MIX_BOX, _lib.MIX_CLASS, _lib.MIX_OBJECT
MODES = {"cutmix": BOX, "classmix": CLASS, "copy_paste": OBJECT}
MODE_NAMES = ("none", "cutmix", "classmix", "copy_paste")
MAX_OBJECTS, MAX_COMPONENTS = _lib.MIX_MAX_OBJECTS, _lib.MIX_MAX_COMPONENTS
MAX_PIXELS = 1 << 28                     # SEGK_CC_MAX_PIXELS
MAX_AREA = 1 << 30

# segk_mix_desc of include/segk.h
DESC = np.dtype([("seed", "<u8"), ("mode", "<i4"), ("partner", "<i4"), ("flip", "<i4"), ("dy", "<i4"), ("dx", "<i4"), ("y0", "<i4"),
                 ("x0", "<i4"), ("y1", "<i4"), ("x1", "<i4"), ("slot", "<i4"), ("pad_", "<i4", (4,))])
assert DESC.itemsize == 64

_IMAGE_DTYPES = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2, torch.uint8: 1}
_LABEL_DTYPES = {torch.int64: 8, torch.uint8: 1}


@dataclass(frozen=True)
class MixPlan:
    """What one sample gets: drawn by Mixer.plan on the host, applied by Mixer.apply on the device."""
    mode: int = NONE                # NONE, BOX, CLASS, OBJECT
    partner: int = 0                # the sample that is pasted from; the sample itself is legal
    flip: int = 0                   # 1: the partner is mirrored horizontally
    dy: int = 0                     # output (y, x) looks at partner (y - dy, flip ? W - 1 - (x - dx) : x - dx)
    dx: int = 0
    box: tuple = (0, 0, 0, 0)       # BOX: (y0, x0, y1, x1) in output coordinates, y1 and x1 exclusive
    seed: int = 0                   # of the selection keys (CLASS, OBJECT)


def _int(v, lo, hi, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def _byte_table(values, what):
    if isinstance(values, (bool, int, np.integer, str, bytes)) or values is None:
        raise ValueError(f"{what}: expected an iterable of values in 0..255, got {values!r}")
    t = np.zeros(256, dtype=np.uint8)
    for v in values:
        t[_int(v, 0, 255, what)] = 1
    return t


def _overlaps(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_plan(k, p, B, H, W):
    """one plan, field by field: the messages"""
    if not isinstance(p, MixPlan):
        raise TypeError(f"plans[{k}]: expected a MixPlan, got {type(p).__name__}")
    _int(p.mode, NONE, OBJECT, f"plans[{k}].mode")
    _int(p.partner, 0, B - 1, f"plans[{k}].partner")
    _int(p.flip, 0, 1, f"plans[{k}].flip")
    _int(p.dy, -(1 << 30), 1 << 30, f"plans[{k}].dy")
    _int(p.dx, -(1 << 30), 1 << 30, f"plans[{k}].dx")
    _int(p.seed, 0, (1 << 64) - 1, f"plans[{k}].seed")
    if not isinstance(p.box, tuple) or len(p.box) != 4:
        raise ValueError(f"plans[{k}].box: (y0, x0, y1, x1), got {p.box!r}")
    y0, x0, y1, x1 = (_int(v, 0, 1 << 30, f"plans[{k}].box") for v in p.box)
    if p.mode == BOX and not (y0 <= y1 <= H and x0 <= x1 <= W):
        raise ValueError(f"plans[{k}].box: {p.box} is not 0 <= y0 <= y1 <= {H}, 0 <= x0 <= x1 <= {W}")


def _plan_table(plans, B, H, W):
    """-> (int64 [B,9]: mode, partner, flip, dy, dx, y0, x0, y1, x1; uint64 [B]: the seeds) of checked plans.  Plans made of
    Python integers inside their ranges pass in one sweep; anything else is walked field by field for its message."""
    ok = False
    try:
        if all(type(p) is MixPlan and type(p.box) is tuple for p in plans):
            rows = [(p.mode, p.partner, p.flip, p.dy, p.dx, p.seed) + p.box for p in plans]
            if all(len(r) == 10 and set(map(type, r)) == {int} for r in rows) and all(0 <= r[5] < 1 << 64 for r in rows):
                t = np.array([r[:5] + r[6:] for r in rows], dtype=np.int64).reshape(B, 9)
                seeds = np.array([r[5] for r in rows], dtype=np.uint64)
                box = t[:, 0] == BOX
                ok = bool(((t[:, 0] >= NONE) & (t[:, 0] <= OBJECT) & (t[:, 1] >= 0) & (t[:, 1] < B) & (t[:, 2] >= 0) & (t[:, 2] <= 1)
                           & (np.abs(t[:, 3:5]) <= 1 << 30).all(1) & (t[:, 5:] >= 0).all(1) & (t[:, 5:] <= 1 << 30).all(1)
                           & (~box | ((t[:, 5] <= t[:, 7]) & (t[:, 7] <= H) & (t[:, 6] <= t[:, 8]) & (t[:, 8] <= W)))).all())
    except OverflowError:
        ok = False
    if not ok:
        for k, p in enumerate(plans):
            _check_plan(k, p, B, H, W)
        t = np.array([[int(v) for v in (p.mode, p.partner, p.flip, p.dy, p.dx) + p.box] for p in plans], dtype=np.int64).reshape(B, 9)
        seeds = np.array([int(p.seed) for p in plans], dtype=np.uint64)
    return t, seeds


class Mixer:
    """(X, y) -> (X', y') with, at probability p per sample, a part of another sample of the batch pasted in.

    mode            "cutmix", "classmix", "copy_paste", or a tuple of them that is drawn from uniformly
    p               probability that a sample is mixed at all
    exclude         classmix: byte values that are never pasted (the ignore value, the background)
    n_classes       classmix: paste min(n, n_classes) of the n candidate classes instead of ceil(n / 2)
    seam_value      None, or the label a pixel gets when a 4-neighbour inside the image lies on the other side of a paste seam
    flip            draw horizontal flips of the partner
    max_shift       copy_paste: shifts are drawn uniformly from +- max_shift of the side
    box_area        cutmix: the box's share of the image area is drawn uniformly from this range
    things, connectivity, min_area, max_area, max_objects, max_components
                    copy_paste: the partner's label map is labelled by segk_cc_label over the classes `things` (a subset of
                    0..7); of the components 1..min(K, max_components) with min_area <= area <= max_area, min(n, max_objects)
                    are pasted

    plan(B, H, W) draws on the host from a NumPy Generator seeded with `seed`; always all of it, B values at a time, in this
    order: u = random(), the index of the mode, the partner, the flip bit, the shifts sy then sx in [-1, 1), the box's area
    share, the exponent of its aspect ratio 2^e with e in [-1, 1), the box's corner y0 then x0, the 64-bit seed.  Two Mixers with one seed draw the same plans;
    reseed() rewinds.  apply() is a pure function of (X, y, plans): it checks every argument before the first launch and never
    synchronises."""

    def __init__(self, mode="cutmix", p=0.5, exclude=(), n_classes=None, seam_value=None, flip=False, max_shift=0.0,
                 box_area=(0.1, 0.5), things=(1, 2, 3, 4, 5, 6, 7), connectivity=4, min_area=64, max_area=None, max_objects=4,
                 max_components=1024, seed=None):
        modes = (mode,) if isinstance(mode, str) else tuple(mode)
        if not modes or any(not isinstance(m, str) or m not in MODES for m in modes):
            raise ValueError(f"mode: one of {tuple(MODES)} or a non-empty tuple of them, got {mode!r}")
        self.modes = tuple(MODES[m] for m in modes)
        if isinstance(p, bool) or not isinstance(p, (int, float, np.floating, np.integer)) or not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"p: a probability in 0..1, got {p!r}")
        self.p = float(p)
        self._exclude = _byte_table(exclude, "exclude")
        self.n_classes = 0 if n_classes is None else _int(n_classes, 1, 256, "n_classes")
        if seam_value is not None and (isinstance(seam_value, bool) or not isinstance(seam_value, (int, np.integer))
                                       or not -(1 << 63) <= int(seam_value) < (1 << 63)):
            raise ValueError(f"seam_value: None or an integer label, got {seam_value!r}")
        self.seam_value = None if seam_value is None else int(seam_value)
        self.flip = bool(flip)
        if isinstance(max_shift, bool) or not isinstance(max_shift, (int, float, np.floating, np.integer)) or not 0.0 <= float(max_shift) <= 1.0:
            raise ValueError(f"max_shift: a fraction of the side in 0..1, got {max_shift!r}")
        self.max_shift = float(max_shift)
        try:
            lo, hi = (float(v) for v in box_area)
        except (TypeError, ValueError):
            raise ValueError(f"box_area: a pair of area shares, got {box_area!r}") from None
        if not 0.0 < lo <= hi <= 1.0:
            raise ValueError(f"box_area: 0 < low <= high <= 1, got {box_area!r}")
        self.box_area = (lo, hi)
        self._things = _class_mask(things, "things")
        if things is None or self._things == 0:
            raise ValueError(f"things: a non-empty subset of 0..{_lib.MAX_CLASSES - 1}, got {things!r}")
        if connectivity not in (4, 8) or isinstance(connectivity, bool):
            raise ValueError(f"connectivity: 4 or 8, got {connectivity!r}")
        self.connectivity = int(connectivity)
        self.min_area = _int(min_area, 0, MAX_AREA, "min_area")
        self.max_area = MAX_AREA if max_area is None else _int(max_area, self.min_area, MAX_AREA, "max_area")
        self.max_objects = _int(max_objects, 1, MAX_OBJECTS, "max_objects")
        self.max_components = _int(max_components, 1, MAX_COMPONENTS, "max_components")
        self.seed = seed
        self._rng = None
        self.last = {}

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

    def plan(self, B, H, W):
        """-> list of B MixPlans for samples of H x W."""
        B, H, W = _int(B, 1, 65535, "B"), _int(H, 1, MAX_PIXELS, "H"), _int(W, 1, MAX_PIXELS, "W")
        rng = self._generator()
        u = rng.random(B)
        mi = rng.integers(0, len(self.modes), size=B)
        partner = rng.integers(0, B, size=B)
        fb = rng.integers(0, 2, size=B)
        sy, sx = rng.uniform(-1.0, 1.0, size=B), rng.uniform(-1.0, 1.0, size=B)
        a = rng.uniform(*self.box_area, size=B)
        e = rng.uniform(-1.0, 1.0, size=B)
        bh = np.clip(np.rint(np.sqrt(a * H * W * 2.0 ** e)), 1, H).astype(np.int64)
        bw = np.clip(np.rint(np.sqrt(a * H * W / 2.0 ** e)), 1, W).astype(np.int64)
        y0 = rng.integers(0, H - bh + 1)
        x0 = rng.integers(0, W - bw + 1)
        seed = rng.integers(0, 1 << 64, size=B, dtype=np.uint64)
        mode = np.where(u < self.p, np.asarray(self.modes, dtype=np.int64)[mi], NONE)
        shift = np.where(mode == OBJECT, self.max_shift, 0.0)
        dy, dx = np.rint(sy * shift * H).astype(np.int64), np.rint(sx * shift * W).astype(np.int64)
        flip = fb if self.flip else np.zeros(B, dtype=np.int64)
        box = np.where((mode == BOX)[:, None], np.stack([y0, x0, y0 + bh, x0 + bw], axis=1), 0)
        return [MixPlan(*row[:5], tuple(row[5:]), s) for row, s in
                zip(np.column_stack([mode, partner, flip, dy, dx, box]).tolist(), seed.tolist())]

    # ------------------------------------------------------------------------------------------------ checks
    def _check(self, X, y, plans, out):
        if not isinstance(X, torch.Tensor) or not isinstance(y, torch.Tensor):
            raise TypeError(f"Mixer: X and y are tensors, got {type(X).__name__} and {type(y).__name__}")
        if X.dtype not in _IMAGE_DTYPES or X.ndim != 4:
            raise ValueError(f"X: float32 / bfloat16 / float16 [B,C,H,W] or uint8 [B,H,W,C], got {X.dtype} {tuple(X.shape)}")
        if X.dtype == torch.uint8:
            B, H, W, C = X.shape
        else:
            B, C, H, W = X.shape
        if not 1 <= C <= 4:
            raise ValueError(f"X: 1..4 channels, got {C} ({tuple(X.shape)})")
        if not 1 <= B <= 65535:
            raise ValueError(f"a batch of {B} samples (1..65535)")
        if H < 1 or W < 1 or H * W > MAX_PIXELS:
            raise ValueError(f"X: images of {H} x {W} (at least 1 x 1, at most 2^28 pixels)")
        if y.dtype not in _LABEL_DTYPES or tuple(y.shape) not in ((B, 1, H, W), (B, H, W)):
            raise ValueError(f"y: int64 or uint8 [{B},1,{H},{W}] or [{B},{H},{W}], got {y.dtype} {tuple(y.shape)}")
        if not isinstance(plans, (list, tuple)) or len(plans) != B:
            raise ValueError(f"plans: a list of {B} MixPlans")
        table, seeds = _plan_table(plans, B, H, W)
        if self.seam_value is not None and y.dtype == torch.uint8 and not 0 <= self.seam_value <= 255:
            raise ValueError(f"seam_value {self.seam_value} does not fit uint8 labels")
        ops._require_cuda(X, "Mixer: X")
        ops._require_cuda(y, "Mixer: y")
        if y.device != X.device:
            raise ValueError(f"y is on {y.device}, X on {X.device}")
        if not X.is_contiguous() or not y.is_contiguous():
            raise ValueError("Mixer: X and y must be contiguous (a strided view would be copied behind the caller's back)")
        if out is not None:
            if not isinstance(out, (list, tuple)) or len(out) != 3 or not all(isinstance(t, torch.Tensor) for t in out):
                raise ValueError("out: None or (X_out, y_out, pasted) tensors")
            Xo, yo, pasted = out
            if Xo.dtype != X.dtype or Xo.shape != X.shape or yo.dtype != y.dtype or yo.shape != y.shape:
                raise ValueError("out: X_out and y_out have the shapes and dtypes of X and y")
            if pasted.dtype != torch.int32 or tuple(pasted.shape) != (B,):
                raise ValueError(f"out: pasted is int32 [{B}], got {pasted.dtype} {tuple(pasted.shape)}")
            if any(t.device != X.device for t in out) or not all(t.is_contiguous() for t in out):
                raise ValueError("out: contiguous tensors on the device of X")
            # partners are read while outputs are written
            if any(_overlaps(o, i) for o in out for i in (X, y)):
                raise ValueError("out: an output overlaps an input in memory (partners are read while outputs are written)")
            if _overlaps(Xo, yo) or _overlaps(Xo, pasted) or _overlaps(yo, pasted):
                raise ValueError("out: the outputs overlap each other in memory")
        return B, C, H, W, table, seeds

    # ------------------------------------------------------------------------------------------------ launches
    def apply(self, X, y, plans, out=None):
        """-> (X', y'): fresh tensors of the inputs' shapes and dtypes, or the tensors of out=(X_out, y_out, pasted).  The
        inputs are not modified; self.last["pasted"] is int32 [B] on the device."""
        B, C, H, W, table, seeds = self._check(X, y, plans, out)
        dev = X.device
        eb, lb = _IMAGE_DTYPES[X.dtype], _LABEL_DTYPES[y.dtype]
        cap = self.max_components
        desc = np.zeros(B, dtype=DESC)
        desc["seed"] = seeds
        for j, name in enumerate(("mode", "partner", "flip", "dy", "dx", "y0", "x0", "y1", "x1")):
            desc[name] = table[:, j]
        slots = {}                                           # partner -> slot, in order of appearance
        for k in np.flatnonzero(table[:, 0] == OBJECT).tolist():
            desc[k]["slot"] = slots.setdefault(int(table[k, 1]), len(slots))
        S = len(slots)
        owners = np.zeros(S, dtype=DESC)
        for partner, slot in slots.items():
            owners[slot]["mode"], owners[slot]["partner"], owners[slot]["slot"] = OBJECT, partner, slot
        selects = bool(((table[:, 0] == CLASS) | (table[:, 0] == OBJECT)).any())
        stride = max(256, cap) if S else 256
        seam = self.seam_value
        launches = []
        with torch.cuda.device(dev):
            s = ops._stream()
            u8, i32 = dict(dtype=torch.uint8, device=dev), dict(dtype=torch.int32, device=dev)
            buf, (p_desc, p_owner, p_excl) = _upload([desc, owners, self._exclude], dev)
            if out is None:
                Xo, yo, pasted = torch.empty_like(X), torch.empty_like(y), torch.zeros((B,), **i32)
            else:
                Xo, yo, pasted = out
                pasted.zero_()
            select = torch.empty((B, stride), **u8)
            ids = rows = None
            keep = [buf, select]                             # what the launches point into
            if S:
                ids = torch.empty((S, H, W), **i32)
                rows = torch.empty((S, 4 + 2 * cap), **i32)
                box, first = torch.empty((cap, 4), **i32), torch.empty((cap,), **i32)
                ws = torch.empty((ws_ints(H, W),), **i32)
                keep += [ids, rows, box, first, ws]
                if lb == 8:
                    bytes_ = torch.empty((S, H, W), **u8)
                    keep.append(bytes_)
                    launches.append(("segk_mix_select", (p_owner, S, B, y.data_ptr(), lb, H, W, 0, 0, 0, S, 0, 0, 0, 1, cap,
                                                         bytes_.data_ptr(), 0, stride, _lib.MIX_STAGE_BYTES, s)))
                for partner, slot in slots.items():
                    mask = bytes_[slot].data_ptr() if lb == 8 else y.data_ptr() + partner * H * W
                    r = rows[slot]
                    launches.append(("segk_cc_label", (mask, ids[slot].data_ptr(), r.data_ptr(), r[4:].data_ptr(), r[4 + cap:].data_ptr(),
                                                       box.data_ptr(), first.data_ptr(), ws.data_ptr(), H, W, self.connectivity,
                                                       self._things, cap, s)))
            if selects:
                launches.append(("segk_mix_select", (p_desc, B, B, y.data_ptr(), lb, H, W, p_excl, self.n_classes, ops._p(rows), S,
                                                     self._things, self.min_area, self.max_area, self.max_objects, cap, 0,
                                                     select.data_ptr(), stride, _lib.MIX_STAGE_SELECT, s)))
            launches.append(("segk_mix_apply", (p_desc, B, X.data_ptr(), y.data_ptr(), Xo.data_ptr(), yo.data_ptr(), pasted.data_ptr(),
                                                C, H, W, eb, lb, select.data_ptr(), stride, ops._p(ids), S, cap,
                                                0 if seam is None else 1, 0 if seam is None else seam, s)))
            for name, args in launches:
                _lib.call(name, *args)
        # of the last batch (tools/kbench.py replays the launches; valid while the batch's inputs and outputs are alive)
        self.last = {"pasted": pasted, "plans": list(plans), "launches": launches, "tables": keep}
        return Xo, yo

    def __call__(self, X, y):
        if not isinstance(X, torch.Tensor) or X.ndim != 4:
            raise ValueError("Mixer: X is a [B,C,H,W] or uint8 [B,H,W,C] tensor")
        B = X.shape[0]
        H, W = (X.shape[1], X.shape[2]) if X.dtype == torch.uint8 else (X.shape[2], X.shape[3])
        return self.apply(X, y, self.plan(B, H, W))


class MixedBatches:
    """Iterable over mixed (X, y) batches made from any iterable of (X, y) batches on the device -- AugmentedBatches, or
    images with a teacher's pseudo-labels as y (ClassMix for the unlabelled route) -- and a Mixer: what train_loop, start and
    train_loop_distill take as their `dataloader`."""

    def __init__(self, batches, mixer):
        self.batches, self.mixer = batches, mixer

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for X, y in self.batches:
            yield self.mixer(X, y)
