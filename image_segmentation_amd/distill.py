"""Distillation: frozen teachers, their views, and the soft-target loss on the fused HIP kernel (the reference
holds no code for it).

    teacher = Teacher([clip_unet, big_unet], flips=("", "h"))         # four views: models-major, then flips
    loss_fn = DistillLoss(hard=CrossEntropyLoss(), alpha=0.7, temperature=2.0)
    train_loop_distill(loader, student, teacher, loss_fn, optimizer, 1, device)

A VIEW is one teacher output for the batch, possibly computed on the flipped batch: the kernel reads it through the flip, so
nothing is flipped back and no probability tensor is ever stored.  teacher_table builds the device kernel's descriptor table on
the host and refuses what the kernel itself cannot check (the table lives in device memory)."""
import inspect
import math

import numpy as np
import torch
from torch import nn

from . import ops
from .tta import FLIPS, KINDS, MAX_VIEWS

# segk_teacher_desc of include/segk.h
TEACHER_DESC = np.dtype([("ptr", "<u8"), ("flip", "<i4"), ("kind", "<i4"), ("weight", "<f4"), ("pad_", "<i4", (3,))])
assert TEACHER_DESC.itemsize == 32


def teacher_table(rows):
    """Descriptor table for segk_distill_fwd / segk_distill_bwd: a TEACHER_DESC array, one row per view in the order given
    (the order is part of the result: fp32 sums in view order).  rows: (address, flip, kind, weight) -- flip a key of
    tta.FLIPS or 0..3, kind a key of tta.KINDS or 0 / 1, weight > 0.  The weights are divided by their sum in float64 and
    rounded once to float32, as tta.view_table does."""
    rows = list(rows)
    if not 1 <= len(rows) <= MAX_VIEWS:
        raise ValueError(f"{len(rows)} teacher views: 1..{MAX_VIEWS} supported")
    table = np.zeros(len(rows), dtype=TEACHER_DESC)
    weights = []
    for v, (ptr, flip, kind, w) in enumerate(rows):
        f = FLIPS.get(flip, flip) if isinstance(flip, str) else flip
        k = KINDS.get(kind, kind) if isinstance(kind, str) else kind
        if f not in (0, 1, 2, 3):
            raise ValueError(f"view {v}: unknown flip {flip!r} (one of {tuple(FLIPS)} or 0..3)")
        if k not in (0, 1):
            raise ValueError(f"view {v}: unknown kind {kind!r} (one of {tuple(KINDS)} or 0 / 1)")
        if int(ptr) <= 0 or int(ptr) % 4:
            raise ValueError(f"view {v}: the tensor address must be non-zero and 4-byte aligned")
        if not (float(w) > 0 and math.isfinite(float(w))):
            raise ValueError(f"view {v}: weight must be positive and finite, got {w}")
        weights.append(float(w))
        table[v] = (int(ptr), int(f), int(k), 0.0, (0, 0, 0))
    total = math.fsum(weights)
    table["weight"] = np.asarray([w / total for w in weights], dtype=np.float64).astype(np.float32)
    return table


class TeacherViews:
    """The teachers' outputs for one batch and the device table that names them.  outputs: V tensors [N,C,H,W] (detached,
    converted to contiguous float32); flips / kinds / weights: one entry per view (default: no flip, logits, equal weights).
    A view with flip f holds the network's output for the batch flipped by f -- as computed, not flipped back."""

    def __init__(self, outputs, flips=None, kinds=None, weights=None):
        outputs = [outputs] if isinstance(outputs, torch.Tensor) else list(outputs)
        V = len(outputs)
        if not 1 <= V <= MAX_VIEWS:
            raise ValueError(f"{V} teacher views: 1..{MAX_VIEWS} supported")
        flips = ("",) * V if flips is None else tuple(flips)
        kinds = ("logits",) * V if kinds is None else tuple(kinds)
        weights = (1.0,) * V if weights is None else tuple(weights)
        if not (len(flips) == len(kinds) == len(weights) == V):
            raise ValueError(f"{V} views need {V} flips, kinds and weights, got {len(flips)}, {len(kinds)}, {len(weights)}")
        outs = []
        for v, t in enumerate(outputs):
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise ValueError(f"teacher view {v}: expected a tensor [N,C,H,W]")
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
            if tuple(t.shape) != tuple(outputs[0].shape) or t.device != outputs[0].device:
                raise ValueError(f"teacher view {v}: shape {tuple(t.shape)} on {t.device}, view 0 has {tuple(outputs[0].shape)} "
                                 f"on {outputs[0].device}")
            outs.append(t)
        self.outputs = outs
        self.host_table = teacher_table((t.data_ptr(), f, k, w)
                                        for t, f, k, w in zip(outs, flips, kinds, weights))
        self.table = torch.from_numpy(self.host_table.view(np.uint8).copy()).to(outs[0].device)
        self.flips = tuple(int(f) for f in self.host_table["flip"])
        self.kinds = tuple(int(k) for k in self.host_table["kind"])
        self.weights = tuple(float(w) for w in self.host_table["weight"])

    def __len__(self):
        return len(self.outputs)


def _takes_one_input(model):
    try:
        params = list(inspect.signature(model.forward).parameters.values())
    except (TypeError, ValueError):
        return True
    required = [p for p in params if p.default is inspect.Parameter.empty
                and p.kind in (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)]
    return len(required) <= 1


class Teacher:
    """Frozen teachers for distillation.  models: one nn.Module or a list (an ensemble); flips: the views of each model, keys
    of tta.FLIPS ("" none, "h" x reversed, "v" y reversed, "hv" both); weights: one positive number per (model, flip) view,
    models-major, None for equal weights.  The parameters are frozen here.  Calling it with a batch X [N,Cin,H,W] runs every
    model in eval mode under no_grad on the (flipped) batch, restores every module's previous mode and returns a TeacherViews.
    Models that take a second input (the prompt model) are refused: there is no prompt to give them."""

    def __init__(self, models, flips=("",), weights=None):
        models = [models] if isinstance(models, nn.Module) else list(models)
        if not models or any(not isinstance(m, nn.Module) for m in models):
            raise ValueError("Teacher: one nn.Module or a non-empty list of them")
        for m in models:
            if not _takes_one_input(m):
                raise ValueError(f"Teacher: {type(m).__name__}.forward takes more than one input (a prompt model): "
                                 "only single-input models can teach")
        flips = (flips,) if isinstance(flips, str) else tuple(flips)
        if not flips or any(f not in FLIPS for f in flips) or len(set(flips)) != len(flips):
            raise ValueError(f"flips: distinct entries of {tuple(FLIPS)}, got {flips!r}")
        n = len(models) * len(flips)
        if n > MAX_VIEWS:
            raise ValueError(f"{n} views ({len(models)} models x {len(flips)} flips): at most {MAX_VIEWS}")
        if weights is not None:
            weights = tuple(float(w) for w in weights)
            if len(weights) != n or any(not (w > 0 and math.isfinite(w)) for w in weights):
                raise ValueError(f"weights: {n} positive finite numbers (models-major, then flips), got {weights}")
        for m in models:
            for p in m.parameters():
                p.requires_grad_(False)
        self.models, self.flips, self.weights = models, flips, weights

    def to(self, *args, **kwargs):
        for m in self.models:
            m.to(*args, **kwargs)
        return self

    @torch.no_grad()
    def __call__(self, X):
        outs, fl = [], []
        for m in self.models:
            modes = [(mod, mod.training) for mod in m.modules()]
            m.eval()
            try:
                for f in self.flips:
                    dims = [d for d, bit in ((3, 1), (2, 2)) if FLIPS[f] & bit]
                    out = m(torch.flip(X, dims) if dims else X)
                    if not isinstance(out, torch.Tensor) or out.dim() != 4:
                        raise ValueError(f"Teacher: {type(m).__name__} returned {type(out).__name__}, expected [N,C,H,W]")
                    outs.append(out)
                    fl.append(f)
            finally:
                for mod, was in modes:
                    mod.training = was
        return TeacherViews(outs, flips=fl, weights=self.weights)


class DistillLoss(nn.Module):
    """alpha * soft + (1 - alpha) * hard(outputs, targets).

    soft = T*T * mean over the counted pixels of KL(q || softmax(outputs / T)), q = the weighted mean over the teacher views of
    softmax(view / T); a pixel counts unless its label equals ignore_index (when targets and ignore_index are given) or the
    teachers' untempered confidence max_k q1_k is below min_confidence; no pixel counted: soft = 0 and no gradient.
    hard: any loss module of this package (or None).  With targets None or hard None, alpha must be 1 and no hard term is
    evaluated.  teacher_views: a TeacherViews, or a tensor / list of tensors taken as logits, no flip, equal weights.
    `last` holds soft, hard, n and n_agree of the latest call as device tensors (no synchronisation)."""

    def __init__(self, hard=None, alpha=0.5, temperature=1.0, ignore_index=None, min_confidence=0.0):
        super().__init__()
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
        if not (float(temperature) > 0 and math.isfinite(float(temperature))):
            raise ValueError(f"temperature must be positive and finite, got {temperature}")
        if not math.isfinite(float(min_confidence)):
            raise ValueError(f"min_confidence must be finite, got {min_confidence}")
        self.hard = hard
        self.alpha = float(alpha)
        self.temperature = float(temperature)
        self.ignore_index = ignore_index
        self.min_confidence = float(min_confidence)
        self.last = {}

    def forward(self, outputs, targets, teacher_views):
        with_hard = targets is not None and self.hard is not None
        if not with_hard and self.alpha != 1.0:
            raise ValueError(f"alpha = {self.alpha} needs a hard loss and targets: without either, alpha must be 1")
        views = teacher_views if isinstance(teacher_views, TeacherViews) else TeacherViews(teacher_views)
        labels = None
        if targets is not None and self.ignore_index is not None:
            labels = targets
            if labels.ndim == 4 and labels.shape[1] == 1:
                labels = labels[:, 0]
            if labels.ndim != 3:
                raise ValueError(f"Unsupported target shape {tuple(targets.shape)}: expected [N, H, W] or [N, 1, H, W]")
        soft, state = ops.DistillFn.apply(outputs, views, labels, self.ignore_index, self.temperature, self.min_confidence)
        hard = self.hard(outputs, targets) if with_hard else None
        self.last = {"soft": soft.detach(), "hard": None if hard is None else hard.detach(), "n": state[1], "n_agree": state[3]}
        if not with_hard:
            return soft
        return self.alpha * soft + (1.0 - self.alpha) * hard
