"""Per-pixel segmentation losses on the fused HIP loss kernel -- drop-in for the reference's
utils/weighted_loss.py:6-98 (WeightedMemoryEfficientDiceLoss), :102-166 (WeightedDiceCELoss), :170-265
(WeightedMemoryEfficientDiceLossPrompt), :268-343 (WeightedDiceNLLLoss) and for torch.nn.CrossEntropyLoss as the reference constructs it (unet/unet.ipynb cell 0; weighted_loss.py:132-138);
MSELoss replaces torch.nn.MSELoss of the autoencoder pretraining (autoencoder/autoencoder.ipynb cell 0) on its own kernels.
Constructor signatures, accepted target shapes and error behaviour follow the reference."""
from typing import Callable, Optional

import torch
from torch import nn

from . import ops


def _check_targets(outputs, targets):
    # weighted_loss.py:141-161 -- [N,H,W] or [N,1,H,W] class indices
    if targets.ndim == 3 or (targets.ndim == 4 and targets.shape[1] == 1):
        return
    if targets.ndim == outputs.ndim and targets.shape[1] != 1:
        raise ValueError(f"Target shape {targets.shape} has multiple channels but expected class indices "
                         f"[N, H, W] or [N, 1, H, W] for CE.")
    raise ValueError(f"Unsupported target shape {targets.shape} for CE. Expected [N, H, W] or [N, 1, H, W].")


def _check_smoothing(label_smoothing):
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing}")
    return eps


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=None, ignore_index=-100, reduction='mean', label_smoothing=0.0) for [N,C,H,W] logits.
    label_smoothing == 0 is the fused CrossEntropy + Dice kernel's path; a non-zero value runs on the hard-pixel loss kernels."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -100, reduction: str = "mean",
                 label_smoothing: float = 0.0):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (the reference's setting) is implemented")
        self.weight = weight
        self.ignore_index = ignore_index
        self.label_smoothing = _check_smoothing(label_smoothing)

    def forward(self, outputs, targets):
        ign = self.ignore_index if self.ignore_index is not None and self.ignore_index >= 0 else None
        if self.label_smoothing != 0.0:
            return ops.HardLossFn.apply(outputs, targets, self.weight, ign, self.label_smoothing, 0.0, None)[0]
        return ops.SegLossFn.apply(outputs, targets, self.weight, ign, 0.0, 0.0, 1.0)


class HardPixelLoss(nn.Module):
    """Class-weighted CrossEntropy that can also weight PIXELS, mean over the kept pixels:
      label_smoothing  eps in [0, 1): nn.CrossEntropyLoss's smoothing;
      gamma            0 or in [1, 8]: the focal modulation (1 - p_t)^gamma on each pixel's loss;
      thresh, min_kept, min_fraction   bootstrapped / OHEM selection: keep the pixels whose CrossEntropy (unweighted,
                       unsmoothed) is at least -log(thresh), and at least the max(min_kept, ceil(min_fraction * n)) hardest of
                       the n labelled pixels of the batch (ties at the last one all kept).  All three at their defaults: every
                       labelled pixel.
    The selection is an exact k-th largest on the device: no sort, no per-pixel float tensor, no host sync; under
    DistributedDataParallel every rank selects over its own batch.  After a call `.last` holds device tensors (no sync):
    "n" (labelled pixels) and "n_kept" as int32, "threshold" (the smallest kept CrossEntropy allowed) as float32.
    Targets [N,H,W] or [N,1,H,W] class indices."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: Optional[int] = -100, label_smoothing: float = 0.0,
                 gamma: float = 0.0, thresh: Optional[float] = None, min_kept: int = 0, min_fraction: float = 0.0):
        super().__init__()
        self.weight = weight
        self.ignore_index = ignore_index
        self.label_smoothing = _check_smoothing(label_smoothing)
        self.gamma = float(gamma)
        if not (self.gamma == 0.0 or 1.0 <= self.gamma <= 8.0):
            raise ValueError(f"gamma must be 0 or lie in [1, 8], got {gamma}")
        if thresh is not None and not 0.0 < float(thresh) <= 1.0:
            raise ValueError(f"thresh must lie in (0, 1], got {thresh}")
        if int(min_kept) != min_kept or min_kept < 0 or min_kept >= 2 ** 31:
            raise ValueError(f"min_kept must be a non-negative integer, got {min_kept}")
        if not 0.0 <= float(min_fraction) <= 1.0:
            raise ValueError(f"min_fraction must lie in [0, 1], got {min_fraction}")
        self.thresh = None if thresh is None else float(thresh)
        self.min_kept = int(min_kept)
        self.min_fraction = float(min_fraction)
        self.last = {}

    def selection(self):
        """None when every labelled pixel is kept, else (theta, min_kept, q16) as segk_hard_loss_fwd takes them: theta =
        -log(thresh) in float64, rounded once to fp32 by the call; q16 = round(min_fraction * 2^16)."""
        if self.thresh is None and self.min_kept == 0 and self.min_fraction == 0.0:
            return None
        import math
        theta = math.inf if self.thresh is None else -math.log(self.thresh) + 0.0
        return theta, self.min_kept, int(round(self.min_fraction * 65536.0))

    def forward(self, outputs, targets):
        _check_targets(outputs, targets)
        ign = self.ignore_index if self.ignore_index is not None and self.ignore_index >= 0 else None
        loss, state = ops.HardLossFn.apply(outputs, targets, self.weight, ign, self.label_smoothing, self.gamma, self.selection())
        counts = state[6:8].view(torch.int32)
        self.last = {"n": counts[0], "n_kept": counts[1], "threshold": state[4]}
        return loss


class FocalLoss(HardPixelLoss):
    """Focal loss (Lin et al. 2017) on [N,C,H,W] logits: mean of (1 - p_t)^gamma * CrossEntropy over the labelled pixels."""

    def __init__(self, gamma: float = 2.0, weight: Optional[torch.Tensor] = None, ignore_index: Optional[int] = -100,
                 label_smoothing: float = 0.0):
        super().__init__(weight=weight, ignore_index=ignore_index, label_smoothing=label_smoothing, gamma=gamma)


class OhemCrossEntropyLoss(HardPixelLoss):
    """Bootstrapped (online hard example mining) CrossEntropy: the mean over the pixels the model gets wrong (probability of
    the label below `thresh`), and at least the max(min_kept, ceil(min_fraction * n)) hardest."""

    def __init__(self, thresh: Optional[float] = 0.7, min_kept: int = 0, min_fraction: float = 0.0,
                 weight: Optional[torch.Tensor] = None, ignore_index: Optional[int] = -100, label_smoothing: float = 0.0):
        super().__init__(weight=weight, ignore_index=ignore_index, label_smoothing=label_smoothing, thresh=thresh,
                         min_kept=min_kept, min_fraction=min_fraction)


def _check_lovasz_weight(weight):
    """class weights of the Lovasz term: finite and non-negative (a zero takes the class out); checked where the host can see
    them, on CPU tensors and sequences -- a device tensor is taken as it is, reading it would be a sync"""
    if weight is None or (isinstance(weight, torch.Tensor) and weight.is_cuda):
        return
    w = torch.as_tensor(weight, dtype=torch.float64)
    if w.dim() != 1 or w.numel() == 0:
        raise ValueError(f"weight must be a vector of class weights, got shape {tuple(w.shape)}")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("weight must be finite and non-negative")


class LovaszSoftmaxLoss(nn.Module):
    """Lovasz-Softmax loss (Berman, Triki, Blaschko 2018), the convex surrogate of mean IoU, on [N,C,H,W]
    logits: per class the pixel errors (1 - p_c where the label is c, p_c elsewhere) sorted descending on the device and
    weighted by the gradient of the Jaccard index along that order; the weighted mean over the classes that enter, then over
    the segments.
      per_image   one sort per image and the mean over the images (images without a labelled pixel stay in the divisor)
                  instead of one sort over the batch;
      classes     "present": the classes with a labelled pixel in the segment; "all": every class;
      weight      class weights of that mean (1 when absent; a zero takes the class out).
    No labelled pixel at all: exactly 0 with a zero gradient (not CrossEntropy's NaN).  Only reduction 'mean' exists; under
    DistributedDataParallel every rank sorts its own batch.  After a call `.last` holds device tensors (no sync): "n" (labelled
    pixels, float64), "present" (int32 [S,C], the classes that entered) and "per_class" (float64 [S,C], the class terms), S = N
    with per_image, else 1.  Targets [N,H,W] or [N,1,H,W] class indices."""

    def __init__(self, per_image: bool = False, classes: str = "present", weight: Optional[torch.Tensor] = None,
                 ignore_index: Optional[int] = None):
        super().__init__()
        if classes not in ("present", "all"):
            raise ValueError(f"classes must be 'present' or 'all', got {classes!r}")
        _check_lovasz_weight(weight)
        self.per_image = bool(per_image)
        self.classes = classes
        self.weight = weight
        self.ignore_index = ignore_index
        self.last = {}

    def forward(self, outputs, targets):
        _check_targets(outputs, targets)
        if self.weight is not None and outputs.dim() == 4 and len(self.weight) != outputs.shape[1]:
            raise ValueError(f"weight has {len(self.weight)} entries, the logits {outputs.shape[1]} classes")
        ign = self.ignore_index if self.ignore_index is not None and self.ignore_index >= 0 else None
        loss, state = ops.LovaszFn.apply(outputs, targets, self.weight, ign, self.per_image, self.classes == "all")
        N, C = outputs.shape[0], outputs.shape[1]
        S = N if self.per_image else 1
        Q = S * C
        self.last = {"n": state[1], "present": state[2 + 3 * Q:2 + 4 * Q].view(S, C).to(torch.int32),
                     "per_class": state[2:2 + Q].view(S, C)}
        return loss


class LovaszCELoss(nn.Module):
    """lovasz_weight * LovaszSoftmaxLoss + ce_weight * CrossEntropyLoss on the same logits, the form the Lovasz term is
    trained in.  class_weights and ignore_index go to both terms; ce_kwargs may hold label_smoothing.  A term whose weight is 0
    launches nothing."""

    def __init__(self, lovasz_weight: float = 1.0, ce_weight: float = 1.0, class_weights: Optional[torch.Tensor] = None,
                 ignore_index: Optional[int] = None, per_image: bool = False, classes: str = "present", ce_kwargs=None):
        super().__init__()
        ce_kwargs = dict(ce_kwargs or {})
        if set(ce_kwargs) - {"label_smoothing"}:
            raise NotImplementedError("extra nn.CrossEntropyLoss kwargs are not supported by the fused kernel "
                                      "(label_smoothing is the one that is)")
        self.lovasz_weight = float(lovasz_weight)
        self.ce_weight = float(ce_weight)
        if self.lovasz_weight == 0.0 and self.ce_weight == 0.0:
            raise ValueError("lovasz_weight and ce_weight are both 0: nothing to compute")
        self.lovasz = LovaszSoftmaxLoss(per_image=per_image, classes=classes, weight=class_weights, ignore_index=ignore_index)
        self.ce = CrossEntropyLoss(weight=class_weights, ignore_index=-100 if ignore_index is None else ignore_index,
                                   label_smoothing=ce_kwargs.get("label_smoothing", 0.0))

    @property
    def last(self):
        return self.lovasz.last

    def forward(self, outputs, targets):
        _check_targets(outputs, targets)
        total = None
        for weight, term in ((self.lovasz_weight, self.lovasz), (self.ce_weight, self.ce)):
            if weight == 0.0:
                continue
            value = term(outputs, targets)
            value = value if weight == 1.0 else weight * value      # a weight of 1 hands the term's own buffer on
            total = value if total is None else total + value
        return total


class MSELoss(nn.Module):
    """nn.MSELoss(size_average=None, reduce=None, reduction='mean') for two same-shaped tensors (the reconstruction and its
    input, utils/training.py:141,234).  'mean' and 'sum' run on the deterministic HIP reduction; 'none' and the legacy
    size_average / reduce flags are not implemented."""

    def __init__(self, size_average=None, reduce=None, reduction: str = "mean"):
        super().__init__()
        if size_average is not None or reduce is not None:
            raise NotImplementedError("the deprecated size_average / reduce arguments are not supported: use reduction=")
        if reduction == "none":
            raise NotImplementedError("reduction='none' is not implemented (the reference uses 'mean')")
        if reduction not in ("mean", "sum"):
            raise ValueError(f"{reduction} is not a valid value for reduction")
        self.reduction = reduction

    def forward(self, input, target):
        return ops.MSELossFn.apply(input, target, self.reduction == "mean")


class WeightedMemoryEfficientDiceLoss(nn.Module):
    def __init__(self, apply_softmax: bool = True, ignore_index: Optional[int] = None,
                 class_weights: Optional[torch.Tensor] = None, smooth: float = 1e-5):
        super().__init__()
        if not apply_softmax:
            raise NotImplementedError("apply_softmax=False: use WeightedMemoryEfficientDiceLossPrompt (weighted_loss.py:170)")
        self.apply_softmax = apply_softmax
        self.ignore_index = ignore_index
        self.smooth = smooth
        self.class_weights = class_weights

    def forward(self, x, y):
        # weighted_loss.py:41-46: only [N,1,H,W] targets pass the reference's shape check
        if not (y.ndim == x.ndim and y.shape[1] == 1):
            raise ValueError(f"Shape mismatch: probs {x.shape}, y {y.shape}")
        return ops.SegLossFn.apply(x, y, self.class_weights, self.ignore_index, self.smooth, 1.0, 0.0)


class WeightedDiceCELoss(nn.Module):
    def __init__(self, dice_weight: float = 1.0, ce_weight: float = 1.0, ignore_index: Optional[int] = None,
                 class_weights: Optional[torch.Tensor] = None, smooth_dice: float = 1e-5, ce_kwargs={}):
        super().__init__()
        if set(ce_kwargs) - {"label_smoothing"}:
            raise NotImplementedError("extra nn.CrossEntropyLoss kwargs are not supported by the fused kernel "
                                      "(label_smoothing is the one that is)")
        self.label_smoothing = _check_smoothing(ce_kwargs.get("label_smoothing", 0.0))
        self.dice_weight = dice_weight
        self.ce_weight = ce_weight
        self.ignore_index = ignore_index
        self.class_weights = class_weights
        self.smooth_dice = smooth_dice

    def forward(self, outputs, targets):
        _check_targets(outputs, targets)
        if self.label_smoothing != 0.0:      # Dice alone on the fused kernel, the smoothed CrossEntropy on the hard-pixel kernels
            dice = ops.SegLossFn.apply(outputs, targets, self.class_weights, self.ignore_index, self.smooth_dice, 1.0, 0.0)
            ce = ops.HardLossFn.apply(outputs, targets, self.class_weights, self.ignore_index, self.label_smoothing, 0.0, None)[0]
            return self.dice_weight * dice + self.ce_weight * ce
        return ops.SegLossFn.apply(outputs, targets, self.class_weights, self.ignore_index, self.smooth_dice,
                                   self.dice_weight, self.ce_weight)


def _log_eps(fn):
    """Map an `nll_nonlin` callable onto the kernel's NLL input: None -> (0, 0.0) (NLL of the values themselves);
    x -> log(x + eps) -> (1, eps), recognised by probing the callable (prompt.ipynb: `lambda x: torch.log(x + 1e-9)`)."""
    if fn is None:
        return 0, 0.0
    with torch.no_grad():
        x = torch.tensor([0.0, 0.25, 1.0], dtype=torch.float64)
        y = fn(x)
        eps = float(torch.exp(y[0]))
        ok = bool(torch.isfinite(y[1:]).all()) and torch.allclose(y[1:], torch.log(x[1:] + eps), rtol=1e-9, atol=1e-12)
        if eps > 0 and not torch.isfinite(y[0]):
            ok = False
    if not ok or eps < 0 or eps > 1e-2:
        raise NotImplementedError("nll_nonlin must be None or x -> log(x + eps): other non-linearities have no HIP kernel")
    return 1, eps


class WeightedMemoryEfficientDiceLossPrompt(nn.Module):
    def __init__(self, dice_nonlin: Callable = None, apply_softmax: bool = True, ignore_index: Optional[int] = None,
                 class_weights: Optional[torch.Tensor] = None, smooth: float = 1e-5):
        super().__init__()
        if dice_nonlin is not None:
            raise NotImplementedError("dice_nonlin has no HIP kernel (the reference never sets it)")
        self.apply_softmax = apply_softmax
        self.ignore_index = ignore_index
        self.smooth = smooth
        self.dice_nonlin = dice_nonlin
        if class_weights is not None:
            assert isinstance(class_weights, torch.Tensor), "class_weights must be a torch.Tensor"
        self.class_weights = class_weights

    def forward(self, x, y):
        # weighted_loss.py:213-217: only [N,1,H,W] passes (the [N,H,W] branch compares y.shape with probs.shape[2:],
        # which can never match, so the reference raises for it)
        if y.ndim != x.ndim:
            raise ValueError(f"Shape mismatch: probs {x.shape}, y {y.shape}")
        elif y.shape[1] != 1:
            raise NotImplementedError("one-hot targets are not supported by the fused kernel")
        if self.apply_softmax:
            return ops.SegLossFn.apply(x, y, self.class_weights, self.ignore_index, self.smooth, 1.0, 0.0)
        return ops.ProbLossFn.apply(x, y, self.class_weights, self.ignore_index, self.smooth, 1.0, 0.0, 0, 0.0)


class WeightedDiceNLLLoss(nn.Module):
    def __init__(self, dice_weight: float = 1.0, nll_weight: float = 1.0, ignore_index: Optional[int] = None,
                 class_weights: Optional[torch.Tensor] = None, smooth_dice: float = 1e-5, apply_softmax: bool = True,
                 dice_nonlin: Callable = None, nll_nonlin: Callable = None, nll_kwargs={}):
        super().__init__()
        if nll_kwargs:
            raise NotImplementedError("extra nn.NLLLoss kwargs are not supported by the fused kernel")
        # like the reference (weighted_loss.py:296-301) dice_nonlin is stored but never reaches the Dice term
        self.dice_weight = dice_weight
        self.nll_weight = nll_weight
        self.ignore_index = ignore_index
        self.class_weights = class_weights
        self.smooth_dice = smooth_dice
        self.apply_softmax = apply_softmax
        self.dice_nonlin = dice_nonlin
        self.nll_nonlin = nll_nonlin
        self._nll_log, self._eps = _log_eps(nll_nonlin)

    def forward(self, outputs, targets):
        _check_targets(outputs, targets)
        if not self.apply_softmax:      # one pass: Dice and NLL of the same probabilities
            return ops.ProbLossFn.apply(outputs, targets, self.class_weights, self.ignore_index, self.smooth_dice,
                                        self.dice_weight, self.nll_weight, self._nll_log, self._eps)
        # reference default: Dice of softmax(outputs) + NLL of nll_nonlin(outputs)
        dice = ops.SegLossFn.apply(outputs, targets, self.class_weights, self.ignore_index, self.smooth_dice, 1.0, 0.0)
        nll = ops.ProbLossFn.apply(outputs, targets, self.class_weights, self.ignore_index, self.smooth_dice, 0.0, 1.0,
                                   self._nll_log, self._eps)
        return self.dice_weight * dice + self.nll_weight * nll
