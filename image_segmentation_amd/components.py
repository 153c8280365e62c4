"""Mask clean-up on the device: connected components of a class mask with their class, area, box and
first pixel, and removal of small / non-largest components by a one-pass neighbour vote -- what a
`mask.cpu()` + `scipy.ndimage.label` post-process does on the host, without leaving the device or synchronising.

    comps = components(pred.mask, min_area=20, keep_largest=(1, 2))
    comps.mask                                   # the cleaned uint8 mask
    k = comps.n                                  # synchronises: the number of components
    comps.box[:k][comps.kept[:k] == 1]           # (y0, x0, y1, x1) of the components that stayed

The kernels are csrc/components.hip (segk_cc_label, segk_cc_clean, segk_mask_finish); there is no CPU path."""
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from . import _lib, ops


def ws_ints(H, W):
    """32-bit words of workspace segk_cc_label / segk_cc_clean need (SEGK_CC_WS_INTS of include/segk.h)"""
    return 16 + 11 * H * W + 2 * H


def _class_mask(classes, what):
    if classes is None:
        return (1 << _lib.MAX_CLASSES) - 1
    if isinstance(classes, (bool, int)) or isinstance(classes, (str, bytes)):
        raise ValueError(f"{what}: expected an iterable of classes, got {classes!r}")
    bits = 0
    for c in classes:
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < _lib.MAX_CLASSES:
            raise ValueError(f"{what}: classes are integers in 0..{_lib.MAX_CLASSES - 1}, got {c!r}")
        bits |= 1 << int(c)
    return bits


@dataclass(frozen=True)
class Clean:
    """The clean-up a Segmenter applies to every mask: the keywords of components()."""
    connectivity: int = 4
    classes: Optional[Tuple[int, ...]] = None
    min_area: int = 0
    keep_largest: Union[bool, Tuple[int, ...]] = False
    max_components: int = 1024

    def __post_init__(self):
        _check_args(self.connectivity, self.classes, self.min_area, self.keep_largest, self.max_components)


def _check_args(connectivity, classes, min_area, keep_largest, max_components):
    """-> (class_mask, keep_mask) after the argument checks (all before any launch)"""
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity: 4 or 8, got {connectivity!r}")
    cmask = _class_mask(classes, "classes")
    if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 0:
        raise ValueError(f"min_area: a non-negative integer, got {min_area!r}")
    if isinstance(max_components, bool) or int(max_components) != max_components or not 1 <= max_components <= 1 << 24:
        raise ValueError(f"max_components: an integer in 1..2^24, got {max_components!r}")
    if keep_largest is False or keep_largest is None:
        kmask = 0
    elif keep_largest is True:
        kmask = cmask
    else:
        kmask = _class_mask(keep_largest, "keep_largest") & cmask
    return cmask, kmask


def as_clean(clean):
    """None, a Clean or a dict of its keywords -> None or a Clean"""
    if clean is None or isinstance(clean, Clean):
        return clean
    if isinstance(clean, dict):
        return Clean(**clean)
    raise ValueError(f"clean: None, a dict or a Clean, got {type(clean).__name__}")


@dataclass
class Components:
    labels: torch.Tensor        # int32 [H,W]: 0 unlabelled, else the id 1..K (every id, also past max_components)
    num: torch.Tensor           # int32 [1] on the device: K
    cls: torch.Tensor           # int32 [cap]   class of component id = row + 1; rows at and past min(K, cap) are zero
    area: torch.Tensor          # int32 [cap]
    box: torch.Tensor           # int32 [cap,4] (y0, x0, y1, x1), y1 and x1 exclusive
    first: torch.Tensor         # int32 [cap]   smallest linear index y*W + x of the component
    kept: torch.Tensor          # int32 [cap]   1 where the component stayed
    new_cls: torch.Tensor       # int32 [cap]   the class its pixels have in `mask`
    mask: torch.Tensor          # uint8 [H,W]   the cleaned mask (equal to the input when nothing was removed)

    @property
    def n(self):
        """K, on the host (synchronises)"""
        return int(self.num.item())


def _check_mask(mask, what="components"):
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{what}: expected a uint8 [H,W] tensor, got {type(mask).__name__}")
    ops._require_cuda(mask, what)
    if mask.dtype != torch.uint8 or mask.ndim != 2 or mask.shape[0] < 1 or mask.shape[1] < 1:
        raise ValueError(f"{what}: expected a uint8 [H,W] mask, got {mask.dtype} {tuple(mask.shape)}")
    if mask.shape[0] * mask.shape[1] > 1 << 28:
        raise ValueError(f"{what}: {tuple(mask.shape)} has more than 2^28 pixels")
    return mask.contiguous()


def components(mask, connectivity=4, classes=None, min_area=0, keep_largest=False, max_components=1024):
    """Label the connected components of a uint8 [H,W] class mask on its device and clean it.

    connectivity    4 or 8
    classes         the classes that are labelled (default: all of 0..7); other pixels get id 0 and never change
    min_area        components smaller than this are removed
    keep_largest    False, True (every labelled class) or an iterable of classes: of each such class only the largest
                    component stays (a tie goes to the lowest id)
    max_components  rows of the per-component arrays; components past it are still labelled and cleaned, num > rows tells

    A removed component takes the class most of its standing 4-neighbours have.  Nothing synchronises with the host and
    the input is not modified."""
    cmask, kmask = _check_args(connectivity, classes, min_area, keep_largest, max_components)
    mask = _check_mask(mask)
    H, W = mask.shape
    cap, dev = int(max_components), mask.device
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        labels = torch.empty((H, W), **i32)
        rows = torch.empty((5, cap), **i32)          # cls, area, first, kept, new_cls
        box = torch.empty((cap, 4), **i32)
        num = torch.empty((1,), **i32)
        ws = torch.empty((ws_ints(H, W),), **i32)
        out = torch.empty_like(mask)
        s = ops._stream()
        _lib.call("segk_cc_label", mask.data_ptr(), labels.data_ptr(), num.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(),
                  box.data_ptr(), rows[2].data_ptr(), ws.data_ptr(), H, W, int(connectivity), cmask, cap, s)
        _lib.call("segk_cc_clean", mask.data_ptr(), out.data_ptr(), ws.data_ptr(), rows[3].data_ptr(), rows[4].data_ptr(), H, W,
                  int(min(min_area, 1 << 30)), kmask, cap, s)
    return Components(labels, num, rows[0], rows[1], box, rows[2], rows[3], rows[4], out)


def mask_finish(mask, num_classes, palette=None, labels=None):
    """color uint8 [H,W,3] (None without a palette), counts int64 [8] and confusion int64 [8,8] (None without labels) of a
    finished uint8 [H,W] mask: the same outputs segk_predict_mask derives from its argmax.  palette: a uint8 [K,3] tensor
    on the mask's device; labels: int64 [H,W] there."""
    mask = _check_mask(mask, "mask_finish")
    H, W = mask.shape
    dev = mask.device
    if mask.data_ptr() % 4:
        mask = mask.clone()
    with torch.cuda.device(dev):
        color = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if palette is not None else None
        counts = torch.zeros((_lib.MAX_CLASSES,), dtype=torch.int64, device=dev)
        M = torch.zeros((_lib.MAX_CLASSES, _lib.MAX_CLASSES), dtype=torch.int64, device=dev) if labels is not None else None
        _lib.call("segk_mask_finish", mask.data_ptr(), ops._p(color), ops._p(palette), counts.data_ptr(), ops._p(labels), ops._p(M),
                  int(num_classes), H, W, ops._stream())
    return color, counts, M
