"""Tiled full-resolution prediction: the host side of segk_tile_gather(_u8) / segk_predict_tiles.

The image is cut at its own resolution into size x size tiles that overlap by `overlap` pixels, the tiles run through the
network as batches, and the overlapping outputs are blended into one mask.  The kernels derive the tile plan from (L, T,
overlap) themselves; tile_axis is that arithmetic on the host.  Nothing here touches the GPU."""
from dataclasses import dataclass
from typing import Optional

from .tta import MERGES

WINDOWS = {"flat": 0, "triangle": 1}           # SEGK_TILE_WINDOW_FLAT / SEGK_TILE_WINDOW_TRIANGLE
PADS = {"zero": 0, "reflect": 1}               # SEGK_TILE_PAD_ZERO / SEGK_TILE_PAD_REFLECT
MAX_TILE = 4096                                # window weights below 2^24: exact in fp32


def _check_size_overlap(size, overlap):
    if int(size) != size or not 1 <= int(size) <= MAX_TILE:
        raise ValueError(f"size: an integer in 1..{MAX_TILE}, got {size!r}")
    if int(overlap) != overlap or not 0 <= int(overlap) <= int(size) // 2:
        raise ValueError(f"overlap: an integer in 0..size // 2 = {int(size) // 2}, got {overlap!r}")


@dataclass(frozen=True)
class Tiles:
    """size: the tile side (None: the Segmenter's target_size); overlap: pixels two neighbouring tiles share, at most
    size // 2 (None: size // 4); window: the blend weight of a tile pixel, "flat" (1) or "triangle" (rising by one per pixel
    from the tile's edge, separable); pad: what a tile shows beyond an image smaller than itself, "reflect" or "zero";
    merge: "prob" (probabilities are averaged) or "logit"."""
    size: Optional[int] = None
    overlap: Optional[int] = None
    window: str = "triangle"
    pad: str = "reflect"
    merge: str = "prob"

    def __post_init__(self):
        if self.size is not None:
            _check_size_overlap(self.size, 0)
            object.__setattr__(self, "size", int(self.size))
        if self.overlap is not None:
            if int(self.overlap) != self.overlap or int(self.overlap) < 0:
                raise ValueError(f"overlap: a non-negative integer, got {self.overlap!r}")
            if self.size is not None:
                _check_size_overlap(self.size, self.overlap)
            object.__setattr__(self, "overlap", int(self.overlap))
        if self.window not in WINDOWS:
            raise ValueError(f"window: one of {tuple(WINDOWS)}, got {self.window!r}")
        if self.pad not in PADS:
            raise ValueError(f"pad: one of {tuple(PADS)}, got {self.pad!r}")
        if self.merge not in MERGES:
            raise ValueError(f"merge: one of {tuple(MERGES)}, got {self.merge!r}")

    def resolve(self, target_size):
        """(size, overlap) with target_size standing in for size=None and size // 4 for overlap=None"""
        if self.size is None and target_size is None:
            raise ValueError("size=None stands for the Segmenter's target_size: pass target_size")
        size = int(target_size) if self.size is None else self.size
        overlap = size // 4 if self.overlap is None else self.overlap
        _check_size_overlap(size, overlap)
        return size, overlap


def tile_axis(L, T, overlap):
    """Origins of the tiles of one axis of length L, ascending.  L <= T: one tile at -((T - L) // 2) (the image centred in
    it, the odd pixel after it).  L > T: ceil((L - T) / s) + 1 tiles at min(i s, L - T), s = T - overlap: the last tile is
    pulled back inside the image, so no tile of a long axis sees padding.  Every coordinate is covered by 1..3 tiles."""
    L, T, overlap = int(L), int(T), int(overlap)
    if L < 1:
        raise ValueError(f"an axis of length {L}")
    _check_size_overlap(T, overlap)
    if L <= T:
        return [-((T - L) // 2)]
    s = T - overlap
    n = -(-(L - T) // s) + 1
    return [min(i * s, L - T) for i in range(n)]


def tile_plan(H, W, tiles, target_size=None):
    """(ys, xs): the tile origins of an H x W image; tile t = iy * len(xs) + ix covers rows ys[iy] .. ys[iy] + size - 1"""
    size, overlap = tiles.resolve(target_size)
    return tile_axis(H, size, overlap), tile_axis(W, size, overlap)
