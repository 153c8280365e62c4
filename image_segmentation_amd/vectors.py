"""Mask vectorisation on the device: the column-major run table (COCO's order), the contour rings and the
corner vertices of every connected component of a class mask -- what a `mask.cpu()` + `cv2.findContours` /
`pycocotools.mask.encode` post-process does on the host, without leaving the device or synchronising.

    vec = vectorize(pred.mask, connectivity=4)
    vec.polygons()                               # synchronises: [(object id, twice the signed area, int32 [n,2] (x, y)), ...]
    vec.coco_rle(1)                              # {"size": [H, W], "counts": [...]} of object 1, uncompressed
    vec.to_coco(image_id=7, category_of_class={1: 1, 2: 2})

The kernels are csrc/vectors.hip (segk_vec_runs, segk_vec_rings) on top of segk_cc_label; there is no CPU path.  The host
methods of Vectors only read its arrays, so they also serve a Vectors made of CPU tensors."""
from dataclasses import dataclass, field
from typing import Tuple

import numpy as np
import torch

from . import _lib, components as _cc, ops

CHUNK = 2048             # SEGK_VEC_CHUNK
MAX_CAP = 1 << 30        # SEGK_VEC_MAX_CAP


def _r4(n):
    return (n + 3) // 4 * 4


def ws_ints(H, W, max_edges):
    """32-bit words of workspace segk_vec_runs / segk_vec_rings need (SEGK_VEC_WS_INTS of include/segk.h)"""
    hw, me = H * W, max_edges
    return (16 + _r4(2 * (me // 4 + 1)) + _r4(2 * ((me + CHUNK - 1) // CHUNK)) + 7 * _r4(me) + _r4(hw) +
            _r4((hw + CHUNK - 1) // CHUNK) + _r4((me + 3) // 4) + _r4((hw + 3) // 4))


def default_capacities(H, W, max_edges=None):
    """(max_runs, max_edges, max_rings, max_vertices) used where the caller gives None (DESIGN.md 3.17 "capacities").  The
    default max_edges is max(4096, H*W/2): exact for every mask whose boundary is at most an eighth of the 4*H*W edges a
    checkerboard has.  runs <= edges + W, rings <= edges / 4 and vertices <= edges hold for every map, so the other three
    follow from max_edges (the caller's, when given) and are exact whenever the edges fit."""
    hw = H * W
    me = min(4 * hw, max(4096, hw // 2)) if max_edges is None else int(max_edges)
    return min(hw, me + W), me, max(1, me // 4), me


def _capacity(name, value, default):
    if value is None:
        return int(default)
    if isinstance(value, bool) or int(value) != value or not 1 <= value <= MAX_CAP:
        raise ValueError(f"{name}: an integer in 1..2^30, got {value!r}")
    return int(value)


def _host(t, n=None):
    """the first n entries of a tensor as a NumPy array"""
    t = t if n is None else t[:n]
    return t.detach().cpu().numpy()


@dataclass
class Vectors:
    run_start: torch.Tensor     # int32 [max_runs]       first t = x*H + y of run r, ascending
    run_obj: torch.Tensor       # int32 [max_runs]       its object id (0: nothing)
    ring_obj: torch.Tensor      # int32 [max_rings]      object id of ring i (rings in ascending head key)
    ring_head: torch.Tensor     # int32 [max_rings]      smallest edge key 4*(y*W + x) + side on the ring
    ring_len: torch.Tensor      # int32 [max_rings]      unit edges on the ring
    ring_area2: torch.Tensor    # int64 [max_rings]      twice the signed area: > 0 outer ring, < 0 hole
    ring_offset: torch.Tensor   # int32 [max_rings + 1]  CSR offsets into xy
    xy: torch.Tensor            # int32 [max_vertices,2] corner vertices (x, y), ring after ring, from the head on
    totals: torch.Tensor        # int32 [4]              true runs, edges, rings, vertices (rings = vertices = -1: edges overflowed)
    num: torch.Tensor           # int32 [1]              K objects
    cls: torch.Tensor           # int32 [max_components] class of object id = row + 1
    area: torch.Tensor          # int32 [max_components]
    box: torch.Tensor           # int32 [max_components,4] (y0, x0, y1, x1), y1 and x1 exclusive
    size: Tuple[int, int]       # (H, W)
    connectivity: int = 4
    max_edges: int = 0          # the capacity the edge count is held against (no array has this length)
    _h: dict = field(default_factory=dict, repr=False, compare=False)

    # ---- host side: one wait for totals, then only the used prefixes are copied (and kept)
    def _counts(self):
        if "totals" not in self._h:
            self._h["totals"] = [int(v) for v in _host(self.totals)]
            self._h["num"] = int(_host(self.num)[0])
        return self._h["totals"]

    def _get(self, name, n):
        if name not in self._h:
            self._h[name] = _host(getattr(self, name), n)
        return self._h[name]

    @property
    def complete(self):
        """True when every array holds the whole result (no capacity was exceeded).  Synchronises."""
        runs, _, rings, verts = self._counts()
        return (runs <= self.run_start.shape[0] and rings >= 0 and rings <= self.ring_obj.shape[0] and
                verts <= self.xy.shape[0] and self._h["num"] <= self.cls.shape[0])

    def _need_rings(self, what):
        _, edges, rings, verts = self._counts()
        if rings < 0:
            raise RuntimeError(f"{what}: {edges} boundary edges exceed max_edges={self.max_edges}: no rings were built")
        if rings > self.ring_obj.shape[0] or verts > self.xy.shape[0]:
            raise RuntimeError(f"{what}: {rings} rings / {verts} vertices exceed max_rings={self.ring_obj.shape[0]} / "
                               f"max_vertices={self.xy.shape[0]}")
        return rings, verts

    def polygons(self, obj=None):
        """[(object id, twice the signed area, int32 [n,2] vertices (x, y)), ...] of every ring, or of the rings of object
        `obj`, in ring order.  The object lies on the right of the walk: outer rings have a positive area, holes a negative."""
        rings, verts = self._need_rings("polygons")
        ro, ra = self._get("ring_obj", rings), self._get("ring_area2", rings)
        off, xy = self._get("ring_offset", rings + 1), self._get("xy", verts)
        return [(int(ro[i]), int(ra[i]), xy[off[i]:off[i + 1]].copy()) for i in range(rings) if obj is None or ro[i] == obj]

    def coco_rle(self, obj):
        """{"size": [H, W], "counts": [...]}: COCO's uncompressed run-length code of object `obj` (column-major, the first
        count is of pixels outside the object), a stable group-by of the run table."""
        H, W = self.size
        runs = self._counts()[0]
        if runs > self.run_start.shape[0]:
            raise RuntimeError(f"coco_rle: {runs} runs exceed max_runs={self.run_start.shape[0]}")
        start, ro = self._get("run_start", runs), self._get("run_obj", runs)
        inside = ro == obj
        length = np.diff(np.append(start.astype(np.int64), H * W))
        first = np.flatnonzero(np.append(True, inside[1:] != inside[:-1]))         # where the groups of equal `inside` start
        counts = np.add.reduceat(length, first).tolist()
        if inside[0]:
            counts = [0] + counts
        return {"size": [H, W], "counts": [int(c) for c in counts]}

    def to_coco(self, image_id, category_of_class, first_id=1, compressed=False):
        """COCO annotation dicts of the objects whose class has an entry in category_of_class (others -- background -- are
        skipped): bbox [x, y, w, h] and area from the component rows, segmentation a polygon list when the object has no hole
        ring, else its uncompressed RLE (iscrowd 1, as COCO reads an RLE); compressed=True writes the RLE counts as COCO's
        compressed string (raster.rle_to_string)."""
        rings, verts = self._need_rings("to_coco")
        k = self._h["num"]
        if k > self.cls.shape[0]:
            raise RuntimeError(f"to_coco: {k} objects exceed max_components={self.cls.shape[0]}")
        cls, area, box = self._get("cls", k), self._get("area", k), self._get("box", k)
        ro, ra = self._get("ring_obj", rings), self._get("ring_area2", rings)
        off, xy = self._get("ring_offset", rings + 1), self._get("xy", verts)
        of_obj = {}
        for i in range(rings):
            of_obj.setdefault(int(ro[i]), []).append(i)
        out = []
        for o in range(1, k + 1):
            c = int(cls[o - 1])
            if c not in category_of_class:
                continue
            mine = of_obj.get(o, [])
            if any(ra[i] < 0 for i in mine):
                seg, crowd = self.coco_rle(o), 1
                if compressed:
                    from .raster import rle_to_string
                    seg["counts"] = rle_to_string(seg["counts"])
            else:
                seg, crowd = [[int(v) for v in xy[off[i]:off[i + 1]].reshape(-1)] for i in mine], 0
            y0, x0, y1, x1 = (int(v) for v in box[o - 1])
            out.append({"id": first_id + len(out), "image_id": image_id, "category_id": category_of_class[c],
                        "bbox": [x0, y0, x1 - x0, y1 - y0], "area": int(area[o - 1]), "iscrowd": crowd, "segmentation": seg})
        return out


def _check_args(connectivity, classes, max_components, caps, H, W):
    """-> (class_mask, (max_runs, max_edges, max_rings, max_vertices)) after the argument checks (all before any launch)"""
    cmask, _ = _cc._check_args(connectivity, classes, 0, False, max_components)
    names = ("max_runs", "max_edges", "max_rings", "max_vertices")
    me = _capacity("max_edges", caps[1], default_capacities(H, W)[1])
    return cmask, tuple(_capacity(n, v, d) for n, v, d in zip(names, caps, default_capacities(H, W, me)))


def as_vectors(vectors):
    """None / False, True or a dict of vectorize()'s keywords -> None or the dict (checked as far as it can be without a mask)"""
    if vectors is None or vectors is False:
        return None
    if vectors is True:
        return {}
    if isinstance(vectors, dict):
        allowed = {"connectivity", "classes", "max_components", "max_runs", "max_edges", "max_rings", "max_vertices"}
        if set(vectors) - allowed:
            raise ValueError(f"vectors: unknown keywords {sorted(set(vectors) - allowed)}")
        kw = dict(vectors)
        _check_args(kw.get("connectivity", 4), kw.get("classes"), kw.get("max_components", 1024),
                    [kw.get(n) for n in ("max_runs", "max_edges", "max_rings", "max_vertices")], 1, 1)
        return kw
    raise ValueError(f"vectors: None, True or a dict, got {type(vectors).__name__}")


def vectorize(mask, connectivity=4, classes=None, max_components=1024, max_runs=None, max_edges=None, max_rings=None,
              max_vertices=None):
    """Vectorise a uint8 [H,W] class mask on its device: its connected components (segk_cc_label, nothing is
    cleaned -- pass a cleaned mask), their run table, contour rings and corner vertices.  A Components is accepted too: its
    cleaned mask is vectorised afresh.

    connectivity    4 or 8: of the components, and of the rings at a vertex where two pixels of one object meet diagonally
    classes         the classes that form objects (default: all of 0..7)
    max_components  rows of cls / area / box
    max_runs, max_edges, max_rings, max_vertices   capacities (default_capacities(H, W)); Vectors.totals tells the true
                    counts, Vectors.complete whether everything fitted

    Nothing synchronises with the host and the input is not modified."""
    if isinstance(mask, _cc.Components):
        mask = mask.mask
    if isinstance(mask, torch.Tensor) and mask.ndim == 2:
        hw = (int(mask.shape[0]), int(mask.shape[1]))
    else:
        hw = (1, 1)
    cmask, (mr, me, mg, mv) = _check_args(connectivity, classes, max_components, [max_runs, max_edges, max_rings, max_vertices], *hw)
    mask = _cc._check_mask(mask, "vectorize")
    H, W = mask.shape
    cap, dev = int(max_components), mask.device
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        labels = torch.empty((H, W), **i32)
        rows = torch.empty((3, cap), **i32)          # cls, area, first
        box = torch.empty((cap, 4), **i32)
        num = torch.empty((1,), **i32)
        ws = torch.empty((max(_cc.ws_ints(H, W), ws_ints(H, W, me)),), **i32)
        runs = torch.empty((2, mr), **i32)
        rings = torch.empty((3, mg), **i32)
        area2 = torch.empty((mg,), dtype=torch.int64, device=dev)
        offset = torch.empty((mg + 1,), **i32)
        xy = torch.empty((mv, 2), **i32)
        totals = torch.empty((4,), **i32)
        s = ops._stream()
        _lib.call("segk_cc_label", mask.data_ptr(), labels.data_ptr(), num.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(),
                  box.data_ptr(), rows[2].data_ptr(), ws.data_ptr(), H, W, int(connectivity), cmask, cap, s)
        _lib.call("segk_vec_runs", labels.data_ptr(), runs[0].data_ptr(), runs[1].data_ptr(), totals.data_ptr(), ws.data_ptr(), H, W,
                  mr, s)
        _lib.call("segk_vec_rings", labels.data_ptr(), rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr(),
                  area2.data_ptr(), offset.data_ptr(), xy.data_ptr(), totals.data_ptr(), ws.data_ptr(), H, W, int(connectivity),
                  me, mg, mv, s)
    return Vectors(runs[0], runs[1], rings[0], rings[1], rings[2], area2, offset, xy, totals, num, rows[0], rows[1], box, (H, W),
                   int(connectivity), me)
