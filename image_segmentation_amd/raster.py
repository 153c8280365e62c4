"""Label rasterisation on the device: COCO-style polygons and run-length codes -> uint8 [H,W] label maps, the
inverse direction of vectors.py -- what a host loop over `pycocotools.mask.frPyObjects` / `cv2.fillPoly` plus one upload per
image does, as one table upload and one launch for a ragged batch.

    shapes = seg.shapes_from_coco(annotations, {17: 1, 18: 2})            # annotation order = paint order
    lab = seg.rasterize(shapes, size=(H, W))                               # uint8 [H,W] on the device
    labs = seg.rasterize_batch([shapes_0, shapes_1], sizes=[(H0, W0), (H1, W1)])
    seg.rasterize(seg.shapes_from_vectors(seg.vectorize(mask)), mask.shape)   # == mask where it was labelled

The kernel is csrc/raster.hip (segk_raster_labels); there is no CPU path.  Everything the device needs is decided on the host
(raster_plan): fixed-point edges, cumulative run starts, per tile the shapes that can touch it.  The compressed RLE string is
host only."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .augment import MAX_SIDE, _upload

TILE_H, TILE_W = 64, 256          # SEGK_RAST_TILE_H, SEGK_RAST_TILE_W
POLYGON, RLE = 0, 1               # SEGK_RAST_POLYGON, SEGK_RAST_RLE
FRAC = 256                        # fixed-point units per pixel
MAX_COORD = 1 << 22               # largest |X| in fixed-point units

# segk_rast_shape and segk_rast_tile of include/segk.h (32 bytes each)
SHAPE_DTYPE = np.dtype([("kind", "<i4"), ("value", "<i4"), ("begin", "<i4"), ("end", "<i4"), ("H", "<i4"), ("pad_", "<i4", (3,))])
TILE_DTYPE = np.dtype([("out_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("list0", "<i4"),
                       ("list1", "<i4")])


class RastShape(C.Structure):
    """segk_rast_shape of include/segk.h"""
    _fields_ = [("kind", C.c_int32), ("value", C.c_int32), ("begin", C.c_int32), ("end", C.c_int32), ("H", C.c_int32),
                ("pad_", C.c_int32 * 3)]


class RastTile(C.Structure):
    """segk_rast_tile of include/segk.h"""
    _fields_ = [("out_off", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("y0", C.c_int32), ("x0", C.c_int32),
                ("list0", C.c_int32), ("list1", C.c_int32)]


# ---------------------------------------------------------------------------------------------- COCO's compressed RLE string
def rle_to_string(counts):
    """COCO's rleToString: from the third count on the difference to the count two before, 5 bits per character (least
    significant group first, bit 0x20: more follow), character = group + 48."""
    out = []
    counts = [int(c) for c in counts]
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if c & 0x10 else (x != 0)
            out.append(chr((c | 0x20 if more else c) + 48))
    return "".join(out)


def rle_from_string(s):
    """the counts of a compressed RLE string (str or bytes): the inverse of rle_to_string"""
    if isinstance(s, (bytes, bytearray)):
        s = s.decode("ascii")
    if not isinstance(s, str):
        raise TypeError(f"rle_from_string: str or bytes, got {type(s).__name__}")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError("rle_from_string: the string ends inside a count")
            c = ord(s[p]) - 48
            if not 0 <= c < 64:
                raise ValueError(f"rle_from_string: character {s[p]!r} at {p} is outside the code")
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


# ---------------------------------------------------------------------------------------------- shapes
def _as_array(a, what):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    try:
        a = np.asarray(a)
    except Exception:
        raise ValueError(f"{what}: not an array of numbers") from None
    if a.dtype.kind not in "iuf":
        raise ValueError(f"{what}: integer or float coordinates, got dtype {a.dtype}")
    return a


def quantize(xy, what="ring"):
    """[n,2] (x, y) in pixel-corner units -> int32 [n,2] with 8 fractional bits: floor(v * 256 + 0.5).  Refuses anything but
    n >= 3 finite vertices with |X| <= 2^22."""
    a = _as_array(xy, what)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 3:
        raise ValueError(f"{what}: expected [n,2] (x, y) with n >= 3, got shape {tuple(a.shape)}")
    if a.dtype.kind == "f":
        if not np.isfinite(a).all():
            raise ValueError(f"{what}: non-finite coordinate")
        a = a.astype(np.float64)
        if np.abs(a).max() > 2 * MAX_COORD:          # keeps the product below exact in float64 and in int64
            raise ValueError(f"{what}: coordinate beyond +-{MAX_COORD // FRAC} pixels")
        q = np.floor(a * FRAC + 0.5).astype(np.int64)
    else:
        if np.abs(a.astype(np.int64)).max() > 2 * MAX_COORD:
            raise ValueError(f"{what}: coordinate beyond +-{MAX_COORD // FRAC} pixels")
        q = a.astype(np.int64) * FRAC
    if np.abs(q).max() > MAX_COORD:
        raise ValueError(f"{what}: coordinate beyond +-{MAX_COORD // FRAC} pixels")
    return np.ascontiguousarray(q.astype(np.int32))


class Shape:
    """One shape of a label map: `value` painted where the shape is inside.

    Shape(rings=[xy, ...], value=1)     even-odd over ALL rings; xy [n,2] (x, y), n >= 3, pixel-corner units, y downwards
    Shape(rle={"size": [H, W], "counts": [...] or "compressed string"}, value=1)     COCO's column-major run-length code

    Checked here: ring shape and length, finite coordinates within +-2^14 pixels, value 0..255, counts >= 0 that sum to H*W."""

    def __init__(self, rings=None, rle=None, value=1):
        if (rings is None) == (rle is None):
            raise ValueError("Shape: exactly one of rings= and rle=")
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= 255:
            raise ValueError(f"Shape: value is an integer in 0..255, got {value!r}")
        self.value = int(value)
        if rings is not None:
            if isinstance(rings, (np.ndarray, torch.Tensor)) and rings.ndim == 2:
                rings = [rings]
            rings = list(rings)
            if not rings:
                raise ValueError("Shape: a polygon has at least one ring")
            self.kind = POLYGON
            self.rings = [quantize(r, f"Shape: ring {i}") for i, r in enumerate(rings)]       # fixed point, int32 [n,2]
            self.size = self.counts = None
            # what raster_plan needs of a polygon, formed once: its edge rows and the pixels its box covers
            self._edges = np.concatenate([np.concatenate([r, np.roll(r, -1, axis=0)], axis=1) for r in self.rings])
            lo, hi = self._edges[:, :2].min(axis=0), self._edges[:, :2].max(axis=0)
            self._box = _centres(lo[1], hi[1]) + _centres(lo[0], hi[0])                         # py0, py1, px0, px1
            return
        if not isinstance(rle, dict) or "size" not in rle or "counts" not in rle:
            raise ValueError('Shape: rle is a dict {"size": [H, W], "counts": [...] or str}')
        size = list(rle["size"])
        if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= MAX_SIDE for v in size):
            raise ValueError(f"Shape: rle size {rle['size']!r}: [H, W] with sides 1..{MAX_SIDE}")
        counts = rle["counts"]
        if isinstance(counts, (str, bytes, bytearray)):
            counts = rle_from_string(counts)
        counts = _as_array(counts, "Shape: rle counts")
        if counts.ndim != 1 or counts.dtype.kind == "f" and not (np.isfinite(counts).all() and (counts == np.floor(counts)).all()):
            raise ValueError("Shape: rle counts are a list of integers")
        counts = counts.astype(np.int64)
        H, W = int(size[0]), int(size[1])
        if counts.size and counts.min() < 0:
            raise ValueError("Shape: negative rle count")
        if int(counts.sum()) != H * W:
            raise ValueError(f"Shape: rle counts sum to {int(counts.sum())}, the size {H} x {W} has {H * W} pixels")
        self.kind, self.rings, self.size, self.counts = RLE, None, (H, W), counts
        start = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(counts) else np.zeros(0, np.int64)
        self._start = start.astype(np.int32)
        fg = np.flatnonzero(counts[1::2] > 0)                   # the box: the columns of the foreground, every row
        if fg.size:
            first, last = 2 * fg[0] + 1, 2 * fg[-1] + 1
            self._box = (0, H, int(start[first]) // H, (int(start[last]) + int(counts[last]) - 1) // H + 1)
        else:
            self._box = (0, 0, 0, 0)

    def __repr__(self):
        what = f"rings={[len(r) for r in self.rings]}" if self.kind == POLYGON else f"rle={self.size[0]}x{self.size[1]}:{len(self.counts)}"
        return f"Shape({what}, value={self.value})"


def shapes_from_coco(annotations, category_to_class, crowd_value=None):
    """COCO annotation dicts -> shapes in annotation order (= paint order).  An annotation whose category_id has no entry in
    category_to_class is skipped.  A polygon segmentation gives one Shape per polygon (their union, as COCO reads them), an RLE
    segmentation (counts as a list or as the compressed string) one Shape.  crowd_value: the value of iscrowd annotations
    (e.g. 255 to ignore them) instead of their class."""
    out = []
    for ann in annotations:
        if ann["category_id"] not in category_to_class:
            continue
        value = category_to_class[ann["category_id"]]
        if crowd_value is not None and ann.get("iscrowd", 0):
            value = crowd_value
        seg = ann["segmentation"]
        if isinstance(seg, dict):
            out.append(Shape(rle=seg, value=value))
            continue
        for poly in seg:
            p = _as_array(poly, "shapes_from_coco: polygon")
            if p.ndim != 1 or p.size % 2:
                raise ValueError(f"shapes_from_coco: annotation {ann.get('id')}: a polygon is a flat list x0, y0, x1, y1, ...")
            out.append(Shape(rings=[p.reshape(-1, 2)], value=value))
    return out


def shapes_from_vectors(vec, value_of_class=None):
    """A Vectors -> one even-odd Shape per object with all its rings (outer rings and holes), in object order.  value_of_class:
    class -> value; objects of other classes are skipped (default: every object, value = its class).  Synchronises, as
    vec.polygons() does."""
    rings = {}
    for obj, _, xy in vec.polygons():
        rings.setdefault(obj, []).append(xy)
    k = vec._h["num"]
    if k > vec.cls.shape[0]:
        raise RuntimeError(f"shapes_from_vectors: {k} objects exceed max_components={vec.cls.shape[0]}")
    cls = vec._get("cls", k)
    out = []
    for o in range(1, k + 1):
        c = int(cls[o - 1])
        if value_of_class is not None and c not in value_of_class:
            continue
        if o in rings:
            out.append(Shape(rings=rings[o], value=c if value_of_class is None else value_of_class[c]))
    return out


# ---------------------------------------------------------------------------------------------- the host tables
def _centres(lo, hi):
    """pixel indices whose centre 256 p + 128 lies in the fixed-point range [lo, hi): (first, one past the last)"""
    return (int(lo) + 127) >> 8, (int(hi) + 127) >> 8


def _check_sizes(shapes_per_image, sizes, what):
    shapes_per_image, sizes = list(shapes_per_image), list(sizes)
    if not sizes or len(shapes_per_image) != len(sizes):
        raise ValueError(f"{what}: {len(shapes_per_image)} shape lists for {len(sizes)} sizes (one each, at least one image)")
    out = []
    for i, (shp, hw) in enumerate(zip(shapes_per_image, sizes)):
        hw = tuple(hw)
        if len(hw) != 2 or any(isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= MAX_SIDE for v in hw):
            raise ValueError(f"{what}: image {i}: size {hw!r}: (H, W) with sides 1..{MAX_SIDE}")
        hw = (int(hw[0]), int(hw[1]))
        shp = list(shp)
        for s in shp:
            if not isinstance(s, Shape):
                raise TypeError(f"{what}: image {i}: expected Shape objects, got {type(s).__name__}")
            if s.kind == RLE and s.size != hw:
                raise ValueError(f"{what}: image {i}: an rle of size {s.size[0]} x {s.size[1]} in an image of {hw[0]} x {hw[1]}")
        out.append((shp, hw))
    return out


def raster_plan(shapes_per_image, sizes):
    """The host tables of one segk_raster_labels launch (DESIGN.md 3.18 "tables") as NumPy arrays:

    edges      int32 [E,4]   (X0, Y0, X1, Y1) of every ring edge, ring after ring, shape after shape
    run_start  int32 [Rn]    cumulative run starts of every RLE shape
    shapes     SHAPE_DTYPE   [S]: all shapes of all images in list order
    shape_list int32 [L]     per tile the shapes whose bounding box meets it, ascending (= paint order)
    tiles      TILE_DTYPE    [T]: image after image, row-major
    out_off    [B] byte offset of every image in the output buffer (multiples of 256); out_bytes: its size"""
    items = _check_sizes(shapes_per_image, sizes, "raster_plan")
    edges, runs, recs = [], [], []
    boxes, base, width = [], [], []                              # per listed shape: its tile box, first tile and tiles per row
    listed = []
    tiles, out_off = [], []
    n_edges = n_runs = n_tiles = 0
    off = 0
    for shp, (H, W) in items:
        nty, ntx = -(-H // TILE_H), -(-W // TILE_W)
        for s in shp:
            if s.kind == POLYGON:
                edges.append(s._edges)
                recs.append((POLYGON, s.value, n_edges, n_edges + len(s._edges), H))
                n_edges += len(s._edges)
            else:
                runs.append(s._start)
                recs.append((RLE, s.value, n_runs, n_runs + len(s._start), H))
                n_runs += len(s._start)
            py0, py1, px0, px1 = s._box
            px0, px1, py0, py1 = max(px0, 0), min(px1, W), max(py0, 0), min(py1, H)
            if px0 >= px1 or py0 >= py1:
                continue                                         # the box misses the image: in no list
            listed.append(len(recs) - 1)
            boxes.append((py0 // TILE_H, (py1 - 1) // TILE_H + 1, px0 // TILE_W, (px1 - 1) // TILE_W + 1))
            base.append(n_tiles)
            width.append(ntx)
        for j in range(nty):
            for i in range(ntx):
                tiles.append((off, H, W, j * TILE_H, i * TILE_W, 0, 0))
        n_tiles += nty * ntx
        out_off.append(off)
        off += (H * W + 255) // 256 * 256
    tile_ids = shape_ids = None
    if listed:                                                   # every (shape, tile of its box) pair, without a Python loop
        ty0, ty1, tx0, tx1 = np.asarray(boxes, np.int64).T
        w = tx1 - tx0
        per_shape = (ty1 - ty0) * w
        first = np.cumsum(per_shape) - per_shape
        rep = lambda a: np.repeat(np.asarray(a, np.int64), per_shape)
        local = np.arange(int(per_shape.sum()), dtype=np.int64) - rep(first)
        tile_ids = rep(base) + (rep(ty0) + local // rep(w)) * rep(width) + rep(tx0) + local % rep(w)
        shape_ids = rep(listed)
    tiles = np.array(tiles, dtype=TILE_DTYPE)
    if tile_ids is not None:
        order = np.argsort(tile_ids, kind="stable")              # the pairs were formed in paint order
        shape_list = shape_ids[order].astype(np.int32)
        per_tile = np.bincount(tile_ids, minlength=n_tiles)
    else:
        shape_list, per_tile = np.zeros(0, np.int32), np.zeros(n_tiles, np.int64)
    ends = np.cumsum(per_tile)
    tiles["list0"], tiles["list1"] = ends - per_tile, ends
    shapes = np.zeros(len(recs), SHAPE_DTYPE)
    for name, col in zip(("kind", "value", "begin", "end", "H"), zip(*recs) if recs else [()] * 5):
        shapes[name] = col
    return {"edges": np.ascontiguousarray(np.concatenate(edges), np.int32) if edges else np.zeros((0, 4), np.int32),
            "run_start": np.concatenate(runs) if runs else np.zeros(0, np.int32),
            "shapes": shapes, "shape_list": shape_list, "tiles": tiles, "out_off": out_off, "out_bytes": off,
            "sizes": [hw for _, hw in items]}


# ---------------------------------------------------------------------------------------------- the launch
def _check_fill(fill, what):
    if isinstance(fill, bool) or not isinstance(fill, (int, np.integer)) or not 0 <= int(fill) <= 255:
        raise ValueError(f"{what}: fill is an integer in 0..255, got {fill!r}")
    return int(fill)


def launch(plan, out, fill, dev):
    """segk_raster_labels for a raster_plan on the current stream of `dev`; out: uint8 device buffer of >= plan["out_bytes"].
    The tables go up as one pinned blob; the returned buffer keeps them alive (stream order does the rest)."""
    with torch.cuda.device(dev):
        blob, (p_tiles, p_shapes, p_list, p_edges, p_runs) = _upload(
            [plan["tiles"], plan["shapes"], plan["shape_list"], plan["edges"], plan["run_start"]], dev)
        _lib.call("segk_raster_labels", p_tiles, len(plan["tiles"]), p_shapes, len(plan["shapes"]), p_list, len(plan["shape_list"]),
                  p_edges, len(plan["edges"]), p_runs, len(plan["run_start"]), out.data_ptr(), int(out.numel()), fill, ops._stream())
    return blob


def rasterize_batch(shapes_per_image, sizes, fill=0, device="cuda"):
    """Label maps of a ragged batch in ONE launch: a list of uint8 [H_i,W_i] tensors (views of one buffer) on `device`.
    Every pixel starts as `fill`; the shapes of an image are painted in list order, a later one over an earlier one.  An image
    without shapes is all `fill`.  Every argument is checked before the launch; nothing synchronises or is read back."""
    fill = _check_fill(fill, "rasterize_batch")
    plan = raster_plan(shapes_per_image, sizes)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"rasterize_batch: device {device!r}: the rasteriser runs on a CUDA / HIP device (there is no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((plan["out_bytes"],), dtype=torch.uint8, device=dev)
    launch(plan, out, fill, dev)
    return [out[o:o + h * w].view(h, w) for o, (h, w) in zip(plan["out_off"], plan["sizes"])]


def rasterize(shapes, size, fill=0, device="cuda"):
    """uint8 [H,W] label map of one image on `device` (rasterize_batch with one image)"""
    return rasterize_batch([shapes], [size], fill=fill, device=device)[0]
