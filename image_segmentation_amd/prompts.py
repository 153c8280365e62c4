"""Point prompts on the device -- the "Prompt Augmentation" cell of the reference's utils/augmentation.ipynb
(create_gaussian_heatmap, select_dominant_class and the retry loop around them) as two launches per batch, and the
click -> heat-map step of prediction.

    sampler = PromptSampler(sigma=3.0, candidates=1000, per_image=2, lut=TRIMAP_TO_PROMPT, seed=0)
    pb = sampler(labels)                                     # labels int64 [B,H,W] / [B,1,H,W] on the device, or a ragged list
    for X, p, y in PromptBatches(loader, sampler): ...       # what train_loop_prompt / eval_loop_prompt iterate over

The reference draws a pixel, builds exp(-d2 / (2 sigma^2)) over the whole image, sums it under every class of the remapped
label map, keeps the class with the largest sum and repeats (up to MAX_ATTEMPTS = 1000 times) until it has two different
classes; the two Gaussians go to 8-bit PNG files, the labels become "selected class or 0".  Here the candidates of a batch
are drawn at once and scored by segk_prompt_scores; segk_prompt_make applies the same "first distinct classes in draw
order" rule and writes the heat-maps and targets.  Every value that decides a result comes from two tables this module
builds on the host in float64 with the reference's own expression (heat_tables), so the heat-maps equal the reference's
files bit for bit.  There is no CPU path."""
import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Union

import numpy as np
import torch

from . import _lib, ops

# the reference's two label remaps as one table (utils/dataset.py target_remap: 255 -> 3; the cell: 3 -> 0, then + 1):
# trimap 0 / 1 / 2 / boundary -> prompt classes 1 (background + boundary) / 2 / 3 / 1; every other value -> 0
TRIMAP_TO_PROMPT = np.zeros(256, dtype=np.uint8)
TRIMAP_TO_PROMPT[[0, 1, 2, 3, 255]] = [1, 2, 3, 1, 1]
TRIMAP_TO_PROMPT.setflags(write=False)

_TAIL = 1e-12        # bound on the Gaussian mass of a whole image outside the scoring window


@lru_cache(maxsize=64)
def heat_tables(sigma, H, W):
    """-> (w float64 [2 R^2 + 1], q uint8 [2 R^2 + 1], R), indexed by the integer squared distance d2 = dy^2 + dx^2:
    w[d2] = exp(-d2 / (2 sigma^2)) -- create_gaussian_heatmap's expression in its precision; q[d2] = (uint8)(255 w[d2]) --
    what the cell writes to the PNG file (non-zero up to d2 = floor(2 sigma^2 ln 255)); R = the smallest integer with
    H * W * exp(-R^2 / (2 sigma^2)) <= 1e-12, the radius of the scoring window: everything the reference sums outside it is
    below 1e-12 in total.  Host only; the arrays are read-only."""
    sigma, H, W = float(sigma), int(H), int(W)
    if not sigma > 0 or not math.isfinite(sigma):
        raise ValueError(f"sigma must be positive, got {sigma}")
    if H < 1 or W < 1:
        raise ValueError(f"image size {H} x {W}")
    two_s2 = 2 * sigma**2
    R = max(0, math.isqrt(max(0, int(two_s2 * math.log(H * W / _TAIL)))) - 1)
    while H * W * math.exp(-R * R / two_s2) > _TAIL:
        R += 1
    if R > 4096:
        raise ValueError(f"sigma {sigma} needs a scoring window of radius {R} (at most 4096)")
    d2 = np.arange(2 * R * R + 1)
    w = np.exp(-d2 / (2 * sigma**2))
    q = (w * 255).astype(np.uint8)
    w.setflags(write=False)
    q.setflags(write=False)
    return w, q, R


_device_tables = {}


def _tables_on(sigma, H, W, dev):
    """(w, nw, q, nq, R) on the device, uploaded once per (sigma, R, device); q is cut behind its last non-zero entry."""
    w, q, R = heat_tables(sigma, H, W)
    key = (float(sigma), R, dev)
    t = _device_tables.get(key)
    if t is None:
        nq = max(1, int(np.flatnonzero(q)[-1]) + 1) if q.any() else 1
        t = (torch.from_numpy(w.copy()).to(dev), len(w), torch.from_numpy(q[:nq].copy()).to(dev), nq, R)
        _device_tables[key] = t
    return t


def _lut_tensor(lut):
    if lut is None:
        return None
    t = np.asarray(lut)
    if t.shape != (256,) or t.dtype.kind not in "iu" or t.min() < 0 or t.max() > 255:
        raise ValueError("lut: 256 integer entries in 0..255")
    return torch.from_numpy(t.astype(np.uint8))


@dataclass
class PromptBatch:
    """What PromptSampler returns.  For a batch [B,H,W] the fields are tensors; for a ragged list of maps, heatmaps and
    targets are lists of per-image tensors ([per_image,1,h,w] and [per_image,h,w])."""
    heatmaps: Union[torch.Tensor, list]     # float32 [B,per_image,1,H,W]: (float)uint8 / 255, the decoded PNG of the reference
    targets: Union[torch.Tensor, list]      # int64 [B,per_image,H,W]: selected class or 0
    classes: torch.Tensor                   # int32 [B,per_image]
    centers: torch.Tensor                   # int32 [B,per_image,2] (y, x)
    valid: torch.Tensor                     # bool [B]: per_image distinct classes were found (else the image is all zero)

    def triples(self, X):
        """(X_rep, heat, target) of the valid images only, each image repeated per_image times next to each other (the
        reference's <name>_1, <name>_2 files): [B',3,H,W], [B',1,H,W], [B',1,H,W] -- the shapes promptDataset batches
        have; lists of [3,h,w] / [1,h,w] / [1,h,w] for ragged input.  This call SYNCHRONISES with the device: the number
        of valid images decides the shapes (a boolean gather)."""
        PI = int(self.classes.shape[1])
        if isinstance(self.heatmaps, list):
            keep = self.valid.tolist()
            if len(X) != len(keep):
                raise ValueError(f"{len(X)} images for {len(keep)} label maps")
            Xs, hs, ts = [], [], []
            for k, ok in enumerate(keep):
                if ok:
                    for j in range(PI):
                        Xs.append(X[k].to(self.heatmaps[k].device))
                        hs.append(self.heatmaps[k][j])
                        ts.append(self.targets[k][j].unsqueeze(0))
            return Xs, hs, ts
        if X.shape[0] != self.valid.shape[0]:
            raise ValueError(f"{X.shape[0]} images for {self.valid.shape[0]} label maps")
        idx = torch.nonzero(self.valid).flatten()
        H, W = self.heatmaps.shape[-2:]
        Xr = X.to(self.heatmaps.device)[idx].repeat_interleave(PI, 0)
        return Xr, self.heatmaps[idx].reshape(-1, 1, H, W), self.targets[idx].reshape(-1, 1, H, W)


class PromptSampler:
    """labels -> PromptBatch.  sigma, candidates (the reference's MAX_ATTEMPTS) and per_image (its two files per image)
    as in the reference's cell; lut: optional 256-entry table applied to the labels first (TRIMAP_TO_PROMPT for raw
    trimaps; None: the labels are classes already; classes are 0..7, anything else counts as 0).

    Without `centers` the call draws `candidates` uniform pixels per image on the device with a generator of its own:
    two samplers with one seed draw the same clicks; reseed() rewinds (an evaluation set that must not move between
    epochs).  With `centers` (integer [B,K,2], y then x; a list of [K,2] for ragged input) the call is a pure function.
    Two launches per batch, no synchronisation with the host."""

    def __init__(self, sigma=3.0, candidates=1000, per_image=2, lut=None, seed=None):
        self.sigma = float(sigma)
        if not self.sigma > 0 or not math.isfinite(self.sigma):
            raise ValueError(f"sigma must be positive, got {sigma}")
        self.candidates, self.per_image = int(candidates), int(per_image)
        if self.candidates < 1 or self.candidates > (1 << 20):
            raise ValueError(f"candidates must be in 1..2^20, got {candidates}")
        if not 1 <= self.per_image <= _lib.MAX_CLASSES - 1:
            raise ValueError(f"per_image must be in 1..{_lib.MAX_CLASSES - 1}, got {per_image}")
        self._lut = _lut_tensor(lut)
        self._lut_dev = {}
        self.seed = seed
        self._gens = {}

    def reseed(self, seed=None):
        """Rewind the click generator to its seed (or to a new one)."""
        if seed is not None:
            self.seed = seed
        self._gens = {}

    def _generator(self, dev):
        g = self._gens.get(dev)
        if g is None:
            g = torch.Generator(device=dev)
            if self.seed is None:
                self.seed = g.seed()
            g.manual_seed(int(self.seed))
            self._gens[dev] = g
        return g

    def _lut_on(self, dev):
        if self._lut is None:
            return None
        if dev not in self._lut_dev:
            self._lut_dev[dev] = self._lut.to(dev)
        return self._lut_dev[dev]

    @staticmethod
    def _check_centers(centers, B, H, W, what="centers"):
        c = torch.as_tensor(np.asarray(centers)) if not isinstance(centers, torch.Tensor) else centers
        if c.ndim != 3 or c.shape[0] != B or c.shape[1] < 1 or c.shape[2] != 2 or torch.is_floating_point(c) or c.dtype == torch.bool:
            raise ValueError(f"{what}: expected integers [{B},K,2] (y, x), got {c.dtype} {tuple(c.shape)}")
        if not c.is_cuda:          # host data is range-checked; device data is not (that would synchronise): the kernels
            lo, hy, hx = int(c.min()), int(c[..., 0].max()), int(c[..., 1].max())       # ignore a centre outside the image
            if lo < 0 or hy >= H or hx >= W:
                raise ValueError(f"{what}: a centre lies outside the {H} x {W} image")
        return c

    def _run(self, labels, centers):
        """labels int64 [B,H,W] on the device, centers int32 [B,K,2] on it -> the five tensors."""
        B, H, W = labels.shape
        if H > 32768 or W > 32768:
            raise ValueError(f"label maps of {H} x {W}: sides up to 32768")
        dev, K, PI = labels.device, int(centers.shape[1]), self.per_image
        centers = centers.to(dev, non_blocking=True).to(torch.int32).contiguous()
        wt, nw, qt, nq, R = _tables_on(self.sigma, H, W, dev)
        lut = self._lut_on(dev)
        scores = torch.empty((B, K, _lib.MAX_CLASSES), dtype=torch.float64, device=dev)
        cls = torch.empty((B, K), dtype=torch.int32, device=dev)
        heat = torch.empty((B, PI, 1, H, W), dtype=torch.float32, device=dev)
        target = torch.empty((B, PI, H, W), dtype=torch.int64, device=dev)
        classes = torch.empty((B, PI), dtype=torch.int32, device=dev)
        cent = torch.empty((B, PI, 2), dtype=torch.int32, device=dev)
        valid = torch.empty((B,), dtype=torch.bool, device=dev)
        with torch.cuda.device(dev):
            s = ops._stream()
            _lib.call("segk_prompt_scores", labels.data_ptr(), ops._p(lut), centers.data_ptr(), wt.data_ptr(), nw, R,
                      scores.data_ptr(), cls.data_ptr(), B, K, H, W, s)
            _lib.call("segk_prompt_make", labels.data_ptr(), ops._p(lut), centers.data_ptr(), cls.data_ptr(), qt.data_ptr(), nq,
                      heat.data_ptr(), target.data_ptr(), classes.data_ptr(), cent.data_ptr(), valid.data_ptr(), B, K, PI, H, W, s)
        self.last_scores, self.last_cls = scores, cls          # per candidate, of the last launch pair (tests, diagnostics)
        return heat, target, classes, cent, valid

    def _draw(self, B, H, W, dev):
        g = self._generator(dev)
        ys = torch.randint(0, H, (B, self.candidates), generator=g, device=dev, dtype=torch.int32)
        xs = torch.randint(0, W, (B, self.candidates), generator=g, device=dev, dtype=torch.int32)
        return torch.stack((ys, xs), dim=-1)

    @staticmethod
    def _label_map(lab, what):
        if not isinstance(lab, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(lab).__name__}")
        if lab.dtype != torch.int64:
            raise TypeError(f"{what}: label maps are int64 (call .long()), got {lab.dtype}")
        return lab

    def __call__(self, labels, centers=None):
        if isinstance(labels, (list, tuple)):                  # ragged: one launch pair per image
            if not labels:
                raise ValueError("PromptSampler: no label maps")
            if centers is not None and len(centers) != len(labels):
                raise ValueError(f"{len(centers)} centre sets for {len(labels)} label maps")
            maps = []
            for k, lab in enumerate(labels):
                lab = self._label_map(lab, f"labels[{k}]")
                if lab.ndim == 3 and lab.shape[0] == 1:
                    lab = lab[0]
                if lab.ndim != 2:
                    raise ValueError(f"labels[{k}]: expected [H,W] or [1,H,W], got {tuple(lab.shape)}")
                maps.append(lab.contiguous().unsqueeze(0))
            cents = []
            for k, lab in enumerate(maps):                     # every argument is checked before the first launch
                H, W = lab.shape[1:]
                if centers is None:
                    cents.append(None)
                else:
                    ck = centers[k]
                    ck = ck.unsqueeze(0) if isinstance(ck, torch.Tensor) else np.asarray(ck)[None]
                    cents.append(self._check_centers(ck, 1, H, W, f"centers[{k}]"))
            for lab in maps:
                ops._require_cuda(lab, "PromptSampler")
            outs = []
            for lab, c in zip(maps, cents):
                H, W = lab.shape[1:]
                outs.append(self._run(lab, self._draw(1, H, W, lab.device) if c is None else c))
            return PromptBatch([o[0][0] for o in outs], [o[1][0] for o in outs], torch.cat([o[2] for o in outs]),
                               torch.cat([o[3] for o in outs]), torch.cat([o[4] for o in outs]))
        labels = self._label_map(labels, "labels")
        if labels.ndim == 4 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if labels.ndim != 3 or labels.shape[0] < 1:
            raise ValueError(f"labels: expected [B,H,W] or [B,1,H,W], got {tuple(labels.shape)}")
        labels = labels.contiguous()
        B, H, W = labels.shape
        if centers is not None:
            centers = self._check_centers(centers, B, H, W)
        ops._require_cuda(labels, "PromptSampler")
        c = self._draw(B, H, W, labels.device) if centers is None else centers
        return PromptBatch(*self._run(labels, c))


class PromptBatches:
    """Iterable over (image, heat-map, target) triples made from a loader of (image, label) batches -- tensors
    [B,3,H,W] / [B,H,W] or [B,1,H,W], or the lists of differently sized tensors a ragged collate function returns -- and a
    PromptSampler: what train_loop_prompt, eval_loop_prompt and start_prompt take as their `dataloader`.  Labels of any
    integer type are widened to int64 on the device.  It never skips a batch (the loops step the optimizer on
    len(dataloader)): a batch without a single valid image raises ValueError.  Each batch synchronises once
    (PromptBatch.triples)."""

    def __init__(self, loader, sampler, device=None):
        self.loader, self.sampler = loader, sampler
        self.device = torch.device("cuda" if device is None else device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for i, (X, y) in enumerate(self.loader):
            if isinstance(y, (list, tuple)):
                y = [t.to(self.device, non_blocking=True).long() for t in y]
                X = [t.to(self.device, non_blocking=True) for t in X]
                n = len(y)
            else:
                y = y.to(self.device, non_blocking=True).long()
                X = X.to(self.device, non_blocking=True)
                n = int(y.shape[0])
            Xr, p, t = self.sampler(y).triples(X)
            if len(Xr) == 0:
                raise ValueError(f"PromptBatches: batch {i} ({n} images) holds no image with {self.sampler.per_image} distinct "
                                 "classes -- prompt training data has at least two classes per image")
            yield Xr, p, t


def point_heatmap(points, H, W, sigma=3.0, device=None):
    """float32 [1,H,W] on the device: the 8-bit Gaussian of one click (y, x), or the maximum of the Gaussians of several --
    what a trained prompt model expects as its second input (segk_prompt_heatmap).  Host points are range-checked."""
    dev = torch.device("cuda" if device is None else device)
    pts = _points_array(points, H, W, "points")
    return _heatmap_on(torch.from_numpy(pts).to(dev, non_blocking=True), H, W, sigma, dev)


def _points_array(points, H, W, what):
    """one (y, x) or a list of them -> int32 [P,2], checked against the image"""
    if isinstance(points, torch.Tensor):
        points = points.cpu().numpy()
    a = np.asarray(points)
    if a.dtype.kind not in "iu" or a.size == 0 or a.shape[-1] != 2 or a.ndim > 2:
        raise ValueError(f"{what}: expected one integer (y, x) or a list of them, got {a.dtype} {a.shape}")
    a = a.reshape(-1, 2)
    if len(a) > 1024:
        raise ValueError(f"{what}: {len(a)} points (at most 1024)")
    if a.min() < 0 or a[:, 0].max() >= H or a[:, 1].max() >= W:
        raise ValueError(f"{what}: a point lies outside the {H} x {W} image")
    return np.ascontiguousarray(a.astype(np.int32))


def _heatmap_on(pts, H, W, sigma, dev):
    if H > 32768 or W > 32768:
        raise ValueError(f"image of {H} x {W}: sides up to 32768")
    _, _, qt, nq, _ = _tables_on(sigma, H, W, dev)
    heat = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("segk_prompt_heatmap", pts.data_ptr(), int(pts.shape[0]), qt.data_ptr(), nq, heat.data_ptr(), H, W, ops._stream())
    return heat
