"""Robustness evaluation -- the experiment of the reference's report section 4.1 ("Robustness exploration", figure 6): a
trained model is scored under eight perturbation types, each at ten increasing severity levels, and mean Dice is plotted
against the level.  The reference holds no code for it (only the report and the README describe it), so the arithmetic is
this project's definition and the default levels are not pinned against the reference: pass `levels=`.

    out = perturb(images, "gaussian_noise", 10, seed=0)       # list of uint8 [H,W,3] device tensors, one launch
    res = robustness_sweep(model, images, labels, num_classes=4, ignore_index=3, target_size=224)
    res["gaussian_blur"]["dice"]                                # mean Dice per level; json.dumps(res) works

Images stay 8-bit interleaved [H,W,3] at their own sizes.  A batch of differently sized images costs one upload of a
descriptor table and one launch (segk_perturb_point or segk_perturb_blur).  Every value that decides a result comes from the
host (value LUT, Gaussian inverse CDF, per-image seeds, occlusion corners); the device combines them with integer arithmetic
only, so the outputs are bit-stable and equal the NumPy restatement of tests/perturb_reference.py.  There is no CPU path."""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

PERTURBATIONS = ("gaussian_noise", "gaussian_blur", "contrast_increase", "contrast_decrease", "brightness_increase",
                 "brightness_decrease", "occlusion", "salt_and_pepper")
# ten levels per type, the first is the clean image; NOT pinned against the reference (it has no code for the experiment)
DEFAULT_LEVELS = {
    "gaussian_noise": tuple(range(0, 20, 2)),                                      # standard deviation
    "gaussian_blur": tuple(range(10)),                                             # passes of the 3 x 3 mask
    "contrast_increase": (1.0, 1.01, 1.02, 1.03, 1.04, 1.05, 1.10, 1.15, 1.20, 1.25),  # factor
    "contrast_decrease": (1.0, 0.95, 0.90, 0.85, 0.80, 0.60, 0.40, 0.30, 0.20, 0.10),  # factor
    "brightness_increase": tuple(range(0, 50, 5)),                                 # added
    "brightness_decrease": tuple(range(0, 50, 5)),                                 # subtracted
    "occlusion": tuple(range(0, 50, 5)),                                           # edge of the black square
    "salt_and_pepper": tuple(round(0.02 * i, 2) for i in range(10)),               # fraction of the elements
}

LUT, GAUSS_NOISE, SALT_PEPPER, OCCLUDE = range(4)            # SEGK_PERTURB_*
GAUSS_ENTRIES = 4096
POINT_TILE = 4096
BLUR_TH, BLUR_TW, BLUR_MAX = 32, 64, 9
MAX_SIDE = 8192
_LUT_KINDS = ("contrast_increase", "contrast_decrease", "brightness_increase", "brightness_decrease")
_M64 = (1 << 64) - 1

# segk_perturb_desc of include/segk.h
DESC = np.dtype([("src", "<u8"), ("dst", "<u8"), ("seed", "<u8"), ("H", "<i4"), ("W", "<i4"), ("src_c", "<i4"),
                 ("tile0", "<i4"), ("p0", "<i4"), ("p1", "<i4"), ("p2", "<i4"), ("pad_", "<i4")])
assert DESC.itemsize == 56


# ------------------------------------------------------------------------------------------------ host side (NumPy only)
def _check_kind(kind):
    if kind not in PERTURBATIONS:
        raise ValueError(f"unknown perturbation {kind!r}: one of {', '.join(PERTURBATIONS)}")


def _check_level(kind, level):
    """The level as the number the kind works with (an int for counts of pixels, passes and grey values)."""
    _check_kind(kind)
    if isinstance(level, (bool, str)) or not isinstance(level, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(level)):
        raise ValueError(f"{kind}: level {level!r} is not a finite number")
    v = float(level)
    if kind == "gaussian_noise":
        ok = 0 <= v <= 255
    elif kind == "gaussian_blur":
        ok = v == int(v) and 0 <= v <= BLUR_MAX
    elif kind == "contrast_increase":
        ok = 1 <= v <= 255
    elif kind == "contrast_decrease":
        ok = 0 <= v <= 1
    elif kind in ("brightness_increase", "brightness_decrease"):
        ok = v == int(v) and 0 <= v <= 255
    elif kind == "occlusion":
        ok = v == int(v) and 0 <= v <= MAX_SIDE
    else:
        ok = 0 <= v <= 1
    if not ok:
        raise ValueError(f"{kind}: level {level!r} is out of range")
    return int(v) if kind in ("gaussian_blur", "brightness_increase", "brightness_decrease", "occlusion") else v


def is_identity(kind, level):
    """True when the level leaves every image as it is (the first of the ten default levels of every kind)."""
    v = _check_level(kind, level)
    return v == 1.0 if kind in ("contrast_increase", "contrast_decrease") else v == 0


def _mix(z):
    """splitmix64 finaliser (the one the kernels hash elements with)."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def cell_seed(seed, kind_index, level_index):
    """The seed robustness_sweep gives perturb() for one (kind, level) cell: a fixed function of its arguments."""
    return _mix((int(seed) * 0x9E3779B97F4A7C15 + int(kind_index) * 1024 + int(level_index) + 1) & _M64)


def image_seed(seed, index):
    """The seed of image `index` of a perturb(images, ..., seed) call."""
    return _mix((_mix(int(seed) & _M64) + (int(index) + 1) * 0x9E3779B97F4A7C15) & _M64)


def _norm_ppf(p):
    """Inverse of the standard normal CDF in float64: Acklam's rational approximation and one Halley step on erfc."""
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02,
         -3.066479806614716e+01, 2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01,
         -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00,
         4.374664141464968e+00, 2.938163982698783e+00)
    d = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)
    if p < 0.02425:
        q = math.sqrt(-2.0 * math.log(p))
        x = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / \
            ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0)
    elif p > 1.0 - 0.02425:
        q = math.sqrt(-2.0 * math.log(1.0 - p))
        x = -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / \
            ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0)
    else:
        q = p - 0.5
        r = q * q
        x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / \
            (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0)
    e = 0.5 * math.erfc(-x / math.sqrt(2.0)) - p
    u = e * math.sqrt(2.0 * math.pi) * math.exp(x * x / 2.0)
    return x - u / (1.0 + x * u / 2.0)


@lru_cache(maxsize=1)
def _ppf_grid():
    z = np.array([_norm_ppf((j + 0.5) / GAUSS_ENTRIES) for j in range(GAUSS_ENTRIES // 2, GAUSS_ENTRIES)], dtype=np.float64)
    return np.concatenate([-z[::-1], z])                     # exactly antisymmetric


@lru_cache(maxsize=64)
def gauss_table(std):
    """int16 [4096]: rint(std * Phi^-1((j + 1/2) / 4096)), the inverse CDF of N(0, std^2) on 4096 equal-mass cells."""
    std = float(std)
    if not (math.isfinite(std) and 0 <= std <= 255):
        raise ValueError(f"gauss_table: standard deviation {std} (0..255)")
    t = np.rint(std * _ppf_grid()).astype(np.int16)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=256)
def value_lut(kind, level):
    """uint8 [256] of the four table kinds: clip(rint(v * level), 0, 255) (contrast) or clip(v +- level, 0, 255) (brightness),
    computed in float64."""
    if kind not in _LUT_KINDS:
        raise ValueError(f"value_lut: {kind!r} is not one of {', '.join(_LUT_KINDS)}")
    lv = _check_level(kind, level)
    v = np.arange(256, dtype=np.float64)
    if kind.startswith("contrast"):
        t = np.rint(v * float(lv))
    else:
        t = v + float(lv) if kind == "brightness_increase" else v - float(lv)
    t = np.clip(t, 0, 255).astype(np.uint8)
    t.setflags(write=False)
    return t


@dataclass
class PerturbPlan:
    """What perturb() launches: drawn on the host by perturb_plan, a pure function of its arguments."""
    kind: str
    level: float
    identity: bool                  # the level leaves the images as they are
    entry: str                      # "segk_perturb_point" | "segk_perturb_blur"
    code: int                       # the point kind (SEGK_PERTURB_*) or the number of blur passes
    table: object                   # uint8 [256] / int16 [4096] / None
    sizes: tuple                    # (H, W) per image
    seeds: tuple                    # per-image hash seed
    params: tuple                   # per-image (p0, p1, p2): threshold, or the square's (y0, x0, edge)


def perturb_plan(kind, level, sizes, seed=0):
    """The plan of perturb(images, kind, level, seed) for images of the given (H, W) sizes.  Per image: the hash seed
    image_seed(seed, i); occlusion draws y0 in [0, H - e] and x0 in [0, W - e] (e = min(edge, H, W)), in this order, from
    np.random.default_rng(image_seed(seed, i))."""
    lv = _check_level(kind, level)
    sizes = tuple((int(H), int(W)) for H, W in sizes)
    for H, W in sizes:
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError(f"image of {H} x {W}: sides 1..{MAX_SIDE}")
    seeds = tuple(image_seed(seed, i) for i in range(len(sizes)))
    params = tuple((0, 0, 0) for _ in sizes)
    entry, code, table = "segk_perturb_point", LUT, None
    if kind in _LUT_KINDS:
        table = value_lut(kind, lv)
    elif kind == "gaussian_noise":
        code, table = GAUSS_NOISE, gauss_table(lv)
    elif kind == "salt_and_pepper":
        code = SALT_PEPPER
        params = tuple((int(math.floor(lv * (1 << 24))), 0, 0) for _ in sizes)
    elif kind == "occlusion":
        code, out = OCCLUDE, []
        for (H, W), s in zip(sizes, seeds):
            e = min(lv, H, W)
            rng = np.random.default_rng(s)
            y0 = int(rng.integers(0, H - e + 1))
            x0 = int(rng.integers(0, W - e + 1))
            out.append((y0, x0, e))
        params = tuple(out)
    else:
        entry, code = "segk_perturb_blur", lv
    return PerturbPlan(kind, lv, is_identity(kind, lv), entry, code, table, sizes, seeds, params)


def _tiles(plan, H, W):
    if plan.entry == "segk_perturb_blur":
        return ((H + BLUR_TH - 1) // BLUR_TH) * ((W + BLUR_TW - 1) // BLUR_TW)
    return (H * W * 3 + POINT_TILE - 1) // POINT_TILE


def _check_images(images):
    """-> list of torch uint8 [H,W,3|4] tensors (NumPy arrays become host tensors); nothing is copied to a device."""
    import torch
    if isinstance(images, (np.ndarray, torch.Tensor)):
        images = list(images) if images.ndim == 4 else [images]
    if not isinstance(images, (list, tuple)) or not images:
        raise TypeError("images: expected a non-empty list of uint8 [H,W,3|4] tensors or arrays")
    out = []
    for k, im in enumerate(images):
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8:
                raise TypeError(f"images[{k}]: images are uint8, got {im.dtype}")
            im = np.ascontiguousarray(im)
            im = torch.from_numpy(im if im.flags.writeable else im.copy())     # torch warns about read-only arrays
        if not isinstance(im, torch.Tensor):
            raise TypeError(f"images[{k}]: expected a tensor or an array, got {type(im).__name__}")
        if im.dtype != torch.uint8:
            raise TypeError(f"images[{k}]: images are uint8, got {im.dtype}")
        if im.ndim != 3 or im.shape[2] not in (3, 4):
            raise ValueError(f"images[{k}]: expected uint8 [H,W,3|4], got {tuple(im.shape)}")
        if not (1 <= im.shape[0] <= MAX_SIDE and 1 <= im.shape[1] <= MAX_SIDE):
            raise ValueError(f"images[{k}]: image of {im.shape[0]} x {im.shape[1]}: sides 1..{MAX_SIDE}")
        out.append(im)
    return out


# ------------------------------------------------------------------------------------------------ device side
def _launch(images, plan):
    """images: checked tensors -> (outputs, (entry, args), keep-alive).  One upload, one launch; the inputs are only read."""
    import torch
    from . import _lib, ops
    from .augment import _upload
    dev = next((im.device for im in images if im.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("perturb: no GPU -- image_segmentation_amd has no CPU path")
        dev = torch.device("cuda", torch.cuda.current_device())
    n = len(images)
    if n > 65535:
        raise ValueError(f"a batch of {n} images (at most 65535)")
    if tuple(tuple(im.shape[:2]) for im in images) != plan.sizes:
        raise ValueError("the plan was drawn for other image sizes")
    with torch.cuda.device(dev):
        srcs = [im.to(dev, non_blocking=True).contiguous() for im in images]
        offs, total = [], 0
        for H, W in plan.sizes:
            offs.append(total)
            total += (H * W * 3 + 255) // 256 * 256
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        outs = [buf[o:o + H * W * 3].view(H, W, 3) for o, (H, W) in zip(offs, plan.sizes)]
        desc = np.zeros(n, dtype=DESC)
        tile = 0
        for k, (H, W) in enumerate(plan.sizes):
            d = desc[k]
            d["src"], d["dst"], d["seed"] = srcs[k].data_ptr(), outs[k].data_ptr(), plan.seeds[k]
            d["H"], d["W"], d["src_c"], d["tile0"] = H, W, srcs[k].shape[2], tile
            d["p0"], d["p1"], d["p2"] = plan.params[k]
            tile += _tiles(plan, H, W)
        if tile >= 1 << 30:
            raise ValueError(f"a batch of {tile} tiles (below 2^30)")
        parts = [desc] + ([plan.table] if plan.table is not None else [])
        tables, ptrs = _upload(parts, dev)
        s = ops._stream()
        if plan.entry == "segk_perturb_blur":
            args = (ptrs[0], n, tile, plan.code, s)
        else:
            args = (ptrs[0], n, tile, plan.code, ptrs[1] if plan.table is not None else 0, s)
        _lib.call(plan.entry, *args)
    return outs, (plan.entry, args), (srcs, tables, buf)


def perturb(images, kind, level, seed=0):
    """Perturb a list of uint8 [H,W,3|4] images (tensors or arrays, host or device, any sizes; alpha is dropped) -> list of
    uint8 [H,W,3] device tensors.  kind: one of PERTURBATIONS; level: the kind's own number (DEFAULT_LEVELS); a level that is
    the identity returns the inputs' values.  One table upload and one launch per call; the inputs are not modified."""
    images = _check_images(images)
    plan = perturb_plan(kind, level, [tuple(im.shape[:2]) for im in images], seed)
    return _launch(images, plan)[0]


def _metrics(M, num_classes, ignore_index):
    """Summed confusion counts [pred, label] -> (mean dice, mean iou, mean accuracy, per-class dice) on the macro,
    ignore-aware path of the eval loops (MetricsHistory)."""
    from .metrics import MetricsHistory
    agg = MetricsHistory(num_classes, ignore_index)
    tp, fp, fn, tn = MetricsHistory.counts_from_confusion(M, int(M.sum()))
    agg.total_tp += tp
    agg.total_fp += fp
    agg.total_fn += fn
    agg.total_tn += tn
    dice, iou, acc = agg.compute_epoch_metrics()

    def num(v):                                  # 0 / 0 (a class neither labelled nor predicted) has no JSON number
        return float(v) if math.isfinite(v) else None
    return num(dice), num(iou), num(acc), [num(v) for v in agg.last_per_class_dice.tolist()]


def robustness_sweep(model, images, labels, num_classes, ignore_index=None, perturbations=PERTURBATIONS, levels=None,
                     seed=0, heatmaps=None, points=None, **segmenter_kw):
    """Score `model` under every (perturbation, level) -> {kind: {"levels", "dice", "iou", "accuracy", "per_class_dice"}}
    (plain lists, json.dumps-able; a class that is neither labelled nor predicted has the Dice None).

    images / labels: as Segmenter takes them (8-bit [H,W,3|4] images; integer label maps at the images' sizes, values outside
    [0, num_classes) are skipped); they are uploaded once.  levels: {kind: sequence} overriding DEFAULT_LEVELS.  Each cell is
    perturb(images, kind, level, cell_seed(seed, kind index in PERTURBATIONS, level index)) -> Segmenter(model,
    **segmenter_kw)(..., labels=) -> the sum of the per-image confusion counts -> MetricsHistory.  Identity levels are the
    clean run, computed once.  heatmaps / points go to the Segmenter unperturbed (prompt models)."""
    import torch
    from .inference import Segmenter, _as_tensor
    perturbations = tuple(perturbations)
    lv = dict(DEFAULT_LEVELS)
    lv.update(levels or {})
    for kind in perturbations:
        _check_kind(kind)
        for x in lv[kind]:
            _check_level(kind, x)
    if len(labels) != len(images):
        raise ValueError(f"{len(labels)} label maps for {len(images)} images")
    segmenter = Segmenter(model, **segmenter_kw)
    param = next(model.parameters(), None)
    if param is None:
        raise ValueError("the model has no parameters")
    dev = param.device
    if dev.type != "cuda":
        raise RuntimeError("robustness_sweep: the model is not on a GPU -- image_segmentation_amd has no CPU path")
    imgs = [im.to(dev, non_blocking=True) for im in _check_images(images)]
    labs = [_as_tensor(lb).to(dev, non_blocking=True) for lb in labels]

    def score(batch):
        preds = segmenter(batch, heatmaps=heatmaps, labels=labs, points=points)
        M = torch.stack([p.confusion for p in preds]).sum(dim=0)
        return _metrics(M, num_classes, ignore_index)

    clean = score([im[..., :3] for im in imgs])
    result = {}
    for kind in perturbations:
        ki = PERTURBATIONS.index(kind)
        cells = [clean if is_identity(kind, x) else score(perturb(imgs, kind, x, cell_seed(seed, ki, li)))
                 for li, x in enumerate(lv[kind])]
        result[kind] = {"levels": [float(x) for x in lv[kind]],
                        "dice": [c[0] for c in cells], "iou": [c[1] for c in cells], "accuracy": [c[2] for c in cells],
                        "per_class_dice": [c[3] for c in cells]}
    return result
