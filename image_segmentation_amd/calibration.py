"""Confidence calibration: measure the 8-bit confidence map of a Prediction, fit the one scalar that
repairs it, apply it at prediction.

    preds = Segmenter(model, return_scores=True)(images)
    rel = reliability(preds, labels, num_classes=4)           # device histogram, segk_calib_hist
    rel.ece(), rel.bins(), rel.per_class()
    fit = fit_temperature(model, images, labels)              # one segk_calib_temps launch per image, one host sync
    preds = Segmenter(model, temperature=fit.temperature, return_scores=True)(images)

The kernels count in integers (csrc/calib.hip); everything after them -- bins, ECE, MCE, the mean NLL and the parabola -- is
float64 arithmetic on the host over at most 32 x 256 x 2 counters.  The reference holds no code for calibration: the
definition is this project's (tests/calibration_reference.py restates it in NumPy)."""
import math
from dataclasses import dataclass, asdict
from typing import List, Optional

import numpy as np
import torch

from . import _lib, ops
from . import inference as I
from . import utils as U

MAX_TEMPS = _lib.MAX_TEMPS
NLL_ONE = 65536            # fixed point of the NLL sums: 2^-16 nat


# ---- host arithmetic on a [256][2] (count, correct) table -----------------------------------------------------------------
def bin_of(q, n):
    """Bin of the 8-bit confidence q among n equal bins: q n // 256"""
    return q * n // 256


def _bins(table, n):
    table = np.asarray(table, dtype=np.int64).reshape(256, 2)
    if not 1 <= int(n) <= 256:
        raise ValueError(f"bins: 1..256, got {n}")
    n = int(n)
    q = np.arange(256)
    b = bin_of(q, n)
    out = []
    for k in range(n):
        sel = b == k
        qs = q[sel]
        count = int(table[sel, 0].sum())
        correct = int(table[sel, 1].sum())
        row = {"lo": int(qs[0]), "hi": int(qs[-1]), "count": count, "correct": correct, "conf": None, "acc": None}
        if count:
            row["conf"] = float((table[sel, 0].astype(np.float64) * (qs / 255.0)).sum() / count)
            row["acc"] = correct / count
        out.append(row)
    return out


def _ece(rows):
    N = sum(r["count"] for r in rows)
    if N == 0:
        return None
    return float(sum(r["count"] / N * abs(r["acc"] - r["conf"]) for r in rows if r["count"]))


def _mce(rows):
    gaps = [abs(r["acc"] - r["conf"]) for r in rows if r["count"]]
    return float(max(gaps)) if gaps else None


class Reliability:
    """The reliability histogram of a set of predictions: hist int64 [C,256,2], hist[m][q] = (pixels predicted as class m at
    confidence q, those of them that are right), on the device until counts() is asked for."""

    def __init__(self, hist, num_classes):
        hist = torch.as_tensor(hist)
        if hist.dtype != torch.int64 or tuple(hist.shape) != (int(num_classes), 256, 2):
            raise ValueError(f"Reliability: an int64 [{num_classes},256,2] histogram, got {hist.dtype} {tuple(hist.shape)}")
        self.hist, self.num_classes = hist, int(num_classes)

    def add_(self, other):
        if not isinstance(other, Reliability) or other.num_classes != self.num_classes:
            raise ValueError("Reliability: histograms of the same number of classes add")
        self.hist += other.hist.to(self.hist.device)
        return self

    def __add__(self, other):
        return Reliability(self.hist.clone(), self.num_classes).add_(other)

    def counts(self):
        """The histogram as a NumPy int64 [C,256,2] array (synchronises)."""
        return self.hist.detach().cpu().numpy()

    def bins(self, n=15):
        """n rows {lo, hi, count, correct, conf, acc}: bin b holds the confidences lo..hi with q n // 256 == b; conf is the
        mean of q / 255 over its pixels, acc the share that is right (None for an empty bin)."""
        return _bins(self.counts().sum(axis=0), n)

    def ece(self, n=15):
        """Expected calibration error: sum_b N_b / N |acc_b - conf_b|; None without pixels"""
        return _ece(self.bins(n))

    def mce(self, n=15):
        """Maximum calibration error over the non-empty bins; None without pixels"""
        return _mce(self.bins(n))

    def per_class(self, n=15):
        """The same per predicted class: a list of {class, pixels, ece, mce, bins}"""
        out = []
        for c, table in enumerate(self.counts()):
            rows = _bins(table, n)
            out.append({"class": c, "pixels": int(table[:, 0].sum()), "ece": _ece(rows), "mce": _mce(rows), "bins": rows})
        return out

    def to_json(self, n=15):
        rows = self.bins(n)
        return {"num_classes": self.num_classes, "pixels": sum(r["count"] for r in rows), "ece": _ece(rows), "mce": _mce(rows),
                "bins": rows, "per_class": self.per_class(n)}


def _ignore(ignore_index, C):
    if ignore_index is None:
        return -1
    if int(ignore_index) != ignore_index or int(ignore_index) < -1:
        raise ValueError(f"ignore_index: a class index, None or -1, got {ignore_index!r}")
    return int(ignore_index)


def reliability(predictions, labels, num_classes, ignore_index=None, out=None):
    """Reliability histogram of Segmenter predictions against label maps at the images' own sizes: one segk_calib_hist launch
    per image into one device buffer, no host sync.  Uses Prediction.raw_mask where clean= was used (the confidence belongs to
    the raw argmax).  A pixel counts when 0 <= label < num_classes and label != ignore_index.  out: a Reliability to add to."""
    predictions = list(predictions)
    C = int(num_classes)
    if not 1 <= C <= _lib.MAX_CLASSES:
        raise ValueError(f"num_classes: 1..{_lib.MAX_CLASSES}, got {num_classes}")
    if len(labels) != len(predictions):
        raise ValueError(f"{len(labels)} label maps for {len(predictions)} predictions")
    ign = _ignore(ignore_index, C)
    for k, p in enumerate(predictions):
        if getattr(p, "confidence", None) is None:
            raise ValueError(f"prediction {k} has no confidence map: Segmenter sets one with tta=, tiles= or return_scores=True "
                             "(and for an ensemble)")
    if out is not None and (not isinstance(out, Reliability) or out.num_classes != C):
        raise ValueError(f"out: a Reliability of {C} classes")
    if not predictions:
        return out if out is not None else Reliability(torch.zeros((C, 256, 2), dtype=torch.int64), C)
    dev = predictions[0].confidence.device
    ops._require_cuda(predictions[0].confidence, "reliability")
    if out is None:
        out = Reliability(torch.zeros((C, 256, 2), dtype=torch.int64, device=dev), C)
    if out.hist.device != dev or not out.hist.is_contiguous():
        raise ValueError("out: its histogram lives on the predictions' device, contiguous")
    with torch.cuda.device(dev):
        for k, p in enumerate(predictions):
            conf = p.confidence.contiguous()
            mask = (p.raw_mask if p.raw_mask is not None else p.mask).contiguous()
            if conf.dtype != torch.uint8 or mask.dtype != torch.uint8 or conf.ndim != 2 or conf.shape != mask.shape:
                raise ValueError(f"prediction {k}: confidence and mask are uint8 [H,W] maps of one size")
            H, W = (int(a) for a in conf.shape)
            lab = I._label_on(labels[k], (H, W), dev, k)
            _lib.call("segk_calib_hist", conf.data_ptr(), mask.data_ptr(), lab.data_ptr(), H, W, C, ign, out.hist.data_ptr(),
                      ops._stream())
    return out


# ---- temperature --------------------------------------------------------------------------------------------------------------
def default_temperatures():
    """T_j = 2^(-2 + j/4), j = 0..16: 0.25 .. 4, T_8 == 1.0 exactly"""
    return [2.0 ** (-2 + j / 4) for j in range(17)]


def inverse_temperatures(temps):
    """The float32 table the kernel multiplies by: 1/T in float64, rounded once"""
    return (1.0 / np.asarray(temps, dtype=np.float64)).astype(np.float32)


def refine_temperature(temps, nll):
    """(T*, index, at_end): the grid argmin (the first minimum; None entries are skipped), refined by the vertex of the parabola
    through the three points around it in log T.  At either end of the grid, beside a None, or where the three points are on a
    line, the grid point itself is reported; at_end flags the first case (the grid should be extended)."""
    temps = [float(t) for t in temps]
    if len(temps) != len(nll) or not temps:
        raise ValueError(f"{len(temps)} temperatures and {len(nll)} NLL values")
    live = [j for j, v in enumerate(nll) if v is not None and math.isfinite(v)]
    if not live:
        return None, None, False
    i = min(live, key=lambda j: (nll[j], j))
    if i == 0 or i == len(temps) - 1:
        return temps[i], i, True
    if nll[i - 1] is None or nll[i + 1] is None or not (math.isfinite(nll[i - 1]) and math.isfinite(nll[i + 1])):
        return temps[i], i, False
    x0, x1, x2 = (math.log(temps[j]) for j in (i - 1, i, i + 1))
    y0, y1, y2 = (float(nll[j]) for j in (i - 1, i, i + 1))
    den = (x1 - x0) * (y1 - y2) - (x1 - x2) * (y1 - y0)
    if den == 0.0:
        return temps[i], i, False
    x = x1 - 0.5 * ((x1 - x0) ** 2 * (y1 - y2) - (x1 - x2) ** 2 * (y1 - y0)) / den
    x = min(max(x, min(x0, x2)), max(x0, x2))
    return math.exp(x), i, False


@dataclass
class TemperatureFit:
    """What fit_temperature returns; plain numbers and lists (json.dump takes to_json())."""
    temperature: Optional[float]          # T*: the refined grid argmin of the mean NLL (None without scored pixels)
    index: Optional[int]                  # the grid argmin
    at_grid_end: bool                     # the argmin is the first or last grid point: not refined, extend temps=
    temperatures: List[float]             # the grid
    nll: List[Optional[float]]            # mean NLL per temperature, nat per pixel
    ece: List[Optional[float]]            # ECE (15 bins) per temperature, from the same pass
    nonfinite: List[int]                  # pixels left out of a temperature's mean: their NLL was not finite
    nll_at_1: Optional[float]             # the values at T = 1 (None when 1.0 is not on the grid)
    ece_at_1: Optional[float]
    nll_best: Optional[float]             # the values at the grid argmin
    ece_best: Optional[float]
    pixels: int                           # valid pixels

    def to_json(self):
        return asdict(self)


def fit_from_counts(temps, hist, nll_fx, nonfinite, valid, bins=15):
    """The fit record from the integer outputs of segk_calib_temps (host arrays): hist [K,256,2], nll_fx [K], nonfinite [K]."""
    temps = [float(t) for t in temps]
    hist = np.asarray(hist, dtype=np.int64).reshape(len(temps), 256, 2)
    valid = int(valid)
    nll, ece = [], []
    for j in range(len(temps)):
        n = valid - int(nonfinite[j])
        nll.append(int(nll_fx[j]) / NLL_ONE / n if n > 0 else None)
        ece.append(_ece(_bins(hist[j], bins)))
    T, i, end = refine_temperature(temps, nll)
    one = temps.index(1.0) if 1.0 in temps else None
    return TemperatureFit(T, i, end, temps, nll, ece, [int(v) for v in nonfinite], None if one is None else nll[one],
                          None if one is None else ece[one], None if i is None else nll[i], None if i is None else ece[i], valid)


def _check_temps(temps):
    temps = default_temperatures() if temps is None else [float(t) for t in temps]
    if not 1 <= len(temps) <= MAX_TEMPS:
        raise ValueError(f"temps: 1..{MAX_TEMPS} temperatures, got {len(temps)}")
    if any(not (t > 0 and math.isfinite(t)) for t in temps):
        raise ValueError(f"temps: positive finite numbers, got {temps}")
    return temps


def fit_temperature(model, images, labels, target_size=224, interpolation="bilinear", antialias=None, temps=None,
                    ignore_index=None, batch_size=32):
    """Temperature scaling of one model that returns logits: the mean NLL and the ECE of every temperature of `temps`
    (default_temperatures()) over the images, evaluated at the images' own sizes, and the refined argmin.

    images / labels: as Segmenter takes them (ragged float [C,H,W] or uint8 [H,W,C] images; integer [H,W] / [1,H,W] maps; a
    pixel counts when 0 <= label < C and label != ignore_index).  Slots are filled as Segmenter fills them, one forward runs
    per chunk of batch_size images and one segk_calib_temps launch per image adds into one set of device accumulators; the
    host waits once, at the end.  Returns a TemperatureFit."""
    if isinstance(model, (list, tuple)):
        raise ValueError("fit_temperature takes one model: fit each model of an ensemble on its own and pass Segmenter one "
                         "temperature per model")
    if I._is_prompt_model(model):
        raise ValueError("fit_temperature needs logits: a PromptModel returns probabilities (its calibration is out of scope)")
    if I._arity(model):
        raise ValueError("fit_temperature takes models whose forward takes the image alone")
    if interpolation not in (U.BILINEAR, U.NEAREST):
        raise ValueError(f"interpolation: '{U.BILINEAR}' or '{U.NEAREST}', got {interpolation!r}")
    T, bs = int(target_size), int(batch_size)
    if T < 1 or bs < 1:
        raise ValueError("batch_size and target_size are positive")
    fixed = I._fixed_input_size(model)
    if fixed is not None and T != fixed:
        raise ValueError(f"the model is a ClipUNet whose ViT takes {fixed} x {fixed} inputs only: target_size must be {fixed}")
    temps = _check_temps(temps)
    K = len(temps)
    images = [I._as_tensor(im) for im in images]
    if len(labels) != len(images):
        raise ValueError(f"{len(labels)} label maps for {len(images)} images")
    C0 = I._num_classes(model)
    if C0 is not None and C0 > _lib.MAX_CLASSES:
        raise ValueError(f"the model has {C0} classes, calibration supports at most {_lib.MAX_CLASSES}")
    param = next(model.parameters(), None)
    if param is None:
        raise ValueError("the model has no parameters")
    ops._require_cuda(param, "fit_temperature")
    dev = param.device
    mode = 1 if interpolation == U.NEAREST else 0
    with I._eval_mode([model]), torch.no_grad(), torch.cuda.device(dev):
        inv = torch.from_numpy(inverse_temperatures(temps)).to(dev)
        acc = torch.zeros(K * 512 + 2 * K + 1, dtype=torch.int64, device=dev)      # hist, nll_fx, nonfinite, valid
        hist, nll_fx, nonf, valid = acc[:K * 512], acc[K * 512:K * 513], acc[K * 513:K * 514], acc[K * 514:]
        for i in range(0, len(images), bs):
            chunk = [im.to(dev, non_blocking=True) for im in images[i:i + bs]]
            X, _, metas = I._slots(dev, chunk, None, T, interpolation, antialias)
            y = I._forward(model, X, None, ("the model", "fit_temperature"))
            C = int(y.shape[1])
            if C > _lib.MAX_CLASSES:
                raise ValueError(f"the model has {C} classes, calibration supports at most {_lib.MAX_CLASSES}")
            ign = _ignore(ignore_index, C)
            s = ops._stream()
            for k, meta in enumerate(metas):
                pl, pt, _, _ = meta["pad"]
                nh, nw = meta["new_size"]
                oh, ow = meta["original_size"]
                lab = I._label_on(labels[i + k], (oh, ow), dev, i + k)
                _lib.call("segk_calib_temps", y[k].data_ptr(), C, T, pt, pl, nh, nw, oh, ow, mode, lab.data_ptr(), ign,
                          inv.data_ptr(), K, hist.data_ptr(), nll_fx.data_ptr(), nonf.data_ptr(), valid.data_ptr(), s)
        host = acc.cpu().numpy()                      # the one host sync
    return fit_from_counts(temps, host[:K * 512], host[K * 512:K * 513], host[K * 513:K * 514], host[K * 514])
