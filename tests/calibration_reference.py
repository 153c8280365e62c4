"""NumPy restatement of confidence calibration (segk_calib_hist, segk_calib_temps and the host arithmetic of
image_segmentation_amd/calibration.py).  There is no reference code for this feature: the project defines the result and
this file pins it.  Host-only.

  hist_reference   the per-class reliability histogram of (confidence, mask, labels)
  sweep            the temperature sweep in float64, or in float32 with the kernel's expression order and its fixed point
  bins / ece / mce / mean_nll / refine   the arithmetic after the counters
  case / TABLE     the inputs tests/test_gpu_calibration.py runs (tests/test_calibration_host.py checks them on the host)"""
import math

import numpy as np

import tta_reference as R
from oracle.fill import fill, labels

NLL_MAX = 262144.0            # SEGK_CALIB_NLL_MAX
IGNORE = 1                    # the class the cases name as ignore_index (where C > 2)


def valid_labels(lab, C, ignore_index=-1):
    lab = np.asarray(lab).reshape(-1)
    ok = (lab >= 0) & (lab < C)
    if ignore_index is not None and ignore_index >= 0:
        ok &= lab != ignore_index
    return ok


def hist_reference(conf, mask, lab, C, ignore_index=-1):
    """int64 [C,256,2]: every valid pixel adds 1 to [m][q][0] and, when m == l, to [m][q][1]; a mask value >= C counts under
    class C - 1 and is never correct"""
    conf, mask, lab = (np.asarray(a).reshape(-1).astype(np.int64) for a in (conf, mask, lab))
    ok = valid_labels(lab, C, ignore_index)
    out = np.zeros((C, 256, 2), dtype=np.int64)
    cls = np.minimum(mask, C - 1)
    np.add.at(out, (cls[ok], conf[ok], 0), 1)
    hit = ok & (mask == lab)
    np.add.at(out, (cls[hit], conf[hit], 1), 1)
    return out


def inverse_temperatures(temps):
    """1/T in float64, rounded once to float32: the device table"""
    return (1.0 / np.asarray(temps, dtype=np.float64)).astype(np.float32)


def sweep(slot, geo, shape, lab, C, inv_T, ignore_index=-1, mode=0, dtype=np.float64):
    """The sweep over the VALID pixels of one image.  slot [C,T,T] float32 logits; geo: pad_top, pad_left, nh, nw; inv_T the
    float32 table.  dtype float64: plain float64 arithmetic on the float32 inputs.  dtype float32: every operation in float32
    in the kernel's order (NumPy's exp / log stand in for expf / logf), then the kernel's fixed point.
    -> dict: z [C,n], best [n], lab [n], p_best [K,n], c = 255 p_best + 0.5 [K,n] (before the cast), q [K,n], nll [K,n],
       hist int64 [K,256,2], valid n, and (float32 only) nll_fx [K], nonfinite [K]"""
    ft = np.dtype(dtype).type
    oh, ow = shape
    view = dict(geo, slot=np.asarray(slot)[:C], flip=0)
    ok = valid_labels(lab, C, ignore_index)
    l = np.asarray(lab).reshape(-1)[ok].astype(np.int64)
    K = len(inv_T)
    with np.errstate(all="ignore"):
        z = R.sample_view(view, oh, ow, mode, ft).reshape(C, -1)[:, ok]
        best = R.argmax_first_nan_max(z)
        n = z.shape[1]
        out = dict(z=z, best=best, lab=l, valid=int(n), p_best=np.zeros((K, n), ft), c=np.zeros((K, n), ft),
                   q=np.zeros((K, n), np.int64), nll=np.zeros((K, n), ft), hist=np.zeros((K, 256, 2), np.int64))
        if ft is np.float32:
            out["nll_fx"], out["nonfinite"] = [0] * K, [0] * K
        cols = np.arange(n)
        for j in range(K):
            s = (z * ft(inv_T[j])).astype(ft)
            mx = s[0]
            for k in range(1, C):
                mx = np.where(s[k] > mx, s[k], mx)
            e = np.exp(s - mx[None]).astype(ft)
            S = np.zeros(n, ft)
            for k in range(C):
                S = S + e[k]
            p = (e / S[None]).astype(ft)
            ps = np.zeros(n, ft)
            for k in range(C):
                ps = ps + p[k]
            pb = (p[best, cols] / ps).astype(ft)
            c = ft(255) * pb + ft(0.5)
            q = np.where(c >= 0, np.minimum(c, ft(255)), ft(0)).astype(np.int64)       # a NaN confidence is stored as 0
            nll = (np.log(S).astype(ft) - (s[l, cols] - mx)).astype(ft)
            out["p_best"][j], out["c"][j], out["q"][j], out["nll"][j] = pb, c, q, nll
            np.add.at(out["hist"][j], (q, 0), 1)
            np.add.at(out["hist"][j], (q[best == l], 1), 1)
            if ft is np.float32:
                fin = nll < np.float32(NLL_MAX)                                       # false for NaN and inf too
                fx = np.floor(np.maximum(nll[fin], 0).astype(np.float64) * 65536.0 + 0.5).astype(np.uint64)
                out["nll_fx"][j] = int(fx.astype(object).sum()) if fx.size else 0
                out["nonfinite"][j] = int((~fin).sum())
    return out


def mean_nll(sw, j):
    """mean of the finite per-pixel NLL values of temperature j (None without any)"""
    v = sw["nll"][j].astype(np.float64)
    v = v[v < NLL_MAX]
    return float(np.maximum(v, 0).mean()) if v.size else None


# ---- after the counters ------------------------------------------------------------------------------------------------------
def bins(table, n):
    """table [256][2] -> n rows (lo, hi, count, correct, conf, acc): bin b holds the q with q n // 256 == b"""
    table = np.asarray(table, dtype=np.int64).reshape(256, 2)
    rows = []
    for b in range(n):
        qs = [q for q in range(256) if q * n // 256 == b]
        count = sum(int(table[q, 0]) for q in qs)
        correct = sum(int(table[q, 1]) for q in qs)
        conf = math.fsum(int(table[q, 0]) * (q / 255.0) for q in qs) / count if count else None
        rows.append((qs[0], qs[-1], count, correct, conf, correct / count if count else None))
    return rows


def ece(table, n=15):
    rows = bins(table, n)
    N = sum(r[2] for r in rows)
    return math.fsum(r[2] / N * abs(r[5] - r[4]) for r in rows if r[2]) if N else None


def mce(table, n=15):
    gaps = [abs(r[5] - r[4]) for r in bins(table, n) if r[2]]
    return max(gaps) if gaps else None


def refine(temps, nll):
    """grid argmin, then the vertex of the parabola through its three points in log T (Lagrange form); the grid point at
    either end -> (T*, index, at_end)"""
    i = int(np.argmin(nll))
    if i == 0 or i == len(temps) - 1:
        return float(temps[i]), i, True
    x = [math.log(temps[j]) for j in (i - 1, i, i + 1)]
    y = [float(nll[j]) for j in (i - 1, i, i + 1)]
    a = np.polyfit(np.asarray(x) - x[1], y, 2)
    return (float(temps[i]) if a[0] <= 0 else math.exp(x[1] - a[1] / (2 * a[0]))), i, False


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------
SHAPES = [(37, 53), (500, 375), (20, 30), (33, 65), (64, 17)]
SIZES = (64, 224)
CLASSES = (1, 2, 3, 4, 5, 8)
# 32 temperatures: the default grid 2^(-2 + j/4), j = 0..16 (entry 8 is 1.0), then 15 more between its points
TABLE = [2.0 ** (-2 + j / 4) for j in range(17)] + [2.0 ** (-2 + (j + 0.5) / 4) for j in range(15)]
KS = {1: slice(8, 9), 17: slice(0, 17), 32: slice(0, 32)}          # K -> the part of TABLE a launch reads


def geometry(shape, T):
    from image_segmentation_amd.utils import _geometry
    nh, nw, pt, pl, _ = _geometry(shape[0], shape[1], T)
    return dict(pad_top=pt, pad_left=pl, nh=nh, nw=nw)


def field(C, T, seed):
    """float32 [C,T,T] logits: per class a plane wave of amplitude 4 (0.5 .. 2 periods across the slot per axis) plus white
    noise in (-0.15, 0.15).  A white field in (-3, 3) has neighbour differences of up to 6, and the float32 rounding of a
    bilinear tap position (about 1.5e-5 of a pixel at these sizes) then moves z by 1e-4 and, at 1/T = 4, one pixel in five
    into the ambiguity window (measured on the host); this field keeps the share below 2 % while the amplitude still fills
    the top bin at 1/T = 1."""
    par = fill((C, 3), seed, 0, 1).numpy().astype(np.float64)
    y, x = np.meshgrid(np.arange(T) / T, np.arange(T) / T, indexing="ij")
    f = np.stack([4 * np.sin(2 * np.pi * ((0.5 + 1.5 * par[k, 0]) * y + (0.5 + 1.5 * par[k, 1]) * x + par[k, 2])) for k in range(C)])
    return (f + fill((C, T, T), seed + 1, -0.15, 0.15).numpy()).astype(np.float32)


def case(n, T, C):
    """(shape, geo, slot float32 [C,T,T], labels int64 [oh,ow], ignore_index): labels over the classes with 255 sprinkled in,
    and class IGNORE named as ignore_index where there are more than two classes"""
    shape = SHAPES[n]
    slot = field(C, T, 7 + 2 * n + 31 * C + T)
    lab = labels(shape, 40 + n + C, C).numpy()
    lab[::7, ::5] = 255
    return shape, geometry(shape, T), slot, lab, (IGNORE if C > 2 else -1)


def ambiguous(s64, d_p, d_z):
    """bool [K,n]: pixels whose bin float32 arithmetic may move -- the float64 255 p_best + 0.5 within 255 4 d_p[j] of an
    integer, or the float64 top-two gap of z below twice the z distance"""
    c = s64["c"]
    near = np.abs(c - np.round(c)) <= 255 * 4 * np.asarray(d_p)[:, None]
    if s64["z"].shape[0] > 1:
        top = np.sort(s64["z"], axis=0)[-2:]
        near = near | ((top[1] - top[0]) < 2 * d_z)[None]
    return near


def distances(s32, s64):
    """(d_nll [K], d_p [K], d_z): the float32 restatement's largest per-pixel distances from float64"""
    d_nll = np.abs(s32["nll"].astype(np.float64) - s64["nll"]).max(axis=1) if s64["valid"] else np.zeros(len(s64["nll"]))
    d_p = np.abs(s32["p_best"].astype(np.float64) - s64["p_best"]).max(axis=1) if s64["valid"] else np.zeros(len(s64["nll"]))
    d_z = float(np.abs(s32["z"].astype(np.float64) - s64["z"]).max()) if s64["valid"] else 0.0
    return d_nll, d_p, d_z
