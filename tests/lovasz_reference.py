"""float64 reference, analytic gradient, float32 restatement, case table and error bounds for the Lovasz-Softmax kernels of
csrc/lovasz.hip, shared by tests/test_lovasz_host.py and tests/test_gpu_lovasz.py.  NumPy only.  Nothing here is
taken from what the kernels return.

Semantics, on logits z [N, C, H, W] fp32, labels y [N, H, W], class weights w (fp32, 1 when absent):

  a pixel COUNTS when 0 <= y < C and y != ignore_index;  segments: per_image -> S = N of L = H W pixels, else S = 1, L = N H W
  p = softmax(z);  for every class c: fg = [y = c],  err_c = fg ? sum_{k != c} p_k : p_c
  word = bits(fp32 err_c) + 1, NAN_WORD for a NaN, 0 for a pixel that does not count;  payload = (fg << 31) | index-in-segment
  order inside (s, c): word descending, index ascending (stable);  G = fg slots, F_i = fg slots among sorted positions 1..i
  J_i = 1 - (G - F_i) / (G + i - F_i), J_0 = 0, g_i = J_i - J_{i-1}  (float64 from integers);  L_{s,c} = sum_i err_i g_i
  c ENTERS s iff s has a counted pixel and (classes == "all" or G_{s,c} > 0)
  loss_s = sum_{c enters} w_c L_{s,c} / sum_{c enters} w_c  (0 when nothing enters or the weights sum to 0);  loss = mean_s loss_s
  coef_c(pixel) = g_i at its sorted position, negated when fg, 0 when the pixel does not count
  a_{s,c} = fp32(w_c / (S sum_{c' enters} w_c')) for entering classes, else 0
  d loss / d z_j = gout sum_c a_{s,c} coef_c p_c ([j = c] - p_j)

Error bound of an error.  A probability errs by K_SM 2^-24 p_k (C + max - z_k) (loss_reference.py: measured there, 4 x margin
included).  With e_p_k = p_k (C + max - z_k), the error of a class carries, in units of 2^-24,
  unit_e = e_p_c                               (fg == 0: the probability itself)
         = sum_{k != c} e_p_k + C u            (fg == 1: the C-term chain u = sum_{k != c} p_k)
k_e = max |err32 - err64| / (2^-24 unit_e + 2^-126) is MEASURED on the host by hard_loss_reference.py's method: the float32 NumPy
restatement (the kernel's operations in the kernel's order, expf taken as the correctly rounded one) against float64 over the
whole case table.  Measured: k_e <= 1.053 (tests/test_lovasz_host.py measures again and asserts that no case exceeds a quarter of
the constant).  The device is allowed four times that, the project's standing margin for the device math library, rounded up to
two digits: K_E = 4.3.

Loss bound (derived).  L_{s,c} is 1-Lipschitz in the max norm of the error vector (g >= 0, sum g = 1, and the Lovasz extension of
a submodular function is the maximum of such linear forms), the class weights are normalised and the mean over segments is a
convex combination, so |loss_dev - loss_64| <= max err_bound + 2^-24 |loss| (the final fp32 rounding) + 1e-12 (the float64 sums).
Equal errors may come in another order on the device: L does not depend on the order inside a group of equal errors.

Gradient bound (derived), against the float64 formula evaluated with the DEVICE's coef and a (its permutation), per element, with
t_c = a_c coef_c p_c, A = sum_c t_c, d_j = t_j - p_j A, in units of 2^-24:
  unit_g_j = K_SM (|a_j coef_j| e_p_j + |A| e_p_j + p_j sum_c |a_c coef_c| e_p_c)      what the probabilities carry
             + 2 |t_j| + p_j (C + 2) sum_c |t_c| + 2 |p_j A| + 2 |d_j|                 the products, the C-term chain, gout"""
import functools
import math

import numpy as np

from bn_reference import U24
from hard_loss_reference import rows, unrows, f32
from loss_reference import K_SM, TINY

MAXC = 8
TILE = 2048                      # SEGK_LOVASZ_TILE
NAN_WORD = 0x3FFFFFFF
K_E = 4.3
F32, F64 = np.float32, np.float64


def scratch_words(C, P, S):
    """SEGK_LOVASZ_SCRATCH_WORDS of include/segk.h, written out independently of ops.py"""
    TS = (P // S + TILE - 1) // TILE
    NT = C * S * TS
    return 2 * NT + 4 * C * P + 256 * NT + 256 * C * S + NT + NT + 2 * C * S


def layout(C, P, S):
    """word offsets of the pieces of the scratch buffer the header documents"""
    TS = (P // S + TILE - 1) // TILE
    NT = C * S * TS
    o = dict(part=0, words=2 * NT, pays=2 * NT + C * P)
    o["gn"] = scratch_words(C, P, S) - 2 * C * S
    return o


def state_doubles(C, S):
    return 2 + 4 * C * S + S


# ---------------------------------------------------------------------------------------- words
def words_of(err32, counted):
    """uint32 words [P, C]: bits(err) + 1, NAN_WORD for a NaN error, 0 for a pixel that does not count"""
    e = np.ascontiguousarray(err32, dtype=F32)
    w = e.view(np.uint32).astype(np.uint64) + 1
    w = np.where(np.isnan(e), NAN_WORD, w)
    return np.where(np.asarray(counted)[:, None], w, 0).astype(np.uint32)


def word_value(words):
    """the errors the words stand for, float64 (NaN for NAN_WORD; 0 for the word 0, which stands for nothing)"""
    w = np.asarray(words, dtype=np.uint32)
    v = (np.where(w == 0, 1, w) - 1).astype(np.uint32).view(F32).astype(F64)
    return np.where(w == NAN_WORD, np.nan, np.where(w == 0, 0.0, v))


def stable_order(words):
    """the permutation of one segment: words descending, ties by index ascending"""
    return np.argsort(-np.asarray(words).astype(np.int64), kind="stable")


def coefficients(fg_sorted):
    """g_i of a sorted fg pattern (bool / 0-1 array), float64 from integers"""
    fg = np.asarray(fg_sorted).astype(np.int64)
    n = len(fg)
    if n == 0:
        return np.zeros(0, dtype=F64)
    G = int(fg.sum())
    F = np.cumsum(fg)
    i = np.arange(1, n + 1, dtype=np.int64)
    J = 1.0 - (G - F).astype(F64) / (G + i - F).astype(F64)
    return np.diff(np.concatenate([[0.0], J]))


# ---------------------------------------------------------------------------------------- per pixel
def _weights(cw, C):
    return np.ones(C, dtype=F64) if cw is None else np.asarray(cw, dtype=F32).astype(F64)


def pixel_terms(zr, y, ignore_index, dt):
    """p [P, C], err [P, C], counted [P], fg [P, C], gap [P, C] = max - z in dtype dt (float32: the kernel's operations in the
    kernel's order, expf evaluated in float64 and rounded once)"""
    P, C = zr.shape
    z = zr.astype(dt)
    with np.errstate(all="ignore"):
        m = np.full(P, -np.inf, dtype=dt)
        for k in range(C):
            m = np.fmax(m, z[:, k])
        e = np.exp((z - m[:, None]).astype(dt).astype(F64)).astype(dt)
        se = np.zeros(P, dtype=dt)
        for k in range(C):
            se = (se + e[:, k]).astype(dt)
        inv = (dt(1) / se).astype(dt)
        p = (e * inv[:, None]).astype(dt)
        ign = -1 if ignore_index is None else int(ignore_index)
        counted = (y >= 0) & (y < C) & (y != ign)
        fg = (np.arange(C)[None, :] == y[:, None]) & counted[:, None]
        u = np.zeros(P, dtype=dt)
        for k in range(C):
            u = (u + np.where(y != k, p[:, k], dt(0))).astype(dt)
        err = np.where(fg, u[:, None], p).astype(dt)
        gap = (m[:, None] - z).astype(F64)
    return dict(p=p, err=err, counted=counted, fg=fg, gap=gap, u=u)


def entering_weights(enters, w, S):
    """(den [S], a [S, C] fp32) of the module docstring; den is added in class order from 0.0, as the kernel adds it"""
    den = np.zeros(enters.shape[0], dtype=F64)
    for c in range(enters.shape[1]):
        den = den + np.where(enters[:, c], w[c], 0.0)
    safe = np.where(den > 0, den, 1.0)
    a = np.where(enters & (den[:, None] > 0), w[None, :] / (S * safe)[:, None], 0.0).astype(F32)
    return den, a


def lovasz_reference(z, y, cw=None, ignore_index=None, per_image=False, classes="present", dt=F64):
    """z [N, C, H, W] fp32, y [N, H, W] int64 -> dict.  dt = float64: the errors are ordered as float64 values; dt = float32: as
    the words of the float32 restatement, which is what the device sorts if its expf equals the correctly rounded one"""
    assert classes in ("present", "all")
    N, C, H, W = z.shape
    P = N * H * W
    S = N if per_image else 1
    L = P // S
    zin = np.asarray(z)
    zin = zin if (zin.dtype == F64 and dt is F64) else zin.astype(F32)      # float64 logits: finite differences of the reference
    zr, yr = rows(zin), np.asarray(y).reshape(-1).astype(np.int64)
    t = pixel_terms(zr, yr, ignore_index, dt)
    err, counted, fg = t["err"], t["counted"], t["fg"]
    w = _weights(cw, C)
    if dt is F32:
        key = words_of(err, counted).astype(np.int64)
        val = word_value(words_of(err, counted))
    else:
        with np.errstate(all="ignore"):
            key = np.where(np.isnan(err), np.inf, err.astype(F64))
        key = np.where(counted[:, None], key, -1.0)
        val = err.astype(F64)
    coef = np.zeros((C, P), dtype=F64)
    Lsc, G = np.zeros((S, C), dtype=F64), np.zeros((S, C), dtype=np.int64)
    n_s = np.zeros(S, dtype=np.int64)
    perm = np.zeros((S, C, L), dtype=np.int64)
    for s in range(S):
        sl = slice(s * L, (s + 1) * L)
        n = int(counted[sl].sum())
        n_s[s] = n
        for c in range(C):
            order = np.argsort(-key[sl, c], kind="stable")
            perm[s, c] = order
            f = fg[sl, c][order][:n]
            g = coefficients(f)
            G[s, c] = int(f.sum())
            with np.errstate(all="ignore"):
                terms = val[sl, c][order][:n] * g
            Lsc[s, c] = float(np.sum(terms)) if n else 0.0
            coef[c, s * L + order[:n]] = np.where(f, -g, g)
    enters = (n_s[:, None] > 0) & ((G > 0) if classes == "present" else np.ones((S, C), dtype=bool))
    den, a = entering_weights(enters, w, S)
    with np.errstate(all="ignore"):
        num = np.where(enters, w[None, :] * Lsc, 0.0).sum(1)
        loss_s = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    loss = float(loss_s.sum() / S)
    t.update(N=N, C=C, H=H, W=W, P=P, S=S, L=L, shape=z.shape, w=w, coef=coef, per_class=Lsc, G=G, n_s=n_s, n=int(n_s.sum()),
             enters=enters, a=a, loss_s=loss_s, loss=loss, perm=perm, val=val, key=key)
    return t


def lovasz_grad_reference(r, gout=1.0, coef=None, a=None):
    """d loss / d z [N, C, H, W] in float64 by the formula, times the fp32 upstream gradient; coef [C, P] and a [S, C] default
    to the reference's own (the GPU test passes the device's)"""
    go = f32(gout)
    coef = r["coef"] if coef is None else np.asarray(coef, dtype=F64)
    a = r["a"] if a is None else a
    P, C, S, L = r["P"], r["C"], r["S"], r["L"]
    p = r["p"].astype(F64)
    seg = np.arange(P) // L
    with np.errstate(all="ignore"):
        t = np.asarray(a, dtype=F64)[seg, :] * coef.T * p            # [P, C]
        A = t.sum(1)
        d = go * (t - p * A[:, None])
    return unrows(np.where(r["counted"][:, None], d, 0.0), r["shape"])


# ---------------------------------------------------------------------------------------- bounds
def _e_p(r):
    with np.errstate(all="ignore"):
        return r["p"].astype(F64) * (r["C"] + r["gap"])


def err_unit(r):
    """unit_e [P, C] of the module docstring (r: a float64 reference)"""
    e_p = _e_p(r)
    others = e_p.sum(1, keepdims=True) - e_p
    with np.errstate(all="ignore"):
        unit = np.where(r["fg"], others + r["C"] * r["u"].astype(F64)[:, None], e_p)
    return np.where(np.isfinite(unit), unit, np.inf)


def err_bound(r):
    """[P, C]: |error| allowed for the device's err_c against float64"""
    return K_E * U24 * err_unit(r) + TINY


def measure(r64, r32):
    """k_e of the module docstring over the counted pixels with finite float64 errors"""
    unit = err_unit(r64)
    ok = r64["counted"][:, None] & np.isfinite(r64["err"]) & np.isfinite(unit)
    with np.errstate(all="ignore"):
        k = np.abs(r32["err"].astype(F64) - r64["err"]) / (U24 * unit + TINY)
    return float(k[ok].max()) if ok.any() else 0.0


def loss_bound(r):
    """|loss_dev - loss_64| allowed (the Lipschitz bound of the module docstring)"""
    eb = err_bound(r)[r["counted"]]
    worst = float(eb.max()) if eb.size else 0.0
    return worst + U24 * abs(r["loss"]) + 1e-12


def grad_bound(r, coef, a, gout=1.0):
    """per element [N, C, H, W] |error| allowed for dlogits against lovasz_grad_reference(r, gout, coef, a)"""
    go = abs(f32(gout))
    P, C, L = r["P"], r["C"], r["L"]
    p, e_p = r["p"].astype(F64), _e_p(r)
    seg = np.arange(P) // L
    with np.errstate(all="ignore"):
        ac = np.abs(np.asarray(a, dtype=F64)[seg, :] * np.asarray(coef, dtype=F64).T)
        t = ac * p
        A = t.sum(1, keepdims=True)                       # an upper bound of |A|
        d = t + p * A
        unit = K_SM * (ac * e_p + A * e_p + p * (ac * e_p).sum(1, keepdims=True)) + 2 * t + p * (C + 2) * A + 2 * p * A + 2 * d
        e = 1.01 * go * U24 * unit + 8 * TINY
    return unrows(np.where(r["counted"][:, None], e, 0.0), r["shape"])


def tie_free_pairs(r, s, c):
    """for segment (s, c) of a float64 reference: bool per adjacent pair (i, i + 1) of its counted sorted positions -- True where
    the float64 errors differ by more than twice the largest bound of the segment.  Every slot in front of such a pair then lies
    above every slot behind it on the device too, whatever the device's errors are inside their bounds"""
    L, n = r["L"], int(r["n_s"][s])
    if n < 2:
        return np.zeros(0, dtype=bool)
    order = r["perm"][s, c][:n]
    v = r["err"][s * L:(s + 1) * L, c].astype(F64)[order]
    b = float(err_bound(r)[s * L:(s + 1) * L, c][order].max())
    with np.errstate(all="ignore"):
        return (v[:-1] - v[1:]) > 2 * b


def guarded_share(r):
    """the share of adjacent pairs of a case that tie_free_pairs leaves undecided"""
    tot = und = 0
    for s in range(r["S"]):
        for c in range(r["C"]):
            d = tie_free_pairs(r, s, c)
            tot += len(d)
            und += int((~d).sum())
    return und / tot if tot else 0.0


# ---------------------------------------------------------------------------------------- case table
# segment lengths: a single slot, a pair, around one wave, around one tile, three tiles, six tiles
LENGTHS = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 17)
BATCHES = (1, 3)
CLASSES = (1, 2, 3, 4, 5, 8)
KINDS = ("normal", "ties", "saturated", "absent", "ignored_image", "outside", "all_ignored")
REGIMES = ("tile_edge", "absent_class", "all_ignored", "heavy_ties", "saturated", "empty_image")


def inputs(kind, C, N, L, seed):
    """logits [N, C, 1, L], labels [N, 1, L], ignore_index of one input family"""
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((N, C, 1, L))).astype(F32)
    y = g.integers(0, C, (N, 1, L)).astype(np.int64)
    ign = None
    if kind == "ties":                       # logits on a grid of 0.5: large groups of equal errors
        z = (np.round(z * 2.0) / 2.0).astype(F32)
    elif kind == "saturated":                # errors of exactly 0 and exactly 1 after rounding: words 1 and bits(1) + 1
        z = np.where(g.random((N, C, 1, L)) < 0.5, F32(60.0), F32(-60.0)).astype(F32)
    elif kind == "absent":                   # the last class is absent from image 0 only
        y[0][y[0] == C - 1] = 0
    elif kind == "ignored_image":            # the last image is all ignore_index
        ign = 255
        y[N - 1] = 255
        y.reshape(-1)[::7] = 255
    elif kind == "outside":                  # labels outside 0 .. C - 1 never count
        y.reshape(-1)[::3] = C
        y.reshape(-1)[1::5] = -3
        ign = 0 if C > 1 else None
    elif kind == "all_ignored":
        ign = 255
        y[...] = 255
    return z, y, ign


@functools.lru_cache(maxsize=None)
def case(C, N, li, per_image):
    """one cell of the table: the input family, the weights and classes = "all" are walked with strides of their own, so that each
    meets every length, class count and both per_image values"""
    L = LENGTHS[li]
    kind = KINDS[(CLASSES.index(C) + li + 2 * N + int(per_image)) % len(KINDS)]
    weighted = (CLASSES.index(C) + li) % 2 == 0
    classes = "all" if (li + N + CLASSES.index(C) // 2) % 3 == 0 else "present"
    gout = 0.5 if (li + C) % 4 == 0 else 1.0
    z, y, ign = inputs(kind, C, N, L, 7000 + 100 * C + 10 * li + N + (5 if per_image else 0))
    cw = (0.5 + 0.25 * np.arange(C)).astype(F32) if weighted else None
    if weighted and C > 2 and li % 2 == 1:
        cw[1] = 0.0                          # a weight of zero takes the class out
    kw = dict(cw=cw, ignore_index=ign, per_image=bool(per_image), classes=classes)
    desc = f"C={C} N={N} L={L} per_image={int(per_image)} {kind} classes={classes} weights={weighted} ignore={ign} gout={gout}"
    return dict(z=z, y=y, kw=kw, gout=gout, kind=kind, desc=desc, L=L)


# the cases whose order is held against float64: tie-free normal logits in segments short enough that at most 1 % of the adjacent
# pairs lie within the guard -- up to 195 slots, and up to one tile with two classes, whose bounds are the smallest
# (tests/test_lovasz_host.py checks the cap on the CPU)
ORDER_CAP = 0.01


def order_case(c):
    N, C = c["z"].shape[:2]
    seg = c["L"] if c["kw"]["per_image"] else N * c["L"]
    return c["kind"] == "normal" and C >= 2 and (seg <= 195 or (C == 2 and seg <= TILE))      # one class: every error is 0


def table():
    return [(C, N, li, pi) for C in CLASSES for N in BATCHES for li in range(len(LENGTHS)) for pi in (False, True)]


# one case above the two levels that engage only past a tile count: a wave of the radix scan walks more than one tile past 16
# tiles per segment, and the fg scan takes a second chunk past 1024 tiles per segment
BIG_L = 1024 * TILE + 1


@functools.lru_cache(maxsize=None)
def big_case():
    z, y, ign = inputs("normal", 2, 1, BIG_L, 7999)
    y.reshape(-1)[5::11] = 255
    kw = dict(cw=None, ignore_index=255, per_image=False, classes="present")
    return dict(z=z, y=y, kw=kw, gout=1.0, kind="normal", desc=f"C=2 N=1 L={BIG_L} (1025 tiles)", L=BIG_L)


def regimes_of(c, r):
    """the regimes of REGIMES a case (with its float64 reference r) populates"""
    out = set()
    if c["L"] in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out.add("tile_edge")
    if ((r["G"] == 0) & (r["n_s"][:, None] > 0)).any():
        out.add("absent_class")
    if r["n"] == 0:
        out.add("all_ignored")
    if c["kind"] == "ties" and r["n"] > 0 and 4 * len(np.unique(r["err"][r["counted"], 0])) <= r["n"]:
        out.add("heavy_ties")
    if c["kind"] == "saturated":
        out.add("saturated")
    if r["S"] > 1 and (r["n_s"] == 0).any() and r["n"] > 0:
        out.add("empty_image")
    return out


if __name__ == "__main__":       # prints the measured constant the docstring quotes
    worst = 0.0
    for key in table():
        c = case(*key)
        k = measure(lovasz_reference(c["z"], c["y"], **c["kw"]), lovasz_reference(c["z"], c["y"], dt=F32, **c["kw"]))
        worst = max(worst, k)
    print("k_e =", worst)
