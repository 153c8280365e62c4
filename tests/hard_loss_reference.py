"""float64 reference, analytic gradient, float32 restatement, radix-select restatement, case table and derived error bounds
for the kernels of csrc/hard_loss.hip (label smoothing, focal modulation, OHEM selection), shared by
tests/test_hard_loss_host.py and tests/test_gpu_hard_loss.py.  NumPy only.  Nothing here is taken from what the kernels return.

Semantics, on logits z [N, C, H, W] fp32, labels y [N, H, W], class weights w (fp32, 1 when absent) and the scalars as the fp32
values the kernel receives (eps = label_smoothing, gamma, theta = fp32(-log(thresh)) or +inf):

  a pixel COUNTS when 0 <= y < C and y != ignore_index;  n = counted pixels;  t = its label
  nl_k = logsumexp(z) - z_k,  p = softmax(z);  key kappa = max(nl_t, 0) (a NaN stays)
  ce   = sum_k a_k nl_k,  a_k = [k = t] (1 - eps) w_t + (eps / C) w_k   (eps == 0: w_t nl_t, whatever the other logits are)
  u    = sum_{k != t} p_k,  mod = u^gamma (1 for gamma == 0),  l = mod ce
  k    = min(n, max(min_kept, (n q + 65535) >> 16)),  q = round(min_fraction 2^16)
  tau  = min(theta, k-th largest key) (theta when k == 0; a NaN key orders above +inf);  K = {counted, kappa >= tau}
  S = sum_K l,  D = sum_K w_t,  loss = S / D;  D == 0: NaN when n == 0, else 0
  g_j  = mod (A p_j - a_j) - gamma u^(gamma - 1) p_t ([j = t] - p_j) ce,  A = sum_k a_k;  d loss / d z_j = gout g_j / D on K

Error bounds follow the summation structure of hard_fwd_kernel, which is loss_fwd_kernel's: loss_reference.chain(P) unit
roundoffs on the sum of the absolute pixel terms (sums of small integers -- pixel counts, unweighted D -- are exact).

Per pixel, the accuracy of the device's expf / logf / powf cannot be derived from the project.  The key is the very evaluation
loss_reference.py measured (K_NLL: |d nl_k| <= K_NLL 2^-24 (C + (max - z_k) + nl_k)), and a probability errs by K_SM 2^-24 p_k
(C + max - z_k).  With e_nl_k and e_p_k those two in units of 2^-24 and K = 1, the pixel term and the gradient carry, in units
of 2^-24 (plus an absolute 2^-126 per operation for results that underflow):

  unit_ce  = sum_k a_k e_nl_k + (C + 3) sum_k |a_k nl_k|                  (c1 = 1 - eps, c2 = eps / C, the products, the C-term sum)
  e_u      = sum_{k != t} e_p_k + C u
  unit_mod = gamma u^(gamma - 1) e_u + mod                                 (0 for gamma == 0)
  unit_l   = mod unit_ce + |ce| unit_mod + |l|
  unit_g_j = unit_mod |A p_j - a_j| + mod (A e_p_j + (C + 4) (A p_j + a_j))
             + [gamma > 0] (unit_f p_t |d_j| |ce| + f (e_p_t |d_j| |ce| + p_t e_p_j |ce| + p_t |d_j| unit_ce) + 5 |f p_t d_j ce|) + |g_j|
             with d_j = [j = t] - p_j,  f = gamma u^(gamma - 1),  unit_f = gamma ((gamma - 1) u^(gamma - 2) e_u + u^(gamma - 1))

k_l = max |l32 - l| / (2^-24 unit_l + slack) and k_g = max |g32 - g| / (2^-24 unit_g + slack) are MEASURED on the host: the
float32 NumPy restatement below (the kernel's operations in the kernel's order; its expf, logf and powf are the correctly rounded
ones, float64 results rounded once, so that the figures are the same on every host) against float64 over the whole case table --
every class count, shape, gamma, smoothing, weight and edge case.  Measured: k_l <= 0.573, k_g <= 0.595 (tests/test_hard_loss_host.py
measures again and asserts that no case exceeds a quarter of the constants).  The device math library may differ from the host's
by a few ulp, so the bounds allow 4 x the measured values, rounded up to two digits: K_L = 2.3, K_G = 2.4.

A counted pixel is `undecided` when its float64 key lies within twice its bound of the float64 tau (the pixel whose key IS the
k-th largest, and pixels with its very logits and label, excepted: they define tau on both sides).  The selection cases that are
compared with float64 as SETS use seeds for which no pixel is undecided; the million-pixel shape is checked through the device's
own words only."""
import functools
import math

import numpy as np

from bn_reference import U24
from loss_reference import K_SM, K_NLL, TINY, chain, loss_launch

MAXC = 8
K_L, K_G = 2.3, 2.4
NAN_WORD = 0x7FC00001
HIST_WORDS = 2048 + 2048 + 1024 + 16
F32, F64 = np.float32, np.float64


def f32(v):
    return float(np.float32(v))


def theta_of(thresh):
    """-log(thresh) in float64, rounded once to fp32 (+inf: no threshold)"""
    return math.inf if thresh is None else f32(-math.log(thresh) + 0.0)


def q16_of(min_fraction):
    return int(round(float(min_fraction) * 65536.0))


def kept_count(n, min_kept, q16):
    return min(n, max(int(min_kept), (n * q16 + 65535) >> 16))


def rows(z):
    """[N, C, H, W] -> [P, C]"""
    N, C, H, W = z.shape
    return np.ascontiguousarray(np.moveaxis(z.reshape(N, C, H * W), 1, 2).reshape(N * H * W, C))


def unrows(g, shape):
    N, C, H, W = shape
    return np.ascontiguousarray(np.moveaxis(g.reshape(N, H * W, C), 2, 1).reshape(N, C, H, W))


# ---------------------------------------------------------------------------------------- words and the radix select
def words_of(kappa32, counted):
    """uint32 word per pixel: bits(kappa) + 1, NAN_WORD for a NaN key, 0 for a pixel that does not count"""
    k = np.asarray(kappa32, dtype=F32)
    w = k.view(np.uint32).astype(np.uint64) + 1
    w = np.where(np.isnan(k), NAN_WORD, w)
    return np.where(counted, w, 0).astype(np.uint32)


def word_value(word):
    """the key a word stands for, as float64 (NaN for NAN_WORD)"""
    if word == NAN_WORD:
        return math.nan
    return float(np.array([word - 1], dtype=np.uint32).view(F32)[0])


def theta_word(theta):
    return int(np.array([theta + 0.0], dtype=F32).view(np.uint32)[0]) + 1


def _scan_from_top(hist, k):
    """the bin holding the k-th word counted from the top bin down, and its rank inside that bin"""
    above = 0
    for b in range(len(hist) - 1, -1, -1):
        if above + int(hist[b]) >= k:
            return b, k - above
        above += int(hist[b])
    raise AssertionError("k exceeds the histogram's total")


def radix_select(words, k):
    """the k-th largest of the non-zero words (1 <= k <= their count) by the kernels' three levels of 11 + 11 + 10 bits"""
    w = np.asarray(words, dtype=np.uint32)
    w = w[w != 0]
    b0, k = _scan_from_top(np.bincount(w >> 21, minlength=2048), k)
    w = w[(w >> 21) == b0]
    b1, k = _scan_from_top(np.bincount((w >> 10) & 2047, minlength=2048), k)
    w = w[((w >> 10) & 2047) == b1]
    b2, k = _scan_from_top(np.bincount(w & 1023, minlength=1024), k)
    return (b0 << 21) | (b1 << 10) | b2


def select_words(words, theta, min_kept, q16, select=radix_select):
    """(word of tau, n, n_kept) of a word set, by `select` (radix_select or exact_select)"""
    w = np.asarray(words, dtype=np.uint32)
    n = int((w != 0).sum())
    k = kept_count(n, min_kept, q16)
    tw = theta_word(theta)
    if k > 0:
        tw = min(tw, int(select(w, k)))
    return tw, n, int((w >= tw).sum())


def exact_select(words, k):
    w = np.asarray(words, dtype=np.uint32)
    w = w[w != 0]
    return int(np.partition(w, len(w) - k)[len(w) - k])


# ---------------------------------------------------------------------------------------- float64 reference
def _weights(cw, C, dt):
    return np.ones(C, dtype=dt) if cw is None else np.asarray(cw, dtype=F32).astype(dt)


def _pixel(zr, y, cw, ignore_index, eps, gamma, dt):
    """the per-pixel quantities in dtype dt, classes in order (float32: the kernel's operations in the kernel's order, with
    expf / logf / powf taken as the correctly rounded ones -- evaluated in float64 and rounded once -- so that the restatement
    does not depend on the host's float32 math library)"""
    exp = lambda v: np.exp(v.astype(F64))
    log = lambda v: np.log(v.astype(F64))
    power = lambda v, g: np.power(v.astype(F64), F64(g))
    P, C = zr.shape
    z = zr.astype(dt)
    one = dt(1)
    m = z.max(1, keepdims=True)
    if dt is F32:
        m = np.full((P, 1), -np.inf, dtype=dt)
        for k in range(C):
            m = np.fmax(m, z[:, k:k + 1])
    with np.errstate(all="ignore"):
        e = exp(z - m).astype(dt)
        se = np.zeros(P, dtype=dt)
        for k in range(C):
            se = (se + e[:, k]).astype(dt)
        inv, lse = (one / se).astype(dt), log(se).astype(dt)
        nl = (lse[:, None] - (z - m)).astype(dt)
        p = (e * inv[:, None]).astype(dt)
        ign = -1 if ignore_index is None else int(ignore_index)
        counted = (y >= 0) & (y < C) & (y != ign)
        t = np.where(counted, y, 0).astype(np.int64)
        oh = (np.arange(C)[None, :] == t[:, None]) & counted[:, None]
        w = _weights(cw, C, dt)
        wt = np.where(counted, w[t], dt(0)).astype(dt)
        nlt = np.where(counted, nl[np.arange(P), t], dt(0)).astype(dt)
        pt = np.where(counted, p[np.arange(P), t], dt(0)).astype(dt)
        kappa = np.where(nlt < 0, dt(0), nlt).astype(dt)
        epsd = dt(F32(eps))
        if dt is F32:
            c1, c2 = F32(1) - epsd, epsd / F32(C)
        else:
            c1, c2 = one - epsd, epsd / dt(C)
        a = (np.where(oh, (c1 * wt)[:, None], dt(0)) + (c2 * w)[None, :]).astype(dt)
        if float(eps) == 0.0:
            a = np.where(oh, wt[:, None], dt(0)).astype(dt)
            A, ce = wt.copy(), (wt * nlt).astype(dt)
        else:
            A, ce = np.zeros(P, dtype=dt), np.zeros(P, dtype=dt)
            for k in range(C):
                A = (A + a[:, k]).astype(dt)
                ce = (ce + (a[:, k] * nl[:, k]).astype(dt)).astype(dt)
        u = np.zeros(P, dtype=dt)
        for k in range(C):
            u = (u + np.where(np.arange(P) * 0 + k != np.where(counted, t, -1), p[:, k], dt(0))).astype(dt)
        g = dt(F32(gamma))
        if float(gamma) != 0.0:
            mod = power(u, g).astype(dt)
            f = (g * power(u, g - one).astype(dt)).astype(dt)
        else:
            mod, f = np.ones(P, dtype=dt), np.zeros(P, dtype=dt)
        l = (mod * ce).astype(dt)
        d = (oh.astype(dt) - p).astype(dt)
        t1 = (mod[:, None] * ((A[:, None] * p).astype(dt) - a).astype(dt)).astype(dt)
        if float(gamma) != 0.0:
            fc = (((f * pt).astype(dt)) * ce).astype(dt)
            grad = (t1 - (fc[:, None] * d).astype(dt)).astype(dt)
        else:
            grad = t1
    return dict(z=z, m=m[:, 0], nl=nl, p=p, counted=counted, t=t, oh=oh, w=w, wt=wt, nlt=nlt, pt=pt, kappa=kappa, a=a, A=A, ce=ce,
                u=u, mod=mod, f=f, l=l, d=d, g=grad)


def _rank(kappa):
    return np.where(np.isnan(kappa), np.inf, kappa)


def hard_reference(z, y, cw=None, ignore_index=None, eps=0.0, gamma=0.0, thresh=None, min_kept=0, min_fraction=0.0, dt=F64):
    """z [N, C, H, W] fp32, y [N, H, W] int64 -> dict of float64 results and the per-pixel quantities the bounds need.  dt =
    float32 gives the restatement of the kernel's per-pixel arithmetic (its sums are then taken by restated_sums)."""
    N, C, H, W = z.shape
    zr, yr = rows(np.asarray(z, dtype=F32)), np.asarray(y).reshape(-1).astype(np.int64)
    r = _pixel(zr, yr, cw, ignore_index, eps, gamma, dt)
    selecting = not (thresh is None and min_kept == 0 and float(min_fraction) == 0.0)
    theta, q16 = theta_of(thresh), q16_of(min_fraction)
    counted = r["counted"]
    n = int(counted.sum())
    k = kept_count(n, min_kept, q16) if selecting else 0
    rank = _rank(r["kappa"].astype(F64))
    kth = None
    tau = 0.0
    if selecting:
        tau = theta
        if k > 0:
            kth = float(np.sort(rank[counted])[n - k])
            tau = min(theta, kth)
    kept = counted & (rank >= tau) if selecting else counted.copy()
    l64, wt64 = r["l"].astype(F64), r["wt"].astype(F64)
    S, D = float(l64[kept].sum()), float(wt64[kept].sum())
    loss = S / D if D > 0 else (math.nan if n == 0 else 0.0)
    r.update(N=N, C=C, H=H, W=W, P=N * H * W, shape=z.shape, eps=f32(eps), gamma=f32(gamma), selecting=selecting, theta=theta,
             q16=q16, min_kept=int(min_kept), k=k, kth=kth, tau=tau, kept=kept, n=n, n_kept=int(kept.sum()), S=S, D=D, loss=loss,
             weighted=cw is not None, rank=rank)
    return r


def hard_grad_reference(r, gout=1.0):
    """analytic d loss / d z [N, C, H, W] in the dtype of r, times the fp32 upstream gradient"""
    go = f32(gout)
    if not r["D"] > 0:
        return np.zeros(r["shape"], dtype=F64)
    g = go * r["g"].astype(F64) / r["D"] * r["kept"][:, None]
    return unrows(np.where(r["kept"][:, None], g, 0.0), r["shape"])


def restated_sums(terms, P):
    """one column of the forward partial rows, then its float64 finish: per-thread chains over the grid-stride passes, the wave
    butterfly, the sixteen wave rows, the block rows by 32 row groups of 8 (hard_fwd_kernel, hard_finalize_block)"""
    nb, n_t, _ = loss_launch(P)
    v = np.zeros(n_t * nb * 1024, dtype=F32)
    v[:P] = np.asarray(terms, dtype=F32)
    v = v.reshape(n_t, nb, 1024)
    acc = np.zeros((nb, 1024), dtype=F32)
    for i in range(n_t):
        acc = (acc + v[i]).astype(F32)
    lanes = acc.reshape(nb, 16, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, :, idx ^ o]).astype(F32)
    part = np.zeros(nb, dtype=F32)
    for w in range(16):
        part = (part + lanes[:, w, 0]).astype(F32)
    col = np.zeros(256, dtype=F64)
    col[:nb] = part
    groups = np.zeros(32, dtype=F64)
    for u in range(8):
        groups += col[32 * u:32 * u + 32]
    tot = 0.0
    for g in groups:
        tot += float(g)
    return tot


def restated_loss(z, y, **kw):
    """(loss, S, D) as float32 values through the float32 restatement: what the kernel returns if the device's expf / logf / powf
    equal NumPy's"""
    r = hard_reference(z, y, dt=F32, **kw)
    S = restated_sums(np.where(r["kept"], r["l"], F32(0)), r["P"])
    D = restated_sums(np.where(r["kept"], r["wt"], F32(0)), r["P"])
    loss = F32(S / D) if D > 0 else F32(math.nan if r["n"] == 0 else 0.0)
    return loss, F32(S), F32(D), r


# ---------------------------------------------------------------------------------------- bounds
def _units(r):
    """unit_l [P], unit_g [P, C], e_kappa [P] of the module docstring, in units of 2^-24 with every K at 1, and the slacks"""
    C = r["C"]
    z, m, nl, p = (r[k].astype(F64) for k in ("z", "m", "nl", "p"))
    a, A, ce, u, mod, f, d, pt = (r[k].astype(F64) for k in ("a", "A", "ce", "u", "mod", "f", "d", "pt"))
    gamma = r["gamma"]
    with np.errstate(all="ignore"):
        gap = m[:, None] - z
        e_nl = C + gap + nl
        e_p = p * (C + gap)
        unit_ce = (a * e_nl).sum(1) + (C + 3) * np.abs(a * nl).sum(1)
        not_t = ~r["oh"]
        e_u = (e_p * not_t).sum(1) + C * u
        us = np.maximum(u, 1e-300)
        if gamma != 0.0:
            unit_mod = gamma * us ** (gamma - 1) * e_u + mod
            unit_f = gamma * (abs(gamma - 1) * us ** (gamma - 2) * e_u + us ** (gamma - 1))
        else:
            unit_mod, unit_f = np.zeros_like(u), np.zeros_like(u)
        unit_l = mod * unit_ce + np.abs(ce) * unit_mod + np.abs(mod * ce)
        e_pt = (e_p * r["oh"]).sum(1)
        ug = unit_mod[:, None] * np.abs(A[:, None] * p - a) + mod[:, None] * (A[:, None] * e_p + (C + 4) * (A[:, None] * p + a))
        if gamma != 0.0:
            ace, ad = np.abs(ce)[:, None], np.abs(d)
            ug = ug + unit_f[:, None] * pt[:, None] * ad * ace + f[:, None] * (e_pt[:, None] * ad * ace + pt[:, None] * e_p * ace
                                                                                 + pt[:, None] * ad * unit_ce[:, None]) \
                + 5 * np.abs(f[:, None] * pt[:, None] * d * ace)
        ug = ug + np.abs(r["g"].astype(F64))
        e_kappa = C + (m - (z * r["oh"]).sum(1)) + r["kappa"].astype(F64)
    slack_l = 16 * TINY * (1 + np.abs(nl).sum(1))
    nonfinite = ~np.isfinite(unit_l)
    return (np.where(nonfinite, np.inf, unit_l), np.where(np.isfinite(ug), ug, np.inf), np.where(np.isfinite(e_kappa), e_kappa, np.inf),
            slack_l)


def key_bound(r):
    """per pixel |error| allowed for the device's key against the float64 key"""
    return K_NLL * U24 * _units(r)[2] + TINY


def pixel_bound(r):
    """per pixel |error| allowed for l"""
    unit_l, _, _, slack = _units(r)
    return K_L * U24 * unit_l + slack


def measure(r64, r32):
    """(k_l, k_g) of the module docstring over the counted pixels with finite float64 values"""
    unit_l, unit_g, _, slack = _units(r64)
    c = r64["counted"]
    with np.errstate(all="ignore"):
        dl = np.abs(r32["l"].astype(F64) - r64["l"]) / (U24 * unit_l + slack)
        dg = np.abs(r32["g"].astype(F64) - r64["g"]) / (U24 * unit_g + slack[:, None])
    ok_l = c & np.isfinite(r64["l"]) & np.isfinite(unit_l)
    ok_g = c[:, None] & np.isfinite(r64["g"]) & np.isfinite(unit_g)
    return (float(dl[ok_l].max()) if ok_l.any() else 0.0), (float(dg[ok_g].max()) if ok_g.any() else 0.0)


def state_bound(r, kept=None):
    """(|error| allowed for the loss, for S, for D) over the kept set `kept` (default: the reference's own)"""
    kept = r["kept"] if kept is None else kept
    P = r["P"]
    l, wt = r["l"].astype(F64), r["wt"].astype(F64)
    S, D = float(l[kept].sum()), float(wt[kept].sum())
    if not kept.any() or not D > 0:
        return 0.0, 0.0, 0.0
    ch = chain(P) * U24
    e_S = ch * float(np.abs(l[kept]).sum()) + float(pixel_bound(r)[kept].sum()) + U24 * abs(S)
    e_D = (ch + U24) * D if r["weighted"] else 0.0
    loss = S / D
    e_loss = 1.01 * (e_S + abs(loss) * e_D) / D + U24 * abs(loss)
    return e_loss, e_S, e_D


def grad_bound(r, gout=1.0, kept=None):
    """per element [N, C, H, W] |error| allowed for dlogits: the pixel's own evaluation, the rounding of gout / D, what D carries"""
    kept = r["kept"] if kept is None else kept
    wt = r["wt"].astype(F64)
    D = float(wt[kept].sum())
    if not D > 0:
        return np.zeros(r["shape"], dtype=F64)
    go = abs(f32(gout))
    _, unit_g, _, slack = _units(r)
    _, _, e_D = state_bound(r, kept)
    g = np.abs(r["g"].astype(F64))
    e = go / D * (K_G * U24 * unit_g + slack[:, None]) + go / D * g * (e_D / D + 4 * U24) + TINY
    return unrows(np.where(kept[:, None], 1.01 * e, 0.0), r["shape"])


def undecided(r):
    """[P] bool: counted pixels whose float64 key lies within twice its bound of the float64 tau; the pixel whose key is the k-th
    largest (when that decides tau) and the pixels with its very logits and label define tau and are excepted"""
    if not r["selecting"]:
        return np.zeros(r["P"], dtype=bool)
    c, rank, tau = r["counted"], r["rank"], r["tau"]
    eb = key_bound(r)
    with np.errstate(all="ignore"):
        close = c & (np.abs(rank - tau) <= 2 * eb) if math.isfinite(tau) else np.zeros(r["P"], dtype=bool)
    if r["kth"] is not None and r["kth"] <= r["theta"]:
        definers = np.flatnonzero(c & (rank == r["kth"]))
        if len(definers):
            d0 = definers[0]
            same = (r["z"] == r["z"][d0]).all(1) & (r["t"] == r["t"][d0]) & c
            close &= ~same
            with np.errstate(all="ignore"):
                close |= c & ~same & (np.abs(rank - tau) <= 2 * np.maximum(eb, eb[d0]))
    return close


# ---------------------------------------------------------------------------------------- case table
# (N, H, W): 1, 3, 255, 70, 4160 and 8198 pixels -- a single pixel, below one thread row, part of one block, a batch boundary,
# across the first block of 4 x 1024, three blocks with a batch boundary; then 1 049 600 pixels (C = 2 only): the 256-row cap,
# the four-in-flight main loop and its tail
SHAPES = [(1, 1, 1), (1, 1, 3), (1, 15, 17), (2, 5, 7), (1, 64, 65), (2, 1, 4099)]
BIG = (1, 1024, 1025)
CLASSES = (2, 3, 4, 5, 8)
GAMMAS = (0.0, 1.0, 2.0, 3.5)
SMOOTHS = (0.0, 0.1)
GOUTS = (1.0, 0.5)
REGIMES = ("off", "theta", "k", "both_theta", "both_k", "k_ge_n", "fraction", "empty", "all_ignored")
SET_REGIMES = ("theta", "k", "both_theta", "both_k", "fraction")       # compared with float64 as sets: undecided must be empty
THRESH = 0.5


def inputs(C, N, H, W, seed):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((N, C, H, W))).astype(F32)
    y = g.integers(0, C, (N, H, W)).astype(np.int64)
    return z, y


def _regime_kwargs(regime, z, y, cw, ign):
    """selection arguments that put the case into `regime`, from the float64 keys of its own inputs"""
    r = hard_reference(z, y, cw=cw, ignore_index=ign)
    n = r["n"]
    keys = np.sort(r["rank"][r["counted"]])[::-1]
    theta = theta_of(THRESH)
    above = int((keys >= theta).sum())
    if regime in ("off", "all_ignored"):
        return {}
    if regime == "theta":
        return dict(thresh=THRESH)
    if regime == "k":
        return dict(min_kept=n // 3 + 1)
    if regime == "both_theta":          # the k-th largest key lies above theta: theta decides
        return dict(thresh=THRESH, min_kept=max(1, above // 2))
    if regime == "both_k":              # more pixels asked for than lie above theta: the k-th key decides
        return dict(thresh=THRESH, min_kept=min(n, above + max(1, (n - above + 1) // 2)))
    if regime == "k_ge_n":
        return dict(min_kept=n + 5)
    if regime == "fraction":
        return dict(min_fraction=0.25)
    if regime == "empty":               # theta = 69 lies above every key and nothing else is asked for
        return dict(thresh=1e-30)
    raise ValueError(regime)


def regime_holds(r, regime):
    """the float64 reference r is in the selection regime its case is named after"""
    theta, kth, n, k, tau = r["theta"], r["kth"], r["n"], r["k"], r["tau"]
    if regime == "all_ignored":
        return n == 0 and math.isnan(r["loss"])
    if n == 0:
        return False
    if regime == "off":
        return not r["selecting"] and r["n_kept"] == n
    if regime == "theta":
        return r["selecting"] and k == 0 and tau == theta and math.isfinite(theta)
    if regime == "k":
        return math.isinf(theta) and 1 <= k < max(n, 2) and tau == kth
    if regime == "both_theta":
        return k >= 1 and theta < kth and tau == theta
    if regime == "both_k":
        return k >= 1 and kth < theta and tau == kth
    if regime == "k_ge_n":
        return k == n and r["n_kept"] == n and r["min_kept"] > n
    if regime == "fraction":
        return k == (n * q16_of(0.25) + 65535) >> 16 and k >= 1 and r["min_kept"] == 0 and tau == kth
    if regime == "empty":
        return k == 0 and r["n_kept"] == 0 and r["loss"] == 0.0 and r["D"] == 0.0
    raise ValueError(regime)


@functools.lru_cache(maxsize=None)
def case(ci, ri):
    """one cell of the table: class count CLASSES[ci] in regime REGIMES[ri]; shape, gamma, smoothing, weights, the ignored class,
    an out-of-range label and the upstream gradient are walked with strides of their own, so that each option meets every
    regime and class count.  -> dict(z, y, kw (arguments of hard_reference), gout, desc, regime, ref (float64))"""
    C, regime = CLASSES[ci], REGIMES[ri]
    N, H, W = SHAPES[(ci + ri) % len(SHAPES)]
    gamma = GAMMAS[(ci + 2 * ri) % 4]
    eps = SMOOTHS[(ci + ri // 2) % 2]
    weighted = (ci + ri) % 2 == 0
    imode = (ci + ri // 3) % 3              # no ignore_index / a class ignored / label 255 ignored
    gout = GOUTS[(ci + ri // 4) % 2]
    for seed in range(9000 + 1000 * ci + 100 * ri, 9000 + 1000 * ci + 100 * ri + 40):
        z, y = inputs(C, N, H, W, seed)
        P = N * H * W
        ign = None
        if P >= 3:
            if imode == 1:
                ign = (ci + ri) % C
            elif imode == 2:
                ign = 255
                y.reshape(-1)[1::5] = 255
            if P >= 70:
                y.reshape(-1)[3] = C            # labels outside [0, C): never counted, whatever ignore_index is
                y.reshape(-1)[7] = -3
        if regime == "all_ignored":
            ign = 255
            y[...] = 255
        cw = (0.5 + 0.25 * np.arange(C)).astype(F32) if weighted else None
        kw = dict(cw=cw, ignore_index=ign, eps=eps, gamma=gamma)
        kw.update(_regime_kwargs(regime, z, y, cw, ign))
        ref = hard_reference(z, y, **kw)
        if regime_holds(ref, regime) and (regime not in SET_REGIMES or not undecided(ref).any()):
            break
    else:
        raise AssertionError(f"no seed puts C={C} {regime} into its regime with an empty undecided set")
    desc = (f"C={C} {regime} N={N} H={H} W={W} gamma={gamma} eps={eps} weights={weighted} ignore={ign} gout={gout} seed={seed} "
            f"sel={ {k: v for k, v in kw.items() if k in ('thresh', 'min_kept', 'min_fraction')} }")
    return dict(z=z, y=y, kw=kw, gout=gout, desc=desc, regime=regime, ref=ref, set_check=regime in SET_REGIMES)


def table():
    return [(ci, ri) for ci in range(len(CLASSES)) for ri in range(len(REGIMES))]


BIG_REGIMES = ("off", "theta", "both_k", "fraction")


@functools.lru_cache(maxsize=None)
def big_case(regime):
    """the million-pixel shape, C = 2: sums against float64, the selection through the device's own words only"""
    N, H, W = BIG
    z, y = inputs(2, N, H, W, 9900)
    y.reshape(-1)[5::11] = 255
    kw = dict(cw=np.array([0.75, 1.5], dtype=F32), ignore_index=255, eps=0.0, gamma=0.0)
    if regime == "theta":
        kw.update(thresh=THRESH)
    elif regime == "both_k":
        kw.update(thresh=THRESH, min_kept=700000)
    elif regime == "fraction":
        kw.update(min_fraction=0.25, gamma=2.0, eps=0.1)
    return dict(z=z, y=y, kw=kw, gout=1.0, desc=f"C=2 {regime} {BIG}", regime=regime, ref=hard_reference(z, y, **kw), set_check=False)


def word_cases():
    """word sets that stress the select: (name, z, y, kw).  Keys come from logits, so that the kernels can produce them."""
    out = []
    z = np.zeros((1, 3, 15, 17), dtype=F32); z[:, 0] = 1.25
    y = np.ones((1, 15, 17), dtype=np.int64)
    out.append(("all words equal", z, y, dict(min_kept=100)))
    z = np.zeros((1, 2, 15, 17), dtype=F32)
    z[0, 0] = (F32(1.0) + F32(2.0 ** -23) * np.arange(255).reshape(15, 17)).astype(F32)      # logits a few ulp apart
    out.append(("words differing in the low 10 bits", z.copy(), np.ones((1, 15, 17), dtype=np.int64), dict(min_kept=77)))
    z, y = inputs(4, 2, 5, 7, 9801)
    out.append(("the k-th in the top bin", z, y, dict(min_kept=1)))
    z, y = inputs(3, 2, 5, 7, 9802)
    z[0, :, 0, 0] = (100.0, 0.0, 0.0); y[0, 0, 0] = 0
    out.append(("one key of exactly 0", z, y, dict(min_kept=70)))
    z, y = inputs(3, 2, 5, 7, 9803)
    z[1, :, 2, 3] = (0.0, -np.inf, 0.0); y[1, 2, 3] = 1
    out.append(("one +inf key", z, y, dict(min_kept=2)))
    z, y = inputs(4, 2, 5, 7, 9804)
    z[1, 2, 4, 6] = np.nan
    out.append(("one NaN pixel", z, y, dict(min_kept=3)))
    return out


def all_cases():
    for ci, ri in table():
        yield case(ci, ri)


if __name__ == "__main__":       # prints the measured constants the docstring quotes
    worst = [0.0, 0.0]
    for c in all_cases():
        kl, kg = measure(c["ref"], hard_reference(c["z"], c["y"], dt=F32, **c["kw"]))
        worst = [max(worst[0], kl), max(worst[1], kg)]
        print(f"{kl:8.4f} {kg:8.4f}  {c['desc']}")
    for name, z, y, kw in word_cases():
        kl, kg = measure(hard_reference(z, y, **kw), hard_reference(z, y, dt=F32, **kw))
        worst = [max(worst[0], kl), max(worst[1], kg)]
        print(f"{kl:8.4f} {kg:8.4f}  {name}")
    print("k_l, k_g =", worst)
