"""CPU restatements of csrc/prompt.hip and the case tables of tests/test_gpu_prompt_matrix.py (NumPy only; nothing here touches
the library).  tests/test_recon_prompt_cases_host.py checks scores / make against the fixture captured from the reference's own
functions (tests/golden/prompt_points.npz) and proves from the restated launch arithmetic that the tables reach what they claim.

  class_of   include/segk.h: a label outside 0..255 is class 0, a table result of 8 or more is class 0, no table is the identity
             on 0..7.
  scores     per candidate and class 0..7 the math.fsum (the exactly rounded sum) of w[d2] over the window |dy|, |dx| <= R
             clipped to the image, terms with d2 >= nw dropped; a centre outside the image gives zeros.  With N terms the
             device's float64 sum, in whatever order, is within (N - 1) 2^-53 sum of the exact sum of its non-negative terms:
             the gate is |dev - ref| <= N 2^-53 ref per entry.
  choose     select_dominant_class: the largest sum among classes 1..7, the lowest class on a tie, 0 below 1e-9.
  stable     the choice cannot change under twice that bound on every sum.
  make       the reference's retry loop as a loop; heat = float32(q[d2]) / float32(255), 0 at d2 >= nq.
  heatmap    q[min over the points inside the image of d2] / 255."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle.fill import u01

NC = 8
U53 = 2.0 ** -53
TRIMAP = np.zeros(256, np.uint8)                      # image_segmentation_amd.TRIMAP_TO_PROMPT (the host test compares them)
TRIMAP[[0, 1, 2, 3, 255]] = [1, 2, 3, 1, 1]
WIDE = ((np.arange(256) * 7 + 3) % 12).astype(np.uint8)          # a table with results 8..11: class 0 by the header
LUTS = {"none": None, "trimap": TRIMAP, "wide": WIDE}


def class_of(label, lut):
    v = np.asarray(label, dtype=np.int64)
    inside = (v >= 0) & (v <= 255)
    idx = np.where(inside, v, 0)
    c = idx if lut is None else np.asarray(lut)[idx].astype(np.int64)
    return np.where(inside & (c < NC), c, 0)


def tables(sigma, n):
    """w[d2] = exp(-d2 / (2 sigma^2)) in float64 and q[d2] = (uint8)(255 w[d2]), n entries each (heat_tables' expressions)"""
    w = np.exp(-np.arange(n) / (2 * float(sigma) ** 2))
    return w, (w * 255).astype(np.uint8)


def choose(s):
    best = 1 + int(np.argmax(s[1:]))                  # the first of equals: the lowest class on a tie
    return 0 if s[best] < 1e-9 else best


def scores(labels, lut, centers, w, nw, R):
    """labels [H,W] int64, centers [K,2] -> (scores [K,8] float64, N [K] terms, cls [K] int32)"""
    H, W = labels.shape
    cm = class_of(labels, lut)
    K = len(centers)
    out, N, cls = np.zeros((K, NC)), np.zeros(K, np.int64), np.zeros(K, np.int32)
    for k, (cy, cx) in enumerate(np.asarray(centers).tolist()):
        if not (0 <= cy < H and 0 <= cx < W):
            continue
        ylo, yhi, xlo, xhi = max(cy - R, 0), min(cy + R, H - 1), max(cx - R, 0), min(cx + R, W - 1)
        yy, xx = np.mgrid[ylo:yhi + 1, xlo:xhi + 1]
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        keep = d2 < nw
        N[k] = int(keep.sum())
        t = w[np.minimum(d2, nw - 1)]
        c = cm[ylo:yhi + 1, xlo:xhi + 1]
        for q in range(NC):
            out[k, q] = math.fsum(t[keep & (c == q)].tolist())
        cls[k] = choose(out[k])
    return out, N, cls


def score_bound(ref, N):
    return N[:, None] * U53 * ref


def stable(ref, N):
    """the choice holds when every sum moves by up to twice its bound"""
    srt = np.sort(ref[:, 1:], axis=1)
    top, second = srt[:, -1], srt[:, -2]
    e = 2 * N * U53 * top
    return (top < 1e-9 - e) | ((top > 1e-9 + e) & (top - second > 2 * e))


def heat_of(d2, q, nq):
    return np.where(d2 < nq, q[np.minimum(d2, nq - 1)], 0).astype(np.float32) / np.float32(255.0)


def make(labels, lut, centers, cls, q, nq, per_image):
    """one image -> (heat [PI,H,W] f32, target [PI,H,W] i64, classes [PI] i32, centres [PI,2] i32, valid)"""
    H, W = labels.shape
    cm = class_of(labels, lut)
    taken, found = [], set()
    k = 0
    while len(taken) < per_image and k < len(cls):     # the retry loop: the next candidate until per_image are taken
        c, (cy, cx) = int(cls[k]), (int(v) for v in centers[k])
        if 1 <= c < NC and c not in found and 0 <= cy < H and 0 <= cx < W:
            taken.append(k)
            found.add(c)
        k += 1
    heat = np.zeros((per_image, H, W), np.float32)
    target = np.zeros((per_image, H, W), np.int64)
    classes, cen = np.zeros(per_image, np.int32), np.zeros((per_image, 2), np.int32)
    if len(taken) < per_image:
        return heat, target, classes, cen, 0
    yy, xx = np.indices((H, W))
    for j, k in enumerate(taken):
        c, cy, cx = int(cls[k]), int(centers[k][0]), int(centers[k][1])
        heat[j] = heat_of((yy - cy) ** 2 + (xx - cx) ** 2, q, nq)
        target[j] = np.where(cm == c, c, 0)
        classes[j], cen[j] = c, (cy, cx)
    return heat, target, classes, cen, 1


def heatmap(points, q, nq, H, W):
    pts = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    pts = pts[(pts[:, 0] >= 0) & (pts[:, 0] < H) & (pts[:, 1] >= 0) & (pts[:, 1] < W)]
    if not len(pts):
        return np.zeros((H, W), np.float32)
    yy, xx = np.indices((H, W))
    d2 = ((yy[None] - pts[:, 0, None, None]) ** 2 + (xx[None] - pts[:, 1, None, None]) ** 2).min(0)
    return heat_of(d2, q, nq)


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------
def score_window(cy, cx, R, H, W):
    """-> (rows, columns, 64-lane passes, live lanes of the last pass) of an inside centre's clipped window"""
    rows = min(cy + R, H - 1) - max(cy - R, 0) + 1
    cols = min(cx + R, W - 1) - max(cx - R, 0) + 1
    passes = (cols + 63) // 64
    return rows, cols, passes, cols - 64 * (passes - 1)


def vec_path(H, W):
    """-> (16-byte path, some 4-pixel vector crosses a row)"""
    vec = (H * W) % 4 == 0
    return vec, vec and W % 4 != 0 and H > 1


def k0_passes(K):
    return (K + 1023) // 1024


# ---- inputs ----------------------------------------------------------------------------------------------------------------
BAD_LABELS = [-1, 256, 2 ** 40 + 3, -2 ** 63]


def draw(n, seed, hi):
    """n integers of 0..hi-1 from the portable fill"""
    return np.minimum((u01(n, seed).astype(np.float64) * hi).astype(np.int64), hi - 1)


def blocky(H, W, seed, values, bad=True):
    """blocks of 5 x 7 pixels with values drawn from `values`, then pixels of every BAD_LABELS value sprinkled at strides
    coprime to the block sizes"""
    values = np.asarray(values, dtype=np.int64)
    gh, gw = (H + 4) // 5, (W + 6) // 7
    g = values[draw(gh * gw, seed, len(values))].reshape(gh, gw)
    lab = np.repeat(np.repeat(g, 5, 0), 7, 1)[:H, :W].copy()
    if bad:
        flat = lab.reshape(-1)
        for i, v in enumerate(BAD_LABELS):
            flat[3 + 5 * i::37 + 4 * i] = v
    return lab


LABEL_VALUES = {"none": list(range(NC)), "trimap": [0, 1, 2, 3, 255, 7], "wide": list(range(256))}

ScoreCase = namedtuple("ScoreCase", "name B H W R nw_disc K lut centres seed")


def _ring(H, W):
    """the four corners and the four edge midpoints"""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]


def _score_cases():
    big = [(y, x) for y in (3, 35, 66) for k in (1, 2, 3) for x in (64 * k - 1, 64 * k + 1) if x < 200]
    rnd = [(int(y), int(x)) for y, x in zip(draw(65, 91, 70), draw(65, 92, 200))]
    full = (_ring(70, 200) + big + rnd)[:65]
    out = [
        ScoreCase("1x1-R0", 1, 1, 1, 0, False, 1, "none", [(0, 0)], 1),
        ScoreCase("1x1-R1", 1, 1, 1, 1, False, 1, "wide", [(0, 0)], 14),       # seed 2 drew class 0
        ScoreCase("row-1x200-R64", 1, 1, 200, 64, False, 5, "none", [(0, 0), (0, 199), (0, 100), (0, 63), (0, 65)], 3),
        ScoreCase("col-200x1-R63", 3, 200, 1, 63, False, 4, "trimap", [(0, 0), (199, 0), (100, 0), (63, 0)], 4),
        ScoreCase("9x40-R32", 3, 9, 40, 32, False, 5, "trimap", [(0, 0), (8, 39), (4, 20), (4, 0), (0, 39)], 5),
        ScoreCase("70x200-R32", 1, 70, 200, 32, False, 65, "wide", full, 6),
        ScoreCase("70x200-R64", 3, 70, 200, 64, False, 65, "none", full, 7),
        ScoreCase("70x200-R63", 1, 70, 200, 63, False, 4, "none", [(35, 63), (35, 65), (0, 127), (69, 129)], 8),
        ScoreCase("70x200-R31", 1, 70, 200, 31, False, 3, "trimap", [(35, 100), (0, 0), (69, 199)], 9),
        ScoreCase("70x200-R1", 3, 70, 200, 1, False, 5, "none", [(0, 0), (69, 199), (35, 100), (0, 100), (35, 199)], 10),
        ScoreCase("70x200-R0", 1, 70, 200, 0, False, 5, "wide", [(0, 0), (69, 199), (35, 100), (12, 64), (35, 63)], 11),
        ScoreCase("70x200-R32-disc", 1, 70, 200, 32, True, 5, "none", [(35, 100), (0, 0), (69, 199), (35, 65), (3, 127)], 12),
        ScoreCase("70x200-outside", 1, 70, 200, 32, False, 4, "none", [(-1, 5), (70, 0), (0, 200), (2 ** 31 - 1, -2 ** 31)], 13),
    ]
    # window heights 1..8 (9 is the 9x40 case): every remainder of the 4-row unroll
    for H in range(1, 9):
        out.append(ScoreCase(f"{H}x40-R32", 1, H, 40, 32, False, 3, "none", [(0, 0), (H - 1, 39), (H // 2, 20)], 20 + H))
    return out


SCORE_CASES = _score_cases()
ALL_ZERO_SCORE_CASES = {"70x200-outside"}            # built to hold class-0 choices only


def score_tables(c):
    """sigma = max(R, 1) / 2: the outer ring (d2 = R^2) still carries exp(-2).  nw = 2 R^2 + 1, or R^2 + 1 (a disc)"""
    nw = (c.R * c.R if c.nw_disc else 2 * c.R * c.R) + 1
    w, _ = tables(max(c.R, 1) / 2.0, nw)
    return w, nw


def score_inputs(c):
    """-> (labels [B,H,W] int64, centres [B,K,2] int32): image b sees the candidates rotated by b"""
    lab = np.stack([blocky(c.H, c.W, 100 * c.seed + b, LABEL_VALUES[c.lut], bad=c.H * c.W > 1) for b in range(c.B)])
    cen = np.array(c.centres, dtype=np.int64).reshape(c.K, 2)
    return lab, np.stack([np.roll(cen, b, 0) for b in range(c.B)]).astype(np.int32)


MakeCase = namedtuple("MakeCase", "H W K per_image nq lut seed")
MAKE_SHAPES = [(1, 1), (3, 5), (33, 47),                              # scalar path
               (8, 8), (16, 64),                                      # 16-byte path, no vector crosses a row
               (2, 2), (4, 1), (1, 4), (4, 3), (4, 7), (12, 5), (6, 10),      # 16-byte path, vectors cross rows
               (4, 255), (32, 32), (4, 257)]                          # 1020, 1024, 1028 pixels: the block edge
MAKE_KS = [1, 5, 1023, 1024, 1025, 2049]
MAKE_PIS = [1, 2, 3, 7]
Q_SIGMA, Q_LEN = 3.0, 1459                                           # the table of sigma 3 at 256 x 256: 100 non-zero entries
NQS = [1, 100, Q_LEN]


def _make_cases():
    out = []
    for i, (H, W) in enumerate(MAKE_SHAPES + [(33, 47), (6, 10), (16, 64)]):
        K = MAKE_KS[(i + 2) % 6]
        pi = MAKE_PIS[(i + i // 4) % 4] if K > 1 else 1
        out.append(MakeCase(H, W, K, min(pi, K), NQS[i % 3], ("none", "trimap", "wide")[(i + i // 3) % 3], 300 + i))
    return out


MAKE_CASES = _make_cases()
JUNK = [0, 8, -3, 2 ** 31 - 1]                       # classes that are ignored


def first_positions(K):
    return sorted({p for p in (0, 255, 256, 1023, 1024, K - 1, K // 3, K // 2, (2 * K) // 3, K - 2) if 0 <= p < K})


def make_inputs(c):
    """-> (labels [3,H,W], centres [3,K,2] int32, cls [3,K] int32, planted): image 0 holds exactly per_image distinct classes,
    image 1 one fewer (it is skipped), image 2 as many of the seven as K allows.  A class's first valid candidate sits at
    0, 255, 256, 1023, 1024, K - 1 (then K/3, K/2, 2K/3, K - 2), later positions first for image 0, so that the second and
    third k0 pass decide; each planted class is preceded, where there is room, by a candidate of the same class whose centre lies
    outside the image, and followed by a duplicate.  `planted` [3] lists (position, class) per image."""
    H, W, K = c.H, c.W, c.K
    values = LABEL_VALUES[c.lut]
    lab = np.stack([blocky(H, W, c.seed * 10 + b, values, bad=H * W >= 8) for b in range(3)])
    cen = np.stack([np.stack([draw(K, c.seed * 10 + 3 + b, H), draw(K, c.seed * 10 + 6 + b, W)], 1) for b in range(3)])
    cls = np.array([[JUNK[(k + b) % 4] for k in range(K)] for b in range(3)], dtype=np.int64)
    pos = first_positions(K)
    planted = []
    for b, want in enumerate((c.per_image, c.per_image - 1, 7)):
        ps = (pos[::-1] if b == 0 else pos)[:min(want, len(pos))]
        row = []
        for j, p in enumerate(sorted(ps)):
            cl = 1 + (j * 3 + b + c.seed) % 7
            while cl in [r[1] for r in row]:
                cl = 1 + cl % 7
            row.append((p, cl))
            cls[b, p] = cl
        free = [k for k in range(K) if k not in ps]
        for (p, cl) in row:
            before = [k for k in free if k < p]
            after = [k for k in free if k > p]
            if before:                               # the same class earlier, its centre outside the image: not taken
                k = before[-1]
                free.remove(k)
                cls[b, k] = cl
                cen[b, k] = [(-1, 0), (0, W), (H, 0), (0, -5)][p % 4]
            if after:                                # and later once more: taken already
                k = after[0]
                free.remove(k)
                cls[b, k] = cl
        planted.append(row)
    return lab, cen.astype(np.int32), cls.astype(np.int32), planted


@lru_cache(maxsize=None)
def q_table():
    return tables(Q_SIGMA, Q_LEN)[1]


HeatCase = namedtuple("HeatCase", "H W P nq kind seed")
HEAT_PS = [1, 2, 255, 256, 257, 1024]


def _heat_cases():
    out = []
    for i, (H, W) in enumerate(MAKE_SHAPES + [(33, 47), (6, 10), (16, 64)]):
        kind = "all outside" if i == 9 else ("some outside" if i % 2 else "inside")
        out.append(HeatCase(H, W, HEAT_PS[(i + 3) % 6], NQS[(i + 1) % 3], kind, 700 + i))
    return out


HEAT_CASES = _heat_cases()


def heat_points(c):
    """[P,2] int32: drawn inside the image (P > H W repeats pixels; every third point repeats its predecessor), then every
    fourth moved outside ("some outside") or all of them"""
    pts = np.stack([draw(c.P, c.seed, c.H), draw(c.P, c.seed + 50, c.W)], 1)
    pts[2::3] = pts[1:-1:3][:len(pts[2::3])]
    out = np.array([(-1, 0), (0, c.W), (c.H, 0), (0, -7), (2 ** 31 - 1, 0), (0, -2 ** 31)], dtype=np.int64)
    if c.kind == "some outside":
        idx = np.arange(1, c.P, 4)
        pts[idx] = out[idx % len(out)]
    elif c.kind == "all outside":
        pts = out[np.arange(c.P) % len(out)]
    return pts.astype(np.int32)
