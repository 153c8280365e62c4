"""NumPy / plain-Python restatement of DESIGN.md 3.19 (object-level evaluation): the segment maps, the pair table in order of
first pixel, the areas, the IoU > 0.5 matching, the per-class statistics and the float64 host formulas.  The device
(csrc/panoptic.hip) must equal every array here bit for bit.  The labelling is tests/components_reference.py (3.3's pinned
definition); everything else is written from the section, with Python integers where a product could leave 64 bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as CR                                                  # noqa: E402

NC, COLS = 8, 16
SEG_ARRAYS = ("area_g", "match_g", "inter_g", "union_g", "area_p", "void_p", "match_p")
PAIR_ARRAYS = ("pair_g", "pair_p", "pair_n")


def label_sides(pred, target, things, connectivity=4, target_objects=None):
    """-> (Lp int32 [H,W], cls_p list, Lg int32 [H,W], cls_g list): both masks labelled with classes=things, or the target's
    labels and classes as given (a label outside 1..K counts as 0)"""
    Lp, rows_p = CR.label(pred, connectivity, things)
    if target_objects is None:
        Lg, rows_g = CR.label(target, connectivity, things)
        cls_g = [r["cls"] for r in rows_g]
    else:
        Lg, cls_g = np.asarray(target_objects[0], dtype=np.int32), [int(c) for c in target_objects[1]]
        Lg = np.where((Lg >= 1) & (Lg <= len(cls_g)), Lg, 0).astype(np.int32)
    return Lp, [r["cls"] for r in rows_p], Lg, cls_g


def segment_maps(pred, target, Lp, Lg, stuff, ignore_index, cap):
    """-> (Sg, Sp) int64 [H,W]: segment of every pixel; target -1 where void"""
    def seg(L, v):
        s = L.astype(np.int64)
        for c in stuff:
            s[(L == 0) & (v == c)] = cap + 1 + c
        return s
    Sp, Sg = seg(Lp, pred), seg(Lg, target)
    void = target >= NC
    if ignore_index is not None:
        void |= target == ignore_index
    Sg[void] = -1
    return Sg, Sp


def evaluate(pred, target, labelled, stuff=(), ignore_index=None, cap=1024, max_pairs=None):
    """The whole result for capacities (cap, max_pairs) as a dict: pairs int64 [P,3] = (g, p, n) in order of first pixel, the
    per-segment arrays of cap + 8 rows with -1 in the rows that are never written, totals [4], stats int64 [8,16] of THIS image,
    Sg / Sp; on overflow totals are -1 and no other entry is filled (pairs is empty, the arrays all -1, stats zero)."""
    Lp, cls_p, Lg, cls_g = labelled
    H, W = pred.shape
    Kp, Kg = len(cls_p), len(cls_g)
    rows = cap + NC
    out = {"Kp": Kp, "Kg": Kg, "cls_p": cls_p, "cls_g": cls_g, "pairs": np.zeros((0, 3), np.int64),
           "stats": np.zeros((NC, COLS), np.int64), "totals": np.full(4, -1, np.int32)}
    for n in SEG_ARRAYS:
        out[n] = np.full(rows, -1, np.int32)
    Sg, Sp = segment_maps(pred, target, Lp, Lg, stuff, ignore_index, cap)
    out["Sg"], out["Sp"] = Sg, Sp
    big = rows + 2
    comb = ((Sg + 1) * big + Sp).reshape(-1)
    keys, first, count = np.unique(comb, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    P = len(keys)
    out["P"] = P
    if Kp > cap or Kg > cap or (max_pairs is not None and P > max_pairs):
        return out
    pairs = np.stack([keys[order] // big - 1, keys[order] % big, count[order]], axis=1).astype(np.int64)
    out["pairs"] = pairs

    def in_use(r, K):
        return r < K or r >= cap
    cls_of = lambda cls, r: cls[r] if r < cap else r - cap
    for r in range(rows):
        if in_use(r, Kg):
            for n in ("area_g", "match_g", "inter_g", "union_g"):
                out[n][r] = 0
        if in_use(r, Kp):
            for n in ("area_p", "void_p", "match_p"):
                out[n][r] = 0
    for g, p, n in pairs.tolist():
        if g >= 1:
            out["area_g"][g - 1] += n
        if p >= 1:
            out["area_p"][p - 1] += n
            if g == -1:
                out["void_p"][p - 1] += n
    for g, p, n in pairs.tolist():
        if g < 1 or p < 1:
            continue
        cg, cp = cls_of(cls_g, g - 1), cls_of(cls_p, p - 1)
        if cg != cp or not 0 <= cg < NC:
            continue
        union = int(out["area_g"][g - 1]) + int(out["area_p"][p - 1]) - n - int(out["void_p"][p - 1])
        if 2 * n > union:
            assert out["match_g"][g - 1] == 0 and out["match_p"][p - 1] == 0, "a second match: the theorem of 3.19 is broken"
            out["match_g"][g - 1], out["inter_g"][g - 1], out["union_g"][g - 1], out["match_p"][p - 1] = p, n, union, g
    st, tot = out["stats"], [P, 0, 0, 0]
    for r in range(rows):
        if in_use(r, Kg) and out["area_g"][r] > 0 and 0 <= cls_of(cls_g, r) < NC:
            c = cls_of(cls_g, r)
            st[c, 14] += 1
            tot[1] += 1
            if out["match_g"][r] == 0:
                st[c, 2] += 1
            else:
                n, union = int(out["inter_g"][r]), int(out["union_g"][r])
                st[c, 0] += 1
                tot[3] += 1
                st[c, 3] += (n << 32) // union
                for k in range(10):
                    if 20 * n >= (10 + k) * union:
                        st[c, 4 + k] += 1
        if in_use(r, Kp) and out["area_p"][r] > 0 and 0 <= cls_of(cls_p, r) < NC:
            c = cls_of(cls_p, r)
            st[c, 15] += 1
            tot[2] += 1
            if out["match_p"][r] == 0 and not 2 * int(out["void_p"][r]) > int(out["area_p"][r]):
                st[c, 1] += 1
    out["totals"] = np.asarray(tot, np.int32)
    return out


def expected_pairs(res, max_pairs):
    """the three pair buffers a call must leave from 0xFF-filled ones"""
    buf = {n: np.full(max_pairs, -1, np.int32) for n in PAIR_ARRAYS}
    for j, n in enumerate(PAIR_ARRAYS):
        buf[n][:len(res["pairs"])] = res["pairs"][:, j]
    return buf


def contingency(res):
    """dense int64 table [target segments incl. void and nothing, predicted segments incl. nothing] with its row / column ids"""
    pairs = res["pairs"]
    gs, ps = sorted(set(pairs[:, 0].tolist())), sorted(set(pairs[:, 1].tolist()))
    T = np.zeros((len(gs), len(ps)), np.int64)
    for g, p, n in pairs.tolist():
        T[gs.index(g), ps.index(p)] = n
    return T, gs, ps


def quality(stats, classes, num_classes):
    """the float64 host formulas of 3.19 on int64 stats [8,16] over `classes` -> plain data: lists of num_classes entries (None
    for a class outside `classes` or with TP + FP + FN == 0) and the means over the classes that have objects"""
    two32 = float(1 << 32)
    out = {k: [None] * num_classes for k in ("pq", "sq", "rq", "f1", "tp", "fp", "fn")}
    seen = []
    for c in classes:
        tp, fp, fn, iou = (int(stats[c][k]) for k in (0, 1, 2, 3))
        out["tp"][c], out["fp"][c], out["fn"][c] = tp, fp, fn
        if tp + fp + fn == 0:
            continue
        seen.append(c)
        out["pq"][c] = (iou / two32) / (tp + fp / 2 + fn / 2)
        out["sq"][c] = (iou / two32) / tp if tp else 0.0
        out["rq"][c] = tp / (tp + fp / 2 + fn / 2)
        out["f1"][c] = []
        for k in range(10):                      # a match below the threshold is a miss on both sides
            t = int(stats[c][4 + k])
            out["f1"][c].append(t / (t + (fp + tp - t) / 2 + (fn + tp - t) / 2))
    mean = lambda v: (sum(v) / len(v)) if v else None
    for k in ("pq", "sq", "rq"):
        out["mean_" + k] = mean([out[k][c] for c in seen])
    out["mean_f1"] = [mean([out["f1"][c][k] for c in seen]) for k in range(10)]
    out["classes"] = list(classes)
    return out
