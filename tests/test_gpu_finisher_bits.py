"""GPU (-m gpu): the five prediction finishers -- segk_predict_mask, segk_predict_merge, segk_predict_tiles, segk_mask_finish,
segk_calib_temps -- driven directly through _lib.call on inputs from oracle.fill (no RNG, no model), every output buffer
(mask, colour, counts, M, conf, scores, hist, nll_fx, nonfinite, valid) compared by SHA-1 with tests/golden/finisher_bits.json.
To keep the fixture small the digests are folded: per entry, class count and mode, and per buffer name, one SHA-1 over
"case:digest;" of that buffer in every case of the group, in case order.

The fixture is a record of the library BEFORE the finishers were folded onto one sampler, one argmax and one mask sink
(csrc/predict_common.hpp): the code may be rearranged, the bytes may not change.  The shapes are the
smallest at which this code can go wrong: outputs below four pixels (the byte tail only), threads that span several rows,
the dword path only, both paths with a row end inside a thread, every class-count instance (C = 5 runs the 8-class one with
padded classes), both resize modes, every present / absent combination of the outputs, labels outside 0..C-1 next to valid
ones, logits with an exact tie, NaN in the first and the last class and +inf, and two sizes that send the grid-stride loop
round a second time (1024 x 800 with counts: the cap is 3 blocks x 256 CUs x 1024 pixels; 4100 x 4100 mask-only: 16384 blocks).

Set SEGK_FINISHER_BITS_OUT=<file> to write the record there instead of comparing (never from the code under test)."""
import hashlib
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle.fill import fill, labels as fill_labels

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finisher_bits.json")
OUT = os.environ.get("SEGK_FINISHER_BITS_OUT")
SIZES = [(1, 1), (1, 3), (2, 2), (3, 1), (5, 3), (4, 4), (7, 9), (37, 53)]
CLASSES = [1, 2, 3, 4, 5, 8]
PROB, LOGIT = 0, 1
_RECORD = {}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    if OUT and _RECORD:
        with open(OUT, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sorted(_RECORD.items()))
                    + "\n}\n")


@pytest.fixture(scope="module")
def want():
    if OUT:
        return None
    with open(GOLDEN) as f:
        return json.load(f)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def dev(t):
    return t.cuda().contiguous()


def logits(shape, seed, lo=-4.0, hi=4.0):
    """[..., C, h, w] in (lo, hi) with, where the plane has room: an exact tie of all classes on row 1 and at (0, 0), NaN in class
    0 at (2, 1), NaN in the last class at (2, 2), +inf in the middle class at (0, 2)"""
    z = fill(shape, seed, lo, hi)
    C, h, w = shape[-3:]
    z[..., :, 0, 0] = 0.5
    if h > 1:
        z[..., :, 1, :] = z[..., :1, 1, :]
    if w > 2:
        z[..., C // 2, 0, 2] = float("inf")
    if h > 2 and w > 2:
        z[..., 0, 2, 1] = float("nan")
        z[..., C - 1, 2, 2] = float("nan")
    return z


def labels_for(total, C, seed):
    """valid classes with -1, C and 255 among them"""
    lab = fill_labels((total,), seed, C)
    i = torch.arange(total)
    lab[i % 7 == 3] = -1
    lab[i % 11 == 5] = C
    lab[i % 13 == 6] = 255
    return lab


def palette_for(C):
    k = np.arange(C)
    return torch.from_numpy(np.stack([(37 * k + 11) % 256, (91 * k + 5) % 256, (53 * k + 200) % 256], 1).astype(np.uint8))


class Outputs:
    """the output buffers a case asked for (absent: None -> NULL), zero-filled; digests of all of them after the call"""

    def __init__(self, **shapes):
        self.t = {k: (None if s is None else torch.zeros(s[0], dtype=s[1], device="cuda")) for k, s in shapes.items()}

    def p(self, name):
        t = self.t[name]
        return None if t is None else t.data_ptr()

    def digests(self):
        torch.cuda.synchronize()
        return {k: hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest() for k, t in self.t.items() if t is not None}


def sink_outputs(total, C, lab, color, counts, conf=None, scores=None, mask=True):
    return Outputs(mask=(total, torch.uint8) if mask else None, color=(total * 3, torch.uint8) if color else None,
                   counts=(8, torch.int64) if counts else None, M=(64, torch.int64) if lab else None,
                   conf=(total, torch.uint8) if conf else None, scores=(C * total, torch.float32) if scores else None)


_FOLD = {}       # group -> buffer name -> running SHA-1


def check(key, got):
    """fold the case's buffer digests into its group: entry / C / mode (a second-trip case is a group of its own)"""
    parts = key.split("/")
    group = key if parts[0].startswith("second_trip") else "/".join(q for i, q in enumerate(parts) if i == 0 or re.fullmatch(r"C\d+|mode\d", q))
    for name, digest in got.items():
        _FOLD.setdefault(group, {}).setdefault(name, hashlib.sha1()).update(f"{key}:{digest};".encode())


def settle(want, entry):
    """compare (or record) the groups of one entry"""
    got = {g: {n: h.hexdigest() for n, h in bufs.items()} for g, bufs in _FOLD.items() if g.split("/")[0] == entry}
    assert got
    if OUT:
        _RECORD.update(got)
        return
    assert sorted(got) == sorted(g for g in want if g.split("/")[0] == entry), "the groups of the fixture are not those of the test"
    bad = [f"{g}: " + ", ".join(n for n in got[g] if got[g][n] != want[g].get(n)) + " differ" for g in sorted(got) if got[g] != want[g]]
    assert not bad, "\n".join(bad)


def sw(flags):
    return "".join("1" if f else "0" for f in flags)


# ---- cases -------------------------------------------------------------------------------------------------------------------
def switch_cases(n_switches, sizes=((7, 9),)):
    """every class count, size and mode with all outputs on; every combination of the switches at `sizes`, every class count
    and mode"""
    on = (True,) * n_switches
    cases = [(s, C, mode, on) for s in SIZES for C in CLASSES for mode in (0, 1)]
    cases += [(s, C, mode, f) for s in sizes for C in CLASSES for mode in (0, 1)
              for f in itertools.product((False, True), repeat=n_switches) if f != on]
    return cases


T_SLOT, PT, PL, NH, NW = 12, 1, 2, 7, 9


def slot_for(C, seed):
    z = fill((C, T_SLOT, T_SLOT), seed, -4.0, 4.0)
    z[:, PT:PT + NH, PL:PL + NW] = logits((C, NH, NW), seed + 1)
    return z


def test_predict_mask(lib, want):
    for (oh, ow), C, mode, (lab, color, counts) in switch_cases(3):
        total = oh * ow
        slot, labs, pal = dev(slot_for(C, 10 + C)), dev(labels_for(total, C, 20 + C)), dev(palette_for(C))
        o = sink_outputs(total, C, lab, color, counts)
        lib.call("segk_predict_mask", slot.data_ptr(), o.p("mask"), o.p("color"), pal.data_ptr() if color else None, o.p("counts"),
                 labs.data_ptr() if lab else None, o.p("M"), C, T_SLOT, PT, PL, NH, NW, oh, ow, mode, None)
        check(f"predict_mask/{oh}x{ow}/C{C}/mode{mode}/{sw((lab, color, counts))}", o.digests())
    settle(want, "predict_mask")


# views with different (T, nh, nw, pad): (T, pad_top, pad_left, nh, nw)
VIEW_GEOMETRY = [(T_SLOT, PT, PL, NH, NW), (16, 0, 3, 16, 11), (10, 2, 0, 5, 10)]
WEIGHTS = {1: (1.0,), 3: (0.5, 0.3, 0.2)}


def view_table(C, V, flips, kinds, seed):
    from image_segmentation_amd.tta import VIEW_DESC
    table, slots = np.zeros(V, dtype=VIEW_DESC), []
    for v in range(V):
        T, pt, pl, nh, nw = VIEW_GEOMETRY[v]
        lo, hi = ((-4.0, 4.0), (0.0, 1.0))[kinds[v]]       # kind 1: values the merge adds as they are (no host softmax: no libm)
        z = fill((C, T, T), seed + 7 * v, lo, hi)
        z[:, pt:pt + nh, pl:pl + nw] = logits((C, nh, nw), seed + 7 * v + 1, lo, hi)
        slots.append(dev(z))
        table[v] = (slots[-1].data_ptr(), T, pt, pl, nh, nw, flips[v], kinds[v], np.float32(WEIGHTS[V][v]), (0, 0))
    return dev(torch.from_numpy(table.view(np.uint8))), slots


def switch_combos(C, n=5):
    return [f for f in itertools.product((False, True), repeat=n) if not all(f)] if C == 5 else [(False,) * n]


def merge_cases():
    all_on = (True,) * 5
    # every size, class count and mode: three views, flips 1 2 3, kinds logits / probabilities / logits, prob merge
    cases = [(s, C, mode, 3, (1, 2, 3), (0, 1, 0), PROB, all_on) for s in SIZES for C in CLASSES for mode in (0, 1)]
    # V = 1 with every flip and V = 3, both merges with the kinds each allows, every class count
    for C in CLASSES:
        for mode in (0, 1):
            for flip in range(4):
                cases.append(((7, 9), C, mode, 1, (flip,), (0,), PROB if flip & 1 else LOGIT, all_on))
            cases.append(((7, 9), C, mode, 3, (0, 3, 1), (0, 0, 0), LOGIT, all_on))
            cases.append(((7, 9), C, mode, 3, (2, 0, 3), (1, 1, 1), PROB, all_on))
    # every combination of the switches (labels + M, colour + palette, counts, conf, scores) at C = 5, all off at the other
    # class counts (the instances without labels), both merges
    for C in CLASSES:
        for mode in (0, 1):
            for merge in (PROB, LOGIT):
                for f in switch_combos(C):
                    cases.append(((7, 9), C, mode, 3, (1, 2, 3), (0, 0, 0), merge, f))
    return cases


def test_predict_merge(lib, want):
    for (oh, ow), C, mode, V, flips, kinds, merge, (lab, color, counts, conf, scores) in merge_cases():
        total = oh * ow
        table, slots = view_table(C, V, flips, kinds, 30 + C)
        labs, pal = dev(labels_for(total, C, 40 + C)), dev(palette_for(C))
        o = sink_outputs(total, C, lab, color, counts, conf, scores)
        lib.call("segk_predict_merge", table.data_ptr(), V, C, merge, mode, oh, ow, o.p("mask"), o.p("color"),
                 pal.data_ptr() if color else None, o.p("counts"), labs.data_ptr() if lab else None, o.p("M"), o.p("conf"), o.p("scores"),
                 None)
        check(f"predict_merge/{oh}x{ow}/C{C}/mode{mode}/V{V}/flips{''.join(map(str, flips))}/kinds{sw(kinds)}/"
                              f"merge{merge}/{sw((lab, color, counts, conf, scores))}", o.digests())
    settle(want, "predict_merge")


def tile_count(L, T, overlap):
    s = T - overlap
    return 1 if L <= T else -(-(L - T) // s) + 1


def tiles_input(C, H, W, T, overlap, kind, seed):
    n = tile_count(H, T, overlap) * tile_count(W, T, overlap)
    return dev(logits((n, C, T, T), seed, *((-4.0, 4.0), (0.0, 1.0))[kind]))


def tiles_cases():
    all_on = (True,) * 5
    # every size and class count at T = 4: an axis with one tile (L <= 4), an axis whose last tile is pulled back (5, 7, 9, 37, 53
    # are no multiples of the stride), overlap 0 and T / 2, both windows
    cases = [(s, C, 4, ov, win, 0, PROB, all_on) for s in SIZES for C in CLASSES for ov in (0, 2) for win in (0, 1)]
    # both merges with the kinds each allows, T = 8 (H = 7: one tile, W = 9: two, the second pulled back by 7)
    for C in CLASSES:
        for win in (0, 1):
            for kind, merge in ((0, PROB), (1, PROB), (0, LOGIT)):
                cases.append(((7, 9), C, 8, 4, win, kind, merge, all_on))
    for C in CLASSES:
        for kind, merge in ((0, PROB), (1, PROB), (0, LOGIT)):
            for f in switch_combos(C):
                cases.append(((7, 9), C, 4, 2, 1, kind, merge, f))
    return cases


def test_predict_tiles(lib, want):
    for (H, W), C, T, ov, win, kind, merge, (lab, color, counts, conf, scores) in tiles_cases():
        total = H * W
        Y, labs, pal = tiles_input(C, H, W, T, ov, kind, 50 + C), dev(labels_for(total, C, 60 + C)), dev(palette_for(C))
        o = sink_outputs(total, C, lab, color, counts, conf, scores)
        lib.call("segk_predict_tiles", Y.data_ptr(), C, kind, merge, win, H, W, T, ov, o.p("mask"), o.p("color"),
                 pal.data_ptr() if color else None, o.p("counts"), labs.data_ptr() if lab else None, o.p("M"), o.p("conf"), o.p("scores"),
                 None)
        check(f"predict_tiles/{H}x{W}/C{C}/T{T}/ov{ov}/win{win}/kind{kind}/merge{merge}/"
                              f"{sw((lab, color, counts, conf, scores))}", o.digests())
    settle(want, "predict_tiles")


def mask_for(total, C, seed):
    """classes 0 .. C + 1 (so some are >= C), with 8, 9 and 255 among them"""
    m = fill_labels((total,), seed, C + 2).to(torch.uint8)
    i = torch.arange(total)
    m[i % 5 == 4] = 8
    m[i % 9 == 7] = 9
    m[i % 17 == 2] = 255
    return m


def test_mask_finish(lib, want):
    all_on = (True,) * 3
    cases = [(s, C, all_on) for s in SIZES for C in CLASSES]
    cases += [(s, C, f) for s in ((2, 2), (7, 9)) for C in CLASSES for f in itertools.product((False, True), repeat=3)
              if f != all_on and any(f)]
    for (H, W), C, (lab, color, counts) in cases:
        total = H * W
        m, labs, pal = dev(mask_for(total, C, 70 + C)), dev(labels_for(total, C, 80 + C)), dev(palette_for(C))
        o = sink_outputs(total, C, lab, color, counts, mask=False)
        lib.call("segk_mask_finish", m.data_ptr(), o.p("color"), pal.data_ptr() if color else None, o.p("counts"),
                 labs.data_ptr() if lab else None, o.p("M"), C, H, W, None)
        got = o.digests()
        got["mask"] = hashlib.sha1(m.cpu().numpy().tobytes()).hexdigest()      # the input: read, never written
        check(f"mask_finish/{H}x{W}/C{C}/{sw((lab, color, counts))}", got)
    settle(want, "mask_finish")


INV_T = {1: (1.0,), 3: (1.0, 0.5, 2.0)}


def calib_call(lib, slot, C, oh, ow, mode, labs, ignore, K):
    inv_t = dev(torch.tensor(INV_T[K], dtype=torch.float32))
    o = Outputs(hist=(K * 512, torch.int64), nll_fx=(K, torch.int64), nonfinite=(K, torch.int64), valid=(1, torch.int64))
    lib.call("segk_calib_temps", slot.data_ptr(), C, T_SLOT, PT, PL, NH, NW, oh, ow, mode, labs.data_ptr(), ignore, inv_t.data_ptr(), K,
             o.p("hist"), o.p("nll_fx"), o.p("nonfinite"), o.p("valid"), None)
    return o.digests()


def test_calib_temps(lib, want):
    cases = [(s, C, mode, 3, -1, False) for s in SIZES for C in CLASSES for mode in (0, 1)]
    cases += [((7, 9), C, mode, K, ign, False) for C in CLASSES for mode in (0, 1) for K in (1, 3) for ign in (-1, C - 1)]
    cases += [((7, 9), C, mode, 3, ign, True) for C in (3, 5) for mode in (0, 1) for ign in (-1, 1)]      # one all-ignored image
    for (oh, ow), C, mode, K, ign, ignored in cases:
        total = oh * ow
        labs = labels_for(total, C, 90 + C)
        if ignored:
            labs = torch.full((total,), ign if ign >= 0 else 255, dtype=torch.int64)
        got = calib_call(lib, dev(slot_for(C, 10 + C)), C, oh, ow, mode, dev(labs), ign, K)
        check(f"calib_temps/{oh}x{ow}/C{C}/mode{mode}/K{K}/ignore{ign}/{'all-ignored' if ignored else 'mixed'}", got)
    settle(want, "calib_temps")


# ---- the grid-stride loop's second trip -----------------------------------------------------------------------------------
def test_second_trip_counting(lib, want):
    """1024 x 800 = 819200 pixels with counts and labels: above the persistent grid's 3 x 256 CUs x 1024 pixels"""
    H, W, C = 1024, 800, 3
    total = H * W
    labs, pal = dev(labels_for(total, C, 101)), dev(palette_for(C))
    slot = dev(slot_for(C, 102))
    o = sink_outputs(total, C, True, True, True)
    lib.call("segk_predict_mask", slot.data_ptr(), o.p("mask"), o.p("color"), pal.data_ptr(), o.p("counts"), labs.data_ptr(), o.p("M"), C,
             T_SLOT, PT, PL, NH, NW, H, W, 0, None)
    check("second_trip/predict_mask", o.digests())
    table, slots = view_table(C, 3, (1, 2, 3), (0, 1, 0), 103)
    o = sink_outputs(total, C, True, True, True, True, True)
    lib.call("segk_predict_merge", table.data_ptr(), 3, C, PROB, 0, H, W, o.p("mask"), o.p("color"), pal.data_ptr(), o.p("counts"),
             labs.data_ptr(), o.p("M"), o.p("conf"), o.p("scores"), None)
    check("second_trip/predict_merge", o.digests())
    Y = tiles_input(C, H, W, 256, 0, 0, 104)
    o = sink_outputs(total, C, True, True, True, True, True)
    lib.call("segk_predict_tiles", Y.data_ptr(), C, 0, PROB, 1, H, W, 256, 0, o.p("mask"), o.p("color"), pal.data_ptr(), o.p("counts"),
             labs.data_ptr(), o.p("M"), o.p("conf"), o.p("scores"), None)
    check("second_trip/predict_tiles", o.digests())
    m = dev(mask_for(total, C, 105))
    o = sink_outputs(total, C, True, True, True, mask=False)
    lib.call("segk_mask_finish", m.data_ptr(), o.p("color"), pal.data_ptr(), o.p("counts"), labs.data_ptr(), o.p("M"), C, H, W, None)
    check("second_trip/mask_finish", o.digests())
    check("second_trip/calib_temps", calib_call(lib, slot, C, H, W, 0, labs, -1, 1))
    settle(want, "second_trip")


def test_second_trip_mask_only(lib, want):
    """4100 x 4100 mask-only: above the 16384 blocks x 1024 pixels of the plain grid"""
    C, side = 3, 4100
    slot = dev(slot_for(C, 106))
    o = sink_outputs(side * side, C, False, False, False)
    lib.call("segk_predict_mask", slot.data_ptr(), o.p("mask"), None, None, None, None, None, C, T_SLOT, PT, PL, NH, NW, side, side, 0, None)
    check("second_trip_mask_only/predict_mask", o.digests())
    settle(want, "second_trip_mask_only")
