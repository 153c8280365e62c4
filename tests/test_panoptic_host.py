"""CPU: proofs about the restatement of DESIGN.md 3.19 (tests/panoptic_reference.py) that do not depend on itself -- the pair
table is lossless and equals sklearn's contingency matrix where sklearn imports, its row and column sums are the component
areas, every match is unique, the hand cases give the numbers written in the case table -- and the host side of
image_segmentation_amd.panoptic: the header macros, the binding and ws_ints agree, the case table crosses every constant
csrc/panoptic.hip declares, no kernel spills, and argument errors are raised before any launch."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panoptic_cases as PC                                                        # noqa: E402
import panoptic_reference as PR                                                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("connectivity", [4, 8])
ALL = pytest.mark.parametrize("name", PC.NAMES)
HEADER = open(os.path.join(ROOT, "include", "segk.h")).read()


def macro(name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)", HEADER).group(1))


def roomy(name, connectivity):
    cap, mp = PC.regimes(name, connectivity)["roomy"]
    return PC.CASES[name], PC.reference(name, connectivity, cap, mp), cap


# ------------------------------------------------------------------------------------------------ the restatement
@ALL
@BOTH
def test_pair_table_is_lossless_and_ordered(name, connectivity):
    case, res, cap = roomy(name, connectivity)
    H, W = case["pred"].shape
    pairs = res["pairs"]
    assert res["totals"][0] == len(pairs) == res["P"] and pairs[:, 2].sum() == H * W and (pairs[:, 2] > 0).all()
    assert len({(g, p) for g, p, _ in pairs.tolist()}) == len(pairs)
    assert pairs[:, 0].min() >= -1 and pairs[:, 1].min() >= 0 and pairs.max(initial=0) <= max(H * W, cap + 8)
    # ascending first pixel, found without np.unique: scan the pixels in raster order
    Sg, Sp = res["Sg"].reshape(-1).tolist(), res["Sp"].reshape(-1).tolist()
    seen, order = set(), []
    for key in zip(Sg, Sp):
        if key not in seen:
            seen.add(key)
            order.append(key)
    assert order == [(g, p) for g, p, _ in pairs.tolist()]


@ALL
@BOTH
def test_sums_are_the_component_areas_and_matches_are_unique(name, connectivity):
    case, res, cap = roomy(name, connectivity)
    Sg, Sp = res["Sg"], res["Sp"]
    for ids, area, S in ((range(1, res["Kg"] + 1), res["area_g"], Sg), (range(1, res["Kp"] + 1), res["area_p"], Sp)):
        count = np.bincount(S[S > 0].reshape(-1), minlength=cap + 9)
        assert np.array_equal(area[:len(ids)], count[1:len(ids) + 1]) and np.array_equal(area[cap:], count[cap + 1:cap + 9])
    vp = np.bincount(Sp[(Sg == -1) & (Sp > 0)].reshape(-1), minlength=cap + 9)[1:]
    used = res["void_p"] >= 0
    assert np.array_equal(res["void_p"][used], vp[used])
    mg, mpd = res["match_g"], res["match_p"]
    tg, tp = mg[mg > 0], mpd[mpd > 0]
    assert len(set(tg.tolist())) == len(tg) == len(tp) == len(set(tp.tolist())) == res["totals"][3]
    for r in np.flatnonzero(mg > 0):                                       # the two sides point at each other, IoU > 1/2 recomputed
        p = mg[r]
        assert mpd[p - 1] == r + 1
        inter = int(((Sg == r + 1) & (Sp == p)).sum())
        union = int(((Sg == r + 1) | ((Sp == p) & (Sg != -1))).sum())
        assert (inter, union) == (res["inter_g"][r], res["union_g"][r]) and 2 * inter > union
    st = res["stats"]
    assert st[:, 0].sum() == res["totals"][3] and st[:, 14].sum() == res["totals"][1] and st[:, 15].sum() == res["totals"][2]
    assert np.array_equal(st[:, 4], st[:, 0]) and (np.diff(st[:, 4:14], axis=1) <= 0).all()
    assert np.array_equal(st[:, 0] + st[:, 2], st[:, 14]) and (st[:, 0] + st[:, 1] <= st[:, 15]).all()
    has = st[:, 0] > 0                                                    # every matched IoU lies in (1/2, 1]
    assert (st[:, 3] <= st[:, 0] << 32).all() and (st[has, 3] > st[has, 0] << 31).all() and not st[~has, 3].any()


@pytest.mark.parametrize("name", [n for n in PC.NAMES if PC.CASES[n]["pred"].size <= 128 * 160])
def test_contingency_equals_sklearn(name):
    cm = pytest.importorskip("sklearn.metrics.cluster").contingency_matrix
    case, res, cap = roomy(name, 4)
    T, gs, ps = PR.contingency(res)
    want = cm(res["Sg"].reshape(-1), res["Sp"].reshape(-1))               # rows / columns in ascending label order
    assert np.array_equal(T, want) and gs == np.unique(res["Sg"]).tolist() and ps == np.unique(res["Sp"]).tolist()


@pytest.mark.parametrize("name", PC.HAND)
@BOTH
def test_hand_cases_give_the_written_numbers(name, connectivity):
    case, res, cap = roomy(name, connectivity)
    want, st = case["want"], res["stats"]
    rows = {c: v for c, v in want.items() if isinstance(c, int)}
    for c in range(8):
        assert tuple(int(v) for v in st[c, :3]) == rows.get(c, (0, 0, 0)), (name, c)
    for c, v in want.get("col3", {}).items():
        assert int(st[c, 3]) == v
    for c, v in want.get("tp_at", {}).items():
        assert st[c, 4:14].tolist() == v
    q = PR.quality(st, sorted(case["things"] + case["stuff"]), 4)
    for c, (tp, fp, fn) in rows.items():
        if tp + fp + fn:
            assert q["rq"][c] == tp / (tp + fp / 2 + fn / 2)
    json.dumps(q)


def test_hand_checked_quality():
    q = PR.quality(PC.reference("cover5", 4, 5, 9)["stats"], [1], 2)
    assert q["pq"][1] == 3435973836 / 2 ** 32 and abs(q["pq"][1] - 0.8) < 2 ** -32 and q["sq"][1] == q["pq"][1] and q["rq"][1] == 1.0
    assert q["f1"][1] == [1.0] * 7 + [0.0] * 3 and q["mean_pq"] == q["pq"][1] and q["pq"][0] is None
    q = PR.quality(PC.reference("half_inside", 4, 5, 9)["stats"], [1], 2)
    assert q["pq"][1] == 0.0 and q["sq"][1] == 0.0 and q["rq"][1] == 0.0 and (q["tp"][1], q["fp"][1], q["fn"][1]) == (0, 1, 1)
    same = PC.reference("identical", 4, 40, 40)["stats"]
    assert (same[:, 3] == same[:, 0] << 32).all() and same[:, 1:3].sum() == 0 and same[:, 0].sum() > 20
    assert PR.quality(same, [0, 1, 2], 4)["mean_pq"] == 1.0
    assert PR.quality(PC.reference("all_nothing", 4, 5, 9)["stats"], [1, 2], 4)["mean_pq"] is None
    from image_segmentation_amd.panoptic import quality_from_stats
    st = PC.reference("noise0.5_3c_33x65", 4, 1000, 3000)["stats"]
    assert quality_from_stats(st.tolist(), [0, 1, 2, 3], 4) == PR.quality(st, [0, 1, 2, 3], 4)


def test_overflow_regimes_of_the_restatement():
    for name in ("split5", "noise0.5_3c_33x65"):
        reg = PC.regimes(name, 4)
        assert set(reg) == {"roomy", "exact", "pairs-1", "components-1"}
        for regime, (cap, mp) in reg.items():
            res = PC.reference(name, 4, cap, mp)
            over = regime.endswith("-1")
            assert (res["totals"].tolist() == [-1] * 4) == over and (len(res["pairs"]) == 0) == over
            assert (not res["stats"].any()) == over and ((res["area_g"] == -1).all() and (res["match_p"] == -1).all()) == over


# ------------------------------------------------------------------------------------------------ constants
def test_header_macros_binding_and_ws_ints_agree():
    from image_segmentation_amd import _lib, build, panoptic as P
    assert "panoptic.hip" in build.SOURCES
    assert (macro("SEGK_PQ_BLOCK_PIXELS"), macro("SEGK_PQ_LDS_SLOTS"), macro("SEGK_PQ_CHUNK"), macro("SEGK_PQ_MIN_SLOTS"),
            macro("SEGK_PQ_STAT_COLS")) == (P.BLOCK_PIXELS, P.LDS_SLOTS, P.CHUNK, P.MIN_SLOTS, P.STAT_COLS) == (2048, 256, 1024, 1024, 16)
    assert re.search(r"#define SEGK_PQ_MAX_PAIRS \(1L << 28\)", HEADER) and P.MAX_PAIRS == 1 << 28
    assert len(_lib.SIGNATURES["segk_pq_pairs"][1]) == 18 and len(_lib.SIGNATURES["segk_pq_match"][1]) == 19
    assert macro("SEGK_ABI_VERSION") == _lib.ABI_VERSION >= 327 and macro("SEGK_ENTRY_COUNT") == len(_lib.SIGNATURES) >= 113
    # the workspace macro, evaluated as written
    body = re.search(r"#define SEGK_PQ_WS_INTS\(H, W, MP, MC\)(.*?)\n(?=/\*)", HEADER, re.S).group(1).replace("\\\n", " ")
    slots = re.search(r"#define SEGK_PQ_SLOTS\(MP\) (.*)", HEADER).group(1)
    r4 = re.search(r"#define SEGK_VEC_R4\(n\) (.*)", HEADER).group(1)

    def c_eval(expr, **names):
        expr = re.sub(r"\(long\)", "", expr)
        expr = re.sub(r"(\d+)L\b", r"\1", expr).replace("/", "//")
        return eval(expr, {"SEGK_PQ_CHUNK": P.CHUNK, "SEGK_PQ_MIN_SLOTS": P.MIN_SLOTS,
                           "SEGK_PQ_SLOTS": lambda MP: c_eval(slots, MP=MP), "SEGK_VEC_R4": lambda n: c_eval(r4, n=n), **names})
    for H, W, mp, cap in ((1, 1, 1, 1), (7, 9, 100, 10), (200, 300, 25594, 23272), (375, 500, 4096, 1024), (3000, 4000, 1 << 22, 1 << 20),
                          (1 << 14, 1 << 14, 1 << 28, 1 << 24)):
        assert c_eval(body, H=H, W=W, MP=mp, MC=cap) == P.ws_ints(H, W, mp, cap), (H, W, mp, cap)
    assert P.ws_ints(1 << 14, 1 << 14, 1 << 28, 1 << 24) * 4 < 1 << 34         # 10 GB at the largest legal call
    for H, W, cap in ((1, 1, 1024), (64, 64, 1024), (375, 500, 1024), (3000, 4000, 1 << 20)):
        assert P.default_max_pairs(H, W, cap) == min(H * W, max(4096, 4 * cap))


def test_case_table_crosses_every_constant():
    """every tile, LDS-table, bitmap and scan-chunk constant of csrc/panoptic.hip has a case on both sides of it"""
    from image_segmentation_amd import panoptic as P
    kern = open(os.path.join(ROOT, "image_segmentation_amd", "csrc", "panoptic.hip")).read()
    declared = set(re.findall(r"\bSEGK_PQ_[A-Z_]+\b", kern))
    assert declared == {"SEGK_PQ_BLOCK_PIXELS", "SEGK_PQ_LDS_SLOTS", "SEGK_PQ_CHUNK", "SEGK_PQ_STAT_COLS", "SEGK_PQ_SLOTS",
                        "SEGK_PQ_MAX_PAIRS", "SEGK_PQ_WS_INTS"}, declared
    assert not re.search(r"constexpr int \w+ = \d{2,}", kern.replace("NOPIX = 0x7fffffff", "")), "a tile constant the header does not export"
    sizes = {n: PC.CASES[n]["pred"].size for n in PC.NAMES}
    # pixels: below one workgroup, exactly one, one more than one (a workgroup whose only wave holds one pixel), many
    assert min(sizes.values()) == 1 and P.BLOCK_PIXELS in sizes.values() and P.BLOCK_PIXELS + 1 in sizes.values()
    assert any(s % 64 for s in sizes.values()) and any(s % 32 and s > 32 for s in sizes.values()) and max(sizes.values()) > 7 * P.BLOCK_PIXELS
    # bitmap words per scan chunk: 32 * CHUNK pixels is one chunk; below, and more than one
    assert any(s < 32 * P.CHUNK for s in sizes.values()) and any(s > 32 * P.CHUNK and s % (32 * P.CHUNK) for s in sizes.values())
    # the LDS table: a workgroup's 2048 pixels hold more distinct pairs than it has slots (keys then go to the global table
    # directly), and in other cases fewer; the global table: more pairs than its floor of slots, and far fewer
    most = 0
    for n in ("noise0.5_3c_200x300", "noise0.9_3c_200x300", "noise0.5_3c_64x129"):
        res = roomy(n, 4)[1]
        key = (res["Sg"].reshape(-1) + 1) * (1 << 32) + res["Sp"].reshape(-1)
        most = max(most, max(len(np.unique(key[i:i + P.BLOCK_PIXELS])) for i in range(0, len(key), P.BLOCK_PIXELS)))
    assert most > 2 * P.LDS_SLOTS
    counts = {n: PC.true_counts(n, 4) for n in PC.NAMES}
    assert max(p for _, p in counts.values()) > 20 * P.MIN_SLOTS and min(p for _, p in counts.values()) == 1
    assert max(k for k, _ in counts.values()) > 8000
    # the statistics flush: a call whose segments span more than one workgroup of the classify pass (2 * (cap + 8) > 256)
    assert any(2 * (k + 8) > 256 for k, _ in counts.values()) and any(2 * (k + 8) < 256 for k, _ in counts.values())


def test_new_kernels_do_not_spill_and_nothing_syncs():
    import importlib.util
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    rep = importlib.util.module_from_spec(spec); spec.loader.exec_module(rep)
    rows = rep.report("panoptic")
    names = " ".join(r["name"] for r in rows)
    for k in ("pq_init_kernel", "pq_insert_kernel", "pq_mark_kernel", "pq_words_kernel", "pq_scan_kernel", "pq_emit_kernel", "pq_zero_kernel",
              "pq_area_kernel", "pq_test_kernel", "pq_classify_kernel"):
        assert k in names, k
    assert len(rows) == 11                                                 # pq_words_kernel in its two forms
    for r in rows:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
    kern = open(os.path.join(ROOT, "image_segmentation_amd", "csrc", "panoptic.hip")).read()
    device = re.sub(r"//.*", "", kern.split("int flat_grid")[0])
    assert "while (" not in device and not re.search(r"\b(float|double)\b", device)      # bounded loops, integers only
    src = open(os.path.join(ROOT, "image_segmentation_amd", "panoptic.py")).read()
    for fn in ("def match_objects(", "    def update("):
        body = src[src.index(fn):]
        body = body[:body.index("\n\n\n") if fn.startswith("def") else body.index("\n\n    def ")]
        assert not re.search(r"\.item\(|\.cpu\(|\.tolist\(|\.numpy\(|synchronize", body), fn


# ------------------------------------------------------------------------------------------------ refusals
def test_abi_refuses_bad_arguments():
    from image_segmentation_amd import _lib
    lib = _lib.load()
    err = lambda: lib.segk_last_error().decode()
    p = 256
    ptrs = [p] * 11
    assert lib.segk_pq_pairs(*ptrs[:10], None, 4, 4, 0, -1, 8, 8, None) == -2 and "NULL" in err()
    assert lib.segk_pq_pairs(*ptrs, 0, 4, 0, -1, 8, 8, None) == -2 and "shape" in err()
    assert lib.segk_pq_pairs(*ptrs, 1 << 15, 1 << 15, 0, -1, 8, 8, None) == -2 and "2^28" in err()
    assert lib.segk_pq_pairs(*ptrs, 4, 4, 256, -1, 8, 8, None) == -2 and "stuff_mask" in err()
    assert lib.segk_pq_pairs(*ptrs, 4, 4, 0, -2, 8, 8, None) == -2 and "ignore_index" in err()
    assert lib.segk_pq_pairs(*ptrs, 4, 4, 0, -1, 0, 8, None) == -2 and "max_components" in err()
    assert lib.segk_pq_pairs(*ptrs, 4, 4, 0, -1, 8, 0, None) == -2 and "max_pairs" in err()
    assert lib.segk_pq_pairs(*ptrs, 4, 4, 0, -1, 8, (1 << 28) + 1, None) == -2 and "max_pairs" in err()
    assert lib.segk_pq_pairs(*ptrs[:10], 260, 4, 4, 0, -1, 8, 8, None) == -2 and "aligned" in err()
    ptrs = [p] * 16
    assert lib.segk_pq_match(*ptrs[:15], None, 8, 8, None) == -2 and "NULL" in err()
    assert lib.segk_pq_match(*ptrs, (1 << 24) + 1, 8, None) == -2 and "max_components" in err()
    assert lib.segk_pq_match(*ptrs, 8, -1, None) == -2 and "max_pairs" in err()
    assert lib.segk_pq_match(*ptrs[:15], 260, 8, 8, None) == -2 and "aligned" in err()


class _Fake(torch.Tensor):
    """a CPU tensor that claims to live on the device: the argument checks run, and any launch would be a test failure"""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = True

    @property
    def device(self):
        return torch.device("cuda", 0)


def test_argument_errors_are_raised_with_no_launch(monkeypatch):
    import image_segmentation_amd as seg
    from image_segmentation_amd import _lib
    calls = []
    monkeypatch.setattr(_lib, "call", lambda *a: calls.append(a))
    m = _Fake(torch.zeros((6, 8), dtype=torch.uint8))
    t = _Fake(torch.zeros((6, 8), dtype=torch.int64))
    bad = [
        (dict(things=None), "things"), (dict(things=3), "iterable"), (dict(things=(8,)), "0..7"), (dict(things=(1,), stuff=(1,)), "share"),
        (dict(things=(), stuff=()), "both empty"), (dict(things=(1,), ignore_index=1), "ignore_index"),
        (dict(things=(1,), ignore_index=1.5), "ignore_index"), (dict(things=(1,), connectivity=6), "connectivity"),
        (dict(things=(1,), max_components=0), "max_components"), (dict(things=(1,), max_pairs=0), "max_pairs"),
        (dict(things=(1,), max_pairs=True), "max_pairs"), (dict(things=(1,), stats=torch.zeros((8, 16))), "stats"),
        (dict(things=(1,), target_objects=(t, t)), "int32"), (dict(things=(1,), target_objects=t), "pair"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            seg.match_objects(m, t, **kw)
    with pytest.raises(ValueError, match="integer map"):
        seg.match_objects(m, _Fake(torch.zeros((6, 8))), (1,))
    with pytest.raises(ValueError, match="integer map"):
        seg.match_objects(m, _Fake(torch.zeros((6, 9), dtype=torch.int64)), (1,))
    with pytest.raises(ValueError, match="uint8"):
        seg.match_objects(t, t, (1,))
    with pytest.raises(ValueError, match="exceed max_components"):
        seg.match_objects(m, t, (1,), max_components=2, target_objects=(_Fake(torch.zeros((6, 8), dtype=torch.int32)),
                                                                         _Fake(torch.zeros(3, dtype=torch.int32))))
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.match_objects(torch.zeros((6, 8), dtype=torch.uint8), t, (1,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.match_objects(m, torch.zeros((6, 8), dtype=torch.int64), (1,))
    for kw, msg in ((dict(num_classes=0), "num_classes"), (dict(num_classes=9), "num_classes"), (dict(num_classes=4, things=(5,)), "below"),
                    (dict(num_classes=4, stuff=(0,), things=(0, 1)), "share"), (dict(num_classes=4, tolerance=1), "unknown")):
        with pytest.raises(ValueError, match=msg):
            seg.PanopticQuality(**kw)
    pq = seg.PanopticQuality(4, stuff=(0,), ignore_index=3)
    assert pq.things == (1, 2) and pq.compute()["images"] == 0 and pq.compute()["mean_pq"] is None
    with pytest.raises(ValueError, match="same classes"):
        pq.add_(seg.PanopticQuality(4))
    with pytest.raises(ValueError, match="label maps"):
        seg.object_quality([m], [], 4)
    assert calls == []


def test_tools_know_the_new_family():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate_objects.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--min-area" in r.stdout and "--keep-largest" in r.stdout and "--things" in r.stdout
    src = open(os.path.join(ROOT, "tools", "kbench.py")).read()
    assert 'sys.argv[1] == "pq"' in src and "def pq():" in src
