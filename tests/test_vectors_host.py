"""CPU: proofs about the restatement of DESIGN.md 3.17 (tests/vector_reference.py) that do not depend on its ring walk -- the
run table rebuilds the map, an even-odd fill of every object's rings is the object, the ring areas sum to the component
area -- and the host side of image_segmentation_amd.vectors: Vectors' methods on CPU tensors made from the restatement, the
argument checks, the workspace size, truncate()."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vector_cases as VC                                                          # noqa: E402
import vector_reference as VR                                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("connectivity", [4, 8])
ALL = pytest.mark.parametrize("name", VC.NAMES)


def polys_of(full, k):
    off = full["ring_offset"]
    return [full["xy"][off[i]:off[i + 1]] for i in np.flatnonzero(full["ring_obj"] == k)]


def vectors_from(full, rows, caps=None):
    """a Vectors of CPU tensors holding the restatement's result (optionally truncated into 0xFF-filled arrays)"""
    from image_segmentation_amd.vectors import Vectors
    runs, E, R, V = (int(v) for v in full["totals"])
    caps = caps or (max(1, runs), max(1, E), max(1, R), max(1, V))
    t = VR.truncate(full, *caps)

    def arr(name, n, dtype=np.int32, tail=()):
        a = np.full((n,) + tail, -1, dtype)
        a[:len(t[name])] = t[name]
        return torch.from_numpy(a)
    K = len(rows)
    i32 = lambda k, shape: torch.from_numpy(np.asarray([r[k] for r in rows], dtype=np.int32).reshape(shape))
    return Vectors(arr("run_start", caps[0]), arr("run_obj", caps[0]), arr("ring_obj", caps[2]), arr("ring_head", caps[2]),
                   arr("ring_len", caps[2]), arr("ring_area2", caps[2], np.int64), arr("ring_offset", caps[2] + 1),
                   arr("xy", caps[3], tail=(2,)), torch.from_numpy(t["totals"].copy()), torch.tensor([K], dtype=torch.int32),
                   i32("cls", K), i32("area", K), i32("box", (K, 4)), full["size"], full["connectivity"], caps[1])


@ALL
@BOTH
def test_run_table_rebuilds_the_map(name, connectivity):
    O, full = VC.object_map(name, connectivity), VC.reference(name, connectivity)
    H, W = O.shape
    s, o = full["run_start"], full["run_obj"]
    assert s[0] == 0 and (np.diff(s) > 0).all() and (o[1:] != o[:-1]).all()
    assert np.array_equal(VR.rebuild_from_runs(s, o, H, W), O)
    assert full["totals"][0] == len(s) <= full["totals"][1] + W            # the bound the default capacities rest on


@ALL
@BOTH
def test_rings_fill_to_their_objects_and_areas_add_up(name, connectivity):
    O, full = VC.object_map(name, connectivity), VC.reference(name, connectivity)
    H, W = O.shape
    runs, E, R, V = (int(v) for v in full["totals"])
    assert E == len(VR.edge_keys(O)) == int(full["ring_len"].sum()) and R == len(full["ring_obj"]) and V == len(full["xy"])
    assert R <= E // 4 and V <= E and (np.diff(full["ring_head"]) > 0).all()
    assert full["ring_offset"][0] == 0 and full["ring_offset"][-1] == V and (np.diff(full["ring_offset"]) >= 4).all()
    for k in np.unique(O[O != 0]):
        mine = full["ring_obj"] == k
        assert np.array_equal(VR.fill_even_odd(polys_of(full, k), H, W), O == k), (name, int(k))
        a2 = full["ring_area2"][mine]
        assert a2.sum() == 2 * int((O == k).sum()) and (a2 != 0).all()
        if connectivity == 4 and name not in VC.RAW:
            assert (a2 > 0).sum() == 1                                     # a 4-connected object has ONE outer ring


def test_hand_checked_records():
    full = VC.reference("1x1", 4)
    assert full["totals"].tolist() == [1, 4, 1, 4] and full["ring_head"].tolist() == [0] and full["ring_area2"].tolist() == [2]
    assert full["xy"].tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    assert VC.reference("zeros", 4)["totals"].tolist() == [1, 0, 0, 0] and VC.reference("zeros", 8)["ring_offset"].tolist() == [0]
    hole = VC.reference("hole", 4)                                         # 3 x 3 ring of class 1 around one background pixel
    assert hole["ring_area2"].tolist() == [18, -2] and hole["ring_len"].tolist() == [12, 4]
    assert hole["ring_head"].tolist() == [0, 4 * 1 + 2]                    # the hole's smallest key: bottom side of pixel (0, 1)
    assert hole["xy"][4:].tolist() == [[2, 1], [1, 1], [1, 2], [2, 2]]     # the hole runs the other way round
    # two pixels of ONE object that touch diagonally: connectivity 4 keeps two rings, connectivity 8 joins them into one
    assert VC.reference("raw_diag_same", 4)["ring_len"].tolist() == [4, 4]
    one = VC.reference("raw_diag_same", 8)
    assert one["ring_len"].tolist() == [8] and one["ring_area2"].tolist() == [4] and len(one["xy"]) == 8
    assert VC.reference("diag_same", 4)["ring_obj"].tolist() == [1, 2] and VC.reference("diag_same", 8)["ring_obj"].tolist() == [1]
    assert VC.reference("diag_other", 8)["ring_obj"].tolist() == [1, 2]
    ch = VC.reference("checker16", 4)
    assert ch["totals"].tolist() == [256, 4 * 256, 256, 4 * 256]
    s = VC.reference("serpentine", 4)
    assert s["totals"][2] == 1 and s["totals"][1] > 4000                    # ONE ring of a few thousand edges
    assert VC.reference("nested3", 4)["totals"][2] == 6 and (VC.reference("nested3", 4)["ring_area2"] < 0).sum() == 3


def test_checker_rings_closed_form_is_the_restatement():
    """the large case of tests/test_gpu_vectors.py is compared with VC.checker_rings alone: here it meets the ring walk"""
    O, full = VC.checker_rings(8)
    want = VR.vectorize(O, 4)
    assert full["size"] == want["size"] and full["totals"].tolist() == want["totals"].tolist() and full["totals"][1:].tolist() == [128, 32, 128]
    for n in ("run_start", "run_obj") + VR.RING_ARRAYS:
        assert full[n].dtype == want[n].dtype and np.array_equal(full[n], want[n]), n
    O, full = VC.checker_rings(1026)                                       # what the GPU test relies on
    E = int(full["totals"][1])
    assert (E + 2047) // 2048 > 1024 and O.max() == E // 4 and np.array_equal(VR.rebuild_from_runs(full["run_start"], full["run_obj"], 1026, 1026), O)


def test_scan_cases_cross_the_trip_size():
    """column segments of the run table = W * ceil(H / 128): one case past 1024 in one tile row, one in two"""
    for name, nj in (("noise0.5_3c_2x1100", 1), ("stripes130x520", 2)):
        H, W = VC.MASKS[name][0].shape
        assert (H + 127) // 128 == nj and 1024 < W * nj <= 2048
        assert VC.reference(name, 4)["totals"][0] > W * nj                 # more runs than segments: the counts are not all 1


def test_cross_check_with_scipy_where_installed():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name in ("hole_island", "nested3", "stripes33x65", "noise0.5_1c_120x77"):
        O, full = VC.object_map(name, 4), VC.reference(name, 4)
        for k in np.unique(O[O != 0])[:40]:                                # holes of a 4-connected object are 8-connected
            pad = np.pad(O == k, 1)
            holes = ndimage.label(~pad, structure=np.ones((3, 3)))[1] - 1
            assert ((full["ring_obj"] == k) & (full["ring_area2"] < 0)).sum() == holes, (name, int(k))


@pytest.mark.parametrize("name", ["hole_island", "checker16", "stripes33x65", "noise0.5_3c_200x300", "1x7", "zeros"])
@BOTH
def test_coco_rle_and_polygons_of_cpu_vectors(name, connectivity):
    O, full = VC.object_map(name, connectivity), VC.reference(name, connectivity)
    H, W = O.shape
    rows = VC.labelled(name, connectivity)[1]
    vec = vectors_from(full, rows)
    assert vec.complete
    for k in list(range(1, len(rows) + 1))[:25]:
        rle = vec.coco_rle(k)
        assert rle["size"] == [H, W] and sum(rle["counts"]) == H * W and all(c > 0 for c in rle["counts"][1:])
        assert (rle["counts"][0] == 0) == bool(O[0, 0] == k)
        assert np.array_equal(VR.rle_decode(rle), O == k)
        polys = vec.polygons(k)
        assert [p[0] for p in polys] == [k] * len(polys) and sum(p[1] for p in polys) == 2 * rows[k - 1]["area"]
        assert np.array_equal(VR.fill_even_odd([p[2] for p in polys], H, W), O == k)
    assert len(vec.polygons()) == full["totals"][2]


def test_to_coco():
    name = "hole_island"
    full, rows = VC.reference(name, 4), VC.labelled(name, 4)[1]
    vec = vectors_from(full, rows)
    ann = vec.to_coco(7, {1: 11}, first_id=100)
    json.dumps(ann)                                                        # plain Python numbers throughout
    assert [a["id"] for a in ann] == [100, 101] and all(a["image_id"] == 7 and a["category_id"] == 11 for a in ann)
    ring, island = ann
    assert ring["bbox"] == [0, 0, 7, 7] and ring["area"] == 24 and ring["iscrowd"] == 1       # it has a hole: RLE
    assert ring["segmentation"]["size"] == [7, 7] and np.array_equal(VR.rle_decode(ring["segmentation"]), VC.object_map(name, 4) == 1)
    assert island["bbox"] == [2, 2, 3, 3] and island["area"] == 9 and island["iscrowd"] == 0
    assert island["segmentation"] == [[2, 2, 5, 2, 5, 5, 2, 5]]
    assert vec.to_coco(1, {}) == [] and vec.to_coco(1, {2: 5}) == []                           # background is skipped
    # every class of a mask with 8 object classes, class 0 left out as background
    name = "noise0.9_8c_120x77"
    full, rows = VC.reference(name, 8), VC.labelled(name, 8)[1]
    ann = vectors_from(full, rows).to_coco("img", {c: c for c in range(1, 8)})
    assert len(ann) == sum(r["cls"] != 0 for r in rows) and [a["id"] for a in ann] == list(range(1, len(ann) + 1))
    assert sum(a["area"] for a in ann) == int((VC.MASKS[name][0] != 0).sum())


def test_truncate_and_incomplete_vectors():
    full, rows = VC.reference("hole_island", 4), VC.labelled("hole_island", 4)[1]
    runs, E, R, V = (int(v) for v in full["totals"])
    t = VR.truncate(full, 3, E, 2, 5)
    assert t["totals"].tolist() == [runs, E, R, V] and len(t["run_start"]) == 3 and len(t["ring_obj"]) == 2
    assert t["ring_offset"].tolist() == full["ring_offset"][:3].tolist() and len(t["xy"]) == 5
    t = VR.truncate(full, runs, E - 1, R, V)
    assert t["totals"].tolist() == [runs, E, -1, -1] and all(len(t[n]) == 0 for n in VR.RING_ARRAYS) and len(t["run_start"]) == runs
    assert np.array_equal(VR.truncate(full, runs + 9, E + 9, R + 9, V + 9)["xy"], full["xy"])
    vec = vectors_from(full, rows, (runs, E - 1, R, V))
    assert not vec.complete and vec.coco_rle(1)["counts"]
    with pytest.raises(RuntimeError, match="max_edges"):
        vec.polygons()
    vec = vectors_from(full, rows, (2, E, R - 1, V))
    assert not vec.complete
    with pytest.raises(RuntimeError, match="max_rings"):
        vec.to_coco(1, {1: 1})
    with pytest.raises(RuntimeError, match="max_runs"):
        vec.coco_rle(1)
    assert not vectors_from(full, rows, (runs, E, R, V - 1)).complete and vectors_from(full, rows, (runs, E, R, V)).complete


def test_argument_checks_and_no_cpu_path():
    import image_segmentation_amd as seg
    from image_segmentation_amd import vectors as V
    m = torch.zeros((4, 5), dtype=torch.uint8)
    with pytest.raises(Exception, match="(?i)cuda|device|gpu"):
        seg.vectorize(m)
    for kw in (dict(connectivity=6), dict(classes=3), dict(classes=(9,)), dict(max_components=0), dict(max_runs=0),
               dict(max_edges=-1), dict(max_rings=True), dict(max_vertices=(1 << 30) + 1), dict(max_edges=2.5)):
        with pytest.raises(ValueError):
            seg.vectorize(m, **kw)                                         # refused before the device is looked at
    with pytest.raises(ValueError):
        seg.vectorize(np.zeros((4, 5), np.uint8))
    assert V.as_vectors(None) is None and V.as_vectors(False) is None and V.as_vectors(True) == {}
    assert V.as_vectors({"connectivity": 8, "max_edges": 100}) == {"connectivity": 8, "max_edges": 100}
    for bad in ({"min_area": 3}, {"connectivity": 5}, {"max_edges": 0}, 4, "yes"):
        with pytest.raises(ValueError):
            V.as_vectors(bad)
    with pytest.raises(ValueError):
        seg.Segmenter(seg.unet(3, 3), vectors={"connectivity": 3})
    assert seg.Segmenter(seg.unet(3, 3)).vectors is None and seg.Prediction.vectors is None


def test_default_capacities_and_workspace_size():
    from image_segmentation_amd import vectors as V, _lib
    for H, W in ((1, 1), (7, 9), (64, 64), (375, 500), (3000, 4000)):
        mr, me, mg, mv = V.default_capacities(H, W)
        assert me == min(4 * H * W, max(4096, H * W // 2)) and mr == min(H * W, me + W) and mg == max(1, me // 4) and mv == me
    # exact for every case whose boundary is within the stated share
    for name in VC.NAMES:
        full = VC.reference(name, 4)
        H, W = full["size"]
        runs, E, R, Vn = (int(v) for v in full["totals"])
        mr, me, mg, mv = V.default_capacities(H, W)
        if E <= me:
            assert runs <= mr and R <= mg and Vn <= mv, name
    txt = open(os.path.join(ROOT, "include", "segk.h")).read()
    body = re.search(r"#define SEGK_VEC_WS_INTS\(H, W, ME\)(.*?)\n(?=/\*)", txt, re.S).group(1).replace("\\\n", " ")
    r4 = re.search(r"#define SEGK_VEC_R4\(n\)\s+(.*)", txt).group(1)
    assert int(re.search(r"#define SEGK_VEC_CHUNK (\d+)", txt).group(1)) == V.CHUNK
    assert "1L << 30" in re.search(r"#define SEGK_VEC_MAX_CAP (.*)", txt).group(1) and V.MAX_CAP == 1 << 30

    def macro(H, W, ME):
        R4 = lambda n: eval(re.sub(r"\(long\)|L\b", "", r4).replace("/", "//"), {"n": n})
        expr = re.sub(r"\(long\)|(?<=\d)L\b", "", body).replace("SEGK_VEC_CHUNK", str(V.CHUNK)).replace("SEGK_VEC_R4", "R4").replace("/", "//")
        return eval(expr, {"R4": R4, "H": H, "W": W, "ME": ME})
    for H, W, ME in ((1, 1, 1), (7, 9, 13), (64, 32, 2048), (65, 33, 2049), (375, 500, 93750), (3000, 4000, 6000000)):
        assert macro(H, W, ME) == V.ws_ints(H, W, ME), (H, W, ME)
        assert V.ws_ints(H, W, ME) >= W * ((H + 127) // 128)               # segk_vec_runs' segment table fits
    assert {"segk_vec_runs", "segk_vec_rings"} <= set(_lib.SIGNATURES)


def test_abi_refuses_bad_arguments():
    from image_segmentation_amd import _lib
    lib = _lib.load()
    err = lambda: lib.segk_last_error().decode()
    p = 256
    assert lib.segk_vec_runs(p, p, p, p, None, 4, 4, 8, None) == -2 and "NULL" in err()
    assert lib.segk_vec_runs(p, p, p, p, p, 0, 4, 8, None) == -2 and "shape" in err()
    assert lib.segk_vec_runs(p, p, p, p, p, 1 << 15, 1 << 15, 8, None) == -2 and "2^28" in err()
    assert lib.segk_vec_runs(p, p, p, p, p, 4, 4, 0, None) == -2 and "max_runs" in err()
    assert lib.segk_vec_runs(p, p, p, p, 260, 4, 4, 8, None) == -2 and "aligned" in err()
    ok = (4, 4, 4, 64, 16, 64)
    assert lib.segk_vec_rings(p, p, p, p, p, p, p, None, p, *ok, None) == -2 and "NULL" in err()
    assert lib.segk_vec_rings(p, p, p, p, p, p, p, p, p, 4, 4, 6, 64, 16, 64, None) == -2 and "connectivity" in err()
    assert lib.segk_vec_rings(p, p, p, p, p, p, p, p, p, 4, 4, 4, 0, 16, 64, None) == -2 and "max_edges" in err()
    assert lib.segk_vec_rings(p, p, p, p, p, p, p, p, p, 4, 4, 4, 64, -3, 64, None) == -2 and "max_rings" in err()
    assert lib.segk_vec_rings(p, p, p, p, p, p, p, p, p, 4, 4, 4, 64, 16, 0, None) == -2 and "max_vertices" in err()
    assert lib.segk_vec_rings(p, p, p, p, 260, p, p, p, p, *ok, None) == -2 and "aligned" in err()


def test_new_kernels_do_not_spill_and_nothing_syncs():
    import importlib.util
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    rep = importlib.util.module_from_spec(spec); spec.loader.exec_module(rep)
    rows = rep.report("vectors")
    assert len(rows) >= 12
    for r in rows:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
    # vectorize() returns without a host synchronisation: nothing in it reads a value back
    src = open(os.path.join(ROOT, "image_segmentation_amd", "vectors.py")).read()
    body = src[src.index("def vectorize("):]
    assert not re.search(r"\.item\(|\.cpu\(|\.tolist\(|\.numpy\(|synchronize", body)
    kern = open(os.path.join(ROOT, "image_segmentation_amd", "csrc", "vectors.hip")).read()
    assert "while (" not in kern.split("extern \"C\"")[0]                   # no device loop without a bound from the host


def test_tools_know_the_new_options():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--coco FILE.json" in r.stdout and "--coco-categories" in r.stdout
    for extra, msg in ((["--coco-categories", "1=cat"], "needs --coco"), (["--coco", "x.json", "--coco-categories", "cat"], "CLASS=NAME"),
                       (["--coco", "x.json", "--coco-categories", "9=cat"], "classes in 0..3")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--checkpoint", "none.pt", "--out", "none", *extra,
                            "a.png"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, r.stderr
    src = open(os.path.join(ROOT, "tools", "kbench.py")).read()
    assert 'sys.argv[1] == "vectors"' in src and "def vectors():" in src
