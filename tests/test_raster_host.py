"""CPU: the host side of label rasterisation (image_segmentation_amd/raster.py) and proofs about its
restatement (tests/raster_reference.py) that do not depend on the kernel: the records and constants against include/segk.h,
every refusal, the tables of raster_plan, COCO's string codec, the restatement against the vector restatement of 3.17 (rings
and run-length codes of every vector case fill back to the map), the register report of the new unit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_cases as RC                                                          # noqa: E402
import raster_reference as RR                                                      # noqa: E402
import vector_cases as VC                                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "segk.h")).read()


def to_shapes(shapes):
    """the dict shapes of the case table as seg.Shape objects"""
    import image_segmentation_amd as seg
    return [seg.Shape(rings=s["rings"], value=s["value"]) if "rings" in s else seg.Shape(rle=s["rle"], value=s["value"]) for s in shapes]


def plan_of(name):
    import image_segmentation_amd as seg
    images, _ = RC.CASES[name]
    return seg.raster_plan([to_shapes(s) for s, _ in images], [hw for _, hw in images])


def cdiv(a, b):
    return -(-a // b)


def test_records_constants_and_entry_match_the_header():
    from image_segmentation_amd import raster as R, _lib
    define = lambda n: int(re.search(rf"#define {n} (\d+)", HEADER).group(1))
    assert (define("SEGK_RAST_TILE_H"), define("SEGK_RAST_TILE_W")) == (R.TILE_H, R.TILE_W) == (RC.TH, RC.TW)
    assert define("SEGK_RAST_MAX_SIDE") == R.MAX_SIDE and (define("SEGK_RAST_POLYGON"), define("SEGK_RAST_RLE")) == (R.POLYGON, R.RLE)
    for name, ct, dt in (("segk_rast_shape", R.RastShape, R.SHAPE_DTYPE), ("segk_rast_tile", R.RastTile, R.TILE_DTYPE)):
        m = re.search(rf"typedef struct {name} \{{\s*/\* one \w+; (\d+) bytes(.*?)\}} {name};", HEADER, re.S)
        size = int(m.group(1))
        assert size == C.sizeof(ct) == dt.itemsize == 32
        body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        fields = []
        for ctype, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
            fields += [(n.strip().split("[")[0], ctype) for n in names.split(",")]
        assert [f for f, _ in fields] == [f[0] for f in ct._fields_] == list(dt.names)
        for (f, ctype), cf in zip(fields, ct._fields_):
            assert getattr(ct, f).offset == dt.fields[f][1] and (C.sizeof(cf[1]) == 8) == (ctype == "int64_t")
    assert define("SEGK_ENTRY_COUNT") == len(_lib.SIGNATURES) and "segk_raster_labels" in _lib.SIGNATURES
    assert define("SEGK_ABI_VERSION") == _lib.ABI_VERSION
    assert "DESIGN.md 3.18" in HEADER[HEADER.index("segk_rast_tile;"):HEADER.index("int segk_raster_labels(")]
    from image_segmentation_amd import build
    assert "raster.hip" in build.SOURCES


def test_every_refusal_comes_before_the_device():
    import image_segmentation_amd as seg
    tri = [(0, 0), (4, 0), (0, 4)]
    for bad in (dict(), dict(rings=[tri], rle={"size": [2, 2], "counts": [4]}), dict(rings=[]), dict(rings=[[(0, 0), (1, 1)]]),
                dict(rings=[np.zeros((3, 3))]), dict(rings=[np.zeros((2, 3, 2))[0:0]]), dict(rings=[[(0, 0), (1, float("nan")), (2, 2)]]),
                dict(rings=[[(0, 0), (float("inf"), 1), (2, 2)]]), dict(rings=[[(0, 0), (16384.01, 1), (2, 2)]]),
                dict(rings=[[(0, 0), (-16385, 1), (2, 2)]]), dict(rings=[[("a", "b")] * 3]),
                dict(rings=[tri], value=256), dict(rings=[tri], value=-1), dict(rings=[tri], value=1.5), dict(rings=[tri], value=True),
                dict(rle={"size": [2, 2]}), dict(rle=[4]), dict(rle={"size": [2, 2, 1], "counts": [4]}),
                dict(rle={"size": [0, 2], "counts": []}), dict(rle={"size": [2, 8193], "counts": [2 * 8193]}),
                dict(rle={"size": [2, 2], "counts": [3]}), dict(rle={"size": [2, 2], "counts": [5, -1]}),
                dict(rle={"size": [2, 2], "counts": [1.5, 2.5]}), dict(rle={"size": [2, 2], "counts": "5"})):
        with pytest.raises((ValueError, TypeError)):
            seg.Shape(**bad)
    assert seg.Shape(rings=[[(0, 0), (16384, 1), (-16384, 2)]]).rings[0].tolist() == [[0, 0], [1 << 22, 256], [-(1 << 22), 512]]
    assert seg.Shape(rings=np.array(tri), value=np.uint8(7)).value == 7 and seg.Shape(rings=[torch.tensor(tri)]).rings[0].shape == (3, 2)
    assert seg.Shape(rle={"size": [2, 2], "counts": "4"}).counts.tolist() == [4]
    ok = seg.Shape(rings=[tri])
    for shapes, sizes in (([[ok]], [(0, 4)]), ([[ok]], [(4, 8193)]), ([[ok]], [(4,)]), ([[ok]], [(4.5, 4)]), ([[ok], []], [(4, 4)]),
                          ([], []), ([[seg.Shape(rle={"size": [2, 2], "counts": [4]})]], [(2, 3)]), ([[{"rings": [tri]}]], [(4, 4)])):
        with pytest.raises((ValueError, TypeError)):
            seg.raster_plan(shapes, sizes)
        with pytest.raises((ValueError, TypeError)):
            seg.rasterize_batch(shapes, sizes)
    for fill in (-1, 256, 0.5, None, True):
        with pytest.raises(ValueError):
            seg.rasterize([ok], (4, 4), fill=fill)
    with pytest.raises(ValueError, match="no CPU path"):
        seg.rasterize([ok], (4, 4), device="cpu")
    with pytest.raises(ValueError):
        seg.shapes_from_coco([{"category_id": 1, "segmentation": [[0, 0, 1, 1, 2]]}], {1: 1})
    with pytest.raises(ValueError):
        seg.shapes_from_coco([{"category_id": 1, "segmentation": [[0, 0, 1, 1]]}], {1: 1})
    # nothing in the launch path reads a value back
    src = open(os.path.join(ROOT, "image_segmentation_amd", "raster.py")).read()
    body = src[src.index("def launch("):]
    assert not re.search(r"\.item\(|\.cpu\(|\.tolist\(|\.numpy\(|synchronize", body)


def test_quantisation_is_floor_of_v_256_plus_half():
    import image_segmentation_amd as seg
    v = [(0.5 / 256, -0.5 / 256), (-0.002, 0.3), (3.999, 2.0 / 3), (1e-9, -1e-9)]
    q = seg.Shape(rings=[v]).rings[0]
    want = [[int(np.floor(x * 256 + 0.5)), int(np.floor(y * 256 + 0.5))] for x, y in v]
    assert q.dtype == np.int32 and q.tolist() == want == RR.quantize(v).tolist() and want[0] == [1, 0] and want[1][0] == -1
    p = seg.raster_plan([[seg.Shape(rings=[v, [(1, 1), (2, 1), (2, 2)]], value=9)]], [(4, 4)])
    e = p["edges"]
    assert e.dtype == np.int32 and e.shape == (7, 4) and e[:4, :2].tolist() == want and e[:4, 2:].tolist() == want[1:] + want[:1]
    assert e[4:].tolist() == [[256, 256, 512, 256], [512, 256, 512, 512], [512, 512, 256, 256]]       # the rings are flattened
    assert p["shapes"][0].tolist()[:5] == (0, 9, 0, 7, 4)


@pytest.mark.parametrize("name", RC.NAMES)
def test_plan_tiles_lists_and_boxes(name):
    from image_segmentation_amd import raster as R
    images, _ = RC.CASES[name]
    p = plan_of(name)
    tiles, lst, shp = p["tiles"], p["shape_list"], p["shapes"]
    assert p["edges"].dtype == p["run_start"].dtype == lst.dtype == np.int32 and tiles.dtype == R.TILE_DTYPE and shp.dtype == R.SHAPE_DTYPE
    assert len(shp) == sum(len(s) for s, _ in images)
    # every tile once, image after image; the images do not overlap in the output
    k = s0 = 0
    prev_end = 0
    for (shapes, (H, W)), off in zip(images, p["out_off"]):
        assert off >= prev_end and off % 256 == 0
        prev_end = off + H * W
        seen = np.zeros((H, W), np.int32)
        boxes = []
        for s in shapes:
            if "rings" in s:
                q = np.concatenate([RR.quantize(r) for r in s["rings"]])
                (xa, ya), (xb, yb) = q.min(axis=0), q.max(axis=0)
                # pixels whose centre 256 p + 128 lies in [min, max) of the vertices
                boxes.append((cdiv(int(ya) - 128, 256), cdiv(int(yb) - 128, 256), cdiv(int(xa) - 128, 256), cdiv(int(xb) - 128, 256)))
            else:
                cols = np.flatnonzero(RR.rle_inside(s["rle"], H, W).any(axis=0))
                boxes.append((0, H, int(cols[0]), int(cols[-1]) + 1) if cols.size else (0, 0, 0, 0))
        for j in range(cdiv(H, RC.TH)):
            for i in range(cdiv(W, RC.TW)):
                t = tiles[k]
                assert (t["out_off"], t["H"], t["W"], t["y0"], t["x0"]) == (off, H, W, j * RC.TH, i * RC.TW)
                seen[t["y0"]:t["y0"] + RC.TH, t["x0"]:t["x0"] + RC.TW] += 1
                y0, y1, x0, x1 = t["y0"], min(t["y0"] + RC.TH, H), t["x0"], min(t["x0"] + RC.TW, W)
                want = [s0 + n for n, (ya, yb, xa, xb) in enumerate(boxes) if max(ya, y0) < min(yb, y1) and max(xa, x0) < min(xb, x1)]
                assert lst[t["list0"]:t["list1"]].tolist() == want, (name, j, i)            # ascending: the paint order
                k += 1
        assert (seen == 1).all()
        for n, s in enumerate(shapes):
            rec = shp[s0 + n]
            assert rec["value"] == s["value"] and rec["H"] == H and rec["kind"] == (R.POLYGON if "rings" in s else R.RLE)
            if "rle" in s:
                counts = s["rle"]["counts"]
                assert p["run_start"][rec["begin"]:rec["end"]].tolist() == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
            else:
                assert rec["end"] - rec["begin"] == sum(len(r) for r in s["rings"])
        s0 += len(shapes)
    assert k == len(tiles) and p["out_bytes"] >= prev_end
    assert tiles["list1"][-1] == len(lst) and (tiles["list0"][1:] == tiles["list1"][:-1]).all()


def test_string_codec():
    import image_segmentation_amd as seg
    # hand-worked: 6 = group 6, nothing follows -> chr(54); 40 = 8 + 32*1: groups 8 (more) and 1 -> chr(8+32+48), chr(1+48);
    # -35 = ...11011101b: groups 29 (bit 0x10 set, rest -2 != -1: more) and 30 (rest -1: last) -> chr(29+32+48), chr(30+48)
    for v, s in ((6, "6"), (40, "X1"), (-35, "mN")):
        assert seg.rle_to_string([v]) == RR.counts_to_string([v]) == s
        assert seg.rle_from_string(s) == RR.string_to_counts(s) == [v]
    # from the fourth count on, differences to the count two before: negative ones need the sign extension
    counts = [0, 100, 3, 60, 40, 2, 1000000, 1, 1, 33, 15, 16, 17, 31, 32, 1023, 1024]
    s = seg.rle_to_string(counts)
    assert s == RR.counts_to_string(counts) and seg.rle_from_string(s) == RR.string_to_counts(s) == counts
    assert seg.rle_from_string(s.encode()) == counts and seg.rle_to_string([]) == "" and seg.rle_from_string("") == []
    for bad in ("X", "\x1f", 7):
        with pytest.raises((ValueError, TypeError)):
            seg.rle_from_string(bad)
    for name in RC.RLE_NAMES:
        for shapes, (H, W) in RC.CASES[name][0]:
            for sh in shapes:
                if "rle" in sh:
                    c = sh["rle"]["counts"]
                    s = seg.rle_to_string(c)
                    assert s == RR.counts_to_string(c) and seg.rle_from_string(s) == c == RR.string_to_counts(s)
                    a = seg.Shape(rle={"size": [H, W], "counts": s}, value=3)
                    assert a.counts.tolist() == c and a.size == (H, W)


def test_hand_checked_maps_of_the_restatement():
    ref = lambda n: RC.reference(n)[0]
    assert ref("unit_1x1").tolist() == [[1]] and (ref("no_shapes") == 3).all()
    # centres on the hypotenuse x + y = 5 are OUT (the crossing lies at the centre: counted, so the count is even again),
    # centres on the left edge x = 0.5 are IN (at or left of the centre), the top row y = 0.5 is IN (Y0 <= Yc), y = 4.5 is OUT
    tri = np.zeros((6, 6), np.uint8)
    for y in range(4):
        tri[y, 0:4 - y] = 1
    assert np.array_equal(ref("centre_triangle"), tri)
    rect = np.zeros((6, 6), np.uint8)
    rect[1:3, 1:4] = 1                                                     # rows 1, 2 (1.5 <= Yc < 3.5), columns 1..3
    assert np.array_equal(ref("scanline_rect"), rect)
    assert ref("bowtie")[5, 6] == 0 and ref("bowtie")[5, 2] == 5 and ref("pentagram")[10, 10] == 0 and ref("pentagram")[4, 10] == 6
    assert not ref("collinear").any()
    sl = ref("sliver")
    assert (sl[:, 5] == 1).all() and not sl[:, 8:10].any() and (sl == 3).sum() > 0 and (sl == 3).sum(axis=1).max() == 1
    for n in ("outside_left", "outside_right", "outside_top", "outside_bottom"):
        assert not ref(n).any()
    assert (ref("overhang") == 4).all()
    assert ref("order_ab")[5, 6] == 2 and ref("order_ba")[5, 6] == 1
    assert ref("two_rings_one_shape")[5, 6] == 0 and ref("two_rings_two_shapes")[5, 6] == 1
    assert ref("value_is_fill")[2, 4] == 0 and ref("value_is_fill")[4, 2] == 2
    d = ref("diag_8x8192")                                                  # below the diagonal y = x / 1024
    assert d[0, 0] == 3 and d[0, 511] == 3 and d[0, 512] == 0 and d[7, 7679] == 3 and d[7, 7680] == 0
    assert np.array_equal(ref("diag_8192x8"), d.T)                          # no centre lies on an edge: the transpose exactly
    assert (ref("rle_all_background") == 1).all() and (ref("rle_all_foreground") == 2).all()
    assert ref("rle_across_columns").T.reshape(-1).tolist() == [0] * 3 + [1] * 9 + [0] * 2 + [1] * 6
    assert ref("rle_zero_counts").T.reshape(-1).tolist() == [0] * 5 + [1] * 10 + [0] * 5    # empty runs between
    b = RC.reference("batch")
    assert [x.shape for x in b] == [(70, 300), (9, 5), (20, 20)] and (b[1] == 8).all()
    for H, W in ((64, 256), (63, 255), (65, 257), (129, 513), (1, 300), (300, 1)):
        lab = ref(f"tiles_{H}x{W}")
        for j in range(cdiv(H, RC.TH)):                                    # the spanning shape reaches every tile that has a centre
            for i in range(cdiv(W, RC.TW)):
                if min(H, W) > 1:
                    assert (lab[j * RC.TH:(j + 1) * RC.TH, i * RC.TW:(i + 1) * RC.TW] != 7).any(), (H, W, j, i)


@pytest.mark.parametrize("name", VC.NAMES)
def test_restatement_fills_the_vector_cases(name):
    """3.18 against 3.17: one even-odd shape per object from the rings of tests/vector_reference.py rebuilds the object map;
    the run-length code of every object decodes to O == k"""
    import image_segmentation_amd as seg
    for connectivity in (4, 8) if name in ("hole_island", "diag_same", "raw_diag_same", "checker16", "noise0.5_3c_37x53") else (4,):
        O, full = VC.object_map(name, connectivity), VC.reference(name, connectivity)
        H, W = O.shape
        off = full["ring_offset"]
        ids = np.unique(O[O != 0])
        shapes = [{"rings": [full["xy"][off[i]:off[i + 1]] for i in np.flatnonzero(full["ring_obj"] == k)], "value": int(k) % 251 + 1}
                  for k in ids]
        want = np.where(O != 0, O % 251 + 1, 0).astype(np.uint8)
        assert np.array_equal(RR.render(shapes, H, W, 0), want), (name, connectivity)
        for k in ids[:12]:
            counts = RR.mask_to_counts(O == k)
            assert np.array_equal(RR.rle_inside({"size": [H, W], "counts": counts}, H, W), O == k)
            s = seg.rle_to_string(counts)
            assert np.array_equal(RR.rle_inside({"size": [H, W], "counts": s}, H, W), O == k)


def test_shapes_from_coco_and_vectors_and_compressed_to_coco():
    import image_segmentation_amd as seg
    from test_vectors_host import vectors_from
    name = "hole_island"
    full, rows = VC.reference(name, 4), VC.labelled(name, 4)[1]
    O = VC.object_map(name, 4)
    vec = vectors_from(full, rows)
    plain, packed = vec.to_coco(7, {1: 11}), vec.to_coco(7, {1: 11}, compressed=True)
    assert plain == vec.to_coco(7, {1: 11}, compressed=False) and isinstance(plain[0]["segmentation"]["counts"], list)
    assert isinstance(packed[0]["segmentation"]["counts"], str) and packed[1] == plain[1]
    assert seg.rle_from_string(packed[0]["segmentation"]["counts"]) == plain[0]["segmentation"]["counts"]
    assert {k: v for k, v in packed[0].items() if k != "segmentation"} == {k: v for k, v in plain[0].items() if k != "segmentation"}
    for anns in (plain, packed):
        shapes = seg.shapes_from_coco(anns, {11: 2})
        assert [s.kind for s in shapes] == [1, 0] and [s.value for s in shapes] == [2, 2]
        assert shapes[0].counts.tolist() == plain[0]["segmentation"]["counts"] and shapes[1].rings[0].tolist() == [[512, 512], [1280, 512], [1280, 1280], [512, 1280]]
    assert seg.shapes_from_coco(plain, {5: 1}) == [] and [s.value for s in seg.shapes_from_coco(plain, {11: 2}, crowd_value=255)] == [255, 2]
    two = seg.shapes_from_coco([{"category_id": 1, "segmentation": [[0, 0, 4, 0, 0, 4], [5, 5, 9, 5, 5, 9.5]]}], {1: 3})
    assert len(two) == 2 and all(len(s.rings) == 1 for s in two)            # one Shape per polygon: their union
    sv = seg.shapes_from_vectors(vec)
    assert [(s.value, len(s.rings)) for s in sv] == [(1, 2), (1, 1)]                       # the ring object carries its hole
    ref = RR.render([{"rings": [r / 256 for r in s.rings], "value": s.value} for s in sv], *O.shape)
    assert np.array_equal(ref, (O != 0).astype(np.uint8))
    assert [s.value for s in seg.shapes_from_vectors(vec, {1: 9})] == [9, 9] and seg.shapes_from_vectors(vec, {2: 9}) == []


def test_abi_refuses_bad_arguments():
    from image_segmentation_amd import _lib
    lib = _lib.load()
    err = lambda: lib.segk_last_error().decode()
    p = 256
    good = [p, 1, p, 1, p, 1, p, 3, p, 0, p, 64, 0, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.segk_raster_labels(*a)
    for i in (0, 2, 4, 6, 8, 10):
        assert call(**{f"a{i}": None}) == -2 and "NULL" in err()
    assert call(a1=0) == -2 and "n_tiles" in err()
    assert call(a1=-1) == -2 and "n_tiles" in err()
    for i in (3, 5, 7, 9):
        assert call(**{f"a{i}": -1}) == -2 and "negative" in err()
    assert call(a11=0) == -2 and "out_bytes" in err()
    assert call(a1=65, a11=64) == -2 and "out_bytes" in err()
    assert call(a12=256) == -2 and "fill" in err()
    assert call(a12=-1) == -2 and "fill" in err()
    assert call(a0=260) == -2 and "misaligned" in err()
    assert call(a6=264) == -2 and "misaligned" in err()


def test_unit_compiles_without_spills_and_tools_know_it():
    import importlib.util
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    rep = importlib.util.module_from_spec(spec); spec.loader.exec_module(rep)
    rows = rep.report("raster")
    assert len(rows) >= 1
    for r in rows:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
    kern = open(os.path.join(ROOT, "image_segmentation_amd", "csrc", "raster.hip")).read()
    dev = kern.split('extern "C"')[0]
    assert "while (" not in dev                                            # no device loop without a bound
    assert not re.search(r"atomic\w*\((?!&s_)", dev)                       # the only atomics are on LDS
    src = open(os.path.join(ROOT, "tools", "kbench.py")).read()
    assert 'sys.argv[1] == "raster"' in src and "def raster():" in src
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rasterize.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--categories" in r.stdout
