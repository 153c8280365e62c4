"""The case table tests/test_vectors_host.py and tests/test_gpu_vectors.py share.  Host-only.

A case is a uint8 class mask with the classes that form objects; its object map at a connectivity is the labelling of
tests/components_reference.py (cached, as is the restatement's result).  RAW cases give the object map itself: maps no
labelling produces (one id on two pixels that touch only diagonally, at connectivity 4) are still defined input of the
C ABI.  The shapes are the smallest at which each mechanism can go wrong: the run-table tile is 128 rows x 32 columns, a
scan block 2048 items, SEGK_CC_TILE 32 rows x 64 columns, and the ONE workgroup that scans the block partials takes 1024 of
them per trip (csrc/scan.hpp): 2 x 1100 and 130 x 520 give it 1100 and 2 * 520 column segments, checker_rings(1026) more than
1024 blocks of 2048 edges."""
import functools

import numpy as np

import components_reference as cref
import vector_reference as vref

FG = (1, 2, 3, 4, 5, 6, 7)          # class 0 is background unless a case says otherwise


def _stripes(H, W, band=4):
    """diagonal bands of the classes 0, 1, 2, `band` pixels wide: rings cross every tile border"""
    y, x = np.mgrid[:H, :W]
    return (((x + y) // band) % 3).astype(np.uint8)


def _nested(n):
    """concentric one-pixel square rings of class 1 around each other, n deep (hole, island, hole ...)"""
    S = 4 * n - 1
    m = np.zeros((S, S), np.uint8)
    for i in range(n):
        m[2 * i:S - 2 * i, 2 * i:S - 2 * i] = 1
        if 2 * i + 1 < S - 2 * i - 1:
            m[2 * i + 1:S - 2 * i - 1, 2 * i + 1:S - 2 * i - 1] = 0
    return m


def _serpentine(S=64):
    """a one-pixel-wide path: every other row, joined alternately at the right and the left end -- ONE ring"""
    m = np.zeros((S, S), np.uint8)
    m[0::2, :] = 1
    for i, y in enumerate(range(1, S - 1, 2)):
        m[y, S - 1 if i % 2 == 0 else 0] = 1
    return m


def _noise(H, W, density, nclass, seed):
    rng = np.random.default_rng(seed)
    fg = rng.random((H, W)) < density
    if nclass == 8:                 # all eight classes form objects, class 0 too; density: the share of pixels != 0
        v = rng.integers(1, 8, (H, W))
    else:
        v = rng.integers(1, nclass + 1, (H, W))
    return np.where(fg, v, 0).astype(np.uint8)


def _frame(H, W):
    m = np.zeros((H, W), np.uint8)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 2
    return m


def _mask_cases():
    c = {}
    c["1x1"] = (np.array([[3]], np.uint8), FG)
    c["1x7"] = (np.array([[1, 1, 0, 2, 2, 2, 1]], np.uint8), FG)
    c["7x1"] = (np.array([[1, 1, 0, 2, 2, 2, 1]], np.uint8).T.copy(), FG)
    c["zeros"] = (np.zeros((5, 6), np.uint8), FG)
    c["full"] = (np.full((6, 9), 4, np.uint8), FG)
    c["frame"] = (_frame(9, 11), FG)
    c["hole"] = (_nested(1), FG)
    island = _nested(2)
    island[3, 3] = 1
    c["hole_island"] = (island, FG)
    c["nested3"] = (_nested(3), FG)
    c["diag_same"] = (np.array([[1, 0], [0, 1]], np.uint8), FG)
    c["diag_other"] = (np.array([[1, 0], [0, 2]], np.uint8), FG)
    c["diag_anti"] = (np.array([[0, 5, 0], [5, 0, 5], [0, 5, 0]], np.uint8), FG)
    y, x = np.mgrid[:16, :16]
    c["checker16"] = ((1 + (x + y) % 2).astype(np.uint8), FG)
    for H, W in ((33, 65), (70, 130), (64, 32), (65, 33), (129, 31)):
        c[f"stripes{H}x{W}"] = (_stripes(H, W), FG)
    c["stripes130x520"] = (_stripes(130, 520, band=13), FG)       # two tile rows: 1040 column segments
    c["noise0.5_3c_2x1100"] = (_noise(2, 1100, 0.5, 3, 2000), FG)   # one tile row: 1100 column segments
    c["serpentine"] = (_serpentine(64), FG)
    sizes = ((37, 53), (120, 77), (200, 300))        # every density and every class count meets every size once
    for i, density in enumerate((0.1, 0.5, 0.9)):
        for j, nclass in enumerate((1, 3, 8)):
            H, W = sizes[(i + j) % 3]
            c[f"noise{density}_{nclass}c_{H}x{W}"] = (_noise(H, W, density, nclass, 1000 + 3 * i + j), None if nclass == 8 else FG)
    return c


MASKS = _mask_cases()
# object maps given directly (not the labelling of any mask at that connectivity)
RAW = {
    "raw_diag_same": np.array([[1, 0], [0, 1]], np.int32),
    "raw_diag_cross": np.array([[1, 2, 0], [2, 1, 2], [0, 2, 1]], np.int32),
    "raw_sparse_ids": np.array([[7, 7, 0, 3], [0, 7, 3, 3], [9, 0, 0, 3]], np.int32),
}
NAMES = list(MASKS) + list(RAW)
MASK_NAMES = list(MASKS)


@functools.lru_cache(maxsize=None)
def labelled(name, connectivity):
    """(labels int32 [H,W], rows) of a mask case"""
    mask, classes = MASKS[name]
    return cref.label(mask, connectivity, classes)


def object_map(name, connectivity):
    return RAW[name] if name in RAW else labelled(name, connectivity)[0]


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    """the complete restatement of a case: computed once, shared, never modified"""
    full = vref.vectorize(object_map(name, connectivity), connectivity)
    for v in full.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return full


def regimes(full):
    """name -> (max_runs, max_edges, max_rings, max_vertices): roomy (everything fits, with slack behind every total), tight
    (the edge capacity exact, the other arrays cut) and overflow (one edge too few), where the case has an edge to lose"""
    runs, E, R, V = (int(v) for v in full["totals"])
    out = {"roomy": (runs + 3, E + 5, R + 2, V + 3),
           "tight": (max(1, runs // 2), max(1, E), max(1, R - 1), max(1, V // 2))}
    if E > 1:
        out["overflow"] = (runs, E - 1, max(1, R), max(1, V))
    return out


def serpentine_capacities():
    """the three edge capacities of the serpentine: exact, one below, and a non-power-of-two above"""
    E = int(reference("serpentine", 4)["totals"][1])
    return {"exact": E, "below": E - 1, "above": E + 37 if (E + 37) & (E + 36) else E + 39}


def checker_rings(S):
    """(object map, complete result at connectivity 4) of the S x S checkerboard whose foreground pixels (x + y odd) each carry
    an id of their own, 1.. in raster order -- in closed form: every foreground pixel is one ring of its four sides, walked
    top, right, bottom, left from its smallest key, all four corners, twice the area of a unit square.  No labelling produces
    this map and the restatement would walk millions of edges; tests/test_vectors_host.py pins the closed form to it at 8 x 8."""
    y, x = np.mgrid[:S, :S]
    fg = ((x + y) & 1) == 1
    p = np.flatnonzero(fg)
    N = len(p)
    O = np.zeros(S * S, np.int32)
    O[p] = np.arange(1, N + 1, dtype=np.int32)
    O = O.reshape(S, S)
    px, py = (p % S).astype(np.int32), (p // S).astype(np.int32)
    corner = np.stack([np.stack([px + dx, py + dy], axis=1) for dx, dy in zip(vref.SX, vref.SY)], axis=1)      # [N, 4, 2]
    start, robj = vref.run_table(O)
    full = {"size": (S, S), "connectivity": 4, "totals": np.array([len(start), 4 * N, N, 4 * N], np.int32),
            "run_start": start, "run_obj": robj,
            "ring_obj": np.arange(1, N + 1, dtype=np.int32), "ring_head": (4 * p).astype(np.int32),
            "ring_len": np.full(N, 4, np.int32), "ring_area2": np.full(N, 2, np.int64),
            "ring_offset": (4 * np.arange(N + 1)).astype(np.int32), "xy": corner.reshape(-1, 2).astype(np.int32)}
    return O, full
