"""NumPy / plain-Python restatement of DESIGN.md 3.17 (mask vectorisation: run table, boundary edges, successor rule, rings,
corner vertices, capacities), shared by tests/test_vectors_host.py and tests/test_gpu_vectors.py.  Written from the
definition: the edges are a set of keys, the successor is looked up in that set from the vertex and the direction vectors,
and every ring is walked edge by edge.  Nothing here is imported by the package."""
import numpy as np

DX = (1, 0, -1, 0)          # direction of side 0..3: E, S, W, N (y grows downwards)
DY = (0, 1, 0, -1)
# start vertex of side s of pixel (x, y), as an offset
SX = (0, 1, 1, 0)
SY = (0, 0, 1, 1)


def run_table(O):
    """(run_start, run_obj) of the column-major reading t = x*H + y"""
    cm = np.ascontiguousarray(O.T).reshape(-1)
    flag = np.ones(cm.shape, bool)
    flag[1:] = cm[1:] != cm[:-1]
    start = np.flatnonzero(flag)
    return start.astype(np.int32), cm[start].astype(np.int32)


def rebuild_from_runs(start, obj, H, W):
    length = np.diff(np.append(start.astype(np.int64), H * W))
    return np.repeat(obj, length).reshape(W, H).T


def edge_keys(O):
    """sorted keys 4*(y*W + x) + side of every boundary edge"""
    H, W = O.shape
    P = np.zeros((H + 2, W + 2), O.dtype)
    P[1:-1, 1:-1] = O
    nb = (P[:-2, 1:-1], P[1:-1, 2:], P[2:, 1:-1], P[1:-1, :-2])          # top, right, bottom, left neighbour
    lin = np.arange(H * W, dtype=np.int64).reshape(H, W)
    keys = [4 * lin[(O != 0) & (nb[s] != O)] + s for s in range(4)]
    return np.sort(np.concatenate(keys))


def successor(O, edges, key, connectivity):
    """the key of the edge that follows `key` (edges: the set of all keys)"""
    H, W = O.shape
    p, d = key >> 2, key & 3
    y, x = divmod(p, W)
    k = O[y, x]
    vx, vy = x + SX[d] + DX[d], y + SY[d] + DY[d]                        # end vertex
    turns = ((d + 1) % 4, d, (d + 3) % 4) if connectivity == 4 else ((d + 3) % 4, d, (d + 1) % 4)
    for nd in turns:
        # the pixel on the right of the unit step from (vx, vy) in direction nd
        px = (2 * vx + DX[nd] - DY[nd] - 1) // 2
        py = (2 * vy + DY[nd] + DX[nd] - 1) // 2
        if 0 <= px < W and 0 <= py < H and O[py, px] == k and 4 * (py * W + px) + nd in edges:
            return 4 * (py * W + px) + nd
    raise AssertionError("an edge without a successor")


def vectorize(O, connectivity=4):
    """The complete result of DESIGN.md 3.17 for the object map O (int [H,W]) as a dict of NumPy arrays."""
    O = np.asarray(O)
    H, W = O.shape
    start, robj = run_table(O)
    keys = edge_keys(O)
    edges = set(int(k) for k in keys)
    seen = set()
    ring_obj, ring_head, ring_len, ring_area2, ring_offset, xy = [], [], [], [], [0], []
    for head in (int(k) for k in keys):                                  # ascending: the first unseen key heads its ring
        if head in seen:
            continue
        walk, key = [], head
        while True:
            seen.add(key)
            walk.append(key)
            key = successor(O, edges, key, connectivity)
            if key == head:
                break
            assert key not in seen
        area2, corners = 0, []
        for i, key in enumerate(walk):
            p, d = key >> 2, key & 3
            y, x = divmod(p, W)
            x0, y0 = x + SX[d], y + SY[d]
            x1, y1 = x0 + DX[d], y0 + DY[d]
            area2 += x0 * y1 - x1 * y0
            if (walk[i - 1] & 3) != d:
                corners.append((x0, y0))
        assert len(corners) >= 4
        ring_obj.append(int(O.reshape(-1)[head >> 2])); ring_head.append(head); ring_len.append(len(walk)); ring_area2.append(area2)
        xy.extend(corners)
        ring_offset.append(len(xy))
    assert len(seen) == len(edges)
    return {
        "size": (H, W), "connectivity": connectivity,
        "totals": np.array([len(start), len(keys), len(ring_obj), len(xy)], np.int32),
        "run_start": start, "run_obj": robj,
        "ring_obj": np.array(ring_obj, np.int32), "ring_head": np.array(ring_head, np.int32),
        "ring_len": np.array(ring_len, np.int32), "ring_area2": np.array(ring_area2, np.int64),
        "ring_offset": np.array(ring_offset, np.int32), "xy": np.array(xy, np.int32).reshape(-1, 2),
    }


RING_ARRAYS = ("ring_obj", "ring_head", "ring_len", "ring_area2", "ring_offset", "xy")


def truncate(full, max_runs, max_edges, max_rings, max_vertices):
    """What the capacities leave of a complete result: totals stay true; every array keeps the prefix that fits; with more edges
    than max_edges the ring and vertex totals are -1 and the ring arrays hold nothing (the device leaves them untouched)."""
    out = dict(full)
    out["totals"] = full["totals"].copy()
    out["run_start"], out["run_obj"] = full["run_start"][:max_runs], full["run_obj"][:max_runs]
    if full["totals"][1] > max_edges:
        out["totals"][2:] = -1
        for n in RING_ARRAYS:
            out[n] = full[n][:0]
        return out
    for n in ("ring_obj", "ring_head", "ring_len", "ring_area2"):
        out[n] = full[n][:max_rings]
    out["ring_offset"] = full["ring_offset"][:max_rings + 1]
    out["xy"] = full["xy"][:max_vertices]
    return out


def fill_even_odd(polys, H, W):
    """even-odd scanline fill of rings given as vertex arrays [n,2] (x, y): the pixel (y, x) is inside when an odd number of
    vertical ring segments lies at or left of its left side -- independent of the walk's direction"""
    acc = np.zeros((H, W + 1), np.int64)
    for v in polys:
        n = len(v)
        for i in range(n):
            (xa, ya), (xb, yb) = v[i], v[(i + 1) % n]
            if xa == xb:
                acc[min(ya, yb):max(ya, yb), xa] += 1
            else:
                assert ya == yb
    return (np.cumsum(acc, axis=1)[:, :W] & 1).astype(bool)


def rle_decode(rle):
    H, W = rle["size"]
    bits = np.repeat(np.arange(len(rle["counts"])) & 1, rle["counts"])
    return bits.reshape(W, H).T.astype(bool)
