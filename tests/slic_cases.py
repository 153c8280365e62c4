"""The case table the superpixel tests share: the smallest images at which csrc/slic.hip can still go wrong.
TS is the kernel's tile (SEGK_SLIC_TILE of include/segk.h).  No image is larger than 65 x 129; the restatement's results
are computed once per process and handed out unchanged."""
import functools
import os
import re
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_reference as R                                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def macro(name):
    txt = open(os.path.join(ROOT, "include", "segk.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\w+)", txt).group(1).rstrip("uUlL"), 0)


TS = macro("SEGK_SLIC_TILE")


@dataclass(frozen=True)
class Case:
    name: str
    image: np.ndarray = None                 # uint8 [H,W,C]
    step: int = 8
    compactness: int = 20
    iterations: int = 10
    space: str = "ycc"

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return isinstance(other, Case) and self.name == other.name


# ------------------------------------------------------------------------------------------------ image contents
def constant(H, W, C, value=(90, 160, 30, 7)):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(value[:C], dtype=np.uint8), (H, W, C)))


def checker(H, W, C, cell=3):
    yy, xx = np.mgrid[0:H, 0:W]
    on = ((yy // cell + xx // cell) & 1).astype(np.uint8)
    img = np.stack([on * 255, on * 40 + 20, (1 - on) * 200, on * 9][:C], axis=-1)
    return np.ascontiguousarray(img.astype(np.uint8))


def noise(H, W, C, seed=0, levels=256):
    rng = np.random.default_rng(7919 * H + 104729 * W + 31 * C + seed)
    v = rng.integers(0, levels, size=(H, W, C))
    return (v * (255 // (levels - 1))).astype(np.uint8)


def two_tone(H, W, kind, C=3):
    """(image, true mask): class 1 right of a straight edge at x = 0.4 W + 1, or below the diagonal 2 y > x + 7"""
    yy, xx = np.mgrid[0:H, 0:W]
    one = (xx >= int(0.4 * W) + 1) if kind == "straight" else (2 * yy > xx + 7)
    a, b = np.asarray([30, 60, 200, 255][:C]), np.asarray([220, 190, 40, 255][:C])
    img = np.where(one[..., None], b, a).astype(np.uint8)
    return np.ascontiguousarray(img), one.astype(np.uint8)


def shifted(mask, by=2):
    """the mask moved `by` pixels to the right, its first column repeated"""
    H, W = mask.shape
    return np.ascontiguousarray(mask[:, np.clip(np.arange(W) - by, 0, W - 1)])


def emptied(H=12, W=12):
    """a three-level grey noise image at which, with step 4 and compactness 1, a cluster loses every pixel after the first
    round (found by search over the seeds of `noise`; tests/test_slic_host.py proves it on the restatement)"""
    return noise(H, W, 1, seed=EMPTY_SEED, levels=3)


EMPTY_SEED = 2

TWO_TONE = {kind: two_tone(48, 80, kind) for kind in ("straight", "diagonal")}

CASES = (
    # smaller than one cell: K = 1
    Case("1x1", noise(1, 1, 3), 8),
    Case("1x7", noise(1, 7, 3), 8, 1, 1, "rgb"),
    Case("5x3", noise(5, 3, 3), 8, 255, 10),
    Case("33x40-step64", noise(33, 40, 3), 64, 20, 2),                             # step past both sides
    # tile edges, ragged last cells, 3 W odd: rows that start at every address mod 4
    Case("33x65-noise", noise(33, 65, 3), 4, 1, 10),
    Case("33x65-checker-rgb", checker(33, 65, 3), 8, 255, 1, "rgb"),
    Case("65x129-noise", noise(65, 129, 3, 1), 16, 20, 10),
    Case("65x129-constant", constant(65, 129, 3), 4, 20, 1),                       # every colour distance ties
    Case("65x129-constant-10", constant(65, 129, 3), 6, 255, 10, "rgb"),
    Case("65x129-grey-step5", noise(65, 129, 1, 2), 5, 7, 10),
    Case("65x129-step64", noise(65, 129, 3, 3, levels=4), 64, 1, 10, "rgb"),
    Case("65x129-rgba", noise(65, 129, 4, 4), 7, 40, 3),
    # the tile exactly
    Case("64x64-grey", noise(64, 64, 1, 5, levels=5), 8, 10, 10, "rgb"),
    Case("64x64-rgb", noise(64, 64, 3, 6), 8, 10, 10, "rgb"),
    Case("64x64-rgba-ycc", noise(64, 64, 4, 7), 4, 255, 1, "ycc"),
    # clean edges, and a cluster that ends up empty
    Case("straight", TWO_TONE["straight"][0], 8, 1, 10),
    Case("diagonal", TWO_TONE["diagonal"][0], 8, 1, 10),
    Case("emptied", emptied(), 4, 1, 10, "rgb"),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def expected(case):
    """(labels, centres, counts) of the restatement, read-only"""
    out = R.slic(case.image, case.step, case.compactness, case.iterations, case.space)
    for a in out:
        a.setflags(write=False)
    return out


def grid_k(case):
    ny, nx = R.grid_of(case.image.shape[0], case.image.shape[1], case.step)
    return ny * nx


# ------------------------------------------------------------------------------------------------ vote and snap
@dataclass(frozen=True)
class SnapCase:
    name: str
    labels: np.ndarray = None                # int32 [H,W]
    k: int = 1
    mask: np.ndarray = None                  # uint8 [H,W]
    weights: Optional[np.ndarray] = None     # uint8 [H,W]
    classes: Tuple[int, ...] = tuple(range(8))
    fill: Tuple[int, ...] = ()
    min_share: int = 128                     # of 256

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return isinstance(other, SnapCase) and self.name == other.name


def _class_noise(H, W, C, seed):
    rng = np.random.default_rng(15485863 * H + 32452843 * W + seed)
    coarse = rng.integers(0, C, size=(H // 5 + 1, W // 5 + 1), dtype=np.uint8)
    m = np.kron(coarse, np.ones((5, 5), dtype=np.uint8))[:H, :W]
    hit = rng.random((H, W)) < 0.05
    m[hit] = rng.integers(0, C, size=(H, W), dtype=np.uint8)[hit]
    return np.ascontiguousarray(m)


def _weights(H, W, seed):
    rng = np.random.default_rng(49979687 * H + 67867967 * W + seed)
    w = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    w[rng.random((H, W)) < 0.3] = 0                                                # zeros: pixels that do not vote
    return w


def _blocks(H, W, side):
    """a segmentation that is no SLIC result: square blocks numbered along the rows"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy // side * (-(-W // side)) + xx // side).astype(np.int32), (-(-H // side)) * (-(-W // side))


def _snap_cases():
    out = []
    # on SLIC's own labels
    c = BY_NAME["65x129-noise"]
    lab, K = np.array(expected(c)[0]), grid_k(c)
    H, W = lab.shape
    m = _class_noise(H, W, 4, 0)
    for share in (0, 128, 256):
        out.append(SnapCase(f"slic-share{share}", lab, K, m, None, min_share=share))
    out.append(SnapCase("slic-weighted", lab, K, m, _weights(H, W, 1), min_share=154))
    # a void band that is filled, never votes; a class outside `classes` neither votes nor changes
    band = m.copy()
    band[(np.roll(m, 1, 0) != m) | (np.roll(m, 1, 1) != m)] = 255
    out.append(SnapCase("slic-void-band", lab, K, band, _weights(H, W, 2), classes=(0, 1, 2), fill=(255,), min_share=128))
    out.append(SnapCase("slic-void-band-nofill", lab, K, band, None, classes=(0, 1, 3), min_share=100))
    # labels outside [0, K), among them the smallest and largest int32
    c = BY_NAME["33x65-noise"]
    lab, K = np.array(expected(c)[0]), grid_k(c)
    H, W = lab.shape
    wild = lab.copy()
    wild[3:9, 10:30] = -1
    wild[20:22, :] = K
    wild[0, 0], wild[0, 1], wild[32, 64] = np.iinfo(np.int32).min, np.iinfo(np.int32).max, K + 5
    out.append(SnapCase("labels-outside", wild, K, _class_noise(H, W, 8, 3), _weights(H, W, 3), min_share=64))
    # another segmentation, a tile edge inside a block, a table larger than the image needs
    lab, K = _blocks(65, 129, 9)
    out.append(SnapCase("blocks", lab, K + 100, _class_noise(65, 129, 8, 4), None, fill=(), min_share=140))
    # one pixel per segment: more keys in a tile than the LDS table holds
    lab = np.arange(64 * 64, dtype=np.int32).reshape(64, 64)
    out.append(SnapCase("pixel-segments", lab, 64 * 64, _class_noise(64, 64, 8, 5), _weights(64, 64, 5), min_share=256))
    # the share test with equality: two segments, each half class 2 and half class 5; 256 * 8 = 128 * 16
    lab = np.zeros((4, 8), dtype=np.int32)
    lab[2:] = 1
    m = np.where(np.arange(8) % 2 == 0, 5, 2).astype(np.uint8) * np.ones((4, 1), dtype=np.uint8)
    out.append(SnapCase("share-equal", lab, 2, np.ascontiguousarray(m), None, min_share=128))
    out.append(SnapCase("share-just-missed", lab, 2, np.ascontiguousarray(m), None, min_share=129))
    out.append(SnapCase("1x1", np.zeros((1, 1), dtype=np.int32), 1, np.full((1, 1), 7, dtype=np.uint8), None))
    return tuple(out)


SNAP_CASES = _snap_cases()
SNAP_BY_NAME = {c.name: c for c in SNAP_CASES}
assert len(SNAP_BY_NAME) == len(SNAP_CASES)


@functools.lru_cache(maxsize=None)
def snap_expected(case):
    """(out, hist, winner) of the restatement, read-only"""
    out = R.snap(case.labels, case.mask, case.k, case.weights, case.classes, case.fill, case.min_share)
    for a in out:
        a.setflags(write=False)
    return out
