"""Case tables of the eval resize / crop / fused-mask matrix (the second half of csrc/resize.hip: segk_resize_pad[_flip],
segk_resize_pad_u8[_flip], segk_crop_resize, segk_predict_mask).  Host-only: namedtuples, ids, the restated launch arithmetic
and the memory a case needs.  tests/test_resize_cases_host.py proves the tables reach every regime; tests/resize_reference.py
holds the references.

A forward case resizes an (H, W) image to (nh, nw) and writes it at (pt, pl) into a [C, T, T] slot; a reverse case crops the
(nh, nw) window at (pt, pl) out of a slot of pitch T and resizes it to (oh, ow).  The shapes are the smallest at which each
hazard exists: side-1 images and windows, up-scaling on one axis and down-scaling on the other, windows strictly inside the
slot or flush with its far edge, tap counts from 1 to 500, threads of predict_mask that span two to four rows."""
from collections import namedtuple

FwdCase = namedtuple("FwdCase", "regime H W nh nw T pt pl")
RevCase = namedtuple("RevCase", "regime T pt pl nh nw oh ow")
WrapCase = namedtuple("WrapCase", "entry C H W nh nw T pt pl modes")

GRID_CAP = 16384                  # blocks of 256 threads: resize_pad, resize_pad_u8, crop_resize, predict_mask without counts
MEM_BUDGET = 256 << 20            # device bytes one GPU case may hold (inputs, outputs, guards)
REF_BUDGET = 64 << 20             # elements-times-taps a NumPy reference of one case may touch

MODES = (0, 1, 2)                 # 0 anti-aliased, 1 nearest, 2 two-tap bilinear
CHANNELS = (1, 3)
DESIGNS = ("dense01", "signed", "constant", "ramp")
FLIPS = (0, 1, 2, 3)
U8_CHANNELS = (1, 3, 4)
REV_CLASSES = (1, 2, 3, 4, 5, 8)
LABEL_VALUES = (-1, 0, 3, 255, 2 ** 31, 2 ** 40 + 1, -(2 ** 63))

FWD_CASES = [
    FwdCase("identity", 16, 16, 16, 16, 16, 0, 0),
    FwdCase("side1", 1, 1, 1, 1, 4, 3, 3),                  # flush with the far corner
    FwdCase("side1", 1, 7, 1, 5, 8, 7, 3),                  # flush with both far edges
    FwdCase("side1", 7, 1, 16, 1, 16, 0, 15),
    FwdCase("side1", 1, 300, 1, 64, 64, 31, 0),
    FwdCase("side1", 500, 375, 1, 1, 4, 1, 2),              # 500 and 375 taps
    FwdCase("anisotropic", 97, 1200, 3, 37, 40, 37, 3),     # ratios 32.3 and 32.4, flush with both far edges
    FwdCase("anisotropic", 5, 40, 64, 8, 64, 0, 28),        # up on y, down on x
    FwdCase("anisotropic", 2, 3, 64, 64, 64, 0, 0),
    FwdCase("near-identity", 33, 65, 32, 63, 64, 16, 0),
    FwdCase("near-identity", 13, 17, 12, 16, 16, 2, 0),
    FwdCase("ratio31", 2000, 3, 64, 2, 64, 0, 31),
    FwdCase("inside", 37, 53, 24, 32, 48, 5, 11),           # off-centre, strictly inside on both axes
    FwdCase("pad00", 37, 53, 24, 32, 48, 0, 0),
    FwdCase("control", 375, 500, 48, 64, 64, 8, 0),         # what process_batch_forward builds: aspect kept, centred
]
FLIP_CASES = [c for c in FWD_CASES if (c.regime, c.H) in (("inside", 37), ("anisotropic", 5))]
U8_CASES = [c for c in FWD_CASES if (c.H, c.W, c.pt) in ((13, 17, 2), (37, 53, 5), (5, 40, 0), (1, 7, 7), (2000, 3, 0), (7, 1, 0))]
I64_CASES = [c for c in FWD_CASES if (c.H, c.W, c.pt) in ((37, 53, 5), (7, 1, 0), (97, 1200, 37))]

REV_CASES = [
    RevCase("identity", 16, 0, 0, 16, 16, 16, 16),
    RevCase("side1", 4, 3, 3, 1, 1, 1, 1),                  # oh ow = 1
    RevCase("side1", 8, 7, 3, 1, 5, 1, 7),                  # oh = 1, oh ow = 7
    RevCase("side1", 8, 7, 3, 1, 5, 1, 3),                  # oh ow = 3
    RevCase("side1", 16, 0, 15, 16, 1, 7, 1),               # nw = 1, ow = 1: a thread spans four rows
    RevCase("side1", 64, 31, 0, 1, 64, 1, 300),             # nh = 1
    RevCase("side1", 4, 1, 2, 1, 1, 500, 375),
    RevCase("anisotropic", 40, 37, 3, 3, 37, 97, 1200),
    RevCase("anisotropic", 64, 0, 28, 64, 8, 5, 40),
    RevCase("anisotropic", 64, 0, 0, 64, 64, 2, 3),         # down 32 and 21.3 without anti-aliasing, oh ow = 6
    RevCase("anisotropic", 64, 0, 0, 64, 64, 3, 2),         # ow = 2
    RevCase("near-identity", 64, 16, 0, 32, 63, 33, 65),
    RevCase("near-identity", 16, 2, 0, 12, 16, 13, 17),
    RevCase("ratio31", 64, 0, 31, 64, 2, 2000, 3),          # ow = 3
    RevCase("inside", 48, 5, 11, 24, 32, 37, 53),
    RevCase("inside", 48, 5, 11, 24, 32, 9, 5),             # ow = 5, oh ow % 4 = 1
    RevCase("pad00", 48, 0, 0, 24, 32, 37, 53),
    RevCase("control", 64, 8, 0, 48, 64, 375, 500),
]
STRADDLE_CASE = RevCase("straddle", 16, 2, 5, 8, 3, 8, 3)   # identity geometry with ow = 3: pixel (y, x) reads slot (2 + y, 5 + x)

WRAP_CASES = [
    WrapCase("resize_pad", 5, 8, 8, 1000, 1019, 1024, 24, 5, (1, 2)),
    WrapCase("resize_pad_i64", 5, 8, 8, 1000, 1019, 1024, 24, 5, (1,)),
    WrapCase("resize_pad_u8", 3, 8, 8, 2064, 2001, 2064, 0, 63, (1, 2)),
]
WRAP_PREDICT = RevCase("wrap", 16, 3, 1, 12, 14, 4100, 4100)
WRAP_PREDICT_C = 2


def fwd_id(c):
    return f"{c.regime}-{c.H}x{c.W}-to-{c.nh}x{c.nw}-T{c.T}-pad{c.pt}.{c.pl}"


def rev_id(c):
    return f"{c.regime}-T{c.T}-pad{c.pt}.{c.pl}-{c.nh}x{c.nw}-to-{c.oh}x{c.ow}"


def wrap_id(c):
    return f"{c.entry}-C{c.C}-T{c.T}"


def window_ok(c):
    """the SEGK_REQUIRE every entry makes of its window"""
    return c.pt >= 0 and c.pl >= 0 and c.pt + c.nh <= c.T and c.pl + c.nw <= c.T


def flush_far(c):
    return c.pt + c.nh == c.T or c.pl + c.nw == c.T


def _trips(items, cap=GRID_CAP):
    blocks = (items + 255) // 256
    return (blocks + cap - 1) // cap


def resize_pad_trips(C, T):
    return _trips(C * T * T)


def resize_pad_u8_trips(T):
    return _trips(T * T)


def crop_resize_trips(C, oh, ow):
    return _trips(C * oh * ow)


def predict_mask_trips(oh, ow):
    """without counts and labels (with either the grid is persistent: three blocks per CU, many trips at any large size)"""
    return _trips((oh * ow + 3) // 4)


def rows_of_a_thread(c):
    """the set of row counts the four flat pixels of one predict_mask thread touch, over the threads of the case"""
    total = c.oh * c.ow
    return {min(p + 3, total - 1) // c.ow - p // c.ow + 1 for p in range(0, min(total, 4 * c.ow + 4), 4)}


def taps(n_in, n_out):
    """about how many taps per output the anti-aliased filter reads along one axis"""
    return 2 * max(n_in / n_out, 1.0) + 1


def fwd_bytes(c, C, elem_bytes=4, in_bytes=None):
    return C * c.H * c.W * (elem_bytes if in_bytes is None else in_bytes) + C * c.T * c.T * elem_bytes + 4096 * elem_bytes


def rev_bytes(c, C):
    total = c.oh * c.ow
    return C * c.T * c.T * 4 + C * total * 4 + total * (1 + 3 + 8) + 3 * 4096 * 4


def fwd_ref_cost(c, C=3):
    return int(C * (c.H * c.nw * taps(c.W, c.nw) + c.nh * c.nw * taps(c.H, c.nh)))
