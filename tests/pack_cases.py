"""Case tables of the pack / layout / gradient-reduce matrix (tests/test_gpu_pack_matrix.py runs them on the GPU,
tests/test_pack_cases_host.py proves on the CPU that every branch named below is reached): the smallest shapes that reach
each branch of csrc/pack.hip, and a Python restatement of its launch arithmetic.  Plain Python, no torch.

  grid cap       the element-wise kernels launch ceil(total / 256) blocks of 256 threads, at most 16384: beyond
                 16384 * 256 items the grid-stride loop takes a second trip.
  `both` kernel  a block owns a 32 (output channels) x 32 (padded input channels) x 9 tile and loads it with float4 when
                 (inside) the 32 padded channels are 32 consecutive logical channels of one source, (cout) the 32 output
                 channels exist, (cin4) Cin % 4 == 0 and (ci4) the first logical channel is a multiple of 4.
  pack_multi     a block finds its tensor by its first block; kinds 1 and 3 take chunks of segk_pack_convt_chunk() elements.
  reduce         S <= 16: one block per output row, eight slabs in flight with a clamped slab index; S > 16: 16 vectors x
                 16 slab lanes per block, eight slabs of a lane in flight (a second trip from S > 128), ceil(nvec / 16) blocks
                 per row; column sums: one block per 8 columns, 32 row lanes with 8 rows in flight (a second trip from
                 rows > 256)."""
from collections import namedtuple

GRID_CAP = 16384
THREADS = 256
CHUNK = 2048                    # segk_pack_convt_chunk(): the GPU test checks the query against it
CH = {"fp32": 16, "bf16": 32}
VEC = {"fp32": 4, "bf16": 8}    # elements of a 16-byte vector
DTYPES = ("fp32", "bf16")


def pad32(c):
    return (c + 31) // 32 * 32


def cdiv(a, b):
    return -(-a // b)


# ---- Conv2d weights --------------------------------------------------------------------------------------------------------
ConvPack = namedtuple("ConvPack", "Cout CA CB Coutp CAp CBp taps mode dtype")
CONV_SHAPES = [(1, 1, 0), (64, 3, 0), (33, 31, 0), (32, 32, 0), (70, 40, 0), (32, 20, 50), (96, 36, 60), (64, 34, 62),
               (128, 64, 64)]
OVER_PADDED = (33, 31, 0, 96, 64, 0)                # Coutp = pad32 + 32, CAp = pad32 + 32
GRANULE16 = [(20, 10, 0, 32, 16, 0), (40, 40, 12, 64, 48, 16)]     # fp32: CAp, CBp multiples of 16
# past the grid cap, Kp = 704 and Np = 672 in both modes (mode 0: K = input channels; mode 1: K = output channels)
PAST_CAP = [ConvPack(650, 330, 340, 672, 352, 352, 9, 0, "bf16"), ConvPack(690, 300, 350, 704, 320, 352, 9, 1, "bf16")]


def _geometry(Cout, CA, CB):
    return (Cout, CA, CB, pad32(Cout), pad32(CA), pad32(CB) if CB else 0)


def _conv_cases():
    out = []
    for shape in CONV_SHAPES:
        for taps in (9, 1):
            if taps == 1 and shape[2]:
                continue                             # the 1x1 layers have one source
            out += [ConvPack(*_geometry(*shape), taps, mode, dt) for mode in (0, 1) for dt in DTYPES]
    out += [ConvPack(*OVER_PADDED, 9, mode, dt) for mode in (0, 1) for dt in DTYPES]
    for g in GRANULE16:
        out += [ConvPack(*g, taps, mode, "fp32") for taps in ((9, 1) if g[2] == 0 else (9,)) for mode in (0, 1)]
    return out + PAST_CAP


CONV_CASES = _conv_cases()


def conv_kn(c):
    """(Kp, Np) of the packed operand"""
    return (c.CAp + c.CBp, c.Coutp) if c.mode == 0 else (c.Coutp, c.CAp + c.CBp)


def conv_total(c):
    Kp, Np = conv_kn(c)
    return Kp * c.taps * Np


def grid_trips(total):
    """trips of the grid-stride loop of the element-wise kernels for the busiest thread"""
    return cdiv(total, min(cdiv(total, THREADS), GRID_CAP) * THREADS)


def conv_case_id(c):
    return f"{c.dtype}-{c.Cout}x{c.CA}+{c.CB}-p{c.Coutp}x{c.CAp}+{c.CBp}-t{c.taps}-m{c.mode}"


# ---- the one-pass forward + data-gradient pack -----------------------------------------------------------------------------
BothCase = namedtuple("BothCase", "Cout CA CB Coutp CAp CBp dtype dgrad")
BOTH_GEOMETRIES = [_geometry(*s) for s in CONV_SHAPES] + [OVER_PADDED]
BOTH_CASES = [BothCase(*g, dt, dgrad) for g in BOTH_GEOMETRIES for dt in DTYPES for dgrad in (True, False)]


def both_case_id(c):
    return f"{c.dtype}-{c.Cout}x{c.CA}+{c.CB}-p{c.Coutp}x{c.CAp}+{c.CBp}-{'both' if c.dgrad else 'fwd'}"


def dual_logical(kp, CA, CAp, CB):
    """logical input channel at padded place kp, or -1 for padding"""
    if kp < CAp:
        return kp if kp < CA else -1
    return CA + kp - CAp if kp - CAp < CB else -1


def both_tiles(g):
    """every 32 x 32 x 9 tile of a geometry -> (source 'A' | 'B', {predicate: holds}) ; the float4 path needs all four"""
    Cout, CA, CB, Coutp, CAp, CBp = g
    out = []
    for kp0 in range(0, CAp + CBp, 32):
        ci0, ci31 = dual_logical(kp0, CA, CAp, CB), dual_logical(kp0 + 31, CA, CAp, CB)
        for co0 in range(0, Coutp, 32):
            out.append(("A" if kp0 < CAp else "B",
                        {"inside": ci0 >= 0 and ci31 == ci0 + 31, "cout": co0 + 32 <= Cout, "cin4": (CA + CB) % 4 == 0,
                         "ci4": ci0 >= 0 and ci0 % 4 == 0}))
    return out


# ---- ConvTranspose2d weights -----------------------------------------------------------------------------------------------
ConvtPack = namedtuple("ConvtPack", "Cin Cout mode dtype")
CONVT_SHAPES = [(1, 1), (32, 32), (40, 70), (128, 64), (96, 33)]
CONVT_CASES = [ConvtPack(*s, mode, dt) for s in CONVT_SHAPES for mode in (0, 1) for dt in DTYPES]


# ---- segk_pack_multi tables ------------------------------------------------------------------------------------------------
# kind 0: 3x3 weight [Cout][d0 + d1][3][3]; kind 1: ConvTranspose weight [d0][Cout][2][2]; kind 2: bias [Cout], d0 = reps;
# kind 3: 1x1 weight [Cout][d0].  dgrad: the entry has a data-gradient destination (never for a bias)
Entry = namedtuple("Entry", "kind Cout d0 d1 dgrad")
K3_SMALL, K3_EXACT, K3_REMAINDER = Entry(3, 5, 20, 0, True), Entry(3, 33, 31, 0, False), Entry(3, 70, 30, 0, True)


def entry_elements(e):
    """elements of each destination of an entry"""
    Coutp = pad32(e.Cout)
    if e.kind == 0:
        return (pad32(e.d0) + (pad32(e.d1) if e.d1 else 0)) * 9 * Coutp
    if e.kind == 2:
        return (e.d0 if e.d0 > 0 else 4) * Coutp
    return pad32(e.d0) * (4 if e.kind == 1 else 1) * Coutp


def entry_blocks(e):
    Coutp = pad32(e.Cout)
    if e.kind == 0:
        return (pad32(e.d0) + (pad32(e.d1) if e.d1 else 0)) // 32 * (Coutp // 32)
    return 1 if e.kind == 2 else cdiv(entry_elements(e), CHUNK)


def _small(i):
    """64 small entries, the kinds cycling, the shapes moving with i"""
    return [Entry(0, 3 + i % 40, 1 + i % 9, (i % 3) * 5, i % 8 != 0), Entry(1, 1 + i % 33, 1 + i % 5, 0, i % 8 != 1),
            Entry(2, 1 + i % 70, (0, 1, 3)[i // 4 % 3], 0, False), Entry(3, 1 + i % 50, 1 + i % 64, 0, i % 8 == 3)][i % 4]


MULTI_TABLES = {
    "one-conv3x3": [Entry(0, 70, 40, 0, True)],
    "one-convt": [Entry(1, 33, 40, 0, True)],
    "one-bias": [Entry(2, 33, 0, 0, False)],
    "one-conv1x1": [K3_REMAINDER],
    "two": [Entry(0, 32, 20, 50, False), Entry(1, 70, 40, 0, False)],
    "nine-interleaved": [Entry(2, 70, 1, 0, False), Entry(0, 96, 36, 60, True), K3_SMALL, Entry(1, 64, 128, 0, True),
                         Entry(0, 64, 34, 62, False), Entry(2, 5, 3, 0, False), K3_EXACT, Entry(1, 1, 1, 0, False),
                         Entry(2, 64, 0, 0, False)],
    "sixty-four": [_small(i) for i in range(64)],
}


# ---- gradient reductions ---------------------------------------------------------------------------------------------------
ReduceShape = namedtuple("ReduceShape", "N CA CB taps Np CAp CBp")


def _reduce_shape(N, CA, CB, taps):
    return ReduceShape(N, CA, CB, taps, pad32(N), pad32(CA), pad32(CB) if CB else 0)


REDUCE_SHAPES = [_reduce_shape(1, 1, 0, 1), ReduceShape(64, 27, 0, 1, 64, 32, 0), _reduce_shape(33, 31, 0, 9),
                 _reduce_shape(64, 40, 72, 9), _reduce_shape(64, 64, 0, 4), _reduce_shape(5, 36, 60, 9),
                 _reduce_shape(2, 32, 0, 1)]
ROW_S = [1, 2, 7, 8, 9, 15, 16]
WIDE_S = [17, 31, 32, 33, 127, 128, 129, 145, 300, 512]
LATTICE_S = ROW_S + WIDE_S
RANDOM_S = [8, 16, 17, 129, 512]
LATTICE_MAX = 8                 # slab elements are integers in [-8, 8]
SENTINEL = float(2 ** 20)       # what padded columns and rows n >= N hold: a leak is a wrong number at a known place
BIG_ROW = _reduce_shape(2, 1376, 0, 9)              # 1376 * 9 * 4 = 49536 bytes of LDS: above 48 KiB, below 64 KiB
BIG_ROW_S = 2


def reduce_form(S):
    return "row" if S <= 16 else "wide"


def reduce_nvec(r):
    return r.taps * (r.CAp + r.CBp) // 4


def wide_trips(S):
    """trips of a slab lane's loop in the wide form (the busiest lane, sl = 0)"""
    return cdiv(S, 128)


def reduce_shape_id(r):
    return f"{r.N}x{r.CA}+{r.CB}x{r.taps}-p{r.Np}x{r.CAp}+{r.CBp}"


# column sums of [rows][Ctot][2] partials
COLSUM_ROWS = [1, 31, 32, 33, 255, 256, 257, 300, 513]
COLSUM_NCOLS = [1, 7, 8, 9, 100]
ColsumCase = namedtuple("ColsumCase", "rows ncols col0 Ctot")
COLSUM_CASES = [ColsumCase(rows, ncols, (0 if (i + j) % 2 == 0 else 5 + j), (0 if (i + j) % 2 == 0 else 5 + j) + ncols + 3)
                for i, rows in enumerate(COLSUM_ROWS) for j, ncols in enumerate(COLSUM_NCOLS)]

# job lists of segk_wgrad_reduce_multi: "W" a wide job, "R" a row job, "C" column sums; n = 1 .. 4, each kind first, in the
# middle and last
JOB_ORDERS = ["W", "R", "C", "WR", "CW", "RC", "WRC", "RCW", "CWR", "RWCR", "CRWC", "WCRW"]


def job_spec(kind, slot):
    """the reduction behind letter `kind` at place `slot` of a job list: (shape index into REDUCE_SHAPES, S) or a ColsumCase"""
    if kind == "W":
        return ((3, 33), (5, 129), (2, 17), (4, 145))[slot]
    if kind == "R":
        return ((2, 7), (3, 16), (5, 9), (1, 15))[slot]
    return COLSUM_CASES[(7, 23, 38, 44)[slot]]


# ---- layout ----------------------------------------------------------------------------------------------------------------
LayoutCase = namedtuple("LayoutCase", "B C H W Cp dtype")
LAYOUT_SHAPES = [(1, 1, 1, 1, 32), (2, 3, 5, 7, 32), (2, 3, 5, 7, 64), (1, 31, 4, 3, 32), (1, 33, 3, 5, 64), (2, 70, 9, 3, 96)]
LAYOUT_CASES = [LayoutCase(*s, dt) for s in LAYOUT_SHAPES for dt in DTYPES] + \
               [LayoutCase(1, 1, 725, 725, 32, "fp32")] + [LayoutCase(1, 9, 683, 683, 32, dt) for dt in DTYPES]


def to_nhwc_items(c):
    """items of nchw_to_nhwc's loop: one 16-byte channel vector of one pixel"""
    return c.B * c.H * c.W * (c.Cp // VEC[c.dtype])


def to_nchw_items(c):
    return c.B * c.C * c.H * c.W


def layout_case_id(c):
    return f"{c.dtype}-{c.B}x{c.C}x{c.H}x{c.W}-p{c.Cp}"


# ---- repack_stale ----------------------------------------------------------------------------------------------------------
REPACK_WEIGHTS = [(3 + i % 37, 1 + i % 11, (i % 4) * 3) for i in range(70)]       # (Cout, CA, CB) of 70 small 3x3 weights
