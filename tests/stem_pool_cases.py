"""Case tables of the stem / pooling / BN-statistics matrix (tests/test_gpu_stem_pool_matrix.py runs them on the GPU,
tests/test_stem_pool_cases_host.py proves on the CPU that every regime named below is populated) and a Python restatement
of the launch arithmetic of csrc/stem.hip and of the pooling entries of csrc/bn_pool.hip, evaluated for NUM_CUS compute
units exactly as conv_cases.py does.  Plain Python, no torch.

The stem (bf16 only, Cin 1..3, W % 16 == 0) streams 16-pixel blocks, nblk = B * H * (W / 16) of them; wave `first` of the
grid owns the blocks first, first + step, first + 2 step, ... with step = 8 * workgroups.  stem_stream_kernel fetches two
of them per pass (blk, blk + step) and multiplies the second only where it exists; stem_wgrad_kernel takes one per trip.
The pooling kernels walk items (2x2 window x 16-byte channel vector) with a grid-stride loop behind a capped grid."""
from collections import namedtuple

NUM_CUS = 256                   # MI355X: the launch arithmetic below is evaluated for it
STEM_WAVES = 8                  # waves per workgroup of both stem kernels
STEM_WG_PER_CU = 2
STEM_S = STEM_WAVES * NUM_CUS * STEM_WG_PER_CU     # 4096: the block stride of a full grid
REF_MADD_CAP = 6 * 10 ** 8      # float64 reference on the CPU: multiply-adds (stem) or elements (pooling) per case
POOL_GRID_CAP = 8192            # maxpool_fwd, maxpool_bwd, bn_relu_apply_pool
STAT_GRID_CAP = 1024            # maxpool_bwd with the BatchNorm reductions (one partial row per block)


def cdiv(a, b):
    return -(-a // b)


# ---- the stem --------------------------------------------------------------------------------------------------------------
StemCase = namedtuple("StemCase", "B Cin H W")


def stem_served(c, Cout=64, dtype="bf16"):
    if dtype != "bf16" or c.B <= 0 or c.H <= 0 or c.W <= 0 or c.W % 16 != 0 or c.Cin < 1 or c.Cin > 3 or Cout != 64:
        return False
    return c.B * c.H * c.W * 64 < 2147483647 * 16 and c.B * c.Cin * c.H * c.W < 2147483647


def stem_nblk(c):
    return c.B * c.H * (c.W // 16)


def stem_rows(c, Cout=64, dtype="bf16"):
    """segk_stem_rows: workgroups (= rows of BatchNorm partials) of stem_stream_kernel, 0 where it does not apply"""
    if not stem_served(c, Cout, dtype):
        return 0
    return min(cdiv(stem_nblk(c), STEM_WAVES), NUM_CUS * STEM_WG_PER_CU, 1024)


def stem_wgrad_slabs(c, Cout=64, dtype="bf16"):
    """segk_stem_wgrad_slabs: workgroups (= slabs [64][32]) of stem_wgrad_kernel"""
    if not stem_served(c, Cout, dtype):
        return 0
    return min(cdiv(stem_nblk(c), STEM_WAVES), NUM_CUS * 2)


def stem_step(c):
    return STEM_WAVES * stem_rows(c)


def stem_wgrad_step(c):
    return STEM_WAVES * stem_wgrad_slabs(c)


def stem_passes(c, first):
    """The passes of stem_stream_kernel's loop for the wave whose first block is `first`: a list of `two` flags (True: the
    pass multiplies blk and blk + step, False: blk alone)."""
    nb, step, out, blk = stem_nblk(c), stem_step(c), [], first
    while blk < nb:
        out.append(blk + step < nb)
        blk += 2 * step
    return out


def stem_pass_patterns(c):
    """{pattern of `two` flags: number of waves of the grid with it}; idle waves have the empty pattern ()"""
    pats = {}
    for f in range(stem_step(c)):
        p = tuple(stem_passes(c, f))
        pats[p] = pats.get(p, 0) + 1
    return pats


def stem_blocks_per_wave(c):
    """most blocks one wave (= one lane's register chain of the statistics) consumes"""
    return cdiv(stem_nblk(c), stem_step(c))


def stem_regime(c):
    nb, S = stem_nblk(c), STEM_S
    if nb <= S:
        return "single"
    if nb < 2 * S:
        return "mixed-pair"
    if nb == 2 * S:
        return "all-pair"
    if nb < 3 * S:
        return "second-pass-tail"
    if nb <= 4 * S:
        return "paired-second-pass"
    return "third-pass"


def stem_wgrad_trips(c):
    """(fewest, most) trips of stem_wgrad_kernel's loop over the waves of the grid (0: an idle wave)"""
    nb, step = stem_nblk(c), stem_wgrad_step(c)
    return nb // step, cdiv(nb, step)


def stem_wgrad_regime(c):
    lo, hi = stem_wgrad_trips(c)
    if hi <= 1:
        return "one-trip"
    if hi == 2:
        return "mixed-trips" if lo == 1 else "two-trips"
    return "three-or-more"


def stem_case_id(c):
    return f"{c.B}x{c.Cin}x{c.H}x{c.W}"


STEM_CASES = [
    StemCase(1, 3, 9, 16),        # 9 blocks: one workgroup and a wave of a second; every block touches both borders
    StemCase(2, 1, 1, 48),        # H = 1: every tap row but the middle one is outside; 6 blocks
    StemCase(3, 2, 5, 32),        # 30 blocks: the last workgroup has two idle waves
    StemCase(3, 2, 683, 48),      # 6147 blocks: S < nblk < 2S, the first 2051 waves pair
    StemCase(8, 1, 512, 32),      # 8192 blocks: exactly 2S, every wave pairs (H even: 2^13 leaves no odd factor)
    StemCase(7, 3, 1465, 16),     # 10255 blocks: a second pass of one block on 2063 waves
    StemCase(1, 3, 13001, 16),    # 13001 blocks: second pass paired on 713 waves, single on the others
    StemCase(3, 2, 5501, 16),     # 16503 blocks: two paired passes, a third pass on 119 waves
]
# the weight gradient's dense run: one trip and mixed trips only (see stem_pool_reference: the bound grows with the trips)
STEM_WGRAD_DENSE = [c for c in STEM_CASES if stem_wgrad_regime(c) in ("one-trip", "mixed-trips")]


def stem_probe_pixels(c):
    """(b, y, x) of the impulse probes: corners, edge middles, both sides of every 16-pixel block boundary of one row (the
    first six boundaries), last row of one image next to the first row of the next, and one pixel of the very last block."""
    B, H, W = c.B, c.H, c.W
    pts = []

    def add(b, y, x):
        if 0 <= b < B and 0 <= y < H and 0 <= x < W and (b, y, x) not in pts:
            pts.append((b, y, x))
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        add(0, y, x)
    for xb in list(range(16, W, 16))[:6]:
        add(0, H // 2, xb - 1); add(0, H // 2, xb)
    add(0, H - 1, W // 3); add(1, 0, W // 3)                    # image boundary (B > 1)
    add(B - 1, H - 1, W - 1); add(B - 1, H - 1, W - 16); add(B - 1, 0, 0)
    for k in range(1, 6):                                        # pixels inside the image, spread over the passes of the loop
        add((B * k // 6) % B, (H * k // 6 + k) % H, (5 * k) % W)
    assert len(pts) <= 64
    return pts


def stem_probe_passes(c):
    """The probes in groups such that no output pixel is reached by two probes of a group (forward impulse run)."""
    passes = []
    for p in stem_probe_pixels(c):
        for g in passes:
            if all(q[0] != p[0] or abs(q[1] - p[1]) > 2 or abs(q[2] - p[2]) > 2 for q in g):
                g.append(p)
                break
        else:
            passes.append([p])
    return passes


def stem_lattice_density(c):
    """Share of non-zero inputs of the forward lattice run.  x in {-1, 0, 1}, w uniform in {-2, .., 2} (E w^2 = 2): E sum z^2 =
    2 * P * K * density per channel, kept below 2^21, an eighth of the exact range 2^24."""
    P, K = c.B * c.H * c.W, 9 * c.Cin
    return min(2.0 / 3.0, 2.0 ** 21 / (2.0 * P * K))


# ---- pooling ---------------------------------------------------------------------------------------------------------------
PoolCase = namedtuple("PoolCase", "dtype B H W Cp")


def pool_vec(dtype):
    return 8 if dtype == "bf16" else 4


def pool_items(c, kernel):
    """items (window x channel vector) the kernel walks: the forward visits whole windows, the others the odd border too"""
    cv = c.Cp // pool_vec(c.dtype)
    if kernel == "fwd":
        return c.B * (c.H // 2) * (c.W // 2) * cv
    return c.B * ((c.H + 1) // 2) * ((c.W + 1) // 2) * cv


def pool_grid(c, kernel):
    """blocks of 256 threads, window_grid() of csrc/channel_lanes.hpp: segk_maxpool2x2_fwd / _bwd / segk_bn_relu_apply_pool
    (cap 8192), kernel "stat": segk_maxpool_bwd_stat_blocks (cap 1024; 0 where the channel vectors are no power of two or more
    than 256)"""
    if c.B <= 0 or c.H < 2 or c.W < 2 or c.Cp <= 0 or c.Cp % 32 != 0:
        return 0
    total = pool_items(c, kernel)
    if total >= 2 ** 31:
        return 0
    if kernel == "stat":
        cv = c.Cp // pool_vec(c.dtype)
        if cv & (cv - 1) or cv > 256:
            return 0
        return min(cdiv(total, 256), STAT_GRID_CAP)
    return min(cdiv(total, 256), POOL_GRID_CAP)


def pool_trips(c, kernel):
    """most trips of the grid-stride loop over the threads of the grid (1: the loop does not stride)"""
    g = pool_grid(c, kernel)
    return cdiv(pool_items(c, kernel), g * 256) if g else 0


def pool_elements(c):
    return c.B * c.H * c.W * c.Cp


def pool_case_id(c):
    return f"{c.dtype}-{c.B}x{c.H}x{c.W}x{c.Cp}"


_SMALL = [(2, 8, 8, 32), (1, 9, 14, 96), (2, 6, 7, 64), (2, 7, 9, 256), (1, 2, 10, 1024), (1, 5, 2, 96), (2, 3, 3, 64)]
POOL_SMALL = [PoolCase(dt, *s) for dt in ("bf16", "fp32") for s in _SMALL]
# the smallest odd x odd images on which the three uncapped kernels stride at Cp = 1024: more than 8192 * 256 items
POOL_STRIDE = [PoolCase("bf16", 1, 257, 259, 1024), PoolCase("fp32", 1, 183, 183, 1024)]
POOL_CASES = POOL_SMALL + POOL_STRIDE

# the fused pooling-backward + BatchNorm-reduce form: (case, accumulate, degenerate channels, z passed)
StatCase = namedtuple("StatCase", "case accumulate degenerate with_z")
STAT_CASES = [StatCase(PoolCase(dt, *s), acc, deg, True)
              for dt in ("bf16", "fp32")
              for s, acc, deg in (((2, 8, 8, 32), 0, False), ((2, 6, 7, 64), 1, True), ((2, 7, 9, 256), 1, False),
                                  ((1, 2, 10, 1024), 1, True), ((2, 3, 3, 64), 0, False))]
STAT_CASES += [
    StatCase(PoolCase("bf16", 2, 259, 261, 64), 1, True, True),        # 1.04 grids of items: strides barely
    StatCase(PoolCase("bf16", 2, 259, 261, 128), 1, True, True),       # three trips
    StatCase(PoolCase("fp32", 2, 259, 261, 64), 1, True, True),        # three trips
    StatCase(PoolCase("fp32", 1, 67, 67, 1024), 1, False, True),       # 256 channel vectors: a thread per vector of the block
    StatCase(PoolCase("bf16", 2, 259, 261, 64), 1, False, False),      # z == NULL on non-degenerate channels, striding
    StatCase(PoolCase("fp32", 2, 7, 9, 256), 0, False, False),         # z == NULL, one trip
]


def stat_case_id(s):
    return pool_case_id(s.case) + ("-acc" if s.accumulate else "") + ("-deg" if s.degenerate else "") + ("" if s.with_z else "-noz")


def stat_degenerate_channels(Cp):
    """channel -> kind for the degenerate STAT cases: scale == 0 with shift > 0 (y = shift everywhere) and with shift < 0 (y = 0
    everywhere), |scale| = |shift| / 1000 (xhat only badly recovered from y)"""
    return {1: "zero+", Cp - 3: "zero-", 10: "tiny"}


# ---- BN-statistics finalisation --------------------------------------------------------------------------------------------
# (MT, C): both launch forms (one block up to 1024 rows, chunked above), the 512-row round trip, padded channels at C > 32
FINALIZE_CASES = [(1, 32), (7, 64), (512, 96), (1024, 32), (1025, 64), (3000, 1024)]
