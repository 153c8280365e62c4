"""Case table of the 3x3 convolution forward / data-gradient matrix (tests/test_gpu_conv_matrix.py runs it on the GPU,
tests/test_conv_instances.py checks on the CPU that it reaches every compiled 3x3 instance of csrc/conv_igemm.hip,
csrc/conv_pipe.hip, csrc/conv_ws.hip and csrc/conv_rs.hip) and a Python mirror of the dispatch.  Plain Python, no torch: both test modules import it.

A case is (dtype, B, H, W, CA, CB, CO1, CO2, prologue, act_out, bias, stats, mode): the arguments of segk_conv3x3 /
segk_conv3x3_act.  dtype "bf16" / "fp32"; CA, CB padded channel counts of the two sources, CO1, CO2 of the two destinations;
prologue: BatchNorm+ReLU on srcA inside the kernel; act_out: through segk_conv3x3_act with the side output; mode 0 forward
weights, 1 data-gradient weights (the reference is then the transposed convolution).  Cases on an image of odd height carry
logical channel counts below the padding (logical_of): 40 of 64 in (bf16), 70 of 96 out."""
from collections import namedtuple

Case = namedtuple("Case", "dtype B H W CA CB CO1 CO2 prologue act_out bias stats mode")

NUM_CUS = 256                   # MI355X: the launch arithmetic below (grids, statistics rows of conv_rs) is evaluated for it
REF_MADD_CAP = 6 * 10 ** 8      # float64 reference on the CPU: P * 9 * (CA + CB) * (CO1 + CO2) multiply-adds per dense case
LDS_BYTES = 160 * 1024
PIXB = 80                       # conv_tile.hpp: LDS pitch of one pixel's 64-byte chunk


def cdiv(a, b):
    return -(-a // b)


# ---- the dispatch: segk_conv_plan (segk_conv_use_rs, use_ws, use_pipe, generic_tile), launch_geo, launch_pipe ----------------
def use_rs(cin, n, dtype, W):
    return dtype == "bf16" and cin in (32, 64) and n % 64 == 0 and W > 16


def use_ws(cin, n, dtype):
    return dtype == "bf16" and cin <= 64 and n % 64 == 0


def use_pipe(cin, n, dtype):
    """channel tile of the producer/consumer kernel (128 | 64) or 0"""
    if dtype != "bf16" or use_ws(cin, n, dtype) or cin < 64:
        return 0
    if n % 128 == 0:
        return 128
    return 64 if n % 64 == 0 and cin >= 128 else 0


def writes_act(cin, n, dtype):
    return use_ws(cin, n, dtype) or use_pipe(cin, n, dtype) != 0


def conv_bm(n):
    return 256 if n % 128 == 0 else 128


def conv_twl(bm, W):
    return 4 if bm == 128 else (5 if W > 16 else 4)


def select(dtype, cin, n, W, bias, prologue, chunks_even=None):
    """(form, template parameters) launch_geo reaches for a valid call; form in rs, ws, pipe, generic.  None: the call is refused
    only together with statistics (is_valid), never here."""
    wide = 5 if W > 16 else 4
    if chunks_even is None:
        chunks_even = (cin // 32) % 2 == 0
    if dtype == "bf16":
        if use_rs(cin, n, dtype, W) and not bias:
            return "rs", (cin // 32, prologue)
        if use_ws(cin, n, dtype):
            return "ws", (wide, prologue)
        pk = use_pipe(cin, n, dtype)
        if pk:
            return "pipe", (wide, prologue, pk, not prologue and not bias and chunks_even)
    if n % 128 == 0:
        return "generic", (dtype, wide, 4, 2, 2, 2, 2, prologue)
    if n % 64 == 0:
        return "generic", (dtype, 4, 2, 2, 2, 1, 1, prologue)
    return "generic", (dtype, 4, 4, 1, 1, 1, 1, prologue)


def spell(form, p):
    b = lambda v: "true" if v else "false"
    if form == "rs":
        return f"conv_rs_kernel<{p[0]},{b(p[1])}>"
    if form == "ws":
        return f"conv_ws_kernel<bf16,{p[0]},{b(p[1])}>"
    if form == "pipe":
        return f"conv3x3_pipe_kernel<{p[0]},{b(p[1])},{p[2]},{b(p[3])}>"
    return "conv_igemm_kernel<{},0,{},{},{},{},{},{},{}>".format(*p[:7], b(p[7]))


def _sel(c):
    return select(c.dtype, c.CA + c.CB, c.CO1 + c.CO2, c.W, c.bias, c.prologue)


def instance_of(c):
    """Name of the kernel instance launch_geo selects for the case, spelled as the compiler prints the instance."""
    return spell(*_sel(c))


def is_valid(c):
    """What segk_conv_igemm_launch and launch_geo accept."""
    cin, n = c.CA + c.CB, c.CO1 + c.CO2
    ok = c.CA > 0 and c.CA % 32 == 0 and c.CB % 32 == 0 and c.CO1 > 0 and c.CO1 % 32 == 0 and c.CO2 % 32 == 0
    ok = ok and not (c.prologue and c.CB)
    ok = ok and (not c.act_out or (c.prologue and not c.bias and not c.CO2 and writes_act(cin, n, c.dtype)))
    ok = ok and not (c.bias and c.stats and use_rs(cin, n, c.dtype, c.W))       # refused: the statistics rows would not match
    return ok


def family_of(c):
    """Kernel family: what shares one body of code and one launch arithmetic."""
    form, p = _sel(c)
    if form == "pipe":
        return f"pipe-{'dma' if p[3] else 'staged'}-{p[2]}"
    return f"generic-{c.dtype}" if form == "generic" else form


PERSISTENT_FAMILIES = ("pipe-staged-128", "pipe-dma-128", "pipe-dma-64", "rs", "ws", "generic-bf16", "generic-fp32")


def tile_shape(c):
    """(TH, TW) of the instance's pixel tile."""
    form, p = _sel(c)
    if form == "rs":
        return 8, 32
    if form == "ws":
        bm, twl = 256, p[0]
    elif form == "pipe":
        bm, twl = 32768 // p[2], p[0]
    else:
        bm, twl = p[2] * p[4] * 32, p[1]
    return bm >> twl, 1 << twl


def stationary_grid(MT, NT):
    """segk_conv_rs_grid and launch_ws: workgroups per XCD (a multiple of the NT channel tiles) and per channel tile, for MT
    pixel tiles"""
    gw = NUM_CUS // 8
    gw -= gw % NT
    gw = max(min(gw, cdiv(MT, 8) * NT), NT)
    return gw, gw // NT


def tiles_of(c):
    """segk_conv_tiles(B, H, W, CA + CB, CO1 + CO2, dtype): rows of the statistics buffer.  Like the query it does not know the
    bias: a biased call of a conv_rs shape gets conv_rs's row count (and is refused with statistics)."""
    cin, n = c.CA + c.CB, c.CO1 + c.CO2
    if use_rs(cin, n, c.dtype, c.W):
        return 8 * stationary_grid(c.B * cdiv(c.W, 32) * cdiv(c.H, 8), n // 64)[1] * 4
    pk = use_pipe(cin, n, c.dtype)
    bm = 256 if use_ws(cin, n, c.dtype) else 32768 // pk if pk else conv_bm(n)
    twl = conv_twl(bm, c.W)
    return c.B * cdiv(c.W, 1 << twl) * cdiv(c.H, bm >> twl)


def units_per_workgroup(c):
    """Most work units (pixel tile x channel tile) one persistent workgroup walks on a device of NUM_CUS compute units:
    launch_pipe_m, launch_ws, segk_conv_rs_grid, launch_pro."""
    form, p = _sel(c)
    n = c.CO1 + c.CO2
    TH, TW = tile_shape(c)
    MT = c.B * cdiv(c.H, TH) * cdiv(c.W, TW)
    if form in ("rs", "ws"):          # the channel tile is fixed per workgroup, GW workgroups of an XCD share its pixel tiles
        return cdiv(cdiv(MT, 8), stationary_grid(MT, n // 64)[1])
    if form == "pipe":
        per_xcd = cdiv(MT * (n // p[2]), 8)
        return cdiv(per_xcd, min(NUM_CUS // 8, per_xcd))
    _, twl, wm, wn, mf, nf, pbuf, _ = p
    es = 2 if c.dtype == "bf16" else 4
    bm, bn, nthr = wm * mf * 32, wn * nf * 32, wm * wn * 64
    rowp = ((TW + 2) * PIXB + 255) & ~255
    lds = max(pbuf * (TH + 2) * rowp + 2 * 3 * bn * PIXB + nthr * 16, bm * (bn * es + 16) + wm * bn * 8)
    per_xcd = cdiv(MT * (n // bn), 8)
    return cdiv(per_xcd, min((NUM_CUS // 8) * min(LDS_BYTES // lds, 1 if nthr == 512 else 2), per_xcd))


def image_kind(c):
    TH, TW = tile_shape(c)
    if c.H < TH and c.W < TW:
        return "sub-tile"
    if c.H % TH == 0 and c.W % TW == 0:
        return "whole"
    return "ragged" if c.H % TH != 0 and c.W % TW != 0 and c.H > TH and c.B >= 2 else "other"


def logical_of(c):
    """(LA, LB, LO1, LO2) logical channel counts: below the padding on images of odd height, the padded counts elsewhere.  The
    last source block is short by less than one K chunk, so that its last chunk is partly filled (bf16, chunks of 32: 24
    short, 40 of 64; fp32, chunks of 16: 8 short, 56 of 64); the last destination block is 26 short (70 of 96)."""
    if c.H % 2 == 0 or c.H == 1:
        return c.CA, c.CB, c.CO1, c.CO2
    short = 24 if c.dtype == "bf16" else 8
    la, lb = (c.CA, c.CB - short) if c.CB else (c.CA - short, 0)
    lo1, lo2 = (c.CO1, c.CO2 - 26) if c.CO2 else (c.CO1 - 26, 0)
    return la, lb, lo1, lo2


def ref_madds(c):
    return c.B * c.H * c.W * 9 * (c.CA + c.CB) * (c.CO1 + c.CO2)


def case_id(c):
    s = f"{c.dtype}-{c.B}x{c.H}x{c.W}-{c.CA}" + (f"+{c.CB}" if c.CB else "") + f"-{c.CO1}" + (f"+{c.CO2}" if c.CO2 else "")
    f = ("p" if c.prologue else "") + ("a" if c.act_out else "") + ("b" if c.bias else "") + ("s" if c.stats else "")
    return s + ("-" + f if f else "") + ("-dgrad" if c.mode else "")


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _mk(dtype, img, cfg):
    """cfg = (CA, CB, CO1, CO2, flags): p prologue, a act_out, b bias, s statistics, m mode-1 weights"""
    CA, CB, CO1, CO2, f = cfg
    return Case(dtype, *img, CA, CB, CO1, CO2, "p" in f, "a" in f, "b" in f, "s" in f, 1 if "m" in f else 0)


def _tile(dtype, cfg, W):
    return tile_shape(_mk(dtype, (1, 1, W), cfg))


# Every entry: dtype, whether the dispatch depends on W > 16, and the arguments of the whole-tile, the ragged and the sub-tile
# image.  An entry whose dispatch depends on W is run at W <= 16 and at W > 16 (two instances, or two kernels: conv_ws serves
# the conv_rs shapes at W <= 16) and its whole-tile arguments on the pair W = 16 / W = 17 at equal height.
_ENTRIES = [
    # Cin = 32: conv_rs<1,*> (W > 16) / conv_ws<4,*>
    ("bf16", True, (32, 0, 64, 0, "s"), (32, 0, 64, 128, "sm"), (32, 0, 128, 0, "")),
    ("bf16", True, (32, 0, 64, 0, "pas"), (32, 0, 64, 128, "ps"), (32, 0, 64, 0, "pa")),
    # Cin = 64: conv_rs<2,*> / conv_ws<4,*>; two sources are 32 + 32 here (the only split of two chunks)
    ("bf16", True, (32, 32, 64, 0, "sm"), (64, 0, 32, 96, "s"), (64, 0, 64, 0, "")),
    ("bf16", True, (64, 0, 64, 0, "pas"), (64, 0, 128, 0, "pas"), (64, 0, 32, 96, "pm")),
    # ... with a bias: conv_ws<5,*> / conv_ws<4,*> (no statistics: the combination is refused at W > 16)
    ("bf16", True, (32, 32, 64, 0, "b"), (64, 0, 32, 96, "bm"), (32, 0, 128, 0, "b")),
    ("bf16", True, (64, 0, 64, 0, "pb"), (32, 0, 64, 128, "pbm"), (64, 0, 64, 0, "pb")),
    # producer/consumer kernel, 128-channel tiles: LDS-DMA (no prologue, no bias, even chunk count), staged (odd chunk count
    # or bias), staged with the prologue
    ("bf16", True, (128, 0, 128, 0, "s"), (64, 128, 32, 96, "sm"), (128, 0, 128, 0, "")),
    ("bf16", True, (96, 0, 128, 0, "sm"), (64, 96, 32, 96, "s"), (128, 0, 128, 0, "b")),
    ("bf16", True, (128, 0, 128, 0, "pas"), (96, 0, 32, 96, "pbsm"), (96, 0, 128, 0, "pa")),
    # ... 64-channel tiles (Cin >= 128, N = 64 | 192)
    ("bf16", True, (128, 0, 64, 0, "s"), (64, 128, 64, 128, "s"), (256, 0, 64, 0, "")),
    ("bf16", True, (160, 0, 64, 0, "sm"), (64, 96, 64, 128, "sm"), (128, 0, 64, 0, "b")),
    ("bf16", True, (128, 0, 64, 0, "pas"), (160, 0, 64, 128, "pbs"), (128, 0, 64, 0, "pam")),
    # generic bf16: N % 64 == 0 is left to it at Cin = 96 only, N % 32 at every Cin
    ("bf16", False, (96, 0, 64, 0, "sm"), (32, 64, 64, 128, "bs"), (96, 0, 64, 0, "")),
    ("bf16", False, (96, 0, 64, 0, "ps"), (96, 0, 64, 128, "pbsm"), (96, 0, 64, 0, "p")),
    ("bf16", False, (64, 0, 32, 0, "s"), (32, 96, 32, 64, "bsm"), (128, 0, 96, 0, "")),
    ("bf16", False, (32, 0, 96, 0, "psm"), (64, 0, 32, 64, "pbs"), (64, 0, 32, 0, "p")),
    # generic fp32: every shape
    ("fp32", True, (32, 0, 128, 0, "s"), (32, 64, 32, 96, "bsm"), (64, 0, 128, 0, "")),
    ("fp32", True, (64, 0, 128, 0, "psm"), (64, 0, 32, 96, "pbs"), (32, 0, 128, 0, "p")),
    ("fp32", False, (64, 0, 64, 0, "sm"), (32, 64, 64, 128, "bs"), (32, 0, 64, 0, "")),
    ("fp32", False, (32, 0, 64, 0, "ps"), (64, 0, 64, 128, "pbsm"), (32, 0, 64, 0, "p")),
    ("fp32", False, (32, 0, 32, 0, "s"), (32, 96, 32, 64, "bsm"), (64, 0, 96, 0, "")),
    ("fp32", False, (64, 0, 96, 0, "psm"), (64, 0, 32, 64, "pbs"), (32, 0, 32, 0, "p")),
]


def _table():
    t = []
    for dtype, wdep, whole, ragged, sub in _ENTRIES:
        if not wdep:          # 8 x 16 tiles at every width
            imgs = [((2, 16, 32), whole), ((2, 13, 21), ragged), ((2, 3, 5), sub), ((1, 1, 1), sub)]
        else:
            th4 = _tile(dtype, whole, 16)[0]
            imgs = [((2, 2 * th4, 16), whole), ((2, _tile(dtype, ragged, 11)[0] + 3, 11), ragged), ((2, 3, 5), sub),
                    ((1, 1, 1), sub), ((2, 2 * th4, 17), whole),
                    ((2, 2 * _tile(dtype, whole, 64)[0], 64), whole), ((2, _tile(dtype, ragged, 41)[0] + 5, 41), ragged),
                    ((2, 3, 17), sub)]
        t += [_mk(dtype, img, cfg) for img, cfg in imgs]
    # the two LDS-DMA families have one entry each: forward and data-gradient weights on a whole-tile and a ragged image of both
    t.append(_mk("bf16", (2, 16, 64), (128, 0, 128, 0, "sm")))
    t.append(_mk("bf16", (2, 13, 41), (64, 128, 32, 96, "s")))
    t.append(_mk("bf16", (2, 32, 64), (128, 0, 64, 0, "sm")))
    t.append(_mk("bf16", (2, 21, 41), (64, 128, 64, 128, "m")))
    return t


CASES = _table()

# Three or more work units on some workgroup (units_per_workgroup): the weight ring, the patch pipeline and the DMA ring run
# across unit boundaries.  Exact lattice run only.
LONG_CASES = [
    Case("bf16", 33, 18, 34, 96, 0, 384, 0, False, False, False, True, 0),        # pipe staged, 128-channel tiles
    Case("bf16", 33, 18, 34, 64, 64, 384, 0, False, False, False, True, 0),       # pipe LDS-DMA, 128-channel tiles
    Case("bf16", 29, 34, 34, 128, 0, 64, 128, False, False, False, True, 1),      # pipe LDS-DMA, 64-channel tiles
    Case("bf16", 22, 18, 34, 64, 0, 256, 0, True, False, False, True, 0),         # conv_rs
    Case("bf16", 44, 34, 12, 64, 0, 256, 0, False, False, False, True, 0),        # conv_ws
    Case("bf16", 38, 18, 34, 96, 0, 64, 128, False, False, False, True, 0),       # generic bf16, two 4-wave workgroups per CU
    Case("fp32", 29, 18, 34, 32, 0, 384, 0, False, False, False, True, 0),        # generic fp32, 8 waves
]

# ---- inputs of the impulse and the lattice run -----------------------------------------------------------------------------------------------
def lattice_density(c):
    """Share of non-zero activations of the lattice run: 2/3 (x uniform in {-1, 0, 1}) unless the statistics would leave the
    exact range.  z is a multiple of 1/2, so z^2 counts in units of 1/4; with w uniform in {-1, -1/2, 0, 1/2, 1} (E w^2 = 1/2)
    E sum z^2 = P * K * density / 2, i.e. 2 * P * K * density units: kept below 2^21, an eighth of 2^24."""
    P, K = c.B * c.H * c.W, 9 * (c.CA + c.CB)
    return min(2.0 / 3.0, 2.0 ** 21 / (2.0 * P * K))


def input_channels(c):
    """padded positions of the logical input channels of [srcA | srcB]"""
    la, lb, _, _ = logical_of(c)
    return list(range(la)) + [c.CA + j for j in range(lb)]


def probe_pixels(c):
    """(b, y, x, k) of the impulse probes: corners, edge middles, both sides of every tile boundary in x and in y (conv_rs:
    of the two-row wave slabs too), first and last pixel of the last (partial) tile, last row of one image and first row of
    the next; k walks the logical input channels, first and last of each source first."""
    B, H, W = c.B, c.H, c.W
    TH, TW = tile_shape(c)
    pts = []

    def add(b, y, x):
        if 0 <= y < H and 0 <= x < W and (b, y, x) not in pts:
            pts.append((b, y, x))
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        add(0, y, x)
    for xb in range(TW, W, TW):
        add(0, H // 2, xb - 1); add(0, H // 2, xb)
    for R in ((2, TH) if _sel(c)[0] == "rs" else (TH,)):
        for yb in range(R, H, R):
            add(B - 1, yb - 1, W // 2); add(B - 1, yb, W // 2)
    add(B - 1, (H - 1) // TH * TH, (W - 1) // TW * TW); add(B - 1, H - 1, W - 1)
    add(0, H - 1, W // 3); add(B - 1, 0, W // 3)
    ch = input_channels(c)
    first = [ch[0], ch[-1], ch[len(ch) // 2], ch[min(31, len(ch) - 1)], ch[min(32, len(ch) - 1)], c.CA - 1 if c.CA - 1 in ch else ch[0]]
    return [(b, y, x, first[i] if i < len(first) else ch[i * 13 % len(ch)]) for i, (b, y, x) in enumerate(pts)]


def probe_passes(c):
    """The probes in as few groups as a greedy pass finds such that no output pixel is reached by two probes of a group (the
    3 x 3 neighbourhoods of two probes of one image do not overlap): every output is then one weight or zero."""
    passes = []
    for p in probe_pixels(c):
        for g in passes:
            if all(q[0] != p[0] or abs(q[1] - p[1]) > 2 or abs(q[2] - p[2]) > 2 for q in g):
                g.append(p)
                break
        else:
            passes.append([p])
    return passes
