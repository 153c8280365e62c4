"""Case table of the weight-gradient kernel matrix (tests/test_gpu_wgrad_matrix.py runs it on the GPU,
tests/test_wgrad_instances.py checks on the CPU that it reaches every compiled instance of csrc/wgrad.hip).
Plain Python, no torch: both test modules import it.

A case is (geo, dtype, CD, CA, CB, B, H, W, prologue, zero_page):
  geo 0 Conv2d 3x3, 1 Conv2d 1x1, 2 ConvTranspose2d(k=2,s=2) (dz := layer input [B,H,W,CD], srcA := output gradient
  [B,2H,2W,CA]); dtype "bf16" / "fp32"; CD, CA, CB padded channel counts of dz and of the two shifted sources;
  prologue: BatchNorm+ReLU on srcA inside the kernel; zero_page: segk_wgrad gets a zero page (False: zeros64 == NULL)."""
from collections import namedtuple

Case = namedtuple("Case", "geo dtype CD CA CB B H W prologue zero_page")

TAPS = {0: 9, 1: 1, 2: 4}
REF_MADD_CAP = 10 ** 9        # float64 reference on the CPU: P * taps * CD * (CA + CB) multiply-adds per case


def workgroup_shape(c):
    """(WC, WI): 32-channel blocks of dz and of the shifted operand per workgroup -- segk_wgrad_wc and launch_geo."""
    wi = 2 if c.CA % 64 == 0 and c.CB % 64 == 0 else 1
    if c.geo in (0, 2) and c.dtype == "bf16" and c.CD % 128 == 0 and wi == 2:
        if c.geo == 2 or c.zero_page:
            return 4, 2
    return (2 if c.CD % 64 == 0 else 1), wi


def uses_dma(c):
    return c.geo == 0 and c.dtype == "bf16" and c.zero_page


def tile_rows(c):
    """dz rows of one 16-pixel-wide tile of the instance that serves the case (WG<T, GEO, WC>::R; 8 for the LDS-DMA kernel)."""
    bf = c.dtype == "bf16"
    if c.geo == 2:
        return (8 if workgroup_shape(c)[0] == 4 else 4) if bf else 2
    return 8 if bf else 4


def tiles_of(c):
    return c.B * -(-c.H // tile_rows(c)) * -(-c.W // 16)


def instance_of(c):
    """Name of the kernel instance launch_geo selects for the case."""
    wc, wi = workgroup_shape(c)
    b = lambda v: "true" if v else "false"
    if uses_dma(c):
        return f"wgrad_dma_kernel<{wc},{wi},{b(c.prologue)},{b(c.H % 8 != 0 or c.W % 16 != 0)}>"
    return f"wgrad_kernel<{c.dtype},{c.geo},{wc},{wi}>"


def family_of(c):
    """Kernel family: what shares one body of code up to the workgroup shape."""
    if uses_dma(c):
        return "dma+prologue" if c.prologue else "dma"
    return f"staged-{c.dtype}-geo{c.geo}"


def image_kind(c):
    R = tile_rows(c)
    if c.H < R and c.W < 16:
        return "sub-tile"
    if c.H % R == 0 and c.W % 16 == 0:
        return "whole" if c.H > R and c.W > 16 and c.B >= 2 else "whole-small"
    return "ragged" if c.H % R != 0 and c.W % 16 != 0 and c.H > R and c.W > 16 else "other"


def ref_madds(c):
    return c.B * c.H * c.W * TAPS[c.geo] * c.CD * (c.CA + c.CB)


def case_id(c):
    s = f"g{c.geo}-{c.dtype}-{c.CD}x{c.CA}" + (f"+{c.CB}" if c.CB else "") + f"-{c.B}x{c.H}x{c.W}"
    return s + ("-pro" if c.prologue else "") + ("" if c.zero_page else "-nozp")


# Channel counts (CD, CA) that reach each workgroup shape: the small ones on the whole-tile and sub-tile images, the large ones
# on the ragged image.  CD = 128 / 256 reach <4,2> only where that shape exists (bf16 3x3 with a zero page, bf16
# ConvTranspose); elsewhere they fall to <2,2>, which those families then test at both widths.
_SHAPES = {(1, 1): ((32, 32), (96, 96)), (1, 2): ((32, 64), (96, 128)), (2, 1): ((64, 32), (192, 96)),
           (2, 2): ((64, 64), (192, 128)), (4, 2): ((128, 64), (256, 128))}
# Second sources (CA, CB) of the concat form, CA != CB, a k-tile boundary between the sources: CA % 64 == 0 with
# CB % 64 != 0 (selects WI = 1), the other way round, and both multiples of 64 (WI = 2).
_CONCAT = ((64, 32), (32, 96), (64, 128))


def _images(R):
    """whole tiles (2 x 2 tiles or more per image, two images), ragged (partial last tile both ways), smaller than a tile"""
    return ((2, 16, 32), (2, 13, 21), (2, R - 1, 7))


def _table():
    t = []
    for geo in (0, 1, 2):
        for dtype in ("bf16", "fp32"):
            for zp in ((True, False) if (geo == 0 and dtype == "bf16") else (True,)):
                for shape, ((cd0, ca0), (cd1, ca1)) in _SHAPES.items():
                    probe = Case(geo, dtype, cd0, ca0, 0, 1, 1, 1, False, zp)
                    if workgroup_shape(probe) != shape:
                        continue      # <4,2> exists for bf16 3x3 with a zero page and bf16 ConvTranspose only
                    R = tile_rows(probe)
                    for pro in ((False, True) if geo == 0 else (False,)):
                        if pro and not (zp and dtype == "bf16") and shape not in ((1, 1), (2, 2)):
                            continue  # the staged kernels apply the prologue while staging, whatever the shape: two shapes
                        for i, (B, H, W) in enumerate(_images(R)):
                            cd, ca = (cd1, ca1) if i == 1 else (cd0, ca0)
                            t.append(Case(geo, dtype, cd, ca, 0, B, H, W, pro, zp))
                if geo == 0:      # torch.cat((skip, upsampled)) in front of a 3x3 convolution; no prologue on that form
                    for j, (ca, cb) in enumerate(_CONCAT):
                        B, H, W = _images(8 if dtype == "bf16" else 4)[1 if j else 0]
                        t.append(Case(geo, dtype, 64 if j < 2 else 128, ca, cb, B, H, W, False, zp))
    # CD % 128 == 0 without a zero page: the dispatch must fall to the register-staged <2,2>, not to a 4 x 2 form
    t.append(Case(0, "bf16", 128, 64, 0, 2, 16, 32, False, False))
    return t


CASES = _table()

# One case per kernel family for the split-K sweep (S below, at and above the tile count): ragged images, so that the last
# slabs own partial tiles.
SPLIT_CASES = [
    Case(0, "bf16", 64, 64, 0, 2, 13, 21, False, True),       # LDS-DMA
    Case(0, "bf16", 128, 64, 0, 2, 13, 21, True, True),       # LDS-DMA with the prologue, the 4 x 2 workgroup
    Case(0, "fp32", 64, 32, 0, 2, 13, 21, False, True),       # register-staged fp32 3x3
    Case(1, "bf16", 32, 64, 0, 2, 13, 21, False, True),       # 1x1
    Case(2, "bf16", 64, 64, 0, 2, 13, 21, False, True),       # ConvTranspose <2,2>
    Case(2, "bf16", 128, 64, 0, 2, 13, 21, False, True),      # ConvTranspose <4,2> (8-row tiles)
]
