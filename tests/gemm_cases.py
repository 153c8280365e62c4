"""Case table of the 1x1-geometry matrix -- segk_linear, segk_linear_splitk, segk_conv1x1, segk_convt2x2_fwd and
segk_convt2x2_dgrad: gemm_dma_kernel (csrc/gemm.hip), convt_stream_kernel (csrc/convt_stream.hip) and the GEO == 1 instances
of conv_igemm_kernel (csrc/conv_igemm.hip) -- and a Python mirror of their dispatch.  tests/test_gpu_gemm_matrix.py runs the
table on the GPU, tests/test_gemm_instances.py checks on the CPU that it reaches every compiled instance.  Plain Python, no
torch: both import it.

A case is (entry, dtype, B, H, W, Cin, Cout, S, bias, act, Lin, Lout): the ABI entry and its arguments.  entry "linear" /
"linear_splitk": M = B * H * W rows (B = 1, W = 16: the strip segk_linear itself forms), K = Cin, N = Cout, S the split (1
elsewhere); "conv1x1": [B, H, W, Cin] -> [B, H, W, Cout]; "convt_fwd": [B, H, W, Cin] -> [B, 2H, 2W, Cout]; "convt_dgrad":
dout [B, 2H, 2W, Cout] -> din [B, H, W, Cin] (Cin, Cout are the layer's in both).  Cin, Cout are the padded channel counts
the kernels see, Lin, Lout the logical ones (equal unless the case carries padding: 40 of 64 in, 70 of 96 out)."""
from collections import namedtuple

from conv_cases import LDS_BYTES, NUM_CUS, PIXB, cdiv

Case = namedtuple("Case", "entry dtype B H W Cin Cout S bias act Lin Lout")

ENTRIES = ("linear", "linear_splitk", "conv1x1", "convt_fwd", "convt_dgrad")
REF_MADD_CAP = 5 * 10 ** 9      # float64 matmul on the CPU: M * K * N multiply-adds per dense case (3152 x 256 x 2560: 0.07 s)
G_BN = 128                      # gemm.hip: channel tile of every work unit


def mk(entry, dtype, B, H, W, Cin, Cout, S=1, bias=False, act=0, Lin=None, Lout=None):
    return Case(entry, dtype, B, H, W, Cin, Cout, S, bias, act, Cin if Lin is None else Lin, Cout if Lout is None else Lout)


def lin(dtype, M, K, N, S=1, bias=False, act=0, Lin=None, Lout=None):
    return mk("linear_splitk" if S else "linear", dtype, 1, M // 16, 16, K, N, S or 1, bias, act, Lin, Lout)


def rows_of(c):
    return c.B * c.H * c.W


def gemm_view(c):
    """(M, K, N, mode) of the GEMM the entry runs: mode 0 plain, 1 pixel-shuffle store, 2 un-shuffle gather"""
    M = rows_of(c)
    if c.entry == "convt_fwd":
        return M, c.Cin, 4 * c.Cout, 1
    if c.entry == "convt_dgrad":
        return M, 4 * c.Cout, c.Cin, 2
    return M, c.Cin, c.Cout, 0


# ---- the dispatch ------------------------------------------------------------------------------------------------------------
def convt_stream_ok(B, H, W, Cin, Cout, dtype):
    """segk_convt_stream_ok"""
    if dtype != "bf16" or W % 16 != 0 or Cout % 32 != 0 or B * H * W * 4 >= 2147483647 or Cin not in (128, 256):
        return False
    nbw, n16 = (8 if Cin == 128 else 4), 4 * Cout // 16
    return n16 % nbw == 0 and n16 // nbw in (1, 2, 4, 8)


def convt_stream_dgrad_ok(B, H, W, Cin, Cout, dtype):
    """segk_convt_stream_dgrad_ok"""
    return dtype == "bf16" and W % 16 == 0 and B * H * W * 4 < 2147483647 and Cin == 128 and Cout == 64


def min_chunks(mode):
    return 16 if mode == 1 else 8


def gemm_dma_ok(M, nchunks, nchA, N, cout_shuffle, lda, mode):
    """segk_gemm_dma_ok"""
    if nchunks < 2 or nchunks < min_chunks(mode) or nchunks & 1 or N % G_BN != 0 or M < 128:
        return False
    if mode == 2 and nchA & 1:
        return False
    if mode == 1 and cout_shuffle % 8 != 0:
        return False
    return (4 * M if mode == 2 else M) * lda * 2 < 4294967296


def gemm_rounds(M, N, ks, bm):
    """gemm_rounds: rounds of the work units on the chip, in units of one 256-row tile's time"""
    return cdiv(cdiv(M, bm) * (N // 128) * ks, NUM_CUS) * bm / 256.0


def dma_bm(M, N, ks):
    """launch_mode"""
    return 320 if gemm_rounds(M, N, ks, 320) < gemm_rounds(M, N, ks, 256) else 256


def splitk_ok(M, K, N, S, dtype="bf16"):
    """what segk_linear_splitk accepts (gemm_dma_launch's own conditions included)"""
    if dtype != "bf16" or M <= 0 or M % 16 or K <= 0 or K % 64 or N <= 0 or S < 1:
        return False
    return gemm_dma_ok(M, K // 32, K // 32, N, N, K, 0) and (K // 64) % S == 0 and K // 64 // S >= 1


def is_valid(c):
    """what the five entries and segk_conv_igemm_launch accept"""
    ch = 32 if c.dtype == "bf16" else 16
    ok = c.entry in ENTRIES and c.dtype in ("bf16", "fp32") and min(c.B, c.H, c.W) > 0 and rows_of(c) * 4 < 2147483647
    ok = ok and c.Cin > 0 and c.Cout > 0 and 0 < c.Lin <= c.Cin and 0 < c.Lout <= c.Cout and c.act in (0, 1) and c.S >= 1
    if c.entry in ("linear", "linear_splitk"):
        ok = ok and c.B == 1 and c.W == 16 and c.H < (1 << 24)
    if c.entry == "linear_splitk":
        return ok and not c.act and splitk_ok(rows_of(c), c.Cin, c.Cout, c.S, c.dtype)
    ok = ok and c.S == 1 and (c.entry == "linear" or not c.act) and not (c.entry == "convt_dgrad" and c.bias)
    if c.entry == "convt_dgrad":          # K = Cout per tap, N = Cin
        return ok and c.Cout % ch == 0 and c.Cin % 32 == 0
    return ok and c.Cin % ch == 0 and c.Cout % 32 == 0


def select(c):
    """(form, parameters) the entry reaches: ("dma", (mode, BM)), ("stream", (KS, NBW, MODE, wpc)) or
    ("generic", (dtype, TWL, WM, WN, MF, NF, PBUF))"""
    M, K, N, mode = gemm_view(c)
    if c.entry == "linear_splitk":
        return "dma", (0, dma_bm(M, N, c.S))
    if c.entry == "convt_fwd" and convt_stream_ok(c.B, c.H, c.W, c.Cin, c.Cout, c.dtype):
        ks, nbw = (4, 8) if c.Cin == 128 else (8, 4)
        return "stream", (ks, nbw, 0, 4 * c.Cout // 16 // nbw)
    if c.entry == "convt_dgrad" and convt_stream_dgrad_ok(c.B, c.H, c.W, c.Cin, c.Cout, c.dtype):
        return "stream", (8, 4, 1, c.Cin // 16 // 4)
    wide = 5 if c.W > 16 else 4
    if c.dtype == "bf16":         # launch_geo<bf16, 1>
        lda = c.Cout if mode == 2 else c.Cin          # ConvArgs::CA
        if gemm_dma_ok(M, K // 32, lda // 32, N, c.Cout if mode == 1 else N, lda, mode):
            return "dma", (mode, dma_bm(M, N, 1))
        if N % 128 == 0:
            return "generic", ("bf16", 4, 2, 2, 2, 2, 2)
        if N % 64 == 0:
            return "generic", ("bf16", 4, 2, 2, 2, 1, 2)
        return "generic", ("bf16", wide, 8, 1, 1, 1, 2)
    if N % 128 == 0:
        return "generic", ("fp32", wide, 4, 2, 2, 2, 2)
    if N % 64 == 0:
        return "generic", ("fp32", wide, 4, 2, 2, 1, 2)
    return "generic", ("fp32", wide, 8, 1, 1, 1, 2)


def spell(form, p):
    if form == "dma":
        return f"gemm_dma_kernel<{p[0]},{p[1]}>"
    if form == "stream":
        return f"convt_stream_kernel<{p[0]},{p[1]},{p[2]}>"
    return "conv_igemm_kernel<{},1,{},{},{},{},{},{},false>".format(*p)


def kernel_of(c):
    """the compiled instance, spelled as tests/test_gemm_instances.py parses the compiler's names"""
    return spell(*select(c))


def instance_of(c):
    """kernel_of with the wave layout (waves that cover all channels) appended for the streaming kernel"""
    form, p = select(c)
    return spell(form, p) + (f" wpc={p[3]}" if form == "stream" else "")


def family_of(c):
    form, p = select(c)
    return f"dma-{p[0]}-{p[1]}" if form == "dma" else f"stream-{p[2]}" if form == "stream" else f"generic-{c.dtype}"


def tile_shape(c):
    """(TH, TW) of the generic kernel's pixel tile; (BM // 16, 16) for the row tile of the LDS-DMA GEMM (rows are not pixels of
    an image there: only TH * TW counts); (1, 16) for the streaming kernel's sixteen-pixel block"""
    form, p = select(c)
    if form == "dma":
        return p[1] // 16, 16
    if form == "stream":
        return 1, 16
    bm, twl = p[2] * p[4] * 32, p[1]
    return bm >> twl, 1 << twl


def units_per_workgroup(c):
    """Most work units one persistent workgroup walks on NUM_CUS compute units: launch_dma, launch_pro"""
    form, p = select(c)
    M, K, N, _ = gemm_view(c)
    if form == "dma":
        per_xcd = cdiv(cdiv(M, p[1]) * (N // G_BN) * c.S, 8)
        return cdiv(per_xcd, min(NUM_CUS // 8, per_xcd))
    assert form == "generic"
    _, twl, wm, wn, mf, nf, pbuf = p
    es = 2 if c.dtype == "bf16" else 4
    bm, bn, nthr = wm * mf * 32, wn * nf * 32, wm * wn * 64
    TH, TW = bm >> twl, 1 << twl
    rowp = (TW * PIXB + 255) & ~255
    lds = max(pbuf * TH * rowp + 2 * bn * PIXB + nthr * 16, bm * (bn * es + 16) + wm * bn * 8)
    per_xcd = cdiv(c.B * cdiv(c.H, TH) * cdiv(c.W, TW) * (N // bn), 8)
    return cdiv(per_xcd, min((NUM_CUS // 8) * min(LDS_BYTES // lds, 1 if nthr == 512 else 2), per_xcd))


def unit_walk(c):
    """(row tile, column tile, K split) of the units workgroup 0 of XCD 0 of the LDS-DMA GEMM walks, in order"""
    form, p = select(c)
    assert form == "dma"
    M, K, N, _ = gemm_view(c)
    NT, U = N // G_BN, cdiv(M, p[1]) * (N // G_BN) * c.S
    upx = cdiv(U, 8)
    gw = min(NUM_CUS // 8, upx)
    return [(u // (NT * c.S), u % NT, (u // NT) % c.S) for u in range(0, min(U, upx), gw)]


def stream_grid(c):
    """(sixteen-pixel blocks, workgroups, streams per workgroup) of convt_stream's launch"""
    form, p = select(c)
    assert form == "stream"
    nblk, streams = c.B * c.H * (c.W // 16), 8 // p[3]
    return nblk, min(cdiv(nblk, streams), NUM_CUS), streams


def blocks_per_stream(c):
    """most trips of a wave group of convt_stream round its ping-pong loop"""
    nblk, g, streams = stream_grid(c)
    return cdiv(nblk, g * streams)


def image_kind(c):
    """whole / ragged / sub-tile (/ other); the LDS-DMA GEMM also "min" (M = 128, its least) and "tile+16" """
    form, p = select(c)
    M = rows_of(c)
    TH, TW = tile_shape(c)
    if form == "stream":
        return "sub-tile" if (c.B, c.H, c.W) == (1, 1, 16) else "whole"
    if form == "dma":
        bm = p[1]
        return "min" if M == 128 else "whole" if M % bm == 0 else "tile+16" if M == bm + 16 else "ragged"
    if c.entry == "linear":
        return "sub-tile" if M == 16 else "whole" if M % (TH * TW) == 0 else "ragged"
    if c.H < TH and c.W < TW:
        return "sub-tile"
    if c.H % TH == 0 and c.W % TW == 0:
        return "whole"
    return "ragged" if c.H % TH != 0 and c.W % TW != 0 and c.H > TH and c.B >= 2 else "other"


def nchunks_of(c):
    return gemm_view(c)[1] // 32


def ref_madds(c):
    M, K, N, _ = gemm_view(c)
    return M * K * N


def case_id(c):
    if c.entry in ("linear", "linear_splitk"):
        s = f"{c.entry}-{c.dtype}-{rows_of(c)}x{c.Cin}x{c.Cout}" + (f"-S{c.S}" if c.entry == "linear_splitk" else "")
    else:
        s = f"{c.entry}-{c.dtype}-{c.B}x{c.H}x{c.W}-{c.Cin}-{c.Cout}"
    if (c.Lin, c.Lout) != (c.Cin, c.Cout):
        s += f"-l{c.Lin}.{c.Lout}"
    f = ("b" if c.bias else "") + ("a" if c.act else "")
    return s + ("-" + f if f else "")


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _generic_cases():
    t = []
    # bf16.  N % 128 and N % 64 on 8 x 16 tiles (128 pixels) at every width; the rest on 256-pixel tiles, 16 x 16 or 8 x 32.
    # K stays below the LDS-DMA GEMM's threshold (8 chunks; 16 for the pixel-shuffle store), or M below its 128 rows.
    for n, k in ((128, 64), (64, 96), (96, 64)):
        bm = 128 if n % 64 == 0 else 256
        t += [lin("bf16", 2 * bm, k, n, 0, True), lin("bf16", bm + 80, k, n, 0, False, 1), lin("bf16", 16, k, n, 0, True, 1),
              lin("bf16", 16, 512, n, 0, False)]                      # M = 16 with a long K: too few rows for the LDS-DMA GEMM
    t += [lin("bf16", 208, 64, 96, 0, True, 0, 40, 70)]
    for n, k in ((128, 64), (256, 224), (64, 32), (192, 96), (96, 64), (32, 160)):
        th = 8 if n % 64 == 0 else 16
        t += [mk("conv1x1", "bf16", 2, 2 * th, 16, k, n, bias=True), mk("conv1x1", "bf16", 2, 2 * th, 17 if n % 64 else 32, k, n),
              mk("conv1x1", "bf16", 2, th + 5, 21, k, n, bias=True), mk("conv1x1", "bf16", 1, 1, 1, k, n, bias=n % 64 == 0)]
    t += [mk("conv1x1", "bf16", 2, 13, 21, 64, 96, bias=True, Lin=40, Lout=70), mk("conv1x1", "bf16", 2, 21, 11, 64, 96, Lin=40, Lout=70),
          mk("conv1x1", "bf16", 2, 16, 17, 64, 96), mk("conv1x1", "bf16", 2, 16, 16, 64, 96), mk("conv1x1", "bf16", 2, 3, 17, 64, 96, bias=True)]
    # ConvTranspose: N = 4 Cout, so Cout = 32 | 96 | 160 is N % 128 and Cout = 48-like counts do not exist (Cout % 32 == 0):
    # the N % 64 / N % 32 forms serve the data gradient only (N = Cin = 64 | 96)
    for cout in (32, 96, 160):
        t += [mk("convt_fwd", "bf16", 2, 16, 16, 64, cout, bias=True), mk("convt_fwd", "bf16", 2, 13, 21, 96, cout),
              mk("convt_fwd", "bf16", 1, 1, 1, 64, cout, bias=True)]
    t += [mk("convt_fwd", "bf16", 2, 13, 21, 64, 96, bias=True, Lin=40, Lout=70)]
    for cin in (128, 64, 96, 32):
        t += [mk("convt_dgrad", "bf16", 2, 16, 32 if cin == 96 else 17, cin, 32), mk("convt_dgrad", "bf16", 2, 21, 21, cin, 96),
              mk("convt_dgrad", "bf16", 1, 1, 1, cin, 32)]
    t += [mk("convt_dgrad", "bf16", 2, 16, 16, 96, 32), mk("convt_dgrad", "bf16", 2, 3, 17, 96, 32), mk("convt_dgrad", "bf16", 2, 21, 11, 96, 96, Lin=70, Lout=40)]
    # fp32: every shape on the generic kernel, 16 x 16 tiles up to W = 16 and 8 x 32 above
    for n, k in ((128, 64), (64, 96), (96, 64)):
        t += [lin("fp32", 512, k, n, 0, True), lin("fp32", 336, k, n, 0, False, 1), lin("fp32", 16, k, n, 0, True, 1)]
    t += [lin("fp32", 400, 768, 256, 0, True, 1), lin("fp32", 208, 64, 96, 0, True, 0, 40, 70)]
    for n, k in ((128, 32), (64, 96), (96, 64)):
        t += [mk("conv1x1", "fp32", 2, 16, 16, k, n, bias=True), mk("conv1x1", "fp32", 2, 16, 17, k, n, bias=True),
              mk("conv1x1", "fp32", 2, 16, 64, k, n), mk("conv1x1", "fp32", 2, 21, 11, k, n), mk("conv1x1", "fp32", 2, 13, 41, k, n, bias=True),
              mk("conv1x1", "fp32", 1, 1, 1, k, n, bias=True), mk("conv1x1", "fp32", 2, 3, 17, k, n)]
    t += [mk("conv1x1", "fp32", 2, 21, 11, 64, 96, bias=True, Lin=56, Lout=70), mk("conv1x1", "fp32", 2, 13, 41, 64, 96, Lin=56, Lout=70)]
    for cout in (32, 96, 160):
        t += [mk("convt_fwd", "fp32", 2, 16, 16, 32, cout, bias=True), mk("convt_fwd", "fp32", 2, 8, 32, 64, cout),
              mk("convt_fwd", "fp32", 2, 21, 11, 64, cout), mk("convt_fwd", "fp32", 2, 13, 41, 32, cout, bias=True)]
    t += [mk("convt_fwd", "fp32", 1, 1, 1, 32, 96, bias=True), mk("convt_fwd", "fp32", 2, 3, 17, 32, 32),
          mk("convt_fwd", "fp32", 2, 13, 41, 64, 96, bias=True, Lin=56, Lout=70)]
    for cin in (128, 64, 96):
        t += [mk("convt_dgrad", "fp32", 2, 16, 16, cin, 32), mk("convt_dgrad", "fp32", 2, 16, 17, cin, 32),
              mk("convt_dgrad", "fp32", 2, 21, 11, cin, 64), mk("convt_dgrad", "fp32", 2, 13, 41, cin, 32),
              mk("convt_dgrad", "fp32", 1, 1, 1, cin, 32), mk("convt_dgrad", "fp32", 2, 3, 17, cin, 32)]
    return t


def _stream_cases():
    t = []
    for cin, couts in ((128, (32, 64, 128, 256)), (256, (32, 64, 128))):          # every wave layout of the two forward instances
        for i, cout in enumerate(couts):
            t += [mk("convt_fwd", "bf16", 2, 5, 48, cin, cout, bias=i % 2 == 0), mk("convt_fwd", "bf16", 1, 1, 16, cin, cout, bias=i % 2 == 1)]
        t += [mk("convt_fwd", "bf16", 3, 7, 32, cin, 64, bias=True, Lin=cin - 24, Lout=38)]
    t += [mk("convt_dgrad", "bf16", 2, 5, 48, 128, 64), mk("convt_dgrad", "bf16", 1, 1, 16, 128, 64),
          mk("convt_dgrad", "bf16", 3, 7, 32, 128, 64, Lin=102, Lout=40)]
    return t


def _dma_cases():
    t = []
    # plain mode, BM = 256: M = 128 (the least), M = BM, M = BM + 16, ragged; K = 8 chunks (the least), 10 and 14 (no multiple of
    # the six slots), 26 (above twice the ring); through segk_linear, and through segk_conv1x1 with M no multiple of 16
    t += [lin("bf16", 128, 256, 128, 0, True), lin("bf16", 256, 320, 256, 0, False), lin("bf16", 272, 448, 128, 0, True, 1),
          lin("bf16", 1168, 832, 384, 0, True), lin("bf16", 400, 768, 256, 0, True, 1), lin("bf16", 144, 3072, 128, 0, False),
          lin("bf16", 1168, 320, 256, 0, True, 0, 296, 230)]
    t += [mk("conv1x1", "bf16", 2, 13, 21, 256, 128, bias=True), mk("conv1x1", "bf16", 2, 16, 16, 448, 256),
          mk("conv1x1", "bf16", 3, 7, 41, 320, 128, bias=True, Lin=296, Lout=102)]
    # split-K: S = 1, 2, 3, and S = 4 at K = 256, the least legal split (two chunks per unit)
    t += [lin("bf16", 256, 256, 256, 1, True), lin("bf16", 400, 384, 128, 2, True), lin("bf16", 272, 768, 256, 3, False),
          lin("bf16", 128, 256, 128, 4, True), lin("bf16", 1168, 1280, 128, 2, True), lin("bf16", 528, 576, 384, 3, True)]
    # BM = 320 (fewer rounds on NUM_CUS compute units): ragged and whole row tiles
    t += [lin("bf16", 3152, 256, 2560, 0, True), lin("bf16", 3200, 320, 2560, 0, False, 1), lin("bf16", 3152, 448, 2560, 0, True, 0, 424, 2534),
          lin("bf16", 3152, 768, 1024, 3, True), lin("bf16", 3200, 256, 1280, 2, False),
          mk("conv1x1", "bf16", 2, 8, 197, 256, 2560, bias=True)]
    # pixel-shuffle store (K >= 16 chunks): Cout = 32 | 96 | 160 put the tap boundary inside the 128-column tile
    t += [mk("convt_fwd", "bf16", 2, 8, 8, 512, 32, bias=True), mk("convt_fwd", "bf16", 1, 16, 16, 512, 96),
          mk("convt_fwd", "bf16", 2, 8, 17, 576, 160, bias=True), mk("convt_fwd", "bf16", 2, 13, 21, 832, 96, bias=True),
          mk("convt_fwd", "bf16", 2, 13, 21, 512, 96, bias=True, Lin=488, Lout=70),
          mk("convt_fwd", "bf16", 2, 8, 197, 512, 640, bias=True), mk("convt_fwd", "bf16", 2, 8, 200, 576, 640)]
    # un-shuffle gather: nchA = 2 (8 chunks, the least) and larger even counts
    t += [mk("convt_dgrad", "bf16", 2, 8, 8, 128, 64 + 0), mk("convt_dgrad", "bf16", 1, 16, 16, 256, 64),
          mk("convt_dgrad", "bf16", 2, 8, 17, 128, 128), mk("convt_dgrad", "bf16", 2, 13, 21, 384, 256),
          mk("convt_dgrad", "bf16", 2, 13, 21, 256, 192, Lin=230, Lout=168),
          mk("convt_dgrad", "bf16", 2, 8, 197, 2560, 64), mk("convt_dgrad", "bf16", 2, 8, 200, 2560, 128)]
    return t


CASES = _generic_cases() + _stream_cases() + _dma_cases()

# Three or more work units on some workgroup of a persistent kernel -- the DMA ring of gemm_dma runs through unit boundaries
# (ring slot, ring parity, the fetch cursor that runs ahead into the next unit, zero_acc), the generic kernel pre-loads the next
# unit's first chunk -- and three or more trips (an odd count, with a last round not every stream takes) round the ping-pong
# loop of convt_stream.  The two exact runs only.
LONG_CASES = [
    lin("bf16", 5776, 320, 3456, 0, True),                         # gemm_dma<0,256>
    lin("bf16", 6160, 448, 3968, 0, True),                         # gemm_dma<0,320>
    lin("bf16", 2576, 960, 2432, 3, True),                         # gemm_dma<0,256> split-K
    lin("bf16", 3152, 1344, 2560, 3, True),                        # gemm_dma<0,320> split-K
    mk("convt_fwd", "bf16", 16, 19, 19, 640, 864, bias=True),      # gemm_dma<1,256>
    mk("convt_fwd", "bf16", 5, 16, 77, 512, 992),                  # gemm_dma<1,320>
    mk("convt_dgrad", "bf16", 16, 19, 19, 3456, 128),              # gemm_dma<2,256>
    mk("convt_dgrad", "bf16", 5, 16, 77, 3968, 64),                # gemm_dma<2,320>
    mk("conv1x1", "bf16", 9, 41, 53, 64, 896, bias=True),          # generic bf16, two 4-wave workgroups per CU
    mk("conv1x1", "fp32", 18, 37, 41, 32, 384, bias=True),         # generic fp32, 8 waves
    mk("convt_fwd", "bf16", 3, 7, 32 * 113, 128, 32, bias=True),   # convt_stream<4,8,0> wpc 1
    mk("convt_fwd", "bf16", 3, 7, 16 * 29, 128, 256),              # ... wpc 8
    mk("convt_fwd", "bf16", 3, 7, 16 * 113, 256, 32),              # convt_stream<8,4,0> wpc 2
    mk("convt_fwd", "bf16", 3, 7, 16 * 29, 256, 128, bias=True),   # ... wpc 8
    mk("convt_dgrad", "bf16", 3, 7, 16 * 113, 128, 64),            # convt_stream<8,4,1>
]

PERSISTENT_FAMILIES = ("dma-0-256", "dma-0-320", "dma-1-256", "dma-1-320", "dma-2-256", "dma-2-320", "generic-bf16", "generic-fp32",
                       "stream-0", "stream-1")
