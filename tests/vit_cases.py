"""Case tables of the ViT / bilinear matrix (tests/test_gpu_vit_matrix.py runs them on the GPU, tests/test_vit_cases_host.py
proves on the CPU that every regime named below is populated) and a Python restatement of the launch arithmetic of the ten
entries of csrc/vit.hip and of the two bilinear entries of csrc/resize.hip.  Plain Python, no torch.

  attention_kernel<T, HD> (fp32/64, fp32/32, bf16/32): grid (ceil(T / 64), B * heads) x 256 threads; a lane is one query, wave w
      takes the key groups (4 keys) w, w + 4, ...; K and V of the head in LDS, Tp = T rounded up to 4, the cross-wave merge
      overlays them ([4][HD + 2][64] floats).
  attention_mfma_kernel (bf16/64): grid (ceil(T / 128), B * heads) x 256; a wave is 32 queries and walks Tp / 32 key blocks,
      Tp = T rounded up to 32; LDS K [Tp][144 B] + V^T [64][2 Tp + 16 B].
  add_layernorm: a wave per row, 4 rows per block, a lane owns float4 number lane + 64 i of the row.
  vit_embed_ln: a wave per token row, a lane owns channel lane + 64 i.
  vit_patchify / vit_tokens_to_grid / bilinear_*: an item per thread behind a capped grid, grid-stride loop."""
from collections import namedtuple

LDS_LIMIT = 160 * 1024
LN_MAX_D = 2048                 # 64 lanes x LN_MAXPER = 32 channels
MOVE_GRID_CAP = 16384           # vit_patchify, vit_tokens_to_grid, the two passes of the separable bilinear backward
BILINEAR_GRID_CAP = 8192        # bilinear_fwd, the 2-D gather backward
REF_COST_CAP = 2 * 10 ** 9      # float64 reference on the CPU: multiply-adds (attention, bilinear) or elements per case


def cdiv(a, b):
    return -(-a // b)


def pad32(n):
    return (n + 31) // 32 * 32


def esize(dtype):
    return 2 if dtype == "bf16" else 4


# ---- attention -------------------------------------------------------------------------------------------------------------
AttnCase = namedtuple("AttnCase", "dtype hd B T heads wide")     # wide: pitches (3D + 8, D + 8) instead of (3D, D)
ATTN_INSTANCES = [("fp32", 64), ("fp32", 32), ("bf16", 32), ("bf16", 64)]
ATTN_DESIGNS = ("routed", "uniform", "ramp_up", "ramp_down", "dense")


def attn_is_mfma(c):
    return c.dtype == "bf16" and c.hd == 64


def attn_pitches(c):
    D = c.heads * c.hd
    return (3 * D + 8, D + 8) if c.wide else (3 * D, D)


def attn_args_ok(c, ldq=None, ldo=None):
    """the SEGK_REQUIRE lines of segk_attention but the LDS one"""
    lq, lo = attn_pitches(c)
    ldq, ldo = lq if ldq is None else ldq, lo if ldo is None else ldo
    D = c.heads * c.hd
    return (c.B > 0 and c.T > 0 and c.heads > 0 and c.hd in (32, 64) and ldq >= 3 * D and ldo >= D and ldq % 8 == 0
            and ldo % 8 == 0 and c.B * c.heads <= 65535)


def attn_tp(c):
    return (c.T + 31) & ~31 if attn_is_mfma(c) else (c.T + 3) & ~3


def valu_overlay_bytes(hd):
    return 4 * (hd + 2) * 64 * 4


def valu_kv_bytes(c):
    return 2 * attn_tp(c) * c.hd * esize(c.dtype)


def attn_lds(c):
    if attn_is_mfma(c):
        Tp = attn_tp(c)
        return Tp * 144 + 64 * (Tp * 2 + 16)
    return max(valu_kv_bytes(c), valu_overlay_bytes(c.hd))


def attn_served(c):
    return attn_args_ok(c) and attn_lds(c) <= LDS_LIMIT


def attn_max_t(dtype, hd):
    T = 1
    while attn_served(AttnCase(dtype, hd, 1, T + 1, 1, 0)):
        T += 1
    return T


def attn_query_blocks(c):
    return cdiv(c.T, 128 if attn_is_mfma(c) else 64)


def valu_wave_trips(c):
    """key groups each of the four waves walks"""
    groups = cdiv(c.T, 4)
    return [len(range(w, groups, 4)) for w in range(4)]


def valu_last_block_queries(c):
    return c.T - 64 * (attn_query_blocks(c) - 1)


def mfma_key_blocks(c):
    return attn_tp(c) >> 5


def mfma_last_block_waves(c):
    """queries of the four waves of the last query block (0: the wave leaves after the barrier)"""
    q0 = 128 * (attn_query_blocks(c) - 1)
    return [max(0, min(32, c.T - (q0 + 32 * w))) for w in range(4)]


def attn_acc_trips(c):
    """most trips of the key loop of one wave: what the accumulation term of the bound counts"""
    return mfma_key_blocks(c) if attn_is_mfma(c) else max(valu_wave_trips(c))


def attn_cost(c):
    return c.B * c.heads * c.T * c.T * c.hd


def attn_case_id(c):
    return f"{c.dtype}-hd{c.hd}-B{c.B}-T{c.T}-h{c.heads}" + ("-wide" if c.wide else "")


VALU_T = [1, 3, 5, 7, 20, 64, 65, 197]       # boundary sizes at B = 1, heads = 1, pitches (3D, D); + the instance's largest T
MFMA_T = [1, 5, 31, 32, 33, 40, 63, 65, 128, 129, 197, 257, 576]
_MULTI_VALU = [(2, 20, 3, 1), (2, 65, 1, 0), (1, 7, 3, 1), (2, 197, 3, 1)]                # (B, T, heads, wide)
_MULTI_MFMA = [(2, 40, 3, 1), (2, 129, 1, 0), (1, 33, 3, 1), (2, 197, 3, 1)]
ATTN_CASES = []
for _dt, _hd in ATTN_INSTANCES:
    _mf = _dt == "bf16" and _hd == 64
    _ts = MFMA_T if _mf else VALU_T + [attn_max_t(_dt, _hd)]
    ATTN_CASES += [AttnCase(_dt, _hd, 1, _t, 1, 0) for _t in _ts]
    ATTN_CASES += [AttnCase(_dt, _hd, _b, _t, _h, _w) for _b, _t, _h, _w in (_MULTI_MFMA if _mf else _MULTI_VALU)]

# routed design: key j carries the +-1 code of its ROUTED_BITS index bits, repeated routed_reps(hd) times; the last head
# dimension is the shift
ROUTED_BITS = 11


def routed_reps(hd):
    return (hd - 1) // ROUTED_BITS


def routed_target(i, T):
    """pi(i): query 0 looks at the last key, the stride is coprime with T, so every key (the first one too) is a target"""
    from math import gcd
    st = 5
    while gcd(st, T) != 1:
        st += 2
    return (T - 1 - i * st) % T


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
LnCase = namedtuple("LnCase", "dtype M D Dp nparts loose")       # loose: part_stride > M * Dp
LN_FORMS = ("add_ln", "add_only", "ln_only")
LN_DESIGNS = ("lattice", "constant", "offset", "dense")


def ln_served(D, Dp, M=1, nparts=1, part_stride=0):
    return (M > 0 and nparts >= 1 and (nparts == 1 or part_stride >= M * Dp) and 0 < D <= LN_MAX_D and Dp >= D and D % 4 == 0
            and Dp % 4 == 0)


def ln_blocks(M):
    return cdiv(M, 4)


def ln_idle_waves(M):
    return 4 * ln_blocks(M) - M


def ln_nq(D):
    return D >> 2


def ln_per4(D):
    """float4 per lane (the busiest lane)"""
    return cdiv(ln_nq(D), 64)


def ln_part_stride(c):
    return c.M * c.Dp + (64 if c.loose else 0)


def ln_case_id(c):
    return f"{c.dtype}-M{c.M}-D{c.D}-Dp{c.Dp}-p{c.nparts}" + ("-loose" if c.loose else "")


LN_CASES = []
for _dt in ("fp32", "bf16"):
    for _i, _D in enumerate((4, 12, 100, 768, 2048)):
        for _j, _M in enumerate((1, 5, 33)):
            _np = (1, 2, 3)[(_i + _j) % 3]
            LN_CASES.append(LnCase(_dt, _M, _D, _D + 4 * ((_i + _j) % 2), _np, int(_np > 1 and (_i + 2 * _j) % 2 == 0)))
    LN_CASES += [LnCase(_dt, 5, 768, 768, 3, 1), LnCase(_dt, 33, 100, 104, 2, 0), LnCase(_dt, 5, 12, 16, 1, 0)]

EmbedCase = namedtuple("EmbedCase", "dtype B T D Dp")
EMBED_DESIGNS = ("lattice", "constant", "offset", "dense")


def embed_served(B, T, D, Dp):
    return B > 0 and T > 1 and 0 < D <= LN_MAX_D and Dp >= D


def embed_per(D):
    return cdiv(D, 64)


def embed_case_id(c):
    return f"{c.dtype}-B{c.B}-T{c.T}-D{c.D}-Dp{c.Dp}"


EMBED_CASES = []
for _dt in ("fp32", "bf16"):
    EMBED_CASES += [EmbedCase(_dt, 1, 2, 32, 32), EmbedCase(_dt, 3, 5, 96, 128), EmbedCase(_dt, 1, 197, 768, 768),
                    EmbedCase(_dt, 3, 2, 2048, 2080), EmbedCase(_dt, 3, 197, 96, 96), EmbedCase(_dt, 1, 5, 768, 800),
                    EmbedCase(_dt, 3, 5, 32, 64), EmbedCase(_dt, 1, 5, 2048, 2048)]


# ---- pure movement ---------------------------------------------------------------------------------------------------------
PatchCase = namedtuple("PatchCase", "dtype B C H W ps Kp")


def patch_served(c):
    return (c.B > 0 and c.C > 0 and c.ps > 0 and c.H >= c.ps and c.W >= c.ps and c.H // c.ps == c.W // c.ps
            and c.Kp >= c.C * c.ps * c.ps and c.Kp % 32 == 0)


def patch_items(c):
    G = c.H // c.ps
    return c.B * G * G * c.Kp


def move_grid(items):
    return min(cdiv(items, 256), MOVE_GRID_CAP)


def move_trips(items, cap=MOVE_GRID_CAP):
    return cdiv(items, min(cdiv(items, 256), cap) * 256)


def patch_case_id(c):
    return f"{c.dtype}-{c.B}x{c.C}x{c.H}x{c.W}-ps{c.ps}-Kp{c.Kp}"


_PATCH = [(2, 3, 32, 32, 16, 768), (2, 3, 28, 28, 14, 608), (1, 1, 64, 64, 32, 1024), (2, 2, 30, 31, 14, 416),
          (1, 3, 32, 32, 16, 800), (1, 3, 1184, 1184, 16, 768)]
PATCH_CASES = [PatchCase(dt, *s) for dt in ("fp32", "bf16") for s in _PATCH]

GridCase = namedtuple("GridCase", "dtype B T D Dp")


def grid_served(c):
    return c.B > 0 and c.T > 1 and c.D > 0 and c.Dp >= c.D and c.Dp % 32 == 0


def grid_items(c):
    return c.B * (c.T - 1) * c.Dp


def grid_case_id(c):
    return f"{c.dtype}-B{c.B}-T{c.T}-D{c.D}-Dp{c.Dp}"


_GRID = [(2, 2, 32, 32), (1, 2, 96, 128), (2, 197, 768, 768), (1, 197, 768, 800), (27, 197, 768, 800)]
GRID_CASES = [GridCase(dt, *s) for dt in ("fp32", "bf16") for s in _GRID]


# ---- bilinear --------------------------------------------------------------------------------------------------------------
BilCase = namedtuple("BilCase", "dtype B C Cp IH IW OH OW")


def bil_served(c):
    return c.B > 0 and c.IH > 0 and c.IW > 0 and c.OH > 0 and c.OW > 0 and c.Cp > 0 and c.Cp % 32 == 0


def bil_cv(c):
    return c.Cp // (8 if c.dtype == "bf16" else 4)


def bil_items(c, kernel):
    """kernel: "fwd" (an item per output pixel), "bwd2d" and "sep_y" (per input pixel), "sep_x" (per OH x IW pixel)"""
    px = {"fwd": c.OH * c.OW, "bwd2d": c.IH * c.IW, "sep_y": c.IH * c.IW, "sep_x": c.OH * c.IW}[kernel]
    return c.B * px * bil_cv(c)


def bil_cap(kernel):
    return BILINEAR_GRID_CAP if kernel in ("fwd", "bwd2d") else MOVE_GRID_CAP


def bil_trips(c, kernel):
    return move_trips(bil_items(c, kernel), bil_cap(kernel))


def bil_ops_form(c):
    """the form ops.BilinearFn.backward picks: separable when the map grows by more than 4x in area"""
    return "separable" if c.OH * c.OW > 4 * c.IH * c.IW else "gather"


def bil_scratch_floats(c):
    return c.B * c.OH * c.IW * c.Cp


def bil_exact(c):
    """up-scaling by 1, 2 or 4 (14 -> 28, 14 -> 56, 3 x 5 -> 6 x 10, the identity): the weights are multiples of 1/8, lattice
    inputs give results that are exact in fp32"""
    return all(o % i == 0 and (o // i) & (o // i - 1) == 0 and o // i <= 4 for i, o in ((c.IH, c.OH), (c.IW, c.OW)))


def bil_cost(c):
    return c.B * c.Cp * max(c.IH * c.IW * c.OH, c.OH * c.OW * c.IW)


def bil_case_id(c):
    return f"{c.dtype}-{c.B}x{c.C}({c.Cp})-{c.IH}x{c.IW}-{c.OH}x{c.OW}"


_BIL = [(2, 32, 32, 14, 14, 28, 28), (1, 32, 32, 14, 14, 56, 56), (1, 32, 32, 14, 14, 224, 224), (2, 32, 32, 7, 7, 10, 13),
        (2, 40, 64, 3, 5, 6, 10), (2, 32, 32, 1, 1, 5, 7), (2, 32, 32, 5, 9, 1, 1), (1, 64, 64, 8, 8, 8, 8),
        (2, 32, 32, 16, 12, 4, 3)]
BIL_SMALL = [BilCase(dt, *s) for dt in ("fp32", "bf16") for s in _BIL]
# the smallest shapes with a second trip behind each cap at Cp = 32, in both dtypes: the item count is pixels x Cp / 4 (fp32)
# or Cp / 8 (bf16), so a bf16 case needs twice the pixels (non-square: the other side of the resize stays tiny)
BIL_STRIDE = [BilCase("fp32", 1, 32, 32, 2, 3, 257, 1021),     # forward: 262397 x 8 items > 8192 x 256
              BilCase("bf16", 1, 32, 32, 2, 3, 513, 1023),     # forward: 524799 x 4 items
              BilCase("fp32", 1, 32, 32, 257, 1021, 2, 3),     # 2-D gather backward
              BilCase("bf16", 1, 32, 32, 513, 1023, 2, 3),     # 2-D gather backward
              BilCase("fp32", 1, 32, 32, 513, 1023, 2, 3),     # separable pass 2 (per input pixel): 524799 x 8 > 16384 x 256
              BilCase("bf16", 1, 32, 32, 1026, 1023, 4, 3),    # separable pass 2: 1049598 x 4 items (1026 / 4: lambda is not 0)
              BilCase("fp32", 1, 32, 32, 2, 1023, 513, 3),     # separable pass 1 (per OH x IW pixel)
              BilCase("bf16", 1, 32, 32, 2, 1023, 1026, 3)]    # separable pass 1: 1049598 x 4 items, 128 MiB of fp32 scratch
BIL_SCRATCH_CAP = 160 * 2 ** 20  # bytes of the separable form's scratch a case may ask for
BIL_CASES = BIL_SMALL + BIL_STRIDE
