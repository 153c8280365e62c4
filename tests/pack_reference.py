"""Restatements of the data-carrying kernels of csrc/pack.hip (tests/test_gpu_pack_matrix.py compares the device with them,
tests/test_pack_cases_host.py checks them on the CPU by identities that do not share their indexing).

Written from the layout statements of include/segk.h, as a SCATTER: every element of the source parameter computes where it
lands and is stored into a zero array.  The kernels gather (one thread per destination element works out which source element
it wants), so the two directions cannot share an index mistake.

  packed weight     [Kp / CH][taps][Np][CH], CH = 16 (fp32) or 32 (bf16): element (k, tap, n) of the GEMM operand B[k][n] of
                    that tap sits at [k // CH][tap][n][k % CH].
  Conv2d, mode 0    k = place of input channel ci among the padded channels of the two sources (below), n = co
  Conv2d, mode 1    k = co, n = place of ci, tap -> taps - 1 - tap (the data gradient is the correlation with the flipped
                    kernel, in and out swapped)
  dual source       ci < CA sits at ci, ci >= CA at CAp + (ci - CA); every other place is padding (zero)
  ConvT, mode 0     k = ci, n = q * Coutp + co (q = 2 i + j, the 2x2 tap): one GEMM makes the four taps of an input pixel
  ConvT, mode 1     k = q * Coutp + co, n = ci: the data gradient gathers the four output pixels of an input pixel
  bias              fp32 [reps][Coutp], reps == 0 meaning 4
  activation        NHWC [B][H][W][Cp], channels >= C are +0

bf16 values are torch's CPU `.to(torch.bfloat16)` (round to nearest even); every comparison with the device is on bit
patterns (`bits`), so -0.0 and the direction of a tie count.

Reductions.  segk_wgrad_reduce adds S fp32 slabs either in slab order (S <= 16: S - 1 roundings) or as 16 interleaved streams
of ceil(S / 16) slabs whose sums are then added in lane order (15 more roundings); each rounding moves the running sum by at
most U = 2^-24 of its magnitude, which never exceeds sum_s |slab_s| (to first order in U, as tests/stem_pool_reference.py
states it):
    |device - exact| <= max(S - 1, ceil(S / 16) + 15) * U * sum_s |slab_s|
The column sums are accumulated in float64 (rows - 1 roundings of 2^-53 each, bounded by rows * 2^-53 * sum |x|) and rounded
once to fp32 (2^-24 |sum|)."""
import torch

U = 2.0 ** -24
CH = {"fp32": 16, "bf16": 32}
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
BITS_DT = {"fp32": torch.int32, "bf16": torch.int16}


def pad32(c):
    return (c + 31) // 32 * 32


def bits(t):
    """the bit patterns of a float32 / bfloat16 tensor"""
    return t.contiguous().view(BITS_DT["fp32" if t.dtype == torch.float32 else "bf16"])


# ---- values ----------------------------------------------------------------------------------------------------------------
TIES = (1 + 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8), -0.0)   # bf16: down, down, up, up (to even)


def special_values(shape, seed):
    """fp32 values for parameters and activations: seeded normal values; every 7th element (from index 3, or the last of a shorter tensor) is an exact bf16
    tie -- 1 + 2^-8 lies midway between 1 and 1 + 2^-7 and rounds to the even 1, 1 + 3 * 2^-8 midway between 1 + 2^-7 and
    1 + 2^-6 and rounds up to the even 1 + 2^-6 -- or its negative, or -0.0"""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    x = torch.randn((n,), generator=g, dtype=torch.float32)
    idx = torch.arange(min(3, n - 1), n, 7)
    x[idx] = torch.tensor(TIES, dtype=torch.float32)[(idx // 7 + seed) % len(TIES)]
    return x.reshape(shape)


# ---- packed weights --------------------------------------------------------------------------------------------------------
def _place(ci, CA, CAp):
    """where logical input channel ci sits among the padded channels of the two sources"""
    return torch.where(ci < CA, ci, CAp + (ci - CA))


def _chunked(Kp, taps, Np, dtype):
    assert Kp % CH[dtype] == 0, (Kp, dtype)
    return torch.zeros((Kp // CH[dtype], taps, Np, CH[dtype]), dtype=torch.float32)


def pack_conv(w, CA, CB, Coutp, CAp, CBp, taps, mode, dtype):
    """Conv2d weight [Cout][CA + CB][taps...] fp32 -> [Kp / CH][taps][Np][CH] in `dtype`"""
    Cout = w.shape[0]
    w = w.reshape(Cout, CA + CB, taps)
    ch = CH[dtype]
    co, ci, tap = torch.meshgrid(torch.arange(Cout), torch.arange(CA + CB), torch.arange(taps), indexing="ij")
    at = _place(ci, CA, CAp)
    if mode == 0:
        out = _chunked(CAp + CBp, taps, Coutp, dtype)
        out[at // ch, tap, co, at % ch] = w
    else:
        out = _chunked(Coutp, taps, CAp + CBp, dtype)
        out[co // ch, taps - 1 - tap, at, co % ch] = w
    return out.to(TORCH_DT[dtype])


def pack_convt(w, Cinp, Coutp, mode, dtype):
    """ConvTranspose2d(k=2, s=2) weight [Cin][Cout][2][2] fp32 -> [Kp / CH][1][Np][CH] in `dtype`"""
    Cin, Cout = w.shape[0], w.shape[1]
    ch = CH[dtype]
    ci, co, i, j = torch.meshgrid(torch.arange(Cin), torch.arange(Cout), torch.arange(2), torch.arange(2), indexing="ij")
    col = (2 * i + j) * Coutp + co
    zero = torch.zeros_like(ci)
    if mode == 0:
        out = _chunked(Cinp, 1, 4 * Coutp, dtype)
        out[ci // ch, zero, col, ci % ch] = w
    else:
        out = _chunked(4 * Coutp, 1, Cinp, dtype)
        out[col // ch, zero, ci, col % ch] = w
    return out.to(TORCH_DT[dtype])


def pack_bias(b, reps, Coutp):
    """bias [Cout] -> fp32 [reps][Coutp]; reps == 0 means 4"""
    out = torch.zeros((reps if reps > 0 else 4, Coutp), dtype=torch.float32)
    out[:, :b.numel()] = b
    return out


def read_packed(p, k, tap, n):
    """what a consumer of a packed weight reads as B[k][n] of `tap` (float64)"""
    ch = p.shape[3]
    return p[k // ch, tap, n, k % ch].double()


# ---- activations -----------------------------------------------------------------------------------------------------------
def to_nhwc(x, Cp, dtype):
    """NCHW fp32 [B,C,H,W] -> NHWC [B,H,W,Cp] in `dtype`, padding channels +0"""
    B, C, H, W = x.shape
    out = torch.zeros((B, H, W, Cp), dtype=torch.float32)
    b, c, h, w = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(H), torch.arange(W), indexing="ij")
    out[b, h, w, c] = x
    return out.to(TORCH_DT[dtype])


def to_nchw(x, C):
    """NHWC [B,H,W,Cp] -> NCHW fp32 [B,C,H,W]"""
    B, H, W, Cp = x.shape
    out = torch.zeros((B, C, H, W), dtype=torch.float32)
    b, h, w, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    out[b, c, h, w] = x[..., :C].float()
    return out


# ---- reductions ------------------------------------------------------------------------------------------------------------
def _logical(t, N, CA, CB, CAp):
    """[Np][taps][Kp] -> the logical [N][CA + CB][taps]"""
    keep = torch.cat([torch.arange(CA), CAp + torch.arange(CB)])
    return t[:N][:, :, keep].permute(0, 2, 1).contiguous()


def reduce_exact(slabs, N, CA, CB, CAp, CBp, taps):
    """slabs [S][Np][taps][CAp + CBp] -> float64 [N][CA + CB][taps]"""
    assert slabs.dim() == 4 and slabs.shape[2] == taps and slabs.shape[3] == CAp + CBp
    return _logical(slabs.sum(0, dtype=torch.float64), N, CA, CB, CAp)


def reduce_bound(slabs, N, CA, CB, CAp, CBp, taps):
    """bound of |segk_wgrad_reduce - reduce_exact| (module docstring), float64 [N][CA + CB][taps]"""
    S = slabs.shape[0]
    return max(S - 1, -(-S // 16) + 15) * U * _logical(slabs.abs().sum(0, dtype=torch.float64), N, CA, CB, CAp)


def colsum_exact(part, col0, ncols):
    """part [rows][Ctot][2] -> float64 [ncols]: the sums of the FIRST float of columns col0 .. col0 + ncols - 1"""
    return part[:, col0:col0 + ncols, 0].sum(0, dtype=torch.float64)


def colsum_bound(part, col0, ncols):
    x = part[:, col0:col0 + ncols, 0]
    return U * x.sum(0, dtype=torch.float64).abs() + part.shape[0] * 2.0 ** -53 * x.abs().sum(0, dtype=torch.float64)
