"""CPU restatements of csrc/recon.hip and the case tables of tests/test_gpu_recon_matrix.py (NumPy / torch only; nothing here
touches the library).  tests/test_recon_prompt_cases_host.py checks the restatements against torch's float64 / ATen results and
proves from the restated launch arithmetic that the tables reach what they claim.

  head          sigmoid(b + conv3x3_pad1(x)) in float64 on the operands the kernel consumes: the act tensor's values and the fp32
                weights (bf16 mode: the weights rounded to bf16), with S = sum |x| |w| + |b| per output.
  head_bound    what the device may differ by, from the reference alone:  gamma_m S / 4 + 4 d_sig.
                  gamma_m S   m = 9 Cin + 1, gamma_m = m u / (1 - m u), u = 2^-24: fp32 accumulation, in any order, of 9 Cin
                              exact (bf16 x bf16 in fp32) or once-rounded (fp32 FMA) products and the bias;
                  1 / 4       the sigmoid's largest slope;
                  d_sig       the largest distance of the float32 restatement of the sigmoid step (sigmoid32: exp, add, divide,
                              one rounding each) from float64 on the same float32 argument, over the case's outputs;
                  4           DESIGN.md 3.4's margin for the device math library against NumPy's.
  sigmoid_bwd   g * (1 - r) * r in float32, in that order, laid out [B,H,W,Cp] with zero padding, rounded to the dtype.
  mse           terms float64(float32(d * d)), d = float32(a - b); math.fsum; times the scale; rounded to float32.  The device's
                fp64 accumulation is within n 2^-53 relative of the exact sum (< 1e-9 at every n here), far under half an fp32
                ulp, so only the final rounding can differ: the gate is one float32 ulp.
  mse_bwd       (float32(norm) * (a - b)) * g in float32, norm = float32(2.0 / n) or 2; db = -da."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from oracle.fill import fill

U24 = 2.0 ** -24
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
CHUNK = {"fp32": 8, "bf16": 16}                      # channels of one staged chunk


def pad32(c):
    return (c + 31) // 32 * 32


def act(x, Cp, dtype):
    """NCHW fp32 -> the act tensor [B,H,W,Cp] in the dtype, padding channels zero"""
    B, C, H, W = x.shape
    out = torch.zeros((B, H, W, Cp), dtype=TORCH_DT[dtype])
    out[..., :C] = x.permute(0, 2, 3, 1).to(TORCH_DT[dtype])
    return out


def _operands(x_act, w, dtype):
    Cin = w.shape[1]
    x64 = x_act[..., :Cin].permute(0, 3, 1, 2).double()
    w64 = (w.to(torch.bfloat16) if dtype == "bf16" else w).double()
    return x64, w64


def head(x_act, w, b, dtype):
    """-> (rec64 [B,Cout,H,W], S, z64); b may be None"""
    x64, w64 = _operands(x_act, w, dtype)
    B, _, H, W = x64.shape
    xp = F.pad(x64, (1, 1, 1, 1))                     # the zero halo
    z = torch.zeros((B, w.shape[0], H, W), dtype=torch.float64)
    S = torch.zeros_like(z)
    for dy in range(3):                              # nine shifted channel contractions, written out
        for dx in range(3):
            win = xp[:, :, dy:dy + H, dx:dx + W]
            z += torch.einsum("bchw,oc->bohw", win, w64[:, :, dy, dx])
            S += torch.einsum("bchw,oc->bohw", win.abs(), w64[:, :, dy, dx].abs())
    if b is not None:
        z += b.double()[None, :, None, None]
        S += b.double().abs()[None, :, None, None]
    return 1.0 / (1.0 + torch.exp(-z)), S, z


def sigmoid32(z):
    """the sigmoid step as the kernel writes it, 1 / (1 + exp(-z)), in float32 with one rounding per operation"""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(-z).astype(np.float32)
        return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)


def saturation(z):
    """float32 sigmoid of a saturated argument as ATen evaluates it: exp overflows to +inf below -88.7, so the result is exactly
    0 there (the float64 value, a denormal, is never formed); exactly 1 above 17"""
    return torch.sigmoid(torch.as_tensor(np.asarray(z, dtype=np.float32))).numpy()


def gamma(m):
    return m * U24 / (1.0 - m * U24)


def d_sig(z64):
    z32 = z64.float()
    return float(np.abs(sigmoid32(z32.numpy()).astype(np.float64) - torch.sigmoid(z32.double()).numpy()).max())


def head_bound(S, z64, Cin):
    """per-output bound of |rec - rec64| (the module docstring derives it)"""
    return gamma(9 * Cin + 1) * S / 4.0 + 4.0 * d_sig(z64)


def head32(x_act, w, b, dtype):
    """the whole step in float32 (torch's CPU conv2d on the same operands, then sigmoid32)"""
    x64, w64 = _operands(x_act, w, dtype)
    z = F.conv2d(x64.float(), w64.float(), None if b is None else b.float(), padding=1)
    return torch.from_numpy(sigmoid32(z.numpy()))


def sigmoid_bwd(drec, rec, Cp, dtype):
    """NCHW fp32 -> dz [B,H,W,Cp] in the dtype"""
    f = drec.float() * (1.0 - rec.float()) * rec.float()
    return act(f, Cp, dtype)


def mse_sum(a, b):
    """the exactly rounded float64 sum of the float32 terms"""
    d = a.float().reshape(-1) - b.float().reshape(-1)
    return math.fsum((d * d).double().tolist())


def mse(a, b, mean, total=None):
    """-> float32 scalar; `total` = mse_sum(a, b) when the caller has it already"""
    n = a.numel()
    s = mse_sum(a, b) if total is None else total
    return np.float32(s * (1.0 / float(n) if mean else 1.0))


def mse_bwd(a, b, g, mean):
    """-> (da, db) float32, ATen's mse_loss_backward rounding"""
    n = a.numel()
    norm = torch.tensor(2.0 / float(n) if mean else 2.0, dtype=torch.float32)
    da = (norm * (a.float() - b.float())) * torch.tensor(g, dtype=torch.float32)
    return da, -da


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------
MSE_MAX_BLOCKS, MSE_UNROLL = 512, 8
MSE_BWD_MAX_BLOCKS = 16384


def mse_blocks(n):
    """segk_mse_blocks"""
    return min(max((n + 256 * MSE_UNROLL * 2 - 1) // (256 * MSE_UNROLL * 2), 1), MSE_MAX_BLOCKS)


def mse_passes(n):
    """-> (outer passes of mse_part_kernel's loop, elements of the last one)"""
    per = mse_blocks(n) * 256 * MSE_UNROLL
    p = (n + per - 1) // per
    return p, n - (p - 1) * per


def mse_bwd_passes(n):
    g = min((n + 255) // 256, MSE_BWD_MAX_BLOCKS)
    return (n + g * 256 - 1) // (g * 256)


def head_chunks(Cin, dtype):
    """-> (chunks, real channels of the last chunk, whether the last bf16 pair is half real)"""
    ck = CHUNK[dtype]
    n = (Cin + ck - 1) // ck
    return n, Cin - (n - 1) * ck, dtype == "bf16" and Cin % 2 == 1


# ---- case tables -----------------------------------------------------------------------------------------------------------
HeadCase = namedtuple("HeadCase", "dtype B H W Cin Cp Cout bias seed")
HEAD_SHAPES = [(1, 1, 1), (1, 7, 13), (1, 32, 32), (1, 33, 32), (1, 32, 33), (1, 31, 65), (1, 65, 31), (3, 37, 61)]
HEAD_CINS = [1, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 96]
HEAD_COUTS = [1, 2, 3, 4, 5, 8, 11]


def _head_cases():
    """Cin and Cout walk the shapes with strides of their own (5 of 13, 3 of 7): sixteen cells per dtype show every value of
    both lists, and the 1x1 and 65x31 shapes meet Cin = 1, 3 and 9, 15.  A seed is replaced here, never a bound, when the host
    test finds a case that misses an input condition."""
    out = []
    for d, dtype in enumerate(("fp32", "bf16")):
        for i in range(16):
            B, H, W = HEAD_SHAPES[i % 8]
            Cin = HEAD_CINS[(5 * i) % 13]
            out.append(HeadCase(dtype, B, H, W, Cin, pad32(Cin), HEAD_COUTS[(3 * i + d) % 7], (i + d) % 3 != 2, 500 + 40 * d + i))
        out.append(HeadCase(dtype, 1, 7, 13, 8, 64, 5, True, 590 + d))          # Cp beyond pad32(Cin)
    return out


HEAD_CASES = _head_cases()


def head_case_id(c):
    return f"{c.dtype}-{c.B}x{c.H}x{c.W}-Cin{c.Cin}-Cp{c.Cp}-Cout{c.Cout}-{'bias' if c.bias else 'nobias'}"


def head_inputs(c):
    """-> (x_act, w, b): x in [0, 1], weights scaled so that z stays O(1), bias in [-0.5, 0.5]"""
    x = fill((c.B, c.Cin, c.H, c.W), c.seed, 0, 1)
    w = fill((c.Cout, c.Cin, 3, 3), c.seed + 1000, -1, 1) * (1.0 / (3.0 * c.Cin ** 0.5))
    b = fill((c.Cout,), c.seed + 2000, -0.5, 0.5) if c.bias else None
    return act(x, c.Cp, c.dtype), w, b


SATURATION_BIASES = [40.0, -40.0, 90.0, -90.0, 104.0, -104.0]

SIGMOID_BWD_SHAPES = [(1, 1, 1), (1, 5, 51), (1, 16, 16), (1, 257, 1), (3, 5, 7)]       # 1, 255, 256, 257 pixels; 3 x 35
SIGMOID_BWD_CHANNELS = [(1, 32), (3, 32), (4, 32), (5, 32), (8, 32), (9, 32), (11, 32), (33, 64), (3, 64)]    # (C, Cp)

# 511 * 4096 is the one n that launches 511 workgroups (511 * 4096 + 1 already launches the cap of 512)
MSE_FWD_N = [1, 7, 255, 256, 257, 4095, 4096, 4097, 256 * 4096, 256 * 4096 + 1, 511 * 4096, 511 * 4096 + 1, 512 * 4096,
             512 * 4096 + 1, 3 * 512 * 4096 + 5]
MSE_BWD_N = [n for n in MSE_FWD_N if n <= 512 * 4096 + 1] + [MSE_BWD_MAX_BLOCKS * 256 + 3]
MSE_GOUTS = [1.0, 0.75, -2.0, 0.0]


def mse_bwd_options(i):
    """(g, mean, db present) of the i-th n: the upstream gradient, the reduction and db walk the n values with strides of their
    own; the two largest n (the last block boundary and the grid stride) take every g"""
    gs = MSE_GOUTS if MSE_BWD_N[i] >= 512 * 4096 + 1 else [MSE_GOUTS[i % 4], MSE_GOUTS[(i + 1) % 4]]
    return [(g, (i + j) % 2, (i + j // 2) % 2 == 0) for j, g in enumerate(gs)]


MSE_MAX_N = max(MSE_FWD_N + MSE_BWD_N)


@lru_cache(maxsize=None)
def mse_master():
    """one input pair for every n: the cases are its prefixes"""
    return fill((MSE_MAX_N,), 11, 0, 1), fill((MSE_MAX_N,), 12, 0, 1)


@lru_cache(maxsize=None)
def mse_master_sum(n):
    a, b = mse_master()
    return mse_sum(a[:n], b[:n])
