"""float64 restatements and derived bounds for the stem kernels (csrc/stem.hip), the 2x2 pooling kernels and the
BN-statistics finalisation (csrc/bn_pool.hip): the inputs and references of tests/test_gpu_stem_pool_matrix.py.  CPU torch
only; nothing here is taken from what the kernels return.  U = 2^-24 is the unit roundoff of fp32.

Stem forward.  The kernel rounds the fp32 image and the fp32 OIHW parameter to bf16 (round to nearest even: rne_bf16), forms
z = sum of K = 9 Cin exact products in fp32 inside ONE MFMA, stores bf16(z) and adds z and z^2 (of the fp32 accumulator) to
the BatchNorm partials.
    dense z:     |got - z| <= e + half a bf16 ulp,   e = K * U * A,  A = sum |w| |x|            (K roundings at most)
    statistics:  a lane adds its n_l = ceil(nblk / step) blocks in a register (one rounding per add, the square is fused), then
                 4 DPP adds over the 16 pixel lanes, then 8 waves in fp32, then the rows in float64:
                 |sum   - sum z|   <= sum e + (n_l + 4 + 8 + 4) * U * sum (|z| + e)
                 |sumsq - sum z^2| <= sum e (2 |z| + e) + (n_l + 4 + 8 + 4) * U * sum (|z| + e)^2
                 (the last 4 as in bn_reference.sum_bound: float64 stage, slack for second-order terms).

Stem weight gradient, dW[n][k] = sum over pixels dz[p][n] * col[p][k].  Products of two bf16 values are exact in fp32.  A
wave adds 16 products per MFMA step into the accumulator, one step per trip: at most 16 * T roundings over its T trips; the
eight waves of a workgroup add up in a tree of depth 3; the S slabs are added in float64 on the host (no rounding that
counts) or in fp32 by segk_wgrad_reduce (S - 1 adds in slab order, or 16 streams of ceil(S / 16) adds and 15 more):
    |slab sum (float64) - dW| <= (16 T + 3 + 2) * U * sum |dz| |col|
    |segk_wgrad_reduce  - dW| <= (16 T + 3 + 2 + max(S - 1, ceil(S / 16) + 15)) * U * sum |dz| |col|
(the 2: slack for second-order terms).  T grows with the image, so the dense run keeps to one and two trips; the lattice run
is exact at any T.

Pooling: forward, backward and the fused apply + pool are restated exactly.  The fused backward + BatchNorm-reduce form
(segk_maxpool2x2_bwd_bnstat) returns partial rows of sum g and sum g * xhat with g = dx where y > 0 and
    xhat = y * xa + xb,  xa = rstd / scale,  xb = -shift * xa - mean * rstd          (channels recovered from y)
    xhat = (z - mean) * rstd                                                          (channels of a from_z thread)
evaluated in fp32.  With XA, T1 = shift * XA, T2 = mean * rstd the exact values: xa is off by at most 4 U |XA| (a division of
up to 2 ulp), xb by 6 U |T1| + 2 U |T2| (xa's error, two products, one subtraction), the fused multiply-add by
U |xhat| <= U (|y XA| + |T1| + |T2|):  |xhat_kernel - xhat| <= U (5 |y XA| + 7 |T1| + 3 |T2|) =: d;  from z: 3 U |xhat|.
A thread adds the 4 pixels of each of its n_t items (n_t trips of the grid-stride loop), thread cv of the block then the
256 / CV threads that share its channels, the rows are added in float64:
    |sum g      - ref| <= (4 n_t + 256 / CV + 4) * U * sum |g|
    |sum g xhat - ref| <= sum |g| d + (4 n_t + 256 / CV + 4) * U * sum |g| (|xhat| + d)
These two hold for the addends the kernel takes (the `*_kernel` sums of stat_reference).  With `accumulate` the main pass
adds G = fl32(dx0 + routed), the value it is about to round to the dtype, while the from_z re-walk reads the stored dx back:
sum g is the sum of G on every channel, sum g xhat the sum of G xhat on the channels recovered from y and of dx xhat on the
from_z channels.  In fp32, and without accumulate, G == dx and nothing changes.  In bf16 with accumulate every addend differs
from the stored one by its rounding, |G - dx| <= half a bf16 ulp of dx, which the chain above does not contain (a first
version of these bounds left it out, and the stored sum lay far outside them; G is the exact gradient rounded once to fp32 and
dx the same rounded once more, so it was the derivation that was wrong, not the kernel).  Against the sums of the
STORED gradient the bounds therefore grow by exactly what that rounding moved, known from the references alone:
    sum |G - dx|   and   sum |G - dx| (|xhat| + d)          (zero in fp32 and without accumulate).
The test asserts both: the kernel's addends within the chain bound (the sharp one: a dropped or doubled item shows), the
stored gradient within the grown one.
Against the TRUE sum g (z - mean) rstd the channels recovered from y add what the rounding of the stored y costs:
sum |g| * half_ulp(y) * |rstd / scale|.

BN finalisation (training): the rows are added in float64 (error e_s <= 2 MT 2^-53 sum |row|), mean and rstd are rounded
once to fp32:  e_mean = U |mean| + e_s1 / count;  e_var = e_s2 / count + 2 |mean| e_s1 / count + 2^-50 (s2 / count + mean^2);
e_rstd = U rstd + rstd^3 e_var / 2;  e_scale = U |scale| + |gamma| e_rstd;  e_shift = |scale| e_mean + |mean| e_scale +
U (|beta| + 2 |mean scale|);  the running statistics are four fp32 operations on top: 4 U (|(1 - m) r| + |m v|) + m e_v.
Eval: rstd = 1 / sqrtf(rvar + eps) is three fp32 operations (add, square root, division of up to 2 ulp): 6 U rstd."""
import zlib

import torch

from bn_reference import U24, apply_reference, half_ulp
from conv_reference import channel_stats, conv3x3
from stem_pool_cases import (cdiv, pool_trips, pool_vec, stat_degenerate_channels, stem_blocks_per_wave, stem_lattice_density,
                             stem_wgrad_slabs, stem_wgrad_trips)

TORCH_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
U53 = 2.0 ** -53


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _uniform(g, shape, lo, hi):
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def rne_bf16(x):
    """fp32 -> the nearest bf16 value, ties to even, as fp32 (finite inputs): the upper 16 bits after adding 0x7FFF + bit 16"""
    b = x.contiguous().view(torch.int32)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & ~0xFFFF
    return r.view(torch.float32)


# ---- stem forward ----------------------------------------------------------------------------------------------------------
def stem_inputs(c, run, probes=None):
    """(x [B,Cin,H,W] fp32, w [64,Cin,3,3] fp32) of one run; impulse: probes = one group of stem_probe_passes, probe i sits in
    input channel i % Cin"""
    g = _gen("stem", run, tuple(c))
    shape = (c.B, c.Cin, c.H, c.W)
    if run == "impulse":
        w = _ints(g, (64, c.Cin, 3, 3), -64, 64) / 64
        w[w == 0] = 0.5                                          # every weight is told apart from "no probe reaches the pixel"
        x = torch.zeros(shape)
        for i, (b, y, xx) in enumerate(probes):
            x[b, i % c.Cin, y, xx] = 1.0
    elif run == "lattice":
        w = _ints(g, (64, c.Cin, 3, 3), -2, 2)
        keep = torch.rand(shape, generator=g) < 1.5 * stem_lattice_density(c)
        x = _ints(g, shape, -1, 1) * keep
    else:
        w = _uniform(g, (64, c.Cin, 3, 3), -1, 1)
        x = _uniform(g, shape, -1, 1)
    return x, w


def stem_reference(x, w):
    """z [B,H,W,64] float64 of the bf16-rounded operands"""
    return conv3x3(rne_bf16(x).double().permute(0, 2, 3, 1).contiguous(), rne_bf16(w).double())


def stem_abs_reference(x, w):
    return conv3x3(rne_bf16(x).double().abs().permute(0, 2, 3, 1).contiguous(), rne_bf16(w).double().abs())


def stem_impulse_expected(c, w, probes):
    """z [B,H,W,64] float64: probe i (channel i % Cin) leaves w[:, ci, ty, tx] at pixel (y - ty + 1, x - tx + 1)"""
    wb = rne_bf16(w).double()
    z = torch.zeros((c.B, c.H, c.W, 64), dtype=torch.float64)
    hit = torch.zeros((c.B, c.H, c.W), dtype=torch.bool)
    for i, (b, y, x) in enumerate(probes):
        for ty in range(3):
            for tx in range(3):
                oy, ox = y - ty + 1, x - tx + 1
                if 0 <= oy < c.H and 0 <= ox < c.W:
                    assert not hit[b, oy, ox], "two probes of one pass reach one output pixel"
                    z[b, oy, ox] = wb[:, i % c.Cin, ty, tx]
                    hit[b, oy, ox] = True
    return z


def stem_xn(x):
    """the padded NHWC bf16 copy of the input [B,H,W,32]: Cin rounded channels, zeros behind"""
    B, Cin, H, W = x.shape
    xn = torch.zeros((B, H, W, 32), dtype=torch.float32)
    xn[..., :Cin] = rne_bf16(x).permute(0, 2, 3, 1)
    return xn.to(torch.bfloat16)                                 # exact: the values are bf16 already


def stem_dense_bounds(c, z, A):
    """(per-element bound of the stored z, bound of the per-channel sum, of the sum of squares): module docstring"""
    e = 9 * c.Cin * U24 * A
    zb = e + half_ulp(z.abs() + e, torch.bfloat16)
    k = stem_blocks_per_wave(c) + 4 + 8 + 4
    za, e2, zz = (z.abs() + e).reshape(-1, 64), e.reshape(-1, 64), z.abs().reshape(-1, 64)
    return zb, e2.sum(0) + k * U24 * za.sum(0), (e2 * (2 * zz + e2)).sum(0) + k * U24 * (za * za).sum(0)


def lattice_is_exact(z):
    """every z an integer below 256 (exact in bf16); per channel sum |z| and sum z^2 below 2^24 (every partial sum in fp32 is
    exact, in any order)"""
    zz = z.double().reshape(-1, z.shape[-1])
    return bool((zz == zz.round()).all() and (zz.abs() < 256).all() and (zz.abs().sum(0) < 2 ** 24).all()
                and ((zz * zz).sum(0) < 2 ** 24).all())


# ---- stem weight gradient --------------------------------------------------------------------------------------------------
def stem_wgrad_inputs(c, run, probes=None):
    """(x [B,Cin,H,W] fp32, dz [B,H,W,64] bf16); impulse: dz holds 1.0 in channel n at probes[n]"""
    g = _gen("stem-wgrad", run, tuple(c))
    shape = (c.B, c.Cin, c.H, c.W)
    if run == "impulse":
        x = _uniform(g, shape, -1, 1)
        dz = torch.zeros((c.B, c.H, c.W, 64))
        for n, (b, y, xx) in enumerate(probes):
            dz[b, y, xx, n] = 1.0
    elif run == "lattice":
        x = _ints(g, shape, -1, 1)
        dz = _ints(g, (c.B, c.H, c.W, 64), -2, 2) * (torch.rand((c.B, c.H, c.W, 64), generator=g) < 0.5)
    else:
        x = _uniform(g, shape, -1, 1)
        dz = _uniform(g, (c.B, c.H, c.W, 64), -1, 1)
    return x, dz.to(torch.bfloat16)


def im2col(x):
    """col [B*H*W, 9 Cin] float64 of the bf16-rounded image, column k = ci * 9 + ty * 3 + tx (the OIHW order), zero outside"""
    B, Cin, H, W = x.shape
    xp = torch.zeros((B, Cin, H + 2, W + 2), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = rne_bf16(x).double()
    cols = [xp[:, ci, ty:ty + H, tx:tx + W] for ci in range(Cin) for ty in range(3) for tx in range(3)]
    return torch.stack(cols, dim=-1).reshape(B * H * W, 9 * Cin)


def stem_wgrad_reference(x, dz):
    """(dW [64, 9 Cin] float64, sum |dz| |col| of the same shape)"""
    col = im2col(x)
    d = dz.double().reshape(-1, 64).t().contiguous()
    return d @ col, d.abs() @ col.abs()


def stem_wgrad_impulse_expected(c, x, probes):
    col = im2col(x)
    want = torch.zeros((64, 9 * c.Cin), dtype=torch.float64)
    for n, (b, y, xx) in enumerate(probes):
        want[n] = col[(b * c.H + y) * c.W + xx]
    return want


def stem_wgrad_bounds(c, A):
    """(bound of the float64 slab sum, bound of segk_wgrad_reduce): module docstring"""
    T, S = stem_wgrad_trips(c)[1], stem_wgrad_slabs(c)
    return (16 * T + 3 + 2) * U24 * A, (16 * T + 3 + 2 + max(S - 1, cdiv(S, 16) + 15)) * U24 * A


# ---- pooling ---------------------------------------------------------------------------------------------------------------
def windows(t):
    """[B,H,W,C] -> the 2x2 windows of the even part [B,Ho,Wo,4,C], position k = 2 * dy + dx (row-major)"""
    B, H, W, C = t.shape
    Ho, Wo = H // 2, W // 2
    return t[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Ho, Wo, 4, C)


def unwindow(win, H, W):
    """the inverse of windows(); the odd border is zero"""
    B, Ho, Wo, _, C = win.shape
    out = torch.zeros((B, H, W, C), dtype=win.dtype)
    out[:, :2 * Ho, :2 * Wo] = win.reshape(B, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, C)
    return out


def plant(x, lo):
    """Plants in x [B,H,W,C] (fp32, in place on a copy) by window number n = (window index + channel) % 8:
    1: equal maxima at (0,1) and (1,0);  2: at (1,0) and (1,1);  3: at (0,0) and (1,1);  4: all four equal;
    5: a negative-only window (values in [lo - 1, lo), lo <= 0);  others: left random."""
    B, H, W, C = x.shape
    win = windows(x).clone()
    Ho, Wo = H // 2, W // 2
    n = (torch.arange(B * Ho * Wo).reshape(B, Ho, Wo, 1) + torch.arange(C)) % 8
    top = win.amax(3) + 0.5
    for kind, ks in ((1, (1, 2)), (2, (2, 3)), (3, (0, 3))):
        for k in ks:
            win[:, :, :, k] = torch.where(n == kind, top, win[:, :, :, k])
    for k in range(4):
        win[:, :, :, k] = torch.where(n == 4, top, win[:, :, :, k])
        win[:, :, :, k] = torch.where(n == 5, lo - 0.0625 - (win[:, :, :, k] - lo).abs().clamp(max=0.9), win[:, :, :, k])
    out = x.clone()
    out[:, :2 * Ho, :2 * Wo] = unwindow(win, 2 * Ho, 2 * Wo)
    return out


def pool_inputs(c, what="pool"):
    """(x [B,H,W,Cp], dy [B,Ho,Wo,Cp], dx0 [B,H,W,Cp] the gradient already there) in the case's dtype, ties planted"""
    dt = TORCH_DT[c.dtype]
    g = _gen(what, tuple(c))
    x = plant(_uniform(g, (c.B, c.H, c.W, c.Cp), -1, 1), -1.0).to(dt)
    dy = _uniform(g, (c.B, c.H // 2, c.W // 2, c.Cp), -1, 1).to(dt)
    dx0 = _uniform(g, (c.B, c.H, c.W, c.Cp), -1, 1).to(dt)
    return x, dy, dx0


def maxpool_fwd_reference(x):
    return windows(x).amax(3)


def first_maximum(win):
    """[B,Ho,Wo,4,C] bool: the first position in row-major order that holds the window's maximum"""
    m = win.amax(3, keepdim=True)
    eq = win == m
    seen = torch.zeros_like(eq[:, :, :, 0])
    sel = torch.zeros_like(eq)
    for k in range(4):
        sel[:, :, :, k] = eq[:, :, :, k] & ~seen
        seen |= eq[:, :, :, k]
    return sel


def maxpool_bwd_presum(x, dy, dx0=None):
    """fp32: dy routed to the first maximum, zero elsewhere and on the odd border, plus dx0 (accumulate) in ONE fp32 add: the
    gradient before it is rounded to the dtype"""
    B, H, W, C = x.shape
    sel = first_maximum(windows(x))
    routed = unwindow(torch.where(sel, dy.unsqueeze(3).expand_as(sel), torch.zeros((), dtype=dy.dtype)), H, W)
    if dx0 is None:
        return routed.float()
    return dx0.float() + routed.float()


def maxpool_bwd_reference(x, dy, dx0=None):
    """dx in x's dtype: dy routed to the first maximum, zero elsewhere and on the odd border; with dx0 (accumulate) the fp32 sum
    dx0 + routed, rounded once to the dtype"""
    return maxpool_bwd_presum(x, dy, dx0).to(x.dtype)


def apply_chunked(z, scale, shift, dtype, chunk=1 << 21):
    """bn_reference.apply_reference over [P, C] rows, a chunk of elements at a time (float64 temporaries stay small)"""
    C = z.shape[-1]
    zf = z.reshape(-1, C)
    out = torch.empty_like(zf)
    rows = max(1, chunk // C)
    for r in range(0, zf.shape[0], rows):
        out[r:r + rows] = apply_reference(zf[r:r + rows], scale, shift, dtype)
    return out.reshape(z.shape)


def apply_pool_inputs(c):
    """(z [B,H,W,Cp] dtype, scale, shift fp32): scale of both signs and zero, and windows (n == 6 of plant's numbering) whose
    four pre-activations are all negative: y == 0 on the whole window"""
    dt = TORCH_DT[c.dtype]
    g = _gen("apply-pool", tuple(c))
    scale = _uniform(g, (c.Cp,), 0.5, 1.5) * torch.where(torch.arange(c.Cp) % 3 == 2, -1.0, 1.0)
    shift = _uniform(g, (c.Cp,), -0.5, 0.5)
    scale[5] = 0.0; shift[5] = 0.25
    scale[6] = 0.0; shift[6] = -0.25
    z = plant(_uniform(g, (c.B, c.H, c.W, c.Cp), -2, 2), -2.0)
    win = windows(z).clone()
    B, Ho, Wo = win.shape[:3]
    n = (torch.arange(B * Ho * Wo).reshape(B, Ho, Wo, 1) + torch.arange(c.Cp)) % 8
    off = torch.where(scale != 0, (-shift - 1.0) / torch.where(scale != 0, scale, torch.ones(())), torch.zeros(()))   # z*scale+shift = -1
    for k in range(4):
        win[:, :, :, k] = torch.where(n == 6, off.expand_as(win[:, :, :, k]), win[:, :, :, k])
    z[:, :2 * Ho, :2 * Wo] = unwindow(win, 2 * Ho, 2 * Wo)
    return z.to(dt), scale, shift


def apply_pool_reference(z, scale, shift, dtype):
    """(y, pooled): y as segk_bn_relu_apply stores it, pooled the maximum of the stored y"""
    y = apply_chunked(z, scale, shift, dtype)
    return y, maxpool_fwd_reference(y)


# ---- pooling backward with the BatchNorm reductions ------------------------------------------------------------------------------
def stat_inputs(s):
    """z, y = relu(bn(z)) as stored, dy, dx0 (all in the dtype) and the fp32 vectors scale, shift, mean, rstd of a training-mode
    BatchNorm on z; degenerate channels as stat_degenerate_channels names them"""
    c = s.case
    dt = TORCH_DT[c.dtype]
    g = _gen("stat", tuple(c), s.degenerate)
    z = _uniform(g, (c.B, c.H, c.W, c.Cp), -2, 2).to(dt)
    gamma = _uniform(g, (c.Cp,), 0.5, 1.5) * torch.where(torch.arange(c.Cp) % 5 == 4, -1.0, 1.0)
    beta = _uniform(g, (c.Cp,), -0.5, 0.5)
    if s.degenerate:
        for ch, kind in stat_degenerate_channels(c.Cp).items():
            if kind == "zero+":
                gamma[ch], beta[ch] = 0.0, 0.4
            elif kind == "zero-":
                gamma[ch], beta[ch] = 0.0, -0.2
            else:
                beta[ch] = beta[ch].abs().clamp(min=0.1)
                gamma[ch] = 1e-3 * beta[ch]
    zf = z.float().reshape(-1, c.Cp)
    mean = zf.double().mean(0).float()
    rstd = (1.0 / torch.sqrt(zf.double().var(0, unbiased=False) + 1e-5)).float()
    scale = gamma * rstd
    shift = beta - mean * scale
    if s.degenerate:                                             # |scale| = |shift| / 1000 on the fp32 vectors the kernel receives
        for ch, kind in stat_degenerate_channels(c.Cp).items():
            if kind == "tiny":
                scale[ch] = shift[ch].abs() / 1000
    y = apply_chunked(z, scale, shift, dt)
    dy = _uniform(g, (c.B, c.H // 2, c.W // 2, c.Cp), -1, 1).to(dt)
    dx0 = _uniform(g, (c.B, c.H, c.W, c.Cp), -1, 1).to(dt)
    return z, y, dy, dx0, scale, shift, mean, rstd


def from_z_channels(scale, shift, dtype, with_z):
    """[Cp] bool: channels whose thread takes xhat from z: any channel of its 16-byte vector has scale == 0 or
    |scale| * 16 < |shift| (fp32), and the caller passed z"""
    vec = pool_vec(dtype)
    bad = (scale == 0) | ((scale.abs() * 16.0) < shift.abs())
    if not with_z:
        bad = torch.zeros_like(bad)
    return bad.reshape(-1, vec).any(1, keepdim=True).expand(-1, vec).reshape(-1)


def stat_reference(s, z, y, dx, scale, shift, mean, rstd, pre=None):
    """Per channel, float64: the two sums of the stored gradient and of the addends the kernel takes (`*_kernel`), each with its
    bound, and the true sum g (z - mean) rstd with its bound (module docstring).  dx is the REFERENCE gradient
    (maxpool_bwd_reference), pre the fp32 value it was rounded from (maxpool_bwd_presum; None: pre == dx)."""
    c = s.case
    C = c.Cp
    sc, sh, mu, rs = scale.double(), shift.double(), mean.double(), rstd.double()
    yy, zz = y.double().reshape(-1, C), z.double().reshape(-1, C)
    g = dx.double().reshape(-1, C) * (yy > 0)
    fz = from_z_channels(scale, shift, c.dtype, s.with_z)
    gk = g if pre is None else pre.double().reshape(-1, C) * (yy > 0)      # sum g: the fp32 value on every channel
    gkx = torch.where(fz, g, gk)                                           # sum g xhat: the from_z re-walk reads dx back
    XA = torch.where(sc != 0, rs / torch.where(sc != 0, sc, torch.ones_like(sc)), torch.zeros_like(sc))
    T1, T2 = sh * XA, mu * rs
    xh_y = yy * XA - T1 - T2
    xh_z = (zz - mu) * rs
    xh = torch.where(fz, xh_z, xh_y)
    d = torch.where(fz, 3 * U24 * xh_z.abs(), U24 * (5 * (yy * XA).abs() + 7 * T1.abs() + 3 * T2.abs()))
    k = 4 * pool_trips(c, "stat") + 256 // (C // pool_vec(c.dtype)) + 4
    ga, gka, gkxa = g.abs(), gk.abs(), gkx.abs()
    r = {"sum_g": g.sum(0), "sum_gx": (g * xh).sum(0), "true_gx": (g * xh_z).sum(0), "from_z": fz,
         "sum_g_kernel": gk.sum(0), "sum_gx_kernel": (gkx * xh).sum(0),
         "bound_g_kernel": k * U24 * gka.sum(0),
         "bound_gx_kernel": (gkxa * d).sum(0) + k * U24 * (gkxa * (xh.abs() + d)).sum(0)}
    # against the STORED gradient: what the one rounding of each addend to the dtype moved, known exactly from the references
    r["bound_g"] = r["bound_g_kernel"] + (gk - g).abs().sum(0)
    r["bound_gx"] = r["bound_gx_kernel"] + ((gkx - g).abs() * (xh.abs() + d)).sum(0)
    cost = (ga * half_ulp(yy, TORCH_DT[c.dtype])).sum(0) * XA.abs()
    r["bound_true"] = r["bound_gx"] + torch.where(fz, torch.zeros_like(cost), cost)
    return r


# ---- BN-statistics finalisation --------------------------------------------------------------------------------------------
def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def finalize_rows(MT, C, per_row=4):
    """Partial rows [MT][C][2] fp32 of `per_row` pixels each: random sums of either sign with a positive variance, and three
    constant-input channels (C >= 64 or the first three): s1 = per_row * a, s2 = fl32(per_row * a * a), so that s2 / count -
    mean^2 cancels to the rounding of a^2 (either sign) or, for a 12-bit a, to zero"""
    g = _gen("finalize", MT, C)
    rows = torch.rand((MT, C, 2), generator=g, dtype=torch.float32)
    rows[:, :, 0] = rows[:, :, 0] * 2 - 1
    rows[:, :, 1] = rows[:, :, 1] * 4 + 3.0
    const = {2: 0.3, 3: 0.7, 4: 1365.0 / 4096, 6: 0.1, 7: 1.9}
    for ch, a in const.items():
        a = torch.tensor(a, dtype=torch.float32)
        rows[:, ch, 0] = per_row * a
        rows[:, ch, 1] = (per_row * a.double() * a.double()).float()
    return rows, sorted(const)


def finalize_reference(rows, count, C_real, gamma, beta, cb, rm0, rv0, momentum, eps, training):
    """float64 values and bounds (module docstring) of scale, shift, mean, rstd, running_mean, running_var over the C_real
    channels.  momentum and eps enter as the fp32 values the kernel receives."""
    m, e = f32(momentum), f32(eps)
    om = f32(1.0 - m)                                            # 1.f - momentum in fp32
    g, be = gamma.double()[:C_real], beta.double()[:C_real]
    cbd = cb.double()[:C_real] if cb is not None else torch.zeros(C_real, dtype=torch.float64)
    rm, rv = rm0.double()[:C_real], rv0.double()[:C_real]
    r = {}
    if training:
        MT = rows.shape[0]
        s = rows.double().sum(0)[:C_real]
        sa = rows.double().abs().sum(0)[:C_real]
        e_s1, e_s2 = 2 * MT * U53 * sa[:, 0], 2 * MT * U53 * sa[:, 1]
        mean = s[:, 0] / count
        raw = s[:, 1] / count - mean * mean
        var = raw.clamp(min=0)
        e_var = e_s2 / count + 2 * mean.abs() * e_s1 / count + 2.0 ** -50 * (s[:, 1].abs() / count + mean * mean)
        rstd = 1.0 / torch.sqrt(var + e)
        e_mean = U24 * mean.abs() + e_s1 / count
        e_rstd = U24 * rstd + 0.5 * rstd ** 3 * e_var
        scale = g * rstd
        e_scale = U24 * scale.abs() + g.abs() * e_rstd
        shift = be - mean * scale
        e_shift = scale.abs() * e_mean + mean.abs() * e_scale + U24 * (be.abs() + 2 * (mean * scale).abs())
        ratio = count / (count - 1.0) if count > 1 else 1.0
        unb = var * ratio
        r.update(raw_var=raw, mean=(mean, e_mean), rstd=(rstd, e_rstd), scale=(scale, e_scale), shift=(shift, e_shift),
                 rmean=(om * rm + m * (mean + cbd), 4 * U24 * ((om * rm).abs() + (m * (mean + cbd)).abs()) + m * e_mean),
                 rvar=(om * rv + m * unb, 4 * U24 * ((om * rv).abs() + m * unb) + m * (U24 * unb + e_var * ratio)))
    else:
        rstd = 1.0 / torch.sqrt(rv + e)
        e_rstd = 6 * U24 * rstd
        scale = g * rstd
        e_scale = U24 * scale.abs() + g.abs() * e_rstd
        dm = cbd - rm
        shift = be + dm * scale
        e_shift = U24 * dm.abs() * scale.abs() + dm.abs() * e_scale + U24 * (be.abs() + 2 * (dm * scale).abs())
        r.update(mean=(rm - cbd, U24 * (rm - cbd).abs()), rstd=(rstd, e_rstd), scale=(scale, e_scale), shift=(shift, e_shift),
                 rmean=(rm, torch.zeros_like(rm)), rvar=(rv, torch.zeros_like(rv)))
    return r
