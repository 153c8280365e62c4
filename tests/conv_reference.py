"""float64 restatement of the 3x3 convolution forward / data gradient (csrc/conv_igemm.hip, conv_pipe.hip,
conv_ws.hip, conv_rs.hip), the inputs of the three runs of tests/test_gpu_conv_matrix.py and the derived bound of its dense run.  CPU torch only; activations are
NHWC [B, H, W, C], weights OIHW as the layer holds them.  Nothing here is taken from what the kernels return.

The dense bound.  Operands are exact in the reference (they are rounded to `dtype` before both sides see them; with the
prologue the activation is what segk_bn_relu_apply stores, restated exactly by bn_reference.apply_reference).  A kernel
forms z = sum of K = 9 (CA + CB) products (+ bias) in fp32, in an order of its own.  Summing K numbers t_i in ANY order
with fp32 adds is off by at most (K - 1) * 2^-24 * sum |t_i| (plus second-order terms); a bf16 x bf16 product is exact in
fp32 (8 + 8 significand bits), an fp32 x fp32 product is rounded once more, which at most doubles the count.  So

    |z_kernel - z| <= e := g * K * 2^-24 * A,      A = sum |w| |x| (+ |bias|),  g = 1 for bf16, 2 for fp32,

and the stored output adds one rounding to `dtype`: |got - z| <= u * |z| + e with u = 2^-8 (bf16) or 2^-23 (fp32).  No
accumulation order can be wrongly rejected by it; it is loose on purpose, the impulse and the lattice run are exact.
The statistics are taken from the fp32 accumulators (bias included) and summed over the P = B*H*W pixels in fp32 in any order:

    |sum_kernel   - sum z|   <= sum_p e_p                    + P * 2^-24 * sum_p (|z_p| + e_p)
    |sumsq_kernel - sum z^2| <= sum_p e_p (2 |z_p| + e_p)    + (P + 1) * 2^-24 * sum_p (|z_p| + e_p)^2

(the + 1: the rounding of the square itself)."""
import zlib

import torch

from bn_reference import apply_reference
from conv_cases import input_channels, lattice_density, logical_of

TORCH_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
U24 = 2.0 ** -24
U_OUT = {"bf16": 2.0 ** -8, "fp32": 2.0 ** -23}
G_PROD = {"bf16": 1, "fp32": 2}


# ---- the operation -----------------------------------------------------------------------------------------------------------
def conv3x3(x, w):
    """out[b, y, x, n] = sum over ty, tx, k of x[b, y + ty - 1, x + tx - 1, k] * w[n, k, ty, tx], zero outside the image."""
    B, H, W, K = x.shape
    xp = torch.zeros((B, H + 2, W + 2, K), dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros((B, H, W, w.shape[0]), dtype=x.dtype)
    for ty in range(3):
        for tx in range(3):
            out += xp[:, ty:ty + H, tx:tx + W, :] @ w[:, :, ty, tx].t()
    return out


def conv3x3_transposed(g, w):
    """The data gradient of conv3x3 (ConvTranspose2d, stride 1, padding 1): every g[b, y, x, co] * w[co, ci, ty, tx] is added to
    out[b, y + ty - 1, x + tx - 1, ci]."""
    B, H, W, _ = g.shape
    op = torch.zeros((B, H + 2, W + 2, w.shape[1]), dtype=g.dtype)
    for ty in range(3):
        for tx in range(3):
            op[:, ty:ty + H, tx:tx + W, :] += g @ w[:, :, ty, tx]
    return op[:, 1:H + 1, 1:W + 1].contiguous()


def prologue(z, scale, shift, dtype):
    """relu(z * scale + shift) rounded to `dtype`, exactly as segk_bn_relu_apply stores it (one fused multiply-add in fp32)"""
    return apply_reference(z, scale, shift, TORCH_DT[dtype])


def channel_stats(z):
    """per-channel (sum, sum of squares) over all pixels, float64"""
    z = z.double().reshape(-1, z.shape[-1])
    return z.sum(0), (z * z).sum(0)


# ---- one problem: inputs of a run and their reference ------------------------------------------------------------------------
class Problem:
    """Inputs of one kernel call in the layout the C ABI takes (xa, xb, bias, scale, shift; w is the fp32 OIHW parameter
    segk_pack_conv_weight receives together with pack_args) and the float64 reference of what it must return."""

    def __init__(self, c, xa, xb, w, bias, scale, shift):
        self.c, self.xa, self.xb, self.w, self.bias, self.scale, self.shift = c, xa, xb, w, bias, scale, shift
        la, lb, lo1, lo2 = logical_of(c)
        assert (lo1 == c.CO1 or not c.CO2) and (la == c.CA or not c.CB)
        if c.mode == 0:      # Cout, CA, CB, Coutp, CAp, CBp of segk_pack_conv_weight
            self.pack_args = (lo1 + lo2, la, lb, c.CO1 + c.CO2, c.CA, c.CB)
        else:                # the layer's outputs are this call's inputs and the other way round
            self.pack_args = (la + lb, lo1, lo2, c.CA + c.CB, c.CO1, c.CO2)
        assert tuple(w.shape) == (self.pack_args[0], self.pack_args[1] + self.pack_args[2], 3, 3)

    def activation(self):
        """what the MFMAs multiply: [B, H, W, CA + CB] in `dtype` (with the prologue: relu(bn(srcA)), the act_out side output)"""
        a = self.xa
        if self.c.prologue:
            a = prologue(self.xa.reshape(-1, self.c.CA), self.scale, self.shift, self.c.dtype).reshape(self.xa.shape)
        return a if self.xb is None else torch.cat([a, self.xb], dim=3)

    def _apply(self, act, w, bias):
        c = self.c
        _, _, lo1, lo2 = logical_of(c)
        x = act[..., input_channels(c)]
        o = conv3x3(x, w) if c.mode == 0 else conv3x3_transposed(x, w)
        out = torch.zeros(act.shape[:3] + (c.CO1 + c.CO2,), dtype=o.dtype)
        out[..., :lo1] = o[..., :lo1]
        out[..., c.CO1:c.CO1 + lo2] = o[..., lo1:]
        return out + bias if bias is not None else out

    def reference(self):
        """z [B, H, W, CO1 + CO2] float64 over the padded channels (zero where no logical channel is)"""
        return self._apply(self.activation().double(), self.w.double(), None if self.bias is None else self.bias.double())

    def abs_reference(self):
        """A = sum |w| |x| (+ |bias|), the scale of the dense bound"""
        return self._apply(self.activation().double().abs(), self.w.double().abs(),
                           None if self.bias is None else self.bias.double().abs())

    def fast_reference(self):
        """fp32 on the CPU through torch's own convolution: exact, and equal to reference(), on lattice inputs only"""
        import torch.nn.functional as F
        c = self.c
        _, _, lo1, lo2 = logical_of(c)
        x = self.activation().float()[..., input_channels(c)].permute(0, 3, 1, 2).contiguous()
        o = (F.conv2d(x, self.w, padding=1) if c.mode == 0 else F.conv_transpose2d(x, self.w, padding=1)).permute(0, 2, 3, 1)
        out = torch.zeros(o.shape[:3] + (c.CO1 + c.CO2,), dtype=torch.float32)
        out[..., :lo1] = o[..., :lo1]
        out[..., c.CO1:c.CO1 + lo2] = o[..., lo1:]
        return out + self.bias if self.bias is not None else out

    def conv_view_weight(self):
        """Wc [CO1 + CO2, CA + CB, 3, 3] float64 with out = conv3x3(activation, Wc) in both modes: the weight an impulse at
        input channel k, seen through tap (ty, tx), leaves in output channel n"""
        c = self.c
        _, _, lo1, lo2 = logical_of(c)
        w = self.w.double() if c.mode == 0 else self.w.double().flip(2, 3).transpose(0, 1)
        rows = list(range(lo1)) + [c.CO1 + j for j in range(lo2)]
        wc = torch.zeros((c.CO1 + c.CO2, c.CA + c.CB, 3, 3), dtype=torch.float64)
        wc[torch.tensor(rows)[:, None], torch.tensor(input_channels(c))[None, :]] = w
        return wc


def _gen(c, run, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(f"{run}/{salt}/{tuple(c)}".encode()))


def _uniform(g, shape, lo, hi):
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _pick(g, shape, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


def _w_shape(c):
    la, lb, lo1, lo2 = logical_of(c)
    return (lo1 + lo2, la + lb, 3, 3) if c.mode == 0 else (la + lb, lo1 + lo2, 3, 3)


def _pad_channels(t, positions, Cp):
    out = torch.zeros(t.shape[:-1] + (Cp,), dtype=t.dtype)
    out[..., positions] = t
    return out


def _out_channels(c):
    _, _, lo1, lo2 = logical_of(c)
    return list(range(lo1)) + [c.CO1 + j for j in range(lo2)]


def _exact_prologue(c, g, on):
    """scale a power of two of both signs, shift = +-0.5 (positive on three channels of four), and the z that makes the
    activation exactly 1.0 where `on` and exactly 0 elsewhere (pre-activation -1): every step is exact in fp32 and in bf16"""
    scale = torch.ldexp(_pick(g, (c.CA,), [1.0, -1.0]), torch.randint(-2, 3, (c.CA,), generator=g))
    shift = torch.full((c.CA,), 0.5)
    shift[3::4] = -0.5
    z = (torch.where(on, 1.0, -1.0) - shift) / scale
    return z, scale, shift


def make_problem(c, run, probes=None):
    """run: "impulse" (probes = one group of conv_cases.probe_passes), "lattice" or "dense"."""
    dt = TORCH_DT[c.dtype]
    la, lb, lo1, lo2 = logical_of(c)
    g = _gen(c, run)
    shape = (c.B, c.H, c.W)
    n_log = lo1 + lo2
    scale = shift = None
    if run == "impulse":
        w = torch.randint(-64, 65, _w_shape(c), generator=g).float() / 64
        bias = _pick(g, (n_log,), [-0.5, -0.25, 0.25, 0.5]) if c.bias else None
        x = torch.zeros(shape + (c.CA + c.CB,))
        for b, y, xx, k in probes:
            x[b, y, xx, k] = 1.0
    elif run == "lattice":
        w = _pick(g, _w_shape(c), [-1.0, -0.5, 0.0, 0.5, 1.0])
        bias = _pick(g, (n_log,), [-1.0, -0.5, 0.0, 0.5, 1.0]) if c.bias else None
        keep = torch.rand(shape + (c.CA + c.CB,), generator=g) < 1.5 * lattice_density(c)     # then 2/3 of those non-zero
        x = _pick(g, shape + (c.CA + c.CB,), [1.0] if c.prologue else [-1.0, 0.0, 1.0]) * keep
        if c.prologue:
            x = x * (torch.rand(x.shape, generator=g) < 2.0 / 3.0)
        x = _pad_channels(x[..., input_channels(c)], input_channels(c), c.CA + c.CB)
    else:
        w = _uniform(g, _w_shape(c), -1, 1).to(dt).float()
        bias = _uniform(g, (n_log,), -1, 1) if c.bias else None
        x = _pad_channels(_uniform(g, shape + (la + lb,), -1, 1), input_channels(c), c.CA + c.CB)
    xa, xb = x[..., :c.CA], (x[..., c.CA:] if c.CB else None)
    if c.prologue and run != "dense":
        xa, scale, shift = _exact_prologue(c, g, xa != 0)
    elif c.prologue:
        xa = _uniform(g, shape + (c.CA,), -2, 2)
        scale = _uniform(g, (c.CA,), -1.5, 1.5)
        shift = _uniform(g, (c.CA,), 0.1, 0.6)
        shift[3::4] *= -1
    if bias is not None:
        bias = _pad_channels(bias, _out_channels(c), c.CO1 + c.CO2)
    return Problem(c, xa.to(dt).contiguous(), None if xb is None else xb.to(dt).contiguous(), w, bias, scale, shift)


# ---- impulse: the expected output by placement -------------------------------------------------------------------------------
def impulse_expected(prob, probes):
    """z [B, H, W, N] float64: the probe at (b, y, x, k) leaves Wc[:, k, ty, tx] at output pixel (y - ty + 1, x - tx + 1), bias
    everywhere, and nothing else.  `reached` [B, H, W] int64: index of the probe that reaches the pixel, or -1."""
    c = prob.c
    wc = prob.conv_view_weight()
    z = torch.zeros((c.B, c.H, c.W, c.CO1 + c.CO2), dtype=torch.float64)
    reached = torch.full((c.B, c.H, c.W), -1, dtype=torch.int64)
    for i, (b, y, x, k) in enumerate(probes):
        for ty in range(3):
            for tx in range(3):
                oy, ox = y - ty + 1, x - tx + 1
                if 0 <= oy < c.H and 0 <= ox < c.W:
                    assert reached[b, oy, ox] < 0, "two probes of one pass reach one output pixel"
                    z[b, oy, ox] = wc[:, k, ty, tx]
                    reached[b, oy, ox] = i
    return (z + prob.bias.double() if prob.bias is not None else z), reached


# ---- exactness conditions and the dense bound --------------------------------------------------------------------------------
def stats_are_exact(z, unit):
    """Every partial sum of z and of z^2 over the pixels, in any order, is exact in fp32: the terms are multiples of `unit`
    (unit^2) and sum |z| / unit, sum z^2 / unit^2 stay below 2^24, per channel."""
    z = z.double().reshape(-1, z.shape[-1])
    assert bool((z / unit == (z / unit).round()).all())
    return bool((z.abs().sum(0) / unit < 2 ** 24).all() and ((z * z).sum(0) / unit ** 2 < 2 ** 24).all())


def dense_bounds(c, z, A):
    """(per-element bound of the stored output, bound of the per-channel sum, of the sum of squares): see the module docstring"""
    K = 9 * (c.CA + c.CB)
    e = G_PROD[c.dtype] * K * U24 * A
    P = c.B * c.H * c.W
    za = (z.abs() + e).reshape(P, -1)
    e2 = e.reshape(P, -1)
    return (U_OUT[c.dtype] * z.abs() + e,
            e2.sum(0) + P * U24 * za.sum(0),
            (e2 * (2 * z.abs().reshape(P, -1) + e2)).sum(0) + (P + 1) * U24 * (za * za).sum(0))
