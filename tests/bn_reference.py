"""float64 references and derived error bounds for the BatchNorm+ReLU backward / apply / channel-sum kernels
(csrc/bn_pool.hip), shared by tests/test_gpu_bn_backward_matrix.py and tests/test_gpu_kernels.py.  CPU torch only.

All tensors are [P, Cp]: z and dy already rounded to the compute dtype, scale / shift / mean / rstd the fp32 vectors exactly as
the kernel receives them.  Nothing here is taken from what the kernels return."""
import torch

U24 = 2.0 ** -24          # unit roundoff of fp32


def lane_geometry(Cp, dtype):
    """lane_geometry(cvec, 128) of csrc/channel_lanes.hpp as bn_pool.hip calls it: (channel vectors per block, pixel rows per block, channel blocks)."""
    vec = 8 if dtype == torch.bfloat16 else 4
    cvec = Cp // vec
    cvb = min(cvec, 128)
    return cvb, 256 // cvb, -(-cvec // cvb)


def reduce_chain(P, Cp, dtype):
    """(n_t, rows, gx) of the reduce passes: gx = min(ceil(P / rows), 512) blocks (segk_bn_bwd_blocks); a thread adds
    n_t = ceil(P / (gx * rows)) terms in fp32, thread 0 of the block then `rows` partial sums in fp32, the finalize pass the gx
    block sums in float64."""
    rows = lane_geometry(Cp, dtype)[1]
    gx = min(-(-P // rows), 512)
    return -(-P // (gx * rows)), rows, gx


def sum_bound(P, Cp, dtype, abs_sum, per_term_roundings=0):
    """|error| of a channel sum the kernels form: (n_t + rows + 4 + roundings per term) * 2^-24 * sum |term| (the 4: the
    float64 stage, the final rounding to fp32 and slack for second-order terms)."""
    n_t, rows, _ = reduce_chain(P, Cp, dtype)
    return (n_t + rows + 4 + per_term_roundings) * U24 * abs_sum


def half_ulp(x, dtype):
    """half a unit in the last place of `dtype` in the binade of |x| (float64 tensor)"""
    mant = 7 if dtype == torch.bfloat16 else 23
    _, e = torch.frexp(x.abs().clamp(min=2.0 ** -120))          # |x| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 2 - mant)


def bwd_reference(z, dy, scale, shift, mean, rstd):
    """g = dy * [z*scale + shift > 0]; dbeta = sum g; dgamma = sum g * xhat; dz = scale * (g - dbeta/P - xhat * dgamma/P), float64.
    z * scale is exact in float64 (two 24-bit significands) and adding shift cannot change the sign, so the mask is the one
    a correctly rounded fmaf gives."""
    P = z.shape[0]
    z64, sc, sh, mu, rs = z.double(), scale.double(), shift.double(), mean.double(), rstd.double()
    g = dy.double() * (z64 * sc + sh > 0)
    xh = (z64 - mu) * rs
    r = {"g": g, "xhat": xh, "dbeta": g.sum(0), "dgamma": (g * xh).sum(0), "abs_g": g.abs().sum(0), "abs_gx": (g * xh).abs().sum(0)}
    r["dz"] = sc * (g - r["dbeta"] / P - xh * r["dgamma"] / P)
    return r


def dz_bound(ref, scale, dtype, e_dbeta, e_dgamma):
    """per element: the fp32 evaluation 8 * 2^-24 * |scale| * (|g| + |c1| + |xhat * c2|), the error of the two sums carried
    through c1 = dbeta / P and c2 = dgamma / P, and half an ulp of `dtype` for the store (taken in the binade the computed
    value can reach: |reference| + the fp32 error)."""
    P = ref["g"].shape[0]
    sc = scale.double().abs()
    c1, c2 = ref["dbeta"] / P, ref["dgamma"] / P
    e32 = 8 * U24 * sc * (ref["g"].abs() + c1.abs() + (ref["xhat"] * c2).abs()) + sc * (e_dbeta / P + ref["xhat"].abs() * e_dgamma / P)
    return e32 + half_ulp(ref["dz"].abs() + e32, dtype)


def apply_reference(z, scale, shift, dtype):
    """relu(fmaf(z, scale, shift)) correctly rounded to fp32, then rounded to `dtype`.  The product is exact in float64; the sum
    is rounded to float64 first, which changes the fp32 result only when the rounded sum sits exactly between two fp32 values:
    those ties are resolved with the exact remainder of the addition (two-sum)."""
    p = z.double() * scale.double()
    sh = shift.double().expand_as(p)
    s = p + sh
    bb = s - p
    err = (p - (s - bb)) + (sh - bb)                     # exact: p + sh == s + err
    r = s.float()
    d = s - r.double()
    inf = torch.full_like(r, float("inf"))
    lo = torch.where(d >= 0, r, torch.nextafter(r, -inf))
    hi = torch.where(d > 0, torch.nextafter(r, inf), r)
    tie = (lo != hi) & ((s - lo.double()) == (hi.double() - s)) & (err != 0)
    r = torch.where(tie, torch.where(err > 0, hi, lo), r)
    return torch.clamp(r, min=0).to(dtype)
