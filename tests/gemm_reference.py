"""float64 restatement of the 1x1-geometry operations -- nn.Linear (+ quick_gelu), its split-K form, Conv2d 1x1,
ConvTranspose2d(k=2, s=2) and its data gradient (csrc/gemm.hip, csrc/convt_stream.hip, GEO == 1 of csrc/conv_igemm.hip) --
the inputs of the three runs of tests/test_gpu_gemm_matrix.py and the derived bound of its dense run.  CPU torch only;
activations are NHWC, weights as the layers hold them: [N][K] for the linear and 1x1 forms, IOHW [Cin][Cout][2][2] for the
ConvTranspose.  Nothing here is taken from what the kernels return.

Every entry is one matrix product Z[M][Ng] = A[M][Kg] . Wg[Kg][Ng] (+ bias), Problem.gemm_operands():
  linear / conv1x1:  A = the rows / pixels,  Wg = w^T
  convt_fwd:         A = the input pixels,   Wg[ci][q * Cout + co] = w[ci][co][q]   (q = 2 ky + kx), Z re-arranged to
                     out[b][2y + ky][2x + kx][co]  (the pixel-shuffle store)
  convt_dgrad:       A[m][q * Cout + co] = dout[b][2y + ky][2x + kx][co]  (the un-shuffle gather), Wg[q * Cout + co][ci] = w[ci][co][q]
and the float64 reference is torch.matmul on the exact operands (they are rounded to `dtype` before both sides see them).

The dense bound is conv_reference's: a kernel sums the K products in fp32 in an order of its own, so
|z_kernel - z| <= e := G_PROD * K * 2^-24 * A with A = |x| . |w| + |bias|, and the stored value adds one rounding:
|got - z| <= U_OUT * |z| + e.  A split-K part is bounded the same way over its own K range (the bias in part 0 only, each
part rounded once); the sum of the parts by the sum of the bounds.  With act = 1 the kernel stores g(z') = z' / (1 + exp(-1.702
z')) of its own fp32 z': |g'| <= 1.1, so |got - g(z)| <= U_OUT * |g(z)| + 1.1 * e + ACT_ULPS * 2^-23 * max(1, |z|), the last
term for the device's fp32 multiply, exp, add and divide."""
import zlib

import torch

from conv_reference import G_PROD, TORCH_DT, U24, U_OUT
from gemm_cases import gemm_view, rows_of

# Error of the device's fp32 quick_gelu (v / (1 + __expf(-1.702 v))) beyond the propagated accumulation error, in units of
# 2^-23 * max(1, |z|).  It is measured, not derived: the worst |got - g(z)| - U_OUT |g(z)| - 1.1 e over the fp32 act cases against
# float64 (profiles/gemm_matrix_parity.txt) and the constant is twice that, rounded up to a power of two.
# Measured worst: -100.67 (linear-fp32-336x64x128-a; -3939 at K = 768) -- negative on all seven cases: the any-order term 1.1 e
# alone already covers the device's multiply, exp, add and divide.  Twice a negative worst lies below every power of two, so the
# constant is 2^0, which keeps the term (and its growth with |z|, the argument of the exp) in the bound.
ACT_ULPS = 1.0


def quick_gelu(z):
    return z * torch.sigmoid(1.702 * z)


# ---- the operations, as the layers state them --------------------------------------------------------------------------------
def linear(x, w, bias=None):
    """x [M, K], w [N, K]"""
    z = torch.matmul(x, w.t())
    return z if bias is None else z + bias


def conv1x1(x, w, bias=None):
    """x [B, H, W, K] NHWC, w [N, K]"""
    return linear(x, w, bias)


def shuffle(z2d, B, H, W, Cout):
    """Z [M, 4 Cout] (tap-major) -> [B, 2H, 2W, Cout]"""
    return z2d.reshape(B, H, W, 2, 2, Cout).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, Cout)


def unshuffle(g, B, H, W, Cout):
    """[B, 2H, 2W, Cout] -> A [M, 4 Cout] (tap-major)"""
    return g.reshape(B, H, 2, W, 2, Cout).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, 4 * Cout)


def convt_weight_fwd(w):
    """IOHW [Cin, Cout, 2, 2] -> Wg [Cin, 4 Cout]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 4 * w.shape[1])


def convt2x2(x, w, bias=None):
    """ConvTranspose2d(k=2, s=2): x [B, H, W, Cin] NHWC, w [Cin, Cout, 2, 2] -> [B, 2H, 2W, Cout]"""
    B, H, W, _ = x.shape
    z = torch.matmul(x.reshape(B * H * W, -1), convt_weight_fwd(w))
    if bias is not None:
        z = z + bias.repeat(4)
    return shuffle(z, B, H, W, w.shape[1])


def convt2x2_dgrad(g, w):
    """its data gradient: g [B, 2H, 2W, Cout] -> [B, H, W, Cin]"""
    B, H2, W2, Cout = g.shape
    return torch.matmul(unshuffle(g, B, H2 // 2, W2 // 2, Cout), convt_weight_fwd(w).t()).reshape(B, H2 // 2, W2 // 2, -1)


# ---- one problem ---------------------------------------------------------------------------------------------------------------
def k_positions(c):
    """positions of the logical K elements in the padded GEMM K (tap-major for the data gradient)"""
    if c.entry == "convt_dgrad":
        return [q * c.Cout + j for q in range(4) for j in range(c.Lout)]
    return list(range(c.Lin))


def n_positions(c):
    """positions of the logical output channels in the padded GEMM N (tap-major for the forward ConvTranspose)"""
    if c.entry == "convt_fwd":
        return [q * c.Cout + j for q in range(4) for j in range(c.Lout)]
    return list(range(c.Lin if c.entry == "convt_dgrad" else c.Lout))


def out_channels(c):
    """(padded, logical) channel count of the stored output"""
    return (c.Cin, c.Lin) if c.entry == "convt_dgrad" else (c.Cout, c.Lout)


class Problem:
    """Inputs of one call in the layout the C ABI takes -- x: the activation in `dtype` ([M, K] rows, NHWC pixels, or dout [B, 2H,
    2W, Cout]); w: the fp32 parameter the pack entry receives; bias: fp32 over the padded GEMM N or None -- and the reference."""

    def __init__(self, c, x, w, bias):
        self.c, self.x, self.w, self.bias = c, x, w, bias
        assert tuple(w.shape) == ((c.Lin, c.Lout, 2, 2) if c.entry.startswith("convt") else (c.Lout, c.Lin))

    def gemm_operands(self, dtype=torch.float64):
        """A [M, Kg], Wg [Kg, Ng] over the padded K and N (zero where no logical channel is), bias [Ng] or None; float64 (fp32
        holds the operands exactly too)"""
        c = self.c
        M, K, N, mode = gemm_view(c)
        x = self.x.to(dtype)
        A = unshuffle(x, c.B, c.H, c.W, c.Cout) if mode == 2 else x.reshape(M, K)
        w = self.w.to(dtype)
        wl = w.t() if mode == 0 else convt_weight_fwd(w) if mode == 1 else convt_weight_fwd(w).t()      # logical [Kl, Nl]
        Wg = torch.zeros((K, N), dtype=dtype)
        Wg[torch.tensor(k_positions(c))[:, None], torch.tensor(n_positions(c))[None, :]] = wl
        return A, Wg, None if self.bias is None else self.bias.to(dtype)

    def arrange(self, z2d):
        """Z [M, Ng] (or [S, M, Ng]) -> the layout of the stored output"""
        c = self.c
        if c.entry == "convt_fwd":
            return shuffle(z2d, c.B, c.H, c.W, c.Cout)
        if c.entry in ("linear", "linear_splitk"):
            return z2d
        return z2d.reshape(c.B, c.H, c.W, -1)

    def k_ranges(self):
        K = gemm_view(self.c)[1]
        return [(s * (K // self.c.S), (s + 1) * (K // self.c.S)) for s in range(self.c.S)]

    def _product(self, A, Wg, bias):
        if self.c.entry != "linear_splitk":
            z = torch.matmul(A, Wg)
            return z if bias is None else z + bias
        parts = [torch.matmul(A[:, a:b], Wg[a:b]) for a, b in self.k_ranges()]
        if bias is not None:
            parts[0] = parts[0] + bias
        return torch.stack(parts)

    def reference(self):
        """float64 pre-activation z in the layout of the stored output; split-K: the parts [S, M, N]"""
        return self.arrange(self._product(*self.gemm_operands()))

    def abs_reference(self):
        A, Wg, bias = self.gemm_operands()
        return self.arrange(self._product(A.abs(), Wg.abs(), None if bias is None else bias.abs()))

    def fast_reference(self):
        """fp32 on the CPU: exact, and equal to reference(), on lattice inputs only"""
        return self.arrange(self._product(*self.gemm_operands(torch.float32)))


def _gen(c, run):
    return torch.Generator().manual_seed(zlib.crc32(f"gemm/{run}/{tuple(c)}".encode()))


def _uniform(g, shape, lo, hi):
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _pick(g, shape, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


def _w_shape(c):
    return (c.Lin, c.Lout, 2, 2) if c.entry.startswith("convt") else (c.Lout, c.Lin)


def k_order(c):
    """The logical K positions in the order the one-hot run visits them: first and last of every 32- and 64-element chunk and
    the last logical position below padding first (a short problem reaches at least those), then all the others."""
    ks = k_positions(c)
    have = set(ks)
    first = [k for k in ks if k % 32 in (0, 31) or k + 1 not in have]      # ... and the last logical position before padding
    seen = set(first)
    return first + [k for k in ks if k not in seen]


def one_hot_k(c):
    """k(m) of the one-hot run, a LongTensor [M]: the rows walk k_order, one step further after every 1009 rows (a prime), so
    that two rows a power of two apart -- what a stale ring slot or a stale register buffer of a persistent kernel would
    deliver -- do not hold the same k"""
    order = torch.tensor(k_order(c))
    m = torch.arange(rows_of(c))
    return order[(m + m // 1009) % len(order)]


def _activation_from_rows(c, A):
    """A [M, Kg] float32 -> the activation in the layout the entry takes"""
    if c.entry == "convt_dgrad":          # inverse of unshuffle
        return A.reshape(c.B, c.H, c.W, 2, 2, c.Cout).permute(0, 1, 3, 2, 4, 5).reshape(c.B, 2 * c.H, 2 * c.W, c.Cout).contiguous()
    if c.entry in ("linear", "linear_splitk"):
        return A
    return A.reshape(c.B, c.H, c.W, -1)


def make_problem(c, run):
    """run: "one-hot", "lattice" or "dense"."""
    dt = TORCH_DT[c.dtype]
    M, K, N, mode = gemm_view(c)
    g = _gen(c, run)
    npos = n_positions(c)
    nb = c.Lout if mode == 1 else len(npos)          # the ConvTranspose bias is per channel, repeated for the four taps
    kpos = torch.tensor(k_positions(c))
    if run == "one-hot":
        w = torch.randint(-64, 65, _w_shape(c), generator=g).float() / 64
        b = torch.randint(-64, 65, (nb,), generator=g).float() / 64 if c.bias else None
        A = torch.zeros((M, K))
        A[torch.arange(M), one_hot_k(c)] = 1.0
    elif run == "lattice":
        w = _pick(g, _w_shape(c), [-1.0, -0.5, 0.0, 0.5, 1.0])
        b = _pick(g, (nb,), [-1.0, -0.5, 0.0, 0.5, 1.0]) if c.bias else None
        A = torch.zeros((M, K))
        A[:, kpos] = _pick(g, (M, len(kpos)), [-1.0, 0.0, 1.0])
    else:
        w = _uniform(g, _w_shape(c), -1, 1).to(dt).float()
        b = _uniform(g, (nb,), -1, 1) if c.bias else None
        A = torch.zeros((M, K))
        A[:, kpos] = _uniform(g, (M, len(kpos)), -1, 1)
    bias = None
    if b is not None:
        bias = torch.zeros((N,))
        bias[npos] = b.repeat(4) if mode == 1 else b
    return Problem(c, _activation_from_rows(c, A).to(dt).contiguous(), w, bias)


# ---- one-hot: the expected output by selection ---------------------------------------------------------------------------------
def one_hot_expected(prob, dtype=torch.float64):
    """z in the layout of the stored output: row m is row k(m) of Wg plus the bias -- one weight per element, no sum (multiples
    of 1/64 up to 2: exact in fp32 too).  Split-K: the part whose K range holds k(m) carries the weight, the others zero; the
    bias rides on part 0."""
    c = prob.c
    _, Wg, bias = prob.gemm_operands(dtype)
    km = one_hot_k(c)
    z = Wg[km]
    if c.entry == "linear_splitk":
        z = torch.stack([z * ((km >= a) & (km < b))[:, None] for a, b in prob.k_ranges()])
        if bias is not None:
            z[0] += bias
    elif bias is not None:
        z = z + bias
    return prob.arrange(z)


def locate(c, idx):
    """index of a stored output element -> (GEMM row m, GEMM column n, tap or None, words that name the element)"""
    idx = [int(i) for i in idx]
    part = ""
    if c.entry == "linear_splitk":
        part, idx = f"part {idx[0]}, ", idx[1:]
    if c.entry in ("linear", "linear_splitk"):
        return idx[0], idx[1], None, f"{part}row {idx[0]}, column {idx[1]}"
    b, y, x, n = idx
    if c.entry == "convt_fwd":
        q = 2 * (y % 2) + x % 2
        m = (b * c.H + y // 2) * c.W + x // 2
        return m, q * c.Cout + n, q, f"output pixel (b,y,x)=({b},{y},{x}) = input pixel {m}, tap {q}, channel {n}"
    return (b * c.H + y) * c.W + x, n, None, f"pixel (b,y,x)=({b},{y},{x}), channel {n}"


# ---- the dense bound -----------------------------------------------------------------------------------------------------------
def dense_bound(c, z, A):
    """per-element bound of the stored output (see the module docstring); z, A as reference() / abs_reference() return them (a
    split-K part's K is its own range)"""
    K = gemm_view(c)[1] // c.S
    e = G_PROD[c.dtype] * K * U24 * A
    if not c.act:
        return U_OUT[c.dtype] * z.abs() + e
    return U_OUT[c.dtype] * quick_gelu(z).abs() + 1.1 * e + ACT_ULPS * 2.0 ** -23 * z.abs().clamp(min=1.0)


def act_excess(c, got, z, A):
    """what ACT_ULPS has to cover: the worst |got - g(z)| - U_OUT |g(z)| - 1.1 e in units of 2^-23 max(1, |z|)"""
    K = gemm_view(c)[1]
    e = G_PROD[c.dtype] * K * U24 * A
    g = quick_gelu(z)
    return float((((got.double() - g).abs() - U_OUT[c.dtype] * g.abs() - 1.1 * e) / (2.0 ** -23 * z.abs().clamp(min=1.0))).max())
