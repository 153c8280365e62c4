"""float64 references, structured inputs and derived bounds for csrc/vit.hip and the bilinear entries of csrc/resize.hip: what
tests/test_gpu_vit_matrix.py compares the kernels with.  CPU torch only; nothing here is taken from what the kernels return,
with one stated exception (EXP_ULPS below).  U = 2^-24 is the unit roundoff of fp32, half a bf16 ulp is at most 2^-8 relative (8 significant bits).  The
library is compiled with -ffp-contract=off: a product and a sum are fused only where the source says fmaf.

What each entry writes (from the kernel code; the GPU test pre-fills every output with a NaN pattern and checks both sides):
    attention          ctx[r * ldo + c] for r < B T, c < heads * hd; columns heads * hd .. ldo of a row are not written
    add_layernorm      h[r * D + c] for r < M, c < D when delta is given (h is read only otherwise); out[r * Dp + c] for c < D
                       when out is given: columns D .. Dp are not written
    vit_embed_ln       h[r * D + c], r < B T, c < D (row b T of image b from cls, the others from proj rows of pitch Dp)
    vit_patchify       rows[i], i < B G G Kp, zero where k >= C ps ps
    vit_tokens_to_grid out[i], i < B (T - 1) Dp, zero where c >= D
    bilinear_fwd / bwd every element of y [B, OH, OW, Cp] / dx [B, IH, IW, Cp]; padding channels are zero because those of the
                       input are

Attention.  q, k, v hold bf16-representable values, so both dtypes see the same numbers; s = fl32(hd^-1/2) is the scale the
entry is given.  With S_ij = s q_i . k_j, m_i = max_j S_ij, w_ij = softmax_j and out_id = sum_j w_ij v_jd in float64:
  scores.   attention_kernel scales q first (one rounding), then runs two fmaf chains of hd / 2 and adds them:
                e_s(i, j) = (hd / 2 + 2) U A_ij,   A_ij = s sum_d |q_id k_jd|
            attention_mfma_kernel: products of bf16 values are exact in fp32, the matrix core adds hd = 64 of them:
                e_s(i, j) = 64 U A_ij
  exponent. p = exp(S_ij - m): the subtraction, the product with log2(e) (with the scale folded in for the MFMA kernel: the
            constant carries 2 roundings) and the constants each move the exponent by at most U |S_ij - m| relative to the
            result, 4 U x_ij in all with x_ij = m_i - S_ij; the running maximum a key meets is never above m_i, so x_ij
            bounds the argument at every trip.  The hardware exp2 behind __expf / exp2f is off by at most EXP_ULPS ulp:
            2 EXP_ULPS U relative.       eta_ij = e_s(i, j) + 4 U x_ij + 2 EXP_ULPS U
            The rescaling factors corr (and the merge factors of attention_kernel) multiply numerator and denominator
            alike: their own error cancels in the quotient, only the roundings of the multiplications stay (next term).
            A weight off by (1 + eta) relative moves the quotient by  sum_j w_ij eta_ij |v_jd| + |out_id| sum_j w_ij eta_ij.
  sums.     attention_kernel, per trip of a wave: one rounding for acc * corr, four fmaf; l alike; the merge: 4 fmaf for the
            numerator, 4 for L, the division (up to 2 ulp: 4 U) and the product: with n = most trips of a wave,
                (10 n + 13) U sum_j w_ij |v_jd|
            attention_mfma_kernel, per key block: o * corr, two MFMAs adding 16 exact products each (33 roundings); l: corr,
            16 adds, the add to l (18); the half-wave add, the division, the product (6):   (51 n + 6) U sum_j w_ij |v_jd|
  P in bf16 (MFMA kernel only): the numerator takes P rounded to bf16, l sums the unrounded values: 2^-8 sum_j w_ij |v_jd|
            (half a bf16 ulp is 2^-8 of a value at the bottom of its binade).  The rising ramp attains it: its weight sits on
            one or two keys with p near 1.
  storage.  bf16: half a bf16 ulp of |out| + everything above; fp32: the final product is counted under "sums".
The bound is e_arith + e_round: e_arith holds the score, exponent and sums terms (worst cases of fp32 arithmetic that real
data stays far below), e_round the two roundings to bf16 (P and the store), which single elements attain in full.
EXP_ULPS cannot be derived from the code, and the measurement asked for does not calibrate it either: it is a placeholder of
1, the smallest positive integer, not a measured property of the device's exp2.  The rule was the smallest integer for which
the worst error / bound of the dense and ramp runs on the MI355X stays at or below 0.5 (a factor of two for data dependence).
Over the 1.1e7 exponentials of those runs the worst ratio moves by less than 0.001 between EXP_ULPS = 0 and 8, because the
score and sums terms lead e_arith: any small integer passes, so the run says only that 1 is not too small.
  With fp32 storage e_round = 0 and the 0.5 is a condition on error / bound itself.  With bf16 storage e_round leads the bound
and is attained, so error / bound approaches 1 whatever the arithmetic does (MI355X: up to 0.99 for bf16/32, 0.75 for
bf16/64); there the 0.5 is put on the part it was meant for:  error <= 0.5 e_arith + e_round  at every element.
tests/test_gpu_vit_matrix.py asserts error / bound <= 1 and (error - e_round) / e_arith <= 0.5 on every dense and ramp case
of all four instances; both figures are recorded in profiles/vit_resize_matrix_parity.txt ("arith" rows).  Measured on the
MI355X, worst (error - e_round) / e_arith:  fp32/64 0.0094,  fp32/32 0.1716,  bf16/32 0.1164,  bf16/64 0.0000.  For the
matrix-core kernel that 0 says its e_round (the worst case of P's rounding over all keys, plus the store) covers the whole
error at every element: the condition is then no sharper than error / bound <= 1, and no arithmetic-only statement about
that kernel follows from the dense and ramp runs.  What pins its masks and fragment layout is the routed and uniform designs,
which are exact.
  The exact designs (routed, uniform at a power-of-two T) need no bound: see routed_inputs and uniform_inputs.  Uniform at
other T: out = fl(A * fl(1 / T)) with A the exact integer sum: 4 U for the division and U for the product, 6 U |out| with slack.

LayerNorm (add_layernorm and vit_embed_ln).  The row v the statistics see is restated exactly in float32 (the fixed-order sum
h + delta_0 + delta_1 + ..., or e + pos).  With n_m the depth of the chain that adds the row (float4 / channels per lane, the
pair sums, 6 shuffle steps, the division) and n_v that of the squared deviations:
    e_mean = n_m U sum |v| / D
    d = v - mean:            e_d = e_mean + U |d|
    var = sum d^2 / D:       e_var = 2 e_mean sum |d| / D + (n_v + 2) U var
    rstd = rsqrt(var + eps): e_rstd = 6 U rstd + rstd^3 e_var / 2             (the sum with eps, rsqrtf of up to 2 ulp)
    t = d rstd:              e_t = e_d rstd + |d| e_rstd + U |t|
    o = t gamma + beta:      e_o = (e_t |gamma| + U |t gamma|) + U |o|,  then half an ulp of the storage type
A one-pass variance (mean of squares minus squared mean) is outside this bound on the offset design (mean 4096, spread 1: the
squares need 25 bits), which the host test shows.  A constant row has d == 0 exactly (the sum of D equal small integers and
its division by D are exact), so out == beta.

Bilinear.  The source index and lambda are restated in float32 exactly as src_index computes them, and the float64 weights
(1 - lambda, lambda) are built from that float32 lambda.  The fp32 forward is restated operation by operation and must be equal;
in bf16 the same value is rounded once more.  Against float64 (bf16 forward, both backward forms): a weight carries at most 5
roundings (1 - lambda twice, the sum of two taps that fall on one pixel twice, the product), the 2-D gather adds its n_y n_x
taps with one fmaf each, the separable form n_x and then n_y (+ 2 for the weights of each pass):
    (max(n_y n_x, n_y + n_x) + 8) U sum |w| |g|,  then half an ulp of the storage type; forward: 12 U sum |w| |x|."""
import zlib

import torch

from bn_reference import U24, half_ulp
from stem_pool_reference import rne_bf16
from vit_cases import (ROUTED_BITS, attn_acc_trips, attn_is_mfma, attn_pitches, embed_per, ln_per4, routed_reps, routed_target)

U = U24
EXP_ULPS = 1                    # a placeholder, not a calibrated value: see the docstring


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _uniform(g, shape, lo, hi):
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def storage_bound(ref, e32, dtype):
    """e32 + half an ulp of the storage type (fp32: the last fp32 rounding is part of e32)"""
    return e32 + half_ulp(ref.abs() + e32, torch.bfloat16) if dtype == "bf16" else e32


# ---- attention -------------------------------------------------------------------------------------------------------------
def attn_scale(hd):
    return float(torch.tensor(hd ** -0.5, dtype=torch.float32))


def routed_scale_c(hd):
    """the power of two c with 2 c reps scale > 200: the gap between the target's score and any other, scaled"""
    c = 1
    while 2 * c * routed_reps(hd) * attn_scale(hd) <= 200:
        c *= 2
    return c


def routed_code(T):
    j = torch.arange(T)
    return torch.stack([((j >> b) & 1).float() * 2 - 1 for b in range(ROUTED_BITS)], 1)        # [T, bits] of +-1


def routed_inputs(c):
    """-> q, k, v [B, heads, T, hd] fp32 and the wanted output V[pi(i)].  Scores are integers times fl(scale) c, all exact in
    fp32; the target's score leads every other by more than 200 after scaling, so every other probability is exp(< -200) = 0
    in fp32 and the target's is exp(0) = 1; the shift dimension puts every real score below -200, a zero K row (score 0) wins"""
    T, hd, reps, cc = c.T, c.hd, routed_reps(c.hd), routed_scale_c(c.hd)
    code = routed_code(T).repeat(1, reps)                                    # [T, reps * bits]
    pi = torch.tensor([routed_target(i, T) for i in range(T)])
    k = torch.zeros((c.B, c.heads, T, hd))
    q = torch.zeros_like(k)
    k[..., :reps * ROUTED_BITS] = code
    k[..., hd - 1] = 1.0
    q[..., :reps * ROUTED_BITS] = cc * code[pi]
    shift = 1
    while shift < 2 * cc * reps * ROUTED_BITS:
        shift *= 2
    q[..., hd - 1] = -float(shift)
    j = torch.arange(T).view(1, 1, T, 1)
    d = torch.arange(hd).view(1, 1, 1, hd)
    b = torch.arange(c.B).view(-1, 1, 1, 1)
    h = torch.arange(c.heads).view(1, -1, 1, 1)
    v = ((((j >> (8 * (d & 1))) + 5 * d + 3 * h + 7 * b) & 0xFF) - 128).float()         # even dims: low byte of j, odd: high
    return q, k, v, v[:, :, pi, :].clone()


def uniform_inputs(c):
    """every key of a head is the same +-1 vector, so the scores of a query are one value computed one way: all p = exp(0) = 1,
    l = T and the numerator the exact integer sum of V"""
    g = _gen("attn-uniform", tuple(c))
    u = _ints(g, (c.B, c.heads, 1, c.hd), 0, 1) * 2 - 1
    k = u.expand(c.B, c.heads, c.T, c.hd).clone()
    q = _ints(g, (c.B, c.heads, c.T, c.hd), -3, 3)
    v = _ints(g, (c.B, c.heads, c.T, c.hd), -8, 8)
    return q, k, v


def uniform_expected(c, v):
    """-> (mean over keys in float64, bound): 0 where T is a power of two"""
    ref = v.double().mean(2, keepdim=True).expand(-1, -1, c.T, -1)
    if c.T & (c.T - 1) == 0:
        return ref, torch.zeros_like(ref)
    return ref, storage_bound(ref, 6 * U * ref.abs(), c.dtype)


def ramp_inputs(c, rising):
    """scaled scores g_i r_j: r runs over [-1, 1] along the keys (rising, or falling), g_i in [40, 80]"""
    g = _gen("attn-ramp", tuple(c))
    T, hd = c.T, c.hd
    u = _ints(g, (c.B, c.heads, 1, hd), 0, 1) * 2 - 1
    r = torch.linspace(-1, 1, T) if T > 1 else torch.ones(1)
    r = r if rising else r.flip(0)
    gi = 40 + 40 * ((torch.arange(T) * 7) % T).float() / T
    k = rne_bf16((r.view(1, 1, T, 1) * u).contiguous())
    q = rne_bf16((gi.view(1, 1, T, 1) / (hd * attn_scale(hd)) * u).contiguous())
    v = rne_bf16(_uniform(g, (c.B, c.heads, T, hd), -1, 1))
    return q, k, v


def dense_inputs(c):
    g = _gen("attn-dense", tuple(c))
    shape = (c.B, c.heads, c.T, c.hd)
    return tuple(rne_bf16(_uniform(g, shape, -2, 2)) for _ in range(3))


def attn_inputs(c, design):
    if design == "routed":
        return routed_inputs(c)[:3]
    if design == "uniform":
        return uniform_inputs(c)
    if design in ("ramp_up", "ramp_down"):
        return ramp_inputs(c, design == "ramp_up")
    return dense_inputs(c)


def pack_qkv(c, q, k, v):
    """-> [B T, ldq] fp32: q | k | v of all heads side by side; the pitch columns hold NaN (nothing may read them)"""
    ldq, _ = attn_pitches(c)
    D = c.heads * c.hd
    out = torch.full((c.B * c.T, ldq), float("nan"))
    for n, t in enumerate((q, k, v)):
        out[:, n * D:(n + 1) * D] = t.permute(0, 2, 1, 3).reshape(c.B * c.T, D)
    return out


def unpack_ctx(c, ctx):
    """[B T, D] -> [B, heads, T, hd]"""
    return ctx.reshape(c.B, c.T, c.heads, c.hd).permute(0, 2, 1, 3)


def attention_reference(q, k, v, scale, dtype=torch.float64):
    """-> (out, w, S): softmax(q k^T scale) v with the score matrix and the weights"""
    S = (q.to(dtype) @ k.to(dtype).transpose(-1, -2)) * scale
    w = torch.softmax(S, -1)
    return w @ v.to(dtype), w, S


def attention_terms(c, q, k, v, scale, exp_ulps=EXP_ULPS):
    """-> (out float64, e_arith, e_round) of a dense or ramp run; the docstring derives the terms"""
    out, w, S = attention_reference(q, k, v, scale)
    A = (q.double().abs() @ k.double().abs().transpose(-1, -2)) * scale
    x = S.max(-1, keepdim=True).values - S
    n = attn_acc_trips(c)
    if attn_is_mfma(c):
        e_s, k_acc, p_bf = 64 * U * A, 51 * n + 6, 2.0 ** -8
    else:
        e_s, k_acc, p_bf = (c.hd // 2 + 2) * U * A, 10 * n + 13, 0.0
    weta = w * (e_s + 4 * U * x + 2 * exp_ulps * U)
    wv = w @ v.double().abs()
    e_arith = (weta @ v.double().abs() + out.abs() * weta.sum(-1, keepdim=True) + k_acc * U * wv) * 1.001
    e32 = e_arith + p_bf * wv * 1.001
    return out, e_arith, storage_bound(out, e32, c.dtype) - e_arith


def attention_bound(c, q, k, v, scale, exp_ulps=EXP_ULPS):
    """-> (out float64, bound = e_arith + e_round)"""
    out, e_arith, e_round = attention_terms(c, q, k, v, scale, exp_ulps)
    return out, e_arith + e_round


def mutant_key(design, T):
    """the key a mutant acts on: one that carries weight -- the last key of the rising ramp, the first of the falling one
    (the other end has weight exp(-80) or less), a middle key of the dense run"""
    return {"ramp_up": T - 1, "ramp_down": 0}.get(design, T // 2)


def attention_mutants(q, k, v, at=None):
    """the three subtly wrong attentions of the issue as (name, q, k, v): (a) key `at` dropped (the last one by default),
    (b) one zero-score key (zero K and V rows, what a padding key let through the mask is) added, (c) V row `at` swapped
    with its neighbour"""
    T = k.shape[2]
    at = T - 1 if at is None else at
    out = []
    if T >= 2:
        keep = [j for j in range(T) if j != at]
        out.append(("a", q, k[:, :, keep], v[:, :, keep]))
    z = torch.zeros_like(k[:, :, :1])
    out.append(("b", q, torch.cat([k, z], 2), torch.cat([v, z], 2)))
    if T >= 2:
        perm = list(range(T))
        other = at + 1 if at + 1 < T else at - 1
        perm[at], perm[other] = other, at
        out.append(("c", q, k, v[:, :, perm]))
    return out


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
def ln_reference(v, gamma, beta, eps, n_m, n_v, dtype):
    """v [M, D] fp32 (the exact row the kernel normalises) -> (out float64, bound)"""
    D = v.shape[1]
    v = v.double()
    g, b = gamma.double(), beta.double()
    mean = v.mean(1, keepdim=True)
    d = v - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    t = d * rstd
    o = t * g + b
    e_mean = n_m * U * v.abs().mean(1, keepdim=True)
    e_d = e_mean + U * d.abs()
    e_var = 2 * e_mean * d.abs().mean(1, keepdim=True) + (n_v + 2) * U * var
    e_rstd = 6 * U * rstd + rstd ** 3 * e_var / 2
    e_t = e_d * rstd + d.abs() * e_rstd + U * t.abs()
    e_o = e_t * g.abs() + U * (t * g).abs() + U * o.abs()
    return o, storage_bound(o, e_o, dtype)


def add_ln_chain(D):
    """(n_m, n_v) of add_layernorm_kernel: per float4 two pair sums and the add to s, 6 shuffles, the division; 4 fmaf per
    float4, 6 shuffles, the division"""
    p = ln_per4(D)
    return 3 * p + 7, 4 * p + 7


def embed_chain(D):
    p = embed_per(D)
    return p + 7, p + 7


def ln_one_pass_f32(v, gamma, beta, eps):
    """the mutant: var = mean(v^2) - mean(v)^2 in float32"""
    mean = v.mean(1, keepdim=True)
    var = ((v * v).mean(1, keepdim=True) - mean * mean).clamp(min=0)
    return (v - mean) * (var + eps).rsqrt() * gamma + beta


def ln_params(D, key, const_gamma=False):
    g = _gen("ln-params", D, key)
    gamma = torch.full((D,), 1.5) if const_gamma else _uniform(g, (D,), 0.5, 1.5) * torch.where(torch.arange(D) % 5 == 4, -1.0, 1.0)
    beta = torch.zeros(D) if const_gamma else _uniform(g, (D,), -0.5, 0.5)
    return gamma, beta


def ln_rows(design, g, shape, dtype_round):
    """an [.., D] fp32 block of the design; dtype_round rounds what is stored in the compute dtype"""
    if design == "lattice":
        return _ints(g, shape, -8, 8)
    if design == "dense":
        return dtype_round(_uniform(g, shape, -2, 2))
    raise ValueError(design)


def add_ln_inputs(c, design):
    """-> (h0 [M, D] fp32, parts [nparts, M, Dp] fp32 holding values of the dtype; pitch columns NaN)"""
    g = _gen("add-ln", design, tuple(c))
    rnd = rne_bf16 if c.dtype == "bf16" else (lambda t: t)
    M, D = c.M, c.D
    parts = torch.full((c.nparts, M, c.Dp), float("nan"))
    if design in ("lattice", "dense"):
        h0 = ln_rows(design, g, (M, D), lambda t: t)
        parts[:, :, :D] = ln_rows(design, g, (c.nparts, M, D), rnd)
    elif design == "constant":                 # h + sum of the parts is one small integer along each row
        h0 = _ints(g, (M, 1), -3, 3).expand(M, D).clone()
        parts[:, :, :D] = _ints(g, (c.nparts, M, 1), -2, 2).expand(c.nparts, M, D)
    else:                                       # offset: mean 4096, spread +-1 (the parts add small bf16-representable values)
        h0 = 4096 + _uniform(g, (M, D), -1, 1)
        parts[:, :, :D] = rnd(_uniform(g, (c.nparts, M, D), -0.125, 0.125))
    return h0, parts


def add_chain_f32(h0, parts, D):
    """the updated h: h0 + part 0 + part 1 + ... in float32, in that order"""
    h = h0.clone()
    for p in parts:
        h = h + p[:, :D]
    return h


def embed_inputs(c, design):
    """-> (proj [B (T - 1), Dp] fp32 of dtype values with NaN pitch columns, cls [D], pos [T, D])"""
    g = _gen("embed", design, tuple(c))
    rnd = rne_bf16 if c.dtype == "bf16" else (lambda t: t)
    B, T, D = c.B, c.T, c.D
    proj = torch.full((B * (T - 1), c.Dp), float("nan"))
    if design in ("lattice", "dense"):
        proj[:, :D] = ln_rows(design, g, (B * (T - 1), D), rnd)
        cls = ln_rows(design, g, (D,), lambda t: t) + (100 if design == "lattice" else 0)
        cls[::2] *= -1                                                     # a spread row however large the offset
        pos = ln_rows(design, g, (T, D), lambda t: t)
    elif design == "constant":
        proj[:, :D] = _ints(g, (B * (T - 1), 1), -3, 3).expand(-1, D)
        cls = torch.full((D,), 5.0)
        pos = _ints(g, (T, 1), -2, 2).expand(T, D).clone()
    else:
        proj[:, :D] = rnd(4096 + _uniform(g, (B * (T - 1), D), -1, 1))
        cls = 4096 + _uniform(g, (D,), -1, 1)
        pos = _uniform(g, (T, D), -1, 1)
    return proj, cls, pos


def embed_rows_f32(c, proj, cls, pos):
    """[B T, D] fp32: e + pos with e = cls for token 0 and image b's proj row t - 1 otherwise (one rounding)"""
    B, T, D = c.B, c.T, c.D
    e = torch.cat([cls.view(1, 1, D).expand(B, 1, D), proj[:, :D].reshape(B, T - 1, D)], 1)
    return (e + pos.view(1, T, D)).reshape(B * T, D)


# ---- pure movement ---------------------------------------------------------------------------------------------------------
def to_dtype(x, dtype):
    return rne_bf16(x) if dtype == "bf16" else x


def coord_code(*dims):
    """[*dims] fp32: (i_last + 16 i_(last - 1) + 67 i_(last - 2) + 131 i_(last - 3)) mod 251 - 125.  Integers of at most 7
    bits, so bf16 keeps them, and 251 is prime: an element moved by fewer than 251 places along any one dimension shows"""
    coef = (1, 16, 67, 131)
    assert len(dims) <= len(coef)
    v = torch.zeros(dims, dtype=torch.int64)
    for n, size in enumerate(reversed(dims)):
        shape = [1] * len(dims)
        shape[len(dims) - 1 - n] = size
        v = v + coef[n] * torch.arange(size).view(shape)
    return (v % 251 - 125).float()


def patch_input(c):
    """fp32: x[b, c, y, x] = its own linear index (below 2^24: exact in fp32), so a misplaced element names where it came
    from.  bf16 would round that to 8 bits and neighbours would coincide: there x is the coordinate code, which still tells
    any element from its neighbours in every dimension"""
    if c.dtype == "bf16":
        return coord_code(c.B, c.C, c.H, c.W)
    n = c.B * c.C * c.H * c.W
    assert n < 2 ** 24
    return torch.arange(n, dtype=torch.float32).reshape(c.B, c.C, c.H, c.W)


def patchify_reference(c, x):
    G, ps = c.H // c.ps, c.ps
    K = c.C * ps * ps
    p = x[:, :, :G * ps, :G * ps].reshape(c.B, c.C, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(c.B * G * G, K)
    out = torch.zeros((c.B * G * G, c.Kp))
    out[:, :K] = p
    return to_dtype(out, c.dtype)


def grid_input(c):
    """as patch_input: linear indices in fp32, the coordinate code in bf16"""
    if c.dtype == "bf16":
        return coord_code(c.B, c.T, c.D)
    n = c.B * c.T * c.D
    assert n < 2 ** 24
    return torch.arange(n, dtype=torch.float32).reshape(c.B, c.T, c.D)


def grid_reference(c, h):
    out = torch.zeros((c.B, c.T - 1, c.Dp))
    out[:, :, :c.D] = h[:, 1:, :]
    return to_dtype(out, c.dtype)


# ---- bilinear --------------------------------------------------------------------------------------------------------------
def src_index_f32(out_size, in_size):
    """src_index of resize.hip for o = 0 .. out_size - 1, in float32: (i0, i1 int64, lambda float32)"""
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size), dtype=torch.float32)
    o = torch.arange(out_size, dtype=torch.float32)
    s = scale * (o + 0.5) - 0.5
    s = torch.where(s < 0, torch.zeros_like(s), s)
    i0 = s.to(torch.int64).clamp(max=in_size - 1)
    i1 = i0 + (i0 < in_size - 1).long()
    return i0, i1, s - i0.float()


def weight_matrix(out_size, in_size):
    """[out, in] float64: (1 - lambda) at i0 plus lambda at i1, lambda the float32 value"""
    i0, i1, lam = src_index_f32(out_size, in_size)
    W = torch.zeros((out_size, in_size), dtype=torch.float64)
    r = torch.arange(out_size)
    W[r, i0] += 1.0 - lam.double()
    W[r, i1] += lam.double()
    return W


def bilinear_inputs(c, design):
    """-> (x [B, IH, IW, Cp], dy [B, OH, OW, Cp]) fp32 of dtype values, padding channels zero"""
    g = _gen("bilinear", design, tuple(c))
    if design == "lattice":
        x, dy = _ints(g, (c.B, c.IH, c.IW, c.Cp), -8, 8), _ints(g, (c.B, c.OH, c.OW, c.Cp), -8, 8)
    else:
        x, dy = (to_dtype(_uniform(g, s, -2, 2), c.dtype) for s in ((c.B, c.IH, c.IW, c.Cp), (c.B, c.OH, c.OW, c.Cp)))
    x[..., c.C:] = 0
    dy[..., c.C:] = 0
    return x, dy


def bilinear_fwd_f32(c, x):
    """the forward kernel's expression in float32, operation by operation (no contraction)"""
    y0, y1, ly = src_index_f32(c.OH, c.IH)
    x0, x1, lx = src_index_f32(c.OW, c.IW)
    ly, lx = ly.view(1, -1, 1, 1), lx.view(1, 1, -1, 1)
    one = torch.tensor(1.0)
    w00, w01, w10, w11 = (one - ly) * (one - lx), (one - ly) * lx, ly * (one - lx), ly * lx
    f = lambda yy, xx: x[:, yy][:, :, xx]
    return w00 * f(y0, x0) + w01 * f(y0, x1) + w10 * f(y1, x0) + w11 * f(y1, x1)


def bilinear_fwd_reference(c, x, absolute=False):
    Wy, Wx = weight_matrix(c.OH, c.IH), weight_matrix(c.OW, c.IW)
    xd = x.double().abs() if absolute else x.double()
    t = torch.einsum("oi,bijc->bojc", Wy, xd)
    return torch.einsum("pj,bojc->bopc", Wx, t)


def bilinear_bwd_reference(c, dy, absolute=False, Wy=None, Wx=None):
    Wy = weight_matrix(c.OH, c.IH) if Wy is None else Wy
    Wx = weight_matrix(c.OW, c.IW) if Wx is None else Wx
    g = dy.double().abs() if absolute else dy.double()
    t = torch.einsum("pj,bopc->bojc", Wx, g)
    return torch.einsum("oi,bojc->bijc", Wy, t)


def bilinear_fwd_bound(c, x, ref):
    return storage_bound(ref, 12 * U * bilinear_fwd_reference(c, x, absolute=True), c.dtype)


def bilinear_bwd_bound(c, dy, ref):
    Wy, Wx = weight_matrix(c.OH, c.IH), weight_matrix(c.OW, c.IW)
    ny, nx = (Wy != 0).sum(0).double().view(1, -1, 1, 1), (Wx != 0).sum(0).double().view(1, 1, -1, 1)
    taps = torch.maximum(ny * nx, ny + nx) + 8
    return storage_bound(ref, taps * U * bilinear_bwd_reference(c, dy, absolute=True), c.dtype)


def bilinear_bwd_mutant(c, dy):
    """one tap's weight moved to its neighbour: output row OH / 2 gives its i0 weight to i1 (or to i0 - 1 at the border)"""
    Wy = weight_matrix(c.OH, c.IH)
    if c.IH < 2:
        return None
    o = c.OH // 2
    i0 = int(src_index_f32(c.OH, c.IH)[0][o])
    to = i0 + 1 if i0 + 1 < c.IH else i0 - 1
    Wy[o, to] += Wy[o, i0]
    Wy[o, i0] = 0
    return bilinear_bwd_reference(c, dy, Wy=Wy)
