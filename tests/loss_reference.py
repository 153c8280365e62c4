"""float64 references, analytic gradients, launch arithmetic and derived error bounds for the kernels of csrc/head.hip and csrc/loss.hip
(output head, CrossEntropy + soft Dice, probability-mode Dice + NLL, prompt remix), shared by tests/test_loss_reference_host.py
and tests/test_gpu_head_loss_matrix.py.  CPU torch only.  Nothing here is taken from what the kernels return.

Semantics (restated from oracle/losses_ref.py, oracle/prompt_ref.py and the header comment of loss.hip), on logits or
probabilities x [N, C, HW] and labels y [N, HW]:

  p        = softmax(x) over C, or x itself in probability mode
  onehot_k = [y == k] for k in [0, C): a label outside [0, C) (-100, 255, C) belongs to no class
  I_k = sum p_k * onehot_k, Sp_k = sum p_k, Sg_k = sum onehot_k over ALL pixels (Dice does not mask pixels)
  den_raw_k = Sp_k + Sg_k + smooth;  dc_k = (2 I_k + smooth) / max(den_raw_k, 1e-8)
  a_k  = w_k / sum of w over the classes that count (every class except an ignore_index inside [0, C); w = class weights or 1;
         with class weights the sum is clamped to 1e-8 from below);  dice = -sum a_k dc_k
  ce   = sum w[y] nll / sum w[y] over the pixels with y in [0, C) and y != ignore_index (NaN when there are none, like torch);
         nll = logsumexp(x) - x_y, or -log(x_y + eps) / -x_y in probability mode (nll_log = 1 / 0)
  loss = dice_weight * dice + ce_weight * ce; with ce_weight = 0 (the Dice-only losses, which never evaluate a CrossEntropy in
         the reference project) the CrossEntropy term is absent, whatever ce is
  state = [loss, ce, dice, ce_den, dc[8], den_raw[8], a[8]]

The scalar parameters (smooth, the two weights, eps, the upstream gradient) are used as the fp32 values the kernels receive.

Gradient (dice with respect to p is G0_k + onehot_k G1_k, G0 = a dc / den_raw, G1 = -2 a / den_raw; with the clip active the
denominator is a constant: G0 = 0, G1 = -2 a / 1e-8), carried through the softmax, plus w[y] / ce_den * (p - onehot) of the
CrossEntropy (probability mode: -w[y] / ce_den / (x_y + eps) or -w[y] / ce_den on the label's class), times the upstream
gradient.  A pixel that does not count for the CrossEntropy gets no CrossEntropy gradient: with every pixel ignored the loss is
NaN and the gradient is the finite Dice part alone (torch's cross_entropy gives zeros there as well).  A pixel that counts while
the weights of all counted pixels sum to zero gets w[y] / ce_den = 0 / 0 = NaN, as torch's nll_loss backward gives; with
ce_weight = 0 there is no CrossEntropy term and no such NaN.

Error bounds follow the summation structure of loss_fwd_kernel: a thread adds n_t = ceil(P / (blocks * 1024)) terms in fp32, the
wave butterfly six more levels, thread i of the block the sixteen wave rows, the finishing block the block rows in float64, and
each state entry is rounded once to fp32: CHAIN(P) = n_t + 6 + 15 + 3 unit roundoffs on the sum of the absolute terms (the 3:
float64 stage, final rounding, second-order slack).  Sums whose terms are small integers (label counts, unweighted pixel counts)
are exact below 2^24 per block row and carry no error at all.

What cannot be derived from the project is the per-pixel accuracy of the device's expf / logf.  It is MEASURED, on the host,
as what fp32 CPU torch (the oracle's arithmetic) shows against float64 on the very inputs of a case, in the units in which
such an evaluation errs (the argument x - max is rounded before the exponential, so the relative error of p grows with
|x - max|):

  k_sm  = max |softmax32 - p| / (2^-24 * p * (C + max - x))                    over p > 1e-30
  k_nll = max |nll32 - nll|   / (2^-24 * (C + (max - x_y) + nll))              softmax mode
  k_log = max |log32(x + eps) - log(x + eps)| / (2^-24 * (1 + |log(x + eps)|))  probability mode, nll_log = 1
  k_mix = max |remix32 - remix| / (2^-24 * (1 + |mask logit|))                  prompt remix (outputs in [0, 1])

(the C in the first two: the sum of the C exponentials is an fp32 chain in the oracle and in the kernels alike).  Measured over
the whole case matrix of tests/test_gpu_head_loss_matrix.py -- C = 1..8, every pixel count and both input families, the +-80,
all-equal and the other edge cases, the three remix shapes: k_sm <= 1.073, k_nll <= 0.937, k_log <= 0.971, k_mix <= 2.104
(tests/test_loss_reference_host.py measures again and asserts that no case exceeds a quarter of the constants).  The device math
library may differ from the host's by a few ulp, so the bounds allow 4 x the measured value, rounded up to two digits:
K_SM = 4.3, K_NLL = 3.8, K_LOG = 3.9, K_MIX = 8.5.  A probability that underflows fp32 (the +-80 case) is covered by an
absolute 2^-126.

Head: logits = bias + sum_c y_c W_kc is one fmaf chain over the Cp staged channels starting from the bias (padded terms are exact
zeros): (C + 1) * 2^-24 * (|bias| + sum |y W|); dy is a chain of ncls fmaf plus half an ulp of the store dtype; dW, db and the two
BatchNorm sums are per-thread chains of n_t = ceil(P / (blocks * rows)) terms, then `rows` partials added in fp32 by one thread,
then the block rows in float64 and one fp32 rounding: (n_t + rows + 4) * 2^-24 * sum |term| plus what each term carries in."""
import torch

from bn_reference import U24, apply_reference, half_ulp

MAXC = 8
K_SM, K_NLL, K_LOG, K_MIX = 4.3, 3.8, 3.9, 8.5
TINY = 2.0 ** -126
F64 = torch.float64


def f32(v):
    """the fp32 value of a scalar parameter, as a Python float"""
    return torch.tensor(float(v), dtype=torch.float32).item()


# ---------------------------------------------------------------------------------------- launch arithmetic
def loss_launch(P):
    """segk_loss_blocks: (blocks = partial rows, terms per thread chain, wave rows per block)."""
    nb = min(max(-(-P // 4096), 1), 256)
    return nb, -(-P // (nb * 1024)), 16


def loss_bwd_launch(P):
    """loss_bwd_kernel / prompt remix / head forward: (blocks of 256 threads, passes of the grid stride)."""
    g = min(-(-P // 256), 4096)
    return g, -(-P // (g * 256))


def head_blocks(P):
    """segk_head_blocks (= segk_head_bwd_blocks)"""
    return min(-(-P // 32), 1024)


def head_lane_geometry(Cp):
    """lane_geometry(cvec, 64) of csrc/channel_lanes.hpp as head.hip calls it: (channel vectors per block, pixel rows per block, channel slices); four channels per
    thread in both dtypes."""
    cvec = Cp // 4
    cvb = min(cvec, 64)
    return cvb, 256 // cvb, -(-cvec // cvb)


def head_bwd_launch(P, Cp):
    """(blocks, terms per thread chain, rows)"""
    rows = head_lane_geometry(Cp)[1]
    nb = head_blocks(P)
    return nb, -(-P // (nb * rows)), rows


def confusion_launch(P):
    g = min(-(-P // 256), 1024)
    return g, -(-P // (g * 256))


def chain(P):
    nb, n_t, _ = loss_launch(P)
    return n_t + 6 + 15 + 3


# ---------------------------------------------------------------------------------------- loss: forward
def loss_reference(x, y, C=None, cw=None, ignore_index=None, smooth=1e-5, dice_weight=1.0, ce_weight=1.0, prob=False, nll_log=1,
                   eps=0.0):
    """x [N, C, HW] fp32 (or float64), y [N, HW] int64 -> dict of float64 results (see the module docstring) plus the per-pixel
    quantities the gradient and the bounds need."""
    x = x.to(F64)
    N, C, HW = x.shape
    y = y.reshape(N, HW).long()
    ign = -1 if ignore_index is None else int(ignore_index)
    smooth, dwt, cwt, eps = f32(smooth), f32(dice_weight), f32(ce_weight), f32(eps)
    w = torch.ones(C, dtype=F64) if cw is None else cw.float().to(F64)
    ks = torch.arange(C).view(1, C, 1)
    oh = (y.unsqueeze(1) == ks).to(F64)
    m = x.max(1, keepdim=True).values
    if prob:
        p = x
        lse = None
    else:
        e = torch.exp(x - m)
        se = e.sum(1, keepdim=True)
        p = e / se
        lse = torch.log(se) + m
    I, Sp, Sg = (p * oh).sum((0, 2)), p.sum((0, 2)), oh.sum((0, 2))
    den_raw = Sp + Sg + smooth
    clip = den_raw < 1e-8
    den = torch.where(clip, torch.full_like(den_raw, 1e-8), den_raw)
    dc = (2 * I + smooth) / den
    valid = torch.ones(C, dtype=torch.bool)
    if 0 <= ign < C:
        valid[ign] = False
    wsum = (w * valid).sum()
    if cw is not None:
        wsum = wsum.clamp(min=1e-8)
    a = w * valid / wsum
    dice = -(a * dc).sum()
    counts = (y >= 0) & (y < C) & (y != ign)
    yc = torch.where(counts, y, torch.zeros_like(y))
    xy = x.gather(1, yc.unsqueeze(1)).squeeze(1)
    if prob:
        nll = -torch.log(xy + eps) if nll_log else -xy
    else:
        nll = lse.squeeze(1) - xy
    wy = w[yc] * counts
    cden = wy.sum()
    num =torch.where(counts, wy * nll, torch.zeros_like(nll)).sum()
    ce = num / cden if cden > 0 else torch.tensor(float("nan"), dtype=F64)
    loss = dwt * dice + (cwt * ce if cwt != 0 else 0.0)
    state = torch.zeros(4 + 3 * MAXC, dtype=F64)
    state[0], state[1], state[2], state[3] = loss, ce, dice, cden
    state[4:4 + C], state[4 + MAXC:4 + MAXC + C], state[4 + 2 * MAXC:4 + 2 * MAXC + C] = dc, den_raw, a
    return dict(N=N, C=C, HW=HW, P=N * HW, x=x, y=y, p=p, oh=oh, m=m, w=w, a=a, I=I, Sp=Sp, Sg=Sg, den_raw=den_raw, den=den, clip=clip,
                dc=dc, dice=dice, ce=ce, ce_den=cden, ce_num=num, ce_abs=torch.where(counts, (wy * nll).abs(), torch.zeros_like(nll)).sum(),
                loss=loss, state=state, counts=counts, yc=yc, xy=xy, nll=nll, wy=wy, prob=prob, nll_log=int(nll_log), eps=eps,
                smooth=smooth, dice_weight=dwt, ce_weight=cwt, weighted=cw is not None)


def loss_grad_reference(r, gout=1.0):
    """analytic d loss / d x [N, C, HW] float64, times the fp32 upstream gradient; also the pieces the bound needs"""
    go = f32(gout)
    a, dc, den_raw = r["a"], r["dc"], r["den_raw"]
    G0 = torch.where(r["clip"], torch.zeros_like(dc), a * dc / torch.where(r["clip"], torch.ones_like(den_raw), den_raw))
    G1 = torch.where(r["clip"], -2 * a / 1e-8, -2 * a / torch.where(r["clip"], torch.ones_like(den_raw), den_raw))
    g = G0.view(1, -1, 1) + r["oh"] * G1.view(1, -1, 1)
    wyn = torch.where(r["counts"] & (r["ce_weight"] != 0), r["wy"] / r["ce_den"], torch.zeros_like(r["wy"])).unsqueeze(1)
    p, oh = r["p"], r["oh"]
    if r["prob"]:
        dd, dot = g, None
        dn = -wyn / (r["x"] + r["eps"]) * oh if r["nll_log"] else -wyn * oh
        dn = torch.where(oh > 0, dn, torch.zeros_like(dn))
    else:
        dot = (p * g).sum(1, keepdim=True)
        dd = p * (g - dot)
        dn = wyn * (p - oh)
    grad = go * (r["dice_weight"] * dd + r["ce_weight"] * dn)
    return dict(grad=grad, G0=G0, G1=G1, g=g, dot=dot, dd=dd, dn=dn, wyn=wyn, go=go)


# ---------------------------------------------------------------------------------------- loss: measured math-library term
def measure_softmax(x, y_counts=None, yc=None):
    """(k_sm, k_nll) of the module docstring for logits x [N, C, HW] fp32"""
    x32 = x.float()
    x64 = x32.to(F64)
    m = x64.max(1, keepdim=True).values
    p64, p32 = torch.softmax(x64, 1), torch.softmax(x32, 1).to(F64)
    ok = p64 > 1e-30
    C = x.shape[1]
    k_sm = ((p32 - p64).abs() / (U24 * p64.clamp(min=1e-300) * (C + m - x64)))[ok].max().item()
    n64, n32 = -torch.log_softmax(x64, 1), (-torch.log_softmax(x32, 1)).to(F64)
    k_nll = ((n32 - n64).abs() / (U24 * (C + (m - x64) + n64))).max().item()
    return k_sm, k_nll


def measure_log(x, eps):
    x32 = x.float()
    e32 = torch.tensor(float(eps), dtype=torch.float32)
    l64, l32 = torch.log(x32.to(F64) + e32.to(F64)), torch.log(x32 + e32).to(F64)
    ok = torch.isfinite(l64)
    return ((l32 - l64).abs() / (U24 * (1 + l64.abs())))[ok].max().item()


# ---------------------------------------------------------------------------------------- loss: bounds
def _ep(r):
    """per element |error| of the device's p"""
    if r["prob"]:
        return torch.zeros_like(r["p"])
    return K_SM * U24 * r["p"] * (r["C"] + r["m"] - r["x"]) + TINY


def _enll(r):
    """per pixel |error| of w[y] * nll"""
    if r["prob"]:
        e = K_LOG * U24 * (1 + r["nll"].abs()) if r["nll_log"] else torch.zeros_like(r["nll"])
    else:
        e = K_NLL * U24 * (r["C"] + (r["m"].squeeze(1) - r["xy"]) + r["nll"])
    e = torch.where(r["counts"], e, torch.zeros_like(e))
    wn = torch.where(r["counts"], (r["wy"] * r["nll"]).abs(), torch.zeros_like(e))
    return r["wy"] * e + (U24 * wn if r["weighted"] else 0.0)


def state_bound(r):
    """|error| allowed per state entry [4 + 3 * 8] (NaN where the reference is NaN: compared by isnan), and the pieces."""
    P, C = r["P"], r["C"]
    ch = chain(P) * U24
    ep = _ep(r)
    e_I = ch * r["I"] + (ep * r["oh"]).sum((0, 2))
    e_Sp = ch * r["p"].abs().sum((0, 2)) + ep.sum((0, 2))
    e_Sg = torch.zeros(C, dtype=F64)                                    # counts: exact
    e_num = ch * r["ce_abs"] + _enll(r).sum()
    e_cden = ch * r["ce_den"] if r["weighted"] else torch.tensor(0.0, dtype=F64)
    e_den = e_I * 0 + e_Sp + e_Sg + 2 ** -52 * r["den_raw"].abs()
    e_dc = 1.01 * (2 * e_I + r["dc"].abs() * torch.where(r["clip"], torch.zeros_like(e_den), e_den)) / r["den"]
    e_dice = (r["a"] * e_dc).sum()
    if r["ce_den"] > 0:
        e_ce = 1.01 * (e_num + r["ce"].abs() * e_cden) / r["ce_den"]
    else:
        e_ce = torch.tensor(float("nan"), dtype=F64)
    e_loss = abs(r["dice_weight"]) * e_dice + (abs(r["ce_weight"]) * e_ce if r["ce_weight"] != 0 else 0.0)
    b = torch.zeros(4 + 3 * MAXC, dtype=F64)
    b[0], b[1], b[2], b[3] = e_loss, e_ce, e_dice, e_cden
    b[4:4 + C], b[4 + MAXC:4 + MAXC + C] = e_dc, e_den
    b = b + U24 * r["state"].abs()                                       # each entry: one rounding to fp32
    if not r["weighted"]:
        b[3] = 0.0                                                       # a pixel count below 2^24
    return b, dict(e_dc=b[4:4 + C], e_den=b[4 + MAXC:4 + MAXC + C], e_a=b[4 + 2 * MAXC:4 + 2 * MAXC + C], e_cden=b[3])


def grad_bound(r, gr):
    """per element |error| allowed for the gradient: the fp32 evaluation per element plus what the state entries carry in"""
    _, s = state_bound(r)
    u = U24
    a, dc, den_raw, clip = r["a"], r["dc"], r["den_raw"], r["clip"]
    safe = lambda v: torch.where(v.abs() > 0, v.abs(), torch.ones_like(v))
    rel_a = s["e_a"] / safe(a)
    rel_den = torch.where(clip, torch.zeros_like(den_raw), s["e_den"] / safe(den_raw))
    dG0 = torch.where(clip, torch.zeros_like(dc), (a * s["e_dc"] / safe(den_raw)) + gr["G0"].abs() * (rel_a + rel_den + 3 * u))
    dG1 = gr["G1"].abs() * (rel_a + rel_den + 3 * u)
    oh, p = r["oh"], r["p"]
    dg = dG0.view(1, -1, 1) + oh * dG1.view(1, -1, 1) + u * gr["g"].abs()
    rel_wyn = (s["e_cden"] / r["ce_den"] if r["ce_den"] > 0 else 0.0) + 2 * u
    wyn = gr["wyn"]
    if r["prob"]:
        ddd = dg
        ddn = gr["dn"].abs() * (rel_wyn + 3 * u)
    else:
        ep = _ep(r)
        g = gr["g"]
        ddot = (ep * g.abs() + p * dg).sum(1, keepdim=True) + (r["C"] + 1) * u * (p * g.abs()).sum(1, keepdim=True)
        ddd = ep * (g - gr["dot"]).abs() + p * (dg + ddot + u * (g.abs() + gr["dot"].abs())) + u * gr["dd"].abs()
        ddn = wyn * rel_wyn * (p - oh).abs() + wyn * (ep + u * (p - oh).abs()) + u * gr["dn"].abs()
    dwt, cwt, go = abs(r["dice_weight"]), abs(r["ce_weight"]), abs(gr["go"])
    return 1.01 * go * (dwt * ddd + cwt * ddn + 3 * u * (dwt * gr["dd"].abs() + cwt * gr["dn"].abs())) + TINY


def one_pixel_effect(r):
    """the largest |change of the loss| that removing ONE pixel from every sum causes (float64, from the reference alone):
    what a kernel that drops a pixel gets wrong at least once.  Softmax or probability mode."""
    p, oh = r["p"], r["oh"]
    a, den_raw = r["a"], r["den_raw"]
    # Dice: dc_k' = (2 (I - p oh) + s) / max(Sp - p + Sg - oh + s, 1e-8) per pixel and class
    I2 = r["I"].view(1, -1, 1) - p * oh
    d2 = (den_raw.view(1, -1, 1) - p - oh).clamp(min=1e-8)
    dice2 = -(a.view(1, -1, 1) * (2 * I2 + r["smooth"]) / d2).sum(1)
    d_dice = dice2 - r["dice"]
    if r["ce_den"] > 0:
        wn = torch.where(r["counts"], r["wy"] * r["nll"], torch.zeros_like(r["nll"]))
        den2 = r["ce_den"] - r["wy"]
        ce2 = torch.where(den2 > 0, (r["ce_num"] - wn) / den2.clamp(min=1e-300), torch.full_like(den2, float("nan")))
        d_ce = (ce2 - r["ce"]).nan_to_num(0.0)
    else:
        d_ce = torch.zeros_like(d_dice)
    return (r["dice_weight"] * d_dice + r["ce_weight"] * d_ce).abs().max().item()


# ---------------------------------------------------------------------------------------- prompt remix
def prompt_mix_reference(clip, mask):
    """clip [N, 4, HW], mask [N, HW] -> final [N, 4, HW] float64 and the softmax / sigmoid"""
    p = torch.softmax(clip.to(F64), 1)
    m = torch.sigmoid(mask.to(F64)).unsqueeze(1)
    final = torch.cat([1 - m, m * (p[:, 0:1] + p[:, 3:4]), m * p[:, 1:2], m * p[:, 2:3]], 1)
    return final, p, m


def prompt_mix_grad_reference(clip, mask, dout):
    """d / d mask logit [N, HW] float64 = (-d0 + d1 (p0 + p3) + d2 p1 + d3 p2) m (1 - m), and the sum of the absolute terms of
    the bracket"""
    _, p, m = prompt_mix_reference(clip, mask)
    d = dout.to(F64)
    terms = torch.stack([-d[:, 0], d[:, 1] * (p[:, 0] + p[:, 3]), d[:, 2] * p[:, 1], d[:, 3] * p[:, 2]], 0)
    mm = m.squeeze(1)
    return terms.sum(0) * mm * (1 - mm), terms.abs().sum(0)


def measure_mix(clip, mask):
    """k_mix of the module docstring: fp32 CPU torch against float64, in units of 2^-24 * (1 + |mask logit|)"""
    f64, _, _ = prompt_mix_reference(clip, mask)
    p = torch.softmax(clip.float(), 1)
    m = torch.sigmoid(mask.float()).unsqueeze(1)
    f32_ = torch.cat([1 - m, m * (p[:, 0:1] + p[:, 3:4]), m * p[:, 1:2], m * p[:, 2:3]], 1).to(F64)
    return ((f32_ - f64).abs() / (U24 * (1 + mask.to(F64).abs().unsqueeze(1)))).max().item()


def prompt_mix_bound(mask):
    """outputs are in [0, 1]: K_MIX * 2^-24 * (1 + |mask logit|), absolute (the argument of the exponential is rounded first,
    and 1 - m cancels for a saturated mask)"""
    return (K_MIX * U24 * (1 + mask.to(F64).abs())).unsqueeze(1) + TINY


def prompt_mix_grad_bound(mask, abs_terms):
    """absolute as well: the bracket is a four-term fp32 sum of products with softmax factors (K_MIX + 8 roundoffs on its
    absolute terms), and m (1 - m) <= 1/4 carries the absolute error of m twice"""
    return (3 * K_MIX + 8) * U24 * (1 + mask.to(F64).abs()) * abs_terms + TINY


# ---------------------------------------------------------------------------------------- head
def head_input(z, scale, shift, dtype):
    """the tensor the _bn forms re-form from the pre-activation: relu(z * scale + shift) rounded to dtype like segk_bn_relu_apply"""
    return apply_reference(z, scale, shift, dtype)


def head_fwd_reference(y, w, b, N, HW):
    """y [P, Cp] (already rounded to the compute dtype), w [ncls, C] fp32, b [ncls] -> logits [N, ncls, HW] float64 and the sum
    of the absolute terms of each chain"""
    C = w.shape[1]
    y64, w64, b64 = y[:, :C].to(F64), w.to(F64), b.to(F64)
    lg = y64 @ w64.t() + b64
    ab = y64.abs() @ w64.abs().t() + b64.abs()
    to = lambda t: t.view(N, HW, -1).permute(0, 2, 1).contiguous()
    return to(lg), to(ab)


def head_fwd_bound(abs_terms, C):
    return 1.01 * (C + 1) * U24 * abs_terms


def head_bwd_reference(dl, y, w, bn=None, z=None):
    """dl [N, ncls, HW] fp32, y [P, Cp] rounded to dtype, w [ncls, C].  bn = (scale, shift, mean, rstd) fp32 [Cp]: also the
    BatchNorm reductions sum g, sum g * xhat with g = dy where y > 0; xhat = (z - mean) * rstd when the pre-activation z is
    given, else recovered from y: (y - shift) / scale * rstd - mean * rstd (0 where scale is 0)."""
    N, ncls, HW = dl.shape
    P, Cp = y.shape
    C = w.shape[1]
    d = dl.to(F64).permute(0, 2, 1).reshape(P, ncls)
    y64, w64 = y.to(F64), torch.zeros(ncls, Cp, dtype=F64)
    w64[:, :C] = w.to(F64)
    r = dict(dy=d @ w64, dy_abs=d.abs() @ w64.abs(), dw=(d.t() @ y64)[:, :C], dw_abs=(d.abs().t() @ y64.abs())[:, :C], db=d.sum(0),
             db_abs=d.abs().sum(0))
    if bn is not None:
        sc, sh, mu, rs = (t.to(F64) for t in bn)
        if z is not None:
            xh = (z.to(F64) - mu) * rs
            xh_abs = z.to(F64).abs() * rs.abs() + (mu * rs).abs()
        else:
            xa = torch.where(sc != 0, rs / torch.where(sc != 0, sc, torch.ones_like(sc)), torch.zeros_like(sc))
            xh = y64 * xa - sh * xa - mu * rs
            xh_abs = (y64 * xa).abs() + (sh * xa).abs() + (mu * rs).abs()
        g = r["dy"] * (y64 > 0)
        e_o = 1.01 * ncls * U24 * r["dy_abs"] * (y64 > 0)            # the fp32 dy the kernel feeds into the sums
        r.update(sg=g.sum(0), sg_abs=g.abs().sum(0), sg_in=e_o.sum(0), sgx=(g * xh).sum(0), sgx_abs=(g * xh).abs().sum(0),
                 sgx_in=(e_o * xh.abs() + g.abs() * 4 * U24 * xh_abs).sum(0))
    return r


def head_dy_bound(r, ncls, dtype):
    e = 1.01 * ncls * U24 * r["dy_abs"]
    return e + half_ulp(r["dy"].abs() + e, dtype)


def head_sum_bound(P, Cp, abs_sum, carried=0.0):
    nb, n_t, rows = head_bwd_launch(P, Cp)
    return (n_t + rows + 4) * U24 * abs_sum + 1.01 * carried


# ---------------------------------------------------------------------------------------- shared inputs of the two test files
def loss_inputs(C, N, HW, seed, family="dense", prob=False):
    """-> x [N, C, HW] fp32, y [N, HW] int64.  dense: logits uniform in [-3, 3], labels uniform.  sparse (the large pixel counts):
    one pixel in 64 is such a foreground pixel, the others are background: label 0, logit of class 0 raised by 14 -- so the sums
    the loss is made of stay dominated by the ~P / 64 foreground pixels and one pixel more or less remains visible in an fp32
    sum over millions.  prob: the fp32 softmax of these logits is the input."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((N, C, HW), generator=g, dtype=torch.float32) * 6 - 3
    y = torch.randint(0, C, (N, HW), generator=g, dtype=torch.int64)
    if family == "sparse":
        bg = torch.rand((N, HW), generator=g) >= 1.0 / 64
        y[bg] = 0
        x[:, 0, :] += 14.0 * bg
    if prob:
        x = torch.softmax(x, 1) if C > 1 else torch.sigmoid(x)          # one class: any value in (0, 1)
    return x, y


# (N, HW, family): pixel counts chosen from the launch arithmetic (see tests/test_gpu_head_loss_matrix.py)
LOSS_SHAPES = [(1, 1, "dense"), (2, 240, "dense"), (64, 64, "dense"), (241, 17, "dense"), (400, 35, "dense"), (1000, 123, "dense"),
               (1024, 128, "dense"), (1311, 100, "dense"), (1044, 1000, "sparse"), (1045, 1000, "sparse")]
LOSS_SHAPES_LARGE = [(1000, 1050, "sparse"), (3001, 1000, "sparse")]          # C in LARGE_CLASSES only
LARGE_CLASSES = (2, 5, 8)
SMOOTHS = (0.0, 1e-5, 1.0)
MIXES = ((1.0, 0.0), (0.0, 1.0), (0.7, 1.3))
GOUTS = (1.0, 0.5)


def loss_case(C, si, prob, large=False):
    """inputs and options of one cell of the matrix: every option list is walked with a stride of its own, so that each class
    count meets each option of each list within the ten shapes.  -> (x, y, kwargs of loss_reference, gout, description)"""
    N, HW, family = (LOSS_SHAPES_LARGE if large else LOSS_SHAPES)[si]
    i = si + (10 if large else 0)
    x, y = loss_inputs(C, N, HW, 1000 * C + 17 * i + (500 if prob else 0), family, prob)
    wmode = (C + i) % 3                               # none / weights / one weight zero
    imode = (C + 2 * i + i // 4) % 4                  # none / inside / 255 / -100
    cw = None
    if wmode:
        cw = torch.linspace(0.3, 1.7, C, dtype=torch.float32)
        if wmode == 2 and C > 1:
            cw[(i + 1) % C] = 0.0
    dwt, cwt = MIXES[(C + i // 2) % 3]
    ign = None
    if imode == 1 and C > 1:
        ign = (C + i) % C
    elif imode == 2:                                  # CrossEntropy only: the Dice of the reference project cannot take such labels
        ign, dwt, cwt = 255, 0.0, 1.0
        y.view(-1)[3::47] = 255
    elif imode == 3:
        y.view(-1)[5::53] = -100
    nll_log = 1 if family == "sparse" else (C + i) % 2
    kw = dict(cw=cw, ignore_index=ign, smooth=SMOOTHS[(2 * C + i) % 3], dice_weight=dwt, ce_weight=cwt, prob=prob,
              nll_log=nll_log if prob else 1, eps=1e-9 if prob and nll_log else 0.0)
    gout = GOUTS[(C + i // 3) % 2]
    desc = (f"C={C} N={N} HW={HW} {family} {'prob' if prob else 'softmax'} weights={('none', 'some', 'one zero')[wmode]} "
            f"ignore={ign} labels={('in range', 'in range', 'some 255', 'some -100')[imode]} smooth={kw['smooth']} mix=({dwt}, {cwt}) "
            f"nll_log={kw['nll_log']} gout={gout} launch={loss_launch(N * HW)}")
    return x, y, kw, gout, desc


def edge_cases():
    """the semantic edges, one case each: (name, x, y, kwargs of loss_reference, gout)"""
    out = []
    x, y = loss_inputs(4, 2, 240, 71)
    y[y == 2] = 3
    out.append(("class 2 absent from the labels", x, y, dict(smooth=1e-5, dice_weight=0.7, ce_weight=1.3), 1.0))
    x, y = loss_inputs(3, 2, 240, 72, prob=True)
    x[:, 1, :] = 0.0
    y[y == 1] = 2
    out.append(("probability class 1 identically zero, smooth 0: clip branch", x, y,
                dict(smooth=0.0, prob=True, nll_log=1, eps=1e-9), 0.5))
    x, y = loss_inputs(3, 2, 240, 73)
    out.append(("every pixel ignored", x, torch.full_like(y, 255), dict(ignore_index=255, dice_weight=0.7, ce_weight=1.3), 1.0))
    x, y = loss_inputs(5, 241, 17, 74)
    out.append(("logits at +-80", torch.where(x > 0, 80.0, -80.0), y, dict(smooth=1.0, dice_weight=0.7, ce_weight=1.3), 1.0))
    x, y = loss_inputs(3, 64, 64, 75)
    out.append(("all logits equal", torch.full_like(x, 1.25), y, dict(cw=torch.tensor([0.5, 1.0, 2.0])), 0.5))
    x, y = loss_inputs(3, 2, 240, 76)
    out.append(("all class weights zero: the 1e-8 clamp of the weight sum", x, y, dict(cw=torch.zeros(3), dice_weight=1.0, ce_weight=0.0), 1.0))
    x, y = loss_inputs(3, 2, 240, 77)
    out.append(("Dice only, every pixel carries the ignored class", x, torch.zeros_like(y),
                dict(ignore_index=0, smooth=1e-5, dice_weight=1.0, ce_weight=0.0), 1.0))
    return out


def degenerate(r):
    """cases whose loss does not depend on any single pixel or whose gradient is identically zero: no floor can be asserted.
    One class under the softmax (p = 1 everywhere), a single pixel, a NaN loss (nothing counts for the CrossEntropy)."""
    return (r["C"] == 1 and not r["prob"]) or r["P"] == 1 or bool(torch.isnan(r["loss"]))


# (N, HW) of the prompt remix: one pixel, two blocks with one thread in the second, the grid stride beyond 4096 blocks
MIX_SHAPES = [(1, 1), (1, 257), (1021, 1029)]


def mix_cases():
    """CLIP logits in [-4, 4]; mask logits in [-6, 6] with every seventh at +-40 (a saturated sigmoid)"""
    out = []
    for i, (N, HW) in enumerate(MIX_SHAPES):
        g = torch.Generator().manual_seed(4000 + i)
        cl = torch.rand((N, 4, HW), generator=g) * 8 - 4
        ml = torch.rand((N, HW), generator=g) * 12 - 6
        ml.view(-1)[::7] = 40.0
        ml.view(-1)[3::14] = -40.0
        out.append((cl, ml))
    return out
