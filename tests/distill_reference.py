"""float64 reference, analytic gradient, launch arithmetic and derived error bounds for the kernels of csrc/distill.hip (the
multi-teacher soft-target loss), shared by tests/test_distill_host.py and tests/test_gpu_distill.py.  CPU torch
only.  Nothing here is taken from what the kernels return.

Semantics, on student logits s [N, C, H, W], V teacher tensors t_v [N, C, H, W] with (flip, kind, weight) each, optional labels
y [N, H, W], and the scalars as the fp32 values the kernel receives (invT = fp32(1 / T), Tsq = fp32(T T), min_conf):

  t_v at student pixel (y, x) is read at (flip & 2 ? H-1-y : y, flip & 1 ? W-1-x : x);  z_v = t_v, kind 1: log(max(t_v, 2^-126))
  q  = sum_v weight_v softmax(z_v invT);  q1 = the same with invT = 1 (q itself when invT == 1);  p = softmax(s invT)
  a pixel COUNTS when (y absent or y != ignore_index) and max_k q1_k >= min_conf
  KL = sum_k q_k (log q_k - log p_k) over q_k > 0;  n = counted pixels;  soft = Tsq sum KL / n, 0 when n == 0
  d soft / d s_k = gout Tsq invT / n (p_k - q_k) at counted pixels, 0 elsewhere (the derivative of the line above up to
                   (sum_v weight_v - 1) p_k: the table weights are rounded to fp32 one by one, so their sum is 1 within V 2^-25)
  n_agree = counted pixels with argmax p == argmax q (first maximum)
  state = [soft, n, sum KL, n_agree, 0 ...]

Error bounds follow the summation structure of distill_fwd_kernel, which is loss_fwd_kernel's: a thread adds n_t = ceil(P /
(blocks 1024)) pixel terms in fp32, the wave butterfly six more levels, one thread the sixteen wave rows, the finishing block
the block rows in float64, one rounding to fp32: loss_reference.chain(P) unit roundoffs on the sum of the absolute pixel terms.
The pixel counts are integer sums: exact.

Per pixel, the accuracy of the device's expf / logf cannot be derived from the project.  Where the evaluation is the one
loss_reference.py measured, its constants are used again: K_SM for a softmax (|dp| <= K_SM 2^-24 p (C + max - x)), K_LOG for the
logarithm of a probability-kind teacher (|dz| <= K_LOG 2^-24 (1 + |z|)).  A temperature adds the rounding of the product
a = x invT before the softmax: 2 2^-24 max |a| relative on every probability.  That gives the per-class bounds ep (student) and
eq (teacher mix: the weighted sum of the views' bounds plus V + 1 roundoffs of the multiply-add chain) which the gradient bound
and the argmax gaps use.

The KL term has one new constant.  Its error is carried in by q (times |log q - log p| + 1), by log p (as for K_NLL: C + (max -
a_k) + nll_k roundoffs, plus the temperature term), by logf(q) (|log q| roundoffs) and by the C-term sum; in units of 2^-24:

  unit = sum_{q_k > 0} [ eq'_k (|D_k| + 1) + q_k (C + (max a - a_k) + nll_k + 2 max|a| [T != 1] + |log q_k| + 2 |D_k|) ] + C sum |q_k D_k|

with D_k = log q_k - log p_k and eq'_k = eq_k / 2^-24 with every K set to 1.  k_kl = max over pixels of |KL32 - KL| / (2^-24
unit + 16 2^-126 sum (1 + |D_k|)) is MEASURED on the host as fp32 CPU torch (the same operations in the same order) against
float64 over the whole case matrix below -- C = 1..8, every shape, view count, flip, kind, temperature, the +-80, all-equal and
exact-zero cases: k_kl <= 0.337 (tests/test_distill_host.py measures again and asserts that no case exceeds a quarter of the
constant).  The device math library may differ from the host's by a few ulp, so the bound allows 4 x the measured value, rounded
up to two digits: K_KL = 1.4.

An argmax is decided when the gap between the float64 maximum and every other class exceeds the sum of the two per-class
bounds.  Classes whose inputs are bit-identical (the student's two logits; every teacher's two values) go through identical
arithmetic in the kernel, come out bit-identical and are decided by the first-maximum rule on both sides: they are not
uncertain, whatever the bound."""
import torch

from bn_reference import U24
from loss_reference import K_SM, K_LOG, TINY, F64, f32, chain, loss_launch

MAXC = 8
K_KL = 1.4


# ---------------------------------------------------------------------------------------- launch arithmetic
def distill_launch(P):
    """segk_distill_fwd: the blocks (= partial rows) of segk_loss_blocks, pixel terms per thread chain, wave rows per block"""
    return loss_launch(P)


def pixels_in_flight(C, forward=True):
    """fwd_pif / bwd_pif of distill.hip for the compiled class count that holds C"""
    nc = C if C <= 4 else 8
    return (4 if nc <= 4 else 2) if forward else (2 if nc <= 4 else 1)


# ---------------------------------------------------------------------------------------- reference
def unflip(t, flip):
    """the teacher tensor as the student's pixels see it"""
    dims = [d for d, bit in ((3, 1), (2, 2)) if flip & bit]
    return torch.flip(t, dims) if dims else t


def table_weights(weights):
    """w_v / sum w in float64, rounded once to fp32 (distill.teacher_table)"""
    w = torch.tensor([float(v) for v in weights], dtype=F64)
    return (w / w.sum()).float()


def _mix(s, teachers, flips, kinds, w32, invT, dt):
    """q, q1, p, log p and the per-view pieces in dtype dt, in the kernel's order of operations"""
    views = []
    q = torch.zeros(s.shape, dtype=dt)
    q1 = torch.zeros(s.shape, dtype=dt)
    it = torch.tensor(invT, dtype=dt)
    for t, fl, kd, w in zip(teachers, flips, kinds, w32):
        z = unflip(t, fl).to(dt)
        if kd:
            z = torch.log(torch.clamp(z, min=torch.tensor(TINY, dtype=dt)))
        a = z * it if invT != 1.0 else z
        pv, p1 = torch.softmax(a, 1), torch.softmax(z, 1)
        q = q + w.to(dt) * pv
        q1 = q1 + w.to(dt) * p1
        views.append(dict(z=z, a=a, pv=pv, w=w.to(dt), kind=kd))
    if invT == 1.0:
        q1 = q
    a = s.to(dt) * it if invT != 1.0 else s.to(dt)
    return q, q1, torch.softmax(a, 1), torch.log_softmax(a, 1), a, views


def _kl_pixels(q, logp):
    pos = q > 0
    D = torch.where(pos, torch.log(torch.where(pos, q, torch.ones_like(q))) - logp, torch.zeros_like(q))
    return (q * D).sum(1), D


def distill_reference(s, teachers, flips, kinds, weights, y=None, ignore_index=None, T=1.0, min_conf=0.0):
    """-> dict of float64 results (see the module docstring) and the per-pixel quantities the gradient and the bounds need"""
    N, C, H, W = s.shape
    invT, Tsq, mc = f32(1.0 / T), f32(T * T), f32(min_conf)
    w32 = table_weights(weights)
    q, q1, p, logp, a, views = _mix(s, teachers, flips, kinds, w32, invT, F64)
    labelled = torch.ones((N, H, W), dtype=torch.bool)
    if y is not None and ignore_index is not None:
        labelled = y.reshape(N, H, W) != int(ignore_index)
    conf = q1.max(1).values
    counted = labelled & (conf >= mc)
    kl, D = _kl_pixels(q, logp)
    n = int(counted.sum())
    sum_kl = kl[counted].sum() if n else torch.tensor(0.0, dtype=F64)
    soft = Tsq * sum_kl / n if n else torch.tensor(0.0, dtype=F64)
    ap, aq = p.argmax(1), q.argmax(1)
    state = torch.zeros(4 + 3 * MAXC, dtype=F64)
    state[0], state[1], state[2], state[3] = soft, n, sum_kl, int(((ap == aq) & counted).sum())
    return dict(N=N, C=C, H=H, W=W, P=N * H * W, V=len(teachers), s=s, teachers=teachers, flips=flips, kinds=kinds, w32=w32,
                invT=invT, Tsq=Tsq, min_conf=mc, q=q, q1=q1, p=p, logp=logp, a=a, views=views, labelled=labelled, conf=conf,
                counted=counted, kl=kl, D=D, n=n, sum_kl=sum_kl, soft=soft, ap=ap, aq=aq, agree=(ap == aq) & counted,
                state=state)


def distill_grad_reference(r, gout=1.0):
    """analytic d soft / d s [N, C, H, W] float64 times the fp32 upstream gradient"""
    go = f32(gout)
    if r["n"] == 0:
        return dict(grad=torch.zeros_like(r["p"]), coef=0.0, go=go)
    coef = go * r["Tsq"] * r["invT"] / r["n"]
    return dict(grad=coef * (r["p"] - r["q"]) * r["counted"].unsqueeze(1), coef=coef, go=go)


# ---------------------------------------------------------------------------------------- per-class bounds
def _temp_term(a, invT):
    """2 max |a| roundoffs relative: the product x invT is rounded before the softmax (absent at invT == 1)"""
    return 2 * a.abs().max(1, keepdim=True).values if invT != 1.0 else torch.zeros_like(a[:, :1])


def _ep(r, k_sm=K_SM):
    a = r["a"]
    return U24 * r["p"] * (k_sm * (r["C"] + a.max(1, keepdim=True).values - a) + _temp_term(a, r["invT"])) + TINY


def _eq(r, k_sm=K_SM, k_log=K_LOG, of="q"):
    """of = "q": the tempered mix; "q1": the untempered one the gate reads"""
    tempered = of == "q" and r["invT"] != 1.0
    e = torch.zeros_like(r["q"])
    for v in r["views"]:
        a = v["a"] if tempered else v["z"]
        pv = v["pv"] if tempered or r["invT"] == 1.0 else torch.softmax(v["z"], 1)
        rel = k_sm * (r["C"] + a.max(1, keepdim=True).values - a) + (_temp_term(a, r["invT"]) if tempered else 0.0)
        if v["kind"]:
            rel = rel + 2 * (r["invT"] if tempered else 1.0) * k_log * (1 + v["z"].abs()).max(1, keepdim=True).values
        e = e + v["w"] * pv * rel
    return U24 * (e + (r["V"] + 1) * (r["q"] if of == "q" else r["q1"])) + TINY


def kl_unit(r):
    """per pixel [N, H, W]: the error of the KL term in units of K_KL (see the module docstring), absolute slack included"""
    a, q, D, C = r["a"], r["q"], r["D"], r["C"]
    pos = q > 0
    eq1 = _eq(r, 1.0, 1.0) - TINY
    logq = torch.where(pos, torch.log(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))
    elp = U24 * (C + (a.max(1, keepdim=True).values - a) - r["logp"] + _temp_term(a, r["invT"]))
    per = eq1 * (D.abs() + 1) + q * (elp + U24 * (logq.abs() + 2 * D.abs()))
    per = torch.where(pos, per, torch.zeros_like(per))
    return per.sum(1) + C * U24 * (q * D).abs().sum(1) + 16 * TINY * (1 + D.abs()).sum(1)


def measure_kl(r):
    """k_kl of the module docstring: the pixel term in fp32 CPU torch, operation for operation, against float64"""
    s32 = r["s"].float()
    q, _, _, logp, _, _ = _mix(s32, [t.float() for t in r["teachers"]], r["flips"], r["kinds"], r["w32"], r["invT"], torch.float32)
    kl32, _ = _kl_pixels(q, logp)
    return ((kl32.to(F64) - r["kl"]).abs() / kl_unit(r)).max().item()


# ---------------------------------------------------------------------------------------- bounds
def state_bound(r):
    """|error| allowed for state[0] (soft) and state[2] (sum KL); n and n_agree are integers"""
    if r["n"] == 0:
        return 0.0, 0.0
    c = r["counted"]
    e_sum = chain(r["P"]) * U24 * r["kl"][c].abs().sum() + K_KL * kl_unit(r)[c].sum()
    e_soft = 1.01 * r["Tsq"] * e_sum / r["n"] + U24 * r["soft"].abs()
    return float(e_soft), float(e_sum + U24 * r["sum_kl"].abs())


def grad_bound(r, gr):
    """per element: the two probabilities' bounds, the subtraction, the three roundings of the coefficient and the product"""
    coef = abs(gr["coef"])
    e = coef * (_ep(r) + _eq(r) + U24 * (r["p"] - r["q"]).abs()) + 4 * U24 * gr["grad"].abs()
    return 1.01 * e * r["counted"].unsqueeze(1) + TINY * r["counted"].unsqueeze(1)


def _same_inputs(x, top):
    """[N, C, H, W] bool: class k of x holds the very bits class `top` holds"""
    return x == x.gather(1, top.unsqueeze(1))


def undecided(r):
    """[N, H, W] bool: pixels where the float64 argmax of p or of q is decided by a gap below the sum of the two classes' bounds
    (classes with bit-identical inputs excepted: see the module docstring).  n_agree is asserted on the others."""
    out = torch.zeros_like(r["counted"])
    tied_q = None
    for t, fl in zip(r["teachers"], r["flips"]):
        same = _same_inputs(unflip(t, fl), r["aq"])
        tied_q = same if tied_q is None else tied_q & same
    for val, err, top, tied in ((r["p"], _ep(r), r["ap"], _same_inputs(r["s"], r["ap"])), (r["q"], _eq(r), r["aq"], tied_q)):
        gap = val.gather(1, top.unsqueeze(1)) - val
        close = (gap < err.gather(1, top.unsqueeze(1)) + err) & ~tied
        out |= close.any(1)
    return out


def gate_undecided(r):
    """[N, H, W] bool: labelled pixels whose confidence lies within its bound of min_conf (n would not be exact there); the
    case matrix is chosen so that there are none, which tests/test_distill_host.py asserts"""
    e = _eq(r, of="q1").gather(1, r["q1"].argmax(1, keepdim=True)).squeeze(1)
    return r["labelled"] & ((r["conf"] - r["min_conf"]).abs() <= e)


# ---------------------------------------------------------------------------------------- shared inputs of the two test files
# (N, H, W): 1, 3, 255, 257, 1023 and 4097 pixels (one thread, less than a wave, around one and four rows of 256, one pixel past
# the first block of 4 x 1024), then two images of 5 x 7 and of 4099 pixels (the batch boundary, both flip axes at odd sizes)
SHAPES = [(1, 1, 1), (1, 1, 3), (1, 15, 17), (1, 257, 1), (1, 31, 33), (1, 17, 241), (2, 5, 7), (2, 1, 4099)]
TEMPS = (0.5, 1.0, 2.0)
GOUTS = (1.0, 0.5)


def inputs(C, N, H, W, V, kinds, seed):
    """student logits uniform in [-3, 3]; a teacher is half the student plus uniform [-4, 4] noise (so that the argmaxes agree at
    some pixels and differ at others), given as logits or as the fp32 softmax of them"""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand((N, C, H, W), generator=g, dtype=torch.float32) * 6 - 3
    ts = []
    for kd in kinds:
        t = 0.5 * s + torch.rand((N, C, H, W), generator=g, dtype=torch.float32) * 8 - 4
        ts.append(torch.softmax(t, 1) if kd else t)
    y = torch.randint(0, C, (N, H, W), generator=g, dtype=torch.int64)
    return s, ts, y


def case(C, si):
    """one cell of the matrix: every option list is walked with a stride of its own, so that each class count meets every flip,
    both kinds, every view count, temperature, label mode and gate within the eight shapes.
    -> (s, teachers, kwargs of distill_reference, gout, description)"""
    N, H, W = SHAPES[si]
    V = 1 + (C + si) % 3
    flips = [(C + 2 * si + 3 * v) % 4 for v in range(V)]
    kinds = [(C + si + v) % 2 for v in range(V)]
    weights = [1.0 + 0.75 * v + 0.5 * (si % 2) for v in range(V)]
    T = TEMPS[(C + si // 2) % 3]
    lmode = (C + 2 * si + si // 4) % 3                  # none / some labels 255 / one class ignored
    s, ts, y = inputs(C, N, H, W, V, kinds, 7000 + 100 * C + si)
    ign, labels = None, None
    if lmode == 1:
        labels, ign = y.clone(), 255
        labels.view(-1)[1::3] = 255
    elif lmode == 2:
        labels, ign = y, (C + si) % C
    gate = (C + si) % 4 == 0
    # between the least and the greatest possible confidence; one class: the confidence is the weight sum, 1 within V 2^-25
    min_conf = (0.5 * (1.0 / C + 1.0) if C > 1 else 0.5) if gate else 0.0
    gout = GOUTS[(C + si // 3) % 2]
    kw = dict(flips=flips, kinds=kinds, weights=weights, y=labels, ignore_index=ign, T=T, min_conf=min_conf)
    desc = (f"C={C} N={N} H={H} W={W} V={V} flips={flips} kinds={kinds} weights={weights} T={T} "
            f"labels={('none', 'some 255', 'class ignored')[lmode]} ignore={ign} min_conf={min_conf:.4f} gout={gout} "
            f"launch={distill_launch(N * H * W)}")
    return s, ts, kw, gout, desc


def edge_cases():
    """the semantic edges, one case each: (name, s, teachers, kwargs of distill_reference, gout)"""
    out = []
    s, ts, y = inputs(3, 2, 5, 7, 2, [0, 1], 7901)
    out.append(("every label ignored", s, ts, dict(flips=[1, 2], kinds=[0, 1], weights=[1, 2], y=torch.full_like(y, 255),
                                                    ignore_index=255, T=2.0), 1.0))
    s, ts, y = inputs(4, 1, 15, 17, 2, [0, 0], 7902)
    out.append(("a gate nothing passes", s, ts, dict(flips=[0, 3], kinds=[0, 0], weights=[1, 1], min_conf=1.5), 1.0))
    s, ts, y = inputs(5, 1, 31, 33, 2, [0, 0], 7903)
    pm = lambda t: torch.where(t > 0, 80.0, -80.0)   # (weight ratios no ratio of class counts equals: q has no exact ties
    #                                                   between classes that differ in a teacher)
    out.append(("logits at +-80, T = 0.5", pm(s), [pm(t) for t in ts], dict(flips=[0, 1], kinds=[0, 0], weights=[1, 2.7], T=0.5), 1.0))
    out.append(("logits at +-80, T = 1", pm(s), [pm(t) for t in ts], dict(flips=[2, 0], kinds=[0, 0], weights=[2.3, 1]), 0.5))
    s, ts, y = inputs(3, 1, 15, 17, 2, [0, 1], 7904)
    out.append(("all logits equal", torch.full_like(s, 1.25), [torch.full_like(s, -0.5), torch.full_like(s, 1.0 / 3)],
                dict(flips=[0, 3], kinds=[0, 1], weights=[1, 2], T=2.0), 1.0))
    s, ts, y = inputs(4, 2, 5, 7, 1, [0], 7905)
    hot = torch.nn.functional.one_hot(y, 4).permute(0, 3, 1, 2).float()
    out.append(("one probability teacher with exact zeros", s, [hot], dict(flips=[0], kinds=[1], weights=[1]), 1.0))
    out.append(("exact zeros beside a logit teacher, T = 2", s, [hot, ts[0]], dict(flips=[3, 1], kinds=[1, 0], weights=[1, 1], T=2.0,
                                                                                 y=y, ignore_index=1), 0.5))
    s, ts, y = inputs(8, 1, 17, 241, 3, [0, 1, 0], 7906)
    out.append(("a gate some pixels pass, three views", s, ts, dict(flips=[1, 2, 3], kinds=[0, 1, 0], weights=[3, 1, 2], T=0.5,
                                                                    min_conf=0.6), 1.0))
    return out


def all_cases():
    """(description, s, teachers, kwargs, gout) of the whole matrix"""
    for C in range(1, MAXC + 1):
        for si in range(len(SHAPES)):
            s, ts, kw, gout, desc = case(C, si)
            yield desc, s, ts, kw, gout
    for name, s, ts, kw, gout in edge_cases():
        yield name, s, ts, kw, gout


def run_reference(s, ts, kw):
    kw = dict(kw)
    return distill_reference(s, ts, kw.pop("flips"), kw.pop("kinds"), kw.pop("weights"), **kw)


if __name__ == "__main__":       # prints the measured constant the docstring quotes
    worst = 0.0
    for desc, s, ts, kw, gout in all_cases():
        k = measure_kl(run_reference(s, ts, kw))
        worst = max(worst, k)
        print(f"{k:8.4f}  {desc}")
    print("k_kl =", worst)
