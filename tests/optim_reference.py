"""NumPy restatement of DESIGN.md section 3.13 (seg.AdamW: global-norm clipping + AdamW + weight EMA), and a plain float64
AdamW + clip + EMA as yardstick.  Test infrastructure only.

The float32 restatement performs every operation of 3.13 on np.float32 values, so each rounds once (NumPy's float32 +, -, *, /
and sqrt are correctly rounded and nothing is contracted); the per-group scalars are formed in float64 and rounded once; the
bias corrections come from running float64 products, one multiplication per applied step, rounded to float32 once.

The norm.  Every gradient is float32, so its square is exact in float64 (24 x 24 = 48 bits) and the sum of squares is a
float64 sum of N exactly representable non-negative terms.  Any summation order of N non-negative terms has a relative error
of at most (N - 1) u / (1 - (N - 1) u), u = 2^-53 (Higham, Accuracy and Stability, section 4.2), so two orders -- the
device's fixed tree and NumPy's pairwise sum -- differ by at most about 2 (N - 1) u = (N - 1) 2^-52 relative in the sum of
squares.  The square root halves a relative error and adds its own rounding (u, twice): the norms differ by at most
(N - 1) 2^-53 + 2^-52 <= N 2^-52 relative.  NORM_REL(N) = N 2^-52 is the bound the tests hold."""
import numpy as np

CHUNK = 4096
F = np.float32


def norm_rel(numel_total):
    return numel_total * 2.0 ** -52


def norm_f64(grads):
    """sqrt of NumPy's float64 sum of squares over all gradients."""
    return float(np.sqrt(sum(np.sum(np.asarray(g, np.float64).ravel() ** 2) for g in grads)))


def clip_coef(norm, max_norm):
    """c = min(1, max_norm / (norm + 1e-6)) in float64, rounded once to float32; 1 without a max_norm."""
    if max_norm is None:
        return F(1.0)
    q = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return F(q) if (q < 1.0 or q != q) else F(1.0)


def group_scalars(lr, betas, eps, weight_decay, ema_decay=None):
    """The per-group float32 scalars, each formed in float64 and rounded once."""
    lr, b1, b2 = float(lr), float(betas[0]), float(betas[1])
    d = 0.0 if ema_decay is None else float(ema_decay)
    return {"lr": F(lr), "decay": F(1.0 - lr * float(weight_decay)), "omb1": F(1.0 - b1), "b2": F(b2), "omb2": F(1.0 - b2),
            "eps": F(float(eps)), "omd": F(1.0 - d), "ema_decay": F(d), "beta1": b1, "beta2": b2}


class StepState:
    """The device step state: t applied steps and the running products beta1^t, beta2^t of every group (float64)."""

    def __init__(self, ngroups, t=0, pows=None):
        self.t = t
        self.pows = [list(p) for p in pows] if pows is not None else [[1.0, 1.0] for _ in range(ngroups)]

    def advance(self, betas):
        self.t += 1
        for pw, (b1, b2) in zip(self.pows, betas):
            pw[0] = float(np.float64(pw[0]) * np.float64(b1))
            pw[1] = float(np.float64(pw[1]) * np.float64(b2))


def adamw_f32(p, g, m, v, s, k, c, pw, t, warmup=False):
    """One step of one tensor, in place on float32 arrays p, m, v (and the shadow s, or None).  k: group_scalars(); c: the clip
    coefficient (float32); pw: the group's running products AFTER this step's advance; t: the step count after the advance."""
    assert all(a.dtype == np.float32 for a in (p, g, m, v)) and (s is None or s.dtype == np.float32)
    bc1, bc2 = F(1.0 - pw[0]), F(1.0 - pw[1])
    step, bc2s = k["lr"] / bc1, np.sqrt(bc2)
    omd = k["omd"]
    if warmup:
        tf = F(t)
        omd = F(1.0) - min(k["ema_decay"], (F(1.0) + tf) / (F(10.0) + tf))
    with np.errstate(all="ignore"):
        gc = g * F(c)
        pd = p * k["decay"]
        mn = m + (gc - m) * k["omb1"]
        vn = v * k["b2"] + (gc * gc) * k["omb2"]
        den = np.sqrt(vn) / bc2s + k["eps"]
        pn = pd - (mn / den) * step
        assert pn.dtype == np.float32 and den.dtype == np.float32
        if s is not None:
            s[...] = s + (pn - s) * omd
        p[...] = pn
        m[...] = mn
        v[...] = vn


def adamw_f64(p, g, m, v, s, lr, betas, eps, weight_decay, t, c=1.0, ema_decay=None):
    """The yardstick: textbook AdamW in float64 (power-form bias corrections), in place."""
    b1, b2 = betas
    g = g * c
    p *= 1.0 - lr * weight_decay
    m += (g - m) * (1.0 - b1)
    v[...] = v * b2 + g * g * (1.0 - b2)
    den = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
    p -= lr / (1.0 - b1 ** t) * (m / den)
    if s is not None:
        s += (p - s) * (1.0 - ema_decay)


def run_f32(params, grads_per_step, group_of, groups, max_grad_norm=None, ema_decay=None, warmup=False, norms=None,
            state=None, ms=None, vs=None, shadows=None):
    """Run the restatement over len(grads_per_step) steps, in place on `params` (float32 arrays; a None gradient leaves the
    tensor out).  groups: list of dicts lr, betas, eps, weight_decay -- or a callable step index -> that list (a scheduler).
    norms: the norm to clip by at every step (the device's own), NumPy's float64 norm when None.  Returns (ms, vs, shadows,
    state)."""
    n = len(params)
    ms = ms if ms is not None else [None] * n
    vs = vs if vs is not None else [None] * n
    shadows = shadows if shadows is not None else [None] * n
    for i, step_grads in enumerate(grads_per_step):
        cfg = groups(i) if callable(groups) else groups
        state = state or StepState(len(cfg))
        live = [j for j in range(n) if step_grads[j] is not None]
        norm = norms[i] if norms is not None else norm_f64([step_grads[j] for j in live])
        c = clip_coef(norm, max_grad_norm)
        state.advance([g["betas"] for g in cfg])
        for j in live:
            if ms[j] is None:
                ms[j], vs[j] = np.zeros_like(params[j]), np.zeros_like(params[j])
            if ema_decay is not None and shadows[j] is None:
                shadows[j] = params[j].copy()
            gr = cfg[group_of[j]]
            k = group_scalars(gr["lr"], gr["betas"], gr["eps"], gr["weight_decay"], ema_decay)
            adamw_f32(params[j], step_grads[j], ms[j], vs[j], shadows[j], k, c, state.pows[group_of[j]], state.t, warmup)
    return ms, vs, shadows, state
