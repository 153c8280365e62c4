"""GPU: segk_hard_loss_fwd / segk_hard_loss_bwd (csrc/hard_loss.hip) and the modules on top of them against the float64 reference
of tests/hard_loss_reference.py.

1. every case of the table: state[0], S and D within their bounds, n exact, dlogits within its bound per element and exactly 0
   off the kept set;
2. the selection through the device's own words: state[5] and n_kept equal an exact NumPy selection over those words bit for bit
   (the million-pixel shape included), the words lie within their bound of the float64 keys, the float64 loss over the device's
   kept set is within bound, and where the table promises an empty `undecided` set the kept set is the reference's;
3. bit relations: everything off is segk_loss_fwd / segk_loss_bwd; thresh = 1, k >= n and min_fraction = 1 are selection off;
   two runs and a run on a side stream give equal bits;
4. the modules in train_loop and on captured logits.

Outputs are NaN / pattern filled before each call and carry guard elements.  Tolerances: derived or measured in
tests/hard_loss_reference.py, none tuned to what the kernels return.

The gradient of segk_loss_bwd at a pixel that does not count is go * (0 * dice term + 0 * (p - onehot)): a zero whose SIGN is the
Dice term's.  segk_hard_loss_bwd writes +0 there; the bit comparison covers every counted pixel, and cases without an uncounted
pixel are compared whole."""
import math

import numpy as np
import pytest
import torch

import hard_loss_reference as hr

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    return _lib


def _args(kw):
    """kwargs of hard_reference -> (class weights, ignore index, eps, gamma, select, theta, min_kept, q16) of the C entry"""
    thresh, mk, mf = kw.get("thresh"), kw.get("min_kept", 0), kw.get("min_fraction", 0.0)
    sel = not (thresh is None and mk == 0 and mf == 0.0)
    theta = hr.theta_of(thresh)
    ign = kw.get("ignore_index")
    return kw.get("cw"), -1 if ign is None else int(ign), float(kw.get("eps", 0.0)), float(kw.get("gamma", 0.0)), int(sel), \
        (theta if sel else 0.0), int(mk), hr.q16_of(mf)


def run_hard(lib, z, y, kw, gout=1.0):
    """-> dict(state [28] float32, words uint32 [28] of it, loss_out, keys [P] uint32 or None, grad [N, C, H, W]) on the CPU"""
    from image_segmentation_amd import ops
    N, C, H, W = z.shape
    P = N * H * W
    cw, ign, eps, gamma, sel, theta, mk, q16 = _args(kw)
    zd, yd = torch.from_numpy(z).cuda().contiguous(), torch.from_numpy(y).cuda().contiguous()
    cwd = None if cw is None else torch.from_numpy(np.asarray(cw, dtype=np.float32)).cuda()
    part = torch.full((lib.query("segk_loss_part_floats", P),), float("nan"), device="cuda")
    state = torch.full((lib.query("segk_loss_state_floats"),), float("nan"), device="cuda")
    out = torch.full((1,), float("nan"), device="cuda")
    keys = torch.full((P + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if sel else None
    hist = torch.full((hr.HIST_WORDS + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if sel else None
    go = torch.tensor([gout], dtype=torch.float32, device="cuda")
    dl = torch.full((z.size + GUARD,), float("nan"), device="cuda")
    p = lambda t: 0 if t is None else t.data_ptr()
    lib.call("segk_hard_loss_fwd", zd.data_ptr(), yd.data_ptr(), p(cwd), N, C, H * W, ign, eps, gamma, sel, theta, mk, q16, p(keys),
             p(hist), part.data_ptr(), state.data_ptr(), out.data_ptr(), ops._stream())
    lib.call("segk_hard_loss_bwd", zd.data_ptr(), yd.data_ptr(), p(cwd), p(keys), state.data_ptr(), go.data_ptr(), N, C, H * W, ign,
             eps, gamma, sel, dl.data_ptr(), ops._stream())
    torch.cuda.current_stream().synchronize()
    assert bool(torch.isnan(dl[z.size:]).all()), "the gradient buffer's guard was written"
    if sel:
        assert bool((keys[P:] == 0x5A5A5A5A).all()) and bool((hist[hr.HIST_WORDS:] == 0x5A5A5A5A).all()), "a guard was written"
    st = state.cpu().numpy()
    return dict(state=st, bits=st.view(np.uint32), loss_out=out.cpu().numpy(), grad=dl[:z.size].cpu().numpy().reshape(z.shape),
                keys=None if keys is None else keys[:P].cpu().numpy().view(np.uint32))


def _close(dev, ref, bound):
    """|dev - ref| <= bound where ref is finite; the same infinity, or NaN for NaN, where it is not"""
    dev, ref, bound = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        ok = np.where(fin, ~(np.abs(dev - ref) > bound), np.where(np.isnan(ref), np.isnan(dev), dev == ref))
    return bool(np.all(ok))


def check(lib, c):
    """sections 1 and 2 of the module docstring for one case"""
    z, y, kw, gout, r = c["z"], c["y"], c["kw"], c["gout"], c["ref"]
    d = run_hard(lib, z, y, kw, gout)
    st, bits = d["state"], d["bits"]
    assert int(bits[6]) == r["n"], c["desc"]
    assert d["loss_out"].view(np.uint32)[0] == bits[0] and st[2] == 0 and not st[8:].any()
    kept = r["kept"]
    if r["selecting"]:
        words = d["keys"]
        tw, n, nk = hr.select_words(words, r["theta"], r["min_kept"], r["q16"], select=hr.exact_select)
        assert (int(bits[5]), int(bits[6]), int(bits[7])) == (tw, n, nk), c["desc"]
        tau_dev = hr.word_value(tw)
        assert (math.isnan(tau_dev) and math.isnan(st[4])) or float(st[4]) == tau_dev
        assert ((words != 0) == r["counted"]).all()
        fin = r["counted"] & np.isfinite(r["kappa"])
        kd = (words[fin] - 1).view(np.float32).astype(np.float64)
        assert (np.abs(kd - r["kappa"][fin]) <= hr.key_bound(r)[fin]).all(), c["desc"]
        odd = r["counted"] & ~np.isfinite(r["kappa"])
        assert (words[odd] == np.where(np.isnan(r["kappa"][odd]), hr.NAN_WORD, 0x7F800001)).all()
        kept = words >= tw
        if c["set_check"]:
            assert (kept == r["kept"]).all(), c["desc"]
    else:
        assert float(st[4]) == 0.0 and int(bits[5]) == 1 and int(bits[7]) == r["n"]
    assert int(bits[7]) == int(kept.sum())
    # the float64 sums over the kept set the device used
    l64, w64 = r["l"].astype(np.float64), r["wt"].astype(np.float64)
    with np.errstate(all="ignore"):
        S, D = float(l64[kept].sum()), float(w64[kept].sum())
        loss = S / D if D > 0 else (math.nan if r["n"] == 0 else 0.0)
    e_loss, e_S, e_D = hr.state_bound(r, kept)
    print(f"{c['desc']}: loss {st[0]:.9g} ref {loss:.9g} bound {e_loss:.3g}  S {st[1]:.9g} ref {S:.9g}  D {st[3]:.9g} ref {D:.9g} "
          f"n {r['n']} kept {int(kept.sum())}")
    assert _close(st[0], loss, e_loss) and _close(st[1], S, e_S) and _close(st[3], D, e_D), c["desc"]
    if not D > 0:
        assert not d["grad"].view(np.uint32).any(), "exact zeros everywhere when no weight is kept"
        assert st[0] == 0.0 if r["n"] else math.isnan(st[0])
        return d
    with np.errstate(all="ignore"):
        g = hr.f32(gout) * r["g"].astype(np.float64) / D
    g = hr.unrows(np.where(kept[:, None], g, 0.0), r["shape"])
    assert _close(d["grad"], g, hr.grad_bound(r, gout, kept)), c["desc"]
    off = ~hr.unrows(np.repeat(kept[:, None], r["C"], 1), r["shape"])
    assert not d["grad"].view(np.uint32)[off].any(), "exactly 0 off the kept set"
    return d


@pytest.mark.parametrize("ci,ri", hr.table())
def test_table_against_float64(lib, ci, ri):
    check(lib, hr.case(ci, ri))


@pytest.mark.parametrize("regime", hr.BIG_REGIMES)
def test_million_pixels(lib, regime):
    d = check(lib, hr.big_case(regime))
    assert int(d["bits"][6]) > 900000


@pytest.mark.parametrize("i", range(6))
def test_word_cases(lib, i):
    name, z, y, kw = hr.word_cases()[i]
    d = check(lib, dict(z=z, y=y, kw=kw, gout=1.0, desc=name, ref=hr.hard_reference(z, y, **kw), set_check=False))
    if name == "all words equal":
        assert int(d["bits"][7]) == 255 and len(set(d["keys"].tolist())) == 1
    if name == "words differing in the low 10 bits":
        assert len(set((d["keys"] >> 10).tolist())) == 1 and int(d["bits"][7]) >= 77
    if name == "one key of exactly 0":
        assert 1 in d["keys"].tolist() and int(d["bits"][7]) == 70
    if name == "one +inf key":
        assert int(d["bits"][5]) < 0x7F800001 and math.isinf(d["state"][0])
    if name == "one NaN pixel":
        assert hr.NAN_WORD in d["keys"].tolist() and math.isnan(d["state"][0])


# ------------------------------------------------------------------------------------------------ bit relations
def _plain_inputs(ci, clean):
    """logits and labels at 255 to 8198 pixels; not clean: every fifth label 255 (ignored) and two labels outside [0, C)"""
    C = hr.CLASSES[ci]
    N, H, W = hr.SHAPES[2 + ci % 4]
    z, y = hr.inputs(C, N, H, W, 9950 + ci)
    if not clean:
        y.reshape(-1)[1::5] = 255
        y.reshape(-1)[3] = C
        y.reshape(-1)[7] = -3
    cw = (0.5 + 0.25 * np.arange(C)).astype(np.float32) if ci % 2 else None
    return z, y, dict(cw=cw, ignore_index=None if clean else 255)


@pytest.mark.parametrize("clean", (False, True))
@pytest.mark.parametrize("ci", range(len(hr.CLASSES)))
def test_everything_off_is_the_fused_cross_entropy(lib, ci, clean):
    from image_segmentation_amd import ops
    z, y, kw = _plain_inputs(ci, clean)
    N, C, H, W = z.shape
    P = N * H * W
    d = run_hard(lib, z, y, kw, 0.5)
    zd, yd = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    cwd = None if kw["cw"] is None else torch.from_numpy(kw["cw"]).cuda()
    ign = -1 if kw["ignore_index"] is None else kw["ignore_index"]
    part = torch.empty(lib.query("segk_loss_part_floats", P), device="cuda")
    state = torch.full((lib.query("segk_loss_state_floats"),), float("nan"), device="cuda")
    go = torch.tensor([0.5], device="cuda")
    dl = torch.full_like(zd, float("nan"))
    p = lambda t: 0 if t is None else t.data_ptr()
    lib.call("segk_loss_fwd", zd.data_ptr(), yd.data_ptr(), p(cwd), N, C, H * W, ign, 1e-5, 0.0, 1.0, part.data_ptr(),
             state.data_ptr(), 0, ops._stream())
    lib.call("segk_loss_bwd", zd.data_ptr(), yd.data_ptr(), p(cwd), state.data_ptr(), go.data_ptr(), N, C, H * W, ign, 0.0, 1.0,
             dl.data_ptr(), ops._stream())
    ref_state, ref_grad = state.cpu().numpy().view(np.uint32), dl.cpu().numpy()
    assert d["bits"][0] == ref_state[0] and d["bits"][3] == ref_state[3]
    r = hr.hard_reference(z, y, **kw)
    counted = hr.unrows(np.repeat(r["counted"][:, None], C, 1), z.shape)
    assert r["n"] > 0 and (clean == bool(r["counted"].all()))
    assert (d["grad"].view(np.uint32)[counted] == ref_grad.view(np.uint32)[counted]).all()
    assert not d["grad"].view(np.uint32)[~counted].any() and not ref_grad[~counted].any()


@pytest.mark.parametrize("ci,gamma,eps", [(0, 0.0, 0.0), (1, 2.0, 0.1), (2, 3.5, 0.0), (3, 0.0, 0.1), (4, 1.0, 0.1)])
def test_selections_that_keep_everything_are_selection_off(lib, ci, gamma, eps):
    z, y, kw = _plain_inputs(ci, False)
    c = dict(z=z, y=y)
    base = dict(kw, gamma=gamma, eps=eps)
    n = hr.hard_reference(c["z"], c["y"], **base)["n"]
    off = run_hard(lib, c["z"], c["y"], base, 0.5)
    assert 0 < n < y.size
    for extra in (dict(thresh=1.0), dict(min_kept=n), dict(min_kept=n + 1000), dict(min_fraction=1.0)):
        d = run_hard(lib, c["z"], c["y"], dict(base, **extra), 0.5)
        for i in (0, 1, 3, 6, 7):
            assert d["bits"][i] == off["bits"][i], (extra, i)
        assert (d["grad"].view(np.uint32) == off["grad"].view(np.uint32)).all(), extra


@pytest.mark.parametrize("ci,ri", [(1, 4), (4, 6), (0, 1)])
def test_two_runs_and_a_side_stream_give_equal_bits(lib, ci, ri):
    c = hr.case(ci, ri)
    a = run_hard(lib, c["z"], c["y"], c["kw"], c["gout"])
    b = run_hard(lib, c["z"], c["y"], c["kw"], c["gout"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run_hard(lib, c["z"], c["y"], c["kw"], c["gout"])
    torch.cuda.current_stream().wait_stream(side)
    for other in (b, s):
        assert (other["bits"] == a["bits"]).all() and (other["grad"].view(np.uint32) == a["grad"].view(np.uint32)).all()
        assert (other["keys"] == a["keys"]).all()


# ------------------------------------------------------------------------------------------------ modules and loops
def _model(seed=11):
    import image_segmentation_amd as seg
    torch.manual_seed(seed)
    return seg.unet(3, 3).cuda()


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((2, 3, 32, 32), generator=g), torch.randint(0, 3, (2, 1, 32, 32), generator=g)


def test_hard_pixel_loss_with_everything_off_trains_like_cross_entropy(lib, monkeypatch):
    import image_segmentation_amd as seg
    from image_segmentation_amd import training
    monkeypatch.setattr(training, "VERBOSE", False)
    batches = [_batch(1), _batch(2)]
    out = []
    for loss_fn in (seg.CrossEntropyLoss(), seg.HardPixelLoss()):
        m = _model()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        out.append((training.train_loop(batches, m, loss_fn, opt, 1, "cuda"), m.state_dict()))
    assert out[0][0] == out[1][0]
    for k, v in out[0][1].items():
        assert torch.equal(v, out[1][1][k]), k


@pytest.mark.parametrize("which", ("focal", "ohem"))
def test_focal_and_ohem_reduce_their_own_loss(lib, which):
    import image_segmentation_amd as seg
    loss_fn = seg.FocalLoss() if which == "focal" else seg.OhemCrossEntropyLoss(thresh=0.7, min_fraction=0.25)
    m = _model()
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    X, y = _batch(3)
    X, y = X.cuda(), y.cuda()
    vals = []
    for _ in range(6):
        opt.zero_grad()
        loss = loss_fn(m(X), y)
        loss.backward()
        opt.step()
        vals.append(loss.item())
    last = loss_fn.last
    assert all(last[k].is_cuda for k in ("n", "n_kept", "threshold"))
    n, nk = int(last["n"].item()), int(last["n_kept"].item())
    print(which, vals, n, nk, last["threshold"].item())
    assert n == 2 * 32 * 32 and (nk == n if which == "focal" else n // 4 <= nk <= n)
    assert all(np.isfinite(vals)) and vals[-1] < vals[0]


def test_dice_ce_with_label_smoothing_matches_float64_on_captured_logits(lib):
    import image_segmentation_amd as seg
    import loss_reference as L
    m = _model()
    X, y = _batch(5)
    y = y.clone()
    y.view(-1)[::7] = 2
    X, y = X.cuda(), y.cuda()
    cw = torch.tensor([0.5, 1.0, 2.0])
    pred = m(X)
    pred.retain_grad()
    loss_fn = seg.WeightedDiceCELoss(dice_weight=0.7, ce_weight=1.3, ignore_index=2, class_weights=cw.cuda(),
                                     ce_kwargs={"label_smoothing": 0.1})
    loss = loss_fn(pred, y)
    (loss * 0.5).backward()
    z = pred.detach().float().cpu()
    yc = y.cpu()[:, 0]
    # Dice alone from the loss reference, the smoothed CrossEntropy from this one, summed as the module sums them
    rd = L.loss_reference(z.reshape(2, 3, -1), yc.reshape(2, -1), cw=cw, ignore_index=2, smooth=1e-5, dice_weight=1.0, ce_weight=0.0)
    gd = L.loss_grad_reference(rd, 0.5 * 0.7)
    rc = hr.hard_reference(z.numpy(), yc.numpy(), cw=cw.numpy(), ignore_index=2, eps=0.1)
    gc = hr.hard_grad_reference(rc, 0.5 * 1.3)
    exp = 0.7 * float(rd["loss"]) + 1.3 * rc["loss"]
    bound = 0.7 * float(L.state_bound(rd)[0][0]) + 1.3 * hr.state_bound(rc)[0] + 4 * 2.0 ** -24 * (abs(exp) + 1)
    print(f"loss {loss.item():.9g} ref {exp:.9g} bound {bound:.3g}")
    assert abs(loss.double().item() - exp) <= bound
    g = gd["grad"].numpy().reshape(z.shape) + gc
    gb = L.grad_bound(rd, gd).numpy().reshape(z.shape) + hr.grad_bound(rc, 0.5 * 1.3) + 4 * 2.0 ** -24 * np.abs(g)
    assert bool((np.abs(pred.grad.double().cpu().numpy() - g) <= gb).all())
    with pytest.raises(NotImplementedError):
        seg.WeightedDiceCELoss(ce_kwargs={"reduction": "sum"})
    # CrossEntropyLoss(label_smoothing=...) is the same kernel call
    ce = seg.CrossEntropyLoss(weight=cw.cuda(), ignore_index=2, label_smoothing=0.1)(pred.detach(), yc.cuda())
    assert abs(ce.double().item() - rc["loss"]) <= hr.state_bound(rc)[0]
