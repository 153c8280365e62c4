"""GPU: segk_lovasz_fwd / segk_lovasz_bwd (csrc/lovasz.hip) and the modules on top of them against tests/lovasz_reference.py.

1. exact layer, through the C ABI with this file's own buffers and from the DEVICE's own words: the payload indices of every
   (segment, class) are a permutation, the sorted words and payloads are the stable NumPy order of the words scattered back to
   pixel order, G and n_s are exact, coef equals float32(g) (signed) bit for bit and is +0 where a pixel does not count, every
   L_{s,c} lies within n_s 2^-53 sum |terms| of math.fsum of the same terms (the slack of any float64 summation order), the entering
   classes and a_{s,c} are exact given G and w;
2. float layer: the decoded words lie within err_bound of the float64 errors, the loss within the Lipschitz bound, dlogits within
   grad_bound of the float64 formula evaluated with the device's own coef and a (so a near-tie between the fp32 and the fp64 order
   can neither fail nor be skipped) and exactly 0 where a pixel does not count; on the order cases of the table the device's
   permutation equals the float64 permutation across every adjacent pair whose float64 errors differ by more than twice the
   largest bound of the segment;
3. relations, bit for bit: a second run and a run on a side stream, grad_out = 0.5, LovaszCELoss with one weight at 0, inputs intact;
4. a NaN logit: NaN loss, no fault, finite coefficients;
5. the modules in train_loop, with torch's AdamW and with seg.AdamW twice from one seed.

Outputs are NaN / pattern filled before each call and carry guard elements.  Tolerances: derived or measured in
tests/lovasz_reference.py, none tuned to what the kernels return."""
import functools
import math

import numpy as np
import pytest
import torch

import lovasz_reference as lr

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=None)
def reference(key):
    c = lr.case(*key)
    return lr.lovasz_reference(c["z"], c["y"], **c["kw"])


def run_lovasz(lib, z, y, kw, gout=1.0):
    """one forward and one backward call -> dict of CPU arrays: state float64, loss_out, coef [C, P], the sorted words and
    payloads [C P] and (G, counted slots) [2 Q] out of the scratch buffer, grad [N, C, H, W]"""
    from image_segmentation_amd import ops
    N, C, H, W = z.shape
    P = N * H * W
    per_image, classes = int(kw["per_image"]), int(kw["classes"] == "all")
    S = N if per_image else 1
    cw, ign = kw.get("cw"), kw.get("ignore_index")
    ign = -1 if ign is None else int(ign)
    zd, yd = torch.from_numpy(z).cuda().contiguous(), torch.from_numpy(y).cuda().contiguous()
    cwd = None if cw is None else torch.from_numpy(np.asarray(cw, dtype=np.float32)).cuda()
    nwords = lr.scratch_words(C, P, S)
    assert 4 * nwords == ops.lovasz_scratch_bytes(C, P, S)
    scratch = torch.full((nwords + GUARD,), FILL, dtype=torch.int32, device="cuda")
    coef = torch.full((C * P + GUARD,), float("nan"), device="cuda")
    state = torch.full((lr.state_doubles(C, S) + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((1,), float("nan"), device="cuda")
    go = torch.tensor([gout], dtype=torch.float32, device="cuda")
    dl = torch.full((z.size + GUARD,), float("nan"), device="cuda")
    p = lambda t: 0 if t is None else t.data_ptr()
    lib.call("segk_lovasz_fwd", zd.data_ptr(), yd.data_ptr(), p(cwd), N, C, H * W, ign, per_image, classes, scratch.data_ptr(),
             4 * nwords, coef.data_ptr(), state.data_ptr(), out.data_ptr(), ops._stream())
    lib.call("segk_lovasz_bwd", zd.data_ptr(), yd.data_ptr(), coef.data_ptr(), state.data_ptr(), go.data_ptr(), N, C, H * W, ign,
             per_image, dl.data_ptr(), ops._stream())
    torch.cuda.current_stream().synchronize()
    assert bool((scratch[nwords:] == FILL).all()), "the scratch buffer's guard was written"
    assert bool(torch.isnan(coef[C * P:]).all()) and bool(torch.isnan(dl[z.size:]).all()), "a guard was written"
    assert bool(torch.isnan(state[lr.state_doubles(C, S):]).all()), "the state's guard was written"
    assert (zd.cpu().numpy().view(np.uint32) == z.view(np.uint32)).all() and (yd.cpu().numpy() == y).all(), "an input was written"
    sc = scratch[:nwords].cpu().numpy().view(np.uint32)
    o = lr.layout(C, P, S)
    return dict(state=state[:lr.state_doubles(C, S)].cpu().numpy(), loss_out=out.cpu().numpy(),
                coef=coef[:C * P].cpu().numpy().reshape(C, P), words=sc[o["words"]:o["words"] + C * P],
                pays=sc[o["pays"]:o["pays"] + C * P], gn=sc[o["gn"]:o["gn"] + 2 * C * S],
                grad=dl[:z.size].cpu().numpy().reshape(z.shape))


def check_exact(c, r, d):
    """section 1 of the module docstring; returns the device's words in pixel order [P, C]"""
    C, S, L, P = r["C"], r["S"], r["L"], r["P"]
    Q = S * C
    st = d["state"]
    w = lr._weights(c["kw"].get("cw"), C)
    uw = np.zeros((P, C), dtype=np.uint32)
    G, n_s, Lsc = np.zeros((S, C), dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros((S, C))
    for s in range(S):
        for k in range(C):
            q = k * S + s
            sw, sp = d["words"][q * L:(q + 1) * L], d["pays"][q * L:(q + 1) * L]
            idx, fgs = (sp & 0x7FFFFFFF).astype(np.int64), (sp >> 31).astype(bool)
            assert (np.sort(idx) == np.arange(L)).all(), f"{c['desc']}: payloads of ({s}, {k}) are no permutation"
            seg = np.zeros(L, dtype=np.uint32)
            seg[idx] = sw
            uw[s * L:(s + 1) * L, k] = seg
            ufg = np.zeros(L, dtype=bool)
            ufg[idx] = fgs
            assert ((seg != 0) == r["counted"][s * L:(s + 1) * L]).all() and (ufg == r["fg"][s * L:(s + 1) * L, k]).all(), c["desc"]
            order = lr.stable_order(seg)
            assert (idx == order).all() and (sw == seg[order]).all(), f"{c['desc']}: ({s}, {k}) is not the stable order"
            n = int((sw != 0).sum())
            G[s, k], n_s[s] = int(fgs.sum()), n
            assert (int(d["gn"][q]), int(d["gn"][Q + q])) == (G[s, k], n), c["desc"]
            g = lr.coefficients(fgs[:n])
            want = np.zeros(L, dtype=np.float32)
            want[idx[:n]] = np.where(fgs[:n], -g, g).astype(np.float32)
            assert (d["coef"][k, s * L:(s + 1) * L].view(np.uint32) == want.view(np.uint32)).all(), f"{c['desc']}: coef of ({s}, {k})"
            with np.errstate(all="ignore"):
                terms = lr.word_value(sw[:n]) * g
            dev = float(st[2 + s * C + k])
            if np.isnan(terms).any():
                assert math.isnan(dev), c["desc"]
            else:
                exact = math.fsum(terms)
                assert abs(dev - exact) <= n * 2.0 ** -53 * float(np.abs(terms).sum()), f"{c['desc']}: L of ({s}, {k}): {dev} {exact}"
            Lsc[s, k] = dev
    assert (G == r["G"]).all() and (n_s == r["n_s"]).all(), c["desc"]
    assert (st[2 + 2 * Q:2 + 3 * Q].reshape(S, C) == G).all() and (st[2 + 4 * Q:2 + 4 * Q + S] == n_s).all() and st[1] == n_s.sum()
    enters = (n_s[:, None] > 0) & ((G > 0) if c["kw"]["classes"] == "present" else np.ones((S, C), dtype=bool))
    assert (st[2 + 3 * Q:2 + 4 * Q].reshape(S, C) == enters).all(), c["desc"]
    _, a = lr.entering_weights(enters, w, S)
    a_dev = st[2 + Q:2 + 2 * Q].reshape(S, C)
    assert (a_dev.astype(np.float32).view(np.uint32) == a.view(np.uint32)).all() and (a_dev == a.astype(np.float64)).all(), c["desc"]
    assert d["loss_out"].astype(np.float64)[0] == st[0] or (math.isnan(st[0]) and math.isnan(d["loss_out"][0]))
    return uw, a


def check_float(c, r, d, uw, a, order_check):
    """section 2 of the module docstring"""
    C, S, L, P = r["C"], r["S"], r["L"], r["P"]
    cnt = r["counted"]
    eb = lr.err_bound(r)
    fin = cnt[:, None] & np.isfinite(r["err"])
    dev_err = lr.word_value(uw)
    worst = float(np.max(np.abs(dev_err - r["err"])[fin] / eb[fin])) if fin.any() else 0.0
    lb = lr.loss_bound(r)
    print(f"{c['desc']}: loss {d['state'][0]:.9g} ref {r['loss']:.9g} bound {lb:.3g}  worst err / bound {worst:.3f}")
    assert (np.abs(dev_err - r["err"])[fin] <= eb[fin]).all(), c["desc"]
    if math.isnan(r["loss"]):
        assert math.isnan(d["state"][0])
    else:
        assert abs(d["state"][0] - r["loss"]) <= lb, c["desc"]
    if r["n"] == 0:
        assert d["loss_out"].view(np.uint32)[0] == 0 and not d["coef"].view(np.uint32).any() and not d["grad"].view(np.uint32).any()
    ref = lr.lovasz_grad_reference(r, c["gout"], coef=d["coef"], a=a)
    gb = lr.grad_bound(r, d["coef"], a, c["gout"])
    ok = np.isfinite(ref)
    assert (np.abs(d["grad"].astype(np.float64) - ref)[ok] <= gb[ok]).all(), c["desc"]
    off = ~np.broadcast_to(lr.unrows(np.repeat(cnt[:, None], C, 1), r["shape"]), r["shape"])
    assert not d["grad"].view(np.uint32)[off].any(), f"{c['desc']}: a gradient where no pixel counts"
    if order_check:
        for s in range(S):
            for k in range(C):
                n = int(r["n_s"][s])
                if n < 2:
                    continue
                decisive = lr.tie_free_pairs(r, s, k)
                block = np.zeros(L, dtype=np.int64)
                block[r["perm"][s, k][:n]] = np.concatenate([[0], np.cumsum(decisive)])
                dev_order = lr.stable_order(uw[s * L:(s + 1) * L, k])[:n]
                assert (block[dev_order] == block[r["perm"][s, k][:n]]).all(), f"{c['desc']}: order of ({s}, {k})"


@pytest.mark.parametrize("C", lr.CLASSES)
def test_table(lib, C):
    for key in lr.table():
        if key[0] != C:
            continue
        c, r = lr.case(*key), reference(key)
        d = run_lovasz(lib, c["z"], c["y"], c["kw"], c["gout"])
        uw, a = check_exact(c, r, d)
        check_float(c, r, d, uw, a, lr.order_case(c))


def test_one_case_above_the_scan_levels(lib):
    """1025 tiles in one segment: every wave of the radix scan walks 65 tiles, the fg scan takes a second chunk"""
    c = lr.big_case()
    r = lr.lovasz_reference(c["z"], c["y"], **c["kw"])
    d = run_lovasz(lib, c["z"], c["y"], c["kw"], c["gout"])
    uw, a = check_exact(c, r, d)
    check_float(c, r, d, uw, a, False)


def test_a_nan_logit_gives_a_nan_loss_and_no_fault(lib):
    N, C, L = 3, 3, lr.TILE + 1
    z, y, _ = lr.inputs("normal", C, N, L, 77)
    z[1, 2, 0, 5] = np.nan
    d = run_lovasz(lib, z, y, dict(cw=None, ignore_index=None, per_image=True, classes="present"))
    assert math.isnan(d["state"][0]) and math.isnan(d["loss_out"][0])
    assert np.isfinite(d["coef"]).all()
    assert np.isfinite(d["state"][1]) and np.isfinite(d["state"][2 + N * C:]).all()          # n; a, G, the entering classes, n_s
    per_class = d["state"][2:2 + N * C].reshape(N, C)
    assert np.isnan(per_class[1]).all() and np.isfinite(per_class[[0, 2]]).all()
    bad = np.zeros(z.shape, dtype=bool)
    bad[1, :, 0, 5] = True
    assert np.isfinite(d["grad"][~bad]).all()


RELATION_KEYS = ((3, 3, 9, True), (2, 1, 7, False), (8, 3, 5, True))


@pytest.mark.parametrize("key", RELATION_KEYS)
def test_runs_are_bit_stable_and_grad_out_scales(lib, key):
    c = lr.case(*key)
    a = run_lovasz(lib, c["z"], c["y"], c["kw"], 1.0)
    b = run_lovasz(lib, c["z"], c["y"], c["kw"], 1.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run_lovasz(lib, c["z"], c["y"], c["kw"], 1.0)
    torch.cuda.current_stream().wait_stream(side)
    for other in (b, s):
        assert (other["state"].view(np.uint64) == a["state"].view(np.uint64)).all()
        assert (other["loss_out"].view(np.uint32) == a["loss_out"].view(np.uint32)).all()
        assert (other["coef"].view(np.uint32) == a["coef"].view(np.uint32)).all()
        assert (other["grad"].view(np.uint32) == a["grad"].view(np.uint32)).all()
        assert (other["words"] == a["words"]).all() and (other["pays"] == a["pays"]).all()
    h = run_lovasz(lib, c["z"], c["y"], c["kw"], 0.5)
    assert (h["grad"].view(np.uint32) == (np.float32(0.5) * a["grad"]).view(np.uint32)).all()


# ------------------------------------------------------------------------------------------------ modules and loops
def _logits(seed=3):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((2, 3, 24, 29), generator=g).cuda().requires_grad_(True)
    y = torch.randint(0, 3, (2, 24, 29), generator=g)
    y.view(-1)[::11] = 2
    return z, y.cuda()


def _value_and_grad(loss_fn, seed=3):
    z, y = _logits(seed)
    keep = z.detach().clone()
    loss = loss_fn(z, y)
    loss.backward()
    assert torch.equal(z.detach(), keep)
    return loss.detach().cpu().numpy().view(np.uint32), z.grad.cpu().numpy().view(np.uint32)


def test_lovasz_ce_with_one_weight_at_zero_is_the_other_term(lib):
    import image_segmentation_amd as seg
    cw = torch.tensor([0.5, 1.0, 2.0]).cuda()
    for per_image in (False, True):
        kw = dict(class_weights=cw, ignore_index=2, per_image=per_image)
        ce = _value_and_grad(seg.CrossEntropyLoss(weight=cw, ignore_index=2))
        both = _value_and_grad(seg.LovaszCELoss(lovasz_weight=0.0, **kw))
        assert (ce[0] == both[0]).all() and (ce[1] == both[1]).all()
        lv = _value_and_grad(seg.LovaszSoftmaxLoss(per_image=per_image, weight=cw, ignore_index=2))
        both = _value_and_grad(seg.LovaszCELoss(ce_weight=0.0, lovasz_weight=1.0, **kw))
        assert (lv[0] == both[0]).all() and (lv[1] == both[1]).all()
        assert lv[1].any()


def test_module_matches_float64_and_reports_last(lib):
    import image_segmentation_amd as seg
    z, y = _logits(4)
    cw = np.array([0.5, 1.0, 2.0], dtype=np.float32)
    loss_fn = seg.LovaszSoftmaxLoss(per_image=True, classes="all", weight=torch.from_numpy(cw).cuda(), ignore_index=1)
    loss = loss_fn(z, y[:, None])
    (loss * 0.5).backward()
    r = lr.lovasz_reference(z.detach().cpu().numpy(), y.cpu().numpy(), cw=cw, ignore_index=1, per_image=True, classes="all")
    assert abs(loss.double().item() - r["loss"]) <= lr.loss_bound(r)
    last = loss_fn.last
    assert all(last[k].is_cuda for k in ("n", "present", "per_class"))
    assert int(last["n"].item()) == r["n"] and last["present"].dtype == torch.int32
    assert (last["present"].cpu().numpy() == r["enters"]).all() and tuple(last["per_class"].shape) == (2, 3)
    eb = float(lr.err_bound(r)[r["counted"]].max())
    assert (np.abs(last["per_class"].cpu().numpy() - r["per_class"]) <= eb + 1e-12).all()
    with pytest.raises(RuntimeError):
        loss_fn(z.detach().cpu(), y.cpu())


def _model(seed=11):
    import image_segmentation_amd as seg
    torch.manual_seed(seed)
    return seg.unet(3, 3).cuda()


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((2, 3, 32, 32), generator=g), torch.randint(0, 3, (2, 1, 32, 32), generator=g)


def test_train_loop_with_lovasz_ce(lib, monkeypatch):
    import image_segmentation_amd as seg
    from image_segmentation_amd import training
    monkeypatch.setattr(training, "VERBOSE", False)
    m = _model()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    loss_fn = seg.LovaszCELoss(per_image=True)
    X, y = _batch(1)
    loss = loss_fn(m(X.cuda()), y.cuda())
    loss.backward()
    assert math.isfinite(loss.item())
    for name, prm in m.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
    opt.zero_grad()
    val = training.train_loop([_batch(1), _batch(2)], m, loss_fn, opt, 1, "cuda")
    assert math.isfinite(float(val))


def test_train_loop_under_seg_adamw_is_bit_stable(lib, monkeypatch):
    import image_segmentation_amd as seg
    from image_segmentation_amd import training
    monkeypatch.setattr(training, "VERBOSE", False)
    out = []
    for _ in range(2):
        m = _model()
        opt = seg.AdamW(m.parameters(), lr=1e-3)
        val = training.train_loop([_batch(1), _batch(2)], m, seg.LovaszCELoss(), opt, 1, "cuda")
        out.append((float(val), {k: v.detach().clone() for k, v in m.state_dict().items()}))
    assert out[0][0] == out[1][0] and math.isfinite(out[0][0])
    for k, v in out[0][1].items():
        assert torch.equal(v, out[1][1][k]), k
