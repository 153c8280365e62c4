"""Pins tests/loss_reference.py itself (no GPU): its values and analytic gradients against float64 torch autograd through a plain
restatement built on torch's own softmax / cross_entropy / nll_loss, against the fp32 oracle, against the golden files captured
from the reference project, its launch arithmetic on hand-computed values, and the measured math-library constants of its
docstring (no case of the matrix may exceed a quarter of the constant the bounds use)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_reference as L
from oracle import losses_ref, prompt_ref
from oracle.fill import fill, labels as fill_labels

CW4 = [0.2046795970925636, 1.0271954434416883, 1.2293222812780409, 0.5]      # tests/test_gpu_prompt.py


def restated(x, y, cw=None, ignore_index=None, smooth=1e-5, dice_weight=1.0, ce_weight=1.0, prob=False, nll_log=1, eps=0.0):
    """the same loss written the way the oracle writes it, in float64 on a leaf tensor"""
    x = x.to(torch.float64).requires_grad_(True)
    N, C, HW = x.shape
    ign = -1 if ignore_index is None else ignore_index
    s, dwt, cwt, eps = L.f32(smooth), L.f32(dice_weight), L.f32(ce_weight), L.f32(eps)
    w = None if cw is None else cw.double()
    p = x if prob else torch.softmax(x, 1)
    onehot = torch.stack([(y == k) for k in range(C)], 1).double()
    inter, sp, sg = (p * onehot).sum(2).sum(0), p.sum(2).sum(0), onehot.sum(2).sum(0)
    dc = (2.0 * inter + s) / torch.clip(sp + sg + s, 1e-8)
    valid = torch.tensor([not (0 <= ign < C and k == ign) for k in range(C)])
    if w is not None:
        dice = -((dc[valid] * w[valid]).sum() / w[valid].sum().clamp(min=1e-8))
    else:
        dice = -dc[valid].mean()
    t = torch.where((y >= 0) & (y < C) & (y != ign), y, torch.full_like(y, -100))
    z = x if not prob else (torch.log(x + eps) if nll_log else x)
    ce = F.nll_loss(z, t, weight=w) if prob else F.cross_entropy(x, t, weight=w)
    return (dwt * dice + cwt * ce) if cwt != 0 else dwt * dice, dice, ce, x


def close(a, b, rel=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    if torch.isnan(b).any():
        return bool((torch.isnan(a) == torch.isnan(b)).all()) and close(a.nan_to_num(0.0), b.nan_to_num(0.0), rel)
    return bool(((a - b).abs() <= rel * b.abs().max().clamp(min=1e-300)).all())


def check_case(x, y, kw, gout, desc):
    r = L.loss_reference(x, y, **kw)
    gr = L.loss_grad_reference(r, gout)
    loss, dice, ce, leaf = restated(x, y, **kw)
    assert close(r["dice"], dice.detach()), desc
    assert close(r["ce"], ce.detach()), desc
    assert close(r["loss"], loss.detach()), desc
    loss.backward()                             # a NaN loss included: torch gives zeros for ignored pixels, 0 / 0 for zero weights
    assert close(gr["grad"], leaf.grad * L.f32(gout)), desc


@pytest.mark.parametrize("prob", [False, True], ids=["softmax", "prob"])
@pytest.mark.parametrize("C", range(1, 9))
def test_reference_equals_float64_autograd(C, prob):
    """every class count and every option combination of the GPU matrix, on the shapes up to 131 100 pixels (the larger ones
    repeat the same options), plus the semantic edges"""
    for si in range(8):
        x, y, kw, gout, desc = L.loss_case(C, si, prob)
        if kw["cw"] is not None and kw["ignore_index"] is not None and float((kw["cw"] * (torch.arange(C) != kw["ignore_index"])).sum()) == 0:
            continue
        check_case(x, y, kw, gout, desc)


def test_reference_edges_equal_float64_autograd():
    for name, x, y, kw, gout in L.edge_cases():
        if "weights zero" in name:
            r = L.loss_reference(x, y, **kw)
            assert r["dice"].item() == 0.0 and torch.isnan(r["ce"]) and r["loss"].item() == 0.0 and (r["a"] == 0).all()
        check_case(x, y, kw, gout, name)
    name, x, y, kw, gout = L.edge_cases()[1]
    r = L.loss_reference(x, y, **kw)
    g = L.loss_grad_reference(r, gout)
    assert bool(r["clip"][1]) and r["dc"][1].item() == 0.0 and g["G0"][1].item() == 0.0 and (g["grad"][:, 1] == 0).all()
    name, x, y, kw, gout = L.edge_cases()[2]
    r = L.loss_reference(x, y, **kw)
    assert torch.isnan(r["loss"]) and r["ce_den"].item() == 0.0 and torch.isfinite(L.loss_grad_reference(r, gout)["grad"]).all()


@pytest.mark.parametrize("C", range(1, 9))
def test_reference_agrees_with_fp32_oracle(C):
    """oracle/losses_ref.py and oracle/prompt_ref.py on fp32 tensors: within fp32 distance (64 * 2^-24 relative to max(1, |v|):
    the oracle adds a few thousand fp32 terms pairwise)"""
    tol = lambda v: 64 * L.U24 * max(1.0, abs(v))
    for si in (1, 2, 3):
        x, y = L.loss_inputs(C, *L.LOSS_SHAPES[si][:2], 900 + C + si)
        N, _, HW = x.shape
        cw = torch.linspace(0.3, 1.7, C) if si != 1 else None
        ign = C - 1 if (si == 3 and C > 1) else None
        x4, y3 = x.view(N, C, HW, 1), y.view(N, HW, 1)
        v = L.loss_reference(x, y, cw=cw, ignore_index=ign, smooth=1.0, dice_weight=0.7, ce_weight=1.3)
        o = losses_ref.dice_ce(x4, y3, 0.7, 1.3, ign, cw, 1.0).item()
        assert abs(v["loss"].item() - o) <= tol(o), (C, si)
        assert abs(v["ce"].item() - losses_ref.cross_entropy(x4, y3, cw, ign).item()) <= tol(v["ce"].item())
        assert abs(v["dice"].item() - losses_ref.soft_dice(x4, y3.unsqueeze(1), 1.0, cw, ign).item()) <= tol(1.0)
        pr = torch.softmax(x, 1) if C > 1 else torch.sigmoid(x)
        v = L.loss_reference(pr, y, cw=cw, ignore_index=ign, smooth=1e-5, dice_weight=0.7, ce_weight=0.3, prob=True, nll_log=1, eps=1e-9)
        o = prompt_ref.dice_nll(pr.view(N, C, HW, 1), y3, 0.7, 0.3, ign, cw, 1e-5, False, lambda t: torch.log(t + 1e-9)).item()
        assert abs(v["loss"].item() - o) <= tol(o), (C, si)
    cl, ml = fill((2, 4, 7, 9), 3, -4, 4), fill((2, 1, 7, 9), 4, -6, 6)
    f, _, _ = L.prompt_mix_reference(cl.view(2, 4, 63), ml.view(2, 63))
    assert (f.view(2, 4, 7, 9) - prompt_ref.prompt_mix(cl, ml).double()).abs().max().item() <= 8 * L.U24


def test_prompt_mix_gradient_equals_autograd():
    cl, ml = fill((3, 4, 50), 5, -4, 4).double(), fill((3, 50), 6, -40, 40).double().requires_grad_(True)
    d = fill((3, 4, 50), 7, -1, 1).double()
    f = prompt_ref.prompt_mix(cl.unsqueeze(-1), ml.unsqueeze(1).unsqueeze(-1)).squeeze(-1)
    (f * d).sum().backward()
    g, _ = L.prompt_mix_grad_reference(cl, ml.detach(), d)
    assert close(g, ml.grad)
    assert close(L.prompt_mix_reference(cl, ml.detach())[0], f.detach())


def test_reference_reproduces_losses_golden(golden):
    """tests/golden/losses_small.npz at the tolerances of test_loss_kernels"""
    g = golden("losses_small")
    x = fill((2, 4, 12, 20), 41, -3, 3).view(2, 4, 240); y = fill_labels((2, 12, 20), 42, 4).view(2, 240)
    w4 = torch.tensor([0.3, 1.1, 0.9, 1.7])
    cases = {"ce": dict(smooth=0.0, dice_weight=0.0, ce_weight=1.0),
             "ce_w": dict(cw=w4, smooth=0.0, dice_weight=0.0, ce_weight=1.0),
             "ce_w_ign3": dict(cw=w4, ignore_index=3, smooth=0.0, dice_weight=0.0, ce_weight=1.0),
             "dice": dict(smooth=1e-5, dice_weight=1.0, ce_weight=0.0),
             "dice_w_ign3": dict(smooth=1.0, cw=w4, ignore_index=3, dice_weight=1.0, ce_weight=0.0),
             "dicece": dict(),
             "dicece_w_ign3": dict(dice_weight=0.7, ce_weight=1.3, ignore_index=3, cw=w4, smooth=1.0)}
    for k, kw in cases.items():
        r = L.loss_reference(x, y, **kw)
        assert abs(r["loss"].item() - float(g[k])) < 5e-6, k
        np.testing.assert_allclose(L.loss_grad_reference(r)["grad"].view(2, 4, 12, 20).numpy(), g[k + "_grad"], rtol=2e-4, atol=2e-8,
                                   err_msg=k)


def test_reference_reproduces_prompt_golden(golden):
    """the loss entries of tests/golden/prompt_small.npz at the tolerances of tests/test_gpu_prompt.py (and the gradients at
    theirs)"""
    g = golden("prompt_small")
    pr = torch.softmax(fill((2, 4, 12, 20), 41, -3, 3), 1).view(2, 4, 240); y = fill_labels((2, 12, 20), 42, 4).view(2, 240)
    cw = torch.tensor(CW4)
    ref = lambda **kw: L.loss_reference(pr, y, **kw)

    def both(tag, parts):
        loss = sum(wt * r["loss"].item() for wt, r in parts)
        grad = sum(wt * L.loss_grad_reference(r)["grad"] for wt, r in parts).view(2, 4, 12, 20).numpy()
        assert abs(loss - float(g[tag + ".loss"])) < 2e-5, tag
        want = g[tag + ".grad"]
        assert np.abs(grad - want).max() < 1e-4 * max(1.0, np.abs(want).max()), tag

    both("prob_log", [(1, ref(prob=True, nll_log=1, eps=1e-9, ignore_index=3, cw=cw, smooth=1.0))])
    both("prob_log_plain", [(1, ref(prob=True, nll_log=1, eps=1e-9))])
    both("prob_identity", [(1, ref(prob=True, nll_log=0, dice_weight=0.7, ce_weight=0.3))])
    both("default_softmax", [(1, ref(cw=cw, dice_weight=1.0, ce_weight=0.0)), (1, ref(cw=cw, prob=True, nll_log=0, dice_weight=0.0))])
    both("softmax_log", [(1, ref(ignore_index=0, dice_weight=1.0, ce_weight=0.0)),
                         (1, ref(ignore_index=0, prob=True, nll_log=1, eps=0.0, dice_weight=0.0))])
    both("dicep_prob", [(1, ref(prob=True, cw=cw, ignore_index=3, smooth=1.0, ce_weight=0.0, nll_log=0))])
    both("dicep_softmax", [(1, ref(ce_weight=0.0))])


def test_launch_arithmetic_by_hand():
    assert L.loss_launch(1) == (1, 1, 16) and L.loss_launch(480) == (1, 1, 16)
    assert L.loss_launch(4096) == (1, 4, 16) and L.loss_launch(4097) == (2, 3, 16)
    assert L.loss_launch(123000)[0] == 31 and L.loss_launch(131072) == (32, 4, 16) and L.loss_launch(131100)[0] == 33
    assert L.loss_launch(1044000)[0] == 255 and L.loss_launch(1045000) == (256, 4, 16)
    assert L.loss_launch(1050000) == (256, 5, 16) and L.loss_launch(3001000) == (256, 12, 16)
    assert L.loss_bwd_launch(1) == (1, 1) and L.loss_bwd_launch(257) == (2, 1) and L.loss_bwd_launch(1048576) == (4096, 1)
    assert L.loss_bwd_launch(1050000) == (4096, 2) and L.loss_bwd_launch(3001000) == (4096, 3)
    assert L.head_blocks(1) == 1 and L.head_blocks(32) == 1 and L.head_blocks(33) == 2 and L.head_blocks(70000) == 1024
    assert L.head_lane_geometry(32) == (8, 32, 1) and L.head_lane_geometry(64) == (16, 16, 1)
    assert L.head_lane_geometry(96) == (24, 10, 1) and L.head_lane_geometry(256) == (64, 4, 1)
    assert L.head_lane_geometry(288) == (64, 4, 2) and L.head_lane_geometry(512) == (64, 4, 2)
    assert L.head_bwd_launch(5, 32) == (1, 1, 32) and L.head_bwd_launch(257, 512) == (9, 8, 4)
    assert L.head_bwd_launch(14000, 256) == (438, 8, 4) and L.head_bwd_launch(70000, 32) == (1024, 3, 32)
    assert L.confusion_launch(255) == (1, 1) and L.confusion_launch(262144) == (1024, 1) and L.confusion_launch(300000) == (1024, 2)
    assert L.chain(4096) == 4 + 6 + 15 + 3


def test_measured_constants_cover_the_matrix():
    """the constants of the bounds are at least 4 x what fp32 CPU torch shows against float64 on every input family of the GPU
    matrix (the shapes above 131 100 pixels draw from the same families; they were measured when the constants were set)"""
    k_sm = k_nll = k_log = k_mix = 0.0
    for C in range(1, 9):
        for si in range(8):
            x, _, _, _, _ = L.loss_case(C, si, False)
            a, b = L.measure_softmax(x)
            k_sm, k_nll = max(k_sm, a), max(k_nll, b)
            x, _, kw, _, _ = L.loss_case(C, si, True)
            if kw["nll_log"]:
                k_log = max(k_log, L.measure_log(x, kw["eps"]))
    for C in L.LARGE_CLASSES:
        a, b = L.measure_softmax(L.loss_inputs(C, 1045, 1000, 77, "sparse")[0])
        k_sm, k_nll = max(k_sm, a), max(k_nll, b)
    for name, x, y, kw, _ in L.edge_cases():
        if kw.get("prob"):
            k_log = max(k_log, L.measure_log(x[x > 0], kw["eps"]))
        else:
            a, b = L.measure_softmax(x)
            k_sm, k_nll = max(k_sm, a), max(k_nll, b)
    for cl, ml in L.mix_cases():
        k_mix = max(k_mix, L.measure_mix(cl, ml))
    print(f"measured: k_sm {k_sm:.3f} k_nll {k_nll:.3f} k_log {k_log:.3f} k_mix {k_mix:.3f}")
    assert 4 * k_sm <= L.K_SM and 4 * k_nll <= L.K_NLL and 4 * k_log <= L.K_LOG and 4 * k_mix <= L.K_MIX


def test_floors_hold_on_the_matrix():
    """the two conditions the GPU test puts on its own bounds, on the shapes that are cheap here: the allowed loss error stays
    below what one dropped pixel changes, the allowed gradient error below 1e-3 of the largest gradient"""
    for prob in (False, True):
        for C in range(1, 9):
            for si in range(1, 6):
                x, y, kw, gout, desc = L.loss_case(C, si, prob)
                r = L.loss_reference(x, y, **kw)
                if L.degenerate(r):
                    continue
                gr = L.loss_grad_reference(r, gout)
                assert L.state_bound(r)[0][0].item() < L.one_pixel_effect(r), desc
                assert L.grad_bound(r, gr).max().item() < 1e-3 * gr["grad"].abs().max().item(), desc
