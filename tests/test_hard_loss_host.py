"""CPU: the float64 reference of the hard-pixel losses (tests/hard_loss_reference.py) against torch, its analytic gradient
against autograd, the radix-select restatement against np.partition, the case table's coverage, the measured constants, the
ABI table, the modules' argument rules, and the compiled code of csrc/hard_loss.hip (no spills, no self-waiting loads)."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import hard_loss_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _torch_loss(c, z64):
    """the definition in torch float64 ops on z64 [N, C, H, W] (requires grad), over the reference's kept set"""
    r, kw = c["ref"], c["kw"]
    N, C, H, W = r["shape"]
    zr = z64.permute(0, 2, 3, 1).reshape(-1, C)
    nl = torch.logsumexp(zr, 1, keepdim=True) - zr
    p = torch.softmax(zr, 1)
    oh = torch.from_numpy(r["oh"])
    w = torch.from_numpy(r["w"].astype(np.float64))
    wt = torch.from_numpy(r["wt"].astype(np.float64))
    eps = r["eps"]
    a = oh * ((1 - eps) * wt)[:, None] + (eps / C) * w[None, :]
    if eps == 0.0:
        ce = wt * (nl * oh).sum(1)
    else:
        ce = (a * nl).sum(1)
    u = (p * ~oh).sum(1)
    l = u ** r["gamma"] * ce if r["gamma"] != 0.0 else ce
    kept = torch.from_numpy(r["kept"])
    D = wt[kept].sum()
    return l[kept].sum() / D, D


@pytest.mark.parametrize("ci", range(len(hr.CLASSES)))
def test_reference_equals_torch_cross_entropy(ci):
    """gamma = 0, selection off: torch.nn.functional.cross_entropy(weight, ignore_index, label_smoothing) in float64"""
    C = hr.CLASSES[ci]
    for si, (N, H, W) in enumerate(hr.SHAPES):
        for eps in hr.SMOOTHS:
            for weighted in (False, True):
                z, y = hr.inputs(C, N, H, W, 29700 + 10 * ci + si)
                ign = (si % C) if si % 2 else None
                cw = (0.5 + 0.25 * np.arange(C)).astype(np.float32) if weighted else None
                r = hr.hard_reference(z, y, cw=cw, ignore_index=ign, eps=eps)
                if r["n"] == 0:
                    assert math.isnan(r["loss"])
                    continue
                ref = torch.nn.functional.cross_entropy(torch.from_numpy(z).to(F64), torch.from_numpy(y),
                                                        weight=None if cw is None else torch.from_numpy(cw).to(F64),
                                                        ignore_index=-100 if ign is None else ign, label_smoothing=hr.f32(eps))
                assert abs(r["loss"] - ref.item()) <= 1e-12 * max(1.0, abs(ref.item())), (C, N, H, W, eps, weighted, ign)


@pytest.mark.parametrize("ci,ri", hr.table())
def test_analytic_gradient_equals_autograd(ci, ri):
    c = hr.case(ci, ri)
    r = c["ref"]
    z64 = torch.from_numpy(c["z"]).to(F64).requires_grad_(True)
    g = hr.hard_grad_reference(r, c["gout"])
    if not r["D"] > 0:
        assert not g.any() and (math.isnan(r["loss"]) if r["n"] == 0 else r["loss"] == 0.0), c["desc"]
        return
    loss, D = _torch_loss(c, z64)
    assert abs(loss.item() - r["loss"]) <= 1e-12 * max(1.0, abs(r["loss"])), c["desc"]
    ga, = torch.autograd.grad(loss * hr.f32(c["gout"]), z64)
    assert np.abs(ga.numpy() - g).max() <= 1e-12 * max(1.0, np.abs(g).max()), c["desc"]
    assert not g[~np.broadcast_to(hr.unrows(np.repeat(r["kept"][:, None], r["C"], 1), r["shape"]), g.shape)].any()


def test_word_cases_gradient_and_select():
    for name, z, y, kw in hr.word_cases():
        r = hr.hard_reference(z, y, **kw)
        r32 = hr.hard_reference(z, y, dt=np.float32, **kw)
        words = hr.words_of(r32["kappa"], r32["counted"])
        tw, n, nk = hr.select_words(words, r["theta"], r["min_kept"], r["q16"])
        assert (tw, n, nk) == hr.select_words(words, r["theta"], r["min_kept"], r["q16"], select=hr.exact_select), name
        assert n == r["n"] and r["k"] >= 1, name
    # the named properties
    cases = {name: (z, y, kw) for name, z, y, kw in hr.word_cases()}
    w = lambda name: hr.words_of(*(lambda r: (r["kappa"], r["counted"]))(hr.hard_reference(*cases[name][:2], dt=np.float32, **cases[name][2])))
    assert len(set(w("all words equal").tolist())) == 1
    low = w("words differing in the low 10 bits")
    assert len(set(low.tolist())) > 100 and len(set((low >> 10).tolist())) == 1
    assert 1 in w("one key of exactly 0").tolist()
    assert 0x7F800001 in w("one +inf key").tolist()
    assert hr.NAN_WORD in w("one NaN pixel").tolist()
    top = w("the k-th in the top bin")
    assert hr.radix_select(top, 1) == top.max()


def test_radix_select_equals_partition_on_adversarial_word_sets():
    g = np.random.default_rng(5)
    sets = [np.full(300, 0x3F800001, dtype=np.uint32),                                   # all equal
            (0x3F800000 + g.integers(1, 1024, 500)).astype(np.uint32),                   # the low 10 bits only
            (0x3F800000 + (g.integers(0, 2048, 500) << 10)).astype(np.uint32) + 1,       # the middle 11 bits only
            (g.integers(0, 2048, 500).astype(np.uint32) << 21) + 1,                      # the top 11 bits only
            g.integers(1, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32),             # anything
            np.array([1, 0x7F800001, hr.NAN_WORD, 0, 0, 5, 5, 5], dtype=np.uint32),      # key 0, +inf, NaN, uncounted pixels, ties
            np.concatenate([np.zeros(50, dtype=np.uint32), np.array([7], dtype=np.uint32)])]
    for s in sets:
        n = int((s != 0).sum())
        for k in sorted(k for k in {1, 2, n // 2, n - 1, n} if 1 <= k <= n):
            assert hr.radix_select(s, k) == hr.exact_select(s, k), (s[:4], k)
            assert hr.exact_select(s, k) == int(np.sort(s[s != 0])[n - k])


def test_case_table_reaches_every_regime_and_setting():
    seen = dict(C=set(), regime=set(), gamma=set(), eps=set(), gout=set(), weights=set(), ignore=set(), shape=set())
    outside = False
    for c in hr.all_cases():
        r, kw = c["ref"], c["kw"]
        seen["C"].add(r["C"]); seen["regime"].add(c["regime"]); seen["gamma"].add(kw["gamma"]); seen["eps"].add(kw["eps"])
        seen["gout"].add(c["gout"]); seen["weights"].add(kw["cw"] is not None); seen["ignore"].add(kw["ignore_index"] is not None)
        seen["shape"].add(r["shape"][0:1] + r["shape"][2:])
        outside |= bool(((c["y"] >= r["C"]) & (c["y"] != 255)).any() and (c["y"] < 0).any())
        assert hr.regime_holds(r, c["regime"]), c["desc"]
        if c["set_check"]:
            assert not hr.undecided(r).any(), c["desc"]
    assert seen["C"] == set(hr.CLASSES) and seen["regime"] == set(hr.REGIMES) and seen["gamma"] == set(hr.GAMMAS)
    assert seen["eps"] == set(hr.SMOOTHS) and seen["gout"] == set(hr.GOUTS) and seen["weights"] == {False, True}
    assert seen["ignore"] == {False, True} and seen["shape"] == set(hr.SHAPES) and outside
    # every regime meets every class count, and each gamma and smoothing some selection
    sel = [c for c in hr.all_cases() if c["ref"]["selecting"]]
    assert {c["kw"]["gamma"] for c in sel} == set(hr.GAMMAS) and {c["kw"]["eps"] for c in sel} == set(hr.SMOOTHS)


def test_measured_constants_leave_a_factor_of_four():
    worst_l = worst_g = 0.0
    todo = [(c["z"], c["y"], c["kw"]) for c in hr.all_cases()] + [(z, y, kw) for _, z, y, kw in hr.word_cases()]
    for z, y, kw in todo:
        kl, kg = hr.measure(hr.hard_reference(z, y, **kw), hr.hard_reference(z, y, dt=np.float32, **kw))
        worst_l, worst_g = max(worst_l, kl), max(worst_g, kg)
    print(f"k_l = {worst_l:.4f} (K_L = {hr.K_L}), k_g = {worst_g:.4f} (K_G = {hr.K_G})")
    assert 0 < worst_l <= hr.K_L / 4 and 0 < worst_g <= hr.K_G / 4


def test_restatement_lies_within_the_bounds():
    """the float32 restatement (NumPy's expf / logf / powf, the kernel's order of additions) against float64: loss, S, D and the
    keys within the bounds the device is held to, and the same kept set where the table promises one"""
    for c in hr.all_cases():
        r = c["ref"]
        loss, S, D, r32 = hr.restated_loss(c["z"], c["y"], **c["kw"])
        if c["set_check"] or not r["selecting"]:
            assert (r32["kept"] == r["kept"]).all(), c["desc"]
            e_loss, e_S, e_D = hr.state_bound(r)
            if math.isnan(r["loss"]):
                assert math.isnan(loss)
            else:
                assert abs(float(loss) - r["loss"]) <= e_loss and abs(float(S) - r["S"]) <= e_S and abs(float(D) - r["D"]) <= e_D, c["desc"]
        ok = r["counted"] & np.isfinite(r["kappa"])
        assert (np.abs(r32["kappa"].astype(np.float64) - r["kappa"])[ok] <= hr.key_bound(r)[ok]).all(), c["desc"]


def test_abi_table_holds_both_entries():
    from image_segmentation_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "segk.h")).read(), flags=re.S)
    for name in ("segk_hard_loss_fwd", "segk_hard_loss_bwd"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m is not None and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    words = int(re.search(r"#define\s+SEGK_HARD_HIST_WORDS\s+(\d+)", txt).group(1))
    from image_segmentation_amd import ops
    assert words == ops.HARD_HIST_WORDS == hr.HIST_WORDS


def test_constructor_rules():
    from image_segmentation_amd import losses
    import image_segmentation_amd as pkg
    assert pkg.HardPixelLoss is losses.HardPixelLoss and pkg.FocalLoss is losses.FocalLoss
    assert pkg.OhemCrossEntropyLoss is losses.OhemCrossEntropyLoss
    for bad in (dict(gamma=0.5), dict(gamma=-1.0), dict(gamma=8.5), dict(gamma=math.nan), dict(label_smoothing=1.0),
                dict(label_smoothing=-0.1), dict(thresh=0.0), dict(thresh=1.5), dict(thresh=-0.2), dict(min_kept=-1),
                dict(min_fraction=-0.1), dict(min_fraction=1.1)):
        with pytest.raises(ValueError):
            losses.HardPixelLoss(**bad)
    with pytest.raises(ValueError):
        losses.CrossEntropyLoss(label_smoothing=1.0)
    with pytest.raises(ValueError):
        losses.FocalLoss(gamma=0.25)
    with pytest.raises(ValueError):
        losses.OhemCrossEntropyLoss(thresh=2.0)
    with pytest.raises(NotImplementedError):
        losses.WeightedDiceCELoss(ce_kwargs={"reduction": "sum"})
    with pytest.raises(NotImplementedError):
        losses.WeightedDiceCELoss(ce_kwargs={"label_smoothing": 0.1, "weight": None})
    with pytest.raises(ValueError):
        losses.WeightedDiceCELoss(ce_kwargs={"label_smoothing": 1.0})
    assert losses.WeightedDiceCELoss(ce_kwargs={"label_smoothing": 0.1}).label_smoothing == 0.1
    m = losses.HardPixelLoss()
    assert m.selection() is None and m.gamma == 0.0 and m.label_smoothing == 0.0
    assert losses.FocalLoss().gamma == 2.0 and losses.FocalLoss().selection() is None
    th, mk, q = losses.OhemCrossEntropyLoss(min_fraction=0.25).selection()
    assert np.float32(th) == np.float32(hr.theta_of(0.7)) and mk == 0 and q == 16384
    th, mk, q = losses.HardPixelLoss(thresh=1.0, min_kept=5).selection()
    assert th == 0.0 and math.copysign(1.0, th) == 1.0 and mk == 5 and q == 0
    assert losses.HardPixelLoss(min_kept=3).selection()[0] == math.inf


def test_which_autograd_node_each_module_calls(monkeypatch):
    """CrossEntropyLoss(label_smoothing=0.0) stays on SegLossFn; smoothing, focal and OHEM go through HardLossFn"""
    from image_segmentation_amd import losses, ops
    calls = []

    class Seg:
        @staticmethod
        def apply(*a):
            calls.append(("seg", a[2:]))
            return torch.zeros(())

    class Hard:
        @staticmethod
        def apply(*a):
            calls.append(("hard", a[2:]))
            return torch.zeros(()), torch.zeros(28)

    monkeypatch.setattr(ops, "SegLossFn", Seg)
    monkeypatch.setattr(ops, "HardLossFn", Hard)
    x, y = torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64)
    losses.CrossEntropyLoss()(x, y)
    losses.CrossEntropyLoss(label_smoothing=0.0, ignore_index=1)(x, y)
    assert calls == [("seg", (None, None, 0.0, 0.0, 1.0)), ("seg", (None, 1, 0.0, 0.0, 1.0))]
    calls.clear()
    losses.CrossEntropyLoss(label_smoothing=0.1)(x, y)
    assert calls == [("hard", (None, None, 0.1, 0.0, None))]
    calls.clear()
    losses.WeightedDiceCELoss()(x, y)
    assert [c[0] for c in calls] == ["seg"] and calls[0][1][3:] == (1.0, 1.0)
    calls.clear()
    losses.WeightedDiceCELoss(dice_weight=0.5, ce_kwargs={"label_smoothing": 0.1})(x, y)
    assert calls == [("seg", (None, None, 1e-5, 1.0, 0.0)), ("hard", (None, None, 0.1, 0.0, None))]
    calls.clear()
    m = losses.OhemCrossEntropyLoss(thresh=0.7, min_kept=10)
    m(x, y.unsqueeze(1))
    assert calls[0][0] == "hard" and calls[0][1][2:4] == (0.0, 0.0) and calls[0][1][4][1:] == (10, 0)
    assert set(m.last) == {"n", "n_kept", "threshold"}
    calls.clear()
    losses.FocalLoss()(x, y)
    assert calls == [("hard", (None, None, 0.0, 2.0, None))]
    with pytest.raises(ValueError):
        losses.HardPixelLoss()(x, torch.zeros(1, 3, 2, 2, dtype=torch.int64))


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_compiled_unit_has_no_spills_and_no_self_waiting_loads():
    seen = set()
    for n_ser, n_loads, _, name in _load_tool("serialized_loads").scan("hard_loss"):
        for h in ("hard_key_kernel", "hard_refine_kernel", "hard_fwd_kernel", "hard_bwd_kernel"):
            if h in name:
                seen.add(h)
                assert n_ser <= 2, f"{name}: {n_ser} of {n_loads} loads wait for themselves"
    assert len(seen) == 4, seen
    rows = _load_tool("spill_report").report("hard_loss")
    assert len(rows) >= 3 + 2 + 12 + 12
    for r in rows:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
