"""Distillation without a GPU: pins tests/distill_reference.py itself (values and analytic gradient against float64 autograd of
a plain restatement on torch's own kl_div, the measured constant of its docstring, the argmax and gate margins of the case
matrix), the host side of the feature (descriptor table, argument errors, exports) and the compiled kernels (no spills, no
loads that wait for themselves, argument validation of the two entries)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(D.all_cases())


def restated(s, ts, flips, kinds, weights, y=None, ignore_index=None, T=1.0, min_conf=0.0):
    """the same loss the way a torch user would write it, in float64 on a leaf tensor"""
    x = s.to(torch.float64).requires_grad_(True)
    invT, Tsq = D.f32(1.0 / T), D.f32(T * T)
    w = D.table_weights(weights).double()
    q, q1 = 0.0, 0.0
    for t, fl, kd, wv in zip(ts, flips, kinds, w):
        z = D.unflip(t, fl).double()
        if kd:
            z = torch.log(z.clamp(min=2.0 ** -126))
        q = q + wv * torch.softmax(z * invT, 1)
        q1 = q1 + wv * torch.softmax(z, 1)
    klmap = F.kl_div(F.log_softmax(x * invT, 1), q, reduction="none").sum(1)
    counted = q1.max(1).values >= D.f32(min_conf)
    if y is not None and ignore_index is not None:
        counted = counted & (y != ignore_index)
    n = int(counted.sum())
    soft = Tsq * klmap[counted].sum() / n if n else (x * 0).sum()
    return soft, n, x


def close(a, b, rel=1e-11):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return bool(((a - b).abs() <= rel * b.abs().max().clamp(min=1e-300)).all())


def test_package_exports_the_distillation_names():
    import image_segmentation_amd as seg
    from image_segmentation_amd import ops, training, _lib
    for name in ("Teacher", "TeacherViews", "DistillLoss", "train_loop_distill"):
        assert hasattr(seg, name), name
    assert hasattr(ops, "DistillFn") and hasattr(training, "train_loop_distill")
    assert "segk_distill_fwd" in _lib.SIGNATURES and "segk_distill_bwd" in _lib.SIGNATURES


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: f"case{i}")
def test_reference_equals_float64_autograd(idx):
    desc, s, ts, kw, gout = CASES[idx]
    r = D.run_reference(s, ts, kw)
    gr = D.distill_grad_reference(r, gout)
    soft, n, leaf = restated(s, ts, **kw)
    assert r["n"] == n, desc
    # the pixel terms cancel (q log q against q log p): absolute agreement at the size of the terms, not of their difference
    assert abs(float(r["soft"]) - float(soft.detach())) <= 1e-11 * abs(float(soft.detach())) + 1e-13 * r["Tsq"] * (1 + float(r["logp"].abs().max())), desc
    (soft * D.f32(gout)).backward()
    # p - q is the derivative up to (sum of the table weights - 1) p: the weights are rounded to fp32 one by one
    slack = abs(gr["coef"]) * abs(float(r["w32"].double().sum()) - 1.0) * r["p"] * 1.000001
    assert bool(((gr["grad"] - leaf.grad).abs() <= slack + 1e-11 * leaf.grad.abs().max()).all()), desc
    assert abs(float(r["w32"].double().sum()) - 1.0) <= r["V"] * 2.0 ** -25, desc
    if n == 0:
        assert float(r["soft"]) == 0.0 and not gr["grad"].any(), desc


def test_measured_constant_stays_below_a_quarter_of_the_bound():
    """k_kl of the docstring, measured again over the whole matrix: the fp32 host evaluation must stay within K_KL / 4"""
    worst = max(D.measure_kl(D.run_reference(s, ts, kw)) for _, s, ts, kw, _ in CASES)
    print(f"k_kl = {worst:.4f} (K_KL = {D.K_KL})")
    assert worst <= D.K_KL / 4
    assert worst > D.K_KL / 16                  # the constant is not padded either


def test_matrix_decides_its_gates_and_nearly_all_argmaxes():
    """from the float64 reference alone: no pixel's confidence lies within its bound of min_conf (n is exact), and the pixels
    whose argmax is not decided by the bound stay below 1 % of the counted pixels of every case"""
    seen_gate_some = seen_none = seen_tied = 0
    for desc, s, ts, kw, _ in CASES:
        r = D.run_reference(s, ts, kw)
        assert not D.gate_undecided(r).any(), desc
        und = (D.undecided(r) & r["counted"]).sum().item()
        assert und <= 0.01 * r["n"], (desc, und, r["n"])
        seen_gate_some += 0 < r["n"] < int(r["labelled"].sum())
        seen_none += r["n"] == 0
        seen_tied += bool((r["p"].max(1).values == r["p"].min(1).values).all()) and r["C"] > 1
    assert seen_gate_some >= 4 and seen_none >= 2 and seen_tied >= 1


def test_matrix_covers_what_the_kernels_branch_on():
    flips, kinds, views, temps, lab = set(), set(), set(), set(), set()
    for C in range(1, 9):
        per_c = set()
        for si in range(len(D.SHAPES)):
            _, _, kw, _, _ = D.case(C, si)
            flips.update(kw["flips"]); kinds.update(kw["kinds"]); views.add(len(kw["flips"])); temps.add(kw["T"])
            lab.add(kw["y"] is None)
            per_c.add((len(kw["flips"]), kw["T"] != 1.0, kw["y"] is None))
        assert len({v for v, _, _ in per_c}) == 3 and len({t for _, t, _ in per_c}) == 2 and len({y for _, _, y in per_c}) == 2
    assert flips == {0, 1, 2, 3} and kinds == {0, 1} and views == {1, 2, 3} and temps == set(D.TEMPS) and lab == {True, False}
    assert sorted(n * h * w for n, h, w in D.SHAPES[:6]) == [1, 3, 255, 257, 1023, 4097]


def test_launch_arithmetic_matches_the_library():
    from image_segmentation_amd import _lib
    for P in (1, 3, 255, 4096, 4097, 8198, 1 << 20, (1 << 20) + 1, 1 << 24):
        nb, n_t, rows = D.distill_launch(P)
        assert _lib.query("segk_loss_part_floats", P) >= 4 * nb          # four words per partial row
        assert nb <= 256 and nb * 1024 * n_t >= P and rows == 16
    assert _lib.query("segk_loss_state_floats") >= 4
    assert D.pixels_in_flight(3) == 4 and D.pixels_in_flight(5) == 2 and D.pixels_in_flight(8, False) == 1


def test_descriptor_layout_matches_the_header():
    from image_segmentation_amd import distill
    txt = open(os.path.join(ROOT, "include", "segk.h")).read()
    body = re.search(r"typedef struct segk_teacher_desc \{(.*?)\} segk_teacher_desc;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(.+)", decl.strip())
        if m:
            for name in m.group(2).split(","):
                arr = re.match(r"\s*(\w+)\[(\d+)\]", name)
                fields.append((arr.group(1), m.group(1), int(arr.group(2))) if arr else (name.strip(), m.group(1), 1))
    ctype = {"uint64_t": "<u8", "int32_t": "<i4", "float": "<f4"}
    want = [(n, ctype[t]) if k == 1 else (n, ctype[t], (k,)) for n, t, k in fields]
    assert np.dtype(want) == distill.TEACHER_DESC and distill.TEACHER_DESC.itemsize == 32
    t = distill.teacher_table([(256, "h", "probs", 1.0), (512, 2, 0, 3.0)])
    assert list(t["flip"]) == [1, 2] and list(t["kind"]) == [1, 0] and list(t["weight"]) == [np.float32(0.25), np.float32(0.75)]
    for bad in ([(0, 0, 0, 1.0)], [(258, 0, 0, 1.0)], [(256, 4, 0, 1.0)], [(256, 0, 2, 1.0)], [(256, 0, 0, 0.0)], [],
                [(256, 0, 0, 1.0)] * 17):
        with pytest.raises(ValueError):
            distill.teacher_table(bad)


def test_argument_errors():
    import image_segmentation_amd as seg
    s = torch.zeros(2, 3, 4, 4, requires_grad=True)
    t = torch.zeros(2, 3, 4, 4)
    loss = seg.DistillLoss(alpha=1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss(s, None, t)
    with pytest.raises(RuntimeError, match="up to 8 classes"):
        loss(torch.zeros(1, 9, 4, 4), None, torch.zeros(1, 9, 4, 4))
    with pytest.raises(ValueError, match="1..16"):
        loss(s, None, [t] * 17)
    with pytest.raises(ValueError, match="class count and resolution"):
        loss(s, None, torch.zeros(2, 4, 4, 4))
    with pytest.raises(ValueError, match="class count and resolution"):
        loss(s, None, torch.zeros(2, 3, 4, 8))
    with pytest.raises(ValueError):
        loss(s, None, [t, torch.zeros(2, 3, 8, 4)])
    with pytest.raises(ValueError, match="alpha must be 1"):
        seg.DistillLoss(hard=seg.CrossEntropyLoss(), alpha=0.5)(s, None, t)
    with pytest.raises(ValueError, match="alpha must be 1"):
        seg.DistillLoss(hard=None, alpha=0.5)(s, torch.zeros(2, 4, 4, dtype=torch.long), t)
    for kw in (dict(alpha=1.5), dict(temperature=0.0), dict(temperature=float("inf")), dict(min_confidence=float("nan"))):
        with pytest.raises(ValueError):
            seg.DistillLoss(**kw)
    with pytest.raises(ValueError, match="more than one input"):
        seg.Teacher(seg.PromptModel.__new__(seg.PromptModel))
    with pytest.raises(ValueError):
        seg.Teacher(torch.nn.Identity(), flips=("h", "h"))
    with pytest.raises(ValueError):
        seg.Teacher([torch.nn.Identity()] * 5, flips=("", "h", "v", "hv"))
    with pytest.raises(ValueError):
        seg.Teacher(torch.nn.Identity(), flips=("", "h"), weights=(1.0,))


def test_teacher_freezes_flips_and_restores_modes():
    """host only: a stand-in network on CPU tensors (Teacher itself launches nothing)"""
    import image_segmentation_amd as seg
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 1), torch.nn.BatchNorm2d(3))
    net.train()
    net[1].eval()                                     # a mixed-mode model: every module gets its own mode back
    X = torch.arange(2 * 2 * 3 * 5, dtype=torch.float32).reshape(2, 2, 3, 5) / 7
    teacher = seg.Teacher(net, flips=("", "h", "v", "hv"), weights=(1, 2, 3, 2))
    before = {k: v.clone() for k, v in net.state_dict().items()}
    views = teacher(X)
    assert net.training and net[0].training and not net[1].training
    assert all(not p.requires_grad for p in net.parameters())
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert views.flips == (0, 1, 2, 3) and views.kinds == (0, 0, 0, 0) and len(views) == 4
    assert views.weights == (0.125, 0.25, 0.375, 0.25)
    net.eval()
    with torch.no_grad():
        base = net(X)
    for out, fl in zip(views.outputs, views.flips):    # a 1x1 network commutes with flips: the view, read through its flip, is base
        assert not out.requires_grad and out.dtype == torch.float32 and out.is_contiguous()
        assert torch.equal(D.unflip(out, fl), base)
    assert [int(a) for a in views.host_table["ptr"]] == [o.data_ptr() for o in views.outputs]


def test_kernels_do_not_spill_and_keep_their_loads_in_flight():
    import importlib.util

    def tool(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        return m
    rows = tool("spill_report").report("distill")
    assert len(rows) == 40, len(rows)                  # forward and backward x 5 class counts x temperature x labels
    for r in rows:
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
    for n_ser, n_loads, _, name in tool("serialized_loads").scan("distill"):
        assert n_ser <= 2, f"{name}: {n_ser} of {n_loads} loads wait for themselves"


def test_entries_validate_before_any_launch():
    """every scalar and host-visible pointer: -2 with a message, nothing launched (there is no GPU here to launch on)"""
    from image_segmentation_amd import _lib
    lib = _lib.load()
    f, P = ctypes.c_float, 256

    def fwd(student=P, table=P, V=1, labels=0, N=1, C=3, H=4, W=4, ign=0, invT=1.0, Tsq=1.0, mc=0.0, part=P, state=P, out=0):
        return lib.segk_distill_fwd(student, table, V, labels, N, C, H, W, ign, f(invT), f(Tsq), f(mc), part, state, out, None)

    def bwd(student=P, table=P, V=1, labels=0, state=P, gout=P, N=1, C=3, H=4, W=4, ign=0, invT=1.0, Tsq=1.0, mc=0.0, ds=P):
        return lib.segk_distill_bwd(student, table, V, labels, state, gout, N, C, H, W, ign, f(invT), f(Tsq), f(mc), ds, None)

    bad = [dict(student=0), dict(table=0), dict(table=264), dict(V=0), dict(V=17), dict(C=0), dict(C=9), dict(N=0), dict(H=0),
           dict(W=-1), dict(N=1 << 11, H=1 << 10, W=1 << 10), dict(invT=0.0), dict(invT=float("inf")), dict(invT=float("nan")),
           dict(Tsq=-1.0), dict(Tsq=float("nan")), dict(mc=float("nan")), dict(mc=float("inf")), dict(labels=4)]
    for kw in bad + [dict(part=0), dict(state=0), dict(part=2), dict(out=2)]:
        assert fwd(**kw) == -2 and lib.segk_last_error(), kw
    for kw in bad + [dict(state=0), dict(gout=0), dict(ds=0), dict(ds=2)]:
        assert bwd(**kw) == -2 and lib.segk_last_error(), kw
