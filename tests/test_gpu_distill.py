"""GPU (-m gpu): the distillation kernels of csrc/distill.hip through the C ABI against float64 (tests/distill_reference.py), then
the module and the training loop.

Kernel matrix (distill_fwd_kernel: blocks = ceil(P / 4096) capped at 256, 1024 threads, four pixels in flight per thread up to
four classes and two above; distill_bwd_kernel: 256-thread blocks, two pixels / one): C = 1..8 (compiled for 1, 2, 3, 4 and 8: 5, 6
and 7 run the clamped-class loads) at 1, 3, 255, 257, 1023 and 4097 pixels (4097: two blocks, remainder loop only) and at two
images of 5 x 7 and of 4099 pixels (the image boundary inside a block, both flip axes at odd sizes).  View count 1..3, flips 0..3,
both kinds, unequal weights, T 0.5 / 1 / 2, labels absent / partly ignored, the confidence gate and the upstream gradient walk
through the cells with strides of their own (distill_reference.case); the semantic edges (every label ignored, a gate nothing
passes, +-80, all-equal logits, exact zeros in a probability teacher) are cases of their own.  Outputs and partial buffers are
NaN-filled with guard elements behind them.

Tolerances: derived or measured in tests/distill_reference.py, none tuned to what the kernels return."""
import numpy as np
import pytest
import torch

import distill_reference as D
import loss_reference as L

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = list(D.all_cases())


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def nans(n):
    return torch.full((n,), NAN, dtype=torch.float32, device="cuda")


def run_distill(lib, s, ts, kw, gout):
    """-> state [28], loss_out, gradient [N, C, H, W], all on the CPU"""
    from image_segmentation_amd import distill
    N, C, H, W = s.shape
    P = N * H * W
    sd = s.cuda().contiguous()
    td = [t.cuda().contiguous() for t in ts]
    host = distill.teacher_table((t.data_ptr(), f, k, w) for t, f, k, w in zip(td, kw["flips"], kw["kinds"], kw["weights"]))
    table = torch.from_numpy(host.view(np.uint8).copy()).cuda()
    y, ign = kw.get("y"), kw.get("ignore_index")
    yd = y.cuda().contiguous() if y is not None and ign is not None else None
    T = float(kw.get("T", 1.0))
    scal = (0 if ign is None else int(ign), 1.0 / T, T * T, float(kw.get("min_conf", 0.0)))
    nb = D.distill_launch(P)[0]
    nf = lib.query("segk_loss_part_floats", P)
    part, state, out = nans(nf + 8), nans(28 + 4), nans(1 + 3)
    lib.call("segk_distill_fwd", sd.data_ptr(), table.data_ptr(), len(td), None if yd is None else yd.data_ptr(), N, C, H, W, *scal,
             part.data_ptr(), state.data_ptr(), out.data_ptr(), _stream())
    go = torch.tensor([gout], dtype=torch.float32, device="cuda")
    ds = nans(P * C + 5)
    lib.call("segk_distill_bwd", sd.data_ptr(), table.data_ptr(), len(td), None if yd is None else yd.data_ptr(), state.data_ptr(),
             go.data_ptr(), N, C, H, W, *scal, ds.data_ptr(), _stream())
    torch.cuda.synchronize()
    part, state, out, ds = part.cpu(), state.cpu(), out.cpu(), ds.cpu()
    assert not torch.isnan(part[:4 * nb].view(-1, 4)[:, 0]).any(), "a partial row was not written"
    assert torch.isnan(part[nf:]).all() and torch.isnan(state[28:]).all() and torch.isnan(out[1:]).all(), "wrote past a buffer"
    assert torch.isnan(ds[P * C:]).all(), "the gradient kernel wrote past its buffer"
    return state[:28], out[0], ds[:P * C].view(N, C, H, W)


def check(lib, s, ts, kw, gout, desc):
    r = D.run_reference(s, ts, kw)
    gr = D.distill_grad_reference(r, gout)
    e_soft, e_sum = D.state_bound(r)
    gb = D.grad_bound(r, gr)
    state, out, ds = run_distill(lib, s, ts, kw, gout)
    st = state.double()
    und = int((D.undecided(r) & r["counted"]).sum())
    lo = int((r["agree"] & ~D.undecided(r)).sum())
    gerr = (ds.double() - gr["grad"]).abs()
    print(f"{desc}\n  soft {st[0]:.9g} ref {float(r['soft']):.9g} err {abs(st[0] - r['soft']):.3g} bound {e_soft:.3g} | sumKL err "
          f"{abs(st[2] - r['sum_kl']):.3g} bound {e_sum:.3g} | n {int(st[1])} ref {r['n']} | n_agree {int(st[3])} in [{lo}, {lo + und}] | "
          f"grad worst err/bound {float((gerr / gb.clamp(min=1e-300)).max()):.3g}")
    assert int(st[1]) == r["n"] and st[1] == float(r["n"]), desc
    assert out.item() == state[0].item(), desc
    assert torch.isfinite(state).all() and not state[4:].any(), desc
    assert abs(st[0] - r["soft"]) <= e_soft, desc
    assert abs(st[2] - r["sum_kl"]) <= e_sum, desc
    assert lo <= int(st[3]) <= lo + und and und <= 0.01 * r["n"], desc
    assert bool((gerr <= gb).all()), desc
    assert not ds[~r["counted"].unsqueeze(1).expand_as(ds)].any(), "an uncounted pixel got a gradient: " + desc
    if r["n"] == 0:
        assert st[0] == 0 and st[2] == 0 and st[3] == 0 and not ds.any(), desc
        assert not torch.signbit(state[0]), desc
    return r, state, ds


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: f"case{i}")
def test_kernels_against_float64(lib, idx):
    desc, s, ts, kw, gout = CASES[idx]
    check(lib, s, ts, kw, gout, desc)


@pytest.mark.parametrize("idx", [5, 14, 23, 39, 46, 63, 66, 71])
def test_two_runs_give_equal_bits(lib, idx):
    desc, s, ts, kw, gout = CASES[idx]
    a, b = run_distill(lib, s, ts, kw, gout), run_distill(lib, s, ts, kw, gout)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), desc
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)), desc


@pytest.mark.parametrize("si", [6, 7])
@pytest.mark.parametrize("flip", [1, 2, 3])
def test_flipped_teacher_with_its_flag_equals_the_unflipped_one(lib, si, flip):
    """both odd-sized shapes; the flipped view is the second of two, with labels and a temperature in play"""
    N, H, W = D.SHAPES[si]
    s, ts, y = D.inputs(4, N, H, W, 2, [0, 1], 7700 + si)
    kw = dict(kinds=[0, 1], weights=[1.0, 2.5], y=y, ignore_index=2, T=2.0, min_conf=0.3)
    a = run_distill(lib, s, ts, dict(kw, flips=[0, 0]), 0.5)
    b = run_distill(lib, s, [ts[0], D.unflip(ts[1], flip).contiguous()], dict(kw, flips=[0, flip]), 0.5)
    assert a[0][1] > 0
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_one_hot_teacher_equals_the_cross_entropy_kernel(lib, C):
    """a one-hot probability teacher at T = 1: KL = -log p_y, so soft is segk_loss_fwd's unweighted ce, within both bounds"""
    x, y = L.loss_inputs(C, 2, 4099, 91 + C)                   # [N, C, HW]
    N, _, HW = x.shape
    hot = torch.nn.functional.one_hot(y, C).permute(0, 2, 1).float().reshape(N, C, 1, HW).contiguous()
    s = x.reshape(N, C, 1, HW)
    kw = dict(flips=[0], kinds=[1], weights=[1.0])
    r = D.run_reference(s, [hot], kw)
    state, _, _ = run_distill(lib, s, [hot], kw, 1.0)
    lr = L.loss_reference(x, y, smooth=0.0, dice_weight=0.0, ce_weight=1.0)
    xd, yd = x.cuda(), y.cuda()
    part, lstate = nans(lib.query("segk_loss_part_floats", N * HW)), nans(28)
    lib.call("segk_loss_fwd", xd.data_ptr(), yd.data_ptr(), None, N, C, HW, -1, 0.0, 0.0, 1.0, part.data_ptr(), lstate.data_ptr(),
             None, _stream())
    torch.cuda.synchronize()
    bound = D.state_bound(r)[0] + float(L.state_bound(lr)[0][1])
    # the two float64 references differ by the off-label mass of the teacher: at most (C - 1) 2^-126 (1 + |log 2^-126 - log p|)
    print(f"C={C} soft {state[0].item():.9g} ce {lstate[1].item():.9g} bound {bound:.3g}")
    assert abs(float(r["soft"]) - float(lr["ce"])) <= 1e-13 * float(lr["ce"])      # (float64 sums in another order)
    assert abs(state[0].double().item() - lstate[1].double().item()) <= bound


# ------------------------------------------------------------------------------------------------ module and loop
def _models(n_teachers):
    import image_segmentation_amd as seg
    torch.manual_seed(11)
    student = seg.unet(3, 3).cuda()
    teachers = []
    for i in range(n_teachers):
        torch.manual_seed(20 + i)
        teachers.append(seg.unet(3, 3).cuda())
    return student, teachers


def _batch(seed, labels=True):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand((2, 3, 32, 32), generator=g)
    y = torch.randint(0, 3, (2, 1, 32, 32), generator=g)
    return (X, y) if labels else (X, None)


def test_module_matches_float64_on_the_captured_logits(lib):
    import image_segmentation_amd as seg
    student, teachers = _models(2)
    teacher = seg.Teacher(teachers, flips=("", "h"), weights=(2, 1, 1, 1))
    X, y = _batch(5)
    y = y.clone()
    y.view(-1)[::5] = 255
    X, y = X.cuda(), y.cuda()
    student.train()
    views = teacher(X)
    assert len(views) == 4 and views.flips == (0, 1, 0, 1) and all(not o.requires_grad for o in views.outputs)
    pred = student(X)
    pred.retain_grad()
    loss_fn = seg.DistillLoss(alpha=1.0, temperature=2.0, ignore_index=255, min_confidence=0.34)
    loss = loss_fn(pred, y, views)
    (loss * 0.5).backward()
    last = loss_fn.last
    assert all(last[k].is_cuda for k in ("soft", "n", "n_agree")) and last["hard"] is None
    r = D.distill_reference(pred.detach().float().cpu(), [o.cpu() for o in views.outputs], list(views.flips), list(views.kinds),
                            [2, 1, 1, 1], y=y.cpu()[:, 0], ignore_index=255, T=2.0, min_conf=0.34)
    assert not D.gate_undecided(r).any()
    gr = D.distill_grad_reference(r, 0.5)
    e_soft, _ = D.state_bound(r)
    print(f"soft {loss.item():.9g} ref {float(r['soft']):.9g} bound {e_soft:.3g} n {int(last['n'])} agree {int(last['n_agree'])}")
    assert 0 < r["n"] < 2 * 32 * 32 and int(last["n"].item()) == r["n"]
    assert abs(loss.double().item() - float(r["soft"])) <= e_soft and loss.item() == last["soft"].item()
    assert bool(((pred.grad.double().cpu() - gr["grad"]).abs() <= D.grad_bound(r, gr)).all())
    und = D.undecided(r) & r["counted"]
    lo = int((r["agree"] & ~und).sum())
    assert lo <= int(last["n_agree"].item()) <= lo + int(und.sum())
    # a plain tensor is a logit teacher without a flip; with a hard loss the sum is formed from the two terms it reports
    mixed = seg.DistillLoss(hard=seg.CrossEntropyLoss(), alpha=0.7, temperature=2.0)
    val = mixed(pred.detach(), y, views.outputs[0])
    exp = 0.7 * mixed.last["soft"] + (1.0 - 0.7) * mixed.last["hard"]
    assert val.item() == exp.item() and mixed.last["hard"].item() == seg.CrossEntropyLoss()(pred.detach(), y[:, 0]).item()


def _snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_loop_trains_the_student_and_leaves_the_teachers_alone(lib, monkeypatch):
    import image_segmentation_amd as seg
    from image_segmentation_amd import training
    monkeypatch.setattr(training, "VERBOSE", False)
    student, teachers = _models(2)
    teachers[0].train()
    teachers[1].eval()
    teacher = seg.Teacher(teachers, flips=("", "v"))
    before = [_snapshot(t) for t in teachers]
    s0 = _snapshot(student)
    loss_fn = seg.DistillLoss(hard=seg.CrossEntropyLoss(), alpha=0.5, temperature=2.0)
    opt = torch.optim.AdamW(student.parameters(), lr=1e-3)
    avg = seg.train_loop_distill([_batch(1), _batch(2)], student, teacher, loss_fn, opt, 1, "cuda")
    assert np.isfinite(avg) and avg > 0
    for t, b in zip(teachers, before):
        after = t.state_dict()
        assert set(after) == set(b) and all(torch.equal(after[k], b[k]) for k in b)
        assert all(not p.requires_grad and p.grad is None for p in t.parameters())
    assert teachers[0].training and all(m.training for m in teachers[0].modules())
    assert not teachers[1].training and not any(m.training for m in teachers[1].modules())
    assert any(not torch.equal(v, s0[k]) for k, v in student.state_dict().items() if v.dtype.is_floating_point)


def test_alpha_zero_is_train_loop_bit_for_bit(lib, monkeypatch):
    import image_segmentation_amd as seg
    from image_segmentation_amd import training
    monkeypatch.setattr(training, "VERBOSE", False)
    batches = [_batch(1), _batch(2), _batch(3)]
    hard = seg.CrossEntropyLoss()
    a, teachers = _models(1)
    opt = torch.optim.AdamW(a.parameters(), lr=1e-3)
    va = training.train_loop(batches, a, hard, opt, 2, "cuda")
    b, _ = _models(0)
    opt = torch.optim.AdamW(b.parameters(), lr=1e-3)
    vb = seg.train_loop_distill(batches, b, seg.Teacher(teachers), seg.DistillLoss(hard=hard, alpha=0.0), opt, 2, "cuda")
    assert va == vb
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_unlabelled_batches_train_with_alpha_one(lib, monkeypatch):
    import image_segmentation_amd as seg
    from image_segmentation_amd import training
    monkeypatch.setattr(training, "VERBOSE", False)
    student, teachers = _models(1)
    s0 = _snapshot(student)
    opt = torch.optim.AdamW(student.parameters(), lr=1e-3)
    loss_fn = seg.DistillLoss(alpha=1.0, temperature=2.0)
    avg = seg.train_loop_distill([_batch(1, labels=False), _batch(2, labels=False)[0]], student, seg.Teacher(teachers, flips=("h",)),
                                 loss_fn, opt, 1, "cuda")
    assert np.isfinite(avg) and avg > 0 and int(loss_fn.last["n"].item()) == 2 * 32 * 32
    assert any(not torch.equal(v, s0[k]) for k, v in student.state_dict().items() if v.dtype.is_floating_point)
    with pytest.raises(ValueError, match="alpha must be 1"):
        seg.train_loop_distill([_batch(1, labels=False)], student, seg.Teacher(teachers), seg.DistillLoss(hard=seg.CrossEntropyLoss()),
                               opt, 1, "cuda")
