"""GPU (-m gpu): the two ends of the full-resolution level without a stored gradient (BatchNorm backward).

  head end  segk_head_bwd_bn_stats + segk_head_bn_bwd_apply   against   segk_head_bwd_bn + segk_bn_relu_bwd_from_part
  stem end  segk_bn_relu_bwd_stats + segk_stem3x3_wgrad_bn     against   segk_bn_relu_bwd + segk_stem3x3_wgrad

In every case the reference is the stored-gradient sequence, called through the same C ABI on the same seeded inputs, and the
comparison is torch.equal: the re-formed gradient is rounded to bf16 exactly where the stored one was, the per-element formula
is one shared device function, and every sum keeps its order.  tests/test_gpu_head_loss_matrix.py,
tests/test_gpu_bn_backward_matrix.py and tests/test_gpu_stem_pool_matrix.py pin the stored-gradient kernels to float64;
equality carries those pins over.  Inputs contain ReLU-dead pixels, one channel with scale == 0 and one with scale < 0.

The module cases run one unet(3, 3) training step at B = 2, 32 x 32 with both values of ops.END_FUSION_MIN_BYTES at 0 and at infinity, and the
trace cases check which entries a step launches at the default value (none of the new ones: the gradient tensors of that
shape are 256 KB, the launch sequence tests/test_gpu_training_trace.py records) and at 0 (each new entry exactly once)."""
import pytest
import torch

from oracle.fill import fill, labels, fill_module

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NEW = ("segk_head_bwd_bn_stats", "segk_head_bn_bwd_apply", "segk_bn_relu_bwd_stats", "segk_stem3x3_wgrad_bn")


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import image_segmentation_amd as s
    from image_segmentation_amd import _lib
    _lib.load()
    s.set_compute_dtype(BF16)
    yield s
    s.set_compute_dtype(BF16)


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


def bn_vectors(Cp, C, seed):
    """scale, shift, mean, rstd [Cp] as segk_bn_finalize leaves them (padded channels all zero), with scale[1] == 0 and
    scale[2] < 0; the shifts put a good part of every channel below the ReLU."""
    scale, shift = fill((Cp,), seed, 0.5, 1.5), fill((Cp,), seed + 1, -0.6, 0.6)
    mean, rstd = fill((Cp,), seed + 2, -0.3, 0.3), fill((Cp,), seed + 3, 0.7, 1.9)
    scale[1], scale[2] = 0.0, -0.8
    for v in (scale, shift, mean, rstd):
        v[C:] = 0.0
    return [v.cuda() for v in (scale, shift, mean, rstd)]


def assert_relu_mixed(z, scale, shift, C):
    act = (z.float() * scale + shift)[..., :C] > 0
    frac = act.float().mean().item()
    assert 0.1 < frac < 0.9, frac                      # ReLU-dead and live pixels both present


# ---------------------------------------------------------------------------------------------------------------------
HEAD_CASES = [(Cp, C, ncls, H, W) for (Cp, C, ncls) in ((64, 64, 3), (32, 32, 4), (64, 40, 1)) for (H, W) in ((13, 21), (96, 96))]
# one more shape: 4.5 times the pixels one pass of the apply grid covers (4096 blocks x 16 pixel rows), so its threads walk
# four or five pixels each (at 96 x 96 the grid is smaller than its cap and every thread has one)
HEAD_CASES.append((64, 64, 3, 384, 384))


@pytest.mark.parametrize("Cp,C,ncls,H,W", HEAD_CASES)
def test_head_end_without_stored_gradient(seg, Cp, C, ncls, H, W):
    from image_segmentation_amd import _lib
    B, P = 2, 2 * H * W
    z = fill((B, H, W, Cp), 11, -2, 2).to(BF16).cuda()
    z[..., C:] = 0
    dl = (fill((B, ncls, H, W), 12, -1, 1) / P).cuda()
    w = fill((ncls, C), 13, -0.5, 0.5).cuda()
    bn = bn_vectors(Cp, C, 20)
    assert_relu_mixed(z, bn[0], bn[1], C)
    bnp = [v.data_ptr() for v in bn]
    nb = _lib.query("segk_head_bwd_blocks", P)
    nparts = _lib.query("segk_head_part_floats", P, Cp)
    s = stream()

    def run(stored):
        part, dw, db = f32(nparts), f32(ncls * C), f32(ncls)
        bnpart, coef, dgamma, dbeta = f32(nb * Cp * 2), f32(2 * Cp), f32(C), f32(C)
        dz = torch.full((B, H, W, Cp), float("nan"), dtype=BF16, device="cuda")
        if stored:
            dy = torch.full((B, H, W, Cp), float("nan"), dtype=BF16, device="cuda")
            _lib.call("segk_head_bwd_bn", dl.data_ptr(), z.data_ptr(), w.data_ptr(), dy.data_ptr(), part.data_ptr(), dw.data_ptr(),
                      db.data_ptr(), B, H, W, Cp, C, ncls, *bnp, bnpart.data_ptr(), 1, s)
            _lib.call("segk_bn_relu_bwd_from_part", dy.data_ptr(), z.data_ptr(), dz.data_ptr(), *bnp, P, Cp, C, bnpart.data_ptr(), nb,
                      dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), 1, s)
        else:
            _lib.call("segk_head_bwd_bn_stats", dl.data_ptr(), z.data_ptr(), w.data_ptr(), part.data_ptr(), dw.data_ptr(),
                      db.data_ptr(), B, H, W, Cp, C, ncls, *bnp, bnpart.data_ptr(), 1, s)
            _lib.call("segk_head_bn_bwd_apply", dl.data_ptr(), z.data_ptr(), w.data_ptr(), dz.data_ptr(), *bnp, B, H, W, Cp, C, ncls,
                      bnpart.data_ptr(), nb, dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), 1, s)
        torch.cuda.synchronize()
        return {"dz": dz, "dgamma": dgamma, "dbeta": dbeta, "dW_head": dw, "db_head": db, "bnpart": bnpart, "coef": coef}

    ref, got = run(True), run(False)
    assert torch.isfinite(ref["dz"].float()).all() and ref["dz"].float().abs().max() > 0
    for k in ref:
        assert torch.equal(ref[k], got[k]), f"{k} differs ({Cp}, {C}, {ncls}) {B}x{H}x{W}"


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,H,W", [(2, 3, 5, 16), (1, 1, 9, 48), (2, 3, 64, 640)])
def test_stem_end_without_stored_gradient(seg, B, Cin, H, W):
    from image_segmentation_amd import _lib
    P, C = B * H * W, 64
    x = fill((B, Cin, H, W), 31, -1, 1).cuda()
    z = fill((B, H, W, C), 32, -2, 2).to(BF16).cuda()
    da = fill((B, H, W, C), 33, -1, 1).to(BF16).cuda()
    bn = bn_vectors(C, C, 40)
    assert_relu_mixed(z, bn[0], bn[1], C)
    bnp = [v.data_ptr() for v in bn]
    S = _lib.query("segk_stem3x3_wgrad_slabs", B, H, W, Cin, C, 1)
    assert S > 0
    if (H, W) == (64, 640):
        assert B * H * (W // 16) > 2 * torch.cuda.get_device_properties(0).multi_processor_count * 8    # waves loop
    nb = _lib.query("segk_bn_bwd_blocks", P, C, 1)
    s = stream()

    def run(stored):
        part, coef, dgamma, dbeta = f32(nb * C * 2), f32(2 * C), f32(C), f32(C)
        slabs, grad = f32(S * 64 * 32), f32(64 * Cin * 9)
        if stored:
            dz = da.clone()                                    # in place, as DoubleConvFn._backward runs it
            _lib.call("segk_bn_relu_bwd", dz.data_ptr(), z.data_ptr(), dz.data_ptr(), *bnp, P, C, C, part.data_ptr(), dgamma.data_ptr(),
                      dbeta.data_ptr(), coef.data_ptr(), 1, s)
            _lib.call("segk_stem3x3_wgrad", x.data_ptr(), dz.data_ptr(), slabs.data_ptr(), B, H, W, Cin, C, 1, s)
        else:
            _lib.call("segk_bn_relu_bwd_stats", da.data_ptr(), z.data_ptr(), *bnp, P, C, C, part.data_ptr(), dgamma.data_ptr(),
                      dbeta.data_ptr(), coef.data_ptr(), 1, s)
            _lib.call("segk_stem3x3_wgrad_bn", x.data_ptr(), da.data_ptr(), z.data_ptr(), *bnp, coef.data_ptr(), slabs.data_ptr(),
                      B, H, W, Cin, C, 1, s)
        _lib.call("segk_wgrad_reduce", slabs.data_ptr(), S, grad.data_ptr(), 64, 9 * Cin, 0, 64, 32, 0, 1, s)
        torch.cuda.synchronize()
        return {"dW": grad, "slabs": slabs, "dgamma": dgamma, "dbeta": dbeta, "coef": coef}

    ref, got = run(True), run(False)
    assert torch.isfinite(ref["dW"]).all() and ref["dW"].abs().max() > 0
    for k in ref:
        assert torch.equal(ref[k], got[k]), f"{k} differs {B}x{Cin}x{H}x{W}"


# ---------------------------------------------------------------------------------------------------------------------
def step(seg, monkeypatch, min_bytes, x_grad=False, train=True, calls=None):
    """One forward + backward of a freshly filled unet(3, 3) at B = 2, 32 x 32 -> (loss, parameter gradients, dx)."""
    from image_segmentation_amd import _lib, ops
    if min_bytes is not None:
        monkeypatch.setattr(ops, "END_FUSION_MIN_BYTES", {"head": min_bytes, "stem": min_bytes})
    seg.set_compute_dtype(BF16)
    ops.invalidate_packed_weights()
    m = seg.unet(3, 3)
    fill_module(m, 1000)
    m = m.cuda()
    m.train() if train else m.eval()
    X = fill((2, 3, 32, 32), 10, 0, 1).cuda()
    y = labels((2, 1, 32, 32), 20, 3).cuda()
    if x_grad:
        X.requires_grad_(True)
    real = _lib.call
    if calls is not None:
        def call(name, *args):
            calls.append(name)
            return real(name, *args)
        monkeypatch.setattr(_lib, "call", call)
    loss = seg.CrossEntropyLoss()(m(X), y)
    loss.backward()
    torch.cuda.synchronize()
    if calls is not None:
        monkeypatch.setattr(_lib, "call", real)
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    return loss.detach().clone(), grads, (X.grad.clone() if x_grad else None)


@pytest.mark.parametrize("mode", ["train", "input_grad", "eval"])
def test_module_step_is_bit_identical(seg, monkeypatch, mode):
    x_grad, train = mode == "input_grad", mode != "eval"
    calls = []
    l1, g1, dx1 = step(seg, monkeypatch, 0, x_grad, train, calls)
    l0, g0, dx0 = step(seg, monkeypatch, float("inf"), x_grad, train)
    assert torch.equal(l0, l1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    head = [c for c in calls if c in NEW[:2]]
    stem = [c for c in calls if c in NEW[2:]]
    if mode == "train":
        assert sorted(head) == sorted(NEW[:2]) and sorted(stem) == sorted(NEW[2:])
    elif mode == "input_grad":                      # the stem has a data gradient: dz1 is stored for it
        assert sorted(head) == sorted(NEW[:2]) and stem == []
        assert dx0 is not None and torch.equal(dx0, dx1) and dx0.abs().max() > 0
    else:                                           # BatchNorm on running statistics: both ends as before
        assert head == [] and stem == []


def test_default_threshold_keeps_the_launch_sequence_of_small_shapes(seg, monkeypatch):
    from image_segmentation_amd import ops
    assert min(ops.END_FUSION_MIN_BYTES.values()) > 2 * 32 * 32 * 64 * 2     # the 256 KB gradients of the recorded trace shape stay stored
    calls = []
    step(seg, monkeypatch, None, calls=calls)
    assert len(calls) > 50 and not any(c in NEW for c in calls)
    calls0 = []
    step(seg, monkeypatch, 0, calls=calls0)
    for name in NEW:
        assert calls0.count(name) == 1, name
    # everything else is the same sequence: the four new entries stand where the stored forms stood
    swap = {"segk_head_bwd_bn_stats": "segk_head_bwd_bn", "segk_head_bn_bwd_apply": "segk_bn_relu_bwd_from_part",
            "segk_bn_relu_bwd_stats": "segk_bn_relu_bwd", "segk_stem3x3_wgrad_bn": "segk_stem3x3_wgrad"}
    assert [swap.get(c, c) for c in calls0] == calls
