"""GPU (-m gpu): reconstruction pretraining on the HIP kernels (reference autoencoder/autoencoder.py:188-191 head,
nn.MSELoss, utils/training.py:123-151 trainReconstruction and :202-239 evalReconstruction).

  * the fused 3x3 + Sigmoid head and its backward against a float64 evaluation of the operands the kernel consumes;
  * MSELoss against F.mse_loss, deterministic to the bit;
  * trainReconstruction against the reference golden, evalReconstruction against its CPU host path, and the hand-off of a
    pretrained encoder to SegmentationAutoencoder(pretrained_encoder_path=...);
  * compiled-code checks of the new unit (no spills, loads kept in flight)."""
import io
import contextlib
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recon_reference as R
from oracle.fill import fill, fill_module

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import image_segmentation_amd as s
    yield s
    s.set_compute_dtype(torch.bfloat16)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _head_case(seg, dtype, B, H, W, Cin, Cout, seed, wscale=None, bias=None):
    from image_segmentation_amd import ops
    from image_segmentation_amd.unet import _FusedBase
    mod = _FusedBase()
    mod.compute_dtype = dtype
    x = fill((B, Cin, H, W), seed, 0, 1)
    w = fill((Cout, Cin, 3, 3), seed + 1, -1, 1) * (wscale if wscale is not None else 1.0 / (3.0 * Cin ** 0.5))
    b = fill((Cout,), seed + 2, -0.5, 0.5) if bias is None else bias
    xa = ops.to_act(x.cuda(), dtype).detach().requires_grad_()
    wp = torch.nn.Parameter(w.clone().cuda())
    bp = torch.nn.Parameter(b.clone().cuda())
    rec = ops.ReconHeadFn.apply(mod, xa, wp, bp)
    return mod, xa, wp, bp, rec


SHAPES = [(1, 7, 13), (2, 32, 48), (3, 37, 61)]


def assert_head_forward(rec, xa, wp, bp, dtype, Cin):
    """per output within the derived gate of tests/recon_reference.py (gamma_m S / 4 + 4 d_sig on the operands the kernel
    consumes) and, where that is looser, within the flat 1e-5 this test has always held"""
    rec64, S, z = R.head(xa.detach().float().cpu().permute(0, 2, 3, 1), wp.detach().cpu(), bp.detach().cpu(), dtype)
    gate = torch.clamp(R.head_bound(S, z, Cin), max=1e-5)
    err = (rec.detach().cpu().double() - rec64).abs()
    print(f"head forward {dtype} Cin={Cin}: max err {err.max().item():.3e}, max err / gate {(err / gate).max().item():.4f}")
    assert bool(torch.isfinite(rec).all()) and bool((err <= gate).all()), float((err / gate).max())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("Cin", [32, 64, 96])
@pytest.mark.parametrize("Cout", [1, 3, 4, 11])
def test_head_fp32_forward_backward_vs_float64(seg, shape, Cin, Cout):
    B, H, W = shape
    _, xa, wp, bp, rec = _head_case(seg, torch.float32, B, H, W, Cin, Cout, 100 + Cin + Cout)
    assert rec.dtype == torch.float32 and rec.is_contiguous() and rec.shape == (B, Cout, H, W)
    drec = fill((B, Cout, H, W), 7, -1, 1)
    rec.backward(drec.cuda())
    torch.cuda.synchronize()
    x64 = xa.detach().float().cpu().double().requires_grad_()
    w64 = wp.detach().cpu().double().requires_grad_()
    b64 = bp.detach().cpu().double().requires_grad_()
    r64 = torch.sigmoid(F.conv2d(x64, w64, b64, padding=1))
    r64.backward(drec.double())
    assert (rec.detach().cpu().double() - r64.detach()).abs().max().item() < 1e-5
    assert_head_forward(rec, xa, wp, bp, "fp32", Cin)
    for mine, ref in ((xa.grad, x64.grad), (wp.grad, w64.grad), (bp.grad, b64.grad)):
        err = (mine.detach().float().cpu().double() - ref).abs().max().item()
        assert err <= 1e-4 * ref.abs().max().item() + 1e-12, (err, ref.abs().max().item())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("Cin", [32, 64, 96])
@pytest.mark.parametrize("Cout", [1, 3, 4, 11])
def test_head_bf16_forward_vs_float64_on_rounded_operands(seg, shape, Cin, Cout):
    """bf16 mode multiplies the bf16 act tensor by the bf16-rounded weights with fp32 accumulation: against float64 on
    exactly those operands, so the check pins the kernel's arithmetic, not the rounding of its inputs."""
    B, H, W = shape
    _, xa, wp, bp, rec = _head_case(seg, torch.bfloat16, B, H, W, Cin, Cout, 200 + Cin + Cout)
    torch.cuda.synchronize()
    x64 = xa.detach().float().cpu().double()
    w64 = wp.detach().cpu().bfloat16().double()
    r64 = torch.sigmoid(F.conv2d(x64, w64, bp.detach().cpu().double(), padding=1))
    assert (rec.detach().cpu().double() - r64).abs().max().item() < 1e-5
    assert_head_forward(rec, xa, wp, bp, "bf16", Cin)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_head_saturation_and_dz_padding(seg, dtype):
    from image_segmentation_amd import ops, _lib
    B, H, W, Cin, Cout = 2, 9, 21, 64, 3
    for sign in (1.0, -1.0):
        bias = torch.full((Cout,), 40.0 * sign)
        _, xa, wp, bp, rec = _head_case(seg, dtype, B, H, W, Cin, Cout, 300, wscale=0.0, bias=bias)
        want = torch.sigmoid(torch.full((1,), 40.0 * sign)).item()
        r = rec.detach().cpu()
        assert torch.isfinite(r).all() and (r == want).all(), (sign, r.flatten()[:4], want)
        rec.backward(fill((B, Cout, H, W), 8, -1, 1).cuda())
        for g in (xa.grad, wp.grad, bp.grad):
            g = g.detach().float().cpu()
            assert torch.isfinite(g).all() and g.abs().max().item() < 1e-12
    # the act-layout gradient: padding channels are written as zeros, whatever the buffer held before
    Cp = ops.pad32(Cout)
    drec = fill((B, Cout, H, W), 9, -1, 1).cuda()
    recv = fill((B, Cout, H, W), 10, 0, 1).cuda()
    dz = torch.full((B, H, W, Cp), float("nan"), dtype=dtype, device="cuda")
    _lib.call("segk_recon_sigmoid_bwd", drec.data_ptr(), recv.data_ptr(), dz.data_ptr(), B, H, W, Cout, Cp,
              ops._DT[dtype], ops._stream())
    torch.cuda.synchronize()
    d = dz.float().cpu()
    assert (d[..., Cout:] == 0).all()
    want = (drec * (1 - recv) * recv).permute(0, 2, 3, 1).to(dtype).float().cpu()
    assert torch.equal(d[..., :Cout], want)


@pytest.mark.parametrize("n", [1, 7, 1000, 4097, 65539, 32 * 3 * 256 * 256])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_mse_matches_torch(seg, n, reduction):
    a = fill((n,), 11, 0, 1).cuda().requires_grad_()
    b = fill((n,), 12, 0, 1).cuda()
    loss = seg.MSELoss(reduction=reduction)(a, b)
    again = seg.MSELoss(reduction=reduction)(a, b)
    assert loss.shape == () and loss.dtype == torch.float32
    assert torch.equal(loss.detach(), again.detach())                # deterministic to the bit
    truth = F.mse_loss(a.detach().double(), b.double(), reduction=reduction).item()
    assert abs(loss.item() - truth) <= 1e-6 * abs(truth)
    ref = F.mse_loss(a.detach(), b, reduction=reduction).item()
    assert abs(loss.item() - ref) <= 1e-6 * abs(ref)
    loss.backward(torch.tensor(0.75, device="cuda"))
    a2 = a.detach().clone().requires_grad_()
    F.mse_loss(a2, b, reduction=reduction).backward(torch.tensor(0.75, device="cuda"))
    err = (a.grad - a2.grad).abs().max().item()
    assert err <= 1e-6 * a2.grad.abs().max().item()


def test_mse_contract(seg):
    a = torch.rand(2, 3, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        seg.MSELoss()(a, torch.rand(2, 3, 8, 7, device="cuda"))
    with pytest.raises(RuntimeError):
        seg.MSELoss()(a.cpu(), a.cpu())
    with pytest.raises(NotImplementedError):
        seg.MSELoss(reduction="none")
    with pytest.raises(NotImplementedError):
        seg.MSELoss(size_average=False)
    # non-fp32 / non-contiguous operands are normalised at the edge; the gradient reaches a target that requires one
    x = torch.rand(2, 3, 8, 8, device="cuda", dtype=torch.float64).requires_grad_()
    t = torch.rand(2, 8, 8, 3, device="cuda").permute(0, 3, 1, 2).requires_grad_()
    seg.MSELoss(reduction="sum")(x, t).backward()
    x2, t2 = x.detach().clone().requires_grad_(), t.detach().clone().requires_grad_()
    F.mse_loss(x2.float(), t2, reduction="sum").backward()
    assert x.grad.dtype == torch.float64
    assert torch.allclose(x.grad.float(), x2.grad.float(), rtol=1e-6, atol=0)
    assert torch.allclose(t.grad, t2.grad, rtol=1e-6, atol=0)


def _recording(loss_fn, seen):
    def fn(pred, X):
        out = loss_fn(pred, X)
        seen.append(out.item())
        return out
    return fn


def test_train_reconstruction_golden_fp32(seg, golden):
    from image_segmentation_amd import training
    g = golden("trainrecon_ae_32")
    seg.set_compute_dtype(torch.float32)
    training.VERBOSE = False
    for acc in (1, 2):
        m = seg.ReconstructionAutoencoder(3, 3, base_channels=32); fill_module(m, 4100); m.cuda()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        data = [(fill((2, 3, 32, 32), 40 + i, 0, 1), torch.zeros(2, 1, 32, 32)) for i in range(3)]
        seen = []
        mean = training.trainReconstruction(data, m, _recording(seg.MSELoss(), seen), opt, acc)
        ref = g[f"acc{acc}_losses"]
        assert abs(seen[0] - float(ref[0])) < 1e-6, (seen[0], float(ref[0]))        # before any optimizer step
        assert np.abs(np.array(seen) - ref).max() < 5e-3, (seen, ref)
        assert abs(mean - float(g[f"acc{acc}_mean"])) < 5e-3
        # Adam turns near-zero gradients into lr-sized steps: the bulk agrees closely, single elements within a few lr
        for mine, want in ((m.decoderOut[0].weight, g[f"acc{acc}_out_w"]),
                           (m.encoder.encoderPart1.conv1.weight, g[f"acc{acc}_w0"])):
            d = np.abs(mine.detach().cpu().numpy() - want)
            assert d.max() < 3.5e-3 and np.median(d) < 2e-4, (d.max(), np.median(d))


def test_train_reconstruction_bf16_finite(seg, golden):
    from image_segmentation_amd import training
    g = golden("trainrecon_ae_32")
    seg.set_compute_dtype(torch.bfloat16)
    training.VERBOSE = False
    m = seg.ReconstructionAutoencoder(3, 3, base_channels=32); fill_module(m, 4100); m.cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    data = [(fill((2, 3, 32, 32), 40 + i, 0, 1), None) for i in range(3)]
    seen = []
    mean = training.trainReconstruction(data, m, _recording(seg.MSELoss(), seen), opt, 2)
    assert np.isfinite(seen).all() and np.isfinite(mean)
    assert abs(seen[0] - float(g["acc1_losses"][0])) < 2e-3, (seen[0], float(g["acc1_losses"][0]))


def test_eval_reconstruction_device_vs_host_path(seg):
    from image_segmentation_amd import training
    from oracle import autoencoder_ref
    seg.set_compute_dtype(torch.float32)
    training.VERBOSE = False
    imgs = [fill((3, 40, 56), 61, 0, 1), fill((4, 64, 48), 62, 0, 1), fill((3, 33, 33), 63, 0, 1)]
    data = [([imgs[0], imgs[1]], None), ([imgs[2]], None)]
    o = autoencoder_ref.ReconstructionAutoencoder(3, 3, base_channels=32); fill_module(o, 4200)
    m = seg.ReconstructionAutoencoder(3, 3, base_channels=32); m.load_state_dict(o.state_dict()); m.cuda()
    want = training.evalReconstruction(data, o, torch.nn.MSELoss(), 32, device="cpu")
    got = training.evalReconstruction(data, m, seg.MSELoss(), 32)
    assert not m.training
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-5 * abs(b), (got, want)


def test_pretrained_encoder_hand_off(seg, tmp_path):
    from image_segmentation_amd import training
    from oracle import autoencoder_ref
    seg.set_compute_dtype(torch.float32)
    training.VERBOSE = False
    r = seg.ReconstructionAutoencoder(3, 3, base_channels=32); fill_module(r, 4100); r.cuda()
    opt = torch.optim.Adam(r.parameters(), lr=1e-3)
    data = [(fill((2, 3, 32, 32), 40 + i, 0, 1), None) for i in range(2)]
    loss = training.trainReconstruction(data, r, seg.MSELoss(), opt, 1)
    path = str(tmp_path / "recon.pt")
    torch.save({"epoch": 1, "model_state_dict": r.state_dict(), "optimizer_state_dict": opt.state_dict(),
                "best_val_loss": float(loss)}, path)
    m = _quiet(seg.SegmentationAutoencoder, 3, 32, 3, pretrained_encoder_path=path, freeze_encoder=True)
    saved = torch.load(path, weights_only=False)["model_state_dict"]
    for k, v in m.encoder.encoder.state_dict().items():
        assert torch.equal(v.cpu(), saved["encoder." + k].cpu()), k
    fill_module(m.decoder, 4300); fill_module(m.finalConv, 4301)
    o = autoencoder_ref.SegmentationAutoencoder(3, 32, 3, None, True)
    o.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    m.cuda().train(); o.train()
    x = fill((2, 3, 32, 32), 44, 0, 1)
    y = torch.from_numpy(np.random.RandomState(0).randint(0, 3, (2, 32, 32)))
    lg = m(x.cuda()); lo = o(x)
    F.cross_entropy(lg, y.cuda()).backward(); F.cross_entropy(lo, y).backward()
    assert (lg.detach().cpu() - lo.detach()).abs().max().item() < 1e-3
    assert all(p.grad is None for p in m.encoder.parameters())
    assert m.finalConv.weight.grad is not None


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_recon_unit_compiled_code():
    """zero spills, zero scratch, and the streaming kernels keep their loads in flight"""
    for r in _load_tool("spill_report").report("recon"):
        assert int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0, r
    seen = set()
    for n_ser, n_loads, _, name in _load_tool("serialized_loads").scan("recon"):
        for h in ("recon_head_fwd_kernel", "sigmoid_bwd_act_kernel", "mse_part_kernel", "mse_bwd_kernel"):
            if h in name:
                seen.add(h)
                assert n_ser <= 2, f"{name}: {n_ser} of {n_loads} loads wait for themselves"
    assert len(seen) == 4, seen
