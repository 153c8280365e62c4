"""CPU: host-side logic of the reconstruction pretraining loops (reference utils/training.py:123-151 trainReconstruction,
:202-239 evalReconstruction) driven with the CPU oracle model and with recording fakes: the protocol (no zero_grad before
the first batch, step / zero_grad placement, grad_sync hooks), the returned averages, and the per-image evaluation at the
original size with RGBA images cut to RGB."""
import numpy as np
import pytest
import torch

from oracle.fill import fill, fill_module
from oracle import autoencoder_ref
from image_segmentation_amd import training

training.VERBOSE = False


def test_train_reconstruction_matches_reference_protocol(golden):
    """same data / model / Adam as tools/gen_golden.py:gen_trainrecon, run through OUR trainReconstruction"""
    g = golden("trainrecon_ae_32")
    for acc in (1, 2):
        m = autoencoder_ref.ReconstructionAutoencoder(3, 3, base_channels=32); fill_module(m, 4100)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        data = [(fill((2, 3, 32, 32), 40 + i, 0, 1), torch.zeros(2, 1, 32, 32)) for i in range(3)]
        seen = []

        class Recording(torch.nn.MSELoss):
            def forward(self, pred, target):
                out = super().forward(pred, target)
                seen.append(out.item())
                return out
        mean = training.trainReconstruction(data, m, Recording(), opt, acc)
        assert m.training
        assert len(seen) == 3
        assert abs(seen[0] - float(g[f"acc{acc}_losses"][0])) < 1e-6         # before any optimizer step
        np.testing.assert_allclose(seen, g[f"acc{acc}_losses"], atol=1e-5)
        assert isinstance(mean, (float, np.floating))
        assert abs(mean - float(g[f"acc{acc}_mean"])) < 1e-5
        assert mean == pytest.approx(np.mean(np.array(seen, dtype=np.float64)), abs=1e-12)
        np.testing.assert_allclose(m.decoderOut[0].weight.detach().numpy(), g[f"acc{acc}_out_w"], atol=2e-5)
        np.testing.assert_allclose(m.encoder.encoderPart1.conv1.weight.detach().numpy(), g[f"acc{acc}_w0"], atol=2e-5)
        np.testing.assert_allclose(m.encoder.encoderPart1.bn1.running_mean.numpy(), g[f"acc{acc}_rm"], atol=1e-6)


def test_train_reconstruction_step_order_and_average():
    calls = []

    class Opt:
        param_groups = [{"lr": 0.1}]
        def zero_grad(self): calls.append("zero")
        def step(self): calls.append("step")

    class GS:
        def arm(self): calls.append("arm")
        def sync(self): calls.append("sync")

    w = torch.nn.Parameter(torch.ones(1))

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = w

        def forward(self, X):
            assert self.training
            return X * self.w

    data = [(torch.full((1, 1), float(i + 1)), None) for i in range(3)]
    targets = []

    def loss_fn(p, X):
        targets.append(X)
        return (p.sum() - 3.0) ** 2
    model = Model().eval()
    avg = training.trainReconstruction(data, model, loss_fn, Opt(), 2, grad_sync=GS())
    # no zero_grad before the first batch; a step after micro-batch 2 and after the last (3rd) one
    assert calls == ["arm", "sync", "step", "zero", "arm", "sync", "step", "zero"]
    # the loss target is the input batch itself
    assert [float(t) for t in targets] == [1.0, 2.0, 3.0]
    # the mean of EVERY micro-batch's unscaled loss (4, 1, 0), not of the stepping ones only (1, 0)
    assert avg == pytest.approx(5.0 / 3.0, rel=1e-12)
    # gradients of the 1st micro-batch are part of the first step: nothing zeroes them before it
    assert w.grad is not None


def test_train_reconstruction_keeps_gradients_present_before_the_first_batch():
    w = torch.nn.Parameter(torch.zeros(1))
    w.grad = torch.full((1,), 5.0)
    seen = []

    class Opt:
        def zero_grad(self): w.grad = None
        def step(self): seen.append(w.grad.clone())

    model = torch.nn.Module(); model.w = w
    model.forward = lambda X: X * model.w
    data = [(torch.ones(1), None)]
    training.trainReconstruction(data, model, lambda p, X: p.sum(), Opt(), 4)
    assert seen[0].item() == pytest.approx(5.0 + 1.0 / 4)


class _Constant(torch.nn.Module):
    """Returns 0.25 everywhere at the network resolution: after the reverse resize each image's prediction is the
    constant 0.25 at its original size, so the per-image MSE is known from the image alone."""
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.inputs = []

    def forward(self, X):
        assert not self.training and not torch.is_grad_enabled()
        self.inputs.append(X.shape)
        return torch.full((X.shape[0], 3) + tuple(X.shape[2:]), 0.25) + 0 * self.p


def test_eval_reconstruction_known_values():
    imgs = [fill((3, 40, 56), 61, 0, 1), fill((4, 64, 48), 62, 0, 1), fill((3, 33, 33), 63, 0, 1)]
    imgs[1][3] = 10.0                        # an alpha channel that would dominate the loss if it were kept
    data = [([imgs[0], imgs[1]], None), ([imgs[2]], None)]
    model = _Constant().train()
    total, mean = training.evalReconstruction(data, model, torch.nn.MSELoss(), 32)
    assert not model.training
    assert all(s[1] == 3 for s in model.inputs)          # alpha dropped from the network input
    per = [float(((0.25 - im[:3].double()) ** 2).mean()) for im in imgs]
    assert total == pytest.approx(sum(per) / 2, rel=1e-6)       # per-image losses summed, divided by the batch count
    assert mean == pytest.approx(sum(per) / 3, rel=1e-6)        # mean over images
    assert abs(total - mean) > 1e-3
