"""The float64 reference of the block matrix: the oracle's own modules (oracle/unet_ref.py: DoubleConvReLU, Down, Up) plus stock
F.max_pool2d, F.conv_transpose2d, F.interpolate(bilinear, align_corners=False), 1x1 / 3x3 conv2d and sigmoid, evaluated on the
CPU and differentiated by autograd.  Nothing of the package is in here.

Reference: the adapter the graphs of tests/block_cases.py run on (reference(case, dtype) -> every output, leaf gradient and
BatchNorm buffer).  Functional: the same with the blocks restated from functional ops and BatchNorm written out; the host test
holds the two together to 1e-12, and this one also records what the guards need -- every BatchNorm output ahead of its ReLU and
every tensor that gets pooled."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import unet_ref

import block_cases as K


class Reference:
    def act_grad(self, t):
        return t

    def dc(self, mod, x):
        return mod(x)

    def block(self, mod, x, x_second=None, emit_pool=False, head=None):
        y = self.dc(mod, x if x_second is None else torch.cat([x, x_second], dim=1))
        if head is not None:
            return F.conv2d(y, head.weight, head.bias)
        return (y, self.maxpool(y)) if emit_pool else y

    def up(self, mod, x1, x2, head=None):
        y = mod(x1, x2)
        return y if head is None else F.conv2d(y, head.weight, head.bias)

    def down(self, mod, x, pooled=None):
        return mod(x)               # the oracle's Down pools itself; `pooled` is the package's shortcut for the same tensor

    def maxpool(self, x):
        return F.max_pool2d(x, 2, 2)

    def convt(self, layer, x):
        return F.conv_transpose2d(x, layer.weight, layer.bias, stride=2)

    def conv1x1(self, layer, x):
        return F.conv2d(x, layer.weight, layer.bias)

    head = conv1x1

    def bilinear(self, x, size):
        return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)

    def recon(self, layer, x):
        return torch.sigmoid(F.conv2d(x, layer.weight, layer.bias, padding=1))


class Functional(Reference):
    """The blocks from functional ops, BatchNorm written out (batch statistics with the biased variance, the unbiased one into
    running_var, momentum update; running statistics in eval mode)."""

    def __init__(self):
        self.bn_out, self.pooled_from = [], []

    def bn(self, z, bn):
        if bn.training:
            n = z.numel() // z.shape[1]
            mean = z.mean(dim=(0, 2, 3))
            var = ((z - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
            with torch.no_grad():
                bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean)
                bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * var * n / (n - 1))
                bn.num_batches_tracked.add_(1)
        else:
            mean, var = bn.running_mean, bn.running_var
        out = (z - mean[None, :, None, None]) / torch.sqrt(var + bn.eps)[None, :, None, None]
        out = out * bn.weight[None, :, None, None] + bn.bias[None, :, None, None]
        self.bn_out.append(out.detach())
        return out

    def dc(self, mod, x):
        s = mod.doubleConvReLU
        a1 = torch.clamp(self.bn(F.conv2d(x, s[0].weight, s[0].bias, padding=1), s[1]), min=0)
        return torch.clamp(self.bn(F.conv2d(a1, s[3].weight, s[3].bias, padding=1), s[4]), min=0)

    def up(self, mod, x1, x2, head=None):
        u = F.conv_transpose2d(x2, mod.upsample.weight, mod.upsample.bias, stride=2)
        return self.block(mod.doubleConv, x1, x_second=u, head=head)

    def down(self, mod, x, pooled=None):
        return self.dc(mod.maxpool_doubleConv[1], self.maxpool(x))

    def maxpool(self, x):
        self.pooled_from.append(x.detach())
        B, C, H, W = x.shape
        w = x[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2)
        return w.amax(dim=(3, 5))


def evaluate(c, dtype=torch.float64, adapter=None):
    """Case c on the CPU in `dtype` -> (OrderedDict of float64 tensors as block_cases.run names them, the adapter)."""
    A = Reference() if adapter is None else adapter
    m = K.build(c, unet_ref).to(dtype)
    res = K.run(c, A, m, lambda t: t.to(dtype))
    return OrderedDict((n, t.double()) for n, t in res.items()), A


def rel_l2(a, ref):
    """||a - ref|| / ||ref|| (||a|| where the reference is identically zero)."""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    d, n = (a - ref).norm().item(), ref.norm().item()
    return d / n if n > 0 else a.norm().item()


def distances(c, got, ref):
    """name -> rel_l2 for every tensor of the reference except the identically-zero conv bias gradients."""
    assert list(got) == list(ref), (list(got), list(ref))
    return OrderedDict((n, rel_l2(got[n], ref[n])) for n in ref if not K.exact_zero(c, n))


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


def guards(c):
    """(smallest |BatchNorm output ahead of its ReLU| / that tensor's RMS over every BatchNorm of the case, smallest gap between
    the two largest values of a pooling window with a positive maximum / the pooled-from tensor's RMS); inf where the case has
    no such tensor.  Both have to exceed 1e-4, otherwise a rounding error decides a ReLU or a pooling route."""
    A = Functional()
    evaluate(c, torch.float64, A)
    g_bn = min((t.abs().min().item() / _rms(t) for t in A.bn_out), default=float("inf"))
    g_pool = float("inf")
    for t in A.pooled_from:
        B, C, H, W = t.shape
        w = t[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        top = w.topk(2, dim=1).values
        live = top[:, 0] > 0
        if live.any():
            g_pool = min(g_pool, (top[live, 0] - top[live, 1]).min().item() / _rms(t))
    return g_bn, g_pool
