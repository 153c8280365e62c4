"""The case table of the block matrix (tests/test_block_cases_host.py, tests/test_gpu_block_matrix.py): every branch of the
autograd nodes of image_segmentation_amd/ops.py -- above all DoubleConvFn, the node behind DoubleConvReLU / Down / Up -- as one
small graph each, with seeded parameters, inputs and upstream gradients (oracle.fill).

A case is (form, mode, B, CA, CB, Cout, H, W, classes, bias, grads) plus the seed its fills derive from and, for the head
forms, the value of ops.HEAD_ON_Z.  The graph of a form is written ONCE, in graph(), against an adapter `A` that supplies the
operations: tests/block_reference.py implements them with the oracle's modules and stock torch ops in float64 on the CPU,
tests/test_gpu_block_matrix.py with the package's public modules and stand-alone nodes.  Nothing here imports the package.

Shapes are the smallest at which each branch still exists.  They are also bounded from above by the two guards of
block_reference.guards (no BatchNorm output and no pooling decision may sit within 1e-4 RMS of a tie): the smallest of n
standard normal values is about 1.25 / n, so a block with more than a few ten thousand BatchNorm outputs cannot pass for any
seed.  Wide blocks (64, 96 channels) therefore run at B = 1, 16x16, and the larger images carry few channels.  A case that
fails a guard or the fp32 yardstick of the host test gets another SEED here -- never another bound there.
"""
from collections import OrderedDict
from typing import NamedTuple

import torch
from torch import nn

from oracle.fill import fill, fill_module

F32, BF16 = 0, 1            # include/segk.h: SEGK_DT_F32, SEGK_DT_BF16


class Case(NamedTuple):
    form: str
    mode: str            # train | eval (frozen BatchNorm: running statistics)
    B: int
    CA: int              # channels of the block input x (first concat operand)
    CB: int              # channels of the second concat operand (0: none); for `up` forms CB == Cout
    Cout: int
    H: int
    W: int
    classes: int         # output channels of the 1x1 head / of the stand-alone layer (0: none)
    bias: bool
    grads: str           # all | nox (all but the block input) | nox2 (all but the second input) | xonly (parameters frozen)
    seed: int = 1
    on_z: bool = True    # ops.HEAD_ON_Z while the case runs (head forms)

    @property
    def id(self):
        s = f"{self.form}/{self.mode}/b{self.B}-{self.CA}+{self.CB}-{self.Cout}-{self.H}x{self.W}/{self.grads}"
        if self.classes:
            s += f"/k{self.classes}"
        if not self.bias:
            s += "/nobias"
        if self.form in HEAD_FORMS:
            s += "/on_z" if self.on_z else "/on_y"
        return s


# forms that run DoubleConvFn (all of them exist in train and eval mode) and the stand-alone nodes
POOL_FORMS = ("pool", "pool_raw", "pool_y", "pool_p")
HEAD_FORMS = ("head", "up_head")
DC_FORMS = ("plain",) + POOL_FORMS + ("xsecond_convt", "xsecond_bilinear", "up") + HEAD_FORMS + ("down_handed", "down_self")
NODE_FORMS = ("maxpool", "convt", "conv1x1", "headfn", "bilinear", "bilinear_2pass", "recon")
SECOND_INPUT = ("xsecond_convt", "xsecond_bilinear", "up", "up_head")


def C(form, mode, B, CA, CB, Cout, H, W, classes=0, bias=True, grads="all", seed=1, on_z=True):
    return Case(form, mode, B, CA, CB, Cout, H, W, classes, bias, grads, seed, on_z)


# Widths: 64 against 96 (padded width 96 is no power of two: segk_maxpool_bwd_stat_blocks declines and the pooling backward
# without the fused reductions runs), 64 against 32 / 96 in bf16 (segk_conv_writes_act_q), 3 -> 64 at W % 16 == 0 against
# W = 40 / 22 and against 3 -> 32 (segk_stem3x3_rows, segk_stem3x3_wgrad_slabs: bf16 only), 8 and 40 (no multiple of 32).
# 17x22: odd height, the last row belongs to no pooling window.
CASES = [
    # ---- plain
    C("plain", "train", 1, 3, 0, 64, 16, 16, seed=107),    # the stem shape (bf16: stem kernels)
    C("plain", "train", 1, 3, 0, 64, 16, 16, grads="nox", seed=107),    # first block of every model: input needs no gradient
    C("plain", "train", 2, 3, 0, 8, 24, 40, bias=False, seed=6),
    C("plain", "train", 1, 32, 0, 40, 18, 22, grads="xonly", seed=3),
    C("plain", "train", 1, 3, 0, 32, 16, 32, grads="nox", seed=23),    # W % 16 == 0 but 32 wide: no stem
    C("plain", "eval", 1, 3, 0, 64, 16, 16, seed=92),
    C("plain", "eval", 1, 8, 0, 40, 17, 22, bias=False, seed=4),
    C("plain", "eval", 1, 32, 0, 32, 16, 16, grads="nox", seed=16),
    C("plain", "eval", 1, 32, 0, 32, 16, 16, grads="xonly", seed=16),
    # ---- pool: both outputs used (skip gradient as an act tensor / from a stock op), one of them only
    C("pool", "train", 1, 3, 0, 64, 16, 16, seed=107),
    C("pool", "train", 1, 8, 0, 96, 16, 16, seed=103),    # the fused reductions decline
    C("pool", "train", 2, 3, 0, 8, 17, 22, seed=3),    # odd height
    C("pool", "train", 1, 3, 0, 64, 16, 16, grads="nox", seed=107),
    C("pool_raw", "train", 1, 3, 0, 64, 16, 16, seed=107),
    C("pool_raw", "train", 1, 32, 0, 96, 16, 16, seed=99),
    C("pool_y", "train", 1, 3, 0, 64, 16, 16, seed=107),
    C("pool_y", "train", 1, 8, 0, 40, 18, 22, seed=12),
    C("pool_p", "train", 1, 3, 0, 64, 16, 16, seed=107),
    C("pool_p", "train", 1, 8, 0, 96, 16, 16, seed=103),
    C("pool_p", "train", 2, 3, 0, 8, 17, 22, seed=3),
    C("pool", "eval", 1, 3, 0, 64, 16, 16, seed=198),
    C("pool", "eval", 1, 8, 0, 96, 16, 16, bias=False, seed=395),
    C("pool_raw", "eval", 2, 3, 0, 8, 17, 22, seed=2),
    C("pool_y", "eval", 1, 32, 0, 32, 16, 16, seed=25),
    C("pool_p", "eval", 1, 32, 0, 32, 16, 16, grads="nox", seed=25),
    # ---- explicit concat of two act tensors (clipunet.DecoderBlock: ConvT2x2Fn / BilinearFn produce the operands)
    C("xsecond_convt", "train", 1, 32, 32, 64, 16, 16, seed=143),
    C("xsecond_convt", "train", 2, 8, 40, 8, 18, 22, bias=False, grads="nox2", seed=13),
    C("xsecond_bilinear", "train", 1, 8, 8, 40, 18, 22, seed=6),
    C("xsecond_bilinear", "train", 1, 32, 32, 32, 16, 16, grads="nox", seed=6),
    C("xsecond_convt", "eval", 1, 32, 32, 64, 16, 16, bias=False, seed=24),
    C("xsecond_bilinear", "eval", 1, 8, 8, 8, 24, 40, grads="nox2", seed=4),
    # ---- up (ConvTranspose2d inside the node; the bias gradient from the concat data-gradient's channel sums)
    C("up", "train", 1, 64, 64, 64, 16, 16, seed=2),
    C("up", "train", 1, 32, 32, 32, 16, 32, grads="nox", seed=111),
    C("up", "train", 2, 8, 8, 8, 18, 22, grads="nox2"),
    C("up", "train", 1, 40, 40, 40, 16, 16, grads="xonly", seed=11),
    C("up", "eval", 1, 32, 32, 32, 16, 16, seed=8),
    C("up", "eval", 1, 64, 64, 64, 16, 16, grads="nox2", seed=11),
    C("up", "eval", 2, 8, 8, 8, 18, 22, grads="nox", seed=3),
    # ---- head inside the node, on the pre-activation and on the block output
    C("head", "train", 1, 3, 0, 64, 16, 16, classes=3, seed=107),
    C("head", "train", 1, 3, 0, 64, 16, 16, classes=3, on_z=False, seed=107),
    C("head", "train", 1, 8, 0, 40, 18, 22, classes=5, grads="nox", seed=12),
    C("head", "train", 1, 8, 0, 40, 18, 22, classes=5, grads="nox", on_z=False, seed=12),
    C("head", "eval", 1, 32, 0, 32, 16, 16, classes=2, seed=16),
    C("head", "eval", 1, 32, 0, 32, 16, 16, classes=2, on_z=False, seed=16),
    C("up_head", "train", 1, 64, 64, 64, 16, 16, classes=3, seed=2),
    C("up_head", "train", 1, 64, 64, 64, 16, 16, classes=3, on_z=False, seed=2),
    C("up_head", "train", 2, 8, 8, 8, 18, 22, classes=4, grads="nox2"),
    C("up_head", "eval", 1, 32, 32, 32, 16, 16, classes=3, seed=8),
    C("up_head", "eval", 1, 32, 32, 32, 16, 16, classes=3, on_z=False, seed=8),
    C("up_head", "eval", 1, 40, 40, 40, 16, 16, classes=2, grads="xonly", seed=5),
    # ---- Down behind a block: handed the pooled tensor the block emitted / pooling itself through MaxPoolFn
    C("down_handed", "train", 1, 3, 0, 8, 24, 40, seed=3),
    C("down_self", "train", 1, 3, 0, 8, 24, 40, seed=3),
    C("down_handed", "train", 2, 3, 0, 8, 17, 22, grads="nox", seed=3),
    C("down_self", "train", 2, 3, 0, 8, 17, 22, grads="nox", seed=3),
    C("down_handed", "eval", 1, 8, 0, 32, 16, 16, seed=32),
    C("down_self", "eval", 1, 8, 0, 32, 16, 16, seed=32),
    # ---- the stand-alone nodes, one case per needs_input_grad pattern each branches on
    C("maxpool", "train", 2, 40, 0, 40, 17, 22, seed=5),
    C("convt", "train", 1, 32, 0, 40, 12, 20, classes=40),
    C("convt", "train", 1, 32, 0, 40, 12, 20, classes=40, grads="nox"),
    C("convt", "train", 2, 8, 0, 8, 9, 11, classes=8, bias=False),
    C("conv1x1", "train", 2, 40, 0, 8, 18, 22, classes=8),
    C("conv1x1", "train", 2, 40, 0, 8, 18, 22, classes=8, grads="nox"),
    C("conv1x1", "train", 1, 32, 0, 64, 16, 16, classes=64, bias=False),
    C("headfn", "train", 2, 40, 0, 40, 18, 22, classes=5),
    C("bilinear", "train", 2, 8, 0, 8, 18, 22),    # 9x11 -> 18x22: single pass
    C("bilinear_2pass", "train", 1, 40, 0, 40, 24, 40),    # 6x10 -> 24x40: the separable two-pass backward
    C("recon", "train", 2, 8, 0, 3, 18, 22, classes=3),
    C("recon", "train", 2, 8, 0, 3, 18, 22, classes=3, grads="nox"),
    C("recon", "train", 2, 8, 0, 3, 18, 22, classes=3, grads="xonly"),
    C("recon", "train", 1, 32, 0, 1, 16, 16, classes=1, bias=False),
]

# Per-tensor factors above the general 3 (test_gpu_block_matrix.py (a)): {case id: {tensor: (factor, reason)}}.  A factor comes
# from a bound derived in tests/stem_pool_reference.py / tests/bn_reference.py for an algorithm include/segk.h documents as
# less accurate, never from what the device produced, and never exceeds 16.
FACTORS = {}


def second_shape(c):
    """Shape of the second input: the source of the ConvTranspose2d / of the bilinear resize."""
    if c.form == "xsecond_bilinear":
        return (c.B, c.CB, max(2, c.H // 3), max(2, c.W // 3))
    if c.form == "xsecond_convt":
        return (c.B, 2 * c.CB, c.H // 2, c.W // 2)
    return (c.B, c.CA + c.CB, c.H // 2, c.W // 2)          # up: ConvTranspose2d(CA + CB -> CB)


def x_shape(c):
    if c.form == "bilinear":
        return (c.B, c.CA, c.H // 2, c.W // 2)
    if c.form == "bilinear_2pass":
        return (c.B, c.CA, c.H // 4, c.W // 4)
    return (c.B, c.CA, c.H, c.W)


class Modules(nn.Module):
    """The parameter holders of one case, under fixed names (the names of the gradients and buffers the runs report)."""


def build(c, lib):
    """lib supplies DoubleConvReLU / Down / Up (oracle.unet_ref or the package: same constructors, same state_dict); the
    stand-alone layers are stock containers in both.  Filled from the case's seed, BatchNorm running statistics moved away
    from (0, 1), train / eval as the case says."""
    m = Modules()
    if c.form in DC_FORMS:
        if c.form in ("up", "up_head"):
            assert c.CB == c.Cout
            m.up = lib.Up(c.CA + c.CB, c.Cout)
        else:
            m.blk = lib.DoubleConvReLU(c.CA + c.CB, c.Cout, bias=c.bias)
        if c.form == "xsecond_convt":
            m.ct = nn.ConvTranspose2d(2 * c.CB, c.CB, kernel_size=2, stride=2, bias=c.bias)
        if c.form in HEAD_FORMS:
            m.head = nn.Conv2d(c.Cout, c.classes, kernel_size=1)
        if c.form in ("down_handed", "down_self"):
            m.down = lib.Down(c.Cout, c.Cout)
    elif c.form == "convt":
        m.ct = nn.ConvTranspose2d(c.CA, c.classes, kernel_size=2, stride=2, bias=c.bias)
    elif c.form == "conv1x1":
        m.c1 = nn.Conv2d(c.CA, c.classes, kernel_size=1, bias=c.bias)
    elif c.form == "headfn":
        m.head = nn.Conv2d(c.CA, c.classes, kernel_size=1)
    elif c.form == "recon":
        m.rc = nn.Conv2d(c.CA, c.classes, kernel_size=3, padding=1, bias=c.bias)
    base = 10000 * c.seed
    fill_module(m, base + 1000)
    k = 0
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(fill(tuple(mod.running_mean.shape), base + 300 + k, -0.2, 0.2))
                mod.running_var.copy_(fill(tuple(mod.running_var.shape), base + 400 + k, 0.5, 1.5))
                k += 1
    m.train(c.mode == "train")
    return m


def inputs(c):
    """fp32 CPU tensors: x and, for the forms with a second input, x2."""
    base = 10000 * c.seed
    out = OrderedDict(x=fill(x_shape(c), base + 1, -1, 1))
    if c.form in SECOND_INPUT:
        out["x2"] = fill(second_shape(c), base + 2, -1, 1)
    return out


def upstream(c, name, shape):
    """The fixed gradient of output `name`, applied as (out * g).sum()."""
    k = {"y": 5, "pooled": 6, "logits": 5, "out": 7}[name]
    return fill(tuple(shape), 10000 * c.seed + k, -1, 1)


def leaf_flags(c):
    """(block input requires grad, second input requires grad, parameters require grad)."""
    return c.grads != "nox", c.grads != "nox2", c.grads != "xonly"


def graph(c, A, m, x, x2=None):
    """The case's graph on adapter A -> OrderedDict of its outputs (the tensors that take an upstream gradient)."""
    f = c.form
    if f == "plain":
        return OrderedDict(y=A.block(m.blk, x))
    if f in POOL_FORMS:
        y, p = A.block(m.blk, x, emit_pool=True)
        if f == "pool":
            y = A.act_grad(y)          # the skip gradient reaches the node as an act tensor, as from a consumer's dgrad kernel
        return OrderedDict(([("y", y)] if f != "pool_p" else []) + ([("pooled", p)] if f != "pool_y" else []))
    if f == "xsecond_convt":
        return OrderedDict(y=A.block(m.blk, x, x_second=A.convt(m.ct, x2)))
    if f == "xsecond_bilinear":
        return OrderedDict(y=A.block(m.blk, x, x_second=A.bilinear(x2, (c.H, c.W))))
    if f == "up":
        return OrderedDict(y=A.up(m.up, x, x2))
    if f == "head":
        return OrderedDict(logits=A.block(m.blk, x, head=m.head))
    if f == "up_head":
        return OrderedDict(logits=A.up(m.up, x, x2, head=m.head))
    if f == "down_handed":
        y, p = A.block(m.blk, x, emit_pool=True)
        return OrderedDict(y=y, out=A.down(m.down, y, pooled=p))
    if f == "down_self":
        y = A.block(m.blk, x)
        return OrderedDict(y=y, out=A.down(m.down, y))
    if f == "maxpool":
        return OrderedDict(y=A.maxpool(x))
    if f == "convt":
        return OrderedDict(y=A.convt(m.ct, x))
    if f == "conv1x1":
        return OrderedDict(y=A.conv1x1(m.c1, x))
    if f == "headfn":
        return OrderedDict(logits=A.head(m.head, x))
    if f in ("bilinear", "bilinear_2pass"):
        return OrderedDict(y=A.bilinear(x, (c.H, c.W)))
    if f == "recon":
        return OrderedDict(y=A.recon(m.rc, x))
    raise ValueError(f)


def run(c, A, m, to, differentiate=True):
    """Run the case: `to` moves / casts an fp32 CPU tensor to where adapter A computes (the modules `m` already are there).
    -> OrderedDict name -> detached tensor: "out.<name>" every output, "d.x" / "d.x2" / "d.<parameter>" every leaf gradient,
    "buf.<name>" every BatchNorm buffer after the step."""
    need_x, need_x2, need_p = leaf_flags(c)
    inp = inputs(c)
    x = to(inp["x"]).requires_grad_(need_x)
    x2 = to(inp["x2"]).requires_grad_(need_x2) if "x2" in inp else None
    for p in m.parameters():
        p.requires_grad_(need_p)
        p.grad = None
    outs = graph(c, A, m, x, x2)
    res = OrderedDict(("out." + n, t.detach()) for n, t in outs.items())
    if differentiate:
        loss = None
        for n, t in outs.items():
            term = (t * to(upstream(c, n, t.shape)).to(t.dtype)).sum()
            loss = term if loss is None else loss + term
        loss.backward()
        if need_x:
            res["d.x"] = x.grad.detach()
        if x2 is not None and need_x2:
            res["d.x2"] = x2.grad.detach()
        if need_p:
            for n, p in m.named_parameters():
                res["d." + n] = p.grad.detach()
    for n, b in m.named_buffers():
        res["buf." + n] = b.detach().clone()
    return res


def exact_zero(c, name):
    """A conv bias ahead of a batch-statistics BatchNorm: its true gradient is identically zero, the device returns exact
    zeros and the reference holds cancellation noise (the rule of test_gpu_modules.check_param_grads)."""
    return c.mode == "train" and name.startswith("d.") and name.endswith(("doubleConvReLU.0.bias", "doubleConvReLU.3.bias"))


def pad32(n):
    return (n + 31) // 32 * 32


def predicates(c, dt, query):
    """The host predicates DoubleConvFn branches on, for case c in compute dtype dt (F32 / BF16), asked of the library through
    query(name, *args) -> {predicate: bool}; only those the case reaches."""
    if c.form not in DC_FORMS:
        return {}
    Cp = pad32(c.Cout)
    out = {"second_operand": c.CB > 0, "cout_multiple_of_32": c.Cout % 32 == 0}
    if c.mode == "train":
        out["conv_writes_act"] = query("segk_conv_writes_act_q", Cp, Cp, dt) != 0
    if c.form in ("pool", "pool_raw", "pool_p", "down_handed"):
        out["pool_bwd_stat_blocks"] = query("segk_maxpool_bwd_stat_blocks", c.B, c.H, c.W, Cp, dt) > 0
    if c.CB == 0:
        out["stem_rows"] = query("segk_stem3x3_rows", c.B, c.H, c.W, c.CA, c.Cout, dt) > 0
        out["stem_wgrad_slabs"] = query("segk_stem3x3_wgrad_slabs", c.B, c.H, c.W, c.CA, c.Cout, dt) > 0
    return out
