"""GPU (-m gpu): the block matrix -- every branch of the autograd nodes of image_segmentation_amd/ops.py (DoubleConvFn behind
DoubleConvReLU / Down / Up with its optional ConvTranspose, pooling and head stages, and the stand-alone MaxPoolFn, ConvT2x2Fn,
Conv1x1Fn, HeadFn, BilinearFn, ReconHeadFn) on the cases of tests/block_cases.py, through the public modules only.

(a) fp32 mode against the float64 reference of tests/block_reference.py: every output, leaf gradient and BatchNorm buffer of
    every case satisfies  e_64 <= 3 * e_o + 1e-7  (relative L2 per tensor), e_o being the distance of the ORACLE's own fp32
    evaluation from float64, recomputed here on the CPU (host gate: e_o <= 5e-6).  The factor 3 is the project's rule for two
    correct fp32 implementations (tests/test_gpu_batch_parity.py measured 1.1-2.4x).  A conv bias ahead of a batch-statistics
    BatchNorm is exactly zero on the device.  Per-tensor factors above 3 live in block_cases.FACTORS with their reason.
(b) bf16 and fp32: relations that hold bit for bit, because the same kernels run in the same order -- a repeated run; a leaf
    without requires_grad; pool with only y consumed against plain; INPLACE_SKIP_GRAD off against on; Down handed the pooled
    tensor against Down pooling itself; a side stream against the default stream.  (No float64 gate in bf16: storage rounding
    alone moves a single block's gradients by 4-6 %, so such a gate would hold nothing the per-kernel matrices do not.)
(c) the caller's tensors are left alone: hooks that keep the skip and the pooled gradient (Python tensors alive or deleted),
    torch.autograd.grad on both, retain_graph and a second backward.

Measured worst e_64 / e_o per form on an MI355X (fp32; the (a) gate allows 3 + 1e-7 / e_o, i.e. 3.2-3.5 at these e_o), with the
tensor: plain 2.48 d.x; pool 2.51, pool_raw 2.51, pool_y 2.48, pool_p 2.63 (all d.x); xsecond_convt 2.67 d(conv1 BN bias);
xsecond_bilinear 2.29 d.x; up 3.02 d(conv1 BN weight) (e_64 1.12e-6 against the bound 1.21e-6); head 2.77 d(head.bias);
up_head 2.73 d(conv1 BN bias); down_handed = down_self 3.06 d(Down's conv1 BN bias) (9.35e-7 against 1.02e-6); MaxPoolFn 0
(exact); ConvT2x2Fn 1.03; Conv1x1Fn 1.01; HeadFn 1.00; BilinearFn 1.19 / 1.20 (two-pass backward); ReconHeadFn 1.06.  No tensor
needed a factor of its own (block_cases.FACTORS is empty): the xhat recovered from y in the fused pooling reductions stays
within the general rule at these sizes.  The whole file takes about five seconds.
"""
import functools

import pytest
import torch

import block_cases as K
import block_reference as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
dt_id = lambda d: "fp32" if d == torch.float32 else "bf16"          # noqa: E731
ids = lambda cs: [c.id for c in cs]                                   # noqa: E731


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import image_segmentation_amd as s
    return s


class _ActGrad(torch.autograd.Function):
    """Identity whose backward hands its gradient on as a FRESH act tensor nobody else holds -- what a consumer block's
    data-gradient kernel hands the producing block (the case where the pooling backward adds into the skip gradient)."""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        from image_segmentation_amd import ops
        return ops.to_act(g.contiguous(), ctx.dtype), None


class Device:
    """The adapter the graphs of block_cases run on: the package's public modules and stand-alone nodes."""

    def __init__(self, dtype):
        from image_segmentation_amd import ops
        from image_segmentation_amd.unet import _FusedBase
        self.ops, self.dtype, self._base, self._holders = ops, dtype, _FusedBase, {}

    def holder(self, layer):
        """The module a stand-alone node keeps its packed weights on (clipunet.DecoderBlock, autoencoder: the owner)."""
        return self._holders.setdefault(id(layer), self._base())

    def act_grad(self, t):
        return _ActGrad.apply(t, self.dtype)

    def block(self, mod, x, x_second=None, emit_pool=False, head=None):
        return mod(x, x_second=x_second, emit_pool=emit_pool, head=head)

    def up(self, mod, x1, x2, head=None):
        return mod(x1, x2, head=head)

    def down(self, mod, x, pooled=None):
        return mod(x, pooled=pooled)

    def maxpool(self, x):
        return self.ops.MaxPoolFn.apply(x, self.dtype)

    def convt(self, layer, x):
        return self.ops.ConvT2x2Fn.apply(self.holder(layer), x, layer.weight, layer.bias)

    def conv1x1(self, layer, x):
        return self.ops.Conv1x1Fn.apply(self.holder(layer), x, layer.weight, layer.bias)

    def head(self, layer, x):
        return self.ops.HeadFn.apply(self.holder(layer), x, layer.weight, layer.bias)

    def bilinear(self, x, size):
        return self.ops.BilinearFn.apply(x, size, self.dtype)

    def recon(self, layer, x):
        return self.ops.ReconHeadFn.apply(self.holder(layer), x, layer.weight, layer.bias)


def device_run(seg, c, dtype, inplace=True, side_stream=False):
    """Case c on the device in compute dtype `dtype` -> OrderedDict of float64 CPU tensors (names of block_cases.run).  Flags
    and the compute dtype are restored whatever happens."""
    from image_segmentation_amd import ops
    saved = (ops.HEAD_ON_Z, ops.INPLACE_SKIP_GRAD, ops.FUSE_BN_REDUCE)
    seg.set_compute_dtype(dtype)
    try:
        ops.HEAD_ON_Z, ops.INPLACE_SKIP_GRAD = c.on_z, inplace
        m = K.build(c, seg).cuda()
        to = lambda t: t.cuda()                     # noqa: E731
        if side_stream:
            torch.cuda.synchronize()
            with torch.cuda.stream(torch.cuda.Stream()):
                res = K.run(c, Device(dtype), m, to)
        else:
            res = K.run(c, Device(dtype), m, to)
        torch.cuda.synchronize()
        return type(res)((n, t.float().cpu().double()) for n, t in res.items())
    finally:
        ops.HEAD_ON_Z, ops.INPLACE_SKIP_GRAD, ops.FUSE_BN_REDUCE = saved
        seg.set_compute_dtype(torch.bfloat16)


_BASE = {}


def base_run(seg, c, dtype):
    """The case's plain run (default stream, flags as the case says), made once and shared by the tests below; never changed."""
    key = (c, dtype)
    if key not in _BASE:
        _BASE[key] = device_run(seg, c, dtype)
    return _BASE[key]


@functools.lru_cache(maxsize=None)
def reference(c):
    """(float64 reference, e_o: the oracle's own fp32 distance from it per tensor) -- CPU only, nothing from the device."""
    ref = R.evaluate(c)[0]
    return ref, R.distances(c, R.evaluate(c, torch.float32)[0], ref)


def assert_same(a, b, names, what):
    for n in names:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs (max |diff| {(a[n] - b[n]).abs().max().item():.3e})"


# ---------------------------------------------------------------------------------------------------------------------------
# (a) fp32 mode against float64
@pytest.mark.parametrize("case", K.CASES, ids=ids(K.CASES))
def test_fp32_against_float64(seg, case):
    ref, e_o = reference(case)
    got = base_run(seg, case, torch.float32)
    assert list(got) == list(ref), (list(got), list(ref))
    factors = K.FACTORS.get(case.id, {})
    worst, bad = (0.0, "", 0.0, 0.0), []
    for n in ref:
        if K.exact_zero(case, n):
            assert got[n].abs().max().item() == 0.0, f"case {case.id}: {n} must be exactly zero ahead of a batch-statistics BN"
            continue
        assert got[n].shape == ref[n].shape, (case.id, n, got[n].shape, ref[n].shape)
        e64 = R.rel_l2(got[n], ref[n])
        bound = factors.get(n, (3.0, ""))[0] * e_o[n] + 1e-7
        ratio = e64 / e_o[n] if e_o[n] > 0 else (0.0 if e64 == 0 else float("inf"))
        worst = max(worst, (ratio, n, e64, e_o[n]))
        if not e64 <= bound:
            bad.append(f"{n}: e_64 {e64:.3e} is {e64 / bound:.1f}x the bound {bound:.3e} (e_o {e_o[n]:.3e})")
    print(f"case {case.id}: worst e_64/e_o {worst[0]:.2f} in {worst[1]} (e_64 {worst[2]:.2e}, e_o {worst[3]:.2e})")
    assert not bad, f"case {case.id}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) relations that hold bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", K.CASES, ids=ids(K.CASES))
def test_second_run_is_identical(seg, case, dtype):
    a = base_run(seg, case, dtype)
    b = device_run(seg, case, dtype)
    assert list(a) == list(b)
    assert_same(a, b, a, f"case {case.id} [{dt_id(dtype)}] run twice")


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", K.CASES, ids=ids(K.CASES))
def test_side_stream_equals_default_stream(seg, case, dtype):
    a = base_run(seg, case, dtype)
    b = device_run(seg, case, dtype, side_stream=True)
    assert list(a) == list(b)
    assert_same(a, b, a, f"case {case.id} [{dt_id(dtype)}] on a side stream")


ALL_LEAVES = [c for c in K.CASES if c.grads == "all"]


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", ALL_LEAVES, ids=ids(ALL_LEAVES))
def test_dropping_a_leaf_leaves_the_other_gradients_alone(seg, case, dtype):
    full = base_run(seg, case, dtype)
    for grads, gone in (("nox", "d.x"), ("nox2", "d.x2")):
        if gone not in full or not any(n.startswith("d.") and n != gone for n in full):
            continue                # no such leaf / no other leaf (MaxPoolFn, BilinearFn: the input is the only one)
        part = device_run(seg, case._replace(grads=grads), dtype)
        assert list(part) == [n for n in full if n != gone], (case.id, grads)
        assert_same(full, part, part, f"case {case.id} [{dt_id(dtype)}] without requires_grad on {gone[2:]}")


POOL_Y = [c for c in K.CASES if c.form == "pool_y"]


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", POOL_Y, ids=ids(POOL_Y))
def test_pool_with_only_y_consumed_equals_plain(seg, case, dtype):
    a = base_run(seg, case, dtype)
    b = device_run(seg, case._replace(form="plain"), dtype)
    assert list(a) == list(b)
    assert_same(a, b, a, f"case {case.id} [{dt_id(dtype)}] against plain")


BOTH_USED = [c for c in K.CASES if c.form in ("pool", "pool_raw", "down_handed")]


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", BOTH_USED, ids=ids(BOTH_USED))
def test_private_skip_gradient_copy_equals_in_place(seg, case, dtype):
    a = base_run(seg, case, dtype)
    b = device_run(seg, case, dtype, inplace=False)
    assert list(a) == list(b)
    assert_same(a, b, a, f"case {case.id} [{dt_id(dtype)}] with INPLACE_SKIP_GRAD = False")


HANDED = [c for c in K.CASES if c.form == "down_handed"]


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", HANDED, ids=ids(HANDED))
def test_down_handed_the_pooled_tensor_equals_down_pooling_itself(seg, case, dtype):
    a = base_run(seg, case, dtype)
    b = base_run(seg, case._replace(form="down_self"), dtype)
    assert_same(a, b, [n for n in a if n.startswith("out.")], f"case {case.id} [{dt_id(dtype)}] against Down pooling itself")


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the caller's tensors are left alone
class _SkipGraph:
    """dc -> (y, pooled); out = up(y, down(y, pooled)): y is used twice, as skip connection and (pooled) on the main path, so
    the node of dc is handed a skip gradient (an act tensor from up's data-gradient kernel) AND a pooled gradient."""

    def __init__(self, seg):
        from oracle.fill import fill, fill_module
        self.dc, self.down, self.up = seg.DoubleConvReLU(3, 64), seg.Down(64, 128), seg.Up(128, 64)
        for mod, base in ((self.dc, 1000), (self.down, 2000), (self.up, 3000)):
            fill_module(mod, base)
            mod.cuda().train()
        self.x = fill((1, 3, 16, 32), 1, 0, 1).cuda()
        self.g = fill((1, 64, 16, 32), 7, -1, 1).cuda()
        self.y, self.pooled = self.dc(self.x, emit_pool=True)

    def loss(self, cut=False):
        if cut:             # the pooled path cut off: y.grad of the detached copy is the skip gradient alone
            self.yd = self.y.detach().requires_grad_(True)
            out = self.up(self.yd, self.down(self.y, pooled=self.pooled).detach())
        else:
            out = self.up(self.y, self.down(self.y, pooled=self.pooled))
        return (out.float() * self.g).sum()

    def dc_grads(self):
        return {n: p.grad.float().clone() for n, p in self.dc.named_parameters()}


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_kept_gradients_survive_the_backward_that_consumed_them(seg, dtype, monkeypatch):
    from image_segmentation_amd import ops
    copies = []
    private_copy = ops._private_act_copy
    monkeypatch.setattr(ops, "_private_act_copy", lambda t, dt: copies.append(1) or private_copy(t, dt))
    seg.set_compute_dtype(dtype)
    try:
        g = _SkipGraph(seg); g.loss().backward(); torch.cuda.synchronize()
        want = g.dc_grads()
        assert not copies, "nobody else holds the skip gradient of the plain run: the pooled gradient is added in place"
        g = _SkipGraph(seg); g.loss(cut=True).backward(); torch.cuda.synchronize()
        skip = g.yd.grad.float().clone()

        def check(how, kept_skip, grads):
            assert torch.equal(kept_skip.detach().float(), skip), f"{how}: the kept skip gradient was changed by the backward"
            for n in want:
                assert torch.equal(grads[n], want[n]), f"{how}: d({n}) differs from the un-hooked run"

        # hooks on both outputs that keep what they are handed, the Python tensors alive / deleted before backward
        for how in ("hooks, tensors alive", "hooks, tensors deleted"):
            g, kept_y, kept_p = _SkipGraph(seg), [], []
            g.y.register_hook(kept_y.append); g.pooled.register_hook(kept_p.append)
            loss = g.loss()
            if how.endswith("deleted"):
                del g.y, g.pooled
            loss.backward(); torch.cuda.synchronize()
            check(how, kept_y[0], g.dc_grads())
        # torch.autograd.grad captures the very tensors the node is handed
        g = _SkipGraph(seg)
        names = [n for n, _ in g.dc.named_parameters()]
        got = torch.autograd.grad(g.loss(), [g.y, g.pooled] + [p for _, p in g.dc.named_parameters()])
        torch.cuda.synchronize()
        check("autograd.grad", got[0], {n: t.float() for n, t in zip(names, got[2:])})
        # retain_graph and a second backward of the same graph
        g, kept_y, kept_p = _SkipGraph(seg), [], []
        g.y.register_hook(kept_y.append); g.pooled.register_hook(kept_p.append)
        loss = g.loss()
        loss.backward(retain_graph=True); torch.cuda.synchronize()
        first, pooled_first = g.dc_grads(), kept_p[0].detach().float().clone()
        check("retain_graph, first backward", kept_y[0], first)
        for p in list(g.dc.parameters()) + list(g.down.parameters()) + list(g.up.parameters()):
            p.grad = None
        loss.backward(); torch.cuda.synchronize()
        check("retain_graph, second backward", kept_y[1], g.dc_grads())
        check("retain_graph, the first backward's tensors after the second", kept_y[0], first)
        assert torch.equal(kept_p[0].detach().float(), pooled_first) and torch.equal(kept_p[1].detach().float(), pooled_first)
    finally:
        seg.set_compute_dtype(torch.bfloat16)
