"""GPU (-m gpu): every compiled instance of the weight-gradient kernels (csrc/wgrad.hip) through the C ABI, one case table
(tests/wgrad_cases.py; tests/test_wgrad_instances.py proves on the CPU that it reaches all of them).

The test owns what ops.wgrad hides: the split-K factor S, the slab buffer (pre-filled with NaN patterns and followed by a
NaN guard of one slab) and the zero page (64 zero bytes between 0xFF neighbours, so a read past the documented 64 bytes
shows up as NaN).

  impulse: dz is zero except for 1.0 in channel n at probe pixel pix[n].  Every product but one is exactly zero, so each
           gradient element must EQUAL one element of the shifted operand (or 0 outside the image), bit for bit, in both
           dtypes: a wrong tap, a dropped edge row, a halo that leaks relu(shift) names its instance, channel, tap and pixel.
  dense:   both operands random in [-1, 1] rounded to `dtype`; reference = the same sums in float64 on the CPU.  Operands
           are exact in the reference, a product of two bf16 values is exact in fp32, accumulation and slabs are fp32 in both
           modes, so ONE bound serves both dtypes: 1e-5 * sqrt(B*H*W) for Conv2d (3x3, 1x1), 1e-4 * sqrt(B*H*W) for
           ConvTranspose2d.  With the BatchNorm+ReLU prologue the reference operand is what segk_bn_relu_apply stores for the
           same z: the prologue form and the materialised-activation form must give the same gradient (DoubleConvFn
           relies on it).
Set SEGK_WGRAD_PARITY_OUT=<file> to record the worst error / bound per instance (profiles/wgrad_matrix_parity.txt)."""
import os

import pytest
import torch
import torch.nn.functional as F

from wgrad_cases import CASES, SPLIT_CASES, TAPS, case_id, instance_of, tile_rows, tiles_of, uses_dma, workgroup_shape

pytestmark = pytest.mark.gpu

TORCH_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
SEGK_DT = {"fp32": 0, "bf16": 1}
NAN_FILL = 0x7FDEAD00          # a quiet-NaN bit pattern: what the kernels must overwrite, and must not touch in the guard
DENSE_BOUND = {0: 1e-5, 1: 1e-5, 2: 1e-4}      # x sqrt(B*H*W), max-abs, both dtypes

_PARITY = {}                   # instance -> [worst error / bound, case id]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_WGRAD_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            f.write("# worst max-abs error / bound of the dense float64 comparison per kernel instance of csrc/wgrad.hip\n"
                    "# (tests/test_gpu_wgrad_matrix.py; bound = 1e-5 * sqrt(B*H*W) for geo 0 and 1, 1e-4 * sqrt(B*H*W) for geo 2,\n"
                    "#  the same for bf16 and fp32; the impulse test of every case is exact)\n")
            for name in sorted(_PARITY):
                f.write(f"{name:40s} {_PARITY[name][0]:.4f}   {_PARITY[name][1]}\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(shape, seed, lo, hi, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo).to(dtype)


@pytest.fixture(scope="module")
def zero_page():
    """64 zero bytes inside an allocation whose every other byte is 0xFF (bf16 0xFFFF and fp32 0xFFFFFFFF are NaNs)."""
    buf = torch.full((8192 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[4096:4096 + 64] = 0
    return buf, buf.data_ptr() + 4096


def probe_pixels(c):
    """(b, y, x) of the impulse probes: corners, edge middles, both sides of every tile boundary in x and in y, first and last
    pixel of the last (partial) tile, last row of one image and first row of the next."""
    B, H, W = c.B, c.H, c.W
    Rs = (4, 8) if (c.geo == 2 and c.dtype == "bf16") else (tile_rows(c),)     # the 4 x 2 ConvTranspose form has 8-row tiles
    pts = []

    def add(b, y, x):
        if 0 <= y < H and 0 <= x < W and (b, y, x) not in pts:
            pts.append((b, y, x))
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        add(0, y, x)
    for xb in range(16, W, 16):
        add(0, H // 2, xb - 1); add(0, H // 2, xb)
    for R in Rs:
        for yb in range(R, H, R):
            add(B - 1, yb - 1, W // 2); add(B - 1, yb, W // 2)
    R = tile_rows(c)
    add(B - 1, (H - 1) // R * R, (W - 1) // 16 * 16); add(B - 1, H - 1, W - 1)
    add(0, H - 1, W // 3); add(B - 1, 0, W // 3)
    assert len(pts) <= c.CD
    return pts


def make_inputs(c, impulse):
    """CPU tensors: dz [B,H,W,CD], the shifted sources a [B,FH,FW,CA] (pre-activation z with the prologue) and b, scale, shift."""
    dt = TORCH_DT[c.dtype]
    f = 2 if c.geo == 2 else 1
    seed = (c.geo * 1000003 + c.CD * 7919 + c.CA * 104729 + c.CB * 1299709 + c.B * 101 + c.H * 31 + c.W * 17 +
            (5 if c.dtype == "bf16" else 0)) % (2 ** 31 - 16)
    if impulse:
        dz = torch.zeros((c.B, c.H, c.W, c.CD), dtype=dt)
        for n, (b, y, x) in enumerate(probe_pixels(c)):
            dz[b, y, x, n] = 1.0
    else:
        dz = _rand((c.B, c.H, c.W, c.CD), seed + 1, -1, 1, dt)
    if c.prologue:
        a = _rand((c.B, f * c.H, f * c.W, c.CA), seed + 2, -2, 2, dt)
        scale = _rand((c.CA,), seed + 4, -1.5, 1.5)
        shift = _rand((c.CA,), seed + 5, 0.1, 0.6)          # relu(shift) > 0 is what a leaking halo would add ...
        shift[3::4] *= -1                                    # ... on three channels of four; negative on the fourth
    else:
        a = _rand((c.B, f * c.H, f * c.W, c.CA), seed + 2, -1, 1, dt)
        scale = shift = None
    b = _rand((c.B, f * c.H, f * c.W, c.CB), seed + 3, -1, 1, dt) if c.CB else None
    return dz, a, b, scale, shift


def split_of(lib, c):
    tiles = lib.query("segk_wgrad_tiles", c.B, c.H, c.W, c.geo, SEGK_DT[c.dtype])
    S = lib.query("segk_wgrad_split", tiles, c.CD, c.CA, c.CB, c.geo, SEGK_DT[c.dtype])
    assert S >= 1
    return S


def run_wgrad(lib, c, inp, S, zeros_ptr):
    """-> (slabs incl. guard as int32 bits [S+1][CD*taps*K], gradient [CD][K][taps] fp32 on the CPU over ALL padded channels)"""
    dz, a, b, scale, shift = inp
    K, taps = c.CA + c.CB, TAPS[c.geo]
    n = c.CD * taps * K
    bits = torch.full((S + 1, n), NAN_FILL, dtype=torch.int32, device="cuda")
    grad = torch.full((c.CD, K, taps), float("nan"), dtype=torch.float32, device="cuda")
    d = [t.cuda() if t is not None else None for t in (dz, a, b, scale, shift)]
    p = lambda t: 0 if t is None else t.data_ptr()
    lib.call("segk_wgrad", p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), bits.data_ptr(), zeros_ptr if c.zero_page else 0,
             S, c.B, c.H, c.W, c.CD, c.CA, c.CB, c.geo, SEGK_DT[c.dtype], _stream())
    lib.call("segk_wgrad_reduce", bits.data_ptr(), S, grad.data_ptr(), c.CD, c.CA, c.CB, c.CD, c.CA, c.CB, taps, _stream())
    torch.cuda.synchronize()
    return bits.cpu(), grad.cpu()


def check_slabs(c, bits, S):
    name = instance_of(c)
    assert torch.isfinite(bits[:S].view(torch.float32)).all(), f"{name} {case_id(c)} S={S}: a slab element was not written"
    assert (bits[S] == NAN_FILL).all(), f"{name} {case_id(c)} S={S}: wrote past the S slabs"


def effective_operand(lib, c, inp):
    """The shifted operand the gradient is defined on, [B,FH,FW,CA+CB] on the CPU in `dtype`: the sources themselves, or with the
    prologue relu(bn(z)) exactly as segk_bn_relu_apply stores it (run on the same z, copied back)."""
    _, a, b, scale, shift = inp
    if c.prologue:
        z = a.cuda(); y = torch.empty_like(z)
        sc, sh = scale.cuda(), shift.cuda()
        lib.call("segk_bn_relu_apply", z.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                 z.numel() // c.CA, c.CA, SEGK_DT[c.dtype], _stream())
        torch.cuda.synchronize()
        a = y.cpu()
        assert (shift > 0).sum() * 2 >= c.CA and (shift < 0).any()
    return a if b is None else torch.cat([a, b], dim=3)


def tap_views(c, a):
    """per tap: the [B,H,W,K] view of the operand that dz pixel (b, y, x) multiplies (zeros outside the image)"""
    if c.geo == 0:
        ap = F.pad(a, (0, 0, 1, 1, 1, 1))
        return [ap[:, ty:ty + c.H, tx:tx + c.W, :] for ty in range(3) for tx in range(3)]
    if c.geo == 1:
        return [a]
    return [a[:, i::2, j::2, :] for i in range(2) for j in range(2)]


def impulse_expected(c, a_eff):
    K, taps = c.CA + c.CB, TAPS[c.geo]
    want = torch.zeros((c.CD, K, taps), dtype=torch.float32)
    views = tap_views(c, a_eff.float())
    for n, (b, y, x) in enumerate(probe_pixels(c)):
        for t in range(taps):
            want[n, :, t] = views[t][b, y, x, :]
    return want


def assert_impulse(c, grad, want, what=""):
    if torch.equal(grad, want):
        return
    pix = probe_pixels(c)
    bad = (grad != want) | torch.isnan(grad)
    idx = bad.nonzero()
    lines = []
    for n, k, t in idx[:12].tolist():
        where = f"probe pixel (b,y,x)={pix[n]}" if n < len(pix) else "a channel without a probe (must be 0)"
        tap = {0: f"tap (ty,tx)=({t // 3},{t % 3})", 1: "tap 0", 2: f"tap (i,j)=({t >> 1},{t & 1})"}[c.geo]
        lines.append(f"  dw[n={n}, k={k}, {tap}] = {grad[n, k, t].item()!r}, want {want[n, k, t].item()!r}; {where}")
    taps_bad = sorted(set(idx[:, 2].tolist()))
    pix_bad = sorted(set(pix[n] if n < len(pix) else None for n in set(idx[:, 0].tolist())), key=str)
    raise AssertionError(f"{instance_of(c)} {case_id(c)} {what}: {len(idx)} gradient elements differ; taps {taps_bad}; "
                         f"probe pixels {pix_bad}\n" + "\n".join(lines))


def dense_reference(c, dz, a_eff):
    P = c.B * c.H * c.W
    d = dz.double().reshape(P, c.CD).t().contiguous()
    return torch.stack([d @ v.reshape(P, -1) for v in tap_views(c, a_eff.double())], dim=2)      # [CD][K][taps]


def dense_ratio(c, grad, ref):
    bound = DENSE_BOUND[c.geo] * (c.B * c.H * c.W) ** 0.5
    assert torch.isfinite(grad).all(), f"{instance_of(c)} {case_id(c)}: non-finite gradient"
    return (grad.double() - ref).abs().max().item() / bound


def record(c, ratio):
    name = instance_of(c)
    if name not in _PARITY or ratio > _PARITY[name][0]:
        _PARITY[name] = [ratio, case_id(c)]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_impulse_is_exact(lib, zero_page, case):
    c = case
    inp = make_inputs(c, impulse=True)
    S = split_of(lib, c)
    bits, grad = run_wgrad(lib, c, inp, S, zero_page[1])
    check_slabs(c, bits, S)
    assert_impulse(c, grad, impulse_expected(c, effective_operand(lib, c, inp)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dense_against_float64(lib, zero_page, case):
    c = case
    inp = make_inputs(c, impulse=False)
    S = split_of(lib, c)
    bits, grad = run_wgrad(lib, c, inp, S, zero_page[1])
    check_slabs(c, bits, S)
    ratio = dense_ratio(c, grad, dense_reference(c, inp[0], effective_operand(lib, c, inp)))
    print(f"{instance_of(c)} {case_id(c)} S={S}: error / bound = {ratio:.4f}")
    record(c, ratio)
    assert ratio <= 1.0, f"{instance_of(c)} {case_id(c)}: max-abs error is {ratio:.3f} x the bound"
    bits2, grad2 = run_wgrad(lib, c, inp, S, zero_page[1])          # fresh buffers: same bits
    assert torch.equal(bits, bits2) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))


@pytest.mark.parametrize("case", SPLIT_CASES, ids=case_id)
def test_split_k_and_slab_hygiene(lib, zero_page, case):
    """Any S >= 1 is valid (include/segk.h): slabs beyond the tile count are written as zeros, nothing past slab S is touched."""
    c = case
    tiles = tiles_of(c)
    imp, den = make_inputs(c, impulse=True), make_inputs(c, impulse=False)
    a_imp, a_den = effective_operand(lib, c, imp), effective_operand(lib, c, den)
    want, ref = impulse_expected(c, a_imp), dense_reference(c, den[0], a_den)
    for S in sorted({1, 2, split_of(lib, c), tiles, tiles + 3}):
        bits, grad = run_wgrad(lib, c, imp, S, zero_page[1])
        check_slabs(c, bits, S)
        assert_impulse(c, grad, want, f"S={S}")
        bits, grad = run_wgrad(lib, c, den, S, zero_page[1])
        check_slabs(c, bits, S)
        if S > tiles:
            assert (bits[tiles:S] << 1 == 0).all(), f"{instance_of(c)} S={S}: slabs beyond the {tiles} tiles are not zero"
        ratio = dense_ratio(c, grad, ref)
        print(f"{instance_of(c)} {case_id(c)} S={S} (tiles {tiles}): error / bound = {ratio:.4f}")
        record(c, ratio)
        assert ratio <= 1.0, f"{instance_of(c)} {case_id(c)} S={S}: max-abs error is {ratio:.3f} x the bound"
        bits2, grad2 = run_wgrad(lib, c, den, S, zero_page[1])
        assert torch.equal(bits, bits2) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32)), f"S={S}: not bit-stable"


@pytest.mark.parametrize("case", [c for c in CASES if c.geo == 0 and c.dtype == "bf16" and not c.zero_page], ids=case_id)
def test_null_zero_page_agrees_with_zero_page(lib, zero_page, case):
    """bf16 3x3 with zeros64 == NULL (register-staged kernel) against the LDS-DMA kernel on the same inputs: the impulse gradient
    bit for bit; dense, each within the bound of the float64 reference."""
    c, cz = case, case._replace(zero_page=True)
    assert not uses_dma(c) and uses_dma(cz) and workgroup_shape(c)[1] == workgroup_shape(cz)[1]
    inp = make_inputs(c, impulse=True)
    S = split_of(lib, c)
    _, g0 = run_wgrad(lib, c, inp, S, zero_page[1])
    _, g1 = run_wgrad(lib, cz, inp, S, zero_page[1])
    assert_impulse(c, g0, g1, "against the zero-page run")
    inp = make_inputs(c, impulse=False)
    ref = dense_reference(c, inp[0], effective_operand(lib, c, inp))
    for cc in (c, cz):
        ratio = dense_ratio(cc, run_wgrad(lib, cc, inp, S, zero_page[1])[1], ref)
        assert ratio <= 1.0, f"{instance_of(cc)} {case_id(cc)}: max-abs error is {ratio:.3f} x the bound"
    assert (zero_page[0][:4096] == 0xFF).all() and (zero_page[0][4096 + 64:] == 0xFF).all()
