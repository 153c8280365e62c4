"""GPU (-m gpu): every reachable instance of the 1x1-geometry kernels -- gemm_dma_kernel (csrc/gemm.hip), convt_stream_kernel
(csrc/convt_stream.hip) and the GEO == 1 instances of conv_igemm_kernel (csrc/conv_igemm.hip) -- through the C ABI only
(segk_pack_conv_weight with taps 1, segk_pack_convt_weight, segk_linear, segk_linear_splitk, segk_conv1x1, segk_convt2x2_fwd,
segk_convt2x2_dgrad), one case table (tests/gemm_cases.py; tests/test_gemm_instances.py proves on the CPU that it reaches all
of them), three runs per case against tests/gemm_reference.py.

The test owns every buffer: the packed weights are pre-filled with NaN and must come back without one; outputs are pre-filled
with a NaN pattern and followed by guard rows that must stay untouched; no NaN may remain inside an output (for the
ConvTranspose: every one of the 2H x 2W pixels is written); padded output channels must be exactly zero; split-K parts are
checked part by part, the guard stands behind the last part.

  one-hot: every row of the A operand is zero except a single 1.0 at k(m), which walks every logical k (the edges of every
           32- and 64-element chunk and the last k below a padded chunk first); for the data gradient that is one (tap, channel)
           of the pixel's 2 x 2 output block.  Weights and bias are multiples of 1/64, so every output element must EQUAL one
           weight plus the bias: a wrong chunk, swizzle, weight-row permutation, tap order or pixel of the shuffle / un-shuffle
           arithmetic names its instance, row or pixel, column, k and tap.
  lattice: x in {-1, 0, 1}, w in {-1, -1/2, 0, 1/2, 1}, bias a multiple of 1/2: every partial sum in any order is exact in fp32,
           so outputs must equal the reference rounded to `dtype`; a split-K part its own K range's product, the bias in part 0
           only.  A skipped or doubled K chunk, a ring-slot or parity slip at a unit boundary cannot hide behind an order.
  dense:   operands uniform in [-1, 1] rounded to `dtype`, float64 torch.matmul on the exact operands, the derived any-order
           bound of gemm_reference.py; the act = 1 cases (quick_gelu in float64) take this run only.
The cases with three or more work units per workgroup, or trips round the streaming kernel's loop (LONG_CASES), take the two
exact runs only.  Equality is numerical equality of every element (NaN equals nothing; -0 equals 0).  The launch arithmetic of
the table is evaluated for 256 compute units: test_device_has_the_compute_units_the_table_was_made_for fails on another device.
Set SEGK_GEMM_PARITY_OUT=<file> to record the worst error / bound per instance (profiles/gemm_matrix_parity.txt)."""
import os

import pytest
import torch

from gemm_cases import CASES, LONG_CASES, NUM_CUS, case_id, gemm_view, instance_of, rows_of, splitk_ok
from gemm_reference import (ACT_ULPS, TORCH_DT, act_excess, dense_bound, locate, make_problem, one_hot_expected, one_hot_k,
                            out_channels, quick_gelu)

pytestmark = pytest.mark.gpu

SEGK_DT = {"fp32": 0, "bf16": 1}
NAN_BITS = {"bf16": 0x7FDE, "fp32": 0x7FDEAD00}      # quiet-NaN patterns: what the kernels must overwrite, and leave in the guards
BITS_DT = {"bf16": torch.int16, "fp32": torch.int32}
GUARD_ROWS = 64                                      # rows / pixels behind every output

_PARITY = {}                   # instance -> [worst error / bound, case id]
_ACT = {}                      # case id -> worst excess of the fp32 quick_gelu (gemm_reference.act_excess)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_GEMM_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            f.write("# worst error / bound of the dense float64 comparison per 1x1-geometry kernel instance of csrc/gemm.hip,\n"
                    "# csrc/convt_stream.hip and csrc/conv_igemm.hip (tests/test_gpu_gemm_matrix.py; wpc: waves that cover all channels):\n"
                    "# the largest over the output elements (split-K: of every part) against the derived any-order bound of\n"
                    "# tests/gemm_reference.py; the one-hot and lattice runs of every case are exact\n")
            for name in sorted(_PARITY):
                f.write(f"{name:46s} {_PARITY[name][0]:.4f}   {_PARITY[name][1]}\n")
            f.write("# fp32 quick_gelu of the device (v / (1 + __expf(-1.702 v))): worst |got - g(z)| - U_OUT |g(z)| - 1.1 e in units of\n"
                    f"# 2^-23 max(1, |z|) per fp32 act case (negative: 1.1 e alone covers it); gemm_reference.ACT_ULPS = {ACT_ULPS:g} is set from these\n")
            for cid in sorted(_ACT):
                f.write(f"{cid:46s} {_ACT[cid]:.4f}\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync(name):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a GPU fault is sticky: nothing more is started on the device in this session
        pytest.exit(f"{name}: the device reported {e}", returncode=3)


def out_shape(c):
    """(rows of the stored output, its channels, the shape the reference has)"""
    M = rows_of(c)
    Cp = out_channels(c)[0]
    if c.entry == "linear":
        return M, Cp, (M, Cp)
    if c.entry == "linear_splitk":
        return c.S * M, Cp, (c.S, M, Cp)
    if c.entry == "convt_fwd":
        return 4 * M, Cp, (c.B, 2 * c.H, 2 * c.W, Cp)
    return M, Cp, (c.B, c.H, c.W, Cp)


def run_gemm(lib, c, prob):
    """One call on fresh buffers -> the stored output on the CPU, in the reference's layout; the packed weights, the cover of
    the output and its guard are checked here."""
    dt, sdt, name = TORCH_DT[c.dtype], SEGK_DT[c.dtype], f"{instance_of(c)} {case_id(c)}"
    _, K, N, mode = gemm_view(c)
    p = lambda t: 0 if t is None else t.data_ptr()
    x, w = prob.x.cuda(), prob.w.contiguous().cuda()
    bias = None if prob.bias is None else prob.bias.cuda()
    wp = torch.full((K * N,), float("nan"), dtype=dt, device="cuda")
    if mode == 0:
        lib.call("segk_pack_conv_weight", p(w), p(wp), c.Lout, c.Lin, 0, c.Cout, c.Cin, 0, 1, 0, sdt, _stream())
    else:
        lib.call("segk_pack_convt_weight", p(w), p(wp), c.Lin, c.Lout, c.Cin, c.Cout, mode - 1, sdt, _stream())
    rows, Cp, shape = out_shape(c)
    out = torch.full((rows + GUARD_ROWS, Cp), NAN_BITS[c.dtype], dtype=BITS_DT[c.dtype], device="cuda")
    M = rows_of(c)
    if c.entry == "linear":
        lib.call("segk_linear", p(x), p(wp), p(bias), p(out), M, c.Cin, c.Cout, c.act, sdt, _stream())
    elif c.entry == "linear_splitk":
        lib.call("segk_linear_splitk", p(x), p(wp), p(bias), p(out), M, c.Cin, c.Cout, c.S, sdt, _stream())
    elif c.entry == "conv1x1":
        lib.call("segk_conv1x1", p(x), p(wp), p(bias), p(out), c.B, c.H, c.W, c.Cin, c.Cout, sdt, _stream())
    elif c.entry == "convt_fwd":
        lib.call("segk_convt2x2_fwd", p(x), p(wp), p(bias), p(out), c.B, c.H, c.W, c.Cin, c.Cout, sdt, _stream())
    else:
        lib.call("segk_convt2x2_dgrad", p(x), p(wp), p(out), c.B, c.H, c.W, c.Cin, c.Cout, sdt, _stream())
    _sync(name)
    assert not bool(torch.isnan(wp).any()), f"{name}: the pack left part of the packed weights unwritten"
    out = out.cpu()
    assert bool((out[rows:] == NAN_BITS[c.dtype]).all()), f"{name}: wrote behind the output"
    got = out[:rows].view(dt).reshape(shape)
    bad = torch.isnan(got.float()).nonzero()
    assert len(bad) == 0, f"{name}: {len(bad)} output elements were not written (or are NaN), first {locate(c, bad[0].tolist())[3]}"
    Cl = out_channels(c)[1]
    assert bool((got[..., Cl:].float() == 0).all()), f"{name}: padded output channels are not zero"
    return got


def describe(c, idx, got, want, one_hot):
    """the first differing elements: row or pixel, column, tap, and for the one-hot run the k of the row"""
    lines = []
    km = one_hot_k(c) if one_hot else None
    for i in idx[:12].tolist():
        m, n, tap, words = locate(c, i)
        s = f"  {words} (GEMM row {m}, column {n}) = {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}"
        if one_hot:
            k = int(km[m])
            s += f"; the row's 1.0 is at k={k}" + (f" (tap {k // c.Cout}, channel {k % c.Cout})" if c.entry == "convt_dgrad" else "")
        lines.append(s)
    return "\n".join(lines)


def assert_equal_outputs(c, run, got, want):
    got, want = got.float(), want.float()
    if torch.equal(got, want):
        return
    idx = (got != want).nonzero()
    raise AssertionError(f"{instance_of(c)} {case_id(c)} {run}: {len(idx)} outputs differ\n" + describe(c, idx, got, want, run == "one-hot"))


def test_device_has_the_compute_units_the_table_was_made_for(lib):
    """Row tile (256 | 320), units per workgroup and blocks per stream of the cases are evaluated for NUM_CUS compute units: on
    another device the table would silently test other instances and no unit boundary."""
    assert torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count == NUM_CUS


@pytest.mark.parametrize("shape", [(128, 256, 128, 1), (128, 256, 128, 2), (128, 256, 128, 4), (128, 256, 128, 3), (128, 256, 128, 8),
                                   (128, 512, 128, 8), (128, 192, 128, 3), (128, 192, 128, 1), (112, 256, 128, 2), (128, 256, 192, 2),
                                   (128, 288, 128, 1), (120, 256, 128, 1), (272, 768, 256, 3), (272, 768, 256, 4), (272, 768, 256, 5),
                                   (272, 768, 256, 6), (272, 768, 256, 12), (272, 768, 256, 24), (128, 256, 128, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_linear_splitk_refuses_exactly_what_the_mirror_refuses(lib, shape):
    M, K, N, S = shape
    x = torch.zeros((max(M, 16), K), dtype=torch.bfloat16, device="cuda")
    wp = torch.zeros((K * N,), dtype=torch.bfloat16, device="cuda")
    out = torch.zeros((max(S, 1) * max(M, 16) + GUARD_ROWS, N), dtype=torch.bfloat16, device="cuda")
    args = (x.data_ptr(), wp.data_ptr(), 0, out.data_ptr(), M, K, N, S, SEGK_DT["bf16"], _stream())
    if splitk_ok(M, K, N, S):
        lib.call("segk_linear_splitk", *args)
        _sync(f"segk_linear_splitk {shape}")
        assert float(out.float().abs().max()) == 0.0
    else:
        with pytest.raises(RuntimeError):
            lib.call("segk_linear_splitk", *args)
    with pytest.raises(RuntimeError, match="bf16"):
        lib.call("segk_linear_splitk", *args[:8], SEGK_DT["fp32"], _stream())


_EXACT = [c for c in CASES if not c.act] + LONG_CASES


@pytest.mark.parametrize("case", _EXACT, ids=case_id)
def test_one_hot_is_exact(lib, case):
    c, dt = case, TORCH_DT[case.dtype]
    prob = make_problem(c, "one-hot")
    z = one_hot_expected(prob, torch.float32)          # multiples of 1/64 up to 2: exact in fp32 and in bf16
    assert_equal_outputs(c, "one-hot", run_gemm(lib, c, prob), z.to(dt))


@pytest.mark.parametrize("case", _EXACT, ids=case_id)
def test_lattice_is_exact(lib, case):
    c, dt = case, TORCH_DT[case.dtype]
    prob = make_problem(c, "lattice")
    z = prob.fast_reference()            # fp32 on the CPU: exact on these inputs (tests/test_gemm_reference_host.py)
    assert_equal_outputs(c, "lattice", run_gemm(lib, c, prob), z.to(dt))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dense_against_float64(lib, case):
    c = case
    prob = make_problem(c, "dense")
    z, A = prob.reference(), prob.abs_reference()
    bound = dense_bound(c, z, A)
    want = quick_gelu(z) if c.act else z
    got = run_gemm(lib, c, prob).double()
    name = f"{instance_of(c)} {case_id(c)}"
    if c.act and c.dtype == "fp32":
        _ACT[case_id(c)] = act_excess(c, got, z, A)
        print(f"{name}: fp32 quick_gelu excess = {_ACT[case_id(c)]:.4f} x 2^-23 max(1, |z|)")
    live = bound > 0                      # padded channels: reference and bound are zero, checked in run_gemm
    ratio = ((got - want).abs()[live] / bound[live]).max().item()
    print(f"{name}: error / bound = {ratio:.4f}")
    inst = instance_of(c)
    if inst not in _PARITY or ratio > _PARITY[inst][0]:
        _PARITY[inst] = [ratio, case_id(c)]
    assert ratio <= 1.0, f"{name}: the error is {ratio:.3f} x the bound"
    if c.entry == "linear_splitk":          # the consumer's sum of the parts: within the sum of the bounds
        assert bool(((got.sum(0) - z.sum(0)).abs() <= bound.sum(0)).all()), name
