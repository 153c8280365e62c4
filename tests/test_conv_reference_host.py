"""CPU: the float64 restatement of the 3x3 convolution the GPU matrix is compared with (tests/conv_reference.py) against
torch's own conv2d / conv_transpose2d in float64, the placement form of the impulse expectation against it, and the property
the exact lattice run relies on: on lattice inputs the CPU's fp32 convolution equals the float64 one bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from conv_cases import CASES, case_id, probe_passes
from conv_reference import (channel_stats, conv3x3, conv3x3_transposed, impulse_expected, make_problem, prologue,
                            stats_are_exact)

SHAPES = [(2, 5, 7, 6, 10), (1, 1, 1, 3, 4)]          # B, H, W, Cin, Cout


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_torch_float64(shape):
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(7)
    x = torch.rand((B, H, W, Ci), generator=g, dtype=torch.float64) * 2 - 1
    w = torch.rand((Co, Ci, 3, 3), generator=g, dtype=torch.float64) * 2 - 1
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    assert (conv3x3(x, w) - ref).abs().max().item() < 1e-13
    gz = torch.rand((B, H, W, Co), generator=g, dtype=torch.float64) * 2 - 1
    ref = F.conv_transpose2d(gz.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    assert (conv3x3_transposed(gz, w) - ref).abs().max().item() < 1e-13
    # the transposed form is the data gradient of the forward form
    xr = x.clone().requires_grad_(True)
    (conv3x3(xr, w) * gz).sum().backward()
    assert (conv3x3_transposed(gz, w) - xr.grad).abs().max().item() < 1e-13
    s1, s2 = channel_stats(gz)
    assert torch.equal(s1, gz.reshape(-1, Co).sum(0)) and torch.equal(s2, (gz * gz).reshape(-1, Co).sum(0))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_prologue_is_one_fused_multiply_add(dtype):
    g = torch.Generator().manual_seed(3)
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    z = (torch.rand((4096, 8), generator=g) * 4 - 2).to(dt)
    sc, sh = torch.rand((8,), generator=g) * 3 - 1.5, torch.rand((8,), generator=g) - 0.5
    exact = torch.clamp(z.double() * sc.double() + sh.double(), min=0)      # float64: 53 bits hold the fp32 product exactly
    got = prologue(z, sc, sh, dtype)
    assert got.dtype == dt
    # correctly rounded: no other value of `dtype` is nearer to the exact result
    ulp = torch.where(exact > 0, 2.0 ** (torch.floor(torch.log2(exact.clamp(min=1e-30))) - (7 if dtype == "bf16" else 23)), 0.0)
    assert bool(((got.double() - exact).abs() <= 0.5 * ulp * (1 + 2.0 ** -20)).all())


_SMALL = [c for c in CASES if c.B * c.H * c.W <= 16 * 17 * 2]


@pytest.mark.parametrize("case", [next(c for c in _SMALL if c.mode == m and bool(c.CB) == cb and c.prologue == p)
                                  for m, cb, p in ((0, True, False), (1, True, False), (0, False, True), (1, False, True))], ids=case_id)
def test_impulse_placement_equals_the_reference(case):
    for probes in probe_passes(case):
        prob = make_problem(case, "impulse", probes)
        z, reached = impulse_expected(prob, probes)
        assert torch.equal(z, prob.reference())
        assert int((reached >= 0).sum()) >= len(probes)
        act = prob.activation().double()
        assert float(act.sum()) == len(probes) and float(act.max()) == 1.0 and float(act.min()) == 0.0


@pytest.mark.parametrize("case", [next(c for c in _SMALL if c.mode == m and c.dtype == d and c.prologue == p and c.bias == b)
                                  for m, d, p, b in ((0, "bf16", False, False), (1, "bf16", True, True), (1, "fp32", False, True),
                                                     (0, "fp32", True, False))], ids=case_id)
def test_lattice_fp32_equals_float64_bit_for_bit(case):
    prob = make_problem(case, "lattice")
    act = prob.activation().double()
    assert set(act.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(prob.w.unique().tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    z64, z32 = prob.reference(), prob.fast_reference()
    assert z32.dtype == torch.float32 and torch.equal(z32.double(), z64)
    assert float(z64.abs().max()) > 1.0 and stats_are_exact(z64, 0.5)
