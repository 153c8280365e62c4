"""CPU: the float64 restatement the 1x1-geometry GPU matrix is compared with (tests/gemm_reference.py) against torch's own
F.linear, F.conv2d(k=1), F.conv_transpose2d(stride=2) and its autograd data gradient in float64; the selection form of the
one-hot expectation against the reference; and the properties the exact lattice run relies on."""
import pytest
import torch
import torch.nn.functional as F

from gemm_cases import CASES, LONG_CASES, REF_MADD_CAP, case_id, gemm_view, ref_madds, rows_of
from gemm_reference import (ACT_ULPS, conv1x1, convt2x2, convt2x2_dgrad, dense_bound, k_order, k_positions, linear, locate,
                            make_problem, one_hot_expected, one_hot_k, quick_gelu)

SHAPES = [(2, 5, 7, 6, 10), (1, 1, 1, 3, 4), (3, 2, 16, 8, 5)]          # B, H, W, Cin, Cout


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_torch_float64(shape):
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1
    x, w, b = r(B, H, W, Ci), r(Co, Ci), r(Co)
    assert (linear(x.reshape(-1, Ci), w, b) - F.linear(x.reshape(-1, Ci), w, b)).abs().max().item() < 1e-13
    ref = F.conv2d(x.permute(0, 3, 1, 2), w[:, :, None, None], b).permute(0, 2, 3, 1)
    assert (conv1x1(x, w, b) - ref).abs().max().item() < 1e-13
    wt = r(Ci, Co, 2, 2)
    xr = x.clone().requires_grad_(True)
    ref = F.conv_transpose2d(xr.permute(0, 3, 1, 2), wt, b, stride=2).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (B, 2 * H, 2 * W, Co)
    assert (convt2x2(x, wt, b) - ref).abs().max().item() < 1e-13
    gz = r(B, 2 * H, 2 * W, Co)
    (ref * gz).sum().backward()
    assert (convt2x2_dgrad(gz, wt) - xr.grad).abs().max().item() < 1e-13
    z = r(64)
    assert (quick_gelu(4 * z) - 4 * z / (1 + torch.exp(-1.702 * 4 * z))).abs().max().item() < 1e-14


def _pick(entry, **kw):
    return next(c for c in CASES if c.entry == entry and ref_madds(c) < 10 ** 8 and rows_of(c) > 16
                and all(getattr(c, k) == v for k, v in kw.items()))


_SMALL = [_pick("linear", dtype="bf16", bias=True, act=0), _pick("linear", dtype="fp32", bias=True, act=0),
          next(c for c in CASES if c.entry == "linear" and c.Lin < c.Cin), _pick("linear_splitk", S=3), _pick("linear_splitk", S=2, bias=True),
          _pick("conv1x1", dtype="bf16", bias=True), next(c for c in CASES if c.entry == "conv1x1" and c.Lout < c.Cout and c.bias),
          _pick("convt_fwd", dtype="bf16", bias=True), _pick("convt_fwd", dtype="fp32", bias=False),
          next(c for c in CASES if c.entry == "convt_fwd" and c.Lout < c.Cout and c.bias),
          _pick("convt_dgrad", dtype="bf16"), _pick("convt_dgrad", dtype="fp32"),
          next(c for c in CASES if c.entry == "convt_dgrad" and c.Lout < c.Cout)]


@pytest.mark.parametrize("case", _SMALL, ids=case_id)
def test_problem_reference_equals_the_layer_on_its_logical_channels(case):
    """Problem.reference() over the padded channels against the layer functions on the logical ones"""
    c = case
    p = make_problem(c, "dense")
    z = p.reference()
    x, w = p.x.double(), p.w.double()
    if c.entry.startswith("convt"):
        b = None if p.bias is None else p.bias.double()[:c.Lout]
        if c.entry == "convt_fwd":
            want = F.conv_transpose2d(x[..., :c.Lin].permute(0, 3, 1, 2), w, b, stride=2).permute(0, 2, 3, 1)
            lo = c.Lout
        else:
            want, lo = convt2x2_dgrad(x[..., :c.Lout], w), c.Lin
            xr = torch.zeros((c.B, c.Lin, c.H, c.W), dtype=torch.float64, requires_grad=True)
            (F.conv_transpose2d(xr, w, stride=2) * x[..., :c.Lout].permute(0, 3, 1, 2)).sum().backward()
            assert (want - xr.grad.permute(0, 2, 3, 1)).abs().max().item() < 1e-11
    else:
        b = None if p.bias is None else p.bias.double()[:c.Lout]
        full = F.linear(x[..., :c.Lin], w, b)
        lo = c.Lout
        if c.entry == "linear_splitk":
            assert tuple(z.shape) == (c.S, rows_of(c), c.Cout)
            first = F.linear(x[..., :c.Cin // c.S], w[:, :c.Cin // c.S], b)
            assert (z[0] - first).abs().max().item() < 1e-11
            z = z.sum(0)
        want = full
    assert (z[..., :lo] - want).abs().max().item() < 1e-11
    assert float(z[..., lo:].abs().max()) == 0.0 if lo < z.shape[-1] else True
    # the bound is positive wherever a logical channel is, and loose enough for the rounding of the output alone
    bound = dense_bound(c, p.reference(), p.abs_reference())
    assert bool((bound[..., :lo] > 0).all())


@pytest.mark.parametrize("case", _SMALL, ids=case_id)
def test_one_hot_selection_equals_the_reference(case):
    c = case
    p = make_problem(c, "one-hot")
    z = one_hot_expected(p)
    assert torch.equal(z, p.reference())
    assert torch.equal(one_hot_expected(p, torch.float32).double(), z)
    A, Wg, _ = p.gemm_operands()
    assert bool((A.sum(1) == 1).all() and (A.max(1).values == 1).all() and (A.min() == 0))
    assert torch.equal(A.argmax(1), one_hot_k(c))
    assert bool((Wg * 64 == (Wg * 64).round()).all()) and float(Wg.abs().max()) <= 1.0
    if c.entry == "convt_dgrad":          # one (tap, channel) of the 2 x 2 block: the other three pixels are zero
        blocks = p.x.double().reshape(c.B, c.H, 2, c.W, 2, c.Cout).abs().sum(-1).permute(0, 1, 3, 2, 4).reshape(-1, 4)
        assert bool(((blocks > 0).sum(1) == 1).all())
    # locate() names the GEMM row and column of a stored element
    idx = (z != 0).nonzero()[-1]
    m, n, tap, words = locate(c, idx.tolist())
    full = (p._product(A, Wg, None) if c.entry != "linear_splitk" else torch.matmul(A, Wg))
    assert float(full[m, n]) == float(Wg[int(one_hot_k(c)[m]), n]) and words


def test_one_hot_walks_every_logical_k():
    for c in CASES + LONG_CASES:
        order, ks = k_order(c), k_positions(c)
        assert sorted(order) == sorted(ks) and len(set(order)) == len(order)
        M = rows_of(c)
        hit = set(one_hot_k(c).tolist())
        edge = {k for k in ks if k % 32 in (0, 31)} | {ks[-1]}
        if M >= len(ks):
            assert hit == set(ks), case_id(c)
        elif M >= len(edge):          # a short problem reaches at least the chunk edges and the last logical k
            assert edge <= hit, case_id(c)
        assert max(hit) < gemm_view(c)[1]
    # the table holds, per entry, a case whose rows reach every k
    for e in ("linear", "linear_splitk", "conv1x1", "convt_fwd", "convt_dgrad"):
        assert any(c.entry == e and rows_of(c) >= len(k_positions(c)) for c in CASES), e


@pytest.mark.timeout(900)
def test_lattice_preconditions_and_reference_sizes():
    """2 K < 2^24: every partial sum of K products (multiples of 1/2, at most 1 each) and the bias is exact in fp32 in any order;
    the lattice reference reaches |z| >= 1 and its operands are not degenerate; fp32 equals float64 bit for bit on it.  The dense
    float64 references stay under the cap (the LONG_CASES take the exact runs only)."""
    for c in CASES + LONG_CASES:
        assert 2 * gemm_view(c)[1] + 4 < 2 ** 24
    for c in CASES:
        assert ref_madds(c) <= REF_MADD_CAP, case_id(c)
    for c in CASES + LONG_CASES:
        if c.act:          # dense only
            continue
        p = make_problem(c, "lattice")
        A, Wg, _ = p.gemm_operands(torch.float32)
        assert bool(((A == A.round()) & (A.abs() <= 1)).all() and ((2 * Wg == (2 * Wg).round()) & (Wg.abs() <= 1)).all())
        z32 = p.fast_reference()
        assert z32.dtype == torch.float32 and float(z32.abs().max()) >= 1.0, case_id(c)
        assert 0.2 < float((p.x != 0).float().mean()) < 0.8, case_id(c)
        if ref_madds(c) <= 10 ** 8:
            assert torch.equal(z32.double(), p.reference()), case_id(c)


def test_act_constant_is_a_power_of_two():
    assert ACT_ULPS >= 1 and 2.0 ** round(torch.log2(torch.tensor(ACT_ULPS)).item()) == ACT_ULPS
