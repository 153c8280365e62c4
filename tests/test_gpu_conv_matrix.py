"""GPU (-m gpu): every reachable 3x3 instance of the convolution forward / data-gradient kernels (csrc/conv_igemm.hip,
csrc/conv_pipe.hip, csrc/conv_ws.hip, csrc/conv_rs.hip) through the C ABI (segk_conv3x3, segk_conv3x3_act), one case table (tests/conv_cases.py;
tests/test_conv_instances.py proves on the CPU that it reaches all of them), three runs per case against
tests/conv_reference.py.

The test owns every buffer: outputs and act_out are pre-filled with a NaN pattern and followed by a guard of NaN rows that
must stay untouched; the statistics buffer holds segk_bn_stats_floats(tiles, Cp) floats of NaN, all tiles * Cp * 2 partials
must come back finite and the guard behind the allocation untouched; padded output channels must be exactly zero.
tiles_of() and writes_act() of the Python mirror are cross-checked against the ABI queries for every case.

  impulse: the input is zero except 1.0 at the probes (corners, edges, both sides of every tile boundary, the last partial
           tile, the image boundary), in as many passes as needed so that no output pixel receives two non-zero products;
           weights are multiples of 1/64.  Every output must EQUAL one weight (plus the bias) or zero -- the zeros everywhere
           else included -- and the statistics totals, summed in float64 over the rows, must equal the reference exactly: a
           wrong, missing or wrapped tap, a leaking halo, a dropped or doubled pixel names its instance, probe, tap and channel.
           With the prologue the activation is exactly 1.0 on the probes and 0 elsewhere while relu(shift) = 0.5 on three
           channels of four: a halo that is transformed instead of zeroed shows up.
  lattice: x in {-1, 0, 1}, w in {-1, -1/2, 0, 1/2, 1}, dense: every partial sum in any order is exact in fp32, so outputs
           must equal the reference rounded to `dtype` and the statistics totals the reference's, exactly.  A skipped K chunk,
           a ring-parity slip at a unit boundary or a wrong second source cannot hide behind an accumulation order.  The cases
           with three or more work units per workgroup (LONG_CASES) take this run only.
  dense:   operands uniform in [-1, 1] rounded to `dtype`, float64 reference on the exact operands, the derived any-order bound
           of conv_reference.py.  Loose on purpose: the two exact runs carry the sharpness.
Equality is numerical equality of every element (NaN equals nothing; -0 equals 0).
Set SEGK_CONV_PARITY_OUT=<file> to record the worst error / bound per instance (profiles/conv_matrix_parity.txt)."""
import os

import pytest
import torch

from conv_cases import (CASES, LONG_CASES, case_id, instance_of, logical_of, probe_passes, tiles_of, writes_act)
from conv_reference import TORCH_DT, channel_stats, dense_bounds, impulse_expected, make_problem

pytestmark = pytest.mark.gpu

SEGK_DT = {"fp32": 0, "bf16": 1}
NAN_BITS = {"bf16": 0x7FDE, "fp32": 0x7FDEAD00}      # quiet-NaN patterns: what the kernels must overwrite, and leave in the guards
BITS_DT = {"bf16": torch.int16, "fp32": torch.int32}
GUARD_ROWS = 64                                      # pixels behind every output
GUARD_FLOATS = 4096                                  # floats behind the statistics buffer

_PARITY = {}                   # instance -> [worst error / bound, what, case id]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_CONV_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            f.write("# worst error / bound of the dense float64 comparison per 3x3 kernel instance of csrc/conv_igemm.hip and\n"
                    "# csrc/conv_rs.hip (tests/test_gpu_conv_matrix.py): the largest of the output elements and of the statistics\n"
                    "# totals (sum, sumsq), each against its derived any-order bound (tests/conv_reference.py); the impulse and\n"
                    "# lattice runs of every case are exact\n")
            for name in sorted(_PARITY):
                f.write(f"{name:46s} {_PARITY[name][0]:.4f}   {_PARITY[name][1]:6s} {_PARITY[name][2]}\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Result:
    pass


def run_conv(lib, c, prob):
    """One call on fresh buffers -> outputs [B,H,W,CO1+CO2], act_out, statistics rows [tiles][Np][2], all on the CPU; the guards
    and the cover of the statistics buffer are checked here."""
    dt, name = TORCH_DT[c.dtype], f"{instance_of(c)} {case_id(c)}"
    P, N, sdt = c.B * c.H * c.W, c.CO1 + c.CO2, SEGK_DT[c.dtype]
    p = lambda t: 0 if t is None else t.data_ptr()
    # the mirror of the dispatch against the ABI's own queries
    tiles = lib.query("segk_conv_tiles", c.B, c.H, c.W, c.CA + c.CB, N, sdt)
    assert tiles == tiles_of(c), f"{name}: segk_conv_tiles = {tiles}, the mirror says {tiles_of(c)}"
    assert bool(lib.query("segk_conv_writes_act_q", c.CA + c.CB, N, sdt)) == bool(writes_act(c.CA + c.CB, N, c.dtype)), name
    d = [None if t is None else t.cuda() for t in (prob.xa, prob.xb, prob.w.contiguous(), prob.bias, prob.scale, prob.shift)]
    xa, xb, w, bias, scale, shift = d
    wp = torch.full(((c.CA + c.CB) * 9 * N,), float("nan"), dtype=dt, device="cuda")
    lib.call("segk_pack_conv_weight", p(w), p(wp), *prob.pack_args, 9, c.mode, sdt, _stream())

    def nan_buffer(rows, C):
        return torch.full((rows + GUARD_ROWS, C), NAN_BITS[c.dtype], dtype=BITS_DT[c.dtype], device="cuda")
    o1, o2 = nan_buffer(P, c.CO1), (nan_buffer(P, c.CO2) if c.CO2 else None)
    act = nan_buffer(P, c.CA) if c.act_out else None
    st = None
    if c.stats:
        nst = lib.query("segk_bn_stats_floats", tiles, N)
        assert nst >= tiles * N * 2, name
        st = torch.full((nst + GUARD_FLOATS,), NAN_BITS["fp32"], dtype=torch.int32, device="cuda")
    if c.act_out:
        lib.call("segk_conv3x3_act", p(xa), p(wp), p(scale), p(shift), p(o1), p(act), p(st), c.B, c.H, c.W, c.CA, c.CO1, sdt,
                 _stream())
    else:
        lib.call("segk_conv3x3", p(xa), p(xb), p(wp), p(bias), p(scale), p(shift), p(o1), p(o2), p(st), c.B, c.H, c.W, c.CA, c.CB,
                 c.CO1, c.CO2, sdt, _stream())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a GPU fault is sticky: nothing more is started on the device in this session
        pytest.exit(f"{name}: the device reported {e}", returncode=3)
    r = Result()
    outs = []
    for what, buf in (("out", o1), ("out2", o2), ("act_out", act)):
        if buf is None:
            continue
        buf = buf.cpu()
        assert bool((buf[P:] == NAN_BITS[c.dtype]).all()), f"{name}: wrote behind {what}"
        outs.append((what, buf[:P].view(dt).reshape(c.B, c.H, c.W, -1)))
    r.out = torch.cat([t for what, t in outs if what != "act_out"], dim=3)
    r.act = outs[-1][1] if c.act_out else None
    r.rows = None
    if c.stats:
        st = st.cpu()
        assert bool((st[nst:] == NAN_BITS["fp32"]).all()), f"{name}: wrote behind the statistics buffer"
        r.rows = st[:tiles * N * 2].view(torch.float32).reshape(tiles, N, 2)
        bad = (~torch.isfinite(r.rows)).nonzero()
        assert len(bad) == 0, f"{name}: {len(bad)} of the {tiles} x {N} x 2 statistics partials were not written, first (row, channel, " \
                              f"which) = {bad[0].tolist()}"
    return r


def padded_channels(c):
    _, _, lo1, lo2 = logical_of(c)
    return list(range(lo1, c.CO1)) + list(range(c.CO1 + lo2, c.CO1 + c.CO2))


def describe(c, idx, got, want, probes=None, reached=None):
    """the first differing elements: pixel, channel, and for the impulse run the probe and the tap that reach the pixel"""
    lines = []
    for b, y, x, n in idx[:12].tolist():
        s = f"  out[b={b}, y={y}, x={x}, n={n}] = {got[b, y, x, n].item()!r}, want {want[b, y, x, n].item()!r}"
        if probes is not None:
            i = int(reached[b, y, x])
            if i >= 0:
                pb, py, px, pk = probes[i]
                s += f"; probe (b,y,x,k)=({pb},{py},{px},{pk}) through tap (ty,tx)=({py - y + 1},{px - x + 1})"
            else:
                s += "; no probe reaches this pixel"
        lines.append(s)
    return "\n".join(lines)


def assert_equal_outputs(c, run, got, want, probes=None, reached=None, what="outputs"):
    got, want = got.float(), want.float()
    if torch.equal(got, want):
        return
    idx = ((got != want) | torch.isnan(got)).nonzero()
    raise AssertionError(f"{instance_of(c)} {case_id(c)} {run}: {len(idx)} {what} differ\n" + describe(c, idx, got, want, probes, reached))


def assert_exact_stats(c, run, rows, z):
    """the rows summed in float64 against the reference's totals, exactly (every partial sum is exact in fp32 by construction)"""
    tot = rows.double().sum(0)
    s1, s2 = channel_stats(z)
    for j, (ref, what) in enumerate(((s1, "sum"), (s2, "sumsq"))):
        bad = (tot[:, j] != ref).nonzero().flatten().tolist()
        assert not bad, f"{instance_of(c)} {case_id(c)} {run}: {what} of {len(bad)} channels differs, first n={bad[0]}: " \
                        f"{tot[bad[0], j].item()!r}, want {ref[bad[0]].item()!r} (a dropped or doubled pixel?)"


def assert_padding_is_zero(c, out):
    pad = padded_channels(c)
    if pad:
        assert bool((out[..., pad].float() == 0).all()), f"{instance_of(c)} {case_id(c)}: padded output channels are not zero"


def check_act(c, run, r, prob):
    if c.act_out:
        assert_equal_outputs(c, run, r.act, prob.activation()[..., :c.CA], what="act_out elements")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_impulse_is_exact(lib, case):
    c, dt = case, TORCH_DT[case.dtype]
    for probes in probe_passes(c):
        prob = make_problem(c, "impulse", probes)
        z, reached = impulse_expected(prob, probes)
        r = run_conv(lib, c, prob)
        assert_equal_outputs(c, "impulse", r.out, z.float().to(dt), probes, reached)
        assert_padding_is_zero(c, r.out)
        check_act(c, "impulse", r, prob)
        if c.stats:
            assert_exact_stats(c, "impulse", r.rows, z)


@pytest.mark.parametrize("case", CASES + LONG_CASES, ids=case_id)
def test_lattice_is_exact(lib, case):
    c, dt = case, TORCH_DT[case.dtype]
    prob = make_problem(c, "lattice")
    z = prob.fast_reference()            # fp32 on the CPU: exact on these inputs (tests/test_conv_reference_host.py)
    r = run_conv(lib, c, prob)
    assert_equal_outputs(c, "lattice", r.out, z.to(dt))
    assert_padding_is_zero(c, r.out)
    check_act(c, "lattice", r, prob)
    if c.stats:
        assert_exact_stats(c, "lattice", r.rows, z)


def record(c, ratio, what):
    name = instance_of(c)
    if name not in _PARITY or ratio > _PARITY[name][0]:
        _PARITY[name] = [ratio, what, case_id(c)]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dense_against_float64(lib, case):
    c = case
    prob = make_problem(c, "dense")
    z, A = prob.reference(), prob.abs_reference()
    b_out, b_sum, b_sq = dense_bounds(c, z, A)
    r = run_conv(lib, c, prob)
    name = f"{instance_of(c)} {case_id(c)}"
    assert bool(torch.isfinite(r.out.float()).all()), f"{name}: non-finite output"
    assert_padding_is_zero(c, r.out)
    check_act(c, "dense", r, prob)
    live = b_out > 0                      # padded channels: reference and bound are zero, checked above
    ratios = {"out": ((r.out.double() - z).abs()[live] / b_out[live]).max().item()}
    if c.stats:
        tot = r.rows.double().sum(0)
        s1, s2 = channel_stats(z)
        for what, got, ref, bound in (("sum", tot[:, 0], s1, b_sum), ("sumsq", tot[:, 1], s2, b_sq)):
            ok = bound > 0
            ratios[what] = ((got - ref).abs()[ok] / bound[ok]).max().item()
            assert bool((got[~ok] == 0).all()), f"{name}: {what} of a padded channel is not zero"
    print(f"{name}: error / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        record(c, v, k)
    for k, v in ratios.items():
        assert v <= 1.0, f"{name}: {k} error is {v:.3f} x the bound"
