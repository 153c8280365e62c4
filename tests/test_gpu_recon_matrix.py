"""GPU (-m gpu): the entries of csrc/recon.hip -- segk_recon_head_fwd, segk_recon_sigmoid_bwd, segk_mse_fwd, segk_mse_bwd --
through the C ABI against the restatements of tests/recon_reference.py, on its case tables
(tests/test_recon_prompt_cases_host.py proves on the CPU that the restatements are right, that the tables reach every chunk,
pair and launch regime they claim, and that a dropped channel, tap or bias cannot hide inside the forward bound).

Inputs are built on the CPU with oracle.fill; padding channels of every act tensor are zero; every output is pre-filled with a
NaN pattern and followed by a guard of the same pattern: after the call every element must be overwritten and the guard
untouched.

  head forward    |rec - rec64| <= gamma_m S / 4 + 4 d_sig per output (recon_reference's docstring derives it; neither term is
                  tuned to the device); zero weights and a bias of +-40, +-90, +-104 give float32 sigmoid's saturation values
                  exactly: finite, 0 at -90 and -104, 1 at +104.
  sigmoid bwd     bit-equal to g * (1 - r) * r in float32 rounded to the dtype; padding channels exactly +0.
  mse forward     within one float32 ulp of the exactly rounded sum (only the final rounding can differ), bit-identical on a
                  second run, exactly 2 * mse_blocks(n) floats of `part` written; the refusals launch nothing.
  mse backward    da and db bit-equal to ATen's rounding.

Measured on an MI355X (SEGK_RECON_PARITY_OUT=<file> writes the record, profiles/recon_matrix_parity.txt):
  head forward    worst error / bound 0.1404 in fp32 (1x1x1, Cin 3, Cout 4, no bias) and 0.1779 in bf16 (1x31x65, Cin 1, Cout 8,
                  no bias); at 31 channels and more at most 0.011.  The small-Cin cells lead because there the bound is mostly
                  the sigmoid term, 4 d_sig of about 6e-8 each.
  mse forward     0 ulp at every n, mean and sum: the device's float32 equals the exactly rounded sum's.
The other gates are equalities."""
import os

import numpy as np
import pytest
import torch

import recon_reference as R
from matrix_helpers import (NAN_BITS, SEGK_DT, assert_identical, assert_within, make_recorder, nan_buffer, ptr, stream, sync,
                            take, write_parity)
from oracle.fill import fill

pytestmark = pytest.mark.gpu

_PARITY, record = make_recorder()


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_RECON_PARITY_OUT")
    if out and _PARITY:
        write_parity(out, _PARITY, "# worst error / bound per entry of tests/test_gpu_recon_matrix.py (bounds derived in\n"
                                   "# tests/recon_reference.py); the pass condition is ratio <= 1\n")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def run_head(lib, xa, w, b, c, what):
    n = c.B * c.Cout * c.H * c.W
    rec = nan_buffer(n, "fp32")
    xd, wd, bd = xa.cuda(), w.cuda(), None if b is None else b.cuda()
    lib.call("segk_recon_head_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(rec), c.B, c.H, c.W, c.Cp, c.Cin, c.Cout, SEGK_DT[c.dtype], stream())
    sync(what)
    return take(rec, n, "fp32", what).reshape(c.B, c.Cout, c.H, c.W)


# ---- segk_recon_head_fwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_case_id)
def test_head_forward_within_the_derived_bound(lib, case):
    c, what = case, f"segk_recon_head_fwd {R.head_case_id(case)}"
    xa, w, b = R.head_inputs(c)
    rec64, S, z = R.head(xa, w, b, c.dtype)
    got = run_head(lib, xa, w, b, c, what)
    record(f"recon_head_fwd {c.dtype}", assert_within(got, rec64, R.head_bound(S, z, c.Cin), what), R.head_case_id(c))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("bias", R.SATURATION_BIASES)
def test_head_saturation_is_float32_sigmoids(lib, dtype, bias):
    c = R.HeadCase(dtype, 2, 9, 21, 17, 32, 3, True, 300)
    xa, _, _ = R.head_inputs(c)
    got = run_head(lib, xa, torch.zeros((c.Cout, c.Cin, 3, 3)), torch.full((c.Cout,), bias), c, f"segk_recon_head_fwd {dtype} bias {bias}")
    want = float(R.saturation([bias])[0])
    assert bool(torch.isfinite(got).all()) and bool((got == want).all()), (bias, got.flatten()[:4].tolist(), want)
    if bias <= -90:
        assert want == 0.0
    if bias >= 104:
        assert want == 1.0


# ---- segk_recon_sigmoid_bwd ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", R.SIGMOID_BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sigmoid_backward_is_the_restatement(lib, shape, dtype):
    B, H, W = shape
    for C, Cp in R.SIGMOID_BWD_CHANNELS:
        what = f"segk_recon_sigmoid_bwd {dtype} {B}x{H}x{W} C={C} Cp={Cp}"
        drec, rec = fill((B, C, H, W), 9 + C, -1, 1), fill((B, C, H, W), 10 + C, 0, 1)
        n = B * H * W * Cp
        dz = nan_buffer(n, dtype)                    # padding channels hold NaN before the call
        dd, rd = drec.cuda(), rec.cuda()
        lib.call("segk_recon_sigmoid_bwd", ptr(dd), ptr(rd), ptr(dz), B, H, W, C, Cp, SEGK_DT[dtype], stream())
        sync(what)
        got = take(dz, n, dtype, what).reshape(B, H, W, Cp)
        assert_identical(bits(got), bits(R.sigmoid_bwd(drec, rec, Cp, dtype)), what)
        assert not bits(got[..., C:]).any(), f"{what}: padding channels are not +0"


# ---- segk_mse_fwd ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def master(lib):
    a, b = R.mse_master()
    return a, b, a.cuda(), b.cuda()


def run_mse_fwd(lib, ad, bd, n, mean, what, part_floats=1024):
    part, out = nan_buffer(1024, "fp32"), nan_buffer(1, "fp32")
    lib.call("segk_mse_fwd", ptr(ad), ptr(bd), ptr(part), part_floats, ptr(out), n, mean, stream())
    sync(what)
    return part, out


@pytest.mark.parametrize("n", R.MSE_FWD_N)
def test_mse_forward_within_one_ulp_and_deterministic(lib, master, n):
    a, b, ad, bd = master
    total = R.mse_master_sum(n)
    nb = R.mse_blocks(n)
    for mean in (1, 0):
        what = f"segk_mse_fwd n={n} {'mean' if mean else 'sum'}"
        part, out = run_mse_fwd(lib, ad, bd, n, mean, what)
        p = part.cpu()
        assert bool((p[:2 * nb] != NAN_BITS["fp32"]).all()), f"{what}: a partial of the {nb} was not written"
        assert bool((p[2 * nb:] == NAN_BITS["fp32"]).all()), f"{what}: wrote behind the {2 * nb} floats of part"
        got = take(out, 1, "fp32", what)
        want = R.mse(a[:n], b[:n], mean, total)
        ulps = abs(float(got[0]) - float(want)) / float(np.spacing(want))
        print(f"{what}: {ulps:.2f} ulp")
        record(f"mse_fwd {'mean' if mean else 'sum'} (ulp)", ulps, f"n={n}")
        assert bool(torch.isfinite(got).all()) and ulps <= 1.0, (what, float(got[0]), float(want))
        part2, out2 = run_mse_fwd(lib, ad, bd, n, mean, what + " again")
        assert torch.equal(out2, out) and torch.equal(part2, part), f"{what}: two runs differ"


def test_mse_forward_refusals_launch_nothing(lib, master):
    _, _, ad, bd = master
    n = 4097                                         # two workgroups: four floats of part
    for kw, n_, mean in ((dict(part_floats=3), n, 1), (dict(), n, 2), (dict(), 0, 1)):
        part, out = nan_buffer(1024, "fp32"), nan_buffer(1, "fp32")
        with pytest.raises(RuntimeError, match="mse_fwd"):
            lib.call("segk_mse_fwd", ptr(ad), ptr(bd), ptr(part), kw.get("part_floats", 1024), ptr(out), n_, mean, stream())
        sync("segk_mse_fwd refusal")
        assert bool((part.cpu() == NAN_BITS["fp32"]).all()) and bool((out.cpu() == NAN_BITS["fp32"]).all())
    run_mse_fwd(lib, ad, bd, n, 1, "segk_mse_fwd part_floats=4", part_floats=4)          # exactly enough is accepted


# ---- segk_mse_bwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.MSE_BWD_N)), ids=lambda i: f"n{R.MSE_BWD_N[i]}")
def test_mse_backward_is_atens_rounding(lib, master, i):
    """the upstream gradient, the reduction and db present / NULL walk the n values; the two largest n take every g"""
    a, b, ad, bd = master
    n = R.MSE_BWD_N[i]
    for g, mean, with_db in R.mse_bwd_options(i):
        what = f"segk_mse_bwd n={n} g={g} {'mean' if mean else 'sum'} db={'yes' if with_db else 'NULL'}"
        da, db = nan_buffer(n, "fp32"), nan_buffer(n, "fp32") if with_db else None
        gd = torch.tensor([g], dtype=torch.float32).cuda()
        lib.call("segk_mse_bwd", ptr(ad), ptr(bd), ptr(gd), ptr(da), ptr(db), n, mean, stream())
        sync(what)
        wa, wb = R.mse_bwd(a[:n], b[:n], g, mean)
        assert_identical(bits(take(da, n, "fp32", what + " da")), bits(wa), what + " da")
        if with_db:
            assert_identical(bits(take(db, n, "fp32", what + " db")), bits(wb), what + " db")
