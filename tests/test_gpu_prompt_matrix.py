"""GPU (-m gpu): the entries of csrc/prompt.hip -- segk_prompt_scores, segk_prompt_make, segk_prompt_heatmap -- through the
C ABI against the restatements of tests/prompt_reference.py, on its case tables (tests/test_recon_prompt_cases_host.py proves on
the CPU that the restatements reproduce the fixture captured from the reference, and that the tables reach one, two and three
64-lane passes, a pass with one live lane, every remainder of the 4-row unroll, the scalar path and the 16-byte path with and
without a vector that crosses a row, and one, two and three k0 passes of the first-candidate search).

Every output is pre-filled with a NaN pattern (a byte or int64 pattern no valid result holds for the integer outputs) and
followed by a guard of the same pattern.

  scores      |dev - ref| <= N 2^-53 ref per entry: any-order summation of N non-negative float64 terms against the exactly
              rounded sum; cls equal wherever the reference's choice is stable under twice that bound (the host test shows every
              candidate of the table is); two runs bit-identical.
  make        heat, target, classes, centres and valid equal to the retry loop, written as a loop.
  heat-map    equal.

Measured on an MI355X (SEGK_PROMPT_PARITY_OUT=<file> writes the record, profiles/prompt_matrix_parity.txt): worst score
error / bound 0.2340 (70x200-R1, nine terms: a last-bit difference against a bound of nine); 0.04 and below at R >= 31; no
candidate unstable, no class differs.  The other gates are equalities."""
import os

import numpy as np
import pytest
import torch

import prompt_reference as P
from matrix_helpers import assert_identical, make_recorder, nan_buffer, ptr, stream, sync, take, write_parity

pytestmark = pytest.mark.gpu

_PARITY, record = make_recorder()
# int32 outputs sit in "fp32" pattern buffers (the pattern, 2145299712, is no class and no coordinate), float64 scores in
# "i64" ones (the pattern reads 1.7e308, no sum of at most 16641 weights <= 1)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_PROMPT_PARITY_OUT")
    if out and _PARITY:
        write_parity(out, _PARITY, "# worst error / bound per case of tests/test_gpu_prompt_matrix.py (bound N 2^-53 ref, derived in\n"
                                   "# tests/prompt_reference.py); the pass condition is ratio <= 1\n")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f64_buffer(n):
    return nan_buffer(n, "i64")


# ---- segk_prompt_scores ----------------------------------------------------------------------------------------------------
def run_scores(lib, labd, lutd, cend, wd, nw, c, what):
    n = c.B * c.K
    sc, cl = f64_buffer(n * P.NC), nan_buffer(n, "fp32")
    lib.call("segk_prompt_scores", ptr(labd), ptr(lutd), ptr(cend), ptr(wd), nw, c.R, ptr(sc), ptr(cl), c.B, c.K, c.H, c.W, stream())
    sync(what)
    return sc, cl


@pytest.mark.parametrize("case", P.SCORE_CASES, ids=lambda c: c.name)
def test_scores_and_classes_against_the_restatement(lib, case):
    c, what = case, f"segk_prompt_scores {case.name}"
    lab, cen = P.score_inputs(c)
    w, nw = P.score_tables(c)
    lut = P.LUTS[c.lut]
    labd, lutd, cend, wd = dev(lab), dev(lut), dev(cen), dev(w)
    sc, cl = run_scores(lib, labd, lutd, cend, wd, nw, c, what)
    n = c.B * c.K
    got = take(sc, n * P.NC, "i64", what + " scores").view(torch.float64).reshape(c.B, c.K, P.NC).numpy()
    cls = take(cl, n, "fp32", what + " cls").view(torch.int32).reshape(c.B, c.K).numpy()
    assert np.isfinite(got).all(), what
    worst, unstable = 0.0, 0
    for b in range(c.B):
        ref, N, rcls = P.scores(lab[b], lut, cen[b], w, nw, c.R)
        err, bound = np.abs(got[b] - ref), P.score_bound(ref, N)
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        worst = max(worst, float(ratio.max()))
        assert (err <= bound).all(), f"{what} image {b}: error is {ratio.max():.3f} x the bound at {np.argwhere(ratio == ratio.max())[0].tolist()}"
        st = P.stable(ref, N)
        unstable += int((~st).sum())
        assert np.array_equal(cls[b][st], rcls[st]), f"{what} image {b}: classes {cls[b][st].tolist()}, want {rcls[st].tolist()}"
        if c.name in P.ALL_ZERO_SCORE_CASES:
            assert not got[b].any() and not cls[b].any(), what
    print(f"{what}: error / bound = {worst:.4f}, unstable {unstable} of {n}")
    record(f"prompt_scores {c.name}", worst, f"B={c.B} K={c.K} R={c.R} lut={c.lut}")
    assert unstable <= 0.01 * n, (unstable, n)
    sc2, cl2 = run_scores(lib, labd, lutd, cend, wd, nw, c, what + " again")
    assert torch.equal(sc2, sc) and torch.equal(cl2, cl), f"{what}: two runs differ"


# ---- segk_prompt_make ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.MAKE_CASES, ids=lambda c: f"{c.H}x{c.W}-K{c.K}-pi{c.per_image}-nq{c.nq}-{c.lut}")
def test_make_is_the_retry_loop(lib, case):
    c, B, PI = case, 3, case.per_image
    what = f"segk_prompt_make {c.H}x{c.W} K={c.K} per_image={PI} nq={c.nq} lut={c.lut}"
    lab, cen, cls, _ = P.make_inputs(c)
    lut, q = P.LUTS[c.lut], P.q_table()
    HW = c.H * c.W
    heat, target = nan_buffer(B * PI * HW, "fp32"), nan_buffer(B * PI * HW, "i64")
    classes, centres, valid = nan_buffer(B * PI, "fp32"), nan_buffer(B * PI * 2, "fp32"), nan_buffer(B, "u8")
    labd, lutd, cend, clsd, qd = dev(lab), dev(lut), dev(cen), dev(cls), dev(q)
    lib.call("segk_prompt_make", ptr(labd), ptr(lutd), ptr(cend), ptr(clsd), ptr(qd), c.nq, ptr(heat), ptr(target), ptr(classes),
             ptr(centres), ptr(valid), B, c.K, PI, c.H, c.W, stream())
    sync(what)
    got_heat = take(heat, B * PI * HW, "fp32", what + " heat").reshape(B, PI, c.H, c.W)
    got_target = take(target, B * PI * HW, "i64", what + " target").reshape(B, PI, c.H, c.W)
    got_classes = take(classes, B * PI, "fp32", what + " classes").view(torch.int32).reshape(B, PI)
    got_centres = take(centres, B * PI * 2, "fp32", what + " centres").view(torch.int32).reshape(B, PI, 2)
    got_valid = take(valid, B, "u8", what + " valid")
    for b in range(B):
        h, t, cl, ce, v = P.make(lab[b], lut, cen[b], cls[b], q, c.nq, PI)
        w_ = f"{what} image {b}"
        assert int(got_valid[b]) == v, f"{w_}: valid = {int(got_valid[b])}, want {v}"
        assert_identical(got_classes[b], torch.from_numpy(cl), w_ + " classes")
        assert_identical(got_centres[b], torch.from_numpy(ce), w_ + " centres")
        assert_identical(got_heat[b].view(torch.int32), torch.from_numpy(h).view(torch.int32), w_ + " heat")
        assert_identical(got_target[b], torch.from_numpy(t), w_ + " target")


# ---- segk_prompt_heatmap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.HEAT_CASES, ids=lambda c: f"{c.H}x{c.W}-P{c.P}-nq{c.nq}-{c.kind.replace(' ', '-')}")
def test_heatmap_is_the_restatement(lib, case):
    c, what = case, f"segk_prompt_heatmap {case.H}x{case.W} P={case.P} nq={case.nq} {case.kind}"
    pts, q = P.heat_points(c), P.q_table()
    HW = c.H * c.W
    heat = nan_buffer(HW, "fp32")
    ptd, qd = dev(pts), dev(q)
    lib.call("segk_prompt_heatmap", ptr(ptd), c.P, ptr(qd), c.nq, ptr(heat), c.H, c.W, stream())
    sync(what)
    got = take(heat, HW, "fp32", what).reshape(c.H, c.W)
    want = torch.from_numpy(P.heatmap(pts, q, c.nq, c.H, c.W))
    assert_identical(got.view(torch.int32), want.view(torch.int32), what)
    if c.kind == "all outside":
        assert not got.any()
