"""GPU (-m gpu): the stem kernels (csrc/stem.hip), the 2x2 pooling kernels and the BN-statistics finalisation
(csrc/bn_pool.hip) through the C ABI against float64, on the case tables of tests/stem_pool_cases.py
(tests/test_stem_pool_cases_host.py proves on the CPU that they reach every regime of the streaming and grid-stride loops).
References and the derivation of every bound: tests/stem_pool_reference.py.

Every output buffer (z, xn, the statistics rows, the slabs, dx, pooled, part, ...) is pre-filled with a NaN pattern and
followed by a guard of the same pattern: after the call every element must be overwritten and the guard untouched.

  stem impulse:  x is zero but for isolated 1.0 pixels: every z equals one bf16-rounded weight or 0; for the weight gradient
                 dz holds 1.0 in channel n at probe n: the gradient equals the shifted bf16-rounded x, columns >= 9 Cin are 0.
  stem lattice:  small integers: z, the statistics' column sums and the gradient equal the reference exactly -- a 16-pixel
                 block counted twice or dropped in the looping cases shows here.
  stem dense:    random inputs against the derived bounds; z is bit-identical with and without the xn / stats outputs.
  pooling:       forward, backward (with and without accumulation) and the fused apply + pool are bit-identical to their
                 restatements; the fused backward + BatchNorm reduce returns that dx and partial rows within derived bounds.
Equality is numerical equality of every element (NaN equals nothing; -0 equals 0).
Set SEGK_STEM_POOL_PARITY_OUT=<file> to record the worst error / bound per kernel and regime
(profiles/stem_pool_matrix_parity.txt)."""
import os

import pytest
import torch

import stem_pool_cases as K
import stem_pool_reference as R
from bn_reference import apply_reference
from conv_reference import channel_stats
from matrix_helpers import (BITS_DT, NAN_BITS, SEGK_DT, TORCH_DT, assert_equal, assert_within, make_recorder, nan_buffer, ptr, stream,
                            sync, take, write_parity)
from stem_pool_cases import FINALIZE_CASES, NUM_CUS, POOL_CASES, STAT_CASES, STEM_CASES, STEM_WGRAD_DENSE, PoolCase

pytestmark = pytest.mark.gpu

_PARITY, record = make_recorder()                   # "kernel quantity regime" -> [worst error / bound, case id]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if cus != NUM_CUS:
        pytest.skip(f"the case tables are evaluated for {NUM_CUS} compute units, this device reports {cus}")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_STEM_POOL_PARITY_OUT")
    if out and _PARITY:
        write_parity(out, _PARITY,
                     "# worst error / bound per kernel, quantity and regime of tests/test_gpu_stem_pool_matrix.py (bounds derived in\n"
                     "# tests/stem_pool_reference.py); 0.0000 on an exact run: every element equal to the float64 restatement\n")


# ---- the restated launch arithmetic against the ABI's own queries ----------------------------------------------------------
def test_restated_grids_equal_the_queries(lib):
    for c in STEM_CASES:
        assert lib.query("segk_stem3x3_rows", c.B, c.H, c.W, c.Cin, 64, 1) == K.stem_rows(c), c
        assert lib.query("segk_stem3x3_wgrad_slabs", c.B, c.H, c.W, c.Cin, 64, 1) == K.stem_wgrad_slabs(c), c
    assert lib.query("segk_stem3x3_rows", 1, 8, 24, 3, 64, 1) == 0 and lib.query("segk_stem3x3_rows", 1, 8, 16, 4, 64, 1) == 0
    assert lib.query("segk_stem3x3_rows", 1, 8, 16, 3, 64, 0) == 0 and lib.query("segk_stem3x3_wgrad_slabs", 1, 8, 16, 3, 32, 1) == 0
    for s in STAT_CASES:
        c = s.case
        assert lib.query("segk_maxpool_bwd_stat_blocks", c.B, c.H, c.W, c.Cp, SEGK_DT[c.dtype]) == K.pool_grid(c, "stat") > 0, c
    for dt in ("bf16", "fp32"):                                   # 12 or 24 channel vectors: not served
        assert lib.query("segk_maxpool_bwd_stat_blocks", 1, 8, 8, 96, SEGK_DT[dt]) == K.pool_grid(PoolCase(dt, 1, 8, 8, 96), "stat") == 0


# ---- stem forward ----------------------------------------------------------------------------------------------------------
def run_stem(lib, c, x, w, with_xn=True, with_stats=True):
    """-> (z [B,H,W,64] bf16, xn [B,H,W,32] bf16 | None, rows [rows,64,2] fp32 | None) on the CPU"""
    what = f"segk_stem3x3 {K.stem_case_id(c)}"
    rows = lib.query("segk_stem3x3_rows", c.B, c.H, c.W, c.Cin, 64, 1)
    assert rows == K.stem_rows(c), f"{what}: segk_stem3x3_rows = {rows}, the restatement says {K.stem_rows(c)}"
    P = c.B * c.H * c.W
    xd, wd = x.cuda(), w.contiguous().cuda()
    z = nan_buffer(P * 64, "bf16")
    xn = nan_buffer(P * 32, "bf16") if with_xn else None
    nst = lib.query("segk_bn_stats_floats", rows, 64)
    assert nst >= rows * 128
    st = nan_buffer(nst, "fp32") if with_stats else None
    lib.call("segk_stem3x3", ptr(xd), ptr(wd), ptr(z), ptr(xn), ptr(st), c.B, c.H, c.W, c.Cin, 64, 1, stream())
    sync(what)
    zc = take(z, P * 64, "bf16", what + " z").reshape(c.B, c.H, c.W, 64)
    xc = take(xn, P * 32, "bf16", what + " xn").reshape(c.B, c.H, c.W, 32) if with_xn else None
    rc = take(st, nst, "fp32", what + " statistics rows", written=rows * 128)[:rows * 128].reshape(rows, 64, 2) if with_stats else None
    return zc, xc, rc


def assert_exact_stats(rows, z, what):
    tot = rows.double().sum(0)
    for j, (ref, name) in enumerate(zip(channel_stats(z), ("sum", "sumsq"))):
        bad = (tot[:, j] != ref).nonzero().flatten().tolist()
        assert not bad, f"{what}: {name} of {len(bad)} channels differs, first n={bad[0]}: {tot[bad[0], j].item()!r}, want " \
                        f"{ref[bad[0]].item()!r} (a dropped or doubled block?)"


@pytest.mark.parametrize("case", STEM_CASES, ids=K.stem_case_id)
def test_stem_impulse_is_exact(lib, case):
    c = case
    for probes in K.stem_probe_passes(c):
        x, w = R.stem_inputs(c, "impulse", probes)
        want = R.stem_impulse_expected(c, w, probes)
        z, xn, rows = run_stem(lib, c, x, w)
        assert_equal(z, want, f"stem impulse {K.stem_case_id(c)} probes {probes}")
        assert_equal(xn, R.stem_xn(x), f"stem impulse {K.stem_case_id(c)} xn")
        assert_exact_stats(rows, want, f"stem impulse {K.stem_case_id(c)}")
    record(f"stem3x3 impulse {K.stem_regime(c)}", 0.0, K.stem_case_id(c))


@pytest.mark.parametrize("case", STEM_CASES, ids=K.stem_case_id)
def test_stem_lattice_is_exact(lib, case):
    c = case
    x, w = R.stem_inputs(c, "lattice")
    want = R.stem_reference(x, w)
    assert R.lattice_is_exact(want)
    z, xn, rows = run_stem(lib, c, x, w)
    assert_equal(z, want, f"stem lattice {K.stem_case_id(c)}")
    assert_equal(xn, R.stem_xn(x), f"stem lattice {K.stem_case_id(c)} xn")
    assert_exact_stats(rows, want, f"stem lattice {K.stem_case_id(c)}")
    record(f"stem3x3 lattice {K.stem_regime(c)}", 0.0, K.stem_case_id(c))


@pytest.mark.parametrize("case", STEM_CASES, ids=K.stem_case_id)
def test_stem_dense_against_float64(lib, case):
    c, cid, reg = case, K.stem_case_id(case), K.stem_regime(case)
    x, w = R.stem_inputs(c, "dense")
    ref = R.stem_reference(x, w)
    zb, b1, b2 = R.stem_dense_bounds(c, ref, R.stem_abs_reference(x, w))
    z, xn, rows = run_stem(lib, c, x, w)
    record(f"stem3x3 dense z {reg}", assert_within(z.float(), ref, zb, f"stem dense {cid} z"), cid)
    tot = rows.double().sum(0)
    s1, s2 = channel_stats(ref)
    record(f"stem3x3 dense sum {reg}", assert_within(tot[:, 0], s1, b1, f"stem dense {cid} sum"), cid)
    record(f"stem3x3 dense sumsq {reg}", assert_within(tot[:, 1], s2, b2, f"stem dense {cid} sumsq"), cid)
    want_xn = R.stem_xn(x)
    assert torch.equal(xn.view(torch.int16), want_xn.view(torch.int16)), f"stem dense {cid}: xn is not the bf16 rounding of x"
    assert bool((xn[..., c.Cin:].view(torch.int16) == 0).all())
    z2, _, rows2 = run_stem(lib, c, x, w, with_xn=False)
    z3, xn3, _ = run_stem(lib, c, x, w, with_stats=False)
    zi = z.view(torch.int16)
    assert torch.equal(zi, z2.view(torch.int16)) and torch.equal(zi, z3.view(torch.int16)), f"stem dense {cid}: z depends on xn / stats"
    assert torch.equal(rows.view(torch.int32), rows2.view(torch.int32)) and torch.equal(xn.view(torch.int16), xn3.view(torch.int16))


# ---- stem weight gradient --------------------------------------------------------------------------------------------------
def run_stem_wgrad(lib, c, x, dz):
    """-> (slabs [S,64,32] fp32, segk_wgrad_reduce's gradient [64, 9 Cin] fp32) on the CPU"""
    what = f"segk_stem3x3_wgrad {K.stem_case_id(c)}"
    S = lib.query("segk_stem3x3_wgrad_slabs", c.B, c.H, c.W, c.Cin, 64, 1)
    assert S == K.stem_wgrad_slabs(c), f"{what}: segk_stem3x3_wgrad_slabs = {S}, the restatement says {K.stem_wgrad_slabs(c)}"
    Kc = 9 * c.Cin
    xd, dd = x.cuda(), dz.contiguous().cuda()
    slabs, grad = nan_buffer(S * 2048, "fp32"), nan_buffer(64 * Kc, "fp32")
    lib.call("segk_stem3x3_wgrad", ptr(xd), ptr(dd), ptr(slabs), c.B, c.H, c.W, c.Cin, 64, 1, stream())
    lib.call("segk_wgrad_reduce", ptr(slabs), S, ptr(grad), 64, Kc, 0, 64, 32, 0, 1, stream())
    sync(what)
    return (take(slabs, S * 2048, "fp32", what + " slabs").reshape(S, 64, 32), take(grad, 64 * Kc, "fp32", what + " gradient").reshape(64, Kc))


def check_slab_padding(c, slabs, what):
    assert bool((slabs[:, :, 9 * c.Cin:] == 0).all()), f"{what}: columns >= 9 Cin of a slab are not zero"


@pytest.mark.parametrize("case", STEM_CASES, ids=K.stem_case_id)
def test_stem_wgrad_impulse_is_exact(lib, case):
    c, cid = case, K.stem_case_id(case)
    probes = K.stem_probe_pixels(c)
    x, dz = R.stem_wgrad_inputs(c, "impulse", probes)
    want = R.stem_wgrad_impulse_expected(c, x, probes)
    slabs, grad = run_stem_wgrad(lib, c, x, dz)
    check_slab_padding(c, slabs, f"stem wgrad impulse {cid}")
    assert_equal(slabs.double().sum(0)[:, :9 * c.Cin], want, f"stem wgrad impulse {cid} (float64 slab sum; rows = probes {probes})")
    assert_equal(grad, want, f"stem wgrad impulse {cid} (segk_wgrad_reduce)")
    record(f"stem3x3_wgrad impulse {K.stem_wgrad_regime(c)}", 0.0, cid)


@pytest.mark.parametrize("case", STEM_CASES, ids=K.stem_case_id)
def test_stem_wgrad_lattice_is_exact(lib, case):
    c, cid = case, K.stem_case_id(case)
    x, dz = R.stem_wgrad_inputs(c, "lattice")
    want, A = R.stem_wgrad_reference(x, dz)
    assert bool((A < 2 ** 24).all())
    slabs, grad = run_stem_wgrad(lib, c, x, dz)
    check_slab_padding(c, slabs, f"stem wgrad lattice {cid}")
    tot = slabs.double().sum(0)[:, :9 * c.Cin]
    assert bool((tot == want).all()), f"stem wgrad lattice {cid}: {int((tot != want).sum())} elements of the float64 slab sum differ, " \
                                      f"worst by {float((tot - want).abs().max())} (a dropped or doubled block?)"
    assert bool((grad.double() == want).all()), f"stem wgrad lattice {cid}: segk_wgrad_reduce differs from the reference"
    record(f"stem3x3_wgrad lattice {K.stem_wgrad_regime(c)}", 0.0, cid)


@pytest.mark.parametrize("case", STEM_WGRAD_DENSE, ids=K.stem_case_id)
def test_stem_wgrad_dense_against_float64(lib, case):
    c, cid, reg = case, K.stem_case_id(case), K.stem_wgrad_regime(case)
    x, dz = R.stem_wgrad_inputs(c, "dense")
    ref, A = R.stem_wgrad_reference(x, dz)
    b_host, b_dev = R.stem_wgrad_bounds(c, A)
    slabs, grad = run_stem_wgrad(lib, c, x, dz)
    check_slab_padding(c, slabs, f"stem wgrad dense {cid}")
    tot = slabs.double().sum(0)[:, :9 * c.Cin]
    record(f"stem3x3_wgrad dense slabs {reg}", assert_within(tot, ref, b_host, f"stem wgrad dense {cid} float64 slab sum"), cid)
    record(f"stem3x3_wgrad dense reduce {reg}", assert_within(grad, ref, b_dev, f"stem wgrad dense {cid} segk_wgrad_reduce"), cid)
    slabs2, grad2 = run_stem_wgrad(lib, c, x, dz)
    assert torch.equal(slabs.view(torch.int32), slabs2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))


# ---- pooling ---------------------------------------------------------------------------------------------------------------
def _trips(c, kernel):
    return f"{c.dtype} trips={K.pool_trips(c, kernel)}"


@pytest.mark.parametrize("case", POOL_CASES, ids=K.pool_case_id)
def test_maxpool_forward_and_backward_are_exact(lib, case):
    c, cid, sdt = case, K.pool_case_id(case), SEGK_DT[case.dtype]
    x, dy, dx0 = R.pool_inputs(c)
    n_in, n_out = x.numel(), dy.numel()
    xd, dyd = x.cuda(), dy.cuda()
    y = nan_buffer(n_out, c.dtype)
    lib.call("segk_maxpool2x2_fwd", ptr(xd), ptr(y), c.B, c.H, c.W, c.Cp, sdt, stream())
    dx = nan_buffer(n_in, c.dtype)
    lib.call("segk_maxpool2x2_bwd", ptr(xd), ptr(dyd), ptr(dx), c.B, c.H, c.W, c.Cp, 0, sdt, stream())
    dxa = nan_buffer(n_in, c.dtype)
    dxa[:n_in] = dx0.reshape(-1).view(BITS_DT[c.dtype]).cuda()
    lib.call("segk_maxpool2x2_bwd", ptr(xd), ptr(dyd), ptr(dxa), c.B, c.H, c.W, c.Cp, 1, sdt, stream())
    sync(f"maxpool {cid}")
    assert_equal(take(y, n_out, c.dtype, f"maxpool_fwd {cid}").reshape(dy.shape), R.maxpool_fwd_reference(x), f"maxpool_fwd {cid}")
    record(f"maxpool2x2_fwd {_trips(c, 'fwd')}", 0.0, cid)
    assert_equal(take(dx, n_in, c.dtype, f"maxpool_bwd {cid}").reshape(x.shape), R.maxpool_bwd_reference(x, dy), f"maxpool_bwd {cid}")
    got = dxa.cpu()
    assert bool((got[n_in:] == NAN_BITS[c.dtype]).all()), f"maxpool_bwd accumulate {cid}: wrote behind the buffer"
    assert_equal(got[:n_in].view(TORCH_DT[c.dtype]).reshape(x.shape), R.maxpool_bwd_reference(x, dy, dx0), f"maxpool_bwd accumulate {cid}")
    record(f"maxpool2x2_bwd {_trips(c, 'bwd')}", 0.0, cid)


@pytest.mark.parametrize("case", POOL_CASES, ids=K.pool_case_id)
def test_bn_relu_apply_pool_is_exact(lib, case):
    c, cid, sdt = case, K.pool_case_id(case), SEGK_DT[case.dtype]
    z, scale, shift = R.apply_pool_inputs(c)
    zd, scd, shd = z.cuda(), scale.cuda(), shift.cuda()
    n_in, n_out = z.numel(), c.B * (c.H // 2) * (c.W // 2) * c.Cp
    y, pooled = nan_buffer(n_in, c.dtype), nan_buffer(n_out, c.dtype)
    lib.call("segk_bn_relu_apply_pool", ptr(zd), ptr(y), ptr(pooled), ptr(scd), ptr(shd), c.B, c.H, c.W, c.Cp, sdt, stream())
    sync(f"bn_relu_apply_pool {cid}")
    want_y, want_p = R.apply_pool_reference(z, scale, shift, TORCH_DT[c.dtype])
    assert bool((R.windows(want_y.float()).amax(3) == 0).any())          # windows whose four y are all zero
    assert_equal(take(y, n_in, c.dtype, f"bn_relu_apply_pool {cid} y").reshape(z.shape), want_y, f"bn_relu_apply_pool {cid} y")
    assert_equal(take(pooled, n_out, c.dtype, f"bn_relu_apply_pool {cid} pooled").reshape(want_p.shape), want_p, f"bn_relu_apply_pool {cid} pooled")
    record(f"bn_relu_apply_pool {_trips(c, 'bwd')}", 0.0, cid)


@pytest.mark.parametrize("stat", STAT_CASES, ids=K.stat_case_id)
def test_maxpool_bwd_bnstat_against_float64(lib, stat):
    s, c, cid, sdt = stat, stat.case, K.stat_case_id(stat), SEGK_DT[stat.case.dtype]
    z, y, dy, dx0, scale, shift, mean, rstd = R.stat_inputs(s)
    nb = lib.query("segk_maxpool_bwd_stat_blocks", c.B, c.H, c.W, c.Cp, sdt)
    assert nb == K.pool_grid(c, "stat") > 0
    n_in = y.numel()
    yd, dyd, zd = y.cuda(), dy.cuda(), (z.cuda() if s.with_z else None)
    vec = [v.cuda() for v in (scale, shift, mean, rstd)]
    dx = nan_buffer(n_in, c.dtype)
    if s.accumulate:
        dx[:n_in] = dx0.reshape(-1).view(BITS_DT[c.dtype]).cuda()
    part = nan_buffer(nb * c.Cp * 2, "fp32")
    lib.call("segk_maxpool2x2_bwd_bnstat", ptr(yd), ptr(dyd), ptr(dx), c.B, c.H, c.W, c.Cp, s.accumulate, *(ptr(v) for v in vec),
             ptr(part), ptr(zd), sdt, stream())
    sync(f"maxpool_bwd_bnstat {cid}")
    pre = R.maxpool_bwd_presum(y, dy, dx0 if s.accumulate else None)
    want_dx = pre.to(TORCH_DT[c.dtype])
    got = dx.cpu()
    assert bool((got[n_in:] == NAN_BITS[c.dtype]).all()), f"maxpool_bwd_bnstat {cid}: wrote behind dx"
    assert bool((got[:n_in] != NAN_BITS[c.dtype]).all()), f"maxpool_bwd_bnstat {cid}: dx elements were not written"
    assert_equal(got[:n_in].view(TORCH_DT[c.dtype]).reshape(y.shape), want_dx, f"maxpool_bwd_bnstat {cid} dx")
    rows = take(part, nb * c.Cp * 2, "fp32", f"maxpool_bwd_bnstat {cid} part").reshape(nb, c.Cp, 2).double().sum(0)
    r = R.stat_reference(s, z, y, want_dx, scale, shift, mean, rstd, pre)
    if s.degenerate:
        assert int(r["from_z"].sum()) == 3 * K.pool_vec(c.dtype)
    else:
        assert not r["from_z"].any()
    reg = f"{c.dtype} trips={K.pool_trips(c, 'stat')}" + ("" if s.with_z else " z=NULL")
    # the addends the kernel takes (the fp32 gradient before its store) within the chain bound, then the stored gradient
    # within that plus what the store's rounding moved (stem_pool_reference's docstring)
    record(f"maxpool2x2_bwd_bnstat sum_g_kernel {reg}",
           assert_within(rows[:, 0], r["sum_g_kernel"], r["bound_g_kernel"], f"bnstat {cid} sum g, the kernel's addends"), cid)
    record(f"maxpool2x2_bwd_bnstat sum_gx_kernel {reg}",
           assert_within(rows[:, 1], r["sum_gx_kernel"], r["bound_gx_kernel"], f"bnstat {cid} sum g xhat, the kernel's addends"), cid)
    record(f"maxpool2x2_bwd_bnstat sum_g {reg}", assert_within(rows[:, 0], r["sum_g"], r["bound_g"], f"bnstat {cid} sum g"), cid)
    record(f"maxpool2x2_bwd_bnstat sum_gx {reg}", assert_within(rows[:, 1], r["sum_gx"], r["bound_gx"], f"bnstat {cid} sum g xhat"), cid)
    record(f"maxpool2x2_bwd_bnstat true_gx {reg}",
           assert_within(rows[:, 1], r["true_gx"], r["bound_true"], f"bnstat {cid} sum g xhat against (z - mean) rstd"), cid)


# ---- BN-statistics finalisation --------------------------------------------------------------------------------------------
def run_finalize(lib, rows, C, Cr, count, cb, gamma, beta, rm0, rv0, training, with_mean=True):
    """-> dict of the C-long outputs on the CPU; running statistics start from rm0 / rv0 with a NaN pattern behind channel Cr"""
    what = f"segk_bn_finalize MT={0 if rows is None else rows.shape[0]} C={C} training={training}"
    part = None
    MT = 0
    if rows is not None:
        MT = rows.shape[0]
        n = lib.query("segk_bn_stats_floats", MT, C)
        part = torch.zeros((n,), dtype=torch.float32, device="cuda")
        part[:MT * C * 2] = rows.reshape(-1).cuda()
    pad = lambda v: None if v is None else torch.cat([v[:Cr], torch.full((C - Cr,), float("nan"))]).cuda()
    gd, bd, cbd = pad(gamma), pad(beta), pad(cb)
    run = {}
    for name, v in (("rmean", rm0), ("rvar", rv0)):
        run[name] = nan_buffer(C, "fp32")
        run[name][:Cr] = v[:Cr].view(torch.int32).cuda()
    out = {name: nan_buffer(C, "fp32") for name in (("scale", "shift", "mean", "rstd") if with_mean else ("scale", "shift"))}
    lib.call("segk_bn_finalize", ptr(part), MT, C, Cr, float(count), ptr(cbd), ptr(gd), ptr(bd), ptr(run["rmean"]), ptr(run["rvar"]),
             0.1, 1e-5, training, ptr(out["scale"]), ptr(out["shift"]), ptr(out.get("mean")), ptr(out.get("rstd")), stream())
    sync(what)
    res = {name: take(buf, C, "fp32", f"{what} {name}") for name, buf in out.items()}
    for name, buf in run.items():
        bits = buf.cpu()
        assert bool((bits[Cr:] == NAN_BITS["fp32"]).all()), f"{what}: {name} of a padded channel (or behind the buffer) was touched"
        res[name] = bits[:Cr].view(torch.float32)
    return res


def check_finalize(res, ref, Cr, what, mode):
    for name in res:
        got = res[name]
        if name in ("scale", "shift", "mean", "rstd"):
            assert bool((got[Cr:].view(torch.int32) << 1 == 0).all()), f"{what}: {name} of a padded channel is not zero"
        want, bound = ref[name]
        if float(bound.max()) == 0:
            assert torch.equal(got[:Cr].double(), want), f"{what}: {name} changed"
        else:
            record(f"bn_finalize {mode} {name}", assert_within(got[:Cr], want, bound, f"{what} {name}"), what)


def _finalize_params(C):
    g = torch.Generator().manual_seed(C)
    u = lambda lo, hi: torch.rand((C,), generator=g) * (hi - lo) + lo
    return u(0.5, 1.5) * torch.where(torch.arange(C) % 4 == 3, -1.0, 1.0), u(-0.5, 0.5), u(-0.2, 0.2), u(-0.1, 0.1), u(0.5, 1.5)


@pytest.mark.parametrize("case", FINALIZE_CASES, ids=str)
def test_bn_finalize_training(lib, case):
    """both launch forms, constant-input channels (the variance cancels to either side of the clamp at 0: rstd = 1 / sqrt(eps)),
    padded channels, the running statistics; count = 1 at MT = 1 (the guard on the unbiased variance)"""
    MT, C = case
    Cr = C - 5 if C > 32 else C
    rows, const = R.finalize_rows(MT, C, per_row=4)
    gamma, beta, cb, rm0, rv0 = _finalize_params(C)
    counts = [float(MT * 4)]
    if MT == 1:
        rows[0, :, 1] = rows[0, :, 0] ** 2 + rows[0, :, 1] / 8           # one pixel: s2 >= s1^2
        counts = [1.0, 4.0]
    for count in counts:
        for bias in (cb, None):
            ref = R.finalize_reference(rows, count, Cr, gamma, beta, bias, rm0, rv0, 0.1, 1e-5, True)
            if MT > 1:
                assert bool((ref["raw_var"][const] < 0).any())
            for rep in range(2):                                     # repeated launches re-use the ticket counters
                res = run_finalize(lib, rows, C, Cr, count, bias, gamma, beta, rm0, rv0, 1)
                assert bool(torch.isfinite(res["rvar"]).all())
                check_finalize(res, ref, Cr, f"MT={MT} C={C} count={count:g} bias={bias is not None}", "training")


@pytest.mark.parametrize("C", [32, 96, 1024])
def test_bn_finalize_eval(lib, C):
    """training = 0: scale / shift from the running statistics, with and without conv_bias, mean / rstd NULL and given; the
    running statistics are left as they are"""
    Cr = C - 5 if C > 32 else C
    gamma, beta, cb, rm0, rv0 = _finalize_params(C)
    rv0[1] = 0.0                                                     # rstd = 1 / sqrt(eps)
    for bias in (cb, None):
        ref = R.finalize_reference(None, 1.0, Cr, gamma, beta, bias, rm0, rv0, 0.1, 1e-5, False)
        for with_mean in (True, False):
            res = run_finalize(lib, None, C, Cr, 1.0, bias, gamma, beta, rm0, rv0, 0, with_mean=with_mean)
            assert ("mean" in res) == with_mean
            check_finalize(res, ref, Cr, f"eval C={C} bias={bias is not None} mean/rstd={'given' if with_mean else 'NULL'}", "eval")
