"""GPU (-m gpu): the ViT encoder kernels (csrc/vit.hip) and the bilinear skip resize (the two entries at the top of
csrc/resize.hip) through the C ABI against float64, on the case tables of tests/vit_cases.py (tests/test_vit_cases_host.py
proves on the CPU that they reach every launch regime and that the bounds separate subtly wrong kernels from right ones).
References, the write contract of every entry and the derivation of every bound: tests/vit_reference.py.

Every output buffer is pre-filled with a NaN pattern and followed by a guard of the same pattern: after the call every
element the contract says is written must be overwritten, everything else (the guard, pitch columns) untouched.

  attention:  routed (the output is one V row, element for element), uniform (the mean over the keys: exact at a power-of-two
              T), two ramps and a dense run against the derived bound, the arithmetic part of the error within half of its
              share of the bound -- all four kernel instances at every regime.
  LayerNorm:  the updated residual stream equals its float32 restatement; constant rows return beta exactly; lattice, offset
              (mean 4096, spread 1) and dense rows within the derived bound; the three call forms.
  movement:   vit_patchify and vit_tokens_to_grid equal their restatement, inputs carry their own coordinates.
  bilinear:   the fp32 forward equals its float32 restatement; bf16 and both backward forms (2-D gather and separable, run on
              every case and compared with each other) within derived bounds, exact on the power-of-two up-scalings.
Equality is numerical equality of every element (NaN equals nothing; -0 equals 0).
Set SEGK_VIT_PARITY_OUT=<file> to record the worst error / bound per kernel, quantity and regime
(profiles/vit_resize_matrix_parity.txt)."""
import os

import pytest
import torch

import vit_cases as K
import vit_reference as R
from matrix_helpers import (NAN_BITS, SEGK_DT, TORCH_DT, assert_equal, assert_within, make_recorder, nan_buffer, ptr, stream, sync,
                            take, write_parity)
from vit_cases import ATTN_CASES, ATTN_INSTANCES, BIL_CASES, EMBED_CASES, GRID_CASES, LN_CASES, PATCH_CASES, AttnCase

pytestmark = pytest.mark.gpu

_PARITY, record = make_recorder()


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_VIT_PARITY_OUT")
    if out and _PARITY:
        write_parity(out, _PARITY,
                     "# worst error / bound per kernel, quantity and regime of tests/test_gpu_vit_matrix.py (bounds derived in\n"
                     f"# tests/vit_reference.py, EXP_ULPS = {R.EXP_ULPS}); 0.0000 on an exact run: every element equal to the restatement\n"
                     "# attention \"arith\" rows: worst (error - e_round) / e_arith, asserted <= 0.5; 0.0000 there: the roundings to bf16\n"
                     "# (e_round) cover the whole error\n", width=66)


def dev(t, dtype):
    """a CPU fp32 tensor holding values of the dtype -> the device tensor in that dtype"""
    return t.to(TORCH_DT[dtype]).contiguous().cuda()


def within_or_equal(got, ref, bound, what):
    if float(bound.max()) == 0:
        assert_equal(got, ref, what)
        return 0.0
    return assert_within(got, ref, bound, what)


# ---- attention -------------------------------------------------------------------------------------------------------------
def attn_regime(c):
    if (c.B, c.heads, c.wide) != (1, 1, 0):
        return "B/heads/pitch"
    if c.T == K.attn_max_t(c.dtype, c.hd):
        return "lds-limit"
    if K.attn_is_mfma(c):
        return "T<32" if c.T < 32 else "key-blocks" if c.T <= 128 else "query-blocks"
    return "empty-waves" if c.T <= 12 else "one-query-block" if c.T <= 64 else "query-blocks"


def run_attention(lib, c, q, k, v, what):
    """-> ctx as [B, heads, T, hd] fp32 on the CPU"""
    ldq, ldo = K.attn_pitches(c)
    D, rows = c.heads * c.hd, c.B * c.T
    qkv = dev(R.pack_qkv(c, q, k, v), c.dtype)
    ctx = nan_buffer(rows * ldo, c.dtype)
    lib.call("segk_attention", ptr(qkv), ptr(ctx), c.B, c.T, c.heads, c.hd, ldq, ldo, R.attn_scale(c.hd), SEGK_DT[c.dtype], stream())
    sync(what)
    mask = torch.zeros((rows, ldo), dtype=torch.bool)
    mask[:, :D] = True
    out = take(ctx, rows * ldo, c.dtype, what, mask=mask).reshape(rows, ldo)[:, :D]
    return R.unpack_ctx(c, out.float())


@pytest.mark.parametrize("case", ATTN_CASES, ids=K.attn_case_id)
def test_attention(lib, case):
    c, cid, reg = case, K.attn_case_id(case), attn_regime(case)
    name = f"attention {c.dtype}/{c.hd}"
    q, k, v, want = R.routed_inputs(c)
    assert_equal(run_attention(lib, c, q, k, v, f"attention routed {cid}"), want, f"attention routed {cid}")
    record(f"{name} routed {reg}", 0.0, cid)
    q, k, v = R.uniform_inputs(c)
    ref, bound = R.uniform_expected(c, v)
    got = run_attention(lib, c, q, k, v, f"attention uniform {cid}")
    record(f"{name} uniform {reg}", within_or_equal(got, ref, bound, f"attention uniform {cid}"), cid)
    for design in ("ramp_up", "ramp_down", "dense"):
        q, k, v = R.attn_inputs(c, design)
        ref, e_arith, e_round = R.attention_terms(c, q, k, v, R.attn_scale(c.hd))
        got = run_attention(lib, c, q, k, v, f"attention {design} {cid}")
        ratio = assert_within(got, ref, e_arith + e_round, f"attention {design} {cid}")
        record(f"{name} {design} {reg}", ratio, cid)
        # the arithmetic alone: what is left of the error beyond the roundings to bf16 (P, the store), which are attained;
        # with fp32 storage e_round is 0 and this is error / bound itself
        arith = float((((got.double() - ref).abs() - e_round).clamp(min=0) / e_arith).max())
        print(f"attention {design} {cid}: (error - e_round) / e_arith = {arith:.4f}")
        record(f"{name} {design} arith {reg}", arith, cid)
        assert arith <= 0.5, f"attention {design} {cid}: (error - e_round) / e_arith = {arith:.3f} > 0.5: EXP_ULPS = {R.EXP_ULPS} is too small"


@pytest.mark.parametrize("inst", ATTN_INSTANCES, ids=lambda i: f"{i[0]}-hd{i[1]}")
def test_attention_refuses_what_does_not_fit(lib, inst):
    dt, hd = inst
    T = K.attn_max_t(dt, hd) + 1
    c = AttnCase(dt, hd, 1, T, 1, 0)
    assert not K.attn_served(c) and K.attn_args_ok(c)
    qkv = torch.zeros((T, 3 * hd), dtype=TORCH_DT[dt], device="cuda")
    ctx = nan_buffer(T * hd, dt)
    with pytest.raises(RuntimeError, match="LDS"):
        lib.call("segk_attention", ptr(qkv), ptr(ctx), 1, T, 1, hd, 3 * hd, hd, R.attn_scale(hd), SEGK_DT[dt], stream())
    with pytest.raises(RuntimeError, match="pitches"):
        lib.call("segk_attention", ptr(qkv), ptr(ctx), 1, 8, 1, hd, 3 * hd + 4, hd, R.attn_scale(hd), SEGK_DT[dt], stream())
    sync("attention refusals")
    assert bool((ctx.cpu() == NAN_BITS[dt]).all())


# ---- add + LayerNorm -------------------------------------------------------------------------------------------------------
def run_add_ln(lib, c, h0, parts, gamma, beta, form, what):
    """-> (h [M, D] fp32, out [M, D] fp32 or None) on the CPU; form: add_ln, add_only (out = 0), ln_only (delta = 0)"""
    M, D, Dp = c.M, c.D, c.Dp
    h = nan_buffer(M * D, "fp32")
    h[:M * D] = h0.reshape(-1).view(torch.int32).cuda()
    stride = K.ln_part_stride(c)
    flat = torch.full((c.nparts * stride,), float("nan"))
    for p in range(c.nparts):
        flat[p * stride:p * stride + M * Dp] = parts[p].reshape(-1)
    delta = dev(flat, c.dtype) if form != "ln_only" else None
    out = nan_buffer(M * Dp, c.dtype) if form != "add_only" else None
    gd, bd = (gamma.cuda(), beta.cuda()) if out is not None else (None, None)
    if c.nparts == 1:
        lib.call("segk_add_layernorm", ptr(h), ptr(delta), ptr(gd), ptr(bd), 1e-5, ptr(out), M, D, Dp, SEGK_DT[c.dtype], stream())
    else:
        lib.call("segk_add_layernorm_parts", ptr(h), ptr(delta), c.nparts, stride, ptr(gd), ptr(bd), 1e-5, ptr(out), M, D, Dp,
                 SEGK_DT[c.dtype], stream())
    sync(what)
    hc = take(h, M * D, "fp32", what + " h").reshape(M, D)
    if out is None:
        return hc, None
    mask = torch.zeros((M, Dp), dtype=torch.bool)
    mask[:, :D] = True
    return hc, take(out, M * Dp, c.dtype, what + " out", mask=mask).reshape(M, Dp)[:, :D].float()


@pytest.mark.parametrize("case", LN_CASES, ids=K.ln_case_id)
def test_add_layernorm(lib, case):
    c, cid = case, K.ln_case_id(case)
    gamma, beta = R.ln_params(c.D, "add")
    n_m, n_v = R.add_ln_chain(c.D)
    name = f"add_layernorm{'_parts' if c.nparts > 1 else ''} {c.dtype}"
    for design in K.LN_DESIGNS:
        h0, parts = R.add_ln_inputs(c, design)
        hsum = R.add_chain_f32(h0, parts, c.D)
        for form in K.LN_FORMS:
            what = f"add_layernorm {form} {design} {cid}"
            h, out = run_add_ln(lib, c, h0, parts, gamma, beta, form, what)
            v = h0 if form == "ln_only" else hsum
            if form == "ln_only":
                assert torch.equal(h.view(torch.int32), h0.view(torch.int32)), f"{what}: h changed"
            else:
                assert_equal(h, hsum, what + " h")
                record(f"{name} h {design}", 0.0, cid)
            if form == "add_only":
                continue
            ref, bound = R.ln_reference(v, gamma, beta, 1e-5, n_m, n_v, c.dtype)
            if design == "constant":
                assert bool((v == v[:, :1]).all())
                assert_equal(out, R.to_dtype(beta, c.dtype).expand_as(out), what + " out == beta")
                record(f"{name} out constant", 0.0, cid)
            else:
                record(f"{name} out {design} {form}", assert_within(out, ref, bound, what + " out"), cid)


def test_add_layernorm_refusals(lib):
    t = torch.zeros(8192, device="cuda")
    for D, Dp in ((2052, 2052), (6, 8), (8, 10), (8, 4)):
        assert not K.ln_served(D, Dp)
        with pytest.raises(RuntimeError, match="hidden size"):
            lib.call("segk_add_layernorm", ptr(t), ptr(t), ptr(t), ptr(t), 1e-5, ptr(t), 1, D, Dp, 0, stream())
    with pytest.raises(RuntimeError, match="partial-product"):
        lib.call("segk_add_layernorm_parts", ptr(t), ptr(t), 2, 39, ptr(t), ptr(t), 1e-5, ptr(t), 5, 8, 8, 0, stream())
    with pytest.raises(RuntimeError, match="hidden size"):
        lib.call("segk_vit_embed_ln", ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 1e-5, ptr(t), 1, 2, 2049, 2080, 0, stream())
    sync("LayerNorm refusals")


# ---- class token + position embedding + pre-LayerNorm ----------------------------------------------------------------------
@pytest.mark.parametrize("case", EMBED_CASES, ids=K.embed_case_id)
def test_vit_embed_ln(lib, case):
    c, cid = case, K.embed_case_id(case)
    n_m, n_v = R.embed_chain(c.D)
    n = c.B * c.T * c.D
    for design in K.EMBED_DESIGNS:
        what = f"vit_embed_ln {design} {cid}"
        gamma, beta = R.ln_params(c.D, "embed", const_gamma=design == "lattice")
        proj, cls, pos = R.embed_inputs(c, design)
        pd, cd, sd, gd, bd = dev(proj, c.dtype), cls.cuda(), pos.contiguous().cuda(), gamma.cuda(), beta.cuda()
        h = nan_buffer(n, "fp32")
        lib.call("segk_vit_embed_ln", ptr(pd), ptr(cd), ptr(sd), ptr(gd), ptr(bd), 1e-5, ptr(h), c.B, c.T, c.D, c.Dp, SEGK_DT[c.dtype], stream())
        sync(what)
        got = take(h, n, "fp32", what).reshape(c.B * c.T, c.D)
        v = R.embed_rows_f32(c, proj, cls, pos)
        ref, bound = R.ln_reference(v, gamma, beta, 1e-5, n_m, n_v, "fp32")
        if design == "constant":
            assert_equal(got, beta.expand_as(got), what + " == beta")
            record(f"vit_embed_ln {c.dtype} constant", 0.0, cid)
        else:
            record(f"vit_embed_ln {c.dtype} {design}", assert_within(got, ref, bound, what), cid)


# ---- pure movement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PATCH_CASES, ids=K.patch_case_id)
def test_vit_patchify(lib, case):
    c, cid = case, K.patch_case_id(case)
    x = R.patch_input(c)
    n = K.patch_items(c)
    xd = x.cuda()
    rows = nan_buffer(n, c.dtype)
    lib.call("segk_vit_patchify", ptr(xd), ptr(rows), c.B, c.C, c.H, c.W, c.ps, c.Kp, SEGK_DT[c.dtype], stream())
    sync(f"vit_patchify {cid}")
    want = R.patchify_reference(c, x)
    assert_equal(take(rows, n, c.dtype, f"vit_patchify {cid}").reshape(want.shape), want, f"vit_patchify {cid} (values name their input element)")
    record(f"vit_patchify {c.dtype} trips={K.move_trips(n)}", 0.0, cid)


@pytest.mark.parametrize("case", GRID_CASES, ids=K.grid_case_id)
def test_vit_tokens_to_grid(lib, case):
    c, cid = case, K.grid_case_id(case)
    h = R.grid_input(c)
    n = K.grid_items(c)
    hd = h.cuda()
    out = nan_buffer(n, c.dtype)
    lib.call("segk_vit_tokens_to_grid", ptr(hd), ptr(out), c.B, c.T, c.D, c.Dp, SEGK_DT[c.dtype], stream())
    sync(f"vit_tokens_to_grid {cid}")
    want = R.grid_reference(c, h)
    assert_equal(take(out, n, c.dtype, f"vit_tokens_to_grid {cid}").reshape(want.shape), want, f"vit_tokens_to_grid {cid} (values name their input element)")
    record(f"vit_tokens_to_grid {c.dtype} trips={K.move_trips(n)}", 0.0, cid)


def test_movement_refusals(lib):
    t = torch.zeros(8192, device="cuda")
    with pytest.raises(RuntimeError, match="Kp"):
        lib.call("segk_vit_patchify", ptr(t), ptr(t), 1, 3, 28, 28, 14, 600, 0, stream())
    with pytest.raises(RuntimeError, match="Kp"):
        lib.call("segk_vit_patchify", ptr(t), ptr(t), 1, 3, 28, 28, 14, 576, 0, stream())
    with pytest.raises(RuntimeError, match="bad shape"):
        lib.call("segk_vit_patchify", ptr(t), ptr(t), 1, 3, 28, 42, 14, 608, 0, stream())
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("segk_vit_tokens_to_grid", ptr(t), ptr(t), 1, 2, 40, 48, 0, stream())
    sync("movement refusals")


# ---- bilinear --------------------------------------------------------------------------------------------------------------
def bil_regime(c):
    trips = {k: K.bil_trips(c, k) for k in ("fwd", "bwd2d", "sep_x", "sep_y")}
    if max(trips.values()) > 1:
        return "strided " + ",".join(k for k, t in trips.items() if t > 1)
    if (c.IH, c.IW) == (c.OH, c.OW):
        return "identity"
    return "exact-weights" if K.bil_exact(c) else "down" if c.OH < c.IH else "up"


def run_bilinear(lib, c, x, dy, what):
    """-> (y, dx of the 2-D gather, dx of the separable form) as fp32 on the CPU"""
    sdt = SEGK_DT[c.dtype]
    n_in, n_out = x.numel(), dy.numel()
    xd, dyd = dev(x, c.dtype), dev(dy, c.dtype)
    y, dx2, dxs = nan_buffer(n_out, c.dtype), nan_buffer(n_in, c.dtype), nan_buffer(n_in, c.dtype)
    scratch = nan_buffer(K.bil_scratch_floats(c), "fp32")
    lib.call("segk_bilinear_fwd", ptr(xd), ptr(y), c.B, c.IH, c.IW, c.OH, c.OW, c.Cp, sdt, stream())
    lib.call("segk_bilinear_bwd", ptr(dyd), ptr(dx2), 0, c.B, c.IH, c.IW, c.OH, c.OW, c.Cp, sdt, stream())
    lib.call("segk_bilinear_bwd", ptr(dyd), ptr(dxs), ptr(scratch), c.B, c.IH, c.IW, c.OH, c.OW, c.Cp, sdt, stream())
    sync(what)
    take(scratch, K.bil_scratch_floats(c), "fp32", what + " scratch")
    return (take(y, n_out, c.dtype, what + " y").reshape(dy.shape).float(), take(dx2, n_in, c.dtype, what + " dx (gather)").reshape(x.shape).float(),
            take(dxs, n_in, c.dtype, what + " dx (separable)").reshape(x.shape).float())


@pytest.mark.parametrize("case", BIL_CASES, ids=K.bil_case_id)
def test_bilinear(lib, case):
    c, cid, reg = case, K.bil_case_id(case), bil_regime(case)
    for design in (("lattice", "dense") if K.bil_exact(c) else ("dense",)):
        what = f"bilinear {design} {cid}"
        x, dy = R.bilinear_inputs(c, design)
        y, dx2, dxs = run_bilinear(lib, c, x, dy, what)
        f32 = R.bilinear_fwd_f32(c, x)
        ref, bref = R.bilinear_fwd_reference(c, x), R.bilinear_bwd_reference(c, dy)
        if c.dtype == "fp32":
            assert_equal(y, f32, what + " y against the float32 restatement")
            record(f"bilinear_fwd fp32 restated {reg}", 0.0, cid)
        exact = design == "lattice"
        fb = torch.zeros_like(ref) if exact else R.bilinear_fwd_bound(c, x, ref)
        bb = torch.zeros_like(bref) if exact else R.bilinear_bwd_bound(c, dy, bref)
        want_y, want_dx = (R.to_dtype(ref.float(), c.dtype), R.to_dtype(bref.float(), c.dtype)) if exact else (ref, bref)
        record(f"bilinear_fwd {c.dtype} {design} {reg}", within_or_equal(y, want_y, fb, what + " y"), cid)
        record(f"bilinear_bwd gather {c.dtype} {design} {reg}", within_or_equal(dx2, want_dx, bb, what + " dx (gather)"), cid)
        record(f"bilinear_bwd separable {c.dtype} {design} {reg}", within_or_equal(dxs, want_dx, bb, what + " dx (separable)"), cid)
        record(f"bilinear_bwd gather-separable {c.dtype} {design} {reg}", within_or_equal(dx2, dxs.double(), 2 * bb, what + " the two forms"), cid)
        assert bool((y[..., c.C:] == 0).all()) and bool((dx2[..., c.C:] == 0).all()) and bool((dxs[..., c.C:] == 0).all()), \
            f"{what}: padding channels are not zero"
        if (c.IH, c.IW) == (c.OH, c.OW):
            assert_equal(y, x, what + " y == x")
            assert_equal(dx2, dy, what + " dx == dy (gather)")
            assert_equal(dxs, dy, what + " dx == dy (separable)")
        if not exact:                       # <fwd(x), g> == <x, bwd(g)> within what the two bounds allow
            lhs = (y.double() * dy.double()).sum()
            slack = (fb * dy.double().abs()).sum() + (bb * x.double().abs()).sum()
            for form, dx in (("gather", dx2), ("separable", dxs)):
                gap = abs(float(lhs - (x.double() * dx.double()).sum()))
                print(f"{what} adjoint ({form}): gap / allowed = {gap / float(slack):.4f}")
                assert gap <= float(slack), f"{what}: adjoint identity ({form}) off by {gap}, allowed {float(slack)}"
                record(f"bilinear adjoint {form} {c.dtype} {reg}", gap / float(slack), cid)
