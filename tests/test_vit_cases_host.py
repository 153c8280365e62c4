"""CPU: the case tables of tests/vit_cases.py reach every regime of the ViT / bilinear kernels (from the restated launch
arithmetic), the restated limits are those of the SEGK_REQUIRE lines, the references of tests/vit_reference.py agree with torch
float64, the structured designs have the properties they claim, and the derived bounds separate subtly wrong kernels
(mutants of the reference) from right ones."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import vit_cases as K
import vit_reference as R
from vit_cases import (ATTN_CASES, ATTN_INSTANCES, BIL_CASES, BIL_SMALL, BIL_STRIDE, EMBED_CASES, GRID_CASES, LN_CASES,
                       PATCH_CASES, REF_COST_CAP, AttnCase, BilCase, GridCase, PatchCase)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image_segmentation_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- limits against the source ---------------------------------------------------------------------------------------------
def test_restated_limits_are_those_of_the_source():
    vit, rs = _src("vit.hip"), _src("resize.hip")
    assert eval(re.search(r'SEGK_REQUIRE\(lds <= ([0-9 *]+), "attention: %d tokens do', vit).group(1)) == K.LDS_LIMIT
    assert len(re.findall(r"lds <= 160 \* 1024", vit)) == 2
    assert "(size_t)Tp * 144 + (size_t)64 * (Tp * 2 + 16)" in vit and "(size_t)2 * Tp * HD * sizeof(T)" in vit
    assert "(size_t)4 * (HD + 2) * 64 * 4" in vit
    assert int(re.search(r"constexpr int LN_MAXPER = (\d+);", vit).group(1)) * 64 == K.LN_MAX_D
    assert "D > 0 && D <= 64 * LN_MAXPER && Dp >= D && D % 4 == 0 && Dp % 4 == 0" in vit
    assert "D > 0 && D <= 64 * LN_MAXPER && Dp >= D," in vit
    assert "nparts >= 1 && (nparts == 1 || part_stride >= M * (long)Dp)" in vit
    assert "ldq >= 3 * heads * head_dim && ldo >= heads * head_dim && ldq % 8 == 0 && ldo % 8 == 0" in vit
    assert "Kp >= C * ps * ps && Kp % 32 == 0" in vit and "H >= ps && W >= ps && H / ps == W / ps" in vit
    assert "T > 1 && D > 0 && Dp >= D && Dp % 32 == 0" in vit
    assert [int(v) for v in re.findall(r"if \(g > (\d+)\)", vit)] == [K.MOVE_GRID_CAP] * 2
    bil = rs[:rs.index("// ---- eval-time")]
    assert [int(v) for v in re.findall(r"if \(g\d? > (\d+)\)", bil)] == [K.BILINEAR_GRID_CAP, K.MOVE_GRID_CAP, K.MOVE_GRID_CAP, K.BILINEAR_GRID_CAP]
    assert bil.count("Cp > 0 && Cp % 32 == 0") == 2
    # both sides of every limit, by the restatement
    assert {(dt, hd): K.attn_max_t(dt, hd) for dt, hd in ATTN_INSTANCES} == {("bf16", 64): 576, ("fp32", 64): 320, ("fp32", 32): 640,
                                                                            ("bf16", 32): 1280}
    for dt, hd in ATTN_INSTANCES:
        t = K.attn_max_t(dt, hd)
        c = AttnCase(dt, hd, 1, t, 1, 0)
        assert K.attn_lds(c) <= K.LDS_LIMIT < K.attn_lds(c._replace(T=t + 1)) and not K.attn_served(c._replace(T=t + 1))
    c = AttnCase("fp32", 32, 1, 8, 1, 0)
    assert K.attn_args_ok(c, 96, 32) and K.attn_args_ok(c, 104, 40) and not K.attn_args_ok(c, 100, 32) and not K.attn_args_ok(c, 88, 32)
    assert not K.attn_args_ok(c, 96, 24) and not K.attn_args_ok(c._replace(hd=48), 144, 48)
    assert K.ln_served(2048, 2048) and not K.ln_served(2052, 2052) and not K.ln_served(6, 8) and K.ln_served(4, 4)
    assert not K.ln_served(8, 10) and not K.ln_served(8, 4) and K.ln_served(8, 8, 5, 2, 40) and not K.ln_served(8, 8, 5, 2, 39)
    assert K.embed_served(1, 2, 2048, 2048) and not K.embed_served(1, 2, 2049, 2080) and not K.embed_served(1, 1, 32, 32)
    p = PatchCase("fp32", 1, 3, 28, 28, 14, 608)
    assert K.patch_served(p) and not K.patch_served(p._replace(Kp=576)) and not K.patch_served(p._replace(Kp=600))
    assert not K.patch_served(p._replace(W=42)) and K.patch_served(p._replace(W=41)) and not K.patch_served(p._replace(H=13))
    g = GridCase("fp32", 1, 2, 40, 64)
    assert K.grid_served(g) and not K.grid_served(g._replace(Dp=32)) and not K.grid_served(g._replace(Dp=48)) and not K.grid_served(g._replace(T=1))
    b = BilCase("fp32", 1, 32, 32, 1, 1, 1, 1)
    assert K.bil_served(b) and not K.bil_served(b._replace(Cp=16)) and not K.bil_served(b._replace(OH=0))


# ---- attention -------------------------------------------------------------------------------------------------------------
def test_attention_table_reaches_every_regime():
    assert all(K.attn_served(c) and K.attn_cost(c) <= REF_COST_CAP for c in ATTN_CASES)
    for dt, hd in ATTN_INSTANCES:
        cs = [c for c in ATTN_CASES if (c.dtype, c.hd) == (dt, hd)]
        single = {c.T: c for c in cs if (c.B, c.heads, c.wide) == (1, 1, 0)}
        assert {c.B for c in cs} == {1, 2} and {c.heads for c in cs} == {1, 3} and {c.wide for c in cs} == {0, 1}
        assert any(c.B == 2 and c.heads == 3 and c.wide for c in cs)
        assert K.attn_max_t(dt, hd) in single                       # the largest LDS launch the entry accepts
        if (dt, hd) == ("bf16", 64):
            assert all(K.attn_is_mfma(c) for c in cs)
            for T in (32, 33, 40, 128, 129, 197, 257, 576):
                assert T in single
            assert any(T < 32 for T in single) and {T % 32 for T in single} >= {1, 31, 0}
            assert all(K.mfma_last_block_waves(single[T])[1:] == [0, 0, 0] for T in single if T < 32)
            assert K.mfma_key_blocks(single[33]) == 2 and K.attn_tp(single[33]) - 33 == 31       # one valid key in the block
            assert K.mfma_last_block_waves(single[40]) == [32, 8, 0, 0]
            assert K.attn_query_blocks(single[128]) == 1 and K.mfma_last_block_waves(single[128]) == [32] * 4
            assert K.attn_query_blocks(single[129]) == 2 and K.mfma_last_block_waves(single[129]) == [1, 0, 0, 0]
            assert K.mfma_key_blocks(single[576]) == 18 and K.attn_lds(single[576]) == 157696
            continue
        assert not any(K.attn_is_mfma(c) for c in cs)
        assert K.valu_wave_trips(single[1]) == K.valu_wave_trips(single[3]) == [1, 0, 0, 0]     # three waves see no key
        assert K.valu_wave_trips(single[5]) == [1, 1, 0, 0]
        assert any(T % 4 for T in single) and any(T % 4 == 0 for T in single)
        assert K.valu_wave_trips(single[20]) == [2, 1, 1, 1]
        assert K.attn_query_blocks(single[64]) == 1 and K.valu_last_block_queries(single[64]) == 64
        assert K.attn_query_blocks(single[65]) == 2 and K.valu_last_block_queries(single[65]) == 1
        ov = K.valu_overlay_bytes(hd)
        assert any(K.valu_kv_bytes(c) < ov for c in cs) and any(K.valu_kv_bytes(c) > ov for c in cs)
        assert K.valu_kv_bytes(single[K.attn_max_t(dt, hd)]) == K.LDS_LIMIT


@pytest.mark.parametrize("case", ATTN_CASES, ids=K.attn_case_id)
def test_routed_and_uniform_designs(case):
    c = case
    q, k, v, want = R.routed_inputs(c)
    s = R.attn_scale(c.hd)
    for t in (q, k, v):
        assert torch.equal(R.rne_bf16(t), t)                                # bf16-representable
    pi = [K.routed_target(i, c.T) for i in range(c.T)]
    assert 0 in pi and c.T - 1 in pi and pi[0] == c.T - 1 and sorted(pi) == list(range(c.T))
    for dt in (torch.float32, torch.float64):
        out, w, S = R.attention_reference(q, k, v, s, dt)
        if dt == torch.float32:                                             # every other probability underflows to exactly 0
            assert torch.equal(out, want) and bool(((w == 0) | (w == 1)).all())
        assert float((out - want.to(dt)).abs().max()) < 1e-80               # float64: exp(-200) is what is left of them
        assert bool((S * 1 < -200).all())                                   # a zero K row (score 0) would win
        top = S.topk(2, -1).values if c.T > 1 else None
        assert c.T == 1 or bool((top[..., 0] - top[..., 1] > 200).all())
    q, k, v = R.uniform_inputs(c)
    out, w, S = R.attention_reference(q, k, v, s, torch.float32)
    assert bool((S == S[..., :1]).all()) and (c.T < 3 or bool((S != 0).any()))          # one score per query, computed one way
    ref, bound = R.uniform_expected(c, v)
    assert bool((v.sum(2).abs() < 2 ** 24).all()) and (float(bound.max()) == 0) == (c.T & (c.T - 1) == 0)
    assert bool(((out.double() - ref).abs() <= bound + 1e-6).all())


def test_routed_code_fits_head_dim_32():
    assert K.routed_reps(32) * K.ROUTED_BITS + 1 <= 32 and K.routed_reps(64) * K.ROUTED_BITS + 1 <= 64 and K.routed_reps(32) >= 1
    assert 2 ** K.ROUTED_BITS >= 1280 and len({tuple(r) for r in R.routed_code(1280).tolist()}) == 1280
    for hd in (32, 64):
        c = R.routed_scale_c(hd)
        assert c & (c - 1) == 0 and 2 * c * K.routed_reps(hd) * R.attn_scale(hd) > 200
        assert c * K.routed_reps(hd) * K.ROUTED_BITS * 4 < 2 ** 24            # every score an integer below 2^24 (times scale)


def test_attention_reference_agrees_with_torch():
    c = AttnCase("fp32", 32, 2, 37, 3, 1)
    q, k, v = R.dense_inputs(c)
    s = R.attn_scale(32)
    out, w, S = R.attention_reference(q, k, v, s)
    want = F.scaled_dot_product_attention(q.double(), k.double(), v.double(), scale=s)
    assert (out - want).abs().max() < 1e-13
    packed = R.pack_qkv(c, q, k, v)
    assert packed.shape == (74, 3 * 96 + 8) and bool(torch.isnan(packed[:, 288:]).all()) and not bool(torch.isnan(packed[:, :288]).any())
    assert torch.equal(packed[37 + 5, 96 + 32:96 + 64], k[1, 1, 5])
    assert torch.equal(R.unpack_ctx(c, packed[:, :96])[1, 2, 7], q[1, 2, 7])
    for d in ("ramp_up", "ramp_down"):
        q, k, v = R.ramp_inputs(c, d == "ramp_up")
        S = R.attention_reference(q, k, v, s)[2]
        assert 60 < float(S.max()) < 90 and -90 < float(S.min()) < -60
        run = S.cummax(-1).values
        assert bool((run[..., 1:] > run[..., :-1]).all()) if d == "ramp_up" else bool((run == run[..., :1]).all())


def _separates(ref, bound, mutant):
    r = (mutant - ref).abs() / bound.clamp(min=1e-300)
    return bool(torch.isnan(mutant).any()) or float(torch.where((mutant - ref) == 0, torch.zeros_like(r), r).max()) >= 2


def _own_bound_must_separate(c, design, name):
    """which mutants the derived bound of a dense / ramp run has to catch by itself.  Each acts on a key that carries weight
    (R.mutant_key).  (a) and (c) move the output by about that weight: far outside the bound -- but for (c) on the ramps of the
    one bf16 case above T = 640, where neighbouring scores are less than 0.13 apart, neighbouring weights nearly equal and the
    swap stays inside a bf16 ulp.  (b) scales the output by 1 - w_z, w_z the weight a score of 0 gets: exp(-40) or less on a
    ramp (never seen), about 1 / (2.4 T) on the dense run -- above fp32's bound at every T, above two bf16 half ulps (2^-8)
    only up to T = 40.  The routed and uniform designs, which are exact, catch what is left."""
    if name == "b":
        return design == "dense" and (c.dtype == "fp32" or c.T <= 40)
    return not (name == "c" and design != "dense" and c.dtype == "bf16" and c.T > 640)


@pytest.mark.parametrize("case", ATTN_CASES, ids=K.attn_case_id)
def test_attention_bounds_separate_the_mutants(case):
    """every dense / ramp run: a dropped key, an added zero-score key and two swapped V rows leave the bound by 2x at some
    element, design by design as _own_bound_must_separate says -- and where the bound cannot see one, the routed or uniform
    run of the same case does"""
    c, s = case, R.attn_scale(case.hd)
    exact = {}
    q, k, v, want = R.routed_inputs(c)
    for name, mq, mk, mv in R.attention_mutants(q, k, v):
        exact[name] = not torch.equal(R.attention_reference(mq, mk, mv, s)[0], want.double())
    q, k, v = R.uniform_inputs(c)
    ref, bound = R.uniform_expected(c, v)
    for name, mq, mk, mv in R.attention_mutants(q, k, v):
        exact[name] = exact[name] or _separates(ref, bound, R.attention_reference(mq, mk, mv, s)[0])
    assert all(exact.values()), exact
    assert set(exact) == ({"a", "b", "c"} if c.T > 1 else {"b"})
    for design in ("ramp_up", "ramp_down", "dense"):
        q, k, v = R.attn_inputs(c, design)
        ref, e_arith, e_round = R.attention_terms(c, q, k, v, s)
        bound = e_arith + e_round
        assert bool((e_arith > 0).all()) and float(bound.max()) < (1e-3 if c.dtype == "fp32" else 2e-2)
        assert bool((e_round == 0).all()) if c.dtype == "fp32" else bool((e_round > 0).all())
        at = R.mutant_key(design, c.T)
        w = R.attention_reference(q, k, v, s)[1]
        assert c.T == 1 or float(w[..., at].max()) > (0.05 if design != "dense" else 1 / (2 * c.T))      # the key carries weight
        for name, mq, mk, mv in R.attention_mutants(q, k, v, at):
            sep = _separates(ref, bound, R.attention_reference(mq, mk, mv, s)[0])
            assert sep or not _own_bound_must_separate(c, design, name), (design, name)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
def test_layernorm_tables_reach_every_regime():
    for dt in ("fp32", "bf16"):
        cs = [c for c in LN_CASES if c.dtype == dt]
        assert all(K.ln_served(c.D, c.Dp, c.M, c.nparts, K.ln_part_stride(c)) and c.M * c.D * 3 <= REF_COST_CAP for c in cs)
        assert {(c.M, c.D) for c in cs} >= {(m, d) for m in (1, 5, 33) for d in (4, 12, 100, 768, 2048)}
        assert all(K.ln_idle_waves(c.M) > 0 for c in cs) and {K.ln_blocks(c.M) for c in cs} == {1, 2, 9}   # every M: waves leave at row >= M
        for D in (4, 12, 100, 768, 2048):
            assert {c.Dp - D for c in cs if c.D == D} == {0, 4}
        assert {c.nparts for c in cs} == {1, 2, 3}
        assert {(c.nparts, c.loose) for c in cs if c.nparts > 1} == {(2, 0), (2, 1), (3, 0), (3, 1)}
        assert all(K.ln_part_stride(c) > c.M * c.Dp for c in cs if c.loose)
        assert {K.ln_per4(c.D) for c in cs} == {1, 3, 8} and K.ln_nq(4) == 1 and K.ln_nq(2048) == 512
        es = [c for c in EMBED_CASES if c.dtype == dt]
        assert all(K.embed_served(c.B, c.T, c.D, c.Dp) for c in es)
        assert {c.T for c in es} == {2, 5, 197} and {c.B for c in es} == {1, 3} and {c.D for c in es} == {32, 96, 768, 2048}
        for D in (32, 96, 768, 2048):
            assert {c.Dp - D for c in es if c.D == D} == {0, 32}
        assert K.embed_per(96) == 2 and 96 % 64 != 0 and any(c.B == 3 and c.T == 197 for c in es)
        assert any((c.B * c.T) % 4 for c in es)


@pytest.mark.parametrize("case", [c for c in LN_CASES if c.D >= 12], ids=K.ln_case_id)
def test_layernorm_reference_designs_and_mutant(case):
    c = case
    gamma, beta = R.ln_params(c.D, "add")
    n_m, n_v = R.add_ln_chain(c.D)
    for design in K.LN_DESIGNS:
        h0, parts = R.add_ln_inputs(c, design)
        assert bool(torch.isnan(parts[:, :, c.D:]).all()) and not bool(torch.isnan(parts[:, :, :c.D]).any())
        v = R.add_chain_f32(h0, parts, c.D)
        ref, bound = R.ln_reference(v, gamma, beta, 1e-5, n_m, n_v, c.dtype)
        want = F.layer_norm(v.double(), (c.D,), gamma.double(), beta.double(), 1e-5)
        assert (ref - want).abs().max() < 1e-9 * max(1.0, float(want.abs().max()))
        if design == "constant":
            assert bool((v == v[:, :1]).all()) and torch.equal(ref, beta.double().expand_as(ref))
        if design == "lattice":
            assert torch.equal(v.double(), h0.double() + parts[:, :, :c.D].double().sum(0))        # the fp32 chain is exact
        if design == "offset":
            assert bool(((v.mean(1) - 4096).abs() < 1).all())
            assert float(bound.max()) < 0.1
            assert _separates(ref, bound, R.ln_one_pass_f32(v, gamma, beta, 1e-5).double())
        if design == "dense":
            # a right two-pass float32 LayerNorm sits inside the bound
            assert bool(((F.layer_norm(v, (c.D,), gamma, beta, 1e-5).double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("case", EMBED_CASES, ids=K.embed_case_id)
def test_embed_reference_and_designs(case):
    c = case
    n_m, n_v = R.embed_chain(c.D)
    for design in K.EMBED_DESIGNS:
        gamma, beta = R.ln_params(c.D, "embed", const_gamma=design == "lattice")
        proj, cls, pos = R.embed_inputs(c, design)
        v = R.embed_rows_f32(c, proj, cls, pos)
        assert v.shape == (c.B * c.T, c.D) and not bool(torch.isnan(v).any())
        for b in range(c.B):
            assert torch.equal(v[b * c.T], cls + pos[0])
            assert torch.equal(v[b * c.T + c.T - 1], proj[b * (c.T - 1) + c.T - 2, :c.D] + pos[c.T - 1])
        ref, bound = R.ln_reference(v, gamma, beta, 1e-5, n_m, n_v, "fp32")
        want = F.layer_norm(v.double(), (c.D,), gamma.double(), beta.double(), 1e-5)
        assert (ref - want).abs().max() < 1e-9 * max(1.0, float(want.abs().max()))
        if design == "constant":
            assert torch.equal(ref, beta.double().expand_as(ref))
        if design == "lattice":
            assert bool((gamma == gamma[0]).all()) and bool((beta == 0).all()) and float(cls.abs().min()) > 50
        if design == "offset":
            assert _separates(ref, bound, R.ln_one_pass_f32(v, gamma, beta, 1e-5).double())


# ---- movement --------------------------------------------------------------------------------------------------------------
def test_movement_tables_and_references():
    for dt in ("fp32", "bf16"):
        ps = [c for c in PATCH_CASES if c.dtype == dt]
        assert all(K.patch_served(c) and K.patch_items(c) <= REF_COST_CAP for c in ps)
        shapes = {(c.C, c.H, c.W, c.ps): c for c in ps}
        assert {(3, 32, 32, 16), (3, 28, 28, 14), (1, 64, 64, 32), (2, 30, 31, 14)} <= set(shapes)
        assert shapes[(3, 28, 28, 14)].Kp == 608 == K.pad32(588) and shapes[(2, 30, 31, 14)].Kp == K.pad32(392) > 392
        assert any(c.Kp > K.pad32(c.C * c.ps * c.ps) for c in ps) and any(c.H % c.ps or c.W % c.ps for c in ps)
        two = [c for c in ps if K.move_trips(K.patch_items(c)) == 2]
        assert len(two) == 1 and all(K.move_trips(K.patch_items(c)) == 1 for c in ps if c not in two)
        c = two[0]                                                   # the smallest: one patch row less fits one trip
        assert K.move_trips(K.patch_items(c._replace(H=c.H - c.ps, W=c.W - c.ps))) == 1 and K.move_grid(K.patch_items(c)) == 16384
        gs = [c for c in GRID_CASES if c.dtype == dt]
        assert all(K.grid_served(c) for c in gs) and {c.T for c in gs} == {2, 197}
        assert any(c.Dp == c.D for c in gs) and any(c.Dp == c.D + 32 for c in gs)
        two = [c for c in gs if K.move_trips(K.grid_items(c)) == 2]
        assert len(two) == 1 and K.move_trips(K.grid_items(two[0]._replace(B=two[0].B - 1))) == 1
    c = PatchCase("fp32", 2, 2, 30, 31, 14, 416)
    x = R.patch_input(c)
    want = F.unfold(x[:, :, :28, :28], 14, stride=14).transpose(1, 2).reshape(8, 392)
    got = R.patchify_reference(c, x)
    assert torch.equal(got[:, :392], want) and bool((got[:, 392:] == 0).all())
    assert torch.equal(R.patchify_reference(c._replace(dtype="bf16"), x), got.to(torch.bfloat16).float())
    g = GridCase("bf16", 2, 5, 40, 64)
    h = R.grid_input(g)
    out = R.grid_reference(g, h)
    assert torch.equal(out[:, :, :40], h[:, 1:].to(torch.bfloat16).float()) and bool((out[:, :, 40:] == 0).all())
    # inputs name their elements: the fp32 ones are linear indices; the bf16 ones survive the rounding and differ from every
    # element fewer than 251 places away along any one dimension (so from all neighbours)
    assert torch.equal(R.patch_input(c).reshape(-1), torch.arange(2 * 2 * 30 * 31).float())
    assert torch.equal(R.grid_input(g._replace(dtype="fp32")).reshape(-1), torch.arange(2 * 5 * 40).float())
    for t in [R.patch_input(p) for p in PATCH_CASES if p.dtype == "bf16"] + [R.grid_input(q) for q in GRID_CASES if q.dtype == "bf16"]:
        assert torch.equal(R.rne_bf16(t), t) and float(t.abs().max()) <= 125
        for dim in range(t.dim()):
            for d in {1, 2, 15, 16, 17, 250} & set(range(1, t.shape[dim])):
                assert bool((t.narrow(dim, d, t.shape[dim] - d) != t.narrow(dim, 0, t.shape[dim] - d)).all())


# ---- bilinear --------------------------------------------------------------------------------------------------------------
def test_bilinear_table_reaches_every_regime():
    assert all(K.bil_served(c) and K.bil_cost(c) <= REF_COST_CAP for c in BIL_CASES)
    for dt in ("fp32", "bf16"):
        shapes = {(c.IH, c.IW, c.OH, c.OW): c for c in BIL_SMALL if c.dtype == dt}
        assert set(shapes) == {(14, 14, 28, 28), (14, 14, 56, 56), (14, 14, 224, 224), (7, 7, 10, 13), (3, 5, 6, 10), (1, 1, 5, 7),
                               (5, 9, 1, 1), (8, 8, 8, 8), (16, 12, 4, 3)}
        assert (shapes[(3, 5, 6, 10)].C, shapes[(3, 5, 6, 10)].Cp) == (40, 64)
        assert {s for s, c in shapes.items() if K.bil_exact(c)} == {(14, 14, 28, 28), (14, 14, 56, 56), (8, 8, 8, 8), (3, 5, 6, 10)}
        assert {K.bil_ops_form(c) for c in shapes.values()} == {"separable", "gather"}
        assert all(K.bil_trips(c, k) == 1 for c in shapes.values() for k in ("fwd", "bwd2d", "sep_x", "sep_y"))
    # a second trip behind each of the four caps in both dtypes (the item count divides the channels by 4 in fp32 and by 8 in
    # bf16), and each such case is the smallest: one row less of the side the kernel's items run over is one trip
    grow = {"fwd": "OH", "bwd2d": "IH", "sep_y": "IH", "sep_x": "OH"}
    for k, side in grow.items():
        for dt in ("fp32", "bf16"):
            two = [c for c in BIL_STRIDE if c.dtype == dt and K.bil_trips(c, k) == 2]
            assert two, (k, dt)
            assert any(K.bil_trips(c._replace(**{side: getattr(c, side) - 1}), k) == 1 for c in two), (k, dt)
    assert K.bil_cv(BilCase("fp32", 1, 32, 32, 1, 1, 1, 1)) == 8 and K.bil_cv(BilCase("bf16", 1, 32, 32, 1, 1, 1, 1)) == 4
    assert all(max(K.bil_trips(c, k) for k in grow) >= 2 for c in BIL_STRIDE)
    assert all(c.IH != c.IW or c.OH != c.OW for c in BIL_STRIDE)
    assert max(K.bil_scratch_floats(c) for c in BIL_CASES) * 4 <= K.BIL_SCRATCH_CAP


@pytest.mark.parametrize("case", BIL_SMALL, ids=K.bil_case_id)
def test_bilinear_references_and_mutant(case):
    c = case
    for design in ("lattice", "dense"):
        x, dy = R.bilinear_inputs(c, design)
        assert bool((x[..., c.C:] == 0).all()) and bool((dy[..., c.C:] == 0).all())
        ref = R.bilinear_fwd_reference(c, x)
        xt = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        yt = F.interpolate(xt, size=(c.OH, c.OW), mode="bilinear", align_corners=False)
        tol = 1e-5 * max(1.0, float(ref.abs().max()))                # torch computes its lambda in float64
        assert (yt.detach().permute(0, 2, 3, 1) - ref).abs().max() < tol
        yt.backward(dy.double().permute(0, 3, 1, 2))
        bref = R.bilinear_bwd_reference(c, dy)
        assert (xt.grad.permute(0, 2, 3, 1) - bref).abs().max() < 1e-5 * max(1.0, float(bref.abs().max()))
        f32 = R.bilinear_fwd_f32(c, x)
        fb = R.bilinear_fwd_bound(c, x, ref)
        assert f32.dtype == torch.float32 and bool(((f32.double() - ref).abs() <= fb).all())
        # the adjoint identity holds between the two references
        lhs, rhs = (ref * dy.double()).sum(), (x.double() * bref).sum()
        assert abs(float(lhs - rhs)) <= 1e-10 * max(1.0, abs(float(lhs)))
        assert bool((ref[..., c.C:] == 0).all()) and bool((bref[..., c.C:] == 0).all())
        if (c.IH, c.IW) == (c.OH, c.OW):
            assert torch.equal(ref, x.double()) and torch.equal(bref, dy.double())
        if design == "lattice" and K.bil_exact(c):
            assert torch.equal(f32.double(), ref) and torch.equal(bref.float().double(), bref)
            # (exact in fp32; bf16 stores the one rounding of that exact value)
        if design == "dense":
            mut = R.bilinear_bwd_mutant(c, dy)
            assert (mut is None) == (c.IH < 2)
            if mut is not None:
                assert _separates(bref, R.bilinear_bwd_bound(c, dy, bref), mut)


def test_src_index_matches_the_kernel_expression():
    i0, i1, lam = R.src_index_f32(224, 14)
    assert lam.dtype == torch.float32 and int(i0[0]) == 0 and float(lam[0]) == 0 and int(i0[-1]) == 13 == int(i1[-1])
    assert int(i0[8]) == 0 and float(lam[8]) == 0.03125 and int(i1[8]) == 1
    i0, i1, lam = R.src_index_f32(5, 1)
    assert i0.tolist() == i1.tolist() == [0] * 5 and float(lam[4]) > 0         # in_size == 1: both taps on pixel 0
    W = R.weight_matrix(5, 1)
    assert torch.equal(W, torch.ones((5, 1), dtype=torch.float64))
