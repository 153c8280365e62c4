"""CPU: the restatements of tests/pack_reference.py against identities that do not share their indexing (a convolution
evaluated from the packed operand by the consumer's reading rule against torch's own, in float64), and the coverage the case
tables of tests/pack_cases.py promise."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import pack_cases as K
import pack_reference as R


def _dense(p):
    """the consumer's reading rule: a packed operand [Kp / CH][taps][Np][CH] read as B[tap][k][n], k = chunk * CH + lane"""
    kc, taps, Np, ch = p.shape
    B = torch.empty((taps, kc * ch, Np), dtype=torch.float64)
    for k in range(kc * ch):
        B[:, k, :] = R.read_packed(p, k, slice(None), slice(None))
    return B


def _conv_from_packed(a, B):
    """3x3, padding 1: out[b][n][y][x] = sum over taps (dy, dx) and k of a[b][k][y + dy - 1][x + dx - 1] * B[3 dy + dx][k][n]"""
    H, W = a.shape[2:]
    ap = F.pad(a, (1, 1, 1, 1))
    return sum(torch.einsum("bkyx,kn->bnyx", ap[:, :, dy:dy + H, dx:dx + W], B[3 * dy + dx]) for dy in range(3) for dx in range(3))


def _padded_concat(xa, xb, CAp, CBp):
    """the activations as the kernels see them: source A's channels, its padding, source B's channels, its padding"""
    Bn, CA, H, W = xa.shape
    out = torch.zeros((Bn, CAp + CBp, H, W), dtype=torch.float64)
    out[:, :CA] = xa
    if xb is not None:
        out[:, CAp:CAp + xb.shape[1]] = xb
    return out


@pytest.mark.parametrize("geo,dtype", [((5, 3, 0, 32, 32, 0), "fp32"), ((33, 20, 50, 64, 32, 64), "fp32"),
                                       ((40, 40, 12, 64, 48, 16), "fp32"), ((5, 3, 0, 32, 32, 0), "bf16"),
                                       ((33, 20, 50, 64, 32, 64), "bf16"), ((40, 40, 12, 96, 64, 32), "bf16")])
def test_restated_conv_packs_compute_the_convolution_and_its_data_gradient(geo, dtype):
    Cout, CA, CB, Coutp, CAp, CBp = geo
    w = R.special_values((Cout, CA + CB, 3, 3), 1)
    wq = w.to(R.TORCH_DT[dtype]).double()
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, CA + CB, 5, 6), generator=g, dtype=torch.float64)
    dy = torch.randn((2, Cout, 5, 6), generator=g, dtype=torch.float64)
    # forward: the mode-0 operand
    fwd = _conv_from_packed(_padded_concat(x[:, :CA], x[:, CA:] if CB else None, CAp, CBp),
                            _dense(R.pack_conv(w, CA, CB, Coutp, CAp, CBp, 9, 0, dtype)))
    assert torch.allclose(fwd[:, :Cout], F.conv2d(x, wq, padding=1), rtol=0, atol=1e-12)
    assert bool((fwd[:, Cout:] == 0).all())
    # data gradient: the same consumer on the output gradient with the mode-1 operand
    dyp = torch.zeros((2, Coutp, 5, 6), dtype=torch.float64)
    dyp[:, :Cout] = dy
    dx = _conv_from_packed(dyp, _dense(R.pack_conv(w, CA, CB, Coutp, CAp, CBp, 9, 1, dtype)))
    want = F.conv_transpose2d(dy, wq, padding=1)
    assert torch.allclose(dx[:, :CA], want[:, :CA], rtol=0, atol=1e-12)
    assert torch.allclose(dx[:, CAp:CAp + CB], want[:, CA:], rtol=0, atol=1e-12)
    pad = torch.ones(CAp + CBp, dtype=torch.bool)
    pad[:CA] = False
    pad[CAp:CAp + CB] = False
    assert bool((dx[:, pad] == 0).all())


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("taps", [9, 1])
def test_data_gradient_pack_is_the_forward_pack_of_the_flipped_transpose(taps, dtype):
    for Cout, Cin in ((33, 31), (70, 40), (1, 1)):
        w = R.special_values((Cout, Cin) + ((3, 3) if taps == 9 else (1, 1)), 3)
        a = R.pack_conv(w, Cin, 0, R.pad32(Cout), R.pad32(Cin), 0, taps, 1, dtype)
        b = R.pack_conv(w.transpose(0, 1).flip(2, 3).contiguous(), Cout, 0, R.pad32(Cin), R.pad32(Cout), 0, taps, 0, dtype)
        assert torch.equal(R.bits(a), R.bits(b))


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("shape", [(3, 5), (40, 33), (33, 70)])
def test_restated_convt_packs_compute_the_transposed_convolution_and_its_data_gradient(shape, dtype):
    Cin, Cout = shape
    Cinp, Coutp = R.pad32(Cin), R.pad32(Cout)
    w = R.special_values((Cin, Cout, 2, 2), 4)
    wq = w.to(R.TORCH_DT[dtype]).double()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, Cin, 3, 4), generator=g, dtype=torch.float64).requires_grad_(True)
    dout = torch.randn((2, Cout, 6, 8), generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, wq, stride=2)
    ref.backward(dout)
    # forward: one GEMM over K = ci makes column q * Coutp + co, stored at output pixel (2 y + i, 2 x + j), q = 2 i + j
    Bf = _dense(R.pack_convt(w, Cinp, Coutp, 0, dtype))[0]
    xp = torch.zeros((2, Cinp, 3, 4), dtype=torch.float64)
    xp[:, :Cin] = x.detach()
    cols = torch.einsum("bkyx,kn->bnyx", xp, Bf).reshape(2, 2, 2, Coutp, 3, 4)          # [b][i][j][co][y][x]
    out = cols.permute(0, 3, 4, 1, 5, 2).reshape(2, Coutp, 6, 8)
    assert torch.allclose(out[:, :Cout], ref.detach(), rtol=0, atol=1e-12) and bool((out[:, Cout:] == 0).all())
    # data gradient: K = q * Coutp + co gathers the four output pixels of an input pixel
    Bd = _dense(R.pack_convt(w, Cinp, Coutp, 1, dtype))[0]
    dp = torch.zeros((2, Coutp, 6, 8), dtype=torch.float64)
    dp[:, :Cout] = dout
    rows = dp.reshape(2, Coutp, 3, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(2, 4 * Coutp, 3, 4)   # [b][q * Coutp + co][y][x]
    din = torch.einsum("bkyx,kn->bnyx", rows, Bd)
    assert torch.allclose(din[:, :Cin], x.grad, rtol=0, atol=1e-12) and bool((din[:, Cin:] == 0).all())


def test_bias_and_layout_restatements():
    b = R.special_values((5,), 6)
    for reps, rows in ((0, 4), (1, 1), (3, 3)):
        p = R.pack_bias(b, reps, 32)
        assert p.shape == (rows, 32) and bool((p[:, :5] == b).all()) and bool((R.bits(p[:, 5:]) == 0).all())
    x = R.special_values((2, 3, 5, 7), 7)
    for dtype in K.DTYPES:
        n = R.to_nhwc(x, 64, dtype)
        assert torch.equal(R.bits(n[..., :3]), R.bits(x.permute(0, 2, 3, 1).to(R.TORCH_DT[dtype])))
        assert bool((R.bits(n[..., 3:]) == 0).all())
        assert torch.equal(R.bits(R.to_nchw(n, 3)), R.bits(x.to(R.TORCH_DT[dtype]).float()))
    t = R.TIES
    q = torch.tensor(t, dtype=torch.float32).to(torch.bfloat16).float().tolist()
    assert q[:4] == [1.0, -1.0, 1 + 2.0 ** -6, -(1 + 2.0 ** -6)]                     # a tie down and a tie up, both signs
    assert int(R.bits(torch.tensor([t[4]], dtype=torch.float32).to(torch.bfloat16))[0]) == -0x8000      # -0.0 keeps its sign


def test_reduce_restatements_on_the_lattice_equal_integer_sums():
    g = torch.Generator().manual_seed(8)
    for r in K.REDUCE_SHAPES:
        S = 19
        slabs = torch.randint(-K.LATTICE_MAX, K.LATTICE_MAX + 1, (S, r.Np, r.taps, r.CAp + r.CBp), generator=g)
        tot = slabs.sum(0)                                                           # int64
        want = torch.empty((r.N, r.CA + r.CB, r.taps), dtype=torch.int64)
        for k in range(r.CA + r.CB):
            want[:, k, :] = tot[:r.N, :, k if k < r.CA else r.CAp + k - r.CA]
        got = R.reduce_exact(slabs.float(), r.N, r.CA, r.CB, r.CAp, r.CBp, r.taps)
        assert got.dtype == torch.float64 and torch.equal(got, want.double())
        bound = R.reduce_bound(slabs.float(), r.N, r.CA, r.CB, r.CAp, r.CBp, r.taps)
        assert bound.shape == got.shape and bool((bound >= 0).all())
    part = torch.randint(-8, 9, (33, 12, 2), generator=g).float()
    assert torch.equal(R.colsum_exact(part, 5, 4), part[:, 5:9, 0].long().sum(0).double())


# ---- coverage of the case tables -------------------------------------------------------------------------------------------
def test_conv_pack_cases_cover_what_they_promise():
    ids = [K.conv_case_id(c) for c in K.CONV_CASES]
    assert len(set(ids)) == len(ids)
    for shape in K.CONV_SHAPES:
        for dt, mode in itertools.product(K.DTYPES, (0, 1)):
            assert K.ConvPack(*K._geometry(*shape), 9, mode, dt) in K.CONV_CASES
            assert (K.ConvPack(*K._geometry(*shape), 1, mode, dt) in K.CONV_CASES) == (shape[2] == 0)
    for c in K.CONV_CASES:
        assert c.Coutp % 32 == 0 and c.CAp % K.CH[c.dtype] == 0 and c.CBp % K.CH[c.dtype] == 0 and (c.CB == 0) == (c.CBp == 0)
        assert c.Coutp >= c.Cout and c.CAp >= c.CA and c.CBp >= c.CB
    assert any(c.Coutp == K.pad32(c.Cout) + 32 and c.CAp == K.pad32(c.CA) + 32 for c in K.CONV_CASES)
    assert any(c.CAp == 16 for c in K.CONV_CASES) and any(c.CAp == 48 and c.CBp == 16 for c in K.CONV_CASES)
    past = [c for c in K.CONV_CASES if K.conv_total(c) > K.GRID_CAP * K.THREADS]
    assert sorted(c.mode for c in past) == [0, 1] and all(K.conv_kn(c) == (704, 672) and K.grid_trips(K.conv_total(c)) == 2 for c in past)
    assert all(K.grid_trips(K.conv_total(c)) == 1 for c in K.CONV_CASES if c not in past)


def test_both_kernel_cases_fail_every_fast_path_predicate_alone():
    tiles = [t for g in K.BOTH_GEOMETRIES for t in K.both_tiles(g)]
    assert any(src == "A" and all(p.values()) for src, p in tiles)
    assert any(src == "B" and all(p.values()) for src, p in tiles)
    assert ("B", {"inside": True, "cout": True, "cin4": True, "ci4": True}) in K.both_tiles(K._geometry(96, 36, 60))
    for name in ("inside", "cout", "cin4", "ci4"):
        alone = [(src, p) for src, p in tiles if not p[name] and all(v for k, v in p.items() if k != name)]
        assert alone, f"no tile fails `{name}` alone"
        if name == "ci4":
            assert any(src == "B" for src, _ in alone)
        if name == "inside":                       # a tile straddling the padding of source A
            assert any(src == "A" for src, _ in alone)
    assert ("B", {"inside": True, "cout": True, "cin4": True, "ci4": False}) in K.both_tiles(K._geometry(64, 34, 62))
    for g in K.BOTH_GEOMETRIES:
        assert g[3] % 32 == 0 and g[4] % 32 == 0 and g[5] % 32 == 0
        assert {K.BothCase(*g, dt, d) for dt in K.DTYPES for d in (True, False)} <= set(K.BOTH_CASES)


def test_pack_multi_tables_cover_what_they_promise():
    T = K.MULTI_TABLES
    assert sorted(len(t) for t in T.values()) == [1, 1, 1, 1, 2, 9, 64]
    assert {t[0].kind for t in T.values() if len(t) == 1} == {0, 1, 2, 3}
    nine = T["nine-interleaved"]
    assert {e.kind for e in nine} == {0, 1, 2, 3} and all(a.kind != b.kind for a, b in zip(nine, nine[1:]))
    assert any(e.dgrad for e in nine) and any(not e.dgrad and e.kind != 2 for e in nine)
    entries = [e for t in T.values() for e in t]
    assert {e.d0 for e in entries if e.kind == 2} >= {0, 1, 3} and not any(e.dgrad for e in entries if e.kind == 2)
    chunked = [K.entry_elements(e) for e in entries if e.kind in (1, 3)]
    assert any(n < K.CHUNK for n in chunked) and any(n % K.CHUNK == 0 for n in chunked)
    assert any(n > K.CHUNK and n % K.CHUNK for n in chunked)
    # a ConvTranspose weight holds Cinp * 4 * Coutp = a multiple of 4096 elements: only the 1x1 weights reach the other two
    assert all(K.entry_elements(e) % (2 * K.CHUNK) == 0 for e in entries if e.kind == 1)
    assert K.entry_elements(K.K3_SMALL) < K.CHUNK == K.entry_elements(K.K3_EXACT) and K.entry_elements(K.K3_REMAINDER) % K.CHUNK
    for kind in (0, 1, 3):                          # with and without a data-gradient destination
        assert {e.dgrad for e in entries if e.kind == kind} == {True, False}
    assert len(K.REPACK_WEIGHTS) == 70 > 64


def test_reduce_cases_cover_what_they_promise():
    assert {K.reduce_form(S) for S in K.LATTICE_S} == {"row", "wide"} == {K.reduce_form(S) for S in K.RANDOM_S}
    assert all(K.reduce_form(S) == "row" for S in K.ROW_S) and all(K.reduce_form(S) == "wide" for S in K.WIDE_S)
    assert any(S % 8 for S in K.ROW_S) and {8, 16} <= set(K.ROW_S)
    assert {K.wide_trips(S) for S in K.WIDE_S} >= {1, 2, 3, 4} and 129 in K.WIDE_S and max(K.LATTICE_S) == 512
    assert any(K.wide_trips(S) > 1 for S in K.RANDOM_S)
    assert max(K.LATTICE_S) * K.LATTICE_MAX < 2 ** 24 and K.SENTINEL > max(K.LATTICE_S) * K.LATTICE_MAX
    shapes = K.REDUCE_SHAPES
    assert any(r.Np > r.N for r in shapes) and any(r.CAp > r.CA for r in shapes) and any(r.CB and r.CBp > r.CB for r in shapes)
    assert any(K.reduce_nvec(r) < 16 for r in shapes) and any(K.reduce_nvec(r) % 16 for r in shapes if K.reduce_nvec(r) > 16)
    assert all((r.CAp + r.CBp) % 32 == 0 for r in shapes + [K.BIG_ROW])
    lds = (K.BIG_ROW.CA + K.BIG_ROW.CB) * K.BIG_ROW.taps * 4
    assert 48 * 1024 < lds <= 64 * 1024 and K.reduce_form(K.BIG_ROW_S) == "row"
    assert {c.rows for c in K.COLSUM_CASES} == set(K.COLSUM_ROWS) and {c.ncols for c in K.COLSUM_CASES} == set(K.COLSUM_NCOLS)
    assert len(K.COLSUM_CASES) == 45 and {c.col0 == 0 for c in K.COLSUM_CASES} == {True, False}
    assert all(c.col0 + c.ncols < c.Ctot for c in K.COLSUM_CASES)
    assert sorted({len(o) for o in K.JOB_ORDERS}) == [1, 2, 3, 4]
    for kind in "WRC":
        assert any(o[0] == kind for o in K.JOB_ORDERS) and any(o[-1] == kind and len(o) > 1 for o in K.JOB_ORDERS)
        assert any(kind in o[1:-1] for o in K.JOB_ORDERS)
    for o in K.JOB_ORDERS:
        for slot, kind in enumerate(o):
            spec = K.job_spec(kind, slot)
            if kind != "C":
                r, S = shapes[spec[0]], spec[1]
                assert K.reduce_form(S) == ("wide" if kind == "W" else "row")
                # a block that took the job before its own would touch row N of that job: inside the slab buffer's tail
                # and the destination's guard
                assert r.taps * (r.CAp + r.CBp) <= 4096 and (r.CA + r.CB) * r.taps <= 4096


def test_layout_cases_cover_what_they_promise():
    cap = K.GRID_CAP * K.THREADS
    assert any(c.Cp > K.pad32(c.C) for c in K.LAYOUT_CASES)
    assert [c for c in K.LAYOUT_CASES if K.to_nhwc_items(c) > cap and K.to_nchw_items(c) <= cap] == [K.LayoutCase(1, 1, 725, 725, 32, "fp32")]
    assert {c.dtype for c in K.LAYOUT_CASES if K.to_nchw_items(c) > cap} == set(K.DTYPES)
    assert all(K.grid_trips(K.to_nchw_items(c)) == 2 for c in K.LAYOUT_CASES if c.H == 683)
    assert K.grid_trips(K.to_nhwc_items(K.LayoutCase(1, 1, 725, 725, 32, "fp32"))) == 2
