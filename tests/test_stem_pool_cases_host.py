"""CPU: the case tables of tests/stem_pool_cases.py reach every regime of the stem's streaming loops and of the pooling
kernels' grid-stride loops (from the restated launch arithmetic, NUM_CUS = 256), the lattice runs are exact by the
references alone, and the references of tests/stem_pool_reference.py agree with torch on small problems."""
import pytest
import torch
import torch.nn.functional as F

import stem_pool_cases as K
import stem_pool_reference as R
from stem_pool_cases import (FINALIZE_CASES, POOL_CASES, POOL_SMALL, POOL_STRIDE, REF_MADD_CAP, STAT_CASES, STEM_CASES, STEM_S,
                             STEM_WGRAD_DENSE, PoolCase, StemCase)


def test_stem_launch_arithmetic():
    assert STEM_S == 4096
    c = StemCase(1, 3, 64, 64)                 # the largest case of the first stem test: 256 blocks, 32 workgroups, no pair
    assert (K.stem_nblk(c), K.stem_rows(c), K.stem_wgrad_slabs(c)) == (256, 32, 32)
    assert set(K.stem_pass_patterns(c)) == {(False,)}
    c = StemCase(32, 3, 512, 512)              # the full-size step: 524288 blocks, capped grid
    assert (K.stem_rows(c), K.stem_wgrad_slabs(c), K.stem_step(c)) == (512, 512, 4096)
    assert K.stem_rows(StemCase(1, 4, 8, 16)) == 0 and K.stem_rows(StemCase(1, 3, 8, 24)) == 0
    assert K.stem_rows(StemCase(1, 3, 8, 16), dtype="fp32") == 0 and K.stem_rows(StemCase(1, 3, 8, 16), Cout=32) == 0


def test_stem_table_reaches_every_regime():
    S = STEM_S
    by = {}
    for c in STEM_CASES:
        assert K.stem_rows(c) > 0 and K.stem_wgrad_slabs(c) > 0
        by.setdefault(K.stem_regime(c), []).append(c)
        assert K.stem_nblk(c) * 16 * 64 * 2 <= 36 * 2 ** 20          # z of at most about 35 MB
        assert K.stem_nblk(c) * 16 * 9 * c.Cin * 64 <= REF_MADD_CAP
    assert set(by) == {"single", "mixed-pair", "all-pair", "second-pass-tail", "paired-second-pass", "third-pass"}
    pat = {c: K.stem_pass_patterns(c) for c in STEM_CASES}
    # nblk <= S: one single block per wave; some with idle waves in the last workgroup (nblk no multiple of 8)
    for c in by["single"]:
        assert set(pat[c]) <= {(False,), ()}
    assert any(K.stem_nblk(c) % 8 != 0 and () in pat[c] for c in by["single"])
    # S < nblk < 2S: some waves pair, others do not
    assert all(set(pat[c]) == {(True,), (False,)} for c in by["mixed-pair"])
    # nblk == 2S: every wave pairs
    assert all(K.stem_nblk(c) == 2 * S and pat[c] == {(True,): S} for c in by["all-pair"])
    # 2S < nblk < 3S: a second pass of one block (the odd tail) on some waves
    assert all(set(pat[c]) == {(True, False), (True,)} for c in by["second-pass-tail"])
    # 3S < nblk <= 4S: a paired second pass beside a single one
    assert all(set(pat[c]) == {(True, True), (True, False)} and K.stem_nblk(c) > 3 * S for c in by["paired-second-pass"])
    # nblk > 4S: a third pass
    assert all(set(pat[c]) == {(True, True, False), (True, True)} and K.stem_nblk(c) > 4 * S for c in by["third-pass"])
    assert {c.Cin for c in STEM_CASES} == {1, 2, 3}
    assert any(c.W == 16 for c in STEM_CASES) and any(c.H == 1 for c in STEM_CASES)
    assert sum(c.H % 2 == 1 for c in STEM_CASES) >= len(STEM_CASES) - 1
    # the weight gradient: one trip, mixed one and two trips, three or more; idle waves in the last workgroup
    regs = {K.stem_wgrad_regime(c) for c in STEM_CASES}
    assert regs == {"one-trip", "mixed-trips", "two-trips", "three-or-more"}
    assert any(K.stem_nblk(c) % 8 != 0 and K.stem_wgrad_trips(c)[0] == 0 for c in STEM_CASES)
    assert {K.stem_wgrad_regime(c) for c in STEM_WGRAD_DENSE} == {"one-trip", "mixed-trips"}
    assert max(K.stem_wgrad_trips(c)[1] for c in STEM_CASES) >= 5


@pytest.mark.parametrize("case", STEM_CASES, ids=K.stem_case_id)
def test_stem_probes_and_lattices(case):
    c = case
    pts = K.stem_probe_pixels(c)
    assert (0, 0, 0) in pts and (0, c.H - 1, c.W - 1) in pts and (c.B - 1, c.H - 1, c.W - 1) in pts
    if c.W > 16:
        assert (0, c.H // 2, 15) in pts and (0, c.H // 2, 16) in pts
    if c.B > 1:
        assert (0, c.H - 1, c.W // 3) in pts and (1, 0, c.W // 3) in pts
    assert sorted(p for g in K.stem_probe_passes(c) for p in g) == sorted(pts)
    # forward lattice: exact by the reference alone, and no 16-pixel block is all zero (a dropped or doubled block shows)
    x, w = R.stem_inputs(c, "lattice")
    z = R.stem_reference(x, w)
    assert R.lattice_is_exact(z)
    assert bool((z.reshape(-1, 16, 64) != 0).any(2).any(1).all())
    s1, s2 = R.channel_stats(z)
    assert bool((s2 > 0).all())
    # weight-gradient lattice: every sum |dz col| below 2^24, every block contributes to some element
    x, dz = R.stem_wgrad_inputs(c, "lattice")
    ref, A = R.stem_wgrad_reference(x, dz)
    assert bool((A < 2 ** 24).all()) and bool((ref == ref.round()).all())
    col = R.im2col(x).reshape(-1, 16, 9 * c.Cin)
    assert bool(((dz.float().reshape(-1, 16, 64) != 0).any(2).any(1) & (col != 0).any(2).any(1)).all())


def test_rne_bf16_is_round_to_nearest_even():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, 1.0 + 2 ** -8 + 2 ** -20, -1.00390625, 3.3895313892515355e38, 1e-40, 0.0])
    # a tie goes to the even neighbour (down at 1 + 2^-8, up at 1 + 3 * 2^-8), anything above a tie goes up
    assert torch.equal(R.rne_bf16(x)[:5], torch.tensor([1.0, 1.0, 1.015625, 1.0078125, -1.0]))
    assert torch.equal(R.rne_bf16(x), x.to(torch.bfloat16).float())
    g = torch.Generator().manual_seed(5)
    r = torch.rand((4096,), generator=g) * 4 - 2
    assert torch.equal(R.rne_bf16(r), r.to(torch.bfloat16).float())


def test_stem_references_agree_with_torch():
    c = StemCase(2, 3, 5, 16)
    x, w = R.stem_inputs(c, "dense")
    z = R.stem_reference(x, w)
    want = F.conv2d(R.rne_bf16(x).double(), R.rne_bf16(w).double(), padding=1).permute(0, 2, 3, 1)
    assert (z - want).abs().max() < 1e-12
    x, dz = R.stem_wgrad_inputs(c, "dense")
    wz = torch.zeros((64, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(R.rne_bf16(x).double(), wz, padding=1).backward(dz.double().permute(0, 3, 1, 2))
    assert (R.stem_wgrad_reference(x, dz)[0] - wz.grad.reshape(64, 27)).abs().max() < 1e-12
    probes = K.stem_probe_passes(c)[0]
    x, w = R.stem_inputs(c, "impulse", probes)
    assert torch.equal(R.stem_impulse_expected(c, w, probes), R.stem_reference(x, w))
    pts = K.stem_probe_pixels(c)
    x, dz = R.stem_wgrad_inputs(c, "impulse", pts)
    assert torch.equal(R.stem_wgrad_impulse_expected(c, x, pts), R.stem_wgrad_reference(x, dz)[0][:, :27])
    xn = R.stem_xn(x)
    assert xn.shape == (2, 5, 16, 32) and bool((xn[..., 3:] == 0).all())
    assert torch.equal(xn[..., :3].float(), x.to(torch.bfloat16).float().permute(0, 2, 3, 1))


def test_pool_launch_arithmetic_and_strides():
    trips = lambda dt, shape, k: K.pool_trips(PoolCase(dt, *shape), k)
    # the first tests' largest problems do not stride
    assert trips("bf16", (2, 16, 24, 64), "stat") == 1 and trips("fp32", (1, 4, 6, 1024), "bwd") == 1
    for c in POOL_SMALL:
        assert all(K.pool_trips(c, k) == 1 for k in ("fwd", "bwd"))
    for c in POOL_STRIDE:                      # all three uncapped kernels stride, barely: the smallest such odd x odd image
        assert [K.pool_trips(c, k) for k in ("fwd", "bwd")] == [2, 2] and K.pool_grid(c, "fwd") == 8192
        assert c.H % 2 == 1 and c.W % 2 == 1
        smaller = c._replace(H=c.H - 2)
        assert K.pool_trips(smaller, "fwd") == 1
    assert K.pool_trips(PoolCase("bf16", 1, 259, 261, 1024), "fwd") == 2 and K.pool_trips(PoolCase("fp32", 1, 259, 261, 1024), "fwd") == 3
    want = {"bf16-2x259x261x64-acc-deg": 2, "bf16-2x259x261x128-acc-deg": 3, "fp32-2x259x261x64-acc-deg": 3,
            "fp32-1x67x67x1024-acc": 2, "bf16-2x259x261x64-acc-noz": 2}
    got = {K.stat_case_id(s): K.pool_trips(s.case, "stat") for s in STAT_CASES if K.pool_trips(s.case, "stat") > 1}
    assert got == want
    assert K.pool_items(PoolCase("bf16", 2, 259, 261, 64), "stat") == 272480                 # 1.04 x 1024 x 256
    assert K.pool_grid(PoolCase("fp32", 1, 67, 67, 1024), "stat") == 1024
    assert 1024 // K.pool_vec("fp32") == 256
    assert K.pool_grid(PoolCase("bf16", 1, 8, 8, 96), "stat") == 0 and K.pool_grid(PoolCase("fp32", 1, 8, 8, 96), "stat") == 0
    assert K.pool_grid(PoolCase("bf16", 1, 8, 8, 4096), "stat") == 0                          # 512 channel vectors
    assert all(K.pool_grid(s.case, "stat") > 0 for s in STAT_CASES)


def test_pool_table_conditions():
    imgs = {(c.H % 2, c.W % 2) for c in POOL_SMALL}
    assert imgs == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert any(c.H == 2 or c.W == 2 for c in POOL_SMALL) and any(c.H == 3 or c.W == 3 for c in POOL_SMALL)
    assert any(c.H == 2 for c in POOL_SMALL) and any(c.W == 2 for c in POOL_SMALL)
    assert {c.Cp for c in POOL_SMALL} == {32, 96, 64, 256, 1024} and any(c.B > 1 for c in POOL_SMALL)
    assert {c.dtype for c in POOL_CASES} == {"bf16", "fp32"}
    assert all(K.pool_elements(c) <= REF_MADD_CAP for c in POOL_CASES + [s.case for s in STAT_CASES])
    strid = [s for s in STAT_CASES if K.pool_trips(s.case, "stat") > 1]
    assert any(s.degenerate for s in strid) and any(not s.with_z and not s.degenerate for s in strid)
    assert all(not s.degenerate for s in STAT_CASES if not s.with_z)


@pytest.mark.parametrize("case", POOL_SMALL, ids=K.pool_case_id)
def test_pool_references_agree_with_torch(case):
    c = case
    x, dy, dx0 = R.pool_inputs(c)
    win = R.windows(x.float())
    n = (torch.arange(win.shape[0] * win.shape[1] * win.shape[2]).reshape(*win.shape[:3], 1) + torch.arange(c.Cp)) % 8
    m = win.amax(3)
    for kind, ks in ((1, (1, 2)), (2, (2, 3)), (3, (0, 3)), (4, (0, 1, 2, 3))):          # the planted ties survive the rounding
        for k in ks:
            assert bool((win[:, :, :, k][n == kind] == m[n == kind]).all())
    if (n == 5).any():
        assert bool((m[n == 5] < 0).all())
    xt = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    yt = F.max_pool2d(xt, 2, 2)
    assert torch.equal(R.maxpool_fwd_reference(x).float(), yt.detach().permute(0, 2, 3, 1))
    yt.backward(dy.float().permute(0, 3, 1, 2))
    assert torch.equal(R.maxpool_bwd_reference(x, dy).float(), xt.grad.permute(0, 2, 3, 1))
    acc = R.maxpool_bwd_reference(x, dy, dx0)
    assert acc.dtype == x.dtype and torch.equal(acc, (dx0.float() + xt.grad.permute(0, 2, 3, 1)).to(x.dtype))
    z, scale, shift = R.apply_pool_inputs(c)
    y, pooled = R.apply_pool_reference(z, scale, shift, x.dtype)
    dead = (n == 6) & ~((scale == 0) & (shift > 0))                  # (a channel with scale == 0 holds relu(shift) everywhere)
    assert dead.any() and bool((R.windows(y.float())[dead.unsqueeze(3).expand(-1, -1, -1, 4, -1)] == 0).all())
    assert bool((pooled.float()[dead] == 0).all()) and bool((y.float() >= 0).all())


def test_stat_reference_small():
    s = next(s for s in STAT_CASES if s.degenerate and s.case.Cp == 64 and s.case.dtype == "bf16" and s.case.H < 10)
    z, y, dy, dx0, scale, shift, mean, rstd = R.stat_inputs(s)
    deg = K.stat_degenerate_channels(64)
    fz = R.from_z_channels(scale, shift, "bf16", True)
    assert set(fz.nonzero().flatten().tolist()) == {ch for d in deg for ch in range(d // 8 * 8, d // 8 * 8 + 8)}
    assert not R.from_z_channels(scale, shift, "bf16", False).any()
    for ch, kind in deg.items():
        if kind == "zero+":
            assert scale[ch] == 0 and shift[ch] > 0 and bool((y[..., ch] > 0).all())
        elif kind == "zero-":
            assert scale[ch] == 0 and shift[ch] < 0 and bool((y[..., ch] == 0).all())
        else:
            assert abs(float(scale[ch]) * 1000 / abs(float(shift[ch])) - 1) < 1e-6
    dx = R.maxpool_bwd_reference(y, dy, dx0)
    pre = R.maxpool_bwd_presum(y, dy, dx0)
    assert pre.dtype == torch.float32 and torch.equal(pre.to(dx.dtype), dx) and not torch.equal(pre, dx.float())
    r = R.stat_reference(s, z, y, dx, scale, shift, mean, rstd, pre)
    ok = ~r["from_z"]
    # what the recovery from y costs stays inside its bound, from the references alone
    assert bool(((r["sum_gx"] - r["true_gx"]).abs() <= r["bound_true"])[ok].all())
    assert bool((r["sum_gx"] == r["true_gx"])[r["from_z"]].all())
    # bf16 with accumulate: the kernel's addends are the fp32 gradient before its store; the stored sums lie within what
    # that store moved, and the from_z channels' sum g xhat takes the stored gradient
    live = r["sum_g"] != 0
    assert bool((r["sum_g_kernel"] != r["sum_g"])[live].any())
    assert bool(((r["sum_g_kernel"] - r["sum_g"]).abs() <= r["bound_g"] - r["bound_g_kernel"] + 1e-12).all())
    assert bool(((r["sum_gx_kernel"] - r["sum_gx"]).abs() <= r["bound_gx"] - r["bound_gx_kernel"] + 1e-12).all())
    assert bool((r["sum_gx_kernel"] == r["sum_gx"])[r["from_z"]].all())
    assert bool((r["bound_gx_kernel"] == r["bound_gx"])[r["from_z"]].all())
    # fp32, or no accumulate: nothing is rounded on the way to the store, and the two pairs of sums and bounds coincide
    for s2 in (next(t for t in STAT_CASES if t.accumulate and t.case.dtype == "fp32" and t.case.H < 10),
               next(t for t in STAT_CASES if not t.accumulate and t.case.dtype == "bf16")):
        z, y, dy, dx0, scale, shift, mean, rstd = R.stat_inputs(s2)
        dx0 = dx0 if s2.accumulate else None
        dx, pre = R.maxpool_bwd_reference(y, dy, dx0), R.maxpool_bwd_presum(y, dy, dx0)
        assert torch.equal(pre, dx.float())
        r = R.stat_reference(s2, z, y, dx, scale, shift, mean, rstd, pre)
        assert all(torch.equal(r[k], r[k + "_kernel"]) for k in ("sum_g", "sum_gx", "bound_g", "bound_gx"))


@pytest.mark.parametrize("case", FINALIZE_CASES, ids=str)
def test_finalize_rows_and_reference(case):
    MT, C = case
    rows, const = R.finalize_rows(MT, C)
    count = float(MT * 4)
    Cr = C - 5 if C > 32 else C
    one = torch.ones(C)
    r = R.finalize_reference(rows, count, Cr, one, 0 * one, None, 0 * one, one, 0.1, 1e-5, True)
    raw = r["raw_var"]
    assert bool((raw[const].abs() < 1e-6).all())                      # the constant channels cancel ...
    if MT > 1:
        assert bool((raw[const] < 0).any()) and bool((raw[const] >= 0).any())     # ... to either side of the clamp
    assert bool((r["rstd"][0][const][raw[const] <= 0] == 1.0 / (torch.tensor(R.f32(1e-5), dtype=torch.float64)).sqrt()).all())
    other = [ch for ch in range(Cr) if ch not in const]
    assert bool((raw[other] > 0).all())
    assert all(bool((e >= 0).all()) for _, e in (r[k] for k in ("mean", "rstd", "scale", "shift", "rmean", "rvar")))
