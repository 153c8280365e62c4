"""GPU (-m gpu): the channel-vector streaming kernels -- BatchNorm finalisation, the BN + ReLU apply pass (alone and with the
2x2 pooling), the three BatchNorm backward forms, MaxPool2d(2,2) forward / backward (plain and with the BatchNorm reductions) and
the channel sum -- driven directly through _lib.call on inputs from oracle.fill (no RNG, no model), every output buffer pre-filled
with NaN (so a store past the written range, or a missing one, changes a digest) and compared by SHA-1 with
tests/golden/bn_pool_bits.json.  The digests are folded: per entry and lane case, and per buffer name, one SHA-1 over
"case:digest;" of that buffer in every case of the group, in case order.

The fixture is a record of the library BEFORE these kernels were folded onto one lane map, one pixel walk, one block row reduce,
one partial-row sum, one statistics finish and one 2x2 window (csrc/channel_lanes.hpp): the code may be
rearranged, the bytes may not change.  The head entries that share the header are held by tests/golden/loss_bits.json.

Shapes, the smallest at which each piece can go wrong (the largest tensor is about 17 MB):
  lanes   both dtypes; Cp 32 (64 / 32 pixel rows per block), Cp 96 (12 / 24 channel vectors: 21 / 10 rows, 4 / 16 idle threads),
          Cp 1056 bf16 and 544 fp32 (132 / 136 vectors: 2 rows, a second channel block with 4 / 8 active vectors); C_real = Cp - 3
  walk    P = 1, rows + 1 (two blocks, tail only), 4 * 512 * rows + rows + 1 (one trip of the four-in-flight loop plus a tail with the
          reduce grid at its cap of 512 blocks), 4096 * rows + 3 (the second trip of the apply grid); at Cp 32 also 31 / 32 / 33 reduce
          blocks; the backward in place (dz == dy) and out of place
  rows    segk_bn_relu_bwd_from_part with 1, 33, 512, 513, 1024 partial rows (the second trip of the sixteen-in-flight walk);
          segk_bn_finalize training with MT 1, 33, 512, 513, 1024 (one block per 32 channels) and 1025, 1057 (the ticket kernel, chunks
          of 33 and 34 rows), C 32 and 64, count 1 and large, conv bias and running statistics null and present; eval mode with and
          without the mean / rstd outputs
  window  (B, H, W) = (1, 2, 2), (2, 5, 7), (1, 4, 6); Cp 32, 64 and 96 (96: plain forms only, the statistics form must report 0
          blocks); accumulate 0 / 1; ties inside a window (inputs on a grid of 1/4); the statistics form without z, and with z while
          one channel has scale = 0 and one 16 |scale| < |shift|; (2, 258, 256) at Cp 32 fp32: 264 192 items, more than the
          1024 x 256 of one trip of the statistics form's grid

Set SEGK_BN_POOL_BITS_OUT=<file> to write the record there instead of comparing (never from the code under test: point SEGK_LIB at
a library built from the parent commit)."""
import hashlib
import json
import os

import pytest
import torch

from oracle.fill import fill

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_pool_bits.json")
OUT = os.environ.get("SEGK_BN_POOL_BITS_OUT")
NAN = float("nan")
SEGK_DT = {torch.float32: 0, torch.bfloat16: 1}
NAME = {torch.float32: "fp32", torch.bfloat16: "bf16"}
LANES = [(torch.bfloat16, 32), (torch.float32, 32), (torch.bfloat16, 96), (torch.float32, 96), (torch.bfloat16, 1056),
         (torch.float32, 544)]
ROWS = (1, 33, 512, 513, 1024)
_RECORD = {}
_FOLD = {}       # group -> buffer name -> running SHA-1


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    if OUT and _RECORD:
        with open(OUT, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sorted(_RECORD.items()))
                    + "\n}\n")


@pytest.fixture(scope="module")
def want():
    if OUT:
        return None
    with open(GOLDEN) as f:
        return json.load(f)


def dev(t):
    return t.cuda().contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def nans(n, dtype=torch.float32):
    return torch.full((int(n),), NAN, dtype=dtype, device="cuda")


def check(group, case, **bufs):
    """fold the SHA-1 of every buffer of a case into its group"""
    torch.cuda.synchronize()
    for name, t in bufs.items():
        if t is not None:
            digest = hashlib.sha1(t.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
            _FOLD.setdefault(group, {}).setdefault(name, hashlib.sha1()).update(f"{case}:{digest};".encode())


def settle(want, prefix):
    """compare (or record) the groups that begin with `prefix`"""
    got = {g: {n: h.hexdigest() for n, h in bufs.items()} for g, bufs in _FOLD.items() if g.startswith(prefix)}
    assert got
    if OUT:
        _RECORD.update(got)
        return
    assert sorted(got) == sorted(g for g in want if g.startswith(prefix)), "the groups of the fixture are not those of the test"
    bad = [f"{g}: " + ", ".join(n for n in got[g] if got[g][n] != want[g].get(n)) + " differ" for g in sorted(got) if got[g] != want[g]]
    assert not bad, "\n".join(bad)


def bn_vectors(Cp, C, seed, special=False):
    """scale (negative on every fifth channel), shift, mean, rstd, zero beyond C; special: scale = 0 on channel 2 and
    16 |scale| < |shift| on channel 5 (the channels whose xhat cannot be recovered from y)"""
    gamma, beta, mean, rstd = fill((Cp,), seed, 0.5, 1.5), fill((Cp,), seed + 1, -0.5, 0.5), fill((Cp,), seed + 2, -0.3, 0.3), \
        fill((Cp,), seed + 3, 0.5, 2.0)
    gamma[1::5] *= -1
    if special:
        gamma[2] = 0.0
        beta[2] = 0.25            # y = relu(shift) > 0 everywhere: the ReLU is active
        gamma[5] = 1.0 / 64
        beta[5] = 0.5
        mean[5] = 0.0
    scale = gamma * rstd
    bn = [scale, beta - mean * scale, mean, rstd]
    for v in bn:
        v[C:] = 0
    return bn


# ---- lanes and pixel walk: apply, the backward forms, the channel sum -----------------------------------------------------------
def lane_rows(Cp, dtype):
    cvec = Cp // (8 if dtype == torch.bfloat16 else 4)
    return 256 // min(cvec, 128)


def walk_pixels(Cp, dtype):
    rows = lane_rows(Cp, dtype)
    P = [1, rows + 1, 4 * 512 * rows + rows + 1, 4096 * rows + 3]
    if Cp == 32:
        P[2:2] = [30 * rows + 1, 31 * rows + 1, 32 * rows + 1]        # 31 / 32 / 33 reduce blocks
    return P


@pytest.mark.parametrize("dtype,Cp", LANES, ids=[f"{NAME[d]}-Cp{c}" for d, c in LANES])
def test_lanes_walk(lib, want, dtype, Cp):
    C, dt, lane = Cp - 3, SEGK_DT[dtype], f"Cp{Cp}{NAME[dtype]}"
    pixels = walk_pixels(Cp, dtype)
    zall, dall = fill((pixels[-1], Cp), 10 + Cp, -2, 2), fill((pixels[-1], Cp), 11 + Cp, -1, 1)
    zall[:, C:] = 0; dall[:, C:] = 0
    zall, dall = dev(zall.to(dtype)), dev(dall.to(dtype))
    bnv = [dev(v) for v in bn_vectors(Cp, C, 20 + Cp)]
    bn = [v.data_ptr() for v in bnv]
    for P in pixels:
        z, dy = zall[:P].contiguous(), dall[:P].contiguous()
        nb = lib.query("segk_bn_bwd_blocks", P, Cp, dt)
        assert nb == min(-(-P // lane_rows(Cp, dtype)), 512)
        y = nans(P * Cp, dtype)
        lib.call("segk_bn_relu_apply", z.data_ptr(), y.data_ptr(), bn[0], bn[1], P, Cp, dt, None)
        check(f"bn_relu_apply/{lane}", f"P{P}", y=y)
        for inplace in (False, True):
            dz = dy.clone() if inplace else nans(P * Cp, dtype)
            part, dgamma, dbeta, coef = nans(nb * Cp * 2), nans(C), nans(C), nans(2 * Cp)
            lib.call("segk_bn_relu_bwd", dz.data_ptr() if inplace else dy.data_ptr(), z.data_ptr(), dz.data_ptr(), *bn, P, Cp, C,
                     part.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), dt, None)
            check(f"bn_relu_bwd/{lane}", f"P{P}/inplace{int(inplace)}", dz=dz, part=part, dgamma=dgamma, dbeta=dbeta, coef=coef)
        part, dgamma, dbeta, coef = nans(nb * Cp * 2), nans(C), nans(C), nans(2 * Cp)
        lib.call("segk_bn_relu_bwd_stats", dy.data_ptr(), z.data_ptr(), *bn, P, Cp, C, part.data_ptr(), dgamma.data_ptr(),
                 dbeta.data_ptr(), coef.data_ptr(), dt, None)
        check(f"bn_relu_bwd_stats/{lane}", f"P{P}", part=part, dgamma=dgamma, dbeta=dbeta, coef=coef)
        part, out = nans(nb * Cp), nans(C)
        lib.call("segk_channel_sum", dy.data_ptr(), P, Cp, C, part.data_ptr(), out.data_ptr(), dt, None)
        check(f"channel_sum/{lane}", f"P{P}", part=part, out=out)
    for entry in ("bn_relu_apply", "bn_relu_bwd", "bn_relu_bwd_stats", "channel_sum"):
        settle(want, f"{entry}/{lane}")


# ---- the float64 sum of partial rows ---------------------------------------------------------------------------------------------
def test_from_part(lib, want):
    P = 67
    for dtype, Cp in ((torch.bfloat16, 32), (torch.float32, 96)):
        C, dt = Cp - 3, SEGK_DT[dtype]
        z, dy = fill((P, Cp), 30 + Cp, -2, 2), fill((P, Cp), 31 + Cp, -1, 1)
        z[:, C:] = 0; dy[:, C:] = 0
        z, dy = dev(z.to(dtype)), dev(dy.to(dtype))
        bnv = [dev(v) for v in bn_vectors(Cp, C, 40 + Cp)]
        for nb in ROWS:
            part = dev(fill((nb, Cp, 2), 50 + nb, -1, 1))
            for inplace in (False, True):
                dz = dy.clone() if inplace else nans(P * Cp, dtype)
                dgamma, dbeta, coef = nans(C), nans(C), nans(2 * Cp)
                lib.call("segk_bn_relu_bwd_from_part", dz.data_ptr() if inplace else dy.data_ptr(), z.data_ptr(), dz.data_ptr(),
                         *[v.data_ptr() for v in bnv], P, Cp, C, part.data_ptr(), nb, dgamma.data_ptr(), dbeta.data_ptr(),
                         coef.data_ptr(), dt, None)
                check(f"bn_relu_bwd_from_part/Cp{Cp}{NAME[dtype]}", f"nb{nb}/inplace{int(inplace)}", dz=dz, dgamma=dgamma, dbeta=dbeta,
                      coef=coef)
    settle(want, "bn_relu_bwd_from_part/")


@pytest.mark.parametrize("C", [32, 64])
def test_bn_finalize(lib, want, C):
    Cr = C - 3
    gamma, beta, bias = dev(fill((C,), 60, 0.5, 1.5)), dev(fill((C,), 61, -0.5, 0.5)), dev(fill((C,), 62, -0.1, 0.1))
    for MT in ROWS + (1025, 1057):
        n = lib.query("segk_bn_stats_floats", MT, C)
        assert n == MT * C * 2 + 32 * C * 4
        sums = torch.stack([fill((MT, C), 63 + MT, -1, 1), fill((MT, C), 64 + MT, 0.5, 2)], dim=2)        # [MT][C][2]: sum, sum of squares
        for count in (1.0, 4096.0 * MT):
            for extras in (False, True):
                stats = nans(n)                                 # the partials, then the ticket kernel's float64 scratch
                stats[:MT * C * 2] = dev(sums).reshape(-1)
                rmean, rvar = (dev(fill((C,), 65, -0.3, 0.3)), dev(fill((C,), 66, 0.5, 2))) if extras else (None, None)
                scale, shift, mean, rstd = nans(C), nans(C), nans(C), nans(C)
                lib.call("segk_bn_finalize", stats.data_ptr(), MT, C, Cr, count, ptr(bias) if extras else None, gamma.data_ptr(),
                         beta.data_ptr(), ptr(rmean), ptr(rvar), 0.1, 1e-5, 1, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                         rstd.data_ptr(), None)
                check(f"bn_finalize/C{C}", f"train/MT{MT}/count{count}/extras{int(extras)}", stats=stats, rmean=rmean, rvar=rvar,
                      scale=scale, shift=shift, mean=mean, rstd=rstd)
    for outputs in (False, True):
        for with_bias in (False, True):
            rmean, rvar = dev(fill((C,), 65, -0.3, 0.3)), dev(fill((C,), 66, 0.5, 2))
            scale, shift = nans(C), nans(C)
            mean, rstd = (nans(C), nans(C)) if outputs else (None, None)
            lib.call("segk_bn_finalize", None, 0, C, Cr, 0.0, ptr(bias) if with_bias else None, gamma.data_ptr(), beta.data_ptr(),
                     rmean.data_ptr(), rvar.data_ptr(), 0.1, 1e-5, 0, scale.data_ptr(), shift.data_ptr(), ptr(mean), ptr(rstd), None)
            check(f"bn_finalize/C{C}", f"eval/outputs{int(outputs)}/bias{int(with_bias)}", rmean=rmean, rvar=rvar, scale=scale,
                  shift=shift, mean=mean, rstd=rstd)
    settle(want, f"bn_finalize/C{C}")


# ---- the 2x2 window --------------------------------------------------------------------------------------------------------------
WINDOWS = [(1, 2, 2), (2, 5, 7), (1, 4, 6)]


def window_inputs(B, H, W, Cp, dtype, seed):
    """z on a grid of 1/4 in [-2, 2] (ties inside the windows), y = relu(z * scale + shift) rounded to dtype, the pooled gradient dy
    and an earlier gradient to accumulate onto; scale = 0 on channel 2 and 16 |scale| < |shift| on channel 5"""
    C = Cp - 3
    bn = bn_vectors(Cp, C, seed, special=True)
    z = torch.round(fill((B, H, W, Cp), seed + 4, -2, 2) * 4) / 4
    z[..., C:] = 0
    z = z.to(dtype)
    y = (z.float() * bn[0] + bn[1]).clamp(min=0).to(dtype)
    dy = fill((B, H // 2, W // 2, Cp), seed + 5, -1, 1).to(dtype)
    dx0 = fill((B, H, W, Cp), seed + 6, -1, 1).to(dtype)
    return dev(z), dev(y), dev(dy), dev(dx0), [dev(v) for v in bn]


def run_window(lib, B, H, W, Cp, dtype, plain=True):
    dt, lane, case = SEGK_DT[dtype], f"Cp{Cp}{NAME[dtype]}", f"{B}x{H}x{W}"
    z, y, dy, dx0, bnv = window_inputs(B, H, W, Cp, dtype, 70 + Cp + H)
    bn = [v.data_ptr() for v in bnv]
    n, npool = B * H * W * Cp, B * (H // 2) * (W // 2) * Cp
    if plain:
        yo, pooled = nans(n, dtype), nans(npool, dtype)
        lib.call("segk_bn_relu_apply_pool", z.data_ptr(), yo.data_ptr(), pooled.data_ptr(), bn[0], bn[1], B, H, W, Cp, dt, None)
        check(f"bn_relu_apply_pool/{lane}", case, y=yo, pooled=pooled)
        pooled = nans(npool, dtype)
        lib.call("segk_maxpool2x2_fwd", y.data_ptr(), pooled.data_ptr(), B, H, W, Cp, dt, None)
        check(f"maxpool2x2_fwd/{lane}", case, pooled=pooled)
        for acc in (0, 1):
            dx = dx0.clone().reshape(-1) if acc else nans(n, dtype)
            lib.call("segk_maxpool2x2_bwd", y.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, H, W, Cp, acc, dt, None)
            check(f"maxpool2x2_bwd/{lane}", f"{case}/acc{acc}", dx=dx)
    nb = lib.query("segk_maxpool_bwd_stat_blocks", B, H, W, Cp, dt)
    if Cp == 96:                 # 12 / 24 channel vectors: not a power of two
        assert nb == 0
        return
    assert nb == min(-(-(B * ((H + 1) // 2) * ((W + 1) // 2) * (Cp // (8 if dt else 4))) // 256), 1024)
    for acc in (0, 1) if plain else (0,):
        for with_z in (False, True):
            dx = dx0.clone().reshape(-1) if acc else nans(n, dtype)
            part = nans(nb * Cp * 2)
            lib.call("segk_maxpool2x2_bwd_bnstat", y.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, H, W, Cp, acc, *bn, part.data_ptr(),
                     z.data_ptr() if with_z else None, dt, None)
            check(f"maxpool2x2_bwd_bnstat/{lane}", f"{case}/acc{acc}/z{int(with_z)}", dx=dx, part=part)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_window(lib, want, dtype):
    for Cp in (32, 64, 96):
        for B, H, W in WINDOWS:
            run_window(lib, B, H, W, Cp, dtype)
    if dtype == torch.float32:
        run_window(lib, 2, 258, 256, 32, dtype, plain=False)       # the second trip of the statistics form's grid
    for entry in ("bn_relu_apply_pool", "maxpool2x2_fwd", "maxpool2x2_bwd", "maxpool2x2_bwd_bnstat"):
        for Cp in (32, 64, 96):
            if entry != "maxpool2x2_bwd_bnstat" or Cp != 96:
                settle(want, f"{entry}/Cp{Cp}{NAME[dtype]}")

