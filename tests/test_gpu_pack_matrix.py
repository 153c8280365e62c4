"""GPU (-m gpu): the kernels of csrc/pack.hip that carry data between the compute kernels -- the weight packs, the one-launch
re-pack, the NCHW <-> NHWC layout passes and the weight-gradient reductions -- through the C ABI against the restatements of
tests/pack_reference.py, on the case tables of tests/pack_cases.py (tests/test_pack_cases_host.py proves on the CPU that the
restatements are right and that the tables reach every branch).

Every destination is pre-filled with a NaN pattern and followed by a guard of the same pattern: after the call every element
must be overwritten and the guard untouched.

  packs, layout   a permutation with a defined rounding: the device's BIT PATTERNS equal the restatement's (-0.0 and the
                  direction of a bf16 tie count; padding is +0).
  reduce lattice  slabs of integers in [-8, 8], the sentinel 2^20 in every padded column and every row n >= N: all sums are
                  exact in fp32 in any order, so the result equals the float64 sum; a slab added twice, dropped, or a leak
                  from the padding is a wrong number at a known place.
  reduce random   within the derived bound of the float64 sum (pack_reference's docstring), bit-identical on a second run,
                  and the multi entry bit-identical to the single entry.
Set SEGK_PACK_PARITY_OUT=<file> to record the worst error / bound per kernel form (profiles/pack_reduce_matrix_parity.txt)."""
import os
from functools import lru_cache

import pytest
import torch

import pack_cases as K
import pack_reference as R
from matrix_helpers import (GUARD, NAN_BITS, SEGK_DT, assert_equal, assert_identical, assert_within, make_recorder, nan_buffer, ptr,
                            stream, sync, take, write_parity)

pytestmark = pytest.mark.gpu

_PARITY, record = make_recorder()                   # "kernel form" -> [worst error / bound, case id]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    yield _lib
    out = os.environ.get("SEGK_PACK_PARITY_OUT")
    if out and _PARITY:
        write_parity(out, _PARITY,
                     "# worst error / bound per reduction form of tests/test_gpu_pack_matrix.py, random slabs (bounds derived in\n"
                     "# tests/pack_reference.py); the pass condition is ratio <= 1; the lattice runs and every pack are exact\n")


def same_bits(got, want, what):
    assert_identical(R.bits(got).reshape(-1), R.bits(want).reshape(-1), what)


@lru_cache(maxsize=None)
def weight(shape, seed):
    return R.special_values(shape, seed)


# ---- Conv2d and ConvTranspose2d weight packs -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CONV_CASES, ids=K.conv_case_id)
def test_pack_conv_weight_is_the_restatement(lib, case):
    c, what = case, f"segk_pack_conv_weight {K.conv_case_id(case)}"
    w = weight((c.Cout, c.CA + c.CB, c.taps), 11)
    wd, n = w.cuda(), K.conv_total(c)
    dst = nan_buffer(n, c.dtype)
    lib.call("segk_pack_conv_weight", ptr(wd), ptr(dst), c.Cout, c.CA, c.CB, c.Coutp, c.CAp, c.CBp, c.taps, c.mode, SEGK_DT[c.dtype],
             stream())
    sync(what)
    same_bits(take(dst, n, c.dtype, what), R.pack_conv(w, c.CA, c.CB, c.Coutp, c.CAp, c.CBp, c.taps, c.mode, c.dtype), what)


@pytest.mark.parametrize("case", K.BOTH_CASES, ids=K.both_case_id)
def test_pack_conv3x3_both_is_the_restatement(lib, case):
    c, what = case, f"segk_pack_conv3x3_both {K.both_case_id(case)}"
    w = weight((c.Cout, c.CA + c.CB, 9), 11)
    wd, n = w.cuda(), (c.CAp + c.CBp) * 9 * c.Coutp
    df = nan_buffer(n, c.dtype)
    dd = nan_buffer(n, c.dtype) if c.dgrad else None
    lib.call("segk_pack_conv3x3_both", ptr(wd), ptr(df), ptr(dd), c.Cout, c.CA, c.CB, c.Coutp, c.CAp, c.CBp, SEGK_DT[c.dtype], stream())
    sync(what)
    same_bits(take(df, n, c.dtype, what + " forward"), R.pack_conv(w, c.CA, c.CB, c.Coutp, c.CAp, c.CBp, 9, 0, c.dtype), what + " forward")
    if c.dgrad:
        same_bits(take(dd, n, c.dtype, what + " data gradient"), R.pack_conv(w, c.CA, c.CB, c.Coutp, c.CAp, c.CBp, 9, 1, c.dtype),
                  what + " data gradient")


@pytest.mark.parametrize("case", K.CONVT_CASES, ids=lambda c: f"{c.dtype}-{c.Cin}x{c.Cout}-m{c.mode}")
def test_pack_convt_weight_is_the_restatement(lib, case):
    c, what = case, f"segk_pack_convt_weight {case}"
    w = weight((c.Cin, c.Cout, 2, 2), 12)
    Cinp, Coutp = K.pad32(c.Cin), K.pad32(c.Cout)
    wd, n = w.cuda(), Cinp * 4 * Coutp
    dst = nan_buffer(n, c.dtype)
    lib.call("segk_pack_convt_weight", ptr(wd), ptr(dst), c.Cin, c.Cout, Cinp, Coutp, c.mode, SEGK_DT[c.dtype], stream())
    sync(what)
    same_bits(take(dst, n, c.dtype, what), R.pack_convt(w, Cinp, Coutp, c.mode, c.dtype), what)


# ---- the one-launch re-pack ------------------------------------------------------------------------------------------------
def entry_param(e, seed):
    return weight({0: (e.Cout, e.d0 + e.d1, 3, 3), 1: (e.d0, e.Cout, 2, 2), 2: (e.Cout,), 3: (e.Cout, e.d0, 1, 1)}[e.kind], seed)


def entry_expected(e, w, dtype, mode):
    Coutp = K.pad32(e.Cout)
    if e.kind == 0:
        return R.pack_conv(w, e.d0, e.d1, Coutp, K.pad32(e.d0), K.pad32(e.d1) if e.d1 else 0, 9, mode, dtype)
    if e.kind == 1:
        return R.pack_convt(w, K.pad32(e.d0), Coutp, mode, dtype)
    if e.kind == 2:
        return R.pack_bias(w, e.d0, Coutp)
    return R.pack_conv(w, e.d0, 0, Coutp, K.pad32(e.d0), 0, 1, mode, dtype)


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("name", list(K.MULTI_TABLES))
def test_pack_multi_is_the_restatement(lib, name, dtype):
    from image_segmentation_amd import ops
    table, what = K.MULTI_TABLES[name], f"segk_pack_multi {name} {dtype}"
    assert lib.query("segk_pack_convt_chunk") == K.CHUNK
    params = [entry_param(e, 20 + i) for i, e in enumerate(table)]
    dev = [p.cuda() for p in params]
    dts = ["fp32" if e.kind == 2 else dtype for e in table]
    fwd = [nan_buffer(K.entry_elements(e), dt) for e, dt in zip(table, dts)]
    dgr = [nan_buffer(K.entry_elements(e), dt) if e.dgrad else None for e, dt in zip(table, dts)]
    # the production builder; a registered ConvTranspose weight carries d0 = d1 = 0 (its shape says the rest)
    sig = tuple((ptr(d), ptr(f), ptr(g), e.kind, 0 if e.kind == 1 else e.d0, e.d1) for d, f, g, e in zip(dev, fwd, dgr, table))
    entries, blocks = ops._pack_table(sig, params)
    assert blocks == sum(K.entry_blocks(e) for e in table)
    tab = torch.frombuffer(entries, dtype=torch.int64).cuda()
    lib.call("segk_pack_multi", ptr(tab), len(table), blocks, SEGK_DT[dtype], stream())
    sync(what)
    for i, (e, w, f, g, dt) in enumerate(zip(table, params, fwd, dgr, dts)):
        n, w_i = K.entry_elements(e), f"{what} entry {i} {tuple(e)}"
        same_bits(take(f, n, dt, w_i + " forward"), entry_expected(e, w, dtype, 0), w_i + " forward")
        if e.dgrad:
            same_bits(take(g, n, dt, w_i + " data gradient"), entry_expected(e, w, dtype, 1), w_i + " data gradient")


def test_pack_multi_refuses_more_than_64_entries(lib):
    tab = torch.zeros((65 * 8,), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="pack_multi: bad arguments"):
        lib.call("segk_pack_multi", ptr(tab), 65, 65, 1, stream())
    sync("segk_pack_multi n = 65")


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_repack_stale_refreshes_seventy_weights_in_two_launches(lib, dtype, monkeypatch):
    """ops.repack_stale over a module of 70 small 3x3 weights registered exactly as DoubleConvFn registers its own: more than
    one table holds, so the second launch runs; every copy equals the restatement of the CHANGED parameter"""
    from image_segmentation_amd import ops
    tdt = R.TORCH_DT[dtype]

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cache = ops.PackCache()
            self.weights = torch.nn.ParameterList([torch.nn.Parameter(weight((Cout, CA + CB, 3, 3), 100 + i).clone())
                                                   for i, (Cout, CA, CB) in enumerate(K.REPACK_WEIGHTS)])

    def stale():
        raise AssertionError("a packed copy was rebuilt one by one")

    def copies(i, builder):
        w, (Cout, CA, CB) = m.weights[i], K.REPACK_WEIGHTS[i]
        f = m.cache.get_pair((f"w{i}f", tdt), (f"w{i}d", tdt), w, builder or (lambda: ops.pack_conv_both(w, CA, CB, tdt)),
                             meta=(ops.PACK_CONV3X3, CA, CB, tdt))
        return f, m.cache.get((f"w{i}d", tdt), w, stale)

    m = Holder().cuda()
    first = [copies(i, None) for i in range(70)]
    ops.repack_stale(m)                              # the first call only notes the epoch
    new = [weight((Cout, CA + CB, 3, 3), 500 + i) for i, (Cout, CA, CB) in enumerate(K.REPACK_WEIGHTS)]
    for w, v in zip(m.weights, new):
        w.data.copy_(v)
    ops.invalidate_packed_weights()
    calls, real = [], lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    ops.repack_stale(m)
    monkeypatch.undo()
    sync(f"repack_stale {dtype}")
    assert [name for name, _ in calls] == ["segk_pack_multi"] * 2
    assert [a[1] for _, a in calls] == [64, 6]
    for i, (Cout, CA, CB) in enumerate(K.REPACK_WEIGHTS):
        f, d = copies(i, stale)
        assert f.data_ptr() == first[i][0].data_ptr() and d.data_ptr() == first[i][1].data_ptr()      # the buffers are re-used
        geo = (CA, CB, K.pad32(Cout), K.pad32(CA), K.pad32(CB) if CB else 0, 9)
        same_bits(f.cpu(), R.pack_conv(new[i], *geo, 0, dtype), f"repack_stale {dtype} weight {i} forward")
        same_bits(d.cpu(), R.pack_conv(new[i], *geo, 1, dtype), f"repack_stale {dtype} weight {i} data gradient")


# ---- weight-gradient reductions --------------------------------------------------------------------------------------------
def make_slabs(r, S, values, seed):
    """[S][Np][taps][CAp + CBp] fp32 on the CPU; every padded column and every row n >= N holds the sentinel"""
    g = torch.Generator().manual_seed(seed)
    shape = (S, r.Np, r.taps, r.CAp + r.CBp)
    if values == "lattice":
        x = torch.randint(-K.LATTICE_MAX, K.LATTICE_MAX + 1, shape, generator=g, dtype=torch.int8).float()
    else:
        x = torch.randn(shape, generator=g, dtype=torch.float32)
    x[:, r.N:] = K.SENTINEL
    x[..., r.CA:r.CAp] = K.SENTINEL
    x[..., r.CAp + r.CB:] = K.SENTINEL
    return x


def upload(x):
    """a device copy with GUARD zero floats behind it"""
    d = torch.zeros((x.numel() + GUARD,), dtype=torch.float32, device="cuda")
    d[:x.numel()] = x.reshape(-1).cuda()
    return d


@lru_cache(maxsize=2)
def slab_stack(r, values):
    """the 512 slabs of a shape, shared by every S of the case table (the first S are used) -> (CPU, device)"""
    x = make_slabs(r, max(K.LATTICE_S), values, 31)
    return x, upload(x)


def weight_job(lib, r, S, src, dst):
    return lib.ReduceJob(ptr(src), ptr(dst), 0, S, r.N, r.CA, r.CB, r.Np, r.CAp, r.CBp, r.taps, 0)


def colsum_job(lib, c, src, dst):
    return lib.ReduceJob(ptr(src), ptr(dst), 1, c.rows, c.Ctot, c.col0, c.ncols, 0, 0, 0, 0, 0)


def run_single(lib, r, S, src, what):
    n = r.N * (r.CA + r.CB) * r.taps
    grad = nan_buffer(n, "fp32")
    lib.call("segk_wgrad_reduce", ptr(src), S, ptr(grad), r.N, r.CA, r.CB, r.Np, r.CAp, r.CBp, r.taps, stream())
    sync(what)
    return take(grad, n, "fp32", what).reshape(r.N, r.CA + r.CB, r.taps)


def run_multi(lib, jobs, what):
    """jobs: (ReduceShape, S, device slabs) or (ColsumCase, device partials) -> the results on the CPU"""
    sizes = [j[0].N * (j[0].CA + j[0].CB) * j[0].taps if len(j) == 3 else j[0].ncols for j in jobs]
    dst = [nan_buffer(n, "fp32") for n in sizes]
    arr = (lib.ReduceJob * len(jobs))(*[weight_job(lib, j[0], j[1], j[2], d) if len(j) == 3 else colsum_job(lib, j[0], j[1], d)
                                         for j, d in zip(jobs, dst)])
    lib.call("segk_wgrad_reduce_multi", arr, len(jobs), stream())
    sync(what)
    out = [take(d, n, "fp32", f"{what} job {i}") for i, (d, n) in enumerate(zip(dst, sizes))]
    return [o.reshape(j[0].N, j[0].CA + j[0].CB, j[0].taps) if len(j) == 3 else o for o, j in zip(out, jobs)]


def form(S):
    return "row" if S <= 16 else f"wide trips={K.wide_trips(S)}"


def check_lattice(lib, r, S, cpu, dev, what):
    want = R.reduce_exact(cpu[:S], r.N, r.CA, r.CB, r.CAp, r.CBp, r.taps)
    assert float(want.abs().max()) < 2 ** 24
    assert_equal(run_single(lib, r, S, dev, what), want, what)
    assert_equal(run_multi(lib, [(r, S, dev)], what + " (multi entry)")[0], want, what + " (multi entry)")


def check_random(lib, r, S, cpu, dev, what):
    ref = R.reduce_exact(cpu[:S], r.N, r.CA, r.CB, r.CAp, r.CBp, r.taps)
    bound = R.reduce_bound(cpu[:S], r.N, r.CA, r.CB, r.CAp, r.CBp, r.taps)
    got = run_single(lib, r, S, dev, what)
    record(f"wgrad_reduce {form(S)}", assert_within(got, ref, bound, what), what)
    same_bits(run_single(lib, r, S, dev, what + " second run"), got, what + " second run")
    same_bits(run_multi(lib, [(r, S, dev)], what + " (multi entry)")[0], got, what + " (multi entry)")


@pytest.mark.parametrize("S", K.LATTICE_S)
@pytest.mark.parametrize("shape", K.REDUCE_SHAPES, ids=K.reduce_shape_id)
def test_wgrad_reduce_lattice_is_exact(lib, shape, S):
    cpu, dev = slab_stack(shape, "lattice")
    check_lattice(lib, shape, S, cpu, dev, f"segk_wgrad_reduce lattice {K.reduce_shape_id(shape)} S={S}")


@pytest.mark.parametrize("S", K.RANDOM_S)
@pytest.mark.parametrize("shape", K.REDUCE_SHAPES, ids=K.reduce_shape_id)
def test_wgrad_reduce_random_within_the_bound(lib, shape, S):
    cpu, dev = slab_stack(shape, "random")
    check_random(lib, shape, S, cpu, dev, f"segk_wgrad_reduce random {K.reduce_shape_id(shape)} S={S}")


def test_wgrad_reduce_row_above_48k_of_lds(lib):
    """a gradient row of 49536 bytes: above the 48 KiB a kernel may take without asking, below the 64 KiB both entries accept"""
    r, S = K.BIG_ROW, K.BIG_ROW_S
    for values, check in (("lattice", check_lattice), ("random", check_random)):
        cpu = make_slabs(r, S, values, 32)
        check(lib, r, S, cpu, upload(cpu), f"segk_wgrad_reduce {values} {K.reduce_shape_id(r)} S={S}")


def test_wgrad_reduce_refuses_a_row_that_is_no_multiple_of_32(lib):
    """CAp + CBp = 48: taps * 48 / 4 vectors would cover the row only for some tap counts, and the multi entry refuses it"""
    src = upload(torch.zeros((2, 32, 9, 48)))
    n = 20 * 40 * 9
    grad = nan_buffer(n, "fp32")
    with pytest.raises(RuntimeError, match="wgrad_reduce: bad arguments"):
        lib.call("segk_wgrad_reduce", ptr(src), 2, ptr(grad), 20, 40, 0, 32, 48, 0, 9, stream())
    with pytest.raises(RuntimeError, match="wgrad_reduce: bad arguments"):
        lib.call("segk_wgrad_reduce", ptr(src), 2, ptr(grad), 20, 30, 10, 32, 32, 16, 9, stream())
    arr = (lib.ReduceJob * 1)(lib.ReduceJob(ptr(src), ptr(grad), 0, 2, 20, 40, 0, 32, 48, 0, 9, 0))
    with pytest.raises(RuntimeError, match="wgrad_reduce_multi: job 0: bad arguments"):
        lib.call("segk_wgrad_reduce_multi", arr, 1, stream())
    sync("segk_wgrad_reduce refusal")
    assert bool((grad.cpu() == NAN_BITS["fp32"]).all()), "a refused call wrote"


def make_partials(c, values, seed):
    """[rows][Ctot][2] fp32: the second float of every pair is NaN (it must never be read)"""
    g = torch.Generator().manual_seed(seed)
    if values == "lattice":
        x = torch.randint(-K.LATTICE_MAX, K.LATTICE_MAX + 1, (c.rows, c.Ctot, 2), generator=g).float()
    else:
        x = torch.randn((c.rows, c.Ctot, 2), generator=g, dtype=torch.float32)
    x[..., 1] = float("nan")
    return x


def colsum_form(c):
    return f"colsum trips={K.cdiv(c.rows, 256)}"


@pytest.mark.parametrize("case", K.COLSUM_CASES, ids=lambda c: f"rows{c.rows}-cols{c.ncols}-at{c.col0}")
def test_column_sums(lib, case):
    c = case
    for values in ("lattice", "random"):
        what = f"segk_wgrad_reduce_multi column sums {values} {tuple(c)}"
        part = make_partials(c, values, 41)
        got = run_multi(lib, [(c, upload(part))], what)[0]
        if values == "lattice":
            assert_equal(got, R.colsum_exact(part, c.col0, c.ncols), what)
        else:
            record(colsum_form(c), assert_within(got, R.colsum_exact(part, c.col0, c.ncols), R.colsum_bound(part, c.col0, c.ncols), what), what)


@pytest.mark.parametrize("order", K.JOB_ORDERS)
def test_wgrad_reduce_multi_job_orders(lib, order):
    """every kind of job first, in the middle and last of a launch of 1 .. 4 jobs: each result is the single launch's, bit
    for bit, and within its bound of the float64 sum; a second launch repeats the bits"""
    what = f"segk_wgrad_reduce_multi jobs {order}"
    jobs, cpu = [], []
    for slot, kind in enumerate(order):
        spec = K.job_spec(kind, slot)
        if kind == "C":
            x = make_partials(spec, "random", 50 + slot)
            jobs.append((spec, upload(x)))
        else:
            r, S = K.REDUCE_SHAPES[spec[0]], spec[1]
            x = make_slabs(r, S, "random", 50 + slot)
            jobs.append((r, S, upload(x)))
        cpu.append(x)
    got = run_multi(lib, jobs, what)
    again = run_multi(lib, jobs, what + " second run")
    for i, (j, x, g, g2) in enumerate(zip(jobs, cpu, got, again)):
        w_i = f"{what} job {i}"
        same_bits(g2, g, w_i + " second run")
        if len(j) == 3:
            r, S, dev = j
            same_bits(g, run_single(lib, r, S, dev, w_i + " single launch"), w_i + " against the single launch")
            args = (r.N, r.CA, r.CB, r.CAp, r.CBp, r.taps)
            record(f"wgrad_reduce_multi {form(S)}", assert_within(g, R.reduce_exact(x, *args), R.reduce_bound(x, *args), w_i), w_i)
        else:
            c = j[0]
            record("wgrad_reduce_multi " + colsum_form(c), assert_within(g, R.colsum_exact(x, c.col0, c.ncols), R.colsum_bound(x, c.col0, c.ncols), w_i), w_i)


# ---- layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.LAYOUT_CASES, ids=K.layout_case_id)
def test_layout_passes_are_the_restatement(lib, case):
    c, cid, sdt = case, K.layout_case_id(case), SEGK_DT[case.dtype]
    x = weight((c.B, c.C, c.H, c.W), 61)
    n = c.B * c.H * c.W * c.Cp
    xd, dst = x.cuda(), nan_buffer(n, c.dtype)
    lib.call("segk_nchw_to_nhwc", ptr(xd), ptr(dst), c.B, c.C, c.H, c.W, c.Cp, sdt, stream())
    sync(f"segk_nchw_to_nhwc {cid}")
    got = take(dst, n, c.dtype, f"segk_nchw_to_nhwc {cid}").reshape(c.B, c.H, c.W, c.Cp)
    want = R.to_nhwc(x, c.Cp, c.dtype)
    same_bits(got, want, f"segk_nchw_to_nhwc {cid}")
    assert bool((R.bits(got[..., c.C:]) == 0).all()), f"segk_nchw_to_nhwc {cid}: a padding channel is not +0"
    src = want.clone()
    src[..., c.C:] = float("nan")                    # the padding of the source must not reach the output
    sd, m = src.cuda(), c.B * c.C * c.H * c.W
    out = nan_buffer(m, "fp32")
    lib.call("segk_nhwc_to_nchw", ptr(sd), ptr(out), c.B, c.C, c.H, c.W, c.Cp, sdt, stream())
    sync(f"segk_nhwc_to_nchw {cid}")
    same_bits(take(out, m, "fp32", f"segk_nhwc_to_nchw {cid}"), R.to_nchw(want, c.C), f"segk_nhwc_to_nchw {cid}")
