"""GPU (-m gpu): the convolution and 1x1-geometry kernels -- conv_igemm_kernel (csrc/conv_igemm.hip), conv3x3_pipe_kernel
(csrc/conv_pipe.hip), conv_ws_kernel (csrc/conv_ws.hip), conv_rs_kernel (csrc/conv_rs.hip), gemm_dma_kernel (csrc/gemm.hip) and
convt_stream_kernel (csrc/convt_stream.hip) -- driven directly through _lib.call on the dense inputs of the two case tables
the project already has (tests/conv_cases.py and tests/gemm_cases.py: no new shape), every output buffer pre-filled with NaN
and followed by a guard of NaN (so a store past the written range, or a missing one, changes a digest) and compared by SHA-1
with tests/golden/conv_bits.json.  The digests are folded: per kernel instance, and per buffer name, one SHA-1 over
"case:digest;" of that buffer in every case of the instance, in table order.

The fixture is a record of the library BEFORE the convolution kernels were split into one unit each and folded onto one unit
walk, patch piece map, pixel test, prologue transform and tile epilogue (csrc/conv_tile.hpp): the code may be
rearranged, the bytes may not change.  It was recorded on an MI355X: the statistics rows of conv_rs_kernel (one per wave slab and
workgroup) and the row tiles of gemm_dma_kernel depend on the 256 compute units.

  3x3   every case of conv_cases.CASES + LONG_CASES, the dense run of conv_reference.make_problem (operands uniform in [-1, 1],
        with the prologue z in [-2, 2]): out, out2, the statistics buffer (all segk_bn_stats_floats(tiles, N) floats: the rows
        the kernel owes and the NaN nobody may touch) and act_out, where the case has them
  1x1   every case of gemm_cases.CASES + LONG_CASES, the dense run of gemm_reference.make_problem: plain (segk_linear,
        segk_linear_splitk, segk_conv1x1), pixel-shuffle (segk_convt2x2_fwd) and un-shuffle (segk_convt2x2_dgrad), with the bias
        and the quick_gelu where the table has them

Set SEGK_CONV_BITS_OUT=<file> to write the record there instead of comparing (never from the code under test: point SEGK_LIB at
a library built from the parent commit)."""
import hashlib
import json
import os

import pytest
import torch

import conv_cases
import conv_reference
import gemm_cases
import gemm_reference

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_bits.json")
OUT = os.environ.get("SEGK_CONV_BITS_OUT")
NAN = float("nan")
SEGK_DT = {"fp32": 0, "bf16": 1}
GUARD_ROWS = 64                # pixels / rows of NaN behind every output
GUARD_FLOATS = 4096            # floats of NaN behind the statistics buffer
_RECORD = {}
_FOLD = {}                     # group -> buffer name -> running SHA-1


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


def _stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.cuda().contiguous()


def nans(rows, C, dtype):
    return torch.full((int(rows), int(C)), NAN, dtype=dtype, device="cuda")


def check(group, case, **bufs):
    """fold the SHA-1 of every buffer of a case (guard included) into its group"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a GPU fault is sticky: nothing more is started on the device in this session
        pytest.exit(f"{group} {case}: the device reported {e}", returncode=3)
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


# ---- the 3x3 kernels -------------------------------------------------------------------------------------------------------------
def run_conv(lib, c):
    dt, sdt = conv_reference.TORCH_DT[c.dtype], SEGK_DT[c.dtype]
    prob = conv_reference.make_problem(c, "dense")
    P, N = c.B * c.H * c.W, c.CO1 + c.CO2
    xa, xb, w, bias, scale, shift = (dev(t) for t in (prob.xa, prob.xb, prob.w, prob.bias, prob.scale, prob.shift))
    wp = torch.full(((c.CA + c.CB) * 9 * N,), NAN, dtype=dt, device="cuda")
    lib.call("segk_pack_conv_weight", ptr(w), ptr(wp), *prob.pack_args, 9, c.mode, sdt, _stream())
    out = nans(P + GUARD_ROWS, c.CO1, dt)
    out2 = nans(P + GUARD_ROWS, c.CO2, dt) if c.CO2 else None
    act = nans(P + GUARD_ROWS, c.CA, dt) if c.act_out else None
    stats = None
    if c.stats:
        tiles = lib.query("segk_conv_tiles", c.B, c.H, c.W, c.CA + c.CB, N, sdt)
        stats = nans(1, lib.query("segk_bn_stats_floats", tiles, N) + GUARD_FLOATS, torch.float32)
    if c.act_out:
        lib.call("segk_conv3x3_act", ptr(xa), ptr(wp), ptr(scale), ptr(shift), ptr(out), ptr(act), ptr(stats), c.B, c.H, c.W, c.CA,
                 c.CO1, sdt, _stream())
    else:
        lib.call("segk_conv3x3", ptr(xa), ptr(xb), ptr(wp), ptr(bias), ptr(scale), ptr(shift), ptr(out), ptr(out2), ptr(stats), c.B,
                 c.H, c.W, c.CA, c.CB, c.CO1, c.CO2, sdt, _stream())
    check("conv3x3/" + conv_cases.instance_of(c), conv_cases.case_id(c), out=out, out2=out2, stats=stats, act_out=act)


_CONV = conv_cases.CASES + conv_cases.LONG_CASES


@pytest.mark.parametrize("instance", sorted({conv_cases.instance_of(c) for c in _CONV}))
def test_conv3x3(lib, want, instance):
    for c in _CONV:
        if conv_cases.instance_of(c) == instance:
            run_conv(lib, c)
    settle(want, f"conv3x3/{instance}")


# ---- the 1x1 geometry: plain, pixel-shuffle and un-shuffle -----------------------------------------------------------------------
def run_gemm(lib, c):
    dt, sdt = gemm_reference.TORCH_DT[c.dtype], SEGK_DT[c.dtype]
    prob = gemm_reference.make_problem(c, "dense")
    M, K, N, mode = gemm_cases.gemm_view(c)
    x, w, bias = dev(prob.x), dev(prob.w), dev(prob.bias)
    wp = torch.full((K * N,), NAN, dtype=dt, device="cuda")
    if mode == 0:
        lib.call("segk_pack_conv_weight", ptr(w), ptr(wp), c.Lout, c.Lin, 0, c.Cout, c.Cin, 0, 1, 0, sdt, _stream())
    else:
        lib.call("segk_pack_convt_weight", ptr(w), ptr(wp), c.Lin, c.Lout, c.Cin, c.Cout, mode - 1, sdt, _stream())
    Cp = gemm_reference.out_channels(c)[0]
    rows = {"linear": M, "linear_splitk": c.S * M, "convt_fwd": 4 * M}.get(c.entry, M)
    out = nans(rows + GUARD_ROWS, Cp, dt)
    if c.entry == "linear":
        lib.call("segk_linear", ptr(x), ptr(wp), ptr(bias), ptr(out), M, c.Cin, c.Cout, c.act, sdt, _stream())
    elif c.entry == "linear_splitk":
        lib.call("segk_linear_splitk", ptr(x), ptr(wp), ptr(bias), ptr(out), M, c.Cin, c.Cout, c.S, sdt, _stream())
    elif c.entry == "conv1x1":
        lib.call("segk_conv1x1", ptr(x), ptr(wp), ptr(bias), ptr(out), c.B, c.H, c.W, c.Cin, c.Cout, sdt, _stream())
    elif c.entry == "convt_fwd":
        lib.call("segk_convt2x2_fwd", ptr(x), ptr(wp), ptr(bias), ptr(out), c.B, c.H, c.W, c.Cin, c.Cout, sdt, _stream())
    else:
        lib.call("segk_convt2x2_dgrad", ptr(x), ptr(wp), ptr(out), c.B, c.H, c.W, c.Cin, c.Cout, sdt, _stream())
    check(gemm_group(c), gemm_cases.case_id(c), out=out)


_GEMM = gemm_cases.CASES + gemm_cases.LONG_CASES


def gemm_group(c):
    return f"{c.entry}/" + gemm_cases.instance_of(c)


@pytest.mark.parametrize("group", sorted({gemm_group(c) for c in _GEMM}))
def test_gemm(lib, want, group):
    for c in _GEMM:
        if gemm_group(c) == group:
            run_gemm(lib, c)
    settle(want, group)
