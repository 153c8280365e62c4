"""What the GPU matrices (test_gpu_stem_pool_matrix.py, test_gpu_vit_matrix.py, test_gpu_resize_matrix.py) share: NaN-patterned
output buffers with a guard behind them (byte- and int64-patterned ones for integer outputs), the element-wise comparisons, the
sticky-error exit and the worst error / bound record."""
import pytest
import torch

TORCH_DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "u8": torch.uint8, "i64": torch.int64}
SEGK_DT = {"fp32": 0, "bf16": 1}
# quiet-NaN patterns: what a kernel must overwrite, and leave in the guard; integer outputs ("u8", "i64") take a pattern no
# valid result of their tests holds
NAN_BITS = {"bf16": 0x7FDE, "fp32": 0x7FDEAD00, "u8": 0xA5, "i64": 0x7FDEAD007FDEAD00}
BITS_DT = {"bf16": torch.int16, "fp32": torch.int32, "u8": torch.uint8, "i64": torch.int64}
GUARD = 4096                                         # elements behind every output buffer


def make_recorder():
    """-> (parity, record): parity maps "kernel quantity regime" -> [worst error / bound, case id]"""
    parity = {}

    def record(name, ratio, cid):
        ratio = float(ratio)
        if name not in parity or ratio > parity[name][0]:
            parity[name] = [ratio, cid]
    return parity, record


def write_parity(path, parity, header, width=58):
    with open(path, "w") as f:
        f.write(header)
        for name in sorted(parity):
            f.write(f"{name:{width}s} {parity[name][0]:.4f}   {parity[name][1]}\n")


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a GPU fault is sticky: nothing more is started on the device in this session
        pytest.exit(f"{what}: the device reported {e}", returncode=3)


def nan_buffer(n, dtype):
    return torch.full((n + GUARD,), NAN_BITS[dtype], dtype=BITS_DT[dtype], device="cuda")


def take(buf, n, dtype, what, written=None, mask=None):
    """the first n elements on the CPU in the dtype; all of them (or the first `written`, or those of the bool `mask`)
    overwritten, the guard -- and with a mask everything outside it -- untouched"""
    bits = buf.cpu()
    assert bool((bits[n:] == NAN_BITS[dtype]).all()), f"{what}: wrote behind the buffer"
    if mask is not None:
        mask = mask.reshape(-1)
        left = ((bits[:n] == NAN_BITS[dtype]) & mask).nonzero()
        assert len(left) == 0, f"{what}: {len(left)} of {int(mask.sum())} elements were not written, first at {int(left[0])}"
        hit = ((bits[:n] != NAN_BITS[dtype]) & ~mask).nonzero()
        assert len(hit) == 0, f"{what}: {len(hit)} elements outside the written region were touched, first at {int(hit[0])}"
        return bits[:n].view(TORCH_DT[dtype])
    w = n if written is None else written
    left = (bits[:w] == NAN_BITS[dtype]).nonzero()
    assert len(left) == 0, f"{what}: {len(left)} of {w} elements were not written, first at {int(left[0])}"
    return bits[:n].view(TORCH_DT[dtype])


def ptr(t):
    return 0 if t is None else t.data_ptr()


def assert_equal(got, want, what):
    got, want = got.float(), want.float()
    if torch.equal(got, want):
        return
    idx = ((got != want) | torch.isnan(got)).nonzero()
    lines = [f"  [{', '.join(map(str, i))}] = {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}" for i in idx[:10].tolist()]
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ\n" + "\n".join(lines))


def assert_identical(got, want, what):
    """integer tensors: every element the same integer (no pass through a float)"""
    assert got.dtype == want.dtype and not got.dtype.is_floating_point and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)}"
    if torch.equal(got, want):
        return
    idx = (got != want).nonzero()
    lines = [f"  [{', '.join(map(str, i))}] = {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}" for i in idx[:10].tolist()]
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ\n" + "\n".join(lines))


def assert_within(got, ref, bound, what):
    """-> worst |got - ref| / bound (0 / 0 counts as 0); fails above 1 or on a non-finite value"""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err).clamp(min=1e-300))
    worst = float(ratio.max())
    print(f"{what}: error / bound = {worst:.4f}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the bound at {tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])}"
    return worst
