"""GPU (-m gpu): the class-count entries of csrc/augment.hip -- segk_label_hist and segk_rgb_label_to_classes -- through the C
ABI against tests/augment_reference.py (label_hist: drop the ignore value first, then clamp to 0..C-1, then count -- utils.py:168-173
as augment.hip cites it; rgb_classes), on its case table: one workgroup, exactly 1024 workgroups, and label counts beyond
1024 * 4096 where the loop takes a fifth pass; a last vector of one, two and three labels; uint8 and int64 labels, the latter with
-5, C, 2^40, -2^63 and the ignore value -100 (tests/test_recon_prompt_cases_host.py checks the restatements, the launch
arithmetic and that clamping before the ignore test gives other counts on these inputs).

Everything is integer: the comparisons are equalities.  counts[256] starts with a non-zero base below C and a sentinel at and
above C; after two calls the entries below C hold base plus twice the restatement and the sentinels are unchanged."""
import numpy as np
import pytest
import torch

import augment_reference as AR
from matrix_helpers import assert_identical, ptr, stream, sync

pytestmark = pytest.mark.gpu
SENTINEL = 0x5EA5EA5EA5EA5EA5                          # counts at and above C; also fits int64, which carries the uint64 buffer
BASE = 1000003                                         # counts[c] starts at BASE + c below C


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_segmentation_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def masters(lib):
    """uint8 and int64 master arrays on both sides: every case counts a prefix"""
    out = {}
    for eb in (1, 8):
        m = AR.hist_labels(eb, AR.HIST_N[-1])
        out[eb] = (m, torch.from_numpy(m).cuda())
    return out


@pytest.mark.parametrize("case", AR.hist_cases(), ids=lambda c: f"{'u8' if c[0] == 1 else 'i64'}-n{c[1]}-C{c[2]}-ign{c[3]}")
def test_label_hist_accumulates_the_restatement(lib, masters, case):
    eb, n, C, ign = case
    what = f"segk_label_hist {'uint8' if eb == 1 else 'int64'} n={n} C={C} ignore={ign}"
    m, md = masters[eb]
    lab = AR.hist_case_labels(m, n, C)
    ld = md[:n] if eb == 1 else torch.where(md[:n] == 300, torch.full_like(md[:n], C), md[:n])
    start = np.full(256, SENTINEL, np.int64)
    start[:C] = BASE + np.arange(C)
    counts = torch.from_numpy(start).cuda()
    for _ in range(2):
        lib.call("segk_label_hist", ptr(ld), n, eb, C, 0 if ign is None else 1, 0 if ign is None else ign, ptr(counts), stream())
    sync(what)
    want = start.copy()
    want[:C] += 2 * AR.label_hist(lab, C, ign)
    assert_identical(counts.cpu(), torch.from_numpy(want), what)


@pytest.mark.parametrize("n", AR.RGB_N)
def test_rgb_label_to_classes_is_the_restatement(lib, n):
    what = f"segk_rgb_label_to_classes n={n}"
    px = AR.rgb_pixels(n)
    out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    pd = torch.from_numpy(px).cuda()
    lib.call("segk_rgb_label_to_classes", ptr(pd), ptr(out), n, stream())
    sync(what)
    got = out.cpu()
    assert bool((got[n:] == 0xA5).all()), f"{what}: wrote behind the buffer"
    assert_identical(got[:n], torch.from_numpy(AR.rgb_classes(px)), what)
