"""MI355X: superpixels on the device (image_segmentation_amd/superpixels.py, csrc/slic.hip) against the
NumPy restatement (tests/slic_reference.py) on the shared case table (tests/slic_cases.py), bit for bit: labels, centres,
counts, hist, winner and the snapped mask of every case, run twice and on a side stream, the inputs left as they were; the
entries into prefilled buffers whose slack must stay; views and unaligned inputs; the C entries' refusals through the binding;
Segmenter(snap=...) against the composition by hand on the plain, merged and tiled routes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_cases as SC                                                            # noqa: E402
import slic_reference as R                                                         # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 64


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as seg
    return seg


def on_side_stream(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return out


def check_superpixels(sp, case, what=""):
    lab, cen, n = SC.expected(case)
    H, W = lab.shape
    ny, nx = R.grid_of(H, W, case.step)
    assert (sp.grid, sp.step, sp.k) == ((ny, nx), case.step, ny * nx)
    assert sp.labels.dtype == sp.centres.dtype == sp.counts.dtype == torch.int32
    assert np.array_equal(sp.counts.cpu().numpy(), n), what
    assert np.array_equal(sp.centres.cpu().numpy(), cen), what
    assert np.array_equal(sp.labels.cpu().numpy(), lab), what


# ------------------------------------------------------------------------------------------------ SLIC
@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_superpixels_equal_the_restatement(seg, case):
    x = torch.from_numpy(case.image.copy()).cuda()
    kw = dict(step=case.step, compactness=case.compactness, iterations=case.iterations, space=case.space)
    first = seg.superpixels(x, **kw)
    check_superpixels(first, case, "first")
    again = seg.superpixels(x, **kw)
    third = on_side_stream(lambda: seg.superpixels(x, **kw))
    for other in (again, third):
        assert torch.equal(other.labels, first.labels) and torch.equal(other.centres, first.centres) and torch.equal(other.counts, first.counts)
    assert np.array_equal(x.cpu().numpy(), case.image)      # the input is left as it was
    if case.image.shape[2] == 1:                            # a grey image may come as [H,W]
        check_superpixels(seg.superpixels(x[..., 0].contiguous(), **kw), case, "[H,W]")


def test_superpixels_of_views_and_unaligned_images(seg):
    """an image at every byte offset mod 4 (the wide path falls back to bytes row by row), a strided view, and an RGBA image
    whose alpha must not matter"""
    case = SC.BY_NAME["33x65-noise"]
    H, W, C = case.image.shape
    kw = dict(step=case.step, compactness=case.compactness, iterations=case.iterations, space=case.space)
    src = torch.from_numpy(case.image.copy()).cuda()
    for off in (1, 2, 3):
        flat = torch.zeros((H * W * C + 8,), dtype=torch.uint8, device="cuda")
        flat[off:off + H * W * C] = src.reshape(-1)
        view = flat[off:off + H * W * C].view(H, W, C)
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        check_superpixels(seg.superpixels(view, **kw), case, f"offset {off}")
    rgba = torch.full((H, W, 4), 77, dtype=torch.uint8, device="cuda")
    rgba[..., :3] = src
    check_superpixels(seg.superpixels(rgba, **kw), case, "rgba")
    check_superpixels(seg.superpixels(rgba[..., :3], **kw), case, "strided")       # not contiguous: copied by the host layer
    grey = SC.BY_NAME["65x129-grey-step5"]
    g = torch.zeros((65 * 129 + 4,), dtype=torch.uint8, device="cuda")
    g[1:1 + 65 * 129] = torch.from_numpy(grey.image.copy()).cuda().reshape(-1)
    check_superpixels(seg.superpixels(g[1:1 + 65 * 129].view(65, 129, 1), step=grey.step, compactness=grey.compactness,
                                      iterations=grey.iterations, space=grey.space), grey, "grey offset 1")


ROWS = (4, 16, 64)                                          # every tile height the entries take; the public layer picks by size


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", ["33x65-noise", "65x129-noise", "65x129-grey-step5", "65x129-step64", "65x129-constant", "emptied"])
def test_every_tile_height_gives_the_same_superpixels(seg, name, rows):
    """the public layer takes 4-row tiles for images this small: the taller tiles are driven through the entries"""
    from image_segmentation_amd import _lib, ops
    case = SC.BY_NAME[name]
    H, W, C = case.image.shape
    S, m, T, space = case.step, case.compactness, case.iterations, _lib.SLIC_SPACES[case.space]
    K = SC.grid_k(case)
    x = torch.from_numpy(case.image.copy()).cuda()
    i32 = dict(dtype=torch.int32, device="cuda")
    lab, cen, cnt, sums = torch.empty((H, W), **i32), torch.empty((K, 5), **i32), torch.empty((K,), **i32), torch.empty((K, 8), **i32)
    s = ops._stream()
    _lib.call("segk_slic_start", x.data_ptr(), cen.data_ptr(), sums.data_ptr(), C, space, S, H, W, K, s)
    for t in range(T):
        _lib.call("segk_slic_assign", x.data_ptr(), cen.data_ptr(), sums.data_ptr(), lab.data_ptr(), C, space, S, m, t, T, rows, H, W, K, s)
        _lib.call("segk_slic_update", cen.data_ptr(), sums.data_ptr(), cnt.data_ptr(), S, H, W, K, s)
    want = SC.expected(case)
    for got, ref in zip((lab, cen, cnt), want):
        assert np.array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("rows", ROWS)
def test_slic_entries_write_what_they_own_and_nothing_else(seg, rows):
    """the three entries driven by hand into prefilled buffers: labels appear in the last round only, the sums are zero between
    rounds, the slack around every buffer stays"""
    from image_segmentation_amd import _lib, ops
    case = SC.BY_NAME["65x129-rgba"]
    H, W, C = case.image.shape
    S, m, T, space = case.step, case.compactness, case.iterations, _lib.SLIC_SPACES[case.space]
    K = SC.grid_k(case)
    x = torch.from_numpy(case.image.copy()).cuda()
    FILL = 0x5A5A5A5A

    def framed(n):
        buf = torch.full((SLACK + n + SLACK,), FILL, dtype=torch.int32, device="cuda")
        return buf, buf[SLACK:SLACK + n]
    (bl, lab), (bc, cen), (bn, cnt), (bs, sums) = framed(H * W), framed(K * 5), framed(K), framed(K * 8)
    s = ops._stream()
    _lib.call("segk_slic_start", x.data_ptr(), cen.data_ptr(), sums.data_ptr(), C, space, S, H, W, K, s)
    f = R.features(case.image, case.space)
    want = R.start_centres(f, S)
    assert np.array_equal(cen.cpu().numpy().reshape(K, 5), want) and (sums == 0).all()
    for t in range(T):
        _lib.call("segk_slic_assign", x.data_ptr(), cen.data_ptr(), sums.data_ptr(), lab.data_ptr(), C, space, S, m, t, T, rows, H, W, K, s)
        assert bool((lab == FILL).all()) == (t < T - 1)
        n_dev = sums.view(K, 8)[:, 0].clone()
        _lib.call("segk_slic_update", cen.data_ptr(), sums.data_ptr(), cnt.data_ptr(), S, H, W, K, s)
        ref_lab = R.assign(f, want, S, m)
        want, n = R.update(f, ref_lab, want)
        assert np.array_equal(n_dev.cpu().numpy(), n) and np.array_equal(cnt.cpu().numpy(), n)
        assert np.array_equal(cen.cpu().numpy().reshape(K, 5), want) and (sums == 0).all()
    assert np.array_equal(lab.cpu().numpy().reshape(H, W), SC.expected(case)[0])
    for buf in (bl, bc, bn, bs):
        assert (buf[:SLACK] == FILL).all() and (buf[-SLACK:] == FILL).all()


# ------------------------------------------------------------------------------------------------ vote and snap
@pytest.mark.parametrize("case", SC.SNAP_CASES, ids=[c.name for c in SC.SNAP_CASES])
def test_snap_equals_the_restatement(seg, case):
    want, hist, win = SC.snap_expected(case)
    lab = torch.from_numpy(case.labels.copy()).cuda()
    mask = torch.from_numpy(case.mask.copy()).cuda()
    w = None if case.weights is None else torch.from_numpy(case.weights.copy()).cuda()
    kw = dict(classes=case.classes, fill=case.fill, min_share=case.min_share / 256.0, weights=w, k=case.k)
    first = seg.snap_mask(mask, lab, **kw)
    assert first.mask.dtype == torch.uint8 and first.hist.dtype == torch.int64 and first.winner.dtype == torch.int32
    assert np.array_equal(first.hist.cpu().numpy(), hist)
    assert np.array_equal(first.winner.cpu().numpy(), win)
    assert np.array_equal(first.mask.cpu().numpy(), want)
    again = seg.snap_mask(mask, lab, **kw)
    third = on_side_stream(lambda: seg.snap_mask(mask, lab, **kw))
    for other in (again, third):
        assert torch.equal(other.mask, first.mask) and torch.equal(other.hist, first.hist) and torch.equal(other.winner, first.winner)
    assert np.array_equal(lab.cpu().numpy(), case.labels) and np.array_equal(mask.cpu().numpy(), case.mask)
    assert w is None or np.array_equal(w.cpu().numpy(), case.weights)


def test_snap_takes_a_superpixels_record_views_and_unaligned_maps(seg):
    case = SC.SNAP_BY_NAME["slic-void-band"]
    want, hist, win = SC.snap_expected(case)
    H, W = case.mask.shape
    slic_case = SC.BY_NAME["65x129-noise"]
    sp = seg.superpixels(torch.from_numpy(slic_case.image.copy()).cuda(), slic_case.step, slic_case.compactness, slic_case.iterations,
                         slic_case.space)
    mask = torch.from_numpy(case.mask.copy()).cuda()
    w = torch.from_numpy(case.weights.copy()).cuda()
    kw = dict(classes=case.classes, fill=case.fill, min_share=case.min_share / 256.0)
    got = seg.snap_mask(mask, sp, weights=w, **kw)
    assert np.array_equal(got.mask.cpu().numpy(), want) and np.array_equal(got.hist.cpu().numpy(), hist)
    # byte maps at an odd address and a label map off the 16-byte grid: the paint kernel's narrow path
    flat = torch.zeros((H * W + 8,), dtype=torch.uint8, device="cuda")
    flat[1:1 + H * W] = mask.reshape(-1)
    odd = flat[1:1 + H * W].view(H, W)
    lflat = torch.zeros((H * W + 4,), dtype=torch.int32, device="cuda")
    lflat[1:1 + H * W] = sp.labels.reshape(-1)
    lodd = lflat[1:1 + H * W].view(H, W)
    assert odd.data_ptr() % 2 == 1 and lodd.data_ptr() % 16 == 4
    for m_, l_ in ((odd, sp.labels), (mask, lodd), (odd, lodd)):
        got = seg.snap_mask(m_, l_, weights=w, k=sp.k, **kw)
        assert np.array_equal(got.mask.cpu().numpy(), want) and np.array_equal(got.winner.cpu().numpy(), win)
    tr = torch.from_numpy(np.ascontiguousarray(case.mask.T)).cuda().t()            # not contiguous: copied by the host layer
    assert not tr.is_contiguous()
    assert np.array_equal(seg.snap_mask(tr, sp, weights=w, **kw).mask.cpu().numpy(), want)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", ["slic-weighted", "blocks", "pixel-segments"])
def test_every_tile_height_gives_the_same_votes(seg, name, rows):
    from image_segmentation_amd import _lib, ops
    case = SC.SNAP_BY_NAME[name]
    H, W = case.mask.shape
    lab, mask = torch.from_numpy(case.labels.copy()).cuda(), torch.from_numpy(case.mask.copy()).cuda()
    w = None if case.weights is None else torch.from_numpy(case.weights.copy()).cuda()
    hist = torch.zeros((case.k, 8), dtype=torch.int64, device="cuda")
    bits = sum(1 << c for c in case.classes)
    _lib.call("segk_snap_vote", lab.data_ptr(), mask.data_ptr(), ops._p(w), hist.data_ptr(), bits, rows, H, W, case.k, ops._stream())
    assert np.array_equal(hist.cpu().numpy(), SC.snap_expected(case)[1])


@pytest.mark.parametrize("rows", ROWS)
def test_snap_entries_write_what_they_own_and_nothing_else(seg, rows):
    from image_segmentation_amd import _lib, ops
    case = SC.SNAP_BY_NAME["labels-outside"]
    want, hist, win = SC.snap_expected(case)
    H, W = case.mask.shape
    K = case.k
    lab = torch.from_numpy(case.labels.copy()).cuda()
    mask = torch.from_numpy(case.mask.copy()).cuda()
    w = torch.from_numpy(case.weights.copy()).cuda()

    def framed(n, dtype, fill):
        buf = torch.full((SLACK + n + SLACK,), fill, dtype=dtype, device="cuda")
        return buf, buf[SLACK:SLACK + n]
    (bh, h), (bw, wi), (bp, pt), (bo, out) = framed(K * 8, torch.int64, 7), framed(K, torch.int32, 7), framed(K, torch.uint8, 7), \
        framed(H * W, torch.uint8, 7)
    h.zero_()
    s = ops._stream()
    _lib.call("segk_snap_vote", lab.data_ptr(), mask.data_ptr(), w.data_ptr(), h.data_ptr(), 255, rows, H, W, K, s)
    assert np.array_equal(h.cpu().numpy().reshape(K, 8), hist)
    _lib.call("segk_snap_paint", lab.data_ptr(), mask.data_ptr(), h.data_ptr(), wi.data_ptr(), pt.data_ptr(), out.data_ptr(), 255, 0, 0, 0,
              case.min_share, H, W, K, s)
    assert np.array_equal(wi.cpu().numpy(), win) and np.array_equal(out.cpu().numpy().reshape(H, W), want)
    for buf in (bh, bw, bp, bo):
        assert (buf[:SLACK] == 7).all() and (buf[-SLACK:] == 7).all()
    # a second vote adds to the table: the caller zeroes it
    _lib.call("segk_snap_vote", lab.data_ptr(), mask.data_ptr(), w.data_ptr(), h.data_ptr(), 255, rows, H, W, K, s)
    assert np.array_equal(h.cpu().numpy().reshape(K, 8), 2 * hist)


def test_c_entries_refuse_through_the_binding(seg):
    from image_segmentation_amd import _lib, ops
    x = torch.zeros((16, 24, 3), dtype=torch.uint8, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    cen, sums, lab, cnt = torch.zeros((6, 5), **i32), torch.zeros((6, 8), **i32), torch.full((16, 24), -9, **i32), torch.zeros((6,), **i32)
    s = ops._stream()
    good = (x.data_ptr(), cen.data_ptr(), sums.data_ptr(), lab.data_ptr(), 3, 1, 8, 20, 0, 1, 64, 16, 24, 6, s)
    for at, value, word in ((4, 2, "C 2"), (5, 3, "space"), (6, 3, "step"), (7, 0, "compactness"), (8, 1, "round"), (9, 21, "iterations"),
                            (10, 8, "tile_rows"), (11, 0, "shape"), (13, 5, "grid"), (3, 0, "NULL"), (2, sums.data_ptr() + 4, "aligned")):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match=word):
            _lib.call("segk_slic_assign", *args)
    with pytest.raises(RuntimeError, match="grid"):
        _lib.call("segk_slic_start", x.data_ptr(), cen.data_ptr(), sums.data_ptr(), 3, 1, 4, 16, 24, 6, s)
    with pytest.raises(RuntimeError, match="distinct"):
        _lib.call("segk_slic_update", cen.data_ptr(), sums.data_ptr(), cen.data_ptr(), 8, 16, 24, 6, s)
    mask, out = torch.zeros((16, 24), dtype=torch.uint8, device="cuda"), torch.zeros((16, 24), dtype=torch.uint8, device="cuda")
    hist, win, pt = torch.zeros((6, 8), dtype=torch.int64, device="cuda"), torch.zeros((6,), **i32), torch.zeros((6,), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="classes_mask"):
        _lib.call("segk_snap_vote", lab.data_ptr(), mask.data_ptr(), 0, hist.data_ptr(), 0, 64, 16, 24, 6, s)
    with pytest.raises(RuntimeError, match="tile_rows"):
        _lib.call("segk_snap_vote", lab.data_ptr(), mask.data_ptr(), 0, hist.data_ptr(), 255, 32, 16, 24, 6, s)
    with pytest.raises(RuntimeError, match="neither"):
        _lib.call("segk_snap_paint", lab.data_ptr(), mask.data_ptr(), hist.data_ptr(), win.data_ptr(), pt.data_ptr(), mask.data_ptr(), 255, 0, 0,
                  0, 128, 16, 24, 6, s)
    with pytest.raises(RuntimeError, match="min_share"):
        _lib.call("segk_snap_paint", lab.data_ptr(), mask.data_ptr(), hist.data_ptr(), win.data_ptr(), pt.data_ptr(), out.data_ptr(), 255, 0, 0,
                  0, 257, 16, 24, 6, s)
    torch.cuda.synchronize()
    assert (lab == -9).all() and (cen == 0).all() and (out == 0).all()             # nothing was launched
    with pytest.raises(ValueError, match="lives on|no CPU path"):
        seg.snap_mask(mask, lab.cpu(), k=6)


# ------------------------------------------------------------------------------------------------ Segmenter(snap=...)
SIZES = [(40, 56), (97, 75), (33, 61)]
T = 64
SNAP = dict(step=8, compactness=10, iterations=4, space="ycc", min_share=0.6, fill=(255,))
STEPS = [dict(op="open", classes=(1, 2, 3), radius=1, fill=0, shape="square"), dict(op="close", classes=(1,), radius=2)]
CLEAN = dict(min_area=20, keep_largest=(1, 2))
ROUTES = {"plain": dict(), "merged": dict(tta=dict(flips=("", "h"))), "tiled": dict(tiles=dict(size=32, overlap=8))}


def blocky(H, W, seed):
    """a uint8 [H,W,3] image of flat 6 x 6 blocks with a little noise: superpixels have edges to follow"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 4, size=(H // 6 + 1, W // 6 + 1, 3)) * 70
    img = np.kron(coarse, np.ones((6, 6, 1), dtype=np.int64))[:H, :W] + rng.integers(0, 20, size=(H, W, 3))
    return np.ascontiguousarray(img.astype(np.uint8))


@pytest.fixture(scope="module")
def setup(seg):
    """the small random-weight U-Net of tests/test_gpu_morph.py, three ragged 8-bit images and their label maps"""
    from oracle.fill import labels, fill_module
    from oracle import resize_ref, unet_ref
    images = [torch.from_numpy(blocky(h, w, 50 + i)) for i, (h, w) in enumerate(SIZES)]
    r = unet_ref.unet(3, 4)
    fill_module(r, 1000)
    Xb, _ = resize_ref.process_batch_forward([im.permute(2, 0, 1).float() / 255.0 for im in images], T)
    with torch.no_grad():
        r.train()
        for _ in range(20):
            r(Xb)
        r.eval()
        r.output.bias -= r(Xb).mean(dim=(0, 2, 3))
    m = seg.unet(3, 4)
    m.load_state_dict(r.state_dict())
    m.cuda().eval()
    labs = [labels(s, 80 + i, 4) for i, s in enumerate(SIZES)]
    return m, images, labs


def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("route", list(ROUTES))
def test_segmenter_snap_equals_the_composition_by_hand(seg, setup, route):
    m, images, labs = setup
    kw = dict(target_size=T, **ROUTES[route])
    plain = seg.Segmenter(m, **kw)(images, labels=labs)
    none = seg.Segmenter(m, snap=None, **kw)(images, labels=labs)
    for a, b in zip(none, plain):                           # snap=None: every output as without it
        assert same(a.mask, b.mask) and same(a.color, b.color) and same(a.counts, b.counts) and same(a.confusion, b.confusion)
        assert a.raw_mask is None and a.superpixels is None and same(a.confidence, b.confidence)
    pal = np.asarray([seg.COLOR_MAP[k] for k in range(4)], dtype=np.uint8)
    differ = 0
    for weighted in ((False,) if route == "plain" else (False, True)):
        snap = dict(SNAP, weighted=weighted)
        for morph, clean in ((None, None), (STEPS, CLEAN)):
            preds = seg.Segmenter(m, snap=snap if morph is None else seg.Snap(**snap), morph=morph, clean=clean, **kw)(images, labels=labs)
            for p, q, im, lab in zip(preds, plain, images, labs):
                assert torch.equal(p.raw_mask, q.mask)       # the argmax, bit for bit
                assert same(p.confidence, q.confidence)
                sp = seg.superpixels(im.cuda(), SNAP["step"], SNAP["compactness"], SNAP["iterations"], SNAP["space"])
                assert torch.equal(p.superpixels.labels, sp.labels) and torch.equal(p.superpixels.counts, sp.counts)
                assert p.superpixels.grid == sp.grid and p.superpixels.k == sp.k
                want = seg.snap_mask(q.mask, sp, min_share=SNAP["min_share"], fill=SNAP["fill"],
                                     weights=q.confidence if weighted else None).mask
                # ... which is the restatement's, on the device's own argmax
                ref = R.snap(sp.labels.cpu().numpy(), q.mask.cpu().numpy(), sp.k, q.confidence.cpu().numpy() if weighted else None,
                             range(8), SNAP["fill"], R.share_of(SNAP["min_share"]))[0]
                assert np.array_equal(want.cpu().numpy(), ref)
                differ += int((ref != q.mask.cpu().numpy()).sum())
                if morph is not None:
                    want = seg.close_mask(seg.open_mask(want, (1, 2, 3), 1, 0, "square"), (1,), 2)
                    comps = seg.components(want, **CLEAN)
                    assert torch.equal(p.components.labels, comps.labels)
                    want = comps.mask
                else:
                    assert p.components is None
                assert torch.equal(p.mask, want)
                mask = p.mask.cpu().numpy()
                assert np.array_equal(p.color.cpu().numpy(), pal[mask])
                assert np.array_equal(p.counts.cpu().numpy(), np.bincount(mask.ravel(), minlength=4))
                lab = lab.numpy()
                conf = np.zeros((4, 4), dtype=np.int64)
                np.add.at(conf, (mask.ravel().astype(np.int64), lab.ravel()), 1)
                assert np.array_equal(p.confusion.cpu().numpy(), conf)
    assert differ > 0                                        # snapping did change something


def test_segmenter_snap_refuses_what_it_cannot_do(seg, setup):
    m, images, labs = setup
    with pytest.raises(ValueError, match="weighted=True"):
        seg.Segmenter(m, target_size=T, snap=dict(weighted=True))                  # the plain route writes no confidence map
    floats = [im.permute(2, 0, 1).float() / 255.0 for im in images]
    calls = []
    hook = m.register_forward_pre_hook(lambda *a: calls.append(1))
    try:
        with pytest.raises(ValueError, match="uint8"):
            seg.Segmenter(m, target_size=T, snap=SNAP)(floats)
        assert not calls                                     # refused before the forward
        seg.Segmenter(m, target_size=T, snap=SNAP)(images[:1])
        assert calls
    finally:
        hook.remove()
