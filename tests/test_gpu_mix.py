"""MI355X: mixed-sample augmentation on the device (image_segmentation_amd/mix.py, csrc/mix.hip) against the
NumPy restatement (tests/mix_reference.py) on the shared case table (tests/mix_cases.py), bit for bit: every case x mode x
image and label format, with and without a seam -- images compared as raw bytes, labels, pasted; the launches themselves into
prefilled buffers whose slack must stay; repeats and a side stream; refused arguments; no synchronisation; MixedBatches in
front of train_loop."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_cases as MC                                                             # noqa: E402
import mix_reference as R                                                          # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 96
IMAGE_DTYPES = {4: (torch.float32,), 2: (torch.bfloat16, torch.float16), 1: (torch.uint8,)}
BITS = {4: torch.int32, 2: torch.int16, 1: torch.uint8}


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as seg
    return seg


def to_device(bits, dtype):
    """integer bit patterns -> a tensor of `dtype` with those bits"""
    eb = bits.dtype.itemsize
    return torch.from_numpy(bits.view({4: np.int32, 2: np.int16, 1: np.uint8}[eb]).copy()).cuda().view(dtype)


def raw(t):
    """a tensor's bits as unsigned integers on the host"""
    eb = t.element_size()
    return t.contiguous().view(BITS[eb]).cpu().numpy().view({4: np.uint32, 2: np.uint16, 1: np.uint8}[eb])


def mixer_for(seg, case, mode, seam):
    return seg.Mixer(MC.MODE_NAMES[mode], seed=0, **case.opts(seam_value=seam))


CELLS = [(c, m) for c in MC.CASES for m in MC.MODES]


@pytest.mark.parametrize("case,mode", CELLS, ids=[f"{c.name}-{MC.MODE_NAMES[m]}" for c, m in CELLS])
def test_every_case_equals_the_restatement(seg, case, mode):
    B, H, W = case.shape
    plans = case.plans(mode)
    side = torch.cuda.Stream()
    for k, (eb, ldt) in enumerate(MC.FORMATS):
        bits = case.image_bits(eb)
        lab = case.labels_as(ldt)
        dtype = IMAGE_DTYPES[eb][k % len(IMAGE_DTYPES[eb])]
        X = to_device(bits, dtype)
        y = torch.from_numpy(lab.copy()).cuda()
        if k % 2:
            y = y[:, None]                                   # [B,1,H,W], as the training loops carry it
        for seam in MC.SEAMS:
            want_X, want_y, want_p, _ = R.mix(bits, lab, plans, nhwc=eb == 1, **case.opts(seam_value=seam))
            mixer = mixer_for(seg, case, mode, seam)
            Xo, yo = mixer.apply(X, y, plans)
            pasted = mixer.last["pasted"]
            assert Xo.dtype == X.dtype and Xo.shape == X.shape and yo.dtype == y.dtype and yo.shape == y.shape
            assert pasted.dtype == torch.int32 and pasted.shape == (B,) and pasted.is_cuda
            tag = (eb, np.dtype(ldt).name, seam)
            assert np.array_equal(raw(Xo), want_X), tag
            assert np.array_equal(yo.cpu().numpy().reshape(B, H, W), want_y), tag
            assert np.array_equal(pasted.cpu().numpy(), want_p), tag
            Xa, ya = mixer.apply(X, y, plans)                # again, and on a side stream
            pa = mixer.last["pasted"]
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                Xs, ys = mixer.apply(X, y, plans)
                ps = mixer.last["pasted"]
            torch.cuda.current_stream().wait_stream(side)
            for a, b in ((Xa, Xo), (Xs, Xo)):
                assert np.array_equal(raw(a), raw(b)), tag
            assert torch.equal(ya, yo) and torch.equal(ys, yo) and torch.equal(pa, pasted) and torch.equal(ps, pasted), tag
        assert np.array_equal(raw(X), bits) and np.array_equal(y.cpu().numpy().reshape(B, H, W), lab)      # inputs untouched


@pytest.mark.parametrize("case,mode", CELLS, ids=[f"{c.name}-{MC.MODE_NAMES[m]}" for c, m in CELLS])
def test_launches_write_their_outputs_and_nothing_else(seg, case, mode):
    """out= places the three outputs inside 0xFF-prefilled buffers: the two launches write every output element and leave the
    slack on both sides as it was (the select table is inspected the same way through mixer.last)"""
    B, H, W = case.shape
    plans = case.plans(mode)
    for eb, ldt in MC.FORMATS:
        bits, lab = case.image_bits(eb), case.labels_as(ldt)
        X, y = to_device(bits, IMAGE_DTYPES[eb][0]), torch.from_numpy(lab.copy()).cuda()
        bufs, outs = [], []
        for t in (X, y, torch.empty((B,), dtype=torch.int32)):
            n = t.numel() * t.element_size()
            buf = torch.full((SLACK + n + SLACK,), 0xFF, dtype=torch.uint8, device="cuda")
            bufs.append((buf, n))
            outs.append(buf[SLACK:SLACK + n].view(t.dtype).view(t.shape))
        mixer = mixer_for(seg, case, mode, 250)
        Xo, yo = mixer.apply(X, y, plans, out=tuple(outs))
        assert Xo is outs[0] and yo is outs[1] and mixer.last["pasted"] is outs[2]
        want_X, want_y, want_p, _ = R.mix(bits, lab, plans, nhwc=eb == 1, **case.opts(seam_value=250))
        assert np.array_equal(raw(Xo), want_X) and np.array_equal(yo.cpu().numpy(), want_y)
        assert np.array_equal(outs[2].cpu().numpy(), want_p)
        for buf, n in bufs:
            assert (buf[:SLACK] == 0xFF).all() and (buf[SLACK + n:] == 0xFF).all()


def test_select_tables_equal_the_restatement(seg):
    """the selection itself: the 256-byte class table and the max_components-byte object table of every mixed sample"""
    for case in MC.CASES:
        B, H, W = case.shape
        o = case.opts()
        for mode in (R.CLASS, R.OBJECT):
            plans = case.plans(mode)
            for ldt in (np.int64, np.uint8):
                lab = case.labels_as(ldt)
                mixer = mixer_for(seg, case, mode, None)
                mixer.apply(to_device(case.image_bits(1), torch.uint8), torch.from_numpy(lab.copy()).cuda(), plans)
                select = mixer.last["tables"][1].cpu().numpy()
                for b, p in enumerate(plans):
                    if p.mode == R.CLASS:
                        want = R.select_classes(lab[p.partner], p.seed, o["exclude"], o.get("n_classes"))
                        assert np.array_equal(select[b, :256], want.astype(np.uint8)), (case.name, b)
                    elif p.mode == R.OBJECT:
                        _, chosen, _ = R.select_objects(lab[p.partner], p.seed, o["things"], o["connectivity"], o["min_area"],
                                                        o.get("max_area"), o["max_objects"], o["max_components"])
                        want = np.zeros(o["max_components"], dtype=np.uint8)
                        want[[i - 1 for i in chosen]] = 1
                        assert np.array_equal(select[b, :o["max_components"]], want), (case.name, b)


def test_refused_arguments(seg):
    case = next(c for c in MC.CASES if c.name == "one_tile")
    B, H, W = case.shape
    plans = case.plans(R.BOX)
    X = to_device(case.image_bits(4), torch.float32)
    y = torch.from_numpy(case.labels.copy()).cuda()
    mixer = seg.Mixer("cutmix", seed=0)
    wide = torch.zeros((B, case.C, H, 2 * W), device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        mixer.apply(wide[..., ::2], y, plans)
    with pytest.raises(ValueError, match="contiguous"):
        mixer.apply(X, torch.zeros((B, W, H), dtype=torch.int64, device="cuda").transpose(1, 2), plans)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixer.apply(X, y.cpu(), plans)
    pasted = torch.zeros((B,), dtype=torch.int32, device="cuda")
    fresh_X, fresh_y = torch.empty_like(X), torch.empty_like(y)
    before_X, before_y = X.clone(), y.clone()
    for out in ((X, fresh_y, pasted), (fresh_X, y, pasted),                        # the inputs themselves
                (X.view(-1)[1:].clone().view(-1), fresh_y, pasted),                # a wrong shape
                (fresh_X, fresh_y, pasted.long()), (fresh_X, fresh_y)):
        with pytest.raises(ValueError):
            mixer.apply(X, y, plans, out=out)
    # a partial overlap: an output that starts inside the input's memory
    pool = torch.zeros((2 * X.numel(),), device="cuda")
    Xin = pool[:X.numel()].view(X.shape)
    Xin.copy_(X)
    with pytest.raises(ValueError, match="overlaps"):
        mixer.apply(Xin, y, plans, out=(pool[X.numel() // 2:X.numel() // 2 + X.numel()].view(X.shape), fresh_y, pasted))
    with pytest.raises(ValueError, match="seam_value"):
        seg.Mixer("cutmix", seam_value=300).apply(X, y.to(torch.uint8), plans)
    # the C entry refuses the same overlap on its own
    from image_segmentation_amd import _lib, ops
    buf, (p_desc,) = seg.mix._upload([np.zeros(B, dtype=seg.mix.DESC)], X.device)
    select = torch.empty((B, 256), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="overlaps an input"):
        _lib.call("segk_mix_apply", p_desc, B, X.data_ptr(), y.data_ptr(), X.data_ptr() + 4, fresh_y.data_ptr(), pasted.data_ptr(), case.C, H,
                  W, 4, 8, select.data_ptr(), 256, 0, 0, 1, 0, 0, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(X.view(torch.int32), before_X.view(torch.int32)) and torch.equal(y, before_y)      # nothing was launched


def test_no_synchronisation(seg):
    X = torch.rand((8, 3, 48, 80), device="cuda")
    y = torch.from_numpy(MC.blocks(8, 48, 80, (0, 1, 2, 7, 255), 9)).cuda()[:, None]
    mixer = seg.Mixer(("cutmix", "classmix", "copy_paste"), p=0.9, exclude=(255,), seam_value=255, flip=True, max_shift=0.25, min_area=8,
                      seed=3)
    mixer(X, y)                                              # the first call loads the library and the kernels
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            Xo, yo = mixer(X, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not [w for w in caught if "synchron" in str(w.message).lower()], [str(w.message) for w in caught]
    plans = mixer.last["plans"]
    assert len({p.mode for p in plans}) >= 3
    want_X, want_y, want_p, _ = R.mix(raw(X), y.cpu().numpy(), plans, exclude=(255,), seam_value=255, min_area=8)
    assert np.array_equal(raw(Xo), want_X) and np.array_equal(yo.cpu().numpy(), want_y)
    assert np.array_equal(mixer.last["pasted"].cpu().numpy(), want_p) and want_p.any()


def test_mixed_batches_drive_train_loop(seg):
    from image_segmentation_amd import training
    from oracle.fill import fill_module
    training.VERBOSE = False
    rng = np.random.default_rng(5)
    sizes = ((40, 56), (33, 61), (48, 48), (64, 37))
    imgs = [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for h, w in sizes]
    labs = [torch.from_numpy(MC.blocks(1, h, w, (0, 1, 2, 3), i)[0].astype(np.uint8)) for i, (h, w) in enumerate(sizes)]
    loader = [(imgs, labs)]

    def run(wrap):
        batches = seg.AugmentedBatches(loader, seg.Augmenter(target_size=32, seed=1))
        if wrap is not None:
            batches = seg.MixedBatches(batches, wrap)
            assert len(batches) == 1
        m = seg.unet(3, 4)
        fill_module(m, 1000)
        m.cuda()
        loss = training.train_loop(batches, m, seg.CrossEntropyLoss(), torch.optim.SGD(m.parameters(), lr=0.01), 1, torch.device("cuda"))
        return loss, m.output.weight.detach().clone()

    plain, w_plain = run(None)
    off, w_off = run(seg.Mixer(("cutmix", "classmix", "copy_paste"), p=0.0, seed=2))
    assert np.isfinite(plain) and np.float64(plain).tobytes() == np.float64(off).tobytes() and torch.equal(w_plain, w_off)
    mixer = seg.Mixer(("cutmix", "classmix", "copy_paste"), p=1.0, min_area=4, max_shift=0.25, flip=True, seed=2)
    on, w_on = run(mixer)
    assert np.isfinite(on) and on > 0 and torch.isfinite(w_on).all()
    assert int(mixer.last["pasted"].sum()) > 0 and np.float64(on).tobytes() != np.float64(plain).tobytes()
