"""GPU (-m gpu): the prediction surface (image_segmentation_amd/inference.py; reference segmentation_webapp/app.py:
250-326) and its two kernels, segk_predict_mask and segk_resize_pad_u8 (csrc/resize.hip).

  1. the fused mask / colour / counts / confusion equal the package's own materialised route (segk_crop_resize +
     torch.argmax + palette index + bincount + segk_confusion) BIT FOR BIT: same device function, same expression order,
     -ffp-contract=off;
  2. against the CPU oracle (oracle/resize_ref.py) a pixel may differ only where the oracle's top-two gap is below twice
     the measured logit distance d, and at most 1 pixel in 2000 does;
  3. an 8-bit interleaved image gives the slot the float route gives for image / 255, bit for bit;
  4. Segmenter end to end on ragged images against both routes, model state untouched, chunking, the prompt model;
  5. argument errors of the device build."""
import warnings

import numpy as np
import pytest
import torch

from oracle.fill import fill, labels, fill_module
from oracle import resize_ref, unet_ref

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (500, 375), (20, 30), (33, 65), (64, 17), (1200, 1600)]
PALETTE = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (90, 160, 250)]


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import image_segmentation_amd as s
    return s


def metas_for(shapes, T):
    from image_segmentation_amd.utils import process_batch_forward
    _, metas = process_batch_forward([torch.zeros((1,) + s) for s in shapes], target_size=T, device="cuda")
    return metas


def fused(slot, meta, mode, palette=None, labs=None, want_counts=True):
    """segk_predict_mask on one slot [C,T,T] -> (mask, color, counts[C], M[C,C])"""
    from image_segmentation_amd import _lib
    C, T, _ = slot.shape
    pl, pt, _, _ = meta["pad"]
    nh, nw = meta["new_size"]
    oh, ow = meta["original_size"]
    mask = torch.full((oh, ow), 77, dtype=torch.uint8, device="cuda")
    color = torch.full((oh, ow, 3), 77, dtype=torch.uint8, device="cuda") if palette is not None else None
    counts = torch.zeros(8, dtype=torch.int64, device="cuda") if want_counts else None
    M = torch.zeros((8, 8), dtype=torch.int64, device="cuda") if labs is not None else None
    p = lambda t: None if t is None else t.data_ptr()
    _lib.call("segk_predict_mask", slot.data_ptr(), mask.data_ptr(), p(color), p(palette), p(counts), p(labs), p(M), C, T, pt, pl,
              nh, nw, oh, ow, mode, torch.cuda.current_stream().cuda_stream)
    return mask, color, None if counts is None else counts[:C], None if M is None else M[:C, :C]


@pytest.mark.parametrize("interp", ["bilinear", "nearest"])
@pytest.mark.parametrize("C", [1, 3, 4, 8])
@pytest.mark.parametrize("T", [64, 224])
def test_fused_mask_equals_materialised_route(seg, T, C, interp):
    from image_segmentation_amd.utils import process_batch_reverse
    from image_segmentation_amd import ops
    metas = metas_for(SHAPES, T)
    logits = fill((len(SHAPES), C, T, T), 7, -3, 3).cuda()
    full = process_batch_reverse(logits, metas, interpolation=interp)
    pal = torch.tensor(PALETTE, dtype=torch.uint8, device="cuda")
    mode = 1 if interp == "nearest" else 0
    for n, ((h, w), meta) in enumerate(zip(SHAPES, metas)):
        lab = labels((h, w), 40 + n, C)
        if n == 1:
            lab[::7, ::5] = 255                                   # ignore pixels: skipped, as segk_confusion skips them
        lab = lab.cuda()
        want = full[n].argmax(0)
        mask, color, counts, M = fused(logits[n], meta, mode, pal, lab)
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (h, w)
        assert torch.equal(mask.long(), want), (n, int((mask.long() != want).sum()))
        assert torch.equal(counts, torch.bincount(mask.flatten().long(), minlength=C))
        assert torch.equal(color, pal[mask.long()])
        assert torch.equal(M, ops.confusion_matrix(full[n], lab, C))
        # every optional output off: the mask alone, nothing else required
        mask2, _, _, _ = fused(logits[n], meta, mode, None, None, want_counts=False)
        assert torch.equal(mask2, mask)


@pytest.mark.parametrize("interp", ["bilinear", "nearest"])
def test_nan_is_maximal_then_first_index_wins(seg, interp):
    from image_segmentation_amd.utils import process_batch_reverse
    T, C = 64, 4
    meta = metas_for([(64, 64)], T)[0]                            # identity geometry: output pixel (y,x) reads slot (y,x)
    slot = fill((C, T, T), 9, -3, 3)
    slot[2, 10, 20] = float("nan")                                # NaN beats every number
    slot[1, 40, 7] = float("nan"); slot[3, 40, 7] = float("nan")  # two NaNs: the first
    slot[0, 30, 40] = 5.0; slot[3, 30, 40] = 5.0                  # exact tie above the fill range: the lowest index
    slot[1, 50, 50] = 4.0; slot[2, 50, 50] = 4.0
    slot = slot.cuda()
    mask, _, counts, _ = fused(slot, meta, 1 if interp == "nearest" else 0)
    assert (int(mask[10, 20]), int(mask[40, 7]), int(mask[30, 40]), int(mask[50, 50])) == (2, 1, 0, 1)
    want = process_batch_reverse(slot[None], [meta], interpolation=interp)[0].argmax(0)
    assert torch.equal(mask.long(), want)
    assert int(counts.sum()) == 64 * 64


@pytest.mark.parametrize("C", [1, 3, 4, 8])
@pytest.mark.parametrize("T", [64, 224])
def test_fused_mask_vs_cpu_oracle(seg, T, C):
    from image_segmentation_amd.utils import process_batch_reverse
    metas = metas_for(SHAPES, T)
    logits = fill((len(SHAPES), C, T, T), 7, -3, 3)
    dev = logits.cuda()
    full = process_batch_reverse(dev, metas, interpolation="bilinear")
    near = process_batch_reverse(dev, metas, interpolation="nearest")
    close = allowed = total = 0
    d = 0.0
    for n, meta in enumerate(metas):
        ref = resize_ref.reverse_resize_and_padding(logits[n], meta, "bilinear")
        d = max(d, float((full[n].cpu() - ref).abs().max()))
    print(f"T={T} C={C}: d = max|GPU logits - oracle logits| = {d:.3e}")
    assert d < 5e-5                                               # the bound of test_gpu_evalpipe.py::test_reverse
    for n, meta in enumerate(metas):
        ref = resize_ref.reverse_resize_and_padding(logits[n], meta, "bilinear")
        mask = fused(dev[n], meta, 0)[0].cpu().long()
        differs = mask != ref.argmax(0)
        if C == 1:
            assert not differs.any()
        else:
            top = ref.topk(2, dim=0).values
            near_tie = (top[0] - top[1]) < 2 * d
            assert not (differs & ~near_tie).any(), (n, int((differs & ~near_tie).sum()))
            allowed += int(near_tie.sum())
        close += int(differs.sum()); total += differs.numel()
        # nearest: no arithmetic, equal everywhere
        rn = resize_ref.reverse_resize_and_padding(logits[n], meta, "nearest")
        assert torch.equal(near[n].cpu(), rn)
        assert torch.equal(fused(dev[n], meta, 1)[0].cpu().long(), rn.argmax(0))
    print(f"T={T} C={C}: {allowed} of {total} pixels lie inside the 2d gap, {close} of them differ from the oracle's argmax")
    assert close <= allowed and allowed * 2000 <= total           # the pixels that MAY differ are at most 1 in 2000


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("cin", [1, 3, 4])
@pytest.mark.parametrize("T", [64, 224])
def test_u8_image_equals_float_route(seg, T, cin, mode):
    from image_segmentation_amd import inference
    from image_segmentation_amd.utils import process_batch_forward, NEAREST, BILINEAR
    interp = NEAREST if mode == 1 else BILINEAR
    antialias = mode == 0
    co = min(cin, 3)
    worst = 0.0
    for i, (h, w) in enumerate(SHAPES):
        u8 = (fill((h, w, cin), 20 + i, 0, 1) * 255).round().byte()
        as_float = u8.permute(2, 0, 1).float().div(255)
        want, wmeta = process_batch_forward([as_float], target_size=T, interpolation=interp, device="cuda", antialias=antialias)
        slot = torch.full((co, T, T), 7.0, device="cuda")
        meta = inference._into_slot(u8.cuda(), slot, T, interp, antialias, "image")
        assert meta == wmeta[0]
        assert torch.equal(slot, want[0]), (h, w, float((slot - want[0]).abs().max()))
        ref, _ = resize_ref.process_batch_forward([as_float], T, nearest=(mode == 1), antialias=antialias)
        worst = max(worst, float((slot.cpu() - ref[0]).abs().max()))
    print(f"T={T} Cin={cin} mode={mode}: max|u8 slot - oracle| = {worst:.3e}")
    assert worst < 2e-6
    # [H,W] is the one-channel form (a prompt heat-map drawn as an 'L' image)
    if cin == 1:
        slot2 = torch.empty((1, T, T), device="cuda")
        inference._into_slot(u8[:, :, 0].cuda(), slot2, T, interp, antialias, "heatmap")
        assert torch.equal(slot2, slot)


E2E_SIZES = [(40, 56), (64, 48), (33, 61), (64, 64), (500, 375), (37, 53)]


def prepared_reference(images, T):
    """oracle U-Net whose eval-mode argmax is not one class everywhere: settled BatchNorm buffers, centred head bias"""
    r = unet_ref.unet(3, 4)
    fill_module(r, 1000)
    Xb, _ = resize_ref.process_batch_forward(images, T)
    with torch.no_grad():
        r.train()
        for _ in range(20):
            r(Xb)
        r.eval()
        r.output.bias -= r(Xb).mean(dim=(0, 2, 3))
    return r


def oracle_check(r, images, masks, gpu_logits, T, cap):
    """pixels may differ from the oracle pipeline only inside twice the measured logit distance; at most `cap` of them do"""
    Xb, metas = resize_ref.process_batch_forward(images, T)
    with torch.no_grad():
        out = r(Xb)
    refs = [resize_ref.reverse_resize_and_padding(o, m) for o, m in zip(out, metas)]
    d = max(float((g.cpu() - ref).abs().max()) for g, ref in zip(gpu_logits, refs))
    close = allowed = total = 0
    for mask, ref in zip(masks, refs):
        differs = mask.cpu().long() != ref.argmax(0)
        top = ref.topk(2, dim=0).values
        near_tie = (top[0] - top[1]) < 2 * d
        assert not (differs & ~near_tie).any()
        close += int(differs.sum()); allowed += int(near_tie.sum()); total += differs.numel()
    hist = torch.bincount(torch.cat([m.flatten() for m in masks]).long().cpu(), minlength=4).double()
    print(f"end to end: d = {d:.3e}, {allowed} of {total} pixels inside the 2d gap, {close} differ from the oracle, "
          f"class shares {(hist / hist.sum()).tolist()}")
    assert close <= allowed <= cap * total
    assert (hist > 0).sum() >= 3                                  # the preparation worked: not one class everywhere
    return d


def test_segmenter_end_to_end(seg):
    from image_segmentation_amd.utils import process_batch_forward, process_batch_reverse
    T = 64
    images = [fill((3,) + s, 70 + i, 0, 1) for i, s in enumerate(E2E_SIZES)]
    u8s = [(im * 255).round().byte().permute(1, 2, 0).contiguous() for im in images]
    u8_as_float = [u.permute(2, 0, 1).float().div(255) for u in u8s]
    r = prepared_reference(images, T)
    seg.set_compute_dtype(torch.float32)
    try:
        m = seg.unet(3, 4)
        m.load_state_dict(r.state_dict())
        m.cuda().eval()
        s32 = seg.Segmenter(m, target_size=T)
        assert s32.num_classes == 4

        def materialised(imgs):
            X, metas = process_batch_forward(imgs, target_size=T, device="cuda")
            with torch.no_grad():
                return process_batch_reverse(m(X), metas), metas

        for inputs, floats in ((images, images), (u8s, u8_as_float), ([u.numpy() for u in u8s], u8_as_float),
                               ([im.cuda() for im in images], images)):
            preds = s32(inputs)
            full, metas = materialised(floats)
            assert len(preds) == len(images)
            for p, f, mt, im in zip(preds, full, metas, images):
                assert p.mask.is_cuda and p.mask.dtype == torch.uint8 and tuple(p.mask.shape) == tuple(im.shape[1:])
                assert torch.equal(p.mask.long(), f.argmax(0))
                assert p.color.dtype == torch.uint8 and torch.equal(p.color, torch.tensor(PALETTE[:4], dtype=torch.uint8,
                                                                                      device="cuda")[p.mask.long()])
                assert p.counts.dtype == torch.int64 and torch.equal(p.counts, torch.bincount(p.mask.flatten().long(), minlength=4))
                assert p.confusion is None and p.meta == mt
            d = oracle_check(r, floats, [p.mask for p in preds], full, T, cap=0.01)
            assert d <= 1.2e-4                                    # eight times the 1.5e-5 the project records for fp32 logits

        # labels: the confusion counts of the same pass equal segk_confusion on the materialised logits
        labs = [labels(s, 80 + i, 4) for i, s in enumerate(E2E_SIZES)]
        labs[2][::3, ::4] = 255
        labs[3] = labs[3][None]
        preds = s32(images, labels=labs)
        full, _ = materialised(images)
        from image_segmentation_amd import ops
        for p, f, lab in zip(preds, full, labs):
            assert torch.equal(p.confusion, ops.confusion_matrix(f, lab.cuda().reshape(f.shape[1:]), 4))

        # chunking, no palette, the one-shot form
        small = seg.Segmenter(m, target_size=T, batch_size=4, palette=None)(images)
        one = seg.predict(m, images, target_size=T)
        for a, b, c in zip(small, s32(images), one):
            assert torch.equal(a.mask, b.mask) and torch.equal(c.mask, b.mask) and a.color is None

        # a model left in train(): mode and every buffer as they were
        m.train()
        m.down1.eval()                                            # a mixed tree comes back mixed
        before = {k: v.clone() for k, v in m.state_dict().items()}
        modes = [x.training for x in m.modules()]
        again = s32(images)
        assert m.training and [x.training for x in m.modules()] == modes
        after = m.state_dict()
        assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
        assert any(k.endswith("num_batches_tracked") for k in before)
        for a, b in zip(again, one):
            assert torch.equal(a.mask, b.mask)
        assert seg.get_compute_dtype() == torch.float32           # the global compute dtype is not touched
    finally:
        seg.set_compute_dtype(torch.bfloat16)


def test_segmenter_device_inputs_do_not_synchronise(seg):
    m = seg.unet(3, 4); fill_module(m, 1000); m.cuda().eval()
    s = seg.Segmenter(m, target_size=64)
    images = [fill((3,) + sz, 70 + i, 0, 1).cuda() for i, sz in enumerate(E2E_SIZES[:3])]
    u8s = [(im * 255).round().byte().permute(1, 2, 0).contiguous() for im in images]
    labs = [labels(sz, 80 + i, 4).cuda() for i, sz in enumerate(E2E_SIZES[:3])]
    s(images, labels=labs); s(u8s)                                # first call: palette upload, lazy initialisation
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception as e:                                        # not every build implements the mode
        pytest.skip(f"sync debug mode unavailable: {e}")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            s(images, labels=labs)
            s(u8s)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sync = [str(w.message) for w in rec if "synchroniz" in str(w.message).lower()]
    assert not sync, sync


def test_segmenter_prompt_model(seg):
    from image_segmentation_amd.utils import process_batch_forward, process_batch_reverse
    seg.set_compute_dtype(torch.float32)
    try:
        clip = seg.unet(3, 4)                  # stand-in for the 4-class CLIP-UNet, as tests/test_gpu_prompt.py builds it
        fill_module(clip, 9000)
        m = seg.PromptModel(clip=clip)
        fill_module(m.mask, 9500)
        m.cuda().eval()
        sizes = E2E_SIZES[:4]
        images = [fill((3,) + s, 70 + i, 0, 1) for i, s in enumerate(sizes)]
        heats = [fill((1,) + s, 90 + i, 0, 1) for i, s in enumerate(sizes)]
        s = seg.Segmenter(m, target_size=64, batch_size=3)
        assert s.num_classes == 4
        preds = s(images, heatmaps=heats)
        X, metas = process_batch_forward(images, target_size=64, device="cuda")
        Hm, _ = process_batch_forward(heats, target_size=64, device="cuda")
        with torch.no_grad():
            full = process_batch_reverse(m(X, Hm), metas)
        for p, f in zip(preds, full):
            assert torch.equal(p.mask.long(), f.argmax(0))
        # 8-bit heat-maps ([H,W], as an 'L' image) take the 8-bit kernel
        h8 = [(h[0] * 255).round().byte() for h in heats]
        preds8 = s(images, heatmaps=h8)
        Hm8, _ = process_batch_forward([h.float().div(255)[None] for h in h8], target_size=64, device="cuda")
        with torch.no_grad():
            full8 = process_batch_reverse(m(X, Hm8), metas)
        for p, f in zip(preds8, full8):
            assert torch.equal(p.mask.long(), f.argmax(0))
        with pytest.raises(ValueError, match="pass heatmaps"):
            s(images)
        with pytest.raises(ValueError, match="heatmap 0 is"):
            s(images[:1], heatmaps=[heats[1]])
        with pytest.raises(ValueError, match="takes the image alone"):
            seg.Segmenter(clip.cuda())(images, heatmaps=heats)
    finally:
        seg.set_compute_dtype(torch.bfloat16)


def test_predict_rejects_bad_arguments(seg):
    from image_segmentation_amd import _lib
    t = torch.zeros(9 * 16 * 16, device="cuda")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()
    with pytest.raises(RuntimeError, match="outside the slot"):
        _lib.call("segk_predict_mask", P(t), P(b), None, None, None, None, None, 4, 16, 10, 0, 8, 8, 4, 4, 0, s)
    with pytest.raises(RuntimeError, match="classes supported, got 9"):
        _lib.call("segk_predict_mask", P(t), P(b), None, None, None, None, None, 9, 16, 0, 0, 8, 8, 4, 4, 0, s)
    with pytest.raises(RuntimeError, match="color and palette come together"):
        _lib.call("segk_predict_mask", P(t), P(b), P(b), None, None, None, None, 4, 16, 0, 0, 8, 8, 4, 4, 0, s)
    with pytest.raises(RuntimeError, match="labels and M come together"):
        _lib.call("segk_predict_mask", P(t), P(b), None, None, None, P(t), None, 4, 16, 0, 0, 8, 8, 4, 4, 0, s)
    with pytest.raises(RuntimeError, match="bad mode"):
        _lib.call("segk_predict_mask", P(t), P(b), None, None, None, None, None, 4, 16, 0, 0, 8, 8, 4, 4, 2, s)
    with pytest.raises(RuntimeError, match="1, 3 or 4"):
        _lib.call("segk_resize_pad_u8", P(b), P(t), 2, 8, 8, 8, 8, 16, 0, 0, 0, s)
    with pytest.raises(RuntimeError, match="outside the target"):
        _lib.call("segk_resize_pad_u8", P(b), P(t), 3, 8, 8, 20, 20, 16, 0, 0, 0, s)
    # Segmenter refuses a short palette before anything is launched
    with pytest.raises(ValueError, match="palette has 2 rows"):
        seg.Segmenter(seg.unet(3, 4).cuda(), target_size=32, palette=[(0, 0, 0), (9, 9, 9)])
