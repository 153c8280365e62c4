"""GPU (-m gpu): confidence calibration -- segk_calib_hist, segk_calib_temps, reliability(), fit_temperature()
and Segmenter(temperature=...).

  1. segk_calib_hist equals the restatement (tests/calibration_reference.py) in every counter; calls add; an all-ignored label
     map leaves the buffer untouched;
  2. at inv_T = 1.0 the sweep's histogram equals, bit for bit, segk_calib_hist of the mask and confidence segk_predict_merge
     returns for the same slot (one view, "prob", weight 1), summed over classes; valid = the valid labels; sum of correct =
     the trace of segk_predict_mask's confusion counts over the valid labels;
  3. against float64, per temperature j.  Mean NLL: |device - float64| <= 4 d_nll[j] + 2^-17, d_nll[j] the float32
     restatement's largest per-pixel NLL distance from float64 on the same input (a mean's error is bounded by the per-pixel
     maximum; 4 covers the device expf / logf against NumPy's, as in 3.4; 2^-17 is the fixed point).  Histogram: a pixel is
     ambiguous when the float64 255 p_best + 0.5 lies within 255 4 d_p[j] of an integer or the float64 top-two gap of z is below
     twice the z distance; an ambiguous pixel may sit in another bin, which moves two entries of a column, so per column (count,
     correct) sum_q |device - float64| <= 2 ambiguous; the total counts are equal.  At most 1 pixel in 20 is ambiguous (a
     condition on the inputs: tests/test_calibration_host.py shows the restatement alone meets it);
  4. two runs are bit-identical in every output;
  5. NaN logits, exact ties, C = 1;
  6. end to end on a small U-Net and ragged images;
  7. refusals."""
import numpy as np
import pytest
import torch

import calibration_reference as CR
from oracle.fill import fill, labels, fill_module

pytestmark = pytest.mark.gpu

SHAPES, SIZES = CR.SHAPES, CR.SIZES
PALETTE = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)]


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import image_segmentation_amd as s
    return s


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def calib_hist(conf, mask, lab, C, ignore=-1, out=None):
    from image_segmentation_amd import _lib
    out = torch.zeros((8, 256, 2), dtype=torch.int64, device="cuda") if out is None else out
    H, W = conf.shape
    _lib.call("segk_calib_hist", P(conf), P(mask), P(lab), H, W, C, ignore, P(out), stream())
    return out


def calib_temps(slot, geo, shape, lab, C, ignore, inv, mode=0, out=None):
    """segk_calib_temps on CUDA tensors; inv: a float32 CUDA tensor (its length is K) -> dict(hist [K,256,2], nll_fx, nonfinite, valid)"""
    from image_segmentation_amd import _lib
    K = int(inv.numel())
    if out is None:
        out = dict(hist=torch.zeros((K, 256, 2), dtype=torch.int64, device="cuda"), nll_fx=torch.zeros(K, dtype=torch.int64, device="cuda"),
                   nonfinite=torch.zeros(K, dtype=torch.int64, device="cuda"), valid=torch.zeros(1, dtype=torch.int64, device="cuda"))
    _lib.call("segk_calib_temps", P(slot), C, slot.shape[-1], geo["pad_top"], geo["pad_left"], geo["nh"], geo["nw"], shape[0], shape[1],
              mode, P(lab), ignore, P(inv), K, P(out["hist"]), P(out["nll_fx"]), P(out["nonfinite"]), P(out["valid"]), stream())
    return out


def merge_one_view(slot, geo, shape, C, mode):
    """segk_predict_merge, one logits view of weight 1, "prob" -> (mask, conf)"""
    from image_segmentation_amd import _lib, tta
    table = tta.view_table([(slot.data_ptr(), slot.shape[-1], geo["pad_top"], geo["pad_left"], geo["nh"], geo["nw"], 0, 0, 1.0)])
    dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
    mask = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    conf = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    _lib.call("segk_predict_merge", P(dev), 1, C, 0, mode, shape[0], shape[1], P(mask), None, None, None, None, None, P(conf), None, stream())
    torch.cuda.synchronize()
    return mask, conf


# ---- 1. the histogram entry --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", CR.CLASSES)
def test_calib_hist_equals_the_restatement(seg, C):
    for n, shape in enumerate(SHAPES):
        u = fill(shape, 300 + n + C, 0, 1).numpy()
        conf = np.where(u < 0.6, 255, np.floor(u * 640) % 256).astype(np.uint8)       # most pixels in the top bin, the rest spread
        mask = labels(shape, 310 + n, C).numpy().astype(np.uint8)
        if n == 0:
            mask[3, ::4] = C + 1                                                      # a mask value past the classes
        lab = labels(shape, 320 + n + C, C).numpy()
        lab[::7, ::5] = 255
        lab[1, :3] = -4
        ign = CR.IGNORE if C > 2 else -1
        want = CR.hist_reference(conf, mask, lab, C, ign)
        dc, dm, dl = torch.from_numpy(conf).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(lab).cuda()
        got = calib_hist(dc, dm, dl, C, ign)
        assert np.array_equal(got[:C].cpu().numpy(), want) and int(got[C:].sum()) == 0, (shape, C)
        assert int(want[:, :, 0].sum()) == int(CR.valid_labels(lab, C, ign).sum())
        calib_hist(dc, dm, dl, C, ign, out=got)                                       # a second call adds
        assert np.array_equal(got[:C].cpu().numpy(), 2 * want)
        before = got.clone()
        calib_hist(dc, dm, torch.full(shape, 255, dtype=torch.int64, device="cuda"), C, ign, out=got)
        if C > 2:
            calib_hist(dc, dm, torch.full(shape, ign, dtype=torch.int64, device="cuda"), C, ign, out=got)
        assert torch.equal(got, before)                                               # all ignored: untouched


# ---- 2. inv_T = 1 is segk_predict_merge ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C", CR.CLASSES)
def test_sweep_at_one_equals_predict_merge(seg, C, mode):
    from image_segmentation_amd import _lib
    one = torch.ones(1, device="cuda")
    for T in SIZES:
        for n in range(len(SHAPES)):
            shape, geo, slot, lab, ign = CR.case(n, T, C)
            slot, dl = torch.from_numpy(slot).cuda(), torch.from_numpy(lab).cuda()
            mask, conf = merge_one_view(slot, geo, shape, C, mode)
            want = calib_hist(conf, mask, dl, C, ign).sum(0)
            got = calib_temps(slot, geo, shape, dl, C, ign, one, mode)
            assert torch.equal(got["hist"][0], want), (T, shape, int((got["hist"][0] - want).abs().sum()))
            nvalid = int(CR.valid_labels(lab, C, ign).sum())
            assert int(got["valid"]) == nvalid == int(got["hist"][0, :, 0].sum())
            only_valid = torch.where(torch.from_numpy(CR.valid_labels(lab, C, ign).reshape(shape)).cuda(), dl, torch.full_like(dl, 255))
            M = torch.zeros((8, 8), dtype=torch.int64, device="cuda")
            m2 = torch.empty(shape, dtype=torch.uint8, device="cuda")
            _lib.call("segk_predict_mask", P(slot), P(m2), None, None, None, P(only_valid), P(M), C, T, geo["pad_top"], geo["pad_left"],
                      geo["nh"], geo["nw"], shape[0], shape[1], mode, stream())
            assert int(got["hist"][0, :, 1].sum()) == int(M.diagonal().sum())
            if C > 1:
                assert 0 < int(M.diagonal().sum()) < nvalid


# ---- 3. against float64 --------------------------------------------------------------------------------------------------------

def reference(n, T, C, mode, K):
    """the float64 restatement of one case over TABLE[:K], reduced to what the gates need"""
    shape, geo, slot, lab, ign = CR.case(n, T, C)
    inv = CR.inverse_temperatures(CR.TABLE[:K])
    s64 = CR.sweep(slot, geo, shape, lab, C, inv, ign, mode, np.float64)
    s32 = CR.sweep(slot, geo, shape, lab, C, inv, ign, mode, np.float32)
    d_nll, d_p, d_z = CR.distances(s32, s64)
    amb = CR.ambiguous(s64, d_p, d_z).sum(axis=1)
    return dict(hist=s64["hist"], nll=[CR.mean_nll(s64, j) for j in range(K)], d_nll=d_nll, d_p=d_p, d_z=d_z, amb=amb, valid=s64["valid"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C", CR.CLASSES)
def test_sweep_against_float64(seg, C, mode):
    worst = dict(nll=0.0, gate=1.0, d_nll=0.0, d_p=0.0, share=0.0, moved=0, amb=0)
    table = torch.from_numpy(CR.inverse_temperatures(CR.TABLE)).cuda()
    for T in SIZES:
        for n in range(len(SHAPES)):
            shape, geo, slot, lab, ign = CR.case(n, T, C)
            Ks = (1, 17) if shape[0] * shape[1] > 100000 else (1, 17, 32)              # the large image: 17 temperatures
            ref = reference(n, T, C, mode, max(Ks))
            slot, dl = torch.from_numpy(slot).cuda(), torch.from_numpy(lab).cuda()
            for K in Ks:
                part = CR.KS[K]
                got = calib_temps(slot, geo, shape, dl, C, ign, table[part], mode)
                hist = got["hist"].cpu().numpy()
                valid, nonf, fx = int(got["valid"]), got["nonfinite"].cpu().numpy(), got["nll_fx"].cpu().numpy()
                assert valid == ref["valid"] and not nonf.any()
                for jj, j in enumerate(range(part.start, part.stop)):
                    nll = int(fx[jj]) / 65536 / valid
                    gate = 4 * ref["d_nll"][j] + 2.0 ** -17
                    moved = np.abs(hist[jj] - ref["hist"][j]).sum(axis=0)               # per column: count, correct
                    share = ref["amb"][j] / valid
                    print(f"C={C} mode={mode} T={T} {shape} K={K} 1/T={float(table[j]):.4f}: |nll - float64| = {abs(nll - ref['nll'][j]):.3e} "
                          f"(gate {gate:.3e}, d_nll {ref['d_nll'][j]:.3e}, d_p {ref['d_p'][j]:.3e}, d_z {ref['d_z']:.3e}); bins moved "
                          f"{moved.tolist()}, ambiguous {int(ref['amb'][j])} of {valid} ({share:.4f})")
                    if abs(nll - ref["nll"][j]) / gate > worst["nll"] / worst["gate"]:
                        worst.update(nll=abs(nll - ref["nll"][j]), gate=gate)
                    worst.update(d_nll=max(worst["d_nll"], ref["d_nll"][j]), d_p=max(worst["d_p"], ref["d_p"][j]),
                                 share=max(worst["share"], share))
                    if moved.max() > worst["moved"]:
                        worst.update(moved=int(moved.max()), amb=int(ref["amb"][j]))
                    assert abs(nll - ref["nll"][j]) <= gate
                    assert int(hist[jj, :, 0].sum()) == valid == int(ref["hist"][j, :, 0].sum())
                    assert moved.max() <= 2 * ref["amb"][j]
                    assert ref["amb"][j] * 20 <= valid
    print(f"C={C} mode={mode} worst: {worst}")


# ---- 4. stability ------------------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_identical(seg):
    table = torch.from_numpy(CR.inverse_temperatures(CR.TABLE)).cuda()
    for n, T, C in ((1, 224, 4), (1, 64, 8), (3, 64, 3)):
        shape, geo, slot, lab, ign = CR.case(n, T, C)
        slot, dl = torch.from_numpy(slot).cuda(), torch.from_numpy(lab).cuda()
        a = calib_temps(slot, geo, shape, dl, C, ign, table)
        b = calib_temps(slot, geo, shape, dl, C, ign, table)
        for k in a:
            assert torch.equal(a[k], b[k]), k
        mask, conf = merge_one_view(slot, geo, shape, C, 0)
        assert torch.equal(calib_hist(conf, mask, dl, C, ign), calib_hist(conf, mask, dl, C, ign))
        calib_temps(slot, geo, shape, dl, C, ign, table, out=a)                       # a second call adds
        for k in a:
            assert torch.equal(a[k], 2 * b[k]), k


# ---- 5. NaN, ties, one class ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_nan_ties_and_one_class(seg, mode):
    T, C = 64, 4
    geo = CR.geometry((T, T), T)                                   # identity geometry: output pixel (y,x) reads slot (y,x)
    inv = torch.from_numpy(CR.inverse_temperatures([0.5, 1.0, 2.0])).cuda()
    slot = fill((C, T, T), 9, -1, 1)
    lab = labels((T, T), 11, C)
    base = calib_temps(slot.cuda(), geo, (T, T), lab.cuda(), C, -1, inv, mode)
    assert int(base["nonfinite"].sum()) == 0
    nan = slot.clone()
    nan[2, 10, 20] = float("nan")
    got = calib_temps(nan.cuda(), geo, (T, T), lab.cuda(), C, -1, inv, mode)
    # the NaN pixels: confidence 0 (bin 0), counted in nonfinite and not in nll_fx, at every temperature.  Nearest: the one
    # pixel; bilinear: a zero-weight tap still carries its NaN, so the three pixels whose second taps read it as well
    k = 1 if mode == 1 else 4
    want = CR.sweep(nan.numpy(), geo, (T, T), lab.numpy(), C, inv.cpu().numpy(), -1, mode, np.float32)
    assert want["nonfinite"] == [k] * 3 and got["nonfinite"].tolist() == [k] * 3 and int(got["valid"]) == T * T
    assert (got["hist"][:, 0, 0] - base["hist"][:, 0, 0]).tolist() == [k] * 3
    for j in range(3):       # the other pixels' sum: the restatement's, within 4 ulp of an NLL below 8 per pixel (expf / logf)
        #                      and one unit of the fixed point where the two round to different sides
        assert abs(int(got["nll_fx"][j]) - want["nll_fx"][j]) <= (4 * 2.0 ** -21 * 65536 + 1) * (T * T)
        assert int(got["nll_fx"][j]) <= int(base["nll_fx"][j]) and int(got["hist"][j, :, 0].sum()) == T * T
    # exact ties give the first class: labels 0 everywhere, every pixel tied between classes 0 and 3 above the rest
    tie = slot.clone()
    tie[0] = 5.0; tie[3] = 5.0
    zero = torch.zeros((T, T), dtype=torch.int64)
    got = calib_temps(tie.cuda(), geo, (T, T), zero.cuda(), C, -1, inv, mode)
    assert got["hist"][:, :, 1].sum(1).tolist() == [T * T] * 3     # best == 0 == label at every pixel
    got = calib_temps(tie.cuda(), geo, (T, T), (zero + 3).cuda(), C, -1, inv, mode)
    assert got["hist"][:, :, 1].sum(1).tolist() == [0] * 3
    # one class: confidence 255 and NLL 0 everywhere
    one = calib_temps(fill((1, T, T), 12, -3, 3).cuda(), geo, (T, T), zero.cuda(), 1, -1, inv, mode)
    assert one["hist"][:, 255, 0].tolist() == [T * T] * 3 and one["hist"][:, 255, 1].tolist() == [T * T] * 3
    assert one["nll_fx"].tolist() == [0, 0, 0] and one["nonfinite"].tolist() == [0, 0, 0] and int(one["valid"]) == T * T


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------

def prepared_unet(seg, base, images):
    """seg.unet(3, 4) whose eval-mode argmax is not one class everywhere (as tests/test_gpu_tta.py prepares its models)"""
    from image_segmentation_amd.utils import process_batch_forward
    m = seg.unet(3, 4); fill_module(m, base); m.cuda()
    X, _ = process_batch_forward([im.cuda() for im in images], target_size=64, device="cuda")
    with torch.no_grad():
        m.train()
        for _ in range(20):
            m(X)
        m.eval()
        m.output.bias -= m(X).mean(dim=(0, 2, 3))
    return m


@pytest.fixture(scope="module")
def fp32(seg):
    seg.set_compute_dtype(torch.float32)
    yield
    seg.set_compute_dtype(torch.bfloat16)


class Scaled(torch.nn.Module):
    def __init__(self, model, inv):
        super().__init__()
        self.model, self.inv = model, inv
        self.output = model.output

    def forward(self, x):
        return self.model(x) * self.inv


E2E_SHAPES = [(37, 53), (64, 17), (50, 75)]


def test_end_to_end(seg, fp32):
    from image_segmentation_amd.utils import process_batch_forward, process_batch_reverse
    images = [fill((3,) + s, 70 + i, 0, 1).cuda() for i, s in enumerate(E2E_SHAPES)]
    m = prepared_unet(seg, 1000, images)
    # labels: the model's own argmax at the image's size with three pixels in ten redrawn, so that neither end of the
    # temperature grid is the obvious answer; 255 sprinkled in, class 3 named as ignore_index
    own = seg.Segmenter(m, target_size=64, palette=None)(images)
    labs = [torch.where(fill(s, 90 + i, 0, 1) < 0.3, labels(s, 80 + i, 4), p.mask.cpu().long()) for i, (s, p) in enumerate(zip(E2E_SHAPES, own))]
    labs[1][::3, ::4] = 255
    # a) the fitted grid argmin against the materialised route, float64 log-softmax on the host
    fit = seg.fit_temperature(m, images, labs, target_size=64, ignore_index=3, batch_size=2)
    temps = seg.default_temperatures()
    assert fit.temperatures == temps and len(fit.nll) == 17 and fit.nonfinite == [0] * 17
    X, metas = process_batch_forward(images, target_size=64, device="cuda")
    with torch.no_grad():
        full = process_batch_reverse(m(X), metas)
    z = np.concatenate([f.cpu().numpy().reshape(4, -1) for f in full], axis=1)
    l = np.concatenate([x.numpy().reshape(-1) for x in labs])
    ok = CR.valid_labels(l, 4, 3)
    z, l = z[:, ok], l[ok]
    assert fit.pixels == int(ok.sum())
    want, d = [], 0.0
    for it in CR.inverse_temperatures(temps):
        per = []
        for ft in (np.float64, np.float32):
            s = (z.astype(ft) * ft(it)).astype(ft)
            mx = s.max(0)
            per.append(np.log(np.exp(s - mx).sum(0, dtype=ft)).astype(ft) - (s[l, np.arange(l.size)] - mx))
        want.append(float(per[0].mean()))
        d = max(d, float(np.abs(per[1].astype(np.float64) - per[0]).max()))
    gate = 4 * d + 2.0 ** -17
    print(f"fit: T* = {fit.temperature:.4f} (grid {temps[fit.index]}), NLL {fit.nll_at_1:.5f} -> {fit.nll_best:.5f}, ECE {fit.ece_at_1:.4f} -> "
          f"{fit.ece_best:.4f}; max |nll - materialised| = {max(abs(a - b) for a, b in zip(fit.nll, want)):.3e} (gate {gate:.3e})")
    assert all(abs(a - b) <= gate for a, b in zip(fit.nll, want))
    order = np.argsort(want)
    assert fit.index == order[0] or (want[order[1]] - want[order[0]] < 2 * gate and fit.index == order[1])
    import json
    json.dumps(fit.to_json())
    # b) temperature=T is the model whose output is multiplied by the float32 1/T, bit for bit
    Tq = 1.7
    inv = float(np.float32(1.0 / Tq))
    for kw in (dict(), dict(tta=seg.TTA(flips=("", "h"))), dict(tiles=seg.Tiles(size=32, overlap=8))):
        a = seg.Segmenter(m, target_size=64, palette=PALETTE, return_scores=True, temperature=Tq, **kw)(images)
        b = seg.Segmenter(Scaled(m, inv), target_size=64, palette=PALETTE, return_scores=True, **kw)(images)
        c = seg.Segmenter(m, target_size=64, palette=PALETTE, return_scores=True, **kw)(images)
        for p, q in zip(a, b):
            assert torch.equal(p.mask, q.mask) and torch.equal(p.confidence, q.confidence) and torch.equal(p.scores, q.scores)
        assert any(not torch.equal(p.confidence, q.confidence) for p, q in zip(a, c))         # and it does something
    # c) temperature=None: today's outputs (the single-view path against the materialised argmax, merged views in bits)
    single = seg.Segmenter(m, target_size=64, palette=PALETTE, temperature=None)(images)
    for p, f in zip(single, full):
        assert p.confidence is None and torch.equal(p.mask.long(), f.argmax(0))
    cold = seg.predict(m, images, target_size=64, palette=PALETTE, temperature=Tq)            # predict() passes it through
    for p, q in zip(cold, seg.Segmenter(Scaled(m, inv), target_size=64, palette=PALETTE)(images)):
        assert p.confidence is None and torch.equal(p.mask, q.mask) and torch.equal(p.color, q.color)
    # d) reliability() over TTA and tiled predictions is the restatement on their own confidence and mask
    for kw in (dict(tta=seg.TTA(flips=("", "h"))), dict(tiles=seg.Tiles(size=32, overlap=8)), dict(tta=seg.TTA(), clean=dict(min_area=6))):
        preds = seg.Segmenter(m, target_size=64, palette=PALETTE, **kw)(images)
        rel = seg.reliability(preds, labs, 4, ignore_index=3)
        want = sum(CR.hist_reference(p.confidence.cpu().numpy(), (p.raw_mask if p.raw_mask is not None else p.mask).cpu().numpy(),
                                     lab.numpy(), 4, 3) for p, lab in zip(preds, labs))
        assert np.array_equal(rel.counts(), want)
        assert rel.ece() == pytest.approx(CR.ece(want.sum(0)), abs=1e-12) and rel.mce() == pytest.approx(CR.mce(want.sum(0)), abs=1e-12)
        again = seg.reliability(preds, labs, 4, ignore_index=3, out=rel)
        assert again is rel and np.array_equal(rel.counts(), 2 * want)
        json.dumps(rel.to_json())


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(seg):
    from image_segmentation_amd import _lib
    T, C = 16, 4
    slot = torch.zeros((C, T, T), device="cuda")
    lab = torch.zeros((8, 8), dtype=torch.int64, device="cuda")
    inv = torch.ones(32, device="cuda")
    out = torch.full((33 * 512 + 80,), 77, dtype=torch.int64, device="cuda")
    hist, nll, nonf, valid = out[:33 * 512], out[33 * 512:33 * 512 + 33], out[33 * 512 + 33:33 * 512 + 66], out[33 * 512 + 66:]

    def call(C=4, K=2, T=T, pt=0, pl=0, nh=16, nw=16, oh=8, ow=8, mode=0, slot=P(slot), lab=P(lab), inv=P(inv), ign=-1, hist=P(hist)):
        _lib.call("segk_calib_temps", slot, C, T, pt, pl, nh, nw, oh, ow, mode, lab, ign, inv, K, hist, P(nll), P(nonf), P(valid), stream())
    for kw, match in ((dict(K=0), "temperatures supported, got 0"), (dict(K=33), "temperatures supported, got 33"),
                      (dict(C=9), "classes supported, got 9"), (dict(C=0), "classes supported"), (dict(pt=1), "window outside the slot"),
                      (dict(nw=17), "window outside the slot"), (dict(pl=-1), "window outside the slot"), (dict(mode=2), "bad mode"),
                      (dict(slot=None), "NULL"), (dict(inv=None), "NULL"), (dict(lab=None), "NULL"), (dict(hist=None), "NULL"),
                      (dict(oh=0), "bad shape"), (dict(ign=-2), "ignore_index"), (dict(lab=P(lab) + 4), "8-byte aligned")):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    conf = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    for args, match in (((P(conf), P(conf), P(lab), 8, 8, 9, -1, P(hist)), "classes supported, got 9"),
                        ((None, P(conf), P(lab), 8, 8, 4, -1, P(hist)), "NULL"), ((P(conf), P(conf), P(lab), 0, 8, 4, -1, P(hist)), "image of")):
        with pytest.raises(RuntimeError, match=match):
            _lib.call("segk_calib_hist", *args, stream())
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                  # nothing was launched
    out.zero_()
    call()                                                          # and the well-formed call goes through
    torch.cuda.synchronize()
    assert int(valid[0]) == 64 and int(hist.sum()) == 2 * 64 * 2 and int(hist[255 * 2 + 1]) == 0 and int(nonf.sum()) == 0
    # the Python surface
    pred = seg.Prediction(torch.zeros((8, 8), dtype=torch.uint8, device="cuda"), None, torch.zeros(4), None, {})
    with pytest.raises(ValueError, match="tta=.*tiles=.*return_scores=True"):
        seg.reliability([pred], [lab], 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.fit_temperature(seg.unet(3, 4), [fill((3, 8, 8), 1, 0, 1)], [lab.cpu()], target_size=16)
    with pytest.raises(ValueError, match="temps"):
        seg.fit_temperature(seg.unet(3, 4).cuda(), [fill((3, 8, 8), 1, 0, 1)], [lab], target_size=16, temps=[1.0] * 33)
