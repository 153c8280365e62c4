"""GPU (-m gpu): tiled full-resolution prediction -- segk_tile_gather_u8 / segk_tile_gather,
segk_predict_tiles and Segmenter(tiles=...), against the NumPy restatement (tests/tiles_reference.py) on the shapes and
plans of tests/tiles_cases.py.

  1. gather: bit for bit, both pad modes, the whole plan in one call and split into tile ranges of 1 and of 3;
  2. blend without device transcendentals: Y holds NaN at every position no pixel maps to.  Probabilities under "prob":
     mask, scores and confidence bit-equal to the float32 restatement.  "logit" on logits: the mask bit-equal (the argmax of
     a = acc / Wtot).  With C = 1 the scores of a "logit" run are softmax over one class, 1.0 wherever a is finite: they are
     compared bit for bit too, which pins that a is finite (no NaN reached it), not its value -- with one class no output
     carries the value of a;
  3. blend with softmax ("prob" on logits, the scores of "logit") against float64.  Score gate: the device's distance is at
     most four times the float32 restatement's own distance (DESIGN.md 3.4's margin for the device expf against NumPy's).
     Mask gate: the mask differs from the float64 argmax only where the float64 top-two gap is below twice the measured
     score distance, and at most 1 pixel in 1000 lies there.  Confidence within +-1;
  4. counts, colour and M from the device mask itself, with and without labels, counts and colour;
  5. two runs are bit-identical; NaN and ties;
  6. Segmenter end to end against the materialised route: restatement gather -> the same model on the same tile batches ->
     restatement blend of the device outputs, under the gates of 2 and 3;
  7. refusals launch nothing."""
import functools

import numpy as np
import pytest
import torch

import tiles_cases as K
import tiles_reference as R
from oracle.fill import fill, labels, fill_module

pytestmark = pytest.mark.gpu

PALETTE = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (90, 160, 250)]
PADS = {"zero": 0, "reflect": 1}
WINDOWS = {"flat": 0, "triangle": 1}
MERGES = {"prob": 0, "logit": 1}


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


# ---- 1. gather ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def source_image(shape, channels, u8):
    if u8:
        return (fill(shape + (channels,), 20 + channels, 0, 1) * 255).round().byte().contiguous()
    return fill((channels,) + shape, 30 + channels, -2, 2).contiguous()


def device_gather(entry, img, c_arg, co, shape, T, o, pad, ranges):
    from image_segmentation_amd import _lib
    n = K.tile_count(shape, T, o)
    out = torch.full((n, co, T, T), 7.0, device="cuda")
    for t0, m in ranges:
        _lib.call(entry, P(img), P(out[t0:]), c_arg, shape[0], shape[1], T, o, PADS[pad], t0, m, stream())
    return out


@pytest.mark.parametrize("pad", ["zero", "reflect"])
@pytest.mark.parametrize("kind,channels", [("u8", 1), ("u8", 3), ("u8", 4), ("float", 1), ("float", 3)])
def test_gather_equals_the_restatement_bit_for_bit(seg, kind, channels, pad):
    entry = "segk_tile_gather_u8" if kind == "u8" else "segk_tile_gather"
    co = min(channels, 3)
    for _, shape, T, o in K.plans():
        img = source_image(shape, channels, kind == "u8")
        want = torch.from_numpy(R.gather(img.numpy(), T, o, pad)).cuda()
        dev = img.cuda()
        n = K.tile_count(shape, T, o)
        assert want.shape == (n, co, T, T)
        for step in (n, 1, 3):
            ranges = [(t0, min(step, n - t0)) for t0 in range(0, n, step)]
            got = device_gather(entry, dev, channels, co, shape, T, o, pad, ranges)
            assert torch.equal(got, want), (shape, T, o, step, int((got != want).sum()))
    # an output that is only 4-byte aligned takes the scalar stores: the same bits
    shape, T, o = (40, 56), 32, 8
    img = source_image(shape, channels, kind == "u8")
    n = K.tile_count(shape, T, o)
    buf = torch.full((n * co * T * T + 1,), 7.0, device="cuda")
    from image_segmentation_amd import _lib
    _lib.call(entry, P(img.cuda()), P(buf[1:]), channels, *shape, T, o, PADS[pad], 0, n, stream())
    assert torch.equal(buf[1:].view(n, co, T, T), torch.from_numpy(R.gather(img.numpy(), T, o, pad)).cuda()) and float(buf[0]) == 7.0


# ---- 2. / 3. blend -----------------------------------------------------------------------------------------------------------

def blend(Y, shape, T, o, window, merge, kind, palette=None, labs=None, want_counts=True, want_scores=True, want_conf=True):
    """segk_predict_tiles on Y [n,C,T,T] (a CUDA tensor) -> dict(mask, color, counts, M, conf, scores)"""
    from image_segmentation_amd import _lib
    H, W = shape
    C = int(Y.shape[1])
    assert Y.shape[0] == K.tile_count(shape, T, o) and Y.is_contiguous()
    out = dict(mask=torch.full((H, W), 77, dtype=torch.uint8, device="cuda"),
               color=torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda") if palette is not None else None,
               counts=torch.zeros(8, dtype=torch.int64, device="cuda") if want_counts else None,
               M=torch.zeros((8, 8), dtype=torch.int64, device="cuda") if labs is not None else None,
               conf=torch.full((H, W), 77, dtype=torch.uint8, device="cuda") if want_conf else None,
               scores=torch.full((C, H, W), 77.0, device="cuda") if want_scores else None)
    _lib.call("segk_predict_tiles", P(Y), C, kind, MERGES[merge], WINDOWS[window], H, W, T, o, P(out["mask"]), P(out["color"]),
              P(palette), P(out["counts"]), P(labs), P(out["M"]), P(out["conf"]), P(out["scores"]), stream())
    torch.cuda.synchronize()
    if want_counts:
        out["counts"] = out["counts"][:C]
    if labs is not None:
        out["M"] = out["M"][:C, :C]
    return out


def same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8))


@pytest.mark.parametrize("window", ["triangle", "flat"])
@pytest.mark.parametrize("C", K.CLASSES)
def test_blend_exact_cases(seg, C, window):
    for i, shape, T, o in K.plans():
        case = dict(shape=shape, T=T, o=o, C=C, seed=300 + i)
        # probabilities under "prob": no transcendental on the device
        Yp = K.poison(K.probabilities(case), case)
        out = blend(torch.from_numpy(Yp).cuda(), shape, T, o, window, "prob", 1)
        mask, conf, scores, _ = R.blend(Yp, *shape, T, o, window, "prob", 1, np.float32)
        assert same_bits(out["mask"], mask), (shape, T, o, int((out["mask"].cpu().numpy() != mask).sum()))
        assert same_bits(out["scores"], scores), (shape, T, o, float(np.abs(out["scores"].cpu().numpy() - scores).max()))
        assert same_bits(out["conf"], conf), (shape, T, o)
        # "logit" on logits: the argmax of a = acc / Wtot
        Yl = K.poison(K.logits(case), case)
        out = blend(torch.from_numpy(Yl).cuda(), shape, T, o, window, "logit", 0)
        mask, conf, scores, a = R.blend(Yl, *shape, T, o, window, "logit", 0, np.float32)
        assert not np.isnan(a).any()
        assert same_bits(out["mask"], mask), (shape, T, o, int((out["mask"].cpu().numpy() != mask).sum()))
        if C == 1:
            assert same_bits(out["scores"], scores) and same_bits(out["conf"], conf) and bool((out["conf"] == 255).all())


def check_against_float64(results, C_of):
    """results: [(device output dict, (mask, conf, scores) in float64, scores of the float32 restatement, C)].  The gates of the
    module docstring over the whole list; returns (device distance, yardstick)."""
    d = max(float(np.abs(o["scores"].cpu().numpy().astype(np.float64) - s64).max()) for o, (_, _, s64), _ in results)
    yard = max(float(np.abs(s32.astype(np.float64) - s64).max()) for _, (_, _, s64), s32 in results)
    close = allowed = total = 0
    worst_conf = 0
    for o, (m64, c64, s64), _ in results:
        differs = o["mask"].cpu().numpy() != m64
        if s64.shape[0] > 1:
            top = np.sort(s64, axis=0)[-2:]
            near_tie = (top[1] - top[0]) < 2 * d
            assert not (differs & ~near_tie).any(), int((differs & ~near_tie).sum())
            allowed += int(near_tie.sum())
        close += int(differs.sum()); total += differs.size
        worst_conf = max(worst_conf, int(np.abs(o["conf"].cpu().numpy().astype(int) - c64.astype(int)).max()))
    print(f"{C_of}: d = max|device scores - float64| = {d:.3e}, yardstick (float32 restatement) = {yard:.3e}, ratio {d / yard:.2f}; "
          f"{allowed} of {total} pixels inside the 2d gap, {close} differ from the float64 argmax; confidence off by at most {worst_conf}")
    assert d <= 4 * yard
    assert close <= allowed and allowed * 1000 <= total
    assert worst_conf <= 1
    return d, yard


@pytest.mark.parametrize("merge", ["prob", "logit"])
def test_blend_with_softmax_against_float64(seg, merge):
    results = []
    for case in K.softmax_cases():
        Y = K.poison(K.logits(case), case)
        args = (Y, *case["shape"], case["T"], case["o"], case["window"], merge, 0)
        out = blend(torch.from_numpy(Y).cuda(), case["shape"], case["T"], case["o"], case["window"], merge, 0)
        m64, c64, s64, _ = R.blend(*args, np.float64)
        _, _, s32, _ = R.blend(*args, np.float32)
        assert not np.isnan(out["scores"].cpu().numpy()).any()
        results.append((out, (m64, c64, s64), s32))
    check_against_float64(results, f"segk_predict_tiles {merge}")


# ---- 4. counts, colour, M ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_labels", [False, True])
@pytest.mark.parametrize("with_counts", [False, True])
@pytest.mark.parametrize("with_color", [False, True])
def test_counts_colour_and_confusion_come_from_the_device_mask(seg, with_color, with_counts, with_labels):
    from image_segmentation_amd import ops
    pal = torch.tensor(PALETTE, dtype=torch.uint8, device="cuda")
    for case in K.softmax_cases()[::3]:
        shape, T, o, C = case["shape"], case["T"], case["o"], case["C"]
        Y = torch.from_numpy(K.poison(K.logits(case), case)).cuda()
        lab = labels(shape, 40 + case["seed"], C + 1)                 # class C is outside [0, C): skipped
        lab[::3, ::2] = 255
        lab[0, 0] = -1
        lab = lab.cuda()
        plain = blend(Y, shape, T, o, case["window"], "prob", 0)
        out = blend(Y, shape, T, o, case["window"], "prob", 0, pal if with_color else None, lab if with_labels else None,
                    want_counts=with_counts, want_scores=False, want_conf=False)
        mask = out["mask"]
        assert torch.equal(mask, plain["mask"]) and int(mask.max()) < C
        if with_counts:
            assert torch.equal(out["counts"], torch.bincount(mask.flatten().long(), minlength=C))
        if with_color:
            assert torch.equal(out["color"], pal[mask.long()])
        if with_labels:
            keep = (lab >= 0) & (lab < C)
            want = torch.zeros((C, C), dtype=torch.int64, device="cuda")
            want.view(-1).index_add_(0, (mask.long() * C + lab.clamp(0, C - 1))[keep], torch.ones_like(lab[keep]))
            assert torch.equal(out["M"], want) and int(want.sum()) == int(keep.sum())
            onehot = torch.nn.functional.one_hot(mask.long(), C).permute(2, 0, 1).float().contiguous()
            folded = torch.where(keep, lab, torch.full_like(lab, 255))
            assert torch.equal(out["M"], ops.confusion_matrix(onehot, folded, C))


# ---- 5. stability, NaN and ties ------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_identical(seg):
    pal = torch.tensor(PALETTE, dtype=torch.uint8, device="cuda")
    for merge in ("prob", "logit"):
        case = dict(shape=(97, 50), T=32, o=16, C=4, seed=900)
        Y = torch.from_numpy(K.logits(case)).cuda()
        lab = labels(case["shape"], 41, 4).cuda()
        a = blend(Y, case["shape"], 32, 16, "triangle", merge, 0, pal, lab)
        b = blend(Y, case["shape"], 32, 16, "triangle", merge, 0, pal, lab)
        for k in a:
            assert torch.equal(a[k].view(torch.uint8) if a[k].dtype == torch.float32 else a[k],
                               b[k].view(torch.uint8) if b[k].dtype == torch.float32 else b[k]), k


def test_nan_and_ties(seg):
    shape, T, o, C = (40, 56), 32, 8, 4
    ys, xs = R.tile_axis(40, T, o), R.tile_axis(56, T, o)
    Y = np.zeros((4, C, T, T), np.float32)

    def put(k, y, x, v, tiles=None):
        """write v into class k at image pixel (y, x) in every tile that covers it (or in `tiles` alone)"""
        for iy, y0 in enumerate(ys):
            for ix, x0 in enumerate(xs):
                t = iy * len(xs) + ix
                if y0 <= y < y0 + T and x0 <= x < x0 + T and (tiles is None or t in tiles):
                    Y[t, k, y - y0, x - x0] = v
    put(2, 3, 4, np.nan)                    # one tile covers (3, 4)
    put(2, 20, 28, np.nan, tiles=[3])       # four tiles cover (20, 28): the NaN sits in the last of them alone
    put(1, 30, 30, 2.0); put(3, 30, 30, 2.0)        # a tie of classes 1 and 3 in every covering tile
    dev = torch.from_numpy(Y).cuda()
    for window in ("flat", "triangle"):
        # a NaN logit under "logit" makes its class win; the confidence of a NaN is 0; ties go to the first class
        out = blend(dev, shape, T, o, window, "logit", 0)
        m, cf = out["mask"], out["conf"]
        assert (int(m[3, 4]), int(m[20, 28]), int(m[30, 30]), int(m[0, 0]), int(m[39, 55])) == (2, 2, 1, 0, 0)
        assert int(cf[3, 4]) == 0 and int(cf[20, 28]) == 0
        want = R.blend(Y, *shape, T, o, window, "logit", 0, np.float32)
        assert same_bits(m, want[0])
        # NaN in probabilities: its class wins as well
        out = blend(dev, shape, T, o, window, "prob", 1)
        assert (int(out["mask"][3, 4]), int(out["mask"][20, 28]), int(out["mask"][30, 30])) == (2, 2, 1)
        assert same_bits(out["mask"], R.blend(Y, *shape, T, o, window, "prob", 1, np.float32)[0])
        # a NaN logit under "prob" poisons the softmax of its tile: every class is NaN there, so class 0
        out = blend(dev, shape, T, o, window, "prob", 0)
        assert (int(out["mask"][3, 4]), int(out["mask"][20, 28]), int(out["mask"][30, 30])) == (0, 0, 1)
        assert int(out["conf"][3, 4]) == 0


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------

E2E_SHAPES = [(40, 56), (33, 70), (16, 16)]


@pytest.fixture(scope="module")
def fp32(seg):
    seg.set_compute_dtype(torch.float32)
    yield
    seg.set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope="module")
def net(seg, fp32):
    """seg.unet(3, 3) filled by fill_module; BatchNorm buffers settled on tiles of the test images and the head bias centred,
    so that the eval-mode argmax is not one class everywhere"""
    m = seg.unet(3, 3); fill_module(m, 4000); m.cuda()
    X = torch.cat([torch.from_numpy(R.gather(fill((3,) + s, 70 + i, 0, 1).numpy(), 32, 8, "reflect")) for i, s in enumerate(E2E_SHAPES)]).cuda()
    with torch.no_grad():
        m.train()
        for _ in range(20):
            m(X)
        m.eval()
        m.output.bias -= m(X).mean(dim=(0, 2, 3))
    return m


def batches_of(counts, batch_size):
    """the forwards Segmenter runs: [[(image, tile0, m)]] (filled across consecutive images, at least one; an
    image with more tiles alone in ceil(n / batch_size) forwards)"""
    out, i = [], 0
    while i < len(counts):
        j, total = i + 1, counts[i]
        while j < len(counts) and total + counts[j] <= batch_size:
            total += counts[j]; j += 1
        if j == i + 1 and counts[i] > batch_size:
            out += [[(i, t0, min(batch_size, counts[i] - t0))] for t0 in range(0, counts[i], batch_size)]
        else:
            out.append([(k, 0, counts[k]) for k in range(i, j)])
        i = j
    return out


def materialised(model, tiles, batch_size, extra=None):
    """tiles: per image the restatement's gathered tiles [n,c,T,T]; -> per image the device outputs Y [n,C,T,T] as NumPy"""
    counts = [len(t) for t in tiles]
    Ys = [[] for _ in tiles]
    with torch.no_grad():
        for batch in batches_of(counts, batch_size):
            X = torch.from_numpy(np.concatenate([tiles[k][t0:t0 + m] for k, t0, m in batch])).cuda()
            if extra is None:
                y = model(X)
            else:
                y = model(X, torch.from_numpy(np.concatenate([extra[k][t0:t0 + m] for k, t0, m in batch])).cuda())
            off = 0
            for k, t0, m in batch:
                Ys[k].append(y[off:off + m].float().cpu().numpy()); off += m
    return [np.concatenate(y) for y in Ys]


def test_batches_of_restates_the_batching():
    assert batches_of([4, 6, 1], 32) == [[(0, 0, 4), (1, 0, 6), (2, 0, 1)]]
    assert batches_of([4, 6, 1], 2) == [[(0, 0, 2)], [(0, 2, 2)], [(1, 0, 2)], [(1, 2, 2)], [(1, 4, 2)], [(2, 0, 1)]]
    assert batches_of([4, 6, 1], 7) == [[(0, 0, 4)], [(1, 0, 6), (2, 0, 1)]]


@pytest.mark.parametrize("batch_size", [2, 32])
@pytest.mark.parametrize("as_u8", [False, True])
def test_segmenter_tiles_end_to_end(seg, net, as_u8, batch_size):
    T, o = 32, 8
    floats = [fill((3,) + s, 70 + i, 0, 1) for i, s in enumerate(E2E_SHAPES)]
    images = [(im * 255).round().byte().permute(1, 2, 0).contiguous() for im in floats] if as_u8 else floats
    tiles = [R.gather(im.numpy(), T, o, "reflect") for im in images]
    assert [len(t) for t in tiles] == [4, 6, 1]
    Ys = materialised(net, tiles, batch_size)
    s = seg.Segmenter(net, target_size=T, tiles=seg.Tiles(), palette=PALETTE[:3], batch_size=batch_size, return_scores=True)
    preds = s(images)
    results = []
    for p, Y, shape in zip(preds, Ys, E2E_SHAPES):
        assert p.meta == {"original_size": shape, "tile_size": T, "overlap": o, "tiles": (len(R.tile_axis(shape[0], T, o)),
                                                                                       len(R.tile_axis(shape[1], T, o)))}
        assert p.mask.is_cuda and p.mask.dtype == torch.uint8 and tuple(p.mask.shape) == shape
        assert p.confidence.dtype == torch.uint8 and tuple(p.confidence.shape) == shape and tuple(p.scores.shape) == (3,) + shape
        assert p.confusion is None and p.raw_mask is None
        assert torch.equal(p.counts, torch.bincount(p.mask.flatten().long(), minlength=3))
        assert torch.equal(p.color, torch.tensor(PALETTE[:3], dtype=torch.uint8, device="cuda")[p.mask.long()])
        m64, c64, s64, _ = R.blend(Y, *shape, T, o, "triangle", "prob", 0, np.float64)
        _, _, s32, _ = R.blend(Y, *shape, T, o, "triangle", "prob", 0, np.float32)
        results.append((dict(mask=p.mask, conf=p.confidence, scores=p.scores), (m64, c64, s64), s32))
    check_against_float64(results, f"Segmenter(tiles) u8={as_u8} batch_size={batch_size}")
    hist = torch.bincount(torch.cat([p.mask.flatten() for p in preds]).long(), minlength=3)
    assert int((hist > 0).sum()) >= 2                              # not one class everywhere: the masks say something
    # "logit" merging and the flat window: the mask is the float32 restatement's, bit for bit (the gate of test 2)
    for p, Y, shape in zip(seg.predict(net, images, target_size=T, tiles=dict(merge="logit", window="flat"), batch_size=batch_size), Ys,
                           E2E_SHAPES):
        assert same_bits(p.mask, R.blend(Y, *shape, T, o, "flat", "logit", 0, np.float32)[0]) and p.scores is None
        assert p.confidence is not None
    # labels, clean= and return_scores= together
    from image_segmentation_amd import ops
    labs = [labels(sh, 80 + i, 3) for i, sh in enumerate(E2E_SHAPES)]
    labs[0][::3, ::4] = 255
    cleaned = seg.Segmenter(net, target_size=T, tiles=seg.Tiles(), palette=PALETTE[:3], batch_size=batch_size, return_scores=True,
                            clean=dict(min_area=4))(images, labels=labs)
    pal = torch.tensor(PALETTE[:3], dtype=torch.uint8, device="cuda")
    for c, p, lab in zip(cleaned, preds, labs):
        assert torch.equal(c.raw_mask, p.mask) and torch.equal(c.confidence, p.confidence) and torch.equal(c.scores, p.scores)
        assert torch.equal(c.mask, seg.components(p.mask, min_area=4).mask) and c.components is not None
        assert torch.equal(c.color, pal[c.mask.long()])
        assert torch.equal(c.counts, torch.bincount(c.mask.flatten().long(), minlength=3))
        onehot = torch.nn.functional.one_hot(c.mask.long(), 3).permute(2, 0, 1).float().contiguous()
        assert torch.equal(c.confusion, ops.confusion_matrix(onehot, lab.cuda(), 3))
    for q, p, lab in zip(s(images, labels=labs), preds, labs):       # without clean=: the confusion counts of the same pass
        onehot = torch.nn.functional.one_hot(p.mask.long(), 3).permute(2, 0, 1).float().contiguous()
        assert torch.equal(q.mask, p.mask) and torch.equal(q.confusion, ops.confusion_matrix(onehot, lab.cuda(), 3))


class TwoInputToy(torch.nn.Module):
    """forward(image, heatmap) -> 3 logits per pixel, element-wise: any batch gives the same bits per tile"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([1.5, -2.0, 0.75]))
        self.v = torch.nn.Parameter(torch.tensor([-1.0, 2.5, 0.5]))

    def forward(self, x, h):
        return (x - 0.5) * self.w.view(1, 3, 1, 1) + h * self.v.view(1, 3, 1, 1)


@pytest.mark.parametrize("batch_size", [2, 32])
def test_segmenter_tiles_two_input_model_with_points(seg, batch_size):
    T, o = 32, 8
    toy = TwoInputToy().cuda()
    images = [fill((3,) + s, 70 + i, 0, 1) for i, s in enumerate(E2E_SHAPES)]
    points = [[(sh[0] // 4, sh[1] // 5), (sh[0] - 1, sh[1] - 1)] for sh in E2E_SHAPES]
    heat = [seg.point_heatmap(p, sh[0], sh[1], device="cuda") for p, sh in zip(points, E2E_SHAPES)]
    s = seg.Segmenter(toy, target_size=T, tiles=seg.Tiles(pad="zero"), palette=PALETTE[:3], batch_size=batch_size, return_scores=True)
    preds = s(images, points=points)
    tiles = [R.gather(im.numpy(), T, o, "zero") for im in images]
    htiles = [R.gather(h.cpu().numpy(), T, o, "zero") for h in heat]       # the heat-map takes its image's plan and pad mode
    Ys = materialised(toy, tiles, batch_size, htiles)
    results = []
    for p, Y, shape in zip(preds, Ys, E2E_SHAPES):
        m64, c64, s64, _ = R.blend(Y, *shape, T, o, "triangle", "prob", 0, np.float64)
        _, _, s32, _ = R.blend(Y, *shape, T, o, "triangle", "prob", 0, np.float32)
        results.append((dict(mask=p.mask, conf=p.confidence, scores=p.scores), (m64, c64, s64), s32))
    check_against_float64(results, f"two-input toy, points, batch_size={batch_size}")
    for a, b in zip(s(images, heatmaps=heat), preds):                  # the same heat-maps handed over as such
        assert torch.equal(a.mask, b.mask) and torch.equal(a.scores, b.scores)
    assert any(float(h.max()) > 0 for h in heat)
    with pytest.raises(ValueError, match="heatmap 0"):
        s(images[:1], heatmaps=[heat[1]])
    with pytest.raises(ValueError, match="heatmaps= or points="):
        s(images)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(seg):
    from image_segmentation_amd import _lib
    C, T, o, H, W = 4, 16, 4, 20, 30
    n = K.tile_count((H, W), T, o)
    Y = torch.zeros((n, C, T, T), device="cuda")
    b = torch.full((4096,), 77, dtype=torch.uint8, device="cuda")
    sc = torch.full((C * H * W,), 77.0, device="cuda")
    img = torch.zeros((3, H, W), device="cuda")
    u8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    tl = torch.full((n, 3, T, T), 77.0, device="cuda")

    def call(Y=P(Y), C=4, kind=0, merge=0, window=1, H=H, W=W, T=T, o=o, mask=P(b), color=None, palette=None, labs=None, M=None, conf=None,
             scores=None):
        _lib.call("segk_predict_tiles", Y, C, kind, merge, window, H, W, T, o, mask, color, palette, None, labs, M, conf, scores, stream())
    for kw, match in ((dict(merge=2), "bad merge"), (dict(merge=-1), "bad merge"), (dict(kind=2), "kind"), (dict(merge=1, kind=1), "needs logits"),
                      (dict(window=2), "bad window"), (dict(C=9), "classes supported, got 9"), (dict(C=0), "classes supported"),
                      (dict(T=0), "tile side"), (dict(T=4097), "tile side"), (dict(o=9), "overlap"), (dict(o=-1), "overlap"),
                      (dict(H=0), "sides positive"), (dict(W=-1), "sides positive"), (dict(H=1 << 16, W=1 << 15), "sides positive"),
                      (dict(mask=P(b) + 1), "4-byte aligned"), (dict(conf=P(b) + 2050), "4-byte aligned"),
                      (dict(scores=P(sc) + 2), "4-byte aligned"), (dict(Y=P(Y) + 2), "4-byte aligned"),
                      (dict(color=P(b) + 1024), "color and palette come together"), (dict(labs=P(sc)), "labels and M come together"),
                      (dict(mask=None), "NULL"), (dict(Y=None), "NULL"), (dict(H=20000, W=20000, T=256, o=0, C=8), "32-bit offsets")):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)

    def gather(entry="segk_tile_gather", src=P(img), out=P(tl), c=3, H=H, W=W, T=T, o=o, pad=1, tile0=0, m=n):
        _lib.call(entry, src, out, c, H, W, T, o, pad, tile0, m, stream())
    for entry, src, c in (("segk_tile_gather", P(img), 3), ("segk_tile_gather_u8", P(u8), 4)):
        for kw, match in ((dict(src=None), "NULL"), (dict(out=None), "NULL"), (dict(T=0), "tile side"), (dict(o=9), "overlap"),
                          (dict(pad=2), "pad mode"), (dict(tile0=-1), "of a plan of"), (dict(m=0), "of a plan of"),
                          (dict(m=n + 1), "of a plan of"), (dict(tile0=n, m=1), "of a plan of"), (dict(out=P(tl) + 2), "aligned"),
                          (dict(H=0), "sides positive"), (dict(c=0), "channels"), (dict(src=src + 2), "aligned")):
            with pytest.raises(RuntimeError, match=match):
                gather(**dict(dict(entry=entry, src=src, c=c), **kw))
    with pytest.raises(RuntimeError, match="1, 3 or 4"):
        gather(entry="segk_tile_gather_u8", src=P(u8), c=2)
    torch.cuda.synchronize()
    assert bool((b == 77).all()) and bool((sc == 77).all()) and bool((tl == 77).all())      # nothing was launched
    call(conf=P(b) + 2048, scores=P(sc))                          # and the well-formed calls go through
    gather()
    torch.cuda.synchronize()
    assert bool((b[:H * W] == 0).all()) and bool((sc == 0.25).all()) and bool((b[2048:2048 + H * W] == 64).all())
    assert bool((tl == 0).all())
    # the Python surface refuses before anything is launched
    m = seg.unet(3, 4).cuda()
    with pytest.raises(ValueError, match="does not combine"):
        seg.Segmenter(m, target_size=32, tiles=seg.Tiles(), tta=seg.TTA())
    with pytest.raises(ValueError, match="multiple of 16"):
        seg.predict(m, [img], target_size=40, tiles=seg.Tiles())
    with pytest.raises(ValueError, match="8-bit inputs"):
        seg.Segmenter(m, target_size=32, tiles=seg.Tiles())([torch.zeros((8, 8, 2), dtype=torch.uint8, device="cuda")])
