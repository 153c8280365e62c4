"""GPU (-m gpu): what the loops of training.py launch on the real HIP modules, as a record -- the four train loops and the three
evaluation loops at B = 2, 32 x 32 (three ragged images for the evaluation loops), compared with
tests/golden/training_trace_gpu.json (stored in the packed form of tests/trace_fixture.py).  The host side of the same loops
(call order on fakes, grad mode, bars, printed text) is tests/test_training_trace_host.py; this file covers what a CPU cannot
reach: the `loss.is_cuda` branch of the evaluation loops with `accumulate_deferred`, and the kernels the loops launch.

Per case the record holds
  * the launch trace: every _lib.call in order, as [entry, args...]; an argument whose argtype in _lib.SIGNATURES is
    c_void_p is recorded only as "ptr" / "null" (None or 0), every other argument as its value -- no address is recorded;
  * the returned numbers as float.hex.

The fixture is a record of the commit BEFORE the loops were folded onto one accumulation window and one evaluation pass
(DESIGN.md 3.9).  Every case builds fresh models (oracle.fill weights) and a fresh optimizer, sets the compute dtype and
starts from ops.invalidate_packed_weights(), so the record does not depend on what ran earlier in the process: the file gives
the same record alone and after tests/test_gpu_modules.py in one pytest process, with every entry's arguments kept.

Set SEGK_TRAINING_TRACE_GPU_OUT=<file> to write the record there instead of comparing."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import trace_fixture
from oracle.fill import fill, labels, fill_module

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "training_trace_gpu.json")
OUT = os.environ.get("SEGK_TRAINING_TRACE_GPU_OUT")
CW4 = [0.25, 1.0, 1.25, 0.5]
RAGGED = [(24, 32), (32, 20), (32, 32)]

_RECORD = {}


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import image_segmentation_amd as s
    from image_segmentation_amd import _lib
    _lib.load()
    yield s
    s.set_compute_dtype(torch.bfloat16)
    if OUT and _RECORD:
        trace_fixture.dump(OUT, _RECORD, "calls")


@pytest.fixture
def trace(seg, monkeypatch):
    from image_segmentation_amd import _lib, ops, training
    calls, real = [], _lib.call

    def call(name, *args):
        types = _lib.SIGNATURES[name][1]
        assert len(types) == len(args), name
        row = [name]
        for t, a in zip(types, args):
            if t is ctypes.c_void_p:
                row.append("null" if a is None or a == 0 else "ptr")
            else:
                row.append(float(a) if isinstance(a, (float, np.floating)) else int(a))
        calls.append(row)
        return real(name, *args)

    monkeypatch.setattr(training, "VERBOSE", False)
    seg.set_compute_dtype(torch.bfloat16)
    ops.invalidate_packed_weights()
    monkeypatch.setattr(_lib, "call", call)
    return calls


def check(name, calls, ret):
    vals = ret if isinstance(ret, tuple) else (ret,)
    got = json.loads(json.dumps({"calls": calls, "result": [float(v).hex() for v in vals]}))
    if OUT:
        _RECORD[name] = got
        return
    want = trace_fixture.load(GOLDEN, "calls")[name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]], "the launch order changed"
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"launch {k}"
    assert got["result"] == want["result"]


def filled(m, base):
    fill_module(m, base)
    return m.cuda()


def stacked(k, heat=False, n_classes=3):
    X, y = fill((2, 3, 32, 32), 10 + k, 0, 1), labels((2, 1, 32, 32), 20 + k, n_classes)
    return (X, fill((2, 1, 32, 32), 30 + k, 0, 1), y) if heat else (X, y)


def ragged(k, sizes, heat=False, n_classes=3):
    X = [fill((3, H, W), 40 + k + i, 0, 1) for i, (H, W) in enumerate(sizes)]
    y = [labels((1, H, W), 50 + k + i, n_classes) for i, (H, W) in enumerate(sizes)]
    return (X, [fill((1, H, W), 60 + k + i, 0, 1) for i, (H, W) in enumerate(sizes)], y) if heat else (X, y)


def prompt_model(seg):
    m = seg.PromptModel(clip=filled(seg.unet(3, 4), 9000))
    fill_module(m.mask, 9500)
    return m.cuda().train()


def prompt_loss(seg, **kw):
    return seg.WeightedDiceNLLLoss(ignore_index=3, class_weights=torch.tensor(CW4), apply_softmax=False,
                                   nll_nonlin=lambda t: torch.log(t + 1e-9), **kw)


@pytest.mark.parametrize("form", ["stacked", "ragged"])
def test_train_loop(seg, trace, form):
    from image_segmentation_amd import training
    m = filled(seg.unet(3, 3), 1000)
    opt = torch.optim.AdamW(m.parameters(), weight_decay=0.01)
    data = [stacked(k) if form == "stacked" else ragged(3 * k, RAGGED[:2]) for k in range(3)]
    avg = training.train_loop(data, m, seg.CrossEntropyLoss(), opt, 2, torch.device("cuda"),
                              target_size=None if form == "stacked" else 32)
    assert np.isfinite(avg) and avg > 0
    check(f"train_loop/{form}", trace, avg)


def test_train_loop_prompt(seg, trace):
    from image_segmentation_amd import training
    m = prompt_model(seg)
    opt = torch.optim.AdamW(m.mask.parameters(), weight_decay=0.01)
    avg = training.train_loop_prompt([stacked(k, heat=True, n_classes=4) for k in range(3)], m, prompt_loss(seg, smooth_dice=1), opt, 2,
                                     torch.device("cuda"))
    assert np.isfinite(avg)
    check("train_loop_prompt", trace, avg)


@pytest.mark.parametrize("with_labels", [True, False])
def test_train_loop_distill(seg, trace, with_labels):
    student = filled(seg.unet(3, 3), 1000)
    teacher = seg.Teacher([filled(seg.unet(3, 3), 2000)])
    opt = torch.optim.AdamW(student.parameters(), weight_decay=0.01)
    if with_labels:
        data = [stacked(k) for k in range(3)]
        loss_fn = seg.DistillLoss(hard=seg.CrossEntropyLoss(), alpha=0.5, temperature=2.0)
    else:
        data = [(stacked(0)[0], None), stacked(1)[0], (stacked(2)[0], None)]
        loss_fn = seg.DistillLoss(alpha=1.0, temperature=2.0)
    avg = seg.train_loop_distill(data, student, teacher, loss_fn, opt, 2, "cuda")
    assert np.isfinite(avg) and avg > 0
    check(f"train_loop_distill/{'labels' if with_labels else 'no_labels'}", trace, avg)


def test_train_reconstruction(seg, trace):
    from image_segmentation_amd import training
    m = filled(seg.ReconstructionAutoencoder(3, 3, base_channels=32), 4100)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    mean = training.trainReconstruction([(stacked(k)[0], None) for k in range(3)], m, seg.MSELoss(), opt, 2)
    assert isinstance(mean, np.float64) and np.isfinite(mean)
    check("trainReconstruction", trace, mean)


def test_eval_loop(seg, trace):
    from image_segmentation_amd import training
    m = filled(seg.unet(3, 3), 1000).train()
    agg = training.MetricsHistory(3)
    ret = training.eval_loop([ragged(0, RAGGED[:2]), ragged(5, RAGGED[2:])], m, seg.CrossEntropyLoss(), torch.device("cuda"), 32, agg)
    assert not m.training and agg._dev_M is not None and float(agg.total_tp.sum() + agg.total_fn.sum()) == 24 * 32 + 32 * 20 + 32 * 32
    check("eval_loop", trace, ret)


def test_eval_loop_prompt(seg, trace):
    from image_segmentation_amd import training
    m = prompt_model(seg)
    agg = training.MetricsHistory(4, ignore_index=3)
    data = [ragged(0, RAGGED[:2], heat=True), ragged(5, RAGGED[2:], heat=True)]
    ret = training.eval_loop_prompt(data, m, prompt_loss(seg), torch.device("cuda"), 32, agg)
    assert not m.training and agg._dev_M is not None
    check("eval_loop_prompt", trace, ret)


def test_eval_reconstruction(seg, trace):
    from image_segmentation_amd import training
    m = filled(seg.ReconstructionAutoencoder(3, 3, base_channels=32), 4200).train()
    imgs = [fill((3, 24, 32), 61, 0, 1), fill((4, 32, 20), 62, 0, 1), fill((3, 32, 32), 63, 0, 1)]
    ret = training.evalReconstruction([([imgs[0], imgs[1]], None), ([imgs[2]], None)], m, seg.MSELoss(), 32)
    assert not m.training and np.isfinite(ret[0]) and isinstance(ret[1], np.float64)
    check("evalReconstruction", trace, ret)


def test_clip_decoder_steps(seg, trace):
    """Two steps of forward, CrossEntropyLoss, backward and AdamW(fused=True) on the CLIP decoder, wrapped as in
    tests/test_gpu_clip.py::test_clip_decoder_one_launch_repack_after_optimizer_step: the backward of Conv1x1Fn, of the
    stand-alone ConvT2x2Fn and of BilinearFn, and in the second forward the one-launch repack with its kind 2 and 3 entries
    (segk_pack_multi with its n and total_blocks).  This case of the fixture is a record of the commit BEFORE the fused-op
    host layer was folded onto one operand path and one packed-weight record."""
    from image_segmentation_amd import ops
    dec = seg.UNetDecoder(64, [64, 32, 32, 32, 32]); head = torch.nn.Conv2d(32, 4, 1)

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.decoder, self.output_layer = dec, head

        def forward(self, x, skips):
            ops.repack_stale(self)
            return self.decoder(x, skips, head=self.output_layer)
    m = Wrap(); fill_module(m, 4100); m.cuda().train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2, fused=True)
    x = fill((2, 64, 4, 4), 11, -1, 1).cuda()
    skips = [fill((2, 64, 4, 4), 20 + i, -1, 1).cuda() for i in range(4)]
    Y = labels((2, 64, 64), 3, 4).cuda()
    loss_fn, losses = seg.CrossEntropyLoss(), []
    for _ in range(2):
        loss = loss_fn(m(x, skips), Y)
        loss.backward(); opt.step(); opt.zero_grad(set_to_none=True)
        losses.append(loss.item())
    assert all(np.isfinite(v) for v in losses)
    names = [c[0] for c in trace]
    assert names.count("segk_pack_multi") == 1 and "segk_bilinear_bwd" in names and "segk_convt2x2_dgrad" in names
    check("clip_decoder_steps", trace, tuple(losses))
