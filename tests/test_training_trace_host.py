"""CPU: what the loops of training.py do to their collaborators, as a record -- the four train loops, the three evaluation
loops and `_start` (through start / start_prompt) driven with recording fakes and compared with
tests/golden/training_trace.json (stored in the packed form of tests/trace_fixture.py).

The fixture is a record of the commit BEFORE the loops were folded onto one accumulation window and one evaluation pass
(DESIGN.md 3.9): the Python may be rearranged, what it calls, in which order and with what, may not change.  Set
SEGK_TRAINING_TRACE_OUT=<file> to write the record there instead of comparing.

Per case the record holds, in order of occurrence,
  * every call on a fake: ["train"/"eval", module], ["forward", module, module.training, torch.is_grad_enabled(), inputs],
    ["loss", arguments], ["zero_grad"], ["step"], ["sched"], ["arm"], ["sync"], ["reset"], ["accumulate", pred, label],
    ["metrics"] and the aggregator's getters by name; a tensor is recorded as [shape, dtype, device], an absent one as null;
  * ["grad", hex]: the accumulated gradient of the loss fake's scalar parameter right after each backward (the
    1 / accumulation_steps scaling and the sum over a window; the fake optimizer's zero_grad really clears it);
  * ["item"]: every Tensor.item() call -- the device-to-host syncs the loops make when the tensors are on a GPU
    (MetricsHistory.compute_epoch_metrics makes three more of its own);
  * the progress bars: desc, total and every set_postfix dictionary; the printed text; the returned value as its type name
    and float.hex of each number.
Every case runs three times: with a recording stand-in installed as training._tqdm ("bar"), with _tqdm = None ("nobar": the
plain iterable, no set_postfix, so one .item() per step instead of two) and with VERBOSE = False ("quiet": nothing is printed
and no bar is made).

Inputs.  The models are elementwise stubs with literal weights, every value is a small multiple of 1/4 and the loss fakes are
linear.  The train batches map onto the 16 x 16 network input with scale 1 (8 x 16 is padded, 16 x 16 is taken as it is), so
every sum is exact in float32 in any order (< 2^15 at a granularity of 2^-4).  The evaluation loops also get an 8 x 8 image,
which is really resized: up by 2 (bilinear weights 1/4 and 3/4 per axis: 2^-6 after both) and back down by 2 (bilinear: the
mean of two neighbours per axis, nearest: one of them), so the two interpolations give different numbers, still exact
(granularity 2^-10, sums of 192 terms < 2^12: 22 bits).  The record depends neither on the vector width nor on the thread
count.  The scalar parameter multiplies the finished sum, so its gradient is one correctly rounded division of an exact number.

Branches of the shared window (training._run_window) and the cases that take them both ways:
  zero_first                      the segmentation loops / trainReconstruction
  stepping                        acc 2 over 3 batches: no, yes (window end), yes (last batch); acc 3 over 1: acc > n
  grad_sync is not None           */gs-sched cases / */plain cases (arm before the stepping backward, sync after it)
  scheduler                       */gs-sched cases / */plain cases and trainReconstruction (never)
  bar has set_postfix             "bar" / "nobar" and "quiet"
  on_loss: stepping only / all    the segmentation loops (_segmentation_epoch) / trainReconstruction
  no step at all (avg of nothing) train_loop/empty
Branches of the shared evaluation pass (training._eval_pass, training._segmentation_eval) and their cases:
  heat-map present                eval_loop_prompt / eval_loop, evalReconstruction
  interpolation                   evalReconstruction bilinear / nearest (the 8 x 8 image makes their returns differ: asserted)
  agg.reset()                     eval_loop / eval_loop_prompt (the pre-loaded counts survive in its metrics)
  loss.is_cuda                    never on the CPU: tests/test_gpu_training_trace.py
  grad_sync and world > 1         never in one process: tests/test_parallel_gloo.py
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import trace_fixture
from image_segmentation_amd import training
from image_segmentation_amd.metrics import MetricsHistory

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "training_trace.json")
OUT = os.environ.get("SEGK_TRAINING_TRACE_OUT")
C = 3
W_A = [[1.0, -1.0, 0.25], [-1.0, 1.0, 0.25], [-0.25, -0.25, 1.0]]
W_B = [[0.5, 0.25, -0.75], [-0.5, 0.75, 0.0], [0.25, -0.5, 0.5]]
V_A = [0.5, -0.25, 1.0]
MODES = ("bar", "nobar", "quiet")

_RECORD = {}


@functools.lru_cache(None)
def golden():
    return trace_fixture.load(GOLDEN, "events")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    if OUT and _RECORD:
        trace_fixture.dump(OUT, {k: _RECORD[k] for k in sorted(_RECORD)}, "events")


def desc(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return [list(t.shape), str(t.dtype), str(t.device)]
    return type(t).__name__


def hexes(v):
    vals = v if isinstance(v, tuple) else (v,)
    return [type(v).__name__, [type(x).__name__ for x in vals], [float(x).hex() for x in vals]]


class Stub(torch.nn.Module):
    """y[n,c] = sum_k w[c,k] x[n,k] (+ h v[c] with a heat-map): a 1x1 convolution spelled with elementwise ops"""

    def __init__(self, ev, name, w, v=None, params=True):
        super().__init__()
        self.ev, self.name = ev, name
        w = torch.tensor(w, dtype=torch.float32)
        v = None if v is None else torch.tensor(v, dtype=torch.float32)
        if params:
            self.w = torch.nn.Parameter(w)
            self.v = None if v is None else torch.nn.Parameter(v)
        else:
            self.w, self.v = w, v

    def train(self, mode=True):
        self.ev.append(["train" if mode else "eval", self.name])
        return super().train(mode)

    def forward(self, x, h=None):
        self.ev.append(["forward", self.name, self.training, torch.is_grad_enabled(), desc(x), desc(h)])
        y = (x.unsqueeze(1) * self.w.view(1, C, 3, 1, 1)).sum(2)
        return y if h is None else y + h * self.v.view(1, C, 1, 1)


class Loss:
    """sum(pred [+ third] * (label + 1)) * 2^-8 * s (segmentation forms) or sum((pred - target) * c) * 2^-8 * s
    (float targets); s is the scalar parameter whose gradient the record holds"""

    def __init__(self, ev):
        self.ev = ev
        self.s = torch.nn.Parameter(torch.tensor(0.5))
        self.s.register_post_accumulate_grad_hook(lambda p: ev.append(["grad", float(p.grad).hex()]))

    def __call__(self, pred, y, *more):
        self.ev.append(["loss", desc(pred), desc(y)] + [desc(m) for m in more])
        p = pred + more[0] if more else pred
        if y is None:
            raw = p.sum()
        elif torch.is_floating_point(y):
            raw = ((p - y) * torch.tensor([1.0, 2.0, -1.0]).view(1, C, 1, 1)).sum()
        else:
            raw = (p * (y.unsqueeze(1).float() + 1.0)).sum()
        return raw * 2.0 ** -8 * self.s


class Opt:
    def __init__(self, ev, loss):
        self.ev, self.loss = ev, loss
        self.param_groups = [{"lr": 0.125}]

    def zero_grad(self):
        self.ev.append(["zero_grad"])
        self.loss.s.grad = None

    def step(self):
        self.ev.append(["step"])


class Sched:
    def __init__(self, ev, opt):
        self.ev, self.opt = ev, opt

    def step(self):
        self.ev.append(["sched"])
        self.opt.param_groups[0]["lr"] *= 0.5


class GS:
    def __init__(self, ev):
        self.ev = ev

    def arm(self):
        self.ev.append(["arm"])

    def sync(self):
        self.ev.append(["sync"])

    def broadcast_buffers(self, model):
        self.ev.append(["broadcast_buffers"])


class Agg(MetricsHistory):
    """Counts that depend on the label alone (no device kernel on the CPU), pre-loaded with non-zero totals."""

    def __init__(self, ev):
        super().__init__(C)
        self.ev = ev
        self.total_tp += torch.tensor([5.0, 1.0, 2.0])
        self.total_fp += torch.tensor([1.0, 7.0, 2.0])
        self.total_fn += torch.tensor([3.0, 1.0, 9.0])
        self.total_tn += torch.tensor([40.0, 40.0, 36.0])

    def reset(self):
        self.ev.append(["reset"])
        super().reset()

    def accumulate(self, pred, label):
        self.ev.append(["accumulate", desc(pred), desc(label)])
        n = torch.tensor([float((label == c).sum()) for c in range(C)], dtype=torch.float64)
        self.total_tp += n
        self.total_fp += torch.tensor([1.0, 2.0, 3.0])
        self.total_fn += torch.tensor([2.0, 0.0, 1.0])
        self.total_tn += label.numel() - n

    def compute_epoch_metrics(self, epsilon=1e-6):
        self.ev.append(["metrics"])
        return super().compute_epoch_metrics(epsilon)

    def get_num_classes(self):
        self.ev.append(["get_num_classes"])
        return super().get_num_classes()

    def get_last_per_class_iou(self):
        self.ev.append(["get_last_per_class_iou"])
        return super().get_last_per_class_iou()

    def get_ignore_index(self):
        self.ev.append(["get_ignore_index"])
        return super().get_ignore_index()


def _grid(H, W):
    return np.meshgrid(np.arange(H), np.arange(W), indexing="ij")


def image(H, W, k, cin=3):
    y, x = _grid(H, W)
    return torch.from_numpy(np.stack([((x * 5 + y * 3 + c * 7 + k) % 8) / 4.0 for c in range(cin)]).astype(np.float32))


def heat(H, W, k):
    y, x = _grid(H, W)
    return torch.from_numpy((((x * 3 + y * 7 + k) % 4) / 4.0).astype(np.float32)).unsqueeze(0)


def label(H, W, k):
    y, x = _grid(H, W)
    return torch.from_numpy(((x + 2 * y + k) % 3).astype(np.int64)).unsqueeze(0)


RAGGED = [(8, 16), (16, 16)]


def train_batch(k, form, ragged):
    """form: "seg" (X, y), "prompt" (X, p, y), "recon" (X, None), "xy"/"xnone"/"x" (the distillation forms)"""
    sizes = RAGGED if ragged else [(16, 16), (16, 16)]
    pack = (lambda ts: list(ts)) if ragged else torch.stack
    X = pack([image(H, W, k + i) for i, (H, W) in enumerate(sizes)])
    p = pack([heat(H, W, k + i) for i, (H, W) in enumerate(sizes)])
    y = pack([label(H, W, k + i) for i, (H, W) in enumerate(sizes)])
    return {"seg": (X, y), "xy": (X, y), "prompt": (X, p, y), "recon": (X, None), "xnone": (X, None), "x": X}[form]


class Bars:
    """Recording stand-in for tqdm: desc, total and every set_postfix dictionary"""

    def __init__(self):
        self.made = []

    def __call__(self, it, **kw):
        rec = {"desc": kw.get("desc"), "total": kw.get("total"), "extra": sorted(set(kw) - {"desc", "total"}), "postfix": []}
        self.made.append(rec)
        return _Bar(it, rec)


class _Bar:
    def __init__(self, it, rec):
        self.it, self.rec = it, rec

    def __iter__(self):
        return iter(self.it)

    def set_postfix(self, d):
        self.rec["postfix"].append({k: float(v).hex() for k, v in d.items()})


def run_case(name, fn, monkeypatch, capsys):
    """fn(ev) -> the value a loop returned; runs in the three modes and compares (or records) each"""
    for mode in MODES:
        ev, bars = [], Bars()
        monkeypatch.setattr(training, "_tqdm", bars if mode == "bar" else None)
        monkeypatch.setattr(training, "VERBOSE", mode != "quiet")
        real_item = torch.Tensor.item

        def item(t):
            ev.append(["item"])
            return real_item(t)
        capsys.readouterr()
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, "item", item)
            ret = fn(ev)
        printed = capsys.readouterr().out
        assert torch.is_grad_enabled()
        if mode == "quiet":
            assert printed == "" and not bars.made
        check(f"{name}/{mode}", {"events": ev, "bars": bars.made, "printed": printed, "return": ret})


def check(name, got):
    got = json.loads(json.dumps(got))
    if OUT:
        _RECORD[name] = got
        return
    want = golden()[name]
    for k, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert g == w, f"event {k}"
    assert len(got["events"]) == len(want["events"])
    assert got == want


# ---- 1. the train loops ---------------------------------------------------------------------------------------------------------

LOOPS = {"train_loop": "seg", "train_loop_prompt": "prompt", "train_loop_distill": "xy", "trainReconstruction": "recon"}


def run_train(ev, loop, form, acc, n, extras, ragged, params=True, device="cpu"):
    loss = Loss(ev)
    opt = Opt(ev, loss)
    kw = {}
    if extras:
        kw["grad_sync"] = GS(ev)
        if loop != "trainReconstruction":
            kw["scheduler"] = Sched(ev, opt)
    if ragged:
        kw["target_size"] = 16
    data = [train_batch(3 * k, form, ragged) for k in range(n)]
    model = Stub(ev, "model", W_A, V_A if form == "prompt" else None, params=params)
    if loop == "trainReconstruction":
        ret = training.trainReconstruction(data, model, loss, opt, acc, device=device, **kw)
    elif loop == "train_loop_distill":
        ret = training.train_loop_distill(data, model, Stub(ev, "teacher", W_B), loss, opt, acc, device, **kw)
    else:
        ret = getattr(training, loop)(data, model, loss, opt, acc, device, **kw)
    return hexes(ret)


@pytest.mark.parametrize("n", [1, 3, 4])
@pytest.mark.parametrize("acc", [1, 2, 3])
@pytest.mark.parametrize("loop", list(LOOPS))
def test_window_grid(loop, acc, n, monkeypatch, capsys):
    """a window that ends on the last batch, a short last window, acc > n -- with grad_sync and (where there is one) scheduler"""
    run_case(f"{loop}/gs-sched/acc{acc}/n{n}", lambda ev: run_train(ev, loop, LOOPS[loop], acc, n, True, False), monkeypatch, capsys)


@pytest.mark.parametrize("loop", list(LOOPS))
def test_plain(loop, monkeypatch, capsys):
    """no scheduler, no grad_sync"""
    run_case(f"{loop}/plain", lambda ev: run_train(ev, loop, LOOPS[loop], 2, 3, False, False), monkeypatch, capsys)


@pytest.mark.parametrize("loop", ["train_loop", "train_loop_prompt", "train_loop_distill"])
def test_ragged_lists(loop, monkeypatch, capsys):
    """target_size=16 on lists of an 8 x 16 and a 16 x 16 image: the resize + pad of images, heat-maps (bilinear), labels (nearest)"""
    run_case(f"{loop}/ragged", lambda ev: run_train(ev, loop, LOOPS[loop], 2, 3, True, True), monkeypatch, capsys)


def test_empty_loader(monkeypatch, capsys):
    def fn(ev):
        ret = run_train(ev, "train_loop", "seg", 2, 0, True, False)
        assert ret[0] == "int"
        return ret
    run_case("train_loop/empty", fn, monkeypatch, capsys)


@pytest.mark.parametrize("form,ragged", [("xy", False), ("xnone", False), ("x", False), ("xnone", True)])
def test_distill_batch_forms(form, ragged, monkeypatch, capsys):
    run_case(f"train_loop_distill/form-{form}{'-ragged' if ragged else ''}",
             lambda ev: run_train(ev, "train_loop_distill", form, 2, 3, True, ragged), monkeypatch, capsys)


@pytest.mark.parametrize("params", [True, False])
def test_train_reconstruction_device_none(params, monkeypatch, capsys):
    def fn(ev):
        ret = run_train(ev, "trainReconstruction", "recon", 2, 3, False, False, params=params, device=None)
        assert ret[0] == "float64"
        return ret
    run_case(f"trainReconstruction/device-none/{'params' if params else 'no-params'}", fn, monkeypatch, capsys)


# ---- 2. the evaluation loops --------------------------------------------------------------------------------------------------

EVAL_SIZES = [[(8, 16), (16, 16)], [(16, 16), (8, 8)]]  # four ragged images in two batches; 8 x 8 is really resized (x 2)


def eval_data(form, rgba=False):
    data, k = [], 0
    for sizes in EVAL_SIZES:
        X = [image(H, W, k + i, 4 if rgba and (H, W) == (8, 16) else 3) for i, (H, W) in enumerate(sizes)]
        p = [heat(H, W, k + i) for i, (H, W) in enumerate(sizes)]
        y = [label(H, W, k + i) for i, (H, W) in enumerate(sizes)]
        data.append({"seg": (X, y), "prompt": (X, p, y), "recon": (X, None)}[form])
        k += 5
    return data


@pytest.mark.parametrize("loop", ["eval_loop", "eval_loop_prompt"])
def test_eval_loops(loop, monkeypatch, capsys):
    def fn(ev):
        prompt = loop == "eval_loop_prompt"
        model = Stub(ev, "model", W_A, V_A if prompt else None).train()
        agg = Agg(ev)
        ret = getattr(training, loop)(eval_data("prompt" if prompt else "seg"), model, Loss(ev), "cpu", 16, agg)
        assert not model.training
        return hexes(ret) + [[float(v).hex() for v in agg.total_tp]]
    run_case(loop, fn, monkeypatch, capsys)


def test_eval_reset_difference():
    """eval_loop drops the counts the aggregator held, eval_loop_prompt adds to them (as the reference does)"""
    if OUT:
        return
    want = golden()
    a, b = want["eval_loop/quiet"], want["eval_loop_prompt/quiet"]
    assert ["reset"] in a["events"] and ["reset"] not in b["events"]
    assert [float.fromhex(x) - float.fromhex(y) for x, y in zip(b["return"][3], a["return"][3])] == [5.0, 1.0, 2.0]
    assert a["return"][2][1:] != b["return"][2][1:]


def test_eval_interpolation_difference():
    """the 8 x 8 image comes back from 16 x 16 through `interpolation`: nearest and bilinear give different losses, and the
    same events"""
    if OUT:
        return
    a, b = golden()["evalReconstruction/bilinear/quiet"], golden()["evalReconstruction/nearest/quiet"]
    assert a["events"] == b["events"] and a["return"][2][0] != b["return"][2][0] and a["return"][2][1] != b["return"][2][1]


@pytest.mark.parametrize("variant,kw,params", [("bilinear", {}, True), ("nearest", {"interpolation": "nearest"}, True),
                                               ("no-params", {}, False), ("device-cpu", {"device": "cpu"}, True)])
def test_eval_reconstruction(variant, kw, params, monkeypatch, capsys):
    """an RGBA image among the four: cut to RGB for the network and for the loss target"""
    def fn(ev):
        model = Stub(ev, "model", W_A, params=params).train()
        ret = training.evalReconstruction(eval_data("recon", rgba=True), model, Loss(ev), 16, **kw)
        assert not model.training and type(ret[1]).__name__ == "float64"
        return hexes(ret)
    run_case(f"evalReconstruction/{variant}", fn, monkeypatch, capsys)


# ---- 3. _start ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prompt", [False, True])
@pytest.mark.parametrize("gs", [False, True])
def test_start(prompt, gs, monkeypatch, capsys, tmp_path):
    """two epochs over fake loops: what each loop call received (grad_sync passed or defaulted is the same call) and the files"""
    for mode in ("bar", "quiet"):
        calls = []
        model = torch.nn.Linear(1, 1)
        opt = torch.optim.SGD(model.parameters(), lr=0.5)
        names = {id(model): "model", id(opt): "optimizer"}
        for n in ("train_dl", "val_dl", "train_loss", "val_loss", "sched", "agg"):
            names[n] = type(n, (), {"state_dict": lambda self: {}})() if n == "sched" else object()
            names[id(names[n])] = n
        grad_sync = GS(calls) if gs else None
        scores = iter([(0.75, 0.5, 0.5), (0.5, 0.75, 0.25)])        # improved, then not

        def say(a):
            return names.get(id(a), a if isinstance(a, (int, str, type(None))) else type(a).__name__)

        def fake(which):
            def loop(*a, **k):
                assert k.get("grad_sync") is grad_sync
                calls.append([which, [say(x) for x in a], {key: say(v) for key, v in sorted(k.items()) if key != "grad_sync"}])
                return next(scores) if which.startswith("eval") else 0.0
            return loop
        for which in ("train_loop", "eval_loop", "train_loop_prompt", "eval_loop_prompt"):
            monkeypatch.setattr(training, which, fake(which))
        monkeypatch.setattr(training, "VERBOSE", mode != "quiet")
        d = tmp_path / f"{mode}"
        capsys.readouterr()
        ret = (training.start_prompt if prompt else training.start)(
            str(d), "m.pt", model, opt, names["train_dl"], names["val_dl"], 2, "cpu", names["train_loss"], names["val_loss"], 16,
            scheduler=names["sched"], agg=names["agg"], load=False, epochs=2, grad_sync=grad_sync)
        printed = capsys.readouterr().out.replace(str(d), "<dir>")
        files = {}
        for root, _, fs in os.walk(d):
            for f in fs:
                path = os.path.join(root, f)
                files[os.path.relpath(path, d)] = sorted(torch.load(path, weights_only=False))
        check(f"start{'_prompt' if prompt else ''}/{'gs' if gs else 'plain'}/{mode}",
              {"events": calls, "printed": printed, "return": hexes(ret), "files": files})
