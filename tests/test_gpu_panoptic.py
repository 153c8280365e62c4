"""MI355X: object-level evaluation (image_segmentation_amd/panoptic.py, csrc/panoptic.hip) against the restatement of DESIGN.md
3.19 in tests/panoptic_reference.py -- EXACT equality of the pair table, every per-segment array, totals and stats, for both
connectivities, through the C ABI (segk_pq_pairs / segk_pq_match on the restatement's label maps) and through
seg.match_objects (on the masks, labelled by segk_cc_label).  Output and workspace buffers start as 0xFF bytes with slack
behind them: what lies at or past a capacity or a total, and everything on overflow, must still be 0xFF afterwards, and nothing
may rest on a zeroed workspace.  There is nothing to tolerance: the arithmetic is integer and the definition makes the result
unique.  The overflow cases are ordinary bounded runs."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panoptic_cases as PC                                                        # noqa: E402
import panoptic_reference as PR                                                    # noqa: E402

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("connectivity", [4, 8])
SLACK = 16
BASE = (np.arange(128, dtype=np.int64).reshape(8, 16) * 1000003 + 7)               # what stats holds before a call


def stuff_mask(case):
    return sum(1 << c for c in case["stuff"])


def run_abi(name, connectivity, cap, mp, stream=None):
    """both entries on the restatement's label maps, every buffer pre-filled with 0xFF -> the whole buffers as NumPy arrays"""
    from image_segmentation_amd import _lib, ops, panoptic as P
    case = PC.CASES[name]
    Lp, cls_p, Lg, cls_g = PC.labelled(name, connectivity)
    H, W = case["pred"].shape
    dev = torch.device("cuda:0")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    pred, target, lp, lg = up(case["pred"], np.uint8), up(case["target"], np.uint8), up(Lp, np.int32), up(Lg, np.int32)

    def cls_rows(cls):                       # cap rows; a labelling with more components than cap shows its first cap classes
        a = np.zeros(cap, np.int32)
        a[:min(cap, len(cls))] = cls[:cap]
        return up(a, np.int32)
    cp, cg = cls_rows(cls_p), cls_rows(cls_g)
    nump, numg = up([len(cls_p)], np.int32), up([len(cls_g)], np.int32)
    full = lambda n, dt=torch.int32: torch.full((n,), -1, dtype=dt, device=dev)
    pairs = {n: full(mp + SLACK) for n in PR.PAIR_ARRAYS}
    seg = {n: full(cap + 8 + SLACK) for n in PR.SEG_ARRAYS}
    totals = full(4)
    stats = torch.from_numpy(BASE.copy()).to(dev)
    ws = full(P.ws_ints(H, W, mp, cap) + SLACK)
    ign = -1 if case["ignore_index"] is None else case["ignore_index"]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
        s = ops._stream()
        _lib.call("segk_pq_pairs", pred.data_ptr(), lp.data_ptr(), nump.data_ptr(), target.data_ptr(), lg.data_ptr(), numg.data_ptr(),
                  *(pairs[n].data_ptr() for n in PR.PAIR_ARRAYS), totals.data_ptr(), ws.data_ptr(), H, W, stuff_mask(case), ign, cap,
                  mp, s)
        _lib.call("segk_pq_match", *(pairs[n].data_ptr() for n in PR.PAIR_ARRAYS), totals.data_ptr(), cp.data_ptr(), nump.data_ptr(),
                  cg.data_ptr(), numg.data_ptr(), *(seg[n].data_ptr() for n in PR.SEG_ARRAYS), stats.data_ptr(), cap, mp, s)
    torch.cuda.synchronize()
    for t, a, what in ((pred, case["pred"], "pred"), (target, case["target"], "target"), (lp, Lp, "pred labels"), (lg, Lg, "target labels")):
        assert np.array_equal(t.cpu().numpy(), a), f"{what} was modified"
    assert (ws[-SLACK:] == -1).all(), "the workspace was written past SEGK_PQ_WS_INTS"
    got = {n: b.cpu().numpy() for n, b in {**pairs, **seg}.items()}
    got["totals"], got["stats"] = totals.cpu().numpy(), stats.cpu().numpy()
    return got


def expected(name, connectivity, cap, mp):
    res = PC.reference(name, connectivity, cap, mp)
    want = {"totals": res["totals"], "stats": BASE + res["stats"]}
    for n, a in PR.expected_pairs(res, mp + SLACK).items():
        want[n] = a
    for n in PR.SEG_ARRAYS:
        want[n] = np.concatenate([res[n], np.full(SLACK, -1, np.int32)])
    return want, res


def compare(got, want, what):
    assert got["totals"].tolist() == want["totals"].tolist(), f"{what}: totals {got['totals'].tolist()}, expected {want['totals'].tolist()}"
    for n in PR.PAIR_ARRAYS + PR.SEG_ARRAYS + ("stats",):
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n)
        bad = np.flatnonzero((got[n] != want[n]).reshape(len(want[n]), -1).any(axis=1))
        assert bad.size == 0, f"{what}: {n} differs in {bad.size} rows, first at {bad[0]}: {got[n][bad[0]]} != {want[n][bad[0]]}"


@pytest.mark.parametrize("name", PC.NAMES)
@BOTH
def test_c_abi_equals_the_restatement(name, connectivity):
    first = None
    for regime, (cap, mp) in PC.regimes(name, connectivity).items():
        got = run_abi(name, connectivity, cap, mp)
        want, res = expected(name, connectivity, cap, mp)
        compare(got, want, f"{name} c{connectivity} {regime} cap={cap} max_pairs={mp}")
        if regime in ("pairs-1", "components-1"):                          # overflow: all -1, nothing else touched
            assert got["totals"].tolist() == [-1] * 4 and np.array_equal(got["stats"], BASE)
            assert all((got[n] == -1).all() for n in PR.PAIR_ARRAYS + PR.SEG_ARRAYS)
        else:
            assert got["totals"][0] == res["P"] and int(got["pair_n"][:res["P"]].sum()) == PC.CASES[name]["pred"].size
        first = first or ((cap, mp), got)
    (cap, mp), got = first                                                 # the roomy regime again, and on a side stream
    again, side = run_abi(name, connectivity, cap, mp), run_abi(name, connectivity, cap, mp, torch.cuda.Stream())
    for n in got:
        assert np.array_equal(again[n], got[n]) and np.array_equal(side[n], got[n]), (name, n)


def device_case(name):
    case = PC.CASES[name]
    dev = torch.device("cuda:0")
    pred, target = torch.from_numpy(case["pred"].copy()).to(dev), torch.from_numpy(case["target"].copy()).to(dev)
    given = None
    if case["target_objects"] is not None:
        given = (torch.from_numpy(case["target_objects"][0].copy()).to(dev), torch.tensor(case["target_objects"][1], dtype=torch.int32, device=dev))
    return case, pred, target, given


def check_match(m, res, cap, what):
    """the defined parts of an ObjectMatch made of torch.empty buffers: the pair prefix, the rows in use, totals"""
    assert m.totals.cpu().numpy().tolist() == res["totals"].tolist(), what
    if res["totals"][0] < 0:
        assert not m.complete
        return
    P = int(res["totals"][0])
    assert m.complete and np.array_equal(m.pairs(), res["pairs"]), what
    for n in PR.SEG_ARRAYS:
        a, w = getattr(m, n).cpu().numpy(), res[n]
        assert a.shape == (cap + 8,) and np.array_equal(a[w >= 0], w[w >= 0]), (what, n)
    assert int(m.pred_num.item()) == res["Kp"] and int(m.target_num.item()) == res["Kg"]
    assert m.pred_cls[:res["Kp"]].cpu().numpy().tolist() == res["cls_p"] and m.target_cls[:res["Kg"]].cpu().numpy().tolist() == res["cls_g"]
    rows = [r for r in range(cap + 8) if res["match_g"][r] > 0]
    assert m.matches().tolist() == [[r + 1, int(res["match_g"][r]), int(res["inter_g"][r]), int(res["union_g"][r])] for r in rows]
    if P > 1500:                                                           # the dense table is for small cases
        return
    T, gs, ps = m.contingency()
    Tr, gr, pr = PR.contingency(res)
    assert np.array_equal(T, Tr) and gs.tolist() == gr and ps.tolist() == pr and T.sum() == m.size[0] * m.size[1] and P == (T > 0).sum()


@pytest.mark.parametrize("name", PC.NAMES)
@BOTH
def test_match_objects_equals_the_restatement(name, connectivity):
    import image_segmentation_amd as seg
    case, pred, target, given = device_case(name)
    for regime, (cap, mp) in PC.regimes(name, connectivity).items():
        res = PC.reference(name, connectivity, cap, mp)
        # the target as the int64 [1,H,W] label map the loaders give, void as -100 where the case has 255 and no ignore_index
        tl = target.long()[None]
        if case["ignore_index"] is None:
            tl = torch.where(tl == 255, -100, tl)
        if given is not None and given[1].shape[0] > cap:                  # the instances are counted on the host: refused
            with pytest.raises(ValueError, match="exceed max_components"):
                seg.match_objects(pred, tl, case["things"], case["stuff"], case["ignore_index"], connectivity, cap, mp, target_objects=given)
            continue
        m = seg.match_objects(pred, tl, case["things"], case["stuff"], case["ignore_index"], connectivity, cap, mp, target_objects=given)
        check_match(m, res, cap, f"{name} c{connectivity} {regime}")
        assert np.array_equal(m.stats.cpu().numpy(), res["stats"])         # a fresh zeroed stats; untouched on overflow
    assert np.array_equal(pred.cpu().numpy(), case["pred"]) and np.array_equal(target.cpu().numpy(), case["target"])


def test_defaults_prediction_and_stats_add_up():
    import image_segmentation_amd as seg
    from image_segmentation_amd import panoptic as P
    a, b = "blobs_shift_128x160", "identical"
    stats = torch.zeros((8, 16), dtype=torch.int64, device="cuda:0")
    total = np.zeros((8, 16), np.int64)
    for name in (a, b):
        case, pred, target, _ = device_case(name)
        H, W = case["pred"].shape
        res = PC.reference(name, 4, 1024, P.default_max_pairs(H, W, 1024))
        holder = type("Pred", (), {"mask": pred})()                        # anything with a .mask: a Prediction
        m = seg.match_objects(holder, target, (1, 2), (0,), 3, stats=stats)
        assert m.pair_g.shape[0] == min(H * W, 4096) and m.stats is stats
        check_match(m, res, 1024, name)
        total += res["stats"]
        assert np.array_equal(stats.cpu().numpy(), total), "stats after two images is the sum of the two restated ones"
    same = PC.reference(b, 4, 1024, 4096)["stats"]                          # pred == target: every IoU is 1
    assert (same[:, 3] == same[:, 0] << 32).all() and (same[:, 1:3] == 0).all() and same[:, 0].sum() == 32


def test_panoptic_quality_equals_the_float64_restatement():
    import image_segmentation_amd as seg
    names = ["noise0.5_3c_33x65", "noise0.5_3c_65x33", "noise0.5_3c_64x129", "noise0.5_3c_32x64"]     # things (1, 2, 3), stuff (0,)
    counts = [PC.true_counts(n, 4) for n in names]
    cap, ps = max(k for k, _ in counts) + 3, sorted(p for _, p in counts)
    assert ps[1] < ps[2]                                                   # the tight table holds two of the four images
    for kw, limit in ((dict(max_components=cap, max_pairs=ps[3] + 5), None), (dict(max_components=cap, max_pairs=ps[1]), ps[1])):
        pq = seg.PanopticQuality(4, things=(1, 2, 3), stuff=(0,), **kw)
        other = seg.PanopticQuality(4, things=(1, 2, 3), stuff=(0,), **kw)
        total, bad = np.zeros((8, 16), np.int64), 0
        for i, name in enumerate(names):
            case, pred, target, _ = device_case(name)
            res = PC.reference(name, 4, cap, kw["max_pairs"])
            (pq if i < 2 else other).update(pred, target)
            total += res["stats"]
            bad += int(res["totals"][0] < 0)
        assert bad == (0 if limit is None else 2)
        out = pq.add_(other).compute()
        want = PR.quality(total, [0, 1, 2, 3], 4)
        for k, v in want.items():
            assert out[k] == v, (k, out[k], v)                              # float64 == float64: the same expressions on equal integers
        assert out["incomplete_images"] == bad and out["images"] == len(names)
        json.dumps(out)
        pq.reset()
        assert pq.compute()["mean_pq"] is None and pq.compute()["images"] == 0
    # things=None: every class but ignore_index; object_quality is update() over a list, labels from the host
    names = ["blobs_shift_128x160"]
    case, pred, target, _ = device_case(names[0])
    out = seg.object_quality([pred], [case["target"].astype(np.int64)], 4, ignore_index=3, max_components=2048)
    lab = PR.label_sides(case["pred"], case["target"], (0, 1, 2), 4)
    res = PR.evaluate(case["pred"], case["target"], lab, (), 3, 2048, 8192)
    assert res["totals"][0] > 0
    want = PR.quality(res["stats"], [0, 1, 2], 4)
    assert all(out[k] == v for k, v in want.items()) and out["incomplete_images"] == 0


def test_cpu_tensors_raise():
    import image_segmentation_amd as seg
    m = torch.zeros((4, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.match_objects(m, m, (1,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.match_objects(m.cuda(), m, (1,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.PanopticQuality(2).update(m, m)


def test_evaluate_objects_tool_writes_the_library_result(tmp_path):
    """tools/evaluate_objects.py --min-area: the JSON it writes is PanopticQuality over the Segmenter's own cleaned masks"""
    import subprocess
    from PIL import Image
    import image_segmentation_amd as seg
    from oracle.fill import fill, fill_module
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = seg.unet(3, 4)
    fill_module(m, 1000)
    torch.save({"model_state_dict": m.state_dict()}, tmp_path / "w.pt")
    (tmp_path / "img").mkdir(); (tmp_path / "lab").mkdir()
    images, labels = [], []
    for i, (h, w) in enumerate(((40, 56), (33, 61))):
        images.append((fill((h, w, 3), 70 + i, 0, 1).numpy() * 255).astype(np.uint8))
        labels.append(PC.noise(h, w, 0.3, 3, 40 + i, void=0.02))
        Image.fromarray(images[-1], "RGB").save(tmp_path / "img" / f"im{i}.png")
        Image.fromarray(labels[-1], "L").save(tmp_path / "lab" / f"im{i}.png")
    m.cuda().eval()
    for extra, clean in ((["--min-area", "6"], dict(min_area=6)),):
        out = tmp_path / f"pq{len(extra)}.json"
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "evaluate_objects.py"), "--checkpoint", str(tmp_path / "w.pt"),
                            "--images", str(tmp_path / "img"), "--labels", str(tmp_path / "lab"), "--size", "64", "--classes", "4",
                            "--things", "1,2", "--stuff", "0", "--ignore-index", "3", "--out", str(out), *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = json.load(open(out))
        preds = seg.Segmenter(m, target_size=64, palette=None, clean=clean)(images)
        want = seg.object_quality(preds, [l.astype(np.int64) for l in labels], 4, things=(1, 2), stuff=(0,), ignore_index=3)
        for k, v in want.items():
            assert got[k] == v, (k, got[k], v)
        assert got["images"] == 2 and got["incomplete_images"] == 0 and got["min_area"] == 6
        # and the restatement on the masks the device produced
        total = np.zeros((8, 16), np.int64)
        for p, l in zip(preds, labels):
            mask = p.mask.cpu().numpy()
            total += PR.evaluate(mask, l, PR.label_sides(mask, l, (1, 2), 4), (0,), 3, 1024, 4096)["stats"]
        assert all(got[k] == v for k, v in PR.quality(total, [0, 1, 2], 4).items())
