"""MI355X: robustness_sweep (image_segmentation_amd/robustness.py) against its own definition -- every cell equals, exactly,
perturb -> Segmenter(labels=) -> summed confusion counts -> MetricsHistory with that cell's seed; identity levels are the clean
run; the result is plain JSON and reproducible."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZES = [(37, 53), (64, 40), (32, 32), (50, 75)]
KINDS = ("gaussian_noise", "gaussian_blur")
LEVELS = {"gaussian_noise": (0, 10, 60), "gaussian_blur": (0, 1, 9)}
T, C, IGNORE = 32, 3, 255


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as s
    return s


@pytest.fixture(scope="module")
def setup(seg):
    torch.manual_seed(0)
    model = seg.unet(3, C).cuda().eval()
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SIZES]
    labels = [np.array([0, 1, 2, 255], np.int64)[rng.integers(0, 4, (H, W))] for H, W in SIZES]
    sweep = seg.robustness_sweep(model, images, labels, C, ignore_index=IGNORE, perturbations=KINDS, levels=LEVELS, seed=5,
                                 target_size=T)
    return model, images, labels, sweep


def by_hand(seg, model, batch, labels):
    """Segmenter(labels=) -> summed confusion -> MetricsHistory, spelled out"""
    from image_segmentation_amd.metrics import MetricsHistory
    preds = seg.Segmenter(model, target_size=T)(batch, labels=labels)
    M = torch.stack([p.confusion for p in preds]).sum(dim=0).cpu()
    assert int(M.sum()) == sum(int((lb != IGNORE).sum()) for lb in labels)       # ignored pixels are not counted
    agg = MetricsHistory(C, IGNORE)
    tp, fp, fn, tn = MetricsHistory.counts_from_confusion(M, int(M.sum()))
    agg.total_tp += tp; agg.total_fp += fp; agg.total_fn += fn; agg.total_tn += tn
    dice, iou, acc = agg.compute_epoch_metrics()
    return dice, iou, acc, agg.last_per_class_dice.tolist()


def cell(res, kind, li):
    r = res[kind]
    return r["dice"][li], r["iou"][li], r["accuracy"][li], r["per_class_dice"][li]


def test_every_cell_equals_the_hand_composition(seg, setup):
    model, images, labels, sweep = setup
    from image_segmentation_amd import robustness as P
    assert set(sweep) == set(KINDS)
    for kind in KINDS:
        assert sweep[kind]["levels"] == [float(x) for x in LEVELS[kind]]
        for li, level in enumerate(LEVELS[kind]):
            batch = seg.perturb(images, kind, level, seed=P.cell_seed(5, P.PERTURBATIONS.index(kind), li))
            want = by_hand(seg, model, batch, labels)
            got = cell(sweep, kind, li)
            assert got == want, (kind, level, got, want)
            assert all(math.isfinite(v) for v in got[:3]) and len(got[3]) == C
    # the perturbation does reach the model: the strongest levels move the score
    assert cell(sweep, "gaussian_noise", 2) != cell(sweep, "gaussian_noise", 0)
    assert cell(sweep, "gaussian_blur", 2) != cell(sweep, "gaussian_blur", 0)


def test_level_zero_cells_are_the_clean_run(seg, setup):
    model, images, labels, sweep = setup
    clean = by_hand(seg, model, images, labels)
    for kind in KINDS:
        assert cell(sweep, kind, 0) == clean
    # and for every kind at its default first level, one level each
    one = seg.robustness_sweep(model, images, labels, C, ignore_index=IGNORE, seed=5, target_size=T,
                               levels={k: seg.DEFAULT_LEVELS[k][:1] for k in seg.PERTURBATIONS})
    assert list(one) == list(seg.PERTURBATIONS)
    for kind in seg.PERTURBATIONS:
        assert cell(one, kind, 0) == clean, kind


def test_result_is_json_and_reproducible(seg, setup):
    model, images, labels, sweep = setup
    assert json.loads(json.dumps(sweep)) == sweep
    again = seg.robustness_sweep(model, images, labels, C, ignore_index=IGNORE, perturbations=KINDS, levels=LEVELS, seed=5,
                                 target_size=T)
    assert again == sweep
    other = seg.robustness_sweep(model, images, labels, C, ignore_index=IGNORE, perturbations=("gaussian_noise",),
                                 levels=LEVELS, seed=6, target_size=T)
    assert other["gaussian_noise"]["dice"][0] == sweep["gaussian_noise"]["dice"][0]


def test_two_input_model_needs_its_prompt(seg, setup):
    _, images, labels, _ = setup
    torch.manual_seed(1)
    m = seg.PromptModel(clip=seg.unet(3, 4)).cuda().eval()
    with pytest.raises(ValueError, match=r"takes \(image, heatmap\)"):
        seg.robustness_sweep(m, images, labels, 4, ignore_index=3, perturbations=("occlusion",),
                             levels={"occlusion": (0, 5)}, target_size=T)
    res = seg.robustness_sweep(m, images, labels, 4, ignore_index=3, perturbations=("occlusion",),
                               levels={"occlusion": (0, 20)}, target_size=T, points=[(3, 4)] * len(images))
    assert len(res["occlusion"]["dice"]) == 2 and json.loads(json.dumps(res)) == res
