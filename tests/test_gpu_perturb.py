"""MI355X: the perturbation kernels (image_segmentation_amd/robustness.py, csrc/perturb.hip) against the NumPy restatement of
their integer arithmetic (tests/perturb_reference.py) -- EXACT equality of every byte, for every kind, on one ragged batch whose
sizes cover images smaller than the blur halo (several reflections), exact tile multiples, one past a tile multiple, rows whose
byte count is no multiple of four, and enough tiles to cross descriptor boundaries.  No tolerance anywhere except the
binomial bounds of the salt-and-pepper statistics, which are derived in the test."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perturb_reference as R                                                      # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (1, 7), (2, 3), (5, 4), (13, 70), (64, 64), (65, 129), (37, 200)]
CASES = [("gaussian_blur", 1), ("gaussian_blur", 2), ("gaussian_blur", 9),
         ("gaussian_noise", 2), ("gaussian_noise", 18),
         ("salt_and_pepper", 0.02), ("salt_and_pepper", 0.18),
         ("occlusion", 5), ("occlusion", 45),
         ("contrast_increase", 1.01), ("contrast_increase", 1.25), ("contrast_decrease", 0.95), ("contrast_decrease", 0.10),
         ("brightness_increase", 5), ("brightness_increase", 45), ("brightness_decrease", 5), ("brightness_decrease", 45)]


@pytest.fixture(scope="module")
def P():
    from image_segmentation_amd import robustness
    return robustness


@pytest.fixture(scope="module")
def batch():
    """the ragged batch: smooth blocks plus noise, so that blur, clipping and the tables all have something to act on"""
    rng = np.random.default_rng(2024)
    imgs = []
    for H, W in SIZES:
        smooth = np.kron(rng.integers(0, 256, (-(-H // 6), -(-W // 6), 3)), np.ones((6, 6, 1), np.int64))[:H, :W]
        imgs.append(np.clip(smooth + rng.integers(-30, 31, (H, W, 3)), 0, 255).astype(np.uint8))
    for im in imgs:
        im.setflags(write=False)
    return imgs


def expected(P, imgs, kind, level, seed):
    """the restatement, fed with what the host drew (per-image seeds, occlusion corners)"""
    plan = P.perturb_plan(kind, level, [im.shape[:2] for im in imgs], seed)
    out = []
    for im, s, prm in zip(imgs, plan.seeds, plan.params):
        if kind == "gaussian_blur":
            out.append(R.blur(im, level))
        elif kind == "gaussian_noise":
            out.append(R.gaussian_noise(im, level, s))
        elif kind == "salt_and_pepper":
            out.append(R.salt_and_pepper(im, level, s))
        elif kind == "occlusion":
            H, W = im.shape[:2]
            assert prm[2] == min(level, H, W)
            out.append(R.occlude(im, *prm))
        else:
            out.append(R.apply_lut(im, kind, level))
    return out


def run(P, imgs, kind, level, seed=0):
    out = P.perturb(imgs, kind, level, seed=seed)
    assert len(out) == len(imgs)
    for o, im in zip(out, imgs):
        assert o.is_cuda and o.dtype == torch.uint8 and tuple(o.shape) == (im.shape[0], im.shape[1], 3)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("kind,level", CASES)
def test_device_equals_restatement_bit_for_bit(P, batch, kind, level):
    got = run(P, batch, kind, level, seed=7)
    want = expected(P, batch, kind, level, 7)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (kind, level, SIZES[k], int((g != w).sum()))
    changed = sum(int((g != im).sum()) for g, im in zip(got, batch))
    assert changed > 0                                          # the case is not a disguised identity


def test_level_zero_is_the_input(P, batch):
    for kind in P.PERTURBATIONS:
        got = run(P, batch, kind, P.DEFAULT_LEVELS[kind][0], seed=3)
        for g, im in zip(got, batch):
            assert np.array_equal(g, im), kind


@pytest.mark.parametrize("kind,level", [("gaussian_blur", 9), ("gaussian_noise", 18), ("occlusion", 5),
                                        ("contrast_decrease", 0.10), ("salt_and_pepper", 0.18)])
def test_input_forms_agree_and_inputs_are_left_alone(P, batch, kind, level):
    want = run(P, batch, kind, level, seed=5)
    # a 4-channel input equals its 3-channel prefix
    rng = np.random.default_rng(1)
    rgba = [np.concatenate([im, rng.integers(0, 256, im.shape[:2] + (1,), dtype=np.uint8)], axis=2) for im in batch]
    for g, w in zip(run(P, rgba, kind, level, seed=5), want):
        assert np.array_equal(g, w)
    # device tensors equal host arrays, and are not modified; so do views at odd addresses
    dev = [torch.from_numpy(im.copy()).cuda() for im in batch]
    keep = [t.clone() for t in dev]
    for g, w in zip(run(P, dev, kind, level, seed=5), want):
        assert np.array_equal(g, w)
    for t, k in zip(dev, keep):
        assert torch.equal(t, k)
    flat = [torch.cat([torch.zeros(1, dtype=torch.uint8), torch.from_numpy(im.copy()).reshape(-1)]).cuda() for im in batch]
    odd = [f[1:].view(im.shape) for f, im in zip(flat, batch)]
    for g, w in zip(run(P, odd, kind, level, seed=5), want):
        assert np.array_equal(g, w)
    # a mixed list: host and device, 3 and 4 channels
    mixed = [dev[k] if k % 2 else rgba[k] for k in range(len(batch))]
    for g, w in zip(run(P, mixed, kind, level, seed=5), want):
        assert np.array_equal(g, w)


def test_seeds(P, batch):
    for kind, level in [("gaussian_noise", 18), ("salt_and_pepper", 0.18), ("occlusion", 5)]:
        a, b, c = run(P, batch, kind, level, seed=1), run(P, batch, kind, level, seed=1), run(P, batch, kind, level, seed=2)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), kind
        assert any(not np.array_equal(x, y) for x, y in zip(a, c)), kind
    # two images of one call do not share their noise
    same = [batch[5], batch[5]]
    a = run(P, same, "gaussian_noise", 18, seed=1)
    assert not np.array_equal(a[0], a[1])


def test_salt_and_pepper_statistics(P):
    """Over 256 x 256 x 3 elements of a mid-grey image the hits are Binomial(n, p) with p = floor(amount 2^24) / 2^24 and,
    given the hits, the salts are Binomial(hits, 1/2): both within four standard deviations sqrt(n p (1 - p))."""
    img = np.full((256, 256, 3), 128, np.uint8)
    n = img.size
    for amount in (0.02, 0.18):
        out = run(P, [img], "salt_and_pepper", amount, seed=11)[0]
        hits = int((out != 128).sum())
        p = math.floor(amount * (1 << 24)) / (1 << 24)
        sigma = math.sqrt(n * p * (1 - p))
        print(f"amount {amount}: {hits} hits of {n}, expected {n * p:.1f}, sigma {sigma:.1f}")
        assert abs(hits - n * p) <= 4 * sigma
        assert abs(hits / n - amount) <= 4 * sigma / n + 2.0 ** -24
        salt = int((out == 255).sum())
        assert salt + int((out == 0).sum()) == hits
        s2 = math.sqrt(hits * 0.25)
        print(f"  salt {salt} of {hits}, sigma {s2:.1f}")
        assert abs(salt - hits / 2) <= 4 * s2


def test_large_batch_crosses_many_descriptors(P):
    """70 images of 3 x 5 and one of 100 x 100: more descriptors than the binary search has steps for any fixed small depth,
    one-tile images next to a many-tile one."""
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (3, 5, 3), dtype=np.uint8) for _ in range(70)]
    imgs.insert(33, rng.integers(0, 256, (100, 100, 3), dtype=np.uint8))
    for kind, level in [("gaussian_blur", 3), ("gaussian_noise", 10)]:
        got, want = run(P, imgs, kind, level, seed=4), expected(P, imgs, kind, level, 4)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), kind


def test_entries_refuse_bad_arguments(P):
    from image_segmentation_amd import _lib
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for name, args in [("segk_perturb_point", (0, 1, 1, 0, d.data_ptr(), s)), ("segk_perturb_point", (d.data_ptr(), 0, 1, 0, d.data_ptr(), s)),
                       ("segk_perturb_point", (d.data_ptr(), 1, 1, 4, d.data_ptr(), s)), ("segk_perturb_point", (d.data_ptr(), 1, 1, 0, 0, s)),
                       ("segk_perturb_point", (d.data_ptr(), 1, -1, 3, 0, s)), ("segk_perturb_blur", (d.data_ptr(), 1, 1, 10, s)),
                       ("segk_perturb_blur", (d.data_ptr(), 1, 1, -1, s)), ("segk_perturb_blur", (0, 1, 1, 1, s))]:
        with pytest.raises(RuntimeError, match=name):
            _lib.call(name, *args)
    _lib.call("segk_perturb_point", d.data_ptr(), 1, 0, 3, 0, s)          # no tiles: nothing is launched
    _lib.call("segk_perturb_blur", d.data_ptr(), 1, 0, 9, s)
    torch.cuda.synchronize()
