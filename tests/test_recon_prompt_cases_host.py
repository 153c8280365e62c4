"""CPU: what tests/test_gpu_recon_matrix.py, tests/test_gpu_prompt_matrix.py and tests/test_gpu_label_count_matrix.py rest on.

  * the restatements (tests/recon_reference.py, tests/prompt_reference.py, tests/augment_reference.py) against pinned data: the
    prompt fixture captured from the reference's own functions, torch's float64 convolution / sigmoid / mse_loss, and ATen's
    float32 mse_loss backward bit for bit;
  * the case tables reach what they claim, derived from the restated launch arithmetic alone;
  * the conditions on the inputs that make the bounds mean something (no unstable class choice; a dropped channel, tap or bias
    moves an output by more than eight times its allowed error).  A case that misses one gets another seed in its table, never
    another bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_reference as AR
import prompt_reference as P
import recon_reference as R
from oracle.fill import fill

FIXTURE_CASES = ["sq256", "odd33x47", "rect128x96", "single64", "zero128", "trimap96x128"]


@pytest.fixture(scope="module")
def seg():
    import image_segmentation_amd as s
    return s


def fixture_stable(scores):
    """tests/test_gpu_prompt_points.py's stable_mask: the reference's choice under the fixture's bound"""
    srt = np.sort(scores[:, 1:], axis=1)
    top, second = srt[:, -1], srt[:, -2]
    return (top < 1e-9 - 4e-12) | ((top > 1e-9 + 4e-12) & (top - second > 4e-12 + 4e-12 * top))


# ---- restatements against pinned data --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_prompt_restatements_reproduce_the_fixture(seg, golden, name):
    g = golden("prompt_points")
    c = {k: g[f"{name}.{k}"] for k in ("labels", "remapped", "centers", "scores", "cls", "taken", "heat8", "masks", "skipped")}
    lut = seg.TRIMAP_TO_PROMPT if name.startswith("trimap") else None
    lab = c["labels"].astype(np.int64)
    H, W = lab.shape
    w, q, Rw = seg.heat_tables(3.0, H, W)
    assert np.array_equal(P.class_of(lab, lut), c["remapped"])
    sc, N, cls = P.scores(lab, lut, c["centers"], w, len(w), Rw)
    ref = c["scores"]
    err = np.abs(sc[:, 1:] - ref[:, 1:])               # the reference sums the whole image, the restatement the window
    assert (err <= 2e-12 + 2e-12 * ref[:, 1:]).all(), float(err.max())
    st = fixture_stable(ref)
    assert np.array_equal(cls[st], c["cls"][st])
    heat, target, classes, cen, valid = P.make(lab, lut, c["centers"], c["cls"], q, len(q), 2)
    assert bool(c["skipped"]) == (valid == 0)
    if c["skipped"]:
        assert not heat.any() and not target.any() and not classes.any() and not cen.any()
        return
    taken = c["taken"]
    assert classes.tolist() == c["cls"][taken].tolist() and cen.tolist() == c["centers"][taken].tolist()
    assert np.array_equal(heat, c["heat8"].astype(np.float32) / np.float32(255.0))
    assert np.array_equal(target, c["masks"].astype(np.int64))
    for j, k in enumerate(taken):                    # one point gives the training form
        assert np.array_equal(P.heatmap([c["centers"][k]], q, len(q), H, W), heat[j])


def test_prompt_tables_and_class_rule(seg):
    assert np.array_equal(P.TRIMAP, seg.TRIMAP_TO_PROMPT)
    w, q, Rw = seg.heat_tables(P.Q_SIGMA, 256, 256)
    assert len(q) == P.Q_LEN and np.array_equal(P.q_table(), q) and np.array_equal(P.tables(P.Q_SIGMA, P.Q_LEN)[0], w)
    assert np.count_nonzero(P.q_table()) == 100 and P.q_table()[99] > 0        # nq = 100 cuts behind the last non-zero entry
    lab = np.array([0, 7, 8, 255, 256, -1, 2 ** 40 + 3, -2 ** 63, 3], dtype=np.int64)
    assert P.class_of(lab, None).tolist() == [0, 7, 0, 0, 0, 0, 0, 0, 3]
    assert P.class_of(lab, P.TRIMAP).tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 1]
    assert int(P.WIDE.max()) == 11 and (P.WIDE >= 8).sum() > 60
    assert P.class_of(np.arange(256), P.WIDE).tolist() == [int(v) if v < 8 else 0 for v in P.WIDE]
    s = np.array([5.0, 1.0, 3.0, 3.0, 0, 0, 0, 0])
    assert P.choose(s) == 2 and P.choose(np.array([9.0, 0, 0, 0, 0, 0, 0, 9.9e-10])) == 0
    assert P.choose(np.array([0, 0, 0, 0, 0, 0, 0, 1e-9])) == 7
    # several points: the maximum of the single heat-maps; points outside contribute nothing
    q = P.q_table()
    pts = [(2, 3), (9, 1), (-1, 4), (5, 12)]
    both = P.heatmap(pts, q, 100, 10, 12)
    assert np.array_equal(both, np.maximum(P.heatmap([pts[0]], q, 100, 10, 12), P.heatmap([pts[1]], q, 100, 10, 12)))
    assert both[2, 3] == 1.0 and not P.heatmap(pts[2:], q, 100, 10, 12).any()


HEAD_HOST = [(2, 9, 11, 5, 3, True, "fp32"), (1, 4, 6, 17, 2, False, "bf16"), (1, 1, 1, 3, 1, True, "bf16")]


@pytest.mark.parametrize("B,H,W,Cin,Cout,bias,dtype", HEAD_HOST)
def test_recon_head_restatement_is_torchs_float64(B, H, W, Cin, Cout, bias, dtype):
    c = R.HeadCase(dtype, B, H, W, Cin, R.pad32(Cin), Cout, bias, 31)
    xa, w, b = R.head_inputs(c)
    assert not xa[..., Cin:].any()
    rec, S, z = R.head(xa, w, b, dtype)
    x64 = xa[..., :Cin].permute(0, 3, 1, 2).double()
    w64 = (w.bfloat16() if dtype == "bf16" else w).double()
    b64 = None if b is None else b.double()
    assert (rec - torch.sigmoid(F.conv2d(x64, w64, b64, padding=1))).abs().max().item() <= 1e-14
    Sref = F.conv2d(x64.abs(), w64.abs(), None if b is None else b64.abs(), padding=1)
    assert (S - Sref).abs().max().item() <= 1e-13 * Sref.abs().max().item()
    # the float32 restatement sits inside the gate it helps to define
    assert ((R.head32(xa, w, b, dtype).double() - rec).abs() <= R.head_bound(S, z, Cin)).all()


def test_sigmoid_restatements():
    z = np.array([40.0, -40.0, 90.0, -90.0, 104.0, -104.0, 0.0], dtype=np.float32)
    got = R.sigmoid32(z)
    sat = R.saturation(z)                            # torch's float32 sigmoid: what the saturation cells expect
    assert np.array_equal(got[[0, 2, 3, 4, 5, 6]], sat[[0, 2, 3, 4, 5, 6]])
    assert abs(float(got[1]) - float(sat[1])) <= float(np.spacing(sat[1]))        # exp(40): the two math libraries differ by an ulp
    assert sat[1] == np.float32(1.0 / (1.0 + np.exp(40.0)))
    for v in (got, sat):
        assert np.isfinite(v).all() and v[0] == 1.0 and v[2] == 1.0 and v[4] == 1.0 and v[3] == 0.0 and v[5] == 0.0
        assert 0.0 < v[1] < 1e-17 and v[6] == 0.5
    drec, rec = fill((2, 3, 4, 5), 3, -1, 1), fill((2, 3, 4, 5), 4, 0, 1)
    want = torch.ops.aten.sigmoid_backward(drec, rec)
    for dtype in ("fp32", "bf16"):
        dz = R.sigmoid_bwd(drec, rec, 32, dtype)
        assert dz.shape == (2, 4, 5, 32) and not dz[..., 3:].any()
        assert torch.equal(dz[..., :3], want.permute(0, 2, 3, 1).to(R.TORCH_DT[dtype]))


@pytest.mark.parametrize("n", [1, 7, 4097, 65539])
@pytest.mark.parametrize("mean", [1, 0])
def test_mse_restatements_are_torchs(n, mean):
    """against F.mse_loss in float64 within 1e-12 on inputs of the lattice k / 1024, where float32(a - b) and float32(d * d) are
    exact (20 bits), so the restatement's terms ARE the float64 terms; on the matrix's own inputs the two float32 roundings
    of a term, (1 + u)^2 (1 + u) with u = 2^-24, bound the distance by 3 u (first order) of the sum of non-negative terms"""
    red = "mean" if mean else "sum"
    a, b = (t[:n] for t in R.mse_master())
    la, lb = (a * 1024).round() / 1024, (b * 1024).round() / 1024
    truth = F.mse_loss(la.double(), lb.double(), reduction=red).item()
    assert abs(R.mse_sum(la, lb) * (1.0 / n if mean else 1.0) - truth) <= 1e-12 * abs(truth)
    assert float(R.mse(la, lb, mean)) == float(np.float32(truth)) or abs(float(R.mse(la, lb, mean)) - truth) <= abs(truth) * 2.0 ** -24
    truth = F.mse_loss(a.double(), b.double(), reduction=red).item()
    assert abs(R.mse_sum(a, b) * (1.0 / n if mean else 1.0) - truth) <= 3.1 * 2.0 ** -24 * abs(truth)
    for g in R.MSE_GOUTS:
        a2, b2 = a.clone().requires_grad_(), b.clone().requires_grad_()
        F.mse_loss(a2, b2, reduction=red).backward(torch.tensor(g))
        da, db = R.mse_bwd(a, b, g, mean)
        assert torch.equal(da.view(torch.int32), a2.grad.view(torch.int32)), (n, mean, g)
        assert torch.equal(db.view(torch.int32), b2.grad.view(torch.int32)), (n, mean, g)


def test_class_count_restatements():
    v = np.array([-100, -5, 0, 1, 3, 4, 255, 2 ** 40, -2 ** 63, 2], dtype=np.int64)
    assert AR.label_hist(v, 4, None).tolist() == [4, 1, 1, 4]
    assert AR.label_hist(v, 4, 255).tolist() == [4, 1, 1, 3]          # dropped before the clamp ...
    assert AR.label_hist(v, 4, 3).tolist() == [4, 1, 1, 3]            # ... so ignoring 3 keeps the clamped 4, 255 and 2^40
    assert AR.label_hist(v, 4, -100).tolist() == [3, 1, 1, 4]
    assert AR.label_hist(v, 1, None).tolist() == [10]
    assert np.array_equal(AR.class_weights([v, v], 4, 255)[0], 2 * AR.label_hist(v, 4, 255))
    got = AR.rgb_classes(np.array(AR.RGB_COLOURS, dtype=np.uint8))
    assert got.dtype == np.uint8 and got.tolist() == [0, 0, 1, 2] + [255] * (len(AR.RGB_COLOURS) - 4)


# ---- the case tables reach what they claim ---------------------------------------------------------------------------------
def test_score_cases_reach_every_lane_pass_and_row_remainder():
    passes, widths, heights, last_live, Ks, Bs, Rs, luts = set(), set(), set(), set(), set(), set(), set(), set()
    for c in P.SCORE_CASES:
        assert len(c.centres) == c.K
        Ks.add(c.K); Bs.add(c.B); Rs.add(c.R); luts.add(c.lut)
        w, nw = P.score_tables(c)
        assert len(w) == nw == (c.R ** 2 if c.nw_disc else 2 * c.R ** 2) + 1
        assert w[min(c.R ** 2, nw - 1)] >= np.exp(-2.0) - 1e-12            # the outer ring still carries weight
        for cy, cx in c.centres:
            if 0 <= cy < c.H and 0 <= cx < c.W:
                rows, cols, np_, live = P.score_window(cy, cx, c.R, c.H, c.W)
                passes.add(np_); widths.add(cols); heights.add(rows); last_live.add((np_, live))
    assert passes == {1, 2, 3}
    assert {1, 3, 63, 65, 127, 129} <= widths                              # whole windows of every R
    assert (2, 1) in last_live and (3, 1) in last_live                     # a pass with exactly one live lane
    assert set(range(1, 10)) <= heights and {h % 4 for h in heights} == {0, 1, 2, 3}
    assert {1, 3, 4, 5, 65} <= Ks and Bs == {1, 3} and Rs == {0, 1, 31, 32, 63, 64} and luts == {"none", "trimap", "wide"}
    assert sum(c.nw_disc for c in P.SCORE_CASES) == 1
    assert {(c.H, c.W) for c in P.SCORE_CASES} >= {(1, 1), (1, 200), (200, 1), (9, 40), (70, 200)}
    c = next(c for c in P.SCORE_CASES if c.name == "9x40-R32")             # clipped on every side
    wins = [P.score_window(cy, cx, c.R, c.H, c.W)[:2] for cy, cx in c.centres]
    assert all(r == 9 and k < 65 for r, k in wins) and (9, 40) in wins
    c = next(c for c in P.SCORE_CASES if c.name == "70x200-R32")           # fits whole, and hangs over each edge
    wins = {P.score_window(cy, cx, 32, 70, 200)[:2] for cy, cx in c.centres}
    assert (65, 65) in wins and (33, 33) in wins and any(r == 65 and k < 65 for r, k in wins) and any(r < 65 and k == 65 for r, k in wins)
    xs = {cx for _, cx in c.centres}
    assert {63, 65, 127, 129, 191, 193} <= xs
    c = next(c for c in P.SCORE_CASES if c.name == "70x200-outside")
    assert not any(0 <= cy < c.H and 0 <= cx < c.W for cy, cx in c.centres)


def test_score_inputs_hold_their_conditions():
    """from the restatement alone: no candidate's class choice is within twice the score bound of changing (1 % are allowed),
    every case but the one built so chooses a non-zero class somewhere, and the bad labels are in the scored windows"""
    total = unstable = 0
    seen_bad = set()
    for c in P.SCORE_CASES:
        lab, cen = P.score_inputs(c)
        w, nw = P.score_tables(c)
        seen_bad |= set(np.unique(lab).tolist()) & set(P.BAD_LABELS)
        any_class = False
        for b in range(c.B):
            ref, N, cls = P.scores(lab[b], P.LUTS[c.lut], cen[b], w, nw, c.R)
            st = P.stable(ref, N)
            total += len(st); unstable += int((~st).sum())
            any_class |= bool(cls.any())
            if c.nw_disc:                            # the disc really drops terms: fewer than the square holds
                full = [P.score_window(cy, cx, c.R, c.H, c.W) for cy, cx in cen[b].tolist()]
                assert all(n < r * k for n, (r, k, _, _) in zip(N.tolist(), full))
        assert any_class == (c.name not in P.ALL_ZERO_SCORE_CASES), c.name
    assert seen_bad == set(P.BAD_LABELS)
    assert unstable == 0 and total > 300, (unstable, total)


def test_make_and_heat_cases_reach_both_paths_and_every_k0_pass():
    paths = {P.vec_path(c.H, c.W) for c in P.MAKE_CASES}
    assert paths == {(False, False), (True, False), (True, True)}
    assert {(c.H, c.W) for c in P.MAKE_CASES} == set(P.MAKE_SHAPES)
    assert {P.vec_path(H, W) for H, W in [(1, 1), (3, 5), (33, 47)]} == {(False, False)}
    assert {P.vec_path(H, W) for H, W in [(8, 8), (16, 64)]} == {(True, False)}
    assert {P.vec_path(H, W) for H, W in [(2, 2), (4, 1), (4, 3), (4, 7), (12, 5), (6, 10), (4, 255), (4, 257)]} == {(True, True)}
    assert P.vec_path(1, 4) == (True, False)         # one row: its single vector cannot cross
    assert sorted(H * W for H, W in P.MAKE_SHAPES[-3:]) == [1020, 1024, 1028]
    assert {c.K for c in P.MAKE_CASES} == set(P.MAKE_KS) and {P.k0_passes(K) for K in P.MAKE_KS} == {1, 2, 3}
    assert {c.per_image for c in P.MAKE_CASES} == set(P.MAKE_PIS) and {c.nq for c in P.MAKE_CASES} == set(P.NQS)
    assert {c.lut for c in P.MAKE_CASES} == {"none", "trimap", "wide"}
    # every k0 pass count and per_image meets both the scalar and the crossing 16-byte path
    for vec in ((False, False), (True, True)):
        assert {P.k0_passes(c.K) for c in P.MAKE_CASES if P.vec_path(c.H, c.W) == vec} == {1, 2, 3}, vec
    firsts, seven, skipped, junk = set(), 0, 0, set()
    for c in P.MAKE_CASES:
        lab, cen, cls, planted = P.make_inputs(c)
        junk |= set(cls.reshape(-1).tolist()) - set(range(1, 8))
        for b in range(3):
            heat, target, classes, oc, valid = P.make(lab[b], P.LUTS[c.lut], cen[b], cls[b], P.q_table(), c.nq, c.per_image)
            distinct = len(planted[b])
            assert valid == (distinct >= c.per_image)
            if b == 0:
                assert distinct == c.per_image and valid
            if b == 1:
                assert distinct == c.per_image - 1 and not valid and not heat.any() and not target.any() and not classes.any()
                skipped += 1
            if valid:                                # the taken candidates are the planted firsts, in candidate order
                want = sorted(planted[b])[:c.per_image]
                assert classes.tolist() == [cl for _, cl in want] and oc.tolist() == [cen[b][p].tolist() for p, _ in want]
                firsts |= {p if p < 1025 else "K-1" for p, _ in want if p in (0, 255, 256, 1023, 1024) or p == c.K - 1}
                seven += distinct == 7 and c.per_image == 7
    assert firsts >= {0, 255, 256, 1023, 1024, "K-1"} and seven >= 1 and skipped == len(P.MAKE_CASES)
    assert junk == {0, 8, -3, 2 ** 31 - 1}             # the classes that are ignored
    assert {c.P for c in P.HEAT_CASES} == set(P.HEAT_PS) and {(c.H, c.W) for c in P.HEAT_CASES} == set(P.MAKE_SHAPES)
    assert {c.kind for c in P.HEAT_CASES} == {"inside", "some outside", "all outside"}
    assert {P.vec_path(c.H, c.W) for c in P.HEAT_CASES if c.P == 1024} and {c.nq for c in P.HEAT_CASES} == set(P.NQS)
    for c in P.HEAT_CASES:
        pts = P.heat_points(c)
        assert pts.shape == (c.P, 2) and pts.dtype == np.int32
        inside = (pts[:, 0] >= 0) & (pts[:, 0] < c.H) & (pts[:, 1] >= 0) & (pts[:, 1] < c.W)
        assert {"inside": inside.all(), "some outside": c.P < 2 or (inside.any() and not inside.all()),
                "all outside": not inside.any()}[c.kind]
        assert c.P < 3 or len(np.unique(pts, axis=0)) < c.P                # duplicates
        assert P.heatmap(pts, P.q_table(), c.nq, c.H, c.W).any() == bool(inside.any())
    big = [c for c in P.HEAT_CASES if c.P > 256]
    assert any((P.heat_points(c)[256:] >= 0).all(1).any() for c in big)    # the staging slices u >= 1 hold live points


def test_mse_and_label_count_launches():
    assert {R.mse_blocks(n) for n in R.MSE_FWD_N} >= {1, 2, 256, 257, 511, 512}
    assert R.mse_blocks(1) == 1 and R.mse_blocks(4096) == 1 and R.mse_blocks(4097) == 2 and R.mse_blocks(10 ** 9) == 512
    assert 2 * R.mse_blocks(10 ** 12) == 1024                              # SEGK_MSE_PART_FLOATS suffices for every n
    assert R.mse_passes(512 * 4096) == (2, 512 * 256 * 8) and R.mse_passes(512 * 4096 + 1) == (3, 1)
    assert R.mse_passes(3 * 512 * 4096 + 5) == (7, 5)
    assert all(R.mse_passes(n)[0] <= 2 for n in R.MSE_FWD_N if n <= 512 * 4096)
    assert [R.mse_bwd_passes(n) for n in R.MSE_BWD_N[-2:]] == [1, 2] and R.MSE_BWD_N[-1] > 16384 * 256
    opts = {o for i in range(len(R.MSE_BWD_N)) for o in R.mse_bwd_options(i)}
    assert {o[0] for o in opts} == set(R.MSE_GOUTS) and {o[1:] for o in opts} == {(0, True), (0, False), (1, True), (1, False)}
    assert R.MSE_MAX_N * 4 <= 26 * 10 ** 6                                 # the largest MSE buffer: 25 MB
    assert AR.hist_launch(1) == (1, 1) and AR.hist_launch(4096) == (1, 4) and AR.hist_launch(4097) == (2, 3)
    assert AR.hist_launch(1024 * 4096) == (1024, 4)                        # 1024 workgroups exactly
    assert AR.hist_launch(1024 * 4096 + 1) == (1024, 5) and AR.hist_launch(1024 * 4096 + 4097) == (1024, 5)    # the stride past the cap
    cases = AR.hist_cases()
    for eb in (1, 8):
        mine = [c for c in cases if c[0] == eb]
        assert [c[1] for c in mine] == AR.HIST_N and {c[2] for c in mine} == set(AR.HIST_CLASSES)
        modes = {"none" if ign is None else "255 at C=4" if (ign, C) == (255, 4) else "-100" if ign == -100 else "inside"
                 for _, _, C, ign in mine}
        assert modes == ({"none", "inside", "255 at C=4"} | ({"-100"} if eb == 8 else set()))
        assert all(ign is None or ign in (255, -100) or 0 <= ign < C for _, _, C, ign in mine)
    m = AR.hist_labels(8, 5000)
    v = AR.hist_case_labels(m, 5000, 21)
    assert {-100, -5, 21, 2 ** 40, -2 ** 63} <= set(v.tolist()) and 300 not in v
    # the order matters on these inputs: clamping before the ignore test gives other counts
    for C, ign in ((4, 255), (21, 20), (4, 3)):
        v = AR.hist_case_labels(m, 5000, C)
        wrong = np.bincount(np.clip(v, 0, C - 1)[np.clip(v, 0, C - 1) != min(max(ign, 0), C - 1)], minlength=C)
        assert not np.array_equal(AR.label_hist(v, C, ign), wrong), (C, ign)
    assert AR.HIST_N[-1] * 8 <= 34 * 10 ** 6                               # the largest label buffer: 33 MB
    px = AR.rgb_pixels(257)
    assert px.shape == (257, 3) and px.dtype == np.uint8 and {tuple(p) for p in px.tolist()} == set(AR.RGB_COLOURS)


# ---- recon forward: the cases and what their inputs must show --------------------------------------------------------------
def test_head_cases_cover_both_lists_in_both_dtypes():
    for dtype in ("fp32", "bf16"):
        mine = [c for c in R.HEAD_CASES if c.dtype == dtype]
        assert {c.Cin for c in mine} == set(R.HEAD_CINS) and {c.Cout for c in mine} == set(R.HEAD_COUTS)
        assert {(c.B, c.H, c.W) for c in mine} == set(R.HEAD_SHAPES)
        assert {c.bias for c in mine} == {True, False}
        assert any(c.Cp == 64 and c.Cin == 8 for c in mine) and all(c.Cp == R.pad32(c.Cin) or c.Cin == 8 for c in mine)
        for H, W in ((1, 1), (65, 31)):
            assert any(c.Cin % 2 for c in mine if (c.H, c.W) == (H, W)), (H, W)
    assert len({R.head_case_id(c) for c in R.HEAD_CASES}) == len(R.HEAD_CASES)
    # chunks of 8 fp32 / 16 bf16 channels: Cin below one chunk, a last chunk that is full, partly real, and half a pair
    f = {Cin: R.head_chunks(Cin, "fp32") for Cin in R.HEAD_CINS}
    b = {Cin: R.head_chunks(Cin, "bf16") for Cin in R.HEAD_CINS}
    assert f[7][:2] == (1, 7) and f[8][:2] == (1, 8) and f[9][:2] == (2, 1) and f[33][:2] == (5, 1) and f[40][:2] == (5, 8)
    assert b[1] == (1, 1, True) and b[15] == (1, 15, True) and b[16] == (1, 16, False) and b[17] == (2, 1, True)
    assert b[33] == (3, 1, True) and b[40] == (3, 8, False) and b[96] == (6, 16, False)
    assert R.gamma(9 * 96 + 1) < 5.2e-5


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_case_id)
def test_head_inputs_show_a_dropped_channel_tap_or_bias(case):
    """removing the last input channel, tap (2,2) or the bias moves some output by more than 8 times that output's allowed
    error: a dropped pair, chunk tail or tap cannot hide inside the bound.  A 1x1 image reads only the centre tap (every other
    tap lies in the zero halo), so there the centre tap stands in for tap (2,2)."""
    c = case
    xa, w, b = R.head_inputs(c)
    assert not xa[..., c.Cin:].any()                   # the header's contract: padding channels are zero
    rec, S, z = R.head(xa, w, b, c.dtype)
    bound = R.head_bound(S, z, c.Cin)
    assert 0 < R.d_sig(z) < 2.0 ** -22 and float(bound.max()) < 2e-4

    def moved(w2, b2):
        return float(((R.head(xa, w2, b2, c.dtype)[0] - rec).abs() / bound).max())
    w2 = w.clone(); w2[:, c.Cin - 1] = 0
    assert moved(w2, b) > 8, "last channel"
    ty, tx = (1, 1) if (c.H, c.W) == (1, 1) else (2, 2)
    w2 = w.clone(); w2[:, :, ty, tx] = 0
    assert moved(w2, b) > 8, "tap"
    if c.bias:
        assert moved(w, None) > 8, "bias"
