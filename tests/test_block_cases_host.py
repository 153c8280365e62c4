"""CPU: the case table of the block matrix (tests/block_cases.py) and its float64 reference (tests/block_reference.py).

  * the reference restated from functional ops (BatchNorm written out) equals the oracle's modules in float64 to 1e-12;
  * every case passes both guards (no ReLU and no pooling route within 1e-4 RMS of a tie);
  * every host predicate the DoubleConvFn node branches on is true in one case and false in another (asked of the library
    itself, so a retuned dispatch rule that takes a branch out of the table fails here);
  * the yardstick: the oracle's own fp32 evaluation of every case sits within 5e-6 (relative L2, every tensor) of float64 --
    a condition on the INPUTS (a noisier case is badly conditioned and gets another seed or shape in the table), and the
    unit tests/test_gpu_block_matrix.py measures the device in."""
import functools

import pytest
import torch

import block_cases as K
import block_reference as R

DC_CASES = [c for c in K.CASES if c.form in K.DC_FORMS]
ids = lambda cs: [c.id for c in cs]          # noqa: E731


@functools.lru_cache(maxsize=None)
def ref64(c):
    return R.evaluate(c)[0]


def test_table_is_complete():
    assert len({c.id for c in K.CASES}) == len(K.CASES)
    forms = {c.form for c in K.CASES}
    assert forms == set(K.DC_FORMS) | set(K.NODE_FORMS)
    for f in K.DC_FORMS:                                   # every DoubleConv form in both modes
        assert {c.mode for c in K.CASES if c.form == f} == {"train", "eval"}, f
    for f in K.HEAD_FORMS:                                 # the head on the pre-activation and on the block output, both modes
        assert {(c.mode, c.on_z) for c in K.CASES if c.form == f} >= {(m, z) for m in ("train", "eval") for z in (True, False)}
    assert {c.grads for c in DC_CASES} == {"all", "nox", "nox2", "xonly"}
    assert any(c.grads == "nox2" for c in K.CASES if c.form in ("up", "up_head"))
    assert any(not c.bias and c.form == "plain" and c.mode == "train" for c in K.CASES)
    assert any(not c.bias and c.mode == "eval" for c in DC_CASES)
    for c in K.CASES:
        assert c.B in (1, 2) and max(c.CA + c.CB, c.Cout, c.classes) <= 128 and c.H * c.W <= 24 * 40, c.id
        if c.form in K.DC_FORMS:
            assert (c.H, c.W) in {(16, 16), (24, 40), (16, 32), (18, 22), (17, 22)}, c.id
    assert any(c.H % 2 == 1 for c in K.CASES if c.form in K.POOL_FORMS + ("down_handed", "down_self", "maxpool"))
    assert {c.Cout for c in DC_CASES} >= {8, 40, 64, 96}
    # the stand-alone nodes: one case per needs_input_grad pattern each branches on
    assert {c.grads for c in K.CASES if c.form == "convt"} >= {"all", "nox"}
    assert {c.grads for c in K.CASES if c.form == "conv1x1"} >= {"all", "nox"}
    assert {c.grads for c in K.CASES if c.form == "recon"} >= {"all", "nox", "xonly"}
    for name, factors in K.FACTORS.items():
        assert name in {c.id for c in K.CASES}
        assert all(3 < f <= 16 and len(why) > 20 for f, why in factors.values()), name


@pytest.mark.parametrize("case", DC_CASES, ids=ids(DC_CASES))
def test_functional_restatement_equals_oracle_modules(case):
    ref = ref64(case)
    fun, _ = R.evaluate(case, torch.float64, R.Functional())
    assert list(fun) == list(ref)
    for n in ref:
        scale = max(1.0, ref[n].abs().max().item())
        assert (fun[n] - ref[n]).abs().max().item() <= 1e-12 * scale, (case.id, n)


@pytest.mark.parametrize("case", K.CASES, ids=ids(K.CASES))
def test_guards(case):
    g_bn, g_pool = R.guards(case)
    assert g_bn > 1e-4, f"{case.id}: a BatchNorm output {g_bn:.2e} RMS from its ReLU's kink -- change the seed"
    assert g_pool > 1e-4, f"{case.id}: a pooling window decided by {g_pool:.2e} RMS -- change the seed"


def test_every_predicate_takes_both_values():
    from image_segmentation_amd import _lib
    seen = {}
    for c in K.CASES:
        for dt, dn in ((K.F32, "fp32"), (K.BF16, "bf16")):
            for pred, val in K.predicates(c, dt, _lib.query).items():
                seen.setdefault(pred, {True: [], False: []})[val].append(f"{c.id} [{dn}]")
    assert set(seen) == {"second_operand", "cout_multiple_of_32", "conv_writes_act", "pool_bwd_stat_blocks", "stem_rows",
                         "stem_wgrad_slabs"}
    for pred, by in sorted(seen.items()):
        print(f"{pred}: true in {len(by[True])} runs (e.g. {by[True][:1]}), false in {len(by[False])} (e.g. {by[False][:1]})")
        assert by[True] and by[False], (pred, "takes one value only: the table lost a branch")
    # ... and within one compute dtype where the rule can go either way there (fp32 has no stem kernel and no act-writing conv)
    for pred, dn in (("conv_writes_act", "bf16"), ("stem_rows", "bf16"), ("pool_bwd_stat_blocks", "bf16"),
                     ("pool_bwd_stat_blocks", "fp32")):
        assert all(any(r.endswith(f"[{dn}]") for r in seen[pred][v]) for v in (True, False)), (pred, dn)
    # the stem predicates are true in a case whose input needs no gradient and in one where it does (two ways to keep x)
    stem = [c for c in K.CASES if K.predicates(c, K.BF16, _lib.query).get("stem_rows")]
    assert {c.grads for c in stem} >= {"all", "nox"} and {c.mode for c in stem} == {"train", "eval"}
    # the fused pooling reductions decline in both dtypes at the same widths, and are asked for in fp32 (the float64 gate)
    assert any(not K.predicates(c, K.F32, _lib.query).get("pool_bwd_stat_blocks", True) for c in K.CASES)


def test_fp32_yardstick():
    worst = (0.0, None, None)
    for c in K.CASES:
        d = R.distances(c, R.evaluate(c, torch.float32)[0], ref64(c))
        n = max(d, key=d.get)
        worst = max(worst, (d[n], c.id, n))
        assert d[n] <= 5e-6, f"{c.id}: the oracle's own fp32 run is {d[n]:.2e} from float64 in {n} -- change the seed or shape"
    print(f"yardstick: fp32 oracle within {worst[0]:.2e} of float64 over {len(K.CASES)} cases (worst {worst[1]}: {worst[2]})")
