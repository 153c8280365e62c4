"""CPU: the host half of seg.AdamW.

  * the float32 restatement (tests/optim_reference.py) against stock torch.optim.AdamW on float64 parameters, with stock
    float32 CPU AdamW as the yardstick: e_64 <= 3 e_o + 1e-7, plain, with clipping and with the EMA;
  * the chunk / block arithmetic of the table builder and the byte images the kernels read;
  * every refusal; state_dict round trips with torch.optim.AdamW in both directions.
No kernel is launched."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import optim_reference as R

SHAPES = [(1,), (3,), (7, 5), (4, 3, 3), (33,), (2, 2)]
GROUP_OF = [0, 1, 0, 1, 0, 1]
GROUPS = [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01},
          {"lr": 3e-3, "betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.0}]
STEPS = 5


def _data(scale=1.0):
    rng = np.random.default_rng(7)
    params = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    grads = [[(scale * rng.standard_normal(s)).astype(np.float32) for s in SHAPES] for _ in range(STEPS)]
    return params, grads


def _stock(params, grads, dtype, max_norm=None, ema_decay=None):
    ps = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in params]
    opt = torch.optim.AdamW([dict(GROUPS[k], params=[p for p, g in zip(ps, GROUP_OF) if g == k]) for k in (0, 1)], foreach=False)
    shadows = [p.detach().clone() for p in ps] if ema_decay is not None else None
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = torch.tensor(g, dtype=dtype)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
        if shadows is not None:
            for s, p in zip(shadows, ps):
                s.lerp_(p.detach(), 1.0 - ema_decay)
    out = [p.detach().double().numpy() for p in ps]
    return out, ([s.double().numpy() for s in shadows] if shadows is not None else None)


def _dist(a, b):
    return max(float(np.abs(np.asarray(x, np.float64) - y).max()) for x, y in zip(a, b))


@pytest.mark.parametrize("max_norm,ema_decay,scale", [(None, None, 1.0), (1.0, None, 1.0), (1.0, None, 1e-3), (None, 0.9, 1.0)])
def test_restatement_tracks_float64_adamw_like_stock_float32_does(max_norm, ema_decay, scale):
    params, grads = _data(scale)
    p64, s64 = _stock(params, grads, torch.float64, max_norm, ema_decay)
    p32, s32 = _stock(params, grads, torch.float32, max_norm, ema_decay)
    mine = [p.copy() for p in params]
    _, _, shadows, state = R.run_f32(mine, grads, GROUP_OF, GROUPS, max_norm, ema_decay)
    assert state.t == STEPS
    e_o, e_64 = _dist(p32, p64), _dist(mine, p64)
    print(f"parameters: e_o {e_o:.3e} e_64 {e_64:.3e}")
    assert e_64 <= 3 * e_o + 1e-7
    if ema_decay is not None:
        e_o, e_64 = _dist(s32, s64), _dist(shadows, s64)
        print(f"shadow: e_o {e_o:.3e} e_64 {e_64:.3e}")
        assert e_64 <= 3 * e_o + 1e-7


def test_yardstick_float64_adamw_is_stock_float64_adamw():
    params, grads = _data()
    p64, s64 = _stock(params, grads, torch.float64, None, 0.9)
    ps = [p.astype(np.float64) for p in params]
    ms, vs, ss = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps], [p.copy() for p in ps]
    for t, step in enumerate(grads, 1):
        for j, g in enumerate(step):
            gr = GROUPS[GROUP_OF[j]]
            R.adamw_f64(ps[j], g.astype(np.float64), ms[j], vs[j], ss[j], gr["lr"], gr["betas"], gr["eps"], gr["weight_decay"], t,
                        ema_decay=0.9)
    assert _dist(ps, p64) < 1e-12 and _dist(ss, s64) < 1e-12


def test_clip_coefficient_regimes():
    assert R.clip_coef(10.0, None) == np.float32(1.0)
    assert R.clip_coef(0.0, 1.0) == np.float32(1.0)                        # a norm of 0: 1 / 1e-6 is clamped to 1
    assert R.clip_coef(0.5, 1.0) == np.float32(1.0)
    assert R.clip_coef(4.0, 1.0) == np.float32(1.0 / (4.0 + 1e-6)) < 1
    assert R.clip_coef(float("inf"), 1.0) == 0.0 and np.isnan(R.clip_coef(float("nan"), 1.0))


def test_table_blocks_and_records():
    from image_segmentation_amd import optim, _lib
    C = optim.CHUNK
    assert C == R.CHUNK == _lib.OPTIM_CHUNK
    numels = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 7 * C]
    block0, total = optim.table_blocks(numels)
    want = [1, 1, 1, 1, 1, 1, 2, 3, 7]
    assert total == sum(want) and block0 == [sum(want[:i]) for i in range(len(want))]
    assert all(b > a for a, b in zip(block0, block0[1:]))                  # strictly monotone: every tensor owns a block
    for n, b0, nb in zip(numels, block0, want):                            # the last block of a tensor is never empty
        assert (nb - 1) * C < n <= nb * C
    with pytest.raises(ValueError):
        optim.table_blocks([4, 0])
    rows = [(0x1000 + 64 * i, 0x2000, 0x3000, 0x4000, 0x5000 if i % 2 else 0, n, i % 2) for i, n in enumerate(numels)]
    tab, tot = optim.build_table(rows)
    assert tot == total and ctypes.sizeof(_lib.OptimRec) == 64 and ctypes.sizeof(_lib.OptimGroup) == 64
    raw = bytes(tab)
    for i, (row, b0) in enumerate(zip(rows, block0)):                      # segk_optim_rec of include/segk.h, field by field
        p, g, m, v, s, n, b, grp = struct.unpack_from("<5QqiI", raw, 64 * i)
        assert (p, g, m, v, s, n, grp) == row and b == b0


def test_group_and_state_images():
    from image_segmentation_amd import optim
    g = dict(GROUPS[0])
    raw = optim.group_scalars(g, 0.99)
    f = struct.unpack_from("<8f2d", raw)
    k = R.group_scalars(g["lr"], g["betas"], g["eps"], g["weight_decay"], 0.99)
    assert len(raw) == 64
    assert [np.float32(x) for x in f[:8]] == [k[n] for n in ("lr", "decay", "omb1", "b2", "omb2", "eps", "omd", "ema_decay")]
    assert f[8:] == (0.9, 0.999)
    img = optim.state_bytes(3, [(0.9 ** 3, 0.5), (0.25, 0.125)])
    assert len(img) == 32 + 2 * (8 + 16 * 2)
    assert struct.unpack_from("<dfii", img) == (0.0, 1.0, 1, 0)
    assert struct.unpack_from("<i4x4d", img, 32) == struct.unpack_from("<i4x4d", img, 32 + 40) == (3, 0.9 ** 3, 0.5, 0.25, 0.125)
    assert optim._running_product(0.9, 3) == 0.9 * 0.9 * 0.9 == R.StepState(1).pows[0][0] * 0.9 * 0.9 * 0.9


def _params(dtype=torch.float32):
    return [torch.nn.Parameter(torch.arange(6, dtype=dtype).reshape(2, 3) / 7), torch.nn.Parameter(torch.ones(5, dtype=dtype))]


@pytest.mark.parametrize("kwargs,word", [({"amsgrad": True}, "amsgrad"), ({"maximize": True}, "maximize"),
                                         ({"capturable": True}, "capturable"), ({"max_grad_norm": 0.0}, "max_grad_norm"),
                                         ({"max_grad_norm": -1.0}, "max_grad_norm"), ({"ema_decay": 0.0}, "ema_decay"),
                                         ({"ema_decay": 1.0}, "ema_decay"), ({"ema_decay": 1.5}, "ema_decay")])
def test_constructor_refusals_name_the_argument(kwargs, word):
    import image_segmentation_amd as seg
    with pytest.raises(ValueError, match=word):
        seg.AdamW(_params(), **kwargs)


def test_other_refusals():
    import image_segmentation_amd as seg
    with pytest.raises(ValueError, match="dtype"):
        seg.AdamW(_params(torch.bfloat16))
    ps = _params()
    opt = seg.AdamW(ps, ema_decay=0.9)
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="re-entrant"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with seg.AdamW(_params()).ema_weights():
            pass


def test_is_an_optimizer_with_stock_layout_and_schedulers():
    import image_segmentation_amd as seg
    ps = _params()
    opt = seg.AdamW([{"params": [ps[0]]}, {"params": [ps[1]], "lr": 1e-2, "weight_decay": 0.0, "betas": (0.8, 0.9)}])
    assert isinstance(opt, torch.optim.Optimizer)
    stock = torch.optim.AdamW([{"params": [ps[0]]}, {"params": [ps[1]], "lr": 1e-2, "weight_decay": 0.0, "betas": (0.8, 0.9)}])
    for mine, theirs in zip(opt.state_dict()["param_groups"], stock.state_dict()["param_groups"]):
        assert set(mine) == set(theirs) | {"bias_products"}
        assert all(mine[k] == theirs[k] for k in theirs)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.5)
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 5e-3]


@pytest.mark.parametrize("ema", [False, True])
def test_state_dict_round_trips_with_stock_adamw(ema):
    import image_segmentation_amd as seg
    ps = _params()
    stock = torch.optim.AdamW(ps, lr=2e-3)
    for _ in range(3):
        for p in ps:
            p.grad = torch.full_like(p, 0.25)
        stock.step()
    sd = stock.state_dict()
    mine = seg.AdamW(ps, ema_decay=0.9 if ema else None)
    mine.load_state_dict(sd)                                   # stock -> seg: no "ema" in it
    assert mine._host_state == (3, None) and mine.param_groups[0]["lr"] == 2e-3
    back = mine.state_dict()
    assert back["param_groups"][0]["bias_products"] == [0.9 * 0.9 * 0.9, 0.999 * 0.999 * 0.999]
    for i in (0, 1):
        assert set(back["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} and float(back["state"][i]["step"]) == 3.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][k], sd["state"][i][k])
    if ema:                                                     # a shadow, as a step would have left it
        for p in ps:
            mine.state[p]["ema"] = p.detach().clone() * 0.5
        back = mine.state_dict()
        assert all(set(back["state"][i]) == {"step", "exp_avg", "exp_avg_sq", "ema"} for i in (0, 1))
        again = seg.AdamW(ps, ema_decay=0.9)
        again.load_state_dict(back)                             # seg -> seg keeps the shadow and the exact products
        assert again._host_state == (3, [(0.9 * 0.9 * 0.9, 0.999 * 0.999 * 0.999)])
        assert all(torch.equal(again.state[p]["ema"], p.detach() * 0.5) for p in ps)
        sdm = again.ema_state_dict(torch.nn.ParameterList(ps))
        assert all(torch.equal(sdm[str(i)], p.detach() * 0.5) for i, p in enumerate(ps))
    fresh = torch.optim.AdamW(ps, lr=1.0)
    fresh.load_state_dict(back)                                 # seg -> stock
    assert fresh.param_groups[0]["lr"] == 2e-3
    before = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = torch.full_like(p, 0.25)
    fresh.step()
    for p, b in zip(ps, before):
        p.data.copy_(b)
    stock.step()                                                # the original run's fourth step: the same update
    assert all(float(fresh.state[p]["step"]) == 4.0 for p in ps)
    assert all(torch.equal(fresh.state[p]["exp_avg"], stock.state[p]["exp_avg"]) for p in ps)


def test_optimizer_kernels_neither_spill_nor_serialise_their_loads():
    """Compiled-code check (hipcc cross-compiles here) of csrc/optim.hip: no spills, no scratch, and fewer than two loads
    that wait for themselves in any of its three kernels."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def tool(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    rows = tool("serialized_loads").scan("optim")
    assert len(rows) == 3 and all(n_ser < 2 and n_loads > 0 for n_ser, n_loads, _, _ in rows), rows
    rep = tool("spill_report").report("optim")
    assert len(rep) == 3 and all(int(r.get("VGPRs Spill", 0)) == 0 and int(r.get("ScratchSize", 0)) == 0 for r in rep), rep
