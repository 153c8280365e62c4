#!/usr/bin/env python3
"""Micro-benchmark of single kernels at U-Net layer shapes (B=32, 256x256 input): conv3x3 forward /
weight-gradient through the C ABI.  Usage: python tools/kbench.py [conv|wgrad|all] [--iters N]
(other families: ends, convt, bn, loss, head, recon, vit, stem, pack, predict, prompt, augment, perturb, components, vectors, tta, tiles, calib, distill, hardloss, lovasz, optim, raster, pq, morph, boundary, slic, mix)"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from image_segmentation_amd import _lib
if "--lib" in sys.argv:                      # diagnostic builds (ablation / stamp variants of libsegk.so)
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from image_segmentation_amd import ops

LAYERS = [  # name, Cin, Cout, HW   (B = 32)
    ("64->64@256", 64, 64, 256), ("128->64@256", 128, 64, 256), ("64->128@256(dgrad up4)", 64, 128, 256),
    ("128->128@128", 128, 128, 128), ("256->256@64", 256, 256, 64), ("512->512@32", 512, 512, 32),
    ("1024->1024@16", 1024, 1024, 16), ("3->64@256", 32, 64, 256),
    # the Cin != Cout layers of the U-Net (first conv of each block and the data gradients of those)
    ("64->128@128", 64, 128, 128), ("128->256@64", 128, 256, 64), ("256->512@32", 256, 512, 32), ("512->1024@16", 512, 1024, 16),
    ("1024->512@32", 1024, 512, 32), ("512->256@64", 512, 256, 64), ("256->128@128", 256, 128, 128),
    ("128->64@128(dgrad)", 128, 64, 128), ("256->128@64(dgrad)", 256, 128, 64), ("512->256@32(dgrad)", 512, 256, 32),
    ("1024->512@16(dgrad)", 1024, 512, 16), ("512->1024@32(dgrad)", 512, 1024, 32), ("256->512@64(dgrad)", 256, 512, 64),
    ("128->256@128(dgrad)", 128, 256, 128),
]


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", type=str, default="")
    ap.add_argument("--pro", action="store_true")
    ap.add_argument("--no-stats", action="store_true", help="conv without the BatchNorm statistics epilogue")
    ap.add_argument("--lib", type=str, default="")
    ap.add_argument("--list", type=str, default="", help="write the layers that ran (name|cin|cout|hw per line) to this file")
    ap.add_argument("--stamps", action="store_true", help="with the stamp build (tools/stamp_build.sh): print the conv_rs "
                    "kernel's per-phase cycle shares (read from the statistics buffer the diagnostic build overwrites)")
    args = ap.parse_args()
    dt = torch.bfloat16
    B = 32
    ran = []
    for name, cin, cout, hw in LAYERS:
        if args.only and args.only not in name:
            continue
        ran.append(f"{name}|{cin}|{cout}|{hw}")
        if args.list:
            open(args.list, "w").write("\n".join(ran) + "\n")
        x = torch.randn((B, hw, hw, cin), device="cuda").to(dt)
        g = torch.randn((B, hw, hw, cout), device="cuda").to(dt)
        w = torch.randn((cout, cin, 3, 3), device="cuda") / (3 * cin ** 0.5)
        wp = ops.pack_conv(w, cin, 0, dt, 0)
        out = torch.empty((B, hw, hw, cout), dtype=dt, device="cuda")
        sc = torch.rand(cin, device="cuda") + 0.5 if args.pro else None
        sh = torch.rand(cin, device="cuda") - 0.5 if args.pro else None
        fl = 2.0 * B * hw * hw * 9 * cin * cout
        by = B * hw * hw * (cin + cout) * 2
        if args.what in ("conv", "all"):
            tiles = _lib.query("segk_conv_tiles", B, hw, hw, cin, cout, 1)
            st = torch.empty((_lib.query("segk_bn_stats_floats", tiles, cout),), dtype=torch.float32, device="cuda")
            us = timeit(lambda: ops.conv3x3(x, x.data_ptr(), cin, 0, 0, wp, out.data_ptr(), cout, 0, 0, B, hw, hw, dt,
                                            scale=sc, shift=sh, stats=None if args.no_stats else st), args.iters)
            print(f"conv  {name:26s} {us:8.1f} us  {fl/us/1e6:7.1f} TF/s  {by/us/1e3:7.1f} GB/s(alg)")
            if args.stamps:
                torch.cuda.synchronize()
                n = min(st.numel() // 2, 256 * 8 * 8)
                t = st[:2 * n].view(torch.int64).view(-1, 8, 8).double().cpu()       # [workgroup][wave][8]
                tot = t[:, :, 6].clamp(min=1)
                names = ["barrier wait", "MFMA loop", "DMA issue", "wait next tile", "epilogue", "loop tail/transform"]
                if cin >= 128:
                    # conv3x3_pipe_kernel (waves 0-3 consumers, 4-7 producers)
                    names = ["step work (MFMA | staging)", "step barrier wait", "stage tile | E1 wait", "store tile",
                             "E2..E3 (refill)", "prologue"]
                    if not args.pro:                                                  # LDS-DMA form (no prologue)
                        names = ["step work (MFMA | DMA issue)", "step barrier wait", "direct epilogue | vmcnt wait", "-",
                                 "zero + first reads", "prologue"]
                print(f"      stamps over {t.shape[0]} workgroups: kernel {tot.mean():.0f} cycles per wave (min {tot.min():.0f} max {tot.max():.0f})")
                for i, nm in enumerate(names):
                    sh = (t[:, :, i] / tot)
                    print(f"        {nm:22s} {100*sh.mean():5.1f} %   waves0-3 {100*sh[:, :4].mean():5.1f} %  waves4-7 {100*sh[:, 4:].mean():5.1f} %   "
                          f"({t[:, :, i].mean():.0f} cycles)")
        if args.what in ("wgrad", "all"):
            def f():
                ops.wgrad(g.data_ptr(), cout, x.data_ptr(), cin, 0, 0, B, hw, hw, 0, dt, "cuda", scale=sc, shift=sh)
            us = timeit(f, args.iters)
            print(f"wgrad {name:26s} {us:8.1f} us  {fl/us/1e6:7.1f} TF/s  {by/us/1e3:7.1f} GB/s(alg)")
            if args.stamps:      # stamp build: wgrad_dma_kernel wrote per-wave phase cycle sums over the head of the slab buffer
                slabs, _ = ops.wgrad(g.data_ptr(), cout, x.data_ptr(), cin, 0, 0, B, hw, hw, 0, dt, "cuda", scale=sc, shift=sh)
                torch.cuda.synchronize()
                t = slabs[:256 * 8 * 8 * 2].view(torch.int64).view(-1, 8).double().cpu()
                t = t[(t[:, 4] > 0) & (t[:, 4] < 1e9)]
                tot = t[:, 4]
                for i, nm in enumerate(["DMA issue + MFMA rows", "wait for the next tile's DMA", "barrier", "slab stores"]):
                    print(f"        {nm:30s} {100 * (t[:, i] / tot).mean():5.1f} %   ({t[:, i].mean():.0f} cycles of {tot.mean():.0f})")


def convt():
    """ConvTranspose2d(k=2,s=2) layers of the U-Net up path: forward, data gradient, weight gradient."""
    dt = torch.bfloat16
    B = 32
    for cin, cout, hw in [(1024, 512, 16), (512, 256, 32), (256, 128, 64), (128, 64, 128)]:
        x = torch.randn((B, hw, hw, cin), device="cuda").to(dt)
        dy = torch.randn((B, 2 * hw, 2 * hw, cout), device="cuda").to(dt)
        w = torch.randn((cin, cout, 2, 2), device="cuda") / cin ** 0.5
        wf, wd = ops.pack_convt(w, dt, 0), ops.pack_convt(w, dt, 1)
        out = torch.empty_like(dy)
        dx = torch.empty_like(x)
        by = B * hw * hw * (cin + 4 * cout) * 2
        fl = 2.0 * B * hw * hw * cin * 4 * cout
        s = torch.cuda.current_stream().cuda_stream
        t1 = timeit(lambda: _lib.call("segk_convt2x2_fwd", x.data_ptr(), wf.data_ptr(), 0, out.data_ptr(), B, hw, hw, cin,
                                      cout, 1, s), 20)
        t2 = timeit(lambda: _lib.call("segk_convt2x2_dgrad", dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, hw, hw, cin,
                                      cout, 1, s), 20)
        t3 = timeit(lambda: ops.wgrad(x.data_ptr(), cin, dy.data_ptr(), cout, 0, 0, B, hw, hw, 2, dt, "cuda"), 20)
        for nm, t in (("fwd", t1), ("dgrad", t2), ("wgrad", t3)):
            print(f"convt {nm:5s} {cin}->{cout}@{hw}  {t:8.1f} us  {fl/t/1e6:7.1f} TF/s  {by/t/1e3:7.1f} GB/s(alg)")


def bn():
    """BatchNorm+ReLU backward (reduce + finalize + apply) at the U-Net activation shapes through ops.py, then every entry of
    bn_pool.hip (finalize, apply, apply + pool, the three backward forms, pooling forward / backward / backward with the
    BatchNorm reductions, channel sum) through the C ABI at 64 ch x 256^2, 128 x 128^2 and 256 x 64^2, B = 32."""
    dt = torch.bfloat16
    B = 32
    for C, hw in [(64, 256), (128, 128), (256, 64), (512, 32), (1024, 16)]:
        P = B * hw * hw
        z = torch.randn((P, C), device="cuda").to(dt)
        dy = torch.randn((P, C), device="cuda").to(dt)
        dz = torch.empty_like(z)
        sc = torch.rand(C, device="cuda") + 0.5; sh = torch.rand(C, device="cuda") - 0.5
        mu = torch.zeros(C, device="cuda"); rs = torch.ones(C, device="cuda")
        t = timeit(lambda: ops.bn_relu_bwd(dy.data_ptr(), z.data_ptr(), dz.data_ptr(), sc, sh, mu, rs, P, C, dt, "cuda"), 20)
        by = 5.0 * P * C * 2
        print(f"bn_bwd C={C:5d}@{hw:3d}  {t:8.1f} us  {by/t/1e3:7.1f} GB/s (5 passes)")
    # every entry of bn_pool.hip through the C ABI at the workload's shapes: median [min..max] of five repeats of 20 launches
    st = ops._stream()
    for C, hw in [(64, 256), (128, 128), (256, 64)]:
        P, ho = B * hw * hw, hw // 2
        z = torch.randn((P, C), device="cuda").to(dt); dy = torch.randn((P, C), device="cuda").to(dt)
        y = torch.relu(z); dz = torch.empty_like(z); pooled = torch.empty((B * ho * ho, C), dtype=dt, device="cuda")
        dp = torch.randn((B * ho * ho, C), device="cuda").to(dt)
        sc = torch.rand(C, device="cuda") + 0.5; sh = torch.rand(C, device="cuda") - 0.5
        mu = torch.zeros(C, device="cuda"); rs = torch.ones(C, device="cuda")
        bnv = (sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr())
        ga = torch.ones(C, device="cuda"); be = torch.zeros(C, device="cuda"); rm = torch.zeros(C, device="cuda"); rv = torch.ones(C, device="cuda")
        o4 = [torch.empty(C, device="cuda") for _ in range(4)]
        coef = torch.empty(2 * C, device="cuda"); dga = torch.empty(C, device="cuda"); dbe = torch.empty(C, device="cuda")
        nb = _lib.query("segk_bn_bwd_blocks", P, C, 1)
        part = torch.rand(max(nb, 1024) * C * 2, device="cuda")
        MT = _lib.query("segk_conv_tiles", B, hw, hw, C, C, 1)
        stats = torch.rand(_lib.query("segk_bn_stats_floats", MT, C), device="cuda")
        nbp = _lib.query("segk_maxpool_bwd_stat_blocks", B, hw, hw, C, 1)
        ppart = torch.empty(nbp * C * 2, device="cuda"); csum = torch.empty(C, device="cuda")
        entries = [
            ("bn_finalize", lambda: _lib.call("segk_bn_finalize", stats.data_ptr(), MT, C, C, float(P), None, ga.data_ptr(), be.data_ptr(),
                                              rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, 1, *[o.data_ptr() for o in o4], st)),
            ("bn_relu_apply", lambda: _lib.call("segk_bn_relu_apply", z.data_ptr(), dz.data_ptr(), bnv[0], bnv[1], P, C, 1, st)),
            ("bn_relu_apply_pool", lambda: _lib.call("segk_bn_relu_apply_pool", z.data_ptr(), dz.data_ptr(), pooled.data_ptr(), bnv[0],
                                                     bnv[1], B, hw, hw, C, 1, st)),
            ("bn_relu_bwd", lambda: _lib.call("segk_bn_relu_bwd", dy.data_ptr(), z.data_ptr(), dz.data_ptr(), *bnv, P, C, C, part.data_ptr(),
                                              dga.data_ptr(), dbe.data_ptr(), coef.data_ptr(), 1, st)),
            ("bn_relu_bwd_stats", lambda: _lib.call("segk_bn_relu_bwd_stats", dy.data_ptr(), z.data_ptr(), *bnv, P, C, C, part.data_ptr(),
                                                    dga.data_ptr(), dbe.data_ptr(), coef.data_ptr(), 1, st)),
            ("bn_relu_bwd_from_part", lambda: _lib.call("segk_bn_relu_bwd_from_part", dy.data_ptr(), z.data_ptr(), dz.data_ptr(), *bnv, P,
                                                        C, C, part.data_ptr(), 1024, dga.data_ptr(), dbe.data_ptr(), coef.data_ptr(), 1, st)),
            ("maxpool2x2_fwd", lambda: _lib.call("segk_maxpool2x2_fwd", y.data_ptr(), pooled.data_ptr(), B, hw, hw, C, 1, st)),
            ("maxpool2x2_bwd", lambda: _lib.call("segk_maxpool2x2_bwd", y.data_ptr(), dp.data_ptr(), dz.data_ptr(), B, hw, hw, C, 0, 1, st)),
            ("maxpool2x2_bwd_bnstat", lambda: _lib.call("segk_maxpool2x2_bwd_bnstat", y.data_ptr(), dp.data_ptr(), dz.data_ptr(), B, hw, hw,
                                                        C, 0, *bnv, ppart.data_ptr(), None, 1, st)),
            ("channel_sum", lambda: _lib.call("segk_channel_sum", dy.data_ptr(), P, C, C, part.data_ptr(), csum.data_ptr(), 1, st)),
        ]
        for name, fn in entries:
            ts = sorted(timeit(fn, 20) for _ in range(5))
            print(f"{name:22s} C={C:4d}@{hw:3d}  {ts[2]:8.1f} us  [{ts[0]:.1f}..{ts[-1]:.1f}]", flush=True)


def loss():
    """Loss forward / backward (CrossEntropy and Dice+CE) through the C ABI at the bench batch: 32 x 3 x 256 x 256 logits."""
    N, C, H, W = 32, 3, 256, 256
    lg = torch.randn((N, C, H, W), device="cuda")
    tg = torch.randint(0, C, (N, H, W), device="cuda")
    part = torch.empty(_lib.query("segk_loss_part_floats", N * H * W), device="cuda")
    state = torch.empty(_lib.query("segk_loss_state_floats"), device="cuda")
    out = torch.empty(1, device="cuda"); go = torch.ones(1, device="cuda"); dl = torch.empty_like(lg)
    st = ops._stream()
    for name, dw, cw in (("ce", 0.0, 1.0), ("dice+ce", 1.0, 1.0)):
        f = lambda: _lib.call("segk_loss_fwd", lg.data_ptr(), tg.data_ptr(), None, N, C, H * W, -1, 1e-5, dw, cw,
                              part.data_ptr(), state.data_ptr(), out.data_ptr(), st)
        b = lambda: _lib.call("segk_loss_bwd", lg.data_ptr(), tg.data_ptr(), None, state.data_ptr(), go.data_ptr(), N, C,
                              H * W, -1, dw, cw, dl.data_ptr(), st)
        tf = timeit(f, 50); tb = timeit(b, 50)
        print(f"loss {name:8s} fwd {tf:7.1f} us ({N*H*W*(4*C+8)/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us ({N*H*W*(8*C+8)/tb/1e3:7.1f} GB/s)"
              f"   value {float(out):.6f}")


def distill():
    """Distillation loss forward / backward (segk_distill_fwd / _bwd) through the C ABI at the bench batch, 32 x C x 256 x 256, for
    C = 3, 4 and V = 1, 3 teacher views (T = 2, no labels), beside segk_loss_fwd / _bwd (CrossEntropy) at the same P and C and the
    stock-torch composition (softmax + flip per teacher, weighted sum, log_softmax, kl_div; its backward through autograd)."""
    import numpy as np
    import torch.nn.functional as F
    from image_segmentation_amd import distill as dmod
    N, H, W, T = 32, 256, 256, 2.0
    P = N * H * W
    st = ops._stream()
    for C in (3, 4):
        lg = torch.randn((N, C, H, W), device="cuda")
        tg = torch.randint(0, C, (N, H, W), device="cuda")
        part = torch.empty(_lib.query("segk_loss_part_floats", P), device="cuda")
        state = torch.empty(_lib.query("segk_loss_state_floats"), device="cuda")
        out = torch.empty(1, device="cuda"); go = torch.ones(1, device="cuda"); dl = torch.empty_like(lg)
        f = lambda: _lib.call("segk_loss_fwd", lg.data_ptr(), tg.data_ptr(), None, N, C, H * W, -1, 1e-5, 0.0, 1.0,
                              part.data_ptr(), state.data_ptr(), out.data_ptr(), st)
        b = lambda: _lib.call("segk_loss_bwd", lg.data_ptr(), tg.data_ptr(), None, state.data_ptr(), go.data_ptr(), N, C,
                              H * W, -1, 0.0, 1.0, dl.data_ptr(), st)
        tf = timeit(f, 50); tb = timeit(b, 50)
        print(f"loss ce    C={C}      fwd {tf:7.1f} us ({P*(4*C+8)/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us ({P*(8*C+8)/tb/1e3:7.1f} GB/s)")
        for V in (1, 3):
            ts = [torch.randn((N, C, H, W), device="cuda") for _ in range(V)]
            flips = [v % 4 for v in range(V)]
            host = dmod.teacher_table((t.data_ptr(), fl, 0, 1.0 + v) for v, (t, fl) in enumerate(zip(ts, flips)))
            table = torch.from_numpy(host.view(np.uint8).copy()).cuda()
            f = lambda: _lib.call("segk_distill_fwd", lg.data_ptr(), table.data_ptr(), V, None, N, C, H, W, 0, 1.0 / T, T * T, 0.0,
                                  part.data_ptr(), state.data_ptr(), out.data_ptr(), st)
            b = lambda: _lib.call("segk_distill_bwd", lg.data_ptr(), table.data_ptr(), V, None, state.data_ptr(), go.data_ptr(), N, C,
                                  H, W, 0, 1.0 / T, T * T, 0.0, dl.data_ptr(), st)
            tf = timeit(f, 50); tb = timeit(b, 50)
            val = float(out)
            w = [float(x) for x in host["weight"]]
            leaf = lg.clone().requires_grad_(True)

            def torch_fwd():
                q = 0
                for t, fl, wv in zip(ts, flips, w):
                    dims = [d for d, bit in ((3, 1), (2, 2)) if fl & bit]
                    p = torch.softmax(t / T, 1)
                    q = q + wv * (torch.flip(p, dims) if dims else p)
                return T * T * F.kl_div(F.log_softmax(leaf / T, 1), q, reduction="sum") / P

            def torch_both():
                leaf.grad = None
                torch_fwd().backward()
            with torch.no_grad():
                ttf = timeit(torch_fwd, 20)
            ttb = timeit(torch_both, 20) - ttf
            print(f"distill    C={C} V={V}  fwd {tf:7.1f} us ({P*4*C*(1+V)/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us ({P*4*C*(2+V)/tb/1e3:7.1f} GB/s)"
                  f"   value {val:.6f}   torch fwd {ttf:7.1f} us  bwd {ttb:7.1f} us  value {float(torch_fwd()):.6f}")


def hardloss():
    """Hard-pixel loss forward / backward (segk_hard_loss_fwd / _bwd) through the C ABI at the bench batch, 32 x 3 x 256 x 256, beside
    segk_loss_fwd / _bwd (CrossEntropy) in the same run: everything off; gamma = 2 with label_smoothing = 0.1; the selection on
    (thresh 0.7, min_fraction 0.25).  Bytes: forward P (4 C + 8), backward P (8 C + 8); the selection adds P (4 + 3 * 4 + 4 C + 8)
    forward (the words written once and read three times, one more pass over logits and labels) and 4 P backward."""
    import math
    N, C, H, W = 32, 3, 256, 256
    P = N * H * W
    lg = torch.randn((N, C, H, W), device="cuda")
    tg = torch.randint(0, C, (N, H, W), device="cuda")
    part = torch.empty(_lib.query("segk_loss_part_floats", P), device="cuda")
    state = torch.empty(_lib.query("segk_loss_state_floats"), device="cuda")
    out = torch.empty(1, device="cuda"); go = torch.ones(1, device="cuda"); dl = torch.empty_like(lg)
    keys = torch.empty(P, dtype=torch.int32, device="cuda")
    hist = torch.empty(ops.HARD_HIST_WORDS, dtype=torch.int32, device="cuda")
    st = ops._stream()
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 50
    f = lambda: _lib.call("segk_loss_fwd", lg.data_ptr(), tg.data_ptr(), None, N, C, H * W, -1, 1e-5, 0.0, 1.0,
                          part.data_ptr(), state.data_ptr(), out.data_ptr(), st)
    b = lambda: _lib.call("segk_loss_bwd", lg.data_ptr(), tg.data_ptr(), None, state.data_ptr(), go.data_ptr(), N, C,
                          H * W, -1, 0.0, 1.0, dl.data_ptr(), st)
    tf = timeit(f, iters); tb = timeit(b, iters)
    fb, bb = P * (4 * C + 8), P * (8 * C + 8)
    print(f"loss ce                    fwd {tf:7.1f} us ({fb/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us ({bb/tb/1e3:7.1f} GB/s)   value {float(out):.6f}")
    theta = -math.log(0.7)
    for name, eps, gamma, sel in (("all off", 0.0, 0.0, 0), ("gamma 2, smoothing 0.1", 0.1, 2.0, 0), ("selection on", 0.0, 0.0, 1)):
        f = lambda: _lib.call("segk_hard_loss_fwd", lg.data_ptr(), tg.data_ptr(), None, N, C, H * W, -1, eps, gamma, sel, theta, 0,
                              16384, keys.data_ptr(), hist.data_ptr(), part.data_ptr(), state.data_ptr(), out.data_ptr(), st)
        b = lambda: _lib.call("segk_hard_loss_bwd", lg.data_ptr(), tg.data_ptr(), None, keys.data_ptr() if sel else None,
                              state.data_ptr(), go.data_ptr(), N, C, H * W, -1, eps, gamma, sel, dl.data_ptr(), st)
        tf = timeit(f, iters); tb = timeit(b, iters)
        nf, nbw = fb + (P * (16 + 4 * C + 8) if sel else 0), bb + (4 * P if sel else 0)
        counts = state[6:8].view(torch.int32).tolist()
        print(f"hard {name:22s}fwd {tf:7.1f} us ({nf/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us ({nbw/tb/1e3:7.1f} GB/s)   value {float(out):.6f}"
              f"   n {counts[0]} kept {counts[1]}")


def lovasz():
    """Lovasz-Softmax forward / backward (segk_lovasz_fwd / _bwd) through the C ABI beside segk_loss_fwd / _bwd (CrossEntropy) and
    the hard-pixel selection in the same run, at the bench batch (32 x 3 x 256 x 256) and at config 5 (8 x 4 x 512 x 512), one
    segment per batch and one per image.  Forward: 1 keys launch, 4 x (histogram, scan, scatter), count, scan, terms = 16 launches;
    bytes P (4 C + 8) + C P (8 written by keys, 4 x (4 + 8 + 8 + 16) by the passes -- words read twice, payloads once, both
    written -- 8 by count, 8 + 4 by terms)."""
    import math
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 50
    st = ops._stream()
    for N, C, H, W in ((32, 3, 256, 256), (8, 4, 512, 512)):
        P = N * H * W
        lg = torch.randn((N, C, H, W), device="cuda")
        tg = torch.randint(0, C, (N, H, W), device="cuda")
        part = torch.empty(_lib.query("segk_loss_part_floats", P), device="cuda")
        state = torch.empty(_lib.query("segk_loss_state_floats"), device="cuda")
        out = torch.empty(1, device="cuda"); go = torch.ones(1, device="cuda"); dl = torch.empty_like(lg)
        keys = torch.empty(P, dtype=torch.int32, device="cuda")
        hist = torch.empty(ops.HARD_HIST_WORDS, dtype=torch.int32, device="cuda")
        f = lambda: _lib.call("segk_loss_fwd", lg.data_ptr(), tg.data_ptr(), None, N, C, H * W, -1, 1e-5, 0.0, 1.0,
                              part.data_ptr(), state.data_ptr(), out.data_ptr(), st)
        b = lambda: _lib.call("segk_loss_bwd", lg.data_ptr(), tg.data_ptr(), None, state.data_ptr(), go.data_ptr(), N, C,
                              H * W, -1, 0.0, 1.0, dl.data_ptr(), st)
        tf = timeit(f, iters); tb = timeit(b, iters)
        fb, bb = P * (4 * C + 8), P * (8 * C + 8)
        print(f"{N}x{C}x{H}x{W}  loss ce             fwd {tf:8.1f} us ({fb/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us ({bb/tb/1e3:7.1f} GB/s)"
              f"   value {float(out):.6f}")
        f = lambda: _lib.call("segk_hard_loss_fwd", lg.data_ptr(), tg.data_ptr(), None, N, C, H * W, -1, 0.0, 0.0, 1, -math.log(0.7),
                              0, 16384, keys.data_ptr(), hist.data_ptr(), part.data_ptr(), state.data_ptr(), out.data_ptr(), st)
        b = lambda: _lib.call("segk_hard_loss_bwd", lg.data_ptr(), tg.data_ptr(), None, keys.data_ptr(), state.data_ptr(),
                              go.data_ptr(), N, C, H * W, -1, 0.0, 0.0, 1, dl.data_ptr(), st)
        tf = timeit(f, iters); tb = timeit(b, iters)
        print(f"{N}x{C}x{H}x{W}  hard selection on   fwd {tf:8.1f} us ({(fb + P*(16+4*C+8))/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us"
              f" ({(bb+4*P)/tb/1e3:7.1f} GB/s)   value {float(out):.6f}")
        for per_image in (0, 1):
            S = N if per_image else 1
            nbytes = ops.lovasz_scratch_bytes(C, P, S)
            scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
            coef = torch.empty((C, P), device="cuda")
            lstate = torch.empty(ops.lovasz_state_doubles(C, S), dtype=torch.float64, device="cuda")
            f = lambda: _lib.call("segk_lovasz_fwd", lg.data_ptr(), tg.data_ptr(), None, N, C, H * W, -1, per_image, 0,
                                  scratch.data_ptr(), nbytes, coef.data_ptr(), lstate.data_ptr(), out.data_ptr(), st)
            b = lambda: _lib.call("segk_lovasz_bwd", lg.data_ptr(), tg.data_ptr(), coef.data_ptr(), lstate.data_ptr(), go.data_ptr(),
                                  N, C, H * W, -1, per_image, dl.data_ptr(), st)
            tf = timeit(f, iters); tb = timeit(b, iters)
            nf, nbw = fb + C * P * (8 + 4 * 36 + 8 + 12), P * (12 * C + 8)
            print(f"{N}x{C}x{H}x{W}  lovasz per_image={per_image}  fwd {tf:8.1f} us ({nf/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us"
                  f" ({nbw/tb/1e3:7.1f} GB/s)   value {float(out):.6f}   scratch {nbytes/2**20:.1f} MiB   n {int(lstate[1].item())}")


def head():
    """Output head on the pre-activation of the last block (forward: BN+ReLU + 1x1 conv to 3 classes; backward incl. the
    BatchNorm reductions) through the C ABI at the bench shape: B = 32, 64 channels, 256 x 256."""
    B, C, H, W, ncls = 32, 64, 256, 256, 3
    dt = torch.bfloat16
    P = B * H * W
    z = torch.randn((P, C), device="cuda").to(dt)
    w = torch.randn((ncls, C), device="cuda") / 8; b = torch.zeros(ncls, device="cuda")
    sc = torch.rand(C, device="cuda") + 0.5; sh = torch.rand(C, device="cuda") - 0.5
    mu = torch.zeros(C, device="cuda"); rs = torch.ones(C, device="cuda")
    logits = torch.empty((B, ncls, H, W), device="cuda"); dl = torch.randn_like(logits)
    dy = torch.empty_like(z)
    part = torch.empty(_lib.query("segk_head_part_floats", P, C), device="cuda")
    nb = _lib.query("segk_head_bwd_blocks", P)
    bnpart = torch.empty(nb * C * 2, device="cuda"); dw = torch.empty((ncls, C), device="cuda"); db = torch.empty(ncls, device="cuda")
    st = ops._stream()
    f = lambda: _lib.call("segk_head_fwd_bn", z.data_ptr(), sc.data_ptr(), sh.data_ptr(), w.data_ptr(), b.data_ptr(),
                          logits.data_ptr(), B, H, W, C, C, ncls, 1, st)
    g = lambda: _lib.call("segk_head_bwd_bn", dl.data_ptr(), z.data_ptr(), w.data_ptr(), dy.data_ptr(), part.data_ptr(),
                          dw.data_ptr(), db.data_ptr(), B, H, W, C, C, ncls, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
                          rs.data_ptr(), bnpart.data_ptr(), 1, st)
    tf = timeit(f, 30); tb = timeit(g, 30)
    print(f"head fwd {tf:7.1f} us ({P*(2*C+4*ncls)/tf/1e3:7.1f} GB/s)   bwd {tb:7.1f} us ({P*(4*C+4*ncls)/tb/1e3:7.1f} GB/s)")


def vit():
    """The four GEMMs of a ViT-B/16 encoder layer at BASELINE config 4 (B = 16, 197 tokens: M = 3152 rows): QKV, out_proj
    (K split three ways), fc1 (+ quick_gelu), fc2 (K split three ways), through the C ABI."""
    dt = torch.bfloat16
    M, D, I = 16 * 197, 768, 3072
    Mp = (M + 15) // 16 * 16
    st = ops._stream()
    def packed(n, k):
        w = torch.randn((n, k), device="cuda") / k ** 0.5
        return ops.pack_conv(w.reshape(n, k, 1, 1), k, 0, dt, 0, taps=1)
    nosplit = os.environ.get("KB_NOSPLIT") is not None      # every GEMM in one piece (segk_linear), no split-K
    for name, K, N, act, S in (("qkv", D, 3 * D, 0, 1), ("out_proj", D, D, 0, 3), ("fc1", D, I, 1, 1), ("fc2", I, D, 0, 3)):
        S = 1 if nosplit else S
        a = torch.randn((Mp, K), device="cuda").to(dt)
        w = packed(N, K)
        bias = torch.zeros(N, device="cuda")
        o = torch.empty((S * Mp, N), dtype=dt, device="cuda")
        if S > 1:
            f = lambda: _lib.call("segk_linear_splitk", a.data_ptr(), w.data_ptr(), bias.data_ptr(), o.data_ptr(), Mp, K, N, S, 1, st)
        else:
            f = lambda: _lib.call("segk_linear", a.data_ptr(), w.data_ptr(), bias.data_ptr(), o.data_ptr(), Mp, K, N, act, 1, st)
        t = timeit(f, 50)
        fl = 2.0 * M * K * N
        print(f"vit {name:9s} M={M} K={K:5d} N={N:5d} S={S}  {t:7.1f} us  {fl/t/1e6:7.1f} TF/s")


def stem():
    """The U-Net stem (3 -> 64 @ 256 x 256 from the NCHW fp32 batch, B = 32): forward with statistics, and weight gradient."""
    B, Cin, Cout, H, W = 32, 3, 64, 256, 256
    x = torch.rand((B, Cin, H, W), device="cuda")
    w = torch.randn((Cout, Cin, 3, 3), device="cuda") / 5
    z = torch.empty((B, H, W, Cout), dtype=torch.bfloat16, device="cuda")
    dz = torch.randn((B, H, W, Cout), device="cuda").to(torch.bfloat16)
    rows = _lib.query("segk_stem3x3_rows", B, H, W, Cin, Cout, 1)
    stats = torch.empty(_lib.query("segk_bn_stats_floats", rows, Cout), device="cuda")
    S = _lib.query("segk_stem3x3_wgrad_slabs", B, H, W, Cin, Cout, 1)
    slabs = torch.empty(S * 64 * 32, device="cuda")
    st = ops._stream()
    tf = timeit(lambda: _lib.call("segk_stem3x3", x.data_ptr(), w.data_ptr(), z.data_ptr(), 0, stats.data_ptr(), B, H, W, Cin,
                                  Cout, 1, st), 30)
    tw = timeit(lambda: _lib.call("segk_stem3x3_wgrad", x.data_ptr(), dz.data_ptr(), slabs.data_ptr(), B, H, W, Cin, Cout, 1, st), 30)
    P = B * H * W
    print(f"stem fwd {tf:7.1f} us ({P*(Cin*4+Cout*2)/tf/1e3:7.1f} GB/s)   wgrad {tw:7.1f} us ({P*(Cin*4+Cout*2)/tw/1e3:7.1f} GB/s)")


def ends():
    """The two ends of the full-resolution level with the stored gradient and without it (ops.END_FUSION_MIN_BYTES is read off
    this table): head end = segk_head_bwd_bn + segk_bn_relu_bwd_from_part against segk_head_bwd_bn_stats + segk_head_bn_bwd_apply,
    stem end = segk_bn_relu_bwd + segk_stem3x3_wgrad against segk_bn_relu_bwd_stats + segk_stem3x3_wgrad_bn, at gradient
    tensors of 16, 67, 134 and 268 MB (B = 2, 8, 16, 32 at 64 channels, 256 x 256; the last is the bench shape).  Seven repeats
    of `iters` launches each: median, and the spread (max - min) of the repeats.  No sequence overwrites its inputs: z and the
    incoming gradient g keep their seeded values through every launch (the stored forms write dy / dz to buffers of their own;
    the in-place apply of DoubleConvFn._backward moves the same bytes)."""
    C, H, W, ncls, Cin = 64, 256, 256, 3, 3
    dt = torch.bfloat16
    st = ops._stream()
    iters = 20
    print(f"{'end':5s} {'MB':>6s} {'stored us':>10s} {'spread':>7s} {'unstored us':>12s} {'spread':>7s} {'gain us':>8s}")
    for B in (2, 8, 16, 32):
        P = B * H * W
        z = torch.randn((P, C), device="cuda").to(dt)
        g = torch.randn((P, C), device="cuda").to(dt)
        dz = torch.empty_like(z); dy = torch.empty_like(z)
        sc = torch.rand(C, device="cuda") + 0.5; sh = torch.rand(C, device="cuda") - 0.5
        mu = torch.zeros(C, device="cuda"); rs = torch.ones(C, device="cuda")
        bn = (sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr())
        coef = torch.empty(2 * C, device="cuda"); dga = torch.empty(C, device="cuda"); dbe = torch.empty(C, device="cuda")
        # head end
        w = torch.randn((ncls, C), device="cuda") / 8
        dl = torch.randn((B, ncls, H, W), device="cuda") / P
        part = torch.empty(_lib.query("segk_head_part_floats", P, C), device="cuda")
        nb = _lib.query("segk_head_bwd_blocks", P)
        bnpart = torch.empty(nb * C * 2, device="cuda"); dw = torch.empty((ncls, C), device="cuda"); db = torch.empty(ncls, device="cuda")

        def head_stored():
            _lib.call("segk_head_bwd_bn", dl.data_ptr(), z.data_ptr(), w.data_ptr(), dy.data_ptr(), part.data_ptr(), dw.data_ptr(),
                      db.data_ptr(), B, H, W, C, C, ncls, *bn, bnpart.data_ptr(), 1, st)
            _lib.call("segk_bn_relu_bwd_from_part", dy.data_ptr(), z.data_ptr(), dz.data_ptr(), *bn, P, C, C, bnpart.data_ptr(), nb,
                      dga.data_ptr(), dbe.data_ptr(), coef.data_ptr(), 1, st)

        def head_unstored():
            _lib.call("segk_head_bwd_bn_stats", dl.data_ptr(), z.data_ptr(), w.data_ptr(), part.data_ptr(), dw.data_ptr(),
                      db.data_ptr(), B, H, W, C, C, ncls, *bn, bnpart.data_ptr(), 1, st)
            _lib.call("segk_head_bn_bwd_apply", dl.data_ptr(), z.data_ptr(), w.data_ptr(), dz.data_ptr(), *bn, B, H, W, C, C, ncls,
                      bnpart.data_ptr(), nb, dga.data_ptr(), dbe.data_ptr(), coef.data_ptr(), 1, st)
        # stem end
        x = torch.rand((B, Cin, H, W), device="cuda")
        S = _lib.query("segk_stem3x3_wgrad_slabs", B, H, W, Cin, C, 1)
        slabs = torch.empty(S * 64 * 32, device="cuda")
        rpart = torch.empty(_lib.query("segk_bn_bwd_blocks", P, C, 1) * C * 2, device="cuda")

        def stem_stored():
            _lib.call("segk_bn_relu_bwd", g.data_ptr(), z.data_ptr(), dz.data_ptr(), *bn, P, C, C, rpart.data_ptr(), dga.data_ptr(),
                      dbe.data_ptr(), coef.data_ptr(), 1, st)
            _lib.call("segk_stem3x3_wgrad", x.data_ptr(), dz.data_ptr(), slabs.data_ptr(), B, H, W, Cin, C, 1, st)

        def stem_unstored():
            _lib.call("segk_bn_relu_bwd_stats", g.data_ptr(), z.data_ptr(), *bn, P, C, C, rpart.data_ptr(), dga.data_ptr(),
                      dbe.data_ptr(), coef.data_ptr(), 1, st)
            _lib.call("segk_stem3x3_wgrad_bn", x.data_ptr(), g.data_ptr(), z.data_ptr(), *bn, coef.data_ptr(), slabs.data_ptr(),
                      B, H, W, Cin, C, 1, st)
        for name, old, new in (("head", head_stored, head_unstored), ("stem", stem_stored, stem_unstored)):
            to, tn = [], []
            for _ in range(7):                          # interleaved, so drift of the box lands on both alike
                to.append(timeit(old, iters)); tn.append(timeit(new, iters))
            to.sort(); tn.sort()
            print(f"{name:5s} {P * C * 2 / 1e6:6.1f} {to[3]:10.1f} {to[-1] - to[0]:7.1f} {tn[3]:12.1f} {tn[-1] - tn[0]:7.1f} "
                  f"{to[3] - tn[3]:8.1f}", flush=True)


def pack():
    """Weight re-layout after an optimizer step: one-pass forward + data-gradient pack against the two per-mode packs,
    all 18 Conv3x3 weights of the U-Net."""
    dt = torch.bfloat16
    shapes = [(64, 3, 0), (64, 64, 0), (128, 64, 0), (128, 128, 0), (256, 128, 0), (256, 256, 0), (512, 256, 0), (512, 512, 0),
              (1024, 512, 0), (1024, 1024, 0), (512, 512, 512), (512, 512, 0), (256, 256, 256), (256, 256, 0),
              (128, 128, 128), (128, 128, 0), (64, 64, 64), (64, 64, 0)]
    ws = [torch.randn((co, ca + cb, 3, 3), device="cuda") for co, ca, cb in shapes]
    t_both = timeit(lambda: [ops.pack_conv_both(w, ca, cb, dt) for w, (co, ca, cb) in zip(ws, shapes)], 20)
    t_two = timeit(lambda: [(ops.pack_conv(w, ca, cb, dt, 0), ops.pack_conv(w, ca, cb, dt, 1)) for w, (co, ca, cb) in zip(ws, shapes)], 20)
    nbytes = sum(w.numel() for w in ws) * (4 + 2 + 2)
    print(f"pack all 18 weights: one-pass {t_both:8.1f} us ({nbytes/t_both/1e3:7.1f} GB/s)   per-mode {t_two:8.1f} us")


def recon():
    """Reconstruction head + MSE of the autoencoder pretraining through the C ABI at B = 32, 256 x 256, Cin 64, Cout 3,
    bf16: fused head forward (3x3 conv + bias + Sigmoid -> fp32 NCHW), MSE forward / backward, Sigmoid backward into the
    act layout.  In the same process, the chain it replaces: segk_conv3x3 to 32 padded channels with bias, then stock
    torch.sigmoid(z.float()).contiguous(), F.mse_loss forward and backward, the Sigmoid backward and to_act of the gradient."""
    import torch.nn.functional as F
    B, Cin, Cout, H, W = 32, 64, 3, 256, 256
    dt = torch.bfloat16
    P, Cp, Coutp = B * H * W, ops.pad32(Cin), ops.pad32(Cout)
    x = torch.rand((B, H, W, Cp), device="cuda").to(dt)
    w = torch.randn((Cout, Cin, 3, 3), device="cuda") / (3 * Cin ** 0.5); b = torch.randn(Cout, device="cuda") * 0.1
    X = torch.rand((B, Cout, H, W), device="cuda")
    rec = torch.empty((B, Cout, H, W), device="cuda"); drec = torch.empty_like(rec)
    dz = torch.empty((B, H, W, Coutp), dtype=dt, device="cuda")
    part = torch.empty(_lib.MSE_PART_FLOATS, device="cuda"); out = torch.empty(1, device="cuda"); go = torch.ones(1, device="cuda")
    st = ops._stream()
    hf = lambda: _lib.call("segk_recon_head_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), rec.data_ptr(), B, H, W, Cp, Cin,
                           Cout, 1, st)
    sb = lambda: _lib.call("segk_recon_sigmoid_bwd", drec.data_ptr(), rec.data_ptr(), dz.data_ptr(), B, H, W, Cout, Coutp, 1, st)
    mf = lambda: _lib.call("segk_mse_fwd", rec.data_ptr(), X.data_ptr(), part.data_ptr(), part.numel(), out.data_ptr(), rec.numel(),
                           1, st)
    mb = lambda: _lib.call("segk_mse_bwd", rec.data_ptr(), X.data_ptr(), go.data_ptr(), drec.data_ptr(), None, rec.numel(), 1, st)

    def fused():
        hf(); mf(); mb(); sb()
    n = rec.numel()
    rows = [("head fwd", hf, P * (Cp * 2 + 4 * Cout)), ("mse fwd", mf, 8.0 * n), ("mse bwd", mb, 12.0 * n),
            ("sigmoid bwd", sb, P * (8.0 * Cout + 2 * Coutp))]
    for name, fn, nbytes in rows:
        t = timeit(fn, 50)
        print(f"recon {name:12s} {t:8.1f} us  {nbytes / t / 1e3:7.1f} GB/s")
    tf = timeit(fused, 30)
    # the replaced chain
    wp = ops.pack_conv(w, Cin, 0, dt, 0)
    b32 = torch.zeros(Coutp, device="cuda"); b32[:Cout] = b
    zb = torch.empty((B, H, W, Coutp), dtype=dt, device="cuda")
    conv = lambda: _lib.call("segk_conv3x3", x.data_ptr(), 0, wp.data_ptr(), b32.data_ptr(), 0, 0, zb.data_ptr(), 0, 0, B, H, W,
                             Cp, 0, Coutp, 0, 1, st)

    def stock():
        conv()
        zl = ops.act_view(zb, Cout).detach().requires_grad_()
        r = torch.sigmoid(zl.float()).contiguous()
        F.mse_loss(r, X).backward()
        ops.to_act(zl.grad, dt)
    tc = timeit(conv, 30)
    ts = timeit(stock, 30)
    print(f"recon replaced: conv3x3 to {Coutp} ch + bias {tc:8.1f} us; whole chain (conv, stock sigmoid / mse fwd+bwd, to_act) "
          f"{ts:8.1f} us")
    print(f"recon fused chain (head fwd, mse fwd, mse bwd, sigmoid bwd) {tf:8.1f} us   = {ts / tf:5.2f}x faster than the "
          f"replaced chain")
    clk = ops.clock_probe()
    print(f"recon clock probe: median {clk['median_ghz']} GHz (mfma_32x32x16), {clk['mfma_16x16x32']['median_ghz']} GHz (mfma_16x16x32)")


def predict():
    """Prediction post-processing through the C ABI: the fused segk_predict_mask (mask + colour + class counts in one pass)
    against the route it replaces -- segk_crop_resize to full-size fp32 logits, torch.argmax, a palette index and
    bincount -- at three output sizes, C = 3 and 4, from a 224 x 224 slot.  Both run in this process, alternating, seven
    rounds each; the line gives the median and the min..max spread.  Bytes per pixel are what each route WRITES."""
    from image_segmentation_amd.utils import _geometry
    T = 224
    st = ops._stream()
    for oh, ow in ((375, 500), (1200, 1600), (3000, 4000)):
        for C in (3, 4):
            nh, nw, pt, pl, _ = _geometry(oh, ow, T)
            slot = torch.randn((C, T, T), device="cuda")
            pal = torch.tensor([(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)], dtype=torch.uint8, device="cuda")
            pal_l = pal[:C]
            mask = torch.empty((oh, ow), dtype=torch.uint8, device="cuda")
            color = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
            counts = torch.zeros(8, dtype=torch.int64, device="cuda")
            full = torch.empty((C, oh, ow), device="cuda")

            def fused():
                _lib.call("segk_predict_mask", slot.data_ptr(), mask.data_ptr(), color.data_ptr(), pal.data_ptr(), counts.data_ptr(),
                          None, None, C, T, pt, pl, nh, nw, oh, ow, 0, st)

            def old():
                _lib.call("segk_crop_resize", slot.data_ptr(), full.data_ptr(), C, T, pt, pl, nh, nw, oh, ow, 0, st)
                m = full.argmax(0)
                return m.to(torch.uint8), pal_l[m], torch.bincount(m.flatten(), minlength=C)
            m_old, c_old, n_old = old()
            counts.zero_(); fused()
            same = bool(torch.equal(mask, m_old) and torch.equal(color, c_old) and torch.equal(counts[:C], n_old))
            iters = 200 if oh * ow < 10 ** 6 else 50
            tf, to = [], []
            for _ in range(7):
                tf.append(timeit(fused, iters)); to.append(timeit(old, iters))
            tf.sort(); to.sort()
            P = oh * ow
            bf, bo = 4, 4 * C + 8 + 1 + 3          # fused: mask + RGB; old: fp32 logits, int64 argmax, uint8 mask, RGB
            print(f"predict {oh}x{ow} C={C}  fused {tf[3]:8.1f} us [{tf[0]:.1f}..{tf[-1]:.1f}] {bf} B/px {P*bf/tf[3]/1e3:7.1f} GB/s   "
                  f"replaced {to[3]:8.1f} us [{to[0]:.1f}..{to[-1]:.1f}] {bo} B/px {P*bo/to[3]/1e3:7.1f} GB/s   "
                  f"{to[3]/tf[3]:5.1f}x   outputs equal: {same}")


def prompt():
    """Point prompts through the C ABI (csrc/prompt.hip): device-event times of the two launches of PromptSampler -- the score
    pass over K candidate windows per image and the make pass that writes heat-maps and targets -- at B = 32, 256 x 256 and
    B = 8, 512 x 512 for K = 64, 256, 1000 (warmed, 100 repetitions per round, seven rounds: median and min..max), the make
    kernel's bytes/s from its byte count (8 B read + 12 B x per_image written per pixel), the whole sampler call, and beside
    them the HOST time of the route it replaces, written out in NumPy as the reference's cell computes it (whole-image
    Gaussian per draw, per-class sums, retry loop; one thread, same label maps).  Also written to
    profiles/prompt_points.json (or the file given with --out)."""
    import json, time
    import numpy as np
    from image_segmentation_amd import prompts
    st = ops._stream()
    PI, sigma = 2, 3.0
    rows = []

    def host_route(maps, max_attempts=1000):
        rng = np.random.RandomState(0)
        t0 = time.perf_counter()
        done = 0
        for m in maps:
            H, W = m.shape
            present = np.unique(m)
            if len(present[present > 0]) < 2:
                continue
            yy, xx = np.indices((H, W))
            found, attempts = [], 0
            while len(found) < 2 and attempts < max_attempts:
                attempts += 1
                cy, cx = rng.randint(0, H), rng.randint(0, W)
                heat = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma ** 2))
                sc = {c: heat[m == c].sum() for c in present[present > 0]}
                best = 0 if all(v < 1e-9 for v in sc.values()) else max(sc, key=sc.get)
                if best > 0 and best not in found:
                    found.append(best)
                    _ = (heat * 255).astype(np.uint8), np.where(m == best, best, 0).astype(np.uint8)
            done += 1
        return done / (time.perf_counter() - t0)

    for B, S in ((32, 256), (8, 512)):
        blocks = torch.randint(1, 4, (B, S // 32, S // 32), device="cuda")
        lab = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()           # blocky class regions 1..3
        wt, nw, qt, nq, R = prompts._tables_on(sigma, S, S, lab.device)
        host_ips = host_route(list(lab.cpu().numpy()))
        for K in (64, 256, 1000):
            cen = torch.stack((torch.randint(0, S, (B, K), device="cuda", dtype=torch.int32),
                               torch.randint(0, S, (B, K), device="cuda", dtype=torch.int32)), -1).contiguous()
            scores = torch.empty((B, K, 8), dtype=torch.float64, device="cuda")
            cls = torch.empty((B, K), dtype=torch.int32, device="cuda")
            heat = torch.empty((B, PI, 1, S, S), device="cuda")
            tgt = torch.empty((B, PI, S, S), dtype=torch.int64, device="cuda")
            classes = torch.empty((B, PI), dtype=torch.int32, device="cuda")
            oc = torch.empty((B, PI, 2), dtype=torch.int32, device="cuda")
            valid = torch.empty((B,), dtype=torch.bool, device="cuda")
            f_sc = lambda: _lib.call("segk_prompt_scores", lab.data_ptr(), 0, cen.data_ptr(), wt.data_ptr(), nw, R,
                                     scores.data_ptr(), cls.data_ptr(), B, K, S, S, st)
            f_mk = lambda: _lib.call("segk_prompt_make", lab.data_ptr(), 0, cen.data_ptr(), cls.data_ptr(), qt.data_ptr(), nq,
                                     heat.data_ptr(), tgt.data_ptr(), classes.data_ptr(), oc.data_ptr(), valid.data_ptr(), B, K,
                                     PI, S, S, st)
            sampler = prompts.PromptSampler(sigma=sigma, candidates=K, per_image=PI, seed=0)
            f_all = lambda: sampler(lab)
            f_sc(); f_mk(); f_all()
            ts, tm, ta = [], [], []
            for _ in range(7):
                ts.append(timeit(f_sc, 100)); tm.append(timeit(f_mk, 100)); ta.append(timeit(f_all, 100))
            ts.sort(); tm.sort(); ta.sort()
            nbytes = B * S * S * (8 + 12 * PI)
            row = {"B": B, "size": S, "K": K, "R": R, "valid_images": int(valid.sum()),
                   "scores_us": {"median": ts[3], "min": ts[0], "max": ts[-1]},
                   "make_us": {"median": tm[3], "min": tm[0], "max": tm[-1]}, "make_bytes": nbytes,
                   "make_GBps": nbytes / tm[3] / 1e3,
                   "sampler_call_us": {"median": ta[3], "min": ta[0], "max": ta[-1]},
                   "host_numpy_route_images_per_s": host_ips, "device_images_per_s": B / (ta[3] * 1e-6)}
            rows.append(row)
            print(f"prompt B={B} {S}x{S} K={K:4d} R={R}  scores {ts[3]:8.1f} us [{ts[0]:.1f}..{ts[-1]:.1f}]   make {tm[3]:7.1f} us "
                  f"[{tm[0]:.1f}..{tm[-1]:.1f}] {nbytes / tm[3] / 1e3:7.1f} GB/s   sampler call (draw + 2 launches) {ta[3]:8.1f} us "
                  f"[{ta[0]:.1f}..{ta[-1]:.1f}] = {B / (ta[3] * 1e-6):9.0f} images/s   host NumPy route {host_ips:7.1f} images/s "
                  f"(host time, one thread)")
    clk = ops.clock_probe()
    out = {"rows": rows, "clock_probe_ghz": clk["median_ghz"], "build_id": _lib.build_id(), "per_image": PI, "sigma": sigma}
    path = os.path.join(ROOT, "profiles", "prompt_points.json")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(f"prompt clock probe: median {clk['median_ghz']} GHz; written to {path}")


def augment():
    """Device-side augmentation through the C ABI (csrc/augment.hip): B = 32 sources of 375 x 500 (uint8 RGB + a one-channel
    label) -> 256 x 256, for plain resize, each of the eight ops and the mixed default.  Per row: device-event time of the
    batch's launches replayed alone (prefilter + resample; warmed, 50 repetitions per round, seven rounds: median and
    min..max), GB/s over the algorithmic bytes (every source read once + X fp32 and y int64 written), the fraction of the
    6.29 TB/s copy ceiling, and the whole Augmenter.apply call (host table work + one pinned upload + the launches).  Also
    written to profiles/kbench_augment.json (or the file given with --out)."""
    import json
    import numpy as np
    from image_segmentation_amd import augment as A
    B, H, W, T, COPY = 32, 375, 500, 256, 6.29e12
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.randint(0, 256, (H, W, 3), generator=g, device="cuda", dtype=torch.uint8) for _ in range(B)]
    labs = [torch.randint(0, 3, (H, W), generator=g, device="cuda", dtype=torch.uint8) for _ in range(B)]
    nbytes = B * (H * W * 4 + T * T * (12 + 8))
    rows = []
    for name, ops_ in [(A.OP_NAMES[o], (o,)) for o in range(9)] + [("mixed", A.ALL_OPS)]:
        aug = A.Augmenter(target_size=T, ops=ops_, label_lut=A.TARGET_REMAP, seed=0)
        plans = aug.plan([(H, W)] * B)
        out = aug.apply(imgs, labs, plans)
        launches = list(aug.last_launches)
        f_k = lambda: [_lib.call(n, *a) for n, a in launches]
        f_all = lambda: aug.apply(imgs, labs, plans)
        tk, ta = [], []
        for _ in range(7):
            tk.append(timeit(f_k, 50)); ta.append(timeit(f_all, 50))
        tk.sort(); ta.sort()
        row = {"op": name, "launches": [n for n, _ in launches], "kernels_us": {"median": tk[3], "min": tk[0], "max": tk[-1]},
               "apply_call_us": {"median": ta[3], "min": ta[0], "max": ta[-1]}, "bytes": nbytes,
               "GBps": nbytes / tk[3] / 1e3, "copy_ceiling_fraction": nbytes / (tk[3] * 1e-6) / COPY,
               "images_per_s_call": B / (ta[3] * 1e-6)}
        rows.append(row)
        print(f"augment {name:12s} B={B} {H}x{W}->{T}  kernels {tk[3]:8.1f} us [{tk[0]:.1f}..{tk[-1]:.1f}] {row['GBps']:7.1f} GB/s "
              f"= {100 * row['copy_ceiling_fraction']:5.2f} % of the copy ceiling   apply() call {ta[3]:8.1f} us "
              f"[{ta[0]:.1f}..{ta[-1]:.1f}] = {row['images_per_s_call']:8.0f} images/s   ({' + '.join(row['launches'])})")
        del out
    clk = ops.clock_probe()
    res = {"rows": rows, "clock_probe_ghz": clk["median_ghz"], "build_id": _lib.build_id(), "B": B, "source": [H, W], "T": T}
    path = os.path.join(ROOT, "profiles", "kbench_augment.json")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"augment clock probe: median {clk['median_ghz']} GHz; written to {path}")


def perturb():
    """Robustness perturbations through the C ABI (csrc/perturb.hip): B = 32 images of 375 x 500 uint8 RGB at their own size,
    every kind at its strongest default level plus blur at 1 pass.  Per row: device-event time of the one launch replayed
    alone (warmed, 50 repetitions per round, seven rounds: median and min..max), GB/s over the 6 bytes per pixel every kind
    must move (3 read + 3 written), the time that floor takes at the copy rate measured here (a device-to-device copy of the
    same bytes, same rounds), and the whole perturb() call (host tables + one pinned upload + the launch).  The last row is
    what follows in a sweep: the 32 segk_resize_pad_u8 launches that bring the batch to 224 x 224.  Also written to
    profiles/kbench_perturb.json (or the file given with --out)."""
    import json
    from image_segmentation_amd import robustness as P
    from image_segmentation_amd.inference import _into_slot
    B, H, W, T = 32, 375, 500, 224
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.randint(0, 256, (H, W, 3), generator=g, device="cuda", dtype=torch.uint8) for _ in range(B)]
    nbytes = B * H * W * 6

    def rounds(fn):
        t = sorted(timeit(fn, 50) for _ in range(7))
        return {"median": t[3], "min": t[0], "max": t[-1]}
    src, dst = torch.cat([im.reshape(-1) for im in imgs]), torch.empty(B * H * W * 3, dtype=torch.uint8, device="cuda")
    tc = rounds(lambda: dst.copy_(src))
    copy_rate = nbytes / (tc["median"] * 1e-6)
    print(f"perturb copy of the same bytes (read {nbytes // 2} + write {nbytes // 2}): {tc['median']:.1f} us = {copy_rate / 1e9:.1f} GB/s")
    rows = []
    cases = [(k, P.DEFAULT_LEVELS[k][-1]) for k in P.PERTURBATIONS]
    cases.insert(2, ("gaussian_blur", 1))
    for kind, level in cases:
        plan = P.perturb_plan(kind, level, [(H, W)] * B, seed=0)
        out, (name, args), keep = P._launch(imgs, plan)
        tk = rounds(lambda: _lib.call(name, *args))
        ta = rounds(lambda: P.perturb(imgs, kind, level, seed=0))
        row = {"kind": kind, "level": level, "launch": name, "kernel_us": tk, "perturb_call_us": ta, "bytes": nbytes,
               "GBps": nbytes / tk["median"] / 1e3, "floor_us_at_copy_rate": tc["median"],
               "copy_rate_fraction": tc["median"] / tk["median"]}
        rows.append(row)
        print(f"perturb {kind:20s} level {level:<5} B={B} {H}x{W}  kernel {tk['median']:8.1f} us [{tk['min']:.1f}..{tk['max']:.1f}] "
              f"{row['GBps']:7.1f} GB/s = {100 * row['copy_rate_fraction']:5.1f} % of the copy rate   perturb() call "
              f"{ta['median']:8.1f} us [{ta['min']:.1f}..{ta['max']:.1f}]   ({name})")
        del out, keep
    X = torch.empty((B, 3, T, T), dtype=torch.float32, device="cuda")
    tr = rounds(lambda: [_into_slot(im, X[k], T, "bilinear", None, "image") for k, im in enumerate(imgs)])
    print(f"perturb then: {B} x segk_resize_pad_u8 -> {T}x{T}  {tr['median']:8.1f} us [{tr['min']:.1f}..{tr['max']:.1f}]")
    clk = ops.clock_probe()
    res = {"rows": rows, "copy_us": tc, "copy_GBps": copy_rate / 1e9, "resize_pad_u8_x32_us": tr, "clock_probe_ghz": clk["median_ghz"],
           "build_id": _lib.build_id(), "B": B, "source": [H, W], "T": T}
    path = os.path.join(ROOT, "profiles", "kbench_perturb.json")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"perturb clock probe: median {clk['median_ghz']} GHz; written to {path}")


def components():
    """Mask clean-up through the C ABI (csrc/components.hip): segk_cc_label, segk_cc_clean (min_area 20, keep_largest of
    classes 1 and 2) and segk_mask_finish on a 375 x 500 and a 1024 x 1024 mask -- smooth blobs with 2 % speckle (the
    realistic case) and uniform 4-class noise (the worst case: a component every few pixels), connectivity 4 and 8.  Beside
    them, on the same box: segk_predict_mask to the same size from a 224 x 224 slot, and the U-Net forward per image (3 -> 4
    classes, B = 32, 224 x 224, the compute dtype in force).  Device-event times, warmed, 100 repetitions per round, seven
    rounds: median and min..max.  Also written to profiles/kbench_components.json (or the file given with --out)."""
    import json
    import image_segmentation_amd as seg
    from image_segmentation_amd.components import ws_ints
    from image_segmentation_amd.utils import _geometry
    st = ops._stream()
    T, cap = 224, 1024

    def rounds(fn, iters=100):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return {"median": t[3], "min": t[0], "max": t[-1]}

    def blobs(H, W, g):
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                                indexing="ij")
        m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        for c, (cy, cx, ry, rx) in ((1, (0.35, 0.3, 0.25, 0.2)), (2, (0.65, 0.7, 0.22, 0.25))):
            d = ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2
            m[d <= 1.0] = c
            m[(d > 1.0) & (d <= 1.25)] = 3
        hit = torch.rand((H, W), generator=g, device="cuda") < 0.02
        return torch.where(hit, torch.randint(0, 4, (H, W), generator=g, device="cuda", dtype=torch.uint8), m)

    model = seg.unet(3, 4).cuda().eval()
    X = torch.randn((32, 3, T, T), device="cuda")
    with torch.no_grad():
        model(X)
        tfwd = rounds(lambda: model(X), 10)
    fwd_us = tfwd["median"] / 32
    print(f"components: U-Net forward B=32 {T}x{T} {tfwd['median']:9.1f} us [{tfwd['min']:.1f}..{tfwd['max']:.1f}] = {fwd_us:7.1f} us per image")
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    pal = torch.tensor([(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)], dtype=torch.uint8, device="cuda")
    for H, W in ((375, 500), (1024, 1024)):
        nh, nw, pt, pl, _ = _geometry(H, W, T)
        slot = torch.randn((4, T, T), device="cuda")
        pm, color = torch.empty((H, W), dtype=torch.uint8, device="cuda"), torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(8, dtype=torch.int64, device="cuda")
        tp = rounds(lambda: _lib.call("segk_predict_mask", slot.data_ptr(), pm.data_ptr(), color.data_ptr(), pal.data_ptr(),
                                      counts.data_ptr(), None, None, 4, T, pt, pl, nh, nw, H, W, 0, st))
        print(f"components {H}x{W}: segk_predict_mask {tp['median']:8.1f} us [{tp['min']:.1f}..{tp['max']:.1f}]")
        for kind in ("blobs", "noise4"):
            m = blobs(H, W, g) if kind == "blobs" else torch.randint(0, 4, (H, W), generator=g, device="cuda", dtype=torch.uint8)
            i32 = dict(dtype=torch.int32, device="cuda")
            labels, num, ws = torch.empty((H, W), **i32), torch.empty(1, **i32), torch.empty(ws_ints(H, W), **i32)
            r, box, out = torch.empty((5, cap), **i32), torch.empty((cap, 4), **i32), torch.empty_like(m)
            for conn in (4, 8):
                f_l = lambda: _lib.call("segk_cc_label", m.data_ptr(), labels.data_ptr(), num.data_ptr(), r[0].data_ptr(), r[1].data_ptr(),
                                        box.data_ptr(), r[2].data_ptr(), ws.data_ptr(), H, W, conn, 255, cap, st)
                f_c = lambda: _lib.call("segk_cc_clean", m.data_ptr(), out.data_ptr(), ws.data_ptr(), r[3].data_ptr(), r[4].data_ptr(), H, W,
                                        20, 0b110, cap, st)
                f_f = lambda: _lib.call("segk_mask_finish", out.data_ptr(), color.data_ptr(), pal.data_ptr(), counts.data_ptr(), None, None,
                                        4, H, W, st)
                f_l(); f_c(); f_f()
                K, changed = int(num.item()), int((out != m).sum())
                tl, tc, tf = rounds(f_l), rounds(f_c), rounds(f_f)
                total = tl["median"] + tc["median"] + tf["median"]
                rows.append({"size": [H, W], "mask": kind, "connectivity": conn, "components": K, "pixels_changed": changed,
                             "label_us": tl, "clean_us": tc, "mask_finish_us": tf, "predict_mask_us": tp,
                             "forward_us_per_image": fwd_us, "label_clean_finish_over_forward": total / fwd_us})
                print(f"components {H}x{W} {kind:6s} c{conn} K={K:7d} changed={changed:7d}  label {tl['median']:8.1f} us "
                      f"[{tl['min']:.1f}..{tl['max']:.1f}]   clean {tc['median']:8.1f} us [{tc['min']:.1f}..{tc['max']:.1f}]   "
                      f"finish {tf['median']:7.1f} us [{tf['min']:.1f}..{tf['max']:.1f}]   sum = {total / fwd_us:5.2f} x forward per image")
    clk = ops.clock_probe()
    res = {"rows": rows, "forward_B32_us": tfwd, "compute_dtype": str(seg.get_compute_dtype()), "clock_probe_ghz": clk["median_ghz"],
           "build_id": _lib.build_id(), "T": T, "max_components": cap}
    path = os.path.join(ROOT, "profiles", "kbench_components.json")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"components clock probe: median {clk['median_ghz']} GHz; written to {path}")


def vectors():
    """Mask vectorisation through the C ABI (csrc/vectors.hip): segk_vec_runs and segk_vec_rings on the labels of
    segk_cc_label (connectivity 4, every class labelled) at 256 x 256, 1024 x 1024 and 3000 x 4000 -- smooth blobs (the realistic
    case) and noise (half the pixels one of three classes: a ring every few pixels).  max_edges is the mask's own edge count
    rounded up to a multiple of 4096 (read once, before the timing), so the round count is the one that mask needs.  Beside each
    line: `mask.cpu()` alone at that size -- the floor of any host route.  Device-event times, warmed, seven rounds: median and
    min..max; mask.cpu() by the host clock around a synchronised copy.  Written to profiles/vectors_kbench.txt (or --out)."""
    import time
    from image_segmentation_amd.components import ws_ints as cc_ws
    from image_segmentation_amd.vectors import ws_ints as vec_ws
    st = ops._stream()
    i32 = dict(dtype=torch.int32, device="cuda")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def rounds(fn, iters):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return t[3], t[0], t[-1]

    def blobs(H, W):
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                                indexing="ij")
        m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        for c, (cy, cx, ry, rx) in ((1, (0.35, 0.3, 0.25, 0.2)), (2, (0.65, 0.7, 0.22, 0.25))):
            d = ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2
            m[d <= 1.0] = c
            m[(d > 1.0) & (d <= 1.25)] = 3
        return m

    g = torch.Generator(device="cuda").manual_seed(0)
    say(f"vectors: build {_lib.build_id()}, clock probe {ops.clock_probe()['median_ghz']} GHz")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None       # one size, e.g. 3000x4000 (a profiler run)
    for H, W in ((256, 256), (1024, 1024), (3000, 4000)):
        if only is not None and only != f"{H}x{W}":
            continue
        iters = 50 if H * W <= 1 << 20 else 5
        for kind in ("blobs", "noise"):
            if kind == "blobs":
                m = blobs(H, W)
            else:
                fg = torch.rand((H, W), generator=g, device="cuda") < 0.5
                m = torch.where(fg, torch.randint(1, 4, (H, W), generator=g, device="cuda", dtype=torch.uint8), torch.zeros((), dtype=torch.uint8, device="cuda"))
            labels, num, totals = torch.empty((H, W), **i32), torch.empty(1, **i32), torch.empty(4, **i32)
            cap = 1024
            r, box = torch.empty((3, cap), **i32), torch.empty((cap, 4), **i32)
            ws = torch.empty(cc_ws(H, W), **i32)
            f_l = lambda: _lib.call("segk_cc_label", m.data_ptr(), labels.data_ptr(), num.data_ptr(), r[0].data_ptr(), r[1].data_ptr(),
                                    box.data_ptr(), r[2].data_ptr(), ws.data_ptr(), H, W, 4, 0b1110, cap, st)
            f_l()
            one = torch.empty(8, **i32)
            wsv = torch.empty(vec_ws(H, W, 1), **i32)                   # a first call with max_edges = 1 only counts the edges
            _lib.call("segk_vec_rings", labels.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(),
                      one.data_ptr(), totals.data_ptr(), wsv.data_ptr(), H, W, 4, 1, 1, 1, st)
            E = int(totals[1].item())
            me = max(4096, (E + 4095) // 4096 * 4096)
            mr, mg = min(H * W, me + W), me // 4
            del ws, wsv
            wsv = torch.empty(vec_ws(H, W, me), **i32)
            runs, rings, xy = torch.empty((2, mr), **i32), torch.empty((3, mg), **i32), torch.empty((me, 2), **i32)
            area2, off = torch.empty(mg, dtype=torch.int64, device="cuda"), torch.empty(mg + 1, **i32)
            f_r = lambda: _lib.call("segk_vec_runs", labels.data_ptr(), runs[0].data_ptr(), runs[1].data_ptr(), totals.data_ptr(),
                                    wsv.data_ptr(), H, W, mr, st)
            f_g = lambda: _lib.call("segk_vec_rings", labels.data_ptr(), rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr(),
                                    area2.data_ptr(), off.data_ptr(), xy.data_ptr(), totals.data_ptr(), wsv.data_ptr(), H, W, 4, me, mg, me, st)
            f_r(); f_g()
            tot = totals.tolist()
            jumps = 1
            while (1 << (jumps - 1)) < me:
                jumps += 1
            tr, tg = rounds(f_r, iters), rounds(f_g, iters)
            cpu = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.cpu()
                cpu.append((time.perf_counter() - t0) * 1e6)
            cpu.sort()
            say(f"vectors {H}x{W} {kind:5s} K={int(num.item()):8d} runs={tot[0]:9d} edges={tot[1]:9d} rings={tot[2]:8d} vertices={tot[3]:9d} "
                f"max_edges={me:9d} ({2 * jumps} jump launches of {13 + 2 * jumps})")
            say(f"    segk_vec_runs {tr[0]:10.1f} us [{tr[1]:.1f}..{tr[2]:.1f}]   segk_vec_rings {tg[0]:10.1f} us [{tg[1]:.1f}..{tg[2]:.1f}]   "
                f"mask.cpu() {cpu[3]:10.1f} us [{cpu[0]:.1f}..{cpu[-1]:.1f}]   rings / mask.cpu() = {tg[0] / cpu[3]:6.2f}")
            del wsv, runs, rings, xy, area2, off
    path = os.path.join(ROOT, "profiles", "vectors_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def raster():
    """Label rasterisation (csrc/raster.hip): segk_raster_labels on (a) the polygons seg.vectorize finds in a
    blob mask at 256 x 256, batch 32, (b) the same at 3000 x 4000 (12 MP), batch 4, (c) 200 random triangles per image at
    512 x 512, batch 32.  Per workload: the launch alone (tables already on the device; device events, warmed, seven rounds:
    median and min..max), the whole seg.rasterize_batch call (host plan, pinned upload, launch; host clock, synchronised), the
    floor (the output bytes at the device-to-device copy rate measured beside it) and the host path it replaces (PIL
    ImageDraw.polygon per shape plus one upload per image; timing only: PIL's fill rule is not the one of 3.18).  Written to
    profiles/raster_kbench.txt (or --out)."""
    import time
    import numpy as np
    from PIL import Image, ImageDraw
    import image_segmentation_amd as seg
    from image_segmentation_amd import raster as R
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def rounds(fn, iters):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return t[3], t[0], t[-1]

    def host_rounds(fn, n=5):
        t = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    def blobs(H, W):
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                                indexing="ij")
        m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        for c, (cy, cx, ry, rx) in ((1, (0.35, 0.3, 0.25, 0.2)), (2, (0.65, 0.7, 0.22, 0.25))):
            d = ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2
            m[d <= 1.0] = c
            m[(d > 1.0) & (d <= 1.25)] = 3
        return m

    def blob_shapes(H, W):
        m = blobs(H, W)
        vec = seg.vectorize(m, classes=(1, 2, 3), max_edges=4 * (H + W) * 8)
        shapes = seg.shapes_from_vectors(vec)
        assert torch.equal(seg.rasterize(shapes, (H, W)), m)                # the loop closes on this mask
        return shapes

    def triangles(H, W, n, seed):
        rng = np.random.default_rng(seed)
        return [seg.Shape(rings=[rng.uniform(-0.1, 1.1, (3, 2)) * (W, H)], value=1 + k % 7) for k in range(n)]

    say(f"raster: build {_lib.build_id()}, clock probe {ops.clock_probe()['median_ghz']} GHz, tile {R.TILE_H} x {R.TILE_W}")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    work = (("blobs256", 256, 256, 32, 50), ("blobs12mp", 3000, 4000, 4, 5), ("triangles200", 512, 512, 32, 20))
    for name, H, W, B, iters in work:
        if only is not None and only != name:
            continue
        if name == "triangles200":
            per_image = [triangles(H, W, 200, 10 + b) for b in range(B)]
        else:
            per_image = [blob_shapes(H, W)] * B
        sizes = [(H, W)] * B
        plan = seg.raster_plan(per_image, sizes)
        out = torch.empty(plan["out_bytes"], dtype=torch.uint8, device=dev)
        other = torch.empty_like(out)
        blob, ptr = R._upload([plan["tiles"], plan["shapes"], plan["shape_list"], plan["edges"], plan["run_start"]], dev)
        st = ops._stream()
        f_k = lambda: _lib.call("segk_raster_labels", ptr[0], len(plan["tiles"]), ptr[1], len(plan["shapes"]), ptr[2], len(plan["shape_list"]),
                                ptr[3], len(plan["edges"]), ptr[4], len(plan["run_start"]), out.data_ptr(), out.numel(), 0, st)
        tk = rounds(f_k, iters)
        tc = rounds(lambda: other.copy_(out), iters)
        rate = 2 * out.numel() / tc[0] / 1e6                                # TB/s of the copy (read + write)
        floor = out.numel() / (rate * 1e6)                                  # us to write the output bytes at that rate
        tw = host_rounds(lambda: seg.rasterize_batch(per_image, sizes))
        polys = [[(s.value, [tuple(v) for v in (r / 256.0).tolist()]) for s in shp for r in s.rings] for shp in per_image]

        def pil():
            for pl in polys:
                im = Image.new("L", (W, H), 0)
                d = ImageDraw.Draw(im)
                for v, xy in pl:
                    d.polygon(xy, fill=v)
                torch.from_numpy(np.array(im)).to(dev)
        tp = host_rounds(pil, 3)
        listed = len(plan["shape_list"]) / len(plan["tiles"])
        say(f"raster {name:12s} {B} x {H}x{W}  shapes/image={len(per_image[0])} edges={len(plan['edges'])} tiles={len(plan['tiles'])} "
            f"shapes/tile={listed:.1f} out={out.numel() / 1e6:.2f} MB")
        say(f"    segk_raster_labels {tk[0]:10.1f} us [{tk[1]:.1f}..{tk[2]:.1f}]   floor (copy {rate:.2f} TB/s) {floor:9.1f} us   "
            f"kernel / floor = {tk[0] / floor:6.2f}")
        say(f"    rasterize_batch (plan + upload + launch) {tw[0]:10.1f} us [{tw[1]:.1f}..{tw[2]:.1f}]   PIL polygon + upload "
            f"{tp[0]:10.1f} us [{tp[1]:.1f}..{tp[2]:.1f}]   PIL / rasterize_batch = {tp[0] / tw[0]:6.2f}")
        del out, other, blob
    path = os.path.join(ROOT, "profiles", "raster_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def pq():
    """Object-level evaluation through the C ABI (csrc/panoptic.hip): segk_pq_pairs and segk_pq_match on the labels
    of segk_cc_label (connectivity 4, things 1..3, stuff 0) at 256 x 256 and 3000 x 4000 -- smooth blobs against the same blobs
    shifted by (1, 2) (the realistic case) and two independent noise masks (half the pixels one of three classes: millions of
    objects and pairs at 12 MP).  max_components and max_pairs are the masks' own counts rounded up to a multiple of 4096 (read
    once, before the timing).  Per entry: device-event time, warmed, seven rounds: median and min..max; the bytes each pass must
    move (pairs: 10 B per pixel for the insert pass plus 16 B per table slot three times; match: 12 B per pair twice plus 28 B per
    segment row twice) over the device-to-device copy rate of a 512 MB buffer measured beside it (the floor); the two labellings, for scale; and the
    host path the entries replace -- both masks .cpu(), scipy.ndimage.label per thing class, np.unique of the combined ids with
    counts -- by the host clock.  Written to profiles/pq_kbench.txt (or --out)."""
    import time
    import numpy as np
    from scipy import ndimage
    from image_segmentation_amd.components import ws_ints as cc_ws
    from image_segmentation_amd.panoptic import ws_ints as pq_ws, MIN_SLOTS
    st = ops._stream()
    i32 = dict(dtype=torch.int32, device="cuda")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def rounds(fn, iters):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return t[3], t[0], t[-1]

    def blobs(H, W):
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                                indexing="ij")
        m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        for c, (cy, cx, ry, rx) in ((1, (0.35, 0.3, 0.25, 0.2)), (2, (0.65, 0.7, 0.22, 0.25))):
            d = ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2
            m[d <= 1.0] = c
            m[(d > 1.0) & (d <= 1.25)] = 3
        return m

    g = torch.Generator(device="cuda").manual_seed(0)

    def noise(H, W):
        fg = torch.rand((H, W), generator=g, device="cuda") < 0.5
        return torch.where(fg, torch.randint(1, 4, (H, W), generator=g, device="cuda", dtype=torch.uint8), torch.zeros((), dtype=torch.uint8, device="cuda"))

    up4096 = lambda n: max(4096, (n + 4095) // 4096 * 4096)
    say(f"pq: build {_lib.build_id()}, clock probe {ops.clock_probe()['median_ghz']} GHz")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None       # one size, e.g. 3000x4000
    for H, W in ((256, 256), (3000, 4000)):
        if only is not None and only != f"{H}x{W}":
            continue
        hw = H * W
        iters = 50 if hw <= 1 << 20 else 5
        for kind in ("blobs", "noise"):
            if kind == "blobs":
                tgt = blobs(H, W)
                pred = torch.roll(tgt, (1, 2), (0, 1)).contiguous()
            else:
                pred, tgt = noise(H, W), noise(H, W)
            labels, num = torch.empty((2, H, W), **i32), torch.empty((2, 4), **i32)
            ws = torch.empty(cc_ws(H, W), **i32)

            def label(side, mask, r, box, cap):
                _lib.call("segk_cc_label", mask.data_ptr(), labels[side].data_ptr(), num[side].data_ptr(), r[0].data_ptr(), r[1].data_ptr(),
                          box.data_ptr(), r[2].data_ptr(), ws.data_ptr(), H, W, 4, 0b1110, cap, st)
            r1, b1 = torch.empty((3, 1), **i32), torch.empty((1, 4), **i32)
            label(0, pred, r1, b1, 1); label(1, tgt, r1, b1, 1)       # a first call with one row only counts the components
            cap = up4096(int(num[:, 0].max().item()))
            rp, rg = torch.empty((3, cap), **i32), torch.empty((3, cap), **i32)
            bp, bg = torch.empty((cap, 4), **i32), torch.empty((cap, 4), **i32)
            f_l = lambda: (label(0, pred, rp, bp, cap), label(1, tgt, rg, bg, cap))
            f_l()
            totals = torch.empty(4, **i32)
            seg_rows = torch.empty((7, cap + 8), **i32)
            stats = torch.zeros((8, 16), dtype=torch.int64, device="cuda")

            def make(mp):
                pairs, wsp = torch.empty((3, mp), **i32), torch.empty(pq_ws(H, W, mp, cap), **i32)
                f_p = lambda: _lib.call("segk_pq_pairs", pred.data_ptr(), labels[0].data_ptr(), num[0].data_ptr(), tgt.data_ptr(),
                                        labels[1].data_ptr(), num[1].data_ptr(), pairs[0].data_ptr(), pairs[1].data_ptr(), pairs[2].data_ptr(),
                                        totals.data_ptr(), wsp.data_ptr(), H, W, 1, -1, cap, mp, st)
                f_m = lambda: _lib.call("segk_pq_match", pairs[0].data_ptr(), pairs[1].data_ptr(), pairs[2].data_ptr(), totals.data_ptr(),
                                        rp[0].data_ptr(), num[0].data_ptr(), rg[0].data_ptr(), num[1].data_ptr(),
                                        *(seg_rows[k].data_ptr() for k in range(7)), stats.data_ptr(), cap, mp, st)
                return pairs, wsp, f_p, f_m
            pairs, wsp, f_p, f_m = make(hw)                             # P <= H*W always fits: this call only counts the pairs
            f_p()
            mp = up4096(int(totals[0].item()))
            del pairs, wsp
            pairs, wsp, f_p, f_m = make(mp)
            f_p(); f_m()
            tot = totals.tolist()
            assert tot[0] > 0 and int(pairs[2][:tot[0]].sum().item()) == hw, "the pair table is not lossless"
            tl, tp, tm = rounds(f_l, iters), rounds(f_p, iters), rounds(f_m, iters)
            src, dst = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
            tc = rounds(lambda: dst.copy_(src), 5)                      # 512 MB each way: larger than the last-level cache
            rate = 2 * src.numel() / tc[0] / 1e6                        # TB/s of the copy (read + write)
            slots = 2 * mp + MIN_SLOTS
            bytes_p, bytes_m = 10 * hw + 3 * 16 * slots + 12 * tot[0], 2 * 12 * tot[0] + 2 * 28 * (cap + 8)
            floor_p, floor_m = bytes_p / (rate * 1e6), bytes_m / (rate * 1e6)
            del src, dst
            host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a, b = pred.cpu().numpy(), tgt.cpu().numpy()
                ids, base = [np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)], [0, 0]
                for side, m in enumerate((a, b)):
                    for c in (1, 2, 3):
                        lab, n = ndimage.label(m == c)
                        ids[side] += np.where(lab > 0, lab + base[side], 0)
                        base[side] += n
                    ids[side][(ids[side] == 0) & (m == 0)] = base[side] + 1
                np.unique(ids[1] * (base[0] + 2) + ids[0], return_counts=True)
                host.append((time.perf_counter() - t0) * 1e6)
            host.sort()
            say(f"pq {H}x{W} {kind:5s} K_pred={int(num[0, 0].item()):8d} K_target={int(num[1, 0].item()):8d} pairs={tot[0]:9d} matches={tot[3]:8d} "
                f"max_components={cap:8d} max_pairs={mp:9d}")
            say(f"    segk_pq_pairs {tp[0]:10.1f} us [{tp[1]:.1f}..{tp[2]:.1f}]   floor ({bytes_p / 1e6:.2f} MB at copy {rate:.2f} TB/s) {floor_p:9.1f} us   "
                f"entry / floor = {tp[0] / floor_p:7.2f}")
            say(f"    segk_pq_match {tm[0]:10.1f} us [{tm[1]:.1f}..{tm[2]:.1f}]   floor ({bytes_m / 1e6:.2f} MB) {floor_m:9.1f} us   "
                f"entry / floor = {tm[0] / floor_m:7.2f}")
            say(f"    two segk_cc_label {tl[0]:10.1f} us [{tl[1]:.1f}..{tl[2]:.1f}]   host path (2 x mask.cpu(), ndimage.label, np.unique) "
                f"{host[1]:12.1f} us [{host[0]:.1f}..{host[-1]:.1f}]   host / (labels + pairs + match) = {host[1] / (tl[0] + tp[0] + tm[0]):8.2f}")
            del pairs, wsp, labels, ws, rp, rg, bp, bg, seg_rows
    path = os.path.join(ROOT, "profiles", "pq_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def morph():
    """Mask morphology (csrc/morph.hip) through image_segmentation_amd.morph: erode, dilate, open_mask, close_mask,
    boundary_distance (disk), label_band (square) and fill_holes on a blob mask with 1 % speckle (classes 0..3, the set = 1 and 2)
    at 256 x 256 (r = 1, 3) and 3000 x 4000 (r = 3, 32).  Per operation: device-event time of its segk_morph launches through the C
    ABI (tables and outputs made before), warmed, seven rounds: median and min..max, and the median of the public call beside
    it (which checks the arguments and builds the tables' bytes on the host per call); the byte model -- per launch one read of the
    map with the halo of every tile and one byte (distance: two) written per pixel, a paint launch two more bytes read per pixel
    -- over the device-to-device copy rate of a 512 MB buffer measured beside it (the floor); and the host path of the same
    job by the host clock, the copies both ways included: mask.cpu(), scipy.ndimage (binary_erosion / binary_dilation with the
    disk up to r = 3, the exact Euclidean transform thresholded above it; maximum_filter != minimum_filter for the band;
    distance_transform_edt on both sides; binary_fill_holes), .cuda().  Written to profiles/morph_kbench.txt (or --out)."""
    import time
    import numpy as np
    import image_segmentation_amd as seg
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    from image_segmentation_amd import morph as M
    TH, TW = _lib.MORPH_TILE_H, _lib.MORPH_TILE_W
    st = ops._stream()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def rounds(fn, iters):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return t[3], t[0], t[-1]

    g = torch.Generator(device="cuda").manual_seed(0)

    def blobs(H, W):
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                                indexing="ij")
        m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        for c, (cy, cx, ry, rx) in ((1, (0.35, 0.3, 0.25, 0.2)), (2, (0.65, 0.7, 0.22, 0.25))):
            d = ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2
            m[d <= 1.0] = c
            m[(d > 1.0) & (d <= 1.25)] = 3
        hit = torch.rand((H, W), generator=g, device="cuda") < 0.01
        return torch.where(hit, torch.randint(0, 4, (H, W), generator=g, device="cuda", dtype=torch.uint8), m)

    def staged(H, W, r):
        """bytes of the map one launch reads: every tile's rows and columns with the halo, clipped to the image"""
        rows = sum(min(H, y + TH + r) - max(0, y - r) for y in range(0, H, TH))
        cols = sum(min(W, x + TW + r) - max(0, x - r) for x in range(0, W, TW))
        return rows * cols

    def disk(r):
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        return yy * yy + xx * xx <= r * r

    def host_erode(S, r):
        return ndimage.binary_erosion(S, disk(r), border_value=1) if r <= 3 else ndimage.distance_transform_edt(S) > r

    def host_dilate(S, r):
        return ndimage.binary_dilation(S, disk(r)) if r <= 3 else ndimage.distance_transform_edt(~S) <= r

    S_of = lambda a: (a == 1) | (a == 2)
    host_ops = {
        "erode": lambda a, r: np.where(S_of(a) & ~host_erode(S_of(a), r), 0, a),
        "dilate": lambda a, r: np.where(~S_of(a) & host_dilate(S_of(a), r), 1, a),
        "open_mask": lambda a, r: np.where(S_of(a) & ~host_dilate(host_erode(S_of(a), r), r), 0, a),
        "close_mask": lambda a, r: np.where(~S_of(a) & host_erode(host_dilate(S_of(a), r), r), 1, a),
        "boundary_distance": lambda a, r: np.where(S_of(a), ndimage.distance_transform_edt(S_of(a)), ndimage.distance_transform_edt(~S_of(a))),
        "label_band": lambda a, r: np.where(ndimage.maximum_filter(a, 2 * r + 1) != ndimage.minimum_filter(a, 2 * r + 1), 255, a),
    }
    say(f"morph: build {_lib.build_id()}, clock probe {ops.clock_probe()['median_ghz']} GHz, tile {TH} x {TW}"
        + ("" if ndimage is not None else ", scipy not installed: no host path"))
    src, dst = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    tc = rounds(lambda: dst.copy_(src), 5)                          # 512 MB each way: larger than the last-level cache
    rate = 2 * src.numel() / tc[0] / 1e6                            # TB/s of the copy (read + write)
    del src, dst
    say(f"morph: device-to-device copy of 512 MB: {rate:.2f} TB/s")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None       # one size, e.g. 3000x4000
    for (H, W), radii in (((256, 256), (1, 3)), ((3000, 4000), (3, 32))):
        if only is not None and only != f"{H}x{W}":
            continue
        hw = H * W
        iters, host_rounds = (50, 3) if hw <= 1 << 20 else (5, 1)
        x = blobs(H, W)
        for r in radii:
            calls = [("erode", dict(classes=(1, 2), radius=r, fill=0), 1, 1, 0),
                     ("dilate", dict(classes=(1, 2), radius=r, value=1), 1, 1, 0),
                     ("open_mask", dict(classes=(1, 2), radius=r, fill=0), 2, 1, 1),
                     ("close_mask", dict(classes=(1, 2), radius=r, value=1), 2, 1, 1),
                     ("boundary_distance", dict(max_radius=r, classes=(1, 2)), 1, 2, 0),
                     ("label_band", dict(width=r, shape="square"), 1, 1, 0)]
            for name, kw, launches, item, paints in calls:
                fn = getattr(seg, name)
                plan = {"erode": M._erode_plan, "dilate": M._dilate_plan, "open_mask": M._open_plan, "close_mask": M._close_plan,
                        "boundary_distance": M._distance_plan, "label_band": M._band_plan}[name](**kw)
                tabs = [M._tables_on(x.device, st, s.tables) for s in plan]
                mid, out = torch.empty_like(x), torch.empty((H, W), dtype=torch.uint16 if item == 2 else torch.uint8, device="cuda")

                def entry():                                        # the launches of the operation, nothing else
                    for k, (s, tab) in enumerate(zip(plan, tabs)):
                        dst = out if k == len(plan) - 1 else mid
                        _lib.call("segk_morph", (mid if k else x).data_ptr(), x.data_ptr() if s.paint else 0, 0 if item == 2 else dst.data_ptr(),
                                  dst.data_ptr() if item == 2 else 0, tab.data_ptr(), tab.data_ptr() + 512, s.value, s.metric, s.radius, H, W, st)
                entry()
                assert torch.equal(out, fn(x, **kw)), name
                t = rounds(entry, iters)
                tcall = rounds(lambda: fn(x, **kw), iters)[0]
                nbytes = launches * (staged(H, W, r) + hw + item * hw) + paints * hw    # halo read, the pixel's own byte again, the output
                floor = nbytes / (rate * 1e6)
                line = (f"morph {H}x{W} r={r:2d} {name:17s} {t[0]:9.1f} us [{t[1]:.1f}..{t[2]:.1f}]   floor ({nbytes / 1e6:7.2f} MB) {floor:7.1f} us   "
                        f"entry / floor = {t[0] / floor:7.2f}   public call {tcall:8.1f} us")
                if ndimage is not None:
                    host = []
                    for _ in range(host_rounds):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res = host_ops[name](x.cpu().numpy(), r)
                        out = torch.from_numpy(res if name == "boundary_distance" else res.astype(np.uint8, copy=False)).cuda()
                        torch.cuda.synchronize()
                        host.append((time.perf_counter() - t0) * 1e6)
                        del out
                    host.sort()
                    line += f"   host {host[len(host) // 2]:12.1f} us   host / entry = {host[len(host) // 2] / t[0]:9.1f}"
                say(line)
        cap = 1 << 20
        f = lambda: seg.fill_holes(x, (1, 2), value=1, max_components=cap)
        res = f()
        t = rounds(f, iters)
        line = (f"morph {H}x{W}      fill_holes        {t[0]:9.1f} us [{t[1]:.1f}..{t[2]:.1f}]   components {int(res.num)} filled {int(res.filled)} "
                f"(byte table + segk_cc_label + fill pass)")
        if ndimage is not None:
            host = []
            for _ in range(host_rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a = x.cpu().numpy()
                out = torch.from_numpy(np.where(ndimage.binary_fill_holes(S_of(a)) & ~S_of(a), 1, a).astype(np.uint8)).cuda()
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e6)
            host.sort()
            line += f"   host {host[len(host) // 2]:12.1f} us   host / entry = {host[len(host) // 2] / t[0]:9.1f}"
        say(line)
        del x
    path = os.path.join(ROOT, "profiles", "morph_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def boundary():
    """Boundary quality (csrc/boundary.hip): segk_boundary_stats + segk_boundary_finish through the C ABI on the
    blob masks with 1 % speckle of the morph bench (the label) and the same blobs moved by (2, 3) with a speckle of their own (the
    prediction), four classes, at 256 x 256 and 3000 x 4000, width 2 and 7, square band, max_distance 32.  Device events, warmed,
    seven rounds: median and min..max.  Beside it (1) the yardstick: the route that exists without the fused kernel -- two
    seg.boundary_distance launches plus the torch comparisons and bincounts that form the band counts ALONE (no confusion, no
    contours, no histogram); the tool checks that its counts are the fused kernel's; (2) the byte floor, 2 bytes read per pixel
    over the device-to-device copy rate of a 512 MB buffer; (3) the host path by the host clock: mask.cpu() and scipy.ndimage
    (binary_erosion for the bands, distance_transform_edt of the complement of each contour set, histograms of the ceilings).
    Written to profiles/boundary_kbench.txt (or --out)."""
    import time
    import numpy as np
    import image_segmentation_amd as seg
    from image_segmentation_amd import boundary as B
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    C, R = 4, 32
    st = ops._stream()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def rounds(fn, iters):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return t[3], t[0], t[-1]

    g = torch.Generator(device="cuda").manual_seed(0)

    def speckled(m):
        hit = torch.rand(m.shape, generator=g, device="cuda") < 0.01
        return torch.where(hit, torch.randint(0, 4, m.shape, generator=g, device="cuda", dtype=torch.uint8), m)

    def blobs(H, W):
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                                indexing="ij")
        m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        for c, (cy, cx, ry, rx) in ((1, (0.35, 0.3, 0.25, 0.2)), (2, (0.65, 0.7, 0.22, 0.25))):
            d = ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2
            m[d <= 1.0] = c
            m[(d > 1.0) & (d <= 1.25)] = 3
        return m

    def host(pred, label, w):
        """the scipy route: the same integers as the device's, every class, both maps"""
        p, l = pred.cpu().numpy(), label.cpu().numpy()
        sq = np.ones((3, 3), dtype=bool)
        out = []
        for c in range(C):
            A, Q = l == c, p == c
            bg, bp = A & ~ndimage.binary_erosion(A, sq, iterations=w, border_value=1), Q & ~ndimage.binary_erosion(Q, sq, iterations=w, border_value=1)
            K = []
            for M in (A, Q):
                o = ~M
                near = np.zeros_like(M)
                near[1:] |= o[:-1]; near[:-1] |= o[1:]; near[:, 1:] |= o[:, :-1]; near[:, :-1] |= o[:, 1:]
                K.append(M & near)
            hist = []
            for src, dst in ((K[1], K[0]), (K[0], K[1])):
                d = np.ceil(ndimage.distance_transform_edt(~dst)[src] - 1e-9).astype(np.int64) if dst.any() else np.full(int(src.sum()), R + 1)
                hist.append(np.bincount(np.minimum(d, R + 1), minlength=R + 2))
            out.append((int(bg.sum()), int(bp.sum()), int((bg & bp).sum()), hist))
        return out

    say(f"boundary: build {_lib.build_id()}, clock probe {ops.clock_probe()['median_ghz']} GHz, tile {_lib.BOUNDARY_TILE_H} x {_lib.BOUNDARY_TILE_W}, "
        f"{C} classes, max_distance {R}" + ("" if ndimage is not None else ", scipy not installed: no host path"))
    src, dst = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    tc = rounds(lambda: dst.copy_(src), 5)
    rate = 2 * src.numel() / tc[0] / 1e6                            # TB/s of the copy (read + write)
    del src, dst
    say(f"boundary: device-to-device copy of 512 MB: {rate:.2f} TB/s")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None       # one size, e.g. 3000x4000
    for H, W in ((256, 256), (3000, 4000)):
        if only is not None and only != f"{H}x{W}":
            continue
        iters = 50 if H * W <= 1 << 20 else 5
        base = blobs(H, W)
        label, pred = speckled(base), speckled(torch.roll(base, (2, 3), (0, 1)))
        for w in (2, 7):
            acc = B.BoundaryStats.zeros(C, R, "cuda")

            def fused():
                _lib.call("segk_boundary_stats", pred.data_ptr(), label.data_ptr(), acc.words.data_ptr(), acc.image_hist.data_ptr(), C, 0, 0, w, R,
                          0, H, W, st)
                _lib.call("segk_boundary_finish", acc.words.data_ptr(), acc.image_hist.data_ptr(), C, R, st)

            def route():                                            # what forms band_g / band_p / band_i without the fused kernel
                dg = seg.boundary_distance(label, w, shape="square").view(torch.int16) != -1
                dp = seg.boundary_distance(pred, w, shape="square").view(torch.int16) != -1
                return (torch.bincount(label[dg].long(), minlength=C), torch.bincount(pred[dp].long(), minlength=C),
                        torch.bincount(label[dg & dp & (label == pred)].long(), minlength=C))

            one = seg.boundary_stats(pred, label, C, w, R, image_border=False)
            for got, want in zip(route(), (one.band_g, one.band_p, one.band_i)):
                assert torch.equal(got, want[:C]), "the yardstick and the fused kernel disagree"
            t, ty = rounds(fused, iters), rounds(route, iters)
            tcall = rounds(lambda: seg.boundary_stats(pred, label, C, w, R, image_border=False, out=acc), iters)[0]
            floor = 2 * H * W / (rate * 1e6)
            line = (f"boundary {H}x{W} width={w} stats+finish {t[0]:9.1f} us [{t[1]:.1f}..{t[2]:.1f}]   yardstick (2 distance launches + torch "
                    f"band counts) {ty[0]:9.1f} us [{ty[1]:.1f}..{ty[2]:.1f}]   yardstick / fused = {ty[0] / t[0]:6.2f}   floor ({2 * H * W / 1e6:6.2f} MB) "
                    f"{floor:6.2f} us   fused / floor = {t[0] / floor:7.1f}   public call {tcall:8.1f} us")
            if ndimage is not None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = host(pred, label, w)
                th = (time.perf_counter() - t0) * 1e6
                hist = one.hist.cpu().numpy()
                for c, (bg, bp, bi, hh) in enumerate(res):
                    assert (bg, bp, bi) == (int(one.band_g[c]), int(one.band_p[c]), int(one.band_i[c])), "scipy and the device disagree on the band"
                    assert np.array_equal(hh[0], hist[0, c]) and np.array_equal(hh[1], hist[1, c]), "scipy and the device disagree on the contours"
                line += f"   host {th:12.1f} us   host / fused = {th / t[0]:9.1f}"
            say(line)
        del base, label, pred
    path = os.path.join(ROOT, "profiles", "boundary_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def slic():
    """Superpixels (csrc/slic.hip) at 256 x 256 and 3000 x 4000 on an RGB image of smooth colour fields with
    noise, step 16, compactness 20, "ycc", 10 iterations: segk_slic_assign alone (a middle round: no labels written, and the
    last one), a whole seg.superpixels call (21 launches), and vote + snap (seg.snap_mask on a four-class blob mask moved by
    two pixels, weighted).  Device events, warmed, seven rounds: median and min..max.  Beside it the byte floor of a whole call
    -- the image read T times plus the labels written once, over the device-to-device copy rate of a 512 MB buffer -- and the
    pixels x candidates per second of the assign kernel.  Written to profiles/slic_kbench.txt (or --out)."""
    import image_segmentation_amd as seg
    S, m, T, space = 16, 20, 10, "ycc"
    st = ops._stream()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def rounds(fn, iters):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return t[3], t[0], t[-1]

    g = torch.Generator(device="cuda").manual_seed(0)

    def picture(H, W):
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                                indexing="ij")
        chans = [128 + 100 * torch.sin(yy / (0.07 * H) + k) * torch.cos(xx / (0.05 * W) - k) for k in range(3)]
        img = torch.stack(chans, dim=-1) + 12 * torch.randn((H, W, 3), generator=g, device="cuda")
        mask = ((torch.sin((yy + 2) / (0.07 * H)) > 0).to(torch.uint8) + 2 * (torch.cos(xx / (0.05 * W)) > 0).to(torch.uint8))
        return img.clamp(0, 255).to(torch.uint8).contiguous(), torch.roll(mask, 2, 1).contiguous()

    say(f"slic: build {_lib.build_id()}, clock probe {ops.clock_probe()['median_ghz']} GHz, tile {_lib.SLIC_TILE} x {_lib.SLIC_TILE}, step {S}, "
        f"compactness {m}, {space}, {T} iterations")
    src, dst = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    tc = rounds(lambda: dst.copy_(src), 5)
    rate = 2 * src.numel() / tc[0] / 1e6                            # TB/s of the copy (read + write)
    del src, dst
    say(f"slic: device-to-device copy of 512 MB: {rate:.2f} TB/s")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None       # one size, e.g. 3000x4000
    for H, W in ((256, 256), (3000, 4000)):
        if only is not None and only != f"{H}x{W}":
            continue
        iters = 50 if H * W <= 1 << 20 else 5
        img, mask = picture(H, W)
        sp = seg.superpixels(img, S, m, T, space)
        conf = torch.randint(0, 256, (H, W), generator=g, device="cuda", dtype=torch.uint8)
        K = sp.k
        sums = torch.zeros((K, _lib.SLIC_SUM_WORDS), dtype=torch.int32, device="cuda")
        labels = torch.empty((H, W), dtype=torch.int32, device="cuda")

        SP = sys.modules["image_segmentation_amd.superpixels"]
        chosen = SP.tile_rows(H, W)

        def assign(rnd, rows):
            def f():                                                # on the converged centres; the sums grow, which costs the same
                _lib.call("segk_slic_assign", img.data_ptr(), sp.centres.data_ptr(), sums.data_ptr(), labels.data_ptr(), 3,
                          _lib.SLIC_SPACES[space], S, m, rnd, T, rows, H, W, K, st)
            return f
        ta, tl = rounds(assign(0, chosen), iters), rounds(assign(T - 1, chosen), iters)
        per_rows = "  ".join(f"{rows} rows {rounds(assign(0, rows), iters)[0]:.1f} us" for rows in _lib.SLIC_TILE_ROWS)
        say(f"slic {H}x{W} assign by tile height (the host layer takes {chosen}): {per_rows}")
        tcall = rounds(lambda: seg.superpixels(img, S, m, T, space), max(iters // 5, 2))
        tsnap = rounds(lambda: seg.snap_mask(mask, sp, min_share=0.5, weights=conf), iters)
        floor = (T * 3 + 4) * H * W / (rate * 1e6)
        say(f"slic {H}x{W} K={K}  assign {ta[0]:9.1f} us [{ta[1]:.1f}..{ta[2]:.1f}] = {9 * H * W / ta[0] / 1e3:7.2f} G candidates/s   assign + labels "
            f"{tl[0]:9.1f} us [{tl[1]:.1f}..{tl[2]:.1f}]   superpixels() {tcall[0]:9.1f} us [{tcall[1]:.1f}..{tcall[2]:.1f}]   byte floor "
            f"({(T * 3 + 4) * H * W / 1e6:7.2f} MB) {floor:7.2f} us   call / floor = {tcall[0] / floor:7.1f}   snap_mask (vote + winner + paint) "
            f"{tsnap[0]:9.1f} us [{tsnap[1]:.1f}..{tsnap[2]:.1f}]")
        del img, mask, sp, conf, sums, labels
    path = os.path.join(ROOT, "profiles", "slic_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def mix():
    """Mixed-sample augmentation (csrc/mix.hip) through image_segmentation_amd.mix at the bench batch, B = 32,
    3 x 256 x 256, int64 labels: float32 NCHW and uint8 NHWC images, each mode (every sample mixed, flips drawn, shifts for
    copy_paste), with and without a seam.  Per line: device-event time of the segk_mix_apply launch alone (tables, id maps and
    outputs made before), warmed, seven rounds: median and min..max; the launches in front of it (segk_mix_select, and for
    copy_paste the byte stage and one segk_cc_label per partner); the public call (plans checked and the descriptor table
    uploaded per call); the byte model -- read one image and the deciding map (labels; for copy_paste the id map too), write
    image and label -- over the device-to-device copy rate of a 512 MB buffer measured beside it (the floor); and the equivalent
    torch expression (index, flip, roll, where) on the same tensors, checked to give the same result.  Written to
    profiles/mix_kbench.txt (or --out)."""
    import numpy as np
    import image_segmentation_amd as seg
    from image_segmentation_amd import mix as M
    st = ops._stream()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def rounds(fn, iters):
        t = sorted(timeit(fn, iters) for _ in range(7))
        return t[3], t[0], t[-1]

    B, C, H, W, cap = 32, 3, 256, 256, 1024
    say(f"mix: build {_lib.build_id()}, clock probe {ops.clock_probe()['median_ghz']} GHz, tile {_lib.MIX_TILE_H} x {_lib.MIX_TILE_W}, "
        f"B = {B}, {C} x {H} x {W}, int64 labels")
    src, dst = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    tc = rounds(lambda: dst.copy_(src), 5)                          # 512 MB each way: larger than the last-level cache
    rate = 2 * src.numel() / tc[0] / 1e6                            # TB/s of the copy (read + write)
    del src, dst
    say(f"mix: device-to-device copy of 512 MB: {rate:.2f} TB/s")
    g = torch.Generator(device="cuda").manual_seed(0)
    # label maps: four classes in cells of 32 x 32 with 1 % speckle
    cells = torch.randint(0, 4, (B, 1, H // 32, W // 32), generator=g, device="cuda")
    y = cells.repeat_interleave(32, 2).repeat_interleave(32, 3)
    hit = torch.rand((B, 1, H, W), generator=g, device="cuda") < 0.01
    y = torch.where(hit, torch.randint(0, 4, (B, 1, H, W), generator=g, device="cuda"), y).contiguous()
    yy = torch.arange(H, device="cuda").view(1, 1, H, 1)
    xx = torch.arange(W, device="cuda").view(1, 1, 1, W)

    def torch_mix(X, plans, sel, ids, seam, nhwc):
        dev = X.device
        col = lambda f: torch.tensor([f(p) for p in plans], device=dev).view(B, 1, 1, 1)
        partner = torch.tensor([p.partner for p in plans], device=dev)
        flip = col(lambda p: p.flip).bool()
        Xp, yp = X[partner], y[partner]
        Xp = torch.where(flip, Xp.flip(2 if nhwc else 3), Xp)
        yp = torch.where(flip, yp.flip(3), yp)
        idp = None
        if ids is not None:
            idp = ids[torch.tensor([int(d) for d in M_slots], device=dev)].view(B, 1, H, W)
            idp = torch.where(flip, idp.flip(3), idp)
        if any(p.dy or p.dx for p in plans):
            Xp, yp = Xp.clone(), yp.clone()
            for b, p in enumerate(plans):
                Xp[b] = torch.roll(Xp[b], (p.dy, p.dx), dims=(0, 1) if nhwc else (1, 2))
                yp[b] = torch.roll(yp[b], (p.dy, p.dx), dims=(1, 2))
                if idp is not None:
                    idp[b] = torch.roll(idp[b], (p.dy, p.dx), dims=(1, 2))
        dy, dx = col(lambda p: p.dy), col(lambda p: p.dx)
        m = (yy >= dy) & (yy < H + dy) & (xx >= dx) & (xx < W + dx)
        mode = plans[0].mode
        if mode == M.BOX:
            m = m & (yy >= col(lambda p: p.box[0])) & (yy < col(lambda p: p.box[2])) & (xx >= col(lambda p: p.box[1])) & (xx < col(lambda p: p.box[3]))
        elif mode == M.CLASS:
            m = m & (yp >= 0) & (yp <= 255) & torch.gather(sel, 1, yp.clamp(0, 255).view(B, -1)).view(B, 1, H, W).bool()
        else:
            m = m & (idp >= 1) & (idp <= cap) & torch.gather(sel, 1, (idp.long() - 1).clamp(0, cap - 1).view(B, -1)).view(B, 1, H, W).bool()
        Xo = torch.where(m.view(B, H, W, 1) if nhwc else m, Xp, X)
        yo = torch.where(m, yp, y)
        if seam is not None:
            s = torch.zeros_like(m)
            s[:, :, 1:] |= m[:, :, 1:] != m[:, :, :-1]
            s[:, :, :-1] |= m[:, :, :-1] != m[:, :, 1:]
            s[:, :, :, 1:] |= m[:, :, :, 1:] != m[:, :, :, :-1]
            s[:, :, :, :-1] |= m[:, :, :, :-1] != m[:, :, :, 1:]
            yo = torch.where(s, torch.full_like(yo, seam), yo)
        return Xo, yo, m.sum((1, 2, 3)).int()

    for name, X in (("float32", torch.rand((B, C, H, W), generator=g, device="cuda")),
                    ("uint8  ", torch.randint(0, 256, (B, H, W, C), generator=g, device="cuda", dtype=torch.uint8))):
        nhwc = X.dtype == torch.uint8
        for mode in ("cutmix", "classmix", "copy_paste"):
            for seam in (None, 255):
                mixer = seg.Mixer(mode, p=1.0, seam_value=seam, flip=True, max_shift=0.25, min_area=64, max_components=cap, seed=0)
                plans = mixer.plan(B, H, W)
                Xo, yo = mixer.apply(X, y, plans)
                last = mixer.last                                   # its launches point into last["tables"], kept alive here
                pasted = last["pasted"].clone()
                front = [l for l in last["launches"] if l[0] != "segk_mix_apply"]
                apply_args = [l for l in last["launches"] if l[0] == "segk_mix_apply"][0][1]
                scratch = torch.zeros((B,), dtype=torch.int32, device="cuda")
                args = list(apply_args)
                args[6] = scratch.data_ptr()                        # pasted is added to: the timed launches add elsewhere
                t = rounds(lambda: _lib.call("segk_mix_apply", *args), 50)
                tf = rounds(lambda: [_lib.call(n, *a) for n, a in front], 20)[0] if front else 0.0
                tcall = rounds(lambda: mixer.apply(X, y, plans), 20)[0]
                sel = last["tables"][1].long() if mode != "cutmix" else None
                ids = last["tables"][2] if mode == "copy_paste" else None
                M_slots = [int(d) for d in np.frombuffer(last["tables"][0][:64 * B].cpu().numpy().tobytes(), dtype=M.DESC)["slot"]]
                expr = lambda: torch_mix(X, plans, sel, ids, seam, nhwc)
                Xt, yt, pt = expr()
                same = torch.equal(Xt.view(torch.uint8), Xo.view(torch.uint8)) and torch.equal(yt, yo) and torch.equal(pt, pasted)
                tt = rounds(expr, 10)[0]
                img = B * C * H * W * X.element_size()
                nbytes = 2 * img + 2 * B * H * W * 8 + (B * H * W * 4 if mode == "copy_paste" else 0)
                floor = nbytes / (rate * 1e6)
                say(f"mix {name} {mode:10s} seam {str(seam):4s} apply {t[0]:8.1f} us [{t[1]:.1f}..{t[2]:.1f}]   floor ({nbytes / 1e6:6.2f} MB) {floor:6.1f} us   "
                    f"apply / floor = {t[0] / floor:5.2f}   select stage {tf:8.1f} us   public call {tcall:8.1f} us   torch {tt:9.1f} us "
                    f"({'same result' if same else 'RESULT DIFFERS'})   torch / apply = {tt / t[0]:6.1f}   pasted {int(pasted.sum()) / (B * H * W):.2f}")
    path = os.path.join(ROOT, "profiles", "mix_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def tta():
    """Multi-view prediction through the C ABI (csrc/predict.hip): segk_predict_merge -- mask, colour, class
    counts and confidence in one pass -- at 1200 x 1600, C = 4, V = 1, 2 and 6 views (224 x 224 slots, flips cycling, equal
    weights, "prob" merge of logits) against the materialised route it replaces: per view segk_crop_resize to full-size fp32
    logits, torch.flip, softmax and a running weighted sum, then argmax, the confidence and segk_mask_finish.  Beside the
    V = 1 line: segk_predict_mask on the same slot.  Both routes run in this process, alternating, seven rounds each: median
    and min..max.  Also written to profiles/kbench_tta.json (or the file given with --out)."""
    import json
    import numpy as np
    from image_segmentation_amd import tta as T_
    from image_segmentation_amd.utils import _geometry
    T, C, oh, ow = 224, 4, 1200, 1600
    st = ops._stream()
    nh, nw, pt, pl, _ = _geometry(oh, ow, T)
    pal = torch.tensor([(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)], dtype=torch.uint8, device="cuda")
    mask, conf = (torch.empty((oh, ow), dtype=torch.uint8, device="cuda") for _ in range(2))
    color = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    full = torch.empty((C, oh, ow), device="cuda")
    dims = {0: (), 1: (-1,), 2: (-2,), 3: (-2, -1)}

    def rounds(fns, iters=50):
        ts = [[] for _ in fns]
        for _ in range(7):
            for t, fn in zip(ts, fns):
                t.append(timeit(fn, iters))
        return [{"median": sorted(t)[3], "min": min(t), "max": max(t)} for t in ts]

    rows = []
    for V in (1, 2, 6):
        slots = [torch.randn((C, T, T), device="cuda") for _ in range(V)]
        table = T_.view_table([(s.data_ptr(), T, pt, pl, nh, nw, v % 4, 0, 1.0) for v, s in enumerate(slots)])
        weights = [torch.tensor(w, device="cuda") for w in table["weight"]]
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()

        def fused():
            _lib.call("segk_predict_merge", dev.data_ptr(), V, C, 0, 0, oh, ow, mask.data_ptr(), color.data_ptr(), pal.data_ptr(),
                      counts.data_ptr(), None, None, conf.data_ptr(), None, st)

        def old():
            acc = None
            for v, s in enumerate(slots):
                _lib.call("segk_crop_resize", s.data_ptr(), full.data_ptr(), C, T, pt, pl, nh, nw, oh, ow, 0, st)
                p = weights[v] * torch.softmax(torch.flip(full, dims[v % 4]) if v % 4 else full, 0)
                acc = p if acc is None else acc + p
            m = acc.argmax(0).to(torch.uint8)
            cf = (255 * (acc.max(0).values / acc.sum(0)) + 0.5).to(torch.uint8)
            _lib.call("segk_mask_finish", m.data_ptr(), color.data_ptr(), pal.data_ptr(), counts.data_ptr(), None, None, C, oh, ow, st)
            return m, cf

        def single():
            _lib.call("segk_predict_mask", slots[0].data_ptr(), mask.data_ptr(), color.data_ptr(), pal.data_ptr(), counts.data_ptr(),
                      None, None, C, T, pt, pl, nh, nw, oh, ow, 0, st)
        m_old, cf_old = old()
        fused()
        differ = int((mask != m_old).sum())
        conf_off = int((conf.int() - cf_old.int()).abs().max())
        fns = [fused, old] + ([single] if V == 1 else [])
        res = rounds(fns)
        row = {"V": V, "size": [oh, ow], "C": C, "T": T, "predict_merge_us": res[0], "materialised_us": res[1],
               "mask_pixels_differing": differ, "confidence_max_difference": conf_off}
        line = (f"tta {oh}x{ow} C={C} V={V}  segk_predict_merge {res[0]['median']:8.1f} us [{res[0]['min']:.1f}..{res[0]['max']:.1f}]   "
                f"materialised {res[1]['median']:9.1f} us [{res[1]['min']:.1f}..{res[1]['max']:.1f}]   "
                f"{res[1]['median'] / res[0]['median']:5.1f}x   mask pixels differing {differ}, confidence off by <= {conf_off}")
        if V == 1:
            row["predict_mask_us"] = res[2]
            line += f"   segk_predict_mask {res[2]['median']:8.1f} us [{res[2]['min']:.1f}..{res[2]['max']:.1f}]"
        rows.append(row)
        print(line)
    clk = ops.clock_probe()
    path = os.path.join(ROOT, "profiles", "kbench_tta.json")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        json.dump({"rows": rows, "clock_probe_ghz": clk["median_ghz"], "build_id": _lib.build_id()}, f, indent=1)
    print(f"tta clock probe: median {clk['median_ghz']} GHz; written to {path}")


def tiles():
    """Tiled full-resolution prediction through the C ABI (csrc/tiles.hip) at 1200 x 1600, C = 4, T = 256,
    overlap 64, triangle window, "prob" merge of logits: segk_tile_gather_u8 of the whole plan plus segk_predict_tiles (mask,
    colour, class counts and confidence in one pass) against the materialised torch route they replace: crop / pad every tile
    out of the image, per-tile softmax, weighted add into full-size fp32 accumulators, divide, argmax, the confidence and
    segk_mask_finish.  The network forward between the two halves is the same for both routes and left out.  Both routes run
    in this process, alternating, seven rounds each: median and min..max.  Written to profiles/kbench_tiles.txt and .json (or
    the .json given with --out, the .txt beside it)."""
    import json
    from image_segmentation_amd import tiles as T_
    H, W, C, T, o = 1200, 1600, 4, 256, 64
    st = ops._stream()
    ys, xs = T_.tile_axis(H, T, o), T_.tile_axis(W, T, o)
    n = len(ys) * len(xs)
    pal = torch.tensor([(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)], dtype=torch.uint8, device="cuda")
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
    Y = torch.randn((n, C, T, T), device="cuda")
    X = torch.empty((n, 3, T, T), device="cuda")
    mask, conf = (torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(2))
    color = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    u = torch.arange(T, device="cuda")
    wa = (torch.minimum(u, T - 1 - u) + 1).float()
    w2 = wa[:, None] * wa[None, :]

    def gather():
        _lib.call("segk_tile_gather_u8", img.data_ptr(), X.data_ptr(), 3, H, W, T, o, 1, 0, n, st)

    def blend():
        _lib.call("segk_predict_tiles", Y.data_ptr(), C, 0, 0, 1, H, W, T, o, mask.data_ptr(), color.data_ptr(), pal.data_ptr(),
                  counts.data_ptr(), None, None, conf.data_ptr(), None, st)

    def fused():
        gather()
        blend()

    def old_gather():
        chw = img.permute(2, 0, 1).float() / 255.0
        return torch.stack([chw[:, y:y + T, x:x + T] for y in ys for x in xs])

    def old_blend():
        acc = torch.zeros((C, H, W), device="cuda")
        t = 0
        for y in ys:
            for x in xs:
                acc[:, y:y + T, x:x + T] += w2 * torch.softmax(Y[t], 0)
                t += 1
        p = acc / acc.sum(0, keepdim=True)
        m = p.argmax(0).to(torch.uint8)
        cf = (255 * p.max(0).values + 0.5).to(torch.uint8)
        _lib.call("segk_mask_finish", m.data_ptr(), color.data_ptr(), pal.data_ptr(), counts.data_ptr(), None, None, C, H, W, st)
        return m, cf

    def old():
        old_gather()
        return old_blend()

    def rounds(fns, iters=20):
        ts = [[] for _ in fns]
        for _ in range(7):
            for t, fn in zip(ts, fns):
                t.append(timeit(fn, iters))
        return [{"median": sorted(t)[3], "min": min(t), "max": max(t)} for t in ts]

    m_old, cf_old = old()
    fused()
    torch.cuda.synchronize()
    differ = int((mask != m_old).sum())
    conf_off = int((conf.int() - cf_old.int()).abs().max())
    tiles_equal = bool(torch.equal(X, old_gather()))
    names = ["fused", "materialised", "segk_tile_gather_u8", "segk_predict_tiles", "torch crop/pad", "torch blend"]
    res = dict(zip(names, rounds([fused, old, gather, blend, old_gather, old_blend])))
    clk = ops.clock_probe()
    lines = [f"tiles {H}x{W} C={C} T={T} overlap={o} ({len(ys)} x {len(xs)} = {n} tiles), triangle window, prob merge of logits"]
    lines += [f"  {k:22s} {v['median']:9.1f} us [{v['min']:.1f}..{v['max']:.1f}]" for k, v in res.items()]
    lines += [f"  materialised / fused   {res['materialised']['median'] / res['fused']['median']:9.1f} x",
              f"  mask pixels differing {differ} of {H * W}, confidence off by <= {conf_off}, gathered tiles equal: {tiles_equal}",
              f"  clock probe: median {clk['median_ghz']} GHz; build {_lib.build_id()}"]
    print("\n".join(lines))
    path = os.path.join(ROOT, "profiles", "kbench_tiles.json")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        json.dump({"size": [H, W], "C": C, "T": T, "overlap": o, "tiles": [len(ys), len(xs)], "us": res,
                   "mask_pixels_differing": differ, "confidence_max_difference": conf_off, "gathered_tiles_equal": tiles_equal,
                   "clock_probe_ghz": clk["median_ghz"], "build_id": _lib.build_id()}, f, indent=1)
    with open(os.path.splitext(path)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def calib():
    """Confidence calibration through the C ABI (csrc/calib.hip) at 1200 x 1600, C = 4, one 224 x 224 slot:
    segk_calib_temps at K = 1 and K = 17 (the default grid) and segk_calib_hist on the mask and confidence of the same slot,
    each on a PEAKED field (every pixel favours one class by 10: almost everything lands in q = 255) and a FLAT one (white
    noise of scale 1).  The yardstick is segk_predict_merge at V = 1 ("prob", mask and confidence only) on the same slot,
    in this process, alternating, seven rounds each: median and min..max.  Also written to profiles/kbench_calib.json (or
    the file given with --out) and the lines to the .txt beside it."""
    import json
    import numpy as np
    from image_segmentation_amd import tta as T_, calibration
    from image_segmentation_amd.utils import _geometry
    T, C, oh, ow = 224, 4, 1200, 1600
    st = ops._stream()
    nh, nw, pt, pl, _ = _geometry(oh, ow, T)
    mask, conf = (torch.empty((oh, ow), dtype=torch.uint8, device="cuda") for _ in range(2))
    g = torch.Generator(device="cuda").manual_seed(0)
    lab = torch.randint(0, C, (oh, ow), device="cuda", generator=g)
    inv = torch.from_numpy(calibration.inverse_temperatures(calibration.default_temperatures())).cuda()
    acc = torch.zeros(17 * 512 + 2 * 17 + 1, dtype=torch.int64, device="cuda")
    hist, nll, nonf, valid = acc[:17 * 512], acc[17 * 512:17 * 513], acc[17 * 513:17 * 514], acc[17 * 514:]
    hist8 = torch.zeros((8, 256, 2), dtype=torch.int64, device="cuda")

    def rounds(fns, iters=50):
        ts = [[] for _ in fns]
        for _ in range(7):
            for t, fn in zip(ts, fns):
                t.append(timeit(fn, iters))
        return [{"median": sorted(t)[3], "min": min(t), "max": max(t)} for t in ts]

    rows, lines = [], []
    for name in ("peaked", "flat"):
        slot = torch.randn((C, T, T), device="cuda", generator=g)
        if name == "peaked":
            slot = 0.1 * slot + 10.0 * torch.nn.functional.one_hot(torch.randint(0, C, (T // 8, T // 8), device="cuda", generator=g), C) \
                .permute(2, 0, 1).repeat_interleave(8, 1).repeat_interleave(8, 2).float()
            slot = slot.contiguous()
        table = T_.view_table([(slot.data_ptr(), T, pt, pl, nh, nw, 0, 0, 1.0)])
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()

        def merge():
            _lib.call("segk_predict_merge", dev.data_ptr(), 1, C, 0, 0, oh, ow, mask.data_ptr(), None, None, None, None, None,
                      conf.data_ptr(), None, st)

        def temps(K, first):
            def f():
                _lib.call("segk_calib_temps", slot.data_ptr(), C, T, pt, pl, nh, nw, oh, ow, 0, lab.data_ptr(), -1,
                          inv.data_ptr() + 4 * first, K, hist.data_ptr(), nll.data_ptr(), nonf.data_ptr(), valid.data_ptr(), st)
            return f

        def hist_entry():
            _lib.call("segk_calib_hist", conf.data_ptr(), mask.data_ptr(), lab.data_ptr(), oh, ow, C, -1, hist8.data_ptr(), st)
        merge()
        acc.zero_()
        temps(1, 8)()
        torch.cuda.synchronize()
        top = int(hist[255 * 2]) / (oh * ow)
        res = dict(zip(["segk_predict_merge V=1", "segk_calib_temps K=1", "segk_calib_temps K=17", "segk_calib_hist"],
                       rounds([merge, temps(1, 8), temps(17, 0), hist_entry])))
        rows.append({"field": name, "size": [oh, ow], "C": C, "T": T, "share_in_top_bin_at_T1": top, "us": res})
        lines.append(f"calib {oh}x{ow} C={C} T={T} {name} field ({top:.3f} of the pixels in q = 255 at 1/T = 1)")
        lines += [f"  {k:24s} {v['median']:9.1f} us [{v['min']:.1f}..{v['max']:.1f}]" for k, v in res.items()]
    clk = ops.clock_probe()
    lines.append(f"  clock probe: median {clk['median_ghz']} GHz; build {_lib.build_id()}")
    print("\n".join(lines))
    path = os.path.join(ROOT, "profiles", "kbench_calib.json")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        json.dump({"rows": rows, "clock_probe_ghz": clk["median_ghz"], "build_id": _lib.build_id()}, f, indent=1)
    with open(os.path.splitext(path)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


def optim():
    """The optimizer step through the C ABI (csrc/optim.hip) on the U-Net's own parameter list (shapes of
    seg.unet(3, 3); no model run): segk_optim_adamw alone, + segk_optim_grad_norm, + the EMA, against the stock compositions
    on the same tensors in this process -- torch.optim.AdamW(fused=True) alone, + clip_grad_norm_, + _foreach_lerp_.
    Alternating order, seven rounds of 20 steps each: median and min..max of the time per step.  Written to
    profiles/optim_kbench.txt (or the file given with --out)."""
    import image_segmentation_amd as seg
    from image_segmentation_amd import optim as O
    shapes = [tuple(p.shape) for p in seg.unet(3, 3).parameters()]
    g = torch.Generator(device="cuda").manual_seed(0)
    ps = [torch.randn(s, device="cuda", generator=g) * 0.05 for s in shapes]
    gs = [torch.randn(s, device="cuda", generator=g) * 1e-3 for s in shapes]
    ms, vs, ss = ([torch.zeros_like(p) for p in ps] for _ in range(3))
    numel = sum(p.numel() for p in ps)
    st = ops._stream()
    group = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01}
    groups = torch.frombuffer(bytearray(O.group_scalars(group, 0.999)), dtype=torch.uint8).cuda()
    state = torch.frombuffer(bytearray(O.state_bytes(0, [(1.0, 1.0)])), dtype=torch.uint8).cuda()

    def table(ema):
        tab, blocks = O.build_table([(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), s.data_ptr() if ema else 0,
                                      p.numel(), 0) for p, gr, m, v, s in zip(ps, gs, ms, vs, ss)])
        return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda(), blocks
    (t0, blocks), (t1, _) = table(False), table(True)
    part = torch.empty(blocks, dtype=torch.float64, device="cuda")
    parity = [0]

    def mine(tab, clip):
        def f():
            if clip:
                _lib.call("segk_optim_grad_norm", tab.data_ptr(), len(ps), blocks, groups.data_ptr(), 1, state.data_ptr(),
                          part.data_ptr(), 1.0, _lib.OPTIM_CLIP, parity[0], st)
            _lib.call("segk_optim_adamw", tab.data_ptr(), len(ps), blocks, groups.data_ptr(), 1, state.data_ptr(),
                      _lib.OPTIM_NORMED if clip else 0, parity[0], st)
            parity[0] ^= 1
        return f
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    for p, gr in zip(params, gs):
        p.grad = gr.clone()
    stock_opt = torch.optim.AdamW(params, weight_decay=0.01, fused=True)
    shadows = [p.detach().clone() for p in params]

    def stock(clip, ema):
        def f():
            if clip:
                torch.nn.utils.clip_grad_norm_(params, 1.0)
            stock_opt.step()
            if ema:
                torch._foreach_lerp_(shadows, [p.detach() for p in params], 1e-3)
        return f
    fns = {"segk_optim_adamw": mine(t0, False), "torch AdamW(fused)": stock(False, False),
           "segk grad_norm + adamw": mine(t0, True), "torch clip_grad_norm_ + AdamW(fused)": stock(True, False),
           "segk grad_norm + adamw + EMA": mine(t1, True), "torch clip + AdamW(fused) + _foreach_lerp_": stock(True, True)}
    ts = {k: [] for k in fns}
    for _ in range(7):
        for k, fn in fns.items():
            ts[k].append(timeit(fn, 20))
    lines = [f"optim: {len(ps)} tensors, {numel} parameters ({numel * 4 / 1e6:.1f} MB each of p, g, m, v, shadow), {blocks} blocks of "
             f"{O.CHUNK} elements; us per step, median [min..max] of 7 rounds x 20 steps, alternating"]
    moved = {"segk_optim_adamw": 7, "torch AdamW(fused)": 7, "segk grad_norm + adamw": 8, "torch clip_grad_norm_ + AdamW(fused)": 10,
             "segk grad_norm + adamw + EMA": 10, "torch clip + AdamW(fused) + _foreach_lerp_": 13}
    for k, t in ts.items():
        med = sorted(t)[3]
        lines.append(f"  {k:44s} {med:9.1f} us [{min(t):.1f}..{max(t):.1f}]  {moved[k]:2d} x {numel * 4 / 1e6:.0f} MB -> "
                     f"{moved[k] * numel * 4 / med / 1e6:.2f} TB/s")
    clk = ops.clock_probe()
    lines.append(f"  clock probe: median {clk['median_ghz']} GHz; build {_lib.build_id()}")
    print("\n".join(lines))
    path = os.path.join(ROOT, "profiles", "optim_kbench.txt")
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "optim":
        optim()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "calib":
        calib()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "tiles":
        tiles()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "tta":
        tta()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "components":
        components()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "vectors":
        vectors()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "raster":
        raster()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "pq":
        pq()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "morph":
        morph()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "boundary":
        boundary()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "slic":
        slic()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "mix":
        mix()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "perturb":
        perturb()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "augment":
        augment()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "prompt":
        prompt()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "predict":
        predict()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "pack":
        pack()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "ends":
        ends()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "stem":
        stem()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "vit":
        vit()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "head":
        head()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "recon":
        recon()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "lovasz":
        lovasz()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "hardloss":
        hardloss()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "distill":
        distill()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "loss":
        loss()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "bn":
        bn()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "convt":
        convt()
        sys.exit(0)
    main()
