#!/usr/bin/env python3
"""Headline benchmark: images/sec of the U-Net 3-class training step (forward + CrossEntropy + backward +
RCCL gradient all-reduce + AdamW) on synthetic 3x256x256 batches, B=32 per GPU (BASELINE.json config 2 at
N=1, config 3 at N=8; weak scaling), on the hand-written HIP kernels in bf16 (fp32 accumulation / statistics /
master parameters).

    python bench.py --gpus N --steps K --warmup W          # N > 1 without a launcher: starts its own N ranks
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --full                                 # + the evidence blocks below (about a minute more)
    python bench.py --dump-outputs DIR                     # + what the last timed step computed, as DIR/<name>.npy

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints the headline fields (metric,
value, unit, ms_per_step, dtype, ...); the blocks below stay null.  With --full the line also carries
  roofline     : the dominant kernel family of the step, timed live with HIP events on the launch stream in
                 a separate instrumented pass (the timed region itself carries no instrumentation);
  cpu_baseline : the CPU oracle (oracle/, stock PyTorch fp32 ops = the reference algorithm) timed on the host
                 cores on a bounded sample of the same workload (rank 0, N=1 only); its `parity` entry is the
                 metric's "IoU parity vs CPU ref": fp32-mode logits / argmax masks / mIoU of the HIP path against
                 that same oracle on the same sample;
  kernels      : per-kernel-family ms/step and achieved TFLOP/s / GB/s (algorithmic counts);
and levels, launch_census, other_configs, clock, allreduce_overlap (profiles/README.md).

--dump-outputs DIR writes, on rank 0, what the caller of the timed step holds after the last timed step (before anything
else runs): loss.npy (float64 scalar), logits.npy (the step's forward output, float32), params.npy / grads.npy (the
trainable parameters after the optimizer step and their gradients, float32, flattened in named_parameters() order) and
buffers.npy (the floating-point buffers, e.g. BatchNorm running statistics).  An array larger than its share of the 64 MB
budget is replaced by a fixed seeded sample of its flattened elements (same indices for params and grads).  Inputs and
initial weights are seeded, so two builds run with the same arguments can be compared array by array.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s, MI355X spec (MI355X_MICROARCH.md); 6.29e12 measured copy ceiling
HBM_COPY = 6.29e12
MFMA_PEAK = {"bf16": 2.5e15, "f32": 157.3e12}
# algorithmic DoubleConv bytes per image (fwd+bwd, phase model), 2 B/elem at 256x256
DC_BYTES_PER_IMAGE_BF16_256 = 593.7e6


def _u01(n, seed):
    """Portable deterministic uniform [0,1) stream of SURVEY.md 8c (splitmix64 finaliser, top 24 bits): the synthetic
    inputs of the benchmark.  Restated here so that only the cpu_baseline leg touches oracle/."""
    import numpy as np
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def fill(shape, seed, lo, hi):
    import numpy as np
    import torch
    n = int(np.prod(shape))
    return torch.from_numpy((lo + (hi - lo) * _u01(n, seed)).astype(np.float32).reshape(shape))


def labels(shape, seed, num_classes):
    import numpy as np
    import torch
    n = int(np.prod(shape))
    lab = np.clip(np.floor(num_classes * _u01(n, seed)), 0, num_classes - 1).astype(np.int64)
    return torch.from_numpy(lab.reshape(shape))


def _sample_index(n, cap, seed):
    """None when n <= cap (keep every element), else a fixed seeded sample of at most `cap` indices, ascending."""
    import numpy as np
    if n <= cap:
        return None
    return np.unique(np.random.default_rng(seed).integers(0, n, size=cap))


def _flat(t, idx):
    import torch
    t = t.detach().reshape(-1)
    if idx is not None:
        t = t[torch.from_numpy(idx).to(t.device)]
    return t.float().cpu().numpy()


def dump_outputs(out_dir, loss, logits, model):
    """--dump-outputs: the arrays the caller of the timed step holds after the last timed step (module docstring), as
    float32 / float64 .npy files under out_dir; logits at most 8 Mi elements, the others 2 Mi each (<= 56 MiB in all)."""
    import numpy as np
    import torch
    cap = 1 << 23
    os.makedirs(out_dir, exist_ok=True)
    params = [p for p in model.parameters() if p.requires_grad]
    flat_p = torch.cat([p.detach().reshape(-1).float() for p in params])
    flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).float()
                        for p in params])
    pidx = _sample_index(flat_p.numel(), cap // 4, seed=2)
    bufs = [b.detach().reshape(-1).float() for b in model.buffers() if b.is_floating_point()]
    flat_b = torch.cat(bufs) if bufs else torch.zeros(0, device=flat_p.device)
    lg = logits.detach()
    lidx = _sample_index(lg.numel(), cap, seed=1)
    arrays = {
        "loss": np.asarray(loss.item(), dtype=np.float64),
        "logits": lg.float().cpu().numpy() if lidx is None else _flat(lg, lidx),
        "params": _flat(flat_p, pidx),
        "grads": _flat(flat_g, pidx),
        "buffers": _flat(flat_b, _sample_index(flat_b.numel(), cap // 4, seed=3)),
    }
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def run_workload(args, world, rank, dev, want_levels=False, dump_dir=None):
    """Build the model of `args` (model / batch / size / dtype / loss), run args.warmup untimed and args.steps timed
    training steps bracketed by barrier + synchronize, write the last timed step's outputs to dump_dir (rank 0, if given),
    then args.profile_steps instrumented steps (HIP events on the launch stream around every kernel family; every rank runs
    them -- they contain the gradient all-reduce -- rank 0 records).
    Returns the max-over-ranks time of the timed region and the per-family (and, for the U-Net, per-level) event sums."""
    import torch
    import torch.distributed as dist
    import image_segmentation_amd as seg
    from image_segmentation_amd import ops
    from image_segmentation_amd.parallel import GradSync

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    prev_dtype = seg.get_compute_dtype()
    seg.set_compute_dtype(dtype)
    B, S = args.batch, args.size
    torch.manual_seed(1234)                       # identical random-init weights on every rank
    ncls = 3
    if args.model == "clipunet":
        ncls = 4
        model = seg.ClipUNet(num_classes=4, encoder=seg.ClipViTEncoder.from_config()).to(dev).train()
    else:
        model = seg.unet(3, 3).to(dev).train()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], weight_decay=0.01, fused=True)
    if args.loss == "ce":
        loss_fn = seg.CrossEntropyLoss()
    else:
        cw = torch.tensor([0.2046795970925636, 1.0271954434416883, 1.2293222812780409])
        loss_fn = seg.WeightedDiceCELoss(smooth_dice=1.0, class_weights=cw)
    X = fill((B, 3, S, S), 1 + 2 * rank, 0, 1).to(dev)           # images resident in HBM before timing
    Y = labels((B, S, S), 2 + 2 * rank, ncls).to(dev)
    gs = GradSync(model) if world > 1 else None

    def step():
        opt.zero_grad(set_to_none=True)
        if gs is not None:
            gs.arm()
        logits = model(X)
        loss = loss_fn(logits, Y)
        if gs is not None:
            gs.backward_begin()
        loss.backward()
        if gs is not None:
            gs.backward_end()
            gs.sync()
        opt.step()
        return loss, logits

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, logits = step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    final_loss = loss.item()
    if dump_dir is not None and rank == 0:
        dump_outputs(dump_dir, loss, logits, model)

    prof, level_prof, overlap = {}, {}, None
    if args.profile_steps > 0:
        if rank == 0:
            ops.TIMER = ops.KernelTimer()
            if want_levels:
                ops.name_levels(model)
            if gs is not None:
                gs.timing = True             # per-bucket launch / completion events of the last instrumented step
        for _ in range(args.profile_steps):
            step()
        if rank == 0:
            prof = ops.TIMER.summary()
            level_prof = ops.TIMER.level_summary() if want_levels else {}
            ops.TIMER = None
            if gs is not None:
                overlap = gs.overlap_trace()
                gs.timing = False
    census = None
    if want_levels and rank == 0 and world == 1:
        # device-side launch census of the step (torch.profiler, 2 steps): every kernel the step puts on the GPU, the
        # optimizer's and torch's fills / copies included -- the span count of `kernels` sees only this package's launches
        from torch.profiler import profile, ProfilerActivity
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with profile(activities=[ProfilerActivity.CUDA]) as tp:
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
        names = {}
        for e in tp.events():
            if e.device_type is not None and str(e.device_type).endswith("CUDA"):
                names[e.name] = names.get(e.name, 0) + 1
        stock = sum(c for k, c in names.items() if "at::native" in k or k.startswith("Mem") or "rocclr" in k)
        census = {"device_launches_per_step": sum(names.values()) / 2.0, "stock_torch_launches_per_step": stock / 2.0,
                  "distinct_kernels": len(names), "method": "torch.profiler CUDA activity over 2 steps after the timed region"}
    if world > 1:
        dist.barrier()
    if gs is not None:
        gs.remove()
    del model, opt, X, Y
    torch.cuda.empty_cache()
    seg.set_compute_dtype(prev_dtype)
    return {"dt": dt, "final_loss": final_loss, "prof": prof, "levels": level_prof, "overlap": overlap, "census": census}


def family_table(prof, n, peak):
    """per-kernel-family ms per step, achieved TFLOP/s and algorithmic GB/s from the instrumented steps"""
    kernels = {}
    for tag, r in prof.items():
        ms = r["ms"] / n
        kernels[tag] = {
            "launches_per_step": r["launches"] // n, "ms_per_step": round(ms, 4),
            "tflops": round(r["flops"] / n / (ms * 1e-3) / 1e12, 2) if ms > 0 else None,
            "alg_GBps": round(r["bytes"] / n / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
        }
    return kernels


def two_roofs(flops, nbytes, seconds, peak):
    """Which roof binds a kernel (or a group of kernels) with these algorithmic counts, and the fraction of it reached:
    bound time = max(flops / MFMA peak, bytes / 8 TB/s); frac = bound time / measured time."""
    t_m, t_h = flops / peak, nbytes / HBM_PEAK
    bound = "mfma" if t_m >= t_h else "hbm"
    return {"bound": bound, "frac": round(max(t_m, t_h) / seconds, 4) if seconds > 0 else None,
            "mfma_frac": round(t_m / seconds, 4) if seconds > 0 else None,
            "hbm_frac": round(t_h / seconds, 4) if seconds > 0 else None}


def level_table(level_prof, n, peak):
    """SURVEY 7 hard part 1 / 8(d): per DoubleConv level x {fwd, dgrad, wgrad} (the 3x3 conv kernels of the block, both convs
    together) the time per step, TFLOP/s, algorithmic GB/s, which roof binds and the fraction of THAT roof; `other` = every
    other launch of the block's autograd node (BatchNorm passes, pooling / head / ConvTranspose kernels, slab reductions)."""
    out = {}
    for (level, phase), r in sorted(level_prof.items()):
        sec = r["ms"] * 1e-3 / n
        row = {"launches": r["launches"] // n, "us": round(sec * 1e6, 1)}
        if phase != "other" and sec > 0:
            fl, by = r["flops"] / n, r["bytes"] / n
            row.update({"tflops": round(fl / sec / 1e12, 1), "alg_GBps": round(by / sec / 1e9, 1)})
            row.update(two_roofs(fl, by, sec, peak))
        out.setdefault(level, {})[phase] = row
    return out


def other_configs(args, world, rank, dev):
    """After the headline timed region: 10 timed steps each of BASELINE config 4 (CLIP-UNet, B=16, 224x224), config 5
    (B=8, 512x512, Dice+CE) and the fp32 parity mode at config 2 -- the mode that meets the north-star parity gate --, each with
    its dominant kernel family and that family's fraction of the roof that binds it."""
    import copy
    out = {}
    for name, over in (("config4_clipunet_B16_224", {"model": "clipunet", "batch": 16, "size": 224, "loss": "ce", "dtype": "bf16"}),
                       ("config5_unet_B8_512_dicece", {"model": "unet", "batch": 8, "size": 512, "loss": "dicece", "dtype": "bf16"}),
                       ("config2_fp32_parity_mode", {"model": "unet", "batch": 32, "size": 256, "loss": "ce", "dtype": "f32"})):
        a = copy.copy(args)
        for k, v in over.items():
            setattr(a, k, v)
        a.steps, a.warmup, a.profile_steps = 10, 3, 2
        try:
            w = run_workload(a, world, rank, dev)
            peak = MFMA_PEAK[a.dtype]
            row = {"ms_per_step": round(w["dt"] / a.steps * 1e3, 3), "value": round(a.batch * a.steps / w["dt"], 2),
                   "unit": "images/sec", "steps": a.steps, "warmup": a.warmup, "dtype": a.dtype,
                   "final_loss": round(w["final_loss"], 5)}
            if w["prof"]:
                dom = max(w["prof"], key=lambda k: w["prof"][k]["ms"])
                r = w["prof"][dom]
                sec = r["ms"] * 1e-3
                row["dominant"] = {"kernel": dom, "launches_per_step": r["launches"] // a.profile_steps,
                                   "ms_per_step": round(r["ms"] / a.profile_steps, 4),
                                   "tflops": round(r["flops"] / sec / 1e12, 1) if sec > 0 else None,
                                   **two_roofs(r["flops"], r["bytes"], sec, peak)}
                vg = w["prof"].get("vit_gemm")
                if vg and vg["ms"] > 0:
                    row["vit_gemm"] = {"launches_per_step": vg["launches"] // a.profile_steps,
                                       "ms_per_step": round(vg["ms"] / a.profile_steps, 4),
                                       "tflops": round(vg["flops"] / (vg["ms"] * 1e-3) / 1e12, 1)}
            out[name] = row
        except Exception as e:              # an extra must never take the headline line down
            out[name] = {"error": f"{type(e).__name__}: {e}"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--loss", choices=["ce", "dicece"], default="ce")
    ap.add_argument("--model", choices=["unet", "clipunet"], default="unet",
                    help="clipunet = BASELINE config 4 (use --batch 16 --size 224): frozen ViT-B/16 (local random-weight "
                         "config) + HIP decoder, 4 classes; not the headline metric")
    ap.add_argument("--full", action="store_true", help="after the headline timed region, also measure the evidence blocks: "
                    "instrumented steps (roofline, kernels), CPU baseline + parity, per-level table, launch census, "
                    "other BASELINE configurations, clock probe")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs to DIR/<name>.npy")
    ap.add_argument("--profile-steps", type=int, default=None, help="instrumented steps for the roofline block "
                    "(default 3 with --full, else 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL); 'gloo' only to rehearse "
                    "the multi-rank code path on a box with fewer GPUs than ranks")
    ap.add_argument("--share-device", action="store_true", help="rehearsal only: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the blocks appended after the headline timed "
                    "region (per-level roofline table, launch census, other BASELINE configurations, clock probe)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.profile_steps is None:
        args.profile_steps = 3 if args.full else 0

    # dmabuf IPC: RCCL needs it on this driver.  Set before torch is imported, for every way a rank can be started -- by
    # the self-launch below (inherited) and by the driver's own `python -m torch.distributed.run ... bench.py` alike.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # Started without a launcher: this process becomes the launcher.  It has not touched the GPU (torch is not even
        # imported yet) and it never exec()s: the N ranks are CHILD processes (one per GPU, RCCL between them); rank 0's
        # JSON line reaches stdout through the inherited descriptor and the child's exit code becomes ours.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ)                                  # carries HSA_ENABLE_IPC_MODE_LEGACY=0 (set above)
        env.setdefault("OMP_NUM_THREADS", "8")
        # rank 0's JSON line is relayed to stdout; anything else a rank writes there (the gloo transport of the rehearsal
        # mode prints connection notes to stdout from C++) goes to stderr, so stdout carries exactly ONE line
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        for line in r.stdout.splitlines():
            print(line, file=sys.stdout if line.startswith("{") else sys.stderr)
        sys.exit(r.returncode)

    import torch
    import torch.distributed as dist
    import image_segmentation_amd as seg
    from image_segmentation_amd import ops
    from image_segmentation_amd.parallel import GradSync

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"error: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks", file=sys.stderr)
        sys.exit(2)
    if args.share_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    B, S = args.batch, args.size
    w = run_workload(args, world, rank, dev, want_levels=(args.full and args.model == "unet" and not args.no_extras),
                     dump_dir=args.dump_outputs)
    dt, final_loss, prof, level_prof, overlap = w["dt"], w["final_loss"], w["prof"], w["levels"], w["overlap"]
    me = {"rank": rank, "device": local, "name": torch.cuda.get_device_name(local)}
    ranks_info = [me]
    if world > 1:
        ranks_info = [None] * world
        dist.all_gather_object(ranks_info, me)
        dist.barrier()
    rehearsal = world > 1 and (args.backend != "nccl" or args.share_device)

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    n = max(1, args.profile_steps)
    peak = MFMA_PEAK[args.dtype]
    kernels = family_table(prof, n, peak)
    roofline = None
    if prof:
        dom = max(prof, key=lambda k: prof[k]["ms"])
        r = prof[dom]
        launches = max(1, r["launches"])
        avg_s = r["ms"] * 1e-3 / launches
        fl, by = r["flops"] / launches, r["bytes"] / launches
        mfma_bound = (fl / peak) >= (by / HBM_PEAK)
        if mfma_bound:
            ach = fl / avg_s / 1e12
            roofline = {"bound": "mfma", "achieved": round(ach, 2), "peak": peak / 1e12, "unit": "TFLOP/s",
                        "frac": round(ach / (peak / 1e12), 4)}
        else:
            ach = by / avg_s / 1e9
            roofline = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                        "frac": round(ach / (HBM_PEAK / 1e9), 4)}
        roofline.update({"kernel": dom, "launches_per_step": r["launches"] // n,
                         "avg_launch_us": round(avg_s * 1e6, 2),
                         "alg_flops_per_launch": fl, "alg_bytes_per_launch": by,
                         "hbm_frac_same_kernel": round(by / avg_s / HBM_PEAK, 4), "traffic": None})
        # HBM bytes per launch from the rocprofv3 PMC passes of this same command (FETCH_SIZE x2 + WRITE_SIZE,
        # gfx950 correction), recorded under profiles/ -- counters cannot be sampled from inside this process
        # The record names the library build (segk_build_id = hash of the kernel sources) it was collected on: it is
        # attached only to a line produced by that same build, otherwise `traffic` stays null with the reason.
        try:
            from image_segmentation_amd import _lib
            import glob
            cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True)   # newest round first
            src, pmc = "profiles/(no r*_pmc_traffic.json)", {}
            for c in cands:
                rec = json.load(open(c))
                if not pmc or rec.get("build_id") == _lib.build_id():
                    src, pmc = os.path.relpath(c, ROOT), rec
                if rec.get("build_id") == _lib.build_id():
                    break
            fam = {"conv3x3_igemm": "conv3x3", "wgrad3x3": "wgrad3x3"}.get(dom)
            if pmc.get("build_id") != _lib.build_id():
                roofline["traffic_note"] = (f"{src} was recorded on library build {pmc.get('build_id')}, this run is "
                                            f"{_lib.build_id()}: not attached")
            elif fam and args.dtype == "bf16" and B == 32 and S == 256 and args.model == "unet":
                roofline["traffic"] = pmc["families"][fam]["hbm_bytes_per_launch"]
                roofline["traffic_source"] = f"{src} (recorded by rocprofv3 --pmc passes of this command on the same build)"
            else:
                roofline["traffic_note"] = "no PMC record for this configuration"
        except Exception as e:
            roofline["traffic_note"] = f"no PMC record: {type(e).__name__}"

    if args.model == "clipunet":
        cfg_name = "BASELINE config 4" if (B == 16 and S == 224 and world == 1) else "custom configuration"
    elif B == 32 and S == 256 and args.loss == "ce" and world == 1:
        cfg_name = "BASELINE config 2"
    elif B == 32 and S == 256 and args.loss == "ce" and world == 8 and not rehearsal:
        cfg_name = "BASELINE config 3"
    elif B == 32 and S == 256 and args.loss == "ce" and not rehearsal:
        cfg_name = f"BASELINE config 3 shape at {world} of its 8 GPUs"
    elif B == 8 and S == 512 and args.loss == "dicece" and world == 1:
        cfg_name = "BASELINE config 5"
    else:
        cfg_name = "custom configuration"
    img_s = world * B * args.steps / dt
    # DoubleConv-scope HBM roofline of SURVEY 8(d): kernels of the 9 DoubleConv blocks only
    dc_tags = ("conv3x3_igemm", "wgrad3x3", "wgrad_reduce", "bn_relu_bwd", "bn_relu_apply")
    dc_ms = sum(kernels[t]["ms_per_step"] for t in dc_tags if t in kernels)
    scope = None
    if dc_ms > 0 and args.dtype == "bf16":
        per_img = DC_BYTES_PER_IMAGE_BF16_256 * (S * S) / (256 * 256)
        gbps = per_img * B / (dc_ms * 1e-3) / 1e9
        scope = {"doubleconv_ms_per_step": round(dc_ms, 3), "alg_bytes_per_image": per_img,
                 "alg_GBps": round(gbps, 1), "frac_of_8TBps": round(gbps * 1e9 / HBM_PEAK, 4),
                 "frac_of_6.29TBps_copy": round(gbps * 1e9 / HBM_COPY, 4)}

    cpu = None
    if args.full and world == 1 and not args.no_cpu_baseline and args.model == "unet":
        cpu = cpu_baseline(S)

    # ---- appended evidence (after the headline timed region, which stays un-instrumented): per-level two-roof table, the
    # other BASELINE configurations and the parity mode through the same code path, and a clock estimate for this box
    levels = level_table(level_prof, n, peak) if level_prof else None
    extras, clock = None, None
    headline = (args.model == "unet" and B == 32 and S == 256 and args.loss == "ce" and args.dtype == "bf16")
    if args.full and not args.no_extras:
        try:
            clock = ops.clock_probe()
        except Exception as e:
            clock = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and headline:
            extras = other_configs(args, world, rank, dev)

    out = {
        "metric": "images/sec (fwd+bwd) U-Net 3-class 256x256; IoU parity vs CPU ref" if args.model == "unet" else
                  "images/sec (frozen ViT-B/16 fwd + decoder fwd+bwd) CLIP-UNet 4-class 224x224 (BASELINE config 4, not the headline metric)",
        "value": round(img_s, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": (f"unet(3,3) train step (fwd + {args.loss} + bwd + grad all-reduce + AdamW), "
                                f"B={B}/GPU 3x{S}x{S}, {cfg_name}") if args.model == "unet" else
                               (f"ClipUNet(4 classes) train step: frozen ViT-B/16 forward (random-init local config) + decoder "
                                f"fwd + {args.loss} + bwd + AdamW, B={B}/GPU 3x{S}x{S}, {cfg_name}"),
                   "global_batch": B * world, "image": [3, S, S], "parallelism": f"dp{world}",
                   "final_loss": round(final_loss, 5),
                   "backend": (args.backend if world > 1 else None),
                   "rccl_ranks": (world if (world > 1 and args.backend == "nccl") else 0),
                   "ranks": ranks_info, "rehearsal": rehearsal},
        "roofline": roofline, "cpu_baseline": cpu, "doubleconv_scope": scope, "kernels": kernels,
        "launches_per_step": sum(k["launches_per_step"] for k in kernels.values()) if kernels else None,
        "launch_census": w.get("census"),
        "levels": levels, "other_configs": extras, "clock": clock, "allreduce_overlap": overlap,
    }
    print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def _host_cpu():
    """(model name, physical cores, logical cpus) of the host, from /proc/cpuinfo."""
    model, phys, logical = "unknown", set(), 0
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "processor":
                logical += 1
            elif k == "model name":
                model = v
            elif k == "physical id":
                pid = v
            elif k == "core id":
                cid = v
                phys.add((pid, cid))
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))       # the cores this process may actually run on (container share)
    except AttributeError:
        usable = logical or 1
    ncores = len(phys) or logical or 1
    return model, min(ncores, usable), usable


def cpu_baseline(S):
    """The CPU oracle (= the reference algorithm in stock PyTorch fp32 ops) on a bounded sample of the same
    workload: 4 of the 32 images per step.  Thread count: a short sweep (one warm-up + one timed step each at the
    usable physical core count, half of it, 32 and 16), then 3 more timed steps at the fastest setting; the reported rate
    is the mean of that setting's timed steps."""
    import torch
    from oracle import unet_ref, losses_ref
    from oracle.fill import fill, labels, fill_module
    cpu_model, phys, usable = _host_cpu()
    Bc = 4
    m = unet_ref.unet(3, 3); fill_module(m, 1000); m.train()
    opt = torch.optim.AdamW(m.parameters(), weight_decay=0.01)
    X = fill((Bc, 3, S, S), 1, 0, 1); Y = labels((Bc, S, S), 2, 3)

    def step():
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = losses_ref.cross_entropy(m(X), Y)
        loss.backward()
        opt.step()
        return time.perf_counter() - t0
    prev_threads = torch.get_num_threads()
    cands = sorted({max(1, phys), max(1, phys // 2), min(32, max(1, phys)), min(16, max(1, phys))}, reverse=True)
    sweep, t_budget = {}, time.perf_counter()
    for n in cands:
        torch.set_num_threads(n)
        step()                                           # warm-up at this setting
        sweep[n] = [step()]
        if time.perf_counter() - t_budget > 60.0:        # bounded: a slow host stops sweeping
            break
    best = min(sweep, key=lambda n: sweep[n][0])
    torch.set_num_threads(best)
    sweep[best] += [step() for _ in range(3)]
    dt = sum(sweep[best]) / len(sweep[best])
    # the FULL bench batch as well (SURVEY 8d asks for B = 32 beside the sub-sample): one warm-up + one timed step of the same
    # oracle at B = 32 at the sub-sample's fastest thread count (~25 s on an EPYC 9575F; all 128 cores were measured 2 x slower:
    # 26.2 vs 12.8 s per step)
    full = {}
    try:
        Xf = fill((32, 3, S, S), 1, 0, 1); Yf = labels((32, S, S), 2, 3)
        mf = unet_ref.unet(3, 3); fill_module(mf, 1000); mf.train()
        optf = torch.optim.AdamW(mf.parameters(), weight_decay=0.01)

        def step_full():
            t0 = time.perf_counter()
            optf.zero_grad()
            losses_ref.cross_entropy(mf(Xf), Yf).backward()
            optf.step()
            return time.perf_counter() - t0
        t_full = time.perf_counter()
        for n in (best,):
            torch.set_num_threads(n)
            step_full()
            full[str(n)] = round(step_full(), 3)
            if time.perf_counter() - t_full > 45.0:      # bounded
                break
        del mf, optf, Xf, Yf
    except Exception as e:                               # the baseline must never take the bench line down
        full = {"error": repr(e)[:200]}
    torch.set_num_threads(prev_threads)
    out = {"value": round(Bc / dt, 3), "unit": "images/sec", "cores": best, "kind": "port",
           "cpu_model": cpu_model, "physical_cores_usable": phys, "logical_cpus_usable": usable,
           "thread_sweep_s_per_step": {str(n): round(v[0], 3) for n, v in sweep.items()},
           "full_batch_B32_s_per_step": full,
           "full_batch_B32_images_per_sec": (round(32.0 / min(v for v in full.values()), 3)
                                             if full and all(isinstance(v, float) for v in full.values()) else None),
           "sample": f"oracle unet(3,3) fp32 train step (fwd+CE+bwd+AdamW), B={Bc} of 32 images 3x{S}x{S}; per thread "
                     f"setting 1 warm-up + 1 timed step, then {len(sweep[best])} timed steps in all at the fastest "
                     f"({best} threads on {cpu_model}, {phys} usable physical cores)"}
    # The metric's second half ("IoU parity vs CPU ref"): the same oracle, here as the CHECKER of the product path on
    # the same sample and the trained oracle weights -- once in fp32 parity mode (the 1e-3 / bit-exact-argmax gate) and
    # once in bf16, the mode the headline number is measured in.
    try:
        import image_segmentation_amd as seg
        from image_segmentation_amd.metrics import MetricsHistory
        prev = seg.get_compute_dtype()
        m.train()
        with torch.no_grad():
            state = {k: v.clone() for k, v in m.state_dict().items()}
            lr = m(X)                                     # training-mode forward (batch statistics), like the bench step
        ce_ref = float(losses_ref.cross_entropy(lr, Y))
        a_cpu = MetricsHistory(3)
        for i in range(Bc):
            a_cpu.accumulate(lr[i].cuda(), Y[i].cuda())
        _, iou_cpu, _ = a_cpu.compute_epoch_metrics()
        out["parity"] = {}
        for name, dt_ in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            seg.set_compute_dtype(dt_)
            hip = seg.unet(3, 3)
            hip.load_state_dict(state)
            hip.cuda().train()
            with torch.no_grad():
                lh = hip(X.cuda())
            ce_hip = float(seg.CrossEntropyLoss()(lh, Y.cuda()))
            a_hip = MetricsHistory(3)
            for i in range(Bc):
                a_hip.accumulate(lh[i], Y[i].cuda())
            _, iou_hip, _ = a_hip.compute_epoch_metrics()
            d = (lh.cpu() - lr).abs()
            same = lh.argmax(1).cpu() == lr.argmax(1)
            agree = float(same.double().mean())
            # a pixel whose two best reference logits are closer than 1e-4 can flip under ANY reordering of fp32 sums (the
            # oracle itself moves by that much between thread counts): disagreements are reported inside / outside such ties
            top2 = lr.topk(2, dim=1).values
            tie = (top2[:, 0] - top2[:, 1]) < 1e-4
            out["parity"][name] = {
                "mode": "exact-fp32 MFMA kernels" if name == "fp32" else "bf16 storage / bf16 MFMA, fp32 accumulation and statistics",
                "max_abs_logit_diff": float(d.max()), "mean_abs_logit_diff": float(d.mean()),
                "argmax_agreement": agree, "argmax_masks_equal": bool(agree == 1.0),
                "pixels": int(same.numel()), "disagreeing_pixels": int((~same).sum()),
                "reference_near_tie_pixels": int(tie.sum()), "disagreeing_outside_near_ties": int((~same & ~tie).sum()),
                "miou_hip": iou_hip, "miou_cpu_ref": iou_cpu, "ce_hip": ce_hip, "ce_cpu_ref": ce_ref}
        seg.set_compute_dtype(prev)
    except Exception as e:          # the baseline number stands on its own; report why the check did not run
        out["parity"] = {"error": f"{type(e).__name__}: {e}"}
    return out


if __name__ == "__main__":
    main()
