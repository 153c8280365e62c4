"""seg.AdamW: the optimizer step of the train loop as HIP kernels -- global-norm gradient clipping, AdamW and a weight EMA in
one streaming pass over every parameter (segk_optim_adamw), behind one deterministic float64 norm pass
(segk_optim_grad_norm) when clipping or the non-finite skip is on.  Replaces the notebooks' `AdamW(weight_decay=0.01)` cell
and what trainers compose around it (clip_grad_norm_, a _foreach_lerp_ EMA).  The arithmetic is defined in DESIGN.md section
3.13; tests/optim_reference.py restates it and the device is held to it bit for bit.

A torch.optim.Optimizer subclass: param groups, LR schedulers, hooks (the packed-weight cache of ops.py hears about every
step through the global post-step hook) and torch.optim.AdamW's state_dict layout.  There is no CPU path: constructing,
state_dict() and argument checking work on the host, step() needs HIP tensors.  step() never synchronises with the host:
the step count, the running bias-correction products, the norm, the clip coefficient and the skip counter live on the device
(`last` holds views of them)."""
import contextlib
import struct

import numpy as np
import torch

from . import _lib, ops

CHUNK = _lib.OPTIM_CHUNK
_HEAD = struct.Struct("<dfii12x")              # norm, clip, finite, skipped (include/segk.h: the optimizer state)
_GROUP = struct.Struct("<8f2d16x")             # segk_optim_group
_STOCK_DEFAULTS = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)     # the param_groups keys of this torch's AdamW


def table_blocks(numels):
    """(block0 of every tensor, total blocks): a tensor owns ceil(numel / CHUNK) consecutive blocks of the launch."""
    block0, blk = [], 0
    for n in numels:
        if n <= 0:
            raise ValueError("optimizer table: tensors of 0 elements are left out by the caller")
        block0.append(blk)
        blk += (n + CHUNK - 1) // CHUNK
    if blk >= 1 << 31:
        raise ValueError("optimizer table: more than 2^31 blocks")
    return block0, blk


def build_table(rows):
    """Host image of the device table: one _lib.OptimRec for each row (p, g, m, v, shadow or 0 -- addresses -- numel, group)
    in launch order -> (the array, total blocks)."""
    block0, total = table_blocks([r[5] for r in rows])
    tab = (_lib.OptimRec * len(rows))()
    for e, (p, g, m, v, s, numel, group), b0 in zip(tab, rows, block0):
        e.p, e.g, e.m, e.v, e.shadow, e.numel, e.block0, e.group = p, g, m, v, s or None, numel, b0, group
    return tab, total


def group_scalars(group, ema_decay):
    """The bytes of one segk_optim_group: every scalar formed in float64 and rounded to float32 once (struct does that)."""
    lr, (b1, b2) = float(group["lr"]), group["betas"]
    d = 0.0 if ema_decay is None else float(ema_decay)
    return _GROUP.pack(lr, 1.0 - lr * float(group["weight_decay"]), 1.0 - b1, b2, 1.0 - b2, float(group["eps"]), 1.0 - d, d,
                       float(b1), float(b2))


def state_bytes(t, pows):
    """Host image of the device step state with slot 0 current: t applied steps, pows = [(beta1^t, beta2^t) per group]."""
    slot = struct.pack("<i4x", t) + b"".join(struct.pack("<2d", *p) for p in pows)
    return _HEAD.pack(0.0, 1.0, 1, 0) + slot + slot


def _running_product(beta, t):
    p = 1.0
    for _ in range(t):           # the device multiplies once per step: the same float64 roundings
        p *= beta
    return p


class AdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay, torch.optim.AdamW's order of operations) with optional global-norm clipping
    (max_grad_norm), a device-side skip of steps whose gradients hold an inf or NaN (skip_nonfinite) and an EMA of the
    weights (ema_decay; ema_warmup: d = min(ema_decay, (1 + t) / (10 + t))).  One step count is kept for all parameters."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=False, *, maximize=False,
                 capturable=False, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        for name, val in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable)):
            if val:
                raise ValueError(f"seg.AdamW: {name}=True is not supported")
        if isinstance(lr, torch.Tensor):
            raise ValueError("seg.AdamW: lr must be a number (a tensor lr belongs to capturable optimizers)")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"seg.AdamW: max_grad_norm must be positive, got {max_grad_norm}")
        if ema_decay is not None and not 0.0 < ema_decay < 1.0:
            raise ValueError(f"seg.AdamW: ema_decay must lie in (0, 1), got {ema_decay}")
        defaults = dict(_STOCK_DEFAULTS, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite, self.ema_decay, self.ema_warmup = bool(skip_nonfinite), ema_decay, bool(ema_warmup)
        self.last = {}                  # grad_norm, clip, skipped, step: device tensors (views of the step state)
        self._swapped = False
        self._host_state = (0, None)    # (t, pows or None) the device state is created from at the next step
        self._dev = None                # device buffers, created by the first step
        self._parity = 0

    def add_param_group(self, group):
        super().add_param_group(group)
        g = self.param_groups[-1]
        for name in ("amsgrad", "maximize", "capturable"):
            if g.get(name):
                raise ValueError(f"seg.AdamW: {name}=True is not supported")
        if not 0.0 <= g["lr"] or not 0.0 <= g["eps"] or not 0.0 <= g["weight_decay"]:
            raise ValueError("seg.AdamW: lr, eps and weight_decay must not be negative")
        if not (0.0 <= g["betas"][0] < 1.0 and 0.0 <= g["betas"][1] < 1.0):
            raise ValueError(f"seg.AdamW: betas must lie in [0, 1), got {g['betas']}")
        for p in g["params"]:
            if p.dtype != torch.float32:
                raise ValueError(f"seg.AdamW: parameter dtype {p.dtype} is not supported (float32 only)")
            if p.is_sparse:
                raise ValueError("seg.AdamW: sparse parameters are not supported")
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError(f"seg.AdamW: at most {_lib.OPTIM_MAX_GROUPS} param groups")
        if getattr(self, "_dev", None) is not None:         # the device state has one product pair per group
            t, pows = self._read_state()
            pows.append((_running_product(g["betas"][0], t), _running_product(g["betas"][1], t)))
            self._host_state, self._dev = (t, pows), None

    # ---- device buffers ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _upload(dst, payload):
        """bytes -> device buffer through pinned memory, asynchronously on the current stream (the pinned block is kept
        by torch's host allocator until the copy has run)."""
        host = torch.empty(len(payload), dtype=torch.uint8, pin_memory=True)
        host.numpy()[:] = np.frombuffer(payload, dtype=np.uint8)
        dst[:len(payload)].copy_(host, non_blocking=True)

    def _pows(self, t, pows):
        return pows if pows is not None else [(_running_product(g["betas"][0], t), _running_product(g["betas"][1], t))
                                              for g in self.param_groups]

    def _device_state(self, dev):
        G = len(self.param_groups)
        if self._dev is None or self._dev["device"] != dev:
            t, pows = self._host_state if self._dev is None else self._read_state()
            image = state_bytes(t, self._pows(t, pows))
            state = torch.empty(len(image), dtype=torch.uint8, device=dev)
            self._upload(state, image)
            slot = 8 + 16 * G
            self._dev = {"device": dev, "state": state, "groups": torch.empty(64 * G, dtype=torch.uint8, device=dev),
                         "group_bytes": None, "table": None, "sig": None, "blocks": 0, "part": None,
                         "views": [{"grad_norm": state[0:8].view(torch.float64)[0], "clip": state[8:12].view(torch.float32)[0],
                                    "skipped": state[16:20].view(torch.int32)[0],
                                    "step": state[32 + k * slot:36 + k * slot].view(torch.int32)[0]} for k in (0, 1)]}
            self._parity = 0
        return self._dev

    def _read_state(self):
        """(t, pows) of the device step state (synchronises: state_dict() and regrouping only)."""
        if self._dev is None:
            return self._host_state[0], self._pows(*self._host_state)
        raw = bytes(self._dev["state"].cpu().numpy())
        G = (len(raw) - 32) // 2 // 16
        off = 32 + self._parity * (8 + 16 * G)
        t = struct.unpack_from("<i", raw, off)[0]
        flat = struct.unpack_from(f"<{2 * G}d", raw, off + 8)
        return t, [(flat[2 * i], flat[2 * i + 1]) for i in range(G)]

    def _init_state(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        if self.ema_decay is not None and "ema" not in st:
            st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)     # the shadow starts from the parameter
        return st

    def _set_table(self, d, rows, dev):
        sig = tuple(rows)
        if d["sig"] != sig:
            tab, blocks = build_table(rows)
            if d["table"] is None or d["table"].numel() < 64 * len(rows):
                d["table"] = torch.empty(64 * len(rows), dtype=torch.uint8, device=dev)
            self._upload(d["table"], bytes(tab))
            d["sig"], d["blocks"] = sig, blocks
        return d["blocks"]

    # ---- the step ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._swapped:
            raise RuntimeError("seg.AdamW.step() inside ema_weights(): the parameters hold the EMA")
        rows, dev = [], None
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                ops._require_cuda(p, "seg.AdamW.step")
                if g.is_sparse:
                    raise ValueError("seg.AdamW: sparse gradients are not supported")
                if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or not p.is_contiguous():
                    raise ValueError("seg.AdamW: parameters and gradients must be dense contiguous float32 on one device")
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise ValueError("seg.AdamW: all parameters must live on one device")
                if p.numel() == 0:
                    continue
                st = self._init_state(p)
                rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             st["ema"].data_ptr() if "ema" in st else 0, p.numel(), gi))
        if not rows:
            return loss
        with torch.cuda.device(dev):
            d = self._device_state(dev)
            blocks = self._set_table(d, rows, dev)
            gbytes = b"".join(group_scalars(g, self.ema_decay) for g in self.param_groups)
            if gbytes != d["group_bytes"]:
                self._upload(d["groups"], gbytes)
                d["group_bytes"] = gbytes
            G, stream = len(self.param_groups), ops._stream()
            normed = self.max_grad_norm is not None or self.skip_nonfinite
            skip = _lib.OPTIM_SKIP_NONFINITE if self.skip_nonfinite else 0
            if normed:
                if d["part"] is None or d["part"].numel() < blocks:
                    d["part"] = torch.empty(blocks, dtype=torch.float64, device=dev)
                _lib.call("segk_optim_grad_norm", d["table"].data_ptr(), len(rows), blocks, d["groups"].data_ptr(), G,
                          d["state"].data_ptr(), d["part"].data_ptr(), self.max_grad_norm or 0.0,
                          (_lib.OPTIM_CLIP if self.max_grad_norm is not None else 0) | skip, self._parity, stream)
            warm = _lib.OPTIM_EMA_WARMUP if self.ema_warmup and self.ema_decay is not None else 0
            _lib.call("segk_optim_adamw", d["table"].data_ptr(), len(rows), blocks, d["groups"].data_ptr(), G,
                      d["state"].data_ptr(), (_lib.OPTIM_NORMED if normed else 0) | skip | warm, self._parity, stream)
        self._parity ^= 1
        self.last = d["views"][self._parity]
        return loss

    # ---- EMA --------------------------------------------------------------------------------------------------------------
    def _exchange(self):
        rows, dev = [], None
        for group in self.param_groups:
            for p in group["params"]:
                s = self.state.get(p, {}).get("ema")
                if s is None or p.numel() == 0:
                    continue
                ops._require_cuda(p, "seg.AdamW.ema_weights")
                dev = p.device
                rows.append((p.data_ptr(), 0, 0, 0, s.data_ptr(), p.numel(), 0))
        if rows:
            with torch.cuda.device(dev):
                tab, blocks = build_table(rows)
                table = torch.empty(64 * len(rows), dtype=torch.uint8, device=dev)
                self._upload(table, bytes(tab))
                _lib.call("segk_optim_adamw", table.data_ptr(), len(rows), blocks, 0, 0, 0, _lib.OPTIM_SWAP, 0, ops._stream())
        ops.invalidate_packed_weights()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside: every parameter holds its EMA and the shadow holds the live weights (exchanged in place by one launch, no
        temporaries); packed weight copies are invalidated on entry and on exit.  Not re-entrant; step() inside raises."""
        if self._swapped:
            raise RuntimeError("seg.AdamW.ema_weights() is not re-entrant")
        if self.ema_decay is None:
            raise RuntimeError("seg.AdamW.ema_weights() needs ema_decay")
        self._exchange()
        self._swapped = True
        try:
            yield self
        finally:
            self._exchange()
            self._swapped = False

    def ema_state_dict(self, model):
        """model.state_dict() with every optimised parameter replaced by a clone of its shadow (a parameter that has not
        taken a step yet keeps its own value); buffers -- BatchNorm running statistics -- stay the live model's."""
        if self.ema_decay is None:
            raise RuntimeError("seg.AdamW.ema_state_dict() needs ema_decay")
        sd = model.state_dict()
        for name, p in model.named_parameters():
            s = self.state.get(p, {}).get("ema")
            if name in sd and s is not None:
                sd[name] = (p if self._swapped else s).detach().clone()
        return sd

    # ---- checkpoints: torch.optim.AdamW's layout, "ema" and "bias_products" beside it ------------------------------------------
    def state_dict(self):
        t, pows = self._read_state()
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(float(t))
        sd = super().state_dict()
        for g, pw in zip(sd["param_groups"], pows):
            g["bias_products"] = [float(pw[0]), float(pw[1])]
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        pows = [g.pop("bias_products", None) for g in self.param_groups]
        steps = [int(st["step"]) for st in self.state.values() if "step" in st]
        t = max(steps) if steps else 0
        for g in self.param_groups:
            for name in ("amsgrad", "maximize", "capturable"):
                if g.get(name):
                    raise ValueError(f"seg.AdamW: {name}=True is not supported")
        self._host_state = (t, None if any(p is None for p in pows) else [tuple(p) for p in pows])
        self._dev, self._parity, self.last = None, 0, {}
