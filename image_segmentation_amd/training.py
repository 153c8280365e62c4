"""Training / evaluation driver -- drop-in for the reference's utils/training.py (train_loop :18-64, eval_loop :67-121,
trainReconstruction :123-151, train_loop_prompt :153-199, evalReconstruction :202-239, eval_loop_prompt :242-296,
start_prompt :299-450, start :453-618) plus train_loop_distill (no counterpart there): same signatures, same
accumulation/step/zero_grad order, same returned averages, same checkpoint dictionary keys.  Pure host logic: the model, loss
and metrics it drives are the HIP-backed modules of this package (or anything honouring the same nn.Module protocol).

Two pieces exist once and the loops are thin callers of them: `_run_window`, the gradient-accumulation
window of the four train loops (`_segmentation_epoch` adds what the three segmentation loops keep and print), and
`_eval_pass`, the per-batch pass of the three evaluation loops (`_segmentation_eval` adds the per-image body, the reduction
and the report of the two segmentation ones).  `start` and `start_prompt` share `_start`.

Differences from the reference, all deliberate:
  * progress bars use tqdm.auto when available (tqdm.notebook needs ipywidgets) and can be silenced;
  * eval_loop prints per-class IoU for agg.get_num_classes() classes instead of a hard-coded 4
    (training.py:81 raises IndexError with a 3-class aggregator);
  * an optional `grad_sync` hook (parallel.GradSync) all-reduces gradients over RCCL right before
    the optimizer's step -- absent in the single-process reference;
  * trainReconstruction / evalReconstruction take the device as an argument (default: the model's parameter device; the
    reference reads a module-global) and keep the per-batch / per-image losses on the device, copying them to the host
    once at the end instead of one `.item()` sync per batch or image.
"""
import os

import numpy as np
import torch

from .metrics import MetricsHistory
from .utils import process_batch_forward, process_batch_reverse, NEAREST

try:                                    # plain tqdm; the reference's tqdm.notebook needs ipywidgets
    from tqdm.auto import tqdm as _tqdm
except Exception:                       # pragma: no cover
    _tqdm = None

VERBOSE = True


def _bar(it, **kw):
    if _tqdm is None or not VERBOSE:
        return it
    return _tqdm(it, **kw)


def _accumulate(agg, pred, label):
    """MetricsHistory.accumulate, through the sync-free device path when the aggregator offers one."""
    fn = getattr(agg, "accumulate_deferred", None)
    (fn or agg.accumulate)(pred, label)


def _say(*a):
    if VERBOSE and _rank_world()[0] == 0:
        print(*a)


def _rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _reduce_eval(total_loss, num_images, agg, device):
    """Data-parallel evaluation: sum the loss, the image count and the aggregator's TP/FP/FN/TN over the ranks, so that
    every rank holds the same epoch metrics (and takes the same "improved?" decision).  Correct both when the validation
    set is sharded over the ranks and when every rank walks all of it (every count is then multiplied by the world
    size, which cancels in the loss average and in IoU / Dice / accuracy)."""
    import torch.distributed as dist
    flush = getattr(agg, "flush", None)
    if flush is not None:
        flush()
    C = agg.get_num_classes()
    dev = torch.device(device) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.zeros(2 + 4 * C, dtype=torch.float64, device=dev)
    t[0], t[1] = total_loss, num_images
    t[2:] = torch.cat([agg.total_tp, agg.total_fp, agg.total_fn, agg.total_tn]).to(dev)
    dist.all_reduce(t)
    t = t.cpu()
    for i, name in enumerate(("total_tp", "total_fp", "total_fn", "total_tn")):
        getattr(agg, name).copy_(t[2 + i * C:2 + (i + 1) * C])
    return t[0].item(), int(round(t[1].item()))


def _run_window(dataloader, model, batch_loss, optimizer, accumulation_steps, grad_sync, *, scheduler, zero_first, on_loss):
    """The gradient-accumulation window of every train loop, once (training.py:18-64, :123-151, :153-199).

    Per micro-batch: `batch_loss(batch)` -> the UNSCALED loss (the caller's unpacking, resize + pad, device moves, forward
    call(s) and loss call); loss / accumulation_steps is backpropagated.  A micro-batch is *stepping* when it closes a window
    of `accumulation_steps` or is the last of the loader: grad_sync (parallel.GradSync, may be None) is armed before that
    backward so that the all-reduce overlaps it and waited for after it, then the optimizer steps, the scheduler (if
    any) steps and the gradients are cleared.  `zero_first` clears the gradients before the first batch as well (the
    reconstruction loop does not: gradients present on entry are part of its first step).  `on_loss(loss, stepping, pbar)`
    ends every micro-batch: it is where a caller keeps what it returns of the losses."""
    model.train()
    if zero_first:
        optimizer.zero_grad()

    n = len(dataloader)
    pbar = _bar(dataloader, total=n, desc="Training")
    for batch_idx, batch in enumerate(pbar):
        loss = batch_loss(batch)

        scaled_loss = loss / accumulation_steps
        stepping = (batch_idx + 1) % accumulation_steps == 0 or (batch_idx + 1) == n
        if grad_sync is not None and stepping:
            grad_sync.arm()               # overlap the RCCL all-reduce with this backward
        scaled_loss.backward()

        if stepping:
            if grad_sync is not None:
                grad_sync.sync()
            optimizer.step()
            if scheduler:
                scheduler.step()
            optimizer.zero_grad()
        on_loss(loss, stepping, pbar)


def _to_network(inputs, y, target_size, device):
    """A train batch on its way to the model: with a `target_size`, resize + pad (images and heat-maps bilinear, labels
    nearest); then the inputs to the device and the labels (None for an unlabelled batch) to the device as int64."""
    if target_size is not None:
        inputs = [process_batch_forward(t, target_size=target_size, device=device)[0] for t in inputs]
        if y is not None:
            y, _ = process_batch_forward(y, target_size=target_size, interpolation=NEAREST, device=device)
    inputs = [t.to(device) for t in inputs]
    if y is not None:
        y = y.to(device).long()
    return inputs, y


def _segmentation_epoch(dataloader, model, batch_loss, optimizer, accumulation_steps, scheduler, grad_sync):
    """One epoch of a segmentation model through _run_window.  Keeps the UNSCALED loss of the last micro-batch of each window
    (training.py:58,62), read right after the step and shown on the bar with the learning rate; prints and returns its
    mean over the optimizer steps (the int 0 when there was no batch)."""
    total_loss = 0.0
    processed_batches = 0

    def on_loss(loss, stepping, pbar):
        nonlocal total_loss, processed_batches
        if stepping:
            total_loss += loss.item()
            processed_batches += 1
            if hasattr(pbar, "set_postfix"):
                pbar.set_postfix({'loss': loss.item(), 'lr': optimizer.param_groups[0]['lr']})

    _run_window(dataloader, model, batch_loss, optimizer, accumulation_steps, grad_sync, scheduler=scheduler, zero_first=True,
                on_loss=on_loss)
    avg_loss = total_loss / processed_batches if processed_batches > 0 else 0
    _say(f"Training Avg loss (per effective batch): {avg_loss:>8f}")
    return avg_loss


def train_loop(dataloader, model, loss_fn, optimizer, accumulation_steps, device, scheduler=None, target_size=None,
               grad_sync=None):
    """One epoch (training.py:18-64).  Returns the mean, over optimizer steps, of the UNSCALED loss of the
    last micro-batch of each accumulation window (training.py:58,62)."""
    def batch_loss(batch):
        X, y = batch
        (X,), y = _to_network((X,), y, target_size, device)
        pred = model(X)
        return loss_fn(pred, y.squeeze(1))

    return _segmentation_epoch(dataloader, model, batch_loss, optimizer, accumulation_steps, scheduler, grad_sync)


def train_loop_prompt(dataloader, model, loss_fn, optimizer, accumulation_steps, device, scheduler=None, target_size=None,
                      grad_sync=None):
    """One epoch of the prompt model (training.py:153-199): batches are (image, heat-map, label) triples; otherwise
    the accumulation / step / averaging protocol of train_loop."""
    def batch_loss(batch):
        X, p, y = batch
        (X, p), y = _to_network((X, p), y, target_size, device)
        pred = model(X, p)
        return loss_fn(pred, y.squeeze(1))

    return _segmentation_epoch(dataloader, model, batch_loss, optimizer, accumulation_steps, scheduler, grad_sync)


def train_loop_distill(dataloader, student, teacher, loss_fn, optimizer, accumulation_steps, device, scheduler=None,
                       target_size=None, grad_sync=None):
    """One epoch of distillation: train_loop's accumulation / step / averaging protocol with the frozen
    teacher (distill.Teacher) run on the same resized batch, BEFORE the student, and loss_fn (distill.DistillLoss) called as
    loss_fn(pred, y, teacher_views).  Batches are (X, y), (X, None) or X alone; without labels y is None and the loss must be
    all soft (alpha = 1)."""
    def batch_loss(batch):
        X, y = (batch[0], batch[1] if len(batch) > 1 else None) if isinstance(batch, (tuple, list)) else (batch, None)
        (X,), y = _to_network((X,), y, target_size, device)
        views = teacher(X)
        pred = student(X)
        return loss_fn(pred, None if y is None else y.squeeze(1), views)

    return _segmentation_epoch(dataloader, student, batch_loss, optimizer, accumulation_steps, scheduler, grad_sync)


def _model_device(model):
    p = next(iter(model.parameters()), None)
    return p.device if p is not None else torch.device("cpu")


def _host_f64(losses):
    """Scalar loss tensors (or numbers) -> float64 numpy array in ONE device-to-host copy: the values the reference's
    per-batch `.item()` list holds."""
    if not losses:
        return np.array([], dtype=np.float64)
    ts = [torch.as_tensor(v).detach().reshape(()).float() for v in losses]
    return torch.stack([t.to(ts[0].device) for t in ts]).cpu().double().numpy()


def trainReconstruction(dataloader, model, loss_fn, optimizer, accumulation_steps, device=None, grad_sync=None):
    """One epoch of reconstruction pretraining (training.py:123-151): loss_fn(model(X), X) for every (X, _) batch through
    _run_window.  Like the reference there is no zero_grad before the first batch, no scheduler and no printed line.
    Returns the mean UNSCALED loss over EVERY micro-batch (train_loop averages the stepping micro-batches only), kept on
    the device until the end."""
    if device is None:
        device = _model_device(model)
    losses = []

    def batch_loss(batch):
        X, _ = batch
        X = X.to(device)
        pred = model(X)
        return loss_fn(pred, X)

    _run_window(dataloader, model, batch_loss, optimizer, accumulation_steps, grad_sync, scheduler=None, zero_first=False,
                on_loss=lambda loss, stepping, pbar: losses.append(loss.detach()))
    return np.mean(_host_f64(losses))


def _eval_pass(batches, model, device, target_size, interpolation, per_image):
    """The per-batch evaluation pass of every evaluation loop, once (training.py:67-121, :202-239, :242-296); the model is
    in eval mode already.  `batches` yields (inputs, sources): `inputs` is a tuple of image lists -- the images, then the
    heat-maps if the model takes them -- and `sources` holds one item per image for `per_image`.  Every input is resized
    + padded to `target_size` (a heat-map takes its image's treatment) and moved to the device, the model runs under
    no_grad, its output is taken back to each image's ORIGINAL size with `interpolation`, and `per_image(pred, source)`
    is called for every image with pred [C, H, W] on the device.  no_grad is held here, around the callable, never across a
    yield: grad mode is global to the thread."""
    with torch.no_grad():
        for inputs, sources in batches:
            X, meta_list = process_batch_forward(inputs[0], target_size=target_size, device=device)
            more = [process_batch_forward(t, target_size=target_size, device=device)[0] for t in inputs[1:]]
            preds = model(X.to(device), *[t.to(device) for t in more])

            preds = process_batch_reverse(preds, meta_list, interpolation=interpolation)

            for pred, source in zip(preds, sources):
                per_image(pred.to(device), source)


def _segmentation_eval(batches, model, loss_fn, device, target_size, agg, num_classes, grad_sync):
    """eval_loop and eval_loop_prompt after their own first lines (eval mode, the aggregator's class count `num_classes`,
    eval_loop's reset): _eval_pass with the per-image loss at the original size and the confusion counts, then the
    epoch's reduction, metrics and report.  Returns (avg_loss, mean_dice, mean_iou).
    A loss on the GPU stays there (float64 device sum, counts through the aggregator's deferred path, one sync at the end);
    a CPU loss never takes the deferred path."""
    num_images_processed = 0
    total_loss = 0.0
    total_dev = None

    def per_image(pred, label):
        nonlocal num_images_processed, total_loss, total_dev
        label = label.to(device).long()

        loss = loss_fn(pred.unsqueeze(0), label.unsqueeze(0).squeeze(1))
        if loss.is_cuda:        # device path: per-image losses and confusion counts stay on the GPU until the end
            total_dev = loss.detach().double() if total_dev is None else total_dev + loss.detach().double()
            _accumulate(agg, pred, label)
        else:
            total_loss += loss.item()
            agg.accumulate(pred, label)

        num_images_processed += 1

    _eval_pass(batches, model, device, target_size, 'bilinear', per_image)

    if total_dev is not None:
        total_loss += total_dev.item()  # float64 sum of the float32 losses, as the reference's `+= loss.item()` builds
    if grad_sync is not None and _rank_world()[1] > 1:
        total_loss, num_images_processed = _reduce_eval(total_loss, num_images_processed, agg, device)
    avg_loss = total_loss / num_images_processed

    mean_dice, mean_iou, mean_acc = agg.compute_epoch_metrics()
    per_class_iou = agg.get_last_per_class_iou()
    ignore_index = agg.get_ignore_index()

    _say(f"\n--- Evaluation Complete ---")
    _say(f"  Images Processed: {num_images_processed}")
    _say(f"  Average Loss (Original Size): {avg_loss:>8f}")
    _say(f"  Ignored Class : {ignore_index}")
    _say(f"  Macro Avg Acc score: {mean_acc:>8f}")
    _say(f"  Macro Avg Dice Score: {mean_dice:>8f}")
    _say(f"  Mean IoU (mIoU): {mean_iou:>8f}")
    _say(f"  --- Per-Class IoU ---")
    for c in range(num_classes):
        _say(f"    Class {c}: {per_class_iou[c].item():>8f}")
    _say("-" * 25)

    return avg_loss, mean_dice, mean_iou


def eval_loop(dataloader, model, loss_fn, device, target_size, agg, grad_sync=None):
    """training.py:67-121: resize+pad -> model (eval mode, no_grad) -> reverse resize -> per-image loss at
    the ORIGINAL size and confusion counts.  Returns (avg_loss, mean_dice, mean_iou)."""
    model.eval()
    num_classes = agg.get_num_classes()
    agg.reset()         # training.py:82.  Here ONLY: the reference's prompt loop (:242-296) never resets its aggregator
    batches = (((X,), y) for X, y in _bar(dataloader, desc="Eval"))
    return _segmentation_eval(batches, model, loss_fn, device, target_size, agg, num_classes, grad_sync)


def eval_loop_prompt(dataloader, model, loss_fn, device, target_size, agg, grad_sync=None):
    """training.py:242-296: eval_loop for (image, heat-map, label) batches; the heat-map takes the image's
    resize + pad.  No agg.reset(), as in the reference.  Returns (avg_loss, mean_dice, mean_iou)."""
    model.eval()
    num_classes = agg.get_num_classes()
    batches = (((X, p), y) for X, p, y in _bar(dataloader, desc="Eval"))
    return _segmentation_eval(batches, model, loss_fn, device, target_size, agg, num_classes, grad_sync)


def evalReconstruction(dataloader, model, loss_fn, target_size, interpolation='bilinear', device=None):
    """training.py:202-239: resize+pad -> model (eval mode, no_grad) -> reverse resize -> per-image loss against the
    ORIGINAL image (an RGBA image is cut to RGB, :231-232).  Returns (sum of per-image losses / number of batches,
    mean per-image loss) -- the reference's two figures."""
    if device is None:
        device = _model_device(model)
    model.eval()
    num_batches = len(dataloader)
    losses = []

    def per_image(p, label):
        p = p.unsqueeze(0)
        label = label.to(device).unsqueeze(0)
        if label.shape[1] == 4 and label.ndim == 4:
            label = label[:, :3, :, :]
        losses.append(loss_fn(p, label.squeeze(1)).detach())

    batches = (((X,), X) for X, _ in _bar(dataloader, total=num_batches, desc="Evaluation"))
    _eval_pass(batches, model, device, target_size, interpolation, per_image)
    vals = _host_f64(losses)
    total_loss = 0.0
    for v in vals:                      # the reference's running `total_loss += loss.item()`
        total_loss += float(v)
    return total_loss / num_batches, np.mean(vals)


def start(*args, **kwargs):
    """training.py:453-618: optional resume, epoch loop, per-epoch metrics file, best-mIoU checkpoint
    (+ weights-only "MO_<name>").  Checkpoint keys are the reference's."""
    return _start(False, *args, **kwargs)


def start_prompt(*args, **kwargs):
    """training.py:299-450: `start` for the prompt model -- the prompt loops, a full (pickled) checkpoint load, the
    metrics history stored inside the checkpoint and no weights-only "MO_" file."""
    return _start(True, *args, **kwargs)


def _start(
        prompt: bool,
        model_save_dir: str,
        model_save_name: str,
        model,
        optimizer,
        train_dataloader,
        val_dataloader,
        accumulation_steps: int,
        device,
        train_loss_fn,
        val_loss_fn,
        target_size: int,
        scheduler=None,
        agg: MetricsHistory = None,
        load: bool = True,
        save: bool = True,
        num_classes: int = 4,
        ignore_index: int = 3,
        epochs: int = 100,
        grad_sync=None,
):
    start_epoch = 0
    best_dev_dice = -np.inf
    best_dev_miou = -np.inf
    best_dev_loss = np.inf
    # data parallel (grad_sync given, one process per GPU): every rank loads the same checkpoint, rank 0's BatchNorm
    # running statistics are broadcast before evaluation (they are per replica during training), the evaluation
    # counts are summed over the ranks so that all ranks take the same decision, and ONLY rank 0 writes files.
    rank, world = _rank_world()

    os.makedirs(model_save_dir, exist_ok=True)
    os.makedirs(f"{model_save_dir}/metrics", exist_ok=True)
    path = f"{model_save_dir}/{model_save_name}"
    if load and os.path.isfile(path):
        _say(f"Loading checkpoint from: {path}")
        checkpoint = torch.load(path, map_location=device, weights_only=not prompt)   # training.py:351 vs :506
        model.load_state_dict(checkpoint["model_state_dict"])
        _say(" -> Model state loaded.")
        try:
            optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
            _say(" -> Optimizer state loaded.")
        except Exception as e:
            _say(f" -> Warning: Could not load optimizer state: {e}. Optimizer will start from scratch.")
        try:
            scheduler.load_state_dict(checkpoint["scheduler_state_dict"])
            _say(" -> Scheduler state loaded.")
        except Exception as e:
            _say(f" -> Warning: Could not load scheduler state: {e}. Scheduler will start from scratch.")
        try:
            agg = checkpoint.get("history")
            agg.to(device)
            _say(" -> Metrics History loaded.")
        except Exception:
            _say(" -> No metric history saved")
            agg = MetricsHistory(num_classes, ignore_index)
        start_epoch = checkpoint.get("epoch", 0)
        best_dev_dice = checkpoint.get("best_dev_dice", -np.inf)
        best_dev_miou = checkpoint.get("best_dev_miou", -np.inf)
        best_dev_loss = checkpoint.get("best_dev_loss", np.inf)
        _say(f" -> Resuming training from epoch {start_epoch + 1}")
        _say(f" -> Loaded best metrics: Dice={best_dev_dice:.6f}, mIoU={best_dev_miou:.6f}, Loss={best_dev_loss:.6f}")
        _say(f" -> Notes from checkpoint: {checkpoint.get('notes', 'N/A')}")
    else:
        _say(f"Checkpoint file not found at {path}. Starting training from scratch.")
    if agg is None:
        agg = MetricsHistory(num_classes, ignore_index)

    _say("\nStarting Training...")
    for t in range(start_epoch, epochs):
        _say(f"Epoch {t+1}\n-------------------------------")
        tl, el = (train_loop_prompt, eval_loop_prompt) if prompt else (train_loop, eval_loop)
        tl(train_dataloader, model, train_loss_fn, optimizer, accumulation_steps, device, scheduler, target_size,
           grad_sync=grad_sync)
        if grad_sync is not None:
            grad_sync.broadcast_buffers(model)
        val_loss, val_dice, val_miou = el(val_dataloader, model, val_loss_fn, device, target_size, agg, grad_sync=grad_sync)
        writer = save and rank == 0

        if writer:
            torch.save({"epoch": t + 1, "history": agg}, f"{model_save_dir}/metrics/{model_save_name}")

        if val_miou > best_dev_miou:
            best_dev_dice, best_dev_miou, best_dev_loss = val_dice, val_miou, val_loss
            if writer:
                _say(f"Validation IoU score improved ({best_dev_miou:.6f}). Saving model...")
                checkpoint = {
                    "epoch": t + 1,
                    "model_state_dict": model.state_dict(),
                    "optimizer_state_dict": optimizer.state_dict(),
                    "best_dev_dice": best_dev_dice,
                    "best_dev_miou": best_dev_miou,
                    "best_dev_loss": best_dev_loss,
                    "notes": f"Model saved based on best Micro Dice. Ignored index for metric: {ignore_index}",
                }
                if scheduler:
                    checkpoint["scheduler_state_dict"] = scheduler.state_dict()
                if prompt:
                    checkpoint["history"] = agg                      # training.py:424
                torch.save(checkpoint, path)
                if not prompt:
                    torch.save({"epoch": t + 1, "model_state_dict": model.state_dict()},
                               f"{model_save_dir}/MO_{model_save_name}")
        else:
            _say(f"Validation IoU score did not improve from {best_dev_miou:.6f}")
        if world > 1 and save:
            import torch.distributed as dist
            dist.barrier()                # nobody reads or overwrites a file rank 0 is still writing

    _say("\n--- Training Finished! ---")
    _say(f"Best validation IoU score achieved: {best_dev_miou:.6f}")
    _say(f"Corresponding validation dice: {best_dev_dice:.6f}")
    _say(f"Corresponding validation loss: {best_dev_loss:.6f}")
    return best_dev_miou, best_dev_dice, best_dev_loss
