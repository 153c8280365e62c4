"""Prediction with a trained model -- the arithmetic of the reference's demo service (prompt_based/segmentation_webapp/
app.py:38-88 load_model, :250-326 decode -> to_tensor -> resize + pad -> model -> reverse -> argmax(0) -> uint8 ->
COLOR_MAP) as a library call; the Flask / base64 / HTML part and create_prompt_mask stay out.

    model = load_checkpoint(seg.unet(3, 4), "unet.pt").cuda()
    pred = Segmenter(model)([np.asarray(PIL.Image.open("cat.jpg").convert("RGB"))])[0]
    PIL.Image.fromarray(pred.color.cpu().numpy(), "RGB").save("cat_mask.png")

Both ends of the forward are HIP kernels of their own (csrc/resize.hip): segk_resize_pad_u8 takes the decoder's 8-bit
interleaved image straight into the network batch, and segk_predict_mask goes from the network output to the uint8 class
mask, the RGB image, the class counts and (with labels) the confusion counts in one pass, without storing the full-size
logits that process_batch_reverse + argmax + a palette index would.  Nothing here synchronises with the host when the
inputs are already on the device; there is no CPU path.

Several views of an image -- flips and target sizes (tta=TTA(...)) and several models (a list: an ensemble) -- are merged
by segk_predict_merge in one pass per image from the views' network outputs: the mask, colour, counts,
confusion counts and a confidence map, again without full-size float images.

tiles=Tiles(...) is the route for images larger than the training crop: the image is cut at its own
resolution into overlapping tiles (segk_tile_gather / _u8), the tiles run as network batches, and segk_predict_tiles blends
the overlapping outputs into the same set of outputs in one pass; nothing is resampled."""
import contextlib
import inspect
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, ops, prompts, tiles as _tiles, tta as _tta
from .augment import _upload
from .clipunet import ClipUNet
from .components import Components, as_clean, components as _components
from .morph import as_morph
from .superpixels import as_snap
from .vectors import as_vectors, vectorize as _vectorize
from . import utils as U

# app.py:187-208 -- the demo's palette and the two class-name tables
COLOR_MAP = {0: (0, 0, 0), 1: (255, 0, 0), 2: (0, 255, 0), 3: (0, 0, 255)}
CLASS_NAMES = {"standard": {0: "Background", 1: "Cat", 2: "Dog", 3: "Boundary"},
               "prompt_model": {0: "Deactivated", 1: "Background+Boundary", 2: "Cat", 3: "Dog"}}


def load_checkpoint(model, path, map_location="cpu", strict=True):
    """app.py:65-84 -- load a checkpoint file into an already built model and return it in eval() mode.  The file may
    hold {"model_state_dict": ...}, {"state_dict": ...} or a bare state dict; a `module.` prefix (DataParallel /
    DistributedDataParallel) is stripped from the keys.  Host-only."""
    checkpoint = torch.load(path, map_location=map_location, weights_only=False)
    if "model_state_dict" in checkpoint:
        state_dict = checkpoint["model_state_dict"]
    elif "state_dict" in checkpoint:
        state_dict = checkpoint["state_dict"]
    else:
        state_dict = checkpoint
    state_dict = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    model.load_state_dict(state_dict, strict=strict)
    return model.eval()


@dataclass
class Prediction:
    mask: torch.Tensor                      # uint8 [H,W] class indices at the image's own size
    color: Optional[torch.Tensor]           # uint8 [H,W,3] (what Image.fromarray(..., "RGB") takes), None without a palette
    counts: torch.Tensor                    # int64 [C] pixels per predicted class
    confusion: Optional[torch.Tensor]       # int64 [C,C], [pred][label]; None without labels
    meta: dict                              # the resize / padding record of process_batch_forward
    raw_mask: Optional[torch.Tensor] = None         # with snap=, morph= or clean=: the argmax (mask is the finished one)
    components: Optional[Components] = None    # with clean=: the components of the mask it was given (components.py)
    # set on merged views, None otherwise; attributes, not dataclass fields: the constructor stays as it was
    confidence = None                          # uint8 [H,W], (uint8)(255 p_best + 0.5)
    scores = None                              # Segmenter(return_scores=True): float32 [C,H,W], the merged probabilities
    vectors = None                             # Segmenter(vectors=...): the vectors.Vectors of `mask`
    superpixels = None                         # Segmenter(snap=...): the superpixels.Superpixels of the input image


def _num_classes(model):
    """Classes of the model's output head, read from the module tree (None when it cannot be told before a forward)."""
    if hasattr(model, "clip") and hasattr(model, "mask"):              # PromptModel: the probabilities of its CLIP branch
        return _num_classes(model.clip)
    for name in ("output", "output_layer", "finalConv"):
        head = getattr(model, name, None)
        if isinstance(head, torch.nn.Conv2d):
            return head.out_channels
    convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    return convs[-1].out_channels if convs else None


def _palette_tensor(palette):
    if palette is None:
        return None
    if isinstance(palette, dict):
        if sorted(palette) != list(range(len(palette))):
            raise ValueError("palette: a mapping must have the keys 0..K-1")
        palette = [palette[k] for k in range(len(palette))]
    t = torch.as_tensor(np.asarray(palette)).cpu()
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1 or bool(((t < 0) | (t > 255)).any()):
        raise ValueError(f"palette: expected K rows of three values in 0..255, got shape {tuple(t.shape)}")
    return t.to(torch.uint8).contiguous()


def _check_classes(C, pal):
    if C > _lib.MAX_CLASSES:
        raise ValueError(f"the model has {C} classes, prediction supports at most {_lib.MAX_CLASSES}")
    if pal is not None and pal.shape[0] < C:
        raise ValueError(f"palette has {pal.shape[0]} rows, the model has {C} classes")


def _as_tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a


def _source(image, c, what):
    """One image or heat-map, checked against a batch of c channels -> (src, u8, cin, H, W): the contiguous tensor a kernel
    reads and whether it is the 8-bit form, uint8 [H,W,cin] (cin of 4: RGBA, the kernels drop A), or the float one, float32
    [cin,H,W]."""
    if image.dtype == torch.uint8:
        if image.ndim == 2:
            image = image.unsqueeze(-1)
        if image.ndim != 3 or image.shape[2] not in (1, 3, 4):
            raise ValueError(f"{what}: 8-bit inputs are [H,W,C] with 1, 3 or 4 channels (or [H,W]), got {tuple(image.shape)}")
        H, W, cin = image.shape
        if min(cin, 3) != c:
            raise ValueError(f"{what}: {min(cin, 3)} channels where the batch has {c}")
        src = image.contiguous()
        if cin == 4 and src.data_ptr() % 4:
            src = src.clone()
        return src, True, cin, H, W
    if not torch.is_floating_point(image) or image.ndim != 3:
        raise ValueError(f"{what}: expected a float [C,H,W] tensor or a uint8 [H,W,C] image, got {image.dtype} {tuple(image.shape)}")
    if image.shape[0] == 4:
        image = image[:3]
    cin, H, W = image.shape
    if cin != c:
        raise ValueError(f"{what}: {cin} channels where the batch has {c}")
    return image.float().contiguous(), False, cin, H, W


def _into_slot(image, slot, T, interpolation, antialias, what, flip=0):
    """One image or heat-map -> its slot [c,T,T]: uint8 [H,W,Cin] / [H,W] through segk_resize_pad_u8, float [C,H,W]
    through segk_resize_pad; with flip (bit 0: x, bit 1: y) the slot of the flipped image, through their _flip forms.
    Returns the metadata."""
    src, u8, cin, H, W = _source(image, slot.shape[0], what)
    if not u8 and not flip:
        return U._resize_pad_into(src, slot, T, interpolation, antialias)
    nh, nw, pt, pl, meta = U._geometry(H, W, T)
    args = (src.data_ptr(), slot.data_ptr(), cin, H, W, nh, nw, T, pt, pl, U._resize_mode(interpolation, antialias))
    if not u8:
        _lib.call("segk_resize_pad_flip", *args, 0, flip, ops._stream())
    elif flip:
        _lib.call("segk_resize_pad_u8_flip", *args, flip, ops._stream())
    else:
        _lib.call("segk_resize_pad_u8", *args, ops._stream())
    return meta


def _slots(dev, images, heatmaps, T, interpolation, antialias, flip=0):
    """The network batch of one (size, flip) -> (X [n,c,T,T], Hm [n,1,T,T] or None, the images' metadata)"""
    n = len(images)
    X = torch.empty((n, _channels(images[0]), T, T), dtype=torch.float32, device=dev)
    metas = [_into_slot(im, X[k], T, interpolation, antialias, "image", flip) for k, im in enumerate(images)]
    if heatmaps is None:
        return X, None, metas
    Hm = torch.empty((n, 1, T, T), dtype=torch.float32, device=dev)
    for k, hm in enumerate(heatmaps):
        hm = _as_tensor(hm).to(dev, non_blocking=True)      # the merged route has uploaded it already, once for all its views
        hmeta = _into_slot(hm, Hm[k], T, interpolation, antialias, "heatmap", flip)
        if hmeta["original_size"] != metas[k]["original_size"]:
            raise ValueError(f"heatmap {k} is {hmeta['original_size']}, its image {metas[k]['original_size']}")
    return X, Hm, metas


def _forward(model, X, Hm, who, inv_T=None):
    """model(X) or model(X, Hm) -> its output, checked to be [n,C,T,T] on the device, as contiguous float32 (times inv_T).
    who = (the model, the caller) as the messages name them: ("model 1", "Segmenter")"""
    y = model(X) if Hm is None else model(X, Hm)
    ops._require_cuda(y, f"{who[1]} (model output)")
    y = y.detach()
    if y.ndim != 4 or y.shape[0] != X.shape[0] or y.shape[2] != X.shape[2] or y.shape[3] != X.shape[3]:
        raise ValueError(f"{who[0]} returned {tuple(y.shape)} for a batch {tuple(X.shape)}")
    if y.dtype != torch.float32 or not y.is_contiguous():
        y = y.float().contiguous()
    return y if inv_T is None else y * inv_T


def _label_on(lab, size, dev, k):
    """Label map k, checked to be an integer [H,W] / [1,H,W] map of `size` -> int64 on the device"""
    lab = _as_tensor(lab)
    if torch.is_floating_point(lab) or tuple(lab.shape) not in (tuple(size), (1,) + tuple(size)):
        raise ValueError(f"labels {k}: expected an integer map of {tuple(size)}, got {lab.dtype} {tuple(lab.shape)}")
    return lab.to(dev, non_blocking=True).long().contiguous()


@contextlib.contextmanager
def _eval_mode(models):
    """eval() on every model; each module's own training flag is put back on the way out"""
    modes = [(m, m.training) for model in models for m in model.modules()]
    try:
        for model in models:
            model.eval()
        yield
    finally:
        for m, was in modes:
            m.training = was


def _channels(image):
    if image.dtype == torch.uint8:
        return 1 if image.ndim == 2 else min(int(image.shape[-1]), 3)
    return min(int(image.shape[0]), 3)


def _arity(model):
    """True for a model whose forward takes (image, heatmap)"""
    return len([p for p in inspect.signature(model.forward).parameters.values()
                if p.default is p.empty and p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]) >= 2


def _is_prompt_model(model):
    return hasattr(model, "clip") and hasattr(model, "mask")


def _fixed_input_size(model):
    """The one input size a ClipUNet (alone or inside a PromptModel) accepts, None for the convolutional models."""
    clip = model.clip if _is_prompt_model(model) else model
    config = getattr(getattr(clip, "encoder", None), "config", None) if isinstance(clip, ClipUNet) else None
    return None if config is None else int(config.image_size)


def _image_size(image):
    return tuple(image.shape[:2]) if image.dtype == torch.uint8 else tuple(image.shape[-2:])


def _gather_tiles(image, out, T, overlap, pad, tile0, what):
    """Tiles tile0 .. tile0 + len(out) - 1 of one image or heat-map -> out [m,c,T,T]: uint8 [H,W,Cin] / [H,W] through
    segk_tile_gather_u8, float [C,H,W] through segk_tile_gather."""
    src, u8, cin, H, W = _source(image, int(out.shape[1]), what)
    _lib.call("segk_tile_gather_u8" if u8 else "segk_tile_gather", src.data_ptr(), out.data_ptr(), cin, H, W, T, overlap, pad,
              tile0, int(out.shape[0]), ops._stream())


def _tile_size_rule(model):
    """(multiple, why): the tile sides a convolutional model accepts -- every 2x2 pooling halves the side exactly and the
    transposed convolutions double it back, so the side is a multiple of 2^poolings"""
    from .autoencoder import Encoder
    from .unet import unet
    rule = (1, "")
    for m in model.modules():
        if isinstance(m, unet):
            rule = max(rule, (16, "a U-Net pools four times"))
        elif isinstance(m, Encoder):
            rule = max(rule, (8, "the autoencoder's encoder pools three times"))
    return rule


def _resolve_outputs(outputs, models, merge):
    """outputs= -> "logits" or "probs" per model (default: "probs" for a PromptModel); "logit" merging refuses probabilities"""
    if outputs is None:
        outputs = ["probs" if _is_prompt_model(m) else "logits" for m in models]
    elif isinstance(outputs, str):
        outputs = [outputs] * len(models)
    outputs = list(outputs)
    if len(outputs) != len(models) or any(o not in _tta.KINDS for o in outputs):
        raise ValueError(f"outputs: one of {tuple(_tta.KINDS)} per model, got {outputs!r}")
    if merge == "logit" and "probs" in outputs:
        raise ValueError('merge="logit" needs models that return logits; a model here returns probabilities')
    return outputs


class Segmenter:
    """Callable prediction pipeline around a trained model: `Segmenter(model)(images)` -> list of Prediction.

    images    list of float [C,H,W] tensors (the contract of process_batch_forward) or uint8 [H,W,C] tensors / NumPy
              arrays, on the host or the device, of any sizes
    heatmaps  for two-input models (PromptModel.forward(x, heatmap)): one float [1,H,W] or uint8 [H,W] / [H,W,1] per image
    points    instead of heatmaps: per image one click (y, x) or a list of clicks, in the image's own pixels; the heat-map
              (the 8-bit Gaussian of the training data, sigma as given to the constructor; several clicks: the maximum of
              theirs) is made on the device by segk_prompt_heatmap and takes the route of a float heat-map
    labels    optional integer [H,W] / [1,H,W] maps at the images' own sizes: the confusion counts come from the same pass
              (labels outside [0,C) are skipped, as the eval loops skip 255 / ignore)

    clean=    None (every output as without it), or a components.Clean / a dict of its keywords (connectivity, classes,
              min_area, keep_largest, max_components): the mask is cleaned on the device; Prediction.mask,
              color, counts and confusion describe the cleaned mask, raw_mask is the argmax and components its components

    morph=    None (every output as without it), or a sequence of morph.MorphStep records / dicts {"op": ..., keywords}
              ("erode", "dilate", "open", "close", "fill_holes", "label_band"): the steps are applied in order to the argmax
              mask on the device, before clean=; Prediction.mask, color, counts and confusion describe the
              final mask, raw_mask is the argmax
    snap=     None (every output as without it), or a superpixels.Snap / a dict of its keywords (step, compactness, iterations,
              space, classes, min_share, fill, weighted): the argmax is snapped to the SLIC superpixels of the input image on
              the device, before morph= and clean=; the images are then uint8 [H,W,C] / [H,W], a float image is
              refused before the forward.  weighted=True lets a vote weigh the confidence map and needs a route that writes one
              (merged views or tiles).  Prediction.superpixels holds the Superpixels, raw_mask the argmax

    Merged views (without them every output and the code path are as above):
    model     a list of models is an ensemble: same class count, same input arity, all on one device
    tta=      a tta.TTA (or a dict of its keywords): the flips and target sizes each model sees and the merge ("prob" /
              "logit"); view order is models-major, then sizes, then flips
    model_weights=  one positive weight per model (equal by default); a view weighs model weight x TTA weight
    outputs=  what a model returns, "logits" or "probs", one string or one per model; default "probs" for a PromptModel,
              else "logits" ("logit" merging refuses probabilities)
    return_scores=  Prediction.scores = the merged, normalised class scores, float32 [C,H,W]
    Prediction.confidence (uint8 [H,W]) is set whenever views are merged; heat-maps and points are flipped with their image.

    Tiled full-resolution prediction (without it every output and the code path are as above):
    tiles=    a tiles.Tiles (or a dict of its keywords): the image is cut at its own size into size x size tiles (default:
              target_size) overlapping by `overlap`, and the tiles' outputs are blended ("triangle" / "flat" window, "prob" /
              "logit" merge); interpolation and antialias are not used.  batch_size counts TILES per forward: a forward is
              filled with consecutive images' tiles (at least one image), an image with more tiles runs alone in
              ceil(n / batch_size) forwards.  One model, no tta=; a ClipUNet needs size == its input size, a U-Net a multiple
              of 16, the autoencoders of 8.  outputs=, return_scores=, clean=, heatmaps / points and labels work as above;
              Prediction.confidence is always set; meta holds original_size, tile_size, overlap and tiles=(ny, nx).

    Calibrated confidence (with None every output and the code path are as above):
    temperature=  a positive float (calibration.fit_temperature finds it), or one per model of an ensemble: each model's
              logits are multiplied by the float32 1/T before the prediction kernels run.  One view: the mask is unchanged
              up to rounding and the confidence is the calibrated one; merged views under "prob": the merge itself changes.
              Refused for outputs="probs".

    Vector output (with None nothing changes on any route):
    vectors=  True or a dict of vectors.vectorize's keywords (connectivity, classes, max_components, max_runs, max_edges,
              max_rings, max_vertices): Prediction.vectors holds the run table, contour rings and corner vertices of the final
              (cleaned) mask, built on the device without a synchronisation."""

    def __init__(self, model, target_size=224, interpolation="bilinear", palette=COLOR_MAP, batch_size=32, antialias=None,
                 sigma=3.0, clean=None, tta=None, model_weights=None, outputs=None, return_scores=False, tiles=None,
                 temperature=None, vectors=None, morph=None, snap=None):
        models = list(model) if isinstance(model, (list, tuple)) else [model]
        if not models:
            raise ValueError("an ensemble needs at least one model")
        model = models[0]
        self.clean = as_clean(clean)
        self.vectors = as_vectors(vectors)
        self.morph = as_morph(morph)
        self.snap = as_snap(snap)
        if not float(sigma) > 0:
            raise ValueError(f"sigma must be positive, got {sigma}")
        self.sigma = float(sigma)
        if interpolation not in (U.BILINEAR, U.NEAREST):
            raise ValueError(f"interpolation: '{U.BILINEAR}' or '{U.NEAREST}', got {interpolation!r}")
        if int(batch_size) < 1 or int(target_size) < 1:
            raise ValueError("batch_size and target_size are positive")
        self.model, self.target_size, self.interpolation = model, int(target_size), interpolation
        self.batch_size, self.antialias = int(batch_size), antialias
        self._palette = _palette_tensor(palette)
        self._palette_dev = {}
        self._two_input = _arity(model)
        self.num_classes = _num_classes(model)
        if self.num_classes is not None:
            _check_classes(self.num_classes, self._palette)
        self.models, self.return_scores = models, bool(return_scores)
        self.tiles = None
        if tiles is not None:
            self._merged = False
            self._init_tiles(tiles, tta, model_weights, outputs)
            self._init_temperature(temperature, self.outputs)
            return
        self._merged = tta is not None or len(models) > 1 or self.return_scores
        if not self._merged:
            if self.snap is not None and self.snap.weighted:
                raise ValueError("snap: weighted=True weighs the votes by the confidence map, which this route does not write: "
                                 "pass tta=, several models, return_scores=True or tiles=")
            if model_weights is not None or outputs is not None:
                raise ValueError("model_weights= and outputs= belong to merged views: pass tta= or several models")
            self._init_temperature(temperature, ["probs" if _is_prompt_model(model) else "logits"])
            return
        if isinstance(tta, dict):
            tta = _tta.TTA(**tta)
        self.tta = _tta.TTA(flips=("",)) if tta is None else tta
        if not isinstance(self.tta, _tta.TTA):
            raise ValueError(f"tta: a TTA or a dict of its keywords, got {type(tta).__name__}")
        for k, m in enumerate(models[1:], 1):
            if _arity(m) != self._two_input:
                raise ValueError(f"model {k} takes {'(image, heatmap)' if _arity(m) else 'the image alone'}, model 0 does not")
            if None not in (_num_classes(m), self.num_classes) and _num_classes(m) != self.num_classes:
                raise ValueError(f"model {k} has {_num_classes(m)} classes, model 0 has {self.num_classes}")
        self.outputs = outputs = _resolve_outputs(outputs, models, self.tta.merge)
        self._views = _tta.view_order(len(models), self.tta, self.target_size, model_weights)
        for k, m in enumerate(models):
            fixed = _fixed_input_size(m)
            if fixed is not None and any(T != fixed for _, T, _, _ in self._views):
                raise ValueError(f"model {k} is a ClipUNet whose ViT takes {fixed} x {fixed} inputs only: "
                                 f"target_size / TTA sizes must be {fixed}")
        self._init_temperature(temperature, outputs)

    def _init_temperature(self, temperature, outputs):
        """self._inv_T: None, or per model the float32 1/T its logits are multiplied by"""
        self._inv_T = None
        if temperature is None:
            return
        if "probs" in outputs:
            raise ValueError('temperature= scales logits: it is refused for outputs="probs" (a PromptModel returns probabilities)')
        temps = list(temperature) if isinstance(temperature, (list, tuple)) else [temperature] * len(self.models)
        if len(temps) != len(self.models):
            raise ValueError(f"temperature: {len(temps)} entries for {len(self.models)} models")
        temps = _tta._positive(temps, "temperature")
        self._inv_T = [float(np.float32(1.0 / t)) for t in temps]           # 1/T in float64, rounded once

    def _init_tiles(self, tiles, tta, model_weights, outputs):
        if isinstance(tiles, dict):
            tiles = _tiles.Tiles(**tiles)
        if not isinstance(tiles, _tiles.Tiles):
            raise ValueError(f"tiles: a Tiles or a dict of its keywords, got {type(tiles).__name__}")
        if tta is not None or len(self.models) > 1 or model_weights is not None:
            raise ValueError("tiles= does not combine with tta=, several models or model_weights=")
        model = self.model
        outputs = _resolve_outputs(outputs, self.models, tiles.merge)
        size, overlap = tiles.resolve(self.target_size)
        fixed = _fixed_input_size(model)
        if fixed is not None and size != fixed:
            raise ValueError(f"the model is a ClipUNet whose ViT takes {fixed} x {fixed} inputs only: the tile size must be {fixed}")
        multiple, why = _tile_size_rule(model)
        if size % multiple:
            raise ValueError(f"tile size {size}: {why}, the tile side must be a multiple of {multiple}")
        self.tiles, self.outputs, self._tile = tiles, outputs, (size, overlap)

    def _palette_on(self, dev):
        if self._palette is None:
            return None
        if dev not in self._palette_dev:
            self._palette_dev[dev] = self._palette.to(dev)
        return self._palette_dev[dev]

    def __call__(self, images, heatmaps=None, labels=None, points=None):
        images = [_as_tensor(im) for im in images]
        n = len(images)
        if points is not None:
            if heatmaps is not None:
                raise ValueError("pass either heatmaps or points, not both")
            if not self._two_input:
                raise ValueError("points were given to a model whose forward takes the image alone")
            if len(points) != n:
                raise ValueError(f"{len(points)} point sets for {n} images")
            sizes = [_image_size(im) for im in images]
            points = [prompts._points_array(p, H, W, f"points[{k}]") for k, (p, (H, W)) in enumerate(zip(points, sizes))]
        if self._two_input and heatmaps is None and points is None:
            raise ValueError("this model takes (image, heatmap): pass heatmaps= or points=")
        if not self._two_input and heatmaps is not None:
            raise ValueError("heatmaps were given to a model whose forward takes the image alone")
        if heatmaps is not None and len(heatmaps) != n:
            raise ValueError(f"{len(heatmaps)} heatmaps for {n} images")
        if labels is not None and len(labels) != n:
            raise ValueError(f"{len(labels)} label maps for {n} images")
        if self.snap is not None:
            for k, im in enumerate(images):
                if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8:
                    raise ValueError(f"image {k}: snap= takes the superpixels of a uint8 [H,W,C] image, got "
                                     f"{getattr(im, 'dtype', type(im).__name__)} {tuple(getattr(im, 'shape', ()))}")
        params = [next(m.parameters(), None) for m in self.models]
        if any(p is None for p in params):
            raise ValueError("the model has no parameters")
        for param in params:
            ops._require_cuda(param, "Segmenter")
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise ValueError("the models of an ensemble live on one device")
        with _eval_mode(self.models), torch.no_grad(), torch.cuda.device(dev):
            if self.tiles is not None:
                return self._tiled(dev, images, heatmaps, points, labels)
            chunk = self._chunk_merged if self._merged else self._chunk
            out = []
            for i in range(0, n, self.batch_size):
                j = min(i + self.batch_size, n)
                hm = None if heatmaps is None else heatmaps[i:j]
                if points is not None:
                    hm = self._click_maps(dev, points[i:j], sizes[i:j])
                out += chunk(dev, images[i:j], hm, None if labels is None else labels[i:j])
        return out

    def _click_maps(self, dev, points, sizes):
        """click(s) -> heat-map on the device, at the image's own size"""
        return [prompts._heatmap_on(torch.from_numpy(p).to(dev, non_blocking=True), H, W, self.sigma, dev)
                for p, (H, W) in zip(points, sizes)]

    def _scale(self, m):
        return None if self._inv_T is None else self._inv_T[m]

    def _palette_for(self, dev, C):
        pal = self._palette_on(dev)
        _check_classes(C, pal)
        return pal

    def _finish(self, dev, C, pal, metas, labels, launch, confident, images):
        """The per-image end of every route: allocate the outputs, load the label map, run the route's one kernel and build
        the Prediction.  launch(k, mask, outs, conf, scores) is that kernel for image k, on pointers: outs = (color, palette,
        counts, labels, confusion), all null with snap=, morph= or clean= -- the kernel then writes the argmax (and confidence /
        scores) alone, and colour, counts and confusion counts come from the finished mask afterwards.  confident: the route
        writes a confidence map (and scores on request); metas[k]["original_size"] is the size of output k; images: the device
        images, which snap= takes its superpixels from."""
        n = len(metas)
        counts = torch.zeros((n, _lib.MAX_CLASSES), dtype=torch.int64, device=dev)
        M = torch.zeros((n, _lib.MAX_CLASSES, _lib.MAX_CLASSES), dtype=torch.int64, device=dev) if labels is not None else None
        cl, s = self.clean, ops._stream()
        preds = []
        for k, meta in enumerate(metas):
            oh, ow = meta["original_size"]
            mask = torch.empty((oh, ow), dtype=torch.uint8, device=dev)
            conf = torch.empty((oh, ow), dtype=torch.uint8, device=dev) if confident else None
            scores = torch.empty((C, oh, ow), dtype=torch.float32, device=dev) if confident and self.return_scores else None
            color = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev) if pal is not None else None
            lab = None if labels is None else _label_on(labels[k], (oh, ow), dev, k)
            outs = (ops._p(color), ops._p(pal), counts[k].data_ptr(), ops._p(lab), ops._p(None if M is None else M[k]))
            Mk = None if M is None else M[k, :C, :C]
            if cl is None and not self.morph and self.snap is None:
                launch(k, mask.data_ptr(), outs, ops._p(conf), ops._p(scores))
                pred = Prediction(mask, color, counts[k, :C], Mk, meta)
            else:
                launch(k, mask.data_ptr(), (0,) * 5, ops._p(conf), ops._p(scores))
                final, comps, sp = mask, None, None
                if self.snap is not None:
                    sp, snapped = self.snap(images[k], mask, conf)
                    final = snapped.mask
                for step in self.morph or ():
                    final = step(final)
                if cl is not None:
                    comps = _components(final, cl.connectivity, cl.classes, cl.min_area, cl.keep_largest, cl.max_components)
                    final = comps.mask
                _lib.call("segk_mask_finish", final.data_ptr(), *outs, C, oh, ow, s)
                pred = Prediction(final, color, counts[k, :C], Mk, meta, mask, comps)
                pred.superpixels = sp
            if confident:
                pred.confidence, pred.scores = conf, scores
            if self.vectors is not None:
                pred.vectors = _vectorize(pred.mask, **self.vectors)
            preds.append(pred)
        return preds

    def _chunk(self, dev, images, heatmaps, labels):
        T = self.target_size
        images = [im.to(dev, non_blocking=True) for im in images]
        X, Hm, metas = _slots(dev, images, heatmaps, T, self.interpolation, self.antialias)
        y = _forward(self.model, X, Hm, ("the model", "Segmenter"), self._scale(0))
        C = int(y.shape[1])
        pal = self._palette_for(dev, C)
        mode = 1 if self.interpolation == U.NEAREST else 0
        s = ops._stream()

        def launch(k, mask, outs, conf, scores):
            pl, pt, _, _ = metas[k]["pad"]
            _lib.call("segk_predict_mask", y[k].data_ptr(), mask, *outs, C, T, pt, pl, *metas[k]["new_size"],
                      *metas[k]["original_size"], mode, s)
        return self._finish(dev, C, pal, metas, labels, launch, False, images)

    def _chunk_merged(self, dev, images, heatmaps, labels):
        """The merged-views form of _chunk: one forward per view over the whole chunk, one table upload for all its images,
        one segk_predict_merge per image."""
        n = len(images)
        images = [im.to(dev, non_blocking=True) for im in images]
        if heatmaps is not None:
            heatmaps = [_as_tensor(hm).to(dev, non_blocking=True) for hm in heatmaps]
        # the network batches, one per (size, flip), shared by the models
        batches, metas = {}, {}
        for _, T, f, _ in self._views:
            if (T, f) not in batches:
                X, Hm, metas[T] = _slots(dev, images, heatmaps, T, self.interpolation, self.antialias, _tta.FLIPS[f])
                batches[(T, f)] = (X, Hm)
        # one forward per view, in view order
        ys, C = [], None
        for m, T, f, _ in self._views:
            y = _forward(self.models[m], *batches[(T, f)], (f"model {m}", "Segmenter"), self._scale(m))
            if C is not None and int(y.shape[1]) != C:
                raise ValueError(f"model {m} returned {int(y.shape[1])} classes, the views before it {C}")
            C = int(y.shape[1])
            ys.append(y)
        pal = self._palette_for(dev, C)
        V = len(self._views)
        table = np.zeros((n, V), dtype=_tta.VIEW_DESC)
        for k in range(n):
            rows = []
            for (m, T, f, w), y in zip(self._views, ys):
                pl, pt, _, _ = metas[T][k]["pad"]
                nh, nw = metas[T][k]["new_size"]
                rows.append((y[k].data_ptr(), T, pt, pl, nh, nw, f, self.outputs[m], w))
            table[k] = _tta.view_table(rows)
        table_dev, (p_table,) = _upload([table], dev)
        merge = _tta.MERGES[self.tta.merge]
        mode = 1 if self.interpolation == U.NEAREST else 0
        s = ops._stream()
        first = metas[self._views[0][1]]

        def launch(k, mask, outs, conf, scores):
            _lib.call("segk_predict_merge", p_table + k * V * _tta.VIEW_DESC.itemsize, V, C, merge, mode,
                      *first[k]["original_size"], mask, *outs, conf, scores, s)
        # the slots and the table (table_dev) are read by launches still in flight: the caching allocator keeps them valid
        # in stream order, as it does for the batch of the single-view path
        return self._finish(dev, C, pal, first, labels, launch, True, images)

    def _tiled(self, dev, images, heatmaps, points, labels):
        """The tiled route: forwards of at most batch_size tiles, filled across consecutive images (at least one image); an
        image with more tiles runs alone.  One segk_predict_tiles per image."""
        T, overlap = self._tile
        n = len(images)
        plans = []
        for k, im in enumerate(images):
            if im.ndim not in (2, 3):
                raise ValueError(f"image {k}: expected a float [C,H,W] tensor or a uint8 [H,W,C] image, got {tuple(im.shape)}")
            H, W = _image_size(im)
            if H < 1 or W < 1:
                raise ValueError(f"image {k} is empty: {tuple(im.shape)}")
            plans.append((H, W, len(_tiles.tile_axis(H, T, overlap)), len(_tiles.tile_axis(W, T, overlap))))
        out, i = [], 0
        while i < n:
            j, total = i + 1, plans[i][2] * plans[i][3]
            while j < n and total + plans[j][2] * plans[j][3] <= self.batch_size:
                total += plans[j][2] * plans[j][3]
                j += 1
            hm = None if heatmaps is None else [_as_tensor(h).to(dev, non_blocking=True) for h in heatmaps[i:j]]
            if points is not None:
                hm = self._click_maps(dev, points[i:j], [p[:2] for p in plans[i:j]])
            out += self._tile_group(dev, [im.to(dev, non_blocking=True) for im in images[i:j]], hm,
                                    None if labels is None else labels[i:j], plans[i:j])
            i = j
        return out

    def _tile_forward(self, dev, parts, c):
        """One forward over the tile ranges `parts` = [(image, heat-map or None, tile0, m)] -> y [sum m, C, T, T] fp32"""
        T, overlap = self._tile
        pad = _tiles.PADS[self.tiles.pad]
        total = sum(m for *_, m in parts)
        X = torch.empty((total, c, T, T), dtype=torch.float32, device=dev)
        Hm = torch.empty((total, 1, T, T), dtype=torch.float32, device=dev) if parts[0][1] is not None else None
        off = 0
        for im, hm, tile0, m in parts:
            _gather_tiles(im, X[off:off + m], T, overlap, pad, tile0, "image")
            if hm is not None:
                _gather_tiles(hm, Hm[off:off + m], T, overlap, pad, tile0, "heatmap")
            off += m
        return _forward(self.model, X, Hm, ("the model", "Segmenter"), self._scale(0))

    def _tile_group(self, dev, images, heatmaps, labels, plans):
        T, overlap = self._tile
        n, c = len(images), _channels(images[0])
        if heatmaps is not None:
            for k, hm in enumerate(heatmaps):
                if _image_size(hm) != plans[k][:2] or _channels(hm) != 1:
                    raise ValueError(f"heatmap {k} is {tuple(hm.shape)}, its image {plans[k][:2]}")
        counts_t = [ny * nx for _, _, ny, nx in plans]
        if n > 1 or counts_t[0] <= self.batch_size:
            y = self._tile_forward(dev, [(im, None if heatmaps is None else heatmaps[k], 0, counts_t[k])
                                         for k, im in enumerate(images)], c)
            offs = np.cumsum([0] + counts_t)
            Ys = [y[offs[k]:offs[k + 1]] for k in range(n)]
        else:       # one image in ceil(n / batch_size) forwards, its outputs collected into one contiguous buffer
            Y = None
            for t0 in range(0, counts_t[0], self.batch_size):
                m = min(self.batch_size, counts_t[0] - t0)
                y = self._tile_forward(dev, [(images[0], None if heatmaps is None else heatmaps[0], t0, m)], c)
                if Y is None:
                    Y = torch.empty((counts_t[0],) + tuple(y.shape[1:]), dtype=torch.float32, device=dev)
                elif y.shape[1] != Y.shape[1]:
                    raise ValueError(f"the model returned {int(y.shape[1])} classes, the forwards before it {int(Y.shape[1])}")
                Y[t0:t0 + m].copy_(y)
            Ys = [Y]
        C = int(Ys[0].shape[1])
        pal = self._palette_for(dev, C)
        kind, merge = _tta.KINDS[self.outputs[0]], _tta.MERGES[self.tiles.merge]
        window = _tiles.WINDOWS[self.tiles.window]
        s = ops._stream()
        metas = [{"original_size": (oh, ow), "tile_size": T, "overlap": overlap, "tiles": (ny, nx)} for oh, ow, ny, nx in plans]

        def launch(k, mask, outs, conf, scores):
            _lib.call("segk_predict_tiles", Ys[k].data_ptr(), C, kind, merge, window, *plans[k][:2], T, overlap, mask, *outs,
                      conf, scores, s)
        # the tile outputs are read by launches still in flight: the caching allocator keeps them valid in stream order
        return self._finish(dev, C, pal, metas, labels, launch, True, images)


def predict(model, images, heatmaps=None, labels=None, points=None, **kw):
    """One-shot convenience: Segmenter(model, **kw)(images, heatmaps, labels, points); clean= and tiles= are Segmenter
    keywords."""
    return Segmenter(model, **kw)(images, heatmaps=heatmaps, labels=labels, points=points)
