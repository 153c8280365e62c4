#!/usr/bin/env python3
"""Segment image files with a trained checkpoint: a thin shell over image_segmentation_amd.Segmenter (the prediction path
of the reference's demo service, segmentation_webapp/app.py:250-326, without the web part).  For every IMG it writes
DIR/<name>_mask.png (8-bit class indices) and, while the palette covers the classes, DIR/<name>_color.png (RGB).
Usage: python tools/predict.py --model {unet,autoencoder,prompt} --checkpoint F --classes 4 --size 224 --out DIR IMG...
--model prompt is the prompt model (a ViT-B/16 ClipUNet built from its configuration, no hub access: every weight comes
from the checkpoint of the whole PromptModel) and needs --point Y,X (repeatable; the clicks apply to every image).  A ClipUNet
alone is driven from the library: Segmenter(model).
--min-area N / --keep-largest [CLASSES] / --connectivity {4,8} clean every mask on the device first (small and
non-largest components take their neighbours' class); --boxes FILE.json writes, per image, the class, area and box
(y0, x0, y1, x1; exclusive ends) of the components that stayed.
--tta h,v,hv adds flipped views to the plain one, --sizes 224,256 several target sizes, a repeated --checkpoint several models
of the same kind (an ensemble); the views are merged on the device (--merge prob averages probabilities,
--merge logit logits) and --confidence DIR writes DIR/<name>_confidence.png (8-bit, 255 = certain).  The prompt model's
ViT takes 224 x 224 inputs only.
--tile N segments every image at its own resolution in N x N tiles that overlap by --tile-overlap M pixels (default N / 4)
and blends the tiles' outputs on the device (--tile-window triangle|flat weighs a tile's pixels, --tile-pad
reflect|zero fills a tile beyond an image smaller than itself, --merge as above); --batch-size then counts tiles per forward.
It does not combine with --tta, --sizes or several --checkpoint; --confidence works with it.
--temperature T divides every model's logits by T before the prediction kernels run (tools/calibrate.py fits
it): the confidence maps become the calibrated ones.  Not for --model prompt, whose outputs are probabilities.
--coco FILE.json writes ONE COCO-style file for all inputs (images, annotations, categories): every connected component of a
final (cleaned) mask whose class has a category becomes an annotation with bbox, area and a polygon list -- or, when it has a
hole, its uncompressed RLE -- built on the device.  --coco-categories 1=cat,2=dog maps classes to category
ids (the class number) and names; the default is every class but 0 under its class name.
--open R / --close R / --fill-holes shape every mask on the device before the clean-up, in that order (spurs and
bridges thinner than the element go, cracks close, holes fill); --morph-classes 1,2 names the classes they act on (default:
every class but 0, closing and filling one class at a time), --morph-shape {disk,square,diamond} the element.
--snap STEP snaps every mask to the SLIC superpixels of its image (grid spacing STEP, 4..64) before all of that (DESIGN.md
3.24): a superpixel whose winning class holds at least --snap-share F of its votes (default 0.5) takes that class;
--snap-compactness M (1..255, default 20) trades colour against squareness, --snap-weighted lets a vote weigh the confidence
map (merged views or --tile only)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", choices=["unet", "autoencoder", "prompt"], default="unet")
    ap.add_argument("--point", action="append", default=[], metavar="Y,X",
                    help="a click in image pixels for --model prompt; repeat for several (the heat-map is the maximum of "
                         "their Gaussians); applies to every image")
    ap.add_argument("--sigma", type=float, default=3.0, help="spread of the click heat-map, as in training")
    ap.add_argument("--checkpoint", required=True, action="append",
                    help="{'model_state_dict': ...}, {'state_dict': ...} or a bare state dict; repeat for an ensemble")
    ap.add_argument("--tta", default=None, metavar="FLIPS", help="comma-separated flips added to the plain view: h, v, hv")
    ap.add_argument("--sizes", default=None, metavar="T,T", help="comma-separated target sizes (default: --size alone)")
    ap.add_argument("--merge", choices=["prob", "logit"], default="prob", help="how the views are merged")
    ap.add_argument("--confidence", metavar="DIR", help="write the merged views' confidence maps as 8-bit PNGs into DIR")
    ap.add_argument("--tile", type=int, default=None, metavar="N", help="tiled full-resolution prediction with N x N tiles")
    ap.add_argument("--tile-overlap", type=int, default=None, metavar="M", help="pixels two neighbouring tiles share (default N / 4)")
    ap.add_argument("--tile-window", choices=["flat", "triangle"], default="triangle", help="blend weight of a tile's pixels")
    ap.add_argument("--tile-pad", choices=["reflect", "zero"], default="reflect", help="a tile's content beyond a smaller image")
    ap.add_argument("--temperature", type=float, default=None, metavar="T", help="divide the logits by T (calibrated confidence)")
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--size", type=int, default=224, help="side of the square network input")
    ap.add_argument("--interpolation", choices=["bilinear", "nearest"], default="bilinear")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--min-area", type=int, default=0, metavar="N", help="remove components of fewer than N pixels")
    ap.add_argument("--keep-largest", nargs="?", const="all", default=None, metavar="CLASSES",
                    help="keep only the largest component of each class (or of the comma-separated CLASSES)")
    ap.add_argument("--connectivity", type=int, choices=[4, 8], default=4)
    ap.add_argument("--max-components", type=int, default=1024, help="components reported per image in --boxes")
    ap.add_argument("--boxes", metavar="FILE.json", help="write the kept components' class, area and box per image")
    ap.add_argument("--coco", metavar="FILE.json", help="write the components of all masks as COCO annotations (polygons / RLE)")
    ap.add_argument("--coco-categories", default=None, metavar="C=NAME,...", help="classes that become categories, with their names")
    ap.add_argument("--open", type=int, default=None, metavar="R", help="open the classes with radius R (1..32)")
    ap.add_argument("--close", type=int, default=None, metavar="R", help="close every class with radius R (1..32)")
    ap.add_argument("--fill-holes", action="store_true", help="fill the holes of every class")
    ap.add_argument("--morph-classes", default=None, metavar="CLASSES", help="comma-separated classes (default: all but 0)")
    ap.add_argument("--morph-shape", choices=["disk", "square", "diamond"], default="disk")
    ap.add_argument("--snap", type=int, default=None, metavar="STEP", help="snap the mask to SLIC superpixels of this spacing (4..64)")
    ap.add_argument("--snap-share", type=float, default=0.5, metavar="F", help="share of a superpixel's votes its winner needs")
    ap.add_argument("--snap-compactness", type=int, default=20, metavar="M", help="1..255: larger keeps superpixels square")
    ap.add_argument("--snap-weighted", action="store_true", help="a vote weighs the confidence map (merged views or --tile)")
    ap.add_argument("images", nargs="+", metavar="IMG")
    args = ap.parse_args()
    try:
        clicks = [tuple(int(v) for v in p.split(",")) for p in args.point]
        if any(len(c) != 2 for c in clicks):
            raise ValueError
    except ValueError:
        ap.error("--point takes Y,X (two integers)")
    if (args.model == "prompt") != bool(clicks):
        ap.error("--model prompt needs --point Y,X, and --point needs --model prompt")

    tiles = None
    if args.tile is not None:
        if args.tta or args.sizes or len(args.checkpoint) > 1:
            ap.error("--tile does not combine with --tta, --sizes or several --checkpoint")
        tiles = dict(size=args.tile, overlap=args.tile_overlap, window=args.tile_window, pad=args.tile_pad, merge=args.merge)
    elif args.tile_overlap is not None or args.tile_window != "triangle" or args.tile_pad != "reflect":
        ap.error("--tile-overlap, --tile-window and --tile-pad need --tile N")

    tta = None
    if tiles is not None:
        pass
    elif args.tta or args.sizes or args.confidence or len(args.checkpoint) > 1 or args.merge != "prob":
        flips = ("",) + tuple(f for f in (args.tta or "").split(",") if f)
        try:
            sizes = tuple(int(t) for t in args.sizes.split(",")) if args.sizes else None
        except ValueError:
            ap.error("--sizes takes comma-separated integers")
        tta = dict(flips=flips, sizes=sizes, merge=args.merge)

    keep = False
    if args.keep_largest is not None:
        try:
            keep = True if args.keep_largest == "all" else tuple(int(c) for c in args.keep_largest.split(","))
        except ValueError:
            ap.error("--keep-largest takes comma-separated class numbers")
    clean = None
    if args.min_area > 0 or keep is not False or args.boxes:
        clean = dict(connectivity=args.connectivity, min_area=args.min_area, keep_largest=keep, max_components=args.max_components)

    morph = None
    if args.open is not None or args.close is not None or args.fill_holes:
        try:
            mcls = tuple(int(c) for c in args.morph_classes.split(",")) if args.morph_classes else tuple(range(1, args.classes))
        except ValueError:
            ap.error("--morph-classes takes comma-separated class numbers")
        if not mcls or any(not 0 <= c < args.classes for c in mcls):
            ap.error(f"--morph-classes: classes in 0..{args.classes - 1}")
        other = next((c for c in range(args.classes) if c not in mcls), None)
        if args.open is not None and other is None:
            ap.error("--open needs a class outside --morph-classes for the opened pixels")
        morph = []
        if args.open is not None:                           # the set as a whole: every pixel keeps its own class
            morph.append(dict(op="open", classes=mcls, radius=args.open, fill=other, shape=args.morph_shape))
        if args.close is not None:
            morph += [dict(op="close", classes=(c,), radius=args.close, shape=args.morph_shape) for c in mcls]
        if args.fill_holes:
            morph += [dict(op="fill_holes", classes=(c,), connectivity=args.connectivity) for c in mcls]
    elif args.morph_classes is not None or args.morph_shape != "disk":
        ap.error("--morph-classes and --morph-shape need --open, --close or --fill-holes")

    snap = None
    if args.snap is not None:
        snap = dict(step=args.snap, compactness=args.snap_compactness, min_share=args.snap_share, weighted=args.snap_weighted)
    elif args.snap_weighted or args.snap_share != 0.5 or args.snap_compactness != 20:
        ap.error("--snap-share, --snap-compactness and --snap-weighted need --snap STEP")

    categories = None
    if args.coco_categories is not None:
        if not args.coco:
            ap.error("--coco-categories needs --coco FILE")
        try:
            categories = {int(c): n for c, n in (item.split("=", 1) for item in args.coco_categories.split(","))}
        except ValueError:
            ap.error("--coco-categories takes CLASS=NAME pairs separated by commas")
        if not categories or any(not 0 <= c < args.classes or not n for c, n in categories.items()):
            ap.error(f"--coco-categories: classes in 0..{args.classes - 1}, each with a name")
    vectors = dict(connectivity=args.connectivity, max_components=args.max_components) if args.coco else None

    import json
    import numpy as np
    from PIL import Image
    import image_segmentation_amd as seg

    def build():
        if args.model == "unet":
            return seg.unet(3, args.classes)
        if args.model == "prompt":
            if args.classes != 4:
                ap.error("the prompt model has 4 classes")
            return seg.PromptModel(clip=seg.ClipUNet(num_classes=4, encoder=seg.ClipViTEncoder.from_config()))
        return seg.SegmentationAutoencoder(3, num_classes=args.classes)
    models = [seg.load_checkpoint(build(), path).cuda() for path in args.checkpoint]
    palette = seg.COLOR_MAP if args.classes <= len(seg.COLOR_MAP) else None
    try:
        segmenter = seg.Segmenter(models if tta is not None else models[0], target_size=args.size, interpolation=args.interpolation,
                                  palette=palette, batch_size=args.batch_size, sigma=args.sigma, clean=clean, tta=tta, tiles=tiles,
                                  temperature=args.temperature, vectors=vectors, morph=morph, snap=snap)
    except ValueError as e:
        ap.error(str(e))
    if args.confidence:
        os.makedirs(args.confidence, exist_ok=True)
    boxes = {}
    os.makedirs(args.out, exist_ok=True)
    names = seg.CLASS_NAMES["prompt_model" if clicks else "standard"]
    if categories is None:
        categories = {c: str(names.get(c, c)) for c in range(1, args.classes)}
    coco = {"images": [], "annotations": [], "categories": [{"id": c, "name": n} for c, n in sorted(categories.items())]}
    for i in range(0, len(args.images), args.batch_size):
        paths = args.images[i:i + args.batch_size]
        preds = segmenter([np.asarray(Image.open(p).convert("RGB")) for p in paths],
                          points=[clicks] * len(paths) if clicks else None)
        for p, pred in zip(paths, preds):
            stem = os.path.join(args.out, os.path.splitext(os.path.basename(p))[0])
            Image.fromarray(pred.mask.cpu().numpy(), "L").save(stem + "_mask.png")
            if pred.color is not None:
                Image.fromarray(pred.color.cpu().numpy(), "RGB").save(stem + "_color.png")
            if args.confidence:
                name = os.path.splitext(os.path.basename(p))[0] + "_confidence.png"
                Image.fromarray(pred.confidence.cpu().numpy(), "L").save(os.path.join(args.confidence, name))
            counts = pred.counts.tolist()
            print(p, " ".join(f"{names.get(k, k)}={c}" for k, c in enumerate(counts)))
            if args.coco:
                vec = pred.vectors
                if not vec.complete:                 # more boundary than the default capacities hold: again, sized by the counts
                    edges, k = int(vec.totals[1].item()), int(vec.num.item())
                    vec = seg.vectorize(pred.mask, connectivity=args.connectivity, max_components=max(k, 1), max_edges=max(edges, 1))
                image_id = len(coco["images"]) + 1
                H, W = vec.size
                coco["images"].append({"id": image_id, "file_name": os.path.basename(p), "height": H, "width": W})
                coco["annotations"] += vec.to_coco(image_id, {c: c for c in categories}, first_id=len(coco["annotations"]) + 1)
            if args.boxes:
                c = pred.components
                k = min(c.n, args.max_components)
                rows = zip(c.kept[:k].tolist(), c.cls[:k].tolist(), c.area[:k].tolist(), c.box[:k].tolist())
                boxes[p] = {"components": c.n, "reported": k,
                            "kept": [{"class": cl, "name": names.get(cl, str(cl)), "area": a, "box": b} for kp, cl, a, b in rows if kp]}
    if args.boxes:
        with open(args.boxes, "w") as f:
            json.dump(boxes, f, indent=1)
    if args.coco:
        with open(args.coco, "w") as f:
            json.dump(coco, f)


if __name__ == "__main__":
    main()
