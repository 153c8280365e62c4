#!/usr/bin/env python3
"""Boundary quality of a trained checkpoint on a folder of images with label maps: a thin shell over
image_segmentation_amd.Segmenter and BoundaryQuality.  For every image IMAGES/<name>.* the label map is
LABELS/<name>.png (8-bit class indices at the image's size; a value equal to --ignore-index or >= --classes is void).  Writes one
JSON file: Boundary IoU, band IoU and accuracy, contour precision / recall / F at the --tolerances, the mean per-image HD95 and the
images whose HD95 lies past --max-distance, per class, and their means.
Usage: python tools/evaluate_boundaries.py --checkpoint F --images DIR --labels DIR --classes 4 --ignore-index 3 --out FILE.json
--open R / --close R / --min-area N shape every predicted mask on the device first (--morph-classes names
the classes they act on, default every class but 0), so two runs with and without them tell what the post-process does to the
contour.  --width W fixes the band's half-width (default: 2 % of each image's diagonal, the published rule, at most 32).
--snap STEP / --snap-share F / --snap-compactness M / --snap-weighted snap every predicted mask to the SLIC superpixels of its
image before that (the flags of tools/predict.py): two runs tell what snapping does to Boundary IoU and HD95.
--snap-weighted runs the single view through the merged route, which writes the confidence map the votes weigh."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXT = (".png", ".jpg", ".jpeg", ".bmp")


def ints_of(ap, text, what):
    try:
        return tuple(int(c) for c in text.split(",") if c != "")
    except ValueError:
        ap.error(f"{what} takes comma-separated integers")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", choices=["unet", "autoencoder"], default="unet")
    ap.add_argument("--checkpoint", required=True, help="{'model_state_dict': ...}, {'state_dict': ...} or a bare state dict")
    ap.add_argument("--images", required=True, metavar="DIR")
    ap.add_argument("--labels", required=True, metavar="DIR")
    ap.add_argument("--out", required=True, metavar="FILE.json")
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--ignore-index", type=int, default=None)
    ap.add_argument("--size", type=int, default=224, help="side of the square network input")
    ap.add_argument("--interpolation", choices=["bilinear", "nearest"], default="bilinear")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--width", type=int, default=None, metavar="W", help="band half-width in pixels (default: 2 %% of the diagonal)")
    ap.add_argument("--max-distance", type=int, default=32, metavar="R", help="cap of the contour distances (1..32)")
    ap.add_argument("--tolerances", default="1,2,3", metavar="PIXELS")
    ap.add_argument("--shape", choices=["square", "diamond", "disk"], default="square", help="metric of the band distance")
    ap.add_argument("--no-image-border", action="store_true", help="the image border makes no band")
    ap.add_argument("--open", type=int, default=0, metavar="R", help="open the predicted mask with radius R first")
    ap.add_argument("--close", type=int, default=0, metavar="R", help="close it with radius R (after --open)")
    ap.add_argument("--min-area", type=int, default=0, metavar="N", help="remove predicted components of fewer than N pixels")
    ap.add_argument("--morph-classes", default=None, metavar="CLASSES", help="comma-separated classes (default: all but 0)")
    ap.add_argument("--morph-shape", choices=["disk", "square", "diamond"], default="disk")
    ap.add_argument("--connectivity", type=int, choices=[4, 8], default=4)
    ap.add_argument("--snap", type=int, default=None, metavar="STEP", help="snap the mask to SLIC superpixels of this spacing (4..64)")
    ap.add_argument("--snap-share", type=float, default=0.5, metavar="F", help="share of a superpixel's votes its winner needs")
    ap.add_argument("--snap-compactness", type=int, default=20, metavar="M", help="1..255: larger keeps superpixels square")
    ap.add_argument("--snap-weighted", action="store_true", help="a vote weighs the confidence map")
    args = ap.parse_args()
    snap = None
    if args.snap is not None:
        snap = dict(step=args.snap, compactness=args.snap_compactness, min_share=args.snap_share, weighted=args.snap_weighted)
    elif args.snap_weighted or args.snap_share != 0.5 or args.snap_compactness != 20:
        ap.error("--snap-share, --snap-compactness and --snap-weighted need --snap STEP")
    morph = None
    if args.open or args.close:
        mcls = ints_of(ap, args.morph_classes, "--morph-classes") if args.morph_classes else tuple(range(1, args.classes))
        if not mcls or any(not 0 <= c < args.classes for c in mcls):
            ap.error(f"--morph-classes: classes in 0..{args.classes - 1}")
        other = next((c for c in range(args.classes) if c not in mcls), None)
        if args.open and other is None:
            ap.error("--open needs a class outside --morph-classes for the opened pixels")
        morph = []
        if args.open:
            morph.append(dict(op="open", classes=mcls, radius=args.open, fill=other, shape=args.morph_shape))
        if args.close:
            morph += [dict(op="close", classes=(c,), radius=args.close, shape=args.morph_shape) for c in mcls]
    clean = dict(connectivity=args.connectivity, min_area=args.min_area) if args.min_area > 0 else None

    import json
    import numpy as np
    import torch
    from PIL import Image
    import image_segmentation_amd as seg
    try:
        bq = seg.BoundaryQuality(args.classes, args.ignore_index, args.width, args.max_distance, ints_of(ap, args.tolerances, "--tolerances"),
                                 args.shape, not args.no_image_border)
        segmenter_morph = seg.morph.as_morph(morph) if morph is not None else None
        snap = seg.Snap(**snap) if snap is not None else None
    except ValueError as e:
        ap.error(str(e))
    names = sorted(f for f in os.listdir(args.images) if f.lower().endswith(EXT))
    pairs = [(os.path.join(args.images, f), os.path.join(args.labels, os.path.splitext(f)[0] + ".png")) for f in names]
    missing = [l for _, l in pairs if not os.path.exists(l)]
    if not pairs or missing:
        ap.error(f"no images in {args.images}" if not pairs else f"{len(missing)} label maps are missing, first {missing[0]}")
    model = seg.unet(3, args.classes) if args.model == "unet" else seg.SegmentationAutoencoder(3, num_classes=args.classes)
    model = seg.load_checkpoint(model, args.checkpoint).cuda()
    segmenter = seg.Segmenter(model, target_size=args.size, interpolation=args.interpolation, palette=None, batch_size=args.batch_size,
                              clean=clean, morph=segmenter_morph, snap=snap,
                              tta=dict(flips=("",)) if snap is not None and snap.weighted else None)
    for i in range(0, len(pairs), args.batch_size):
        batch = pairs[i:i + args.batch_size]
        preds = segmenter([np.asarray(Image.open(p).convert("RGB")) for p, _ in batch])
        for pred, (_, l) in zip(preds, batch):                     # no sync: the counts stay on the device until compute()
            try:
                bq.update(pred, torch.from_numpy(np.asarray(Image.open(l).convert("L"))).to(pred.mask.device))
            except ValueError as e:                                # a label of another size, a diagonal past the widest band
                ap.error(f"{l}: {e}")
    out = bq.compute()
    out.update(ignore_index=args.ignore_index, width=args.width, shape=args.shape, image_border=not args.no_image_border,
               open=args.open, close=args.close, min_area=args.min_area, snap=args.snap,
               snap_share=args.snap_share if args.snap is not None else None,
               snap_compactness=args.snap_compactness if args.snap is not None else None, snap_weighted=args.snap_weighted)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    show = lambda v: "-" if v is None else f"{v:.4f}"
    first = out["tolerances"][0] if out["tolerances"] else None
    print(f"{out['images']} images  Boundary IoU {show(out['mean_boundary_iou'])}  band IoU {show(out['mean_band_iou'])}  "
          f"F@{first} {show(out['mean_contour_f'].get(first))}  HD95 {show(out['mean_hd95'])} ({sum(out['hd95_capped'])} capped)")


if __name__ == "__main__":
    main()
