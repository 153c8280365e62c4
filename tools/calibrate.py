#!/usr/bin/env python3
"""Confidence calibration of a trained checkpoint over image files: a thin shell over image_segmentation_amd.fit_temperature
and reliability.  Every image IMAGES/<name>.* is paired with LABELS/<name>.png, an 8-bit map of class ids
(values outside [0, classes) are not scored).  Writes JSON: the temperature grid with the mean NLL and ECE of every point, the
fitted temperature, NLL and ECE before (T = 1) and after, and the reliability bins overall and per predicted class, before and
after; plotting is left to the reader.
Usage: python tools/calibrate.py --model {unet,autoencoder} --checkpoint F --classes 4 --ignore-index 3 --target-size 224
       --images DIR --labels DIR --out calibration.json [--bins 15] [--temps T,T,...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", choices=["unet", "autoencoder"], default="unet")
    ap.add_argument("--checkpoint", required=True, help="{'model_state_dict': ...}, {'state_dict': ...} or a bare state dict")
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--ignore-index", type=int, default=None, help="label value left out of every count")
    ap.add_argument("--target-size", type=int, default=224, help="side of the square network input")
    ap.add_argument("--interpolation", choices=["bilinear", "nearest"], default="bilinear")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--bins", type=int, default=15, help="reliability bins in the report")
    ap.add_argument("--temps", default=None, metavar="T,T", help="the temperature grid (default: 2^(-2 + j/4), j = 0..16)")
    ap.add_argument("--images", required=True, help="folder of image files")
    ap.add_argument("--labels", required=True, help="folder of <name>.png class-id maps")
    ap.add_argument("--out", required=True, help="JSON file to write")
    args = ap.parse_args()
    try:
        temps = [float(t) for t in args.temps.split(",")] if args.temps else None
    except ValueError:
        ap.error("--temps takes comma-separated numbers")

    import numpy as np
    from PIL import Image
    import image_segmentation_amd as seg

    names = sorted(f for f in os.listdir(args.images) if not f.startswith("."))
    if not names:
        ap.error(f"no files in {args.images}")
    images, labels = [], []
    for f in names:
        lab = os.path.join(args.labels, os.path.splitext(f)[0] + ".png")
        if not os.path.exists(lab):
            ap.error(f"{f} has no label {lab}")
        images.append(np.asarray(Image.open(os.path.join(args.images, f)).convert("RGB")))
        labels.append(np.asarray(Image.open(lab).convert("L")).astype(np.int64))
    model = seg.unet(3, args.classes) if args.model == "unet" else seg.SegmentationAutoencoder(3, num_classes=args.classes)
    model = seg.load_checkpoint(model, args.checkpoint).cuda()
    kw = dict(target_size=args.target_size, interpolation=args.interpolation, batch_size=args.batch_size)
    try:
        fit = seg.fit_temperature(model, images, labels, temps=temps, ignore_index=args.ignore_index, **kw)
    except ValueError as e:
        ap.error(str(e))
    report = {"images": len(images), "classes": args.classes, "ignore_index": args.ignore_index, "fit": fit.to_json()}
    for key, T in (("before", None), ("after", fit.temperature)):
        if key == "after" and T is None:
            break
        preds = seg.Segmenter(model, palette=None, return_scores=True, temperature=T, **kw)(images)
        for p in preds:
            p.scores = None
        report[key] = seg.reliability(preds, labels, args.classes, ignore_index=args.ignore_index).to_json(args.bins)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    fmt = lambda v: "none" if v is None else f"{v:.4f}"       # noqa: E731
    print(f"T* = {fmt(fit.temperature)}{' (at the end of the grid)' if fit.at_grid_end else ''} over {fit.pixels} pixels: "
          f"NLL {fmt(fit.nll_at_1)} -> {fmt(fit.nll_best)}, ECE {fmt(fit.ece_at_1)} -> {fmt(fit.ece_best)}")


if __name__ == "__main__":
    main()
