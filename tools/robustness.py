#!/usr/bin/env python3
"""Robustness sweep of a trained checkpoint over image files: a thin shell over image_segmentation_amd.robustness_sweep (the
experiment of the reference's report section 4.1 / figure 6: eight perturbation types at ten severity levels).  Every image
IMAGES/<name>.* is paired with LABELS/<name>.png, an 8-bit map of class ids (values outside [0, classes) are not scored).
Writes the result dict as JSON; plotting is left to the reader.
Usage: python tools/robustness.py --model {unet,autoencoder} --checkpoint F --classes 4 --ignore-index 3 --target-size 224
       --images DIR --labels DIR --out sweep.json [--only kind[,kind]] [--seed N]"""
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
    ap.add_argument("--ignore-index", type=int, default=None, help="class left out of the macro means")
    ap.add_argument("--target-size", type=int, default=224, help="side of the square network input")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--images", required=True, help="folder of image files")
    ap.add_argument("--labels", required=True, help="folder of <name>.png class-id maps")
    ap.add_argument("--only", default="", metavar="KIND[,KIND]", help="a subset of the eight perturbations")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="JSON file to write")
    args = ap.parse_args()

    import numpy as np
    from PIL import Image
    import image_segmentation_amd as seg

    kinds = tuple(k for k in args.only.split(",") if k) or seg.PERTURBATIONS
    for k in kinds:
        if k not in seg.PERTURBATIONS:
            ap.error(f"--only: unknown perturbation {k!r} (one of {', '.join(seg.PERTURBATIONS)})")
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
    res = seg.robustness_sweep(model, images, labels, args.classes, ignore_index=args.ignore_index, perturbations=kinds,
                               seed=args.seed, target_size=args.target_size, batch_size=args.batch_size, palette=None)
    with open(args.out, "w") as f:
        json.dump({"images": len(images), "seed": args.seed, "classes": args.classes, "ignore_index": args.ignore_index,
                   "sweep": res}, f, indent=1)
    for k in kinds:
        print(k, " ".join("nan" if d is None else f"{d:.4f}" for d in res[k]["dice"]))


if __name__ == "__main__":
    main()
