#!/usr/bin/env python3
"""Object-level evaluation of a trained checkpoint on a folder of images with label maps: a thin shell over
image_segmentation_amd.Segmenter and PanopticQuality.  For every image IMAGES/<name>.* the label map is
LABELS/<name>.png (8-bit class indices at the image's size; a value equal to --ignore-index or above 7 is void).  Writes one JSON
file: Panoptic Quality, segmentation and recognition quality, object F1 at IoU 0.50 .. 0.95 and TP / FP / FN per class, their
means, and the number of images whose object or pair count exceeded the capacities (they add nothing).
Usage: python tools/evaluate_objects.py --checkpoint F --images DIR --labels DIR --classes 4 --things 1,2 --stuff 0
       --ignore-index 3 --out FILE.json
--min-area N / --keep-largest [CLASSES] / --connectivity {4,8} clean every predicted mask on the device first,
so two runs with and without them measure what the clean-up is worth in objects found, missed and invented."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXT = (".png", ".jpg", ".jpeg", ".bmp")


def classes_of(ap, text, what):
    try:
        return tuple(int(c) for c in text.split(",") if c != "")
    except ValueError:
        ap.error(f"{what} takes comma-separated class numbers")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", choices=["unet", "autoencoder"], default="unet")
    ap.add_argument("--checkpoint", required=True, help="{'model_state_dict': ...}, {'state_dict': ...} or a bare state dict")
    ap.add_argument("--images", required=True, metavar="DIR")
    ap.add_argument("--labels", required=True, metavar="DIR")
    ap.add_argument("--out", required=True, metavar="FILE.json")
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--things", default=None, metavar="CLASSES", help="classes whose connected components are objects "
                    "(default: every class that is neither stuff nor --ignore-index)")
    ap.add_argument("--stuff", default="", metavar="CLASSES", help="classes that are one segment each")
    ap.add_argument("--ignore-index", type=int, default=None)
    ap.add_argument("--size", type=int, default=224, help="side of the square network input")
    ap.add_argument("--interpolation", choices=["bilinear", "nearest"], default="bilinear")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--min-area", type=int, default=0, metavar="N", help="remove predicted components of fewer than N pixels")
    ap.add_argument("--keep-largest", nargs="?", const="all", default=None, metavar="CLASSES",
                    help="keep only the largest predicted component of each class (or of the comma-separated CLASSES)")
    ap.add_argument("--connectivity", type=int, choices=[4, 8], default=4)
    ap.add_argument("--max-components", type=int, default=1024)
    ap.add_argument("--max-pairs", type=int, default=None)
    args = ap.parse_args()
    things = None if args.things is None else classes_of(ap, args.things, "--things")
    stuff = classes_of(ap, args.stuff, "--stuff")
    keep = False
    if args.keep_largest is not None:
        keep = True if args.keep_largest == "all" else classes_of(ap, args.keep_largest, "--keep-largest")
    clean = None
    if args.min_area > 0 or keep is not False:
        clean = dict(connectivity=args.connectivity, min_area=args.min_area, keep_largest=keep, max_components=args.max_components)

    import json
    import numpy as np
    import torch
    from PIL import Image
    import image_segmentation_amd as seg
    try:
        pq = seg.PanopticQuality(args.classes, things, stuff, args.ignore_index, connectivity=args.connectivity,
                                 max_components=args.max_components, max_pairs=args.max_pairs)
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
                              clean=clean)
    for i in range(0, len(pairs), args.batch_size):
        batch = pairs[i:i + args.batch_size]
        preds = segmenter([np.asarray(Image.open(p).convert("RGB")) for p, _ in batch])
        for pred, (_, l) in zip(preds, batch):                     # no sync: the counts stay on the device until compute()
            pq.update(pred, torch.from_numpy(np.asarray(Image.open(l).convert("L"))).to(pred.mask.device))
    out = pq.compute()
    out.update(things=list(pq.things), stuff=list(pq.stuff), ignore_index=args.ignore_index, connectivity=args.connectivity,
               min_area=args.min_area, keep_largest=args.keep_largest)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    show = lambda v: "-" if v is None else f"{v:.4f}"
    print(f"{out['images']} images ({out['incomplete_images']} incomplete)  PQ {show(out['mean_pq'])}  SQ {show(out['mean_sq'])}  "
          f"RQ {show(out['mean_rq'])}  F1@0.5 {show(out['mean_f1'][0])}")


if __name__ == "__main__":
    main()
