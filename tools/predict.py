#!/usr/bin/env python3
"""Segment image files with a trained checkpoint: a thin shell over image_segmentation_amd.Segmenter (the prediction path
of the reference's demo service, segmentation_webapp/app.py:250-326, without the web part).  For every IMG it writes
DIR/<name>_mask.png (8-bit class indices) and, while the palette covers the classes, DIR/<name>_color.png (RGB).
Usage: python tools/predict.py --model {unet,autoencoder} --checkpoint F --classes 4 --size 224 --out DIR IMG...
(models that need the hub to construct -- ClipUNet, PromptModel -- are driven from the library: Segmenter(model))"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", choices=["unet", "autoencoder"], default="unet")
    ap.add_argument("--checkpoint", required=True, help="{'model_state_dict': ...}, {'state_dict': ...} or a bare state dict")
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--size", type=int, default=224, help="side of the square network input")
    ap.add_argument("--interpolation", choices=["bilinear", "nearest"], default="bilinear")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("images", nargs="+", metavar="IMG")
    args = ap.parse_args()

    import numpy as np
    from PIL import Image
    import image_segmentation_amd as seg

    if args.model == "unet":
        model = seg.unet(3, args.classes)
    else:
        model = seg.SegmentationAutoencoder(3, num_classes=args.classes)
    model = seg.load_checkpoint(model, args.checkpoint).cuda()
    palette = seg.COLOR_MAP if args.classes <= len(seg.COLOR_MAP) else None
    segmenter = seg.Segmenter(model, target_size=args.size, interpolation=args.interpolation, palette=palette,
                              batch_size=args.batch_size)
    os.makedirs(args.out, exist_ok=True)
    names = seg.CLASS_NAMES["standard"]
    for i in range(0, len(args.images), args.batch_size):
        paths = args.images[i:i + args.batch_size]
        preds = segmenter([np.asarray(Image.open(p).convert("RGB")) for p in paths])
        for p, pred in zip(paths, preds):
            stem = os.path.join(args.out, os.path.splitext(os.path.basename(p))[0])
            Image.fromarray(pred.mask.cpu().numpy(), "L").save(stem + "_mask.png")
            if pred.color is not None:
                Image.fromarray(pred.color.cpu().numpy(), "RGB").save(stem + "_color.png")
            counts = pred.counts.tolist()
            print(p, " ".join(f"{names.get(k, k)}={c}" for k, c in enumerate(counts)))


if __name__ == "__main__":
    main()
