#!/usr/bin/env python3
"""COCO annotations -> one uint8 PNG label map per image, rasterised on the device (image_segmentation_amd.rasterize_batch,
DESIGN.md 3.18): polygons and RLE (uncompressed or the compressed string), annotation order = paint order.

    python tools/rasterize.py instances.json --categories 17=1,dog=2 --out labels/ [--fill 0] [--crowd-value 255] [--batch 32]
                                [--void-band W [--void-value 255]]

--categories maps a COCO category (its id, or its name from the file's "categories") to the class value painted; annotations
of other categories are skipped.  --void-band W gives the hard-edged polygon labels the ignore band Pascal VOC and the pet
trimaps have: every pixel within W (1..32, Euclidean) of a pixel with a different label becomes --void-value, on the device
(image_segmentation_amd.label_band).  The PNG of an image is named after its file_name (extension replaced by .png)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_categories(text, coco, ap):
    by_name = {c["name"]: c["id"] for c in coco.get("categories", [])}
    out = {}
    for part in text.split(","):
        key, sep, val = part.partition("=")
        if not sep or not val.strip().isdigit() or not 0 <= int(val) <= 255:
            ap.error(f"--categories: {part!r}: expected CATEGORY=CLASS with CLASS in 0..255")
        key = key.strip()
        if key in by_name:
            out[by_name[key]] = int(val)
        elif key.lstrip("-").isdigit():
            out[int(key)] = int(val)
        else:
            ap.error(f"--categories: {key!r} is neither a category id nor a name of the file's categories")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("coco", metavar="FILE.json")
    ap.add_argument("--categories", required=True, metavar="CATEGORY=CLASS,...")
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--fill", type=int, default=0, help="value of the pixels no shape covers (default 0)")
    ap.add_argument("--crowd-value", type=int, default=None, help="value of iscrowd annotations instead of their class")
    ap.add_argument("--batch", type=int, default=32, help="images per launch (default 32)")
    ap.add_argument("--void-band", type=int, default=None, metavar="W", help="void band of W pixels around every label change")
    ap.add_argument("--void-value", type=int, default=None, metavar="V", help="its value (default 255)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()
    if args.void_value is not None and args.void_band is None:
        ap.error("--void-value needs --void-band W")
    if args.void_band is not None and not 1 <= args.void_band <= 32:
        ap.error("--void-band: 1..32")
    void_value = 255 if args.void_value is None else args.void_value
    if not 0 <= void_value <= 255:
        ap.error("--void-value: 0..255")
    if args.batch < 1:
        ap.error("--batch: at least 1")
    coco = json.load(open(args.coco))
    cats = parse_categories(args.categories, coco, ap)

    import numpy as np                                      # noqa: F401
    from PIL import Image
    import image_segmentation_amd as seg
    per_image = {}
    for ann in coco.get("annotations", []):
        per_image.setdefault(ann["image_id"], []).append(ann)
    os.makedirs(args.out, exist_ok=True)
    images = coco["images"]
    for k in range(0, len(images), args.batch):
        chunk = images[k:k + args.batch]
        shapes = [seg.shapes_from_coco(per_image.get(im["id"], []), cats, crowd_value=args.crowd_value) for im in chunk]
        labs = seg.rasterize_batch(shapes, [(im["height"], im["width"]) for im in chunk], fill=args.fill, device=args.device)
        if args.void_band is not None:
            labs = [seg.label_band(lab, args.void_band, value=void_value) for lab in labs]
        for im, lab in zip(chunk, labs):
            name = os.path.splitext(os.path.basename(im["file_name"]))[0] + ".png"
            Image.fromarray(lab.cpu().numpy(), "L").save(os.path.join(args.out, name))
    print(f"{len(images)} label maps -> {args.out}")


if __name__ == "__main__":
    main()
