#!/usr/bin/env python3
"""Write an `astrain`-style folder (color/*.jpg|png, label/*.png) from a folder of images and labels: a thin shell over
image_segmentation_amd.augment -- what the reference's utils/augmentation.ipynb does offline with imgaug, here on the device.

    python tools/augment.py --color Train/color --label Train/label --out astrain --copies 8 --pairs 126 --seed 0

Every source image is written `--copies` times, each copy with one op drawn from the eight augmenters (pad to square, resize
to --size); `--pairs` adds that many merged pairs (cell 17: two images of the same orientation side by side).  Labels may be
one-channel class / trimap files or the colour files of the reference (black / red / green / white); the output labels are
one-channel class maps.  Decoding and encoding go through PIL on the host; everything between runs on the GPU."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(path, label):
    from PIL import Image
    im = Image.open(path)
    if label and im.mode in ("L", "P", "1", "I"):
        return np.asarray(im.convert("L") if im.mode != "P" else im, dtype=np.uint8)
    return np.asarray(im.convert("RGB"), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--color", required=True, help="folder of source images")
    ap.add_argument("--label", required=True, help="folder of label files (<stem>.png)")
    ap.add_argument("--out", required=True, help="output folder (color/ and label/ are created in it)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--copies", type=int, default=8, help="augmented copies per source image")
    ap.add_argument("--pairs", type=int, default=0, help="merged pairs to add")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--format", choices=("jpg", "png"), default="jpg", help="file type of the colour outputs")
    args = ap.parse_args()
    import torch
    from PIL import Image
    from image_segmentation_amd import augment as A

    stems = sorted(os.path.splitext(f)[0] for f in os.listdir(args.color) if f.lower().endswith((".jpg", ".jpeg", ".png"))
                   and os.path.exists(os.path.join(args.label, os.path.splitext(f)[0] + ".png")))
    if not stems:
        raise SystemExit("no image with a label file was found")
    names = {os.path.splitext(f)[0]: f for f in os.listdir(args.color)}
    for sub in ("color", "label"):
        os.makedirs(os.path.join(args.out, sub), exist_ok=True)

    def save(X8, y, out_names):
        X8, y = X8.cpu().numpy(), y.cpu().numpy()
        for k, n in enumerate(out_names):
            Image.fromarray(X8[k], "RGB").save(os.path.join(args.out, "color", f"{n}.{args.format}"))
            Image.fromarray(y[k, 0].astype(np.uint8), "L").save(os.path.join(args.out, "label", f"{n}.png"))

    def fetch(batch):
        imgs = [torch.from_numpy(load(os.path.join(args.color, names[s]), False)).cuda() for s in batch]
        labs = [torch.from_numpy(load(os.path.join(args.label, s + ".png"), True)).cuda() for s in batch]
        return imgs, labs

    aug = A.Augmenter(target_size=args.size, seed=args.seed)
    written = 0
    for i in range(0, len(stems), args.batch):
        batch = stems[i:i + args.batch]
        imgs, labs = fetch(batch)
        for c in range(args.copies):
            plans = aug.plan([tuple(t.shape[:2]) for t in imgs])
            X8, y = aug.apply(imgs, labs, plans, out="uint8")
            save(X8, y, [f"{s}_{A.OP_NAMES[p.op]}_{c}" for s, p in zip(batch, plans)])
            written += len(batch)
    rng = np.random.default_rng(args.seed)
    done = attempts = 0
    while done < args.pairs and attempts < 10 * args.pairs and len(stems) >= 2:
        attempts += 1
        a, b = (stems[j] for j in rng.choice(len(stems), 2, replace=False))
        imgs, labs = fetch([a, b])
        (h1, w1), (h2, w2) = imgs[0].shape[:2], imgs[1].shape[:2]
        if (h1 > w1) != (h2 > w2):               # mismatched orientations: the reference's cell skips the pair too
            continue
        X8, y = A.merge_pairs(imgs[:1], labs[:1], imgs[1:], labs[1:], target_size=args.size, out="uint8")
        save(X8, y, [f"pair_{done}"])
        done += 1
    print(f"wrote {written} augmented images and {done} merged pairs to {args.out}")


if __name__ == "__main__":
    main()
