#!/usr/bin/env python3
"""Distil one or more trained checkpoints into a U-Net student over image files: a thin shell over
image_segmentation_amd.Teacher, DistillLoss and train_loop_distill.  With --labels every image IMAGES/<name>.* is
paired with LABELS/<name>.png, an 8-bit map of class ids, and the loss is alpha * soft + (1 - alpha) * CrossEntropy; without,
the images are unlabelled and the loss is the soft term alone.  Writes the student as {"epoch", "model_state_dict"}.
Usage: python tools/distill.py --teacher unet:big.pt [--teacher autoencoder:other.pt ...] [--student start.pt] --classes 4
       --images DIR [--labels DIR] --out student.pt [--epochs 10] [--alpha 0.5] [--temperature 2] [--flips ,h]
       [--min-confidence 0] [--ignore-index 3] [--target-size 224] [--batch-size 32] [--lr 1e-3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--teacher", action="append", required=True, metavar="MODEL:FILE",
                    help="a teacher checkpoint, MODEL one of unet / autoencoder; repeat for an ensemble")
    ap.add_argument("--student", default=None, help="checkpoint the U-Net student starts from (default: a fresh one)")
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--images", required=True, help="folder of image files")
    ap.add_argument("--labels", default=None, help="folder of <name>.png class-id maps (default: unlabelled, alpha = 1)")
    ap.add_argument("--out", required=True, help="checkpoint file to write")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=None, help="weight of the soft term (default: 0.5 with labels, 1 without)")
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--flips", default="", metavar="F,F", help="teacher views per model: comma-separated of '', h, v, hv")
    ap.add_argument("--min-confidence", type=float, default=0.0, help="leave out pixels the teachers are less sure of")
    ap.add_argument("--ignore-index", type=int, default=None, help="label value left out of both terms")
    ap.add_argument("--target-size", type=int, default=224, help="side of the square network input")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()

    import numpy as np
    import torch
    from PIL import Image
    import image_segmentation_amd as seg

    def build(kind):
        if kind == "unet":
            return seg.unet(3, args.classes)
        if kind == "autoencoder":
            return seg.SegmentationAutoencoder(3, num_classes=args.classes)
        ap.error(f"unknown teacher model {kind!r}: unet or autoencoder")

    teachers = []
    for spec in args.teacher:
        kind, _, path = spec.partition(":")
        if not path:
            ap.error(f"--teacher takes MODEL:FILE, got {spec!r}")
        teachers.append(seg.load_checkpoint(build(kind), path).cuda())
    student = seg.unet(3, args.classes)
    if args.student:
        student = seg.load_checkpoint(student, args.student)
    student = student.cuda()

    names = sorted(f for f in os.listdir(args.images) if not f.startswith("."))
    if not names:
        ap.error(f"no files in {args.images}")
    samples = []
    for f in names:
        img = torch.from_numpy(np.asarray(Image.open(os.path.join(args.images, f)).convert("RGB")).copy()).permute(2, 0, 1).float() / 255
        lab = None
        if args.labels:
            path = os.path.join(args.labels, os.path.splitext(f)[0] + ".png")
            if not os.path.exists(path):
                ap.error(f"{f} has no label {path}")
            lab = torch.from_numpy(np.asarray(Image.open(path).convert("L")).astype(np.int64)).unsqueeze(0)
        samples.append((img, lab))

    def batches():          # lists of differently sized images: train_loop_distill resizes and pads them to target_size
        order = torch.randperm(len(samples)).tolist()
        out = []
        for i in range(0, len(order), args.batch_size):
            chunk = [samples[j] for j in order[i:i + args.batch_size]]
            out.append(([c[0] for c in chunk], [c[1] for c in chunk] if args.labels else None))
        return out

    alpha = args.alpha if args.alpha is not None else (0.5 if args.labels else 1.0)
    hard = seg.CrossEntropyLoss(ignore_index=-100 if args.ignore_index is None else args.ignore_index) if args.labels else None
    try:
        teacher = seg.Teacher(teachers, flips=tuple(args.flips.split(",")))
        loss_fn = seg.DistillLoss(hard=hard, alpha=alpha, temperature=args.temperature, ignore_index=args.ignore_index,
                                  min_confidence=args.min_confidence)
    except ValueError as e:
        ap.error(str(e))
    optimizer = torch.optim.AdamW(student.parameters(), lr=args.lr)
    for epoch in range(args.epochs):
        avg = seg.train_loop_distill(batches(), student, teacher, loss_fn, optimizer, 1, "cuda", target_size=args.target_size)
        last = loss_fn.last
        n = max(int(last["n"].item()), 1)
        print(f"epoch {epoch + 1}: loss {avg:.6f}  (last batch: soft {last['soft'].item():.6f}, "
              f"student agrees with the teachers on {int(last['n_agree'].item()) / n:.1%} of {n} pixels)")
    torch.save({"epoch": args.epochs, "model_state_dict": student.state_dict()}, args.out)


if __name__ == "__main__":
    main()
