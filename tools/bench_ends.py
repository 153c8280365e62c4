#!/usr/bin/env python3
"""bench.py with the unstored-gradient form of the two ends of the full-resolution level switched per end, for same-box A/B
runs of each end on its own (profiles/end_fusion_ab.txt).  Usage: python tools/bench_ends.py {both|head|stem|none} [bench.py
arguments]: the named end(s) take the unstored form at every size, the other the stored sequence; nothing else of the run
differs from `python bench.py`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    which = sys.argv.pop(1) if len(sys.argv) > 1 else ""
    if which not in ("both", "head", "stem", "none"):
        sys.exit(__doc__)
    from image_segmentation_amd import ops
    ops.END_FUSION_MIN_BYTES = {end: 0 if which in (end, "both") else float("inf") for end in ("head", "stem")}
    import bench
    bench.main()


if __name__ == "__main__":
    main()
