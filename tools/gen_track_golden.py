"""Generates tests/golden/track_windows.json from the reference's own, unmodified lines.

    python tools/gen_track_golden.py --reference <checkout of the reference project>

Runs only where the reference exists.  altfreezing/demo.py cannot be imported without cv2, pynvml and sklearn, so the lines
that build the clips of a track (from ``clips_for_video = []`` up to ``preds = []``, found by those text anchors) are
executed as they stand with ``tuples`` / ``tracks`` / ``cfg_obj.clip_size`` supplied; altfreezing/test_tools/utils.py is loaded
by file path with an empty stand-in for the ``cv2`` module it imports and never calls in ``get_crop_box``.  Nothing from the
reference is copied into the repository: only the recorded index lists and boxes are written.

Written (tests/golden/track_windows.json):
  windows     per track length T in TRACK_LENGTHS the index lists of the reference's clips at clip_size 32
  crop_boxes  get_crop_box(shape, box, 0.5) for seeded boxes, some of them clipped by the frame edge
"""
import argparse
import importlib.util
import json
import os
import sys
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TRACK_LENGTHS = [1, 2, 3, 5, 16, 31, 32, 33, 40]
CLIP_SIZE = 32
BOX_SEED, N_BOXES, FRAME_SHAPE = 7, 12, (360, 640)
START, STOP = "clips_for_video = []", "preds = []"


def reference_windows(demo_py, T, clip_size):
    lines = open(demo_py).read().splitlines()
    lo = next(i for i, l in enumerate(lines) if l.strip() == START)
    hi = next(i for i, l in enumerate(lines) if i > lo and l.strip() == STOP)
    block = textwrap.dedent("\n".join(lines[lo:hi]))
    ns = {"tuples": [(0, T)], "tracks": [[None] * T], "cfg_obj": types.SimpleNamespace(clip_size=clip_size)}
    exec(compile(block, demo_py, "exec"), ns)
    return [[int(j) for _, j in clip] for clip in ns["clips_for_video"]]


def load_utils(path):
    had = "cv2" in sys.modules
    if not had:
        sys.modules["cv2"] = types.ModuleType("cv2")              # imported at the top of the file, not called by get_crop_box
    try:
        spec = importlib.util.spec_from_file_location("ref_test_tools_utils", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if not had:
            del sys.modules["cv2"]
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(GOLDEN, "track_windows.json"))
    args = ap.parse_args()
    demo_py = os.path.join(args.reference, "altfreezing", "demo.py")
    utils = load_utils(os.path.join(args.reference, "altfreezing", "test_tools", "utils.py"))
    windows = {str(T): reference_windows(demo_py, T, CLIP_SIZE) for T in TRACK_LENGTHS}
    rng = np.random.default_rng(BOX_SEED)
    h, w = FRAME_SHAPE
    boxes = []
    for i in range(N_BOXES):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        if i % 3 == 0:                                            # near a corner: the grown box is clipped on two sides
            cx, cy = rng.choice([15.0, w - 15.0]), rng.choice([12.0, h - 12.0])
        bw, bh = rng.uniform(30, 220), rng.uniform(30, 220)
        box = np.array([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2])
        boxes.append({"box": box.tolist(), "crop_box": [int(v) for v in utils.get_crop_box(FRAME_SHAPE, box, scale=0.5)]})
    out = {"clip_size": CLIP_SIZE, "source": "altfreezing/demo.py clips_for_video lines; altfreezing/test_tools/utils.py get_crop_box",
           "windows": windows, "frame_shape": list(FRAME_SHAPE), "crop_boxes": boxes}
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", args.out, {k: len(v) for k, v in windows.items()})


if __name__ == "__main__":
    main()
