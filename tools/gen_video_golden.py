"""Generates tests/golden/video_tracks.json from the reference's own, unmodified tracking functions.

    python tools/gen_video_golden.py --reference <checkout of the reference project>

Runs only where the reference exists.  ``get_valid_faces`` (altfreezing/test_tools/ct/detection/utils.py), ``iou``
(ct/tracking/sort.py) and ``simple_tracking`` / ``multiple_tracking`` / ``find_longest`` (ct/operations.py) are pure numpy, but
their modules import cv2, matplotlib, scipy, filterpy and test_tools.utils at the top and never call them in these functions.  The
three files are loaded by file path, as a stand-in package so that ``from .tracking.sort import iou`` resolves, with empty stand-ins
in ``sys.modules`` for the absent imports for the duration of the load.  Nothing from the reference is copied into the repository:
only the seeded inputs and the recorded index lists are written.

Written (tests/golden/video_tracks.json), per case:
  frames   the detector-style input, per frame a list of faces {"box": [4], "lm": [5][2], "score"} (float32 values)
  args     the get_valid_faces arguments (max_count, thres, at_least)
  valid    per frame the indices (into that frame's input list) of the faces get_valid_faces keeps
  tracks   multiple_tracking(valid faces): per track one index per frame, into that frame's INPUT list
  spans / span_tracks   find_longest(valid faces): the (start, un_reach_end) tuples and per span the track, indices as above;
           "raises": "NotImplementedError" instead when the reference raises it
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STUBS = ["cv2", "matplotlib", "matplotlib.pyplot", "matplotlib.patches", "scipy", "scipy.optimize", "filterpy", "filterpy.kalman",
         "test_tools", "test_tools.utils"]


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):                                  # `from stub import anything` succeeds; nothing of it is called
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def load_reference(reference):
    """the reference's ct/detection/utils.py, ct/tracking/sort.py and ct/operations.py as modules of a stand-in package"""
    ct = os.path.join(reference, "altfreezing", "test_tools", "ct")
    saved = {k: sys.modules.get(k) for k in STUBS}
    made = []
    try:
        for k in STUBS:
            if saved[k] is None:
                sys.modules[k] = _Stub(k)
        for name, path in (("ref_ct", ct), ("ref_ct.tracking", os.path.join(ct, "tracking")), ("ref_ct.detection", os.path.join(ct, "detection"))):
            pkg = types.ModuleType(name)
            pkg.__path__ = [path]
            sys.modules[name] = pkg
            made.append(name)
        mods = {}
        for name, rel in (("ref_ct.tracking.sort", "tracking/sort.py"), ("ref_ct.operations", "operations.py"),
                          ("ref_ct.detection.utils", "detection/utils.py")):
            spec = importlib.util.spec_from_file_location(name, os.path.join(ct, rel))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            made.append(name)
            spec.loader.exec_module(mod)
            mods[name] = mod
    finally:
        for k in STUBS:
            if saved[k] is None:
                sys.modules.pop(k, None)
        for name in made:
            sys.modules.pop(name, None)
    return mods["ref_ct.detection.utils"], mods["ref_ct.operations"]


# ---- seeded detection lists ------------------------------------------------------------------------------------------------

def face(cx, cy, half, score, rng):
    box = np.array([cx - half, cy - half * 1.2, cx + half, cy + half * 1.2], dtype=np.float32)
    lm = (np.array([[-0.4, -0.3], [0.4, -0.3], [0.0, 0.1], [-0.3, 0.5], [0.3, 0.5]]) * half + [cx, cy] + rng.normal(0, 0.5, (5, 2))).astype(np.float32)
    return (box, lm, np.float32(score))


def walk(rng, n, cx, cy, half, score=0.99, vx=0.0, vy=0.0, jitter=1.5):
    out = []
    for _ in range(n):
        cx, cy = cx + vx + rng.normal(0, jitter), cy + vy + rng.normal(0, jitter)
        out.append(face(cx, cy, half + rng.normal(0, 0.5), score - rng.uniform(0, 0.01), rng))
    return out


def cases():
    out = {}
    args = dict(max_count=10, thres=0.5, at_least=False)
    rng = np.random.default_rng(11)
    out["steady"] = ([[f] for f in walk(rng, 14, 300, 200, 60)], args)
    rng = np.random.default_rng(12)                               # two faces on one line walk through each other
    a, b = walk(rng, 24, 150, 200, 50, vx=14.0), walk(rng, 24, 480, 204, 50, vx=-14.0, score=0.97)
    out["crossing"] = ([[x, y] for x, y in zip(a, b)], args)
    rng = np.random.default_rng(13)                               # the second face overlaps the first in frame 0, a third stands apart
    a, b, c = walk(rng, 10, 300, 200, 60), walk(rng, 10, 312, 206, 60, score=0.95), walk(rng, 10, 520, 200, 40, score=0.9)
    out["overlap_in_frame0"] = ([[x, y, z] for x, y, z in zip(a, b, c)], args)
    for name, s0 in (("frame0_score_079", 0.79), ("frame0_score_080", 0.80)):
        rng = np.random.default_rng(14)
        a = walk(rng, 12, 300, 200, 60)
        a[0] = (a[0][0], a[0][1], np.float32(s0))
        out[name] = ([[f] for f in a], args)
    rng = np.random.default_rng(15)                               # a face gone for three frames: no whole-video track, several spans
    a = walk(rng, 26, 300, 200, 60)
    out["vanishes"] = ([[f] if not 9 <= i < 12 else [] for i, f in enumerate(a)], args)
    rng = np.random.default_rng(16)                               # two faces, one gone from frame 8 on: the track count changes mid-run
    a, b = walk(rng, 20, 200, 200, 50), walk(rng, 20, 450, 200, 50, score=0.96)
    frames = [[x, y] if i < 8 else [x] for i, (x, y) in enumerate(zip(a, b))]
    frames[0] = [(a[0][0], a[0][1], np.float32(0.7)), b[0]]       # frame 0 refuses the face that stays
    out["count_changes"] = (frames, args)
    rng = np.random.default_rng(17)
    a = walk(rng, 12, 300, 200, 60)
    out["last_frame_empty"] = ([[f] for f in a[:-1]] + [[]], args)
    rng = np.random.default_rng(18)                               # 13 faces per frame in descending score order, the last ones weak
    rows = [walk(rng, 9, 60 + 45 * k, 100 + 30 * (k % 3), 18, score=0.99 - 0.045 * k, jitter=0.5) for k in range(13)]
    out["more_than_ten"] = ([[r[i] for r in rows] for i in range(9)], args)
    rng = np.random.default_rng(19)                               # weak first faces kept by at_least, weak second faces dropped
    a, b = walk(rng, 10, 300, 200, 60, score=0.45), walk(rng, 10, 520, 200, 40, score=0.3)
    a[0] = (a[0][0], a[0][1], np.float32(0.9))
    out["at_least"] = ([[x, y] for x, y in zip(a, b)], dict(max_count=10, thres=0.5, at_least=True))
    rng = np.random.default_rng(19)
    a, b = walk(rng, 10, 300, 200, 60, score=0.45), walk(rng, 10, 520, 200, 40, score=0.3)
    a[0] = (a[0][0], a[0][1], np.float32(0.9))
    out["not_at_least"] = ([[x, y] for x, y in zip(a, b)], args)
    return out


def index_of(face_obj, faces):
    return next(k for k, f in enumerate(faces) if f is face_obj)


def record(det_utils, ops, frames, args):
    valid = det_utils.get_valid_faces(frames, **args)
    # get_valid_faces makes new tuples: a kept face is found again in its frame's input by its score and first coordinate
    valid_idx = []
    for faces_in, faces_out in zip(frames, valid):
        idx, k = [], 0
        for f in faces_out:
            while not (faces_in[k][2] == f[2] and float(faces_in[k][0][0]) == float(f[0][0])):
                k += 1
            idx.append(k)
            k += 1
        valid_idx.append(idx)
        assert all(f[0].dtype == np.float64 and f[1].dtype == np.float64 for f in faces_out)

    def as_input_indices(track, start):
        return [valid_idx[start + t][index_of(f, valid[start + t])] for t, f in enumerate(track)]

    rec = {"args": args, "valid": valid_idx,
           "frames": [[{"box": [float(v) for v in f[0]], "lm": [[float(v) for v in p] for p in f[1]], "score": float(f[2])} for f in faces]
                      for faces in frames]}
    rec["tracks"] = [as_input_indices(t, 0) for t in ops.multiple_tracking(valid)]
    try:
        spans, tracks = ops.find_longest(valid)
        rec["spans"] = [[int(a), int(b)] for a, b in spans]
        rec["span_tracks"] = [as_input_indices(t, s[0]) for s, t in zip(spans, tracks)]
    except NotImplementedError:
        rec["raises"] = "NotImplementedError"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(GOLDEN, "video_tracks.json"))
    a = ap.parse_args()
    det_utils, ops = load_reference(a.reference)
    out = {"source": "altfreezing/test_tools/ct: detection/utils.py get_valid_faces, tracking/sort.py iou, operations.py "
                     "simple_tracking / multiple_tracking / find_longest, executed unmodified",
           "cases": {name: record(det_utils, ops, frames, args) for name, (frames, args) in cases().items()}}
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    for name, rec in out["cases"].items():
        print(name, "tracks", len(rec["tracks"]), "spans", rec.get("spans", rec.get("raises")))


if __name__ == "__main__":
    main()
