"""Writes tests/golden/bytetrack_tracks.json: a scripted call driven through the REFERENCE's own ``BYTETracker``
(preprocessing/ByteTrack/byte_tracker.py), frame by frame, with what it returned.  tests/test_tracker_host.py replays the file
through ``af_mi355x.tracker.ByteTracker``.

    python tools/gen_bytetrack_golden.py [--reference DIR]

The reference's matching.py imports three packages that are not installed where this runs; this script puts stand-ins of its
own into ``sys.modules`` before importing it:
  lap          ``lapjv(cost, extend_cost=True, cost_limit=t)``: scipy's ``linear_sum_assignment`` on lap's extended matrix (side
               n + m, padding ``t / 2``, the padding-to-padding block 0).  The script keeps no two costs equal (+-0.3 px of seeded
               jitter on every coordinate) and the stand-in ASSERTS that the optimum of every matrix it solves is unique - exchanging
               the columns of any two rows raises the cost by more than 1e-9 unless the exchange pairs nothing differently - so any
               exact solver, lapjv included, returns these pairs;
  cython_bbox  ``bbox_overlaps`` in numpy, with its + 1 pixel convention;
  cv2          empty (matching.py imports it and uses nothing of it).

The script (240 frames of 640x480, ``track_thresh = 0.8, track_buffer = 90, match_thresh = 0.8, mot20 = False``, 30 fps): faces A
and B on smooth paths that cross with IoU > 0.5 for several frames; C absent for 40 frames and back (lost, re-found); D absent for
longer than the buffer (removed; a new id on return); A with scores between 0.1 and ``track_thresh`` for a while; a one-frame false
detection (an unconfirmed track that dies); two near-identical boxes for a few frames (duplicate removal); a frame without
detections; ``tracks_in = []`` on alternate frames (``detect_every = 2``); and a stretch handed over in the tracker's ARRAY form,
because a list of ``STrack`` - all af_realtime.py ever passes - never reaches the second association (byte_tracker.py:232-261);
the rows go in as an ndarray subclass with a truth value, since :228 tests ``not output_results`` on whatever it is given.
Each of these is asserted to have happened before the file is written.
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
W, H, FRAMES = 640, 480, 240
ARGS = dict(track_thresh=0.8, track_buffer=90, match_thresh=0.8, mot20=False)
EVENTS = {"second_match": [], "solved": 0, "duplicates_dropped": []}
_frame = [0]


def _unique_optimum(ext, rows, cols, n, m):
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            r1, c1, r2, c2 = rows[i], cols[i], rows[j], cols[j]
            if (r1 >= n and r2 >= n) or (c1 >= m and c2 >= m):
                continue                               # padding exchanged with padding: the same pairs
            delta = ext[r1, c2] + ext[r2, c1] - ext[r1, c1] - ext[r2, c2]
            assert delta > 1e-9, "frame %d: the assignment is not unique (exchange of rows %d, %d changes the cost by %g)" % (
                _frame[0], r1, r2, delta)


def _lapjv(cost, extend_cost=True, cost_limit=np.inf):
    assert extend_cost and np.isfinite(cost_limit)
    n, m = cost.shape
    ext = np.full((n + m, n + m), cost_limit / 2.0)
    ext[n:, m:] = 0
    ext[:n, :m] = cost
    rows, cols = linear_sum_assignment(ext)
    _unique_optimum(ext, rows, cols, n, m)
    EVENTS["solved"] += 1
    x, y = -np.ones(n, dtype=int), -np.ones(m, dtype=int)
    for r, c in zip(rows, cols):
        if r < n and c < m:
            x[r], y[c] = c, r
    if cost_limit == 0.5 and (x >= 0).any():           # 0.5 is the second association's limit alone (byte_tracker.py:302)
        EVENTS["second_match"].append(_frame[0])
    return float(ext[rows, cols].sum()), x, y


def _bbox_overlaps(a, b):
    out = np.zeros((len(a), len(b)))
    for k in range(len(b)):
        area = (b[k, 2] - b[k, 0] + 1) * (b[k, 3] - b[k, 1] + 1)
        for n in range(len(a)):
            iw = min(a[n, 2], b[k, 2]) - max(a[n, 0], b[k, 0]) + 1
            ih = min(a[n, 3], b[k, 3]) - max(a[n, 1], b[k, 1]) + 1
            if iw > 0 and ih > 0:
                out[n, k] = iw * ih / float((a[n, 2] - a[n, 0] + 1) * (a[n, 3] - a[n, 1] + 1) + area - iw * ih)
    return out


def import_reference_tracker(reference):
    for name, attrs in (("lap", {"lapjv": _lapjv}), ("cython_bbox", {"bbox_overlaps": _bbox_overlaps}), ("cv2", {})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    pkg = types.ModuleType("ref_bytetrack")              # the directory as a package of its own: no parent __init__ runs
    pkg.__path__ = [os.path.join(reference, "preprocessing", "ByteTrack")]
    sys.modules["ref_bytetrack"] = pkg
    bt = importlib.import_module("ref_bytetrack.byte_tracker")
    inner = bt.remove_duplicate_stracks

    def watched(a, b):
        ra, rb = inner(a, b)
        if len(ra) < len(a) or len(rb) < len(b):
            EVENTS["duplicates_dropped"].append(_frame[0])
        return ra, rb
    bt.remove_duplicate_stracks = watched
    return bt


class _Rows(np.ndarray):
    """byte_tracker.py:228 asks ``if not output_results`` before it looks at the type, which numpy refuses for a plain array of
    more than one element: the array form is entered with an array that answers that question"""

    def __bool__(self):
        return self.size > 0


def script(seed=20):
    """per frame ``(form, [[x, y, w, h, score], ...])``; form "stracks" (af_realtime.py:386) or "array" (tlbr rows)"""
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(FRAMES):
        dets = []
        a = [100 + 2.0 * f if f < 120 else 340 - 1.5 * (f - 120), 100 + 0.3 * f, 110, 130, 0.95]
        b = [400 - 2.0 * f if f < 120 else 160 + 1.0 * (f - 120), 122 + 0.2 * f, 100, 120, 0.93]
        c = [250 + 20 * np.sin(f / 25.0), 320 + 10 * np.cos(f / 30.0), 90, 100, 0.92]
        d = [510 - 0.2 * f, 330 - 0.1 * f, 85, 95, 0.94]
        if 30 <= f < 42:
            a[4] = 0.6                                   # between 0.1 and track_thresh, in the list form: first association
        if 180 <= f < 200:
            b[4] = 0.5                                   # the same in the array form: second association
        dets.append(a)
        dets.append(b)
        if not 100 <= f < 140:
            dets.append(c)
        if f < 21 or f >= 135:
            dets.append(d)
        if f == 50:
            dets.append([20, 20, 90, 90, 0.96])          # a false detection, one frame
        if 150 <= f < 153:
            dets.append([a[0] + 2.5, a[1] + 1.5, a[2] + 1, a[3] - 1, 0.91])     # A seen twice
        if f == 160 or (f >= 210 and f % 2 == 1):
            dets = []
        rows = []
        for x, y, w, h, s in dets:
            j = rng.uniform(-0.3, 0.3, 4)
            rows.append([float(x + j[0]), float(y + j[1]), float(w + j[2]), float(h + j[3]), float(s + rng.uniform(-0.004, 0.004))])
        frames.append(("array" if 176 <= f < 204 else "stracks", rows))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bytetrack_tracks.json"))
    a = ap.parse_args()
    if a.reference is None:
        import ref_import
        a.reference = ref_import.REFERENCE_ROOT
    bt = import_reference_tracker(a.reference)
    assert bt.BaseTrack._count == 0
    tracker = bt.BYTETracker(types.SimpleNamespace(**ARGS), frame_rate=30.0)
    out, was_lost, ids_of_d, cross = [], set(), set(), 0
    reactivated, removed_ids, dead_unconfirmed = [], set(), set()
    for f, (form, rows) in enumerate(script()):
        _frame[0] = f
        if len(rows) >= 2 and f < 120:
            ta = np.array([[r[0], r[1], r[0] + r[2], r[1] + r[3]] for r in rows[:2]])
            cross += _bbox_overlaps(ta[:1], ta[1:])[0, 0] > 0.5
        if form == "stracks":
            tracks_in = [bt.STrack(np.asarray(r[:4], dtype=np.float32), score=float(np.float32(r[4]))) for r in rows]
            online = tracker.update(tracks_in, (H, W), (H, W))
        else:                                            # tlbr rows; (H, W) against (W, H) makes the reference's scale 1
            arr = np.array([[r[0], r[1], r[0] + r[2], r[1] + r[3], r[4]] for r in rows], dtype=np.float64).reshape(-1, 5)
            online = tracker.update(arr.view(_Rows), (H, W), (W, H))
        for t in tracker.tracked_stracks:
            if t.track_id in was_lost and t.state == bt.TrackState.Tracked:
                reactivated.append(f)
                was_lost.discard(t.track_id)
        was_lost |= {t.track_id for t in tracker.lost_stracks}
        for t in tracker.removed_stracks:
            removed_ids.add(t.track_id)
            if not t.is_activated:
                dead_unconfirmed.add(t.track_id)
        for t in online:
            if abs(t.tlbr[0] - (510 - 0.2 * f)) < 8 and abs(t.tlbr[1] - (330 - 0.1 * f)) < 8:
                ids_of_d.add(t.track_id)
        out.append({
            "form": form, "img_info": [H, W], "img_size": [H, W] if form == "stracks" else [W, H], "detections": rows,
            "tracker_frame_id": tracker.frame_id,
            "tracks": [{"track_id": int(t.track_id), "tlbr": [float(v) for v in t.tlbr], "score": float(t.score), "state": int(t.state),
                        "is_activated": bool(t.is_activated)} for t in online],
            "tracked_ids": [int(t.track_id) for t in tracker.tracked_stracks],
            "lost_ids": [int(t.track_id) for t in tracker.lost_stracks],
            "n_removed": len(tracker.removed_stracks)})
    events = {"reactivated": sorted(set(reactivated)), "second_match": EVENTS["second_match"], "removed_ids": sorted(removed_ids),
              "dead_unconfirmed_ids": sorted(dead_unconfirmed), "duplicates_dropped": EVENTS["duplicates_dropped"],
              "ids_of_the_face_that_left_for_longer_than_the_buffer": sorted(ids_of_d), "crossing_frames_iou_over_half": int(cross),
              "empty_frames": [f for f, fr in enumerate(out) if not fr["detections"]], "matrices_solved": EVENTS["solved"]}
    assert len(out) == FRAMES and max(len(fr["tracks"]) for fr in out) >= 3
    assert events["reactivated"], "no track was re-activated"
    assert events["second_match"], "no second-association match"
    assert events["dead_unconfirmed_ids"], "no unconfirmed track died"
    assert set(events["removed_ids"]) - set(events["dead_unconfirmed_ids"]), "no confirmed track was removed"
    assert len(events["ids_of_the_face_that_left_for_longer_than_the_buffer"]) == 2, events
    assert events["duplicates_dropped"], "no duplicate was dropped"
    assert events["crossing_frames_iou_over_half"] >= 5, events
    assert 160 in events["empty_frames"] and len(events["empty_frames"]) > 10
    doc = {"what": "tracks the reference BYTETracker returned for a scripted call (tools/gen_bytetrack_golden.py)", "args": ARGS,
           "frame_rate": 30.0, "first_track_id": 1, "events": events, "frames": out}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
    print("wrote %s: %d bytes, events %s" % (a.out, os.path.getsize(a.out), json.dumps(events)))


if __name__ == "__main__":
    main()
