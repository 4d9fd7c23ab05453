"""CPU: tracker.ByteTracker against tracks recorded from the reference's own BYTETracker (tests/golden/bytetrack_tracks.json,
written by tools/gen_bytetrack_golden.py), and iou_distance on hand-worked boxes.

  replay     per frame the returned track ids (in order), states and activation flags are equal, the tracker's tracked and lost
             lists hold the same ids, and tlbr agrees within 1e-6 px: both sides are fp64 with the same operations on boxes under
             2 000 px, 240 steps of round-off stay many orders below that, and a logic slip moves a box by whole pixels
  fixture    it contains a re-activation, a second-association match, a removed track, a dead unconfirmed track, a dropped
             duplicate and empty frames - and the replayed tracker shows the same events itself
  iou        three pairs worked by hand, the + 1 pixel convention among them
"""
import json
import os
import types

import numpy as np
import pytest

from af_mi355x import tracker
from af_mi355x.tracker import ByteTracker, STrack, iou_distance

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bytetrack_tracks.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _tracks_in(frame):
    rows = frame["detections"]
    if frame["form"] == "stracks":                    # af_realtime.py:384-386: float32 rows, a Python float score
        return [STrack(np.asarray(r[:4], dtype=np.float32), score=float(np.float32(r[4]))) for r in rows]
    return np.array([[r[0], r[1], r[0] + r[2], r[1] + r[3], r[4]] for r in rows], dtype=np.float64).reshape(-1, 5)


def test_replay_of_the_reference_tracks(golden):
    tr = ByteTracker(types.SimpleNamespace(**golden["args"]), frame_rate=golden["frame_rate"])
    worst, was_lost, reactivated, second = 0.0, set(), [], []
    real = tracker.linear_assignment

    def watched(cost, thresh):
        out = real(cost, thresh)
        if thresh == 0.5 and len(out[0]):
            second.append(f)
        return out
    tracker.linear_assignment = watched
    try:
        for f, frame in enumerate(golden["frames"]):
            online = tr.update(_tracks_in(frame), tuple(frame["img_info"]), tuple(frame["img_size"]))
            want = frame["tracks"]
            assert [t.track_id for t in online] == [w["track_id"] for w in want], f
            assert [t.state for t in online] == [w["state"] for w in want], f
            assert [t.is_activated for t in online] == [w["is_activated"] for w in want], f
            assert [t.score for t in online] == [w["score"] for w in want], f
            assert tr.frame_id == frame["tracker_frame_id"], f
            assert [t.track_id for t in tr.tracked_stracks] == frame["tracked_ids"], f
            assert [t.track_id for t in tr.lost_stracks] == frame["lost_ids"], f
            assert len(tr.removed_stracks) == frame["n_removed"], f
            for t, w in zip(online, want):
                d = float(np.abs(t.tlbr - np.asarray(w["tlbr"])).max())
                worst = max(worst, d)
                assert d <= 1e-6, (f, t.track_id, d)
            for t in tr.tracked_stracks:
                if t.track_id in was_lost:
                    reactivated.append(f)
                    was_lost.discard(t.track_id)
            was_lost |= {t.track_id for t in tr.lost_stracks}
    finally:
        tracker.linear_assignment = real
    print("worst |tlbr - reference| = %.3g px over %d frames" % (worst, len(golden["frames"])))
    ev = golden["events"]
    assert sorted(set(reactivated)) == ev["reactivated"] and second == ev["second_match"]
    assert sorted({t.track_id for t in tr.removed_stracks}) == ev["removed_ids"]
    assert sorted({t.track_id for t in tr.removed_stracks if not t.is_activated}) == ev["dead_unconfirmed_ids"]
    assert min(t.track_id for t in tr.removed_stracks) >= golden["first_track_id"] == 1


def test_the_fixture_is_not_a_trivial_script(golden):
    ev, frames = golden["events"], golden["frames"]
    assert len(frames) >= 240 and os.path.getsize(GOLDEN) < 512 * 1024
    assert ev["reactivated"] and ev["second_match"] and ev["duplicates_dropped"] and ev["dead_unconfirmed_ids"]
    assert set(ev["removed_ids"]) - set(ev["dead_unconfirmed_ids"])                      # a confirmed track was removed too
    assert len(ev["ids_of_the_face_that_left_for_longer_than_the_buffer"]) == 2          # and came back under a new id
    assert ev["crossing_frames_iou_over_half"] >= 5
    assert max(len(fr["tracks"]) for fr in frames) >= 3
    empty = [f for f, fr in enumerate(frames) if not fr["detections"]]
    assert empty == ev["empty_frames"] and len(empty) > 10
    assert any(b - a == 2 for a, b in zip(empty, empty[1:]))                             # alternate frames: detect_every = 2
    thr = golden["args"]["track_thresh"]
    assert any(0.1 < r[4] < thr for fr in frames if fr["form"] == "stracks" for r in fr["detections"])
    assert any(0.1 < r[4] < thr for fr in frames if fr["form"] == "array" for r in fr["detections"])
    assert {fr["form"] for fr in frames} == {"stracks", "array"}


def test_iou_distance_on_hand_worked_pairs():
    a = [np.array([0.0, 0.0, 9.0, 9.0])]
    # identical boxes: 10 x 10 pixels each in the + 1 convention, IoU 1
    assert iou_distance(a, [np.array([0.0, 0.0, 9.0, 9.0])])[0, 0] == 0.0
    # shifted by 5 in x: intersection (9 - 5 + 1) * 10 = 50, union 100 + 100 - 50 = 150; without the + 1 it would be 36 / 126
    assert iou_distance(a, [np.array([5.0, 0.0, 14.0, 9.0])])[0, 0] == pytest.approx(1 - 50.0 / 150.0, abs=1e-15)
    # touching at x = 10 with no shared pixel: min(9, 19) - max(0, 10) + 1 = 0 -> no overlap; sharing the column x = 9: 1 * 10 / 190
    assert iou_distance(a, [np.array([10.0, 0.0, 19.0, 9.0])])[0, 0] == 1.0
    assert iou_distance(a, [np.array([9.0, 0.0, 18.0, 9.0])])[0, 0] == pytest.approx(1 - 10.0 / 190.0, abs=1e-15)
    # the track form reads .tlbr; an empty side gives an empty matrix
    t = STrack([0.0, 0.0, 9.0, 9.0], 0.9)             # tlwh: tlbr (0, 0, 9, 9)
    assert iou_distance([t], [t]).tolist() == [[0.0]] and iou_distance([], [t]).shape == (0, 1)


def test_linear_assignment_keeps_a_match_only_within_the_limit():
    cost = np.array([[0.1, 0.9], [0.85, 0.2], [0.95, 0.97]])
    m, ua, ub = tracker.linear_assignment(cost, 0.8)
    assert m.tolist() == [[0, 0], [1, 1]] and list(ua) == [2] and list(ub) == []
    m, ua, ub = tracker.linear_assignment(np.array([[0.81]]), 0.8)                      # above the limit: both stay unmatched
    assert len(m) == 0 and list(ua) == [0] and list(ub) == [0]
    m, ua, ub = tracker.linear_assignment(np.zeros((0, 3)), 0.8)
    assert len(m) == 0 and list(ua) == [] and list(ub) == [0, 1, 2]
