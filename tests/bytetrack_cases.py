"""The sequences the device-tracker tests replay, and how two trackers are compared after a frame.

A sequence is ``(args, frames)``; a frame is ``(form, rows)`` with ``form`` "stracks" (rows x, y, w, h, score as float32: what
``RealtimeCall._track`` builds), "array" ((n, 5) fp64 tlbr + score) or "empty".  ``golden()`` is the reference's own recording;
the four scripts cover, between them, two faces crossing with IoU over 0.5, a face absent for longer than the buffer, alternate
empty frames (``detect_every = 2``), a one-frame detection that dies unconfirmed, low-score rows for the second association and
32 faces at once."""
import json
import os
import types

import numpy as np

from af_mi355x.tracker import STrack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bytetrack_tracks.json")
SIZE = (720, 1280)


def _args(track_thresh=0.8, track_buffer=90, match_thresh=0.8):
    return types.SimpleNamespace(track_thresh=track_thresh, track_buffer=track_buffer, match_thresh=match_thresh, mot20=False)


def golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    frames = []
    for fr in g["frames"]:
        rows = np.asarray(fr["detections"], dtype=np.float64).reshape(-1, 5)
        if len(rows) == 0:
            frames.append(("empty", rows))
        elif fr["form"] == "stracks":
            frames.append(("stracks", rows.astype(np.float32)))
        else:
            frames.append(("array", np.concatenate([rows[:, :2], rows[:, :2] + rows[:, 2:4], rows[:, 4:]], axis=1)))
    return types.SimpleNamespace(**g["args"]), frames, g


def _face(rng, cx, cy, w, h, score, jitter=1.5):
    j = rng.normal(0.0, jitter, 4)
    return [cx - w / 2 + j[0], cy - h / 2 + j[1], w + j[2], h + j[3], score + rng.uniform(-0.02, 0.02)]


def _list(rows):
    return ("stracks", np.asarray(rows, dtype=np.float32).reshape(-1, 5)) if len(rows) else ("empty", np.zeros((0, 5)))


def crossing():
    """two faces pass through each other (IoU over 0.5 for several frames), then part"""
    rng, frames = np.random.default_rng(11), []
    for f in range(48):
        a = _face(rng, 300 + 9.0 * f, 300 + 0.5 * f, 120, 150, 0.93)
        b = _face(rng, 732 - 9.0 * f, 310 - 0.4 * f, 110, 140, 0.90)
        frames.append(_list([a, b]))
    return _args(), frames


def absent():
    """array form, buffer 8: a face leaves for 14 frames and comes back under a new id; another is seen with a low score for a
    while (second association); a third shows up for one frame only and dies unconfirmed"""
    rng, frames = np.random.default_rng(12), []
    for f in range(44):
        rows = []
        if f < 10 or f >= 24:
            rows.append(_face(rng, 250 + 2.0 * f, 240, 130, 160, 0.92))
        rows.append(_face(rng, 800 - 1.5 * f, 400, 140, 170, 0.55 if 14 <= f < 20 else 0.91))
        if f == 5:
            rows.append(_face(rng, 1050, 150, 100, 120, 0.95))
        r = np.asarray(rows, dtype=np.float64)
        frames.append(("array", np.concatenate([r[:, :2], r[:, :2] + r[:, 2:4], r[:, 4:]], axis=1)))
    return _args(track_buffer=8), frames


def alternate():
    """``detect_every = 2``: every other frame has no detection; two faces, one of which stops being detected for good"""
    rng, frames = np.random.default_rng(13), []
    for f in range(40):
        if f % 2:
            frames.append(_list([]))
            continue
        rows = [_face(rng, 400 + 3.0 * f, 300, 150, 180, 0.94)]
        if f < 16:
            rows.append(_face(rng, 900, 350 + 2.0 * f, 120, 150, 0.91))
        frames.append(_list(rows))
    return _args(track_buffer=6), frames


def crowd():
    """32 faces at once on a grid, each drifting its own way; two of them blink out for a frame"""
    rng, frames = np.random.default_rng(14), []
    drift = rng.uniform(-2.0, 2.0, (32, 2))
    for f in range(8):
        rows = []
        for i in range(32):
            if f == 4 and i in (7, 20):
                continue
            cx, cy = 90 + 150 * (i % 8) + drift[i, 0] * f, 100 + 170 * (i // 8) + drift[i, 1] * f
            rows.append(_face(rng, cx, cy, 90, 110, 0.93, jitter=1.0))
        frames.append(_list(rows))
    return _args(), frames


SCRIPTS = {"crossing": crossing, "absent": absent, "alternate": alternate, "crowd": crowd}


def sequence(name):
    """``(args, frames, frame_rate)`` of "golden" or a script"""
    if name == "golden":
        args, frames, g = golden()
        return args, frames, g["frame_rate"]
    args, frames = SCRIPTS[name]()
    return args, frames, 30.0


ALL = ("golden",) + tuple(SCRIPTS)


def tracks_in(frame):
    """a frame as ``ByteTracker.update`` takes it (a fresh object every time: the array form is scaled in place)"""
    form, rows = frame
    if form == "empty":
        return []
    if form == "stracks":
        return [STrack(r[:4], score=float(r[4])) for r in rows]
    return rows.copy()


def assert_same_frame(ref, got, online_ref, online_got, dump, where):
    """the statement ``ref`` (bytetrack_ref.RefByteTracker) and a ``DeviceByteTracker`` ``got`` after the same frame: every number
    equal, by ``np.array_equal`` where it is a float"""
    assert [t.track_id for t in online_got] == [t.track_id for t in online_ref], where
    assert [t.state for t in online_got] == [t.state for t in online_ref], where
    assert [t.is_activated for t in online_got] == [t.is_activated for t in online_ref], where
    assert [t.score for t in online_got] == [t.score for t in online_ref], where
    for a, b in zip(online_got, online_ref):
        assert np.array_equal(a.tlbr, b.tlbr), (where, a.track_id, a.tlbr, b.tlbr)
    assert got.frame_id == ref.frame_id, where
    assert got.tracked_ids == [t.track_id for t in ref.tracked_stracks], where
    assert got.lost_ids == [t.track_id for t in ref.lost_stracks], where
    assert got.removed_ids == ref.removed_ids, where
    assert dump["frame_id"] == ref.frame_id and dump["count"] == ref._count, where
    for slots, tracks in ((dump["tracked"], ref.tracked_stracks), (dump["lost"], ref.lost_stracks)):
        assert [int(s["id"]) for s in slots] == [t.track_id for t in tracks], where
        for s, t in zip(slots, tracks):
            assert np.array_equal(s["mean"], np.asarray(t.mean)), (where, t.track_id, "mean")
            assert np.array_equal(s["cov"], np.asarray(t.covariance)), (where, t.track_id, "covariance")
            assert (int(s["state"]), bool(s["activated"]), int(s["frame_id"]), int(s["start_frame"]), int(s["tracklet_len"])) == \
                (t.state, t.is_activated, t.frame_id, t.start_frame, t.tracklet_len), (where, t.track_id)


def rows_in_place(make_tracker, to_tensor, launch):
    """a scripted detector's (B, N, 15) rows and counts handed to ``rows_job`` where they lie, six ticks of six calls: rows on and
    just under ``start_conf`` and ``start_min_size``, counts of 0, one call with a ``detect_size`` scale-back; the result must be
    ``RealtimeCall._track``'s filter followed by the statement.  ``make_tracker(args)`` -> a DeviceByteTracker, ``to_tensor(numpy)``
    -> a tensor where that tracker reads, ``launch(jobs)`` -> their parsed records"""
    import bytetrack_ref as ref
    from af_mi355x.detector import YuNet
    B, N, TICKS_I = 6, 16, 6
    rng = np.random.default_rng(31)
    args = _args()
    start_conf, start_min_size = 0.76, 20
    scales = [(1.0, 1.0)] * B
    scales[4] = (1280 / 608.0, 720 / 352.0)                                  # this call detects on a 608 x 352 copy of its 1280 x 720 frames
    refs = [ref.RefByteTracker(args, 30.0) for _ in range(B)]
    devs = [make_tracker(args) for _ in range(B)]
    cut = {"conf": 0, "size": 0, "empty": 0, "kept": 0}
    for tick in range(TICKS_I):
        rows = rng.uniform(0.0, 1.0, (B, N, 15)).astype(np.float32)          # what lies past a count is never read as a face
        counts = np.zeros(B, dtype=np.int32)
        for b in range(B):
            n = 0 if (b == 2 and tick % 2) or b == 5 else 4
            counts[b] = n
            for i in range(n):
                w, h, score = 60.0, 70.0, 0.9 + 0.01 * i
                if i == 1:
                    score = 0.76 if tick % 2 else np.float32(0.7599999)      # on the limit (kept) and just under it (cut)
                if i == 2:
                    w, h = (19.98, 19.0) if tick % 2 else (20.0, 12.0)       # just under start_min_size (cut) and on it (kept)
                x, y = 40 + 110 * i + 3.0 * tick + rng.uniform(-1, 1), 50 + 30 * b + 2.0 * tick + rng.uniform(-1, 1)
                sx, sy = scales[b]
                rows[b, i, :5] = [x / sx, y / sy, w / sx, h / sy, score]
        d_rows, d_counts = to_tensor(rows), to_tensor(counts)
        jobs = [devs[b].rows_job(d_rows[b], d_counts[b:b + 1], start_conf, start_min_size, scales[b]) for b in range(B)]
        records = launch(jobs)
        for b in range(B):
            dets = rows[b, :counts[b]]
            if scales[b] != (1.0, 1.0):
                dets = YuNet.scale_rows(dets, *scales[b])
            tracks_in = []
            for d in dets:                                                   # RealtimeCall._track
                d = np.asarray(d, dtype=np.float32)
                if d[4] >= start_conf and max(d[2], d[3]) >= start_min_size:
                    tracks_in.append(STrack(d[:4], score=float(d[4])))
                else:
                    cut["conf" if d[4] < start_conf else "size"] += 1
            cut["empty"] += len(dets) == 0
            cut["kept"] += len(tracks_in)
            want = refs[b].update(tracks_in, (720, 1280), (720, 1280))
            got = devs[b].absorb(records[b])
            assert_same_frame(refs[b], devs[b], want, got, devs[b].state_dump(), (tick, b))
    assert cut["conf"] >= 10 and cut["size"] >= 10 and cut["empty"] >= 8 and cut["kept"] > 60, cut
