"""The sequences the device-tracker tests replay, and how two trackers are compared after a frame.

A sequence is ``(args, frames)``; a frame is ``(form, rows)`` with ``form`` "stracks" (rows x, y, w, h, score as float32: what
``RealtimeCall._track`` builds), "array" ((n, 5) fp64 tlbr + score) or "empty".  ``golden()`` is the reference's own recording;
the four scripts cover, between them, two faces crossing with IoU over 0.5, a face absent for longer than the buffer, alternate
empty frames (``detect_every = 2``), a one-frame detection that dies unconfirmed, low-score rows for the second association and
32 faces at once.  ``DENSE`` names the dense, contested sequences: seeded walks and packed crowds of overlapping faces (``dense``)
and three scripts built by hand; ``dense_stats`` counts what a sequence makes the statement do.  ``run_batch`` steps many device
trackers together, ``lone_run`` one alone."""
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


# ---- dense, contested sequences ----------------------------------------------------------------------------------------------------------
# What the scripts above never give the solver: an augmenting path that re-routes at more than 8 x 5, more detections than tracks, a
# tracked face dropped as the duplicate of a lost one, an id removed twice.  ``dense`` draws such frames from a seed; three scripts are
# built by hand with the statement in the loop.  ``dense_stats(name)`` counts, on the statement alone, what a sequence reached.
BANDS = ((0.60, 0.91, 0.99), (0.20, 0.15, 0.78), (0.12, 0.81, 0.89), (0.08, 0.01, 0.09))      # (probability, lowest, highest score)
ORIGIN = 60.0                                                    # the arena's top left corner


def _as_frame(form, rows):
    """rows (x, y, w, h, score) as a frame of ``form``"""
    if len(rows) == 0:
        return ("empty", np.zeros((0, 5)))
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    if form == "stracks":
        return ("stracks", r.astype(np.float32))
    return ("array", np.concatenate([r[:, :2], r[:, :2] + r[:, 2:4], r[:, 4:]], axis=1))


def dense(seed, faces, frames, arena, form, buffer, p_seen, p_dup, p_fp, p_empty):
    """``faces`` boxes of 70-130 px on a damped random walk (velocity += N(0, 1.5), then x 0.9) inside ``arena`` = (width, height),
    bouncing off its edges, so that they overlap all the time.  Per frame a face is detected with probability ``p_seen`` (jitter
    N(0, 2) on x, y, w, h; the score from ``BANDS``), with probability ``p_dup`` a second time (score 0.3-0.99); while a draw stays
    under ``p_fp`` a false positive is added anywhere (score 0.05-0.99); the rows are shuffled; with probability ``p_empty`` the
    frame is empty."""
    rng = np.random.default_rng(seed)
    span = np.asarray(arena, dtype=np.float64)
    size = rng.uniform(70.0, 130.0, (faces, 2))
    pos = rng.uniform(0.0, 1.0, (faces, 2)) * span               # the box's centre, relative to the arena's top left corner
    vel = np.zeros((faces, 2))
    chance = np.array([b[0] for b in BANDS])
    out = []
    for _ in range(frames):
        vel = (vel + rng.normal(0.0, 1.5, (faces, 2))) * 0.9
        pos = pos + vel
        for lim, beyond in ((0.0, pos < 0.0), (span, pos > span)):
            pos = np.where(beyond, 2.0 * lim - pos, pos)
            vel = np.where(beyond, -vel, vel)
        rows = []
        for i in range(faces):
            if rng.random() >= p_seen:
                continue
            _, lo, hi = BANDS[int(rng.choice(len(BANDS), p=chance))]
            box = np.concatenate([ORIGIN + pos[i] - 0.5 * size[i], size[i]])
            rows.append([*(box + rng.normal(0.0, 2.0, 4)), rng.uniform(lo, hi)])
            if rng.random() < p_dup:
                rows.append([*(box + rng.normal(0.0, 2.0, 4)), rng.uniform(0.3, 0.99)])
        while rng.random() < p_fp:
            rows.append([*(ORIGIN + rng.uniform(0.0, 1.0, 2) * span), *rng.uniform(70.0, 130.0, 2), rng.uniform(0.05, 0.99)])
        order = rng.permutation(len(rows))
        rows = [rows[k] for k in order]
        out.append(_as_frame(form, [] if rng.random() < p_empty else rows))
    return _args(track_buffer=buffer), out


def walk(seed, frames=60, form=None):
    """the seed's walk: 6 to 10 faces in 260 x 200 px, buffer 0, 2, 5 or 9; even seeds in the "stracks" form, odd ones as arrays"""
    return dense(seed, 6 + seed % 5, frames, (260, 200), form or ("stracks", "array")[seed % 2], (0, 2, 5, 9)[seed % 4],
                 p_seen=0.85, p_dup=0.15, p_fp=0.3, p_empty=0.05)


PACKED = ((100, 22, "stracks", 1), (101, 23, "array", 0), (102, 24, "stracks", 2))       # (seed, faces, form, buffer)


def packed(k):
    """a packed crowd of 30 frames: 22 to 24 faces in 700 x 450 px"""
    seed, faces, form, buffer = PACKED[k]
    return dense(seed, faces, 30, (700, 450), form, buffer, p_seen=0.93, p_dup=0.04, p_fp=0.15, p_empty=0.03)


class _Spy:
    """the statement's ``linear_assignment`` and ``_drop_duplicates`` wrapped while a script runs: what they were asked and answered"""

    def __init__(self):
        self.solved, self.dropped = [], []                        # (cost, n, m, thresh, matches); (tracked + lost, tracked dropped)

    def __enter__(self):
        import bytetrack_ref as ref
        self._ref, self._la, self._dd = ref, ref.linear_assignment, ref._drop_duplicates

        def la(cost, n, m, thresh):
            out = self._la(cost, n, m, thresh)
            self.solved.append(([list(r) for r in cost], n, m, thresh, list(out[0])))
            return out

        def dd(a, b):
            out = self._dd(a, b)
            self.dropped.append((len(a) + len(b), len(a) - len(out[0])))
            return out
        ref.linear_assignment, ref._drop_duplicates = la, dd
        return self

    def __exit__(self, *exc):
        self._ref.linear_assignment, self._ref._drop_duplicates = self._la, self._dd


def _det(x, y, w, h, score):
    return [float(x), float(y), float(w), float(h), float(score)]


def usurper():
    """buffer 30: face 1 moves right at 12 px per frame for 10 frames and is then no longer detected; from frame 10 on a face is
    detected 8 steps ahead of it, standing still.  The lost track coasts onto the younger tracked one, ``_drop_duplicates`` drops the
    TRACKED one, and the face is re-found under id 1."""
    import bytetrack_ref as ref
    args = _args(track_buffer=30)
    tr, frames, seen = ref.RefByteTracker(args, 30.0), [], {}
    with _Spy() as spy:
        for f in range(24):
            x = 100 + 12 * f if f < 10 else 100 + 12 * 9 + 12 * 8
            frames.append(_as_frame("stracks", [_det(x, 200, 80, 100, 0.95)]))
            tr.update(tracks_in(frames[-1]), SIZE, SIZE)
            seen[f] = ([t.track_id for t in tr.tracked_stracks], [t.track_id for t in tr.lost_stracks], spy.dropped[-1][1])
    assert seen[10][:2] == ([2], [1]), seen[10]
    assert seen[18] == ([], [1], 1), seen[18]                      # the tracked face is dropped as the duplicate of the lost one
    assert seen[19][0] == [1] and seen[23][:2] == ([1], []), (seen[19], seen[23])
    return args, frames


def back_at_once():
    """buffer 2: two lost faces pass ``max_time_lost`` and are removed, stay in the lost list for one call, are detected again on
    exactly that call and are re-found: their ids are in ``removed_ids`` although they are tracked.  The first is then lost on a
    frame with detections and leaves the lost list at once, without a second entry; the second is lost on a frame without any,
    stays lost for the buffer and is removed a second time: its id repeats in ``removed_ids``."""
    import bytetrack_ref as ref
    args = _args(track_buffer=2)
    tr, frames = ref.RefByteTracker(args, 30.0), []
    a, b, c = _det(100, 100, 100, 120, 0.95), _det(400, 150, 90, 110, 0.94), _det(700, 300, 110, 130, 0.93)

    def step(rows):
        frames.append(_as_frame("stracks", rows))
        tr.update(tracks_in(frames[-1]), SIZE, SIZE)
        return [t.track_id for t in tr.tracked_stracks], [t.track_id for t in tr.lost_stracks]
    for f in range(4):
        assert step([a, b, c]) == ([1, 2, 3], [])
    assert step([c]) == ([3], [1, 2]) and step([c]) == ([3], [1, 2])
    assert step([c]) == ([3], [1, 2]) and tr.removed_ids == [1, 2]               # past the buffer: removed, and lost for one more call
    tracked, lost = step([a, b, c])
    assert sorted(tracked) == [1, 2, 3] and lost == [] and tr.removed_ids == [1, 2]          # back on exactly that call, under their ids
    for f in range(2):
        step([a, b, c])
    tracked, lost = step([b, c])
    assert sorted(tracked) == [2, 3] and lost == [] and tr.removed_ids == [1, 2]             # lost among detections: it leaves at once
    tracked, lost = step([])
    assert tracked == [] and sorted(lost) == [2, 3]                              # lost on a frame without detections: it stays
    step([])
    tracked, lost = step([])
    assert (tracked, lost) == ([], []) and sorted(tr.removed_ids) == [1, 2, 2, 3]            # the id's repeat
    for f in range(2):
        step([a, c])
    assert [t.track_id for t in tr.tracked_stracks] == [4, 5]
    return args, frames


def twins():
    """two detections with identical boxes and scores on one track, for several frames: the two costs are exactly equal.  A third
    face is one frame old when two detections contest its unconfirmed association at 0.7."""
    import bytetrack_ref as ref
    args = _args(track_buffer=5)
    tr, frames = ref.RefByteTracker(args, 30.0), []
    equal = contested = 0
    with _Spy() as spy:
        for f in range(14):
            a = _det(100 + 2 * f, 100, 100, 120, 0.95)
            rows = [a, list(a)] if 3 <= f < 10 else [a]
            if f == 6:
                rows.append(_det(500, 300, 100, 120, 0.94))        # the third face
            if f == 7:
                rows += [_det(508, 300, 100, 120, 0.93), _det(494, 302, 100, 120, 0.92)]
            at = len(spy.solved)
            frames.append(_as_frame("stracks", rows))
            tr.update(tracks_in(frames[-1]), SIZE, SIZE)
            first, _, unconfirmed = spy.solved[at:at + 3]
            equal += any(len(set(r)) < len(r) and min(r) <= first[3] and r.count(min(r)) > 1 for r in first[0])
            contested += any(sum(c <= 0.7 for c in r) >= 2 for r in unconfirmed[0])
    assert equal >= 5 and contested >= 1, (equal, contested)
    return args, frames


HAND = {"usurper": usurper, "back_at_once": back_at_once, "twins": twins}
WALKS = tuple("walk%d" % s for s in range(8))
CROWDS = tuple("packed%d" % k for k in range(len(PACKED)))
DENSE = WALKS + CROWDS + tuple(HAND)
_dense = {}


def sequence(name):
    """``(args, frames, frame_rate)`` of "golden", a script or a name of ``DENSE``"""
    if name == "golden":
        args, frames, g = golden()
        return args, frames, g["frame_rate"]
    if name in DENSE:
        if name not in _dense:
            _dense[name] = walk(int(name[4:])) if name in WALKS else packed(int(name[6:])) if name in CROWDS else HAND[name]()
        return _dense[name][0], list(_dense[name][1]), 30.0
    args, frames = SCRIPTS[name]()
    return args, frames, 30.0


ALL = ("golden",) + tuple(SCRIPTS)


def _row_greedy(cost, n, m, thresh):
    """every row in turn takes its cheapest free column under the limit"""
    taken, out = set(), []
    for i in range(n):
        free = [j for j in range(m) if j not in taken and cost[i][j] <= thresh]
        if free:
            j = min(free, key=lambda j: cost[i][j])
            taken.add(j)
            out.append((i, j))
    return out


_stats = {}


def dense_stats(name):
    """what sequence ``name`` makes the statement do, from the statement alone: ``problems`` [(cost, n, m, thresh)] every
    association it solved with n, m > 0; of those ``non_greedy`` whose solution differs from row-greedy, ``n_lt_m``, ``n_gt_m``,
    ``largest`` (n, m) with the greatest min(n, m); ``refound`` tracks that went from the lost to the tracked list, ``repeated``
    ids more than once in ``removed_ids``, ``second_frames`` with a second-association match, ``tracked_dropped`` by
    ``_drop_duplicates``, ``held`` the most tracked + lost (in front of ``_drop_duplicates``), ``rows`` the most rows of a frame"""
    if name in _stats:
        return _stats[name]
    import bytetrack_ref as ref
    args, frames, rate = sequence(name)
    tr = ref.RefByteTracker(args, rate)
    s = dict(problems=[], non_greedy=0, n_lt_m=0, n_gt_m=0, largest=(0, 0), refound=0, repeated=0, second_frames=0, tracked_dropped=0,
             held=0, rows=0, frames=len(frames))
    with _Spy() as spy:
        for frame in frames:
            lost_before = {t.track_id for t in tr.lost_stracks}
            tr.update(tracks_in(frame), SIZE, SIZE)
            s["refound"] += len(lost_before & {t.track_id for t in tr.tracked_stracks})
            s["rows"] = max(s["rows"], len(frame[1]))
    s["second_frames"] = tr.second_matches
    s["repeated"] = sum(tr.removed_ids.count(t) > 1 for t in set(tr.removed_ids))
    s["held"], s["tracked_dropped"] = max(h for h, _ in spy.dropped), sum(d for _, d in spy.dropped)
    for cost, n, m, thresh, matches in spy.solved:
        if n == 0 or m == 0:
            continue
        s["problems"].append((cost, n, m, thresh))
        s["non_greedy"] += sorted(matches) != sorted(_row_greedy(cost, n, m, thresh))
        s["n_lt_m"] += n < m
        s["n_gt_m"] += n > m
        if min(n, m) > min(s["largest"]):
            s["largest"] = (n, m)
    _stats[name] = s
    return s


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


# ---- many device trackers stepped together -----------------------------------------------------------------------------------------------
def shifted(name, shift):
    """``sequence(name)`` with ``shift`` empty frames in front"""
    args, frames, rate = sequence(name)
    return args, [("empty", None)] * shift + list(frames), rate


def log_entry(tr, online):
    """what a ``DeviceByteTracker`` returned and kept after a frame, as plain values"""
    return ([(o.track_id, o.tlbr.tobytes(), o.score, o.state, o.is_activated) for o in online], tr.frame_id, list(tr.tracked_ids),
            list(tr.lost_ids), list(tr.removed_ids))


def lone_run(script):
    """``script`` = (args, frames, rate) on a lone device tracker: (the ``log_entry`` of every frame, the final state bytes)"""
    from af_mi355x import device_tracker as dt
    args, frames, rate = script
    tr, log = dt.DeviceByteTracker(args, rate, device="cuda"), []
    for frame in frames:
        log.append(log_entry(tr, tr.update(tracks_in(frame), SIZE, SIZE)))
    return log, tr._state.cpu().numpy().tobytes()


def run_batch(scripts, guard):
    """one device tracker per script = (args, frames, rate), stepped together by ``update_calls`` (one launch per 64 of them), with
    ``guard`` bytes of 0xA5 around every state block and around the records.  Returns the record bytes of every tick, the
    trackers, their ``log_entry`` per tick and the guarded buffers as host arrays."""
    import torch
    from af_mi355x import device_tracker as dt
    n, stride = len(scripts), dt.STATE_BYTES + guard
    states = torch.full((guard + n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    records = torch.full((2 * guard + n * dt.RECORD_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    rec_view = records[guard:guard + n * dt.RECORD_BYTES].view(n, dt.RECORD_BYTES)
    trackers = []
    for t, (args, frames, rate) in enumerate(scripts):
        tr = dt.DeviceByteTracker(args, rate, device="cuda")
        tr._state = states[guard + t * stride:guard + t * stride + dt.STATE_BYTES]
        tr.reset()
        trackers.append(tr)
    raw, logs = [], [[] for _ in range(n)]

    def upload(rows):
        dev = torch.from_numpy(rows).cuda()
        return dev.data_ptr(), dev
    for tick in range(max(len(s[1]) for s in scripts)):
        live_now = [t for t in range(n) if tick < len(scripts[t][1])]
        jobs = [trackers[t]._input_job(tracks_in(scripts[t][1][tick]), SIZE, SIZE, upload) for t in live_now]
        out = dt.update_calls(jobs, torch.device("cuda"), rec_view[:len(jobs)])
        host = out.cpu().numpy()
        raw.append(host.tobytes())
        for t, rec in zip(live_now, dt.parse_records(host)):
            logs[t].append(log_entry(trackers[t], trackers[t].absorb(rec)))
    return raw, trackers, logs, states.cpu().numpy(), records.cpu().numpy()
