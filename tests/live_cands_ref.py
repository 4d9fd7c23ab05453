"""The statement of the live candidate stage (csrc/af_live_core.h) and the scripts its tests replay.

The statement is ``live.track_candidates`` itself, behind ``bytetrack_ref.RefByteTracker`` and ``RealtimeCall._track``'s start filter,
with ``RealtimeCall._after``'s purge of ``last_lm`` in front (``RefLive``).  ``expected`` turns what it returned on a frame into the
candidate record the launch must write, field for field.

A script is a list of frames; a frame is a dict: ``form`` ("list": float32 (n, 15) YuNet rows read in place, ``cap`` rows of
storage, the rest junk; "stracks" / "array" / "empty": a frame of tests/bytetrack_cases.py), ``rows``, ``scale`` (the detect-size
scale-back), ``shape``, ``idx`` (the frame index), ``mesh_every``, ``crop_scale``, ``exclude``, ``purged`` and the start filter.
The scripts are built with the statement in the loop, so that a frame can be placed exactly on an edge: each builder asserts that
the condition it is named for was reached.
"""
import copy

import numpy as np

import bytetrack_cases as cases
import bytetrack_ref as ref
from af_mi355x import _lib, live
from af_mi355x.detector import YuNet
from af_mi355x.evaluator import get_crop_box
from af_mi355x.tracker import STrack, iou_distance

EXCLUDE = (0.70, 0.70, 1.00, 1.00)
FAR = (2.0, 2.0, 3.0, 3.0)                                    # a self-view rectangle no centre reaches
STD5 = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
DEFAULTS = dict(form="list", rows=None, scale=(1.0, 1.0), shape=(96, 131), mesh_every=1, crop_scale=0.6, exclude=EXCLUDE, purged=(),
                start_conf=0.76, start_min_size=20, cap=None)


def tiles_of(box) -> int:
    """the 8 x 32 tiles of a crop rectangle's half-size image (csrc/af_quality.hip)"""
    w, h = max(1, (box[2] - box[0]) // 2), max(1, (box[3] - box[1]) // 2)
    return -(-w // 32) * -(-h // 8)


class RefLive:
    """one call: the statement's tracker, its ``CallState`` and the frame's ``track_candidates``"""

    def __init__(self, args, rate=30.0):
        self.tracker, self.state = ref.RefByteTracker(args, rate), live.CallState()

    def step(self, fr):
        """-> (online, found, before): the tracker's tracks, ``track_candidates``' tuple, the tids cached before the frame"""
        for tid in fr["purged"]:                                               # RealtimeCall._after, the step before
            self.state.last_lm.pop(tid, None)
        H, W = fr["shape"]
        dets, tracks_in = None, []
        if fr["form"] == "list":
            rows = np.asarray(fr["rows"], dtype=np.float32).reshape(-1, 15)
            dets = rows if tuple(fr["scale"]) == (1.0, 1.0) else YuNet.scale_rows(rows, *fr["scale"])      # RealtimeCall._detect
            for d in dets:                                                     # RealtimeCall._track
                d = np.asarray(d, dtype=np.float32)
                if d[4] >= fr["start_conf"] and max(d[2], d[3]) >= fr["start_min_size"]:
                    tracks_in.append(STrack(d[:4], score=float(d[4])))
            online = self.tracker.update(tracks_in, (H, W), (H, W))
        else:
            online = self.tracker.update(cases.tracks_in((fr["form"], fr["rows"])), cases.SIZE, cases.SIZE)
        before = set(self.state.last_lm)
        found = live.track_candidates(self.state, fr["idx"], (H, W), dets, online, fr["mesh_every"], fr["crop_scale"], fr["exclude"])
        return online, found, before


def expected(fr, online, found, before, state):
    """the candidate record of a frame: ``(header dict, [entry dict per returned track])``"""
    rects, candidates, alive, kept = found
    by_tid = {c[0]: c for c in candidates}
    H, W = fr["shape"]
    entries, tiles, n = [], 0, 0
    for tr in online:
        tid = tr.track_id
        e = dict(tid=tid, flags=0, tlbr=np.asarray(tr.tlbr).astype(np.float32), lm5=np.zeros((5, 2), np.float32), box=(0, 0, 0, 0),
                 first_tile=tiles, cand=-1)
        entries.append(e)
        if tid not in kept:
            e["flags"] = _lib.AF_LIVE_EXCLUDED
            continue
        assert tid in alive and np.array_equal(kept[tid], e["tlbr"]) and kept[tid].dtype == np.float32
        refreshed = tid in state.last_lm and state.last_lm[tid]["frame_idx"] == fr["idx"]
        if refreshed:
            e["flags"] |= _lib.AF_LIVE_REFRESHED
        if tid in by_tid:
            _, tlbr, lm5, box = by_tid[tid]
            e.update(flags=e["flags"] | _lib.AF_LIVE_CANDIDATE, lm5=lm5, box=box, cand=n)
            n += 1
            tiles += tiles_of(box)
        elif ((fr["idx"] % fr["mesh_every"]) == 0 or tid not in before) and not refreshed:
            e["flags"] |= _lib.AF_LIVE_NO_POINTS
        else:                                                                  # it had points: its crop box is empty
            box = tuple(int(v) for v in get_crop_box((H, W), e["tlbr"], scale=fr["crop_scale"]))
            assert box[2] <= box[0] or box[3] <= box[1]
            e.update(flags=e["flags"] | _lib.AF_LIVE_EMPTY_BOX, lm5=np.asarray(state.last_lm[tid]["lm5"], np.float32), box=box)
    assert [e["box"] for e in entries if e["cand"] >= 0] == rects
    return dict(frame_idx=fr["idx"], n_online=len(online), n_cands=n, tiles=tiles, bad=0, overflow=0), entries


def assert_record(rec, want, where):
    head, entries = want
    for key, v in head.items():
        assert int(rec[key]) == v, (where, key, int(rec[key]), v)
    for i, e in enumerate(entries):
        got = rec["online"][i]
        assert (int(got["tid"]), int(got["flags"]), int(got["first_tile"]), int(got["cand"])) == (e["tid"], e["flags"], e["first_tile"], e["cand"]), \
            (where, i, got, e)
        assert np.array_equal(got["tlbr"], e["tlbr"]) and np.array_equal(got["lm5"], e["lm5"]), (where, i, got, e)
        assert tuple(int(v) for v in got["box"]) == tuple(e["box"]), (where, i, got, e)
    assert not rec["online"][len(entries):].tobytes().strip(b"\0"), where      # the entries behind n_online are zero


def assert_found(got, want, where):
    """``device_tracker.candidates_of`` against ``track_candidates``' tuple: the same values with the same types"""
    assert got[0] == want[0] and all(type(v) is int for r in got[0] for v in r), where
    assert got[2] == want[2] and list(got[3]) == list(want[3]), where
    for tid in want[3]:
        assert got[3][tid].dtype == np.float32 and np.array_equal(got[3][tid], want[3][tid]), (where, tid)
    assert len(got[1]) == len(want[1]), where
    for a, b in zip(got[1], want[1]):
        assert a[0] == b[0] and a[3] == b[3] and type(a[0]) is int, where
        assert a[1].dtype == b[1].dtype == np.float32 and np.array_equal(a[1], b[1]), where
        assert a[2].dtype == b[2].dtype == np.float32 and a[2].shape == b[2].shape == (5, 2) and np.array_equal(a[2], b[2]), where


# ---- the frames ---------------------------------------------------------------------------------------------------------------------------
def face(x, y, w, h, score, lm=0.0):
    """a YuNet row: the box, the score and five points inside the box, shifted by ``lm`` pixels"""
    pts = STD5 * [w, h] + [x, y] + lm
    return np.concatenate([[x, y, w, h, score], pts.ravel()]).astype(np.float32)


class Builder:
    def __init__(self, args=None, **defaults):
        self.args = args if args is not None else cases._args()
        self.defaults = dict(DEFAULTS, **defaults)
        self.probe, self.frames = RefLive(self.args), []

    def _frame(self, rows, over):
        fr = dict(self.defaults, **over)
        fr["idx"] = over.get("idx", len(self.frames))
        if fr["form"] == "list":
            fr["rows"] = np.asarray(rows, dtype=np.float32).reshape(-1, 15)
        else:
            fr["rows"] = rows
        return fr

    def peek(self, rows=(), **over):
        """what the frame would give, without taking it"""
        return copy.deepcopy(self.probe).step(self._frame(rows, over))

    def add(self, rows=(), **over):
        fr = self._frame(rows, over)
        self.frames.append(fr)
        return self.probe.step(fr)


def _flags(b, out):
    """{tid: flags} of the frame just added"""
    online, found, before = out
    return {e["tid"]: e["flags"] for e in expected(b.frames[-1], online, found, before, b.probe.state)[1]}


def exclusion():
    """a centre exactly on each of the four edges of the self-view rectangle (excluded: both ends count), and one fp64 step
    outside (kept).  The frame is 64 x 128, so a normalised edge c / 128 times 128 is c again."""
    b = Builder(shape=(64, 128))
    H, W = 64, 128
    for f in range(3):
        b.add([face(40 + f, 12, 30, 34, 0.95)])
    f, seen = 3, []
    for edge in range(4):
        for outside in (False, True):
            rows = [face(40 + f, 12 + 0.5 * f, 30, 34, 0.95)]
            box = b.peek(rows, exclude=FAR)[0][0].tlbr
            cx, cy = 0.5 * (box[0] + box[2]), 0.5 * (box[1] + box[3])
            c, size = (cx, W) if edge % 2 == 0 else (cy, H)
            n = c / size
            assert n * size == c
            if outside:
                n = np.nextafter(n, np.inf if edge < 2 else -np.inf)
                assert (n * size > c) if edge < 2 else (n * size < c)
            rect = [0.0, 0.0, 1.0, 1.0]
            rect[edge] = float(n)
            flags = _flags(b, b.add(rows, exclude=tuple(rect)))
            assert bool(flags[1] & _lib.AF_LIVE_EXCLUDED) == (not outside), (edge, outside)
            seen.append((edge, outside))
            f += 1
    assert len(seen) == 8
    return b


def _det_box(row):
    r = np.asarray(row, dtype=np.float32)
    return np.array([[r[0], r[1], r[0] + r[2], r[1] + r[3]]], dtype=np.float32)


def _iou(box, row):
    """the pick's IoU of a track's box and a row, as track_candidates forms it"""
    return (1.0 - iou_distance(np.array([box], dtype=np.float32), _det_box(row))[0])[0]


def _on_the_limit(b):
    """-> (wide, row): the track's own detection, 3.7 times as wide as the track - the filter barely follows an aspect ratio, so
    its IoU with the updated box stays under 0.4 - and a row under start_conf, of the box's height and left edge and exactly 2 / 5
    of its width in the + 1 convention, whose IoU with the float32 box is therefore the double 0.4 itself.  Such a width is a
    float32 for one box in five; the detection's width is moved by quarter pixels until it is."""
    from fractions import Fraction
    for width in np.arange(110.0, 130.0, 0.25):
        wide = face(65 - width / 2, 20, width, 34, 0.95)
        online = b.peek([wide])[0]
        if len(online) != 1:
            continue
        box = online[0].tlbr.astype(np.float32)
        w = (Fraction(float(box[2])) - Fraction(float(box[0])) + 1) * 2 / 5 - 1
        if _iou(box, wide) < 0.4 and Fraction(float(np.float32(float(w)))) == w:
            return wide, face(box[0], box[1], np.float32(float(w)), box[3] - box[1], 0.5, lm=1.0)
    raise AssertionError("no detection width gives a box with a float32 two fifths")


def threshold():
    """the pick's limit: a row whose IoU with the track's float32 box IS the double 0.4 (taken: the limit counts), the same row with its right
    edge one float32 step further left (not taken: a mesh frame without points, skipped although the cache holds some); two rows of equal IoU
    (the first wins), both ways round."""
    b = Builder()
    for f in range(6):
        b.add([face(50, 20, 30, 34, 0.95)])
    for under in (False, True):
        wide, row = _on_the_limit(b)
        box = b.peek([wide])[0][0].tlbr.astype(np.float32)
        assert _iou(box, row) == 0.4 and _iou(box, wide) < 0.4
        if under:
            corner = row[0] + row[2]                                           # float32: the row's right edge, one step to the left
            while row[0] + row[2] == corner:
                row[2] = np.nextafter(row[2], np.float32(0))
            assert row[0] + row[2] == np.nextafter(corner, np.float32(0)) and 0.39999 < _iou(box, row) < 0.4
        online, found, before = out = b.add([wide, row])
        flags = _flags(b, out)
        assert 1 in before and len(online) == 1
        if under:
            assert flags[1] == _lib.AF_LIVE_NO_POINTS and not found[0]
        else:
            assert flags[1] & _lib.AF_LIVE_CANDIDATE and np.array_equal(found[1][0][2].ravel(), row[5:15])
        for f in range(2):
            b.add([face(50, 20, 30, 34, 0.95)])
    for first in (0, 1):                                                       # equal IoU: the first row wins
        own, twin = face(50, 20, 30, 34, 0.95), face(50, 20, 30, 34, 0.5, lm=2.0)
        rows = [twin, own] if first == 0 else [own, twin]
        online, found, before = b.add(rows)
        assert len(online) == 1 and np.array_equal(found[1][0][2].ravel(), rows[0][5:15]) and not np.array_equal(rows[0][5:15], rows[1][5:15])
    return b


def cache():
    """mesh_every = 4: non-mesh frames served by the cache; a new track on a non-mesh frame (refreshes); a frame without detection
    and a frame of no rows; a purge while the track is lost, then its return on a non-mesh frame (refreshes although the slot still
    holds its points); a purged tid the tracker does not hold"""
    b = Builder(mesh_every=4, shape=(96, 131))
    a = lambda f, lm=0.0: face(20 + f, 20, 30, 34, 0.95, lm=lm)
    c = lambda f, lm=0.0: face(80, 40 + 0.5 * f, 28, 32, 0.93, lm=lm)
    R, C = _lib.AF_LIVE_REFRESHED, _lib.AF_LIVE_CANDIDATE
    assert _flags(b, b.add([a(0)]))[1] == R | C                               # 0: a mesh frame
    for f in (1, 2):
        online, found, before = out = b.add([a(f, lm=3.0)])
        assert _flags(b, out)[1] == C and np.array_equal(found[1][0][2].ravel(), a(0)[5:15])     # the cache, not this frame's points
    b.add([a(3), c(3)])                                                        # 3: the second face, unconfirmed
    b.add([a(4), c(4)])                                                        # 4: a mesh frame: confirmed; both refresh
    assert _flags(b, b.add([a(5)], form="list"))[1] == C                       # 5: the second face is lost
    assert b.add(form="empty")[0] == []                                        # 6: no detection
    assert b.add([])[0] == []                                                  # 7: a detection without rows
    online, found, before = out = b.add([c(8), face(5, 60, 28, 30, 0.94)], purged=(1, 77))     # 8: a mesh frame; tid 1 purged while lost
    assert 1 in {t.track_id for t in b.probe.tracker.lost_stracks} and 1 not in b.probe.state.last_lm
    third = face(5, 60, 28, 30, 0.94)
    online, found, before = out = b.add([a(9, lm=5.0), c(9), third])           # 9: tid 1 is back on a non-mesh frame, uncached
    flags = _flags(b, out)
    assert flags[1] == R | C and 1 not in before and np.array_equal(b.probe.state.last_lm[1]["lm5"].ravel(), a(9, lm=5.0)[5:15])
    assert flags[3] == R | C and 3 not in before and flags[2] == C            #    and so is the third face, confirmed on this frame
    assert set(_flags(b, b.add([a(10, lm=1.0), c(10), third])).values()) == {C}                 # 10: everybody from the cache
    b.add([a(11), c(11)])
    return b


def edges():
    """a detect-size scale-back by (2.5, 1.5) of rows at odd integers - every scaled value ends in .5 - with crop_scale 0.5, so that
    get_crop_box rounds ties; a box clamped at all four edges; a box past the right edge whose crop is empty (alive, no candidate)"""
    b = Builder(scale=(2.5, 1.5), crop_scale=0.5, shape=(96, 131), start_min_size=10)
    small = lambda x, y, w, h, s, lm=0.0: face(x, y, w, h, s, lm=lm) / np.array([2.5, 1.5] * 7 + [1.0], dtype=np.float32)
    ties = 0
    for f in range(4):
        row = face(9 + 2 * f, 7, 13, 21, 0.95)
        row[5:15] = np.arange(5, 15) * 2 + 1
        dets = YuNet.scale_rows(row[None], 2.5, 1.5).astype(np.float32)
        assert all(float(v) % 1.0 == 0.5 for v in dets[0, [0, 1, 2, 3]]) and all(float(v) % 1.0 == 0.5 for v in dets[0, 5:14])
        online, found, before = b.add([row, small(-20, -15, 171, 126, 0.94)])
        ties += sum(float(v) % 1.0 == 0.5 for c in found[1] for v in c[1])
    assert (0, 0, 130, 95) in found[0] and ties >= 1
    for f in range(3):
        out = b.add([small(160, 30, 30, 34, 0.95), small(-20, -15, 171, 126, 0.94)])
    flags = _flags(b, out)
    assert _lib.AF_LIVE_EMPTY_BOX | _lib.AF_LIVE_REFRESHED in flags.values() and len(out[1][2]) == 2 and len(out[1][0]) == 1
    return b


def reuse():
    """buffer 2: a face leaves and is removed, the next face takes over its tracker slot on a non-mesh frame and must not be served
    the first one's points; a frame of 40 rows whose 38th carries the points"""
    b = Builder(args=cases._args(track_buffer=2), mesh_every=50)
    for f in range(3):
        b.add([face(20, 20, 30, 34, 0.95)])
    for f in range(4):
        b.add([])
    assert 1 in b.probe.tracker.removed_ids
    for f in range(3):
        out = b.add([face(70, 30, 30, 34, 0.95, lm=1.5)])
    assert _flags(b, out) == {2: _lib.AF_LIVE_CANDIDATE} and np.array_equal(b.probe.state.last_lm[2]["lm5"].ravel(), face(70, 30, 30, 34, 0.95, lm=1.5)[5:15])
    junk = [face(2 + (i % 7), 60 + (i % 5), 21, 22, 0.3, lm=float(i)) for i in range(37)]
    own, twin = face(70, 30, 30, 34, 0.95), face(70, 30, 30, 34, 0.5, lm=4.0)
    online, found, before = b.add(junk + [twin, own], idx=50)                  # a mesh frame: the points are row 37's
    assert len(b.frames[-1]["rows"]) == 39 and np.array_equal(found[1][0][2].ravel(), twin[5:15])
    return b


def _with_points(name):
    """a script of tests/bytetrack_cases.py: its "stracks" frames as YuNet rows read in place, with five points each"""
    args, frames, rate = cases.sequence(name)
    b = Builder(args=args, shape=cases.SIZE, start_conf=0.0, start_min_size=0.0, mesh_every=3)
    for form, rows in frames:
        if form == "stracks":
            b.add([np.concatenate([r[:5], (STD5 * r[2:4] + r[:2]).ravel()]) for r in np.asarray(rows, dtype=np.float32)])
        else:
            b.add(rows, form=form)
    return b


BUILDERS = {"exclusion": exclusion, "threshold": threshold, "cache": cache, "edges": edges, "reuse": reuse}
BUILDERS.update({name: (lambda name=name: _with_points(name)) for name in cases.ALL + cases.DENSE})
_built = {}


def script(name):
    """``(args, frames)`` of a script, built once"""
    if name not in _built:
        b = BUILDERS[name]()
        _built[name] = (b.args, b.frames)
    return _built[name]


ALL = tuple(BUILDERS)


def has_points(name) -> bool:
    """whether any frame of the script carries five points: not so a sequence of arrays"""
    return any(fr["form"] == "list" and len(fr["rows"]) for fr in script(name)[1])


# ---- a frame as a job of a DeviceByteTracker ---------------------------------------------------------------------------------------------
def job_of(tracker, fr, slot, to_tensor, keep):
    """the ``live_job`` of frame ``fr`` for ``tracker`` (made with ``candidates=True``); ``to_tensor(numpy)`` -> a tensor where the
    tracker reads; what must outlive the launch is appended to ``keep``"""
    extra = dict(frame_idx=fr["idx"], slot=slot, shape=fr["shape"], mesh_every=fr["mesh_every"], crop_scale=fr["crop_scale"],
                 exclude_rect=fr["exclude"], purged=fr["purged"])
    if fr["form"] == "list":
        n = len(fr["rows"])
        stored = np.full((n + 3, 15), 7.0e3, dtype=np.float32)                # what lies past the count is never read
        stored[:n] = fr["rows"]
        rows, count = to_tensor(stored), to_tensor(np.array([n], dtype=np.int32))
        keep += [rows, count]
        return tracker.live_rows_job(rows, count, fr["start_conf"], fr["start_min_size"], fr["scale"], **extra)
    if fr["form"] == "empty":
        return tracker.live_job(tracker.empty_job(), **extra)

    def to_memory(rows64):
        t = to_tensor(rows64)
        keep.append(t)
        return t.data_ptr(), t
    return tracker.live_job(tracker._input_job(cases.tracks_in((fr["form"], fr["rows"])), cases.SIZE, cases.SIZE, to_memory), **extra)
