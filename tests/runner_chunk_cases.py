"""Scripted videos for the evaluator's chunk stage, and the walk that feeds them to it chunk by chunk.

A case is ``Case(name, rows, reached, shape, fps, frame_ids, **args)``: ``rows[i]`` the detector's (n, 15) float32 rows of the i-th
kept frame, whose index in the video is ``frame_ids[i]`` (by default every frame is kept), ``reached(chunks, run)`` asserts - on the STATEMENT's chunks and run (tests/runner_chunk_ref.py) - that the script got to the
corner it was written for.  ``laid_out(rows, max_rows)`` puts a chunk's rows where a detector leaves them: (n, max_rows, 15) float32
with garbage behind the counts.  ``walk(case, size, step)`` cuts the frames into chunks of ``size`` and advances the frame-store slot as
``VideoRunner.run`` does.

Geometry to keep in mind: the loop hands ``STrack`` a tlbr box where it takes tlwh (runner.py:251), so the track of a detection
(x, y, w, h) has the box (x, y, 2x + w, 2y + h); only a face near the origin overlaps its own detection with IoU >= 0.4 and gets
YuNet's five points."""
import types

import numpy as np

from af_mi355x import runner as R
import runner_chunk_ref as ref

STD5 = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
F32 = np.float32


def row(x, y, w, h, score=0.95):
    """one YuNet row; the five points sit in the box, so they move with it"""
    x, y, w, h = (F32(v) for v in (x, y, w, h))
    lm = STD5 * [float(w), float(h)] + [float(x), float(y)]
    return np.concatenate([[x, y, w, h, F32(score)], lm.ravel()]).astype(np.float32)


def frame(*rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 15)


def under(v):
    """one float32 step under v"""
    return np.nextafter(F32(v), F32(-np.inf))


class Case:
    def __init__(self, name, rows, reached, shape=(480, 640, 3), fps=30.0, frame_ids=None, **args):
        self.name, self.rows, self.reached, self.shape, self.fps = name, rows, reached, tuple(shape), fps
        self.frame_ids = list(range(len(rows))) if frame_ids is None else list(frame_ids)
        self.args = types.SimpleNamespace(**dict(R.DEFAULTS, **dict(dict(detect_every=1, min_det_side=40, min_det_area=1600, min_track_side=50), **args)))
        self.detect_every = R.detect_rhythm(self.args.detect_every, R.sane_fps(fps))
        self.budget_frames = args.get("budget", 400)

    def ref_run(self):
        return ref.RefRun(self.args, self.shape, self.detect_every, self.budget_frames, self.fps)

    def plan(self):
        from af_mi355x import runner_device
        return runner_device.ChunkPlan(self.args, self.shape, self.detect_every, self.budget_frames, self.fps)


def laid_out(rows, max_rows, seed=0):
    rng = np.random.default_rng(seed)
    out = rng.uniform(-500.0, 1500.0, (len(rows), max_rows, 15)).astype(np.float32)          # garbage behind the counts
    counts = np.zeros(len(rows), dtype=np.int32)
    for j, r in enumerate(rows):
        out[j, :len(r)] = r
        counts[j] = len(r)
    return out, counts


def walk(case, size, step):
    """``step(rows of the chunk, frame ids, first slot) -> (any frame processed, stop)`` per chunk of ``size`` frames"""
    base = 0
    for lo in range(0, len(case.rows), size):
        ids = case.frame_ids[lo:lo + size]
        processed, stop = step(case.rows[lo:lo + size], ids, base)
        if processed:
            base += len(ids)
        if stop:
            break


def _frames(chunks):
    return [f for c in chunks for f in c["frames"]]


def _cands(chunks):
    return [c for ch in chunks for c in ch["cands"]]


# ---- the scripts -------------------------------------------------------------------------------------------------------------------------

def _filters():
    # H = 480, exclude_bottom_frac 0.10: the limit is float32(432); side 80, area 4000
    rows = frame(row(10, 10, 80, 60), row(110, 10, under(80), 60),                    # the longer side on the limit, and under it
                 row(210, 10, 50, 80), row(310, 10, 50, under(80)),                   # the area 4000, and under it
                 row(410, 392, 60, 80), row(510, under(392), 60, 80))                 # the centre on the bottom limit, and over it
    def reached(chunks, run):
        assert _frames(chunks)[0]["n_rows"] == 3 and all(f["n_rows"] == 3 for f in _frames(chunks)[1:])
    return Case("filters", [rows] * 3, reached, min_det_side=80, min_det_area=4000, exclude_bottom_frac=0.10)


def _start():
    good, weak, small = frame(row(10, 10, 20, 15, F32(0.6))), frame(row(10, 10, 100, 100, under(F32(0.6)))), frame(row(10, 10, under(20), 15, 0.9))
    face = [frame(row(10 + k, 10, 100, 100)) for k in range(8)]
    rows = [weak, good, good, small, good, good, good] + face        # the start completes on frame 6: in mid-chunk at 5 and at 16
    def reached(chunks, run):
        flags = [f["flags"] for f in _frames(chunks)]
        assert flags[:7] == [ref.NEED_DETECT | ref.DROPPED] * 7 and flags[7] & ref.PROCESSED and len(_cands(chunks)) >= 4
    return Case("start", rows, reached, smart_start=True, start_after_n=3, start_conf=0.6, start_min_size=20)


def _budget():
    rows = [frame(row(10 + k, 10, 100, 100)) for k in range(12)]
    def reached(chunks, run):
        flags = [f["flags"] for f in _frames(chunks)]
        assert sum(bool(f & ref.PROCESSED) for f in flags) == 7 and flags[7] == ref.NOT_REACHED
    return Case("budget", rows, reached, budget=7)


def _mesh():
    # a face that walks away from the origin until its track's box no longer overlaps its detection (no five points: the cache
    # serves a non-mesh frame, a mesh frame skips it), a face far from the origin (never any points), a face under min_track_side
    rows = [frame(row(10 + 5 * k, 10 + 5 * k, 100, 100), row(300, 200, 100, 90), row(2, 2, 40, 41)) for k in range(14)]
    def reached(chunks, run):
        cands, frames = _cands(chunks), _frames(chunks)
        assert all(len(f["ids"]) == 2 for f in frames[1:]) and all(c["tid"] == 1 for c in cands)       # the small one is no id, the far one no candidate
        at = [sum(len(ch["frames"]) for ch in chunks[:i]) + c["frame_pos"] for i, ch in enumerate(chunks) for c in ch["cands"]]
        stale = [k for k, c in zip(at, cands) if not np.array_equal(c["lm5"], rows[k][0, 5:].reshape(5, 2))]
        assert stale and all(k % 3 for k in stale)                   # the cache served non-mesh frames
        assert any(k % 3 == 0 and k not in at for k in range(min(stale), 14))          # and a mesh frame without points was skipped
    return Case("mesh", rows, reached, mesh_every=3, min_track_side=96)


def _switch():
    face = frame(row(10, 10, 100, 100))
    rows = [face, face, frame(), face, face, face]                   # track_buffer 0: the lost track is removed at once; the face comes back as id 2
    def reached(chunks, run):
        assert [c["tid"] for c in _cands(chunks)] == [1, 1, 2, 2] and run.st.id_switches == 1
    return Case("switch", rows, reached, track_buffer=0)


def _crop():
    # crop_scale 0.5 on boxes of odd width: .5 coordinates on both sides (half to even); a box that grows over all four edges
    rows = [frame(row(12 + k, 8, 70 + k, 71)) for k in range(6)] + [frame(row(5, 5, 420, 320))] * 3
    def reached(chunks, run):
        cands = _cands(chunks)
        halves = 0
        for c in cands:
            x0, y0, x1, y1 = np.rint(c["tlbr64"])
            for v in (x0 - 0.5 * (x1 - x0), x1 + 0.5 * (x1 - x0), y0 - 0.5 * (y1 - y0), y1 + 0.5 * (y1 - y0)):
                halves += (v % 1.0 == 0.5 and 0 < v < 479)
        assert halves >= 2 and any(c["box"] == [0, 0, 639, 479] for c in cands)
    return Case("crop", rows, reached, crop_scale=0.5, min_det_area=0)


def _sliver():
    rows = [frame(row(0, 0, 0.3, 100), row(200, 10, 100, 100))] * 3   # a box that rounds to no width: the empty crop
    def reached(chunks, run):
        assert all(f["ids"] == [1, 2] for f in _frames(chunks)) and not _cands(chunks)
    return Case("sliver", rows, reached, min_det_area=0)


def _grid(n, dx=0.0):
    return frame(*[row(4 + 110 * (i % 8) + dx, 4 + 100 * (i // 8), 60, 50, 0.9 + 0.001 * i) for i in range(n)])


def _many():
    rows = [_grid(32, 0.5 * k) for k in range(4)]
    def reached(chunks, run):
        assert all(f["n_rows"] == 32 for f in _frames(chunks)) and len(_frames(chunks)[0]["ids"]) == 32 and not any(c["overflow"] for c in chunks)
    return Case("many", rows, reached, shape=(720, 1280, 3), exclude_bottom_frac=0.0)


def _too_many_rows():
    rows = [_grid(8), _grid(33), _grid(8)]
    def reached(chunks, run):
        last = chunks[-1]
        assert last["overflow"] == ref.OVERFLOW_DETS and last["frames"][-1]["flags"] & ref.REFUSED and len(_frames(chunks)) == 2
    return Case("too_many_rows", rows, reached, shape=(720, 1280, 3), exclude_bottom_frac=0.0)


def _too_many_tracks():
    rows = [_grid(32), frame(row(900, 600, 60, 50)), _grid(4)]       # 32 tracks go lost, a new one comes: 33
    def reached(chunks, run):
        last = chunks[-1]
        assert last["overflow"] == ref.OVERFLOW_TRACKS and last["frames"][-1]["flags"] & ref.REFUSED and len(_frames(chunks)) == 2
    return Case("too_many_tracks", rows, reached, shape=(720, 1280, 3), exclude_bottom_frac=0.0)


def _dense(name, seed, **args):
    """a walk of tests/bytetrack_cases.py (40 frames of 6 to 10 faces that overlap all the time, with doubles, false positives and
    empty frames), moved to the origin - where a track's box still overlaps its own detection - and clamped there"""
    import bytetrack_cases
    _, walked = bytetrack_cases.walk(seed, frames=40, form="stracks")
    shift = bytetrack_cases.ORIGIN
    rows = [frame(*[row(max(x - shift, 0.0), max(y - shift, 0.0), w, h, s) for x, y, w, h, s in r.tolist()]) for _, r in walked]
    def reached(chunks, run):
        assert not any(c["overflow"] for c in chunks) and len(_frames(chunks)) == 40
        assert len(_cands(chunks)) >= 80 and run.st.id_switches >= 10 and max(len(f["ids"]) for f in _frames(chunks)) >= 6
    return Case(name, rows, reached, min_det_area=0, min_det_side=0, min_track_side=60, exclude_bottom_frac=0.0, **args)


def golden_case(name, run):
    """a run of tests/golden/runner_video.json as a case: the frames its window plan keeps, with the rows the file holds for them"""
    args = {k: v for k, v in run["args"].items() if k != "mot20"}
    fps = R.sane_fps(run["fps"])
    plan = R.WindowPlan(int(run["total_frames"]), int(args["clip_size"]), args["stride"], args["max_frame"], fps)
    kept = [i for i in range(run["n_frames"]) if plan.keep(i)]
    rows = [np.asarray(run["rows"][i], dtype=np.float32).reshape(-1, 15) for i in kept]
    case = Case("golden_" + name, rows, lambda chunks, ref_run: None, shape=run["frame_shape"], fps=fps, frame_ids=kept, **args)
    case.args = types.SimpleNamespace(**dict(R.DEFAULTS, **args))
    case.detect_every, case.budget_frames = R.detect_rhythm(case.args.detect_every, fps), plan.budget_frames
    return case


CASES = [_filters(), _start(), _budget(), _mesh(), _switch(), _crop(), _sliver(), _many(), _too_many_rows(), _too_many_tracks(),
         _dense("dense_walk4", 4, track_buffer=0, mesh_every=1), _dense("dense_walk3", 3, track_buffer=5, mesh_every=3)]
REFUSING = ("too_many_rows", "too_many_tracks")
