"""The statement of the evaluator's chunk stage (csrc/af_runner_core.h): the loop lines of ``runner.VideoRunner.run`` between the
detection and the gate, with ``runner.track_stage`` driven by ``bytetrack_ref.RefByteTracker`` - the fixed-order fp64 tracker the
device core equals bit for bit.

``RefRun(args, shape, detect_every, budget_frames, fps).chunk(rows, frame_ids, first_slot)`` walks one chunk (``rows``: per frame
the (n, 15) float32 rows of the detector) and returns what the chunk record holds, as a dict; ``compare(rec, state, want, run)``
asserts that a parsed record and state block (``runner_device.parse_record`` / ``parse_state``) equal it, value for value.

The two caps are the core's, not the loop's: more than 32 rows past the filters refuse the frame before anything changed, more than
32 tracked + lost faces (counted where the core counts them, in front of ``_drop_duplicates``) refuse it behind the tracker."""
import types

import numpy as np

import bytetrack_ref
from af_mi355x import runner as R

NEED_DETECT, DROPPED, PROCESSED, NOT_REACHED, REFUSED = 1, 2, 4, 8, 16
OVERFLOW_DETS, OVERFLOW_TRACKS = 1, 2
MAX_TRACKS = MAX_DETS = 32


def tiles_of(w: int, h: int) -> int:
    return ((w + 31) // 32) * ((h + 7) // 8)


class RefRun:
    def __init__(self, args, shape, detect_every: int, budget_frames: int, fps: float):
        self.args, self.shape, self.detect_every, self.budget_frames = args, tuple(shape), int(detect_every), int(budget_frames)
        tracker = bytetrack_ref.RefByteTracker(types.SimpleNamespace(track_thresh=args.track_thresh, track_buffer=args.track_buffer,
                                                                     match_thresh=args.match_thresh, mot20=False), frame_rate=fps)
        self.st = R._RunState(tracker)
        self.started, self.consec, self.processed_after_start, self.stop = (not args.smart_start), 0, 0, False
        self.poisoned = False                      # behind a refusal by the tracker nothing of the state is compared

    def _update_counting(self, call):
        """``call()`` with the size of tracked + lost noted where the core checks it: in front of ``_drop_duplicates``"""
        seen, inner = [], bytetrack_ref._drop_duplicates

        def noting(a, b):
            seen.append(len(a) + len(b))
            return inner(a, b)
        bytetrack_ref._drop_duplicates = noting
        try:
            out = call()
        finally:
            bytetrack_ref._drop_duplicates = inner
        return out, seen[-1]

    def chunk(self, rows, frame_ids, first_slot: int) -> dict:
        a, st = self.args, self.st
        out = {"frames": [], "cands": [], "overflow": 0, "overflow_frame": 0, "tiles_half": 0, "tiles_full": 0}
        for j, k in enumerate(frame_ids):
            if self.stop:
                break
            need = (not self.started) or (k % self.detect_every == 0) or (st.tracker.tracked_stracks == [])
            dets = rows[j] if need else None
            flags = NEED_DETECT if need else 0
            if not self.started:
                self.consec = self.consec + 1 if (dets is not None and R.faces_valid(dets, a.start_conf, a.start_min_size)) else 0
                if self.consec >= a.start_after_n:
                    self.started = True
                out["frames"].append({"flags": flags | DROPPED, "n_rows": 0, "ids": []})
                continue
            if self.processed_after_start >= self.budget_frames:
                self.stop = True
                out["frames"] += [{"flags": NOT_REACHED, "n_rows": 0, "ids": []} for _ in frame_ids[j:]]
                break
            n_rows = 0
            if dets is not None and len(dets) > 0:
                n_rows = len(R.filter_detections(dets, self.shape[0], a.min_det_side, a.min_det_area, a.exclude_bottom_frac))
            if n_rows > MAX_DETS:
                out["overflow"], out["overflow_frame"] = OVERFLOW_DETS, j
                out["frames"].append({"flags": flags | REFUSED, "n_rows": 0, "ids": []})
                break
            self.processed_after_start += 1
            before = st.prev_ids
            cands, held = self._update_counting(lambda: R.track_stage(st, k, first_slot + j, self.shape, dets, a))
            if held > MAX_TRACKS:
                out["overflow"], out["overflow_frame"], self.poisoned = OVERFLOW_TRACKS, j, True
                out["frames"].append({"flags": flags | PROCESSED | REFUSED, "n_rows": n_rows, "ids": None})
                break
            ids = list(st.prev_ids) if st.prev_ids is not before else []       # track_stage makes a new list whenever a box passed
            out["frames"].append({"flags": flags | PROCESSED, "n_rows": n_rows, "ids": ids})
            by_id = {t.track_id: t for t in st.tracker.tracked_stracks}
            for c in cands:
                x1, y1, x2, y2 = c.rect
                w, h = x2 - x1, y2 - y1
                out["cands"].append({"frame_pos": j, "slot": c.slot, "tid": c.tid, "tlbr64": by_id[c.tid].tlbr.copy(),
                                     "lm5": np.asarray(st.last_lm[c.tid]["lm5"], dtype=np.float32).copy(), "box": [x1, y1, x2, y2],
                                     "record": c.record, "tile_half": out["tiles_half"], "tile_full": out["tiles_full"]})
                out["tiles_half"] += tiles_of(max(1, w // 2), max(1, h // 2))
                out["tiles_full"] += tiles_of(w, h)
        return out


def compare(rec, state, want, run: RefRun, n_frames: int):
    """a parsed record and state block against the statement's chunk ``want`` and its run ``run`` after that chunk"""
    head = rec["head"]
    assert (int(head["overflow"]), int(head["overflow_frame"])) == (want["overflow"], want["overflow_frame"])
    assert int(head["n_frames"]) == n_frames and int(head["bad"]) == 0
    assert len(want["frames"]) <= n_frames
    for j, fr in enumerate(want["frames"]):
        got = rec["frames"][j]
        assert int(got["flags"]) == fr["flags"], (j, int(got["flags"]), fr["flags"])
        if fr["ids"] is not None:
            assert int(got["n_rows"]) == fr["n_rows"] and got["ids"][:int(got["n_ids"])].tolist() == fr["ids"], j
    assert int(head["n_cands"]) == len(want["cands"])
    assert (int(head["tiles_half"]), int(head["tiles_full"])) == (want["tiles_half"], want["tiles_full"])
    for got, c in zip(rec["cands"], want["cands"]):
        assert (int(got["frame_pos"]), int(got["slot"]), int(got["tid"]), int(got["flags"])) == (c["frame_pos"], c["slot"], c["tid"], 0)
        assert np.array_equal(got["tlbr"], c["tlbr64"].astype(np.float32)) and np.array_equal(got["lm5"], c["lm5"])
        assert got["box"].tolist() == c["box"] and (int(got["tile_half"]), int(got["tile_full"])) == (c["tile_half"], c["tile_full"])
    if run.poisoned:
        return
    st = run.st
    assert (int(head["started"]), int(head["consec"]), int(head["processed_after_start"]), int(head["stop"])) == \
        (int(run.started), run.consec, run.processed_after_start, int(run.stop))
    assert (int(head["id_switches"]), int(head["frames_seen"])) == (st.id_switches, st.frames_seen)
    for key in ("started", "consec", "processed_after_start", "stop", "id_switches", "frames_seen"):
        assert int(state[key]) == int(head[key]), key
    n_prev = int(state["n_prev"])
    if st.prev_boxes is None:
        assert n_prev == 0
    else:
        assert np.array_equal(state["prev_boxes"][:n_prev], st.prev_boxes) and state["prev_ids"][:n_prev].tolist() == list(st.prev_ids)
    trk, tracker = state["trk"], st.tracker
    assert (int(trk["frame_id"]), int(trk["count"])) == (tracker.frame_id, tracker._count)
    for name, tracks in (("tracked", tracker.tracked_stracks), ("lost", tracker.lost_stracks)):
        slots = trk[name][:int(trk["n_" + name])].tolist()
        assert [int(trk["slot"][s]["id"]) for s in slots] == [t.track_id for t in tracks], name
        for s, t in zip(slots, tracks):
            assert trk["slot"][s]["mean"].tolist() == list(t.mean) and trk["slot"][s]["cov"].tolist() == [list(r) for r in t.covariance]
            tid = t.track_id                                   # the cache: the slot's entry is the track's, or there is none
            if tid in st.last_lm:
                assert int(state["cache_tid"][s]) == tid and np.array_equal(state["cache_lm"][s], np.asarray(st.last_lm[tid]["lm5"], np.float32))
            else:
                assert int(state["cache_tid"][s]) != tid
