"""ByteTrack on the device: ``tracker.ByteTracker.update`` of many trackers in one launch (csrc/af_track_core.h).

    tr = DeviceByteTracker(args, frame_rate=30, device="cuda:0")
    online = tr.update(tracks_in, img_info, img_size)          # ByteTracker's call: a list of STrack, an (n, 5) array, or []
    records = update_calls([tr.rows_job(rows[b], counts[b:b + 1], start_conf, start_min_size), other.empty_job(), ...])
    online = tr.absorb(record_bytes)                           # after the records came back, whoever copied them

A tracker's state is one block of device memory that only the kernel reads and writes; what a caller sees - ``frame_id``,
``tracked_ids``, ``lost_ids``, ``removed_ids`` (``removed_stracks``' ids, in order and with its repeats) - is kept on the host
from the records.  ``update_calls`` enqueues one launch per 64 jobs on the current stream and returns the device tensor of their
records; it does not wait.  ``rows_job`` hands the kernel a detector's float32 rows where the detector left them, with
``RealtimeCall._track``'s start filter and ``YuNet.scale_rows``' scale-back done on the device.  ``host=True`` keeps the state in
host memory and runs the same source on the CPU (``af_bytetrack_update_host``): no GPU is needed.

The arithmetic is fp64 in one written-down order (tests/bytetrack_ref.py states it in numpy), so a device tracker equals that
statement bit for bit; it equals ``tracker.ByteTracker``, whose sums BLAS orders, in every discrete result and to round-off in the
boxes.  More than ``MAX_DETS`` detections in one frame, or more than ``MAX_TRACKS`` tracked and lost faces, raise RuntimeError.

``candidates=True``: the state block also holds the five-point cache, and ``update_live_calls`` runs the tracker and,
behind it in the same launch, ``live.track_candidates`` on the tracks it returned (csrc/af_live_core.h): ``live_job`` wraps a
tracker job with the frame index, the ring slot, the frame size, ``mesh_every``, ``crop_scale``, ``exclude_rect`` and the purged
tids; the launch leaves the tracker's record and one candidate record per job, ``parse_live_records`` reads the latter and
``candidates_of`` turns one into ``track_candidates``' tuple."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import AF_TRACK_FORM_ARRAY, AF_TRACK_FORM_EMPTY, AF_TRACK_FORM_LIST, AF_TRACK_FORM_LIST64, AF_TRACK_MAX_CALLS

MAX_TRACKS, MAX_DETS = _lib.AF_TRACK_MAX_TRACKS, _lib.AF_TRACK_MAX_DETS
_SLOTS = MAX_TRACKS + MAX_DETS
STATE_BYTES, RECORD_BYTES = int(_lib.lib.af_bytetrack_state_bytes()), int(_lib.lib.af_bytetrack_record_bytes())

_SLOT = np.dtype([("mean", "<f8", 8), ("cov", "<f8", (8, 8)), ("tlwh", "<f8", 4), ("score", "<f8"), ("id", "<i4"), ("state", "<i4"),
                  ("activated", "<i4"), ("frame_id", "<i4"), ("start_frame", "<i4"), ("tracklet_len", "<i4"), ("was_removed", "<i4"),
                  ("in_use", "<i4")])
_STATE = np.dtype([("magic", "<i4"), ("frame_id", "<i4"), ("count", "<i4"), ("n_tracked", "<i4"), ("n_lost", "<i4"),
                   ("max_time_lost", "<i4"), ("overflowed", "<i4"), ("reserved", "<i4"), ("track_thresh", "<f8"), ("match_thresh", "<f8"),
                   ("det_thresh", "<f8"), ("reserved2", "<f8"), ("tracked", "<i4", _SLOTS), ("lost", "<i4", _SLOTS), ("slot", _SLOT, _SLOTS)])
_ONLINE = np.dtype([("tlbr", "<f8", 4), ("score", "<f8"), ("id", "<i4"), ("state", "<i4"), ("activated", "<i4"), ("reserved", "<i4")])
_RECORD = np.dtype([("frame_id", "<i4"), ("overflow", "<i4"), ("n_online", "<i4"), ("n_tracked", "<i4"), ("n_lost", "<i4"),
                    ("n_removed", "<i4"), ("reserved", "<i4", 2), ("online", _ONLINE, MAX_TRACKS), ("tracked_ids", "<i4", MAX_TRACKS),
                    ("lost_ids", "<i4", MAX_TRACKS), ("removed_ids", "<i4", MAX_TRACKS)])
if _STATE.itemsize != STATE_BYTES or _RECORD.itemsize != RECORD_BYTES:
    raise ImportError("device_tracker: libafhip.so lays a tracker out in %d + %d bytes, this module in %d + %d"
                      % (STATE_BYTES, RECORD_BYTES, _STATE.itemsize, _RECORD.itemsize))

LIVE_STATE_BYTES, LIVE_RECORD_BYTES = int(_lib.lib.af_live_state_bytes()), int(_lib.lib.af_live_record_bytes())
LIVE_PER_LAUNCH = int(_lib.lib.af_live_calls_per_launch())
_LIVE_ENTRY = np.dtype([("tid", "<i4"), ("flags", "<i4"), ("tlbr", "<f4", 4), ("lm5", "<f4", (5, 2)), ("box", "<i4", 4), ("first_tile", "<i4"),
                        ("cand", "<i4")])
_LIVE_RECORD = np.dtype([("frame_idx", "<i4"), ("slot", "<i4"), ("n_online", "<i4"), ("n_cands", "<i4"), ("tiles", "<i4"), ("bad", "<i4"),
                         ("overflow", "<i4"), ("reserved", "<i4"), ("online", _LIVE_ENTRY, MAX_TRACKS)])
_LIVE_STATE = np.dtype([("trk", _STATE), ("cache_tid", "<i4", _SLOTS), ("cache_lm", "<f4", (_SLOTS, 10))])
if _LIVE_STATE.itemsize != LIVE_STATE_BYTES or _LIVE_RECORD.itemsize != LIVE_RECORD_BYTES:
    raise ImportError("device_tracker: libafhip.so lays a live call out in %d + %d bytes, this module in %d + %d"
                      % (LIVE_STATE_BYTES, LIVE_RECORD_BYTES, _LIVE_STATE.itemsize, _LIVE_RECORD.itemsize))

_OVERFLOW = {_lib.AF_TRACK_OVERFLOW_DETS: "more than AF_TRACK_MAX_DETS = %d detections passed the start filter in one frame" % MAX_DETS,
             _lib.AF_TRACK_OVERFLOW_TRACKS: "more than AF_TRACK_MAX_TRACKS = %d tracked and lost faces; reset() the tracker" % MAX_TRACKS,
             _lib.AF_TRACK_NOT_RESET: "the state block was never reset"}


class Track:
    """a returned track: ``track_id``, ``tlbr`` (fp64), ``score``, ``state``, ``is_activated``"""
    __slots__ = ("track_id", "tlbr", "score", "state", "is_activated")

    def __init__(self, track_id, tlbr, score, state, is_activated):
        self.track_id, self.tlbr, self.score, self.state, self.is_activated = track_id, tlbr, score, state, is_activated

    @property
    def tlwh(self):
        r = self.tlbr.copy()
        r[2:] -= r[:2]
        return r

    def __repr__(self):
        return "Track(%d)" % self.track_id


def _aligned_bytes(n: int) -> np.ndarray:
    return np.zeros((n + 7) // 8, dtype=np.float64).view(np.uint8)[:n]


class DeviceByteTracker:
    def __init__(self, args, frame_rate=30, device=None, host: bool = False, candidates: bool = False):
        self.args = args
        self.candidates = bool(candidates)                        # the state block carries the five-point cache (``live_job``)
        self.state_bytes = LIVE_STATE_BYTES if self.candidates else STATE_BYTES
        self.track_thresh, self.match_thresh = float(args.track_thresh), float(args.match_thresh)
        self.buffer_size = int(frame_rate / 30.0 * args.track_buffer)
        self.host = bool(host)
        if self.host:
            self.device, self._state = None, _aligned_bytes(self.state_bytes)
        else:
            import torch
            self.device = torch.device("cuda" if device is None else device)
            self._state = torch.empty(self.state_bytes, dtype=torch.uint8, device=self.device)
        self._record = _aligned_bytes(RECORD_BYTES)
        self._keep = None                                         # the uploaded rows of the last ``update``, alive until the next
        self.reset()

    def reset(self):
        """a fresh tracker: no track, ``frame_id`` 0, the next id 1"""
        fresh = self._state if self.host else _aligned_bytes(self.state_bytes)
        reset = _lib.lib.af_live_reset if self.candidates else _lib.lib.af_bytetrack_reset
        _lib.check(reset(C.c_void_p(fresh.ctypes.data), self.track_thresh, self.match_thresh, self.buffer_size),
                   "af_live_reset" if self.candidates else "af_bytetrack_reset")
        if not self.host:
            import torch
            self._state.copy_(torch.from_numpy(fresh))
        self.frame_id, self.tracked_ids, self.lost_ids, self.removed_ids, self.removed_now = 0, [], [], [], []

    state_ptr = property(lambda self: self._state.ctypes.data if self.host else self._state.data_ptr())

    # -- jobs -----------------------------------------------------------------------------------------------
    def _job(self, form, rows=0, count_ptr=0, count=0, max_rows=0, stride=5, img_info=(1, 1), img_size=(1, 1), start_conf=0.0,
             start_min_size=0.0, scale=(1.0, 1.0)) -> _lib.TrackCall:
        c = _lib.TrackCall()
        c.state, c.rows, c.count_ptr = self.state_ptr, rows or None, count_ptr or None
        c.count, c.max_rows, c.form, c.row_stride = int(count), int(max_rows), form, int(stride)
        c.img_info[0], c.img_info[1] = int(img_info[0]), int(img_info[1])
        c.img_size[0], c.img_size[1] = int(img_size[0]), int(img_size[1])
        # ``d[4] >= start_conf`` on a float32 row compares in float32 (a Python float is a weak scalar): the limits go down as float32
        c.start_conf, c.start_min_size = float(np.float32(start_conf)), float(np.float32(start_min_size))
        c.scale_x, c.scale_y = float(scale[0]), float(scale[1])
        return c

    def empty_job(self) -> _lib.TrackCall:
        """a frame without detections (``update([])``)"""
        return self._job(AF_TRACK_FORM_EMPTY)

    def rows_job(self, rows, count, start_conf: float, start_min_size: float, scale=(1.0, 1.0)) -> _lib.TrackCall:
        """a detector's rows read in place: ``rows`` an (N, >= 5) float32 device tensor (x, y, w, h, score, ...) whose rows are
        contiguous, ``count`` a one-element int32 device tensor (both must stay alive until the launch has run); the rows are scaled
        back by ``scale`` = (sx, sy) and filtered as ``RealtimeCall._track`` filters them"""
        if rows.dim() != 2 or rows.shape[1] < 5 or rows.stride(1) != 1 or str(rows.dtype) != "torch.float32":
            raise ValueError("device_tracker: rows must be (N, >= 5) float32 with contiguous rows, got %s %s" % (tuple(rows.shape), rows.dtype))
        if count.numel() != 1 or str(count.dtype) != "torch.int32":
            raise ValueError("device_tracker: count must be one int32 element")
        stride = rows.stride(0) if rows.shape[0] > 1 else rows.shape[1]
        return self._job(AF_TRACK_FORM_LIST, rows.data_ptr(), count.data_ptr(), 0, rows.shape[0], stride, start_conf=start_conf,
                         start_min_size=start_min_size, scale=scale)

    def live_job(self, job: _lib.TrackCall, frame_idx: int, slot: int, shape, mesh_every: int, crop_scale: float, exclude_rect, purged=(),
                 rows_floats: int = 0) -> _lib.LiveCall:
        """``job`` (``empty_job`` / ``rows_job`` of this tracker, made with ``candidates=True``) with what the candidate stage needs:
        the frame's index, its ring slot and (H, W, ...) ``shape``; ``purged``: the tids the call's books dropped on the step
        before - those the tracker's last record still names are sent, their cache entries go before the frame;
        ``rows_floats``: the float32 values readable behind the job's rows"""
        if not self.candidates:
            raise ValueError("device_tracker: live_job needs a tracker made with candidates=True")
        held = set(self.tracked_ids) | set(self.lost_ids)
        gone = [int(t) for t in purged if t in held][:MAX_TRACKS]
        c = _lib.LiveCall()
        c.track, c.rows_floats = job, int(rows_floats)
        c.frame_idx, c.slot, c.mesh_every = int(frame_idx), int(slot), int(mesh_every)
        c.frame_h, c.frame_w, c.n_purged = int(shape[0]), int(shape[1]), len(gone)
        c.crop_scale = float(crop_scale)
        for k in range(4):
            c.exclude[k] = float(exclude_rect[k])
        for k, tid in enumerate(gone):
            c.purged[k] = tid
        return c

    def live_rows_job(self, rows, count, start_conf: float, start_min_size: float, scale, **live) -> _lib.LiveCall:
        """``live_job`` over ``rows_job`` of a detector's (N, 15) float32 rows read in place"""
        floats = (rows.untyped_storage().nbytes() // 4 - rows.storage_offset()) if hasattr(rows, "untyped_storage") else rows.numel()
        return self.live_job(self.rows_job(rows, count, start_conf, start_min_size, scale), rows_floats=floats, **live)

    def cache_dump(self) -> dict:
        """the five-point cache, for tests: ``{tid: float32 (5, 2)}`` (waits for the device)"""
        raw = self._state if self.host else self._state.cpu().numpy()
        st = np.frombuffer(raw.tobytes(), dtype=_LIVE_STATE, count=1)[0]
        return {int(t): st["cache_lm"][i].reshape(5, 2).copy() for i, t in enumerate(st["cache_tid"]) if t != 0}

    def _input_job(self, tracks_in, img_info, img_size, to_memory):
        """``ByteTracker.update``'s ``tracks_in`` as a job; ``to_memory(numpy fp64 rows)`` -> (pointer, keep-alive)"""
        if isinstance(tracks_in, np.ndarray):
            if tracks_in.size == 0:
                return self.empty_job()
            rows = np.ascontiguousarray(tracks_in, dtype=np.float64).reshape(-1, 5)
            form = AF_TRACK_FORM_ARRAY
        else:
            if len(tracks_in) == 0:
                return self.empty_job()
            rows = np.array([[*np.asarray(d._tlwh if hasattr(d, "_tlwh") else d.tlwh, dtype=np.float64), float(d.score)]
                             for d in tracks_in], dtype=np.float64).reshape(-1, 5)
            form = AF_TRACK_FORM_LIST64
        ptr, self._keep = to_memory(rows)
        return self._job(form, ptr, 0, len(rows), len(rows), 5, img_info, img_size)

    # -- one tracker ----------------------------------------------------------------------------------------
    def update(self, tracks_in, img_info, img_size):
        """``ByteTracker.update``: the confirmed tracks of this frame (``Track``s, in the reference's order)"""
        if self.host:
            job = self._input_job(tracks_in, img_info, img_size, lambda rows: (rows.ctypes.data, rows))
            _lib.check(_lib.lib.af_bytetrack_update_host(C.byref(job), C.c_void_p(self._record.ctypes.data)), "af_bytetrack_update_host")
            return self.absorb(self._record)
        import torch

        def upload(rows):
            t = torch.from_numpy(rows).to(self.device)
            return t.data_ptr(), t
        with torch.cuda.device(self.device):
            job = self._input_job(tracks_in, img_info, img_size, upload)
            records = update_calls([job], self.device)
            return self.absorb(records[0].cpu().numpy())

    def absorb(self, record):
        """the host side of an update: ``record`` (RECORD_BYTES uint8, or a parsed one) -> the returned tracks; keeps the lists"""
        rec = record if isinstance(record, np.void) else np.frombuffer(np.ascontiguousarray(record).tobytes(), dtype=_RECORD, count=1)[0]
        code = int(rec["overflow"])
        if code:
            raise RuntimeError("device_tracker: %s" % _OVERFLOW.get(code, "overflow code %d" % code))
        self.frame_id = int(rec["frame_id"])
        self.tracked_ids = rec["tracked_ids"][:int(rec["n_tracked"])].tolist()
        self.lost_ids = rec["lost_ids"][:int(rec["n_lost"])].tolist()
        self.removed_now = rec["removed_ids"][:int(rec["n_removed"])].tolist()
        self.removed_ids += self.removed_now
        return [Track(int(o["id"]), o["tlbr"].copy(), float(o["score"]), int(o["state"]), bool(o["activated"]))
                for o in rec["online"][:int(rec["n_online"])]]

    def state_dump(self) -> dict:
        """the state block, for tests: ``{"frame_id", "count", "tracked": [slot records], "lost": [slot records]}`` (waits for the device)"""
        raw = self._state if self.host else self._state.cpu().numpy()
        st = np.frombuffer(raw.tobytes()[:STATE_BYTES], dtype=_STATE, count=1)[0]
        return {"frame_id": int(st["frame_id"]), "count": int(st["count"]),
                "tracked": [st["slot"][i] for i in st["tracked"][:int(st["n_tracked"])]],
                "lost": [st["slot"][i] for i in st["lost"][:int(st["n_lost"])]]}


def update_calls(jobs, device, records=None):
    """one launch per 64 ``jobs`` (``empty_job`` / ``rows_job`` of distinct trackers on ``device``) on the current stream; returns the
    (len(jobs), RECORD_BYTES) uint8 device tensor of their records - ``records`` itself when one is handed in - without waiting"""
    import torch
    n = len(jobs)
    if records is None:
        records = torch.empty(n, RECORD_BYTES, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        for lo in range(0, n, AF_TRACK_MAX_CALLS):
            chunk = jobs[lo:lo + AF_TRACK_MAX_CALLS]
            table = (_lib.TrackCall * len(chunk))(*chunk)
            _lib.check(_lib.lib.af_bytetrack_update_calls(table, len(chunk), C.c_void_p(records[lo].data_ptr()), stream),
                       "af_bytetrack_update_calls")
    return records


def parse_records(raw) -> np.ndarray:
    """(n, RECORD_BYTES) uint8 host bytes -> n parsed records for ``absorb``"""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=_RECORD)


def update_live_calls(jobs, device, track_records=None, records=None):
    """``af_live_update_calls`` per 64 ``jobs`` (``live_job``s of distinct trackers on ``device``) on the current stream: the tracker
    and the candidate stage of every job; returns the (len(jobs), RECORD_BYTES) and (len(jobs), LIVE_RECORD_BYTES) uint8 device
    tensors of the tracker's and the candidate records - the ones handed in, if any - without waiting.  ``live_launches(len(jobs))``
    kernels are enqueued."""
    import torch
    n = len(jobs)
    if track_records is None:
        track_records = torch.empty(n, RECORD_BYTES, dtype=torch.uint8, device=device)
    if records is None:
        records = torch.empty(n, LIVE_RECORD_BYTES, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        for lo in range(0, n, AF_TRACK_MAX_CALLS):
            chunk = jobs[lo:lo + AF_TRACK_MAX_CALLS]
            table = (_lib.LiveCall * len(chunk))(*chunk)
            _lib.check(_lib.lib.af_live_update_calls(table, len(chunk), C.c_void_p(track_records[lo].data_ptr()), C.c_void_p(records[lo].data_ptr()),
                                                     stream), "af_live_update_calls")
    return track_records, records


def live_launches(n_jobs: int) -> int:
    """the kernels ``update_live_calls`` enqueues for ``n_jobs`` jobs: the jobs of a launch travel in its arguments"""
    full, rest = divmod(n_jobs, AF_TRACK_MAX_CALLS)
    return full * -(-AF_TRACK_MAX_CALLS // LIVE_PER_LAUNCH) + -(-rest // LIVE_PER_LAUNCH)


def update_live_host(job, track_record=None, record=None):
    """one ``live_job`` of a ``host=True`` tracker through ``af_live_update_host``: -> (tracker record bytes, candidate record bytes)"""
    track_record = _aligned_bytes(RECORD_BYTES) if track_record is None else track_record
    record = _aligned_bytes(LIVE_RECORD_BYTES) if record is None else record
    _lib.check(_lib.lib.af_live_update_host(C.byref(job), C.c_void_p(track_record.ctypes.data), C.c_void_p(record.ctypes.data)), "af_live_update_host")
    return track_record, record


def parse_live_records(raw) -> np.ndarray:
    """(n, LIVE_RECORD_BYTES) uint8 host bytes -> n parsed candidate records"""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=_LIVE_RECORD)


def candidates_of(rec):
    """a parsed candidate record -> ``live.track_candidates``' tuple ``(rects, candidates, alive, kept_boxes)`` with the host's own
    types: tids and rectangle sides as Python ints, boxes float32 (4,), points float32 (5, 2), in the tracker's order"""
    code = int(rec["overflow"])
    if code:
        raise RuntimeError("device_tracker: %s" % _OVERFLOW.get(code, "overflow code %d" % code))
    kept_boxes, candidates, alive = {}, [], set()
    for e in rec["online"][:int(rec["n_online"])]:
        flags = int(e["flags"])
        if flags & _lib.AF_LIVE_EXCLUDED:
            continue
        tid, tlbr = int(e["tid"]), e["tlbr"].copy()
        kept_boxes[tid] = tlbr
        alive.add(tid)
        if flags & _lib.AF_LIVE_CANDIDATE:
            candidates.append((tid, tlbr, e["lm5"].copy(), tuple(int(v) for v in e["box"])))
    return [c[3] for c in candidates], candidates, alive, kept_boxes
