"""The evaluator's chunk stage on the device: the host stage of ``runner.VideoRunner`` for all frames of a chunk in one launch
(csrc/af_runner_core.h, include/af_hip.h "chunk stage").

    plan = ChunkPlan(args, shape, detect_every, budget_frames, fps)       # the loop's parameters as the launch compares them
    state = plan.reset()                                                  # a fresh run: a host block; a device run is a copy of it
    record = track_chunk_host(plan, state, rows, counts, first_slot, frame_ids)      # the same source on the CPU
    rec = parse_record(record, len(frame_ids))                            # rec["head"], rec["frames"][j], rec["cands"][i]

``rows``: (n, max_rows, >= 15) float32, ``counts``: (n,) int32 - what a detector leaves for a chunk of n frames.  The launch itself
(``af_runner_track_chunk``) is enqueued by ``runner._DeviceSide.track_chunk`` on the detector's device tensors.  A refusal - more
than ``MAX_DETS`` rows past the detection filters in one frame, more than ``MAX_TRACKS`` tracked and lost faces - is a code in the
record's header; ``refusal(rec, frame_ids)`` turns it into the ``RuntimeError`` to raise."""
import ctypes as C

import numpy as np

from . import _lib
from .device_tracker import _STATE as _TRACKER_STATE
from .device_tracker import MAX_DETS, MAX_TRACKS, _aligned_bytes

MAX_FRAMES = _lib.AF_RUNNER_MAX_FRAMES
NEED_DETECT, DROPPED, PROCESSED, NOT_REACHED, REFUSED = (_lib.AF_RUNNER_NEED_DETECT, _lib.AF_RUNNER_DROPPED, _lib.AF_RUNNER_PROCESSED,
                                                          _lib.AF_RUNNER_NOT_REACHED, _lib.AF_RUNNER_REFUSED)
CAND_BAD = _lib.AF_RUNNER_CAND_BAD
_SLOTS = MAX_TRACKS + MAX_DETS
STATE_BYTES = int(_lib.lib.af_runner_state_bytes())

STATE = np.dtype([("trk", _TRACKER_STATE), ("magic", "<i4"), ("started", "<i4"), ("consec", "<i4"), ("processed_after_start", "<i4"),
                  ("stop", "<i4"), ("id_switches", "<i4"), ("frames_seen", "<i4"), ("n_prev", "<i4"), ("prev_boxes", "<f4", (MAX_TRACKS, 4)),
                  ("prev_ids", "<i4", MAX_TRACKS), ("cache_tid", "<i4", _SLOTS), ("cache_lm", "<f4", (_SLOTS, 5, 2))])
HEADER = np.dtype([(n, "<i4") for n in ("started", "consec", "processed_after_start", "stop", "id_switches", "frames_seen", "overflow",
                                        "overflow_frame", "n_cands", "tiles_half", "tiles_full", "bad", "n_frames")] + [("reserved", "<i4", 3)])
FRAME = np.dtype([("flags", "<i4"), ("n_rows", "<i4"), ("n_ids", "<i4"), ("reserved", "<i4"), ("ids", "<i4", MAX_TRACKS)])
CAND = np.dtype([("frame_pos", "<i4"), ("slot", "<i4"), ("tid", "<i4"), ("flags", "<i4"), ("tlbr", "<f4", 4), ("lm5", "<f4", (5, 2)),
                 ("box", "<i4", 4), ("tile_half", "<i4"), ("tile_full", "<i4")])
CANDS_OFFSET = HEADER.itemsize + MAX_FRAMES * FRAME.itemsize


def record_bytes(n_frames: int) -> int:
    """the bytes of the record of a chunk of `n_frames` frames"""
    return int(_lib.lib.af_runner_record_bytes(int(n_frames)))


def record_dtype(n_frames: int) -> np.dtype:
    return np.dtype([("head", HEADER), ("frames", FRAME, MAX_FRAMES), ("cands", CAND, int(n_frames) * MAX_TRACKS)])


if STATE.itemsize != STATE_BYTES or any(record_dtype(n).itemsize != record_bytes(n) for n in (1, MAX_FRAMES)):
    raise ImportError("runner_device: libafhip.so lays a run out in %d bytes and a record of %d frames in %d, this module in %d and %d"
                      % (STATE_BYTES, MAX_FRAMES, record_bytes(MAX_FRAMES), STATE.itemsize, record_dtype(MAX_FRAMES).itemsize))

_REFUSALS = {_lib.AF_TRACK_OVERFLOW_DETS: "more than AF_TRACK_MAX_DETS = %d detections passed the detection filters" % MAX_DETS,
             _lib.AF_TRACK_OVERFLOW_TRACKS: "more than AF_TRACK_MAX_TRACKS = %d tracked and lost faces" % MAX_TRACKS,
             _lib.AF_TRACK_NOT_RESET: "the run's state block was never reset"}


class ChunkPlan:
    """the loop's parameters as the chunk stage compares them: the detection filters and the start in float32 (a Python float
    against a float32 row compares in float32), ``min_track_side`` and ``crop_scale`` in fp64; ``args``: the runner's namespace"""

    def __init__(self, args, shape, detect_every: int, budget_frames: int, fps: float):
        f32 = lambda v: float(np.float32(v))
        self.frame_h, self.frame_w = int(shape[0]), int(shape[1])
        self.track_thresh, self.match_thresh = float(args.track_thresh), float(args.match_thresh)
        self.buffer_size = int(fps / 30.0 * args.track_buffer)
        self.started = not args.smart_start
        self.detect_every, self.start_after_n = int(detect_every), int(args.start_after_n)
        self.mesh_every, self.budget_frames = int(args.mesh_every), int(budget_frames)
        self.start_conf, self.start_min_size = f32(args.start_conf), f32(args.start_min_size)
        self.min_det_side = f32(args.min_det_side) if args.min_det_side > 0 else 0.0
        self.min_det_area = f32(args.min_det_area) if args.min_det_area and args.min_det_area > 0 else 0.0
        self.bottom_limit = 0.0
        if args.exclude_bottom_frac and args.exclude_bottom_frac > 0:
            self.bottom_limit = f32(self.frame_h * (1.0 - float(args.exclude_bottom_frac)))
            if not self.bottom_limit > 0.0:
                raise ValueError("runner: exclude_bottom_frac %r leaves no frame (tracker=\"device\")" % (args.exclude_bottom_frac,))
        self.min_track_side, self.crop_scale = float(args.min_track_side), float(args.crop_scale)

    def reset(self) -> np.ndarray:
        """a fresh run's state block (host bytes, 8-byte aligned)"""
        state = _aligned_bytes(STATE_BYTES)
        _lib.check(_lib.lib.af_runner_reset(C.c_void_p(state.ctypes.data), self.track_thresh, self.match_thresh, self.buffer_size,
                                            int(self.started)), "af_runner_reset")
        return state

    def chunk(self, state_ptr: int, rows_ptr: int, counts_ptr: int, record_ptr: int, rows_floats: int, max_rows: int, row_stride: int,
              first_slot: int, frame_ids) -> _lib.RunnerChunk:
        if not 1 <= len(frame_ids) <= MAX_FRAMES:
            raise ValueError("runner: a chunk of %d frames (1 to %d)" % (len(frame_ids), MAX_FRAMES))
        c = _lib.RunnerChunk()
        c.state, c.rows, c.counts, c.record, c.rows_floats = state_ptr, rows_ptr, counts_ptr, record_ptr, int(rows_floats)
        c.n_frames, c.max_rows, c.row_stride, c.first_slot = len(frame_ids), int(max_rows), int(row_stride), int(first_slot)
        c.frame_h, c.frame_w, c.detect_every, c.start_after_n = self.frame_h, self.frame_w, self.detect_every, self.start_after_n
        c.mesh_every, c.budget_frames = self.mesh_every, self.budget_frames
        c.start_conf, c.start_min_size, c.min_det_side, c.min_det_area = self.start_conf, self.start_min_size, self.min_det_side, self.min_det_area
        c.bottom_limit, c.min_track_side, c.crop_scale = self.bottom_limit, self.min_track_side, self.crop_scale
        for j, k in enumerate(frame_ids):
            c.frame_idx[j] = int(k)
        return c


def track_chunk_host(plan: ChunkPlan, state: np.ndarray, rows: np.ndarray, counts: np.ndarray, first_slot: int, frame_ids, record=None) -> np.ndarray:
    """``af_runner_track_chunk_host``: the chunk stage on the CPU.  ``state``: the run's host block (``plan.reset()``), advanced in
    place; ``rows`` (n, max_rows, >= 15) float32 and ``counts`` (n,) int32, C-contiguous; returns the record's bytes (``record``
    itself when one of ``record_bytes(n)`` 8-byte aligned bytes is handed in)"""
    n = len(frame_ids)
    if rows.dtype != np.float32 or rows.ndim != 3 or rows.shape[0] != n or not rows.flags.c_contiguous:
        raise ValueError("runner: rows must be C-contiguous (%d, max_rows, >= 15) float32, got %s %s" % (n, rows.shape, rows.dtype))
    if counts.dtype != np.int32 or counts.shape != (n,) or not counts.flags.c_contiguous:
        raise ValueError("runner: counts must be (%d,) int32" % n)
    if record is None:
        record = _aligned_bytes(record_bytes(n))
    c = plan.chunk(state.ctypes.data, rows.ctypes.data, counts.ctypes.data, record.ctypes.data, rows.size, rows.shape[1], rows.shape[2],
                   first_slot, frame_ids)
    _lib.check(_lib.lib.af_runner_track_chunk_host(C.byref(c)), "af_runner_track_chunk_host")
    return record


def parse_record(raw, n_frames: int) -> np.void:
    """the record's bytes (at least ``record_bytes(n_frames)`` of them) -> its parsed form"""
    dt = record_dtype(n_frames)
    return np.frombuffer(np.ascontiguousarray(raw).tobytes()[:dt.itemsize], dtype=dt, count=1)[0]


def parse_state(raw) -> np.void:
    """a run's state block, for tests"""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=STATE, count=1)[0]


def refusal(rec, frame_ids):
    """None, or the ``RuntimeError`` for the refusal the record's header carries"""
    code = int(rec["head"]["overflow"])
    if not code:
        return None
    j = int(rec["head"]["overflow_frame"])
    frame = frame_ids[j] if 0 <= j < len(frame_ids) else j
    return RuntimeError("runner: frame %d: %s" % (frame, _REFUSALS.get(code, "refusal code %d" % code)))
