"""The live call on the MI355X: captured frames and tracked faces in, a score per closed window out (``LiveCall``).

The reference's live path is ``RealtimeAF.step`` (test/af_realtime.py:372-509): detect, track, landmarks, then per tracked face a
crop cut on the host out of a channel-reversed copy of the frame (:434-438), a host list of crops per track (:450-460), and - when
a track holds ``clip_size`` frames and ``stride`` frames have passed since its last score (:462-465) - ``FasterCropAlignXRay`` over
the 32 host crops and ``infer_scores`` (:318-339).  ``LiveCall`` is that method behind the tracker: ``step`` copies the captured
frame ONCE into a device ring of the last ``ring_frames`` frames, a track keeps no pixels - per frame only ``(frame index, crop
rectangle, landmark record)`` - and all windows that close on a step are fitted on the host with the aligner's own arithmetic
(``aligner.fit_window``), warped in one launch out of rectangles of the resident frames
(``af_warp_affine_window_rects_bgr_u8`` for frames as they are captured, B, G, R; csrc/af_align.hip) and scored by one replay of a
HIP graph of ``forward_clips_u8`` at the batch size they pad to.  One score read-back per step is the only wait.

What stays with the caller: the detector and the tracker (``faces`` carry their track ids), the five landmarks per face (YuNet's,
or FaceMesh's as in :420-432; the 68 points are zeros as in :448 - the aligner fits on the five), the self-view exclusion
(:403), the Laplacian quality weight (:439-442: a face the caller rejects is simply not handed in that step) and everything
``_flush_and_infer`` does with a score after it exists (:340-358).  ``RealtimeCall`` further down is the caller that supplies all of
these: the captured frame is its only input.  ``CallServer`` at the end steps many such calls on launches they share (one YuNet
call per frame size, one quality launch, one warp and one replay per batch of closed windows, whichever calls they belong to).
There is no CPU fallback: without the HIP library the calls fail.
"""
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ._staging import is_crop
from .frames import ConvertedFrame, FrameResizer, StoreTable, upload_bytes
from .aligner import STD_POINTS_256
from .evaluator import (RECTS, RECTS_BGR, FrameStore, StoresWarp, WindowWarp, _clip_buffers, _fit, _FrameTrack, _network_device, _padded, get_crop_box,
                        partition)
from .tracker import ByteTracker, STrack, iou_distance

_FORMS = {"rgb": RECTS, "bgr": RECTS_BGR}


def _known_order(channel_order: str) -> str:
    if channel_order not in _FORMS:
        raise ValueError("live: channel_order 'bgr' or 'rgb', not %r" % (channel_order,))
    return channel_order


class _ClosedWindows:
    """The scoring loop of the windows that closed on a step, a call's own or a server's: ``max_batch`` clips - the static input
    of the replayed forwards -, the ``LiveScorer`` per batch size on the front of them (``scorers``, made on first use) and the
    pinned score buffer."""

    def __init__(self, network, clip_size: int, size: int, max_batch: int, device):
        self.network, self.clip_size, self.size, self.max_batch, self.device = network, clip_size, size, max_batch, device
        self.clip = _clip_buffers(1, max_batch, clip_size, size, device)[0]
        self.scorers = {}
        self._host = None

    def scorer(self, run: int):
        from .classifier import LiveScorer
        if run not in self.scorers:
            self.scorers[run] = LiveScorer(self.network, self.clip_size, self.size, batch=run, clip=self.clip[:run])
        return self.scorers[run]

    def __call__(self, n_windows: int, warp, before_wait=None, count=lambda key: None) -> np.ndarray:
        """the scores of `n_windows` windows, float32: per ``max_batch`` of them ``warp(first, n, run, clip)`` - which warps windows
        [first, first + n), the last one repeated up to `run`, into `clip` - and one replay; one read-back and one wait, in
        front of which ``before_wait(stream)`` is called.  ``count``: ``ServerStats.count``."""
        cur, parts = torch.cuda.current_stream(self.device), []
        for first, n, run in partition(n_windows, self.max_batch):
            scorer = self.scorer(run)
            warp(first, n, run, scorer.clip)
            count("warp")
            parts.append(scorer.replay()[:n].to(torch.float32, copy=True))         # the next replay of this size overwrites its scores
            count("replay")
        if self._host is None or self._host.numel() < n_windows:
            self._host = torch.empty(max(64, n_windows), dtype=torch.float32, pin_memory=True)
        self._host[:n_windows].copy_(parts[0] if len(parts) == 1 else torch.cat(parts), non_blocking=True)
        if before_wait is not None:
            before_wait(cur)
        cur.synchronize()
        count("wait")
        return self._host[:n_windows].numpy().copy()


class _DeviceSide(NamedTuple):
    """what a call keeps on the device for one frame size"""
    store: FrameStore                        # the last ``ring_frames`` frames, used as a ring
    warp: Optional[WindowWarp]               # the warp of the call's channel order out of it,
    scoring: Optional[_ClosedWindows]        # into the clip buffer of this (a served call has neither: its server has them)


class _TrackState:
    """af_realtime.py's ``cur_infos[tid]`` / ``_since_emit[tid]`` / ``missed[tid]``; an entry is ``(frame index, record)``"""
    __slots__ = ("entries", "since_emit", "missed")

    def __init__(self):
        self.entries, self.since_emit, self.missed = [], 0, 0


class LiveCall:
    """``LiveCall(network).step(frame, faces)`` -> ``[(tid, score), ...]`` for the windows that closed on this frame.

    ``network``: any of ``I3D8x8`` / ``FtcnTT8x8`` / ``SlowFast8x8`` on a HIP device in eval mode, or a ``Classifier`` around one, as
    for ``LiveScorer``.  ``frame``: the captured HxWx3 uint8 C-contiguous frame, B, G, R as ``cv2.VideoCapture`` delivers it
    (``channel_order="rgb"`` for R, G, B frames).  ``faces``: per tracked face of this frame ``(tid, tlbr float32[4], lm5
    float32[5, 2])`` in frame coordinates.  Behind the tracker the body of ``RealtimeAF.step`` becomes::

        call = LiveCall(network)                                       # once per call
        faces = [(t.track_id, t.tlbr, lm5_of(t)) for t in online]      # the caller's tracker, landmarks and quality gate
        results = call.step(frame_bgr, faces)                          # :401-509

    Bookkeeping, line for line the reference's (without its FaceMesh and quality lines): the crop is ``get_crop_box((H, W), tlbr,
    crop_scale)`` (:435), a degenerate box is skipped (:437), the record is ``(tlbr - corner, lm5 - corner, zeros(68, 2), crop
    box)`` (:445-450), a track keeps its last ``clip_size`` entries (:457-460), a window closes when the track holds ``clip_size``
    frames and ``since_emit >= stride`` (:462-465), a scored track keeps ``entries[-keep_tail:]`` with ``keep_tail = max(0,
    clip_size - stride)`` - for ``keep_tail == 0`` that slice keeps everything, as the reference does (:475-479) - and a track not
    seen for ``drop_after`` steps is purged (:483-499; ``purged`` lists the tids the last step dropped).

    The frame ring.  Frame k sits in slot ``k % ring_frames`` of a device ring (``frame_view(k)`` is its device (H, W, 3) view, for
    a detector that reads it there); it arrives through a pinned staging slot, one H2D copy per step, whatever the number of faces.
    ``ring_frames`` must be at least ``clip_size + drop_after``: a track seen on consecutive steps and then missed for up to
    ``drop_after - 1`` names no frame older than that.  The defaults keep the reference's ``drop_after = 90`` and take a ring of 128
    frames (354 MB at 720p).  A track that comes and goes more than once, or whose boxes are degenerate for a while, can still hold
    an entry that has left the ring; where the reference would go on holding that crop on the host, ``step`` drops such entries
    from the front of the track, so its next window closes later and never reads an overwritten frame.  A change of the frame
    size mid-call re-opens the ring for the new size and drops the entries of all tracks (their counters stay).

    Window close.  The windows that closed on a step go, ``max_batch`` at a time, through ONE warp launch into the static clip
    buffer and ONE replay of the HIP graph recorded (``LiveScorer``, on first use of a batch size) from ``forward_clips_u8(...,
    return_scores=True)`` at the next of 1, 2, 4 ... ``max_batch`` clips; a short batch is padded by repeating its last window.
    The scores are ``infer_scores``' values at that batch size, bit for bit.  A window whose crops do not fit their canvas raises
    the aligner's ``ValueError`` (the bookkeeping of the step is complete by then).

    Streams.  Every step waits, on the stream that is current when it is called, for the event the step before recorded behind
    its last launch: a ring slot or the clip buffer is rewritten only after the warp that may read it, and a warp reads a frame
    only after its upload, whichever streams the steps were called on.  A pinned staging slot is refilled only after the copy
    that last left it (an event per slot).  ``uploaded_bytes`` counts the frame bytes sent to the device."""

    def __init__(self, network, clip_size: int = 32, size: int = 224, stride: int = 52, crop_scale: float = 0.6, ring_frames: int = 128,
                 max_batch: int = 16, drop_after: int = 90, channel_order: str = "bgr"):
        self.network = getattr(network, "network", network)
        self.clip_size, self.size, self.stride = int(clip_size), int(size), int(stride)
        self.crop_scale, self.ring_frames = float(crop_scale), int(ring_frames)
        self.max_batch, self.drop_after = int(max_batch), int(drop_after)
        self.channel_order = _known_order(channel_order)
        if self.clip_size < 1 or self.stride < 1 or self.drop_after < 1:
            raise ValueError("live: clip_size, stride and drop_after are at least 1")
        if self.ring_frames < self.clip_size + self.drop_after:
            raise ValueError("live: ring_frames %d is less than clip_size + drop_after = %d: a window could name an overwritten frame"
                             % (self.ring_frames, self.clip_size + self.drop_after))
        self.frame_idx = -1
        self.purged: List = []
        self.uploaded_bytes = 0
        self._tracks = {}                  # tid -> _TrackState
        self._shape = None
        self._first = 0                    # the oldest frame index the ring may hold (moved by a re-open)
        self._ring: Optional[_DeviceSide] = None     # for the current frame size
        self._done = None                  # recorded behind the last launch of every step

    # clips per forward -> LiveScorer on the front of the ring's clip buffer
    _scorers = property(lambda self: self._ring.scoring.scorers if self._ring is not None and self._ring.scoring is not None else {})

    # -- the host side: af_realtime.py:401-505 ---------------------------------------------------------
    def step(self, frame: np.ndarray, faces: Sequence[Tuple], alive: Sequence = ()) -> List[Tuple]:
        self.admit(frame)
        return self.advance(faces, alive)

    def admit(self, frame: np.ndarray) -> int:
        """the first half of ``step``: the captured frame goes into the ring, once (:373-376); returns its index.  Between
        ``admit`` and ``advance`` a caller may read the frame where it now lies (``frame_view``): a detector, the quality gate."""
        k = self.admit_books(frame)
        self._store_frame(frame, k % self.ring_frames)
        return k

    def admit_books(self, frame) -> int:
        """``admit`` without the pixels: checks the frame, counts it and re-opens the ring when its size has changed; returns its
        index.  The caller then moves the pixels into ring slot ``index % ring_frames`` (``CallServer`` does, for all its calls'
        converted frames - ``YuvFrame``s, ``CapturedFrame``s - at once)."""
        if not isinstance(frame, ConvertedFrame) and (not is_crop(frame) or not frame.flags.c_contiguous):
            raise AssertionError("live: a frame must be a C-contiguous HxWx3 uint8 numpy array, a YuvFrame or a CapturedFrame")
        self.frame_idx += 1
        if self._shape != tuple(frame.shape):
            self._open_ring(frame.shape)
        return self.frame_idx

    def advance(self, faces: Sequence[Tuple], alive: Sequence = ()) -> List[Tuple]:
        """the second half of ``step``: the tracks move on by the faces of the admitted frame (:401-499).  ``alive``: tids that
        were tracked on this frame but contribute no entry - no landmarks, or rejected by the quality gate (:407 against :431-442):
        their ``missed`` count resets as for a face that was handed in, and nothing else happens to them."""
        ready = self.advance_host(faces, alive)
        if not ready:
            return []
        scores = self._score(ready)                                                    # :472
        return [(tid, float(s)) for (tid, _), s in zip(ready, scores)]

    def advance_host(self, faces: Sequence[Tuple], alive: Sequence = ()) -> List[Tuple]:
        """the books of ``advance`` without the scoring: returns the windows that closed on this frame, ``[(tid, [(frame index,
        record)] * clip_size)]``.  ``advance`` scores them itself; ``CallServer`` scores the windows of many calls together."""
        H, W = self._shape[:2]
        oldest = self._oldest()
        alive, ready = set(alive), []
        for tid in alive:                                                              # :409-411
            if tid not in self._tracks:
                self._tracks[tid] = _TrackState()
        for tid, tlbr, lm5 in faces:
            tlbr = np.asarray(tlbr, dtype=np.float32).reshape(4)
            alive.add(tid)                                                             # :407
            tr = self._tracks.get(tid)
            if tr is None:                                                             # :409-411
                tr = self._tracks[tid] = _TrackState()
            x1, y1, x2, y2 = map(int, get_crop_box((H, W), tlbr, scale=self.crop_scale))    # :435-436
            if x2 <= x1 or y2 <= y1:                                                   # :437
                continue
            top_left = np.array([[x1, y1]], dtype=np.float32)                         # :445-450
            record = ((tlbr.reshape(2, 2) - top_left).reshape(-1), np.asarray(lm5, dtype=np.float32).reshape(5, 2) - top_left,
                      np.zeros((68, 2), np.float32), np.array([x1, y1, x2, y2], dtype=np.int32))
            tr.entries.append((self.frame_idx, record))
            tr.since_emit += 1                                                         # :453
            if tr.entries[0][0] < oldest:                                              # not the reference's: entries that left the ring
                tr.entries = [e for e in tr.entries if e[0] >= oldest]
            if len(tr.entries) > self.clip_size:                                       # :457-460
                tr.entries = tr.entries[-self.clip_size:]
            if len(tr.entries) == self.clip_size and tr.since_emit >= self.stride:     # :462-465
                tr.since_emit = 0
                ready.append((tid, list(tr.entries)))
        keep_tail = max(0, self.clip_size - self.stride)                               # :475-479
        for tid, _ in ready:
            self._tracks[tid].entries = self._tracks[tid].entries[-keep_tail:]
        self.purged = []
        for tid in list(self._tracks):                                                 # :483-499
            tr = self._tracks[tid]
            if tid in alive:
                tr.missed = 0
            else:
                tr.missed += 1
                if tr.missed >= self.drop_after:
                    del self._tracks[tid]
                    self.purged.append(tid)
        return ready

    def frame_view(self, k: int) -> torch.Tensor:
        """the device (H, W, 3) uint8 view of frame ``k`` (``call.frame_idx`` is the last one), in the channel order it was captured
        in; valid on the stream ``step`` was called on until ``ring_frames`` more frames have arrived"""
        k = int(k)
        if self._ring is None or not self._oldest() <= k <= self.frame_idx:
            raise ValueError("live: frame %d is not resident (frames %d .. %d are)" % (k, self._oldest(), self.frame_idx))
        return self._ring.store.view(k % self.ring_frames)

    def _oldest(self) -> int:
        """the oldest frame index the ring still holds"""
        return max(self._first, self.frame_idx - self.ring_frames + 1)

    # -- the device side ---------------------------------------------------------------------------------
    def _open_ring(self, shape):
        """a ring for frames of `shape`; the entries of all tracks name frames of the old one and are dropped"""
        if self._ring is not None:
            torch.cuda.synchronize(self._ring.store.device)                            # nothing still reads the old ring or clip buffer
        self._ring = None                                                              # the old buffers go before the new ones come
        self._ring = self._new_ring(shape)
        self._shape, self._first = tuple(shape), self.frame_idx
        for tr in self._tracks.values():
            tr.entries = []

    def _new_ring(self, shape):
        dev = _network_device(self.network)
        with torch.cuda.device(dev):
            store = FrameStore(dev, self.channel_order)
            store.open(shape, self.ring_frames)
            warp = WindowWarp(_FORMS[self.channel_order], store, self.clip_size, self.size, self.max_batch)
            return _DeviceSide(store, warp, _ClosedWindows(self.network, self.clip_size, self.size, self.max_batch, dev))

    def _store_frame(self, frame: np.ndarray, slot: int):
        """host frame -> a pinned staging slot -> ring slot `slot`, asynchronous on the current stream"""
        ring = self._ring.store
        with torch.cuda.device(ring.device):
            cur = torch.cuda.current_stream(ring.device)
            if self._done is None:
                self._done = torch.cuda.Event()
            else:
                cur.wait_event(self._done)
            ring.put([frame], slot)
            self._done.record(cur)
        self.uploaded_bytes += upload_bytes(frame)

    def _score(self, ready) -> np.ndarray:
        """``ready``: ``[(tid, [(frame index, record)] * clip_size)]`` -> their scores, float32: one fit per window, one launch and
        one replay per ``max_batch`` windows, one read-back"""
        ring, T = self._ring, self.clip_size
        std_points = STD_POINTS_256 * self.size / 256.0
        entries = [e for _, win in ready for e in win]
        track = _FrameTrack([rec for _, rec in entries], [k % self.ring_frames for k, _ in entries], self._shape)
        windows = [list(range(w * T, (w + 1) * T)) for w in range(len(ready))]

        def warp(first, n, run, clip):
            ids, fits = _padded(track, windows, first, n, run, std_points)
            ring.warp(track, [windows[k] for k in ids], track.frame, 0, clip, fits)
        with torch.cuda.device(ring.store.device):
            return ring.scoring(len(windows), warp, before_wait=self._done.record)


# ---- the quality gate: af_realtime.py:262-276 -------------------------------------------------------------------------------------

def quality_weight(min_side: float, lap: float, q_weighting: bool = True, q_min_size_soft: int = 64, q_min_size_hard: int = 32,
                   q_lap_soft: float = 20.0, q_lap_hard: float = 5.0) -> float:
    """the weight ``_frame_quality_weight`` gives a crop whose shorter side is ``min_side`` and whose half-size Laplacian variance
    is ``lap`` (:268-276): 0 under either hard limit, else 1 or the product of the two ramps between the hard and soft limits"""
    if min_side < q_min_size_hard or lap < q_lap_hard:
        return 0.0
    if not q_weighting:
        return 1.0
    size_w = 1.0 if min_side >= q_min_size_soft else max(0.0, (min_side - q_min_size_hard) / max(1.0, (q_min_size_soft - q_min_size_hard)))
    lap_w = 1.0 if lap >= q_lap_soft else max(0.0, (lap - q_lap_hard) / max(1e-6, (q_lap_soft - q_lap_hard)))
    return float(size_w * lap_w)


_SUMS_DTYPE = np.dtype([("s1", "<i8"), ("s2", "<i8"), ("n_px", "<i4"), ("r", "<i4")])          # af_quality_sums


class _QualitySums:
    """what both forms of the quality launch share: the device and pinned records, one launch per 64 rectangles, one pinned
    read-back on the current stream - the only wait - and the lap each rectangle's three integers give.  ``launches`` counts the
    calls into the C function."""

    def __init__(self, device):
        self.device, self.launches = device, 0
        self._dev = self._host = None

    def _sums(self, sizes, grey: bool, launch, what: str, full: bool = False, both: bool = False):
        """``sizes``: (h, w) per rectangle; ``launch(lo, hi, sums, grey, grey_bytes, stream, full)`` calls the C function for
        rectangles [lo, hi) -> ``[(n_px, S1, S2)]`` as Python integers (and, with ``grey``, the list of (dh, dw) uint8 grey images;
        ``full``: the measured images are the rectangles themselves, (h, w)).  ``both`` (without ``grey``): the half-size launches,
        then the full-size ones, and ONE read-back -> the two lists."""
        import ctypes as C
        from . import _lib
        n = len(sizes)
        if n == 0:
            return ([], []) if grey or both else []
        passes = (False, True) if both else (bool(full),)
        halves = [(h, w) if full else (max(1, h // 2), max(1, w // 2)) for h, w in sizes]
        rec, total = C.sizeof(_lib.QualitySums), n * len(passes)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._dev is None or self._dev.numel() < total * rec:
                with torch.inference_mode(False):
                    self._dev = torch.empty(max(total, _lib.QUALITY_MAX_RECTS) * rec, dtype=torch.uint8, device=self.device)
                    self._host = torch.empty(self._dev.numel(), dtype=torch.uint8, pin_memory=True)
            gbuf = torch.empty(sum(h * w for h, w in halves), dtype=torch.uint8, device=self.device) if grey else None
            goff = 0
            for p, mode in enumerate(passes):
                for lo in range(0, n, _lib.QUALITY_MAX_RECTS):             # one launch for up to 64 faces
                    hi = min(n, lo + _lib.QUALITY_MAX_RECTS)
                    gn = sum(h * w for h, w in halves[lo:hi]) if grey else 0
                    _lib.check(launch(lo, hi, C.c_void_p(self._dev.data_ptr() + (p * n + lo) * rec),
                                      C.c_void_p(gbuf.data_ptr() + goff if grey else None), gn, C.c_void_p(cur.cuda_stream), mode), what)
                    self.launches += 1
                    goff += gn
            self._host[:total * rec].copy_(self._dev[:total * rec], non_blocking=True)
            cur.synchronize()
            raw = np.frombuffer(self._host.numpy()[:total * rec].tobytes(), dtype=_SUMS_DTYPE)
            out = [(int(r["n_px"]), int(r["s1"]), int(r["s2"])) for r in raw]
            if both:
                return out[:n], out[n:]
            if not grey:
                return out
            flat, images, off = gbuf.cpu().numpy(), [], 0
            for h, w in halves:
                images.append(flat[off:off + h * w].reshape(h, w).copy())
                off += h * w
            return out, images

    def __call__(self, rects):
        out = []
        for (n_px, s1, s2), (x0, y0, x1, y1) in zip(self.sums(rects), (r[-4:] for r in rects)):
            out.append((float(min(y1 - y0, x1 - x0)), (n_px * s2 - s1 * s1) / (n_px * n_px)))
        return out

    def full_size(self, rects):
        """``[(min_side, lap)]`` of the same rectangles measured as they are, without the half-size stage: the evaluator's
        ``variance_of_laplacian(crop_rgb)`` (altfreezing/TEST2.py:296-299).  One launch of ``af_face_laplacian_stores_u8`` per 64
        rectangles (counted in ``launches``) and one read-back."""
        out = []
        for (n_px, s1, s2), (x0, y0, x1, y1) in zip(self.full_sums(rects), (r[-4:] for r in rects)):
            out.append((float(min(y1 - y0, x1 - x0)), (n_px * s2 - s1 * s1) / (n_px * n_px)))
        return out


class FaceQuality(_QualitySums):
    """``FaceQuality(store, channel_order)(rects)`` -> ``[(min_side, lap), ...]``: the pixel part of the quality gate (:265-267,
    :191-192) for every rectangle ``(slot, x0, y0, x1, y1)`` of the resident frames of ``store`` (an ``evaluator.FrameStore``) in
    one launch of ``af_face_quality_u8`` (csrc/af_quality.hip) and one pinned read-back on the current stream - the only wait.  The
    kernel returns three exact integers per rectangle; ``lap = (n_px * S2 - S1^2) / n_px^2`` is formed here from Python integers
    with one fp64 division.  ``sums(rects, grey=True)`` also returns the half-size grey images (tests)."""

    def __init__(self, store: FrameStore, channel_order: str = "bgr"):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        super().__init__(store.device)
        self.store, self.bgr = store, int(_known_order(channel_order) == "bgr")
        self._fn = _lib.lib.af_face_quality_u8

    def sums(self, rects, grey: bool = False):
        """-> ``[(n_px, S1, S2)]`` as Python integers (and, with ``grey``, the list of (dh, dw) uint8 grey images)"""
        import ctypes as C
        from .evaluator import _RECT_DTYPE
        store = self.store
        items = np.zeros(len(rects), dtype=_RECT_DTYPE)
        for i, (slot, x0, y0, x1, y1) in enumerate(rects):
            items[i] = (slot, x0, y0, y1 - y0, x1 - x0, 0, 0, 0)

        def launch(lo, hi, sums, gptr, gn, stream, full=False):
            return self._fn(C.c_void_p(store.dev.data_ptr()), store.plan_source(), C.c_void_p(items[lo:hi].ctypes.data), hi - lo, self.bgr,
                            sums, gptr, gn, stream)
        return self._sums([(int(r["ih"]), int(r["iw"])) for r in items], grey, launch, "face_quality_u8")

    def full_sums(self, rects, grey: bool = False):
        """``sums`` of the rectangles at full size (the (h, w) grey images with ``grey``): the one store through the several-store
        entry point, which is the only one the full-size mode has"""
        if getattr(self, "_stores", None) is None:
            self._stores = StoresQuality(self.device)
        order = "bgr" if self.bgr else "rgb"
        launched = self._stores.launches
        try:
            return self._stores.full_sums([(self.store, order) + tuple(r) for r in rects], grey)
        finally:
            self.launches += self._stores.launches - launched


# ---- the whole live step: af_realtime.py:372-509 ----------------------------------------------------------------------------------

class CallState:
    """what ``track_faces`` keeps between frames: ``last_lm`` (:250) and ``_q_hist`` (:239)"""

    def __init__(self):
        import collections
        self.last_lm = {}
        self.q_hist = collections.defaultdict(lambda: collections.deque(maxlen=64))


def in_exclude(box, H: int, W: int, exclude_rect) -> bool:
    """the centre of ``box`` lies in the self-view rectangle, given in normalised coordinates (:311-315)"""
    x1, y1, x2, y2 = box
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    x1n, y1n, x2n, y2n = exclude_rect
    return (x1n * W <= cx <= x2n * W) and (y1n * H <= cy <= y2n * H)


def track_faces(state: CallState, frame_idx: int, shape, dets, online, quality, gate, mesh_every: int = 1, crop_scale: float = 0.6,
                exclude_rect=(0.70, 0.70, 1.00, 1.00), landmarks=None, frame_view=None):
    """``track_gate`` behind ``track_candidates``: see there.  ``quality(rects)`` -> ``[(min_side, lap)]`` for rectangles ``(x0,
    y0, x1, y1)`` of this frame, called once with all of them (not at all without one); ``gate(min_side, lap)`` -> the weight."""
    found = track_candidates(state, frame_idx, shape, dets, online, mesh_every, crop_scale, exclude_rect, landmarks, frame_view)
    rects = found[0]
    return track_gate(state, found, quality(rects) if rects else [], gate)


def track_candidates(state: CallState, frame_idx: int, shape, dets, online, mesh_every: int = 1, crop_scale: float = 0.6,
                     exclude_rect=(0.70, 0.70, 1.00, 1.00), landmarks=None, frame_view=None):
    """The host part of ``RealtimeAF.step`` between the tracker and the window bookkeeping (:390-442), without a device call of
    its own, in two halves around the quality measurement so that a server can measure the crops of many calls in one launch.
    This half (:390-437): ``dets``: this frame's (N, 15) float32 YuNet rows, or None; ``online``: the tracker's tracks
    (``track_id``, ``tlbr``).  Returns ``(rects, candidates, alive, kept_boxes)``, ``rects`` - the crop rectangles ``(x0, y0, x1,
    y1)`` whose quality is wanted - first; the whole tuple goes to ``track_gate``.  The order of the skips is the reference's: an
    excluded track is not alive, a track skipped later is."""
    H, W = int(shape[0]), int(shape[1])
    det_tlbr = None
    if dets is not None and len(dets) > 0:                                             # :391-396
        dets = np.asarray(dets, dtype=np.float32)
        det_tlbr = np.concatenate([dets[:, :2], dets[:, :2] + dets[:, 2:4]], axis=1).astype(np.float32)
    kept_boxes, candidates, alive = {}, [], set()
    for tr in online or []:                                                            # :401
        if in_exclude(tr.tlbr, H, W, exclude_rect):                                    # :403
            continue
        tid = tr.track_id
        tlbr = np.asarray(tr.tlbr).astype(np.float32).copy()
        kept_boxes[tid] = tlbr                                                         # :407
        alive.add(tid)
        yunet_lm5 = None
        if det_tlbr is not None:                                                       # :413-418
            ious = 1.0 - iou_distance(np.array([tr.tlbr], dtype=np.float32), det_tlbr)[0]
            k = int(np.argmax(ious))
            if ious[k] >= 0.4:
                yunet_lm5 = dets[k][5:15].reshape(5, 2)
        fm = None
        if (frame_idx % mesh_every) == 0 or (tid not in state.last_lm):                # :421-426
            fm = landmarks(frame_view, tr.tlbr) if landmarks is not None else None
            if fm is None and yunet_lm5 is not None:
                fm = {"lm5": yunet_lm5, "lm68": None}
            if fm is not None:
                state.last_lm[tid] = {**fm, "frame_idx": frame_idx}
        else:                                                                          # :427-430
            cached = state.last_lm.get(tid)
            if cached is not None:
                fm = {"lm5": cached["lm5"], "lm68": cached["lm68"]}
            elif yunet_lm5 is not None:
                fm = {"lm5": yunet_lm5, "lm68": None}
        if fm is None:                                                                 # :431-432
            continue
        x1, y1, x2, y2 = map(int, get_crop_box((H, W), tlbr, scale=crop_scale))        # :435-436, on the float32 box as LiveCall
        if x2 <= x1 or y2 <= y1:                                                       # :437
            continue
        candidates.append((tid, tlbr, np.asarray(fm["lm5"], dtype=np.float32), (x1, y1, x2, y2)))
    return [c[3] for c in candidates], candidates, alive, kept_boxes


def track_gate(state: CallState, found, measured, gate):
    """the second half (:438-442): ``found`` from ``track_candidates``, ``measured`` = ``[(min_side, lap)]`` of its rectangles,
    ``gate(min_side, lap)`` -> the weight.  Returns ``(faces, alive, kept_boxes, rects)``: ``faces`` - ``(tid, tlbr float32, lm5)``
    of the tracks that go on to the windows; ``alive`` - the tids of the tracks that were kept past the self-view exclusion but go
    no further (no landmarks, a degenerate crop box, or a weight of 0); ``kept_boxes`` as :407; ``rects`` as they were measured."""
    rects, candidates, alive, kept_boxes = found
    faces = []
    for (tid, tlbr, lm5, _), (min_side, lap) in zip(candidates, measured):
        state.q_hist[tid].append((float(min_side), float(lap)))                        # :440
        if gate(min_side, lap) <= 0.0:                                                 # :441-442
            continue
        faces.append((tid, tlbr, lm5))
    return faces, alive - {f[0] for f in faces}, kept_boxes, rects


def _detect_size(size):
    """``detect_size`` as a call keeps it: None, or (dw, dh) as two positive ints"""
    if size is None:
        return None
    dw, dh = (int(v) for v in size)
    if dw < 1 or dh < 1:
        raise ValueError("realtime: detect_size %r: two positive numbers (dw, dh), or None" % (size,))
    return dw, dh


def _scale_back(rows: np.ndarray, shape, size) -> np.ndarray:
    """(n, 15) YuNet rows found on a frame of `shape` resized to `size` = (dw, dh) -> the frame's own, float64"""
    from .detector import YuNet
    return YuNet.scale_rows(rows, shape[1] / size[0], shape[0] / size[1])


class _Detections:
    """the read-back of a step's detector results: ``read([(rows, counts), ...])`` - device tensors, (B, N, 15) and (B,) - -> the
    (n, 15) float32 numpy rows of every frame, in order.  The counts and the first 64 rows of every frame come back in one pinned
    copy and one wait; one more copy and wait only for a frame with more rows.  ``count``: ``ServerStats.count``."""

    def __init__(self):
        self._host = None
        self.extra = []                     # the host bytes of the last read's ``extra`` tensors, in order

    def read(self, results, device, count=lambda key: None, extra=()) -> List[np.ndarray]:
        """``extra``: uint8 device tensors (a multiple of 4 bytes each, the device tracker's records) that ride in the same copy
        and wait; their bytes are in ``self.extra`` afterwards"""
        packed, places, at = [], [], 0
        for rows, counts in results:                                                   # a result: its counts, then its first rows
            b, first = rows.shape[0], min(64, rows.shape[1])
            packed += [counts[:b].to(torch.float32), rows[:, :first].reshape(-1)]
            places.append((rows, first, at))
            at += b * (1 + first * 15)
        riders = []
        for t in extra:
            riders.append((at, t.numel() // 4))
            packed.append(t.reshape(-1).view(torch.float32))
            at += t.numel() // 4
        if self._host is None or self._host.numel() < at:
            self._host = torch.empty(max(at, 16 * (1 + 64 * 15)), dtype=torch.float32, pin_memory=True)
        self._host[:at].copy_(torch.cat(packed), non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
        count("wait")
        host, out = self._host.numpy(), []
        self.extra = [host[lo:lo + n].view(np.uint8).copy() for lo, n in riders]
        for rows, first, at in places:
            for b in range(rows.shape[0]):
                n = int(host[at + b])
                if n > first:
                    out.append(rows[b, :n].cpu().numpy())
                    count("wait")
                else:
                    lo = at + rows.shape[0] + b * first * 15
                    out.append(host[lo:lo + n * 15].reshape(n, 15).copy())
        return out


class RealtimeCall:
    """``RealtimeCall(network, detector).step(frame_bgr)`` -> ``[(tid, score), ...]``: the whole of ``RealtimeAF.step``
    (test/af_realtime.py:372-509) with the captured frame as its only input, by composition over ``LiveCall``.

    One host-to-device copy per frame: ``LiveCall.admit`` puts the frame into the ring, the detector reads it there
    (``detector.detect(call.frame_view(k)[None])``), the quality gate is one ``FaceQuality`` launch over rectangles of the same
    resident frame, and a window that closes is warped out of it.  A step waits for the device at most twice without a window
    close (the detections, the quality sums) and three times with one (the scores).

    ``detector``: a ``YuNet`` (``detector=None`` with ``modelPath`` builds one with ``conf``, 0.3, 5000 as :219) or any object with
    ``detect(frames_u8) -> (rows, counts)`` device tensors.  The tracker is ``tracker.ByteTracker`` with ``track_thresh``,
    ``track_buffer``, ``match_thresh`` at 30 fps.  ``landmarks``: an optional callable ``(frame_view, tlbr) -> {'lm5', 'lm68'} |
    None`` where the reference has FaceMesh; without it the call behaves as the reference does when FaceMesh finds nothing: YuNet's
    five points, with the ``last_lm`` cache.  Every other keyword is ``RealtimeAF``'s with its default, plus ``LiveCall``'s
    ``ring_frames``, ``max_batch``, ``channel_order``, ``size``.  After the scores (:340-358, :501-505): ``score_is_real``,
    ``running_scores``, ``clip_hist`` and ``state[tid]["fake"]`` (median of 5 with hysteresis 0.75 / 0.65), ``last_boxes`` and
    ``pick_interlocutor_id``; the entries of purged tids are dropped (:489-499).  Not built: ``last_aligned``, the Win32 apps.

    ``detect_size=(dw, dh)``: a detecting tick resizes the resident frame to dw x dh on the device (``frames.FrameResizer``,
    cv2.resize's arithmetic), runs the detector there and hands the tracker the rows scaled back to the frame (float64, YuNet's
    row layout: ``YuNet.scale_rows`` with W / dw and H / dh, as demo2.py does).  ``None`` (the default) detects at full size.

    ``tracker="device"``: the tracker is a ``device_tracker.DeviceByteTracker`` - its launch follows the detector's on the rows where
    they lie (the start filter and the scale-back happen there), its record rides in the read-back of the rows, so a step waits no
    more often; a frame without detection enqueues the launch and reads nothing.  Every discrete result is the host tracker's, the
    boxes agree to round-off.  ``"host"`` (the default) is ``tracker.ByteTracker``.

    ``candidates="device"`` (needs ``tracker="device"`` and no ``landmarks`` hook): ``track_candidates`` - the self-view exclusion, the
    five-point pick, the ``mesh_every`` cache and the crop box - runs behind the tracker in the tracker's launch
    (csrc/af_live_core.h), the quality launch takes its rectangles from the record that stage leaves
    (``af_face_quality_records_u8``), and rows, both records and the quality sums come back in ONE copy behind ONE wait: a step
    waits once, twice when a window closes, where ``"host"`` (the default) waits once more.  Every result is that of
    ``candidates="host"`` on the same tracker, bit for bit.  The five-point cache then lives in the tracker's device block
    (``tracker.cache_dump()`` reads it, with a wait): ``host.last_lm`` stays empty in this mode."""

    def __init__(self, network, detector=None, modelPath=None, conf: float = 0.8, clip_size: int = 32, stride: int = 52,
                 crop_scale: float = 0.6, drop_after: int = 90, detect_every: int = 1, mesh_every: int = 1, start_conf: float = 0.76,
                 start_min_size: int = 80, q_weighting: bool = True, q_min_size_soft: int = 64, q_min_size_hard: int = 32,
                 q_lap_soft: float = 20.0, q_lap_hard: float = 5.0, exclude_rect=(0.70, 0.70, 1.00, 1.00), score_is_real: bool = False,
                 track_thresh: float = 0.8, track_buffer: int = 90, match_thresh: float = 0.8, landmarks=None, size: int = 224,
                 ring_frames: int = 128, max_batch: int = 16, channel_order: str = "bgr", detect_size=None,
                 tracker: str = "host", candidates: str = "host"):
        import collections
        from types import SimpleNamespace
        self.detect_size = _detect_size(detect_size)
        self._resizer = None
        if detector is None:
            if modelPath is None:
                raise ValueError("realtime: a detector, or the modelPath of the YuNet file to build one from")
            from .detector import YuNet
            detector = YuNet(modelPath, confThreshold=conf, nmsThreshold=0.3, topK=5000)
        self.detector, self.landmarks = detector, landmarks
        self.call = self._ring_type(network, clip_size=clip_size, size=size, stride=stride, crop_scale=crop_scale, ring_frames=ring_frames,
                             max_batch=max_batch, drop_after=drop_after, channel_order=channel_order)
        if tracker not in ("host", "device"):
            raise ValueError("realtime: tracker %r: \"host\" or \"device\"" % (tracker,))
        if candidates not in ("host", "device"):
            raise ValueError("realtime: candidates %r: \"host\" or \"device\"" % (candidates,))
        if candidates == "device" and tracker != "device":
            raise ValueError("realtime: candidates=\"device\" needs tracker=\"device\": the candidate stage runs in the device tracker's launch, on the "
                             "tracks where that leaves them")
        if candidates == "device" and landmarks is not None:
            raise ValueError("realtime: candidates=\"device\" needs landmarks=None: the hook reads a frame on the host between the tracker and the "
                             "crop box, where this mode has no host trip")
        tracker_args = SimpleNamespace(track_thresh=track_thresh, track_buffer=track_buffer, match_thresh=match_thresh, mot20=False)
        self.tracker_mode, self.candidates_mode = tracker, candidates
        if tracker == "device":
            from .device_tracker import DeviceByteTracker
            self.tracker = DeviceByteTracker(tracker_args, frame_rate=30.0, device=_network_device(getattr(network, "network", network)),
                                             candidates=candidates == "device")
            self._track_pending = []             # [(records, [tracker])] enqueued and not read yet: they ride in the next read
        else:
            self.tracker = ByteTracker(tracker_args, frame_rate=30.0)
        self.detect_every, self.mesh_every = int(detect_every), int(mesh_every)
        self.start_conf, self.start_min_size = float(start_conf), int(start_min_size)
        self._gate = dict(q_weighting=bool(q_weighting), q_min_size_soft=int(q_min_size_soft), q_min_size_hard=int(q_min_size_hard),
                          q_lap_soft=float(q_lap_soft), q_lap_hard=float(q_lap_hard))
        self.exclude_rect, self.score_is_real = tuple(exclude_rect), bool(score_is_real)
        self.drop_after, self.crop_scale = int(drop_after), float(crop_scale)
        self.host = CallState()
        self.running_scores = collections.defaultdict(list)
        self.clip_hist = collections.defaultdict(lambda: collections.deque(maxlen=5))
        self.state, self.last_boxes = {}, {}
        self.detections = None                       # the rows the last detect frame handed the tracker's filter (N, 15) float32
        self._quality = self._quality_ring = self._records_quality = None
        self._detections = _Detections()

    _ring_type = LiveCall
    frame_idx = property(lambda self: self.call.frame_idx)
    uploaded_bytes = property(lambda self: self.call.uploaded_bytes)
    purged = property(lambda self: self.call.purged)

    def _detect(self, view, tracked=None) -> np.ndarray:
        """the detector on the resident frame and the one read-back of its rows; with the device tracker (``tracked``: a list)
        the tracker's launch follows the detector's on the rows where they lie, its record rides in the same read-back and the
        tracks it returned are appended to ``tracked``"""
        rows, counts = self._detector_rows(view)
        with torch.cuda.device(rows.device):
            if tracked is None:
                found = self._detections.read([(rows, counts)], rows.device)[0]
            else:
                self._enqueue_tracker(self._rows_job(rows[0], counts[0:1], view.shape))
                found = self._detections.read([(rows, counts)], rows.device, extra=[r for r, _ in self._track_pending])[0]
                tracked += _absorb_records(self._track_pending, self._detections.extra)[self.tracker]
        return found if self.detect_size is None else _scale_back(found, view.shape, self.detect_size)

    def _detector_rows(self, view):
        """the detector's launches on the resident frame, resized first where the call has a ``detect_size``: device (rows, counts)"""
        if self.detect_size is not None:
            if self._resizer is None:
                self._resizer = FrameResizer(view.device)
            with torch.cuda.device(view.device):
                small = self._resizer.resize([view], self.detect_size)
            return self.detector.detect(small)
        return self.detector.detect(view[None])

    def _live_job(self, k: int, shape, rows=None, count=None):
        """this call's tracker-and-candidates job for frame `k` (``candidates="device"``): on a detector's rows (N, 15) and count
        (1,) read in place, or without a detection"""
        extra = dict(frame_idx=k, slot=k % self.call.ring_frames, shape=shape, mesh_every=self.mesh_every, crop_scale=self.crop_scale,
                     exclude_rect=self.exclude_rect, purged=self.call.purged)
        if rows is None:
            return self.tracker.live_job(self.tracker.empty_job(), **extra)
        size = self.detect_size
        return self.tracker.live_rows_job(rows, count, self.start_conf, self.start_min_size,
                                          (1.0, 1.0) if size is None else (shape[1] / size[0], shape[0] / size[1]), **extra)

    def _came_back(self, dets, track_record, record, sums):
        """the host side of a ``candidates="device"`` frame once its records are back: the rows kept in ``detections``, the tracker's
        lists, ``track_candidates``' tuple from the candidate record and ``[(min_side, lap)]`` of its rectangles from `sums` (this
        call's ``MAX_TRACKS`` parsed ``af_quality_sums``) -> ``(found, measured)`` for ``track_gate``"""
        from .device_tracker import candidates_of
        if dets is not None:
            self.detections = dets
        self.tracker.absorb(track_record)
        found = candidates_of(record)
        if int(record["bad"]):
            raise RuntimeError("live: the quality launch refused a rectangle of frame %d: %r" % (int(record["frame_idx"]), found[0]))
        measured = [(float(min(y1 - y0, x1 - x0)), (int(r["n_px"]) * int(r["s2"]) - int(r["s1"]) ** 2) / (int(r["n_px"]) * int(r["n_px"])))
                    for r, (x0, y0, x1, y1) in zip(sums, found[0])]
        return found, measured

    def _step_device(self, frame) -> List[Tuple]:
        """``step`` with ``candidates="device"``: detector, tracker and candidates, quality - enqueued one behind the other on
        the resident frame - and ONE read-back of rows, records and sums"""
        from .device_tracker import parse_live_records, parse_records, update_live_calls
        call = self.call
        k = call.admit(frame)
        view, dev = call.frame_view(k), self.tracker.device
        detect = k % max(1, self.detect_every) == 0
        with torch.cuda.device(dev):
            results = [self._detector_rows(view)] if detect else []
            job = self._live_job(k, frame.shape, results[0][0][0], results[0][1][0:1]) if detect else self._live_job(k, frame.shape)
            track_records, records = update_live_calls([job], dev)
            if self._records_quality is None:
                self._records_quality = RecordsQuality(dev)
            sums = self._records_quality.enqueue([(records[0], call._ring.store, call.channel_order, k % call.ring_frames)])
            read = self._detections.read(results, dev, extra=[track_records, records, sums])
        dets = None
        if detect:
            dets = read[0] if self.detect_size is None else _scale_back(read[0], view.shape, self.detect_size)
        raw_t, raw_r, raw_s = self._detections.extra
        found, measured = self._came_back(dets, parse_records(raw_t)[0], parse_live_records(raw_r)[0], RecordsQuality.parse(raw_s))
        faces, alive, kept_boxes, _ = track_gate(self.host, found, measured, self._weight)
        return self._after(call.advance(faces, alive), kept_boxes)

    def _rows_job(self, rows, count, shape):
        """this call's device-tracker job on a detector's rows (N, 15) and count (1,), read in place"""
        size = self.detect_size
        return self.tracker.rows_job(rows, count, self.start_conf, self.start_min_size,
                                     (1.0, 1.0) if size is None else (shape[1] / size[0], shape[0] / size[1]))

    def _enqueue_tracker(self, job):
        from .device_tracker import update_calls
        self._track_pending.append((update_calls([job], self.tracker.device), [self.tracker]))

    def _track(self, k: int, shape, dets, online=None):
        """:382-437 for frame `k`, whose detections are `dets` (None when the detector did not run on it): they are kept in
        ``detections``, filtered into the tracker, and the tracks go through ``track_candidates``, whose result this returns.
        ``online``: the tracks of this frame where the device tracker has filtered and tracked already"""
        H, W = shape[:2]
        tracks_in = []
        if dets is not None:
            self.detections = dets
        if online is None:
            for d in (dets if dets is not None else ()):                               # :382-386
                d = np.asarray(d, dtype=np.float32)
                if d[4] >= self.start_conf and max(d[2], d[3]) >= self.start_min_size:
                    tracks_in.append(STrack(d[:4], score=float(d[4])))
            online = self.tracker.update(tracks_in, (H, W), (H, W))                    # :388
        return track_candidates(self.host, k, (H, W), dets, online, self.mesh_every, self.crop_scale, self.exclude_rect, self.landmarks,
                                self.call.frame_view(k) if self.landmarks is not None else None)

    def _weight(self, min_side: float, lap: float) -> float:
        return quality_weight(min_side, lap, **self._gate)

    def _frame_quality(self, rects):
        ring = self.call._ring.store
        if self._quality_ring is not ring:                                             # a new ring after a change of the frame size
            self._quality, self._quality_ring = FaceQuality(ring, self.call.channel_order), ring
        slot = self.call.frame_idx % self.call.ring_frames
        return self._quality([(slot,) + tuple(r) for r in rects])

    def step(self, frame: np.ndarray) -> List[Tuple]:
        if self.candidates_mode == "device":
            return self._step_device(frame)
        call = self.call
        k = call.admit(frame)                                                          # :373-376, the one upload
        online = [] if self.tracker_mode == "device" else None
        dets = self._detect(call.frame_view(k), online) if k % max(1, self.detect_every) == 0 else None      # :378-380
        if online is not None and dets is None:                                        # no detection: enqueued, read with the next rows
            with torch.cuda.device(self.tracker.device):
                self._enqueue_tracker(self.tracker.empty_job())
        found = self._track(k, frame.shape, dets, online)
        faces, alive, kept_boxes, _ = track_gate(self.host, found, self._frame_quality(found[0]) if found[0] else [], self._weight)
        results = call.advance(faces, alive)                                           # :445-499
        return self._after(results, kept_boxes)

    def _after(self, results, kept_boxes):
        """what the reference does with a score once it exists (:340-358), the purge of a dropped tid's entries (:489-499) and the
        last known boxes (:501-505)"""
        out = []
        for tid, s in results:
            s = 1.0 - float(s) if self.score_is_real else float(s)                     # :340-341
            self.running_scores[tid].append(s)
            out.append((tid, s))
            self.clip_hist[tid].append(s)
            sm = float(np.median(self.clip_hist[tid]))
            st = self.state.get(tid, {"fake": False})
            if not st["fake"] and sm >= 0.75:
                st["fake"] = True
            elif st["fake"] and sm < 0.65:
                st["fake"] = False
            self.state[tid] = st
        for tid in self.call.purged:
            self.host.last_lm.pop(tid, None)
            self.running_scores.pop(tid, None)
            self.last_boxes.pop(tid, None)
        tracks = self.call._tracks
        persisting = {tid: box for tid, box in self.last_boxes.items() if tid not in tracks or tracks[tid].missed < self.drop_after}
        persisting.update(kept_boxes)
        self.last_boxes = persisting
        return out

    def pick_interlocutor_id(self, H: int, W: int):
        """the largest face outside the self-view rectangle, or the largest of all when every face is inside it (:279-291)"""
        if not self.last_boxes:
            return None
        area = lambda b: (b[2] - b[0]) * (b[3] - b[1])
        cand = [(tid, area(b)) for tid, b in self.last_boxes.items() if not in_exclude(b, H, W, self.exclude_rect)]
        if not cand:
            cand = [(tid, area(b)) for tid, b in self.last_boxes.items()]
        return max(cand, key=lambda t: t[1])[0]


def _absorb_records(pending, host_bytes) -> dict:
    """the device tracker's records that came back: ``pending`` = [(records, [tracker, ...])] in the order they were enqueued,
    ``host_bytes`` their bytes; every tracker absorbs its records in that order; -> {tracker: the tracks of its LAST record};
    empties ``pending``"""
    from .device_tracker import parse_records
    last, came_back = {}, list(zip(pending, host_bytes))
    del pending[:]                                                # before a tracker past its cap raises: a record is absorbed once
    for (_, trackers), raw in came_back:
        for tr, rec in zip(trackers, parse_records(raw)):
            last[tr] = tr.absorb(rec)
    return last


# ---- many calls per device: the launches of one step shared by every call ---------------------------------------------------------

class _ServedRing(LiveCall):
    """the books and the frame ring of one call of a ``CallServer``: no warp, clip buffer or event of its own - the server's
    launches read the ring, and the server orders the steps"""

    def _new_ring(self, shape):
        dev = _network_device(self.network)
        with torch.cuda.device(dev):
            store = FrameStore(dev, self.channel_order)
            store.open(shape, self.ring_frames)
        return _DeviceSide(store, None, None)

    def _store_frame(self, frame: np.ndarray, slot: int):
        ring = self._ring.store
        with torch.cuda.device(ring.device):
            ring.put([frame], slot)
        self.uploaded_bytes += upload_bytes(frame)

    def _score(self, ready):
        raise RuntimeError("live: a served call is scored by its CallServer")


class _ServedCall(RealtimeCall):
    """a call's state inside a ``CallServer``: ``RealtimeCall``'s attributes, stepped only by the server"""
    _ring_type = _ServedRing

    def step(self, frame):
        raise RuntimeError("live: a served call is stepped by its CallServer (server.step({cid: frame}))")


class StoresQuality(_QualitySums):
    """``FaceQuality`` over rectangles of several frame stores: ``rects = [(store, channel_order, slot, x0, y0, x1, y1)]`` in one
    launch of ``af_face_quality_stores_u8`` per 64 rectangles, whatever their stores, and one read-back"""

    def __init__(self, device):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        super().__init__(device)
        self._fn = _lib.lib.af_face_quality_stores_u8
        self._full_fn = _lib.lib.af_face_laplacian_stores_u8

    def sums(self, rects, grey: bool = False, full: bool = False, both: bool = False):
        import ctypes as C
        from .evaluator import _RECT_DTYPE

        def launch(lo, hi, sums, gptr, gn, stream, full=False):
            table = StoreTable()                                           # the stores of this launch
            items = np.zeros(hi - lo, dtype=_RECT_DTYPE)
            for i, (store, order, slot, x0, y0, x1, y1) in enumerate(rects[lo:hi]):
                items[i] = (slot, x0, y0, y1 - y0, x1 - x0, 0, 0, table.index(store, order))
            fn = self._full_fn if full else self._fn
            return fn(table.array(), len(table.refs), C.c_void_p(items.ctypes.data), hi - lo, sums, gptr, gn, stream)
        return self._sums([(r[6] - r[4], r[5] - r[3]) for r in rects], grey, launch,
                          "face_quality_stores_u8 / face_laplacian_stores_u8" if both else "face_laplacian_stores_u8" if full else "face_quality_stores_u8",
                          full, both)

    def full_sums(self, rects, grey: bool = False):
        """``sums`` of the rectangles at full size: ``af_face_laplacian_stores_u8``; with ``grey`` the (h, w) grey images"""
        return self.sums(rects, grey, full=True)

    def half_and_full(self, rects):
        """``[(min_side, half-size lap, full-size lap)]``: both modes of the kernel on the same rectangles - one launch of each per
        64 rectangles - behind ONE read-back: what the evaluator's gate measures of a crop while ``_qstat`` is short"""
        half, full = self.sums(rects, both=True)
        lap = lambda t: (t[0] * t[2] - t[1] * t[1]) / (t[0] * t[0])
        return [(float(min(r[6] - r[4], r[5] - r[3])), lap(h), lap(f)) for r, h, f in zip(rects, half, full)]


class RecordsQuality:
    """The quality launch on the candidate records of live calls where the candidate stage left them
    (``af_face_quality_records_u8``): ``enqueue([(record, store, channel_order, slot)])`` - ``record`` a call's
    (LIVE_RECORD_BYTES,) uint8 device tensor, its frame in ``slot`` of ``store`` - enqueues one launch per 64 jobs on the current
    stream and returns the uint8 device tensor of ``len(jobs) * MAX_TRACKS`` ``af_quality_sums`` without waiting; candidate k of
    job j is entry ``j * MAX_TRACKS + k`` of ``parse``'s result.  ``launches`` counts the calls into the C function."""

    def __init__(self, device):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        self.device, self.launches = device, 0
        self._fn = _lib.lib.af_face_quality_records_u8

    def enqueue(self, jobs, grey=None, grey_stride: int = 0) -> torch.Tensor:
        import ctypes as C
        from . import _lib
        per = _lib.AF_TRACK_MAX_TRACKS * C.sizeof(_lib.QualitySums)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            with torch.inference_mode(False):
                sums = torch.empty(max(1, len(jobs)) * per, dtype=torch.uint8, device=self.device)
            for lo in range(0, len(jobs), _lib.QUALITY_MAX_RECTS):                     # one launch for up to 64 calls
                chunk, table = jobs[lo:lo + _lib.QUALITY_MAX_RECTS], StoreTable()
                items = (_lib.LiveQualityJob * len(chunk))()
                for item, (record, store, order, slot) in zip(items, chunk):
                    item.record, item.store, item.slot = record.data_ptr(), table.index(store, order), int(slot)
                gptr = None if grey is None else grey.data_ptr() + lo * _lib.AF_TRACK_MAX_TRACKS * int(grey_stride)
                _lib.check(self._fn(table.array(), len(table.refs), items, len(chunk), C.c_void_p(sums.data_ptr() + lo * per), C.c_void_p(gptr),
                                    int(grey_stride), C.c_void_p(cur.cuda_stream)), "face_quality_records_u8")
                self.launches += 1
        return sums[:len(jobs) * per]

    @staticmethod
    def parse(raw) -> np.ndarray:
        """the host bytes of ``enqueue``'s tensor -> the parsed ``af_quality_sums``"""
        return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=_SUMS_DTYPE)


class ServerStats:
    """what a ``CallServer`` enqueued and waited for: ``last`` for the last step, ``total`` since the server was made, each with
    ``detect`` (calls of ``af_yunet_detect_frames``, or of a detector's ``detect_views``), ``quality``, ``warp`` (launches),
    ``replay`` (graph replays), ``wait`` (host waits for the device), ``convert`` (launches of ``af_yuv420_to_rgb_u8`` / ``af_yuv_to_rgb_ex_u8``),
    ``yuv_copies`` (host-to-device copies of staged YUV planes), ``capture`` (launches of ``af_capture_to_stores_u8``), ``resize``
    (launches of ``af_resize_frames_u8``) and ``track`` (launches of ``af_bytetrack_update_calls``, and the kernels of
    ``af_live_update_calls`` for the calls with ``candidates="device"``, whose ``af_face_quality_records_u8`` launch counts under
    ``quality``; in ``VideoRunner``, of ``af_runner_track_chunk``)"""
    KEYS = ("detect", "quality", "warp", "replay", "wait")
    YUV_KEYS = ("convert", "yuv_copies")       # appear in ``last`` / ``total`` once a step has YUV frames; read as 0 before
    CAPTURE_KEYS = ("capture",)                # likewise once a step has captured frames
    RESIZE_KEYS = ("resize",)                  # likewise once a call with a ``detect_size`` has detected
    TRACK_KEYS = ("track",)                    # likewise once a call with ``tracker="device"`` has stepped: launches of ``af_bytetrack_update_calls``

    class _Counts(dict):
        def __missing__(self, key):
            if key in ServerStats.YUV_KEYS or key in ServerStats.CAPTURE_KEYS or key in ServerStats.RESIZE_KEYS or key in ServerStats.TRACK_KEYS:
                return 0
            raise KeyError(key)

    def __init__(self):
        self.steps = 0
        self.last = self._Counts.fromkeys(self.KEYS, 0)
        self.total = self._Counts.fromkeys(self.KEYS, 0)

    def begin(self):
        self.steps += 1
        self.last = self._Counts.fromkeys(self.KEYS, 0)

    def count(self, key: str, n: int = 1):
        self.last[key] += n
        self.total[key] += n


class CallServer:
    """Many live calls on one device: ``server.step({cid: frame, ...})`` -> ``{cid: [(tid, score), ...]}`` does for every call in
    the mapping what ``RealtimeCall.step`` does for one, on launches that all of them share.

        server = CallServer(network, modelPath="face_detection_yunet_2023mar.onnx")
        a, b = server.open(), server.open(channel_order="rgb", detect_every=2)
        results = server.step({a: frame_a, b: frame_b})          # a call that is not in the mapping does not advance
        server.call(a).running_scores, server.call(a).state      # a call's state: ``RealtimeCall``'s attributes
        server.close(b)

    ``clip_size``, ``size`` and ``max_batch`` belong to the server (one network, one clip buffer); every other keyword of
    ``RealtimeCall`` is a call's own - ``call_defaults`` here, overridden per call in ``open`` - as are its frame size, tracker,
    ``CallState`` and frame ring.  ``detector``: a ``YuNet`` (or ``modelPath`` to build one with ``conf``), or any object with
    ``detect_views(views) -> (rows, counts)``.  ``detect_size=(dw, dh)`` (a call's own, ``None`` by default) detects that call's
    frames resized to dw x dh, as ``RealtimeCall`` does: calls of any frame sizes that share a detect size share one resize launch
    and one ``detect_views``.  ``tracker="device"`` (a call's own, ``"host"`` by default): the trackers of all such calls of a tick run
    as one launch per 64 calls behind the ``detect_views`` launches - on their rows in place where they detected, without a detection
    otherwise - and their records ride in the read-back of the rows; ``stats`` counts ``track``.  ``candidates="device"``
    (a call's own, ``"host"`` by default; needs ``tracker="device"`` and no ``landmarks`` hook): the tracker AND ``track_candidates``
    of all such calls of a tick run in ``af_live_update_calls`` (as many launches as their arguments need), ONE
    ``af_face_quality_records_u8`` launch measures their crops out of the records that leaves, and rows, records and sums come back
    in the one read-back of the rows - on a tick without a detection too, since the candidates come from the record: a tick whose
    calls are all in this mode waits once, twice when a window closes.  Calls in the other modes keep their launches.

    A frame is a numpy array, a ``YuvFrame`` or a ``CapturedFrame`` (the mapping may mix them).  The ``CapturedFrame``s of a step are
    admitted together - one fill, one copy, one ``af_capture_to_stores_u8`` launch per 64 - as are its ``YuvFrame``s: the
    host planes of all calls fill one pinned slot and cross in one copy, and one conversion launch (``YuvConverter``'s) per 64 frames
    converts them - and the device-resident ones where they lie - into the calls' own ring slots, each in its call's
    ``channel_order``.  The conversion needs no wait.

    One step, whatever the number of calls: every frame is admitted into its call's ring (one upload per frame); the calls that
    detect on this frame are grouped by frame shape and each group goes through ``detect_views`` 64 frames at a time, all counts
    and first rows coming back in one pinned copy; per call the tracker and ``track_candidates``; one ``af_face_quality_stores_u8``
    launch per 64 crop rectangles of all calls and one read-back; per call ``track_gate`` and ``advance_host``; the windows that
    closed - ordered as the mapping iterates, then as each call orders its own - go ``max_batch`` at a time through one plan and
    one warp out of all the rings into the server's clip buffer and one replay at the next of 1, 2, 4 ... ``max_batch`` clips (a
    short batch repeats its last window), with one read-back of the scores; per call ``RealtimeCall._after``.  That is at most
    three host waits per step (four when one frame has more than 64 faces).  The scores are ``forward_clips_u8(...,
    return_scores=True)``'s at that batch size, bit for bit; every other result is a lone ``RealtimeCall``'s on the same frames.

    Streams: a step waits, on the stream it is called on, for the event the step before recorded behind its last launch, as
    ``LiveCall`` does; the rings are read and written only here; ``close`` and a change of a call's frame size (which re-opens
    that call's ring, as in ``LiveCall``) wait for the device first.  ``stats``: ``ServerStats``."""

    def __init__(self, network, detector=None, modelPath=None, max_batch: int = 16, clip_size: int = 32, size: int = 224, conf: float = 0.8,
                 **call_defaults):
        self.network = getattr(network, "network", network)
        if detector is None:
            if modelPath is None:
                raise ValueError("server: a detector, or the modelPath of the YuNet file to build one from")
            from .detector import YuNet
            detector = YuNet(modelPath, confThreshold=conf, nmsThreshold=0.3, topK=5000)
        self.detector = detector
        self.clip_size, self.size, self.max_batch = int(clip_size), int(size), int(max_batch)
        self.call_defaults = self._a_calls_own(call_defaults)
        self.device = _network_device(self.network)
        self.stats = ServerStats()
        self.uploaded_bytes = 0
        self._calls: Dict[int, _ServedCall] = {}
        self._next = 0
        self._quality = StoresQuality(self.device)
        self._warp = StoresWarp(self.device, self.clip_size, self.size, self.max_batch)
        self._resizer: Optional[FrameResizer] = None        # made when the first call with a ``detect_size`` detects
        self._converters = {}                     # converter class -> one with its own pinned ring: the frames of a kind of all calls of a step share one slot
        self._scoring: Optional[_ClosedWindows] = None      # the clip buffer and the scorers, made when the first window closes
        self._done = None                  # recorded behind the last launch of every step
        self._detections = _Detections()
        self._track_pending = []                  # the device trackers' records enqueued and not read yet
        self._records_quality: Optional[RecordsQuality] = None      # made when the first call with ``candidates="device"`` steps

    _scorers = property(lambda self: self._scoring.scorers if self._scoring is not None else {})

    @staticmethod
    def _a_calls_own(keywords) -> dict:
        for name in ("network", "detector", "modelPath", "clip_size", "size", "max_batch"):
            if name in keywords:
                raise TypeError("server: %s belongs to the server, not to a call" % name)
        return dict(keywords)

    # -- calls ---------------------------------------------------------------------------------------------
    def open(self, **overrides) -> int:
        """a new call with the server's defaults and these ``RealtimeCall`` keywords; returns its id"""
        args = dict(self.call_defaults, **CallServer._a_calls_own(overrides))
        cid, self._next = self._next, self._next + 1
        self._calls[cid] = _ServedCall(self.network, detector=self.detector, clip_size=self.clip_size, size=self.size,
                                       max_batch=self.max_batch, **args)
        return cid

    def close(self, cid: int) -> None:
        """ends a call: waits for the device, then frees the call's ring and state"""
        self._calls[cid]                                             # KeyError for an unknown call
        torch.cuda.synchronize(self.device)
        del self._calls[cid]

    def call(self, cid: int) -> RealtimeCall:
        return self._calls[cid]

    def __len__(self):
        return len(self._calls)

    # -- the step ------------------------------------------------------------------------------------------
    def step(self, frames: Mapping[int, np.ndarray]) -> Dict[int, List[Tuple]]:
        calls = [(cid, self._calls[cid], frame) for cid, frame in frames.items()]          # KeyError before anything moves
        self.stats.begin()
        if not calls:
            return {}
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._done is None:
                self._done = torch.cuda.Event()
            else:
                cur.wait_event(self._done)
            try:
                return self._step(calls, cur)
            finally:
                self._done.record(cur)

    def _step(self, calls, cur):
        ticks = []
        converted = {}
        for cid, c, frame in calls:                                                        # 1. the uploads
            if isinstance(frame, ConvertedFrame):                                          # the books now, the pixels of all of them below
                ticks.append(c.call.admit_books(frame))
                c.call.uploaded_bytes += frame.upload_bytes
                converted.setdefault(frame.converter, []).append((frame, c.call._ring.store, c.call.channel_order, ticks[-1] % c.call.ring_frames))
            else:
                ticks.append(c.call.admit(frame))
            self.uploaded_bytes += upload_bytes(frame)
        for kind, jobs in converted.items():                                               # per kind one fill, one copy, one launch per 64
            conv = self._converters.get(kind)
            if conv is None:
                conv = self._converters[kind] = kind(self.device)
            launched, copied = conv.launches, conv.copies
            conv.convert(jobs)
            for key, n in zip(conv.stat_keys, (conv.launches - launched, conv.copies - copied)):
                if key is not None:
                    self.stats.count(key, n)
        detecting = [i for i, (_, c, _) in enumerate(calls) if ticks[i] % max(1, c.detect_every) == 0]
        in_launch = [i for i, (_, c, _) in enumerate(calls) if c.candidates_mode == "device"]        # tracker and candidates in one launch
        on_device = [i for i, (_, c, _) in enumerate(calls) if c.tracker_mode == "device" and c.candidates_mode != "device"]
        online, came_back, riders = {}, {}, []

        def trackers(places):
            """behind the detector launches: one tracker launch per 64 calls with a device tracker - the calls that detected on
            their rows where they lie (``places[j]`` = (rows, counts, b) of view j), the others without a detection; for the calls
            with ``candidates="device"`` the tracker-and-candidates launches and ONE quality launch on the records they leave.
            -> (the device tensors to read back, whether this tick needs them)"""
            view_of = {i: j for j, i in enumerate(detecting)}
            if on_device:
                from .device_tracker import update_calls
                jobs = []
                for i in on_device:
                    c = calls[i][1]
                    if i in view_of:
                        rows, counts, b = places[view_of[i]]
                        jobs.append(c._rows_job(rows[b], counts[b:b + 1], calls[i][2].shape))
                    else:
                        jobs.append(c.tracker.empty_job())
                self._track_pending.append((update_calls(jobs, self.device), [calls[i][1].tracker for i in on_device]))
                self.stats.count("track", -(-len(jobs) // 64))
            if in_launch:
                from .device_tracker import live_launches, update_live_calls
                jobs = []
                for i in in_launch:
                    c = calls[i][1]
                    if i in view_of:
                        rows, counts, b = places[view_of[i]]
                        jobs.append(c._live_job(ticks[i], calls[i][2].shape, rows[b], counts[b:b + 1]))
                    else:
                        jobs.append(c._live_job(ticks[i], calls[i][2].shape))
                track_records, records = update_live_calls(jobs, self.device)
                self.stats.count("track", live_launches(len(jobs)))
                if self._records_quality is None:
                    self._records_quality = RecordsQuality(self.device)
                launched = self._records_quality.launches
                sums = self._records_quality.enqueue([(records[j], calls[i][1].call._ring.store, calls[i][1].call.channel_order,
                                                       ticks[i] % calls[i][1].call.ring_frames) for j, i in enumerate(in_launch)])
                self.stats.count("quality", self._records_quality.launches - launched)
                riders[:] = [track_records, records, sums]
            return [r for r, _ in self._track_pending] + riders, bool(riders)

        def tracked():
            from .device_tracker import MAX_TRACKS, parse_live_records, parse_records
            n = len(self._track_pending)
            got = _absorb_records(self._track_pending, self._detections.extra[:n])
            online.update({i: got[calls[i][1].tracker] for i in on_device})
            if riders:
                raw_t, raw_r, raw_s = self._detections.extra[n:n + 3]
                sums = RecordsQuality.parse(raw_s)
                came_back.update({i: (t, r, sums[j * MAX_TRACKS:(j + 1) * MAX_TRACKS])
                                  for j, (i, t, r) in enumerate(zip(in_launch, parse_records(raw_t), parse_live_records(raw_r)))})
        dets = dict(zip(detecting, self._detect([calls[i][1].call.frame_view(ticks[i]) for i in detecting],
                                                [calls[i][1].detect_size for i in detecting], trackers, tracked)))       # 2.
        found, wanted, measured_here = [], [], {}
        for i, (cid, c, frame) in enumerate(calls):                                        # 3. trackers, candidates
            if i in came_back:                                                             #    both ran on the device already
                f, measured_here[i] = c._came_back(dets.get(i), *came_back[i])
                found.append(f)
                continue
            f = c._track(ticks[i], frame.shape, dets.get(i), online.get(i, []) if c.tracker_mode == "device" else None)
            found.append(f)
            ring, slot = c.call._ring.store, ticks[i] % c.call.ring_frames
            wanted += [(ring, c.call.channel_order, slot) + tuple(r) for r in f[0]]
        launched = self._quality.launches                                                  # 4. one gate for all
        measured = self._quality(wanted) if wanted else []
        self.stats.count("quality", self._quality.launches - launched)
        self.stats.count("wait", 1 if wanted else 0)
        ready, kept, at = [], [], 0
        for i, ((cid, c, frame), f) in enumerate(zip(calls, found)):                       # 5. the books
            if i in measured_here:
                faces, alive, kept_boxes, _ = track_gate(c.host, f, measured_here[i], c._weight)
            else:
                faces, alive, kept_boxes, _ = track_gate(c.host, f, measured[at:at + len(f[0])], c._weight)
                at += len(f[0])
            kept.append(kept_boxes)
            ready.append(c.call.advance_host(faces, alive))
        scores = self._score([(c.call, win) for (_, c, _), wins in zip(calls, ready) for _, win in wins])
        out, at = {}, 0
        for (cid, c, _), wins, kept_boxes in zip(calls, ready, kept):                      # 6.
            results = [(tid, float(s)) for (tid, _), s in zip(wins, scores[at:at + len(wins)])]
            at += len(wins)
            out[cid] = c._after(results, kept_boxes)
        return out

    def _detect(self, views, sizes=None, trackers=None, tracked=None) -> List[np.ndarray]:
        """the rows of every view, in order: the views grouped by detect size where their call has one (``sizes[i]``) and by shape
        otherwise, one ``detect_views`` per 64 of a group, and the one read-back of all their rows (``_Detections``).  The views
        of one detect size, whatever their own sizes, are resized in one launch per 64 and detected where they land; their rows
        are scaled back per view."""
        if not views:
            if trackers is not None:
                extra, needed = trackers({})       # enqueued; no rows, so the trackers' records ride in the next read - unless
                if needed:                         # the tick's candidates come from them: then they are read now, in one wait
                    self._detections.read([], self.device, self.stats.count, extra)
                    tracked()
            return []
        from . import _lib
        sizes = list(sizes) if sizes is not None else [None] * len(views)
        full, views, groups, by_size = list(views), list(views), {}, {}
        for i, size in enumerate(sizes):
            if size is not None:
                by_size.setdefault(size, []).append(i)
        if by_size and self._resizer is None:
            self._resizer = FrameResizer(self.device)
        for size, members in by_size.items():
            launched = self._resizer.launches
            small = self._resizer.resize_views([full[i] for i in members], size)
            self.stats.count("resize", self._resizer.launches - launched)
            for at, i in enumerate(members):
                views[i] = small[at]
        for i, v in enumerate(views):
            groups.setdefault(("resized",) + sizes[i] if sizes[i] is not None else tuple(v.shape), []).append(i)
        order, results, places = [], [], {}
        for members in groups.values():
            for lo in range(0, len(members), _lib.YUNET_MAX_LIST):
                chunk = members[lo:lo + _lib.YUNET_MAX_LIST]
                results.append(self.detector.detect_views([views[i] for i in chunk]))
                self.stats.count("detect")
                order += chunk
                if trackers is not None:
                    places.update({i: tuple(results[-1][:2]) + (b,) for b, i in enumerate(chunk)})
        extra = trackers(places)[0] if trackers is not None else []
        read = self._detections.read(results, self.device, self.stats.count, extra)
        if extra:
            tracked()
        out = [None] * len(views)
        for i, rows in zip(order, read):
            out[i] = rows if sizes[i] is None else _scale_back(rows, full[i].shape, sizes[i])
        return out

    def _score(self, closed) -> np.ndarray:
        """``closed``: ``[(the call's ``_ServedRing``, [(frame index, record)] * clip_size)]`` in the server's order -> their scores, float32:
        one fit per window, one plan, one warp and one replay per ``max_batch`` windows, one read-back"""
        if not closed:
            return np.zeros(0, dtype=np.float32)
        if self._scoring is None:
            self._scoring = _ClosedWindows(self.network, self.clip_size, self.size, self.max_batch, self.device)
        std_points = STD_POINTS_256 * self.size / 256.0
        windows, idx = [], list(range(self.clip_size))
        for books, win in closed:
            track = _FrameTrack([rec for _, rec in win], [k % books.ring_frames for k, _ in win], books._shape)
            windows.append((books._ring.store, books.channel_order, track.frame, track, _fit(track, idx, std_points)))
        return self._scoring(len(windows), lambda first, n, run, clip: self._warp(windows[first:first + n] + [windows[first + n - 1]] * (run - n), clip),
                             count=self.stats.count)
