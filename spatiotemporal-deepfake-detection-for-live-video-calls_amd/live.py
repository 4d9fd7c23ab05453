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
``_flush_and_infer`` does with a score after it exists (:340-358).  There is no CPU fallback: without the HIP library the calls fail.
"""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ._staging import is_crop
from .aligner import STD_POINTS_256
from .evaluator import RECTS, RECTS_BGR, FrameStore, WindowWarp, _clip_buffers, _FrameTrack, _network_device, _padded, get_crop_box, partition

_FORMS = {"rgb": RECTS, "bgr": RECTS_BGR}


class _DeviceSide(NamedTuple):
    """what a call keeps on the device for one frame size"""
    store: FrameStore             # the last ``ring_frames`` frames, used as a ring
    warp: WindowWarp              # the warp of the call's channel order out of it,
    clip: torch.Tensor            # into this: ``max_batch`` clips, the static input of the replayed forwards


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
        if channel_order not in _FORMS:
            raise ValueError("live: channel_order 'bgr' or 'rgb', not %r" % (channel_order,))
        self.channel_order = channel_order
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
        self._scorers = {}                 # clips per forward -> LiveScorer on the front of the ring's clip buffer
        self._done = None                  # recorded behind the last launch of every step
        self._host = None

    # -- the host side: af_realtime.py:401-505 ---------------------------------------------------------
    def step(self, frame: np.ndarray, faces: Sequence[Tuple]) -> List[Tuple]:
        if not is_crop(frame) or not frame.flags.c_contiguous:
            raise AssertionError("live: a frame must be a C-contiguous HxWx3 uint8 numpy array")
        self.frame_idx += 1
        H, W = frame.shape[:2]
        if self._shape != frame.shape:
            self._open_ring(frame.shape)
        self._store_frame(frame, self.frame_idx % self.ring_frames)
        oldest = max(self._first, self.frame_idx - self.ring_frames + 1)
        alive, ready = set(), []
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
        if not ready:
            return []
        scores = self._score(ready)                                                    # :472
        return [(tid, float(s)) for (tid, _), s in zip(ready, scores)]

    def frame_view(self, k: int) -> torch.Tensor:
        """the device (H, W, 3) uint8 view of frame ``k`` (``call.frame_idx`` is the last one), in the channel order it was captured
        in; valid on the stream ``step`` was called on until ``ring_frames`` more frames have arrived"""
        k = int(k)
        if self._ring is None or not max(self._first, self.frame_idx - self.ring_frames + 1) <= k <= self.frame_idx:
            raise ValueError("live: frame %d is not resident (frames %d .. %d are)"
                             % (k, max(self._first, self.frame_idx - self.ring_frames + 1), self.frame_idx))
        return self._ring.store.view(k % self.ring_frames)

    # -- the device side ---------------------------------------------------------------------------------
    def _open_ring(self, shape):
        """a ring for frames of `shape`; the entries of all tracks name frames of the old one and are dropped"""
        if self._ring is not None:
            torch.cuda.synchronize(self._ring.store.device)                            # nothing still reads the old ring or clip buffer
        self._ring, self._scorers = None, {}
        self._ring = self._new_ring(shape)
        self._shape, self._first = tuple(shape), self.frame_idx
        for tr in self._tracks.values():
            tr.entries = []

    def _new_ring(self, shape):
        dev = _network_device(self.network)
        with torch.cuda.device(dev):
            store = FrameStore(dev)
            store.open(shape, self.ring_frames)
            warp = WindowWarp(_FORMS[self.channel_order], store, self.clip_size, self.size, self.max_batch)
            return _DeviceSide(store, warp, _clip_buffers(1, self.max_batch, self.clip_size, self.size, dev)[0])

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
        self.uploaded_bytes += frame.nbytes

    def _scorer(self, run: int):
        from .classifier import LiveScorer
        if run not in self._scorers:
            self._scorers[run] = LiveScorer(self.network, self.clip_size, self.size, batch=run, clip=self._ring.clip[:run])
        return self._scorers[run]

    def _score(self, ready) -> np.ndarray:
        """``ready``: ``[(tid, [(frame index, record)] * clip_size)]`` -> their scores, float32: one fit per window, one launch and
        one replay per ``max_batch`` windows, one read-back"""
        ring, T = self._ring.store, self.clip_size
        std_points = STD_POINTS_256 * self.size / 256.0
        entries = [e for _, win in ready for e in win]
        track = _FrameTrack([rec for _, rec in entries], [k % self.ring_frames for k, _ in entries], self._shape)
        windows = [list(range(w * T, (w + 1) * T)) for w in range(len(ready))]
        with torch.cuda.device(ring.device):
            cur = torch.cuda.current_stream(ring.device)
            parts = []
            for first, n, run in partition(len(windows), self.max_batch):
                ids, fits = _padded(track, windows, first, n, run, std_points)
                scorer = self._scorer(run)
                self._ring.warp(track, [windows[k] for k in ids], track.frame, 0, scorer.clip, fits)
                parts.append(scorer.replay()[:n].to(torch.float32, copy=True))     # the next replay of this size overwrites its scores
            if self._host is None or self._host.numel() < len(windows):
                self._host = torch.empty(max(64, len(windows)), dtype=torch.float32, pin_memory=True)
            self._host[:len(windows)].copy_(parts[0] if len(parts) == 1 else torch.cat(parts), non_blocking=True)
            self._done.record(cur)
            cur.synchronize()
        return self._host[:len(windows)].numpy().copy()
