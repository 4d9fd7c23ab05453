"""The offline evaluator on the MI355X: decoded frames in, video score out (``VideoScorer``), and the clip loop it ends in - every
sliding window of a face track aligned and scored on the GPU (``TrackScorer``).

The reference (altfreezing/demo.py:304-339) walks over EVERY ``clip_size``-frame window of a face track, stride 1: align the
window's crops (``FasterCropAlignXRay``), normalise, forward at batch 1, sigmoid; the mean over the windows is the video's
score (:339).  Consecutive windows share all but one crop.  ``TrackScorer`` uploads each crop of a track ONCE into a device
pool, fits every window's similarity on the host with the aligner's own arithmetic (``aligner.fit_window``), and
aligns ``batch`` windows per launch straight out of the pool (``af_warp_affine_windows_u8``, csrc/af_align.hip) into the uint8
clip buffer ``I3D8x8.forward_clips_u8`` consumes.  Nothing is synchronised before the end of the track.

``VideoScorer`` joins the stages in front of it (demo.py ``eval_video_demo_timed``): every decoded frame is uploaded ONCE into a
device frame store, the RetinaFace detector reads views of that store, the detections come back in one copy, the tracks are
built on the host, and the window batches are warped out of rectangles of the resident frames
(``af_warp_affine_window_rects_u8``) - no crop is cut on the host and no pixel crosses PCIe twice.

Restated from the reference: the window index lists (demo.py:275-302, ``clip_windows``), the crop box and the per-face record
(demo.py:245-269 with ``get_crop_box``, test_tools/utils.py:13-24: ``crop_records``), the per-video summary (demo.py:333-340,
346-349: ``summarise``), and the grouping of detections into tracks: ``get_valid_faces`` (test_tools/ct/detection/utils.py:75-89),
``iou`` (test_tools/ct/tracking/sort.py:30-45), ``simple_tracking`` / ``multiple_tracking`` / ``find_longest``
(test_tools/ct/operations.py:13-80).  The tracking functions are pinned by tests/golden/video_tracks.json, which
tools/gen_video_golden.py records from the reference's own functions (their modules are loaded by file path with empty stand-ins
for cv2, matplotlib, scipy and filterpy, which they import and these functions never call).  NOT here: the 68-point landmarks
(the aligner fits on the five points only and RetinaFace always supplies them, so no score depends on lm68), video decoding,
the visualisation writer.  There is no CPU fallback: without the HIP library the calls fail.
"""
import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ._staging import _COPY_THREADS, _SPLIT_BYTES, PinnedRing, _pool, crop_rect, cuda_device, is_crop, packed_rgb, stage_rects
from .aligner import STD_POINTS_256, canvas_misfit, fit_window
from .frames import CaptureConverter, ConvertedFrame, YuvConverter, YuvFrame, StoreTable

_FRAME_DTYPE = np.dtype([("offset", "<i8"), ("ih", "<i4"), ("iw", "<i4"), ("x", "<i4"), ("y", "<i4")])       # af_align_frame
_RECT_DTYPE = np.dtype([(n, "<i4") for n in ("frame", "rx", "ry", "ih", "iw", "x", "y", "reserved")])            # af_frame_rect
_WINDOW_DTYPE = np.dtype([("tfm", "<f8", (6,)), ("canvas_h", "<i4"), ("canvas_w", "<i4")])                  # af_window_desc
_POOL_SLACK = 16          # the kernel reads tap pairs as 6 bytes: 3 readable bytes behind the last crop (af_hip.h)
_STAGE_BYTES = 16 << 20   # one staging slot: about a clip's worth of crops, the size the aligner's ring was measured at


def clip_windows(T: int, clip_size: int = 32) -> List[List[int]]:
    """Index lists of the clips of a track of T frames (what demo.py:275-302 builds): every stride-1 window for
    ``T >= clip_size``; a shorter track gives ONE clip of exactly ``clip_size`` indices, the track in the middle with
    ``(clip_size - T) // 2`` indices in front and the rest behind.  Both paddings start again from the same cycle: the
    interior of the track walked backwards, ``T-2, T-3 .. 1``, over and over; a track of one or two frames has no interior
    and repeats its first frame in front and its last behind.  An empty track has no clip."""
    T, clip_size = int(T), int(clip_size)
    if T <= 0:
        return []
    if T >= clip_size:
        return [list(range(first, first + clip_size)) for first in range(T - clip_size + 1)]
    front = (clip_size - T) // 2
    back = clip_size - T - front
    if T > 2:
        cycle = lambda k: T - 2 - k % (T - 2)                       # noqa: E731
        head, tail = [cycle(k) for k in range(front)], [cycle(k) for k in range(back)]
    else:
        head, tail = [0] * front, [T - 1] * back
    return [head + list(range(T)) + tail]


def get_crop_box(shape, box, scale: float = 0.5) -> np.ndarray:
    """The crop around a detector box (what test_tools/utils.py:13-24 computes): the box rounded to integers, grown on every
    side by ``scale`` times its width / height, cut to the frame (x to ``[0, width-1]``, y to ``[0, height-1]``) and rounded
    again (half to even, as numpy rounds) - integers ``(x0, y0, x1, y1)``."""
    frame_h, frame_w = int(shape[0]), int(shape[1])
    x0, y0, x1, y1 = (float(v) for v in np.rint(np.asarray(box, dtype=np.float64).reshape(4)))
    grow_x, grow_y = scale * (x1 - x0), scale * (y1 - y0)
    sides = [min(max(x0 - grow_x, 0.0), frame_w - 1.0), min(max(y0 - grow_y, 0.0), frame_h - 1.0),
             min(max(x1 + grow_x, 0.0), frame_w - 1.0), min(max(y1 + grow_y, 0.0), frame_h - 1.0)]
    return np.rint(sides).astype(int)


def crop_records(frame_shape, track):
    """Per tracked face ``(box, lm5, lm68, ...)`` of one track (frame coordinates) the pair ``(crop_box, record)``
    (what demo.py:245-269 stores per face): ``crop_box = get_crop_box(frame_shape, box, 0.5)``, the frame's crop is
    ``frame[y0:y1, x0:x1]`` of it, and ``record = (box, lm5, lm68 relative to the crop's corner, crop_box)`` is what the
    aligner takes per frame."""
    shape = tuple(frame_shape)[:2]
    out = []
    for face in track:
        crop_box = get_crop_box(shape, face[0], scale=0.5)
        corner = crop_box[:2]
        moved = [np.asarray(face[0]).reshape(4) - np.tile(corner, 2), np.asarray(face[1]) - corner, np.asarray(face[2]) - corner]
        out.append((crop_box, (moved[0], moved[1], moved[2], crop_box)))
    return out


def summarise(frame_ids_per_clip, preds, threshold: float = 0.04) -> dict:
    """demo.py:333-340, 346-349: ``video_score`` = mean of the clips' scores (0.0 without clips), ``pred_label`` =
    ``video_score > threshold``, ``frame_res`` = per frame index the mean of the scores of the clips that contain it - a clip
    that holds a frame k times (a padded short track) counts k times, as the reference's per-frame ``append`` does."""
    preds = [float(p) for p in preds]
    seen = {}
    for ids, p in zip(frame_ids_per_clip, preds):
        for f_id in ids:
            seen.setdefault(int(f_id), []).append(p)
    video_score = float(np.mean(preds)) if len(preds) > 0 else 0.0
    return {"video_score": video_score, "pred_label": int(video_score > threshold), "preds": preds,
            "frame_res": {k: float(np.mean(v)) for k, v in seen.items()}}


def get_valid_faces(detect_results, max_count: int = 10, thres: float = 0.5, at_least: bool = False):
    """Per frame the detector's faces ``(box, lm5, score)`` that count (test_tools/ct/detection/utils.py:75-89): the first
    ``max_count`` of the frame, of those the ones with ``score >= thres`` - and, with ``at_least``, the frame's first face whatever
    its score.  Box and landmarks come back as float64 copies, the score as it was."""
    out = []
    for faces in detect_results:
        kept = []
        for j, face in enumerate(faces[:max_count]):
            if face[-1] < thres and not (j == 0 and at_least):
                continue
            box, lm, score = face
            kept.append((box.astype(np.float64), lm.astype(np.float64), score))
        out.append(kept)
    return out


def iou(a, b):
    """intersection over union of two ``[x1, y1, x2, y2]`` boxes (test_tools/ct/tracking/sort.py:30-45), in that order of operations"""
    w = np.maximum(0.0, np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]))
    h = np.maximum(0.0, np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]))
    both = w * h
    return both / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - both)


def _admitted(faces, index: int, thres: float) -> bool:
    """frame 0's gate of ``simple_tracking``: face ``index`` exists, scores at least 0.8 and overlaps no earlier face of the frame
    by more than ``thres``"""
    if len(faces) <= index or faces[index][-1] < 0.8:
        return False
    return not any(iou(faces[k][0], faces[index][0]) > thres for k in range(index))


def _successor(faces, last, thres: float):
    """the face of the next frame a track goes on with: the first one of the largest IoU with the track's last face; None (the
    track dies) on a frame without faces or when that IoU is below ``thres``"""
    if len(faces) == 0:
        return None
    overlaps = [iou(f[0], last[0]) for f in faces]
    best = 0
    for k in range(1, len(faces)):                                # the first of equals, as a stable descending sort puts it in front
        if overlaps[k] > overlaps[best]:
            best = k
    return None if overlaps[best] < thres else faces[best]


def simple_tracking(batch_landmarks, index: int = 0, thres: float = 0.5):
    """The track that starts at face ``index`` of frame 0 and takes, frame by frame, the face that overlaps its last one most
    (test_tools/ct/operations.py:13-35); None when frame 0 refuses the face or the track dies before the last frame.  A face is
    ``(box, ..., score)``; the track holds the input's own face objects."""
    track = []
    for i, faces in enumerate(batch_landmarks):
        if i == 0:
            if not _admitted(faces, index, thres):
                return None
            track.append(faces[index])
        else:
            face = _successor(faces, track[-1], thres)
            if face is None:
                return None
            track.append(face)
    return track


def multiple_tracking(batch_landmarks):
    """one ``simple_tracking`` per face of FRAME 0 (operations.py:38-45): a face that first shows up later starts no track"""
    tracks = [simple_tracking(batch_landmarks, index=i) for i in range(len(batch_landmarks[0]))]
    return [t for t in tracks if t is not None]


class _GrowingTracks:
    """``multiple_tracking(detect_res[start:start + length])`` for growing ``length`` without starting over: a greedy track over a
    longer run of frames is the track over the shorter run plus one face, and a track that has died stays dead"""

    def __init__(self, detect_res, start: int, thres: float = 0.5):
        self.res, self.start, self.thres = detect_res, start, thres
        first = detect_res[start]
        self.tracks = [[first[i]] for i in range(len(first)) if _admitted(first, i, thres)]
        self.limit = [None] * len(self.tracks)                    # the longest run of frames the track spans, None while it lives
        self.done = 1

    def upto(self, length: int):
        while self.done < length:
            faces = self.res[self.start + self.done]
            for t, track in enumerate(self.tracks):
                if self.limit[t] is None:
                    face = _successor(faces, track[-1], self.thres)
                    if face is None:
                        self.limit[t] = self.done
                    else:
                        track.append(face)
            self.done += 1
        return [track[:length] for track, limit in zip(self.tracks, self.limit) if limit is None or limit >= length]


def find_longest(detect_res):
    """The runs of frames that can be tracked when no track spans the whole video (operations.py:47-80): from ``start`` the run
    grows while the number of tracks stays what it was and is not 0; a run of more than two frames gives the span
    ``(start, un_reach_end)`` - the frame that broke the run is left out, the video's end is kept - and its FIRST track; the next
    run starts where this one ended.  Returns ``(spans, tracks)``.  The reference tracks every prefix of every run from scratch;
    here a run's tracks grow by one frame at a time, with the same results."""
    fc = len(detect_res)
    spans, all_tracks = [], []
    start = end = 0
    while start < fc - 1:
        grow = _GrowingTracks(detect_res, start)
        previous_count = -1
        for end in range(start + 2, fc + 1):
            count = len(grow.upto(end - start))
            if (count != previous_count and previous_count != -1) or count == 0:
                break
            previous_count = count
        if end - start > 2:
            un_reach_end = end - 1 if end != fc else end
            sub_tracks = grow.upto(un_reach_end - start)
            if end == fc and len(sub_tracks) == 0:
                un_reach_end = end - 1
                sub_tracks = grow.upto(un_reach_end - start)
            if len(sub_tracks) > 0:
                spans.append((start, un_reach_end))
                all_tracks.append(sub_tracks[0])
            else:
                raise NotImplementedError
            end = un_reach_end
        start = end
    return spans, all_tracks


class _Track:
    """host arrays of one track: what every window's fit and table rows are cut from"""

    def __init__(self, infos, crops):
        if len(infos) != len(crops):
            raise ValueError("evaluator: %d landmark records for %d crops" % (len(infos), len(crops)))
        for im in crops:
            if not is_crop(im):
                raise AssertionError("aligner: images must be HxWx3 uint8 numpy arrays")
        self.crops = list(crops)
        self.n = len(crops)
        if self.n:
            self.boxes = np.array([info[3] for info in infos])            # as FasterCropAlignXRay.__call__ builds them
            self.five = np.array([info[1] for info in infos])
            self.ih = np.array([im.shape[0] for im in crops], dtype=np.int64)
            self.iw = np.array([im.shape[1] for im in crops], dtype=np.int64)
            self.bytes = (self.ih * self.iw * 3 + 15) // 16 * 16

    def source(self, idx: np.ndarray, where: np.ndarray):
        """the values of ``POOL.source`` for track positions `idx` that sit at `where`: the crops' pool offsets"""
        return (where,)


class _WarpForm(NamedTuple):
    """one form of the window-batch warp (csrc/af_align.hip)"""
    item: np.dtype                # the planner's record per (window, frame)
    source: Tuple[str, ...]       # its fields that say where the frame's pixels are; a track's ``source`` gives their values
    table_bytes: str              # the C entry points: the size of a batch's table, the planner that fills it, the launch that reads it
    plan: str
    launch: str


POOL = _WarpForm(_FRAME_DTYPE, ("offset",), "af_window_batch_table_bytes", "af_window_batch_plan_u8", "af_warp_affine_windows_u8")
RECTS = _WarpForm(_RECT_DTYPE, ("frame", "rx", "ry"), "af_window_rects_table_bytes", "af_window_rects_plan_u8", "af_warp_affine_window_rects_u8")
RECTS_BGR = RECTS._replace(launch="af_warp_affine_window_rects_bgr_u8")     # the same rectangles of frames whose bytes are B, G, R
STORES = RECTS._replace(plan="af_window_rects_plan_stores_u8", launch="af_warp_affine_window_stores_u8")      # ... of several stores


def partition(n_windows: int, batch: int):
    """``[(first window, windows, clips in the forward)]``: full batches, then the rest padded to a power of two"""
    out, lo = [], 0
    while lo < n_windows:
        n = min(batch, n_windows - lo)
        run = batch
        if n < batch:
            run = 1
            while run < n:
                run *= 2
            run = min(run, batch)
        out.append((lo, n, run))
        lo += n
    return out


def _fit(track, idx: Sequence[int], std_points: np.ndarray):
    """one window's transform, canvas and paste offsets, exactly as FasterCropAlignXRay.__call__ computes them"""
    idx = np.asarray(idx)
    tfm, _, h, w, diff = fit_window(track.boxes[idx], track.five[idx], std_points)
    return tfm, int(h), int(w), diff.astype(np.int64)


def _padded(track, windows, first: int, n: int, run: int, std_points: np.ndarray):
    """window numbers and fits of one forward of ``partition``: windows [first, first + n), the last one repeated up to `run`"""
    ids = list(range(first, first + n)) + [first + n - 1] * (run - n)
    fits = [_fit(track, windows[k], std_points) for k in ids[:n]]
    return ids, fits + [fits[-1]] * (run - n)


def _network_device(network, device=None) -> torch.device:
    dev = cuda_device(device if device is not None else next(network.parameters()).device)
    if dev.type != "cuda":
        raise RuntimeError("the MI355X evaluator only runs on a HIP device (no CPU fallback); the network is on %s" % dev)
    return dev


def _clip_buffers(count: int, batch: int, clip_size: int, size: int, device) -> List[torch.Tensor]:
    with torch.inference_mode(False):                             # buffers that outlive a caller's inference_mode block stay writable
        return [torch.empty((batch, clip_size, size, size, 3), dtype=torch.uint8, device=device) for _ in range(count)]


class _Resident:
    """pixels on the device (``dev``, with the slack bytes the kernel may read behind the last one) that arrive through a ring of
    pinned staging slots; ``uploaded_bytes`` counts what was sent"""

    def __init__(self, device):
        self.device, self.dev, self.uploaded_bytes = device, None, 0
        self._stage = PinnedRing(min_bytes=_STAGE_BYTES)

    def _reserve(self, need: int, nbytes: int):
        if self.dev is None or self.dev.numel() < need:
            self.dev = None                                        # give the old buffer back before taking a larger one
            with torch.inference_mode(False):
                self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def _send(self, slot, used: int, offset: int):
        """pinned slot -> device memory at `offset`, asynchronous"""
        self.dev[offset:offset + used].copy_(slot.host[:used], non_blocking=True)
        slot.record()          # behind the copy: nothing else reads the pinned slot (the warps read `dev`, in stream order behind it)
        self.uploaded_bytes += used


class CropPool(_Resident):
    """the crops of a track, each whole and once, 16-byte aligned one behind the other in at most `pool_bytes` of device memory"""

    def __init__(self, device, pool_bytes: int):
        super().__init__(device)
        self.pool_bytes = int(pool_bytes)

    def upload(self, track: _Track, lo: int, hi: int) -> np.ndarray:
        """crops [lo, hi) of the track -> the pool: a few pinned staging slots in turn (filled by the copy threads), one
        asynchronous copy per slot.  Returns the crops' pool offsets (index: frame - lo)."""
        from . import _lib
        offs = np.zeros(hi - lo, dtype=np.int64)
        offs[1:] = np.cumsum(track.bytes[lo:hi])[:-1]
        total = int(track.bytes[lo:hi].sum())
        if total + _POOL_SLACK > self.pool_bytes:
            raise ValueError("evaluator: %d frames (%d bytes) do not fit the pool of %d bytes" % (hi - lo, total, self.pool_bytes))
        self._reserve(total + _POOL_SLACK, min(self.pool_bytes, max(total + _POOL_SLACK, 64 << 20)))
        i = lo
        while i < hi:
            j, used = i, 0
            while j < hi and (j == i or used + int(track.bytes[j]) <= _STAGE_BYTES):
                used += int(track.bytes[j])
                j += 1
            slot = self._stage.acquire(used)                       # one crop larger than a slot gets a slot of its size
            rects = (_lib.StageRect * (j - i))()
            keep = []                                              # arrays whose addresses are in `rects` live until the copies return
            for k in range(i, j):
                (address, pitch, rows, row), im = crop_rect(track.crops[k])
                keep.append(im)
                rects[k - i] = _lib.StageRect(address, int(offs[k - lo] - offs[i - lo]), pitch, rows, row)
            stage_rects(slot.host.data_ptr(), rects, j - i, used)
            del keep
            self._send(slot, used, int(offs[i - lo]))
            i = j
        return offs

    def plan_source(self):
        return self.dev.numel()


class FrameStore(_Resident):
    """`capacity` decoded frames of one `shape`, packed, slot after slot in one device buffer: a whole video, a window through
    which a longer one passes, or a ring of a call's last frames.  ``channel_order``: the byte order of a pixel in the store,
    which only a conversion into the store needs to know (``YuvFrame``s, ``CapturedFrame``s); numpy frames are stored as they come."""

    def __init__(self, device, channel_order: str = "rgb"):
        super().__init__(device)
        self.shape, self.frame_nbytes, self.capacity = None, 0, 0
        self.channel_order = channel_order
        self._yuv = self._capture = None

    def open(self, shape, capacity: int):
        self.shape, self.capacity = tuple(shape), int(capacity)
        self.frame_nbytes = int(shape[0]) * int(shape[1]) * 3
        need = self.capacity * self.frame_nbytes + _POOL_SLACK    # 3 readable bytes behind the last frame (af_hip.h)
        self._reserve(need, need)

    def put(self, frames, first_slot: int):
        """host frames -> consecutive slots of the store from `first_slot`: pinned slots in turn, each filled by the copy threads
        in bands of rows, one asynchronous copy per slot.  A frame whose pixels are not packed RGB bytes (a channel-reversed
        view) costs a strided host pass here instead of a memcpy per band.

        A list of ``YuvFrame`` (a list is all numpy or all ``YuvFrame``) is converted on the way: host planes go tightly into
        a pinned slot (1.5 to 3 bytes per pixel), one copy moves them to the slot's device twin and one ``YuvConverter`` launch
        per staging slot writes the store's slots in its ``channel_order``; device-resident planes are read where they are.
        A list of ``CapturedFrame`` goes the same way through ``af_capture_to_stores_u8``: only each frame's rectangle is staged."""
        from . import _lib
        if any(isinstance(f, ConvertedFrame) for f in frames):
            return self._put_converted(list(frames), first_slot)
        h, w = self.shape[:2]
        fb, row = self.frame_nbytes, w * 3
        per_slot = max(1, _STAGE_BYTES // fb)
        for i in range(0, len(frames), per_slot):
            chunk = frames[i:i + per_slot]
            used = len(chunk) * fb
            slot = self._stage.acquire(used)                       # one frame larger than a slot gets a slot of its size
            host = slot.host.numpy()[:used].reshape(len(chunk), h, w, 3)
            bands = max(1, min(h, -(-_COPY_THREADS // len(chunk)))) if used >= _SPLIT_BYTES else 1
            rects, n, strided = (_lib.StageRect * (len(chunk) * bands))(), 0, []
            for k, im in enumerate(chunk):
                packed = packed_rgb(im)
                for t in range(bands):
                    r0, r1 = h * t // bands, h * (t + 1) // bands
                    if packed:
                        rects[n] = _lib.StageRect(im.__array_interface__["data"][0] + r0 * im.strides[0], k * fb + r0 * row,
                                                  im.strides[0], r1 - r0, row)
                        n += 1
                    else:
                        strided.append((host[k, r0:r1], im[r0:r1]))
            if n:
                stage_rects(slot.host.data_ptr(), rects, n, used)
            if len(strided) > 1:
                list(_pool().map(lambda job: np.copyto(*job), strided))
            elif strided:
                np.copyto(*strided[0])
            self._send(slot, used, (first_slot + i) * fb)

    def _put_converted(self, frames, first_slot: int):
        """``put`` for ``YuvFrame``s or ``CapturedFrame``s: chunks of at most ``_STAGE_BYTES`` of host bytes and one launch's frames,
        each one fill, one copy and one launch"""
        kind = type(frames[0])
        if not issubclass(kind, ConvertedFrame) or not all(type(f) is kind for f in frames):
            raise ValueError("evaluator: a list of frames is all numpy arrays or all YuvFrame or all CapturedFrame")
        if kind is YuvFrame:
            converter = self._yuv = self._yuv if self._yuv is not None else YuvConverter(self.device, self._stage)
        else:
            converter = self._capture = self._capture if self._capture is not None else CaptureConverter(self.device, self._stage)
        i = 0
        while i < len(frames):
            j, used = i, 0
            while j < len(frames) and j - i < converter.max_frames and (j == i or used + frames[j].upload_bytes <= _STAGE_BYTES):
                used += frames[j].upload_bytes
                j += 1
            converter.convert([(f, self, self.channel_order, first_slot + k) for k, f in enumerate(frames[i:j], i)])
            self.uploaded_bytes += used
            i = j

    def view(self, slot: int, n: Optional[int] = None) -> torch.Tensor:
        """the device (H, W, 3) view of slot `slot`, or the (n, H, W, 3) view of the `n` slots from it on"""
        h, w = self.shape[:2]
        frames = self.dev[slot * self.frame_nbytes:(slot + (1 if n is None else n)) * self.frame_nbytes]
        return frames.view(h, w, 3) if n is None else frames.view(n, h, w, 3)

    def plan_source(self):
        from . import _lib
        h, w = self.shape[:2]
        self._desc = _lib.FrameStore(self.dev.numel(), self.frame_nbytes, w * 3, self.capacity, h, w, 0)
        return C.byref(self._desc)


class WindowWarp:
    """One form of the window-batch warp over the device pixels of `source`: fills the planner's records for a batch of windows,
    has the planner write the batch's table into a slot of its ring of tables, sends the table and launches."""

    def __init__(self, form: _WarpForm, source: Optional[_Resident], clip_size: int = 32, size: int = 224, batch: int = 16, device=None):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        self.form, self.source, self.device = form, source, source.device if device is None else device
        self.clip_size, self.size, self.batch = int(clip_size), int(size), int(batch)
        if not (1 <= self.batch <= _lib.WINDOW_MAX_BATCH and 1 <= self.clip_size <= _lib.ALIGN_MAX_FRAMES):
            raise ValueError("evaluator: batch 1..%d, clip_size 1..%d" % (_lib.WINDOW_MAX_BATCH, _lib.ALIGN_MAX_FRAMES))
        if self.size % 4 or not 0 < self.size <= _lib.WINDOW_MAX_SIZE:
            raise ValueError("evaluator: size must be a multiple of 4, at most %d" % _lib.WINDOW_MAX_SIZE)
        self._table_bytes, self._plan_fn, self._launch = (getattr(_lib.lib, name) for name in (form.table_bytes, form.plan, form.launch))
        self.table_bytes = int(self._table_bytes(self.batch, self.clip_size))
        self.tables = PinnedRing(min_bytes=self.table_bytes)      # three slots: the host runs up to two batches ahead of the device

    def _records(self, n: int):
        return np.zeros(n, dtype=_WINDOW_DTYPE), np.zeros((n, self.clip_size), dtype=self.form.item)

    @staticmethod
    def _fill(desc, items, w: int, fit, ih, iw):
        """what every form's records of window `w` hold: the transform, the canvas, the crops' sizes and paste offsets"""
        tfm, h, wd, diff = fit
        desc[w] = (np.asarray(tfm, dtype=np.float64).reshape(6), h, wd)
        items["ih"][w], items["iw"][w] = ih, iw
        items["x"][w], items["y"][w] = diff[:, 0], diff[:, 1]

    def __call__(self, track, windows, offs: np.ndarray, first_frame: int, out: torch.Tensor, fits):
        """windows (index lists into the track, whose frame j sits at ``offs[j - first_frame]`` of the source) with their `fits`
        -> table -> pinned slot -> device; one launch into `out`"""
        desc, items = self._records(len(windows))
        for w, (idx, fit) in enumerate(zip(windows, fits)):
            ii = np.asarray(idx)
            self._fill(desc, items, w, fit, track.ih[ii], track.iw[ii])
            for name, values in zip(self.form.source, track.source(ii, offs[ii - first_frame])):
                items[name][w] = values
        self._send(desc, items, (self.source.plan_source(),), (C.c_void_p(self.source.dev.data_ptr()),), out)

    def _plan(self, desc, items, where: tuple, table: int):
        """the filled records -> the batch's table at host address `table` (host only).  The planner names the (window, frame) it
        refuses, whatever its reason: the aligner's canvas-misfit ``ValueError`` only if that one really misfits its canvas."""
        from . import _lib
        bad_w, bad_f = C.c_int32(-1), C.c_int32(-1)
        rc = self._plan_fn(desc.ctypes.data, items.ctypes.data, len(desc), self.clip_size, self.size, *where, table, self.table_bytes,
                           C.byref(bad_w), C.byref(bad_f))
        if rc != 0 and bad_w.value >= 0:
            f, d = items[bad_w.value, bad_f.value], desc[bad_w.value]
            if f["x"] < 0 or f["y"] < 0 or f["x"] + f["iw"] > d["canvas_w"] or f["y"] + f["ih"] > d["canvas_h"]:
                canvas_misfit(bad_f.value, f["iw"], f["ih"], f["x"], f["y"], d["canvas_w"], d["canvas_h"], window=bad_w.value)
        _lib.check(rc, self.form.plan[3:])

    def _send(self, desc, items, where: tuple, pixels: tuple, out: torch.Tensor):
        """everything behind the filled records, for every form: table slot, plan, copy, launch.  `where` / `pixels`: what the
        form's planner takes for the place of the pixels, and what its launch takes in front of the table"""
        from . import _lib
        slot = self.tables.acquire(self.table_bytes, self.device)
        self._plan(desc, items, where, slot.host.data_ptr())
        used = int(self._table_bytes(len(desc), self.clip_size))
        slot.dev[:used].copy_(slot.host[:used], non_blocking=True)
        # behind the copy, not the launch: the host rewrites only the pinned table; its twin is next written by the copy of three
        # batches later, which the stream orders behind this launch
        slot.record()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self._launch(*pixels, C.c_void_p(slot.dev.data_ptr()), len(desc), self.clip_size, self.size, C.c_void_p(out.data_ptr()), stream),
                   self.form.launch[3:])


class StoresWarp(WindowWarp):
    """the window-batch warp out of several frame stores (``af_window_rects_plan_stores_u8`` /
    ``af_warp_affine_window_stores_u8``): ``warp(windows, out)`` with ``windows = [(store, channel_order, slots, track, fit)]`` -
    ``track`` a ``_FrameTrack`` of the window's ``clip_size`` frames, which sit in ``slots`` of ``store`` - plans one table, sends
    it through a ring of pinned slots and launches once.  ``launches`` counts the launches."""

    def __init__(self, device, clip_size: int, size: int, batch: int):
        super().__init__(STORES, None, clip_size, size, batch, device)
        self.launches = 0

    def __call__(self, windows, out: torch.Tensor):
        desc, items = self._records(len(windows))
        table = StoreTable()
        for w, (store, order, slots, track, fit) in enumerate(windows):
            self._fill(desc, items, w, fit, track.ih, track.iw)
            items["frame"][w], items["rx"][w], items["ry"][w], items["reserved"][w] = slots, track.rx, track.ry, table.index(store, order)
        with torch.cuda.device(self.device):
            self._send(desc, items, (table.array(), len(table.refs)), (), out)
        self.launches += 1


class _WindowScorer:
    """What TrackScorer and VideoScorer share: the double clip buffer, the segments of a track that does not fit the device memory
    it may use, and the loop that enqueues a track - ``partition``, the per-window fits, the warps, the forwards - over the
    ``WindowWarp`` and the device pixels (``source``) it has.  A subclass says how a track's pixels get there: ``_upload`` brings
    frames [lo, hi) of a track onto the device and returns where each one sits."""

    def __init__(self, network, form: _WarpForm, source: _Resident, clip_size: int, size: int, batch: int, pool_bytes: int):
        self.network = getattr(network, "network", network)
        self.device = source.device
        self.source = source
        self.warp = WindowWarp(form, source, clip_size, size, batch)
        self.clip_size, self.size, self.batch = self.warp.clip_size, self.warp.size, self.warp.batch
        self.pool_bytes = int(pool_bytes)
        self.std_points = STD_POINTS_256 * self.size / 256.0
        self._clips = None

    @property
    def uploaded_bytes(self) -> int:
        """pixel bytes sent to the device by the last call"""
        return self.source.uploaded_bytes

    def partition(self, n_windows: int):
        return partition(n_windows, self.batch)

    def _buffers(self):
        if self._clips is None:                                   # two: one batch is warped while the forward of the one before reads its own
            self._clips = _clip_buffers(2, self.batch, self.clip_size, self.size, self.device)
        return self._clips

    def _segments(self, track, windows):
        """[(first frame, end frame, windows)]: the whole track if its crops fit the pool, else runs of consecutive windows whose
        frames fit - the next run starts at the next window, so neighbours overlap by clip_size - 1 frames"""
        room = self.pool_bytes - _POOL_SLACK
        if track.bytes.sum() <= room or len(windows) <= 1:
            return [(0, track.n, windows)]
        segs, k = [], 0
        while k < len(windows):
            lo = windows[k][0]
            hi, used, j = lo, 0, k
            while j < len(windows):                                # stride-1 windows: window j ends one frame after window j - 1
                end = windows[j][-1] + 1
                grow = int(track.bytes[hi:end].sum())
                if used + grow > room:
                    break
                used, hi, j = used + grow, end, j + 1
            if j == k:
                raise ValueError("evaluator: one window of %d frames does not fit the pool of %d bytes" % (self.clip_size, self.pool_bytes))
            segs.append((lo, hi, windows[k:j]))
            k = j
        return segs

    def _aligned(self, track, windows) -> torch.Tensor:
        """the warp stage alone for windows (index lists) of one track whose frames fit the device memory at once"""
        windows = [list(map(int, w)) for w in windows]
        for w in windows:
            if len(w) != self.clip_size or min(w) < 0 or max(w) >= track.n:
                raise ValueError("evaluator: a window is %d indices into the track's %d frames" % (self.clip_size, track.n))
        out = torch.empty((len(windows), self.clip_size, self.size, self.size, 3), dtype=torch.uint8, device=self.device)
        if not windows:
            return out
        with torch.cuda.device(self.device):
            lo, hi = min(min(w) for w in windows), max(max(w) for w in windows) + 1
            offs = self._upload(track, lo, hi)
            for k in range(0, len(windows), self.batch):
                batch = windows[k:k + self.batch]
                self.warp(track, batch, offs, lo, out[k:k + self.batch], [_fit(track, idx, self.std_points) for idx in batch])
        return out

    def _score_device(self, track, windows) -> List[torch.Tensor]:
        """enqueue everything for the windows of one track; returns the per-forward score tensors (device, unsynchronised)"""
        parts = []
        with torch.cuda.device(self.device):
            clips = self._buffers()
            segs = self._segments(track, windows)
            seg_of = [s for s, (_, _, ws) in enumerate(segs) for _ in ws]
            resident, offs = -1, None
            # the forwards follow partition() of ALL windows, wherever the pool's segments end (a batch size picks the engine's
            # kernels, so the scores would otherwise move with the cuts): a batch that straddles a cut is warped in two launches,
            # one before and one after the next segment's upload, into the same clip buffer
            for turn, (first, n, run) in enumerate(self.partition(len(windows))):
                ids, fits = _padded(track, windows, first, n, run, self.std_points)
                buf = clips[turn % len(clips)][:run]
                a = 0
                while a < run:
                    b = a
                    while b < run and seg_of[ids[b]] == seg_of[ids[a]]:
                        b += 1
                    if seg_of[ids[a]] != resident:
                        resident = seg_of[ids[a]]
                        offs = self._upload(track, segs[resident][0], segs[resident][1])
                    self.warp(track, [windows[k] for k in ids[a:b]], offs, segs[resident][0], buf[a:b], fits[a:b])
                    a = b
                with torch.inference_mode():
                    parts.append(self.network.forward_clips_u8(buf, return_scores=True)["scores"][:n])
        return parts

    def _score_tracks(self, tracks, threshold: float) -> dict:
        """demo.py:304-340, 346-349 over ``(first frame, track)`` pairs: all tracks are enqueued before the first score is read
        back - the only synchronisation - and summarised"""
        clips, frame_ids, parts = [], [], []
        for track_i, (start, track) in enumerate(tracks):
            windows = clip_windows(track.n, self.clip_size)
            if not windows:
                continue
            clips += [[(track_i, j) for j in w] for w in windows]
            frame_ids += [[start + j for j in w] for w in windows]
            parts += self._score_device(track, windows)
        preds = torch.cat(parts).float().cpu().numpy() if parts else np.zeros(0, dtype=np.float32)
        res = summarise(frame_ids, preds, threshold)
        res["clips"] = clips
        return res


class TrackScorer(_WindowScorer):
    """``TrackScorer(network)``: all sliding windows of a face track, aligned and scored on the GPU.

    ``network``: an ``I3D8x8`` on a HIP device in eval mode, or a ``Classifier`` (its ``.network`` is used).  One scorer works on
    the stream that is current when it is called and owns its pool, clip buffers and tables; the network's engines are not
    shared between streams, so scorers that run at the same time on different streams each take a network of their own.

    ``score_track(infos, crops)`` equals, per window ``w`` of ``clip_windows(len(crops), clip_size)``,
    ``sigmoid(classifier(normalise(FasterCropAlignXRay(size)(infos[w], crops[w]))))``: the fits are the aligner's own doubles,
    the warp is bit-exact with its kernel, and the forward is ``forward_clips_u8`` on batches of ``partition(n_windows)``.

    The last batch of a track is usually short.  It is padded by repeating its last window up to the next power of two (at most
    ``batch``): the forward then only ever runs at 1, 2, 4 ... ``batch`` clips - a handful of engines, each a few GB of
    activations - and wastes less than half a batch; a clip's score does not depend on its position in a batch.

    ``pool_bytes`` bounds the device memory for crops (default 512 MiB, about a thousand 420-pixel crops).  A longer track is cut
    into segments that overlap by ``clip_size - 1`` frames; the scores do not depend on where the cuts fall."""

    def __init__(self, network, clip_size: int = 32, size: int = 224, batch: int = 16, device: Optional[torch.device] = None,
                 pool_bytes: int = 512 << 20):
        pool = CropPool(_network_device(getattr(network, "network", network), device), pool_bytes)
        super().__init__(network, POOL, pool, clip_size, size, batch, pool_bytes)

    def _upload(self, track: _Track, lo: int, hi: int) -> np.ndarray:
        return self.source.upload(track, lo, hi)

    # -- public ------------------------------------------------------------------------------------
    def aligned_windows(self, infos, crops, windows) -> torch.Tensor:
        """the warp stage alone: uint8 CUDA tensor (len(windows), clip_size, size, size, 3), window ``w`` =
        ``FasterCropAlignXRay(size)(infos[windows[w]], crops[windows[w]])``.  The frames the windows use must fit the pool."""
        self.source.uploaded_bytes = 0
        return self._aligned(_Track(infos, crops), windows)

    def score_track(self, infos, crops) -> np.ndarray:
        """float32 fake probabilities, one per window of ``clip_windows(len(crops), clip_size)``, in that order"""
        track = _Track(infos, crops)
        self.source.uploaded_bytes = 0
        windows = clip_windows(track.n, self.clip_size)
        if not windows:
            return np.zeros(0, dtype=np.float32)
        parts = self._score_device(track, windows)
        return torch.cat(parts).float().cpu().numpy()             # the only synchronisation of the track

    def score_video(self, frame_shape, frames, tracks, spans, threshold: float = 0.04) -> dict:
        """demo.py:245-340, 346-349 for the tracks of one video.  ``tracks[i]``: the tracked faces ``(box, lm5, lm68, ...)`` of
        track i, one per frame of ``range(*spans[i])``; ``frames``: the decoded HxWx3 uint8 frames.  Returns ``video_score``,
        ``pred_label``, ``preds`` (per clip, track by track), ``clips`` (per clip its ``(track, index in track)`` pairs) and
        ``frame_res`` (``summarise``).  All tracks are enqueued before the first score is read back."""
        self.source.uploaded_bytes = 0

        def host_cut_tracks():
            for (start, end), faces in zip(spans, tracks):
                assert end - start == len(faces)
                recs = crop_records(frame_shape, faces)
                crops = [frames[f][b[1]:b[3], b[0]:b[2]] for f, (b, _) in zip(range(start, end), recs)]
                yield start, _Track([info for _, info in recs], crops)
        return self._score_tracks(host_cut_tracks(), threshold)


DETECT_BATCH = 50         # test_tools/common.py:82: the detector sees partition(frames, 50)
_NO_LM68 = np.zeros((0, 2))


class _FrameTrack:
    """host arrays of one track whose crops are rectangles of decoded frames: ``frame_ids[j]`` is the frame of track position j
    and ``rects[j]`` = (x0, y0, x1, y1) the rectangle ``frame[y0:y1, x0:x1]`` (default: the record's crop box, cut to the frame as
    a numpy slice cuts it)"""

    def __init__(self, infos, frame_ids, frame_shape, rects=None):
        if len(infos) != len(frame_ids):
            raise ValueError("evaluator: %d landmark records for %d frames" % (len(infos), len(frame_ids)))
        self.n = len(infos)
        self.frame = np.asarray(list(frame_ids), dtype=np.int64)
        if self.n:
            self.boxes = np.array([info[3] for info in infos])
            self.five = np.array([info[1] for info in infos])
            r = np.asarray(self.boxes if rects is None else rects, dtype=np.int64).reshape(self.n, 4)
            if (r < 0).any():
                raise ValueError("evaluator: a crop rectangle with a negative coordinate")
            self.rx, self.ry = r[:, 0], r[:, 1]
            self.iw = np.minimum(r[:, 2], int(frame_shape[1])) - self.rx
            self.ih = np.minimum(r[:, 3], int(frame_shape[0])) - self.ry
            self.bytes = np.full(self.n, int(frame_shape[0]) * int(frame_shape[1]) * 3, dtype=np.int64)

    def source(self, idx: np.ndarray, where: np.ndarray):
        """the values of ``RECTS.source`` for track positions `idx` whose frames sit in the store's slots `where`"""
        return where, self.rx[idx], self.ry[idx]


class VideoScorer(_WindowScorer):
    """``VideoScorer(detector, network).score(frames)``: the reference's offline evaluator (demo.py ``eval_video_demo_timed``) from
    decoded frames to the video's score, on ONE device-resident copy of the frames.

    ``detector``: a ``retinaface.FaceDetector`` on the network's device (None when detections are always handed in);
    ``network``: as for ``TrackScorer``, whose fit, partition, padding, table ring and double clip buffer this class shares.

    ``score`` stages the frames through pinned slots into a device frame store, ``DETECT_BATCH`` frames at a time, and calls
    ``detector.detect_device(max_count=10, min_score=0.5)`` on views of the store as each batch lands - the host stages the next
    batch while the device works on this one.  The detections come back in one copy (the first of the call's two waits), are
    grouped into tracks on the host (``multiple_tracking``, else ``find_longest``) and every window of every track is warped out
    of rectangles of the resident frames (``af_warp_affine_window_rects_u8``) and scored; reading the scores back is the second
    wait.  Everything is enqueued on the stream that is current when ``score`` is called.  (Refilling a pinned slot waits for the
    copy that last left it, as every staging ring does.)

    ``scale_detect=True`` detects as the reference's ``FaceDetector.scale_detect`` does: every detector batch is resized out of the
    store to ``retinaface.scale_detect_size`` (half size up to 1920 on the long side) in one launch (``frames.FrameResizer``),
    detected there with ``min_score=0.5`` and no cap on the boxes, and on the host the rows are scaled back and filtered
    (``post_detect`` / ``check_valid``) before the first 10 are kept - on score-sorted rows that is ``get_valid_faces`` behind
    ``scale_detect``.  Tracks, warps (out of the full-size store) and scores are untouched by it.

    ``frame_bytes`` bounds the frame store.  A video that does not fit is detected batch by batch through the store and then
    scored track by track in frame segments that overlap by ``clip_size - 1`` and are uploaded again from the host frames; the
    scores do not depend on where the cuts fall.  ``uploaded_bytes`` is what the last call sent to the device."""

    def __init__(self, detector, network, clip_size: int = 32, size: int = 224, batch: int = 16, frame_bytes: int = 4 << 30,
                 scale_detect: bool = False):
        super().__init__(network, RECTS, FrameStore(_network_device(getattr(network, "network", network))), clip_size, size, batch, frame_bytes)
        self.detector = detector
        self.scale_detect, self._resizer = bool(scale_detect), None
        if detector is not None and torch.device(detector.device) != self.device:
            raise ValueError("evaluator: the detector is on %s, the network on %s" % (detector.device, self.device))
        self._frames, self._resident = None, False

    # -- the frame store -----------------------------------------------------------------------------
    def _open_store(self, frames):
        """checks the frames and sizes the store for them: all of them when ``frame_bytes`` allows, else as many as it holds"""
        shape = tuple(frames[0].shape)
        if any(isinstance(im, YuvFrame) for im in frames):
            if not all(isinstance(im, YuvFrame) and im.shape == shape for im in frames):
                raise ValueError("evaluator: a list of frames is all numpy arrays or all YuvFrame, of one size")
        else:
            for im in frames:
                if not is_crop(im) or im.shape != shape:
                    raise AssertionError("evaluator: frames must be HxWx3 uint8 numpy arrays of one size")
        nbytes = shape[0] * shape[1] * 3
        capacity = min(len(frames), (self.pool_bytes - _POOL_SLACK) // nbytes)
        self._frames, self._resident = frames, capacity == len(frames)
        if capacity < min(len(frames), max(DETECT_BATCH if self.detector is not None else 1, self.clip_size)):
            raise ValueError("evaluator: frame_bytes %d holds %d frames of %d bytes, fewer than a detector batch or a window"
                             % (self.pool_bytes, capacity, nbytes))
        self.source.open(shape, capacity)

    def _upload(self, track: _FrameTrack, lo: int, hi: int) -> np.ndarray:
        """the store slots of track positions [lo, hi): where the frames already sit when the whole video is resident, else the
        segment's frames are uploaded again into the front of the store"""
        if self._resident:
            return track.frame[lo:hi]
        if hi - lo > self.source.capacity:
            raise ValueError("evaluator: %d frames do not fit the frame store of %d" % (hi - lo, self.source.capacity))
        self.source.put([self._frames[f] for f in track.frame[lo:hi]], 0)
        return np.arange(hi - lo, dtype=np.int64)

    def _segments(self, track: _FrameTrack, windows):
        return [(0, track.n, windows)] if self._resident else super()._segments(track, windows)

    # -- the detector stage --------------------------------------------------------------------------
    def _detect(self):
        """upload + detect in ``partition(frames, DETECT_BATCH)`` batches, one read-back: ``get_valid_faces(detector.detect(batch))``
        per batch, bit for bit"""
        if self.detector is None:
            raise ValueError("evaluator: no detector and no detections")
        if self.scale_detect:
            return self._detect_scaled()
        n, store = len(self._frames), self.source
        found = []
        for lo in range(0, n, DETECT_BATCH):
            hi = min(lo + DETECT_BATCH, n)
            first = lo if self._resident else 0                    # not resident: every batch passes through the front of the store
            store.put(self._frames[lo:hi], first)
            rows, counts = self.detector.detect_device(store.view(first, hi - lo), max_count=10, min_score=0.5)
            found.append(torch.cat([rows.view(torch.int32).reshape(hi - lo, -1), counts.reshape(hi - lo, 1)], 1))    # bits, no arithmetic
        back = torch.cat(found).cpu().numpy()                      # rows and counts of all frames in one copy: the first wait
        counts = back[:, -1]
        rows = np.ascontiguousarray(back[:, :-1]).view(np.float32).reshape(n, -1, 15)
        return [[(rows[b, i, :4].astype(np.float64), rows[b, i, 5:15].reshape(5, 2).astype(np.float64), rows[b, i, 4])
                 for i in range(int(counts[b]))] for b in range(n)]

    def _detect_scaled(self):
        """``_detect`` on frames resized to ``scale_detect_size``: ``get_valid_faces(detector.scale_detect(batch))`` per batch.  The
        device cuts at score 0.5 and caps nothing (a cap of 10 in front of ``check_valid`` could drop a face the reference keeps);
        the counts come back first, then the rows up to the largest count."""
        from .frames import FrameResizer
        from .retinaface import post_detect, scale_detect_scale, scale_detect_size
        n, store = len(self._frames), self.source
        h, w = store.shape[:2]
        dw, dh = scale_detect_size(h, w)
        if dw < 1 or dh < 1:
            raise ValueError("evaluator: scale_detect would detect frames of %dx%d at %dx%d" % (w, h, dw, dh))
        if self._resizer is None:
            self._resizer = FrameResizer(self.device)
        found = []
        for lo in range(0, n, DETECT_BATCH):
            hi = min(lo + DETECT_BATCH, n)
            first = lo if self._resident else 0
            store.put(self._frames[lo:hi], first)
            small = self._resizer.resize(store.view(first, hi - lo), (dw, dh))
            found.append(self.detector.detect_device(small, min_score=0.5))
        counts = torch.cat([c for _, c in found]).cpu().numpy()    # the first wait
        most = max(1, int(counts.max()))
        rows = torch.cat([r[:, :most] for r, _ in found]).cpu().numpy()
        faces = [[(rows[b, i, :4].copy(), rows[b, i, 5:15].reshape(5, 2).copy(), rows[b, i, 4]) for i in range(int(counts[b]))] for b in range(n)]
        return get_valid_faces(post_detect(faces, scale_detect_scale(h, w), w, h), max_count=10, thres=0.5)

    # -- public ------------------------------------------------------------------------------------
    def aligned_windows(self, frames, frame_ids, infos, windows, rects=None) -> torch.Tensor:
        """the warp stage alone: uint8 CUDA tensor (len(windows), clip_size, size, size, 3).  Track position j is the rectangle
        ``rects[j]`` = (x0, y0, x1, y1) (default: the crop box ``infos[j][3]``) of ``frames[frame_ids[j]]``; window ``w`` equals
        ``TrackScorer.aligned_windows`` on the crops ``frame[y0:y1, x0:x1]`` cut on the host.  All frames are uploaded, so they
        must fit ``frame_bytes``."""
        frames = list(frames)
        self.source.uploaded_bytes = 0
        with torch.cuda.device(self.device):
            self._open_store(frames)
            if not self._resident:
                raise ValueError("evaluator: %d frames do not fit frame_bytes %d" % (len(frames), self.pool_bytes))
            track = _FrameTrack(infos, frame_ids, self.source.shape, rects)
            if track.n and (track.frame.min() < 0 or track.frame.max() >= len(frames)):
                raise ValueError("evaluator: a frame index outside the %d frames" % len(frames))
            self.source.put(frames, 0)
            return self._aligned(track, windows)

    def score(self, frames, detections=None, threshold: float = 0.04) -> dict:
        """``frames``: the decoded HxWx3 uint8 frames of one video, all of one size (a channel-reversed view, as
        ``grab_all_frames(cvt=True)`` returns, is taken as it is).  ``detections``: per frame the faces ``(box, lm5, score)``, the
        first value ``detect_all`` returns and demo.py caches; given, they replace the detector stage.  Returns what
        ``TrackScorer.score_video`` returns (``video_score``, ``pred_label``, ``preds``, ``clips``, ``frame_res``) for the tracks
        demo.py:235-238 builds, plus ``detections``, ``tracks`` (each face ``(box, lm5, score)``) and ``spans``."""
        frames = list(frames)
        self.source.uploaded_bytes = 0
        if not frames:
            res = summarise([], [], threshold)
            res.update(clips=[], detections=[], tracks=[], spans=[])
            return res
        with torch.cuda.device(self.device):
            self._open_store(frames)
            if detections is None:
                detections = self._detect()
            else:
                detections = [list(faces) for faces in detections]
                if len(detections) != len(frames):
                    raise ValueError("evaluator: detections for %d frames, %d frames" % (len(detections), len(frames)))
                if self._resident:
                    self.source.put(frames, 0)
            tracks = multiple_tracking(detections)
            spans = [(0, len(detections))] * len(tracks)
            if len(tracks) == 0:
                spans, tracks = find_longest(detections)

            def resident_tracks():
                for (start, end), faces in zip(spans, tracks):
                    assert end - start == len(faces)
                    recs = crop_records(self.source.shape, [(f[0], f[1], _NO_LM68, f[-1]) for f in faces])
                    yield start, _FrameTrack([info for _, info in recs], range(start, end), self.source.shape)
            res = self._score_tracks(resident_tracks(), threshold)
        res.update(detections=detections, tracks=tracks, spans=spans)
        self._frames = None                                        # the host frames are the caller's
        return res
