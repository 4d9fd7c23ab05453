"""The offline evaluator's clip loop on the MI355X: every sliding window of a face track aligned and scored on the GPU.

The reference (altfreezing/demo.py:304-339) walks over EVERY ``clip_size``-frame window of a face track, stride 1: align the
window's crops (``FasterCropAlignXRay``), normalise, forward at batch 1, sigmoid; the mean over the windows is the video's
score (:339).  Consecutive windows share all but one crop.  ``TrackScorer`` uploads each crop of a track ONCE into a device
pool, fits every window's similarity on the host with the aligner's own arithmetic (``aligner.estimate_batch_transform``), and
aligns ``batch`` windows per launch straight out of the pool (``af_warp_affine_windows_u8``, csrc/af_align.hip) into the uint8
clip buffer ``I3D8x8.forward_clips_u8`` consumes.  Nothing is synchronised before the end of the track.

Restated from the reference: the window index lists (demo.py:275-302, ``clip_windows``), the crop box and the per-face record
(demo.py:245-269 with ``get_crop_box``, test_tools/utils.py:13-24: ``crop_records``), the per-video summary (demo.py:333-340,
346-349: ``summarise``).  NOT here: grouping detections into tracks (``multiple_tracking`` / ``find_longest``: their module
imports matplotlib and filterpy, absent here, so it cannot be pinned), video decoding, the visualisation writer.  There is no
CPU fallback: without the HIP library the calls fail.
"""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from .aligner import STD_POINTS_256, _COPY_THREADS, _pool, estimate_batch_transform

_FRAME_DTYPE = np.dtype([("offset", "<i8"), ("ih", "<i4"), ("iw", "<i4"), ("x", "<i4"), ("y", "<i4")])       # af_align_frame
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


def _is_crop(im) -> bool:
    return isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3


class _Track:
    """host arrays of one track: what every window's fit and table rows are cut from"""

    def __init__(self, infos, crops):
        if len(infos) != len(crops):
            raise ValueError("evaluator: %d landmark records for %d crops" % (len(infos), len(crops)))
        for im in crops:
            if not _is_crop(im):
                raise AssertionError("aligner: images must be HxWx3 uint8 numpy arrays")
        self.crops = list(crops)
        self.n = len(crops)
        if self.n:
            self.boxes = np.array([info[3] for info in infos])            # as FasterCropAlignXRay.__call__ builds them
            self.five = np.array([info[1] for info in infos])
            self.ih = np.array([im.shape[0] for im in crops], dtype=np.int64)
            self.iw = np.array([im.shape[1] for im in crops], dtype=np.int64)
            self.bytes = (self.ih * self.iw * 3 + 15) // 16 * 16


class TrackScorer:
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
        from . import _lib                                        # fails loudly when libafhip.so is missing
        self.network = getattr(network, "network", network)
        self.clip_size, self.size, self.batch = int(clip_size), int(size), int(batch)
        if not (1 <= self.batch <= _lib.WINDOW_MAX_BATCH and 1 <= self.clip_size <= _lib.ALIGN_MAX_FRAMES):
            raise ValueError("evaluator: batch 1..%d, clip_size 1..%d" % (_lib.WINDOW_MAX_BATCH, _lib.ALIGN_MAX_FRAMES))
        if self.size % 4 or not 0 < self.size <= _lib.WINDOW_MAX_SIZE:
            raise ValueError("evaluator: size must be a multiple of 4, at most %d" % _lib.WINDOW_MAX_SIZE)
        dev = torch.device(device if device is not None else next(self.network.parameters()).device)
        if dev.type != "cuda":
            raise RuntimeError("the MI355X evaluator only runs on a HIP device (no CPU fallback); the network is on %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.pool_bytes = int(pool_bytes)
        self.std_points = STD_POINTS_256 * self.size / 256.0
        self.table_bytes = int(_lib.lib.af_window_batch_table_bytes(self.batch, self.clip_size))
        self.uploaded_bytes = 0                                   # crop bytes sent to the device by the last call
        self._pool_dev = None
        self._clips = None
        self._tables = None
        self._stage = None
        self._stage_turn = self._table_turn = 0                  # each ring is walked round-robin on its own

    # -- the partition of a track's windows into forwards -----------------------------------------
    def partition(self, n_windows: int):
        """``[(first window, windows, clips in the forward)]``: full batches, then the rest padded to a power of two"""
        out, lo = [], 0
        while lo < n_windows:
            n = min(self.batch, n_windows - lo)
            run = self.batch
            if n < self.batch:
                run = 1
                while run < n:
                    run *= 2
                run = min(run, self.batch)
            out.append((lo, n, run))
            lo += n
        return out

    # -- device state ------------------------------------------------------------------------------
    def _buffers(self):
        if self._clips is None:
            with torch.inference_mode(False):                     # buffers that outlive a caller's inference_mode block stay writable
                shape = (self.batch, self.clip_size, self.size, self.size, 3)
                self._clips = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(2)]
                # tables: pinned host + device twin + the event behind the copy out of the pinned one (the host rewrites a slot
                # only after that copy has left it).  Three slots: the host runs up to two batches ahead of the device.
                self._tables = [[torch.empty(self.table_bytes, dtype=torch.uint8, pin_memory=True),
                                 torch.empty(self.table_bytes, dtype=torch.uint8, device=self.device), None] for _ in range(3)]
                self._stage = [[torch.empty(_STAGE_BYTES, dtype=torch.uint8, pin_memory=True), None] for _ in range(3)]
        return self._clips

    def _upload(self, track: _Track, lo: int, hi: int) -> np.ndarray:
        """crops [lo, hi) of the track -> the device pool, each crop whole and once: a few pinned staging slots in turn (filled by
        the aligner's copy threads), one asynchronous copy per slot.  Returns the crops' pool offsets (index: frame - lo)."""
        from . import _lib
        offs = np.zeros(hi - lo, dtype=np.int64)
        offs[1:] = np.cumsum(track.bytes[lo:hi])[:-1]
        total = int(track.bytes[lo:hi].sum())
        if total + _POOL_SLACK > self.pool_bytes:
            raise ValueError("evaluator: %d frames (%d bytes) do not fit the pool of %d bytes" % (hi - lo, total, self.pool_bytes))
        if self._pool_dev is None or self._pool_dev.numel() < total + _POOL_SLACK:
            self._pool_dev = None                                  # give the old pool back before taking a larger one
            with torch.inference_mode(False):
                self._pool_dev = torch.empty(min(self.pool_bytes, max(total + _POOL_SLACK, 64 << 20)), dtype=torch.uint8, device=self.device)
        i = lo
        while i < hi:
            j, used = i, 0
            while j < hi and (j == i or used + int(track.bytes[j]) <= _STAGE_BYTES):
                used += int(track.bytes[j])
                j += 1
            slot = self._stage[self._stage_turn % len(self._stage)]
            self._stage_turn += 1
            if slot[1] is not None:
                slot[1].synchronize()                              # the copy of three slots ago has left the pinned buffer
            if slot[0].numel() < used:                             # one crop larger than a slot
                with torch.inference_mode(False):
                    slot[0] = torch.empty(used, dtype=torch.uint8, pin_memory=True)
            rects = (_lib.StageRect * (j - i))()
            keep = []                                              # arrays whose addresses are in `rects` live until the copies return
            for k in range(i, j):
                im = track.crops[k]
                st = im.strides
                if st[2] != 1 or st[1] != 3 or st[0] < im.shape[1] * 3:
                    im = np.ascontiguousarray(im)
                    st = im.strides
                keep.append(im)
                rects[k - i] = _lib.StageRect(im.__array_interface__["data"][0], int(offs[k - lo] - offs[i - lo]),
                                              st[0] if im.shape[0] > 1 else im.shape[1] * 3, im.shape[0], im.shape[1] * 3)
            base, n = slot[0].data_ptr(), j - i
            nt = min(_COPY_THREADS, n)
            if nt > 1 and used >= (1 << 20):
                cuts = [n * t // nt for t in range(nt + 1)]
                def part(t):
                    _lib.check(_lib.lib.af_stage_rows_u8(C.c_void_p(base), C.byref(rects, cuts[t] * C.sizeof(_lib.StageRect)), cuts[t + 1] - cuts[t]),
                               "stage_rows_u8")
                list(_pool().map(part, range(nt)))
            else:
                _lib.check(_lib.lib.af_stage_rows_u8(C.c_void_p(base), rects, n), "stage_rows_u8")
            del keep
            o = int(offs[i - lo])
            self._pool_dev[o:o + used].copy_(slot[0][:used], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            slot[1] = ev
            self.uploaded_bytes += used
            i = j
        return offs

    def _fit(self, track: _Track, idx: Sequence[int]):
        """one window's canvas, paste offsets and transform, exactly as FasterCropAlignXRay.__call__ computes them
        (faster_crop_align_xray.py:21-66)"""
        idx = np.asarray(idx)
        boxes, five = track.boxes[idx], track.five[idx]
        left_top = boxes[:, :2].min(0)
        w, h = boxes[:, 2:].max(0) - left_top
        diff = boxes[:, :2] - left_top[None]
        tfm, _ = estimate_batch_transform(five + diff[:, None, :], self.std_points)
        return tfm, int(h), int(w), diff.astype(np.int64)

    def _warp(self, track: _Track, windows, offs: np.ndarray, first_frame: int, out: torch.Tensor, fits=None):
        """table of one batch of windows (index lists into the track) -> pinned slot -> device; one launch into `out`"""
        from . import _lib
        n = len(windows)
        desc = np.zeros(n, dtype=_WINDOW_DTYPE)
        frames = np.zeros((n, self.clip_size), dtype=_FRAME_DTYPE)
        for w, idx in enumerate(windows):
            tfm, h, wd, diff = fits[w] if fits is not None else self._fit(track, idx)
            desc[w] = (np.asarray(tfm, dtype=np.float64).reshape(6), h, wd)
            ii = np.asarray(idx)
            frames["offset"][w] = offs[ii - first_frame]
            frames["ih"][w], frames["iw"][w] = track.ih[ii], track.iw[ii]
            frames["x"][w], frames["y"][w] = diff[:, 0], diff[:, 1]
        slot = self._tables[self._table_turn % len(self._tables)]
        self._table_turn += 1
        if slot[2] is not None:
            slot[2].synchronize()
        bad_w, bad_f = C.c_int32(-1), C.c_int32(-1)
        rc = _lib.lib.af_window_batch_plan_u8(desc.ctypes.data, frames.ctypes.data, n, self.clip_size, self.size, self._pool_dev.numel(),
                                              slot[0].data_ptr(), self.table_bytes, C.byref(bad_w), C.byref(bad_f))
        if rc != 0 and bad_w.value >= 0:
            f = frames[bad_w.value, bad_f.value]
            # numpy refuses new_image[y:y+ih, x:x+iw] = image for a crop that sticks out of the canvas
            raise ValueError("aligner: window %d frame %d (%dx%d at %d,%d) does not fit the %dx%d canvas"
                             % (bad_w.value, bad_f.value, f["iw"], f["ih"], f["x"], f["y"], desc[bad_w.value]["canvas_w"], desc[bad_w.value]["canvas_h"]))
        _lib.check(rc, "window_batch_plan_u8")
        used = int(_lib.lib.af_window_batch_table_bytes(n, self.clip_size))
        slot[1][:used].copy_(slot[0][:used], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        slot[2] = ev
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.lib.af_warp_affine_windows_u8(C.c_void_p(self._pool_dev.data_ptr()), C.c_void_p(slot[1].data_ptr()), n, self.clip_size,
                                                      self.size, C.c_void_p(out.data_ptr()), stream), "warp_affine_windows_u8")

    def _segments(self, track: _Track, windows):
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

    # -- public ------------------------------------------------------------------------------------
    def aligned_windows(self, infos, crops, windows) -> torch.Tensor:
        """the warp stage alone: uint8 CUDA tensor (len(windows), clip_size, size, size, 3), window ``w`` =
        ``FasterCropAlignXRay(size)(infos[windows[w]], crops[windows[w]])``.  The frames the windows use must fit the pool."""
        track = _Track(infos, crops)
        windows = [list(map(int, w)) for w in windows]
        for w in windows:
            if len(w) != self.clip_size or min(w) < 0 or max(w) >= track.n:
                raise ValueError("evaluator: a window is %d indices into the track's %d frames" % (self.clip_size, track.n))
        out = torch.empty((len(windows), self.clip_size, self.size, self.size, 3), dtype=torch.uint8, device=self.device)
        if not windows:
            return out
        self.uploaded_bytes = 0
        with torch.cuda.device(self.device):
            self._buffers()
            lo, hi = min(min(w) for w in windows), max(max(w) for w in windows) + 1
            offs = self._upload(track, lo, hi)
            for k in range(0, len(windows), self.batch):
                self._warp(track, windows[k:k + self.batch], offs, lo, out[k:k + self.batch])
        return out

    def _score_device(self, track: _Track, windows) -> List[torch.Tensor]:
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
                ids = list(range(first, first + n)) + [first + n - 1] * (run - n)
                fits = [self._fit(track, windows[k]) for k in ids[:n]]
                fits += [fits[-1]] * (run - n)
                buf = clips[turn % 2][:run]
                a = 0
                while a < run:
                    b = a
                    while b < run and seg_of[ids[b]] == seg_of[ids[a]]:
                        b += 1
                    if seg_of[ids[a]] != resident:
                        resident = seg_of[ids[a]]
                        offs = self._upload(track, segs[resident][0], segs[resident][1])
                    self._warp(track, [windows[k] for k in ids[a:b]], offs, segs[resident][0], buf[a:b], fits[a:b])
                    a = b
                with torch.inference_mode():
                    parts.append(self.network.forward_clips_u8(buf, return_scores=True)["scores"][:n])
        return parts

    def score_track(self, infos, crops) -> np.ndarray:
        """float32 fake probabilities, one per window of ``clip_windows(len(crops), clip_size)``, in that order"""
        track = _Track(infos, crops)
        self.uploaded_bytes = 0
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
        clips, frame_ids, parts = [], [], []
        self.uploaded_bytes = 0
        for track_i, ((start, end), faces) in enumerate(zip(spans, tracks)):
            assert end - start == len(faces)
            recs = crop_records(frame_shape, faces)
            crops = [frames[f][b[1]:b[3], b[0]:b[2]] for f, (b, _) in zip(range(start, end), recs)]
            track = _Track([info for _, info in recs], crops)
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
