"""``TilePicker``: the reference's ``LargestTilePicker`` (test/capture_tile.py:55-109) and the clamp of its capture loop (:203-208)
on frames that stay on the device - the three statements behind ``CapturedFrame``'s part of that loop: ``picker.pick(frame)``, the
clamp, ``frame[t:b, l:r]``.

The pixel work - grey, GaussianBlur, Canny with its hysteresis, dilate, findContours(RETR_EXTERNAL) + boundingRect, ``_valid``, and
for the fallback absdiff, threshold, medianBlur, two dilations, contours again - is csrc/af_tile.hip: a dozen short launches on the
current stream and ONE read-back of 2.6 KB (a second one only when the first sequence found no tile and the motion sequence runs).
The host keeps what is a few integers: ``roi.var() < 50`` as ``n S2 - S1^2 < 50 n^2`` on the exact sums the device returns, the sort,
the 16:9 fit, the smoothing and the countdown.  It equals tests/tile_ref.py - the numpy restatement of OpenCV 4.x's plain C++ path,
pinned by hand-worked anchors and unpinned against cv2 itself, absent where this is built - box for box.  The integer variance test
and numpy's fp64 ``var()`` can differ only within rounding of exactly 50.  There is no CPU fallback: without the HIP library the
picker fails.  Not built: the Win32 calls, ``mss`` and the preview window of that file."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from ._staging import cuda_device
from .frames import CapturedFrame

Box = Tuple[int, int, int, int]
_MIN_W, _MIN_H, _AR_LO, _AR_HI = 200, 120, 1.2, 2.2        # LargestTilePicker._valid


class _Source:
    """a frame where the kernels read it: ``view`` the (H, W, 3) device view, its address, pitch, size and byte order"""
    __slots__ = ("view", "h", "w", "pitch", "bgr")

    def __init__(self, view: torch.Tensor, bgr: bool):
        if view.dtype != torch.uint8 or view.dim() != 3 or view.shape[2] != 3:
            raise ValueError("tile: a frame is (H, W, 3) uint8, got %s %s" % (tuple(view.shape), view.dtype))
        h, w = int(view.shape[0]), int(view.shape[1])
        if (w > 1 and view.stride(1) != 3) or view.stride(2) != 1 or (h > 1 and view.stride(0) < 3 * w):
            raise ValueError("tile: a frame has packed pixels and rows that do not overlap (strides %s)" % (tuple(view.stride()),))
        self.view, self.h, self.w, self.bgr = view, h, w, bool(bgr)
        self.pitch = int(view.stride(0)) if h > 1 else 3 * w


class TilePicker:
    """``TilePicker(device=None, channel_order="bgr")``: one call grid's speaker-tile choice, frame after frame.

    ``tiles(frame)`` -> the largest valid textured tile ``(x0, y0, x1, y1)`` or None; ``motion(frame)`` -> the 16:9 box round what
    moved since the last frame ``motion`` saw, or None (always None for the first); ``pick(frame)`` -> the reference's state machine
    over the two: smoothing with a = 0.6, ten frames of the last tile when nothing is found, then the full frame; ``motion`` runs -
    and its previous grey image is replaced - only when ``tiles`` gave nothing, as in the reference.  ``roi(frame)`` ->
    ``(view, (l, t, r, b))``: the clamped pick and the tile as a device view of the resident frame; ``CapturedFrame(view, "bgr")``
    (the picker's ``channel_order``) hands it to ``FrameStore.put``.  ``reset()`` forgets the state.

    ``frame``: a host (H, W, 3) uint8 array or a CUDA uint8 tensor, in ``channel_order`` (the reference's frames are BGR); a
    ``(FrameStore, slot)`` pair, in the store's own order; or a ``CapturedFrame``, which the capture launch converts into a slot the
    picker owns - BGRA + rect + max_w + pick is one upload and no download.  Host arrays and captured frames land in that one slot:
    the view ``roi`` returns is overwritten by the picker's next call, so consume it on the same stream before then.  Both sides of
    a frame are 8 to 8192 pixels; smaller ones are refused with ``ValueError``.

    An overflow of the device's list of 64 valid boxes or a tripped loop bound raises; it is never another answer.
    ``RealtimeCall`` re-opens its ring when the frame size changes, so a tile that moves or resizes from frame to frame is not wired
    into it here: a caller crops to a fixed size, or scores a tile that stands still."""

    def __init__(self, device=None, channel_order: str = "bgr"):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        if channel_order not in ("bgr", "rgb"):
            raise ValueError("tile: channel_order %r is not bgr or rgb" % (channel_order,))
        self.device = cuda_device(device)
        self.channel_order = channel_order
        self.params = {"min_w": _MIN_W, "min_h": _MIN_H, "ar_lo": _AR_LO, "ar_hi": _AR_HI, "area_frac": 0.10}
        self._store = None                                        # the slot host arrays and captured frames are put into
        self._ws, self._ws_shape = None, None
        self._grey, self._host = None, None
        self.launches = self.readbacks = 0
        self.reset()

    def reset(self) -> None:
        self.prev_tile: Optional[Box] = None
        self.cool = 0
        self._prev = None                                         # index of the previous grey image in self._grey, or None

    # ---- frames
    def _resident(self, frame) -> _Source:
        from .evaluator import FrameStore
        if isinstance(frame, torch.Tensor):
            if not frame.is_cuda or frame.device != self.device:
                raise ValueError("tile: a tensor frame on %s, the picker on %s" % (frame.device, self.device))
            src = _Source(frame, self.channel_order == "bgr")
        elif isinstance(frame, tuple) and len(frame) == 2 and isinstance(frame[0], FrameStore):
            store, slot = frame
            if store.device != self.device:
                raise ValueError("tile: a frame store on %s, the picker on %s" % (store.device, self.device))
            if not 0 <= int(slot) < store.capacity:
                raise ValueError("tile: slot %d of a frame store of %d" % (slot, store.capacity))
            src = _Source(store.view(int(slot)), store.channel_order == "bgr")
        elif isinstance(frame, (np.ndarray, CapturedFrame)):
            if isinstance(frame, np.ndarray) and not (frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3):
                raise ValueError("tile: a frame is (H, W, 3) uint8, got %s %s" % (frame.shape, frame.dtype))
            if self._store is None:
                self._store = FrameStore(self.device, self.channel_order)
            with torch.cuda.device(self.device):
                if self._store.shape != tuple(frame.shape):
                    self._store.open(tuple(frame.shape), 1)
                self._store.put([frame], 0)
            src = _Source(self._store.view(0), self.channel_order == "bgr")
        else:
            raise ValueError("tile: a frame is a numpy array, a CUDA tensor, a (FrameStore, slot) pair or a CapturedFrame, not %s" % type(frame).__name__)
        from . import _lib
        if not (_lib.TILE_MIN_SIDE <= src.h <= _lib.TILE_MAX_SIDE and _lib.TILE_MIN_SIDE <= src.w <= _lib.TILE_MAX_SIDE):
            raise ValueError("tile: a frame of %dx%d (both sides %d to %d)" % (src.w, src.h, _lib.TILE_MIN_SIDE, _lib.TILE_MAX_SIDE))
        return src

    def _buffers(self, src: _Source):
        from . import _lib
        if self._ws_shape != (src.h, src.w):
            if self._prev is not None:
                raise ValueError("tile: a frame of %dx%d after frames of %dx%d: reset() between sizes" % ((src.w, src.h) + self._ws_shape[::-1]))
            need = _lib.lib.af_tile_workspace_bytes(src.h, src.w)
            with torch.inference_mode(False):
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                self._grey = torch.empty((2, src.h * src.w), dtype=torch.uint8, device=self.device)
                if self._host is None:
                    self._host = torch.empty(C.sizeof(_lib.TileResult), dtype=torch.uint8, pin_memory=True)
            self._ws_shape = (src.h, src.w)
        return self._ws

    def _read(self, what: str):
        """the one read-back of a sequence: the result at the workspace's start"""
        from . import _lib
        n = C.sizeof(_lib.TileResult)
        self._host.copy_(self._ws[:n], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self.readbacks += 1
        res = _lib.TileResult.from_buffer_copy(self._host.numpy().tobytes())
        if res.error:
            raise _lib.AfError("%s: a device loop hit its bound (error word %d): the labelling is wrong" % (what, res.error))
        if res.overflow:
            raise _lib.AfError("%s: more than %d valid boxes" % (what, _lib.TILE_MAX_BOXES))
        return res

    @staticmethod
    def _source_desc(src: _Source):
        from . import _lib
        return _lib.TileSource(src.view.data_ptr(), src.pitch, src.h, src.w, int(src.bgr), 0)

    # ---- the two sequences
    def _survivors(self, src: _Source):
        """[(root, (x, y, w, h), n, S1, S2)] of the external boxes that pass ``_valid``, by ascending root"""
        from . import _lib
        p = self.params
        with torch.cuda.device(self.device):
            ws = self._buffers(src)
            params = _lib.TileParams(int(p["min_w"]), int(p["min_h"]), float(p["ar_lo"]), float(p["ar_hi"]), p["area_frac"] * src.w * src.h)
            desc = self._source_desc(src)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.af_tile_candidates_u8(C.byref(desc), C.byref(params), C.c_void_p(ws.data_ptr()), ws.numel(), None, stream),
                       "tile_candidates_u8")
            self.launches += 1
            res = self._read("tile_candidates_u8")
        return [(b.root, (b.x, b.y, b.w, b.h), b.n_px, b.s1, b.s2) for b in res.box[:res.count]]

    def _tiles(self, src: _Source) -> Optional[Box]:
        cand = []
        for _, (x, y, w, h), n, s1, s2 in self._survivors(src):
            if n == 0 or n * s2 - s1 * s1 < 50 * n * n:           # roi.size == 0 or roi.var() < 50, in Python's integers
                continue
            cand.append((w * h, (x, y, x + w, y + h)))
        if not cand:
            return None
        cand.sort(reverse=True)
        return cand[0][1]

    def _motion(self, src: _Source) -> Optional[Box]:
        from . import _lib
        H, W = src.h, src.w
        with torch.cuda.device(self.device):
            ws = self._buffers(src)
            desc = self._source_desc(src)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            first = self._prev is None
            cur = 0 if first else 1 - self._prev
            prev = None if first else C.c_void_p(self._grey[self._prev].data_ptr())
            _lib.check(_lib.lib.af_tile_motion_u8(C.byref(desc), prev, C.c_void_p(self._grey[cur].data_ptr()), 0.01 * W * H,
                                                  C.c_void_p(ws.data_ptr()), ws.numel(), None, stream), "tile_motion_u8")
            self.launches += 1
            self._prev = cur
            if first:
                return None
            res = self._read("tile_motion_u8")
        x1, y1, x2, y2 = res.x1, res.y1, res.x2, res.y2
        if x2 <= x1 or y2 <= y1:
            return None
        ar = 16 / 9
        ww, hh = x2 - x1, y2 - y1
        if ww / hh > ar:
            nh = int(ww / ar); cy = (y1 + y2) // 2; y1 = max(0, cy - nh // 2); y2 = min(H, y1 + nh)
        else:
            nw = int(hh * ar); cx = (x1 + x2) // 2; x1 = max(0, cx - nw // 2); x2 = min(W, x1 + nw)
        return (x1, y1, x2, y2)

    def _pick(self, src: _Source) -> Box:
        box = self._tiles(src) or self._motion(src)
        if box is None:
            if self.prev_tile is not None and self.cool > 0:
                self.cool -= 1
                return self.prev_tile
            return (0, 0, src.w, src.h)
        if self.prev_tile is not None:
            a = 0.6
            box = tuple(int(a * p + (1 - a) * b) for p, b in zip(self.prev_tile, box))
        self.prev_tile, self.cool = box, 10
        return box

    # ---- public
    def tiles(self, frame) -> Optional[Box]:
        return self._tiles(self._resident(frame))

    def motion(self, frame) -> Optional[Box]:
        return self._motion(self._resident(frame))

    def pick(self, frame) -> Box:
        return self._pick(self._resident(frame))

    def roi(self, frame):
        src = self._resident(frame)
        l, t, r, b = self._pick(src)
        l = max(0, min(src.w - 1, l))
        t = max(0, min(src.h - 1, t))
        r = max(l + 1, min(src.w, r))
        b = max(t + 1, min(src.h, b))
        return src.view[t:b, l:r], (l, t, r, b)
