"""Frames on their way into and out of the frame stores: YUV frames in, downscaled detector batches out.

YUV frames as a caller has them - what a WebRTC stack (I420), a hardware decoder (NV12, P010), a webcam (YUY2 / UYVY), an MJPEG
decoder (full-range planar 4:2:2 / 4:4:4) or ffmpeg / PyAV hands over - and their way into the frame stores: ``YuvFrame`` names the
planes, the colour matrix and the range, ``YuvConverter`` stages host planes through one pinned slot and one copy and converts every
frame of a call to it, whatever its size, format, depth, colour, store and byte order, in one launch per ``AF_YUV_MAX_FRAMES`` frames:
``af_yuv420_to_rgb_u8`` (csrc/af_yuv.hip) when all frames are 8-bit 4:2:0 at OpenCV's colour, else ``af_yuv_to_rgb_ex_u8``
(csrc/af_yuv_formats.hip).

The conversion has OpenCV's fixed-point form; at BT.601 limited range it is OpenCV's ``cvtColor(..., COLOR_YUV2BGR_NV12 / _I420 /
_YUY2 ...)``, the other tables (BT.709, full range, 10-bit) are derived in include/af_hip.h.  One (U, V) per chroma block, nothing
interpolated.  It equals the numpy statements tests/yuv_ref.py and tests/yuv_formats_ref.py byte for byte and is unpinned against cv2
itself, which is absent where this is built.  Not built: NV24 / NV42, packed 10-bit, 12-bit, BT.2020, chroma siting / interpolation.
There is no CPU fallback: without the HIP library the conversion fails.

``FrameResizer`` is the other direction: ``cv2.resize(frame, (dw, dh))`` (the default ``INTER_LINEAR``) of frames that already sit on
the device - slots of frame stores, views, a batch - into one detector batch, in one launch of ``af_resize_frames_u8`` per
``AF_RESIZE_MAX_FRAMES`` frames (csrc/af_resize.hip).  It equals tests/resize_ref.py, the numpy restatement of OpenCV's plain C++
path, byte for byte; that restatement is unpinned against cv2 itself, and an IPP-enabled OpenCV may differ from it.

``CapturedFrame`` is the entry for what a screen or window capture hands over: a BGRA (RGBA, BGR, RGB) bitmap, its client rectangle
and the reference's ``max_w`` rule.  ``CaptureConverter`` puts every such frame of a call into its store slot in one launch of
``af_capture_to_stores_u8`` per ``AF_CAPTURE_MAX_FRAMES`` frames (csrc/af_capture.hip), which drops the alpha byte, cuts the
rectangle, orders the bytes as the store has them and reduces with ``cv2.INTER_AREA``'s arithmetic (OpenCV 4.x resize.cpp).  It equals
tests/capture_ref.py byte for byte; that statement is pinned by hand-worked anchors and by its tie to tests/quality_ref.py's
``half_size``, not against cv2 itself.  Not built: upscaling, ``INTER_AREA`` inside ``FrameResizer``, bottom-up bitmaps, 16-bit and
float captures.  There is no CPU fallback here either."""
import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._staging import _COPY_THREADS, _SPLIT_BYTES, PinnedRing, cuda_device, stage_rects

# the 8-bit 4:2:0 formats of ``af_yuv420_to_rgb_u8``: format -> (chroma is one interleaved plane, the first chroma byte / plane in memory is V)
FORMATS = {"nv12": (True, False), "nv21": (True, True), "i420": (False, False), "yv12": (False, True)}
# every format ``YuvFrame`` takes -> (AF_YUV_LAYOUT_ code, component order code) of ``af_yuv_to_rgb_ex_u8`` (include/af_hip.h)
YUV_FORMATS = {"nv12": (1, 0), "nv21": (1, 1), "i420": (0, 0), "yv12": (0, 1), "i422": (2, 0), "nv16": (3, 0), "i444": (4, 0),
               "yuy2": (5, 0), "uyvy": (5, 1), "yvyu": (5, 2), "p010": (6, 0), "i010": (7, 0)}
# layout code -> (planes: "planar" (y, u, v), "semi" (y, uv) or "packed" (y alone), rows of Y per chroma row, pixels per (U, V) in a row,
# bytes per sample)
YUV_LAYOUTS = {0: ("planar", 2, 2, 1), 1: ("semi", 2, 2, 1), 2: ("planar", 1, 2, 1), 3: ("semi", 1, 2, 1), 4: ("planar", 1, 1, 1),
               5: ("packed", 1, 2, 1), 6: ("semi", 2, 2, 2), 7: ("planar", 2, 2, 2)}
MATRICES = {"bt601": 0, "bt709": 1}
_FRAME_ALIGN = 16         # a frame's planes start on a 16-byte boundary of the staging slot: aligned vector loads for the usual widths


def _plane(name: str, p, sample: int = 1):
    """checks one plane of `sample`-byte samples; returns (is a device tensor, rows, row bytes, pitch in bytes)"""
    np_type, torch_type = (np.uint8, torch.uint8) if sample == 1 else (np.uint16, torch.uint16)
    if isinstance(p, np.ndarray):
        dev, dtype_ok, strides = False, p.dtype == np_type, p.strides
    elif isinstance(p, torch.Tensor):
        if not p.is_cuda:
            raise ValueError("yuv: plane %s is a CPU tensor: planes are numpy arrays or CUDA tensors" % name)
        dev, dtype_ok, strides = True, p.dtype == torch_type, tuple(st * sample for st in p.stride())
    else:
        raise ValueError("yuv: plane %s is a %s: planes are numpy arrays or CUDA tensors" % (name, type(p).__name__))
    if not dtype_ok or p.ndim != 2:
        raise ValueError("yuv: plane %s must be a 2-D uint%d array" % (name, 8 * sample))
    rows, row = int(p.shape[0]), int(p.shape[1]) * sample
    if rows < 1 or row < 1:
        raise ValueError("yuv: plane %s is empty (%d x %d)" % (name, rows, p.shape[1]))
    if p.shape[1] > 1 and strides[1] != sample:
        raise ValueError("yuv: plane %s has element stride %d: the bytes of a row must be contiguous" % (name, strides[1]))
    pitch = int(strides[0]) if rows > 1 else row
    if pitch < row:
        raise ValueError("yuv: plane %s has row pitch %d, shorter than its row of %d bytes" % (name, pitch, row))
    if sample == 2 and (pitch % 2 or _address(p) % 2):
        raise ValueError("yuv: plane %s has an odd address or row pitch (%d): uint16 planes are 2-byte aligned" % (name, pitch))
    return dev, rows, row, pitch


class ConvertedFrame:
    """A frame that is converted on its way into a frame store (``YuvFrame``, ``CapturedFrame``) instead of being copied as it is:
    ``shape`` is the (h, w, 3) of the stored frame, ``on_device`` / ``device`` say where its bytes are, ``nbytes`` is what staging
    a host frame copies, ``planes()`` lists those bytes as ``[(array, rows, row bytes, pitch)]`` in staging order, and ``converter``
    is the class whose ``convert`` takes it.  What admits frames tests for this class, not for its kinds."""
    __slots__ = ()
    converter = None

    @property
    def upload_bytes(self) -> int:
        """what admitting the frame sends to the device: its bytes, or nothing when they are already there"""
        return 0 if self.on_device else self.nbytes


class YuvFrame(ConvertedFrame):
    """One YUV frame: ``YuvFrame(fmt, y, u=None, v=None, uv=None, *, matrix="bt601", full_range=False)``.

    ``fmt`` and the planes it takes (h rows, w pixels; ``w`` is even, ``h`` is even where chroma is halved vertically):

    ==========================  ================================================================================  ========
    ``nv12`` ``nv21``           ``y`` (h, w) and ``uv`` (h / 2, w): U, V, U, V ... - V first for nv21             2 x 2
    ``i420`` ``yv12``           ``y``, ``u`` and ``v`` (h / 2, w / 2); the two differ only in ``from_packed``     2 x 2
    ``yuy2`` ``uyvy`` ``yvyu``  one packed plane (h, 2 w), handed in as ``y``: Y0 U Y1 V / U Y0 V Y1 / Y0 V Y1 U  2 x 1
    ``i422``                    ``y`` (h, w), ``u`` and ``v`` (h, w / 2)                                          2 x 1
    ``nv16``                    ``y`` (h, w) and ``uv`` (h, w), U first                                           2 x 1
    ``i444``                    ``y``, ``u`` and ``v`` (h, w)                                                     1 x 1
    ``p010``                    ``y`` (h, w) and ``uv`` (h / 2, w) of uint16, the value in bits 15..6             2 x 2
    ``i010``                    ``y`` (h, w), ``u`` and ``v`` (h / 2, w / 2) of uint16, the value in the low bits 2 x 2
    ==========================  ================================================================================  ========

    ``matrix``: ``"bt601"`` or ``"bt709"``; ``full_range``: Y spans 0..255 (JFIF) instead of 16..235.  At the defaults the four
    4:2:0 formats and the packed 4:2:2 ones are OpenCV's ``cvtColor``; every other table is this project's (include/af_hip.h says
    how it is derived).  A (U, V) serves the pixels of its block; nothing is interpolated.  The stored frame is 8-bit.

    Planes are 2-D uint8 (uint16 for the 10-bit formats, at even addresses and pitches) with unit element stride and a row stride of
    at least the row.  Either all planes are numpy arrays, or all are CUDA ``torch`` tensors on the device of the store they go to.
    ``shape`` is ``(h, w, 3)``, the shape of the converted frame.

    Host planes are copied (into a pinned slot) before the call that takes the frame returns.  Device planes are read where they
    are, on the stream that is current when the frame is handed in: the caller guarantees they are ready on that stream and stay
    unchanged until the work the call enqueued has run."""

    __slots__ = ("fmt", "y", "u", "v", "uv", "shape", "on_device", "interleaved", "swap_uv", "matrix", "full_range", "layout", "order", "_planes")

    def __init__(self, fmt: str, y, u=None, v=None, uv=None, *, matrix: str = "bt601", full_range: bool = False):
        if fmt not in YUV_FORMATS:
            raise ValueError("yuv: format %r is not one of %s" % (fmt, ", ".join(sorted(YUV_FORMATS))))
        if matrix not in MATRICES:
            raise ValueError("yuv: format %r: matrix %r is not one of %s" % (fmt, matrix, ", ".join(sorted(MATRICES))))
        self.fmt, self.y, self.u, self.v, self.uv = fmt, y, u, v, uv
        self.matrix, self.full_range = matrix, bool(full_range)
        self.layout, self.order = YUV_FORMATS[fmt]
        kind, vdiv, hdiv, sample = YUV_LAYOUTS[self.layout]
        self.interleaved, self.swap_uv = kind == "semi", kind == "semi" and self.order == 1
        if kind == "packed":
            if u is not None or v is not None or uv is not None:
                raise ValueError("yuv: format %r takes one packed plane of (h, 2 w) bytes, handed in as y" % fmt)
            named = [("y", y)]
        elif kind == "semi":
            if uv is None or u is not None or v is not None:
                raise ValueError("yuv: %s takes y and uv (one interleaved chroma plane)" % fmt)
            named = [("y", y), ("uv", uv)]
        else:
            if u is None or v is None or uv is not None:
                raise ValueError("yuv: %s takes y, u and v" % fmt)
            named = [("y", y), ("u", u), ("v", v)]
            self.order = 0                                        # the planes are named: their order in memory does not matter
        checked = [_plane(n, p) if sample == 1 else _plane(n, p, sample) for n, p in named]
        if len({c[0] for c in checked}) != 1:
            raise ValueError("yuv: planes are all numpy arrays or all CUDA tensors, not mixed")
        self.on_device = checked[0][0]
        if self.on_device and len({p.device for _, p in named}) != 1:
            raise ValueError("yuv: the planes are on different devices")
        h, w = checked[0][1], checked[0][2] // sample
        if kind == "packed":
            if w % 4:
                raise ValueError("yuv: a packed %s plane has 4 bytes per pixel pair, not rows of %d bytes" % (fmt, w))
            w //= 2
        if w % 2 or (vdiv == 2 and h % 2):
            if vdiv == 2:
                raise ValueError("yuv: a 4:2:0 frame (%s) has even height and width, not %d x %d" % (fmt, h, w))
            raise ValueError("yuv: a %s frame has even width, not %d x %d" % (fmt, h, w))
        want = (h // vdiv, w if kind == "semi" else w // hdiv)
        for (n, _), c in zip(named[1:], checked[1:]):
            if (c[1], c[2] // sample) != want:
                raise ValueError("yuv: plane %s is %d x %d, %d x %d for a %s frame of %d x %d" % (n, c[1], c[2] // sample, want[0], want[1], fmt, h, w))
        if kind == "planar" and checked[1][3] != checked[2][3]:
            raise ValueError("yuv: planes u and v have row pitches %d and %d: one chroma pitch per frame" % (checked[1][3], checked[2][3]))
        self.shape = (h, w, 3)
        self._planes = [(p, c[1], c[2], c[3]) for (_, p), c in zip(named, checked)]

    @classmethod
    def from_packed(cls, buf, h: int, w: int, fmt: str, *, matrix: str = "bt601", full_range: bool = False) -> "YuvFrame":
        """the one 2-D array OpenCV and most decoders use for a planar or semi-planar frame (numpy or a CUDA tensor): h rows of Y, then
        the chroma as `fmt` lays it out - ``(h * 3 / 2, w)`` for the 4:2:0 formats (uint16 for p010 / i010), ``(2 h, w)`` for i422 and
        nv16, ``(3 h, w)`` for i444.  Views of `buf`, no copies.  The planar formats need `buf` contiguous (a chroma row is not a row of
        `buf`); the semi-planar ones take any row pitch.  The packed formats are one plane already: hand it to ``YuvFrame``."""
        if fmt not in YUV_FORMATS:
            raise ValueError("yuv: format %r is not one of %s" % (fmt, ", ".join(sorted(YUV_FORMATS))))
        kind, vdiv, hdiv, _ = YUV_LAYOUTS[YUV_FORMATS[fmt][0]]
        if kind == "packed":
            raise ValueError("yuv: format %r is one packed plane: YuvFrame(%r, plane)" % (fmt, fmt))
        h, w = int(h), int(w)
        if h < 1 or w < 2 or w % 2 or (vdiv == 2 and h % 2):
            if vdiv == 2:
                raise ValueError("yuv: a 4:2:0 frame (%s) has even height and width, not %d x %d" % (fmt, h, w))
            raise ValueError("yuv: a %s frame has even width, not %d x %d" % (fmt, h, w))
        crows, ccols = h // vdiv, w // hdiv                       # of one of the two chroma planes
        rows = h + 2 * crows * ccols // w
        if buf.ndim != 2 or tuple(buf.shape) != (rows, w):
            raise ValueError("yuv: a packed %s frame of %d x %d is a (%d, %d) array, not %s" % (fmt, h, w, rows, w, tuple(buf.shape)))
        colour = dict(matrix=matrix, full_range=full_range)
        if kind == "semi":
            return cls(fmt, buf[:h], uv=buf[h:], **colour)
        contiguous = buf.flags.c_contiguous if isinstance(buf, np.ndarray) else buf.is_contiguous()
        if not contiguous:
            raise ValueError("yuv: a packed %s frame must be contiguous" % fmt)
        flat = buf.reshape(-1)
        q = crows * ccols
        first, second = (flat[h * w + k * q:h * w + (k + 1) * q].reshape(crows, ccols) for k in (0, 1))
        v_first = YUV_FORMATS[fmt][1] == 1
        return cls(fmt, buf[:h], u=second if v_first else first, v=first if v_first else second, **colour)

    @property
    def legacy(self) -> bool:
        """an 8-bit 4:2:0 frame at OpenCV's colour: what ``af_yuv420_to_rgb_u8`` converts"""
        return self.fmt in FORMATS and self.matrix == "bt601" and not self.full_range

    @property
    def nbytes(self) -> int:
        """the bytes of the frame's planes: 1.5 per pixel at 8-bit 4:2:0, 2 at 4:2:2, 3 at 4:4:4 and at 10-bit 4:2:0"""
        return sum(rows * row for _, rows, row, _ in self._planes)

    @property
    def device(self) -> Optional[torch.device]:
        return self.y.device if self.on_device else None

    def planes(self):
        """``[(plane, rows, row bytes, pitch in bytes)]`` in staging order: Y (or the packed plane), then the chroma plane(s) (U
        before V)"""
        return self._planes


# format -> (bytes per pixel, the first byte of a pixel is B)
CAPTURE_FORMATS = {"bgra": (4, True), "rgba": (4, False), "bgr": (3, True), "rgb": (3, False)}


def capture_size(h: int, w: int, max_w: int) -> Tuple[int, int]:
    """``(dw, dh)`` a captured h x w frame is stored at (test/capture_tile.py:199-201): down to `max_w` columns when it has more,
    the height by the same ratio in Python floats, truncated; unchanged otherwise"""
    if max_w > 0 and w > max_w:
        return int(max_w), int(h * (max_w / w))
    return int(w), int(h)


class CapturedFrame(ConvertedFrame):
    """One captured bitmap: ``CapturedFrame(pixels, fmt="bgra", rect=None, max_w=0, size=None)``.

    ``pixels``: (H, W, 4) uint8 for ``"bgra"`` / ``"rgba"`` or (H, W, 3) for ``"bgr"`` / ``"rgb"`` - a numpy array, or a CUDA tensor
    on the device of the store it goes to - with unit element stride, a pixel stride of its channels and any row pitch of at least
    the row; top-down.  The fourth byte never reaches a result.  ``rect = (x0, y0, x1, y1)``: the client area, inside the frame
    (default: all of it).  The stored size: ``capture_size(rh, rw, max_w)`` of the rectangle - the reference's rule - or
    ``size = (dw, dh)``, which must not exceed the rectangle (upscaling is not built); a smaller size is reached with
    ``cv2.INTER_AREA``'s arithmetic on the device.  ``shape`` is the STORED ``(dh, dw, 3)``: rings, stores and trackers downstream
    see the downscaled frame, as the reference's loop does.

    Of a host frame only the rectangle is copied (rh tight rows of rw * channels bytes into a pinned slot) before the call that
    takes the frame returns.  A device frame is read where it lies, under ``YuvFrame``'s stream contract: ready on the stream that
    is current when the frame is handed in, unchanged until the work that call enqueued has run."""

    __slots__ = ("fmt", "pixels", "rect", "shape", "on_device", "channels", "src_bgr", "pitch", "rect_shape", "_view")

    def __init__(self, pixels, fmt: str = "bgra", rect=None, max_w: int = 0, size=None):
        if fmt not in CAPTURE_FORMATS:
            raise ValueError("capture: format %r is not one of %s" % (fmt, ", ".join(sorted(CAPTURE_FORMATS))))
        ch, self.src_bgr = CAPTURE_FORMATS[fmt]
        if isinstance(pixels, np.ndarray):
            dev, dtype_ok, strides = False, pixels.dtype == np.uint8, pixels.strides
        elif isinstance(pixels, torch.Tensor):
            if not pixels.is_cuda:
                raise ValueError("capture: the pixels are a CPU tensor: a numpy array or a CUDA tensor")
            dev, dtype_ok, strides = True, pixels.dtype == torch.uint8, tuple(pixels.stride())
        else:
            raise ValueError("capture: the pixels are a %s: a numpy array or a CUDA tensor" % type(pixels).__name__)
        if not dtype_ok or pixels.ndim != 3:
            raise ValueError("capture: the pixels must be a 3-D uint8 array")
        H, W = int(pixels.shape[0]), int(pixels.shape[1])
        if int(pixels.shape[2]) != ch:
            raise ValueError("capture: %s pixels have %d channels, the array has %d" % (fmt, ch, int(pixels.shape[2])))
        if H < 1 or W < 1:
            raise ValueError("capture: the frame is empty (%d x %d)" % (H, W))
        if strides[2] != 1:
            raise ValueError("capture: element stride %d: the bytes of a pixel must be contiguous" % strides[2])
        if W > 1 and strides[1] != ch:
            raise ValueError("capture: pixel stride %d, not the %d bytes of a %s pixel" % (strides[1], ch, fmt))
        pitch = int(strides[0]) if H > 1 else W * ch
        if pitch < W * ch:
            raise ValueError("capture: row pitch %d, shorter than a row of %d bytes" % (pitch, W * ch))
        x0, y0, x1, y1 = (0, 0, W, H) if rect is None else (int(v) for v in rect)
        if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
            raise ValueError("capture: rect (%d, %d, %d, %d) leaves the frame of %d x %d" % (x0, y0, x1, y1, W, H))
        rh, rw = y1 - y0, x1 - x0
        if size is not None:
            dw, dh = int(size[0]), int(size[1])
            if dw > rw or dh > rh:
                raise ValueError("capture: size %d x %d exceeds the rectangle of %d x %d: upscaling is not built" % (dw, dh, rw, rh))
        else:
            dw, dh = capture_size(rh, rw, int(max_w))
        if dw < 1 or dh < 1:
            raise ValueError("capture: a stored size of %d x %d" % (dw, dh))
        self.fmt, self.pixels, self.rect, self.channels, self.pitch, self.on_device = fmt, pixels, (x0, y0, x1, y1), ch, pitch, dev
        self.rect_shape, self.shape = (rh, rw), (dh, dw, 3)
        self._view = pixels[y0:y1, x0:x1]

    @property
    def nbytes(self) -> int:
        """the bytes of the rectangle: what staging a host frame copies"""
        return self.rect_shape[0] * self.rect_shape[1] * self.channels

    @property
    def device(self) -> Optional[torch.device]:
        return self.pixels.device if self.on_device else None

    def planes(self):
        """``[(the rectangle, rows, row bytes, pitch)]``: one plane"""
        rh, rw = self.rect_shape
        return [(self._view, rh, rw * self.channels, self.pitch)]


def upload_bytes(frame) -> int:
    """the bytes a frame sends to the device when it is admitted: a numpy frame's own, a ``ConvertedFrame``'s if they are on the host"""
    return frame.upload_bytes if isinstance(frame, ConvertedFrame) else frame.nbytes


def store_ref(store, channel_order: str):
    """the ``af_store_ref`` of a ``FrameStore`` whose pixels are in `channel_order`"""
    from . import _lib
    h, w = store.shape[:2]
    return _lib.StoreRef(store.dev.data_ptr(), _lib.FrameStore(store.dev.numel(), store.frame_nbytes, w * 3, store.capacity, h, w, 0),
                         int(channel_order == "bgr"), 0)


class StoreTable:
    """the stores of one launch: ``index(store, channel_order)`` -> the pair's index in this launch; ``refs``: the ``af_store_ref``s
    in order of first use.  Asked once per item, inside the loop that fills the items."""

    def __init__(self):
        self._at, self.refs = {}, []

    def index(self, store, order: str) -> int:
        at = self._at.get((id(store), order))
        if at is None:
            at = self._at[(id(store), order)] = len(self.refs)
            self.refs.append(store_ref(store, order))
        return at

    def array(self):
        from . import _lib
        return (_lib.StoreRef * len(self.refs))(*self.refs)


def launch_stores(refs):
    """the ``af_store_ref`` of every item of one launch -> (the array of the distinct ones in order of first use, its length, every
    item's index into it).  Distinct by identity: ``_Converter.convert`` hands each (store, order) pair's one ``StoreTable`` ref."""
    from . import _lib
    distinct, at = [], {}
    for ref in refs:
        if id(ref) not in at:
            at[id(ref)] = len(distinct)
            distinct.append(ref)
    return (_lib.StoreRef * max(1, len(distinct)))(*distinct), len(distinct), [at[id(ref)] for ref in refs]


def _address(p) -> int:
    return p.__array_interface__["data"][0] if isinstance(p, np.ndarray) else p.data_ptr()


def staged_offsets(frames: Sequence[YuvFrame]) -> Tuple[List[int], int]:
    """where each host frame's planes start in a staging slot (device-resident frames: -1), and the bytes used"""
    offs, used = [], 0
    for f in frames:
        if f.on_device:
            offs.append(-1)
        else:
            used = -(-used // _FRAME_ALIGN) * _FRAME_ALIGN
            offs.append(used)
            used += f.nbytes
    return offs, used


def stage_planes(base: int, frames: Sequence[YuvFrame], offs: Sequence[int], nbytes: int) -> None:
    """the planes of the host frames -> memory at address `base`, frame i from ``offs[i]`` on as tight Y rows, then tight chroma rows
    (U before V): ``af_stage_rows_u8``, one memcpy per plane whose pitch equals its row, else one per row.  From 1 MiB on every plane
    goes as an upper and a lower band of rows, the upper bands on one copy thread and the lower ones on the other."""
    from . import _lib
    bands = _COPY_THREADS if nbytes >= _SPLIT_BYTES else 1
    rects = []
    for t in range(bands):
        for f, off in zip(frames, offs):
            if off < 0:
                continue
            for p, rows, row, pitch in f.planes():
                r0, r1 = rows * t // bands, rows * (t + 1) // bands
                if r1 > r0:
                    rects.append(_lib.StageRect(_address(p) + r0 * pitch, off + r0 * row, pitch, r1 - r0, row))
                off += rows * row
    if rects:
        stage_rects(base, (_lib.StageRect * len(rects))(*rects), len(rects), nbytes)


class _Converter:
    """``convert([(frame, FrameStore, channel_order, slot), ...])`` for one kind of ``ConvertedFrame``: every frame into its slot of
    its store, converted on the device.  The host bytes of all frames go tightly into ONE pinned slot - behind them, for a kind
    whose launch reads its table from device memory, the tables of the launches - and cross in ONE asynchronous copy; one launch per
    ``max_frames`` frames follows on the current stream and reads host frames from the slot's device twin, device-resident ones
    where they are.  The slot's event is recorded behind the last launch, the last reader of both buffers; nothing waits.
    ``launches`` and ``copies`` count what was enqueued.  A kind says: ``frame_type``, ``what`` (its word in messages),
    ``max_frames``, ``stat_keys`` (a server's counters of its launches and copies), ``_room`` and ``_plan``."""
    frame_type, what, holds, max_frames, stat_keys = None, "", "bytes", 0, (None, None)

    def __init__(self, device, stage: Optional[PinnedRing] = None):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        self.device = device
        self._stage = stage if stage is not None else PinnedRing(min_bytes=1 << 20, headroom=True)
        self.launches = self.copies = 0

    def _room(self, frames) -> int:
        """the bytes the table of one launch over `frames` may need in the staging slot (0: the table travels by value)"""
        return 0

    def _plan(self, frames, addresses, refs, slots, table_host: int, table_dev: int, room: int):
        """plans one launch -> (the bytes of the table written at `table_host`, ``launch(stream)``)"""
        raise NotImplementedError

    def convert(self, jobs) -> None:
        jobs = list(jobs)
        if not jobs:
            return
        frames = [j[0] for j in jobs]
        for f, store, order, slot in jobs:
            if not isinstance(f, self.frame_type):
                raise ValueError("%s: a list of frames is all numpy arrays or all YuvFrame or all CapturedFrame" % self.what)
            if tuple(f.shape) != tuple(store.shape):
                raise ValueError("%s: a frame of %s for a store of %s" % (self.what, f.shape, tuple(store.shape)))
            if f.on_device and f.device != store.device:
                raise ValueError("%s: the %s are on %s, the frame store on %s" % (self.what, self.holds, f.device, store.device))
        table = StoreTable()
        refs = [table.refs[table.index(j[1], j[2])] for j in jobs]
        with torch.cuda.device(self.device):
            offs, used = staged_offsets(frames)
            parts, total = [], used
            for lo in range(0, len(jobs), self.max_frames):
                hi = min(lo + self.max_frames, len(jobs))
                room = self._room(frames[lo:hi])
                if room:
                    total = -(-total // _FRAME_ALIGN) * _FRAME_ALIGN
                parts.append((lo, hi, total, room))
                total += room
            slot, host_base, dev_base = None, 0, 0
            if total:
                slot = self._stage.acquire(total, self.device)
                host_base, dev_base = slot.host.data_ptr(), slot.dev.data_ptr()
            if used:
                stage_planes(host_base, frames, offs, used)
            end, launches = used, []
            for lo, hi, at, room in parts:
                wrote, launch = self._plan(frames[lo:hi], [None if o < 0 else dev_base + o for o in offs[lo:hi]], refs[lo:hi],
                                           [j[3] for j in jobs[lo:hi]], host_base + at, dev_base + at, room)
                if wrote:
                    end = at + wrote
                launches.append(launch)
            if end:
                slot.dev[:end].copy_(slot.host[:end], non_blocking=True)
                self.copies += 1
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for launch in launches:
                launch(stream)
                self.launches += 1
            if slot is not None:
                slot.record()          # behind the last launch: it reads the device twin, which the next copy into this slot rewrites


class YuvConverter(_Converter):
    """``_Converter`` for ``YuvFrame``s: one launch per ``AF_YUV_MAX_FRAMES`` frames; its table travels to the kernel by value, so
    ``copies`` counts the copies of staged host planes alone.  A ``convert`` whose frames are all 8-bit 4:2:0 at OpenCV's colour
    (``YuvFrame.legacy``) launches ``af_yuv420_to_rgb_u8`` (csrc/af_yuv.hip); any other launches ``af_yuv_to_rgb_ex_u8``
    (csrc/af_yuv_formats.hip) for all its frames, whatever the mix of layouts, depths and colours."""
    frame_type, what, holds, max_frames, stat_keys = YuvFrame, "yuv", "planes", 64, ("convert", "yuv_copies")

    @staticmethod
    def table(frames: Sequence[YuvFrame], addresses: Sequence[int], stores, slots: Sequence[int]):
        """the planner's part, host only: ``frames[i]`` whose planes start at device address ``addresses[i]`` (tight Y, then tight
        chroma; None: the frame's own device planes) into slot ``slots[i]`` of ``stores[i]`` (an ``_lib.StoreRef`` each) -> the
        ``YuvItem`` array of one launch"""
        from . import _lib
        descs = (_lib.YuvFrameDesc * max(1, len(frames)))()
        store_arr, n_stores, index = launch_stores(stores)
        for i, (f, base, slot) in enumerate(zip(frames, addresses, slots)):
            h, w = f.shape[:2]
            if not f.legacy:
                raise ValueError("yuv: a %s frame (%s, %s range) is not one af_yuv420_to_rgb_u8 converts"
                                 % (f.fmt, f.matrix, "full" if f.full_range else "limited"))
            if base is None:
                ptrs = [_address(p) for p, _, _, _ in f.planes()]
                y_pitch, c_pitch = f.planes()[0][3], f.planes()[1][3]
            else:
                ptrs, y_pitch, c_pitch = [base, base + h * w], w, (w if f.interleaved else w // 2)
                if not f.interleaved:
                    ptrs.append(base + h * w + h * w // 4)
            descs[i] = _lib.YuvFrameDesc(ptrs[0], ptrs[1], None if f.interleaved else ptrs[2], y_pitch, c_pitch, h, w,
                                         int(f.interleaved), int(f.swap_uv), index[i], int(slot))
        items = (_lib.YuvItem * max(1, len(frames)))()
        _lib.check(_lib.lib.af_yuv420_plan_u8(C.byref(descs), len(frames), C.byref(store_arr), n_stores, C.byref(items)), "yuv420_plan_u8")
        return items

    @staticmethod
    def table_ex(frames: Sequence[YuvFrame], addresses: Sequence[int], stores, slots: Sequence[int]):
        """``table`` for frames of any format and colour -> the ``YuvItemEx`` array of one launch of ``af_yuv_to_rgb_ex_u8``; staged
        planes lie tight one behind the other in ``planes()`` order"""
        from . import _lib
        descs = (_lib.YuvFrameEx * max(1, len(frames)))()
        store_arr, n_stores, index = launch_stores(stores)
        for i, (f, base, slot) in enumerate(zip(frames, addresses, slots)):
            h, w = f.shape[:2]
            if base is None:
                ptrs, pitches = [_address(p) for p, _, _, _ in f.planes()], [pitch for _, _, _, pitch in f.planes()]
            else:
                ptrs, pitches = [], []
                for _, rows, row, _ in f.planes():
                    ptrs.append(base)
                    pitches.append(row)
                    base += rows * row
            ptrs, pitches = ptrs + [None, None], pitches + [0]
            descs[i] = _lib.YuvFrameEx(ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], h, w, f.layout, f.order, MATRICES[f.matrix],
                                       int(f.full_range), index[i], int(slot))
        items = (_lib.YuvItemEx * max(1, len(frames)))()
        _lib.check(_lib.lib.af_yuv_plan_ex_u8(C.byref(descs), len(frames), C.byref(store_arr), n_stores, C.byref(items)), "yuv_plan_ex_u8")
        return items

    def convert(self, jobs) -> None:
        jobs = list(jobs)
        self._legacy = all(getattr(j[0], "legacy", True) for j in jobs)       # decided for the whole batch: one kernel per convert
        super().convert(jobs)

    def _plan(self, frames, addresses, refs, slots, table_host, table_dev, room):
        from . import _lib
        n = len(frames)
        if self._legacy:
            items = self.table(frames, addresses, refs, slots)
            return 0, lambda stream: _lib.check(_lib.lib.af_yuv420_to_rgb_u8(C.byref(items), n, stream), "yuv420_to_rgb_u8")
        items = self.table_ex(frames, addresses, refs, slots)
        return 0, lambda stream: _lib.check(_lib.lib.af_yuv_to_rgb_ex_u8(C.byref(items), n, stream), "yuv_to_rgb_ex_u8")


class CaptureConverter(_Converter):
    """``_Converter`` for ``CapturedFrame``s: ``CaptureConverter(device, stage=None).convert([(frame, store, channel_order, slot),
    ...])`` - one pinned fill, one copy and one launch of ``af_capture_to_stores_u8`` per ``AF_CAPTURE_MAX_FRAMES`` frames, which may
    differ in size, format, rectangle, mode, store and byte order.  The launch reads its table (it holds the area tables) from
    device memory: the tables lie behind the pixels in the same pinned slot and cross in the same copy, so ``copies`` is one per
    ``convert`` - also for device-resident frames, whose table still has to cross."""
    frame_type, what, holds, max_frames, stat_keys = CapturedFrame, "capture", "pixels", 64, ("capture", None)

    @staticmethod
    def descs(frames: Sequence[CapturedFrame], addresses: Sequence[Optional[int]], stores, slots: Sequence[int]):
        """``frames[i]`` whose rectangle lies tight at device address ``addresses[i]`` (None: where the frame's own device pixels
        are, at their pitch) into slot ``slots[i]`` of ``stores[i]`` (an ``_lib.StoreRef`` each) -> (the ``af_capture_frame`` array,
        the ``af_store_ref`` array, its length)"""
        from . import _lib
        descs = (_lib.CaptureFrame * max(1, len(frames)))()
        store_arr, n_stores, index = launch_stores(stores)
        for i, (f, base, slot) in enumerate(zip(frames, addresses, slots)):
            (rh, rw), (dh, dw, _) = f.rect_shape, f.shape
            src, pitch = (_address(f._view), f.pitch) if base is None else (base, rw * f.channels)
            descs[i] = _lib.CaptureFrame(src, pitch, rh, rw, f.channels, int(f.src_bgr), index[i], int(slot), dh, dw)
        return descs, store_arr, n_stores

    @staticmethod
    def table_bytes(frames: Sequence[CapturedFrame]) -> int:
        """an upper bound of the bytes of the table of one launch over `frames`"""
        from . import _lib
        descs = (_lib.CaptureFrame * max(1, len(frames)))(*[_lib.CaptureFrame(None, 0, f.rect_shape[0], f.rect_shape[1], f.channels, 0, 0, 0,
                                                                                 f.shape[0], f.shape[1]) for f in frames])
        n = _lib.lib.af_capture_table_bytes(C.byref(descs), len(frames))
        if n < 0:
            raise ValueError("capture: %d frames of %s: at most %d per launch, every side 1 to %d, no upscaling"
                             % (len(frames), sorted({f.rect_shape + f.shape[:2] for f in frames}), _lib.CAPTURE_MAX_FRAMES, _lib.CAPTURE_MAX_SIDE))
        return n

    @staticmethod
    def table(frames, addresses, stores, slots, table_address: int, table_bytes: int) -> int:
        """the planner's part, host only: the table of one launch at host address `table_address`; returns the bytes used"""
        from . import _lib
        descs, store_arr, n_stores = CaptureConverter.descs(frames, addresses, stores, slots)
        used = C.c_int64(0)
        _lib.check(_lib.lib.af_capture_plan_u8(C.byref(descs), len(frames), C.byref(store_arr), n_stores, C.c_void_p(table_address), table_bytes,
                                               C.byref(used)), "capture_plan_u8")
        return used.value

    def _room(self, frames) -> int:
        return self.table_bytes(frames)

    def _plan(self, frames, addresses, refs, slots, table_host, table_dev, room):
        from . import _lib
        used, n = self.table(frames, addresses, refs, slots, table_host, room), len(frames)
        return used, lambda stream: _lib.check(_lib.lib.af_capture_to_stores_u8(C.c_void_p(table_dev), n, stream), "capture_to_stores_u8")


CapturedFrame.converter, YuvFrame.converter = CaptureConverter, YuvConverter


def _tensor_ref(t: torch.Tensor):
    """the ``af_store_ref`` of a (B, H, W, 3) or (H, W, 3) uint8 device tensor with packed pixels: B frames (or one) of a store"""
    from . import _lib
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError("resize: frames must be (H, W, 3) or (B, H, W, 3) uint8, got %s %s" % (tuple(t.shape), t.dtype))
    if t.stride(-1) != 1 or t.stride(-2) != 3:
        raise ValueError("resize: frames must have packed pixels (strides (..., 3, 1))")
    b = t.shape[0] if t.dim() == 4 else 1
    h, w = int(t.shape[-3]), int(t.shape[-2])
    if b < 1 or h < 1 or w < 1:
        raise ValueError("resize: empty frames %s" % (tuple(t.shape),))
    pitch = max(int(t.stride(-3)), 3 * w) if h > 1 else 3 * w
    span = (h - 1) * pitch + 3 * w
    stride = max(int(t.stride(0)), span) if t.dim() == 4 and b > 1 else span
    if (h > 1 and t.stride(-3) < 3 * w) or (t.dim() == 4 and b > 1 and t.stride(0) < span):
        raise ValueError("resize: rows or frames overlap (strides %s)" % (tuple(t.stride()),))
    return _lib.StoreRef(t.data_ptr(), _lib.FrameStore((b - 1) * stride + span, stride, pitch, b, h, w, 0), 0, 0), b


class FrameResizer:
    """``cv2.resize(frame, (dw, dh))`` of frames that are on `device`, into a detector batch: ``resize(frames, (dw, dh))`` ->
    a (B, dh, dw, 3) uint8 device tensor, enqueued on the current stream without a host synchronisation.

    ``frames``: a (B, H, W, 3) uint8 device tensor, or a list whose entries are (H, W, 3) device views (pixels packed, rows may be
    pitched) or ``(FrameStore, slot)`` pairs; the entries may differ in size and come from different stores
    (``resize_views`` is the list form under the name the servers use).  All entries of one call go out in ONE launch per
    ``AF_RESIZE_MAX_FRAMES`` frames.  Channels are treated alike: the byte order of the source is the byte order of the result.

    The resizer owns a ring of pinned tables (the planner's output crosses in one asynchronous copy per launch) and one output
    buffer per (B, size), RE-USED: the tensor a call returns is overwritten by the next call with the same B and size, so consume
    it (on the same stream) before then, or clone it.  ``launches`` counts the launches enqueued."""

    def __init__(self, device=None):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        self.device = cuda_device(device)
        self._tables = PinnedRing(slots=4, min_bytes=1 << 16, headroom=True)
        self._out = {}
        self._launch = _lib.lib.af_resize_frames_u8
        self.launches = 0

    @staticmethod
    def plan(jobs, refs, table_address: int, table_bytes: int) -> int:
        """the planner's part, host only: ``jobs`` = [(index into refs, frame, destination address, destination pitch, dw, dh)] and
        ``refs`` = [``_lib.StoreRef``] -> the launch's table at host address `table_address`; returns the bytes used"""
        from . import _lib
        arr = (_lib.ResizeJob * max(1, len(jobs)))(*[_lib.ResizeJob(int(r), int(f), int(d), int(p), int(dh), int(dw)) for r, f, d, p, dw, dh in jobs])
        store_arr = (_lib.StoreRef * max(1, len(refs)))(*refs)
        used = C.c_int64(0)
        _lib.check(_lib.lib.af_resize_plan_u8(C.byref(arr), len(jobs), C.byref(store_arr), len(refs), C.c_void_p(table_address), table_bytes,
                                              C.byref(used)), "resize_plan_u8")
        return used.value

    @staticmethod
    def table_bytes(sizes) -> int:
        """an upper bound of the table's bytes for destinations of ``sizes`` = [(dw, dh)]"""
        from . import _lib
        arr = (_lib.ResizeJob * max(1, len(sizes)))(*[_lib.ResizeJob(0, 0, None, 0, int(dh), int(dw)) for dw, dh in sizes])
        n = _lib.lib.af_resize_table_bytes(C.byref(arr), len(sizes))
        if n < 0:
            raise ValueError("resize: %d destinations of %s: at most %d per launch, each 1 to %d in both directions"
                             % (len(sizes), sorted(set(sizes)), _lib.RESIZE_MAX_FRAMES, _lib.RESIZE_MAX_SIDE))
        return n

    def _sources(self, frames):
        """-> ([StoreRef], [(index into them, frame)])"""
        table, extra, src = StoreTable(), [], []
        if isinstance(frames, torch.Tensor):
            frames = [frames]
        for f in frames:
            if isinstance(f, torch.Tensor):
                if f.device != self.device:
                    raise ValueError("resize: a frame on %s, the resizer on %s" % (f.device, self.device))
                ref, b = _tensor_ref(f)
                extra.append(ref)
                src += [(-len(extra), k) for k in range(b)]      # negative: an index into `extra`, resolved below
            else:
                store, slot = f
                if store.device != self.device:
                    raise ValueError("resize: a frame store on %s, the resizer on %s" % (store.device, self.device))
                if not 0 <= int(slot) < store.capacity:
                    raise ValueError("resize: slot %d of a frame store of %d" % (slot, store.capacity))
                src.append((table.index(store, "rgb"), int(slot)))
        refs = table.refs + extra
        return refs, [(r if r >= 0 else len(table.refs) - r - 1, k) for r, k in src]

    def resize(self, frames, size: Tuple[int, int]) -> torch.Tensor:
        from . import _lib
        dw, dh = int(size[0]), int(size[1])
        if not (1 <= dw <= _lib.RESIZE_MAX_SIDE and 1 <= dh <= _lib.RESIZE_MAX_SIDE):
            raise ValueError("resize: a destination of %dx%d (1 to %d in both directions)" % (dw, dh, _lib.RESIZE_MAX_SIDE))
        refs, src = self._sources(frames)
        if not src:
            raise ValueError("resize: no frames")
        b = len(src)
        with torch.cuda.device(self.device):
            out = self._out.get((b, dw, dh))
            if out is None:
                with torch.inference_mode(False):
                    out = self._out[(b, dw, dh)] = torch.empty((b, dh, dw, 3), dtype=torch.uint8, device=self.device)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for lo in range(0, b, _lib.RESIZE_MAX_FRAMES):
                part = src[lo:lo + _lib.RESIZE_MAX_FRAMES]
                used_refs = sorted({r for r, _ in part})
                at = {r: i for i, r in enumerate(used_refs)}
                jobs = [(at[r], k, out.data_ptr() + (lo + i) * dh * dw * 3, dw * 3, dw, dh) for i, (r, k) in enumerate(part)]
                need = self.table_bytes([(dw, dh)] * len(part))
                slot = self._tables.acquire(need, self.device)
                used = self.plan(jobs, [refs[r] for r in used_refs], slot.host.data_ptr(), slot.host.numel())
                slot.dev[:used].copy_(slot.host[:used], non_blocking=True)
                _lib.check(self._launch(C.c_void_p(slot.dev.data_ptr()), len(part), stream), "resize_frames_u8")
                slot.record()                                     # behind the launch, the last reader of both buffers
                self.launches += 1
        return out

    def resize_views(self, views, size: Tuple[int, int]) -> torch.Tensor:
        """``resize`` on a list of (H, W, 3) device views out of several stores, of any sizes: what a server's detecting tick has"""
        return self.resize(list(views), size)
