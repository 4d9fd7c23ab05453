"""Host pixels on their way to the device, the parts every caller shares: what counts as a crop, which device a caller means, a
crop's rectangle for ``af_stage_rows_u8``, the fan-out of that copy over the copy threads, and the ring of pinned buffers the
copies land in.  The aligner stages a clip's crops through it, the evaluator its crops, frames and window tables."""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

_COPY_THREADS = 2          # measured on the MI355X host: 1 thread 45 GB/s, 2 threads 72 GB/s, 4+ slower (memory-bound copies)
_SPLIT_BYTES = 1 << 20     # a smaller copy is over before a second thread has picked its half up
_copy_pool = None


def _pool():
    global _copy_pool
    if _copy_pool is None:
        _copy_pool = ThreadPoolExecutor(max_workers=_COPY_THREADS, thread_name_prefix="af-align-stage")
    return _copy_pool


def is_crop(im) -> bool:
    """an HxWx3 uint8 numpy array"""
    return isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3


def cuda_device(device=None) -> torch.device:
    """`device` (default: the current one) as a CUDA device with its index spelled out"""
    dev = torch.device(device if device is not None else "cuda")
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def packed_rgb(im: np.ndarray) -> bool:
    """the pixels of a crop are packed R, G, B bytes and its rows do not overlap: a row is one memcpy"""
    st = im.strides
    return st[2] == 1 and st[1] == 3 and st[0] >= im.shape[1] * 3


def crop_rect(im: np.ndarray):
    """``((address, pitch, rows, row bytes), array to keep alive)`` of a crop: the crop's own memory when its pixels are packed RGB
    bytes (a row or column slice of a larger picture is), else a contiguous copy.  The array must live until the copy has run."""
    if not packed_rgb(im):
        im = np.ascontiguousarray(im)
    row = im.shape[1] * 3
    return (im.__array_interface__["data"][0], im.strides[0] if im.shape[0] > 1 else row, im.shape[0], row), im


def stage_rects(base: int, rects, n: int, nbytes: int) -> None:
    """the first `n` of the ``StageRect`` array `rects` -> memory at address `base` (af_stage_rows_u8: one memcpy per row; ctypes
    releases the GIL), from `nbytes` = 1 MiB on as two halves on the copy threads.  The rectangles' sources must stay alive.
    (Staging in four chunks, each crossing PCIe while the next is copied, was tried: the extra pool round trips and small copies
    cost more than the overlap gained - host-inclusive 1 780 -> 860 clips/s.)"""
    from . import _lib

    def part(lo, hi):
        _lib.check(_lib.lib.af_stage_rows_u8(C.c_void_p(base), C.byref(rects, lo * C.sizeof(_lib.StageRect)), hi - lo), "stage_rows_u8")
    nt = min(_COPY_THREADS, n) if nbytes >= _SPLIT_BYTES else 1
    if nt > 1:
        cuts = [n * t // nt for t in range(nt + 1)]
        list(_pool().map(part, cuts[:-1], cuts[1:]))
    else:
        part(0, n)


class _Slot:
    __slots__ = ("host", "dev", "done")

    def __init__(self):
        self.host = self.dev = self.done = None

    def record(self) -> None:
        """the slot's last reader has just been enqueued on the current stream: the slot is free again once that has run"""
        self.done = torch.cuda.Event()
        self.done.record()


class PinnedRing:
    """`slots` pinned host buffers, each with an event and - for callers that hand ``acquire`` a device - a device twin, used
    round-robin.  ``acquire`` gives a slot out only after the event recorded behind its last reader (``slot.record()``) has
    completed, so neither an asynchronous copy nor a kernel sees a buffer change under it; `slots` fillings may be in flight.  A
    slot holds at least `min_bytes`; one that is too small is replaced by one of the bytes asked for, plus a quarter with
    `headroom`.  The buffers are made outside inference mode, so they stay writable after a caller's inference_mode block."""

    def __init__(self, slots: int = 3, min_bytes: int = 1 << 20, headroom: bool = False):
        self.slots = [_Slot() for _ in range(slots)]
        self.min_bytes, self.headroom = int(min_bytes), headroom
        self.turn = 0                      # acquisitions so far
        self._lock = threading.Lock()

    @property
    def last(self) -> _Slot:
        """the slot the last ``acquire`` gave out"""
        return self.slots[(self.turn - 1) % len(self.slots)]

    def acquire(self, nbytes: int, device=None) -> _Slot:
        with self._lock:
            slot = self.slots[self.turn % len(self.slots)]
            self.turn += 1
        if slot.done is not None:
            slot.done.synchronize()
        if slot.host is None or slot.host.numel() < nbytes or (device is not None and (slot.dev is None or slot.dev.device != device)):
            cap = max(nbytes + (nbytes // 4 if self.headroom else 0), self.min_bytes)
            with torch.inference_mode(False):
                slot.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
                slot.dev = torch.empty(cap, dtype=torch.uint8, device=device) if device is not None else None
        return slot
