"""YuNet face detector on the MI355X: the live-call loop's detection stage (preprocessing/yunet/yunet.py: YuNet, i.e.
cv2.FaceDetectorYN on face_detection_yunet_2023mar.onnx) as HIP kernels (csrc/af_yunet.hip).

- `build_plan(graph)` matches a parsed ONNX graph (onnx_min) against exactly the YuNet-2023mar topology and returns the
  fixed plan the kernels implement; any other graph raises ValueError naming the first node that does not match.
- `pack_weights(plan)` lays the plan's weights out as the flat fp32 blob af_yunet_detect reads.
- `YuNet` is a drop-in for the reference wrapper (same constructor, name, setBackendAndTarget, setInputSize, infer);
  `YuNet.detect` is the batched device API.
There is no CPU fallback: infer / detect need a HIP device."""
import ctypes as C
import hashlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import onnx_min
from ._device import DeviceModel

OUTPUT_NAMES = ["%s_%d" % (k, s) for k in ("cls", "obj", "bbox", "kps") for s in (8, 16, 32)]
HEAD_KINDS = (("cls", 1), ("obj", 1), ("bbox", 4), ("kps", 10))      # channel order of the packed head: 16 channels
STRIDES = (8, 16, 32)
# (cin, cout) of the DP units in graph order; units 0, 4, 6, 8 are followed by MaxPool 2x2/2, units 12, 13 are the neck
UNIT_CHANNELS = [(16, 16), (16, 16), (16, 32), (32, 32), (32, 64)] + [(64, 64)] * 9
POOLED_UNITS = (0, 4, 6, 8)


@dataclass
class Unit:
    cin: int
    cout: int
    pw: np.ndarray           # [cout, cin, 1, 1]
    pb: np.ndarray
    dw: np.ndarray           # [cout, 1, 3, 3]
    db: np.ndarray
    out: str                 # name of the tensor after the ReLU
    pool: Optional[str] = None
    neck: Optional[Tuple[str, str]] = None     # (a, b): input = a + up2(b)


@dataclass
class Plan:
    stem_w: np.ndarray
    stem_b: np.ndarray
    units: List[Unit]
    heads: List[Dict[str, Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]]   # per level: kind -> (pw, pb, dw, db)
    resize_scales: Tuple[float, ...]
    opset: int
    num_params: int = 0
    head_inputs: List[str] = field(default_factory=list)


def padded_size(w: int, h: int) -> Tuple[int, int]:
    """FaceDetectorYN pads the frame bottom / right with zeros to a multiple of 32"""
    return ((w - 1) // 32 + 1) * 32, ((h - 1) // 32 + 1) * 32


def num_anchors(w: int, h: int) -> int:
    pw, ph = padded_size(w, h)
    return sum((pw // s) * (ph // s) for s in STRIDES)


class _Cursor:
    def __init__(self, g: onnx_min.Graph):
        self.g, self.i = g, 0

    def fail(self, why: str, node=None):
        n = node if node is not None else (self.g.nodes[self.i] if self.i < len(self.g.nodes) else None)
        where = "end of graph" if n is None else "node %d %s %s -> %s" % (self.g.nodes.index(n), n.op_type, n.inputs, n.outputs)
        raise ValueError("not the YuNet-2023mar graph: %s (%s)" % (why, where))

    def take(self, op: str, inp: Optional[str] = None, **attrs):
        if self.i >= len(self.g.nodes):
            self.fail("expected %s" % op)
        n = self.g.nodes[self.i]
        if n.op_type != op:
            self.fail("expected %s" % op)
        if inp is not None and (not n.inputs or n.inputs[0] != inp):
            self.fail("expected input %s" % inp)
        for k, v in attrs.items():
            if n.attrs.get(k) != v:
                self.fail("attribute %s = %r, expected %r" % (k, n.attrs.get(k), v))
        self.i += 1
        return n

    def init(self, n, k: int, shape) -> np.ndarray:
        name = n.inputs[k] if len(n.inputs) > k else None
        t = self.g.initializers.get(name)
        if t is None:
            self.fail("input %d is not an initializer" % k, n)
        if tuple(t.dims) != tuple(shape):
            self.fail("initializer %s has shape %s, expected %s" % (name, t.dims, tuple(shape)), n)
        return t.array

    def conv(self, inp, cin, cout, k, stride=1, group=1):
        p = (k - 1) // 2
        n = self.take("Conv", inp, kernel_shape=(k, k), strides=(stride, stride), pads=(p, p, p, p), group=group,
                      dilations=(1, 1))
        if len(n.inputs) != 3:
            self.fail("conv without bias", n)
        w = self.init(n, 1, (cout, cin // group, k, k)).astype(np.float32)
        b = self.init(n, 2, (cout,)).astype(np.float32)
        return n.outputs[0], w, b

    def unit(self, inp, cin, cout) -> Unit:
        t, pw, pb = self.conv(inp, cin, cout, 1)
        t, dw, db = self.conv(t, cout, cout, 3, group=cout)
        r = self.take("Relu", t)
        return Unit(cin, cout, pw, pb, dw, db, r.outputs[0])


def build_plan(g: onnx_min.Graph) -> Plan:
    """Match `g` against the YuNet-2023mar graph (node by node, every shape and attribute) and return its fixed plan."""
    cur = _Cursor(g)
    if len(g.inputs) != 1 or len(g.inputs[0].shape) != 4 or g.inputs[0].shape[1] != 3:
        raise ValueError("not the YuNet-2023mar graph: input %s" % (g.inputs,))
    if [o.name for o in g.outputs] != OUTPUT_NAMES:
        raise ValueError("not the YuNet-2023mar graph: outputs %s, expected %s" % ([o.name for o in g.outputs], OUTPUT_NAMES))
    t, sw, sb = cur.conv(g.inputs[0].name, 3, 16, 3, stride=2)
    t = cur.take("Relu", t).outputs[0]
    units: List[Unit] = []
    full = {}
    scales = None
    for u, (cin, cout) in enumerate(UNIT_CHANNELS):
        neck = None
        if u in (12, 13):                                    # 242 = 223 + up2(236); 252 = 214 + up2(246)
            lat = full[8 if u == 12 else 6]
            rz = cur.take("Resize", t, mode=b"nearest", coordinate_transformation_mode=b"asymmetric", nearest_mode=b"floor")
            if len(rz.inputs) != 3:
                cur.fail("Resize without scales", rz)
            sc = tuple(float(v) for v in cur.init(rz, 2, (4,)))
            if sc != (1.0, 1.0, 2.0, 2.0):
                cur.fail("Resize scales %s, expected (1, 1, 2, 2)" % (sc,), rz)
            scales = sc
            add = cur.take("Add")
            if add.inputs != [lat, rz.outputs[0]]:
                cur.fail("expected Add(%s, %s)" % (lat, rz.outputs[0]), add)
            neck = (lat, t)
            t = add.outputs[0]
        unit = cur.unit(t, cin, cout)
        unit.neck = neck
        t = full[u] = unit.out
        if u in POOLED_UNITS:
            mp = cur.take("MaxPool", t, kernel_shape=(2, 2), strides=(2, 2), pads=(0, 0, 0, 0))
            if mp.attrs.get("ceil_mode", 0) != 0:
                cur.fail("MaxPool ceil_mode", mp)
            unit.pool = t = mp.outputs[0]
        units.append(unit)
    head_inputs = [full[13], full[12], full[11]]              # strides 8, 16, 32
    heads: List[Dict[str, tuple]] = [{} for _ in STRIDES]
    head_out: Dict[Tuple[str, int], str] = {}
    for kind, ch in (("cls", 1), ("bbox", 4), ("obj", 1), ("kps", 10)):        # graph order of the head convs
        for lvl, src in enumerate(head_inputs):
            t1, pw, pb = cur.conv(src, 64, ch, 1)
            t2, dw, db = cur.conv(t1, ch, ch, 3, group=ch)
            heads[lvl][kind] = (pw, pb, dw, db)
            head_out[(kind, lvl)] = t2
    for kind, ch in (("cls", 1), ("obj", 1), ("bbox", 4), ("kps", 10)):        # graph order of the output tails
        for lvl in range(3):
            tr = cur.take("Transpose", head_out[(kind, lvl)], perm=(0, 2, 3, 1))
            rs = cur.take("Reshape", tr.outputs[0])
            shape = cur.init(rs, 1, (3,))
            if [int(v) for v in shape] != [1, -1, ch]:      # batch 1 is baked into the file; the plan batches natively
                cur.fail("Reshape to %s, expected (1, -1, %d)" % (list(shape), ch), rs)
            last = rs
            if kind in ("cls", "obj"):
                last = cur.take("Sigmoid", rs.outputs[0])
            if last.outputs[0] != "%s_%d" % (kind, STRIDES[lvl]):
                cur.fail("output %s, expected %s_%d" % (last.outputs[0], kind, STRIDES[lvl]), last)
    if cur.i != len(g.nodes):
        cur.fail("unexpected trailing node")
    nparams = sum(t.array.size for t in g.initializers.values())
    return Plan(sw, sb, units, heads, scales, g.opset, nparams, head_inputs)


def pack_weights(plan: Plan) -> np.ndarray:
    """the flat fp32 weight blob of af_yunet_detect (csrc/af_yunet.hip): stem [ky][kx][ci][16] + bias; per unit 1x1 [ci][co] +
    bias, depthwise [tap][c] + bias; per level the 16-channel head (cls, obj, bbox, kps) in the same two-conv layout"""
    parts = [plan.stem_w.transpose(2, 3, 1, 0).ravel(), plan.stem_b]
    for u in plan.units:
        parts += [u.pw[:, :, 0, 0].T.ravel(), u.pb, u.dw[:, 0].reshape(u.cout, 9).T.ravel(), u.db]
    for lvl in plan.heads:
        pw = np.concatenate([lvl[k][0][:, :, 0, 0] for k, _ in HEAD_KINDS], 0)          # [16, 64]
        pb = np.concatenate([lvl[k][1] for k, _ in HEAD_KINDS])
        dw = np.concatenate([lvl[k][2][:, 0].reshape(-1, 9) for k, _ in HEAD_KINDS], 0)  # [16, 9]
        db = np.concatenate([lvl[k][3] for k, _ in HEAD_KINDS])
        parts += [pw.T.ravel(), pb, dw.T.ravel(), db]
    return np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).ravel() for p in parts]))


def split_raw(raw: np.ndarray, w: int, h: int) -> Dict[str, np.ndarray]:
    """the per-anchor head outputs af_yunet_detect writes ([B][anchors][16]) as the 12 graph outputs, (B, n, C) each"""
    pw, ph = padded_size(w, h)
    out, off = {}, 0
    lv = []
    for s in STRIDES:
        n = (pw // s) * (ph // s)
        lv.append((s, off, n))
        off += n
    c0 = 0
    for kind, ch in HEAD_KINDS:
        for s, o, n in lv:
            out["%s_%d" % (kind, s)] = raw[:, o:o + n, c0:c0 + ch]
        c0 += ch
    return {k: out[k] for k in OUTPUT_NAMES}


class YuNet(DeviceModel):
    """Drop-in for preprocessing/yunet/yunet.py YuNet (cv2.FaceDetectorYN), running on the current HIP device."""

    _weight_floats_fn = "af_yunet_weight_floats"
    _workspace_bytes_fn = "af_yunet_workspace_bytes"
    _detect_fn = ("af_yunet_detect", "YUNET_LAUNCHES")

    def __init__(self, modelPath, inputSize=[320, 320], confThreshold=0.6, nmsThreshold=0.3, topK=5000, backendId=0, targetId=0):
        self._modelPath = modelPath
        self._inputSize = tuple(int(v) for v in inputSize)      # [w, h]
        self._confThreshold = float(confThreshold)
        self._nmsThreshold = float(nmsThreshold)
        self._topK = int(topK)
        self._backendId = backendId
        self._targetId = targetId
        if not 1 <= self._topK <= 8192:
            raise ValueError("topK %d out of [1, 8192]" % self._topK)
        with open(modelPath, "rb") as f:
            data = f.read()
        self.sha256 = hashlib.sha256(data).hexdigest()
        self.plan = build_plan(onnx_min.parse_model(data))
        super().__init__(pack_weights(self.plan))

    @property
    def name(self):
        return self.__class__.__name__

    def setBackendAndTarget(self, backendId, targetId):
        """accepted and recorded: there is one backend (the HIP kernels) and one target (the current device)"""
        self._backendId = backendId
        self._targetId = targetId

    def setInputSize(self, input_size):
        self._inputSize = tuple(int(v) for v in input_size)

    # ---- device side
    def _desc(self, b, h, w, frame_stride, row_pitch, conf, nms, top_k):
        from . import _lib
        return _lib.YunetDesc(b, h, w, top_k, frame_stride, row_pitch, conf, nms)

    def detect(self, frames_u8, raw: bool = False, conf: Optional[float] = None, nms: Optional[float] = None,
               top_k: Optional[int] = None, timings=None):
        """Batched device API: `frames_u8` a (B, H, W, 3) uint8 BGR tensor on a HIP device (rows may be padded; pixels packed).
        Returns (rows (B, top_k, 15) f32, counts (B,) int32) device tensors on the current stream, without a host
        synchronisation; rows past counts[b] are unspecified.  One instance may serve several streams at once: each
        (device, stream) has its own scratch workspace, and the kernels of one call touch no other call's memory.  raw=True also returns the (B, anchors, 16) head outputs
        (see split_raw).  `timings`: a list that receives the per-kernel device times in ms (this call synchronises)."""
        import torch
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.device.type != "cuda":
            raise RuntimeError("YuNet.detect needs a (B, H, W, 3) uint8 tensor on a HIP device (there is no CPU path)")
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
            raise ValueError("frames must be (B, H, W, 3) uint8, got %s %s" % (tuple(frames_u8.shape), frames_u8.dtype))
        if frames_u8.stride(3) != 1 or frames_u8.stride(2) != 3:
            raise ValueError("frames must have packed BGR pixels (strides (..., 3, 1))")
        b, h, w, _ = frames_u8.shape
        top_k = self._topK if top_k is None else int(top_k)
        desc = self._desc(b, h, w, frames_u8.stride(0), frames_u8.stride(1), self._confThreshold if conf is None else float(conf),
                          self._nmsThreshold if nms is None else float(nms), top_k)
        dev = frames_u8.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            ws = self._workspace(dev, cur, desc)
            wt = self._weights(dev)
            rows = torch.empty(b, top_k, 15, dtype=torch.float32, device=dev)
            counts = torch.empty(b, dtype=torch.int32, device=dev)
            rawt = torch.empty(b, num_anchors(w, h), 16, dtype=torch.float32, device=dev) if raw else None
            stream = C.c_void_p(cur.cuda_stream)
            args = [C.byref(desc), C.c_void_p(wt.data_ptr()), C.c_void_p(frames_u8.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                    C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(rawt.data_ptr() if raw else None), stream]
            self._call(self._detect_fn, args, timings)
        return (rows, counts, rawt) if raw else (rows, counts)

    def detect_views(self, views, raw: bool = False, conf: Optional[float] = None, nms: Optional[float] = None,
                     top_k: Optional[int] = None):
        """``detect`` on frames that lie anywhere on one device: `views` a list of at most 64 (H, W, 3) uint8 device views of equal
        shape and strides (slots of different frame rings, say).  One call of ``af_yunet_detect_frames``: the frame pointers
        travel in the first kernel's launch arguments, no frame is copied.  Returns what ``detect`` returns on their stack."""
        import torch
        from . import _lib
        views = list(views)
        if not 1 <= len(views) <= _lib.YUNET_MAX_LIST:
            raise ValueError("detect_views: %d frames (1 to %d per call)" % (len(views), _lib.YUNET_MAX_LIST))
        v0 = views[0]
        for v in views:
            if not isinstance(v, torch.Tensor) or v.device.type != "cuda":
                raise RuntimeError("YuNet.detect_views needs (H, W, 3) uint8 tensors on a HIP device (there is no CPU path)")
            if v.dtype != torch.uint8 or v.dim() != 3 or v.shape[2] != 3:
                raise ValueError("frames must be (H, W, 3) uint8, got %s %s" % (tuple(v.shape), v.dtype))
            if v.stride(2) != 1 or v.stride(1) != 3:
                raise ValueError("frames must have packed BGR pixels (strides (..., 3, 1))")
            if v.shape != v0.shape or v.stride() != v0.stride() or v.device != v0.device:
                raise ValueError("detect_views: the frames of one call have one shape, one row pitch and one device")
        b, (h, w, _) = len(views), v0.shape
        top_k = self._topK if top_k is None else int(top_k)
        desc = self._desc(b, h, w, v0.stride(0) * h, v0.stride(0), self._confThreshold if conf is None else float(conf),
                          self._nmsThreshold if nms is None else float(nms), top_k)
        dev = v0.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            ws = self._workspace(dev, cur, desc)
            wt = self._weights(dev)
            rows = torch.empty(b, top_k, 15, dtype=torch.float32, device=dev)
            counts = torch.empty(b, dtype=torch.int32, device=dev)
            rawt = torch.empty(b, num_anchors(w, h), 16, dtype=torch.float32, device=dev) if raw else None
            ptrs = (C.c_void_p * b)(*[v.data_ptr() for v in views])
            self._call(("af_yunet_detect_frames", None),
                       [C.byref(desc), C.c_void_p(wt.data_ptr()), ptrs, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(rows.data_ptr()),
                        C.c_void_p(counts.data_ptr()), C.c_void_p(rawt.data_ptr() if raw else None), C.c_void_p(cur.cuda_stream)], None)
        return (rows, counts, rawt) if raw else (rows, counts)

    # ---- detection on downscaled frames
    @staticmethod
    def scale_rows(rows, sx: float, sy: float) -> np.ndarray:
        """(n, 15) rows found on a resized frame -> the full frame's, as demo2.py:196-208 scales them: float64; x, w and the
        landmark x's times `sx`, y, h and the landmark y's times `sy`, the score untouched"""
        return np.asarray(rows, dtype=np.float64).reshape(-1, 15) * np.array([sx, sy] * 7 + [1.0], dtype=np.float64)

    def _resizer(self, device):
        from .frames import FrameResizer
        resizers = self.__dict__.setdefault("_resizers", {})
        if device not in resizers:
            resizers[device] = FrameResizer(device)
        return resizers[device]

    def detect_resized(self, frames, size, conf: Optional[float] = None, nms: Optional[float] = None, top_k: Optional[int] = None):
        """``detect`` on frames resized on the device to ``size`` = (dw, dh) with cv2.resize's arithmetic (``frames.FrameResizer``),
        the rows scaled back to each frame's own size: what demo2.py does with ``--yunet_res``.  `frames`: a (B, H, W, 3) uint8
        device tensor, or a list of (H, W, 3) device views / ``(FrameStore, slot)`` pairs that may differ in size - they share one
        resize launch and one detector call per 64.  Returns a list of (n, 15) **float64** numpy arrays, one per frame
        (``scale_rows`` with sx = W / dw, sy = H / dh, on the host); this call waits for the device once."""
        import torch
        if isinstance(frames, torch.Tensor):
            if frames.dim() != 4:
                raise ValueError("frames must be (B, H, W, 3) uint8, got %s" % (tuple(frames.shape),))
            dev, shapes = frames.device, [tuple(frames.shape[1:3])] * frames.shape[0]
        else:
            frames = list(frames)
            if not frames:
                return []
            first = frames[0] if isinstance(frames[0], torch.Tensor) else frames[0][0]
            dev = first.device
            shapes = [tuple(f.shape[:2]) if isinstance(f, torch.Tensor) else tuple(f[0].shape[:2]) for f in frames]
        dw, dh = int(size[0]), int(size[1])
        out = []
        with torch.cuda.device(dev):
            small = self._resizer(dev).resize(frames, (dw, dh))
            for lo in range(0, small.shape[0], 64):
                rows, counts = self.detect(small[lo:lo + 64], conf=conf, nms=nms, top_k=top_k)
                rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
                out += [rows[b, :int(counts[b])] for b in range(rows.shape[0])]
        return [self.scale_rows(r, w / dw, h / dh) for r, (h, w) in zip(out, shapes)]

    def infer_resized(self, image, size):
        """``infer`` as demo2.py:194-196 calls it: one H x W x 3 uint8 BGR frame of any size, resized on the device to ``size`` =
        (dw, dh) and detected there (the preset input size is not consulted).  Returns the (N, 15) rows scaled back to the frame,
        **float64**, or np.empty((0, 5)) when there is no face."""
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("infer_resized needs an H x W x 3 uint8 BGR image, got %s %s" % (image.shape, image.dtype))
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        rows = self.detect_resized(torch.from_numpy(np.ascontiguousarray(image)).to(dev).unsqueeze(0), size)[0]
        return rows if len(rows) else np.empty(shape=(0, 5))

    def infer(self, image):
        """FaceDetectorYN.detect on one H x W x 3 uint8 BGR frame of the preset input size: (N, 15) float32, or
        np.empty((0, 5)) when there is no face (as the reference wrapper returns)."""
        image = np.asarray(image)
        w, h = self._inputSize
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("infer needs an H x W x 3 uint8 BGR image, got %s %s" % (image.shape, image.dtype))
        if image.shape[:2] != (h, w):
            raise ValueError("image size %dx%d does not match the input size %dx%d (setInputSize)" % (
                image.shape[1], image.shape[0], w, h))
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        frame = torch.from_numpy(np.ascontiguousarray(image)).to(dev).unsqueeze(0)
        rows, counts = self.detect(frame)
        n = int(counts[0].item())
        if n == 0:
            return np.empty(shape=(0, 5))
        return rows[0, :n].cpu().numpy()
