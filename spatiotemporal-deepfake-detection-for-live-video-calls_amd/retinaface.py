"""RetinaFace face detector on the MI355X: the offline evaluator's detect_all front (test_tools/ct/detection: RetinaFace,
mobilenet0.25, and alignment.batch_detect's post_process) as HIP kernels (csrc/af_retinaface.hip).

- `state_dict_layout()` is the reference RetinaFace(cfg_mnet).state_dict() layout: 300 (key, shape) pairs in order.
- `load(model_path)` reads a checkpoint like load_model / load_net (unwrap "state_dict", strip "module."), but every key
  must be present with its shape: the reference's strict=False would keep random initial values, which cannot be restated.
- `pack_weights(sd)` folds BN (eps 1e-5) and lays the weights out as the flat fp32 blob af_retinaface_detect reads.
- `FaceDetector` is a drop-in for the reference FaceDetector (same constructor, detect, __call__); `detect_device` is the
  batched device API and `postprocess_device` runs the decode + post-process alone on given head outputs.
`scale_detect` is not provided: it resizes with cv2.resize, which is not restated here.
There is no CPU fallback: detection needs a HIP device."""
import ctypes as C
import math
import os
from collections import OrderedDict
from typing import List, Optional, Tuple

import numpy as np

from ._device import DeviceModel

STEPS = (8, 16, 32)
MIN_SIZES = ((16, 32), (64, 128), (256, 512))
VARIANCE = (0.1, 0.2)
MEAN = (104, 117, 123)
CONF_THRESHOLD, TOP_K, NMS_THRESHOLD, KEEP_TOP_K = 0.02, 5000, 0.4, 750
BN_EPS = 1e-5
# MobileNetV1 (mobilenet0.25): conv_bn(3, 8, 2), then conv_dw (cin, cout, stride); stage1 = first 6, stage2 = next 6
DW_BLOCKS = [(8, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1),
             (64, 128, 2), (128, 128, 1), (128, 128, 1), (128, 128, 1), (128, 128, 1), (128, 128, 1),
             (128, 256, 2), (256, 256, 1)]
SSH_CONVS = [("conv3X3", 64, 32), ("conv5X5_1", 64, 16), ("conv5X5_2", 16, 16), ("conv7X7_2", 16, 16), ("conv7x7_3", 16, 16)]
HEADS = [("BboxHead", 4), ("ClassHead", 2), ("LandmarkHead", 10)]     # channels per anchor; 2 anchors per pixel


def _stage_key(i: int) -> str:
    """state-dict prefix of MobileNetV1 layer i (0 = conv_bn, 1..13 = conv_dw)"""
    if i < 6:
        return "body.stage1.%d" % i
    if i < 12:
        return "body.stage2.%d" % (i - 6)
    return "body.stage3.%d" % (i - 12)


def _bn(prefix: str, c: int):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)),
            (prefix + ".running_var", (c,)), (prefix + ".num_batches_tracked", ())]


def state_dict_layout() -> List[Tuple[str, tuple]]:
    """(key, shape) of RetinaFace(cfg_mnet, phase="test").state_dict(), in order (IntermediateLayerGetter keeps stage1..3)"""
    L = [(_stage_key(0) + ".0.weight", (8, 3, 3, 3))] + _bn(_stage_key(0) + ".1", 8)
    for i, (cin, cout, _) in enumerate(DW_BLOCKS, 1):
        p = _stage_key(i)
        L += [(p + ".0.weight", (cin, 1, 3, 3))] + _bn(p + ".1", cin)
        L += [(p + ".3.weight", (cout, cin, 1, 1))] + _bn(p + ".4", cout)
    for name, cin in (("output1", 64), ("output2", 128), ("output3", 256)):
        L += [("fpn.%s.0.weight" % name, (64, cin, 1, 1))] + _bn("fpn.%s.1" % name, 64)
    for name in ("merge1", "merge2"):
        L += [("fpn.%s.0.weight" % name, (64, 64, 3, 3))] + _bn("fpn.%s.1" % name, 64)
    for s in (1, 2, 3):
        for name, cin, cout in SSH_CONVS:
            L += [("ssh%d.%s.0.weight" % (s, name), (cout, cin, 3, 3))] + _bn("ssh%d.%s.1" % (s, name), cout)
    for head, k in (("ClassHead", 2), ("BboxHead", 4), ("LandmarkHead", 10)):
        for l in range(3):
            L += [("%s.%d.conv1x1.weight" % (head, l), (2 * k, 64, 1, 1)), ("%s.%d.conv1x1.bias" % (head, l), (2 * k,))]
    return L


def check_state_dict(sd) -> None:
    """every layout key present with its shape (extra keys are ignored, as load_state_dict(strict=False) does)"""
    for key, shape in state_dict_layout():
        if key not in sd:
            raise KeyError("RetinaFace checkpoint lacks %s" % key)
        got = tuple(sd[key].shape)
        if got != tuple(shape):
            raise ValueError("RetinaFace checkpoint %s has shape %s, expected %s" % (key, got, tuple(shape)))


def _strip(sd, prefix="module."):
    return OrderedDict((k[len(prefix):] if k.startswith(prefix) else k, v) for k, v in sd.items())


def load(model_path) -> "OrderedDict":
    """load_model's reading of a checkpoint: torch.load on the CPU, unwrap "state_dict", strip "module."; then checked"""
    import torch
    if model_path is None:
        raise ValueError("RetinaFace needs a model_path: the reference downloads mobilenet0.25_Final.pth when it is None, "
                         "this mirror never fetches anything")
    sd = torch.load(model_path, map_location="cpu")
    if "state_dict" in sd.keys():
        sd = sd["state_dict"]
    sd = _strip(sd)
    check_state_dict(sd)
    return sd


# ---- weight packing (csrc/af_retinaface.hip: make_layout)
def _np(t) -> np.ndarray:
    return t.detach().cpu().double().numpy() if hasattr(t, "detach") else np.asarray(t, np.float64)


def _fold(sd, conv_key: str, bn_prefix: str):
    w = _np(sd[conv_key])
    g, b, m, v = (_np(sd[bn_prefix + s]) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    scale = g / np.sqrt(v + BN_EPS)
    return w * scale.reshape(-1, 1, 1, 1), b - m * scale


def _pack_mfma(w: np.ndarray, bias: np.ndarray) -> List[np.ndarray]:
    """[cout][cin][ks][ks] -> B fragments [tap][cin / 16][cout / 16][lane = 16 kq + col][j], k = 16 c + 4 kq + j"""
    cout, cin, ks, _ = w.shape
    cinp = (cin + 15) // 16 * 16
    t = np.zeros((ks * ks, cinp, cout))
    t[:, :cin, :] = w.transpose(2, 3, 1, 0).reshape(ks * ks, cin, cout)
    t = t.reshape(ks * ks, cinp // 16, 4, 4, cout // 16, 16).transpose(0, 1, 4, 2, 5, 3)
    return [t.ravel(), bias]


def pack_weights(sd) -> np.ndarray:
    parts = []
    w, b = _fold(sd, _stage_key(0) + ".0.weight", _stage_key(0) + ".1")
    parts += [w.transpose(2, 3, 1, 0).ravel(), b]
    for i, (cin, cout, _) in enumerate(DW_BLOCKS, 1):
        p = _stage_key(i)
        w, b = _fold(sd, p + ".0.weight", p + ".1")
        parts += [w[:, 0].reshape(cin, 9).T.ravel(), b]
        parts += _pack_mfma(*_fold(sd, p + ".3.weight", p + ".4"))
    for name in ("output1", "output2", "output3", "merge1", "merge2"):
        parts += _pack_mfma(*_fold(sd, "fpn.%s.0.weight" % name, "fpn.%s.1" % name))
    for s in (1, 2, 3):
        for name, _, _ in SSH_CONVS:
            parts += _pack_mfma(*_fold(sd, "ssh%d.%s.0.weight" % (s, name), "ssh%d.%s.1" % (s, name)))
    for l in range(3):
        w = np.concatenate([_np(sd["%s.%d.conv1x1.weight" % (h, l)]) for h, _ in HEADS], 0)    # [32, 64, 1, 1]
        b = np.concatenate([_np(sd["%s.%d.conv1x1.bias" % (h, l)]) for h, _ in HEADS])
        parts += _pack_mfma(w, b)
    return np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).astype(np.float32))


# ---- geometry
def feature_maps(h: int, w: int):
    return [(math.ceil(h / s), math.ceil(w / s)) for s in STEPS]


def num_anchors(h: int, w: int) -> int:
    return sum(2 * fh * fw for fh, fw in feature_maps(h, w))


def priors(h: int, w: int) -> np.ndarray:
    """PriorBox(cfg_mnet, (h, w)).forward(): (cx, cy, s_kx, s_ky) per anchor, computed in double, rounded to fp32"""
    out = []
    for k, (fh, fw) in enumerate(feature_maps(h, w)):
        step = STEPS[k]
        ii, jj = np.meshgrid(np.arange(fh, dtype=np.float64), np.arange(fw, dtype=np.float64), indexing="ij")
        cx = ((jj + 0.5) * step / w).ravel()
        cy = ((ii + 0.5) * step / h).ravel()
        for_anchor = []
        for ms in MIN_SIZES[k]:
            for_anchor.append(np.stack([cx, cy, np.full_like(cx, ms / w), np.full_like(cy, ms / h)], 1))
        out.append(np.stack(for_anchor, 1).reshape(-1, 4))
    return np.concatenate(out, 0).astype(np.float32)


def _split_rows(rows: np.ndarray, n: int):
    """(n, 15) detection rows -> post_process's [(box (4,), landmarks (5, 2), score)] list"""
    return [(rows[i, :4].copy(), rows[i, 5:15].reshape(5, 2).copy(), rows[i, 4]) for i in range(n)]


# ---- FaceDetector.scale_detect's host steps (test_tools/ct/detection/__init__.py:10-51), restated

SCALE_DETECT_MAX_RES = 1920


def scale_detect_scale(h: int, w: int):
    """``resize_scale`` for frames of h x w: the int 2 up to 1920 on the long side, ``2 * max(h, w) / 1920`` (a float) above"""
    return 2 * (max(h, w) / SCALE_DETECT_MAX_RES if max(h, w) > SCALE_DETECT_MAX_RES else 1)


def scale_detect_size(h: int, w: int) -> Tuple[int, int]:
    """``(resize_w, resize_h)``: the size scale_detect detects frames of h x w at; (0, 0) for a 1 x 1 frame"""
    s = scale_detect_scale(h, w)
    return int(w / s), int(h / s)


def check_valid(face, w, h) -> bool:
    """a face (box, landmarks, score) whose box is ordered and lies, with every landmark, in [0, w) x [0, h)"""
    box, pts = face[0], face[1]
    if box[0] > box[2] or box[1] > box[3]:
        return False
    if not (0 <= box[0] < w and 0 <= box[1] < h and 0 <= box[2] < w and 0 <= box[3] < h):
        return False
    return all(0 <= p[0] < w and 0 <= p[1] < h for p in pts)


def post_detect(detect_results, scale, w, h):
    """boxes and landmarks of every frame's faces times `scale` (float32 products, as numpy gives ``float32 array * python
    number``), faces that fail ``check_valid`` on the w x h frame dropped; scores untouched"""
    out = []
    for faces in detect_results:
        scaled = [(box * scale, ldm * scale, score) for box, ldm, score in faces]
        out.append([f for f in scaled if check_valid(f, w=w, h=h)])
    return out


class FaceDetector(DeviceModel):
    """Drop-in for test_tools/ct/detection.FaceDetector (RetinaFace, mobilenet0.25) on HIP device `gpu_id`."""

    _weight_floats_fn = "af_retinaface_weight_floats"
    _workspace_bytes_fn = "af_retinaface_workspace_bytes"
    _detect_fn = ("af_retinaface_detect", "RETINAFACE_LAUNCHES")
    _postprocess_fn = ("af_retinaface_postprocess", "RETINAFACE_POST_LAUNCHES")

    def __init__(self, gpu_id=0, model_path=None, network="mobilenet"):
        if network != "mobilenet":
            raise ValueError("network %r: only mobilenet (mobilenet0.25) is restated" % (network,))
        if gpu_id is None or int(gpu_id) < 0:
            raise ValueError("gpu_id %r: there is no CPU path, pass a HIP device index" % (gpu_id,))
        self.gpu_id = int(gpu_id)
        self.network = network
        self.state_dict = load(model_path)
        super().__init__(pack_weights(self.state_dict))

    @classmethod
    def from_state_dict(cls, sd, gpu_id=0):
        """a detector on already-loaded weights (the reference's key names); checked like load()"""
        self = cls.__new__(cls)
        if int(gpu_id) < 0:
            raise ValueError("gpu_id %r: there is no CPU path" % (gpu_id,))
        self.gpu_id, self.network = int(gpu_id), "mobilenet"
        sd = _strip(sd)
        check_state_dict(sd)
        self.state_dict = sd
        DeviceModel.__init__(self, pack_weights(sd))
        return self

    @property
    def device(self):
        import torch
        return torch.device("cuda", self.gpu_id)

    # ---- device side
    @staticmethod
    def _desc(b, h, w, frame_stride, row_pitch, keep_top_k, max_count, min_score):
        from . import _lib
        return _lib.RetinafaceDesc(b, h, w, int(keep_top_k), frame_stride, row_pitch, int(max_count), 0, float(min_score))

    def detect_device(self, frames_u8, keep_top_k: int = KEEP_TOP_K, max_count: int = 0, min_score: float = 0.0,
                      raw: bool = False, timings=None):
        """Batched device API: `frames_u8` a (B, H, W, 3) uint8 tensor on a HIP device, channels as the caller holds them
        (pixels packed; rows and frames may be strided, so a channel-reversed view must be made contiguous first).
        Returns (rows (B, K, 15) f32, counts (B,) int32) on the current stream without a host synchronisation; a row is
        x1 y1 x2 y2 score l0x l0y .. l4y, rows past counts[b] are unspecified.  K = min(keep_top_k, max_count) (max_count
        <= 0: keep_top_k); rows with score < min_score are cut (get_valid_faces(max_count, min_score) on the full result).
        raw=True also returns (loc (B, A, 4), conf (B, A, 2) after the softmax, landms (B, A, 10)).  `timings`: a list
        that receives the per-launch device times in ms (this call synchronises)."""
        import torch
        from . import _lib
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.device.type != "cuda":
            raise RuntimeError("detect_device needs a (B, H, W, 3) uint8 tensor on a HIP device (there is no CPU path)")
        if frames_u8.dtype != torch.uint8:
            raise TypeError("frames must be uint8, got %s" % frames_u8.dtype)
        if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
            raise ValueError("frames must be (B, H, W, 3), got %s" % (tuple(frames_u8.shape),))
        if frames_u8.stride(3) != 1 or frames_u8.stride(2) != 3:
            raise ValueError("frames must have packed pixels (strides (..., 3, 1))")
        b, h, w, _ = frames_u8.shape
        desc = self._desc(b, h, w, frames_u8.stride(0), frames_u8.stride(1), keep_top_k, max_count, min_score)
        dev = frames_u8.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            ws = self._workspace(dev, cur, desc)
            wt = self._weights(dev)
            k = _lib.lib.af_retinaface_max_rows(C.byref(desc))
            rows = torch.empty(b, k, 15, dtype=torch.float32, device=dev)
            counts = torch.empty(b, dtype=torch.int32, device=dev)
            a = num_anchors(h, w)
            rawt = torch.empty(16 * b * a, dtype=torch.float32, device=dev) if raw else None
            args = [C.byref(desc), C.c_void_p(wt.data_ptr()), C.c_void_p(frames_u8.data_ptr()), C.c_void_p(ws.data_ptr()),
                    ws.numel(), C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()),
                    C.c_void_p(rawt.data_ptr() if raw else None), C.c_void_p(cur.cuda_stream)]
            self._call(self._detect_fn, args, timings)
        if not raw:
            return rows, counts
        loc = rawt[:4 * b * a].view(b, a, 4)
        conf = rawt[4 * b * a:6 * b * a].view(b, a, 2)
        landms = rawt[6 * b * a:].view(b, a, 10)
        return rows, counts, (loc, conf, landms)

    def postprocess_device(self, loc, conf, landms, h: int, w: int, keep_top_k: int = KEEP_TOP_K, max_count: int = 0,
                           min_score: float = 0.0, timings=None):
        """decode + post_process alone on (B, A, 4) loc, (B, A, 2) conf (after the softmax), (B, A, 10) landms f32 device
        tensors of an h x w frame: (rows, counts) as detect_device returns them"""
        import torch
        from . import _lib
        b = loc.shape[0]
        a = num_anchors(h, w)
        for t, k in ((loc, 4), (conf, 2), (landms, 10)):
            if t.dtype != torch.float32 or tuple(t.shape) != (b, a, k) or not t.is_contiguous() or t.device.type != "cuda":
                raise ValueError("postprocess needs contiguous (%d, %d, %d) f32 device tensors" % (b, a, k))
        desc = self._desc(b, h, w, 0, 3 * w, keep_top_k, max_count, min_score)
        dev = loc.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            ws = self._workspace(dev, cur, desc)
            k = _lib.lib.af_retinaface_max_rows(C.byref(desc))
            rows = torch.empty(b, k, 15, dtype=torch.float32, device=dev)
            counts = torch.empty(b, dtype=torch.int32, device=dev)
            args = [C.byref(desc), C.c_void_p(loc.data_ptr()), C.c_void_p(conf.data_ptr()), C.c_void_p(landms.data_ptr()),
                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()),
                    C.c_void_p(cur.cuda_stream)]
            self._call(self._postprocess_fn, args, timings)
        return rows, counts

    # ---- the reference's interface
    @staticmethod
    def _as_batch(images):
        """what batch_detect accepts -> ((B, H, W, 3) uint8 torch tensor, single-frame flag)"""
        import torch
        if isinstance(images, np.ndarray):
            if images.ndim not in (3, 4):
                raise ValueError("images must be HWC or NHWC, got shape %s" % (images.shape,))
            single = images.ndim == 3
            arr = images[None] if single else images
            if arr.dtype != np.uint8:
                raise TypeError("images must be uint8, got %s" % arr.dtype)
            t = torch.from_numpy(np.ascontiguousarray(arr))
        elif isinstance(images, (list, tuple)):
            if not images:
                raise ValueError("empty list of images")
            shapes = {np.shape(x) for x in images}
            if len(shapes) != 1:
                raise ValueError("Input images must be of same size, got %s" % sorted(shapes))
            dtypes = {np.asarray(x).dtype if not isinstance(x, torch.Tensor) else x.dtype for x in images}
            if dtypes != {np.dtype(np.uint8)} and dtypes != {torch.uint8}:
                raise TypeError("images must be uint8, got %s" % sorted(map(str, dtypes)))
            single = False
            t = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x) for x in images], 0)))
        elif isinstance(images, torch.Tensor):
            if images.dim() not in (3, 4):
                raise ValueError("images must be HWC or NHWC, got shape %s" % (tuple(images.shape),))
            if images.dtype != torch.uint8:
                raise TypeError("images must be uint8, got %s" % images.dtype)
            single = images.dim() == 3
            t = (images.unsqueeze(0) if single else images).contiguous()
        else:
            raise NotImplementedError(type(images))
        if t.shape[-1] != 3:
            raise ValueError("images must have 3 channels, got shape %s" % (tuple(t.shape),))
        return t, single

    def detect(self, images):
        """batch_detect: per frame a list of (box f32 (4,), landmarks f32 (5, 2), score f32) in descending score order;
        the single list for one HWC frame"""
        t, single = self._as_batch(images)
        dev = self.device
        rows, counts = self.detect_device(t.to(dev, non_blocking=False))
        rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
        out = [_split_rows(rows[b], int(counts[b])) for b in range(rows.shape[0])]
        return out[0] if single else out

    def scale_detect_device(self, frames_u8, keep_top_k: int = KEEP_TOP_K, max_count: int = 0, min_score: float = 0.0, timings=None):
        """``detect_device`` on `frames_u8` (B, H, W, 3) resized on the device to ``scale_detect_size(H, W)`` with cv2.resize's
        arithmetic (``frames.FrameResizer``).  Returns ``(rows, counts, scale)``: rows and counts as ``detect_device`` returns
        them, in the coordinates of the RESIZED frames; multiply boxes and landmarks by `scale` (``scale_detect_scale``) and apply
        ``check_valid`` against (W, H) to get what ``scale_detect`` returns.  No host synchronisation."""
        from .frames import FrameResizer
        if frames_u8.dim() != 4:
            raise ValueError("frames must be (B, H, W, 3), got %s" % (tuple(frames_u8.shape),))
        h, w = int(frames_u8.shape[1]), int(frames_u8.shape[2])
        dw, dh = scale_detect_size(h, w)
        if dw < 1 or dh < 1:
            raise ValueError("scale_detect: frames of %dx%d would be detected at %dx%d (cv2.resize fails there in the reference)" % (w, h, dw, dh))
        resizers = self.__dict__.setdefault("_resizers", {})
        rs = resizers.get(frames_u8.device)
        if rs is None:
            rs = resizers[frames_u8.device] = FrameResizer(frames_u8.device)
        small = rs.resize(frames_u8, (dw, dh))
        rows, counts = self.detect_device(small, keep_top_k, max_count, min_score, timings=timings)
        return rows, counts, scale_detect_scale(h, w)

    def scale_detect(self, images):
        """the reference's ``scale_detect``: frames up to 1920 on the long side are detected at half size, larger ones at 960 on
        the long side, and the boxes and landmarks are scaled back (``post_detect``: faces that leave the frame are dropped).
        The frames are uploaded as ``detect`` uploads them and resized on the device.  Returns what ``detect`` returns."""
        t, single = self._as_batch(images)
        h, w = int(t.shape[1]), int(t.shape[2])
        dw, dh = scale_detect_size(h, w)
        if dw < 1 or dh < 1:
            raise ValueError("scale_detect: frames of %dx%d would be detected at %dx%d (cv2.resize fails there in the reference)" % (w, h, dw, dh))
        rows, counts, scale = self.scale_detect_device(t.to(self.device, non_blocking=False))
        rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
        out = post_detect([_split_rows(rows[b], int(counts[b])) for b in range(rows.shape[0])], scale, w, h)
        return out[0] if single else out

    def __call__(self, images):
        return self.detect(images)
