"""``cv2.resize(img, (dw, dh))`` with the default ``INTER_LINEAR`` for HxWxC uint8 images in numpy, the statement
csrc/af_resize.hip is checked against, and the host steps of the reference's ``FaceDetector.scale_detect``
(test_tools/ct/detection/__init__.py:10-56) around it.

The resize follows the plain C++ path of OpenCV 4.x ``resize.cpp`` (``resize`` -> ``ResizeAreaFastVec`` for the exact 2x case,
``HResizeLinear`` / ``VResizeLinear`` with ``FixedPtCast<int, uchar, 22>`` otherwise).  cv2 is not installed where this project is
built, so the restatement is pinned by hand-worked anchors (tests/test_resize_host.py): it is **unpinned against cv2 itself**, and
an OpenCV built with IPP may take another path than the plain one restated here.

  identity    (dw, dh) == (w, h): a copy
  scales      inv_x = dw / w in fp64, scale_x = 1.0 / inv_x (not w / dw: the two can differ in the last bit); the same for y
  exact 2x    abs(scale_x - 2) < DBL_EPSILON and abs(scale_y - 2) < DBL_EPSILON: OpenCV switches INTER_LINEAR to the fast area
              path, (a + b + c + d + 2) >> 2 per channel (quality_ref.half_size's first case).  Both axes must be 2: 24x11 -> 12x5
              is bilinear on both axes, and so is a 4x scale.
  columns     fx = float32((dx + 0.5) * scale_x - 0.5), product and difference in fp64, one rounding to fp32
              sx = floor(fx); fx = float32(fx - sx)
              sx < 0: sx = 0, fx = 0;  sx >= w - 1: sx = w - 1, fx = 0 (the second tap is then never read: its weight is 0)
              a1 = rint(fx * 2048f), a0 = rint((1f - fx) * 2048f): fp32 products, half to even, int16
              H[dx] = S[sx] * a0 + S[sx + 1] * a1 in int32
  rows        the same fy, sy, b0, b1 without the clamp of fy; the source rows sy and sy + 1 are each clipped to [0, h - 1]
  byte        (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2 in int32 with arithmetic shifts; it cannot leave 0..255

Knowing difference from the sources: none in the arithmetic.  Where OpenCV writes ``S[sx] * 2048`` for the columns right of
``xmax`` this multiplies by a0 = 2048 and adds 0 * the clamped neighbour, which is the same integer.
"""
import numpy as np

F32 = np.float32
DBL_EPSILON = float(np.finfo(np.float64).eps)
COEF_BITS = 11
ONE = 1 << COEF_BITS


def scale_of(src: int, dst: int) -> float:
    """cv2.resize's fp64 scale of one axis: 1 / (dst / src)"""
    inv = float(dst) / float(src)
    return 1.0 / inv


def is_area2(w: int, h: int, dw: int, dh: int) -> bool:
    return abs(scale_of(w, dw) - 2.0) < DBL_EPSILON and abs(scale_of(h, dh) - 2.0) < DBL_EPSILON


def coefs(src: int, dst: int, clamp: bool):
    """``(index int32, a0 int16, a1 int16)`` arrays of one axis; ``clamp``: the column rule, else the row rule (index -1 .. src - 1)"""
    scale = scale_of(src, dst)
    idx, a0, a1 = np.zeros(dst, np.int32), np.zeros(dst, np.int16), np.zeros(dst, np.int16)
    for d in range(dst):
        f = F32((d + 0.5) * scale - 0.5)                       # python floats: fp64 product and difference, one rounding
        s = int(np.floor(f))
        f = F32(f - F32(s))
        if clamp:
            if s < 0:
                s, f = 0, F32(0)
            if s >= src - 1:
                s, f = src - 1, F32(0)
        idx[d] = s
        a0[d] = int(np.rint(F32(F32(1) - f) * F32(ONE)))
        a1[d] = int(np.rint(f * F32(ONE)))
    return idx, a0, a1


def resize_linear(img: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """``cv2.resize(img, (dw, dh))`` of an HxWxC uint8 image"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("resize_linear takes an HxWxC uint8 image, got %s %s" % (img.shape, img.dtype))
    h, w = img.shape[:2]
    if dw < 1 or dh < 1:
        raise ValueError("resize_linear: a destination of %dx%d" % (dw, dh))
    if (dw, dh) == (w, h):
        return img.copy()
    if is_area2(w, h, dw, dh):
        c = img.astype(np.int32)
        return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = coefs(w, dw, True)
    sy, b0, b1 = coefs(h, dh, False)
    s = img.astype(np.int32)
    sx1 = np.minimum(sx + 1, w - 1)                            # read only with a weight of 0 when it was clamped
    hor = s[:, sx] * a0.astype(np.int32)[None, :, None] + s[:, sx1] * a1.astype(np.int32)[None, :, None]     # (h, dw, C) int32
    r0, r1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    b0, b1 = b0.astype(np.int32)[:, None, None], b1.astype(np.int32)[:, None, None]
    out = (((b0 * (hor[r0] >> 4)) >> 16) + ((b1 * (hor[r1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ---- FaceDetector.scale_detect's host steps (test_tools/ct/detection/__init__.py)

MAX_RES = 1920


def scale_detect_scale(h: int, w: int):
    """lines 43-49: ``resize_scale`` for frames of h x w: the int 2 up to 1920 on the long side, a float above"""
    init_scale = max(h, w) / MAX_RES if max(h, w) > MAX_RES else 1
    return 2 * init_scale


def scale_detect_size(h: int, w: int):
    """lines 50-51: ``(resize_w, resize_h)``, the size the frames are detected at.  1x1 gives (0, 0): cv2.resize fails there"""
    s = scale_detect_scale(h, w)
    return int(w / s), int(h / s)


def _bounded(v, low, up) -> bool:
    return bool(v >= low and v < up)


def check_valid(face, w, h) -> bool:
    box = face[0]
    if box[0] > box[2] or box[1] > box[3]:
        return False
    for i, bound in zip((0, 1, 2, 3), (w, h, w, h)):
        if not _bounded(box[i], 0, bound):
            return False
    for p in face[1]:
        for i, bound in zip((0, 1), (w, h)):
            if not _bounded(p[i], 0, bound):
                return False
    return True


def post_detect(detect_results, scale, w, h):
    """boxes and landmarks times `scale` in the dtype numpy gives ``float32 array * python number`` (float32), invalid faces dropped"""
    out = []
    for faces in detect_results:
        kept = []
        for box, ldm, score in faces:
            face = (box * scale, ldm * scale, score)
            if check_valid(face, w=w, h=h):
                kept.append(face)
        out.append(kept)
    return out
