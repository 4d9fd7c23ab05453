"""What the reference's capture code does to a bitmap before ``RealtimeAF.step`` sees it, in numpy - the statement
csrc/af_capture.hip is checked against (test/win_capture.py:37, :110-115; test/capture_tile.py:190, :199-201):

    frame = cv2.cvtColor(bitmap, cv2.COLOR_BGRA2BGR)                                 the alpha byte is dropped
    frame = frame[y0:y1, x0:x1]                                                       the window's client rectangle
    if max_w > 0 and frame.shape[1] > max_w:
        frame = cv2.resize(frame, (max_w, int(frame.shape[0] * (max_w / frame.shape[1]))), interpolation=cv2.INTER_AREA)

``area_resize`` restates cv2.INTER_AREA for 8-bit images from OpenCV 4.x's resize.cpp, per channel, for dw <= w and dh <= h:

    dw == w and dh == h                     a copy
    w == 2 dw and h == 2 dh                 (a + b + c + d + 2) >> 2                                      (ResizeAreaFastVec)
    w % dw == 0 and h % dh == 0             fp32(integer box sum) * (fp32(1) / fp32(kx ky)), half to even  (ResizeAreaFast_Invoker)
    otherwise                               computeResizeAreaTab on BOTH axes - also when one of them is a whole ratio, which does
                                            not give the box bytes - with fp32 accumulation in table order  (ResizeArea_Invoker)

The table and the rounding are tests/quality_ref.py's ``area_table`` and ``_round_sat_u8``, imported, not restated.  cv2 is not
installed where this project is built, so - like the warp, the YUV and the bilinear resize statements - this one is pinned by
hand-worked anchors and by its tie to the already pinned ``quality_ref.half_size`` (tests/test_capture_host.py), not against cv2."""
import numpy as np

from quality_ref import F32, _round_sat_u8, area_table

FORMATS = {"bgra": (4, "bgr"), "rgba": (4, "rgb"), "bgr": (3, "bgr"), "rgb": (3, "rgb")}


def capture_size(h: int, w: int, max_w: int):
    """``(dw, dh)``: test/capture_tile.py:199-201"""
    if max_w > 0 and w > max_w:
        new_h = int(h * (max_w / w))
        return max_w, new_h
    return w, h


def mode(h: int, w: int, dh: int, dw: int) -> str:
    if dw == w and dh == h:
        return "copy"
    if w == 2 * dw and h == 2 * dh:
        return "area2"
    if w % dw == 0 and h % dh == 0:
        return "box"
    return "table"


def area_resize(img: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """``cv2.resize(img, (dw, dh), interpolation=cv2.INTER_AREA)`` of an HxWxC uint8 image, dw <= W and dh <= H"""
    h, w, ch = img.shape
    assert 1 <= dw <= w and 1 <= dh <= h
    m = mode(h, w, dh, dw)
    if m == "copy":
        return img.copy()
    if m == "area2":
        c = img.astype(np.int32)
        return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    if m == "box":
        kx, ky = w // dw, h // dh
        box = img.astype(np.int64).reshape(dh, ky, dw, kx, ch).sum(axis=(1, 3))
        return _round_sat_u8(box.astype(F32) * (F32(1.0) / F32(kx * ky)))
    xtab, ytab = area_table(w, dw), area_table(h, dh)
    src = img.astype(F32)
    # the horizontal pass of a source row does not depend on the destination row that asks for it: all h rows at once, each
    # element still buf = buf + s * alpha over the x taps in table order (quality_ref.half_size computes it per (dy, sy) instead)
    buf = np.zeros((h, dw, ch), F32)
    for dx, sx, alpha in xtab:
        buf[:, dx] = buf[:, dx] + src[:, sx] * alpha          # fp32 multiply, then fp32 add: no fused multiply-add
    out = np.zeros((dh, dw, ch), F32)
    started = set()
    for dy, sy, beta in ytab:
        if dy in started:
            out[dy] = out[dy] + beta * buf[sy]
        else:
            out[dy] = beta * buf[sy]
            started.add(dy)
    return _round_sat_u8(out)


def captured(pixels: np.ndarray, fmt: str, rect, dw: int, dh: int, order: str) -> np.ndarray:
    """the (dh, dw, 3) frame a store in `order` holds for a captured bitmap: alpha stripped, cropped, resized, ordered"""
    _, src_order = FORMATS[fmt]
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, pixels.shape[1], pixels.shape[0])
    frame = np.ascontiguousarray(pixels[y0:y1, x0:x1, :3])
    small = area_resize(frame, dw, dh)
    return small if order == src_order else np.ascontiguousarray(small[..., ::-1])
