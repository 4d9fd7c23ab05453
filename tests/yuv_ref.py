"""numpy restatement of OpenCV's YUV 4:2:0 -> BGR / RGB conversion (``cvtColor(..., COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12)``,
modules/imgproc/src/color_yuv.simd.hpp): the fixed-point BT.601 limited-range arithmetic, integer only, one (U, V) per 2 x 2 block of
Y, no chroma interpolation.  Like quality_ref.py it restates OpenCV's code and is NOT pinned against cv2 itself, which is absent
where this is built; tests/test_yuv_host.py pins it with hand-worked anchors and its sums over the whole (Y, U, V) cube."""
import numpy as np

CY, CUB, CUG, CVG, CVR, SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20
HALF = 1 << (SHIFT - 1)


def yuv_to_bgr(Y, U, V) -> np.ndarray:
    """element-wise (Y, U, V) uint8 arrays of one shape -> (..., 3) uint8, channels B, G, R"""
    y = np.maximum(0, np.asarray(Y).astype(np.int32) - 16) * np.int32(CY)
    u = np.asarray(U).astype(np.int32) - 128
    v = np.asarray(V).astype(np.int32) - 128
    r = (y + HALF + CVR * v) >> SHIFT                      # int32 throughout; >> on a signed numpy integer is arithmetic
    g = (y + HALF + CVG * v + CUG * u) >> SHIFT
    b = (y + HALF + CUB * u) >> SHIFT
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def planes_to_bgr(y, u, v) -> np.ndarray:
    """Y (h, w) and U, V (h / 2, w / 2) -> (h, w, 3) B, G, R: every 2 x 2 block of Y shares its (U, V)"""
    h, w = y.shape
    if h % 2 or w % 2 or u.shape != (h // 2, w // 2) or v.shape != u.shape:
        raise ValueError("yuv_ref: %s Y with %s U and %s V" % (y.shape, u.shape, v.shape))
    return yuv_to_bgr(y, np.repeat(np.repeat(u, 2, 0), 2, 1), np.repeat(np.repeat(v, 2, 0), 2, 1))


def split_packed(buf: np.ndarray, h: int, w: int, fmt: str):
    """the (h * 3 / 2, w) packed buffer of `fmt` -> copies of its (Y, U, V) planes"""
    buf = np.ascontiguousarray(buf)
    assert buf.shape == (h * 3 // 2, w) and buf.dtype == np.uint8
    y, c = buf[:h].copy(), buf[h:].reshape(-1)
    if fmt in ("nv12", "nv21"):
        first, second = c[0::2].reshape(h // 2, w // 2).copy(), c[1::2].reshape(h // 2, w // 2).copy()
    elif fmt in ("i420", "yv12"):
        q = h * w // 4
        first, second = c[:q].reshape(h // 2, w // 2).copy(), c[q:].reshape(h // 2, w // 2).copy()
    else:
        raise ValueError(fmt)
    return (y, second, first) if fmt in ("nv21", "yv12") else (y, first, second)


def packed_to(buf: np.ndarray, h: int, w: int, fmt: str, order: str = "bgr") -> np.ndarray:
    """cvtColor(buf, COLOR_YUV2<order>_<fmt>): the packed buffer -> (h, w, 3) in `order` ('bgr' or 'rgb')"""
    bgr = planes_to_bgr(*split_packed(buf, h, w, fmt))
    return bgr if order == "bgr" else np.ascontiguousarray(bgr[..., ::-1])


def pack(y, u, v, fmt: str) -> np.ndarray:
    """(Y, U, V) planes -> the packed (h * 3 / 2, w) buffer of `fmt`"""
    h, w = y.shape
    first, second = (v, u) if fmt in ("nv21", "yv12") else (u, v)
    if fmt in ("nv12", "nv21"):
        c = np.stack([first, second], axis=-1).reshape(h // 2, w)
    else:
        c = np.concatenate([first.reshape(-1), second.reshape(-1)]).reshape(h // 2, w)
    return np.concatenate([y, c], axis=0)
