"""numpy statement of the YUV conversions of csrc/af_yuv_formats.hip, on top of yuv_ref.py: twelve formats (8-bit 4:2:0, packed / planar /
semi-planar 4:2:2, planar 4:4:4, 10-bit 4:2:0), BT.601 and BT.709, limited and full range.

The arithmetic has OpenCV's form (color_yuv.simd.hpp) - int32, a shift by 20 - and at (bt601, limited, 8-bit) OpenCV's own table, which
yuv_ref.py holds; there the packed 4:2:2 formats are OpenCV's COLOR_YUV2BGR_YUY2 / _UYVY / _YVYU, which use the same helper per pixel
pair.  Every other table is NOT OpenCV's: ``table`` derives it from Kr and Kb as exact rationals, each coefficient rounded half up to
2^-20.  Like yuv_ref.py this is unpinned against cv2 itself, absent where this is built; tests/test_yuv_formats_host.py pins it with
hand-worked anchors and against the fp64 conversion over the whole 8-bit cube and a 10-bit lattice."""
from fractions import Fraction

import numpy as np

import yuv_ref as R

SHIFT, HALF = R.SHIFT, R.HALF
KR_KB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}
#         planes ("planar" y, u, v / "semi" y, uv / "packed" one plane), rows of Y per chroma row, pixels per (U, V) in a row, bits
FORMATS = {"nv12": ("semi", 2, 2, 8), "nv21": ("semi", 2, 2, 8), "i420": ("planar", 2, 2, 8), "yv12": ("planar", 2, 2, 8),
           "yuy2": ("packed", 1, 2, 8), "uyvy": ("packed", 1, 2, 8), "yvyu": ("packed", 1, 2, 8), "i422": ("planar", 1, 2, 8),
           "nv16": ("semi", 1, 2, 8), "i444": ("planar", 1, 1, 8), "p010": ("semi", 2, 2, 10), "i010": ("planar", 2, 2, 10)}
PACKED_AT = {"yuy2": (0, 2, 1, 3), "uyvy": (1, 3, 0, 2), "yvyu": (0, 2, 3, 1)}       # byte of Y0, Y1, U, V in a pixel pair's four
COLOURS = [(m, f) for f in (False, True) for m in ("bt601", "bt709")]


def _half_up(x: Fraction) -> int:
    return (x * (1 << SHIFT) + Fraction(1, 2)).__floor__()


def scales(full_range: bool, bits: int):
    """(luma scale, chroma scale) onto 0..255 as exact rationals"""
    if full_range:
        return (Fraction(1), Fraction(1)) if bits == 8 else (Fraction(255, 1023), Fraction(255, 1023))
    return (Fraction(255, 219), Fraction(255, 224)) if bits == 8 else (Fraction(255, 876), Fraction(255, 896))


def exact(matrix: str, full_range: bool, bits: int):
    """(CY, CVR, CVG, CUG, CUB) as exact rationals"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc = scales(full_range, bits)
    return sy, 2 * (1 - kr) * sc, -2 * kr * (1 - kr) / kg * sc, -2 * kb * (1 - kb) / kg * sc, 2 * (1 - kb) * sc


def table(matrix: str = "bt601", full_range: bool = False, bits: int = 8):
    """(CY, CVR, CVG, CUG, CUB) in units of 2^-20: OpenCV's at (bt601, limited, 8-bit), else derived"""
    if (matrix, bool(full_range), bits) == ("bt601", False, 8):
        return R.CY, R.CVR, R.CVG, R.CUG, R.CUB
    return tuple(_half_up(c) for c in exact(matrix, full_range, bits))


def offsets(full_range: bool, bits: int):
    """(Yoff, Cmid)"""
    return (0 if full_range else 16 << (bits - 8)), 128 << (bits - 8)


def terms(Y, U, V, matrix="bt601", full_range=False, bits=8):
    """element-wise samples -> the three int64 sums in front of the shift (R, G, B), unclamped"""
    cy, cvr, cvg, cug, cub = table(matrix, full_range, bits)
    yoff, cmid = offsets(full_range, bits)
    y = np.maximum(0, np.asarray(Y).astype(np.int64) - yoff) * cy
    u, v = np.asarray(U).astype(np.int64) - cmid, np.asarray(V).astype(np.int64) - cmid
    return y + HALF + cvr * v, y + HALF + cvg * v + cug * u, y + HALF + cub * u


def yuv_to_bgr(Y, U, V, matrix="bt601", full_range=False, bits=8) -> np.ndarray:
    """element-wise samples (values 0 .. 2^bits - 1) of one shape -> (..., 3) uint8, channels B, G, R"""
    r, g, b = terms(Y, U, V, matrix, full_range, bits)
    assert max(int(np.abs(c).max()) for c in (r, g, b)) < 2 ** 31
    return np.clip(np.stack([b >> SHIFT, g >> SHIFT, r >> SHIFT], axis=-1), 0, 255).astype(np.uint8)      # >> on signed: arithmetic


def real_bgr(Y, U, V, matrix="bt601", full_range=False, bits=8) -> np.ndarray:
    """the exact conversion in fp64, unrounded and unclamped: (..., 3) B, G, R on the 0..255 scale"""
    cy, cvr, cvg, cug, cub = (float(c) for c in exact(matrix, full_range, bits))
    yoff, cmid = offsets(full_range, bits)
    y = np.maximum(0, np.asarray(Y).astype(np.float64) - yoff) * cy
    u, v = np.asarray(U).astype(np.float64) - cmid, np.asarray(V).astype(np.float64) - cmid
    return np.stack([y + cub * u, y + cvg * v + cug * u, y + cvr * v], axis=-1)


def values(raw, fmt):
    """samples as they lie in memory -> their values: p010 holds them in bits 15..6, i010 in the low bits (clamped to 1023)"""
    if fmt == "p010":
        return np.asarray(raw) >> 6
    if fmt == "i010":
        return np.minimum(np.asarray(raw), 1023)
    return np.asarray(raw)


def chroma_shape(fmt, h, w):
    _, vdiv, hdiv, _ = FORMATS[fmt]
    return h // vdiv, w // hdiv


def pack(y, u, v, fmt):
    """Y (h, w) and U, V at the format's chroma size, as stored samples -> the planes in the order ``YuvFrame`` takes them:
    (packed,), (y, uv) or (y, u, v)"""
    kind = FORMATS[fmt][0]
    h, w = y.shape
    assert u.shape == v.shape == chroma_shape(fmt, h, w), (fmt, y.shape, u.shape)
    if kind == "packed":
        out = np.zeros((h, w // 2, 4), y.dtype)
        a, b, c, d = PACKED_AT[fmt]
        out[..., a], out[..., b], out[..., c], out[..., d] = y[:, 0::2], y[:, 1::2], u, v
        return (out.reshape(h, 2 * w),)
    if kind == "semi":
        first, second = (v, u) if fmt == "nv21" else (u, v)
        return y.copy(), np.stack([first, second], axis=-1).reshape(u.shape[0], 2 * u.shape[1])
    return y.copy(), u.copy(), v.copy()


def split(planes, fmt):
    """the inverse of ``pack``: planes -> (Y, U, V) stored samples, U and V at the format's chroma size"""
    kind = FORMATS[fmt][0]
    if kind == "packed":
        p = planes[0].reshape(planes[0].shape[0], -1, 4)
        a, b, c, d = PACKED_AT[fmt]
        y = np.stack([p[..., a], p[..., b]], axis=-1).reshape(p.shape[0], -1)
        return y, p[..., c].copy(), p[..., d].copy()
    if kind == "semi":
        y, uv = planes
        first, second = uv[:, 0::2].copy(), uv[:, 1::2].copy()
        return (y, second, first) if fmt == "nv21" else (y, first, second)
    return tuple(planes)


def buffer(planes, fmt):
    """planes of a planar or semi-planar format -> the one contiguous 2-D array ``YuvFrame.from_packed`` takes (V before U for yv12)"""
    kind = FORMATS[fmt][0]
    assert kind != "packed"
    y = planes[0]
    rest = list(planes[1:])
    if fmt == "yv12":
        rest = rest[::-1]
    return np.concatenate([y.reshape(-1)] + [p.reshape(-1) for p in rest]).reshape(-1, y.shape[1])


def kwargs(planes, fmt):
    """planes -> the keyword arguments of ``YuvFrame(fmt, **...)``"""
    kind = FORMATS[fmt][0]
    if kind == "packed":
        return dict(y=planes[0])
    return dict(y=planes[0], uv=planes[1]) if kind == "semi" else dict(y=planes[0], u=planes[1], v=planes[2])


def convert(planes, fmt, matrix="bt601", full_range=False, order="bgr") -> np.ndarray:
    """the planes of one frame as ``YuvFrame`` takes them -> (h, w, 3) uint8 in `order` ('bgr' or 'rgb')"""
    _, vdiv, hdiv, bits = FORMATS[fmt]
    y, u, v = (values(p, fmt) for p in split(planes, fmt))
    h, w = y.shape
    assert w % 2 == 0 and h % vdiv == 0 and u.shape == v.shape == (h // vdiv, w // hdiv)
    u, v = (np.repeat(np.repeat(c, vdiv, 0), hdiv, 1) for c in (u, v))
    bgr = yuv_to_bgr(y, u, v, matrix, full_range, bits)
    return bgr if order == "bgr" else np.ascontiguousarray(bgr[..., ::-1])


def random_planes(fmt, h, w, seed):
    """random stored samples of one frame: any 16 bits for p010 (the low six are to be ignored) and for i010 (values above 1023
    are to be clamped)"""
    rng = np.random.default_rng(seed)
    bits = FORMATS[fmt][3]
    dtype, top = (np.uint8, 256) if bits == 8 else (np.uint16, 65536)
    ch = chroma_shape(fmt, h, w)
    y, u, v = (rng.integers(0, top, s, dtype=dtype) for s in ((h, w), ch, ch))
    if fmt == "i010":                                             # mostly in range, some above
        y, u, v = (np.where(c % 8 == 0, c, c & 1023).astype(np.uint16) for c in (y, u, v))
    return pack(y, u, v, fmt)
