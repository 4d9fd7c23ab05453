"""The pixel part of the reference's quality gate in numpy, the statement csrc/af_quality.hip is checked against:
``_frame_quality_weight`` (test/af_realtime.py:265-267) with ``variance_of_laplacian`` (:191-192),

    small = cv2.resize(crop_rgb, (max(1, w // 2), max(1, h // 2)), interpolation=cv2.INTER_AREA)
    lap = cv2.Laplacian(cv2.cvtColor(small, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()

restated from OpenCV 4.x's sources (resize.cpp: ResizeAreaFastVec / ResizeAreaFast_Invoker / computeResizeAreaTab + ResizeArea_Invoker;
color_rgb: the 15-bit RGB2GRAY; deriv.cpp: Laplacian with ksize 1 and BORDER_DEFAULT).  cv2 is not installed where this project is
built, so - like the aligner's warp - the restatement is pinned by hand-worked cases (tests/test_realtime_host.py), not against cv2.

  half size   dw = max(1, w // 2), dh = max(1, h // 2), per channel, to uint8:
              w == 2 dw and h == 2 dh       (a + b + c + d + 2) >> 2
              both w / dw and h / dh whole  fp32(box sum) * fp32(1 / area), rounded half to even
              otherwise                     the area table: cell bounds in fp64, weights cast to fp32, fp32 accumulation along x in
                                            table order, then over the rows with their weights, rounded half to even, saturated
  grey        (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15 on the resized bytes
  Laplacian   up + down + left + right - 4 * centre, BORDER_REFLECT_101 (index -1 -> 1, n -> n - 2, a dimension of 1 -> 0)
  sums        S1 = sum L, S2 = sum L^2, n_px = dw * dh, all exact integers; lap = (n_px * S2 - S1^2) / n_px^2
"""
import numpy as np

F32 = np.float32


def area_table(ssize: int, dsize: int):
    """computeResizeAreaTab: ``[(destination index, source index, fp32 weight)]`` in table order"""
    scale = ssize / dsize                                    # fp64
    tab = []
    for dx in range(dsize):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            tab.append((dx, sx1 - 1, F32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            tab.append((dx, sx, F32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            tab.append((dx, sx2, F32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
    return tab


def _round_sat_u8(v) -> np.ndarray:
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)      # rint: half to even, as cvRound


def half_size(crop: np.ndarray) -> np.ndarray:
    """``cv2.resize(crop, (max(1, w // 2), max(1, h // 2)), interpolation=cv2.INTER_AREA)`` of an HxWx3 uint8 crop"""
    h, w = crop.shape[:2]
    dw, dh = max(1, w // 2), max(1, h // 2)
    if w == 2 * dw and h == 2 * dh:
        c = crop.astype(np.int32)
        return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    if w % dw == 0 and h % dh == 0:
        kx, ky = w // dw, h // dh
        box = crop.astype(np.int32).reshape(dh, ky, dw, kx, 3).sum(axis=(1, 3))
        return _round_sat_u8(box.astype(F32) * (F32(1.0) / F32(kx * ky)))
    xtab, ytab = area_table(w, dw), area_table(h, dh)
    src = crop.astype(F32)
    out = np.zeros((dh, dw, 3), F32)
    started = set()
    for dy, sy, beta in ytab:
        buf = np.zeros((dw, 3), F32)
        for dx, sx, alpha in xtab:
            buf[dx] = buf[dx] + src[sy, sx] * alpha           # fp32 multiply, then fp32 add: no fused multiply-add
        if dy in started:
            out[dy] = out[dy] + beta * buf
        else:
            out[dy] = beta * buf
            started.add(dy)
    return _round_sat_u8(out)


def grey(small: np.ndarray, channel_order: str = "rgb") -> np.ndarray:
    s = small.astype(np.int32)
    r, b = (s[..., 0], s[..., 2]) if channel_order == "rgb" else (s[..., 2], s[..., 0])
    return ((r * 9798 + s[..., 1] * 19235 + b * 3735 + 16384) >> 15).astype(np.uint8)


def _reflect101(i: int, n: int) -> int:
    return 0 if n == 1 else (-i if i < 0 else (2 * n - 2 - i if i >= n else i))


def laplacian(g: np.ndarray) -> np.ndarray:
    """int64 (dh, dw): the 4-neighbour Laplacian of a uint8 image with BORDER_REFLECT_101"""
    n, m = g.shape
    v = g.astype(np.int64)
    rows_up, rows_dn = [_reflect101(y - 1, n) for y in range(n)], [_reflect101(y + 1, n) for y in range(n)]
    cols_l, cols_r = [_reflect101(x - 1, m) for x in range(m)], [_reflect101(x + 1, m) for x in range(m)]
    return v[rows_up] + v[rows_dn] + v[:, cols_l] + v[:, cols_r] - 4 * v


def quality_sums(crop: np.ndarray, channel_order: str = "rgb"):
    """``(n_px, S1, S2, grey image)`` of a crop as Python integers and a (dh, dw) uint8 array"""
    g = grey(half_size(crop), channel_order)
    lap = laplacian(g)
    return int(g.size), int(lap.sum()), int((lap * lap).sum()), g


def variance(n_px: int, s1: int, s2: int) -> float:
    """the population variance from exact integers, one fp64 division"""
    return (n_px * s2 - s1 * s1) / (n_px * n_px)


def min_side_and_lap(crop: np.ndarray, channel_order: str = "rgb"):
    n, s1, s2, _ = quality_sums(crop, channel_order)
    return float(min(crop.shape[:2])), variance(n, s1, s2)
