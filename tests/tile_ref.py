"""The reference's speaker-tile choice in numpy, the statement csrc/af_tile.hip and ``TilePicker`` are checked against:
``LargestTilePicker`` (test/capture_tile.py:55-109) and the clamp of ``iter_roi_frames`` (:204-207),

    g = cv2.GaussianBlur(cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY), (5, 5), 0)
    e = cv2.dilate(cv2.Canny(g, 50, 150), np.ones((3, 3), np.uint8), 1)
    cnts, _ = cv2.findContours(e, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)          # boundingRect, _valid, roi.var() < 50, sort

restated from OpenCV 4.x's plain C++ path (color_rgb: the 15-bit BGR2GRAY; smooth: the 8-bit fixed-point Gaussian; canny.cpp;
morph; contours + shapedescr).  cv2 is not installed where this project is built, so - like tests/capture_ref.py and
tests/quality_ref.py - the restatement is pinned by the hand-worked cases of tests/test_tile_host.py: unpinned vs cv2 itself,
absent here.

  grey       (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15                                        (quality_ref.grey)
  blur       the tabulated kernel [1, 4, 6, 4, 1] / 16 as 8.8 fixed point on both axes: exact, so g = (S + 128) >> 8 with
             S = sum k_i k_j p, BORDER_REFLECT_101
  Sobel      3 x 3 dx, dy of g as integers, BORDER_REPLICATE; m = |dx| + |dy| (L1); m outside the image is 0
  NMS        candidate: m > 50 and, with TG22 = 13573, x = |dx|, y = |dy| << 15:
               y < x * TG22               horizontal   m > left and m >= right
               y > x * TG22 + (x << 16)   vertical     m > up and m >= down
               otherwise                  diagonal     dx, dy of equal sign: (x-1, y-1) and (x+1, y+1), else the other diagonal;
                                                       both comparisons strict
             strong: a candidate with m > 150
  edges      every candidate that is 8-connected, through candidates, to a strong one: a set, so OpenCV's stack order does not
             matter
  dilate     3 x 3 once: the maximum over the neighbours inside the image
  contours   RETR_EXTERNAL + boundingRect: the 8-connected components of the non-zero pixels that are not enclosed.  A component
             is kept when it touches the image border, or is 4-adjacent to background that is 4-connected to the border (OpenCV
             pads one zero pixel; both cases are "4-adjacent to the padded background's outer component").  Its box is
             (minx, miny, maxx - minx + 1, maxy - miny + 1).
  choice     _valid, roi = g[y+4:y+h-4, x+4:x+w-4] of the BLURRED grey, roi.size == 0 or roi.var() < 50 rejects, the largest
             (area, box) tuple wins.  Under _valid's own constants h >= 120, so the slice bounds are never negative; with the
             constants opened (tests) a box of 8 or fewer rows or columns has an empty roi - no wrap-around reading.
  motion     runs only when the above gave nothing, and only then is prev_gray replaced.  UNBLURRED grey; |diff| > 16;
             medianBlur 5 of a 0 / 255 image: at least 13 of the 25 BORDER_REPLICATE neighbours set; two 5 x 5 dilations: a 9 x 9
             maximum inside the image; boxes with w * h >= 0.01 * W * H, their union, the 16:9 fit in Python ints
  pick       smoothing with a = 0.6 and int(), the cool = 10 countdown, the full-frame default; ``roi`` adds the clamp.
"""
import numpy as np
from scipy import ndimage

import quality_ref as Q

TG22 = 13573                       # int(0.4142135623730950488016887242097 * 2 ** 15 + 0.5)
LOW, HIGH = 50, 150
EIGHT = np.ones((3, 3), dtype=bool)
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
# LargestTilePicker._valid's constants, in the order the device is handed them
VALID = {"min_w": 200, "min_h": 120, "ar_lo": 1.2, "ar_hi": 2.2, "area_frac": 0.10}
VAR_MIN, MOTION_FRAC, MOTION_THRESHOLD = 50, 0.01, 16


def grey(frame: np.ndarray, channel_order: str = "bgr") -> np.ndarray:
    return Q.grey(frame, channel_order)


def _reflect101(i: int, n: int) -> int:
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


def blur(g: np.ndarray) -> np.ndarray:
    """``cv2.GaussianBlur(g, (5, 5), 0)`` of a uint8 image with both sides >= 3"""
    h, w = g.shape
    v = g.astype(np.int64)
    k = (1, 4, 6, 4, 1)                                        # * 16 = the 8.8 fixed-point taps; S below carries the factor 256
    rows = sum(k[i] * v[[_reflect101(y + i - 2, h) for y in range(h)]] for i in range(5))
    s = sum(k[j] * rows[:, [_reflect101(x + j - 2, w) for x in range(w)]] for j in range(5))
    return ((s + 128) >> 8).astype(np.uint8)


def sobel(g: np.ndarray):
    """(dx, dy) int32: the 3 x 3 Sobel derivatives with BORDER_REPLICATE"""
    p = np.pad(g.astype(np.int32), 1, mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy


def nms_classes(dx: np.ndarray, dy: np.ndarray) -> np.ndarray:
    """uint8 (H, W): 0 none, 1 candidate, 2 strong candidate"""
    h, w = dx.shape
    dx, dy = dx.astype(np.int64), dy.astype(np.int64)
    m = np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1)                                          # the magnitude outside the image is 0
    at = lambda oy, ox: mp[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]
    x, y = np.abs(dx), np.abs(dy) << 15
    horizontal = y < x * TG22
    vertical = ~horizontal & (y > x * TG22 + (x << 16))
    same = (dx ^ dy) >= 0                                      # the signs of dx and dy agree (neither is 0 on this branch)
    keep = np.where(horizontal, (m > at(0, -1)) & (m >= at(0, 1)),
                    np.where(vertical, (m > at(-1, 0)) & (m >= at(1, 0)),
                             np.where(same, (m > at(-1, -1)) & (m > at(1, 1)), (m > at(-1, 1)) & (m > at(1, -1)))))
    keep &= m > LOW
    return np.where(keep, np.where(m > HIGH, 2, 1), 0).astype(np.uint8)


def hysteresis(cls: np.ndarray) -> np.ndarray:
    """uint8 0 / 255: the candidates 8-connected, through candidates, to a strong one"""
    lab, n = ndimage.label(cls > 0, structure=EIGHT)
    keep = np.zeros(n + 1, bool)
    keep[np.unique(lab[cls == 2])] = True
    keep[0] = False
    return np.where(keep[lab], 255, 0).astype(np.uint8)


def canny(g: np.ndarray) -> np.ndarray:
    return hysteresis(nms_classes(*sobel(g)))


def box_max(mask: np.ndarray, r: int) -> np.ndarray:
    """the maximum over the (2 r + 1)^2 neighbours inside the image: r = 1 is one 3 x 3 dilation, r = 4 two 5 x 5 ones"""
    h, w = mask.shape
    p = np.pad(mask, r)
    out = np.zeros_like(mask)
    for oy in range(2 * r + 1):
        for ox in range(2 * r + 1):
            out = np.maximum(out, p[oy:oy + h, ox:ox + w])
    return out


def components(mask: np.ndarray):
    """The 8-connected components of the non-zero pixels of `mask` -> ``(labels, comps)``: ``labels`` int32 (H, W), a pixel's
    component named by the smallest flat index y * W + x of its pixels (the device's root), -1 for background; ``comps`` a list of
    ``(root, (x, y, w, h), external)`` by ascending root."""
    h, w = mask.shape
    fg = mask != 0
    lab, n = ndimage.label(fg, structure=EIGHT)
    pad_bg = np.pad(~fg, 1, constant_values=True)
    blab, _ = ndimage.label(pad_bg, structure=FOUR)
    outer = blab == blab[0, 0]                                 # the padded background's component that holds the pad
    near = outer[:-2, 1:-1] | outer[2:, 1:-1] | outer[1:-1, :-2] | outer[1:-1, 2:]      # 4-adjacent to it
    labels = np.full((h, w), -1, np.int32)
    comps = []
    for k, sl in enumerate(ndimage.find_objects(lab), 1):
        ys, xs = sl
        part = lab[sl] == k
        root = int(np.flatnonzero(lab.reshape(-1) == k)[0])
        labels[sl][part] = root
        comps.append((root, (xs.start, ys.start, xs.stop - xs.start, ys.stop - ys.start), bool((near[sl] & part).any())))
    comps.sort()
    return labels, comps


def external_boxes(mask: np.ndarray):
    """``cv2.findContours(mask, cv2.RETR_EXTERNAL, ...)`` + ``cv2.boundingRect``: the boxes, by ascending root"""
    return [box for _, box, ext in components(mask)[1] if ext]


def valid(W, H, ww, hh, p=VALID) -> bool:
    if ww < p["min_w"] or hh < p["min_h"]:
        return False
    ar = ww / float(hh)
    return p["ar_lo"] <= ar <= p["ar_hi"] and ww * hh >= p["area_frac"] * W * H


def roi_of(g: np.ndarray, box):
    x, y, w, h = box
    if w <= 8 or h <= 8:
        return g[0:0, 0:0]
    return g[y + 4:y + h - 4, x + 4:x + w - 4]


def tile_candidates(frame: np.ndarray, channel_order: str = "bgr", params=VALID):
    """-> ``(survivors, stages)``: ``survivors`` = [(root, (x, y, w, h), n, S1, S2)] of the external boxes that pass ``_valid``,
    with the exact sums of the blurred grey over the inset roi, by ascending root; ``stages`` = dict of g, cls, edges, mask, labels"""
    H, W = frame.shape[:2]
    g = blur(grey(frame, channel_order))
    cls = nms_classes(*sobel(g))
    e = hysteresis(cls)
    mask = box_max(e, 1)
    labels, comps = components(mask)
    out = []
    for root, box, ext in comps:
        if not ext or not valid(W, H, box[2], box[3], params):
            continue
        r = roi_of(g, box).astype(np.int64)
        out.append((root, box, int(r.size), int(r.sum()), int((r * r).sum())))
    return out, {"g": g, "cls": cls, "edges": e, "mask": mask, "labels": labels, "comps": comps}


def variances(survivors):
    """numpy's fp64 ``roi.var()`` of every survivor with a non-empty roi (the tests keep each 1e-6 away from 50)"""
    return [(n * s2 - s1 * s1) / (n * n) for _, _, n, s1, s2 in survivors if n]


def choose(survivors):
    """the variance test in integers and the sort of :71-74 -> (x0, y0, x1, y1) or None"""
    cand = []
    for _, (x, y, w, h), n, s1, s2 in survivors:
        if n == 0 or n * s2 - s1 * s1 < VAR_MIN * n * n:
            continue
        cand.append((w * h, (x, y, x + w, y + h)))
    if not cand:
        return None
    cand.sort(reverse=True)
    return cand[0][1]


def tiles(frame: np.ndarray, channel_order: str = "bgr", params=VALID):
    return choose(tile_candidates(frame, channel_order, params)[0])


def median5(th: np.ndarray) -> np.ndarray:
    """``cv2.medianBlur(th, 5)`` of a 0 / 1 image: at least 13 of the 25 BORDER_REPLICATE neighbours set"""
    h, w = th.shape
    p = np.pad(th.astype(np.int32), 2, mode="edge")
    cnt = sum(p[oy:oy + h, ox:ox + w] for oy in range(5) for ox in range(5))
    return (cnt >= 13).astype(np.uint8)


def motion_mask(g: np.ndarray, prev: np.ndarray) -> np.ndarray:
    th = (np.abs(g.astype(np.int32) - prev.astype(np.int32)) > MOTION_THRESHOLD).astype(np.uint8)
    return box_max(median5(th), 4)


def motion_union(mask: np.ndarray):
    """-> (x1, y1, x2, y2, count) over the components with w * h >= 0.01 * W * H.  Nested components lie inside their parent's
    box, so the union over ALL components equals the union over the external ones the reference walks."""
    H, W = mask.shape
    x1, y1, x2, y2, count = W, H, 0, 0, 0
    for _, (x, y, w, h), _ in components(mask)[1]:
        if w * h < MOTION_FRAC * W * H:
            continue
        x1, y1, x2, y2, count = min(x1, x), min(y1, y), max(x2, x + w), max(y2, y + h), count + 1
    return x1, y1, x2, y2, count


def fit_16_9(x1, y1, x2, y2, W, H):
    """:89-95 as written, in Python ints and floats"""
    if x2 <= x1 or y2 <= y1:
        return None
    ar = 16 / 9
    ww, hh = x2 - x1, y2 - y1
    if ww / hh > ar:
        nh = int(ww / ar); cy = (y1 + y2) // 2; y1 = max(0, cy - nh // 2); y2 = min(H, y1 + nh)
    else:
        nw = int(hh * ar); cx = (x1 + x2) // 2; x1 = max(0, cx - nw // 2); x2 = min(W, x1 + nw)
    return (x1, y1, x2, y2)


def smooth(prev, box, a=0.6):
    return tuple(int(a * p + (1 - a) * b) for p, b in zip(prev, box))


def clamp(box, W, H):
    """iter_roi_frames:204-207"""
    l, t, r, b = box
    l = max(0, min(W - 1, l))
    t = max(0, min(H - 1, t))
    r = max(l + 1, min(W, r))
    b = max(t + 1, min(H, b))
    return l, t, r, b


class Picker:
    """``LargestTilePicker`` on the statement's stages; ``tiles_fn`` / ``motion_fn`` (tests of the state machine alone) replace
    them.  ``motion_runs`` counts the calls of ``_motion``."""

    def __init__(self, channel_order: str = "bgr", params=VALID, tiles_fn=None):
        self.order, self.params, self.tiles_fn = channel_order, params, tiles_fn
        self.reset()

    def reset(self):
        self.prev_gray, self.prev_tile, self.cool, self.motion_runs = None, None, 0, 0

    def tiles(self, frame):
        return self.tiles_fn(frame) if self.tiles_fn else tiles(frame, self.order, self.params)

    def motion(self, frame):
        self.motion_runs += 1
        H, W = frame.shape[:2]
        g = grey(frame, self.order)
        if self.prev_gray is None:
            self.prev_gray = g.copy()
            return None
        mask = motion_mask(g, self.prev_gray)
        self.prev_gray = g
        x1, y1, x2, y2, _ = motion_union(mask)
        return fit_16_9(x1, y1, x2, y2, W, H)

    def pick(self, frame):
        box = self.tiles(frame) or self.motion(frame)
        if box is None:
            if self.prev_tile is not None and self.cool > 0:
                self.cool -= 1
                return self.prev_tile
            return (0, 0, frame.shape[1], frame.shape[0])
        if self.prev_tile is not None:
            box = smooth(self.prev_tile, box)
        self.prev_tile, self.cool = box, 10
        return box

    def roi(self, frame):
        l, t, r, b = clamp(self.pick(frame), frame.shape[1], frame.shape[0])
        return frame[t:b, l:r], (l, t, r, b)
