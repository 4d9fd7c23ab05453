"""CPU: tests/tile_ref.py - the numpy statement of LargestTilePicker (test/capture_tile.py:55-109) that csrc/af_tile.hip and
TilePicker are checked against - pinned by hand-worked cases.  OpenCV is absent here, so these anchors, worked from OpenCV 4.x's
sources, are what ties the statement down: unpinned vs cv2 itself.

  blur      one pixel of 32 in zeros: 36 * 32 = 4.5 * 256 rounds UP to 5 ((S + 128) >> 8); 24 * 32 -> 3, 6 * 32 -> 1 (0.75), 1 * 32 -> 0;
            BORDER_REFLECT_101: the pixel at (1, 1) is seen twice from row -1 and column -1, so g[0, 0] = (4 + 4)^2 * 32 >> 8 = 8
  NMS       one case per branch on hand-made dx, dy: the tie that > (left, up) / >= (right, down) decides, both diagonals (strict on
            both sides), the branch boundaries at tan 22.5 (dy 41 | 42 at dx 100) and tan 67.5 (dy 241 | 242), m = 50 | 51, 150 | 151
  contours  the component / nesting rule against a tiny pure-Python flood fill on masks up to 12 x 12: a ring in a ring in a ring
            (touching the border and not), a diagonal-only closed loop (it encloses: the background is 4-connected), a component on
            the border, random masks
  motion    a 20 x 20 block that differs by 16 (nothing) and by 17 (the worked box), the median's corner arithmetic
  pick      smoothing, the countdown to the full frame, prev_gray replaced only on the motion path
  grid      a drawn 640 x 360 grid: two textured tiles, a flat one, a narrow one -> the larger textured tile within 3 px
"""
import numpy as np

import tile_ref as T


def test_blur_rounding_and_reflect101():
    g = np.zeros((9, 9), np.uint8)
    g[4, 4] = 32
    b = T.blur(g)
    assert b[4, 4] == 5                                        # 36 * 32 = 1152 = 4.5 * 256: half rounds up
    assert b[4, 5] == b[5, 4] == 3 and b[5, 5] == 2            # 24 * 32 = 768, 16 * 32 = 512: exact
    assert b[4, 6] == 1 and b[6, 6] == 0                       # 6 * 32 = 192 -> 0.75 -> 1;  1 * 32 = 32 -> 0.125 -> 0
    assert b[5, 6] == b[6, 5] == 1                             # 4 * 32 = 128 = 0.5 * 256: half rounds up again
    assert b[4, 7] == 0 and b.sum() == 5 + 4 * 3 + 4 * 2 + 4 * 1 + 8 * 1
    g = np.zeros((8, 8), np.uint8)
    g[1, 1] = 32
    b = T.blur(g)
    assert b[0, 0] == 8                                        # rows 2 1 0 1 2: row 1 twice, 4 + 4, and so the columns: 64 * 32 >> 8
    assert b[1, 1] == 6                                        # rows 1 0 1 2 3: row 1 at 1 + 6 = 7, columns too: 49 * 32 = 6.125 * 256
    assert b[0, 1] == 7                                        # 8 * 7 * 32 = 7 * 256
    g = np.zeros((8, 8), np.uint8)
    g[7, 7] = 32                                               # the far corner: rows 5 6 7 6 5, the corner once, weight 6
    assert T.blur(g)[7, 7] == 5 and T.blur(g)[6, 6] == (16 * 32 + 128) >> 8 == 2
    flat = np.full((8, 11), 201, np.uint8)
    assert np.array_equal(T.blur(flat), flat)                  # the taps sum to 256


def test_grey_is_the_15_bit_formula_in_both_orders():
    px = np.array([[[10, 200, 30]]], np.uint8)                 # B, G, R
    want = (30 * 9798 + 200 * 19235 + 10 * 3735 + 16384) >> 15
    assert T.grey(px, "bgr")[0, 0] == want == 128              # 4194674 >> 15
    assert T.grey(px[..., ::-1], "rgb")[0, 0] == want


def test_sobel_replicates_the_border():
    g = np.array([[0, 10, 20], [0, 10, 20], [0, 10, 20]], np.uint8)
    dx, dy = T.sobel(g)
    assert dx[1, 1] == 4 * 20 and dx[1, 0] == 4 * 10 and dx[0, 0] == 40 and not dy.any()
    dx, dy = T.sobel(g.T.copy())
    assert dy[1, 1] == 80 and dy[0, 1] == 40 and not dx.any()  # dy = the row below minus the row above


def _cls(dx_rows, dy_rows):
    return T.nms_classes(np.array(dx_rows, np.int32), np.array(dy_rows, np.int32))


def test_nms_one_case_per_branch():
    z = [0, 0, 0, 0]
    # horizontal (dy = 0): m = 60 100 100 60.  x = 0: 60 >= 100 fails; x = 1: 100 > 60 and 100 >= 100 keeps; x = 2: 100 > 100 fails -
    # the tie that > / >= decides; x = 3: 60 > 100 fails
    assert _cls([z, [60, 100, 100, 60], z], [z, z, z]).tolist() == [z, [0, 1, 0, 0], z]
    assert _cls([[60, 100, 100, 60]], [z]).tolist() == [[0, 1, 0, 0]]
    # vertical (dx = 0): the same column-wise: up strict, down >=
    col = _cls([[0], [0], [0], [0]], [[60], [100], [100], [60]])
    assert col[:, 0].tolist() == [0, 1, 0, 0]
    # diagonal, dx and dy of equal sign: neighbours (x-1, y-1) and (x+1, y+1), both strict
    e = [0, 0, 0]
    assert _cls([[39, 0, 0], [0, 40, 0], e], [[40, 0, 0], [0, 40, 0], e])[1, 1] == 1           # 80 > 79 and 80 > 0
    assert _cls([[40, 0, 0], [0, 40, 0], e], [[40, 0, 0], [0, 40, 0], e])[1, 1] == 0           # 80 > 80 fails
    assert _cls([e, [0, 40, 0], [0, 0, 40]], [e, [0, 40, 0], [0, 0, 40]])[1, 1] == 0           # ... on the other side too
    assert _cls([[0, 0, 40], [0, 40, 0], e], [[0, 0, 40], [0, 40, 0], e])[1, 1] == 1           # the other diagonal is not asked
    # ... of opposite sign: (x+1, y-1) and (x-1, y+1)
    assert _cls([[0, 0, 40], [0, 40, 0], e], [[0, 0, -40], [0, -40, 0], e])[1, 1] == 0
    assert _cls([[40, 0, 0], [0, 40, 0], e], [[-40, 0, 0], [0, -40, 0], e])[1, 1] == 1
    assert _cls([e, [0, -40, 0], [-40, 0, 0]], [e, [0, 40, 0], [40, 0, 0]])[1, 1] == 0


def test_nms_branch_boundaries_and_thresholds():
    # tan 22.5 deg * 100 = 41.42: dy = 41 is horizontal (the right neighbour of equal m is tolerated), dy = 42 is diagonal (it is not asked)
    assert (41 << 15) < 100 * T.TG22 <= (42 << 15)
    assert _cls([[100, 100]], [[41, 41]]).tolist() == [[1, 0]]                                 # horizontal: 141 > 0, >= 141 | 141 > 141 fails
    assert _cls([[100, 100]], [[42, 42]]).tolist() == [[1, 1]]                                 # diagonal: the row above and below are outside: 0
    # tan 67.5 deg * 100 = 241.4: dy = 241 diagonal, 242 vertical
    assert (241 << 15) <= 100 * T.TG22 + (100 << 16) < (242 << 15)
    assert _cls([[100], [100]], [[242], [242]])[:, 0].tolist() == [2, 0]                       # vertical: the tie below fails the lower one
    assert _cls([[100], [100]], [[241], [241]])[:, 0].tolist() == [2, 2]                       # diagonal: the neighbours are outside
    assert T.TG22 == int(0.4142135623730950488016887242097 * (1 << 15) + 0.5)
    for m, want in ((50, 0), (51, 1), (150, 1), (151, 2)):
        assert _cls([[m]], [[0]])[0, 0] == want


def test_hysteresis_is_connectivity_to_a_strong_candidate():
    cls = np.array([[1, 0, 0, 0, 1, 1],
                    [0, 1, 0, 0, 0, 0],
                    [0, 0, 2, 0, 0, 1],
                    [0, 0, 0, 0, 0, 1]], np.uint8)
    want = np.array([[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]], np.uint8) * 255
    assert np.array_equal(T.hysteresis(cls), want)             # the diagonal chain reaches the strong pixel; the two others do not


# ---- the component and nesting rule against a flood fill
def _flood(mask):
    """pure Python: [(root, (x, y, w, h), external)] by the rule's words - 8-connected set pixels; kept when 4-adjacent to background
    that is 4-connected to the one-pixel pad round the image"""
    h, w = len(mask), len(mask[0])
    pad = [[0] * (w + 2)] + [[0] + [1 if v else 0 for v in row] + [0] for row in mask] + [[0] * (w + 2)]
    outer, todo = {(0, 0)}, [(0, 0)]
    while todo:
        y, x = todo.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < h + 2 and 0 <= xx < w + 2 and not pad[yy][xx] and (yy, xx) not in outer:
                outer.add((yy, xx))
                todo.append((yy, xx))
    seen, out = set(), []
    for y0 in range(h):
        for x0 in range(w):
            if not mask[y0][x0] or (y0, x0) in seen:
                continue
            comp, todo = {(y0, x0)}, [(y0, x0)]
            while todo:
                y, x = todo.pop()
                for yy in (y - 1, y, y + 1):
                    for xx in (x - 1, x, x + 1):
                        if 0 <= yy < h and 0 <= xx < w and mask[yy][xx] and (yy, xx) not in comp:
                            comp.add((yy, xx))
                            todo.append((yy, xx))
            seen |= comp
            ys, xs = [p[0] for p in comp], [p[1] for p in comp]
            ext = any((y + 1 + dy, x + 1 + dx) in outer for y, x in comp for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))
            out.append((y0 * w + x0, (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1), ext))
    return sorted(out)


def ring(mask, lo, hi):
    mask[lo, lo:hi + 1] = mask[hi, lo:hi + 1] = mask[lo:hi + 1, lo] = mask[lo:hi + 1, hi] = 255


def nesting_patterns():
    """name -> (mask, [(box, external)] by ascending root): the hand-stated expectations, shared with the GPU tests"""
    out = {}
    m = np.zeros((12, 12), np.uint8)
    ring(m, 0, 11); ring(m, 2, 9); ring(m, 4, 7)
    out["rings on the border"] = (m, [((0, 0, 12, 12), True), ((2, 2, 8, 8), False), ((4, 4, 4, 4), False)])
    m = np.zeros((12, 12), np.uint8)
    ring(m, 1, 10); ring(m, 3, 8); m[5:7, 5:7] = 255
    out["rings inside"] = (m, [((1, 1, 10, 10), True), ((3, 3, 6, 6), False), ((5, 5, 2, 2), False)])
    m = np.zeros((11, 11), np.uint8)
    for y in range(11):
        for x in range(11):
            if abs(y - 5) + abs(x - 5) == 4:
                m[y, x] = 255                                  # a diamond: consecutive pixels touch only by their corners
    m[5, 5] = 255
    out["diagonal loop"] = (m, [((1, 1, 9, 9), True), ((5, 5, 1, 1), False)])
    m = np.zeros((9, 12), np.uint8)
    m[3:6, 0] = 255; m[8, 4:7] = 255; m[2, 5] = 255
    out["on the border"] = (m, [((5, 2, 1, 1), True), ((0, 3, 1, 3), True), ((4, 8, 3, 1), True)])
    m = np.zeros((10, 10), np.uint8)
    ring(m, 1, 8); m[1, 4] = 0; m[4:6, 4:6] = 255              # a gap of one pixel opens the ring: its inside reaches the border
    out["open ring"] = (m, [((1, 1, 8, 8), True), ((4, 4, 2, 2), True)])
    return out


def random_in_ring(rng, density, knock_out):
    """12 x 12: random 6 x 6 content, a clear gap, a ring of set pixels, a clear margin; `knock_out`: one ring pixel (not a corner)
    cleared, which lets the outer background in"""
    inner = (rng.random((6, 6)) < density).astype(np.uint8)
    mask = np.pad(np.pad(np.pad(inner, 1), 1, constant_values=1), 1)
    if knock_out:
        mask[1, int(rng.integers(3, 9))] = 0
    return mask


def test_components_and_nesting_against_the_flood_fill():
    for name, (mask, want) in nesting_patterns().items():
        labels, comps = T.components(mask)
        assert comps == _flood(mask.tolist()), name
        assert [(b, e) for _, b, e in comps] == want, name
        assert T.external_boxes(mask) == [b for b, e in want if e], name
        for root, (x, y, w, h), _ in comps:
            assert labels[root // mask.shape[1], root % mask.shape[1]] == root and (labels == root).sum() >= 1
            assert root == np.flatnonzero(labels.reshape(-1) == root)[0]
        assert ((labels >= 0) == (mask != 0)).all()
    rng = np.random.default_rng(5)
    enclosed = 0
    for k in range(120):
        h, w = rng.integers(1, 13, 2)
        mask = (rng.random((h, w)) < (0.3, 0.5, 0.6, 0.8)[k % 4]).astype(np.uint8)
        assert T.components(mask)[1] == _flood(mask.tolist()), mask
    opened = 0
    for k in range(40):                                        # random 6 x 6 content in a ring; every other ring has one pixel knocked out
        mask = random_in_ring(rng, (0.3, 0.5, 0.6)[k % 3], k % 2 == 1)
        comps = T.components(mask)[1]
        assert comps == _flood(mask.tolist()), mask
        inner = [e for r, _, e in comps if r != comps[0][0]]
        enclosed += sum(not e for e in inner)
        opened += sum(inner) if k % 2 else 0
    assert enclosed >= 20 and opened >= 10                     # the closed rings enclose, the opened ones let the background in


def test_box_max_stays_inside_the_image():
    m = np.zeros((6, 7), np.uint8)
    m[0, 0] = m[5, 3] = 255
    d = T.box_max(m, 1)
    want = np.zeros((6, 7), np.uint8)
    want[0:2, 0:2] = 255; want[4:6, 2:5] = 255
    assert np.array_equal(d, want)
    assert np.array_equal(T.box_max(m, 4), T.box_max(T.box_max(T.box_max(T.box_max(m, 1), 1), 1), 1))


# ---- motion
def _block_pair(delta):
    a = np.full((40, 40, 3), 100, np.uint8)
    b = a.copy()
    b[10:30, 10:30] = 100 + delta                              # equal channels: grey = the value
    return a, b


def test_motion_threshold_median_and_fit():
    a, b = _block_pair(17)
    th = (np.abs(T.grey(b).astype(int) - T.grey(a)) > 16).astype(np.uint8)
    med = T.median5(th)
    assert th.sum() == 400 and med.sum() == 400 - 4 * 3        # per corner (10,10): 9, (10,11) and (11,10): 12 of 25 < 13; (10,12): 15, (11,11): 16
    assert not med[10, 10] and not med[10, 11] and not med[11, 10] and med[10, 12] and med[11, 11]
    edge = np.zeros((8, 8), np.uint8)
    edge[:, :2] = 1                                            # BORDER_REPLICATE: column 0 counts three times at x = 0: 5 * 4 = 20 of 25
    assert T.median5(edge)[:, 0].all() and T.median5(edge)[:, 1].all() and not T.median5(edge)[:, 2].any()      # x = 2: 5 * 2 = 10 < 13
    mask = T.motion_mask(T.grey(b), T.grey(a))
    assert T.motion_union(mask) == (6, 6, 34, 34, 1)           # rows / columns 10..29 survive the median, 9 x 9 maximum: 6..33
    assert T.fit_16_9(6, 6, 34, 34, 40, 40) == (0, 6, 40, 34)  # nw = int(28 * 16 / 9) = 49, cx = 20, x1 = max(0, 20 - 24), x2 = min(40, 49)
    assert T.fit_16_9(0, 10, 40, 20, 40, 40) == (0, 4, 40, 26)  # wider than 16:9: nh = int(40 / (16 / 9)) = 22, cy = 15, y1 = 4
    assert T.fit_16_9(40, 40, 0, 0, 40, 40) is None
    p = T.Picker(tiles_fn=lambda f: None)
    assert p.pick(a) == (0, 0, 40, 40) and p.motion_runs == 1  # the first frame: prev_gray is taken, nothing found, no previous tile
    assert p.pick(b) == (0, 6, 40, 34)
    q = T.Picker(tiles_fn=lambda f: None)
    a16, b16 = _block_pair(16)                                 # |diff| = 16 is not > 16
    assert q.pick(a16) == (0, 0, 40, 40) and q.pick(b16) == (0, 0, 40, 40) and q.prev_tile is None
    small = np.zeros((40, 40), np.uint8)
    small[5:8, 5:9] = 255                                      # w * h = 12 < 0.01 * 1600 = 16: not counted
    assert T.motion_union(small) == (40, 40, 0, 0, 0)
    small[5:9, 5:9] = 255                                      # 16 >= 16.0: counted
    assert T.motion_union(small) == (5, 5, 9, 9, 1)


# ---- the state machine
def test_pick_smoothing_countdown_and_prev_gray():
    script = [(100, 50, 500, 300), (105, 51, 505, 301), None]
    frames = [np.full((360, 640, 3), v, np.uint8) for v in (10, 20, 30)]
    calls = []
    p = T.Picker(tiles_fn=lambda f: (calls.append(1), script[min(len(calls) - 1, 2)])[1])
    assert p.pick(frames[0]) == (100, 50, 500, 300) and p.cool == 10 and p.prev_gray is None and p.motion_runs == 0
    # 0.6 * 100 + 0.4 * 105 = 102.0; 0.6 * 50 + 0.4 * 51 = 50.4 -> 50; 0.6 * 500 + 0.4 * 505 = 502.0; 0.6 * 300 + 0.4 * 301 = 300.4 -> 300
    assert p.pick(frames[1]) == (102, 50, 502, 300) and p.prev_gray is None and p.motion_runs == 0
    # tiles gives nothing: _motion runs, takes its first prev_gray, finds nothing; the countdown hands the last tile out ten times
    assert p.pick(frames[2]) == (102, 50, 502, 300) and p.cool == 9 and p.motion_runs == 1
    assert np.array_equal(p.prev_gray, np.full((360, 640), 30, np.uint8))
    for k in range(9):
        assert p.pick(frames[2]) == (102, 50, 502, 300) and p.cool == 8 - k
    assert p.pick(frames[2]) == (0, 0, 640, 360) and p.cool == 0 and p.prev_tile == (102, 50, 502, 300)
    # a tile again: smoothed against the tile of long ago, and prev_gray is NOT replaced on this path
    calls.clear()
    before = p.prev_gray
    runs = p.motion_runs
    assert p.pick(frames[0]) == (int(0.6 * 102 + 0.4 * 100), 50, int(0.6 * 502 + 0.4 * 500), 300) == (101, 50, 501, 300)
    assert p.prev_gray is before and p.motion_runs == runs and p.cool == 10
    assert T.clamp((-5, 400, 700, 380), 640, 360) == (0, 359, 640, 360)
    assert T.clamp((639, 10, 639, 5), 640, 360) == (639, 10, 640, 11)
    view, box = T.Picker(tiles_fn=lambda f: (10, 20, 700, 30)).roi(frames[0])
    assert box == (10, 20, 640, 30) and view.shape == (10, 630, 3)


def test_the_binding_matches_the_header_and_refuses_without_a_gpu():
    import ctypes as C
    from af_mi355x import _lib
    assert C.sizeof(_lib.TileSource) == 32 and C.sizeof(_lib.TileParams) == 32 and C.sizeof(_lib.TileBox) == 40
    assert C.sizeof(_lib.TileResult) == 48 + 40 * _lib.TILE_MAX_BOXES and C.sizeof(_lib.TileOutputs) == 7 * 8
    n = 23 * 37
    pad = lambda v: (v + 255) & ~255                           # noqa: E731
    assert _lib.lib.af_tile_workspace_bytes(23, 37) == 4096 + pad(4 * n) + pad(16 * n) + 6 * pad(n)
    assert _lib.lib.af_tile_workspace_bytes(7, 8) == -1 and _lib.lib.af_tile_workspace_bytes(8, 8193) == -1
    p = _lib.TileParams(1, 1, 0.0, 1e18, 0.0)
    small = _lib.TileSource(1 << 20, 24, 7, 8, 1, 0)           # refused before the pointer is looked at
    assert _lib.lib.af_tile_candidates_u8(C.byref(small), C.byref(p), C.c_void_p(1 << 20), 1 << 30, None, None) == -1
    assert b"both sides 8 to 8192" in _lib.lib.af_last_error()
    ok = _lib.TileSource(1 << 20, 24, 8, 8, 1, 0)
    assert _lib.lib.af_tile_candidates_u8(C.byref(ok), C.byref(p), C.c_void_p(1 << 20), 100, None, None) == -1
    assert b"workspace of 100 bytes" in _lib.lib.af_last_error()
    assert _lib.lib.af_tile_candidates_u8(C.byref(ok), C.byref(p), C.c_void_p((1 << 20) + 8), 1 << 30, None, None) == -1
    assert _lib.lib.af_tile_motion_u8(C.byref(ok), None, None, 0.0, C.c_void_p(1 << 20), 1 << 30, None, None) == -1
    assert _lib.lib.af_tile_components_u8(None, 8, 8, 8, None, None, C.c_void_p(1 << 20), 1 << 30, None, None) == -1
    thin = _lib.TileSource(1 << 20, 23, 8, 8, 1, 0)            # a pitch below the row
    assert _lib.lib.af_tile_candidates_u8(C.byref(thin), C.byref(p), C.c_void_p(1 << 20), 1 << 30, None, None) == -1


# ---- the drawn grid
def drawn_grid():
    """640 x 360, BGR: tile A 300 x 180 at (20, 20) and tile B 240 x 150 at (360, 30), both a left-to-right ramp (their left edge is a
    weak step of 30 that only hysteresis keeps) under a slow vertical wave; a flat tile 260 x 140 at (20, 210); a narrow one
    100 x 130 at (400, 200)"""
    f = np.full((360, 640, 3), 30, np.uint8)

    def textured(x, y, w, h):
        ramp = np.linspace(60, 220, w)[None, :] + 12 * np.sin(np.arange(h) / 9.0)[:, None]
        f[y:y + h, x:x + w] = np.clip(ramp, 0, 255).astype(np.uint8)[..., None]

    textured(20, 20, 300, 180)
    textured(360, 30, 240, 150)
    f[210:350, 20:280] = 120
    f[200:330, 400:500] = (90, 160, 200)
    return f


def test_drawn_grid_picks_the_larger_textured_tile():
    f = drawn_grid()
    survivors, stages = T.tile_candidates(f)
    boxes = {b for _, b, _, _, _ in survivors}
    assert len(survivors) == 3                                 # A, B and the flat tile pass _valid; the narrow one does not
    assert not any(abs(x - 400) <= 3 and abs(y - 200) <= 3 for x, y, _, _ in boxes)
    var = T.variances(survivors)
    assert all(abs(v - 50) >= 1e-6 for v in var) and sorted(v < 50 for v in var) == [False, False, True]
    got = T.tiles(f)
    assert max(abs(a - b) for a, b in zip(got, (20, 20, 320, 200))) <= 3, got
    assert (stages["cls"] == 1).any() and (stages["cls"] == 2).any()
    assert T.Picker().pick(f) == got
