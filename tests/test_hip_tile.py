"""GPU: the speaker-tile choice on the device.  csrc/af_tile.hip and ``TilePicker`` against tests/tile_ref.py - the numpy statement
of LargestTilePicker (test/capture_tile.py:55-109), pinned by tests/test_tile_host.py and unpinned against cv2 itself, absent here -
by ``np.array_equal``: there is no tolerance anywhere.

  sizes       w x h: 8 x 8 (smaller is refused), 37 x 23, one exact 32 x 8 tile, 33 x 9 (a tile + 1 on each axis), the 1-row and
              1-column seams 64 x 9 and 9 x 64, and 70 x 40; tight sources and ones at an odd address with an odd pitch; both byte orders
  stages      random 0..255 frames: g, the class map, the edges, the dilated mask, labels, boxes, external bytes, the survivors'
              records with _valid opened to 1 x 1 through the parameters
  hysteresis  a weak staircase edge across five tile columns and four tile rows whose only strong pixels lie in the first tile
  components  random masks at densities 0.3 / 0.5 / 0.6 and the nesting patterns of the host tests through af_tile_components_u8
  overflow    more than 64 survivors: the flag in the record, an exception from TilePicker
  motion      the same sizes: grey, threshold (differences of 15 .. 18 straddle 16), median, 9 x 9 maximum, union; first frame None
  TilePicker  a 12-frame scripted 640 x 360 sequence (tile found, tile lost -> motion, nothing -> countdown -> full frame) and a
              5-frame one where motion finds a box, for host, CUDA-tensor (bgr and rgb), store-slot and CapturedFrame(bgra, max_w=480)
              inputs; roi's view bytes
Every low-level call checks: error word 0, guard bytes round every output, the workspace and the source untouched; one test runs
every sequence twice and compares the records bit for bit.  Each test first asserts, on the statement alone, that its input
produced the case it is about.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import af_mi355x
import capture_ref as CR
import tile_ref as T
import test_tile_host as TH
from af_mi355x import _lib, evaluator, frames as F

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 256, 0xA5
SIZES = [(8, 8), (23, 37), (8, 32), (9, 33), (9, 64), (64, 9), (40, 70)]       # h, w
OPEN = {"min_w": 1, "min_h": 1, "ar_lo": 0.0, "ar_hi": 1e18, "area_frac": 0.0}
_cache = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """`nbytes` of device memory whose first byte lies at an address = `skew` mod `align`, between two runs of sentinel bytes"""

    def __init__(self, nbytes, align=256, skew=0):
        self.raw = torch.full((nbytes + 2 * GUARD + align,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.start = GUARD + (skew - self.raw.data_ptr() - GUARD) % align
        self.body = self.raw[self.start:self.start + nbytes]
        self.ptr = C.c_void_p(self.body.data_ptr())

    def intact(self):
        return bool((self.raw[:self.start] == SENTINEL).all()) and bool((self.raw[self.start + self.body.numel():] == SENTINEL).all())

    def numpy(self, dtype=np.uint8):
        return self.body.cpu().numpy().view(dtype)


def _params(p, h, w):
    return _lib.TileParams(p["min_w"], p["min_h"], p["ar_lo"], p["ar_hi"], p["area_frac"] * w * h)


def _source(frame, layout):
    """the frame on the device: tight, or from an odd address at an odd pitch -> (Guarded, pitch)"""
    h, w = frame.shape[:2]
    pitch = 3 * w if layout == "tight" else (3 * w + 4) | 1
    buf = Guarded((h - 1) * pitch + 3 * w, 256, 0 if layout == "tight" else 1)
    rows = torch.as_strided(buf.body, (h, 3 * w), (pitch, 1))
    rows.copy_(torch.from_numpy(np.array(frame).reshape(h, 3 * w)).cuda())
    return buf, pitch


class Call:
    """the buffers of one low-level call on an h x w frame and what came back"""
    NAMES = (("g", 1), ("cls", 1), ("edges", 1), ("mask", 1), ("labels", 4), ("boxes", 16), ("external", 1))

    def __init__(self, h, w):
        self.h, self.w, n = h, w, h * w
        need = _lib.lib.af_tile_workspace_bytes(h, w)
        assert need > 0
        self.ws = Guarded(need)
        self.out = {name: Guarded(n * size, 4) for name, size in self.NAMES}
        self.outputs = _lib.TileOutputs(*[self.out[name].ptr for name, _ in self.NAMES])

    def finish(self, what, rc):
        _lib.check(rc, what)
        torch.cuda.synchronize()
        assert self.ws.intact() and all(o.intact() for o in self.out.values()), "%s wrote outside its buffers" % what
        raw = self.ws.numpy()[:C.sizeof(_lib.TileResult)].tobytes()
        self.res = _lib.TileResult.from_buffer_copy(raw)
        assert self.res.error == 0, "%s: error word %d" % (what, self.res.error)
        return raw

    def image(self, name, dtype=np.uint8):
        a = self.out[name].numpy(dtype)
        return a.reshape(self.h, self.w, -1) if name == "boxes" else a.reshape(self.h, self.w)

    def survivors(self):
        return [(b.root, (b.x, b.y, b.w, b.h), b.n_px, b.s1, b.s2) for b in self.res.box[:self.res.count]]


def candidates(frame, order="bgr", layout="tight", params=OPEN):
    h, w = frame.shape[:2]
    call = Call(h, w)
    src, pitch = _source(frame, layout)
    before = src.raw.clone()
    desc = _lib.TileSource(src.ptr, pitch, h, w, int(order == "bgr"), 0)
    p = _params(params, h, w)
    raw = call.finish("tile_candidates_u8", _lib.lib.af_tile_candidates_u8(C.byref(desc), C.byref(p), call.ws.ptr, call.ws.body.numel(),
                                                                          C.byref(call.outputs), _stream()))
    assert torch.equal(src.raw, before)
    return call, raw


def components(mask, g=None, params=OPEN, pitched=False):
    h, w = mask.shape
    call = Call(h, w)
    pitch = w + 3 if pitched else w
    m = Guarded((h - 1) * pitch + w, 1, 0)
    torch.as_strided(m.body, (h, w), (pitch, 1)).copy_(torch.from_numpy(np.ascontiguousarray(mask)).cuda())
    gd = None if g is None else torch.from_numpy(np.ascontiguousarray(g)).cuda()
    p = _params(params, h, w) if params is not None else None
    raw = call.finish("tile_components_u8", _lib.lib.af_tile_components_u8(
        m.ptr, pitch, h, w, None if gd is None else C.c_void_p(gd.data_ptr()), None if p is None else C.byref(p), call.ws.ptr,
        call.ws.body.numel(), C.byref(call.outputs), _stream()))
    return call, raw


def motion(frame, prev_grey, order="bgr", layout="tight"):
    h, w = frame.shape[:2]
    call = Call(h, w)
    src, pitch = _source(frame, layout)
    grey = Guarded(h * w, 1, 0)
    prev = None if prev_grey is None else torch.from_numpy(np.ascontiguousarray(prev_grey)).cuda()
    desc = _lib.TileSource(src.ptr, pitch, h, w, int(order == "bgr"), 0)
    raw = call.finish("tile_motion_u8", _lib.lib.af_tile_motion_u8(C.byref(desc), None if prev is None else C.c_void_p(prev.data_ptr()), grey.ptr,
                                                                  T.MOTION_FRAC * w * h, call.ws.ptr, call.ws.body.numel(), C.byref(call.outputs),
                                                                  _stream()))
    assert grey.intact()
    return call, raw, grey.numpy().reshape(h, w)


def check_components(call, mask, want_survivors=None):
    """labels, boxes, external bytes and the count against the statement's components of `mask`"""
    h, w = mask.shape
    labels, comps = T.components(mask)
    boxes = np.empty((h, w, 4), np.int32)
    boxes[...] = (w, h, -1, -1)
    external = np.zeros((h, w), np.uint8)
    for root, (x, y, bw, bh), ext in comps:
        boxes[root // w, root % w] = (x, y, x + bw - 1, y + bh - 1)
        external[root // w, root % w] = ext
    assert np.array_equal(call.image("mask"), np.where(mask != 0, 255, 0).astype(np.uint8)) or np.array_equal(call.image("mask"), mask)
    assert np.array_equal(call.image("labels", np.int32), labels)
    assert np.array_equal(call.image("boxes", np.int32), boxes)
    assert np.array_equal(call.image("external"), external)
    assert call.res.components == len(comps)
    if want_survivors is not None:
        if len(want_survivors) > _lib.TILE_MAX_BOXES:
            assert call.res.overflow and call.res.count == _lib.TILE_MAX_BOXES
        else:
            assert not call.res.overflow and call.survivors() == want_survivors
    return comps


def _frame(h, w):
    """a random 0..255 frame of this size: the first seed whose statement holds weak and strong candidates in both byte orders (the
    blur leaves an 8 x 8 frame little contrast)"""
    key = ("frame", h, w)
    if key not in _cache:
        for seed in range(200):
            f = np.random.default_rng(100 * h + w + 7919 * seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
            cls = [T.nms_classes(*T.sobel(T.blur(T.grey(f, order)))) for order in ("bgr", "rgb")]
            if all((c == 1).any() and (c == 2).any() for c in cls):
                break
        f.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def _stages(h, w, order):
    key = ("stages", h, w, order)
    if key not in _cache:
        _cache[key] = T.tile_candidates(_frame(h, w), order, OPEN)
    return _cache[key]


def test_small_frames_are_refused():
    assert _lib.lib.af_tile_workspace_bytes(7, 8) == -1 and _lib.lib.af_tile_workspace_bytes(8, 7) == -1
    assert _lib.lib.af_tile_workspace_bytes(8, 8) > 0
    picker = af_mi355x.TilePicker()
    for shape in ((7, 8, 3), (8, 7, 3)):
        with pytest.raises(ValueError):
            picker.tiles(np.zeros(shape, np.uint8))
        with pytest.raises(ValueError):
            picker.motion(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    src = torch.zeros((7, 8, 3), dtype=torch.uint8, device="cuda")
    desc, p = _lib.TileSource(src.data_ptr(), 24, 7, 8, 1, 0), _params(OPEN, 7, 8)
    assert _lib.lib.af_tile_candidates_u8(C.byref(desc), C.byref(p), C.c_void_p(ws.data_ptr()), ws.numel(), None, _stream()) == -1
    assert picker.tiles(np.zeros((8, 8, 3), np.uint8)) is None


@pytest.mark.parametrize("layout", ["tight", "odd"])
@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("h,w", SIZES)
def test_candidate_stages_equal_the_statement(h, w, order, layout):
    survivors, st = _stages(h, w, order)
    assert (st["cls"] == 1).any() and (st["cls"] == 2).any() and (st["edges"] != 0).any()
    call, _ = candidates(_frame(h, w), order, layout)
    assert np.array_equal(call.image("g"), st["g"])
    assert np.array_equal(call.image("cls"), st["cls"])
    assert np.array_equal(call.image("edges"), st["edges"])
    assert np.array_equal(call.image("mask"), st["mask"])
    check_components(call, st["mask"], survivors)


def _staircase():
    """40 x 150: above a staircase that falls one row per five columns the frame is 100, below it 135 - a weak step (m about 87) that
    crosses five tile columns and four tile rows; under its first four columns lies a 4 x 2 patch of 255, the only strong contrast"""
    f = np.empty((40, 150, 3), np.uint8)
    yy, xx = np.mgrid[0:40, 0:150]
    edge = 5 + xx // 5
    below = yy >= edge
    f[...] = np.where(below, 135, 100)[..., None]
    f[below & (xx < 4) & (yy < edge + 2)] = 255
    return f


def test_hysteresis_crosses_tile_seams():
    f = _staircase()
    survivors, st = T.tile_candidates(f, "bgr", OPEN)
    ys, xs = np.nonzero(st["cls"] == 2)
    assert len(ys) and {(y // 8, x // 32) for y, x in zip(ys, xs)} == {(0, 0)}          # every strong pixel lies in the first tile
    ey, ex = np.nonzero(st["edges"])
    assert len({(y // 8, x // 32) for y, x in zip(ey, ex)}) >= 6 and ex.max() >= 140     # ... and the chain reaches the far end
    weak_only = np.minimum(st["cls"], 1)
    assert not T.hysteresis(weak_only).any()                                            # without them there is no edge at all
    call, _ = candidates(f)
    assert np.array_equal(call.image("cls"), st["cls"])
    assert np.array_equal(call.image("edges"), st["edges"])
    check_components(call, st["mask"], survivors)


@pytest.mark.parametrize("density", [0.3, 0.5, 0.6])
@pytest.mark.parametrize("h,w", [(8, 8), (23, 37), (9, 33), (64, 9), (40, 70)])
def test_random_masks_through_the_components_stage(h, w, density):
    rng = np.random.default_rng(int(1000 * density) + 31 * h + w)
    mask = np.where(rng.random((h, w)) < density, 255, 0).astype(np.uint8)
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    want = []
    for root, box, ext in T.components(mask)[1]:
        if ext:
            r = T.roi_of(g, box).astype(np.int64)
            want.append((root, box, int(r.size), int(r.sum()), int((r * r).sum())))
    call, _ = components(mask, g, pitched=(h + w) % 2 == 1)
    check_components(call, mask, want)
    call, _ = components(mask, None, None)                       # no selection: no records
    check_components(call, mask)
    assert call.res.count == 0


def test_nesting_patterns_through_the_components_stage():
    rng = np.random.default_rng(11)
    masks = [(name, m, want) for name, (m, want) in TH.nesting_patterns().items()]
    masks += [("random in ring %d" % k, TH.random_in_ring(rng, 0.5, k % 2 == 1), None) for k in range(4)]
    big = np.zeros((40, 70), np.uint8)                           # the rings again, across tile seams, with a 9 x 9 roi inside
    TH.ring(big[:, :40], 1, 38); TH.ring(big[:, :40], 5, 34); big[10:27, 45:62] = 255; big[17, 20] = 255
    masks.append(("big", big, [((1, 1, 38, 38), True), ((5, 5, 30, 30), False), ((45, 10, 17, 17), True), ((20, 17, 1, 1), False)]))
    for name, m, want in masks:
        g = rng.integers(0, 256, m.shape, dtype=np.uint8)
        comps = T.components(m)[1]
        if want is not None:
            assert [(b, e) for _, b, e in comps] == want, name
        survivors = []
        for root, box, ext in comps:
            if ext:
                r = T.roi_of(g, box).astype(np.int64)
                survivors.append((root, box, int(r.size), int(r.sum()), int((r * r).sum())))
        call, _ = components(m, g)
        check_components(call, m, survivors)
        if name == "big":
            assert [s[2] for s in call.survivors()] == [30 * 30, 9 * 9]


def _dots():
    """64 x 128: a bright 3 x 3 dot every 8 pixels - 128 small closed edge loops"""
    f = np.full((64, 128, 3), 20, np.uint8)
    for y in range(2, 64, 8):
        for x in range(2, 128, 8):
            f[y:y + 3, x:x + 3] = 240
    return f


def test_overflow_is_flagged_and_raises():
    f = _dots()
    survivors, st = T.tile_candidates(f, "bgr", OPEN)
    assert len(survivors) > _lib.TILE_MAX_BOXES
    call, _ = candidates(f)
    check_components(call, st["mask"], survivors)
    assert call.res.overflow and call.res.count == _lib.TILE_MAX_BOXES
    picker = af_mi355x.TilePicker()
    picker.params = dict(OPEN)
    with pytest.raises(_lib.AfError):
        picker.tiles(f)
    picker.params = dict(OPEN, min_w=1000)                       # nothing passes: no overflow, no tile
    assert picker.tiles(f) is None


def _motion_pair(h, w):
    """prev in 0 .. 200 and a frame that differs from it by 0 or by 15 .. 18 grey levels (equal channels: the grey moves by as much)
    inside random blobs"""
    rng = np.random.default_rng(17 * h + w)
    prev = rng.integers(0, 200, (h, w), dtype=np.uint8)
    blobs = T.box_max((rng.random((h, w)) < 0.04).astype(np.uint8), 2) != 0
    delta = np.where(blobs, rng.integers(15, 19, (h, w)), 0) * rng.choice([-1, 1], (h, w))
    cur = np.clip(prev.astype(np.int32) + delta, 0, 255).astype(np.uint8)
    return np.repeat(prev[..., None], 3, 2), np.repeat(cur[..., None], 3, 2)


@pytest.mark.parametrize("layout", ["tight", "odd"])
@pytest.mark.parametrize("h,w", SIZES)
def test_motion_stages_equal_the_statement(h, w, layout):
    a, b = _motion_pair(h, w)
    ga, gb = T.grey(a), T.grey(b)
    diff = np.abs(gb.astype(np.int32) - ga)
    assert (diff == 16).any() and (diff == 17).any()             # the pair straddles the threshold
    th = (diff > 16).astype(np.uint8)
    med = T.median5(th)
    mask = T.box_max(med, 4)
    assert th.any() and not np.array_equal(th, med)
    call, _, grey = motion(b, ga, "bgr", layout)
    assert np.array_equal(grey, gb) and np.array_equal(call.image("g"), gb)
    assert np.array_equal(call.image("cls"), th)
    assert np.array_equal(call.image("edges"), med)
    assert np.array_equal(call.image("mask"), mask * 255)
    check_components(call, mask)
    r = call.res
    assert (r.x1, r.y1, r.x2, r.y2, r.union_count) == T.motion_union(mask)
    first, _, grey = motion(np.ascontiguousarray(b[..., ::-1]), None, "rgb", layout)      # the first frame: the grey alone
    assert np.array_equal(grey, gb) and first.res.union_count == 0 and first.res.components == 0


def test_two_runs_give_identical_records():
    f = _frame(40, 70)
    assert candidates(f)[1] == candidates(f)[1]
    a, b = _motion_pair(40, 70)
    assert motion(b, T.grey(a))[1] == motion(b, T.grey(a))[1]
    mask = np.where(np.random.default_rng(3).random((40, 70)) < 0.5, 255, 0).astype(np.uint8)
    assert components(mask, T.grey(a))[1] == components(mask, T.grey(a))[1]
    assert candidates(_dots())[1][:48] == candidates(_dots())[1][:48]      # overflowed: which 64 arrive first is not fixed, the header is


# ---- TilePicker
def _sequences():
    """name -> 640 x 360 BGR frames"""
    if "seq" not in _cache:
        grid = TH.drawn_grid()
        blank = np.full((360, 640, 3), 30, np.uint8)
        shifted = np.full_like(blank, 30)
        shifted[4:, 6:] = grid[:-4, :-6]

        def block(x):
            f = blank.copy()
            f[100:220, x:x + 200] = 90
            return f

        _cache["seq"] = {"countdown": [grid] + [blank] * 11, "motion": [grid, shifted, blank, block(100), block(140)]}
    return _cache["seq"]


def _statement(name, small):
    """the statement's boxes and roi crops for a sequence; `small`: on the frames CapturedFrame(bgra, max_w=480) stores"""
    key = ("want", name, small)
    if key not in _cache:
        frames = _sequences()[name]
        if small:
            done = {}
            for f in frames:
                if id(f) not in done:
                    done[id(f)] = CR.area_resize(f, 480, 270)
            frames = [done[id(f)] for f in frames]
        p = T.Picker()
        out = []
        for f in frames:
            crop, box = p.roi(f)
            out.append((box, crop.copy(), p.prev_tile, p.cool))
        for f in {id(f): f for f in frames}.values():
            assert all(abs(v - 50) >= 1e-6 for v in T.variances(T.tile_candidates(f)[0]))
        _cache[key] = (frames, out)
    return _cache[key]


def test_the_scripts_produce_their_cases():
    for small, (W, H) in ((False, (640, 360)), (True, (480, 270))):
        _, out = _statement("countdown", small)
        boxes = [o[0] for o in out]
        assert boxes[0] != (0, 0, W, H) and boxes[1:11] == [boxes[0]] * 10 and boxes[11] == (0, 0, W, H)
        assert max(abs(a - b * W // 640) for a, b in zip(boxes[0], (20, 20, 320, 200))) <= 3
        _, out = _statement("motion", small)
        boxes = [o[0] for o in out]
        assert len(set(boxes)) == 4 and boxes[2] == boxes[1] and boxes[1] != boxes[0]      # smoothed, held, then two motion boxes
        assert [o[3] for o in out] == [10, 10, 9, 10, 10]


KINDS = ["host", "tensor", "tensor-rgb", "slot", "captured"]


def _feed(kind, frame, store, k):
    if kind == "host":
        return frame
    if kind == "tensor":
        return torch.from_numpy(frame).cuda()
    if kind == "tensor-rgb":
        return torch.from_numpy(np.ascontiguousarray(frame[..., ::-1])).cuda()
    if kind == "slot":
        store.put([frame], k % 2)
        return (store, k % 2)
    bgra = np.concatenate([frame, np.full(frame.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return F.CapturedFrame(bgra, "bgra", max_w=480)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["countdown", "motion"])
def test_picker_equals_the_statement(name, kind):
    small = kind == "captured"
    frames, want = _statement(name, small)
    picker = af_mi355x.TilePicker(channel_order="rgb" if kind == "tensor-rgb" else "bgr")
    store = evaluator.FrameStore(picker.device, "bgr")
    store.open((360, 640, 3), 2)
    for k, (f, (box, crop, prev_tile, cool)) in enumerate(zip(_sequences()[name], want)):
        view, got = picker.roi(_feed(kind, f, store, k))
        assert got == box and picker.prev_tile == prev_tile and picker.cool == cool, (k, got, box)
        got_crop = view.cpu().numpy()
        assert np.array_equal(got_crop[..., ::-1] if kind == "tensor-rgb" else got_crop, crop), k
    assert picker.readbacks <= 2 * len(want)
    picker.reset()
    assert picker.prev_tile is None and picker.cool == 0
    assert picker.motion(_feed(kind, _sequences()[name][0], store, 0)) is None           # the first frame after a reset


def test_pick_tiles_and_motion_are_the_statements():
    frames, _ = _statement("motion", False)
    picker, ref = af_mi355x.TilePicker(), T.Picker()
    assert ref.tiles(frames[0]) is not None and picker.tiles(frames[0]) == ref.tiles(frames[0])
    assert picker.tiles(frames[2]) is None
    for f in frames[2:]:
        assert picker.motion(f) == ref.motion(f)
    assert ref.prev_tile is None and picker.prev_tile is None
    assert picker.pick(frames[0]) == ref.pick(frames[0])
