"""GPU: the three launches live.CallServer shares between calls, each against the existing single-store launch it restates.

  yunet    af_yunet_detect_frames (YuNet.detect_views) on three 96 x 131 frames in three separate allocations, one of them a view
           into the middle of a larger ring: counts, rows up to each count and the raw head outputs are torch.equal to
           YuNet.detect on the stacked copy, for B = 1 and B = 3, at conf 0.05
  warp     af_warp_affine_window_stores_u8 over store 0 (96 x 131, B, G, R) and store 1 (80 x 112, R, G, B): window 0 out of store
           1, windows 1 and 2 out of store 0, one rectangle ending on the last pixel of its store's last frame; every window's
           bytes equal the single-store launch of that store's form; the same with the stores' order exchanged; a table of
           another form writes nothing
  quality  af_face_quality_stores_u8 (live.StoresQuality) on rectangles interleaved over the two stores: sums and grey bytes equal
           af_face_quality_u8 per store (live.FaceQuality), and the same in reversed order
"""
import ctypes as C

import numpy as np
import pytest
import torch

from af_mi355x import _lib, evaluator, frames, live
from test_hip_yunet import MODEL, frames as yunet_frames

pytestmark = pytest.mark.gpu
SHAPES = ((96, 131), (80, 112))                                   # store 0: row pitch 393 bytes; store 1: 336
ORDERS = ("bgr", "rgb")
N_FRAMES = (5, 4)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


# ---- YuNet on a list of frames -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def yunet():
    from af_mi355x.detector import YuNet
    return YuNet(MODEL, confThreshold=0.05)


@pytest.fixture(scope="module")
def scattered():
    """three frames in three allocations - the second one slot 2 of a ring of 5, the third behind an odd offset - and their stack"""
    h, w = SHAPES[0]
    fr = yunet_frames(3, w, h, seed=23)                           # frame 0 holds a detection of score 0.09 (fp64 graph)
    dev = _dev()
    ring = torch.zeros(5, h, w, 3, dtype=torch.uint8, device=dev)
    ring[2] = torch.from_numpy(fr[1]).to(dev)
    odd = torch.zeros(h * w * 3 + 7, dtype=torch.uint8, device=dev)
    odd[7:] = torch.from_numpy(fr[2]).to(dev).reshape(-1)
    views = [torch.from_numpy(fr[0]).to(dev), ring[2], odd[7:].view(h, w, 3)]
    assert len({v.untyped_storage().data_ptr() for v in views}) == 3 and views[2].data_ptr() % 2 == 1
    return views, torch.from_numpy(fr).to(dev)


@pytest.mark.parametrize("batch", [1, 3])
def test_detect_views_equals_detect_on_the_stacked_copy(yunet, scattered, batch):
    views, stacked = scattered
    rows, counts, raw = yunet.detect_views(views[:batch], raw=True)
    wrows, wcounts, wraw = yunet.detect(stacked[:batch], raw=True)
    assert torch.equal(counts, wcounts) and torch.equal(raw, wraw)
    for b in range(batch):
        n = int(counts[b])
        assert torch.equal(rows[b, :n], wrows[b, :n]), b
    print("detect_views B = %d: counts %s" % (batch, counts.tolist()))
    assert int(counts.sum()) >= 1
    if batch == 3:
        assert len(yunet.detect_views(views)) == 2                # without raw: (rows, counts)


def test_detect_views_refuses_what_one_launch_cannot_take(yunet, scattered):
    views, _ = scattered
    with pytest.raises(ValueError):
        yunet.detect_views([])
    with pytest.raises(ValueError):
        yunet.detect_views(views[:1] * 65)
    with pytest.raises(ValueError):
        yunet.detect_views([views[0], views[1][:80]])             # two shapes
    with pytest.raises(RuntimeError):
        yunet.detect_views([views[0].cpu()])


# ---- the two stores ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stores():
    rng = np.random.default_rng(21)
    out = []
    for (h, w), n in zip(SHAPES, N_FRAMES):
        store = evaluator.FrameStore(_dev())
        store.open((h, w, 3), n)
        store.put([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)], 0)
        out.append(store)
    return out


def _refs(stores, order):
    return (_lib.StoreRef * 2)(*[frames.store_ref(stores[i], ORDERS[i]) for i in order])


# ---- the warp ----------------------------------------------------------------------------------------------------------------------

CLIP, SIZE = 8, 64
WINDOW_STORE = (1, 0, 0)


def _windows():
    """three windows of 8 rectangles: descriptors, and rectangles with the window's store in `reserved`.  Rectangle (0, 7) ends on
    the last pixel of the last frame of store 1, rectangle (2, 3) on that of store 0; the frame numbers 0..3 occur in both stores"""
    rng = np.random.default_rng(22)
    desc = np.zeros(3, dtype=evaluator._WINDOW_DTYPE)
    rects = np.zeros((3, CLIP), dtype=evaluator._RECT_DTYPE)
    for w, s in enumerate(WINDOW_STORE):
        (h, wd), n = SHAPES[s], N_FRAMES[s]
        ch, cw = int(rng.integers(70, 90)), int(rng.integers(80, 100))
        ang, sc = rng.uniform(-0.4, 0.4), SIZE / 70.0 * rng.uniform(0.8, 1.3)
        a, b = sc * np.cos(ang), sc * np.sin(ang)
        desc[w] = ([a, -b, rng.uniform(-10, 15), b, a, rng.uniform(-10, 15)], ch, cw)
        for t in range(CLIP):
            iw, ih = int(rng.integers(30, 70)), int(rng.integers(30, 60))
            rx, ry, f = int(rng.integers(0, wd - iw + 1)), int(rng.integers(0, h - ih + 1)), (w + t) % 4
            if (w, t) in ((0, 7), (2, 3)):
                rx, ry, f = wd - iw, h - ih, n - 1
            rects[w, t] = (f, rx, ry, ih, iw, int(rng.integers(0, cw - iw + 1)), int(rng.integers(0, ch - ih + 1)), s)
    return desc, rects


def _single(stores, desc, rects, s):
    """the windows of store `s` through the existing single-store planner and the launch of that store's byte order"""
    mine = [w for w, ws in enumerate(WINDOW_STORE) if ws == s]
    d, r = np.ascontiguousarray(desc[mine]), np.ascontiguousarray(rects[mine])
    r["reserved"] = 0
    table = np.zeros(_lib.lib.af_window_rects_table_bytes(len(mine), CLIP) // 8, dtype=np.int64)
    _lib.check(_lib.lib.af_window_rects_plan_u8(d.ctypes.data, r.ctypes.data, len(mine), CLIP, SIZE, stores[s].plan_source(), table.ctypes.data,
                                                table.nbytes, None, None), "plan")
    out = torch.zeros((len(mine), CLIP, SIZE, SIZE, 3), dtype=torch.uint8, device=_dev())
    fn = "af_warp_affine_window_rects_bgr_u8" if ORDERS[s] == "bgr" else "af_warp_affine_window_rects_u8"
    table = torch.from_numpy(table).to(_dev())
    _lib.check(getattr(_lib.lib, fn)(C.c_void_p(stores[s].dev.data_ptr()), C.c_void_p(table.data_ptr()), len(mine),
                                     CLIP, SIZE, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), fn)
    torch.cuda.synchronize()
    return dict(zip(mine, out))


def _several(stores, desc, rects, order):
    r = rects.copy()
    r["reserved"] = [[order.index(s)] * CLIP for s in WINDOW_STORE]
    table = np.zeros(_lib.lib.af_window_rects_table_bytes(3, CLIP) // 8, dtype=np.int64)
    bw, bf = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib.af_window_rects_plan_stores_u8(desc.ctypes.data, r.ctypes.data, 3, CLIP, SIZE, _refs(stores, order), 2, table.ctypes.data,
                                                 table.nbytes, C.byref(bw), C.byref(bf))
    assert rc == 0 and (bw.value, bf.value) == (-1, -1), _lib.lib.af_last_error()
    table = torch.from_numpy(table).to(_dev())
    out = torch.full((3, CLIP, SIZE, SIZE, 3), 7, dtype=torch.uint8, device=_dev())
    _lib.check(_lib.lib.af_warp_affine_window_stores_u8(C.c_void_p(table.data_ptr()), 3, CLIP, SIZE, C.c_void_p(out.data_ptr()),
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "stores warp")
    torch.cuda.synchronize()
    return out, table


@pytest.fixture(scope="module")
def warped_alone(stores):
    desc, rects = _windows()
    want = {}
    for s in (0, 1):
        want.update(_single(stores, desc, rects, s))
    assert sorted(want) == [0, 1, 2] and all(bool(v.any()) for v in want.values())
    return desc, rects, want


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_windows_out_of_two_stores_equal_the_single_store_launches(stores, warped_alone, order):
    desc, rects, want = warped_alone
    (h0, w0), (h1, w1) = SHAPES
    assert tuple(rects[0, 7][["frame", "rx", "ry"]]) == (N_FRAMES[1] - 1, w1 - rects[0, 7]["iw"], h1 - rects[0, 7]["ih"])
    assert tuple(rects[2, 3][["frame", "rx", "ry"]]) == (N_FRAMES[0] - 1, w0 - rects[2, 3]["iw"], h0 - rects[2, 3]["ih"])
    got, table = _several(stores, desc, rects, list(order))
    for w in range(3):
        assert torch.equal(got[w], want[w]), (w, int((got[w] != want[w]).sum()))
    # a table of this form is no table for the single-store launch, and the other way round: nothing is written
    out = torch.full((3, CLIP, SIZE, SIZE, 3), 9, dtype=torch.uint8, device=_dev())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.af_warp_affine_window_rects_u8(C.c_void_p(stores[0].dev.data_ptr()), C.c_void_p(table.data_ptr()), 3, CLIP, SIZE,
                                                       C.c_void_p(out.data_ptr()), stream), "rects")
    single = np.zeros(table.numel(), dtype=np.int64)
    r = rects.copy()
    r["frame"], r["rx"], r["ry"], r["reserved"] = 0, 0, 0, 0
    _lib.check(_lib.lib.af_window_rects_plan_u8(desc.ctypes.data, r.ctypes.data, 3, CLIP, SIZE, stores[0].plan_source(), single.ctypes.data,
                                                single.nbytes, None, None), "plan")
    single = torch.from_numpy(single).to(_dev())
    _lib.check(_lib.lib.af_warp_affine_window_stores_u8(C.c_void_p(single.data_ptr()), 3, CLIP, SIZE, C.c_void_p(out.data_ptr()), stream), "stores")
    torch.cuda.synchronize()
    assert bool((out == 9).all())


def test_stores_warp_class_gives_the_same_bytes(stores, warped_alone):
    """live.StoresWarp, the caller CallServer uses: the same three windows from track records"""
    desc, rects, want = warped_alone
    warp = live.StoresWarp(_dev(), CLIP, SIZE, 4)
    windows = []
    for w, s in enumerate(WINDOW_STORE):
        r = rects[w]
        track = type("T", (), dict(rx=r["rx"], ry=r["ry"], ih=r["ih"], iw=r["iw"]))
        fit = (desc[w]["tfm"], int(desc[w]["canvas_h"]), int(desc[w]["canvas_w"]), np.stack([r["x"], r["y"]], 1).astype(np.int64))
        windows.append((stores[s], ORDERS[s], r["frame"], track, fit))
    out = torch.zeros((4, CLIP, SIZE, SIZE, 3), dtype=torch.uint8, device=_dev())
    warp(windows + windows[-1:], out)
    torch.cuda.synchronize()
    assert warp.launches == 1 and all(torch.equal(out[w], want[w]) for w in range(3)) and torch.equal(out[3], want[2])


# ---- the quality gate --------------------------------------------------------------------------------------------------------------

# (x0, y0, w, h): every form of the half-size step, sizes off the 8 x 32 tile, the origin, the far corner of the smaller frame
QSHAPES = [(10, 10, 2, 2), (20, 7, 1, 5), (30, 9, 5, 1), (40, 11, 3, 3), (50, 13, 4, 4), (60, 15, 5, 4), (3, 2, 101, 75), (0, 0, 37, 23),
           (112 - 41, 80 - 29, 41, 29), (5, 9, 70, 66), (33, 20, 64, 58)]


def test_quality_over_two_stores_equals_the_single_store_launch(stores):
    rects = [(stores[i % 2], ORDERS[i % 2], (i * 3) % 4, x, y, x + w, y + h) for i, (x, y, w, h) in enumerate(QSHAPES)]     # interleaved
    alone = [live.FaceQuality(stores[s], ORDERS[s]) for s in (0, 1)]
    want, want_grey = [], []
    for i, (store, _, slot, x0, y0, x1, y1) in enumerate(rects):
        sums, greys = alone[i % 2].sums([(slot, x0, y0, x1, y1)], grey=True)
        want.append(sums[0])
        want_grey.append(greys[0])
    assert len(set(want)) >= 8                                                    # the rectangles measure different things
    both = live.StoresQuality(_dev())
    got, grey = both.sums(rects, grey=True)
    assert both.launches == 1 and got == want
    assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(grey, want_grey))
    back, back_grey = both.sums(rects[::-1], grey=True)
    assert back == want[::-1] and all(np.array_equal(g, w) for g, w in zip(back_grey, want_grey[::-1]))
    assert both(rects) == [a for i, r in enumerate(rects) for a in alone[i % 2]([r[2:]])]
    # the same rectangle in the two stores is two measurements: the store index is read
    x, y, w, h = QSHAPES[9]
    pair = both.sums([(stores[0], "bgr", 1, x, y, x + w, y + h), (stores[1], "rgb", 1, x, y, x + w, y + h)])
    assert pair == [alone[0].sums([(1, x, y, x + w, y + h)])[0], alone[1].sums([(1, x, y, x + w, y + h)])[0]] and pair[0] != pair[1]
    many = [(stores[i % 2], ORDERS[i % 2], 1, i, 0, i + 4, 6) for i in range(70)]        # more than one launch's worth
    assert both.sums(many) == [alone[i % 2].sums([(1, i, 0, i + 4, 6)])[0] for i in range(70)] and both.launches == 6
    with pytest.raises(_lib.AfError):
        both.sums([(stores[1], "rgb", 0, 112 - 3, 0, 112 + 1, 4)])                       # inside store 0's frame, outside store 1's
    with pytest.raises(_lib.AfError):
        both.sums([(stores[1], "rgb", 4, 0, 0, 4, 4)])                                   # slot 4: store 0 has it, store 1 has not
