"""CPU: the host side of live.CallServer and the host halves of the several-stores entry points.  No device is touched.

  halves      track_candidates + track_gate composed equal track_faces on the scripted input of tests/test_realtime_host.py's kind
              (an excluded track, no landmarks, cached landmarks, a quality reject, a degenerate box, detections every other step);
              advance_host + the scoring equal LiveCall.step's books against the reference loop of tests/test_live_host.py
  planner     af_window_rects_plan_stores_u8 against a numpy restatement of its table: two stores of different pitch, size and
              byte order, the same frame indices used in both (an ignored store index would show), the last pixel of a store
  refusals    a store index out of range; a rectangle that leaves its frame in store 1 only; 3 bytes of slack missing behind store
              1 only - AF_ERR_ARG with the window and frame named
  arguments   af_yunet_detect_frames, af_face_quality_stores_u8 and the stores warp refuse bad arguments before any device call
  one planner the single-store and the several-stores planner write the same table for the same rectangles of store 0, refuse the
              same cases with the same code and the same (window, frame), and stamp a refused table as no table; the shared tail
              of WindowWarp / StoresWarp raises the aligner's canvas-misfit ValueError only for a rectangle that misfits its canvas
  one check   a table of broken stores, refused by all five entry points that take a store, each under its own name
"""
import ctypes as C
import types

import numpy as np
import pytest

import test_live_host as LH
import test_realtime_host as RH
from af_mi355x import _lib, evaluator, frames, live

L = _lib.lib


def test_abi_stays_six_and_the_structs_have_the_headers_layout():
    assert L.af_version() == 6
    assert C.sizeof(_lib.StoreRef) == 8 + 40 + 8 and _lib.StoreRef.desc.offset == 8 and _lib.StoreRef.bgr.offset == 48
    assert _lib.MAX_STORES == 64 and _lib.YUNET_MAX_LIST == 64


# ---- the two halves of track_faces -------------------------------------------------------------------------------------------------

def test_the_halves_of_track_faces_compose_to_track_faces():
    gate = lambda m, l: live.quality_weight(m, l)                                      # noqa: E731
    script = RH._host_script()
    whole, halves = live.CallState(), live.CallState()
    rejected = with_rects = 0
    for s, (dets, online, _) in enumerate(script):
        want = live.track_faces(whole, s, (RH.H, RH.W), dets, online, lambda rects, s=s: [RH._stub_quality(s, r) for r in rects], gate,
                                mesh_every=3, exclude_rect=RH.EXCLUDE)
        found = live.track_candidates(halves, s, (RH.H, RH.W), dets, online, mesh_every=3, exclude_rect=RH.EXCLUDE)
        rects = found[0]
        assert rects == want[3] and all(len(r) == 4 for r in rects)
        got = live.track_gate(halves, found, [RH._stub_quality(s, r) for r in rects], gate)
        assert [f[0] for f in got[0]] == [f[0] for f in want[0]], s
        for f, w in zip(got[0], want[0]):
            assert np.array_equal(f[1], w[1]) and np.array_equal(f[2], w[2]) and f[1].dtype == f[2].dtype == np.float32
        assert got[1] == want[1] and got[3] == want[3] and set(got[2]) == set(want[2])
        assert all(np.array_equal(got[2][t], want[2][t]) for t in want[2])
        rejected += 4 in got[1] and 30 <= s < 35
        with_rects += bool(rects)
    assert rejected == 5 and with_rects >= 100                                          # the blurry steps; most steps measure something
    assert set(whole.last_lm) == set(halves.last_lm)
    assert {t: list(v) for t, v in whole.q_hist.items()} == {t: list(v) for t, v in halves.q_hist.items()}


# ---- the two halves of LiveCall.advance --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 8, 52])
def test_advance_host_keeps_the_reference_loops_books(stride):
    script = LH.scripted_call()
    ring = LH.CLIP + LH.DROP
    call = LH.RecordingCall(clip_size=LH.CLIP, size=64, stride=stride, crop_scale=0.6, ring_frames=ring, max_batch=16, drop_after=LH.DROP)
    want = LH.reference_loop(script, LH.CLIP, stride, 0.6, LH.DROP)
    closed = 0
    for s, faces in enumerate(script):
        call.admit(LH._frame(s))
        ready = call.advance_host(faces)                                                # the books alone: nothing is scored
        batch, purged = want[s]
        assert call.scored == [] and sorted(call.purged) == purged, s
        assert [tid for tid, _ in ready] == [tid for tid, _, _ in batch], s
        for (tid, win), (_, ids, infos) in zip(ready, batch):
            assert [k for k, _ in win] == ids and all(LH._same_record(rec, info) for (_, rec), info in zip(win, infos)), (s, tid)
        closed += len(ready)
    assert closed > 3
    # advance is the composition: the windows advance_host returns are the windows it scores
    a = LH.RecordingCall(clip_size=LH.CLIP, size=64, stride=stride, crop_scale=0.6, ring_frames=ring, max_batch=16, drop_after=LH.DROP)
    for s, faces in enumerate(script[:60]):
        a.admit(LH._frame(s))
        n = len(a.scored)
        results = a.advance(faces)
        assert [t for t, _ in results] == [t for t, _, _ in want[s][0]] and len(a.scored) - n == bool(want[s][0])


# ---- the planner over several stores -----------------------------------------------------------------------------------------------

RECT = np.dtype([(n, "<i4") for n in ("frame", "rx", "ry", "ih", "iw", "x", "y", "reserved")])
WINDOW = np.dtype([("tfm", "<f8", (6,)), ("canvas_h", "<i4"), ("canvas_w", "<i4")])
ITEM = np.dtype([("first", "<u8"), ("ih", "<i4"), ("iw", "<i4"), ("x", "<i4"), ("y", "<i4"), ("pitch", "<i4"), ("bgr", "<i4")])
SHAPES = ((96, 131, 14), (80, 112, 9))                           # (height, width, frames) of store 0 and store 1
BASES = (0x7f0000001000, 0x7e0000000040)                          # addresses only: the planner never reads through them


def _ref(i, slack=3, bgr=None, base=None):
    h, w, n = SHAPES[i]
    return _lib.StoreRef(BASES[i] if base is None else base, _lib.FrameStore(n * h * w * 3 + slack, h * w * 3, w * 3, n, h, w, 0),
                         (1 - i) if bgr is None else bgr, 0)


def _stores(*refs):
    return (_lib.StoreRef * len(refs))(*refs)


def _case(rng, n_windows, clip, store_of):
    desc, rects = np.zeros(n_windows, dtype=WINDOW), np.zeros((n_windows, clip), dtype=RECT)
    for w in range(n_windows):
        h, wd, n = SHAPES[store_of[w]]
        rects["frame"][w] = (w + np.arange(clip)) % 9             # the same frame numbers in both stores
        rects["ih"][w], rects["iw"][w] = rng.integers(1, 40, clip), rng.integers(1, 50, clip)
        rects["ry"][w], rects["rx"][w] = rng.integers(0, h - 40, clip), rng.integers(0, wd - 50, clip)
        rects["x"][w], rects["y"][w] = rng.integers(0, 9, clip), rng.integers(0, 9, clip)
        rects["reserved"][w] = store_of[w]
        desc[w] = ([1.1, -0.1, 3.0, 0.1, 1.1, -2.0], int((rects["y"][w] + rects["ih"][w]).max()), int((rects["x"][w] + rects["iw"][w]).max()))
    return desc, rects


def _plan(desc, rects, size, stores, n_stores=None, table=None):
    n, clip = rects.shape
    if table is None:
        table = np.zeros(L.af_window_rects_table_bytes(n, clip) // 8, dtype=np.int64)
    bw, bf = C.c_int32(-7), C.c_int32(-7)
    rc = L.af_window_rects_plan_stores_u8(desc.ctypes.data, rects.ctypes.data, n, clip, size, stores, len(stores) if n_stores is None else n_stores,
                                          table.ctypes.data, table.nbytes, C.byref(bw), C.byref(bf))
    return rc, bw.value, bf.value, table


def test_stores_plan_table_against_restatement():
    rng = np.random.default_rng(11)
    store_of = [1, 0, 0, 1, 0]
    desc, rects = _case(rng, 5, 4, store_of)
    h1, w1, n1 = SHAPES[1]
    rects[3, 2] = (n1 - 1, w1 - 2, h1 - 1, 1, 2, 0, 0, 1)         # the last two pixels of the last frame of store 1
    rc, bw, bf, table = _plan(desc, rects, 8, _stores(_ref(0), _ref(1)))
    assert rc == 0 and (bw, bf) == (-1, -1), L.af_last_error()
    raw = table.view(np.uint8)
    assert raw[:16].view("<i4").tolist() == [5, 4, 8, 2]         # kind 2: neither the pool nor the single-store launch takes this table
    items = raw[16 + 5 * 48:16 + 5 * 48 + 20 * 32].view(ITEM).reshape(5, 4)
    for w, s in enumerate(store_of):
        h, wd, _ = SHAPES[s]
        r = rects[w]
        want = BASES[s] + r["frame"].astype(np.int64) * (h * wd * 3) + r["ry"].astype(np.int64) * (wd * 3) + r["rx"] * 3
        np.testing.assert_array_equal(items["first"][w].astype(np.int64), want)
        assert (items["pitch"][w] == wd * 3).all() and (items["bgr"][w] == 1 - s).all()
        for k in ("ih", "iw", "x", "y"):
            np.testing.assert_array_equal(items[k][w], r[k])
    assert int(items["first"][3, 2]) + 6 == BASES[1] + n1 * h1 * w1 * 3
    # the stores exchanged, and the indices with them: the same table
    swapped = rects.copy()
    swapped["reserved"] = 1 - rects["reserved"]
    rc, _, _, other = _plan(desc, swapped, 8, _stores(_ref(1), _ref(0)))
    assert rc == 0 and np.array_equal(other, table)
    # the transform is the single-store planner's
    single = np.zeros_like(table)
    st = _lib.FrameStore(14 * 96 * 131 * 3 + 3, 96 * 131 * 3, 131 * 3, 14, 96, 131, 0)
    r0 = rects.copy()
    r0[3, 2] = r0[3, 1]
    assert L.af_window_rects_plan_u8(desc.ctypes.data, r0.ctypes.data, 5, 4, 8, C.byref(st), single.ctypes.data, single.nbytes, None, None) == 0
    assert np.array_equal(single.view(np.uint8)[16:16 + 5 * 48], raw[16:16 + 5 * 48])


def test_stores_plan_refuses_a_store_index_out_of_range():
    rng = np.random.default_rng(12)
    desc, rects = _case(rng, 3, 4, [0, 1, 0])
    both = _stores(_ref(0), _ref(1))
    assert _plan(desc, rects, 8, both)[0] == 0
    for value in (2, -1, 64):
        r = rects.copy()
        r["reserved"][1, 2] = value
        rc, bw, bf, table = _plan(desc, r, 8, both)
        assert rc == -1 and (bw, bf) == (1, 2), value
        msg = L.af_last_error().decode()
        assert "window 1 frame 2" in msg and "store" in msg
        assert table.view(np.uint8)[:16].view("<i4")[3] != 2     # a refused table is no table of this form
    r = rects.copy()                                              # one store handed in: index 1 is out of range
    rc, bw, bf, _ = _plan(desc, r, 8, both, n_stores=1)
    assert rc == -1 and (bw, bf) == (1, 0) and "window 1 frame 0" in L.af_last_error().decode()


def test_stores_plan_refuses_a_rectangle_that_leaves_its_frame_in_store_1_only():
    rng = np.random.default_rng(13)
    desc, rects = _case(rng, 2, 3, [0, 1])
    desc["canvas_w"], desc["canvas_h"] = 400, 400
    both = _stores(_ref(0), _ref(1))
    h1, w1, n1 = SHAPES[1]
    inside0 = (3, w1 - 10, h1 - 10, 20, 20, 0, 0)                 # fits a 96 x 131 frame, leaves an 80 x 112 one
    rects[0, 1] = inside0 + (0,)
    assert _plan(desc, rects, 8, both)[0] == 0
    rects[1, 2] = inside0 + (1,)
    rc, bw, bf, _ = _plan(desc, rects, 8, both)
    assert rc == -1 and (bw, bf) == (1, 2)
    msg = L.af_last_error().decode()
    assert "window 1 frame 2" in msg and "leaves" in msg and "store 1" in msg
    rects[1, 2] = (n1, 0, 0, 4, 4, 0, 0, 1)                       # frame 9: there in store 0 (14 frames), not in store 1 (9)
    rc, bw, bf, _ = _plan(desc, rects, 8, both)
    assert rc == -1 and (bw, bf) == (1, 2) and "window 1 frame 2" in L.af_last_error().decode()
    rects[1, 2] = (n1, 0, 0, 4, 4, 0, 0, 0)
    assert _plan(desc, rects, 8, both)[0] == 0
    rects["x"][0, 2] = 400                                        # and the canvas misfit is named as the single-store planner names it
    rc, bw, bf, _ = _plan(desc, rects, 8, both)
    assert rc == -1 and (bw, bf) == (0, 2) and "does not fit" in L.af_last_error().decode()


def test_stores_plan_wants_the_slack_behind_each_store():
    rng = np.random.default_rng(14)
    desc, rects = _case(rng, 2, 3, [0, 1])
    desc["canvas_w"], desc["canvas_h"] = 400, 400
    (h0, w0, n0), (h1, w1, n1) = SHAPES
    rects[0, 0] = (n0 - 1, w0 - 1, h0 - 1, 1, 1, 0, 0, 0)         # the last pixel of store 0
    rects[1, 1] = (n1 - 1, w1 - 1, h1 - 1, 1, 1, 0, 0, 1)         # the last pixel of store 1
    assert _plan(desc, rects, 8, _stores(_ref(0), _ref(1)))[0] == 0
    for slack, want in ((3, 0), (2, -1), (0, -1)):
        rc, bw, bf, _ = _plan(desc, rects, 8, _stores(_ref(0), _ref(1, slack=slack)))
        assert rc == want, slack
        if want:
            assert (bw, bf) == (1, 1)
            msg = L.af_last_error().decode()
            assert "window 1 frame 1" in msg and "3 readable bytes" in msg and "store 1" in msg
    rc, bw, bf, _ = _plan(desc, rects, 8, _stores(_ref(0, slack=2), _ref(1)))
    assert rc == -1 and (bw, bf) == (0, 0)
    rects[1, 1] = (n1 - 1, w1 - 2, h1 - 1, 1, 1, 0, 0, 1)         # one pixel earlier: the frame's own last pixel is the slack
    assert _plan(desc, rects, 8, _stores(_ref(0), _ref(1, slack=0)))[0] == 0


def test_stores_plan_and_launch_refuse_bad_arguments_without_a_device():
    rng = np.random.default_rng(15)
    desc, rects = _case(rng, 2, 3, [0, 1])
    both = _stores(_ref(0), _ref(1))
    rc, _, _, table = _plan(desc, rects, 8, both)
    assert rc == 0
    args = lambda **k: [k.get("desc", desc.ctypes.data), k.get("rects", rects.ctypes.data), k.get("n", 2), k.get("clip", 3),  # noqa: E731
                        k.get("size", 8), k.get("stores", both), k.get("n_stores", 2), k.get("table", table.ctypes.data),
                        k.get("table_bytes", table.nbytes), None, None]
    assert L.af_window_rects_plan_stores_u8(*args()) == 0
    h0, w0, n0 = SHAPES[0]
    short = _ref(0)
    short.desc.row_pitch = w0 * 3 - 1
    small = _ref(0)
    small.desc.store_bytes = n0 * h0 * w0 * 3 - 1
    many = (_lib.StoreRef * 65)(*[_ref(0)] * 65)
    for bad in (dict(desc=None), dict(rects=None), dict(table=None), dict(stores=None), dict(n=0), dict(n=_lib.WINDOW_MAX_BATCH + 1),
                dict(clip=0), dict(clip=_lib.ALIGN_MAX_FRAMES + 1), dict(size=0), dict(size=6), dict(size=_lib.WINDOW_MAX_SIZE + 4),
                dict(table_bytes=table.nbytes - 8), dict(n_stores=0), dict(stores=many, n_stores=65),
                dict(stores=_stores(_ref(0), _ref(1, base=0))), dict(stores=_stores(short, _ref(1))), dict(stores=_stores(small, _ref(1)))):
        assert L.af_window_rects_plan_stores_u8(*args(**bad)) == -1, bad
        assert L.af_last_error()
    assert L.af_window_rects_plan_stores_u8(*args(stores=many, n_stores=64)) == 0
    one = C.c_void_p(table.ctypes.data)
    assert L.af_warp_affine_window_stores_u8(None, 2, 3, 8, one, None) == -1 and b"null" in L.af_last_error()
    assert L.af_warp_affine_window_stores_u8(one, 2, 3, 8, None, None) == -1
    for n, clip, size in ((0, 3, 8), (65, 3, 8), (2, 0, 8), (2, 65, 8), (2, 3, 6), (2, 3, 1028)):
        assert L.af_warp_affine_window_stores_u8(one, n, clip, size, one, None) == -1, (n, clip, size)
    assert L.af_warp_affine_window_stores_u8(one, 2, 3, 8, C.c_void_p(table.ctypes.data + 2), None) == -1


# ---- one planner behind both entry points ------------------------------------------------------------------------------------------

SINGLE_ITEM = np.dtype([("offset", "<i8"), ("ih", "<i4"), ("iw", "<i4"), ("x", "<i4"), ("y", "<i4"), ("pitch", "<i4"), ("reserved", "<i4")])


def _plan_single(desc, rects, size, slack=3):
    n, clip = rects.shape
    h, w, frames = SHAPES[0]
    st = _lib.FrameStore(frames * h * w * 3 + slack, h * w * 3, w * 3, frames, h, w, 0)
    table = np.zeros(L.af_window_rects_table_bytes(n, clip) // 8, dtype=np.int64)
    bw, bf = C.c_int32(-7), C.c_int32(-7)
    rc = L.af_window_rects_plan_u8(desc.ctypes.data, rects.ctypes.data, n, clip, size, C.byref(st), table.ctypes.data, table.nbytes,
                                   C.byref(bw), C.byref(bf))
    return rc, bw.value, bf.value, table


def _store0_case(seed):
    desc, rects = _case(np.random.default_rng(seed), 3, 4, [0, 0, 0])
    desc["canvas_w"], desc["canvas_h"] = 400, 400
    return desc, rects


def test_both_planners_write_the_same_table_for_one_store():
    desc, rects = _store0_case(21)
    h, w, n = SHAPES[0]
    rects[2, 3] = (n - 1, w - 2, h - 1, 1, 2, 0, 0, 0)           # the last two pixels of the store
    rc, bw, bf, single = _plan_single(desc, rects, 8)
    assert rc == 0 and (bw, bf) == (-1, -1), L.af_last_error()
    rc, bw, bf, listed = _plan(desc, rects, 8, _stores(_ref(0)))
    assert rc == 0 and (bw, bf) == (-1, -1), L.af_last_error()
    a, b = single.view(np.uint8), listed.view(np.uint8)
    assert a[:16].view("<i4").tolist() == [3, 4, 8, 1] and b[:16].view("<i4").tolist() == [3, 4, 8, 2]      # the header apart from kind
    assert np.array_equal(a[16:16 + 3 * 48], b[16:16 + 3 * 48])                                           # the transforms
    items = slice(16 + 3 * 48, 16 + 3 * 48 + 12 * 32)
    one, many = a[items].view(SINGLE_ITEM), b[items].view(ITEM)
    np.testing.assert_array_equal(many["first"].astype(np.int64), BASES[0] + one["offset"])
    for k in ("ih", "iw", "x", "y", "pitch"):
        np.testing.assert_array_equal(one[k], many[k])
    flat = rects.reshape(-1)
    np.testing.assert_array_equal(one["offset"], flat["frame"].astype(np.int64) * (h * w * 3) + flat["ry"].astype(np.int64) * (w * 3) + flat["rx"] * 3)
    assert (one["reserved"] == 0).all() and (many["bgr"] == 1).all() and _ref(0).bgr == 1
    assert (one["pitch"] == w * 3).all()


def test_both_planners_refuse_alike():
    h, w, n = SHAPES[0]

    def leaves(desc, rects):
        rects[1, 2] = (0, w - 10, 5, 20, 11, 0, 0, 0)            # one pixel over the right edge of its frame
        return 3

    def ends_the_store(desc, rects):
        rects[1, 2] = (n - 1, w - 1, h - 1, 1, 1, 0, 0, 0)       # the last pixel of a store with 2 bytes behind it
        return 2

    def misfit(desc, rects):
        rects["x"][1, 2] = 400 - rects["iw"][1, 2] + 1
        return 3

    def bad_canvas(desc, rects):
        desc["canvas_h"][1] = 0
        return 3

    for case in (leaves, ends_the_store, misfit, bad_canvas):
        desc, rects = _store0_case(22)
        slack = case(desc, rects)
        rc1, bw1, bf1, single = _plan_single(desc, rects, 8, slack=slack)
        said1 = L.af_last_error().decode()
        rc2, bw2, bf2, listed = _plan(desc, rects, 8, _stores(_ref(0, slack=slack)))
        said2 = L.af_last_error().decode()
        assert rc1 == rc2 == -1, case.__name__
        assert said1.startswith("aligner: " if case is misfit else "window_rects_plan: ") and \
            said2.startswith("aligner: " if case is misfit else "window_rects_plan_stores: "), (said1, said2)
        assert ("does not fit" in said1) == ("does not fit" in said2) == (case is misfit), (said1, said2)
        if case is bad_canvas:
            assert "bad canvas" in said1 and "bad canvas" in said2
            continue
        assert (bw1, bf1) == (bw2, bf2) == (1, 2), case.__name__
        assert "window 1 frame 2" in said1 and "window 1 frame 2" in said2
        for table in (single, listed):
            assert table.view(np.uint8)[:16].view("<i4")[3] not in (0, 1, 2), case.__name__      # a refused table is no table
        assert ("leaves" in said1) == ("leaves" in said2) == (case is leaves)
        assert ("3 readable bytes" in said1) == ("3 readable bytes" in said2) == (case is ends_the_store)


def test_the_warps_shared_tail_calls_only_a_canvas_misfit_a_canvas_misfit():
    """WindowWarp._plan, the host part of the tail every form of the warp shares, over a 64 x 64 store of 4 frames that lives in
    host memory (the planner reads no pixel): the planner names the (window, frame) of every refusal, and only a rectangle that
    really misfits its canvas becomes the aligner's ValueError"""
    store = evaluator.FrameStore(None, "bgr")
    store.open((64, 64, 3), 4)
    fit = (np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), 40, 40, np.zeros((2, 2), dtype=np.int64))

    def records(warp, rx):
        desc, items = warp._records(1)
        warp._fill(desc, items, 0, fit, [20, 20], [20, 20])
        items["frame"][0], items["rx"][0], items["ry"][0] = [0, 3], [10, rx], [10, 10]
        return desc, items

    single = evaluator.WindowWarp(evaluator.RECTS_BGR, store, clip_size=2, size=8, batch=2)
    listed = evaluator.StoresWarp("cpu", clip_size=2, size=8, batch=2)               # the device is the launch's: not touched here
    table = np.zeros(single.table_bytes // 8, dtype=np.int64)
    forms = ((single, lambda: (store.plan_source(),)), (listed, lambda: ((_lib.StoreRef * 1)(frames.store_ref(store, "bgr")), 1)))
    for warp, where in forms:
        warp._plan(*records(warp, 44), where(), table.ctypes.data)                     # 44 + 20 = 64: the rectangle ends with its frame
        assert table.view(np.uint8)[:16].view("<i4").tolist()[:3] == [1, 2, 8]
        with pytest.raises(_lib.AfError, match="window 0 frame 1.*leaves") as refused:
            warp._plan(*records(warp, 45), where(), table.ctypes.data)
        assert "does not fit" not in str(refused.value)
        desc, items = records(warp, 44)
        items["x"][0, 1] = 21                                                          # 21 + 20 > 40
        with pytest.raises(ValueError, match=r"window 0 frame 1 \(20x20 at 21,0\) does not fit the 40x40 canvas"):
            warp._plan(desc, items, where(), table.ctypes.data)


# ---- one store check behind five entry points --------------------------------------------------------------------------------------

def _broken_stores():
    """store 1 (80 x 112, 9 frames; even, so that a YUV frame of its size exists) with one field wrong at a time"""
    h, w, n = SHAPES[1]
    return {"pitch": dict(row_pitch=w * 3 - 1), "stride": dict(frame_stride=(h - 1) * w * 3 + w * 3 - 1), "bytes": dict(store_bytes=n * h * w * 3 - 1),
            "no frames": dict(n_frames=0), "width": dict(width=32768, row_pitch=32768 * 3, frame_stride=h * 32768 * 3, store_bytes=1 << 40)}


def _broken(fields):
    ref = _ref(1, slack=0)
    for k, v in fields.items():
        setattr(ref.desc, k, v)
    return ref


@pytest.mark.parametrize("what", list(_broken_stores()))
def test_a_broken_store_is_refused_by_every_entry_point_under_its_own_name(what):
    ref = _broken(_broken_stores()[what])
    h, w, n = SHAPES[1]
    desc, rects = np.zeros(1, dtype=WINDOW), np.zeros((1, 2), dtype=RECT)
    desc[0] = ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 40, 40)
    rects["ih"], rects["iw"] = 10, 12
    table = np.zeros(L.af_window_rects_table_bytes(1, 2) // 8, dtype=np.int64)
    sums = np.zeros(64 * 3, dtype=np.int64)
    pixels = C.c_void_p(BASES[1])                                 # an address only: every refusal comes before the first device call
    plan = [desc.ctypes.data, rects.ctypes.data, 1, 2, 8]
    calls = {"window_rects_plan": lambda: L.af_window_rects_plan_u8(*plan, C.byref(ref.desc), table.ctypes.data, table.nbytes, None, None),
             "window_rects_plan_stores": lambda: L.af_window_rects_plan_stores_u8(*plan, _stores(ref), 1, table.ctypes.data, table.nbytes, None, None),
             "face_quality": lambda: L.af_face_quality_u8(pixels, C.byref(ref.desc), rects.ctypes.data, 2, 1, C.c_void_p(sums.ctypes.data), None, 0, None),
             "face_quality_stores": lambda: L.af_face_quality_stores_u8(_stores(ref), 1, rects.ctypes.data, 2, C.c_void_p(sums.ctypes.data), None, 0, None)}
    if what != "width":                                           # a YUV frame of 32768 columns is refused before its store is looked at
        frame = (_lib.YuvFrameDesc * 1)(_lib.YuvFrameDesc(0x1000, 0x2000, None, w, w, h, w, 1, 0, 0, n - 1))      # nv12 into the last slot
        items = (_lib.YuvItem * 1)()
        calls["yuv420_plan"] = lambda: L.af_yuv420_plan_u8(C.byref(frame), 1, C.byref(_stores(ref)), 1, C.byref(items))
    for name, call in calls.items():
        assert call() == -1, (what, name)
        assert L.af_last_error().decode().startswith(name + ": "), (what, name, L.af_last_error())
    good = _ref(1, slack=0)                                        # and the store as it should be passes all five (no rectangle ends it)
    ref.desc = good.desc
    assert all(call() == 0 for name, call in calls.items() if "quality" not in name), L.af_last_error()


# ---- the other two entry points: every refusal comes before the first device call ---------------------------------------------------

def test_yunet_detect_frames_refuses_bad_arguments_without_a_device():
    buf = np.zeros(64, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    desc = lambda b: _lib.YunetDesc(b, 96, 131, 100, 0, 393, 0.5, 0.3)                 # noqa: E731  frame_stride 0: it is not read
    ptrs = lambda n, hole=None: (C.c_void_p * n)(*[None if i == hole else buf.ctypes.data for i in range(n)])       # noqa: E731
    call = lambda d, frames: L.af_yunet_detect_frames(C.byref(d) if d is not None else None, p, frames, p, 1 << 20, p, p, None, None)   # noqa: E731
    assert call(desc(3), ptrs(3, hole=1)) == -1 and b"frame 1" in L.af_last_error()
    assert call(desc(65), ptrs(65)) == -1 and b"at most 64" in L.af_last_error()
    assert call(desc(0), ptrs(1)) == -1
    assert call(desc(2), None) == -1 and call(None, ptrs(2)) == -1
    d = desc(2)
    d.row_pitch = 392                                             # the checks of af_yunet_detect behind the list's own
    assert call(d, ptrs(2)) == -1 and b"row pitch" in L.af_last_error()
    d = desc(2)
    d.top_k = 0
    assert call(d, ptrs(2)) == -1
    assert L.af_yunet_detect_frames(C.byref(desc(2)), None, ptrs(2), p, 1 << 20, p, p, None, None) == -1          # weights
    assert L.af_yunet_detect_frames(C.byref(desc(2)), p, ptrs(2), p, 16, p, p, None, None) == -1                  # workspace too small
    assert b"workspace" in L.af_last_error()


def test_face_quality_stores_refuses_bad_arguments_without_a_device():
    buf = np.zeros(64 * 3, dtype=np.int64)
    sums = C.c_void_p(buf.ctypes.data)
    both = _stores(_ref(0), _ref(1))
    rects = np.zeros(65, dtype=RECT)
    rects["ih"], rects["iw"] = 10, 12
    rects["reserved"] = np.arange(65) % 2
    call = lambda stores, ns, r, n: L.af_face_quality_stores_u8(stores, ns, r.ctypes.data if r is not None else None, n, sums, None, 0, None)  # noqa: E731
    assert call(both, 2, rects, 65) == -1 and b"at most 64" in L.af_last_error()
    assert call(both, 2, rects, -1) == -1
    assert call(both, 2, rects, 0) == 0                           # nothing to do, nothing launched
    many = (_lib.StoreRef * 65)(*[_ref(0)] * 65)
    assert call(many, 65, rects, 4) == -1 and b"stores" in L.af_last_error()
    assert call(both, 0, rects, 4) == -1
    assert call(None, 2, rects, 4) == -1 and call(both, 2, None, 4) == -1
    assert L.af_face_quality_stores_u8(both, 2, rects.ctypes.data, 4, None, None, 0, None) == -1
    r = rects.copy()
    r["reserved"][3] = 2
    assert call(both, 2, r, 4) == -1 and b"rectangle 3" in L.af_last_error()
    h1, w1, n1 = SHAPES[1]
    r = rects.copy()
    r[3] = (0, w1 - 10, 0, 10, 12, 0, 0, 1)                       # inside a frame of store 0, over the edge of one of store 1
    assert call(both, 2, r, 4) == -1 and b"rectangle 3" in L.af_last_error() and b"store 1" in L.af_last_error()
    r = rects.copy()
    r[3] = (n1, 0, 0, 10, 12, 0, 0, 1)
    assert call(both, 2, r, 4) == -1 and b"rectangle 3" in L.af_last_error()
    assert call(_stores(_ref(0), _ref(1, base=0)), 2, rects, 4) == -1 and b"store 1" in L.af_last_error()


def test_call_server_keeps_what_is_the_servers_out_of_a_call():
    assert live.CallServer.__init__.__defaults__ is not None
    for name in ("clip_size", "size", "max_batch"):
        with pytest.raises(TypeError, match="belongs to the server"):
            live.CallServer.open(types.SimpleNamespace(call_defaults={}), **{name: 4})
    stats = live.ServerStats()
    stats.begin()
    stats.count("detect")
    stats.count("wait", 2)
    stats.begin()
    stats.count("wait")
    assert stats.steps == 2 and stats.last == dict(detect=0, quality=0, warp=0, replay=0, wait=1) and stats.total["wait"] == 3
