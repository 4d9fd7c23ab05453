"""CPU: the host side of VideoScorer (evaluator.py).

  * get_valid_faces / multiple_tracking / find_longest against tests/golden/video_tracks.json, which tools/gen_video_golden.py
    recorded by executing the reference's own functions (test_tools/ct/detection/utils.py:75-89, ct/operations.py:13-80) on seeded
    detection lists: every case must reproduce exactly, tracks as per-frame indices into the input lists, spans as tuples;
  * af_window_rects_plan_u8 (the table of one window-batch warp launch out of resident frames): offsets and pitch against a short
    restatement, and its refusals - a rectangle that leaves its frame, one that does not fit its canvas (window and frame named as
    the pool form names them), a store that ends without the 3 bytes of slack.
No device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_json
from af_mi355x import _lib, evaluator

GOLDEN = load_json("video_tracks.json")["cases"]
NEEDED = ["steady", "crossing", "overlap_in_frame0", "frame0_score_079", "frame0_score_080", "vanishes", "last_frame_empty",
          "more_than_ten", "at_least"]


def _frames(case):
    return [[(np.array(f["box"], dtype=np.float32), np.array(f["lm"], dtype=np.float32), np.float32(f["score"])) for f in faces]
            for faces in case["frames"]]


def _valid(case):
    """(the frames, get_valid_faces of them, per frame the input index of every kept face)"""
    frames = _frames(case)
    valid = evaluator.get_valid_faces(frames, **case["args"])
    idx = []
    for faces_in, faces_out in zip(frames, valid):
        found = []
        for f in faces_out:
            hits = [k for k, g in enumerate(faces_in) if g[2] == f[2] and np.array_equal(g[0].astype(np.float64), f[0])
                    and np.array_equal(g[1].astype(np.float64), f[1])]
            assert len(hits) == 1
            found.append(hits[0])
        idx.append(found)
    return frames, valid, idx


def _indices(track, start, valid, idx):
    out = []
    for t, f in enumerate(track):
        k = [j for j, g in enumerate(valid[start + t]) if g is f]                 # a track holds the input's own face objects
        assert len(k) == 1
        out.append(idx[start + t][k[0]])
    return out


def test_the_fixture_holds_the_cases_the_tracking_contract_names():
    assert set(NEEDED) <= set(GOLDEN)
    g = GOLDEN
    assert len(g["steady"]["tracks"]) == 1 and len(g["crossing"]["tracks"]) == 2
    assert len(g["overlap_in_frame0"]["frames"][0]) == 3 and len(g["overlap_in_frame0"]["tracks"]) == 2   # the overlapping face starts none
    assert g["frame0_score_079"]["tracks"] == [] and len(g["frame0_score_080"]["tracks"]) == 1
    assert g["vanishes"]["tracks"] == [] and len(g["vanishes"]["spans"]) > 1
    assert g["last_frame_empty"]["frames"][-1] == [] and g["last_frame_empty"]["spans"] == [[0, len(g["last_frame_empty"]["frames"]) - 1]]
    assert all(len(f) > 10 for f in g["more_than_ten"]["frames"]) and all(len(v) <= 10 for v in g["more_than_ten"]["valid"])
    assert g["at_least"]["args"]["at_least"] is True and g["at_least"]["valid"] != g["not_at_least"]["valid"]


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_valid_faces_tracks_and_spans_equal_the_reference(name):
    case = GOLDEN[name]
    frames, valid, idx = _valid(case)
    assert idx == case["valid"]
    for faces in valid:
        for box, lm, score in faces:
            assert box.dtype == np.float64 and lm.dtype == np.float64 and box.shape == (4,) and lm.shape == (5, 2)
            assert isinstance(score, np.float32)                              # the score is handed on as it came
    tracks = evaluator.multiple_tracking(valid)
    assert [_indices(t, 0, valid, idx) for t in tracks] == case["tracks"]
    assert all(len(t) == len(frames) for t in tracks)
    if "raises" in case:
        with pytest.raises(NotImplementedError):
            evaluator.find_longest(valid)
        return
    spans, span_tracks = evaluator.find_longest(valid)
    assert [tuple(s) for s in spans] == [tuple(s) for s in case["spans"]] and all(isinstance(s, tuple) for s in spans)
    assert [_indices(t, s[0], valid, idx) for s, t in zip(spans, span_tracks)] == case["span_tracks"]
    assert all(len(t) == b - a for (a, b), t in zip(spans, span_tracks))


def test_find_longest_equals_tracking_every_prefix_from_scratch():
    """the incremental form against the reference's quadratic loop written out with multiple_tracking, on every golden case and
    on random appearances and disappearances"""
    def quadratic(res):
        fc, spans, tracks, start, end, prev = len(res), [], [], 0, 0, -1
        while start < fc - 1:
            for end in range(start + 2, fc + 1):
                got = evaluator.multiple_tracking(res[start:end])
                if (len(got) != prev and prev != -1) or len(got) == 0:
                    break
                prev = len(got)
            if end - start > 2:
                stop = end - 1 if end != fc else end
                sub = evaluator.multiple_tracking(res[start:stop])
                if end == fc and len(sub) == 0:
                    stop = end - 1
                    sub = evaluator.multiple_tracking(res[start:stop])
                assert len(sub) > 0
                spans.append((start, stop))
                tracks.append(sub[0])
                prev, end = -1, stop
            start = end
        return spans, tracks

    inputs = [_valid(case)[1] for case in GOLDEN.values() if "raises" not in case]
    rng = np.random.default_rng(77)
    for _ in range(20):
        n = int(rng.integers(3, 40))
        res = []
        for i in range(n):
            faces = []
            for k in range(3):
                if rng.uniform() < 0.8:
                    c = 100.0 + 150.0 * k + rng.normal(0, 8.0)
                    faces.append((np.array([c - 40, 60.0, c + 40, 160.0]), np.zeros((5, 2)), np.float32(rng.choice([0.95, 0.85, 0.7]))))
            res.append(faces)
        inputs.append(res)
    for res in inputs:
        want, got = quadratic(res), evaluator.find_longest(res)
        assert got[0] == want[0] and len(got[1]) == len(want[1])
        for a, b in zip(got[1], want[1]):
            assert len(a) == len(b) and all(x is y for x, y in zip(a, b))


def test_iou_arithmetic():
    a, b = np.array([0.0, 0.0, 10.0, 10.0]), np.array([5.0, 5.0, 15.0, 15.0])
    assert evaluator.iou(a, b) == 25.0 / (100.0 + 100.0 - 25.0) and evaluator.iou(a, a) == 1.0
    assert evaluator.iou(a, np.array([20.0, 20.0, 30.0, 30.0])) == 0.0


# ---- the launch table of the resident-frame form ---------------------------------------------------------------------------------

RECT = np.dtype([(n, "<i4") for n in ("frame", "rx", "ry", "ih", "iw", "x", "y", "reserved")])
WINDOW = np.dtype([("tfm", "<f8", (6,)), ("canvas_h", "<i4"), ("canvas_w", "<i4")])
ITEM = np.dtype([("offset", "<i8"), ("ih", "<i4"), ("iw", "<i4"), ("x", "<i4"), ("y", "<i4"), ("pitch", "<i4"), ("reserved", "<i4")])
H, W, N_FRAMES = 359, 641, 7                                     # row pitch 1 923 bytes: no multiple of 4
PITCH, FRAME_BYTES = W * 3, H * W * 3


def _store(store_bytes=N_FRAMES * FRAME_BYTES + 3, **k):
    return _lib.FrameStore(store_bytes, k.get("frame_stride", FRAME_BYTES), k.get("row_pitch", PITCH), k.get("n_frames", N_FRAMES),
                           k.get("height", H), k.get("width", W), 0)


def _case(rng, n_windows, clip_size):
    desc, rects = np.zeros(n_windows, dtype=WINDOW), np.zeros((n_windows, clip_size), dtype=RECT)
    for w in range(n_windows):
        rects["frame"][w] = (w + np.arange(clip_size)) % N_FRAMES
        rects["ih"][w], rects["iw"][w] = rng.integers(1, 120, clip_size), rng.integers(1, 200, clip_size)
        rects["ry"][w], rects["rx"][w] = rng.integers(0, H - 120, clip_size), rng.integers(0, W - 200, clip_size)
        rects["x"][w], rects["y"][w] = rng.integers(0, 9, clip_size), rng.integers(0, 9, clip_size)
        desc[w] = ([1.1, -0.1, 3.0, 0.1, 1.1, -2.0], int((rects["y"][w] + rects["ih"][w]).max()), int((rects["x"][w] + rects["iw"][w]).max()))
    return desc, rects


def _plan(desc, rects, size, store, table=None):
    n, clip = rects.shape
    if table is None:
        table = np.zeros(_lib.lib.af_window_rects_table_bytes(n, clip) // 8, dtype=np.int64)
    bw, bf = C.c_int32(-7), C.c_int32(-7)
    rc = _lib.lib.af_window_rects_plan_u8(desc.ctypes.data, rects.ctypes.data, n, clip, size, C.byref(store), table.ctypes.data, table.nbytes,
                                          C.byref(bw), C.byref(bf))
    return rc, bw.value, bf.value, table


def test_rect_structs_and_table_size():
    assert C.sizeof(_lib.FrameRect) == RECT.itemsize == 32 and C.sizeof(_lib.FrameStore) == 40 and ITEM.itemsize == 32
    assert _lib.lib.af_window_rects_table_bytes(16, 32) == _lib.WINDOW_TABLE_HEADER + 16 * 48 + 16 * 32 * 32
    for bad in ((0, 32), (_lib.WINDOW_MAX_BATCH + 1, 32), (16, 0), (16, _lib.ALIGN_MAX_FRAMES + 1)):
        assert _lib.lib.af_window_rects_table_bytes(*bad) == 0
    assert _lib.lib.af_version() == 6                            # new entry points within ABI 6, as the pool form was added


def test_rect_plan_table_against_restatement():
    rng = np.random.default_rng(1)
    desc, rects = _case(rng, 5, 4)
    rects[4, 3] = (N_FRAMES - 1, W - 2, H - 1, 1, 2, 0, 0, 0)     # the last two pixels of the last frame of the store
    rc, bw, bf, table = _plan(desc, rects, 8, _store())
    assert rc == 0 and (bw, bf) == (-1, -1), _lib.lib.af_last_error()
    raw = table.view(np.uint8)
    assert raw[:16].view("<i4").tolist() == [5, 4, 8, 1]         # kind 1: the pool form's launch refuses this table and vice versa
    items = raw[16 + 5 * 48:16 + 5 * 48 + 20 * 32].view(ITEM)
    flat = rects.reshape(-1)
    want_off = flat["frame"].astype(np.int64) * FRAME_BYTES + flat["ry"].astype(np.int64) * PITCH + flat["rx"] * 3
    np.testing.assert_array_equal(items["offset"], want_off)
    for k in ("ih", "iw", "x", "y"):
        np.testing.assert_array_equal(items[k], flat[k])
    assert (items["pitch"] == PITCH).all() and PITCH % 4 != 0
    assert int(items["offset"][-1]) + 6 == N_FRAMES * FRAME_BYTES                                   # two pixels before the end of the frames


def test_rect_plan_refuses_a_rectangle_that_leaves_its_frame():
    rng = np.random.default_rng(2)
    desc, rects = _case(rng, 3, 4)
    assert _plan(desc, rects, 8, _store())[0] == 0
    for field, value in (("rx", -1), ("ry", -1), ("frame", N_FRAMES), ("frame", -1), ("ih", 0), ("iw", 0)):
        r = rects.copy()
        r[field][1, 2] = value
        rc, bw, bf, _ = _plan(desc, r, 8, _store())
        assert rc == -1 and b"window 1 frame 2" in _lib.lib.af_last_error(), (field, value)
    r = rects.copy()                                              # one pixel over the right edge / the bottom edge of its frame: its
    r[2, 0] = (0, W - 10, 5, 20, 11, 0, 0, 0)                     # bytes would still lie inside the store (the next row, the next frame)
    d = desc.copy()
    d["canvas_w"], d["canvas_h"] = 400, 400
    rc, bw, bf, _ = _plan(d, r, 8, _store())
    assert rc == -1 and (bw, bf) == (2, 0) and b"leaves" in _lib.lib.af_last_error()
    r[2, 0] = (0, 5, H - 10, 11, 20, 0, 0, 0)
    assert _plan(d, r, 8, _store())[0] == -1 and b"leaves" in _lib.lib.af_last_error()
    r[2, 0] = (0, 5, H - 10, 10, 20, 0, 0, 0)
    assert _plan(d, r, 8, _store())[0] == 0


def test_rect_plan_names_the_window_and_frame_that_do_not_fit_the_canvas():
    rng = np.random.default_rng(3)
    desc, rects = _case(rng, 4, 6)
    rects["x"][2, 3] = desc["canvas_w"][2] - rects["iw"][2, 3] + 1
    rc, bw, bf, _ = _plan(desc, rects, 8, _store())
    assert rc == -1 and (bw, bf) == (2, 3)
    msg = _lib.lib.af_last_error().decode()
    assert "window 2 frame 3" in msg and "does not fit" in msg
    rects["x"][2, 3] = 0
    rects["y"][1, 0] = -1
    rc, bw, bf, _ = _plan(desc, rects, 8, _store())
    assert rc == -1 and (bw, bf) == (1, 0) and "window 1 frame 0" in _lib.lib.af_last_error().decode()


def test_rect_plan_wants_three_bytes_of_slack_only_behind_the_store():
    rng = np.random.default_rng(4)
    desc, rects = _case(rng, 2, 3)
    d = desc.copy()
    d["canvas_w"], d["canvas_h"] = 700, 400
    # rectangles that end with their frame, inside the store: the bytes behind them are the next frame's, no slack asked
    rects[0, 0] = (0, W - 5, H - 4, 4, 5, 0, 0, 0)
    rects[0, 1] = (N_FRAMES - 2, 0, 0, H, W, 0, 0, 0)
    frames_end = N_FRAMES * FRAME_BYTES
    assert _plan(d, rects, 8, _store(frames_end))[0] == 0
    rects[1, 2] = (N_FRAMES - 1, W - 1, H - 1, 1, 1, 0, 0, 0)     # the last pixel of the store
    for slack, want in ((3, 0), (2, -1), (0, -1)):
        rc = _plan(d, rects, 8, _store(frames_end + slack))[0]
        assert rc == want, slack
        if want:
            assert b"3 readable bytes" in _lib.lib.af_last_error()
    rects[1, 2] = (N_FRAMES - 1, W - 2, H - 1, 1, 1, 0, 0, 0)     # one pixel earlier: the frame's own last pixel is the slack
    assert _plan(d, rects, 8, _store(frames_end))[0] == 0
    assert _plan(d, rects, 8, _store(frames_end - 1))[0] == -1     # a store that does not hold its frames


def test_rect_plan_and_launch_refuse_bad_arguments_without_a_device():
    rng = np.random.default_rng(5)
    desc, rects = _case(rng, 2, 3)
    rc, _, _, table = _plan(desc, rects, 8, _store())
    assert rc == 0
    L = _lib.lib
    st = _store()
    args = lambda **k: [k.get("desc", desc.ctypes.data), k.get("rects", rects.ctypes.data), k.get("n", 2), k.get("clip", 3),  # noqa: E731
                        k.get("size", 8), k.get("store", C.byref(st)), k.get("table", table.ctypes.data),
                        k.get("table_bytes", table.nbytes), None, None]
    assert L.af_window_rects_plan_u8(*args()) == 0
    for bad in (dict(desc=None), dict(rects=None), dict(table=None), dict(store=None), dict(n=0), dict(n=_lib.WINDOW_MAX_BATCH + 1),
                dict(clip=0), dict(clip=_lib.ALIGN_MAX_FRAMES + 1), dict(size=0), dict(size=6), dict(size=_lib.WINDOW_MAX_SIZE + 4),
                dict(table_bytes=table.nbytes - 8), dict(store=C.byref(_store(row_pitch=PITCH - 1))),
                dict(store=C.byref(_store(frame_stride=FRAME_BYTES - 1))), dict(store=C.byref(_store(n_frames=0))),
                dict(store=C.byref(_store(row_pitch=1 << 31, frame_stride=1 << 40, store_bytes=1 << 50)))):
        assert L.af_window_rects_plan_u8(*args(**bad)) == -1, bad
        assert L.af_last_error()
    one = C.c_void_p(table.ctypes.data)
    assert L.af_warp_affine_window_rects_u8(None, one, 2, 3, 8, one, None) == -1 and b"null" in L.af_last_error()
    assert L.af_warp_affine_window_rects_u8(one, None, 2, 3, 8, one, None) == -1
    assert L.af_warp_affine_window_rects_u8(one, one, 2, 3, 8, None, None) == -1
    for n, clip, size in ((0, 3, 8), (65, 3, 8), (2, 0, 8), (2, 65, 8), (2, 3, 6), (2, 3, 1028)):
        assert L.af_warp_affine_window_rects_u8(one, one, n, clip, size, one, None) == -1, (n, clip, size)
    assert L.af_warp_affine_window_rects_u8(one, one, 2, 3, 8, C.c_void_p(table.ctypes.data + 2), None) == -1
