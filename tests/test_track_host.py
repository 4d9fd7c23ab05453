"""CPU: the host side of the offline evaluator's clip loop (evaluator.py; reference altfreezing/demo.py:245-340).

  * clip_windows / get_crop_box / crop_records against tests/golden/track_windows.json, which tools/gen_track_golden.py recorded
    from the reference's own lines (demo.py:275-302 executed as they stand, test_tools/utils.py:13-24 imported);
  * af_window_batch_plan_u8 (the table of one window-batch warp launch) against a short restatement: offsets, canvases and paste
    positions, the inverted matrices bit for bit against oracle/aligner_oracle.invert_affine (OpenCV's order of operations, what
    the single-clip path computes), the error that names window and frame, refused arguments;
  * the per-video summary (video_score, frame_res) against the reference's loop written out here.
No device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import aligner_oracle as ao  # noqa: E402
from af_mi355x import _lib, evaluator  # noqa: E402


def test_clip_windows_equal_the_reference_lists():
    g = load_json("track_windows.json")
    assert sorted(int(t) for t in g["windows"]) == [1, 2, 3, 5, 16, 31, 32, 33, 40]
    for t, want in g["windows"].items():
        got = evaluator.clip_windows(int(t), g["clip_size"])
        assert got == want, t
        assert all(len(w) == g["clip_size"] for w in got)
    assert evaluator.clip_windows(0) == []
    assert evaluator.clip_windows(44) == [list(range(s, s + 32)) for s in range(13)]


def test_crop_records_equal_the_reference_boxes():
    g = load_json("track_windows.json")
    shape = tuple(g["frame_shape"])
    assert any(c["crop_box"][0] == 0 or c["crop_box"][1] == 0 or c["crop_box"][2] == shape[1] - 1 or c["crop_box"][3] == shape[0] - 1
               for c in g["crop_boxes"]), "no box clipped by the frame edge in the fixture"
    rng = np.random.default_rng(3)
    track = []
    for c in g["crop_boxes"]:
        box = np.array(c["box"])
        assert evaluator.get_crop_box(shape, box).tolist() == c["crop_box"]
        track.append((box, rng.uniform(0, 300, (5, 2)), rng.uniform(0, 300, (68, 2)), 0.9))
    recs = evaluator.crop_records(shape + (3,), track)
    assert len(recs) == len(track)
    for (big, info), c, face in zip(recs, g["crop_boxes"], track):
        assert big.tolist() == c["crop_box"] and len(info) == 4 and info[3] is big
        tl = np.array(c["crop_box"][:2], dtype=np.float64)
        np.testing.assert_array_equal(info[1], face[1] - tl)                 # demo.py:252-256
        np.testing.assert_array_equal(info[2], face[2] - tl)
        np.testing.assert_array_equal(info[0], (face[0].reshape(2, 2) - tl).reshape(-1))


# ---- the launch table ------------------------------------------------------------------------------------------------------

FRAME = np.dtype([("offset", "<i8"), ("ih", "<i4"), ("iw", "<i4"), ("x", "<i4"), ("y", "<i4")])
WINDOW = np.dtype([("tfm", "<f8", (6,)), ("canvas_h", "<i4"), ("canvas_w", "<i4")])


def test_table_structs_match_the_header():
    assert C.sizeof(_lib.AlignFrame) == FRAME.itemsize == 24
    assert C.sizeof(_lib.WindowDesc) == WINDOW.itemsize == 56
    assert _lib.lib.af_window_batch_table_bytes(16, 32) == _lib.WINDOW_TABLE_HEADER + 16 * 48 + 16 * 32 * 24
    for bad in ((0, 32), (_lib.WINDOW_MAX_BATCH + 1, 32), (16, 0), (16, _lib.ALIGN_MAX_FRAMES + 1)):
        assert _lib.lib.af_window_batch_table_bytes(*bad) == 0


def _case(rng, n_windows, clip_size, track_len):
    """stride-1 windows over a pool of `track_len` crops, each window with its own transform, canvas and paste offsets"""
    ih, iw = rng.integers(20, 60, track_len), rng.integers(20, 60, track_len)
    offs = np.concatenate([[0], np.cumsum((ih * iw * 3 + 15) // 16 * 16)])
    desc, frames = np.zeros(n_windows, dtype=WINDOW), np.zeros((n_windows, clip_size), dtype=FRAME)
    for w in range(n_windows):
        idx = np.arange(w, w + clip_size) % track_len
        px, py = rng.integers(0, 9, clip_size), rng.integers(0, 9, clip_size)
        ang, sc = rng.uniform(-0.5, 0.5), rng.uniform(0.3, 2.0)
        desc[w] = ([sc * np.cos(ang), -sc * np.sin(ang), rng.uniform(-20, 20), sc * np.sin(ang), sc * np.cos(ang), rng.uniform(-20, 20)],
                   int((py + ih[idx]).max()), int((px + iw[idx]).max()))
        frames["offset"][w], frames["ih"][w], frames["iw"][w], frames["x"][w], frames["y"][w] = offs[idx], ih[idx], iw[idx], px, py
    return desc, frames, int(offs[-1]) + 16


def _plan(desc, frames, size, pool_bytes, table=None):
    n, clip = frames.shape
    if table is None:
        table = np.zeros(_lib.lib.af_window_batch_table_bytes(n, clip) // 8, dtype=np.int64)       # 8-byte aligned
    bw, bf = C.c_int32(-7), C.c_int32(-7)
    rc = _lib.lib.af_window_batch_plan_u8(desc.ctypes.data, frames.ctypes.data, n, clip, size, pool_bytes, table.ctypes.data,
                                          table.nbytes, C.byref(bw), C.byref(bf))
    return rc, bw.value, bf.value, table


def _parse(table, n, clip):
    raw = table.view(np.uint8)
    head = raw[:16].view("<i4").tolist()
    mats = raw[16:16 + n * 48].view("<f8").reshape(n, 6)
    items = raw[16 + n * 48:16 + n * 48 + n * clip * 24].view(FRAME)
    return head, mats, items


@pytest.mark.parametrize("n_windows,clip_size,size", [(5, 4, 8), (16, 32, 224), (1, 1, 4)])
def test_plan_table_against_restatement(n_windows, clip_size, size):
    rng = np.random.default_rng(100 + n_windows)
    desc, frames, pool = _case(rng, n_windows, clip_size, n_windows + clip_size - 1)
    rc, bw, bf, table = _plan(desc, frames, size, pool)
    assert rc == 0 and (bw, bf) == (-1, -1), _lib.lib.af_last_error()
    head, mats, items = _parse(table, n_windows, clip_size)
    assert head == [n_windows, clip_size, size, 0]
    for w in range(n_windows):
        want = ao.invert_affine(desc["tfm"][w])                   # the single-clip path's inversion, same order of operations
        assert [float(v).hex() for v in mats[w]] == [float(v).hex() for v in want], w
    np.testing.assert_array_equal(items, frames.reshape(-1))      # work item k is (window k // clip_size, frame k % clip_size)


def test_plan_names_the_window_and_frame_of_a_crop_that_does_not_fit():
    rng = np.random.default_rng(5)
    desc, frames, pool = _case(rng, 4, 6, 9)
    frames["x"][2, 3] = desc["canvas_w"][2] - frames["iw"][2, 3] + 1          # one pixel over the right edge of window 2's canvas only
    rc, bw, bf, _ = _plan(desc, frames, 8, pool)
    assert rc == -1 and (bw, bf) == (2, 3)
    msg = _lib.lib.af_last_error().decode()
    assert "window 2 frame 3" in msg and "does not fit" in msg
    frames["x"][2, 3] = 0
    frames["y"][1, 0] = -1
    rc, bw, bf, _ = _plan(desc, frames, 8, pool)
    assert rc == -1 and (bw, bf) == (1, 0) and "window 1 frame 0" in _lib.lib.af_last_error().decode()


def test_plan_and_launch_refuse_bad_arguments_without_a_device():
    rng = np.random.default_rng(6)
    desc, frames, pool = _case(rng, 2, 3, 4)
    ok = _plan(desc, frames, 8, pool)
    assert ok[0] == 0
    table = ok[3]
    L = _lib.lib
    args = lambda **k: [k.get("desc", desc.ctypes.data), k.get("frames", frames.ctypes.data), k.get("n", 2), k.get("clip", 3),  # noqa: E731
                        k.get("size", 8), k.get("pool", pool), k.get("table", table.ctypes.data),
                        k.get("table_bytes", table.nbytes), None, None]
    assert L.af_window_batch_plan_u8(*args()) == 0                                # bad_window / bad_frame are optional
    for bad in (dict(desc=None), dict(frames=None), dict(table=None), dict(n=0), dict(n=_lib.WINDOW_MAX_BATCH + 1), dict(clip=0),
                dict(clip=_lib.ALIGN_MAX_FRAMES + 1), dict(size=0), dict(size=6), dict(size=_lib.WINDOW_MAX_SIZE + 4),
                dict(table_bytes=table.nbytes - 8), dict(pool=0)):
        assert L.af_window_batch_plan_u8(*args(**bad)) == -1, bad
        assert L.af_last_error()
    # a crop that ends less than 3 bytes before the end of the pool (the kernel reads tap pairs as 6 bytes), or starts before it
    last = int((frames["offset"] + frames["ih"].astype(np.int64) * frames["iw"] * 3).max())
    assert L.af_window_batch_plan_u8(*args(pool=last + 3)) == 0
    assert L.af_window_batch_plan_u8(*args(pool=last + 2)) == -1 and b"leaves the pool" in L.af_last_error()
    f2 = frames.copy()
    f2["offset"][0, 0] = -16
    assert L.af_window_batch_plan_u8(*args(frames=f2.ctypes.data)) == -1
    d2 = desc.copy()
    d2["canvas_w"][1] = 40000
    assert L.af_window_batch_plan_u8(*args(desc=d2.ctypes.data)) == -1 and b"canvas" in L.af_last_error()
    # the launch: every argument check comes before the device is touched
    one = C.c_void_p(table.ctypes.data)
    assert L.af_warp_affine_windows_u8(None, one, 2, 3, 8, one, None) == -1 and b"null" in L.af_last_error()
    assert L.af_warp_affine_windows_u8(one, None, 2, 3, 8, one, None) == -1
    assert L.af_warp_affine_windows_u8(one, one, 2, 3, 8, None, None) == -1
    for n, clip, size in ((0, 3, 8), (65, 3, 8), (2, 0, 8), (2, 65, 8), (2, 3, 6), (2, 3, 1028)):
        assert L.af_warp_affine_windows_u8(one, one, n, clip, size, one, None) == -1, (n, clip, size)
    assert L.af_warp_affine_windows_u8(one, one, 2, 3, 8, C.c_void_p(table.ctypes.data + 2), None) == -1      # misaligned output


# ---- the per-video summary ---------------------------------------------------------------------------------------------------

def test_summary_arithmetic_matches_the_reference_loop():
    """two tracks: 40 frames from frame 10 (9 windows) and 5 frames from frame 3 (one padded window that holds frames several
    times); made-up float32 scores; demo.py:304-340, 346-349 written out"""
    rng = np.random.default_rng(8)
    spans = [(10, 50), (3, 8)]
    clips, ids = [], []
    for ti, (start, end) in enumerate(spans):
        for w in evaluator.clip_windows(end - start, 32):
            clips.append([(ti, j) for j in w])
            ids.append([start + j for j in w])
    assert len(clips) == 10 and ids[-1].count(3 + 3) > 1
    scores = rng.uniform(0, 1, len(clips)).astype(np.float32)
    preds, frame_res = [], {}
    for frame_ids, s in zip(ids, scores):
        pred = float(s)
        for f_id in frame_ids:
            frame_res.setdefault(f_id, []).append(pred)
        preds.append(pred)
    video_score = float(np.mean(preds)) if len(preds) > 0 else 0.0
    for thr in (0.04, 0.99):
        got = evaluator.summarise(ids, scores, threshold=thr)
        assert got["video_score"] == video_score and got["pred_label"] == int(video_score > thr) and got["preds"] == preds
        assert set(got["frame_res"]) == set(frame_res) == set(range(10, 50)) | set(range(3, 8))
        for k, v in frame_res.items():
            assert got["frame_res"][k] == float(np.mean(v)), k
    # the padded window counts frame 6 as often as it holds it: its mean is that one score, frame 10 sees only window 0
    assert got["frame_res"][6] == preds[-1] and got["frame_res"][10] == preds[0]
    empty = evaluator.summarise([], [])
    assert empty["video_score"] == 0.0 and empty["pred_label"] == 0 and empty["preds"] == [] and empty["frame_res"] == {}
