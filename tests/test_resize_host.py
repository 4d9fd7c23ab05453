"""CPU: the host side of the resize path.  No device is touched.

  restatement  tests/resize_ref.py against hand-worked anchors - the restatement of OpenCV's resize.cpp is unpinned against cv2
               itself, which is absent here
  planner      af_resize_plan_u8: modes, addresses, pitches, the first_tile prefix; its coefficient tables equal the restatement's
               for seven (w, dw) pairs; jobs of one geometry share a table; every refusal, named through af_last_error, stamps
               the header
  scale_detect the reference's detect size, post_detect and check_valid, in resize_ref and in af_mi355x.retinaface
  ABI          af_version() stays 6, the header declares the entry points, _lib binds them
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resize_ref as R
from af_mi355x import _lib, retinaface as RF

L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def test_a_row_of_five_to_two_has_the_quarter_taps():
    # scale 2.5: fx = 0.5 * 2.5 - 0.5 = 0.75 -> sx 0, a = (512, 1536);  fx = 1.5 * 2.5 - 0.5 = 3.25 -> sx 3, a = (1536, 512)
    sx, a0, a1 = R.coefs(5, 2, True)
    assert sx.tolist() == [0, 3] and a0.tolist() == [512, 1536] and a1.tolist() == [1536, 512]
    row = np.array([[[0], [100], [7], [40], [200]]], np.uint8)                  # 1 x 5, one channel
    # one source row: sy = 0, both rows clip to it, b0 + b1 = 2048.  H = 100 * 1536 = 153600 and 40 * 1536 + 200 * 512 = 163840;
    # (2048 * (H >> 4)) >> 16 in two parts b0, b1: H = 153600 -> H >> 4 = 9600; fy = 0 -> b = (2048, 0): (2048 * 9600) >> 16 = 300,
    # (300 + 0 + 2) >> 2 = 75;  H = 163840 -> 10240 -> 320 -> 80
    assert R.resize_linear(row, 2, 1)[0, :, 0].tolist() == [75, 80]


def test_two_by_two_to_one_is_the_rounded_mean():
    img = np.array([[[1, 10, 255], [2, 20, 255]], [[3, 30, 255], [5, 41, 254]]], np.uint8)
    assert R.resize_linear(img, 1, 1).tolist() == [[[(1 + 2 + 3 + 5 + 2) >> 2, (10 + 20 + 30 + 41 + 2) >> 2, (255 * 3 + 254 + 2) >> 2]]]
    assert R.is_area2(2, 2, 1, 1) and R.is_area2(1920, 1080, 960, 540)


def test_an_upscale_clamps_at_both_ends():
    # 2 -> 4, scale 0.5: fx = -0.25, 0.25, 0.75, 1.25.  Columns: sx -1 -> (0, fx 0); 0, fx .25; 0, fx .75; sx 1 >= w - 1 -> (1, fx 0)
    sx, a0, a1 = R.coefs(2, 4, True)
    assert sx.tolist() == [0, 0, 0, 1] and a0.tolist() == [2048, 1536, 512, 2048] and a1.tolist() == [0, 512, 1536, 0]
    # rows keep fy: sy -1 with fy .75, and sy 1 with fy .25, whose second row 2 is clipped to 1
    sy, b0, b1 = R.coefs(2, 4, False)
    assert sy.tolist() == [-1, 0, 0, 1] and b0.tolist() == [512, 1536, 512, 1536] and b1.tolist() == [1536, 512, 1536, 512]
    img = np.array([[[0], [200]], [[100], [40]]], np.uint8)
    out = R.resize_linear(img, 4, 4)[..., 0]
    assert out[0].tolist() == [0, 50, 150, 200]          # rows -1 and 0 both clip to row 0: the weights add up to 2048
    assert out[3].tolist() == [100, 85, 55, 40]          # rows 1 and 2 both clip to row 1
    # row 1: fy .25 between rows 0 and 1; column 1: H0 = 200 * 512 = 102400, H1 = 100 * 1536 + 40 * 512 = 174080
    # ((1536 * 6400) >> 16) + ((512 * 10880) >> 16) + 2 = 150 + 85 + 2 = 237; >> 2 = 59
    assert out[1, 1] == 59 and out[1].tolist() == [25, 59, 126, 160]


def test_even_width_and_odd_height_is_bilinear_on_both_axes():
    assert not R.is_area2(24, 11, 12, 5) and not R.is_area2(32, 16, 8, 4) and not R.is_area2(24, 10, 12, 10)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (11, 24, 3), dtype=np.uint8)
    out = R.resize_linear(img, 12, 5)
    # x: scale exactly 2 -> fx = 2 dx + 0.5: taps (2 dx, 2 dx + 1) at 1024 / 1024;  y: scale 2.2 -> sy 0, 2, 5, 7, 9
    sx, a0, a1 = R.coefs(24, 12, True)
    assert sx.tolist() == list(range(0, 24, 2)) and set(a0.tolist()) == {1024} and set(a1.tolist()) == {1024}
    sy, b0, b1 = R.coefs(11, 5, False)
    assert sy.tolist() == [0, 2, 5, 7, 9] and b0.tolist() == [819, 410, 2048, 1638, 1229] and b1.tolist() == [1229, 1638, 0, 410, 819]
    s = img.astype(np.int64)
    h5 = (s[5, 0::2] + s[5, 1::2]) * 1024                                       # row 2 of the output is source row 5 alone
    assert np.array_equal(out[2], ((((2048 * (h5 >> 4)) >> 16) + 2) >> 2).astype(np.uint8))
    area = ((s[0:10:2, 0::2] + s[0:10:2, 1::2] + s[1:10:2, 0::2] + s[1:10:2, 1::2] + 2) >> 2).astype(np.uint8)
    assert not np.array_equal(out, area)                                         # what the 2 x 2 path would have given


def test_identity_is_a_copy_and_bad_input_is_refused():
    img = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    out = R.resize_linear(img, 7, 5)
    assert np.array_equal(out, img) and out is not img
    with pytest.raises(ValueError):
        R.resize_linear(img, 0, 0)
    with pytest.raises(ValueError):
        R.resize_linear(img.astype(np.float32), 3, 3)


def test_the_scale_is_one_over_the_inverse():
    assert R.scale_of(1920, 960) == 2.0 and R.scale_of(641, 320) == 1.0 / (320 / 641)
    differing = [(w, dw) for w in range(1, 200) for dw in range(1, 200) if R.scale_of(w, dw) != w / dw]
    assert differing, "1 / (dw / w) and w / dw differ in the last bit for some sizes: the restatement must use the first"


# ---- the planner -------------------------------------------------------------------------------------------------------------------

def _ref(base, n, h, w, pitch=None, bgr=0):
    pitch = 3 * w if pitch is None else pitch
    stride = h * pitch
    return _lib.StoreRef(base, _lib.FrameStore(n * stride, stride, pitch, n, h, w, 0), bgr, 0)


def _plan(jobs, refs, table_bytes=None, n=None):
    """-> (rc, table bytes as a numpy array, used)"""
    arr = (_lib.ResizeJob * max(1, len(jobs)))(*jobs)
    stores = (_lib.StoreRef * max(1, len(refs)))(*refs)
    n = len(jobs) if n is None else n
    need = L.af_resize_table_bytes(C.byref(arr), len(jobs)) if table_bytes is None else table_bytes
    buf = np.zeros(max(need, 8) // 8 + 1, np.int64)                             # 8-byte aligned
    used = C.c_int64(-7)
    rc = L.af_resize_plan_u8(C.byref(arr), n, C.byref(stores), len(refs), C.c_void_p(buf.ctypes.data), need, C.byref(used))
    return rc, buf.view(np.uint8), used.value


def _header(table):
    return _lib.ResizeHeader.from_buffer_copy(table[:C.sizeof(_lib.ResizeHeader)].tobytes())


def _item(table, i):
    lo = C.sizeof(_lib.ResizeHeader) + i * C.sizeof(_lib.ResizeItem)
    return _lib.ResizeItem.from_buffer_copy(table[lo:lo + C.sizeof(_lib.ResizeItem)].tobytes())


def _coefs(table, offset, n):
    raw = table[offset:offset + 8 * n].view(np.dtype([("idx", "<i4"), ("a0", "<i2"), ("a1", "<i2")]))
    return raw["idx"], raw["a0"], raw["a1"]


@pytest.mark.parametrize("w,dw", [(641, 320), (1920, 960), (3840, 960), (1920, 640), (7, 16), (1, 1), (1, 3)])
def test_the_planners_coefficients_equal_the_restatements(w, dw):
    # as columns (w -> dw, the height chosen so that the job is bilinear) and as rows (h = w -> dh = dw)
    h, dh = 5, 3
    rc, t, used = _plan([_lib.ResizeJob(0, 0, 0x2000, 3 * dw, dh, dw), _lib.ResizeJob(1, 0, 0x2000, 9, dw, 3)], [_ref(0x1000, 1, h, w), _ref(0x1000, 1, w, 4)])
    assert rc == 0, L.af_last_error()
    it = _item(t, 0)
    assert it.mode == _lib.RESIZE_LINEAR and (it.h, it.w, it.dh, it.dw) == (h, w, dh, dw)
    for got, want in zip(_coefs(t, it.xtab, dw), R.coefs(w, dw, True)):
        assert np.array_equal(got, want)
    for got, want in zip(_coefs(t, it.ytab, dh), R.coefs(h, dh, False)):
        assert np.array_equal(got, want)
    it = _item(t, 1)
    assert it.mode == _lib.RESIZE_LINEAR
    for got, want in zip(_coefs(t, it.ytab, dw), R.coefs(w, dw, False)):
        assert np.array_equal(got, want)
    assert used == _header(t).used_bytes <= t.size


def test_the_plan_of_mixed_jobs():
    refs = [_ref(0x10000, 4, 359, 641, pitch=1928), _ref(0x900000, 2, 16, 24, bgr=1), _ref(0xa00000, 1, 40, 64)]
    jobs = [_lib.ResizeJob(0, 3, 0x5000, 960, 179, 320), _lib.ResizeJob(1, 1, 0x6000, 40, 8, 12), _lib.ResizeJob(2, 0, 0x7000, 200, 40, 64),
            _lib.ResizeJob(0, 0, 0x8000, 961, 179, 320), _lib.ResizeJob(1, 0, 0x9000, 36, 5, 12)]
    rc, t, used = _plan(jobs, refs)
    assert rc == 0, L.af_last_error()
    hd = _header(t)
    assert (hd.kind, hd.n) == (_lib.RESIZE_KIND, 5)
    tiles = [-(-(dh * -(-dw // 4)) // 256) for dh, dw in ((179, 320), (8, 12), (40, 64), (179, 320), (5, 12))]
    assert list(hd.first_tile)[:6] == np.concatenate([[0], np.cumsum(tiles)]).tolist() and hd.total_tiles == sum(tiles)
    assert all(v == hd.total_tiles for v in list(hd.first_tile)[5:])
    items = [_item(t, i) for i in range(5)]
    assert [it.mode for it in items] == [_lib.RESIZE_LINEAR, _lib.RESIZE_AREA2, _lib.RESIZE_COPY, _lib.RESIZE_LINEAR, _lib.RESIZE_LINEAR]
    assert [it.src for it in items] == [0x10000 + 3 * 359 * 1928, 0x900000 + 16 * 72, 0xa00000, 0x10000, 0x900000]
    assert [it.dst for it in items] == [0x5000, 0x6000, 0x7000, 0x8000, 0x9000]
    assert [(it.src_pitch, it.dst_pitch, it.runs_x) for it in items] == [(1928, 960, 80), (72, 40, 3), (192, 200, 16), (1928, 961, 80), (72, 36, 3)]
    # jobs of one geometry share their tables; 16 -> 5 rows and 24 -> 12 columns get their own
    assert (items[0].xtab, items[0].ytab) == (items[3].xtab, items[3].ytab) and items[0].xtab != items[0].ytab
    base = C.sizeof(_lib.ResizeHeader) + 5 * C.sizeof(_lib.ResizeItem)
    assert sorted([items[0].xtab, items[0].ytab, items[4].xtab, items[4].ytab]) == [base, base + 8 * 320, base + 8 * (320 + 179), base + 8 * (320 + 179 + 12)]
    assert used == base + 8 * (320 + 179 + 12 + 5) == hd.used_bytes
    assert (items[1].xtab, items[1].ytab, items[2].xtab, items[2].ytab) == (0, 0, 0, 0)


def test_sixty_four_jobs_of_one_geometry_share_one_pair_of_tables():
    jobs = [_lib.ResizeJob(0, k, 0x100000 + k * 4096, 30, 4, 10) for k in range(64)]
    rc, t, used = _plan(jobs, [_ref(0x1000, 64, 9, 21)])
    assert rc == 0, L.af_last_error()
    assert len({(_item(t, i).xtab, _item(t, i).ytab) for i in range(64)}) == 1
    assert used == C.sizeof(_lib.ResizeHeader) + 64 * C.sizeof(_lib.ResizeItem) + 8 * 14
    assert L.af_resize_table_bytes(C.byref((_lib.ResizeJob * 64)(*jobs)), 64) == used + 63 * 8 * 14       # the bound assumes no sharing


REFUSALS = [
    ("65 frames", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30, 4, 10)] * 64, [_ref(0x1000, 1, 9, 21)], n=65)),
    ("names store 1 of 1", lambda: _plan([_lib.ResizeJob(1, 0, 0x2000, 30, 4, 10)], [_ref(0x1000, 1, 9, 21)])),
    ("names store -1 of 1", lambda: _plan([_lib.ResizeJob(-1, 0, 0x2000, 30, 4, 10)], [_ref(0x1000, 1, 9, 21)])),
    ("names frame 2 of store 0 of 2 frames", lambda: _plan([_lib.ResizeJob(0, 2, 0x2000, 30, 4, 10)], [_ref(0x1000, 2, 9, 21)])),
    ("names frame -1", lambda: _plan([_lib.ResizeJob(0, -1, 0x2000, 30, 4, 10)], [_ref(0x1000, 2, 9, 21)])),
    ("a destination of 0x4", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30, 4, 0)], [_ref(0x1000, 1, 9, 21)], table_bytes=4096)),
    ("a destination of 10x0", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30, 0, 10)], [_ref(0x1000, 1, 9, 21)], table_bytes=4096)),
    ("a destination of 8193x4", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30000, 4, 8193)], [_ref(0x1000, 1, 9, 21)], table_bytes=4096)),
    ("a destination of 10x8193", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30, 8193, 10)], [_ref(0x1000, 1, 9, 21)], table_bytes=4096)),
    ("destination pitch 29 is shorter than a row of 30 bytes", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 29, 4, 10)], [_ref(0x1000, 1, 9, 21)])),
    ("null destination", lambda: _plan([_lib.ResizeJob(0, 0, None, 30, 4, 10)], [_ref(0x1000, 1, 9, 21)])),
    ("null base pointer", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30, 4, 10)], [_ref(None, 1, 9, 21)])),
    ("row pitch 62", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30, 4, 10)], [_ref(0x1000, 1, 9, 21, pitch=62)])),
    ("the table needs 456 bytes, the buffer has 448", lambda: _plan([_lib.ResizeJob(0, 0, 0x2000, 30, 4, 10)], [_ref(0x1000, 1, 9, 21)], table_bytes=448)),
]


@pytest.mark.parametrize("text,call", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_planner_refuses(text, call):
    rc, t, used = call()
    assert rc == -1                                                             # AF_ERR_ARG
    assert text in L.af_last_error().decode(), L.af_last_error()
    assert _header(t).kind == -1 and used == 0                                  # stamped: no launch takes this table


def test_null_arguments_and_a_buffer_below_the_header_are_refused():
    jobs = (_lib.ResizeJob * 1)(_lib.ResizeJob(0, 0, 0x2000, 30, 4, 10))
    stores = (_lib.StoreRef * 1)(_ref(0x1000, 1, 9, 21))
    buf = np.zeros(128, np.int64)
    used = C.c_int64(0)
    for args in ((None, 1, C.byref(stores), 1, C.c_void_p(buf.ctypes.data), 1024, C.byref(used)),
                 (C.byref(jobs), 1, None, 1, C.c_void_p(buf.ctypes.data), 1024, C.byref(used)),
                 (C.byref(jobs), 1, C.byref(stores), 1, None, 1024, C.byref(used)),
                 (C.byref(jobs), 1, C.byref(stores), 1, C.c_void_p(buf.ctypes.data), 1024, None)):
        assert L.af_resize_plan_u8(*args) == -1 and b"null argument" in L.af_last_error()
    assert L.af_resize_plan_u8(C.byref(jobs), 1, C.byref(stores), 1, C.c_void_p(buf.ctypes.data), 100, C.byref(used)) == -1
    assert b"for its header alone" in L.af_last_error() and not buf.any()        # too small to stamp: left alone
    assert L.af_resize_plan_u8(C.byref(jobs), 1, C.byref(stores), 1, C.c_void_p(buf.ctypes.data + 4), 1024, C.byref(used)) == -1
    assert b"8-byte aligned" in L.af_last_error()
    assert L.af_resize_table_bytes(C.byref(jobs), 65) == -1 and L.af_resize_table_bytes(None, 1) == -1


def test_the_launch_refuses_on_the_host_before_any_device_call():
    assert L.af_resize_frames_u8(None, 1, None) == -1 and b"null table" in L.af_last_error()
    assert L.af_resize_frames_u8(C.c_void_p(0x1000), 65, None) == -1 and b"65 frames" in L.af_last_error()
    assert L.af_resize_frames_u8(C.c_void_p(0x1004), 1, None) == -1 and b"8-byte aligned" in L.af_last_error()
    assert L.af_resize_frames_u8(C.c_void_p(0x1000), 0, None) == 0               # nothing to do: no launch


# ---- scale_detect's host steps -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mod", [R, RF], ids=["resize_ref", "retinaface"])
def test_scale_detect_size(mod):
    assert mod.scale_detect_size(1080, 1920) == (960, 540) and mod.scale_detect_scale(1080, 1920) == 2
    assert mod.scale_detect_size(359, 641) == (320, 179)
    assert mod.scale_detect_size(2160, 3840) == (960, 540) and mod.scale_detect_scale(2160, 3840) == 4.0
    assert mod.scale_detect_size(1920, 1080) == (540, 960)
    assert mod.scale_detect_size(1, 1) == (0, 0)               # cv2.resize fails on it in the reference; scale_detect raises


def test_a_frame_too_small_to_halve_is_refused():
    det = RF.FaceDetector.__new__(RF.FaceDetector)             # no weights, no device: the size check comes first
    with pytest.raises(ValueError, match="1x1 .* 0x0"):
        det.scale_detect([np.zeros((1, 1, 3), np.uint8)])


def _face(box, pts, score=0.9):
    return np.array(box, np.float32), np.array(pts, np.float32).reshape(5, 2), np.float32(score)


@pytest.mark.parametrize("mod", [R, RF], ids=["resize_ref", "retinaface"])
def test_check_valid_and_post_detect(mod):
    pts = [[10, 10]] * 5
    ok = _face([5, 6, 20, 30], pts)
    assert mod.check_valid(ok, w=100, h=50)
    assert not mod.check_valid(_face([21, 6, 20, 30], pts), w=100, h=50)        # x1 > x2
    assert not mod.check_valid(_face([5, 31, 20, 30], pts), w=100, h=50)        # y1 > y2
    assert not mod.check_valid(_face([-0.5, 6, 20, 30], pts), w=100, h=50)      # below 0
    assert not mod.check_valid(_face([5, 6, 100, 30], pts), w=100, h=50)        # the bound itself is outside
    assert not mod.check_valid(_face([5, 6, 20, 50], pts), w=100, h=50)
    assert not mod.check_valid(_face([5, 6, 20, 30], [[10, 10]] * 4 + [[10, 50]]), w=100, h=50)
    assert not mod.check_valid(_face([5, 6, 20, 30], [[10, 10]] * 4 + [[-1, 10]]), w=100, h=50)
    assert mod.check_valid(_face([5, 5, 5, 5], pts), w=100, h=50)               # an empty box passes, as in the reference
    out = mod.post_detect([[ok, _face([5, 6, 60, 30], pts)], []], scale=2, w=100, h=100)
    assert [len(f) for f in out] == [1, 0]                                       # 60 * 2 = 120 leaves the frame
    box, ldm, score = out[0][0]
    assert box.dtype == np.float32 and ldm.dtype == np.float32 and box.tolist() == [10, 12, 40, 60] and ldm.shape == (5, 2) and score == ok[2]
    s = 2 * (2500 / 1920)                                                        # a float scale: still a float32 product
    box = mod.post_detect([[ok]], scale=s, w=1000, h=1000)[0][0][0]
    assert box.dtype == np.float32 and np.array_equal(box, ok[0] * np.float32(s))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------

def test_the_abi_version_stays_and_the_header_declares_the_entry_points():
    assert L.af_version() == 6 == _lib.AF_ABI_VERSION
    with open(os.path.join(ROOT, "include", "af_hip.h")) as f:
        text = f.read()
    for name in ("af_resize_table_bytes", "af_resize_plan_u8", "af_resize_frames_u8"):
        assert re.search(r"\b%s\(" % name, text) and name in _lib.ABI
    assert "#define AF_RESIZE_MAX_FRAMES 64" in text and _lib.RESIZE_MAX_FRAMES == 64
    assert "#define AF_RESIZE_MAX_SIDE %d" % _lib.RESIZE_MAX_SIDE in text
    assert C.sizeof(_lib.ResizeHeader) == 288 and C.sizeof(_lib.ResizeItem) == 56 and C.sizeof(_lib.ResizeCoef) == 8 and C.sizeof(_lib.ResizeJob) == 32
    from af_mi355x import build
    assert "af_resize.hip" in build.SOURCES
