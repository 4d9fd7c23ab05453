"""CPU: the host side of the captured-frame path.  No device is touched.

  statement    tests/capture_ref.py against anchors worked by hand here (a BOX whose sums land on .5, the same values through AREA2, a
               TABLE row with its fp32 weights) and against the already pinned quality_ref.half_size on every size of 1..9 x 1..9;
               capture_size against the reference's formula.  The statement is unpinned against cv2 itself, which is absent here
  CapturedFrame  the four formats, rect, max_w and size, and what it refuses
  planner      af_capture_plan_u8: struct sizes, the mode of one job of each kind, addresses, pitches, the swap flag, the area tables
               (indices and fp32 weights bit for bit quality_ref.area_table's, shared by jobs of one geometry), the tile prefix,
               every refusal with the stamped header; the launch entry refuses n > 64 before any device call
  staging      a pitched host frame with a rect lands as tight rows
  ABI          af_version() stays 6, the header declares the entry points, _lib binds them
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import capture_ref as R
import quality_ref as Q
import resize_ref as RS
from af_mi355x import _lib, frames as F

L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the statement -----------------------------------------------------------------------------------------------------------------

def _grey3(rows):
    """an HxWx3 image whose three channels are `rows`, `rows` + 10 and `rows` + 20"""
    a = np.asarray(rows, dtype=np.uint8)
    return np.stack([a, a + 10, a + 20], -1)


def test_a_box_whose_sums_land_on_a_half_rounds_to_even():
    img = _grey3([[1, 2, 2, 3]] * 3)                                                 # 4 x 3 -> 2 x 3: kx = 2, ky = 1
    assert R.mode(3, 4, 3, 2) == "box"
    # (1 + 2) * 0.5 = 1.5 -> 2 and (2 + 3) * 0.5 = 2.5 -> 2: half to even, not half up
    assert np.array_equal(R.area_resize(img, 2, 3), _grey3([[2, 2]] * 3))


def test_the_same_values_through_area2_round_half_up():
    img = _grey3([[1, 2, 2, 3]] * 2)                                                 # 4 x 2 -> 2 x 1
    assert R.mode(2, 4, 1, 2) == "area2"
    # (1 + 2 + 1 + 2 + 2) >> 2 = 2 and (2 + 3 + 2 + 3 + 2) >> 2 = 3
    assert np.array_equal(R.area_resize(img, 2, 1), _grey3([[2, 3]]))


def test_a_table_row_worked_with_its_fp32_weights():
    assert R.mode(1, 3, 1, 2) == "table"
    # 3 -> 2: scale 1.5; cell 0 = [0, 1.5): pixel 0 whole (1 / 1.5), half of pixel 1 (0.5 / 1.5); cell 1 = [1.5, 3): half of pixel 1, pixel 2
    w23, w13 = F32(1.0 / 1.5), F32(0.5 / 1.5)
    assert Q.area_table(3, 2) == [(0, 0, w23), (0, 1, w13), (1, 1, w13), (1, 2, F32(1.0 / 1.5))]
    assert Q.area_table(1, 1) == [(0, 0, F32(1.0))]
    a, b, c = 10, 20, 31
    left = F32(F32(F32(0) + F32(a) * w23) + F32(b) * w13)                           # 6.67 + 6.67
    right = F32(F32(F32(0) + F32(b) * w13) + F32(c) * w23)                          # 6.67 + 20.67
    want = [int(np.rint(F32(1.0) * left)), int(np.rint(F32(1.0) * right))]
    assert want == [13, 27]
    img = np.array([[[a, 0, 255], [b, 0, 255], [c, 0, 255]]], np.uint8)
    assert R.area_resize(img, 2, 1).tolist() == [[[13, 0, 255], [27, 0, 255]]]


def test_one_whole_axis_goes_through_both_tables():
    """7 x 12 -> 3 x 4: x is a whole ratio (3), y is not: the mode is the table's and x has a table of three taps of fp32(1 / 3) per
    cell, accumulated as fp32 products - not the integer box sum the BOX mode would take on x.  (At this size the two round alike on
    every image tried - a result is a multiple of 1 / 21 in exact arithmetic, never near a tie - so the path is pinned here, by the
    mode and the table, and by the planner's tests; the bytes are pinned against a fp64 evaluation.)"""
    assert R.mode(7, 12, 3, 4) == "table" and R.mode(6, 12, 3, 4) == "box"
    assert [t[:2] for t in Q.area_table(12, 4)] == [(d, 3 * d + k) for d in range(4) for k in range(3)]
    img = np.random.default_rng(0).integers(0, 256, (7, 12, 3), dtype=np.uint8)
    got = R.area_resize(img, 4, 3)
    assert got.shape == (3, 4, 3)
    # x by box sums in fp64, y by the table's weights in fp64: within one grey level of the fp32 table form everywhere
    ytab = Q.area_table(7, 3)
    exact = np.zeros((3, 4, 3))
    for dy, sy, beta in ytab:
        exact[dy] += float(beta) * img[sy].astype(np.float64).reshape(4, 3, 3).sum(1) / 3.0
    assert np.abs(got.astype(np.float64) - exact).max() <= 0.5 + 1e-3


def test_the_statement_at_half_size_is_the_pinned_half_size():
    rng = np.random.default_rng(1)
    modes = set()
    for h in range(1, 10):
        for w in range(1, 10):
            c = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            dw, dh = max(1, w // 2), max(1, h // 2)
            modes.add(R.mode(h, w, dh, dw))
            assert np.array_equal(R.area_resize(c, dw, dh), Q.half_size(c)), (h, w)
    assert modes == {"copy", "area2", "box", "table"}


def test_the_two_statements_of_the_2x2_mean_agree():
    """capture_ref's AREA2 and resize_ref's fast area path state one piece of device code (area2 in csrc/af_frame_runs.h)"""
    rng = np.random.default_rng(3)
    for (h, w), (dh, dw) in (((6, 10), (3, 5)), ((2, 2), (1, 1)), ((16, 24), (8, 12))):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert R.mode(h, w, dh, dw) == "area2" and RS.is_area2(w, h, dw, dh)
        assert np.array_equal(R.area_resize(img, dw, dh), RS.resize_linear(img, dw, dh)), (h, w)
    img = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    assert np.array_equal(R.area_resize(img, 5, 3), img) and np.array_equal(RS.resize_linear(img, 5, 3), img)


def test_capture_size_is_the_references_formula():
    for h, w, max_w in ((1440, 2560, 960), (1080, 1920, 960), (719, 1279, 960), (1001, 1999, 960)):
        want = (max_w, int(h * (max_w / w))) if max_w > 0 and w > max_w else (w, h)
        assert F.capture_size(h, w, max_w) == R.capture_size(h, w, max_w) == want, (h, w)
    assert F.capture_size(1440, 2560, 960) == (960, 540) and F.capture_size(1080, 1920, 960) == (960, 540)
    assert F.capture_size(719, 1279, 960) == (960, 539) and F.capture_size(1001, 1999, 960) == (960, 480)
    assert F.capture_size(719, 960, 960) == (960, 719) and F.capture_size(719, 1279, 0) == (1279, 719)


def test_captured_strips_crops_resizes_and_orders():
    px = np.random.default_rng(2).integers(0, 256, (6, 9, 4), dtype=np.uint8)
    got = R.captured(px, "bgra", (1, 2, 9, 6), 4, 2, "rgb")                          # 8 x 4 -> 4 x 2: area2
    want = R.area_resize(np.ascontiguousarray(px[2:6, 1:9, :3]), 4, 2)[..., ::-1]
    assert np.array_equal(got, want) and np.array_equal(R.captured(px, "rgba", (1, 2, 9, 6), 4, 2, "rgb"), want[..., ::-1])
    other = px.copy()
    other[..., 3] ^= 0xFF                                                            # alpha never enters
    assert np.array_equal(R.captured(other, "bgra", (1, 2, 9, 6), 4, 2, "rgb"), got)


# ---- CapturedFrame -----------------------------------------------------------------------------------------------------------------

def test_capturedframe_takes_the_four_formats():
    for fmt, ch, bgr in (("bgra", 4, True), ("rgba", 4, False), ("bgr", 3, True), ("rgb", 3, False)):
        f = F.CapturedFrame(np.zeros((6, 10, ch), np.uint8), fmt)
        assert f.shape == (6, 10, 3) and f.channels == ch and f.src_bgr == bgr and not f.on_device and f.device is None
        assert f.nbytes == f.upload_bytes == 6 * 10 * ch == F.upload_bytes(f) and f.pitch == 10 * ch and f.rect_shape == (6, 10)
        assert isinstance(f, F.ConvertedFrame) and f.converter is F.CaptureConverter
    wide = np.zeros((8, 50), np.uint8)
    pitched = np.lib.stride_tricks.as_strided(wide[:, 1:], (8, 12, 4), (50, 4, 1))       # odd address, pitch 50
    f = F.CapturedFrame(pitched, "bgra", rect=(1, 2, 11, 7), max_w=4)
    assert f.pitch == 50 and f.rect_shape == (5, 10) and f.shape == (2, 4, 3) and f.nbytes == 5 * 10 * 4
    (view, rows, row, pitch), = f.planes()
    assert (rows, row, pitch) == (5, 40, 50) and view.__array_interface__["data"][0] == wide.ctypes.data + 1 + 2 * 50 + 4
    assert F.CapturedFrame(pitched, "bgra", size=(12, 8)).shape == (8, 12, 3)
    assert F.CapturedFrame(pitched, "bgra", rect=(0, 0, 12, 8), size=(5, 3)).shape == (3, 5, 3)
    assert F.CapturedFrame(np.zeros((1440, 2560, 4), np.uint8), max_w=960).shape == (540, 960, 3)


def test_capturedframe_refuses_what_it_cannot_take():
    px = np.zeros((6, 10, 4), np.uint8)
    with pytest.raises(ValueError, match="format 'argb'"):
        F.CapturedFrame(px, "argb")
    with pytest.raises(ValueError, match="bgr pixels have 3 channels, the array has 4"):
        F.CapturedFrame(px, "bgr")
    with pytest.raises(ValueError, match="bgra pixels have 4 channels, the array has 3"):
        F.CapturedFrame(px[..., :3].copy(), "bgra")
    with pytest.raises(ValueError, match="3-D uint8"):
        F.CapturedFrame(px.astype(np.uint16))
    with pytest.raises(ValueError, match="3-D uint8"):
        F.CapturedFrame(px[0])
    with pytest.raises(ValueError, match="element stride"):
        F.CapturedFrame(np.zeros((6, 10, 8), np.uint8)[..., ::2])                    # a non-unit element stride
    with pytest.raises(ValueError, match="element stride"):
        F.CapturedFrame(px[..., ::-1])
    with pytest.raises(ValueError, match="pixel stride"):
        F.CapturedFrame(px[..., :3], "bgr")                                          # bgr bytes 4 apart: strip on the device instead
    with pytest.raises(ValueError, match="pixel stride"):
        F.CapturedFrame(px[:, ::2])
    with pytest.raises(ValueError, match="row pitch"):
        F.CapturedFrame(px[::-1])                                                    # bottom-up
    for rect in ((0, 0, 11, 6), (0, 0, 10, 7), (-1, 0, 10, 6), (4, 0, 4, 6), (0, 5, 10, 3)):
        with pytest.raises(ValueError, match=re.escape("rect (%d, %d, %d, %d) leaves the frame of 10 x 6" % rect)):
            F.CapturedFrame(px, rect=rect)
    with pytest.raises(ValueError, match=r"size 9 x 3 exceeds the rectangle of 8 x 4"):
        F.CapturedFrame(px, rect=(1, 1, 9, 5), size=(9, 3))                         # upscaling
    with pytest.raises(ValueError, match=r"size 8 x 5 exceeds the rectangle of 8 x 4"):
        F.CapturedFrame(px, rect=(1, 1, 9, 5), size=(8, 5))
    with pytest.raises(ValueError, match="stored size"):
        F.CapturedFrame(px, size=(0, 3))
    with pytest.raises(ValueError, match="CPU tensor"):
        F.CapturedFrame(torch.zeros((6, 10, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="numpy array or a CUDA tensor"):
        F.CapturedFrame(px.tolist())


class _FakeStore:
    """stands in for a FrameStore where no device exists: what a converter reads of one before it touches the device"""
    def __init__(self, shape):
        self.shape, self.device = shape, torch.device("cpu")


def test_mixed_lists_are_refused():
    from af_mi355x import evaluator
    cap = F.CapturedFrame(np.zeros((4, 6, 4), np.uint8))
    yuv = F.YuvFrame("nv12", np.zeros((4, 6), np.uint8), uv=np.zeros((2, 6), np.uint8))
    store = evaluator.FrameStore.__new__(evaluator.FrameStore)                      # put's check comes before any device work
    store._yuv = store._capture = None
    for frames in ([cap, np.zeros((4, 6, 3), np.uint8)], [np.zeros((4, 6, 3), np.uint8), cap], [cap, yuv], [yuv, cap]):
        with pytest.raises(ValueError, match="all numpy arrays or all YuvFrame or all CapturedFrame"):
            store.put(frames, 0)
    conv = F.CaptureConverter(torch.device("cpu"))
    with pytest.raises(ValueError, match="all numpy arrays or all YuvFrame or all CapturedFrame"):
        conv.convert([(cap, _FakeStore((4, 6, 3)), "bgr", 0), (yuv, _FakeStore((4, 6, 3)), "bgr", 1)])
    with pytest.raises(ValueError, match=r"a frame of \(4, 6, 3\) for a store of \(2, 3, 3\)"):
        conv.convert([(cap, _FakeStore((2, 3, 3)), "bgr", 0)])
    with pytest.raises(ValueError, match="all numpy arrays or all YuvFrame or all CapturedFrame"):
        F.YuvConverter(torch.device("cpu")).convert([(cap, _FakeStore((4, 6, 3)), "bgr", 0)])


# ---- the planner -------------------------------------------------------------------------------------------------------------------

CAP = 5
BASES = (0x7000_0000_0000, 0x7100_0000_0100, 0x7200_0000_0040, 0x7300_0000_0000, 0x7400_0000_0000)
SRC = 0x6000_0000_0000


def _store(base, h, w, capacity=CAP, bgr=1, slack=16, pitch=None, stride=None):
    pitch = 3 * w if pitch is None else pitch
    stride = h * pitch if stride is None else stride
    return _lib.StoreRef(base, _lib.FrameStore(capacity * stride + slack, stride, pitch, capacity, h, w, 0), bgr, 0)


def _plan(descs, stores, table_bytes=None, buf=None):
    d = (_lib.CaptureFrame * max(1, len(descs)))(*descs)
    s = (_lib.StoreRef * max(1, len(stores)))(*stores)
    need = L.af_capture_table_bytes(C.byref(d), len(descs))
    buf = np.full(max(need, 1 << 12) // 8 + 1, -1, np.int64) if buf is None else buf
    used = C.c_int64(-5)
    rc = L.af_capture_plan_u8(C.byref(d), len(descs), C.byref(s), len(stores), C.c_void_p(buf.ctypes.data),
                              buf.nbytes if table_bytes is None else table_bytes, C.byref(used))
    return rc, buf.view(np.uint8), used.value, need


def _header(table):
    return _lib.CaptureHeader.from_buffer_copy(table[:C.sizeof(_lib.CaptureHeader)].tobytes())


def _items(table, n):
    at = C.sizeof(_lib.CaptureHeader)
    return [_lib.CaptureItem.from_buffer_copy(table[at + i * C.sizeof(_lib.CaptureItem):at + (i + 1) * C.sizeof(_lib.CaptureItem)].tobytes())
            for i in range(n)]


def _area_table(table, offset, d):
    """the area table at `offset` as quality_ref.area_table lists it"""
    first = table[offset:offset + 4 * (d + 1)].view(np.int32)
    taps = offset + (4 * (d + 1) + 7) // 8 * 8
    out = []
    for i in range(d):
        for t in range(first[i], first[i + 1]):
            tap = _lib.CaptureTap.from_buffer_copy(table[taps + 8 * t:taps + 8 * t + 8].tobytes())
            out.append((i, tap.idx, F32(tap.weight)))
    return out, int(first[d])


def _same_table(got, want):
    return len(got) == len(want) and all(a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() for a, b in zip(got, want))


#        src, pitch, h, w, channels, src_bgr, store, slot, dh, dw
def _five():
    stores = [_store(BASES[0], 3, 5, bgr=1), _store(BASES[1], 3, 5, bgr=0), _store(BASES[2], 2, 3, bgr=1), _store(BASES[3], 26, 75, bgr=0),
              _store(BASES[4], 3, 6, bgr=1)]
    descs = [_lib.CaptureFrame(SRC + 0x1001, 37, 3, 5, 4, 1, 0, 0, 3, 5),          # COPY, bgra, odd address and pitch -> byte loads
             _lib.CaptureFrame(SRC + 0x2000, 40, 6, 10, 4, 1, 1, 4, 3, 5),         # AREA2, bgra into an rgb store -> swap, dword loads
             _lib.CaptureFrame(SRC + 0x3000, 36, 4, 12, 3, 0, 2, 2, 2, 3),         # BOX kx 4 ky 2, rgb into a bgr store -> swap
             _lib.CaptureFrame(SRC + 0x4000, 812, 70, 203, 4, 0, 3, 1, 26, 75),    # TABLE, rgba into an rgb store
             _lib.CaptureFrame(SRC + 0x5000, 24, 7, 6, 4, 1, 4, 3, 3, 6)]          # TABLE with dw == w
    return descs, stores


def test_the_structs_have_the_headers_sizes():
    assert C.sizeof(_lib.CaptureFrame) == 48 and C.sizeof(_lib.CaptureItem) == 72 and C.sizeof(_lib.CaptureTap) == 8
    assert C.sizeof(_lib.CaptureHeader) == 4 * (4 + 65 + 3) == 288


def test_the_planner_fills_modes_addresses_pitches_flags_tables_and_the_tile_prefix():
    descs, stores = _five()
    rc, table, used, need = _plan(descs, stores)
    assert rc == 0, L.af_last_error()
    hd, (a, b, c, d, e) = _header(table), _items(table, 5)
    assert (hd.kind, hd.n, hd.used_bytes) == (_lib.CAPTURE_KIND, 5, used) and 0 < used <= need
    assert [it.mode for it in (a, b, c, d, e)] == [_lib.CAPTURE_COPY, _lib.CAPTURE_AREA2, _lib.CAPTURE_BOX, _lib.CAPTURE_TABLE, _lib.CAPTURE_TABLE]
    assert [(it.src, it.src_pitch, it.channels) for it in (a, b, c, d, e)] == [(SRC + 0x1001, 37, 4), (SRC + 0x2000, 40, 4), (SRC + 0x3000, 36, 3),
                                                                              (SRC + 0x4000, 812, 4), (SRC + 0x5000, 24, 4)]
    assert [(it.dst, it.dst_pitch) for it in (a, b, c, d, e)] == [(BASES[0], 15), (BASES[1] + 4 * 45, 15), (BASES[2] + 2 * 18, 9),
                                                                  (BASES[3] + 26 * 225, 225), (BASES[4] + 3 * 54, 18)]
    assert [(it.h, it.w, it.dh, it.dw, it.runs_x) for it in (a, b, c, d, e)] == [(3, 5, 3, 5, 2), (6, 10, 3, 5, 2), (4, 12, 2, 3, 1),
                                                                                 (70, 203, 26, 75, 19), (7, 6, 3, 6, 2)]
    assert [it.swap for it in (a, b, c, d, e)] == [0, 1, 1, 0, 0]                 # the store's bgr against src_bgr
    assert [it.dword for it in (a, b, c, d, e)] == [0, 1, 0, 1, 1]                # 4 channels at a 4-aligned address and pitch
    assert [it.xk for it in (a, b, c, d, e)] == [0, 0, 0, 4, 1]                   # the most taps of one destination column
    assert (c.kx, c.ky) == (4, 2) and F32(c.inv_area).tobytes() == (F32(1.0) / F32(8)).tobytes()
    # the tile prefix: runs of 4 pixels, 256 runs per tile; 26 x 19 = 494 runs are 2 tiles
    tiles = [-(-(it.dh * it.runs_x) // _lib.CAPTURE_TILE) for it in (a, b, c, d, e)]
    assert tiles == [1, 1, 1, 2, 1] and list(hd.first_tile[:6]) == [0, 1, 2, 3, 5, 6] and hd.total_tiles == 6
    assert all(t == 6 for t in hd.first_tile[5:])
    # the area tables: quality_ref's, bit for bit, behind the items, each 8-aligned
    end = C.sizeof(_lib.CaptureHeader) + 5 * C.sizeof(_lib.CaptureItem)
    assert d.xtab == end and all(off % 8 == 0 for off in (d.xtab, d.ytab, e.xtab, e.ytab)) and (a.xtab, b.ytab, c.xtab) == (0, 0, 0)
    for off, s, dd in ((d.xtab, 203, 75), (d.ytab, 70, 26), (e.xtab, 6, 6), (e.ytab, 7, 3)):
        got, n_taps = _area_table(table, off, dd)
        want = Q.area_table(s, dd)
        assert n_taps == len(want) and _same_table(got, want), (s, dd)
    assert [t[1:] for t in _area_table(table, e.xtab, 6)[0]] == [(k, F32(1.0)) for k in range(6)]


def test_jobs_of_one_geometry_share_their_tables():
    descs, stores = _five()
    twice = descs + [_lib.CaptureFrame(SRC + 0x9000, 900, 70, 203, 3, 1, 3, 2, 26, 75),       # both tables of job 3
                     _lib.CaptureFrame(SRC + 0xa000, 900, 70, 6, 3, 1, 4, 0, 3, 6)]           # x of job 4, a new y table (70 -> 3)
    rc, table, used, _ = _plan(twice, stores)
    assert rc == 0, L.af_last_error()
    items = _items(table, 7)
    assert (items[5].xtab, items[5].ytab) == (items[3].xtab, items[3].ytab) and items[6].xtab == items[4].xtab
    assert items[6].ytab not in (items[3].ytab, items[4].ytab)
    got, _ = _area_table(table, items[6].ytab, 3)
    assert _same_table(got, Q.area_table(70, 3))
    rc, _, used_once, _ = _plan(descs, stores)
    extra = 7 * 72 - 5 * 72 + (4 * 4 + 8 * len(Q.area_table(70, 3)))
    assert used == used_once + extra


def _refused(descs, stores, *words, **kw):
    rc, table, used, _ = _plan(descs, stores, **kw)
    msg = L.af_last_error()
    assert rc == -1 and used == 0, msg
    assert _header(table).kind == -1, "a refused table is stamped"
    for w in words:
        assert w in msg, msg


def test_the_planner_refuses():
    descs, stores = _five()

    def changed(i, **kw):
        out = [_lib.CaptureFrame.from_buffer_copy(d) for d in descs]
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out
    _refused([descs[0]] * 65, stores, b"65 frames", b"at most 64")
    rc, _, _, _ = _plan([descs[0]] * 64, stores)
    assert rc == 0
    _refused(changed(1, h=0), stores, b"frame 1", b"every side 1 to 8192")
    _refused(changed(1, w=8193, pitch=40000), stores, b"frame 1", b"every side 1 to 8192")
    _refused(changed(1, dh=0), stores, b"frame 1", b"every side 1 to 8192")
    _refused(changed(1, dw=-3), stores, b"frame 1", b"every side 1 to 8192")
    _refused(changed(0, w=4, dw=5), stores, b"frame 0", b"upscaling")
    _refused(changed(0, h=2, dh=3), stores, b"frame 0", b"upscaling")
    _refused(changed(1, pitch=39), stores, b"frame 1", b"pitch 39", b"row of 40")
    _refused(changed(2, pitch=35), stores, b"frame 2", b"pitch 35", b"row of 36")
    _refused(changed(2, channels=2), stores, b"frame 2", b"2 channels")
    _refused(changed(2, channels=5, pitch=100), stores, b"frame 2", b"5 channels")
    _refused(changed(3, store=5), stores, b"frame 3", b"store 5 of 5")
    _refused(changed(3, store=-1), stores, b"frame 3", b"store -1")
    _refused(changed(3, slot=CAP), stores, b"frame 3", b"slot 5 leaves store 3")
    _refused(changed(3, slot=-1), stores, b"frame 3", b"slot -1")
    _refused(changed(1, store=2), stores, b"frame 1", b"does not fit store 2")                  # a store of another frame size
    _refused(changed(1, src=None), stores, b"frame 1", b"null source")
    bad = list(stores)
    bad[2] = _store(BASES[2], 2, 3, slack=-1)                                                  # the last slot is a byte short
    _refused(descs, bad, b"store 2", b"do not fit")
    bad[2] = _store(BASES[2], 2, 3, pitch=8)
    _refused(descs, bad, b"store 2", b"row pitch 8")
    bad[2] = _lib.StoreRef(None, stores[2].desc, 1, 0)
    _refused(descs, bad, b"store 2", b"null base")
    _refused(descs, [], b"0 stores")
    rc, _, used, _ = _plan(descs, stores)
    _refused(descs, stores, b"the table needs %d bytes" % used, table_bytes=used - 1)          # a short table buffer
    rc, _, again, _ = _plan(descs, stores, table_bytes=used)
    assert rc == 0 and again == used
    # null pointers: nothing to stamp without a table
    d = (_lib.CaptureFrame * 5)(*descs)
    s = (_lib.StoreRef * 5)(*stores)
    n = C.c_int64(0)
    buf = np.zeros(4096, np.int64)
    assert L.af_capture_plan_u8(C.byref(d), 5, C.byref(s), 5, None, 1 << 15, C.byref(n)) == -1 and b"null" in L.af_last_error()
    assert L.af_capture_plan_u8(C.byref(d), 5, C.byref(s), 5, C.c_void_p(buf.ctypes.data), buf.nbytes, None) == -1 and b"null" in L.af_last_error()
    assert L.af_capture_plan_u8(None, 5, C.byref(s), 5, C.c_void_p(buf.ctypes.data), buf.nbytes, C.byref(n)) == -1 and b"null" in L.af_last_error()
    assert buf.view(np.int32)[0] == -1
    buf[:] = 0
    assert L.af_capture_plan_u8(C.byref(d), 5, None, 5, C.c_void_p(buf.ctypes.data), buf.nbytes, C.byref(n)) == -1 and buf.view(np.int32)[0] == -1
    assert L.af_capture_table_bytes(None, 1) == -1 and L.af_capture_table_bytes(C.byref(d), 65) == -1
    up = (_lib.CaptureFrame * 1)(changed(0, w=4, dw=5)[0])
    assert L.af_capture_table_bytes(C.byref(up), 1) == -1


def test_the_launch_refuses_before_any_device_call():
    assert L.af_capture_to_stores_u8(None, 1, None) == -1 and b"null" in L.af_last_error()
    assert L.af_capture_to_stores_u8(C.c_void_p(0x1000), _lib.CAPTURE_MAX_FRAMES + 1, None) == -1 and b"at most 64" in L.af_last_error()
    assert L.af_capture_to_stores_u8(C.c_void_p(0x1004), 1, None) == -1 and b"8-byte aligned" in L.af_last_error()
    assert L.af_capture_to_stores_u8(C.c_void_p(0x1000), -1, None) == -1
    assert L.af_capture_to_stores_u8(C.c_void_p(0x1000), 0, None) == 0                          # nothing to do, nothing launched


def test_the_python_table_is_the_planners():
    """CaptureConverter.table: a staged frame is its tight rectangle behind one address, a device-resident one keeps its own pitch"""
    wide = np.zeros((8, 52), np.uint8)
    px = np.lib.stride_tricks.as_strided(wide, (8, 12, 4), (52, 4, 1))
    f = F.CapturedFrame(px, "bgra", rect=(1, 1, 11, 7), max_w=5)                              # 10 x 6 -> 5 x 3: area2
    g = F.CapturedFrame(px[:7, :6], "rgba", size=(6, 3))                                      # 6 x 7 -> 6 x 3: table
    assert f.shape == (3, 5, 3) and g.shape == (3, 6, 3)
    ref_a, ref_b = _store(BASES[1], 3, 5, bgr=0), _store(BASES[4], 3, 6, bgr=1)
    frames, addresses, refs, slots = [f, g, f], [0x9000, 0xa000, None], [ref_a, ref_b, ref_a], [0, 3, 4]
    room = F.CaptureConverter.table_bytes(frames)
    buf = np.zeros(room // 8 + 1, np.int64)
    used = F.CaptureConverter.table(frames, addresses, refs, slots, buf.ctypes.data, buf.nbytes)
    base = wide.ctypes.data
    descs = [_lib.CaptureFrame(0x9000, 40, 6, 10, 4, 1, 0, 0, 3, 5), _lib.CaptureFrame(0xa000, 24, 7, 6, 4, 0, 1, 3, 3, 6),
             _lib.CaptureFrame(base + 52 + 4, 52, 6, 10, 4, 1, 0, 4, 3, 5)]
    rc, want, want_used, need = _plan(descs, [ref_a, ref_b])
    assert rc == 0 and used == want_used <= room == need and np.array_equal(buf.view(np.uint8)[:used], want[:used])
    a, b, c = _items(buf.view(np.uint8), 3)
    assert (a.src, a.src_pitch, a.mode, a.swap, a.dword) == (0x9000, 40, _lib.CAPTURE_AREA2, 1, 1)
    assert (b.src, b.src_pitch, b.mode, b.swap) == (0xa000, 24, _lib.CAPTURE_TABLE, 1)
    assert (c.src, c.src_pitch, c.dst) == (base + 56, 52, BASES[1] + 4 * 45)
    with pytest.raises(_lib.AfError, match="slot 5 leaves store"):
        F.CaptureConverter.table([f], [0x9000], [ref_a], [5], buf.ctypes.data, buf.nbytes)
    assert buf.view(np.int32)[0] == -1


# ---- staging -----------------------------------------------------------------------------------------------------------------------

def test_a_pitched_frame_with_a_rect_is_staged_as_tight_rows(monkeypatch):
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 256, (9, 61), dtype=np.uint8)
    bgra = np.lib.stride_tricks.as_strided(wide[:, 1:], (9, 14, 4), (61, 4, 1))                # odd address, odd pitch
    bgr = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    f, g = F.CapturedFrame(bgra, "bgra", rect=(2, 1, 13, 8)), F.CapturedFrame(bgr, "bgr", rect=(1, 0, 6, 5))
    offs, used = F.staged_offsets([f, g])
    assert f.nbytes == 7 * 11 * 4 == 308 and offs == [0, 320] and used == 320 + 5 * 5 * 3     # the second on a 16-byte boundary
    want = np.full(used + 8, 0xEE, np.uint8)
    want[:308] = bgra[1:8, 2:13].reshape(-1)
    want[320:395] = bgr[:, 1:6].reshape(-1)
    for split in (1 << 20, 1):                                                                  # whole rectangles; two bands on the copy threads
        monkeypatch.setattr(F, "_SPLIT_BYTES", split)
        out = np.full(used + 8, 0xEE, np.uint8)
        F.stage_planes(out.ctypes.data, [f, g], offs, used)
        assert np.array_equal(out, want), split


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

def test_the_abi_stays_six_and_declares_the_capture_entry_points():
    assert L.af_version() == 6 and _lib.AF_ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "af_hip.h")).read()
    for name, res in (("af_capture_plan_u8", "int"), ("af_capture_to_stores_u8", "int"), ("af_capture_table_bytes", "int64_t")):
        assert re.search(r"\b%s %s\(" % (res, name), header) and name in _lib.ABI and hasattr(L, name)
    assert int(re.search(r"#define AF_CAPTURE_MAX_FRAMES (\d+)", header).group(1)) == _lib.CAPTURE_MAX_FRAMES == 64
    assert int(re.search(r"#define AF_CAPTURE_MAX_SIDE (\d+)", header).group(1)) == _lib.CAPTURE_MAX_SIDE
    assert int(re.search(r"#define AF_CAPTURE_KIND (0x[0-9a-f]+)", header).group(1), 16) == _lib.CAPTURE_KIND
    from af_mi355x import CapturedFrame
    assert CapturedFrame is F.CapturedFrame
