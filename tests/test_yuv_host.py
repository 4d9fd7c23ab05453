"""CPU: the host side of the YUV 4:2:0 path.  No device is touched.

  restatement  tests/yuv_ref.py against hand-worked anchors and its channel sums over the whole 256^3 cube of (Y, U, V) - the
               restatement of OpenCV's integer code is unpinned against cv2 itself, which is absent here
  YuvFrame     what it refuses (odd sizes, dtype, pitch, strides, plane shapes, mixed host / device planes) and that from_packed
               takes views
  planner      af_yuv420_plan_u8: absolute addresses, pitches, flags and first_tile of a three-item table into three stores, and
               every refusal, named through af_last_error; the launch's own host checks refuse before any device call
  staging      pitched I420 and NV12 frames land as tight Y then chroma bytes
  ABI          af_version() stays 6, the header declares the entry points, _lib binds them
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import yuv_ref as R
from af_mi355x import _lib, frames as F

L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ANCHORS = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)),
           ((41, 240, 110), (255, 0, 0)), ((255, 255, 255), (255, 125, 255)), ((0, 0, 0), (0, 154, 0)), ((128, 0, 255), (0, 77, 255))]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def test_the_restatement_gives_the_anchors():
    for yuv, bgr in ANCHORS:
        assert tuple(int(c) for c in R.yuv_to_bgr(*[np.uint8(x) for x in yuv])) == bgr, yuv


def test_the_restatements_sums_over_the_whole_cube():
    g = np.arange(256, dtype=np.uint8)
    u, v = np.broadcast_to(g[:, None], (256, 256)), np.broadcast_to(g[None, :], (256, 256))
    total = np.zeros(3, dtype=np.int64)
    for y in range(256):
        total += R.yuv_to_bgr(np.full((256, 256), y, np.uint8), u, v).reshape(-1, 3).sum(0, dtype=np.int64)
    assert total.tolist() == [2154640128, 2179469722, 2158595072]


def test_the_packed_layouts_of_the_restatement_agree():
    rng = np.random.default_rng(3)
    y, u, v = rng.integers(0, 256, (4, 6), dtype=np.uint8), rng.integers(0, 256, (2, 3), dtype=np.uint8), rng.integers(0, 256, (2, 3), dtype=np.uint8)
    want = R.planes_to_bgr(y, u, v)
    assert np.array_equal(want[2:4, 4:6], np.broadcast_to(R.yuv_to_bgr(y[2:4, 4:6], u[1, 2], v[1, 2]), (2, 2, 3)))     # one (U, V) per block
    for fmt in F.FORMATS:
        buf = R.pack(y, u, v, fmt)
        assert buf.shape == (6, 6) and np.array_equal(R.packed_to(buf, 4, 6, fmt), want), fmt
        assert np.array_equal(R.packed_to(buf, 4, 6, fmt, "rgb"), want[..., ::-1])
    assert not np.array_equal(R.pack(y, u, v, "nv12"), R.pack(y, u, v, "nv21"))


# ---- YuvFrame ----------------------------------------------------------------------------------------------------------------------

def _planes(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def test_yuvframe_takes_the_four_formats():
    y, u, v = _planes(4, 6)
    for fmt in ("i420", "yv12"):
        f = F.YuvFrame(fmt, y, u=u, v=v)
        assert f.shape == (4, 6, 3) and not f.on_device and not f.interleaved and f.nbytes == f.upload_bytes == 36 and not f.swap_uv
    uv = np.stack([u, v], -1).reshape(2, 6)
    f = F.YuvFrame("nv12", y, uv=uv)
    assert f.shape == (4, 6, 3) and f.interleaved and not f.swap_uv and F.YuvFrame("nv21", y, uv=uv).swap_uv
    assert [(p.shape, rows, row, pitch) for p, rows, row, pitch in f.planes()] == [((4, 6), 4, 6, 6), ((2, 6), 2, 6, 6)]
    wide = np.zeros((4, 9), np.uint8)
    assert F.YuvFrame("nv12", wide[:, :6], uv=wide[:2, 3:]).planes()[0][3] == 9                      # a pitched view is fine
    assert F.upload_bytes(f) == 36 and F.upload_bytes(np.zeros((4, 6, 3), np.uint8)) == 72


def test_yuvframe_refuses_what_it_cannot_convert():
    y, u, v = _planes(4, 6)
    uv = np.zeros((2, 6), np.uint8)
    with pytest.raises(ValueError, match="format 'yuy2'"):
        F.YuvFrame("yuy2", y, u=u, v=v)
    with pytest.raises(ValueError, match="even height and width"):
        F.YuvFrame("nv12", np.zeros((3, 6), np.uint8), uv=uv)
    with pytest.raises(ValueError, match="even height and width"):
        F.YuvFrame("nv12", np.zeros((4, 5), np.uint8), uv=uv)
    with pytest.raises(ValueError, match="2-D uint8"):
        F.YuvFrame("nv12", y.astype(np.int16), uv=uv)
    with pytest.raises(ValueError, match="2-D uint8"):
        F.YuvFrame("nv12", y[None], uv=uv)
    with pytest.raises(ValueError, match="row pitch"):
        F.YuvFrame("nv12", np.lib.stride_tricks.as_strided(y, (4, 6), (3, 1)), uv=uv)           # rows overlap
    with pytest.raises(ValueError, match="row pitch"):
        F.YuvFrame("nv12", y[::-1], uv=uv)                                                         # negative row stride
    with pytest.raises(ValueError, match="element stride"):
        F.YuvFrame("nv12", np.zeros((4, 12), np.uint8)[:, ::2], uv=uv)
    with pytest.raises(ValueError, match="element stride"):
        F.YuvFrame("nv12", y[:, ::-1], uv=uv)
    with pytest.raises(ValueError, match="plane uv is 2 x 3"):
        F.YuvFrame("nv12", y, uv=u)
    with pytest.raises(ValueError, match="plane v is 2 x 2"):
        F.YuvFrame("i420", y, u=u, v=v[:, :2])
    with pytest.raises(ValueError, match="takes y and uv"):
        F.YuvFrame("nv12", y, u=u, v=v)
    with pytest.raises(ValueError, match="takes y, u and v"):
        F.YuvFrame("i420", y, uv=uv)
    with pytest.raises(ValueError, match="numpy arrays or CUDA tensors"):
        F.YuvFrame("nv12", y, uv=torch.zeros((2, 6), dtype=torch.uint8))                          # a CPU tensor is neither
    with pytest.raises(ValueError, match="numpy arrays or CUDA tensors"):
        F.YuvFrame("nv12", y.tolist(), uv=uv)
    meta = torch.zeros((2, 6), dtype=torch.uint8, device="meta")                                  # stands in for a device plane: no GPU here
    with pytest.raises(ValueError):
        F.YuvFrame("nv12", y, uv=meta)


def test_mixed_host_and_device_planes_are_refused(monkeypatch):
    """a CUDA tensor cannot be made without a device, so `_plane`'s verdict on the second plane is scripted"""
    real = F._plane
    monkeypatch.setattr(F, "_plane", lambda name, p: ((name == "uv"),) + real(name, p)[1:])
    with pytest.raises(ValueError, match="not mixed"):
        F.YuvFrame("nv12", np.zeros((4, 6), np.uint8), uv=np.zeros((2, 6), np.uint8))


def test_from_packed_shares_memory_with_its_buffer():
    h, w = 4, 6
    y, u, v = _planes(h, w, 1)
    for fmt in F.FORMATS:
        buf = R.pack(y, u, v, fmt)
        f = F.YuvFrame.from_packed(buf, h, w, fmt)
        for p, _, _, _ in f.planes():
            assert np.shares_memory(p, buf)
        assert np.array_equal(f.y, y)
        if f.interleaved:
            assert f.uv.shape == (2, 6) and f.swap_uv == (fmt == "nv21")
        else:
            assert np.array_equal(f.u, u) and np.array_equal(f.v, v) and not f.swap_uv       # named planes, whatever their order in memory
        buf[0, 0] ^= 255
        assert f.y[0, 0] == buf[0, 0]
    pitched = np.zeros((6, 9), np.uint8)[:, :6]
    assert F.YuvFrame.from_packed(pitched, 4, 6, "nv12").planes()[1][3] == 9
    with pytest.raises(ValueError, match="contiguous"):
        F.YuvFrame.from_packed(pitched, 4, 6, "i420")
    with pytest.raises(ValueError, match=r"\(6, 6\) array"):
        F.YuvFrame.from_packed(np.zeros((4, 6), np.uint8), 4, 6, "nv12")
    with pytest.raises(ValueError, match="even height and width"):
        F.YuvFrame.from_packed(np.zeros((9, 5), np.uint8), 6, 5, "nv12")


# ---- the planner -------------------------------------------------------------------------------------------------------------------

CAP = 7
BASES = (0x7000_0000_0000, 0x7100_0000_0100, 0x7200_0000_0040)


def _store(base, h, w, capacity=CAP, bgr=1, slack=16, pitch=None, stride=None):
    pitch = 3 * w if pitch is None else pitch
    stride = h * pitch if stride is None else stride
    return _lib.StoreRef(base, _lib.FrameStore(capacity * stride + slack, stride, pitch, capacity, h, w, 0), bgr, 0)


def _plan(descs, stores):
    d = (_lib.YuvFrameDesc * max(1, len(descs)))(*descs)
    s = (_lib.StoreRef * max(1, len(stores)))(*stores)
    items = (_lib.YuvItem * max(1, len(descs)))()
    return L.af_yuv420_plan_u8(C.byref(d), len(descs), C.byref(s), len(stores), C.byref(items)), items


def _tiles(h, w):
    return -(-((h // 2) * -(-w // _lib.YUV_RUN)) // _lib.YUV_TILE)


def _three():
    stores = [_store(BASES[0], 2, 2, bgr=1), _store(BASES[1], 4, 10, bgr=0), _store(BASES[2], 34, 66, bgr=1)]
    descs = [_lib.YuvFrameDesc(0x1000, 0x2000, None, 2, 2, 2, 2, 1, 0, 0, 0),                       # nv12 2 x 2 -> slot 0 of store 0
             _lib.YuvFrameDesc(0x3001, 0x4003, 0x5005, 13, 6, 4, 10, 0, 1, 1, 5),                   # yv12 order, pitched, -> slot 5 of store 1
             _lib.YuvFrameDesc(0x6000, 0x7000, None, 66, 80, 34, 66, 1, 1, 2, CAP - 1)]             # nv21 -> the last slot of store 2
    return descs, stores


def test_the_planner_fills_addresses_pitches_flags_and_the_tile_prefix():
    assert C.sizeof(_lib.YuvItem) == 56 and C.sizeof(_lib.YuvFrameDesc) == 64
    assert 8 + _lib.YUV_MAX_FRAMES * C.sizeof(_lib.YuvItem) <= 4096                              # the table travels as a kernel argument
    descs, stores = _three()
    rc, items = _plan(descs, stores)
    assert rc == 0, L.af_last_error()
    a, b, c = items[0], items[1], items[2]
    assert (a.y, a.c0, a.c1, a.dst) == (0x1000, 0x2000, None, BASES[0])
    assert (a.y_pitch, a.c_pitch, a.dst_pitch, a.h, a.w, a.interleaved, a.swap_uv, a.bgr) == (2, 2, 6, 2, 2, 1, 0, 1)
    assert (b.y, b.c0, b.c1, b.dst) == (0x3001, 0x4003, 0x5005, BASES[1] + 5 * 4 * 10 * 3)
    assert (b.y_pitch, b.c_pitch, b.dst_pitch, b.h, b.w, b.interleaved, b.swap_uv, b.bgr) == (13, 6, 30, 4, 10, 0, 1, 0)
    assert (c.y, c.c0, c.c1, c.dst) == (0x6000, 0x7000, None, BASES[2] + (CAP - 1) * 34 * 66 * 3)
    assert (c.y_pitch, c.c_pitch, c.dst_pitch, c.h, c.w, c.interleaved, c.swap_uv, c.bgr) == (66, 80, 198, 34, 66, 1, 1, 1)
    assert [it.first_tile for it in (a, b, c)] == [0, 1, 2] and [_tiles(2, 2), _tiles(4, 10), _tiles(34, 66)] == [1, 1, 1]
    # more than one tile per item: 130 x 64 is 65 x 8 = 520 runs = 3 tiles, 18 x 130 is 9 x 17 = 153 runs = 1 tile
    big = [_lib.YuvFrameDesc(0x1000, 0x2000, None, 64, 64, 130, 64, 1, 0, 0, 0), _lib.YuvFrameDesc(0x1000, 0x2000, None, 130, 130, 18, 130, 1, 0, 1, 1),
           _lib.YuvFrameDesc(0x1000, 0x2000, None, 64, 64, 130, 64, 1, 0, 0, 2)]
    rc, items = _plan(big, [_store(BASES[0], 130, 64), _store(BASES[1], 18, 130)])
    assert rc == 0 and [items[i].first_tile for i in range(3)] == [0, 3, 4] and (_tiles(130, 64), _tiles(18, 130)) == (3, 1)
    # a store with padded rows and frames: the pitch and stride are the store's
    rc, items = _plan([_lib.YuvFrameDesc(0x1000, 0x2000, None, 10, 10, 4, 10, 1, 0, 0, 2)], [_store(BASES[0], 4, 10, pitch=37, stride=160)])
    assert rc == 0 and items[0].dst == BASES[0] + 2 * 160 and items[0].dst_pitch == 37


def _refused(descs, stores, *words):
    rc, _ = _plan(descs, stores)
    msg = L.af_last_error()
    assert rc == -1, msg
    for w in words:
        assert w in msg, msg


def test_the_planner_refuses():
    descs, stores = _three()

    def changed(i, **kw):
        out = [_lib.YuvFrameDesc.from_buffer_copy(d) for d in descs]
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out
    _refused(changed(1, h=3), stores, b"frame 1", b"even")
    _refused(changed(2, w=65), stores, b"frame 2", b"even")
    _refused(changed(0, h=0), stores, b"frame 0", b"positive")
    _refused(changed(0, w=-2), stores, b"frame 0", b"positive")
    _refused(changed(1, y_pitch=9), stores, b"frame 1", b"Y pitch 9")
    _refused(changed(1, c_pitch=4), stores, b"frame 1", b"chroma pitch 4")
    _refused(changed(2, c_pitch=65), stores, b"frame 2", b"chroma pitch 65", b"row of 66")          # interleaved: a chroma row is w bytes
    _refused(changed(1, v=None), stores, b"frame 1", b"null plane")
    _refused(changed(1, store=3), stores, b"frame 1", b"store 3 of 3")
    _refused(changed(1, store=-1), stores, b"frame 1", b"store -1")
    _refused(changed(1, store=2), stores, b"frame 1", b"does not fit store 2")                     # another frame size
    _refused(changed(1, slot=CAP), stores, b"frame 1", b"slot 7 leaves store 1")
    _refused(changed(1, slot=-1), stores, b"frame 1", b"slot -1")
    # the destination must lie wholly inside the store's bytes: the last slot of a store that is one byte short
    short = list(stores)
    short[2] = _store(BASES[2], 34, 66, slack=-1)
    _refused(descs, short, b"frame 2", b"leaves store 2")
    rc, _ = _plan(changed(2, slot=CAP - 2), short)
    assert rc == 0
    short[2] = _store(BASES[2], 34, 66, pitch=197)
    _refused(descs, short, b"store 2", b"row pitch 197")
    short[2] = _lib.StoreRef(None, stores[2].desc, 1, 0)
    _refused(descs, short, b"store 2", b"null base")
    many = [descs[0]] * (_lib.YUV_MAX_FRAMES + 1)
    _refused(many, stores, b"65 frames", b"at most 64")
    rc, _ = _plan([descs[0]] * _lib.YUV_MAX_FRAMES, stores)
    assert rc == 0
    _refused(descs, [], b"0 stores")


def test_the_launch_checks_its_table_before_any_device_call():
    descs, stores = _three()
    rc, items = _plan(descs, stores)
    assert rc == 0
    assert L.af_yuv420_to_rgb_u8(C.byref(items), 0, None) == 0                                    # nothing to do, nothing launched
    assert L.af_yuv420_to_rgb_u8(None, 1, None) == -1 and b"null" in L.af_last_error()
    assert L.af_yuv420_to_rgb_u8(C.byref(items), _lib.YUV_MAX_FRAMES + 1, None) == -1 and b"at most 64" in L.af_last_error()
    for field, value, word in (("w", 9, b"even"), ("h", 0, b"positive"), ("y_pitch", 9, b"Y pitch"), ("c_pitch", 4, b"chroma pitch"),
                               ("dst_pitch", 29, b"destination pitch"), ("dst", None, b"null"), ("c1", None, b"null"), ("first_tile", 2, b"first_tile")):
        rc, items = _plan(descs, stores)
        setattr(items[1], field, value)
        assert L.af_yuv420_to_rgb_u8(C.byref(items), 3, None) == -1, field
        assert b"item 1" in L.af_last_error() and word in L.af_last_error(), L.af_last_error()


def test_the_python_table_is_the_planners():
    """YuvConverter.table: staged frames are tight planes behind one address, device-resident ones keep their own pitches"""
    y, u, v = _planes(4, 10, 2)
    wide = np.zeros((6, 13), np.uint8)
    i420, nv21 = F.YuvFrame("i420", y, u=u, v=v), F.YuvFrame("nv21", wide[:4, :10], uv=wide[4:, 3:])
    ref = _store(BASES[1], 4, 10, bgr=0)
    items = F.YuvConverter.table([i420, nv21, nv21], [0x9000, 0xa000, None], [ref, ref, ref], [0, 3, 6])
    a, b, c = items[0], items[1], items[2]
    assert (a.y, a.c0, a.c1, a.y_pitch, a.c_pitch, a.interleaved, a.swap_uv) == (0x9000, 0x9000 + 40, 0x9000 + 50, 10, 5, 0, 0)
    assert (b.y, b.c0, b.c1, b.y_pitch, b.c_pitch, b.interleaved, b.swap_uv) == (0xa000, 0xa000 + 40, None, 10, 10, 1, 1)
    base = wide.__array_interface__["data"][0]
    assert (c.y, c.c0, c.y_pitch, c.c_pitch) == (base, base + 4 * 13 + 3, 13, 13)
    assert [it.dst for it in (a, b, c)] == [BASES[1], BASES[1] + 3 * 120, BASES[1] + 6 * 120] and a.bgr == 0
    with pytest.raises(_lib.AfError, match="slot 7 leaves store"):
        F.YuvConverter.table([i420], [0x9000], [ref], [7])


# ---- staging -----------------------------------------------------------------------------------------------------------------------

def test_pitched_frames_are_staged_as_tight_planes(monkeypatch):
    h, w = 6, 10
    rng = np.random.default_rng(5)
    ybuf, ubuf, vbuf = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w + 3), (h // 2, w // 2 + 1), (h // 2, w // 2 + 1)))
    i420 = F.YuvFrame("i420", ybuf[:, :w], u=ubuf[:, :w // 2], v=vbuf[:, :w // 2])
    packed = rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)
    nv12 = F.YuvFrame.from_packed(packed, h, w, "nv12")
    offs, used = F.staged_offsets([i420, nv12])
    assert offs == [0, 96] and used == 96 + 90                                                    # 90 bytes each, the second on a 16-byte boundary
    want = np.full(used + 8, 0xEE, np.uint8)
    want[:90] = np.concatenate([ybuf[:, :w].reshape(-1), ubuf[:, :w // 2].reshape(-1), vbuf[:, :w // 2].reshape(-1)])
    want[96:186] = packed.reshape(-1)
    for split in (1 << 20, 1):                                                                    # whole planes; two bands on the copy threads
        monkeypatch.setattr(F, "_SPLIT_BYTES", split)
        out = np.full(used + 8, 0xEE, np.uint8)
        F.stage_planes(out.ctypes.data, [i420, nv12], offs, used)
        assert np.array_equal(out, want), split


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

def test_the_abi_stays_six_and_declares_the_yuv_entry_points():
    assert L.af_version() == 6 and _lib.AF_ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "af_hip.h")).read()
    for name in ("af_yuv420_plan_u8", "af_yuv420_to_rgb_u8"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.ABI and getattr(L, name).restype is C.c_int
    assert int(re.search(r"#define AF_YUV_MAX_FRAMES (\d+)", header).group(1)) == _lib.YUV_MAX_FRAMES == 64
    from af_mi355x import YuvFrame
    assert YuvFrame is F.YuvFrame
