"""GPU: captured bitmaps in, the same bytes and the same scores out.  af_capture_to_stores_u8 (csrc/af_capture.hip) against
tests/capture_ref.py - the numpy statement of the alpha drop, the crop and cv2.INTER_AREA, pinned by tests/test_capture_host.py and
unpinned against cv2 itself, absent here - byte for byte, and every entry point that takes a frame against its own run on the
statement's frames.  Every comparison is equality; there is no tolerance.  The network is the shrunken synthetic I3D of
tests/test_hip_live.py (f16, 8 frames of 64 x 64).

  launch        bgra / rgba / bgr / rgb x host and device sources x bgr and rgb stores x a tight bitmap and one that starts at an odd
                address with an odd pitch and a rect at (1, 1), one launch per case into slot 1 of a three-slot store filled with a
                sentinel: slot 1 equals the statement, slots 0 and 2 and the 16 slack bytes keep the sentinel.  The cases, h x w:
                COPY 3 x 5; AREA2 6 x 10 -> 3 x 5; BOX 6 x 9 -> 2 x 3, 4 x 12 -> 2 x 3 (kx 4, ky 2) and the tie case 3 x 4 -> 3 x 2
                (1, 2 -> 2 and 2, 3 -> 2: half to even); TABLE 5 x 7 -> 2 x 3, 8 x 8 -> 3 x 3, 11 x 13 -> 4 x 5, one whole axis
                7 x 12 -> 3 x 4, dw == w 7 x 6 -> 3 x 6, and 70 x 203 -> 26 x 75: 19 runs of 4 pixels per row, the last of 3 pixels,
                494 runs = two tiles of 256 with rows that straddle the tile boundary and a partial last tile; and, for the two
                forms of the kernel's table loop (at most 4 taps per column, unrolled; any number, a loop), 3 x 11 -> 2 x 2 (6 taps)
                and 2 x 37 -> 1 x 3 (13 taps, and a sum that lands on 105.5 exactly: one fused multiply-add turns the byte into
                105) next to the cases above (at most 4)
  several       64 frames of mixed size, mode, format, store, order and residence in one launch; 65 make two; 64 frames of 33 tiles
                each, more tiles than the launch's grid of 2048 workgroups
  put           FrameStore.put of captured frames equals put of the statement's arrays
  LiveCall      bgra bitmaps with a rect and a max_w that lands in TABLE mode against a twin stepped with the statement's frames:
                frame bytes, results and books, across the ring's wrap; bgr, rgb, and on a side stream
  RealtimeCall  the scripted two-face call as bgra bitmaps (rect, AREA2) against its twin on the statement's frames
  CallServer    a mapping of numpy, I420 YuvFrame and CapturedFrame calls (host bgra AREA2, device rgba COPY) against lone
                RealtimeCalls (books) and a server fed the converted frames (scores): one capture launch per tick

Each equality test first asserts, on the twin alone, that the script produced its cases.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import af_mi355x
import capture_ref as R
import quality_ref as Q
import test_hip_live as TL
import test_hip_server as TS
import test_hip_yuv as TY
from af_mi355x import _lib, evaluator, frames as F

pytestmark = pytest.mark.gpu
CLIP, SIZE = TL.CLIP, TL.SIZE
SENTINEL = 0xA5
#        h, w, dh, dw, mode
CASES = [(3, 5, 3, 5, "copy"), (6, 10, 3, 5, "area2"), (6, 9, 2, 3, "box"), (4, 12, 2, 3, "box"), (3, 4, 3, 2, "box"),
         (5, 7, 2, 3, "table"), (8, 8, 3, 3, "table"), (11, 13, 4, 5, "table"), (7, 12, 3, 4, "table"), (7, 6, 3, 6, "table"),
         (70, 203, 26, 75, "table"), (3, 11, 2, 2, "table"), (2, 37, 1, 3, "table")]
FORMATS = ["bgra", "rgba", "bgr", "rgb"]
_sources = {}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _source(h, w, seed=0):
    """(an h x w x 4 random bitmap, shared by every test that needs this size; the tie case has its worked values)"""
    key = (h, w, seed)
    if key not in _sources:
        px = np.random.default_rng(1000 * h + w + 7919 * seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
        if (h, w) == (3, 4) and seed == 0:
            px[..., 0], px[..., 1], px[..., 2] = [1, 2, 2, 3], [11, 12, 12, 13], [21, 22, 22, 23]
        px.setflags(write=False)
        _sources[key] = px
    return _sources[key]


def _wants(h, w, dh, dw, seed=0):
    """the statement's resize of the first three channels of `_source(h, w)`, computed once"""
    key = ("want", h, w, dh, dw, seed)
    if key not in _sources:
        out = R.area_resize(np.ascontiguousarray(_source(h, w, seed)[..., :3]), dw, dh)
        out.setflags(write=False)
        _sources[key] = out
    return _sources[key]


def _want(h, w, dh, dw, fmt, order, seed=0):
    small = _wants(h, w, dh, dw, seed)
    return small if order == R.FORMATS[fmt][1] else np.ascontiguousarray(small[..., ::-1])


def _frame(h, w, dh, dw, fmt, layout, device=None, seed=0):
    """the CapturedFrame of `_source(h, w)` in `fmt`: the bitmap itself (tight), or the bitmap as the rectangle at (1, 1) of a larger
    one that starts one byte into its buffer and has an odd row pitch; on `device` the same views of a CUDA tensor"""
    ch = R.FORMATS[fmt][0]
    px = _source(h, w, seed)[..., :ch]
    if layout == "tight":
        px = np.array(px)                                                            # a writable, contiguous copy
        return F.CapturedFrame(px if device is None else torch.from_numpy(px).to(device), fmt, size=(dw, dh))
    H, W = h + 2, w + 3
    pitch = W * ch + 1 + (W * ch) % 2                                                # odd
    buf = np.full(1 + H * pitch, 0x3C, np.uint8)
    big = np.lib.stride_tricks.as_strided(buf[1:], (H, W, ch), (pitch, ch, 1))
    big[1:1 + h, 1:1 + w] = px
    if device is not None:
        big = torch.from_numpy(buf).to(device)[1:].as_strided((H, W, ch), (pitch, ch, 1))
        assert big.data_ptr() % 2 == 1
    f = F.CapturedFrame(big, fmt, rect=(1, 1, 1 + w, 1 + h), size=(dw, dh))
    assert f.pitch % 2 == 1 and f.rect_shape == (h, w)
    return f


def _store(h, w, order, capacity=3):
    store = evaluator.FrameStore(_dev(), order)
    store.open((h, w, 3), capacity)
    store.dev.fill_(SENTINEL)
    assert store.dev.numel() == capacity * h * w * 3 + 16
    return store


# ---- the launch ----------------------------------------------------------------------------------------------------------------------

def test_the_cases_are_the_modes_they_are_meant_to_be():
    for h, w, dh, dw, m in CASES:
        assert R.mode(h, w, dh, dw) == m, (h, w, dh, dw)
    assert _wants(3, 4, 3, 2)[..., 0].tolist() == [[2, 2]] * 3                      # the tie case: 1.5 -> 2, 2.5 -> 2
    most = lambda s, d: max(sum(1 for t in Q.area_table(s, d) if t[0] == i) for i in range(d))
    assert [most(w, dw) for h, w, dh, dw, m in CASES if m == "table"] == [3, 4, 4, 3, 1, 4, 6, 13]   # the kernel's forms: <= 4, any
    runs = -(-75 // _lib.CAPTURE_RUN)
    assert runs == 19 and 75 % _lib.CAPTURE_RUN == 3 and _lib.CAPTURE_TILE % runs and _lib.CAPTURE_TILE < 26 * runs < 2 * _lib.CAPTURE_TILE


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_launch_equals_the_statement_and_writes_nothing_else(fmt, where):
    dev = _dev()
    conv = F.CaptureConverter(dev)
    n = 0
    for h, w, dh, dw, m in CASES:
        for order in ("bgr", "rgb"):
            for layout in ("tight", "pitched"):
                want = _want(h, w, dh, dw, fmt, order)
                frame = _frame(h, w, dh, dw, fmt, layout, dev if where == "device" else None)
                assert frame.on_device == (where == "device") and frame.shape == (dh, dw, 3)
                store = _store(dh, dw, order)
                conv.convert([(frame, store, order, 1)])
                torch.cuda.synchronize()
                got = store.dev.cpu().numpy()
                fb = dh * dw * 3
                case = (fmt, where, h, w, dh, dw, order, layout)
                assert np.array_equal(got[fb:2 * fb].reshape(dh, dw, 3), want), (case, int((got[fb:2 * fb] != want.reshape(-1)).sum()))
                assert (got[:fb] == SENTINEL).all() and (got[2 * fb:] == SENTINEL).all() and got[2 * fb:].size == fb + 16, case
                n += 1
    assert conv.launches == conv.copies == n == 4 * len(CASES)


def test_the_alpha_byte_never_reaches_a_result():
    h, w, dh, dw = 11, 13, 4, 5
    px = _source(h, w).copy()
    stores = []
    for flip in (0, 0xFF):
        other = px.copy()
        other[..., 3] ^= flip
        store = _store(dh, dw, "bgr")
        F.CaptureConverter(_dev()).convert([(F.CapturedFrame(other, "bgra", size=(dw, dh)), store, "bgr", 1)])
        stores.append(store)
    assert torch.equal(stores[0].dev, stores[1].dev) and np.array_equal(stores[0].view(1).cpu().numpy(), _want(h, w, dh, dw, "bgra", "bgr"))


def _mixed_jobs(n):
    """n jobs that cycle through the cases, the formats, both layouts, both orders and both residences; one store per (size, order)"""
    dev = _dev()
    slots, jobs, wants = {}, [], []
    for k in range(n):
        h, w, dh, dw, _ = CASES[k % len(CASES)]
        fmt, order, layout = FORMATS[(k // 3) % 4], ("bgr", "rgb")[(k // 2) % 2], ("tight", "pitched")[(k // 5) % 2]
        slots.setdefault((dh, dw, order), []).append(k)
        jobs.append([_frame(h, w, dh, dw, fmt, layout, dev if k % 3 == 1 else None, seed=k), (dh, dw, order), order, None])
        wants.append(_want(h, w, dh, dw, fmt, order, seed=k))
    stores = {key: _store(key[0], key[1], key[2], capacity=len(members) + 2) for key, members in slots.items()}
    for key, members in slots.items():
        for at, k in enumerate(reversed(members)):                                   # slots 1 .. : 0 and the last keep the sentinel
            jobs[k][1], jobs[k][3] = stores[key], 1 + at
    return [tuple(j) for j in jobs], wants, stores


@pytest.mark.parametrize("n,launches", [(_lib.CAPTURE_MAX_FRAMES, 1), (_lib.CAPTURE_MAX_FRAMES + 1, 2)])
def test_mixed_frames_share_launches(n, launches):
    jobs, wants, stores = _mixed_jobs(n)
    assert len(stores) > 8 and {j[0].fmt for j in jobs} == set(FORMATS) and {j[0].on_device for j in jobs} == {False, True}
    conv = F.CaptureConverter(_dev())
    conv.convert(jobs)
    torch.cuda.synchronize()
    assert (conv.launches, conv.copies) == (launches, 1)
    for (frame, store, order, slot), want in zip(jobs, wants):
        assert np.array_equal(store.view(slot).cpu().numpy(), want), (frame.fmt, frame.rect_shape, frame.shape, order)
    for (dh, dw, _), store in stores.items():
        fb = dh * dw * 3
        assert bool((store.dev[:fb] == SENTINEL).all()) and bool((store.dev[(store.capacity - 1) * fb:] == SENTINEL).all())


BIG = [(66, 512), (132, 1024), (198, 1024), (100, 700)]          # h x w -> 66 x 512: COPY, AREA2, BOX (kx 2, ky 3), TABLE


def test_a_launch_of_more_tiles_than_workgroups():
    """64 frames of 128 runs x 66 rows = 33 tiles each into the 64 slots of one store: 2112 tiles for a grid of 2048 workgroups, so
    the first 64 workgroups take a second tile (the last two frames: BOX and TABLE)"""
    assert [R.mode(h, w, 66, 512) for h, w in BIG] == ["copy", "area2", "box", "table"] and (1024 // 512, 198 // 66) == (2, 3)
    store = _store(66, 512, "bgr", capacity=_lib.CAPTURE_MAX_FRAMES)
    jobs, wants = [], []
    for k in range(_lib.CAPTURE_MAX_FRAMES):
        (h, w), fmt, seed = BIG[k % 4], ("bgra", "rgb")[(k // 4) % 2], (k // 8) % 2
        jobs.append((_frame(h, w, 66, 512, fmt, "tight", seed=seed), store, "bgr", k))
        wants.append(_want(h, w, 66, 512, fmt, "bgr", seed=seed))
    frames = [j[0] for j in jobs]
    table = np.zeros(F.CaptureConverter.table_bytes(frames) // 8 + 1, np.int64)       # the planner alone, for the header it writes
    F.CaptureConverter.table(frames, [0x1000] * len(frames), [F.store_ref(store, "bgr")] * len(frames), list(range(len(frames))),
                             table.ctypes.data, table.nbytes)
    header = _lib.CaptureHeader.from_buffer_copy(table.tobytes()[:C.sizeof(_lib.CaptureHeader)])
    assert header.total_tiles == 64 * 33 > 2048                                      # the launch's grid, which _lib does not export
    conv = F.CaptureConverter(_dev())
    conv.convert(jobs)
    torch.cuda.synchronize()
    assert (conv.launches, conv.copies) == (1, 1)
    want = np.concatenate([np.stack(wants).reshape(-1), np.full(16, SENTINEL, np.uint8)])
    bad = np.flatnonzero(store.dev.cpu().numpy() != want)
    assert bad.size == 0, "%d bytes differ, the first at %d of slots of %d" % (bad.size, bad[0], 66 * 512 * 3)


def test_put_of_captured_frames_equals_put_of_the_statements_arrays(monkeypatch):
    h, w, dh, dw = 70, 203, 26, 75
    a, b = _store(dh, dw, "rgb", capacity=8), _store(dh, dw, "rgb", capacity=8)
    frames = [_frame(h, w, dh, dw, "bgra", ("tight", "pitched")[k % 2], seed=k) for k in range(5)]
    monkeypatch.setattr(evaluator, "_STAGE_BYTES", 2 * h * w * 4 + 10)             # two frames per chunk: 2 + 2 + 1
    a.put(frames, 2)
    b.put([_want(h, w, dh, dw, "bgra", "rgb", seed=k) for k in range(5)], 2)
    torch.cuda.synchronize()
    assert a._capture.launches == 3 and a._capture.copies == 3 and a.uploaded_bytes == 5 * h * w * 4 and a._yuv is None
    assert torch.equal(a.dev, b.dev) and bool((a.view(0, 2) == SENTINEL).all()) and bool((a.view(7) == SENTINEL).all())
    a.put([_frame(h, w, dh, dw, "rgb", "pitched", _dev(), seed=9)], 0)              # device-resident: no pixels are sent
    assert a.uploaded_bytes == 5 * h * w * 4 and np.array_equal(a.view(0).cpu().numpy(), _want(h, w, dh, dw, "rgb", "rgb", seed=9))
    with pytest.raises(ValueError, match="all numpy arrays or all YuvFrame or all CapturedFrame"):
        a.put([frames[0], np.zeros((dh, dw, 3), np.uint8)], 0)
    with pytest.raises(ValueError, match="for a store of"):
        a.put([_frame(5, 7, 2, 3, "bgra", "tight")], 0)


# ---- LiveCall ------------------------------------------------------------------------------------------------------------------------

LIVE_STEPS, LIVE_RING = 20, 14
LIVE_BITMAP, LIVE_RECT, LIVE_MAX_W = (160, 211), (3, 5, 206, 155), 130             # a 203 x 150 client area -> 130 x 96, TABLE


def _live_bitmaps():
    return [np.random.default_rng(500 + s).integers(0, 256, LIVE_BITMAP + (4,), dtype=np.uint8) for s in range(LIVE_STEPS)]


def _live_call(order):
    return af_mi355x.LiveCall(TL._net(), clip_size=CLIP, size=SIZE, stride=2, ring_frames=LIVE_RING, drop_after=LIVE_RING - CLIP,
                              channel_order=order)


def _live_books(call):
    return (call.frame_idx, sorted(call.purged), {tid: ([k for k, _ in tr.entries], tr.missed, tr.since_emit) for tid, tr in call._tracks.items()})


@pytest.fixture(scope="module")
def live_twin():
    """per channel order: the twin stepped with the statement's frames - per step its results, its books and its frame"""
    script = TL._script(LIVE_STEPS, {1: 0, 2: 0}, seed=9)
    dw, dh = R.capture_size(150, 203, LIVE_MAX_W)
    assert (dw, dh) == (130, 96) and R.mode(150, 203, dh, dw) == "table"
    out = {}
    for order in ("bgr", "rgb"):
        call, rows = _live_call(order), []
        for s, px in enumerate(_live_bitmaps()):
            frame = R.captured(px, "bgra", LIVE_RECT, dw, dh, order)
            rows.append((call.step(frame, script[s]), _live_books(call), frame))
        out[order] = rows
    return script, out


def _step_live_with_captures(order, script, twin):
    call = _live_call(order)
    for s, px in enumerate(_live_bitmaps()):
        frame = F.CapturedFrame(px, "bgra", rect=LIVE_RECT, max_w=LIVE_MAX_W)
        assert frame.shape == (96, 130, 3)
        got = call.step(frame, script[s])
        want, books, ref_frame = twin[s]
        assert call._shape == (96, 130, 3)
        assert torch.equal(call.frame_view(s).cpu(), torch.from_numpy(ref_frame)), (order, s)
        assert got == want, (order, s, got, want)
        assert _live_books(call) == books, (order, s)
        assert call.uploaded_bytes == (s + 1) * 150 * 203 * 4
    return call


def test_the_live_twin_produces_the_cases(live_twin):
    _, twins = live_twin
    for order, rows in twins.items():
        closes = [s for s, (results, _, _) in enumerate(rows) if results]
        assert len(closes) >= 4 and closes[0] < LIVE_RING and closes[-1] >= LIVE_RING + 2, (order, closes)     # before and after the ring's wrap
        assert all(sorted(t for t, _ in rows[s][0]) == [1, 2] and all(0.0 < sc < 1.0 for _, sc in rows[s][0]) for s in closes)
    assert twins["bgr"][15][0] == twins["rgb"][15][0] and not np.array_equal(twins["bgr"][0][2], twins["rgb"][0][2])


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_a_live_call_on_captured_frames_equals_its_twin(live_twin, order):
    script, twins = live_twin
    _step_live_with_captures(order, script, twins[order])


def test_a_live_call_on_captured_frames_on_a_side_stream(live_twin):
    script, twins = live_twin
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _step_live_with_captures("bgr", script, twins["bgr"])
    side.synchronize()


# ---- RealtimeCall and CallServer -------------------------------------------------------------------------------------------------------

STEPS, RING = TY.STEPS, TY.RING


def _bitmap(stored_bgr, fmt, how, seed, device=None):
    """a captured bitmap whose conversion is `stored_bgr` (B, G, R): the frame - every pixel doubled in both directions for "area2" -
    as the rectangle at (2, 1) of a larger bitmap of random bytes, alpha random"""
    ch, src_order = R.FORMATS[fmt]
    inner = stored_bgr if src_order == "bgr" else stored_bgr[..., ::-1]
    if how == "area2":
        inner = np.repeat(np.repeat(inner, 2, axis=0), 2, axis=1)
    h, w = inner.shape[:2]
    big = np.random.default_rng(seed).integers(0, 256, (h + 3, w + 5, ch), dtype=np.uint8)
    big[1:1 + h, 2:2 + w, :3] = inner
    H, W = stored_bgr.shape[:2]
    frame = F.CapturedFrame(big if device is None else torch.from_numpy(big).to(device), fmt, rect=(2, 1, 2 + w, 1 + h), max_w=W)
    assert frame.shape == (H, W, 3)
    return frame, big


def test_a_realtime_call_on_bgra_frames_equals_its_twin():
    H, W = 96, 130
    script = TY._yuv_script((H, W), 4, range(10, 15), (14, 22, 0.5, 0.1), (50, 40, 5.0, 2.5))
    det = TS.StubDetector({"A": [(bgr, rows) for _, bgr, rows in script]})
    twin, rows = TY._realtime(det), []
    for _, bgr, _ in script:
        rows.append((twin.step(bgr), TY._books(twin)))
    closes = [s for s, (results, _) in enumerate(rows) if results]
    assert len(closes) >= 2 and any(s < RING for s in closes) and any(s >= RING for s in closes), closes     # across a ring wrap
    assert any(b["purged"] for _, b in rows) and any(v[1] < 5.0 for v in twin.host.q_hist[1])               # a purge; the gate said no
    call = TY._realtime(det)
    for s, (_, bgr, _) in enumerate(script):
        frame, big = _bitmap(bgr, "bgra", "area2", s)
        if s == 0:
            assert np.array_equal(R.captured(big, "bgra", frame.rect, W, H, "bgr"), bgr) and R.mode(2 * H, 2 * W, H, W) == "area2"
        got = call.step(frame)
        assert torch.equal(call.call.frame_view(s).cpu(), torch.from_numpy(bgr))
        assert got == rows[s][0], (s, got, rows[s][0])
        TY._same_books(TY._books(call), rows[s][1])
        assert call.uploaded_bytes == (s + 1) * 4 * H * W * 4
    assert {t: list(v) for t, v in call.host.q_hist.items()} == {t: list(v) for t, v in twin.host.q_hist.items()}


#          frame size, channel order, how the frames arrive, seed, blurry ticks, face 1, face 2
SERVED = {"A": ((96, 130), "bgr", "bgra host area2", 4, range(10, 15), (14, 22, 0.5, 0.1), (50, 40, 5.0, 2.5)),
          "B": ((80, 112), "rgb", "i420 host", 6, range(13, 18), (8, 20, 0.25, 0.1), (52, 30, 2.5, 2.0)),
          "C": ((96, 130), "rgb", "rgba device copy", 5, range(18, 23), (12, 24, 0.4, 0.1), (52, 38, 5.0, 2.5)),
          "D": ((96, 130), "bgr", "numpy", 7, range(12, 17), (13, 23, 0.45, 0.1), (51, 39, 5.0, 2.5))}
SERVED_OPENS = {"A": 0, "B": 5, "C": 0, "D": 0}
SERVED_ABSENT = {"A": (16, 17)}


def _serving(tick):
    return [n for n in SERVED if SERVED_OPENS[n] <= tick and tick not in SERVED_ABSENT.get(n, ())]


@pytest.fixture(scope="module")
def served():
    """the scripts, the stub detector that knows every converted frame, and per tick and call a lone RealtimeCall's results and
    books on the converted frames"""
    scripts = {n: TY._yuv_script(c[0], c[3], c[4], c[5], c[6]) for n, c in SERVED.items()}
    det = TS.StubDetector({n: [(TY._in_order(bgr, SERVED[n][1]), rows) for _, bgr, rows in scripts[n]] for n in SERVED})
    lone, own, ticks = {}, {n: 0 for n in SERVED}, []
    for tick in range(STEPS):
        row = {}
        for n in _serving(tick):
            if n not in lone:
                lone[n] = TY._realtime(det, SERVED[n][1])
            k = own[n]
            own[n] += 1
            row[n] = (k, lone[n].step(TY._in_order(scripts[n][k][1], SERVED[n][1])), TY._books(lone[n]))
        ticks.append(row)
    return scripts, det, ticks


def _served_frame(name, script_row, converted, seed):
    """-> (the frame to hand the server, the bytes it uploads)"""
    (h, w), order, how = SERVED[name][:3]
    buf, bgr, _ = script_row
    if converted or how == "numpy":
        return TY._in_order(bgr, order), h * w * 3
    if how == "i420 host":
        return F.YuvFrame.from_packed(buf, h, w, "i420"), h * w * 3 // 2
    if how == "bgra host area2":
        return _bitmap(bgr, "bgra", "area2", seed)[0], 4 * h * w * 4
    return _bitmap(bgr, "rgba", "copy", seed, _dev())[0], 0


def test_the_served_scripts_produce_the_cases(served):
    _, _, ticks = served
    closes = [{n: len(r[1]) for n, r in row.items() if r[1]} for row in ticks]
    assert any(len(c) >= 2 for c in closes) and any(len(c) == 1 for c in closes), closes      # shared batches, and a call's own batch
    assert all(any(n in c for c in closes) for n in SERVED), closes                          # every way a frame arrives is scored
    assert any(r[1] and r[0] >= RING for row in ticks for r in row.values())                  # a close after a ring wrap
    assert any(r[2]["purged"] for row in ticks for r in row.values())


def test_the_server_on_mixed_frames_equals_lone_calls_and_a_server_on_converted_frames(served):
    scripts, det, ticks = served
    mixed, plain = [af_mi355x.CallServer(TL._net(), detector=det, clip_size=CLIP, size=SIZE, **TS._args("bgr")) for _ in range(2)]
    cids, uploaded = {}, {n: 0 for n in SERVED}
    for tick, row in enumerate(ticks):
        for n in SERVED:
            if SERVED_OPENS[n] == tick:
                cids[n] = mixed.open(channel_order=SERVED[n][1])
                assert plain.open(channel_order=SERVED[n][1]) == cids[n]
        names = list(row)
        handed = {n: _served_frame(n, scripts[n][row[n][0]], False, 100 * tick + len(n)) for n in names}
        got = mixed.step({cids[n]: handed[n][0] for n in names})
        want = plain.step({cids[n]: _served_frame(n, scripts[n][row[n][0]], True, 0)[0] for n in names})
        assert got == want and list(got) == [cids[n] for n in names], (tick, got, want)      # scores bit for bit, at the same batches
        closing = [n for n in names if row[n][1]]
        for n in names:
            k, results, books = row[n]
            c = mixed.call(cids[n])
            assert torch.equal(c.call.frame_view(k).cpu(), torch.from_numpy(TY._in_order(scripts[n][k][1], SERVED[n][1]))), (tick, n)
            assert [t for t, _ in got[cids[n]]] == [t for t, _ in results], (tick, n)
            TY._same_books(TY._books(c), books, scored=False)                                 # a lone call's, whatever the batch
            TY._same_books(TY._books(c), TY._books(plain.call(cids[n])))
            if closing == [n]:                                                                # the batch a lone call pads to: its scores
                assert got[cids[n]] == results, (tick, n)
            uploaded[n] += handed[n][1]
            assert c.uploaded_bytes == uploaded[n], (tick, n)
        st = mixed.stats.last
        n_cap = sum("bgra" in SERVED[n][2] or "rgba" in SERVED[n][2] for n in names)
        n_yuv = sum("i420" in SERVED[n][2] for n in names)
        assert n_cap >= 1 and st["capture"] == 1 and st["convert"] == (1 if n_yuv else 0) and st["wait"] <= 3, (tick, st)
        assert st["wait"] == plain.stats.last["wait"] and plain.stats.last["capture"] == 0    # the conversion needs no wait
        assert mixed.uploaded_bytes == sum(uploaded.values())
    assert mixed.stats.total["capture"] == STEPS and plain.stats.total["capture"] == 0
