"""GPU: YUV 4:2:0 frames in, the same bytes and the same scores out.  af_yuv420_to_rgb_u8 (csrc/af_yuv.hip) against tests/yuv_ref.py
- the numpy restatement of OpenCV's integer conversion, pinned by tests/test_yuv_host.py and unpinned against cv2 itself, absent
here - byte for byte, and every entry point that takes a frame against its own run on the converted frames.  The network is the
shrunken synthetic I3D of tests/test_hip_live.py (f16, 8 frames of 64 x 64).

  launch        nv12 / nv21 / i420 / yv12 x bgr / rgb x sizes whose rows end in tails of 2, 4 and 6 pixels and start at byte addresses
                that are 2 mod 4 x tight and pitched planes (odd Y pitch, odd base address) x host and device-resident planes, into
                slot 1 of a three-slot store filled with a sentinel: slot 1 equals yuv_ref, slots 0 and 2 and the 16 slack bytes
                keep the sentinel
  cube          one 4096 x 4096 frame holds every (Y, U, V) once: equal to yuv_ref and to the cube sums tests/test_yuv_host.py
                pins, nv12 -> bgr and i420 -> rgb
  several       three frames of different size, format and order into three stores in one launch; AF_YUV_MAX_FRAMES + 1 frames make
                two launches
  put           FrameStore.put in three staging chunks
  LiveCall      a call stepped with YuvFrames (I420 host, then NV12 device-resident; a size change; the ring wraps) against a twin
                stepped with yuv_ref's arrays: frame_view bytes and every (tid, score); bgr, rgb, and on a side stream
  RealtimeCall  the scripted two-face call of tests/test_hip_realtime.py at 96 x 130 as I420 against its twin on the converted frames
  CallServer    two I420 host calls of different sizes, one NV12 device-resident call and one numpy call in one mapping against lone
                RealtimeCalls (books) and against a server fed the converted frames (scores, which depend on the batch the server
                pads to, as tests/test_hip_server.py says): one convert launch and one copy per tick, at most three waits
  VideoScorer   aligned_windows and score on YuvFrames equal those on the converted frames

Each equality test first asserts, on the twin alone, that the script produced its cases.
"""
import numpy as np
import pytest
import torch

import af_mi355x
import test_hip_live as TL
import test_hip_server as TS
import test_hip_video as TV
import yuv_ref as R
from af_mi355x import _lib, evaluator, frames as F, live
from af_mi355x.evaluator import get_crop_box

pytestmark = pytest.mark.gpu
CLIP, SIZE = TL.CLIP, TL.SIZE
SENTINEL = 0xA5
SIZES = [(2, 2), (2, 6), (4, 10), (6, 18), (2, 16), (2, 32), (34, 66), (18, 130)]      # tails of 2 and 6, rows at 2 mod 4
SIZES += [(6, 12), (4, 20)]                                     # a tail of 4 pixels behind the 8-pixel run this kernel has
FORMATS = ["nv12", "nv21", "i420", "yv12"]


def _packed(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)


def _frame(buf, h, w, fmt, layout="tight", device=None):
    """the YuvFrame of a packed buffer: its own views (tight), or copies of its planes inside wider arrays that start one byte in
    (odd base address, odd Y pitch); on `device` the same views of CUDA tensors"""
    if layout == "tight":
        return F.YuvFrame.from_packed(buf if device is None else torch.from_numpy(buf).to(device), h, w, fmt)
    y, u, v = R.split_packed(buf, h, w, fmt)

    def wide(plane, extra):
        rows, row = plane.shape
        out = np.full((rows, row + extra), 0x3C, np.uint8)
        out[:, 1:row + 1] = plane
        out = out if device is None else torch.from_numpy(out).to(device)
        return out[:, 1:row + 1]
    if F.FORMATS[fmt][0]:
        first, second = (v, u) if fmt == "nv21" else (u, v)
        return F.YuvFrame(fmt, wide(y, 3), uv=wide(np.stack([first, second], -1).reshape(h // 2, w), 5))
    return F.YuvFrame(fmt, wide(y, 3), u=wide(u, 2 + (w // 2) % 2), v=wide(v, 2 + (w // 2) % 2))


def _store(h, w, order, capacity=3):
    store = evaluator.FrameStore(torch.device("cuda", torch.cuda.current_device()), order)
    store.open((h, w, 3), capacity)
    store.dev.fill_(SENTINEL)
    assert store.dev.numel() == capacity * h * w * 3 + 16
    return store


# ---- the launch ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_launch_equals_the_restatement_and_writes_nothing_else(fmt, where):
    dev = torch.device("cuda", torch.cuda.current_device())
    conv = F.YuvConverter(dev)
    assert any((3 * w) % 4 == 2 for _, w in SIZES) and {w % 8 for _, w in SIZES} == {0, 2, 4, 6}
    n = 0
    for (h, w) in SIZES:
        for order in ("bgr", "rgb"):
            for layout in ("tight", "pitched"):
                buf = _packed(h, w, seed=h * 1000 + w)
                want = R.packed_to(buf, h, w, fmt, order)
                frame = _frame(buf, h, w, fmt, layout, dev if where == "device" else None)
                assert frame.on_device == (where == "device")
                if layout == "pitched":
                    assert frame.planes()[0][3] % 2 == 1 and (where == "host" or frame.y.data_ptr() % 2 == 1)
                store = _store(h, w, order)
                conv.convert([(frame, store, order, 1)])
                torch.cuda.synchronize()
                got = store.dev.cpu().numpy()
                fb = h * w * 3
                case = (fmt, where, h, w, order, layout)
                assert np.array_equal(got[fb:2 * fb].reshape(h, w, 3), want), (case, int((got[fb:2 * fb] != want.reshape(-1)).sum()))
                assert (got[:fb] == SENTINEL).all() and (got[2 * fb:] == SENTINEL).all() and got[2 * fb:].size == fb + 16, case
                n += 1
    assert conv.launches == n == 4 * len(SIZES) and conv.copies == (n if where == "host" else 0)


@pytest.fixture(scope="module")
def cube():
    """(Y, U, V planes of a 4096 x 4096 frame that holds every (Y, U, V) exactly once, yuv_ref's B, G, R image of it): block b of
    the 2048 x 2048 chroma grid has (U, V) = ((b >> 8) & 255, b & 255) and the four Y values 4 * (b >> 16) + {0, 1, 2, 3}"""
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    u, v = ((b >> 8) & 255).astype(np.uint8), (b & 255).astype(np.uint8)
    y = np.zeros((4096, 4096), np.uint8)
    base = (4 * (b >> 16)).astype(np.uint8)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = base, base + 1, base + 2, base + 3
    want = R.planes_to_bgr(y, u, v)
    assert want.reshape(-1, 3).sum(0, dtype=np.int64).tolist() == [2154640128, 2179469722, 2158595072]
    return y, u, v, torch.from_numpy(want)


@pytest.mark.parametrize("fmt,order", [("nv12", "bgr"), ("i420", "rgb")])
def test_the_whole_cube_in_one_launch(cube, fmt, order):
    y, u, v, want = cube
    dev = torch.device("cuda", torch.cuda.current_device())
    frame = F.YuvFrame.from_packed(torch.from_numpy(R.pack(y, u, v, fmt)).to(dev), 4096, 4096, fmt)
    store = _store(4096, 4096, order, capacity=1)
    conv = F.YuvConverter(dev)
    conv.convert([(frame, store, order, 0)])
    got = store.view(0)
    sums = got.reshape(-1, 3).sum(0, dtype=torch.int64).tolist()
    assert (sums if order == "bgr" else sums[::-1]) == [2154640128, 2179469722, 2158595072]
    want = want.to(dev)
    assert torch.equal(got, want if order == "bgr" else want.flip(-1))
    assert conv.launches == 1 and bool((store.dev[-16:] == SENTINEL).all())


def test_frames_of_different_size_format_and_order_share_a_launch():
    dev = torch.device("cuda", torch.cuda.current_device())
    cases = [(34, 66, "nv21", "bgr", 0, "host"), (18, 130, "i420", "rgb", 2, "device"), (4, 10, "yv12", "bgr", 1, "host")]
    jobs, singles, wants = [], [], []
    for h, w, fmt, order, slot, where in cases:
        buf = _packed(h, w, seed=w)
        wants.append(R.packed_to(buf, h, w, fmt, order))
        for out in (jobs, singles):
            out.append((_frame(buf, h, w, fmt, "pitched", dev if where == "device" else None), _store(h, w, order), order, slot))
    together, alone = F.YuvConverter(dev), F.YuvConverter(dev)
    together.convert(jobs)
    for job in singles:
        alone.convert([job])
    torch.cuda.synchronize()
    assert (together.launches, together.copies, alone.launches, alone.copies) == (1, 1, 3, 2)
    for (h, w, _, _, slot, _), a, b, want in zip(cases, jobs, singles, wants):
        assert torch.equal(a[1].dev, b[1].dev) and np.array_equal(a[1].view(slot).cpu().numpy(), want)
        rest = torch.cat([a[1].dev[:slot * h * w * 3], a[1].dev[(slot + 1) * h * w * 3:]])
        assert bool((rest == SENTINEL).all())


def test_more_frames_than_a_table_holds_make_two_launches():
    dev = torch.device("cuda", torch.cuda.current_device())
    n = _lib.YUV_MAX_FRAMES + 1
    store = _store(2, 2, "bgr", capacity=n)
    bufs = [_packed(2, 2, seed=k) for k in range(n)]
    conv = F.YuvConverter(dev)
    conv.convert([(F.YuvFrame.from_packed(b, 2, 2, "nv12"), store, "bgr", n - 1 - k) for k, b in enumerate(bufs)])
    torch.cuda.synchronize()
    assert conv.launches == 2 and conv.copies == 1
    got = store.view(0, n).cpu().numpy()
    for k, b in enumerate(bufs):
        assert np.array_equal(got[n - 1 - k], R.packed_to(b, 2, 2, "nv12")), k
    assert bool((store.dev[-16:] == SENTINEL).all())


def test_put_converts_in_staging_chunks(monkeypatch):
    h, w = 34, 66
    store = _store(h, w, "rgb", capacity=8)
    bufs = [_packed(h, w, seed=20 + k) for k in range(5)]
    monkeypatch.setattr(evaluator, "_STAGE_BYTES", 2 * h * w * 3 // 2 + 10)                       # two frames per chunk: 2 + 2 + 1
    store.put([F.YuvFrame.from_packed(b, h, w, "i420") for b in bufs], 2)
    torch.cuda.synchronize()
    assert store._yuv.launches == 3 and store._yuv.copies == 3 and store.uploaded_bytes == 5 * h * w * 3 // 2
    for k, b in enumerate(bufs):
        assert np.array_equal(store.view(2 + k).cpu().numpy(), R.packed_to(b, h, w, "i420", "rgb")), k
    assert bool((store.view(0, 2) == SENTINEL).all()) and bool((store.view(7) == SENTINEL).all())
    dev = torch.device("cuda", torch.cuda.current_device())
    store.put([F.YuvFrame.from_packed(torch.from_numpy(bufs[0]).to(dev), h, w, "i420")], 0)      # device-resident: nothing is sent
    assert store.uploaded_bytes == 5 * h * w * 3 // 2 and store._yuv.copies == 3
    assert np.array_equal(store.view(0).cpu().numpy(), R.packed_to(bufs[0], h, w, "i420", "rgb"))
    with pytest.raises(ValueError, match="all numpy arrays or all YuvFrame"):
        store.put([F.YuvFrame.from_packed(bufs[0], h, w, "i420"), np.zeros((h, w, 3), np.uint8)], 0)
    with pytest.raises(ValueError, match="for a store of"):
        store.put([F.YuvFrame.from_packed(_packed(4, 10, 1), 4, 10, "i420")], 0)


# ---- LiveCall ------------------------------------------------------------------------------------------------------------------------

LIVE_STEPS, LIVE_RING, LIVE_SWITCH, LIVE_RESIZE = 24, 14, 12, 16
LIVE_SHAPES = ((96, 130), (80, 112))                               # before and from step LIVE_RESIZE on


def _live_inputs():
    out = []
    for s in range(LIVE_STEPS):
        h, w = LIVE_SHAPES[s >= LIVE_RESIZE]
        out.append((h, w, _packed(h, w, seed=300 + s)))
    return out


def _live_call(order):
    return af_mi355x.LiveCall(TL._net(), clip_size=CLIP, size=SIZE, stride=2, ring_frames=LIVE_RING, drop_after=LIVE_RING - CLIP,
                              channel_order=order)


@pytest.fixture(scope="module")
def live_twin():
    """per channel order: the twin stepped with yuv_ref's arrays - per step its results and its frame"""
    script = TL._script(LIVE_STEPS, {1: 0, 2: 0}, seed=9)
    out = {}
    for order in ("bgr", "rgb"):
        call, rows = _live_call(order), []
        for s, (h, w, buf) in enumerate(_live_inputs()):
            frame = R.packed_to(buf, h, w, "i420" if s < LIVE_SWITCH else "nv12", order)
            rows.append((call.step(frame, script[s]), frame))
        out[order] = rows
    return script, out


def _step_live_with_yuv(order, script, twin):
    call = _live_call(order)
    dev = torch.device("cuda", torch.cuda.current_device())
    uploaded = 0
    for s, (h, w, buf) in enumerate(_live_inputs()):
        if s < LIVE_SWITCH:
            frame = F.YuvFrame.from_packed(buf, h, w, "i420")
            uploaded += h * w * 3 // 2
        else:                                                      # a decoder's output: made on the stream the step runs on
            frame = F.YuvFrame.from_packed(torch.from_numpy(buf).to(dev, non_blocking=True), h, w, "nv12")
        got = call.step(frame, script[s])
        want, ref_frame = twin[s]
        assert call._shape == (h, w, 3) and call.frame_idx == s
        assert torch.equal(call.frame_view(s).cpu(), torch.from_numpy(ref_frame)), (order, s)
        assert got == want, (order, s, got, want)
        assert call.uploaded_bytes == uploaded
    assert call._first == LIVE_RESIZE
    return call


def test_the_live_twin_produces_the_cases(live_twin):
    _, twins = live_twin
    for order, rows in twins.items():
        closes = [s for s, (results, _) in enumerate(rows) if results]
        assert closes == [7, 9, 11, 13, 15, 23], (order, closes)   # before the switch, across it, after the wrap (15), after the re-open
        assert all(sorted(t for t, _ in rows[s][0]) == [1, 2] and all(0.0 < sc < 1.0 for _, sc in rows[s][0]) for s in closes)
    assert LIVE_RING < LIVE_RESIZE and twins["bgr"][15][0] == twins["rgb"][15][0]
    assert not np.array_equal(twins["bgr"][0][1], twins["rgb"][0][1])


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_a_live_call_on_yuv_frames_equals_its_twin(live_twin, order):
    script, twins = live_twin
    _step_live_with_yuv(order, script, twins[order])


def test_a_live_call_on_yuv_frames_on_a_side_stream(live_twin):
    script, twins = live_twin
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _step_live_with_yuv("bgr", script, twins["bgr"])
    side.synchronize()


# ---- RealtimeCall --------------------------------------------------------------------------------------------------------------------

STEPS, DROP, STRIDE = TS.TICKS, TS.DROP, TS.STRIDE
RING = CLIP + DROP


def _yuv_script(shape, seed, blurry, face1, face2):
    """tests/test_hip_server.py's script of one call with frames that come from YUV: per tick the packed I420 buffer, yuv_ref's
    B, G, R frame of it and the YuNet rows of two faces.  Face 1 is blurry - its crop flat in Y, U and V - on the `blurry` ticks;
    face 2 walks into the self-view rectangle and back out"""
    H, W = shape
    (x1, y1, dx1, dy1), (x2, y2, dx2, dy2) = face1, face2
    rng = np.random.default_rng(seed)
    std = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
    out = []
    for s in range(STEPS):
        y, u, v = (rng.integers(0, 256, sh, dtype=np.uint8) for sh in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
        t = min(max(s - 8, 0), 8) if s < 22 else max(0, 8 - (s - 21))
        faces = [(x1 + dx1 * s, y1 + dy1 * s, 30, 34, 0.95), (x2 + dx2 * t, y2 + dy2 * t, 28, 32, 0.93)]
        rows = []
        for x, yy, w, h, sc in faces:
            j = rng.uniform(-0.3, 0.3, 4)
            x, yy, w, h = x + j[0], yy + j[1], w + j[2], h + j[3]
            lm = std * [w, h] + [x, yy] + rng.normal(0, 0.4, (5, 2))
            rows.append(np.concatenate([[x, yy, w, h], [sc + rng.uniform(-0.004, 0.004)], lm.ravel()]))
        rows = np.asarray(rows, dtype=np.float32)
        if s in blurry:
            bx1, by1, bx2, by2 = map(int, get_crop_box((H, W), [rows[0, 0], rows[0, 1], rows[0, 0] + rows[0, 2], rows[0, 1] + rows[0, 3]], scale=0.6))
            r0, r1, c0, c1 = max(0, by1 - 6) // 2, (by2 + 7) // 2, max(0, bx1 - 6) // 2, (bx2 + 7) // 2      # whole chroma blocks
            y[2 * r0:2 * r1, 2 * c0:2 * c1], u[r0:r1, c0:c1], v[r0:r1, c0:c1] = 100, 120, 140
        out.append((R.pack(y, u, v, "i420"), R.planes_to_bgr(y, u, v), rows))
    return out


def _in_order(bgr, order):
    return bgr if order == "bgr" else np.ascontiguousarray(bgr[..., ::-1])


def _books(c):
    return dict(purged=sorted(c.purged), state={t: dict(v) for t, v in c.state.items()}, clip_hist={t: list(v) for t, v in c.clip_hist.items()},
                running=sorted(c.running_scores), detections=None if c.detections is None else c.detections.copy(),
                last_boxes={t: np.array(b) for t, b in c.last_boxes.items()}, frame_idx=c.frame_idx)


def _same_books(got, want, scored=True):
    assert got["purged"] == want["purged"] and got["running"] == want["running"] and got["frame_idx"] == want["frame_idx"]
    assert np.array_equal(got["detections"], want["detections"]) and TS._same_boxes(got["last_boxes"], want["last_boxes"])
    if scored:
        assert got["state"] == want["state"] and got["clip_hist"] == want["clip_hist"]


def _realtime(det, order="bgr"):
    return af_mi355x.RealtimeCall(TL._net(), detector=det, clip_size=CLIP, size=SIZE, **TS._args(order))


def test_a_realtime_call_on_i420_frames_equals_its_twin():
    H, W = 96, 130
    script = _yuv_script((H, W), 4, range(10, 15), (14, 22, 0.5, 0.1), (50, 40, 5.0, 2.5))
    det = TS.StubDetector({"A": [(bgr, rows) for _, bgr, rows in script]})
    twin, rows = _realtime(det), []
    for _, bgr, _ in script:
        rows.append((twin.step(bgr), _books(twin)))
    closes = [s for s, (results, _) in enumerate(rows) if results]
    assert len(closes) >= 2 and any(s < RING for s in closes) and any(s >= RING for s in closes), closes     # across a ring wrap
    assert any(b["purged"] for _, b in rows) and any(v[1] < 5.0 for v in twin.host.q_hist[1])               # a purge; the gate said no
    call = _realtime(det)
    for s, (buf, bgr, _) in enumerate(script):
        got = call.step(F.YuvFrame.from_packed(buf, H, W, "i420"))
        assert torch.equal(call.call.frame_view(s).cpu(), torch.from_numpy(bgr))
        assert got == rows[s][0], (s, got, rows[s][0])
        _same_books(_books(call), rows[s][1])
        assert call.uploaded_bytes == (s + 1) * H * W * 3 // 2
    assert {t: list(v) for t, v in call.host.q_hist.items()} == {t: list(v) for t, v in twin.host.q_hist.items()}


# ---- CallServer ----------------------------------------------------------------------------------------------------------------------

#          frame size, channel order, how the frames arrive, seed, blurry ticks, face 1, face 2
SERVED = {"A": ((96, 130), "bgr", "i420 host", 4, range(10, 15), (14, 22, 0.5, 0.1), (50, 40, 5.0, 2.5)),
          "B": ((80, 112), "rgb", "i420 host", 6, range(13, 18), (8, 20, 0.25, 0.1), (52, 30, 2.5, 2.0)),
          "C": ((96, 130), "rgb", "nv12 device", 5, range(18, 23), (12, 24, 0.4, 0.1), (52, 38, 5.0, 2.5)),
          "D": ((96, 130), "bgr", "numpy", 7, range(12, 17), (13, 23, 0.45, 0.1), (51, 39, 5.0, 2.5))}
SERVED_OPENS = {"A": 0, "B": 5, "C": 0, "D": 0}
SERVED_ABSENT = {"A": (16, 17)}


def _serving(tick):
    return [n for n in SERVED if SERVED_OPENS[n] <= tick and tick not in SERVED_ABSENT.get(n, ())]


@pytest.fixture(scope="module")
def served():
    """the scripts, the stub detector that knows every converted frame, and per tick and call a lone RealtimeCall's results and
    books on the converted frames"""
    scripts = {n: _yuv_script(c[0], c[3], c[4], c[5], c[6]) for n, c in SERVED.items()}
    det = TS.StubDetector({n: [(_in_order(bgr, SERVED[n][1]), rows) for _, bgr, rows in scripts[n]] for n in SERVED})
    lone, own, ticks = {}, {n: 0 for n in SERVED}, []
    for tick in range(STEPS):
        row = {}
        for n in _serving(tick):
            if n not in lone:
                lone[n] = _realtime(det, SERVED[n][1])
            k = own[n]
            own[n] += 1
            row[n] = (k, lone[n].step(_in_order(scripts[n][k][1], SERVED[n][1])), _books(lone[n]))
        ticks.append(row)
    return scripts, det, ticks


def _served_frame(name, script_row, converted):
    (h, w), order, how = SERVED[name][:3]
    buf, bgr, _ = script_row
    if converted or how == "numpy":
        return _in_order(bgr, order)
    if how == "i420 host":
        return F.YuvFrame.from_packed(buf, h, w, "i420")
    y, u, v = R.split_packed(buf, h, w, "i420")
    dev = torch.device("cuda", torch.cuda.current_device())
    return F.YuvFrame.from_packed(torch.from_numpy(R.pack(y, u, v, "nv12")).to(dev), h, w, "nv12")


def test_the_served_scripts_produce_the_cases(served):
    _, _, ticks = served
    closes = [{n: len(r[1]) for n, r in row.items() if r[1]} for row in ticks]
    assert any(len(c) >= 2 for c in closes) and any(len(c) == 1 for c in closes), closes      # shared batches, and a call's own batch
    assert all(any(n in c for c in closes) for n in SERVED), closes                          # every way a frame arrives is scored
    assert any(r[1] and r[0] >= RING for row in ticks for r in row.values())                  # a close after a ring wrap
    assert any(r[2]["purged"] for row in ticks for r in row.values())
    assert all("A" not in ticks[t] for t in SERVED_ABSENT["A"]) and "B" not in ticks[4] and "B" in ticks[5]


def test_the_server_on_mixed_frames_equals_lone_calls_and_a_server_on_converted_frames(served):
    scripts, det, ticks = served
    servers = [af_mi355x.CallServer(TL._net(), detector=det, clip_size=CLIP, size=SIZE, **TS._args("bgr")) for _ in range(2)]
    mixed, plain = servers
    cids, uploaded = {}, {n: 0 for n in SERVED}
    per_pixel = {"i420 host": 1.5, "nv12 device": 0.0, "numpy": 3.0}
    for tick, row in enumerate(ticks):
        for n in SERVED:
            if SERVED_OPENS[n] == tick:
                cids[n] = mixed.open(channel_order=SERVED[n][1])
                assert plain.open(channel_order=SERVED[n][1]) == cids[n]
        names = list(row)
        got = mixed.step({cids[n]: _served_frame(n, scripts[n][row[n][0]], False) for n in names})
        want = plain.step({cids[n]: _served_frame(n, scripts[n][row[n][0]], True) for n in names})
        assert got == want and list(got) == [cids[n] for n in names], (tick, got, want)      # scores bit for bit, at the same batches
        closing = [n for n in names if row[n][1]]
        for n in names:
            k, results, books = row[n]
            c = mixed.call(cids[n])
            (h, w), order = SERVED[n][:2]
            assert torch.equal(c.call.frame_view(k).cpu(), torch.from_numpy(_in_order(scripts[n][k][1], order))), (tick, n)
            assert [t for t, _ in got[cids[n]]] == [t for t, _ in results], (tick, n)
            _same_books(_books(c), books, scored=False)                                       # a lone call's, whatever the batch
            _same_books(_books(c), _books(plain.call(cids[n])))
            if closing == [n]:                                                                # the batch a lone call pads to: its scores
                assert got[cids[n]] == results, (tick, n)
            uploaded[n] += int(h * w * per_pixel[SERVED[n][2]])
            assert c.uploaded_bytes == uploaded[n], (tick, n)
        st = mixed.stats.last
        n_yuv = sum(SERVED[n][2] != "numpy" for n in names)
        n_host = sum(SERVED[n][2] == "i420 host" for n in names)
        assert n_yuv >= 1 and st["convert"] == 1 and st["yuv_copies"] == (1 if n_host else 0) and st["wait"] <= 3, (tick, st)
        assert st["wait"] == plain.stats.last["wait"] and plain.stats.last["convert"] == 0     # the conversion needs no wait
        assert mixed.uploaded_bytes == sum(uploaded.values())
    assert mixed.stats.total["convert"] == STEPS and mixed.stats.total["yuv_copies"] == STEPS
    assert plain.uploaded_bytes == sum(3 * SERVED[n][0][0] * SERVED[n][0][1] for row in ticks for n in row)


# ---- VideoScorer ---------------------------------------------------------------------------------------------------------------------

def _video_frames(n, h, w, fmt, seed):
    bufs = [_packed(h, w, seed + k) for k in range(n)]
    return [F.YuvFrame.from_packed(b, h, w, fmt) for b in bufs], [R.packed_to(b, h, w, fmt, "rgb") for b in bufs]


def test_the_video_scorers_warp_on_yuv_frames():
    H, W = 360, 642                                                # tests/test_hip_video.py's 359 x 641, made even
    rng = np.random.default_rng(12)
    yuv, rgb = _video_frames(8, H, W, "nv12", 40)
    rects = [(0, 0, 150, 140), (30, 40, 200, 190), (300, 100, 460, 260), (W - 160, H - 130, W, H)]
    infos = [(None, TV._five(rng, r), None, np.array(r)) for r in rects]
    frame_ids = [4, 5, 6, 7]
    windows = evaluator.clip_windows(4, 4)
    vs = evaluator.VideoScorer(None, TL._net(), clip_size=4, size=SIZE, batch=4)
    want = vs.aligned_windows(rgb, frame_ids, infos, windows).cpu()
    assert bool(want.any()) and vs.uploaded_bytes == 8 * H * W * 3
    got = vs.aligned_windows(yuv, frame_ids, infos, windows).cpu()
    assert torch.equal(got, want) and vs.uploaded_bytes == 8 * H * W * 3 // 2
    assert np.array_equal(vs.source.view(7).cpu().numpy(), rgb[7])


def test_the_video_scorers_score_on_yuv_frames():
    shape, _, detections = TV._crossing_video(71, n_frames=12)
    H, W = shape[:2]
    yuv, rgb = _video_frames(12, H, W, "i420", 60)
    net = TL._net()
    vs = evaluator.VideoScorer(None, net, clip_size=CLIP, size=SIZE, batch=4)
    want = vs.score(rgb, detections=detections)
    assert len(want["tracks"]) == 2 and len(want["preds"]) == 2 * (12 - CLIP + 1) and vs.uploaded_bytes == 12 * H * W * 3
    got = vs.score(yuv, detections=detections)
    TV._same_result(got, want)
    assert got["spans"] == want["spans"] and vs.uploaded_bytes == 12 * H * W * 3 // 2
    small = evaluator.VideoScorer(None, net, clip_size=CLIP, size=SIZE, batch=4, frame_bytes=10 * H * W * 3 + 16)      # two segments
    cut = small.score(yuv, detections=detections)
    TV._same_result(cut, want)
    assert small.uploaded_bytes > 12 * H * W * 3 // 2
    with pytest.raises(ValueError, match="all numpy arrays or all YuvFrame"):
        vs.score([yuv[0]] + rgb[1:], detections=detections)
