"""GPU: YUV frames of every built layout, depth and colour in, the statement's bytes and the same scores out.  af_yuv_to_rgb_ex_u8
(csrc/af_yuv_formats.hip) against tests/yuv_formats_ref.py - the numpy statement tests/test_yuv_formats_host.py pins - byte for byte,
and every entry point that takes a frame against its own run on the statement's converted frames.  The network is the shrunken
synthetic I3D of tests/test_hip_live.py (f16, 8 frames of 64 x 64).

  launch        per format x host / device planes: bgr and rgb stores x the sizes (w x h) 2 x 2, 6 x 4 (row 1 starts at byte 18), 10 x 6
                (a full run and a one-pair tail), 12 x 2 (a two-pair tail), 24 x 8, 26 x 6 and 30 x 4 (full runs and a one- and a
                three-pair tail), and 10 x 5 and 6 x 1 where chroma keeps its rows x planes that start 0 to 3 bytes (one sample at 16
                bits) into their buffer with pitches of row + 0, 1, 2, 7 samples, the four colours in turn: slot 1 of a three-slot
                store equals the statement, slots 0 and 2 and the slack keep the sentinel
  pitched       the C entry points on a store whose rows are 3 w + 5 bytes apart and whose slot starts at an odd byte: the rows
                equal the statement, the bytes between rows, before and behind the slot keep the sentinel
  cube          one 4096 x 4096 i444 frame holds every (Y, U, V) once, per (matrix, range); a 512 x 3698 frame holds the 10-bit
                lattice of tests/test_yuv_formats_host.py, as i010 and as p010
  old formats   the new launch on nv12 / nv21 / i420 / yv12 at the default colour equals af_yuv420_to_rgb_u8 byte for byte
  mixed         twelve frames of twelve formats, four sizes, both byte orders, all four colours, host and device planes into five
                stores (a store has one size and one order here, so four sizes cannot share three) in ONE launch of the new kernel
                and one copy; 65 frames make two launches; a batch of old-format default-colour frames makes the OLD launch
  end to end    LiveCall (host yuy2, then device full-range i422, a size change, the ring wraps), RealtimeCall on yuy2 and on
                full-range i422, a CallServer tick of nv12 + yuy2 + p010 + bt709-i420 calls (one conversion launch and at most one
                copy per tick), VideoScorer.score and VideoRunner.run on uyvy: frame bytes, books and scores bit for bit those on
                the statement's converted frames

Each equality test first asserts, on the twin alone, that the script produced its cases.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import af_mi355x
import test_hip_live as TL
import test_hip_runner as TR
import test_hip_server as TS
import test_hip_video as TV
import test_hip_yuv as TY
import yuv_formats_ref as X
from af_mi355x import _lib, evaluator, frames as F
from af_mi355x.evaluator import get_crop_box

pytestmark = pytest.mark.gpu
CLIP, SIZE = TL.CLIP, TL.SIZE
SENTINEL = 0xA5
SIZES = [(2, 2), (6, 4), (10, 6), (12, 2), (24, 8), (26, 6), (30, 4)]      # (w, h)
ODD_SIZES = [(10, 5), (6, 1)]                                               # where chroma is not halved vertically
VARIANTS = [(0, 0), (1, 1), (2, 2), (3, 7)]                                 # (samples the plane starts into its buffer, extra samples per row)
ALL = list(X.FORMATS)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _sizes(fmt):
    return SIZES + (ODD_SIZES if X.FORMATS[fmt][1] == 1 else [])


def _wide(plane, off, extra, device=None):
    """`plane` inside a buffer it starts `off` samples into (one sample at 16 bits), its rows `extra` samples longer; on `device` the
    same view of a CUDA tensor"""
    rows, cols = plane.shape
    off = min(off, 1) if plane.itemsize == 2 else off
    flat = np.full(off + rows * (cols + extra), 0x3C, plane.dtype)
    flat[off:].reshape(rows, cols + extra)[:, :cols] = plane
    if device is not None:
        flat = torch.from_numpy(flat).to(device)
    return flat[off:].reshape(rows, cols + extra)[:, :cols]


def _frame(planes, fmt, variant=(0, 0), device=None, **colour):
    off, extra = variant
    if (off, extra) == (0, 0):
        planes = [p if device is None else torch.from_numpy(p).to(device) for p in planes]
    else:
        planes = [_wide(p, off, extra, device) for p in planes]
    return F.YuvFrame(fmt, **X.kwargs(planes, fmt), **colour)


def _store(h, w, order, capacity=3):
    store = evaluator.FrameStore(_dev(), order)
    store.open((h, w, 3), capacity)
    store.dev.fill_(SENTINEL)
    assert store.dev.numel() == capacity * h * w * 3 + 16
    return store


class Counted:
    """counts the calls of the two conversion launches of the library"""

    def __init__(self, monkeypatch):
        self.old = self.new = 0
        old, new = _lib.lib.af_yuv420_to_rgb_u8, _lib.lib.af_yuv_to_rgb_ex_u8

        def call_old(*a):
            self.old += 1
            return old(*a)

        def call_new(*a):
            self.new += 1
            return new(*a)
        monkeypatch.setattr(_lib.lib, "af_yuv420_to_rgb_u8", call_old)
        monkeypatch.setattr(_lib.lib, "af_yuv_to_rgb_ex_u8", call_new)


# ---- the launch ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("fmt", ALL)
def test_one_launch_equals_the_statement_and_writes_nothing_else(fmt, where, monkeypatch):
    counted = Counted(monkeypatch)
    conv = F.YuvConverter(_dev())
    sizes = _sizes(fmt)
    assert {w % 8 for w, _ in sizes} == {0, 2, 4, 6} and (6, 4) in sizes
    cases = []
    for w, h in sizes:
        for order in ("bgr", "rgb"):
            for variant in VARIANTS:
                matrix, full = X.COLOURS[len(cases) % 4]
                if fmt in F.FORMATS and (matrix, full) == ("bt601", False):
                    matrix = "bt709"                                  # the default colour of an old format is the old launch's: below
                planes = X.random_planes(fmt, h, w, seed=1000 * h + w)
                want = X.convert(planes, fmt, matrix, full, order)
                frame = _frame(planes, fmt, variant, _dev() if where == "device" else None, matrix=matrix, full_range=full)
                assert frame.on_device == (where == "device") and frame.shape == (h, w, 3)
                if variant[1] and h > 1:
                    assert frame.planes()[0][3] == frame.planes()[0][2] + variant[1] * planes[0].itemsize
                    assert where == "host" or frame.y.data_ptr() % 4 == (2 if planes[0].itemsize == 2 else variant[0])
                store = _store(h, w, order)
                conv.convert([(frame, store, order, 1)])
                cases.append(((fmt, where, w, h, order, variant, matrix, full), store, want, frame))
    torch.cuda.synchronize()
    for case, store, want, _ in cases:
        got = store.dev.cpu().numpy()
        fb = want.size
        assert np.array_equal(got[fb:2 * fb].reshape(want.shape), want), (case, int((got[fb:2 * fb] != want.reshape(-1)).sum()))
        assert (got[:fb] == SENTINEL).all() and (got[2 * fb:] == SENTINEL).all() and got[2 * fb:].size == fb + 16, case
    n = len(cases)
    assert conv.launches == n == 8 * len(sizes) and conv.copies == (n if where == "host" else 0) and (counted.old, counted.new) == (0, n)


@pytest.mark.parametrize("fmt", ALL)
def test_a_pitched_store_keeps_the_bytes_between_its_rows(fmt):
    """through the C entry points: FrameStore's rows are tight, a caller's need not be"""
    dev = _dev()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    runs = []
    for k, (w, h) in enumerate(_sizes(fmt)):
        matrix, full = X.COLOURS[k % 4]
        bgr = k % 2
        planes = X.random_planes(fmt, h, w, seed=77 + k)
        want = X.convert(planes, fmt, matrix, full, "bgr" if bgr else "rgb")
        frame = _frame(planes, fmt, VARIANTS[1 + k % 3], dev, matrix=matrix, full_range=full)
        lead, pitch = 7 + k % 2, 3 * w + 5                        # slots that start at odd and at even bytes; rows of both in every slot
        stride = h * pitch + 3
        buf = torch.full((lead + 3 * stride + 16,), SENTINEL, dtype=torch.uint8, device=dev)
        ref = _lib.StoreRef(buf.data_ptr() + lead, _lib.FrameStore(3 * stride + 16, stride, pitch, 3, h, w, 0), bgr, 0)
        items = F.YuvConverter.table_ex([frame], [None], [ref], [1])
        assert items[0].dst == buf.data_ptr() + lead + stride and items[0].dst_pitch == pitch
        _lib.check(_lib.lib.af_yuv_to_rgb_ex_u8(C.byref(items), 1, stream), "yuv_to_rgb_ex_u8")
        runs.append(((fmt, w, h, matrix, full), buf, want, lead + stride, pitch, frame))
    torch.cuda.synchronize()
    assert any((b.data_ptr() + at) % 2 for _, b, _, at, _, _ in runs) and any((b.data_ptr() + at) % 2 == 0 for _, b, _, at, _, _ in runs)
    for case, buf, want, at, pitch, _ in runs:
        got = buf.cpu().numpy()
        h, w = want.shape[:2]
        rows = np.lib.stride_tricks.as_strided(got[at:], (h, pitch), (pitch, 1))
        assert np.array_equal(rows[:, :3 * w].reshape(h, w, 3), want), case
        mask = np.ones(got.size, bool)
        for r in range(h):
            mask[at + r * pitch:at + r * pitch + 3 * w] = False
        assert (got[mask] == SENTINEL).all(), case


# ---- the cube and the lattice --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cube():
    """the Y, U, V planes of a 4096 x 4096 i444 frame that holds every (Y, U, V) exactly once, on the device and on the host"""
    p = np.arange(1 << 24, dtype=np.int32).reshape(4096, 4096)
    planes = ((p >> 16).astype(np.uint8), ((p >> 8) & 255).astype(np.uint8), (p & 255).astype(np.uint8))
    return planes, [torch.from_numpy(c).to(_dev()) for c in planes]


@pytest.mark.parametrize("matrix,full", X.COLOURS)
def test_the_whole_cube_in_one_launch(cube, matrix, full, monkeypatch):
    counted = Counted(monkeypatch)
    (y, u, v), on_device = cube
    order = "bgr" if full else "rgb"
    want = torch.from_numpy(np.concatenate([X.yuv_to_bgr(y[r:r + 256], u[r:r + 256], v[r:r + 256], matrix, full) for r in range(0, 4096, 256)]))
    store = _store(4096, 4096, order, capacity=1)
    conv = F.YuvConverter(_dev())
    conv.convert([(F.YuvFrame("i444", *on_device, matrix=matrix, full_range=full), store, order, 0)])
    want = want.to(_dev())
    assert torch.equal(store.view(0), want if order == "bgr" else want.flip(-1))
    assert conv.launches == 1 and (counted.old, counted.new) == (0, 1) and bool((store.dev[-16:] == SENTINEL).all())


@pytest.fixture(scope="module")
def lattice():
    """4:2:0 samples of a 512 x 3698 frame: chroma block (i, j) holds the i-th (U, V) of the lattice and the four Y values 4 j + {0, 1,
    2, 3}, so every one of the 1024 Y meets every (U, V) of the lattice once"""
    from test_yuv_formats_host import LATTICE
    c = np.array(LATTICE, dtype=np.uint16)
    n = len(c)
    u = np.broadcast_to(np.repeat(c, n)[:, None], (n * n, 256)).copy()
    v = np.broadcast_to(np.tile(c, n)[:, None], (n * n, 256)).copy()
    y = np.zeros((2 * n * n, 512), np.uint16)
    base = (4 * np.arange(256, dtype=np.uint16))[None, :]
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = base, base + 1, base + 2, base + 3
    assert y.shape == (2 * n * n, 512) and int(y.max()) == 1023 and {0, 64, 512, 940 + 20, 1023} <= set(LATTICE)
    return y, u, v


@pytest.mark.parametrize("fmt", ["i010", "p010"])
def test_the_10_bit_lattice_in_one_launch(lattice, fmt):
    y, u, v = lattice
    h, w = y.shape
    if fmt == "p010":                                             # the value in bits 15..6; the low six bits are to be ignored
        junk = np.random.default_rng(6).integers(0, 64, y.shape, dtype=np.uint16)
        y, u, v = (y << 6) | junk, (u << 6) | junk[:h // 2, :w // 2], (v << 6) | junk[h // 2:, w // 2:]
    planes = X.pack(y, u, v, fmt)
    conv = F.YuvConverter(_dev())
    jobs, wants = [], []
    for k, (matrix, full) in enumerate(X.COLOURS):
        order = "bgr" if k % 2 else "rgb"
        wants.append(X.convert(planes, fmt, matrix, full, order))
        jobs.append((_frame(planes, fmt, (0, 0), _dev() if k < 2 else None, matrix=matrix, full_range=full), _store(h, w, order, capacity=1), order, 0))
    conv.convert(jobs)                                            # the four colours in one launch
    torch.cuda.synchronize()
    assert conv.launches == 1 and conv.copies == 1
    for (_, store, _, _), want, colour in zip(jobs, wants, X.COLOURS):
        assert np.array_equal(store.view(0).cpu().numpy(), want), (fmt, colour)
    assert len({want.tobytes() for want in wants}) == 4


# ---- the new launch on the old formats -----------------------------------------------------------------------------------------------

class ExOnly(F.YuvConverter):
    """a converter that sends every batch through the new launch"""

    def convert(self, jobs):
        self._legacy = False
        F._Converter.convert(self, list(jobs))


@pytest.mark.parametrize("fmt", list(F.FORMATS))
def test_the_new_launch_on_the_old_formats_equals_the_old_launch(fmt, monkeypatch):
    counted = Counted(monkeypatch)
    old, new = F.YuvConverter(_dev()), ExOnly(_dev())
    pairs = []
    for w, h in SIZES + [(66, 34), (130, 18)]:
        for k, variant in enumerate(VARIANTS):
            planes = X.random_planes(fmt, h, w, seed=31 * h + w + k)
            order = "bgr" if k % 2 else "rgb"
            stores, frames = [], []
            for conv in (old, new):
                frames.append(_frame(planes, fmt, variant, _dev() if k < 2 else None))
                assert frames[-1].legacy
                stores.append(_store(h, w, order))
                conv.convert([(frames[-1], stores[-1], order, 1)])
            pairs.append(((fmt, w, h, variant), stores, X.convert(planes, fmt, order=order), frames))
    torch.cuda.synchronize()
    assert counted.old == counted.new == len(pairs) == old.launches == new.launches
    for case, (a, b), want, _ in pairs:
        assert torch.equal(a.dev, b.dev), case
        assert np.array_equal(b.view(1).cpu().numpy(), want), case


# ---- mixed launches ------------------------------------------------------------------------------------------------------------------

def test_twelve_formats_share_one_launch(monkeypatch):
    counted = Counted(monkeypatch)
    sizes = [(26, 6), (10, 6), (66, 34), (130, 18)]               # (w, h); 66 x 34 as yvyu is 34 x 9 = 306 runs: two tiles
    stores = {(26, 6, "bgr"): _store(6, 26, "bgr", 6), (26, 6, "rgb"): _store(6, 26, "rgb", 6), (10, 6, "rgb"): _store(6, 10, "rgb", 6),
              (66, 34, "bgr"): _store(34, 66, "bgr", 6), (130, 18, "rgb"): _store(18, 130, "rgb", 6)}
    jobs, singles, wants, slots = [], [], [], {}
    for k, fmt in enumerate(ALL):
        w, h = sizes[k % 4]
        has = [o for o in ("bgr", "rgb") if (w, h, o) in stores]
        order = has[(k // 4) % len(has)]
        matrix, full = X.COLOURS[(k + k // 4) % 4]
        planes = X.random_planes(fmt, h, w, seed=500 + k)
        wants.append(X.convert(planes, fmt, matrix, full, order))
        slot = slots[(w, h, order)] = slots.get((w, h, order), -1) + 1
        jobs.append((_frame(planes, fmt, VARIANTS[k % 4], _dev() if k % 3 == 0 else None, matrix=matrix, full_range=full), stores[(w, h, order)], order, slot))
        singles.append((jobs[-1][0], _store(h, w, order, 6), order, slot))
    assert len(jobs) == 12 and {j[0].fmt for j in jobs} == set(ALL) and {j[2] for j in jobs} == {"bgr", "rgb"}
    assert {(j[0].matrix, j[0].full_range) for j in jobs} == set(X.COLOURS) and {j[0].on_device for j in jobs} == {False, True}
    assert len({id(j[1]) for j in jobs}) == 5 and max(slots.values()) >= 2
    together, alone = F.YuvConverter(_dev()), F.YuvConverter(_dev())
    together.convert(jobs)
    assert (together.launches, together.copies, counted.old, counted.new) == (1, 1, 0, 1)
    for job in singles:
        alone.convert([job])
    torch.cuda.synchronize()
    assert alone.launches == 12 and alone.copies == sum(not j[0].on_device for j in jobs)
    for (frame, store, order, slot), single, want in zip(jobs, singles, wants):
        assert np.array_equal(store.view(slot).cpu().numpy(), want), (frame.fmt, order, slot)
        assert torch.equal(single[1].view(slot), store.view(slot))
    for (w, h, order), store in stores.items():
        used = slots[(w, h, order)] + 1
        assert bool((store.dev[used * h * w * 3:] == SENTINEL).all()), (w, h, order)


def test_more_frames_than_a_table_holds_make_two_launches_and_old_batches_keep_the_old_launch(monkeypatch):
    counted = Counted(monkeypatch)
    n = _lib.YUV_MAX_FRAMES + 1
    store = _store(2, 2, "bgr", capacity=n)
    planes = [X.random_planes("yuy2", 2, 2, seed=k) for k in range(n)]
    conv = F.YuvConverter(_dev())
    conv.convert([(F.YuvFrame("yuy2", p[0]), store, "bgr", n - 1 - k) for k, p in enumerate(planes)])
    torch.cuda.synchronize()
    assert conv.launches == 2 and conv.copies == 1 and (counted.old, counted.new) == (0, 2)
    got = store.view(0, n).cpu().numpy()
    for k, p in enumerate(planes):
        assert np.array_equal(got[n - 1 - k], X.convert(p, "yuy2")), k
    assert bool((store.dev[-16:] == SENTINEL).all())
    # every frame an old format at the default colour: the old launch, as before
    old_planes = [X.random_planes(fmt, 2, 2, seed=k) for k, fmt in enumerate(F.FORMATS)]
    conv.convert([(F.YuvFrame(fmt, **X.kwargs(p, fmt)), store, "bgr", k) for k, (fmt, p) in enumerate(zip(F.FORMATS, old_planes))])
    assert conv.launches == 3 and (counted.old, counted.new) == (1, 2)
    # one frame of another colour among them: the whole batch goes through the new launch
    jobs = [(F.YuvFrame(fmt, **X.kwargs(p, fmt), full_range=(k == 2)), store, "bgr", k) for k, (fmt, p) in enumerate(zip(F.FORMATS, old_planes))]
    conv.convert(jobs)
    torch.cuda.synchronize()
    assert conv.launches == 4 and (counted.old, counted.new) == (1, 3)
    for k, (fmt, p) in enumerate(zip(F.FORMATS, old_planes)):
        assert np.array_equal(store.view(k).cpu().numpy(), X.convert(p, fmt, "bt601", k == 2)), fmt


# ---- end to end: the scripts ---------------------------------------------------------------------------------------------------------

def _flat(fmt, value):
    """the stored sample of an 8-bit value"""
    return {"p010": value << 8, "i010": value << 2}.get(fmt, value)


def _picture(rng, fmt, h, w, patch=None):
    """random stored samples of one frame; `patch` = (r0, r1, c0, c1) in pixels, on even bounds: flat in Y, U and V"""
    _, vdiv, hdiv, bits = X.FORMATS[fmt]
    dtype, top = (np.uint8, 256) if bits == 8 else (np.uint16, 1024)
    ch = X.chroma_shape(fmt, h, w)
    y, u, v = (rng.integers(0, top, s).astype(dtype) for s in ((h, w), ch, ch))
    if fmt == "p010":
        y, u, v = y << 6, u << 6, v << 6
    if patch is not None:
        r0, r1, c0, c1 = patch
        y[r0:r1, c0:c1] = _flat(fmt, 100)
        u[r0 // vdiv:-(-r1 // vdiv), c0 // hdiv:-(-c1 // hdiv)] = _flat(fmt, 120)
        v[r0 // vdiv:-(-r1 // vdiv), c0 // hdiv:-(-c1 // hdiv)] = _flat(fmt, 140)
    return X.pack(y, u, v, fmt)


def _call_script(shape, fmt, colour, seed, blurry, face1, face2):
    """tests/test_hip_yuv.py's script of one call for any format and colour: per tick the planes, the statement's B, G, R frame of them
    and the YuNet rows of two faces.  Face 1 is blurry - its crop flat in Y, U and V - on the `blurry` ticks; face 2 walks into the
    self-view rectangle and back out"""
    H, W = shape
    (x1, y1, dx1, dy1), (x2, y2, dx2, dy2) = face1, face2
    rng = np.random.default_rng(seed)
    std = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
    out = []
    for s in range(TY.STEPS):
        t = min(max(s - 8, 0), 8) if s < 22 else max(0, 8 - (s - 21))
        faces = [(x1 + dx1 * s, y1 + dy1 * s, 30, 34, 0.95), (x2 + dx2 * t, y2 + dy2 * t, 28, 32, 0.93)]
        rows = []
        for x, yy, w, h, sc in faces:
            j = rng.uniform(-0.3, 0.3, 4)
            x, yy, w, h = x + j[0], yy + j[1], w + j[2], h + j[3]
            lm = std * [w, h] + [x, yy] + rng.normal(0, 0.4, (5, 2))
            rows.append(np.concatenate([[x, yy, w, h], [sc + rng.uniform(-0.004, 0.004)], lm.ravel()]))
        rows = np.asarray(rows, dtype=np.float32)
        patch = None
        if s in blurry:
            bx1, by1, bx2, by2 = map(int, get_crop_box((H, W), [rows[0, 0], rows[0, 1], rows[0, 0] + rows[0, 2], rows[0, 1] + rows[0, 3]], scale=0.6))
            patch = (max(0, by1 - 6) // 2 * 2, min(H, (by2 + 7) // 2 * 2), max(0, bx1 - 6) // 2 * 2, min(W, (bx2 + 7) // 2 * 2))      # whole chroma blocks
        planes = _picture(rng, fmt, H, W, patch)
        out.append((planes, X.convert(planes, fmt, *colour), rows))
    return out


def _yuv(planes, fmt, colour, device=False):
    return _frame(planes, fmt, (0, 0), _dev() if device else None, matrix=colour[0], full_range=colour[1])


# ---- LiveCall ------------------------------------------------------------------------------------------------------------------------

LIVE = (("yuy2", ("bt601", False), False), ("i422", ("bt601", True), True))      # before and from step TY.LIVE_SWITCH on: format, colour, on device
LIVE_SHAPES = ((95, 130), (80, 112))                               # before and from step TY.LIVE_RESIZE on; 95: chroma keeps its rows


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_a_live_call_on_yuy2_and_full_range_i422_frames_equals_its_twin(order):
    script = TL._script(TY.LIVE_STEPS, {1: 0, 2: 0}, seed=9)
    rng = np.random.default_rng(300)
    inputs = []
    for s in range(TY.LIVE_STEPS):
        fmt, colour, on_device = LIVE[s >= TY.LIVE_SWITCH]
        h, w = LIVE_SHAPES[s >= TY.LIVE_RESIZE]
        planes = _picture(rng, fmt, h, w)
        inputs.append((planes, fmt, colour, on_device, X.convert(planes, fmt, *colour, order)))
    twin, rows = TY._live_call(order), []
    for s, (_, _, _, _, frame) in enumerate(inputs):
        rows.append(twin.step(frame, script[s]))
    closes = [s for s, results in enumerate(rows) if results]
    assert any(s < TY.LIVE_SWITCH for s in closes) and any(TY.LIVE_SWITCH <= s < TY.LIVE_RING for s in closes), closes      # both formats
    assert any(TY.LIVE_RING <= s < TY.LIVE_RESIZE for s in closes) and any(s >= TY.LIVE_RESIZE for s in closes), closes    # the wrap; the re-open
    assert all(sorted(t for t, _ in rows[s]) == [1, 2] for s in closes) and TY.LIVE_RING < TY.LIVE_RESIZE
    call, uploaded = TY._live_call(order), 0
    for s, (planes, fmt, colour, on_device, frame) in enumerate(inputs):
        got = call.step(_yuv(planes, fmt, colour, on_device), script[s])
        uploaded += 0 if on_device else 2 * frame.shape[0] * frame.shape[1]
        assert call._shape == frame.shape and call.frame_idx == s
        assert torch.equal(call.frame_view(s).cpu(), torch.from_numpy(frame)), (order, s)
        assert got == rows[s], (order, s, got, rows[s])
        assert call.uploaded_bytes == uploaded
    assert call._first == TY.LIVE_RESIZE


# ---- RealtimeCall --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,colour,shape", [("yuy2", ("bt601", False), (95, 130)), ("i422", ("bt601", True), (96, 130))])
def test_a_realtime_call_equals_its_twin(fmt, colour, shape):
    H, W = shape
    script = _call_script(shape, fmt, colour, 4, range(10, 15), (14, 22, 0.5, 0.1), (50, 40, 5.0, 2.5))
    det = TS.StubDetector({"A": [(bgr, rows) for _, bgr, rows in script]})
    twin, rows = TY._realtime(det), []
    for _, bgr, _ in script:
        rows.append((twin.step(bgr), TY._books(twin)))
    closes = [s for s, (results, _) in enumerate(rows) if results]
    assert len(closes) >= 2 and any(s < TY.RING for s in closes) and any(s >= TY.RING for s in closes), closes     # across a ring wrap
    assert any(b["purged"] for _, b in rows) and any(v[1] < 5.0 for v in twin.host.q_hist[1])                     # a purge; the gate said no
    call = TY._realtime(det)
    for s, (planes, bgr, _) in enumerate(script):
        got = call.step(_yuv(planes, fmt, colour))
        assert torch.equal(call.call.frame_view(s).cpu(), torch.from_numpy(bgr))
        assert got == rows[s][0], (s, got, rows[s][0])
        TY._same_books(TY._books(call), rows[s][1])
        assert call.uploaded_bytes == (s + 1) * H * W * 2
    assert {t: list(v) for t, v in call.host.q_hist.items()} == {t: list(v) for t, v in twin.host.q_hist.items()}


# ---- CallServer ----------------------------------------------------------------------------------------------------------------------

#          frame size, channel order, format, colour, planes on the device, seed, blurry ticks, face 1, face 2
SERVED = {"A": ((96, 130), "bgr", "nv12", ("bt601", False), True, 4, range(10, 15), (14, 22, 0.5, 0.1), (50, 40, 5.0, 2.5)),
          "B": ((81, 112), "rgb", "yuy2", ("bt601", False), False, 6, range(13, 18), (8, 20, 0.25, 0.1), (52, 30, 2.5, 2.0)),
          "C": ((96, 130), "rgb", "p010", ("bt709", False), True, 5, range(18, 23), (12, 24, 0.4, 0.1), (52, 38, 5.0, 2.5)),
          "D": ((96, 130), "bgr", "i420", ("bt709", False), False, 7, range(12, 17), (13, 23, 0.45, 0.1), (51, 39, 5.0, 2.5))}
SERVED_OPENS = {"A": 0, "B": 5, "C": 0, "D": 0}
SERVED_ABSENT = {"D": (16, 17)}
STAGED = {"A": 0.0, "B": 2.0, "C": 0.0, "D": 1.5}                  # host bytes per pixel


def _serving(tick):
    return [n for n in SERVED if SERVED_OPENS[n] <= tick and tick not in SERVED_ABSENT.get(n, ())]


@pytest.fixture(scope="module")
def served():
    """the scripts, the stub detector that knows every converted frame, and per tick and call a lone RealtimeCall's results and
    books on the statement's converted frames"""
    scripts = {n: _call_script(c[0], c[2], c[3], *c[5:]) for n, c in SERVED.items()}
    det = TS.StubDetector({n: [(TY._in_order(bgr, SERVED[n][1]), rows) for _, bgr, rows in scripts[n]] for n in SERVED})
    lone, own, ticks = {}, {n: 0 for n in SERVED}, []
    for tick in range(TY.STEPS):
        row = {}
        for n in _serving(tick):
            if n not in lone:
                lone[n] = TY._realtime(det, SERVED[n][1])
            k = own[n]
            own[n] += 1
            row[n] = (k, lone[n].step(TY._in_order(scripts[n][k][1], SERVED[n][1])), TY._books(lone[n]))
        ticks.append(row)
    return scripts, det, ticks


def test_the_served_scripts_produce_the_cases(served):
    _, _, ticks = served
    closes = [{n: len(r[1]) for n, r in row.items() if r[1]} for row in ticks]
    assert any(len(c) >= 2 for c in closes), closes                                           # shared batches
    assert all(any(n in c for c in closes) for n in SERVED), closes                          # every format is scored
    assert any(r[1] and r[0] >= TY.RING for row in ticks for r in row.values())               # a close after a ring wrap
    assert any(r[2]["purged"] for row in ticks for r in row.values())
    assert all("D" not in ticks[t] for t in SERVED_ABSENT["D"]) and "B" not in ticks[4] and "B" in ticks[5]


def test_the_server_on_four_formats_equals_lone_calls_and_a_server_on_converted_frames(served, monkeypatch):
    counted = Counted(monkeypatch)
    scripts, det, ticks = served
    mixed, plain = [af_mi355x.CallServer(TL._net(), detector=det, clip_size=CLIP, size=SIZE, **TS._args("bgr")) for _ in range(2)]
    cids, uploaded = {}, {n: 0 for n in SERVED}
    for tick, row in enumerate(ticks):
        for n in SERVED:
            if SERVED_OPENS[n] == tick:
                cids[n] = mixed.open(channel_order=SERVED[n][1])
                assert plain.open(channel_order=SERVED[n][1]) == cids[n]
        names = list(row)
        before = counted.new
        got = mixed.step({cids[n]: _yuv(scripts[n][row[n][0]][0], SERVED[n][2], SERVED[n][3], SERVED[n][4]) for n in names})
        want = plain.step({cids[n]: TY._in_order(scripts[n][row[n][0]][1], SERVED[n][1]) for n in names})
        assert got == want and list(got) == [cids[n] for n in names], (tick, got, want)      # scores bit for bit, at the same batches
        closing = [n for n in names if row[n][1]]
        for n in names:
            k, results, books = row[n]
            c = mixed.call(cids[n])
            (h, w), order = SERVED[n][:2]
            assert torch.equal(c.call.frame_view(k).cpu(), torch.from_numpy(TY._in_order(scripts[n][k][1], order))), (tick, n)
            assert [t for t, _ in got[cids[n]]] == [t for t, _ in results], (tick, n)
            TY._same_books(TY._books(c), books, scored=False)                                 # a lone call's, whatever the batch
            TY._same_books(TY._books(c), TY._books(plain.call(cids[n])))
            if closing == [n]:                                                                # the batch a lone call pads to: its scores
                assert got[cids[n]] == results, (tick, n)
            uploaded[n] += int(h * w * STAGED[n])
            assert c.uploaded_bytes == uploaded[n], (tick, n)
        st = mixed.stats.last
        n_host = sum(STAGED[n] > 0 for n in names)
        assert st["convert"] == 1 and counted.new == before + 1 and st["yuv_copies"] == (1 if n_host else 0) and st["wait"] <= 3, (tick, st)
        assert st["wait"] == plain.stats.last["wait"] and plain.stats.last["convert"] == 0     # the conversion needs no wait
        assert mixed.uploaded_bytes == sum(uploaded.values())
    assert mixed.stats.total["convert"] == TY.STEPS == counted.new and counted.old == 0


# ---- VideoScorer and VideoRunner -----------------------------------------------------------------------------------------------------

def test_the_video_scorer_scores_uyvy_frames():
    shape, _, detections = TV._crossing_video(71, n_frames=12)
    H, W = shape[:2]
    rng = np.random.default_rng(60)
    planes = [_picture(rng, "uyvy", H, W) for _ in range(12)]
    yuv, rgb = [F.YuvFrame("uyvy", p[0]) for p in planes], [X.convert(p, "uyvy", order="rgb") for p in planes]
    vs = evaluator.VideoScorer(None, TL._net(), clip_size=CLIP, size=SIZE, batch=4)
    want = vs.score(rgb, detections=detections)
    assert len(want["tracks"]) == 2 and len(want["preds"]) == 2 * (12 - CLIP + 1) and vs.uploaded_bytes == 12 * H * W * 3
    got = vs.score(yuv, detections=detections)
    TV._same_result(got, want)
    assert got["spans"] == want["spans"] and vs.uploaded_bytes == 12 * H * W * 2


def test_the_video_runner_runs_uyvy_frames():
    h, w = 97, 132                                                 # an odd height: 4:2:2 keeps its chroma rows
    rng = np.random.default_rng(12)
    planes, bgr = [], []
    for f in range(TR.FRAMES):
        y, u, v = rng.integers(16, 236, (h, w), dtype=np.uint8), rng.integers(96, 160, (h, w // 2), dtype=np.uint8), \
            rng.integers(96, 160, (h, w // 2), dtype=np.uint8)
        if f in TR.BLURRY:
            y[:72, :70], u[:72, :35], v[:72, :35] = 90, 128, 128
        planes.append(X.pack(y, u, v, "uyvy"))
        bgr.append(X.convert(planes[-1], "uyvy"))
    script = list(zip(bgr, TR._rows()))
    want = TR._runner(TR._StubDetector(script), detect_batch=16).run(bgr, fps=30.0)
    assert sum(len(v) for v in want["track_clip_scores"].values()) >= 4
    yuv = [af_mi355x.YuvFrame("uyvy", p[0]) for p in planes]
    got = TR._runner(TR._StubDetector(script), detect_batch=16).run(yuv, fps=30.0)
    assert TR._plain(got) == TR._plain(want)
    as_rgb = TR._runner(TR._StubDetector(script, [np.ascontiguousarray(f[..., ::-1]) for f in bgr]), channel_order="rgb", detect_batch=16).run(yuv, fps=30.0)
    assert TR._plain(as_rgb) == TR._plain(want)
