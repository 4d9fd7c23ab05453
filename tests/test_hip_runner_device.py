"""GPU: ``VideoRunner(tracker="device")`` - the chunk stage as one launch, the quality launch out of its record, the run.

  (a) chunk    ``af_runner_track_chunk`` against its host twin (the same source on the CPU, pinned against the statement by
               tests/test_runner_device_host.py): the record's bytes and the state's bytes after every chunk of the four golden
               runs and of the scripts of tests/runner_chunk_cases.py, at chunk sizes 1, 5 and 16; the same chunk twice from the
               same state gives the same bytes; the guard bands around state and record hold
  (b) quality  ``af_face_quality_table_u8`` against ``af_face_quality_stores_u8`` / ``af_face_laplacian_stores_u8`` on the same
               rectangles of a random 3-slot store of 70 x 90 pixels: sums and grey bytes equal, for 0, 1, 64, 65 and 130
               candidates, both byte orders, both modes; a rectangle outside its frame and a slot outside the store are skipped
               and flagged, the others exact; sums behind the count stay zero; guard bands hold
  (c) run      with test_hip_runner's stub detector and script: ``VideoRunner(tracker="device").run`` equals ``VideoRunner().run``
               key for key, trace and score bits included, at chunk sizes 1, 5 and 16, for RGB and I420 frames; one wait and one
               ``track`` launch per chunk against the host mode's two waits; the overflow raises
"""
import ctypes as C

import numpy as np
import pytest
import torch

import af_mi355x
import runner_chunk_cases as cases
import runner_chunk_ref as ref
import yuv_ref
from af_mi355x import _lib
from af_mi355x import runner_device as RD
from conftest import load_json
from test_hip_runner import ARGS, BLURRY, FRAMES, H, W, _plain, _rows, _runner, _StubDetector

pytestmark = pytest.mark.gpu
GUARD, MAX_ROWS = 256, 40
RUNS = load_json("runner_video.json")["runs"]
ALL = [cases.golden_case(name, RUNS[name]) for name in sorted(RUNS)] + cases.CASES


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n_bytes, fill):
    whole = torch.full((n_bytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + n_bytes]


def _intact(whole, n_bytes, fill):
    host = whole.cpu().numpy()
    return bool((host[:GUARD] == fill).all() and (host[GUARD + n_bytes:] == fill).all())


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------

def _launch(plan, state, rows, counts, record, first_slot, ids):
    chunk = plan.chunk(state.data_ptr(), rows.data_ptr(), counts.data_ptr(), record.data_ptr(), rows.numel(), rows.shape[1], rows.shape[2],
                       first_slot, ids)
    _lib.check(_lib.lib.af_runner_track_chunk(C.byref(chunk), _stream()), "af_runner_track_chunk")


@pytest.mark.parametrize("size", [1, 5, 16])
@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_a_the_launch_equals_its_host_twin(case, size):
    plan = case.plan()
    host_state = plan.reset()
    whole_state, state = _guarded(RD.STATE_BYTES, 0xA5)
    state.copy_(torch.from_numpy(host_state))
    n_chunks = []

    def step(rows, ids, base):
        laid, counts = cases.laid_out(rows, MAX_ROWS, seed=base)
        n = RD.record_bytes(len(ids))
        want = np.full(n // 8, 0, dtype=np.float64).view(np.uint8)
        want[:] = 0x5A
        RD.track_chunk_host(plan, host_state, laid, counts, base, ids, want)
        d_rows, d_counts = torch.from_numpy(laid).cuda(), torch.from_numpy(counts).cuda()
        whole, record = _guarded(n, 0x5A)
        whole2, record2 = _guarded(n, 0x5A)
        before = state.clone()
        _launch(plan, state, d_rows, d_counts, record, base, ids)
        _launch(plan, before, d_rows, d_counts, record2, base, ids)                 # the same chunk from the same state
        torch.cuda.synchronize()
        got = record.cpu().numpy()
        assert got.tobytes() == want.tobytes(), "the record of chunk %d" % len(n_chunks)
        assert state.cpu().numpy().tobytes() == host_state.tobytes(), "the state after chunk %d" % len(n_chunks)
        assert torch.equal(record, record2) and torch.equal(state, before)
        assert _intact(whole, n, 0x5A) and _intact(whole2, n, 0x5A) and _intact(whole_state, RD.STATE_BYTES, 0xA5)
        n_chunks.append(len(ids))
        rec = RD.parse_record(got, len(ids))
        head = rec["head"]
        return any(int(f["flags"]) & RD.PROCESSED for f in rec["frames"][:len(ids)]), bool(head["stop"]) or bool(head["overflow"])
    cases.walk(case, size, step)
    assert n_chunks


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------

SH, SW, SLOTS = 70, 90, 3


def _rects(n, seed=3):
    """(slot, x1, y1, x2, y2): the corners first, then random ones of every parity"""
    fixed = [(0, 5, 7, 6, 8), (1, 11, 3, 12, 5), (2, SW - 31, SH - 23, SW, SH), (1, 2, 4, 39, 27), (0, 0, 0, 67, 45), (2, 10, 10, 11, 60),
             (0, 3, 3, 43, 33), (1, 0, 0, SW, SH)]        # 1 x 1; 1 x 2; ending on the store's last pixel; 37 x 23 and 67 x 45 (area table); a column
    rng = np.random.default_rng(seed)
    out = list(fixed)
    while len(out) < n:
        w, h = int(rng.integers(1, 50)), int(rng.integers(1, 40))
        x, y = int(rng.integers(0, SW - w + 1)), int(rng.integers(0, SH - h + 1))
        out.append((int(rng.integers(0, SLOTS)), x, y, x + w, y + h))
    return out[:n]


def _record_of(rects, n_frames):
    rec = np.zeros(1, dtype=RD.record_dtype(n_frames))[0]
    half = full = 0
    for i, (slot, x1, y1, x2, y2) in enumerate(rects):
        c = rec["cands"][i]
        c["frame_pos"], c["slot"], c["tid"], c["box"] = i // RD.MAX_TRACKS, slot, i + 1, (x1, y1, x2, y2)
        c["tile_half"], c["tile_full"] = half, full
        w, h = x2 - x1, y2 - y1
        half += ref.tiles_of(max(1, w // 2), max(1, h // 2))
        full += ref.tiles_of(w, h)
    rec["head"]["n_cands"], rec["head"]["tiles_half"], rec["head"]["tiles_full"], rec["head"]["n_frames"] = len(rects), half, full, n_frames
    return rec


@pytest.fixture(scope="module")
def store():
    rng = np.random.default_rng(21)
    pixels = torch.from_numpy(rng.integers(0, 256, (SLOTS, SH, SW, 3), dtype=np.uint8)).cuda()
    desc = _lib.FrameStore(pixels.numel(), SH * SW * 3, SW * 3, SLOTS, SH, SW, 0)
    return pixels, desc


def _reference(store, rects, bgr, full):
    """``af_face_quality_stores_u8`` / ``af_face_laplacian_stores_u8`` on the rectangles, 64 per launch: [(n_px, s1, s2)], [grey bytes]"""
    pixels, desc = store
    refs = (_lib.StoreRef * 1)(_lib.StoreRef(pixels.data_ptr(), desc, bgr, 0))
    fn = _lib.lib.af_face_laplacian_stores_u8 if full else _lib.lib.af_face_quality_stores_u8
    sums, greys = [], []
    for lo in range(0, len(rects), _lib.QUALITY_MAX_RECTS):
        part = rects[lo:lo + _lib.QUALITY_MAX_RECTS]
        items = (_lib.FrameRect * len(part))(*[_lib.FrameRect(s, x1, y1, y2 - y1, x2 - x1, 0, 0, 0) for s, x1, y1, x2, y2 in part])
        sizes = [((x2 - x1) if full else max(1, (x2 - x1) // 2)) * ((y2 - y1) if full else max(1, (y2 - y1) // 2)) for _, x1, y1, x2, y2 in part]
        d_sums = torch.zeros(len(part) * 24, dtype=torch.uint8, device="cuda")
        grey = torch.zeros(sum(sizes), dtype=torch.uint8, device="cuda")
        _lib.check(fn(refs, 1, items, len(part), C.c_void_p(d_sums.data_ptr()), C.c_void_p(grey.data_ptr()), grey.numel(), _stream()), "reference")
        torch.cuda.synchronize()
        raw = np.frombuffer(d_sums.cpu().numpy().tobytes(), dtype=af_mi355x.live._SUMS_DTYPE)
        sums += [(int(r["n_px"]), int(r["s1"]), int(r["s2"])) for r in raw]
        g, at = grey.cpu().numpy(), 0
        for s in sizes:
            greys.append(g[at:at + s].tobytes())
            at += s
    return sums, greys


def _table(store, rec, n_frames, bgr, full, stride=SH * SW):
    pixels, desc = store
    capacity = n_frames * RD.MAX_TRACKS
    d_rec = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).cuda()
    whole_s, d_sums = _guarded(capacity * 24, 0x77)
    whole_g, d_grey = _guarded(capacity * stride, 0x66)
    one = _lib.StoreRef(pixels.data_ptr(), desc, bgr, 0)
    _lib.check(_lib.lib.af_face_quality_table_u8(C.byref(one), C.c_void_p(d_rec.data_ptr()), capacity, int(full), C.c_void_p(d_sums.data_ptr()),
                                                 C.c_void_p(d_grey.data_ptr()), stride, _stream()), "af_face_quality_table_u8")
    torch.cuda.synchronize()
    assert _intact(whole_s, capacity * 24, 0x77) and _intact(whole_g, capacity * stride, 0x66)
    raw = np.frombuffer(d_sums.cpu().numpy().tobytes(), dtype=af_mi355x.live._SUMS_DTYPE)
    return [(int(r["n_px"]), int(r["s1"]), int(r["s2"])) for r in raw], d_grey.cpu().numpy().reshape(capacity, stride), RD.parse_record(d_rec.cpu().numpy(), n_frames)


@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
@pytest.mark.parametrize("bgr", [0, 1], ids=["rgb", "bgr"])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 130])
def test_b_the_table_launch_equals_the_listed_launch(store, n, bgr, full):
    n_frames = 5                                              # 160 places
    rects = _rects(n)
    want, greys = _reference(store, rects, bgr, full)
    got, grey, rec = _table(store, _record_of(rects, n_frames), n_frames, bgr, full)
    assert got[:n] == want and all(s == (0, 0, 0) for s in got[n:])
    for k, g in enumerate(greys):
        assert grey[k, :len(g)].tobytes() == g and (grey[k, len(g):] == 0x66).all(), k
    assert (grey[n:] == 0x66).all() and int(rec["head"]["bad"]) == 0 and not rec["cands"]["flags"].any()


@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
def test_b_a_bad_candidate_is_skipped_and_flagged(store, full):
    rects = _rects(8)
    bad = list(rects)
    bad[2] = (2, SW - 31, SH - 23, SW + 1, SH)                # one column outside its frame
    bad[4] = (SLOTS, 0, 0, 67, 45)                            # a slot outside the store
    want, _ = _reference(store, rects, 1, full)
    got, _, rec = _table(store, _record_of(bad, 1), 1, 1, full)
    flagged = [i for i in range(8) if int(rec["cands"][i]["flags"]) & RD.CAND_BAD]
    assert flagged == [2, 4] and int(rec["head"]["bad"]) == 1
    for i in range(8):
        assert got[i] == ((0, 0, 0) if i in flagged else want[i]), i
    assert all(s == (0, 0, 0) for s in got[8:])


def test_b_the_table_launch_checks_its_arguments(store):
    pixels, desc = store
    one = _lib.StoreRef(pixels.data_ptr(), desc, 0, 0)
    sums = torch.zeros(24, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(RD.record_bytes(1), dtype=torch.uint8, device="cuda")
    assert _lib.lib.af_face_quality_table_u8(C.byref(one), C.c_void_p(rec.data_ptr()), 64 * 32 + 1, 0, C.c_void_p(sums.data_ptr()), None, 0, _stream()) != 0
    assert _lib.lib.af_face_quality_table_u8(C.byref(one), None, 1, 0, C.c_void_p(sums.data_ptr()), None, 0, _stream()) != 0
    assert _lib.lib.af_face_quality_table_u8(C.byref(one), C.c_void_p(rec.data_ptr()), 0, 0, C.c_void_p(sums.data_ptr()), None, 0, _stream()) == 0


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def script():
    rng = np.random.default_rng(9)
    frames = []
    for f in range(FRAMES):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if f in BLURRY:
            frame[:72, :70] = 90
        frames.append(frame)
    return list(zip(frames, _rows()))


def _same_trace(a, b):
    assert a["processed"] == b["processed"] and a["flush_groups"] == b["flush_groups"] and a["slots_used"] == b["slots_used"]
    assert [tuple(q) for q in a["qstat"]] == [tuple(q) for q in b["qstat"]] and len(a["clips"]) == len(b["clips"])
    for x, y in zip(a["clips"], b["clips"]):
        assert (x["tid"], x["frame_idx"], x["slots"]) == (y["tid"], y["frame_idx"], y["slots"])
        for rx, ry in zip(x["records"], y["records"]):
            assert all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(rx, ry))


@pytest.fixture(scope="module")
def host_run(script):
    r = _runner(_StubDetector(script), detect_batch=5)
    return r.run([f for f, _ in script], fps=30.0), r


@pytest.mark.parametrize("detect_batch", [1, 5, 16])
def test_c_the_device_run_equals_the_host_run(script, host_run, detect_batch):
    want, host = host_run
    det = _StubDetector(script)
    r = _runner(det, detect_batch=detect_batch, tracker="device")
    out = r.run([f for f, _ in script], fps=30.0)
    assert sum(len(v) for v in want["track_clip_scores"].values()) >= 4
    assert _plain(out) == _plain(want)                        # key for key, the score bits included
    _same_trace(r.trace, host.trace)
    assert det.batches == [detect_batch] * (FRAMES // detect_batch) + ([FRAMES % detect_batch] if FRAMES % detect_batch else [])
    for c in r.chunks:                                        # one wait per chunk and one per flush; the host mode takes two
        assert c["wait"] == (1 + c["closes"] if c["frames"] else c["closes"]), c
        assert c.get("track", 0) == c["detect"] == (1 if c["frames"] else 0), c
        assert c["quality"] <= 2
    for c in host.chunks:
        assert c["wait"] == (2 + c["closes"] if c["frames"] else c["closes"]) and c.get("track", 0) == 0, c
    same = _runner(_StubDetector(script), detect_batch=detect_batch)              # the host mode on the same chunks
    same.run([f for f, _ in script], fps=30.0)
    for mine, its in zip(r.chunks, same.chunks):              # the full-size launch only while _qstat is short; the host mode
        assert mine["quality"] == its["quality"] or (its["quality"] == 0 and mine["quality"] in (1, 2)), (mine, its)      # launches nothing for a chunk without a face
    assert r.chunks[0]["quality"] == 2 and (detect_batch == 16 or [c for c in r.chunks if c["frames"]][-1]["quality"] == 1)
    assert out["stats"]["track"] == sum(1 for c in r.chunks if c["frames"])


def test_c_rgb_frames_on_the_device_path(script, host_run):
    reversed_frames = [np.ascontiguousarray(f[..., ::-1]) for f, _ in script]
    r = _runner(_StubDetector(script, reversed_frames), channel_order="rgb", detect_batch=16, tracker="device")
    assert _plain(r.run(reversed_frames, fps=30.0)) == _plain(host_run[0])
    _same_trace(r.trace, host_run[1].trace)


def test_c_i420_frames_on_the_device_path():
    h, w = 96, 132
    rng = np.random.default_rng(12)
    planes, bgr = [], []
    for f in range(FRAMES):
        y, u, v = rng.integers(16, 236, (h, w), dtype=np.uint8), rng.integers(96, 160, (h // 2, w // 2), dtype=np.uint8), \
            rng.integers(96, 160, (h // 2, w // 2), dtype=np.uint8)
        if f in BLURRY:
            y[:72, :70], u[:36, :35], v[:36, :35] = 90, 128, 128
        planes.append((y, u, v))
        bgr.append(yuv_ref.planes_to_bgr(y, u, v))
    script = list(zip(bgr, _rows()))
    yuv = [af_mi355x.YuvFrame("i420", y, u, v) for y, u, v in planes]
    host = _runner(_StubDetector(script), detect_batch=16)
    want = host.run(yuv, fps=30.0)
    assert sum(len(v) for v in want["track_clip_scores"].values()) >= 4
    r = _runner(_StubDetector(script), detect_batch=16, tracker="device")
    assert _plain(r.run(yuv, fps=30.0)) == _plain(want)
    _same_trace(r.trace, host.trace)


class _Crowd:
    """a detector that sees 33 faces in the third frame it is shown"""

    def __init__(self):
        self.shown = 0

    def detect(self, frames_u8):
        b = frames_u8.shape[0]
        rows = torch.zeros(b, 40, 15, dtype=torch.float32)
        counts = torch.zeros(b, dtype=torch.int32)
        for k in range(b):
            n = 33 if self.shown == 2 else 1
            for i in range(n):
                rows[k, i, :5] = torch.tensor([2.0 + 3 * i, 2.0, 40.0, 44.0, 0.9])
            counts[k] = n
            self.shown += 1
        return rows.to(frames_u8.device), counts.to(frames_u8.device)


@pytest.mark.parametrize("detect_batch", [1, 4])
def test_c_more_faces_than_the_tracker_holds_raise(detect_batch):
    frames = [np.zeros((H, W, 3), dtype=np.uint8) for _ in range(8)]
    r = _runner(_Crowd(), detect_batch=detect_batch, detect_every=1, tracker="device")
    with pytest.raises(RuntimeError, match=r"frame 2: more than AF_TRACK_MAX_DETS = 32 detections"):
        r.run(frames, fps=30.0)
