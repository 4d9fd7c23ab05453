"""GPU: cv2.resize on the device (csrc/af_resize.hip, frames.FrameResizer) and detection on downscaled frames on top of it.

  kernel        byte equality with tests/resize_ref.py for nine H x W -> dh x dw cases (the 2 x 2 path, bilinear down and up, a
                copy, 1 x 1), sources with a row pitch of 3 w + 5, destinations with a padded pitch, 4-byte aligned and not; every
                byte outside the dh rows of 3 dw bytes - pitch padding, the guards around every job and around the buffer - keeps
                its value.  One launch of 64 jobs of mixed geometries out of three stores (one of them B, G, R): every job equals
                the restatement and its own single-job launch; two runs are bitwise equal; a launch whose n differs from the
                table's writes nothing; one launch of 2112 tiles, more than its grid of 2048 workgroups
  FrameResizer  a batch tensor, pitched views of several sizes and (FrameStore, slot) pairs, in one launch each
  scale_detect  FaceDetector.scale_detect on 359 x 641 and 240 x 320 frames equals post_detect(detect(resize_ref frames)), row for row
  YuNet         detect_resized equals detect on the host-resized frame followed by the float64 scaling; infer_resized likewise
  VideoScorer   scale_detect=True: the detections are get_valid_faces(post_detect(detect(resize_ref frames))) per batch of 50, the
                result is that of the same scorer handed those detections
  RealtimeCall  detect_size=(80, 60) over a script of 30 frames of 96 x 128: the detector is shown resize_ref(frame), and tids,
                scores and detections equal a RealtimeCall without a detect size whose detector returns the scaled-back rows
  CallServer    two calls of 96 x 128 and 72 x 100 with one detect size: one detect call and one resize launch per tick
                (ServerStats); per call the tids and detections are a lone RealtimeCall's with that detect_size, and so are the
                scores, bit for bit, on the ticks where only that call closes windows (the server scores the windows of all calls
                of a tick in one batch, so on other ticks the batch differs); on every tick the results equal, bit for bit, those
                of a server without a detect size whose detector returns the scaled-back rows
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import af_mi355x
import resize_ref as R
from conftest import GOLDEN
from af_mi355x import _lib, evaluator, frames as F, retinaface as rf, synth
from af_mi355x.classifier import Classifier, I3D8x8

pytestmark = pytest.mark.gpu
L = _lib.lib
GUARD, FILL = 64, 0xA5


# ---- the kernel --------------------------------------------------------------------------------------------------------------------

def _store(frames, bgr=0):
    """(n, h, w, 3) host frames -> (device buffer, af_store_ref): rows 3 w + 5 bytes apart, frames h * pitch + 11 bytes apart"""
    n, h, w, _ = frames.shape
    pitch = 3 * w + 5
    stride = h * pitch + 11
    host = np.full(n * stride, 0x5A, np.uint8)
    np.lib.stride_tricks.as_strided(host, (n, h, 3 * w), (stride, pitch, 1))[:] = frames.reshape(n, h, 3 * w)
    dev = torch.from_numpy(host).cuda()
    return dev, _lib.StoreRef(dev.data_ptr(), _lib.FrameStore(n * stride, stride, pitch, n, h, w, 0), bgr, 0)


def _layout(sizes, aligned):
    """where each job's rows go in one destination buffer: [(offset, pitch)], the buffer's size.  aligned: pitches and offsets are
    multiples of 4 (dword stores); else the pitch is 3 dw + 7 rounded up to odd and every job starts at an odd address"""
    places, at = [], GUARD
    for dw, dh in sizes:
        pitch = -(-(3 * dw + 4) // 4) * 4 if aligned else (3 * dw + 7) | 1
        at = -(-at // 4) * 4 + (0 if aligned else 1)
        places.append((at, pitch))
        at += dh * pitch + GUARD
    return places, at


def _launch(refs, jobs, aligned, out=None, n_launch=None, header=None):
    """jobs = [(store, frame, dw, dh)] in ONE launch -> (the whole destination buffer as numpy, the layout); a list handed in as
    `header` receives the planned table's af_resize_header"""
    places, total = _layout([(dw, dh) for _, _, dw, dh in jobs], aligned)
    if out is None:
        out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    arr = (_lib.ResizeJob * len(jobs))(*[_lib.ResizeJob(s, f, out.data_ptr() + off, pitch, dh, dw) for (s, f, dw, dh), (off, pitch) in zip(jobs, places)])
    stores = (_lib.StoreRef * len(refs))(*refs)
    need = L.af_resize_table_bytes(C.byref(arr), len(jobs))
    table = torch.zeros(need // 8 + 1, dtype=torch.int64)
    used = C.c_int64(0)
    _lib.check(L.af_resize_plan_u8(C.byref(arr), len(jobs), C.byref(stores), len(refs), C.c_void_p(table.data_ptr()), need, C.byref(used)), "plan")
    if header is not None:
        header.append(_lib.ResizeHeader.from_buffer_copy(table.numpy().tobytes()[:C.sizeof(_lib.ResizeHeader)]))
    table_dev = table.cuda()
    _lib.check(L.af_resize_frames_u8(C.c_void_p(table_dev.data_ptr()), len(jobs) if n_launch is None else n_launch,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "launch")
    torch.cuda.synchronize()
    return out.cpu().numpy(), places


def _expected(total, places, images):
    want = np.full(total, FILL, np.uint8)
    for (off, pitch), im in zip(places, images):
        dh, dw = im.shape[:2]
        np.lib.stride_tricks.as_strided(want[off:], (dh, 3 * dw), (pitch, 1))[:] = im.reshape(dh, 3 * dw)
    return want


def _rows(buf, place, dw, dh):
    off, pitch = place
    return np.lib.stride_tricks.as_strided(buf[off:], (dh, 3 * dw), (pitch, 1)).reshape(dh, dw, 3).copy()


CASES = [(16, 24, 8, 12), (2, 2, 1, 1), (13, 27, 6, 13), (359, 641, 179, 320), (11, 24, 5, 12), (16, 32, 4, 8), (5, 7, 11, 16), (40, 64, 40, 64),
         (1, 1, 3, 3)]
_REF = {}


def _case(h, w, dh, dw):
    """the source frames of a case and their restated resize, computed once"""
    if (h, w, dh, dw) not in _REF:
        src = np.random.default_rng(h * 1000 + w).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        _REF[(h, w, dh, dw)] = (src, [R.resize_linear(f, dw, dh) for f in src])
    return _REF[(h, w, dh, dw)]


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("h,w,dh,dw", CASES, ids=["%dx%d-%dx%d" % c for c in CASES])
def test_the_launch_equals_the_restatement_and_writes_nothing_else(h, w, dh, dw, aligned):
    src, want = _case(h, w, dh, dw)
    dev, ref = _store(src)
    got, places = _launch([ref], [(0, 1, dw, dh), (0, 0, dw, dh)], aligned)
    expect = _expected(got.size, places, [want[1], want[0]])
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, "%d bytes differ, the first at %d (rows at %s)" % (bad.size, bad[0], places)
    assert (dev.cpu().numpy() == _store(src)[0].cpu().numpy()).all()             # the source is only read


def _mixed():
    rng = np.random.default_rng(17)
    stores = [rng.integers(0, 256, (4, 13, 27, 3), dtype=np.uint8), rng.integers(0, 256, (3, 16, 24, 3), dtype=np.uint8),
              rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)]
    sizes = [[(13, 6), (27, 13), (9, 4), (28, 13)], [(12, 8), (12, 5), (24, 16), (8, 4), (1, 1)], [(16, 11), (7, 5), (3, 2)]]      # (dw, dh)
    jobs = [(i % 3, (i // 3) % len(stores[i % 3]), *sizes[i % 3][(i // 3) % len(sizes[i % 3])]) for i in range(64)]
    return stores, jobs


def test_sixty_four_mixed_jobs_out_of_three_stores_in_one_launch():
    stores, jobs = _mixed()
    held = [_store(s, bgr=int(k == 1)) for k, s in enumerate(stores)]             # the second store is B, G, R: bytes pass through
    refs = [r for _, r in held]
    assert len({(s, dw, dh) for s, _, dw, dh in jobs}) == 12
    want = [R.resize_linear(stores[s][f], dw, dh) for s, f, dw, dh in jobs]
    for aligned in (True, False):
        got, places = _launch(refs, jobs, aligned)
        assert np.array_equal(got, _expected(got.size, places, want))
        again, _ = _launch(refs, jobs, aligned)
        assert np.array_equal(again, got)                                        # run to run
        if aligned:
            for i, (s, f, dw, dh) in enumerate(jobs):                            # each job alone: the same bytes
                alone, place = _launch(refs, [(s, f, dw, dh)], aligned)
                assert np.array_equal(_rows(alone, place[0], dw, dh), _rows(got, places[i], dw, dh)), i


BIG = [(66, 512), (132, 1024), (100, 700)]           # h x w -> 66 x 512: a copy, the 2 x 2 path, bilinear


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
def test_a_launch_of_more_tiles_than_workgroups(aligned):
    """64 jobs of 128 runs x 66 rows = 33 tiles each: 2112 tiles for a grid of 2048 workgroups, so the first 64 workgroups take a
    second tile (the last two jobs: a copy and the 2 x 2 path when aligned, bilinear and a copy when not)"""
    assert not R.is_area2(512, 66, 512, 66) and R.is_area2(1024, 132, 512, 66) and not R.is_area2(700, 100, 512, 66)
    held = [_store(_case(h, w, 66, 512)[0]) for h, w in BIG]
    jobs = [((i + int(aligned)) % 3, (i // 3) % 2, 512, 66) for i in range(64)]
    want = [_case(*BIG[s], 66, 512)[1][f] for s, f, _, _ in jobs]
    header = []
    got, places = _launch([r for _, r in held], jobs, aligned, header=header)
    assert header[0].total_tiles == 64 * 33 > 2048                               # the launch's grid, which _lib does not export
    bad = np.flatnonzero(got != _expected(got.size, places, want))
    assert bad.size == 0, "%d bytes differ, the first at %d (rows at %s)" % (bad.size, bad[0], places[:3])


def test_a_launch_whose_n_differs_from_the_tables_writes_nothing():
    src, _ = _case(13, 27, 6, 13)
    _, ref = _store(src)
    for n_launch in (1, 3):
        got, _ = _launch([ref], [(0, 0, 13, 6), (0, 1, 13, 6)], True, n_launch=n_launch)
        assert (got == FILL).all()


# ---- FrameResizer ------------------------------------------------------------------------------------------------------------------

def test_frame_resizer_takes_batches_views_and_store_slots():
    rng = np.random.default_rng(3)
    rs = F.FrameResizer("cuda")
    batch = rng.integers(0, 256, (3, 24, 36, 3), dtype=np.uint8)
    out = rs.resize(torch.from_numpy(batch).cuda(), (18, 12))
    assert out.shape == (3, 12, 18, 3) and out.dtype == torch.uint8 and rs.launches == 1
    assert np.array_equal(out.cpu().numpy(), np.stack([R.resize_linear(f, 18, 12) for f in batch]))
    assert rs.resize(torch.from_numpy(batch).cuda(), (18, 12)).data_ptr() == out.data_ptr()        # one buffer per (B, size), re-used
    wide = torch.from_numpy(rng.integers(0, 256, (30, 50, 3), dtype=np.uint8)).cuda()
    small = torch.from_numpy(rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)).cuda()
    store = evaluator.FrameStore(torch.device("cuda", torch.cuda.current_device()))
    kept = [rng.integers(0, 256, (20, 31, 3), dtype=np.uint8) for _ in range(3)]
    with torch.cuda.device(store.device):
        store.open((20, 31, 3), 3)
        store.put(kept, 0)
    views = [wide[3:28, 5:45], small, (store, 2), (store, 0)]                     # a pitched view: 25 x 40 of 30 x 50
    out = rs.resize_views(views, (10, 7)).cpu().numpy()
    assert rs.launches == 3
    for got, im in zip(out, [wide[3:28, 5:45].cpu().numpy(), small.cpu().numpy(), kept[2], kept[0]]):
        assert np.array_equal(got, R.resize_linear(im, 10, 7))
    with pytest.raises(ValueError, match="a destination of 0x4"):
        rs.resize(views, (0, 4))
    with pytest.raises(ValueError, match="packed pixels"):
        rs.resize([wide[:, ::2]], (4, 4))
    with pytest.raises(ValueError, match="slot 3"):
        rs.resize([(store, 3)], (4, 4))


# ---- FaceDetector.scale_detect -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "retinaface.json")) as f:
        return json.load(f)


_DETECTORS = {}


def _detector(golden, recipe):
    if recipe not in _DETECTORS:
        _DETECTORS[recipe] = rf.FaceDetector.from_state_dict(synth.retinaface_state_dict(golden["weight_seed"], recipe), gpu_id=0)
    return _DETECTORS[recipe]


def _same_faces(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for (box, ldm, score), (box2, ldm2, score2) in zip(got, want):
        assert box.dtype == box2.dtype and ldm.shape == (5, 2) and np.array_equal(box, box2) and np.array_equal(ldm, ldm2) and score == score2


@pytest.mark.parametrize("h,w", [(359, 641), (240, 320)])
def test_scale_detect_equals_detect_on_host_resized_frames(golden, h, w):
    det = _detector(golden, "dense")
    seeds = [c["frame_seed"] for c in golden["cases"] if (c["h"], c["w"]) == (h, w)]
    frames = [synth.retinaface_frames(1, h, w, seed=s)[0] for s in seeds]
    dw, dh = R.scale_detect_size(h, w)
    assert (dw, dh) == (w // 2, h // 2) and R.is_area2(w, h, dw, dh) == (h % 2 == 0 and w % 2 == 0)
    small = [R.resize_linear(f, dw, dh) for f in frames]
    raw = det.detect(small)
    want = R.post_detect(raw, R.scale_detect_scale(h, w), w, h)
    got = det.scale_detect(frames)
    print("scale_detect %dx%d: faces found / kept per frame" % (w, h), [(len(a), len(b)) for a, b in zip(raw, want)])
    assert sum(len(f) for f in want) >= 1
    for a, b in zip(got, want):
        _same_faces(a, b)
    _same_faces(det.scale_detect(frames[0]), want[0])                           # one HWC frame: the single list
    rows, counts, scale = det.scale_detect_device(torch.from_numpy(np.stack(frames)).cuda())
    rows2, counts2 = det.detect_device(torch.from_numpy(np.stack(small)).cuda())
    assert scale == 2 and torch.equal(counts, counts2) and all(torch.equal(rows[b, :int(counts[b])], rows2[b, :int(counts[b])]) for b in range(len(frames)))


# ---- YuNet -------------------------------------------------------------------------------------------------------------------------

def test_yunet_detect_resized_equals_detect_on_the_host_resized_frame_scaled_back():
    from af_mi355x.detector import YuNet
    from test_hip_yunet import MODEL, frames as yunet_frames
    det = YuNet(MODEL, confThreshold=0.05)
    fr = yunet_frames(3, 641, 359, seed=51)
    dev = torch.device("cuda", torch.cuda.current_device())
    total = 0
    for dw, dh in ((320, 320), (320, 179)):
        got = det.detect_resized(torch.from_numpy(fr).to(dev), (dw, dh))
        for b in range(len(fr)):
            rows, counts = det.detect(torch.from_numpy(R.resize_linear(fr[b], dw, dh)[None]).to(dev))
            want = rows[0, :int(counts[0])].cpu().numpy().astype(np.float64) * np.array([641 / dw, 359 / dh] * 7 + [1.0])
            assert got[b].dtype == np.float64 and got[b].shape == want.shape and np.array_equal(got[b], want), (dw, dh, b)
            assert len(want) == 0 or np.array_equal(got[b][:, 14], rows[0, :len(want), 14].cpu().numpy().astype(np.float64))     # the score is untouched
            total += len(want)
        one = det.infer_resized(fr[0], (dw, dh))
        assert np.array_equal(one, got[0]) if len(got[0]) else one.shape == (0, 5)
    print("yunet detect_resized: %d faces compared" % total)
    assert total >= 1
    views = [torch.from_numpy(fr[0]).to(dev), torch.from_numpy(np.ascontiguousarray(fr[1][:300, :500])).to(dev)]       # two sizes, one call
    got = det.detect_resized(views, (320, 320))
    for v, g in zip(views, got):
        rows, counts = det.detect(torch.from_numpy(R.resize_linear(v.cpu().numpy(), 320, 320)[None]).to(dev))
        want = rows[0, :int(counts[0])].cpu().numpy().astype(np.float64) * np.array([v.shape[1] / 320, v.shape[0] / 320] * 7 + [1.0])
        assert np.array_equal(g, want)


# ---- VideoScorer -------------------------------------------------------------------------------------------------------------------

SHIFTS = [(0, 0), (0, 0), (1, 2)]
N_VIDEO = 52                         # two detector batches


def test_video_scorer_scale_detect(golden, weights0):
    case = next(c for c in golden["cases"] if c["name"] == "dense_359x641")
    det = _detector(golden, "dense")
    frame = synth.retinaface_frames(1, case["h"], case["w"], seed=case["frame_seed"])[0]
    frames = [np.ascontiguousarray(np.roll(frame, SHIFTS[i % len(SHIFTS)], axis=(0, 1))) for i in range(N_VIDEO)]
    h, w = frame.shape[:2]
    dw, dh = R.scale_detect_size(h, w)
    raw = []
    for lo in range(0, N_VIDEO, 50):
        raw += R.post_detect(det.detect([R.resize_linear(f, dw, dh) for f in frames[lo:lo + 50]]), R.scale_detect_scale(h, w), w, h)
    want = evaluator.get_valid_faces(raw, thres=0.5)
    assert min(len(f) for f in want) >= 1
    clf = Classifier(precision="f16")
    clf.network.load_state_dict(weights0)
    net = clf.cuda().eval()
    vs = evaluator.VideoScorer(det, net, scale_detect=True)
    res = vs.score(frames)
    assert len(res["detections"]) == N_VIDEO
    for a, b in zip(res["detections"], want):
        assert all(f[0].dtype == np.float64 for f in a)
        _same_faces(a, b)
    assert vs.uploaded_bytes == sum(f.nbytes for f in frames)
    handed = vs.score(frames, detections=want)
    assert res["video_score"] == handed["video_score"] and res["pred_label"] == handed["pred_label"] and res["spans"] == handed["spans"]
    assert len(res["preds"]) == len(handed["preds"]) >= 1 and all(a == b for a, b in zip(res["preds"], handed["preds"]))
    assert res["frame_res"] == handed["frame_res"]
    plain = evaluator.VideoScorer(det, net)                                      # the default detects at full size, as before
    assert plain.scale_detect is False


# ---- RealtimeCall and CallServer ---------------------------------------------------------------------------------------------------

CLIP, SIZE = 8, 64
DROP, STRIDE, STEPS = 6, 3, 30
RING = CLIP + DROP
GATE = dict(q_min_size_soft=24, q_min_size_hard=12, q_lap_soft=20.0, q_lap_hard=5.0)
ARGS = dict(stride=STRIDE, ring_frames=RING, drop_after=DROP, start_conf=0.76, start_min_size=20, exclude_rect=(0.70, 0.70, 1.00, 1.00), **GATE)
_nets = {}


def _net():
    if "i3d" not in _nets:
        net = I3D8x8(clip_size=CLIP, crop_size=SIZE, precision="f16")
        net.load_state_dict(synth.synthetic_state_dict(net.spec, seed=5))
        _nets["i3d"] = net.cuda().eval()
    return _nets["i3d"]


def _script(h, w, size, seed, face1, face2):
    """per step: the frame, the rows the detector finds on the frame resized to `size` (the layout the existing realtime scripts
    use: x, y, w, h, score, five landmarks), and those rows scaled back by hand - float64, columns alternately times W / dw and
    H / dh, the last one untouched"""
    rng = np.random.default_rng(seed)
    std = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
    vec = np.array([w / size[0], h / size[1]] * 7 + [1.0], dtype=np.float64)
    out = []
    for s in range(STEPS):
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rows = []
        for (x, y, dx, dy, fw, fh), sc in zip((face1, face2), (0.95, 0.93)):
            j = rng.uniform(-0.3, 0.3, 4)
            x, y, fw, fh = x + dx * s + j[0], y + dy * s + j[1], fw + j[2], fh + j[3]
            lm = std * [fw, fh] + [x, y] + rng.normal(0, 0.4, (5, 2))
            rows.append(np.concatenate([[x, y, fw, fh], [sc + rng.uniform(-0.004, 0.004)], lm.ravel()]))
        found = (np.asarray(rows, dtype=np.float64) / vec).astype(np.float32)   # on the resized frame
        out.append((frame, found, found.astype(np.float64) * vec))
    return out


class _Stub:
    """scripted rows, looked up by the bytes of the frame the detector is shown (KeyError: it was shown something else)"""

    def __init__(self, rows_by_frame, shape=None):
        self.rows, self.shape, self.calls = rows_by_frame, shape, 0

    def _answer(self, views):
        dev = views[0].device
        rows = torch.zeros(len(views), 16, 15, dtype=torch.float32, device=dev)
        counts = []
        for b, v in enumerate(views):
            assert self.shape is None or tuple(v.shape) == self.shape
            mine = self.rows[v.cpu().numpy().tobytes()]
            rows[b, :len(mine)] = torch.from_numpy(np.asarray(mine, dtype=np.float32)).to(dev)
            counts.append(len(mine))
        self.calls += 1
        return rows, torch.tensor(counts, dtype=torch.int32, device=dev)

    def detect(self, frames_u8):
        assert frames_u8.is_cuda and frames_u8.shape[0] == 1
        return self._answer([frames_u8[0]])

    def detect_views(self, views):
        return self._answer(list(views))


def _stubs(scripts, size):
    """(a detector that must be shown resize_ref(frame) and answers on it, one that is shown the frame and answers the scaled-back rows)"""
    small = {R.resize_linear(f, *size).tobytes(): found for sc in scripts for f, found, _ in sc}
    full = {f.tobytes(): back for sc in scripts for f, _, back in sc}
    return _Stub(small, (size[1], size[0], 3)), _Stub(full)


def test_realtime_call_detects_on_the_resized_frame():
    size = (80, 60)
    script = _script(96, 128, size, 4, (14, 22, 0.5, 0.1, 30, 34), (52, 40, 0.3, 0.2, 28, 32))
    on_small, on_full = _stubs([script], size)
    call = af_mi355x.RealtimeCall(_net(), detector=on_small, clip_size=CLIP, size=SIZE, detect_size=size, **ARGS)
    hand = af_mi355x.RealtimeCall(_net(), detector=on_full, clip_size=CLIP, size=SIZE, **ARGS)
    assert call.detect_size == size and hand.detect_size is None
    closed = 0
    for s, (frame, _, back) in enumerate(script):
        got, want = call.step(frame), hand.step(frame)
        assert got == want, (s, got, want)
        assert call.detections.dtype == np.float64 and np.array_equal(call.detections, back)
        assert np.array_equal(call.detections.astype(np.float32), hand.detections)
        assert sorted(call.purged) == sorted(hand.purged) and call.state == hand.state and call.uploaded_bytes == (s + 1) * frame.nbytes
        closed += len(got)
    assert closed >= 2 and on_small.calls == STEPS
    with pytest.raises(ValueError, match="detect_size"):
        af_mi355x.RealtimeCall(_net(), detector=on_small, clip_size=CLIP, size=SIZE, detect_size=(0, 4), **ARGS)


def test_call_server_shares_one_detect_call_and_one_resize_launch():
    size = (64, 48)                                                             # 96 x 128 -> the 2 x 2 path; 72 x 100 -> bilinear
    scripts = {"A": _script(96, 128, size, 4, (14, 22, 0.5, 0.1, 30, 34), (52, 40, 0.3, 0.2, 28, 32)),
               "B": _script(72, 100, size, 6, (8, 20, 0.25, 0.1, 30, 34), (40, 26, 0.3, 0.1, 28, 32))}
    orders = {"A": "bgr", "B": "rgb"}
    on_small, on_full = _stubs(scripts.values(), size)
    server = af_mi355x.CallServer(_net(), detector=on_small, clip_size=CLIP, size=SIZE, detect_size=size, **ARGS)
    plain = af_mi355x.CallServer(_net(), detector=on_full, clip_size=CLIP, size=SIZE, **ARGS)        # the same launches, handed the scaled-back rows
    lone = {n: af_mi355x.RealtimeCall(_net(), detector=on_small, clip_size=CLIP, size=SIZE, detect_size=size, channel_order=orders[n], **ARGS)
            for n in scripts}
    ids = {n: server.open(channel_order=orders[n]) for n in scripts}
    ids2 = {n: plain.open(channel_order=orders[n]) for n in scripts}
    assert server.call(ids["A"]).detect_size == size and plain.call(ids2["A"]).detect_size is None
    assert server.stats.last["resize"] == 0
    closed = alone = 0
    for s in range(STEPS):
        tick = {"A": s} if s == 0 else {"A": s, "B": s - 1}                     # B joins a tick later: its windows close on other ticks
        before = on_small.calls
        got = server.step({ids[n]: scripts[n][k][0] for n, k in tick.items()})
        assert server.stats.last["detect"] == 1 and server.stats.last["resize"] == 1 and on_small.calls == before + 1, (s, dict(server.stats.last))
        want = plain.step({ids2[n]: scripts[n][k][0] for n, k in tick.items()})
        closing = [n for n in tick if got[ids[n]]]
        for n, k in tick.items():
            assert got[ids[n]] == want[ids2[n]], (s, n)                           # bit for bit: the same batches
            mine = lone[n].step(scripts[n][k][0])
            assert [t for t, _ in mine] == [t for t, _ in got[ids[n]]], (s, n)
            if closing == [n]:                                                  # the tick's only windows: the lone call scores the same batch
                assert mine == got[ids[n]], (s, n)
                alone += 1
            c = server.call(ids[n])
            assert np.array_equal(c.detections, scripts[n][k][2]) and np.array_equal(c.detections, lone[n].detections)
            assert c.state.keys() == lone[n].state.keys() and sorted(c.purged) == sorted(lone[n].purged)
        closed += sum(len(v) for v in got.values())
    assert closed >= 4 and alone >= 4, (closed, alone)
    assert server.stats.total["resize"] == STEPS and server.stats.total["detect"] == STEPS
