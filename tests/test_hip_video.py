"""GPU: VideoScorer (evaluator.py) - frames in, video score out, on one device-resident copy of the frames.

  warp          af_warp_affine_window_rects_u8 on rectangles of resident 359x641 frames (row pitch 1 923 bytes) EQUALS
                TrackScorer.aligned_windows on crops cut from the same frames on the host, every byte; the same again with the
                frame outside every rectangle set to 255 and to 0 (no neighbouring pixel reaches the result)
  header        a launch whose n_windows / clip_size / size differ from the table's writes nothing
  scores        VideoScorer.score with injected detections EQUALS TrackScorer.score_video on host-cut crops of the same tracks:
                preds, frame_res and video_score bit for bit, f16 and bf16, and again with a frame store that forces two segments
  end to end    a video of one recorded RetinaFace fixture frame repeated and shifted by whole pixels: detections equal
                FaceDetector.detect + get_valid_faces, the result equals detect -> tracks -> score_video, each frame uploaded once
  repeatable    run to run and from two streams at once
"""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from af_mi355x import _lib, aligner, evaluator, retinaface as rf, synth
from af_mi355x.classifier import Classifier

pytestmark = pytest.mark.gpu
H, W = 359, 641

_nets = {}


def _net(dtype, weights0, copy=0):
    if (dtype, copy) not in _nets:
        clf = Classifier(precision=dtype)
        clf.network.load_state_dict(weights0)
        _nets[(dtype, copy)] = clf.cuda().eval()
    return _nets[(dtype, copy)]


# ---- 1. the warp ----------------------------------------------------------------------------------------------------------------

def _five(rng, rect):
    """five landmarks inside a rectangle, relative to its corner (what crop_records hands the aligner)"""
    x0, y0, x1, y1 = rect
    std = (aligner.STD_POINTS_317 - aligner.STD_POINTS_317.mean(0)) / 317.0
    return std * max(8.0, min(x1 - x0, y1 - y0)) + [(x1 - x0) / 2.0, (y1 - y0) / 2.0] + rng.normal(0, 0.7, (5, 2))


def _face_rects(rng, n):
    out = []
    for _ in range(n):
        w, h = int(rng.integers(120, 200)), int(rng.integers(120, 200))
        x0, y0 = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        out.append((x0, y0, x0 + w, y0 + h))
    return out


def _warp_case(name):
    """(number of frames, clip_size, size, batch, rectangles per track position, windows)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "corners_and_slivers":                             # (0, 0); the last pixel of the last frame of the store; 1 and 2 wide
        rects = _face_rects(rng, 6)
        rects[0] = (0, 0, 150, 140)
        rects[2] = (300, 100, 301, 260)
        rects[3] = (400, 90, 402, 250)
        rects[5] = (W - 160, H - 130, W, H)
        return 6, 4, 224, 16, rects, evaluator.clip_windows(6, 4)
    if name == "padded_short_track":                              # T = 3: one window of 32 with repeated indices, n = 1
        return 7, 32, 224, 16, _face_rects(rng, 3), evaluator.clip_windows(3, 32)
    if name == "sixteen_windows_224":
        return 40, 25, 224, 16, _face_rects(rng, 40), evaluator.clip_windows(40, 25)
    if name == "sixteen_windows_64_in_batches_of_5":
        return 40, 25, 64, 5, _face_rects(rng, 40), evaluator.clip_windows(40, 25)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["corners_and_slivers", "padded_short_track", "sixteen_windows_224", "sixteen_windows_64_in_batches_of_5"])
def test_rectangles_of_resident_frames_equal_host_cut_crops(name, weights0):
    n_frames, clip, size, batch, rects, windows = _warp_case(name)
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n_frames)]
    T = len(rects)
    frame_ids = [n_frames - T + j for j in range(T)]             # the track ends with the last frame of the store
    infos = [(None, _five(rng, r), None, np.array(r)) for r in rects]
    if name == "corners_and_slivers":
        assert rects[0][:2] == (0, 0) and rects[5][2:] == (W, H) and frame_ids[5] == n_frames - 1
        assert {r[2] - r[0] for r in rects} >= {1, 2}
    if name == "padded_short_track":
        assert len(windows) == 1 and len(set(windows[0])) == 3
    if name.startswith("sixteen"):
        assert len(windows) == 16
    net = _net("f16", weights0)
    crops = [frames[f][r[1]:r[3], r[0]:r[2]] for f, r in zip(frame_ids, rects)]
    want = evaluator.TrackScorer(net, clip_size=clip, size=size, batch=batch).aligned_windows(infos, crops, windows).cpu().numpy()
    assert want.any() and want.shape == (len(windows), clip, size, size, 3)
    vs = evaluator.VideoScorer(None, net, clip_size=clip, size=size, batch=batch)
    got = vs.aligned_windows(frames, frame_ids, infos, windows)
    assert got.is_cuda and got.dtype == torch.uint8
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "differs in %d bytes" % int((got != want).sum())
    assert vs.uploaded_bytes == sum(f.nbytes for f in frames)
    for fill in (255, 0):                                         # nothing outside a rectangle may reach the result
        walled = [np.full((H, W, 3), fill, dtype=np.uint8) for _ in range(n_frames)]
        for f, r in zip(frame_ids, rects):
            walled[f][r[1]:r[3], r[0]:r[2]] = frames[f][r[1]:r[3], r[0]:r[2]]
        got = vs.aligned_windows(walled, frame_ids, infos, windows).cpu().numpy()
        assert np.array_equal(got, want), "fill %d: differs in %d bytes" % (fill, int((got != want).sum()))


# ---- 2. the header ---------------------------------------------------------------------------------------------------------------

def test_a_launch_that_does_not_match_its_table_writes_nothing():
    RECT = evaluator._RECT_DTYPE
    n, clip, size = 2, 3, 8
    store = torch.randint(0, 256, (4 * H * W * 3 + 16,), dtype=torch.uint8, device="cuda")
    desc = np.zeros(n, dtype=evaluator._WINDOW_DTYPE)
    rects = np.zeros((n, clip), dtype=RECT)
    for w in range(n):
        desc[w] = ([0.05, 0.0, 0.0, 0.0, 0.05, 0.0], 100, 120)
        for t in range(clip):
            rects[w, t] = (w + t, 10 * t, 20, 100, 120, 0, 0, 0)
    table = np.zeros(_lib.lib.af_window_rects_table_bytes(n, clip) // 8, dtype=np.int64)
    st = _lib.FrameStore(store.numel(), H * W * 3, W * 3, 4, H, W, 0)
    assert _lib.lib.af_window_rects_plan_u8(desc.ctypes.data, rects.ctypes.data, n, clip, size, C.byref(st), table.ctypes.data, table.nbytes,
                                            None, None) == 0, _lib.lib.af_last_error()
    dev_table = torch.from_numpy(table).cuda()
    out = torch.full((n * clip * size * size * 3,), 0xAB, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    launch = lambda fn, a, b, c: getattr(_lib.lib, fn)(C.c_void_p(store.data_ptr()), C.c_void_p(dev_table.data_ptr()), a, b, c,  # noqa: E731
                                                       C.c_void_p(out.data_ptr()), stream)
    for a, b, c in ((1, clip, size), (n, clip - 1, size), (n, clip, 4)):
        assert launch("af_warp_affine_window_rects_u8", a, b, c) == 0
        torch.cuda.synchronize()
        assert bool((out == 0xAB).all()), (a, b, c)
    assert launch("af_warp_affine_windows_u8", n, clip, size) == 0  # the pool form's launch does not take a table of rectangles
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    assert launch("af_warp_affine_window_rects_u8", n, clip, size) == 0
    torch.cuda.synchronize()
    assert not bool((out == 0xAB).all())


# ---- 3. scores with injected detections --------------------------------------------------------------------------------------------

def _crossing_video(seed, n_frames=40, shape=(360, 640, 3)):
    """frames and detect_all-style detections of two faces that walk through each other"""
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n_frames)]
    std = (aligner.STD_POINTS_317 - aligner.STD_POINTS_317.mean(0)) * (45.0 / 90.0) * (180.0 / 317.0)
    detections = []
    for i in range(n_frames):
        faces = []
        for cx, cy, score in ((150.0 + 8.5 * i, 150.0, 0.99), (490.0 - 8.5 * i, 190.0, 0.95)):
            cx, cy = cx + rng.normal(0, 1.0), cy + rng.normal(0, 1.0)
            half = 45.0 + rng.normal(0, 0.5)
            box = np.array([cx - half, cy - half, cx + half, cy + half], dtype=np.float32)
            faces.append((box, (std + [cx, cy] + rng.normal(0, 0.5, (5, 2))).astype(np.float32), np.float32(score)))
        detections.append(faces)
    return shape, frames, evaluator.get_valid_faces(detections)


def _composition(scorer, shape, frames, detections, threshold=0.04):
    """the parent's way: tracks on the host, crops cut on the host, TrackScorer.score_video"""
    tracks = evaluator.multiple_tracking(detections)
    spans = [(0, len(detections))] * len(tracks)
    if not tracks:
        spans, tracks = evaluator.find_longest(detections)
    with_lm68 = [[(f[0], f[1], np.zeros((0, 2)), f[-1]) for f in t] for t in tracks]
    return scorer.score_video(shape, frames, with_lm68, spans, threshold), tracks, spans


def _same_result(got, want):
    assert got["preds"] == want["preds"] and len(got["preds"]) > 0
    assert got["frame_res"] == want["frame_res"] and got["video_score"] == want["video_score"]
    assert got["pred_label"] == want["pred_label"] and got["clips"] == want["clips"]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_scores_equal_score_video_on_host_cut_crops(dtype, weights0):
    shape, frames, detections = _crossing_video(71)
    net = _net(dtype, weights0)
    want, tracks, spans = _composition(evaluator.TrackScorer(net), shape, frames, detections)
    assert len(tracks) == 2 and len(want["preds"]) == 18
    vs = evaluator.VideoScorer(None, net)
    got = vs.score(frames, detections=detections)
    print(dtype, "preds", got["preds"][:3], "video_score", got["video_score"])
    _same_result(got, want)
    assert got["spans"] == spans and len(got["tracks"]) == 2 and all(a is b for t, u in zip(got["tracks"], tracks) for a, b in zip(t, u))
    assert vs.uploaded_bytes == sum(f.nbytes for f in frames)
    # a frame store of 36 frames: each track goes through it in two segments (windows 0-4, then 5-8 from frame 5 on)
    small = evaluator.VideoScorer(None, net, frame_bytes=36 * frames[0].nbytes + 16)
    cut = small.score(frames, detections=detections)
    track = evaluator._FrameTrack([(None, np.zeros((5, 2)), None, np.array([0, 0, 9, 9]))] * 40, range(40), shape)
    segs = small._segments(track, evaluator.clip_windows(40, 32))
    assert [(a, b, len(ws)) for a, b, ws in segs] == [(0, 36, 5), (5, 40, 4)]                 # neighbours overlap by clip_size - 1 frames
    _same_result(cut, want)
    assert small.uploaded_bytes == 2 * (36 + 35) * frames[0].nbytes
    with pytest.raises(ValueError, match="fewer than"):
        evaluator.VideoScorer(None, net, frame_bytes=20 * frames[0].nbytes).score(frames, detections=detections)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------

SHIFTS = [(0, 0), (0, 0), (1, 2)]     # whole-pixel (down, right) shifts, chosen on the CPU with tests/retinaface_ref.py on the fixture
N_VIDEO = 52                          # frame: seven faces of frame 0 are tracked through them with IoU >= 0.67; two detector batches

_e2e = {}


def _fixture_video():
    if not _e2e:
        with open(os.path.join(GOLDEN, "retinaface.json")) as f:
            g = json.load(f)
        case = next(c for c in g["cases"] if c["name"] == "sparse_359x641")
        recorded = np.load(os.path.join(GOLDEN, "retinaface_dets.npz"))[case["name"]]
        assert (recorded[:10, 4] >= 0.8).sum() >= 3                 # the recorded detections of the frame: faces a track may start from
        frame = synth.retinaface_frames(1, case["h"], case["w"], seed=case["frame_seed"])[0]
        bgr = [np.ascontiguousarray(np.roll(frame, SHIFTS[i % len(SHIFTS)], axis=(0, 1))[..., ::-1]) for i in range(N_VIDEO)]
        _e2e["frames"] = [f[..., ::-1] for f in bgr]               # channel-reversed views, as grab_all_frames(cvt=True) returns them
        _e2e["detector"] = rf.FaceDetector.from_state_dict(synth.retinaface_state_dict(g["weight_seed"], case["recipe"]), gpu_id=0)
    return _e2e["frames"], _e2e["detector"]


def _equal_detections(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert len(a) == len(b)
        for (box, lm, score), (box2, lm2, score2) in zip(a, b):
            assert box.dtype == lm.dtype == np.float64 and np.array_equal(box, box2) and np.array_equal(lm, lm2) and score == score2


def test_frames_in_score_out_equals_the_composition_of_the_stages(weights0):
    frames, det = _fixture_video()
    assert frames[0].strides[2] == -1
    net = _net("f16", weights0)
    vs = evaluator.VideoScorer(det, net)
    res = vs.score(frames)
    raw = []
    for lo in range(0, len(frames), 50):                            # detect_all: partition(frames, 50), flattened, get_valid_faces
        raw += det.detect(frames[lo:lo + 50])
    detections = evaluator.get_valid_faces(raw, thres=0.5)
    _equal_detections(res["detections"], detections)
    want, tracks, spans = _composition(evaluator.TrackScorer(net), frames[0].shape, frames, detections)
    print("tracks", len(tracks), "spans", spans, "windows", len(want["preds"]), "video_score", res["video_score"])
    assert len(tracks) >= 1, "the fixture video yields no track"
    assert len(want["preds"]) >= 2 * vs.batch and max(b - a for a, b in spans) - vs.clip_size + 1 > vs.batch   # two forwards' worth
    _same_result(res, want)
    assert res["spans"] == spans and len(res["tracks"]) == len(tracks)
    for t, u in zip(res["tracks"], tracks):
        _equal_detections([t], [u])
    assert vs.uploaded_bytes == sum(f.nbytes for f in frames)
    _e2e["res"] = res


# ---- 5. repeatable ---------------------------------------------------------------------------------------------------------------

def test_run_to_run_and_two_streams(weights0):
    frames, det = _fixture_video()
    vs = evaluator.VideoScorer(det, _net("f16", weights0))
    first = _e2e.get("res") or vs.score(frames)
    again = vs.score(frames)
    _same_result(again, first)
    _equal_detections(again["detections"], first["detections"])
    # two scorers, each with a network of its own, on two streams at the same time (injected detections: one detector)
    shape, video, detections = _crossing_video(72)
    want = evaluator.VideoScorer(None, _net("f16", weights0)).score(video, detections=detections)
    scorers = [evaluator.VideoScorer(None, _net("f16", weights0, copy)) for copy in (0, 1)]
    got, errors = [None, None], []

    def work(k):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                got[k] = scorers[k].score(video, detections=detections)
        except Exception as e:                                      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    _same_result(got[0], want)
    _same_result(got[1], want)
