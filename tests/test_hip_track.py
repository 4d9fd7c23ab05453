"""GPU: TrackScorer (evaluator.py) - every sliding window of a face track aligned by ONE window-batch warp launch per batch
(af_warp_affine_windows_u8) out of crops uploaded once, and scored by the existing forward.

  aligned windows   BIT-EXACT, every byte, against oracle/aligner_oracle.crop_align on the window's own frames
  scores            EXACTLY those of forward_clips_u8(return_scores=True) fed the oracle's aligned windows in TrackScorer.partition's
                    batches (identical input bytes; the engine is bitwise repeatable and independent of the batch position)
  logits            against the CPU fp32 oracle forward of the oracle-aligned clip under tests/test_hip_forward.py's gates:
                    f16 1e-3, bf16 3e-3 absolute (the O(0.3) logits of the seeded checkpoint; 7e-3 relative is its gate for hot ones)
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import aligner_oracle as ao  # noqa: E402
import i3d_oracle as oracle  # noqa: E402
from af_mi355x import aligner, evaluator  # noqa: E402
from af_mi355x.classifier import Classifier  # noqa: E402

pytestmark = pytest.mark.gpu
LOGIT_TOL = {"f16": 1e-3, "bf16": 3e-3}                    # tests/test_hip_forward.py
SIZE = 224


def _smaller_crops(frames, seed):
    """crops a few pixels smaller than their boxes (as tests/test_hip_aligner.py::_clip makes them), handed over as views"""
    infos, crops = aligner.synthetic_clip(frames=frames, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return infos, [c[:c.shape[0] - int(rng.integers(0, 9)), :c.shape[1] - int(rng.integers(0, 9))] for c in crops]


TRACKS = {
    "t44": lambda: aligner.synthetic_clip(frames=44, seed=21),                      # 13 windows
    "t40_mirrored": lambda: aligner.synthetic_clip(frames=40, seed=22, mirrored=True),
    "t32": lambda: aligner.synthetic_clip(frames=32, seed=23),                      # one window
    "t20": lambda: aligner.synthetic_clip(frames=20, seed=24),                      # one padded window with repeated frames
    "t36_smaller_crops": lambda: _smaller_crops(36, 25),
}
_cache = {}


def _track(name):
    """(infos, crops, windows, the oracle's aligned windows (W, 32, 224, 224, 3) uint8) - the oracle runs once per track"""
    if name not in _cache:
        infos, crops = TRACKS[name]()
        windows = evaluator.clip_windows(len(crops), 32)
        want = np.stack([ao.crop_align([(a, b.copy(), c.copy(), d.copy()) for a, b, c, d in (infos[j] for j in w)],
                                       [crops[j] for j in w], size=SIZE)[1] for w in windows])
        _cache[name] = (infos, crops, windows, want)
    return _cache[name]


_nets = {}


def _net(dtype, weights0, copy=0):
    if (dtype, copy) not in _nets:
        clf = Classifier(precision=dtype)
        clf.network.load_state_dict(weights0)
        _nets[(dtype, copy)] = clf.cuda().eval()
    return _nets[(dtype, copy)]


@pytest.mark.parametrize("name", list(TRACKS))
def test_aligned_windows_bit_exact_vs_oracle(name, weights0):
    infos, crops, windows, want = _track(name)
    scorer = evaluator.TrackScorer(_net("f16", weights0))
    got = scorer.aligned_windows(infos, crops, windows)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape == (len(windows), 32, SIZE, SIZE, 3)
    got = got.cpu().numpy()
    assert got.any(), "all-zero output"
    for w in range(len(windows)):
        assert (got[w] == want[w]).all(), "window %d differs in %d bytes" % (w, int((got[w] != want[w]).sum()))
    assert scorer.uploaded_bytes == int(((np.array([c.shape[0] * c.shape[1] * 3 for c in crops]) + 15) // 16 * 16).sum())   # each crop once
    if name == "t20":
        assert len(set(windows[0])) == 20 and len(windows[0]) == 32


def test_window_batch_equals_the_single_clip_kernel(weights0):
    """the same bytes as the existing per-clip path (FasterCropAlignXRay -> af_warp_affine_clip_u8) on the windows of a track"""
    infos, crops, windows, _ = _track("t44")
    got = evaluator.TrackScorer(_net("f16", weights0), batch=8).aligned_windows(infos, crops, windows).cpu().numpy()
    al = aligner.FasterCropAlignXRay(SIZE)
    for w, idx in enumerate(windows):
        _, want = al([infos[j] for j in idx], [crops[j] for j in idx])
        assert (got[w] == want).all(), w


def _reference_scores(net, scorer, want_u8):
    """forward_clips_u8 on the oracle's windows in the scorer's own partition (the short batch padded with its last window)"""
    out = []
    for lo, n, run in scorer.partition(len(want_u8)):
        batch = np.concatenate([want_u8[lo:lo + n]] + [want_u8[lo + n - 1:lo + n]] * (run - n))
        with torch.inference_mode():
            s = net.network.forward_clips_u8(torch.from_numpy(batch).cuda(), return_scores=True)["scores"]
        out.append(s[:n].float().cpu().numpy())
    return np.concatenate(out)


def test_partition_shapes(weights0):
    scorer = evaluator.TrackScorer(_net("f16", weights0))
    assert scorer.partition(0) == [] and scorer.partition(1) == [(0, 1, 1)] and scorer.partition(13) == [(0, 13, 16)]
    assert scorer.partition(369) == [(16 * k, 16, 16) for k in range(23)] + [(368, 1, 1)]
    assert scorer.partition(37) == [(0, 16, 16), (16, 16, 16), (32, 5, 8)]
    assert evaluator.TrackScorer(_net("f16", weights0), batch=12).partition(21) == [(0, 12, 12), (12, 9, 12)]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_scores_equal_the_existing_forward_on_oracle_windows(dtype, weights0):
    net = _net(dtype, weights0)
    # t44 at batch 4: forwards of 4, 4, 4 and 1 in a row through the two alternating clip buffers
    for name, batch in (("t44", 16), ("t44", 4), ("t20", 16), ("t36_smaller_crops", 4)):
        infos, crops, windows, want_u8 = _track(name)
        scorer = evaluator.TrackScorer(net, batch=batch)
        got = scorer.score_track(infos, crops)
        want = _reference_scores(net, scorer, want_u8)
        print(dtype, name, "scores", got[:3], "...")
        assert got.dtype == np.float32 and got.shape == (len(windows),)
        assert np.array_equal(got, want), (name, np.abs(got - want).max())
        assert ((got > 0) & (got < 1)).all()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_logits_close_to_the_fp32_reference(dtype, weights0):
    infos, crops, windows, want_u8 = _track("t44")
    pick = [0, 12]
    net = _net(dtype, weights0)
    scorer = evaluator.TrackScorer(net)
    clips = scorer.aligned_windows(infos, crops, [windows[w] for w in pick])
    with torch.inference_mode():
        out = net.network.forward_clips_u8(clips, return_scores=True)
    got = out["final_output"].float().cpu().flatten()
    want = oracle.forward(weights0, oracle.normalize(torch.from_numpy(want_u8[pick]))).flatten()
    err = (got - want).abs().max().item()
    print("%s windows %s: hip %s oracle %s max|d| %.3e (gate %.1e)" % (dtype, pick, got.tolist(), want.tolist(), err, LOGIT_TOL[dtype]))
    assert err <= LOGIT_TOL[dtype], (dtype, err)
    probs = scorer.score_track(infos, crops)[pick]
    assert np.abs(probs - oracle.scores(want.view(-1, 1)).numpy().flatten()).max() <= LOGIT_TOL[dtype]      # |sigmoid'| <= 1/4


def test_segments_do_not_change_the_scores(weights0):
    infos, crops = aligner.synthetic_clip(frames=70, seed=31)
    net = _net("f16", weights0)
    whole = evaluator.TrackScorer(net)
    want = whole.score_track(infos, crops)
    sizes = (np.array([c.shape[0] * c.shape[1] * 3 for c in crops]) + 15) // 16 * 16
    small = evaluator.TrackScorer(net, pool_bytes=int(sizes[:40].sum()) + 64)
    segs = small._segments(evaluator._Track(infos, crops), evaluator.clip_windows(70, 32))
    assert len(segs) >= 3 and all(b[0] == a[1] - 31 for a, b in zip(segs, segs[1:]))       # neighbours overlap by clip_size - 1 frames
    assert sum(len(s[2]) for s in segs) == 39
    got = small.score_track(infos, crops)
    assert got.shape == (39,) and np.array_equal(got, want)
    assert small.uploaded_bytes > whole.uploaded_bytes == int(sizes.sum())
    with pytest.raises(ValueError, match="does not fit the pool"):
        evaluator.TrackScorer(net, pool_bytes=int(sizes[:20].sum())).score_track(infos, crops)


def test_two_scorers_on_two_streams(weights0):
    a, b = aligner.synthetic_clip(frames=40, seed=41), aligner.synthetic_clip(frames=36, seed=42)
    sa, sb = evaluator.TrackScorer(_net("f16", weights0, 0)), evaluator.TrackScorer(_net("f16", weights0, 1))
    want_a, want_b = sa.score_track(*a), sb.score_track(*b)
    torch.cuda.synchronize()
    track_a, track_b = evaluator._Track(*a), evaluator._Track(*b)
    st_a, st_b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(st_a):                                # both tracks enqueued before either is read back
        parts_a = sa._score_device(track_a, evaluator.clip_windows(40, 32))
    with torch.cuda.stream(st_b):
        parts_b = sb._score_device(track_b, evaluator.clip_windows(36, 32))
    with torch.cuda.stream(st_a):
        got_a = torch.cat(parts_a).float().cpu().numpy()
    with torch.cuda.stream(st_b):
        got_b = torch.cat(parts_b).float().cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
    assert not np.array_equal(got_a[:5], got_b[:5])


def test_errors_and_empty_track(weights0):
    scorer = evaluator.TrackScorer(_net("f16", weights0))
    infos, crops = aligner.synthetic_clip(frames=33, seed=51)
    with pytest.raises(AssertionError):
        scorer.score_track(infos, [crops[0].astype(np.float32)] + crops[1:])
    grown = list(crops)
    grown[5] = np.zeros((crops[5].shape[0] + 400, crops[5].shape[1], 3), dtype=np.uint8)     # taller than any window's canvas
    with pytest.raises(ValueError, match=r"window 0 frame 5 .* does not fit"):
        scorer.score_track(infos, grown)
    with pytest.raises(ValueError, match=r"window 0 frame 4 .* does not fit"):
        scorer.aligned_windows(infos, grown, evaluator.clip_windows(33, 32)[1:])
    empty = scorer.score_track([], [])
    assert empty.dtype == np.float32 and empty.shape == (0,)
    assert scorer.aligned_windows(infos, crops, []).shape == (0, 32, SIZE, SIZE, 3)
    res = scorer.score_video((720, 1280, 3), [], [], [])
    assert res["video_score"] == 0.0 and res["pred_label"] == 0 and res["preds"] == [] and res["frame_res"] == {} and res["clips"] == []
    got = scorer.score_track(infos, crops)                       # the scorer still works after the refused calls
    assert got.shape == (2,) and np.isfinite(got).all()


def _video(seed, n_frames=48, shape=(720, 1280, 3)):
    """frames + two tracks in frame coordinates: 40 frames from frame 2 (9 windows), 20 frames from frame 25 (one padded window)"""
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(n_frames)]
    std = aligner.STD_POINTS_317 - 30.0
    tracks, spans = [], [(2, 42), (25, 45)]
    for ti, (start, end) in enumerate(spans):
        cx, cy, faces = 400.0 + 500.0 * ti, 330.0, []
        for _ in range(start, end):
            cx, cy = cx + rng.normal(0, 2.0), cy + rng.normal(0, 2.0)
            half = 90.0 + rng.normal(0, 1.0)
            box = np.array([cx - half, cy - half, cx + half, cy + half])
            lm5 = (std - std.mean(0)) * (half / 90.0) + np.array([cx, cy]) + rng.normal(0, 0.8, (5, 2))
            lm68 = np.array([cx, cy]) + rng.normal(0, 40.0, (68, 2))
            faces.append((box, lm5, lm68, 0.99))
        tracks.append(faces)
    return shape, frames, tracks, spans


def test_score_video_equals_the_per_window_results_combined_on_the_host(weights0):
    shape, frames, tracks, spans = _video(61)
    scorer = evaluator.TrackScorer(_net("f16", weights0))
    res = scorer.score_video(shape, frames, tracks, spans, threshold=0.04)
    preds, frame_res, clips = [], {}, []
    for ti, ((start, end), faces) in enumerate(zip(spans, tracks)):                 # demo.py:245-340 with score_track per track
        recs = evaluator.crop_records(shape, faces)
        crops = [frames[f][b[1]:b[3], b[0]:b[2]] for f, (b, _) in zip(range(start, end), recs)]
        scores = scorer.score_track([info for _, info in recs], crops)
        windows = evaluator.clip_windows(end - start, 32)
        assert len(scores) == len(windows)
        for w, s in zip(windows, scores):
            pred = float(s)
            for j in w:
                frame_res.setdefault(start + j, []).append(pred)
            preds.append(pred)
            clips.append([(ti, j) for j in w])
    video_score = float(np.mean(preds))
    assert len(preds) == 10 and res["preds"] == preds and res["clips"] == clips
    assert res["video_score"] == video_score and res["pred_label"] == int(video_score > 0.04)
    assert set(res["frame_res"]) == set(frame_res)
    for k, v in frame_res.items():
        assert res["frame_res"][k] == float(np.mean(v)), k
    assert len(frame_res[30]) == 10                              # frame 30: all nine windows of track 0 + the padded window of track 1
    assert len(frame_res[43]) == 3                               # frame 43 = index 18 of track 1: once itself, once in either padding
