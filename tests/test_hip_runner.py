"""GPU: runner.VideoRunner - a video's frames in, the dataset evaluator's dict out - on the shapes of tests/test_hip_realtime.py
(96 x 131 frames, the shrunken synthetic I3D in f16, 8 frames of 64 x 64).

  (a) composition  a stub detector that recognises a frame by its bytes (a chunk arrives as one (B, H, W, 3) view) returns
                   scripted rows: two faces, one of them blurry (a flat patch) for five frames.  ``run`` equals the hand
                   composition written out below - ByteTracker, the loop of altfreezing/TEST2.py:486-621, quality_ref /
                   runner_ref on host crops, StreamingCropAligner + forward_clips_u8 at the padded batch size: the warped clips
                   and the scores bit for bit, the dict key for key
  (b) chunks       detect_batch 1, 5 and 16 give identical dicts; at most three waits per chunk without a flush (two are taken:
                   the rows, both quality figures in one read-back), one more per flush
  (c) channels     RGB frames and I420 ``YuvFrame``s give the result of the B, G, R frames
  (d) detector     with the real YuNet on seeded frames the chunked ``detect`` hands the loop ``YuNet.infer``'s rows
"""
import os
import types

import numpy as np
import pytest
import torch

import af_mi355x
import quality_ref as Q
import runner_ref
import yuv_ref
from af_mi355x import aligner, live, synth
from af_mi355x import runner as R
from af_mi355x.classifier import I3D8x8
from af_mi355x.evaluator import get_crop_box
from af_mi355x.tracker import ByteTracker, STrack, iou_distance

pytestmark = pytest.mark.gpu
H, W = 96, 131
CLIP, SIZE, FRAMES = 8, 64, 48
MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yunet_2023mar.onnx")
GATE = dict(q_weighting=True, q_min_size_soft=24, q_min_size_hard=12, q_lap_soft=20.0, q_lap_hard=5.0)
# the faces sit near the origin: the loop hands STrack a tlbr box where it takes tlwh (TEST2.py:535), so a track's box is
# (x, y, 2x + w, 2y + h) and YuNet's five points are used only where that box and the detection overlap with IoU >= 0.4
ARGS = dict(clip_size=CLIP, crop_scale=0.2, stride=0, detect_every=3, mesh_every=3, batch_clips=3, min_det_side=20, min_det_area=900,
            exclude_bottom_frac=0.10, min_track_side=30, **GATE)
TIMINGS = ("video_path", "elapsed_s", "fps", "latency_ms_clip_mean", "gpu_mem_alloc_peak_mb", "gpu_mem_reserved_peak_mb", "cpu_mem_peak_mb",
           "stats")
_nets = {}


def _net():
    if "i3d" not in _nets:
        net = I3D8x8(clip_size=CLIP, crop_size=SIZE, precision="f16")
        net.load_state_dict(synth.synthetic_state_dict(net.spec, seed=5))
        _nets["i3d"] = net.cuda().eval()
    return _nets["i3d"]


def _rows(n=FRAMES, seed=4):
    """per frame the YuNet rows of two faces, and of a third detection that one of the filters drops"""
    rng = np.random.default_rng(seed)
    std = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
    out = []
    for f in range(n):
        faces = [(5 + 0.10 * f, 4 + 0.05 * f, 40, 44, 0.95), (24 - 0.05 * f, 16 + 0.04 * f, 44, 46, 0.93)]
        faces.append([(70, 5, 15, 18, 0.9), (70, 30, 22, 30, 0.9), (60, 70, 30, 32, 0.9)][f % 3])      # short; small; in the bottom tenth
        rows = []
        for x, y, w, h, sc in faces:
            j = rng.uniform(-0.3, 0.3, 4)
            x, y, w, h = x + j[0], y + j[1], w + j[2], h + j[3]
            lm = std * [w, h] + [x, y] + rng.normal(0, 0.4, (5, 2))
            rows.append(np.concatenate([[x, y, w, h], [sc + rng.uniform(-0.004, 0.004)], lm.ravel()]))
        out.append(np.asarray(rows, dtype=np.float32))
    return out


BLURRY = range(14, 19)                     # the frames on which the first face's crop is a flat patch


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


class _StubDetector:
    """scripted rows for the frames it recognises by their bytes, wherever in a chunk they arrive"""

    def __init__(self, script, frames=None):
        self.rows = {(f if frames is None else frames[i]).tobytes(): r for i, (f, r) in enumerate(script)}
        self.batches = []

    def detect(self, frames_u8):
        assert frames_u8.is_cuda and frames_u8.dim() == 4 and frames_u8.shape[3] == 3
        b = frames_u8.shape[0]
        self.batches.append(b)
        rows = torch.zeros(b, 16, 15, dtype=torch.float32, device=frames_u8.device)
        counts = torch.zeros(b, dtype=torch.int32, device=frames_u8.device)
        host = frames_u8.cpu().numpy()
        for k in range(b):
            mine = self.rows[host[k].tobytes()]
            rows[k, :len(mine)] = torch.from_numpy(mine).to(frames_u8.device)
            counts[k] = len(mine)
        return rows, counts


class _Watching(R._DeviceSide):
    """the runner's device side, keeping what it warped for every flush group and the rows every detect handed over"""
    warped, handed = [], []

    def score(self, group):
        out = super().score(group)
        run = 1
        while run < len(group):
            run *= 2
        type(self).warped.append(self.scoring.scorer(run).clip[:run].clone().cpu())
        return out

    def detect(self, first_slot, n):
        rows = super().detect(first_slot, n)
        type(self).handed += rows
        return rows


def _runner(detector, watch=False, **kw):
    r = af_mi355x.VideoRunner(_net(), detector=detector, size=SIZE, **dict(ARGS, **kw))
    if watch:
        _Watching.warped, _Watching.handed = [], []
        r.side_type = _Watching
    return r


def _plain(out):
    return {k: v for k, v in out.items() if k not in TIMINGS}


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------

def _hand_composition(script, order="bgr"):
    """altfreezing/TEST2.py:303-797 by hand for ARGS (no smart start, a frame count, no thinning): the window ranges, ByteTracker,
    the loop written out, the gate on quality_ref / runner_ref of host crops, one StreamingCropAligner per track, the eager forward
    at the batch size a flush group pads to"""
    net = _net()
    a = types.SimpleNamespace(**dict(R.DEFAULTS, **ARGS))
    tracker = ByteTracker(types.SimpleNamespace(track_thresh=a.track_thresh, track_buffer=a.track_buffer, match_thresh=a.match_thresh, mot20=False),
                          frame_rate=30.0)
    total, stride = len(script), CLIP // 2                                                                        # :446, stride 0
    starts = list(range(0, max(0, total - CLIP) + 1, stride))                                                     # :448-449
    assert len(starts) <= a.max_frame // CLIP                                                                     # :452-455: no thinning
    ranges = [(s, min(s + CLIP - 1, total - 1)) for s in starts]                                                  # :457
    aligners, held, last_lm, last_win = {}, {}, {}, {}
    batch, groups, clips, scores_of, qstat = [], [], [], {}, []
    prev_boxes = prev_ids = None
    id_switches = frames_seen = 0

    def flush():                                                                                                  # :393-439
        if not batch:
            return
        stack = torch.stack([c for _, c in batch])
        run = 1
        while run < len(batch):
            run *= 2
        padded = torch.cat([stack] + [stack[-1:]] * (run - len(batch)))
        with torch.inference_mode():
            scores = net.forward_clips_u8(padded, return_scores=True)["scores"][:len(batch)].float().cpu()
        for (tid, _), s in zip(batch, scores.tolist()):
            scores_of.setdefault(tid, []).append(float(s))
        groups.append([tid for tid, _ in batch])
        clips.append(padded.cpu())
        batch.clear()

    for f, (frame, rows) in enumerate(script):
        assert any(lo <= f <= hi for lo, hi in ranges)                                                            # :492: every frame is kept
        need_detect = (f % a.detect_every == 0) or (tracker.tracked_stracks == [])                                # :496-500
        det_tlbr, dets_np, tracks_in = None, None, []
        if need_detect and len(rows) > 0:                                                                         # :516-537
            d = np.asarray(rows, dtype=np.float32)
            mask = (np.maximum(d[:, 2], d[:, 3]) >= a.min_det_side) & (d[:, 2] * d[:, 3] >= a.min_det_area) \
                & (d[:, 1] + 0.5 * d[:, 3] < H * (1.0 - a.exclude_bottom_frac))
            dets_np = d[mask]
            boxes = [np.array([r[0], r[1], r[0] + r[2], r[1] + r[3]], dtype=np.float32) for r in dets_np]
            tracks_in = [STrack(b, score=float(r[4])) for b, r in zip(boxes, dets_np)]                            # :535, tlbr as it is
            det_tlbr = np.asarray(boxes, dtype=np.float32) if boxes else None
        online = tracker.update(tracks_in, (H, W), (H, W))                                                        # :538
        large = [t for t in online if max(t.tlbr[2] - t.tlbr[0], t.tlbr[3] - t.tlbr[1]) >= a.min_track_side]      # :546-548
        if large:                                                                                                 # :551-558
            cur = np.stack([t.tlbr.astype(np.float32) for t in large], 0)
            if prev_boxes is not None:
                dist = iou_distance(prev_boxes, cur)
                for i in range(len(prev_boxes)):
                    j = int(np.argmin(dist[i]))
                    id_switches += int(1.0 - float(dist[i, j]) >= 0.5 and prev_ids[i] != large[j].track_id)
            prev_boxes, prev_ids = cur, [t.track_id for t in large]
        frames_seen += 1
        frgb = frame[..., ::-1] if order == "bgr" else frame                                                      # :578
        for tr in large:
            tid = tr.track_id
            lm = None
            if det_tlbr is not None:                                                                              # :569-574
                ious = 1.0 - iou_distance(np.array([tr.tlbr], dtype=np.float32), det_tlbr)[0]
                k = int(np.argmax(ious))
                if ious[k] >= 0.4:
                    lm = dets_np[k][5:15].reshape(5, 2)
            if f % a.mesh_every == 0 or tid not in last_lm:                                                       # :577-586, no FaceMesh
                if lm is not None:
                    last_lm[tid] = lm
            else:
                lm = last_lm[tid]
            if lm is None:
                continue
            x1, y1, x2, y2 = map(int, get_crop_box((H, W), tr.tlbr, scale=a.crop_scale))                          # :593-595
            if x2 <= x1 or y2 <= y1:
                continue
            crop = frgb[y1:y2, x1:x2]                                                                             # :597
            min_side, lap = Q.min_side_and_lap(crop, "rgb")                                                       # :289-291
            wq = live.quality_weight(min_side, lap, **GATE)                                                       # :292-295
            if not (min_side < a.q_min_size_hard or lap < a.q_lap_hard) and len(qstat) < 50:                      # :296-299
                qstat.append(runner_ref.min_side_and_full_lap(crop, "rgb"))
            if wq > 0.0:                                                                                          # :599-609
                top_left = np.array([[x1, y1]], dtype=np.float32)
                record = ((tr.tlbr.reshape(2, 2).astype(np.float32) - top_left).reshape(-1), lm.astype(np.float32) - top_left,
                          np.zeros((68, 2), np.float32), np.array([x1, y1, x2, y2], dtype=np.int32))
                if tid not in aligners:
                    aligners[tid] = aligner.StreamingCropAligner(size=SIZE, capacity=32, max_crop_pixels=H * W)
                aligners[tid].push(record, np.ascontiguousarray(crop))
                held[tid] = held.get(tid, 0) + 1
            wid = next((k for k, (lo, hi) in enumerate(ranges) if lo <= f <= hi), -1)                             # :459-463
            if held.get(tid, 0) >= CLIP and wid != -1 and last_win.get(tid) != wid:                               # :611-618
                assert held[tid] == CLIP
                batch.append((tid, aligners[tid].align_last(CLIP)[1].clone()))
                last_win[tid], held[tid] = wid, 0
                if len(batch) >= a.batch_clips:
                    flush()
    flush()                                                                                                       # :621
    verdict = R.video_verdict(scores_of, qstat, a)
    want = {"frames_processed": len(script), "video_score": verdict["video_score"], "pred_label": verdict["pred_label"],
            "num_tracks": verdict["num_tracks"], "id_switch_rate_per_1k_frames": id_switches / max(1, frames_seen) * 1000.0,
            "per_person_scores": verdict["per_person_scores"], "per_person_labels": verdict["per_person_labels"], "track_clip_scores": scores_of}
    return want, groups, clips, qstat


@pytest.fixture(scope="module")
def hand(script):
    return _hand_composition(script)


@pytest.fixture(scope="module")
def chunks_of_five(script):
    det = _StubDetector(script)
    r = _runner(det, watch=True, detect_batch=5)
    out = r.run([f for f, _ in script], fps=30.0)
    return out, r, det, list(_Watching.warped)


def test_the_run_equals_the_hand_composition(script, hand, chunks_of_five):
    want, groups, clips, qstat = hand
    out, r, det, warped = chunks_of_five
    assert len(want["track_clip_scores"]) == 2 and [len(g) for g in groups] == [3, 3, 1], groups          # 3 pad to 4 clips; a last short one
    assert sum(len(v) for v in want["track_clip_scores"].values()) >= 4 and len(qstat) == 50
    assert r.trace["flush_groups"] == groups and [list(q) for q in r.trace["qstat"]] == [list(q) for q in qstat]
    assert len(warped) == len(clips) and all(torch.equal(g, w) for g, w in zip(warped, clips))            # the clips, bit for bit
    assert out["track_clip_scores"] == want["track_clip_scores"]                                          # the scores, bit for bit
    assert _plain(out) == want                                                                            # the dict, key for key
    assert all(0.0 < s < 1.0 for v in out["track_clip_scores"].values() for s in v)
    assert set(TIMINGS) <= set(out) and out["latency_ms_clip_mean"] > 0 and out["gpu_mem_alloc_peak_mb"] > 0 and out["cpu_mem_peak_mb"] > 0
    assert det.batches == [5] * 9 + [3] and out["stats"]["detect"] == 10 and out["stats"]["replay"] == len(groups)
    closing = {tid: [c["frame_idx"] for c in r.trace["clips"] if c["tid"] == tid] for tid in (1, 2)}
    assert closing[1][0] == closing[2][0] and closing[1][1] > closing[2][1]          # the blurry frames gave track 1 no entry: it closes later
    assert out["frames_processed"] == FRAMES and r.trace["slots_used"] == FRAMES


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("detect_batch", [1, 16])
def test_the_chunk_size_changes_nothing(script, chunks_of_five, detect_batch):
    det = _StubDetector(script)
    r = _runner(det, detect_batch=detect_batch)
    out = r.run([f for f, _ in script], fps=30.0)
    assert _plain(out) == _plain(chunks_of_five[0])
    assert det.batches == ([1] * FRAMES if detect_batch == 1 else [16, 16, 16])
    for chunk in r.chunks:                                    # the rows; the quality sums; the scores of a flush
        assert chunk["wait"] <= 2 + chunk["closes"] and chunk["detect"] == (1 if chunk["frames"] else 0), chunk
        assert chunk["replay"] == chunk["warp"] == chunk["closes"]


def test_waits_per_chunk(chunks_of_five):
    out, r, _, _ = chunks_of_five
    assert any(c["closes"] == 0 for c in r.chunks) and any(c["closes"] == 1 for c in r.chunks)
    for c in r.chunks:
        assert c["wait"] <= 3 + c["closes"], c                # the bound a chunk is held to: at most three waits without a flush
        assert c["wait"] == (2 + c["closes"] if c["frames"] else c["closes"]), c      # what it takes: the rows, the quality sums, a flush
        if c["frames"]:
            assert c["quality"] <= 2                          # one half-size launch, one full-size launch while _qstat is short
    first, late = r.chunks[0], [c for c in r.chunks if c["frames"]][-1]
    assert first["quality"] == 2 and late["quality"] == 1     # _qstat is full by then: no full-size launch
    assert out["stats"]["wait"] == sum(c["wait"] for c in r.chunks)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------

def test_rgb_frames_give_the_result_of_bgr_frames(script, chunks_of_five):
    reversed_frames = [np.ascontiguousarray(f[..., ::-1]) for f, _ in script]
    r = _runner(_StubDetector(script, reversed_frames), channel_order="rgb", detect_batch=16)
    assert _plain(r.run(reversed_frames, fps=30.0)) == _plain(chunks_of_five[0])


def test_i420_frames_give_the_result_of_their_bgr_frames():
    h, w = 96, 132                                            # 4:2:0 frames have even sides
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
    want = _runner(_StubDetector(script), detect_batch=16).run(bgr, fps=30.0)
    assert sum(len(v) for v in want["track_clip_scores"].values()) >= 4
    yuv = [af_mi355x.YuvFrame("i420", y, u, v) for y, u, v in planes]
    got = _runner(_StubDetector(script), detect_batch=16).run(yuv, fps=30.0)
    assert _plain(got) == _plain(want)
    as_rgb = _runner(_StubDetector(script, [np.ascontiguousarray(f[..., ::-1]) for f in bgr]), channel_order="rgb", detect_batch=16).run(yuv, fps=30.0)
    assert _plain(as_rgb) == _plain(want)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------

def test_the_chunked_detect_hands_over_yunet_infer_rows():
    from af_mi355x.detector import YuNet
    size, n = 320, 5
    alone = YuNet(MODEL, inputSize=[size, size], confThreshold=0.05)
    frames = [np.ascontiguousarray(synth.synthetic_clips_u8(1, seed=51 + i, kind="smooth" if i % 2 == 0 else "uniform", num_frames=1, size=size)[0, 0].numpy())
              for i in range(n)]
    want = [alone.infer(f) for f in frames]
    assert sum(len(w) for w in want) >= 1
    r = _runner(YuNet(MODEL, inputSize=[size, size], confThreshold=0.05), watch=True, detect_batch=2)
    out = r.run(frames, fps=30.0)
    got = list(_Watching.handed)
    assert len(got) == n and out["frames_processed"] == n and out["stats"]["detect"] == 3          # chunks of 2, 2 and 1
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == (len(w), 15) and (len(w) == 0 or np.array_equal(g, w))
