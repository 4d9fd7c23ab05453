"""GPU: live.RealtimeCall - captured frame in, scores out - on the network, clip size and frame size tests/test_hip_live.py uses
(96 x 131 frames, a shrunken synthetic I3D in f16, 8 frames of 64 x 64).

  (a) detector    with the real YuNet at a low threshold on three seeded frames the detections RealtimeCall hands its tracker are
                  bit for bit YuNet.infer(frame)'s, and uploaded_bytes grows by exactly one frame per step
  (b) composition a stub detector returns scripted device rows: two moving faces, one of them in the self-view rectangle for a
                  while, one blurry (a flat patch) for five frames so that the gate rejects it.  At least two windows close across
                  a ring wrap (asserted first); tids, scores and purged are bit for bit those of the hand composition - ByteTracker,
                  the host loop written out, quality_ref on host crops, a second LiveCall.step(frame, faces, alive=...); state and
                  clip_hist follow af_realtime.py:349-358
  (c) channels    channel_order="rgb" with reversed frames gives the scores of "bgr"
"""
import collections
import os
import types

import numpy as np
import pytest
import torch

import af_mi355x
import quality_ref as Q
from af_mi355x import live, synth
from af_mi355x.classifier import I3D8x8
from af_mi355x.evaluator import get_crop_box
from af_mi355x.tracker import ByteTracker, STrack, iou_distance

pytestmark = pytest.mark.gpu
H, W = 96, 131
CLIP, SIZE = 8, 64
DROP, STRIDE, STEPS = 6, 3, 40
RING = CLIP + DROP
EXCLUDE = (0.70, 0.70, 1.00, 1.00)
GATE = dict(q_min_size_soft=24, q_min_size_hard=12, q_lap_soft=20.0, q_lap_hard=5.0)
MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yunet_2023mar.onnx")
_nets = {}


def _net():
    if "i3d" not in _nets:
        net = I3D8x8(clip_size=CLIP, crop_size=SIZE, precision="f16")
        net.load_state_dict(synth.synthetic_state_dict(net.spec, seed=5))
        _nets["i3d"] = net.cuda().eval()
    return _nets["i3d"]


def _call(detector, **kw):
    args = dict(clip_size=CLIP, size=SIZE, stride=STRIDE, ring_frames=RING, drop_after=DROP, start_conf=0.76, start_min_size=20,
                exclude_rect=EXCLUDE, **GATE)
    args.update(kw)
    return af_mi355x.RealtimeCall(_net(), detector=detector, **args)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------

def test_the_detector_reads_the_resident_frame():
    from af_mi355x.detector import YuNet
    size = 320
    alone = YuNet(MODEL, inputSize=[size, size], confThreshold=0.05)
    call = _call(YuNet(MODEL, inputSize=[size, size], confThreshold=0.05))
    total = 0
    for i in range(3):
        kind = "smooth" if i % 2 == 0 else "uniform"
        frame = np.ascontiguousarray(synth.synthetic_clips_u8(1, seed=51 + i, kind=kind, num_frames=1, size=size)[0, 0].numpy())
        want = alone.infer(frame)
        call.step(frame)
        got = call.detections
        assert got.dtype == np.float32 and got.shape == (len(want), 15) and (len(want) == 0 or np.array_equal(got, want)), i
        assert call.uploaded_bytes == (i + 1) * frame.nbytes
        total += len(want)
    assert total >= 1


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------

def _scripted(seed=4):
    """per step: the frame and the YuNet rows of two faces.  Face A drifts right and is blurry (its crop a flat patch) on steps
    10..14; face B walks into the self-view rectangle (steps 12..21) and back out"""
    rng = np.random.default_rng(seed)
    std = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
    out = []
    for s in range(STEPS):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        t = min(max(s - 8, 0), 8) if s < 22 else max(0, 8 - (s - 21))
        faces = [(14 + 0.5 * s, 22 + 0.1 * s, 30, 34, 0.95), (50 + 5.0 * t, 40 + 2.5 * t, 28, 32, 0.93)]
        rows = []
        for x, y, w, h, sc in faces:
            j = rng.uniform(-0.3, 0.3, 4)
            x, y, w, h = x + j[0], y + j[1], w + j[2], h + j[3]
            lm = std * [w, h] + [x, y] + rng.normal(0, 0.4, (5, 2))
            rows.append(np.concatenate([[x, y, w, h], [sc + rng.uniform(-0.004, 0.004)], lm.ravel()]))
        rows = np.asarray(rows, dtype=np.float32)
        if 10 <= s < 15:
            x1, y1, x2, y2 = map(int, get_crop_box((H, W), [rows[0, 0], rows[0, 1], rows[0, 0] + rows[0, 2], rows[0, 1] + rows[0, 3]], scale=0.6))
            frame[max(0, y1 - 6):y2 + 6, max(0, x1 - 6):x2 + 6] = 90
        out.append((frame, rows))
    return out


class _StubDetector:
    def __init__(self, script):
        self.script, self.calls, self.seen = script, 0, []

    def detect(self, frames_u8):
        assert frames_u8.is_cuda and frames_u8.shape == (1, H, W, 3)
        self.seen.append(frames_u8[0].cpu().numpy())              # the resident frame, as the detector finds it
        rows = torch.zeros(1, 16, 15, dtype=torch.float32, device=frames_u8.device)
        mine = self.script[self.calls][1]
        rows[0, :len(mine)] = torch.from_numpy(mine).to(frames_u8.device)
        self.calls += 1
        return rows, torch.tensor([len(mine)], dtype=torch.int32, device=frames_u8.device)


def _in_exclude(box):
    cx, cy = 0.5 * (box[0] + box[2]), 0.5 * (box[1] + box[3])
    return (EXCLUDE[0] * W <= cx <= EXCLUDE[2] * W) and (EXCLUDE[1] * H <= cy <= EXCLUDE[3] * H)


def _hand_composition(script, order="bgr"):
    """af_realtime.py:372-509 by hand: ByteTracker, the host loop written out, the gate on quality_ref of host crops, LiveCall"""
    tracker = ByteTracker(types.SimpleNamespace(track_thresh=0.8, track_buffer=90, match_thresh=0.8, mot20=False), frame_rate=30.0)
    call = af_mi355x.LiveCall(_net(), clip_size=CLIP, size=SIZE, stride=STRIDE, ring_frames=RING, drop_after=DROP, channel_order=order)
    last_lm, out = {}, []
    for s, (frame, dets) in enumerate(script):
        tracks_in = [STrack(d[:4], score=float(d[4])) for d in dets if d[4] >= 0.76 and max(d[2], d[3]) >= 20]       # :382-386
        online = tracker.update(tracks_in, (H, W), (H, W))                                                           # :388
        det_tlbr = np.asarray([[d[0], d[1], d[0] + d[2], d[1] + d[3]] for d in dets], dtype=np.float32)               # :394-396
        faces, alive, rejected, excluded = [], [], [], []
        for tr in online:                                                                                            # :401
            if _in_exclude(tr.tlbr):                                                                                 # :403
                excluded.append(tr.track_id)
                continue
            alive.append(tr.track_id)                                                                                # :407
            ious = 1.0 - iou_distance(np.array([tr.tlbr], dtype=np.float32), det_tlbr)[0]                            # :415-418
            k = int(np.argmax(ious))
            fm = dets[k][5:15].reshape(5, 2) if ious[k] >= 0.4 else None                                             # :425, mesh_every = 1
            if fm is None:
                continue
            last_lm[tr.track_id] = fm
            tlbr = tr.tlbr.astype(np.float32)
            x1, y1, x2, y2 = map(int, get_crop_box((H, W), tlbr, scale=0.6))                                         # :435-437
            if x2 <= x1 or y2 <= y1:
                continue
            min_side, lap = Q.min_side_and_lap(frame[y1:y2, x1:x2], order)                                           # :438-439
            if live.quality_weight(min_side, lap, **GATE) <= 0.0:                                                    # :441
                rejected.append(tr.track_id)
                continue
            faces.append((tr.track_id, tlbr, fm.astype(np.float32)))
        results = call.step(frame, faces, alive=[t for t in alive if t not in {f[0] for f in faces}])
        out.append((results, sorted(call.purged), rejected, excluded))
    return out


@pytest.fixture(scope="module")
def script():
    return _scripted()


@pytest.fixture(scope="module")
def hand(script):
    return _hand_composition(script)


def test_the_step_equals_the_hand_composition(script, hand):
    closes = [s for s, (results, _, _, _) in enumerate(hand) if results]
    assert len(closes) >= 2 and any(s < RING for s in closes) and any(s >= RING for s in closes), closes
    assert sum(bool(r[2]) for r in hand) == 5 and sum(bool(r[3]) for r in hand) >= 5          # the blurry steps, the self-view steps
    det = _StubDetector(script)
    call = _call(det)
    clip_hist, state = collections.defaultdict(lambda: collections.deque(maxlen=5)), {}
    running, purged_tids = collections.defaultdict(list), set()
    for s, (frame, _) in enumerate(script):
        got = call.step(frame)
        want, purged, _, _ = hand[s]
        assert got == want and sorted(call.purged) == purged, (s, got, want)
        assert np.array_equal(det.seen[-1], frame) and call.uploaded_bytes == (s + 1) * frame.nbytes
        for tid, sc in got:                                                                   # :349-358
            clip_hist[tid].append(sc)
            sm = float(np.median(clip_hist[tid]))
            st = state.get(tid, {"fake": False})
            if not st["fake"] and sm >= 0.75:
                st["fake"] = True
            elif st["fake"] and sm < 0.65:
                st["fake"] = False
            state[tid] = st
            running[tid].append(sc)
        for tid in purged:                                                                    # :489-499
            running.pop(tid, None)
            purged_tids.add(tid)
        assert call.state == state and {t: list(v) for t, v in call.clip_hist.items()} == {t: list(v) for t, v in clip_hist.items()}
    assert det.calls == STEPS and call.frame_idx == STEPS - 1
    assert 2 in purged_tids and dict(call.running_scores) == dict(running)          # a purged tid's scores go with it (:496)
    assert call.pick_interlocutor_id(H, W) in call.last_boxes
    assert any(v[1] < 5.0 for v in call.host.q_hist[1])           # the blurry crops were measured, recorded and rejected


def test_rgb_frames_give_the_scores_of_bgr_frames(script, hand):
    call = _call(_StubDetector(script), channel_order="rgb")
    for s, (frame, _) in enumerate(script):
        assert call.step(np.ascontiguousarray(frame[..., ::-1])) == hand[s][0], s
