"""CPU: the per-track bookkeeping of live.LiveCall against the reference's own loop.

`reference_loop` below is test/af_realtime.py:401-505 (RealtimeAF.step behind the tracker) written out as a plain loop, the line
numbers cited, minus the FaceMesh lines (:413-432: the caller hands the five landmarks in) and the quality lines (:439-442, and
:403, the self-view exclusion: a face the caller rejects is not handed in).  LiveCall runs here with a fake frame store and a fake
warp + scorer that record what they are given; compared per step: the closed windows as (tid, frame ids, crop boxes) with the
records the aligner would get, and the tids purged.  No GPU, no libafhip call.
"""
import collections

import numpy as np
import pytest

from af_mi355x import live
from af_mi355x.evaluator import get_crop_box

H, W = 96, 131
CLIP, DROP = 8, 6
STEPS = 150


def reference_loop(script, clip_size, stride, crop_scale, drop_after):
    """-> per step (closed windows [(tid, frame ids, records)], purged tids)"""
    cur_imgs, cur_infos, since_emit = {}, {}, collections.Counter()          # :251-256 (cur_imgs holds the frame index of a crop)
    missed, last_boxes = collections.Counter(), {}                            # :213, :257
    out = []
    frame_idx = -1
    for faces in script:
        frame_idx += 1                                                         # :373
        ready, kept_boxes, batch = [], {}, []                                  # :398-399
        for tid, tlbr, lm5_in in faces:                                        # :401
            tlbr = np.asarray(tlbr, dtype=np.float32)
            kept_boxes[tid] = tlbr.astype(np.float32).copy()                   # :407
            if tid not in cur_imgs:                                            # :409-411
                cur_imgs[tid], cur_infos[tid] = [], []
                since_emit[tid] = 0
            big = get_crop_box((H, W), tlbr, scale=crop_scale)                 # :435
            x1, y1, x2, y2 = map(int, big)                                     # :436
            if x2 <= x1 or y2 <= y1:                                           # :437
                continue
            top_left = np.array([[x1, y1]], dtype=np.float32)                 # :445
            new_box = (tlbr.reshape(2, 2).astype(np.float32) - top_left).reshape(-1)      # :446
            lm5 = np.asarray(lm5_in).astype(np.float32) - top_left             # :447
            lm68 = np.zeros((68, 2), np.float32)                               # :448
            cur_infos[tid].append((new_box, lm5, lm68, np.array([x1, y1, x2, y2], dtype=np.int32)))     # :450
            cur_imgs[tid].append(frame_idx)                                    # :451
            since_emit[tid] += 1                                               # :453
            if len(cur_imgs[tid]) > clip_size:                                 # :457-460
                cur_imgs[tid] = cur_imgs[tid][-clip_size:]
                cur_infos[tid] = cur_infos[tid][-clip_size:]
            if len(cur_imgs[tid]) == clip_size and since_emit[tid] >= stride:  # :462
                since_emit[tid] = 0                                            # :463
                batch.append((tid, list(cur_imgs[tid]), list(cur_infos[tid])))  # :464, _enqueue_clip :293-309
                ready.append(tid)                                              # :465
        if ready:                                                              # :470
            keep_tail = max(0, clip_size - stride)                             # :475
            for tid in ready:                                                  # :476-478
                cur_imgs[tid] = cur_imgs[tid][-keep_tail:]
                cur_infos[tid] = cur_infos[tid][-keep_tail:]
        alive = set(kept_boxes.keys())                                         # :480
        purged = []
        known_tids = set(cur_imgs) | set(missed) | set(last_boxes)             # :483
        for tid in known_tids:                                                 # :484
            if tid in alive:                                                   # :485-486
                missed[tid] = 0
            else:
                missed[tid] += 1                                               # :488
                if missed[tid] >= drop_after:                                  # :489
                    cur_imgs.pop(tid, None)                                    # :491-499
                    cur_infos.pop(tid, None)
                    since_emit.pop(tid, None)
                    last_boxes.pop(tid, None)
                    missed.pop(tid, None)
                    purged.append(tid)
        persisting = {tid: box for tid, box in last_boxes.items() if missed.get(tid, 0) < drop_after}   # :502-503
        persisting.update(kept_boxes)                                          # :504
        last_boxes = persisting                                                # :505
        out.append((batch, sorted(purged)))
    return out


class RecordingCall(live.LiveCall):
    """LiveCall with the device taken out: the frame store records (frame, slot), the warp + scorer records its windows and
    answers with a number made from them"""

    def __init__(self, *a, **k):
        super().__init__(None, *a, **k)
        self.stored, self.scored = [], []

    def _new_ring(self, shape):
        return None

    def _store_frame(self, frame, slot):
        self.stored.append((int(frame[0, 0, 0]) | int(frame[0, 0, 1]) << 8, slot, frame.shape))

    def _score(self, ready):
        self.scored.append(ready)
        return np.array([float(win[-1][0]) + 0.001 * len(ready) for _, win in ready], dtype=np.float32)


def _face(rng, tid, step, degenerate=False):
    cx, cy = 30.0 + 9.0 * (tid % 7) + 0.1 * step, 40.0 + 0.05 * step
    half = 12.0 + rng.uniform(0, 2)
    tlbr = np.array([cx - half, cy - half, cx + half, cy + half], dtype=np.float32)
    if degenerate:                                            # left of the frame: get_crop_box cuts both x to 0
        tlbr = np.array([-60.0, 20.0, -40.0, 50.0], dtype=np.float32)
    lm5 = np.array([cx, cy], dtype=np.float32) + rng.normal(0, 3, (5, 2)).astype(np.float32)
    return tid, tlbr, lm5


def scripted_call(seed=0):
    """150 steps: track 1 steady; tracks 2 and 3 start together (they close on the same steps); track 4 vanishes for DROP - 1 steps
    and returns (kept); track 5 vanishes for DROP steps (purged) and a face with tid 5 comes back (starts empty); track 6's box
    is degenerate for a few steps in the middle of its life"""
    rng = np.random.default_rng(seed)
    script = []
    for s in range(STEPS):
        faces = [_face(rng, 1, s)]
        if s >= 5:
            faces += [_face(rng, 2, s), _face(rng, 3, s)]
        if not 40 <= s < 40 + DROP - 1:
            faces.append(_face(rng, 4, s))
        if s < 60 or s >= 60 + DROP:
            faces.append(_face(rng, 5, s))
        if 20 <= s < 120:
            faces.append(_face(rng, 6, s, degenerate=70 <= s < 74))
        script.append(faces)
    return script


def _frame(step):
    f = np.zeros((H, W, 3), dtype=np.uint8)
    f[0, 0, 0], f[0, 0, 1] = step & 255, step >> 8
    return f


def _same_record(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 4


@pytest.mark.parametrize("stride", [1, 8, 32, 52])
def test_live_call_keeps_the_reference_loops_books(stride):
    script = scripted_call()
    ring = CLIP + DROP                                         # the constructor's minimum: the script never needs more
    call = RecordingCall(clip_size=CLIP, size=64, stride=stride, crop_scale=0.6, ring_frames=ring, max_batch=16, drop_after=DROP)
    want = reference_loop(script, CLIP, stride, 0.6, DROP)
    closed_together = kept = purges = degenerate = 0
    lengths_5, lengths_1 = [], {}
    for s, faces in enumerate(script):
        n_scored = len(call.scored)
        results = call.step(_frame(s), faces)
        batch, purged = want[s]
        assert call.frame_idx == s and call.stored[-1] == (s, s % ring, (H, W, 3)) and len(call.stored) == s + 1
        assert sorted(call.purged) == purged, s
        got = call.scored[n_scored] if len(call.scored) > n_scored else []
        assert len(call.scored) - n_scored == (1 if batch else 0)
        assert [tid for tid, _ in got] == [tid for tid, _, _ in batch], s
        for (tid, win), (_, ids, infos) in zip(got, batch):
            assert [k for k, _ in win] == ids and len(ids) == CLIP, (s, tid)
            assert ids[-1] == s and ids[0] > s - ring                        # every frame of the window is still in the ring
            assert all(_same_record(rec, info) for (_, rec), info in zip(win, infos)), (s, tid)
            assert [tuple(rec[3]) for _, rec in win] == [tuple(info[3]) for info in infos]
        assert results == [(tid, float(np.float32(s + 0.001 * len(batch)))) for tid, _, _ in batch]
        closed_together += {2, 3} <= {tid for tid, _, _ in batch}
        purges += len(purged)
        kept += s == 40 + DROP - 1 and 4 in call._tracks and len(call._tracks[4].entries) > 1
        degenerate += s == 72 and call._tracks[6].missed == 0
        lengths_1[s] = len(call._tracks[1].entries)
        if 5 in call._tracks:
            lengths_5.append((s, len(call._tracks[5].entries)))
    # the script did what it says
    assert closed_together >= 1 and kept == 1 and degenerate == 1
    assert purges == 2 and want[60 + DROP - 1][1] == [5] and want[120 + DROP - 1][1] == [6]
    assert (60 + DROP, 1) in lengths_5 and (60 + DROP - 1, 0) not in lengths_5 and all(s != 60 + DROP - 1 for s, _ in lengths_5)
    assert sum(len(b) for b, _ in want) > (0 if stride > STEPS else 3)
    if stride == 52:                                           # keep_tail == 0: list[-0:] keeps the whole window, as the reference does
        assert [i for i, (b, _) in enumerate(want) if any(t == 1 for t, _, _ in b)] == [51, 103]
        assert lengths_1[51] == CLIP and lengths_1[52] == CLIP
    if stride == 1:                                            # keep_tail = CLIP - 1: a window per step once the track is full
        assert lengths_1[CLIP - 1] == CLIP - 1 and all(any(t == 1 for t, _, _ in want[i][0]) for i in range(CLIP - 1, STEPS))


def test_ring_frames_must_hold_a_window_and_a_gap():
    with pytest.raises(ValueError, match="ring_frames"):
        RecordingCall(clip_size=32, drop_after=90, ring_frames=121)
    with pytest.raises(ValueError, match="ring_frames"):
        RecordingCall(clip_size=32, ring_frames=96)                             # drop_after defaults to the reference's 90
    assert RecordingCall().ring_frames >= 32 + 90                              # the defaults agree with each other
    RecordingCall(clip_size=32, drop_after=90, ring_frames=122)
    with pytest.raises(ValueError, match="channel_order"):
        RecordingCall(channel_order="bgra")


def test_entries_that_left_the_ring_are_dropped_and_a_new_frame_size_reopens_it():
    """a track seen every third step spans 3 * CLIP frames, more than the ring holds: where the reference would go on holding its
    host crops, LiveCall drops the entries whose frames were overwritten, so no window ever names one"""
    rng = np.random.default_rng(3)
    ring = CLIP + DROP
    call = RecordingCall(clip_size=CLIP, size=64, stride=1, ring_frames=ring, drop_after=DROP)
    for s in range(90):
        call.step(_frame(s), [_face(rng, 9, s)] if s % 3 == 0 else [])
        ids = [k for k, _ in call._tracks[9].entries]
        assert ids and ids[-1] == s - s % 3
        if s % 3 == 0:                                         # checked where a window could close: on a step that saw the track
            assert min(ids) > s - ring and len(ids) == min(s // 3 + 1, 5)
    assert call.scored == []                                   # 14 frames hold 5 sightings: the window of 8 never fills
    with pytest.raises(ValueError):
        call.frame_view(0)
    # frame size change: the ring is re-opened, the windows start again, the counters stay
    call = RecordingCall(clip_size=CLIP, size=64, stride=4, ring_frames=ring, drop_after=DROP)
    for s in range(10):
        call.step(_frame(s), [_face(rng, 1, s)])
    assert len(call.scored) == 1 and len(call._tracks[1].entries) == 6
    big = np.zeros((H + 2, W, 3), dtype=np.uint8)
    assert call.step(big, [_face(rng, 1, 10)]) == []
    assert [k for k, _ in call._tracks[1].entries] == [10] and call._first == 10 and call.stored[-1][2] == (H + 2, W, 3)
    with pytest.raises(AssertionError):
        call.step(big[:, ::2], [])                             # not C-contiguous
