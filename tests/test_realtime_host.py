"""CPU: the host side of live.RealtimeCall, and tests/quality_ref.py - the numpy statement the quality kernel is checked against.

  restatement   quality_ref on crops worked out by hand here: 2x2 and 4x4 (the (a + b + c + d + 2) >> 2 form), 3x3 and 1x6 (whole
                ratios: box sum times fp32 1 / area), 1x5 and 5x4 (the area table; 1x5 has ratios 1 and 2.5, so it is a table case
                although one ratio is whole), a constant crop (lap = 0), a checkerboard of two-pixel blocks (every L = +-1020)
  weight        live.quality_weight against af_realtime.py:268-276 written out
  host loop     live.track_faces against af_realtime.py:390-442 written out (FaceMesh finding nothing), 150 steps with stub
                quality values: an excluded track, a track with no IoU match and no cache, cached landmarks (mesh_every = 3), a
                quality reject that stays alive, detect_every = 2
  alive=        LiveCall: a tid passed only in ``alive`` never closes a window and is not purged; without it the tid goes after
                drop_after steps
"""
import collections
import types

import numpy as np
import pytest

import quality_ref as Q
from af_mi355x import live
from af_mi355x.evaluator import get_crop_box
from af_mi355x.tracker import iou_distance


def _grey3(v):
    return np.repeat(np.asarray(v, dtype=np.uint8)[..., None], 3, axis=-1)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

def test_two_by_two_and_four_by_four_by_hand():
    crop = np.array([[[10, 20, 30], [11, 21, 33]], [[12, 22, 35], [14, 25, 38]]], dtype=np.uint8)
    small = Q.half_size(crop)
    # (10 + 11 + 12 + 14 + 2) >> 2 = 12, (20 + 21 + 22 + 25 + 2) >> 2 = 22, (30 + 33 + 35 + 38 + 2) >> 2 = 34
    assert small.tolist() == [[[12, 22, 34]]]
    # grey: (12 * 9798 + 22 * 19235 + 34 * 3735 + 16384) >> 15 = (117576 + 423170 + 126990 + 16384) >> 15 = 684120 >> 15 = 20
    assert Q.grey(small).tolist() == [[20]]
    # as B, G, R bytes: (34 * 9798 + 22 * 19235 + 12 * 3735 + 16384) >> 15 = (333132 + 423170 + 44820 + 16384) >> 15 = 817506 >> 15 = 24
    assert Q.grey(small, "bgr").tolist() == [[24]]
    assert Q.quality_sums(crop)[:3] == (1, 0, 0)                 # one pixel: every neighbour is the pixel itself
    four = _grey3([[0, 4, 100, 104], [8, 12, 108, 112], [50, 50, 7, 9], [50, 50, 9, 12]])
    g = Q.grey(Q.half_size(four))
    # blocks: (0 + 4 + 8 + 12 + 2) >> 2 = 6, (424 + 2) >> 2 = 106, 50, (7 + 9 + 9 + 12 + 2) >> 2 = 9; grey of (v, v, v) is v
    assert g.tolist() == [[6, 106], [50, 9]]
    # n = 2: index -1 -> 1 and index 2 -> 0, so both vertical neighbours are the other row and both horizontal ones the other column
    want = [[2 * 50 + 2 * 106 - 4 * 6, 2 * 9 + 2 * 6 - 4 * 106], [2 * 6 + 2 * 9 - 4 * 50, 2 * 106 + 2 * 50 - 4 * 9]]
    assert Q.laplacian(g).tolist() == want == [[288, -394], [-170, 276]]
    n, s1, s2, _ = Q.quality_sums(four)
    assert (n, s1, s2) == (4, 0, 288 ** 2 + 394 ** 2 + 170 ** 2 + 276 ** 2)
    assert Q.variance(n, s1, s2) == pytest.approx(np.var(np.array(want, dtype=np.float64)), rel=1e-14)


def test_whole_ratio_form_by_hand():
    three = _grey3([[1, 2, 3], [4, 5, 6], [7, 8, 4]])            # sum 40: fp32(40) * fp32(1 / 9) = 4.44 -> 4
    assert Q.half_size(three).tolist() == [[[4, 4, 4]]]
    half = _grey3([[1, 2, 3], [4, 5, 6], [7, 8, 4 + 1]])         # sum 41 -> 4.56 -> 5
    assert Q.half_size(half).tolist() == [[[5, 5, 5]]]
    tie = _grey3([[9], [0], [0], [0], [0], [0]])                 # 1 wide, 6 high: dw = 1, dh = 3, ratios 1 and 2: box of 2 -> 4.5 -> 4 (half to even)
    assert Q.half_size(tie)[:, 0, 0].tolist() == [4, 0, 0]
    tie[0, 0] = 11                                               # 5.5 -> 6
    assert Q.half_size(tie)[:, 0, 0].tolist() == [6, 0, 0]
    assert Q.quality_sums(three)[:3] == (1, 0, 0)


def test_area_table_by_hand():
    f = np.float32
    # 5 -> 2: scale 2.5; cell 0 covers [0, 2.5): pixels 0 and 1 whole (1 / 2.5), half of pixel 2 (0.5 / 2.5); cell 1 covers [2.5, 5)
    assert Q.area_table(5, 2) == [(0, 0, f(0.4)), (0, 1, f(0.4)), (0, 2, f(0.2)), (1, 2, f(0.2)), (1, 3, f(0.4)), (1, 4, f(0.4))]
    assert Q.area_table(4, 2) == [(0, 0, f(0.5)), (0, 1, f(0.5)), (1, 2, f(0.5)), (1, 3, f(0.5))]
    assert Q.area_table(1, 1) == [(0, 0, f(1.0))]
    # 7 -> 3: scale 7 / 3; cell 1 covers [2.333, 4.667): 2 / 3 of pixel 2, pixel 3, 2 / 3 of pixel 4
    t = [e for e in Q.area_table(7, 3) if e[0] == 1]
    assert [e[1] for e in t] == [2, 3, 4] and t[1][2] == f(3.0 / 7.0) and abs(float(t[0][2]) - 2.0 / 7.0) < 1e-7
    row = _grey3([[10, 20, 30, 40, 50]])                         # 1 high, 5 wide: ratios 1 and 2.5 - the table, not the whole-ratio form
    assert Q.half_size(row)[0, :, 0].tolist() == [18, 42]        # 4 + 8 + 6 and 6 + 16 + 20
    col = _grey3([[10], [20], [30], [40], [50]])
    assert Q.half_size(col)[:, 0, 1].tolist() == [18, 42]
    five_by_four = _grey3([[10, 20, 30, 40, 50]] * 4)            # w = 5, h = 4: x by the table, y two rows at 0.5 each
    g = Q.grey(Q.half_size(five_by_four))
    assert g.tolist() == [[18, 42], [18, 42]]
    assert Q.laplacian(g).tolist() == [[48, -48], [48, -48]]     # 18 + 18 + 42 + 42 - 72 and 42 + 42 + 18 + 18 - 168
    n, s1, s2, _ = Q.quality_sums(five_by_four)
    assert (n, s1, s2) == (4, 0, 4 * 48 * 48) and Q.variance(n, s1, s2) == 2304.0


def test_constant_crop_and_checkerboard():
    flat = np.full((37, 23, 3), 77, dtype=np.uint8)
    n, s1, s2, g = Q.quality_sums(flat)
    assert (n, s1, s2) == (18 * 11, 0, 0) and (g == 77).all() and Q.variance(n, s1, s2) == 0.0
    yy, xx = np.mgrid[0:24, 0:32]
    board = _grey3(np.where(((yy // 2) + (xx // 2)) % 2 == 0, 255, 0))
    n, s1, s2, g = Q.quality_sums(board)
    assert g.shape == (12, 16) and set(np.unique(g)) == {0, 255}
    lap = Q.laplacian(g)
    assert set(np.unique(np.abs(lap[1:-1, 1:-1]))) == {1020}     # 4 * 255 against 0, and the reflected border keeps the parity
    assert (n, s1, s2) == (192, 0, 192 * 1020 * 1020)


# ---- the weight --------------------------------------------------------------------------------------------------------------------------

def _reference_weight(min_side, lap, q_weighting, soft, hard, lap_soft, lap_hard):      # af_realtime.py:268-276
    if min_side < hard or lap < lap_hard:
        return 0.0
    if not q_weighting:
        return 1.0
    size_w = 1.0 if min_side >= soft else max(0.0, (min_side - hard) / max(1.0, (soft - hard)))
    lap_w = 1.0 if lap >= lap_soft else max(0.0, (lap - lap_hard) / max(1e-6, (lap_soft - lap_hard)))
    return float(size_w * lap_w)


def test_quality_weight_is_the_references():
    for side in (0.0, 31.0, 32.0, 40.0, 63.0, 64.0, 300.0):
        for lap in (0.0, 4.999, 5.0, 12.5, 19.9, 20.0, 1e4):
            for weighting in (True, False):
                assert live.quality_weight(side, lap, weighting) == _reference_weight(side, lap, weighting, 64, 32, 20.0, 5.0)
    assert live.quality_weight(48.0, 12.5) == 0.25 and live.quality_weight(32.0, 5.0) == 0.0 and live.quality_weight(31.9, 99.0) == 0.0
    assert live.quality_weight(40.0, 3.0, q_lap_hard=2.0, q_lap_soft=4.0, q_min_size_hard=40, q_min_size_soft=40) == 0.5


# ---- the host loop -----------------------------------------------------------------------------------------------------------------------

H, W = 240, 320
EXCLUDE = (0.70, 0.70, 1.00, 1.00)


def reference_host_loop(script, mesh_every, crop_scale, gate):
    """af_realtime.py:390-442 per step, FaceMesh finding nothing -> (faces, alive \\ faces, kept_boxes); plus last_lm and _q_hist"""
    last_lm, q_hist = {}, collections.defaultdict(lambda: collections.deque(maxlen=64))
    out = []
    for frame_idx, (dets, online, qvals) in enumerate(script):
        det_tlbr, dets_np = [], None                                                   # :391
        if dets is not None and len(dets) > 0:                                         # :392-395
            dets_np = np.asarray(dets, dtype=np.float32)
            for d in dets_np:
                x, y, wf, hf = d[:4]
                det_tlbr.append([x, y, x + wf, y + hf])
        det_tlbr = np.asarray(det_tlbr, dtype=np.float32) if det_tlbr else None        # :396
        faces, kept_boxes = [], {}
        for tr in online:                                                              # :401
            x1, y1, x2, y2 = tr.tlbr                                                   # :311-315
            cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
            if (EXCLUDE[0] * W <= cx <= EXCLUDE[2] * W) and (EXCLUDE[1] * H <= cy <= EXCLUDE[3] * H):     # :403
                continue
            tid = tr.track_id
            kept_boxes[tid] = tr.tlbr.astype(np.float32).copy()                        # :407
            yunet_lm5 = None
            if det_tlbr is not None and len(det_tlbr) > 0:                             # :414-418
                ious = 1.0 - iou_distance(np.array([tr.tlbr], dtype=np.float32), det_tlbr)[0]
                k = int(np.argmax(ious))
                if ious[k] >= 0.4:
                    yunet_lm5 = dets_np[k][5:15].reshape(5, 2)
            fm = None
            if (frame_idx % mesh_every) == 0 or (tid not in last_lm):                  # :421
                if fm is None and yunet_lm5 is not None:                               # :425
                    fm = {"lm5": yunet_lm5, "lm68": None}
                if fm is not None:                                                     # :426
                    last_lm[tid] = {**fm, "frame_idx": frame_idx}
            else:
                cached = last_lm.get(tid)                                              # :428-430
                if cached is not None:
                    fm = {"lm5": cached["lm5"], "lm68": cached["lm68"]}
                elif yunet_lm5 is not None:
                    fm = {"lm5": yunet_lm5, "lm68": None}
            if fm is None:                                                             # :431
                continue
            big = get_crop_box((H, W), tr.tlbr.astype(np.float32), scale=crop_scale)   # :435 (on the float32 box, as LiveCall cuts it)
            bx1, by1, bx2, by2 = map(int, big)
            if bx2 <= bx1 or by2 <= by1:                                               # :437
                continue
            q_side, q_lap = _stub_quality(frame_idx, (bx1, by1, bx2, by2))              # :439, the stub's value for this crop
            q_hist[tid].append((q_side, q_lap))                                        # :440
            if gate(q_side, q_lap) <= 0.0:                                             # :441
                continue
            faces.append((tid, tr.tlbr.astype(np.float32), fm["lm5"].astype(np.float32), (bx1, by1, bx2, by2)))
        out.append((faces, set(kept_boxes) - {f[0] for f in faces}, kept_boxes))
    return out, last_lm, q_hist


def _host_script(steps=150, seed=3):
    """per step (dets or None, online tracks, quality values in crop order).  Track 1 steady; 2 walks into the self-view rectangle
    and out; 3 never has a detection near it until step 60 (no IoU match, no cache); 4 is blurry on steps 30..34; 5 is degenerate
    for a while; detections only on even steps (detect_every = 2)"""
    rng = np.random.default_rng(seed)
    script = []
    for s in range(steps):
        boxes = {1: (40 + 0.2 * s, 30 + 0.1 * s, 50, 60), 2: (150 + 1.2 * s, 100 + 0.8 * s, 44, 52), 3: (20, 150, 46, 50),
                 4: (120 - 0.1 * s, 20, 48, 56)}
        if 50 <= s < 90:
            boxes[5] = (-80.0, 40.0, 20.0, 30.0) if 60 <= s < 66 else (200.0, 30.0, 40.0, 44.0)
        online, rows = [], []
        for tid, (x, y, w, h) in boxes.items():
            j = rng.uniform(-0.4, 0.4, 4)
            tlbr = np.array([x + j[0], y + j[1], x + w + j[2], y + h + j[3]], dtype=np.float64)
            online.append(types.SimpleNamespace(track_id=tid, tlbr=tlbr))
            if tid == 3 and s < 60:
                continue                                          # the detector does not see face 3 yet
            lm = rng.uniform(0, 1, (5, 2)) * [w, h] + [x, y]
            rows.append(np.concatenate([[x + rng.uniform(-2, 2), y + rng.uniform(-2, 2), w, h], [0.9], lm.ravel()]))
        dets = np.asarray(rows, dtype=np.float32) if s % 2 == 0 else None
        script.append((dets, online, None))
    return script


def _stub_quality(step, rect):
    """(min_side, lap) of a crop without pixels: track 4's crop (the only one whose left edge lies in 80..100) is blurry on steps 30..34"""
    x0, y0, x1, y1 = rect
    blurry = 30 <= step < 35 and 80 <= x0 <= 100
    return float(min(x1 - x0, y1 - y0)), 2.0 if blurry else 50.0 + 0.01 * x0 + 0.001 * step


def test_track_faces_is_the_reference_loop():
    gate = lambda m, l: live.quality_weight(m, l)
    base = _host_script()
    state, got, blurry_recorded = live.CallState(), [], 0
    for s, (dets, online, _) in enumerate(base):
        calls = []

        def quality(rects, s=s, calls=calls):
            calls.append(len(rects))
            return [_stub_quality(s, r) for r in rects]
        got.append(live.track_faces(state, s, (H, W), dets, online, quality, gate, mesh_every=3, exclude_rect=EXCLUDE))
        assert len(calls) <= 1                                    # every crop of a frame in one call
        blurry_recorded += 30 <= s < 35 and state.q_hist[4][-1][1] == 2.0
    want, last_lm, q_hist = reference_host_loop(base, 3, 0.6, gate)
    excluded = no_landmarks = cached = rejected = degenerate = 0
    for s, ((faces, alive, kept, rects), (wfaces, walive, wkept)) in enumerate(zip(got, want)):
        assert [f[0] for f in faces] == [f[0] for f in wfaces], s
        for f, wf in zip(faces, wfaces):
            assert f[1].dtype == np.float32 and np.array_equal(f[1], wf[1]) and f[2].dtype == np.float32 and np.array_equal(f[2], wf[2]), s
        assert alive == walive and set(kept) == set(wkept) and all(np.array_equal(kept[t], wkept[t]) for t in kept), s
        assert [r for r in rects if r in [wf[3] for wf in wfaces]] == [wf[3] for wf in wfaces], s
        online = base[s][1]
        excluded += any(t.track_id not in kept for t in online)
        no_landmarks += 3 in alive and s < 60
        cached += base[s][0] is None and any(f[0] == 1 for f in faces)
        rejected += 4 in alive and 30 <= s < 35
        degenerate += 5 in alive and 60 <= s < 66
    assert excluded >= 10 and no_landmarks == 60 and cached >= 50 and rejected == 5 and degenerate == 6
    assert set(state.last_lm) == set(last_lm) and all(np.array_equal(state.last_lm[t]["lm5"], last_lm[t]["lm5"]) and
                                                       state.last_lm[t]["frame_idx"] == last_lm[t]["frame_idx"] for t in last_lm)
    assert {t: list(v) for t, v in state.q_hist.items()} == {t: list(v) for t, v in q_hist.items()}
    assert len(state.q_hist[4]) == 64 and blurry_recorded == 5                              # a rejected crop is recorded before the gate


# ---- LiveCall's alive= -------------------------------------------------------------------------------------------------------------------

class RecordingCall(live.LiveCall):
    """LiveCall without the device: frames are dropped, windows are recorded"""

    def __init__(self, **k):
        super().__init__(None, **k)
        self.scored = []

    def _new_ring(self, shape):
        return None

    def _store_frame(self, frame, slot):
        pass

    def _score(self, ready):
        self.scored.append([tid for tid, _ in ready])
        return np.zeros(len(ready), dtype=np.float32)


def test_alive_keeps_a_track_that_contributes_nothing():
    frame = np.zeros((96, 131, 3), dtype=np.uint8)
    face = lambda tid: (tid, np.array([30, 30, 60, 66], dtype=np.float32), np.zeros((5, 2), np.float32) + 40)
    call = RecordingCall(clip_size=4, size=64, stride=2, ring_frames=16, drop_after=5)
    purged_at = {}
    for s in range(40):
        faces = [face(1)] + ([face(3)] if s < 3 else [])
        call.step(frame, faces, alive=[2])                       # tid 2: tracked, never a usable crop
        for tid in call.purged:
            purged_at[tid] = s
        assert 2 in call._tracks and call._tracks[2].missed == 0 and call._tracks[2].entries == []
    assert purged_at == {3: 2 + 5}                               # last seen on step 2, purged drop_after steps later; 2 never
    assert call.scored and all(2 not in tids for tids in call.scored) and any(1 in tids for tids in call.scored)
    for s in range(5):                                           # without alive= the same tid goes after drop_after steps
        assert 2 in call._tracks
        call.step(frame, [face(1)])
    assert 2 not in call._tracks and call.purged == [2]
    call.admit(frame)                                            # the two halves by themselves are the step
    call.advance([face(1)], alive=(7,))
    assert 7 in call._tracks and call.frame_idx == 45
