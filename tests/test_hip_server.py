"""GPU: live.CallServer - many live calls stepped on shared launches - against lone RealtimeCall objects fed the same frames, on the
network, clip size and frame sizes tests/test_hip_live.py and tests/test_hip_realtime.py use (a shrunken synthetic I3D in f16, 8
frames of 64 x 64; frames of 96 x 131 and of 80 x 112).

  three calls   A and B are 96 x 131 B, G, R; C is 80 x 112 R, G, B; each has its own script of stub detections (two faces, one
                blurry for five ticks, one walking through the self-view rectangle).  B opens at tick 5, A is absent from the
                mapping on ticks 16 and 17, C is closed after tick 33.  Per call and per tick the tids, purged, state, clip_hist,
                the keys of running_scores, detections and last_boxes equal a lone RealtimeCall's; the scores are bit for bit
                forward_clips_u8(clips, return_scores=True) at the padded batch size, clips being the tick's windows in the
                server's order warped the parents' way (StreamingCropAligner over host-cut crops); with max_batch = 16 and with
                max_batch = 2.  The cases the scripts must produce are asserted on the reference alone, first.
  economy       from server.stats: one detect call per frame size, one quality launch per tick with candidates, one warp and one
                replay per max_batch windows, at most three host waits per tick, uploaded_bytes = the frames handed in
  real YuNet    three calls of one size at conf 0.05: every call's detections are YuNet.infer(frame)'s, one detect launch per tick
"""
import copy

import numpy as np
import pytest
import torch

import af_mi355x
from af_mi355x import aligner, live, synth
from af_mi355x.classifier import I3D8x8
from af_mi355x.evaluator import get_crop_box, partition
from test_hip_yunet import MODEL, frames as yunet_frames

pytestmark = pytest.mark.gpu
CLIP, SIZE = 8, 64
DROP, STRIDE, TICKS = 6, 3, 40
RING = CLIP + DROP
EXCLUDE = (0.70, 0.70, 1.00, 1.00)
GATE = dict(q_min_size_soft=24, q_min_size_hard=12, q_lap_soft=20.0, q_lap_hard=5.0)
#        frame size, channel order, seed, blurry ticks of face 1 (the call's own ticks), face 1's start and drift, face 2's start and drift
CALLS = {"A": ((96, 131), "bgr", 4, range(10, 15), (14, 22, 0.5, 0.1), (50, 40, 5.0, 2.5)),
         "B": ((96, 131), "bgr", 5, range(18, 23), (12, 24, 0.4, 0.1), (52, 38, 5.0, 2.5)),
         "C": ((80, 112), "rgb", 6, range(13, 18), (8, 20, 0.25, 0.1), (52, 30, 2.5, 2.0))}
OPENS = {"A": 0, "B": 5, "C": 0}
ABSENT = {"A": (16, 17)}
CLOSES = {"C": 34}                                                # closed before this tick
_nets = {}


def _net():
    if "i3d" not in _nets:
        net = I3D8x8(clip_size=CLIP, crop_size=SIZE, precision="f16")
        net.load_state_dict(synth.synthetic_state_dict(net.spec, seed=5))
        _nets["i3d"] = net.cuda().eval()
    return _nets["i3d"]


def _args(order):
    return dict(stride=STRIDE, ring_frames=RING, drop_after=DROP, start_conf=0.76, start_min_size=20, exclude_rect=EXCLUDE,
                channel_order=order, **GATE)


def stepping(tick):
    """the calls in a tick's mapping, in its order"""
    return [n for n in CALLS if OPENS[n] <= tick < CLOSES.get(n, TICKS) and tick not in ABSENT.get(n, ())]


def scripted(name):
    """per tick of the call: the frame and the YuNet rows of two faces (tests/test_hip_realtime.py's script, per call): face 1
    drifts and is blurry - its crop a flat patch - on the call's blurry ticks; face 2 walks into the self-view rectangle (ticks 12..21)
    and back out"""
    (H, W), _, seed, blurry, (x1, y1, dx1, dy1), (x2, y2, dx2, dy2) = CALLS[name]
    rng = np.random.default_rng(seed)
    std = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
    out = []
    for s in range(TICKS):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        t = min(max(s - 8, 0), 8) if s < 22 else max(0, 8 - (s - 21))
        faces = [(x1 + dx1 * s, y1 + dy1 * s, 30, 34, 0.95), (x2 + dx2 * t, y2 + dy2 * t, 28, 32, 0.93)]
        rows = []
        for x, y, w, h, sc in faces:
            j = rng.uniform(-0.3, 0.3, 4)
            x, y, w, h = x + j[0], y + j[1], w + j[2], h + j[3]
            lm = std * [w, h] + [x, y] + rng.normal(0, 0.4, (5, 2))
            rows.append(np.concatenate([[x, y, w, h], [sc + rng.uniform(-0.004, 0.004)], lm.ravel()]))
        rows = np.asarray(rows, dtype=np.float32)
        if s in blurry:
            bx1, by1, bx2, by2 = map(int, get_crop_box((H, W), [rows[0, 0], rows[0, 1], rows[0, 0] + rows[0, 2], rows[0, 1] + rows[0, 3]], scale=0.6))
            frame[max(0, by1 - 6):by2 + 6, max(0, bx1 - 6):bx2 + 6] = 90
        out.append((frame, rows))
    return out


class StubDetector:
    """scripted YuNet rows, looked up by the bytes of the resident frame the detector is shown: ``detect`` as RealtimeCall calls
    it, ``detect_views`` as CallServer does"""

    def __init__(self, scripts):
        self.rows = {frame.tobytes(): rows for script in scripts.values() for frame, rows in script}
        self.frames_seen = 0

    def _answer(self, views):
        dev = views[0].device
        rows = torch.zeros(len(views), 16, 15, dtype=torch.float32, device=dev)
        counts = []
        for b, v in enumerate(views):
            mine = self.rows[v.cpu().numpy().tobytes()]           # KeyError: the detector was shown something else than the frame
            rows[b, :len(mine)] = torch.from_numpy(mine).to(dev)
            counts.append(len(mine))
        self.frames_seen += len(views)
        return rows, torch.tensor(counts, dtype=torch.int32, device=dev)

    def detect(self, frames_u8):
        assert frames_u8.is_cuda and frames_u8.shape[0] == 1
        return self._answer([frames_u8[0]])

    def detect_views(self, views):
        assert len({tuple(v.shape) for v in views}) == 1
        return self._answer(list(views))


class _Parent:
    """one StreamingCropAligner per face over host-cut crops of the R, G, B frame (af_realtime.py:434-451), as
    tests/test_hip_live.py composes it"""

    def __init__(self, shape, order, crop_scale=0.6):
        self.shape, self.order, self.crop_scale, self.aligners = shape, order, crop_scale, {}

    def push(self, frame, faces):
        H, W = self.shape
        frgb = frame[..., ::-1] if self.order == "bgr" else frame
        for tid, tlbr, lm5 in faces:
            x1, y1, x2, y2 = map(int, get_crop_box((H, W), tlbr, scale=self.crop_scale))
            top_left = np.array([[x1, y1]], dtype=np.float32)
            record = ((tlbr.reshape(2, 2).astype(np.float32) - top_left).reshape(-1), lm5.astype(np.float32) - top_left,
                      np.zeros((68, 2), np.float32), np.array([x1, y1, x2, y2], dtype=np.int32))
            if tid not in self.aligners:
                self.aligners[tid] = aligner.StreamingCropAligner(size=SIZE, capacity=32, max_crop_pixels=H * W)
            self.aligners[tid].push(record, frgb[y1:y2, x1:x2])

    def clip(self, tid):
        return self.aligners[tid].align_last(CLIP)[1].clone()


@pytest.fixture(scope="module")
def scripts():
    return {name: scripted(name) for name in CALLS}


@pytest.fixture(scope="module")
def reference(scripts):
    """the three calls as lone RealtimeCall objects, stepped on the ticks the server steps them on.  Per tick and call: what the
    call returned and kept, the faces it handed its LiveCall (recorded at ``advance``), the tracks its tracker had online, and the
    closed windows warped the parents' way"""
    det = StubDetector(scripts)
    lone, parents, own, seen = {}, {}, {}, {}
    out = []
    for tick in range(TICKS):
        row = {}
        for name in stepping(tick):
            (H, W), order = CALLS[name][:2]
            if name not in lone:
                c = lone[name] = af_mi355x.RealtimeCall(_net(), detector=det, clip_size=CLIP, size=SIZE, **_args(order))
                parents[name], own[name], seen[name] = _Parent((H, W), order), 0, {}
                advance, update = c.call.advance, c.tracker.update

                def recording_advance(faces, alive=(), advance=advance, log=seen[name]):
                    log["faces"], log["alive"] = list(faces), set(alive)
                    return advance(faces, alive)

                def recording_update(*a, update=update, log=seen[name]):
                    log["online"] = update(*a)
                    return log["online"]
                c.call.advance, c.tracker.update = recording_advance, recording_update
            c = lone[name]
            frame = scripts[name][own[name]][0]
            own[name] += 1
            measured = {t: len(v) for t, v in c.host.q_hist.items()}
            results = c.step(frame)
            log = seen[name]
            parents[name].push(frame, log["faces"])
            crops = sum(len(v) - measured.get(t, 0) for t, v in c.host.q_hist.items())
            row[name] = dict(
                results=results, tids=[t for t, _ in results], purged=sorted(c.purged), state=copy.deepcopy(c.state),
                clip_hist={t: list(v) for t, v in c.clip_hist.items()}, running=sorted(c.running_scores), detections=c.detections.copy(),
                last_boxes={t: b.copy() for t, b in c.last_boxes.items()}, clips=[parents[name].clip(t) for t, _ in results],
                crops=crops, rejected=crops - len(log["faces"]), excluded=sum(live.in_exclude(t.tlbr, H, W, EXCLUDE) for t in log["online"]),
                frame=frame, call_tick=own[name] - 1)
        out.append(row)
    return out


def test_the_scripts_produce_the_cases(reference):
    closes = [{n: len(r["tids"]) for n, r in row.items() if r["tids"]} for row in reference]
    assert any("C" in c and ("A" in c or "B" in c) for c in closes), closes              # both frame sizes on one tick
    assert any(sum(c.values()) >= 3 for c in closes) and any(sum(c.values()) == 3 for c in closes), closes
    assert any(r["tids"] and r["call_tick"] >= RING for row in reference for r in row.values())      # a close after a ring wrap
    assert any(r["rejected"] for row in reference for r in row.values())                 # the gate says no
    assert any(r["excluded"] for row in reference for r in row.values())                 # the self-view rectangle
    assert any(len(c) >= 2 for c in closes)                                              # windows of several calls on one tick
    assert all("A" not in row for t, row in enumerate(reference) if t in ABSENT["A"]) and "B" not in reference[4] and "B" in reference[5]
    assert "C" in reference[33] and "C" not in reference[34]
    assert any(r["purged"] for row in reference for r in row.values())


def _same_boxes(a, b):
    return set(a) == set(b) and all(np.array_equal(a[t], b[t]) for t in a)


@pytest.mark.parametrize("max_batch", [16, 2])
def test_the_server_equals_lone_calls_and_the_parents_scores(scripts, reference, max_batch):
    net = _net()
    server = af_mi355x.CallServer(net, detector=StubDetector(scripts), max_batch=max_batch, clip_size=CLIP, size=SIZE, **_args("bgr"))
    cids, uploaded, split = {}, 0, 0
    for tick, row in enumerate(reference):
        for name in CALLS:
            if OPENS[name] == tick:
                cids[name] = server.open(channel_order=CALLS[name][1])
            if CLOSES.get(name) == tick:
                server.close(cids.pop(name))
                with pytest.raises(KeyError):
                    server.step({max(cids.values()) + 1: row["A"]["frame"]})
        names = stepping(tick)
        assert names == list(row) and all(n in cids for n in names)
        got = server.step({cids[n]: row[n]["frame"] for n in names})
        assert list(got) == [cids[n] for n in names]
        uploaded += sum(row[n]["frame"].nbytes for n in names)
        assert server.uploaded_bytes == uploaded
        # the books of every call are a lone call's
        for n in names:
            want, c = row[n], server.call(cids[n])
            assert [t for t, _ in got[cids[n]]] == want["tids"] and sorted(c.purged) == want["purged"], (tick, n)
            assert c.state == want["state"] and {t: list(v) for t, v in c.clip_hist.items()} == want["clip_hist"], (tick, n)
            assert sorted(c.running_scores) == want["running"] and np.array_equal(c.detections, want["detections"]), (tick, n)
            assert _same_boxes(c.last_boxes, want["last_boxes"]) and c.frame_idx == want["call_tick"], (tick, n)
        # the scores are the eager forward's on the parents' clips, in the server's order, at the server's batch sizes
        clips = [clip for n in names for clip in row[n]["clips"]]
        scores = [s for n in names for _, s in got[cids[n]]]
        parts = partition(len(clips), max_batch)
        for first, k, run in parts:
            batch = torch.stack(clips[first:first + k] + [clips[first + k - 1]] * (run - k))
            with torch.inference_mode():
                want = net.forward_clips_u8(batch, return_scores=True)["scores"][:k].float().cpu()
            assert torch.equal(torch.tensor(scores[first:first + k], dtype=torch.float32), want), (tick, first, scores, want)
            if (first, k, run) == parts[-1]:                      # what the last warp left in the clip buffer: the parents' bytes
                assert torch.equal(server._scorers[run].clip, batch), (tick, first)
        split += len(parts) > 1
        # economy
        st = server.stats.last
        assert st["detect"] == len({CALLS[n][0] for n in names}) and st["quality"] == (1 if sum(row[n]["crops"] for n in names) else 0), (tick, st)
        assert st["warp"] == st["replay"] == len(parts) and st["wait"] <= 3, (tick, st)
        assert st["wait"] == 1 + st["quality"] + (1 if clips else 0)
    assert server.stats.steps == TICKS and server.stats.total["detect"] == sum(len({CALLS[n][0] for n in stepping(t)}) for t in range(TICKS))
    assert (split >= 1) == (max_batch == 2) and len(server) == 2
    assert server.call(cids["A"]).pick_interlocutor_id(96, 131) in server.call(cids["A"]).last_boxes
    with pytest.raises(RuntimeError):
        server.call(cids["A"]).step(reference[0]["A"]["frame"])   # a served call's ring belongs to the server


def test_a_new_frame_size_reopens_only_that_calls_ring(scripts):
    server = af_mi355x.CallServer(_net(), detector=StubDetector(scripts), clip_size=CLIP, size=SIZE, **_args("bgr"))
    a, b = server.open(), server.open()
    for s in range(3):
        server.step({a: scripts["A"][s][0], b: scripts["B"][s][0]})
    ring_b = server.call(b).call._ring.store
    out = server.step({a: np.ascontiguousarray(scripts["C"][3][0]), b: scripts["B"][3][0]})          # call a now sends 80 x 112
    assert out == {a: [], b: []} and server.stats.last["detect"] == 2
    assert server.call(a).call._ring.store.shape == (80, 112, 3) and server.call(a).call._first == 3
    assert server.call(b).call._ring.store is ring_b and server.call(b).frame_idx == 3
    assert server.step({b: scripts["B"][4][0]}) == {b: []} and server.call(a).frame_idx == 3         # a call not in the mapping stands still
    assert server.step({}) == {}


def test_three_calls_share_one_real_yunet_launch():
    from af_mi355x.detector import YuNet
    h, w = 96, 131
    alone = YuNet(MODEL, inputSize=[w, h], confThreshold=0.05)
    server = af_mi355x.CallServer(_net(), detector=YuNet(MODEL, inputSize=[w, h], confThreshold=0.05), clip_size=CLIP, size=SIZE, **_args("bgr"))
    cids = [server.open() for _ in range(3)]
    frames = [yunet_frames(3, w, h, seed=seed) for seed in (23, 51, 31)]          # per call; each set holds a detection at conf 0.05
    total = 0
    for tick in range(3):
        server.step({cid: np.ascontiguousarray(frames[i][tick]) for i, cid in enumerate(cids)})
        assert server.stats.last["detect"] == 1 and server.stats.last["wait"] <= 3
        for i, cid in enumerate(cids):
            want, got = alone.infer(frames[i][tick]), server.call(cid).detections
            assert got.dtype == np.float32 and got.shape == (len(want), 15) and (len(want) == 0 or np.array_equal(got, want)), (tick, i)
            total += len(want)
        assert server.uploaded_bytes == (tick + 1) * 3 * h * w * 3
    assert total >= 1


class _ManyRows:
    """a detector that answers, for the frame whose first byte is k, with k rows (no kernel of the library is involved)"""

    def __init__(self, capacity=80):
        rng = np.random.default_rng(9)
        self.rows = rng.uniform(1.0, 60.0, (capacity, 15)).astype(np.float32)
        self.rows[:, 4] = 0.5                                     # under start_conf: the rows reach ``detections`` and no tracker

    def detect_views(self, views):
        counts = torch.stack([v[0, 0, 0] for v in views]).to(torch.int32)
        return torch.from_numpy(self.rows).to(views[0].device)[None].repeat(len(views), 1, 1), counts

    def detect(self, frames_u8):
        return self.detect_views([frames_u8[0]])


def test_a_frame_with_more_than_64_rows_costs_one_more_wait_and_loses_none():
    """the second copy of the detection read-back, in both of its callers: a 64 x 64 frame for which the detector reports 65 rows"""
    net, det = torch.nn.Linear(1, 1).cuda(), _ManyRows()          # the network only names the device: no window closes here
    frame = lambda k: np.full((64, 64, 3), k, dtype=np.uint8)    # noqa: E731
    lone = af_mi355x.RealtimeCall(net, detector=det, clip_size=CLIP, size=SIZE, **_args("bgr"))
    for k in (64, 65, 3):
        assert lone.step(frame(k)) == [] and np.array_equal(lone.detections, det.rows[:k]) and lone.detections.shape == (k, 15)
    server = af_mi355x.CallServer(net, detector=det, clip_size=CLIP, size=SIZE, **_args("bgr"))
    a, b = server.open(), server.open()
    waits = []
    for ka, kb in ((64, 7), (65, 7), (7, 65), (65, 65)):
        assert server.step({a: frame(ka), b: frame(kb)}) == {a: [], b: []}
        assert np.array_equal(server.call(a).detections, det.rows[:ka]) and np.array_equal(server.call(b).detections, det.rows[:kb])
        assert server.stats.last["detect"] == 1 and server.stats.last["quality"] == 0
        waits.append(server.stats.last["wait"])
    assert waits == [1, 2, 2, 3]                                  # the read-back, and one more per frame with more than 64 rows
