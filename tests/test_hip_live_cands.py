"""GPU: ``candidates="device"`` - a live tick's face stage without a host trip (csrc/af_live.hip, csrc/af_quality.hip).

  a  af_live_update_calls against its host twin af_live_update_host (which tests/test_live_cands_host.py pins to
     live.track_candidates) on the scripts of tests/live_cands_ref.py: the tracker's record, the candidate record and the state
     block equal byte for byte after every frame, for 1, 2, 64 and 65 calls per step; the same step twice from the same state gives
     the same bytes; the guard bands around every state block and around the records are untouched
  b  af_face_quality_records_u8 against af_face_quality_stores_u8 on the same rectangles: sums and grey bytes, for 0 / 1 / 64 jobs
     of 0, 1 and 32 candidates over three stores of different sizes, pitches and byte orders; a rectangle outside its frame and a
     slot outside its store are skipped and flagged while the others stay exact; the sums behind a job's count stay zero
  c  RealtimeCall(tracker="device", candidates="device") against candidates="host" over 150 scripted steps (the script of
     tests/test_hip_realtime.py, four seeds on end): a stride that wraps the ring, detect_every=2 and a detect_size; one wait per
     step, one more when a window closes; the host mode waits once more on every step that has a candidate
  d  a CallServer whose calls mix tracker="host", tracker="device" and candidates="device" at two frame sizes against the all-host
     server; with every call in the new mode at most two waits and exactly one records-quality launch per tick
  e  the ValueErrors of the keyword; the C entry refuses null, misaligned and shared blocks
All comparisons are exact.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import af_mi355x
import device_tracker_server_cases as sc
import live_cands_ref as L
from af_mi355x import _lib, live
from af_mi355x import device_tracker as dt

pytestmark = pytest.mark.gpu
GUARD = 512


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- a ---------------------------------------------------------------------------------------------------------------------------
def _twins(n):
    """n calls, call t on script t % len(ALL): per call a device tracker between guard bands and its host twin"""
    stride = dt.LIVE_STATE_BYTES + GUARD
    states = torch.full((GUARD + n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    device, host, scripts = [], [], []
    for t in range(n):
        args, frames = L.script(L.ALL[t % len(L.ALL)])
        d = dt.DeviceByteTracker(args, 30.0, device="cuda", candidates=True)
        d._state = states[GUARD + t * stride:GUARD + t * stride + dt.LIVE_STATE_BYTES]
        d.reset()
        device.append(d)
        host.append(dt.DeviceByteTracker(args, 30.0, host=True, candidates=True))
        scripts.append(frames)
    return states, device, host, scripts


def _state_bytes(states, t):
    at = GUARD + t * (dt.LIVE_STATE_BYTES + GUARD)
    return states[at:at + dt.LIVE_STATE_BYTES].tobytes()


@pytest.mark.parametrize("n", (1, 2, 64, 65))
def test_a_the_launch_equals_its_host_twin(n):
    states, device, host, scripts = _twins(n)
    trecs = torch.full((2 * GUARD + n * dt.RECORD_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    recs = torch.full((2 * GUARD + n * dt.LIVE_RECORD_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    trec_view = trecs[GUARD:GUARD + n * dt.RECORD_BYTES].view(n, dt.RECORD_BYTES)
    rec_view = recs[GUARD:GUARD + n * dt.LIVE_RECORD_BYTES].view(n, dt.LIVE_RECORD_BYTES)
    to_device = lambda a: torch.from_numpy(a).cuda()
    cands = 0
    for tick in range(max(len(s) for s in scripts)):
        now = [t for t in range(n) if tick < len(scripts[t])]
        keep = []
        jobs = [L.job_of(device[t], scripts[t][tick], tick % 5, to_device, keep) for t in now]
        trec_view.zero_()                                                      # the tracker writes the used part of its record only
        if n == 2:                                                             # the same step twice from the same state
            before = states.clone()
            dt.update_live_calls(jobs, torch.device("cuda"), trec_view[:len(now)], rec_view[:len(now)])
            first = (trec_view.cpu().numpy().tobytes(), rec_view.cpu().numpy().tobytes(), states.cpu().numpy().tobytes())
            states.copy_(before)
            trec_view.zero_()
        dt.update_live_calls(jobs, torch.device("cuda"), trec_view[:len(now)], rec_view[:len(now)])
        got_t, got_r, got_s = trec_view.cpu().numpy(), rec_view.cpu().numpy(), states.cpu().numpy()
        if n == 2:
            assert first == (got_t.tobytes(), got_r.tobytes(), got_s.tobytes()), tick
        for j, t in enumerate(now):
            want_t, want_r = dt.update_live_host(L.job_of(host[t], scripts[t][tick], tick % 5, torch.from_numpy, keep))
            assert got_t[j].tobytes() == want_t.tobytes(), (n, tick, t, "tracker record")
            assert got_r[j].tobytes() == want_r.tobytes(), (n, tick, t, "candidate record")
            assert _state_bytes(got_s, t) == host[t]._state.tobytes(), (n, tick, t, "state")
            host[t].absorb(want_t)
            device[t].absorb(got_t[j])
            cands += int(dt.parse_live_records(got_r[j])[0]["n_cands"])
    stride = dt.LIVE_STATE_BYTES + GUARD
    for t in range(n):
        at = GUARD + t * stride
        assert (got_s[at - GUARD:at] == 0xA5).all() and (got_s[at + dt.LIVE_STATE_BYTES:at + stride] == 0xA5).all(), t
    for whole, size in ((trecs.cpu().numpy(), n * dt.RECORD_BYTES), (recs.cpu().numpy(), n * dt.LIVE_RECORD_BYTES)):
        assert (whole[:GUARD] == 0xA5).all() and (whole[GUARD + size:] == 0xA5).all()
    assert cands >= 5 * min(n, 5)


# ---- b ---------------------------------------------------------------------------------------------------------------------------
STORES = (dict(h=96, w=131, pitch=393, n=4, bgr=1), dict(h=80, w=112, pitch=341, n=3, bgr=0), dict(h=50, w=67, pitch=202, n=5, bgr=1))


@pytest.fixture(scope="module")
def stores():
    """three stores of different sizes, row pitches (one packed, two padded) and byte orders: (device bytes, af_store_ref)"""
    rng, out = np.random.default_rng(41), []
    for s in STORES:
        stride = s["h"] * s["pitch"] + 7
        buf = torch.from_numpy(rng.integers(0, 256, s["n"] * stride, dtype=np.uint8)).cuda()
        out.append((buf, _lib.StoreRef(buf.data_ptr(), _lib.FrameStore(buf.numel(), stride, s["pitch"], s["n"], s["h"], s["w"], 0), s["bgr"], 0)))
    return out


def _record(rng, s, n_cands, slot):
    """a candidate record of n_cands rectangles of a frame of store s, other entries between them, as the candidate stage writes it"""
    rec = np.zeros(1, dtype=dt._LIVE_RECORD)[0]
    others = 0 if n_cands == dt.MAX_TRACKS else int(rng.integers(0, min(4, dt.MAX_TRACKS - n_cands) + 1))
    kinds = rng.permutation([1] * n_cands + [0] * others)
    tiles = k = 0
    for i, kind in enumerate(kinds):
        e = rec["online"][i]
        e["tid"], e["first_tile"], e["cand"] = i + 1, tiles, -1
        if not kind:
            e["flags"] = (_lib.AF_LIVE_EXCLUDED, _lib.AF_LIVE_NO_POINTS)[i % 2]
            continue
        w = int(rng.choice([1, 2, 3, int(rng.integers(4, 70)), s["w"]]))
        h = int(rng.choice([1, 2, 5, int(rng.integers(4, 50)), s["h"]]))
        w, h = min(w, s["w"]), min(h, s["h"])
        x, y = int(rng.integers(0, s["w"] - w + 1)), int(rng.integers(0, s["h"] - h + 1))
        e["flags"], e["box"], e["cand"] = _lib.AF_LIVE_CANDIDATE, (x, y, x + w, y + h), k
        tiles += L.tiles_of((x, y, x + w, y + h))
        k += 1
    rec["slot"], rec["n_online"], rec["n_cands"], rec["tiles"] = slot, len(kinds), n_cands, tiles
    return rec


def _listed(stores, rects):
    """af_face_quality_stores_u8 on ``rects`` = [(store index, slot, x0, y0, x1, y1)]: -> ([(n_px, s1, s2)], [grey bytes])"""
    from af_mi355x.evaluator import _RECT_DTYPE
    refs = (_lib.StoreRef * len(stores))(*[r for _, r in stores])
    sums_out, grey_out = [], []
    for lo in range(0, len(rects), _lib.QUALITY_MAX_RECTS):
        chunk = rects[lo:lo + _lib.QUALITY_MAX_RECTS]
        items = np.zeros(len(chunk), dtype=_RECT_DTYPE)
        for i, (s, slot, x0, y0, x1, y1) in enumerate(chunk):
            items[i] = (slot, x0, y0, y1 - y0, x1 - x0, 0, 0, s)
        sizes = [max(1, (r[5] - r[3]) // 2) * max(1, (r[4] - r[2]) // 2) for r in chunk]
        sums = torch.zeros(len(chunk) * 24, dtype=torch.uint8, device="cuda")
        grey = torch.zeros(sum(sizes), dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib.af_face_quality_stores_u8(refs, len(stores), C.c_void_p(items.ctypes.data), len(chunk), C.c_void_p(sums.data_ptr()),
                                                      C.c_void_p(grey.data_ptr()), grey.numel(), _stream()), "af_face_quality_stores_u8")
        raw, g, at = live.RecordsQuality.parse(sums.cpu().numpy()), grey.cpu().numpy(), 0
        for r, size in zip(raw, sizes):
            sums_out.append((int(r["n_px"]), int(r["s1"]), int(r["s2"])))
            grey_out.append(g[at:at + size].tobytes())
            at += size
    return sums_out, grey_out


GREY_STRIDE = 48 * 66                                          # the largest half-size image of the largest store


def _from_records(stores, records, slots=None, store_of=None):
    """af_face_quality_records_u8 on numpy records, job j out of store j % 3: -> (parsed sums, grey bytes (jobs, 32, GREY_STRIDE),
    the records as the launch left them)"""
    n = len(records)
    refs = (_lib.StoreRef * len(stores))(*[r for _, r in stores])
    dev = torch.from_numpy(np.array(records, dtype=dt._LIVE_RECORD).view(np.uint8).reshape(max(n, 1) if n else 0, -1).copy()).cuda() if n else \
        torch.zeros(0, dt.LIVE_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    jobs = (_lib.LiveQualityJob * max(n, 1))()
    for j in range(n):
        jobs[j].record, jobs[j].store = dev[j].data_ptr(), (j % 3 if store_of is None else store_of[j])
        jobs[j].slot = int(records[j]["slot"]) if slots is None else slots[j]
    sums = torch.full((max(n, 1) * dt.MAX_TRACKS * 24,), 0x5A, dtype=torch.uint8, device="cuda")
    grey = torch.zeros(max(n, 1) * dt.MAX_TRACKS * GREY_STRIDE, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.af_face_quality_records_u8(refs, len(stores), jobs, n, C.c_void_p(sums.data_ptr()), C.c_void_p(grey.data_ptr()), GREY_STRIDE,
                                                   _stream()), "af_face_quality_records_u8")
    torch.cuda.synchronize()
    return (live.RecordsQuality.parse(sums.cpu().numpy()), grey.cpu().numpy().reshape(max(n, 1), dt.MAX_TRACKS, GREY_STRIDE),
            dt.parse_live_records(dev.cpu().numpy()) if n else [])


@pytest.mark.parametrize("n_jobs", (0, 1, 64))
@pytest.mark.parametrize("n_cands", (0, 1, 32))
def test_b_the_records_launch_equals_the_listed_launch(stores, n_jobs, n_cands):
    rng = np.random.default_rng(100 * n_jobs + n_cands)
    records = [_record(rng, STORES[j % 3], n_cands if (j % 5 or n_jobs == 1) else max(0, n_cands - 1 - j % 3), int(rng.integers(0, STORES[j % 3]["n"])))
               for j in range(n_jobs)]
    sums, grey, after = _from_records(stores, records)
    if n_jobs == 0:
        assert (sums.view(np.uint8) == 0x5A).all()                             # nothing to do: nothing written
        return
    rects, where = [], []
    for j, rec in enumerate(records):
        for e in rec["online"][:int(rec["n_online"])]:
            if int(e["flags"]) & _lib.AF_LIVE_CANDIDATE:
                rects.append((j % 3, int(rec["slot"])) + tuple(int(v) for v in e["box"]))
                where.append((j, int(e["cand"])))
    want_sums, want_grey = _listed(stores, rects) if rects else ([], [])
    assert len(rects) == sum(int(r["n_cands"]) for r in records)
    filled = set()
    for (j, k), want, g in zip(where, want_sums, want_grey):
        got = sums[j * dt.MAX_TRACKS + k]
        assert (int(got["n_px"]), int(got["s1"]), int(got["s2"])) == want, (j, k)
        assert grey[j, k, :len(g)].tobytes() == g, (j, k)
        filled.add(j * dt.MAX_TRACKS + k)
    for i in range(n_jobs * dt.MAX_TRACKS):                                    # the sums behind a job's count stay zero
        assert i in filled or not sums[i].tobytes().strip(b"\0"), i
    assert all(int(r["bad"]) == 0 for r in after) and np.array(records, dtype=dt._LIVE_RECORD).tobytes() == np.array(after).tobytes()


def test_b_a_bad_rectangle_and_a_bad_slot_are_skipped_and_flagged(stores):
    rng = np.random.default_rng(43)
    records = [_record(rng, STORES[j % 3], 5, 1) for j in range(6)]
    victim = [i for i in range(dt.MAX_TRACKS) if int(records[1]["online"][i]["flags"]) & _lib.AF_LIVE_CANDIDATE][2]
    box = records[1]["online"][victim]["box"]
    box[0], box[2] = STORES[1]["w"] - 3, STORES[1]["w"] + 1                     # leaves its frame on the right
    slots = [1] * 6
    slots[3] = STORES[0]["n"]                                                  # job 3 (store 0) names a slot outside its store
    sums, grey, after = _from_records(stores, records, slots=slots)
    rects, where = [], []
    for j, rec in enumerate(records):
        for i, e in enumerate(rec["online"][:int(rec["n_online"])]):
            if int(e["flags"]) & _lib.AF_LIVE_CANDIDATE and j != 3 and (j, i) != (1, victim):
                rects.append((j % 3, 1) + tuple(int(v) for v in e["box"]))
                where.append((j, int(e["cand"])))
    want_sums, want_grey = _listed(stores, rects)
    for (j, k), want, g in zip(where, want_sums, want_grey):                   # the others stay exact
        got = sums[j * dt.MAX_TRACKS + k]
        assert (int(got["n_px"]), int(got["s1"]), int(got["s2"])) == want and grey[j, k, :len(g)].tobytes() == g, (j, k)
    assert [int(r["bad"]) for r in after] == [0, 1, 0, 1, 0, 0]
    for j, rec in enumerate(after):
        for i, e in enumerate(rec["online"]):
            is_cand = bool(int(records[j]["online"][i]["flags"]) & _lib.AF_LIVE_CANDIDATE)
            flagged = bool(int(e["flags"]) & _lib.AF_LIVE_BAD)
            assert flagged == (is_cand and (j == 3 or (j, i) == (1, victim))), (j, i)
    k = int(records[1]["online"][victim]["cand"])
    assert not sums[dt.MAX_TRACKS + k].tobytes().strip(b"\0") and not sums[3 * dt.MAX_TRACKS:4 * dt.MAX_TRACKS].tobytes().strip(b"\0")


# ---- c ---------------------------------------------------------------------------------------------------------------------------
STEPS_C = 150


@pytest.fixture(scope="module")
def long_script():
    from test_hip_realtime import _scripted
    steps = [s for seed in (4, 5, 6, 7) for s in _scripted(seed)]
    assert len(steps) >= STEPS_C
    return steps[:STEPS_C]


class _Stub:
    """scripted YuNet rows for one call; shown a resized frame it answers in that frame's coordinates"""

    def __init__(self, script, shape, every=1):
        self.script, self.shape, self.every, self.calls = script, shape, every, 0

    def detect(self, frames_u8):
        h, w = frames_u8.shape[1:3]
        mine = self.script[self.calls * self.every][1] / np.array([self.shape[1] / w, self.shape[0] / h] * 7 + [1.0], dtype=np.float32)
        self.calls += 1
        rows = torch.zeros(1, 16, 15, dtype=torch.float32, device=frames_u8.device)
        rows[0, :len(mine)] = torch.from_numpy(mine.astype(np.float32)).to(frames_u8.device)
        return rows, torch.tensor([len(mine)], dtype=torch.int32, device=frames_u8.device)


def _kept(c):
    return dict(purged=sorted(c.purged), state=copy.deepcopy(c.state), clip_hist={t: list(v) for t, v in c.clip_hist.items()},
                running={t: list(v) for t, v in c.running_scores.items()},
                detections=None if c.detections is None else np.array(c.detections, copy=True),
                last_boxes={t: np.array(b, copy=True) for t, b in c.last_boxes.items()},
                q_hist={t: list(v) for t, v in c.host.q_hist.items() if len(v)})


def _same_kept(a, b):
    same = all(a[k] == b[k] for k in ("purged", "state", "clip_hist", "running", "q_hist"))
    same = same and (a["detections"] is None) == (b["detections"] is None)
    same = same and (a["detections"] is None or (a["detections"].dtype == b["detections"].dtype and np.array_equal(a["detections"], b["detections"])))
    same = same and list(a["last_boxes"]) == list(b["last_boxes"])
    return same and all(a["last_boxes"][t].dtype == b["last_boxes"][t].dtype and np.array_equal(a["last_boxes"][t], b["last_boxes"][t]) for t in a["last_boxes"])


class _Waits:
    """counts the host's waits for the device: every ``Stream.synchronize``"""

    def __init__(self, monkeypatch):
        self.n = 0
        real = torch.cuda.Stream.synchronize

        def counted(stream):
            self.n += 1
            return real(stream)
        monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted)

    def take(self):
        n, self.n = self.n, 0
        return n


@pytest.mark.parametrize("variant", ("wrap", "detect_every", "detect_size"))
def test_c_a_call_equals_the_host_candidates(long_script, variant, monkeypatch):
    from test_hip_realtime import CLIP, DROP, EXCLUDE, GATE, H, RING, SIZE, STRIDE, W, _net
    # with detect_every=2 a face has an entry on every other frame: eight of them span 15 frames, so that call's ring is twice as long
    extra = {"wrap": {}, "detect_every": dict(detect_every=2, ring_frames=2 * RING), "detect_size": dict(detect_size=(88, 64))}[variant]
    every = extra.get("detect_every", 1)
    args = dict(dict(clip_size=CLIP, size=SIZE, stride=STRIDE, ring_frames=RING, drop_after=DROP, start_conf=0.76, start_min_size=20,
                     exclude_rect=EXCLUDE, tracker="device", **GATE), **extra)
    host = af_mi355x.RealtimeCall(_net(), detector=_Stub(long_script, (H, W), every), candidates="host", **args)
    device = af_mi355x.RealtimeCall(_net(), detector=_Stub(long_script, (H, W), every), candidates="device", **args)
    waits = _Waits(monkeypatch)
    scored = with_candidates = purged = counted = 0
    for s, (frame, _) in enumerate(long_script):
        measured, scorers = 0 if host._quality is None else host._quality.launches, (len(host.call._scorers), len(device.call._scorers))
        want = host.step(frame)
        measured = (0 if host._quality is None else host._quality.launches) - measured
        waits_host = waits.take()
        got = device.step(frame)
        waits_device = waits.take()
        assert got == want, (variant, s, got, want)                            # tids and scores, bit for bit
        assert _same_kept(_kept(device), _kept(host)), (variant, s)
        if scorers == (len(host.call._scorers), len(device.call._scorers)):              # (recording a forward for a new batch size waits on its own)
            assert waits_device == 1 + bool(want), (variant, s, waits_device)
            if s % every == 0 and measured:
                assert waits_host == waits_device + 1, (variant, s, waits_host, waits_device)
            counted += 1
        scored, with_candidates, purged = scored + len(want), with_candidates + bool(measured), purged + len(host.purged)
    assert scored >= 4 and with_candidates >= 30 and purged >= 2 and s >= 2 * RING and counted >= STEPS_C - 8, (variant, scored, with_candidates, purged, counted)
    # the host mode reads a tick without a detection with the next rows: its lists lag by the records still pending, 2 frames each
    assert device.tracker.frame_id == host.tracker.frame_id + 2 * len(host._track_pending) > 0 and not device._track_pending


# ---- d ---------------------------------------------------------------------------------------------------------------------------
def _serve(scripts, modes):
    from test_hip_device_tracker import ShapeStub, _call_args
    from test_hip_server import CLIP, SIZE, _net
    server = af_mi355x.CallServer(_net(), detector=ShapeStub(scripts), clip_size=CLIP, size=SIZE)
    cids = {n: server.open(**dict(_call_args(n), **modes[n])) for n in scripts}
    launches, ticks = lambda: 0 if server._records_quality is None else server._records_quality.launches, []
    for s in range(sc.TICKS):
        before = launches()
        got = server.step({cids[n]: scripts[n][s][0] for n in scripts})
        ticks.append(({n: got[cids[n]] for n in scripts}, {n: _kept(server.call(cids[n])) for n in scripts}, dict(server.stats.last),
                      server.stats.last["track"], launches() - before))
    return ticks


HOST, TRACKER, NEW = dict(tracker="host"), dict(tracker="device"), dict(tracker="device", candidates="device")


@pytest.mark.parametrize("modes", ({"A": NEW, "B": TRACKER, "C": HOST}, {"A": HOST, "B": NEW, "C": NEW}, {"A": NEW, "B": NEW, "C": NEW}, {"A": NEW}),
                         ids=("mixed", "mixed2", "all", "alone"))
def test_d_a_server_of_mixed_calls_equals_the_all_host_server(modes):
    scripts = {n: script for n, script in sc.scripts().items() if n in modes}          # "alone": every other tick no call detects
    want = _serve(scripts, {n: HOST for n in scripts})
    got = _serve(scripts, modes)
    all_new = all(m is NEW for m in modes.values())
    scored = 0
    for s, ((got_h, kept_h, stats_h, _, _), (got_d, kept_d, stats_d, track_d, launches_d)) in enumerate(zip(want, got)):
        assert got_d == got_h, (s, got_d, got_h)                               # per call and tick: tids and scores, bit for bit
        for n in scripts:
            assert _same_kept(kept_d[n], kept_h[n]), (s, n)
        assert launches_d == 1 and track_d >= 1, (s, launches_d, track_d)      # one records-quality launch for all calls of the new mode
        assert all(stats_d[k] == stats_h[k] for k in ("detect", "warp", "replay")), (s, stats_d, stats_h)
        if all_new:
            assert stats_d["wait"] == 1 + bool(stats_h["replay"]) <= 2 and stats_d["quality"] == 1, (s, stats_d)
            assert track_d == 1                                                # three calls fit one launch's arguments
        scored += sum(len(v) for v in got_h.values())
    assert scored >= 6 if len(modes) == 3 else any(kept["A"]["q_hist"] for _, kept, _, _, _ in got)        # alone, A never holds a whole window in its ring


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def test_e_the_keyword_and_the_c_entry_refuse_what_they_cannot_do():
    from test_hip_server import CLIP, SIZE, _net
    stub = _Stub([], (96, 131))
    with pytest.raises(ValueError, match="tracker=\"device\""):
        af_mi355x.RealtimeCall(_net(), detector=stub, clip_size=CLIP, size=SIZE, ring_frames=100, candidates="device")
    with pytest.raises(ValueError, match="reads a frame on the host"):
        af_mi355x.RealtimeCall(_net(), detector=stub, clip_size=CLIP, size=SIZE, ring_frames=100, tracker="device", candidates="device",
                               landmarks=lambda view, box: None)
    with pytest.raises(ValueError, match="\"host\" or \"device\""):
        af_mi355x.RealtimeCall(_net(), detector=stub, clip_size=CLIP, size=SIZE, ring_frames=100, tracker="device", candidates="gpu")
    server = af_mi355x.CallServer(_net(), detector=stub, clip_size=CLIP, size=SIZE, ring_frames=100, tracker="device", candidates="device")
    assert server.call(server.open()).candidates_mode == "device" and server.call(server.open(candidates="host")).candidates_mode == "host"
    with pytest.raises(ValueError, match="tracker=\"device\""):
        server.open(tracker="host")
    with pytest.raises(ValueError, match="reads a frame on the host"):
        server.open(landmarks=lambda view, box: None)
    a, b = (dt.DeviceByteTracker(L.cases._args(), 30.0, device="cuda", candidates=True) for _ in range(2))
    trec = torch.zeros(2 * dt.RECORD_BYTES + 8, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(2 * dt.LIVE_RECORD_BYTES + 8, dtype=torch.uint8, device="cuda")
    job = lambda tr: tr.live_job(tr.empty_job(), frame_idx=0, slot=0, shape=(96, 131), mesh_every=1, crop_scale=0.6, exclude_rect=L.EXCLUDE)
    fn = lambda jobs, n, t=trec.data_ptr(), r=rec.data_ptr(): _lib.lib.af_live_update_calls((_lib.LiveCall * len(jobs))(*jobs) if jobs else None, n,
                                                                                             C.c_void_p(t), C.c_void_p(r), _stream())
    assert fn([job(a), job(b)], 2) == 0
    assert fn(None, 1) != 0 and fn([job(a)], 1, 0) != 0 and fn([job(a)], 1, r=0) != 0                       # null
    assert fn([job(a)], 1, trec.data_ptr() + 4) != 0 and fn([job(a)], 1, r=rec.data_ptr() + 4) != 0        # misaligned
    assert fn([job(a)], 0) != 0 and fn([job(a)] * 65, 65) != 0                                              # 1 to 64 calls
    assert fn([job(a), job(a)], 2) != 0 and b"share a state block" in _lib.lib.af_last_error()
    bad = job(a)
    bad.mesh_every = 0
    assert fn([job(b), bad], 2) != 0                                                                        # refused before the first launch
    torch.cuda.synchronize()
    assert a.update([], (96, 131), (96, 131)) == [] and a.frame_id == 4                                     # the tracker's own entry works on the bigger block
