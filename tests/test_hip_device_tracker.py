"""GPU: the device tracker (csrc/af_track.hip) against its numpy statement (tests/bytetrack_ref.py), and CallServer / RealtimeCall
with ``tracker="device"`` against the host tracker.

  g  af_track_probe_f64: fp64 divide and square root in device code give numpy's results bit for bit - what h rests on
  h  DeviceByteTracker.update on the golden and every script equals the statement by np.array_equal after every frame; 65 trackers
     on time-shifted scripts stepped by update_calls (two launches) each equal their lone run; the guard bands around every state
     block and around the records are untouched
  i  a scripted detector's (B, N, 15) rows and counts read in place: rows under start_conf or start_min_size, counts of 0 and a
     detect_size scale-back give RealtimeCall._track's filter followed by the statement
  j  CallServer(tracker="device") against CallServer() on three scripted calls (tests/device_tracker_server_cases.py)
  k  RealtimeCall(tracker="device") against RealtimeCall() on one of them
  l  two runs of h's batch give the same record bytes
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import af_mi355x
import bytetrack_cases as cases
import bytetrack_ref as ref
import device_tracker_server_cases as sc
from af_mi355x import _lib, live
from af_mi355x import device_tracker as dt

pytestmark = pytest.mark.gpu
GUARD = 512


# ---- g ---------------------------------------------------------------------------------------------------------------------------
def _probe_inputs():
    rng = np.random.default_rng(7)
    x, y = [], []
    a, b = rng.uniform(0.5, 2.0, 512) * 2.0 ** rng.integers(-300, 300, 512), rng.uniform(0.5, 2.0, 512) * 2.0 ** rng.integers(-300, 300, 512)
    x += list(a); y += list(b)                                             # anything
    m, d = np.floor(rng.uniform(2 ** 25, 2 ** 26, 512)), np.floor(rng.uniform(2 ** 25, 2 ** 26, 512))
    x += list(m * d); y += list(d)                                         # exact quotients,
    x += list(np.nextafter(m * d, np.inf)); y += list(d)                   #   and their neighbours
    x += list(np.nextafter(m * d, 0.0)); y += list(d)
    k = np.floor(rng.uniform(1, 2 ** 20, 512))
    x += list((2 * k + 1) * 2.0 ** -1040); y += [2.0 ** 35] * 512          # subnormal quotients exactly on a rounding tie
    x += list(rng.uniform(1.0, 2.0, 512) * 2.0 ** -1030); y += list(rng.uniform(1.0, 2.0, 512) * 2.0 ** rng.integers(20, 44, 512))   # subnormal
    s = np.floor(rng.uniform(2, 2 ** 26, 341))
    x += list(s * s) + list(np.nextafter(s * s, np.inf)) + list(np.nextafter(s * s, 0.0)); y += [3.0] * 1023      # next to perfect squares
    x += [0.0]; y += [1.0]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert len(x) == len(y) == 4096
    return x, y


def test_g_divide_and_square_root_are_correctly_rounded_on_the_device():
    x, y = _probe_inputs()
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    q, r = torch.empty_like(dx), torch.empty_like(dx)
    _lib.check(_lib.lib.af_track_probe_f64(dx.data_ptr(), dy.data_ptr(), q.data_ptr(), r.data_ptr(), len(x),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "af_track_probe_f64")
    q, r = q.cpu().numpy(), r.cpu().numpy()
    want_q, want_r = x / y, np.sqrt(x)
    bad_q, bad_r = np.flatnonzero(q.view(np.int64) != want_q.view(np.int64)), np.flatnonzero(r.view(np.int64) != want_r.view(np.int64))
    sub = (want_q != 0) & (np.abs(want_q) < 2.0 ** -1022)
    print("divide: %d of %d differ (%d subnormal quotients); sqrt: %d differ" % (len(bad_q), len(x), int(sub.sum()), len(bad_r)))
    assert sub.sum() >= 1000
    assert len(bad_q) == 0, [(x[i].hex(), y[i].hex(), q[i].hex(), want_q[i].hex()) for i in bad_q[:4]]
    assert len(bad_r) == 0, [(x[i].hex(), r[i].hex(), want_r[i].hex()) for i in bad_r[:4]]


# ---- h, l ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.ALL)
def test_h_the_kernel_equals_the_statement(name):
    args, frames, rate = cases.sequence(name)
    a, b = ref.RefByteTracker(args, rate), dt.DeviceByteTracker(args, rate, device="cuda")
    whole = torch.full((dt.STATE_BYTES + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    b._state = whole[GUARD:GUARD + dt.STATE_BYTES]
    b.reset()
    for f, frame in enumerate(frames):
        oa = a.update(cases.tracks_in(frame), cases.SIZE, cases.SIZE)
        ob = b.update(cases.tracks_in(frame), cases.SIZE, cases.SIZE)
        cases.assert_same_frame(a, b, oa, ob, b.state_dump(), (name, f))
    host = whole.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + dt.STATE_BYTES:] == 0xA5).all()


BATCH, SHIFTS, KINDS = 65, 7, ("crossing", "absent", "alternate")


@pytest.fixture(scope="module")
def lone_runs():
    """per (kind, shift): after every frame what a lone DeviceByteTracker.update returned and kept"""
    return {(kind, shift): cases.lone_run(cases.shifted(kind, shift)) for kind in KINDS for shift in range(SHIFTS)}


def _run_batch():
    """65 trackers, tracker t on kind t % 3 shifted by t % 7 frames, stepped together: two launches per tick.  Returns the record
    bytes of every tick, the trackers, their per-tick results and the guarded buffers."""
    return cases.run_batch([cases.shifted(KINDS[t % 3], t % SHIFTS) for t in range(BATCH)], GUARD)


@pytest.fixture(scope="module")
def batch():
    return _run_batch()


def test_h_sixty_five_trackers_in_two_launches_each_equal_their_lone_run(batch, lone_runs):
    raw, trackers, logs, states, records = batch
    stride = dt.STATE_BYTES + GUARD
    for t in range(BATCH):
        log, final = lone_runs[KINDS[t % 3], t % SHIFTS]
        assert logs[t] == log, t
        at = GUARD + t * stride
        assert states[at:at + dt.STATE_BYTES].tobytes() == final, t
        assert (states[at - GUARD:at] == 0xA5).all() and (states[at + dt.STATE_BYTES:at + stride] == 0xA5).all(), t
    assert (records[:GUARD] == 0xA5).all() and (records[GUARD + BATCH * dt.RECORD_BYTES:] == 0xA5).all()
    assert any(len(entry[0]) == 2 for entry in logs[0]) and max(len(log) for log in logs) > 48


def test_l_the_batch_is_deterministic(batch):
    again = _run_batch()
    assert again[0] == batch[0]
    assert again[3].tobytes() == batch[3].tobytes()


# ---- i ---------------------------------------------------------------------------------------------------------------------------
def test_i_detector_rows_are_read_where_they_lie():
    cases.rows_in_place(lambda args: dt.DeviceByteTracker(args, 30.0, device="cuda"), lambda a: torch.from_numpy(a).cuda(),
                        lambda jobs: dt.parse_records(dt.update_calls(jobs, torch.device("cuda")).cpu().numpy()))


# ---- j, k ------------------------------------------------------------------------------------------------------------------------
class ShapeStub:
    """scripted YuNet rows: a call is known by the shape of the frame the detector is shown and gets its next rows"""

    def __init__(self, scripts):
        self.rows = {sc.seen_shape(n): [scripts[n][s][1] for s in sc.detect_ticks(n)] for n in scripts}
        self.at = {shape: 0 for shape in self.rows}

    def _answer(self, views):
        dev = views[0].device
        rows = torch.zeros(len(views), 16, 15, dtype=torch.float32, device=dev)
        counts = []
        for b, v in enumerate(views):
            shape = tuple(v.shape[:2])
            mine = self.rows[shape][self.at[shape]]
            self.at[shape] += 1
            rows[b, :len(mine)] = torch.from_numpy(mine).to(dev)
            counts.append(len(mine))
        return rows, torch.tensor(counts, dtype=torch.int32, device=dev)

    def detect(self, frames_u8):
        return self._answer([frames_u8[0]])

    def detect_views(self, views):
        return self._answer(list(views))


def _call_args(name):
    from test_hip_server import DROP, EXCLUDE, GATE, RING, STRIDE
    c = sc.CALLS[name]
    return dict(stride=STRIDE, ring_frames=RING, drop_after=DROP, start_conf=sc.START_CONF, start_min_size=sc.START_MIN_SIZE, exclude_rect=EXCLUDE,
                channel_order=c["order"], detect_every=c["detect_every"], detect_size=c["detect_size"], **GATE)


def _kept(c):
    return dict(purged=sorted(c.purged), state=copy.deepcopy(c.state), clip_hist={t: list(v) for t, v in c.clip_hist.items()},
                running={t: list(v) for t, v in c.running_scores.items()},
                detections=None if c.detections is None else np.array(c.detections, copy=True),
                last_boxes={t: b.copy() for t, b in c.last_boxes.items()})


def _same_kept(a, b):
    same = all(a[k] == b[k] for k in ("purged", "state", "clip_hist", "running"))
    same = same and (a["detections"] is None) == (b["detections"] is None)
    same = same and (a["detections"] is None or (a["detections"].dtype == b["detections"].dtype and np.array_equal(a["detections"], b["detections"])))
    return same and set(a["last_boxes"]) == set(b["last_boxes"]) and all(np.array_equal(a["last_boxes"][t], b["last_boxes"][t]) for t in a["last_boxes"])


def _serve(scripts, mode):
    from test_hip_server import CLIP, SIZE, _net
    server = af_mi355x.CallServer(_net(), detector=ShapeStub(scripts), clip_size=CLIP, size=SIZE, tracker=mode)
    cids = {n: server.open(**_call_args(n)) for n in scripts}
    ticks = []
    for s in range(sc.TICKS):
        got = server.step({cids[n]: scripts[n][s][0] for n in scripts})
        ticks.append(({n: got[cids[n]] for n in scripts}, {n: _kept(server.call(cids[n])) for n in scripts}, dict(server.stats.last),
                      server.stats.last["track"]))
    return ticks, server


def test_j_the_server_with_device_trackers_equals_the_server_with_host_trackers():
    scripts = sc.scripts()
    host, _ = _serve(scripts, "host")
    device, server = _serve(scripts, "device")
    scored = 0
    for s, ((got_h, kept_h, stats_h, track_h), (got_d, kept_d, stats_d, track_d)) in enumerate(zip(host, device)):
        assert got_d == got_h, (s, got_d, got_h)                             # tids and scores, bit for bit
        for n in scripts:
            assert _same_kept(kept_d[n], kept_h[n]), (s, n)
        assert stats_d["wait"] <= stats_h["wait"] and track_d == 1 and track_h == 0, (s, stats_d, stats_h)
        assert all(stats_d[k] == stats_h[k] for k in ("detect", "quality", "warp", "replay")), (s, stats_d, stats_h)
        scored += sum(len(v) for v in got_h.values())
    assert scored >= 6 and any(len(k["A"]["last_boxes"]) for _, k, _, _ in host)
    assert all(server.call(c).tracker.frame_id > 0 for c in range(3))


def test_k_a_lone_call_with_a_device_tracker_equals_one_with_the_host_tracker():
    from test_hip_server import CLIP, SIZE, _net
    scripts = sc.scripts()
    for name in ("A", "B"):                                                  # alternate empty frames; the scale-back
        one = {name: scripts[name]}
        host = af_mi355x.RealtimeCall(_net(), detector=ShapeStub(one), clip_size=CLIP, size=SIZE, **_call_args(name))
        device = af_mi355x.RealtimeCall(_net(), detector=ShapeStub(one), clip_size=CLIP, size=SIZE, tracker="device", **_call_args(name))
        scored = 0
        for s, (frame, _) in enumerate(scripts[name]):
            want, got = host.step(frame), device.step(frame)
            assert got == want, (name, s, got, want)
            assert _same_kept(_kept(device), _kept(host)), (name, s)
            scored += len(want)
        assert scored >= 2 or name == "A", name                               # A's face is seen on every other frame only
        assert device.tracker.tracked_ids or device.tracker.lost_ids
