"""CPU: the live candidate stage's host entry (af_live_update_host, the launch's own source compiled for the CPU) against its
statement - live.track_candidates behind bytetrack_ref.RefByteTracker, with the purge list (tests/live_cands_ref.py).

Every script - the reference's ByteTrack recording and the scripts and dense sequences of tests/bytetrack_cases.py, their list frames
as YuNet rows with five points each, and the scripts of live_cands_ref.py that reach the exclusion edges, the 0.4 limit of the pick, equal IoUs, the
cache rule's branches, a purge and a return, frames without detection, the scale-back, the clamp, an empty crop, 32 tracks, a
reused slot and a frame of more than 32 rows - is replayed frame by frame: the candidate record equals the statement's field for
field, ``candidates_of`` equals ``track_candidates``' tuple with its types, the cache holds the statement's points for every track
the tracker holds, the tracker's state equals the statement's tracker, and the guard bytes around the state and both records are
untouched.  No tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bytetrack_cases as cases
import live_cands_ref as L
from af_mi355x import _lib
from af_mi355x import device_tracker as dt

GUARD = 256


def _guarded(size):
    whole = np.zeros((size + 2 * GUARD) // 8, dtype=np.float64).view(np.uint8)
    whole[:] = 0xA5
    return whole, whole[GUARD:GUARD + size]


def _intact(blocks):
    return all((w[:GUARD] == 0xA5).all() and (w[GUARD + len(v):] == 0xA5).all() for w, v in blocks)


def _replay(name):
    """the script on a host tracker between guard bytes; yields per frame (frame, statement, tracker, online, record)"""
    args, frames = L.script(name)
    want = L.RefLive(args)
    tr = dt.DeviceByteTracker(args, 30.0, host=True, candidates=True)
    blocks = [_guarded(dt.LIVE_STATE_BYTES), _guarded(dt.RECORD_BYTES), _guarded(dt.LIVE_RECORD_BYTES)]
    tr._state = blocks[0][1]
    tr.reset()
    for f, fr in enumerate(frames):
        keep = []
        job = L.job_of(tr, fr, f % 7, torch.from_numpy, keep)
        dt.update_live_host(job, blocks[1][1], blocks[2][1])
        assert _intact(blocks), (name, f)
        online = tr.absorb(blocks[1][1])
        rec = dt.parse_live_records(blocks[2][1])[0]
        assert int(rec["slot"]) == f % 7
        yield f, fr, want, tr, online, rec


@pytest.mark.parametrize("name", L.ALL)
def test_the_host_entry_equals_track_candidates(name):
    cands = refreshed = most = 0
    slots = {}
    for f, fr, want, tr, online, rec in _replay(name):
        ref_online, found, before = want.step(fr)
        cases.assert_same_frame(want.tracker, tr, ref_online, online, tr.state_dump(), (name, f))
        L.assert_record(rec, L.expected(fr, ref_online, found, before, want.state), (name, f))
        L.assert_found(dt.candidates_of(rec), found, (name, f))
        held = set(tr.tracked_ids) | set(tr.lost_ids)
        cache = tr.cache_dump()
        assert {t for t in cache if t in held} == {t for t in want.state.last_lm if t in held}, (name, f)
        for tid in held & set(cache):
            assert np.array_equal(cache[tid], np.asarray(want.state.last_lm[tid]["lm5"], dtype=np.float32)), (name, f, tid)
        cands += len(found[0])
        most = max(most, int(rec["n_online"]))
        refreshed += sum(bool(int(e["flags"]) & _lib.AF_LIVE_REFRESHED) for e in rec["online"])
        st = np.frombuffer(tr._state.tobytes(), dtype=dt._LIVE_STATE, count=1)[0]
        for i, tid in enumerate(st["cache_tid"]):
            if tid:
                slots.setdefault(i, set()).add(int(tid))
    if L.has_points(name):                                                   # a sequence of arrays has no points
        assert cands > 0 and refreshed > 0, name
    if name == "reuse":
        assert any(len(tids) >= 2 for tids in slots.values())                # a tracker slot served two tracks, one after the other
    if name == "crowd":
        assert most == 32 and len(slots) >= 24                                # 32 returned tracks; those outside the self-view rectangle cached


def test_a_tracker_past_its_cap_refuses_both_records():
    args = cases._args()
    tr = dt.DeviceByteTracker(args, 30.0, host=True, candidates=True)
    rows = [L.face(20 + 40 * (i % 16), 20 + 50 * (i // 16), 30, 34, 0.95) for i in range(dt.MAX_DETS + 1)]
    fr = dict(L.DEFAULTS, rows=np.asarray(rows, dtype=np.float32), shape=cases.SIZE, idx=0)
    keep = []
    trec, rec = dt.update_live_host(L.job_of(tr, fr, 0, torch.from_numpy, keep))
    parsed = dt.parse_live_records(rec)[0]
    assert int(parsed["overflow"]) == _lib.AF_TRACK_OVERFLOW_DETS and int(parsed["n_online"]) == 0 and not parsed["online"].tobytes().strip(b"\0")
    with pytest.raises(RuntimeError, match="AF_TRACK_MAX_DETS"):
        dt.candidates_of(parsed)
    with pytest.raises(RuntimeError, match="AF_TRACK_MAX_DETS"):
        tr.absorb(trec)


def test_the_c_entries_refuse_what_they_cannot_run():
    args = cases._args()
    tr = dt.DeviceByteTracker(args, 30.0, host=True, candidates=True)
    trec, rec = np.zeros(dt.RECORD_BYTES // 8 + 1), np.zeros(dt.LIVE_RECORD_BYTES // 8 + 1)
    good = lambda **kw: tr.live_job(tr.empty_job(), **dict(dict(frame_idx=0, slot=0, shape=(96, 131), mesh_every=1, crop_scale=0.6, exclude_rect=L.EXCLUDE), **kw))
    host = lambda job, a=trec.ctypes.data, b=rec.ctypes.data: _lib.lib.af_live_update_host(C.byref(job) if job is not None else None, C.c_void_p(a), C.c_void_p(b))
    assert host(good()) == 0
    assert host(None) != 0 and host(good(), 0) != 0 and host(good(), b=0) != 0                 # null
    assert host(good(), trec.ctypes.data + 4) != 0 and host(good(), b=rec.ctypes.data + 4) != 0  # misaligned
    for bad in (dict(mesh_every=0), dict(frame_idx=-1), dict(slot=-1), dict(shape=(0, 131)), dict(shape=(96, 40000))):
        assert host(good(**bad)) != 0, bad
    job = good()
    job.n_purged = dt.MAX_TRACKS + 1
    assert host(job) != 0
    job = good()
    job.track.state = tr.state_ptr + 4
    assert host(job) != 0
    rows, count = torch.zeros(4, 15), torch.tensor([4], dtype=torch.int32)
    job = tr.live_rows_job(rows, count, 0.76, 20, (1.0, 1.0), frame_idx=0, slot=0, shape=(96, 131), mesh_every=1, crop_scale=0.6, exclude_rect=L.EXCLUDE)
    assert host(job) == 0
    job.rows_floats = 4 * 15 - 1                                              # one float short of the rows it names
    assert host(job) != 0 and b"floats" in _lib.lib.af_last_error()
    narrow = torch.zeros(4, 14)                                               # rows without the five points
    job = tr.live_job(tr.rows_job(narrow, count, 0.76, 20), rows_floats=56, frame_idx=0, slot=0, shape=(96, 131), mesh_every=1, crop_scale=0.6,
                      exclude_rect=L.EXCLUDE)
    assert host(job) != 0
    # a plain tracker block - af_bytetrack_reset's - is refused before anything behind it is read
    plain = dt.DeviceByteTracker(args, 30.0, host=True)
    job = good()
    job.track.state = plain.state_ptr
    assert host(job) == 0 and int(dt.parse_live_records(rec.view(np.uint8)[:dt.LIVE_RECORD_BYTES])[0]["overflow"]) == _lib.AF_TRACK_NOT_RESET
    with pytest.raises(ValueError, match="candidates=True"):
        plain.live_job(plain.empty_job(), frame_idx=0, slot=0, shape=(96, 131), mesh_every=1, crop_scale=0.6, exclude_rect=L.EXCLUDE)
    # the records launch: null, misaligned, too many jobs
    q = _lib.lib.af_face_quality_records_u8
    ref, jobs = (_lib.StoreRef * 1)(), (_lib.LiveQualityJob * 1)()
    assert q(None, 1, jobs, 1, C.c_void_p(rec.ctypes.data), None, 0, None) != 0
    assert q(ref, 1, None, 1, C.c_void_p(rec.ctypes.data), None, 0, None) != 0
    assert q(ref, 1, jobs, 1, None, None, 0, None) != 0
    assert q(ref, 1, jobs, 1, C.c_void_p(rec.ctypes.data + 4), None, 0, None) != 0
    assert q(ref, 1, jobs, _lib.QUALITY_MAX_RECTS + 1, C.c_void_p(rec.ctypes.data), None, 0, None) != 0
    assert q(ref, 0, jobs, 1, C.c_void_p(rec.ctypes.data), None, 0, None) != 0
    assert q(ref, 1, jobs, 1, C.c_void_p(rec.ctypes.data), None, 0, None) != 0                # a store without a base pointer
    assert q(ref, 1, jobs, 0, C.c_void_p(rec.ctypes.data), None, 0, None) == 0                # no job: nothing to do


def test_the_launches_a_tick_needs_follow_from_the_argument_space():
    assert 1 <= dt.LIVE_PER_LAUNCH <= _lib.AF_TRACK_MAX_CALLS
    assert C.sizeof(_lib.LiveCall) == C.sizeof(_lib.TrackCall) + 8 + 24 + 8 + 32 + 4 * dt.MAX_TRACKS == 280
    assert [dt.live_launches(n) for n in (0, 1, dt.LIVE_PER_LAUNCH, dt.LIVE_PER_LAUNCH + 1, 64, 65)] == \
        [0, 1, 1, 2, -(-64 // dt.LIVE_PER_LAUNCH), -(-64 // dt.LIVE_PER_LAUNCH) + 1]
