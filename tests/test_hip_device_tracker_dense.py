"""GPU: the device tracker (csrc/af_track.hip) on the dense, contested sequences of tests/bytetrack_cases.py (``DENSE``) - what
tests/test_device_tracker_dense_host.py pins for the host build of csrc/af_track_core.h, on the build whose lane-0 sections are fenced
by barriers and whose scratch lies in LDS: assignments that re-route at up to 24 x 24, more detections than tracks, a tracked face
dropped as the duplicate of a lost one, a removed face back on the call it leaves, costs that are exactly equal.

  lone     DeviceByteTracker.update, the state between 0xA5 guard bands, equals the statement by np.array_equal after every frame
  batched  65 trackers, tracker t on DENSE[t % 14] behind t % 5 empty frames, stepped together by update_calls (two launches per
           tick): every tracker's log and final state bytes equal its lone run; the guard bands around every state block and around
           the records are untouched; a second run gives the same record bytes
All comparisons are exact.
"""
import pytest
import torch

import bytetrack_cases as cases
import bytetrack_ref as ref
from af_mi355x import device_tracker as dt

pytestmark = pytest.mark.gpu
GUARD = 512
BATCH, SHIFTS = 65, 5


@pytest.mark.parametrize("name", cases.DENSE)
def test_the_kernel_equals_the_statement(name):
    args, frames, rate = cases.sequence(name)
    assert len(frames) <= 60
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


def _script(t):
    return cases.DENSE[t % len(cases.DENSE)], t % SHIFTS


@pytest.fixture(scope="module")
def lone_runs():
    """per (name, shift) of the batch: after every frame what a lone DeviceByteTracker.update returned and kept"""
    return {key: cases.lone_run(cases.shifted(*key)) for key in sorted({_script(t) for t in range(BATCH)})}


def _run_batch():
    return cases.run_batch([cases.shifted(*_script(t)) for t in range(BATCH)], GUARD)


@pytest.fixture(scope="module")
def batch():
    return _run_batch()


def test_sixty_five_trackers_in_two_launches_each_equal_their_lone_run(batch, lone_runs):
    raw, trackers, logs, states, records = batch
    stride = dt.STATE_BYTES + GUARD
    for t in range(BATCH):
        log, final = lone_runs[_script(t)]
        assert len(logs[t]) == len(log)
        for f, (got, want) in enumerate(zip(logs[t], log)):
            assert got == want, (t, _script(t), f)
        at = GUARD + t * stride
        assert states[at:at + dt.STATE_BYTES].tobytes() == final, (t, _script(t))
        assert (states[at - GUARD:at] == 0xA5).all() and (states[at + dt.STATE_BYTES:at + stride] == 0xA5).all(), t
    assert (records[:GUARD] == 0xA5).all() and (records[GUARD + BATCH * dt.RECORD_BYTES:] == 0xA5).all()
    assert len(raw) == 60 + SHIFTS - 1 and len(raw[0]) == BATCH * dt.RECORD_BYTES            # all 65 stepped together: two launches
    assert max(len(entry[0]) for log in logs for entry in log) >= 20                          # a packed crowd among them


def test_the_batch_is_deterministic(batch):
    again = _run_batch()
    assert again[0] == batch[0]
    assert again[3].tobytes() == batch[3].tobytes()
