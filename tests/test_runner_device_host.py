"""CPU: ``VideoRunner(tracker="device")`` and the chunk stage's host twin (``af_runner_track_chunk_host``, the source the device
launch runs: csrc/af_runner_core.h) - no GPU is needed.

  golden   the four golden runs of tests/golden/runner_video.json replayed through ``VideoRunner(tracker="device")`` with a scripted
           side whose ``track_chunk`` runs the host twin on the golden rows, laid out as a detector leaves them: every assertion of
           test_runner_host.test_the_loop_equals_the_reference_loop, at chunk sizes 1, 5 and 16 - and, chunk by chunk, the twin's
           record and state against the statement (tests/runner_chunk_ref.py: the loop's lines with ``RefByteTracker``)
  scripts  tests/runner_chunk_cases.py: the twin against the statement after every chunk, on scripts that reach the filter and
           start limits, the start and the budget in mid-chunk, the five-point cache, the id switch, the crop box's corners, 32
           faces, both refusals and two dense walks of overlapping faces; the guard bytes around the state and the record hold
  errors   what the constructor and a refusal raise
"""
import types

import numpy as np
import pytest

from af_mi355x import runner as R
from af_mi355x import runner_device as RD
import runner_chunk_cases as cases
import runner_chunk_ref as ref
from test_runner_host import RUNS, SIZE, ScriptedSide

GUARD = 64
MAX_ROWS = 40


def _guarded(n_bytes, fill):
    """(the whole buffer, the 8-byte aligned view of `n_bytes` in its middle); the bands around the view are `fill`"""
    whole = np.full(n_bytes // 8 + 2 * GUARD // 8, 0, dtype=np.float64).view(np.uint8)
    whole[:] = fill
    return whole, whole[GUARD:GUARD + n_bytes]


def _intact(whole, n_bytes, fill):
    return bool((whole[:GUARD] == fill).all() and (whole[GUARD + n_bytes:] == fill).all())


class TwinRun:
    """a run of the host twin with guard bands around its state and around every record, and the statement beside it"""

    def __init__(self, plan, ref_run):
        self.plan, self.ref = plan, ref_run
        self.whole, self.state = _guarded(RD.STATE_BYTES, 0xA5)
        self.state[:] = plan.reset()
        self.chunks = []

    def chunk(self, rows, ids, first_slot, seed=0):
        laid, counts = cases.laid_out(rows, MAX_ROWS, seed)
        n = RD.record_bytes(len(ids))
        whole, record = _guarded(n, 0x5A)
        RD.track_chunk_host(self.plan, self.state, laid, counts, first_slot, ids, record)
        assert _intact(whole, n, 0x5A) and _intact(self.whole, RD.STATE_BYTES, 0xA5)
        rec = RD.parse_record(record, len(ids))
        want = self.ref.chunk(rows, ids, first_slot)
        self.chunks.append(want)
        ref.compare(rec, RD.parse_state(self.state), want, self.ref, len(ids))
        return rec, record


# ---- golden ----------------------------------------------------------------------------------------------------------------------------

class TwinSide(ScriptedSide):
    """the scripted side of test_runner_host, with the chunk stage done by the host twin"""

    def open_tracker(self, plan):
        run = self.run
        args = types.SimpleNamespace(**dict(R.DEFAULTS, **{k: v for k, v in run["args"].items() if k != "mot20"}))
        self.twin = TwinRun(plan, ref.RefRun(args, run["frame_shape"], plan.detect_every, plan.budget_frames, R.sane_fps(run["fps"])))
        self.tracks = 0

    def track_chunk(self, frames, first_slot, frame_ids, full):
        self.put(frames, first_slot)
        rows = self.detect(first_slot, len(frames))
        assert [self.frame_at[first_slot + k] for k in range(len(frames))] == list(frame_ids)
        rec, _ = self.twin.chunk(rows, list(frame_ids), first_slot, seed=first_slot)
        self.tracks += 1
        fake = [types.SimpleNamespace(frame_idx=frame_ids[int(c["frame_pos"])], slot=int(c["slot"]), rect=tuple(int(v) for v in c["box"]))
                for c in rec["cands"][:int(rec["head"]["n_cands"])]]
        return rec, (self.quality(fake, full) if fake and not int(rec["head"]["overflow"]) else [])


def _replay(name, detect_batch):
    run = RUNS[name]
    h, w, _ = run["frame_shape"]
    frames = [np.zeros((h, w, 3), dtype=np.uint8) for _ in range(run["n_frames"])]
    index_of = {id(f): i for i, f in enumerate(frames)}
    args = {k: v for k, v in run["args"].items() if k != "mot20"}
    r = R.VideoRunner(None, detector=object(), size=SIZE, detect_batch=detect_batch, tracker="device", **args)
    sides = []
    r.side_type = lambda runner, shape, capacity: sides.append(TwinSide(runner, shape, capacity, run, index_of)) or sides[-1]
    out = r.run(frames if run["total_frames"] else iter(frames), fps=run["fps"], total_frames=run["total_frames"])
    return run, r, sides[0], out


@pytest.mark.parametrize("detect_batch", [1, 5, 16])
@pytest.mark.parametrize("name", sorted(RUNS))
def test_the_device_loop_equals_the_reference_loop(name, detect_batch):
    run, r, side, out = _replay(name, detect_batch)
    trace, want = r.trace, run["returned"]
    assert trace["processed"] == run["processed"]
    assert side.gate_at == len(run["gate"]) and side.group_at == len(run["scores"])
    assert [list(q) for q in trace["qstat"]] == run["qstat"]
    assert trace["flush_groups"] == run["flush_groups"]
    assert len(trace["clips"]) == len(run["clips"])
    for got, want_clip in zip(trace["clips"], run["clips"]):
        assert got["tid"] == want_clip["tid"] and [side.frame_at[s] for s in got["slots"]] == want_clip["frame_ids"]
        assert [[float(v) for v in rec[0]] for rec in got["records"]] == want_clip["boxes"]
        assert [[float(v) for v in rec[1].ravel()] for rec in got["records"]] == want_clip["lm5"]
        assert [[int(v) for v in rec[3]] for rec in got["records"]] == want_clip["big"]
        assert all(rec[2].shape == (68, 2) and not rec[2].any() for rec in got["records"])
    assert [[tid for tid, _ in g] for g in side.groups] == run["flush_groups"]
    assert {str(k): v for k, v in out["track_clip_scores"].items()} == run["track_clip_scores"]
    assert {str(k): v for k, v in out["per_person_scores"].items()} == want["per_person_scores"]
    assert {str(k): v for k, v in out["per_person_labels"].items()} == want["per_person_labels"]
    for key in ("frames_processed", "video_score", "pred_label", "num_tracks", "id_switch_rate_per_1k_frames"):
        assert out[key] == want[key], key
    assert set(want) <= set(out) and out["stats"]["chunks"] == len(r.chunks)
    assert set(run["detected"]) <= {i for ids in side.detects for i in ids}
    assert all(len(ids) <= detect_batch for ids in side.detects) and trace["slots_used"] <= side.capacity
    assert (side.full_asked > 0) == bool(run["qstat"]) and (len(run["qstat"]) < 50 or side.full_asked < len(side.detects))
    assert side.tracks == len(side.detects)                   # one chunk stage per detect


# ---- scripts ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [1, 5, 16])
@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_the_host_twin_equals_the_statement(case, size):
    twin = TwinRun(case.plan(), case.ref_run())
    last = {}

    def step(rows, ids, base):
        rec, raw = twin.chunk(rows, ids, base)
        last["rec"], last["raw"], last["ids"] = rec, raw, ids
        head = rec["head"]
        return any(int(f["flags"]) & RD.PROCESSED for f in rec["frames"][:len(ids)]), bool(head["stop"]) or bool(head["overflow"])
    cases.walk(case, size, step)
    case.reached(twin.chunks, twin.ref)
    if case.name in cases.REFUSING:                           # the record is untouched past the refusing frame
        rec, j = last["rec"], int(last["rec"]["head"]["overflow_frame"])
        frames = np.frombuffer(last["raw"].tobytes(), dtype=np.uint8)[RD.HEADER.itemsize:RD.CANDS_OFFSET].reshape(RD.MAX_FRAMES, -1)
        assert (frames[j + 1:] == 0x5A).all()
        cands = np.frombuffer(last["raw"].tobytes(), dtype=np.uint8)[RD.CANDS_OFFSET:].reshape(-1, RD.CAND.itemsize)
        assert (cands[int(rec["head"]["n_cands"]):] == 0x5A).all()
        err = RD.refusal(rec, last["ids"])
        assert isinstance(err, RuntimeError) and "frame %d" % last["ids"][j] in str(err) and "= 32" in str(err)


def test_a_refused_run_refuses_every_later_chunk():
    case = next(c for c in cases.CASES if c.name == "too_many_tracks")
    plan = case.plan()
    state = plan.reset()
    laid, counts = cases.laid_out(case.rows[:2], MAX_ROWS)
    first = RD.parse_record(RD.track_chunk_host(plan, state, laid, counts, 0, [0, 1]), 2)
    assert int(first["head"]["overflow"]) == ref.OVERFLOW_TRACKS
    again = RD.parse_record(RD.track_chunk_host(plan, state, laid[:1], counts[:1], 2, [2]), 1)
    assert int(again["head"]["overflow"]) == ref.OVERFLOW_TRACKS and int(again["head"]["n_cands"]) == 0
    blank = np.zeros(RD.STATE_BYTES // 8, dtype=np.float64).view(np.uint8)
    never = RD.parse_record(RD.track_chunk_host(plan, blank, laid[:1], counts[:1], 0, [0]), 1)
    assert "never reset" in str(RD.refusal(never, [0]))


def test_the_twin_checks_its_arguments():
    case = cases.CASES[0]
    plan, (laid, counts) = case.plan(), cases.laid_out(case.rows[:2], MAX_ROWS)
    state = plan.reset()
    with pytest.raises(ValueError):
        RD.track_chunk_host(plan, state, laid.astype(np.float64), counts, 0, [0, 1])
    with pytest.raises(ValueError):
        RD.track_chunk_host(plan, state, laid, counts, 0, list(range(65)))
    with pytest.raises(RuntimeError, match="15 or more"):
        RD.track_chunk_host(plan, state, np.ascontiguousarray(laid[:, :, :14]), counts, 0, [0, 1])
    with pytest.raises(RuntimeError, match="index -1"):
        RD.track_chunk_host(plan, state, laid, counts, 0, [0, -1])


# ---- errors ----------------------------------------------------------------------------------------------------------------------------

def test_construction_errors():
    with pytest.raises(ValueError, match="landmarks"):
        R.VideoRunner(None, detector=object(), tracker="device", landmarks=lambda frame, box: None)
    with pytest.raises(ValueError, match="detect_batch is 65"):
        R.VideoRunner(None, detector=object(), tracker="device", detect_batch=65)
    with pytest.raises(ValueError, match="tracker one of host, device"):
        R.VideoRunner(None, detector=object(), tracker="gpu")
    assert R.VideoRunner(None, detector=object()).tracker == "host"
    assert R.VideoRunner(None, detector=object(), tracker="device", detect_batch=64).tracker == "device"
    R.VideoRunner(None, detector=object(), tracker="host", detect_batch=65, landmarks=lambda frame, box: None)
