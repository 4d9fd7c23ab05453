"""CPU: ``af_mi355x.runner`` - the dataset evaluator's per-video loop - against the reference's own loop and by hand.

  golden    tests/golden/runner_video.json holds what ``VideoRunner.run`` of altfreezing/TEST2.py did on four scripted videos
            (tools/gen_runner_golden.py).  ``runner.VideoRunner`` replays them with its device side scripted - YuNet's rows, the
            gate's two Laplacian figures per crop and the scores come from the file - at three chunk sizes: the processed frames,
            every clip (tid, frame ids, boxes, five points, crop boxes), the flush groups, ``_qstat``, the per-person scores and
            labels, ``video_score`` and the id-switch rate are EQUAL, floats included
  pooling   the functions behind the loop on lists worked by hand: empty, single, tied
  planning  the window plan, the fps check, the detection rhythm
  store     the ``ValueError`` for a frame store that does not fit
  ref       tests/runner_ref.py's two hand-worked crops
"""
import types

import numpy as np
import pytest

from af_mi355x import runner as R
from conftest import load_json
import runner_ref

GOLDEN = load_json("runner_video.json")
RUNS = GOLDEN["runs"]
SIZE = GOLDEN["imsize"]


class ScriptedSide:
    """the runner's device side from the golden file: no pixels are read"""

    def __init__(self, runner, shape, capacity, run, index_of):
        self.run, self.capacity, self.index_of = run, capacity, index_of
        self.frame_at, self.gate_at, self.group_at = {}, 0, 0
        self.detects, self.groups, self.full_asked = [], [], 0

    def put(self, frames, first_slot):
        assert first_slot >= 0 and first_slot + len(frames) <= self.capacity
        for k, f in enumerate(frames):
            self.frame_at[first_slot + k] = self.index_of[id(f)]

    def view(self, slot):
        raise AssertionError("no landmarks hook in this replay")

    def detect(self, first_slot, n):
        ids = [self.frame_at[first_slot + k] for k in range(n)]
        assert ids == sorted(ids)
        self.detects.append(ids)
        return [np.asarray(self.run["rows"][i], dtype=np.float32).reshape(-1, 15) for i in ids]

    def quality(self, cands, full):
        out = []
        self.full_asked += bool(full)
        for c in cands:
            rec = self.run["gate"][self.gate_at]
            self.gate_at += 1
            x0, y0, x1, y1 = c.rect
            assert rec["frame"] == c.frame_idx == self.frame_at[c.slot] and rec["shape"] == [y1 - y0, x1 - x0]
            # the full-size figure only where the reference took it: a crop it did not measure has none to give, and the loop
            # must not want it (a None in _qstat fails the comparison)
            out.append((float(min(rec["shape"])), rec["lap"], rec["full"] if full else None))
        return out

    def score(self, group):
        scores = self.run["scores"][self.group_at]
        self.group_at += 1
        assert len(scores) == len(group)
        self.groups.append(group)
        return np.asarray(scores, dtype=np.float32)


def _replay(name, detect_batch):
    run = RUNS[name]
    h, w, _ = run["frame_shape"]
    frames = [np.zeros((h, w, 3), dtype=np.uint8) for _ in range(run["n_frames"])]
    index_of = {id(f): i for i, f in enumerate(frames)}
    args = {k: v for k, v in run["args"].items() if k != "mot20"}
    r = R.VideoRunner(None, detector=object(), size=SIZE, detect_batch=detect_batch, **args)
    sides = []
    r.side_type = lambda runner, shape, capacity: sides.append(ScriptedSide(runner, shape, capacity, run, index_of)) or sides[-1]
    out = r.run(frames if run["total_frames"] else iter(frames), fps=run["fps"], total_frames=run["total_frames"])
    return run, r, sides[0], out


@pytest.mark.parametrize("detect_batch", [1, 5, 16])
@pytest.mark.parametrize("name", sorted(RUNS))
def test_the_loop_equals_the_reference_loop(name, detect_batch):
    run, r, side, out = _replay(name, detect_batch)
    trace, want = r.trace, run["returned"]
    assert trace["processed"] == run["processed"]
    assert side.gate_at == len(run["gate"]) and side.group_at == len(run["scores"])
    assert [list(q) for q in trace["qstat"]] == run["qstat"]
    assert trace["flush_groups"] == run["flush_groups"]
    assert len(trace["clips"]) == len(run["clips"])
    for got, ref in zip(trace["clips"], run["clips"]):
        assert got["tid"] == ref["tid"] and [side.frame_at[s] for s in got["slots"]] == ref["frame_ids"]
        assert [[float(v) for v in rec[0]] for rec in got["records"]] == ref["boxes"]
        assert [[float(v) for v in rec[1].ravel()] for rec in got["records"]] == ref["lm5"]
        assert [[int(v) for v in rec[3]] for rec in got["records"]] == ref["big"]
        assert all(rec[2].shape == (68, 2) and not rec[2].any() for rec in got["records"])
    assert [[tid for tid, _ in g] for g in side.groups] == run["flush_groups"]
    assert {str(k): v for k, v in out["track_clip_scores"].items()} == run["track_clip_scores"]
    assert {str(k): v for k, v in out["per_person_scores"].items()} == want["per_person_scores"]
    assert {str(k): v for k, v in out["per_person_labels"].items()} == want["per_person_labels"]
    for key in ("frames_processed", "video_score", "pred_label", "num_tracks", "id_switch_rate_per_1k_frames"):
        assert out[key] == want[key], key
    assert set(want) <= set(out) and out["stats"]["chunks"] == len(r.chunks)
    # a frame the reference asked YuNet about was detected here too (here every kept frame is), and nothing unkept was uploaded
    assert set(run["detected"]) <= {i for ids in side.detects for i in ids}
    assert all(len(ids) <= detect_batch for ids in side.detects) and trace["slots_used"] <= side.capacity
    # the full-size measurement is asked for only while _qstat is short at a chunk's start
    assert (side.full_asked > 0) == bool(run["qstat"]) and (len(run["qstat"]) < 50 or side.full_asked < len(side.detects))


def test_what_the_golden_runs_exercise():
    a, b, c, d = (RUNS[k] for k in "abcd")
    assert len(a["track_clip_scores"]) >= 2 and len(a["clips"]) >= 4 and len(a["gate"]) > 50 == len(a["qstat"])
    assert b["args"]["smart_start"] and min(b["processed"]) > 36 and max(b["processed"]) >= 112 and len(b["processed"]) < 32
    assert any(g["weight"] == 0.0 for g in c["gate"]) and c["low_quality"] and c["returned"]["pred_label"] == 1
    assert c["returned"]["video_score"] <= c["args"]["optimal_threshold"] and c["returned"]["id_switch_rate_per_1k_frames"] > 0
    assert d["total_frames"] == 0 and not d["clips"] and d["returned"]["video_score"] == 0.0 and len(d["processed"]) == d["args"]["max_frame"]


@pytest.mark.parametrize("method", R.POOL_METHODS)
def test_every_pool_method_on_the_golden_scores(method):
    a = RUNS["a"]
    args = types.SimpleNamespace(**dict(a["args"], pool_method=method))
    got = R.video_verdict({int(k): v for k, v in a["track_clip_scores"].items()}, [tuple(q) for q in a["qstat"]], args)
    want = a["pool_methods"][method]
    assert {str(k): v for k, v in got["per_person_scores"].items()} == want["per_person_scores"]
    assert {str(k): v for k, v in got["per_person_labels"].items()} == want["per_person_labels"]
    assert got["video_score"] == want["video_score"] and got["pred_label"] == want["pred_label"] and got["low_quality"] == a["low_quality"]


def test_the_qa_rule_flips_the_label_of_a_low_quality_video():
    c = RUNS["c"]
    args = types.SimpleNamespace(**c["args"])
    scores = {int(k): v for k, v in c["track_clip_scores"].items()}
    low = R.video_verdict(scores, [tuple(q) for q in c["qstat"]], args)
    assert low["low_quality"] and not any(low["per_person_labels_std"].values()) and any(low["per_person_labels_qa"].values())
    assert low["pred_label"] == 1
    fine = R.video_verdict(scores, [(300, 50.0)] * 3, args)
    assert not fine["low_quality"] and fine["pred_label"] == 0 and fine["video_score"] == low["video_score"]
    assert R.video_verdict(scores, [], args)["low_quality"] is False                      # no record: not low


# ---- pooling, by hand ----------------------------------------------------------------------------------------------------------------

FIVE = [0.4, 0.1, 0.9, 0.2, 0.3]                          # sorted: 0.1 0.2 0.3 0.4 0.9


def test_pool_track_by_hand():
    ap = pytest.approx
    assert R.pool_track(FIVE, "mean") == ap(0.38) and R.pool_track(FIVE, "median") == 0.3
    assert R.pool_track(FIVE, "topk", topk_ratio=0.2) == 0.9                               # ceil(0.2 * 5) = 1
    assert R.pool_track(FIVE, "topk", topk_ratio=0.3) == ap(0.65)                          # ceil(1.5) = 2: mean(0.4, 0.9)
    assert R.pool_track(FIVE, "topk_median", topk_ratio=0.5) == 0.4                        # 3 of them: 0.3 0.4 0.9
    assert R.pool_track(FIVE, "percentile", percentile_p=80.0) == ap(0.5)                  # position 3.2: 0.4 + 0.2 * 0.5
    assert R.pool_track(FIVE, "percentile", percentile_p=250.0) == 0.9                     # clipped to 100
    assert R.pool_track(FIVE, "trimmed_mean", trim_ratio=0.2) == ap(0.3)                   # a = 1: mean(0.2, 0.3, 0.4)
    assert R.pool_track(FIVE, "trimmed_mean", trim_ratio=0.9) == ap(0.3)                   # clipped to 0.49: a = 2, b = 3
    assert R.pool_track(FIVE, "logit_median") == ap(0.3)                                   # the logit is monotone
    assert R.pool_track(FIVE, "adaptive") == ap(0.3)                                       # q75 - q25 = 0.2: the logit median
    tight = [0.80, 0.82, 0.84, 0.86, 0.88]
    assert R.pool_track(tight, "adaptive", percentile_p=80.0) == ap(0.864)                 # 0.04: the percentile
    assert R.pool_track(FIVE, "no such method") == 0.3                                     # as written: the median
    assert R.pool_track([0.0, 1.0], "logit_median") == ap(0.5)                             # clipped to 1e-6 .. 1 - 1e-6


@pytest.mark.parametrize("method", R.POOL_METHODS)
def test_pool_track_empty_single_tied(method):
    assert R.pool_track([], method) == 0.0
    assert R.pool_track([0.7], method) == pytest.approx(0.7, abs=1e-12)
    assert R.pool_track([0.25] * 4, method) == pytest.approx(0.25, abs=1e-12)


def test_score_with_stability_by_hand():
    assert R.score_with_stability([], 0.5) == 0.0
    # q85 at position 3.4: 0.4 + 0.4 * 0.5 = 0.6; q25 = 0.2; spread 0.4 > 0.25 and the median 0.3 < 0.85
    assert R.score_with_stability(FIVE, 0.3) == pytest.approx(0.3 * 0.85 ** (0.4 / 0.25))
    assert R.score_with_stability([0.2, 0.9, 0.9, 0.95, 0.99], 0.9) == 0.9                 # spread, but the median is high
    assert R.score_with_stability([0.5, 0.5, 0.5], 0.5) == 0.5 and R.score_with_stability([0.4], 0.4) == 0.4
    raw, pen = R.person_scores({1: FIVE, 2: [0.5], 3: []}, min_clips=1)
    assert raw == {1: 0.3, 2: 0.5}                                                         # no clip, under min_clips: no entry
    assert pen[1] == pytest.approx(0.3 * 0.85 ** 1.6) and pen[2] == 0.5
    assert R.person_scores({1: FIVE, 2: [0.5]}, min_clips=2)[0] == {1: 0.3}
    assert R.person_scores({1: FIVE}, disable_penalty=True)[1] == {1: 0.3}


def test_quality_rule_quantiles_and_labels_by_hand():
    assert R.low_quality_rule([]) == (False, None, None)
    assert R.low_quality_rule([(100, 30.0), (300, 10.0), (250, 20.0)]) == (False, 250.0, 20.0)
    assert R.low_quality_rule([(100, 30.0), (200, 40.0)]) == (True, 150.0, 35.0)           # the side
    assert R.low_quality_rule([(300, 10.0), (300, 12.0)])[0] is True                       # the Laplacian
    q = R.track_quantiles({1: FIVE, 2: []})
    assert set(q) == {1} and q[1]["q50"] == 0.3 and q[1]["q75"] == pytest.approx(0.4) and q[1]["q90"] == pytest.approx(0.7)
    per_person = {1: 0.3, 2: 0.45}
    quants = {1: {"q75": 0.4, "q90": 0.7}, 2: {"q75": 0.2, "q90": 0.5}}
    assert R.person_labels(per_person, quants, False) == ({1: 0, 2: 1}, {1: 0, 2: 0}, {1: 0, 2: 1})
    assert R.person_labels(per_person, quants, True) == ({1: 0, 2: 1}, {1: 1, 2: 0}, {1: 1, 2: 1})
    assert R.person_labels({1: 0.4}, {}, True) == ({1: 0}, {1: 0}, {1: 0})                 # > threshold, not >=; no quantiles: no hit
    empty = R.video_verdict({}, [], types.SimpleNamespace(**R.DEFAULTS))
    assert empty["video_score"] == 0.0 and empty["pred_label"] == 0 and empty["num_tracks"] == 0


# ---- planning ------------------------------------------------------------------------------------------------------------------------

def test_window_plan_by_hand():
    p = R.WindowPlan(120, 8, 2, 32, 30.0)                 # 57 starts, 32 // 8 = 4 windows: linspace(0, 56, 4) -> 0 18 37 56
    assert p.starts == [0, 36, 74, 112] and p.ranges == [(0, 7), (36, 43), (74, 81), (112, 119)] and p.budget_frames == 32
    assert [p.window_id(i) for i in (0, 7, 8, 36, 81, 119, 120)] == [0, 0, -1, 1, 2, 3, -1]
    assert p.keep(7) and not p.keep(8) and not p.keep(120)
    p = R.WindowPlan(20, 8, 0, 400, 30.0)                 # stride 0: half a clip; the ranges overlap, the first one wins
    assert p.starts == [0, 4, 8, 12] and p.budget_frames == 32 and [p.window_id(i) for i in (3, 7, 8, 11, 12, 19)] == [0, 0, 1, 1, 2, 3]
    p = R.WindowPlan(5, 8, 5, 400, 30.0)                  # shorter than a clip: one window, cut to the video
    assert p.ranges == [(0, 4)] and p.budget_frames == 5
    p = R.WindowPlan(0, 8, 5, 0, 25.0)                    # no frame count: everything kept, no window; the budget is 20 s
    assert p.ranges is None and p.keep(10 ** 6) and p.window_id(3) == -1 and p.budget_frames == 500
    assert R.WindowPlan(0, 8, 5, 40, 25.0).budget_frames == 40


def test_fps_check_and_detection_rhythm():
    assert [R.sane_fps(v) for v in (None, 0, 4.9, 5, 29.97, 240, 241)] == [30.0, 30.0, 30.0, 5.0, 29.97, 240.0, 30.0]
    assert R.detect_rhythm(3, 30.0) == 3 and R.detect_rhythm(0, 30.0) == 4 and R.detect_rhythm(0, 240.0) == 8 and R.detect_rhythm(0, 5.0) == 1


def test_detection_filters_by_hand():
    rows = np.zeros((4, 15), dtype=np.float32)
    rows[:, :5] = [[10, 10, 90, 70, 0.9], [10, 10, 79, 79, 0.9], [10, 10, 100, 39, 0.9], [10, 80, 90, 70, 0.9]]
    kept = R.filter_detections(rows, 120, 80, 4000, 0.10)        # the second is short, the third small, the fourth's centre at 115 >= 108
    assert kept.dtype == np.float32 and kept.tolist() == rows[:1].tolist()
    assert len(R.filter_detections(rows, 120, 0, 0, 0)) == 4
    assert R.faces_valid(rows, 0.6, 20) and not R.faces_valid(rows, 0.95, 20) and not R.faces_valid(rows[:0], 0.6, 20) and not R.faces_valid(None, 0, 0)


# ---- the frame store and the arguments ----------------------------------------------------------------------------------------------

def test_a_frame_store_that_does_not_fit_names_the_bytes():
    frames = [np.zeros((120, 160, 3), dtype=np.uint8) for _ in range(40)]
    r = R.VideoRunner(None, detector=object(), clip_size=8, detect_batch=4, frame_bytes=1 << 20)
    need = (40 + 2 * 4) * 120 * 160 * 3 + 16                  # starts 0 5 .. 30: 7 ranges of 8 = 56 > the 40 frames -> 40 + 8 slots
    with pytest.raises(ValueError, match="needs %d bytes" % need):
        r.run(frames)
    with pytest.raises(ValueError, match="needs %d bytes" % ((400 + 8) * 120 * 160 * 3 + 16)):
        r.run(iter(frames))                                   # no length, no frame count: the budget is max_frame
    assert r.frame_store_bytes((120, 160, 3), 56, 40) == need
    assert R.VideoRunner(None, detector=object()).run([]) is None


def test_arguments():
    r = R.VideoRunner(None, detector=object())
    assert (r.args.track_thresh, r.args.track_buffer, r.args.match_thresh) == (0.6, 2000, 0.6)
    assert (r.args.crop_scale, r.args.detect_every, r.args.stride, r.args.batch_clips, r.args.optimal_threshold) == (1.0, 3, 5, 8, 0.4)
    assert (r.detect_batch, r.size, r.max_batch, r.channel_order, r.landmarks) == (16, 224, 16, "bgr", None)
    R.VideoRunner(None, detector=object(), cfg_path="i3d_ori.yaml", detector_res=320, amp=False)      # accepted, not read
    with pytest.raises(TypeError, match="drop_after"):
        R.VideoRunner(None, detector=object(), drop_after=90)
    with pytest.raises(ValueError):
        R.VideoRunner(None)
    with pytest.raises(ValueError):
        R.VideoRunner(None, detector=object(), pool_method="mode")
    import af_mi355x
    assert af_mi355x.VideoRunner is R.VideoRunner


# ---- tests/runner_ref.py ---------------------------------------------------------------------------------------------------------------

def test_the_full_size_laplacian_reference_by_hand():
    for crop, n_px, s1, s2 in runner_ref.HAND_WORKED:
        assert runner_ref.full_sums(crop)[:3] == (n_px, s1, s2) and runner_ref.full_sums(crop, "bgr")[:3] == (n_px, s1, s2)
    assert runner_ref.full_variance(runner_ref.HAND_WORKED[0][0]) == 5424.0
    assert runner_ref.full_variance(runner_ref.HAND_WORKED[1][0]) == (9 * 306 - 4) / 81
    assert runner_ref.min_side_and_full_lap(runner_ref.HAND_WORKED[0][0]) == (1.0, 5424.0)
    assert runner_ref.full_sums(np.full((1, 1, 3), 7, np.uint8))[:3] == (1, 0, 0)
