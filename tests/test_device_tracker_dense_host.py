"""CPU: the device tracker's statement (tests/bytetrack_ref.py) and host entry on the dense, contested sequences of
tests/bytetrack_cases.py (``DENSE``): eight random walks of 6 to 10 overlapping faces, three packed crowds of 22 to 24 and three
scripts built by hand (a tracked face dropped as the duplicate of a lost one, a removed face back on the call it leaves, two
detections of exactly equal cost).

  conditions  what the sequences make the statement do, counted by ``dense_stats`` on the statement alone: re-routed assignments,
              problems with more columns than rows and the reverse, re-found tracks, ids removed twice, second-association matches,
              20 x 20 problems - and that none of them comes near the caps of 32
  host entry  ``DeviceByteTracker(host=True)`` against the statement by ``assert_same_frame`` after every frame, between guard bytes
  tracker     the statement beside ``tracker.ByteTracker``: every discrete result equal on every frame; means, covariances and boxes
              within ``test_device_tracker_host.BOUND``
  solver      every cost matrix the statement solved on these sequences, solved again by ``tracker.linear_assignment`` (scipy on the
              extended matrix): the totals - matched costs plus ``thresh`` per row left alone - agree to 1e-12 (both are exact optima
              in fp64, of 64 terms or fewer), and where the pairs are the same set, the leftovers are too
"""
import numpy as np
import pytest

import bytetrack_cases as cases
import bytetrack_ref as ref
from af_mi355x import tracker
from test_device_tracker_host import BOUND, _guarded

COUNTED = ("non_greedy", "n_lt_m", "n_gt_m", "refound", "repeated", "second_frames", "tracked_dropped")


def test_the_dense_sequences_reach_what_they_were_made_for():
    stats = {name: cases.dense_stats(name) for name in cases.DENSE}
    for name, s in stats.items():
        print("%-12s %2d frames, %3d associations: %3d non-greedy, %3d n < m, %3d n > m, largest %2d x %2d; %3d re-found, %2d ids removed twice, "
              "%2d second-association frames, %d tracked dropped; tracked + lost <= %2d, rows <= %2d"
              % (name, s["frames"], len(s["problems"]), s["non_greedy"], s["n_lt_m"], s["n_gt_m"], *s["largest"], s["refound"], s["repeated"],
                 s["second_frames"], s["tracked_dropped"], s["held"], s["rows"]))
    for name, s in stats.items():                                         # the caps are 32: no sequence may end in a refusal
        assert s["held"] <= 28 and s["rows"] <= 30 and s["frames"] <= 60, (name, s["held"], s["rows"], s["frames"])
    walks = {k: sum(stats[name][k] for name in cases.WALKS) for k in COUNTED}
    crowds = {k: sum(stats[name][k] for name in cases.CROWDS) for k in COUNTED}
    print("walks ", walks)
    print("crowds", crowds)
    assert len(cases.WALKS) == 8 and all(stats[name]["frames"] == 60 for name in cases.WALKS)
    assert walks["non_greedy"] >= 60 and walks["n_lt_m"] >= 100 and walks["n_gt_m"] >= 100, walks
    assert walks["refound"] >= 150 and walks["repeated"] >= 8 and walks["second_frames"] >= 60, walks
    assert len(cases.CROWDS) == 3 and all(stats[name]["frames"] == 30 for name in cases.CROWDS)
    assert any(min(stats[name]["largest"]) >= 20 for name in cases.CROWDS) and crowds["non_greedy"] >= 20, crowds
    forms = {name: {form for form, _ in cases.sequence(name)[1]} - {"empty"} for name in cases.WALKS + cases.CROWDS}
    assert all(len(f) == 1 for f in forms.values())
    assert [forms["walk%d" % s] for s in range(8)] == [{"stracks"}, {"array"}] * 4
    assert {"stracks"} in [forms[name] for name in cases.CROWDS] and {"array"} in [forms[name] for name in cases.CROWDS]
    assert stats["usurper"]["tracked_dropped"] >= 1
    assert stats["back_at_once"]["repeated"] >= 1 and stats["back_at_once"]["refound"] >= 2
    assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(cases.walk(3)[1], cases.sequence("walk3")[1]))      # seeded


@pytest.mark.parametrize("name", cases.DENSE)
def test_the_host_entry_equals_the_statement(name):
    from af_mi355x.device_tracker import DeviceByteTracker
    args, frames, rate = cases.sequence(name)
    a, b = ref.RefByteTracker(args, rate), DeviceByteTracker(args, rate, host=True)
    intact = _guarded(b)
    for f, frame in enumerate(frames):
        oa = a.update(cases.tracks_in(frame), cases.SIZE, cases.SIZE)
        ob = b.update(cases.tracks_in(frame), cases.SIZE, cases.SIZE)
        cases.assert_same_frame(a, b, oa, ob, b.state_dump(), (name, f))
        assert intact(), (name, f)


@pytest.mark.parametrize("name", cases.DENSE)
def test_the_statement_equals_the_host_tracker(name):
    args, frames, rate = cases.sequence(name)
    a, b = ref.RefByteTracker(args, rate), tracker.ByteTracker(args, rate)
    worst = {"mean": 0.0, "covariance": 0.0, "tlbr": 0.0}
    for f, frame in enumerate(frames):
        oa = a.update(cases.tracks_in(frame), cases.SIZE, cases.SIZE)
        ob = b.update(cases.tracks_in(frame), cases.SIZE, cases.SIZE)
        assert [t.track_id for t in oa] == [t.track_id for t in ob], (name, f)
        assert [t.state for t in oa] == [t.state for t in ob] and [t.is_activated for t in oa] == [t.is_activated for t in ob], (name, f)
        assert [t.score for t in oa] == [t.score for t in ob], (name, f)
        assert a.frame_id == b.frame_id, (name, f)
        assert [t.track_id for t in a.tracked_stracks] == [t.track_id for t in b.tracked_stracks], (name, f)
        assert [t.track_id for t in a.lost_stracks] == [t.track_id for t in b.lost_stracks], (name, f)
        assert a.removed_ids == [t.track_id for t in b.removed_stracks], (name, f)
        for x, y in zip(a.tracked_stracks + a.lost_stracks, b.tracked_stracks + b.lost_stracks):
            assert (x.state, x.is_activated, x.frame_id, x.start_frame, x.tracklet_len) == \
                (y.state, y.is_activated, y.frame_id, y.start_frame, y.tracklet_len), (name, f, x.track_id)
            worst["mean"] = max(worst["mean"], float(np.abs(np.asarray(x.mean) - y.mean).max()))
            worst["covariance"] = max(worst["covariance"], float(np.abs(np.asarray(x.covariance) - y.covariance).max()))
            worst["tlbr"] = max(worst["tlbr"], float(np.abs(x.tlbr - y.tlbr).max()))
    print("%-12s worst |mean| %.3g |covariance| %.3g |tlbr| %.3g" % (name, worst["mean"], worst["covariance"], worst["tlbr"]))
    for key, bound in BOUND.items():
        assert worst[key] <= bound, (name, key, worst[key])


def _total(cost, matches, n, thresh):
    """the matched costs plus ``thresh`` for every row left alone"""
    return sum(float(cost[i][j]) for i, j in matches) + thresh * (n - len(matches))


def test_the_solver_reaches_scipys_optimum_on_every_harvested_matrix():
    solved = same = biggest = 0
    worst = 0.0
    for name in cases.DENSE:
        for k, (cost, n, m, thresh) in enumerate(cases.dense_stats(name)["problems"]):
            got_m, got_a, got_b = ref.linear_assignment(cost, n, m, thresh)
            want_m, want_a, want_b = tracker.linear_assignment(np.asarray(cost, dtype=np.float64).reshape(n, m), thresh)
            want_m = [tuple(int(v) for v in p) for p in want_m]
            assert len({i for i, _ in got_m}) == len(got_m) == len({j for _, j in got_m}), (name, k)
            assert all(cost[i][j] <= thresh for i, j in got_m), (name, k)
            assert sorted(got_a) == sorted(set(range(n)) - {i for i, _ in got_m}) and sorted(got_b) == sorted(set(range(m)) - {j for _, j in got_m})
            d = abs(_total(cost, got_m, n, thresh) - _total(cost, want_m, n, thresh))
            worst = max(worst, d)
            assert d <= 1e-12, (name, k, n, m, thresh, d)
            if sorted(got_m) == sorted(want_m):
                assert got_m == want_m and got_a == [int(v) for v in want_a] and got_b == [int(v) for v in want_b], (name, k)
                same += 1
            solved += 1
            biggest = max(biggest, min(n, m))
    print("%d matrices, %d with scipy's own pairs, the largest %d wide; worst |total - scipy's| %.3g" % (solved, same, biggest, worst))
    assert solved >= 500 and biggest >= 20 and same >= solved // 2
