"""CPU: the numpy statement of the dualrun video path (tests/dualvideo_ref.py, what the HIP kernels equal bit for bit) against what the
reference's own functions returned on seeded tracks (tests/golden/dual_video.*, tools/gen_dual_video_golden.py), and the host helpers
of ``af_mi355x.dual_video`` against the reference's clip-buffer loop restated here."""
import numpy as np
import pytest

from conftest import load_json, load_npz
import dualvideo_ref as R
from af_mi355x import dual_video as DV


@pytest.fixture(scope="module")
def golden():
    doc, st = load_json("dual_video.json"), load_npz("dual_video.npz")
    tracks, clips, videos = [], [], []
    for vi, v in enumerate(doc["videos"]):
        by_key = {}
        for ti, t in enumerate(v["tracks"]):
            for s in t["clips"]:
                by_key.setdefault(t["key"], []).append(len(clips))
                clips.append((len(tracks), s, doc["T"]))
            tracks.append((st["v%d_t%d_lmk" % (vi, ti)], st["v%d_t%d_au" % (vi, ti)]))
        videos.append([(k, by_key[k]) for k in DV.person_key_order(by_key)])
    stats = {k: st["stats_" + k] for k in ("au_mean", "au_std", "lmk_mean", "lmk_std")}
    return doc, st, tracks, clips, videos, stats


def test_golden_shape(golden):
    doc, st, tracks, clips, videos, _ = golden
    assert doc["P"] == 478 and len(doc["videos"]) == 3 and max(len(v["tracks"]) for v in doc["videos"]) <= 4
    assert max(t["n"] for v in doc["videos"] for t in v["tracks"]) <= 40
    assert st["ref_A_clip"].shape == (len(clips), 8, 36) and st["ref_L_clip"].shape == (len(clips), 8, 132)
    assert [c for _, c, _ in clips] == [s for v in doc["videos"] for t in v["tracks"] for s in DV.clip_windows(t["n"])]


def test_the_key_set_and_the_least_point_count_agree_everywhere():
    """the key set reaches index 466, so 467 points are the least a frame can have (make_lmk_features.py:52 computes that; the
    comment beside it says 309): the kernel's table, the header's bound, the binding's and the module's are the statement's"""
    import os
    import re
    from conftest import ROOT
    from af_mi355x import _lib
    assert len(R.KEY_IDX) == 66 and R.KEY_IDX[-3:] == (R.NOSE, R.ML, R.MR) and len(set(R.KEY_IDX)) == 66
    assert max(R.KEY_IDX) + 1 == DV.MIN_POINTS == _lib.DUALV_MIN_POINTS == 467 and DV.MAX_CLIP_FRAMES == _lib.DUALV_MAX_T == 16
    hdr = open(os.path.join(ROOT, "include", "af_hip.h")).read()
    assert int(re.search(r"#define AF_DUALV_MIN_POINTS (\d+)", hdr).group(1)) == 467
    src = open(os.path.join(ROOT, "spatiotemporal-deepfake-detection-for-live-video-calls_amd", "csrc", "af_dual_video.hip")).read()
    table = re.search(r"DV_KEY_IDX\[DV_PTS\] = \{(.*?)\}", src, flags=re.S).group(1)
    assert tuple(int(v) for v in table.replace("\n", " ").split(",")) == R.KEY_IDX
    with pytest.raises(ValueError, match="467"):
        DV.DualTrack(np.zeros((8, 466, 2), np.float32), np.zeros((8, 12), np.float32), "0")


def test_au_features_equal_the_reference_bit_for_bit_where_order_free(golden):
    doc, st, tracks, clips, _, stats = golden
    A, _, nv = R.features(tracks, clips, T=8, mode="none")
    assert np.array_equal(A, st["ref_A_none"]) and np.array_equal(nv, st["ref_nvalid"])
    assert (nv < 8).sum() >= 3, "the golden holds dropped frames"
    A, _, _ = R.features(tracks, clips, T=8, mode="global", stats=stats)
    assert np.array_equal(A, st["ref_A_global"])
    assert (stats["au_std"] < 1e-6).any(), "a std under the floor"


def test_landmark_and_clip_mode_features_within_the_measured_tolerance(golden):
    doc, st, tracks, clips, _, _ = golden
    tol = 8 * doc["measured"]["tolerance_basis"]
    assert 0 < tol < 1e-4
    nose = doc["nose_cols"]
    keep = np.arange(len(clips)) != doc["held_clip"]
    _, L, _ = R.features(tracks, clips, T=8, mode="none")
    d_lmk = np.abs(L - st["ref_L_none"]).max()
    A, Lc, _ = R.features(tracks, clips, T=8, mode="clip")
    d_clip = max(np.abs(Lc - st["ref_L_clip"]).max(), np.abs(A[keep] - st["ref_A_clip"][keep]).max())
    print("max |statement - reference|: landmarks before z-score %.3g, clip mode %.3g, bound %.3g" % (d_lmk, d_clip, tol))
    assert d_lmk <= tol and d_clip <= tol
    assert (L[:, :, nose] == 0).all() and (Lc[:, :, nose] == 0).all()
    # every column the comparison covers is non-degenerate in the reference's own figures
    sd_l = st["ref_L_none"].std(axis=1, ddof=1)
    sd_l[:, nose] = 1
    assert (sd_l >= 1e-3).all() and (st["ref_A_none"][keep].std(axis=1, ddof=1) >= 1e-3).all()


def test_identical_rows_in_clip_mode_are_finite_and_bounded(golden):
    """8 identical AU rows: std 0 is clamped to 1e-6, so the z-score is the mean's own rounding error over 1e-6 (torch's comes out
    near 0.12 on such a clip) - no figure to compare, only a bound: |x - mean| <= |x| 2^-22 for a sequential fp32 sum of 8 equal
    terms divided by 8 (2x is exact; 3x .. 7x each round by at most half an ulp of a value below 8 |x|, 8x by half an ulp of one
    below 16 |x|: 7/8 |x| 2^-22 at worst after the exact division by 8)."""
    doc, st, tracks, clips, _, _ = golden
    t, s, n = clips[doc["held_clip"]]
    aus = tracks[t][1][s:s + n]
    assert (aus == aus[0]).all()
    A, _, _ = R.clip_features(tracks[t][0][s:s + n], aus, T=8, mode="clip")
    x = R.au_rows(aus)
    assert np.isfinite(A).all()
    assert (np.abs(A) <= np.abs(x) * 2.0 ** -22 / 1e-6).all()
    rows = np.full((8, 5), [0.1, 1 / 3, 0.7, 123.456, 1e-3], dtype=np.float32)
    z = R.nan_to_num(R.zscore_clip(rows))
    assert np.isfinite(z).all() and (np.abs(z) <= np.abs(rows) * 2.0 ** -22 / 1e-6).all()


# ---- clip windows: handle_clip_buffers (preprocessing/preprocessing_parallel.py:353-418) restated ------------------------------------

def buffers_loop(au_present, lmk_present, length=8, step=4):
    """the frames of every clip the reference's loop writes, as (first frame, AU source frames, landmark source frames)"""
    au_buf, land_buf, frames = [], [], []
    last = {"aus": None, "landmarks": None}                                    # :364
    written = []
    for f, (a, l) in enumerate(zip(au_present, lmk_present)):
        frames.append(f)                                                       # :367 clip_buffer gets the face crop
        if a:
            last["aus"] = f                                                    # :370-371
        if l:
            last["landmarks"] = f                                              # :372-373
        au_buf.append(last["aus"])                                             # :376
        land_buf.append(last["landmarks"])                                     # :377
        if len(frames) >= length:                                              # :382
            au_seq = [x for x in au_buf[:length] if x is not None]             # :383
            land_seq = [x for x in land_buf[:length] if x is not None]         # :384
            if len(au_seq) >= length and len(land_seq) >= length:              # :386
                written.append((frames[0], au_seq, land_seq))                  # :393-400
            frames, au_buf, land_buf = frames[step:], au_buf[step:], land_buf[step:]     # :416-418
    return written


@pytest.mark.parametrize("n", [7, 8, 11, 12, 13])
@pytest.mark.parametrize("lead", [0, 3, 9])
def test_clip_windows_and_fill_last_known_equal_the_buffer_loop(n, lead):
    present_a = np.ones(n, bool)
    present_l = np.ones(n, bool)
    present_a[:lead] = False
    present_l[:min(lead, 2)] = False                                           # the landmarks come earlier than the AUs
    if n > lead + 3:
        present_l[lead + 2] = False                                            # a hole mid-track
        present_a[n - 1] = False
    rows = np.arange(n, dtype=np.float32)[:, None]
    fa, first_a = DV.fill_last_known(rows, present_a)
    fl, first_l = DV.fill_last_known(rows, present_l)
    starts = DV.clip_windows(n, first_known=max(first_a, first_l))
    want = buffers_loop(present_a, present_l)
    assert starts == [w[0] for w in want]
    for s, au_src, land_src in want:
        assert fa[s:s + 8, 0].tolist() == au_src and fl[s:s + 8, 0].tolist() == land_src
    assert DV.clip_windows(n) == list(range(0, n - 7, 4))


def test_fill_last_known_without_any_row_and_person_key_order():
    rows, first = DV.fill_last_known(np.zeros((4, 2)), [False] * 4)
    assert first == 4 and DV.clip_windows(4, first_known=first) == []
    assert DV.person_key_order(["10", "2", "id_3", "track_1", "2b"]) == ["2", "10", "2b", "id_3", "track_1"]
    assert DV.person_key_order(["1", "1", "0"]) == ["0", "1"]


# ---- the reduction statement against track_reduce / agg_video / aggregate_video_predictions -----------------------------------------

def test_fusion_reduction_statement_equals_the_reference(golden):
    """Medians and the max pick elements: exact.  A mean is an fp32 sum in some order (torch's is not the statement's sequential
    one), and two orders of one sum differ by roundings of its partial sums, which are as large as its largest terms, not as its
    result: a track whose logits reach 2 and cancel to 0.03 comes out 3.9e-8 apart, 21 ulp of 0.03 and a third of an ulp of its terms.  So
    the bound is one ulp of the largest |clip logit| of the video."""
    doc, st, _, clips, videos, _ = golden
    nv = np.ones(len(clips), np.int32)
    groups = [[c for _, c in v] for v in videos]
    for name, want in doc["fusion"].items():
        tm, vm = name.split("/")
        got = R.reduce_fusion(st["red_logits"], nv, groups, tm, vm)
        for g, w, grp in zip(got, want, groups):
            ulp = np.spacing(np.abs(st["red_logits"][[c for t in grp for c in t]]).max())
            tl, wl = g["track_logit"], np.asarray(w["track_logit"], np.float32)
            if tm == "median":
                assert np.array_equal(tl, wl)
            else:
                print(name, "track means: max |statement - reference| %.3g, bound %.3g" % (np.abs(tl - wl).max(), ulp))
                assert (np.abs(tl - wl) <= ulp).all()
            if tm == "median" and vm in ("max", "median"):
                assert g["video_logit"] == np.float32(w["video_logit"])
            else:
                assert abs(g["video_logit"] - np.float32(w["video_logit"])) <= ulp
            assert abs(float(g["video_prob"]) - w["video_prob"]) <= 2 ** -23


def test_best_reduction_statement_equals_the_reference(golden):
    doc, st, _, clips, videos, _ = golden
    nv = np.ones(len(clips), np.int32)
    groups = [[c for _, c in v] for v in videos]
    for mode, want in doc["best"].items():
        got = R.best_aggregate(st["red_probs"], nv, groups, mode, doc["prob_thresh"])
        for g, w, v in zip(got, want, videos):
            for i, (key, _) in enumerate(v):
                assert float(g["track_score"][i]) == w["tracks"][key]["track_score"], (mode, key)        # fp64, exact
                assert int(g["track_pred"][i]) == w["tracks"][key]["track_pred"]
            assert float(g["video_score"]) == w["video_score"] and g["video_pred"] == w["video_pred"]
    # the statement's own sigmoid is the correctly rounded one: within an ulp of torch's
    assert (np.abs(R.sigmoid(st["red_logits"]) - st["red_probs"]) <= np.spacing(st["red_probs"])).all()


def test_lower_median_and_midpoint_median_differ_on_an_even_count(golden):
    doc, st, _, clips, videos, _ = golden
    even = [c for v in videos for _, c in v if len(c) % 2 == 0 and len(set(st["red_logits"][c].tolist())) == len(c)]
    assert even, "the golden holds a track with an even count of distinct logits"
    c = even[0]
    lo = R.lower_median(st["red_logits"][c])
    assert lo == np.sort(st["red_logits"][c])[len(c) // 2 - 1] and lo != np.float32(np.median(st["red_logits"][c]))
    p = st["red_probs"][c].astype(np.float64)
    assert R.mid_median(p) == np.median(p) != np.sort(p)[len(c) // 2 - 1]


def test_sigmoid_to_logit_equals_the_reference(golden):
    doc = golden[0]
    for p, want in doc["sigmoid_to_logit"]:
        assert DV.sigmoid_to_logit(p) == want
