"""GPU: af_dual_clip_features_ex and af_lmk_video_reduce (csrc/af_dual_video.hip) equal the numpy statement tests/lmkdisc_ref.py, with
guard bands around every output; ``LMKDisc`` sits within the dual-encoder gate of the reference's fp64 logits
(tests/golden/lmk_disc.*); ``LmkVideoScorer`` equals the hand composition statement features -> ``LMKDisc`` -> the reduce launch.

The video score is the one figure that is not exact: the device's fp64 ``log1p`` / ``exp`` are not numpy's.  Measured on the cases of
``test_reduction_equals_the_statement`` on an MI355X: max |device - statement| = 0.0 (``VIDEO_SCORE_MEASURED``; the test prints it).
The test asserts at 8 x that figure and never above (3 n_tracks + 1) * 2^-49, what two-ulp ``log1p`` and ``exp`` plus the sequential
sum allow for values below 16."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
import dualvideo_ref as R
import lmkdisc_ref as S
from test_hip_dualvideo import F_SENT, I_SENT, assert_guards, gen_track, guarded, run_features
from af_mi355x import dual_video as DV, dualrun

pytestmark = pytest.mark.gpu
VIDEO_SCORE_MEASURED = 0.0             # max |device - statement| of video_score, measured on the GPU (see the module docstring)


def run_ex(tracks, clips, T=8, rot=False, pad_zero=True, mode="none", pitch_pad=0, aus=None, stats=None):
    """af_dual_clip_features_ex on its own.  tracks: [lmk (n, P, 2)]; aus: None (A null, the tracks' au pointers null) or [au (n, K)].
    Guard bands around L, nvalid (and A).  -> (L, nvalid) or (A, L, nvalid)"""
    from af_mi355x import _lib
    keep, table = [], (_lib.DualvTrack * len(tracks))()
    K = 0 if aus is None else aus[0].shape[1]
    for i, lmk in enumerate(tracks):
        n, P = lmk.shape[:2]
        lb = torch.full((n, 2 * P + pitch_pad), F_SENT, dtype=torch.float32)
        lb[:, :2 * P] = torch.from_numpy(lmk.reshape(n, 2 * P))
        lb = lb.cuda()
        ab = None if aus is None else torch.from_numpy(np.ascontiguousarray(aus[i], np.float32)).cuda()
        keep += [lb, ab]
        table[i] = _lib.DualvTrack(lb.data_ptr(), None if ab is None else ab.data_ptr(), 2 * P + pitch_pad, K, n)
    tt = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    ct = torch.tensor([[t, f, n, 0] for t, f, n in clips], dtype=torch.int32).cuda()
    nc = len(clips)
    sdev = [torch.from_numpy(np.asarray(stats[k], np.float32)).cuda() for k in ("au_mean", "au_std", "lmk_mean", "lmk_std")] if stats else []
    opts = _lib.DualvOpts(T, K, {"none": 0, "clip": 1, "global": 2}[mode], 0, 1, 1, *[t.data_ptr() for t in sdev])
    Lb, L = guarded(nc * T * 132, torch.float32, F_SENT)
    Nb, N = guarded(nc, torch.int32, I_SENT)
    Ab, A = guarded(nc * T * 3 * K, torch.float32, F_SENT) if K else (None, None)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.af_dual_clip_features_ex(C.c_void_p(tt.data_ptr()), len(tracks), C.c_void_p(ct.data_ptr()), nc, C.byref(opts), int(rot),
                                                 int(pad_zero), None if A is None else C.c_void_p(A.data_ptr()), C.c_void_p(L.data_ptr()),
                                                 C.c_void_p(N.data_ptr()), st), "features_ex")
    torch.cuda.synchronize()
    assert_guards(Lb, nc * T * 132, F_SENT), assert_guards(Nb, nc, I_SENT)
    out = (L.cpu().numpy().reshape(nc, T, 132), N.cpu().numpy())
    if K:
        assert_guards(Ab, nc * T * 3 * K, F_SENT)
        out = (A.cpu().numpy().reshape(nc, T, 3 * K),) + out
    return out


def check_ex(tracks, clips, T=8, rot=False, pad_zero=True, mode="none", **kw):
    L, nv = run_ex(tracks, clips, T=T, rot=rot, pad_zero=pad_zero, mode=mode, **kw)
    wL, wnv = S.features(tracks, clips, T=T, rot_invariant=rot, pad="zero" if pad_zero else "fixT", mode=mode)
    assert np.array_equal(nv, wnv), (nv, wnv)
    assert np.array_equal(L, wL), "L differs from the statement (T %d rot %s pad_zero %s mode %s)" % (T, rot, pad_zero, mode)
    return L, nv


def lmk_track(rng, n, P=478):
    """a track whose mouth line tilts and whose nose moves from frame to frame"""
    lmk = gen_track(rng, n, P)[0]
    ang = rng.uniform(-0.6, 0.6, n)
    mid = np.asarray([0.5, 0.7]) + rng.normal(0, 0.01, (n, 2))
    half = 0.1 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    lmk[:, R.ML], lmk[:, R.MR] = (mid - half).astype(np.float32), (mid + half).astype(np.float32)
    return lmk


# ---- the feature launch --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,pitch_pad", [(467, 0), (478, 3)])                  # row pitches 934 and 959
@pytest.mark.parametrize("rot", [False, True])
def test_clip_lengths_1_to_8_in_both_pad_modes(P, pitch_pad, rot):
    rng = np.random.default_rng(P + rot)
    tracks = [lmk_track(rng, n, P) for n in (1, 3, 8, 9)]
    clips = [(0, 0, 1), (1, 0, 3), (1, 1, 2), (2, 0, 8), (2, 2, 6)] + [(3, 9 - n, n) for n in range(1, 9)] + [(3, 0, 8)]
    L, nv = check_ex(tracks, clips, rot=rot, pitch_pad=pitch_pad)
    assert nv.tolist() == [c[2] for c in clips]
    for i, n in enumerate(nv):
        assert L[i, :n].any() and not L[i, n:].any() and not np.signbit(L[i, n:]).any()
    again, _ = run_ex(tracks, clips, rot=rot, pitch_pad=pitch_pad)
    assert again.tobytes() == L.tobytes()                                        # a rerun is bit-identical
    check_ex(tracks, clips, rot=rot, pad_zero=False, pitch_pad=pitch_pad)        # fixT: the last row repeated
    check_ex(tracks, clips, rot=rot, pad_zero=False, mode="clip", pitch_pad=pitch_pad)      # ... and the clip z-score behind the rotation


def test_T16_and_a_centre_crop():
    rng = np.random.default_rng(16)
    tracks = [lmk_track(rng, 20), lmk_track(rng, 9)]
    clips = [(0, 0, 16), (0, 4, 16), (1, 0, 9), (0, 7, 1), (0, 3, 12)]
    for rot in (False, True):
        check_ex(tracks, clips, T=16, rot=rot)
        check_ex(tracks, clips, T=5, rot=rot, pad_zero=False, mode="clip")       # fixT keeps the centred 5 rows of the longer clips
    L, nv = run_ex(tracks, clips, T=5, rot=True)                                 # collate_pad never shortens: longer than T is a bad record
    assert nv.tolist() == [0, 0, 0, 1, 0] and not L[[0, 1, 2, 4]].any()


@pytest.mark.parametrize("rot", [False, True])
def test_dropped_frames_an_empty_clip_and_a_record_that_leaves_its_track(rot):
    rng = np.random.default_rng(3)
    lmk = lmk_track(rng, 40)
    for f in (0, 12, 23):                                    # ml == mr: the first, a middle and the last frame of a clip
        lmk[f, R.MR] = lmk[f, R.ML]
    lmk[26, R.ML, 1] = np.nan
    lmk[27, R.MR, 0] = np.inf
    lmk[32:40, R.MR] = lmk[32:40, R.ML]                      # every frame of a clip
    lmk[33, R.ML] = np.nan
    clips = [(0, 0, 8), (0, 8, 8), (0, 16, 8), (0, 24, 8), (0, 32, 8), (0, 30, 4), (0, 36, 8), (1, 0, 8), (0, -1, 4), (0, 0, 17)]
    L, nv = check_ex([lmk], clips[:6], rot=rot)
    assert nv.tolist() == [7, 7, 7, 6, 0, 2] and not L[4].any()
    L, nv = run_ex([lmk], clips, rot=rot)
    assert nv.tolist() == [7, 7, 7, 6, 0, 2, 0, 0, 0, 0] and not L[6:].any()
    check_ex([lmk], clips[:6], rot=rot, pad_zero=False, mode="clip")


def test_mouth_line_horizontal_vertical_and_reversed():
    rng = np.random.default_rng(9)
    lmk = gen_track(rng, 8)[0]
    lmk[:, R.NOSE] = (0.5, 0.5)
    ends = [((0.4, 0.7), (0.6, 0.7)), ((0.6, 0.7), (0.4, 0.7)), ((0.5, 0.6), (0.5, 0.8)), ((0.5, 0.8), (0.5, 0.6)),
            ((0.4, 0.6), (0.6, 0.8)), ((0.6, 0.8), (0.4, 0.6)), ((0.4, 0.7), (0.6, 0.7)), ((0.375, 0.75), (0.625, 0.75))]
    for f, (ml, mr) in enumerate(ends):
        lmk[f, R.ML], lmk[f, R.MR] = ml, mr
    L, nv = check_ex([lmk], [(0, 0, 8)], rot=True)
    plain, _ = check_ex([lmk], [(0, 0, 8)], rot=False)
    assert nv[0] == 8
    pts, raw = L[0].reshape(8, 66, 2), plain[0].reshape(8, 66, 2)
    assert np.array_equal(pts[7], raw[7]) and np.array_equal(pts[1], -raw[1])    # horizontal, dy exactly 0: untouched; reversed: negated
    assert (np.abs(pts[:, S.PT_MR, 1] - pts[:, S.PT_ML, 1]) <= 1e-6).all() and (pts[:, S.PT_MR, 0] > pts[:, S.PT_ML, 0]).all()
    assert np.allclose(pts[2, :, 0], raw[2, :, 1], atol=1e-6) and np.allclose(pts[2, :, 1], -raw[2, :, 0], atol=1e-6)   # a quarter turn


def test_ex_with_action_units_and_the_plain_entry_agree():
    rng = np.random.default_rng(4)
    both = [gen_track(rng, 12), gen_track(rng, 9)]
    for t in both:
        t[0][:] = lmk_track(rng, len(t[0]))
    clips = [(0, 0, 8), (0, 4, 8), (1, 0, 9), (1, 3, 2)]
    lm, au = [t[0] for t in both], [t[1] for t in both]
    for mode in ("none", "clip"):
        want = run_features(both, clips, T=8, mode=mode)                         # af_dual_clip_features
        got = run_ex(lm, clips, T=8, rot=False, pad_zero=False, mode=mode, aus=au)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        A, L, nv = run_ex(lm, clips, T=8, rot=True, pad_zero=False, mode=mode, aus=au)
        assert A.tobytes() == want[0].tobytes() and np.array_equal(nv, want[2])
        assert np.array_equal(L, S.features(lm, clips, T=8, rot_invariant=True, pad="fixT", mode=mode)[0])


def test_ex_refuses_zero_padding_with_a_zscore_or_action_units():
    from af_mi355x import _lib
    opts = _lib.DualvOpts(8, 0, 1, 0, 0, 0, None, None, None, None)
    args = (None, 0, None, 0, C.byref(opts), 0, _lib.DUALV_PAD_ZERO, None, None, None, None)
    assert _lib.lib.af_dual_clip_features_ex(*args) != 0 and b"zero padding" in _lib.lib.af_last_error()
    opts.zscore_mode = 0
    assert _lib.lib.af_dual_clip_features_ex(*args) == 0                        # no clips: nothing to do
    assert _lib.lib.af_dual_clip_features_ex(*args[:6], 2, *args[7:]) != 0


# ---- LMKDisc -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    doc, st, src_doc, src = load_json("lmk_disc.json"), load_npz("lmk_disc.npz"), load_json("dual_video.json"), load_npz("dual_video.npz")
    raw = [[src["v%d_t%d_lmk" % (vi, ti)] for ti in range(len(v["tracks"]))] for vi, v in enumerate(src_doc["videos"])]
    keys = [[t["key"] for t in v["tracks"]] for v in src_doc["videos"]]
    nets = {}
    for variant, kw in doc["variants"].items():
        m = dualrun.LMKDisc(132, **kw)
        assert m.load({"model": dualrun.lmk_disc_synthetic_state_dict(132, seed=doc["weights_seed"], **kw)}) == ([], [])
        nets[variant] = m.cuda().eval()
    return dict(doc=doc, st=st, raw=raw, keys=keys, nets=nets)


def case_inputs(g, case):
    """(x (B, T, 132), mask (B, T)) of a golden case: the statement's rows, which are the reference's bit for bit"""
    feats = [S.clip_features(g["raw"][vi][ti][s:s + n], T=case["T"]) for vi, ti, s, n in case["clips"]]
    assert [f[1] for f in feats] == case["lengths"]
    x = torch.from_numpy(np.stack([f[0] for f in feats])).cuda()
    mask = torch.arange(case["T"]).expand(len(feats), -1) >= torch.tensor(case["lengths"]).view(-1, 1)
    return x, mask.cuda()


@pytest.mark.parametrize("name", ["b6", "b1", "t16", "nomask", "depth1"])
def test_lmkdisc_sits_within_the_gate_of_the_reference_fp64_logits(golden, name):
    case = next(c for c in golden["doc"]["cases"] if c["name"] == name)
    net = golden["nets"][case["variant"]]
    x, mask = case_inputs(golden, case)
    with torch.inference_mode():
        got = net(x, key_padding_mask=mask if case["masked"] else None)
        assert got.shape == (len(case["clips"]),) and got.dtype == torch.float32 and got.is_cuda
        d = np.abs(got.cpu().numpy().astype(np.float64) - golden["st"]["logits_" + name])
        print("%s: max |logit - reference fp64| %.3g" % (name, d.max()))
        assert d.max() <= 3e-5
        for b in range(len(case["clips"])):                                      # a clip's logit does not depend on its batch
            one = net(x[b:b + 1], key_padding_mask=mask[b:b + 1] if case["masked"] else None)
            assert torch.equal(one, got[b:b + 1])


def test_lmkdisc_mask_contract(golden):
    net = golden["nets"]["ff512"]
    x = torch.zeros((2, 8, 132), device="cuda")
    hole = torch.zeros((2, 8), dtype=torch.bool, device="cuda")
    hole[0, 3] = True
    with pytest.raises(ValueError, match="suffix"):
        net(x, key_padding_mask=hole)
    with pytest.raises(ValueError, match="valid frame"):
        net(x, key_padding_mask=torch.ones((2, 8), dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        net(x, key_padding_mask=torch.zeros((2, 7), dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        net(torch.zeros((2, 17, 132), device="cuda"))
    ok = torch.zeros((2, 8), dtype=torch.bool, device="cuda")
    ok[1, 5:] = True
    net(x, key_padding_mask=ok)
    assert net._mask_checked[0] is ok                                            # remembered: not read back again until modified


# ---- the reduction -------------------------------------------------------------------------------------------------------------------

def run_lmk_reduce(logits, nvalid, videos, invert=False, thresh=0.5):
    from af_mi355x import _lib
    nc, nt, nv = len(logits), sum(len(v) for v in videos), len(videos)
    vt, tc, ci = [0], [0], []
    for tracks in videos:
        for clips in tracks:
            ci += list(clips)
            tc.append(len(ci))
        vt.append(len(tc) - 1)
    dev = lambda a, dt: torch.tensor(a, dtype=dt).cuda()                       # noqa: E731
    lg, nvd = torch.from_numpy(np.asarray(logits, np.float32)).cuda(), dev(list(nvalid), torch.int32)
    vtd, tcd, cid = dev(vt, torch.int32), dev(tc, torch.int32), dev(ci if ci else [0], torch.int32)
    spec = [("clip_score", torch.float64, nc, F_SENT), ("track_score", torch.float64, nt, F_SENT), ("track_pred", torch.int32, nt, I_SENT),
            ("track_count", torch.int32, nt, I_SENT), ("video_score", torch.float64, nv, F_SENT), ("video_pred", torch.int32, nv, I_SENT),
            ("video_count", torch.int32, nv, I_SENT)]
    bufs = {name: guarded(n, dt, s) for name, dt, n, s in spec}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.af_lmk_video_reduce(C.c_void_p(lg.data_ptr()), C.c_void_p(nvd.data_ptr()), nc, C.c_void_p(vtd.data_ptr()), nv,
                                            C.c_void_p(tcd.data_ptr()), nt, C.c_void_p(cid.data_ptr()), int(invert), C.c_double(thresh),
                                            *[C.c_void_p(bufs[name][1].data_ptr()) for name, _, _, _ in spec], st), "lmk_reduce")
    torch.cuda.synchronize()
    for name, _, n, s in spec:
        assert_guards(bufs[name][0], n, s)
    return {name: bufs[name][1].cpu().numpy() for name, _, _, _ in spec}


def reduce_cases():
    """1 to 3 videos of 1 to 4 tracks of 1 to 5 clips, logits of +-40 (scores that clip), a track of nvalid == 0 clips only, a video
    with no surviving track"""
    rng = np.random.default_rng(31)
    out = []
    for sizes in ([[1]], [[2, 5], [3]], [[1, 2, 3, 4], [5, 4], [2, 2, 1]]):
        videos, n = [], 0
        for tracks in sizes:
            videos.append([list(range(n + sum(tracks[:i]), n + sum(tracks[:i + 1]))) for i in range(len(tracks))])
            n += sum(tracks)
        logits = rng.normal(0, 2, n).astype(np.float32)
        nvalid = np.full(n, 8, np.int32)
        out.append((logits, nvalid, videos))
    logits, nvalid, videos = out[-1]
    logits[[0, 3, 10]], logits[[1, 11]] = 40.0, -40.0
    nvalid[videos[0][1]] = 0                                                   # a track left empty
    nvalid[videos[0][3][1]] = 0                                                # 4 clips -> 3
    for clips in videos[2]:
        nvalid[clips] = 0                                                      # a video left empty
    return out


@pytest.mark.parametrize("invert", [False, True])
def test_reduction_equals_the_statement(invert):
    worst, diffs = 0.0, []
    for logits, nvalid, videos in reduce_cases():
        for thresh in (0.5, 0.37):
            got = run_lmk_reduce(logits, nvalid, videos, invert, thresh)
            score, want = S.reduce_lmk(logits, nvalid, videos, invert, thresh)
            named = sorted(c for v in videos for t in v for c in t)
            assert np.array_equal(got["clip_score"][named], score[named])
            for name in ("track_score", "track_pred", "track_count"):
                assert np.array_equal(got[name], np.concatenate([w[name] for w in want])), name
            assert got["video_count"].tolist() == [w["n_tracks"] for w in want]
            assert got["video_pred"].tolist() == [w["video_pred"] for w in want]
            for v, w in enumerate(want):
                d = abs(got["video_score"][v] - w["video_score"])
                worst = max(worst, d)
                diffs.append((d, min(8 * VIDEO_SCORE_MEASURED, (3 * w["n_tracks"] + 1) * 2.0 ** -49)))
                if w["n_tracks"] == 0:
                    assert got["video_score"][v] == 0.0 and got["video_pred"][v] == 0
    print("max |device video_score - statement| %.3g" % worst)
    assert all(d <= bound for d, bound in diffs), [x for x in diffs if x[0] > x[1]]
    logits, nvalid, videos = reduce_cases()[-1]
    assert run_lmk_reduce(logits, nvalid, videos, invert)["video_count"].tolist() == [3, 2, 0]


def test_clip_scores_outside_the_csr_stay_untouched():
    got = run_lmk_reduce(np.asarray([0.5, -1.0, 2.0], np.float32), [8, 8, 8], [[[2], [0]]])
    assert got["clip_score"][1] == F_SENT and got["track_score"].tolist() == S.clip_score(np.asarray([2.0, 0.5], np.float32)).tolist()


# ---- LmkVideoScorer ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def videos(golden):
    """the golden's three videos, and a fourth with a clip and a track whose frames are all dropped"""
    g = golden
    vids = [[DV.DualTrack(lmk, None, key) for lmk, key in zip(v, k)] for v, k in zip(g["raw"], g["keys"])]
    rng = np.random.default_rng(77)
    a, b, c = lmk_track(rng, 16), lmk_track(rng, 8), lmk_track(rng, 11)
    a[8:16, R.MR] = a[8:16, R.ML]                                              # its third clip window (8..15) loses every frame
    b[:, R.ML, 0] = np.nan                                                     # a track with nothing left
    vids.append([DV.DualTrack(a, None, "track_0", clips=[(0, 8), (4, 8), (8, 8)]), DV.DualTrack(b, None, "track_1"),
                 DV.DualTrack(c, None, "track_2", clips=[(0, 5), (3, 8), (10, 1)])])
    return vids


def hand_composition(net, vids, T, rot, invert, thresh):
    tracks = [tr.landmarks for v in vids for tr in v]
    clips, groups, n = [], [], 0
    for v in vids:
        groups.append([])
        for tr in v:
            groups[-1].append(list(range(len(clips), len(clips) + len(tr.clips))))
            clips += [(n, f, ln) for f, ln in tr.clips]
            n += 1
    L, nv = S.features(tracks, clips, T=T, rot_invariant=rot)
    mask = torch.arange(T).expand(len(clips), -1) >= torch.from_numpy(np.maximum(nv, 1)).view(-1, 1)
    with torch.inference_mode():
        logits = net(torch.from_numpy(L).cuda(), key_padding_mask=mask.cuda()).cpu().numpy()
    red = run_lmk_reduce(logits, nv, groups, invert, thresh)
    out, t = [], 0
    for vi, v in enumerate(vids):
        rec = {"clips": [(tr.key, float(red["clip_score"][c])) for tr, cl in zip(v, groups[vi]) for c in cl if nv[c] > 0],
               "tracks": {tr.key: {"score_track_median": float(red["track_score"][t + i]), "pred": int(red["track_pred"][t + i])}
                          for i, tr in enumerate(v) if red["track_count"][t + i] > 0},
               "score_video_or": float(red["video_score"][vi]), "pred": int(red["video_pred"][vi]), "n_tracks": int(red["video_count"][vi])}
        out.append(rec)
        t += len(v)
    return out, L, nv, logits, groups


@pytest.mark.parametrize("rot,invert", [(False, False), (True, True)])
def test_scorer_equals_the_hand_composition(golden, videos, rot, invert):
    net = golden["nets"]["ff512"]
    want, L, nv, logits, groups = hand_composition(net, videos, 8, rot, invert, 0.4)
    scorer = DV.LmkVideoScorer(net, T=8, rot_invariant=rot, invert=invert, thresh=0.4)
    gL, gnv = scorer.features(videos)
    assert np.array_equal(gL.cpu().numpy(), L) and np.array_equal(gnv.cpu().numpy(), nv)
    if not rot:
        assert np.array_equal(L[:len(golden["doc"]["clips"])], golden["st"]["ref_L_rot0"])       # the reference's own rows
    score, glog, _ = scorer.clip_scores(videos)
    keep = nv > 0
    assert np.array_equal(glog[keep], logits[keep]) and np.array_equal(score[keep], S.clip_score(logits, invert)[keep])
    got = scorer.score(videos)
    assert got == want
    for chunk in (1, 7):
        assert DV.LmkVideoScorer(net, T=8, rot_invariant=rot, invert=invert, thresh=0.4, chunk_clips=chunk).score(videos) == want
    assert DV.CHUNK_CLIPS > len(nv) > 7
    # the exact levels against the statement; the last video: a clip, then a whole track, left out
    _, ref = S.reduce_lmk(logits, nv, groups, invert, 0.4)
    for g, w, v in zip(got, ref, videos):
        kept = [i for i, n in enumerate(w["track_count"]) if n]
        assert [g["tracks"][v[i].key]["score_track_median"] for i in kept] == [float(w["track_score"][i]) for i in kept]
        assert g["n_tracks"] == w["n_tracks"] == len(g["tracks"]) and len(g["clips"]) == int(w["track_count"].sum())
    assert got[3]["n_tracks"] == 2 and list(got[3]["tracks"]) == ["track_0", "track_2"] and len(got[3]["clips"]) == 2 + 3


def test_host_and_device_resident_tracks_agree(golden, videos):
    net = golden["nets"]["ff512"]
    on_dev = []
    for v in videos:
        row = []
        for tr in v:
            buf = torch.zeros((tr.n, 2 * 478 + 3), dtype=torch.float32, device="cuda")          # padded rows
            buf[:, :956] = torch.from_numpy(tr.landmarks.reshape(-1, 956)).cuda()
            row.append(DV.DualTrack(buf[:, :956].unflatten(1, (478, 2)), None, tr.key, clips=tr.clips))
        on_dev.append(row)
    assert on_dev[0][0].landmarks.stride() == (959, 2, 1)
    scorer = DV.LmkVideoScorer(net)
    want = scorer.score(videos)
    assert scorer.score(on_dev) == want and scorer.score([on_dev[0], videos[1], on_dev[2], videos[3]]) == want


def test_scorer_contract_errors_come_before_any_launch(golden, monkeypatch):
    from af_mi355x import _lib
    net = golden["nets"]["ff512"]
    launched = []
    for name in ("af_dual_clip_features_ex", "af_lmk_video_reduce", "af_dual_branch_encoders"):
        monkeypatch.setattr(_lib.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    rng = np.random.default_rng(0)
    lmk, au = gen_track(rng, 20)
    with pytest.raises(ValueError, match="landmarks alone"):
        DV.LmkVideoScorer(net).score([[DV.DualTrack(lmk, au, "0")]])
    with pytest.raises(ValueError, match="longer than T"):
        DV.LmkVideoScorer(net, T=6).score([[DV.DualTrack(lmk, None, "0")]])
    with pytest.raises(ValueError, match="distinct"):
        DV.LmkVideoScorer(net).score([[DV.DualTrack(lmk, None, "0"), DV.DualTrack(lmk, None, "0")]])
    with pytest.raises(ValueError):
        DV.LmkVideoScorer(net, T=17)
    with pytest.raises(ValueError):
        DV.LmkVideoScorer(dualrun.DualEncoderAU_LMK())
    assert not launched


# ---- DualVideoScorer(rot_invariant) ----------------------------------------------------------------------------------------------------

def test_dual_video_scorer_rot_invariant(golden):
    src_doc, src = load_json("dual_video.json"), load_npz("dual_video.npz")
    sp = dualrun.DualSpec()
    net = dualrun.DualEncoderAU_LMK(mlp_ratio=float(sp.ff) / sp.d_model)
    net.load_state_dict(dualrun.dual_synthetic_state_dict(sp, seed=3))
    net = net.cuda().eval()
    vids, tracks, clips = [], [], []
    for vi, v in enumerate(src_doc["videos"]):
        vids.append([])
        for ti, t in enumerate(v["tracks"]):
            lmk, au = src["v%d_t%d_lmk" % (vi, ti)], src["v%d_t%d_au" % (vi, ti)]
            vids[-1].append(DV.DualTrack(lmk, au, t["key"]))
            clips += [(len(tracks), s, 8) for s in t["clips"]]
            tracks.append((lmk, au))
    wA, wL, wnv = R.features(tracks, clips, T=8, mode="clip")
    A, L, nv = DV.DualVideoScorer(net, rot_invariant=True).features(vids)
    assert np.array_equal(A.cpu().numpy(), wA) and np.array_equal(nv.cpu().numpy(), wnv)
    assert np.array_equal(L.cpu().numpy(), S.features([t[0] for t in tracks], clips, T=8, rot_invariant=True, pad="fixT", mode="clip")[0])
    assert not np.array_equal(L.cpu().numpy(), wL)
    for kw in ({}, {"rot_invariant": False}):                                    # the default is today's output
        A, L, nv = DV.DualVideoScorer(net, **kw).features(vids)
        assert np.array_equal(A.cpu().numpy(), wA) and np.array_equal(L.cpu().numpy(), wL) and np.array_equal(nv.cpu().numpy(), wnv)
    assert DV.DualVideoScorer(net, rot_invariant=True).score(vids) != DV.DualVideoScorer(net).score(vids)
    with pytest.raises(ValueError, match="action units"):
        DV.DualVideoScorer(net).features([[DV.DualTrack(tracks[0][0], None, "0")]])
