"""GPU: af_dual_clip_features and af_dual_video_reduce (csrc/af_dual_video.hip) equal the numpy statement tests/dualvideo_ref.py bit
for bit, with guard bands around every output, and ``DualVideoScorer`` equals the hand composition statement features -> the
existing DualEncoderAU_LMK forward -> statement reduction on the golden's videos (tests/golden/dual_video.*)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_json, load_npz
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dualrun_oracle  # noqa: E402
import dualvideo_ref as R  # noqa: E402
from af_mi355x import dual_video as DV, dualrun  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, F_SENT, I_SENT = 64, 12345.0, -77
MODES = {"none": 0, "clip": 1, "global": 2}
APPLY = {"both": 0, "au": 1, "lmk": 2}


def gen_track(rng, n, P=478, K=12):
    base = rng.uniform(0.2, 0.8, (P, 2))
    base[R.ML], base[R.MR] = (0.4, 0.7), (0.6, 0.7)
    lmk = (base[None] + rng.normal(0, 0.01, (n, P, 2))).astype(np.float32)
    return lmk, rng.uniform(0, 1, (n, K)).astype(np.float32)


def guarded(n, dtype, sentinel):
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def assert_guards(buf, n, sentinel):
    assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all()), "a write outside the output"


def run_features(tracks, clips, T=8, mode="clip", apply="both", stats=None, use_delta=True, use_delta2=True, pad=0):
    """the launch on its own, rows of 2P + pad and K + pad floats, guard bands around A, L and nvalid"""
    from af_mi355x import _lib
    keep, table = [], (_lib.DualvTrack * len(tracks))()
    K = tracks[0][1].shape[1]
    for i, (lmk, au) in enumerate(tracks):
        n, P = lmk.shape[:2]
        lb = torch.full((n, 2 * P + pad), F_SENT, dtype=torch.float32)
        lb[:, :2 * P] = torch.from_numpy(lmk.reshape(n, 2 * P))
        ab = torch.full((n, K + pad), F_SENT, dtype=torch.float32)
        ab[:, :K] = torch.from_numpy(au)
        lb, ab = lb.cuda(), ab.cuda()
        keep += [lb, ab]
        table[i] = _lib.DualvTrack(lb.data_ptr(), ab.data_ptr(), 2 * P + pad, K + pad, n)
    tt = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    ct = torch.tensor([[t, f, n, 0] for t, f, n in clips], dtype=torch.int32).cuda()
    F = K * (1 + int(use_delta) + int(use_delta2))
    nc = len(clips)
    sdev = [torch.from_numpy(np.asarray(stats[k], np.float32)).cuda() for k in ("au_mean", "au_std", "lmk_mean", "lmk_std")] if stats else []
    opts = _lib.DualvOpts(T, K, MODES[mode], APPLY[apply], int(use_delta), int(use_delta2), *[t.data_ptr() for t in sdev])
    Ab, A = guarded(nc * T * F, torch.float32, F_SENT)
    Lb, L = guarded(nc * T * 132, torch.float32, F_SENT)
    Nb, N = guarded(nc, torch.int32, I_SENT)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.af_dual_clip_features(C.c_void_p(tt.data_ptr()), len(tracks), C.c_void_p(ct.data_ptr()), nc, C.byref(opts),
                                              C.c_void_p(A.data_ptr()), C.c_void_p(L.data_ptr()), C.c_void_p(N.data_ptr()), st), "features")
    torch.cuda.synchronize()
    assert_guards(Ab, nc * T * F, F_SENT), assert_guards(Lb, nc * T * 132, F_SENT), assert_guards(Nb, nc, I_SENT)
    return A.cpu().numpy().reshape(nc, T, F), L.cpu().numpy().reshape(nc, T, 132), N.cpu().numpy()


def check_features(tracks, clips, nan=False, **kw):
    got = run_features(tracks, clips, **kw)
    kw.pop("pad", None)
    want = R.features(tracks, clips, **kw)
    for g, w, name in zip(got, want, ("A", "L", "nvalid")):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=nan), "%s differs from the statement (%s)" % (name, kw)
    return got


@pytest.mark.parametrize("P,pad", [(467, 0), (478, 3)])
@pytest.mark.parametrize("T", [8, 5])
def test_features_equal_the_statement_over_clip_lengths(P, pad, T):
    rng = np.random.default_rng(P + T)
    tracks = [gen_track(rng, 14, P)]
    clips = [(0, 0, 8), (0, 3, 5), (0, 2, 11), (0, 13, 1), (0, 6, 8), (0, 0, 14)]          # padded, centre-cropped, one row
    _, _, nv = check_features(tracks, clips, T=T, pad=pad)
    assert nv.tolist() == [8, 5, 11, 1, 8, 14]


def test_dropped_frames_are_compacted_and_an_empty_clip_is_zeros():
    rng = np.random.default_rng(3)
    lmk, au = gen_track(rng, 40)
    for f in (0, 12, 23):                                    # ml == mr: first, a middle and the last frame of a clip
        lmk[f, R.MR] = lmk[f, R.ML]
    lmk[26, R.ML, 1] = np.nan
    lmk[27, R.MR, 0] = np.inf
    lmk[32:40, R.MR] = lmk[32:40, R.ML]                      # every frame of the last clip
    lmk[33, R.ML] = np.nan
    clips = [(0, 0, 8), (0, 8, 8), (0, 16, 8), (0, 24, 8), (0, 32, 8), (0, 30, 4)]
    A, L, nv = check_features([(lmk, au)], clips)
    assert nv.tolist() == [7, 7, 7, 6, 0, 2]
    assert not A[4].any() and not L[4].any()
    for mode in ("none", "global"):
        stats = {"au_mean": np.zeros(36), "au_std": np.ones(36), "lmk_mean": np.zeros(132), "lmk_std": np.ones(132)}
        A, L, nv = check_features([(lmk, au)], clips, mode=mode, stats=stats if mode == "global" else None)
        assert nv[4] == 0 and not A[4].any() and not L[4].any()


@pytest.mark.parametrize("mode", ["none", "clip", "global"])
@pytest.mark.parametrize("apply", ["both", "au", "lmk"])
def test_every_zscore_mode_and_apply(mode, apply):
    rng = np.random.default_rng(11)
    tracks = [gen_track(rng, 19), gen_track(rng, 9)]
    stats = {"au_mean": rng.normal(0.3, 0.2, 36), "au_std": rng.uniform(0.1, 0.5, 36), "lmk_mean": rng.normal(0, 0.5, 132),
             "lmk_std": rng.uniform(0.2, 1.5, 132)}
    stats["au_std"][[3, 20]] = [1e-9, 0.0]                  # under the floor
    stats["lmk_std"][7] = np.nan
    clips = [(0, s, 8) for s in DV.clip_windows(19)] + [(1, 0, 8), (1, 1, 6)]
    check_features(tracks, clips, mode=mode, apply=apply, stats=stats if mode == "global" else None, nan=True)
    for d1, d2 in ((True, False), (False, True), (False, False)):
        check_features(tracks, clips[:2], mode=mode, apply=apply, stats=None if mode != "global" else
                       {k: v[:12 * (1 + d1 + d2)] if k.startswith("au") else v for k, v in stats.items()}, use_delta=d1, use_delta2=d2, nan=True)


def test_non_finite_points_and_action_units():
    rng = np.random.default_rng(5)
    lmk, au = gen_track(rng, 8)
    lmk[1, 33, 0], lmk[2, 7, 1], lmk[5, 163, 0] = np.nan, np.inf, -np.inf        # not the nose, not a mouth corner
    au[3, 2], au[4, 5], au[6, 7] = np.nan, np.inf, -np.inf
    clips = [(0, 0, 8)]
    big = np.finfo(np.float32).max
    A, L, _ = check_features([(lmk, au)], clips, mode="clip", apply="au")        # the landmarks only go through nan_to_num
    assert L[0, 1, 0] == 0 and L[0, 2, 3] == big and L[0, 5, 4] == -big and np.isfinite(A).all()
    A, L, _ = check_features([(lmk, au)], clips, mode="clip", apply="both")
    assert np.isfinite(A).all() and np.isfinite(L).all()
    A, L, _ = check_features([(lmk, au)], clips, mode="none", nan=True)          # passed through
    assert np.isnan(L[0, 1, 0]) and L[0, 2, 3] == np.inf and L[0, 5, 4] == -np.inf and np.isnan(A[0, 3, 2]) and A[0, 4, 5] == np.inf
    lmk[4, R.NOSE, 0] = np.nan                                                   # the nose: its frame stays, every x of it is NaN
    check_features([(lmk, au)], clips, mode="none", nan=True)
    check_features([(lmk, au)], clips, mode="clip")


def test_identical_rows_clip():
    rng = np.random.default_rng(8)
    lmk, au = gen_track(rng, 8)
    au[:] = au[0]
    lmk[:] = lmk[0]
    A, L, _ = check_features([(lmk, au)], [(0, 0, 8)], mode="clip")
    x = R.au_rows(au)
    assert np.isfinite(A).all() and (np.abs(A) <= np.abs(x) * 2.0 ** -22 / 1e-6).all()


@pytest.mark.parametrize("count", [1, 131])
def test_clip_counts_and_tracks_sharing_frames(count):
    rng = np.random.default_rng(count)
    tracks = [gen_track(rng, 70), gen_track(rng, 75)]
    clips = ([(0, s, 8) for s in range(63)] + [(1, s, 8) for s in range(68)])[:count] if count > 1 else [(1, 67, 8)]
    assert len(clips) == count
    check_features(tracks, clips)


def test_a_clip_record_that_leaves_its_track_reads_nothing():
    rng = np.random.default_rng(2)
    tracks = [gen_track(rng, 10)]
    A, L, nv = run_features(tracks, [(0, 4, 8), (1, 0, 8), (0, -1, 4), (0, 0, 17), (0, 0, 8)])
    assert nv.tolist() == [0, 0, 0, 0, 8] and not A[:4].any() and not L[:4].any()


# ---- the reduction ---------------------------------------------------------------------------------------------------------------

def run_reduce(logits, nvalid, videos, family, tmode, vmode="max", thresh=0.5):
    from af_mi355x import _lib
    nc, nt, nv = len(logits), sum(len(v) for v in videos), len(videos)
    vt, tc, ci = [0], [0], []
    for tracks in videos:
        for clips in tracks:
            ci += list(clips)
            tc.append(len(ci))
        vt.append(len(tc) - 1)
    dev = lambda a, dt: torch.tensor(a, dtype=dt).cuda()                       # noqa: E731
    lg, nvd = torch.from_numpy(np.asarray(logits, np.float32)).cuda(), dev(nvalid, torch.int32)
    vtd, tcd, cid = dev(vt, torch.int32), dev(tc, torch.int32), dev(ci if ci else [0], torch.int32)
    spec = [("track_logit", torch.float32, nt, F_SENT), ("track_prob", torch.float32, nt, F_SENT), ("video_logit", torch.float32, nv, F_SENT),
            ("video_prob", torch.float32, nv, F_SENT), ("clip_prob", torch.float32, nc, F_SENT), ("track_score", torch.float64, nt, F_SENT),
            ("track_pred", torch.int32, nt, I_SENT), ("video_score", torch.float64, nv, F_SENT), ("video_pred", torch.int32, nv, I_SENT),
            ("track_count", torch.int32, nt, I_SENT)]
    bufs = {name: guarded(n, dt, s) for name, dt, n, s in spec}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.af_dual_video_reduce(C.c_void_p(lg.data_ptr()), C.c_void_p(nvd.data_ptr()), nc, C.c_void_p(vtd.data_ptr()), nv,
                                             C.c_void_p(tcd.data_ptr()), nt, C.c_void_p(cid.data_ptr()), family, tmode, vmode, C.c_double(thresh),
                                             *[C.c_void_p(bufs[name][1].data_ptr()) for name, _, _, _ in spec], st), "reduce")
    torch.cuda.synchronize()
    for name, _, n, s in spec:
        assert_guards(bufs[name][0], n, s)
    return {name: bufs[name][1].cpu().numpy() for name, _, _, _ in spec}


@pytest.fixture(scope="module")
def reduce_case():
    """tracks of 1, 2, 3, 4, 65 and 300 clips (a wavefront, a chunk of 256 and more), ties and repeats, a video of one track, one of
    70 tracks, clips skipped at a track's start and end, a track and a video left empty, +-inf logits"""
    rng = np.random.default_rng(21)
    sizes = [[1, 2, 3, 4, 65, 300], [5], [int(n) for n in rng.integers(1, 6, 70)], [3, 2], [4, 1]]
    videos, n = [], 0
    for tracks in sizes:
        videos.append([list(range(n + sum(tracks[:i]), n + sum(tracks[:i + 1]))) for i in range(len(tracks))])
        n += sum(tracks)
    logits = rng.normal(0, 2, n).astype(np.float32)
    logits[rng.integers(0, n, 60)] = np.float32(0.75)                          # repeats
    logits[1], logits[2] = logits[2], logits[1]
    logits[3:6] = logits[3]                                                    # a track of one value
    nvalid = np.full(n, 8, np.int32)
    big = videos[0][4]
    nvalid[[big[0], big[1], big[-1], big[30]]] = 0                             # start, end and inside a track
    nvalid[videos[0][3]] = [0, 8, 8, 0]
    nvalid[videos[3][0]] = 0                                                   # a track left empty
    nvalid[videos[4][0]] = 0
    nvalid[videos[4][1]] = 0                                                   # a video left empty
    v1 = videos[1][0]
    logits[v1[0]], logits[v1[3]] = np.inf, -np.inf
    logits[videos[2][5][0]] = np.inf
    logits[videos[2][9][0]] = -np.inf
    return logits, nvalid, videos


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("tmode", ["median", "mean"])
@pytest.mark.parametrize("vmode", ["max", "median", "mean"])
def test_fusion_family_equals_the_statement(reduce_case, tmode, vmode):
    from af_mi355x import _lib
    logits, nvalid, videos = reduce_case
    got = run_reduce(logits, nvalid, videos, _lib.DUALV_FAMILY_FUSION, _lib.DUALV_TRACK[tmode], _lib.DUALV_VIDEO[vmode])
    want = R.reduce_fusion(logits, nvalid, videos, tmode, vmode)
    for name in ("track_logit", "track_prob", "track_count"):
        assert same(got[name], np.concatenate([w[name] for w in want])), name
    for name in ("video_logit", "video_prob"):
        assert same(got[name], [w[name] for w in want]), name
    assert np.isnan(got["video_logit"][4]) and got["track_count"][-2:].tolist() == [0, 0]
    assert (got["clip_prob"] == F_SENT).all() and (got["track_pred"] == I_SENT).all()      # the other family's outputs stay untouched


@pytest.mark.parametrize("mode", ["track_mean", "track_median", "track_majority"])
@pytest.mark.parametrize("thresh", [0.5, 0.594])
def test_best_family_equals_the_statement(reduce_case, mode, thresh):
    from af_mi355x import _lib
    logits, nvalid, videos = reduce_case
    got = run_reduce(logits, nvalid, videos, _lib.DUALV_FAMILY_BEST, _lib.DUALV_BEST[mode], 0, thresh)
    want = R.reduce_best(logits, nvalid, videos, mode, thresh)
    assert same(got["clip_prob"], R.sigmoid(logits))
    for name in ("track_score", "track_pred", "track_count"):
        assert same(got[name], np.concatenate([w[name] for w in want])), name
    for name in ("video_score", "video_pred"):
        assert same(got[name], [w[name] for w in want]), name
    assert got["video_score"][4] == 0.0 and got["video_pred"][4] == 0
    assert (got["track_logit"] == F_SENT).all() and (got["video_prob"] == F_SENT).all()


def test_lower_and_midpoint_medians_differ_on_the_device():
    from af_mi355x import _lib
    logits = np.asarray([0.3, -1.2, 2.0, 0.9], np.float32)
    nv, videos = np.full(4, 8, np.int32), [[[0, 1, 2, 3]]]
    f = run_reduce(logits, nv, videos, _lib.DUALV_FAMILY_FUSION, _lib.DUALV_TRACK["median"], 0)
    b = run_reduce(logits, nv, videos, _lib.DUALV_FAMILY_BEST, _lib.DUALV_BEST["track_median"], 0)
    assert f["track_logit"][0] == np.float32(0.3)
    p = R.sigmoid(logits).astype(np.float64)
    assert b["track_score"][0] == (p[0] + p[3]) / 2 == np.median(p)


# ---- DualVideoScorer ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup():
    g = load_json("f7_dualrun.json")
    sp = dualrun.DualSpec()
    sd = dualrun.dual_synthetic_state_dict(sp, seed=g["weights_seed"])
    net = dualrun.DualEncoderAU_LMK(au_dim=sp.au_dim, lmk_dim=sp.lmk_dim, d_model=sp.d_model, depth=sp.depth, heads=sp.heads,
                                    mlp_ratio=float(sp.ff) / sp.d_model, pool_tau=sp.pool_tau)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    doc, st = load_json("dual_video.json"), load_npz("dual_video.npz")
    raw, flat_tracks, flat_clips, groups = [], [], [], []
    for vi, v in enumerate(doc["videos"]):
        raw.append([(t["key"], st["v%d_t%d_lmk" % (vi, ti)], st["v%d_t%d_au" % (vi, ti)]) for ti, t in enumerate(v["tracks"])])
        by_key = {}
        for ti, t in enumerate(v["tracks"]):
            for s in t["clips"]:
                by_key.setdefault(t["key"], []).append(len(flat_clips))
                flat_clips.append((len(flat_tracks), s, 8))
            flat_tracks.append(raw[-1][ti][1:])
        groups.append([by_key[k] for k in DV.person_key_order(by_key)])
    # the hand composition: statement features -> the existing forward on the GPU -> (below) the statement reduction
    A, L, nv = R.features(flat_tracks, flat_clips, T=8, mode="clip")
    with torch.inference_mode():
        logits = net(torch.from_numpy(A).cuda(), torch.from_numpy(L).cuda())["bin_logits"].cpu().numpy()
    videos = [[DV.DualTrack(lmk, au, key) for key, lmk, au in v] for v in raw]
    return dict(doc=doc, st=st, sp=sp, sd=sd, net=net, raw=raw, videos=videos, groups=groups, A=A, L=L, nv=nv, logits=logits)


def test_scorer_equals_the_hand_composition(setup):
    s = setup
    scorer = DV.DualVideoScorer(s["net"])
    A, L, nv = scorer.features(s["videos"])
    assert np.array_equal(A.cpu().numpy(), s["A"]) and np.array_equal(L.cpu().numpy(), s["L"]) and np.array_equal(nv.cpu().numpy(), s["nv"])
    logits, nv = scorer.clip_logits(s["videos"])
    assert np.array_equal(logits, s["logits"])
    for tm, vm in (("median", "max"), ("mean", "median"), ("median", "mean")):
        got = DV.DualVideoScorer(s["net"], track_reduce=tm, video_agg=vm).score(s["videos"])
        want = R.reduce_fusion(s["logits"], s["nv"], s["groups"], tm, vm)
        for g, w, v, grp in zip(got, want, s["doc"]["videos"], s["groups"]):
            assert g["prob_video_dual"] == float(w["video_prob"]) and g["logit_video"] == float(w["video_logit"])
            assert g["prob_dual_per_track"] == [float(x) for x in w["track_prob"]]
            assert g["track_keys"] == DV.person_key_order(t["key"] for t in v["tracks"])
            assert g["n_clips"] == sum(len(c) for c in grp) == len(g["tracks"]) and g["agg"] == {"track": tm, "video": vm}
    for mode in ("track_mean", "track_median", "track_majority"):
        got = DV.DualVideoScorer(s["net"], agg_mode=mode, prob_thresh=0.45).score(s["videos"])
        want = R.reduce_best(s["logits"], s["nv"], s["groups"], mode, 0.45)
        for g, w, v in zip(got, want, s["doc"]["videos"]):
            keys = DV.person_key_order(t["key"] for t in v["tracks"])
            assert [g["tracks"][k]["track_score"] for k in keys] == [float(x) for x in w["track_score"]]
            assert [g["tracks"][k]["track_pred"] for k in keys] == [int(x) for x in w["track_pred"]]
            assert g["video_score"] == float(w["video_score"]) and g["video_pred"] == w["video_pred"]
            assert list(g["tracks"]) == [t["key"] for t in v["tracks"]]                # first seen, as the reference's dict fills


@pytest.mark.parametrize("chunk", [1, 7])
def test_results_do_not_depend_on_the_chunk_size(setup, chunk):
    s = setup
    assert DV.CHUNK_CLIPS > len(s["logits"]) > 7
    logits, nv = DV.DualVideoScorer(s["net"], chunk_clips=chunk).clip_logits(s["videos"])
    assert np.array_equal(logits, s["logits"]) and np.array_equal(nv, s["nv"])
    assert DV.DualVideoScorer(s["net"], chunk_clips=chunk).score(s["videos"]) == DV.DualVideoScorer(s["net"]).score(s["videos"])


def test_host_and_device_resident_tracks_agree(setup):
    s = setup
    on_dev = []
    for v in s["raw"]:
        row = []
        for key, lmk, au in v:
            buf = torch.zeros((lmk.shape[0], 2 * 478 + 3), dtype=torch.float32, device="cuda")       # padded rows
            buf[:, :956] = torch.from_numpy(lmk.reshape(-1, 956)).cuda()
            row.append(DV.DualTrack(buf[:, :956].unflatten(1, (478, 2)), torch.from_numpy(au).cuda(), key))
        on_dev.append(row)
    assert on_dev[0][0].landmarks.stride() == (959, 2, 1)
    scorer = DV.DualVideoScorer(s["net"])
    assert scorer.score(on_dev) == scorer.score(s["videos"])
    mixed = [on_dev[0], s["videos"][1], on_dev[2]]
    assert scorer.score(mixed) == scorer.score(s["videos"])


def test_fuse_equals_gated_moe_by_hand(setup):
    s = setup
    st = load_npz("f7_dualrun.npz")
    moe = dualrun.GatedMoE()
    moe.load_state_dict({k[len("moe_w_"):]: torch.from_numpy(st[k]) for k in st.files if k.startswith("moe_w_")})
    moe = moe.cuda().eval()
    p_rgb = [0.91, 0.08, 0.5]
    scorer = DV.DualVideoScorer(s["net"])
    z, g = scorer.fuse(s["videos"], p_rgb, moe)
    z_dual = torch.tensor([[r["logit_video"]] for r in scorer.score(s["videos"])], dtype=torch.float32).cuda()
    z_rgb = torch.tensor([[DV.sigmoid_to_logit(p)] for p in p_rgb], dtype=torch.float32).cuda()
    with torch.inference_mode():
        wz, wg = moe(z_rgb, z_dual)
    assert torch.equal(z, wz) and torch.equal(g, wg) and z.shape == (3, 1)
    with pytest.raises(ValueError):
        DV.DualVideoScorer(s["net"], agg_mode="track_mean").fuse(s["videos"], p_rgb, moe)


def test_logits_sit_within_the_oracle_on_the_reference_features(setup):
    s = setup
    keep = np.arange(len(s["logits"])) != s["doc"]["held_clip"]
    want, _ = dualrun_oracle.dual_forward(s["sd"], torch.from_numpy(s["st"]["ref_A_clip"]), torch.from_numpy(s["st"]["ref_L_clip"]), None,
                                          heads=s["sp"].heads, tau=s["sp"].pool_tau)
    got, _ = DV.DualVideoScorer(s["net"]).clip_logits(s["videos"])
    d = np.abs(got - want.numpy())
    print("max |logit - oracle| %.3g (held clip: %.3g)" % (d[keep].max(), d[~keep].max()))
    np.testing.assert_allclose(got[keep], want.numpy()[keep], rtol=0, atol=2e-5)


def test_contract_errors_come_before_any_launch(setup, monkeypatch):
    from af_mi355x import _lib
    s = setup
    launched = []
    for name in ("af_dual_clip_features", "af_dual_video_reduce", "af_dual_branch_encoders"):
        monkeypatch.setattr(_lib.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    rng = np.random.default_rng(0)
    lmk, au = gen_track(rng, 20)
    with pytest.raises(ValueError, match="467"):
        DV.DualTrack(lmk[:, :466], au, "0")
    with pytest.raises(ValueError, match="au_dim"):
        DV.DualVideoScorer(s["net"]).score([[DV.DualTrack(lmk, au[:, :11], "0")]])
    with pytest.raises(ValueError, match="au_dim"):
        DV.DualVideoScorer(s["net"], use_delta2=False).score([[DV.DualTrack(lmk, au, "0")]])
    for clips in ([(0, 17)], [(0, 0)], [(15, 8)], [(-1, 4)]):
        with pytest.raises(ValueError):
            DV.DualTrack(lmk, au, "0", clips=clips)
    for T in (0, 17):
        with pytest.raises(ValueError):
            DV.DualVideoScorer(s["net"], T=T)
    with pytest.raises(ValueError, match="stats"):
        DV.DualVideoScorer(s["net"], zscore_mode="global")
    with pytest.raises(ValueError):
        DV.DualVideoScorer(s["net"], zscore_mode="global", stats={"au_mean": np.zeros(35), "au_std": np.ones(36), "lmk_mean": np.zeros(132),
                                                                 "lmk_std": np.ones(132)})
    rgb = dualrun.DualEncoderRGB(36, 132, 2048, ff_dim=3.0)
    with pytest.raises(ValueError, match="V"):
        DV.DualVideoScorer(rgb)
    with pytest.raises(ValueError):
        DV.DualVideoScorer(s["net"], agg_mode="track_max")
    with pytest.raises(ValueError):
        DV.DualTrack(torch.from_numpy(lmk), torch.from_numpy(au), "0")                  # host tensors: numpy is the host form
    assert not launched
