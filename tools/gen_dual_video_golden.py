"""Writes tests/golden/dual_video.npz + .json: seeded raw landmark / AU tracks of three small videos and what the REFERENCE's own
functions make of them - ``_seq_to_features`` (dualrun/data/make_lmk_features.py), ``seq_au_to_features`` and ``infer_au_order``
(data/make_au_features.py), ``VideoDataset._fixT``, ``normalize_features``, ``track_reduce``, ``agg_video``,
``get_person_id_from_path``, ``sigmoid_to_logit`` (rgb/fusion.py) and ``aggregate_video_predictions`` (cli/best.py).

    python tools/gen_dual_video_golden.py [--reference DIR]

The reference files are loaded by path (oracle/ref_import.py names the tree).  ``cv2`` and ``mediapipe``, which
make_lmk_features.py imports at the top and which are not installed where this runs, are stand-ins by name; nothing on the paths
run here touches them.  tests/dualvideo_ref.py (the numpy statement the kernels equal) is measured against the recorded features
here, and the figure goes into the json: tests/test_dualvideo_host.py asserts at 8 x it.

Asserted before anything is written: every feature column of every clip has a reference std >= 1e-3 over its 8 rows, except the
nose point's two columns (exactly 0 everywhere) and the AU columns of ONE clip, whose 8 AU rows are identical (held by
``last_known_data``); every track has fewer than 8 clips, so numpy's mean of the clip probabilities is a plain sequential sum."""
import argparse
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, _p))
sys.path.insert(0, ROOT)
import dualvideo_ref as R              # noqa: E402

P, K, T = 478, 12, 8
AU_NAMES = ["AU%02d" % i for i in (1, 2, 4, 6, 7, 10, 12, 14, 15, 17, 23, 24)]
VIDEOS = [("vid_a", [("10", 12), ("2", 20), ("track_1", 29), ("2b", 8)]),
          ("vid_b", [("0", 16), ("1", 35)]),
          ("vid_c", [("id_3", 11)])]
HELD = (0, 2, 8)                        # video, track, first frame: AU rows first .. first + 7 are one held row
SAME_MOUTH = (0, 1, 9)                  # ml == mr on this frame: dropped (scale 0)
NAN_MOUTH = (1, 1, 17)                  # NaN in ml: dropped (scale not finite)


def load_reference(reference):
    dual = os.path.join(reference, "dualrun")
    for name in ("cv2", "mediapipe"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, dual)

    def by_path(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(dual, *parts))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    lmk = by_path("make_lmk_features", "data", "make_lmk_features.py")
    au = by_path("make_au_features", "data", "make_au_features.py")
    fusion = by_path("ref_fusion", "rgb", "fusion.py")
    best = by_path("ref_best", "cli", "best.py")
    return lmk, au, fusion, best


def draw_inputs():
    rng = np.random.default_rng(20240611)
    q = lambda x, bits: (np.round(np.asarray(x) * (1 << bits)) / (1 << bits)).astype(np.float32)       # noqa: E731
    videos = []
    for vi, (_, tracks) in enumerate(VIDEOS):
        out = []
        for ti, (key, n) in enumerate(tracks):
            base = rng.uniform(0.2, 0.8, (P, 2))
            base[R.NOSE], base[R.ML], base[R.MR] = (0.5, 0.55), (0.4, 0.7), (0.6, 0.7)
            walk = np.cumsum(rng.normal(0, 0.004, (n, 1, 2)), axis=0)
            lmk = q(base[None] + walk + rng.normal(0, 0.01, (n, P, 2)), 14)
            aus = q(rng.uniform(0, 1, (n, K)), 10)
            if (vi, ti) == HELD[:2]:
                aus[HELD[2]:HELD[2] + T] = aus[HELD[2]]
            if (vi, ti) == SAME_MOUTH[:2]:
                lmk[SAME_MOUTH[2], R.MR] = lmk[SAME_MOUTH[2], R.ML]
            if (vi, ti) == NAN_MOUTH[:2]:
                lmk[NAN_MOUTH[2], R.ML, 0] = np.nan
            out.append((key, lmk, aus))
        videos.append(out)
    return videos


def write_npz(path, arrays):
    """an .npz whose bytes depend on the arrays alone (np.savez stamps each member with the time of day)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dual_video"))
    opt = ap.parse_args()
    if opt.reference is None:
        import ref_import
        opt.reference = ref_import.REFERENCE_ROOT
    LM, AU, FU, BE = load_reference(opt.reference)
    from af_mi355x import dual_video as DV

    videos = draw_inputs()
    arrays, doc_videos = {}, []
    stats_rng = np.random.default_rng(77)
    stats = {"au_mean": stats_rng.normal(0.3, 0.2, 3 * K).astype(np.float32), "au_std": stats_rng.uniform(0.1, 0.5, 3 * K).astype(np.float32),
             "lmk_mean": stats_rng.normal(0, 0.5, R.LMK_DIM).astype(np.float32), "lmk_std": stats_rng.uniform(0.2, 1.5, R.LMK_DIM).astype(np.float32)}
    stats["au_std"][5] = np.float32(1e-9)                              # under the floor
    for k, v in stats.items():
        arrays["stats_" + k] = v
    # load_norm_stats floors the stds once (fusion.py:74-76); normalize_features clamps again
    ref_stats = {"au_mean": stats["au_mean"], "au_std": np.maximum(stats["au_std"], 1e-6), "lmk_mean": stats["lmk_mean"],
                 "lmk_std": np.maximum(stats["lmk_std"], 1e-6)}

    feats = {k: [] for k in ("A_none", "L_none", "A_global", "A_clip", "L_clip")}
    nvalid, clip_keys, clip_video, clip_paths, held_clip = [], [], [], [], None
    for vi, tracks in enumerate(videos):
        doc_tracks = []
        for ti, (key, lmk, aus) in enumerate(tracks):
            arrays["v%d_t%d_lmk" % (vi, ti)], arrays["v%d_t%d_au" % (vi, ti)] = lmk, aus
            starts = DV.clip_windows(len(lmk))
            assert 1 <= len(starts) < 8
            doc_tracks.append({"key": key, "n": int(len(lmk)), "clips": starts})
            for ci, s in enumerate(starts):
                path = "/data/Deepfakes/%s/%s/clip_%03d" % (VIDEOS[vi][0], key, ci)
                assert FU.get_person_id_from_path(path) == key
                F_l, _ = LM._seq_to_features([f for f in lmk[s:s + T]], rot_invariant=False)
                seq = [{n: float(v) for n, v in zip(AU_NAMES, row)} for row in aus[s:s + T]]
                order = AU.infer_au_order(seq)
                assert order == AU_NAMES
                F_a = AU.seq_au_to_features(seq, order, True, True)
                a = FU.VideoDataset._fixT(torch.from_numpy(np.asarray(F_a, np.float32)), T)
                l = FU.VideoDataset._fixT(torch.from_numpy(np.asarray(F_l, np.float32)), T)
                for mode, st in (("none", None), ("global", ref_stats), ("clip", None)):
                    ra, rl = FU.normalize_features(a, l, st, mode=mode, apply="both")
                    feats["A_" + mode].append(ra.numpy())
                    if mode != "global":
                        feats["L_" + mode].append(rl.numpy())
                if (vi, ti, s) == HELD:
                    held_clip = len(nvalid)
                nvalid.append(F_l.shape[0])
                clip_keys.append(key), clip_video.append(vi), clip_paths.append(path)
        doc_videos.append({"name": VIDEOS[vi][0], "tracks": doc_tracks})
    for k in feats:
        arrays["ref_" + k] = np.stack(feats[k]).astype(np.float32)
    nvalid = np.asarray(nvalid, np.int32)
    arrays["ref_nvalid"] = nvalid
    n_clips = len(nvalid)
    assert held_clip is not None and (nvalid < T).sum() >= 3 and nvalid.min() >= 1

    # which columns are degenerate: the nose's two everywhere, the held clip's AU columns, nothing else
    nose_cols = [2 * R.KEY_IDX.index(R.NOSE), 2 * R.KEY_IDX.index(R.NOSE) + 1]
    sd_l = arrays["ref_L_none"].std(axis=1, ddof=1)
    sd_a = arrays["ref_A_none"].std(axis=1, ddof=1)
    assert (arrays["ref_L_none"][:, :, nose_cols] == 0).all() and (arrays["ref_L_clip"][:, :, nose_cols] == 0).all()
    ok_l = np.ones(R.LMK_DIM, bool)
    ok_l[nose_cols] = False
    assert (sd_l[:, ok_l] >= 1e-3).all(), "a landmark column is degenerate"
    deg = [c for c in range(n_clips) if (sd_a[c] < 1e-3).any()]
    assert deg == [held_clip] and (sd_a[held_clip] == 0).all(), deg

    # the statement against the reference's figures
    tracks_flat, clips_flat = [], []
    for vi, tracks in enumerate(videos):
        for ti, (key, lmk, aus) in enumerate(tracks):
            clips_flat += [(len(tracks_flat), s, T) for s in doc_videos[vi]["tracks"][ti]["clips"]]
            tracks_flat.append((lmk, aus))
    sA, sL, snv = R.features(tracks_flat, clips_flat, T=T, mode="none")
    assert np.array_equal(snv, nvalid) and np.array_equal(sA, arrays["ref_A_none"])
    gA, _, _ = R.features(tracks_flat, clips_flat, T=T, mode="global", stats=stats)
    assert np.array_equal(gA, arrays["ref_A_global"])
    cA, cL, _ = R.features(tracks_flat, clips_flat, T=T, mode="clip")
    keep = np.asarray([c != held_clip for c in range(n_clips)])
    d_lmk = float(np.abs(sL - arrays["ref_L_none"]).max())
    d_clip = float(max(np.abs(cL - arrays["ref_L_clip"]).max(), np.abs(cA[keep] - arrays["ref_A_clip"][keep]).max()))

    # the reductions on seeded clip logits with ties and repeats
    rng = np.random.default_rng(5)
    logits = rng.normal(0, 2, n_clips).astype(np.float32)
    logits[1] = logits[0]                                              # a tie inside a track of 2
    logits[3], logits[5] = logits[2], logits[4]                        # repeats inside a track of 4
    arrays["red_logits"] = logits
    probs = torch.sigmoid(torch.from_numpy(logits)).numpy()
    arrays["red_probs"] = probs
    fusion = {}
    for tm in ("median", "mean"):
        for vm in ("max", "median", "mean"):
            per_video = []
            for vi in range(len(videos)):
                idx = [c for c in range(n_clips) if clip_video[c] == vi]
                ld = torch.from_numpy(logits[idx]).view(-1, 1)
                tr = FU.track_reduce(ld, [clip_keys[c] for c in idx], mode=tm)
                vid = FU.agg_video(tr, vm)
                per_video.append({"track_logit": [float(x) for x in tr.view(-1)], "video_logit": float(vid.item()),
                                  "video_prob": float(torch.sigmoid(vid).item())})
            fusion["%s/%s" % (tm, vm)] = per_video
    best = {}
    for mode in ("track_mean", "track_median", "track_majority"):
        meta = [(clip_paths[c], VIDEOS[clip_video[c]][0], clip_keys[c]) for c in range(n_clips)]
        vids, _ = BE.aggregate_video_predictions(clip_paths, {p: "Deepfakes" for p in clip_paths}, meta, np.zeros(n_clips, int), probs, 0.5, mode)
        best[mode] = [{"tracks": {k: {"track_score": float(t["track_score"]), "track_pred": int(t["track_pred"]), "probs": [float(x) for x in t["probs"]]}
                                  for k, t in vids["Deepfakes::" + name]["tracks"].items()},
                       "video_score": float(vids["Deepfakes::" + name]["video_score"]), "video_pred": int(vids["Deepfakes::" + name]["video_pred"])}
                      for name, _ in VIDEOS]
    med = [len(t["clips"]) for v in doc_videos for t in v["tracks"]]
    assert any(n % 2 == 0 and n >= 2 for n in med)
    p_rgb = [0.0, 1e-7, 0.25, 0.5, 0.9731, 1.0]
    doc = {"what": "seeded dualrun tracks and the reference's own results on them (tools/gen_dual_video_golden.py)",
           "numpy": np.__version__, "torch": torch.__version__.split("+")[0], "P": P, "K": K, "T": T, "videos": doc_videos,
           "clip_keys": clip_keys, "clip_video": clip_video, "held_clip": held_clip, "nose_cols": nose_cols,
           "measured": {"lmk_before_zscore": d_lmk, "clip_mode": d_clip, "tolerance_basis": max(d_lmk, d_clip)},
           "fusion": fusion, "best": best, "prob_thresh": 0.5,
           "sigmoid_to_logit": [[p, FU.sigmoid_to_logit(p)] for p in p_rgb]}
    write_npz(opt.out + ".npz", arrays)
    with open(opt.out + ".json", "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote %s.npz (%d bytes) and .json; %d clips, nvalid %s, held clip %d; max |statement - reference|: lmk %.3g, clip mode %.3g"
          % (opt.out, os.path.getsize(opt.out + ".npz"), n_clips, nvalid.tolist(), held_clip, d_lmk, d_clip))


if __name__ == "__main__":
    main()
