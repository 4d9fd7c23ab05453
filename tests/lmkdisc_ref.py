"""The statement of cli/test.py's LMKDisc path in numpy: what ``af_dual_clip_features_ex`` and ``af_lmk_video_reduce``
(csrc/af_dual_video.hip) compute beyond tests/dualvideo_ref.py, in a fixed arithmetic order, so that the kernels can equal it bit for
bit.  tests/test_lmkdisc_host.py pins it against what the reference's own functions returned (tests/golden/lmk_disc.*).

The mouth-line rotation (make_lmk_features.py:145-150, 173-176), fp32 unless said otherwise, every operation one rounding:
  ml_c, mr_c = (ml - nose) / div, (mr - nose) / div,  div = scale + float32(1e-6)
  dx, dy     = mr_c - ml_c
  c, s       = float32(dx / h), float32(-dy / h),  h = sqrt(dx dx + dy dy), all in fp64 (the products are exact there)
               THIS is the definition of cos(-atan2(dy, dx)) and sin(-atan2(dy, dx)) here: divide and square root are correctly
               rounded on every machine, libm's trigonometry is not.  dx = dy = 0 (atan2(0, 0) = 0): c = 1, s = 0.
  x', y'     = fl(fl(x c) + fl(y (-s))),  fl(fl(x s) + fl(y c))       (points @ R.T with R = [[c, -s], [s, c]], sequentially)
Padding (data/vox_ds.py:19-26): the surviving rows, then T - nvalid rows of +0.0.
The reduction (cli/test.py:86-94, 205-212): clip_score = float64(sigmoid) or 1.0 - it; ``median_by_key`` and ``noisy_or`` with
test.py's own numpy calls."""
import numpy as np

import dualvideo_ref as R

F32 = np.float32
PT_NOSE, PT_ML, PT_MR = (R.KEY_IDX.index(i) for i in (R.NOSE, R.ML, R.MR))      # rows of the 66-point key set


def rotation(dx, dy):
    """(c, s) as fp32 for fp32 dx, dy"""
    dx, dy = F32(dx), F32(dy)
    if dx == 0 and dy == 0:
        return F32(1), F32(0)
    with np.errstate(all="ignore"):
        x, y = np.float64(dx), np.float64(dy)
        h = np.sqrt(x * x + y * y)
        return F32(x / h), F32(-y / h)


def rotate_row(row):
    """one (132,) normalised row -> the row turned so that its mouth line is horizontal"""
    pts = np.asarray(row, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        d = (pts[PT_MR] - pts[PT_ML]).astype(F32)
        c, s = rotation(d[0], d[1])
        x, y = pts[:, 0], pts[:, 1]
        xr = ((x * c).astype(F32) + (y * F32(-s)).astype(F32)).astype(F32)
        yr = ((x * s).astype(F32) + (y * c).astype(F32)).astype(F32)
    return np.stack([xr, yr], axis=1).reshape(-1)


def lmk_rows(lmk, rot_invariant=False):
    """(n, P, 2) raw landmarks -> ((nvalid, 132) features of the surviving frames, nvalid)"""
    rows, nv = R.lmk_rows(lmk)
    if rot_invariant and nv:
        rows = np.stack([rotate_row(r) for r in rows])
    return rows, nv


def zero_pad(rows, T):
    """collate_pad for a batch whose longest clip has T rows"""
    assert rows.shape[0] <= T
    out = np.zeros((T, rows.shape[1]), F32)
    out[:rows.shape[0]] = rows
    return out


def clip_features(lmk, T=8, rot_invariant=False, pad="zero", mode="none", stats=None):
    """one clip's raw rows -> (L (T, 132), nvalid).  pad "zero": test.py's form (a clip longer than T is a bad record: zeros, 0);
    pad "fixT": fixT and normalize_features on the rotated rows, DualVideoScorer's landmark half"""
    rows, nv = lmk_rows(lmk, rot_invariant)
    if nv == 0 or (pad == "zero" and len(lmk) > T):
        return np.zeros((T, R.LMK_DIM), F32), 0
    if pad == "zero":
        assert mode == "none"
        return zero_pad(rows, T), nv
    dummy = np.zeros((T, 1), F32)
    return R.normalize(dummy, R.fix_t(rows, T), mode, "lmk" if mode != "none" else "both", stats)[1], nv


def features(tracks, clips, **kw):
    """tracks: [lmk (n, P, 2)]; clips: [(track, first, len)] -> L (C, T, 132), nvalid (C,) int32"""
    out = [clip_features(tracks[t][f:f + n], **kw) for t, f, n in clips]
    return np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], np.int32)


# ---- the reduction -----------------------------------------------------------------------------------------------------------------

def clip_score(logits, invert=False):
    """fp64: float(sigmoid) as test.py:205-206 hands it on, 1.0 - it with --invert (:211-212)"""
    s = R.sigmoid(logits).astype(np.float64)
    return 1.0 - s if invert else s


def median_by_key(values, keys):
    bins = {}
    for k, v in zip(keys, values):
        bins.setdefault(k, []).append(float(v))
    return {k: float(np.median(vs)) for k, vs in bins.items()}


def noisy_or(p_tracks):
    p = np.clip(np.asarray(p_tracks, np.float64), 1e-6, 1 - 1e-6)
    return float(1.0 - np.exp(np.log1p(-p).sum()))


def reduce_lmk(logits, nvalid, videos, invert=False, thresh=0.5):
    """videos: [[clip numbers of track 0], [of track 1], ...] per video (every track its own key).  -> (clip_score (C,) fp64,
    per video {"track_score", "track_pred", "track_count" per track - 0.0 / 0 / 0 for a track left empty -, "video_score",
    "video_pred", "n_tracks"})"""
    score = clip_score(logits, invert)
    out = []
    for tracks in videos:
        ts, tp, tc = [], [], []
        for clips in tracks:
            used = [c for c in clips if nvalid[c] > 0]
            tc.append(len(used))
            med = median_by_key([score[c] for c in used], ["t"] * len(used)).get("t", 0.0)
            ts.append(med), tp.append(int(bool(used) and med >= thresh))
        p = noisy_or([s for s, n in zip(ts, tc) if n])
        out.append({"track_score": np.asarray(ts, np.float64), "track_pred": np.asarray(tp, np.int32), "track_count": np.asarray(tc, np.int32),
                    "video_score": np.float64(p), "video_pred": int(p >= thresh), "n_tracks": int(sum(1 for n in tc if n))})
    return score, out
