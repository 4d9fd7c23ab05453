"""The statement of the dualrun video path in numpy: what ``af_dual_clip_features`` and ``af_dual_video_reduce`` (csrc/af_dual_video.hip)
compute, in a fixed arithmetic order, so that the kernels can equal it bit for bit.  tests/test_dualvideo_host.py pins it against what
the reference's own functions returned (tests/golden/dual_video.*); DESIGN 21 has the reasons for the order.

Every value is np.float32 unless said otherwise, and every operation below is one rounding:
  scale   = sqrt(fl(dx * dx) + fl(dy * dy)),  dx, dy = mouth left - mouth right;  a frame is dropped when scale is not finite or
            < float32(1e-8); the divisor is scale + float32(1e-6) (numpy >= 2 keeps that sum in fp32; numpy 1.x made it fp64)
  lmk     = (point - nose) / divisor
  au      = X | X[r] - X[r-1] | d1[r] - d1[r-1], row 0 of a difference being the row minus itself
  fixT    = the centred T rows, or the rows and then the last one repeated
  clip    : mean = (((0 + x0) + x1) + ...) / T;  std = sqrt((((0 + d0 d0) + d1 d1) + ...) / (T - 1)), d = x - mean;  floor 1e-6
  global  : (x - mean) / floor(floor(std));  nan_to_num in both modes on both modalities;  none: untouched
The reduction: sigmoid(x) = float32(1 / (1 + exp(-float64(x)))); medians pick elements (torch.median: the lower middle; np.median:
the fp64 midpoint), means are sequential sums in input order (fp32 for the fusion family, fp64 for best.py's)."""
import numpy as np

F32 = np.float32
KEY_IDX = (33, 7, 163, 144, 145, 153, 154, 155, 133, 173, 157, 158, 159, 160, 161, 246, 70, 63, 105, 66, 107, 55, 65, 52, 53, 46,
           263, 249, 390, 373, 374, 380, 381, 382, 362, 398, 384, 385, 386, 387, 388, 466, 300, 293, 334, 296, 336, 285, 295, 282, 283, 276,
           61, 146, 91, 181, 84, 17, 314, 405, 321, 375, 291, 1, 78, 308)
NOSE, ML, MR = 1, 78, 308
LMK_DIM = 2 * len(KEY_IDX)


def lmk_rows(lmk):
    """(n, P, 2) raw landmarks -> ((nvalid, 132) features of the surviving frames, nvalid)"""
    lmk = np.asarray(lmk, dtype=F32)
    rows = []
    with np.errstate(all="ignore"):
        for xy in lmk:
            d = xy[ML] - xy[MR]
            scale = np.sqrt(F32(d[0] * d[0]) + F32(d[1] * d[1]), dtype=F32)
            if not np.isfinite(scale) or scale < F32(1e-8):
                continue
            div = F32(scale + F32(1e-6))
            rows.append(((xy[list(KEY_IDX)] - xy[NOSE]) / div).astype(F32).reshape(-1))
    return (np.stack(rows) if rows else np.zeros((0, LMK_DIM), F32)), len(rows)


def au_rows(aus, use_delta=True, use_delta2=True):
    """(n, K) raw AUs -> (n, K * (1 + delta + delta2))"""
    X = np.asarray(aus, dtype=F32)
    with np.errstate(all="ignore"):
        d1 = X - np.concatenate([X[:1], X[:-1]])
        d2 = d1 - np.concatenate([d1[:1], d1[:-1]])
    return np.concatenate([X] + ([d1] if use_delta else []) + ([d2] if use_delta2 else []), axis=1).astype(F32)


def fix_t(x, T):
    n = x.shape[0]
    if n == T:
        return x
    if n > T:
        s = (n - T) // 2
        return x[s:s + T]
    return np.concatenate([x, np.repeat(x[-1:], T - n, axis=0)])


def _floor(s):
    return np.where(s < F32(1e-6), F32(1e-6), s).astype(F32)           # keeps NaN, like clamp_min and np.maximum


def nan_to_num(x):
    big = np.finfo(F32).max
    return np.where(np.isnan(x), F32(0), np.where(x == np.inf, big, np.where(x == -np.inf, -big, x))).astype(F32)


def zscore_clip(x):
    """(T, D) -> (x - mean) / max(std, 1e-6) in the fixed order (not yet nan_to_num'd)"""
    T = x.shape[0]
    with np.errstate(all="ignore"):
        s = np.zeros(x.shape[1], F32)
        for t in range(T):
            s = (s + x[t]).astype(F32)
        mu = (s / F32(T)).astype(F32)
        ss = np.zeros(x.shape[1], F32)
        for t in range(T):
            d = (x[t] - mu).astype(F32)
            ss = (ss + (d * d).astype(F32)).astype(F32)
        sd = _floor(np.sqrt((ss / F32(T - 1)).astype(F32), dtype=F32))
        return ((x - mu) / sd).astype(F32)


def normalize(au, lmk, mode="clip", apply="both", stats=None):
    if mode == "none":
        return au, lmk
    if mode == "global":
        assert stats is not None
        with np.errstate(all="ignore"):
            if apply in ("both", "au"):
                au = ((au - np.asarray(stats["au_mean"], F32)) / _floor(_floor(np.asarray(stats["au_std"], F32)))).astype(F32)
            if apply in ("both", "lmk"):
                lmk = ((lmk - np.asarray(stats["lmk_mean"], F32)) / _floor(_floor(np.asarray(stats["lmk_std"], F32)))).astype(F32)
        return nan_to_num(au), nan_to_num(lmk)
    assert mode == "clip"
    if apply in ("both", "au"):
        au = zscore_clip(au)
    if apply in ("both", "lmk"):
        lmk = zscore_clip(lmk)
    return nan_to_num(au), nan_to_num(lmk)


def clip_features(lmk, aus, T=8, mode="clip", apply="both", stats=None, use_delta=True, use_delta2=True):
    """one clip's raw rows -> (A (T, F_au), L (T, 132), nvalid); a clip with no landmark row left is zeros"""
    L, nv = lmk_rows(lmk)
    A = au_rows(aus, use_delta, use_delta2)
    if nv == 0:
        return np.zeros((T, A.shape[1]), F32), np.zeros((T, LMK_DIM), F32), 0
    A, L = normalize(fix_t(A, T), fix_t(L, T), mode, apply, stats)
    return A, L, nv


def features(tracks, clips, **kw):
    """tracks: [(lmk (n, P, 2), aus (n, K))]; clips: [(track, first, len)] -> A (C, T, F), L (C, T, 132), nvalid (C,) int32"""
    out = [clip_features(tracks[t][0][f:f + n], tracks[t][1][f:f + n], **kw) for t, f, n in clips]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.asarray([o[2] for o in out], np.int32))


# ---- the reduction -----------------------------------------------------------------------------------------------------------------

def sigmoid(x):
    with np.errstate(all="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))).astype(F32)


def _seq_sum(values, dtype):
    s = dtype(0)
    with np.errstate(all="ignore"):
        for v in values:
            s = dtype(s + dtype(v))
    return s


def lower_median(values):
    """torch.median of a 1-d fp32 tensor: the lower of the two middle values; NaN if any"""
    v = np.asarray(values, F32)
    if np.isnan(v).any():
        return F32(np.nan)
    return np.sort(v, kind="stable")[(len(v) - 1) // 2]


def mid_median(values):
    """np.median of fp64 values"""
    v = np.asarray(values, np.float64)
    if np.isnan(v).any():
        return np.float64(np.nan)
    s = np.sort(v, kind="stable")
    lo, hi = s[(len(v) - 1) // 2], s[len(v) // 2]
    with np.errstate(all="ignore"):
        return lo if len(v) % 2 else np.float64((lo + hi) / 2.0)


def reduce_fusion(logits, nvalid, videos, track_mode="median", video_mode="max"):
    """videos: [[clip numbers of track 0], [of track 1], ...] per video, tracks already in person_key_order.
    -> per video {"track_logit": [...] (NaN for a track left empty), "track_count", "video_logit", "video_prob"}"""
    out = []
    for tracks in videos:
        tl, tc = [], []
        for clips in tracks:
            vals = [F32(logits[c]) for c in clips if nvalid[c] > 0]
            tc.append(len(vals))
            if not vals:
                tl.append(F32(np.nan))
            elif track_mode == "median":
                tl.append(lower_median(vals))
            else:
                with np.errstate(all="ignore"):
                    tl.append(F32(_seq_sum(vals, F32) / F32(len(vals))))
        kept = [z for z, n in zip(tl, tc) if n]
        if not kept:
            z = F32(np.nan)
        elif video_mode == "median":
            z = lower_median(kept)
        elif video_mode == "mean":
            with np.errstate(all="ignore"):
                z = F32(_seq_sum(kept, F32) / F32(len(kept)))
        else:
            z = F32(np.nan) if np.isnan(kept).any() else np.max(np.asarray(kept, F32))
        out.append({"track_logit": np.asarray(tl, F32), "track_prob": sigmoid(np.asarray(tl, F32)), "track_count": np.asarray(tc, np.int32),
                    "video_logit": F32(z), "video_prob": sigmoid(z)})
    return out


def best_aggregate(probs, nvalid, videos, agg_mode="track_mean", thresh=0.5):
    """best.py's aggregation on clip probabilities (fp32 values, used as fp64 like ``float(y_score_clip[i])``)"""
    out = []
    for tracks in videos:
        ts, tp, tc = [], [], []
        for clips in tracks:
            p = [np.float64(F32(probs[c])) for c in clips if nvalid[c] > 0]
            tc.append(len(p))
            if not p:
                ts.append(np.float64(0.0)), tp.append(0)
                continue
            with np.errstate(all="ignore"):
                mean = np.float64(_seq_sum(p, np.float64) / np.float64(len(p)))
            if agg_mode == "track_mean":
                score, pred = mean, int(mean >= thresh)
            elif agg_mode == "track_median":
                score = mid_median(p)
                pred = int(score >= thresh)
            else:
                fake = sum(1 for v in p if v >= thresh)
                score, pred = mean, int(np.float64(fake) / np.float64(len(p)) >= 0.5)
            ts.append(score), tp.append(pred)
        kept = [(s, q) for s, q, n in zip(ts, tp, tc) if n]
        top = 0.0
        for i, (s, _) in enumerate(kept):
            if i == 0 or s > top:
                top = s
        out.append({"track_score": np.asarray(ts, np.float64), "track_pred": np.asarray(tp, np.int32), "track_count": np.asarray(tc, np.int32),
                    "video_score": np.float64(top), "video_pred": int(any(q == 1 for _, q in kept))})
    return out


def reduce_best(logits, nvalid, videos, agg_mode="track_mean", thresh=0.5):
    return best_aggregate(sigmoid(logits), nvalid, videos, agg_mode, thresh)
