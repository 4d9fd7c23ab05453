"""The statement of ``af_mi355x.eval_suite``: the reference's evaluation protocol (altfreezing/ds.py), its threshold picker
(dualrun/train/thresholds.py) and the summary figures of altfreezing/TEST2.py:1115-1137, in numpy alone (no sklearn).

The two threshold-free metrics are stated on integers.  For a pool ``(y, s)``: ``order = argsort(-s, kind="stable")``; ``rank_of_item``
is each item's position in it, ``group_of_rank`` the tie-group id along the sorted scores (equal scores share a group) and
``label_of_rank`` the label along them.  For an index row ``idx`` (any length, repeats allowed):

    cnt[r]        draws of rank r
    pos_g, neg_g  per-group sums of cnt, by label;  tp_g, fp_g their inclusive prefix sums;  P, N the totals
    U2     = sum_g pos_g (2 (N - fp_g) + neg_g)                an exact integer; AUROC = U2 / (2 P N), ONE fp64 division
    ap_sum = sum_g pos_g (tp_g / (tp_g + fp_g))                fp64; groups with pos_g == 0 contribute exactly 0 and are never
                                                               divided (leading groups nobody drew have tp + fp == 0); AP = ap_sum / P

The order of ``ap_sum`` is part of the statement, because csrc/af_eval.hip follows it: the ranks are dealt to ``THREADS`` threads in
contiguous chunks of ``ceil(n / THREADS)``; a group's term belongs to the thread that owns the group's LAST rank; a thread adds its
terms in rank order, from 0.0; the ``THREADS`` partial sums are then folded by the tree ``p[i] += p[i + h]`` for h = THREADS / 2 .. 1.
A product and a quotient are rounded once each, nothing is contracted.  (Adding the 0.0 of a skipped group changes no bit of a
non-negative sum, so the vectorised form below adds zeros where the kernel adds nothing.)

For a threshold tau: ``cut`` = pool items with ``s >= tau``; ``tp_cut`` / ``fp_cut`` = the draws of rank < cut, by label.
"""
import csv
import json
import os

import numpy as np

THREADS = 256                # the kernel's workgroup size: part of the order of ap_sum
MAX_POOL = 16384             # the kernel's counts live in LDS


# ---- the pool and the rows --------------------------------------------------------------------------------------------------------------

def make_pool(y, s):
    y, s = np.asarray(y), np.asarray(s, np.float64)
    if y.ndim != 1 or y.shape != s.shape or y.size == 0:
        raise ValueError("a pool is two equal, non-empty vectors (labels %s, scores %s)" % (y.shape, s.shape))
    if not np.isfinite(s).all():
        raise ValueError("a pool's scores are finite")
    n = y.size
    order = np.argsort(-s, kind="stable")
    rank_of_item = np.empty(n, np.int32)
    rank_of_item[order] = np.arange(n, dtype=np.int32)
    ss = s[order]
    group_of_rank = np.concatenate([[0], np.cumsum(ss[1:] != ss[:-1])]).astype(np.int32)
    label_of_rank = (y[order] == 1).astype(np.uint8)
    return {"n": n, "y": (y == 1).astype(np.int64), "s": s, "order": order, "rank_of_item": rank_of_item, "group_of_rank": group_of_rank,
            "label_of_rank": label_of_rank, "sorted_scores": ss, "groups": int(group_of_rank[-1]) + 1}


def cut_of(pool, threshold):
    return 0 if threshold is None else int(np.count_nonzero(pool["s"] >= threshold))


def flatten_rows(rows):
    """a list of index arrays -> (flat int64, row_off int64[rows + 1])"""
    rows = [np.asarray(r).astype(np.int64, copy=False).ravel() for r in rows]
    off = np.zeros(len(rows) + 1, np.int64)
    if rows:
        off[1:] = np.cumsum([r.size for r in rows])
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)), off


def rank_rows(pool, rows, cut=0):
    """the integers and ap_sum of every row, in the stated order -> dict of arrays: u2, ap_sum, P, N, tp_cut, fp_cut"""
    n = pool["n"]
    flat, off = flatten_rows(rows)
    R = len(off) - 1
    if flat.size and (flat.min() < 0 or flat.max() >= n):
        raise ValueError("an index outside the pool of %d" % n)
    row_id = np.repeat(np.arange(R), np.diff(off))
    cnt = np.bincount(row_id * n + pool["rank_of_item"][flat], minlength=R * n).reshape(R, n).astype(np.int64)
    lab = pool["label_of_rank"].astype(bool)
    tp = np.cumsum(cnt * lab, axis=1)
    fp = np.cumsum(cnt * ~lab, axis=1)
    P, N = tp[:, -1], fp[:, -1]
    g = pool["group_of_rank"]
    ends = np.flatnonzero(np.concatenate([g[1:] != g[:-1], [True]]))          # a group's last rank
    tp_g, fp_g = tp[:, ends], fp[:, ends]
    pos_g = np.diff(tp_g, axis=1, prepend=0)
    neg_g = np.diff(fp_g, axis=1, prepend=0)
    u2 = (pos_g * (2 * (N[:, None] - fp_g) + neg_g)).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        term = np.where(pos_g > 0, pos_g.astype(np.float64) * (tp_g.astype(np.float64) / (tp_g + fp_g).astype(np.float64)), 0.0)
    chunk = -(-n // THREADS)
    at = np.zeros((R, THREADS * chunk), np.float64)
    at[:, ends] = term
    at = at.reshape(R, THREADS, chunk)
    part = np.zeros((R, THREADS), np.float64)
    for j in range(chunk):                                                    # a thread's terms, in rank order
        part = part + at[:, :, j]
    h = THREADS // 2
    while h >= 1:                                                             # the tree over threads
        part = part[:, :h] + part[:, h:2 * h]
        h //= 2
    tp_cut = tp[:, cut - 1] if cut > 0 else np.zeros(R, np.int64)
    fp_cut = fp[:, cut - 1] if cut > 0 else np.zeros(R, np.int64)
    return {"u2": u2.astype(np.int64), "ap_sum": part[:, 0], "P": P.astype(np.int32), "N": N.astype(np.int32),
            "tp_cut": tp_cut.astype(np.int32), "fp_cut": fp_cut.astype(np.int32)}


def finish_rows(raw):
    """what the host does behind the launch: the two divisions and the confusion counts -> the dict ``RankMetrics.rows`` returns"""
    P, N = raw["P"].astype(np.int64), raw["N"].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        auc = np.where(P * N > 0, raw["u2"].astype(np.float64) / (2 * P * N).astype(np.float64), np.nan)
        ap = np.where(P > 0, raw["ap_sum"] / P.astype(np.float64), np.nan)
    tp, fp = raw["tp_cut"].astype(np.int64), raw["fp_cut"].astype(np.int64)
    return {"auc": auc, "ap": ap, "P": P, "N": N, "tp": tp, "fp": fp, "tn": N - fp, "fn": P - tp, "u2": raw["u2"], "ap_sum": raw["ap_sum"]}


def rows(pool, rows_, threshold=None):
    return finish_rows(rank_rows(pool, rows_, cut_of(pool, threshold)))


def macro_at(tp, fp, tn, fn):
    """sklearn's precision_score / recall_score / f1_score(average="macro", zero_division=0) from the four counts of a binary problem:
    a class counts when it is in the truth or in the predictions; a 0 / 0 is 0 -> (precision, recall, f1)"""
    tp, fp, tn, fn = int(tp), int(fp), int(tn), int(fn)
    pr, rc, f1 = [], [], []
    for hit, pred, true in ((tn, tn + fn, tn + fp), (tp, tp + fp, tp + fn)):
        if pred + true == 0:
            continue
        pr.append(hit / pred if pred else 0.0)
        rc.append(hit / true if true else 0.0)
        f1.append(2 * hit / (pred + true))
    return float(np.mean(pr)), float(np.mean(rc)), float(np.mean(f1))


# ---- the ROC curve and the threshold picker (dualrun/train/thresholds.py) ------------------------------------------------------------------

def curve_counts(pool):
    """cumulative (tps, fps) at the group ends of the whole pool, every item drawn once"""
    raw_cnt = np.ones(pool["n"], np.int64)
    lab = pool["label_of_rank"].astype(bool)
    g = pool["group_of_rank"]
    ends = np.flatnonzero(np.concatenate([g[1:] != g[:-1], [True]]))
    return np.cumsum(raw_cnt * lab)[ends].astype(np.int32), np.cumsum(raw_cnt * ~lab)[ends].astype(np.int32)


def roc_from_counts(tps, fps, pool):
    """roc_curve(y, s) (drop_intermediate=True) from the integer curve -> (fpr, tpr, thresholds, kept tps, kept fps)"""
    tps, fps = np.asarray(tps, np.int64), np.asarray(fps, np.int64)
    g = pool["group_of_rank"]
    thr = pool["sorted_scores"][np.flatnonzero(np.concatenate([g[1:] != g[:-1], [True]]))]
    if len(fps) > 2:
        keep = np.flatnonzero(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])
        tps, fps, thr = tps[keep], fps[keep], thr[keep]
    tps, fps, thr = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thr]
    with np.errstate(invalid="ignore", divide="ignore"):
        fpr = fps / fps[-1] if fps[-1] > 0 else np.full(len(fps), np.nan)
        tpr = tps / tps[-1] if tps[-1] > 0 else np.full(len(tps), np.nan)
    return fpr, tpr, thr, tps, fps


def roc_curve(pool):
    return roc_from_counts(*curve_counts(pool), pool)[:3]


def stats_from_counts(tp, fp, P, N):
    """_stats_at_threshold from the confusion counts"""
    tp, fp, P, N = int(tp), int(fp), int(P), int(N)
    fn, tn = P - tp, N - fp
    TPR, FPR = tp / max(tp + fn, 1), fp / max(fp + tn, 1)
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return {"tn": tn, "fp": fp, "fn": fn, "tp": tp, "TPR": TPR, "FPR": FPR, "balacc": 0.5 * (TPR + (1.0 - FPR)), "youden": TPR - FPR,
            "acc": (tp + tn) / (P + N), "f1": f1}


def pick_threshold(fpr, tpr, thr, tps, fps, metric="youden", target_fpr=None):
    """threshold_from_roc's choice on a curve -> (best_t, stats)"""
    P, N = int(tps[-1]), int(fps[-1])
    if target_fpr is not None:
        mask = fpr <= float(target_fpr)
        if not np.any(mask):
            idx = int(np.argmin(fpr))
        else:
            idx = int(np.arange(len(fpr))[mask][int(np.argmax(tpr[mask]))])
    elif metric == "youden":
        idx = int(np.argmax(tpr - fpr))
    elif metric == "balacc":
        idx = int(np.argmax(0.5 * (tpr + (1.0 - fpr))))
    elif metric == "auc":
        mask = np.isfinite(thr)
        if not mask.any():
            idx = int(np.argmax(tpr - fpr))
        else:
            idx = int(np.where(mask)[0][int(np.argmin(fpr[mask] ** 2 + (1.0 - tpr[mask]) ** 2))])
    else:
        key = metric if metric in ("acc", "f1") else "youden"
        idx = int(np.argmax([stats_from_counts(a, b, P, N)[key] for a, b in zip(tps, fps)]))
    return float(thr[idx]), stats_from_counts(tps[idx], fps[idx], P, N)


def threshold_from_roc(probs, y, metric="youden", target_fpr=None):
    pool = make_pool(y, probs)
    return pick_threshold(*roc_from_counts(*curve_counts(pool), pool), metric=metric, target_fpr=target_fpr)


# ---- TEST2.main's summary (altfreezing/TEST2.py:1115-1137) --------------------------------------------------------------------------------

def table_from(y_true, y_pred, auc, ap):
    y_true, y_pred = np.asarray(y_true).astype(np.int64), np.asarray(y_pred).astype(np.int64)
    tp, tn = int(((y_true == 1) & (y_pred == 1)).sum()), int(((y_true == 0) & (y_pred == 0)).sum())
    fp, fn = int(((y_true == 0) & (y_pred == 1)).sum()), int(((y_true == 1) & (y_pred == 0)).sum())
    labels = sorted(set(y_true.tolist()) | set(y_pred.tolist()))
    cm = [[int(((y_true == a) & (y_pred == b)).sum()) for b in labels] for a in labels]
    P = tp + fn
    return {"videos": int(y_true.size), "accuracy": (tp + tn) / y_true.size, "auc_roc": float(auc) if 0 < P < y_true.size else float("nan"),
            "pr_auc": float(ap) if P > 0 else 0.0, "f1": 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0,
            "tp": tp, "tn": tn, "fp": fp, "fn": fn, "confusion_matrix": cm}


def video_table(y_true, y_score, threshold, y_pred=None):
    """accuracy, AUROC (NaN when one class), AP, F1 and the confusion matrix; ``y_pred`` None: ``score > threshold``, the rule of
    the runner's per-person label"""
    y_true, y_score = np.asarray(y_true), np.asarray(y_score, np.float64)
    if y_pred is None:
        y_pred = (y_score > threshold).astype(np.int64)
    pool = make_pool(y_true, y_score)
    r = rows(pool, [np.arange(pool["n"])])
    return table_from(y_true, y_pred, r["auc"][0], r["ap"][0])


# ---- altfreezing/ds.py ------------------------------------------------------------------------------------------------------------------

PERF_COLUMNS = ("fps", "latency_ms_clip_mean", "gpu_mem_alloc_peak_mb", "gpu_mem_reserved_peak_mb", "cpu_mem_peak_mb")
PERF_KEYS = ("fps", "latency_ms", "gpu_alloc_mb", "gpu_reserved_mb", "cpu_peak_mb")
FIXED_RATIOS = {"ffpp": 4.0, "celebdf": 1.91, "ffiw": 1.0}
SUMMARY_HEADER = ["dataset", "method", "n_avail_real", "n_avail_fake", "fake_per_real", "runs", "auc_mean", "auc_sd", "auc_ci_lo", "auc_ci_hi",
                  "ap_mean", "ap_sd", "ap_ci_lo", "ap_ci_hi", "f1_macro@tau_mean", "f1_macro@tau_sd", "precision_macro@tau_mean",
                  "precision_macro@tau_sd", "recall_macro@tau_mean", "recall_macro@tau_sd", "fps_mean", "fps_p95", "lat_p50", "lat_mean", "lat_p95",
                  "gpu_alloc_p95", "gpu_reserved_p95", "cpu_peak_p95", "out_dir"]
SEED_HEADER = ["seed", "n_pool", "n_real", "n_fake", "threshold", "auc_mean", "auc_sd", "ap_mean", "ap_sd", "f1_macro@tau_mean", "f1_macro@tau_sd",
               "precision_macro@tau_mean", "precision_macro@tau_sd", "recall_macro@tau_mean", "recall_macro@tau_sd"]


def load_per_video(path):
    with open(path, newline="") as f:
        table = list(csv.DictReader(f))
    if not table:
        raise ValueError("CSV vuoto: %s" % path)
    y_true = np.array([int(d["gt_label"]) for d in table], int)
    y_score = np.array([float(d["video_score"]) for d in table], float)

    def getf(k):
        vals = []
        for d in table:
            try:
                vals.append(float(d[k]))
            except Exception:
                vals.append(np.nan)
        return np.array(vals, float)
    return (y_true, y_score) + tuple(getf(k) for k in PERF_COLUMNS)


def summarize_perf(x):
    x = np.asarray(x, float)
    x = x[np.isfinite(x)]
    if x.size == 0:
        return {"mean": np.nan, "p50": np.nan, "p95": np.nan}
    return {"mean": float(np.mean(x)), "p50": float(np.percentile(x, 50)), "p95": float(np.percentile(x, 95))}


def pick_counts(nR, nF, fake_per_real):
    if fake_per_real <= 0:
        return nR, 0
    rA = min(nR, int(nF / fake_per_real)); fA = int(round(rA * fake_per_real))
    fB = min(nF, int(nR * fake_per_real)); rB = int(round(fB / fake_per_real))
    return (rA, fA) if (rA + fA) >= (rB + fB) else (rB, fB)


def ratio_match_indices(y_true, fake_per_real, rng, frac=1.0):
    real_idx = np.where(y_true == 0)[0]; fake_idx = np.where(y_true == 1)[0]
    if real_idx.size == 0 or fake_idx.size == 0:
        raise ValueError("Classi insufficienti per ratio-matching.")
    nRmax, nFmax = pick_counts(len(real_idx), len(fake_idx), fake_per_real)
    nR = max(1, int(nRmax * frac)); nF = max(1, int(nFmax * frac))
    sel_R = rng.choice(real_idx, size=nR, replace=False)
    sel_F = rng.choice(fake_idx, size=nF, replace=False)
    return np.concatenate([sel_R, sel_F])


def stratified_test_folds(y, seed, n_splits=5):
    """StratifiedKFold(n_splits, shuffle=True, random_state=seed).split(y, y)'s test index sets, in fold order"""
    y = np.asarray(y)
    if n_splits > y.size:
        raise ValueError("Cannot have number of splits n_splits=%d greater than the number of samples: n_samples=%d." % (n_splits, y.size))
    rng = np.random.RandomState(seed)
    _, y_idx, y_inv = np.unique(y, return_index=True, return_inverse=True)
    _, class_perm = np.unique(y_idx, return_inverse=True)
    y_encoded = class_perm[y_inv]                                             # classes by first appearance
    n_classes = len(y_idx)
    if np.all(n_splits > np.bincount(y_encoded)):
        raise ValueError("n_splits=%d cannot be greater than the number of members in each class." % n_splits)
    y_order = np.sort(y_encoded)
    allocation = np.asarray([np.bincount(y_order[i::n_splits], minlength=n_classes) for i in range(n_splits)])
    test_folds = np.empty(len(y), dtype="i")
    for k in range(n_classes):
        folds_for_class = np.arange(n_splits).repeat(allocation[:, k])
        rng.shuffle(folds_for_class)
        test_folds[y_encoded == k] = folds_for_class
    return [np.flatnonzero(test_folds == i) for i in range(n_splits)]


def mean_sd(a):
    x = np.asarray(a, float)
    return float(np.nanmean(x)), float(np.nanstd(x, ddof=1))


def make_config(per_video, dataset, method, fake_per_real, bootstrap=2000, seed=42, outdir="results_suite", threshold=0.04):
    """asdict(EvalConfig(...)), key for key"""
    return {"per_video": per_video, "dataset": dataset, "method": method, "fake_per_real": fake_per_real, "bootstrap": bootstrap, "seed": seed,
            "outdir": outdir, "threshold": threshold, "wandb": False, "wandb_project": None, "wandb_entity": None}


def plan_run(y, s, fake_per_real, seed, bootstrap):
    """the reference's draws, in its order -> (idx_pool, [fold index sets], [bootstrap index rows]); all rows index the POOL"""
    y = np.asarray(y)
    rng = np.random.default_rng(seed)
    idx_pool = ratio_match_indices(y, fake_per_real, rng)
    yt_pool = y[idx_pool]
    folds = stratified_test_folds(yt_pool, seed)
    pos, neg = np.where(yt_pool == 1)[0], np.where(yt_pool == 0)[0]
    boots = [np.concatenate([rng.choice(pos, len(pos), True), rng.choice(neg, len(neg), True)]) for _ in range(bootstrap)]
    return idx_pool, folds, boots


def assemble_run(config, y, idx_pool, n_folds, res, perf=None):
    """run_one's dict from the metrics of the rows (folds first, then the resamples), key for key"""
    y = np.asarray(y)
    yt_pool = y[idx_pool]
    per_fold, precL, recL, f1L = [], [], [], []
    for k in range(n_folds):
        if res["P"][k] == 0 or res["N"][k] == 0:
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        prec, rec, f1m = macro_at(res["tp"][k], res["fp"][k], res["tn"][k], res["fn"][k])
        per_fold.append({"fold": k + 1, "n": int(res["P"][k] + res["N"][k]), "n_real": int(res["N"][k]), "n_fake": int(res["P"][k]),
                         "auc": float(res["auc"][k]), "ap": float(res["ap"][k]), "f1_macro_at_tau": f1m, "precision_macro_at_tau": prec,
                         "recall_macro_at_tau": rec})
        precL.append(prec); recL.append(rec); f1L.append(f1m)
    aucL, apL = [f["auc"] for f in per_fold], [f["ap"] for f in per_fold]
    auc_bs, ap_bs = res["auc"][n_folds:], res["ap"][n_folds:]
    lo_auc, hi_auc = np.nanpercentile(auc_bs, [2.5, 97.5]) if len(auc_bs) else (np.nan, np.nan)
    lo_ap, hi_ap = np.nanpercentile(ap_bs, [2.5, 97.5]) if len(ap_bs) else (np.nan, np.nan)
    perf = perf if perf is not None else [np.zeros(0)] * 5
    return {
        "config": dict(config),
        "counts_available": {"real": int((y == 0).sum()), "fake": int((y == 1).sum()), "total": int(len(y))},
        "subset": {"n": int(len(idx_pool)), "n_real": int((yt_pool == 0).sum()), "n_fake": int((yt_pool == 1).sum())},
        "metrics_mean_sd": {
            "auc_mean": float(np.mean(aucL)), "auc_sd": float(np.std(aucL, ddof=1)),
            "ap_mean": float(np.mean(apL)), "ap_sd": float(np.std(apL, ddof=1)),
            "f1_macro@tau_mean": float(np.mean(f1L)), "f1_macro@tau_sd": float(np.std(f1L, ddof=1)),
            "precision_macro@tau_mean": float(np.mean(precL)), "precision_macro@tau_sd": float(np.std(precL, ddof=1)),
            "recall_macro@tau_mean": float(np.mean(recL)), "recall_macro@tau_sd": float(np.std(recL, ddof=1))},
        "bootstrap_ci": {"B": int(len(auc_bs)), "auc_ci95": [float(lo_auc), float(hi_auc)], "ap_ci95": [float(lo_ap), float(hi_ap)]},
        "per_fold": per_fold,
        "hardware_stats": {k: summarize_perf(x) for k, x in zip(PERF_KEYS, perf)},
    }


def run_one(y, s, fake_per_real, seed, bootstrap=2000, threshold=0.04, perf=None, config=None):
    """ds.run_one on arrays"""
    y, s = np.asarray(y), np.asarray(s, float)
    idx_pool, folds, boots = plan_run(y, s, fake_per_real, seed, bootstrap)
    pool = make_pool(y[idx_pool], s[idx_pool])
    res = rows(pool, folds + boots, threshold)
    config = config or make_config(None, None, None, fake_per_real, bootstrap, seed, None, threshold)
    return assemble_run(config, y, idx_pool, len(folds), res, perf)


def infer_ratio(ds, y):
    if FIXED_RATIOS.get(ds) is not None:
        return FIXED_RATIOS[ds]
    y = np.asarray(y)
    return float(int((y == 1).sum()) / max(1, int((y == 0).sum())))


def seed_row(seed, threshold, result):
    mm, subs = result["metrics_mean_sd"], result["subset"]
    return [seed, subs["n"], subs["n_real"], subs["n_fake"], threshold] + [mm[k] for k in SEED_HEADER[5:]]


def summary_row(ds, method, fpr, results, out_dir):
    """main's row of summary_all.csv: mean and SD over the seeds' means, the CI and hardware figures of the LAST seed"""
    mm = [r["metrics_mean_sd"] for r in results]
    last = results[-1]
    auc, ap, f1 = mean_sd([m["auc_mean"] for m in mm]), mean_sd([m["ap_mean"] for m in mm]), mean_sd([m["f1_macro@tau_mean"] for m in mm])
    prec, rec = mean_sd([m["precision_macro@tau_mean"] for m in mm]), mean_sd([m["recall_macro@tau_mean"] for m in mm])
    hw, bs = last["hardware_stats"], last["bootstrap_ci"]
    return [ds, method, last["counts_available"]["real"], last["counts_available"]["fake"], fpr, len(results),
            auc[0], auc[1], bs["auc_ci95"][0], bs["auc_ci95"][1], ap[0], ap[1], bs["ap_ci95"][0], bs["ap_ci95"][1],
            f1[0], f1[1], prec[0], prec[1], rec[0], rec[1], hw["fps"]["mean"], hw["fps"]["p95"], hw["latency_ms"]["p50"],
            hw["latency_ms"]["mean"], hw["latency_ms"]["p95"], hw["gpu_alloc_mb"]["p95"], hw["gpu_reserved_mb"]["p95"], hw["cpu_peak_mb"]["p95"], out_dir]


def run(jobs, seeds, threshold, bootstrap=2000, outdir=None):
    """ds.main over ``jobs`` = [(dataset, method, per_video)]; per_video a CSV path or ``(y, s)`` / ``(y, s, fps, lat, gpu_a, gpu_r, cpu_m)``
    -> (summary rows with the header first, {(dataset, method): [run_one's dict per seed]})"""
    out_rows, results = [list(SUMMARY_HEADER)], {}
    for ds, method, per_video in jobs:
        data = load_per_video(per_video) if isinstance(per_video, (str, os.PathLike)) else tuple(per_video)
        y, s, perf = data[0], data[1], (data[2:7] if len(data) >= 7 else None)
        fpr = infer_ratio(ds, y)
        out_dir_ds = os.path.join(outdir, ds, method) if outdir is not None else None
        if out_dir_ds is not None:
            os.makedirs(out_dir_ds, exist_ok=True)
        per_seed = []
        for sd in seeds:
            cfg = make_config(per_video if isinstance(per_video, (str, os.PathLike)) else None, ds, method, fpr, bootstrap, sd, out_dir_ds, threshold)
            result = run_one(y, s, fpr, sd, bootstrap, threshold, perf, cfg)
            per_seed.append(result)
            if out_dir_ds is not None:
                with open(os.path.join(out_dir_ds, "summary_seed%d.json" % sd), "w") as f:
                    json.dump(result, f)
                with open(os.path.join(out_dir_ds, "metrics_seed%d.csv" % sd), "w", newline="") as f:
                    w = csv.writer(f)
                    w.writerow(SEED_HEADER)
                    w.writerow(seed_row(sd, threshold, result))
        results[(ds, method)] = per_seed
        out_rows.append(summary_row(ds, method, fpr, per_seed, out_dir_ds))
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)
        with open(os.path.join(outdir, "summary_all.csv"), "w", newline="") as f:
            csv.writer(f).writerows(out_rows)
    return out_rows, results
