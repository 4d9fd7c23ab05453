"""Writes tests/golden/eval_suite.npz / .json: the REFERENCE's evaluation protocol (altfreezing/ds.py) and threshold picker
(dualrun/train/thresholds.py) on per-video tables the reference ships, next to what its own run recorded for them.

    python tools/gen_eval_golden.py [--reference DIR]

Runs only where the reference and sklearn exist: ``ds.py`` and ``thresholds.py`` are loaded by path.  Written:
  pools      labels, scores and the perf columns ``load_per_video`` reads (arrays only; a perf column with no finite value is left out);
  recorded   the reference's ``summary_seed42..46.json`` of a pool - kept only when ``ds.run_one``, run where this runs, reproduces it at
             1e-12 (numpy's ``default_rng`` stream and sklearn are then the recorded ones); what did not is listed under ``dropped``;
             the paths of its ``config`` are blanked;
  b64        ``ds.run_one`` at B = 64 for every pool and two seeds;
  thresholds ``threshold_from_roc`` for every metric and for target_fpr in {0, 0.05, 1};
  test2      accuracy, AUROC, AP, F1 and the confusion matrix of TEST2.py:1123-1128, by sklearn;
  measured   max |tests/evalsuite_ref.py - sklearn| of AUROC and AP over every fold and resample row of the B = 64 runs.
The statement must equal every reference dict at 1e-12, or nothing is written.
"""
import argparse
import importlib.util
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, _p))
import evalsuite_ref as E              # noqa: E402

POOLS = {  # key: (csv, dataset, recorded summaries' directory or None, threshold)
    "ffiw": ("demo_test/per_video_ffiw.csv", "ffiw", "demo_test/ffiw/RetinaFaceDemo", 0.04),
    "celebdf": ("demo_test/per_video_celebdf.csv", "celebdf", "demo_test/celebdf/RetinaFaceDemo", 0.04),
    "ffpp_demo": ("demo_test/per_videoDEMOff++.csv", "ffpp", "demo_test/ffpp/RetinaFaceDemo", 0.04),
    "ffpp_percentile": ("new_demo_test/ffpp/percentile/percentile.csv", "ffpp", "new_demo_test/ffpp/RetinaFaceDemo", 0.362),
    "faceshifter_adaptive": ("new_demo_test/ffpp_faceshifter_mixed/adaptive/per_video.csv", "ffpp_faceshifter_mixed", None, 0.362),
}
SEEDS, B64_SEEDS, GATE = (42, 43, 44, 45, 46), (42, 43), 1e-12
METRICS = ("youden", "balacc", "auc", "acc", "f1")
TARGETS = (0.0, 0.05, 1.0)


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plain(o):
    """numpy scalars -> Python's, for json"""
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    if isinstance(o, np.generic):
        return o.item()
    return o


def worst_difference(a, b, skip=("config",)):
    """max |a - b| over every number of two nested dicts; inf on a structural difference; NaN equals NaN"""
    if isinstance(a, dict):
        if not isinstance(b, dict) or set(a) != set(b):
            return math.inf
        return max([worst_difference(a[k], b[k], skip) for k in a if k not in skip] + [0.0])
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return math.inf
        return max([worst_difference(x, y, skip) for x, y in zip(a, b)] + [0.0])
    if isinstance(a, (int, float, np.generic)) and isinstance(b, (int, float, np.generic)):
        if math.isnan(a) or math.isnan(b):
            return 0.0 if math.isnan(a) and math.isnan(b) else math.inf
        return abs(float(a) - float(b))
    return 0.0 if a == b else math.inf


def blank_paths(result):
    result = dict(result)
    result["config"] = dict(result["config"], per_video=None, outdir=None)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "eval_suite"))
    opt = ap.parse_args()
    if opt.reference is None:
        import ref_import
        opt.reference = ref_import.REFERENCE_ROOT
    alt = os.path.join(opt.reference, "altfreezing")
    ds = load(os.path.join(alt, "ds.py"), "ref_ds")
    TH = load(os.path.join(opt.reference, "dualrun", "train", "thresholds.py"), "ref_thresholds")
    from sklearn.metrics import accuracy_score, average_precision_score, confusion_matrix, f1_score, roc_auc_score, roc_curve

    arrays, doc = {}, {"what": "altfreezing/ds.py and dualrun/train/thresholds.py of the reference on its own per-video tables "
                               "(tools/gen_eval_golden.py)", "gate": GATE, "pools": {}, "recorded": {}, "dropped": [], "b64": {},
                       "thresholds": {}, "test2": {}, "curve": {}}
    d_auc = d_ap = 0.0
    for key, (rel, dataset, rec_dir, tau) in POOLS.items():
        path = os.path.join(alt, rel)
        y, s, *perf = ds.load_per_video(path)
        mine = E.load_per_video(path)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip((y, s, *perf), mine)), key
        ratio = ds.infer_ratio(dataset, path)
        assert ratio == E.infer_ratio(dataset, y)
        arrays[key + "_y"], arrays[key + "_s"] = y.astype(np.int8), s.astype(np.float64)
        has_perf = [bool(np.isfinite(p).any()) for p in perf]
        for name, p, keep in zip(E.PERF_COLUMNS, perf, has_perf):
            if keep:
                arrays["%s_perf_%s" % (key, name)] = p.astype(np.float64)
        pool = E.make_pool(y, s)
        ties = int(np.bincount(pool["group_of_rank"]).max())
        doc["pools"][key] = {"source": rel, "dataset": dataset, "fake_per_real": ratio, "threshold": tau, "n": int(len(y)),
                             "largest_tie": ties, "perf": [n for n, k in zip(E.PERF_COLUMNS, has_perf) if k]}

        def both(seed, B, thr, fpr):
            cfg = ds.EvalConfig(per_video=path, dataset=dataset, method="RetinaFaceDemo", fake_per_real=fpr, bootstrap=B, seed=seed,
                                outdir="out", threshold=thr)
            want = ds.run_one(cfg)
            got = E.run_one(y, s, fpr, seed, B, thr, perf, E.make_config(path, dataset, "RetinaFaceDemo", fpr, B, seed, "out", thr))
            assert got["config"] == want["config"], (got["config"], want["config"])
            d = worst_difference(plain(want), got)
            assert d <= GATE, "%s seed %d B %d: the statement is %.3g from the reference" % (key, seed, B, d)
            return plain(want)

        # the recorded summaries that the reference's own run_one reproduces here
        doc["recorded"][key] = {}
        for seed in SEEDS if rec_dir else ():
            with open(os.path.join(alt, rec_dir, "summary_seed%d.json" % seed)) as f:
                rec = json.load(f)
            c = rec["config"]
            assert c["seed"] == seed and os.path.basename(c["per_video"].replace("\\", "/")) == os.path.basename(rel), c
            here = both(seed, c["bootstrap"], c["threshold"], c["fake_per_real"])
            d = worst_difference(rec, here)
            print("%s seed %d: recorded vs the reference run here %.3g" % (key, seed, d))
            if d <= GATE:
                doc["recorded"][key][str(seed)] = blank_paths(rec)
            else:
                doc["dropped"].append({"pool": key, "seed": seed, "difference": d if math.isfinite(d) else "structure"})
        # B = 64
        doc["b64"][key] = {}
        for seed in B64_SEEDS:
            doc["b64"][key][str(seed)] = blank_paths(both(seed, 64, tau, ratio))
            idx_pool, folds, boots = E.plan_run(y, s, ratio, seed, 64)
            yt, st = y[idx_pool], s[idx_pool]
            r = E.rows(E.make_pool(yt, st), folds + boots, tau)
            for i, row in enumerate(folds + boots):
                d_auc = max(d_auc, abs(r["auc"][i] - roc_auc_score(yt[row], st[row])))
                d_ap = max(d_ap, abs(r["ap"][i] - average_precision_score(yt[row], st[row])))
        # thresholds
        fpr_, tpr_, thr_ = roc_curve(y, s)
        mf, mt, mthr = E.roc_curve(pool)
        assert np.array_equal(fpr_, mf) and np.array_equal(tpr_, mt) and np.array_equal(thr_, mthr), key
        doc["curve"][key] = {"points": int(len(thr_)), "groups": pool["groups"]}
        doc["thresholds"][key] = {}
        for name, kw in [(m, {"metric": m}) for m in METRICS] + [("target_fpr_%g" % t, {"target_fpr": t}) for t in TARGETS]:
            best_t, stats = TH.threshold_from_roc(s, y, **kw)
            mine_t, mine_stats = E.threshold_from_roc(s, y, **kw)
            assert mine_t == best_t and worst_difference(plain(stats), mine_stats) <= GATE, (key, name)
            doc["thresholds"][key][name] = {"best_t": best_t, "stats": plain(stats)}
        # TEST2.main's summary
        y_pred = (s > tau).astype(int)
        t2 = {"videos": int(len(y)), "accuracy": accuracy_score(y, y_pred), "f1": f1_score(y, y_pred),
              "auc_roc": roc_auc_score(y, s) if len(set(y.tolist())) > 1 else float("nan"), "pr_auc": average_precision_score(y, s),
              "confusion_matrix": confusion_matrix(y, y_pred).tolist()}
        mine = E.video_table(y, s, tau)
        assert worst_difference(plain(t2), {k: mine[k] for k in t2}) <= GATE, (key, t2, mine)
        doc["test2"][key] = plain(t2)

    for must in ("ffiw", "celebdf"):
        assert "42" in doc["recorded"][must], "the %s seed-42 summary did not reproduce" % must
    doc["measured"] = {"auc": d_auc, "ap": d_ap, "rows": 69 * len(B64_SEEDS) * len(POOLS)}
    np.savez_compressed(opt.out + ".npz", **arrays)
    with open(opt.out + ".json", "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))                               # unsorted: the dicts keep the reference's key order
    print("wrote %s.npz (%d bytes), .json (%d bytes); recorded kept %s, dropped %s; max |statement - sklearn| auc %.3g ap %.3g" % (
        opt.out, os.path.getsize(opt.out + ".npz"), os.path.getsize(opt.out + ".json"),
        {k: sorted(v) for k, v in doc["recorded"].items()}, doc["dropped"], d_auc, d_ap))


if __name__ == "__main__":
    main()
