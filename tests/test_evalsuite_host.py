"""CPU: the numpy statement tests/evalsuite_ref.py against what the reference itself computed (tests/golden/eval_suite.*, written by
tools/gen_eval_golden.py): its recorded ``summary_seed*.json``, its ``run_one`` at B = 64, its ``threshold_from_roc`` and TEST2's
summary figures by sklearn.

Floats are compared at 1e-12.  That figure is derived, not measured: every value lies in [0, 1]; AUROC is one division of exact
integers; AP is a sum of at most n <= 4096 non-negative fp64 terms, each a rounded product of a rounded quotient, so the statement
and sklearn (which orders the same sum differently) are each within (n + 8) 2^-53 < 5e-13 of the exact value.  What the generator
measured against sklearn is in the fixture (``measured``) and printed."""
import math

import numpy as np
import pytest

from conftest import load_json, load_npz
import evalsuite_ref as E

GATE = 1e-12
POOLS = ("ffiw", "celebdf", "ffpp_demo", "ffpp_percentile", "faceshifter_adaptive")


@pytest.fixture(scope="module")
def golden():
    return load_json("eval_suite.json"), load_npz("eval_suite.npz")


def pool_arrays(golden, key):
    """(y, s, perf) of a fixture pool; a perf column the fixture leaves out had no finite value: NaN"""
    doc, arr = golden
    y, s = arr[key + "_y"].astype(int), arr[key + "_s"]
    perf = [arr["%s_perf_%s" % (key, c)] if c in doc["pools"][key]["perf"] else np.full(len(y), np.nan) for c in E.PERF_COLUMNS]
    return y, s, perf


def worst_difference(a, b, skip=("config",)):
    """max |a - b| over every number of two nested structures; inf where they differ in shape, a key or a string; NaN equals NaN"""
    if isinstance(a, dict):
        if not isinstance(b, dict) or set(a) != set(b):
            return math.inf
        return max([worst_difference(a[k], b[k], skip) for k in a if k not in skip] + [0.0])
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return math.inf
        return max([worst_difference(x, y, skip) for x, y in zip(a, b)] + [0.0])
    if isinstance(a, (int, float, np.generic)) and not isinstance(a, (bool, np.bool_)) and isinstance(b, (int, float, np.generic)):
        if math.isnan(a) or math.isnan(b):
            return 0.0 if math.isnan(a) and math.isnan(b) else math.inf
        return abs(float(a) - float(b))
    return 0.0 if a == b else math.inf


def integers_of(d):
    """every int of a nested structure, in order (bools apart)"""
    if isinstance(d, dict):
        return [v for k in sorted(d) for v in integers_of(d[k])]
    if isinstance(d, (list, tuple)):
        return [v for x in d for v in integers_of(x)]
    return [int(d)] if isinstance(d, (int, np.integer)) and not isinstance(d, (bool, np.bool_)) else []


def test_the_fixture_holds_what_the_issue_names(golden):
    doc, arr = golden
    assert set(doc["pools"]) == set(POOLS) and not doc["dropped"]
    assert "42" in doc["recorded"]["ffiw"] and "42" in doc["recorded"]["celebdf"]
    assert doc["pools"]["ffiw"]["n"] == 1000 and doc["pools"]["celebdf"]["n"] == 518 and doc["pools"]["faceshifter_adaptive"]["n"] == 2000
    assert doc["pools"]["ffpp_percentile"]["largest_tie"] > 200 and doc["pools"]["faceshifter_adaptive"]["largest_tie"] > 200
    assert doc["recorded"]["ffpp_percentile"]["42"]["bootstrap_ci"]["auc_ci95"][1] == 1.0      # a CI that touches 1.0
    print("generator: max |statement - sklearn| AUROC %.3g, AP %.3g over %d rows" % (doc["measured"]["auc"], doc["measured"]["ap"], doc["measured"]["rows"]))
    assert doc["measured"]["auc"] <= GATE and doc["measured"]["ap"] <= GATE


@pytest.mark.parametrize("key", POOLS)
def test_subset_and_fold_counts_equal_the_recorded_ones(golden, key):
    doc = golden[0]
    y, s, _ = pool_arrays(golden, key)
    meta = doc["pools"][key]
    for seed, want in doc["b64"][key].items():
        idx_pool, folds, boots = E.plan_run(y, s, meta["fake_per_real"], int(seed), 64)
        nR, nF = E.pick_counts(int((y == 0).sum()), int((y == 1).sum()), meta["fake_per_real"])
        assert want["subset"] == {"n": nR + nF, "n_real": nR, "n_fake": nF} == {"n": len(idx_pool), "n_real": int((y[idx_pool] == 0).sum()),
                                                                                 "n_fake": int((y[idx_pool] == 1).sum())}
        assert len(set(idx_pool.tolist())) == len(idx_pool)                      # drawn without replacement
        assert sorted(np.concatenate(folds).tolist()) == list(range(len(idx_pool)))           # five disjoint folds that cover the pool
        yt = y[idx_pool]
        for f, rec in zip(folds, want["per_fold"]):
            assert (len(f), int((yt[f] == 0).sum()), int((yt[f] == 1).sum())) == (rec["n"], rec["n_real"], rec["n_fake"])
        assert len(boots) == 64 and all(len(b) == len(idx_pool) and (yt[b] == 1).sum() == nF for b in boots)
    if key == "celebdf":
        assert (nR, nF) == (178, 340) and len(y) == 518


@pytest.mark.parametrize("key", POOLS)
def test_run_one_equals_the_reference_at_b64(golden, key):
    doc = golden[0]
    y, s, perf = pool_arrays(golden, key)
    meta = doc["pools"][key]
    for seed, want in doc["b64"][key].items():
        got = E.run_one(y, s, meta["fake_per_real"], int(seed), 64, meta["threshold"], perf)
        d = worst_difference(want, got)
        print("%s seed %s: max |statement - reference| %.3g" % (key, seed, d))
        assert d <= GATE
        assert integers_of({k: v for k, v in want.items() if k != "config"}) == integers_of({k: v for k, v in got.items() if k != "config"})
        assert list(got) == list(want) and list(got["metrics_mean_sd"]) == list(want["metrics_mean_sd"])          # key for key, in order
        assert list(got["config"]) == list(want["config"])


@pytest.mark.parametrize("key", ["ffiw", "celebdf", "ffpp_demo", "ffpp_percentile"])
def test_run_one_equals_the_recorded_summaries(golden, key):
    doc = golden[0]
    y, s, perf = pool_arrays(golden, key)
    seeds = ["42"] if key in ("ffpp_demo", "ffpp_percentile") else sorted(doc["recorded"][key])
    assert "42" in seeds
    for seed in seeds:
        rec = doc["recorded"][key][seed]
        c = rec["config"]
        assert c["bootstrap"] == 2000 and c["seed"] == int(seed)
        got = E.run_one(y, s, c["fake_per_real"], c["seed"], c["bootstrap"], c["threshold"], perf)
        d = worst_difference(rec, got)
        print("%s seed %s: max |statement - recorded| %.3g" % (key, seed, d))
        assert d <= GATE


def test_hardware_stats_are_nan_aware(golden):
    doc = golden[0]
    y, s, perf = pool_arrays(golden, "ffiw")
    got = E.run_one(y, s, 1.0, 42, 8, 0.04, perf)["hardware_stats"]
    assert all(math.isnan(v) for stat in got.values() for v in stat.values())   # the ffiw table has no perf column
    y, s, perf = pool_arrays(golden, "ffpp_percentile")
    assert doc["pools"]["ffpp_percentile"]["perf"]
    got = E.run_one(y, s, 4.0, 42, 8, 0.362, perf)["hardware_stats"]
    assert worst_difference(doc["b64"]["ffpp_percentile"]["42"]["hardware_stats"], got) <= GATE
    assert E.summarize_perf(np.array([1.0, np.nan, 3.0, np.inf])) == {"mean": 2.0, "p50": 2.0, "p95": pytest.approx(2.9, abs=1e-15)}


@pytest.mark.parametrize("key", POOLS)
def test_thresholds_equal_the_reference(golden, key):
    doc = golden[0]
    y, s, _ = pool_arrays(golden, key)
    assert len(doc["thresholds"][key]) == 8
    pool = E.make_pool(y, s)
    fpr, tpr, thr = E.roc_curve(pool)
    assert len(thr) == doc["curve"][key]["points"] and pool["groups"] == doc["curve"][key]["groups"] and thr[0] == np.inf
    for name, want in doc["thresholds"][key].items():
        kw = {"target_fpr": float(name[len("target_fpr_"):])} if name.startswith("target_fpr_") else {"metric": name}
        best_t, stats = E.threshold_from_roc(s, y, **kw)
        assert best_t == want["best_t"], name
        assert [stats[k] for k in ("tn", "fp", "fn", "tp")] == [want["stats"][k] for k in ("tn", "fp", "fn", "tp")], name
        assert worst_difference(want["stats"], stats) <= GATE, name


@pytest.mark.parametrize("key", POOLS)
def test_video_table_equals_sklearn(golden, key):
    doc = golden[0]
    y, s, _ = pool_arrays(golden, key)
    want = doc["test2"][key]
    got = E.video_table(y, s, doc["pools"][key]["threshold"])
    assert got["confusion_matrix"] == want["confusion_matrix"] == [[got["tn"], got["fp"]], [got["fn"], got["tp"]]]
    assert worst_difference(want, {k: got[k] for k in want}) <= GATE
    one = E.video_table(np.ones(4, int), [0.1, 0.9, 0.5, 0.7], 0.4)             # one class: NaN AUROC, a 2 x 2 matrix only if predicted
    assert math.isnan(one["auc_roc"]) and one["pr_auc"] == 1.0 and one["confusion_matrix"] == [[0, 0], [1, 3]]


# ---- hand-worked anchors ----------------------------------------------------------------------------------------------------------------

def test_anchor_n2():
    pool = E.make_pool([0, 1], [0.2, 0.7])
    assert pool["rank_of_item"].tolist() == [1, 0] and pool["group_of_rank"].tolist() == [0, 1] and pool["label_of_rank"].tolist() == [1, 0]
    r = E.rows(pool, [[0, 1], [1, 0], [0, 0, 1], [1], [0], []], threshold=0.5)
    assert r["u2"].tolist() == [2, 2, 4, 0, 0, 0] and r["auc"][:3].tolist() == [1.0, 1.0, 1.0] and np.isnan(r["auc"][3:]).all()
    assert r["ap"][:4].tolist() == [1.0, 1.0, 1.0, 1.0] and np.isnan(r["ap"][4:]).all()
    assert (r["tp"].tolist(), r["fp"].tolist(), r["tn"].tolist(), r["fn"].tolist()) == ([1, 1, 1, 1, 0, 0], [0] * 6, [1, 1, 2, 0, 1, 0], [0] * 6)
    worse = E.rows(E.make_pool([1, 0], [0.2, 0.7]), [[0, 1]])                   # the negative on top: U2 = 0, AP = 1 / 2
    assert worse["u2"][0] == 0 and worse["auc"][0] == 0.0 and worse["ap"][0] == 0.5
    fpr, tpr, thr = E.roc_curve(pool)
    assert fpr.tolist() == [0.0, 0.0, 1.0] and tpr.tolist() == [0.0, 1.0, 1.0] and thr.tolist() == [np.inf, 0.7, 0.2]


def test_anchor_all_tied_is_exactly_one_half():
    y = np.array([1, 0, 0, 1, 0, 1, 1])
    pool = E.make_pool(y, np.full(7, 0.25))
    assert pool["groups"] == 1 and pool["order"].tolist() == list(range(7))     # stable: ties keep their order
    r = E.rows(pool, [np.arange(7), [0, 0, 1], [3, 4, 4, 4, 5]])
    assert r["auc"].tolist() == [0.5, 0.5, 0.5]                                  # U2 = P N exactly
    assert r["u2"].tolist() == [12, 2, 6] and r["ap"].tolist() == [4 / 7, 2 / 3, 2 / 5]       # AP of one group: the positive share


def test_anchor_separated_is_exactly_one():
    y = np.array([0] * 5 + [1] * 4)
    pool = E.make_pool(y, np.arange(9) / 10)
    rng = np.random.default_rng(1)
    rows_ = [np.arange(9)] + [np.concatenate([rng.choice(np.arange(5, 9), 4), rng.choice(5, 5)]) for _ in range(5)]
    r = E.rows(pool, rows_, threshold=0.45)
    assert (r["auc"] == 1.0).all() and (r["ap"] == 1.0).all() and (r["tp"] == 4).all() and (r["fp"] == 0).all()


def test_anchor_undrawn_leading_groups_give_no_nan():
    y = np.array([1, 0, 1, 0, 1, 0])
    s = np.array([0.9, 0.9, 0.8, 0.5, 0.5, 0.1])
    pool = E.make_pool(y, s)
    r = E.rows(pool, [[3, 4, 5, 4]])                                             # nobody drew the two best-scored groups: 0 / 0 there
    # group {0.5}: pos 2, neg 1, tp 2, fp 1;  group {0.1}: pos 0, neg 1 -> U2 = 2 (2 (2 - 1) + 1) = 6, AP = 2 (2 / 3) / 2
    assert r["u2"][0] == 6 and r["auc"][0] == 6 / 8 and r["ap"][0] == (2 * (2 / 3)) / 2 and not np.isnan(r["ap_sum"][0])
    mid = E.rows(pool, [np.arange(6)], threshold=0.5)                            # the cut in the middle of nothing: s >= 0.5 is 5 items
    assert (mid["tp"][0], mid["fp"][0], mid["tn"][0], mid["fn"][0]) == (3, 2, 1, 0)


def test_macro_figures_and_zero_division():
    assert E.macro_at(3, 2, 1, 0) == (np.mean([1 / 1, 3 / 5]), np.mean([1 / 3, 3 / 3]), np.mean([2 / 4, 6 / 8]))
    assert E.macro_at(0, 0, 4, 2) == (np.mean([4 / 6, 0.0]), np.mean([1.0, 0.0]), np.mean([8 / 10, 0.0]))    # nothing predicted positive
    assert E.macro_at(0, 0, 5, 0) == (1.0, 1.0, 1.0)                             # one class in truth and predictions: one label
    assert E.mean_sd([1.0, np.nan, 3.0]) == (2.0, math.sqrt(2.0))


def test_run_one_raises_where_the_reference_raises(golden):
    with pytest.raises(ValueError, match="Classi insufficienti"):
        E.run_one(np.ones(20, int), np.linspace(0, 1, 20), 1.0, 42, 4)
    with pytest.raises(ValueError):
        E.run_one(np.array([0, 1, 1, 1, 1, 1, 1, 1]), np.linspace(0, 1, 8), 1.0, 42, 4)       # a pool of 2: five folds do not fit
    with pytest.raises(ValueError, match="outside the pool"):
        E.rows(E.make_pool([0, 1], [0.1, 0.2]), [[0, 2]])


def test_run_writes_the_reference_formats(golden, tmp_path):
    import csv
    import json
    y, s, perf = pool_arrays(golden, "celebdf")
    jobs = [("celebdf", "RetinaFaceDemo", (y, s, *perf)), ("mine", "demo", (y[:200], s[:200]))]
    table, results = E.run(jobs, [42, 43, 44], 0.04, bootstrap=16, outdir=str(tmp_path))
    assert table[0] == E.SUMMARY_HEADER and len(table) == 3 and all(len(r) == len(E.SUMMARY_HEADER) for r in table)
    assert table[1][4] == 1.91 and table[2][4] == float((y[:200] == 1).sum() / (y[:200] == 0).sum())           # fixed and inferred ratios
    per_seed = results[("celebdf", "RetinaFaceDemo")]
    assert table[1][6:8] == list(E.mean_sd([r["metrics_mean_sd"]["auc_mean"] for r in per_seed]))
    assert table[1][8:10] == per_seed[-1]["bootstrap_ci"]["auc_ci95"]             # the CI of the last seed
    with open(tmp_path / "celebdf" / "RetinaFaceDemo" / "summary_seed43.json") as f:
        assert worst_difference(json.load(f), per_seed[1], skip=()) == 0.0
    with open(tmp_path / "celebdf" / "RetinaFaceDemo" / "metrics_seed44.csv", newline="") as f:
        head, row = list(csv.reader(f))
    assert head == E.SEED_HEADER and row == [str(v) for v in E.seed_row(44, 0.04, per_seed[2])]
    with open(tmp_path / "summary_all.csv", newline="") as f:
        assert [r[:2] for r in csv.reader(f)] == [["dataset", "method"], ["celebdf", "RetinaFaceDemo"], ["mine", "demo"]]
