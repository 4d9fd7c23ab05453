"""GPU: af_rank_metrics_rows and af_rank_curve (csrc/af_eval.hip) equal the numpy statement tests/evalsuite_ref.py, with guard bands
around every output; ``RankMetrics``, ``EvalSuite``, ``threshold_from_roc`` and ``video_table`` equal the statement's dicts and sit
within 1e-12 of what the reference recorded (tests/golden/eval_suite.*).

``u2, P, N, tp_cut, fp_cut`` are integers: ``np.array_equal``.  ``ap_sum`` is fp64 added in the order the statement spells out, every
product, quotient and sum rounded once: measured on an MI355X over every case of this file, max |device - statement| = 0.0
(``AP_SUM_MEASURED``; the tests print it).  The assertion stands at 8 x that figure - equality - and never above (n + 2) 2^-52, what
a sum of n rounded terms allows."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
import evalsuite_ref as E
from test_evalsuite_host import POOLS, integers_of, pool_arrays, worst_difference
from test_hip_dualvideo import I_SENT, assert_guards, guarded
from af_mi355x import eval_suite as ES

pytestmark = pytest.mark.gpu
AP_SUM_MEASURED = 0.0                  # max |device ap_sum - statement| measured on the GPU (see the module docstring)
T = E.THREADS


def ap_tolerance(n):
    return min(8 * AP_SUM_MEASURED, (n + 2) * 2.0 ** -52)


@pytest.fixture(scope="module")
def golden():
    return load_json("eval_suite.json"), load_npz("eval_suite.npz")


@pytest.fixture(scope="module")
def rm():
    return ES.RankMetrics()


def device_pool(pool):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
    return dev(pool["rank_of_item"]), dev(pool["group_of_rank"]), dev(pool["label_of_rank"])


def launch_rows(pool, rows, cut=0, flat_off=None):
    """af_rank_metrics_rows on its own, guard bands around the rows and the error word -> (records, error word)"""
    from af_mi355x import _lib
    flat, off = flat_off if flat_off is not None else E.flatten_rows(rows)
    R = len(off) - 1
    rk, gr, lb = device_pool(pool)
    idx = torch.from_numpy(np.asarray(flat, np.int32) if len(flat) else np.zeros(1, np.int32)).cuda()
    offd = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    Ob, O = guarded(4 * R, torch.int64, I_SENT)
    Eb, Er = guarded(1, torch.int32, I_SENT)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.af_rank_metrics_rows(C.c_void_p(rk.data_ptr()), C.c_void_p(gr.data_ptr()), C.c_void_p(lb.data_ptr()), pool["n"],
                                             C.c_void_p(idx.data_ptr()), len(flat), C.c_void_p(offd.data_ptr()), R, int(cut),
                                             C.c_void_p(O.data_ptr()), C.c_void_p(Er.data_ptr()), st), "rank_metrics_rows")
    torch.cuda.synchronize()
    assert_guards(Ob, 4 * R, I_SENT), assert_guards(Eb, 1, I_SENT)
    return O.cpu().numpy().view(ES.ROW_DTYPE), int(Er.cpu()[0])


WORST = {"ap": 0.0}


def check_rows(pool, rows, cut=0):
    got, err = launch_rows(pool, rows, cut)
    want = E.rank_rows(pool, rows, cut)
    assert err == 0 and len(got) == len(rows)
    for k in ("u2", "P", "N", "tp_cut", "fp_cut"):
        assert np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])
    d = float(np.abs(got["ap_sum"] - want["ap_sum"]).max()) if len(rows) else 0.0
    WORST["ap"] = max(WORST["ap"], d)
    print("n %d, %d rows, cut %d: max |device ap_sum - statement| %.3g (so far %.3g)" % (pool["n"], len(rows), cut, d, WORST["ap"]))
    assert not np.isnan(got["ap_sum"]).any() and d <= ap_tolerance(pool["n"])
    return got


def random_pool(rng, n, levels):
    y = rng.integers(0, 2, n)
    y[0], y[-1] = 0, 1
    return E.make_pool(y, rng.integers(0, levels, n) / levels)


def some_rows(rng, n, count):
    """`count` rows: lengths 0, 1, n, 3 n and random ones, repeats allowed"""
    lengths = ([0, 1, n, 3 * n] + [int(v) for v in rng.integers(0, 2 * n + 1, max(0, count - 4))])[:count]
    return [rng.integers(0, n, ln) for ln in lengths]


# ---- the launch against the statement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 63, 64, 65, T, T + 1, 2 * T, 2 * T + 1, 1000])
def test_rows_equal_the_statement(n):
    rng = np.random.default_rng(n)
    for levels in (3, n // 2 + 1, 10 * n):                                        # long ties, short ties, hardly any
        pool = random_pool(rng, n, levels)
        g = pool["group_of_rank"]
        mid = next((r for r in range(1, n) if g[r] == g[r - 1]), n // 2)          # a cut inside a tie group, where there is one
        for count, cut in ((1, 0), (5, n), (69, mid)):
            check_rows(pool, some_rows(rng, n, count), cut)
    rows = some_rows(rng, n, 5)
    a = check_rows(pool, rows, mid)
    b, _ = launch_rows(pool, None, mid, flat_off=E.flatten_rows(rows))
    assert a.tobytes() == b.tobytes()                                            # a rerun is bit-identical


def test_largest_pool_with_a_row_of_16384_draws():
    rng = np.random.default_rng(16384)
    n = E.MAX_POOL
    pool = random_pool(rng, n, 4000)                                              # chunks of 64 ranks, ties of about 4
    check_rows(pool, [rng.integers(0, n, n), np.arange(n), np.zeros(0, int), rng.integers(0, n, 7)], cut=n // 3)


def test_tie_groups_over_chunk_and_wave_seams():
    n = 1000                                                                      # chunks of 4 ranks: thread seams at 4 k, wave seams at 256 k
    rng = np.random.default_rng(5)
    y = rng.integers(0, 2, n)
    base = -np.arange(n, dtype=np.float64)                                        # distinct, descending: item i has rank i
    for lo, hi in ((250, 263), (3, 5), (508, 517), (600, 900), (996, 1000)):      # over thread and wave seams, whole chunks, the tail
        s = base.copy()
        s[lo:hi] = s[lo]
        pool = E.make_pool(y, s)
        assert pool["rank_of_item"].tolist() == list(range(n)) and pool["groups"] == n - (hi - lo) + 1
        check_rows(pool, some_rows(rng, n, 5) + [np.arange(lo, hi), np.arange(lo + 1, hi - 1)], cut=(lo + hi) // 2)
    s = base.copy()
    for lo in range(0, n, 7):                                                     # groups of 7 everywhere: every seam inside one
        s[lo:lo + 7] = s[lo]
    check_rows(E.make_pool(y, s), some_rows(rng, n, 5), cut=501)


@pytest.mark.parametrize("n", [2, 65, 1000, 5000])
def test_one_tie_group_spans_the_pool(n):
    rng = np.random.default_rng(n)
    y = rng.integers(0, 2, n)
    y[0], y[-1] = 0, 1
    pool = E.make_pool(y, np.full(n, 0.5))
    got = check_rows(pool, some_rows(rng, n, 5) + [np.arange(n)], cut=n)
    r = ES.finish_rows(got)
    ok = r["P"] * r["N"] > 0
    assert ok.any() and (r["auc"][ok] == 0.5).all()                               # exactly one half, whatever was drawn
    assert np.array_equal(r["tp"], r["P"]) and np.array_equal(r["fp"], r["N"])


def test_all_draws_on_one_item_per_class_and_undrawn_leading_groups():
    rng = np.random.default_rng(8)
    n = 777
    pool = random_pool(rng, n, 300)
    pos_items, neg_items = np.flatnonzero(pool["y"] == 1), np.flatnonzero(pool["y"] == 0)
    low = pool["order"][n // 2:]                                                  # nobody draws the best-scored half
    rows = [np.r_[np.full(400, pos_items[3]), np.full(377, neg_items[5])], np.full(9, pos_items[0]), np.full(9, neg_items[0]),
            rng.choice(low, 500), pool["order"][-1:], pool["order"][-3:]]
    got = check_rows(pool, rows, cut=n // 2)
    assert got["P"].tolist()[:3] == [400, 9, 0] and got["N"].tolist()[:3] == [377, 0, 9]
    assert (got["tp_cut"][3:] == 0).all() and (got["fp_cut"][3:] == 0).all()


def test_an_index_outside_the_pool_is_skipped_and_counted(rm):
    from af_mi355x import _lib
    rng = np.random.default_rng(2)
    n = 300
    pool = random_pool(rng, n, 50)
    rows = some_rows(rng, n, 5)
    bad = [np.r_[rows[2], [n, -1, 2 ** 31 - 1]], np.r_[[-(2 ** 31)], rows[3]], rows[4]]
    got, err = launch_rows(pool, bad, cut=10)                                     # the guards are checked in launch_rows
    want = E.rank_rows(pool, [rows[2], rows[3], rows[4]], 10)
    assert err == 4 and all(np.array_equal(got[k], want[k]) for k in ("u2", "P", "N", "tp_cut", "fp_cut"))
    off = np.array([0, 5, 3, 9], np.int64)                                        # a row table that goes back, one that leaves the buffer
    got, err = launch_rows(pool, None, flat_off=(np.arange(8), off))
    assert err == 2 and got["P"][1] == 0 and got["N"][1] == 0 and got["P"][2] == 0
    p = rm.pool(pool["y"], pool["s"])
    before = rm.launches
    with pytest.raises(ValueError, match="outside the pool"):
        rm.rows(p, bad)
    assert rm.launches == before                                                  # refused before the upload
    rm.host_check = False
    try:
        with pytest.raises(_lib.AfError, match="4 indices"):
            rm.rows(p, bad)
    finally:
        rm.host_check = True
    assert np.array_equal(rm.rows(p, rows)["u2"], E.rank_rows(pool, rows)["u2"])  # and the next call is sound


def test_a_pool_above_the_lds_bound_is_refused_before_any_launch(rm, monkeypatch):
    from af_mi355x import _lib
    launched = []
    for name in ("af_rank_metrics_rows", "af_rank_curve"):
        monkeypatch.setattr(_lib.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    n = E.MAX_POOL + 1
    with pytest.raises(ValueError, match="16384"):
        rm.pool(np.arange(n) % 2, np.linspace(0, 1, n))
    with pytest.raises(ValueError):
        ES.EvalSuite().run_one(np.arange(2 * n) % 2, np.linspace(0, 1, 2 * n), 1.0, 42, 4)
    with pytest.raises(ValueError):
        rm.pool([0, 1], [0.5, np.nan])
    assert not launched
    monkeypatch.undo()
    assert _lib.lib.af_rank_metrics_rows(None, None, None, n, None, 0, None, 0, 0, None, None, None) != 0


# ---- the curve and the thresholds ------------------------------------------------------------------------------------------------------

def launch_curve(pool):
    from af_mi355x import _lib
    n = pool["n"]
    rk, gr, lb = device_pool(pool)
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    Tb, Tp = guarded(n, torch.int32, I_SENT)
    Fb, Fp = guarded(n, torch.int32, I_SENT)
    Gb, G = guarded(1, torch.int32, I_SENT)
    Eb, Er = guarded(1, torch.int32, I_SENT)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.af_rank_curve(C.c_void_p(rk.data_ptr()), C.c_void_p(gr.data_ptr()), C.c_void_p(lb.data_ptr()), n, C.c_void_p(idx.data_ptr()),
                                      n, C.c_void_p(Tp.data_ptr()), C.c_void_p(Fp.data_ptr()), C.c_void_p(G.data_ptr()), C.c_void_p(Er.data_ptr()),
                                      st), "rank_curve")
    torch.cuda.synchronize()
    for b, k in ((Tb, n), (Fb, n), (Gb, 1), (Eb, 1)):
        assert_guards(b, k, I_SENT)
    groups = int(G.cpu()[0])
    assert int(Er.cpu()[0]) == 0 and (Tp[groups:] == I_SENT).all() and (Fp[groups:] == I_SENT).all()         # nothing behind the last group
    return Tp[:groups].cpu().numpy(), Fp[:groups].cpu().numpy()


def test_curve_equals_the_statement(golden, rm):
    y, s, _ = pool_arrays(golden, "ffpp_percentile")
    for yy, ss in ((y, s), ([0, 1], [0.2, 0.7]), ([1, 0, 1], [0.3, 0.3, 0.3])):
        pool = E.make_pool(yy, ss)
        tps, fps = launch_curve(pool)
        wt, wf = E.curve_counts(pool)
        assert np.array_equal(tps, wt) and np.array_equal(fps, wf) and len(tps) == pool["groups"]
        p = rm.pool(yy, ss)
        ct, cf = rm.curve_counts(p)
        assert np.array_equal(ct, wt) and np.array_equal(cf, wf)
        for a, b in zip(rm.curve(p), E.roc_curve(pool)):
            assert np.array_equal(a, b)
    assert golden[0]["pools"]["ffpp_percentile"]["largest_tie"] > 200 and len(wt) == 1


@pytest.mark.parametrize("key", POOLS)
def test_thresholds_and_video_table_equal_the_reference(golden, key):
    doc = golden[0]
    y, s, _ = pool_arrays(golden, key)
    for name, want in doc["thresholds"][key].items():
        kw = {"target_fpr": float(name[len("target_fpr_"):])} if name.startswith("target_fpr_") else {"metric": name}
        best_t, stats = ES.threshold_from_roc(s, y, **kw)
        assert (best_t, stats) == E.threshold_from_roc(s, y, **kw), name
        assert best_t == want["best_t"] and worst_difference(want["stats"], stats) <= 1e-12, name
    got = ES.video_table(y, s, doc["pools"][key]["threshold"])
    assert worst_difference(E.video_table(y, s, doc["pools"][key]["threshold"]), got) <= ap_tolerance(len(y))
    assert worst_difference(doc["test2"][key], {k: got[k] for k in doc["test2"][key]}) <= 1e-12


# ---- EvalSuite -------------------------------------------------------------------------------------------------------------------------

def assert_dicts(want, got, tol):
    assert list(got) == list(want)
    assert integers_of({k: v for k, v in want.items() if k != "config"}) == integers_of({k: v for k, v in got.items() if k != "config"})
    d = worst_difference(want, got, skip=())
    assert d <= tol, d
    return d


@pytest.mark.parametrize("key", POOLS)
def test_run_one_equals_the_statement_at_b64(golden, key):
    doc = golden[0]
    y, s, perf = pool_arrays(golden, key)
    meta = doc["pools"][key]
    suite = ES.EvalSuite()
    got = suite.run_one(y, s, meta["fake_per_real"], 42, 64, meta["threshold"], perf)
    assert (suite.metrics.launches, suite.metrics.uploads, suite.metrics.readbacks) == (1, 2, 1)      # pool + ONE staging copy, launch, read-back
    want = E.run_one(y, s, meta["fake_per_real"], 42, 64, meta["threshold"], perf)
    d = assert_dicts(want, got, 2 * ap_tolerance(got["subset"]["n"]))
    print("%s: max |device dict - statement| %.3g" % (key, d))
    assert worst_difference(doc["b64"][key]["42"], got) <= 1e-12                   # ... and the reference's own run_one


@pytest.mark.parametrize("key", ["ffiw", "celebdf"])
def test_run_one_at_b2000_sits_on_the_recorded_summary(golden, key):
    rec = golden[0]["recorded"][key]["42"]
    y, s, perf = pool_arrays(golden, key)
    c = rec["config"]
    assert c["bootstrap"] == 2000
    suite = ES.EvalSuite()
    got = suite.run_one(y, s, c["fake_per_real"], 42, 2000, c["threshold"], perf)
    d = worst_difference(rec, got)
    print("%s seed 42, B = 2000: max |device - recorded| %.3g; CI %s / %s; host seconds %s" % (
        key, d, got["bootstrap_ci"]["auc_ci95"], got["bootstrap_ci"]["ap_ci95"], suite.timing))
    assert d <= 1e-12
    for k in ("auc_ci95", "ap_ci95"):
        assert np.abs(np.subtract(got["bootstrap_ci"][k], rec["bootstrap_ci"][k])).max() <= 1e-12
    assert_dicts(E.run_one(y, s, c["fake_per_real"], 42, 2000, c["threshold"], perf), got, 2 * ap_tolerance(got["subset"]["n"]))
    again = suite.run_one(y, s, c["fake_per_real"], 42, 2000, c["threshold"], perf)
    assert json.dumps(again) == json.dumps(got)                                   # bit-identical from run to run


def test_run_equals_the_statement_and_round_trips(golden, tmp_path):
    seeds = [42, 43, 44, 45, 46]
    jobs = []
    for key, ds in (("celebdf", "celebdf"), ("ffpp_percentile", "ffpp")):
        y, s, perf = pool_arrays(golden, key)
        jobs.append((ds, "RetinaFaceDemo", (y, s, *perf)))
    out = str(tmp_path / "suite")
    table, results = ES.EvalSuite().run(jobs, seeds, 0.362, bootstrap=64, outdir=out)
    want_table, want = E.run(jobs, seeds, 0.362, bootstrap=64, outdir=str(tmp_path / "statement"))
    tol = 2 * ap_tolerance(2000)
    assert table[0] == want_table[0] == ES.SUMMARY_HEADER and len(table) == 3
    for row, wrow in zip(table[1:], want_table[1:]):
        assert row[:6] == wrow[:6] and worst_difference(wrow[6:-1], row[6:-1]) <= tol
    for job, per_seed in results.items():
        assert len(per_seed) == 5
        for seed, got, w in zip(seeds, per_seed, want[job]):
            assert_dicts(dict(w, config=dict(w["config"], outdir=got["config"]["outdir"])), got, tol)
            with open("%s/%s/%s/summary_seed%d.json" % (out, job[0], job[1], seed)) as f:
                assert worst_difference(json.load(f), got, skip=()) == 0.0
            with open("%s/%s/%s/metrics_seed%d.csv" % (out, job[0], job[1], seed)) as f:
                assert f.read().splitlines() == [",".join(ES.SEED_HEADER), ",".join(str(v) for v in ES.seed_row(seed, 0.362, got))]
    with open(out + "/summary_all.csv") as f:
        lines = f.read().splitlines()
    assert lines[0] == ",".join(ES.SUMMARY_HEADER) and [ln.split(",")[0] for ln in lines[1:]] == ["celebdf", "ffpp"]
    assert not math.isnan(table[2][20])                                            # the percentile table has perf columns


def test_run_one_raises_where_the_reference_raises():
    suite = ES.EvalSuite()
    with pytest.raises(ValueError, match="Classi insufficienti"):
        suite.run_one(np.ones(20, int), np.linspace(0, 1, 20), 1.0, 42, 4)
    with pytest.raises(ValueError):
        suite.run_one(np.array([0, 1, 1, 1, 1, 1, 1, 1]), np.linspace(0, 1, 8), 1.0, 42, 4)
    assert suite.metrics.launches == 0
