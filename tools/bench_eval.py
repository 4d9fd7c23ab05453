"""EvalSuite on one MI355X: the device time of the rank-metrics launch and the host-inclusive cost of one ``run_one`` beside the numpy
statement (and, where sklearn imports, the reference's per-resample sklearn loop) on the same host.

    python tools/bench_eval.py [--bootstrap 2000] [--reps 50] [--windows 5] [--runs 21] [--json profiles/eval_bench.json]
    python tools/bench_eval.py --draw device [...] [--json profiles/eval_draw_bench.json]

For the ffiw pool (n = 1000) and the 2000-video pool of tests/golden/eval_suite.npz - the only files read - at B = 2000:
rows_device   af_rank_metrics_rows on resident index rows (the 5 folds + B resamples of seed 42), device events around `--reps`
              back-to-back launches after a warm-up, `--windows` such windows, no copy inside the window;
run_one       EvalSuite.run_one, host-inclusive (wall clock around the call, which ends in its own read-back), `--runs` calls,
              alternating with
statement     tests/evalsuite_ref.run_one (numpy) on the same arguments, `--runs` // 3 calls;
sklearn_loop  roc_auc_score + average_precision_score once per fold and resample, as ds.run_one calls them - or, where sklearn does
              not import, a note; the 3.25 s measured for the reference's run_one on a 4-thread CPU box is context, not a ratio;
draw_share    the share of run_one spent drawing the index rows on the host with the reference's own rng calls.
`faster_beyond_spread` is the one condition: the slowest GPU run_one is faster than the fastest statement run_one.  Nothing is gated.
`--draw device` measures the other question instead - where the B resample rows are drawn - on the same two pools, in one session:
run_one       EvalSuite(draw="host").run_one and EvalSuite(draw="device").run_one, alternating, `--runs` calls each, host-inclusive; the
              dicts must be equal; `draw_share` of each leg is timing["draw"] / timing["total"];
draw_device   af_pcg64_draw_rows (scan, resolve, emit) into a resident buffer, device events around `--reps` back-to-back calls;
rows_device   af_rank_metrics_rows on those rows, the same way.
`device_faster_beyond_spread`: the slowest device-draw run_one is faster than the fastest host-draw run_one of this session.
Prints one JSON line and writes it to `--json`.  A run without a GPU fails."""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

POOLS = {"ffiw": 0.04, "faceshifter_adaptive": 0.362}
REFERENCE_CPU_BOX_S = 3.25         # ds.run_one on demo_test/per_video_ffiw.csv, B = 2000, 4 threads, numpy 2.2.6, sklearn 1.7.2


def _spread(v):
    v = sorted(v)
    mid = v[len(v) // 2]
    return {"p50": mid, "min": v[0], "max": v[-1], "mean": statistics.fmean(v), "spread": (v[-1] - v[0]) / mid, "n": len(v)}


def bench_pool(key, tau, doc, arr, B, reps, windows, runs):
    import evalsuite_ref as E
    from af_mi355x import _lib, eval_suite as ES
    y, s = arr[key + "_y"].astype(int), arr[key + "_s"]
    ratio = doc["pools"][key]["fake_per_real"]
    suite = ES.EvalSuite()
    out = {"n": int(len(y)), "fake_per_real": ratio, "threshold": tau, "bootstrap": B}

    # the launch on resident rows
    idx_pool, folds, boots = E.plan_run(y, s, ratio, 42, B)
    pool = suite.metrics.pool(y[idx_pool], s[idx_pool])
    flat, off = E.flatten_rows(folds + boots)
    R = len(off) - 1
    dflat, doff = torch.from_numpy(flat.astype(np.int32)).cuda(), torch.from_numpy(off).cuda()
    dout, derr = torch.empty(4 * R, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    rank, group, label, _ = suite.metrics._pool_pointers(pool)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        _lib.check(_lib.lib.af_rank_metrics_rows(rank, group, label, pool.n, C.c_void_p(dflat.data_ptr()), len(flat), C.c_void_p(doff.data_ptr()), R,
                                                 pool.cut(tau), C.c_void_p(dout.data_ptr()), C.c_void_p(derr.data_ptr()), stream), "rank_metrics_rows")
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    assert int(derr.cpu()[0]) == 0
    us = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            launch()
        t1.record()
        t1.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / reps)
    out["pool_n"], out["rows"], out["draws"] = pool.n, R, int(len(flat))
    out["rows_device_us"] = dict(_spread(us), launches_per_window=reps)

    # run_one: the GPU and the statement, alternating
    gpu, ref, share = [], [], []
    want = None
    for i in range(3):
        got = suite.run_one(y, s, ratio, 42, B, tau)
    for i in range(runs):
        t = time.perf_counter()
        got = suite.run_one(y, s, ratio, 42, B, tau)
        gpu.append(time.perf_counter() - t)
        share.append(suite.timing["draw"] / suite.timing["total"])
        if i % 3 == 0:
            t = time.perf_counter()
            want = E.run_one(y, s, ratio, 42, B, tau)
            ref.append(time.perf_counter() - t)
    assert json.dumps(got) == json.dumps(want), "the GPU run_one and the statement differ"
    out["run_one_gpu_s"], out["run_one_statement_s"] = _spread(gpu), _spread(ref)
    out["draw_share"] = statistics.fmean(share)
    out["last_timing_s"] = suite.timing
    out["statement_over_gpu_p50"] = out["run_one_statement_s"]["p50"] / out["run_one_gpu_s"]["p50"]
    out["faster_beyond_spread"] = bool(out["run_one_gpu_s"]["max"] < out["run_one_statement_s"]["min"])

    # the reference's way: two sklearn calls per row
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
    except Exception as e:                                                        # noqa: BLE001
        out["sklearn_loop_s"] = None
        out["sklearn_note"] = "sklearn does not import here (%s); for context only, not a ratio: the reference's run_one took %.2f s on a 4-thread CPU box" % (
            type(e).__name__, REFERENCE_CPU_BOX_S)
    else:
        yt, st = y[idx_pool], s[idx_pool]
        secs = []
        for _ in range(2):
            t = time.perf_counter()
            for row in folds + boots:
                roc_auc_score(yt[row], st[row]), average_precision_score(yt[row], st[row])
            secs.append(time.perf_counter() - t)
        out["sklearn_loop_s"] = _spread(secs)
        out["sklearn_loop_over_gpu_run_one"] = out["sklearn_loop_s"]["p50"] / out["run_one_gpu_s"]["p50"]
    return out


def _device_us(launch, reps, windows):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            launch()
        t1.record()
        t1.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / reps)
    return dict(_spread(us), launches_per_window=reps)


def bench_draw(key, tau, doc, arr, B, reps, windows, runs):
    """the two draw legs of run_one side by side, and the device time of the draw and of the metrics launch on resident buffers"""
    import evalsuite_ref as E
    from af_mi355x import _lib, eval_suite as ES
    y, s = arr[key + "_y"].astype(int), arr[key + "_s"]
    ratio = doc["pools"][key]["fake_per_real"]
    legs = {"host": ES.EvalSuite(draw="host"), "device": ES.EvalSuite(draw="device")}
    out = {"n": int(len(y)), "fake_per_real": ratio, "threshold": tau, "bootstrap": B}
    secs, share, got = {k: [] for k in legs}, {k: [] for k in legs}, {}
    for k, suite in legs.items():
        for _ in range(3):
            suite.run_one(y, s, ratio, 42, B, tau)
    for _ in range(runs):
        for k, suite in legs.items():
            t = time.perf_counter()
            got[k] = suite.run_one(y, s, ratio, 42, B, tau)
            secs[k].append(time.perf_counter() - t)
            share[k].append(suite.timing["draw"] / suite.timing["total"])
    assert json.dumps(got["host"]) == json.dumps(got["device"]), "the two draw modes differ"
    for k, suite in legs.items():
        out["run_one_%s_draw_s" % k] = _spread(secs[k])
        out["draw_share_%s" % k] = statistics.fmean(share[k])
        out["last_timing_%s_s" % k] = suite.timing
        out["staged_bytes_per_run_one_%s" % k] = suite.metrics.staged_bytes // (runs + 3)
    out["draw_result"] = legs["device"].metrics.last_draw
    out["host_over_device_p50"] = out["run_one_host_draw_s"]["p50"] / out["run_one_device_draw_s"]["p50"]
    out["device_faster_beyond_spread"] = bool(out["run_one_device_draw_s"]["max"] < out["run_one_host_draw_s"]["min"])

    # the launches on resident buffers: the rows of seed 42 behind the five fold rows, as bootstrap_rows_raw lays them out
    idx_pool, folds, _ = E.plan_run(y, s, ratio, 42, 0)
    rm = legs["device"].metrics
    pool = rm.pool(y[idx_pool], s[idx_pool])
    yt = y[idx_pool]
    pos, neg = np.where(yt == 1)[0], np.where(yt == 0)[0]
    a, b, F = len(pos), len(neg), len(folds)
    rng = np.random.default_rng(42)
    ES.ratio_match_indices(y, ratio, rng)
    start, _, cap = rm._draw_plan(a, a, b, b, B, rng, [True, True], None)
    fold_off = a + b + np.concatenate([[0], np.cumsum([len(f) for f in folds])]).astype(np.int64)
    row_base, R = int(fold_off[-1]), F + B
    n_idx = row_base + B * (a + b)
    didx = torch.zeros(n_idx, dtype=torch.int32, device="cuda")
    didx[:row_base] = torch.from_numpy(np.concatenate([pos, neg] + folds).astype(np.int32)).cuda()
    doff = torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    doff[:F + 1] = torch.from_numpy(fold_off).cuda()
    dres = torch.zeros(C.sizeof(_lib.DrawResult), dtype=torch.uint8, device="cuda")
    dout, derr = torch.empty(4 * R, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(_lib.lib.af_pcg64_draw_workspace_bytes(cap)), dtype=torch.uint8, device="cuda")
    rank, group, label, _ = rm._pool_pointers(pool)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def draw():
        _lib.check(_lib.lib.af_pcg64_draw_rows(C.byref(start), a, a, b, b, B, C.c_void_p(didx.data_ptr()), C.c_void_p(didx.data_ptr() + 4 * a), cap,
                                               C.c_void_p(didx.data_ptr() + 4 * row_base), C.c_void_p(doff.data_ptr() + 8 * F), row_base,
                                               C.c_void_p(dres.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), stream), "pcg64_draw_rows")

    def rows():
        _lib.check(_lib.lib.af_rank_metrics_rows(rank, group, label, pool.n, C.c_void_p(didx.data_ptr()), n_idx, C.c_void_p(doff.data_ptr()), R,
                                                 pool.cut(tau), C.c_void_p(dout.data_ptr()), C.c_void_p(derr.data_ptr()), stream), "rank_metrics_rows")
    out["pool_n"], out["rows"], out["draws"] = pool.n, R, int(B * (a + b))
    out["draw_device_us"] = _device_us(draw, reps, windows)
    out["rows_device_us"] = _device_us(rows, reps, windows)
    res = _lib.DrawResult.from_buffer_copy(dres.cpu().numpy().tobytes())
    assert res.error == 0 and int(derr.cpu()[0]) == 0 and res.consumed == legs["device"].metrics.last_draw["consumed"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bootstrap", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--draw", choices=("host", "device"), default="host",
                    help="device: compare EvalSuite(draw='device') with draw='host' and time the draw launches (profiles/eval_draw_bench.json)")
    ap.add_argument("--json", default=None)
    opt = ap.parse_args()
    if opt.json is None:
        opt.json = os.path.join(ROOT, "profiles", "eval_draw_bench.json" if opt.draw == "device" else "eval_bench.json")
    assert torch.cuda.is_available(), "bench_eval needs a GPU"
    with open(os.path.join(ROOT, "tests", "golden", "eval_suite.json")) as f:
        doc = json.load(f)
    arr = np.load(os.path.join(ROOT, "tests", "golden", "eval_suite.npz"))
    props = torch.cuda.get_device_properties(0)
    res = {"tool": "bench_eval" if opt.draw == "host" else "bench_eval --draw device", "device": props.name, "arch": getattr(props, "gcnArchName", ""), "host": platform.node(),
           "numpy": np.__version__, "gated": False,
           "reference_run_one_cpu_box_s": REFERENCE_CPU_BOX_S}
    for key, tau in POOLS.items():
        res[key] = (bench_draw if opt.draw == "device" else bench_pool)(key, tau, doc, arr, opt.bootstrap, opt.reps, opt.windows, opt.runs)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(opt.json), exist_ok=True)
    with open(opt.json, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
