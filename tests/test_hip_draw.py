"""GPU: af_pcg64_draw_rows (csrc/af_draw.hip) draws what numpy draws - the rows ``np.array_equal`` to the statement tests/pcg64_ref.py
(which tests/test_pcg64_host.py holds against numpy itself), the words consumed equal, the caller's generator left in numpy's final
state - and ``EvalSuite(draw="device")`` returns the dicts and writes the files of ``EvalSuite(draw="host")``.

Everything here is integer arithmetic: every comparison is equality.  The one bound that is not a measurement of this code is the
staging cap of the issue, 4 (n + sum of the fold sizes + len(pos) + len(neg)) + 4096 bytes per ``run_one`` whatever B: it is held
against ``RankMetrics.staged_bytes``, the bytes the row calls copy to the device - the fold rows, their offsets, ``pos`` and ``neg``.  The
pool's own resident upload (``RankMetrics.pool``: 13 n bytes, the same in both modes and independent of B) is not part of that count."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import pcg64_ref as R
from conftest import load_json, load_npz
from test_evalsuite_host import POOLS, pool_arrays, worst_difference
from test_hip_dualvideo import I_SENT, assert_guards, guarded
from test_pcg64_host import CASES, STARTS, numpy_rows, pools, same_state, start_rng, statement
from af_mi355x import eval_suite as ES

pytestmark = pytest.mark.gpu
HEAVY = (2 ** 31 + 1, 257, 3 * 2 ** 30, 130, 2)           # bounds, counts, rows: about half of the words are rejected


@pytest.fixture(scope="module")
def golden():
    return load_json("eval_suite.json"), load_npz("eval_suite.npz")


@pytest.fixture(scope="module")
def rm():
    return ES.RankMetrics()


def raw_draw(sd, bound_a, count_a, bound_b, count_b, rows, items_a=None, items_b=None, max_rejects=None, row_base=0):
    """af_pcg64_draw_rows on its own, guard bands around idx, row_off and the result -> (idx int32, row_off, DrawResult, return code)"""
    from af_mi355x import _lib
    cap = _lib.DRAW_MAX_REJECTS if max_rejects is None else max_rejects
    s, inc, has, uinteger = R.unpack(sd)
    start = _lib.Pcg64State(s >> 64, s & R.M64, inc >> 64, inc & R.M64, has, uinteger)
    n = rows * (count_a + count_b)
    dev = [None if it is None else torch.from_numpy(np.asarray(it, np.int32)).cuda() for it in (items_a, items_b)]
    Ib, I = guarded(n, torch.int32, I_SENT)
    Ob, O = guarded(rows + 1, torch.int64, I_SENT)
    Rb, Rs = guarded(C.sizeof(_lib.DrawResult) // 4, torch.int32, I_SENT)
    ws_bytes = int(_lib.lib.af_pcg64_draw_workspace_bytes(cap))
    assert ws_bytes >= 12 * cap
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = _lib.lib.af_pcg64_draw_rows(C.byref(start), bound_a, count_a, bound_b, count_b, rows, C.c_void_p(0 if dev[0] is None else dev[0].data_ptr()),
                                     C.c_void_p(0 if dev[1] is None else dev[1].data_ptr()), cap, C.c_void_p(I.data_ptr()), C.c_void_p(O.data_ptr()),
                                     row_base, C.c_void_p(Rs.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert_guards(Ib, n, I_SENT), assert_guards(Ob, rows + 1, I_SENT), assert_guards(Rb, C.sizeof(_lib.DrawResult) // 4, I_SENT)
    res = _lib.DrawResult.from_buffer_copy(Rs.cpu().numpy().tobytes()) if rc == 0 else None
    return I.cpu().numpy(), O.cpu().numpy(), res, rc


def check_against_statement(rm, sd, bound_a, count_a, bound_b, count_b, rows, items_a=None, items_b=None):
    """drawn_rows from the state `sd` against the statement: rows, words consumed and the generator's final state"""
    bg = np.random.PCG64()
    bg.state = sd
    rng = np.random.Generator(bg)
    want, consumed, final = R.draw_rows(sd, bound_a, count_a, bound_b, count_b, rows, items_a, items_b)
    got, used = rm.drawn_rows(bound_a, count_a, bound_b, count_b, rows, rng, items_a, items_b)
    assert got.shape == want.shape and np.array_equal(got, want), (np.flatnonzero(got != want)[:8], got[:8], want[:8])
    assert used == consumed and same_state(rng.bit_generator.state, final)
    return rm.last_draw


@pytest.mark.parametrize("buffered", STARTS)
@pytest.mark.parametrize("case", list(CASES))
def test_drawn_rows_equal_the_statement_and_leave_numpys_state(rm, case, buffered):
    a, b, B, seed = case
    start, want, consumed, final = statement(case, buffered)
    rng, ref = start_rng(seed, buffered), start_rng(seed, buffered)
    got, used = rm.drawn_rows(a, a, b, b, B, rng, *pools(a, b))
    assert got.shape == want.shape and np.array_equal(got, want), (np.flatnonzero(got != want)[:8], got[:8], want[:8])
    assert used == consumed and same_state(rng.bit_generator.state, final)
    assert rm.last_draw["rejected"] == consumed - B * ((a if a > 1 else 0) + b)
    if not buffered:
        assert rm.last_draw["rejected"] == CASES[case]
    assert np.array_equal(numpy_rows(ref, a, b, B), got)                          # numpy itself, and where it stands afterwards
    assert same_state(rng.bit_generator.state, ref.bit_generator.state) and rng.random() == ref.random()


@pytest.mark.parametrize("rows", [1, 33])
def test_seams_of_tiles_threads_and_segments(rm, rows):
    counts = [1, 63, 64, 65, 255, 256, 257, 1023]                                 # an emit thread owns 16 words, a workgroup 4096
    for buffered in STARTS:
        sd = start_rng(100 + rows, buffered).bit_generator.state
        for ca, cb in zip(counts, counts[::-1]):
            check_against_statement(rm, sd, ca, ca, cb, cb, rows, 5 + np.arange(ca), 9000 + np.arange(cb))      # a count of 1: a bound of 1
            check_against_statement(rm, sd, 1000003, ca, 77, cb, rows)                                          # value mode, small bounds
        check_against_statement(rm, sd, 300, 300, 7, 0, rows, np.arange(300))                                   # an empty segment
        check_against_statement(rm, sd, 7, 0, 4100, 4100, rows, None, np.arange(4100))                          # ... in front; a tile seam
        check_against_statement(rm, sd, 1, 1, 1, 1, rows, [4], [6])                                             # no word at all
        check_against_statement(rm, sd, 1, 3, 1, 2, rows)
        check_against_statement(rm, sd, 5, 0, 9, 0, rows)                                                       # no draw at all


@pytest.mark.parametrize("buffered", STARTS)
def test_value_mode_where_half_of_the_words_are_rejected(rm, buffered):
    sd = start_rng(9, buffered).bit_generator.state
    info = check_against_statement(rm, sd, *HEAVY)
    T = HEAVY[4] * (HEAVY[1] + HEAVY[3])
    print("heavy: %s" % info)
    assert info["consumed"] > 1.5 * T and info["rejected"] == info["consumed"] - T and info["listed"] >= info["rejected"]
    info = check_against_statement(rm, sd, HEAVY[2], 1000, HEAVY[0], 31, 1)                                    # the bounds the other way round
    assert info["rejected"] > 200
    check_against_statement(rm, sd, 2 ** 32 - 1, 700, 2, 65, 3)                                                # the largest bound


def test_an_overflowing_list_is_flagged_and_nothing_is_drawn(rm):
    from af_mi355x import _lib
    sd = start_rng(9, 1).bit_generator.state
    idx, off, res, rc = raw_draw(sd, *HEAVY, max_rejects=4)
    assert rc == 0 and res.error != 0 and res.consumed == -1 and res.listed > 4
    assert (idx == I_SENT).all()                                                  # no row was written
    bg = np.random.PCG64()
    bg.state = sd
    rng = np.random.Generator(bg)
    with pytest.raises(_lib.AfError, match="overflowed"):
        rm.drawn_rows(*HEAVY, rng, max_rejects=4)
    assert rng.bit_generator.state == sd                                          # the generator stays where it was
    check_against_statement(rm, sd, *HEAVY)                                       # and the next call is sound
    check_against_statement(rm, sd, 300, 300, 218, 218, 7, np.arange(300), np.arange(218))


def test_guard_bands_row_table_and_reruns():
    case = (9973, 6007, 24, 3)
    a, b, B, _ = case
    for buffered in STARTS:
        start, want, consumed, final = statement(case, buffered)
        i1, o1, r1, rc = raw_draw(start, a, a, b, b, B, *pools(a, b), row_base=1234)     # the guards are checked in raw_draw
        i2, o2, r2, _ = raw_draw(start, a, a, b, b, B, *pools(a, b), row_base=1234)
        assert rc == 0 and r1.error == 0 and np.array_equal(i1, want)
        assert i1.tobytes() == i2.tobytes() and o1.tobytes() == o2.tobytes() and bytes(r1) == bytes(r2)
        assert np.array_equal(o1, 1234 + np.arange(B + 1) * (a + b))
        assert (r1.consumed, r1.rejected, r1.has_uint32) == (consumed, consumed - B * (a + b), final["has_uint32"])
        assert not final["has_uint32"] or r1.uinteger == final["uinteger"]
    _, o, r, rc = raw_draw(start, a, a, b, b, 0, *pools(a, b), row_base=7)                # no rows: the table's one entry, nothing consumed
    assert rc == 0 and o.tolist() == [7] and (r.consumed, r.error, r.has_uint32, r.uinteger) == (0, 0, start["has_uint32"], start["uinteger"])


def test_refusals_come_before_any_launch(rm, monkeypatch):
    from af_mi355x import _lib
    launched = []
    for name in ("af_pcg64_draw_rows", "af_rank_metrics_rows"):
        monkeypatch.setattr(_lib.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    rng = np.random.default_rng(1)
    before = rng.bit_generator.state
    with pytest.raises(ValueError, match="2\\^32"):
        rm.drawn_rows(2 ** 32, 5, 7, 5, 1, rng)
    with pytest.raises(ValueError, match="2\\^32"):
        rm.drawn_rows(7, 5, 0, 5, 1, rng)
    for other in (np.random.MT19937(1), np.random.PCG64DXSM(1), np.random.Philox(1)):
        with pytest.raises(ValueError, match="PCG64"):
            rm.drawn_rows(7, 5, 7, 5, 1, np.random.Generator(other))
    with pytest.raises(ValueError, match="PCG64"):
        rm.drawn_rows(7, 5, 7, 5, 1, np.random.RandomState(1))
    with pytest.raises(ValueError, match="2\\^31"):
        rm.drawn_rows(7, 2 ** 15, 7, 2 ** 15, 2 ** 15, rng)
    with pytest.raises(ValueError, match="items"):
        rm.drawn_rows(8, 7, 5, 5, 1, rng, np.arange(7), np.arange(5))
    with pytest.raises(ValueError, match="items"):
        rm.drawn_rows(7, 6, 5, 5, 1, rng, np.arange(7), np.arange(5))
    with pytest.raises(ValueError, match="rejected"):
        rm.drawn_rows(2 ** 31 + 1, 5000, 2, 5, 1, rng)                            # about 5000 expected rejections, 2048 allowed
    with pytest.raises(ValueError):
        rm.drawn_rows(7, 5, 7, 5, 1, rng, max_rejects=_lib.DRAW_MAX_REJECTS + 1)
    p = rm.pool([0, 1, 1, 0], [0.1, 0.9, 0.8, 0.3])
    with pytest.raises(ValueError, match="PCG64"):
        rm.bootstrap_rows_raw(p, [np.arange(4)], [1, 2], [0, 3], 8, np.random.Generator(np.random.MT19937(1)))
    with pytest.raises(ValueError, match="outside the pool"):
        rm.bootstrap_rows_raw(p, [np.arange(4)], [1, 4], [0, 3], 8, rng)
    with pytest.raises(ValueError):
        ES.EvalSuite(draw="gpu")
    assert not launched and rng.bit_generator.state == before
    # 16 384 items at B = 10 000 pass the default list's precheck whatever the split: the worst is about 625 expected rejections
    worst = max((10000 * (a + 16384 - a) * max(2 ** 32 % a, 2 ** 32 % (16384 - a)) / (2 ** 32 - max(2 ** 32 % a, 2 ** 32 % (16384 - a))), a)
                for a in range(1, 16384))
    print("largest expected rejection count over the splits of 16384 at B = 10000: %.0f (a = %d)" % worst)
    assert worst[0] <= _lib.DRAW_MAX_REJECTS / ES.DRAW_LIST_SHARE
    monkeypatch.undo()
    # the C entry refuses the same by itself
    some = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")                 # a valid address for every pointer: none is reached
    ptr, start = C.c_void_p(some.data_ptr()), _lib.Pcg64State(1, 2, 3, 5, 0, 0)

    def refused(bound_a, count_a, bound_b, count_b, rows, items=None, cap=16, ws_bytes=1 << 16, state=start):
        rc = _lib.lib.af_pcg64_draw_rows(C.byref(state), bound_a, count_a, bound_b, count_b, rows, items, items, cap, ptr, ptr, 0, ptr, ptr, ws_bytes, None)
        return rc != 0 and b"pcg64_draw_rows" in _lib.lib.af_last_error()
    for args in ((2 ** 32, 5, 7, 5, 1), (7, 5, 2 ** 32, 5, 1), (0, 5, 7, 5, 1), (7, -1, 7, 5, 1), (7, 5, 7, 5, -1), (7, 2 ** 15, 7, 2 ** 15, 2 ** 15)):
        assert refused(*args), args
    assert refused(8, 7, 7, 7, 1, items=ptr) and refused(7, 7, 7, 8, 1, items=ptr)               # items: the bound is the count
    assert refused(7, 5, 7, 5, 1, cap=0) and refused(7, 5, 7, 5, 1, cap=_lib.DRAW_MAX_REJECTS + 1) and refused(7, 5, 7, 5, 1, ws_bytes=64)
    assert refused(7, 5, 7, 5, 1, state=_lib.Pcg64State(1, 2, 3, 4, 0, 0)) and refused(7, 5, 7, 5, 1, state=_lib.Pcg64State(1, 2, 3, 5, 2, 0))
    torch.cuda.synchronize()
    assert _lib.lib.af_pcg64_draw_rows(None, 7, 5, 7, 5, 1, None, None, 16, None, None, 0, None, None, 0, None) != 0
    assert _lib.lib.af_pcg64_draw_workspace_bytes(0) == 0 and _lib.lib.af_pcg64_draw_workspace_bytes(_lib.DRAW_MAX_REJECTS + 1) == 0


# ---- EvalSuite(draw="device") ------------------------------------------------------------------------------------------------------------

def staging_cap(n, pos, neg):
    return 4 * (n + n + pos + neg) + 4096                                          # the folds partition the pool: their sizes sum to n


@pytest.mark.parametrize("key", POOLS)
def test_run_one_device_equals_host_at_b64(golden, key):
    y, s, perf = pool_arrays(golden, key)
    meta = golden[0]["pools"][key]
    host, dev = ES.EvalSuite(draw="host"), ES.EvalSuite(draw="device")
    want = host.run_one(y, s, meta["fake_per_real"], 42, 64, meta["threshold"], perf)
    got = dev.run_one(y, s, meta["fake_per_real"], 42, 64, meta["threshold"], perf)
    assert got == want, worst_difference(want, got, skip=())
    assert json.dumps(got) == json.dumps(want)
    m = dev.metrics
    assert (m.launches, m.readbacks) == (4, 1)                                     # scan, resolve, emit, metrics; ONE read-back
    sub = got["subset"]
    assert m.staged_bytes <= staging_cap(sub["n"], sub["n_fake"], sub["n_real"])
    assert set(dev.timing) == set(host.timing) == {"draw", "rows", "total"} and 0 < dev.timing["draw"] < dev.timing["total"]
    print("%s: staged %d bytes of %d allowed; draw %s; timing %s" % (key, m.staged_bytes, staging_cap(sub["n"], sub["n_fake"], sub["n_real"]),
                                                                      m.last_draw, dev.timing))


def test_run_one_device_at_b2000_sits_on_the_recorded_summary_and_stages_no_more(golden):
    key = "ffiw"
    rec = golden[0]["recorded"][key]["42"]
    y, s, perf = pool_arrays(golden, key)
    c = rec["config"]
    assert c["bootstrap"] == 2000
    host, dev = ES.EvalSuite(draw="host"), ES.EvalSuite(draw="device")
    got = dev.run_one(y, s, c["fake_per_real"], 42, 2000, c["threshold"], perf)
    big = dev.metrics.staged_bytes
    d = worst_difference(rec, got)
    print("%s seed 42, B = 2000, device draw: max |device - recorded| %.3g; draw %s; host seconds %s" % (key, d, dev.metrics.last_draw, dev.timing))
    assert d <= 1e-12
    assert got == host.run_one(y, s, c["fake_per_real"], 42, 2000, c["threshold"], perf)
    assert dev.metrics.readbacks == 1 and dev.metrics.last_draw["consumed"] >= 2000 * got["subset"]["n"]
    small = ES.EvalSuite(draw="device")
    small.run_one(y, s, c["fake_per_real"], 42, 64, c["threshold"], perf)
    sub = got["subset"]
    assert big == small.metrics.staged_bytes <= staging_cap(sub["n"], sub["n_fake"], sub["n_real"])       # whatever B
    assert host.metrics.staged_bytes > 4 * 2000 * sub["n"]                        # the host draw stages every row
    again = dev.run_one(y, s, c["fake_per_real"], 42, 2000, c["threshold"], perf)
    assert json.dumps(again) == json.dumps(got) and dev.metrics.readbacks == 2


def test_run_writes_identical_files_in_both_modes(golden, tmp_path, monkeypatch):
    jobs = []
    for key, ds in (("celebdf", "celebdf"), ("ffpp_percentile", "ffpp")):
        y, s, perf = pool_arrays(golden, key)
        jobs.append((ds, "RetinaFaceDemo", (y, s, *perf)))
    tables = {}
    for mode in ("host", "device"):
        (tmp_path / mode).mkdir()
        monkeypatch.chdir(tmp_path / mode)                                        # the files name their directory: the same relative one
        tables[mode] = ES.EvalSuite(draw=mode).run(jobs, [42, 43], 0.362, bootstrap=64, outdir="suite")
    assert tables["host"][0] == tables["device"][0] and tables["host"][1] == tables["device"][1]
    names = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "host") for d, _, fs in os.walk(tmp_path / "host") for f in fs)
    assert len(names) == 2 * 2 * 2 + 1 and "suite/summary_all.csv" in names
    for name in names:
        assert (tmp_path / "host" / name).read_bytes() == (tmp_path / "device" / name).read_bytes(), name
