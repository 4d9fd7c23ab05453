"""``EvalSuite``: what the reference does with per-video scores - the evaluation protocol of altfreezing/ds.py (one ratio-matched
subset, five stratified folds, a stratified bootstrap of B resamples, mean +- SD over the seeds), ``threshold_from_roc`` of
dualrun/train/thresholds.py and the summary figures of altfreezing/TEST2.py:1115-1137 - without sklearn.

The reference calls ``roc_auc_score`` and ``average_precision_score`` once per resample: two sorts and two curves each.  Here the pool
is sorted ONCE on the host (``np.argsort`` of at most 16 384 floats); a resample is then a vector of draw counts over that order, and
both metrics are sums over the tie groups of the sorted scores:

    U2     = sum_g pos_g (2 (N - fp_g) + neg_g)     an exact integer; AUROC = U2 / (2 P N), one fp64 division on the host
    ap_sum = sum_g pos_g (tp_g / (tp_g + fp_g))     fp64 in a fixed order; AP = ap_sum / P

csrc/af_eval.hip computes them for all rows of a call in one launch, one workgroup per row, the counts in LDS - which bounds a pool at
16 384 items; a larger one is refused with ``ValueError``.  The five folds and the B resamples of ``run_one`` are ONE call: one staging
copy, one launch, one read-back.  The index rows are drawn on the host by the reference's own ``default_rng`` calls in its order -
that is what makes its recorded confidence intervals reproducible, and it is most of what a run still costs.  The results equal
tests/evalsuite_ref.py (numpy) - the integers exactly, ``ap_sum`` bit for bit - and repeat bit for bit.  There is no CPU fallback:
without the HIP library the classes fail.

``EvalSuite(draw="device")`` draws the B resample rows on the GPU instead, from numpy's own PCG64 stream (csrc/af_draw.hip, DESIGN 26;
the numpy statement is tests/pcg64_ref.py): the ``bit_generator.state`` the host has reached after ratio-matching goes to the device,
three launches (scan, resolve, emit) write the rows straight into the buffer the metrics launch reads, and the host sets the
generator to where numpy would have left it.  Same dicts, same files; nothing proportional to B n is staged or touched by the host.
``"host"`` stays the default.  Not built: pools above 16 384, generators other than PCG64, W&B logging, ``batch_eval.py``,
``results/gen_tables.py``."""
import csv
import ctypes as C
import json
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._staging import cuda_device

ROW_DTYPE = np.dtype([("u2", "<i8"), ("ap_sum", "<f8"), ("P", "<i4"), ("N", "<i4"), ("tp_cut", "<i4"), ("fp_cut", "<i4")])
PERF_COLUMNS = ("fps", "latency_ms_clip_mean", "gpu_mem_alloc_peak_mb", "gpu_mem_reserved_peak_mb", "cpu_mem_peak_mb")
PERF_KEYS = ("fps", "latency_ms", "gpu_alloc_mb", "gpu_reserved_mb", "cpu_peak_mb")
FIXED_RATIOS = {"ffpp": 4.0, "celebdf": 1.91, "ffiw": 1.0}             # Fake:Real, ds.py:207-211
SUMMARY_HEADER = ["dataset", "method", "n_avail_real", "n_avail_fake", "fake_per_real", "runs", "auc_mean", "auc_sd", "auc_ci_lo", "auc_ci_hi",
                  "ap_mean", "ap_sd", "ap_ci_lo", "ap_ci_hi", "f1_macro@tau_mean", "f1_macro@tau_sd", "precision_macro@tau_mean",
                  "precision_macro@tau_sd", "recall_macro@tau_mean", "recall_macro@tau_sd", "fps_mean", "fps_p95", "lat_p50", "lat_mean", "lat_p95",
                  "gpu_alloc_p95", "gpu_reserved_p95", "cpu_peak_p95", "out_dir"]
SEED_HEADER = ["seed", "n_pool", "n_real", "n_fake", "threshold", "auc_mean", "auc_sd", "ap_mean", "ap_sd", "f1_macro@tau_mean", "f1_macro@tau_sd",
               "precision_macro@tau_mean", "precision_macro@tau_sd", "recall_macro@tau_mean", "recall_macro@tau_sd"]


PCG64_MULT = 0x2360ED051FC65DA44385DF649FCCF645
DRAW_LIST_SHARE = 4                    # a draw is refused where the expected rejections exceed 1 / 4 of the default list


# ---- numpy's PCG64 state ------------------------------------------------------------------------------------------------

def pcg64_state(rng) -> Tuple[int, int, int, int]:
    """(state, inc, has_uint32, uinteger) of a ``Generator`` over ``PCG64``; any other bit generator is a ``ValueError``"""
    bg = getattr(rng, "bit_generator", None)
    if not isinstance(bg, np.random.PCG64):
        raise ValueError("eval: the device draw restates numpy's PCG64 stream; this generator runs on %s" % type(bg).__name__)
    sd = bg.state
    return int(sd["state"]["state"]), int(sd["state"]["inc"]), int(sd["has_uint32"]), int(sd["uinteger"])


def pcg64_advance(s: int, inc: int, k: int) -> int:
    """the 128-bit state k outputs on: the LCG's O(log k) jump"""
    mask = (1 << 128) - 1
    a, c, A, Cc = PCG64_MULT, inc, 1, 0
    while k:
        if k & 1:
            A, Cc = (A * a) & mask, (Cc * a + c) & mask
        a, c = (a * a) & mask, ((a + 1) * c) & mask
        k >>= 1
    return (A * s + Cc) & mask


# ---- the launch ------------------------------------------------------------------------------------------------------------------------

class Pool:
    """a scored pool resident on the device: ``y`` (1 = fake), ``s``, the stable descending ``order`` and, along it, the scores, the
    tie-group ids and the labels; ``dev`` holds rank_of_item, group_of_rank, every index once (int32 each) and label_of_rank (uint8)"""
    __slots__ = ("n", "y", "s", "order", "sorted_scores", "group_of_rank", "label_of_rank", "group_ends", "dev", "device")

    @property
    def groups(self) -> int:
        return int(self.group_of_rank[-1]) + 1

    def cut(self, threshold) -> int:
        """pool items with ``s >= threshold``: the ranks below it are the predicted positives"""
        return 0 if threshold is None else int(np.count_nonzero(self.s >= threshold))


class RankMetrics:
    """``RankMetrics(device=None)``: AUROC, AP and confusion counts of index rows over one pool, all rows in one launch.

    ``pool(y, s)`` -> a resident ``Pool`` (labels 1 = positive, finite scores; at most 16 384 items, else ``ValueError``).
    ``rows(pool, rows, threshold=None)``: ``rows`` a list of index arrays (items of the pool, any length, repeats allowed) or a
    ``(flat, offsets)`` pair -> dict of numpy arrays ``auc, ap, P, N, tp, fp, tn, fn, u2, ap_sum``, one entry per row; a row with
    ``P N == 0`` has NaN AUROC, one with ``P == 0`` NaN AP; tp .. fn count the draws against ``s >= threshold``.
    ``curve(pool)`` -> ``fpr, tpr, thresholds`` as sklearn's ``roc_curve`` returns them (``drop_intermediate`` applied on the host).
    An index outside the pool is refused before the upload; the kernel skips and counts one all the same, and a non-zero count raises.
    ``drawn_rows(bound_a, count_a, bound_b, count_b, rows, rng, items_a=None, items_b=None, max_rejects=None)`` -> ``(flat int64 rows,
    words consumed)``: what ``rows`` rounds of ``rng.choice(items_a, count_a)``, ``rng.choice(items_b, count_b)`` return (without items:
    ``rng.integers(0, bound, count)``), drawn on the device from ``rng``'s PCG64 state; ``rng`` is left where numpy would leave it.
    ``bootstrap_rows_raw(pool, folds, pos, neg, B, rng, cut)`` -> the records of the fold rows and of B such resamples of ``pos`` and
    ``neg``, drawn and measured on the device: two small staging copies, four launches, one read-back.
    ``staged_bytes`` counts what the row calls copied to the device (a pool's own upload apart)."""

    def __init__(self, device=None):
        from . import _lib                                        # fails loudly when libafhip.so is missing
        self.device = cuda_device(device)
        self.host_check = True
        self._in = self._out = self._dev_in = self._dev_out = self._draw_ws = None
        self.launches = self.uploads = self.readbacks = self.staged_bytes = 0
        self.queued_at = 0.0                                      # perf_counter() when bootstrap_rows_raw had queued its launches
        self.last_draw: Dict[str, int] = {}

    def pool(self, y, s) -> Pool:
        from . import _lib
        y, s = np.asarray(y), np.asarray(s, np.float64)
        if y.ndim != 1 or y.shape != s.shape or y.size == 0:
            raise ValueError("eval: a pool is two equal, non-empty vectors (labels %s, scores %s)" % (y.shape, s.shape))
        if y.size > _lib.RANK_MAX_POOL:
            raise ValueError("eval: a pool of %d items; above %d the draw counts do not fit the LDS of a workgroup" % (y.size, _lib.RANK_MAX_POOL))
        if not np.isfinite(s).all():
            raise ValueError("eval: a pool's scores are finite")
        p = Pool()
        p.n, p.y, p.s, p.device = int(y.size), (y == 1).astype(np.int64), s, self.device
        p.order = np.argsort(-s, kind="stable")
        p.sorted_scores = s[p.order]
        p.group_of_rank = np.concatenate([[0], np.cumsum(p.sorted_scores[1:] != p.sorted_scores[:-1])]).astype(np.int32)
        p.label_of_rank = p.y[p.order].astype(np.uint8)
        p.group_ends = np.flatnonzero(np.concatenate([p.group_of_rank[1:] != p.group_of_rank[:-1], [True]]))
        rank_of_item = np.empty(p.n, np.int32)
        rank_of_item[p.order] = np.arange(p.n, dtype=np.int32)
        words = np.concatenate([rank_of_item, p.group_of_rank, np.arange(p.n, dtype=np.int32)])
        host = np.concatenate([words.view(np.uint8), p.label_of_rank])
        with torch.cuda.device(self.device), torch.inference_mode(False):
            p.dev = torch.from_numpy(host).to(self.device)
        self.uploads += 1
        return p

    # ---- buffers: one pinned pair and one device pair, grown as needed
    def _buffers(self, in_bytes: int, out_bytes: int):
        with torch.inference_mode(False):
            if self._in is None or self._in.numel() < in_bytes:
                cap = max(in_bytes + in_bytes // 4, 1 << 16)
                self._in = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
                self._dev_in = torch.empty(cap, dtype=torch.uint8, device=self.device)
            if self._out is None or self._out.numel() < out_bytes:
                cap = max(out_bytes + out_bytes // 4, 1 << 16)
                self._out = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
                self._dev_out = torch.empty(cap, dtype=torch.uint8, device=self.device)

    def _pool_pointers(self, pool: Pool):
        if not isinstance(pool, Pool) or pool.device != self.device:
            raise ValueError("eval: a pool made by this RankMetrics' pool() on %s" % (self.device,))
        base, n = pool.dev.data_ptr(), pool.n
        return C.c_void_p(base), C.c_void_p(base + 4 * n), C.c_void_p(base + 12 * n), base + 8 * n      # rank, group, label, every index

    def _read_back(self, nbytes: int) -> np.ndarray:
        self._out[:nbytes].copy_(self._dev_out[:nbytes], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self.readbacks += 1
        return self._out[:nbytes].numpy().copy()

    def _finish(self, what: str, nbytes: int, got: Optional[np.ndarray] = None) -> np.ndarray:
        """the one read-back of a call -> the bytes, the error word last"""
        got = self._read_back(nbytes) if got is None else got
        err = int(got[-4:].view(np.int32)[0])
        if err:
            from . import _lib
            raise _lib.AfError("%s: %d indices, ranks or rows left the pool and were skipped: the figures are wrong" % (what, err))
        return got

    def rows_raw(self, pool: Pool, rows, cut: int = 0) -> np.ndarray:
        """the launch: -> a structured array (``ROW_DTYPE``: u2, ap_sum, P, N, tp_cut, fp_cut), one record per row"""
        from . import _lib
        rank, group, label, _ = self._pool_pointers(pool)
        if isinstance(rows, tuple) and len(rows) == 2:
            flat, off = np.asarray(rows[0]).ravel(), np.asarray(rows[1], np.int64).ravel()
            if off.size == 0 or off[0] != 0 or off[-1] != flat.size or (np.diff(off) < 0).any():
                raise ValueError("eval: offsets run from 0 to the %d indices without going back" % flat.size)
        else:
            rows = [np.asarray(r).ravel() for r in rows]
            off = np.zeros(len(rows) + 1, np.int64)
            if rows:
                off[1:] = np.cumsum([r.size for r in rows])
            flat = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        R, n_idx = off.size - 1, int(flat.size)
        if flat.size and flat.dtype.kind not in "iu":
            raise ValueError("eval: indices are integers, got %s" % flat.dtype)
        if not 0 <= int(cut) <= pool.n:
            raise ValueError("eval: cut %d of a pool of %d" % (cut, pool.n))
        if n_idx >= 2 ** 31:
            raise ValueError("eval: %d indices in one call (below 2^31)" % n_idx)
        if self.host_check and n_idx and (int(flat.min()) < 0 or int(flat.max()) >= pool.n):
            raise ValueError("eval: an index outside the pool of %d items" % pool.n)
        if R == 0:
            return np.zeros(0, ROW_DTYPE)
        off_bytes, out_bytes = 8 * (R + 1), ROW_DTYPE.itemsize * R + 8
        with torch.cuda.device(self.device):
            self._buffers(off_bytes + 4 * n_idx, out_bytes)
            stage = self._in.numpy()
            stage[:off_bytes].view(np.int64)[:] = off
            stage[off_bytes:off_bytes + 4 * n_idx].view(np.int32)[:] = flat
            used = off_bytes + 4 * n_idx
            self._dev_in[:used].copy_(self._in[:used], non_blocking=True)
            self.uploads += 1
            self.staged_bytes += used
            base, out = self._dev_in.data_ptr(), self._dev_out.data_ptr()
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.af_rank_metrics_rows(rank, group, label, pool.n, C.c_void_p(base + off_bytes), n_idx, C.c_void_p(base), R, int(cut),
                                                     C.c_void_p(out), C.c_void_p(out + out_bytes - 4), stream), "rank_metrics_rows")
            self.launches += 1
            got = self._finish("rank_metrics_rows", out_bytes)
        return got[:ROW_DTYPE.itemsize * R].view(ROW_DTYPE)

    def rows(self, pool: Pool, rows, threshold=None) -> Dict[str, np.ndarray]:
        return finish_rows(self.rows_raw(pool, rows, pool.cut(threshold)))

    # ---- rows drawn on the device from numpy's PCG64 stream (csrc/af_draw.hip)
    def _draw_plan(self, bound_a, count_a, bound_b, count_b, rows, rng, with_items, max_rejects):
        """every host check of a draw, before anything is staged or launched -> (Pcg64State, (state, inc, has, uinteger), capacity)"""
        from . import _lib
        words = pcg64_state(rng)
        bound_a, count_a, bound_b, count_b, rows = int(bound_a), int(count_a), int(bound_b), int(count_b), int(rows)
        for m in (bound_a, bound_b):
            if not 1 <= m <= 2 ** 32 - 1:
                raise ValueError("eval: a bound of %d (1 to 2^32 - 1: numpy draws the bound 2^32 another way)" % m)
        if count_a < 0 or count_b < 0 or rows < 0:
            raise ValueError("eval: counts %d and %d, %d rows" % (count_a, count_b, rows))
        if rows * (count_a + count_b) >= 2 ** 31:
            raise ValueError("eval: %d rows of %d + %d draws (below 2^31 in one call)" % (rows, count_a, count_b))
        for m, c, has in ((bound_a, count_a, with_items[0]), (bound_b, count_b, with_items[1])):
            if has and m != c:
                raise ValueError("eval: a bound of %d over %d items" % (m, c))
        if max_rejects is None:
            cap = _lib.DRAW_MAX_REJECTS
            active = [(m, c) for m, c in ((bound_a, count_a), (bound_b, count_b)) if m > 1 and c > 0]
            T = rows * sum(c for _, c in active)
            thr = max([2 ** 32 % m for m, _ in active], default=0)
            if DRAW_LIST_SHARE * T * thr > cap * (2 ** 32 - thr):
                raise ValueError("eval: about %d of %d words would be rejected (2^32 mod bound = %d); the list of %d holds %d x that at most"
                                 % (T * thr // (2 ** 32 - thr), T, thr, cap, DRAW_LIST_SHARE))
        else:
            cap = int(max_rejects)
            if not 1 <= cap <= _lib.DRAW_MAX_REJECTS:
                raise ValueError("eval: a rejection list of %d entries (1 to %d)" % (cap, _lib.DRAW_MAX_REJECTS))
        s, inc, has, uinteger = words
        m64 = (1 << 64) - 1
        return _lib.Pcg64State(s >> 64, s & m64, inc >> 64, inc & m64, has, uinteger), words, cap

    def _launch_draw(self, start, bounds, rows, items, cap, idx_ptr, row_off_ptr, row_base, result_ptr):
        """queues the three draw launches on the current stream"""
        from . import _lib
        need = int(_lib.lib.af_pcg64_draw_workspace_bytes(cap))
        with torch.inference_mode(False):
            if self._draw_ws is None or self._draw_ws.numel() < need:
                self._draw_ws = torch.empty(int(_lib.lib.af_pcg64_draw_workspace_bytes(_lib.DRAW_MAX_REJECTS)), dtype=torch.uint8, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.lib.af_pcg64_draw_rows(C.byref(start), bounds[0], bounds[1], bounds[2], bounds[3], rows, C.c_void_p(items[0]),
                                               C.c_void_p(items[1]), cap, C.c_void_p(idx_ptr), C.c_void_p(row_off_ptr), row_base,
                                               C.c_void_p(result_ptr), C.c_void_p(self._draw_ws.data_ptr()), self._draw_ws.numel(), stream),
                   "pcg64_draw_rows")
        self.launches += 3

    def _finish_draw(self, raw: np.ndarray, words, rng) -> int:
        """the read-back ``af_draw_result``: raises where the list overflowed, else moves ``rng`` to numpy's final state -> words consumed"""
        from . import _lib
        r = _lib.DrawResult.from_buffer_copy(raw.tobytes())
        self.last_draw = {k: int(getattr(r, k)) for k in ("consumed", "outputs", "has_uint32", "uinteger", "rejected", "listed", "error")}
        if r.error:
            raise _lib.AfError("pcg64_draw_rows: error %d with %d words listed for rejection: the list overflowed and no rows were drawn" % (
                r.error, r.listed))
        s, inc, has, uinteger = words
        if r.consumed > 0 and r.outputs != (r.consumed - has + 1) // 2:
            raise _lib.AfError("pcg64_draw_rows: %d outputs for %d words" % (r.outputs, r.consumed))
        if r.consumed > 0:
            rng.bit_generator.state = {"bit_generator": "PCG64", "state": {"state": pcg64_advance(s, inc, int(r.outputs)), "inc": inc},
                                       "has_uint32": int(r.has_uint32), "uinteger": int(r.uinteger)}
        return int(r.consumed)

    def drawn_rows(self, bound_a, count_a, bound_b, count_b, rows, rng, items_a=None, items_b=None, max_rejects=None):
        """the draw alone, rows back on the host (tests and debugging) -> (flat int64 array in numpy's order, words consumed)"""
        from . import _lib
        items = [None if it is None else np.ascontiguousarray(np.asarray(it).ravel(), np.int32) for it in (items_a, items_b)]
        counts = [int(count_a), int(count_b)]
        for i, it in enumerate(items):
            if it is not None and len(it) != int((bound_a, bound_b)[i]):
                raise ValueError("eval: a bound of %d over %d items" % ((bound_a, bound_b)[i], len(it)))
        start, words, cap = self._draw_plan(bound_a, counts[0], bound_b, counts[1], rows, rng, [it is not None for it in items], max_rejects)
        rows, n = int(rows), int(rows) * (counts[0] + counts[1])
        with torch.cuda.device(self.device), torch.inference_mode(False):
            dev = [None if it is None or len(it) == 0 else torch.from_numpy(it).to(self.device) for it in items]
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
            off = torch.empty(rows + 1, dtype=torch.int64, device=self.device)
            res = torch.empty(C.sizeof(_lib.DrawResult), dtype=torch.uint8, device=self.device)
            self._launch_draw(start, (int(bound_a), counts[0], int(bound_b), counts[1]), rows, [0 if d is None else d.data_ptr() for d in dev],
                              cap, idx.data_ptr(), off.data_ptr(), 0, res.data_ptr())
            raw, flat, table = res.cpu().numpy(), idx[:n].cpu().numpy(), off.cpu().numpy()
            self.readbacks += 1
        consumed = self._finish_draw(raw, words, rng)
        if not np.array_equal(table, np.arange(rows + 1, dtype=np.int64) * (counts[0] + counts[1])):
            raise _lib.AfError("pcg64_draw_rows: a wrong row table")
        out = flat.astype(np.int64)
        for (lo, hi), it in zip(((0, counts[0]), (counts[0], counts[0] + counts[1])), items):
            if it is None and n:                                             # value mode: the uint32 draw itself
                v = out.reshape(rows, -1)
                v[:, lo:hi] &= 0xffffffff
        return out, consumed

    def bootstrap_rows_raw(self, pool: Pool, folds, pos, neg, B: int, rng, cut: int = 0) -> np.ndarray:
        """the fold rows and B resamples ``[rng.choice(pos, len(pos)), rng.choice(neg, len(neg))]`` of the pool: the resamples are drawn
        on the device behind the fold rows and one ``af_rank_metrics_rows`` call covers both -> ``ROW_DTYPE`` records, folds first.
        Staged: the fold rows and their offsets, ``pos`` and ``neg``; read back once: the records, the draw's result, the error word."""
        from . import _lib
        rank, group, label, _ = self._pool_pointers(pool)
        folds = [np.asarray(f).ravel() for f in folds]
        pos, neg, B = np.asarray(pos).ravel(), np.asarray(neg).ravel(), int(B)
        F, a, b = len(folds), int(pos.size), int(neg.size)
        for v in folds + [pos, neg]:
            if v.size and v.dtype.kind not in "iu":
                raise ValueError("eval: indices are integers, got %s" % v.dtype)
            if self.host_check and v.size and (int(v.min()) < 0 or int(v.max()) >= pool.n):
                raise ValueError("eval: an index outside the pool of %d items" % pool.n)
        if not 0 <= int(cut) <= pool.n:
            raise ValueError("eval: cut %d of a pool of %d" % (cut, pool.n))
        if B < 0 or a < 1 or b < 1:
            raise ValueError("eval: %d resamples of %d positives and %d negatives" % (B, a, b))
        start, words, cap = self._draw_plan(a, a, b, b, B, rng, [True, True], None)
        fold_off = np.full(F + 1, a + b, np.int64)                            # idx: pos, neg, the fold rows, then the rows drawn here -
        if F:                                                                 # the rows of one table follow one another
            fold_off[1:] += np.cumsum([f.size for f in folds])
        row_base = int(fold_off[-1])
        R, n_idx = F + B, row_base + B * (a + b)
        if n_idx >= 2 ** 31:
            raise ValueError("eval: %d indices in one call (below 2^31)" % n_idx)
        off_bytes, rec_bytes = 8 * (R + 1), ROW_DTYPE.itemsize * R
        res_bytes = C.sizeof(_lib.DrawResult)
        out_bytes = rec_bytes + res_bytes + 8                                 # records, af_draw_result, padding, the error word last
        with torch.cuda.device(self.device):
            self._buffers(off_bytes + 4 * n_idx, out_bytes)
            stage = self._in.numpy()
            head = 8 * (F + 1)
            stage[:head].view(np.int64)[:] = fold_off
            staged = stage[head:head + 4 * row_base].view(np.int32)
            staged[:] = np.concatenate([pos, neg] + folds)
            self._dev_in[:head].copy_(self._in[:head], non_blocking=True)
            self._dev_in[off_bytes:off_bytes + 4 * row_base].copy_(self._in[head:head + 4 * row_base], non_blocking=True)
            self.uploads += 2
            self.staged_bytes += head + 4 * row_base
            base, out = self._dev_in.data_ptr(), self._dev_out.data_ptr()
            idx = base + off_bytes
            self._launch_draw(start, (a, a, b, b), B, [idx, idx + 4 * a], cap, idx + 4 * row_base, base + 8 * F, row_base, out + rec_bytes)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.af_rank_metrics_rows(rank, group, label, pool.n, C.c_void_p(idx), n_idx, C.c_void_p(base), R, int(cut),
                                                     C.c_void_p(out), C.c_void_p(out + out_bytes - 4), stream), "rank_metrics_rows")
            self.launches += 1
            self.queued_at = time.perf_counter()
            got = self._read_back(out_bytes)
        self._finish_draw(got[rec_bytes:rec_bytes + res_bytes], words, rng)
        self._finish("rank_metrics_rows", out_bytes, got)
        return got[:rec_bytes].view(ROW_DTYPE)

    def curve_counts(self, pool: Pool) -> Tuple[np.ndarray, np.ndarray]:
        """cumulative (tps, fps) at every tie group's end over the whole pool, each item drawn once: the integer ROC curve"""
        from . import _lib
        rank, group, label, every = self._pool_pointers(pool)
        n = pool.n
        out_bytes = 8 * n + 8
        with torch.cuda.device(self.device):
            self._buffers(0, out_bytes)
            out = self._dev_out.data_ptr()
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.af_rank_curve(rank, group, label, n, C.c_void_p(every), n, C.c_void_p(out), C.c_void_p(out + 4 * n),
                                              C.c_void_p(out + 8 * n), C.c_void_p(out + 8 * n + 4), stream), "rank_curve")
            self.launches += 1
            words = self._finish("rank_curve", out_bytes).view(np.int32)
        G = int(words[2 * n])
        if G != pool.groups:
            raise _lib.AfError("rank_curve: %d tie groups on the device, %d on the host" % (G, pool.groups))
        return words[:G].copy(), words[n:n + G].copy()

    def curve(self, pool: Pool):
        return roc_from_counts(*self.curve_counts(pool), pool)[:3]


def finish_rows(raw: np.ndarray) -> Dict[str, np.ndarray]:
    """the host's part behind the launch: two divisions per row and the confusion counts"""
    P, N = raw["P"].astype(np.int64), raw["N"].astype(np.int64)
    u2, ap_sum = raw["u2"].copy(), raw["ap_sum"].copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        auc = np.where(P * N > 0, u2.astype(np.float64) / (2 * P * N).astype(np.float64), np.nan)
        ap = np.where(P > 0, ap_sum / P.astype(np.float64), np.nan)
    tp, fp = raw["tp_cut"].astype(np.int64), raw["fp_cut"].astype(np.int64)
    return {"auc": auc, "ap": ap, "P": P, "N": N, "tp": tp, "fp": fp, "tn": N - fp, "fn": P - tp, "u2": u2, "ap_sum": ap_sum}


def macro_at(tp, fp, tn, fn) -> Tuple[float, float, float]:
    """sklearn's precision_score / recall_score / f1_score(average="macro", zero_division=0) of a binary problem from its four
    counts: a class counts when it is in the truth or in the predictions; a 0 / 0 is 0 -> (precision, recall, f1)"""
    tp, fp, tn, fn = int(tp), int(fp), int(tn), int(fn)
    pr, rc, f1 = [], [], []
    for hit, pred, true in ((tn, tn + fn, tn + fp), (tp, tp + fp, tp + fn)):
        if pred + true == 0:
            continue
        pr.append(hit / pred if pred else 0.0)
        rc.append(hit / true if true else 0.0)
        f1.append(2 * hit / (pred + true))
    return float(np.mean(pr)), float(np.mean(rc)), float(np.mean(f1))


_metrics: Dict[torch.device, RankMetrics] = {}


def _rank_metrics(device=None) -> RankMetrics:
    dev = cuda_device(device)
    if dev not in _metrics:
        _metrics[dev] = RankMetrics(dev)
    return _metrics[dev]


# ---- thresholds (dualrun/train/thresholds.py) ---------------------------------------------------------------------------------------------

def roc_from_counts(tps, fps, pool: Pool):
    """``roc_curve`` from the integer curve: drop_intermediate (first, last and every point where a second difference of fps or tps
    is non-zero), the origin with threshold inf in front -> (fpr, tpr, thresholds, kept tps, kept fps)"""
    tps, fps = np.asarray(tps, np.int64), np.asarray(fps, np.int64)
    thr = pool.sorted_scores[pool.group_ends]
    if len(fps) > 2:
        keep = np.flatnonzero(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])
        tps, fps, thr = tps[keep], fps[keep], thr[keep]
    tps, fps, thr = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thr]
    fpr = fps / fps[-1] if fps[-1] > 0 else np.full(len(fps), np.nan)
    tpr = tps / tps[-1] if tps[-1] > 0 else np.full(len(tps), np.nan)
    return fpr, tpr, thr, tps, fps


def stats_from_counts(tp, fp, P, N) -> Dict:
    """``_stats_at_threshold`` from the confusion counts"""
    tp, fp, P, N = int(tp), int(fp), int(P), int(N)
    fn, tn = P - tp, N - fp
    TPR, FPR = tp / max(tp + fn, 1), fp / max(fp + tn, 1)
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return {"tn": tn, "fp": fp, "fn": fn, "tp": tp, "TPR": TPR, "FPR": FPR, "balacc": 0.5 * (TPR + (1.0 - FPR)), "youden": TPR - FPR,
            "acc": (tp + tn) / (P + N), "f1": f1}


def threshold_from_roc(probs, y, metric: str = "youden", target_fpr: Optional[float] = None, device=None):
    """the reference's ``threshold_from_roc`` -> ``(best_t, stats)``.  The curve's counts come from one launch; a point's statistics
    are its own ``(tps, fps)``, so the ``acc`` and ``f1`` searches cost no pass over the samples per threshold."""
    rm = _rank_metrics(device)
    pool = rm.pool(y, probs)
    fpr, tpr, thr, tps, fps = roc_from_counts(*rm.curve_counts(pool), pool)
    P, N = int(tps[-1]), int(fps[-1])
    if target_fpr is not None:
        mask = fpr <= float(target_fpr)
        idx = int(np.argmin(fpr)) if not np.any(mask) else int(np.arange(len(fpr))[mask][int(np.argmax(tpr[mask]))])
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


# ---- TEST2.main's summary -----------------------------------------------------------------------------------------------------------------

def video_table(y_true, y_score, threshold, y_pred=None, device=None) -> Dict:
    """the figures of altfreezing/TEST2.py:1123-1128: accuracy, AUROC (NaN when one class), AP, F1 and the confusion matrix.
    ``y_pred`` None: ``score > threshold``, the rule of the runner's per-person label."""
    y_true, y_score = np.asarray(y_true).astype(np.int64), np.asarray(y_score, np.float64)
    y_pred = (y_score > threshold).astype(np.int64) if y_pred is None else np.asarray(y_pred).astype(np.int64)
    rm = _rank_metrics(device)
    pool = rm.pool(y_true, y_score)
    r = rm.rows(pool, [np.arange(pool.n)])
    tp, tn = int(((y_true == 1) & (y_pred == 1)).sum()), int(((y_true == 0) & (y_pred == 0)).sum())
    fp, fn = int(((y_true == 0) & (y_pred == 1)).sum()), int(((y_true == 1) & (y_pred == 0)).sum())
    labels = sorted(set(y_true.tolist()) | set(y_pred.tolist()))
    cm = [[int(((y_true == a) & (y_pred == b)).sum()) for b in labels] for a in labels]
    P, n = tp + fn, int(y_true.size)
    return {"videos": n, "accuracy": (tp + tn) / n, "auc_roc": float(r["auc"][0]) if 0 < P < n else float("nan"),
            "pr_auc": float(r["ap"][0]) if P > 0 else 0.0, "f1": 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0,
            "tp": tp, "tn": tn, "fp": fp, "fn": fn, "confusion_matrix": cm}


# ---- altfreezing/ds.py --------------------------------------------------------------------------------------------------------------------

def load_per_video(path):
    """``ds.load_per_video``: (y_true, y_score, fps, latency, gpu_alloc, gpu_reserved, cpu_peak); a missing or unreadable perf cell is NaN"""
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


def summarize_perf(x) -> Dict[str, float]:
    x = np.asarray(x, float)
    x = x[np.isfinite(x)]
    if x.size == 0:
        return {"mean": np.nan, "p50": np.nan, "p95": np.nan}
    return {"mean": float(np.mean(x)), "p50": float(np.percentile(x, 50)), "p95": float(np.percentile(x, 95))}


def pick_counts(nR: int, nF: int, fake_per_real: float) -> Tuple[int, int]:
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
    if nR == 0 or nF == 0:
        raise ValueError("Campioni insufficienti dopo ratio-matching.")
    sel_R = rng.choice(real_idx, size=nR, replace=False)
    sel_F = rng.choice(fake_idx, size=nF, replace=False)
    return np.concatenate([sel_R, sel_F])


def stratified_test_folds(y, seed: int, n_splits: int = 5) -> List[np.ndarray]:
    """the test index sets of ``StratifiedKFold(n_splits, shuffle=True, random_state=seed).split(y, y)``, in fold order: the sorted
    encoded labels dealt round-robin give every fold its count per class, and ``RandomState(seed)`` shuffles each class's fold vector"""
    y = np.asarray(y)
    if n_splits > y.size:
        raise ValueError("Cannot have number of splits n_splits=%d greater than the number of samples: n_samples=%d." % (n_splits, y.size))
    rng = np.random.RandomState(seed)
    _, y_idx, y_inv = np.unique(y, return_index=True, return_inverse=True)
    _, class_perm = np.unique(y_idx, return_inverse=True)
    y_encoded = class_perm[y_inv]                                             # classes in order of first appearance
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


def mean_sd(a) -> Tuple[float, float]:
    x = np.asarray(a, float)
    return float(np.nanmean(x)), float(np.nanstd(x, ddof=1))


def make_config(per_video, dataset, method, fake_per_real, bootstrap=2000, seed=42, outdir="results_suite", threshold=0.04) -> Dict:
    """``asdict(EvalConfig(...))``, key for key"""
    return {"per_video": per_video, "dataset": dataset, "method": method, "fake_per_real": fake_per_real, "bootstrap": bootstrap, "seed": seed,
            "outdir": outdir, "threshold": threshold, "wandb": False, "wandb_project": None, "wandb_entity": None}


def infer_ratio(ds: str, y) -> float:
    if FIXED_RATIOS.get(ds) is not None:
        return FIXED_RATIOS[ds]
    y = np.asarray(y)
    return float(int((y == 1).sum()) / max(1, int((y == 0).sum())))


def seed_row(seed, threshold, result) -> list:
    """the data row of ``metrics_seed*.csv``"""
    mm, subs = result["metrics_mean_sd"], result["subset"]
    return [seed, subs["n"], subs["n_real"], subs["n_fake"], threshold] + [mm[k] for k in SEED_HEADER[5:]]


def summary_row(ds, method, fpr, results, out_dir) -> list:
    """a row of ``summary_all.csv``: mean and SD over the seeds' means; the CI and the hardware figures of the LAST seed, as ds.main
    reports them"""
    mm, last = [r["metrics_mean_sd"] for r in results], results[-1]
    auc, ap, f1 = mean_sd([m["auc_mean"] for m in mm]), mean_sd([m["ap_mean"] for m in mm]), mean_sd([m["f1_macro@tau_mean"] for m in mm])
    prec, rec = mean_sd([m["precision_macro@tau_mean"] for m in mm]), mean_sd([m["recall_macro@tau_mean"] for m in mm])
    hw, bs = last["hardware_stats"], last["bootstrap_ci"]
    return [ds, method, last["counts_available"]["real"], last["counts_available"]["fake"], fpr, len(results),
            auc[0], auc[1], bs["auc_ci95"][0], bs["auc_ci95"][1], ap[0], ap[1], bs["ap_ci95"][0], bs["ap_ci95"][1],
            f1[0], f1[1], prec[0], prec[1], rec[0], rec[1], hw["fps"]["mean"], hw["fps"]["p95"], hw["latency_ms"]["p50"],
            hw["latency_ms"]["mean"], hw["latency_ms"]["p95"], hw["gpu_alloc_mb"]["p95"], hw["gpu_reserved_mb"]["p95"], hw["cpu_peak_mb"]["p95"], out_dir]


class EvalSuite:
    """``EvalSuite(device=None, draw="host")``: ``python ds.py`` on the GPU.

    ``run_one(y, s, fake_per_real, seed, bootstrap=2000, threshold=0.04, perf=None)`` -> ``ds.run_one``'s dict (``counts_available``,
    ``subset``, ``metrics_mean_sd``, ``bootstrap_ci``, ``per_fold``, ``hardware_stats``; ``config`` echoes the arguments): the subset,
    the folds and the resamples are drawn on the host as the reference draws them, the 5 + B rows are one ``RankMetrics.rows`` call,
    the percentiles are ``np.nanpercentile``.  ``perf``: the five perf columns of ``load_per_video``, or None.  ``ValueError`` where
    the reference raises: a class missing from the table or from a fold, nothing left after ratio-matching.
    ``run(jobs, seeds, threshold, bootstrap=2000, outdir=None)``: ``ds.main`` over ``jobs = [(dataset, method, per_video)]``, per_video
    a CSV path or the tuple ``load_per_video`` returns (or ``(y, s)``) -> ``(rows of summary_all.csv, header first,
    {(dataset, method): [run_one's dict per seed]})``; with ``outdir`` it writes ``<dataset>/<method>/summary_seed*.json``,
    ``metrics_seed*.csv`` and ``summary_all.csv`` in the reference's formats.  No W&B.
    ``timing`` holds the host seconds of the last ``run_one``: ``draw`` (the index rows), ``rows`` (staging, launch, read-back) and ``total``.
    ``draw="device"``: the B resamples are drawn on the GPU from the same PCG64 stream (``RankMetrics.bootstrap_rows_raw``) - the same
    dicts and files; ``timing["draw"]`` is then the time until the launches are queued, ``rows`` the wait and the read-back."""

    def __init__(self, device=None, draw: str = "host"):
        if draw not in ("host", "device"):
            raise ValueError("eval: draw is 'host' or 'device', got %r" % (draw,))
        self.draw = draw
        self.metrics = RankMetrics(device)
        self.device = self.metrics.device
        self.timing: Dict[str, float] = {}

    load_per_video = staticmethod(load_per_video)

    def run_one(self, y, s, fake_per_real, seed, bootstrap=2000, threshold=0.04, perf=None, config: Optional[Dict] = None) -> Dict:
        t0 = time.perf_counter()
        y, s = np.asarray(y), np.asarray(s, float)
        rng = np.random.default_rng(seed)
        idx_pool = ratio_match_indices(y, fake_per_real, rng)
        yt_pool, st_pool = y[idx_pool], s[idx_pool]
        folds = stratified_test_folds(yt_pool, seed)
        pos, neg = np.where(yt_pool == 1)[0], np.where(yt_pool == 0)[0]
        if self.draw == "device":
            pool = self.metrics.pool(yt_pool, st_pool)
            res = finish_rows(self.metrics.bootstrap_rows_raw(pool, folds, pos, neg, bootstrap, rng, pool.cut(threshold)))
            t1 = self.metrics.queued_at
        else:
            boots = [np.concatenate([rng.choice(pos, len(pos), True), rng.choice(neg, len(neg), True)]) for _ in range(bootstrap)]
            t1 = time.perf_counter()
            pool = self.metrics.pool(yt_pool, st_pool)
            res = self.metrics.rows(pool, folds + boots, threshold)
        t2 = time.perf_counter()
        per_fold, precL, recL, f1L = [], [], [], []
        for k in range(len(folds)):
            if res["P"][k] == 0 or res["N"][k] == 0:
                raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
            prec, rec, f1m = macro_at(res["tp"][k], res["fp"][k], res["tn"][k], res["fn"][k])
            per_fold.append({"fold": k + 1, "n": int(res["P"][k] + res["N"][k]), "n_real": int(res["N"][k]), "n_fake": int(res["P"][k]),
                             "auc": float(res["auc"][k]), "ap": float(res["ap"][k]), "f1_macro_at_tau": f1m, "precision_macro_at_tau": prec,
                             "recall_macro_at_tau": rec})
            precL.append(prec); recL.append(rec); f1L.append(f1m)
        aucL, apL = [f["auc"] for f in per_fold], [f["ap"] for f in per_fold]
        auc_bs, ap_bs = res["auc"][len(folds):], res["ap"][len(folds):]
        lo_auc, hi_auc = np.nanpercentile(auc_bs, [2.5, 97.5]) if len(auc_bs) else (np.nan, np.nan)
        lo_ap, hi_ap = np.nanpercentile(ap_bs, [2.5, 97.5]) if len(ap_bs) else (np.nan, np.nan)
        perf = perf if perf is not None else [np.zeros(0)] * 5
        out = {
            "config": dict(config) if config is not None else make_config(None, None, None, fake_per_real, bootstrap, seed, None, threshold),
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
        t3 = time.perf_counter()
        self.timing = {"draw": t1 - t0, "rows": t2 - t1, "total": t3 - t0}
        return out

    def run(self, jobs: Sequence, seeds: Sequence[int], threshold: float, bootstrap: int = 2000, outdir: Optional[str] = None):
        out_rows, results = [list(SUMMARY_HEADER)], {}
        for ds, method, per_video in jobs:
            is_path = isinstance(per_video, (str, os.PathLike))
            data = load_per_video(per_video) if is_path else tuple(per_video)
            y, s, perf = data[0], data[1], (data[2:7] if len(data) >= 7 else None)
            fpr = infer_ratio(ds, y)
            out_dir_ds = os.path.join(outdir, ds, method) if outdir is not None else None
            if out_dir_ds is not None:
                os.makedirs(out_dir_ds, exist_ok=True)
            per_seed = []
            for sd in seeds:
                cfg = make_config(per_video if is_path else None, ds, method, fpr, bootstrap, sd, out_dir_ds, threshold)
                result = self.run_one(y, s, fpr, sd, bootstrap, threshold, perf, cfg)
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
