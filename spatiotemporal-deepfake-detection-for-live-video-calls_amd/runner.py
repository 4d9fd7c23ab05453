"""The dataset evaluator's per-video loop on the MI355X: a video's frames in, what ``VideoRunner.run`` of the reference's
altfreezing/TEST2.py (:303-797, driven by batch_eval.py) returns out - the loop that produced the reference's own pipeline table.

``VideoRunner(network, detector).run(frames, fps, total_frames)`` restates that method as it is written, odd parts included (each
is marked "as written" where it stands), over device stages that already exist: YuNet on resident frames, the quality gate
(csrc/af_quality.hip, both of its modes), the window warp out of a frame store and ``LiveScorer`` replays.  Where the live step
(``live.RealtimeCall``) waits for the device twice per frame, this loop takes the frames ``detect_batch`` at a time: below the
tracker (:540) nothing of the host stage depends on a quality result or a score, so a chunk goes through ONE detect, one round of
host tracking, one half-size quality launch per 64 crop rectangles of the whole chunk, and the shared scoring.  With
``tracker="device"`` that round of host tracking is one launch on the detector's rows where they lie (csrc/af_runner_core.h),
the quality launch takes its rectangles from that launch's record in device memory, and a chunk waits for the device once.

Not built: ``cv2.VideoCapture`` (the caller decodes; ``frames`` is what ``cap.read()`` gives), FaceMesh (``landmarks`` is the hook
where the reference has it; without it the loop behaves as the reference does when FaceMesh finds nothing), the CSV and metrics
code of ``TEST2.main``, and ``flush_and_infer``'s skip of a clip whose alignment raises (a crop here is a rectangle of its frame and
always fits its canvas; a planner refusal raises).  There is no CPU fallback: without the HIP library ``run`` fails.
"""
import ctypes as C
import platform
import time
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch

from . import live
from ._staging import is_crop
from .aligner import STD_POINTS_256, fit_window
from .frames import YuvFrame
from .evaluator import _POOL_SLACK, _FrameTrack, get_crop_box
from .tracker import ByteTracker, STrack, iou_distance

try:
    import resource
except ImportError:                                        # only on Unix (:21-24)
    resource = None

# TEST2.py:963-1042: the argparse names that reach ``run``, with their defaults
DEFAULTS = dict(
    optimal_threshold=0.4, max_frame=400, clip_size=32, crop_scale=1.0, conf=0.7, track_thresh=0.6, track_buffer=2000, match_thresh=0.6,
    detect_every=3, stride=5, smart_start=False, start_after_n=5, start_conf=0.6, start_min_size=20, mesh_every=3, q_weighting=True,
    q_min_size_soft=72, q_min_size_hard=48, q_lap_soft=24, q_lap_hard=8, batch_clips=8, pool_method="median", percentile_p=70.0,
    trim_ratio=0.2, topk_ratio=0.3, min_clips=1, verbose_pool=False, disable_penalty=False, qa_min_side=240, qa_min_lap=16.0,
    qa_q75_thr=0.30, qa_q90_thr=0.90, min_det_side=80, min_det_area=4000, exclude_bottom_frac=0.10, min_track_side=96)
# ... and those accepted for a caller that passes ``vars(args)``, which nothing here reads: input / output, the checkpoint, the
# detector's input size (YuNet here reads the frame at its own size, as :346 sets it), FaceMesh, autocast
UNUSED = ("dataset_root", "out_csv_pervideo", "out_csv_summary", "list_path", "cfg_path", "ckpt_path", "detector_res", "dump_clip_scores",
          "dump_track_scores", "roi_scale", "mp_min_det", "mp_min_trk", "refine_size", "amp", "channels_last")
OWN = dict(size=224, max_batch=16, frame_bytes=4 << 30, channel_order="bgr", detect_batch=16, landmarks=None, tracker="host")
TRACKERS = ("host", "device")
POOL_METHODS = ("median", "mean", "topk", "topk_median", "percentile", "trimmed_mean", "logit_median", "adaptive")
QSTAT_MAX = 50                                             # :297


# ---- after the loop: TEST2.py:627-797 ---------------------------------------------------------------------------------------------

def score_with_stability(scores, base: float) -> float:
    """:627-634: ``base`` damped by 0.85 ** (spread / 0.25) when the series is unstable - the spread is the 85th minus the 25th
    percentile, called iqr there (as written) - and its median is below 0.85; 0.0 for no scores"""
    s = np.asarray(scores, float)
    if s.size == 0:
        return 0.0
    iqr = np.percentile(s, 85) - np.percentile(s, 25)
    if iqr > 0.25 and np.median(s) < 0.85:
        return base * (0.85 ** (iqr / 0.25))
    return base


def _logit_median(s: np.ndarray) -> float:
    se = np.clip(s, 1e-6, 1 - 1e-6)
    med = np.median(np.log(se / (1 - se)))
    return float(1 / (1 + np.exp(-med)))


def pool_track(scores, method: str = "median", topk_ratio: float = 0.2, percentile_p: float = 80.0, trim_ratio: float = 0.2) -> float:
    """:636-683, ``_pool_track``: a track's clip scores -> one score, by one of ``POOL_METHODS``; 0.0 for no scores; a method it
    does not know falls back to the median (as written)"""
    s = np.asarray(scores, float)
    if s.size == 0:
        return 0.0
    if method == "mean":
        return float(np.mean(s))
    if method == "median":
        return float(np.median(s))
    if method == "logit_median":
        return _logit_median(s)
    if method in ("topk", "topk_median"):
        k = max(1, int(np.ceil(topk_ratio * s.size)))
        top = np.sort(s)[-k:]
        return float(np.mean(top) if method == "topk" else np.median(top))
    if method == "percentile":
        return float(np.percentile(s, float(np.clip(percentile_p, 0.0, 100.0))))
    if method == "trimmed_mean":
        t = float(np.clip(trim_ratio, 0.0, 0.49))
        ss = np.sort(s)
        a = int(ss.size * t)
        return float(np.mean(ss[a:max(a + 1, ss.size - a)]))
    if method == "adaptive":                               # a narrow distribution: the high percentile; else the logit median
        if np.percentile(s, 75) - np.percentile(s, 25) < 0.15:
            return float(np.percentile(s, float(np.clip(percentile_p, 0.0, 100.0))))
        return _logit_median(s)
    return float(np.median(s))


def low_quality_rule(qstat, qa_min_side: float = 240, qa_min_lap: float = 16.0):
    """:685-694: ``(low_quality, median min side, median full-size Laplacian variance)`` of the ``_qstat`` records ``(min side,
    lap)``; ``(False, None, None)`` without one"""
    if not qstat:
        return False, None, None
    ms = np.array(qstat, float)
    side, lap = float(np.median(ms[:, 0])), float(np.median(ms[:, 1]))
    return bool(side < qa_min_side or lap < qa_min_lap), side, lap


def track_quantiles(track_clip_scores) -> Dict:
    """:722-728: per track with a score the 10 / 25 / 50 / 75 / 90th percentiles"""
    out = {}
    for tid, ss in track_clip_scores.items():
        s = np.array(ss, float)
        if s.size:
            qs = np.percentile(s, [10, 25, 50, 75, 90])
            out[tid] = {"q10": float(qs[0]), "q25": float(qs[1]), "q50": float(qs[2]), "q75": float(qs[3]), "q90": float(qs[4])}
    return out


def person_scores(track_clip_scores, pool_method: str = "median", topk_ratio: float = 0.3, percentile_p: float = 70.0,
                  trim_ratio: float = 0.2, min_clips: int = 1, disable_penalty: bool = False):
    """:703-714: ``(raw_scores, per_person)`` - the pooled and the stability-damped score of every track with ``min_clips`` clips"""
    raw_scores, per_person = {}, {}
    for tid, scores in track_clip_scores.items():
        if len(scores) < min_clips:
            continue
        raw = pool_track(scores, method=pool_method, topk_ratio=topk_ratio, percentile_p=percentile_p, trim_ratio=trim_ratio)
        pen = raw if disable_penalty else score_with_stability(scores, raw)
        raw_scores[tid], per_person[tid] = float(raw), float(pen)
    return raw_scores, per_person


def person_labels(per_person, quants, low_quality: bool, optimal_threshold: float = 0.4, qa_q75_thr: float = 0.30, qa_q90_thr: float = 0.90):
    """:731-746: ``(standard, QA, fused)`` labels per track: the standard one is ``score > threshold``; the QA one - only for a
    low-quality video - ``q75 >= qa_q75_thr or q90 >= qa_q90_thr``; the fused one their OR"""
    std = {tid: int(per_person[tid] > optimal_threshold) for tid in per_person}
    if low_quality:
        qa = {}
        for tid in per_person:
            q = quants.get(tid)
            qa[tid] = int(bool(q and (q["q75"] >= qa_q75_thr or q["q90"] >= qa_q90_thr)))
    else:
        qa = {tid: 0 for tid in per_person}
    return std, qa, {tid: int(std.get(tid, 0) or qa.get(tid, 0)) for tid in per_person}


def video_verdict(track_clip_scores, qstat, args) -> dict:
    """:685-749 as one call: ``args`` has the attributes ``DEFAULTS`` names.  ``video_score`` is the largest RAW track score,
    whatever the penalty and the labels say (as written: it feeds the AUC)"""
    low, med_side, med_lap = low_quality_rule(qstat, args.qa_min_side, args.qa_min_lap)
    raw, per_person = person_scores(track_clip_scores, args.pool_method, args.topk_ratio, args.percentile_p, args.trim_ratio, args.min_clips,
                                    args.disable_penalty)
    quants = track_quantiles(track_clip_scores)
    std, qa, fused = person_labels(per_person, quants, low, args.optimal_threshold, args.qa_q75_thr, args.qa_q90_thr)
    return {"video_score": float(max(raw.values())) if raw else 0.0, "pred_label": int(any(v == 1 for v in fused.values())),
            "num_tracks": len(per_person), "per_person_scores": per_person, "per_person_labels": fused, "per_person_labels_std": std,
            "per_person_labels_qa": qa, "track_quantiles": quants, "low_quality": low, "q_med_min_side": med_side, "q_med_lap": med_lap}


# ---- in front of the loop: TEST2.py:328-340, :442-480 -----------------------------------------------------------------------------

def sane_fps(fps) -> float:
    """:329-331: a missing rate, or one outside [5, 240], is 30"""
    fps = float(fps or 30.0)
    return 30.0 if fps < 5 or fps > 240 else fps


def detect_rhythm(detect_every: int, fps: float) -> int:
    """:337-340: the caller's when positive, else adaptive, about fps / 8 within [1, 8]"""
    return int(detect_every) if detect_every > 0 else max(1, min(8, round(fps / 8)))


class WindowPlan:
    """:442-480: which frames of the video are read at all (``keep``), the window a frame lies in (``window_id``, the FIRST range that
    holds it - the ranges overlap whenever ``stride < clip_size`` -) and how many frames the loop may process (``budget_frames``).
    Windows start every ``stride`` frames (0: half a clip); more than ``budget // clip_size`` of them are thinned with ``linspace``.
    ``total_frames == 0`` (a container without a frame count): every frame is kept, ``window_id`` is -1 for all of them, so no clip
    is ever enqueued and the video scores 0.0 - as written."""

    def __init__(self, total_frames: int, clip_size: int, stride: int, max_frame: int, fps: float):
        default_budget = max_frame if max_frame > 0 else int(fps * 20)
        self.total_frames, self.ranges, self.starts = int(total_frames), None, None
        if self.total_frames > 0:
            stride = stride if stride > 0 else max(1, clip_size // 2)
            starts = list(range(0, max(0, self.total_frames - clip_size) + 1, stride))
            max_windows = max(1, default_budget // max(1, clip_size))
            if len(starts) > max_windows:
                starts = [starts[i] for i in np.linspace(0, len(starts) - 1, max_windows, dtype=int)]
            self.starts = starts
            self.ranges = [(s, min(s + clip_size - 1, self.total_frames - 1)) for s in starts]
            self.budget_frames = sum(hi - lo + 1 for lo, hi in self.ranges)
        else:
            self.budget_frames = default_budget

    def keep(self, i: int) -> bool:
        return True if self.ranges is None else any(lo <= i <= hi for lo, hi in self.ranges)

    def window_id(self, i: int) -> int:
        if self.ranges is not None:
            for k, (lo, hi) in enumerate(self.ranges):
                if lo <= i <= hi:
                    return k
        return -1


def faces_valid(dets, start_conf: float, start_min_size: float) -> bool:
    """:279-285: one detection at least as confident and as large as a start asks for"""
    if dets is None or len(dets) == 0:
        return False
    return any(d[4] >= start_conf and max(d[2], d[3]) >= start_min_size for d in dets)


def filter_detections(dets, frame_h: int, min_det_side, min_det_area, exclude_bottom_frac) -> np.ndarray:
    """:517-531: the rows (float32) that are no micro-face - longer side, area - and whose centre is not in the bottom band"""
    dets_np = np.asarray(dets, dtype=np.float32)
    w, h, y = dets_np[:, 2], dets_np[:, 3], dets_np[:, 1]
    mask = np.ones(len(dets_np), dtype=bool)
    if min_det_side > 0:
        mask &= (np.maximum(w, h) >= min_det_side)
    if min_det_area and min_det_area > 0:
        mask &= ((w * h) >= min_det_area)
    if exclude_bottom_frac and exclude_bottom_frac > 0:
        mask &= ((y + 0.5 * h) < frame_h * (1.0 - float(exclude_bottom_frac)))
    return dets_np[mask]


class _Candidate:
    """a tracked face of one processed frame that reached the quality gate (:597)"""
    __slots__ = ("frame_idx", "slot", "tid", "record", "rect", "min_side", "lap", "full")

    def __init__(self, frame_idx, slot, tid, record, rect):
        self.frame_idx, self.slot, self.tid, self.record, self.rect = frame_idx, slot, tid, record, rect
        self.min_side = self.lap = self.full = None


def track_stage(st, frame_idx: int, slot: int, shape, dets, args, landmarks=None, frame_view=None) -> List[_Candidate]:
    """:515-597 for one processed frame - ``live.track_candidates``' sibling: this loop has the three detection filters,
    ``min_track_side`` and the id-switch count, and neither the self-view exclusion nor the ``drop_after`` purge.  ``st``: the run's
    state (``tracker``, ``last_lm``, ``prev_boxes`` / ``prev_ids`` / ``id_switches`` / ``frames_seen``); ``dets``: the frame's YuNet
    rows, or None when the loop did not ask for a detection.  Returns the faces whose crop is to be measured, in track order."""
    H, W = int(shape[0]), int(shape[1])
    det_tlbr, dets_np, tracks_in = [], None, []
    if dets is not None and len(dets) > 0:
        dets_np = filter_detections(dets, H, args.min_det_side, args.min_det_area, args.exclude_bottom_frac)
        for d in dets_np:
            x, y, w, h, score = d[:5]
            tlbr = np.array([x, y, x + w, y + h], dtype=np.float32)
            tracks_in.append(STrack(tlbr, score=float(score)))     # as written (:535): STrack takes tlwh and is handed tlbr, so a
            det_tlbr.append(tlbr)                                  # track's box is (x, y, x + w, y + h) read as (x, y, w, h)
    det_tlbr = np.asarray(det_tlbr, dtype=np.float32) if det_tlbr else None
    online = st.tracker.update(tracks_in, (H, W), (H, W))                                  # :538

    cur_boxes, cur_ids = [], []                                                            # :543-559, the id coherence
    for tr in online or []:
        if max(tr.tlbr[2] - tr.tlbr[0], tr.tlbr[3] - tr.tlbr[1]) < args.min_track_side:
            continue
        cur_boxes.append(tr.tlbr.astype(np.float32))
        cur_ids.append(tr.track_id)
    if len(cur_boxes) > 0:
        cur_boxes = np.stack(cur_boxes, 0)
        if st.prev_boxes is not None and st.prev_ids is not None:
            dist = iou_distance(st.prev_boxes, cur_boxes)
            for i_prev in range(st.prev_boxes.shape[0]):
                j = int(np.argmin(dist[i_prev]))
                if 1.0 - float(dist[i_prev, j]) >= 0.5 and st.prev_ids[i_prev] != cur_ids[j]:
                    st.id_switches += 1
        st.prev_boxes, st.prev_ids = cur_boxes, cur_ids            # as written: a frame without a box keeps the older ones
    st.frames_seen += 1

    out = []
    for tr in online or []:                                                                # :561-597
        if max(tr.tlbr[2] - tr.tlbr[0], tr.tlbr[3] - tr.tlbr[1]) < args.min_track_side:
            continue
        tid = tr.track_id
        st.buffers.setdefault(tid, [])                                                     # :567
        yunet_lm5 = None
        if det_tlbr is not None and len(det_tlbr) > 0:                                     # :569-574
            ious = 1.0 - iou_distance(np.array([tr.tlbr], dtype=np.float32), det_tlbr)[0]
            k = int(np.argmax(ious))
            if ious[k] >= 0.4:
                yunet_lm5 = dets_np[k][5:15].reshape(5, 2)
        fm = None
        if (frame_idx % args.mesh_every) == 0 or (tid not in st.last_lm):                  # :577-586
            fm = landmarks(frame_view(slot), tr.tlbr) if landmarks is not None else None
            if fm is None and yunet_lm5 is not None:
                fm = {"lm5": yunet_lm5, "lm68": None}
            if fm is not None:
                st.last_lm[tid] = {**fm, "frame_idx": frame_idx}
        else:
            cached = st.last_lm.get(tid)
            if cached is not None:
                fm = {"lm5": cached["lm5"], "lm68": cached["lm68"]}
            elif yunet_lm5 is not None:
                fm = {"lm5": yunet_lm5, "lm68": None}
        if fm is None:
            continue
        x1, y1, x2, y2 = map(int, get_crop_box((H, W), tr.tlbr, scale=args.crop_scale))    # :593-595
        if x2 <= x1 or y2 <= y1:
            continue
        top_left = np.array([[x1, y1]], dtype=np.float32)                                  # :600-606
        lm68 = fm["lm68"]
        record = ((tr.tlbr.reshape(2, 2).astype(np.float32) - top_left).reshape(-1), np.asarray(fm["lm5"]).astype(np.float32) - top_left,
                  np.zeros((68, 2), np.float32) if lm68 is None else np.asarray(lm68).astype(np.float32) - top_left,      # :368-371
                  np.array([x1, y1, x2, y2], dtype=np.int32))
        out.append(_Candidate(frame_idx, slot, tid, record, (x1, y1, x2, y2)))
    return out


def record_candidates(st, rec, quality, frame_ids) -> List[_Candidate]:
    """the chunk stage's record (``runner_device.parse_record``) and the figures ``[(min side, half-size lap, full-size lap or
    None)]`` of its candidates as ``track_stage``'s candidates of the chunk's frames, measured; the records are formed with
    ``track_stage``'s expressions"""
    for fr in rec["frames"][:len(frame_ids)]:
        for tid in fr["ids"][:int(fr["n_ids"])].tolist():
            st.buffers.setdefault(tid, [])                                                     # :567
    out = []
    for i, cd in enumerate(rec["cands"][:int(rec["head"]["n_cands"])]):
        if int(cd["flags"]):
            raise RuntimeError("runner: the quality launch refused candidate %d of the chunk (slot %d, box %s)" % (i, int(cd["slot"]), cd["box"].tolist()))
        x1, y1, x2, y2 = (int(v) for v in cd["box"])
        top_left = np.array([[x1, y1]], dtype=np.float32)                                  # :600-606
        record = ((cd["tlbr"].reshape(2, 2).astype(np.float32) - top_left).reshape(-1), cd["lm5"].astype(np.float32) - top_left,
                  np.zeros((68, 2), np.float32), np.array([x1, y1, x2, y2], dtype=np.int32))
        c = _Candidate(frame_ids[int(cd["frame_pos"])], int(cd["slot"]), int(cd["tid"]), record, (x1, y1, x2, y2))
        c.min_side, c.lap, c.full = quality[i]
        out.append(c)
    return out


def hard_limits_pass(min_side: float, lap: float, args) -> bool:
    """:292: the crop is neither too small nor too blurry to be used at all"""
    return not (min_side < args.q_min_size_hard or lap < args.q_lap_hard)


def quality_weight(min_side: float, lap: float, args) -> float:
    """:292-301 without its ``_qstat`` lines - the live step's gate (af_realtime.py:268-276) line for line - at this loop's limits"""
    return live.quality_weight(min_side, lap, q_weighting=args.q_weighting, q_min_size_soft=args.q_min_size_soft,
                               q_min_size_hard=args.q_min_size_hard, q_lap_soft=args.q_lap_soft, q_lap_hard=args.q_lap_hard)


class _RunState:
    """what one ``run`` keeps: :313-352"""

    def __init__(self, tracker):
        self.tracker = tracker
        self.buffers = {}                      # tid -> [(slot, record, weight)]: cur_imgs / cur_infos / cur_w as one list
        self.last_lm, self.last_win = {}, {}
        self.track_clip_scores = {}
        self.batch = []                        # batch_imgs / batch_infos / batch_tid: [(tid, [(slot, record)], enqueue time)]
        self.clip_latency_ms = []
        self.prev_boxes = self.prev_ids = None
        self.id_switches = self.frames_seen = 0
        self.qstat = []
        self.processed_ids, self.clips, self.flush_groups = [], [], []     # the record a test compares: see ``VideoRunner.trace``


class _DeviceSide:
    """everything of a run that touches the device: the frame store, the detector, both modes of the quality kernel, the warp and
    the replays.  ``VideoRunner.side_type`` names the class, so a host test scripts these five calls (``put``, ``view``, ``detect``,
    ``quality``, ``score``)."""

    def __init__(self, runner, shape, capacity: int):
        from .evaluator import FrameStore, StoresWarp, _network_device
        self.runner, self.shape = runner, tuple(shape)
        self.device = _network_device(runner.network)
        self.count = runner.stats.count
        with torch.cuda.device(self.device):
            self.store = FrameStore(self.device, runner.channel_order)
            self.store.open(shape, capacity)
        self.quality_launch = live.StoresQuality(self.device)
        if runner._scoring is None:                                   # the clip buffer, the graphs and the table ring outlive a run
            runner._scoring = (live._ClosedWindows(runner.network, runner.clip_size, runner.size, runner.max_batch, self.device),
                               StoresWarp(self.device, runner.clip_size, runner.size, runner.max_batch))
        self.scoring, self.warp = runner._scoring
        self.detections = live._Detections()
        self.std_points = STD_POINTS_256 * runner.size / 256.0

    def put(self, frames, first_slot: int):
        with torch.cuda.device(self.device):
            self.store.put(frames, first_slot)

    def view(self, slot: int):
        return self.store.view(slot)

    def detect(self, first_slot: int, n: int) -> List[np.ndarray]:
        """the YuNet rows of the `n` frames from `first_slot` on: one ``detect`` on their contiguous slots, one read-back"""
        with torch.cuda.device(self.device):
            rows, counts = self.runner.detector.detect(self.store.view(first_slot, n))
            self.count("detect")
            return self.detections.read([(rows, counts)], self.device, self.count)

    def quality(self, cands, full: bool):
        """``[(min side, half-size lap, full-size lap or None)]`` of the candidates' crop rectangles: one half-size launch per 64
        of them, with ``full`` one launch of the kernel's full-size mode per 64 as well, and ONE read-back"""
        q, order = self.quality_launch, self.runner.channel_order
        rects = [(self.store, order, c.slot) + tuple(c.rect) for c in cands]
        launched = q.launches
        out = q.half_and_full(rects) if full else [m + (None,) for m in q(rects)]
        self.count("quality", q.launches - launched)
        self.count("wait")
        return out

    # -- tracker="device" ---------------------------------------------------------------------------------------------------------
    def open_tracker(self, plan):
        """a fresh run on the device: the state block, and ONE buffer (with its pinned twin) for a chunk's record and the two
        arrays of quality sums, so that all three come back in one copy"""
        from . import _lib, runner_device as RD
        from .frames import store_ref
        self.plan, self._rd = plan, RD
        frames = self.runner.detect_batch
        self._cap, self._rec_bytes, rec = frames * RD.MAX_TRACKS, RD.record_bytes(frames), C.sizeof(_lib.QualitySums)
        self._sums_bytes = self._cap * rec
        with torch.cuda.device(self.device), torch.inference_mode(False):
            self._run_state = torch.from_numpy(plan.reset()).to(self.device)
            self._chunk_dev = torch.zeros(self._rec_bytes + 2 * self._sums_bytes, dtype=torch.uint8, device=self.device)
            self._chunk_host = torch.zeros(self._chunk_dev.numel(), dtype=torch.uint8, pin_memory=True)
        self._store_ref = store_ref(self.store, self.runner.channel_order)
        self._rows = None                                             # the detector's tensors, alive until the next chunk

    def track_chunk(self, frames, first_slot: int, frame_ids, full: bool):
        """a chunk's upload, detection, host stage and quality measurement without a read-back in between: ``put``, ``detect``,
        one ``af_runner_track_chunk`` on the rows where the detector left them, the half-size ``af_face_quality_table_u8`` on the
        record where that launch left it - with ``full`` the full-size one as well -, one pinned copy of the record and both arrays
        of sums, one wait.  Returns ``(record, [(min side, half-size lap, full-size lap or None)])``, a figure per candidate."""
        from . import _lib
        RD, n, lib = self._rd, len(frames), _lib.lib
        with torch.cuda.device(self.device):
            self.store.put(frames, first_slot)
            rows, counts = self.runner.detector.detect(self.store.view(first_slot, n))
            self.count("detect")
            if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] < 15 or rows.dtype != torch.float32 or counts.dtype != torch.int32 or counts.numel() != n:
                raise ValueError("runner: a detector's rows are (%d, N, >= 15) float32 with (%d,) int32 counts, got %s %s and %s %s"
                                 % (n, n, tuple(rows.shape), rows.dtype, tuple(counts.shape), counts.dtype))
            rows, counts = rows.contiguous(), counts.contiguous()
            self._rows = (rows, counts)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            base = self._chunk_dev.data_ptr()
            chunk = self.plan.chunk(self._run_state.data_ptr(), rows.data_ptr(), counts.data_ptr(), base, rows.numel(), rows.shape[1], rows.shape[2],
                                    first_slot, frame_ids)
            _lib.check(lib.af_runner_track_chunk(C.byref(chunk), stream), "af_runner_track_chunk")
            self.count("track")
            for mode in ((0, 1) if full else (0,)):
                sums = C.c_void_p(base + self._rec_bytes + mode * self._sums_bytes)
                _lib.check(lib.af_face_quality_table_u8(C.byref(self._store_ref), C.c_void_p(base), n * RD.MAX_TRACKS, mode, sums, None, 0, stream),
                           "af_face_quality_table_u8")
                self.count("quality")
            self._chunk_host.copy_(self._chunk_dev, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            self.count("wait")
        host = self._chunk_host.numpy()
        rec = RD.parse_record(host[:self._rec_bytes], n)
        count = int(rec["head"]["n_cands"])
        sums = np.frombuffer(host[self._rec_bytes:].tobytes(), dtype=live._SUMS_DTYPE).reshape(2, self._cap)
        lap = lambda r: (int(r["n_px"]) * int(r["s2"]) - int(r["s1"]) * int(r["s1"])) / (int(r["n_px"]) * int(r["n_px"]))
        quality = []
        for i, cd in enumerate(rec["cands"][:count]):
            x1, y1, x2, y2 = (int(v) for v in cd["box"])
            bad = int(cd["flags"]) or int(sums[0, i]["n_px"]) == 0
            quality.append((float(min(y2 - y1, x2 - x1)), None if bad else lap(sums[0, i]), lap(sums[1, i]) if full and not bad else None))
        return rec, quality

    def score(self, group) -> np.ndarray:
        """the scores of one flush group ``[(tid, [(slot, record)])]``: per clip ONE fit over all of its buffered entries and the
        warp of its first ``clip_size`` frames (:401, :408-413), ``max_batch`` clips per warp launch and replay, one read-back"""
        T, windows = self.runner.clip_size, []
        for _, entries in group:
            whole = _FrameTrack([rec for _, rec in entries], [slot for slot, _ in entries], self.shape)
            tfm, _, h, w, diff = fit_window(whole.boxes, whole.five, self.std_points)
            head = entries[:T] + [entries[-1]] * max(0, T - len(entries))                  # :409-411: a short clip repeats its last frame
            track = _FrameTrack([rec for _, rec in head], [slot for slot, _ in head], self.shape)
            fit = (tfm, int(h), int(w), np.concatenate([diff[:T], np.repeat(diff[-1:], max(0, T - len(entries)), axis=0)]).astype(np.int64))
            windows.append((self.store, self.runner.channel_order, track.frame, track, fit))
        with torch.cuda.device(self.device):
            return self.scoring(len(windows), lambda first, n, run, clip: self.warp(windows[first:first + n] + [windows[first + n - 1]] * (run - n), clip),
                                count=self.count)


class VideoRunner:
    """``VideoRunner(network, detector=None, modelPath=None, **args).run(frames, fps=30.0, total_frames=None)`` -> the dict
    ``VideoRunner.run(video_path)`` of altfreezing/TEST2.py returns (None for no frames, as there).

    ``network``: as for ``LiveCall``.  ``detector``: a ``YuNet`` (``None`` with ``modelPath`` builds one with ``conf``, 0.3, 5000 as
    :266) or any object with ``detect(frames_u8 (B, H, W, 3)) -> (rows, counts)`` device tensors.  ``**args``: TEST2.py's argparse
    names with its defaults (``DEFAULTS``; those of ``UNUSED`` are accepted and not read), plus ``size`` (the network's input side),
    ``max_batch`` (clips per forward), ``frame_bytes`` (the bound of the frame store), ``channel_order`` ("bgr", what ``cap.read()``
    gives, or "rgb"), ``detect_batch`` (frames per chunk) and ``landmarks`` (``RealtimeCall``'s hook where the reference has
    FaceMesh).

    ``frames``: an iterable of H x W x 3 uint8 arrays, or of ``YuvFrame``s; ``fps``: the container's rate; ``total_frames``: its
    frame count (default ``len(frames)`` when that exists, else 0 - see ``WindowPlan`` for what 0 means).

    The loop is :303-621 as written: the fps sanity check, the adaptive ``detect_every``, a fresh ``ByteTracker(frame_rate=fps)``
    per run (track ids restart at 1), the window plan, ``smart_start`` (detection is forced until ``start_after_n`` consecutive
    frames had a valid face, and those frames are dropped), ``need_detect``'s third clause (no tracked face: a frame without
    detections marks every track lost, so the frame after a skipped one detects again, whatever ``detect_every`` says), the budget
    break, ``track_stage``, the gate with ``_qstat`` (the full-size measurement: only of crops that pass the hard limits, only
    with ``q_weighting``, only the first 50), the buffers, the enqueue rule (``clip_size`` buffered entries, a window other than -1
    that this track has not used; then the buffer is cleared), the ``batch_clips`` flush and the final flush.

    The device side.  Every kept frame is uploaded once into a frame store of ``budget_frames + 2 * detect_batch`` slots (fewer
    for a shorter list); frames processed after the start keep their slots for the whole run, because a track's buffer may name
    old frames, and a chunk that lies wholly before the start gives its slots to the next.  ``ValueError`` names the bytes needed
    when that does not fit ``frame_bytes``.  Per chunk of ``detect_batch`` kept frames: one ``detect`` on the contiguous slots
    (every frame of the chunk is detected; the rows of a frame whose ``need_detect`` turns out false are dropped, which changes
    nothing the reference computes), one read-back, the host stage frame by frame, one half-size quality launch per 64 crop
    rectangles of the chunk, - while ``_qstat`` holds fewer than 50 records at the chunk's start - one full-size launch per 64 of
    them as well, one read-back of both, then the gate and the bookkeeping in frame order.  A flush group is warped out of the store
    and replayed exactly as the reference forms it, so the padded batch sizes - and with them the score bits - do not depend on
    ``detect_batch``.  ``stats``: ``live.ServerStats`` (``last``: the last chunk or flush; ``chunks``: per chunk its counts and
    ``closes``).

    ``tracker="device"`` (``"host"`` by default; no ``landmarks`` hook, ``detect_batch`` at most 64): the host stage of a chunk is
    one launch of one wave (csrc/af_runner_core.h) that walks the chunk's frames on the detector's rows in device memory - the
    rhythm, the start, the budget, the filters, the tracker in ``device_tracker``'s fixed-order fp64 (tests/bytetrack_ref.py), the
    id-switch count, the five points and the crop boxes - and writes a chunk record; the quality launches take rectangles, slots
    and tile prefixes from that record (``af_face_quality_table_u8``); the record and both arrays of sums come back in one pinned
    copy behind ONE wait; the rows are not read back.  The gate and the books run on the host as before.  More than 32 rows past
    the detection filters in a frame, or more than 32 tracked and lost faces, raise ``RuntimeError`` naming the frame.  ``stats``
    counts ``track``, the chunk launches."""

    side_type = _DeviceSide
    DEFAULTS, UNUSED = DEFAULTS, UNUSED

    def __init__(self, network, detector=None, modelPath=None, **args):
        unknown = sorted(set(args) - set(DEFAULTS) - set(UNUSED) - set(OWN))
        if unknown:
            raise TypeError("runner: unknown argument(s) %s" % ", ".join(unknown))
        merged = dict(DEFAULTS, **{k: v for k, v in args.items() if k in DEFAULTS})
        if merged["pool_method"] not in POOL_METHODS:
            raise ValueError("runner: pool_method one of %s, not %r" % (", ".join(POOL_METHODS), merged["pool_method"]))
        self.args = SimpleNamespace(**merged)
        own = dict(OWN, **{k: v for k, v in args.items() if k in OWN})
        self.size, self.max_batch, self.frame_bytes = int(own["size"]), int(own["max_batch"]), int(own["frame_bytes"])
        self.channel_order, self.detect_batch, self.landmarks = live._known_order(own["channel_order"]), int(own["detect_batch"]), own["landmarks"]
        self.clip_size = int(self.args.clip_size)
        if self.clip_size < 1 or self.detect_batch < 1 or self.args.batch_clips < 1 or self.args.mesh_every < 1:
            raise ValueError("runner: clip_size, detect_batch, batch_clips and mesh_every are at least 1")
        self.tracker = own["tracker"]
        if self.tracker not in TRACKERS:
            raise ValueError("runner: tracker one of %s, not %r" % (", ".join(TRACKERS), self.tracker))
        if self.tracker == "device" and self.landmarks is not None:
            raise ValueError("runner: tracker=\"device\" has no landmarks hook (the hook reads a frame on the host between two tracker updates)")
        if self.tracker == "device" and self.detect_batch > 64:
            raise ValueError("runner: tracker=\"device\" takes at most 64 frames per chunk, detect_batch is %d" % self.detect_batch)
        if detector is None:
            if modelPath is None:
                raise ValueError("runner: a detector, or the modelPath of the YuNet file to build one from")
            from .detector import YuNet
            detector = YuNet(modelPath, confThreshold=self.args.conf, nmsThreshold=0.3, topK=5000)
        self.network, self.detector = getattr(network, "network", network), detector
        self.stats = live.ServerStats()
        self.chunks: List[dict] = []
        self.trace: Optional[dict] = None      # of the last run: processed frame ids, enqueued clips, flush groups, ``_qstat``
        self._scoring = None

    def frame_store_bytes(self, shape, budget_frames: int, n_frames: Optional[int] = None) -> int:
        """the bytes of the frame store a run over frames of `shape` needs"""
        slots = (budget_frames if n_frames is None else min(budget_frames, n_frames)) + 2 * self.detect_batch
        return slots * int(shape[0]) * int(shape[1]) * 3 + _POOL_SLACK

    # -- the loop: TEST2.py:303-621 ------------------------------------------------------------------------------------------------
    def run(self, frames, fps: float = 30.0, total_frames: Optional[int] = None, video_path=None):
        a, T = self.args, self.clip_size
        n_frames = len(frames) if hasattr(frames, "__len__") else None
        if total_frames is None:
            total_frames = n_frames or 0
        if torch.cuda.is_available():
            torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        real_fps = sane_fps(fps)                                                           # :329-331
        st = _RunState(ByteTracker(SimpleNamespace(track_thresh=a.track_thresh, track_buffer=a.track_buffer, match_thresh=a.match_thresh,
                                                   mot20=False), frame_rate=real_fps))      # :334, :305-311
        detect_every = detect_rhythm(a.detect_every, real_fps)                             # :337-340
        source = iter(frames)
        first = next(source, None)                                                         # :342-343
        if first is None:
            return None
        shape = tuple(first.shape)
        H, W = shape[:2]
        plan = WindowPlan(int(total_frames), T, a.stride, a.max_frame, real_fps)           # :442-480
        need = self.frame_store_bytes(shape, plan.budget_frames, n_frames)
        if need > self.frame_bytes:
            raise ValueError("runner: the frame store of this run needs %d bytes (%d frames of %d x %d), frame_bytes is %d"
                             % (need, (need - _POOL_SLACK) // (H * W * 3), W, H, self.frame_bytes))
        self.stats, self.chunks, self.trace = live.ServerStats(), [], None                      # of this run
        side = self.side_type(self, shape, (need - _POOL_SLACK) // (H * W * 3))
        on_device = self.tracker == "device"
        if on_device:
            from . import runner_device
            side.open_tracker(runner_device.ChunkPlan(a, shape, detect_every, plan.budget_frames, real_fps))

        started, consec = (not a.smart_start), 0                                           # :349-352
        processed_after_start = frames_processed = 0
        frame_idx, base, stop, exhausted = -1, 0, False, False
        pending = first

        def flush():                                                                       # :393-439
            if not st.batch:
                return
            group, st.batch = st.batch, []
            scores = side.score([(tid, entries) for tid, entries, _ in group])
            now = time.perf_counter()
            for s, (tid, _, t_enq) in zip(scores, group):
                st.track_clip_scores.setdefault(tid, []).append(float(s))
                st.clip_latency_ms.append((now - t_enq) * 1000.0)
            st.flush_groups.append([tid for tid, _, _ in group])

        while not stop and not exhausted:
            chunk = []                                                                     # the next ``detect_batch`` kept frames
            while len(chunk) < self.detect_batch:
                frame = pending if pending is not None else next(source, None)
                pending = None
                if frame is None:
                    exhausted = True
                    break
                frame_idx += 1                                                             # :489
                if not plan.keep(frame_idx):                                               # :492-493
                    continue
                if not isinstance(frame, YuvFrame) and not is_crop(frame):
                    raise AssertionError("runner: a frame must be an HxWx3 uint8 numpy array or a YuvFrame")
                if tuple(frame.shape) != shape:
                    raise ValueError("runner: frame %d is %r, the video's frames are %r" % (frame_idx, tuple(frame.shape), shape))
                chunk.append((frame_idx, frame))
            if not chunk:
                break
            self.stats.begin()
            cands, kept_slots = [], False
            if on_device:                                                                  # the host stage as one launch: DESIGN 28
                short = bool(a.q_weighting) and len(st.qstat) < QSTAT_MAX
                ids = [k for k, _ in chunk]
                rec, quality = side.track_chunk([f for _, f in chunk], base, ids, short)
                refused = runner_device.refusal(rec, ids)
                if refused is not None:
                    raise refused
                head = rec["head"]
                done = [k for k, fr in zip(ids, rec["frames"]) if int(fr["flags"]) & runner_device.PROCESSED]
                started, consec, stop = bool(head["started"]), int(head["consec"]), bool(head["stop"])
                processed_after_start = int(head["processed_after_start"])
                frames_processed += len(done)
                kept_slots = bool(done)
                st.processed_ids += done
                st.id_switches, st.frames_seen = int(head["id_switches"]), int(head["frames_seen"])
                cands = record_candidates(st, rec, quality, ids)
            else:
                side.put([f for _, f in chunk], base)
                rows = side.detect(base, len(chunk))
            for j, (k, _) in enumerate(() if on_device else chunk):                        # the host stage, in frame order
                need_detect = (not started) or (k % detect_every == 0) or (st.tracker.tracked_stracks == [])      # :496-500
                dets = rows[j] if need_detect else None                                    # :503
                if not started:                                                            # :505-508, as written: these frames are dropped
                    consec = consec + 1 if (dets is not None and faces_valid(dets, a.start_conf, a.start_min_size)) else 0
                    if consec >= a.start_after_n:
                        started = True
                    continue
                if processed_after_start >= plan.budget_frames:                            # :510
                    stop = True
                    break
                processed_after_start += 1
                frames_processed += 1
                kept_slots = True
                st.processed_ids.append(k)
                cands += track_stage(st, k, base + j, shape, dets, a, self.landmarks, side.view)

            if cands and not on_device:                                                    # :598, for the whole chunk
                short = bool(a.q_weighting) and len(st.qstat) < QSTAT_MAX                  # :293, :297: is the second figure still wanted
                for c, (min_side, lap, full) in zip(cands, side.quality(cands, short)):
                    c.min_side, c.lap, c.full = min_side, lap, full
            closes = len(st.flush_groups)
            for c in cands:                                                                # :598-618, in frame order
                wq = quality_weight(c.min_side, c.lap, a)
                if a.q_weighting and hard_limits_pass(c.min_side, c.lap, a) and len(st.qstat) < QSTAT_MAX:       # :292-299
                    st.qstat.append((int(c.min_side), c.full))
                buf = st.buffers[c.tid]
                if wq > 0.0:
                    buf.append((c.slot, c.record, wq))
                wid = plan.window_id(c.frame_idx)
                if len(buf) >= T:                                                          # :611, as written: >=, and a buffer that
                    if wid != -1 and st.last_win.get(c.tid) != wid:                        # waits for a new window grows past clip_size
                        entries = [(slot, rec) for slot, rec, _ in buf]
                        # enqueue_clip (:354-391) pads a buffer shorter than clip_size with its last entry - none is, behind the
                        # test above - and keeps the buffer's tail for the next window (:378-388); the clear() below erases that
                        st.batch.append((c.tid, entries, time.perf_counter()))
                        st.clips.append({"tid": c.tid, "frame_idx": c.frame_idx, "slots": [slot for slot, _ in entries],
                                         "records": [rec for _, rec in entries]})
                        st.last_win[c.tid] = wid
                        buf.clear()                                                        # :616: no second clip in the same window
                        if len(st.batch) >= a.batch_clips:                                 # :617-618
                            flush()
            if kept_slots:                                                                 # a chunk wholly before the start is overwritten
                base += len(chunk)
            self.chunks.append(dict(self.stats.last, closes=len(st.flush_groups) - closes, frames=len(chunk)))

        if st.batch:                                                                       # :621
            self.stats.begin()
            closes = len(st.flush_groups)
            flush()
            self.chunks.append(dict(self.stats.last, closes=len(st.flush_groups) - closes, frames=0))

        out = video_verdict(st.track_clip_scores, st.qstat, a)                             # :627-749
        elapsed = time.perf_counter() - t0
        cpu_peak_mb = float("nan")                                                         # :756-771
        if resource is not None and platform.system() != "Windows":
            peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
            cpu_peak_mb = peak / (1024 * 1024) if platform.system() == "Darwin" else peak / 1024.0
        gpu = torch.cuda.is_available()
        self.trace = {"processed": st.processed_ids, "clips": st.clips, "flush_groups": st.flush_groups, "qstat": list(st.qstat),
                      "slots_used": base}
        return {
            "video_path": video_path,
            "frames_processed": frames_processed,
            "elapsed_s": elapsed,
            "fps": frames_processed / max(1e-6, elapsed),
            "latency_ms_clip_mean": (sum(st.clip_latency_ms) / len(st.clip_latency_ms)) if st.clip_latency_ms else float("nan"),
            "video_score": out["video_score"],
            "pred_label": out["pred_label"],
            "num_tracks": out["num_tracks"],
            "id_switch_rate_per_1k_frames": (st.id_switches / max(1, st.frames_seen)) * 1000.0,                          # :777
            "gpu_mem_alloc_peak_mb": torch.cuda.max_memory_allocated() / 1024 / 1024 if gpu else float("nan"),
            "gpu_mem_reserved_peak_mb": torch.cuda.max_memory_reserved() / 1024 / 1024 if gpu else float("nan"),
            "cpu_mem_peak_mb": cpu_peak_mb,
            "per_person_scores": out["per_person_scores"],
            "per_person_labels": out["per_person_labels"],
            "track_clip_scores": {tid: list(v) for tid, v in st.track_clip_scores.items()},
            "stats": dict(self.stats.total, chunks=len(self.chunks)),
        }
