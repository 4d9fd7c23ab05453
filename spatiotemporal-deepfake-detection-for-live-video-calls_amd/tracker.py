"""ByteTrack on the host, on numpy + scipy alone: the tracker behind ``RealtimeAF.step`` (test/af_realtime.py:388), restated from
preprocessing/ByteTrack/{basetrack,kalman_filter,byte_tracker}.py and the parts of matching.py that ``BYTETracker.update`` and
af_realtime.py:415 use (``iou_distance``, ``ious``, ``linear_assignment``, ``fuse_score``).  No ``lap``, ``cython_bbox``, ``cv2`` or
torch; the per-frame work is a handful of 8x8 matrices per face, which is host work.

What differs from the reference, on purpose:
  * track ids come from a counter of the ``ByteTracker`` instance (the reference's is one class attribute shared by every tracker
    of the process); the first id is 1, where a fresh reference process starts;
  * ``lap.lapjv`` is ``scipy.optimize.linear_sum_assignment`` on the same extended matrix (``linear_assignment`` below).
What does not differ, although it looks odd: an empty ``tracks_in`` (every non-detect frame with ``detect_every > 1``) predicts
nothing, marks every tracked face lost, returns no track and counts the frame twice (byte_tracker.py:195-217, :221); a list of ``STrack`` (what af_realtime.py
hands over) has no second association, because the split by ``track_thresh`` happens only for the array form (:232-261); the
tracks removed this frame are subtracted from the lost list one call late (:353-354).  tests/golden/bytetrack_tracks.json holds
tracks recorded from the reference's own ``BYTETracker`` (tools/gen_bytetrack_golden.py); tests/test_tracker_host.py replays them.
"""
import numpy as np
import scipy.linalg
from scipy.optimize import linear_sum_assignment

NEW, TRACKED, LOST, REMOVED = 0, 1, 2, 3           # basetrack.py TrackState


class KalmanFilter:
    """constant-velocity filter over (cx, cy, aspect, height) and their rates (kalman_filter.py); the noise scales with the height"""

    def __init__(self):
        self._motion = np.eye(8)
        self._motion[:4, 4:] = np.eye(4)           # dt = 1
        self._observe = np.eye(4, 8)
        self._w_pos, self._w_vel = 1.0 / 20, 1.0 / 160

    def initiate(self, xyah):
        mean = np.r_[xyah, np.zeros_like(xyah)]
        h = xyah[3]
        std = [2 * self._w_pos * h, 2 * self._w_pos * h, 1e-2, 2 * self._w_pos * h,
               10 * self._w_vel * h, 10 * self._w_vel * h, 1e-5, 10 * self._w_vel * h]
        return mean, np.diag(np.square(std))

    def multi_predict(self, mean, covariance):
        """(N, 8) means and (N, 8, 8) covariances one step on; the products in the reference's order, for the same round-off"""
        h = mean[:, 3]
        one = np.ones_like(h)
        std = [self._w_pos * h, self._w_pos * h, 1e-2 * one, self._w_pos * h, self._w_vel * h, self._w_vel * h, 1e-5 * one, self._w_vel * h]
        sqr = np.square(np.r_[std]).T
        noise = np.asarray([np.diag(sqr[i]) for i in range(len(mean))])
        mean = np.dot(mean, self._motion.T)
        left = np.dot(self._motion, covariance).transpose((1, 0, 2))
        return mean, np.dot(left, self._motion.T) + noise

    def project(self, mean, covariance):
        h = mean[3]
        std = [self._w_pos * h, self._w_pos * h, 1e-1, self._w_pos * h]
        return np.dot(self._observe, mean), np.linalg.multi_dot((self._observe, covariance, self._observe.T)) + np.diag(np.square(std))

    def update(self, mean, covariance, xyah):
        pm, pc = self.project(mean, covariance)
        chol, lower = scipy.linalg.cho_factor(pc, lower=True, check_finite=False)
        gain = scipy.linalg.cho_solve((chol, lower), np.dot(covariance, self._observe.T).T, check_finite=False).T
        return mean + np.dot(xyah - pm, gain.T), covariance - np.linalg.multi_dot((gain, pc, gain.T))


class STrack:
    """one face: a detection (``STrack(tlwh, score)``) until the tracker activates it, a filtered track after"""
    _kalman = KalmanFilter()

    def __init__(self, tlwh, score):
        self._tlwh = np.asarray(tlwh, dtype=float)
        self.kalman_filter = None
        self.mean = self.covariance = None
        self.is_activated = False
        self.score = score
        self.tracklet_len = 0
        self.track_id, self.state = 0, NEW
        self.frame_id = self.start_frame = 0

    @property
    def end_frame(self):
        return self.frame_id

    @staticmethod
    def multi_predict(tracks):
        if not tracks:
            return
        mean = np.asarray([t.mean.copy() for t in tracks])
        cov = np.asarray([t.covariance for t in tracks])
        for i, t in enumerate(tracks):
            if t.state != TRACKED:
                mean[i][7] = 0                       # a lost face keeps its position rate, not its growth
        mean, cov = STrack._kalman.multi_predict(mean, cov)
        for t, m, c in zip(tracks, mean, cov):
            t.mean, t.covariance = m, c

    def activate(self, kalman_filter, frame_id, track_id):
        self.kalman_filter, self.track_id = kalman_filter, track_id
        self.mean, self.covariance = kalman_filter.initiate(self.tlwh_to_xyah(self._tlwh))
        self.tracklet_len, self.state = 0, TRACKED
        if frame_id == 1:                            # only the faces of a tracker's first frame are confirmed at once
            self.is_activated = True
        self.frame_id = self.start_frame = frame_id

    def re_activate(self, det, frame_id):
        self.mean, self.covariance = self.kalman_filter.update(self.mean, self.covariance, self.tlwh_to_xyah(det.tlwh))
        self.tracklet_len, self.state, self.is_activated = 0, TRACKED, True
        self.frame_id, self.score = frame_id, det.score

    def update(self, det, frame_id):
        self.frame_id = frame_id
        self.tracklet_len += 1
        self.mean, self.covariance = self.kalman_filter.update(self.mean, self.covariance, self.tlwh_to_xyah(det.tlwh))
        self.state, self.is_activated, self.score = TRACKED, True, det.score

    @property
    def tlwh(self):
        if self.mean is None:
            return self._tlwh.copy()
        r = self.mean[:4].copy()
        r[2] *= r[3]
        r[:2] -= r[2:] / 2
        return r

    @property
    def tlbr(self):
        r = self.tlwh.copy()
        r[2:] += r[:2]
        return r

    @staticmethod
    def tlwh_to_xyah(tlwh):
        r = np.asarray(tlwh).copy()
        r[:2] += r[2:] / 2
        r[2] /= r[3]
        return r

    @staticmethod
    def tlbr_to_tlwh(tlbr):
        r = np.asarray(tlbr).copy()
        r[2:] -= r[:2]
        return r

    def __repr__(self):
        return "STrack(%d, %d-%d)" % (self.track_id, self.start_frame, self.end_frame)


def ious(a, b) -> np.ndarray:
    """(len(a), len(b)) IoU of tlbr boxes in ``cython_bbox.bbox_overlaps``' convention: a box covers the pixels x0 .. x1 inclusive,
    so widths, heights and the intersection's sides all carry + 1 (two identical 10-wide boxes: 11 * 11 / (11 * 11))"""
    out = np.zeros((len(a), len(b)), dtype=float)
    if out.size == 0:
        return out
    a, b = np.ascontiguousarray(a, dtype=float), np.ascontiguousarray(b, dtype=float)
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]) + 1
    ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]) + 1
    hit = (iw > 0) & (ih > 0)
    inter = np.where(hit, iw * ih, 0.0)
    union = area_a[:, None] + area_b[None, :] - inter        # cython_bbox: float(area_a + area_b - iw * ih)
    out[hit] = inter[hit] / union[hit]
    return out


def iou_distance(a, b) -> np.ndarray:
    """1 - IoU between two lists of tracks, or of tlbr arrays when either list starts with one (matching.py:117-135)"""
    if (len(a) > 0 and isinstance(a[0], np.ndarray)) or (len(b) > 0 and isinstance(b[0], np.ndarray)):
        ta, tb = a, b
    else:
        ta, tb = [t.tlbr for t in a], [t.tlbr for t in b]
    return 1 - ious(ta, tb)


def fuse_score(cost: np.ndarray, detections) -> np.ndarray:
    """1 - IoU * detection score (matching.py:217-225)"""
    if cost.size == 0:
        return cost
    scores = np.array([d.score for d in detections])
    scores = np.expand_dims(scores, axis=0).repeat(cost.shape[0], axis=0)
    return 1 - (1 - cost) * scores


def linear_assignment(cost: np.ndarray, thresh: float):
    """``(matches (k, 2), unmatched rows, unmatched columns)`` as matching.py:83-94 gets them from
    ``lap.lapjv(cost, extend_cost=True, cost_limit=thresh)``.

    The equivalence.  With a finite ``cost_limit`` lapjv does not solve the n x m problem: it solves the square one of side n + m
    whose top-left block is ``cost``, whose bottom-right m x n block is 0 and whose other two blocks are ``thresh / 2``, and
    reports row i as unmatched when its column lies in the padding.  Leaving row i and column j both to the padding costs
    ``thresh / 2 + thresh / 2``, so an optimum pairs them only when ``cost[i, j] <= thresh`` (at equality either is optimal: a
    tie), and the freed padding rows and columns pair among themselves at 0.  Any exact solver of that square matrix returns the
    same pairs whenever the optimum is unique; ``linear_sum_assignment`` is one.  The ``<= thresh`` test below therefore never
    fires on an optimum - it is kept as the statement of what a match is."""
    n, m = cost.shape
    if cost.size == 0:
        return np.empty((0, 2), dtype=int), tuple(range(n)), tuple(range(m))
    ext = np.full((n + m, n + m), thresh / 2.0)
    ext[n:, m:] = 0
    ext[:n, :m] = cost
    rows, cols = linear_sum_assignment(ext)
    matches = [[r, c] for r, c in zip(rows, cols) if r < n and c < m and cost[r, c] <= thresh]
    hit_r, hit_c = {r for r, _ in matches}, {c for _, c in matches}
    return (np.asarray(matches, dtype=int).reshape(-1, 2), np.array([r for r in range(n) if r not in hit_r], dtype=int),
            np.array([c for c in range(m) if c not in hit_c], dtype=int))


def _joined(a, b):
    seen, out = set(), []
    for t in list(a) + list(b):
        if t.track_id not in seen:
            seen.add(t.track_id)
            out.append(t)
    return out


def _without(a, b):
    drop = {t.track_id for t in b}
    keep = {}
    for t in a:
        keep[t.track_id] = t
    return [t for tid, t in keep.items() if tid not in drop]


def _drop_duplicates(a, b):
    """of a tracked and a lost track that overlap with IoU > 0.85 the one with the shorter life goes (byte_tracker.py:387-400)"""
    dist = iou_distance(a, b)
    da, db = set(), set()
    for p, q in zip(*np.where(dist < 0.15)):
        if a[p].frame_id - a[p].start_frame > b[q].frame_id - b[q].start_frame:
            db.add(q)
        else:
            da.add(p)
    return [t for i, t in enumerate(a) if i not in da], [t for i, t in enumerate(b) if i not in db]


class ByteTracker:
    """``ByteTracker(args, frame_rate).update(tracks_in, img_info, img_size)`` -> the confirmed tracks of this frame.

    ``args``: ``track_thresh``, ``track_buffer``, ``match_thresh``, ``mot20`` (af_realtime.py / app_realtime.py: 0.8, 90, 0.8,
    False).  ``tracks_in``: a list of ``STrack(tlwh, score)`` as af_realtime.py:386 builds it, or an (N, 5) array of ``x0, y0, x1,
    y1, score`` rows, which is split at ``track_thresh`` into a first and a second association (the array is scaled in place by
    ``min(img_size[0] / img_info[1], img_size[1] / img_info[0])``, as the reference does)."""

    def __init__(self, args, frame_rate=30):
        self.tracked_stracks, self.lost_stracks, self.removed_stracks = [], [], []
        self.frame_id = 0
        self.args = args
        self.det_thresh = args.track_thresh + 0.1
        self.buffer_size = int(frame_rate / 30.0 * args.track_buffer)
        self.max_time_lost = self.buffer_size
        self.kalman_filter = KalmanFilter()
        self._count = 0

    def _next_id(self):
        self._count += 1
        return self._count

    def _nothing_detected(self):
        self.frame_id += 1                           # a second time: ``update`` has counted the frame already (:221, :197)
        removed = []
        for t in self.tracked_stracks:
            if t.state == TRACKED:
                t.state = LOST
                self.lost_stracks.append(t)
        for t in self.lost_stracks:
            if self.frame_id - t.end_frame > self.max_time_lost:
                t.state = REMOVED
                removed.append(t)
        self.tracked_stracks = [t for t in self.tracked_stracks if t.state == TRACKED]
        self.lost_stracks = _without(self.lost_stracks, removed)
        self.removed_stracks.extend(removed)
        self.tracked_stracks, self.lost_stracks = _drop_duplicates(self.tracked_stracks, self.lost_stracks)
        return []

    def update(self, tracks_in, img_info, img_size):
        if isinstance(tracks_in, np.ndarray) and tracks_in.size == 0:
            tracks_in = []
        self.frame_id += 1
        if isinstance(tracks_in, (list, tuple)) and len(tracks_in) == 0:
            return self._nothing_detected()
        activated, refound, lost, removed = [], [], [], []
        second = []
        if isinstance(tracks_in, list) and isinstance(tracks_in[0], STrack):
            detections = tracks_in
        else:
            scores, boxes = tracks_in[:, 4], tracks_in[:, :4]
            boxes /= min(img_size[0] / float(img_info[1]), img_size[1] / float(img_info[0]))
            high = scores > self.args.track_thresh
            low = np.logical_and(scores > 0.1, scores < self.args.track_thresh)
            detections = [STrack(STrack.tlbr_to_tlwh(b), s) for b, s in zip(boxes[high], scores[high])]
            second = [STrack(STrack.tlbr_to_tlwh(b), s) for b, s in zip(boxes[low], scores[low])]

        unconfirmed = [t for t in self.tracked_stracks if not t.is_activated]
        confirmed = [t for t in self.tracked_stracks if t.is_activated]

        # first association: confirmed and lost tracks, predicted, against the high-score detections
        pool = _joined(confirmed, self.lost_stracks)
        STrack.multi_predict(pool)
        dists = iou_distance(pool, detections)
        if not self.args.mot20:
            dists = fuse_score(dists, detections)
        matches, u_track, u_det = linear_assignment(dists, self.args.match_thresh)
        for it, idet in matches:
            t = pool[it]
            if t.state == TRACKED:
                t.update(detections[idet], self.frame_id)
                activated.append(t)
            else:
                t.re_activate(detections[idet], self.frame_id)
                refound.append(t)

        # second association: the tracked faces still unmatched against the low-score detections, by IoU alone
        rest = [pool[i] for i in u_track if pool[i].state == TRACKED]
        matches, u_rest, _ = linear_assignment(iou_distance(rest, second), 0.5)
        for it, idet in matches:
            t = rest[it]
            if t.state == TRACKED:
                t.update(second[idet], self.frame_id)
                activated.append(t)
            else:
                t.re_activate(second[idet], self.frame_id)
                refound.append(t)
        for it in u_rest:
            if rest[it].state != LOST:
                rest[it].state = LOST
                lost.append(rest[it])

        # unconfirmed tracks (one frame old) against what the first association left; an unmatched one dies
        detections = [detections[i] for i in u_det]
        dists = iou_distance(unconfirmed, detections)
        if not self.args.mot20:
            dists = fuse_score(dists, detections)
        matches, u_unconfirmed, u_det = linear_assignment(dists, 0.7)
        for it, idet in matches:
            unconfirmed[it].update(detections[idet], self.frame_id)
            activated.append(unconfirmed[it])
        for it in u_unconfirmed:
            unconfirmed[it].state = REMOVED
            removed.append(unconfirmed[it])

        # new tracks
        for i in u_det:
            if detections[i].score < self.det_thresh:
                continue
            detections[i].activate(self.kalman_filter, self.frame_id, self._next_id())
            activated.append(detections[i])

        for t in self.lost_stracks:
            if self.frame_id - t.end_frame > self.max_time_lost:
                t.state = REMOVED
                removed.append(t)

        self.tracked_stracks = [t for t in self.tracked_stracks if t.state == TRACKED]
        self.tracked_stracks = _joined(_joined(self.tracked_stracks, activated), refound)
        self.lost_stracks = _without(self.lost_stracks, self.tracked_stracks)
        self.lost_stracks.extend(lost)
        self.lost_stracks = _without(self.lost_stracks, self.removed_stracks)      # this frame's removals leave one call later
        self.removed_stracks.extend(removed)
        self.tracked_stracks, self.lost_stracks = _drop_duplicates(self.tracked_stracks, self.lost_stracks)
        return [t for t in self.tracked_stracks if t.is_activated]
