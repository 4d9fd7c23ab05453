"""The statement of the device tracker (csrc/af_track_core.h): ``tracker.ByteTracker`` once more, with every sum written out.

The list logic is tracker.py's, line for line.  What differs is that nothing here calls BLAS, LAPACK or scipy: a number is a Python
float (IEEE binary64, one rounding per ``*``, ``+``, ``-``, ``/`` and ``math.sqrt``) and every product of matrices is three loops
that sum over k ascending from 0.0, zeros of the motion and observation matrices included.  The core does the same operations in
the same order under ``fp contract(off)``, so the two can be equal bit for bit; tracker.py, whose sums BLAS orders, can not.

  predict   mean' = mean F^T;  cov' = (F cov) F^T + diag(std^2)                                      (all 8 x 8 x 8)
  project   pm = H mean;  pc = (H cov) H^T + diag(std^2)
  update    L = chol(pc), row by row, ``s = pc[i][j]; s -= L[i][k] * L[j][k]`` for k < j ascending;
            B = (cov H^T)^T;  forward ``y[i] = (B[i] - sum_{k<i} L[i][k] y[k]) / L[i][i]`` with the sum taken as repeated
            subtraction, k ascending;  backward ``x[i] = (y[i] - sum_{k>i} L[k][i] x[k]) / L[i][i]``, i descending, k ascending;
            gain = x^T;  mean' = mean + (z - pm) gain^T;  cov' = cov - (gain pc) gain^T
  assign    the rectangular form of ``tracker.linear_assignment``'s square matrix: n rows, the m columns of the cost and n more
            that cost ``thresh`` each (a row left alone); shortest augmenting paths with potentials; a pair counts when its cost
            is <= thresh.  Sum over matched (cost - thresh) is the square problem's objective less a constant.
"""
import math

import numpy as np

NEW, TRACKED, LOST, REMOVED = 0, 1, 2, 3
W_POS, W_VEL = 1.0 / 20, 1.0 / 160
F = [[1.0 if (i == j or j == i + 4) else 0.0 for j in range(8)] for i in range(8)]
H = [[1.0 if i == j else 0.0 for j in range(8)] for i in range(4)]


def _matmul(a, b_t):
    """a (n x k) times the transpose of b_t (m x k): out[i][j] = sum_k a[i][k] * b_t[j][k], k ascending from 0.0"""
    out = []
    for row in a:
        line = []
        for col in b_t:
            acc = 0.0
            for k in range(len(row)):
                acc = acc + row[k] * col[k]
            line.append(acc)
        out.append(line)
    return out


def _t(a):
    return [list(r) for r in zip(*a)]


def initiate(xyah):
    h = xyah[3]
    std = [2 * W_POS * h, 2 * W_POS * h, 1e-2, 2 * W_POS * h, 10 * W_VEL * h, 10 * W_VEL * h, 1e-5, 10 * W_VEL * h]
    return list(xyah) + [0.0] * 4, [[std[i] * std[i] if i == j else 0.0 for j in range(8)] for i in range(8)]


def predict(mean, cov):
    h = mean[3]
    std = [W_POS * h, W_POS * h, 1e-2, W_POS * h, W_VEL * h, W_VEL * h, 1e-5, W_VEL * h]
    new_mean = _matmul([mean], F)[0]
    left = _matmul(F, _t(cov))
    full = _matmul(left, F)
    return new_mean, [[full[i][j] + (std[i] * std[i] if i == j else 0.0) for j in range(8)] for i in range(8)]


def project(mean, cov):
    h = mean[3]
    std = [W_POS * h, W_POS * h, 1e-1, W_POS * h]
    pm = [r[0] for r in _matmul(H, [mean])]
    pc = _matmul(_matmul(H, _t(cov)), H)
    return pm, [[pc[i][j] + (std[i] * std[i] if i == j else 0.0) for j in range(4)] for i in range(4)]


def cholesky(a):
    low = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(i + 1):
            s = a[i][j]
            for k in range(j):
                s = s - low[i][k] * low[j][k]
            low[i][j] = math.sqrt(s) if i == j else s / low[j][j]
    return low


def solve(low, b):
    """x of (low low^T) x = b for the four entries of one column b"""
    y = [0.0] * 4
    for i in range(4):
        s = b[i]
        for k in range(i):
            s = s - low[i][k] * y[k]
        y[i] = s / low[i][i]
    x = [0.0] * 4
    for i in (3, 2, 1, 0):
        s = y[i]
        for k in range(i + 1, 4):
            s = s - low[k][i] * x[k]
        x[i] = s / low[i][i]
    return x


def kalman_update(mean, cov, z):
    pm, pc = project(mean, cov)
    low = cholesky(pc)
    b = _matmul(H, cov)                                           # (cov H^T)^T: b[i][j] = sum_k H[i][k] cov[j][k]
    gain = [solve(low, [b[i][r] for i in range(4)]) for r in range(8)]          # 8 x 4
    innovation = [z[i] - pm[i] for i in range(4)]
    step = _matmul([innovation], gain)[0]
    t1 = _matmul(gain, _t(pc))                                    # gain pc, 8 x 4
    t2 = _matmul(t1, gain)
    return [mean[i] + step[i] for i in range(8)], [[cov[i][j] - t2[i][j] for j in range(8)] for i in range(8)]


def to_xyah(tlwh):
    x, y, w, h = tlwh
    return [x + w / 2, y + h / 2, w / h, h]


class Track:
    def __init__(self, tlwh, score):
        self._tlwh = [float(v) for v in tlwh]
        self.mean = self.covariance = None
        self.is_activated = False
        self.score = float(score)
        self.tracklet_len = 0
        self.track_id, self.state = 0, NEW
        self.frame_id = self.start_frame = 0

    end_frame = property(lambda self: self.frame_id)

    @property
    def tlwh(self):
        if self.mean is None:
            return np.array(self._tlwh)
        x, y, a, h = self.mean[:4]
        w = a * h
        return np.array([x - w / 2, y - h / 2, w, h])

    @property
    def tlbr(self):
        x, y, w, h = (float(v) for v in self.tlwh)
        return np.array([x, y, w + x, h + y])

    def activate(self, frame_id, track_id):
        self.track_id = track_id
        self.mean, self.covariance = initiate(to_xyah(self._tlwh))
        self.tracklet_len, self.state = 0, TRACKED
        if frame_id == 1:
            self.is_activated = True
        self.frame_id = self.start_frame = frame_id

    def re_activate(self, det, frame_id):
        self.mean, self.covariance = kalman_update(self.mean, self.covariance, to_xyah([float(v) for v in det.tlwh]))
        self.tracklet_len, self.state, self.is_activated = 0, TRACKED, True
        self.frame_id, self.score = frame_id, det.score

    def update(self, det, frame_id):
        self.frame_id = frame_id
        self.tracklet_len += 1
        self.mean, self.covariance = kalman_update(self.mean, self.covariance, to_xyah([float(v) for v in det.tlwh]))
        self.state, self.is_activated, self.score = TRACKED, True, det.score


def multi_predict(tracks):
    for t in tracks:
        mean = list(t.mean)
        if t.state != TRACKED:
            mean[7] = 0.0
        t.mean, t.covariance = predict(mean, t.covariance)


def iou_cost(a, b, scores=None):
    """1 - IoU in the + 1 convention, n x m lists; with ``scores`` fused: 1 - (1 - cost) * score"""
    out = []
    for p in a:
        p = [float(v) for v in p]
        area_a = (p[2] - p[0] + 1) * (p[3] - p[1] + 1)
        line = []
        for j, q in enumerate(b):
            q = [float(v) for v in q]
            area_b = (q[2] - q[0] + 1) * (q[3] - q[1] + 1)
            iw = min(p[2], q[2]) - max(p[0], q[0]) + 1
            ih = min(p[3], q[3]) - max(p[1], q[1]) + 1
            iou = 0.0
            if iw > 0 and ih > 0:
                inter = iw * ih
                iou = inter / (area_a + area_b - inter)
            cost = 1 - iou
            if scores is not None:
                cost = 1 - (1 - cost) * scores[j]
            line.append(cost)
        out.append(line)
    return out


def linear_assignment(cost, n, m, thresh):
    """``(matches [(row, col)] by ascending row, unmatched rows, unmatched columns)`` of an n x m cost (a list of rows)"""
    if n == 0 or m == 0:
        return [], list(range(n)), list(range(m))
    cols = m + n
    inf = float("inf")
    u, v = [0.0] * (n + 1), [0.0] * (cols + 1)
    owner, way = [0] * (cols + 1), [0] * (cols + 1)              # 1-based; column 0 is the root of a path
    for i in range(1, n + 1):
        owner[0] = i
        j0 = 0
        minv, used = [inf] * (cols + 1), [False] * (cols + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = owner[j0], inf, 0
            for j in range(1, cols + 1):
                if used[j]:
                    continue
                c = cost[i0 - 1][j - 1] if j <= m else thresh
                cur = c - u[i0] - v[j]
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                if minv[j] < delta:
                    delta, j1 = minv[j], j
            for j in range(cols + 1):
                if used[j]:
                    u[owner[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if owner[j0] == 0:
                break
        while j0:
            owner[j0] = owner[way[j0]]
            j0 = way[j0]
    col_of = [-1] * n
    for j in range(1, m + 1):
        if owner[j] and cost[owner[j] - 1][j - 1] <= thresh:
            col_of[owner[j] - 1] = j - 1
    matches = [(i, col_of[i]) for i in range(n) if col_of[i] >= 0]
    hit = {c for _, c in matches}
    return matches, [i for i in range(n) if col_of[i] < 0], [j for j in range(m) if j not in hit]


def _joined(a, b):
    seen, out = set(), []
    for t in list(a) + list(b):
        if t.track_id not in seen:
            seen.add(t.track_id)
            out.append(t)
    return out


def _without(a, drop):
    keep = {}
    for t in a:
        keep[t.track_id] = t
    return [t for tid, t in keep.items() if tid not in drop]


def _drop_duplicates(a, b):
    dist = iou_cost([t.tlbr for t in a], [t.tlbr for t in b])
    da, db = set(), set()
    for p in range(len(a)):
        for q in range(len(b)):
            if dist[p][q] < 0.15:
                if a[p].frame_id - a[p].start_frame > b[q].frame_id - b[q].start_frame:
                    db.add(q)
                else:
                    da.add(p)
    return [t for i, t in enumerate(a) if i not in da], [t for i, t in enumerate(b) if i not in db]


class RefByteTracker:
    """``tracker.ByteTracker``'s interface (``mot20`` False).  ``tracks_in``: a list of objects with ``_tlwh`` / ``tlwh`` and
    ``score`` (``tracker.STrack`` or ``Track``), or the (n, 5) array.  ``removed_ids``: the ids of ``removed_stracks``, in order
    and with its repeats; ``removed_now``: those of the last call."""

    def __init__(self, args, frame_rate=30):
        self.tracked_stracks, self.lost_stracks = [], []
        self.removed_ids, self.removed_now, self._removed_set = [], [], set()
        self.frame_id = 0
        self.track_thresh, self.match_thresh = float(args.track_thresh), float(args.match_thresh)
        self.det_thresh = self.track_thresh + 0.1
        self.max_time_lost = int(frame_rate / 30.0 * args.track_buffer)
        self._count = 0
        self.second_matches = 0

    def _next_id(self):
        self._count += 1
        return self._count

    def _remove(self, removed):
        self.removed_now = [t.track_id for t in removed]
        self.removed_ids += self.removed_now
        self._removed_set |= set(self.removed_now)

    def _nothing_detected(self):
        self.frame_id += 1
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
        self.lost_stracks = _without(self.lost_stracks, {t.track_id for t in removed})
        self._remove(removed)
        self.tracked_stracks, self.lost_stracks = _drop_duplicates(self.tracked_stracks, self.lost_stracks)
        return []

    def update(self, tracks_in, img_info, img_size):
        if isinstance(tracks_in, np.ndarray) and tracks_in.size == 0:
            tracks_in = []
        self.frame_id += 1
        if isinstance(tracks_in, (list, tuple)) and len(tracks_in) == 0:
            return self._nothing_detected()
        activated, refound, lost, removed, second = [], [], [], [], []
        if isinstance(tracks_in, list):
            detections = [Track([float(v) for v in d._tlwh], float(d.score)) for d in tracks_in]
        else:
            scale = min(img_size[0] / float(img_info[1]), img_size[1] / float(img_info[0]))
            detections = []
            for row in tracks_in:
                x0, y0, x1, y1 = (float(v) / scale for v in row[:4])
                s = float(row[4])
                if s > self.track_thresh:
                    detections.append(Track([x0, y0, x1 - x0, y1 - y0], s))
                elif 0.1 < s < self.track_thresh:
                    second.append(Track([x0, y0, x1 - x0, y1 - y0], s))

        unconfirmed = [t for t in self.tracked_stracks if not t.is_activated]
        confirmed = [t for t in self.tracked_stracks if t.is_activated]
        pool = _joined(confirmed, self.lost_stracks)
        multi_predict(pool)
        dists = iou_cost([t.tlbr for t in pool], [d.tlbr for d in detections], [d.score for d in detections])
        matches, u_track, u_det = linear_assignment(dists, len(pool), len(detections), self.match_thresh)
        for it, idet in matches:
            t = pool[it]
            if t.state == TRACKED:
                t.update(detections[idet], self.frame_id)
                activated.append(t)
            else:
                t.re_activate(detections[idet], self.frame_id)
                refound.append(t)

        rest = [pool[i] for i in u_track if pool[i].state == TRACKED]
        matches, u_rest, _ = linear_assignment(iou_cost([t.tlbr for t in rest], [d.tlbr for d in second]), len(rest), len(second), 0.5)
        self.second_matches += 1 if matches else 0
        for it, idet in matches:
            rest[it].update(second[idet], self.frame_id)
            activated.append(rest[it])
        for it in u_rest:
            rest[it].state = LOST
            lost.append(rest[it])

        detections = [detections[i] for i in u_det]
        dists = iou_cost([t.tlbr for t in unconfirmed], [d.tlbr for d in detections], [d.score for d in detections])
        matches, u_unconfirmed, u_det = linear_assignment(dists, len(unconfirmed), len(detections), 0.7)
        for it, idet in matches:
            unconfirmed[it].update(detections[idet], self.frame_id)
            activated.append(unconfirmed[it])
        for it in u_unconfirmed:
            unconfirmed[it].state = REMOVED
            removed.append(unconfirmed[it])

        for i in u_det:
            if detections[i].score < self.det_thresh:
                continue
            detections[i].activate(self.frame_id, self._next_id())
            activated.append(detections[i])

        for t in self.lost_stracks:
            if self.frame_id - t.end_frame > self.max_time_lost:
                t.state = REMOVED
                removed.append(t)

        self.tracked_stracks = [t for t in self.tracked_stracks if t.state == TRACKED]
        self.tracked_stracks = _joined(_joined(self.tracked_stracks, activated), refound)
        self.lost_stracks = _without(self.lost_stracks, {t.track_id for t in self.tracked_stracks})
        self.lost_stracks.extend(lost)
        self.lost_stracks = _without(self.lost_stracks, self._removed_set)         # this frame's removals leave one call later
        self._remove(removed)
        self.tracked_stracks, self.lost_stracks = _drop_duplicates(self.tracked_stracks, self.lost_stracks)
        return [t for t in self.tracked_stracks if t.is_activated]
