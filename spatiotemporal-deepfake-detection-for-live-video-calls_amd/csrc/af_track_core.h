// ByteTrack for one tracker and one frame: the whole of tracker.ByteTracker.update (tracker.py), once as source for the device and
// the host (include/af_hip.h, "device tracker"; the numpy statement is tests/bytetrack_ref.py).
//
// The same functions run as one wave of 64 lanes on the device and as plain loops on the host:
//   TRK_FOR(i, n)   lane l takes i = l, l + 64, ... on the device; the host walks 0 .. n - 1
//   TRK_LANE0       the list bookkeeping: one lane on the device, everything on the host
//   TRK_SYNC()      __syncthreads() of the one-wave workgroup; between a lane-0 section and the lanes that read what it wrote
// Lanes map to the 8 x 8 elements of a covariance in the Kalman products and to (track, detection) pairs in the IoU matrices.
// Arithmetic: fp64, the including file sits below `#pragma clang fp contract(off)`; every product of matrices sums over k ascending
// from 0.0, one rounding per multiply and per add, zeros of the motion and observation matrices included; the 4 x 4 Cholesky
// factor goes row by row and the two triangular solves subtract over k ascending - the order tests/bytetrack_ref.py writes out.
// The assignment is the rectangular form of tracker.linear_assignment's (n + m)^2 matrix: n rows, the m cost columns and n more
// at `thresh` (a row left alone), solved by shortest augmenting paths with potentials on lane 0.
// Bounds: lists and slots are indexed only below TRK_S, rows only below the call's limit; the record's lists are cut at TRK_T.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/af_hip.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TRK_FOR(i, n) for (int i = (int)threadIdx.x; i < (n); i += 64)
#define TRK_SYNC() __syncthreads()
#define TRK_LANE0 (threadIdx.x == 0)
#else
#define TRK_FOR(i, n) for (int i = 0; i < (n); ++i)
#define TRK_SYNC() ((void)0)
#define TRK_LANE0 true
#endif
#define TRK_HD __host__ __device__ static inline

namespace af {
namespace trk {

constexpr int TRK_T = AF_TRACK_MAX_TRACKS, TRK_D = AF_TRACK_MAX_DETS, TRK_S = TRK_T + TRK_D, TRK_C = TRK_T + TRK_D + 1;
constexpr int32_t TRK_MAGIC = 0x4b525442;                     // "BTRK"
enum { ST_NEW = 0, ST_TRACKED = 1, ST_LOST = 2, ST_REMOVED = 3 };

struct Slot {
    double mean[8], cov[64], tlwh[4], score;
    int32_t id, state, activated, frame_id, start_frame, tracklet_len, was_removed, in_use;
};
struct State {
    int32_t magic, frame_id, count, n_tracked, n_lost, max_time_lost, overflowed, reserved;
    double track_thresh, match_thresh, det_thresh, reserved2;
    int32_t tracked[TRK_S], lost[TRK_S];                      // slot indices, in the order of tracked_stracks / lost_stracks
    Slot slot[TRK_S];
};
struct OnlineRow {
    double tlbr[4], score;
    int32_t id, state, activated, reserved;
};
struct Record {
    int32_t frame_id, overflow, n_online, n_tracked, n_lost, n_removed, reserved[2];
    OnlineRow online[TRK_T];
    int32_t tracked_ids[TRK_T], lost_ids[TRK_T], removed_ids[TRK_T];
};
struct Call {                                                 // af_track_call as the core reads it
    State* state;
    const void* rows;
    const int32_t* count_ptr;
    int32_t limit, form, stride;
    float start_conf, start_min_size;
    double sx, sy;                                            // list form: the scale-back; array form: sx is the box divisor
    const int32_t* pick;                                      // TRK_FORM_PICKED: the `limit` row indices that enter, in order
};
constexpr int32_t TRK_FORM_PICKED = 4;                        // the evaluator's loop (af_runner_core.h); not a form of af_track_call
struct Scratch {                                              // LDS on the device
    double cost[TRK_T * TRK_D];
    double P[64], m[8], z[4];
    double det_tlwh[TRK_D][4], det_score[TRK_D];
    double u[TRK_T + 1], v[TRK_C], minv[TRK_C];
    int32_t owner[TRK_C], way[TRK_C], used[TRK_C];
    int32_t match[TRK_T], colhit[TRK_D];
    int32_t hi[TRK_D], lo[TRK_D], pool[TRK_T], unconfirmed[TRK_T], rest[TRK_T];
    int32_t activated[TRK_S], refound[TRK_T], lost_new[TRK_T], removed[TRK_T], seen[TRK_S], da[TRK_S], db[TRK_S];
    int32_t n_hi, n_lo, n_pool, n_unc, n_rest, n_act, n_ref, n_lost_new, n_removed, overflow, empty, fid;
};

TRK_HD double motion(int i, int j) { return (i == j || j == i + 4) ? 1.0 : 0.0; }
TRK_HD double observe(int i, int j) { return i == j ? 1.0 : 0.0; }
constexpr double TRK_W_POS = 1.0 / 20, TRK_W_VEL = 1.0 / 160;

TRK_HD void slot_tlbr(const Slot& s, double* o) {             // STrack.tlwh, .tlbr of a track with a mean
    const double h = s.mean[3], w = s.mean[2] * h;
    const double x = s.mean[0] - w / 2, y = s.mean[1] - h / 2;
    o[0] = x; o[1] = y; o[2] = w + x; o[3] = h + y;
}
TRK_HD void det_tlbr(const double* t, double* o) { o[0] = t[0]; o[1] = t[1]; o[2] = t[2] + t[0]; o[3] = t[3] + t[1]; }

TRK_HD double iou_cost(const double* p, const double* q) {     // 1 - IoU, the + 1 convention
    const double area_a = (p[2] - p[0] + 1) * (p[3] - p[1] + 1), area_b = (q[2] - q[0] + 1) * (q[3] - q[1] + 1);
    const double iw = (p[2] < q[2] ? p[2] : q[2]) - (p[0] > q[0] ? p[0] : q[0]) + 1;
    const double ih = (p[3] < q[3] ? p[3] : q[3]) - (p[1] > q[1] ? p[1] : q[1]) + 1;
    double iou = 0.0;
    if (iw > 0 && ih > 0) {
        const double inter = iw * ih;
        iou = inter / (area_a + area_b - inter);
    }
    return 1 - iou;
}

// ---- Kalman filter: one element (r, c) of the new covariance, and for c == 0 entry r of the new mean, from the staged copies ----
TRK_HD void predict_elem(const double* P, const double* m, int r, int c, double* cov_out, double* mean_out) {
    const double h = m[3];
    double left[8];
    for (int j = 0; j < 8; ++j) {
        double acc = 0.0;
        for (int k = 0; k < 8; ++k) acc = acc + motion(r, k) * P[k * 8 + j];
        left[j] = acc;
    }
    double acc = 0.0;
    for (int k = 0; k < 8; ++k) acc = acc + left[k] * motion(c, k);
    double noise = 0.0;
    if (r == c) {
        const double std = (r == 2) ? 1e-2 : (r == 6) ? 1e-5 : (r < 4 ? TRK_W_POS * h : TRK_W_VEL * h);
        noise = std * std;
    }
    *cov_out = acc + noise;
    if (c == 0) {
        double a = 0.0;
        for (int k = 0; k < 8; ++k) a = a + m[k] * motion(r, k);
        *mean_out = a;
    }
}

TRK_HD void solve4(const double* L, const double* b, double* x) {
    double y[4];
    for (int i = 0; i < 4; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - L[i * 4 + k] * y[k];
        y[i] = s / L[i * 4 + i];
    }
    for (int i = 3; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 4; ++k) s = s - L[k * 4 + i] * x[k];
        x[i] = s / L[i * 4 + i];
    }
}

TRK_HD void update_elem(const double* P, const double* m, const double* z, int r, int c, double* cov_out, double* mean_out) {
    const double h = m[3];
    double pm[4], hp[32], pc[16], L[16];
    for (int i = 0; i < 4; ++i) {
        double acc = 0.0;
        for (int k = 0; k < 8; ++k) acc = acc + observe(i, k) * m[k];
        pm[i] = acc;
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 8; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 8; ++k) acc = acc + observe(i, k) * P[k * 8 + j];
            hp[i * 8 + j] = acc;
        }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 8; ++k) acc = acc + hp[i * 8 + k] * observe(j, k);
            double noise = 0.0;
            if (i == j) {
                const double std = (i == 2) ? 1e-1 : TRK_W_POS * h;
                noise = std * std;
            }
            pc[i * 4 + j] = acc + noise;
        }
    for (int i = 0; i < 16; ++i) L[i] = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = pc[i * 4 + j];
            for (int k = 0; k < j; ++k) s = s - L[i * 4 + k] * L[j * 4 + k];
            L[i * 4 + j] = (i == j) ? sqrt(s) : s / L[j * 4 + j];
        }
    double gr[4], gc[4], b[4];
    for (int i = 0; i < 4; ++i) {
        double acc = 0.0;
        for (int k = 0; k < 8; ++k) acc = acc + observe(i, k) * P[r * 8 + k];
        b[i] = acc;
    }
    solve4(L, b, gr);
    for (int i = 0; i < 4; ++i) {
        double acc = 0.0;
        for (int k = 0; k < 8; ++k) acc = acc + observe(i, k) * P[c * 8 + k];
        b[i] = acc;
    }
    solve4(L, b, gc);
    double t1[4];
    for (int j = 0; j < 4; ++j) {
        double acc = 0.0;
        for (int k = 0; k < 4; ++k) acc = acc + gr[k] * pc[k * 4 + j];
        t1[j] = acc;
    }
    double t2 = 0.0;
    for (int k = 0; k < 4; ++k) t2 = t2 + t1[k] * gc[k];
    *cov_out = P[r * 8 + c] - t2;
    if (c == 0) {
        double step = 0.0;
        for (int k = 0; k < 4; ++k) step = step + (z[k] - pm[k]) * gr[k];
        *mean_out = m[r] + step;
    }
}

// the slot's mean and covariance one step on (predict != 0) or corrected by the measurement sc->z; every lane takes part
TRK_HD void kalman(Slot& s, Scratch* sc, int predict) {
    TRK_FOR(l, 64) {
        sc->P[l] = s.cov[l];
        if (l < 8) sc->m[l] = (predict && l == 7 && s.state != ST_TRACKED) ? 0.0 : s.mean[l];
    }
    TRK_SYNC();
    TRK_FOR(l, 64) {
        double cv, mv = 0.0;
        if (predict) predict_elem(sc->P, sc->m, l >> 3, l & 7, &cv, &mv);
        else update_elem(sc->P, sc->m, sc->z, l >> 3, l & 7, &cv, &mv);
        s.cov[l] = cv;
        if ((l & 7) == 0) s.mean[l >> 3] = mv;
    }
    TRK_SYNC();
}

// ---- assignment (lane 0): sc->match[i] = the column of row i or -1, sc->colhit[j] ----
TRK_HD void assign(Scratch* sc, int n, int m, double thresh) {
    for (int i = 0; i < n; ++i) sc->match[i] = -1;
    for (int j = 0; j < m; ++j) sc->colhit[j] = 0;
    if (n == 0 || m == 0) return;
    const int cols = m + n;
    const double inf = INFINITY;
    for (int i = 0; i <= n; ++i) sc->u[i] = 0.0;
    for (int j = 0; j <= cols; ++j) { sc->v[j] = 0.0; sc->owner[j] = 0; sc->way[j] = 0; }
    for (int i = 1; i <= n; ++i) {
        sc->owner[0] = i;
        int j0 = 0;
        for (int j = 0; j <= cols; ++j) { sc->minv[j] = inf; sc->used[j] = 0; }
        for (int guard = 0; guard <= cols; ++guard) {          // a path visits a column once: at most cols + 1 rounds
            sc->used[j0] = 1;
            const int i0 = sc->owner[j0];
            double delta = inf;
            int j1 = 0;
            for (int j = 1; j <= cols; ++j) {
                if (sc->used[j]) continue;
                const double cst = j <= m ? sc->cost[(i0 - 1) * m + (j - 1)] : thresh;
                const double cur = cst - sc->u[i0] - sc->v[j];
                if (cur < sc->minv[j]) { sc->minv[j] = cur; sc->way[j] = j0; }
                if (sc->minv[j] < delta) { delta = sc->minv[j]; j1 = j; }
            }
            for (int j = 0; j <= cols; ++j) {
                if (sc->used[j]) { sc->u[sc->owner[j]] += delta; sc->v[j] -= delta; }
                else sc->minv[j] -= delta;
            }
            j0 = j1;
            if (sc->owner[j0] == 0) break;
        }
        for (int guard = 0; guard <= cols && j0; ++guard) {
            sc->owner[j0] = sc->owner[sc->way[j0]];
            j0 = sc->way[j0];
        }
    }
    for (int j = 1; j <= m; ++j) {
        const int i = sc->owner[j];
        if (i >= 1 && i <= n && sc->cost[(i - 1) * m + (j - 1)] <= thresh) { sc->match[i - 1] = j - 1; sc->colhit[j - 1] = 1; }
    }
}

// the cost matrix of rows (slots) against cols (detections) into sc->cost, then the assignment
TRK_HD void associate(State* st, Scratch* sc, const int32_t* rows, int n, const int32_t* cols, int m, int fuse, double thresh) {
    TRK_FOR(p, n * m) {
        const int i = p / m, j = p % m;
        double a[4], b[4];
        slot_tlbr(st->slot[rows[i]], a);
        det_tlbr(sc->det_tlwh[cols[j]], b);
        double cst = iou_cost(a, b);
        if (fuse) cst = 1 - (1 - cst) * sc->det_score[cols[j]];
        sc->cost[p] = cst;
    }
    TRK_SYNC();
    if (TRK_LANE0) assign(sc, n, m, thresh);
    TRK_SYNC();
}

// a matched pair: the Kalman correction by every lane, the track's books by lane 0 (STrack.update / .re_activate)
TRK_HD void matched(State* st, Scratch* sc, int slot, int det) {
    Slot& s = st->slot[slot];
    if (TRK_LANE0) {
        const double* t = sc->det_tlwh[det];
        sc->z[0] = t[0] + t[2] / 2; sc->z[1] = t[1] + t[3] / 2; sc->z[2] = t[2] / t[3]; sc->z[3] = t[3];
    }
    TRK_SYNC();
    kalman(s, sc, 0);
    if (TRK_LANE0) {
        if (s.state == ST_TRACKED) {
            s.tracklet_len += 1;
            sc->activated[sc->n_act++] = slot;
        } else {
            s.tracklet_len = 0;
            sc->refound[sc->n_ref++] = slot;
        }
        s.frame_id = sc->fid;
        s.state = ST_TRACKED;
        s.activated = 1;
        s.score = sc->det_score[det];
    }
    TRK_SYNC();
}

// the call's rows into sc->det_*, split into hi (first association) and lo (second); lane 0
TRK_HD void parse(const State* st, const Call& c, Scratch* sc) {
    sc->n_hi = sc->n_lo = 0;
    sc->overflow = 0;
    int n = 0, kept = 0;
    if (c.form != AF_TRACK_FORM_EMPTY) {
        n = c.count_ptr ? *c.count_ptr : c.limit;
        if (n > c.limit) n = c.limit;
    }
    for (int i = 0; i < n; ++i) {
        double t[4], score;
        int low = 0;
        if (c.form == TRK_FORM_PICKED) {                       // runner.py:251: STrack(tlbr, score) - the corner enters as (w, h)
            const float* r = (const float*)c.rows + (int64_t)c.pick[i] * c.stride;
            const float x1 = r[0] + r[2], y1 = r[1] + r[3];
            t[0] = r[0]; t[1] = r[1]; t[2] = x1; t[3] = y1; score = r[4];
        } else if (c.form == AF_TRACK_FORM_LIST) {
            const float* r = (const float*)c.rows + (int64_t)i * c.stride;
            const float x = (float)((double)r[0] * c.sx), y = (float)((double)r[1] * c.sy);
            const float w = (float)((double)r[2] * c.sx), h = (float)((double)r[3] * c.sy);
            const float s = (float)((double)r[4] * c.sx);      // YuNet.scale_rows scales every even column, the one :385 reads as the score too
            if (!(s >= c.start_conf && (w > h ? w : h) >= c.start_min_size)) continue;
            t[0] = x; t[1] = y; t[2] = w; t[3] = h; score = s;
        } else if (c.form == AF_TRACK_FORM_LIST64) {
            const double* r = (const double*)c.rows + (int64_t)i * c.stride;
            t[0] = r[0]; t[1] = r[1]; t[2] = r[2]; t[3] = r[3]; score = r[4];
        } else {
            const double* r = (const double*)c.rows + (int64_t)i * c.stride;
            const double x0 = r[0] / c.sx, y0 = r[1] / c.sx, x1 = r[2] / c.sx, y1 = r[3] / c.sx;
            score = r[4];
            if (score > st->track_thresh) low = 0;
            else if (score > 0.1 && score < st->track_thresh) low = 1;
            else continue;
            t[0] = x0; t[1] = y0; t[2] = x1 - x0; t[3] = y1 - y0;
        }
        if (kept == TRK_D) { sc->overflow = AF_TRACK_OVERFLOW_DETS; return; }
        for (int k = 0; k < 4; ++k) sc->det_tlwh[kept][k] = t[k];
        sc->det_score[kept] = score;
        if (low) sc->lo[sc->n_lo++] = kept; else sc->hi[sc->n_hi++] = kept;
        ++kept;
    }
    sc->empty = n == 0 || (c.form != AF_TRACK_FORM_ARRAY && kept == 0);
}

// _drop_duplicates on the state's lists, then the record; the slots no list names are freed
TRK_HD void finish(State* st, Scratch* sc, Record* rec, int overflow) {
    const int na = st->n_tracked, nb = st->n_lost;
    TRK_FOR(i, TRK_S) { sc->da[i] = 0; sc->db[i] = 0; }
    TRK_SYNC();
    if (!overflow) {
        TRK_FOR(p, na * nb) {
            const int i = p / nb, j = p % nb;
            const Slot& a = st->slot[st->tracked[i]];
            const Slot& b = st->slot[st->lost[j]];
            double ta[4], tb[4];
            slot_tlbr(a, ta);
            slot_tlbr(b, tb);
            if (iou_cost(ta, tb) < 0.15) {
                if (a.frame_id - a.start_frame > b.frame_id - b.start_frame) sc->db[j] = 1; else sc->da[i] = 1;
            }
        }
    }
    TRK_SYNC();
    if (TRK_LANE0) {
        int k = 0;
        for (int i = 0; i < na; ++i) if (!sc->da[i]) st->tracked[k++] = st->tracked[i];
        st->n_tracked = k;
        k = 0;
        for (int j = 0; j < nb; ++j) if (!sc->db[j]) st->lost[k++] = st->lost[j];
        st->n_lost = k;
        for (int i = 0; i < TRK_S; ++i) st->slot[i].in_use = 0;
        for (int i = 0; i < st->n_tracked; ++i) st->slot[st->tracked[i]].in_use = 1;
        for (int j = 0; j < st->n_lost; ++j) st->slot[st->lost[j]].in_use = 1;
        if (overflow) st->overflowed = overflow;
        rec->frame_id = st->frame_id;
        rec->overflow = overflow;
        rec->n_tracked = st->n_tracked < TRK_T ? st->n_tracked : TRK_T;
        rec->n_lost = st->n_lost < TRK_T ? st->n_lost : TRK_T;
        rec->n_removed = sc->n_removed;
        int on = 0;
        for (int i = 0; i < rec->n_tracked; ++i) {
            const Slot& s = st->slot[st->tracked[i]];
            rec->tracked_ids[i] = s.id;
            if (!s.activated || sc->empty) continue;
            OnlineRow& o = rec->online[on++];
            slot_tlbr(s, o.tlbr);
            o.score = s.score; o.id = s.id; o.state = s.state; o.activated = s.activated; o.reserved = 0;
        }
        rec->n_online = on;
        for (int j = 0; j < rec->n_lost; ++j) rec->lost_ids[j] = st->slot[st->lost[j]].id;
        for (int i = 0; i < sc->n_removed; ++i) rec->removed_ids[i] = st->slot[sc->removed[i]].id;
        rec->reserved[0] = rec->reserved[1] = 0;
    }
    TRK_SYNC();
}

TRK_HD void refuse(const State* st, Record* rec, int code) {
    if (TRK_LANE0) {
        rec->frame_id = st->magic == TRK_MAGIC ? st->frame_id : 0;
        rec->overflow = code;
        rec->n_online = rec->n_tracked = rec->n_lost = rec->n_removed = 0;
        rec->reserved[0] = rec->reserved[1] = 0;
    }
}

TRK_HD void update(const Call& c, Record* rec, Scratch* sc) {
    State* st = c.state;
    if (st->magic != TRK_MAGIC) { refuse(st, rec, AF_TRACK_NOT_RESET); return; }
    if (st->overflowed) { refuse(st, rec, st->overflowed); return; }
    if (TRK_LANE0) {
        parse(st, c, sc);
        sc->n_act = sc->n_ref = sc->n_lost_new = sc->n_removed = sc->n_pool = sc->n_unc = sc->n_rest = 0;
    }
    TRK_SYNC();
    if (sc->overflow) { refuse(st, rec, sc->overflow); return; }

    if (sc->empty) {                                           // _nothing_detected
        if (TRK_LANE0) {
            st->frame_id += 2;
            for (int i = 0; i < st->n_tracked; ++i) {
                st->slot[st->tracked[i]].state = ST_LOST;
                st->lost[st->n_lost++] = st->tracked[i];
            }
            st->n_tracked = 0;
            int k = 0;
            for (int j = 0; j < st->n_lost; ++j) {
                Slot& s = st->slot[st->lost[j]];
                if (st->frame_id - s.frame_id > st->max_time_lost) {
                    s.state = ST_REMOVED;
                    s.was_removed = 1;
                    sc->removed[sc->n_removed++] = st->lost[j];
                } else st->lost[k++] = st->lost[j];
            }
            st->n_lost = k;
        }
        TRK_SYNC();
        finish(st, sc, rec, 0);
        return;
    }

    if (TRK_LANE0) {
        st->frame_id += 1;
        sc->fid = st->frame_id;
        for (int i = 0; i < st->n_tracked; ++i) {
            const int s = st->tracked[i];
            if (st->slot[s].activated) sc->pool[sc->n_pool++] = s; else sc->unconfirmed[sc->n_unc++] = s;
        }
        for (int j = 0; j < st->n_lost; ++j) sc->pool[sc->n_pool++] = st->lost[j];
    }
    TRK_SYNC();
    for (int p = 0; p < sc->n_pool; ++p) kalman(st->slot[sc->pool[p]], sc, 1);

    // first association: confirmed and lost tracks against the high-score detections
    associate(st, sc, sc->pool, sc->n_pool, sc->hi, sc->n_hi, 1, st->match_thresh);
    for (int i = 0; i < sc->n_pool; ++i)
        if (sc->match[i] >= 0) matched(st, sc, sc->pool[i], sc->hi[sc->match[i]]);
    if (TRK_LANE0) {
        for (int i = 0; i < sc->n_pool; ++i)
            if (sc->match[i] < 0 && st->slot[sc->pool[i]].state == ST_TRACKED) sc->rest[sc->n_rest++] = sc->pool[i];
        int k = 0;                                             // the detections the first association left, in order
        for (int j = 0; j < sc->n_hi; ++j) if (!sc->colhit[j]) sc->hi[k++] = sc->hi[j];
        sc->n_hi = k;
    }
    TRK_SYNC();

    // second association: the tracked faces still unmatched against the low-score detections, by IoU alone
    associate(st, sc, sc->rest, sc->n_rest, sc->lo, sc->n_lo, 0, 0.5);
    for (int i = 0; i < sc->n_rest; ++i) {
        if (sc->match[i] >= 0) matched(st, sc, sc->rest[i], sc->lo[sc->match[i]]);
        else if (TRK_LANE0) {
            st->slot[sc->rest[i]].state = ST_LOST;
            sc->lost_new[sc->n_lost_new++] = sc->rest[i];
        }
    }
    TRK_SYNC();

    // unconfirmed tracks against what the first association left; an unmatched one dies
    associate(st, sc, sc->unconfirmed, sc->n_unc, sc->hi, sc->n_hi, 1, 0.7);
    for (int i = 0; i < sc->n_unc; ++i) {
        if (sc->match[i] >= 0) matched(st, sc, sc->unconfirmed[i], sc->hi[sc->match[i]]);
        else if (TRK_LANE0) {
            st->slot[sc->unconfirmed[i]].state = ST_REMOVED;
            sc->removed[sc->n_removed++] = sc->unconfirmed[i];
        }
    }
    TRK_SYNC();

    if (TRK_LANE0) {
        int overflow = 0;
        for (int j = 0; j < sc->n_hi && !overflow; ++j) {      // new tracks
            if (sc->colhit[j]) continue;
            const int d = sc->hi[j];
            if (sc->det_score[d] < st->det_thresh) continue;
            int free_slot = -1;
            for (int i = 0; i < TRK_S && free_slot < 0; ++i) if (!st->slot[i].in_use) free_slot = i;
            if (free_slot < 0) { overflow = AF_TRACK_OVERFLOW_TRACKS; break; }
            Slot& s = st->slot[free_slot];
            const double* t = sc->det_tlwh[d];
            const double h = t[3];
            s.mean[0] = t[0] + t[2] / 2; s.mean[1] = t[1] + t[3] / 2; s.mean[2] = t[2] / t[3]; s.mean[3] = h;
            for (int k = 4; k < 8; ++k) s.mean[k] = 0.0;
            for (int k = 0; k < 64; ++k) s.cov[k] = 0.0;
            for (int k = 0; k < 8; ++k) {
                const double std = (k == 2) ? 1e-2 : (k == 6) ? 1e-5 : (k < 4 ? 2 * TRK_W_POS * h : 10 * TRK_W_VEL * h);
                s.cov[k * 8 + k] = std * std;
            }
            for (int k = 0; k < 4; ++k) s.tlwh[k] = t[k];
            s.score = sc->det_score[d];
            s.id = ++st->count;
            s.state = ST_TRACKED;
            s.activated = sc->fid == 1 ? 1 : 0;
            s.frame_id = s.start_frame = sc->fid;
            s.tracklet_len = 0;
            s.was_removed = 0;
            s.in_use = 1;
            sc->activated[sc->n_act++] = free_slot;
        }
        for (int j = 0; j < st->n_lost; ++j) {
            Slot& s = st->slot[st->lost[j]];
            if (sc->fid - s.frame_id > st->max_time_lost) {
                s.state = ST_REMOVED;
                sc->removed[sc->n_removed++] = st->lost[j];
            }
        }
        // tracked = joined(joined(still tracked, activated), refound); lost = without(lost, tracked) + newly lost, less the
        // tracks removed on an EARLIER call: this call's removals stay in the lost list until the next one
        for (int i = 0; i < TRK_S; ++i) sc->seen[i] = 0;
        int k = 0;
        for (int i = 0; i < st->n_tracked; ++i) {
            const int s = st->tracked[i];
            if (st->slot[s].state == ST_TRACKED && !sc->seen[s]) { sc->seen[s] = 1; st->tracked[k++] = s; }
        }
        for (int i = 0; i < sc->n_act; ++i) {
            const int s = sc->activated[i];
            if (!sc->seen[s]) { sc->seen[s] = 1; st->tracked[k++] = s; }
        }
        for (int i = 0; i < sc->n_ref; ++i) {
            const int s = sc->refound[i];
            if (!sc->seen[s]) { sc->seen[s] = 1; st->tracked[k++] = s; }
        }
        st->n_tracked = k;
        k = 0;
        for (int j = 0; j < st->n_lost; ++j) {
            const int s = st->lost[j];
            if (!sc->seen[s] && !st->slot[s].was_removed) st->lost[k++] = s;
        }
        for (int j = 0; j < sc->n_lost_new; ++j) {
            const int s = sc->lost_new[j];
            if (!st->slot[s].was_removed) st->lost[k++] = s;
        }
        st->n_lost = k;
        for (int i = 0; i < sc->n_removed; ++i) st->slot[sc->removed[i]].was_removed = 1;
        if (!overflow && st->n_tracked + st->n_lost > TRK_T) overflow = AF_TRACK_OVERFLOW_TRACKS;
        sc->overflow = overflow;
    }
    TRK_SYNC();
    finish(st, sc, rec, sc->overflow);
}

}  // namespace trk
}  // namespace af
