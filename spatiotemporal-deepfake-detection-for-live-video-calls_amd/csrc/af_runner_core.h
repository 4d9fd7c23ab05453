// The dataset evaluator's chunk stage: what runner.VideoRunner.run does on the host for every kept frame of a chunk (the loop's
// host stage and runner.track_stage), once as source for the device and the host (include/af_hip.h, "chunk stage"; the
// numpy statement is tests/runner_chunk_ref.py).
//
// One wave per run walks the chunk's frames in order.  Per frame lane 0 decides (rhythm, smart start, budget) and filters the
// detector's rows into a list of row indices; af_track_core.h's update runs on that list with every lane (TRK_FORM_PICKED) and
// leaves its record in the scratch; lane 0 then does the frame's bookkeeping - min_track_side, the id-switch count, the
// five-point pick, the mesh_every cache, get_crop_box - and appends the frame's candidates to the chunk record.
// Arithmetic: the detection filters and the start in float32, everything else fp64, under `#pragma clang fp contract(off)` of the
// including file; float32 boxes are widened to fp64 before an IoU, as tracker.ious does.
// Bounds: frames below c.n_frames <= AF_RUNNER_MAX_FRAMES, rows below min(counts[j], c.max_rows), picked rows below TRK_D, tracks
// below TRK_T, slots below TRK_S, candidates below n_frames * TRK_T (a frame appends at most TRK_T); all checked on the host or
// compile-time constants.
#pragma once
#include "af_track_core.h"

namespace af {
namespace run {

using trk::TRK_D;
using trk::TRK_S;
using trk::TRK_T;
constexpr int32_t RUN_MAGIC = 0x4e555243;                     // "CRUN"
constexpr int RUN_TILE_H = 8, RUN_TILE_W = 32;                // af_quality.hip's tile of measured pixels

struct State {
    trk::State trk;
    int32_t magic, started, consec, processed_after_start, stop, id_switches, frames_seen, n_prev;
    float prev_boxes[TRK_T][4];
    int32_t prev_ids[TRK_T];
    int32_t cache_tid[TRK_S];                                 // 0: no entry; else the track the slot's points belong to
    float cache_lm[TRK_S][10];
};
struct Record {
    af_runner_header head;
    af_runner_frame frames[AF_RUNNER_MAX_FRAMES];
    af_runner_cand cands[1];                                  // n_frames * TRK_T of them
};
struct Scratch {                                              // LDS on the device
    trk::Scratch trk;
    trk::Record rec;
    int32_t pick[TRK_D];
    float det_tlbr[TRK_D][4];
    float cur_boxes[TRK_T][4];
    int32_t cur_ids[TRK_T], cur_row[TRK_T];
    int32_t action, n_pick, n_cur;
};
enum { ACT_NEXT = 0, ACT_TRACK = 1, ACT_END = 2 };

TRK_HD int tiles_of(int w, int h) { return ((w + RUN_TILE_W - 1) / RUN_TILE_W) * ((h + RUN_TILE_H - 1) / RUN_TILE_H); }
TRK_HD double clamp_to(double v, double hi) { return fmin(fmax(v, 0.0), hi); }
TRK_HD void widen(const float* b, double* o) { for (int k = 0; k < 4; ++k) o[k] = (double)b[k]; }

// YuNet's five points for a track: of n rows - det(d, t) puts row d's float32 (x, y, x + w, y + h) into t - the first of highest
// IoU with the track's float32 box, if that IoU is 0.4 or more; else -1.  Shared with the live candidate stage (af_live_core.h).
template <class Det>
TRK_HD int pick_row(const float* box, int n, Det det) {
    double a[4], b[4], best = 0.0;
    int at = -1;
    widen(box, a);
    for (int d = 0; d < n; ++d) {
        float t[4];
        det(d, t);
        widen(t, b);
        const double iou = 1.0 - trk::iou_cost(a, b);
        if (at < 0 || iou > best) { best = iou; at = d; }
    }
    return (at >= 0 && best >= 0.4) ? at : -1;
}

// get_crop_box((frame_h, frame_w), b, scale), fp64: the box rounded, grown by scale times its sides, cut to the frame and rounded
// again; false when the rectangle is empty
TRK_HD bool crop_box(const double* b, double scale, int frame_w, int frame_h, int32_t* box) {
    const double x0 = rint(b[0]), y0 = rint(b[1]), x1 = rint(b[2]), y1 = rint(b[3]);
    const double gx = scale * (x1 - x0), gy = scale * (y1 - y0);
    const double wm = (double)frame_w - 1.0, hm = (double)frame_h - 1.0;
    box[0] = (int)rint(clamp_to(x0 - gx, wm)); box[1] = (int)rint(clamp_to(y0 - gy, hm));
    box[2] = (int)rint(clamp_to(x1 + gx, wm)); box[3] = (int)rint(clamp_to(y1 + gy, hm));
    return box[2] > box[0] && box[3] > box[1];
}

// lane 0: the frame's fate before the tracker.  Returns ACT_TRACK with sc->pick / sc->n_pick set when the tracker is to run.
TRK_HD int before(const af_runner_chunk& c, int j, State* rs, Record* out, Scratch* sc) {
    const int k = c.frame_idx[j];
    af_runner_frame& fr = out->frames[j];
    const bool need = !rs->started || (k % c.detect_every) == 0 || rs->trk.n_tracked == 0;
    int cnt = need ? c.counts[j] : 0;
    if (cnt > c.max_rows) cnt = c.max_rows;
    if (cnt < 0) cnt = 0;
    const float* rows = c.rows + (int64_t)j * c.max_rows * c.row_stride;
    fr.flags = need ? AF_RUNNER_NEED_DETECT : 0;
    fr.n_rows = fr.n_ids = fr.reserved = 0;
    if (!rs->started) {                                        // the smart start: these frames are dropped
        bool valid = false;
        for (int i = 0; i < cnt && !valid; ++i) {
            const float* r = rows + (int64_t)i * c.row_stride;
            valid = r[4] >= c.start_conf && (r[2] > r[3] ? r[2] : r[3]) >= c.start_min_size;
        }
        rs->consec = valid ? rs->consec + 1 : 0;
        if (rs->consec >= c.start_after_n) rs->started = 1;
        fr.flags |= AF_RUNNER_DROPPED;
        return ACT_NEXT;
    }
    if (rs->processed_after_start >= c.budget_frames) {        // the budget: this frame and the rest are left alone
        rs->stop = 1;
        for (int q = j; q < c.n_frames; ++q) {
            af_runner_frame& f = out->frames[q];
            f.flags = AF_RUNNER_NOT_REACHED;
            f.n_rows = f.n_ids = f.reserved = 0;
        }
        return ACT_END;
    }
    int n = 0;
    for (int i = 0; i < cnt; ++i) {                            // filter_detections, float32
        const float* r = rows + (int64_t)i * c.row_stride;
        const float w = r[2], h = r[3], y = r[1];
        if (c.min_det_side > 0.f && !((w > h ? w : h) >= c.min_det_side)) continue;
        if (c.min_det_area > 0.f && !(w * h >= c.min_det_area)) continue;
        if (c.bottom_limit > 0.f && !(y + 0.5f * h < c.bottom_limit)) continue;
        if (n == TRK_D) {                                      // refused before anything of the run has changed
            out->head.overflow = AF_TRACK_OVERFLOW_DETS;
            out->head.overflow_frame = j;
            fr.flags |= AF_RUNNER_REFUSED;
            return ACT_END;
        }
        sc->pick[n] = i;
        sc->det_tlbr[n][0] = r[0]; sc->det_tlbr[n][1] = r[1]; sc->det_tlbr[n][2] = r[0] + r[2]; sc->det_tlbr[n][3] = r[1] + r[3];
        ++n;
    }
    sc->n_pick = n;
    fr.n_rows = n;
    rs->processed_after_start += 1;
    fr.flags |= AF_RUNNER_PROCESSED;
    return ACT_TRACK;
}

// lane 0: runner.track_stage behind the tracker's update, whose record is sc->rec
TRK_HD void after(const af_runner_chunk& c, int j, State* rs, Record* out, Scratch* sc) {
    const int k = c.frame_idx[j];
    af_runner_frame& fr = out->frames[j];
    const float* rows = c.rows + (int64_t)j * c.max_rows * c.row_stride;
    const int n_on = sc->rec.n_online < TRK_T ? sc->rec.n_online : TRK_T;
    int n_cur = 0;
    for (int i = 0; i < n_on; ++i) {                           // min_track_side, fp64
        const double* b = sc->rec.online[i].tlbr;
        const double w = b[2] - b[0], h = b[3] - b[1];
        if ((w > h ? w : h) < c.min_track_side) continue;
        for (int q = 0; q < 4; ++q) sc->cur_boxes[n_cur][q] = (float)b[q];
        sc->cur_ids[n_cur] = sc->rec.online[i].id;
        sc->cur_row[n_cur] = i;
        fr.ids[n_cur] = sc->rec.online[i].id;
        ++n_cur;
    }
    fr.n_ids = n_cur;
    if (n_cur > 0) {                                           // the id coherence against the last frame that had a box
        for (int p = 0; p < rs->n_prev; ++p) {
            double a[4], b[4], best = 0.0;
            int at = -1;
            widen(rs->prev_boxes[p], a);
            for (int q = 0; q < n_cur; ++q) {
                widen(sc->cur_boxes[q], b);
                const double d = trk::iou_cost(a, b);
                if (at < 0 || d < best) { best = d; at = q; }
            }
            if (1.0 - best >= 0.5 && rs->prev_ids[p] != sc->cur_ids[at]) rs->id_switches += 1;
        }
        for (int q = 0; q < n_cur; ++q) {
            for (int e = 0; e < 4; ++e) rs->prev_boxes[q][e] = sc->cur_boxes[q][e];
            rs->prev_ids[q] = sc->cur_ids[q];
        }
        rs->n_prev = n_cur;
    }
    rs->frames_seen += 1;

    const int capacity = c.n_frames * TRK_T;
    for (int q = 0; q < n_cur; ++q) {
        const int tid = sc->cur_ids[q];
        const float* lm = nullptr;
        const int at = pick_row(sc->cur_boxes[q], sc->n_pick, [sc](int d, float* t) { for (int e = 0; e < 4; ++e) t[e] = sc->det_tlbr[d][e]; });
        if (at >= 0) lm = rows + (int64_t)sc->pick[at] * c.row_stride + 5;
        int slot = -1;                                         // the track's slot carries its cache entry
        for (int i = 0; i < rs->trk.n_tracked && i < TRK_S && slot < 0; ++i) {
            const int s = rs->trk.tracked[i];
            if (s >= 0 && s < TRK_S && rs->trk.slot[s].id == tid) slot = s;
        }
        if (slot < 0) continue;                                // an online track is a tracked one: not reached
        const bool cached = rs->cache_tid[slot] == tid;
        if ((k % c.mesh_every) == 0 || !cached) {
            if (!lm) continue;                                 // no points: the face is skipped, the cache stays
            for (int e = 0; e < 10; ++e) rs->cache_lm[slot][e] = lm[e];
            rs->cache_tid[slot] = tid;
        }
        int32_t box[4];
        if (!crop_box(sc->rec.online[sc->cur_row[q]].tlbr, c.crop_scale, c.frame_w, c.frame_h, box)) continue;
        const int bx1 = box[0], by1 = box[1], bx2 = box[2], by2 = box[3];
        const int n = out->head.n_cands;
        if (n >= capacity) continue;                           // a frame appends at most TRK_T: not reached
        af_runner_cand& cd = out->cands[n];
        cd.frame_pos = j; cd.slot = c.first_slot + j; cd.tid = tid; cd.flags = 0;
        for (int e = 0; e < 4; ++e) cd.tlbr[e] = sc->cur_boxes[q][e];
        for (int e = 0; e < 10; ++e) cd.lm5[e] = rs->cache_lm[slot][e];
        cd.box[0] = bx1; cd.box[1] = by1; cd.box[2] = bx2; cd.box[3] = by2;
        const int w = bx2 - bx1, h = by2 - by1;
        cd.tile_half = out->head.tiles_half;
        cd.tile_full = out->head.tiles_full;
        out->head.tiles_half += tiles_of(w / 2 > 1 ? w / 2 : 1, h / 2 > 1 ? h / 2 : 1);
        out->head.tiles_full += tiles_of(w, h);
        out->head.n_cands = n + 1;
    }
}

TRK_HD void put_scalars(const State* rs, Record* out) {
    af_runner_header& h = out->head;
    h.started = rs->started; h.consec = rs->consec; h.processed_after_start = rs->processed_after_start; h.stop = rs->stop;
    h.id_switches = rs->id_switches; h.frames_seen = rs->frames_seen;
}

TRK_HD void chunk(const af_runner_chunk& c, Scratch* sc) {
    State* rs = (State*)c.state;
    Record* out = (Record*)c.record;
    if (TRK_LANE0) {
        af_runner_header& h = out->head;
        h.overflow = h.overflow_frame = h.n_cands = h.tiles_half = h.tiles_full = h.bad = 0;
        h.n_frames = c.n_frames;
        h.reserved[0] = h.reserved[1] = h.reserved[2] = 0;
        sc->action = ACT_NEXT;
        if (rs->magic != RUN_MAGIC) { h.overflow = AF_TRACK_NOT_RESET; sc->action = ACT_END; }
        else if (rs->trk.overflowed) { h.overflow = rs->trk.overflowed; sc->action = ACT_END; }
    }
    TRK_SYNC();
    if (sc->action == ACT_END) {
        if (TRK_LANE0) {
            af_runner_header& h = out->head;
            h.started = h.consec = h.processed_after_start = h.stop = h.id_switches = h.frames_seen = 0;
        }
        return;
    }
    for (int j = 0; j < c.n_frames; ++j) {
        if (TRK_LANE0) sc->action = rs->stop ? ACT_END : before(c, j, rs, out, sc);
        TRK_SYNC();
        const int action = sc->action;
        TRK_SYNC();
        if (action == ACT_END) break;
        if (action == ACT_NEXT) continue;
        trk::Call call;
        call.state = &rs->trk;
        call.rows = c.rows + (int64_t)j * c.max_rows * c.row_stride;
        call.count_ptr = nullptr;
        call.limit = sc->n_pick;
        call.form = sc->n_pick > 0 ? trk::TRK_FORM_PICKED : AF_TRACK_FORM_EMPTY;
        call.stride = c.row_stride;
        call.start_conf = call.start_min_size = 0.f;
        call.sx = call.sy = 1.0;
        call.pick = sc->pick;
        trk::update(call, &sc->rec, &sc->trk);
        TRK_SYNC();
        if (sc->rec.overflow) {                                // the tracker refused: the walk ends at this frame
            if (TRK_LANE0) {
                out->head.overflow = sc->rec.overflow;
                out->head.overflow_frame = j;
                out->frames[j].flags |= AF_RUNNER_REFUSED;
            }
            break;
        }
        if (TRK_LANE0) after(c, j, rs, out, sc);
        TRK_SYNC();
    }
    if (TRK_LANE0) put_scalars(rs, out);
}

}  // namespace run
}  // namespace af
