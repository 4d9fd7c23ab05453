// A live tick's face stage for one call: the tracker's update and, on the tracks it returned, live.track_candidates (live.py; the
// reference's af_realtime.py:390-437), once as source for the device and the host (include/af_hip.h, "a live tick's face stage";
// DESIGN 30; the statement is live.track_candidates itself, driven by tests/live_cands_ref.py).
//
// One wave per call.  af_track_core.h's update runs unchanged and leaves its record where the caller wants it.  Then every lane
// takes one returned track - the self-view exclusion, the float32 box and the five-point pick over ALL rows of the frame
// (af_runner_core.h's pick_row) - and lane 0 walks the tracks in the tracker's order: the mesh_every cache, get_crop_box
// (af_runner_core.h's crop_box), the tile prefix of the quality launch.
// Arithmetic: fp64 under `#pragma clang fp contract(off)` of the including file, except where the host works in float32: the
// scaled-back rows, a row's x + w and y + h, the track's box as the pick and the crop box read it.
// Bounds: tracks below TRK_T, slots below TRK_S, rows below min(count, the call's limit) - the host entry checks that limit * stride
// floats are readable and stride >= 15 -, purged tids below min(n_purged, TRK_T).
#pragma once
#include "af_runner_core.h"

namespace af {
namespace live {

using trk::TRK_S;
using trk::TRK_T;
constexpr int32_t LIVE_MAGIC = 0x4556494c;                    // "LIVE", in trk::State::reserved: readable in any tracker block

struct State {
    trk::State trk;
    int32_t cache_tid[TRK_S];                                 // 0: no entry; else the track the slot's points belong to
    float cache_lm[TRK_S][10];
};
struct Job {                                                  // af_live_call behind its tracker call, as the core reads it
    double crop_scale, exclude[4];
    int32_t frame_idx, slot, mesh_every, frame_h, frame_w, n_purged;
    int32_t purged[TRK_T];
};
struct Scratch {                                              // LDS on the device
    trk::Scratch trk;
    int32_t row[TRK_T];                                       // the picked row of track i, or -1
    int32_t n_rows, n_online;
};

// column `col` of a detector row scaled back as YuNet.scale_rows does it, then cast as track_candidates casts the rows
TRK_HD float scaled(const trk::Call& c, const float* r, int col) {
    const double s = col == 14 ? 1.0 : ((col & 1) ? c.sy : c.sx);
    return (float)((double)r[col] * s);
}

TRK_HD void header(af_live_record* out, const Job& j, int overflow) {
    out->frame_idx = j.frame_idx; out->slot = j.slot;
    out->n_online = out->n_cands = out->tiles = out->bad = out->reserved = 0;
    out->overflow = overflow;
}

TRK_HD void clear(af_live_entry& e) {
    e.tid = e.flags = e.first_tile = e.cand = 0;
    for (int k = 0; k < 4; ++k) { e.tlbr[k] = 0.f; e.box[k] = 0; }
    for (int k = 0; k < 10; ++k) e.lm5[k] = 0.f;
}

TRK_HD void candidates(const trk::Call& c, const Job& j, const trk::Record* trec, af_live_record* out, Scratch* sc) {
    State* ls = (State*)c.state;
    if (TRK_LANE0) {
        header(out, j, trec->overflow);
        int n_on = trec->overflow ? 0 : trec->n_online;
        sc->n_online = n_on < 0 ? 0 : (n_on > TRK_T ? TRK_T : n_on);
        int n = 0;                                             // all rows of the frame, not only those past the start filter
        if (c.form == AF_TRACK_FORM_LIST) {
            n = c.count_ptr ? *c.count_ptr : c.limit;
            if (n > c.limit) n = c.limit;
            if (n < 0) n = 0;
        }
        sc->n_rows = n;
        if (!trec->overflow) {                                 // the tids the books purged since the last frame count as uncached
            const int np = j.n_purged < TRK_T ? j.n_purged : TRK_T;
            for (int s = 0; s < TRK_S; ++s)
                for (int p = 0; p < np; ++p)
                    if (ls->cache_tid[s] != 0 && ls->cache_tid[s] == j.purged[p]) ls->cache_tid[s] = 0;
        }
    }
    TRK_SYNC();
    const int n_on = sc->n_online, n_rows = sc->n_rows;
    TRK_FOR(i, TRK_T) {                                        // a lane per track: exclusion, float32 box, the pick
        af_live_entry& e = out->online[i];
        clear(e);
        sc->row[i] = -1;
        if (i < n_on) {
            e.cand = -1;
            const double* b = trec->online[i].tlbr;
            e.tid = trec->online[i].id;
            for (int k = 0; k < 4; ++k) e.tlbr[k] = (float)b[k];
            const double cx = 0.5 * (b[0] + b[2]), cy = 0.5 * (b[1] + b[3]);
            const double W = (double)j.frame_w, H = (double)j.frame_h;
            if (j.exclude[0] * W <= cx && cx <= j.exclude[2] * W && j.exclude[1] * H <= cy && cy <= j.exclude[3] * H) e.flags = AF_LIVE_EXCLUDED;
            else
                sc->row[i] = run::pick_row(e.tlbr, n_rows, [&c](int d, float* t) {
                    const float* r = (const float*)c.rows + (int64_t)d * c.stride;
                    const float x = scaled(c, r, 0), y = scaled(c, r, 1);
                    t[0] = x; t[1] = y; t[2] = x + scaled(c, r, 2); t[3] = y + scaled(c, r, 3);
                });
        }
    }
    TRK_SYNC();
    if (TRK_LANE0) {
        int n_cands = 0, tiles = 0;
        for (int i = 0; i < n_on; ++i) {
            af_live_entry& e = out->online[i];
            e.first_tile = tiles;                              // of every entry, so that the prefixes ascend: the quality launch bisects them
            if (e.flags & AF_LIVE_EXCLUDED) continue;
            int slot = -1;                                     // the track's slot carries its cache entry
            for (int q = 0; q < ls->trk.n_tracked && q < TRK_S && slot < 0; ++q) {
                const int s = ls->trk.tracked[q];
                if (s >= 0 && s < TRK_S && ls->trk.slot[s].id == e.tid) slot = s;
            }
            if (slot < 0) { e.flags |= AF_LIVE_NO_POINTS; continue; }      // a returned track is a tracked one: not reached
            const bool cached = ls->cache_tid[slot] == e.tid;
            if ((j.frame_idx % j.mesh_every) == 0 || !cached) {
                if (sc->row[i] < 0) { e.flags |= AF_LIVE_NO_POINTS; continue; }   // no points: skipped, the cache stays
                const float* r = (const float*)c.rows + (int64_t)sc->row[i] * c.stride;
                for (int k = 0; k < 10; ++k) ls->cache_lm[slot][k] = scaled(c, r, 5 + k);
                ls->cache_tid[slot] = e.tid;
                e.flags |= AF_LIVE_REFRESHED;
            }
            for (int k = 0; k < 10; ++k) e.lm5[k] = ls->cache_lm[slot][k];
            double b[4];
            run::widen(e.tlbr, b);
            if (!run::crop_box(b, j.crop_scale, j.frame_w, j.frame_h, e.box)) { e.flags |= AF_LIVE_EMPTY_BOX; continue; }
            const int w = e.box[2] - e.box[0], h = e.box[3] - e.box[1];
            e.flags |= AF_LIVE_CANDIDATE;
            e.cand = n_cands++;
            tiles += run::tiles_of(w / 2 > 1 ? w / 2 : 1, h / 2 > 1 ? h / 2 : 1);
        }
        out->n_online = n_on;
        out->n_cands = n_cands;
        out->tiles = tiles;
    }
    TRK_SYNC();
}

// the whole stage of one call; a block that af_live_reset did not fill is refused before anything of it is read past the tracker's
TRK_HD void update(const trk::Call& c, const Job& j, trk::Record* trec, af_live_record* out, Scratch* sc) {
    if (c.state->reserved != LIVE_MAGIC) {
        trk::refuse(c.state, trec, AF_TRACK_NOT_RESET);
        if (TRK_LANE0) header(out, j, AF_TRACK_NOT_RESET);
        TRK_FOR(i, TRK_T) clear(out->online[i]);
        return;
    }
    trk::update(c, trec, &sc->trk);
    TRK_SYNC();
    candidates(c, j, trec, out, sc);
}

}  // namespace live
}  // namespace af
